"""Batched decode on the GPU (``-m gpu``): B independent sequences, one row each, in one pass.

Kernels against the one-row kernels bit for bit; B = 1 of generate_batch against generate token for token; every row of a
batched pass against the oracle with the bounds tests/test_model_gpu.py uses per weight format; weights read once per pass
(launch counts); the models outside the batched step decline and keep the per-sequence loop."""
import pytest
import torch

from helpers import ATTN_PICK_SHAPES, ATTN_PICK_WINDOWS

pytestmark = pytest.mark.gpu

import lit_parrot_amd as L  # noqa: E402
from lit_parrot_amd import _hip, ops  # noqa: E402
from lit_parrot_amd import adapter as A  # noqa: E402
from lit_parrot_amd.config import Config, name_to_config  # noqa: E402
from lit_parrot_amd.generate import base as gb  # noqa: E402
from lit_parrot_amd.synth import is_linear_key, synthetic_prompt, synthetic_state_dict  # noqa: E402
from oracle import int4 as o4  # noqa: E402
from oracle import model as om  # noqa: E402

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
TINY = ["tiny-neox", "tiny-llama", "tiny-llama-gqa", "tiny-llama-hs128", "tiny-falcon-gqa", "tiny-falcon-mqa"]
MODEL_SEED = 4321


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    return torch.pow(2.0, torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -100))) - 7)


def k_row_for(cfg):  # tests/test_model_gpu.py, default rsqrt rounding
    if cfg.n_query_groups == 1 and cfg.n_head > 1:
        return 0
    return 1.5 if cfg._norm_class == "LayerNorm" else 3


def hip_model(cfg, sd, mode=None):
    with L.quantization(mode):
        model = L.GPT(cfg)
    model.load_state_dict(sd, strict=mode is None or mode.startswith("gptq"))
    return model.to(BF).to(DEV).eval()


def bf16_sd(cfg):
    return {k: v.to(BF) for k, v in synthetic_state_dict(cfg, MODEL_SEED, perturb=True).items()}


@pytest.fixture
def engine_off():
    gb.ENGINE_DEFAULT = False
    yield
    gb.ENGINE_DEFAULT = "auto"


@pytest.fixture
def batched_switch():
    yield ops
    ops.BATCHED_DECODE = True


# ---- 1. attention kernel
ATTN = [(4, 1, 64, 64), (2, 4, 128, 128), (1, 16, 64, 32), (2, 3, 128, 64)]  # MHA, GQA, MQA with 16 heads per group, ragged chunk


@pytest.mark.parametrize("n_groups,q_per_kv,hs,n_elem", ATTN)
@pytest.mark.parametrize("S,nsplit,mode", [(40, 1, 0), (40, 1, 1), (96, 3, 0)])
@pytest.mark.parametrize("B", [1, 2, 3, 8])
def test_attn_rows_equal_one_row_calls(n_groups, q_per_kv, hs, n_elem, S, nsplit, mode, B):
    """attn_fused_decode_rows == B attn_fused_decode calls on copies of the caches: y and every K/V slot bit for bit, positions 0,
    mid-window and past S (ring wrap), called twice (the tickets re-arm)."""
    rows_equal_one_row_calls(n_groups, q_per_kv, hs, n_elem, S, nsplit, mode, B)


@pytest.mark.parametrize("hs,q_per_kv", ATTN_PICK_SHAPES)
@pytest.mark.parametrize("S,nsplit,mode", ATTN_PICK_WINDOWS)
def test_attn_rows_equal_one_row_calls_over_the_pick_grid(hs, q_per_kv, S, nsplit, mode):
    """The same at every point of the launch's pick grid (helpers.ATTN_PICK_*), three rows: positions 0, mid-window and past S."""
    rows_equal_one_row_calls(2, q_per_kv, hs, hs, S, nsplit, mode, 3)


def rows_equal_one_row_calls(n_groups, q_per_kv, hs, n_elem, S, nsplit, mode, B):
    g = gen(31 + B)
    n_head, width = n_groups * q_per_kv, n_groups * (q_per_kv + 2) * hs
    cos, sin = (t.to(DEV) for t in om.rope_tables(1024, n_elem, BF, math_dtype=BF))
    kc = torch.randn((B, n_groups, S, hs), generator=g).to(BF).to(DEV)
    vc = torch.randn((B, n_groups, S, hs), generator=g).to(BF).to(DEV)
    kr, vr = kc.clone(), vc.clone()
    ws = ops.attn_workspace(B, n_head, hs, nsplit, DEV)
    ws1 = ops.attn_workspace(1, n_head, hs, nsplit, DEV)
    tickets = torch.zeros((B * n_head,), dtype=torch.int32, device=DEV)
    t1 = torch.zeros((n_head,), dtype=torch.int32, device=DEV)
    base = [0, S // 2, S + 3, 5, S - 1, 2 * S + 1, S, 1][:B]
    ops.ATTN_SOFTMAX_MODE = mode
    try:
        for call in range(2):
            pos = torch.tensor([p + call for p in base], dtype=torch.int32, device=DEV)
            qkv = torch.randn(B, width, generator=g).to(BF).to(DEV)
            y = torch.empty((B, n_head * hs), dtype=BF, device=DEV)
            ops.attn_fused_decode_rows(qkv, cos, sin, n_elem, pos, kc, vc, n_groups, q_per_kv, hs, S, nsplit, ws, tickets, y)
            for b in range(B):
                yb = torch.empty((1, n_head * hs), dtype=BF, device=DEV)
                ops.attn_fused_decode(qkv[b:b + 1], cos, sin, n_elem, pos[b:b + 1], kr[b], vr[b], n_groups, q_per_kv, hs, S, nsplit,
                                      ws1, t1, yb)
                assert torch.equal(y[b], yb[0]), f"row {b} (pos {int(pos[b])}) differs from the one-row kernel"
            assert torch.equal(kc, kr) and torch.equal(vc, vr), "K/V caches differ"
            assert int(tickets.abs().sum()) == 0, "arrival tickets must be re-armed"
    finally:
        ops.ATTN_SOFTMAX_MODE = 0


# ---- 2. embedding and sampling rows
def test_embedding_rows_equal_the_one_row_kernel():
    g = gen(5)
    V, d, B, Lt = 500, 128, 5, 12
    wte = torch.randn(V, d, generator=g).to(BF).to(DEV)
    tokens = torch.randint(0, V, (B, Lt), generator=g).to(DEV)
    pos = torch.tensor([0, 3, 11, 7, 3], dtype=torch.int32, device=DEV)
    out = torch.empty((B, d), dtype=BF, device=DEV)
    ops.embedding_rows(wte, tokens, pos, out)
    for b in range(B):
        ref = torch.empty((1, d), dtype=BF, device=DEV)
        ops.embedding(wte, tokens[b], pos[b:b + 1], 1, ref)
        assert torch.equal(out[b], ref[0])
    ops.embedding_rows(wte, tokens[:, :1].contiguous(), None, out)  # no positions: column 0 of every row
    assert torch.equal(out, wte[tokens[:, 0]])


@pytest.mark.parametrize("V", [500, 512, 5])
@pytest.mark.parametrize("sampler", [None, (0.8, 5), (1.0, None), (0.5, 1)])
def test_sampling_rows_equal_the_one_row_kernels(V, sampler):
    """Per row: the one-row kernel's token and advance bit for bit (ties: lowest index); frozen rows at end and after eos_id."""
    g = gen(V)
    B, Lt, eos = 6, 16, 3
    logits = (torch.randn(B, V, generator=g) * 3).to(BF)
    logits[1, V // 2] = logits[1, V // 3] = logits[1].max() + 1  # a tie: the lower index wins
    logits[2] = 0.25  # all equal
    logits = logits.to(DEV)
    noise = torch.empty((B, V), dtype=BF, device=DEV).exponential_(1)
    tokens = torch.randint(4, V if V > 4 else 5, (B, Lt), generator=g).to(DEV)
    pos = torch.tensor([0, 5, 9, 14, 7, 6], dtype=torch.int32, device=DEV)
    end = torch.tensor([16, 16, 16, 15, 16, 8], dtype=torch.int32, device=DEV)  # row 3: next position 15 = end -> frozen
    tokens[4, 7] = eos  # row 4: last token is eos -> frozen
    tokens[5, 6] = eos  # row 5: frozen only when eos_id is given (its next position 7 is still before end 8)
    for eos_id in (-1, eos):
        tok, p = tokens.clone(), pos.clone()
        if sampler is None:
            ops.argmax_advance_rows(logits, tok, p, end, eos_id)
        else:
            ops.topk_sample_rows(logits, sampler[0], sampler[1], noise, tok, p, end, eos_id)
        for b in range(B):
            p0 = int(pos[b])
            frozen = p0 + 1 >= int(end[b]) or (eos_id >= 0 and int(tokens[b, p0]) == eos_id)
            if frozen:
                assert torch.equal(tok[b], tokens[b]) and int(p[b]) == p0, f"row {b} should be frozen"
                continue
            tr, pr = tokens[b].clone(), pos[b:b + 1].clone()
            if sampler is None:
                ops.argmax_advance(logits[b], tr, pr)
            else:
                ops.topk_sample(logits[b], sampler[0], sampler[1], noise[b], tr, pr)
            assert torch.equal(tok[b], tr) and int(p[b]) == int(pr) == p0 + 1, f"row {b}"
        if sampler is None:
            assert int(tok[1, 6]) == V // 3 and int(tok[2, 10]) == 0


# ---- 3. B = 1 is generate()
@pytest.mark.parametrize("mode", [None, "gptq.int4-g128"])
def test_batch_of_one_is_generate(engine_off, mode):
    cfg = Config.from_name("tiny-llama")
    sd = bf16_sd(cfg)
    if mode is not None:
        sd = o4.quantize_state_dict(sd, 128, is_linear_key)
    model = hip_model(cfg, sd, mode)
    prompt = synthetic_prompt(cfg, 9, 2).to(DEV)
    for kw in (dict(top_k=1), dict(temperature=0.8, top_k=20), dict(temperature=1.0)):
        torch.manual_seed(11)
        a = L.generate(model, prompt, 40, 48, **kw)
        torch.manual_seed(11)
        (b,) = L.generate_batch(model, [prompt], 40, 48, **kw)
        assert torch.equal(a, b), f"{mode} {kw}: generate_batch([p]) != generate(p)"
        assert b.dtype == prompt.dtype and b.device == prompt.device
    # eos: cut before it, as generate() does
    (full,) = L.generate_batch(model, [prompt], 40, 48, top_k=1)
    eos = int(full[14])
    assert torch.equal(L.generate(model, prompt, 40, 48, top_k=1, eos_id=eos), L.generate_batch(model, [prompt], 40, 48, top_k=1, eos_id=eos)[0])


# ---- 4. rows are as accurate as one sequence
def forced_rows(model, prompts, steps, S):
    """Prefill the (B, T) prompts, then teacher-force `steps` (B, 1) tokens through GPT.forward: the logits of every step."""
    B, T = prompts.shape
    model.reset_cache()
    with torch.no_grad():
        model(prompts.to(DEV), S, torch.arange(T, device=DEV))
        out = []
        for i in range(steps.shape[1]):
            out.append(model(steps[:, i:i + 1].to(DEV), S, torch.tensor([T + i], device=DEV))[:, 0].float().cpu())
    return out


def oracle_rows(cfg, sd, linear_mode, prompts, steps, S, **kw):
    B, T = prompts.shape
    rows = []
    for b in range(B):
        o = om.OracleGPT(cfg, sd, linear_mode, **kw)
        with torch.no_grad():
            o(prompts[b:b + 1], S, torch.arange(T))
            rows.append([o(steps[b:b + 1, i:i + 1], S, torch.tensor([T + i]))[0, 0].float() for i in range(steps.shape[1])])
    return [torch.stack([rows[b][i] for b in range(B)]) for i in range(steps.shape[1])]


def forcing_inputs(cfg, B=3, T=6, n=10):
    tok = torch.stack([synthetic_prompt(cfg, T + n, 40 + b) for b in range(B)])
    return tok[:, :T], tok[:, T:]


@pytest.mark.parametrize("name", TINY)
def test_batched_forward_bf16_rows_match_the_oracle(name, batched_switch):
    """Every row of the batched pass equals the per-sequence loop bit for bit, and the oracle within the row-ulp bound of
    tests/test_model_gpu.py.  (MQA: bit-identity with the reference holds for that file's golden cases; on these prompts the
    single-sequence path itself is up to 1 row-ulp from the oracle, so MQA takes the LayerNorm families' 1.5.)"""
    cfg = Config.from_name(name)
    sd = bf16_sd(cfg)
    model = hip_model(cfg, sd)
    prompts, steps = forcing_inputs(cfg)
    S = 12  # positions reach 15: the ring wraps
    got = forced_rows(model, prompts, steps, S)
    assert model._workspaces.get((3, 3, str(DEV), "rows")) is not None, "the batched pass did not run"
    ops.BATCHED_DECODE = False
    loop = forced_rows(model, prompts, steps, S)
    assert all(torch.equal(a, b) for a, b in zip(got, loop)), "batched rows differ from the per-sequence loop"
    want = oracle_rows(cfg, sd, "dense", prompts, steps, S)
    k = k_row_for(cfg) or 1.5
    for i, (a, b) in enumerate(zip(got, want)):
        ulp_row = ulp_bf16(b.abs().amax(dim=-1, keepdim=True))
        d = (a - b).abs()
        assert not bool((d > 1e-3 + k * ulp_row).any()), f"{name} step {i}: worst {float((d / ulp_row).max()):.2f} row-ulp"


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-neox", "tiny-falcon-gqa"])
def test_batched_forward_int4_rows_match_the_oracle(name):
    cfg = Config.from_name(name)
    qsd = o4.quantize_state_dict(bf16_sd(cfg), 128, is_linear_key)
    model = hip_model(cfg, qsd, "gptq.int4-g128")
    prompts, steps = forcing_inputs(cfg, B=5)  # 5 rows: a 4-row and a 1-row GEMV pass
    got = forced_rows(model, prompts, steps, 12)
    want = oracle_rows(cfg, qsd, "gptq", prompts, steps, 12, tile_cols=128)
    for i, (a, b) in enumerate(zip(got, want)):
        assert float((a - b).abs().max()) <= 1e-2 * max(1.0, float(b.abs().max())), f"{name} step {i}"


def test_batched_forward_nf4_rows_match_the_per_sequence_loop(batched_switch):
    from lit_parrot_amd.checkpoint import stream_load

    cfg = Config(**{**name_to_config["tiny-llama-hs128"], "intermediate_size": 384})
    sd = synthetic_state_dict(cfg, seed=7, dtype=BF)
    with torch.device("cuda"), L.quantization("bnb.nf4"):
        model = L.GPT(cfg)
    model = model.to(BF).eval()
    assert stream_load(model, sd) == []
    prompts, steps = forcing_inputs(cfg, B=6)
    got = forced_rows(model, prompts, steps, 12)
    ops.BATCHED_DECODE = False
    want = forced_rows(model, prompts, steps, 12)
    for i, (a, b) in enumerate(zip(got, want)):
        assert float((a - b).abs().max()) <= 1e-2 * max(1.0, float(b.abs().max())), f"step {i}"


def greedy_agreement(hip_tokens, oracle_model, T, max_seq):  # tests/test_model_gpu.py
    exact, n = 0, len(hip_tokens) - T
    pos = torch.arange(T)
    with torch.no_grad():
        logits = oracle_model(hip_tokens[:T].view(1, -1), max_seq, pos)[0, -1].float()
        for i in range(n):
            tok = int(hip_tokens[T + i])
            top = float(logits.max())
            assert float(logits[tok]) >= top - 2 * float(ulp_bf16(torch.tensor(top))), f"token {i}: {tok} is not a (near-)argmax"
            exact += int(int(logits.argmax()) == tok)
            if i + 1 < n:
                pos = pos[-1:] + 1
                logits = oracle_model(hip_tokens[T + i].view(1, 1), max_seq, pos)[0, -1].float()
    return exact / n


@pytest.mark.parametrize("name", ["tiny-llama-gqa", "tiny-neox", "tiny-falcon-mqa"])
def test_generate_batch_greedy_rows_follow_the_oracle(engine_off, name):
    cfg = Config.from_name(name)
    sd = bf16_sd(cfg)
    model = hip_model(cfg, sd)
    prompts = [synthetic_prompt(cfg, T, 9 + T) for T in (5, 12, 9)]
    ys = L.generate_batch(model, [p.to(DEV) for p in prompts], 40, 20, top_k=1)  # window 20 < 40: every row wraps
    for p, y in zip(prompts, ys):
        y = y.cpu()
        assert y.shape == (40,) and torch.equal(y[:p.numel()], p)
        assert greedy_agreement(y, om.OracleGPT(cfg, sd), p.numel(), 20) >= 0.9
    # captured replay == eager launches
    sess = next(s for k, s in model._decode_sessions.items() if k[0] == "batch")
    assert sess.graph is not None
    model._decode_sessions.clear()
    orig = gb.BatchDecodeSession.__init__
    try:
        gb.BatchDecodeSession.__init__ = lambda self, *a, **k: orig(self, *a, **{**k, "use_graph": False})
        eager = L.generate_batch(model, [p.to(DEV) for p in prompts], 40, 20, top_k=1)
    finally:
        gb.BatchDecodeSession.__init__ = orig
    for a, b in zip(ys, eager):
        assert torch.equal(a, b), "hipGraph replay and eager launches disagree"
    # sampled rows of different lengths: replay == eager too
    torch.manual_seed(3)
    s1 = L.generate_batch(model, [p.to(DEV) for p in prompts], 30, 20, temperature=0.8, top_k=10)
    model._decode_sessions.clear()
    try:
        gb.BatchDecodeSession.__init__ = lambda self, *a, **k: orig(self, *a, **{**k, "use_graph": False})
        torch.manual_seed(3)
        s2 = L.generate_batch(model, [p.to(DEV) for p in prompts], 30, 20, temperature=0.8, top_k=10)
    finally:
        gb.BatchDecodeSession.__init__ = orig
    assert all(torch.equal(a, b) for a, b in zip(s1, s2))


def test_generate_batch_eos_cuts_each_row(engine_off):
    cfg = Config.from_name("tiny-llama")
    model = hip_model(cfg, bf16_sd(cfg))
    prompts = [synthetic_prompt(cfg, T, 60 + T).to(DEV) for T in (4, 7)]
    full = L.generate_batch(model, prompts, 30, 32, top_k=1)
    eos = int(full[0][10])
    got = L.generate_batch(model, prompts, 30, 32, top_k=1, eos_id=eos)
    for p, g_ in zip(prompts, got):
        assert torch.equal(g_, L.generate(model, p, 30, 32, top_k=1, eos_id=eos))
    assert got[0].numel() <= 10 and eos not in got[0][4:].tolist()


# ---- 5. weights are read once per pass
def _count(prof, pred):
    return sum(n for k, (_, n) in prof.items() if pred(k))


@pytest.mark.parametrize("mode,per", [(None, 2), ("gptq.int4-g128", 4), ("bnb.nf4", 4)])
@pytest.mark.parametrize("B", [2, 5, 8])
def test_one_batched_step_reads_the_weights_once_per_pass(engine_off, mode, per, B):
    cfg = Config(**{**name_to_config["tiny-llama-hs128"], "intermediate_size": 384})
    sd = bf16_sd(cfg)
    if mode == "gptq.int4-g128":
        sd = o4.quantize_state_dict(sd, 128, is_linear_key)
    if mode == "bnb.nf4":
        from lit_parrot_amd.checkpoint import stream_load

        with torch.device("cuda"), L.quantization(mode):
            model = L.GPT(cfg)
        model = model.to(BF).eval()
        assert stream_load(model, sd) == []
    else:
        model = hip_model(cfg, sd, mode)
    prompts = [synthetic_prompt(cfg, 6, b).to(DEV) for b in range(B)]
    one = gb.DecodeSession(model, 32, 16, True, use_graph=False, engine=False)
    one.prefill(prompts[0])
    _hip.prof_begin()
    one.step()
    p1 = _hip.prof_end()
    sess = gb.BatchDecodeSession(model, B, 32, 16, True, use_graph=False)
    sess.prefill(prompts, 16)
    _hip.prof_begin()
    sess.step()
    pb = _hip.prof_end()
    gemv = lambda k: k.endswith("gemv") or k.endswith("gemv_dual")  # noqa: E731
    assert _count(p1, gemv) > 0
    assert _count(pb, gemv) == -(-B // per) * _count(p1, gemv), (p1, pb)
    assert _count(pb, lambda k: k == "embedding_rows") == 1
    assert _count(pb, lambda k: k == "attn_fused_decode_rows") == cfg.n_layer
    assert _count(pb, lambda k: k == "argmax_advance_rows") == 1
    assert _count(pb, lambda k: k in ("embedding", "attn_fused_decode", "argmax_advance", "rope_kvappend", "attn_decode")) == 0


# ---- 6. declines and switching
def _declined_models():
    cfg = Config.from_name("tiny-llama")
    sd = bf16_sd(cfg)
    yield "LLM.int8", hip_model(cfg, dict(sd), "bnb.int8")
    acfg = A.Config.from_name("tiny-llama", adapter_start_layer=1)
    am = A.GPT(acfg)
    am.load_state_dict(sd, strict=False)
    yield "adapter", am.to(BF).to(DEV).eval()
    wide = Config(**{**name_to_config["tiny-falcon-7b"], "name": "tiny-falcon-7b-wide", "n_head": 18, "n_embd": 18 * 32})
    yield "query heads", hip_model(wide, bf16_sd(wide))


def test_models_outside_the_batched_step_decline_and_keep_the_loop(batched_switch):
    for why, model in _declined_models():
        cfg = model.config
        prompts = [synthetic_prompt(cfg, 5, b).to(DEV) for b in range(3)]
        with pytest.raises(L.ParrotHipError, match=why):
            L.generate_batch(model, prompts, 12, 16, top_k=1)
        p, s = forcing_inputs(cfg, B=3, T=5, n=3)
        a = forced_rows(model, p, s, 16)
        ops.BATCHED_DECODE = False
        b = forced_rows(model, p, s, 16)
        ops.BATCHED_DECODE = True
        assert all(torch.equal(x, y) for x, y in zip(a, b)), why


def test_switching_between_generate_and_generate_batch(engine_off):
    cfg = Config.from_name("tiny-llama-gqa")
    sd = bf16_sd(cfg)
    prompts = [synthetic_prompt(cfg, T, 70 + T).to(DEV) for T in (6, 9)]

    def fresh():
        return hip_model(cfg, sd)

    want_one = L.generate(fresh(), prompts[0], 30, 32, top_k=1)
    want_batch = L.generate_batch(fresh(), prompts, 30, 32, top_k=1)
    model = fresh()
    assert torch.equal(L.generate(model, prompts[0], 30, 32, top_k=1), want_one)
    got = L.generate_batch(model, prompts, 30, 32, top_k=1)
    assert all(torch.equal(a, b) for a, b in zip(got, want_batch))
    assert model.kv_caches[0][0].shape[0] == 2
    assert torch.equal(L.generate(model, prompts[0], 30, 32, top_k=1), want_one)
    assert model.kv_caches[0][0].shape[0] == 1
    got = L.generate_batch(model, prompts, 30, 32, top_k=1)
    assert all(torch.equal(a, b) for a, b in zip(got, want_batch))
    assert len(model._decode_sessions) <= gb.MAX_SESSIONS_PER_MODEL
