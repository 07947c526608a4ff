"""Prompt-lookup speculative decoding on the GPU (``-m gpu``).

The drafting and the verification kernel against their plain-Python restatement (tests/test_speculative_host.py); the consecutive-
rows attention against M sequential one-row calls bit for bit; the logits of the M-row verification pass against M one-row steps
bit for bit; generate_speculative token for token against generate(top_k=1) - the judge is the existing function, engine off -
and its step accounting against the simulated loop."""
import numpy as np
import pytest
import torch

from helpers import ATTN_PICK_SHAPES, ATTN_PICK_WINDOWS

pytestmark = pytest.mark.gpu

import lit_parrot_amd as L  # noqa: E402
from lit_parrot_amd import ops  # noqa: E402
from lit_parrot_amd.config import Config, name_to_config  # noqa: E402
from lit_parrot_amd.generate import base as gb  # noqa: E402
from lit_parrot_amd.synth import is_linear_key, synthetic_prompt, synthetic_state_dict  # noqa: E402
from oracle import int4 as o4  # noqa: E402
from oracle import model as om  # noqa: E402
from test_speculative_host import draft_rule, simulate, verify_rule  # noqa: E402

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
TINY = ["tiny-neox", "tiny-llama", "tiny-llama-gqa", "tiny-llama-hs128", "tiny-falcon-gqa", "tiny-falcon-mqa"]
QUANT = ["tiny-llama", "tiny-neox", "tiny-falcon-gqa"]
MODEL_SEED = 4321


def gen(seed):
    return torch.Generator().manual_seed(seed)


def tiny_cfg(name, mode=None):
    if name == "tiny-neox-wide-vocab":  # lm_head is a one-row launch of 8 rows per wave (N x slabs > 16 K): the packed lane sum
        return Config(**{**name_to_config["tiny-neox"], "name": name, "vocab_size": 16500, "padded_vocab_size": 16512})
    if mode == "bnb.nf4" and name == "tiny-llama":  # Linear4bit needs every in_features to be a multiple of 64 (352 is not)
        return Config(**{**name_to_config[name], "intermediate_size": 384})
    return Config.from_name(name)


def build_model(name, mode=None, seed=MODEL_SEED):
    cfg = tiny_cfg(name, mode)
    sd = {k: v.to(BF) for k, v in synthetic_state_dict(cfg, seed, perturb=True).items()}
    if mode == "bnb.nf4":
        from lit_parrot_amd.checkpoint import stream_load

        with torch.device("cuda"), L.quantization(mode):
            model = L.GPT(cfg)
        model = model.to(BF).eval()
        assert stream_load(model, sd) == []
        return cfg, model
    if mode is not None:
        sd = o4.quantize_state_dict(sd, 128, is_linear_key)
    with L.quantization(mode):
        model = L.GPT(cfg)
    model.load_state_dict(sd, strict=True)
    return cfg, model.to(BF).to(DEV).eval()


@pytest.fixture
def engine_off():
    gb.ENGINE_DEFAULT = False
    yield
    gb.ENGINE_DEFAULT = "auto"


def state_buf():
    return torch.zeros((ops.SPEC_STATE_WORDS,), dtype=torch.int32, device=DEV)


def i32(*v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


# ---- 1. the drafting kernel
def run_draft(tokens, pos, K, nmax=3, nmin=1):
    buf = torch.tensor(tokens, dtype=torch.int64, device=DEV)
    st = state_buf()
    ops.ngram_draft(buf, i32(pos), K, nmax, nmin, st)
    return buf.cpu().tolist(), st.cpu().tolist()


def check_draft(tokens, pos, K, nmax=3, nmin=1):
    tokens = [int(t) for t in tokens]
    got, st = run_draft(tokens, pos, K, nmax, nmin)
    drafts, matched = draft_rule(tokens, pos, K, nmax, nmin)
    want = list(tokens)
    for i, d in enumerate(drafts):
        if pos + 1 + i < len(want):
            want[pos + 1 + i] = d
    assert got == want, f"pos {pos} K {K} n {nmax}..{nmin}: drafts {got[pos + 1:pos + 1 + K]}, the rule gives {drafts}"
    assert st[ops.SPEC_MATCHED] == matched and st[ops.SPEC_POS] == pos and st[ops.SPEC_LAST] == tokens[pos]
    return matched


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7])
def test_ngram_draft_follows_the_rule(K):
    g = gen(100 + K)
    hits = 0
    # random buffers over a small alphabet (many repeats of every length), drafts written over whatever lies behind pos
    for L_, vocab in ((40, 3), (300, 6), (700, 40), (2500, 12)):
        tokens = torch.randint(0, vocab, (L_,), generator=g).tolist()
        for pos in sorted({0, 1, 2, 3, L_ // 3, L_ // 2, L_ - K - 2, L_ - K - 1, L_ - 2, L_ - 1}):  # the last ones: drafts past the buffer are dropped
            for nmax, nmin in ((3, 1), (5, 2), (1, 1), (16, 16)):
                hits += check_draft(tokens, pos, K, nmax, nmin) > 0
    assert hits > 20
    # planted repeats in a buffer of distinct tokens: the LATEST earlier occurrence wins, whatever thread finds it
    base = list(range(1000, 1600))
    gram = [7, 8, 9]
    for starts in ([10], [10, 200], [10, 200, 590], [300, 301 + 256], [0, 256, 512]):
        t = list(base)
        for s in starts:
            t[s:s + 3] = gram
            t[s + 3] = 5000 + s  # what followed this occurrence
        pos = 598
        t[pos - 2:pos + 1] = gram
        drafts, matched = draft_rule(t, pos, K)
        latest = max(starts)
        assert drafts[0] == 5000 + latest and matched == min(K, pos - (latest + 3) + 1)
        assert check_draft(t, pos, K) == matched
    # no match at all, and pos smaller than every n
    check_draft(base, 300, K)
    assert check_draft([3, 3, 9, 9], 0, K, 3, 2) == 0 and check_draft([3, 3, 9, 9], 1, K, 3, 3) == 0
    # a continuation that runs into pos: tokens ... a b X | a b  -> X a b, then padding with tokens[pos]
    t = list(base[:50]) + [1, 2, 77, 1, 2] + [0] * 8
    assert check_draft(t, 54, K) == min(K, 3)
    # a cycle of period 1: the continuation is one token long
    assert check_draft([4] * 20 + [0] * 8, 19, K) == 1


# ---- 2. the verification kernel
def logits_with_argmax(arg, V, g):
    lg = (torch.randn(len(arg), V, generator=g) * 2).to(BF)
    for m, a in enumerate(arg):
        lg[m, a] = lg[m].max() + 1
    return lg


def check_verify(arg, tokens, pos, end, eos_id=-1, V=520, logits=None, g=None):
    M = len(arg)
    lg = (logits if logits is not None else logits_with_argmax(arg, V, g or gen(3))).to(DEV)
    tok = torch.tensor(tokens, dtype=torch.int64, device=DEV)
    p, st, rp = i32(pos), state_buf(), torch.full((M,), -1, dtype=torch.int32, device=DEV)
    st[ops.SPEC_ACCEPTED], st[ops.SPEC_STEPS] = 10, 20
    ops.verify_advance(lg, tok, p, i32(end), eos_id, st, rp)
    want = [int(t) for t in tokens]
    p_new, c = verify_rule(list(arg), want, pos, end, eos_id)
    assert tok.cpu().tolist() == want and int(p) == p_new, f"arg {arg} pos {pos} end {end} eos {eos_id}: pos {int(p)} want {p_new}"
    st = st.cpu().tolist()
    assert (st[ops.SPEC_ACCEPTED], st[ops.SPEC_STEPS]) == ((10, 20) if c is None else (10 + c, 21))
    assert rp.cpu().tolist() == [p_new + m for m in range(M)], "row_pos: the positions of the next step's rows"
    return c


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("V", [520, 517, 5])
def test_verify_advance_follows_the_rule(K, V):
    g = gen(K * 10 + V)
    M, Lt, pos = K + 1, 40, 9
    base = torch.randint(0, min(V, 400), (Lt,), generator=g).tolist()
    truth = [(7 * m + 1) % V for m in range(M)]  # the rows' arg-max tokens (V = 5: with repeats)
    for c_want in range(K + 1):  # every accepted count: drafts 0 .. c-1 right, draft c wrong
        t = list(base)
        t[pos + 1:pos + 1 + K] = truth[:K]
        if c_want < K:
            t[pos + 1 + c_want] = (truth[c_want] + 1) % V
        assert check_verify(truth, t, pos, Lt, V=V, g=g) == c_want
    t = list(base)
    t[pos + 1:pos + 1 + K] = truth[:K]
    # the end cut: no token at or past `end`, for every end around the rows
    for end in range(pos, pos + M + 3):
        c = check_verify(truth, t, pos, end, V=V, g=g)
        assert c == (None if pos + 1 >= end else min(K, end - pos - 2))
    # the buffer itself is an end: L = pos + 3 leaves room for one accepted draft
    assert check_verify(truth, t[:pos + 3], pos, 10 ** 6, V=V, g=g) == min(K, 1)
    # the eos cut: eos at row e is written and ends the step; the next call is frozen
    for e in range(M):
        eos, first = truth[e], truth.index(truth[e])  # cut at the FIRST row that produces it
        t2 = list(t)
        t2[pos] = (eos + 1) % V  # (the token at pos is not eos: the sequence is live)
        assert check_verify(truth, t2, pos, Lt, eos_id=eos, V=V, g=g) == first
        t2[pos + 1 + first] = eos
        assert check_verify(truth, t2, pos + 1 + first, Lt, eos_id=eos, V=V, g=g) is None
    if V > 5:  # an eos nobody produces changes nothing
        t2 = list(t)
        t2[pos] = 2
        assert check_verify(truth, t2, pos, Lt, eos_id=4, V=V, g=g) == K


def test_verify_advance_ties_and_argmax_advance_agree():
    """A planted tie takes the lowest index, and with all drafts right the result is M consecutive argmax_advance calls."""
    g = gen(8)
    V, M, Lt, pos = 1000, 5, 32, 6
    lg = (torch.randn(M, V, generator=g) * 2).to(BF)
    top = lg.max() + 2
    lg[1, 900] = lg[1, 33] = lg[1, 500] = top  # row 1: three equal maxima -> 33
    lg[3] = 0.5                                # row 3: all equal -> 0
    lg = lg.to(DEV)
    tok = torch.randint(0, V, (Lt,), generator=g).to(DEV)
    ref, p_ref = tok.clone(), i32(pos)
    for m in range(M):
        ops.argmax_advance(lg[m], ref, p_ref)
    assert int(ref[pos + 2]) == 33 and int(ref[pos + 4]) == 0
    drafts = tok.clone()
    drafts[pos + 1:pos + M] = ref[pos + 1:pos + M]  # all four drafts right
    p, st = i32(pos), state_buf()
    ops.verify_advance(lg, drafts, p, i32(Lt), -1, st)
    assert torch.equal(drafts, ref) and int(p) == int(p_ref) == pos + M
    assert st.cpu().tolist()[ops.SPEC_ACCEPTED] == M - 1
    wrong = tok.clone()
    wrong[pos + 1] = ref[pos + 1]
    wrong[pos + 2] = 500  # the tie's other index is NOT the arg-max
    p = i32(pos)
    ops.verify_advance(lg, wrong, p, i32(Lt), -1, state_buf())
    assert int(p) == pos + 2 and int(wrong[pos + 2]) == 33


# ---- 3. the consecutive-rows attention
ATTN = [(4, 1, 64, 64), (2, 4, 128, 128), (1, 16, 64, 32), (2, 3, 128, 64)]  # the shapes of test_attn_rows_equal_one_row_calls


@pytest.mark.parametrize("n_groups,q_per_kv,hs,n_elem", ATTN)
@pytest.mark.parametrize("S,nsplit,mode", [(40, 1, 0), (40, 1, 1), (96, 3, 0)])
@pytest.mark.parametrize("M", [2, 4, 8])
def test_attn_seq_equals_sequential_one_row_calls(n_groups, q_per_kv, hs, n_elem, S, nsplit, mode, M):
    """rope_kvappend + attn_fused_decode_seq over M rows == M attn_fused_decode calls on copies of the caches: y and every K/V
    slot bit for bit, at position 0, mid-window and up to the last slot, called twice (the tickets re-arm)."""
    seq_equals_sequential_one_row_calls(n_groups, q_per_kv, hs, n_elem, S, nsplit, mode, M)


@pytest.mark.parametrize("hs,q_per_kv", ATTN_PICK_SHAPES)
@pytest.mark.parametrize("S,nsplit,mode", ATTN_PICK_WINDOWS)
def test_attn_seq_equals_sequential_one_row_calls_over_the_pick_grid(hs, q_per_kv, S, nsplit, mode):
    """The same at every point of the launch's pick grid (helpers.ATTN_PICK_*), three rows."""
    seq_equals_sequential_one_row_calls(2, q_per_kv, hs, hs, S, nsplit, mode, 3)


def seq_equals_sequential_one_row_calls(n_groups, q_per_kv, hs, n_elem, S, nsplit, mode, M):
    g = gen(77 + M)
    n_head, width = n_groups * q_per_kv, n_groups * (q_per_kv + 2) * hs
    cos, sin = (t.to(DEV) for t in om.rope_tables(1024, n_elem, BF, math_dtype=BF))
    ws = ops.attn_workspace(M, n_head, hs, nsplit, DEV)
    ws1 = ops.attn_workspace(1, n_head, hs, nsplit, DEV)
    tickets = torch.zeros((M * n_head,), dtype=torch.int32, device=DEV)
    t1 = torch.zeros((n_head,), dtype=torch.int32, device=DEV)
    q_scratch = torch.empty((M, n_head * hs), dtype=BF, device=DEV)
    ops.ATTN_SOFTMAX_MODE = mode
    try:
        for p0 in (0, S // 2 - 1, S - M):
            kc = torch.randn((n_groups, S, hs), generator=g).to(BF).to(DEV)
            vc = torch.randn((n_groups, S, hs), generator=g).to(BF).to(DEV)
            kr, vr = kc.clone(), vc.clone()
            for call in range(2):
                pos = i32(p0 if call == 0 else max(p0 - 1, 0))
                qkv = torch.randn(M, width, generator=g).to(BF).to(DEV)
                y = torch.empty((M, n_head * hs), dtype=BF, device=DEV)
                ops.rope_kvappend(qkv, cos, sin, n_elem, pos, n_groups, q_per_kv, hs, S, q_scratch, kc, vc)
                ops.attn_fused_decode_seq(qkv, cos, sin, n_elem, pos, kc, vc, n_groups, q_per_kv, hs, S, nsplit, ws, tickets, y)
                for m in range(M):
                    ym = torch.empty((1, n_head * hs), dtype=BF, device=DEV)
                    ops.attn_fused_decode(qkv[m:m + 1], cos, sin, n_elem, pos + m, kr, vr, n_groups, q_per_kv, hs, S, nsplit, ws1, t1, ym)
                    assert torch.equal(y[m], ym[0]), f"row {m} (pos {int(pos) + m}) differs from the one-row kernel"
                assert torch.equal(kc, kr) and torch.equal(vc, vr), "K/V caches differ"
                assert int(tickets.abs().sum()) == 0, "arrival tickets must be re-armed"
    finally:
        ops.ATTN_SOFTMAX_MODE = 0


# ---- 4. the M-row verification pass == M one-row steps
def rows_vs_one_row_steps(model, cfg, K, T=9, S=32):
    M = K + 1
    toks = synthetic_prompt(cfg, T + M, 5).to(DEV)
    one = gb.DecodeSession(model, S, S, greedy=False, use_graph=False, engine=False)  # the step ends at the logits
    one.tokens[:T + M].copy_(toks)
    one.prefill(toks[:T])
    want = []
    for m in range(M):
        one.pos.fill_(T - 1 + m)
        want.append(one.step().clone())
    k_want = [(k.clone(), v.clone()) for k, v in one.caches]
    spec = gb.SpeculativeSession(model, S, S, draft_len=K, use_graph=False)
    assert spec.caches[0][0].data_ptr() == one.caches[0][0].data_ptr()
    for k, v in spec.caches:
        k.zero_(), v.zero_()
    spec.prefill(toks[:T], S)
    spec.tokens[:T + M].copy_(toks)
    got = model.run_rows(spec.ws_rows, spec.tokens, spec.pos, spec.pos, S, spec.caches, model.rope_cache)
    assert got.shape == (M, cfg.padded_vocab_size)
    for m in range(M):
        assert torch.equal(got[m], want[m]), f"row {m}: max |diff| {float((got[m].float() - want[m].float()).abs().max())}"
    for i, ((k, v), (k0, v0)) in enumerate(zip(spec.caches, k_want)):
        for what, a, b in (("K", k, k0), ("V", v, v0)):
            bad = (a[:, :T + M - 1].view(torch.int16) != b[:, :T + M - 1].view(torch.int16)).any(-1).nonzero().tolist()
            assert not bad, f"layer {i} {what} cache: (group, slot) {bad} differ from the one-row steps' (prompt slots 0..{T - 1})"


@pytest.mark.parametrize("name", TINY)
@pytest.mark.parametrize("K", [1, 3, 7])
def test_verification_rows_bf16_equal_one_row_steps(name, K):
    cfg, model = build_model(name)
    rows_vs_one_row_steps(model, cfg, K)


@pytest.mark.parametrize("mode", ["gptq.int4-g128", "bnb.nf4"])
@pytest.mark.parametrize("name", QUANT)
@pytest.mark.parametrize("K", [1, 4, 7])
def test_verification_rows_4bit_equal_one_row_steps(name, mode, K):
    cfg, model = build_model(name, mode)
    rows_vs_one_row_steps(model, cfg, K)


@pytest.mark.parametrize("mode", ["gptq.int4-g128", "bnb.nf4"])
@pytest.mark.parametrize("K", [1, 2, 5])
def test_verification_rows_4bit_equal_one_row_steps_where_the_one_row_gemv_packs_its_sums(mode, K):
    """The one-row int4 / NF4 GEMV adds a row's 64 lane partials in a different order when it takes 8 rows per wave (SwiGLU pairs,
    N x slabs > 16 K); the multi-row launches of the same Linear follow that order, or these rows would differ in the last bit."""
    cfg, model = build_model("tiny-neox-wide-vocab", mode)
    rows_vs_one_row_steps(model, cfg, K)
    cfg, model = build_model("tiny-llama-gqa", "gptq.int4-g128")
    rows_vs_one_row_steps(model, cfg, K)


# ---- 5. end to end: generate_speculative == generate(top_k=1)
def eager(model, fn):
    """Run fn with SpeculativeSession(use_graph=False): eager launches instead of the captured steps."""
    orig = gb.SpeculativeSession.__init__
    model.__dict__.pop("_decode_sessions", None)
    try:
        gb.SpeculativeSession.__init__ = lambda self, *a, **k: orig(self, *a, **{**k, "use_graph": False})
        return fn()
    finally:
        gb.SpeculativeSession.__init__ = orig
        model.__dict__.pop("_decode_sessions", None)


def looping_prompt(cfg, T, seed):
    """A prompt that repeats a span of itself, as the prompts this feature is for do (the lookup has something to find)."""
    p = synthetic_prompt(cfg, T, seed)
    p[T // 2:T // 2 + T // 4] = p[:T // 4]
    return p


@pytest.mark.parametrize("mode", [None, "gptq.int4-g128"])
@pytest.mark.parametrize("name", TINY)
def test_generate_speculative_equals_generate(engine_off, name, mode):
    cfg, model = build_model(name, mode)
    N, S = 72, 80
    total_accepted = 0
    for T, seed in ((12, 3), (5, 8)):
        prompt = looping_prompt(cfg, T, seed).to(DEV)
        want = L.generate(model, prompt, N, S, top_k=1)
        eos = int(want[T + 9])
        want_eos = L.generate(model, prompt, N, S, top_k=1, eos_id=eos)
        for K in (1, 3, 7):
            got, stats = L.generate_speculative(model, prompt, N, S, draft_len=K, return_stats=True)
            assert torch.equal(got, want), f"{name} {mode} K={K}: tokens differ from generate(top_k=1)"
            assert got.dtype == prompt.dtype and got.device == prompt.device
            sim, n = simulate(want.tolist(), T, N, K)
            assert stats == sim and n == N, f"K={K}: {stats}, simulated {sim}"
            total_accepted += stats["accepted"]
            assert torch.equal(eager(model, lambda: L.generate_speculative(model, prompt, N, S, draft_len=K)), want), f"eager K={K}"
            got_eos, stats_eos = L.generate_speculative(model, prompt, N, S, draft_len=K, eos_id=eos, return_stats=True)
            assert torch.equal(got_eos, want_eos) and got_eos.numel() <= T + 9
            sim_eos, n_eos = simulate(want.tolist(), T, N, K, eos_id=eos)
            assert stats_eos == sim_eos and n_eos == got_eos.numel()
    assert total_accepted >= 1, "no draft was ever accepted: the M-row step went untested"


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-falcon-mqa"])
def test_generate_speculative_up_to_block_size(engine_off, name):
    """max_returned_tokens == block_size: the last rows sit on the last RoPE row and cache slot; eos as the first token."""
    cfg, model = build_model(name)
    B = cfg.block_size
    prompt = looping_prompt(cfg, 20, 4).to(DEV)
    want = L.generate(model, prompt, B, B, top_k=1)
    for K in (1, 3, 7):
        got, stats = L.generate_speculative(model, prompt, B, B, draft_len=K, return_stats=True)
        assert torch.equal(got, want)
        assert stats == simulate(want.tolist(), 20, B, K)[0]
    first = int(want[20])
    assert torch.equal(L.generate_speculative(model, prompt, B, B, eos_id=first), L.generate(model, prompt, B, B, top_k=1, eos_id=first))
    # a prompt that ends within M of the limit: only one-row steps
    got, stats = L.generate_speculative(model, want[:B - 3], B, B, draft_len=7, return_stats=True)
    assert torch.equal(got, L.generate(model, want[:B - 3], B, B, top_k=1)) and stats == {"steps": 2, "accepted": 0, "matched_steps": 0}


def pythia():
    cfg = Config.from_name("pythia-160m")
    sd = {k: v.to(BF) for k, v in synthetic_state_dict(cfg, 1234).items()}
    model = L.GPT(cfg)
    model.load_state_dict(sd, strict=True)
    return cfg, model.to(BF).to(DEV).eval()


def test_pythia160m_golden_prompt(engine_off, golden_dir):
    """The Pythia-160M golden prompt for 64 tokens: generate()'s tokens, the simulated loop's steps, and at least one accepted
    draft (the reference's own run of this prompt accepts 22 of 63 with one draft)."""
    g = np.load(golden_dir / "generate_bf16.npz")
    cfg, model = pythia()
    prompt = torch.from_numpy(g["prompt"]).to(DEV)
    T, N = 128, 192
    want = L.generate(model, prompt, N, N, top_k=1)
    for K in (1, 3, 7):
        got, stats = L.generate_speculative(model, prompt, N, N, draft_len=K, return_stats=True)
        assert torch.equal(got, want), f"K={K}"
        sim, _ = simulate(want.tolist(), T, N, K)
        print(f"pythia-160m K={K}: {stats} (simulated {sim})")
        assert stats == sim
        assert stats["accepted"] >= 1
        assert stats["steps"] + stats["accepted"] == N - T - 1


# ---- 6. step accounting with the draft hook
def test_hook_fed_the_true_continuation_and_wrong_tokens(engine_off):
    cfg, model = build_model("tiny-llama-gqa")
    T = 10
    prompt = synthetic_prompt(cfg, T, 12).to(DEV)
    for K, N in ((1, 41), (3, 51), (7, 75), (3, 40), (7, 60)):
        M = K + 1
        want = L.generate(model, prompt, N, 80, top_k=1)
        truth = torch.cat([want, want.new_zeros(M)])

        def right(sess):
            p = int(sess.pos)
            sess.tokens[p + 1:p + 1 + K].copy_(truth[p + 1:p + 1 + K][: sess.tokens.numel() - p - 1])
            return K

        got, stats = L.generate_speculative(model, prompt, N, 80, draft_len=K, return_stats=True, draft_hook=right)
        assert torch.equal(got, want)
        n = N - T - 1  # tokens after the first, which is sampled from the prompt's logits without a step
        assert stats["steps"] == -(-n // M) and stats["steps"] + stats["accepted"] == n, (K, N, stats)
        sim, _ = simulate(want.tolist(), T, N, K, drafter=lambda known, p: (truth[p + 1:p + 1 + K].tolist(), K))
        assert stats == sim

        def wrong(sess):
            p = int(sess.pos)
            k = min(K, sess.tokens.numel() - p - 1)
            sess.tokens[p + 1:p + 1 + k].copy_((truth[p + 1:p + 1 + k] + 1) % cfg.padded_vocab_size)
            return K

        got, stats = L.generate_speculative(model, prompt, N, 80, draft_len=K, return_stats=True, draft_hook=wrong)
        assert torch.equal(got, want) and stats["accepted"] == 0 and stats["steps"] == n
        assert eager(model, lambda: torch.equal(L.generate_speculative(model, prompt, N, 80, draft_len=K, draft_hook=right), want))


# ---- 7. switching
def test_switching_between_generate_and_generate_speculative(engine_off):
    prompt = None
    outs = []
    for order in (("g",), ("s",), ("g", "s", "g", "s")):
        cfg, model = build_model("tiny-llama")
        prompt = looping_prompt(cfg, 12, 3).to(DEV)
        for what in order:
            if what == "g":
                outs.append(L.generate(model, prompt, 60, 64, top_k=1))
            else:
                outs.append(L.generate_speculative(model, prompt, 60, 64, draft_len=3))
    assert all(torch.equal(o, outs[0]) for o in outs)
    assert len(model._decode_sessions) == 2
