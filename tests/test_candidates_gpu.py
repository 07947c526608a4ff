"""Candidates of one prompt on the GPU (``-m gpu``): n rows on one shared prompt cache.

The attention kernel against the batched kernel bit for bit (both kinds of workgroup, both settings of the switch); the tokens of
generate_candidates against generate_batch([p] * n) under the same seed and, greedy, against generate(); one captured step for
prompts of any length whose tail fits; the prompt prefilled and stored once (launch counts, sentinel slots)."""
import pytest
import torch

from helpers import ATTN_PICK_SHAPES, ATTN_PICK_WINDOWS

pytestmark = pytest.mark.gpu

import lit_parrot_amd as L  # noqa: E402
from lit_parrot_amd import _hip, ops  # noqa: E402
from lit_parrot_amd.config import Config, name_to_config  # noqa: E402
from lit_parrot_amd.generate import base as gb  # noqa: E402
from lit_parrot_amd.synth import is_linear_key, synthetic_prompt, synthetic_state_dict  # noqa: E402
from oracle import int4 as o4  # noqa: E402
from oracle import model as om  # noqa: E402

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
MODEL_SEED = 4321
S_GEN, RETURNED = 96, 90  # with ATTN_SPLIT_KEYS = 32: three splits of 32 slots
SEED = 11                 # (1.0, None), n = 8: the rows differ under this seed (asserted below)


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture
def engine_off():
    gb.ENGINE_DEFAULT = False
    yield
    gb.ENGINE_DEFAULT = "auto"


@pytest.fixture
def split_keys_32():
    ops.ATTN_SPLIT_KEYS = 32
    yield
    ops.ATTN_SPLIT_KEYS = 1024


@pytest.fixture
def share_switch():
    default = ops.CANDIDATES_SHARE_LOADS
    yield ops
    ops.CANDIDATES_SHARE_LOADS = default


# ---- 1. the kernel against the rows kernel
ATTN = [(4, 1, 64, 64), (2, 2, 32, 32), (2, 4, 128, 128), (2, 3, 128, 64), (1, 16, 64, 32)]  # MHA, 2 per group, GQA, ragged chunk, MQA
# (320, 2): per = 160 keys takes the 16-wave variant at every head size.  T: around the split borders, T = 1 and T = S - 1
WINDOWS = [(40, 1, 0, (1, 20, 39)), (40, 1, 1, (1, 20, 39)), (96, 3, 0, (1, 32, 33, 64, 70, 95)), (320, 2, 0, (160, 200))]


@pytest.mark.parametrize("n_groups,q_per_kv,hs,n_elem", ATTN)
@pytest.mark.parametrize("S,nsplit,mode,Ts", WINDOWS)
@pytest.mark.parametrize("B", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("share", [True, False])
def test_attn_prefix_equals_the_rows_kernel(n_groups, q_per_kv, hs, n_elem, S, nsplit, mode, Ts, B, share, share_switch):
    """attn_fused_decode_prefix == attn_fused_decode_rows on B caches cat(prefix[:, :T], tail[b][:, :S - T]): y and the appended
    row bit for bit, every other tail slot and the shared cache untouched, the tickets re-armed; called twice, the second time one
    position further.  Row positions are spread over [T, S - 1] and include pos = T."""
    prefix_equals_the_rows_kernel(n_groups, q_per_kv, hs, n_elem, S, nsplit, mode, Ts, B, share)


@pytest.mark.parametrize("hs,q_per_kv", ATTN_PICK_SHAPES)
@pytest.mark.parametrize("S,nsplit,mode", ATTN_PICK_WINDOWS)
@pytest.mark.parametrize("share", [True, False])
def test_attn_prefix_equals_the_rows_kernel_over_the_pick_grid(hs, q_per_kv, S, nsplit, mode, share, share_switch):
    """The same at every point of the launch's pick grid (helpers.ATTN_PICK_*), three rows; T = 1, the border of the two splits and
    three slots past it (with ``share`` the first split then goes to the shared-load launch)."""
    prefix_equals_the_rows_kernel(2, q_per_kv, hs, hs, S, nsplit, mode, (1, S // 2, S // 2 + 3), 3, share)


def prefix_equals_the_rows_kernel(n_groups, q_per_kv, hs, n_elem, S, nsplit, mode, Ts, B, share):
    g = gen(31 + B)
    n_head, width = n_groups * q_per_kv, n_groups * (q_per_kv + 2) * hs
    cos, sin = (t.to(DEV) for t in om.rope_tables(1024, n_elem, BF, math_dtype=BF))
    ws, ws_ref = (ops.attn_workspace(B, n_head, hs, nsplit, DEV) for _ in range(2))
    tickets, t_ref = (torch.zeros((B * n_head,), dtype=torch.int32, device=DEV) for _ in range(2))
    ops.ATTN_SOFTMAX_MODE, ops.CANDIDATES_SHARE_LOADS = mode, share
    try:
        for T in Ts:
            S_tail = S - T + 3  # (not a round number: the tail's own stride)
            prefix = [torch.randn((n_groups, S, hs), generator=g).to(BF).to(DEV) for _ in range(2)]
            tails = [torch.randn((B, n_groups, S_tail, hs), generator=g).to(BF).to(DEV) for _ in range(2)]
            ref = [torch.cat([p[:, :T].expand(B, -1, -1, -1), t[:, :, :S - T]], dim=2).contiguous() for p, t in zip(prefix, tails)]
            prefix0 = [p.clone() for p in prefix]
            plen = torch.tensor([T], dtype=torch.int32, device=DEV)
            kc, vc = (ops.PrefixCache(p, t, plen) for p, t in zip(prefix, tails))
            base = [T + (b * (S - 1 - T)) // max(B - 1, 1) for b in range(B)]  # T .. S - 1
            for call in range(2):
                pos_l = [min(p + call, S - 1) for p in base]
                pos = torch.tensor(pos_l, dtype=torch.int32, device=DEV)
                qkv = torch.randn(B, width, generator=g).to(BF).to(DEV)
                y, y_ref = (torch.empty((B, n_head * hs), dtype=BF, device=DEV) for _ in range(2))
                want_tails = [t.clone() for t in tails]
                ops.attn_fused_decode_rows(qkv, cos, sin, n_elem, pos, ref[0], ref[1], n_groups, q_per_kv, hs, S, nsplit, ws_ref, t_ref, y_ref)
                ops.attn_fused_decode_prefix(qkv, cos, sin, n_elem, pos, kc, vc, n_groups, q_per_kv, hs, S, nsplit, ws, tickets, y)
                for b in range(B):
                    assert torch.equal(y[b], y_ref[b]), f"T={T} call {call}: row {b} (pos {pos_l[b]}) differs from the rows kernel"
                    for w, r in zip(want_tails, ref):
                        w[b, :, pos_l[b] - T] = r[b, :, pos_l[b]]
                for t, w in zip(tails, want_tails):
                    assert torch.equal(t, w), f"T={T} call {call}: the appended row differs or another tail slot changed"
                assert all(torch.equal(p, p0) for p, p0 in zip(prefix, prefix0)), "the shared cache changed"
                assert int(tickets.abs().sum()) == 0, f"T={T} call {call}: arrival tickets must be re-armed"
    finally:
        ops.ATTN_SOFTMAX_MODE = 0


# ---- 2. tokens
TINY = ["tiny-llama", "tiny-llama-gqa", "tiny-neox", "tiny-llama-hs128", "tiny-falcon-gqa", "tiny-falcon-mqa"]
MODELS = [(n, None) for n in TINY] + [("tiny-llama", "gptq.int4-g128"), ("tiny-llama-hs128", "bnb.nf4")]
_models = {}


def model_pair(name, mode):
    """Two copies of one model, built once per session: the candidates (and generate()) run on the first, whose caches stay
    batch-1; generate_batch on the second, whose caches are n rows wide."""
    if (name, mode) in _models:
        return _models[(name, mode)]
    pair = []
    for _ in range(2):
        if mode == "bnb.nf4":  # as tests/test_batch_decode_gpu.py::test_batched_forward_nf4_rows_match_the_per_sequence_loop
            from lit_parrot_amd.checkpoint import stream_load

            cfg = Config(**{**name_to_config[name], "intermediate_size": 384})
            sd = synthetic_state_dict(cfg, seed=7, dtype=BF)
            with torch.device("cuda"), L.quantization(mode):
                model = L.GPT(cfg)
            model = model.to(BF).eval()
            assert stream_load(model, sd) == []
        else:
            cfg = Config.from_name(name)
            sd = {k: v.to(BF) for k, v in synthetic_state_dict(cfg, MODEL_SEED, perturb=True).items()}
            if mode is not None:
                sd = o4.quantize_state_dict(sd, 128, is_linear_key)
            with L.quantization(mode):
                model = L.GPT(cfg)
            model.load_state_dict(sd, strict=True)
            model = model.to(BF).to(DEV).eval()
        pair.append(model)
    _models[(name, mode)] = tuple(pair)
    return _models[(name, mode)]


def prompt_of(cfg, T):
    return synthetic_prompt(cfg, T, 9 + T).to(DEV)


@pytest.mark.parametrize("name,mode", MODELS)
@pytest.mark.parametrize("kw", [dict(top_k=1), dict(temperature=0.8, top_k=20), dict(temperature=1.0)], ids=["greedy", "t0.8-k20", "t1.0"])
@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("share", [True, False])
def test_candidates_are_the_rows_of_generate_batch(engine_off, split_keys_32, share_switch, name, mode, kw, n, share):
    """T = 70: two shared splits and one mixed; T = 20: no shared split.  Under both settings of the switch."""
    cand, batch = model_pair(name, mode)
    ops.CANDIDATES_SHARE_LOADS = share
    for T in (70, 20):
        p = prompt_of(cand.config, T)
        torch.manual_seed(SEED)
        got = L.generate_candidates(cand, p, n, RETURNED, S_GEN, **kw)
        torch.manual_seed(SEED)
        want = L.generate_batch(batch, [p] * n, RETURNED, S_GEN, **kw)
        assert len(got) == n
        for b, (a, w) in enumerate(zip(got, want)):
            assert torch.equal(a, w), f"{name} {mode} {kw} n={n} T={T}: row {b} differs from generate_batch"
            assert a.dtype == p.dtype and a.device == p.device and a.numel() == RETURNED
        if "top_k" in kw and kw["top_k"] == 1:
            one = L.generate(cand, p, RETURNED, S_GEN, top_k=1)
            assert all(torch.equal(a, one) for a in got), "greedy rows differ from generate()"
        if kw == dict(temperature=1.0) and n == 8:
            assert any(not torch.equal(got[0], a) for a in got[1:]), "the sampled rows are all equal: nothing exercised rows at different states"


@pytest.mark.parametrize("name,mode", [("tiny-llama", None), ("tiny-falcon-gqa", None)])
def test_eos_cuts_each_candidate_as_generate_batch_does(engine_off, split_keys_32, name, mode):
    cand, batch = model_pair(name, mode)
    p = prompt_of(cand.config, 70)
    full = L.generate_candidates(cand, p, 3, RETURNED, S_GEN, top_k=1)
    eos = int(full[0][80])
    for kw in (dict(top_k=1), dict(temperature=1.0)):
        torch.manual_seed(SEED)
        got = L.generate_candidates(cand, p, 3, RETURNED, S_GEN, eos_id=eos, **kw)
        torch.manual_seed(SEED)
        want = L.generate_batch(batch, [p] * 3, RETURNED, S_GEN, eos_id=eos, **kw)
        assert all(torch.equal(a, w) for a, w in zip(got, want)), kw
    got = L.generate_candidates(cand, p, 3, RETURNED, S_GEN, top_k=1, eos_id=eos)
    assert all(a.numel() <= 80 and eos not in a[70:].tolist() for a in got)
    assert torch.equal(got[0], L.generate(cand, p, RETURNED, S_GEN, top_k=1, eos_id=eos))


# ---- 3. one graph for many prompts
def _session(model):
    return [s for k, s in model._decode_sessions.items() if k[0] == "candidates"]


def test_one_captured_step_serves_every_prompt_whose_tail_fits(engine_off, split_keys_32, share_switch):
    cand, batch = model_pair("tiny-llama-gqa", None)
    ops.CANDIDATES_SHARE_LOADS = True  # the step whose workgroups decide their kind from the device's prefix_len
    cand.__dict__.pop("_decode_sessions", None)
    kw = dict(temperature=0.8, top_k=20)

    def both(T):
        p = prompt_of(cand.config, T)
        torch.manual_seed(SEED)
        got = L.generate_candidates(cand, p, 3, RETURNED, S_GEN, **kw)
        torch.manual_seed(SEED)
        want = L.generate_batch(batch, [p] * 3, RETURNED, S_GEN, **kw)
        assert all(torch.equal(a, w) for a, w in zip(got, want)), f"T={T}"
        return got

    first = both(70)
    (sess,) = _session(cand)
    graph = sess.graph
    assert graph is not None and sess.S_tail == 64
    for T in (40, 80):  # a shorter and a longer prompt: tails of 50 and 10 slots fit the 64
        both(T)
        assert _session(cand) == [sess] and sess.graph is graph, f"T={T}: the session was rebuilt"
    both(20)  # a tail of 70 slots does not fit
    assert len(_session(cand)) == 2 and _session(cand)[-1].S_tail == 128
    # captured replay == eager launches
    cand._decode_sessions.clear()
    orig = gb.CandidateSession.__init__
    try:
        gb.CandidateSession.__init__ = lambda self, *a, **k: orig(self, *a, **{**k, "use_graph": False})
        torch.manual_seed(SEED)
        eager = L.generate_candidates(cand, prompt_of(cand.config, 70), 3, RETURNED, S_GEN, **kw)
        assert _session(cand)[0].graph is None
    finally:
        gb.CandidateSession.__init__ = orig
        cand._decode_sessions.clear()
    assert all(torch.equal(a, b) for a, b in zip(first, eager)), "hipGraph replay and eager launches disagree"


# ---- 4. stored and computed once
def _count(prof, pred):
    return sum(n for k, (_, n) in prof.items() if pred(k))


def test_the_prompt_is_prefilled_and_stored_once(engine_off, split_keys_32, share_switch):
    cand, _ = model_pair("tiny-llama", None)
    ops.CANDIDATES_SHARE_LOADS = True  # the shared-load launch in front of the per-row launch
    cfg = cand.config
    n, T = 4, 70
    p = prompt_of(cfg, T)
    is_gemm = lambda k: k.endswith("gemm")  # noqa: E731  (the prompt path's Linears: more than GEMV_MAX_ROWS rows)
    one = gb.DecodeSession(cand, S_GEN, RETURNED, True, use_graph=False, engine=False)
    _hip.prof_begin()
    one.prefill(p)
    prefill = _hip.prof_end()
    assert _count(prefill, is_gemm) > 0
    cand.__dict__.pop("_decode_sessions", None)
    orig = gb.CandidateSession.__init__
    try:
        gb.CandidateSession.__init__ = lambda self, *a, **k: orig(self, *a, **{**k, "use_graph": False})
        L.generate_candidates(cand, p, n, RETURNED, S_GEN, top_k=1)  # builds the session and the caches
        (sess,) = _session(cand)
        for k, v in cand.kv_caches:
            assert k.shape == v.shape == (1, cfg.n_query_groups, S_GEN, cfg.head_size)
            k.fill_(7.0), v.fill_(7.0)  # sentinel
        assert sess.kv_bytes() == 2 * cfg.n_layer * cfg.n_query_groups * cfg.head_size * 2 * (S_GEN + n * 64)
        _hip.prof_begin()
        L.generate_candidates(cand, p, n, RETURNED, S_GEN, top_k=1)
        prof = _hip.prof_end()
        assert _session(cand) == [sess]
    finally:
        gb.CandidateSession.__init__ = orig
        cand._decode_sessions.clear()
    for k, v in cand.kv_caches:
        for c in (k, v):
            assert bool((c[:, :, T:] == 7.0).all()), "a slot past the prompt was written in the shared cache"
            assert not bool((c[:, :, :T] == 7.0).all(dim=-1).any()), "a prompt slot was not written"
    steps = RETURNED - T - 1
    assert _count(prof, is_gemm) == _count(prefill, is_gemm), "the prompt went through the network more than once"
    assert cfg.q_per_kv <= 2 and ops.attn_nsplit(cfg.n_query_groups, S_GEN, cfg.q_per_kv, 1) == 3  # two launches per layer with the switch on
    assert _count(prof, lambda k: k == "attn_fused_decode_prefix") == 2 * cfg.n_layer * steps
    assert _count(prof, lambda k: k == "attn_fused_decode_rows") == 0
    assert _count(prof, lambda k: k == "embedding_rows") == steps and _count(prof, lambda k: k == "argmax_advance_rows") == steps + 1


# ---- 5. capture() leaves every session as the prompt left it
def _single(model, greedy):
    return gb.DecodeSession(model, 32, 32, greedy, sampler=None if greedy else (0.8, 20))


SESSIONS = {
    "single-greedy": (lambda m: _single(m, True), lambda s, p: s.prefill(p[0])),
    "single-sampled": (lambda m: _single(m, False), lambda s, p: s.prefill(p[0])),
    "batch": (lambda m: gb.BatchDecodeSession(m, 2, 32, 32, False, (0.8, 20)), lambda s, p: s.prefill(p, 32)),
    "candidates": (lambda m: gb.CandidateSession(m, 2, 32, gb.candidate_tail_slots(32, 8), False, (0.8, 20)), lambda s, p: s.prefill(p[0], 32)),
    "speculative": (lambda m: gb.SpeculativeSession(m, 32, 32, draft_len=2), lambda s, p: s.prefill(p[0], 32)),
}


@pytest.mark.parametrize("kind", list(SESSIONS))
def test_capture_restores_what_the_step_writes(kind):
    """After an 8-token prompt in a window of 32: capture() (a warm-up step and the capture itself) leaves tokens, pos, end, state,
    every K/V cache and tail and the device generator bit for bit as they were, a second capture() keeps the graph(s), and a step
    then advances."""
    cfg = Config.from_name("tiny-llama")
    model = L.GPT(cfg)
    model.load_state_dict({k: v.to(BF) for k, v in synthetic_state_dict(cfg, MODEL_SEED, perturb=True).items()}, strict=True)
    model = model.to(BF).to(DEV).eval()
    make, prefill = SESSIONS[kind]
    sess = make(model)
    speculative = kind == "speculative"
    torch.manual_seed(SEED)
    with torch.no_grad():
        prefill(sess, [prompt_of(cfg, 8), synthetic_prompt(cfg, 8, 3).to(DEV)])

        def snapshot():
            named = {n: getattr(sess, n) for n in ("tokens", "pos", "end", "state") if hasattr(sess, n)}
            for i, (k, v) in enumerate(sess.caches + getattr(sess, "tails", [])):
                named[f"k{i}"], named[f"v{i}"] = k, v
            named["generator"] = torch.cuda.get_rng_state(DEV)
            return {n: t.clone() for n, t in named.items()}

        def graphs():
            return list(sess.graphs.values()) if speculative else [sess.graph]

        before = snapshot()
        assert int(before["pos"].min()) == 7 and bool(before["k0"].any()), "the prompt is not in the session"
        sess.capture()
        after = snapshot()
        assert before.keys() == after.keys()
        for n in before:
            assert torch.equal(before[n], after[n]), f"{kind}: capture() changed {n}"
        captured = graphs()
        assert len(captured) == (2 if speculative else 1) and all(g is not None for g in captured)
        sess.capture()
        assert all(a is b for a, b in zip(captured, graphs())) and len(graphs()) == len(captured), f"{kind}: captured twice"
        sess.step(True) if speculative else sess.step()
        assert bool((sess.pos > before["pos"]).all()), f"{kind}: pos did not advance"
        if speculative:
            assert int(sess.state[ops.SPEC_POS]) == int(sess.pos) > int(before["state"][ops.SPEC_POS])
