"""Every executor on the retrieval model (tests/retrieval_model.py): the next token is decided by ONE key slot (``-m gpu``).

Forced tokens (written into the session's ``tokens`` between steps, as test_engine_gpu.py::run_session does) put needles at the
slots where the executors partition, merge, wrap or join their keys; every decided row must emit ``expected_next`` - ten lines of
Python over the token list - and its logits must agree with the bf16 oracle's within the bounds the suite already applies against
the oracle.  tests/test_retrieval_host.py proves on the CPU that the oracle alone answers all of these with a margin of at least
4 x the widest bound, and that one lost key makes them fail.

Smallest top-1 - top-2 gap over all forced rows checked here, measured on an MI355X / the oracle's over the same rows (largest
|logit|): tiny-llama 4.62 / 4.62 (24), tiny-llama-gqa 9.19 / 9.19 (34), tiny-neox-hs64 9.19 / 9.19 (34), tiny-falcon-40b 15.5 / 15.5
(48), tiny-falcon-7b 14.5 / 14.5 (45); int4 and LLM.int8 weights give the same gaps (free-running oracle: 4.56 for tiny-llama).
Largest |logit - oracle| / scale seen: bf16 9.1e-3 (bound 3.1e-2), int4 1.36e-2 (1.5e-2), int8 9.1e-3 (3e-2).
"""
import functools
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

import lit_parrot_amd as L  # noqa: E402
import retrieval_model as rm  # noqa: E402
from lit_parrot_amd import ops  # noqa: E402
from lit_parrot_amd.engine import StreamEngine  # noqa: E402
from lit_parrot_amd.generate import base as gb  # noqa: E402
from lit_parrot_amd.synth import is_linear_key  # noqa: E402
from oracle import int4 as o4  # noqa: E402
from oracle import model as om  # noqa: E402
from test_engine_gpu import cpu_rsqrt_mode  # noqa: E402,F401  (autouse: the CPU-run reference's rsqrt rounding)

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
BF16 = ["tiny-llama", "tiny-llama-gqa", "tiny-neox-hs64", "tiny-falcon-40b", "tiny-falcon-7b"]
MODELS = [(n, "bf16") for n in BF16] + [("tiny-llama", "int4"), ("tiny-falcon-40b", "int4"), ("tiny-llama", "int8")]
ROW_MODELS = [m for m in MODELS if m[1] != "int8"]  # LLM.int8 Linears decode one sequence at a time (model.py)
EXECUTORS = {"multi-launch": dict(engine=False, use_graph=True), "multi-launch-eager": dict(engine=False, use_graph=False),
             "engine": dict(engine=True, use_graph=True)}
# |logit - bf16 oracle's| per decided row: (max / scale, mean / scale or None, absolute mean or None), scale = max(1, max |oracle logit|):
# the bounds of test_engine_gpu.py's comparisons against the oracle
BOUNDS = {"bf16": (2 ** -5, 2e-3, None), "int4": (1.5e-2, None, 3e-3), "int8": (3e-2, None, None)}


@functools.lru_cache(maxsize=None)
def family(name):
    cfg, sd, ids = rm.retrieval_model(name)
    return cfg, sd, ids, om.OracleGPT(cfg, sd, "dense"), rm.forced_scenarios(cfg, ids)


@functools.lru_cache(maxsize=None)
def gpu_model(name, mode):
    cfg, sd, ids, _, _ = family(name)
    if mode == "int4":
        with L.quantization("gptq.int4-g128"):
            model = L.GPT(cfg)
        model.load_state_dict(o4.quantize_state_dict(sd, 128, is_linear_key), strict=True)
    elif mode == "int8":
        with L.quantization("bnb.int8"):
            model = L.GPT(cfg)
        model.load_state_dict(dict(sd), strict=False)  # (quantises on arrival, as test_engine_gpu.py::int8_model)
    else:
        model = L.GPT(cfg)
        model.load_state_dict(sd, strict=True)
    return model.to(BF).to(DEV).eval()


_ORACLE = {}


def oracle_logits(name, what):
    """The bf16 oracle's logits of scenario list ``what``: computed once, shared by every weight format and executor."""
    if (name, what) not in _ORACLE:
        _, _, _, oracle, scs = family(name)
        memo = {}
        _ORACLE[(name, what)] = [rm.oracle_rows(oracle, sc, memo) for sc in scs[what]]
    return _ORACLE[(name, what)]


def check(name, mode, ids, sc, got, ref, what):
    """The assertions of one scenario: tokens, then logits against the oracle row by row (decided rows)."""
    got = got.float().cpu()
    n, margin, _ = rm.check_rows(ids, sc, got, f"{name} {mode} {what}")
    tol_max, tol_mean, tol_mean_abs = BOUNDS[mode]
    worst = 0.0
    for i, p in enumerate(sc.rows):
        if sc.expect(ids, p) is None:
            continue
        d = (got[i] - ref[i]).abs()
        scale = max(1.0, float(ref[i].abs().max()))
        worst = max(worst, float(d.max()) / scale)
        assert float(d.max()) <= tol_max * scale, (name, mode, what, p, float(d.max()), scale)
        assert tol_mean is None or float(d.mean()) <= tol_mean * scale, (name, mode, what, p, float(d.mean()), scale)
        assert tol_mean_abs is None or float(d.mean()) <= tol_mean_abs, (name, mode, what, p, float(d.mean()))
    return n, margin, worst


def report(name, mode, what, stats):
    n = sum(s[0] for s in stats)
    print(f"retrieval {name} {mode} {what}: {n} rows, smallest margin {min(s[1] for s in stats):.2f}, "
          f"largest |logit - oracle| / scale {max(s[2] for s in stats):.2e}")
    assert n > 0


def make_session(model, sc_list, **executor):
    S = sc_list[0].S
    assert all(sc.S == S for sc in sc_list)
    total = max(len(sc.tokens) for sc in sc_list) + 1
    model.reset_cache()
    model.__dict__.pop("_decode_sessions", None)
    sess = gb.DecodeSession(model, S, total, True, use_graph=executor["use_graph"], engine=executor["engine"])
    assert (sess.eng is not None) == executor["engine"]
    return sess


@torch.no_grad()
def run_forced(sess, sc, after_prefill=None):
    """``sc``'s tokens through ``sess``: the prompt, then one step per forced token.  Returns the logits of rows T-1 .. (n, V)."""
    toks = torch.tensor(sc.tokens, device=DEV)
    T, n = sc.T, len(sc.tokens)
    logits = sess.prefill(toks[:T])
    rows = [logits.view(-1).float().clone()]
    ops.argmax_advance(logits, sess.tokens, sess.pos)
    sess.tokens[:n].copy_(toks)
    sess.capture()
    if after_prefill is not None:
        after_prefill(sess)
    for _ in range(T, n):
        rows.append(sess.step().float().clone())
        sess.tokens[:n].copy_(toks)  # force: the step wrote its own arg-max behind its row
    sess.check_error()
    assert int(sess.pos.item()) == n
    return torch.stack(rows)


def run_scenarios(name, mode, what, executor):
    cfg, _, ids, _, scs = family(name)
    model = gpu_model(name, mode)
    if executor["engine"]:
        assert StreamEngine.supported(model) is None
    ref = oracle_logits(name, what)
    sessions = {}  # one per window size, serving its scenarios in turn
    stats = []
    for sc, r in zip(scs[what], ref):
        if sc.S not in sessions:
            sessions.clear()
            sessions[sc.S] = make_session(model, [x for x in scs[what] if x.S == sc.S], **executor)
        stats.append(check(name, mode, ids, sc, run_forced(sessions[sc.S], sc), r, what))
    report(name, mode, what, stats)


# ------------------------------------------------------------------------------------------------ one sequence
@pytest.mark.parametrize("executor", list(EXECUTORS))
@pytest.mark.parametrize("name,mode", MODELS)
def test_long_window_edges(name, mode, executor):
    """T = 1100 in S = 1200: one needle per class per scenario, at block edges, the prompt's last two slots and both sides of every
    split edge of the engine (8 CUs per head: 144 keys each) and of the multi-launch step (2 splits of 600 slots); the first logits
    come out of the prompt pass (the MFMA prefill's last row), the others out of decode steps."""
    run_scenarios(name, mode, "edges", EXECUTORS[executor])


@pytest.mark.parametrize("executor", list(EXECUTORS))
@pytest.mark.parametrize("name,mode", MODELS)
def test_growing_window(name, mode, executor):
    """The rows that see 32, 33, 64, 65, 128 and 129 keys - where the engine brings in its 2nd, 4th and 8th CU - ask for a needle in
    the first split and for one in the last, and again a few rows later."""
    run_scenarios(name, mode, "growing", EXECUTORS[executor])


@pytest.mark.parametrize("executor", ["multi-launch", "engine"])
@pytest.mark.parametrize("name,mode", MODELS)
def test_ring_window(name, mode, executor):
    """S = 48 (every ring slot holds a needle that is asked for as the oldest key and as the newest) and S = 160: found S - 1 rows
    behind the needle, NONE one row later."""
    run_scenarios(name, mode, "ring48", EXECUTORS[executor])
    run_scenarios(name, mode, "ring160", EXECUTORS[executor])


@pytest.mark.parametrize("engine", [False, True])
@pytest.mark.parametrize("name,mode", MODELS)
def test_generate_is_the_automaton(name, mode, engine, monkeypatch):
    """Free-running ``generate(top_k=1)`` on both executors: the ring wraps ((40, 48, 70): the prompt's needles are evicted, their
    emitted copies keep the answers alive), and a 600-token prompt."""
    _, _, ids, _, _ = family(name)
    model = gpu_model(name, mode)
    monkeypatch.setattr(gb, "ENGINE_DEFAULT", engine)
    for T, S, n in ((40, 48, 70), (600, 640, 60)):
        prompt = rm.free_prompt(ids, T, seed=T)
        model.reset_cache()
        model.__dict__.pop("_decode_sessions", None)
        y = L.generate(model, torch.tensor(prompt, device=DEV), T + n, S, top_k=1).cpu().tolist()
        sess = next(iter(model._decode_sessions.values()))
        assert (sess.eng is not None) == engine
        sess.check_error()
        assert y == rm.automaton(ids, prompt, T + n, S), (name, mode, engine, T, S)
    model.__dict__.pop("_decode_sessions", None)


@pytest.mark.parametrize("executor", list(EXECUTORS))
@pytest.mark.parametrize("name,mode", [("tiny-llama-gqa", "bf16"), ("tiny-falcon-40b", "int4")])
def test_an_erased_key_slot_is_missed(name, mode, executor):
    """The answers hang on the ONE slot: the K and V rows of a needle's slot zeroed in the cache behind the prompt pass (a change of
    the data, not of the executor), and the decode rows of its class answer "not found" while the other classes are still found;
    a different needle slot in every scenario tried."""
    cfg, _, ids, _, scs = family(name)
    model = gpu_model(name, mode)
    sess = make_session(model, scs["edges"], **EXECUTORS[executor])
    erased = 0
    for sc in scs["edges"][:: max(1, len(scs["edges"]) // 4)]:
        slots = [p for p in range(sc.T - 1) if ids.kind[sc.tokens[p]][0] == "N"]
        slot = slots[erased % len(slots)]

        def erase(s, slot=slot):
            for k, v in s.caches[:1]:
                k[:, slot].zero_()
                v[:, slot].zero_()

        blind = rm.Scenario(tokens=sc.tokens[:slot] + [ids.fill[0]] + sc.tokens[slot + 1:], T=sc.T, S=sc.S)
        got = run_forced(sess, sc, erase).argmax(dim=-1).cpu().tolist()
        rows = [(i, p) for i, p in enumerate(sc.rows) if p >= sc.T and sc.expect(ids, p) is not None]
        assert [got[i] for i, _ in rows] == [blind.expect(ids, p) for _, p in rows], (name, mode, executor, slot)
        b = ids.kind[sc.tokens[slot]][1]
        assert any(blind.expect(ids, p) == ids.NONE[b] != sc.expect(ids, p) for _, p in rows)
        erased += 1
    assert erased >= 3


def test_no_garbage_collection_inside_a_capture():
    """Dropped models leave their captured graphs to the cyclic collector (model <-> cached sessions); a collection inside ANOTHER
    capture destroys them there and the process aborts.  The collector is off while a step is being captured -
    the warm-up step in front runs with it on - and back on afterwards."""
    _, _, ids, _, scs = family("tiny-llama")
    sess = make_session(gpu_model("tiny-llama", "bf16"), scs["growing"][:1], engine=False, use_graph=True)
    seen, step = [], sess._step
    sess._step = lambda: (seen.append(gc.isenabled()), step())[1]
    assert gc.isenabled()
    with torch.no_grad():
        ops.argmax_advance(sess.prefill(torch.tensor(scs["growing"][0].tokens[:20], device=DEV)), sess.tokens, sess.pos)
        sess.capture()
    assert seen == [True, False] and gc.isenabled() and sess.graph is not None


# ------------------------------------------------------------------------------------------------ prompts
@pytest.mark.parametrize("name,mode", MODELS)
def test_prompt_pass_last_row(name, mode):
    """Prompts of 32 and 100 (the row-by-row prompt attention) and 257 and 512 tokens (the MFMA kernel): the last row asks for a
    needle at a key-block edge or in row T - 2; the other classes are asked by decode steps."""
    run_scenarios(name, mode, "prefill", EXECUTORS["multi-launch"])


@torch.no_grad()
@pytest.mark.parametrize("name,mode", MODELS)
def test_prompt_pass_every_row(name, mode):
    """``model(idx)`` returns the logits of ALL rows: every query row of a prompt must find the needle planted before it (or none) -
    without a cache (positions 0 .. T-1: the MFMA kernel from 160 rows on) and through the cache (the row-by-row kernel)."""
    cfg, _, ids, oracle, _ = family(name)
    model = gpu_model(name, mode)
    for T in (100, 257, 512):
        prompt = rm.all_rows_prompt(ids, T, seed=T)
        sc = rm.Scenario(tokens=prompt, T=1, S=T)  # rows 0 .. T-1, all keys in the window
        idx = torch.tensor(prompt).view(1, -1)
        ref = oracle(idx)[0].float()
        model.reset_cache()
        stats = [check(name, mode, ids, sc, model(idx.to(DEV))[0], ref, f"all rows, T={T}")]
        model.reset_cache()
        got = model(idx.to(DEV), T + 8, torch.arange(T, device=DEV))[0]
        stats.append(check(name, mode, ids, sc, got, ref, f"all rows through the cache, T={T}"))
        report(name, mode, f"all rows T={T}", stats)
    model.reset_cache()


@torch.no_grad()
@pytest.mark.parametrize("mfma", [False, True])
@pytest.mark.parametrize("name,mode", MODELS)
def test_prompt_in_two_calls(name, mode, mfma):
    """A prompt processed in two multi-row calls (driven as CandidateSession.prefill drives ``run_rows``): the second call's rows
    start at pos0 = 37 behind the first call's keys, where the needle its last row asks for lies.  ``mfma``: the second call through
    the matrix-core kernel (the ``run_rows`` argument that says the call does not wrap the ring), else through the row-by-row kernel."""
    cfg, _, ids, oracle, _ = family(name)
    model = gpu_model(name, mode)
    T1, T2, S = 37, 200, 300
    for slot in (0, 15, 16, 31, 32, 35, 36):
        sc = rm.prefill_scenario(ids, T1 + T2, S, [slot, T1, T1 + T2 - 2], seed=slot)
        ref = rm.oracle_rows(oracle, rm.Scenario(tokens=sc.tokens[: sc.T], T=sc.T, S=S))
        sess = make_session(model, [sc], engine=False, use_graph=False)
        toks = torch.tensor(sc.tokens, device=DEV)
        sess.tokens[: len(sc.tokens)].copy_(toks)
        sess.pos.zero_()
        for T0, M in ((0, T1), (T1, T2)):
            ws = model.workspace(M, DEV, 1)
            sess.pos.fill_(T0)
            logits = model.run_rows(ws, sess.tokens, sess.pos, sess.pos, S, sess.caches, model.rope_cache, pos_is_zero=T0 == 0 or mfma)
        one = rm.Scenario(tokens=sc.tokens[: sc.T], T=sc.T, S=S)
        check(name, mode, ids, one, logits.view(1, -1), ref, f"two calls, needle at {slot}, mfma={mfma}")
    model.reset_cache()


# ------------------------------------------------------------------------------------------------ rows
def force_rows(sess, follow):
    sess.tokens[:, : follow.shape[1]].copy_(follow)


@torch.no_grad()
def run_rows_session(sess, scs, prefill):
    """The scenarios ``scs`` as the rows of a batched / candidates session.  Returns a (rows of the scenario, V) tensor per row."""
    n_steps = len(scs[0].tokens) - scs[0].T
    assert all(len(sc.tokens) - sc.T == n_steps for sc in scs)
    width = max(len(sc.tokens) for sc in scs)
    follow = torch.zeros((len(scs), width), dtype=torch.int64)
    for b, sc in enumerate(scs):
        follow[b, : len(sc.tokens)] = torch.tensor(sc.tokens)
    follow = follow.to(DEV)
    prefill(sess)
    sess.capture()
    rows = [sess.first_logits.float().clone()]
    sess.sample(sess.first_logits, -1)
    force_rows(sess, follow)
    for _ in range(n_steps):
        sess.step()
        rows.append(sess.ws.logits.float().clone())
        force_rows(sess, follow)
    assert sess.pos.cpu().tolist() == [len(sc.tokens) for sc in scs]
    rows = torch.stack(rows)  # (steps + 1, B, V)
    return [rows[:, b] for b in range(len(scs))]


@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("name,mode", ROW_MODELS)
def test_batched_rows_find_their_own_needles(name, mode, B):
    """BatchDecodeSession: every row has its own prompt length (40 .. 600), needle slots and answers - the same class has a
    different answer in every row, so a row that reads another row's cache or position emits that row's answer."""
    cfg, _, ids, _, scs = family(name)
    scs, ref = scs[f"batch{B}"], oracle_logits(name, f"batch{B}")
    model = gpu_model(name, mode)
    assert model.batched_decode_unsupported() is None
    answers = [{ids.kind[t][1:] for t in sc.tokens if ids.kind[t][0] == "N"} for sc in scs]
    assert all(a.isdisjoint(b) for i, a in enumerate(answers) for b in answers[i + 1:])
    model.reset_cache()
    model.__dict__.pop("_decode_sessions", None)
    total = max(len(sc.tokens) for sc in scs) + 1
    sess = gb.BatchDecodeSession(model, B, scs[0].S, total, True)
    got = run_rows_session(sess, scs, lambda s: s.prefill([torch.tensor(sc.tokens[: sc.T], device=DEV) for sc in scs], total))
    report(name, mode, f"batch{B}", [check(name, mode, ids, sc, g, r, f"batch row {b} of {B}") for b, (sc, g, r) in enumerate(zip(scs, got, ref))])
    model.reset_cache()


@pytest.mark.parametrize("n,share", [(4, False), (4, True), (8, True)])
@pytest.mark.parametrize("name,mode", ROW_MODELS)
def test_candidates_find_the_shared_and_their_own_needles(name, mode, n, share, monkeypatch):
    """CandidateSession, a 600-token prompt in 704 slots: needles on both sides of every edge of the splits the rows share
    (``shared_splits``), at the prompt's last slot and at the tails' first; every row plants its own answer in its tail and must
    find that one, never a sibling's.  With and without the shared-load launch in front of the per-row launch."""
    cfg, _, ids, _, scs = family(name)
    scs, ref = scs[f"candidates{n}"], oracle_logits(name, f"candidates{n}")
    monkeypatch.setattr(ops, "ATTN_SPLIT_KEYS", rm.CAND_SPLIT_KEYS[n])
    monkeypatch.setattr(ops, "CANDIDATES_SHARE_LOADS", share)
    T, S = rm.CAND_T, rm.CAND_S
    nsplit = ops.attn_nsplit(cfg.n_query_groups, S, cfg.q_per_kv, 1)
    per = -(-S // nsplit)
    edges = {(j + 1) * per for j in gb.shared_splits(S, nsplit, T)}
    assert len(edges) >= 4 and {e - d for e in edges for d in (0, 1)} | {T - 1, T} == set(rm.candidate_slots(n))
    model = gpu_model(name, mode)
    assert model.batched_decode_unsupported() is None
    model.reset_cache()
    model.__dict__.pop("_decode_sessions", None)
    total = max(len(sc.tokens) for sc in scs) + 1
    sess = gb.CandidateSession(model, n, S, gb.candidate_tail_slots(total, T), True)
    stats = []
    for g in range(0, len(scs), n):
        group = scs[g:g + n]
        assert len({tuple(sc.tokens[:T]) for sc in group}) == 1 and len({sc.tokens[T + g // n % 2] for sc in group}) == n
        got = run_rows_session(sess, group, lambda s: s.prefill(torch.tensor(group[0].tokens[:T], device=DEV), total))
        stats += [check(name, mode, ids, sc, x, r, f"candidate {b} of {n}, group {g // n}") for b, (sc, x, r) in enumerate(zip(group, got, ref[g:g + n]))]
    report(name, mode, f"candidates{n} share={share}", stats)
    model.reset_cache()


@pytest.mark.parametrize("name,mode", ROW_MODELS)
def test_speculative_is_the_automaton(name, mode, monkeypatch):
    """generate_speculative on a prompt that ends in a query: the trajectory repeats (Q -> N -> Q -> ...), so the n-gram drafts are
    accepted and the multi-row verification pass decides tokens - which must be the automaton's."""
    _, _, ids, _, _ = family(name)
    model = gpu_model(name, mode)
    assert model.speculative_decode_unsupported() is None
    monkeypatch.setattr(gb, "ENGINE_DEFAULT", False)
    for T, n, draft_len in ((40, 80, 3), (600, 60, 7)):
        prompt = rm.free_prompt(ids, T, seed=T)
        model.reset_cache()
        model.__dict__.pop("_decode_sessions", None)
        y, stats = gb.generate_speculative(model, torch.tensor(prompt, device=DEV), T + n, T + n + 8, draft_len=draft_len, return_stats=True)
        assert y.cpu().tolist() == rm.automaton(ids, prompt, T + n, T + n + 8), (name, mode, T)
        assert stats["accepted"] >= 1 and stats["matched_steps"] >= 1 and stats["steps"] < n - 1, stats
    model.__dict__.pop("_decode_sessions", None)
    model.reset_cache()
