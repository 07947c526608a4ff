"""The retrieval model (tests/retrieval_model.py) on the CPU oracle alone: the conditions tests/test_retrieval_gpu.py relies on.

bf16 OracleGPT, the five families: free-running generation equals the plain-Python automaton, every forced scenario of the GPU
tests is answered right, the smallest top-1 - top-2 gap is at least 4 x the largest logit difference the GPU tests accept
(two logits moving by the whole bound in opposite directions cannot flip an answer), and an attention that loses ONE key makes
the scenarios fail - the proof that they can.
"""
import functools

import pytest
import torch

import retrieval_model as rm
from lit_parrot_amd.config import Config
from lit_parrot_amd.synth import is_linear_key
from oracle import int4 as o4
from oracle import model as om

BF = torch.bfloat16
FAMILIES = ["tiny-llama", "tiny-llama-gqa", "tiny-neox-hs64", "tiny-falcon-40b", "tiny-falcon-7b"]
GPU_MAX_BOUND = 2 ** -5  # x the largest |logit|: the bf16 bound of test_retrieval_gpu.py (the widest of its three)


@functools.lru_cache(maxsize=None)
def family(name):
    cfg, sd, ids = rm.retrieval_model(name)
    return cfg, sd, ids, om.OracleGPT(cfg, sd, "dense")


def run_all(name, oracle=None):
    """Every forced scenario of the GPU tests through the oracle: (rows checked, smallest margin, largest |logit|)."""
    cfg, _, ids, dense = family(name)
    oracle = oracle or dense
    n, margin, largest, memo = 0, float("inf"), 0.0, {}
    for what, scs in rm.forced_scenarios(cfg, ids).items():
        for sc in scs:
            a, b, c = rm.check_rows(ids, sc, rm.oracle_rows(oracle, sc, memo), f"{name} {what}")
            n, margin, largest = n + a, min(margin, b), max(largest, c)
    return n, margin, largest


@pytest.mark.parametrize("name", FAMILIES)
def test_state_dict_has_the_models_keys(name):
    """strict=True loading, fp32, synthetic_state_dict's key order; two entries of 1.0 per embedded token."""
    from lit_parrot_amd.synth import synthetic_state_dict

    cfg = Config.from_name(name, block_size=2048, n_layer=2)
    sd, ids = rm.retrieval_state_dict(cfg, *rm.default_classes(cfg))
    ref = synthetic_state_dict(cfg)
    assert list(sd) == list(ref)
    assert all(sd[k].shape == ref[k].shape and sd[k].dtype == torch.float32 for k in sd)
    wte = sd["transformer.wte.weight"][: ids.n_vocab]
    assert ((wte == 1).sum(dim=1) == 2).all() and ((wte != 0).sum(dim=1) == 2).all()
    assert ids.n_vocab <= cfg.vocab_size and len(set(map(tuple, wte.tolist()))) == ids.n_vocab


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("T,S,n", [(40, 48, 70), (600, 640, 60)])
def test_free_running_oracle_is_the_automaton(name, T, S, n):
    """(40, 48, 70): the ring wraps and the prompt's needles are evicted while their emitted copies keep the answer alive."""
    cfg, _, ids, oracle = family(name)
    prompt = rm.free_prompt(ids, T, seed=T)
    oracle.reset_cache()
    logits = []
    y = om.generate(oracle, torch.tensor(prompt), T + n, S, greedy_ties_lowest=True, logits_log=logits)
    assert y.tolist() == rm.automaton(ids, prompt, T + n, S)
    kinds = {ids.kind[t][0] for t in y.tolist()[T:]}
    assert kinds == {"N", "Q", "NONE"}  # the walk meets found and not-found answers
    scale = max(float(l.float().abs().max()) for l in logits)
    margin = min(float(l.float().topk(2).values.diff().abs()) for l in logits)
    assert margin >= 4 * GPU_MAX_BOUND * scale, (margin, scale)


@pytest.mark.parametrize("name", FAMILIES)
def test_forced_scenarios_are_answered_with_margin(name):
    n, margin, largest = run_all(name)
    print(f"{name}: {n} rows, smallest margin {margin:.2f}, largest |logit| {largest:.1f}")
    assert n > 500
    assert margin >= 4 * GPU_MAX_BOUND * largest, (margin, largest)


@pytest.mark.parametrize("name,mode", [("tiny-llama", "gptq"), ("tiny-falcon-40b", "gptq"), ("tiny-llama", "int8")])
def test_quantised_oracles_answer_the_long_window(name, mode):
    """Two-valued rows quantise exactly: the int4 g128 and LLM.int8 oracles answer like the bf16 one."""
    cfg, sd, ids, _ = family(name)
    if mode == "gptq":
        oracle = om.OracleGPT(cfg, o4.quantize_state_dict(sd, 128, is_linear_key), "gptq", tile_cols=128)
    else:
        oracle = om.OracleGPT(cfg, sd, "int8")
    margin, largest = float("inf"), 0.0
    for sc in rm.forced_scenarios(cfg, ids)["edges"][:3]:
        _, m, l = rm.check_rows(ids, sc, rm.oracle_rows(oracle, sc), f"{name} {mode}")
        margin, largest = min(margin, m), max(largest, l)
    assert margin >= 4 * GPU_MAX_BOUND * largest, (margin, largest)


@pytest.mark.parametrize("name", FAMILIES)
def test_every_row_of_a_prompt_is_answered(name):
    """The all-rows prompts of test_retrieval_gpu.py::test_prompt_pass_every_row: one oracle call, every row checked."""
    cfg, _, ids, oracle = family(name)
    for T in (100, 257, 512):
        prompt = rm.all_rows_prompt(ids, T, seed=T)
        sc = rm.Scenario(tokens=prompt, T=1, S=T)
        with torch.no_grad():
            logits = oracle(torch.tensor(prompt).view(1, -1))[0].float()
        n, margin, largest = rm.check_rows(ids, sc, logits, f"{name} all rows")
        assert n >= T // 3 and margin >= 4 * GPU_MAX_BOUND * largest, (n, margin, largest)
        kinds = {ids.kind[sc.expect(ids, p)][0] for p in sc.rows if sc.expect(ids, p) is not None}
        assert kinds == {"N", "Q", "NONE"}


def test_ring_scenarios_cover_the_ring():
    """S = 48: a needle in EVERY ring slot is asked for as the oldest key and as the newest; S = 160 (positions end at
    block_size): a sample of the slots, and at least one NONE right behind every eviction."""
    for name in ("tiny-llama", "tiny-falcon-40b"):
        cfg, _, ids, _ = family(name)
        scs = rm.forced_scenarios(cfg, ids)
        oldest, newest = rm.ring_coverage(ids, scs["ring48"][0])
        assert len(oldest) == 48 and len(newest) == 48, (name, len(oldest), len(newest))
        oldest, newest = rm.ring_coverage(ids, scs["ring160"][0])
        assert len(oldest) >= 4 and len(newest) >= 4
        for sc in scs["ring48"] + scs["ring160"]:
            assert len(sc.tokens) - sc.T >= 2 * sc.S
            evicted = [p for p in sc.rows if ids.kind[sc.tokens[p]][0] == "Q" and p - sc.S >= 0
                       and ids.kind[sc.tokens[p - sc.S]][:2] == ("N", ids.kind[sc.tokens[p]][1])]
            assert evicted and all(sc.expect(ids, p) == ids.NONE[ids.kind[sc.tokens[p]][1]] for p in evicted)


def test_edge_slots_restate_the_engines_partition():
    assert rm.engine_split_per(32, 64) == (1, 32) and rm.engine_split_per(33, 64) == (2, 24)
    assert rm.engine_split_per(64, 64) == (2, 32) and rm.engine_split_per(65, 64) == (4, 24)
    assert rm.engine_split_per(128, 64) == (4, 32) and rm.engine_split_per(129, 64) == (8, 24)
    assert rm.engine_split_per(1100, 64) == (8, 144) and rm.engine_split_per(1100, 128) == (8, 140)
    slots = rm.edge_slots(1100, 1200, 64, 6)
    assert {0, 1, 31, 32, 33, 63, 64, 127, 128, 255, 256, 511, 512, 513, 1098, 1099} <= set(slots)
    assert {s * 144 + d for s in range(1, 8) for d in (-1, 0)} <= set(slots) and {599, 600} <= set(slots)


# ---- an attention that is wrong by ONE key
def lose_key(column):
    """F.scaled_dot_product_attention as oracle.model sees it, with one key removed from single-row (decode) calls:
    ``column(n_valid)`` -> the slot to clear."""
    real = torch.nn.functional.scaled_dot_product_attention

    def sdpa(q, k, v, attn_mask=None, **kw):
        if attn_mask is not None and q.size(-2) == 1:
            attn_mask = attn_mask.clone()
            attn_mask[..., column(int(attn_mask[0, 0, 0].sum()))] = False
        return real(q, k, v, attn_mask=attn_mask, **kw)

    return sdpa


BROKEN = {
    "oldest": lambda n: 0,
    "newest-but-one": lambda n: n - 2,
    "split-edge": lambda n: 3 * rm.engine_split_per(n, 64)[1],
}


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-falcon-7b"])
@pytest.mark.parametrize("which", list(BROKEN))
def test_one_lost_key_fails_the_scenarios(name, which, monkeypatch):
    """The same scenarios, the oracle's attention short of one key (decode rows only): wrong answers are reported.  With
    N(0, 0.02) weights this moves the logits by a tenth of the bound at these windows (testing section)."""
    cfg, _, ids, oracle = family(name)
    scs = rm.forced_scenarios(cfg, ids)
    monkeypatch.setattr(om.F, "scaled_dot_product_attention", lose_key(BROKEN[which]))
    wrong = 0
    for sc in scs["edges"] + scs["growing"]:
        try:
            rm.check_rows(ids, sc, rm.oracle_rows(oracle, sc), which)
        except AssertionError as e:
            assert "emitted" in str(e)
            wrong += 1
    assert wrong >= 1, f"no scenario noticed the lost key ({which})"
    monkeypatch.undo()
    for sc in scs["edges"][:2]:
        rm.check_rows(ids, sc, rm.oracle_rows(oracle, sc), "restored")
