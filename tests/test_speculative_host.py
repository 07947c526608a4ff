"""Prompt-lookup speculative decoding, CPU side: the new entry points are declared and exported and refuse bad arguments without
a device; generate_speculative / GPT.speculative_decode_unsupported check their inputs before any device work; and the rules of
the two new kernels restated in plain Python (``draft_rule``, ``verify_rule``, ``simulate``) - tests/test_speculative_gpu.py
compares the kernels and the loop's step accounting against these."""
import numpy as np
import pytest
import torch

import lit_parrot_amd as L
from lit_parrot_amd import _hip
from lit_parrot_amd import adapter as A
from lit_parrot_amd.config import Config, name_to_config

NEW = ["parrot_ngram_draft", "parrot_verify_advance", "parrot_attn_fused_decode_seq"]
P = 0x10000  # a 16-byte aligned stand-in pointer: every call below fails its checks before anything is launched


# ------------------------------------------------------------------------------------------------ the rules, restated
def draft_rule(tokens, pos, K, ngram_max=3, ngram_min=1):
    """``tokens[0 .. pos]`` are known.  For n = ngram_max .. ngram_min (an n with pos - n + 1 < 0 is skipped): the largest j with
    j + n <= pos and tokens[j:j+n] == tokens[pos-n+1:pos+1]; on the first n with a match draft i = tokens[j+n+i] while j+n+i <= pos.
    Every other draft is tokens[pos].  Returns (the K drafts, how many were copied)."""
    tokens = [int(t) for t in tokens]
    for n in range(ngram_max, ngram_min - 1, -1):
        if pos - n + 1 < 0:
            continue
        tail = tokens[pos - n + 1:pos + 1]
        for j in range(pos - n, -1, -1):
            if tokens[j:j + n] == tail:
                follow = j + n
                return [tokens[follow + i] if follow + i <= pos else tokens[pos] for i in range(K)], min(K, pos - follow + 1)
    return [tokens[pos]] * K, 0


def verify_rule(argmaxes, tokens, pos, end, eos_id=-1):
    """Greedy verification of M = len(argmaxes) rows on the list ``tokens`` (changed in place; ``tokens[pos+1 .. pos+M-1]`` are
    the drafts).  Returns (new pos, accepted count, or None when the sequence is frozen: nothing written, no advance)."""
    stop = min(end, len(tokens))
    if pos + 1 >= stop or (eos_id >= 0 and tokens[pos] == eos_id):
        return pos, None
    K = len(argmaxes) - 1
    c = 0
    while (c < K and argmaxes[c] == tokens[pos + 1 + c] and not (eos_id >= 0 and argmaxes[c] == eos_id)
           and pos + 2 + c < stop):  # (the token after an accepted draft needs a slot before `end`)
        c += 1
    tokens[pos + 1 + c] = argmaxes[c]
    return pos + c + 1, c


def simulate(full, T, max_returned_tokens, K, ngram_max=3, ngram_min=1, eos_id=None, limit=None, drafter=None):
    """The loop of generate_speculative replayed on ``full``, the tokens plain greedy decoding produces WITHOUT eos_id (prompt of T
    tokens first): the M-row step is taken when the drafting matched and pos + M <= limit, else the one-row step.  ``drafter(known,
    pos) -> (drafts, matched)`` replaces the lookup.  Returns {steps, accepted, matched_steps} and the length of the result."""
    full = [int(t) for t in full]
    M = K + 1
    limit = max_returned_tokens if limit is None else limit
    p, steps, accepted, matched_steps = T, 0, 0, 0
    while True:
        stop_eos = eos_id is not None and full[p] == eos_id
        if stop_eos or p + 1 >= max_returned_tokens:
            break
        drafts, matched = drafter(full[:p + 1], p) if drafter else draft_rule(full[:p + 1], p, K, ngram_max, ngram_min)
        steps += 1
        if matched > 0 and p + M <= limit:
            buf = full[:p + 1] + list(drafts) + [0]
            p_new, c = verify_rule(full[p + 1:p + 1 + M], buf, p, max_returned_tokens, -1 if eos_id is None else eos_id)
            assert buf[:p_new + 1] == full[:p_new + 1]
            accepted += c
            matched_steps += 1
            p = p_new
        else:
            p += 1
    return {"steps": steps, "accepted": accepted, "matched_steps": matched_steps}, (p if stop_eos else p + 1)


def test_the_restated_rules_on_small_cases():
    #          0  1  2  3  4  5  6  7  8
    toks = [5, 6, 7, 8, 5, 6, 7, 9, 6, 7]
    assert draft_rule(toks, 9, 3) == ([9, 6, 7], 3)            # (6, 7) at 5..6 is the latest earlier occurrence: 9, 6, 7 follow
    assert draft_rule(toks, 9, 5) == ([9, 6, 7, 7, 7], 3)      # the continuation runs into pos: padded with tokens[pos]
    assert draft_rule(toks, 6, 2) == ([8, 5], 2)               # (5, 6, 7) at 0..2
    assert draft_rule(toks, 7, 4) == ([9, 9, 9, 9], 0)         # 9 was never seen
    assert draft_rule(toks, 0, 2) == ([5, 5], 0)               # nothing before position 0
    assert draft_rule([4, 4], 1, 3, 3, 1) == ([4, 4, 4], 1)    # n = 3, 2 skipped (pos < n); j = 0, one token follows up to pos
    assert draft_rule(toks, 9, 2, ngram_max=3, ngram_min=3) == ([7, 7], 0)  # (9, 6, 7) never occurred before
    buf = [1, 2, 3, 4, 0, 0]
    assert verify_rule([3, 4, 9], buf, 1, 6) == (4, 2) and buf == [1, 2, 3, 4, 9, 0]
    buf = [1, 2, 3, 4, 0, 0]
    assert verify_rule([3, 7, 9], buf, 1, 6) == (3, 1) and buf == [1, 2, 3, 7, 0, 0]
    buf = [1, 2, 3, 4, 0, 0]
    assert verify_rule([3, 4, 9], buf, 1, 4) == (3, 1) and buf == [1, 2, 3, 4, 0, 0]   # end = 4: nothing written at 4
    buf = [1, 2, 3, 4, 0, 0]
    assert verify_rule([3, 4, 9], buf, 1, 6, eos_id=3) == (2, 0)                      # eos is written, not passed
    assert verify_rule([3, 4, 9], buf, 2, 6, eos_id=3) == (2, None)                   # and then frozen
    assert verify_rule([3, 4, 9], [1, 2, 3, 4, 0, 0], 5, 6) == (5, None)


def test_the_rule_accepts_what_the_issue_counted_on_the_reference_run(golden_dir):
    """The reference's own Pythia-160M greedy run (tests/golden/generate_bf16.npz): n-grams 3..1 accept 22 of the 63 decode tokens
    with one draft (41 steps instead of 63).  Seven drafts accept 37 when the rule alone is counted; the loop, which takes the
    one-row step once pos + 8 would pass the 192 tokens, accepts 32 of them (31 steps)."""
    g = np.load(golden_dir / "generate_bf16.npz")
    full = g["tokens"].tolist()
    s1, n1 = simulate(full, 128, 192, 1)
    assert (s1["accepted"], s1["steps"], n1) == (22, 41, 192)
    rule_alone, _ = simulate(full + [0] * 8, 128, 192, 7, limit=10 ** 6)
    assert rule_alone["accepted"] == 37 and rule_alone["steps"] + rule_alone["accepted"] == 63
    s7, _ = simulate(full, 128, 192, 7)
    assert (s7["accepted"], s7["steps"]) == (32, 31)


# ------------------------------------------------------------------------------------------------ C ABI
def test_new_entry_points_are_declared_and_exported(hip_lib):
    from test_abi_and_host import declared_functions

    for n in NEW:
        assert n in declared_functions() and n in _hip.SIGNATURES and hasattr(hip_lib, n), n
    names = [hip_lib.parrot_kernel_name(i).decode() for i in range(64)]
    for k in ("ngram_draft", "verify_advance", "attn_fused_decode_seq"):
        assert k in names, k


@pytest.mark.parametrize("bad", [dict(tokens=None), dict(pos=None), dict(state=None), dict(L=0), dict(K=0), dict(K=8), dict(nmax=17),
                                 dict(nmin=0), dict(nmax=1, nmin=2)])
def test_ngram_draft_rejects_bad_arguments(hip_lib, bad):
    a = dict(tokens=P, L=64, pos=P, K=3, nmax=3, nmin=1, state=P)
    a.update(bad)
    assert hip_lib.parrot_ngram_draft(*a.values(), None) == -1, _hip.last_error()


@pytest.mark.parametrize("bad", [dict(logits=None), dict(tokens=None), dict(pos=None), dict(end=None), dict(state=None), dict(M=1),
                                 dict(M=9), dict(ldl=99), dict(L=1), dict(eos_id=-2), dict(V=0)])
def test_verify_advance_rejects_bad_arguments(hip_lib, bad):
    a = dict(logits=P, V=100, ldl=104, M=4, tokens=P, L=64, pos=P, end=P, eos_id=-1, state=P, row_pos=None)
    a.update(bad)
    assert hip_lib.parrot_verify_advance(*a.values(), None) == -1, _hip.last_error()


def _attn_seq(lib, **kw):
    # a consistent call: 2 groups x 2 query heads of 64 dims, window 32, 2 splits, M = 3
    a = dict(qkv=P, ldqkv=2 * 4 * 64, M=3, cos=P, sin=P, n_elem=64, pos=P, n_groups=2, q_per_kv=2, hs=64, S=32, nsplit=2, ws=P,
             tickets=P, n_tickets=3 * 4, k=P, v=P, y=P, ldy=4 * 64, softmax_mode=0)
    a.update(kw)
    return lib.parrot_attn_fused_decode_seq(*a.values(), None)


@pytest.mark.parametrize("bad", [dict(M=0), dict(M=9), dict(pos=None), dict(qkv=None), dict(k=None), dict(ldqkv=2 * 4 * 64 - 8),
                                 dict(ldy=4 * 64 - 1), dict(n_tickets=11), dict(tickets=None), dict(nsplit=0), dict(softmax_mode=2),
                                 dict(M=5, S=4, n_tickets=20, nsplit=1)])
def test_attn_fused_decode_seq_rejects_bad_arguments(hip_lib, bad):
    assert _attn_seq(hip_lib, **bad) == -1, _hip.last_error()


def test_attn_fused_decode_seq_scope_matches_the_one_row_kernel(hip_lib):
    assert _attn_seq(hip_lib, q_per_kv=17, ldqkv=2 * 19 * 64, ldy=34 * 64, n_tickets=3 * 34) == -3
    assert "query heads" in _hip.last_error()
    assert _attn_seq(hip_lib, hs=80, n_elem=80, ldqkv=2 * 4 * 80, ldy=4 * 80) == -3
    assert _attn_seq(hip_lib, softmax_mode=1) == -3  # softmax_mode 1: one split only, as the one-row call


# ------------------------------------------------------------------------------------------------ host checks
def test_generate_speculative_checks_its_arguments_without_a_device():
    cfg = Config.from_name("tiny-llama")
    model = L.GPT(cfg).to(torch.bfloat16)
    p = torch.arange(4)
    with pytest.raises(L.ParrotHipError, match="HIP device"):  # a CPU model: no fallback
        L.generate_speculative(model, p, 8, 8)
    for k in (0, 8, -1):
        with pytest.raises(L.ParrotHipError, match="draft_len"):
            L.generate_speculative(model, p, 8, 8, draft_len=k)
    with pytest.raises(L.ParrotHipError, match="n-grams"):
        L.generate_speculative(model, p, 8, 8, ngram_max=1, ngram_min=2)
    with pytest.raises(L.ParrotHipError, match="sliding window"):  # a window shorter than the result
        L.generate_speculative(model, p, 12, 8)
    with pytest.raises(AssertionError):  # generate()'s own checks
        L.generate_speculative(model, p, 4, 8)
    with pytest.raises(AssertionError):
        L.generate_speculative(model, torch.arange(8), 12, 6)
    with pytest.raises(L.ParrotHipError, match="block_size"):
        L.generate_speculative(model, p, cfg.block_size + 1, cfg.block_size)
    with pytest.raises(L.ParrotHipError, match="GPT models"):
        L.generate_speculative(torch.nn.Linear(2, 2), p, 8, 8)
    assert "generate_speculative" in L.__all__


def test_models_outside_the_speculative_step_are_named():
    assert L.GPT(Config.from_name("tiny-llama")).speculative_decode_unsupported() is None
    assert L.GPT(Config.from_name("tiny-falcon-mqa")).speculative_decode_unsupported() is None
    with L.quantization("bnb.int8"):
        int8 = L.GPT(Config.from_name("tiny-llama"))
    assert "LLM.int8" in int8.speculative_decode_unsupported()
    adapter = A.GPT(A.Config.from_name("tiny-llama", adapter_start_layer=1))
    assert "adapter" in adapter.speculative_decode_unsupported()
    wide = Config(**{**name_to_config["tiny-falcon-7b"], "name": "tiny-falcon-7b-wide", "n_head": 18, "n_embd": 18 * 32})
    assert wide.q_per_kv == 18 and "query heads" in L.GPT(wide).speculative_decode_unsupported()
    odd = Config(**{**name_to_config["tiny-llama"], "name": "tiny-llama-hs16", "n_head": 8})
    if odd.head_size not in (32, 64, 128):
        assert "head size" in L.GPT(odd).speculative_decode_unsupported()
    for why, m in (("LLM.int8", int8), ("adapter", adapter)):
        with pytest.raises(L.ParrotHipError, match=why):
            L.generate_speculative(m, torch.arange(4), 8, 8)
