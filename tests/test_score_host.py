"""Scoring, CPU side: the two entry points are declared, exported and bound and refuse bad arguments without a launch; the windows
of perplexity() score every token but the first exactly once; the Python entry points check their inputs before any device work."""
import pytest
import torch

import lit_parrot_amd as L
from lit_parrot_amd import _hip, score
from lit_parrot_amd.config import Config

P = 0x10000  # a 16-byte aligned stand-in pointer: every call below fails its checks before anything is launched


# ---- ABI
def test_entry_points_are_declared_exported_and_bound(hip_lib):
    from test_abi_and_host import declared_functions

    declared = declared_functions()
    for n in ("parrot_token_logprob_rows", "parrot_logprob_advance_rows"):
        assert n in declared and n in _hip.SIGNATURES and hasattr(hip_lib, n)
    assert sorted(_hip.SIGNATURES) == declared, "_hip.py must bind every declared function, and nothing else"
    names = [hip_lib.parrot_kernel_name(i).decode() for i in range(64)]
    assert "token_logprob_rows" in names and "logprob_advance_rows" in names
    assert names.index("logprob_advance_rows") == names.index("token_logprob_rows") + 1 == names.index("?") - 1, "appended last"


def _rows(lib, **kw):
    a = dict(logits=P, V=64, ldl=64, M=3, targets=P, logprob=P, is_greedy=P)
    a.update(kw)
    return lib.parrot_token_logprob_rows(*a.values(), None)


def _advance(lib, **kw):
    a = dict(logits=P, V=64, ldl=64, B=3, tokens=P, ldt=16, pos=P, end=P, logprob=P, is_greedy=P, ldo=16)
    a.update(kw)
    return lib.parrot_logprob_advance_rows(*a.values(), None)


@pytest.mark.parametrize("bad,word", [(dict(logits=None), "null pointer"), (dict(targets=None), "null pointer"), (dict(logprob=None), "null pointer"),
                                      (dict(V=0), "V=0"), (dict(V=-3), "V=-3"), (dict(M=0), "M=0"), (dict(M=-1), "M=-1"),
                                      (dict(ldl=63), "ldl=63")])
def test_token_logprob_rows_rejects_bad_arguments(hip_lib, bad, word):
    assert _rows(hip_lib, **bad) == -1
    err = _hip.last_error()
    assert "token_logprob_rows" in err and word in err, err


@pytest.mark.parametrize("bad,word", [(dict(logits=None), "null pointer"), (dict(tokens=None), "null pointer"), (dict(pos=None), "null pointer"),
                                      (dict(end=None), "null pointer"), (dict(logprob=None), "null pointer"), (dict(is_greedy=None), "null pointer"),
                                      (dict(V=0), "V=0"), (dict(B=0), "B=0"), (dict(B=9), "B=9"), (dict(ldl=63), "ldl=63"),
                                      (dict(ldo=0), "ldo=0"), (dict(ldo=-4), "ldo=-4"), (dict(ldt=0), "ldt=0")])
def test_logprob_advance_rows_rejects_bad_arguments(hip_lib, bad, word):
    assert _advance(hip_lib, **bad) == -1
    err = _hip.last_error()
    assert "logprob_advance_rows" in err and word in err, err


def test_more_rows_than_the_batched_step_are_refused(hip_lib):
    from lit_parrot_amd import ops

    assert _advance(hip_lib, B=ops.GEMV_MAX_ROWS + 1) == -1 and f"1 .. {ops.GEMV_MAX_ROWS}" in _hip.last_error()


# ---- the windows of perplexity()
def check_windows(n, window, stride):
    wins = score.score_windows(n, window, stride)
    scored = []
    for k, (start, stop, first) in enumerate(wins):
        assert 0 <= start < first < stop <= n, (n, window, stride, wins)  # a scored token has the one before it in its pass
        assert stop - start <= window, f"a pass of {stop - start} tokens in a window of {window}"
        assert (start, first) == (0, 1) if k == 0 else first == wins[k - 1][1], "a pass scores from where the last one stopped"
        scored += range(first, stop)
    assert scored == list(range(1, n)), f"n={n} window={window} stride={stride}: scored {scored}"
    return wins


@pytest.mark.parametrize("w", [2, 3, 8, 64])
def test_score_windows_score_every_token_but_the_first_exactly_once(w):
    """The issue's grid: n in {2, 3, window, window + 1, 3 * window - 1} x stride in {1, w // 2, w}.  (Its pair "(1, 1)" as a window
    of ONE token cannot score anything - a scored token needs the one before it in its pass - and raises, below.)"""
    for stride in sorted({1, max(1, w // 2), w}):
        for n in sorted({2, 3, w, w + 1, 3 * w - 1}):
            if n >= 2:
                wins = check_windows(n, w, stride)
                if n <= w:
                    assert wins == [(0, n, 1)]
    # full passes add `stride` scored tokens behind window - stride tokens of context
    assert score.score_windows(10, 4, 2) == [(0, 4, 1), (2, 6, 4), (4, 8, 6), (6, 10, 8)]
    assert score.score_windows(10, 4, 4) == [(0, 4, 1), (3, 7, 4), (6, 10, 7)]  # stride == window: one token of context
    assert score.score_windows(6, 4, 1) == [(0, 4, 1), (1, 5, 4), (2, 6, 5)]


@pytest.mark.parametrize("n,window,stride", [(1, 4, 2), (0, 4, 2), (8, 1, 1), (8, 0, 1), (8, 4, 0), (8, 4, 5), (8, 4, -1), (8.0, 4, 2)])
def test_score_windows_rejects_bad_arguments(n, window, stride):
    with pytest.raises(ValueError, match="score_windows"):
        score.score_windows(n, window, stride)


# ---- input checks, each before any device work (the models live on the CPU)
def tiny():
    return L.GPT(Config.from_name("tiny-llama")).to(torch.bfloat16)


def test_the_entry_points_are_exported():
    for n in ("token_logprobs", "continuation_logprobs", "rank_continuations", "perplexity", "score_windows"):
        assert getattr(L, n) is getattr(score, n) and n in L.__all__


def test_a_model_of_another_class_is_refused():
    lin = torch.nn.Linear(4, 4)
    for call in (lambda: L.token_logprobs(lin, torch.arange(4)), lambda: L.perplexity(lin, torch.arange(4)),
                 lambda: L.continuation_logprobs(lin, torch.arange(4), [torch.arange(2)], 8),
                 lambda: L.rank_continuations(lin, torch.arange(4), [torch.arange(2)], 8)):
        with pytest.raises(L.ParrotHipError, match="GPT models"):
            call()


def test_a_cpu_model_is_refused():
    model = tiny()
    for call in (lambda: L.token_logprobs(model, torch.arange(4)), lambda: L.perplexity(model, torch.arange(4)),
                 lambda: L.continuation_logprobs(model, torch.arange(4), [torch.arange(2)], 8)):
        with pytest.raises(L.ParrotHipError, match="HIP device"):
            call()


def test_token_logprobs_checks_its_tokens():
    model = tiny()
    with pytest.raises(L.ParrotHipError, match="at least 2"):
        L.token_logprobs(model, torch.arange(1))
    with pytest.raises(L.ParrotHipError, match="1-D"):
        L.token_logprobs(model, torch.zeros((2, 4), dtype=torch.int64))
    with pytest.raises(L.ParrotHipError, match="block_size"):
        L.token_logprobs(model, torch.zeros((model.config.block_size + 1,), dtype=torch.int64))


def test_continuations_are_checked():
    model = tiny()
    p = torch.arange(4)
    with pytest.raises(L.ParrotHipError, match="continuation 1 is empty"):
        L.continuation_logprobs(model, p, [torch.arange(2), torch.arange(0)], 8)
    with pytest.raises(L.ParrotHipError, match="1 to 8"):
        L.continuation_logprobs(model, p, [torch.arange(2)] * 9, 8)
    with pytest.raises(L.ParrotHipError, match="1 to 8"):
        L.continuation_logprobs(model, p, [], 8)
    with pytest.raises(L.ParrotHipError, match="1-D"):
        L.continuation_logprobs(model, p, [torch.zeros((1, 2), dtype=torch.int64)], 8)
    with pytest.raises(L.ParrotHipError, match="prompt is empty"):
        L.continuation_logprobs(model, torch.arange(0), [torch.arange(2)], 8)
    with pytest.raises(L.ParrotHipError, match="no sliding window"):  # 4 + 5 > 8: the longest continuation decides
        L.continuation_logprobs(model, p, [torch.arange(2), torch.arange(5)], 8)
    with pytest.raises(L.ParrotHipError, match="HIP device"):  # 4 + 4 == 8 fits: only the device is wrong
        L.continuation_logprobs(model, p, [torch.arange(2), torch.arange(4)], 8)
    with pytest.raises(L.ParrotHipError, match="block_size"):
        L.continuation_logprobs(model, p, [torch.arange(2)], model.config.block_size + 1)


def test_an_int8_model_is_declined_with_the_reason_and_the_way_out():
    with L.quantization("bnb.int8"):
        int8 = L.GPT(Config.from_name("tiny-llama"))
    why = int8.batched_decode_unsupported()
    assert "LLM.int8" in why
    for call in (L.continuation_logprobs, L.rank_continuations):
        with pytest.raises(L.ParrotHipError) as e:
            call(int8, torch.arange(4), [torch.arange(2)], 8)
        assert why in str(e.value) and "token_logprobs" in str(e.value)
