"""Scoring on the HIP path: how likely a model finds GIVEN tokens.

    token_logprobs(model, idx)                          log P(idx[t] | idx[:t]) for t = 1 .. T-1: one prompt pass + one launch
    continuation_logprobs(model, prompt, continuations) the same for up to 8 continuations of ONE prompt, prefilled once
    rank_continuations(...)                             their order by summed (or mean) log-probability
    perplexity(model, tokens)                           exp(mean negative log-likelihood) over strided windows

The logits never leave bf16 and are never copied: ``ops.token_logprob_rows`` reads each row once and writes one float per token
(the torch route, ``F.log_softmax(model(idx).float(), -1).gather(...)``, makes a T x V fp32 copy and three launches).  The
continuations run on the candidates step (generate/base.py::CandidateSession): one shared prompt cache, a short tail cache per
row, ``ops.logprob_advance_rows`` as the step's last launch, captured once and replayed ``max(len) - 1`` times.
"""
import math
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import ops
from ._hip import ParrotHipError
from .generate import base as gb
from .model import GPT

Scores = Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]


def _tokens_1d(fn: str, what: str, t: torch.Tensor, least: int) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.is_floating_point():
        raise ParrotHipError(f"{fn}: {what} must be a 1-D token tensor")
    if t.numel() < least:
        raise ParrotHipError(f"{fn}: {what} is empty" if least == 1 else f"{fn}: {what} holds {t.numel()} tokens; at least {least} are needed")


@torch.no_grad()
def token_logprobs(model: torch.nn.Module, idx: torch.Tensor, *, return_greedy: bool = False) -> Scores:
    """float32 (T-1,): entry t-1 is log P(idx[t] | idx[:t]) under ``model``, computed from the logits ``model(idx[None])`` returns
    (the same pass: T rows from position 0, no cache) in fp32.  With ``return_greedy`` also a bool (T-1,): whether ``idx[t]`` is
    the arg-max of its row (``generate(top_k=1)``'s tie rule: the lowest index).  Every model the prompt path runs."""
    if not isinstance(model, GPT):
        raise ParrotHipError("token_logprobs() drives lit_parrot_amd.GPT models")
    _tokens_1d("token_logprobs", "idx", idx, 2)
    T, c = idx.numel(), model.config
    if T > c.block_size:
        raise ParrotHipError(f"token_logprobs: {T} tokens exceed block_size={c.block_size}; score windows of it (perplexity())")
    dev = gb._cuda_device("token_logprobs", model)
    idx = idx.to(device=dev, dtype=torch.int64).contiguous()
    if model.rope_cache is None:
        model.rope_cache = model.build_rope_cache(idx)
    # GPT.forward's pass without a cache: all T rows of lm_head, one scratch K/V pair that serves every layer in turn
    ws = model.workspace(T, dev)
    scratch = tuple(torch.empty((c.n_query_groups, T, c.head_size), dtype=torch.bfloat16, device=dev) for _ in range(2))
    logits = model.run_rows(ws, idx, None, ws.zero_pos, T, [scratch] * c.n_layer, model.rope_cache, pos_is_zero=True)
    logprob = torch.empty((T - 1,), dtype=torch.float32, device=dev)
    greedy = torch.empty((T - 1,), dtype=torch.int32, device=dev) if return_greedy else None
    ops.token_logprob_rows(logits[:T - 1], idx[1:], logprob, greedy)
    return (logprob, greedy.bool()) if return_greedy else logprob


@torch.no_grad()
def continuation_logprobs(model: torch.nn.Module, prompt: torch.Tensor, continuations: Sequence[torch.Tensor], max_seq_length: int, *,
                          return_greedy: bool = False) -> Union[List[torch.Tensor], Tuple[List[torch.Tensor], List[torch.Tensor]]]:
    """For each of 1 to 8 ``continuations`` (non-empty 1-D token tensors, lengths may differ) a float32 (len_b,) tensor: entry i is
    log P(continuation[i] | prompt, continuation[:i]).  The prompt is prefilled once; all rows attend to its one cache.  With
    ``return_greedy`` also the bool tensors that say where a continuation's token is the arg-max (all True: the continuation is
    what ``generate(top_k=1)`` would have produced).  ``max_seq_length`` is the window of the cache; it must hold the prompt and
    the longest continuation (no sliding window, as in generate_candidates)."""
    fn = "continuation_logprobs"
    if not isinstance(model, GPT):
        raise ParrotHipError(f"{fn}() drives lit_parrot_amd.GPT models")
    _tokens_1d(fn, "the prompt", prompt, 1)
    continuations = list(continuations)
    if not 1 <= len(continuations) <= ops.GEMV_MAX_ROWS:
        raise ParrotHipError(f"{fn}: {len(continuations)} continuations; the scoring step takes 1 to {ops.GEMV_MAX_ROWS} rows")
    for b, cont in enumerate(continuations):
        _tokens_1d(fn, f"continuation {b}", cont, 1)
    why = model.batched_decode_unsupported()
    if why is not None:
        raise ParrotHipError(f"{fn}: {why}; use token_logprobs() on the concatenation of the prompt and each continuation")
    T, longest = prompt.numel(), max(c.numel() for c in continuations)
    block_size = model.config.block_size
    if max_seq_length > block_size:
        raise ParrotHipError(f"{fn}: max_seq_length={max_seq_length} exceeds block_size={block_size}: positions past the RoPE tables")
    if T + longest > max_seq_length:
        raise ParrotHipError(f"{fn}: the prompt ({T} tokens) and the longest continuation ({longest}) exceed max_seq_length="
                             f"{max_seq_length}: the shared prompt cache and the rows' own caches are addressed by position (no "
                             "sliding window)")
    gb._cuda_device(fn, model)
    n = len(continuations)
    tail = gb.candidate_tail_slots(T + longest, T)
    # (a captured step keeps the attention launches it was captured with: the switch is part of the key)
    key = ("score", n, max_seq_length, tail, bool(ops.CANDIDATES_SHARE_LOADS))
    sess = gb._cached_session(model, key, max_seq_length, lambda: gb.ScoringSession(model, n, max_seq_length, tail))
    dev = sess.device
    sess.prefill(prompt.to(device=dev, dtype=torch.int64), [c.to(device=dev, dtype=torch.int64) for c in continuations])
    sess.capture()
    sess.score_first()
    for _ in range(longest - 1):
        sess.step()
    logprobs = [sess.logprob[b, T:T + c.numel()].clone() for b, c in enumerate(continuations)]
    if not return_greedy:
        return logprobs
    return logprobs, [sess.is_greedy[b, T:T + c.numel()].bool() for b, c in enumerate(continuations)]


def rank_continuations(model: torch.nn.Module, prompt: torch.Tensor, continuations: Sequence[torch.Tensor], max_seq_length: int, *,
                       length_normalize: bool = False) -> Tuple[List[int], torch.Tensor]:
    """(order, totals): ``totals[b]`` (float32, on the model's device) is continuation b's summed log-probability behind ``prompt``
    - its mean with ``length_normalize`` - and ``order`` lists the continuations from the most to the least likely."""
    logprobs = continuation_logprobs(model, prompt, continuations, max_seq_length)
    totals = torch.stack([lp.mean() if length_normalize else lp.sum() for lp in logprobs])
    return torch.argsort(totals, descending=True, stable=True).tolist(), totals


def score_windows(n_tokens: int, window: int, stride: int) -> List[Tuple[int, int, int]]:
    """The passes that score tokens 1 .. n_tokens-1 exactly once with at most ``window`` tokens per pass: a list of
    (start, stop, first_scored) - the pass runs tokens[start:stop] and its scores of the positions first_scored .. stop-1 count.
    The first pass starts at 0 and scores from 1; each later one scores from where the last stopped, behind ``window - stride``
    tokens of context (at least the one token before it), so a full pass adds ``stride`` scored tokens (``window - 1`` when
    ``stride == window``).  A window needs two tokens: the scored one and the one before it."""
    if not (isinstance(n_tokens, int) and isinstance(window, int) and isinstance(stride, int)):
        raise ValueError("score_windows: n_tokens, window and stride are integers")
    if n_tokens < 2:
        raise ValueError(f"score_windows: n_tokens={n_tokens}; two tokens are the least that can be scored")
    if window < 2:
        raise ValueError(f"score_windows: window={window}; a window holds a scored token and at least the one before it")
    if not 1 <= stride <= window:
        raise ValueError(f"score_windows: stride={stride} outside 1 .. window={window}")
    context = max(1, window - stride)
    out = [(0, min(window, n_tokens), 1)]
    while out[-1][1] < n_tokens:
        first = out[-1][1]
        start = first - context
        out.append((start, min(start + window, n_tokens), first))
    return out


def perplexity(model: torch.nn.Module, tokens: torch.Tensor, *, window: Optional[int] = None,
               stride: Optional[int] = None) -> Tuple[float, float, int]:
    """(ppl, nll_sum, n_scored) of a token sequence of any length: ``token_logprobs`` over the passes of ``score_windows`` (defaults:
    ``window = block_size``, ``stride = window // 2``); every token but the first is scored once, ``ppl = exp(nll_sum / n_scored)``."""
    if not isinstance(model, GPT):
        raise ParrotHipError("perplexity() drives lit_parrot_amd.GPT models")
    _tokens_1d("perplexity", "tokens", tokens, 2)
    window = model.config.block_size if window is None else window
    stride = max(1, window // 2) if stride is None else stride
    if window > model.config.block_size:
        raise ParrotHipError(f"perplexity: window={window} exceeds block_size={model.config.block_size}")
    total = None
    for start, stop, first in score_windows(tokens.numel(), window, stride):
        part = token_logprobs(model, tokens[start:stop])[first - start - 1:].double().sum()
        total = part if total is None else total + part
    n_scored = tokens.numel() - 1
    nll = -float(total)  # the one host read
    return math.exp(nll / n_scored), nll, n_scored
