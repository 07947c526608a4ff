"""The decode loop: ``generate()`` with the reference's signature (generate/base.py:92-159), hipGraph-captured.

Reference loop per token: index_select the new token, ``model(x, max_seq_length, input_pos)``, divide by the
temperature, optional top-k crop, softmax, multinomial, out-of-place ``index_copy`` into the token buffer and, when
``eos_id`` is given, a host sync to compare (:131-157).  Here the loop state lives on the device:

    tokens  int64[max_returned_tokens]   the prompt, then every sampled token
    pos     int32[1]                     position of the row being decoded

and one decode step — embedding of ``tokens[pos]``, every block, final norm, lm_head and, for greedy decoding, the
arg-max that writes ``tokens[pos+1]`` and advances ``pos`` — is a fixed launch sequence captured ONCE per
(model, max_seq_length, sampling parameters) in a hipGraph and replayed per token.  Greedy decoding (``top_k == 1``, which
is how the reference spells it: there is no argmax branch) never touches the host inside the loop unless ``eos_id`` is set.
With ``top_k != 1`` (the reference's default call: temperature 0.8, top_k 200) the sampling step is inside the graph too:
torch draws the Exponential(1) noise that ``torch.multinomial`` draws internally (``noise.exponential_(1)``, graph-safe
Philox: the same generator consumption) and ``parrot_topk_sample`` does the rest - temperature, top-k crop, softmax,
arg-max of probs / noise - with the arithmetic of the torch device ops the reference runs (:139-144), so the same torch seed
draws the same tokens as those ops do on this device (tests/test_model_gpu.py::test_sampling_in_the_graph_draws_the_tokens_of_the_torch_ops).

The prompt is prefilled in one multi-row pass (same kernels, M = T rows) that computes only the last row of lm_head
(the reference computes all T rows and discards T-1 of them, :135-136).
"""
import contextlib
import gc
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch

from .. import ops
from .._hip import ParrotHipError
from ..model import GPT, Rows
from ..weights import weights_generation


@contextlib.contextmanager
def _capturing(graph: "torch.cuda.CUDAGraph"):
    """``torch.cuda.graph(graph)`` with Python's cyclic garbage collector out of the way.  A model and its cached sessions refer
    to each other (``model._decode_sessions`` <-> ``session.model``), so a dropped model leaves its captured graphs and their memory
    pools to the collector; a collection that falls INSIDE a capture destroys them there, which the runtime answers with an error
    in a destructor: the process aborts.  (torch no longer collects on entering ``torch.cuda.graph``.)  The collector stays off
    until the capture has ended; the dead cycles go with the next regular collection."""
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            yield
    finally:
        if was_enabled:
            gc.enable()


# ------------------------------------------------------------------------------------------------ what every session shares
def _check_args(fn: str, model: torch.nn.Module, lengths: Sequence[int], max_returned_tokens: int, max_seq_length: int,
                length_first: bool = False) -> None:
    """The model class and generate()'s checks (reference generate/base.py:118-127) for a prompt of each of ``lengths`` tokens.
    ``length_first``: generate()'s own order, whose first assert - the reference's first line - comes before the model's class."""
    if length_first:
        assert max_returned_tokens > lengths[0]
    if not isinstance(model, GPT):
        raise ParrotHipError(f"{fn}() drives lit_parrot_amd.GPT models")
    block_size = model.config.block_size
    for T in lengths:
        assert max_returned_tokens > T
        assert max_seq_length <= block_size
        if max_returned_tokens > block_size:
            # positions index the RoPE tables (block_size rows); the reference fails at rope.index_select in this case
            # (lit_gpt/model.py:88) - here the kernels would read past the tables on the device
            raise ParrotHipError(f"max_returned_tokens={max_returned_tokens} exceeds block_size={block_size}: "
                                 "positions past the RoPE tables")
        assert max_seq_length >= T, f"Cannot forward sequence of length {T}, max seq length is only {max_seq_length}"


def _cuda_device(fn: str, model: GPT) -> torch.device:
    dev = model.transformer.wte.weight.device
    if dev.type != "cuda":
        raise ParrotHipError(f"{fn}() runs on the HIP device only: move the model to cuda (no CPU fallback)")
    return dev


def _run_prompt(model: GPT, tokens: torch.Tensor, T: int, zero_pos: torch.Tensor, S: int, caches: List) -> torch.Tensor:
    """``tokens[:T]`` through the multi-row path (M = T rows) into ``caches`` (one ``(k, v)`` of (n_groups, S, hs) per layer);
    returns the last row's logits (1, V).  ``zero_pos``: an int32[1] on the device that holds 0."""
    ws = model.workspace(T, tokens.device, 1)
    # the prompt starts at position 0: its attention may take the MFMA kernel (no ring wrap in the call)
    return model.run_rows(ws, tokens, None, zero_pos, S, caches, model.rope_cache, pos_is_zero=True)


def _capture(step: Callable[[], object], written: Sequence[torch.Tensor], device: torch.device, draws_rng: bool) -> "torch.cuda.CUDAGraph":
    """The graph of ``step()``: warmed up outside the capture on a side stream (lazy W4K repacks, workspace allocations), then
    captured.  ``written`` names the loop state the step writes; it is put back after the warm-up and after the capture (which
    only records the launches), so the caller's state is what it was.  A sampling step (``draws_rng``) draws from torch's
    generator: its state is put back too, so the warm-up does not use up draws of the caller's seed."""
    kept = [t.clone() for t in written]
    rng = torch.cuda.get_rng_state(device) if draws_rng else None

    def restore() -> None:
        for t, t0 in zip(written, kept):
            t.copy_(t0)

    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)
    restore()
    graph = torch.cuda.CUDAGraph()
    with _capturing(graph):
        step()
    restore()
    if rng is not None:
        torch.cuda.set_rng_state(rng, device)
    return graph


class _Session:
    """The construction and the capture the sessions share.  A session adds its buffers, ``_step`` (the launch sequence that
    gets captured) and, where the step writes something else than tokens, pos and the K/V caches, ``_written``."""

    def _open(self, fn: str, model: GPT, max_seq_length: int, tokens_shape: Tuple[int, ...], kv_batch: int, use_graph: bool) -> None:
        """The device (``fn``: the entry point an error names), the token buffer, the model's RoPE tables and its ``kv_caches``
        with batch ``kv_batch`` and a window of ``max_seq_length`` slots, rebuilt when they are anything else."""
        self.model, self.S, self.use_graph = model, max_seq_length, use_graph
        # the state of the weights the session's buffers, images and captured launches belong to: stale under any other
        self.weights_generation = weights_generation(model)
        self.device = _cuda_device(fn, model)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.tokens = torch.zeros(tokens_shape, dtype=torch.int64, device=self.device)
        if model.rope_cache is None:
            model.rope_cache = model.build_rope_cache(self.tokens)
        kv = model.kv_caches
        if not kv or kv[0][0].size(2) != max_seq_length or kv[0][0].size(0) != kv_batch:
            model.kv_caches = model.build_kv_caches(self.tokens.new_empty((kv_batch, 0)), max_seq_length, model.rope_cache[0].size(-1))

    def _drop_reference_weights(self) -> None:
        """One resident image of the int4 weights: W4K (the multi-launch step's and every prompt's format; the engine keeps
        its E4 copy beside it).  The reference-layout buffers are released; state_dict() / get_weight() rebuild them exactly."""
        if RELEASE_REFERENCE_BUFFERS:
            for m in self.model.modules():
                release = getattr(m, "release_reference", None)
                if release is not None:
                    release()

    def _written(self) -> List[torch.Tensor]:
        return [self.tokens, self.pos] + [t for kv in self.caches for t in kv]

    def capture(self) -> None:
        if self.graph is None and self.use_graph:
            self.graph = _capture(self._step, self._written(), self.device, self.sampler is not None)


class DecodeSession(_Session):
    """Static buffers + captured graph of the single-token step for one (model, max_seq_length, greedy) choice."""

    def __init__(self, model: GPT, max_seq_length: int, max_tokens: int, greedy: bool, use_graph: bool = True,
                 engine: Optional[bool] = None, sampler: Optional[Tuple[float, Optional[int]]] = None) -> None:
        self._open("generate", model, max_seq_length, (max_tokens + 1,), 1, use_graph)
        self.greedy = greedy
        # (temperature, top_k) of the in-graph sampling step when not greedy; None: the step ends at the logits
        self.sampler = None if greedy else sampler
        self.noise: Optional[torch.Tensor] = None
        self.pos = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self.ws = model.workspace(1, self.device, 1)
        self.caches = [(k[0], v[0]) for k, v in model.kv_caches]
        # one launch per token when the model fits the stream engine (csrc/engine.hip), else 5 launches per block
        from ..engine import StreamEngine

        self.eng = None
        if engine is None:
            engine = ENGINE_DEFAULT
        if engine == "auto":
            engine = StreamEngine.faster_than_multi_launch(model, max_seq_length, ENGINE_AUTO_MIN_WINDOW)
        if engine and StreamEngine.supported(model) is None:
            self.eng = StreamEngine(model, self.tokens, self.pos, self.caches, max_seq_length, greedy)
        self._drop_reference_weights()

    # one decode step = the launch sequence that gets captured
    def _step(self) -> None:
        if self.eng is not None:
            logits = self.eng.step()  # embedding .. lm_head (.. arg-max + advance when greedy) in one launch
        else:
            logits = self.model.run_rows(self.ws, self.tokens, self.pos, self.pos, self.S, self.caches, self.model.rope_cache)
            if self.greedy:
                ops.argmax_advance(logits, self.tokens, self.pos)
        if self.sampler is not None:
            self.sample(logits)

    def sample(self, logits: torch.Tensor) -> None:
        """``tokens[pos + 1]`` = the next token drawn from ``logits`` (the row at ``pos``), ``pos += 1``: arg-max when greedy,
        else the reference's temperature / top-k / softmax / multinomial step (generate/base.py:136-153) as one torch draw of
        the noise + one launch (ops.topk_sample)."""
        if self.greedy:
            ops.argmax_advance(logits, self.tokens, self.pos)
            return
        if self.sampler is None:
            raise ParrotHipError("this session was built without sampling parameters")
        if self.noise is None:
            self.noise = torch.empty((logits.numel(),), dtype=torch.bfloat16, device=self.device)
        self.noise.exponential_(1)  # what torch.multinomial draws internally: same generator consumption
        ops.topk_sample(logits.view(-1), self.sampler[0], self.sampler[1], self.noise, self.tokens, self.pos)

    def prefill(self, prompt: torch.Tensor) -> torch.Tensor:
        """Run the T prompt rows, leave ``pos`` = T-1 and return the logits of the last prompt token."""
        T = prompt.numel()
        self.tokens[:T].copy_(prompt)
        self.pos.zero_()
        logits = _run_prompt(self.model, self.tokens, T, self.pos, self.S, self.caches)
        self.pos.fill_(T - 1)
        return logits

    def step(self) -> torch.Tensor:
        """Decode the token at ``pos``; returns the logits buffer (V,) of that step."""
        if self.graph is not None:
            self.graph.replay()
        else:
            self._step()
        return self.eng.logits[0] if self.eng is not None else self.ws.logits[0]

    def check_error(self) -> None:
        """Host-side check (syncs) of the executor's in-launch waits: the stream engine's error word.  A step whose waits gave
        up decoded garbage: fail loudly, never report its tokens or its speed."""
        if self.eng is not None:
            self.eng.check_error()


# The one-launch stream engine (engine.py) for the models it is built for (Llama-2 7B family, int4 g128).  Measured on
# Llama-2-7B int4: its token time barely moves with the context (K/V rows stream through the same LDS ring
# as the weights, on all 256 CUs), the multi-launch step's grows; they cross below 1k keys.  With bf16 weights (two loader
# waves, a parallel-residual block with three hand-offs instead of five) it is ahead at every window: StableLM-3B 752 vs
# 654 tokens/s behind a 512-token prompt.  "auto" picks by weight format and window size.
ENGINE_DEFAULT = "auto"
ENGINE_AUTO_MIN_WINDOW = 1024
# A decode session frees the reference-layout copy of every GPTQ int4 Linear (quantize/gptq.py): Llama-2-7B
# int4 then holds 3.5 GB of weights instead of 7 (multi-launch step) and Falcon-40B int4 44 GB instead of 66 (engine: W4K + E4).
RELEASE_REFERENCE_BUFFERS = True
MAX_SESSIONS_PER_MODEL = 4  # captured steps kept per model (keyed by window, greedy / sampling parameters), least recently used first out


def _cached_session(model: GPT, key: Tuple, max_tokens: int, make: Callable):
    """The session under ``key`` in the model's LRU cache of captured steps (single-sequence and batched sessions alike), rebuilt
    by ``make()`` when it is missing, too short, no longer holds the model's current KV caches, or was built from other weights."""
    cache: Dict[Tuple, object] = model.__dict__.setdefault("_decode_sessions", {})
    sess = cache.get(key)
    stale = (
        sess is None
        or sess.tokens.shape[-1] < max_tokens + 1
        or not model.kv_caches
        or model.kv_caches[0][0].data_ptr() != sess.caches[0][0].data_ptr()
        or sess.weights_generation != weights_generation(model)
    )
    if stale:
        cache.pop(key, None)
        sess = None  # (the old session's buffers go before the new one's are allocated)
        while len(cache) >= MAX_SESSIONS_PER_MODEL:  # a caller that varies temperature / top_k per request must not pile up graphs
            cache.pop(next(iter(cache)))
        sess = make()
    else:
        cache.pop(key)  # (re-inserted below: the dict's order is the order of last use)
    cache[key] = sess
    return sess


def _session(model: GPT, max_seq_length: int, max_tokens: int, greedy: bool,
             sampler: Optional[Tuple[float, Optional[int]]] = None) -> DecodeSession:
    sampler = None if greedy else sampler
    return _cached_session(model, (max_seq_length, greedy, sampler), max_tokens,
                           lambda: DecodeSession(model, max_seq_length, max_tokens, greedy, sampler=sampler))


@torch.no_grad()
def generate(
    model: torch.nn.Module,
    idx: torch.Tensor,
    max_returned_tokens: int,
    max_seq_length: int,
    *,
    temperature: float = 1.0,
    top_k: Optional[int] = None,
    eos_id: Optional[int] = None,
) -> torch.Tensor:
    """Continue the prompt ``idx`` (T,) up to ``max_returned_tokens`` tokens; same arguments and return value as the
    reference (generate/base.py:93-159): a 1-D tensor holding the prompt followed by the generated tokens, cut after
    ``eos_id`` when it is produced.  Call ``model.reset_cache()`` between prompts like the reference's ``main``."""
    T = idx.size(0)
    _check_args("generate", model, [T], max_returned_tokens, max_seq_length, length_first=True)
    dtype = idx.dtype
    greedy = top_k == 1 and temperature > 0
    sess = _session(model, max_seq_length, max_returned_tokens, greedy, (float(temperature), top_k))
    logits = sess.prefill(idx.to(device=sess.device, dtype=torch.int64))
    sess.capture()

    n_new = max_returned_tokens - T
    for i in range(n_new):
        # `logits` belong to the row at `pos` = T-1+i; sample tokens[T+i] from them and advance `pos`: the first token here,
        # the later ones inside the captured step (arg-max, or the noise draw + parrot_topk_sample)
        if i == 0:
            sess.sample(logits)
        if eos_id is not None and int(sess.tokens[T + i]) == eos_id:  # host sync, as in the reference (:156-157)
            # the reference returns idx[:input_pos], which stops BEFORE the eos token despite its comment
            break
        if i + 1 < n_new:
            logits = sess.step()
    else:
        i = n_new
    out = sess.tokens[: T + i].to(dtype).clone()
    sess.check_error()  # a bounded in-launch wait gave up (e.g. fewer CUs than resident workgroups): fail loudly
    return out


# ------------------------------------------------------------------------------------------------ batched decode
class BatchDecodeSession(_Session):
    """Static buffers + captured graph of the batched step: B independent sequences (1 <= B <= 8), one row each.

        tokens  int64[B][L]   row b: prompt b, then its sampled tokens
        pos     int32[B]      position of row b's token being decoded
        end     int32[B]      row b stops before position end[b] (max_returned_tokens)

    One step embeds ``tokens[b, pos[b]]`` for every row, runs every block over the B rows (each Linear's weights are streamed once
    per 4 rows - int4 / NF4 - or per 2 rows - bf16 -, one attention launch per layer for all rows, each row in its own cache slice
    ``kv_caches[i][0][b]``), lm_head on all rows and one sampling launch that advances every row that is not frozen (at ``end``
    or after ``eos_id``).  The stream engine is batch-1: this step is always the multi-launch one."""

    def __init__(self, model: GPT, B: int, max_seq_length: int, max_tokens: int, greedy: bool,
                 sampler: Optional[Tuple[float, Optional[int]]] = None, eos_id: int = -1, use_graph: bool = True) -> None:
        self._open_rows("generate_batch", model, B, max_seq_length, max_tokens + 1, B, greedy, sampler, eos_id, use_graph,
                        Rows.SEQUENCES)
        self.caches = list(model.kv_caches)  # (B, n_groups, S, hs) per layer
        self._drop_reference_weights()

    def _open_rows(self, fn: str, model: GPT, B: int, max_seq_length: int, length: int, kv_batch: int, greedy: bool,
                   sampler: Optional[Tuple[float, Optional[int]]], eos_id: int, use_graph: bool, rows: Rows) -> None:
        """The buffers of a step over B rows, each with a token buffer of ``length``; ``rows``: what the rows are to the workspace."""
        self._open(fn, model, max_seq_length, (B, length), kv_batch, use_graph)
        self.B, self.greedy, self.eos_id = B, greedy, eos_id
        self.sampler = None if greedy else sampler
        dev = self.device
        self.pos = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.end = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.zero_pos = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.ws = model.workspace(B, dev, B, rows)
        V = model.config.padded_vocab_size
        self.first_logits = torch.empty((B, V), dtype=torch.bfloat16, device=dev)  # the prompts' last rows
        self.noise = torch.empty((B, V), dtype=torch.bfloat16, device=dev) if self.sampler is not None else None

    def sample(self, logits: torch.Tensor, eos_id: int) -> None:
        """Row b: ``tokens[b, pos[b] + 1]`` = the token drawn from ``logits[b]``, ``pos[b] += 1``, unless the row is frozen.  The noise
        of all rows is drawn by one ``exponential_`` call (B = 1 consumes the generator as generate() does)."""
        if self.greedy:
            ops.argmax_advance_rows(logits, self.tokens, self.pos, self.end, eos_id)
            return
        self.noise.exponential_(1)
        ops.topk_sample_rows(logits, self.sampler[0], self.sampler[1], self.noise, self.tokens, self.pos, self.end, eos_id)

    def _step(self) -> None:
        logits = self.model.run_rows(self.ws, self.tokens, self.pos, self.pos, self.S, self.caches, self.model.rope_cache)
        self.sample(logits, self.eos_id)

    def prefill(self, prompts: Sequence[torch.Tensor], max_returned_tokens: int) -> None:
        """Each prompt through the multi-row path into its own cache slice; leaves pos[b] = T_b - 1 and the last rows' logits in
        ``first_logits``."""
        for b, p in enumerate(prompts):
            T = p.numel()
            self.tokens[b, :T].copy_(p)
            logits = _run_prompt(self.model, self.tokens[b], T, self.zero_pos, self.S, [(k[b], v[b]) for k, v in self.caches])
            self.first_logits[b].copy_(logits[0])
        self.pos.copy_(torch.tensor([p.numel() - 1 for p in prompts], dtype=torch.int32))
        self.end.fill_(max_returned_tokens)

    def step(self) -> None:
        if self.graph is not None:
            self.graph.replay()
        else:
            self._step()

    def all_frozen(self) -> bool:
        """One host read of every row's position and last token: True once no row can advance (at ``end`` or after ``eos_id``)."""
        pos = self.pos.long()
        state = torch.stack([pos, self.tokens.gather(1, pos.view(-1, 1)).view(-1), self.end.long()]).cpu()
        return bool(((state[0] + 1 >= state[2]) | (state[1] == self.eos_id)).all())


def _decode_rows(sess: BatchDecodeSession, prompts: Sequence[torch.Tensor], max_returned_tokens: int,
                 eos_id: Optional[int]) -> List[torch.Tensor]:
    """The loop behind a prefilled session of rows: every row, its prompt included, cut at its position and before ``eos_id``."""
    sess.capture()
    sess.sample(sess.first_logits, -1)  # the first token of every row is drawn whatever the prompt's last token is
    for _ in range(max_returned_tokens - min(p.numel() for p in prompts) - 1):
        if eos_id is not None and sess.all_frozen():  # host sync, as in generate()
            break
        sess.step()
    tokens, pos = sess.tokens.cpu(), sess.pos.cpu()
    out = []
    for b, p in enumerate(prompts):
        n = int(pos[b]) + 1
        if eos_id is not None and n > p.numel() and int(tokens[b, n - 1]) == int(eos_id):
            n -= 1  # the reference returns idx[:input_pos]: the eos token is not part of the result
        out.append(sess.tokens[b, :n].to(p.dtype).clone())
    return out


def _batch_prompts(prompts: Union[torch.Tensor, Sequence[torch.Tensor]]) -> List[torch.Tensor]:
    if isinstance(prompts, torch.Tensor):
        if prompts.dim() != 2:
            raise ParrotHipError(f"generate_batch: a tensor of prompts must be (B, T), got shape {tuple(prompts.shape)}")
        prompts = list(prompts)
    prompts = list(prompts)
    for b, p in enumerate(prompts):
        if not isinstance(p, torch.Tensor) or p.dim() != 1:
            raise ParrotHipError(f"generate_batch: prompt {b} must be a 1-D token tensor")
        if p.numel() == 0:
            raise ParrotHipError(f"generate_batch: prompt {b} is empty")
    if not 1 <= len(prompts) <= ops.GEMV_MAX_ROWS:
        raise ParrotHipError(f"generate_batch: {len(prompts)} prompts; the batched step takes 1 to {ops.GEMV_MAX_ROWS} sequences")
    return prompts


@torch.no_grad()
def generate_batch(
    model: torch.nn.Module,
    prompts: Union[torch.Tensor, Sequence[torch.Tensor]],
    max_returned_tokens: int,
    max_seq_length: int,
    *,
    temperature: float = 1.0,
    top_k: Optional[int] = None,
    eos_id: Optional[int] = None,
) -> List[torch.Tensor]:
    """``generate()`` for up to 8 prompts at once: row b of the result is what ``generate(model, prompts[b], ...)`` returns - the
    prompt followed by its generated tokens, at most ``max_returned_tokens`` long, cut before ``eos_id``.  ``prompts``: a list
    of 1-D token tensors (lengths may differ) or a (B, T) tensor.  Every step decodes all rows in one captured batched pass
    (BatchDecodeSession), so the weights are read once per pass instead of once per sequence."""
    prompts = _batch_prompts(prompts)
    _check_args("generate_batch", model, [p.numel() for p in prompts], max_returned_tokens, max_seq_length)  # row by row
    _cuda_device("generate_batch", model)
    why = model.batched_decode_unsupported()
    if why is not None:
        raise ParrotHipError(f"generate_batch: {why}; use generate() per prompt")
    B = len(prompts)
    greedy = top_k == 1 and temperature > 0
    sampler = None if greedy else (float(temperature), top_k)
    eos = -1 if eos_id is None else int(eos_id)
    sess = _cached_session(model, ("batch", B, max_seq_length, greedy, sampler, eos), max_returned_tokens,
                           lambda: BatchDecodeSession(model, B, max_seq_length, max_returned_tokens, greedy, sampler, eos))
    sess.prefill([p.to(device=sess.device, dtype=torch.int64) for p in prompts], max_returned_tokens)
    return _decode_rows(sess, prompts, max_returned_tokens, eos_id)


# ------------------------------------------------------------------------------------------------ candidates of one prompt
TAIL_BUCKET = 64  # a candidate's own cache holds the generated tokens only, rounded up to this many slots


def candidate_tail_slots(max_returned_tokens: int, T: int) -> int:
    """Slots of a candidate's tail cache: ``max_returned_tokens - T`` rounded up to a multiple of TAIL_BUCKET (the session key)."""
    return -(-(max_returned_tokens - T) // TAIL_BUCKET) * TAIL_BUCKET


def shared_splits(S: int, nsplit: int, T: int) -> List[int]:
    """The splits of a window of ``S`` slots in ``nsplit`` parts whose keys all lie inside a prompt of ``T`` tokens: the same for
    every candidate, so the attention serves them with workgroups that load each K/V row once for several rows
    (csrc/attn.hip, attn_prefix_decode_kernel).  ``per = ceil(S / nsplit)``; split j is shared when ``(j + 1) * per <= T``; never
    the last one, which ends at S > pos >= T."""
    per = -(-S // nsplit)
    T = min(max(T, 0), S)
    return [j for j in range(nsplit - 1) if (j + 1) * per <= T]


def ticket_arrivals(S: int, nsplit: int, T: int, share: bool = True) -> Tuple[int, int]:
    """Arrivals at one (row, group, chunk) ticket from the shared-load launch and from the per-row launch: together always
    ``nsplit``, and the per-row launch, which merges, always makes the last one."""
    n = len(shared_splits(S, nsplit, T)) if share and nsplit > 1 else 0
    return n, nsplit - n


class CandidateSession(BatchDecodeSession):
    """Static buffers + captured graph of the candidates step: n rows (1 <= n <= 8) that continue ONE prompt.

        tokens      int64[n][L]   every row: the prompt, then the row's sampled tokens
        pos, end    int32[n]      as in BatchDecodeSession
        prefix_len  int32[1]      the prompt length T, on the device: one captured step serves every prompt whose tail fits
        caches      the model's batch-1 ``kv_caches`` (n_groups, S, hs): the prompt at slots 0 .. T-1, prefilled ONCE
        tails       (n, n_groups, S_tail, hs) per layer, K and V: row b's position p >= T at ``tail[b][:, p - T]``

    The step is BatchDecodeSession's with ``ops.attn_fused_decode_prefix`` as the attention, which computes every row bit for bit
    as ``attn_fused_decode_rows`` does on n full caches that each hold a copy of the prompt: ``generate_candidates`` returns
    ``generate_batch(model, [idx] * n, ...)``'s tokens with one prefill and one copy of the prompt K/V.  Positions address both
    caches directly, so the window must hold every position (no ring wrap)."""

    def __init__(self, model: GPT, n: int, max_seq_length: int, tail_slots: int, greedy: bool,
                 sampler: Optional[Tuple[float, Optional[int]]] = None, eos_id: int = -1, use_graph: bool = True) -> None:
        # (no position reaches the window's end: the token buffer is as long as the window)
        self._open_rows("generate_candidates", model, n, max_seq_length, max_seq_length + 1, 1, greedy, sampler, eos_id, use_graph,
                        Rows.SHARED_PREFIX)
        self.S_tail = tail_slots
        dev, c = self.device, model.config
        self.prefix_len = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.caches = [(k[0], v[0]) for k, v in model.kv_caches]  # the shared prompt cache: (n_groups, S, hs) per layer
        shape = (n, c.n_query_groups, tail_slots, c.head_size)
        self.tails = [(torch.zeros(shape, dtype=torch.bfloat16, device=dev), torch.zeros(shape, dtype=torch.bfloat16, device=dev))
                      for _ in range(c.n_layer)]
        self.prefix_caches = [(ops.PrefixCache(k, tk, self.prefix_len), ops.PrefixCache(v, tv, self.prefix_len))
                              for (k, v), (tk, tv) in zip(self.caches, self.tails)]
        self._drop_reference_weights()

    def kv_bytes(self) -> int:
        """Bytes of K/V this session holds: the shared cache once and the n tails."""
        return sum(t.numel() * t.element_size() for pair in self.caches + self.tails for t in pair)

    def _step(self) -> None:
        logits = self.model.run_rows(self.ws, self.tokens, self.pos, self.pos, self.S, self.prefix_caches, self.model.rope_cache)
        self.sample(logits, self.eos_id)

    def _written(self) -> List[torch.Tensor]:
        # The step writes tokens, pos and tail slots only, never the shared cache.  A tail slot is always written by its own step
        # before a later step reads it, so the tokens do not need the tails put back; they are, so that capture() leaves no trace
        # (its warm-up at pos = T - 1 writes slot 0 of every tail)
        return [self.tokens, self.pos] + [t for kv in self.tails for t in kv]

    def prefill(self, prompt: torch.Tensor, max_returned_tokens: int) -> None:
        """The prompt ONCE through the multi-row path into the shared cache; every row starts from its last row's logits at
        pos = T - 1."""
        T = prompt.numel()
        self.tokens[:, :T] = prompt
        logits = _run_prompt(self.model, self.tokens[0], T, self.zero_pos, self.S, self.caches)
        self.first_logits.copy_(logits[:1].expand(self.B, -1))
        self.pos.fill_(T - 1)
        self.end.fill_(max_returned_tokens)
        self.prefix_len.fill_(T)


@torch.no_grad()
def generate_candidates(
    model: torch.nn.Module,
    idx: torch.Tensor,
    n: int,
    max_returned_tokens: int,
    max_seq_length: int,
    *,
    temperature: float = 1.0,
    top_k: Optional[int] = None,
    eos_id: Optional[int] = None,
) -> List[torch.Tensor]:
    """``n`` samples of ONE prompt (the reference scripts' ``for _ in range(return_candidates): generate(...)``): exactly the tokens
    of ``generate_batch(model, [idx] * n, max_returned_tokens, max_seq_length, ...)`` under the same torch seed - row b draws from
    its own noise row, greedy rows equal ``generate()`` - with the prompt prefilled once and its K/V stored once: all rows attend to
    the one shared prompt cache and each keeps a short cache of its own for the tokens it generates (CandidateSession)."""
    if not isinstance(idx, torch.Tensor) or idx.dim() != 1 or idx.numel() == 0:
        raise ParrotHipError("generate_candidates: the prompt must be a non-empty 1-D token tensor")
    T = idx.numel()
    _check_args("generate_candidates", model, [T], max_returned_tokens, max_seq_length)
    if not isinstance(n, int) or not 1 <= n <= ops.GEMV_MAX_ROWS:
        raise ParrotHipError(f"generate_candidates: n={n}; the candidates step takes 1 to {ops.GEMV_MAX_ROWS} rows")
    why = model.batched_decode_unsupported()
    if why is not None:
        raise ParrotHipError(f"generate_candidates: {why}; use generate() per candidate")
    if max_seq_length < max_returned_tokens:
        raise ParrotHipError(f"generate_candidates: max_seq_length={max_seq_length} < max_returned_tokens={max_returned_tokens}: the shared "
                             "prompt cache and the candidates' own caches are addressed by position (no sliding window); use "
                             "generate_batch(model, [idx] * n, ...)")
    _cuda_device("generate_candidates", model)
    greedy = top_k == 1 and temperature > 0
    sampler = None if greedy else (float(temperature), top_k)
    eos = -1 if eos_id is None else int(eos_id)
    tail = candidate_tail_slots(max_returned_tokens, T)
    # (a captured step keeps the attention launches it was captured with: the switch is part of the key)
    key = ("candidates", n, max_seq_length, tail, greedy, sampler, eos, bool(ops.CANDIDATES_SHARE_LOADS))
    sess = _cached_session(model, key, max_returned_tokens, lambda: CandidateSession(model, n, max_seq_length, tail, greedy, sampler, eos))
    sess.prefill(idx.to(device=sess.device, dtype=torch.int64), max_returned_tokens)
    return _decode_rows(sess, [idx] * n, max_returned_tokens, eos_id)


class ScoringSession(CandidateSession):
    """CandidateSession with the tokens GIVEN: n rows (1 <= n <= 8) that continue ONE prompt with known continuations, scored.

        tokens      int64[n][L]     row b: the prompt, then continuation b, written ahead of time and never by the step
        end         int32[n]        T + len_b: row b freezes once its last token is scored
        logprob     float32[n][L]   column p: log P(tokens[b, p] | tokens[b, :p]) for T <= p < end[b]
        is_greedy   int32[n][L]     column p: whether tokens[b, p] is the arg-max of that row of logits

    The step is the candidates step with ``ops.logprob_advance_rows`` in the place of the sampling launch (score.py)."""

    def __init__(self, model: GPT, n: int, max_seq_length: int, tail_slots: int, use_graph: bool = True) -> None:
        super().__init__(model, n, max_seq_length, tail_slots, True, use_graph=use_graph)
        self.logprob = torch.zeros(self.tokens.shape, dtype=torch.float32, device=self.device)
        self.is_greedy = torch.zeros(self.tokens.shape, dtype=torch.int32, device=self.device)

    def sample(self, logits: torch.Tensor, eos_id: int = -1) -> None:
        """Row b: the token at ``tokens[b, pos[b] + 1]`` scored against ``logits[b]``, ``pos[b] += 1``, unless the row is at its end."""
        ops.logprob_advance_rows(logits, self.tokens, self.pos, self.end, self.logprob, self.is_greedy)

    def _written(self) -> List[torch.Tensor]:
        return super()._written() + [self.logprob, self.is_greedy]

    def prefill(self, prompt: torch.Tensor, continuations: Sequence[torch.Tensor]) -> None:
        """The prompt ONCE into the shared cache (CandidateSession.prefill) and every continuation behind it in its row."""
        T = self.T = prompt.numel()
        for b, c in enumerate(continuations):
            self.tokens[b, T:T + c.numel()].copy_(c)
        super().prefill(prompt, 0)
        self.end.copy_(torch.tensor([T + c.numel() for c in continuations], dtype=torch.int32))

    def score_first(self) -> None:
        """Entry 0 of every row from the prompt's last-row logits, in one ``token_logprob_rows`` launch; leaves ``pos`` = T."""
        T = self.T
        first = torch.empty((self.B,), dtype=torch.float32, device=self.device)
        greedy = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        ops.token_logprob_rows(self.first_logits, self.tokens[:, T].contiguous(), first, greedy)
        self.logprob[:, T] = first
        self.is_greedy[:, T] = greedy
        self.pos.fill_(T)


# ------------------------------------------------------------------------------------------------ speculative decode
def _check_speculative(model: GPT, max_seq_length: int, max_tokens: int, draft_len: int, ngram_max: int, ngram_min: int) -> None:
    """What the speculative step asks of its parameters, of the model and of the window (session and entry point alike)."""
    if not 1 <= draft_len <= ops.MAX_DRAFT_LEN:
        raise ParrotHipError(f"draft_len={draft_len}: the speculative step verifies 1 to {ops.MAX_DRAFT_LEN} drafts")
    if not 1 <= ngram_min <= ngram_max <= ops.MAX_NGRAM:
        raise ParrotHipError(f"n-grams {ngram_min} .. {ngram_max}: 1 <= ngram_min <= ngram_max <= {ops.MAX_NGRAM} expected")
    why = model.speculative_decode_unsupported()
    if why is not None:
        raise ParrotHipError(f"generate_speculative: {why}; use generate()")
    if max_seq_length < max_tokens:
        raise ParrotHipError(f"generate_speculative: max_seq_length={max_seq_length} < max_returned_tokens={max_tokens}: the "
                             "rows of a speculative step must not wrap the cache ring (no sliding window); use generate()")


class SpeculativeSession(_Session):
    """Greedy decoding of ONE sequence that verifies ``draft_len`` guessed tokens per weight pass (prompt-lookup speculative
    decoding).  The drafts are what followed the last earlier occurrence of the sequence's newest n-gram (``ops.ngram_draft``); the
    token at ``pos`` and the K drafts behind it go through the network as the M = K + 1 rows of one pass, every row bit for bit
    what the one-row step computes for it, and ``ops.verify_advance`` keeps the drafts that are the arg-max of the row before them.
    The tokens are therefore exactly ``generate(top_k=1)``'s; only the number of steps changes.

        tokens  int64[max_tokens + 1]   the prompt, the generated tokens and, behind ``pos``, the current drafts
        pos     int32[1]                position of the newest known token
        end     int32[1]                no token is written at or past it (max_returned_tokens)
        state   int32[8]                ops.SPEC_*: what the host reads once per step

    Two steps are captured over these buffers, each ending with the drafting for the next one:
        rows:  M-row pass -> verify_advance -> ngram_draft          one:  one-row pass -> argmax_advance -> ngram_draft
    ``generate_speculative`` replays ``rows`` when the last drafting found an earlier occurrence and ``pos + M`` stays inside the
    token buffer, the cache and the RoPE tables, else ``one``: no row is ever computed at a position outside them.

    ``draft_hook(session) -> int``, when given, replaces the lookup kernel: it writes ``tokens[pos+1 .. pos+K]`` and returns how
    many of them are guesses (0: take the one-row step).  It runs on the host between the replays, outside the captured steps."""

    def __init__(self, model: GPT, max_seq_length: int, max_tokens: int, draft_len: int = 1, ngram_max: int = 3, ngram_min: int = 1,
                 eos_id: int = -1, use_graph: bool = True, draft_hook: Optional[Callable[["SpeculativeSession"], int]] = None) -> None:
        _check_speculative(model, max_seq_length, max_tokens, draft_len, ngram_max, ngram_min)
        self._open("generate_speculative", model, max_seq_length, (max_tokens + 1,), 1, use_graph)
        self.K, self.M = draft_len, draft_len + 1
        self.ngram_max, self.ngram_min, self.eos_id, self.draft_hook = ngram_max, ngram_min, eos_id, draft_hook
        dev = self.device
        self.pos = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.end = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.state = torch.zeros((ops.SPEC_STATE_WORDS,), dtype=torch.int32, device=dev)
        self.ws_one = model.workspace(1, dev, 1)
        self.ws_rows = model.workspace(self.M, dev, self.M, Rows.DRAFTS)
        self.graphs: Dict[bool, torch.cuda.CUDAGraph] = {}  # True: the M-row step, False: the one-row step
        self.caches = [(k[0], v[0]) for k, v in model.kv_caches]
        self._drop_reference_weights()

    def draft(self) -> None:
        """The lookup kernel (the hook, when there is one, is called by the loop instead: it is host code)."""
        if self.draft_hook is None:
            ops.ngram_draft(self.tokens, self.pos, self.K, self.ngram_max, self.ngram_min, self.state)

    def _step_rows(self) -> torch.Tensor:
        logits = self.model.run_rows(self.ws_rows, self.tokens, self.pos, self.pos, self.S, self.caches, self.model.rope_cache)
        ops.verify_advance(logits, self.tokens, self.pos, self.end, self.eos_id, self.state)
        self.draft()
        return logits

    def _step_one(self) -> torch.Tensor:
        logits = self.model.run_rows(self.ws_one, self.tokens, self.pos, self.pos, self.S, self.caches, self.model.rope_cache)
        ops.argmax_advance(logits, self.tokens, self.pos)
        self.draft()
        return logits

    def prefill(self, prompt: torch.Tensor, max_returned_tokens: int) -> torch.Tensor:
        """Run the T prompt rows, leave ``pos`` = T-1 and return the logits of the last prompt token (DecodeSession.prefill)."""
        T = prompt.numel()
        self.tokens[:T].copy_(prompt)
        self.pos.zero_()
        self.end.fill_(max_returned_tokens)
        self.state.zero_()
        logits = _run_prompt(self.model, self.tokens, T, self.pos, self.S, self.caches)
        self.pos.fill_(T - 1)
        return logits

    def _written(self) -> List[torch.Tensor]:
        return super()._written() + [self.state]

    def capture(self, rows: bool = True) -> None:
        """Capture the one-row step and, with ``rows``, the M-row step (each once).  The warm-up runs at the position the prompt
        left: the caller passes ``rows`` only when ``pos + M`` is inside every buffer there."""
        if not self.use_graph:
            return
        for is_rows, step in ((True, self._step_rows), (False, self._step_one)):
            if is_rows not in self.graphs and (rows or not is_rows):
                self.graphs[is_rows] = _capture(step, self._written(), self.device, False)

    def step(self, rows: bool) -> torch.Tensor:
        """One step: the M-row verification pass (``rows``) or the one-row step; returns that pass's logits buffer."""
        if self.use_graph:
            self.graphs[rows].replay()
            return self.ws_rows.logits if rows else self.ws_one.logits
        return self._step_rows() if rows else self._step_one()

    def read(self, hook_matched: int = 0) -> Tuple[int, int, int]:
        """The step's one host read: (pos, drafts the last drafting matched, tokens[pos])."""
        if self.draft_hook is None:
            st = self.state.cpu()
            return int(st[ops.SPEC_POS]), int(st[ops.SPEC_MATCHED]), int(st[ops.SPEC_LAST])
        p = int(self.pos)
        return p, hook_matched, int(self.tokens[p])


@torch.no_grad()
def generate_speculative(
    model: torch.nn.Module,
    idx: torch.Tensor,
    max_returned_tokens: int,
    max_seq_length: int,
    *,
    draft_len: int = 1,
    ngram_max: int = 3,
    ngram_min: int = 1,
    eos_id: Optional[int] = None,
    return_stats: bool = False,
    draft_hook: Optional[Callable[[SpeculativeSession], int]] = None,
):
    """What ``generate(model, idx, max_returned_tokens, max_seq_length, top_k=1, eos_id=eos_id)`` returns, token for token, in
    fewer weight passes: every step verifies ``draft_len`` tokens guessed by prompt lookup (SpeculativeSession) next to the one it
    decodes.  Greedy only - rejection sampling would not reproduce the reference's draws.  With ``return_stats`` the result is
    ``(tokens, {"steps": weight passes after the prompt, "accepted": drafts kept, "matched_steps": passes that verified drafts})``.
    ``draft_hook`` (tests, tools/spec_bench.py) replaces the lookup, see SpeculativeSession."""
    T = idx.size(0)
    _check_args("generate_speculative", model, [T], max_returned_tokens, max_seq_length, length_first=True)
    _check_speculative(model, max_seq_length, max_returned_tokens, draft_len, ngram_max, ngram_min)
    _cuda_device("generate_speculative", model)
    eos = -1 if eos_id is None else int(eos_id)
    make = lambda: SpeculativeSession(model, max_seq_length, max_returned_tokens, draft_len, ngram_max, ngram_min, eos,  # noqa: E731
                                      draft_hook=draft_hook)
    if draft_hook is not None:
        sess = make()  # (a hook is the caller's object: its session is not kept)
    else:
        sess = _cached_session(model, ("speculative", max_seq_length, draft_len, ngram_max, ngram_min, eos), max_returned_tokens, make)
    M = sess.M
    limit = min(max_returned_tokens, max_seq_length, model.config.block_size)  # rows at pos .. pos+M-1 need pos + M <= limit
    dtype = idx.dtype
    logits = sess.prefill(idx.to(device=sess.device, dtype=torch.int64), max_returned_tokens)
    sess.capture(rows=T - 1 + M <= limit)  # (a prompt that ends within M of the limit never takes the M-row step)
    ops.argmax_advance(logits, sess.tokens, sess.pos)  # the first token, as generate() samples it
    sess.draft()
    steps = matched_steps = hook_matched = 0
    while True:
        if draft_hook is not None:
            hook_matched = int(draft_hook(sess))
        p, matched, last = sess.read(hook_matched)  # host sync, the one generate() pays with eos_id
        stop_eos = eos_id is not None and last == eos
        if stop_eos or p + 1 >= max_returned_tokens:
            break
        rows = matched > 0 and p + M <= limit
        sess.step(rows)
        steps += 1
        matched_steps += int(rows)
    # generate() returns idx[:input_pos]: the eos token is not part of the result
    out = sess.tokens[: p if stop_eos else p + 1].to(dtype).clone()
    if return_stats:
        return out, {"steps": steps, "accepted": int(sess.state[ops.SPEC_ACCEPTED]), "matched_steps": matched_steps}
    return out
