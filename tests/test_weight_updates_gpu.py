"""Derived state follows the weights: every executor decodes with the CURRENT weights (the rule: lit-parrot_amd/weights.py).

Every case: build a model with weights A, use an entry point once so that its session, captured graph, kernel-layout copies and
engine images exist, change the weights towards B in one of the supported ways - with or without ``model.reset_cache()`` in
between -, use the entry point again and compare with a fresh twin that was filled with the same result the same way and never
saw A.  Every comparison is bit equality: greedy tokens ``torch.equal``, logits and log-probs equal as bits.  There is no
tolerance in this file.  ``test_two_fresh_twins_agree`` holds two fresh twins of B to the same equality once per executor and
format, so that an inequality elsewhere is never blamed on staleness wrongly.  That the updates move the logits far beyond any
tolerance of the suite is shown on the CPU oracle (tests/test_weight_updates_host.py, the pairs of ``weight_updates.PAIRS``).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import lit_parrot_amd as L  # noqa: E402
import weight_updates as wu  # noqa: E402
from lit_parrot_amd.chat import base as chat  # noqa: E402
from lit_parrot_amd.checkpoint import stream_load  # noqa: E402
from lit_parrot_amd.generate import base as gb  # noqa: E402
from lit_parrot_amd.quantize.gptq import ColBlockQuantizedLinear, rtn_quantize  # noqa: E402
from lit_parrot_amd.synth import is_linear_key  # noqa: E402
from lit_parrot_amd.weights import weights_generation  # noqa: E402
from oracle import int4 as o4  # noqa: E402

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
T, N = wu.PROMPT_T, 20  # prompt tokens, returned tokens = window
MODES = {"bf16": None, "int4": "gptq.int4-g128", "nf4": "bnb.nf4", "int8": "bnb.int8"}
SHAPES = {"bf16": "tiny-llama", "int4": "tiny-llama", "int8": "tiny-llama", "nf4": "tiny-llama-hs128-i384", "bf16-neox": "tiny-neox-hs64"}


@pytest.fixture
def engine_off(hip_lib):
    gb.ENGINE_DEFAULT = False
    yield
    gb.ENGINE_DEFAULT = "auto"


@pytest.fixture
def executor(request, hip_lib):
    """The step's executor, forced: "engine" (the one-launch stream engine) or "multi-launch"; hands the test ``engine: bool``."""
    gb.ENGINE_DEFAULT = request.param == "engine"
    yield request.param == "engine"
    gb.ENGINE_DEFAULT = "auto"


# ------------------------------------------------------------------------------------------------ models and updates
def mode_of(fmt):
    return MODES[fmt.split("-")[0]]


def empty(fmt):
    with torch.device(DEV), L.quantization(mode_of(fmt)):
        model = L.GPT(wu.config(SHAPES[fmt]))
    return model.to(BF).eval()


def fresh(fmt, sd):
    """A new model object filled by ``stream_load`` (dense weights are quantised on the way in)."""
    model = empty(fmt)
    assert stream_load(model, sd) == []
    return model


def load_whole(fmt, model, sd):
    """``load_state_dict`` of a whole checkpoint, in the form each format takes it."""
    if fmt == "int4":
        model.load_state_dict(o4.quantize_state_dict(sd, 128, is_linear_key), strict=True)
    else:
        model.load_state_dict(dict(sd), strict=mode_of(fmt) is None)


def cpu_and_back(model, name):
    model.cpu()
    model.to(DEV)


def copy_through_data(model, name):
    model.transformer.h[0].attn.proj.weight.data.copy_(wu.update_of(name, "proj")[wu.PROJ])  # nothing sees this ...
    L.weights_changed(model)  # ... so the caller says it


# update -> (what it does to the used model, the weights a twin is filled with, how the twin is filled)
def apply_update(update, fmt, model):
    """Returns the twin: a fresh model object filled the same way with the same result."""
    name = SHAPES[fmt]
    pair = {"a": "whole", "b": "whole", "c": "fc_2", "d": "proj", "e": None}[update]
    assert pair is None or (name, pair) in wu.PAIRS, "an update that the host file does not prove to be visible"
    if update == "a":
        load_whole(fmt, model, wu.weights(name, "B"))
        twin = empty(fmt)
        load_whole(fmt, twin, wu.weights(name, "B"))
        return twin
    if update == "b":
        assert stream_load(model, wu.weights(name, "B")) == []
        return fresh(fmt, wu.weights(name, "B"))
    if update == "c":
        assert stream_load(model, wu.update_of(name, "fc_2")) == []
        return fresh(fmt, wu.updated(name, "fc_2"))
    if update == "d":
        copy_through_data(model, name)
        return fresh(fmt, wu.updated(name, "proj"))
    if update == "e":
        cpu_and_back(model, name)
        return None  # (the judge is the model's own output from before)
    raise KeyError(update)


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, i)
        n = int((bits(x) != bits(y)).sum())
        assert n == 0, f"{what}: result {i}: {n} of {x.numel()} values differ from the fresh twin's"


# ------------------------------------------------------------------------------------------------ entry points
def run_generate(model, fmt, with_engine):
    """``generate`` greedy: the tokens, and - from the session it used, as the library's cache hands it out - the logits of the
    prompt's last row and of the first decode step (a partial update may leave most arg-maxes where they were)."""
    p = wu.prompt(SHAPES[fmt]).to(DEV)
    y = L.generate(model, p, N, N, top_k=1)
    with torch.no_grad():
        sess = gb._session(model, N, N, True)
        assert sess.graph is not None and (sess.eng is not None) == with_engine
        first = sess.prefill(p).clone()
        sess.sample(first)
        step = sess.step().clone()
        sess.check_error()
    return [y, first, step]


def two_prompts(fmt):
    p = wu.prompt(SHAPES[fmt]).to(DEV)
    return [p, p.flip(0)[:T - 3].contiguous()]


def chat_tokens(model, fmt):
    p = wu.prompt(SHAPES[fmt]).to(DEV)
    out = [t.view(-1) for t in chat.generate(model, p, N, N, top_k=1, stop_tokens=([3, 1, 2],))]
    return [torch.cat(out)]


ENTRY = {
    "generate_batch": lambda m, fmt: L.generate_batch(m, two_prompts(fmt), N, N, top_k=1),
    "generate_candidates": lambda m, fmt: L.generate_candidates(m, wu.prompt(SHAPES[fmt]).to(DEV), 2, N, N, top_k=1),
    "generate_speculative": lambda m, fmt: [L.generate_speculative(m, wu.prompt(SHAPES[fmt]).to(DEV), N, N, draft_len=2)],
    "chat": chat_tokens,
    "token_logprobs": lambda m, fmt: [L.token_logprobs(m, wu.prompt(SHAPES[fmt]).to(DEV))],
}


def run_forward(model, fmt):
    """``model(idx)`` without and with ``input_pos``: no session, no graph - the control."""
    idx = wu.prompt(SHAPES[fmt]).to(DEV).view(1, -1)
    with torch.no_grad():
        plain = model(idx)
        model.reset_cache()
        cached = model(idx, N, torch.arange(T, device=DEV))
    return [plain, cached]


# ------------------------------------------------------------------------------------------------ generate: the matrix
# executor -> format -> the updates defined for it.  The stream engine is not built for NF4 Linears; bf16-neox is there for the
# engine: LayerNorm and a bias on every Linear, whose addresses the engine's op table holds next to the images (no SwiGLU: no c)
MATRIX = {
    "multi-launch": {"bf16": "abcde", "int4": "abce", "nf4": "abc", "int8": "abc"},
    "engine": {"bf16": "abcde", "int4": "abce", "int8": "abc", "bf16-neox": "abd"},
}
GENERATE_CASES = [(ex, fmt, u) for ex, fmts in MATRIX.items() for fmt, updates in fmts.items() for u in updates]
TWIN_CASES = [(ex, fmt) for ex, fmts in MATRIX.items() for fmt in fmts]


@pytest.mark.parametrize("reset", [True, False], ids=["reset_cache", "no_reset"])
@pytest.mark.parametrize("executor,fmt,update", GENERATE_CASES, indirect=["executor"])
def test_generate_decodes_with_the_current_weights(executor, fmt, update, reset):
    engine = executor
    model = fresh(fmt, wu.weights(SHAPES[fmt], "A"))
    before = run_generate(model, fmt, engine)
    twin = apply_update(update, fmt, model)
    if reset:
        model.reset_cache()
    after = run_generate(model, fmt, engine)
    want = before if twin is None else run_generate(twin, fmt, engine)
    same_bits(after, want, f"generate / {fmt} / update {update}")
    if twin is not None:
        assert any(int((bits(x) != bits(y)).sum()) for x, y in zip(before[1:], after[1:])), "the update did not change the logits at all"


# ------------------------------------------------------------------------------------------------ the other entry points
@pytest.mark.parametrize("fmt", ["bf16", "int4"])
@pytest.mark.parametrize("entry", list(ENTRY))
def test_other_entry_points_decode_with_the_current_weights(engine_off, entry, fmt):
    model = fresh(fmt, wu.weights(SHAPES[fmt], "A"))
    before = ENTRY[entry](model, fmt)
    twin = apply_update("b", fmt, model)  # (no reset_cache: the session, its graph and its buffers are all still there)
    after = ENTRY[entry](model, fmt)
    same_bits(after, ENTRY[entry](twin, fmt), f"{entry} / {fmt}")
    assert not all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(before, after)), "the update did not change the result at all"


@pytest.mark.parametrize("update", ["a", "b", "c"])
@pytest.mark.parametrize("fmt", ["bf16", "int4", "nf4", "int8"])
def test_forward_runs_on_the_current_weights(hip_lib, fmt, update):
    model = fresh(fmt, wu.weights(SHAPES[fmt], "A"))
    before = run_forward(model, fmt)
    twin = apply_update(update, fmt, model)
    after = run_forward(model, fmt)
    same_bits(after, run_forward(twin, fmt), f"model(idx) / {fmt} / update {update}")
    assert all(int((bits(x) != bits(y)).sum()) for x, y in zip(before, after))


# ------------------------------------------------------------------------------------------------ two fresh twins
@pytest.mark.parametrize("executor,fmt", TWIN_CASES, indirect=["executor"])
def test_two_fresh_twins_agree_on_generate(executor, fmt):
    engine = executor
    a, b = (fresh(fmt, wu.weights(SHAPES[fmt], "B")) for _ in range(2))
    same_bits(run_generate(a, fmt, engine), run_generate(b, fmt, engine), f"two fresh twins / generate / {fmt}")
    same_bits(run_forward(a, fmt), run_forward(b, fmt), f"two fresh twins / model(idx) / {fmt}")


@pytest.mark.parametrize("fmt", ["bf16", "int4"])
@pytest.mark.parametrize("entry", list(ENTRY))
def test_two_fresh_twins_agree(engine_off, entry, fmt):
    a, b = (fresh(fmt, wu.weights(SHAPES[fmt], "B")) for _ in range(2))
    same_bits(ENTRY[entry](a, fmt), ENTRY[entry](b, fmt), f"two fresh twins / {entry} / {fmt}")


# ------------------------------------------------------------------------------------------------ the unchanged path stays cheap
@pytest.mark.parametrize("fmt", ["bf16", "int4", "int8"])
def test_nothing_is_rebuilt_while_the_weights_stay(hip_lib, fmt):
    """No change of the weights: a second ``generate()`` replays the captured graph of the first (same session object), and after
    ``reset_cache()`` - which drops the KV caches the session was built over, so the session is built anew as before this rule
    existed - the new engine takes the model's images as they are: same keys, same device addresses, nothing repacked."""
    gb.ENGINE_DEFAULT = True
    try:
        model = fresh(fmt, wu.weights(SHAPES[fmt], "A"))
        p = wu.prompt(SHAPES[fmt]).to(DEV)
        g0 = weights_generation(model)
        y0 = L.generate(model, p, N, N, top_k=1)
        sess = gb._session(model, N, N, True)
        assert sess.graph is not None and sess.eng is not None and sess.weights_generation == g0
        graph = sess.graph
        y1 = L.generate(model, p, N, N, top_k=1)
        assert gb._session(model, N, N, True) is sess and sess.graph is graph and len(model._decode_sessions) == 1
        assert weights_generation(model) == g0, "decoding is not a change of the weights"

        def addresses():
            return {k: (v[0] if isinstance(v, tuple) else v).data_ptr() for k, v in model._engine_images.items()}

        images = addresses()
        assert images
        model.reset_cache()
        y2 = L.generate(model, p, N, N, top_k=1)
        sess2 = gb._session(model, N, N, True)
        assert sess2.eng is not None and sess2.graph is not None
        assert addresses() == images, "a rebuilt engine repacked images although the weights did not change"
        assert torch.equal(y0, y1) and torch.equal(y0, y2)
    finally:
        gb.ENGINE_DEFAULT = "auto"


# ------------------------------------------------------------------------------------------------ A -> B -> A
@pytest.mark.parametrize("reset", [True, False], ids=["reset_cache", "no_reset"])
def test_double_reload_on_int8_engine(hip_lib, reset):
    """A -> B -> A with no decode in between: every LLM.int8 ``Parameter`` is replaced twice, and the allocator may hand A's second
    copy the address of its first.  A key made of (address, version) cannot tell the three states apart; the epochs can.  The
    result is that of a fresh model filled with A."""
    gb.ENGINE_DEFAULT = True
    try:
        name = SHAPES["int8"]
        model = fresh("int8", wu.weights(name, "A"))
        run_generate(model, "int8", True)
        assert stream_load(model, wu.weights(name, "B")) == []
        assert stream_load(model, wu.weights(name, "A")) == []
        if reset:
            model.reset_cache()
        got = run_generate(model, "int8", True)
        same_bits(got, run_generate(fresh("int8", wu.weights(name, "A")), "int8", True), "int8 engine after A -> B -> A")
    finally:
        gb.ENGINE_DEFAULT = "auto"


# ------------------------------------------------------------------------------------------------ released reference buffers
def test_reference_buffers_stay_usable_after_a_session_released_them(engine_off):
    """After an int4 ``generate`` the reference-layout buffers are released (W4K is the one resident image).  Reading one then
    returns the full tensor; assigning ``scales`` / ``zeros`` and calling ``pack_weight`` - the reference interface's way of
    putting other weights in - takes effect: the next ``generate`` gives what a fresh model gives that took the same calls
    without ever decoding.  (``ParrotHipError`` would be the other acceptable answer; a silent no-op is not.)"""
    name = SHAPES["int4"]
    assert (name, "proj") in wu.PAIRS
    model = fresh("int4", wu.weights(name, "A"))
    reader, lin = model.transformer.h[1].mlp.proj, model.transformer.h[0].attn.proj
    kept = [t.clone() for t in (reader.quant_weight, reader.scales, reader.zeros)]
    before = run_generate(model, "int4", False)
    assert gb.RELEASE_REFERENCE_BUFFERS and reader._released and lin._released
    assert all(m._released for m in model.modules() if isinstance(m, ColBlockQuantizedLinear))
    g0 = weights_generation(model)
    qw = reader.quant_weight
    assert qw.shape == (reader.out_features, reader.in_features // 2) and qw.stride() == (1, reader.out_features)
    assert all(torch.equal(a, b) for a, b in zip(kept, (qw, reader.scales, reader.zeros))), "the buffers came back changed"
    assert weights_generation(model) == g0, "reading a buffer is not a change of the weights"

    def put_b_in(m):
        target = m.transformer.h[0].attn.proj
        w = wu.update_of(name, "proj")[wu.PROJ].to(DEV)
        _, s, z = rtn_quantize(w, target.tile_cols)
        target.scales = s
        target.zeros = z
        target.pack_weight(w)

    assert lin._released
    try:
        put_b_in(model)
    except L.ParrotHipError:
        return  # the loud answer
    assert weights_generation(model) != g0
    twin = fresh("int4", wu.weights(name, "A"))
    put_b_in(twin)
    after = run_generate(model, "int4", False)
    same_bits(after, run_generate(twin, "int4", False), "int4 after assigning released reference buffers")
    assert any(int((bits(x) != bits(y)).sum()) for x, y in zip(before[1:], after[1:])), "the assignment was lost"
