"""Derived state follows the weights: the host half (no device).  The rule is in lit-parrot_amd/weights.py.

What is checked here: every supported way of changing weights moves ``weights_generation(model)`` and nothing else does; the
session caches of generate/base.py and chat/base.py call a session stale under another generation; the stream engine's image
key (``weights.image_stamp``) follows the weights, its SwiGLU partner's included; the LLM.int8 SwiGLU pair follows both halves;
and - on the CPU oracle - the updates tests/test_weight_updates_gpu.py uses move the logits far beyond any tolerance of the suite.
"""
from types import SimpleNamespace

import pytest
import torch

import lit_parrot_amd as L
import weight_updates as wu
from lit_parrot_amd.chat import base as cb
from lit_parrot_amd.checkpoint import stream_load
from lit_parrot_amd.generate import base as gb
from lit_parrot_amd.quantize.bnb import InferenceLinear8bitLt
from lit_parrot_amd.quantize.gptq import ColBlockQuantizedLinear
from lit_parrot_amd.weights import image_stamp, weights_generation
from oracle import model as om

BF = torch.bfloat16
NAMES = ["tiny-llama", "tiny-neox"]


def bf16_gpt(name, dtype=BF):
    model = L.GPT(wu.config(name)).to(dtype)
    model.load_state_dict(wu.weights(name, "A", dtype))
    return model


def int4_gpt(name):
    with L.quantization("gptq.int4-g128"):
        return L.GPT(wu.config(name))


def one_key(name):
    return wu.PROJ  # (both families have it)


CHANGES = {
    "load_state_dict": lambda m, name: m.load_state_dict(wu.weights(name, "B")),
    "stream_load": lambda m, name: stream_load(m, wu.weights(name, "B")),
    "stream_load_one_key": lambda m, name: stream_load(m, {one_key(name): wu.weights(name, "B")[one_key(name)]}),
    "weights_changed": lambda m, name: L.weights_changed(m),
    "data_copy_then_weights_changed": lambda m, name: (m.transformer.h[0].attn.proj.weight.data.copy_(wu.weights(name, "B")[wu.PROJ]),
                                                       L.weights_changed(m)),
    "to_same_dtype": lambda m, name: m.to(BF),
}
NO_CHANGES = {
    "state_dict": lambda m: m.state_dict(),
    "named_parameters": lambda m: list(m.named_parameters()),
    "reset_cache": lambda m: m.reset_cache(),
    "read_a_weight": lambda m: (m.lm_head.weight, m.transformer.h[0].attn.proj.weight.data, m.transformer.wte.weight.sum()),
    "eval": lambda m: m.eval(),
}


# ------------------------------------------------------------------------------------------------ the generation
@pytest.mark.parametrize("change", list(CHANGES))
@pytest.mark.parametrize("name", NAMES)
def test_every_supported_change_moves_the_generation(name, change):
    model = bf16_gpt(name)
    g0 = model.weights_generation
    assert isinstance(g0, int) and g0 == weights_generation(model)
    CHANGES[change](model, name)
    g1 = model.weights_generation
    assert g1 != g0
    CHANGES[change](model, name)  # and again: no value comes back
    assert model.weights_generation not in (g0, g1)


@pytest.mark.parametrize("name", NAMES)
def test_casting_the_model_moves_the_generation(name):
    model = bf16_gpt(name, torch.float32)
    g0 = model.weights_generation
    model = model.to(BF)
    assert model.weights_generation != g0


@pytest.mark.parametrize("name", NAMES)
def test_an_int4_model_moves_the_generation_with_its_linears(name):
    model = int4_gpt(name)
    lin = model.transformer.h[1].mlp.proj
    assert isinstance(lin, ColBlockQuantizedLinear)
    seen = [model.weights_generation]

    def moved(what):
        g = model.weights_generation
        assert g not in seen, what
        seen.append(g)

    lin.scales.fill_(0.01)
    lin.zeros.fill_(8.0)
    lin.pack_weight(torch.zeros(lin.out_features, lin.in_features))
    moved("pack_weight")
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    assert model.weights_generation == seen[-1]  # (state_dict() is a read)
    model.load_state_dict(sd)
    moved("load_state_dict")
    lin._packed = torch.zeros(1)  # (stands for the kernel-layout copy: there is no device here)
    lin.scales = torch.full_like(lin.scales, 0.02)  # the idiom of GPTQQuantizer.quantize and synth.build_synthetic_model
    moved("assigning a reference buffer")
    assert lin._packed is None, "an assigned reference buffer leaves the old kernel-layout copy in place"
    lin._packed = torch.zeros(1)
    L.weights_changed(model)
    moved("weights_changed")
    assert lin._packed is None
    _ = lin.quant_weight, lin.scales, lin.zeros, list(model.named_buffers())
    assert model.weights_generation == seen[-1], "reading a buffer is not a change"
    assert seen == sorted(seen)


@pytest.mark.parametrize("read", list(NO_CHANGES))
@pytest.mark.parametrize("name", NAMES)
def test_reads_do_not_move_the_generation(name, read):
    model = bf16_gpt(name)
    g0 = model.weights_generation
    NO_CHANGES[read](model)
    assert model.weights_generation == g0


def test_weights_changed_is_public_and_takes_a_model():
    assert "weights_changed" in L.__all__
    with pytest.raises(L.ParrotHipError):
        L.weights_changed({"not": "a model"})


def test_weights_changed_drops_every_piece_of_derived_state():
    model = bf16_gpt("tiny-llama")
    model.__dict__["_decode_sessions"] = {"k": object()}
    model.__dict__["_chat_sessions"] = {"k": object()}
    model.__dict__["_engine_images"] = {"k": object()}
    L.weights_changed(model)
    assert not any(n in model.__dict__ for n in ("_decode_sessions", "_chat_sessions", "_engine_images"))


# ------------------------------------------------------------------------------------------------ the session caches
class StubSession(SimpleNamespace):
    """What the caches look at: the token buffer, the caches it was built over and the generation it was built under."""


def stub_for(model, length=33):
    return StubSession(tokens=torch.zeros(length, dtype=torch.int64), caches=[(k, v) for k, v in model.kv_caches],
                       weights_generation=weights_generation(model))


def model_with_caches(name="tiny-llama"):
    model = bf16_gpt(name)
    model.kv_caches = [(torch.zeros(4), torch.zeros(4))]
    return model


def decode_session(model, key=("k",)):
    return gb._cached_session(model, key, 32, lambda: stub_for(model))


def chat_session(model, monkeypatch):
    monkeypatch.setattr(cb, "ChatSession", lambda model, S, max_tokens, greedy, sampler: stub_for(model, max_tokens + 1))
    return cb._session(model, 32, 32, True, 1, 2)


@pytest.mark.parametrize("kind", ["decode", "chat"])
@pytest.mark.parametrize("change", list(CHANGES))
def test_a_cached_session_does_not_survive_a_change_of_the_weights(kind, change, monkeypatch):
    get = decode_session if kind == "decode" else (lambda m: chat_session(m, monkeypatch))
    model = model_with_caches()
    first = get(model)
    assert get(model) is first, "nothing changed: the captured step is reused"
    for read in NO_CHANGES.values():
        if read is not NO_CHANGES["reset_cache"]:  # (reset_cache drops the KV caches, which rebuilds a session by the older rule)
            read(model)
    assert get(model) is first
    CHANGES[change](model, "tiny-llama")
    second = get(model)
    assert second is not first, f"{change}: the session built from the old weights came back"
    assert get(model) is second


def test_the_session_cache_keeps_its_bound_and_its_order():
    """As test_model_gpu.py::test_captured_steps_per_model_are_bounded describes them: at most MAX_SESSIONS_PER_MODEL sessions, the
    least recently used goes first, and coming back to a kept key neither rebuilds it nor leaves it at the front."""
    model = model_with_caches()
    keys = [("k", i) for i in range(gb.MAX_SESSIONS_PER_MODEL + 3)]
    for k in keys:
        decode_session(model, k)
        assert len(model._decode_sessions) <= gb.MAX_SESSIONS_PER_MODEL
    kept = list(model._decode_sessions)
    assert kept == keys[-gb.MAX_SESSIONS_PER_MODEL:]
    first = model._decode_sessions[kept[0]]
    assert decode_session(model, kept[0]) is first
    assert list(model._decode_sessions) == kept[1:] + kept[:1]
    L.weights_changed(model)  # a change of the weights empties the cache; the bound holds for what comes after
    for k in keys:
        decode_session(model, k)
    assert list(model._decode_sessions) == keys[-gb.MAX_SESSIONS_PER_MODEL:] and all(s is not first for s in model._decode_sessions.values())


def test_a_real_session_records_the_generation_it_is_built_under():
    """``_Session._open`` is where every session class starts; it stamps the generation before anything is built from the weights."""
    import inspect

    src = inspect.getsource(gb._Session._open)
    assert "self.weights_generation = weights_generation(model)" in src
    assert src.index("self.weights_generation") < src.index("self.tokens =")


# ------------------------------------------------------------------------------------------------ the engine's image key
def test_the_image_stamp_follows_the_weights():
    model = bf16_gpt("tiny-llama")
    mlp = model.transformer.h[1].mlp
    proj = model.transformer.h[0].attn.proj

    def stamps():
        return image_stamp(model, proj), image_stamp(model, mlp.fc_1, mlp.fc_2), image_stamp(model, mlp.proj, None, 0, 128)

    s0 = stamps()
    assert stamps() == s0 and len(set(s0)) == 3, "equal while nothing changes, distinct per Linear / pair / chunk"
    assert image_stamp(model, proj, generation=weights_generation(model)) == s0[0]
    b = wu.weights("tiny-llama", "B")
    v0 = proj.weight._version
    proj.weight.data.copy_(b[wu.PROJ])
    assert proj.weight._version == v0, "torch does not see a .data edit: that is why the stamp cannot rest on _version"
    assert stamps() == s0, "... and neither can anything else, until the caller says so"
    L.weights_changed(model)
    s1 = stamps()
    assert all(x != y for x, y in zip(s0, s1))
    stream_load(model, {wu.FC2: b[wu.FC2]})  # only the partner of the pair changes
    s2 = stamps()
    assert s2[1] != s1[1], "the image of a SwiGLU pair outlived a change of its partner"
    stream_load(model, b)
    assert all(x != y for x, y in zip(s2, stamps()))


def test_the_image_stamp_of_quantised_linears_follows_their_own_epoch():
    model = int4_gpt("tiny-llama")
    mlp = model.transformer.h[1].mlp
    s0 = image_stamp(model, mlp.fc_1, mlp.fc_2)
    mlp.fc_2.scales.fill_(0.01)
    mlp.fc_2.zeros.fill_(8.0)
    mlp.fc_2.pack_weight(torch.zeros(mlp.fc_2.out_features, mlp.fc_2.in_features))
    s1 = image_stamp(model, mlp.fc_1, mlp.fc_2)
    assert s1 != s0 and s1[0] == s0[0] and s1[1] != s0[1]
    assert image_stamp(model, mlp.fc_1, mlp.fc_2) == s1


# ------------------------------------------------------------------------------------------------ the LLM.int8 SwiGLU pair
def fake_int8(lin, seed):
    """An already quantised weight without the device quantiser: int8 rows and their scales."""
    g = torch.Generator().manual_seed(seed)
    CB = torch.randint(-127, 128, (lin.out_features, lin.in_features), generator=g, dtype=torch.int8)
    lin.weight = torch.nn.Parameter(CB, requires_grad=False)
    lin.weight.CB, lin.weight.SCB = CB, torch.rand(lin.out_features, generator=g)


def test_the_int8_pair_is_valid_for_the_epochs_of_both_partners():
    fc_1, fc_2 = InferenceLinear8bitLt(8, 4, bias=False), InferenceLinear8bitLt(8, 4, bias=False)
    fake_int8(fc_1, 1)
    fake_int8(fc_2, 2)
    CB, SCB = fc_1.pair_with(fc_2)
    assert torch.equal(CB, torch.cat([fc_1.weight.data, fc_2.weight.data])) and torch.equal(SCB, torch.cat([fc_1.weight.SCB, fc_2.weight.SCB]))
    assert fc_1.pair_with(fc_2)[0] is CB, "nothing changed: the pair is built once"
    # the partner alone gets another weight and goes through ``_apply`` (what ``.to()`` runs; ``_quantize_weight`` moves the epoch
    # the same way, on the device)
    e0 = fc_2.image_epoch
    fake_int8(fc_2, 3)
    fc_2._apply(lambda t: t)
    assert fc_2.image_epoch > e0 and fc_1._pair is not None
    CB2, SCB2 = fc_1.pair_with(fc_2)
    assert torch.equal(CB2[4:], fc_2.weight.data) and torch.equal(SCB2[4:], fc_2.weight.SCB), "fc_1 kept the old half of a changed fc_2"
    assert torch.equal(CB2[:4], fc_1.weight.data) and not torch.equal(CB2, CB)


# ------------------------------------------------------------------------------------------------ non-vacuity
@pytest.fixture(scope="module")
def oracle_logits():
    cache = {}

    def get(name, update):
        if (name, update) not in cache:
            sd = wu.weights(name, "A", torch.float32) if update is None else wu.updated(name, update, torch.float32)
            with torch.no_grad():
                cache[(name, update)] = om.OracleGPT(wu.config(name), sd)(wu.prompt(name).view(1, -1))[0].float()
        return cache[(name, update)]

    return get


@pytest.mark.parametrize("name,update", wu.PAIRS)
def test_updates_move_the_logits_beyond_every_tolerance(oracle_logits, name, update):
    """The loosest comparison of two executors in the suite allows 2^-5 x max(1, scale) on a logit.  Every update
    the GPU file applies moves some logit of the 12-token prompt by at least 4 x that, on the fp32 oracle: a tensor left behind
    by an update shows in a bit-for-bit comparison AND could not have passed any other test of the suite either.
    Measured (fp32 oracle, seeds 4321 -> 999): tiny-llama whole 1.40 / fc_2 0.227 / proj 0.971 against a margin of 0.125;
    tiny-neox-hs64 whole 1.70 / proj 1.03 against 0.173 / 0.144; tiny-llama-hs128 (intermediate 384) whole 1.63 / fc_2 0.289 against 0.143."""
    a, b = oracle_logits(name, None), oracle_logits(name, update)
    moved = float((a - b).abs().max())
    scale = max(1.0, float(a.abs().max()), float(b.abs().max()))
    margin = 4 * 2.0 ** -5 * scale
    agree = float((a.argmax(-1) == b.argmax(-1)).float().mean())
    print(f"{name} / {update}: max |d logit| {moved:.4g}, margin {margin:.4g}, arg-max agreement {agree:.2f}")
    assert moved >= margin, f"{name} / {update}: the update moves the logits by {moved:.4g} only (margin {margin:.4g}): scale the tensor (weight_updates.SCALE)"
