"""CPU-side checks of the LLaMA-Adapter / Adapter-v2 surface: parameter names and filters against the reference's lists
(tests/golden/adapter.npz), the merged-checkpoint load, and argument validation of the new C entry points (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

import lit_parrot_amd
from lit_parrot_amd import _hip
from lit_parrot_amd import adapter as A
from lit_parrot_amd import adapter_v2 as V
from lit_parrot_amd.synth import synthetic_state_dict

CASES = ["llama_gqa", "falcon_mqa", "neox", "llama_hs128", "llama_gqa_s0", "neox_v1"]


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(golden_dir / "adapter.npz")


def _model(g, case):
    name, start, v2 = (str(x) for x in g[f"{case}/cfg"])
    model = A.GPT(A.Config.from_name(name, adapter_start_layer=int(start)))
    if v2 == "1":
        V.add_adapter_v2_parameters_to_linear_layers(model)
    return model, v2 == "1"


def test_submodules_are_importable_like_the_reference():
    import lit_parrot_amd.adapter
    import lit_parrot_amd.adapter_v2

    assert lit_parrot_amd.adapter.GPT is A.GPT and lit_parrot_amd.adapter_v2.GPT is A.GPT
    assert "adapter" not in lit_parrot_amd.__all__  # the package's top-level names are unchanged
    cfg = A.Config.from_name("tiny-llama")
    assert (cfg.adapter_prompt_length, cfg.adapter_start_layer) == (10, 2)
    assert A.GPT.from_name("tiny-llama", adapter_start_layer=1).config.adapter_start_layer == 1


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_and_filters_equal_the_reference(g, case):
    model, v2 = _model(g, case)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[f"keys/{case}"]]
    filt = V.adapter_filter if v2 else A.adapter_filter
    assert [k for k, v in sd.items() if filt(k, v)] == [str(k) for k in g[f"filter/{case}"]]
    c = model.config
    for i, block in enumerate(model.transformer.h):
        if i >= c.adapter_start_layer:
            assert block.attn.gating_factor.shape == (1, c.n_head, 1, 1)
            assert block.attn.adapter_wte.weight.shape == (c.adapter_prompt_length, c.n_embd)
        else:
            assert not hasattr(block.attn, "gating_factor")
    if v2:
        lin = model.transformer.h[0].mlp.proj
        assert torch.equal(lin.adapter_scale, torch.ones(c.n_embd)) and torch.equal(lin.adapter_bias, torch.zeros(c.n_embd))
        assert not lin.adapter_scale.requires_grad


def test_mark_only_adapter_trainable():
    model = A.GPT(A.Config.from_name("tiny-llama", adapter_start_layer=1))
    A.mark_only_adapter_as_trainable(model)
    assert {n for n, p in model.named_parameters() if p.requires_grad} == {
        "transformer.h.1.attn.adapter_wte.weight", "transformer.h.1.attn.gating_factor"}
    V.add_adapter_v2_parameters_to_linear_layers(model)
    V.mark_only_adapter_v2_as_trainable(model)
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    assert "lm_head.adapter_scale" in trainable and "transformer.ln_f.weight" in trainable
    assert "lm_head.weight" not in trainable and "transformer.h.0.attn.attn.weight" not in trainable


def test_merged_checkpoint_loads_strict(g, tmp_path):
    """The fork's load: base lit_model.pth updated with the adapter file (``ckpt.get("model", ckpt)``), strict=True."""
    model, _ = _model(g, "llama_gqa")
    base = synthetic_state_dict(model.config, 4321, perturb=True)
    adapter_only = {k: v.clone() + 0.5 for k, v in model.state_dict().items() if V.adapter_filter(k, v) and k not in base}
    torch.save(base, tmp_path / "lit_model.pth")
    torch.save({"model": adapter_only}, tmp_path / "adapter.pth")
    ckpt = torch.load(tmp_path / "lit_model.pth")
    extra = torch.load(tmp_path / "adapter.pth")
    ckpt.update(extra.get("model", extra))
    model.load_state_dict(ckpt, strict=True)
    got = model.state_dict()
    assert torch.equal(got["transformer.h.1.attn.gating_factor"], adapter_only["transformer.h.1.attn.gating_factor"])
    assert torch.equal(got["lm_head.adapter_scale"], adapter_only["lm_head.adapter_scale"])
    with pytest.raises(RuntimeError):
        model.load_state_dict(base, strict=True)  # the base file alone misses the adapter keys


def test_adapter_entry_points_reject_bad_arguments(hip_lib):
    lib = hip_lib
    fake = 0x10000  # never dereferenced: every call below fails its argument checks before a launch
    # prefix attention: null pointers, aT out of range, bad group counts, head sizes
    assert lib.parrot_attn_adapter_prefix(fake, 1, None, fake, fake, 10, 2, 2, 64, fake, 256, 0, None) == -1
    assert lib.parrot_attn_adapter_prefix(fake, 1, fake, fake, fake, 65, 2, 2, 64, fake, 256, 0, None) == -3
    assert "65" in _hip.last_error()
    assert lib.parrot_attn_adapter_prefix(fake, 1, fake, fake, fake, 0, 2, 2, 64, fake, 256, 0, None) == -1
    assert lib.parrot_attn_adapter_prefix(fake, 1, fake, fake, fake, 10, 0, 2, 64, fake, 256, 0, None) == -1
    assert lib.parrot_attn_adapter_prefix(fake, 1, fake, fake, fake, 10, 2, 0, 64, fake, 256, 0, None) == -1
    assert lib.parrot_attn_adapter_prefix(fake, 1, fake, fake, fake, 10, 2, 2, 96, fake, 384, 0, None) == -3
    assert lib.parrot_attn_adapter_prefix(fake, 1, fake, fake, fake, 10, 2, 2, 64, fake, 255, 0, None) == -1  # ldy
    assert lib.parrot_attn_adapter_prefix(fake, 1, fake, fake, fake, 10, 2, 2, 64, fake, 256, 2, None) == -1  # softmax_mode
    assert lib.parrot_attn_adapter_prefix(fake, 0, fake, fake, fake, 10, 2, 2, 64, fake, 256, 0, None) == -1  # M
    fused = lambda aT, ng=2, ak=fake: lib.parrot_attn_fused_decode_adapter(  # noqa: E731
        fake, fake, fake, 32, fake, ng, 2, 64, 16, 1, None, None, fake, fake, fake, ak, fake, fake, aT, 0, None)
    assert fused(65) == -3 and fused(0) == -1 and fused(10, ng=0) == -1 and fused(10, ak=None) == -1
    # adapter Linear: partner vectors without a SwiGLU partner, aliasing / missing inputs of the element-wise pass
    ad = _hip.ParrotAdapter(fake, fake, fake, None)
    assert lib.parrot_bf16_gemv_adapter(fake, None, fake, 64, 1, None, None, 0, fake, 64, 64, 64, 0, None, C.byref(ad), None) == -1
    assert "partner" in _hip.last_error()
    assert lib.parrot_bf16_gemv_adapter(None, None, fake, 64, 1, None, None, 0, fake, 64, 64, 64, 0, None, None, None) == -1
    ok = _hip.ParrotAdapter(fake, fake, None, None)
    assert lib.parrot_adapter_epilogue(None, None, 64, 1, 64, C.byref(ok), 0, None, 0, fake, 64, None) == -1
    assert lib.parrot_adapter_epilogue(fake, None, 64, 1, 64, C.byref(ok), 0, None, 0, fake, 64, None) == -1  # out aliases t
    assert lib.parrot_adapter_epilogue(fake, None, 64, 1, 64, C.byref(ok), 3, None, 0, fake + 256, 64, None) == -1  # SWIGLU, no t2
    assert lib.parrot_adapter_epilogue(fake, None, 64, 1, 64, C.byref(ok), 1, None, 0, fake + 256, 64, None) == -1  # no residual
    assert lib.parrot_adapter_epilogue(fake, None, 32, 1, 64, C.byref(ok), 0, None, 0, fake + 256, 64, None) == -1  # ldt


def test_forward_refuses_cpu_tensors():
    model = A.GPT(A.Config.from_name("tiny-llama", adapter_start_layer=1)).to(torch.bfloat16)
    with pytest.raises(lit_parrot_amd.ParrotHipError):
        model(torch.zeros((1, 3), dtype=torch.int64))
