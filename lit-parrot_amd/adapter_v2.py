"""LLaMA-Adapter v2 behind the reference's ``lit_gpt.adapter_v2`` surface.

``add_adapter_v2_parameters_to_linear_layers(model)`` gives every ``nn.Linear`` of an ``adapter.GPT`` - ``lm_head``,
``attn.attn``, ``attn.proj`` and the MLP Linears - an ``adapter_bias`` (zeros) and an ``adapter_scale`` (ones) of
``out_features`` elements, as the reference does (lit_gpt/adapter_v2.py:34-53).  The Linear then computes
``adapter_scale * (F.linear(x, W, b) + adapter_bias)`` - in bf16 three roundings - before the residual add, GELU or SwiGLU.
The model's ``_linear`` finds the two vectors on the module and hands them to the adapter entry points of the dense
kernels (``parrot_bf16_gemv_adapter`` fused into the decode GEMV, ``parrot_adapter_epilogue`` after the prompt GEMMs).
Quantized Linears have no adapter kernels: a model that carries the vectors on one is refused with ``ParrotHipError``.
"""
from typing import Any

import torch
import torch.nn as nn

from . import ops
from ._hip import ParrotHipError
from .adapter import GPT, Config  # noqa: F401  (the reference module exposes the adapter GPT too)

_V2_KEYS = ("adapter_wte", "gating_factor", "adapter_scale", "adapter_bias", "norm_1", "norm_2", "ln_f")


def adapter_filter(key: str, value: Any) -> bool:
    """True for what Adapter-v2 trains: the v1 prefix and gates, the Linears' scale / bias vectors and the norms."""
    return any(s in key for s in _V2_KEYS)


def mark_only_adapter_v2_as_trainable(model: nn.Module) -> None:
    """requires_grad only on the Adapter-v2 parameters."""
    for name, param in model.named_parameters():
        param.requires_grad = adapter_filter(name, param)


def _adapter_v2_forward(self: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    """A stand-alone call of an adapter-v2 Linear, on the HIP kernels (the model itself goes through ``model._linear``)."""
    if hasattr(self, "hip_linear"):
        raise ParrotHipError("adapter-v2 vectors on a quantized Linear have no HIP kernel")
    rows = x.reshape(-1, x.shape[-1]).contiguous()
    out = torch.empty((rows.shape[0], self.out_features), dtype=rows.dtype, device=rows.device)
    ops.bf16_linear(self.weight.data, rows, out, bias=None if self.bias is None else self.bias.data,
                    adapter=ops.Adapter(self.adapter_scale.data, self.adapter_bias.data))
    return out.view(*x.shape[:-1], self.out_features)


def adapter_v2_linear_with_bias_and_scale(layer: nn.Linear) -> nn.Linear:
    """Attach ``adapter_bias`` (zeros) and ``adapter_scale`` (ones), frozen, in the weight's dtype and device."""
    n, w = layer.weight.shape[0], layer.weight
    layer.adapter_bias = nn.Parameter(torch.zeros(n, dtype=w.dtype, device=w.device), requires_grad=False)
    layer.adapter_scale = nn.Parameter(torch.ones(n, dtype=w.dtype, device=w.device), requires_grad=False)
    layer.forward = _adapter_v2_forward.__get__(layer, layer.__class__)
    return layer


def add_adapter_v2_parameters_to_linear_layers(model: nn.Module) -> None:
    for module in model.modules():
        if isinstance(module, nn.Linear):
            adapter_v2_linear_with_bias_and_scale(module)
