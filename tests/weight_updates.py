"""What the weight-update tests share (test_weight_updates_host.py, test_weight_updates_gpu.py): the shapes, the two sets of
weights A and B and the updates that lead from one to the other.

A model is built with weights A (seed 4321), used, and updated towards B (seed 999); a fresh twin filled with the same result
is the judge.  The host file proves on the CPU oracle that every (shape, update) pair listed in ``PAIRS`` moves the logits by at
least 4 x the bound any executor comparison of the suite allows (2^-5 x max(1, scale)), so weights left
behind by an update cannot hide inside a tolerance; the GPU file uses no pair that is not listed.
"""
import functools
from typing import Dict

import torch

from lit_parrot_amd.config import Config, name_to_config
from lit_parrot_amd.synth import synthetic_prompt, synthetic_state_dict

SEED_A, SEED_B = 4321, 999
PROMPT_T, PROMPT_SEED = 12, 3
FC2 = "transformer.h.1.mlp.fc_2.weight"   # the SwiGLU partner: int8 ``_pair``, the engine's partner stamp, ``packed2``
PROJ = "transformer.h.0.attn.proj.weight"

# update -> the keys of B that replace A's (None: all of them)
UPDATES = {"whole": None, "fc_2": (FC2,), "proj": (PROJ,)}
# Replaced tensors are B's times this factor where B's own values move the logits by less than the margin (measured on the
# oracle, fp32, by test_updates_move_the_logits_beyond_every_tolerance, which prints the figures)
SCALE: Dict = {}  # (none needed: the smallest movement is 1.8 x the margin, tiny-llama / fc_2)
PAIRS = [
    ("tiny-llama", "whole"), ("tiny-llama", "fc_2"), ("tiny-llama", "proj"),
    ("tiny-neox-hs64", "whole"), ("tiny-neox-hs64", "proj"),
    ("tiny-llama-hs128-i384", "whole"), ("tiny-llama-hs128-i384", "fc_2"),
]


def config(name: str) -> Config:
    if name == "tiny-llama-hs128-i384":  # every in_features a multiple of 64, as the NF4 Linears need (test_nf4.py)
        return Config(**{**name_to_config["tiny-llama-hs128"], "intermediate_size": 384})
    return Config.from_name(name)


@functools.lru_cache(maxsize=None)
def _weights(name: str, which: str, dtype: torch.dtype) -> Dict[str, torch.Tensor]:
    sd = synthetic_state_dict(config(name), SEED_A if which == "A" else SEED_B, perturb=True)
    return {k: v.to(torch.bfloat16).to(dtype) for k, v in sd.items()}


def weights(name: str, which: str, dtype: torch.dtype = torch.bfloat16) -> Dict[str, torch.Tensor]:
    """Weights "A" or "B" of a shape, rounded to bf16 (the checkpoint's precision) and then held in ``dtype``: computed once, the
    tensors are shared and nobody writes to them."""
    return dict(_weights(name, which, dtype))


def update_of(name: str, update: str, dtype: torch.dtype = torch.bfloat16) -> Dict[str, torch.Tensor]:
    """The tensors an update loads: all of B, or the one replaced tensor (scaled where ``SCALE`` says so)."""
    b = weights(name, "B", dtype)
    keys = UPDATES[update]
    if keys is None:
        return b
    f = SCALE.get((name, update), 1.0)
    return {k: (b[k].float() * f).to(torch.bfloat16).to(dtype) for k in keys}


def updated(name: str, update: str, dtype: torch.dtype = torch.bfloat16) -> Dict[str, torch.Tensor]:
    """The full state dict after the update: A with the update's tensors in place."""
    return {**weights(name, "A", dtype), **update_of(name, update, dtype)}


def prompt(name: str, T: int = PROMPT_T) -> torch.Tensor:
    return synthetic_prompt(config(name), T, PROMPT_SEED)
