"""LLaMA-Adapter (v1) models behind the reference's ``lit_gpt.adapter`` surface, executed by the HIP kernels.

Interface (reference lit_gpt/adapter.py): ``Config`` with ``adapter_prompt_length`` / ``adapter_start_layer`` (:26-29);
``GPT`` with ``adapter_kv_caches`` cleared by ``reset_cache`` (:54-56); ``Block(config, block_idx)`` and
``CausalSelfAttention(config, block_idx)`` whose ``forward`` take and return the ``adapter_kv_cache`` (3-tuples, :125-261);
a layer with ``block_idx >= adapter_start_layer`` owns ``adapter_wte`` (aT prefix embeddings) and ``gating_factor``
(1, n_head, 1, 1).  Module and parameter names are the reference's, so its adapter checkpoints load by key.

The prefix of a layer: keys / values = the layer's own QKV Linear (adapter-v2 affine included, no norm, no RoPE) applied
to ``adapter_wte.weight``; every roped query row attends to all aT of them with a softmax of its own, and
``y = y + gating_factor * ay`` before ``proj``.  Here that term is added by the attention kernels themselves: a decode
step keeps ONE attention launch per layer (``parrot_attn_fused_decode_adapter``), prompts and the other multi-row paths
add it with one launch after the attention (``parrot_attn_adapter_prefix``).

Deliberate differences from the reference (documented in DESIGN.md): the prefix keys / values are GQA-native
``(1, n_query_groups, aT, head_size)`` (the reference expands them to n_head with repeat_interleave, :240-243), like the
KV cache.  They live in persistent per-layer buffers that are refilled IN PLACE - never reallocated - at the first call
after construction or ``reset_cache()`` (and by every call without a KV cache, which the reference also recomputes), so a
captured decode step always reads the current prefix.
"""
from dataclasses import dataclass
from typing import Any, List, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import ops
from ._hip import ParrotHipError
from .config import Config as BaseConfig
from .model import GPT as BaseModel
from .model import Block as BaseBlock
from .model import CausalSelfAttention as BaseCausalSelfAttention
from .model import KVCache, RoPECache, Workspace, _linear, norm_class


@dataclass
class Config(BaseConfig):
    adapter_prompt_length: int = 10
    adapter_start_layer: int = 2


class GPT(BaseModel):
    """``model.GPT`` whose blocks know their index and whose adapted layers carry a gated prefix."""

    def __init__(self, config: Config) -> None:
        nn.Module.__init__(self)
        assert config.padded_vocab_size is not None
        self.config = config
        self.lm_head = nn.Linear(config.n_embd, config.padded_vocab_size, bias=False)
        self.transformer = nn.ModuleDict(
            dict(
                wte=nn.Embedding(config.padded_vocab_size, config.n_embd),
                h=nn.ModuleList(Block(config, i) for i in range(config.n_layer)),
                ln_f=norm_class(config)(config.n_embd, eps=config.norm_eps),
            )
        )
        self.rope_cache: Optional[RoPECache] = None
        self.mask_cache: Optional[torch.Tensor] = None
        self.kv_caches: List[KVCache] = []
        # per layer: the prefix (keys, values) views (1, n_groups, aT, hs) of the persistent buffers, None for a plain layer;
        # empty = to be (re)filled before the next step
        self.adapter_kv_caches: List[Optional[KVCache]] = []
        self._workspaces = {}

    @classmethod
    def from_name(cls, name: str, **kwargs: Any) -> "GPT":
        return cls(Config.from_name(name, **kwargs))

    def reset_cache(self) -> None:
        super().reset_cache()
        self.adapter_kv_caches.clear()

    def fill_adapter_prefix(self, device) -> None:
        """(Re)compute every adapted layer's prefix keys / values from the current weights into its persistent buffers."""
        if torch.cuda.is_current_stream_capturing():
            raise ParrotHipError("the adapter prefix must be filled before a decode step is captured")
        for block in self.transformer.h:
            block.attn.fill_prefix(device)
        self.adapter_kv_caches = [block.attn.prefix_kv() for block in self.transformer.h]

    def run_rows(self, ws: Workspace, tokens: torch.Tensor, tok_pos: Optional[torch.Tensor], pos: torch.Tensor, S: int,
                 caches: List[KVCache], rope: RoPECache, *, rope_local: bool = False, pos_is_zero: bool = False) -> torch.Tensor:
        if not self.adapter_kv_caches:  # first call after construction / reset_cache(): outside any capture (prefill, warm-up)
            self.fill_adapter_prefix(ws.x.device)
        return super().run_rows(ws, tokens, tok_pos, pos, S, caches, rope, rope_local=rope_local, pos_is_zero=pos_is_zero)

    def forward(self, idx: torch.Tensor, max_seq_length: Optional[int] = None, input_pos: Optional[torch.Tensor] = None,
                lm_head_chunk_size: int = 0) -> Union[torch.Tensor, List[torch.Tensor]]:
        if input_pos is None and idx.is_cuda:
            self.fill_adapter_prefix(idx.device)  # the reference recomputes the prefix in every call without a KV cache
        out = super().forward(idx, max_seq_length, input_pos)
        if lm_head_chunk_size > 0:
            return list(out.split(lm_head_chunk_size, dim=1))
        return out


class Block(BaseBlock):
    """``model.Block`` with the adapter attention; ``forward`` passes the prefix through like the reference (:125-160)."""

    def __init__(self, config: Config, block_idx: int) -> None:
        nn.Module.__init__(self)
        self.norm_1 = norm_class(config)(config.n_embd, eps=config.norm_eps)
        self.attn = CausalSelfAttention(config, block_idx)
        if not config.shared_attention_norm:
            self.norm_2 = norm_class(config)(config.n_embd, eps=config.norm_eps)
        from .model import GptNeoxMLP, LLaMAMLP

        self.mlp = LLaMAMLP(config) if config._mlp_class == "LLaMAMLP" else GptNeoxMLP(config)
        self.config = config

    def forward(self, x: torch.Tensor, rope: RoPECache, max_seq_length: int, mask: Optional[torch.Tensor] = None,
                input_pos: Optional[torch.Tensor] = None, kv_cache: Optional[KVCache] = None,
                adapter_kv_cache: Optional[KVCache] = None) -> Tuple[torch.Tensor, Optional[KVCache], Optional[KVCache]]:
        with self.attn.using_prefix(adapter_kv_cache, x.device) as adapter_kv_cache:
            out, kv_cache = super().forward(x, rope, max_seq_length, mask, input_pos, kv_cache)
        return out, kv_cache, adapter_kv_cache


class _PrefixScope:
    """Run an attention module with a given (or freshly computed) prefix, then restore its persistent one."""

    def __init__(self, attn: "CausalSelfAttention", adapter_kv_cache: Optional[KVCache], device) -> None:
        self.attn, self.kv, self.device = attn, adapter_kv_cache, device

    def __enter__(self) -> Optional[KVCache]:
        a = self.attn
        self.saved = a._prefix_kv
        if not a.adapted:
            return self.kv
        if self.kv is None:
            a._prefix_kv = None
            a.fill_prefix(self.device)
            self.kv = a.prefix_kv()
        else:
            ak, av = self.kv
            a._prefix_kv = (ak.reshape(ak.shape[-3:]), av.reshape(av.shape[-3:]))
        return self.kv

    def __exit__(self, *exc) -> None:
        self.attn._prefix_kv = self.saved


class CausalSelfAttention(BaseCausalSelfAttention):
    """``model.CausalSelfAttention`` plus the gated attention over the adaption prompt (:165-261)."""

    def __init__(self, config: Config, block_idx: int) -> None:
        super().__init__(config)
        if block_idx >= config.adapter_start_layer:
            self.adapter_wte = nn.Embedding(config.adapter_prompt_length, config.n_embd)
            self.gating_factor = nn.Parameter(torch.zeros(1, config.n_head, 1, 1))
        self.block_idx = block_idx
        self._prefix_kv: Optional[Tuple[torch.Tensor, torch.Tensor]] = None  # persistent (n_groups, aT, hs) keys / values

    @property
    def adapted(self) -> bool:
        return self.block_idx >= self.config.adapter_start_layer

    def fill_prefix(self, device) -> None:
        """Prefix keys / values = this layer's QKV Linear (with its adapter-v2 affine, without norm) over ``adapter_wte``,
        split per query group with no RoPE (:234-243) - written in place into the persistent buffers."""
        if not self.adapted:
            return
        c = self.config
        aT = c.adapter_prompt_length
        shape = (c.n_query_groups, aT, c.head_size)
        kv = self._prefix_kv
        if kv is None or kv[0].device != torch.device(device) or tuple(kv[0].shape) != shape:
            kv = self._prefix_kv = tuple(torch.empty(shape, dtype=torch.bfloat16, device=device) for _ in range(2))
        wte = self.adapter_wte.weight.data
        if wte.dtype != torch.bfloat16 or not wte.is_cuda:
            raise ParrotHipError("adapter_wte must be bf16 on the HIP device: convert the model with .to(torch.bfloat16).to('cuda')")
        aqkv = torch.empty((aT, c.qkv_size), dtype=torch.bfloat16, device=device)
        _linear(self.attn, wte, aqkv)
        # the split of parrot_qkv_rope_kvappend with a rotary width of 0: q / k / v copied as they are, slot m = row m
        q = torch.empty((aT, c.n_head * c.head_size), dtype=torch.bfloat16, device=device)
        zero = torch.zeros((1,), dtype=torch.int32, device=device)
        unused = torch.zeros((8,), dtype=torch.float16, device=device)  # RoPE tables: not read with n_elem = 0
        ops.rope_kvappend(aqkv, unused, unused, 0, zero, c.n_query_groups, c.q_per_kv, c.head_size, aT, q, kv[0], kv[1])

    def prefix_kv(self) -> Optional[KVCache]:
        """The prefix as the ``adapter_kv_cache`` of the reference's forward, GQA-native: (1, n_groups, aT, hs) views."""
        if not self.adapted or self._prefix_kv is None:
            return None
        return self._prefix_kv[0].unsqueeze(0), self._prefix_kv[1].unsqueeze(0)

    def adapter_prefix(self) -> Optional[ops.AdapterPrefix]:
        if not self.adapted:
            return None
        if self._prefix_kv is None:
            raise ParrotHipError("adapter layer without its prefix: run the model through GPT.forward / generate()")
        return ops.AdapterPrefix(self._prefix_kv[0], self._prefix_kv[1], self.gating_factor.data.reshape(-1))

    def using_prefix(self, adapter_kv_cache: Optional[KVCache], device) -> _PrefixScope:
        return _PrefixScope(self, adapter_kv_cache, device)

    def forward(self, x: torch.Tensor, rope: RoPECache, max_seq_length: int, mask: Optional[torch.Tensor] = None,
                input_pos: Optional[torch.Tensor] = None, kv_cache: Optional[KVCache] = None,
                adapter_kv_cache: Optional[KVCache] = None) -> Tuple[torch.Tensor, Optional[KVCache], Optional[KVCache]]:
        with self.using_prefix(adapter_kv_cache, x.device) as adapter_kv_cache:
            y, kv_cache = super().forward(x, rope, max_seq_length, mask, input_pos, kv_cache)
        return y, kv_cache, adapter_kv_cache


def adapter_filter(key: str, value: Any) -> bool:
    """True for the parameters LLaMA-Adapter trains (the prefix embeddings and the gates)."""
    return any(s in key for s in ("adapter_wte", "gating_factor"))


def mark_only_adapter_as_trainable(model: nn.Module) -> None:
    """requires_grad only on the adapter parameters."""
    for name, param in model.named_parameters():
        param.requires_grad = adapter_filter(name, param)
