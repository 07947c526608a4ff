"""Batched decode, CPU side: the new entry points are declared and exported, refuse bad arguments without a device, and
generate_batch / GPT.batched_decode_unsupported check their inputs before any device work."""
import pytest
import torch

import lit_parrot_amd as L
from lit_parrot_amd import _hip
from lit_parrot_amd import adapter as A
from lit_parrot_amd.config import Config, name_to_config

NEW = ["parrot_attn_fused_decode_rows", "parrot_embedding_rows", "parrot_argmax_advance_rows", "parrot_topk_sample_rows"]
P = 0x10000  # a 16-byte aligned stand-in pointer: every call below fails its checks before anything is launched


def test_new_entry_points_are_declared_and_exported(hip_lib):
    from test_abi_and_host import declared_functions

    for n in NEW:
        assert n in declared_functions() and n in _hip.SIGNATURES and hasattr(hip_lib, n), n
    names = [hip_lib.parrot_kernel_name(i).decode() for i in range(64)]
    for k in ("attn_fused_decode_rows", "embedding_rows", "argmax_advance_rows", "topk_sample_rows"):
        assert k in names, k


def _attn(lib, **kw):
    # a consistent call: 2 groups x 2 query heads of 64 dims, window 32, 2 splits, B = 2
    a = dict(qkv=P, ldqkv=2 * 4 * 64, B=2, cos=P, sin=P, n_elem=64, pos=P, n_groups=2, q_per_kv=2, hs=64, S=32, nsplit=2, ws=P,
             tickets=P, n_tickets=2 * 4, k=P, v=P, kv_bstride=2 * 32 * 64, y=P, ldy=4 * 64, softmax_mode=0)
    a.update(kw)
    return lib.parrot_attn_fused_decode_rows(*a.values(), None)


@pytest.mark.parametrize("bad", [dict(B=0), dict(B=9), dict(pos=None), dict(qkv=None), dict(ldqkv=2 * 4 * 64 - 8), dict(ldqkv=2 * 4 * 64 + 4),
                                 dict(ldy=4 * 64 - 1), dict(kv_bstride=2 * 32 * 64 - 8), dict(kv_bstride=2 * 32 * 64 + 4),
                                 dict(n_tickets=7), dict(tickets=None), dict(nsplit=0), dict(softmax_mode=2)])
def test_attn_fused_decode_rows_rejects_bad_arguments(hip_lib, bad):
    assert _attn(hip_lib, **bad) == -1, _hip.last_error()


def test_attn_fused_decode_rows_scope_matches_the_one_row_kernel(hip_lib):
    assert _attn(hip_lib, q_per_kv=17, ldqkv=2 * 19 * 64, ldy=34 * 64, n_tickets=2 * 34) == -3  # FUSED_ATTN_MAX_Q_PER_KV
    assert "query heads" in _hip.last_error()
    assert _attn(hip_lib, hs=80, n_elem=80, ldqkv=2 * 4 * 80, ldy=4 * 80, kv_bstride=2 * 32 * 80) == -3
    assert _attn(hip_lib, softmax_mode=1) == -3  # softmax_mode 1: one split only, as the one-row call
    assert hip_lib.parrot_attn_workspace_floats(3, 8, 64, 2) == 3 * hip_lib.parrot_attn_workspace_floats(1, 8, 64, 2)


@pytest.mark.parametrize("bad", [dict(B=0), dict(B=9), dict(tokens=None), dict(ld_tokens=0), dict(ldo=60), dict(d=60, ldo=64)])
def test_embedding_rows_rejects_bad_arguments(hip_lib, bad):
    a = dict(wte=P, d=64, tokens=P, ld_tokens=8, pos=P, B=2, out=P, ldo=64)
    a.update(bad)
    assert hip_lib.parrot_embedding_rows(*a.values(), None) == -1, _hip.last_error()


@pytest.mark.parametrize("bad", [dict(B=0), dict(B=9), dict(pos=None), dict(end=None), dict(tokens=None), dict(ldl=99), dict(ldt=1),
                                 dict(eos_id=-2)])
def test_sampling_rows_reject_bad_arguments(hip_lib, bad):
    a = dict(logits=P, V=100, ldl=104, B=2, tokens=P, ldt=16, pos=P, end=P, eos_id=-1)
    a.update(bad)
    assert hip_lib.parrot_argmax_advance_rows(*a.values(), None) == -1, _hip.last_error()
    t = dict(logits=a["logits"], V=a["V"], ldl=a["ldl"], B=a["B"], temperature=0.8, top_k=5, noise=P, tokens=a["tokens"], ldt=a["ldt"],
             pos=a["pos"], end=a["end"], eos_id=a["eos_id"])
    assert hip_lib.parrot_topk_sample_rows(*t.values(), None) == -1, _hip.last_error()


def test_topk_sample_rows_needs_noise_and_a_positive_temperature(hip_lib):
    a = dict(logits=P, V=100, ldl=104, B=2, temperature=0.8, top_k=5, noise=None, tokens=P, ldt=16, pos=P, end=P, eos_id=-1)
    assert hip_lib.parrot_topk_sample_rows(*a.values(), None) == -1
    a.update(noise=P, temperature=0.0)
    assert hip_lib.parrot_topk_sample_rows(*a.values(), None) == -1 and "temperature" in _hip.last_error()


def test_generate_batch_checks_its_arguments_without_a_device():
    cfg = Config.from_name("tiny-llama")
    model = L.GPT(cfg).to(torch.bfloat16)
    p = torch.arange(4)
    with pytest.raises(L.ParrotHipError, match="empty"):
        L.generate_batch(model, [p, torch.zeros(0, dtype=torch.int64)], 8, 8, top_k=1)
    with pytest.raises(L.ParrotHipError, match="1 to 8"):
        L.generate_batch(model, [p] * 9, 8, 8, top_k=1)
    with pytest.raises(L.ParrotHipError, match="1 to 8"):
        L.generate_batch(model, [], 8, 8, top_k=1)
    with pytest.raises(AssertionError):  # generate()'s max_returned_tokens > T, row by row
        L.generate_batch(model, [p, torch.arange(8)], 8, 8, top_k=1)
    with pytest.raises(AssertionError):  # max_seq_length >= T
        L.generate_batch(model, [p, torch.arange(8)], 12, 6, top_k=1)
    with pytest.raises(L.ParrotHipError, match="block_size"):
        L.generate_batch(model, [p], cfg.block_size + 1, cfg.block_size, top_k=1)
    with pytest.raises(L.ParrotHipError, match="HIP device"):
        L.generate_batch(model, [p, p + 1], 8, 8, top_k=1)
    with pytest.raises(L.ParrotHipError, match="HIP device"):
        L.generate_batch(model, torch.stack([p, p + 1]), 8, 8, top_k=1)
    with pytest.raises(L.ParrotHipError, match=r"\(B, T\)"):
        L.generate_batch(model, torch.zeros((2, 2, 2), dtype=torch.int64), 8, 8, top_k=1)


def test_models_outside_the_batched_step_are_named():
    assert L.GPT(Config.from_name("tiny-llama")).batched_decode_unsupported() is None
    assert L.GPT(Config.from_name("tiny-falcon-mqa")).batched_decode_unsupported() is None
    wide = Config(**{**name_to_config["tiny-falcon-7b"], "name": "tiny-falcon-7b-wide", "n_head": 18, "n_embd": 18 * 32})
    assert wide.q_per_kv == 18 and "query heads" in L.GPT(wide).batched_decode_unsupported()
    assert "adapter" in A.GPT(A.Config.from_name("tiny-llama", adapter_start_layer=1)).batched_decode_unsupported()
    with L.quantization("bnb.int8"):
        int8 = L.GPT(Config.from_name("tiny-llama"))
    assert "LLM.int8" in int8.batched_decode_unsupported()
