"""Candidates of one prompt, CPU side: generate_candidates is exported and checks its inputs before any device work, the new
attention entry point is declared, exported and refuses bad arguments without a launch, and the split rule of its two kinds of
workgroup is the one written out here."""
import pytest
import torch

import lit_parrot_amd as L
from lit_parrot_amd import _hip
from lit_parrot_amd import adapter as A
from lit_parrot_amd.config import Config
from lit_parrot_amd.generate import base as gb

P = 0x10000  # a 16-byte aligned stand-in pointer: every call below fails its checks before anything is launched


def test_generate_candidates_is_exported():
    assert callable(L.generate_candidates) and "generate_candidates" in L.__all__
    assert L.generate_candidates is gb.generate_candidates


def test_entry_point_is_declared_and_exported(hip_lib):
    from test_abi_and_host import declared_functions

    n = "parrot_attn_fused_decode_prefix"
    assert n in declared_functions() and n in _hip.SIGNATURES and hasattr(hip_lib, n)
    assert "attn_fused_decode_prefix" in [hip_lib.parrot_kernel_name(i).decode() for i in range(64)]


# ---- input checks, each before any device work (the models live on the CPU)
def tiny():
    return L.GPT(Config.from_name("tiny-llama")).to(torch.bfloat16)


@pytest.mark.parametrize("n", [0, 9])
def test_n_outside_the_batched_rows_is_refused(n):
    with pytest.raises(L.ParrotHipError, match="1 to 8"):
        L.generate_candidates(tiny(), torch.arange(4), n, 8, 8, top_k=1)


def test_a_cpu_model_is_refused():
    with pytest.raises(L.ParrotHipError, match="HIP device"):
        L.generate_candidates(tiny(), torch.arange(4), 2, 8, 8, top_k=1)


def test_a_window_shorter_than_the_result_names_the_fallback():
    with pytest.raises(L.ParrotHipError, match="generate_batch"):
        L.generate_candidates(tiny(), torch.arange(4), 2, 12, 8, top_k=1)


def test_a_model_of_another_class_is_refused():
    with pytest.raises(L.ParrotHipError, match="GPT models"):
        L.generate_candidates(torch.nn.Linear(4, 4), torch.arange(4), 2, 8, 8, top_k=1)


def test_generates_asserts_fire():
    model = tiny()
    cfg = model.config
    with pytest.raises(AssertionError):  # max_returned_tokens > T
        L.generate_candidates(model, torch.arange(8), 2, 8, 8, top_k=1)
    with pytest.raises(AssertionError):  # max_seq_length >= T
        L.generate_candidates(model, torch.arange(8), 2, 12, 6, top_k=1)
    with pytest.raises(AssertionError):  # max_seq_length <= block_size
        L.generate_candidates(model, torch.arange(4), 2, 8, cfg.block_size + 1, top_k=1)
    with pytest.raises(L.ParrotHipError, match="block_size"):
        L.generate_candidates(model, torch.arange(4), 2, cfg.block_size + 1, cfg.block_size, top_k=1)
    with pytest.raises(L.ParrotHipError, match="1-D"):
        L.generate_candidates(model, torch.zeros((2, 4), dtype=torch.int64), 2, 8, 8, top_k=1)


def test_models_outside_the_batched_step_are_declined_with_its_reason():
    with L.quantization("bnb.int8"):
        int8 = L.GPT(Config.from_name("tiny-llama"))
    adapter = A.GPT(A.Config.from_name("tiny-llama", adapter_start_layer=1))
    for model, word in ((int8, "LLM.int8"), (adapter, "adapter")):
        why = model.batched_decode_unsupported()
        assert word in why
        with pytest.raises(L.ParrotHipError) as e:
            L.generate_candidates(model, torch.arange(4), 2, 8, 8, top_k=1)
        assert why in str(e.value)


# ---- ABI: argument errors without a launch
def _attn(lib, **kw):
    # a consistent call: 2 groups x 2 query heads of 64 dims, window 32 in 2 splits, tails of 64 slots, B = 2
    a = dict(qkv=P, ldqkv=2 * 4 * 64, B=2, cos=P, sin=P, n_elem=64, pos=P, prefix_len=P, n_groups=2, q_per_kv=2, hs=64, S=32, nsplit=2,
             ws=P, tickets=P, n_tickets=2 * 4, k=P, v=P, k_tail=P, v_tail=P, S_tail=64, y=P, ldy=4 * 64, share=1, softmax_mode=0)
    a.update(kw)
    return lib.parrot_attn_fused_decode_prefix(*a.values(), None)


@pytest.mark.parametrize("bad", [dict(qkv=None), dict(pos=None), dict(prefix_len=None), dict(k=None), dict(v=None), dict(k_tail=None),
                                 dict(v_tail=None), dict(y=None), dict(B=0), dict(B=9), dict(S_tail=0), dict(S_tail=-64),
                                 dict(ldqkv=2 * 4 * 64 - 8), dict(ldqkv=2 * 4 * 64 + 4), dict(ldy=4 * 64 - 1), dict(n_tickets=7),
                                 dict(tickets=None), dict(nsplit=0), dict(softmax_mode=2), dict(k_tail=P + 8)])
def test_attn_fused_decode_prefix_rejects_bad_arguments(hip_lib, bad):
    assert _attn(hip_lib, **bad) == -1, _hip.last_error()


def test_attn_fused_decode_prefix_scope_matches_the_rows_kernel(hip_lib):
    assert _attn(hip_lib, hs=48, n_elem=48, ldqkv=2 * 4 * 48, ldy=4 * 48) == -3
    assert "head size" in _hip.last_error()
    assert _attn(hip_lib, q_per_kv=17, ldqkv=2 * 19 * 64, ldy=34 * 64, n_tickets=2 * 34) == -3  # FUSED_ATTN_MAX_Q_PER_KV
    assert "query heads" in _hip.last_error()
    assert _attn(hip_lib, softmax_mode=1) == -3  # softmax_mode 1: one split only, as the rows call


# ---- geometry: which splits are shared, and the arrivals per ticket
def restated(S, nsplit, T):
    """The rule in plain words: split j covers slots [j * per, (j + 1) * per); it is shared when all of them are prompt slots
    (< T).  With T <= S - 1 that never holds for the last split, which reaches slot S - 1."""
    per = (S + nsplit - 1) // nsplit
    return [j for j in range(nsplit) if all(s < T for s in range(j * per, (j + 1) * per))]


GEOMETRY = {  # (S, nsplit): {T: shared splits}; per = 32 and 160
    (96, 3): {0: [], 1: [], 31: [], 32: [0], 33: [0], 95: [0, 1]},
    (320, 2): {0: [], 1: [], 159: [], 160: [0], 161: [0], 319: [0]},
}


@pytest.mark.parametrize("S,nsplit", list(GEOMETRY))
def test_shared_splits_and_ticket_arrivals(S, nsplit):
    per = -(-S // nsplit)
    assert sorted(GEOMETRY[(S, nsplit)]) == [0, 1, per - 1, per, per + 1, S - 1]
    for T, want in GEOMETRY[(S, nsplit)].items():
        assert gb.shared_splits(S, nsplit, T) == want == restated(S, nsplit, T), (S, nsplit, T)
        first, second = gb.ticket_arrivals(S, nsplit, T)
        assert first == len(want) and first + second == nsplit and second >= 1  # the per-row launch arrives last and merges
        assert gb.ticket_arrivals(S, nsplit, T, share=False) == (0, nsplit)
    # the split that holds any position p >= T is never shared
    for T in GEOMETRY[(S, nsplit)]:
        for p in range(T, S):
            assert p // per not in gb.shared_splits(S, nsplit, T)
    assert gb.shared_splits(S, 1, S - 1) == [] and gb.ticket_arrivals(S, 1, S - 1) == (0, 1)
    assert gb.shared_splits(S, nsplit, 10 ** 6) == gb.shared_splits(S, nsplit, S)  # T is clamped to the window
    assert gb.shared_splits(S, nsplit, -5) == []


def test_tail_slots_are_rounded_up_to_the_bucket():
    assert [gb.candidate_tail_slots(90, T) for T in (89, 70, 26, 25, 20)] == [64, 64, 64, 128, 128]
