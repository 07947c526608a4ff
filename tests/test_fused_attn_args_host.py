"""The five fused decode-attention entry points refuse the same bad calls in the same words (no GPU: every call below fails
its checks before anything is launched).  One table of single faults, run against every entry point that has the argument:
the return code, the entry point's name in front of the message and the fragment that names the fault."""
import pytest

from lit_parrot_amd import _hip

P = 0x10000  # a 16-byte aligned stand-in pointer
EINVAL, EUNSUPPORTED = -1, -3

# a consistent call of each entry point, in the order of its C arguments (the stream follows): 2 groups x 2 query heads of 64
# dims, a window of 32 slots in 2 splits; 2 rows where the call has rows
_ONE = dict(qkv=P, cos=P, sin=P, n_elem=64, pos=P, n_groups=2, q_per_kv=2, hs=64, S=32, nsplit=2, ws=P, tickets=P, k=P, v=P, y=P)
_ROWS = dict(qkv=P, ldqkv=512, B=2, cos=P, sin=P, n_elem=64, pos=P, n_groups=2, q_per_kv=2, hs=64, S=32, nsplit=2, ws=P, tickets=P,
             n_tickets=8, k=P, v=P)
CALLS = {
    "attn_fused_decode": dict(_ONE, softmax_mode=0),
    "attn_fused_decode_adapter": dict(_ONE, ak=P, av=P, gate=P, aT=10, softmax_mode=0),
    "attn_fused_decode_rows": dict(_ROWS, kv_bstride=2 * 32 * 64, y=P, ldy=256, softmax_mode=0),
    "attn_fused_decode_seq": dict(_ROWS, y=P, ldy=256, softmax_mode=0),
    "attn_fused_decode_prefix": dict(qkv=P, ldqkv=512, B=2, cos=P, sin=P, n_elem=64, pos=P, prefix_len=P, n_groups=2, q_per_kv=2, hs=64,
                                     S=32, nsplit=2, ws=P, tickets=P, n_tickets=8, k=P, v=P, k_tail=P, v_tail=P, S_tail=64, y=P, ldy=256,
                                     share=1, softmax_mode=0),
}
ROWS_OF_THE_TABLE = {"attn_fused_decode": 23, "attn_fused_decode_adapter": 28, "attn_fused_decode_rows": 31, "attn_fused_decode_seq": 29,
                     "attn_fused_decode_prefix": 35}  # how many of FAULTS each entry point has the argument for
FAULTS = [  # (what is wrong - the first key, the others keep the rest of the call consistent -, return code, fragment of the message)
    (dict(qkv=None), EINVAL, "null pointer"), (dict(pos=None), EINVAL, "null pointer"), (dict(k=None), EINVAL, "null pointer"),
    (dict(v=None), EINVAL, "null pointer"), (dict(y=None), EINVAL, "null pointer"), (dict(prefix_len=None), EINVAL, "null pointer"),
    (dict(k_tail=None), EINVAL, "null pointer"), (dict(v_tail=None), EINVAL, "null pointer"), (dict(ak=None), EINVAL, "null adapter pointer"),
    (dict(gate=None), EINVAL, "null adapter pointer"),
    (dict(n_groups=0), EINVAL, "bad shape"), (dict(q_per_kv=0), EINVAL, "bad shape"), (dict(S=0), EINVAL, "bad shape"),
    (dict(S_tail=0), EINVAL, "S_tail=0"), (dict(aT=0), EINVAL, "aT=0"), (dict(aT=65), EUNSUPPORTED, "adapter_prompt_length"),
    (dict(B=0), EINVAL, "B=0 (1 .. 8)"), (dict(B=9, n_tickets=36), EINVAL, "B=9 (1 .. 8)"),
    (dict(softmax_mode=2), EINVAL, "softmax_mode must be 0 or 1"), (dict(softmax_mode=1), EUNSUPPORTED, "softmax_mode 1"),
    (dict(q_per_kv=17, ldqkv=2 * 19 * 64, ldy=34 * 64, n_tickets=2 * 34), EUNSUPPORTED, "query heads"),
    (dict(hs=48, n_elem=48), EUNSUPPORTED, "head size 48 not built"),
    (dict(n_elem=3), EINVAL, "n_elem=3"), (dict(n_elem=66), EINVAL, "n_elem=66"), (dict(cos=None), EINVAL, "rope tables"),
    (dict(sin=None), EINVAL, "rope tables"), (dict(nsplit=0), EINVAL, "nsplit"), (dict(nsplit=65536), EINVAL, "nsplit"),
    (dict(ws=None), EINVAL, "workspace and tickets"), (dict(tickets=None), EINVAL, "workspace and tickets"),
    (dict(n_tickets=7), EINVAL, "7 tickets"), (dict(ldqkv=504), EINVAL, "ldqkv=504"), (dict(ldqkv=516), EINVAL, "ldqkv=516"),
    (dict(ldy=255), EINVAL, "ldy=255"), (dict(kv_bstride=4088), EINVAL, "kv_bstride=4088"), (dict(kv_bstride=4100), EINVAL, "kv_bstride=4100"),
    (dict(qkv=P + 8), EINVAL, "16-byte alignment"), (dict(k=P + 8), EINVAL, "16-byte alignment"), (dict(v=P + 8), EINVAL, "16-byte alignment"),
    (dict(k_tail=P + 8), EINVAL, "16-byte alignment"), (dict(v_tail=P + 8), EINVAL, "16-byte alignment"), (dict(av=P + 8), EINVAL, "16-byte aligned"),
]


@pytest.mark.parametrize("entry", list(CALLS))
def test_every_fused_entry_point_refuses_the_table(hip_lib, entry):
    fn, base, n = getattr(hip_lib, "parrot_" + entry), CALLS[entry], 0
    assert len(base) + 1 == len(_hip.SIGNATURES["parrot_" + entry][1])  # every C argument, and the stream
    # the adapter entry point is its own checks, then the one-row call: what that call refuses carries the one-row name
    who = (entry + ": ", "attn_fused_decode: ") if entry == "attn_fused_decode_adapter" else (entry + ": ",)
    for bad, rc, fragment in FAULTS:
        if next(iter(bad)) not in base:
            continue  # the entry point has no such argument
        call = dict(base, **{k: v for k, v in bad.items() if k in base})
        assert fn(*call.values(), None) == rc, (bad, _hip.last_error())
        assert _hip.last_error().startswith(who) and fragment in _hip.last_error(), (bad, _hip.last_error())
        n += 1
    assert n == ROWS_OF_THE_TABLE[entry]


def test_consecutive_rows_must_fit_the_cache(hip_lib):
    call = dict(CALLS["attn_fused_decode_seq"], B=8, S=4, n_tickets=32)
    assert hip_lib.parrot_attn_fused_decode_seq(*call.values(), None) == EINVAL
    assert _hip.last_error() == "attn_fused_decode_seq: M=8 rows do not fit a cache of 4 slots"
