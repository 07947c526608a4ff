"""The prompt GEMM entry points write inside the workspace their sizing functions advertise (runs on the MI355X box: ``-m gpu``).

Each C entry point is called directly on a workspace that is a slice of a larger buffer: exactly the advertised size, 64 sentinel
floats (256 bytes for int8) on each side.  Afterwards the sentinels are intact and the output equals, bit for bit, the same call
through ``ops``.  The shapes are chosen by asking parrot_gemm_plan, so that every route runs split and unsplit, and with SWIGLU
where the route takes it; the expected (route, split) of each case is asserted, so a change of heuristics cannot quietly empty a case.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from lit_parrot_amd import _hip, ops  # noqa: E402
from lit_parrot_amd._hip import EPI_NONE, EPI_RESIDUAL, EPI_SWIGLU, check, ptr, stream  # noqa: E402
from lit_parrot_amd.quantize import bnb  # noqa: E402
from lit_parrot_amd.quantize.gptq import ColBlockQuantizedLinear  # noqa: E402
from oracle import int4 as o4  # noqa: E402
from oracle import int8 as o8  # noqa: E402

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
BF16, W4, W4C = 0, 1, 2
GEN1, G2, G2_W4, G2_W4C = 0, 1, 2, 3
GUARD = 64  # floats on each side of the workspace


def gen(seed):
    return torch.Generator().manual_seed(seed)


def guarded(nbytes_or_floats, dtype, fill):
    """(whole buffer, the slice of exactly that many elements between two guards of 256 bytes)"""
    guard = GUARD * 4 // torch.empty((), dtype=dtype).element_size()
    whole = torch.full((guard + nbytes_or_floats + guard,), fill, dtype=dtype, device=DEV)
    return whole, whole[guard:guard + nbytes_or_floats], guard


def assert_guards(whole, guard, fill, what):
    assert torch.all(whole[:guard] == fill) and torch.all(whole[-guard:] == fill), f"{what}: wrote outside the advertised workspace"


def w4_packed(N, K, group, seed):
    w = (torch.randn(N, K, generator=gen(seed)) * 0.02).to(BF)
    qw, s, z = o4.rtn_quantize(w, group, BF)
    lin = ColBlockQuantizedLinear(K, N, False, bits=4, tile_cols=group)
    lin.quant_weight.copy_(qw)
    lin.scales, lin.zeros = s.clone(), z.clone()
    return lin.to(DEV).packed()


def w4c_packed(N, K, seed):
    lin = bnb.Linear4bit(K, N, False, quant_type="nf4", compress_statistics=False)
    lin.load_state_dict({"weight": (torch.randn(N, K, generator=gen(seed)) * 0.02).to(BF)})
    lin = lin.to("cuda").to(BF)
    return lin.packed(), lin._codes


# kind, M, N, K, group, epilogue, norm kind -> (route, K is split)
CASES = [
    (BF16, 40, 128, 1024, 0, EPI_NONE, 0, (G2, True)),
    (BF16, 300, 389, 512, 0, EPI_RESIDUAL, 0, (G2, False)),
    (BF16, 40, 128, 1056, 0, EPI_SWIGLU, 0, (GEN1, True)),
    (BF16, 40, 128, 96, 0, EPI_SWIGLU, 0, (GEN1, False)),
    (W4, 129, 96, 512, 64, EPI_NONE, 1, (G2_W4, True)),      # norm fused: xn and xs written by the norm launch
    (W4, 129, 96, 256, 64, EPI_RESIDUAL, 2, (G2_W4, False)),  # LayerNorm fused, one pass
    (W4, 70, 160, 512, 128, EPI_SWIGLU, 0, (G2_W4, True)),
    (W4, 70, 160, 256, 128, EPI_SWIGLU, 0, (G2_W4, False)),
    (W4, 37, 64, 256, 32, EPI_NONE, 0, (GEN1, False)),
    (W4, 37, 64, 1024, 32, EPI_SWIGLU, 0, (GEN1, True)),
    (W4C, 37, 128, 256, 64, EPI_NONE, 0, (G2_W4C, False)),
    (W4C, 40, 128, 1024, 64, EPI_SWIGLU, 0, (G2_W4C, True)),
]


@pytest.mark.parametrize("kind,M,N,K,group,epi,norm_kind,want", CASES)
def test_entry_points_stay_inside_the_advertised_workspace(kind, M, N, K, group, epi, norm_kind, want):
    lib = _hip.load()
    p = (C.c_int64 * 12)()
    assert lib.parrot_gemm_plan(kind, M, N, K, group, epi, K, 1, norm_kind, p) == 0
    assert (p[0], p[1] > 1, p[2]) == (want[0], want[1], int(norm_kind != 0)), list(p)
    g = gen(70)
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.1).to(BF).to(DEV)
    res = torch.randn(M, N, generator=g).to(BF).to(DEV) if epi == EPI_RESIDUAL else None
    swi = epi == EPI_SWIGLU
    norm = None
    if norm_kind:
        norm = ops.Norm(norm_kind, (1 + 0.1 * torch.randn(K, generator=g)).to(BF).to(DEV),
                        (0.1 * torch.randn(K, generator=g)).to(BF).to(DEV) if norm_kind == 2 else None, 1e-5)
    ref, out = (torch.full((M, N), 3.0, dtype=BF, device=DEV) for _ in range(2))
    n = lib.parrot_gemm_workspace_floats(M, N, K, group, epi)
    assert n >= p[11]
    whole, ws, guard = guarded(n, torch.float32, 12345.0)
    tail = (ptr(res), N if res is not None else 0, ptr(out), N, N, K)
    if kind == BF16:
        W, W2 = ((torch.randn(N, K, generator=g) * 0.05).to(BF).to(DEV) for _ in range(2))
        ops.bf16_linear(W, x, ref, epilogue=epi, residual=res, weight2=W2 if swi else None)
        check(lib.parrot_bf16_gemm(ptr(W), ptr(W2) if swi else None, ptr(x), K, M, None, *tail, epi, None, ptr(ws), stream()), "parrot_bf16_gemm")
    elif kind == W4:
        pk, pk2 = w4_packed(N, K, group, 71), w4_packed(N, K, group, 72) if swi else None
        ops.w4_linear(pk, N, K, group, x, ref, epilogue=epi, residual=res, packed2=pk2, norm=norm)
        check(lib.parrot_w4_gemm(ptr(pk), ptr(pk2), ptr(x), K, M, None, *tail, group, epi, C.byref(norm.c_struct(K)) if norm else None,
                                 ptr(ws), stream()), "parrot_w4_gemm")
    else:
        (pk, codes), pk2 = w4c_packed(N, K, 73), w4c_packed(N, K, 74)[0] if swi else None
        ops.w4c_linear(pk, codes[0], codes[1], N, K, group, x, ref, epilogue=epi, residual=res, packed2=pk2)
        check(lib.parrot_w4c_gemm(ptr(pk), ptr(pk2), ptr(codes[0]), ptr(x), K, M, None, *tail, group, epi, None, ptr(ws), stream()), "parrot_w4c_gemm")
    torch.cuda.synchronize()
    assert_guards(whole, guard, 12345.0, f"kind {kind} {M}x{N}x{K}")
    assert torch.equal(out, ref), f"{int((out != ref).sum())} elements differ from the call through ops"


@pytest.mark.parametrize("M,N,K,epi,split,shift", [(40, 128, 512, EPI_SWIGLU, False, 0), (40, 128, 1024, EPI_NONE, True, 0),
                                                   (40, 128, 512, EPI_SWIGLU, False, 4)])
def test_w8_entry_point_stays_inside_the_advertised_workspace(M, N, K, epi, split, shift):
    """shift: bytes by which the workspace pointer misses a 16-byte boundary - the entry point rounds it up and carves from there, and
    the advertised size has room for that."""
    lib = _hip.load()
    swi = epi == EPI_SWIGLU
    g = gen(75)
    W = (torch.randn(N * (2 if swi else 1), K, generator=g) * 0.02).to(BF)
    x = torch.randn(M, K, generator=g).to(BF)
    x[0, 3], x[M // 2, K - 1], x[M - 1, 17] = 9.5, -7.25, 6.0  # outlier columns: the fp16 operands at the end of the workspace are used
    cb, scb = (t.to(DEV) for t in o8.quantize_weight_rows(W))
    act = ops.w8_prep_act(x.to(DEV), 6.0, ops.W8Act(M, K, DEV))
    ref, out = (torch.full((M, N), 3.0, dtype=BF, device=DEV) for _ in range(2))
    ops.w8_linear(cb, scb, N, K, act, ref, epilogue=epi)
    n = lib.parrot_w8_gemm_workspace_bytes(M, N, K, epi)
    nw = 2 if swi else 1
    # more than one K range exactly when the sizing holds more than one set of int32 sums (+ one fp32 outlier part) per weight
    assert (n > 3 * M * N * 4 * nw + (M + nw * N) * K * 2) == split
    whole, ws, guard = guarded(n + shift, torch.uint8, 0xA5)
    ws = ws[shift:]  # exactly n bytes; the head guard grows by `shift`
    assert ws.numel() == n and ws.data_ptr() % 16 == shift
    check(lib.parrot_w8_gemm(ptr(cb), ptr(scb), ptr(act.xq), ptr(act.xout), ptr(act.sca), ptr(act.nout), ptr(act.oidx), M, None, None, 0,
                             ptr(out), N, N, K, epi, ptr(ws), stream()), "parrot_w8_gemm")
    torch.cuda.synchronize()
    assert_guards(whole, guard, 0xA5, f"w8 {M}x{N}x{K}")
    assert torch.all(whole[guard:guard + shift] == 0xA5)
    assert torch.equal(out, ref), f"{int((out != ref).sum())} elements differ from the call through ops"
