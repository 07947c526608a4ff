"""parrot_gemm_plan: one plan decides route, split and workspace layout of every prompt GEMM - checked on the host, no GPU.

What each region must hold is restated here from the kernels' write sets, independently of csrc/gemm_plan.h:
  xn     M x K bf16                        norm_kernel<.., true> writes the normalised rows with leading dimension K
  xs     ceil(M / 128) * 128 x ngroups     gemm2_xsum_kernel / the fused norm, [group][row] with rows padded to the 128-row tile
         M x ngroups                       gemm_xsum_kernel (first-generation route); nothing for codebooks and bf16
  part   ksplit x M x N                    the SPLIT instantiations, only when ksplit > 1
  part2  ksplit x M x N                    the same for the second weight of a split SWIGLU call
"""
import ctypes as C
import itertools
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

EPI_NONE, EPI_RESIDUAL, EPI_GELU, EPI_SWIGLU = 0, 1, 2, 3
BF16, W4, W4C = 0, 1, 2
GEN1, G2, G2_W4, G2_W4C = 0, 1, 2, 3
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
FIELDS = ("route", "ksplit", "norm_fused", "xn_off", "xn_len", "xs_off", "xs_len", "part_off", "part_len", "part2_off", "part2_len", "total")

# (kind, N, K, group, epilogue, [(route, tile, ksplit, parrot_gemm_workspace_floats) at M = 9, 32, 128, 512, 2048]) as the commit before the
# plan computed them: the Linears of Llama-2-7B (int4 g128 and bf16), StableLM-3B (bf16), Falcon-40B (int4 g128) and Falcon-7B
# (int4, per-channel scales), each with the epilogues the model uses on it
PINNED_M = (9, 32, 128, 512, 2048)
PINNED = [
    (1, 12288, 4096, 128, 0, [(2, 128, 5, 885024), (2, 128, 5, 3146752), (2, 128, 5, 8130560), (2, 128, 1, 1064960), (2, 128, 1, 4259840)]),  # llama2-7b qkv
    (1, 4096, 4096, 128, 1, [(2, 128, 8, 317440), (2, 128, 8, 1118208), (2, 128, 8, 4460544), (2, 128, 4, 9453568), (2, 128, 1, 16842752)]),  # llama2-7b attn.proj
    (1, 11008, 4096, 128, 3, [(2, 128, 5, 1585440), (2, 128, 5, 5637120), (2, 128, 5, 14356480), (2, 128, 1, 1064960), (2, 128, 1, 4259840)]),  # llama2-7b fc
    (1, 4096, 11008, 128, 1, [(2, 128, 8, 355456), (2, 128, 8, 1235712), (2, 128, 8, 4909824), (2, 128, 4, 11250688), (2, 128, 1, 16953344)]),  # llama2-7b mlp.proj
    (1, 32000, 4096, 128, 0, [(2, 128, 2, 598528), (2, 128, 2, 2117632), (2, 128, 2, 8458240), (2, 128, 1, 1064960), (2, 128, 1, 4259840)]),  # llama2-7b lm_head
    (0, 12288, 4096, 0, 0, [(1, 128, 5, 884736), (1, 128, 5, 3145728), (1, 128, 5, 7864320), (1, 256, 1, 0), (1, 256, 1, 0)]),  # llama2-7b qkv
    (0, 4096, 4096, 0, 1, [(1, 128, 8, 294912), (1, 128, 8, 1048576), (1, 128, 8, 4194304), (1, 256, 4, 8388608), (1, 256, 1, 16777216)]),  # llama2-7b attn.proj
    (0, 11008, 4096, 0, 3, [(0, 64, 8, 1585152), (0, 64, 8, 5636096), (0, 64, 4, 11272192), (0, 64, 1, 0), (0, 128, 1, 0)]),  # llama2-7b fc
    (0, 4096, 11008, 0, 1, [(1, 128, 8, 294912), (1, 128, 8, 1048576), (1, 128, 8, 4194304), (1, 256, 4, 8388608), (1, 256, 1, 16777216)]),  # llama2-7b mlp.proj
    (0, 32000, 4096, 0, 0, [(1, 128, 2, 576000), (1, 128, 2, 2048000), (1, 128, 2, 8192000), (1, 256, 1, 0), (1, 256, 1, 0)]),  # llama2-7b lm_head
    (0, 12288, 4096, 0, 0, [(1, 128, 5, 884736), (1, 128, 5, 3145728), (1, 128, 5, 7864320), (1, 256, 1, 0), (1, 256, 1, 0)]),  # stablelm-3b qkv
    (0, 4096, 4096, 0, 1, [(1, 128, 8, 294912), (1, 128, 8, 1048576), (1, 128, 8, 4194304), (1, 256, 4, 8388608), (1, 256, 1, 16777216)]),  # stablelm-3b attn.proj
    (0, 16384, 4096, 0, 2, [(1, 128, 4, 589824), (1, 128, 4, 2097152), (1, 128, 4, 8388608), (1, 256, 1, 16777216), (1, 256, 1, 0)]),  # stablelm-3b fc
    (0, 4096, 16384, 0, 1, [(1, 128, 8, 294912), (1, 128, 8, 1048576), (1, 128, 8, 4194304), (1, 256, 4, 8388608), (1, 256, 1, 16777216)]),  # stablelm-3b mlp.proj
    (0, 4096, 16384, 0, 0, [(1, 128, 8, 294912), (1, 128, 8, 1048576), (1, 128, 8, 4194304), (1, 256, 4, 8388608), (1, 256, 1, 16777216)]),  # stablelm-3b mlp.proj
    (0, 50688, 4096, 0, 0, [(1, 128, 1, 0), (1, 128, 1, 0), (1, 128, 1, 0), (1, 256, 1, 0), (1, 256, 1, 0)]),  # stablelm-3b lm_head
    (1, 9216, 8192, 128, 0, [(2, 128, 7, 664128), (2, 128, 7, 2361344), (2, 128, 7, 8790016), (2, 128, 1, 2129920), (2, 128, 1, 8519680)]),  # falcon-40b qkv
    (1, 8192, 8192, 128, 1, [(2, 128, 8, 634880), (2, 128, 8, 2236416), (2, 128, 8, 8921088), (2, 128, 2, 10518528), (2, 128, 1, 8519680)]),  # falcon-40b attn.proj
    (1, 32768, 8192, 128, 2, [(2, 128, 2, 634880), (2, 128, 2, 2236416), (2, 128, 2, 8921088), (2, 128, 1, 2129920), (2, 128, 1, 8519680)]),  # falcon-40b fc
    (1, 8192, 32768, 128, 1, [(2, 128, 8, 770048), (2, 128, 8, 2654208), (2, 128, 8, 10518528), (2, 128, 2, 16908288), (2, 128, 1, 34078720)]),  # falcon-40b mlp.proj
    (1, 8192, 32768, 128, 0, [(2, 128, 8, 770048), (2, 128, 8, 2654208), (2, 128, 8, 10518528), (2, 128, 2, 16908288), (2, 128, 1, 34078720)]),  # falcon-40b mlp.proj
    (1, 65024, 8192, 128, 0, [(2, 128, 1, 45056), (2, 128, 1, 139264), (2, 128, 1, 532480), (2, 128, 1, 2129920), (2, 128, 1, 8519680)]),  # falcon-40b lm_head
    (1, 4672, 4544, -1, 0, [(2, 128, 1, 128), (2, 128, 1, 128), (2, 128, 1, 128), (2, 128, 1, 512), (2, 128, 1, 2048)]),  # falcon-7b qkv
    (1, 4544, 4544, -1, 1, [(2, 128, 1, 128), (2, 128, 1, 128), (2, 128, 1, 128), (2, 128, 1, 512), (2, 128, 1, 2048)]),  # falcon-7b attn.proj
    (1, 18176, 4544, -1, 2, [(2, 128, 1, 128), (2, 128, 1, 128), (2, 128, 1, 128), (2, 128, 1, 512), (2, 128, 1, 2048)]),  # falcon-7b fc
    (1, 4544, 18176, -1, 1, [(2, 128, 1, 128), (2, 128, 1, 128), (2, 128, 1, 128), (2, 128, 1, 512), (2, 128, 1, 2048)]),  # falcon-7b mlp.proj
    (1, 4544, 18176, -1, 0, [(2, 128, 1, 128), (2, 128, 1, 128), (2, 128, 1, 128), (2, 128, 1, 512), (2, 128, 1, 2048)]),  # falcon-7b mlp.proj
    (1, 65024, 4544, -1, 0, [(2, 128, 1, 128), (2, 128, 1, 128), (2, 128, 1, 128), (2, 128, 1, 512), (2, 128, 1, 2048)]),  # falcon-7b lm_head
]

# (kind, N, K, group): the shapes of tests/test_kernels_gpu.py and tests/test_nf4.py, then one of each model Linear above
SHAPES = [(W4, 96, 512, 128), (W4, 256, 4096, 128), (W4, 200, 352, 128), (W4, 128, 256, -1), (W4, 64, 256, 32), (W4, 130, 11008, 128),
          (W4, 72, 4544, -1), (W4, 2048, 256, 128), (W4, 2048, 256, 64), (W4, 2048, 256, -1), (W4, 96, 512, 64), (W4, 2048, 11008, 128),
          (W4, 8192, 2048, 128), (W4, 160, 512, 128),
          (BF16, 64, 128, 0), (BF16, 300, 768, 0), (BF16, 128, 4096, 0), (BF16, 1000, 352, 0), (BF16, 1024, 4096, 0), (BF16, 389, 1024, 0),
          (BF16, 3200, 512, 0), (BF16, 256, 2048, 0), (BF16, 128, 64, 0), (BF16, 160, 512, 0), (BF16, 128, 1056, 0),
          (W4C, 384, 1024, 64), (W4C, 130, 4096, 64), (W4C, 2048, 256, 64), (W4C, 64, 256, 64), (W4C, 40, 320, 64), (W4C, 96, 11008, 64),
          (W4C, 24, 8192, 64)] + sorted({(kind, N, K, group) for kind, N, K, group, _, _ in PINNED})
SWEEP_M = (9, 37, 128, 129, 200, 640, 1500, 2048)


def plan(lib, kind, M, N, K, group, epi, ldx=None, aligned=1, norm=0):
    out = (C.c_int64 * 12)(*([-7] * 12))
    rc = lib.parrot_gemm_plan(kind, M, N, K, group, epi, K if ldx is None else ldx, aligned, norm, out)
    return rc, dict(zip(FIELDS, out))


def sizing(lib, kind, M, N, K, group, epi):
    return lib.parrot_gemm_workspace_floats(M, N, K, 0 if kind == BF16 else group, epi)


@pytest.fixture(scope="module")
def header_plans(tmp_path_factory):
    """tools/gemm_plan_dump.cpp built from csrc/gemm_plan.h with a host C++ compiler alone: calls -> [(rc, route, tile, ksplit,
    norm_fused, the eight region numbers, total)].  The tile variant the launch code switches on is visible only here."""
    repo = Path(__file__).resolve().parents[1]
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler: csrc/gemm_plan.h must build without hipcc"
    exe = tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_dump"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", str(repo / "tools" / "gemm_plan_dump.cpp"), "-o", str(exe)], check=True)

    def run(calls):
        text = "".join(" ".join(map(str, c)) + "\n" for c in calls)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(calls)
        return [tuple(map(int, line.split())) for line in out]

    return run


def test_anchor_llama2_7b_qkv_at_128_rows(hip_lib, header_plans):
    """Derivable by hand: 128 rows x 12288 columns = 96 tiles of 128 x 128 on the LDS-DMA int4 kernel -> 512 / 96 = 5 splits, and
    5 x 128 x 12288 floats (31 MB) of partial results behind 128 x 32 activation sums."""
    rc, p = plan(hip_lib, W4, 128, 12288, 4096, 128, EPI_NONE)
    assert rc == OK and (p["route"], p["ksplit"]) == (G2_W4, 5)
    assert (p["xs_off"], p["xs_len"], p["part_off"], p["part_len"], p["part2_len"]) == (0, 128 * 32, 128 * 32, 5 * 128 * 12288, 0)
    assert p["total"] == 128 * 32 + 5 * 128 * 12288
    assert header_plans([(W4, 128, 12288, 4096, 128, EPI_NONE, 0)])[0][:4] == (OK, G2_W4, 128, 5)  # 128-wide tiles


@pytest.mark.parametrize("kind,N,K,group,epi,want", PINNED, ids=lambda v: None)
def test_route_tile_split_and_sizing_are_those_of_the_commit_before_the_plan(hip_lib, header_plans, kind, N, K, group, epi, want):
    got = header_plans([(kind, M, N, K, group, epi, 0) for M in PINNED_M])
    for M, (route, tile, ksplit, floats), h in zip(PINNED_M, want, got):
        assert h[:4] == (OK, route, tile, ksplit), (M, h)
        rc, p = plan(hip_lib, kind, M, N, K, group, epi)
        assert rc == OK and (p["route"], p["ksplit"]) == (route, ksplit), (M, p)
        assert tuple(p[f] for f in FIELDS) == (h[1],) + h[3:], (M, p, h)  # the library answers with the header's plan
        assert p["total"] <= sizing(hip_lib, kind, M, N, K, group, epi) <= floats, (M, p)  # the sizing may be tighter, never larger


def expected_fused(kind, K, group, norm):
    """Where the C entry point took the norm before the plan existed: gemm2_w4_takes (K % 64 == 0, whole K-steps per group, slabs on
    even slices - always so for these groups) and norm_xsum_takes."""
    return int(kind == W4 and norm in (1, 2) and group in (64, 128) and K % group == 0 and K <= 16384)


@pytest.mark.parametrize("kind,N,K,group", SHAPES)
def test_regions_are_disjoint_inside_the_total_and_hold_what_their_writers_write(hip_lib, header_plans, kind, N, K, group):
    ok_calls = []
    G = 0 if kind == BF16 else -(-K // (group if 0 < group <= K else K))  # quantisation groups per row
    seen = 0
    for M, epi, dldx, aligned, norm in itertools.product(SWEEP_M, (EPI_NONE, EPI_RESIDUAL, EPI_SWIGLU), (0, 8, 4), (1, 0), (0, 1, 2)):
        rc, p = plan(hip_lib, kind, M, N, K, group, epi, K + dldx, aligned, norm)
        if dldx == 4 or not aligned:  # the entry points refuse such rows (check_linear_args) and so does the plan
            assert rc == EINVAL and p["total"] == -7
            continue
        takes_g2 = K % 64 == 0 and (kind == BF16 or (group if 0 < group <= K else K) % 64 == 0)
        if K % 32 != 0 or (kind == W4C and not takes_g2):
            assert rc == EUNSUPPORTED
            continue
        assert rc == OK
        seen += 1
        want_route = {BF16: G2 if takes_g2 and epi != EPI_SWIGLU else GEN1, W4: G2_W4 if takes_g2 else GEN1, W4C: G2_W4C}[kind]
        assert p["route"] == want_route, (M, epi, p)
        assert 1 <= p["ksplit"] <= 8
        assert p["norm_fused"] == expected_fused(kind, K, group, norm), (M, epi, norm, p)
        spans = [(p[n + "_off"], p[n + "_len"]) for n in ("xn", "xs", "part", "part2")]
        assert all(off >= 0 and ln >= 0 and off + ln <= p["total"] for off, ln in spans), p
        live = sorted(s for s in spans if s[1] > 0)
        assert all(a[0] + a[1] <= b[0] for a, b in zip(live, live[1:])), p
        split = p["ksplit"] * M * N if p["ksplit"] > 1 else 0
        assert p["xn_len"] * 2 >= (M * K if p["norm_fused"] else 0)
        assert p["xs_len"] >= {G2_W4: -(-M // 128) * 128 * G, GEN1: M * G if kind == W4 else 0}.get(p["route"], 0)
        assert p["part_len"] >= split and p["part2_len"] >= (split if epi == EPI_SWIGLU else 0)
        assert p["total"] <= sizing(hip_lib, kind, M, N, K, group, epi), (M, epi, norm, p)
        ok_calls.append(((kind, M, N, K, group, epi, norm), p))
    assert seen or K % 32 != 0 or kind == W4C
    for (call, p), h in zip(ok_calls, header_plans([c for c, _ in ok_calls])):
        assert h[0] == OK and tuple(p[f] for f in FIELDS) == (h[1],) + h[3:], (call, p, h)
        M, tile = call[1], h[2]
        if p["route"] == GEN1:  # 128 x 128 tiles only from 512 of them on
            assert tile == (128 if -(-M // 128) * -(-N // 128) >= 512 else 64), (call, h)
        elif p["route"] == G2:  # 256 rows where they pad the prompt no further than 128-row tiles do
            assert tile == (256 if -(-M // 256) * 256 == -(-M // 128) * 128 else 128), (call, h)
        else:
            assert tile == 128, (call, h)


def test_the_plan_refuses_what_the_entry_points_refuse(hip_lib):
    for norm in (-1, 3):  # make_norm_args: kind must be 0, 1 or 2
        assert plan(hip_lib, W4, 128, 96, 512, 64, EPI_NONE, norm=norm)[0] == EINVAL
    assert plan(hip_lib, 3, 128, 96, 512, 64, EPI_NONE)[0] == EINVAL and plan(hip_lib, W4, 8, 96, 512, 64, EPI_NONE)[0] == EINVAL
    assert plan(hip_lib, W4, 128, 96, 512, 64, 4)[0] == EINVAL and plan(hip_lib, W4, 128, 96, 512, 64, EPI_NONE, ldx=504)[0] == EINVAL
    # a known norm that is not fused is an answer, not an error: bf16 and codebook calls never fuse it
    for kind, group in ((BF16, 0), (W4C, 64), (W4, 32)):
        rc, p = plan(hip_lib, kind, 128, 96, 512, group, EPI_NONE, norm=1)
        assert rc == OK and p["norm_fused"] == 0 and p["xn_len"] == 0
    # sizing builds only plans that exist: a successful call leaves no error behind
    hip_lib.parrot_w4_packed_bytes(8, 100, 32)  # (fails: K % 32) sets the last error
    before = hip_lib.parrot_last_error()
    assert b"multiple of 32" in before
    assert sizing(hip_lib, W4, 37, 64, 256, 32, EPI_NONE) > 0 and sizing(hip_lib, W4, 128, 96, 512, 64, EPI_SWIGLU) > 0
    assert sizing(hip_lib, BF16, 40, 128, 1056, 0, EPI_SWIGLU) > 0
    assert hip_lib.parrot_last_error() == before


def test_nothing_overflows_32_bits_at_the_largest_call(hip_lib):
    M, N, K = 65535 * 64, 50688, 4096
    for kind, group, epi in ((BF16, 0, EPI_NONE), (BF16, 0, EPI_SWIGLU), (W4, 128, EPI_SWIGLU), (W4, 32, EPI_NONE), (W4C, 64, EPI_NONE)):
        rc, p = plan(hip_lib, kind, M, N, K, group, epi, norm=1 if kind == W4 else 0)
        assert rc == OK and p["ksplit"] == 1 and p["part_len"] == 0  # 32768 row tiles: nothing to split
        G = K // group if group else 0
        want_xs = {GEN1: M * G if kind == W4 else 0, G2_W4: -(-M // 128) * 128 * G}.get(p["route"], 0)
        want_xn = (M * K + 1) // 2 if p["norm_fused"] else 0  # 8.6e9 floats
        assert (p["xn_len"], p["xs_len"], p["total"]) == (want_xn, want_xs, want_xn + want_xs)
        assert sizing(hip_lib, kind, M, N, K, group, epi) >= p["total"]
    # a wide call (520 x 2^20 outputs, 5.5e8 floats each way): K is split only below ~256 tiles, so its 40960 tiles run in one pass and
    # the partial results of a split call stay far below 2^31 floats; whichever way, the region is exactly ksplit x M x N
    rc, p = plan(hip_lib, BF16, 520, 1 << 20, 4096, 0, EPI_NONE)
    assert rc == OK and p["part_len"] == p["total"] == (p["ksplit"] * 520 * (1 << 20) if p["ksplit"] > 1 else 0)
    assert p["ksplit"] == 1


def test_w8_workspace_is_never_more_than_the_closed_formula_it_replaces(hip_lib):
    for M, N, K, epi in itertools.product((9, 40, 130, 300, 1100, 2048), (128, 300, 520, 3000, 11008), (128, 256, 512, 11008 // 128 * 128), (EPI_NONE, EPI_SWIGLU)):
        nw = 2 if epi == EPI_SWIGLU else 1
        got = hip_lib.parrot_w8_gemm_workspace_bytes(M, N, K, epi)
        # 1 <= ksplit <= 8: int32 sums per split and weight, one fp32 outlier part per weight, the fp16 outlier operands
        assert (1 + 1) * M * N * 4 * nw + (M + nw * N) * K * 2 <= got <= (8 + 1) * M * N * 4 * nw + (M + nw * N) * K * 2 + 64
    assert hip_lib.parrot_w8_gemm_workspace_bytes(8, 128, 512, 0) == 0 and hip_lib.parrot_w8_gemm_workspace_bytes(40, 128, 320, 0) == 0


class _FakeLib:
    """parrot_gemm_plan of the real library (host arithmetic), or a forced answer; the launches only record their arguments."""

    def __init__(self, real, force=None):
        self.real, self.force, self.plan_calls, self.gemm_calls = real, force, [], []

    def parrot_gemm_plan(self, *a):
        self.plan_calls.append(a[:9])
        rc = self.real.parrot_gemm_plan(*a)
        if self.force is not None:
            a[9][2] = self.force
        return rc

    def parrot_gemm_workspace_floats(self, *a):
        return self.real.parrot_gemm_workspace_floats(*a)

    def parrot_w4_gemm(self, *a):
        self.gemm_calls.append(a)
        return 0


@pytest.mark.parametrize("group,force,want_fused", [(64, None, True), (128, None, True), (32, None, False), (64, 0, False), (32, 1, True)])
def test_w4_linear_asks_the_plan_whether_the_norm_is_fused(hip_lib, monkeypatch, group, force, want_fused):
    """ops.w4_linear mirrored the C predicate by hand; where the two disagreed the call ended in PARROT_EUNSUPPORTED.  Now the
    answer of parrot_gemm_plan (out[2]) decides: fused -> the norm goes to parrot_w4_gemm with the caller's rows; not fused ->
    the rows go through _prenorm and the GEMM gets no norm.  Runs on CPU tensors with the launches stubbed."""
    from lit_parrot_amd import ops

    M, N, K = 40, 96, 512
    fake = _FakeLib(hip_lib, force)
    prenormed = []
    xn = torch.zeros((M, K), dtype=torch.bfloat16)

    def prenorm(x, norm):
        prenormed.append((x, norm))
        return xn, None

    monkeypatch.setattr(ops._hip, "load", lambda: fake)
    monkeypatch.setattr(ops, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "stream", lambda: 0)
    monkeypatch.setattr(ops, "_prenorm", prenorm)
    x, out = torch.zeros((M, K), dtype=torch.bfloat16), torch.zeros((M, N), dtype=torch.bfloat16)
    packed = torch.zeros((64,), dtype=torch.uint8)
    norm = ops.Norm(2, torch.ones(K, dtype=torch.bfloat16), torch.zeros(K, dtype=torch.bfloat16), 1e-5)
    ops.w4_linear(packed, N, K, group, x, out, epilogue=EPI_RESIDUAL, residual=out, norm=norm)
    assert fake.plan_calls == [(W4, M, N, K, group, EPI_RESIDUAL, K, 1, 2)]
    (call,) = fake.gemm_calls
    if want_fused:
        assert not prenormed and call[2] == x.data_ptr() and call[14] is not None
    else:
        assert len(prenormed) == 1 and prenormed[0][0] is x and prenormed[0][1] is norm
        assert call[2] == xn.data_ptr() and call[14] is None
    # no norm, or a decode call: the plan is not asked
    fake.plan_calls.clear()
    ops.w4_linear(packed, N, K, group, x, out)
    assert fake.plan_calls == []
