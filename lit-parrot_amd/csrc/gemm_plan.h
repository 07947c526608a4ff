// How one prompt GEMM call (M > 8 rows) runs: which kernel, which tile, how K is split and where everything lives in the
// caller's workspace.  Host arithmetic only - no HIP type, compiles with a plain C++ compiler - so that the sizing
// (parrot_gemm_workspace_floats), the entry points (gemm.hip), the launch code (gemm.hip, gemm2.hip) and parrot_gemm_plan all read
// the SAME numbers: a kernel writes where the plan says, and the caller allocated what the plan's total says.
//
// Workspace of parrot_bf16_gemm / parrot_w4_gemm / parrot_w4c_gemm, in floats, regions in this order (absent ones have length 0):
//   xn     ceil(M K / 2)         the normalised rows (bf16, leading dimension K) when parrot_w4_gemm fuses the norm
//   xs     Mpad x ngroups        int4 on the LDS-DMA kernel: per-group activation sums, [group][row], Mpad = M rounded up to 128
//          M x ngroups           int4 on the first-generation kernel: the same sums as [row][group]
//   part   ksplit x M x N        fp32 partial results when K is split
//   part2  ksplit x M x N        the same for the second weight of a split SWIGLU call
#pragma once
#include "w4_plan.h"

namespace parrot {

constexpr int GBK = 32;                          // K-tile of the first-generation kernel (gemm.hip)
constexpr int G2M = 128, G2N = 128, G2K = 64;    // tile of the LDS-DMA kernels (gemm2.hip)
constexpr int kNormXsumMaxD = 16384;             // widest row the norm kernel takes (norm.hip: kNormThreads * 8 * kNormV)

enum GemmKind : int { GEMM_BF16 = 0, GEMM_W4 = 1, GEMM_W4C = 2 };
enum GemmRoute : int {
    GEMM_ROUTE_GEN1 = 0,    // gemm_kernel (gemm.hip): bf16 SWIGLU, K % 64 != 0, int4 groups that are not multiples of 64
    GEMM_ROUTE_G2 = 1,      // gemm2_kernel (bf16, LDS-DMA)
    GEMM_ROUTE_G2_W4 = 2,   // gemm2_w4_kernel (int4, LDS-DMA)
    GEMM_ROUTE_G2_W4C = 3,  // gemm2_w4_kernel with a codebook (NF4 / FP4)
};

struct GemmSpan {
    int64_t off, len;  // floats from the start of the workspace
};

struct GemmPlan {
    int route;       // GemmRoute
    int tile;        // GEN1: 128 | 64 (square tiles); G2: tile rows 128 | 256; G2_W4(C): tile columns 128 | 256
    int ksplit;      // 1 = one pass; > 1: partial results + launch_splitk_epilogue
    int norm_fused;  // parrot_w4_gemm applies the norm itself (one launch writes xn and xs)
    GemmSpan xn, xs, part, part2;
    int64_t total;   // floats
};

// ---------------------------------------------------------------- first-generation kernel (gemm.hip)
// 128 x 128 tiles only when they alone give the chip >= 2 workgroups per CU; otherwise 64 x 64 (4x the workgroups)
inline bool gemm_big_tiles(int M, int N) {
    const int env = tune_env("PARROT_GEMM_BIG_MIN", 512);  // PARROT_GEMM_BIG_MIN: minimum number of 128 x 128 tiles for the big-tile kernel (experiment hook)
    return (int64_t)((M + 127) / 128) * ((N + 127) / 128) >= env;
}

// K splits for launches with too few tiles to fill the chip (short prompts): equal ranges of whole quantisation groups,
// at least 8 K-tiles each, at most 8 splits, aiming at >= ~1536 workgroups
inline int gemm_ksplit(int M, int N, int K, int gs_tiles) {
    const int env = tune_env("PARROT_GEMM_KSPLIT", -2);  // PARROT_GEMM_KSPLIT: 0 = never split (A/B), n = force
    if (env == 0) return 1;
    const int64_t tiles = gemm_big_tiles(M, N) ? (int64_t)((M + 127) / 128) * ((N + 127) / 128) : (int64_t)((M + 63) / 64) * ((N + 63) / 64);
    const int ktiles = K / GBK;
    int ks = env > 0 ? env : (int)(1536 / (tiles > 0 ? tiles : 1));
    if (ks > 8) ks = 8;
    while (ks > 1 && (ktiles % (ks * gs_tiles) != 0 || ktiles / ks < 8)) --ks;
    return ks < 1 ? 1 : ks;
}

// ---------------------------------------------------------------- LDS-DMA bf16 kernel (gemm2.hip)
inline bool gemm2_enabled() {
    const int env = tune_env("PARROT_GEMM2", 1);  // PARROT_GEMM2=0: A/B against the first-generation kernel
    return env != 0;
}

// (the 16-byte rows its LDS-DMA needs - ldx % 8 == 0, x and W 16-byte aligned - are what check_linear_args demands of every Linear call)
inline bool gemm2_takes(int K, int epilogue) { return gemm2_enabled() && epilogue != PARROT_EPI_SWIGLU && K % G2K == 0; }

// tile rows: 256 (8 waves, one workgroup per CU) for prompts that fill whole 256-row tiles as well as 128-row ones
inline int gemm2_wm(int M) {
    const int env = tune_env("PARROT_GEMM2_WM", 0);  // PARROT_GEMM2_WM = 2 | 4 (A/B)
    if (env == 2 || env == 4) return env;
    return (M + 255) / 256 * 256 == (M + 127) / 128 * 128 ? 4 : 2;
}

// K splits when the tiles alone leave most of the chip idle: aim at ~512 workgroups of 128 x 128 (two fit a CU) or 256 of
// 256 x 128 (one per CU), whole 64-deep steps, at least 8 per split
inline int gemm2_ksplit(int M, int N, int K) {
    const int wm = gemm2_wm(M), tm = wm * 64;
    const int64_t tiles = (int64_t)((M + tm - 1) / tm) * ((N + G2N - 1) / G2N);
    const int ktiles = K / G2K;
    const int target = tune_env("PARROT_GEMM2_SPLIT_TARGET", wm == 4 ? 256 : 512);  // PARROT_GEMM2_SPLIT_TARGET: workgroups to aim at when splitting
    const int full = wm == 4 ? 128 : 256;  // more tiles than this: no split
    int ks = tiles > full ? 1 : (int)(target / (tiles > 0 ? tiles : 1));
    if (ks > 8) ks = 8;
    while (ks > 1 && ktiles / ks < 8) --ks;  // (uneven ranges are fine: split z owns steps [z kt / ks, (z + 1) kt / ks))
    return ks < 1 ? 1 : ks;
}

// ---------------------------------------------------------------- LDS-DMA int4 kernel (gemm2.hip)
// the int4 kernel takes whole K-steps per group and slab boundaries on K-step boundaries
inline bool gemm2_w4_takes(const W4Plan& plan, int K) {
    if (!gemm2_enabled() || K % G2K != 0 || plan.Gs % 2 != 0) return false;
    for (int c = 0; c < plan.nslabs; ++c)
        if (plan.slab[c].slice0 % 2 != 0) return false;
    return true;
}

// tile shape of the int4 kernel (wave columns)
inline int gemm2_w4_wn(int M) {
    const int env = tune_env("PARROT_GEMM2_W4_WN", 0);  // PARROT_GEMM2_W4_WN = 2 | 4 (A/B)
    (void)M;
    // measured (Llama-2-7B int4, 128- and 32-token prompts, uneven split-K): WN = 2 3.97 / 3.80 ms, WN = 4 4.77 / 4.33 ms - the wide
    // shape does not pay; it stays selectable for A/B
    return env == 4 ? 4 : 2;
}

inline int gemm2_w4_ksplit(int M, int N, int K, const W4Plan& plan) {
    const int wn = gemm2_w4_wn(M);
    const int tn = wn * 64;
    const int64_t tiles = (int64_t)((M + G2M - 1) / G2M) * ((N + tn - 1) / tn);
    const int ktiles = K / G2K, Gt = plan.Gs / 2;
    const int env_target = tune_env("PARROT_GEMM2_W4_SPLIT_TARGET", 0), env_max = tune_env("PARROT_GEMM2_W4_KSMAX", 8);  // (A/B)
    const int target = env_target > 0 ? env_target : (wn == 4 ? 256 : 512);  // workgroups that fill the chip
    // launches with fewer tiles than this split K; 256 tiles still split two ways: two workgroups fit a CU (Falcon-40B 128-token prefill 25.8 -> 23.2 ms)
    const int thr = tune_env("PARROT_GEMM2_W4_SPLIT_BELOW", 257);
    int ks = tiles >= (wn == 4 ? 128 : thr) ? 1 : (int)(target / (tiles > 0 ? tiles : 1));
    if (ks > env_max) ks = env_max;
    const int G_all = (ktiles + Gt - 1) / Gt;
    while (ks > 1 && (G_all / ks < 1 || ktiles / ks < 4)) --ks;  // whole groups per split, ranges need not be equal
    return ks < 1 ? 1 : ks;
}

// norm + per-group sums of a prompt's rows in one launch (norm.hip): groups of G = 64 / 128 over rows of d elements
inline bool norm_xsum_takes(int norm_kind, int d, int G) { return (norm_kind == 1 || norm_kind == 2) && (G == 64 || G == 128) && d % G == 0 && d <= kNormXsumMaxD; }

// ---------------------------------------------------------------- the plan
// w4: the weight layout of an int4 / codebook call (w4_make_plan), unused for bf16.  norm_kind != 0 asks for a norm in front: the
// plan fuses it where parrot_w4_gemm can (norm_fused) and is otherwise that of the same call on rows normalised beforehand.
// The entry points have checked their arguments (check_linear_args: 16-byte rows) before they come here.
// Returns what the entry point returns for a shape it does not take.
inline int gemm_make_plan(int kind, int M, int N, int K, const W4Plan* w4, int epilogue, int norm_kind, GemmPlan* p) {
    const bool swi = epilogue == PARROT_EPI_SWIGLU;
    *p = GemmPlan{};
    int64_t xs_len = 0;
    if (kind == GEMM_BF16) {
        PARROT_UNSUPPORTED(K % GBK == 0, "bf16_gemm: K=%d must be a multiple of %d", K, GBK);
        if (gemm2_takes(K, epilogue)) {
            p->route = GEMM_ROUTE_G2, p->tile = gemm2_wm(M) * 64, p->ksplit = gemm2_ksplit(M, N, K);
        } else {
            p->route = GEMM_ROUTE_GEN1, p->tile = gemm_big_tiles(M, N) ? 128 : 64, p->ksplit = gemm_ksplit(M, N, K, 1);
        }
    } else {
        const bool g2 = gemm2_w4_takes(*w4, K);
        if (kind == GEMM_W4C)
            PARROT_UNSUPPORTED(g2, "w4c_gemm: needs K %% 64 == 0 and blocks that are multiples of 64 (K=%d block=%d)", K, w4->Gs * 32);
        if (g2) {
            p->route = kind == GEMM_W4C ? GEMM_ROUTE_G2_W4C : GEMM_ROUTE_G2_W4, p->tile = gemm2_w4_wn(M) * 64, p->ksplit = gemm2_w4_ksplit(M, N, K, *w4);
            p->norm_fused = kind == GEMM_W4 && norm_xsum_takes(norm_kind, K, w4->Gs * 32);
            xs_len = kind == GEMM_W4C ? 0 : (int64_t)((M + G2M - 1) / G2M) * G2M * w4->ngroups;  // codebook weights need no activation sums
        } else {
            p->route = GEMM_ROUTE_GEN1, p->tile = gemm_big_tiles(M, N) ? 128 : 64, p->ksplit = gemm_ksplit(M, N, K, w4->Gs);
            xs_len = (int64_t)M * w4->ngroups;
        }
    }
    const int64_t part_len = p->ksplit > 1 ? (int64_t)p->ksplit * M * N : 0;
    int64_t off = 0;
    auto take = [&off](int64_t len) {
        const GemmSpan s = {off, len};
        off += len;
        return s;
    };
    p->xn = take(p->norm_fused ? ((int64_t)M * K + 1) / 2 : 0);
    p->xs = take(xs_len);
    p->part = take(part_len);
    p->part2 = take(swi ? part_len : 0);
    p->total = off;
    return PARROT_OK;
}

// ---------------------------------------------------------------- LLM.int8 prompt GEMM (w8.hip)
inline int w8_gemm2_ksplit(int M, int N, int K) {
    const int64_t tiles = (int64_t)((M + 127) / 128) * ((N + 127) / 128);
    const int ktiles = K / 128;
    const int target = tune_env("PARROT_W8_SPLIT_TARGET", 512);  // PARROT_W8_SPLIT_TARGET: workgroups to aim at when splitting K
    int ks = tiles > 256 ? 1 : (int)(target / (tiles > 0 ? tiles : 1));  // up to 256 tiles: split, two workgroups fit a CU
    if (ks > 8) ks = 8;
    while (ks > 1 && ktiles / ks < 4) --ks;
    return ks < 1 ? 1 : ks;
}

// Workspace of parrot_w8_gemm: byte offsets from the workspace pointer rounded up to 16 bytes, so that every region keeps its alignment
// under any caller's pointer (`total` has room for that rounding).
//   part, part2   ks x M x N int32 sums per K range (part2: the second weight of SWIGLU)
//   O1, O2        M x N fp32 outlier part per weight
//   subA, subB    fp16 operands of the outlier GEMM: A[:, idx] (M x K at worst) and dequant(CB[:, idx]) (N x K per weight), 16-byte aligned
struct W8GemmPlan {
    int ks;
    int64_t part, part2, O1, O2, subA, subB, total;
};

inline W8GemmPlan w8_gemm_make_plan(int M, int N, int K, int epilogue) {
    const int64_t nw = epilogue == PARROT_EPI_SWIGLU ? 2 : 1, mn4 = (int64_t)M * N * 4;
    W8GemmPlan p;
    p.ks = w8_gemm2_ksplit(M, N, K);
    p.part = 0;
    p.part2 = p.part + (nw - 1) * p.ks * mn4;
    p.O1 = p.part + nw * p.ks * mn4;
    p.O2 = p.O1 + (nw - 1) * mn4;
    p.subA = (p.O1 + nw * mn4 + 15) & ~(int64_t)15;
    p.subB = p.subA + (int64_t)M * K * 2;
    p.total = p.subB + nw * N * K * 2 + 16;
    return p;
}

}  // namespace parrot
