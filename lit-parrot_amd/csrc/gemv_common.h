// The format-independent parts of the decode GEMVs: w4_gemv_kernel (w4.hip), bf16_gemv_kernel (dense.hip) and
// w8_fused_kernel (w8.hip).  DESIGN.md §4 "What the GEMV structure is built around" gives the measurements.
// Workgroup = nslabs x wps waves; wave (slab c, j) streams slab c of K for the RU consecutive rows of row group j.
// Per format, in the kernels: the weight requests (*_ISSUE_ROW), PRIME and the dot loop - where the compiler's vmcnt
// bookkeeping lives - and the int8 quantiser and epilogue.
// The fused-norm prologue (request of the input rows and norm parameters, statistics, apply) is the same text in the three
// kernels too, but stays written out in each: as a __forceinline__ function - every signature tried - it changes the
// register counts (bf16: 58 of 64 variants, typically +4 VGPRs, some a wave of occupancy less), because a callee is
// optimised on its own before it is inlined.  Until that is solved, a change to one copy goes into all three.
#pragma once
#include <type_traits>

#include "parrot_common.h"

namespace parrot {

// rounds of the cooperative request: thread t owns the 16-byte chunks t, t + nthreads, ... of a row of x, so the fused
// norm covers K <= kMaxChunkIt * 8 * nthreads (checked on the host: gemv_fused_norm_lds)
constexpr int kMaxChunkIt = 4;

// ---------------------------------------------------------------- wave priorities
// The SIMDs arbitrate oldest-first.  The prologue runs at s_setprio 3 (kernel entry; 0 before the dot loop): without it the
// 3rd / 4th workgroup of a CU gets its norm instructions in only when the older workgroups' dot loops stall (measured: norm
// ready at +3.4 us in the first workgroup of a CU, +7.5 .. +10 us in the last), and the launch ends with the slowest.
// In the dot loop (call before row u is consumed) the priority falls TOP -> 0 over the batch, so that waves that are behind
// overtake waves that are ahead: oldest-first lets the first workgroup of a CU finish early and leaves its share of the
// memory queue idle.  TOP is 3 for int4 and int8 and 2 for bf16; bf16's 2 has NOT been measured against 3.
template <int RU, int TOP>
__device__ __forceinline__ void gemv_prio_ladder(int u) {
    static_assert(TOP == 2 || TOP == 3, "s_setprio takes an immediate: the steps are written out");
    if (RU >= 4) {
        if (u == 0) __builtin_amdgcn_s_setprio(TOP);
        if (u == RU / 4) __builtin_amdgcn_s_setprio(TOP - 1);
        if (u == RU / 2) __builtin_amdgcn_s_setprio(TOP - 2);
        if (TOP == 3 && u == (3 * RU) / 4) __builtin_amdgcn_s_setprio(0);
    }
}

// ---------------------------------------------------------------- epilogue
// One thread per (row of the batch, m): threadIdx.x = row * M + m.  Set up before the batch loop; then per batch t
//   request()    at the START of the batch: the thread's bias / residual elements and, with AD, the four adapter-v2 values.
//                Every thread, clamped, always (a load behind a condition costs the compiler its static vmcnt bookkeeping),
//                so that the kernel's tail does not end with "load residual -> wait a full memory latency -> add -> store";
//   sum_store()  after the batch's barrier, threads < R * M (the guard stays in the kernel: inside, it costs an s_xor):
//                sums the slabs' partials rd[wave][(u * M + m) * NW + q] in ascending slab order (fixed: the result does
//                not depend on the launch), applies the epilogue, stores.
// `any`: a readable address for the operands the call does not have (the weights).
struct GemvEpiOperands {
    bf16_t res, bias;
    float as, ab, as2, ab2;  // adapter-v2 scale / bias, and the SwiGLU partner's
};
template <int M, bool DUAL, bool AD>
struct GemvEpilogue {
    const bf16_t* res_p;
    const bf16_t* bias_p;
    bool has_res, has_bias;
    int ldr, e_m, e_ur;
    __device__ __forceinline__ GemvEpilogue(const void* any, const bf16_t* bias, const bf16_t* residual, int ldr_)
        : res_p(residual != nullptr ? residual : reinterpret_cast<const bf16_t*>(any)),
          bias_p(bias != nullptr ? bias : reinterpret_cast<const bf16_t*>(any)),
          has_res(residual != nullptr), has_bias(bias != nullptr), ldr(ldr_), e_m(threadIdx.x % M), e_ur(threadIdx.x / M) {}
    __device__ __forceinline__ GemvEpiOperands request(int N, int R, int t, AdapterArgs ad = AdapterArgs{}) const {
        const int e_col = min(((int)blockIdx.x + t * (int)gridDim.x) * R + e_ur, N - 1);
        GemvEpiOperands e;
        e.res = res_p[has_res ? (int64_t)e_m * ldr + e_col : 0];
        e.bias = bias_p[has_bias ? e_col : 0];
        e.as = 1.f, e.ab = 0.f, e.as2 = 1.f, e.ab2 = 0.f;
        if constexpr (AD) {
            if (ad.scale != nullptr) e.as = bf2f(ad.scale[e_col]);
            if (ad.bias != nullptr) e.ab = bf2f(ad.bias[e_col]);
            if (DUAL && ad.scale2 != nullptr) e.as2 = bf2f(ad.scale2[e_col]);
            if (DUAL && ad.bias2 != nullptr) e.ab2 = bf2f(ad.bias2[e_col]);
        }
        return e;
    }
    template <int RU>
    __device__ __forceinline__ void sum_store(float (*rd)[RU * M * (DUAL ? 2 : 1)], int nslabs, int wps, int N, int R, int t, int epi,
                                              GemvEpiOperands e, bf16_t* out, int ldo) const {
        constexpr int NW = DUAL ? 2 : 1;
        const int m = threadIdx.x % M, ur = threadIdx.x / M;
        const int jj = ur / RU, u = ur % RU;
        const int col = ((int)blockIdx.x + t * (int)gridDim.x) * R + ur;
        if (col < N) {
            float a0 = 0.f, a1 = 0.f;
            for (int c = 0; c < nslabs; ++c) {
                a0 += rd[c * wps + jj][(u * M + m) * NW];
                if (DUAL) a1 += rd[c * wps + jj][(u * M + m) * NW + 1];
            }
            if constexpr (AD)
                out[(int64_t)m * ldo + col] =
                    apply_epilogue_adapter_vals(epi, a0, a1, has_bias, bf2f(e.bias), bf2f(e.res), e.as, e.ab, e.as2, e.ab2);
            else
                out[(int64_t)m * ldo + col] = apply_epilogue_vals(epi, a0, a1, has_bias, bf2f(e.bias), bf2f(e.res));
        }
    }
};

// ---------------------------------------------------------------- host
// fused norm with `nthreads` threads: kMaxChunkIt request rounds cover K, the normalised rows [M][K] bf16 fit LDS (*lds)
inline int gemv_fused_norm_lds(const char* who, const NormArgs& na, int M, int K, int nthreads, size_t* lds) {
    *lds = 0;
    if (na.kind == 0) return PARROT_OK;
    PARROT_UNSUPPORTED((K >> 3) <= kMaxChunkIt * nthreads, "%s: fused norm needs K <= %d with this workgroup shape", who,
                       8 * kMaxChunkIt * nthreads);
    *lds = (size_t)M * K * 2;
    PARROT_UNSUPPORTED(*lds <= 64 * 1024, "%s: fused norm needs %zu B of LDS", who, *lds);
    return PARROT_OK;
}

// workgroups resident at once: 256 CUs x the workgroups of `nwaves` that fit the `cu_waves` wave slots the VGPRs leave
inline int gemv_resident(int cu_waves, int nwaves) { return 256 * (cu_waves / nwaves > 0 ? cu_waves / nwaves : 1); }

// Grid = what is resident at once; every workgroup walks `iters` batches of R rows (batch t of workgroup b = rows of block
// b + t * grid), so that no workgroup starts late and pays the activation / norm chain behind everybody else's weight
// stream (measured on lm_head: a 4th-round workgroup entered at +11 us and had its norm ready 6.5 us later).
struct GemvGrid {
    int iters;
    unsigned grid;
};
inline GemvGrid gemv_grid(int N, int R, int resident) {
    const int batches = (N + R - 1) / R;
    const int iters = (batches + resident - 1) / resident;
    return GemvGrid{iters, (unsigned)((batches + iters - 1) / iters)};
}

// Row-chunk loop of an entry point: CAP input rows per launch; go(std::integral_constant<int, rows>, x, residual, out)
// launches the kernel instantiated for `rows` (1 .. CAP) on the chunk's pointers.
template <int MM, typename F>
inline int gemv_launch_rows(int rows, F& go, const void* x, const void* residual, void* out) {
    if constexpr (MM > 1) {
        if (rows < MM) return gemv_launch_rows<MM - 1>(rows, go, x, residual, out);
    }
    return go(std::integral_constant<int, MM>{}, x, residual, out);
}
template <int CAP, typename F>
inline int gemv_for_row_chunks(const void* x, int ldx, int M, const void* residual, int ldr, void* out, int ldo, F go) {
    const bf16_t* xb = (const bf16_t*)x;
    const bf16_t* rb = (const bf16_t*)residual;
    bf16_t* ob = (bf16_t*)out;
    for (int m0 = 0; m0 < M; m0 += CAP) {
        const int rc = gemv_launch_rows<CAP>(M - m0 < CAP ? M - m0 : CAP, go, xb + (int64_t)m0 * ldx,
                                             rb ? rb + (int64_t)m0 * ldr : nullptr, ob + (int64_t)m0 * ldo);
        if (rc != PARROT_OK) return rc;
    }
    return PARROT_OK;
}

}  // namespace parrot
