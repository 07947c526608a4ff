// Dense bf16 Linear for the decode step: y = epilogue(x @ W^T + b), W (N, K) row-major bf16.
// Reference: torch.nn.Linear on the bf16-true path (lit_gpt/model.py:29,188,190,281-282,293-295).
//
// Memory-bound GEMV on the skeleton shared with the int4 kernel (gemv_common.h), which is where it was measured:
//   * workgroup = nslabs x wps waves; wave (slab c, j) owns the chunks of slab c of K (16 B = 8 bf16 per lane and load,
//     J loads per row, 64 lanes = 1 KiB contiguous each) of RU consecutive rows of row group j;
//   * the activations - and the optional RMSNorm / LayerNorm of them - are prepared ONCE per workgroup through LDS
//     (the first version normalised all of K in every 4-row wave: more VALU work than the dot products);
//   * weight rows go through a rolling window (PRIME rows requested ahead) so that a wave never sits in the issue of
//     loads the CU cannot accept yet; every load is unconditional (clamped), or the compiler loses its vmcnt bookkeeping;
//   * the grid is what is resident at once and every workgroup walks `iters` batches of rows;
//   * fp32 accumulation through v_dot2c_f32_bf16, wave reduction (DPP), cross-slab reduction in LDS, fused epilogue
//     whose bias / residual elements are requested at batch start.
#include "gemv_common.h"

namespace parrot {

constexpr int kDenseJ = 4;         // 16-B loads per lane per row (max)
constexpr int kDenseMaxSlabs = 16;  // K <= 32768

// AD: the adapter-v2 affine in the epilogue (its four elements requested at batch start like the bias); AD = false is the plain kernel
template <int M, bool DUAL, int J, int RU, int MAXW, bool AD = false>
__global__ void __launch_bounds__(MAXW * 64)
bf16_gemv_kernel(const uint4* __restrict__ W, const uint4* __restrict__ W2, const bf16_t* __restrict__ x, int ldx,
                 const bf16_t* __restrict__ bias, const bf16_t* residual, int ldr, bf16_t* out, int ldo, int N, int K,
                 int wps, int nslabs, int epi, int iters, NormArgs na, AdapterArgs ad) {
    constexpr int NW = DUAL ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char dense_smem[];  // normalised activations [M][K] bf16 (norm only)
    __shared__ float red[2][MAXW][RU * M * NW];
    __shared__ float stat[16];
    __builtin_amdgcn_s_setprio(3);  // prologue at raised wave priority (gemv_common.h)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = nslabs * wps;
    const int slab = wave / wps, j = wave % wps;
    const int chunks = K >> 3;  // 16-B units per row
    const int c0 = (int)((int64_t)slab * chunks / nslabs), c1 = (int)((int64_t)(slab + 1) * chunks / nslabs);
    const int R = wps * RU;
    const int nthreads = nwaves * 64;

    int cidx[J];
    bool cok[J];
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
        const int c = c0 + jj * 64 + lane;
        cok[jj] = c < c1;
        cidx[jj] = cok[jj] ? c : c1 - 1;
    }
    uint32_t xr[M][J][4];
    uint4 cx[M][kMaxChunkIt], cw[kMaxChunkIt], cb[kMaxChunkIt];
    if (na.kind == 0) {
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int jj = 0; jj < J; ++jj) {
                uint4 v = reinterpret_cast<const uint4*>(x + (int64_t)m * ldx)[cidx[jj]];
                if (!cok[jj]) v = make_uint4(0, 0, 0, 0);
                xr[m][jj][0] = v.x;
                xr[m][jj][1] = v.y;
                xr[m][jj][2] = v.z;
                xr[m][jj][3] = v.w;
            }
    } else {
#pragma unroll
        for (int it = 0; it < kMaxChunkIt; ++it) {
            cw[it] = cb[it] = make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int m = 0; m < M; ++m) cx[m][it] = make_uint4(0, 0, 0, 0);
            if (it * nthreads < chunks) {  // workgroup-uniform: rounds past the row are skipped, not computed on zeros
                const int c = threadIdx.x + it * nthreads;
                const int cc = c < chunks ? c : chunks - 1;
                cw[it] = reinterpret_cast<const uint4*>(na.weight)[cc];
                if (na.kind == 2 && na.bias != nullptr) cb[it] = reinterpret_cast<const uint4*>(na.bias)[cc];
#pragma unroll
                for (int m = 0; m < M; ++m) cx[m][it] = reinterpret_cast<const uint4*>(x + (int64_t)m * ldx)[cc];
            }
        }
    }

    uint4 w[NW][RU][J];
    constexpr int PRIME = RU >= 4 ? 2 : 1;  // rows requested ahead (J x 1 KiB per wave each)
#define DENSE_ROW0(T) (((int)blockIdx.x + (T) * (int)gridDim.x) * R + j * RU)
#define DENSE_ISSUE_ROW(T, U)                                                       \
    {                                                                               \
        const int64_t row_ = min(DENSE_ROW0(T) + (U), N - 1);                       \
        _Pragma("unroll") for (int jj = 0; jj < J; ++jj) {                          \
            w[0][U][jj] = load_nt16(W + row_ * chunks + cidx[jj]);                  \
            if (DUAL) w[1][U][jj] = load_nt16(W2 + row_ * chunks + cidx[jj]);       \
        }                                                                           \
    }
#pragma unroll
    for (int u = 0; u < PRIME; ++u) DENSE_ISSUE_ROW(0, u)
    asm volatile("" ::: "memory");  // keep the remaining requests below the prologue

    if (na.kind != 0) {  // fused RMSNorm / LayerNorm of the input rows, once per workgroup, through LDS
        uint4* xn = reinterpret_cast<uint4*>(dense_smem);
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float s1 = 0.f;
#pragma unroll
            for (int it = 0; it < kMaxChunkIt; ++it) {
                if (it * nthreads < chunks) {
                    const uint32_t dw[4] = {cx[m][it].x, cx[m][it].y, cx[m][it].z, cx[m][it].w};
                    float t = 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) t += norm_stat1(dw[i], na.kind);
                    s1 += (threadIdx.x + it * nthreads < chunks) ? t : 0.f;
                }
            }
            s1 = block_sum_waves(s1, stat, nwaves);
            float mean = 0.f, r;
            if (na.kind == 2) {
                mean = s1 / (float)na.d;
                float s2 = 0.f;
#pragma unroll
                for (int it = 0; it < kMaxChunkIt; ++it) {
                    if (threadIdx.x + it * nthreads < chunks) {
                        const uint32_t dw[4] = {cx[m][it].x, cx[m][it].y, cx[m][it].z, cx[m][it].w};
#pragma unroll
                        for (int i = 0; i < 4; ++i) s2 += norm_stat2(dw[i], mean);
                    }
                }
                r = norm_scale(na, block_sum_waves(s2, stat, nwaves));
            } else {
                r = norm_scale(na, s1);
            }
#pragma unroll
            for (int it = 0; it < kMaxChunkIt; ++it) {
                const int c = threadIdx.x + it * nthreads;
                if (c < chunks) {
                    const uint32_t dx[4] = {cx[m][it].x, cx[m][it].y, cx[m][it].z, cx[m][it].w};
                    const uint32_t dwt[4] = {cw[it].x, cw[it].y, cw[it].z, cw[it].w};
                    const uint32_t dbs[4] = {cb[it].x, cb[it].y, cb[it].z, cb[it].w};
                    uint32_t o[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) o[i] = norm_apply(dx[i], dwt[i], dbs[i], na.kind, mean, r);
                    xn[(int64_t)m * chunks + c] = make_uint4(o[0], o[1], o[2], o[3]);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int jj = 0; jj < J; ++jj) {
                uint4 v = xn[(int64_t)m * chunks + cidx[jj]];
                if (!cok[jj]) v = make_uint4(0, 0, 0, 0);
                xr[m][jj][0] = v.x;
                xr[m][jj][1] = v.y;
                xr[m][jj][2] = v.z;
                xr[m][jj][3] = v.w;
            }
    }

    __builtin_amdgcn_s_setprio(0);
    const GemvEpilogue<M, DUAL, AD> ep(W, bias, residual, ldr);
    for (int t = 0; t < iters; ++t) {
        float(*rd)[RU * M * NW] = red[t & 1];
        const GemvEpiOperands eo = ep.request(N, R, t, ad);
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            if (u + PRIME < RU) {
                DENSE_ISSUE_ROW(t, u + PRIME)
            } else if (t + 1 < iters) {
                DENSE_ISSUE_ROW(t + 1, u + PRIME - RU)
            }
            asm volatile("" ::: "memory");
            gemv_prio_ladder<RU, 2>(u);
            float part[NW][M];
#pragma unroll
            for (int q = 0; q < NW; ++q)
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    float p0 = 0.f, p1 = 0.f;
#pragma unroll
                    for (int jj = 0; jj < J; ++jj) {
                        const uint4 ww = w[q][u][jj];
                        p0 = dot2_bf16(ww.x, xr[m][jj][0], p0);
                        p1 = dot2_bf16(ww.y, xr[m][jj][1], p1);
                        p0 = dot2_bf16(ww.z, xr[m][jj][2], p0);
                        p1 = dot2_bf16(ww.w, xr[m][jj][3], p1);
                    }
                    part[q][m] = wave_sum_to_lane63(p0 + p1);
                }
#pragma unroll
            for (int q = 0; q < NW; ++q)
#pragma unroll
                for (int m = 0; m < M; ++m)
                    if (lane == 63) rd[wave][(u * M + m) * NW + q] = part[q][m];
        }
        __syncthreads();
        if ((int)threadIdx.x < R * M) ep.template sum_store<RU>(rd, nslabs, wps, N, R, t, epi, eo, out, ldo);
    }
#undef DENSE_ISSUE_ROW
#undef DENSE_ROW0
}

template <int M, int J, int MAXW>
static int bf16_gemv_launch_jw(const void* W, const void* W2, const void* x, int ldx, const void* bias,
                               const void* residual, int ldr, void* out, int ldo, int N, int K, int epi, const NormArgs& na,
                               int nslabs, const AdapterArgs* ad, hipStream_t st) {
    constexpr int RU = 4, RUD = 2;  // rows per wave and batch (single weight / SwiGLU pair)
    const bool dual = epi == PARROT_EPI_SWIGLU;
    const int ru = dual ? RUD : RU;
    int wps = MAXW / nslabs;
    if (wps > 4) wps = 4;
    while (wps > 1 && (int64_t)wps * ru * 256 > N) --wps;  // small N: keep at least ~256 workgroups
    if (na.kind != 0)  // the cooperative norm covers 4 x 8 x nthreads elements of K
        while (wps * nslabs < MAXW && (K >> 3) > 4 * 64 * nslabs * wps) ++wps;
    const int nthreads = 64 * nslabs * wps;
    size_t lds;
    const int rc = gemv_fused_norm_lds("bf16_gemv", na, M, K, nthreads, &lds);
    if (rc != PARROT_OK) return rc;
    const int per_simd = J <= 5 ? 4 : (J <= 6 ? 3 : 2);  // waves per SIMD the build's VGPR count allows (<= 128 / 170 / 256)
    const GemvGrid g = gemv_grid(N, wps * ru, gemv_resident(4 * per_simd, nslabs * wps));
    const dim3 grid(g.grid), block(nthreads);
    const AdapterArgs adv = ad ? *ad : AdapterArgs{nullptr, nullptr, nullptr, nullptr};
#define PARROT_DENSE_GO(KID, DUALV, RUV, ADV)                                                                             \
    return launch(KID, bf16_gemv_kernel<M, DUALV, J, RUV, MAXW, ADV>, grid, block, lds, st, (const uint4*)W, (const uint4*)W2, \
                  (const bf16_t*)x, ldx, (const bf16_t*)bias, (const bf16_t*)residual, ldr, (bf16_t*)out, ldo, N, K, wps,      \
                  nslabs, epi, g.iters, na, adv)
    if (dual) {
        if (ad) PARROT_DENSE_GO(K_BF16_GEMV_DUAL, true, RUD, true);
        PARROT_DENSE_GO(K_BF16_GEMV_DUAL, true, RUD, false);
    }
    if (ad) PARROT_DENSE_GO(K_BF16_GEMV, false, RU, true);
    PARROT_DENSE_GO(K_BF16_GEMV, false, RU, false);
#undef PARROT_DENSE_GO
}

template <int M, int J>
static int bf16_gemv_launch_j(const void* W, const void* W2, const void* x, int ldx, const void* bias,
                              const void* residual, int ldr, void* out, int ldo, int N, int K, int epi, const NormArgs& na,
                              int nslabs, const AdapterArgs* ad, hipStream_t st) {
    if (nslabs <= 8) return bf16_gemv_launch_jw<M, J, 8>(W, W2, x, ldx, bias, residual, ldr, out, ldo, N, K, epi, na, nslabs, ad, st);
    if constexpr (J <= 4) return bf16_gemv_launch_jw<M, J, 16>(W, W2, x, ldx, bias, residual, ldr, out, ldo, N, K, epi, na, nslabs, ad, st);
    set_error("bf16_gemv: K=%d needs more than 8 slabs of %d loads", K, J);
    return PARROT_EUNSUPPORTED;
}

template <int M>
static int bf16_gemv_launch(const void* W, const void* W2, const void* x, int ldx, const void* bias,
                            const void* residual, int ldr, void* out, int ldo, int N, int K, int epi, const NormArgs& na,
                            const AdapterArgs* ad, hipStream_t st) {
    const int chunks = K / 8;
    const int nslabs = (chunks + 64 * kDenseJ - 1) / (64 * kDenseJ);
    const int per_slab = (chunks + nslabs - 1) / nslabs;  // 16-B units of the largest slab
    const int jn = (per_slab + 63) / 64;
#define PARROT_DENSE_J(JV) \
    if (jn <= JV) return bf16_gemv_launch_j<M, JV>(W, W2, x, ldx, bias, residual, ldr, out, ldo, N, K, epi, na, nslabs, ad, st)
    PARROT_DENSE_J(1);
    PARROT_DENSE_J(2);
    PARROT_DENSE_J(3);
    PARROT_DENSE_J(4);
#undef PARROT_DENSE_J
    set_error("bf16_gemv: K=%d too large", K);
    return PARROT_EUNSUPPORTED;
}

}  // namespace parrot

using namespace parrot;

namespace parrot {

static int bf16_gemv_entry(const void* W, const void* W2, const void* x, int ldx, int M, const void* bias, const void* residual,
                           int ldr, void* out, int ldo, int N, int K, int epilogue, const parrot_norm_t* norm,
                           const AdapterArgs* ad, void* stream) {
    int rc = check_linear_args("bf16_gemv", W, W2, x, ldx, M, residual, ldr, out, ldo, N, K, epilogue);
    if (rc != PARROT_OK) return rc;
    PARROT_UNSUPPORTED(K % 8 == 0, "bf16_gemv: K=%d must be a multiple of 8", K);
    PARROT_UNSUPPORTED(K <= 64 * 8 * kDenseJ * kDenseMaxSlabs, "bf16_gemv: K=%d too large", K);
    PARROT_UNSUPPORTED(!(epilogue == PARROT_EPI_SWIGLU && bias), "bf16_gemv: SWIGLU epilogue takes no bias");
    NormArgs na;
    rc = make_norm_args(norm, K, &na);
    if (rc != PARROT_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    return gemv_for_row_chunks<2>(x, ldx, M, residual, ldr, out, ldo, [&](auto rows, const void* xm, const void* rm, void* om) {
        return bf16_gemv_launch<decltype(rows)::value>(W, W2, xm, ldx, bias, rm, ldr, om, ldo, N, K, epilogue, na, ad, st);
    });
}

// adapter-v2 vectors of the GEMV / element-wise entry points: every vector given is 2-byte aligned device memory; the partner's
// pair only with a partner
int make_adapter_args(const char* who, const parrot_adapter_t* adapter, int epilogue, AdapterArgs* ad) {
    *ad = AdapterArgs{nullptr, nullptr, nullptr, nullptr};
    if (adapter == nullptr) return PARROT_OK;
    PARROT_REQUIRE(epilogue == PARROT_EPI_SWIGLU || (adapter->scale2 == nullptr && adapter->bias2 == nullptr),
                   "%s: scale2 / bias2 belong to the SWIGLU partner", who);
    for (const void* p : {adapter->scale, adapter->bias, adapter->scale2, adapter->bias2})
        PARROT_REQUIRE((reinterpret_cast<uintptr_t>(p) & 1u) == 0, "%s: misaligned adapter vector", who);
    ad->scale = (const bf16_t*)adapter->scale;
    ad->bias = (const bf16_t*)adapter->bias;
    ad->scale2 = (const bf16_t*)adapter->scale2;
    ad->bias2 = (const bf16_t*)adapter->bias2;
    return PARROT_OK;
}

// one thread per output element: out = epilogue(affine(t)), t = bf16(acc + bias) of a PARROT_EPI_NONE GEMM (prompts)
__global__ void __launch_bounds__(256)
adapter_epilogue_kernel(const bf16_t* __restrict__ t, const bf16_t* __restrict__ t2, int ldt, int M, int N, AdapterArgs ad, int epi,
                        const bf16_t* residual, int ldr, bf16_t* out, int ldo) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
    if (col >= N || m >= M) return;
    const float v = bf2f(t[(int64_t)m * ldt + col]);
    const float v2 = epi == PARROT_EPI_SWIGLU ? bf2f(t2[(int64_t)m * ldt + col]) : 0.f;
    const float res = epi == PARROT_EPI_RESIDUAL ? bf2f(residual[(int64_t)m * ldr + col]) : 0.f;
    const float a_s = ad.scale ? bf2f(ad.scale[col]) : 1.f, a_b = ad.bias ? bf2f(ad.bias[col]) : 0.f;
    const float a_s2 = ad.scale2 ? bf2f(ad.scale2[col]) : 1.f, a_b2 = ad.bias2 ? bf2f(ad.bias2[col]) : 0.f;
    out[(int64_t)m * ldo + col] = apply_epilogue_adapter_vals(epi, v, v2, false, 0.f, res, a_s, a_b, a_s2, a_b2);
}

}  // namespace parrot

extern "C" {

int parrot_bf16_gemv(const void* W, const void* W2, const void* x, int ldx, int M, const void* bias,
                     const void* residual, int ldr, void* out, int ldo, int N, int K, int epilogue,
                     const parrot_norm_t* norm, void* stream) {
    return bf16_gemv_entry(W, W2, x, ldx, M, bias, residual, ldr, out, ldo, N, K, epilogue, norm, nullptr, stream);
}

int parrot_bf16_gemv_adapter(const void* W, const void* W2, const void* x, int ldx, int M, const void* bias,
                             const void* residual, int ldr, void* out, int ldo, int N, int K, int epilogue,
                             const parrot_norm_t* norm, const parrot_adapter_t* adapter, void* stream) {
    AdapterArgs ad;
    const int rc = make_adapter_args("bf16_gemv_adapter", adapter, epilogue, &ad);
    if (rc != PARROT_OK) return rc;
    return bf16_gemv_entry(W, W2, x, ldx, M, bias, residual, ldr, out, ldo, N, K, epilogue, norm, adapter ? &ad : nullptr, stream);
}

int parrot_adapter_epilogue(const void* t, const void* t2, int ldt, int M, int N, const parrot_adapter_t* adapter, int epilogue,
                            const void* residual, int ldr, void* out, int ldo, void* stream) {
    PARROT_REQUIRE(t && out, "adapter_epilogue: null pointer");
    PARROT_REQUIRE(M >= 1 && N >= 1 && M <= 65535, "adapter_epilogue: bad shape M=%d N=%d", M, N);
    PARROT_REQUIRE(epilogue >= PARROT_EPI_NONE && epilogue <= PARROT_EPI_SWIGLU, "adapter_epilogue: unknown epilogue %d", epilogue);
    PARROT_REQUIRE((epilogue == PARROT_EPI_SWIGLU) == (t2 != nullptr), "adapter_epilogue: second input iff SWIGLU");
    PARROT_REQUIRE((epilogue == PARROT_EPI_RESIDUAL) == (residual != nullptr), "adapter_epilogue: residual iff RESIDUAL epilogue");
    PARROT_REQUIRE(ldt >= N && ldo >= N && (!residual || ldr >= N), "adapter_epilogue: leading dimension too small");
    PARROT_REQUIRE(out != t && (!t2 || out != t2), "adapter_epilogue: out must not alias the GEMM result");
    AdapterArgs ad;
    const int rc = make_adapter_args("adapter_epilogue", adapter, epilogue, &ad);
    if (rc != PARROT_OK) return rc;
    return launch(K_ADAPTER_EPI, adapter_epilogue_kernel, dim3((N + 255) / 256, M), dim3(256), 0, (hipStream_t)stream,
                  (const bf16_t*)t, (const bf16_t*)t2, ldt, M, N, ad, epilogue, (const bf16_t*)residual, ldr, (bf16_t*)out, ldo);
}

}  // extern "C"
