// CausalSelfAttention without the two Linears (lit_gpt/model.py:194-275):
//   qkv_rope_kvappend : per-group q/k/v split (:208-214), partial RoPE (:226-232, apply_rope :330-336),
//                       KV-cache write (:243-245).  GQA is stored natively: one K/V head per query group
//                       (the reference expands K/V to n_head with repeat_interleave, :217-220).
//   attn_decode       : softmax(q k^T / sqrt(hs)) v over the cached slots the causal mask admits
//                       (:256-275 with the mask rows built at :88-92), flash-decoding style split over the
//                       sequence + a combine pass.
//
// Cache layout: [n_groups][S][hs] bf16.  Slot of position p is p % S: when p >= S this overwrites the oldest
// entry, which is what the reference's roll-left + write-last does (:238-245) up to slot order.
//
// Decode attention is memory-bound on K/V rows.  A K (or V) row of hs bf16 is read by hs/8 lanes with one
// 16-B load each, so one wave instruction covers 64*8/hs rows (1 KiB contiguous); scores are reduced over
// those lanes with shuffles; every (wave, row-slot) keeps its own online-softmax state (m, l, acc[8]) in
// registers and the states are merged once at the end through LDS.
#include <hip/hip_fp16.h>

#include <type_traits>

#include "parrot_common.h"

namespace parrot {

// ------------------------------------------------------------------------------------------ rope + kv append
// one thread per (row m, head-slot j in [0, n_groups*(q_per_kv+2)), pair index i in [0, hs/2))
__global__ void __launch_bounds__(256)
rope_kvappend_kernel(const bf16_t* __restrict__ qkv, int ldqkv, int M, const __half* __restrict__ rope_cos,
                     const __half* __restrict__ rope_sin, int n_elem, int rope_local, const int32_t* __restrict__ pos_ptr, int n_groups,
                     int q_per_kv, int hs, int S, bf16_t* __restrict__ q_out, bf16_t* __restrict__ k_cache,
                     bf16_t* __restrict__ v_cache) {
    const int half_hs = hs >> 1;
    const int per_group = q_per_kv + 2;
    const int slots = n_groups * per_group;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(tid % half_hs);
    const int j = (int)((tid / half_hs) % slots);
    const int m = (int)(tid / ((int64_t)half_hs * slots));
    if (m >= M) return;
    const int g = j / per_group, t = j % per_group;  // t < q_per_kv: query head; == q_per_kv: key; else value
    const int pos = pos_ptr[0] + m;
    const bf16_t* src = qkv + (int64_t)m * ldqkv + (int64_t)j * hs;
    bf16_t* dst;
    if (t < q_per_kv)
        dst = q_out + ((int64_t)m * n_groups * q_per_kv + (int64_t)g * q_per_kv + t) * hs;
    else if (t == q_per_kv)
        dst = k_cache + ((int64_t)g * S + (pos % S)) * hs;
    else
        dst = v_cache + ((int64_t)g * S + (pos % S)) * hs;

    const int half_n = n_elem >> 1;
    // element pair handled by this thread: (i, i + half_n) inside the rotary part, or two pass-through dims
    if (t <= q_per_kv && i < half_n) {
        const float x1 = bf2f(src[i]), x2 = bf2f(src[i + half_n]);
        const int64_t rrow = rope_local ? m : pos;  // tables pre-indexed per row (Block.forward callers) or absolute
        const float c1 = __half2float(rope_cos[rrow * n_elem + i]);
        const float s1 = __half2float(rope_sin[rrow * n_elem + i]);
        const float c2 = __half2float(rope_cos[rrow * n_elem + i + half_n]);
        const float s2 = __half2float(rope_sin[rrow * n_elem + i + half_n]);
        // roped = x*cos + rotate_half(x)*sin, every product and the sum rounded to fp32 separately (no FMA),
        // as the reference's promoted bf16*fp16 tensor ops do (model.py:330-336)
        const float o1 = __fadd_rn(__fmul_rn(x1, c1), __fmul_rn(-x2, s1));
        const float o2 = __fadd_rn(__fmul_rn(x2, c2), __fmul_rn(x1, s2));
        dst[i] = f2bf(o1);
        dst[i + half_n] = f2bf(o2);
    } else {
        // pass-through: value heads entirely, and dims >= n_elem of q/k.  Thread i covers 2 dims.
        const int base = (t <= q_per_kv) ? n_elem : 0;
        const int idx = (t <= q_per_kv) ? (i - half_n) * 2 : i * 2;
        dst[base + idx] = src[base + idx];
        dst[base + idx + 1] = src[base + idx + 1];
    }
}

// The same, eight dims per thread (16-byte loads / stores): one thread per (row, head slot, 8-dim chunk).  Chunk u of a query / key head
// inside the first half of the rotary part handles dims 8u .. 8u+7 AND their partners 8u + n_elem/2 ..; the chunks of the second half
// idle (their partner thread wrote them); everything else is a 16-byte copy.  Needs hs % 8 == 0, n_elem % 16 == 0 and 16-byte rows
// (every BASELINE config); the pair kernel above stays for the rest.  StableLM-3B, 512 rows x 12288 columns: 16.7 -> 9.3 us per launch.
__global__ void __launch_bounds__(256)
rope_kvappend8_kernel(const bf16_t* __restrict__ qkv, int ldqkv, int M, const __half* __restrict__ rope_cos,
                      const __half* __restrict__ rope_sin, int n_elem, int rope_local, const int32_t* __restrict__ pos_ptr, int n_groups,
                      int q_per_kv, int hs, int S, bf16_t* __restrict__ q_out, bf16_t* __restrict__ k_cache,
                      bf16_t* __restrict__ v_cache) {
    const unsigned U = (unsigned)hs >> 3;  // chunks per head
    const unsigned per_group = (unsigned)q_per_kv + 2, slots = (unsigned)n_groups * per_group;
    const unsigned per_row = slots * U;
    const int m = (int)blockIdx.y;
    const unsigned w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= per_row) return;
    const unsigned j = w / U, u = w - j * U;
    const unsigned g = j / per_group, t = j - g * per_group;  // t < q_per_kv: query head; == q_per_kv: key; else value
    const int pos = pos_ptr[0] + m;
    const bf16_t* src = qkv + (int64_t)m * ldqkv + (int64_t)j * hs;
    bf16_t* dst;
    if (t < (unsigned)q_per_kv)
        dst = q_out + ((int64_t)m * n_groups * q_per_kv + (int64_t)g * q_per_kv + t) * hs;
    else if (t == (unsigned)q_per_kv)
        dst = k_cache + ((int64_t)g * S + (pos % S)) * hs;
    else
        dst = v_cache + ((int64_t)g * S + (pos % S)) * hs;
    const unsigned half_n = (unsigned)n_elem >> 1, uh = half_n >> 3, un = (unsigned)n_elem >> 3;
    if (t <= (unsigned)q_per_kv && u < un) {
        if (u >= uh) return;  // second half of the rotary part: written by the thread of chunk u - uh
        const uint4 a = *reinterpret_cast<const uint4*>(src + 8 * u), b = *reinterpret_cast<const uint4*>(src + 8 * u + half_n);
        const int64_t rrow = rope_local ? m : pos;
        const __half* cr = rope_cos + rrow * n_elem + 8 * u;
        const __half* sr = rope_sin + rrow * n_elem + 8 * u;
        const uint4 c1 = *reinterpret_cast<const uint4*>(cr), s1 = *reinterpret_cast<const uint4*>(sr);
        const uint4 c2 = *reinterpret_cast<const uint4*>(cr + half_n), s2 = *reinterpret_cast<const uint4*>(sr + half_n);
        const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
        const uint32_t c1w[4] = {c1.x, c1.y, c1.z, c1.w}, s1w[4] = {s1.x, s1.y, s1.z, s1.w};
        const uint32_t c2w[4] = {c2.x, c2.y, c2.z, c2.w}, s2w[4] = {s2.x, s2.y, s2.z, s2.w};
        uint32_t o1[4], o2[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            bf16_t r1[2], r2[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float x1 = h ? bfhi(aw[d]) : bflo(aw[d]), x2 = h ? bfhi(bw[d]) : bflo(bw[d]);
                const float fc1 = __half2float(__ushort_as_half((unsigned short)(c1w[d] >> (16 * h))));
                const float fs1 = __half2float(__ushort_as_half((unsigned short)(s1w[d] >> (16 * h))));
                const float fc2 = __half2float(__ushort_as_half((unsigned short)(c2w[d] >> (16 * h))));
                const float fs2 = __half2float(__ushort_as_half((unsigned short)(s2w[d] >> (16 * h))));
                // (the pair kernel's arithmetic: every product and the sum rounded to fp32 separately, no FMA)
                r1[h] = f2bf(__fadd_rn(__fmul_rn(x1, fc1), __fmul_rn(-x2, fs1)));
                r2[h] = f2bf(__fadd_rn(__fmul_rn(x2, fc2), __fmul_rn(x1, fs2)));
            }
            o1[d] = (uint32_t)r1[0] | ((uint32_t)r1[1] << 16);
            o2[d] = (uint32_t)r2[0] | ((uint32_t)r2[1] << 16);
        }
        *reinterpret_cast<uint4*>(dst + 8 * u) = make_uint4(o1[0], o1[1], o1[2], o1[3]);
        *reinterpret_cast<uint4*>(dst + 8 * u + half_n) = make_uint4(o2[0], o2[1], o2[2], o2[3]);
    } else {
        *reinterpret_cast<uint4*>(dst + 8 * u) = *reinterpret_cast<const uint4*>(src + 8 * u);
    }
}

// ------------------------------------------------------------------------------------------ decode attention
constexpr int kAttnWaves = 4;

// partial state layout in the workspace: [M][n_head][nsplit][hs + 2] floats: acc[hs], m, l
// HQ = query heads of the group processed in one pass over the K/V rows (1 for MHA, up to 4 for GQA/MQA)
//
// PM ("softmax_mode 1", parity runs only): the softmax as torch's CPU flash-attention kernel computes it for the bf16 reference
// (lit_gpt/model.py:256-275 -> scaled_dot_product_attention): the probabilities p = exp(s - max) are ROUNDED TO bf16 before
// they multiply V, with the row maximum of the whole key block as the reference point (torch walks the keys in blocks of 512:
// for windows up to 512 keys that is the global maximum, and this mode is refused beyond), while the denominator sums the
// unrounded p; accurate expf.  It needs the maximum before the first product, hence a pass over the K rows (scores only) in
// front of the normal one.  The default (PM = false) keeps p in fp32: closer to the exact result, further from the
// reference's bits.
template <int HS, int HQ, bool PM = false>
__global__ void __launch_bounds__(kAttnWaves * 64)
attn_decode_kernel(const bf16_t* __restrict__ q, const int32_t* __restrict__ pos_ptr, const bf16_t* __restrict__ k_cache,
                   const bf16_t* __restrict__ v_cache, int n_groups, int q_per_kv, int S, int nsplit,
                   float* __restrict__ ws, bf16_t* __restrict__ y, int ldy) {
    constexpr int LPR = HS / 8;    // lanes per K/V row
    constexpr int RPW = 64 / LPR;  // rows per wave instruction
    constexpr int STRIDE = kAttnWaves * RPW;
    __shared__ float sh_acc[HQ][kAttnWaves][HS];  // one merged state per wave
    __shared__ float sh_m[HQ][kAttnWaves], sh_l[HQ][kAttnWaves];

    const int g = blockIdx.x, split = blockIdx.y, m = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, dl = lane % LPR;
    const int n_head = n_groups * q_per_kv;
    const int pos = pos_ptr[0] + m;
    const int n_valid = min(pos + 1, S);  // slots 0..n_valid-1 hold the admitted keys
    const int per = (S + nsplit - 1) / nsplit;
    const int s_begin = split * per, s_end = min(n_valid, s_begin + per);
    const int s_last = max(s_end - 1, 0);
    const float scale = 1.0f / sqrtf((float)HS);
    const uint4* kc = reinterpret_cast<const uint4*>(k_cache + (int64_t)g * S * HS);
    const uint4* vc = reinterpret_cast<const uint4*>(v_cache + (int64_t)g * S * HS);
    const int s_first = s_begin + wave * RPW;

    for (int h0 = 0; h0 < q_per_kv; h0 += HQ) {
        // the same key loop as the fused single-token kernel below: packed-bf16 dot2 scores, DPP sums over the lanes of a
        // key, two K/V register sets in ping-pong with unconditional (clamped) loads, slots merged in-wave
        uint32_t qp[HQ][4];
        float mrun[HQ], lrun[HQ], acc[HQ][8];
#pragma unroll
        for (int hh = 0; hh < HQ; ++hh) {
            const int head = g * q_per_kv + min(h0 + hh, q_per_kv - 1);
            const uint4 qv = reinterpret_cast<const uint4*>(q + ((int64_t)m * n_head + head) * HS)[dl];
            qp[hh][0] = qv.x;
            qp[hh][1] = qv.y;
            qp[hh][2] = qv.z;
            qp[hh][3] = qv.w;
            mrun[hh] = -INFINITY;
            lrun[hh] = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[hh][e] = 0.f;
        }
        float gmax[HQ];  // PM: the maximum score over all the keys of this row and head
        if constexpr (PM) {
#pragma unroll
            for (int hh = 0; hh < HQ; ++hh) gmax[hh] = -INFINITY;
            for (int s0 = s_first; s0 < s_end; s0 += STRIDE) {
                const uint4 kv = kc[(int64_t)min(s0 + sub, s_last) * LPR + dl];
#pragma unroll
                for (int hh = 0; hh < HQ; ++hh) {
                    float p0 = dot2_bf16(kv.x, qp[hh][0], 0.f), p1 = dot2_bf16(kv.y, qp[hh][1], 0.f);
                    p0 = dot2_bf16(kv.z, qp[hh][2], p0);
                    p1 = dot2_bf16(kv.w, qp[hh][3], p1);
                    if (s0 + sub < s_end) gmax[hh] = fmaxf(gmax[hh], group_sum<LPR>(p0 + p1) * scale);
                    else (void)group_sum<LPR>(p0 + p1);
                }
            }
            __syncthreads();  // (the previous head chunk's merge has finished reading sh_m)
#pragma unroll
            for (int hh = 0; hh < HQ; ++hh) {
                gmax[hh] = slot_allreduce<LPR, true>(gmax[hh]);
                if (lane == 0) sh_m[hh][wave] = gmax[hh];
            }
            __syncthreads();
#pragma unroll
            for (int hh = 0; hh < HQ; ++hh) {
                for (int t = 0; t < kAttnWaves; ++t) gmax[hh] = fmaxf(gmax[hh], sh_m[hh][t]);
                mrun[hh] = gmax[hh];
            }
        }
        auto step = [&](const uint4 kv, const uint4 vv, int s) {
            const bool ok = s < s_end;
            const uint32_t vd[4] = {vv.x, vv.y, vv.z, vv.w};
            float vf[8];
#pragma unroll
            for (int jq = 0; jq < 4; ++jq) {
                vf[2 * jq] = bflo(vd[jq]);
                vf[2 * jq + 1] = bfhi(vd[jq]);
            }
#pragma unroll
            for (int hh = 0; hh < HQ; ++hh) {
                float p0 = dot2_bf16(kv.x, qp[hh][0], 0.f), p1 = dot2_bf16(kv.y, qp[hh][1], 0.f);
                p0 = dot2_bf16(kv.z, qp[hh][2], p0);
                p1 = dot2_bf16(kv.w, qp[hh][3], p1);
                const float sc_ = ok ? group_sum<LPR>(p0 + p1) * scale : -INFINITY;
                if constexpr (PM) {
                    const float p = ok ? expf(sc_ - gmax[hh]) : 0.f;
                    const float pr = rbf(p);  // the probability as the reference's P.V product sees it
                    lrun[hh] += p;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[hh][e] = fmaf(pr, vf[e], acc[hh][e]);
                    continue;
                }
                const float mn = fmaxf(mrun[hh], sc_);
                const float corr = (mn == -INFINITY) ? 1.f : __expf(mrun[hh] - mn);
                const float p = (mn == -INFINITY) ? 0.f : __expf(sc_ - mn);
                lrun[hh] = lrun[hh] * corr + p;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[hh][e] = acc[hh][e] * corr + p * vf[e];
                mrun[hh] = mn;
            }
        };
        const int sc0 = min(s_first + sub, s_last);
        uint4 k0 = kc[(int64_t)sc0 * LPR + dl], v0 = vc[(int64_t)sc0 * LPR + dl];
        for (int s0 = s_first; s0 < s_end; s0 += 2 * STRIDE) {
            const int sn1 = min(s0 + STRIDE + sub, s_last);
            const uint4 k1 = kc[(int64_t)sn1 * LPR + dl], v1 = vc[(int64_t)sn1 * LPR + dl];
            step(k0, v0, s0 + sub);
            const int sn2 = min(s0 + 2 * STRIDE + sub, s_last);
            k0 = kc[(int64_t)sn2 * LPR + dl];
            v0 = vc[(int64_t)sn2 * LPR + dl];
            if (s0 + STRIDE < s_end) step(k1, v1, s0 + STRIDE + sub);  // wave-uniform
        }
        __syncthreads();  // the previous head chunk's merge has finished reading the LDS states
#pragma unroll
        for (int hh = 0; hh < HQ; ++hh) {
            const float mw = slot_allreduce<LPR, true>(mrun[hh]);
            const float c = (mrun[hh] == -INFINITY) ? 0.f : __expf(mrun[hh] - mw);
            lrun[hh] = slot_allreduce<LPR, false>(lrun[hh] * c);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[hh][e] = slot_allreduce<LPR, false>(acc[hh][e] * c);
            mrun[hh] = mw;
            if (sub == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) sh_acc[hh][wave][dl * 8 + e] = acc[hh][e];
                if (dl == 0) {
                    sh_m[hh][wave] = mrun[hh];
                    sh_l[hh][wave] = lrun[hh];
                }
            }
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < HQ * HS; idx += kAttnWaves * 64) {
            const int hh = idx / HS, d = idx % HS;
            if (h0 + hh < q_per_kv) {
                float mx = -INFINITY;
                for (int t = 0; t < kAttnWaves; ++t) mx = fmaxf(mx, sh_m[hh][t]);
                float l = 0.f, a = 0.f;
                for (int t = 0; t < kAttnWaves; ++t) {
                    const float mt = sh_m[hh][t];
                    const float w = (mt == -INFINITY) ? 0.f : __expf(mt - mx);
                    l += sh_l[hh][t] * w;
                    a += sh_acc[hh][t][d] * w;
                }
                const int head = g * q_per_kv + h0 + hh;
                if (nsplit == 1) {
                    y[(int64_t)m * ldy + (int64_t)head * HS + d] = f2bf(a / l);
                } else {
                    float* p = ws + (((int64_t)m * n_head + head) * nsplit + split) * (HS + 2);
                    p[d] = a;
                    if (d == 0) {
                        p[HS] = mx;
                        p[HS + 1] = l;
                    }
                }
            }
        }
    }
}

// merge the nsplit partial states of one (row, head); one thread per output dim
template <int HS>
__global__ void __launch_bounds__(HS)
attn_combine_kernel(const float* __restrict__ ws, int nsplit, bf16_t* __restrict__ y, int ldy, int n_head) {
    const int head = blockIdx.x, m = blockIdx.y, d = threadIdx.x;
    const float* p = ws + ((int64_t)m * n_head + head) * nsplit * (HS + 2);
    float mx = -INFINITY;
    for (int t = 0; t < nsplit; ++t) mx = fmaxf(mx, p[t * (HS + 2) + HS]);
    float l = 0.f, a = 0.f;
    for (int t = 0; t < nsplit; ++t) {
        const float mt = p[t * (HS + 2) + HS];
        const float w = (mt == -INFINITY) ? 0.f : __expf(mt - mx);
        l += p[t * (HS + 2) + HS + 1] * w;
        a += p[t * (HS + 2) + d] * w;
    }
    y[(int64_t)m * ldy + (int64_t)head * HS + d] = f2bf(a / l);
}

// ------------------------------------------------------------------------------------------ fused decode step
// One launch per layer for a single new token (M = 1): q/k/v split + RoPE + KV append + attention over the cache +
// the cross-split combine.  Replaces rope_kvappend + attn_decode + attn_combine (3 launches) on the decode path.
//   * every workgroup (group g, split j) ropes q, k_new, v_new of its group itself (a few hundred elements);
//   * the workgroup whose slot range contains slot(pos) writes the new K/V row to the cache; in the loop that row is
//     taken from registers, never from the global copy that is being written;
//   * partial softmax states go to the workspace with write-through (agent-scope) stores; an arrival ticket per group
//     elects the last workgroup, which merges the splits (guide recipe: sc1 payload -> every wave vmcnt(0) -> barrier
//     -> one relaxed agent atomic; reducer reads with agent-scope loads).  The ticket is reset by the reducer.
constexpr int kFusedMaxQ = 16;  // query heads per group held in LDS

__device__ __forceinline__ void store_agent(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float load_agent(const float* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// diagnostic stamps (tools/microbench.py --attn): 100 MHz clock of workgroup (0,0,0) at phase boundaries; the buffer
// pointer is a kernel argument (a scalar load - see w4.hip for why it must not be a global)
__device__ __forceinline__ void attn_stamp(unsigned long long* dbg, int i) {
    if (dbg != nullptr && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        dbg[i] = __builtin_amdgcn_s_memrealtime();
}
#ifdef PARROT_DIAG
static unsigned long long* g_attn_dbg_host = nullptr;  // diagnostic build only: set by parrot_tune_attn_stamps
#else
static constexpr unsigned long long* g_attn_dbg_host = nullptr;
#endif

// ------------------------------------------------------------------------------------------ LLaMA-Adapter prefix
// lit_gpt/adapter.py:226-254: every roped query row attends to ALL aT prefix keys of its group (no mask, no RoPE on the prefix,
// a softmax of its own, scale 1/sqrt(hs)) and y = y + gating_factor * ay, each of the three results rounded to bf16.
// One wave per (row, head): lane j scores prefix key j, then each lane owns the output dims lane, lane + 64.  Both kernels that
// add the term (the fused decode step and the multi-row pass) call this one function, so they agree bit for bit.
constexpr int kAdapterMaxT = 64;

struct AdapterAttnArgs {
    const bf16_t* ak;    // [n_groups][aT][HS]
    const bf16_t* av;    // [n_groups][aT][HS]
    const bf16_t* gate;  // [n_head]
    int aT;
};

template <int HS>
__device__ __forceinline__ void adapter_prefix_wave(const bf16_t* q, const bf16_t* __restrict__ ak, const bf16_t* __restrict__ av,
                                                    int aT, bool pm, float (&ay)[(HS + 63) / 64]) {
    constexpr int ND = (HS + 63) / 64, PV = 8;  // output dims per lane; prefix value rows requested per batch
    const int lane = threadIdx.x & 63;
    const float scale = 1.0f / sqrtf((float)HS);
    // the first PV value rows do not depend on the scores: requested here, their latency hides behind the score loop (rows past aT
    // are clamped and never used)
    float vb[ND][PV];
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int u = 0; u < PV; ++u) vb[i][u] = bf2f(av[(int64_t)min(u, aT - 1) * HS + min(lane + 64 * i, HS - 1)]);
    float s = -INFINITY;
    if (lane < aT) {
        const uint4* kr = reinterpret_cast<const uint4*>(ak + (int64_t)lane * HS);
        const uint4* qr = reinterpret_cast<const uint4*>(q);
        float p0 = 0.f, p1 = 0.f;
#pragma unroll 4  // (fully unrolled, the 2 x HS/8 16-B loads of a 128-dim row are all hoisted: the 16-wave kernel spilled)
        for (int c = 0; c < HS / 8; ++c) {
            const uint4 kv = kr[c], qv = qr[c];
            p0 = dot2_bf16(kv.x, qv.x, p0);
            p1 = dot2_bf16(kv.y, qv.y, p1);
            p0 = dot2_bf16(kv.z, qv.z, p0);
            p1 = dot2_bf16(kv.w, qv.w, p1);
        }
        s = __fmul_rn(__fadd_rn(p0, p1), scale);
    }
    const float mx = wave_max(s);
    const float p = lane < aT ? expf(__fsub_rn(s, mx)) : 0.f;
    const float l = wave_sum(p);
    const float pr = pm ? rbf(p) : p;  // softmax_mode 1: the probabilities rounded to bf16 before P.V, the sum from the unrounded ones
    // P.V in key order (a = fma(p_j, v_j, a), j = 0 .. aT-1), PV value rows per batch requested together
    float acc[ND];
#pragma unroll
    for (int i = 0; i < ND; ++i) acc[i] = 0.f;
    for (int j0 = 0; j0 < aT; j0 += PV) {
        if (j0 > 0) {
#pragma unroll
            for (int i = 0; i < ND; ++i)
#pragma unroll
                for (int u = 0; u < PV; ++u)
                    vb[i][u] = bf2f(av[(int64_t)min(j0 + u, aT - 1) * HS + min(lane + 64 * i, HS - 1)]);
        }
#pragma unroll
        for (int u = 0; u < PV; ++u) {
            if (j0 + u < aT) {  // wave-uniform
                const float pj = __shfl(pr, j0 + u, 64);
#pragma unroll
                for (int i = 0; i < ND; ++i) acc[i] = fmaf(pj, vb[i][u], acc[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < ND; ++i) ay[i] = rbf(__fdiv_rn(acc[i], l));
}

// y = bf16(y + bf16(gate * ay)) (the gating product and the sum rounded separately, as two bf16 tensor ops do)
__device__ __forceinline__ bf16_t adapter_combine(float y, float gate, float ay) {
    return f2bf(__fadd_rn(y, rbf(__fmul_rn(gate, ay))));
}

// LDS of the fused kernel's prefix outputs; only the AD instantiations call this, so the plain kernel allocates nothing
template <int N>
__device__ __forceinline__ float* adapter_lds() {
    __shared__ float buf[N];
    return buf;
}

// the fused kernel's workgroup: wave hh < HQ computes query head h0 + hh of group g into sh_ay[hh][*]
template <int HS, int HQ, bool PM>
__device__ __forceinline__ void adapter_prefix_heads(const AdapterAttnArgs& aa, const bf16_t (*sh_q)[HS], int g, int h0, int q_per_kv,
                                                     float* sh_ay) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave < HQ && h0 + wave < q_per_kv) {
        float ay[(HS + 63) / 64];
        adapter_prefix_wave<HS>(sh_q[h0 + wave], aa.ak + (int64_t)g * aa.aT * HS, aa.av + (int64_t)g * aa.aT * HS, aa.aT, PM, ay);
#pragma unroll
        for (int i = 0; i < (HS + 63) / 64; ++i)
            if (lane + 64 * i < HS) sh_ay[wave * HS + lane + 64 * i] = ay[i];
    }
}

// multi-row pass (prompts, rope_local, the unfused single-row path): one wave per (head, row), in place on y
template <int HS>
__global__ void __launch_bounds__(64)
attn_adapter_prefix_kernel(const bf16_t* __restrict__ q, int n_head, AdapterAttnArgs aa, int q_per_kv, bf16_t* y, int ldy, int pm) {
    const int head = blockIdx.x, m = blockIdx.y, lane = threadIdx.x;
    const int g = head / q_per_kv;
    float ay[(HS + 63) / 64];
    adapter_prefix_wave<HS>(q + ((int64_t)m * n_head + head) * HS, aa.ak + (int64_t)g * aa.aT * HS, aa.av + (int64_t)g * aa.aT * HS,
                            aa.aT, pm != 0, ay);
    const float gate = bf2f(aa.gate[head]);
#pragma unroll
    for (int i = 0; i < (HS + 63) / 64; ++i) {
        const int d = lane + 64 * i;
        if (d < HS) {
            bf16_t* yp = y + (int64_t)m * ldy + (int64_t)head * HS + d;
            *yp = adapter_combine(bf2f(*yp), gate, ay[i]);
        }
    }
}

// Batched decode (parrot_attn_fused_decode_rows): B independent sequences, one row each.  Row b reads qkv + b * ldqkv, its
// own position pos[b], its own caches at + b * kv_bstride, writes y + b * ldy, and owns the workspace slice and the n_head
// tickets from b * n_head on.  The row index is folded into grid.z (b * chunks + chunk).
struct AttnRowsArgs {
    int ldqkv, ldy;
    int64_t kv_bstride;
};

// AD: the LLaMA-Adapter prefix term is added by the workgroup that writes y (AD = false is the plain kernel)
// ROWS: the batched-decode instantiation; with ROWS = false `rows` is never read and the kernel is the one-row kernel
// SEQ (with ROWS): the rows are CONSECUTIVE tokens of ONE sequence (parrot_attn_fused_decode_seq): row b sits at position
// pos[0] + b and attends to slots 0 .. pos[0] + b of the one shared cache (kv_bstride 0).  The K/V rows of all the rows were
// appended by parrot_qkv_rope_kvappend in the launch before, so this instantiation appends nothing and no workgroup reads a
// slot that another workgroup of the same launch writes; a row's own K/V still come from its registers.
template <int HS, int HQ, int WAVES, bool PM = false, bool AD = false, bool ROWS = false, bool SEQ = false>  // PM: "softmax_mode 1", see attn_decode_kernel
__global__ void __launch_bounds__(WAVES * 64)
attn_fused_decode_kernel(const bf16_t* __restrict__ qkv, const __half* __restrict__ rope_cos,
                         const __half* __restrict__ rope_sin, int n_elem, const int32_t* __restrict__ pos_ptr,
                         bf16_t* __restrict__ k_cache, bf16_t* __restrict__ v_cache, int n_groups, int q_per_kv, int S,
                         int nsplit, float* __restrict__ ws, unsigned int* __restrict__ tickets, bf16_t* __restrict__ y,
                         unsigned long long* dbg, AdapterAttnArgs aa, AttnRowsArgs rows) {
    constexpr int LPR = HS / 8;
    constexpr int RPW = 64 / LPR;
    attn_stamp(dbg, 0);
    __shared__ float sh_acc[HQ][WAVES][HS];  // one merged state per wave
    __shared__ float sh_m[HQ][WAVES], sh_l[HQ][WAVES];
    __shared__ __attribute__((aligned(16))) bf16_t sh_q[kFusedMaxQ][HS];  // roped q rows as bf16 (the scale is applied to the score)
    __shared__ __attribute__((aligned(16))) bf16_t sh_kv[2][HS];  // roped k_new, v_new as stored in the cache
    __shared__ int sh_last;

    const int n_head = n_groups * q_per_kv;
    int chunk = blockIdx.z;  // chunk of the group's query heads
    int seq_row = 0;         // SEQ: this row's offset from pos[0]
    unsigned int* ticket;
    if constexpr (ROWS) {
        const int nchunk = (q_per_kv + HQ - 1) / HQ;
        const int b = blockIdx.z / nchunk;
        chunk = blockIdx.z - b * nchunk;
        qkv += (int64_t)b * rows.ldqkv;
        if constexpr (SEQ)
            seq_row = b;
        else
            pos_ptr += b;
        k_cache += b * rows.kv_bstride;
        v_cache += b * rows.kv_bstride;
        ws += (int64_t)b * n_head * nsplit * (HS + 2);
        y += (int64_t)b * rows.ldy;
        ticket = &tickets[b * n_head + blockIdx.x * nchunk + chunk];
    } else {
        ticket = &tickets[blockIdx.x * gridDim.z + blockIdx.z];
    }
    const int g = blockIdx.x, split = blockIdx.y;
    const int h0 = chunk * HQ;  // this workgroup's chunk of the group's query heads (GQA: chunks run in parallel)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, dl = lane % LPR;
    const int pos = SEQ ? pos_ptr[0] + seq_row : pos_ptr[0];
    const int n_valid = min(pos + 1, S);
    const int slot_new = pos % S;
    const int per = (S + nsplit - 1) / nsplit;
    const int s_begin = split * per, s_end = min(n_valid, s_begin + per);
    const float scale = 1.0f / sqrtf((float)HS);
    const int half_n = n_elem >> 1;

    const uint4* kc = reinterpret_cast<const uint4*>(k_cache + (int64_t)g * S * HS);
    const uint4* vc = reinterpret_cast<const uint4*>(v_cache + (int64_t)g * S * HS);
    constexpr int STRIDE = WAVES * RPW;
    // Load order matters (vmcnt retires in order): first the small L2-resident operands of the RoPE phase (this
    // group's q/k/v rows, cos/sin), then the first K/V rows of this wave, which do not depend on q — their HBM latency
    // overlaps the split + RoPE phase.  (Rows past the range are clamped; the appended row is replaced later.)
    constexpr int ROPE_IT = ((kFusedMaxQ + 2) * HS + WAVES * 64 - 1) / (WAVES * 64);
    const bf16_t* grp = qkv + (int64_t)g * (q_per_kv + 2) * HS;
    const int n_rope_elems = (q_per_kv + 2) * HS;
    float rx[ROPE_IT], ro[ROPE_IT], rc[ROPE_IT], rs[ROPE_IT];
#pragma unroll
    for (int it = 0; it < ROPE_IT; ++it) {
        const int idx = threadIdx.x + it * WAVES * 64;
        rx[it] = ro[it] = rs[it] = 0.f;
        rc[it] = 1.f;
        if (idx < n_rope_elems) {
            const int t = idx / HS, d = idx % HS;
            rx[it] = bf2f(grp[idx]);
            if (t <= q_per_kv && d < n_elem) {
                rc[it] = __half2float(rope_cos[(int64_t)pos * n_elem + d]);
                rs[it] = __half2float(rope_sin[(int64_t)pos * n_elem + d]);
                ro[it] = d < half_n ? -bf2f(grp[idx + half_n]) : bf2f(grp[idx - half_n]);
            }
        }
    }
    const int s_first = s_begin + wave * RPW;
    // first K/V rows of this wave: requested here, before the RoPE phase (clamped, unconditional)
    const int sc_first = min(s_first + sub, max(s_end - 1, 0));
    const uint4 kv_cur = kc[(int64_t)sc_first * LPR + dl];
    const uint4 vv_cur = vc[(int64_t)sc_first * LPR + dl];

    // ---- split + RoPE of this group's rows (reference model.py:208-232): x*cos + rotate_half(x)*sin, each product and
    // the sum rounded to fp32 separately; elements outside the rotary part pass through (cos = 1, sin = 0 is exact)
#pragma unroll
    for (int it = 0; it < ROPE_IT; ++it) {
        const int idx = threadIdx.x + it * WAVES * 64;
        if (idx < n_rope_elems) {
            const int t = idx / HS, d = idx % HS;
            const float v = __fadd_rn(__fmul_rn(rx[it], rc[it]), __fmul_rn(ro[it], rs[it]));
            const bf16_t vb = f2bf(v);
            if (t < q_per_kv)
                sh_q[t][d] = vb;
            else
                sh_kv[t - q_per_kv][d] = vb;
        }
    }
    __syncthreads();
    attn_stamp(dbg, 1);
    // ---- KV append by the workgroup that owns the new slot (SEQ: appended by the launch before)
    if (!SEQ && chunk == 0 && slot_new >= s_begin && slot_new < s_begin + per && threadIdx.x < 2 * LPR) {
        const int which = threadIdx.x / LPR, c = threadIdx.x % LPR;
        bf16_t* dst = (which ? v_cache : k_cache) + ((int64_t)g * S + slot_new) * HS;
        reinterpret_cast<uint4*>(dst)[c] = reinterpret_cast<const uint4*>(sh_kv[which])[c];
    }
    const uint4 knew = reinterpret_cast<const uint4*>(sh_kv[0])[dl];
    const uint4 vnew = reinterpret_cast<const uint4*>(sh_kv[1])[dl];

    {
        uint32_t qp[HQ][4];  // this lane's 8 dims of every query head, packed bf16 pairs (operand of v_dot2_f32_bf16)
        float mrun[HQ], lrun[HQ], acc[HQ][8];
#pragma unroll
        for (int hh = 0; hh < HQ; ++hh) {
            const int hq = min(h0 + hh, q_per_kv - 1);
            const uint4 qv = reinterpret_cast<const uint4*>(sh_q[hq])[dl];
            qp[hh][0] = qv.x;
            qp[hh][1] = qv.y;
            qp[hh][2] = qv.z;
            qp[hh][3] = qv.w;
            mrun[hh] = -INFINITY;
            lrun[hh] = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[hh][e] = 0.f;
        }
        const int s_last = max(s_end - 1, 0);
        float gmax[HQ];  // PM: the maximum score over all the keys of this head
        if constexpr (PM) {
#pragma unroll
            for (int hh = 0; hh < HQ; ++hh) gmax[hh] = -INFINITY;
            for (int s0 = s_first; s0 < s_end; s0 += STRIDE) {
                const int sk = min(s0 + sub, s_last);
                uint4 kv = kc[(int64_t)sk * LPR + dl];
                if (sk == slot_new) kv = knew;  // the row being appended by this launch
#pragma unroll
                for (int hh = 0; hh < HQ; ++hh) {
                    float p0 = dot2_bf16(kv.x, qp[hh][0], 0.f), p1 = dot2_bf16(kv.y, qp[hh][1], 0.f);
                    p0 = dot2_bf16(kv.z, qp[hh][2], p0);
                    p1 = dot2_bf16(kv.w, qp[hh][3], p1);
                    const float sc_ = group_sum<LPR>(p0 + p1) * scale;
                    if (s0 + sub < s_end) gmax[hh] = fmaxf(gmax[hh], sc_);
                }
            }
#pragma unroll
            for (int hh = 0; hh < HQ; ++hh) {
                gmax[hh] = slot_allreduce<LPR, true>(gmax[hh]);
                if (lane == 0) sh_m[hh][wave] = gmax[hh];
            }
            __syncthreads();
#pragma unroll
            for (int hh = 0; hh < HQ; ++hh) {
                for (int t = 0; t < WAVES; ++t) gmax[hh] = fmaxf(gmax[hh], sh_m[hh][t]);
                mrun[hh] = gmax[hh];
            }
            __syncthreads();  // (sh_m is written again by the wave merge below)
        }
        // one step = the STRIDE keys of the workgroup; this lane: key s, dims 8*dl .. 8*dl+7
        auto step = [&](uint4 kv, uint4 vv, int s) {
            const bool ok = s < s_end;
            if ((ok ? s : s_last) == slot_new) {  // the row being appended by this launch: use the in-register copy
                kv = knew;
                vv = vnew;
            }
            const uint32_t vd[4] = {vv.x, vv.y, vv.z, vv.w};
            float vf[8];
#pragma unroll
            for (int jq = 0; jq < 4; ++jq) {
                vf[2 * jq] = bflo(vd[jq]);
                vf[2 * jq + 1] = bfhi(vd[jq]);
            }
#pragma unroll
            for (int hh = 0; hh < HQ; ++hh) {
                // q.k over this lane's 8 dims straight from the packed bf16 pairs, then over the LPR lanes of the key
                float p0 = dot2_bf16(kv.x, qp[hh][0], 0.f), p1 = dot2_bf16(kv.y, qp[hh][1], 0.f);
                p0 = dot2_bf16(kv.z, qp[hh][2], p0);
                p1 = dot2_bf16(kv.w, qp[hh][3], p1);
                const float sc_ = ok ? group_sum<LPR>(p0 + p1) * scale : -INFINITY;  // a masked key never raises the maximum
                if constexpr (PM) {
                    const float p = ok ? expf(sc_ - gmax[hh]) : 0.f;
                    const float pr = rbf(p);  // the probability as the reference's P.V product sees it
                    lrun[hh] += p;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[hh][e] = fmaf(pr, vf[e], acc[hh][e]);
                    continue;
                }
                const float mn = fmaxf(mrun[hh], sc_);
                const float corr = (mn == -INFINITY) ? 1.f : __expf(mrun[hh] - mn);
                const float p = (mn == -INFINITY) ? 0.f : __expf(sc_ - mn);
                lrun[hh] = lrun[hh] * corr + p;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[hh][e] = acc[hh][e] * corr + p * vf[e];
                mrun[hh] = mn;
            }
        };
        // two register sets in ping-pong; every load is unconditional (rows past the range are clamped and masked in
        // step()): loads behind run-time conditions cost the compiler its vmcnt bookkeeping
        uint4 k0 = kv_cur, v0 = vv_cur;
        for (int s0 = s_first; s0 < s_end; s0 += 2 * STRIDE) {
            const int sn1 = min(s0 + STRIDE + sub, s_last);
            const uint4 k1 = kc[(int64_t)sn1 * LPR + dl], v1 = vc[(int64_t)sn1 * LPR + dl];
            step(k0, v0, s0 + sub);
            const int sn2 = min(s0 + 2 * STRIDE + sub, s_last);
            k0 = kc[(int64_t)sn2 * LPR + dl];
            v0 = vc[(int64_t)sn2 * LPR + dl];
            if (s0 + STRIDE < s_end) step(k1, v1, s0 + STRIDE + sub);  // wave-uniform
        }
        attn_stamp(dbg, 2);
        // merge the RPW row slots of this wave: first the slots' common maximum, then every lane rescales its own state ONCE
        // and the rest is plain sums (the pairwise merge re-evaluated two exponentials per step and value); one state per
        // wave goes to LDS
#pragma unroll
        for (int hh = 0; hh < HQ; ++hh) {
            const float mw = slot_allreduce<LPR, true>(mrun[hh]);
            const float c = (mrun[hh] == -INFINITY) ? 0.f : __expf(mrun[hh] - mw);
            lrun[hh] = slot_allreduce<LPR, false>(lrun[hh] * c);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[hh][e] = slot_allreduce<LPR, false>(acc[hh][e] * c);
            mrun[hh] = mw;
            if (sub == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) sh_acc[hh][wave][dl * 8 + e] = acc[hh][e];
                if (dl == 0) {
                    sh_m[hh][wave] = mrun[hh];
                    sh_l[hh][wave] = lrun[hh];
                }
            }
        }
        if constexpr (AD) {
            if (nsplit == 1) adapter_prefix_heads<HS, HQ, PM>(aa, sh_q, g, h0, q_per_kv, adapter_lds<HQ * HS>());
        }
        __syncthreads();
        attn_stamp(dbg, 3);
        for (int idx = threadIdx.x; idx < HQ * HS; idx += WAVES * 64) {
            const int hh = idx / HS, d = idx % HS;
            if (h0 + hh < q_per_kv) {
                constexpr int NSLOT = WAVES;
                float mx = -INFINITY;
                for (int t = 0; t < NSLOT; ++t) mx = fmaxf(mx, sh_m[hh][t]);
                float l = 0.f, a = 0.f;
                for (int t = 0; t < NSLOT; ++t) {
                    const float mt = sh_m[hh][t];
                    const float wgt = (mt == -INFINITY) ? 0.f : __expf(mt - mx);
                    l += sh_l[hh][t] * wgt;
                    a += sh_acc[hh][t][d] * wgt;
                }
                const int head = g * q_per_kv + h0 + hh;
                if (nsplit == 1) {
                    if constexpr (AD)
                        y[(int64_t)head * HS + d] = adapter_combine(rbf(a / l), bf2f(aa.gate[head]), adapter_lds<HQ * HS>()[hh * HS + d]);
                    else
                        y[(int64_t)head * HS + d] = f2bf(a / l);
                } else {
                    float* p = ws + ((int64_t)head * nsplit + split) * (HS + 2);
                    store_agent(p + d, a);
                    if (d == 0) {
                        store_agent(p + HS, mx);
                        store_agent(p + HS + 1, l);
                    }
                }
            }
        }
    }
    attn_stamp(dbg, 4);
    if (nsplit == 1) return;
    // ---- arrival ticket: the last workgroup of this group merges the splits
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its write-through stores
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sh_last = (t == (unsigned int)(nsplit - 1));
        if (sh_last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
    }
    __syncthreads();
    if (!sh_last) return;
    if constexpr (AD) {
        adapter_prefix_heads<HS, HQ, PM>(aa, sh_q, g, h0, q_per_kv, adapter_lds<HQ * HS>());
        __syncthreads();
    }
    for (int idx = threadIdx.x; idx < HQ * HS; idx += WAVES * 64) {
        const int hq = h0 + idx / HS, d = idx % HS;
        if (hq >= q_per_kv) continue;
        const int head = g * q_per_kv + hq;
        const float* p = ws + (int64_t)head * nsplit * (HS + 2);
        float mx = -INFINITY;
        for (int t = 0; t < nsplit; ++t) mx = fmaxf(mx, load_agent(p + t * (HS + 2) + HS));
        float l = 0.f, a = 0.f;
        for (int t = 0; t < nsplit; ++t) {
            const float mt = load_agent(p + t * (HS + 2) + HS);
            const float wgt = (mt == -INFINITY) ? 0.f : __expf(mt - mx);
            l += load_agent(p + t * (HS + 2) + HS + 1) * wgt;
            a += load_agent(p + t * (HS + 2) + d) * wgt;
        }
        if constexpr (AD)
            y[(int64_t)head * HS + d] = adapter_combine(rbf(a / l), bf2f(aa.gate[head]), adapter_lds<HQ * HS>()[(idx / HS) * HS + d]);
        else
            y[(int64_t)head * HS + d] = f2bf(a / l);
    }
}

// ------------------------------------------------------------------------------------------ host: one fused decode call
// What a fused decode call consists of.  Every extern "C" entry point fills one, field by name, and names its kind;
// check_fused_call and the launch functions read nothing else.  What a kind does not have stays 0.
enum class FusedKind { OneRow, Rows, Seq, Prefix };  // Rows: B sequences of one row each; Seq: B consecutive rows of one sequence

struct FusedAttnCall {
    const void* qkv;
    int ldqkv, B;  // (one row: 0, 1)
    const void *rope_cos, *rope_sin;
    int n_elem;
    const int32_t* pos;
    int n_groups, q_per_kv, hs, S, nsplit;
    void *workspace, *tickets;
    int n_tickets;
    void *k_cache, *v_cache;
    int64_t kv_bstride;  // Rows only, else 0
    void* y;
    int ldy, softmax_mode;
    hipStream_t st;
    // Prefix only: the rows' own tails behind the shared cache
    const int32_t* prefix_len;
    void *k_tail, *v_tail;
    int S_tail, share_loads;
};

// The run-time to compile-time choices of the launches below, each written once: f receives std::integral_constant values.
template <int V>
using int_c = std::integral_constant<int, V>;

template <typename F>
static int with_head_size(const char* who, int hs, F&& f) {
    switch (hs) {
        case 32: return f(int_c<32>{});
        case 64: return f(int_c<64>{});
        case 128: return f(int_c<128>{});
        default: break;
    }
    set_error("%s: head size %d not built (32, 64, 128)", who, hs);
    return PARROT_EUNSUPPORTED;
}

// query heads of a group per pass over its K/V rows
template <typename F>
static int with_heads_per_pass(int q_per_kv, F&& f) {
    if (q_per_kv == 1) return f(int_c<1>{});
    if (q_per_kv == 2) return f(int_c<2>{});
    return f(int_c<4>{});
}

// f(waves, PM) of the fused kernels: "softmax_mode 1" always runs 16 waves; the default softmax runs 16 waves when a split holds
// more keys than kAttnWaves waves cover in two steps, else kAttnWaves
template <int HS, typename F>
static int with_waves(int S, int nsplit, int softmax_mode, F&& f) {
    const int per = (S + nsplit - 1) / nsplit;
    if (softmax_mode == 1) return f(int_c<16>{}, std::true_type{});
    if (per > 2 * kAttnWaves * (64 / (HS / 8))) return f(int_c<16>{}, std::false_type{});
    return f(int_c<kAttnWaves>{}, std::false_type{});
}

template <int HS, bool AD = false, bool ROWS = false, bool SEQ = false>
static int attn_fused_launch(const FusedAttnCall& c, AdapterAttnArgs aa = {}) {
    const int kid = SEQ ? K_ATTN_FUSED_SEQ : (ROWS ? K_ATTN_FUSED_ROWS : K_ATTN_FUSED);
    const AttnRowsArgs rows{c.ldqkv, c.ldy, c.kv_bstride};
    return with_heads_per_pass(c.q_per_kv, [&](auto hq) {
        return with_waves<HS>(c.S, c.nsplit, c.softmax_mode, [&](auto w, auto pm) {
            constexpr int HQ = decltype(hq)::value, W = decltype(w)::value;
            const dim3 grid(c.n_groups, c.nsplit, c.B * ((c.q_per_kv + HQ - 1) / HQ));
            return launch(kid, attn_fused_decode_kernel<HS, HQ, W, decltype(pm)::value, AD, ROWS, SEQ>, grid, dim3(W * 64), 0, c.st,
                          (const bf16_t*)c.qkv, (const __half*)c.rope_cos, (const __half*)c.rope_sin, c.n_elem, c.pos, (bf16_t*)c.k_cache,
                          (bf16_t*)c.v_cache, c.n_groups, c.q_per_kv, c.S, c.nsplit, (float*)c.workspace, (unsigned int*)c.tickets,
                          (bf16_t*)c.y, g_attn_dbg_host, aa, rows);
        });
    });
}

template <int HS>
static int attn_launch(const void* q, int M, const int32_t* pos, const void* k_cache, const void* v_cache, int n_groups,
                       int q_per_kv, int S, int nsplit, void* ws, void* y, int ldy, int softmax_mode, hipStream_t st) {
    const dim3 grid(n_groups, nsplit, M), block(kAttnWaves * 64);
    const int rc = with_heads_per_pass(q_per_kv, [&](auto hq) {
        auto go = [&](auto pm) {
            return launch(K_ATTN_DECODE, attn_decode_kernel<HS, decltype(hq)::value, decltype(pm)::value>, grid, block, 0, st, (const bf16_t*)q,
                          pos, (const bf16_t*)k_cache, (const bf16_t*)v_cache, n_groups, q_per_kv, S, nsplit, (float*)ws, (bf16_t*)y, ldy);
        };
        return softmax_mode == 1 ? go(std::true_type{}) : go(std::false_type{});
    });
    if (rc != PARROT_OK || nsplit == 1) return rc;
    return launch(K_ATTN_COMBINE, attn_combine_kernel<HS>, dim3(n_groups * q_per_kv, M), dim3(HS), 0, st, (const float*)ws,
                  nsplit, (bf16_t*)y, ldy, n_groups * q_per_kv);
}

// ------------------------------------------------------------------------------------------ candidates: one shared prompt cache
// parrot_attn_fused_decode_prefix: B rows continue ONE prompt of T tokens.  The logical window of row b, slots 0 .. pos[b], is the
// shared cache (slots < T, written once by the prompt) followed by the row's own tail (slot s >= T at tail[b][s - T]); the new K/V
// row goes to the tail.  The split geometry is the rows kernel's for (S, nsplit) - per, the 16-wave decision, the partial-state
// layout, the tickets, the reducer's order - and the key loop, the slot / wave merges and the reducer below are the statements of
// attn_fused_decode_kernel, so every partial state and every y is the one parrot_attn_fused_decode_rows computes on B full caches
// that each hold a copy of the prompt (tests/test_candidates_gpu.py compares the bits).  It is a kernel of its own and not two more
// template switches of attn_fused_decode_kernel: with them the existing instantiations changed registers and occupancy.
// Two launches per layer:
//   KIND 2, first, only when q_per_kv <= 2, nsplit > 1 and B > 1: a workgroup takes the 4 / q_per_kv rows of one row block as
//     "virtual query heads" of the group (HQ = 4) for a split with s_begin + per <= T, whose keys are the same for every row: it
//     ropes row b's q at pos[b], loads each K/V row once, keeps one softmax state per (row, head), writes the rows' partial states
//     and arrives once at each row's ticket.  Workgroups of other splits exit at once.  It never merges: the last split ends at
//     S > pos[b] >= T and is never shared, so no ticket reaches nsplit here.
//   KIND 1, second: the batched kernel's workgroup with the address translation.  Workgroups of the splits the first launch served
//     exit without an arrival, so every ticket counts exactly nsplit arrivals and the last arriver of this launch merges.
// T is clamped to [0, S], pos to [0, S-1] and the tail index to [0, S_tail-1]: no address leaves the buffers whatever they hold.
struct AttnPrefixArgs {
    int ldqkv, ldy;
    bf16_t* k_tail;             // [B][n_groups][S_tail][hs]
    bf16_t* v_tail;
    const int32_t* prefix_len;  // T, on the device: one captured launch serves every prompt length
    int S_tail, B, share;       // share: splits entirely below T belong to the KIND 2 launch
};

template <int HS, int HQ, int WAVES, bool PM, int KIND>
__global__ void __launch_bounds__(WAVES * 64)
attn_prefix_decode_kernel(const bf16_t* __restrict__ qkv, const __half* __restrict__ rope_cos, const __half* __restrict__ rope_sin,
                          int n_elem, const int32_t* __restrict__ pos_ptr, const bf16_t* __restrict__ k_cache,
                          const bf16_t* __restrict__ v_cache, int n_groups, int q_per_kv, int S, int nsplit, float* __restrict__ ws,
                          unsigned int* __restrict__ tickets, bf16_t* __restrict__ y, AttnPrefixArgs pa) {
    constexpr int LPR = HS / 8;
    constexpr int RPW = 64 / LPR;
    constexpr int STRIDE = WAVES * RPW;
    constexpr int NQ = KIND == 2 ? HQ : kFusedMaxQ;  // roped q rows held in LDS
    __shared__ float sh_acc[HQ][WAVES][HS];  // one merged state per wave
    __shared__ float sh_m[HQ][WAVES], sh_l[HQ][WAVES];
    __shared__ __attribute__((aligned(16))) bf16_t sh_q[NQ][HS];
    __shared__ __attribute__((aligned(16))) bf16_t sh_kv[2][HS];  // roped k_new, v_new as stored in the tail (KIND 1)
    __shared__ int sh_last;

    const int n_head = n_groups * q_per_kv;
    const int g = blockIdx.x, split = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, dl = lane % LPR;
    // KIND 1: blockIdx.z = row * nchunk + chunk of the group's query heads, as in the batched kernel
    // KIND 2: blockIdx.z = block of R rows; virtual head t is query head t % q_per_kv of row rb * R + t / q_per_kv (one chunk)
    const int nchunk = (q_per_kv + HQ - 1) / HQ;
    const int b = KIND == 1 ? blockIdx.z / nchunk : 0;
    const int chunk = KIND == 1 ? blockIdx.z - b * nchunk : 0;
    const int rb = blockIdx.z, R = HQ / q_per_kv;
    const int h0 = chunk * HQ;
    const int T = min(max(pa.prefix_len[0], 0), S);
    const int per = (S + nsplit - 1) / nsplit;
    const int s_begin = split * per;
    // every key of the split is a prompt key, the same for all rows (never the last split)
    const bool shared = split < nsplit - 1 && s_begin + per <= T;
    if (KIND == 2 ? !shared : (shared && pa.share != 0)) return;  // the other launch's split (workgroup-uniform, before any barrier)

    const int pos = min(max(pos_ptr[b], 0), S - 1);
    const int n_valid = pos + 1;
    const int slot_new = KIND == 2 ? -1 : pos;  // (a shared split never holds a row's new slot)
    const int s_end = KIND == 2 ? s_begin + per : min(n_valid, s_begin + per);
    const float scale = 1.0f / sqrtf((float)HS);
    const int half_n = n_elem >> 1;
    const int tail_new = min(max(pos - T, 0), pa.S_tail - 1);  // KIND 1: where the new K/V row goes

    const uint4* kc = reinterpret_cast<const uint4*>(k_cache + (int64_t)g * S * HS);
    const uint4* vc = reinterpret_cast<const uint4*>(v_cache + (int64_t)g * S * HS);
    const int64_t toff = ((int64_t)b * n_groups + g) * pa.S_tail * HS;
    const uint4* kt = reinterpret_cast<const uint4*>(pa.k_tail + toff);
    const uint4* vt = reinterpret_cast<const uint4*>(pa.v_tail + toff);
    // this lane's 16 bytes of the K / V row of logical slot s: the base is picked per key, the load itself stays unconditional
    auto ldk = [&](int s) -> uint4 {
        if constexpr (KIND == 2) {
            return kc[(int64_t)s * LPR + dl];
        } else {
            const bool low = s < T;
            return (low ? kc : kt)[(int64_t)(low ? s : min(s - T, pa.S_tail - 1)) * LPR + dl];
        }
    };
    auto ldv = [&](int s) -> uint4 {
        if constexpr (KIND == 2) {
            return vc[(int64_t)s * LPR + dl];
        } else {
            const bool low = s < T;
            return (low ? vc : vt)[(int64_t)(low ? s : min(s - T, pa.S_tail - 1)) * LPR + dl];
        }
    };

    // ---- load order as in attn_fused_decode_kernel: the RoPE operands, then this wave's first K/V rows, then the RoPE arithmetic
    // (x*cos + rotate_half(x)*sin, each product and the sum rounded to fp32 separately; cos = 1, sin = 0 outside the rotary part)
    constexpr int ROPE_IT = ((KIND == 2 ? HQ : kFusedMaxQ + 2) * HS + WAVES * 64 - 1) / (WAVES * 64);
    const bf16_t* grp = qkv + (int64_t)b * pa.ldqkv + (int64_t)g * (q_per_kv + 2) * HS;
    const int n_rope_elems = KIND == 2 ? HQ * HS : (q_per_kv + 2) * HS;  // KIND 2: the query heads of the R rows, no k / v
    float rx[ROPE_IT], ro[ROPE_IT], rc[ROPE_IT], rs[ROPE_IT];
#pragma unroll
    for (int it = 0; it < ROPE_IT; ++it) {
        const int idx = threadIdx.x + it * WAVES * 64;
        rx[it] = ro[it] = rs[it] = 0.f;
        rc[it] = 1.f;
        if (idx < n_rope_elems) {
            const int t = idx / HS, d = idx % HS;
            const bf16_t* src = grp + idx;
            int rpos = pos;
            bool rotary = t <= q_per_kv;
            if constexpr (KIND == 2) {
                const int row = min(rb * R + t / q_per_kv, pa.B - 1);  // (a ragged block ropes the last row again and drops it)
                src = grp + (int64_t)row * pa.ldqkv + (t % q_per_kv) * HS + d;
                rpos = min(max(pos_ptr[row], 0), S - 1);
                rotary = true;
            }
            rx[it] = bf2f(src[0]);
            if (rotary && d < n_elem) {
                rc[it] = __half2float(rope_cos[(int64_t)rpos * n_elem + d]);
                rs[it] = __half2float(rope_sin[(int64_t)rpos * n_elem + d]);
                ro[it] = d < half_n ? -bf2f(src[half_n]) : bf2f(src[-half_n]);
            }
        }
    }
    const int s_first = s_begin + wave * RPW;
    const int s_last = max(s_end - 1, 0);
    const int sc_first = min(s_first + sub, s_last);
    const uint4 kv_cur = ldk(sc_first);
    const uint4 vv_cur = ldv(sc_first);
#pragma unroll
    for (int it = 0; it < ROPE_IT; ++it) {
        const int idx = threadIdx.x + it * WAVES * 64;
        if (idx < n_rope_elems) {
            const int t = idx / HS, d = idx % HS;
            const float v = __fadd_rn(__fmul_rn(rx[it], rc[it]), __fmul_rn(ro[it], rs[it]));
            const bf16_t vb = f2bf(v);
            if (KIND == 2 || t < q_per_kv)
                sh_q[t][d] = vb;
            else
                sh_kv[t - q_per_kv][d] = vb;
        }
    }
    __syncthreads();
    uint4 knew = kv_cur, vnew = vv_cur;  // (KIND 2: never used)
    if constexpr (KIND == 1) {
        // ---- KV append to the row's tail by the workgroup that owns the new slot
        if (chunk == 0 && slot_new >= s_begin && slot_new < s_begin + per && threadIdx.x < 2 * LPR) {
            const int which = threadIdx.x / LPR, c = threadIdx.x % LPR;
            bf16_t* dst = (which ? pa.v_tail : pa.k_tail) + toff + (int64_t)tail_new * HS;
            reinterpret_cast<uint4*>(dst)[c] = reinterpret_cast<const uint4*>(sh_kv[which])[c];
        }
        knew = reinterpret_cast<const uint4*>(sh_kv[0])[dl];
        vnew = reinterpret_cast<const uint4*>(sh_kv[1])[dl];
    }

    {
        uint32_t qp[HQ][4];  // this lane's 8 dims of every query head, packed bf16 pairs (operand of v_dot2_f32_bf16)
        float mrun[HQ], lrun[HQ], acc[HQ][8];
#pragma unroll
        for (int hh = 0; hh < HQ; ++hh) {
            const int hq = KIND == 2 ? hh : min(h0 + hh, q_per_kv - 1);
            const uint4 qv = reinterpret_cast<const uint4*>(sh_q[hq])[dl];
            qp[hh][0] = qv.x;
            qp[hh][1] = qv.y;
            qp[hh][2] = qv.z;
            qp[hh][3] = qv.w;
            mrun[hh] = -INFINITY;
            lrun[hh] = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[hh][e] = 0.f;
        }
        float gmax[HQ];  // PM: the maximum score over all the keys of this head
        if constexpr (PM) {
#pragma unroll
            for (int hh = 0; hh < HQ; ++hh) gmax[hh] = -INFINITY;
            for (int s0 = s_first; s0 < s_end; s0 += STRIDE) {
                const int sk = min(s0 + sub, s_last);
                uint4 kv = ldk(sk);
                if (sk == slot_new) kv = knew;  // the row being appended by this launch
#pragma unroll
                for (int hh = 0; hh < HQ; ++hh) {
                    float p0 = dot2_bf16(kv.x, qp[hh][0], 0.f), p1 = dot2_bf16(kv.y, qp[hh][1], 0.f);
                    p0 = dot2_bf16(kv.z, qp[hh][2], p0);
                    p1 = dot2_bf16(kv.w, qp[hh][3], p1);
                    const float sc_ = group_sum<LPR>(p0 + p1) * scale;
                    if (s0 + sub < s_end) gmax[hh] = fmaxf(gmax[hh], sc_);
                }
            }
#pragma unroll
            for (int hh = 0; hh < HQ; ++hh) {
                gmax[hh] = slot_allreduce<LPR, true>(gmax[hh]);
                if (lane == 0) sh_m[hh][wave] = gmax[hh];
            }
            __syncthreads();
#pragma unroll
            for (int hh = 0; hh < HQ; ++hh) {
                for (int t = 0; t < WAVES; ++t) gmax[hh] = fmaxf(gmax[hh], sh_m[hh][t]);
                mrun[hh] = gmax[hh];
            }
            __syncthreads();  // (sh_m is written again by the wave merge below)
        }
        // one step = the STRIDE keys of the workgroup; this lane: key s, dims 8*dl .. 8*dl+7
        auto step = [&](uint4 kv, uint4 vv, int s) {
            const bool ok = s < s_end;
            if ((ok ? s : s_last) == slot_new) {  // the row being appended by this launch: use the in-register copy
                kv = knew;
                vv = vnew;
            }
            const uint32_t vd[4] = {vv.x, vv.y, vv.z, vv.w};
            float vf[8];
#pragma unroll
            for (int jq = 0; jq < 4; ++jq) {
                vf[2 * jq] = bflo(vd[jq]);
                vf[2 * jq + 1] = bfhi(vd[jq]);
            }
#pragma unroll
            for (int hh = 0; hh < HQ; ++hh) {
                float p0 = dot2_bf16(kv.x, qp[hh][0], 0.f), p1 = dot2_bf16(kv.y, qp[hh][1], 0.f);
                p0 = dot2_bf16(kv.z, qp[hh][2], p0);
                p1 = dot2_bf16(kv.w, qp[hh][3], p1);
                const float sc_ = ok ? group_sum<LPR>(p0 + p1) * scale : -INFINITY;  // a masked key never raises the maximum
                if constexpr (PM) {
                    const float p = ok ? expf(sc_ - gmax[hh]) : 0.f;
                    const float pr = rbf(p);  // the probability as the reference's P.V product sees it
                    lrun[hh] += p;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[hh][e] = fmaf(pr, vf[e], acc[hh][e]);
                    continue;
                }
                const float mn = fmaxf(mrun[hh], sc_);
                const float corr = (mn == -INFINITY) ? 1.f : __expf(mrun[hh] - mn);
                const float p = (mn == -INFINITY) ? 0.f : __expf(sc_ - mn);
                lrun[hh] = lrun[hh] * corr + p;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[hh][e] = acc[hh][e] * corr + p * vf[e];
                mrun[hh] = mn;
            }
        };
        // two register sets in ping-pong; every load is unconditional (rows past the range are clamped and masked in step())
        uint4 k0 = kv_cur, v0 = vv_cur;
        for (int s0 = s_first; s0 < s_end; s0 += 2 * STRIDE) {
            const int sn1 = min(s0 + STRIDE + sub, s_last);
            const uint4 k1 = ldk(sn1), v1 = ldv(sn1);
            step(k0, v0, s0 + sub);
            const int sn2 = min(s0 + 2 * STRIDE + sub, s_last);
            k0 = ldk(sn2);
            v0 = ldv(sn2);
            if (s0 + STRIDE < s_end) step(k1, v1, s0 + STRIDE + sub);  // wave-uniform
        }
        // merge the RPW row slots of this wave, one state per wave to LDS
#pragma unroll
        for (int hh = 0; hh < HQ; ++hh) {
            const float mw = slot_allreduce<LPR, true>(mrun[hh]);
            const float c = (mrun[hh] == -INFINITY) ? 0.f : __expf(mrun[hh] - mw);
            lrun[hh] = slot_allreduce<LPR, false>(lrun[hh] * c);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[hh][e] = slot_allreduce<LPR, false>(acc[hh][e] * c);
            mrun[hh] = mw;
            if (sub == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) sh_acc[hh][wave][dl * 8 + e] = acc[hh][e];
                if (dl == 0) {
                    sh_m[hh][wave] = mrun[hh];
                    sh_l[hh][wave] = lrun[hh];
                }
            }
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < HQ * HS; idx += WAVES * 64) {
            const int hh = idx / HS, d = idx % HS;
            const int row = KIND == 2 ? rb * R + hh / q_per_kv : b;  // KIND 2: the row of virtual head hh
            if (KIND == 2 ? row < pa.B : h0 + hh < q_per_kv) {
                constexpr int NSLOT = WAVES;
                float mx = -INFINITY;
                for (int t = 0; t < NSLOT; ++t) mx = fmaxf(mx, sh_m[hh][t]);
                float l = 0.f, a = 0.f;
                for (int t = 0; t < NSLOT; ++t) {
                    const float mt = sh_m[hh][t];
                    const float wgt = (mt == -INFINITY) ? 0.f : __expf(mt - mx);
                    l += sh_l[hh][t] * wgt;
                    a += sh_acc[hh][t][d] * wgt;
                }
                const int head = g * q_per_kv + (KIND == 2 ? hh % q_per_kv : h0 + hh);
                if (nsplit == 1) {
                    y[(int64_t)row * pa.ldy + (int64_t)head * HS + d] = f2bf(a / l);
                } else {
                    float* p = ws + (((int64_t)row * n_head + head) * nsplit + split) * (HS + 2);
                    store_agent(p + d, a);
                    if (d == 0) {
                        store_agent(p + HS, mx);
                        store_agent(p + HS + 1, l);
                    }
                }
            }
        }
    }
    if (nsplit == 1) return;
    // ---- arrival tickets (they only count; nobody waits): the last workgroup of a (row, group, chunk) merges the splits
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its write-through stores
    __syncthreads();
    if constexpr (KIND == 2) {  // one arrival per served row; the merge is the per-row launch's
        if ((int)threadIdx.x < R && rb * R + (int)threadIdx.x < pa.B)
            __hip_atomic_fetch_add(&tickets[(rb * R + threadIdx.x) * n_head + g], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    unsigned int* ticket = &tickets[b * n_head + g * nchunk + chunk];
    if (threadIdx.x == 0) {
        const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sh_last = (t == (unsigned int)(nsplit - 1));
        if (sh_last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
    }
    __syncthreads();
    if (!sh_last) return;
    for (int idx = threadIdx.x; idx < HQ * HS; idx += WAVES * 64) {
        const int hq = h0 + idx / HS, d = idx % HS;
        if (hq >= q_per_kv) continue;
        const int head = g * q_per_kv + hq;
        const float* p = ws + ((int64_t)b * n_head + head) * nsplit * (HS + 2);
        float mx = -INFINITY;
        for (int t = 0; t < nsplit; ++t) mx = fmaxf(mx, load_agent(p + t * (HS + 2) + HS));
        float l = 0.f, a = 0.f;
        for (int t = 0; t < nsplit; ++t) {
            const float mt = load_agent(p + t * (HS + 2) + HS);
            const float wgt = (mt == -INFINITY) ? 0.f : __expf(mt - mx);
            l += load_agent(p + t * (HS + 2) + HS + 1) * wgt;
            a += load_agent(p + t * (HS + 2) + d) * wgt;
        }
        y[(int64_t)b * pa.ldy + (int64_t)head * HS + d] = f2bf(a / l);
    }
}

// both launches of one layer (see above); the per-row launch always runs
template <int HS>
static int attn_prefix_launch(const FusedAttnCall& c) {
    AttnPrefixArgs pa{c.ldqkv, c.ldy, (bf16_t*)c.k_tail, (bf16_t*)c.v_tail, c.prefix_len, c.S_tail, c.B, c.share_loads};
    pa.share = pa.share != 0 && c.nsplit > 1 && c.q_per_kv <= 2 && c.B > 1;
    auto go = [&](auto hq, auto w, auto pm, auto kind, dim3 grid) {
        constexpr int W = decltype(w)::value;
        return launch(K_ATTN_FUSED_PREFIX, attn_prefix_decode_kernel<HS, decltype(hq)::value, W, decltype(pm)::value, decltype(kind)::value>,
                      grid, dim3(W * 64), 0, c.st, (const bf16_t*)c.qkv, (const __half*)c.rope_cos, (const __half*)c.rope_sin, c.n_elem, c.pos,
                      (const bf16_t*)c.k_cache, (const bf16_t*)c.v_cache, c.n_groups, c.q_per_kv, c.S, c.nsplit, (float*)c.workspace,
                      (unsigned int*)c.tickets, (bf16_t*)c.y, pa);
    };
    if (pa.share) {  // KIND 2 is built for HQ = 4 and the default softmax only; its waves are the rows kernel's decision
        const int R = 4 / c.q_per_kv;
        const dim3 grid2(c.n_groups, c.nsplit - 1, (c.B + R - 1) / R);  // (the last split is never shared)
        const int rc = with_waves<HS>(c.S, c.nsplit, 0, [&](auto w, auto) { return go(int_c<4>{}, w, std::false_type{}, int_c<2>{}, grid2); });
        if (rc != PARROT_OK) return rc;
    }
    return with_heads_per_pass(c.q_per_kv, [&](auto hq) {
        const dim3 grid(c.n_groups, c.nsplit, c.B * ((c.q_per_kv + decltype(hq)::value - 1) / decltype(hq)::value));
        return with_waves<HS>(c.S, c.nsplit, c.softmax_mode, [&](auto w, auto pm) { return go(hq, w, pm, int_c<1>{}, grid); });
    });
}

// softmax_mode 1 needs the whole window in one key block of the reference's kernel: one split, at most 512 slots
static int check_softmax_mode(const char* who, int softmax_mode, int S, int nsplit) {
    PARROT_REQUIRE(softmax_mode == 0 || softmax_mode == 1, "%s: softmax_mode must be 0 or 1", who);
    PARROT_UNSUPPORTED(softmax_mode == 0 || (nsplit == 1 && S <= 512),
                       "%s: softmax_mode 1 (the reference's bf16 probabilities) is built for one split and windows up to 512 slots (S=%d nsplit=%d)", who, S, nsplit);
    return PARROT_OK;
}

// every condition of a fused decode call, once and in one order; `who` names the entry point in the messages (the head size is
// refused by with_head_size)
static int check_fused_call(const char* who, const FusedAttnCall& c, FusedKind kind) {
    const bool rows = kind != FusedKind::OneRow, prefix = kind == FusedKind::Prefix;
    PARROT_REQUIRE(!rows || (c.B >= 1 && c.B <= kMaxDecodeRows), "%s: B=%d (1 .. %d)", who, c.B, kMaxDecodeRows);
    {
        const int rc = check_softmax_mode(who, c.softmax_mode, c.S, c.nsplit);
        if (rc != PARROT_OK) return rc;
    }
    PARROT_REQUIRE(c.qkv && c.pos && c.k_cache && c.v_cache && c.y && (!prefix || (c.prefix_len && c.k_tail && c.v_tail)), "%s: null pointer", who);
    const bool shape_ok = c.n_groups >= 1 && c.q_per_kv >= 1 && c.S >= 1;
    if (prefix) PARROT_REQUIRE(shape_ok && c.S_tail >= 1, "%s: bad shape (S=%d S_tail=%d)", who, c.S, c.S_tail);
    PARROT_REQUIRE(shape_ok, "%s: bad shape", who);
    PARROT_UNSUPPORTED(c.q_per_kv <= kFusedMaxQ, "%s: at most %d query heads per group (got %d)", who, kFusedMaxQ, c.q_per_kv);
    PARROT_REQUIRE(c.n_elem % 2 == 0 && c.n_elem >= 0 && c.n_elem <= c.hs, "%s: bad n_elem=%d", who, c.n_elem);
    PARROT_REQUIRE(c.n_elem == 0 || (c.rope_cos && c.rope_sin), "%s: rope tables missing", who);
    PARROT_REQUIRE(c.nsplit >= 1 && c.nsplit <= 65535, "%s: nsplit out of range", who);
    PARROT_REQUIRE(c.nsplit == 1 || (c.workspace && c.tickets), "%s: workspace and tickets required when nsplit > 1", who);
    if (rows) {
        const int n_head = c.n_groups * c.q_per_kv;
        PARROT_REQUIRE(!c.tickets || c.n_tickets >= c.B * n_head, "%s: %d tickets, B * n_head = %d needed", who, c.n_tickets, c.B * n_head);
        PARROT_REQUIRE(c.ldqkv >= c.n_groups * (c.q_per_kv + 2) * c.hs && c.ldqkv % 8 == 0, "%s: ldqkv=%d too small or not a multiple of 8", who, c.ldqkv);
        PARROT_REQUIRE(c.ldy >= n_head * c.hs, "%s: ldy=%d too small", who, c.ldy);
    }
    PARROT_REQUIRE(kind != FusedKind::Rows || (c.kv_bstride >= (int64_t)c.n_groups * c.S * c.hs && c.kv_bstride % 8 == 0),
                   "%s: kv_bstride=%lld below n_groups * S * hs or not a multiple of 8", who, (long long)c.kv_bstride);
    PARROT_REQUIRE(kind != FusedKind::Seq || c.B <= c.S, "%s: M=%d rows do not fit a cache of %d slots", who, c.B, c.S);
    PARROT_REQUIRE(aligned16(c.qkv) && aligned16(c.k_cache) && aligned16(c.v_cache) && (!prefix || (aligned16(c.k_tail) && aligned16(c.v_tail))),
                   "%s: 16-byte alignment", who);
    return PARROT_OK;
}

// check, then the launch of the kind; `aa`: the one-row call of an adapter layer
static int fused_attn_call(const char* who, const FusedAttnCall& c, FusedKind kind, const AdapterAttnArgs* aa = nullptr) {
    const int rc = check_fused_call(who, c, kind);
    if (rc != PARROT_OK) return rc;
    return with_head_size(who, c.hs, [&](auto hs) {
        constexpr int HS = decltype(hs)::value;
        switch (kind) {
            case FusedKind::OneRow: return aa ? attn_fused_launch<HS, true>(c, *aa) : attn_fused_launch<HS>(c);
            case FusedKind::Rows: return attn_fused_launch<HS, false, true>(c);
            case FusedKind::Seq: return attn_fused_launch<HS, false, true, true>(c);
            default: return attn_prefix_launch<HS>(c);
        }
    });
}

// the one-row call of both one-row entry points (`aa`: an adapter layer's): one row, no row strides, n_head tickets
static int one_row_call(const void* qkv, const void* rope_cos, const void* rope_sin, int n_elem, const int32_t* pos, int n_groups,
                        int q_per_kv, int hs, int S, int nsplit, void* workspace, void* tickets, void* k_cache, void* v_cache, void* y,
                        int softmax_mode, void* stream, const AdapterAttnArgs* aa) {
    FusedAttnCall c{};
    c.qkv = qkv, c.B = 1, c.rope_cos = rope_cos, c.rope_sin = rope_sin, c.n_elem = n_elem, c.pos = pos;
    c.n_groups = n_groups, c.q_per_kv = q_per_kv, c.hs = hs, c.S = S, c.nsplit = nsplit;
    c.workspace = workspace, c.tickets = tickets, c.k_cache = k_cache, c.v_cache = v_cache, c.y = y;
    c.softmax_mode = softmax_mode, c.st = (hipStream_t)stream;
    return fused_attn_call("attn_fused_decode", c, FusedKind::OneRow, aa);
}

// prefix K/V, gate and aT of the two adapter entry points
static int check_adapter_attn(const char* who, const void* ak, const void* av, const void* gate, int aT, int n_groups, int q_per_kv,
                              int hs, AdapterAttnArgs* aa) {
    PARROT_REQUIRE(ak && av && gate, "%s: null adapter pointer", who);
    PARROT_REQUIRE(n_groups >= 1 && q_per_kv >= 1 && aT >= 1, "%s: bad shape n_groups=%d q_per_kv=%d aT=%d", who, n_groups, q_per_kv, aT);
    PARROT_UNSUPPORTED(aT <= kAdapterMaxT, "%s: adapter_prompt_length %d > %d is not built (one prefix key per lane)", who, aT, kAdapterMaxT);
    PARROT_UNSUPPORTED(hs == 32 || hs == 64 || hs == 128, "%s: head size %d not built (32, 64, 128)", who, hs);
    PARROT_REQUIRE(aligned16(ak) && aligned16(av) && (reinterpret_cast<uintptr_t>(gate) & 1u) == 0, "%s: ak / av must be 16-byte aligned", who);
    *aa = AdapterAttnArgs{(const bf16_t*)ak, (const bf16_t*)av, (const bf16_t*)gate, aT};
    return PARROT_OK;
}

}  // namespace parrot

using namespace parrot;

extern "C" {

int parrot_qkv_rope_kvappend(const void* qkv, int ldqkv, int M, const void* rope_cos, const void* rope_sin, int n_elem,
                             int rope_local, const int32_t* pos, int n_groups, int q_per_kv, int hs, int S, void* q_out, void* k_cache,
                             void* v_cache, void* stream) {
    PARROT_REQUIRE(qkv && pos && q_out && k_cache && v_cache, "qkv_rope_kvappend: null pointer");
    PARROT_REQUIRE(M >= 1 && n_groups >= 1 && q_per_kv >= 1 && hs >= 2 && S >= 1, "qkv_rope_kvappend: bad shape");
    PARROT_REQUIRE(hs % 2 == 0 && n_elem % 2 == 0 && n_elem >= 0 && n_elem <= hs,
                   "qkv_rope_kvappend: hs=%d and n_elem=%d must be even, n_elem <= hs", hs, n_elem);
    PARROT_REQUIRE(n_elem == 0 || (rope_cos && rope_sin), "qkv_rope_kvappend: rope tables missing");
    PARROT_REQUIRE(ldqkv >= n_groups * (q_per_kv + 2) * hs, "qkv_rope_kvappend: ldqkv too small");
    PARROT_REQUIRE(M <= S, "qkv_rope_kvappend: M=%d rows do not fit a cache of %d slots", M, S);
    const bool tables_ok = n_elem == 0 || (aligned16(rope_cos) && aligned16(rope_sin));
    if (hs % 8 == 0 && n_elem % 16 == 0 && ldqkv % 8 == 0 && aligned16(qkv) && aligned16(q_out) && aligned16(k_cache) && aligned16(v_cache) &&
        tables_ok && M <= 65535) {
        const unsigned per_row = (unsigned)(n_groups * (q_per_kv + 2) * (hs / 8));
        return launch(K_ROPE_KVAPPEND, rope_kvappend8_kernel, dim3((per_row + 255) / 256, (unsigned)M), dim3(256), 0, (hipStream_t)stream,
                      (const bf16_t*)qkv, ldqkv, M, (const __half*)rope_cos, (const __half*)rope_sin, n_elem, rope_local, pos, n_groups, q_per_kv,
                      hs, S, (bf16_t*)q_out, (bf16_t*)k_cache, (bf16_t*)v_cache);
    }
    const int64_t total = (int64_t)M * n_groups * (q_per_kv + 2) * (hs / 2);
    return launch(K_ROPE_KVAPPEND, rope_kvappend_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                  (hipStream_t)stream, (const bf16_t*)qkv, ldqkv, M, (const __half*)rope_cos, (const __half*)rope_sin,
                  n_elem, rope_local, pos, n_groups, q_per_kv, hs, S, (bf16_t*)q_out, (bf16_t*)k_cache, (bf16_t*)v_cache);
}

#ifdef PARROT_DIAG
int parrot_tune_attn_stamps(void* dbg8_u64) {  // diagnostic build: device buffer of 8 uint64, or NULL to switch off
    g_attn_dbg_host = (unsigned long long*)dbg8_u64;
    return PARROT_OK;
}
#endif

int parrot_attn_fused_decode(const void* qkv, const void* rope_cos, const void* rope_sin, int n_elem, const int32_t* pos,
                             int n_groups, int q_per_kv, int hs, int S, int nsplit, void* workspace, void* tickets,
                             void* k_cache, void* v_cache, void* y, int softmax_mode, void* stream) {
    return one_row_call(qkv, rope_cos, rope_sin, n_elem, pos, n_groups, q_per_kv, hs, S, nsplit, workspace, tickets, k_cache, v_cache, y,
                        softmax_mode, stream, nullptr);
}

// (the one-row call behind the adapter's own checks: what both share is reported under the one-row name)
int parrot_attn_fused_decode_adapter(const void* qkv, const void* rope_cos, const void* rope_sin, int n_elem, const int32_t* pos,
                                     int n_groups, int q_per_kv, int hs, int S, int nsplit, void* workspace, void* tickets,
                                     void* k_cache, void* v_cache, void* y, const void* ak, const void* av, const void* gate, int aT,
                                     int softmax_mode, void* stream) {
    AdapterAttnArgs aa;
    const int rc = check_adapter_attn("attn_fused_decode_adapter", ak, av, gate, aT, n_groups, q_per_kv, hs, &aa);
    if (rc != PARROT_OK) return rc;
    return one_row_call(qkv, rope_cos, rope_sin, n_elem, pos, n_groups, q_per_kv, hs, S, nsplit, workspace, tickets, k_cache, v_cache, y,
                        softmax_mode, stream, &aa);
}

int parrot_attn_fused_decode_rows(const void* qkv, int ldqkv, int B, const void* rope_cos, const void* rope_sin, int n_elem,
                                  const int32_t* pos, int n_groups, int q_per_kv, int hs, int S, int nsplit, void* workspace,
                                  void* tickets, int n_tickets, void* k_cache, void* v_cache, int64_t kv_bstride, void* y, int ldy,
                                  int softmax_mode, void* stream) {
    FusedAttnCall c{};
    c.qkv = qkv, c.ldqkv = ldqkv, c.B = B, c.rope_cos = rope_cos, c.rope_sin = rope_sin, c.n_elem = n_elem, c.pos = pos;
    c.n_groups = n_groups, c.q_per_kv = q_per_kv, c.hs = hs, c.S = S, c.nsplit = nsplit;
    c.workspace = workspace, c.tickets = tickets, c.n_tickets = n_tickets, c.k_cache = k_cache, c.v_cache = v_cache;
    c.y = y, c.ldy = ldy, c.softmax_mode = softmax_mode, c.st = (hipStream_t)stream;
    c.kv_bstride = kv_bstride;
    return fused_attn_call("attn_fused_decode_rows", c, FusedKind::Rows);
}

int parrot_attn_fused_decode_seq(const void* qkv, int ldqkv, int M, const void* rope_cos, const void* rope_sin, int n_elem,
                                 const int32_t* pos, int n_groups, int q_per_kv, int hs, int S, int nsplit, void* workspace,
                                 void* tickets, int n_tickets, void* k_cache, void* v_cache, void* y, int ldy, int softmax_mode,
                                 void* stream) {
    FusedAttnCall c{};
    c.qkv = qkv, c.ldqkv = ldqkv, c.B = M, c.rope_cos = rope_cos, c.rope_sin = rope_sin, c.n_elem = n_elem, c.pos = pos;
    c.n_groups = n_groups, c.q_per_kv = q_per_kv, c.hs = hs, c.S = S, c.nsplit = nsplit;
    c.workspace = workspace, c.tickets = tickets, c.n_tickets = n_tickets, c.k_cache = k_cache, c.v_cache = v_cache;
    c.y = y, c.ldy = ldy, c.softmax_mode = softmax_mode, c.st = (hipStream_t)stream;
    return fused_attn_call("attn_fused_decode_seq", c, FusedKind::Seq);
}

int parrot_attn_fused_decode_prefix(const void* qkv, int ldqkv, int B, const void* rope_cos, const void* rope_sin, int n_elem,
                                    const int32_t* pos, const int32_t* prefix_len, int n_groups, int q_per_kv, int hs, int S, int nsplit,
                                    void* workspace, void* tickets, int n_tickets, const void* k_cache, const void* v_cache, void* k_tail,
                                    void* v_tail, int S_tail, void* y, int ldy, int share_loads, int softmax_mode, void* stream) {
    FusedAttnCall c{};
    c.qkv = qkv, c.ldqkv = ldqkv, c.B = B, c.rope_cos = rope_cos, c.rope_sin = rope_sin, c.n_elem = n_elem, c.pos = pos;
    c.n_groups = n_groups, c.q_per_kv = q_per_kv, c.hs = hs, c.S = S, c.nsplit = nsplit;
    c.workspace = workspace, c.tickets = tickets, c.n_tickets = n_tickets, c.k_cache = const_cast<void*>(k_cache), c.v_cache = const_cast<void*>(v_cache);
    c.y = y, c.ldy = ldy, c.softmax_mode = softmax_mode, c.st = (hipStream_t)stream;
    // (the shared cache is only read: attn_prefix_decode_kernel takes it as const)
    c.prefix_len = prefix_len, c.k_tail = k_tail, c.v_tail = v_tail, c.S_tail = S_tail, c.share_loads = share_loads;
    return fused_attn_call("attn_fused_decode_prefix", c, FusedKind::Prefix);
}

int parrot_attn_adapter_prefix(const void* q, int M, const void* ak, const void* av, const void* gate, int aT, int n_groups,
                               int q_per_kv, int hs, void* y, int ldy, int softmax_mode, void* stream) {
    AdapterAttnArgs aa;
    int rc = check_adapter_attn("attn_adapter_prefix", ak, av, gate, aT, n_groups, q_per_kv, hs, &aa);
    if (rc != PARROT_OK) return rc;
    PARROT_REQUIRE(q && y, "attn_adapter_prefix: null pointer");
    PARROT_REQUIRE(softmax_mode == 0 || softmax_mode == 1, "attn_adapter_prefix: softmax_mode must be 0 or 1");
    PARROT_REQUIRE(M >= 1 && M <= 65535 && n_groups * q_per_kv <= 65535, "attn_adapter_prefix: M / n_head out of range");
    PARROT_REQUIRE(ldy >= n_groups * q_per_kv * hs, "attn_adapter_prefix: ldy too small");
    PARROT_REQUIRE(aligned16(q), "attn_adapter_prefix: q must be 16-byte aligned");
    const int n_head = n_groups * q_per_kv;
    return with_head_size("attn_adapter_prefix", hs, [&](auto HS) {
        return launch(K_ATTN_ADAPTER_PREFIX, attn_adapter_prefix_kernel<decltype(HS)::value>, dim3(n_head, M), dim3(64), 0, (hipStream_t)stream,
                      (const bf16_t*)q, n_head, aa, q_per_kv, (bf16_t*)y, ldy, softmax_mode);
    });
}

int64_t parrot_attn_workspace_floats(int M, int n_head, int hs, int nsplit) {
    return (int64_t)M * n_head * nsplit * (hs + 2);
}

int parrot_attn_decode(const void* q, int M, const int32_t* pos, const void* k_cache, const void* v_cache, int n_groups,
                       int q_per_kv, int hs, int S, int nsplit, void* workspace, void* y, int ldy, int softmax_mode, void* stream) {
    {
        const int rc = check_softmax_mode("attn_decode", softmax_mode, S, nsplit);
        if (rc != PARROT_OK) return rc;
    }
    PARROT_REQUIRE(q && pos && k_cache && v_cache && y, "attn_decode: null pointer");
    PARROT_REQUIRE(M >= 1 && n_groups >= 1 && q_per_kv >= 1 && S >= 1, "attn_decode: bad shape");
    PARROT_REQUIRE(nsplit >= 1 && nsplit <= 65535 && M <= 65535, "attn_decode: nsplit/M out of range");
    PARROT_REQUIRE(nsplit == 1 || workspace, "attn_decode: workspace required when nsplit > 1");
    PARROT_REQUIRE(ldy >= n_groups * q_per_kv * hs, "attn_decode: ldy too small");
    PARROT_REQUIRE(aligned16(q) && aligned16(k_cache) && aligned16(v_cache), "attn_decode: q/k/v must be 16-byte aligned");
    return with_head_size("attn_decode", hs, [&](auto HS) {
        return attn_launch<decltype(HS)::value>(q, M, pos, k_cache, v_cache, n_groups, q_per_kv, S, nsplit, workspace, y, ldy, softmax_mode,
                                                (hipStream_t)stream);
    });
}

}  // extern "C"
