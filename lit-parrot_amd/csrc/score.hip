// Scoring: the log-probability a row of logits gives to a GIVEN token (validation loss, perplexity, ranking of continuations).
//     logprob = x_t - lse,   lse = mx + log(sum_i exp(x_i - mx)),   mx = max_i x_i            (fp32, expf / logf)
// and is_greedy: whether t is the token parrot_argmax_advance would emit for the row.  One workgroup per row, the row read from
// memory once: no (rows x V) fp32 copy of the logits, no log_softmax + gather + arg-max launches.
#include "parrot_common.h"

namespace parrot {

constexpr int kScoreThreads = 1024;  // the workgroup of the sampling kernels (misc.hip, kSampleThreads)

// The logits of a thread, as SampleElems of misc.hip holds them: NCH > 0: chunks of 8 consecutive elements t, t + 1024, ... in
// registers (one 16-byte load each, all requested before the first use; the row 16-byte aligned, V a multiple of 8,
// V <= 8192 * NCH); NCH = 0: any V and alignment, re-read element by element in every pass.
// each(f) calls f(index, value) for the thread's elements in ascending index order.
template <int NCH>
struct ScoreElems {
    uint32_t tv[NCH > 0 ? NCH : 1][4];
    const bf16_t* logits;
    int V;
    __device__ __forceinline__ void load() {
        if constexpr (NCH > 0) {
            const uint4* lg = reinterpret_cast<const uint4*>(logits);
            const int chunks = V >> 3;
            uint4 v4[NCH];
#pragma unroll
            for (int j = 0; j < NCH; ++j) v4[j] = lg[min((int)threadIdx.x + j * kScoreThreads, chunks - 1)];  // (clamped: in bounds)
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                tv[j][0] = v4[j].x;
                tv[j][1] = v4[j].y;
                tv[j][2] = v4[j].z;
                tv[j][3] = v4[j].w;
            }
        }
    }
    template <class F>
    __device__ __forceinline__ void each(F f) const {
        if constexpr (NCH > 0) {
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int c = (int)threadIdx.x + j * kScoreThreads;
                if (c < (V >> 3)) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) f(c * 8 + e, (e & 1) ? bfhi(tv[j][e >> 1]) : bflo(tv[j][e >> 1]));
                }
            }
        } else {
            for (int i = threadIdx.x; i < V; i += kScoreThreads) f(i, bf2f(logits[i]));
        }
    }
};

// Scores token t against one row of V >= 1 logits; thread 0 stores the results.  Called by every thread of the workgroup.
//   arg-max: argmax_row's rule (misc.hip) - a NaN logit counts as -inf, the lowest index wins a tie; (value, -index) is a total
//            order, so the winner does not depend on how the elements are dealt to the threads;
//   mx:      the winner's value (the maximum over the non-NaN logits);
//   sum:     a NaN logit makes exp(NaN - mx) = NaN and with it the sum and the result: NaN propagates.
// t outside [0, V): NaN and is_greedy = 0, nothing is read for it.
template <int NCH>
__device__ __forceinline__ void score_row(const bf16_t* __restrict__ logits, int V, int64_t t, float* __restrict__ logprob,
                                          int32_t* __restrict__ is_greedy) {
    __shared__ float redf[kScoreThreads / 64];
    __shared__ int redi[kScoreThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ScoreElems<NCH> el;
    el.logits = logits;
    el.V = V;
    el.load();
    float best = -INFINITY;
    int bi = 0x7fffffff;  // (a thread without elements: loses against every index)
    el.each([&](int i, float v) {
        if (v != v) v = -INFINITY;
        if (bi == 0x7fffffff || v > best) {  // (indices ascend per thread: a tie keeps the lower one)
            best = v;
            bi = i;
        }
    });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (ov > best || (ov == best && oi < bi)) {
            best = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        redf[wave] = best;
        redi[wave] = bi;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kScoreThreads / 64; ++w) {  // every thread: the same 16 pairs in the same order
        const float ov = redf[w];
        const int oi = redi[w];
        if (ov > best || (ov == best && oi < bi)) {
            best = ov;
            bi = oi;
        }
    }
    __syncthreads();  // (redf is written again below)
    const float mx = best;
    float sum = 0.f;
    el.each([&](int, float v) { sum += expf(v - mx); });
    sum = wave_sum(sum);
    if (lane == 0) redf[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        sum = 0.f;
        for (int w = 0; w < kScoreThreads / 64; ++w) sum += redf[w];
        const bool inside = t >= 0 && t < (int64_t)V;
        const float lse = mx + logf(sum);
        *logprob = inside ? bf2f(logits[t]) - lse : __uint_as_float(0x7fc00000u);
        if (is_greedy != nullptr) *is_greedy = (inside && t == (int64_t)bi) ? 1 : 0;
    }
}

// one workgroup per row m of logits [M][ldl]: the rows of a prompt pass
template <int NCH>
__global__ void __launch_bounds__(kScoreThreads)
token_logprob_rows_kernel(const bf16_t* __restrict__ logits, int V, int ldl, const int64_t* __restrict__ targets,
                          float* __restrict__ logprob, int32_t* __restrict__ is_greedy) {
    const int m = blockIdx.x;
    score_row<NCH>(logits + (int64_t)m * ldl, V, targets[m], logprob + m, is_greedy != nullptr ? is_greedy + m : nullptr);
}

// The teacher-forced twin of argmax_advance_rows_kernel (misc.hip): one workgroup per row b of logits [B][ldl]; the token at
// tokens[b][pos[b] + 1] is already there and is scored, never written.  Frozen rows (block-uniform: every thread reads the same
// words) write nothing and do not advance.
template <int NCH>
__global__ void __launch_bounds__(kScoreThreads)
logprob_advance_rows_kernel(const bf16_t* __restrict__ logits, int V, int ldl, const int64_t* __restrict__ tokens, int ldt,
                            int32_t* __restrict__ pos, const int32_t* __restrict__ end, float* __restrict__ logprob,
                            int32_t* __restrict__ is_greedy, int ldo) {
    const int b = blockIdx.x;
    const int p = pos[b];
    if (p + 1 >= end[b] || p + 1 >= ldt || p + 1 >= ldo || p + 1 < 0) return;
    const int64_t o = (int64_t)b * ldo + (p + 1);
    score_row<NCH>(logits + (int64_t)b * ldl, V, tokens[(int64_t)b * ldt + (p + 1)], logprob + o, is_greedy + o);
    if (threadIdx.x == 0) pos[b] = p + 1;  // (every thread read pos[b] before score_row's barriers)
}

// rows in registers when every row is 16-byte aligned and a multiple of 8 long
static inline bool score_rows_vec(const void* logits, int V, int ldl, int rows) {
    return V % 8 == 0 && aligned16(logits) && (rows == 1 || ldl % 8 == 0);
}

}  // namespace parrot

using namespace parrot;

extern "C" {

#define PARROT_SCORE_GO(KID, KERNEL, ROWS, ...)                                                                              \
    do {                                                                                                                     \
        const bool vec = score_rows_vec(logits, V, ldl, ROWS);                                                               \
        if (vec && V <= 8192 * 4)                                                                                            \
            return launch(KID, KERNEL<4>, dim3(ROWS), dim3(kScoreThreads), 0, (hipStream_t)stream, __VA_ARGS__);             \
        if (vec && V <= 8192 * 8)                                                                                            \
            return launch(KID, KERNEL<8>, dim3(ROWS), dim3(kScoreThreads), 0, (hipStream_t)stream, __VA_ARGS__);             \
        return launch(KID, KERNEL<0>, dim3(ROWS), dim3(kScoreThreads), 0, (hipStream_t)stream, __VA_ARGS__);                 \
    } while (0)

int parrot_token_logprob_rows(const void* logits, int V, int ldl, int M, const int64_t* targets, float* logprob, int32_t* is_greedy,
                              void* stream) {
    PARROT_REQUIRE(logits && targets && logprob, "token_logprob_rows: null pointer");
    PARROT_REQUIRE(V >= 1, "token_logprob_rows: V=%d (at least one logit)", V);
    PARROT_REQUIRE(M >= 1, "token_logprob_rows: M=%d (at least one row)", M);
    PARROT_REQUIRE(ldl >= V, "token_logprob_rows: ldl=%d is smaller than V=%d", ldl, V);
    PARROT_SCORE_GO(K_TOKEN_LOGPROB_ROWS, token_logprob_rows_kernel, M, (const bf16_t*)logits, V, ldl, targets, logprob, is_greedy);
}

int parrot_logprob_advance_rows(const void* logits, int V, int ldl, int B, const int64_t* tokens, int ldt, int32_t* pos,
                                const int32_t* end, float* logprob, int32_t* is_greedy, int ldo, void* stream) {
    PARROT_REQUIRE(logits && tokens && pos && end && logprob && is_greedy, "logprob_advance_rows: null pointer");
    PARROT_REQUIRE(V >= 1, "logprob_advance_rows: V=%d (at least one logit)", V);
    PARROT_REQUIRE(B >= 1 && B <= kMaxDecodeRows, "logprob_advance_rows: B=%d (1 .. %d)", B, kMaxDecodeRows);
    PARROT_REQUIRE(ldl >= V, "logprob_advance_rows: ldl=%d is smaller than V=%d", ldl, V);
    PARROT_REQUIRE(ldt >= 1, "logprob_advance_rows: ldt=%d", ldt);
    PARROT_REQUIRE(ldo >= 1, "logprob_advance_rows: ldo=%d", ldo);
    PARROT_SCORE_GO(K_LOGPROB_ADVANCE_ROWS, logprob_advance_rows_kernel, B, (const bf16_t*)logits, V, ldl, tokens, ldt, pos, end,
                    logprob, is_greedy, ldo);
}

#undef PARROT_SCORE_GO

}  // extern "C"
