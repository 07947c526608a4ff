// Small ops of the decode step: token embedding gather and the greedy sampling step.
#include "parrot_common.h"

namespace parrot {

// x[m] = wte[tokens[base + m]]  (lit_gpt/model.py:99); 16-B copies
__global__ void __launch_bounds__(256)
embedding_kernel(const uint4* __restrict__ wte, int d16, const int64_t* __restrict__ tokens,
                 const int32_t* __restrict__ pos_ptr, uint4* __restrict__ out, int ldo16) {
    const int m = blockIdx.y;
    const int64_t base = pos_ptr ? (int64_t)pos_ptr[0] : 0;
    const int64_t tok = tokens[base + m];
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < d16; c += gridDim.x * blockDim.x)
        out[(int64_t)m * ldo16 + c] = wte[tok * d16 + c];
}

// batched decode: x[b] = wte[tokens[b * ld_tokens + (pos ? pos[b] : 0)]], one row per sequence
__global__ void __launch_bounds__(256)
embedding_rows_kernel(const uint4* __restrict__ wte, int d16, const int64_t* __restrict__ tokens, int ld_tokens,
                      const int32_t* __restrict__ pos, uint4* __restrict__ out, int ldo16) {
    const int b = blockIdx.y;
    const int64_t tok = tokens[(int64_t)b * ld_tokens + (pos ? pos[b] : 0)];
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < d16; c += gridDim.x * blockDim.x)
        out[(int64_t)b * ldo16 + c] = wte[tok * d16 + c];
}

// Batched decode: row b of the sampling step is frozen (no token write, no advance) once its next position would reach end[b]
// (or the row of its token buffer) or its last written token is eos_id (-1: none).  A frozen row re-runs its own position in
// the next step, which rewrites the same K/V slot with the same values.  Block-uniform: every thread reads the same words.
__device__ __forceinline__ bool decode_row_frozen(const int64_t* tokens_row, int ldt, int pos, int end, int eos_id) {
    return pos + 1 >= end || pos + 1 >= ldt || (eos_id >= 0 && tokens_row[pos] == (int64_t)eos_id);
}

// generate/base.py:136-153 with temperature > 0 and top_k = 1: the sampled token is the arg-max of the logits.
// (The reference draws from a one-hot multinomial; with tied maxima it picks one of them at random, here the
// lowest index wins.)  Single workgroup; then the loop state advances: tokens[pos+1] = best, pos += 1.
constexpr int kArgmaxThreads = 1024;
// the arg-max of one row of logits; the result is valid in thread 0 (0x7fffffff: no element)
__device__ __forceinline__ int argmax_row(const bf16_t* __restrict__ logits, int V, int vec) {
    __shared__ float sv[kArgmaxThreads / 64];
    __shared__ int si[kArgmaxThreads / 64];
    float best = -INFINITY;
    int bi = 0x7fffffff;
    // 16-byte chunks (8 logits), thread t owns chunks t, t + 1024, ...: kArgmaxIt of them are requested together
    // (clamped, unconditional) before the first compare; indices ascend per thread, so ties keep the lowest.
    // (The row must be 16-byte aligned: checked on the host; a ragged tail is masked by index.)
    constexpr int kArgmaxIt = 4;
    const int chunks = (V + 7) >> 3;
    const uint4* lg = reinterpret_cast<const uint4*>(logits);
    if (!vec) {  // fewer than 8 logits or an unaligned row: element loads
        for (int i = threadIdx.x; i < V; i += kArgmaxThreads) {
            float v = bf2f(logits[i]);
            if (v != v) v = -INFINITY;
            if (bi == 0x7fffffff || v > best) {
                best = v;
                bi = i;
            }
        }
    }
    for (int c0 = threadIdx.x; vec && c0 < chunks; c0 += kArgmaxThreads * kArgmaxIt) {
        uint4 v4[kArgmaxIt];
#pragma unroll
        for (int k = 0; k < kArgmaxIt; ++k) v4[k] = lg[min(c0 + k * kArgmaxThreads, (V >> 3) - 1)];
#pragma unroll
        for (int k = 0; k < kArgmaxIt; ++k) {
            const int c = c0 + k * kArgmaxThreads;
            const uint32_t dw[4] = {v4[k].x, v4[k].y, v4[k].z, v4[k].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int i = c * 8 + e;
                float v = (e & 1) ? bfhi(dw[e >> 1]) : bflo(dw[e >> 1]);
                if (c >= (V >> 3)) v = (i < V) ? bf2f(logits[i < V ? i : 0]) : -INFINITY;  // ragged tail chunk: element loads
                if (v != v) v = -INFINITY;  // a NaN logit never wins
                if (i < V && (bi == 0x7fffffff || v > best)) {
                    best = v;
                    bi = i;
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (ov > best || (ov == best && oi < bi)) {
            best = ov;
            bi = oi;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sv[wave] = best;
        si[wave] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kArgmaxThreads / 64; ++w)
            if (sv[w] > best || (sv[w] == best && si[w] < bi)) {
                best = sv[w];
                bi = si[w];
            }
    }
    return bi;
}

__global__ void __launch_bounds__(kArgmaxThreads)
argmax_advance_kernel(const bf16_t* __restrict__ logits, int V, int vec, int64_t* __restrict__ tokens, int32_t* __restrict__ pos_ptr) {
    const int bi = argmax_row(logits, V, vec);
    if (threadIdx.x == 0) {
        const int pos = pos_ptr[0];
        tokens[pos + 1] = (bi == 0x7fffffff) ? 0 : bi;
        pos_ptr[0] = pos + 1;
    }
}

// batched decode: one workgroup per row b of logits [B][ldl]; tokens [B][ldt], pos [B], end [B]
__global__ void __launch_bounds__(kArgmaxThreads)
argmax_advance_rows_kernel(const bf16_t* __restrict__ logits, int V, int ldl, int vec, int64_t* __restrict__ tokens, int ldt,
                           int32_t* __restrict__ pos, const int32_t* __restrict__ end, int eos_id) {
    const int b = blockIdx.x;
    int64_t* trow = tokens + (int64_t)b * ldt;
    const int p = pos[b];
    if (decode_row_frozen(trow, ldt, p, end[b], eos_id)) return;
    const int bi = argmax_row(logits + (int64_t)b * ldl, V, vec);
    if (threadIdx.x == 0) {
        trow[p + 1] = (bi == 0x7fffffff) ? 0 : bi;
        pos[b] = p + 1;
    }
}

// generate/base.py:136-153 with top_k != 1 (the reference's default call is temperature 0.8, top_k 200): the whole sampling
// step in one launch, with the arithmetic of the torch device ops the reference runs there, so that the same generator state
// draws the same token (tools/probes/torch_sampling_probe.py checks each equivalence on the GPU):
//     logits = logits / temperature                      bf16(float(l) * (1.0f / T))  (bf16 tensor / python scalar)
//     v, _ = topk(logits, k); logits = where(logits < v[[-1]], -inf, logits)    kept: the values >= the k-th largest
//     probs = softmax(logits)                            bf16(exp(x - max) / sum), fp32 inside
//     idx = multinomial(probs, 1)                        = argmax(probs / q), q = empty_like(probs).exponential_(1): the caller
//                                                        draws q with that very torch call (same generator consumption, graph
//                                                        safe) and hands it over; ties: the lowest index
//     tokens[pos + 1] = idx; pos += 1
// torch.multinomial's validity checks (two host syncs per token) are not reproduced.  One workgroup: the k-th largest value by a
// two-pass radix select over the 16-bit keys (256-bin histograms in LDS), then the maximum / sum, then the arg-max.
constexpr int kSampleThreads = 1024;
__device__ __forceinline__ uint32_t bf16_key(bf16_t b) {  // monotone: a < b (as numbers) <=> key(a) < key(b); -0 < +0
    return (b & 0x8000u) ? (uint32_t)(uint16_t)~b : (uint32_t)b | 0x8000u;
}
// bin (from the top) in which the running count reaches k: wave 0 scans the 256-bin histogram, 4 bins per lane from the top;
// returns the bin and, through *before, how many elements lie in the bins above it
__device__ __forceinline__ int select_bin(const uint32_t* hist, uint32_t k, uint32_t* before) {
    const int lane = threadIdx.x & 63;
    uint32_t h[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h[i] = hist[255 - (4 * lane + i)];
        s += h[i];
    }
    uint32_t incl = s;  // inclusive prefix over the lanes (lane 0 = the top bins)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, off, 64);
        if (lane >= off) incl += o;
    }
    const uint32_t excl = incl - s;
    const bool mine = excl < k && k <= incl;
    int bin = -1;
    uint32_t bef = 0;
    if (mine) {
        uint32_t c = excl;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (bin < 0 && c + h[i] >= k) {
                bin = 255 - (4 * lane + i);
                bef = c;
            }
            c += h[i];
        }
    }
    const uint64_t who = __ballot(mine);
    const int src = who ? __ffsll((long long)who) - 1 : 0;
    *before = (uint32_t)__shfl((int)bef, src, 64);
    return __shfl(bin, src, 64);
}
// The scaled logits of a thread: NCH > 0: chunks of 8 consecutive elements t, t + 1024, ... held in registers (one 16-byte load
// each; the row 16-byte aligned, V a multiple of 8, V <= 8192 * NCH); NCH = 0: any V, re-read element by element in every pass.
// each(f) calls f(index, scaled bf16) for the thread's elements in ascending index order.
template <int NCH>
struct SampleElems {
    uint32_t tv[NCH > 0 ? NCH : 1][4];
    const bf16_t* logits;
    int V;
    float inv_t;
    __device__ __forceinline__ bf16_t scaled(bf16_t l) const { return f2bf(__fmul_rn(bf2f(l), inv_t)); }
    __device__ __forceinline__ void load() {
        if constexpr (NCH > 0) {
            const uint4* lg = reinterpret_cast<const uint4*>(logits);
            const int chunks = V >> 3;
            uint4 v4[NCH];
#pragma unroll
            for (int j = 0; j < NCH; ++j) v4[j] = lg[min((int)threadIdx.x + j * kSampleThreads, chunks - 1)];
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const uint32_t dw[4] = {v4[j].x, v4[j].y, v4[j].z, v4[j].w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    tv[j][e] = (uint32_t)scaled((bf16_t)(dw[e] & 0xffffu)) | ((uint32_t)scaled((bf16_t)(dw[e] >> 16)) << 16);
            }
        }
    }
    template <class F>
    __device__ __forceinline__ void each(F f) const {
        if constexpr (NCH > 0) {
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int c = (int)threadIdx.x + j * kSampleThreads;
                if (c < (V >> 3)) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) f(c * 8 + e, (bf16_t)((e & 1) ? (tv[j][e >> 1] >> 16) : (tv[j][e >> 1] & 0xffffu)));
                }
            }
        } else {
            for (int i = threadIdx.x; i < V; i += kSampleThreads) f(i, scaled(logits[i]));
        }
    }
};

// the sampled index of one row; valid in thread 0 (0x7fffffff: no element)
template <int NCH>
__device__ __forceinline__ int topk_sample_row(const bf16_t* __restrict__ logits, int V, float inv_temperature, int top_k,
                                               const bf16_t* __restrict__ noise, bf16_t* __restrict__ probs_out) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sel[2];
    __shared__ float redf[kSampleThreads / 64];
    __shared__ int redi[kSampleThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    SampleElems<NCH> el;
    el.logits = logits;
    el.V = V;
    el.inv_t = inv_temperature;
    el.load();
    // ---- the k-th largest scaled logit (as a key); top_k <= 0 or >= V: everything is kept
    uint32_t kth_key = 0u;
    if (top_k > 0 && top_k < V) {
        uint32_t k = (uint32_t)top_k, hi = 0;
        for (int pass = 0; pass < 2; ++pass) {
            for (int i = threadIdx.x; i < 256; i += kSampleThreads) hist[i] = 0u;
            __syncthreads();
            el.each([&](int, bf16_t t) {
                const uint32_t key = bf16_key(t);
                if (pass == 0)
                    atomicAdd(&hist[key >> 8], 1u);
                else if ((key >> 8) == hi)
                    atomicAdd(&hist[key & 0xffu], 1u);
            });
            __syncthreads();
            if (wave == 0) {
                uint32_t before;
                const int bin = select_bin(hist, k, &before);
                if (lane == 0) {
                    sel[0] = (uint32_t)bin;
                    sel[1] = before;
                }
            }
            __syncthreads();
            if (pass == 0) {
                hi = sel[0];
                k -= sel[1];
            } else {
                kth_key = (hi << 8) | sel[0];
            }
            __syncthreads();
        }
    }
    // ---- maximum and sum of exp over the kept values (fp32; the maximum is always kept)
    float mx = -INFINITY;
    el.each([&](int, bf16_t t) { mx = fmaxf(mx, bf2f(t)); });
    mx = wave_max(mx);
    if (lane == 0) redf[wave] = mx;
    __syncthreads();
    for (int w = 0; w < kSampleThreads / 64; ++w) mx = fmaxf(mx, redf[w]);
    __syncthreads();
    float sum = 0.f;
    el.each([&](int, bf16_t t) {
        if (bf16_key(t) >= kth_key) sum += expf(bf2f(t) - mx);
    });
    sum = wave_sum(sum);
    if (lane == 0) redf[wave] = sum;
    __syncthreads();
    sum = 0.f;
    for (int w = 0; w < kSampleThreads / 64; ++w) sum += redf[w];
    // ---- arg-max of probs / q (both bf16, the quotient rounded to bf16), lowest index on ties
    float best = -INFINITY;
    int bi = 0x7fffffff;
    el.each([&](int i, bf16_t t) {
        const bf16_t pb = bf16_key(t) >= kth_key ? f2bf(__fdiv_rn(expf(bf2f(t) - mx), sum)) : (bf16_t)0;
        if (probs_out != nullptr) probs_out[i] = pb;
        // (a cropped element has probability 0 and never beats a kept one: its noise is not even read)
        float r = pb != 0 ? bf2f(f2bf(__fdiv_rn(bf2f(pb), bf2f(noise[i])))) : 0.f;
        if (r != r) r = -INFINITY;
        if (bi == 0x7fffffff || r > best) {  // (indices ascend per thread: a tie keeps the lower one)
            best = r;
            bi = i;
        }
    });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) {
            best = ov;
            bi = oi;
        }
    }
    __syncthreads();
    if (lane == 0) {
        redf[wave] = best;
        redi[wave] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kSampleThreads / 64; ++w)
            if (redi[w] != 0x7fffffff && (bi == 0x7fffffff || redf[w] > best || (redf[w] == best && redi[w] < bi))) {
                best = redf[w];
                bi = redi[w];
            }
    }
    return bi;
}

template <int NCH>
__global__ void __launch_bounds__(kSampleThreads)
topk_sample_kernel(const bf16_t* __restrict__ logits, int V, float inv_temperature, int top_k, const bf16_t* __restrict__ noise,
                   bf16_t* __restrict__ probs_out, int64_t* __restrict__ tokens, int32_t* __restrict__ pos_ptr) {
    const int bi = topk_sample_row<NCH>(logits, V, inv_temperature, top_k, noise, probs_out);
    if (threadIdx.x == 0) {
        const int pos = pos_ptr[0];
        tokens[pos + 1] = (bi == 0x7fffffff) ? 0 : bi;
        pos_ptr[0] = pos + 1;
    }
}

// batched decode: one workgroup per row b of logits [B][ldl] and noise [B][V]; tokens [B][ldt], pos [B], end [B]
template <int NCH>
__global__ void __launch_bounds__(kSampleThreads)
topk_sample_rows_kernel(const bf16_t* __restrict__ logits, int V, int ldl, float inv_temperature, int top_k,
                        const bf16_t* __restrict__ noise, int64_t* __restrict__ tokens, int ldt, int32_t* __restrict__ pos,
                        const int32_t* __restrict__ end, int eos_id) {
    const int b = blockIdx.x;
    int64_t* trow = tokens + (int64_t)b * ldt;
    const int p = pos[b];
    if (decode_row_frozen(trow, ldt, p, end[b], eos_id)) return;
    const int bi = topk_sample_row<NCH>(logits + (int64_t)b * ldl, V, inv_temperature, top_k, noise + (int64_t)b * V, nullptr);
    if (threadIdx.x == 0) {
        trow[p + 1] = (bi == 0x7fffffff) ? 0 : bi;
        pos[b] = p + 1;
    }
}

// Device-side stop-sequence check of the chat loop (chat/base.py:80-87 restated on the token buffer): after the sampling
// step has written tokens[pos] (generated token number t = pos - first_gen), a stop sequence of n tokens matches iff
// t >= L - 1 (L = longest stop sequence: the reference's look-back buffer is still filling before that and its tail holds
// the filler) and tokens[pos-n+1 .. pos] equals it; sequences are tried in list order, the first hit is latched:
// flag[0] = t of the hit (-1: none so far), flag[1] = n.  One wave; the host reads the flag every few tokens instead of
// comparing on the host after every token.
__global__ void __launch_bounds__(64)
stop_check_kernel(const int64_t* __restrict__ tokens, const int32_t* __restrict__ pos_ptr, const int32_t* __restrict__ first_gen,
                  const int64_t* __restrict__ stop_flat, const int32_t* __restrict__ stop_off, int n_stop, int L,
                  int32_t* __restrict__ flag) {
    if (flag[0] >= 0) return;  // latched
    const int pos = pos_ptr[0];
    const int t = pos - first_gen[0];
    if (t < L - 1) return;
    for (int s = 0; s < n_stop; ++s) {
        const int o = stop_off[s], n = stop_off[s + 1] - o;
        bool eq = true;
        for (int i = threadIdx.x; i < n; i += 64) eq = eq && (tokens[pos - n + 1 + i] == stop_flat[o + i]);
        if (__all(eq)) {  // uniform
            if (threadIdx.x == 0) {
                flag[0] = t;
                flag[1] = n;
            }
            return;
        }
    }
}


// ------------------------------------------------------------------------------------------ prompt-lookup speculative decoding
// Loop state beside tokens / pos, int32 words: the drafting and the verification kernel each own some of them and the host
// reads all of them in one copy per step.
enum SpecState : int {
    SPEC_MATCHED = 0,   // ngram_draft: drafts of its last call that were copied from an earlier occurrence (0: no match)
    SPEC_ACCEPTED = 1,  // verify_advance: accepted drafts, summed over its calls
    SPEC_STEPS = 2,     // verify_advance: its calls that advanced
    SPEC_POS = 3,       // ngram_draft: pos[0] as it saw it
    SPEC_LAST = 4,      // ngram_draft: tokens[pos[0]] (the host's eos test)
    SPEC_WORDS = 8
};
constexpr int kDraftThreads = 256;
constexpr int kMaxDraftLen = kMaxDecodeRows - 1;
constexpr int kMaxNgram = 16;

// Prompt lookup: tokens[0 .. pos] are known.  For n = ngram_max down to ngram_min (an n longer than the sequence is skipped), find the
// LARGEST j with j + n <= pos and tokens[j .. j+n-1] == tokens[pos-n+1 .. pos] - the last earlier occurrence of the newest n-gram -
// and copy what followed it: draft i = tokens[j + n + i] while that index is <= pos.  Every other draft slot (all K without a match)
// repeats tokens[pos].  The K drafts go to tokens[pos+1 .. pos+K] (slots past the buffer are dropped), beyond the valid part.
// One workgroup; thread t walks the candidates pos-n-t, pos-n-t-256, ... downwards, so its first hit is its largest, and the
// workgroup's answer is one max-reduction over those: the result does not depend on scheduling.
__global__ void __launch_bounds__(kDraftThreads)
ngram_draft_kernel(int64_t* __restrict__ tokens, int L, const int32_t* __restrict__ pos_ptr, int K, int ngram_max, int ngram_min,
                   int32_t* __restrict__ state) {
    __shared__ int sh_best[kDraftThreads / 64];
    const int pos = pos_ptr[0];
    if (pos < 0 || pos >= L) return;  // (never in the decode loop: nothing to read)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int hit_j = -1, hit_n = 0;
    for (int n = ngram_max; n >= ngram_min; --n) {
        if (pos - n + 1 < 0) continue;  // uniform
        const int64_t* tail = tokens + (pos - n + 1);
        int best = -1;
        for (int j = pos - n - (int)threadIdx.x; j >= 0; j -= kDraftThreads) {
            bool eq = true;
            for (int i = n - 1; i >= 0 && eq; --i) eq = tokens[j + i] == tail[i];
            if (eq) {
                best = j;
                break;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) best = max(best, __shfl_xor(best, off, 64));
        if (lane == 0) sh_best[wave] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kDraftThreads / 64; ++w) best = max(best, sh_best[w]);
        __syncthreads();  // (sh_best is written again for the next n)
        if (best >= 0) {  // uniform
            hit_j = best;
            hit_n = n;
            break;
        }
    }
    const int64_t last = tokens[pos];
    const int follow = hit_j + hit_n;  // first token after the earlier occurrence (<= pos when there is one)
    if ((int)threadIdx.x < K) {
        const int i = threadIdx.x;
        const int64_t d = (hit_j >= 0 && follow + i <= pos) ? tokens[follow + i] : last;
        if (pos + 1 + i < L) tokens[pos + 1 + i] = d;
    }
    if (threadIdx.x == 0) {
        state[SPEC_MATCHED] = hit_j >= 0 ? min(K, pos - follow + 1) : 0;
        state[SPEC_POS] = pos;
        state[SPEC_LAST] = (int32_t)last;
    }
}

// Greedy verification of the M = K + 1 rows of a speculative step: row m holds the logits of position pos + m, whose input token
// was tokens[pos + m] (m >= 1: draft m - 1).  a_m = argmax_row(logits[m]) - the device function of argmax_advance, so the bits and
// the tie rule are its own.  c = the number of leading drafts with a_m == tokens[pos+1+m], cut so that no token is written at or
// past min(end, L) and, with eos_id >= 0, at the first a_m == eos_id (the eos token is written; the sequence is then frozen as
// decode_row_frozen says, and a later call neither writes nor advances).  Then tokens[pos+1+c] = a_c, pos += c + 1.  Rows after
// the first rejected one are not even read.  One workgroup, rows in turn.
__global__ void __launch_bounds__(kArgmaxThreads)
verify_advance_kernel(const bf16_t* __restrict__ logits, int V, int ldl, int vec, int M, int64_t* __restrict__ tokens, int L,
                      int32_t* __restrict__ pos_ptr, const int32_t* __restrict__ end_ptr, int eos_id, int32_t* __restrict__ state,
                      int32_t* __restrict__ row_pos) {
    __shared__ int sh_more;
    const int pos = pos_ptr[0];
    const int stop = min(end_ptr[0], L);
    if (decode_row_frozen(tokens, L, pos, end_ptr[0], eos_id)) {
        if (row_pos != nullptr && (int)threadIdx.x < M) row_pos[threadIdx.x] = pos + threadIdx.x;
        return;
    }
    for (int m = 0; m < M; ++m) {
        const int bi = argmax_row(logits + (int64_t)m * ldl, V, vec);
        if (threadIdx.x == 0) {
            const int a = (bi == 0x7fffffff) ? 0 : bi;
            // draft m is accepted when it is the arg-max, is not eos, and the token after it still has a slot
            const bool more = m + 1 < M && tokens[pos + 1 + m] == (int64_t)a && !(eos_id >= 0 && a == eos_id) && pos + 2 + m < stop;
            if (!more) {
                tokens[pos + 1 + m] = a;  // (pos + 1 + m < stop: by the frozen test for m = 0, by `more` of row m - 1 after)
                pos_ptr[0] = pos + m + 1;
                state[SPEC_ACCEPTED] += m;
                state[SPEC_STEPS] += 1;
                if (row_pos != nullptr)
                    for (int r = 0; r < M; ++r) row_pos[r] = pos + m + 1 + r;
            }
            sh_more = more;
        }
        __syncthreads();  // (also orders thread 0's reads of argmax_row's LDS before the next row's writes)
        if (!sh_more) return;
    }
}

}  // namespace parrot

using namespace parrot;

extern "C" {

int parrot_embedding(const void* wte, int d, const int64_t* tokens, const int32_t* pos, int M, void* out, int ldo,
                     void* stream) {
    PARROT_REQUIRE(wte && tokens && out, "embedding: null pointer");
    PARROT_REQUIRE(M >= 1 && M <= 65535 && d >= 8 && d % 8 == 0 && ldo % 8 == 0 && ldo >= d,
                   "embedding: d and ldo must be multiples of 8 (d=%d ldo=%d M=%d)", d, ldo, M);
    PARROT_REQUIRE(aligned16(wte) && aligned16(out), "embedding: pointers must be 16-byte aligned");
    const int d16 = d / 8;
    return launch(K_EMBEDDING, embedding_kernel, dim3((d16 + 255) / 256, M), dim3(256), 0, (hipStream_t)stream,
                  (const uint4*)wte, d16, tokens, pos, (uint4*)out, ldo / 8);
}

int parrot_stop_check(const int64_t* tokens, const int32_t* pos, const int32_t* first_gen, const int64_t* stop_flat,
                      const int32_t* stop_off, int n_stop, int longest, int32_t* flag, void* stream) {
    PARROT_REQUIRE(tokens && pos && first_gen && flag, "stop_check: null pointer");
    PARROT_REQUIRE(n_stop >= 0 && longest >= 1, "stop_check: bad arguments n_stop=%d longest=%d", n_stop, longest);
    PARROT_REQUIRE(n_stop == 0 || (stop_flat && stop_off), "stop_check: stop sequences missing");
    return launch(K_STOP_CHECK, stop_check_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, tokens, pos, first_gen, stop_flat,
                  stop_off, n_stop, longest, flag);
}

int parrot_topk_sample(const void* logits, int V, float temperature, int top_k, const void* noise_exp1, void* probs_out,
                       int64_t* tokens, int32_t* pos, void* stream) {
    PARROT_REQUIRE(logits && noise_exp1 && tokens && pos, "topk_sample: null pointer");
    PARROT_REQUIRE(V >= 1, "topk_sample: V=%d", V);
    PARROT_REQUIRE(temperature > 0.f, "topk_sample: temperature must be positive (got %g)", (double)temperature);
    // the row in registers when it is 16-byte aligned, a multiple of 8 long and at most 32768 elements; else re-read per pass
    const bool vec = V % 8 == 0 && aligned16(logits);
#define PARROT_SAMPLE_GO(NCHV)                                                                                                    \
    return launch(K_TOPK_SAMPLE, topk_sample_kernel<NCHV>, dim3(1), dim3(kSampleThreads), 0, (hipStream_t)stream, (const bf16_t*)logits, \
                  V, 1.0f / temperature, top_k, (const bf16_t*)noise_exp1, (bf16_t*)probs_out, tokens, pos)
    if (vec && V <= 8192 * 4) PARROT_SAMPLE_GO(4);
    PARROT_SAMPLE_GO(0);
#undef PARROT_SAMPLE_GO
}

int parrot_argmax_advance(const void* logits, int V, int64_t* tokens, int32_t* pos, void* stream) {
    PARROT_REQUIRE(logits && tokens && pos, "argmax_advance: null pointer");
    PARROT_REQUIRE(V >= 1, "argmax_advance: V=%d", V);
    const int vec = (V >= 8 && aligned16(logits)) ? 1 : 0;
    return launch(K_ARGMAX, argmax_advance_kernel, dim3(1), dim3(kArgmaxThreads), 0, (hipStream_t)stream,
                  (const bf16_t*)logits, V, vec, tokens, pos);
}

int parrot_embedding_rows(const void* wte, int d, const int64_t* tokens, int ld_tokens, const int32_t* pos, int B, void* out, int ldo,
                          void* stream) {
    PARROT_REQUIRE(B >= 1 && B <= kMaxDecodeRows, "embedding_rows: B=%d (1 .. %d)", B, kMaxDecodeRows);
    PARROT_REQUIRE(wte && tokens && out, "embedding_rows: null pointer");
    PARROT_REQUIRE(ld_tokens >= 1, "embedding_rows: ld_tokens=%d", ld_tokens);
    PARROT_REQUIRE(d >= 8 && d % 8 == 0 && ldo % 8 == 0 && ldo >= d,
                   "embedding_rows: d and ldo must be multiples of 8 (d=%d ldo=%d)", d, ldo);
    PARROT_REQUIRE(aligned16(wte) && aligned16(out), "embedding_rows: pointers must be 16-byte aligned");
    const int d16 = d / 8;
    return launch(K_EMBEDDING_ROWS, embedding_rows_kernel, dim3((d16 + 255) / 256, B), dim3(256), 0, (hipStream_t)stream,
                  (const uint4*)wte, d16, tokens, ld_tokens, pos, (uint4*)out, ldo / 8);
}

// the argument checks of the two batched sampling steps
static int check_sample_rows(const char* who, const void* logits, int V, int ldl, int B, const void* tokens, int ldt, const void* pos,
                             const void* end, int eos_id) {
    PARROT_REQUIRE(B >= 1 && B <= kMaxDecodeRows, "%s: B=%d (1 .. %d)", who, B, kMaxDecodeRows);
    PARROT_REQUIRE(logits && tokens && pos && end, "%s: null pointer", who);
    PARROT_REQUIRE(V >= 1 && ldl >= V && ldt >= 2, "%s: bad shape V=%d ldl=%d ldt=%d", who, V, ldl, ldt);
    PARROT_REQUIRE(eos_id >= -1, "%s: eos_id=%d (-1: none)", who, eos_id);
    return PARROT_OK;
}

int parrot_argmax_advance_rows(const void* logits, int V, int ldl, int B, int64_t* tokens, int ldt, int32_t* pos, const int32_t* end,
                               int eos_id, void* stream) {
    const int rc = check_sample_rows("argmax_advance_rows", logits, V, ldl, B, tokens, ldt, pos, end, eos_id);
    if (rc != PARROT_OK) return rc;
    const int vec = (V >= 8 && aligned16(logits) && ldl % 8 == 0) ? 1 : 0;
    return launch(K_ARGMAX_ROWS, argmax_advance_rows_kernel, dim3(B), dim3(kArgmaxThreads), 0, (hipStream_t)stream,
                  (const bf16_t*)logits, V, ldl, vec, tokens, ldt, pos, end, eos_id);
}

int parrot_topk_sample_rows(const void* logits, int V, int ldl, int B, float temperature, int top_k, const void* noise_exp1,
                            int64_t* tokens, int ldt, int32_t* pos, const int32_t* end, int eos_id, void* stream) {
    const int rc = check_sample_rows("topk_sample_rows", logits, V, ldl, B, tokens, ldt, pos, end, eos_id);
    if (rc != PARROT_OK) return rc;
    PARROT_REQUIRE(noise_exp1, "topk_sample_rows: null pointer");
    PARROT_REQUIRE(temperature > 0.f, "topk_sample_rows: temperature must be positive (got %g)", (double)temperature);
    // as parrot_topk_sample, every row in registers when they all are 16-byte aligned
    const bool vec = V % 8 == 0 && ldl % 8 == 0 && aligned16(logits);
#define PARROT_SAMPLE_ROWS_GO(NCHV)                                                                                               \
    return launch(K_TOPK_SAMPLE_ROWS, topk_sample_rows_kernel<NCHV>, dim3(B), dim3(kSampleThreads), 0, (hipStream_t)stream,      \
                  (const bf16_t*)logits, V, ldl, 1.0f / temperature, top_k, (const bf16_t*)noise_exp1, tokens, ldt, pos, end, eos_id)
    if (vec && V <= 8192 * 4) PARROT_SAMPLE_ROWS_GO(4);
    PARROT_SAMPLE_ROWS_GO(0);
#undef PARROT_SAMPLE_ROWS_GO
}

int parrot_ngram_draft(int64_t* tokens, int L, const int32_t* pos, int draft_len, int ngram_max, int ngram_min, int32_t* state,
                       void* stream) {
    PARROT_REQUIRE(tokens && pos && state, "ngram_draft: null pointer");
    PARROT_REQUIRE(L >= 1, "ngram_draft: L=%d", L);
    PARROT_REQUIRE(draft_len >= 1 && draft_len <= kMaxDraftLen, "ngram_draft: draft_len=%d (1 .. %d)", draft_len, kMaxDraftLen);
    PARROT_REQUIRE(ngram_min >= 1 && ngram_max >= ngram_min && ngram_max <= kMaxNgram,
                   "ngram_draft: n-grams %d .. %d (1 <= ngram_min <= ngram_max <= %d)", ngram_min, ngram_max, kMaxNgram);
    return launch(K_NGRAM_DRAFT, ngram_draft_kernel, dim3(1), dim3(kDraftThreads), 0, (hipStream_t)stream, tokens, L, pos, draft_len,
                  ngram_max, ngram_min, state);
}

int parrot_verify_advance(const void* logits, int V, int ldl, int M, int64_t* tokens, int L, int32_t* pos, const int32_t* end,
                          int eos_id, int32_t* state, int32_t* row_pos, void* stream) {
    PARROT_REQUIRE(logits && tokens && pos && end && state, "verify_advance: null pointer");
    PARROT_REQUIRE(M >= 2 && M <= kMaxDecodeRows, "verify_advance: M=%d rows (2 .. %d: one token and 1 .. %d drafts)", M, kMaxDecodeRows,
                   kMaxDraftLen);
    PARROT_REQUIRE(V >= 1 && ldl >= V && L >= 2, "verify_advance: bad shape V=%d ldl=%d L=%d", V, ldl, L);
    PARROT_REQUIRE(eos_id >= -1, "verify_advance: eos_id=%d (-1: none)", eos_id);
    const int vec = (V >= 8 && aligned16(logits) && ldl % 8 == 0) ? 1 : 0;
    return launch(K_VERIFY_ADVANCE, verify_advance_kernel, dim3(1), dim3(kArgmaxThreads), 0, (hipStream_t)stream, (const bf16_t*)logits,
                  V, ldl, vec, M, tokens, L, pos, end, eos_id, state, row_pos);
}

}  // extern "C"
