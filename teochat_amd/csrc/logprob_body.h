// The device body of the log-softmax over a row of fp32 logits, shared by logprob.hip (the values teo_logprob_rows returns) and beam.hip
// (the candidate keys of teo_beam_select): one visiting order, one summation order, exact comparisons.  Called by whole 1024-thread
// workgroups only.
#pragma once
#include <limits.h>

#include "ops.h"

namespace teo {

// Every entry of the row, NaN read as -inf, handed to f(value, index).  Thread t takes the quads t, t + 1024, ... (four consecutive
// entries each) by ascending index and then the entries behind the last whole quad: one 16-byte load per quad where the row is aligned
// for it, four scalar loads elsewhere -- the SAME entries in the SAME order in both forms, so a row's results do not depend on where
// it lies.
template <typename F>
__device__ __forceinline__ void logprob_visit(const float* __restrict__ row, int vocab, F f) {
    const int nq = vocab >> 2;
    auto take = [&](float v, int i) { f(v == v ? v : -INFINITY, i); };
    if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) {
        for (int q = threadIdx.x; q < nq; q += 1024) {
            const float4 v = *reinterpret_cast<const float4*>(row + 4 * q);
            take(v.x, 4 * q); take(v.y, 4 * q + 1); take(v.z, 4 * q + 2); take(v.w, 4 * q + 3);
        }
    } else {
        for (int q = threadIdx.x; q < nq; q += 1024) {
            const float a = row[4 * q], b = row[4 * q + 1], c = row[4 * q + 2], d = row[4 * q + 3];
            take(a, 4 * q); take(b, 4 * q + 1); take(c, 4 * q + 2); take(d, 4 * q + 3);
        }
    }
    for (int i = (nq << 2) + threadIdx.x; i < vocab; i += 1024) take(row[i], i);
}

// The best entry by (key(value) descending, index ascending) among those BEHIND (pv, pi) in that order (first: among all), for every
// thread of the 1024-thread workgroup.  Exact comparisons only, so the result does not depend on the reduction's shape.
// (-inf, INT_MAX): none left.
template <typename K>
__device__ __forceinline__ void logprob_next_best(const float* __restrict__ row, int vocab, bool first, float pv, int pi, float* red_v,
                                                  int* red_i, float& best, int& bi, K key) {
    best = -INFINITY; bi = INT_MAX;
    logprob_visit(row, vocab, [&](float x, int i) {
        const float v = key(x);
        const bool behind = first || v < pv || (v == pv && i > pi);
        if (behind && (v > best || (v == best && i < bi))) { best = v; bi = i; }
    });
    wave_argmax(best, bi);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();                                // (the previous pass's readers are done with red_v / red_i)
    if (l == 0) { red_v[w] = best; red_i[w] = bi; }
    __syncthreads();
    best = red_v[0]; bi = red_i[0];
#pragma unroll
    for (int j = 1; j < 16; ++j) {
        const float ov = red_v[j];
        const int oi = red_i[j];
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
}

// The row's normaliser: m = the largest entry and mi its first index, logS = log sum exp(x_i - m) -- per thread by ascending index, wave
// butterfly (6 levels), tree over the 16 wave sums (4 levels); expf / logf, no fast forms.  `finite`: m is a finite number (uniform over
// the workgroup); logS = 0 otherwise.  log softmax(row)[i] = (x_i - m) - logS.
__device__ __forceinline__ void logprob_norm(const float* __restrict__ row, int vocab, float* red_v, int* red_i, float* red_s, float& m, int& mi,
                                             float& logS, bool& finite) {
    logprob_next_best(row, vocab, true, 0.f, 0, red_v, red_i, m, mi, [](float x) { return x; });
    finite = m > -INFINITY && m < INFINITY;
    logS = 0.f;
    if (finite) {
        float s = 0.f;
        const float mm = m;
        logprob_visit(row, vocab, [&](float v, int) { s += expf(v - mm); });
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) red_s[threadIdx.x >> 6] = s;
        __syncthreads();
        logS = logf(group_sum<16>(red_s[threadIdx.x & 15]));
    }
}

}  // namespace teo
