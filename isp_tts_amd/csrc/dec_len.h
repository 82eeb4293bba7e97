// The decoder length of one utterance from its durations, as the two length regulators report it - shared by them
// (glue.hip, hard_duration.hip) and by the per-item infer kernel (aligner.hip), whose frames_wanted is that length without a clamp.
#pragma once
#include "common.h"

namespace {

constexpr int64_t kHdRepMax = 1 << 30;      // one token's repeats are cut here (sums of 512 of them stay inside int64 by far)

// reps of token l.  kRound: the regulator's (float(dur) + 0.5) truncated (:423); otherwise the plain integer duration (the
// averager's cumsum, :451).  Negative and NaN durations - outside both operators' domain - count as 0, so that every index
// derived from the sums stays inside the arrays.
template <bool kRound>
__device__ __forceinline__ int64_t hd_reps(const float* __restrict__ dur_f, const int64_t* __restrict__ dur_i, int64_t idx) {
#pragma clang fp contract(off)
    if (dur_f || kRound) {
        const float f = (dur_f ? dur_f[idx] : (float)dur_i[idx]) + (kRound ? 0.5f : 0.0f);
        return f >= 1.0f ? (int64_t)fminf(f, (float)kHdRepMax) : 0;       // (NaN compares false)
    }
    const int64_t d = dur_i[idx];
    return d < 0 ? 0 : (d > kHdRepMax ? kHdRepMax : d);
}

// The soft regulator's length: the fp32 sum of dur[0 .. L) taken sequentially in index order (what a CPU reduction over <= a
// few hundred values does), continued from `s`; one thread calls it.  kCum: cum[t + 1] = the sum through token t.
template <bool kCum>
__device__ __forceinline__ float soft_dur_sum(const float* __restrict__ dur, int L, float s, float* __restrict__ cum) {
    for (int t = 0; t < L; ++t) {
        s += dur[t];
        if constexpr (kCum) cum[t + 1] = s;
    }
    return s;
}
__device__ __forceinline__ int64_t soft_dec_len(float s) {
#pragma clang fp contract(off)
    return (int64_t)(s + 0.5f);
}

}  // namespace
