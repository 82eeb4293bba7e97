// Speech marks (isp_tts_amd/longform.py): the sample range of every token and word of an item, in the item's own audio or in
// its joined document - from the durations the regulator consumed, the vocoder's lengths, a conditioner's bounds and the
// join's outputs, in one launch and without a host read.  include/ispk.h has the definition (steps 1 .. 6, the clamps and
// their order); the names below are its names.
//
//   speech_marks_kernel<kRound>   grid B, 256 threads, one workgroup per item.  The item's scalars (lengths, bounds, offset,
//                      document) are uniform loads.  The n + 1 cumulative values go to LDS: soft, the clamped durations are
//                      staged in LDS by all threads and ONE thread adds them in token order with soft_dur_sum<true> - the
//                      regulator's fp32 sequence bit for bit, which is the contract, so the loop is not parallelised; hard,
//                      the integer repeats (hd_reps<true>) by a shuffle scan inside each wave and the wave totals through
//                      LDS, as hard_duration.hip scans them, kept in int64.  Every thread then maps its tokens' two
//                      boundaries through steps 1 .. 6 (the map is monotone, so starts <= ends and consecutive tokens tile)
//                      and stores the pair; a word's (min start, max end) are 64-bit LDS minima / maxima - order-free, so the
//                      bits do not depend on the schedule - written out by thread w.  Plain vector stores, no global atomics.
//
// gfx950 resources (csrc/resource_report.py marks.hip; no spills, no scratch): soft 29 VGPRs, LDS 49,184 B static; hard 34 VGPRs,
// LDS 49,216 B.  Inside a captured graph, 64 items with 64 words and every optional input (tools/time_longform.py): 3.9 us at
// 32 tokens in both modes; at 4,096 tokens 25.9 us hard and 59.8 us soft - there the one-thread sum is more than half.
#include "common.h"
#include "dec_len.h"

namespace {

constexpr int kMarksMaxL = 4096;                   // tokens per item
constexpr int kMarksMaxW = 1024;                   // words per item
constexpr int kMarksMaxD = 1024;                   // documents (the join's limit)
constexpr int kMarksMaxHop = 1 << 20;
constexpr int kMarksThreads = 256;
constexpr int kMarksDurAt = kMarksMaxL + 4;        // soft: the staged durations follow the kMarksMaxL + 1 fp32 sums

__device__ __forceinline__ int64_t marks_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool kRound>
__global__ __launch_bounds__(kMarksThreads) void speech_marks_kernel(
    const float* __restrict__ duration, int64_t ld_duration, const int64_t* __restrict__ text_len,
    const int64_t* __restrict__ audio_len, const int64_t* __restrict__ bounds, const int64_t* __restrict__ item_offset,
    const int64_t* __restrict__ doc, const int64_t* __restrict__ doc_len, const int64_t* __restrict__ doc_bounds,
    const int64_t* __restrict__ word_id, int64_t* __restrict__ token_marks, int64_t* __restrict__ word_marks, int hop, int L, int S,
    int D, int W) {
#pragma clang fp contract(off)
    // hard: C_t int64 [n + 1].  soft: s_t fp32 [n + 1] in the first half, d'_t fp32 [n] from float kMarksDurAt on
    __shared__ int64_t cum_i[kMarksMaxL + 4];
    __shared__ int64_t w_lo[kMarksMaxW], w_hi[kMarksMaxW];
    __shared__ int64_t wave_tot[kMarksThreads / 64];
    static_assert((kMarksDurAt + kMarksMaxL) * sizeof(float) <= sizeof(cum_i), "the staged durations fit behind the sums");
    float* cum_f = reinterpret_cast<float*>(cum_i);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    const int64_t tl = text_len ? text_len[b] : (int64_t)L;
    int n = (tl >= 0 && tl <= L) ? (int)tl : 0;
    const int64_t al = audio_len[b], len = (al >= 0 && al <= S) ? al : 0;
    int64_t s_b = 0, e_b = len;
    if (bounds) {
        s_b = marks_clamp(bounds[2 * (int64_t)b], 0, len);
        e_b = marks_clamp(bounds[2 * (int64_t)b + 1], s_b, len);
    }
    int64_t off = 0, dl = 0, ds = 0, de = 0;
    if (item_offset) {                                                     // the join group (uniform)
        off = item_offset[b];
        const int64_t d = doc[b];
        if (off < 0 || d < 0 || d >= D) {
            n = 0;                                                         // dropped: every mark is -1
        } else {
            dl = doc_len[d];
            dl = dl < 0 ? 0 : dl;
            de = dl;
            if (doc_bounds) {
                ds = marks_clamp(doc_bounds[2 * d], 0, dl);
                de = marks_clamp(doc_bounds[2 * d + 1], ds, dl);
            }
        }
    }
    for (int w = tid; w < W; w += kMarksThreads) { w_lo[w] = INT64_MAX; w_hi[w] = -1; }

    const float* __restrict__ drow = duration + (int64_t)b * ld_duration;
    if constexpr (kRound) {
        if (tid == 0) cum_i[0] = 0;
        int64_t carry = 0;
        for (int base = 0; base < n; base += kMarksThreads) {              // (uniform trip count)
            const int l = base + tid;
            int64_t v = l < n ? hd_reps<true>(drow, nullptr, l) : 0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int64_t up = __shfl_up(v, o, 64);
                if (lane >= o) v += up;
            }
            if (lane == 63) wave_tot[wv] = v;
            __syncthreads();
            int64_t before = carry;
            for (int k = 0; k < wv; ++k) before += wave_tot[k];
            carry += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
            if (l < n) cum_i[l + 1] = v + before;
            __syncthreads();                                               // wave_tot is rewritten by the next trip
        }
    } else {
        float* dur_s = cum_f + kMarksDurAt;
        for (int l = tid; l < n; l += kMarksThreads) {
            const float d = drow[l];
            dur_s[l] = d > 0.0f ? d : 0.0f;                                // (NaN compares false)
        }
        __syncthreads();
        if (tid == 0) {
            cum_f[0] = 0.0f;
            soft_dur_sum<true>(dur_s, n, 0.0f, cum_f);
        }
    }
    __syncthreads();

    // boundary t in [0, n] -> its sample: steps 1 .. 6 of the header
    auto mark = [&](int t) -> int64_t {
        int64_t m;
        if constexpr (kRound) {
            m = (int64_t)hop * cum_i[t];                                   // < 2^20 * 2^12 * 2^30
        } else {
            const double v = (double)cum_f[t] * (double)hop + 0.5;         // >= 0.5: truncation is the floor
            m = v >= (double)(len + 1) ? len : (int64_t)v;
        }
        m = marks_clamp(m, 0, len);
        m = marks_clamp(m, s_b, e_b) - s_b;
        if (item_offset) {
            m = marks_clamp(m + off, 0, dl);
            m = marks_clamp(m, ds, de) - ds;
        }
        return m;
    };

    int64_t* __restrict__ trow = token_marks + (int64_t)b * L * 2;
    const int64_t* __restrict__ wrow = word_id ? word_id + (int64_t)b * L : nullptr;
    for (int t = tid; t < L; t += kMarksThreads) {
        int64_t a = -1, e = -1;
        if (t < n) {
            a = mark(t);
            e = mark(t + 1);
            if (wrow && W > 0) {
                const int64_t w = wrow[t];
                if (w >= 0 && w < W) {
                    __hip_atomic_fetch_min(&w_lo[w], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_max(&w_hi[w], e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        trow[2 * t] = a;
        trow[2 * t + 1] = e;
    }
    if (W > 0) {                                                           // (uniform; word_marks is not NULL then)
        __syncthreads();
        int64_t* __restrict__ orow = word_marks + (int64_t)b * W * 2;
        for (int w = tid; w < W; w += kMarksThreads) {
            const int64_t lo = w_lo[w];
            orow[2 * w] = lo == INT64_MAX ? -1 : lo;
            orow[2 * w + 1] = lo == INT64_MAX ? -1 : w_hi[w];
        }
    }
}

}  // namespace

extern "C" int32_t ispk_speech_marks(const float* duration, int64_t ld_duration, const int64_t* text_len, const int64_t* audio_len,
                                     const int64_t* bounds, const int64_t* item_offset, const int64_t* doc, const int64_t* doc_len,
                                     const int64_t* doc_bounds, const int64_t* word_id, int64_t* token_marks, int64_t* word_marks,
                                     int32_t hop, int32_t round, int32_t B, int32_t L, int32_t S, int32_t D, int32_t W,
                                     ispk_stream_t stream) {
    ISPK_REQUIRE(duration && audio_len && token_marks, ISPK_E_NULL, "ispk_speech_marks: null pointer");
    const bool joined = item_offset || doc || doc_len;
    ISPK_REQUIRE(!joined || (item_offset && doc && doc_len), ISPK_E_NULL,
                 "ispk_speech_marks: item_offset, doc and doc_len are given together or not at all");
    ISPK_REQUIRE(!doc_bounds || joined, ISPK_E_NULL, "ispk_speech_marks: doc_bounds without the join group");
    ISPK_REQUIRE(!(word_id && W > 0) || word_marks, ISPK_E_NULL, "ispk_speech_marks: word_id without word_marks");
    ISPK_REQUIRE(B >= 0 && B <= 65535 && L >= 0 && L <= kMarksMaxL && W >= 0 && W <= kMarksMaxW, ISPK_E_SHAPE,
                 "ispk_speech_marks: bad shape B=%d L=%d W=%d (B <= 65535, L <= %d, W <= %d)", B, L, W, kMarksMaxL, kMarksMaxW);
    ISPK_REQUIRE(W == 0 || word_marks, ISPK_E_NULL, "ispk_speech_marks: W=%d words without word_marks", W);
    ISPK_REQUIRE(hop >= 1 && hop <= kMarksMaxHop, ISPK_E_SHAPE, "ispk_speech_marks: hop %d outside [1, 2^20]", hop);
    ISPK_REQUIRE(S >= 0, ISPK_E_SHAPE, "ispk_speech_marks: S=%d outside [0, 2^31)", S);
    ISPK_REQUIRE(ld_duration >= L, ISPK_E_SHAPE, "ispk_speech_marks: row stride %lld shorter than the rows (L=%d)",
                 (long long)ld_duration, L);
    ISPK_REQUIRE(!joined || (D >= 1 && D <= kMarksMaxD), ISPK_E_SHAPE, "ispk_speech_marks: D=%d documents outside [1, %d]", D,
                 kMarksMaxD);
    if (B == 0 || L == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (round)
        hipLaunchKernelGGL(speech_marks_kernel<true>, dim3(B), dim3(kMarksThreads), 0, s, duration, ld_duration, text_len, audio_len,
                           bounds, item_offset, doc, doc_len, doc_bounds, word_id, token_marks, word_marks, hop, L, S, D, W);
    else
        hipLaunchKernelGGL(speech_marks_kernel<false>, dim3(B), dim3(kMarksThreads), 0, s, duration, ld_duration, text_len, audio_len,
                           bounds, item_offset, doc, doc_len, doc_bounds, word_id, token_marks, word_marks, hop, L, S, D, W);
    return ispk_launch_status();
}
