// Word-level prosody (isp_tts_amd/longform.py): a per-token gain envelope on the items' waveforms, one launch, no atomics, no
// host read.  include/ispk.h has the definition (live tokens, the ramp half-width h, the weight w); the names below are its names.
//
//   gain_envelope_kernel   grid (ceil(S / 4096), B), 256 threads; a workgroup owns 4,096 samples of one item, every lane four
//                      groups of four consecutive samples (one 16-byte load and store each; consecutive lanes, consecutive
//                      groups).  The loads are issued first, so that their latency covers what follows.  The tokens' ends,
//                      clamped to the length and with a dead token counting as +infinity, do not decrease.  Four searches
//                      over them in global memory find the tokens kf and kl that hold the tile's first and last sample, the
//                      live token before kf and the live token after kl.  With more than 256 tokens every wave runs them 64
//                      probes wide (a round cuts the range into 64 pieces, one probe per lane and a ballot: two rounds for
//                      4,096 tokens; two searches share a round) - six dependent round trips.  With up to 256 tokens a wave
//                      loads every end and gain once, four a lane, and the searches become counts of ballots: one round trip.
//                      Either way only the range of ends and gains from that predecessor to that successor, and no
//                      other mark, goes to LDS.  A lane then finds the token of a sample by binary search in LDS, its live
//                      neighbours by two more (zero-length tokens between two live ones share an end, so "the first end >= my
//                      start" and "the first end > my end" are the neighbours), and keeps the token's constants in registers
//                      until a sample leaves it: with tokens longer than four samples that is one look-up per group.
//                      Contraction is off; a sample is one product with e, e = g or g_j + (g_k - g_j) w.
// A row is taken 16 bytes at a time when both bases are 16-byte aligned and both strides are multiples of four; a group that
// crosses the item's length (loads) or the row's end (stores) and every other row go one float at a time.  Marks that do not
// tile give searches that end anywhere inside [0, L): every index is formed inside the staged range, so nothing outside the
// item's rows is touched.  An item's bits depend on that item alone, and `out` may be `audio`: a lane reads its sixteen
// samples before it writes them, and no other lane touches them.
//
// gfx950 resources (csrc/resource_report.py prosody.hip; no spills, no scratch): 56 VGPRs, no static LDS, 8 L bytes of dynamic
// LDS (1 KB at 128 tokens, 32 KB at 4,096).  Inside a captured graph, 64 items of 131,072 samples with 128 tokens each and ramp
// 128 (tools/time_prosody.py): 26.5 us, 2.5 times the 10.7 us that 67 MB take at 6.3 TB/s; DESIGN.md 4.26 says what was tried.
#include "common.h"

namespace {

constexpr int kGainMaxL = 4096;                    // tokens per item (the marks' limit)
constexpr int kGainTile = 4096;                    // samples per workgroup: 16 per thread
constexpr int kGainThreads = 256;
constexpr int kGainSmallL = 256;                   // up to this many tokens a wave holds all ends in registers
constexpr int kGainGroups = kGainTile / (4 * kGainThreads);
constexpr int kGainMaxRamp = 1 << 22;              // 4 h stays below 2^24: (2 i + 1) and 4 h are exact in fp32
constexpr uint32_t kGainDead = 0xFFFFFFFFu;        // the staged end of a dead token: above every length

// what a sample needs of the token that holds it: valid for n in [s, e)
struct GainToken {
    int64_t s, e;                                  // the token's range (the tail: [E, len))
    int hl, hr;                                    // ramp half-widths at its start and end (0: none)
    float g, gl, gr;                               // its gain, the live predecessor's and the live successor's
};

__global__ __launch_bounds__(kGainThreads) void gain_envelope_kernel(const float* audio, int64_t ld_audio,
                                                                    const int64_t* __restrict__ audio_len,
                                                                    const int64_t* __restrict__ token_marks,
                                                                    const float* __restrict__ token_gain, float* out,
                                                                    int64_t ld_out, int L, int S, int ramp, int vec) {
#pragma clang fp contract(off)   // e is the rounded product plus the rounded sum, a sample the rounded product with e
    extern __shared__ uint32_t gain_lds[];                                 // 8 L bytes: what the tile's tokens can need at most
    uint32_t* end_s = gain_lds;
    float* g_s = reinterpret_cast<float*>(gain_lds + L);
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int64_t n0 = (int64_t)blockIdx.x * kGainTile;
    const int64_t al = audio_len[b], len = (al >= 0 && al <= S) ? al : 0;
    const float* arow = audio + (int64_t)b * ld_audio;
    float* orow = out + (int64_t)b * ld_out;

    // the lane's samples, before anything else: nothing at or past len is read
    float x[kGainGroups][4];
#pragma unroll
    for (int u = 0; u < kGainGroups; ++u) {
        const int64_t n = n0 + 4 * (u * kGainThreads + tid);
        if (vec && n + 4 <= len) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(arow + n);
            x[u][0] = v[0]; x[u][1] = v[1]; x[u][2] = v[2]; x[u][3] = v[3];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) x[u][i] = n + i < len ? arow[n + i] : 0.0f;
        }
    }

    int cnt = 0;                                                           // staged tokens [a, a + cnt)
    int64_t before = 0;                                                    // the end in front of token a
    if (n0 < len) {                                                        // (uniform) else the tile is silence
        const int64_t n1 = n0 + kGainTile < len ? n0 + kGainTile : len;
        const int64_t* __restrict__ mrow = token_marks + (int64_t)b * L * 2;
        // the end of token l as the searches see it (l in [0, L))
        auto end_of = [&](int l) -> int64_t {
            const int64_t s = mrow[2 * (int64_t)l], e = mrow[2 * (int64_t)l + 1];
            return (s < 0 || e < 0) ? INT64_MAX : (e < len ? e : len);
        };
        // Two searches in lockstep, each wave for itself: the first l in [lo, hi) with end > t, hi when there is none.  A
        // round cuts the range into 64 pieces, lane c probes the last token of piece c, and the first lane that sees a larger
        // end names the piece: 4,096 tokens take two rounds, and the two loads of a round are in flight together.
        auto search2 = [&](int lo1, int hi1, int64_t t1, int lo2, int hi2, int64_t t2, int& r1, int& r2) {
            while (lo1 < hi1 || lo2 < hi2) {                               // (uniform: the ballots are)
                const int s1 = (hi1 - lo1 + 63) >> 6, s2 = (hi2 - lo2 + 63) >> 6;
                int i1 = lo1 + (lane + 1) * s1 - 1, i2 = lo2 + (lane + 1) * s2 - 1;
                i1 = i1 < hi1 ? i1 : hi1 - 1;
                i2 = i2 < hi2 ? i2 : hi2 - 1;
                const int64_t v1 = end_of(i1 < 0 ? 0 : i1), v2 = end_of(i2 < 0 ? 0 : i2);      // (an empty range: any token)
                const unsigned long long m1 = __ballot(v1 > t1), m2 = __ballot(v2 > t2);
                if (lo1 < hi1) {
                    if (m1 == 0) {
                        lo1 = hi1;
                    } else {
                        const int f = __ffsll(m1) - 1, last = lo1 + (f + 1) * s1 - 1;
                        hi1 = last < hi1 ? last : hi1 - 1;                 // its end is larger: the answer if no earlier one is
                        lo1 += f * s1;
                    }
                }
                if (lo2 < hi2) {
                    if (m2 == 0) {
                        lo2 = hi2;
                    } else {
                        const int f = __ffsll(m2) - 1, last = lo2 + (f + 1) * s2 - 1;
                        hi2 = last < hi2 ? last : hi2 - 1;
                        lo2 += f * s2;
                    }
                }
            }
            r1 = lo1;
            r2 = lo2;
        };
        const float* __restrict__ grow = token_gain + (int64_t)b * L;
        if (L <= kGainSmallL) {
            // Up to 256 tokens: a wave holds every end (and gain) in four registers a lane, ONE round trip behind the
            // samples' loads.  The ends do not decrease, so "the first l with end > t" is the count of ends <= t - ballots
            // and popcounts - and an end that a later step needs comes from its lane by a shuffle.
            int64_t v[kGainSmallL / 64];
            float gv[kGainSmallL / 64];
#pragma unroll
            for (int j = 0; j < kGainSmallL / 64; ++j) {
                const int l = lane + 64 * j;
                v[j] = l < L ? end_of(l) : INT64_MAX;
                gv[j] = l < L ? grow[l] : 0.0f;
            }
            auto count = [&](int64_t t, bool or_equal) {                  // tokens with end < t, or <= t
                int c = 0;
#pragma unroll
                for (int j = 0; j < kGainSmallL / 64; ++j)
                    c += __popcll(__ballot(lane + 64 * j < L && (or_equal ? v[j] <= t : v[j] < t)));
                return c;
            };
            auto value_at = [&](int t) {                                   // (uniform t in [0, L))
                int64_t pick = v[0];
#pragma unroll
                for (int j = 1; j < kGainSmallL / 64; ++j) pick = (t >> 6) == j ? v[j] : pick;
                return (int64_t)__shfl((long long)pick, t & 63, 64);
            };
            const int kf = count(n0, true);                                // the first l with end > n0
            int kl = count(n1 - 1, true);                                  // the first l with end >= n1
            kl = kl < kf ? kf : kl;
            const int64_t sf = kf > 0 ? value_at(kf - 1) : 0;
            const int64_t el = kl < L ? value_at(kl) : INT64_MAX;
            int a = kf > 0 ? count(sf, false) : 0;                         // the first l with end >= sf
            const int z = el != INT64_MAX ? count(el, true) : L;           // the first l with end > el
            const int last = el != INT64_MAX ? (z < L ? z : L - 1) : kl - 1;
            if (a > L - 1) a = L - 1;
            cnt = last >= a ? last - a + 1 : 0;
            before = a > 0 ? value_at(a - 1) : 0;
            if (tid < 64) {                                                // (every wave holds the same: one writes)
#pragma unroll
                for (int j = 0; j < kGainSmallL / 64; ++j) {
                    const int l = lane + 64 * j;
                    if (l >= a && l <= last) {                             // (last < L)
                        end_s[l - a] = v[j] == INT64_MAX ? kGainDead : (uint32_t)v[j];
                        g_s[l - a] = gv[j];
                    }
                }
            }
        } else {
            // kf: the first l with end > n0;  kl: the first l with end >= n1  (L when there is none)
            int kf, kl;
            search2(0, L, n0, 0, L, n1 - 1, kf, kl);
            kl = kl < kf ? kf : kl;
            const int64_t sf = kf > 0 ? end_of(kf - 1) : 0;                // where kf starts: its live predecessor ends there
            const int64_t el = kl < L ? end_of(kl) : INT64_MAX;
            // a: the first l in [0, kf) with end >= sf (kf when there is none);  z: the first l in (kl, L) with end > el
            int a, z;
            search2(0, kf, sf - 1, el != INT64_MAX ? kl + 1 : L, L, el, a, z);
            const int last = el != INT64_MAX ? (z < L ? z : L - 1) : kl - 1;      // the last token worth staging
            if (a > L - 1) a = L - 1;
            cnt = last >= a ? last - a + 1 : 0;                            // <= L <= kGainMaxL
            before = a > 0 ? end_of(a - 1) : 0;
            for (int t = tid; t < cnt; t += kGainThreads) {
                const int64_t e = end_of(a + t);
                end_s[t] = e == INT64_MAX ? kGainDead : (uint32_t)e;       // e <= len < 2^31
                g_s[t] = grow[a + t];
            }
        }
        if (before == INT64_MAX) before = 0;                               // (only marks that do not tile)
    }
    __syncthreads();

    // the first staged t with end > v, or >= v  (cnt when there is none; a dead token's end is above every v)
    auto first_gt = [&](int64_t v) {
        int lo = 0, hi = cnt;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)end_s[mid] > v) hi = mid; else lo = mid + 1;
        }
        return lo;
    };
    auto first_ge = [&](int64_t v) {
        int lo = 0, hi = cnt;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)end_s[mid] >= v) hi = mid; else lo = mid + 1;
        }
        return lo;
    };
    auto start_of = [&](int t) -> int64_t { return t > 0 ? (int64_t)end_s[t - 1] : before; };
    // the token that holds sample n (n < len)
    auto token_at = [&](int64_t n) {
        GainToken k;
        k.hl = k.hr = 0;
        k.gl = k.gr = k.g = 1.0f;
        k.e = len;
        const int t = first_gt(n);
        if (t >= cnt || end_s[t] == kGainDead) {                           // behind the last live token: it lends its gain
            k.s = t > 0 ? (int64_t)end_s[t - 1] : 0;
            if (t > 0 && k.s > 0) {
                const int j = first_ge(k.s);                               // j < t: end_s[t - 1] qualifies
                k.g = g_s[j];
            }
            return k;
        }
        k.s = start_of(t);
        k.e = (int64_t)end_s[t];
        k.g = g_s[t];
        const int64_t half = (k.e - k.s) / 2;
        if (k.s > 0) {
            const int j = first_ge(k.s);                                   // the live predecessor ends where t starts
            if (j < t) {
                const int64_t hj = ((int64_t)end_s[j] - start_of(j)) / 2;
                int64_t h = hj < half ? hj : half;
                h = h < ramp ? h : ramp;
                if (h > 0) { k.hl = (int)h; k.gl = g_s[j]; }
            }
        }
        const int m = first_gt(k.e);                                       // the live successor: the first end past t's
        if (m < cnt && end_s[m] != kGainDead) {
            const int64_t hm = ((int64_t)end_s[m] - k.e) / 2;
            int64_t h = hm < half ? hm : half;
            h = h < ramp ? h : ramp;
            if (h > 0) { k.hr = (int)h; k.gr = g_s[m]; }
        }
        return k;
    };
    auto envelope = [&](const GainToken& k, int64_t n) {
        if (n < k.s + k.hl) {
            const int64_t i = n - k.s + k.hl;
            const float w = (float)(2 * i + 1) / (float)(4 * (int64_t)k.hl);
            const float d = k.g - k.gl;
            const float dw = d * w;
            return k.gl + dw;
        }
        if (n >= k.e - k.hr) {
            const int64_t i = n - k.e + k.hr;
            const float w = (float)(2 * i + 1) / (float)(4 * (int64_t)k.hr);
            const float d = k.gr - k.g;
            const float dw = d * w;
            return k.g + dw;
        }
        return k.g;
    };

    GainToken k;
    k.s = 0; k.e = -1;                                                     // holds nothing yet
    k.hl = k.hr = 0;
    k.g = k.gl = k.gr = 1.0f;
#pragma unroll
    for (int u = 0; u < kGainGroups; ++u) {
        const int64_t n = n0 + 4 * (u * kGainThreads + tid);
        if (n >= S) break;
        float y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            y[i] = 0.0f;
            if (n + i < len) {
                if (n + i >= k.e || n + i < k.s) k = token_at(n + i);
                y[i] = x[u][i] * envelope(k, n + i);
            }
        }
        if (vec && n + 4 <= S) {
            f32x4 v;
            v[0] = y[0]; v[1] = y[1]; v[2] = y[2]; v[3] = y[3];
            *reinterpret_cast<f32x4*>(orow + n) = v;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (n + i < S) orow[n + i] = y[i];
        }
    }
}

}  // namespace

extern "C" int32_t ispk_gain_envelope_tile_samples(void) { return kGainTile; }

extern "C" int32_t ispk_gain_envelope_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len,
                                          const int64_t* token_marks, const float* token_gain, int32_t ramp, float* out,
                                          int64_t ld_out, int32_t B, int32_t L, int32_t S, ispk_stream_t stream) {
    ISPK_REQUIRE(audio && audio_len && token_marks && token_gain && out, ISPK_E_NULL, "ispk_gain_envelope_f32: null pointer");
    ISPK_REQUIRE(B >= 0 && B <= 65535 && L >= 1 && L <= kGainMaxL && S >= 0, ISPK_E_SHAPE,
                 "ispk_gain_envelope_f32: bad shape B=%d L=%d S=%d (B <= 65535, 1 <= L <= %d, 0 <= S < 2^31)", B, L, S, kGainMaxL);
    ISPK_REQUIRE(ld_audio >= S && ld_out >= S, ISPK_E_SHAPE,
                 "ispk_gain_envelope_f32: row strides ld_audio=%lld ld_out=%lld shorter than the rows (S=%d)", (long long)ld_audio,
                 (long long)ld_out, S);
    ISPK_REQUIRE(ramp >= 0 && ramp < kGainMaxRamp, ISPK_E_SHAPE, "ispk_gain_envelope_f32: ramp %d outside [0, 2^22)", ramp);
    if (B == 0 || S == 0) return 0;
    if (!(out == audio && (ld_out == ld_audio || B == 1))) {               // in place, or apart
        const uintptr_t a0 = (uintptr_t)audio, o0 = (uintptr_t)out;
        const uintptr_t a1 = a0 + 4 * ((uintptr_t)(B - 1) * (uintptr_t)ld_audio + (uintptr_t)S);
        const uintptr_t o1 = o0 + 4 * ((uintptr_t)(B - 1) * (uintptr_t)ld_out + (uintptr_t)S);
        ISPK_REQUIRE(a1 <= o0 || o1 <= a0, ISPK_E_SHAPE,
                     "ispk_gain_envelope_f32: out overlaps audio without being audio (same base and row stride)");
    }
    const int vec = ispk_aligned(audio, 16) && ispk_aligned(out, 16) && ld_audio % 4 == 0 && ld_out % 4 == 0;
    hipLaunchKernelGGL(gain_envelope_kernel, dim3((unsigned)(((int64_t)S + kGainTile - 1) / kGainTile), B), dim3(kGainThreads),
                       8 * (size_t)L,
                       reinterpret_cast<hipStream_t>(stream), audio, ld_audio, audio_len, token_marks, token_gain, out, ld_out, L, S,
                       ramp, vec);
    return ispk_launch_status();
}
