// Document join (isp_tts_amd/longform.py): the sentences of a padded batch put back together per document, in reading order,
// with pauses, crossfades and fades, in two launches and without a host read.  include/ispk.h has the definition (ov, adv,
// off, the ramps h and t, the weights); the names below are its names.
//
//   join_plan_kernel   ONE workgroup of max(B, D) threads rounded up to whole waves, thread i = item i.  (doc, pos, n, start, pause) of every item go to LDS;
//                      an item's rank among the valid ones is the count of items whose key (doc, pos, b) is smaller - B
//                      broadcast reads per thread, at most 2^20 integer compares in all.  Thread r then owns the item at sorted
//                      position r: overlap and advance from its successor, its offset by walking back to the first item of its
//                      document (integer sums: the order changes nothing), the ramps from its predecessor's overlap.  Thread d
//                      finds document d's item range by two binary searches over the sorted document ids.  Integers only, no
//                      atomics, every output word written by one thread.
//   join_kernel        grid (ceil(S_out / 4096), D), 256 threads.  A workgroup copies its document's item range of the plan
//                      into LDS and finds by binary search the items k0 .. k1 whose offsets bracket its tile.  Only the last
//                      item k that starts at or before a sample, and k - 1, can cover it (an item ends no later than its second
//                      successor starts, since ov <= n / 2 on both sides).  With fewer than 8 items under the tile - sentences
//                      are longer than tiles - they are visited one by one in document order with the plan entry in
//                      registers, 8 loads of a thread in flight at a time (the index clamped into the item, so that the load
//                      needs no condition); otherwise every sample searches its k in [k0, k1].  Either way a sample is the product
//                      (g w) x of the one item, or the sum of the two in document order, by one shared expression; contraction
//                      is off.  Each lane loads and stores one float per trip (consecutive lanes, consecutive samples: the
//                      source offset of an item is arbitrary, so wider accesses would not be aligned).
// Both are pure functions of their inputs: a document's bits depend on its own items alone, not on B, on the other documents
// or on the order of the items in b (ties in (doc, pos) apart), and repeated calls and graph replays repeat theirs.
//
// The plan, int64 / int32 words at strides of 1024 entries (ispk_join_plan_bytes() = 36,864 B), per sorted position r:
//   off int64 | item (b) | n | s | h | t    and per document d:  first sorted position | item count
//
// gfx950 resources (csrc/resource_report.py join.hip; no spills, no scratch):
//   join_plan_kernel   18 VGPRs, LDS 57,344 B static
//   join_kernel        90 VGPRs, LDS 32,768 B static
#include "common.h"

namespace {

constexpr int kJoinMax = 1024;                     // items and documents per call
constexpr int kJoinTile = 4096;                    // output samples per workgroup: 16 per thread, in 2 groups of 8
constexpr int kJoinThreads = 256;
constexpr int kJoinMaxFade = 1 << 23;
constexpr int kJoinLoopItems = 8;                  // up to this many items under a tile are visited one by one

struct JoinPlan {
    int64_t off[kJoinMax];
    int item[kJoinMax], n[kJoinMax], s[kJoinMax], h[kJoinMax], t[kJoinMax];
    int doc_first[kJoinMax], doc_count[kJoinMax];
};
static_assert(sizeof(JoinPlan) == 36864, "the plan's layout is part of the header's description");

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the first r in [0, n) with a[r] >= v (n when there is none)
__device__ __forceinline__ int lower_bound(const int* a, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kJoinMax) void join_plan_kernel(const int64_t* __restrict__ audio_len, const int64_t* __restrict__ doc,
                                                            const int64_t* __restrict__ pos, const int64_t* __restrict__ pause,
                                                            const int64_t* __restrict__ bounds, JoinPlan* __restrict__ plan,
                                                            int64_t* __restrict__ item_offset, int64_t* __restrict__ item_len,
                                                            int64_t* __restrict__ doc_len, int64_t* __restrict__ wanted_len,
                                                            int B, int S, int D, int S_out, int fade) {
    __shared__ int64_t pos_s[kJoinMax], pause_s[kJoinMax], adv_s[kJoinMax], off_s[kJoinMax];
    __shared__ int doc_s[kJoinMax], n_s[kJoinMax], start_s[kJoinMax], order[kJoinMax], ov_s[kJoinMax], sdoc_s[kJoinMax];
    const int i = threadIdx.x;
    int n = 0, start = 0, dc = -1;
    int64_t ps = 0, pz = 0;
    if (i < B) {
        const int64_t al = audio_len[i], len = (al >= 0 && al <= S) ? al : 0;
        int64_t s0 = 0, e0 = len;
        if (bounds) {
            s0 = clamp64(bounds[2 * i], 0, len);
            e0 = clamp64(bounds[2 * i + 1], s0, len);
        }
        n = (int)(e0 - s0);
        start = (int)s0;
        const int64_t d = doc[i];
        dc = (d >= 0 && d < D) ? (int)d : -1;
        ps = pos[i];
        pz = pause ? pause[i] : 0;
    }
    doc_s[i] = dc; pos_s[i] = ps; pause_s[i] = pz; n_s[i] = n; start_s[i] = start;
    __syncthreads();

    // rank by counting: every thread reads the same j (an LDS broadcast)
    int rank = 0, nvalid = 0;
#pragma unroll 8
    for (int j = 0; j < B; ++j) {                                          // (no branch: eight pairs of reads in flight)
        const int dj = doc_s[j];
        const int64_t pj = pos_s[j];
        const bool valid = dj >= 0;
        nvalid += valid ? 1 : 0;
        rank += (valid && (dj < dc || (dj == dc && (pj < ps || (pj == ps && j < i))))) ? 1 : 0;
    }
    if (dc >= 0) order[rank] = i;
    else if (i < B) { item_offset[i] = -1; item_len[i] = 0; }
    __syncthreads();

    // sorted position r = i: overlap and advance
    const int r = i;
    int b = -1, nb = 0, ov = 0, dr = INT32_MAX;
    int64_t adv = 0;
    if (r < nvalid) {
        b = order[r];
        dr = doc_s[b];
        nb = n_s[b];
        const int64_t p = pause_s[b];
        if (p >= 0) {
            adv = (int64_t)nb + (p < S_out ? p : (int64_t)S_out);
        } else {
            if (r + 1 < nvalid && doc_s[order[r + 1]] == dr) {
                const int64_t want = p < -(int64_t)INT32_MAX ? (int64_t)INT32_MAX : -p;
                const int half = nb / 2, half_next = n_s[order[r + 1]] / 2;
                const int m = half < half_next ? half : half_next;
                ov = want < m ? (int)want : m;
            }
            adv = nb - ov;
        }
    }
    sdoc_s[r] = dr; ov_s[r] = ov; adv_s[r] = adv;
    __syncthreads();

    if (r < nvalid) {
        int64_t off = 0;
        int k = r;
        while (k > 0 && sdoc_s[k - 1] == dr) { --k; off += adv_s[k]; }     // k ends at the document's first item
        off_s[r] = off;
        const int fd = fade < nb / 2 ? fade : nb / 2;
        const int ov_prev = r > k ? ov_s[r - 1] : 0;
        plan->off[r] = off;
        plan->item[r] = b;
        plan->n[r] = nb;
        plan->s[r] = start_s[b];
        plan->h[r] = ov_prev > 0 ? ov_prev : fd;
        plan->t[r] = ov > 0 ? ov : fd;
        item_offset[b] = off;
        item_len[b] = nb;
    }
    __syncthreads();

    if (i < D) {
        const int lo = lower_bound(sdoc_s, nvalid, i), hi = lower_bound(sdoc_s, nvalid, i + 1);
        const int64_t wanted = hi > lo ? off_s[hi - 1] + adv_s[hi - 1] : 0;
        plan->doc_first[i] = lo;
        plan->doc_count[i] = hi - lo;
        wanted_len[i] = wanted;
        doc_len[i] = wanted < S_out ? wanted : (int64_t)S_out;
    }
}

__global__ __launch_bounds__(kJoinThreads) void join_kernel(const float* __restrict__ audio, int64_t ld_audio,
                                                           const float* __restrict__ gain, const JoinPlan* __restrict__ plan,
                                                           const int64_t* __restrict__ doc_len, float* __restrict__ out,
                                                           int64_t ld_out, int S_out) {
#pragma clang fp contract(off)   // a sample is the rounded products and their rounded sum, as the header defines it
    __shared__ int64_t off_s[kJoinMax];
    __shared__ int item_s[kJoinMax], n_s[kJoinMax], s_s[kJoinMax], h_s[kJoinMax], t_s[kJoinMax];
    __shared__ float g_s[kJoinMax];
    const int d = blockIdx.y, tid = threadIdx.x;
    const int64_t o0 = (int64_t)blockIdx.x * kJoinTile;
    const int64_t oend = o0 + kJoinTile < S_out ? o0 + kJoinTile : (int64_t)S_out;
    float* __restrict__ orow = out + (int64_t)d * ld_out;
    const int64_t dl = doc_len[d];
    const int first = plan->doc_first[d], count = plan->doc_count[d];       // (three loads in one round trip)
    if (o0 >= dl) {                                                        // (uniform) behind the document: silence
        for (int64_t o = o0 + tid; o < oend; o += kJoinThreads) orow[o] = 0.f;
        return;
    }                                                                      // from here count >= 1: dl > 0
    for (int k = tid; k < count; k += kJoinThreads) {
        const int b = plan->item[first + k];
        off_s[k] = plan->off[first + k];
        item_s[k] = b;
        n_s[k] = plan->n[first + k];
        s_s[k] = plan->s[first + k];
        h_s[k] = plan->h[first + k];
        t_s[k] = plan->t[first + k];
        g_s[k] = gain ? gain[b] : 1.0f;
    }
    __syncthreads();

    // the last item that starts at or before `o`, searched in [lo, hi] (off_s[lo] <= o holds: off_s[0] = 0)
    auto last_at = [&](int64_t o, int lo, int hi) {
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off_s[mid] <= o) lo = mid; else hi = mid - 1;
        }
        return lo;
    };
    // (g w) x of a sample: the one expression of both paths below
    auto term = [&](int64_t n, int64_t h, int64_t t, float g, float x, int64_t i) {
        const float head = i < h ? (float)(2 * i + 1) / (float)(2 * h) : 1.0f;
        const float tail = i >= n - t ? (float)(2 * (n - 1 - i) + 1) / (float)(2 * t) : 1.0f;
        const float w = head * tail;
        const float gw = g * w;
        return gw * x;
    };
    auto source = [&](int k) { return audio + ((int64_t)item_s[k] * ld_audio + s_s[k]); };
    const int64_t lim = oend < dl ? oend : dl;                             // samples at or past it are silence
    const int k0 = last_at(o0, 0, count - 1), k1 = last_at(lim - 1, k0, count - 1);
    const int ka = k0 > 0 ? k0 - 1 : 0;                                    // the first item that can reach into the tile
    if (k1 - ka < kJoinLoopItems) {
        // Few items under the tile (the usual case: sentences are longer than tiles): item by item in document order, the
        // item's plan entry in registers, every thread its 8 samples.  Only the items k - 1 and k of the path below can
        // cover a sample, so both paths add the same terms in the same order.
        constexpr int kPer = kJoinTile / kJoinThreads, kGroup = 8;
        float v[kPer];
        unsigned covered = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) v[j] = 0.f;
        for (int k = ka; k <= k1; ++k) {                                   // (uniform)
            const int64_t off = off_s[k], n = n_s[k], h = h_s[k], t = t_s[k];
            if (n == 0) continue;
            const float g = g_s[k];
            const float* __restrict__ src = source(k);
#pragma unroll
            for (int jj = 0; jj < kPer; jj += kGroup) {
                const int64_t g0 = o0 + jj * kJoinThreads, g1 = g0 + kGroup * kJoinThreads;
                if (off >= g1 || off + n <= g0 || g0 >= lim) continue;     // (uniform) the item misses these 2,048 samples
                // eight loads in flight: the index is clamped into the item, so the load needs no condition
                float x[kGroup];
#pragma unroll
                for (int u = 0; u < kGroup; ++u) {
                    const int64_t i = g0 + u * kJoinThreads + tid - off;
                    x[u] = src[i < 0 ? 0 : (i >= n ? n - 1 : i)];
                }
#pragma unroll
                for (int u = 0; u < kGroup; ++u) {
                    const int j = jj + u;
                    const int64_t o = g0 + u * kJoinThreads + tid, i = o - off;
                    if (o < lim && i >= 0 && i < n) {
                        const float y = term(n, h, t, g, x[u], i);
                        v[j] = (covered >> j & 1u) ? v[j] + y : y;
                        covered |= 1u << j;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int64_t o = o0 + j * kJoinThreads + tid;
            if (o < oend) orow[o] = v[j];
        }
        return;
    }
    // Many short items under one tile: per sample, the last item that starts at or before it.
    for (int64_t o = o0 + tid; o < oend; o += kJoinThreads) {
        float v = 0.f;
        if (o < dl) {
            const int k = last_at(o, k0, k1);
            bool have = false;
            if (k > 0) {
                const int64_t i = o - off_s[k - 1];
                if (i < n_s[k - 1]) { v = term(n_s[k - 1], h_s[k - 1], t_s[k - 1], g_s[k - 1], source(k - 1)[i], i); have = true; }
            }
            const int64_t i = o - off_s[k];
            if (i < n_s[k]) {
                const float x = term(n_s[k], h_s[k], t_s[k], g_s[k], source(k)[i], i);
                v = have ? v + x : x;
            }
        }
        orow[o] = v;
    }
}

}  // namespace

extern "C" int32_t ispk_join_tile_samples(void) { return kJoinTile; }
extern "C" int32_t ispk_join_plan_bytes(void) { return (int32_t)sizeof(JoinPlan); }

extern "C" int32_t ispk_join_plan(const int64_t* audio_len, const int64_t* doc, const int64_t* pos, const int64_t* pause,
                                  const int64_t* bounds, void* plan, int64_t plan_bytes, int64_t* item_offset, int64_t* item_len,
                                  int64_t* doc_len, int64_t* wanted_len, int32_t B, int32_t S, int32_t D, int32_t S_out,
                                  int32_t fade, ispk_stream_t stream) {
    ISPK_REQUIRE(audio_len && doc && pos && plan && item_offset && item_len && doc_len && wanted_len, ISPK_E_NULL,
                 "ispk_join_plan: null pointer");
    ISPK_REQUIRE(B >= 0 && B <= kJoinMax && D >= 1 && D <= kJoinMax && S >= 0 && S_out >= 0, ISPK_E_SHAPE,
                 "ispk_join_plan: bad shape B=%d D=%d S=%d S_out=%d (B, D <= 1024)", B, D, S, S_out);
    ISPK_REQUIRE(fade >= 0 && fade < kJoinMaxFade, ISPK_E_SHAPE, "ispk_join_plan: fade %d outside [0, 2^23)", fade);
    ISPK_REQUIRE(plan_bytes >= (int64_t)sizeof(JoinPlan), ISPK_E_SHAPE, "ispk_join_plan: plan of %lld B, %zu needed",
                 (long long)plan_bytes, sizeof(JoinPlan));
    ISPK_REQUIRE(ispk_aligned(plan, 16), ISPK_E_ALIGN, "ispk_join_plan: the plan must be 16-byte aligned");
    if (B == 0) return 0;
    const int threads = ((B > D ? B : D) + 63) / 64 * 64;                  // thread i: item i, sorted position i, document i
    hipLaunchKernelGGL(join_plan_kernel, dim3(1), dim3(threads), 0, reinterpret_cast<hipStream_t>(stream), audio_len, doc, pos,
                       pause, bounds, static_cast<JoinPlan*>(plan), item_offset, item_len, doc_len, wanted_len, B, S, D, S_out,
                       fade);
    return ispk_launch_status();
}

extern "C" int32_t ispk_join_f32(const float* audio, int64_t ld_audio, const float* gain, const void* plan, const int64_t* doc_len,
                                 float* out, int64_t ld_out, int32_t B, int32_t S, int32_t D, int32_t S_out,
                                 ispk_stream_t stream) {
    ISPK_REQUIRE(audio && plan && doc_len && out, ISPK_E_NULL, "ispk_join_f32: null pointer");
    ISPK_REQUIRE(B >= 0 && B <= kJoinMax && D >= 1 && D <= kJoinMax && S >= 0 && S_out >= 0, ISPK_E_SHAPE,
                 "ispk_join_f32: bad shape B=%d D=%d S=%d S_out=%d (B, D <= 1024)", B, D, S, S_out);
    ISPK_REQUIRE(ld_audio >= S && ld_out >= S_out, ISPK_E_SHAPE,
                 "ispk_join_f32: row strides ld_audio=%lld ld_out=%lld shorter than the rows (S=%d, S_out=%d)", (long long)ld_audio,
                 (long long)ld_out, S, S_out);
    ISPK_REQUIRE(ispk_aligned(plan, 16), ISPK_E_ALIGN, "ispk_join_f32: the plan must be 16-byte aligned");
    if (B == 0 || S_out == 0) return 0;
    hipLaunchKernelGGL(join_kernel, dim3((unsigned)(((int64_t)S_out + kJoinTile - 1) / kJoinTile), D), dim3(kJoinThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), audio, ld_audio, gain, static_cast<const JoinPlan*>(plan), doc_len, out,
                       ld_out, S_out);
    return ispk_launch_status();
}
