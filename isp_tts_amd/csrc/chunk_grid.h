// The 8,192-sample chunk grid: the time-domain machinery under the conditioner (condition.hip), the equalizer (equalizer.hip),
// the segmenter (segment.hip) and the noise profile (noise.hip).  This header is the only place that knows the grid and the
// order of the sums on it; what a kernel does with a chunk (a filter state, a scan, a plan) stays in its own file.
//
// Grid.  Fixed to sample 0 of every item: a chunk is kGridChunk = 32 samples = one lane, a segment kGridThreads = 256 chunks =
// 8,192 samples = one workgroup, grid (ceil(S / 8192), B).  A hop is 256 samples = eight lanes, a trim frame 1,024 samples =
// four hops.
//
// Banks.  The segment sits in LDS as 256 rows of kGridPad = 36 floats: the 16 lanes of a ds_read_b128 group then hit 16
// distinct bank quads (36 l mod 64 takes 16 values a multiple of 4 apart), where a stride of 32 would put them all on two.
// The four spare floats behind a chunk are the caller's (the equalizer keeps a section's entry state there).
//
// Bits.  The trim frames of the conditioner, the segmenter and the noise profile are one definition, this one: a lane adds the
// squares of its 32 samples in sample order with fma in float64 (chunk_square_sum), a hop is its eight lanes added in lane
// order (hop_fold), p_t = (((h_t + h_t+1) + h_t+2) + h_t+3) / 1024 over the hops that exist (frame_power), the threshold is
// ref * factor with ref the max of p_t or a constant (frame_threshold), and the ends follow from the first and last active
// frames (trim_start, trim_end).  Every value depends on the item's samples and length alone - not on B, the row stride, the
// alignment or the workgroup size of the kernel that asks - and the tests compare the three operators bit for bit.
//
// To change the grid, keep:
//   - kGridPad a multiple of 4 (rows are read and written as float4) with 16 consecutive rows on 16 distinct bank quads;
//   - kGridHop a multiple of kGridChunk and kGridSeg a multiple of kGridHop, so that a hop never straddles two workgroups and
//     the conditioner's `start`, a multiple of the hop, falls on a chunk boundary;
//   - the order of every sum above: a change moves the bits of all three operators together, and of their host references
//     (tests/*_host.py) with them.
#pragma once
#include <algorithm>

#include "common.h"

constexpr int kGridThreads = 256;
constexpr int kGridChunk = 32;                            // samples per lane
constexpr int kGridSeg = kGridThreads * kGridChunk;       // 8,192 samples per workgroup
constexpr int kGridPad = kGridChunk + 4;                  // LDS floats per chunk
constexpr int kGridHop = 256, kGridFrame = 1024;
constexpr int kGridHopChunks = kGridHop / kGridChunk;     // 8 lanes per hop
constexpr int kGridSegHops = kGridSeg / kGridHop;         // 32
static_assert(kGridPad % 4 == 0 && kGridChunk % 4 == 0, "chunk rows are read and written as float4");
static_assert(kGridHop % kGridChunk == 0 && kGridSeg % kGridHop == 0 && kGridFrame == 4 * kGridHop && kGridSegHops <= kGridThreads,
              "a hop is whole lanes of one workgroup, a frame four hops");

// xs[chunk c][k] = x(base + 32 c + k), 0 at or past len.  Nothing at or past len is read.  float4 loads where `vec` (the row
// base is 16-byte aligned; base is a multiple of 4) and the four samples lie below len, scalar loads near len.
__device__ __forceinline__ void stage_chunks(float* xs, const float* __restrict__ row, int64_t base, int64_t len, int vec, int tid) {
    for (int g = tid; g < kGridSeg / 4; g += kGridThreads) {
        const int64_t i = base + 4 * (int64_t)g;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (vec && i + 4 <= len) {
            v = *reinterpret_cast<const f32x4*>(row + i);
        } else {
            if (i < len) v.x = row[i];
            if (i + 1 < len) v.y = row[i + 1];
            if (i + 2 < len) v.z = row[i + 2];
            if (i + 3 < len) v.w = row[i + 3];
        }
        *reinterpret_cast<f32x4*>(xs + (g >> 3) * kGridPad + (g & 7) * 4) = v;
    }
}

// The chunk read-back: each(k, x) for the lane's 32 samples as doubles, in sample order (float4 reads, each consumed as it
// arrives: a caller that only folds the samples keeps four of them in registers, not 32).
template <typename F>
__device__ __forceinline__ void each_sample(const float* xs, int tid, F&& each) {
    const float* p = xs + tid * kGridPad;
#pragma unroll
    for (int k4 = 0; k4 < kGridChunk / 4; ++k4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * k4);
        const double xd[4] = {(double)v.x, (double)v.y, (double)v.z, (double)v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) each(4 * k4 + q, xd[q]);
    }
}
__device__ __forceinline__ void load_chunk(const float* xs, int tid, double x[kGridChunk]) {
    each_sample(xs, tid, [&](int k, double v) { x[k] = v; });
}
__device__ __forceinline__ double chunk_square_sum(const float* xs, int tid) {
    double e = 0.0;
    each_sample(xs, tid, [&](int, double v) { e = fma(v, v, e); });
    return e;
}

// Hop j of the segment from the lanes' square sums part[kGridThreads], in lane order (behind the barrier that follows the
// lanes' stores).
__device__ __forceinline__ double hop_fold(const double* part, int j) {
    double t = 0.0;
    for (int q = 0; q < kGridHopChunks; ++q) t += part[j * kGridHopChunks + q];
    return t;
}

// p_t of an item of nh hops (and frames)
__device__ __forceinline__ double frame_power(const double* hop, int t, int nh) {
    double p = hop[t];
    if (t + 1 < nh) p += hop[t + 1];
    if (t + 2 < nh) p += hop[t + 2];
    if (t + 3 < nh) p += hop[t + 3];
    return p / (double)kGridFrame;
}

// Max of one double per lane (any order gives the same bits); every lane gets it.  No barrier behind the read of red[0]: a
// caller that writes red again puts one first.
template <int kLanes>
__device__ __forceinline__ double block_max(double x, int tid, double* red) {
    red[tid] = x;
    __syncthreads();
    for (int s = kLanes / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    return red[0];
}

// The trim threshold from the lanes' maxima of p_t (how a kernel walks its frames is its own): ref * factor, ref = max_t p_t
// with `ref_is_max`.  block_max's barriers.
template <int kLanes>
__device__ __forceinline__ double frame_threshold(double lane_max, bool ref_is_max, double ref, double factor, int tid, double* red) {
    const double mx = block_max<kLanes>(lane_max, tid, red);
    return ref_is_max ? mx * factor : ref * factor;
}

// The first and last active frames from the lanes' own (0x7fffffff and -1 for a lane without one; last < 0: no active frame).
// ired: 2 kLanes ints.  Ends with a barrier.
template <int kLanes>
__device__ __forceinline__ void active_range(int& first, int& last, int tid, int* ired) {
    ired[tid] = first, ired[kLanes + tid] = last;
    __syncthreads();
    for (int s = kLanes / 2; s > 0; s >>= 1) {
        if (tid < s) {
            ired[tid] = min(ired[tid], ired[tid + s]);
            ired[kLanes + tid] = max(ired[kLanes + tid], ired[kLanes + tid + s]);
        }
        __syncthreads();
    }
    first = ired[0], last = ired[kLanes];
    __syncthreads();
}

// The trimmed item's ends from its first / last active frames and the padding in frames.
__device__ __forceinline__ int64_t trim_start(int first, int pad_frames) {
    return std::max<int64_t>(0, (int64_t)kGridHop * ((int64_t)first - pad_frames));
}
__device__ __forceinline__ int64_t trim_end(int last, int pad_frames, int64_t len) {
    return std::min<int64_t>(len, (int64_t)kGridHop * ((int64_t)last + pad_frames) + kGridFrame);
}

// Exclusive scan over the workgroup's lanes (Hillis-Steele in LDS), a sum or a max; `total` is the reduction over all lanes.
// `identity` is what lane 0 gets.  Ends with a barrier, after which buf is free again.
template <bool kMax, int kLanes>
__device__ __forceinline__ int block_scan_excl(int v, int identity, int tid, int* buf, int& total) {
#pragma unroll 1
    for (int k = 0; (1 << k) < kLanes; ++k) {
        buf[tid] = v;
        __syncthreads();
        const int src = tid - (1 << k);
        if (src >= 0) v = kMax ? max(v, buf[src]) : v + buf[src];
        __syncthreads();
    }
    buf[tid] = v;
    __syncthreads();
    const int excl = tid ? buf[tid - 1] : identity;
    total = buf[kLanes - 1];
    __syncthreads();
    return excl;
}

// Sum of one double per lane in a fixed tree order; every lane gets the result.  Ends with a barrier.
template <int kLanes>
__device__ __forceinline__ double block_sum(double x, int tid, double* red) {
    red[tid] = x;
    __syncthreads();
    for (int s = kLanes / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

namespace {

// grid (ceil(S / 8192), B): dst[b * stride + h] = hop h of item b, for the hops that hold a sample of the item (h < ceil(len /
// 256)); a workgroup at or past len returns.
template <int kLanes = kGridThreads>    // (a template so that a file which never launches it compiles no copy)
__global__ __launch_bounds__(kLanes) void hop_sums_kernel(const float* __restrict__ audio, int64_t ld, const int64_t* __restrict__ audio_len,
                                                                int S, int vec, double* __restrict__ dst, int64_t stride) {
    __shared__ __attribute__((aligned(16))) float xs[kGridThreads * kGridPad];
    __shared__ double part[kGridThreads];
    static_assert(kLanes == kGridThreads, "one lane per chunk");
    const int tid = threadIdx.x, w = blockIdx.x, b = blockIdx.y;
    const int64_t len = valid_len(audio_len, b, S), base = (int64_t)w * kGridSeg;
    if (base >= len) return;                                            // (uniform) no frame of the item reads a hop from here
    stage_chunks(xs, audio + (int64_t)b * ld, base, len, vec, tid);
    __syncthreads();
    part[tid] = chunk_square_sum(xs, tid);
    __syncthreads();
    if (tid < kGridSegHops) {
        const int64_t h = (int64_t)w * kGridSegHops + tid;
        if (h * kGridHop < len) dst[(int64_t)b * stride + h] = hop_fold(part, tid);
    }
}

}  // namespace
