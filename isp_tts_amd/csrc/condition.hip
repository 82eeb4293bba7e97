// Audio conditioning at both ends of the pipeline (no counterpart in the reference, which takes recordings as they come and
// returns the vocoder's fp32): silence trimming, loudness normalisation to ITU-R BS.1770-4 and conversion to PCM16, on a padded
// mono batch fp32 [B][S] with int64 audio_len [B] (a length below 0 or above S counts as 0, as in ispk_resample_f32).
//
// Definitions.
//   Trim      frames t = 0 .. ceil(len / 256) - 1, frame t = x[256 t, 256 t + 1024) cut at len, p_t = (sum of squares) / 1024 in
//             float64; frame t is active when p_t > ref * factor with ref = max_t p_t ("max") or a constant, factor =
//             10^(-top_db / 10) made on the host.  No active frame: start = end = 0.  Otherwise with the first / last active
//             frames f, l: start = max(0, 256 (f - pad_frames)), end = min(len, 256 (l + pad_frames) + 1024).  Trimming off:
//             start = 0, end = len.
//   Loudness  on x[start, end) with zero filter state at start.  K-weighting = a high shelf then a high-pass, two biquads whose
//             coefficients the host derives for the sample rate (data.k_weighting).  Blocks of 2 fs / 5 samples every fs / 10,
//             only those wholly inside [start, end); z_j = the mean square of block j, l_j = -0.691 + 10 log10 z_j; absolute gate
//             l_j > -70, relative gate l_j > -0.691 + 10 log10(mean z over the absolutely gated blocks) - 10; L = -0.691 +
//             10 log10(mean z over the blocks passing both), -inf without such a block.  peak = max |x| over [start, end).
//   Apply     gain = 10^((target - L) / 20), capped at peak_limit / peak when peak > 0, 1 when L = -inf or the gain is off;
//             out[b][i] = fp32(gain_b) * x[b][start_b + i] for i < end_b - start_b, then zeros; out_len = end - start.
//   PCM16     q = clamp(rint(32768 x + d), -32768, 32767), half to even, 0 past audio_len.  d = 0, or the TPDF dither
//             (h(2 i) - h(2 i + 1)) 2^-32 with h(k) = drop_hash(row seed of (seed, b), k) of dropout.h: a pure function of
//             (seed, b, i).
//
// The meter is a serial recurrence s' = A s + B x over the 4 states of the cascade (transposed direct form II), in float64.
// It runs as a chunked scan on a grid fixed to sample 0: a chunk is 32 samples, a segment 256 chunks = one workgroup.  `start`
// is a multiple of 256, so it always falls on a chunk boundary and the zero-entry final state of a chunk does not depend on it.
//   cond_chunk_kernel   grid (W, B).  Stages the segment in LDS (chunk_grid.h: the grid, its staging and the order of the hop
//                       sums, shared with the segmenter and the noise profile, whose frames are these bit for bit);
//                       every lane runs its chunk from zero state; writes the 256-sample square sums (hops: a trim frame is four),
//                       every chunk's final state, and - after a scan across the lanes with the host's A^(32 2^k) - the segment's.
//   cond_meter_kernel   grid (W, B).  Every workgroup derives (start, end) from the hop sums by itself; a workgroup whose
//                       segment meets [start, end) builds its entry state (the chunk states of start's segment from start on,
//                       then the whole segments between, folded with A^8192), scans its own chunks for every lane's entry state,
//                       reruns the chunks from the true states and accumulates y^2 into the 100 ms steps (relative to start)
//                       and max |x|.  The lanes' step sums are reduced in a fixed order to <= 12 step partials per segment.
//   cond_gate_kernel    grid (B).  Step sums from the segments' partials in segment order, a block = four consecutive steps, the
//                       two gates, L, peak and the gain.
// Every sum runs in a fixed order that depends only on the item (never on B or on another item); no atomics, no host read.
// cond_apply_kernel / pcm16_kernel are streaming, one launch each.
#include <math.h>

#include <algorithm>

#include "chunk_grid.h"
#include "dropout.h"

namespace {

constexpr int kCdSegSteps = 12;                     // steps a segment can meet: ceil(8192 / 800) + 1 at the lowest rate
constexpr int kCdGroups = 16;                       // lane groups of the step reduction
constexpr int kCdPowers = 9;                        // A^(32 2^k), k = 0 .. 8; the last is A^8192
constexpr int kCdTable = 8 + 16 * kCdPowers;
constexpr int kCdMinRate = 8000, kCdMaxRate = 768000;

struct Kw {
    double b0, b1, b2, a1, a2, d1, d2;
};

__device__ __forceinline__ Kw kw_load(const double* __restrict__ tab) {
    Kw c;
    c.b0 = tab[0], c.b1 = tab[1], c.b2 = tab[2], c.a1 = tab[3], c.a2 = tab[4], c.d1 = tab[5], c.d2 = tab[6];
    return c;
}

// One sample through the shelf (b, a) and the high-pass ([1, -2, 1], d), transposed direct form II; returns the output.
__device__ __forceinline__ double kw_step(const Kw& c, double x, double s[4]) {
    const double y1 = fma(c.b0, x, s[0]);
    s[0] = fma(-c.a1, y1, fma(c.b1, x, s[1]));
    s[1] = fma(-c.a2, y1, c.b2 * x);
    const double y2 = y1 + s[2];
    s[2] = fma(-c.d1, y2, fma(-2.0, y1, s[3]));
    s[3] = fma(-c.d2, y2, y1);
    return y2;
}

// v += P u, P a row-major 4 x 4 (uniform address: scalar loads)
__device__ __forceinline__ void mat_acc(const double* __restrict__ P, const double u[4], double v[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double acc = v[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = fma(P[4 * i + j], u[j], acc);
        v[i] = acc;
    }
}

// Inclusive scan over the workgroup's lanes of S_c = A^32 S_(c-1) + v_c (Hillis-Steele, in registers; st is the exchange
// buffer).  Ends with every lane's result also in st[.][tid], after a barrier.
__device__ __forceinline__ void cd_scan(double (*st)[kGridThreads], const double* __restrict__ tab, int tid, double v[4]) {
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
        st[0][tid] = v[0], st[1][tid] = v[1], st[2][tid] = v[2], st[3][tid] = v[3];
        __syncthreads();
        const int src = tid - (1 << k);
        if (src >= 0) {
            const double u[4] = {st[0][src], st[1][src], st[2][src], st[3][src]};
            mat_acc(tab + 8 + 16 * k, u, v);
        }
        __syncthreads();
    }
    st[0][tid] = v[0], st[1][tid] = v[1], st[2][tid] = v[2], st[3][tid] = v[3];
    __syncthreads();
}

struct CondArgs {
    int64_t ld;
    int S, W, NH, NS, step, vec;
    int trim_mode, pad_frames, gain_mode;     // trim_mode 0 off, 1 ref = max, 2 ref folded into trim_thr
    double trim_thr, target, peak_limit;
    double *hop, *chunk, *seg, *segstep, *segpeak, *steps;
};

__global__ __launch_bounds__(kGridThreads) void cond_chunk_kernel(const float* __restrict__ audio, const int64_t* __restrict__ audio_len,
                                                                  const double* __restrict__ tab, const CondArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[kGridThreads * kGridPad];
    __shared__ double st[4][kGridThreads];
    const int tid = threadIdx.x, w = blockIdx.x, b = blockIdx.y;
    const int64_t len = valid_len(audio_len, b, a.S);
    stage_chunks(xs, audio + (int64_t)b * a.ld, (int64_t)w * kGridSeg, len, a.vec, tid);
    __syncthreads();
    const Kw c = kw_load(tab);
    double s[4] = {0.0, 0.0, 0.0, 0.0}, e = 0.0;
    each_sample(xs, tid, [&](int, double x) {
        e = fma(x, x, e);                                               // chunk_square_sum's chain, in the filter's pass
        kw_step(c, x, s);
    });
    st[0][tid] = e;
    __syncthreads();
    if (tid < kGridSegHops) {
        const int h = w * kGridSegHops + tid;
        if (h < a.NH) a.hop[(int64_t)b * a.NH + h] = hop_fold(st[0], tid);
    }
    __syncthreads();
    double* f = a.chunk + (((int64_t)b * a.W + w) * kGridThreads + tid) * 4;
    f[0] = s[0], f[1] = s[1], f[2] = s[2], f[3] = s[3];
    cd_scan(st, tab, tid, s);
    if (tid == kGridThreads - 1) {
        double* g = a.seg + ((int64_t)b * a.W + w) * 4;
        g[0] = s[0], g[1] = s[1], g[2] = s[2], g[3] = s[3];
    }
}

// (start, end) of item b from its hop sums; every thread gets them.  Uses red / ired as scratch and ends with a barrier.
__device__ __forceinline__ void cd_bounds(const double* __restrict__ hop, int64_t len, const CondArgs& a, int tid, double* red,
                                          int* ired, int64_t& start, int64_t& end) {
    start = 0, end = len;
    if (a.trim_mode == 0) return;
    const int nh = (int)((len + kGridHop - 1) / kGridHop);
    double thr = a.trim_thr;
    if (a.trim_mode == 1) {
        double mx = 0.0;
        for (int t = tid; t < nh; t += kGridThreads) mx = fmax(mx, frame_power(hop, t, nh));
        thr = frame_threshold<kGridThreads>(mx, true, 0.0, a.trim_thr, tid, red);
        __syncthreads();                                                // (red is st[0]: the caller's scans write it next)
    }
    int first = 0x7fffffff, last = -1;
    for (int t = tid; t < nh; t += kGridThreads)
        if (frame_power(hop, t, nh) > thr) {
            first = min(first, t);
            last = max(last, t);
        }
    active_range<kGridThreads>(first, last, tid, ired);
    if (last < 0) {
        start = end = 0;
        return;
    }
    start = trim_start(first, a.pad_frames);
    end = trim_end(last, a.pad_frames, len);
}

__global__ __launch_bounds__(kGridThreads) void cond_meter_kernel(const float* __restrict__ audio, const int64_t* __restrict__ audio_len,
                                                                  const double* __restrict__ tab, int64_t* __restrict__ bounds,
                                                                  const CondArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[kGridThreads * kGridPad];
    __shared__ double st[4][kGridThreads];
    __shared__ int ired[2 * kGridThreads];
    const int tid = threadIdx.x, w = blockIdx.x, b = blockIdx.y;
    const int64_t len = valid_len(audio_len, b, a.S);
    int64_t start, end;
    cd_bounds(a.hop + (int64_t)b * a.NH, len, a, tid, st[0], ired, start, end);
    if (w == 0 && tid == 0) bounds[2 * b] = start, bounds[2 * b + 1] = end;
    const int64_t segb = (int64_t)w * kGridSeg;
    if (end <= start || segb >= end || segb + kGridSeg <= start) return;      // (uniform) nothing of [start, end) here

    // the state at this segment's first sample
    const int vs = (int)(start / kGridSeg);
    const int64_t cs = start / kGridChunk;
    double E[4] = {0.0, 0.0, 0.0, 0.0};
    if (w > vs) {
        const double* f = a.chunk + (((int64_t)b * a.W + vs) * kGridThreads + tid) * 4;
        const bool live = (int64_t)vs * kGridThreads + tid >= cs;
        double v[4] = {live ? f[0] : 0.0, live ? f[1] : 0.0, live ? f[2] : 0.0, live ? f[3] : 0.0};
        cd_scan(st, tab, tid, v);
        E[0] = st[0][kGridThreads - 1], E[1] = st[1][kGridThreads - 1], E[2] = st[2][kGridThreads - 1], E[3] = st[3][kGridThreads - 1];
        __syncthreads();
        for (int u = vs + 1; u < w; ++u) {
            const double* g = a.seg + ((int64_t)b * a.W + u) * 4;
            double n[4] = {g[0], g[1], g[2], g[3]};
            mat_acc(tab + 8 + 16 * (kCdPowers - 1), E, n);
            E[0] = n[0], E[1] = n[1], E[2] = n[2], E[3] = n[3];
        }
    }
    const int64_t cg = (int64_t)w * kGridThreads + tid;                   // this lane's chunk on the item's grid
    const int64_t cb = cg * kGridChunk;
    const bool live = cg >= cs && cb < end;
    double s[4];
    {
        const double* f = a.chunk + (((int64_t)b * a.W + w) * kGridThreads + tid) * 4;
        const bool in = cg >= cs;
        double v[4] = {in ? f[0] : 0.0, in ? f[1] : 0.0, in ? f[2] : 0.0, in ? f[3] : 0.0};
        if (tid == 0) mat_acc(tab + 8, E, v);
        cd_scan(st, tab, tid, v);
        const int p = max(tid - 1, 0);
        s[0] = tid ? st[0][p] : E[0], s[1] = tid ? st[1][p] : E[1], s[2] = tid ? st[2][p] : E[2], s[3] = tid ? st[3][p] : E[3];
    }
    stage_chunks(xs, audio + (int64_t)b * a.ld, segb, len, a.vec, tid);
    __syncthreads();                                                    // (also: every lane has read its entry state from st)

    // rerun from the true state: y^2 into the step the sample belongs to (a chunk meets at most two), max |x|
    const Kw c = kw_load(tab);
    double a0 = 0.0, a1 = 0.0;
    float pk = 0.f;
    int j0 = -100;
    if (live) {
        const int64_t rel = cb - start;
        j0 = (int)(rel / a.step);
        const int kend = (int)std::min<int64_t>(kGridChunk, end - cb);
        const int nb = (int)std::min<int64_t>(kend, (int64_t)(j0 + 1) * a.step - rel);   // samples of step j0 in this chunk
        const float* x = xs + tid * kGridPad;
#pragma unroll
        for (int k4 = 0; k4 < kGridChunk / 4; ++k4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * k4);
            const float xf[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = 4 * k4 + q;
                const double y = kw_step(c, (double)xf[q], s);
                const double sq = y * y;
                a0 += k < nb ? sq : 0.0;
                a1 += (k >= nb && k < kend) ? sq : 0.0;
                pk = k < kend ? fmaxf(pk, fabsf(xf[q])) : pk;
            }
        }
    }
    // step partials of the segment: thread (k, g) adds the lanes 16 g .. 16 g + 15 of step jlo + k in lane order, thread k the
    // 16 groups in order
    double* A0 = st[0];
    double* A1 = st[1];
    double* part = st[2];                                               // [kCdSegSteps][kCdGroups] (192 of st[2..3]'s 512)
    float* fpk = reinterpret_cast<float*>(ired + kGridThreads);
    A0[tid] = a0, A1[tid] = a1, ired[tid] = j0, fpk[tid] = pk;
    __syncthreads();
    const int jlo = (int)((std::max<int64_t>(segb, start) - start) / a.step);
    if (tid < kCdSegSteps * kCdGroups) {
        const int j = jlo + tid / kCdGroups, g = tid % kCdGroups;
        double t = 0.0;
        for (int l = g * (kGridThreads / kCdGroups); l < (g + 1) * (kGridThreads / kCdGroups); ++l) {
            const int jl = ired[l];
            if (jl + 1 == j) t += A1[l];
            if (jl == j) t += A0[l];
        }
        part[tid] = t;
    }
    for (int sft = kGridThreads / 2; sft > 0; sft >>= 1) {                // (the peak: a max, any order gives the same bits)
        __syncthreads();
        if (tid < sft) fpk[tid] = fmaxf(fpk[tid], fpk[tid + sft]);
    }
    __syncthreads();
    if (tid < kCdSegSteps) {
        double t = 0.0;
        for (int g = 0; g < kCdGroups; ++g) t += part[tid * kCdGroups + g];
        a.segstep[((int64_t)b * a.W + w) * kCdSegSteps + tid] = t;
    }
    if (tid == 0) a.segpeak[(int64_t)b * a.W + w] = (double)fpk[0];
}

__device__ __forceinline__ double block_z(const double* __restrict__ st, int64_t j, double block_len) {
    return (((st[j] + st[j + 1]) + st[j + 2]) + st[j + 3]) / block_len;
}

__global__ __launch_bounds__(kGridThreads) void cond_gate_kernel(const int64_t* __restrict__ bounds, double* __restrict__ loudness,
                                                                 float* __restrict__ peak, float* __restrict__ gain, const CondArgs a) {
    __shared__ double red[kGridThreads];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t start = bounds[2 * b], end = bounds[2 * b + 1];       // (cond_meter_kernel's: 0 <= start <= end <= S)
    const int64_t nsteps = (end - start) / a.step, nblk = nsteps >= 4 ? nsteps - 3 : 0;
    double* steps = a.steps + (int64_t)b * a.NS;
    for (int64_t j = tid; j < nsteps; j += kGridThreads) {
        const int64_t lo = start + j * a.step, hi = lo + a.step - 1;
        double t = 0.0;
        for (int64_t w = lo / kGridSeg; w <= hi / kGridSeg; ++w) {
            const int64_t jlo = (std::max<int64_t>(w * kGridSeg, start) - start) / a.step;
            t += a.segstep[((int64_t)b * a.W + w) * kCdSegSteps + (j - jlo)];
        }
        steps[j] = t;
    }
    __syncthreads();
    const double block_len = 4.0 * (double)a.step;
    double sum = 0.0, cnt = 0.0;
    for (int64_t j = tid; j < nblk; j += kGridThreads) {
        const double z = block_z(steps, j, block_len);
        if (-0.691 + 10.0 * log10(z) > -70.0) sum += z, cnt += 1.0;
    }
    const double sum1 = block_sum<kGridThreads>(sum, tid, red), cnt1 = block_sum<kGridThreads>(cnt, tid, red);
    double L = -(double)__builtin_inff();
    if (cnt1 > 0.0) {
        const double gamma = -0.691 + 10.0 * log10(sum1 / cnt1) - 10.0;
        sum = 0.0, cnt = 0.0;
        for (int64_t j = tid; j < nblk; j += kGridThreads) {
            const double z = block_z(steps, j, block_len);
            const double l = -0.691 + 10.0 * log10(z);
            if (l > -70.0 && l > gamma) sum += z, cnt += 1.0;
        }
        const double sum2 = block_sum<kGridThreads>(sum, tid, red), cnt2 = block_sum<kGridThreads>(cnt, tid, red);
        if (cnt2 > 0.0) L = -0.691 + 10.0 * log10(sum2 / cnt2);
    }
    double pk = 0.0;
    if (end > start)
        for (int64_t w = start / kGridSeg + tid; w <= (end - 1) / kGridSeg; w += kGridThreads) pk = fmax(pk, a.segpeak[(int64_t)b * a.W + w]);
    pk = block_max<kGridThreads>(pk, tid, red);
    if (tid == 0) {
        double g = 1.0;
        if (a.gain_mode && L > -(double)__builtin_inff()) {
            g = pow(10.0, (a.target - L) / 20.0);
            if (pk > 0.0) g = fmin(g, a.peak_limit / pk);
        }
        loudness[b] = L, peak[b] = (float)pk, gain[b] = (float)g;
    }
}

// ------------------------------------------------------------------------------------------------------------ apply, PCM16
constexpr int kApThreads = 256;
constexpr int kApPer = 16;                          // samples per thread (four float4)

__global__ __launch_bounds__(kApThreads) void cond_apply_kernel(const float* __restrict__ audio, int64_t ld, const int64_t* __restrict__ bounds,
                                                                const float* __restrict__ gain, float* __restrict__ out, int64_t ld_out,
                                                                int64_t* __restrict__ out_len, int S, int S_out, int vec) {
    const int b = blockIdx.y;
    int64_t start = bounds[2 * b], end = bounds[2 * b + 1];
    if (!(0 <= start && start <= end && end <= S)) start = end = 0;     // (device data)
    const int64_t n = std::min<int64_t>(end - start, S_out);
    if (blockIdx.x == 0 && threadIdx.x == 0 && out_len) out_len[b] = n;
    const float g = gain ? gain[b] : 1.f;
    const float* x = audio + (int64_t)b * ld + start;
    float* o = out + (int64_t)b * ld_out;
    const bool v4 = vec && start % 4 == 0;
    const int64_t i0 = ((int64_t)blockIdx.x * kApThreads + threadIdx.x) * 4;
#pragma unroll
    for (int r = 0; r < kApPer / 4; ++r) {
        const int64_t i = i0 + (int64_t)r * gridDim.x * kApThreads * 4;
        if (i >= S_out) break;
        if (v4 && i + 4 <= S_out) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (i + 4 <= n) {
                v = *reinterpret_cast<const f32x4*>(x + i);
                v.x = g * v.x, v.y = g * v.y, v.z = g * v.z, v.w = g * v.w;
            } else {
                if (i < n) v.x = g * x[i];
                if (i + 1 < n) v.y = g * x[i + 1];
                if (i + 2 < n) v.z = g * x[i + 2];
            }
            *reinterpret_cast<f32x4*>(o + i) = v;
        } else {
            for (int e = 0; e < 4 && i + e < S_out; ++e) o[i + e] = i + e < n ? g * x[i + e] : 0.f;
        }
    }
}

__device__ __forceinline__ int16_t pcm_one(float x, uint64_t rs, uint32_t i, int dither) {
    double v = (double)x * 32768.0;
    if (dither) {
        const int64_t h1 = drop_hash(rs, 2u * i), h2 = drop_hash(rs, 2u * i + 1u);
        v += (double)(h1 - h2) * (1.0 / 4294967296.0);
    }
    if (!(v == v)) return 0;
    v = fmin(fmax(rint(v), -32768.0), 32767.0);
    return (int16_t)(int)v;
}

__global__ __launch_bounds__(kApThreads) void pcm16_kernel(const float* __restrict__ audio, int64_t ld, const int64_t* __restrict__ audio_len,
                                                           int16_t* __restrict__ out, int64_t ld_out, int S, int vec, int dither,
                                                           uint64_t seed) {
    const int b = blockIdx.y;
    const int64_t len = valid_len(audio_len, b, S);
    uint64_t rs = seed + (uint64_t)b + 0x9e3779b97f4a7c15ull;           // splitmix64 of (mixed seed + b): the row's two seed words
    rs = (rs ^ (rs >> 30)) * 0xbf58476d1ce4e5b9ull;
    rs = (rs ^ (rs >> 27)) * 0x94d049bb133111ebull;
    rs ^= rs >> 31;
    const float* x = audio + (int64_t)b * ld;
    int16_t* o = out + (int64_t)b * ld_out;
    const int64_t i = ((int64_t)blockIdx.x * kApThreads + threadIdx.x) * 4;
    if (i >= S) return;
    float xv[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec && i + 4 <= len) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + i);
        xv[0] = v.x, xv[1] = v.y, xv[2] = v.z, xv[3] = v.w;
    } else {
        for (int e = 0; e < 4; ++e)
            if (i + e < len) xv[e] = x[i + e];
    }
    int16_t q[4];
    for (int e = 0; e < 4; ++e) q[e] = i + e < len ? pcm_one(xv[e], rs, (uint32_t)(i + e), dither) : (int16_t)0;
    if (vec && i + 4 <= S) {
        bf16x4 pk;
        pk.x = q[0], pk.y = q[1], pk.z = q[2], pk.w = q[3];
        *reinterpret_cast<bf16x4*>(o + i) = pk;
    } else {
        for (int e = 0; e < 4 && i + e < S; ++e) o[i + e] = q[e];
    }
}

struct CondLayout {
    int W, NH, NS;
    int64_t hop, chunk, seg, segstep, segpeak, steps, total;           // offsets and the total, in doubles
};

CondLayout cond_layout(int B, int S, int step) {
    CondLayout l;
    l.W = std::max(1, (S + kGridSeg - 1) / kGridSeg);
    l.NH = std::max(1, (S + kGridHop - 1) / kGridHop);
    l.NS = S / step + 1;
    int64_t at = 0;
    l.hop = at, at += (int64_t)B * l.NH;
    l.chunk = at, at += (int64_t)B * l.W * kGridThreads * 4;
    l.seg = at, at += (int64_t)B * l.W * 4;
    l.segstep = at, at += (int64_t)B * l.W * kCdSegSteps;
    l.segpeak = at, at += (int64_t)B * l.W;
    l.steps = at, at += (int64_t)B * l.NS;
    l.total = at;
    return l;
}

bool ranges_overlap(const void* p, int64_t pb, const void* q, int64_t qb) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}

}  // namespace

extern "C" int32_t ispk_audio_measure_f64(const float* audio, int64_t ld_audio, const int64_t* audio_len, const double* table,
                                          int64_t table_doubles, int64_t* bounds, double* loudness, float* peak, float* gain,
                                          float* workspace, int64_t workspace_floats, int32_t B, int32_t S, int32_t sample_rate,
                                          int32_t trim_mode, double trim_threshold, int32_t pad_frames, int32_t gain_mode,
                                          double target_lufs, double peak_limit, ispk_stream_t stream) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= (1 << 24), ISPK_E_SHAPE,
                 "ispk_audio_measure_f64: bad shape B=%d S=%d (B <= 65535, S <= 2^24)", B, S);
    ISPK_REQUIRE(sample_rate > 0 && sample_rate % 10 == 0, ISPK_E_SHAPE,
                 "ispk_audio_measure_f64: a 100 ms step of %d Hz is not a whole number of samples", sample_rate);
    ISPK_REQUIRE(sample_rate >= kCdMinRate && sample_rate <= kCdMaxRate, ISPK_E_UNSUPPORTED,
                 "ispk_audio_measure_f64: %d Hz is not supported: %d .. %d Hz", sample_rate, kCdMinRate, kCdMaxRate);
    ISPK_REQUIRE(trim_mode >= 0 && trim_mode <= 2 && pad_frames >= 0 && pad_frames <= (1 << 16) && (trim_mode == 0 || trim_threshold >= 0.0),
                 ISPK_E_SHAPE, "ispk_audio_measure_f64: bad trim mode %d, pad_frames %d or threshold %g", trim_mode, pad_frames,
                 trim_threshold);
    ISPK_REQUIRE(!gain_mode || (peak_limit > 0.0 && target_lufs == target_lufs), ISPK_E_SHAPE,
                 "ispk_audio_measure_f64: bad target %g LUFS or peak limit %g", target_lufs, peak_limit);
    if (B == 0) return 0;
    ISPK_REQUIRE(audio && audio_len && table && bounds && loudness && peak && gain && workspace, ISPK_E_NULL,
                 "ispk_audio_measure_f64: null pointer");
    ISPK_REQUIRE(table_doubles == kCdTable, ISPK_E_SHAPE, "ispk_audio_measure_f64: a table of %lld doubles, expected %d",
                 (long long)table_doubles, kCdTable);
    ISPK_REQUIRE(ld_audio >= S, ISPK_E_SHAPE, "ispk_audio_measure_f64: row stride %lld below S=%d", (long long)ld_audio, S);
    const CondLayout l = cond_layout(B, S, sample_rate / 10);
    ISPK_REQUIRE(workspace_floats >= 2 * l.total && ispk_aligned(workspace, 8), ISPK_E_ALIGN,
                 "ispk_audio_measure_f64: the workspace needs %lld floats at an 8-byte boundary, got %lld", (long long)(2 * l.total),
                 (long long)workspace_floats);
    double* ws = reinterpret_cast<double*>(workspace);
    CondArgs a;
    a.ld = ld_audio, a.S = S, a.W = l.W, a.NH = l.NH, a.NS = l.NS, a.step = sample_rate / 10;
    a.vec = ld_audio % 4 == 0 && ispk_aligned(audio, 16);
    a.trim_mode = trim_mode, a.pad_frames = pad_frames, a.gain_mode = gain_mode;
    a.trim_thr = trim_threshold, a.target = target_lufs, a.peak_limit = peak_limit;
    a.hop = ws + l.hop, a.chunk = ws + l.chunk, a.seg = ws + l.seg, a.segstep = ws + l.segstep, a.segpeak = ws + l.segpeak;
    a.steps = ws + l.steps;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cond_chunk_kernel, dim3(l.W, B), dim3(kGridThreads), 0, st, audio, audio_len, table, a);
    hipLaunchKernelGGL(cond_meter_kernel, dim3(l.W, B), dim3(kGridThreads), 0, st, audio, audio_len, table, bounds, a);
    hipLaunchKernelGGL(cond_gate_kernel, dim3(B), dim3(kGridThreads), 0, st, bounds, loudness, peak, gain, a);
    return ispk_launch_status();
}

extern "C" int32_t ispk_audio_apply_f32(const float* audio, int64_t ld_audio, const int64_t* bounds, const float* gain, float* out,
                                        int64_t ld_out, int64_t* out_len, int32_t B, int32_t S, int32_t S_out, ispk_stream_t stream) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= (1 << 24) && S_out >= 0 && S_out <= (1 << 24), ISPK_E_SHAPE,
                 "ispk_audio_apply_f32: bad shape B=%d S=%d S_out=%d", B, S, S_out);
    if (B == 0) return 0;
    ISPK_REQUIRE(audio && bounds && out, ISPK_E_NULL, "ispk_audio_apply_f32: null pointer");
    ISPK_REQUIRE(ld_audio >= S && ld_out >= S_out, ISPK_E_SHAPE, "ispk_audio_apply_f32: row strides %lld, %lld below S=%d, S_out=%d",
                 (long long)ld_audio, (long long)ld_out, S, S_out);
    ISPK_REQUIRE(!ranges_overlap(audio, 4 * ((int64_t)(B - 1) * ld_audio + S), out, 4 * ((int64_t)(B - 1) * ld_out + S_out)), ISPK_E_SHAPE,
                 "ispk_audio_apply_f32: out may not alias audio (the shift reads ahead of what it writes)");
    const int vec = ld_audio % 4 == 0 && ld_out % 4 == 0 && ispk_aligned(audio, 16) && ispk_aligned(out, 16);
    const int64_t per_block = (int64_t)kApThreads * kApPer;
    const unsigned gx = (unsigned)std::max<int64_t>(1, ((int64_t)S_out + per_block - 1) / per_block);   // (S_out = 0: out_len alone)
    hipLaunchKernelGGL(cond_apply_kernel, dim3(gx, B), dim3(kApThreads), 0, reinterpret_cast<hipStream_t>(stream), audio, ld_audio,
                       bounds, gain, out, ld_out, out_len, S, S_out, vec);
    return ispk_launch_status();
}

extern "C" int32_t ispk_pcm16(const float* audio, int64_t ld_audio, const int64_t* audio_len, int16_t* out, int64_t ld_out, int32_t B,
                              int32_t S, int32_t dither, uint64_t seed, ispk_stream_t stream) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= (1 << 24), ISPK_E_SHAPE, "ispk_pcm16: bad shape B=%d S=%d", B, S);
    if (B == 0 || S == 0) return 0;
    ISPK_REQUIRE(audio && audio_len && out, ISPK_E_NULL, "ispk_pcm16: null pointer");
    ISPK_REQUIRE(ld_audio >= S && ld_out >= S, ISPK_E_SHAPE, "ispk_pcm16: row strides %lld, %lld below S=%d", (long long)ld_audio,
                 (long long)ld_out, S);
    const int vec = ld_audio % 4 == 0 && ld_out % 4 == 0 && ispk_aligned(audio, 16) && ispk_aligned(out, 8);
    const unsigned gx = (unsigned)(((int64_t)S + kApThreads * 4 - 1) / (kApThreads * 4));
    hipLaunchKernelGGL(pcm16_kernel, dim3(gx, B), dim3(kApThreads), 0, reinterpret_cast<hipStream_t>(stream), audio, ld_audio, audio_len,
                       out, ld_out, S, vec, dither != 0, mix_seed(seed));
    return ispk_launch_status();
}
