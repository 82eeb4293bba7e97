// Screen (no counterpart in the reference, whose corpus arrives curated): per item of a padded mono batch fp32 [B][S] with
// int64 audio_len [B] (a length below 0 or above S counts as 0) the measurements that decide whether a piece is fit to train on -
// non-finite samples, peak, DC, power, clipping (runs at the rail), digital dropouts (runs of exact zeros inside the signal), the
// long-term average spectrum over the 1024 / 256 frames and the bandwidth read off it - and a word of flags.  include/ispk.h has
// the definitions.  A non-finite sample is counted and read as 0 by everything else.
//
//   screen_tile_kernel   grid (ceil(S / 4096), B), 512 threads.  A workgroup owns kTile = 4,096 samples of one item and the <= 16
//                        frames that START in them (frame f = samples [256 f, 256 f + 1024), no padding), so it stages 4,864
//                        samples in LDS, zeros past the length (float4 loads when the row allows).  Every lane takes 8 consecutive
//                        samples: peak, float64 sum and sum of squares, then a butterfly and the eight waves in order.  The zero
//                        runs by tile_runs below.  The frames go four at a time through fft.h as in stft_tile.h (a dead group
//                        transforms zeros); after a round lane k adds |X_f[k]|^2 (fp32) of the round's frames in frame order into
//                        its float64 sum, which goes to the workspace as the tile's partial [513].  A workgroup at or past the
//                        length returns.
//   screen_item_kernel   grid (B), 512 threads.  The tiles' statistics (lane-strided, a butterfly, the waves in order: an order
//                        that depends on the length alone); ltas[k] = (the partials in tile order) / F; the peak over bins 2 ..
//                        512 and band_bin by max-reductions; the dropouts by walk_runs; thr = peak * rail_ratio for the next pass.
//   screen_rail_kernel   grid (ceil(S / 4096), B).  The second tile pass: stages 4,096 samples and summarises the runs at the rail.
//   screen_flag_kernel   grid (B).  walk_runs over the rail summaries, then the flags.
//
// Runs.  A predicate gives every sample a class (0: not in a run; zero: 1; rail: 1 at +thr, 2 at -thr); a run is a maximal
// stretch of one non-zero class.  tile_runs<P> reports per tile the run that touches its first sample (head), the one that
// touches its last (tail; the same run when it spans the tile) and, of the runs that touch neither, the number and samples of
// those of at least min_len, the start of the first such, and the longest of any length: a run start is found per sample, an
// exclusive max-scan over the workgroup hands every lane the last start before its strip.  walk_runs<kZero> walks an item's
// tiles in order (staged 256 at a time in LDS, lane 0 walks), joining a tail to the next head of its class; with kZero a run
// that starts at sample 0 or ends at n - 1 is padding and is left out.
//
// LDS of screen_tile_kernel (stft_tile.h's analysis-only layout, kAnalysisLds): 8 KB twiddles, 16 KB ping, 4 KB window, 19 KB
// of staged samples, 16 KB pong (one 4 KB slot per group: no synthesis side, so none of the 80 KB of frame slots) = 64,512 B
// dynamic, two workgroups (16 waves) per CU.
// Bits.  Every sum runs in an order fixed by the item's length; integers and maxima do not depend on the order; no atomics.  An
// item's results depend on that item alone - not on B, S, the row stride, the alignment or what lies behind its length.
//
// gfx950 resources (csrc/resource_report.py screen.hip; no spills, no scratch):
//   screen_tile_kernel   54 VGPRs, LDS 64,512 B dynamic + 384 B static (two workgroups per CU)
//   screen_item_kernel   44 VGPRs, LDS 8,384 B        screen_rail_kernel   37 VGPRs, LDS 16,576 B
//   screen_flag_kernel   46 VGPRs, LDS 8,192 B
#include <math.h>

#include <algorithm>

#include "common.h"
#include "stft_tile.h"

namespace {

constexpr int kScStrip = kTile / kThreads;                 // 8 consecutive samples per lane
constexpr int kScWaves = kThreads / kWave;                 // 8
constexpr int kScChunk = 256;                              // tile summaries staged in LDS for the walk
constexpr int kScFlagThreads = 256;
constexpr int kScMaxSamples = 1 << 24;                     // CONDITION_MAX_SAMPLES
constexpr int kScTileWords = kBins + 3 + 4 + 4;            // per tile, in 8-byte words: partial [513], TileStat, two RunRec
static_assert(kScStrip == 8, "two float4 per lane");
static_assert(kAnalysisLds == 64512, "the resource line above and DESIGN.md 4.31 quote this");

struct TileStat {
    double sum, sumsq;
    float peak;
    int nonfinite;
};
struct RunRec {
    int head, head_cls, tail, tail_cls;                    // lengths (0: none) and classes of the runs at the tile's two ends
    int runs, samples, longest, first;                     // of the runs that touch neither end; first: offset in the tile
};
static_assert(sizeof(TileStat) == 24 && sizeof(RunRec) == 32, "kScTileWords");

struct ZeroPred {
    __device__ __forceinline__ int operator()(float x) const { return x == 0.f ? 1 : 0; }
};
struct RailPred {
    float thr;
    __device__ __forceinline__ int operator()(float x) const { return thr > 0.f ? (x >= thr ? 1 : x <= -thr ? 2 : 0) : 0; }
};

struct ScreenArgs {
    int S, W, parts, rail_mode, min_run, min_dropout, min_band_bin;
    float rail, rail_ratio;
    double band_factor, max_dc, min_peak;
    int64_t per_item;                                      // workspace words per item
    double* ws;
    int32_t *nonfinite, *clip_runs, *dropout_runs, *band_bin, *flags;
    float* peak;
    double *dc, *power, *ltas;
    int64_t *clip_samples, *clip_longest, *clip_first, *dropout_samples, *dropout_longest;
};

// the item's workspace: partials [W][513], TileStat [W], RunRec zero [W], RunRec rail [W], thr
__device__ __forceinline__ double* ws_partial(const ScreenArgs& a, int b) { return a.ws + (int64_t)b * a.per_item; }
__device__ __forceinline__ TileStat* ws_stat(const ScreenArgs& a, int b) {
    return reinterpret_cast<TileStat*>(ws_partial(a, b) + (int64_t)a.W * kBins);
}
__device__ __forceinline__ RunRec* ws_zero(const ScreenArgs& a, int b) { return reinterpret_cast<RunRec*>(ws_stat(a, b) + a.W); }
__device__ __forceinline__ RunRec* ws_rail(const ScreenArgs& a, int b) { return ws_zero(a, b) + a.W; }
__device__ __forceinline__ float* ws_thr(const ScreenArgs& a, int b) { return reinterpret_cast<float*>(ws_rail(a, b) + a.W); }

__device__ __forceinline__ int sc_frames(int n) { return n >= kNfft ? (n - kNfft) / kHop + 1 : 0; }
__device__ __forceinline__ float sc_finite(float x, int& bad) {
    bad += !is_finite(x);
    return finite_or_zero(x);
}

// xs[j] = x(base + j) for j < count (a multiple of 4), 0 at or past n, a non-finite sample as 0; returns the lane's number of
// non-finite samples among j < kTile.  base is a multiple of 4, so a row that allows float4 loads allows them here.  (Not
// stft_tile.h's stage_flat: base is never negative here, and the tests of i >= 0 that a negative base needs do not fold away.)
__device__ __forceinline__ int sc_stage(float* xs, const float* __restrict__ row, int base, int n, int count, int vec, int tid) {
    int bad = 0;
    for (int g = tid; g < count / 4; g += kThreads) {
        const int i = base + 4 * g;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (vec && i + 4 <= n) {
            v = *reinterpret_cast<const f32x4*>(row + i);
        } else {
            if (i < n) v.x = row[i];
            if (i + 1 < n) v.y = row[i + 1];
            if (i + 2 < n) v.z = row[i + 2];
            if (i + 3 < n) v.w = row[i + 3];
        }
        int own = 0, halo = 0;
        int& cnt = 4 * g < kTile ? own : halo;
        v.x = sc_finite(v.x, cnt), v.y = sc_finite(v.y, cnt), v.z = sc_finite(v.z, cnt), v.w = sc_finite(v.w, cnt);
        bad += own;
        *reinterpret_cast<f32x4*>(xs + 4 * g) = v;
    }
    return bad;
}

// Exclusive max-scan over the workgroup's kThreads lanes; lane 0 gets -1.  buf: kScWaves ints.  Ends with a barrier.
__device__ __forceinline__ int sc_excl_max(int v, int tid, int* buf) {
    const int lane = tid % kWave, w = tid / kWave;
    int inc = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int t = __shfl_up(inc, off, kWave);
        if (lane >= off) inc = max(inc, t);
    }
    if (lane == kWave - 1) buf[w] = inc;
    int excl = __shfl_up(inc, 1, kWave);
    if (lane == 0) excl = -1;
    __syncthreads();
    for (int i = 0; i < w; ++i) excl = max(excl, buf[i]);
    __syncthreads();
    return excl;
}

// The run summary of the tile's m <= kTile samples xs[0, m) (xs holds kTile floats at least), written by lane 0.  sh: 48 ints.
template <typename P>
__device__ __forceinline__ void tile_runs(const float* xs, int m, int min_len, P pred, int tid, int* sh, RunRec* out) {
    const int i0 = tid * kScStrip;
    int c[kScStrip + 2];                                    // c[q + 1]: the class of sample i0 + q; 0 outside [0, m)
    {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(xs + i0), hi = *reinterpret_cast<const f32x4*>(xs + i0 + 4);
        const float v[kScStrip] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int q = 0; q < kScStrip; ++q) c[q + 1] = i0 + q < m ? pred(v[q]) : 0;
        c[0] = tid > 0 ? pred(xs[i0 - 1]) : 0;              // (i0 - 1 < m or the strip is empty: then nothing below looks at it)
        c[kScStrip + 1] = (tid + 1 < kThreads && i0 + kScStrip < m) ? pred(xs[i0 + kScStrip]) : 0;
    }
    int last = -1;
#pragma unroll
    for (int q = 0; q < kScStrip; ++q)
        if (c[q + 1] && c[q] != c[q + 1]) last = i0 + q;
    if (tid < 4) sh[8 + tid] = 0;                           // head, head_cls, tail, tail_cls
    int start = sc_excl_max(last, tid, sh);
    int runs = 0, samples = 0, longest = 0, first = kTile;
#pragma unroll
    for (int q = 0; q < kScStrip; ++q) {
        const int cls = c[q + 1], i = i0 + q;
        if (!cls) continue;
        if (c[q] != cls) start = i;
        if (c[q + 2] != cls) {                              // the run ends here
            const int len = i - start + 1;
            if (start == 0) sh[8] = len, sh[9] = cls;
            if (i == m - 1) sh[10] = len, sh[11] = cls;
            if (start != 0 && i != m - 1) {
                longest = max(longest, len);
                if (len >= min_len) ++runs, samples += len, first = min(first, start);
            }
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        runs += __shfl_xor(runs, off, kWave);
        samples += __shfl_xor(samples, off, kWave);
        longest = max(longest, __shfl_xor(longest, off, kWave));
        first = min(first, __shfl_xor(first, off, kWave));
    }
    if (tid % kWave == 0) {
        int* p = sh + 12 + 4 * (tid / kWave);
        p[0] = runs, p[1] = samples, p[2] = longest, p[3] = first;
    }
    __syncthreads();
    if (tid == 0) {
        RunRec r;
        r.head = sh[8], r.head_cls = sh[9], r.tail = sh[10], r.tail_cls = sh[11];
        r.runs = 0, r.samples = 0, r.longest = 0, r.first = kTile;
        for (int w = 0; w < kScWaves; ++w) {
            const int* p = sh + 12 + 4 * w;
            r.runs += p[0], r.samples += p[1], r.longest = max(r.longest, p[2]), r.first = min(r.first, p[3]);
        }
        *out = r;
    }
    __syncthreads();                                        // sh is free again
}

// What walk_runs returns to lane 0.
struct RunTotals {
    int runs;
    int64_t samples, longest, first;
};

// The runs of an item of n samples from its ceil(n / kTile) tile summaries, in order.  `stage`: kScChunk RunRec of LDS.  Every
// lane of the workgroup calls it (the staging and its barriers); the result is lane 0's.
template <bool kZero>
__device__ __forceinline__ RunTotals walk_runs(const RunRec* __restrict__ recs, int n, int min_len, int tid, int threads, RunRec* stage) {
    RunTotals t;
    t.runs = 0, t.samples = 0, t.longest = 0, t.first = -1;
    int64_t run_len = 0, run_start = 0;
    int run_cls = 0;
    auto close = [&](bool at_end) {
        if (run_len > 0 && (!kZero || (run_start > 0 && !at_end))) {
            t.longest = std::max(t.longest, run_len);
            if (run_len >= min_len) {
                ++t.runs, t.samples += run_len;
                if (t.first < 0) t.first = run_start;
            }
        }
        run_len = 0;
    };
    const int Wn = (n + kTile - 1) / kTile;
    for (int w0 = 0; w0 < Wn; w0 += kScChunk) {
        const int cnt = min(kScChunk, Wn - w0);
        __syncthreads();
        for (int i = tid; i < cnt * 8; i += threads) reinterpret_cast<int*>(stage)[i] = reinterpret_cast<const int*>(recs + w0)[i];
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < cnt; ++j) {
                const RunRec r = stage[j];
                const int64_t base = (int64_t)(w0 + j) * kTile;
                const int m = (int)std::min<int64_t>(kTile, n - base);
                if (r.head > 0) {
                    if (run_len > 0 && r.head_cls == run_cls) {
                        run_len += r.head;
                    } else {
                        close(false);
                        run_start = base, run_len = r.head, run_cls = r.head_cls;
                    }
                    if (r.head < m) close(false);
                } else {
                    close(false);
                }
                if (r.head < m) {                           // no run spans the tile
                    t.longest = std::max<int64_t>(t.longest, r.longest);
                    if (r.runs > 0) {
                        if (t.first < 0) t.first = base + r.first;
                        t.runs += r.runs, t.samples += r.samples;
                    }
                    if (r.tail > 0) run_start = base + m - r.tail, run_len = r.tail, run_cls = r.tail_cls;
                }
            }
    }
    if (tid == 0) close(true);
    return t;
}

__global__ __launch_bounds__(kThreads) void screen_tile_kernel(const float* __restrict__ audio, int64_t ld, const int64_t* __restrict__ audio_len,
                                                               const float* __restrict__ tables, int vec, const ScreenArgs a) {
    extern __shared__ float4 lds_raw[];
    __shared__ double red_d[2 * kScWaves];
    __shared__ float red_f[kScWaves];
    __shared__ int red_i[kScWaves], sh[48];
    const TileLds tile = carve_tile(lds_raw, kAnalysisStage);     // four slots behind the staged samples: the groups' pong buffers
    float* xs = tile.win + kNfft;

    const int tid = threadIdx.x, w = blockIdx.x, b = blockIdx.y, g = tid / kGT, lt = tid % kGT;
    const int n = valid_len(audio_len, b, a.S), base = w * kTile;
    if (base >= n) return;                                  // (uniform) no tile of the item's own
    const int m = min(kTile, n - base);
    const int F = sc_frames(n), f_lo = w * kSegs, nf = (a.parts & 2) ? min(F - f_lo, kSegs) : 0;

    int bad = sc_stage(xs, audio + (int64_t)b * ld, base, n, nf > 0 ? kAnalysisStage : kTile, vec, tid);
    if (nf > 0) load_tables(tile.tw, tile.win, tables, tid);
    __syncthreads();

    // peak and sums: the lane's 8 samples in order, a butterfly, the waves in order
    float pk = 0.f;
    double s = 0.0, ss = 0.0;
    {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(xs + tid * kScStrip), hi = *reinterpret_cast<const f32x4*>(xs + tid * kScStrip + 4);
        const float v[kScStrip] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int q = 0; q < kScStrip; ++q) {                // (zeros at or past m change nothing)
            const double x = (double)v[q];
            pk = fmaxf(pk, fabsf(v[q]));
            s += x;
            ss = fma(x, x, ss);
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        pk = fmaxf(pk, __shfl_xor(pk, off, kWave));
        bad += __shfl_xor(bad, off, kWave);
        s += __shfl_xor(s, off, kWave);
        ss += __shfl_xor(ss, off, kWave);
    }
    if (tid % kWave == 0) red_d[tid / kWave] = s, red_d[kScWaves + tid / kWave] = ss, red_f[tid / kWave] = pk, red_i[tid / kWave] = bad;
    __syncthreads();
    if (tid == 0) {
        TileStat t;
        t.sum = 0.0, t.sumsq = 0.0, t.peak = 0.f, t.nonfinite = 0;
        for (int k = 0; k < kScWaves; ++k)
            t.sum += red_d[k], t.sumsq += red_d[kScWaves + k], t.peak = fmaxf(t.peak, red_f[k]), t.nonfinite += red_i[k];
        ws_stat(a, b)[w] = t;
    }

    if (a.parts & 1) {
        tile_runs(xs, m, a.min_dropout, ZeroPred(), tid, sh, ws_zero(a, b) + w);
    } else if (tid == 0) {
        RunRec r = {0, 0, 0, 0, 0, 0, 0, kTile};
        ws_zero(a, b)[w] = r;
    }

    if (nf > 0) {                                           // (uniform) the frames that start in this tile
        cf* A = tile.ping + g * kHalf;
        cf* Bf = reinterpret_cast<cf*>(tile.frames + g * kNfft);
        double acc = 0.0, acc512 = 0.0;                     // bins tid and (lane 0) 512
        for (int r = 0; r * kGroups < nf; ++r) {
            const int fs = r * kGroups + g;
            gather_zero_padded(A, tile.win, (f_lo + fs) * kHop, n, fs < nf, lt, [&](int i) { return xs[i - base]; });
            __syncthreads();
            fft<false, kGT, kTw>(A, Bf, kHalf, lt, tile.tw);
            for (int q = 0; q < kGroups && r * kGroups + q < nf; ++q) {      // ascending frames
                const cf* Z = reinterpret_cast<const cf*>(tile.frames + q * kNfft);
                const cf X = real_split(Z, tid, kHalf, tile.tw[tid]);
                acc += (double)(X.x * X.x + X.y * X.y);
                if (tid == 0) {
                    const cf Y = real_split(Z, kHalf, kHalf, tile.tw[kHalf]);
                    acc512 += (double)(Y.x * Y.x + Y.y * Y.y);
                }
            }
        }
        double* part = ws_partial(a, b) + (int64_t)w * kBins;
        part[tid] = acc;
        if (tid == 0) part[kHalf] = acc512;
    }
}

__global__ __launch_bounds__(kThreads) void screen_item_kernel(const int64_t* __restrict__ audio_len, const ScreenArgs a) {
    __shared__ RunRec stage[kScChunk];
    __shared__ double red_d[2 * kScWaves];
    __shared__ float red_f[kScWaves];
    __shared__ int red_i[kScWaves];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n = valid_len(audio_len, b, a.S);
    const int Wn = (n + kTile - 1) / kTile, F = sc_frames(n), WF = (a.parts & 2) ? (F + kSegs - 1) / kSegs : 0;

    // statistics
    float pk = 0.f;
    int bad = 0;
    double s = 0.0, ss = 0.0;
    const TileStat* st = ws_stat(a, b);
    for (int w = tid; w < Wn; w += kThreads) {
        const TileStat t = st[w];
        pk = fmaxf(pk, t.peak), bad += t.nonfinite, s += t.sum, ss += t.sumsq;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        pk = fmaxf(pk, __shfl_xor(pk, off, kWave));
        bad += __shfl_xor(bad, off, kWave);
        s += __shfl_xor(s, off, kWave);
        ss += __shfl_xor(ss, off, kWave);
    }
    if (tid % kWave == 0) red_d[tid / kWave] = s, red_d[kScWaves + tid / kWave] = ss, red_f[tid / kWave] = pk, red_i[tid / kWave] = bad;
    __syncthreads();
    if (tid == 0) {
        s = 0.0, ss = 0.0, pk = 0.f, bad = 0;
        for (int k = 0; k < kScWaves; ++k) s += red_d[k], ss += red_d[kScWaves + k], pk = fmaxf(pk, red_f[k]), bad += red_i[k];
        a.peak[b] = pk, a.nonfinite[b] = bad;
        a.dc[b] = n ? s / (double)n : 0.0, a.power[b] = n ? ss / (double)n : 0.0;
        *ws_thr(a, b) = a.rail_mode ? a.rail : pk * a.rail_ratio;
    }
    __syncthreads();                                        // red_* are read

    // the long-term average spectrum, its peak over bins 2 .. 512 and the last bin within band_db of it
    const double* part = ws_partial(a, b);
    double v[2] = {0.0, 0.0}, top = 0.0;
    for (int q = 0; q < 2; ++q) {
        const int k = tid + q * kThreads;
        if (k >= kBins) break;
        double acc = 0.0;
        for (int w = 0; w < WF; ++w) acc += part[(int64_t)w * kBins + k];
        v[q] = F ? acc / (double)F : 0.0;
        a.ltas[(int64_t)b * kBins + k] = v[q];
        if (k >= 2) top = fmax(top, v[q]);
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) top = fmax(top, __shfl_xor(top, off, kWave));
    if (tid % kWave == 0) red_d[tid / kWave] = top;
    __syncthreads();
    top = 0.0;
    for (int k = 0; k < kScWaves; ++k) top = fmax(top, red_d[k]);
    const double level = top * a.band_factor;
    int band = -1;
    if (v[0] >= level) band = tid;
    if (tid == 0 && v[1] >= level) band = kHalf;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) band = max(band, __shfl_xor(band, off, kWave));
    if (tid % kWave == 0) red_i[tid / kWave] = band;
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < kScWaves; ++k) band = max(band, red_i[k]);
        a.band_bin[b] = (WF == 0 || !(top > 0.0)) ? -1 : band;
    }

    // dropouts
    RunTotals t = walk_runs<true>(ws_zero(a, b), (a.parts & 1) ? n : 0, a.min_dropout, tid, kThreads, stage);
    if (tid == 0) {
        a.dropout_runs[b] = t.runs, a.dropout_samples[b] = t.samples;
        a.dropout_longest[b] = t.longest >= a.min_dropout ? t.longest : 0;
    }
}

__global__ __launch_bounds__(kThreads) void screen_rail_kernel(const float* __restrict__ audio, int64_t ld, const int64_t* __restrict__ audio_len,
                                                               int vec, const ScreenArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[kTile];
    __shared__ int sh[48];
    const int tid = threadIdx.x, w = blockIdx.x, b = blockIdx.y;
    const int n = valid_len(audio_len, b, a.S), base = w * kTile;
    if (base >= n) return;                                  // (uniform)
    sc_stage(xs, audio + (int64_t)b * ld, base, n, kTile, vec, tid);
    __syncthreads();
    RailPred p;
    p.thr = *ws_thr(a, b);
    tile_runs(xs, min(kTile, n - base), a.min_run, p, tid, sh, ws_rail(a, b) + w);
}

__global__ __launch_bounds__(kScFlagThreads) void screen_flag_kernel(const int64_t* __restrict__ audio_len, const ScreenArgs a) {
    __shared__ RunRec stage[kScChunk];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n = valid_len(audio_len, b, a.S);
    RunTotals t = walk_runs<false>(ws_rail(a, b), (a.parts & 1) ? n : 0, a.min_run, tid, kScFlagThreads, stage);
    if (tid == 0) {
        a.clip_runs[b] = t.runs, a.clip_samples[b] = t.samples, a.clip_longest[b] = t.longest, a.clip_first[b] = t.first;
        const int band = a.band_bin[b];
        const double dc = a.dc[b];
        int f = 0;
        f |= t.runs > 0 ? 1 : 0;
        f |= (a.min_band_bin >= 0 && band >= 0 && band < a.min_band_bin) ? 2 : 0;
        f |= fabs(dc) > a.max_dc ? 4 : 0;
        f |= a.dropout_runs[b] > 0 ? 8 : 0;
        f |= a.nonfinite[b] > 0 ? 16 : 0;
        f |= (double)a.peak[b] <= a.min_peak ? 32 : 0;
        f |= sc_frames(n) == 0 ? 64 : 0;
        a.flags[b] = f;
    }
}

int64_t screen_words(int S) { return (int64_t)kScTileWords * std::max(1, (S + kTile - 1) / kTile) + 1; }

}  // namespace

extern "C" int32_t ispk_screen_tile_samples(void) { return kTile; }

extern "C" int32_t ispk_screen_workspace_bytes(int32_t B, int32_t S, int64_t* bytes) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= kScMaxSamples, ISPK_E_SHAPE,
                 "ispk_screen_workspace_bytes: bad shape B=%d S=%d (B <= 65535, 0 <= S <= 2^24)", B, S);
    ISPK_REQUIRE(bytes, ISPK_E_NULL, "ispk_screen_workspace_bytes: null pointer");
    *bytes = 8 * (int64_t)B * screen_words(S);
    return 0;
}

extern "C" int32_t ispk_screen_f64(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables, int32_t parts,
                                   int32_t rail_mode, float rail, float rail_ratio, int32_t min_run, int32_t min_dropout,
                                   double band_factor, int32_t min_band_bin, double max_dc, double min_peak, int32_t* nonfinite,
                                   float* peak, double* dc, double* power, int32_t* clip_runs, int64_t* clip_samples,
                                   int64_t* clip_longest, int64_t* clip_first, int32_t* dropout_runs, int64_t* dropout_samples,
                                   int64_t* dropout_longest, double* ltas, int32_t* band_bin, int32_t* flags, void* workspace,
                                   int64_t workspace_bytes, int32_t B, int32_t S, ispk_stream_t stream) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= kScMaxSamples, ISPK_E_SHAPE,
                 "ispk_screen_f64: bad shape B=%d S=%d (B <= 65535, 0 <= S <= 2^24)", B, S);
    ISPK_REQUIRE(parts >= 1 && parts <= 3, ISPK_E_SHAPE, "ispk_screen_f64: parts %d is not a mask of 1 (levels and runs) and 2 (spectrum)", parts);
    ISPK_REQUIRE((rail_mode == 0 && rail_ratio > 0.f && rail_ratio <= 1.f) || (rail_mode == 1 && rail > 0.f && isfinite(rail)), ISPK_E_SHAPE,
                 "ispk_screen_f64: bad rail mode %d with rail %g, rail_ratio %g (mode 0: 0 < ratio <= 1; mode 1: a positive finite rail)",
                 rail_mode, (double)rail, (double)rail_ratio);
    ISPK_REQUIRE(min_run >= 1 && min_dropout >= 1, ISPK_E_SHAPE, "ispk_screen_f64: min_run %d, min_dropout %d below 1", min_run, min_dropout);
    ISPK_REQUIRE(band_factor > 0.0 && band_factor < 1.0 && min_band_bin >= -1 && min_band_bin <= kBins, ISPK_E_SHAPE,
                 "ispk_screen_f64: band_factor %g outside (0, 1) or min_band_bin %d outside -1 .. %d", band_factor, min_band_bin, kBins);
    ISPK_REQUIRE(max_dc >= 0.0 && min_peak >= 0.0, ISPK_E_SHAPE, "ispk_screen_f64: max_dc %g or min_peak %g is negative or NaN", max_dc, min_peak);
    if (B == 0) return 0;
    ISPK_REQUIRE(audio && audio_len && tables && nonfinite && peak && dc && power && clip_runs && clip_samples && clip_longest && clip_first &&
                     dropout_runs && dropout_samples && dropout_longest && ltas && band_bin && flags && workspace,
                 ISPK_E_NULL, "ispk_screen_f64: null pointer");
    ISPK_REQUIRE(ld_audio >= S, ISPK_E_SHAPE, "ispk_screen_f64: row stride %lld below S=%d", (long long)ld_audio, S);
    const int64_t words = screen_words(S);
    ISPK_REQUIRE(workspace_bytes >= 8 * (int64_t)B * words && ispk_aligned(workspace, 8), ISPK_E_ALIGN,
                 "ispk_screen_f64: the workspace needs %lld bytes at an 8-byte boundary, got %lld", (long long)(8 * (int64_t)B * words),
                 (long long)workspace_bytes);
    ScreenArgs a;
    a.S = S, a.W = std::max(1, (S + kTile - 1) / kTile), a.parts = parts, a.rail_mode = rail_mode, a.min_run = min_run;
    a.min_dropout = min_dropout, a.min_band_bin = min_band_bin, a.rail = rail, a.rail_ratio = rail_ratio;
    a.band_factor = band_factor, a.max_dc = max_dc, a.min_peak = min_peak, a.per_item = words;
    a.ws = reinterpret_cast<double*>(workspace);
    a.nonfinite = nonfinite, a.clip_runs = clip_runs, a.dropout_runs = dropout_runs, a.band_bin = band_bin, a.flags = flags;
    a.peak = peak, a.dc = dc, a.power = power, a.ltas = ltas;
    a.clip_samples = clip_samples, a.clip_longest = clip_longest, a.clip_first = clip_first;
    a.dropout_samples = dropout_samples, a.dropout_longest = dropout_longest;
    const int vec = ld_audio % 4 == 0 && ispk_aligned(audio, 16);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned W = (unsigned)((S + kTile - 1) / kTile);
    if (W) hipLaunchKernelGGL(screen_tile_kernel, dim3(W, B), dim3(kThreads), kAnalysisLds, st, audio, ld_audio, audio_len, tables, vec, a);
    hipLaunchKernelGGL(screen_item_kernel, dim3(B), dim3(kThreads), 0, st, audio_len, a);
    if (W && (parts & 1)) hipLaunchKernelGGL(screen_rail_kernel, dim3(W, B), dim3(kThreads), 0, st, audio, ld_audio, audio_len, vec, a);
    hipLaunchKernelGGL(screen_flag_kernel, dim3(B), dim3(kScFlagThreads), 0, st, audio_len, a);
    return ispk_launch_status();
}
