// Declipper (no counterpart in the reference, whose corpus arrives curated): the clipped samples of a padded mono batch fp32
// [B][S] with int64 audio_len [B] (a length below 0 or above S counts as 0) are restored by Janssen's AR interpolation (Janssen,
// Veldhuis & Vries 1986) in float64.  include/ispk.h has the definition; tests/declip_reference.py restates it in numpy.
//
//   declip_peak_kernel    grid (ceil(S / 4096), B), 256 threads: the tile's max |x| (a non-finite sample reads as 0) to the workspace.
//   declip_thr_kernel     grid (B): the item's peak over its tiles, thr = peak * rail_ratio or the given rail (Screen's, value for
//                         value).
//   declip_solve_kernel   grid (ceil(S / 512), B), 256 threads.  A workgroup owns the segment [512 j, 512 j + 512) of one item and
//                         writes exactly those output samples (zeros at or past the length).  Every lane holds two of them.  No
//                         sample of the segment at the rail, or an item whose incoming flags lack bit 1: the registers go back
//                         out (8-byte loads and stores where both rows allow) - the whole cost on clean audio.  Otherwise the window
//                         [512 j - 256, 512 j + 768) is staged in float64 with the classes of 63 more samples on either side: a
//                         sample at the rail is unknown iff its run has at least min_run samples, which its left and right extents,
//                         each capped at min_run, decide - no scan across segments.  The unknown positions are compacted in order
//                         (a wave scan, the waves in order).  None in the own segment: a copy.  More than 256 in the window: dense,
//                         a copy.  Else `iterations` passes of
//                           autocorrelation   lag k on wave k mod 4, lanes stride the window, a butterfly;
//                           Levinson-Durbin   wave 0, lane j holds a[j] and r[j], the cross terms by shuffles;
//                           b[k]              lanes 0 .. order;
//                           band and rhs      B_UU's lower band [m][33] from the index distances; one lane per unknown runs its
//                                             <= 65 taps over the known neighbours;
//                           Cholesky          left-looking, column by column: eight lanes per row of the column share its <= 32
//                                             products (a three-step butterfly), two barriers a column;
//                           two solves        wave 0, column-oriented: lane l carries the pending sum of row i +- l, one shuffle
//                                             a row hands it on - no reduction on the chain;
//                           consistency       w[u] = s max(s x_u, s orig_u).
//                         A pivot that is not positive, a prediction error that is not positive or a non-finite solution makes
//                         the segment dense.  The segment's own unknowns are rounded once to fp32; every other sample keeps its
//                         bits.  The segment's counts and output peak go to the workspace.
//   declip_item_kernel    grid (B): the segments' counts and peaks in a fixed order, the flags.
//
// LDS of declip_solve_kernel (all dynamic, every offset a multiple of 16): window 8,192 B, band 67,584 B (the staged classes lie
// in it before the band is built), rhs 2,048, r / a / b 960, the unknowns' clipped values 1,024, their positions 512, the unknown
// mask 1,024, 64 B of words = 81,408 B: two workgroups (8 waves) per CU of 160 KiB.
// Bits.  Every sum runs in an order fixed by the window alone; no atomics.  An item's results depend on that item alone - not on
// B, S, the row strides, the alignment or what lies behind its length.
//
// gfx950 resources (csrc/resource_report.py declip.hip; no spills, no scratch):
//   declip_peak_kernel    8 VGPRs, LDS 16 B          declip_thr_kernel    15 VGPRs, LDS 16 B
//   declip_solve_kernel   64 VGPRs, LDS 81,408 B dynamic, none static (two workgroups per CU)
//   declip_item_kernel    32 VGPRs, LDS 112 B
#include <math.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int kDcSeg = 512, kDcHalo = 256, kDcWin = kDcSeg + 2 * kDcHalo;       // H, the overlap on either side, N <= 1024
constexpr int kDcMaxU = 256;                                                  // DECLIP_MAX_UNKNOWNS
constexpr int kDcMaxOrder = 32, kDcLd = kDcMaxOrder + 1;                       // band row: the diagonal and 32 sub-diagonals
constexpr int kDcMaxRun = 64, kDcMaxIter = 8;
constexpr int kDcSide = kDcMaxRun - 1;                                         // classes staged on either side of the window
constexpr int kDcCls = kDcWin + 2 * kDcSide;                                   // 1,150
constexpr int kDcThreads = 256, kDcWaves = kDcThreads / kWave;
constexpr int kDcTile = 4096;                                                  // samples per workgroup of the peak pass
constexpr int kDcMaxSamples = 1 << 24;                                         // CONDITION_MAX_SAMPLES
constexpr int kDcCoef = 40;                                                    // r, a, b: 33 values each in 40 slots

constexpr int kOffWin = 0;
constexpr int kOffBand = kOffWin + 8 * kDcWin;
constexpr int kOffRhs = kOffBand + 8 * kDcMaxU * kDcLd;
constexpr int kOffCoef = kOffRhs + 8 * kDcMaxU;
constexpr int kOffOrig = kOffCoef + 8 * 3 * kDcCoef;
constexpr int kOffIdx = kOffOrig + 4 * kDcMaxU;
constexpr int kOffUnk = kOffIdx + 2 * kDcMaxU;
constexpr int kOffWords = kOffUnk + kDcWin;
constexpr int kDcLds = kOffWords + 64;
static_assert(kDcLds == 81408 && 2 * kDcLds <= 160 * 1024, "two workgroups per CU; the header above and DESIGN.md 4.35 quote this");
static_assert(kOffBand % 16 == 0 && kOffRhs % 16 == 0 && kOffCoef % 16 == 0 && kOffOrig % 16 == 0 && kOffIdx % 16 == 0 &&
                  kOffUnk % 16 == 0 && kOffWords % 16 == 0, "carve offsets");
static_assert(kDcCls <= 8 * kDcMaxU * kDcLd, "the staged classes lie in the band");
static_assert(kDcThreads == kDcMaxU && kDcThreads * 4 == kDcWin && kDcThreads * 2 == kDcSeg && kDcThreads == 8 * kDcMaxOrder,
              "one lane per unknown, four window samples and two own samples per lane, eight lanes per row of a column");

struct SegRec {
    int clip, restored, state;                             // state 0: a copy, 1: solved, 2: dense
    float peak;                                            // of the segment's output
};
static_assert(sizeof(SegRec) == 16, "two workspace words");

struct DeclipArgs {
    int S, W4, J, rail_mode, min_run, order, iterations;
    float rail, rail_ratio;
    int64_t per_item;                                      // workspace words per item
    double* ws;
    const int32_t* in_flags;
    float *thr, *peak;
    int64_t *out_len, *clip_samples, *restored;
    int32_t *windows, *dense, *flags;
};

// the item's workspace: SegRec [J], then the peak partials float [W4]
__device__ __forceinline__ SegRec* ws_rec(const DeclipArgs& a, int b) { return reinterpret_cast<SegRec*>(a.ws + (int64_t)b * a.per_item); }
__device__ __forceinline__ float* ws_part(const DeclipArgs& a, int b) { return reinterpret_cast<float*>(ws_rec(a, b) + a.J); }

__device__ __forceinline__ bool dc_skipped(const DeclipArgs& a, int b) { return a.in_flags && !(a.in_flags[b] & 1); }

__global__ __launch_bounds__(kDcThreads) void declip_peak_kernel(const float* __restrict__ audio, int64_t ld, const int64_t* __restrict__ audio_len,
                                                                 int vec, const DeclipArgs a) {
    __shared__ float red[kDcWaves];
    const int tid = threadIdx.x, w = blockIdx.x, b = blockIdx.y;
    const int n = valid_len(audio_len, b, a.S), base = w * kDcTile;
    if (base >= n) return;                                  // (uniform) the item reduction reads the tiles below the length only
    const float* row = audio + (int64_t)b * ld;
    float pk = 0.f;
#pragma unroll
    for (int q = 0; q < kDcTile / (4 * kDcThreads); ++q) {
        const int i = base + 4 * (tid + q * kDcThreads);
        if (vec && i + 4 <= n) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + i);
            pk = fmaxf(pk, fmaxf(fmaxf(fabsf(finite_or_zero(v.x)), fabsf(finite_or_zero(v.y))), fmaxf(fabsf(finite_or_zero(v.z)), fabsf(finite_or_zero(v.w)))));
        } else {
            for (int e = 0; e < 4; ++e)
                if (i + e < n) pk = fmaxf(pk, fabsf(finite_or_zero(row[i + e])));
        }
    }
    pk = wave_max(pk);
    if (tid % kWave == 0) red[tid / kWave] = pk;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kDcWaves; ++k) pk = fmaxf(pk, red[k]);
        ws_part(a, b)[w] = pk;
    }
}

__global__ __launch_bounds__(kDcThreads) void declip_thr_kernel(const int64_t* __restrict__ audio_len, const DeclipArgs a) {
    __shared__ float red[kDcWaves];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n = valid_len(audio_len, b, a.S), Wn = (n + kDcTile - 1) / kDcTile;
    const float* part = ws_part(a, b);
    float pk = 0.f;
    for (int w = tid; w < Wn; w += kDcThreads) pk = fmaxf(pk, part[w]);
    pk = wave_max(pk);
    if (tid % kWave == 0) red[tid / kWave] = pk;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kDcWaves; ++k) pk = fmaxf(pk, red[k]);
        a.thr[b] = a.rail_mode ? a.rail : pk * a.rail_ratio;
    }
}

__global__ __launch_bounds__(kDcThreads) void declip_solve_kernel(const float* __restrict__ audio, int64_t ld, const int64_t* __restrict__ audio_len,
                                                                  float* __restrict__ out, int64_t ldo, int vec, const DeclipArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    double* win = reinterpret_cast<double*>(lds + kOffWin);
    double* band = reinterpret_cast<double*>(lds + kOffBand);
    signed char* cls = reinterpret_cast<signed char*>(lds + kOffBand);      // until the band is built
    double* rhs = reinterpret_cast<double*>(lds + kOffRhs);
    double* rr = reinterpret_cast<double*>(lds + kOffCoef);
    double* aa = rr + kDcCoef;
    double* bb = aa + kDcCoef;
    float* orig = reinterpret_cast<float*>(lds + kOffOrig);
    unsigned short* idx = reinterpret_cast<unsigned short*>(lds + kOffIdx);
    unsigned char* unk = lds + kOffUnk;
    int* mi = reinterpret_cast<int*>(lds + kOffWords);     // [0, 4) the waves' unknowns, [4, 8) their own-segment unknowns, 8: failed
    float* mf = reinterpret_cast<float*>(mi + 12);         // [0, 4) the waves' peaks

    const int tid = threadIdx.x, lane = tid % kWave, wv = tid / kWave, j = blockIdx.x, b = blockIdx.y;
    const int n = valid_len(audio_len, b, a.S);
    const int s0 = j * kDcSeg, s1 = min(s0 + kDcSeg, a.S);  // this workgroup writes out[s0, s1)
    const float* row = audio + (int64_t)b * ld;
    float* orow = out + (int64_t)b * ldo;
    const float thr = a.thr[b];
    const int order = a.order, mr = a.min_run;

    // the lane's two samples of the segment, bits as they are; 0 at or past the length
    const int p = s0 + 2 * tid;
    float v0 = 0.f, v1 = 0.f;
    if (vec && p + 2 <= n) {
        const f32x2 t = *reinterpret_cast<const f32x2*>(row + p);
        v0 = t.x, v1 = t.y;
    } else {
        if (p < n) v0 = row[p];
        if (p + 1 < n) v1 = row[p + 1];
    }

    // writes the lane's two samples, then the segment's record (the output's peak with non-finite samples read as 0)
    auto finish = [&](int clip, int restored, int state) {
        if (vec && p + 2 <= s1) {
            f32x2 t;
            t.x = v0, t.y = v1;
            *reinterpret_cast<f32x2*>(orow + p) = t;
        } else {
            if (p < s1) orow[p] = v0;
            if (p + 1 < s1) orow[p + 1] = v1;
        }
        const float pk = wave_max(fmaxf(fabsf(finite_or_zero(v0)), fabsf(finite_or_zero(v1))));
        if (lane == 0) mf[wv] = pk;
        __syncthreads();
        if (tid == 0 && s0 < n) {
            SegRec r;
            r.clip = clip, r.restored = restored, r.state = state;
            r.peak = fmaxf(fmaxf(mf[0], mf[1]), fmaxf(mf[2], mf[3]));
            ws_rec(a, b)[j] = r;
        }
    };

    const float f0 = finite_or_zero(v0), f1 = finite_or_zero(v1);
    const int at = thr > 0.f && (fabsf(f0) >= thr || fabsf(f1) >= thr) && !dc_skipped(a, b);
    if (tid == 0) mi[8] = 0;
    const int wave_at = __any(at);
    if (lane == 0) mi[wv] = wave_at;
    __syncthreads();
    if (!(mi[0] | mi[1] | mi[2] | mi[3])) {                 // (uniform) nothing at the rail in the segment: the copy
        finish(0, 0, 0);
        return;
    }

    // the window in float64 and the classes of the window and kDcSide samples on either side
    const int lo = max(s0 - kDcHalo, 0), hi = min(s0 + kDcSeg + kDcHalo, n), N = hi - lo, hb = lo - kDcSide;
    for (int k = tid; k < kDcCls; k += kDcThreads) {
        const int g = hb + k;
        float x = 0.f;
        if (g >= 0 && g < n) x = finite_or_zero(row[g]);
        cls[k] = x >= thr ? 1 : x <= -thr ? 2 : 0;          // (thr > 0 here; 0 outside the item)
        if (k >= kDcSide && k < kDcSide + N) win[k - kDcSide] = (double)x;
    }
    __syncthreads();

    // unknown: a sample at the rail whose run has at least min_run samples - the extents to either side, capped
    int u[4], cnt = 0, own = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = 4 * tid + q;
        u[q] = 0;
        if (i < N) {
            const int k = i + kDcSide, c = cls[k];
            if (c) {
                int L = 1, R = 1;
                while (L < mr && cls[k - L] == c) ++L;
                while (L + R - 1 < mr && cls[k + R] == c) ++R;
                u[q] = L + R - 1 >= mr;
            }
        }
        cnt += u[q];
        own += u[q] && lo + i >= s0 && lo + i < s0 + kDcSeg;
    }
    int inc = cnt;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int t = __shfl_up(inc, off, kWave);
        if (lane >= off) inc += t;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) own += __shfl_xor(own, off, kWave);
    if (lane == kWave - 1) mi[wv] = inc;
    if (lane == 0) mi[4 + wv] = own;
    __syncthreads();
    int pos = inc - cnt;
    for (int w = 0; w < wv; ++w) pos += mi[w];
    const int m = mi[0] + mi[1] + mi[2] + mi[3], ownT = mi[4] + mi[5] + mi[6] + mi[7];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = 4 * tid + q;
        unk[i] = (unsigned char)u[q];
        if (u[q]) {
            if (pos < kDcMaxU) idx[pos] = (unsigned short)i, orig[pos] = (float)win[i];
            ++pos;
        }
    }
    if (ownT == 0 || m > kDcMaxU) {                         // (uniform) nothing of its own to solve, or too much to solve
        finish(ownT, 0, ownT ? 2 : 0);
        return;
    }
    __syncthreads();                                        // idx, orig, unk; the classes are read

    for (int it = 0; it < a.iterations; ++it) {
        // 1. r[k] = sum w[i] w[i + k]
        for (int k = wv; k <= order; k += kDcWaves) {
            double s = 0.0;
            for (int i = lane; i < N - k; i += kWave) s = fma(win[i], win[i + k], s);
            s = wave_sum(s);
            if (lane == 0) rr[k] = k == 0 ? s * (1.0 + 1e-9) : s;
        }
        __syncthreads();
        if (rr[0] == 0.0) break;                            // (uniform) an all-zero window
        // 2. Levinson-Durbin: lane l holds a[l] and r[l]
        if (wv == 0) {
            const double rl = lane <= order ? rr[lane] : 0.0;
            double al = lane == 0 ? 1.0 : 0.0, e = rr[0];
            bool bad = false;
            for (int i = 1; i <= order; ++i) {
                const int src = (i - lane) & (kWave - 1);
                const bool in = lane >= 1 && lane < i;
                const double rv = __shfl(rl, src, kWave), av = __shfl(al, src, kWave);
                const double acc = wave_sum(in ? al * rv : 0.0) + __shfl(rl, i, kWave);
                const double k = -acc / e;
                if (in) al = fma(k, av, al);
                if (lane == i) al = k;
                e *= 1.0 - k * k;
                bad |= !(e > 0.0);
            }
            if (lane <= order) aa[lane] = al;
            if (lane == 0 && bad) mi[8] = 1;
        }
        __syncthreads();
        // 3. b[k] = sum a[i] a[i + k]
        if (tid <= order) {
            double s = 0.0;
            for (int i = 0; i + tid <= order; ++i) s = fma(aa[i], aa[i + tid], s);
            bb[tid] = s;
        }
        __syncthreads();
        // 4. the lower band of B_UU and the right-hand side -B_UK x_K
        for (int e = tid; e < m * kDcLd; e += kDcThreads) {
            const int i = e / kDcLd, d = e % kDcLd, col = i - d;
            double v = 0.0;
            if (col >= 0 && d <= order) {
                const int dist = (int)idx[i] - (int)idx[col];
                if (dist <= order) v = bb[dist];
            }
            band[e] = v;
        }
        if (tid < m) {
            const int q = idx[tid], t1 = min(N - 1, q + order);
            double s = 0.0;
            for (int t = max(0, q - order); t <= t1; ++t)
                if (!unk[t]) s = fma(bb[abs(t - q)], win[t], s);
            rhs[tid] = -s;
        }
        __syncthreads();
        // banded Cholesky, left-looking: column jc from the columns before it; eight lanes share a row's products
        {
            const int d = tid >> 3, part = tid & 7;
            for (int jc = 0; jc < m; ++jc) {
                const int ri = jc + d;
                const bool act = d < order && ri < m;
                double s = 0.0;
                if (act)
                    for (int c = part + 1; c <= order - d; c += 8) s = fma(band[ri * kDcLd + d + c], band[jc * kDcLd + c], s);
                s += __shfl_xor(s, 1, kWave);
                s += __shfl_xor(s, 2, kWave);
                s += __shfl_xor(s, 4, kWave);
                double t = 0.0;
                if (act && part == 0) {
                    t = band[ri * kDcLd + d] - s;
                    if (d == 0) {
                        if (!(t > 0.0)) mi[8] = 1;
                        t = sqrt(t);
                        band[jc * kDcLd] = t;
                    }
                }
                __syncthreads();
                const double ljj = band[jc * kDcLd];
                if (act && part == 0 && d > 0) band[ri * kDcLd + d] = t / ljj;
                if (tid == 1 && jc + order < m) band[(jc + order) * kDcLd + order] /= ljj;      // the row without products
                __syncthreads();
            }
        }
        // L y = rhs, then L^T x = y: lane l carries the pending sum of row i + l (i - l), handed on by one shuffle a row
        if (wv == 0) {
            double acc = 0.0;
            for (int i = 0; i < m; ++i) {
                double y = (rhs[i] - acc) / band[i * kDcLd];
                y = __shfl(y, 0, kWave);
                if (lane == 0) rhs[i] = y;
                if (lane >= 1 && lane <= order && i + lane < m) acc = fma(band[(i + lane) * kDcLd + lane], y, acc);
                acc = __shfl_down(acc, 1, kWave);
                if (lane == kWave - 1) acc = 0.0;
            }
            acc = 0.0;
            for (int i = m - 1; i >= 0; --i) {
                double x = (rhs[i] - acc) / band[i * kDcLd];
                x = __shfl(x, 0, kWave);
                if (lane == 0) rhs[i] = x;
                if (lane >= 1 && lane <= order && i - lane >= 0) acc = fma(band[i * kDcLd + lane], x, acc);
                acc = __shfl_down(acc, 1, kWave);
                if (lane == kWave - 1) acc = 0.0;
            }
        }
        __syncthreads();
        // 5. consistent with the clipping: never inside the rail
        if (tid < m) {
            const double x = rhs[tid], o = (double)orig[tid];
            if (!(fabs(x) <= 1.7976931348623157e308)) mi[8] = 1;
            win[idx[tid]] = o > 0.0 ? fmax(x, o) : fmin(x, o);
        }
        __syncthreads();
        if (mi[8]) break;                                   // (uniform)
    }
    if (mi[8]) {                                            // (uniform) a non-finite intermediate: left as it is
        finish(ownT, 0, 2);
        return;
    }
    if (p < n && unk[p - lo]) v0 = (float)win[p - lo];
    if (p + 1 < n && unk[p + 1 - lo]) v1 = (float)win[p + 1 - lo];
    finish(ownT, ownT, 1);
}

__global__ __launch_bounds__(kDcThreads) void declip_item_kernel(const int64_t* __restrict__ audio_len, const DeclipArgs a) {
    __shared__ long long red_l[2 * kDcWaves];
    __shared__ int red_i[2 * kDcWaves];
    __shared__ float red_f[kDcWaves];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n = valid_len(audio_len, b, a.S), Jn = (n + kDcSeg - 1) / kDcSeg;
    const SegRec* rec = ws_rec(a, b);
    long long clip = 0, rest = 0;
    int solved = 0, dense = 0;
    float pk = 0.f;
    for (int j = tid; j < Jn; j += kDcThreads) {
        const SegRec r = rec[j];
        clip += r.clip, rest += r.restored, solved += r.state == 1, dense += r.state == 2, pk = fmaxf(pk, r.peak);
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        clip += __shfl_xor(clip, off, kWave);
        rest += __shfl_xor(rest, off, kWave);
        solved += __shfl_xor(solved, off, kWave);
        dense += __shfl_xor(dense, off, kWave);
        pk = fmaxf(pk, __shfl_xor(pk, off, kWave));
    }
    if (tid % kWave == 0) {
        const int w = tid / kWave;
        red_l[w] = clip, red_l[kDcWaves + w] = rest, red_i[w] = solved, red_i[kDcWaves + w] = dense, red_f[w] = pk;
    }
    __syncthreads();
    if (tid == 0) {
        clip = 0, rest = 0, solved = 0, dense = 0, pk = 0.f;
        for (int k = 0; k < kDcWaves; ++k)
            clip += red_l[k], rest += red_l[kDcWaves + k], solved += red_i[k], dense += red_i[kDcWaves + k], pk = fmaxf(pk, red_f[k]);
        a.out_len[b] = n, a.peak[b] = pk, a.clip_samples[b] = clip, a.restored[b] = rest, a.windows[b] = solved, a.dense[b] = dense;
        a.flags[b] = (rest > 0 ? 1 : 0) | (dense > 0 ? 2 : 0) | (dc_skipped(a, b) ? 4 : 0);
    }
}

int64_t declip_words(int S) {
    const int64_t J = std::max(1, (S + kDcSeg - 1) / kDcSeg), W4 = std::max(1, (S + kDcTile - 1) / kDcTile);
    return 2 * J + (W4 + 1) / 2;
}

}  // namespace

extern "C" int32_t ispk_declip_max_unknowns(void) { return kDcMaxU; }

extern "C" int32_t ispk_declip_workspace_bytes(int32_t B, int32_t S, int64_t* bytes) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= kDcMaxSamples, ISPK_E_SHAPE,
                 "ispk_declip_workspace_bytes: bad shape B=%d S=%d (B <= 65535, 0 <= S <= 2^24)", B, S);
    ISPK_REQUIRE(bytes, ISPK_E_NULL, "ispk_declip_workspace_bytes: null pointer");
    *bytes = 8 * (int64_t)B * declip_words(S);
    return 0;
}

extern "C" int32_t ispk_declip_f64(const float* audio, int64_t ld_audio, const int64_t* audio_len, const int32_t* in_flags, int32_t rail_mode,
                                   float rail, float rail_ratio, int32_t min_run, int32_t order, int32_t iterations, float* out,
                                   int64_t ld_out, int64_t* out_len, float* thr, float* peak, int64_t* clip_samples, int64_t* restored,
                                   int32_t* windows, int32_t* dense, int32_t* flags, void* workspace, int64_t workspace_bytes, int32_t B,
                                   int32_t S, ispk_stream_t stream) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= kDcMaxSamples, ISPK_E_SHAPE,
                 "ispk_declip_f64: bad shape B=%d S=%d (B <= 65535, 0 <= S <= 2^24)", B, S);
    ISPK_REQUIRE((rail_mode == 0 && rail_ratio > 0.f && rail_ratio <= 1.f) || (rail_mode == 1 && rail > 0.f && isfinite(rail)), ISPK_E_SHAPE,
                 "ispk_declip_f64: bad rail mode %d with rail %g, rail_ratio %g (mode 0: 0 < ratio <= 1; mode 1: a positive finite rail)",
                 rail_mode, (double)rail, (double)rail_ratio);
    ISPK_REQUIRE(min_run >= 1 && min_run <= kDcMaxRun && order >= 1 && order <= kDcMaxOrder && iterations >= 1 && iterations <= kDcMaxIter,
                 ISPK_E_SHAPE, "ispk_declip_f64: min_run %d outside 1 .. %d, order %d outside 1 .. %d or iterations %d outside 1 .. %d", min_run,
                 kDcMaxRun, order, kDcMaxOrder, iterations, kDcMaxIter);
    if (B == 0) return 0;
    ISPK_REQUIRE(audio && audio_len && out && out_len && thr && peak && clip_samples && restored && windows && dense && flags && workspace,
                 ISPK_E_NULL, "ispk_declip_f64: null pointer");
    ISPK_REQUIRE(ld_audio >= S && ld_out >= S, ISPK_E_SHAPE, "ispk_declip_f64: row stride %lld or %lld below S=%d", (long long)ld_audio,
                 (long long)ld_out, S);
    {   // out of place only: the neighbouring windows read each other's clipped values
        const uintptr_t a0 = (uintptr_t)audio, a1 = a0 + 4 * ((uint64_t)(B - 1) * ld_audio + S);
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + 4 * ((uint64_t)(B - 1) * ld_out + S);
        ISPK_REQUIRE(S == 0 || a1 <= o0 || o1 <= a0, ISPK_E_SHAPE, "ispk_declip_f64: out overlaps audio (out of place only)");
    }
    const int64_t words = declip_words(S);
    ISPK_REQUIRE(workspace_bytes >= 8 * (int64_t)B * words && ispk_aligned(workspace, 8), ISPK_E_ALIGN,
                 "ispk_declip_f64: the workspace needs %lld bytes at an 8-byte boundary, got %lld", (long long)(8 * (int64_t)B * words),
                 (long long)workspace_bytes);
    ISPK_RESERVE_LDS(declip_solve_kernel, kDcLds, "ispk_declip_f64");
    DeclipArgs a;
    a.S = S, a.W4 = std::max(1, (S + kDcTile - 1) / kDcTile), a.J = std::max(1, (S + kDcSeg - 1) / kDcSeg);
    a.rail_mode = rail_mode, a.min_run = min_run, a.order = order, a.iterations = iterations, a.rail = rail, a.rail_ratio = rail_ratio;
    a.per_item = words, a.ws = reinterpret_cast<double*>(workspace), a.in_flags = in_flags;
    a.thr = thr, a.peak = peak, a.out_len = out_len, a.clip_samples = clip_samples, a.restored = restored;
    a.windows = windows, a.dense = dense, a.flags = flags;
    const int vec4 = ld_audio % 4 == 0 && ispk_aligned(audio, 16);
    const int vec2 = ld_audio % 2 == 0 && ld_out % 2 == 0 && ispk_aligned(audio, 8) && ispk_aligned(out, 8);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned W4 = (unsigned)((S + kDcTile - 1) / kDcTile), J = (unsigned)((S + kDcSeg - 1) / kDcSeg);
    if (W4) hipLaunchKernelGGL(declip_peak_kernel, dim3(W4, B), dim3(kDcThreads), 0, st, audio, ld_audio, audio_len, vec4, a);
    hipLaunchKernelGGL(declip_thr_kernel, dim3(B), dim3(kDcThreads), 0, st, audio_len, a);
    if (J) hipLaunchKernelGGL(declip_solve_kernel, dim3(J, B), dim3(kDcThreads), kDcLds, st, audio, ld_audio, audio_len, out, ld_out, vec2, a);
    hipLaunchKernelGGL(declip_item_kernel, dim3(B), dim3(kDcThreads), 0, st, audio_len, a);
    return ispk_launch_status();
}
