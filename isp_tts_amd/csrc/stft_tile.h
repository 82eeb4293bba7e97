// The 1024 / 256 STFT tile: the frame machinery under the Vocos ISTFT head (vocoder.hip), the denoiser (denoise.hip) and
// Griffin-Lim (griffinlim.hip); the noise reducer and the phase vocoder (noise.hip, stretch.hip) run on it too, and the screen
// and the noise profile on its analysis-only half.  n_fft = win = 1024, hop 256, 513 bins; this header is the only place that
// knows the tile, and what a kernel does with a frame (its prologue, shrink, projection, error sums) stays in its own file.
//
// Tile.  Grid (ceil(samples / 4096), B), 512 threads = kGroups = 4 groups of kGT = 128.  A workgroup writes kSegs = 16 hop
// segments (kTile = 4096 samples) of ONE utterance.  With `pad` samples in front of the signal (384 or 512, the caller's framing),
// sample s takes frames floor((s + pad) / 256) - 3 .. floor((s + pad) / 256), so the tile at hop q0 needs up to 20 frames (q0 - 2
// .. q0 + 17 at pad 384, q0 - 1 .. q0 + 17 at pad 512) within the utterance's own.  The frames it shares with a neighbouring
// tile are transformed by both: no atomics, no second pass, nothing in HBM between analysis and synthesis.  Frames run four at a
// time, one per group (a round), each through 512-point complex Stockham FFTs (fft.h: the real transform of 1024 points as a
// half-length complex one), and an inverse lands in the frame's 4 KB slot: z[m] = x[2m] + i x[2m+1] is the frame's 1024 real
// samples in order.  A group whose slot index is at or past the frame count still runs its round on zeros (its slot is
// never read), so that every barrier is reached by all four groups.  Then overlap_add() sums each output sample's <= 4 frames.
//
// LDS (dynamic, kLds = 110,592 B, so one workgroup of 8 waves per CU): 8 KB twiddles W_1024^m, 16 KB of ping buffers (4 groups
// x 512 float2), 4 KB window, 80 KB of frame slots (kSlots = 20 x 1024 floats).  A kernel may keep floats of its own between
// the window and the slots (carve_tile's `extra`; the denoiser's 516 thresholds make 112,656 B).
//
// Banks.  Every wave belongs to one transform, so running four side by side changes no LDS access pattern: the float2 passes
// read conflict-free (32 consecutive float2 = the 64 banks) and the stores of the first two radix-4 passes (strides of 4 and 16
// float2 inside a 16-lane group, banks modulo 32) are 4-way; the later passes store runs of 16 consecutive float2.  Four groups
// keep two waves per SIMD to overlap those stores with the other groups' arithmetic.
//
// Bits.  A frame's arithmetic depends on the utterance's length n and the frame index f alone (and on what the caller's
// per-bin step reads: a seed, a strength), and a sample's on (n, s) alone - not on the tile, on B, on the padded length or on
// the row's neighbours.  Every sum runs in a fixed order (overlap-add in ascending frame order) and there are no atomics: a
// ragged batch gives each utterance the bits it gets alone, and repeated calls and graph replays repeat theirs.
//
// To change the tile (kSegs, kSlots, kGroups), keep:
//   - kSlots >= the frames that touch a tile (kSegs + 3 + one more when pad is no multiple of the hop), rounded up to a
//     multiple of kGroups: the round loop writes slot r * kGroups + g for every g;
//   - kLds plus a caller's extra floats under the 160 KB of a CU;
//   - every __syncthreads() reached by all kGroups groups: nothing between the table load and the end of the rounds may be
//     skipped per group (dead groups transform zeros instead);
//   - kTw = 1024 and kHalf = 512 are what fft.h's five passes and real_split expect of these callers.
#pragma once
#include "fft.h"

constexpr int kHop = 256;
constexpr int kNfft = 1024;
constexpr int kHalf = kNfft / 2;                   // 512: the complex transform's length
constexpr int kBins = kHalf + 1;                   // 513
constexpr int kSegs = 16;                          // hop segments written per workgroup
constexpr int kTile = kSegs * kHop;                // 4096 samples
constexpr int kSlots = kSegs + 4;                  // frame slots: up to 20 frames touch a tile, five whole rounds
constexpr int kGroups = 4;                         // transforms side by side
constexpr int kGT = 128;                           // threads per transform
constexpr int kThreads = kGroups * kGT;
constexpr int kTw = 1024;                          // W_1024^m: the 512-point FFT's twiddles, the split's and the merge's
constexpr int kTableFloats = 2 * 2048 + kNfft;     // a caller's table: data.features.twiddles() (W_2048), then the window
constexpr size_t kLds = sizeof(cf) * (kTw + kGroups * kHalf) + sizeof(float) * (kNfft + kSlots * kNfft);
static_assert(kSlots % kGroups == 0 && kSlots >= kSegs + 4, "slots: every frame touching a tile, in whole rounds");
static_assert(kLds == 110592, "the resource lines of vocoder.hip, denoise.hip and griffinlim.hip quote this");

struct TileLds {
    cf* tw;                                        // [kTw]
    cf* ping;                                      // [kGroups][512]
    float* win;                                    // [1024], then the caller's `extra` floats (even: the slots are float2)
    float* frames;                                 // [kSlots][1024]
};

__device__ __forceinline__ TileLds carve_tile(void* lds_raw, int extra = 0) {
    TileLds t;
    t.tw = reinterpret_cast<cf*>(lds_raw);
    t.ping = t.tw + kTw;
    t.win = reinterpret_cast<float*>(t.ping + kGroups * kHalf);
    t.frames = t.win + kNfft + extra;
    return t;
}

// tw = W_1024^m (every second entry of the table's W_2048), win = the table's window; the caller's barrier follows
__device__ __forceinline__ void load_tables(cf* tw, float* win, const float* __restrict__ tables, int tid) {
    const cf* tw2048 = reinterpret_cast<const cf*>(tables);
    for (int i = tid; i < kTw; i += kThreads) tw[i] = tw2048[2 * i];
    for (int i = tid; i < kNfft; i += kThreads) win[i] = tables[2 * 2048 + i];
}

// A[m] = (x[i0 + 2m], x[i0 + 2m + 1]) times the window, m < 512, by the group's 128 threads: the frame's 1024 samples as the
// half-length complex sequence.  x is `sample(i)` for i inside [0, n) of a live frame and 0 elsewhere - a select, so sample()
// never sees an index outside the utterance.  n >= 0, so one unsigned compare covers both ends of the range.
template <typename F>
__device__ __forceinline__ void gather_zero_padded(cf* A, const float* win, int i0, int n, bool live, int lt, F&& sample) {
    for (int m = lt; m < kHalf; m += kGT) {
        const int ia = i0 + 2 * m, ib = ia + 1;
        const float xa = live && (unsigned)ia < (unsigned)n ? sample(ia) : 0.f;
        const float xb = live && (unsigned)ib < (unsigned)n ? sample(ib) : 0.f;
        A[m] = make_float2(xa * win[2 * m], xb * win[2 * m + 1]);
    }
}

// The same A for frame f of a center = true framing with reflect padding: x[r(256 f - 512 + j)], r the reflection at 0 and
// n - 1 (n >= 513 and 0 <= f < 1 + n / 256 keep every index inside [0, n)).  Reads HBM: the reflected ends are no tile's own.
__device__ __forceinline__ void gather_reflected(cf* A, const float* win, const float* __restrict__ xrow, int f, int n, int lt) {
    const int i0 = f * kHop - kHalf;
    for (int m = lt; m < kHalf; m += kGT) {
        int ia = i0 + 2 * m, ib = ia + 1;
        ia = ia < 0 ? -ia : ia >= n ? 2 * (n - 1) - ia : ia;
        ib = ib < 0 ? -ib : ib >= n ? 2 * (n - 1) - ib : ib;
        A[m] = make_float2(xrow[ia] * win[2 * m], xrow[ib] * win[2 * m + 1]);
    }
}

// The analysis-only tile (the screen, the noise profile): no synthesis side, so instead of the kSlots frame slots the tile's
// kAnalysisStage = 4,864 samples - 16 frames of 1024 every 256 - staged once behind the window (carve_tile's `extra`), and one
// 4 KB pong slot per group behind them: 64,512 B, two workgroups per CU.
constexpr int kAnalysisStage = kTile + kNfft - kHop;
constexpr size_t kAnalysisLds = sizeof(cf) * (kTw + kGroups * kHalf) + sizeof(float) * (kNfft + kAnalysisStage + kGroups * kNfft);
static_assert(kAnalysisStage % 4 == 0, "float4 staging; the pong slots behind the staged samples are float2");

// xs[j] = x(base + j) for j < count (a multiple of 4, as base is: a row that allows float4 loads allows them here), 0 outside
// [0, n); nothing outside [0, n) is read.  base may be negative (a centred framing's first tile).
__device__ __forceinline__ void stage_flat(float* xs, const float* __restrict__ row, int base, int n, int count, int vec, int tid) {
    for (int q = tid; q < count / 4; q += kThreads) {
        const int i = base + 4 * q;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (vec && i >= 0 && i + 4 <= n) {
            v = *reinterpret_cast<const f32x4*>(row + i);
        } else {
            if (i >= 0 && i < n) v.x = row[i];
            if (i + 1 >= 0 && i + 1 < n) v.y = row[i + 1];
            if (i + 2 >= 0 && i + 2 < n) v.z = row[i + 2];
            if (i + 3 >= 0 && i + 3 < n) v.w = row[i + 3];
        }
        *reinterpret_cast<f32x4*>(xs + 4 * q) = v;
    }
}

// a dead group's round: an all-zero half-length spectrum (or sequence)
__device__ __forceinline__ void clear_frame(cf* A, int lt) {
    for (int m = lt; m < kHalf; m += kGT) A[m] = make_float2(0.f, 0.f);
}

// The group's 257 bin pairs (k, 512 - k), k <= 256, of Y / 1024 into the half-length spectrum of the inverse transform:
// Z_k = (Y_k + conj Y_{512-k}) + i (Y_k - conj Y_{512-k}) conj(W_1024^k), and Z_{512-k} likewise (the real inverse as a
// 512-point complex one).  pair(k, m, xk, xm) is the caller's per-bin step: it sets xk = Y_k / 1024 and xm = Y_m / 1024,
// m = 512 - k (the same bin at k = 256; a caller that reads HBM per bin issues both loads before it computes).  The imaginary
// parts of bins 0 and 512 are dropped, as irfft does.  griffinlim.hip writes this loop out in its kernel: keep the two alike.
template <typename F>
__device__ __forceinline__ void pack_pairs(cf* A, int lt, const cf* tw, F&& pair) {
    for (int k = lt; k <= 256; k += kGT) {
        const int m = kHalf - k;
        cf xk, xm;
        pair(k, m, xk, xm);
        if (k == 0) {
            xk.y = 0.f;
            xm.y = 0.f;
        }
        {   // Z_k
            const cf e = make_float2(xk.x + xm.x, xk.y - xm.y), d = make_float2(xk.x - xm.x, xk.y + xm.y);
            const cf o = ctw<true>(d, tw[k]);
            A[k] = make_float2(e.x - o.y, e.y + o.x);
        }
        if (k > 0 && k < 256) {   // Z_{512-k}
            const cf e = make_float2(xm.x + xk.x, xm.y - xk.y), d = make_float2(xm.x - xk.x, xm.y + xk.y);
            const cf o = ctw<true>(d, tw[m]);
            A[m] = make_float2(e.x - o.y, e.y + o.x);
        }
    }
}

// Samples [m0, mv) of the tile: the window-weighted overlap-add of each sample's <= 4 frames among the utterance's own
// [0, n_frames), divided by the sum of their w^2, both in ascending frame order.  Slot 0 holds frame f_lo; `pad` is the
// number of samples in front of the signal in the framing (u = m + pad is the position in the padded signal).
__device__ __forceinline__ void overlap_add(float* __restrict__ orow, const float* frames, const float* win, int m0, int mv,
                                            int pad, int f_lo, int n_frames, int tid) {
    for (int m = m0 + tid; m < mv; m += kThreads) {
        const int u = m + pad;
        const int fmin = u >= kNfft ? (u - kNfft) / kHop + 1 : 0, fmax = min(n_frames - 1, u / kHop);
        float acc = 0.f, env = 0.f;
        for (int f = fmin; f <= fmax; ++f) {
            const int j = u - f * kHop;
            const float wj = win[j];
            acc = fmaf(frames[(f - f_lo) * kNfft + j], wj, acc);
            env = fmaf(wj, wj, env);
        }
        orow[m] = acc / env;
    }
}
