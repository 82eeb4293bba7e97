// NoiseReducer (isp_tts_amd/data/noise.py; no counterpart in the reference, whose corpus arrives clean): stationary noise
// reduction of a padded mono batch fp32 [B][S] with int64 audio_len [B] (a length below 0 or above S counts as 0).  The noise
// spectrum of a recording is learnt from its own pauses (the profile), then every frame is attenuated with a Wiener gain that is
// smoothed over time and frequency (the reduce).  include/ispk.h has the definitions.  The STFT is the denoiser's: 1024 / 256,
// periodic Hann, center = true with reflect padding, F = 1 + n / 256 frames.
//
// The profile, four launches, no atomics:
//   hop_sums_kernel    chunk_grid.h's: grid (ceil(S / 8192), B), the float64 hop sums into the item's workspace.  The trim
//                      frames are the header's one definition, so they are the conditioner's and the segmenter's bit for bit.
//   nz_plan_kernel     grid (B), 1,024 lanes.  p_t and their max, thr; every lane counts the active frames of its strip of
//                      consecutive frames, an exclusive scan turns that into cum[t] = the active frames before t; STFT frame f
//                      (trim frame t = f - 2) is a noise frame when 2 <= f <= n / 256 - 2 and cum[min(T, t + guard + 1)] ==
//                      cum[max(0, t - guard)].  Writes the mask, noise_frames, frames and flags.
//   nz_tile_kernel     grid (S / 4096 + 1, B), 512 lanes.  A workgroup owns the 16 frames f in [16 w, 16 w + 16); it compacts
//                      its noise frames in order, stages samples [4096 w - 512, 4096 w + 4352) in LDS (a noise frame lies wholly
//                      inside the item: no reflection) and runs them four at a time through fft.h as screen_tile_kernel does;
//                      lane k adds |X_f[k]|^2 (fp32) in frame order into its float64 sum, the tile's partial [513].  LDS is
//                      stft_tile.h's analysis-only layout (no synthesis side): 64,512 B, two workgroups per CU.
//   nz_item_kernel     grid (B): noise[k] = (the partials in tile order) / noise_frames, zeros below min_noise_frames.
//
// The reduce, one launch:
//   nz_reduce_kernel   the denoiser's tile (stft_tile.h: grid (ceil(S / 4096), B), the <= 19 frames f_lo .. f_hi - 1 that touch
//                      the tile, one 4 KB slot each) with the smoothed gain between analysis and synthesis.  Time smoothing
//                      needs the raw gains of Tt <= 2 frames on either side of a frame, so:
//                        halo     one round: the <= 2 Tt frames f_lo - Tt .. f_lo - 1 and f_hi .. f_hi + Tt - 1 that exist are
//                                 transformed (the frame slots, still free, are the pong buffers) and only their raw-gain rows
//                                 (smoothed over the bins) are kept - below in the ring, above in two rows of their own;
//                        forward  every frame of the tile into its slot (the half-length spectrum Z);
//                        inverse  round r (slots 4 r .. 4 r + 3) reads the gain rows of slots 4 r - 2 .. 4 r + 5.  They live in
//                                 a ring of 8 rows of 516 floats: each group first writes the raw gains of slot 4 r + 2 + g from
//                                 that slot's Z (untouched so far: the inverses have reached slot 4 r - 1) into a row of its
//                                 own, a barrier, smooths them over the bins into the ring over the row of slot 4 r - 6 + g
//                                 (last read a round ago), a barrier, then per bin pair G = the triangular mean over the rows
//                                 that exist (the smoothing is separable: bins first, then frames, each renormalised), Y = X G
//                                 / 1024 packed for the inverse (pack_pairs), the inverse into the slot.  Every raw gain is
//                                 computed once per tile, and a bin costs 2 Fk + 1 and 2 Tt + 1 LDS reads, not their product.
//                      then the overlap-add over the item's F frames.  Samples at or past n are written as 0; an item below 513
//                      samples, with flag bits 1 or 2, or with an index outside [0, P) is copied.  Dead groups transform zeros:
//                      every barrier is reached by all four.  Nothing at or past n is read.
//   LDS of the reduce: the tile's 110,592 B + 15 rows of 516 floats (beta * profile, the ring of 8, two upper halo rows, a raw
//   row per group) = 141,552 B dynamic, one workgroup per CU as the denoiser.  (A gain row for each of 24 frames beside the tile
//   would be 160,128 B of the CU's 163,840.)
// Bits.  A frame's arithmetic depends on (n, f) and the item's profile alone, a sample's on (n, s); every sum runs in a fixed
// order (G: bins ascending, then frames ascending); no atomics.
//
// gfx950 resources (csrc/resource_report.py noise.hip; no spills, no scratch):
//   nz_reduce_kernel   58 VGPRs, LDS 141,552 B dynamic (one workgroup per CU)
//   nz_tile_kernel     48 VGPRs, LDS 64,512 B dynamic + 80 B static (two workgroups per CU)
//   hop_sums_kernel    22 VGPRs, LDS 38,912 B        nz_plan_kernel     18 VGPRs, LDS 12,288 B
//   nz_item_kernel     14 VGPRs, no LDS
#include <math.h>

#include <algorithm>

#include "chunk_grid.h"
#include "stft_tile.h"

namespace {

constexpr int kNzMinLen = kHalf + 1;                // below this the reflection is undefined: copy, flag short
constexpr int kNzRow = 516;                         // a row of 513 bins, padded to whole float4s
constexpr int kNzMaxTt = 2, kNzMaxFk = 8;
constexpr int kNzRing = 8;                          // bin-smoothed gain rows of slots 4 r - 2 .. 4 r + 5
constexpr int kNzExtra = kNzRow * (1 + kNzRing + kNzMaxTt + kGroups);
constexpr size_t kNzReduceLds = kLds + sizeof(float) * kNzExtra;
constexpr int kNzMaxSamples = 1 << 24;              // the profile's S: CONDITION_MAX_SAMPLES, as the screen
constexpr int kNzMaxGuard = 1 << 16;
constexpr int kNzFlagNoProfile = 1, kNzFlagShort = 2;
static_assert(kNzRing == 2 * kGroups && kNzRing >= kGroups + 2 * kNzMaxTt && (kNzRing & (kNzRing - 1)) == 0, "the ring holds a round and its halo");
static_assert(kNzRow % 4 == 0 && kNzRow >= kBins, "the frame slots behind the rows are read and written as float2 / float4");
static_assert(kNzReduceLds == 141552 && kNzReduceLds <= 160 * 1024, "the header above and DESIGN.md 4.32 quote this");

// ------------------------------------------------------------------------------------------------------------ profile
constexpr int kNzPlanThreads = 1024;
static_assert(kGridHop == kHop && kGridFrame == kNfft, "a trim frame t is the STFT frame t + 2: one hop, one frame length");
static_assert(kAnalysisLds == 64512, "the header above quotes this");

struct NzLayout {
    int NH, W;                                      // hops an item can have; tiles of 16 STFT frames
    int64_t cum, mask, part, count, per_item;       // offsets and size in 8-byte words
};

NzLayout nz_layout(int S) {
    NzLayout l;
    l.NH = std::max(1, (S + kHop - 1) / kHop);
    l.W = S / kHop / kSegs + 1;                     // frames 0 .. S / 256
    const int64_t ints = (l.NH + 2) / 2;            // NH + 1 int32
    l.cum = l.NH, l.mask = l.cum + ints, l.part = l.mask + ints, l.count = l.part + (int64_t)l.W * kBins;
    l.per_item = l.count + 1;
    return l;
}

struct NzArgs {
    int S, NH, W, ref_mode, guard, min_frames;
    int64_t cum, mask, part, count, per_item;
    double factor, ref;
    double* ws;
    double* noise;
    int32_t *noise_frames, *frames, *flags;
};

__device__ __forceinline__ double* nz_hop(const NzArgs& a, int b) { return a.ws + (int64_t)b * a.per_item; }
__device__ __forceinline__ int* nz_cum(const NzArgs& a, int b) { return reinterpret_cast<int*>(nz_hop(a, b) + a.cum); }
__device__ __forceinline__ int* nz_mask(const NzArgs& a, int b) { return reinterpret_cast<int*>(nz_hop(a, b) + a.mask); }
__device__ __forceinline__ double* nz_part(const NzArgs& a, int b) { return nz_hop(a, b) + a.part; }
__device__ __forceinline__ int* nz_count(const NzArgs& a, int b) { return reinterpret_cast<int*>(nz_hop(a, b) + a.count); }

__global__ __launch_bounds__(kNzPlanThreads) void nz_plan_kernel(const int64_t* __restrict__ audio_len, const NzArgs a) {
    constexpr int kNT = kNzPlanThreads;
    __shared__ double red[kNT];
    __shared__ int ired[kNT];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n = valid_len(audio_len, b, a.S);
    const int T = (n + kHop - 1) / kHop;
    const double* hop = nz_hop(a, b);
    int* cum = nz_cum(a, b);
    int* mask = nz_mask(a, b);

    double mx = 0.0;
    for (int t = tid; t < T; t += kNT) mx = fmax(mx, frame_power(hop, t, T));
    const double thr = frame_threshold<kNT>(mx, a.ref_mode == 0, a.ref, a.factor, tid, red);

    // cum[t] = the active frames before t, t <= T: a strip of consecutive frames per lane
    const int L = (T + kNT - 1) / kNT, t0 = min(T, tid * L), t1 = min(T, t0 + L);
    int act = 0;
    for (int t = t0; t < t1; ++t) act += frame_power(hop, t, T) > thr;
    int total;
    int before = block_scan_excl<false, kNT>(act, 0, tid, ired, total);
    for (int t = t0; t < t1; ++t) {
        cum[t] = before;
        before += frame_power(hop, t, T) > thr;
    }
    if (tid == 0) cum[T] = total;
    __syncthreads();                                                    // cum is written (this workgroup's own stores)

    const int F = n >= kNzMinLen ? 1 + n / kHop : 0, f_last = n / kHop - 2;
    int cnt = 0;
    for (int f = tid; f <= a.NH; f += kNT) {
        int m = 0;
        if (F > 0 && f >= 2 && f <= f_last) {
            const int t = f - 2;                                        // t <= n / 256 - 4 < T
            m = cum[min(T, t + a.guard + 1)] == cum[max(0, t - a.guard)];
        }
        mask[f] = m;
        cnt += m;
    }
    ired[tid] = cnt;
    __syncthreads();
    for (int s = kNT / 2; s > 0; s >>= 1) {
        if (tid < s) ired[tid] += ired[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        cnt = ired[0];
        *nz_count(a, b) = cnt;
        a.noise_frames[b] = cnt, a.frames[b] = F;
        a.flags[b] = (cnt < a.min_frames ? kNzFlagNoProfile : 0) | (F == 0 ? kNzFlagShort : 0);
    }
}

__global__ __launch_bounds__(kThreads) void nz_tile_kernel(const float* __restrict__ audio, int64_t ld, const int64_t* __restrict__ audio_len,
                                                           const float* __restrict__ tables, int vec, const NzArgs a) {
    extern __shared__ float4 lds_raw[];
    __shared__ int list[kSegs], listed;
    const TileLds tile = carve_tile(lds_raw, kAnalysisStage);     // four slots behind the staged samples: the groups' pong buffers
    float* xs = tile.win + kNfft;

    const int tid = threadIdx.x, w = blockIdx.x, b = blockIdx.y, g = tid / kGT, lt = tid % kGT;
    const int n = valid_len(audio_len, b, a.S);
    if (tid == 0) {                                         // the tile's noise frames, ascending
        const int* mask = nz_mask(a, b);
        int c = 0;
        for (int i = 0; i < kSegs; ++i) {
            const int f = w * kSegs + i;
            if (f <= a.NH && mask[f]) list[c++] = f;
        }
        listed = c;
    }
    __syncthreads();
    const int nf = listed;
    double* part = nz_part(a, b) + (int64_t)w * kBins;
    if (nf == 0) {                                          // (uniform)
        part[tid] = 0.0;
        if (tid == 0) part[kHalf] = 0.0;
        return;
    }

    const int base = w * kTile - kHalf;                     // frame f reads [256 f - 512, 256 f + 512); a multiple of 4
    stage_flat(xs, audio + (int64_t)b * ld, base, n, kAnalysisStage, vec, tid);
    load_tables(tile.tw, tile.win, tables, tid);
    __syncthreads();

    cf* A = tile.ping + g * kHalf;
    cf* Bf = reinterpret_cast<cf*>(tile.frames + g * kNfft);
    double acc = 0.0, acc512 = 0.0;                         // bins tid and (lane 0) 512
    for (int r = 0; r * kGroups < nf; ++r) {
        const int fs = r * kGroups + g;
        const int f = fs < nf ? list[fs] : w * kSegs;
        gather_zero_padded(A, tile.win, f * kHop - kHalf, n, fs < nf, lt, [&](int i) { return xs[i - base]; });
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
    part[tid] = acc;
    if (tid == 0) part[kHalf] = acc512;
}

__global__ __launch_bounds__(kThreads) void nz_item_kernel(const int64_t* __restrict__ audio_len, const NzArgs a) {
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n = valid_len(audio_len, b, a.S);
    const int F = n >= kNzMinLen ? 1 + n / kHop : 0, WF = (F + kSegs - 1) / kSegs;
    const int cnt = *nz_count(a, b);
    const bool ok = cnt > 0 && cnt >= a.min_frames;
    const double* part = nz_part(a, b);
    for (int k = tid; k < kBins; k += kThreads) {
        double acc = 0.0;
        if (ok)
            for (int w = 0; w < WF; ++w) acc += part[(int64_t)w * kBins + k];
        a.noise[(int64_t)b * kBins + k] = ok ? acc / (double)cnt : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------------------ reduce
__device__ __forceinline__ float nz_power(cf X) { return fmaf(X.x, X.x, X.y * X.y); }

// row[k] = max(1 - nb[k] / |X[k]|^2, g_min), g_min where |X[k]|^2 = 0 (IEEE division; -inf and NaN fall to the floor), k <= 512,
// from the frame's half-length spectrum Z, by the group's 128 lanes
__device__ __forceinline__ void nz_gain_row(float* row, const cf* Z, const cf* tw, const float* nb, float g_min, int lt) {
    for (int k = lt; k < kBins; k += kGT) {
        const float m2 = nz_power(real_split(Z, k, kHalf, tw[k]));
        row[k] = m2 > 0.f ? fmaxf(1.0f - nb[k] / m2, g_min) : g_min;
    }
}

// h[k] = (sum_e w_k[e] g[k + e]) / (sum_e w_k[e]) over the bins 0 <= k + e <= 512, w_k[e] = Fk + 1 - |e|, e ascending, by the
// group's 128 lanes
__device__ __forceinline__ void nz_smooth_row(float* h, const float* g, int Fk, int lt) {
    for (int k = lt; k < kBins; k += kGT) {
        const int e0 = max(-Fk, -k), e1 = min(Fk, kHalf - k);
        float acc = 0.f;
        int wk_sum = 0;
        for (int e = e0; e <= e1; ++e) {
            const int w = Fk + 1 - abs(e);
            acc = fmaf((float)w, g[k + e], acc);
            wk_sum += w;
        }
        h[k] = acc / (float)wk_sum;
    }
}

__global__ void __launch_bounds__(kThreads) nz_reduce_kernel(const float* __restrict__ audio, int64_t lda, const int64_t* __restrict__ audio_len,
                                                             const float* __restrict__ tables, const double* __restrict__ noise, int P,
                                                             const int32_t* __restrict__ index, const int32_t* __restrict__ flags, double over,
                                                             float g_min, int Tt, int Fk, float* __restrict__ out, int64_t ldo, int S) {
    extern __shared__ float4 lds_raw[];
    const TileLds tile = carve_tile(lds_raw, kNzExtra);
    float* nb = tile.win + kNfft;                                        // [516]: beta * noise[k]
    float* ring = nb + kNzRow;                                           // [8][516]: bin-smoothed gains of slots -2 .. nf - 1, modulo 8
    float* upper = ring + kNzRing * kNzRow;                              // [2][516]: of the frames f_hi, f_hi + 1
    float* raw = upper + (kNzMaxTt + threadIdx.x / kGT) * kNzRow;        // [4][516]: the group's raw gains, before the bins are smoothed

    const int b = blockIdx.y, tid = threadIdx.x, g = tid / kGT, lt = tid % kGT;
    const int n = valid_len(audio_len, b, S);
    const int m0 = blockIdx.x * kTile, m1 = min(S, m0 + kTile);
    const int mv = max(m0, min(n, m1));                                  // [m0, mv) are the tile's samples inside the item
    const float* xrow = audio + (int64_t)b * lda;
    float* orow = out + (int64_t)b * ldo;
    const int prow = index ? index[b] : b;
    const bool copy = n < kNzMinLen || prow < 0 || prow >= P || (flags && (flags[b] & (kNzFlagNoProfile | kNzFlagShort)));

    if (copy) {                                                          // (uniform)
        for (int m = m0 + tid; m < mv; m += kThreads) orow[m] = xrow[m];
    } else if (mv > m0) {
        const int q0 = blockIdx.x * kSegs, F = 1 + n / kHop;
        const int f_lo = max(0, q0 - 1), f_hi = min(F, (mv - 1 + kHalf) / kHop + 1), nf = f_hi - f_lo;
        load_tables(tile.tw, tile.win, tables, tid);
        for (int i = tid; i < kBins; i += kThreads) nb[i] = (float)(over * noise[(int64_t)prow * kBins + i]);
        __syncthreads();
        cf* A = tile.ping + g * kHalf;
        auto slot = [&](int s) { return reinterpret_cast<cf*>(tile.frames + s * kNfft); };
        auto gains = [&](int s) { return s >= nf ? upper + (s - nf) * kNzRow : ring + ((s + kNzRing) & (kNzRing - 1)) * kNzRow; };

        if (Tt > 0) {                                                    // (uniform) the halo: slots -2, -1, nf, nf + 1
            const int s = g < 2 ? g - 2 : nf + g - 2;
            const int f = f_lo + s;
            const bool live = (g < 2 ? -s <= Tt : s - nf < Tt) && f >= 0 && f < F;
            if (live) gather_reflected(A, tile.win, xrow, f, n, lt);
            else clear_frame(A, lt);
            __syncthreads();
            fft<false, kGT, kTw>(A, slot(g), kHalf, lt, tile.tw);
            if (live) nz_gain_row(raw, slot(g), tile.tw, nb, g_min, lt);
            __syncthreads();
            if (live) nz_smooth_row(gains(s), raw, Fk, lt);
        }
        for (int r = 0; r * kGroups < nf; ++r) {                         // analysis: Z of every frame into its slot
            const int fs = r * kGroups + g;                              // fs >= nf: transformed, never read
            if (fs < nf) gather_reflected(A, tile.win, xrow, f_lo + fs, n, lt);
            else clear_frame(A, lt);
            __syncthreads();                                             // (also: the halo's rows are written, its slots free)
            fft<false, kGT, kTw>(A, slot(fs), kHalf, lt, tile.tw);
        }
        if (g < 2 && g < nf) nz_gain_row(raw, slot(g), tile.tw, nb, g_min, lt);
        __syncthreads();
        if (g < 2 && g < nf) nz_smooth_row(gains(g), raw, Fk, lt);
        for (int r = 0; r * kGroups < nf; ++r) {
            const int sa = r * kGroups + 2 + g, fs = r * kGroups + g;
            __syncthreads();                                             // the group's raw row is read
            if (sa < nf) nz_gain_row(raw, slot(sa), tile.tw, nb, g_min, lt);
            __syncthreads();
            if (sa < nf) nz_smooth_row(gains(sa), raw, Fk, lt);
            __syncthreads();
            cf* Bf = slot(fs);
            if (fs < nf) {
                // G = the triangular mean over the frames f + d in [0, F) of their bin-smoothed rows, d ascending
                auto smoothed = [&](int k) {
                    float num = 0.f;
                    int wt_sum = 0;
                    for (int d = -Tt; d <= Tt; ++d) {
                        const int f = f_lo + fs + d;
                        if (f < 0 || f >= F) continue;
                        num = fmaf((float)(Tt + 1 - abs(d)), gains(fs + d)[k], num);
                        wt_sum += Tt + 1 - abs(d);
                    }
                    return num / (float)wt_sum * (1.0f / kNfft);
                };
                pack_pairs(A, lt, tile.tw, [&](int k, int m, cf& xk, cf& xm) {
                    const cf X = real_split(Bf, k, kHalf, tile.tw[k]);
                    const float gk = smoothed(k);
                    xk = make_float2(X.x * gk, X.y * gk);
                    if (k == 256) {
                        xm = xk;
                    } else {
                        const cf Xm = real_split(Bf, m, kHalf, tile.tw[m]);
                        const float gm = smoothed(m);
                        xm = make_float2(Xm.x * gm, Xm.y * gm);
                    }
                });
            } else {
                clear_frame(A, lt);
            }
            __syncthreads();
            fft<true, kGT, kTw>(A, Bf, kHalf, lt, tile.tw);
        }
        overlap_add(orow, tile.frames, tile.win, m0, mv, kHalf, f_lo, F, tid);   // pad 512: center = true
    }
    for (int m = mv + tid; m < m1; m += kThreads) orow[m] = 0.f;
}

}  // namespace

extern "C" int32_t ispk_noise_tile_samples(void) { return kTile; }

extern "C" int32_t ispk_noise_workspace_bytes(int32_t B, int32_t S, int64_t* bytes) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= kNzMaxSamples, ISPK_E_SHAPE,
                 "ispk_noise_workspace_bytes: bad shape B=%d S=%d (B <= 65535, 0 <= S <= 2^24)", B, S);
    ISPK_REQUIRE(bytes, ISPK_E_NULL, "ispk_noise_workspace_bytes: null pointer");
    *bytes = 8 * (int64_t)B * nz_layout(S).per_item;
    return 0;
}

extern "C" int32_t ispk_noise_profile_f64(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables, double factor,
                                          int32_t ref_mode, double ref, int32_t guard, int32_t min_noise_frames, double* noise,
                                          int32_t* noise_frames, int32_t* frames, int32_t* flags, void* workspace, int64_t workspace_bytes,
                                          int32_t B, int32_t S, ispk_stream_t stream) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= kNzMaxSamples, ISPK_E_SHAPE,
                 "ispk_noise_profile_f64: bad shape B=%d S=%d (B <= 65535, 0 <= S <= 2^24)", B, S);
    ISPK_REQUIRE((ref_mode == 0 || ref_mode == 1) && factor >= 0.0 && (ref_mode == 0 || ref >= 0.0), ISPK_E_SHAPE,
                 "ispk_noise_profile_f64: bad ref mode %d, factor %g or ref %g", ref_mode, factor, ref);
    ISPK_REQUIRE(guard >= 0 && guard <= kNzMaxGuard && min_noise_frames >= 1, ISPK_E_SHAPE,
                 "ispk_noise_profile_f64: guard %d outside 0 .. %d frames or min_noise_frames %d below 1", guard, kNzMaxGuard, min_noise_frames);
    if (B == 0 || S == 0) return 0;
    ISPK_REQUIRE(audio && audio_len && tables && noise && noise_frames && frames && flags && workspace, ISPK_E_NULL,
                 "ispk_noise_profile_f64: null pointer");
    ISPK_REQUIRE(ld_audio >= S, ISPK_E_SHAPE, "ispk_noise_profile_f64: row stride %lld below S=%d", (long long)ld_audio, S);
    const NzLayout l = nz_layout(S);
    ISPK_REQUIRE(workspace_bytes >= 8 * (int64_t)B * l.per_item && ispk_aligned(workspace, 8), ISPK_E_ALIGN,
                 "ispk_noise_profile_f64: the workspace needs %lld bytes at an 8-byte boundary, got %lld", (long long)(8 * (int64_t)B * l.per_item),
                 (long long)workspace_bytes);
    NzArgs a;
    a.S = S, a.NH = l.NH, a.W = l.W, a.ref_mode = ref_mode, a.guard = guard, a.min_frames = min_noise_frames;
    a.cum = l.cum, a.mask = l.mask, a.part = l.part, a.count = l.count, a.per_item = l.per_item;
    a.factor = factor, a.ref = ref;
    a.ws = reinterpret_cast<double*>(workspace);
    a.noise = noise, a.noise_frames = noise_frames, a.frames = frames, a.flags = flags;
    const int vec = ld_audio % 4 == 0 && ispk_aligned(audio, 16);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(hop_sums_kernel<>, dim3((S + kGridSeg - 1) / kGridSeg, B), dim3(kGridThreads), 0, st, audio, ld_audio, audio_len, S,
                       vec, a.ws, a.per_item);
    hipLaunchKernelGGL(nz_plan_kernel, dim3(B), dim3(kNzPlanThreads), 0, st, audio_len, a);
    hipLaunchKernelGGL(nz_tile_kernel, dim3(l.W, B), dim3(kThreads), kAnalysisLds, st, audio, ld_audio, audio_len, tables, vec, a);
    hipLaunchKernelGGL(nz_item_kernel, dim3(B), dim3(kThreads), 0, st, audio_len, a);
    return ispk_launch_status();
}

extern "C" int32_t ispk_noise_reduce_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables,
                                         const double* noise, int32_t P, const int32_t* index, const int32_t* flags, double over, double g_min,
                                         int32_t smooth_frames, int32_t smooth_bins, float* out, int64_t ld_out, int32_t B, int32_t S,
                                         ispk_stream_t stream) {
    if (B == 0 || S == 0) return 0;
    ISPK_REQUIRE(audio && tables && noise && out, ISPK_E_NULL, "ispk_noise_reduce_f32: null pointer");
    ISPK_REQUIRE(B >= 1 && B <= 65535 && S >= 1 && S <= INT32_MAX - 2 * kTile && P >= 1, ISPK_E_SHAPE,
                 "ispk_noise_reduce_f32: bad shape B=%d S=%d P=%d (B <= 65535, S <= 2^31 - 8193, P >= 1)", B, S, P);
    ISPK_REQUIRE(ld_audio >= S && ld_out >= S, ISPK_E_SHAPE,
                 "ispk_noise_reduce_f32: row strides ld_audio=%lld ld_out=%lld shorter than the rows (S=%d)", (long long)ld_audio,
                 (long long)ld_out, S);
    ISPK_REQUIRE(out != audio, ISPK_E_SHAPE, "ispk_noise_reduce_f32: out may not be audio (neighbouring tiles read the halo)");
    ISPK_REQUIRE(over >= 0.0 && isfinite(over) && g_min > 0.0 && g_min <= 1.0, ISPK_E_SHAPE,
                 "ispk_noise_reduce_f32: over %g is negative or not finite, or g_min %g outside (0, 1]", over, g_min);
    ISPK_REQUIRE(smooth_frames >= 0 && smooth_frames <= kNzMaxTt && smooth_bins >= 0 && smooth_bins <= kNzMaxFk, ISPK_E_SHAPE,
                 "ispk_noise_reduce_f32: smooth_frames %d outside 0 .. %d or smooth_bins %d outside 0 .. %d", smooth_frames, kNzMaxTt,
                 smooth_bins, kNzMaxFk);
    ISPK_RESERVE_LDS(nz_reduce_kernel, kNzReduceLds, "ispk_noise_reduce_f32");
    hipLaunchKernelGGL(nz_reduce_kernel, dim3((S + kTile - 1) / kTile, B), dim3(kThreads), kNzReduceLds,
                       reinterpret_cast<hipStream_t>(stream), audio, ld_audio, audio_len, tables, noise, P, index, flags, over, (float)g_min,
                       smooth_frames, smooth_bins, out, ld_out, S);
    return ispk_launch_status();
}
