// TimeStretch (isp_tts_amd/data/stretch.py; no counterpart in the reference, which never changes a waveform's tempo): the phase
// vocoder of torchaudio / librosa on the 1024 / 256 STFT tile, for a padded mono batch fp32 [B][S] with int64 audio_len [B] (a
// length below 0 or above S counts as 0) and a rate per item (one scalar, or float64 [B] on the device).  include/ispk.h has the
// definition.  Output frame j reads the analysis frames i_j = floor(j r) and i_j + 1: their magnitudes are interpolated, and the
// phase advances by arg X_{i_j + 1} - arg X_{i_j} per output frame.
//
// Phases.  Only exp(i P_j) is used, and w_k + wrap(d - w_k) = d modulo 2 pi, so the recurrence is a product of unit phasors:
//   e_0 = u(X_0),  e_{j+1} = e_j u(X_{i_j + 1}) conj(u(X_{i_j})),  u(z) = z / |z|, u(0) = 1,
// in float64 per bin, with no atan2 and no angle that grows (the textbook's reaches 4e5 rad, where an fp32 ulp is 0.03 rad).  A
// step costs two square roots and one division in float64; |e_j| drifts from 1 by about 1e-16 sqrt(j).
//
// Three launches, no atomics, nothing per (frame, bin) in HBM:
//   st_chunk_kernel   grid (C - 1, B), C = ceil(out_samples / 4096), 512 lanes.  Chunk w is the output frames [max(0, 16 w - 1),
//                     16 (w + 1) - 1): from the first frame that touches output tile w to the first that touches tile w + 1.  The
//                     workgroup streams the analysis frames its output frames read (st_stream below) and lane k multiplies bin k's
//                     steps in ascending j (lane 0 also bin 512); chunk 0 starts from u(X_0).  Writes the product, float64 re [513]
//                     and im [513].  Chunks whose successor holds no output sample return at once.  LDS: the tile's tables and
//                     ping buffers and the ring, no frame slots: 61,440 B, two workgroups per CU.
//   st_scan_kernel    grid (B), one lane per bin: the exclusive product over the item's chunks in order, in place (row w becomes
//                     e at the first frame of tile w).  Lane 0 writes out_len, wanted and flags.
//   st_synth_kernel   the denoiser's tile (stft_tile.h: grid (C, B), the <= 19 output frames that touch the tile, one 4 KB slot
//                     each).  Per output frame all 512 lanes (one per bin) read the two analysis spectra from the ring, form M_j
//                     and Y_j = M_j e_j / 1024 from the running e (registers, started from the scan's row; tile 0 starts from
//                     u(X_0) itself) and leave Y_j in the frame's slot as the half-length array (bin 512's real part beside bin
//                     0's); four such frames make an inverse round (pack_pairs from the slot, the inverse back into it).  Then
//                     overlap_add over the item's Fo output frames.  Samples at or past out_len are written as 0; a short item or
//                     one with a bad rate is copied.  LDS: the tile's 110,592 B + the ring = 143,360 B, one workgroup per CU.
// st_stream: analysis frames ascend with j, so they pass through a ring of 8 half-length spectra (32 KB), four at a time, one
// per group.  After the round that ends with frame a - 1 every output frame with i_j + 1 < a is processed in order; a frame
// still pending has i_j >= a - 1, and the next round overwrites frames a - 8 .. a - 5 only.  At r = 2 a chunk streams 32 to 34
// frames, a tile up to 40.  Frames at or past F are zeros (X_F = 0 is read when i_j = F - 1); dead groups transform zeros so
// that every barrier is reached by all four.  Nothing at or past n is read.
// Bits.  An item's arithmetic depends on its samples, n and r alone: chunk and tile boundaries are functions of j, every product
// runs in ascending j, overlap-add in ascending frame order.
//
// gfx950 resources (csrc/resource_report.py stretch.hip; no spills, no scratch):
//   st_synth_kernel   108 VGPRs, LDS 143,360 B dynamic (one workgroup per CU)
//   st_chunk_kernel   76 VGPRs, LDS 61,440 B dynamic (two workgroups per CU)
//   st_scan_kernel    14 VGPRs, no LDS
#include <math.h>

#include <algorithm>

#include "common.h"
#include "stft_tile.h"

namespace {

constexpr int kStMinLen = kHalf + 1;                // below this the reflection is undefined: copy, flag short
constexpr int kStRing = 8;                          // half-length spectra of consecutive analysis frames, two rounds
constexpr int kStRingFloats = kStRing * kNfft;
constexpr int kStMaxSamples = 1 << 24;              // CONDITION_MAX_SAMPLES
constexpr int kStFlagShort = 1, kStFlagTruncated = 2, kStFlagBadRate = 4;
constexpr double kStMinRate = 0.5, kStMaxRate = 2.0;
constexpr int kStRow = 2 * kBins;                   // a chunk's row: re [513], im [513]
constexpr size_t kStChunkLds = sizeof(cf) * (kTw + kGroups * kHalf) + sizeof(float) * (kNfft + kStRingFloats);
constexpr size_t kStSynthLds = kLds + sizeof(float) * kStRingFloats;
static_assert((kStRing & (kStRing - 1)) == 0 && kStRing >= 2 * kGroups, "a pending output frame reads frames a - 1 and a of the last two rounds");
static_assert(kStChunkLds == 61440 && 2 * kStChunkLds <= 160 * 1024, "two workgroups per CU; the header above quotes this");
static_assert(kStSynthLds == 143360 && kStSynthLds <= 160 * 1024, "the header above and DESIGN.md 4.33 quote this");

struct StPlan {
    int n, F, Fo, flags;                            // samples, analysis frames, output frames
    int out_len, tiles;                             // samples written, output tiles that hold one
    int64_t wanted;
    double r;
    bool copy;
};

// What an item is and how long it gets, from device data alone: the same in all three kernels.
__device__ __forceinline__ StPlan st_plan(const int64_t* __restrict__ audio_len, const double* __restrict__ rates, double rate, int b,
                                          int S, int out_samples) {
    StPlan p;
    p.n = valid_len(audio_len, b, S);
    p.r = rates ? rates[b] : rate;
    const bool bad = !(p.r >= kStMinRate && p.r <= kStMaxRate);          // NaN compares false
    const bool shrt = p.n < kStMinLen;
    p.copy = bad || shrt;
    p.flags = (shrt ? kStFlagShort : 0) | (bad ? kStFlagBadRate : 0);
    p.F = 0, p.Fo = 0, p.wanted = p.n;
    if (!p.copy) {
        p.F = 1 + p.n / kHop;
        p.wanted = (int64_t)rint((double)p.n / p.r);                     // round half to even
        int j = (int)ceil((double)p.F / p.r);                            // the smallest j with j r >= F, by the products themselves
        while (j > 0 && (double)(j - 1) * p.r >= (double)p.F) --j;
        while ((double)j * p.r < (double)p.F) ++j;
        p.Fo = j;
    }
    if (p.wanted > out_samples) p.flags |= kStFlagTruncated;
    p.out_len = (int)(p.wanted < out_samples ? p.wanted : out_samples);
    p.tiles = (p.out_len + kTile - 1) / kTile;
    return p;
}

__device__ __forceinline__ int st_first_frame(int w) { return w > 0 ? w * kSegs - 1 : 0; }   // of output tile / chunk w

// One bin of one output frame, from the half-length spectra of the analysis frames i_j (Za) and i_j + 1 (Zb): their magnitudes
// and the unit step u(Xb) conj(u(Xa)), in float64 from the fp32 spectra.
struct StBin {
    double ma, mb, ax, ay, da, sx, sy;              // |Xa|, |Xb|; u(Xa) = (ax, ay) / da; the step
    __device__ __forceinline__ void start(double& x, double& y) const { x = ax / da, y = ay / da; }
};
__device__ __forceinline__ StBin st_bin(const cf* Za, const cf* Zb, int k, const cf* tw) {
    const cf w = tw[k];
    const cf Xa = real_split(Za, k, kHalf, w), Xb = real_split(Zb, k, kHalf, w);
    StBin s;
    double ax = Xa.x, ay = Xa.y, bx = Xb.x, by = Xb.y;
    s.ma = sqrt(ax * ax + ay * ay), s.mb = sqrt(bx * bx + by * by);
    double da = s.ma, db = s.mb;
    if (!(da > 0.0)) ax = 1.0, ay = 0.0, da = 1.0;                       // u(0) = 1: arg 0 = 0
    if (!(db > 0.0)) bx = 1.0, by = 0.0, db = 1.0;
    s.ax = ax, s.ay = ay, s.da = da;
    const double inv = 1.0 / (da * db);
    s.sx = (bx * ax + by * ay) * inv, s.sy = (by * ax - bx * ay) * inv;
    return s;
}

struct StPhasor {
    double x, y;
    __device__ __forceinline__ void times(double sx, double sy) {
        const double nx = x * sx - y * sy, ny = x * sy + y * sx;
        x = nx, y = ny;
    }
};

// Streams the analysis frames that the output frames [j0, j1) read through `ring`, four at a time, and calls per_j(j, Za, Zb, a_j)
// for every j in order as soon as both of its spectra are there.  Every lane of the workgroup takes every branch alike; per_j may
// use the ping buffers between barriers of its own.  Ends behind a barrier (fft's last, or per_j's).
template <typename F>
__device__ __forceinline__ void st_stream(const TileLds& tile, cf* ring, const float* __restrict__ xrow, int n, int frames, double r, int j0,
                                          int j1, int g, int lt, F&& per_j) {
    cf* A = tile.ping + g * kHalf;
    int a = (int)floor((double)j0 * r);                                  // the next analysis frame to transform
    int j = j0;
    while (j < j1) {
        const int f = a + g;
        if (f < frames) gather_reflected(A, tile.win, xrow, f, n, lt);
        else clear_frame(A, lt);
        __syncthreads();                                                 // (also: per_j's reads of the ring are done)
        fft<false, kGT, kTw>(A, ring + (f & (kStRing - 1)) * kHalf, kHalf, lt, tile.tw);
        a += kGroups;
        while (j < j1) {
            const double t = (double)j * r;
            const int i = (int)floor(t);
            if (i + 1 >= a) break;
            per_j(j, ring + (i & (kStRing - 1)) * kHalf, ring + ((i + 1) & (kStRing - 1)) * kHalf, t - (double)i);
            ++j;
        }
    }
}

struct StArgs {
    const int64_t* audio_len;
    const double* rates;
    double rate;
    double* ws;                                     // [B][C][2][513]
    int S, out_samples, C;
};

__device__ __forceinline__ double* st_row(const StArgs& a, int b, int w) { return a.ws + ((int64_t)b * a.C + w) * kStRow; }

__global__ void __launch_bounds__(kThreads) st_chunk_kernel(const float* __restrict__ audio, int64_t lda, const float* __restrict__ tables,
                                                            const StArgs a) {
    extern __shared__ float4 lds_raw[];
    const TileLds tile = carve_tile(lds_raw);                            // the slots' place holds the ring
    cf* ring = reinterpret_cast<cf*>(tile.frames);
    const int tid = threadIdx.x, w = blockIdx.x, b = blockIdx.y, g = tid / kGT, lt = tid % kGT;
    const StPlan p = st_plan(a.audio_len, a.rates, a.rate, b, a.S, a.out_samples);
    if (p.copy || w + 1 >= p.tiles) return;                              // (uniform) nobody reads this chunk's product
    load_tables(tile.tw, tile.win, tables, tid);
    __syncthreads();
    StPhasor e = {1.0, 0.0}, e512 = {1.0, 0.0};                          // bins tid and (lane 0) 512
    st_stream(tile, ring, audio + (int64_t)b * lda, p.n, p.F, p.r, st_first_frame(w), min(p.Fo, st_first_frame(w + 1)), g, lt,
              [&](int j, const cf* Za, const cf* Zb, double) {
                  const StBin s = st_bin(Za, Zb, tid, tile.tw);
                  if (j == 0) s.start(e.x, e.y);
                  e.times(s.sx, s.sy);
                  if (tid == 0) {
                      const StBin t = st_bin(Za, Zb, kHalf, tile.tw);
                      if (j == 0) t.start(e512.x, e512.y);
                      e512.times(t.sx, t.sy);
                  }
              });
    double* row = st_row(a, b, w);
    row[tid] = e.x, row[kBins + tid] = e.y;
    if (tid == 0) row[kHalf] = e512.x, row[kBins + kHalf] = e512.y;
}

__global__ void __launch_bounds__(kThreads) st_scan_kernel(const StArgs a, int64_t* __restrict__ out_len, int64_t* __restrict__ wanted,
                                                           int32_t* __restrict__ flags) {
    const int tid = threadIdx.x, b = blockIdx.x;
    const StPlan p = st_plan(a.audio_len, a.rates, a.rate, b, a.S, a.out_samples);
    if (tid == 0) out_len[b] = p.out_len, wanted[b] = p.wanted, flags[b] = p.flags;
    if (p.copy) return;
    for (int k = tid; k < kBins; k += kThreads) {
        StPhasor e = {1.0, 0.0};
        for (int w = 0; w < p.tiles; ++w) {                              // row w: the chunk's product -> the product of the chunks before it
            double* row = st_row(a, b, w);
            const bool more = w + 1 < p.tiles;                           // the last tile's chunk was not computed
            const double sx = more ? row[k] : 1.0, sy = more ? row[kBins + k] : 0.0;
            row[k] = e.x, row[kBins + k] = e.y;
            e.times(sx, sy);
        }
    }
}

__global__ void __launch_bounds__(kThreads) st_synth_kernel(const float* __restrict__ audio, int64_t lda, const float* __restrict__ tables,
                                                            float* __restrict__ out, int64_t ldo, const StArgs a) {
    extern __shared__ float4 lds_raw[];
    const TileLds tile = carve_tile(lds_raw, kStRingFloats);
    cf* ring = reinterpret_cast<cf*>(tile.win + kNfft);
    const int tid = threadIdx.x, w = blockIdx.x, b = blockIdx.y, g = tid / kGT, lt = tid % kGT;
    const StPlan p = st_plan(a.audio_len, a.rates, a.rate, b, a.S, a.out_samples);
    const int m0 = w * kTile, m1 = min(a.out_samples, m0 + kTile);
    const int mv = max(m0, min(p.out_len, m1));                          // [m0, mv) are the tile's samples inside the item's output
    const float* xrow = audio + (int64_t)b * lda;
    float* orow = out + (int64_t)b * ldo;

    if (p.copy) {                                                        // (uniform) out_len <= n
        for (int m = m0 + tid; m < mv; m += kThreads) orow[m] = xrow[m];
    } else if (mv > m0) {
        const int f_lo = st_first_frame(w), f_hi = min(p.Fo, (mv - 1 + kHalf) / kHop + 1);
        load_tables(tile.tw, tile.win, tables, tid);
        StPhasor e = {1.0, 0.0}, e512 = {1.0, 0.0};                      // bins tid and (lane 0) 512; tile 0 takes u(X_0) at j = 0
        if (w > 0) {
            const double* row = st_row(a, b, w);
            e.x = row[tid], e.y = row[kBins + tid];
            if (tid == 0) e512.x = row[kHalf], e512.y = row[kBins + kHalf];
        }
        __syncthreads();
        cf* A = tile.ping + g * kHalf;
        auto slot = [&](int s) { return reinterpret_cast<cf*>(tile.frames + s * kNfft); };
        // slots [s0, s0 + count) hold Y / 1024 (entry 0: the real parts of bins 0 and 512): the inverse of each back into its slot
        auto inverse_round = [&](int s0, int count) {
            __syncthreads();
            cf* Bf = slot(s0 + g);                                       // s0 + 3 < kSlots: s0 is a multiple of 4 below 20
            if (g < count) {
                pack_pairs(A, lt, tile.tw, [&](int k, int m, cf& xk, cf& xm) {
                    if (k == 0) {
                        const cf y = Bf[0];
                        xk = make_float2(y.x, 0.f), xm = make_float2(y.y, 0.f);
                    } else {
                        xk = Bf[k], xm = Bf[m];
                    }
                });
            } else {
                clear_frame(A, lt);
            }
            __syncthreads();
            fft<true, kGT, kTw>(A, Bf, kHalf, lt, tile.tw);
        };
        int done = 0;                                                    // slots already inverted, a multiple of 4
        st_stream(tile, ring, xrow, p.n, p.F, p.r, f_lo, f_hi, g, lt, [&](int j, const cf* Za, const cf* Zb, double aj) {
            cf* Y = slot(j - f_lo);
            const double scale = 1.0 / kNfft;
            const StBin s = st_bin(Za, Zb, tid, tile.tw);
            if (j == 0) s.start(e.x, e.y);
            const double M = ((1.0 - aj) * s.ma + aj * s.mb) * scale;
            cf y = make_float2((float)(M * e.x), (float)(M * e.y));
            e.times(s.sx, s.sy);
            if (tid == 0) {
                const StBin t = st_bin(Za, Zb, kHalf, tile.tw);
                if (j == 0) t.start(e512.x, e512.y);
                y.y = (float)(((1.0 - aj) * t.ma + aj * t.mb) * scale * e512.x);
                e512.times(t.sx, t.sy);
            }
            Y[tid] = y;
            if (j + 1 - f_lo - done == kGroups) {
                inverse_round(done, kGroups);
                done += kGroups;
            }
        });
        if (f_hi - f_lo > done) inverse_round(done, f_hi - f_lo - done);
        overlap_add(orow, tile.frames, tile.win, m0, mv, kHalf, f_lo, p.Fo, tid);   // pad 512: center = true
    }
    for (int m = mv + tid; m < m1; m += kThreads) orow[m] = 0.f;
}

}  // namespace

extern "C" int32_t ispk_stretch_tile_samples(void) { return kTile; }

extern "C" int32_t ispk_stretch_workspace_bytes(int32_t B, int32_t S, int32_t out_samples, int64_t* bytes) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= kStMaxSamples && out_samples >= 0 && out_samples <= kStMaxSamples, ISPK_E_SHAPE,
                 "ispk_stretch_workspace_bytes: bad shape B=%d S=%d out_samples=%d (B <= 65535, 0 <= S, out_samples <= 2^24)", B, S,
                 out_samples);
    ISPK_REQUIRE(bytes, ISPK_E_NULL, "ispk_stretch_workspace_bytes: null pointer");
    *bytes = 8 * (int64_t)B * std::max(1, (out_samples + kTile - 1) / kTile) * kStRow;
    return 0;
}

extern "C" int32_t ispk_stretch_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables, double rate,
                                    const double* rates, float* out, int64_t ld_out, int32_t out_samples, int64_t* out_len,
                                    int64_t* wanted, int32_t* flags, void* workspace, int64_t workspace_bytes, int32_t B, int32_t S,
                                    ispk_stream_t stream) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 1 && S <= kStMaxSamples && out_samples >= 1 && out_samples <= kStMaxSamples, ISPK_E_SHAPE,
                 "ispk_stretch_f32: bad shape B=%d S=%d out_samples=%d (B <= 65535, 1 <= S, out_samples <= 2^24)", B, S, out_samples);
    ISPK_REQUIRE(rates || (rate >= kStMinRate && rate <= kStMaxRate), ISPK_E_SHAPE,
                 "ispk_stretch_f32: rate %g outside [0.5, 2] (the ring of analysis spectra holds two rounds of four frames)", rate);
    if (B == 0) return 0;
    ISPK_REQUIRE(audio && audio_len && tables && out && out_len && wanted && flags && workspace, ISPK_E_NULL,
                 "ispk_stretch_f32: null pointer");
    ISPK_REQUIRE(ld_audio >= S && ld_out >= out_samples, ISPK_E_SHAPE,
                 "ispk_stretch_f32: row strides ld_audio=%lld ld_out=%lld shorter than the rows (S=%d, out_samples=%d)", (long long)ld_audio,
                 (long long)ld_out, S, out_samples);
    ISPK_REQUIRE(out != audio, ISPK_E_SHAPE, "ispk_stretch_f32: out may not be audio (every tile reads the item's analysis frames)");
    const int C = (out_samples + kTile - 1) / kTile;
    const int64_t need = 8 * (int64_t)B * C * kStRow;
    ISPK_REQUIRE(workspace_bytes >= need && ispk_aligned(workspace, 8), ISPK_E_ALIGN,
                 "ispk_stretch_f32: the workspace needs %lld bytes at an 8-byte boundary, got %lld", (long long)need, (long long)workspace_bytes);
    ISPK_RESERVE_LDS(st_synth_kernel, kStSynthLds, "ispk_stretch_f32");
    StArgs a;
    a.audio_len = audio_len, a.rates = rates, a.rate = rate, a.ws = reinterpret_cast<double*>(workspace);
    a.S = S, a.out_samples = out_samples, a.C = C;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (C > 1) hipLaunchKernelGGL(st_chunk_kernel, dim3(C - 1, B), dim3(kThreads), kStChunkLds, st, audio, ld_audio, tables, a);
    hipLaunchKernelGGL(st_scan_kernel, dim3(B), dim3(kThreads), 0, st, a, out_len, wanted, flags);
    hipLaunchKernelGGL(st_synth_kernel, dim3(C, B), dim3(kThreads), kStSynthLds, st, audio, ld_audio, tables, out, ld_out, a);
    return ispk_launch_status();
}
