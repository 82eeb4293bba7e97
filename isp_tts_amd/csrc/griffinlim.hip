// Griffin-Lim mel inversion (isp_tts_amd/griffinlim.py): the mel -> magnitude product and ONE projection of the iteration per
// launch - STFT, replace the magnitude with the target and keep the phase, ISTFT - in the framing of the feature extractor
// (csrc/features.hip): n_fft = win = 1024, hop 256, periodic Hann, 384 zeros on both sides, no centring, so an utterance of
// T frames has n = 256 T samples (include/ispk.h has the definition).
//
//   griffinlim_kernel<kInit, kFast>  the 1024 / 256 tile of stft_tile.h (geometry, LDS, bank and bit-reproducibility notes are
//                    there) with the extractor's framing: sample s takes frames floor((s + 384) / 256) - 3 .. floor((s + 384) /
//                    256), so the tile at hop q0 needs the up-to-20 frames q0 - 2 .. q0 + 17 within [0, T).  Per frame:
//                      gather    (step) 1024 samples x[256 f - 384 + j] inside [0, n), zero elsewhere (gather_zero_padded: a
//                                select, never an index outside the utterance), times the window, into the ping buffer;
//                      forward   (step) 512-point FFT into the frame's slot;
//                      project   per bin pair (k, 512 - k): step: X by real_split, Y = M X / sqrt(|X|^2) (IEEE sqrt and
//                                division), Y = M where |X|^2 = 0; init: Y = M (cos, sin)(2 pi u), u = (hash >> 8) 2^-24 from
//                                drop_hash(seed, 513 f + k) by sincospif.  M = 0 gives exactly 0.  Y / 1024 is packed straight into
//                                the inverse's half-length spectrum: the loop of stft_tile.h's pack_pairs, written out here
//                                (keep the two alike);
//                      inverse   512-point FFT back into the slot;
//                    then the overlap-add over the utterance's T frames (the w^2 sum is positive for every s < n and every
//                    T >= 1).  Samples at or past n are written as 0.  A frame's arithmetic depends on (n, f, seed) alone.
//                    griffinlim_kernel<false, true> is the fast (momentum) step: the step with a second input row `prev` and
//                    a scalar alpha = momentum / (1 + momentum); its gather takes fma(-alpha, prev[i], x[i]) under the same
//                    select and nothing else differs.  The textbook iteration takes the phase of STFT(x_n) - alpha STFT(x_{n-1});
//                    the STFT is linear, so that is STFT(x_n - alpha x_{n-1}): one more waveform read per sample, no spectrum in
//                    HBM, still one launch per iteration.  A compile-time variant: <false> and <true> keep their code.
//   griffinlim_error_kernel  grid (ceil(T / 16), B), 512 threads: the spectral convergence's per-frame sums.  The analysis half of
//                    the step - the same gather, forward FFT, real_split - of 16 frames, 4 at a time, one per group; a frame
//                    belongs to one workgroup (no halo).  Thread t of the group accumulates (sqrt(|X[k]|^2) - M[k])^2 and M[k]^2
//                    over k = t, t + 128, .. <= 512 with fma, then a fixed tree (shuffles within a wave, the group's two waves
//                    through LDS) gives work[b][f] = (num_f, den_f), fp32, for f < Tb.  LDS: 32 KB ping + pong, 8 KB twiddles,
//                    4 KB window, 64 B of partials.
//   griffinlim_error_sum_kernel  grid B, 256 threads: float64 sums of work[b][0 .. Tb) (thread-strided in ascending f, then a
//                    fixed tree in LDS), err[b] = (float)sqrt(num / den); 0 for Tb = 0, and with den = 0: 0 if num = 0, else +inf.
//   mel_to_linear_kernel  grid (ceil(T / 8), B), 256 threads.  exp(mel) of 8 frames into LDS, then thread k accumulates
//                    sum_m P[k][m] exp(mel[m][f]) for the 8 frames in ascending m (P is read transposed: lanes on k), clamps at 0.
//
// gfx950 resources (csrc/resource_report.py griffinlim.hip; no spills, no scratch):
//   griffinlim_kernel<false>        76 VGPRs, LDS 110,592 B dynamic (one workgroup of 8 waves per CU: the LDS sets the occupancy
//                                   of 2 waves per SIMD; the report's register-only 6, 7 at the init's count, binds nothing)
//   griffinlim_kernel<true>         66 VGPRs, LDS 110,592 B dynamic
//   griffinlim_kernel<false, true>  74 VGPRs, LDS 110,592 B dynamic
//   griffinlim_error_kernel         60 VGPRs, LDS 45,120 B dynamic
//   griffinlim_error_sum_kernel     14 VGPRs, LDS 4,096 B static
//   mel_to_linear_kernel      60 VGPRs (fp32 and fp16 mel), LDS 4,096 B static
#include <math.h>

#include "common.h"
#include "dropout.h"
#include "stft_tile.h"

namespace {

constexpr int kPad = (kNfft - kHop) / 2;           // 384 zeros on each side, the extractor's pad
constexpr int kMaxFrames = (INT32_MAX - 2 * kTile) / kHop;

constexpr int kMelFrames = 8;                      // frames per workgroup of mel_to_linear_kernel
constexpr int kMelThreads = 256;
constexpr int kMaxMels = 128;

// Y / 1024 of the projection: M X / |X|, M where |X|^2 = 0, exactly 0 for M = 0
__device__ __forceinline__ cf project(cf X, float M) {
    if (M == 0.f) return make_float2(0.f, 0.f);
    const float ms = M * (1.0f / kNfft), m2 = X.x * X.x + X.y * X.y;
    if (!(m2 > 0.f)) return make_float2(ms, 0.f);
    const float g = ms / sqrtf(m2);
    return make_float2(X.x * g, X.y * g);
}

// Y / 1024 of the initial spectrum: M exp(2 pi i u), u = (hash >> 8) 2^-24 a function of (seed, f, k) alone
__device__ __forceinline__ cf hashed_phase(float M, uint64_t seed, int f, int k) {
    if (M == 0.f) return make_float2(0.f, 0.f);
    const uint32_t h = drop_hash(seed, (uint32_t)f * (uint32_t)kBins + (uint32_t)k);
    float s, c;
    sincospif((float)(h >> 8) * (2.0f / 16777216.0f), &s, &c);      // 2 u: exact in fp32
    const float ms = M * (1.0f / kNfft);
    return make_float2(ms * c, ms * s);
}

template <bool kInit, bool kFast = false>
__global__ void __launch_bounds__(kThreads) griffinlim_kernel(const float* __restrict__ audio, int64_t lda,
                                                              const float* __restrict__ prev, int64_t ldp, float alpha,
                                                              const float* __restrict__ mag, int64_t ldm,
                                                              const int64_t* __restrict__ mel_len,
                                                              const float* __restrict__ tables, float* __restrict__ out,
                                                              int64_t ldo, int64_t* __restrict__ audio_len, int T,
                                                              uint64_t seed) {
    extern __shared__ float4 lds_raw[];
    const TileLds tile = carve_tile(lds_raw);

    const int b = blockIdx.y, tid = threadIdx.x, g = tid / kGT, lt = tid % kGT;
    const int Tb = valid_len(mel_len, b, T), n = Tb * kHop, S = T * kHop;
    const int m0 = blockIdx.x * kTile, m1 = min(S, m0 + kTile);
    const int mv = max(m0, min(n, m1));                               // [m0, mv) are the tile's samples inside the utterance
    static_assert(!(kInit && kFast), "the initial waveform reads no audio");
    const float* xrow = kInit ? nullptr : audio + (int64_t)b * lda;
    const float* prow = kFast ? prev + (int64_t)b * ldp : nullptr;
    const float* mrow = mag + (int64_t)b * ldm;
    float* orow = out + (int64_t)b * ldo;
    if (blockIdx.x == 0 && tid == 0 && audio_len) audio_len[b] = n;

    if (mv > m0) {
        const int q0 = blockIdx.x * kSegs;
        const int f_lo = max(0, q0 - 2), f_hi = min(Tb, (mv - 1 + kPad) / kHop + 1), nf = f_hi - f_lo;   // nf <= kSlots
        load_tables(tile.tw, tile.win, tables, tid);
        __syncthreads();
        cf* A = tile.ping + g * kHalf;
        for (int r = 0; r * kGroups < nf; ++r) {
            const int fs = r * kGroups + g, f = f_lo + fs;            // slot and frame; fs >= nf: transformed, never read
            const bool live = fs < nf;
            cf* Bf = reinterpret_cast<cf*>(tile.frames + fs * kNfft);
            if (!kInit) {
                const int i0 = f * kHop - kPad;                       // the frame's first sample
                if (kFast)                                            // x[i] - alpha prev[i]: one select covers both rows
                    gather_zero_padded(A, tile.win, i0, n, live, lt, [&](int i) { return fmaf(-alpha, prow[i], xrow[i]); });
                else
                    gather_zero_padded(A, tile.win, i0, n, live, lt, [&](int i) { return xrow[i]; });
                __syncthreads();
                fft<false, kGT, kTw>(A, Bf, kHalf, lt, tile.tw);
            }
            const float* mf = mrow + (int64_t)f * kBins;
            for (int k = lt; k <= 256; k += kGT) {                    // pack_pairs of stft_tile.h, written out (see the header)
                const int m = kHalf - k;
                const float Mk = live ? mf[k] : 0.f, Mm = live ? mf[m] : 0.f;
                cf xk, xm;
                if (kInit) {
                    xk = hashed_phase(Mk, seed, f, k);
                    xm = k == 256 ? xk : hashed_phase(Mm, seed, f, m);
                } else {
                    xk = project(real_split(Bf, k, kHalf, tile.tw[k]), Mk);
                    xm = k == 256 ? xk : project(real_split(Bf, m, kHalf, tile.tw[m]), Mm);
                }
                if (k == 0) {                                         // irfft drops the imaginary parts of DC and Nyquist
                    xk.y = 0.f;
                    xm.y = 0.f;
                }
                {   // Z_k
                    const cf e = make_float2(xk.x + xm.x, xk.y - xm.y), d = make_float2(xk.x - xm.x, xk.y + xm.y);
                    const cf o = ctw<true>(d, tile.tw[k]);
                    A[k] = make_float2(e.x - o.y, e.y + o.x);
                }
                if (k > 0 && k < 256) {   // Z_{512-k}
                    const cf e = make_float2(xm.x + xk.x, xm.y - xk.y), d = make_float2(xm.x - xk.x, xm.y + xk.y);
                    const cf o = ctw<true>(d, tile.tw[m]);
                    A[m] = make_float2(e.x - o.y, e.y + o.x);
                }
            }
            __syncthreads();
            fft<true, kGT, kTw>(A, Bf, kHalf, lt, tile.tw);
        }
        overlap_add(orow, tile.frames, tile.win, m0, mv, kPad, f_lo, Tb, tid);
    }
    for (int m = mv + tid; m < m1; m += kThreads) orow[m] = 0.f;
}

// ---- spectral convergence: the analysis half of the step per frame, then one float64 sum per utterance
constexpr int kErrFrames = 16;                     // frames per workgroup of griffinlim_error_kernel
constexpr size_t kErrLds = sizeof(cf) * (kTw + 2 * kGroups * kHalf) + sizeof(float) * kNfft + sizeof(float2) * kGroups * 2;
constexpr int kSumThreads = 256;

__global__ void __launch_bounds__(kThreads) griffinlim_error_kernel(const float* __restrict__ audio, int64_t lda,
                                                                    const float* __restrict__ mag, int64_t ldm,
                                                                    const int64_t* __restrict__ mel_len,
                                                                    const float* __restrict__ tables, float* __restrict__ work,
                                                                    int64_t ldw, int T) {
    extern __shared__ float4 lds_raw[];
    cf* tw = reinterpret_cast<cf*>(lds_raw);                          // [kTw]
    cf* ping = tw + kTw;                                              // [kGroups][512]
    cf* pong = ping + kGroups * kHalf;                                // [kGroups][512]
    float* win = reinterpret_cast<float*>(pong + kGroups * kHalf);    // [1024]
    float2* part = reinterpret_cast<float2*>(win + kNfft);            // [kGroups][2]: one (num, den) per wave

    const int b = blockIdx.y, tid = threadIdx.x, g = tid / kGT, lt = tid % kGT;
    const int Tb = valid_len(mel_len, b, T), n = Tb * kHop, f0 = blockIdx.x * kErrFrames;
    if (f0 >= Tb) return;
    const float* xrow = audio + (int64_t)b * lda;
    const float* mrow = mag + (int64_t)b * ldm;
    float* wrow = work + (int64_t)b * ldw;
    load_tables(tw, win, tables, tid);
    __syncthreads();
    cf *A = ping + g * kHalf, *Bf = pong + g * kHalf;
    const int nf = min(kErrFrames, Tb - f0);
    for (int r = 0; r * kGroups < nf; ++r) {
        const int f = f0 + r * kGroups + g;
        const bool live = f < Tb;                                     // a group past Tb transforms zeros and writes nothing
        gather_zero_padded(A, win, f * kHop - kPad, n, live, lt, [&](int i) { return xrow[i]; });
        __syncthreads();
        fft<false, kGT, kTw>(A, Bf, kHalf, lt, tw);
        // thread-strided partials over the 513 bins in ascending k, then a fixed tree: lanes, then the group's two waves
        const float* mf = mrow + (int64_t)f * kBins;
        float num = 0.f, den = 0.f;
        for (int k = lt; k < kBins; k += kGT) {
            const cf X = real_split(Bf, k, kHalf, tw[k]);
            const float M = live ? mf[k] : 0.f, d = sqrtf(X.x * X.x + X.y * X.y) - M;
            num = fmaf(d, d, num);
            den = fmaf(M, M, den);
        }
        for (int off = 32; off > 0; off >>= 1) {
            num += __shfl_down(num, off, 64);
            den += __shfl_down(den, off, 64);
        }
        if (lt % 64 == 0) part[g * 2 + lt / 64] = make_float2(num, den);
        __syncthreads();
        if (live && lt == 0) {
            const float2 p0 = part[g * 2], p1 = part[g * 2 + 1];
            wrow[2 * (int64_t)f] = p0.x + p1.x;
            wrow[2 * (int64_t)f + 1] = p0.y + p1.y;
        }
        // the next round's gather writes A, its barrier precedes the next write of `part`
    }
}

__global__ void __launch_bounds__(kSumThreads) griffinlim_error_sum_kernel(const float* __restrict__ work, int64_t ldw,
                                                                           const int64_t* __restrict__ mel_len,
                                                                           float* __restrict__ err, int T) {
    __shared__ double sn[kSumThreads], sd[kSumThreads];
    const int b = blockIdx.x, tid = threadIdx.x, Tb = valid_len(mel_len, b, T);
    const float* wrow = work + (int64_t)b * ldw;
    double num = 0.0, den = 0.0;
    for (int f = tid; f < Tb; f += kSumThreads) {                     // ascending f per thread, then a fixed tree
        num += (double)wrow[2 * (int64_t)f];
        den += (double)wrow[2 * (int64_t)f + 1];
    }
    sn[tid] = num;
    sd[tid] = den;
    __syncthreads();
    for (int s = kSumThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            sn[tid] += sn[tid + s];
            sd[tid] += sd[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double nu = sn[0], de = sd[0];
        err[b] = de > 0.0 ? (float)sqrt(nu / de) : (nu == 0.0 ? 0.f : (float)(nu / de));   // den = 0: 0, or +inf (NaN stays NaN)
    }
}

template <typename TM>
__global__ void __launch_bounds__(kMelThreads) mel_to_linear_kernel(const TM* __restrict__ mel, int64_t sb, int64_t sc, int64_t st,
                                                                    const int64_t* __restrict__ mel_len,
                                                                    const float* __restrict__ pinv_t, float* __restrict__ mag,
                                                                    int64_t ldm, int n_mels, int T) {
    __shared__ float e[kMaxMels][kMelFrames];
    const int b = blockIdx.y, t0 = blockIdx.x * kMelFrames, tid = threadIdx.x;
    const int nv = min(kMelFrames, valid_len(mel_len, b, T) - t0);
    if (nv <= 0) return;
    const TM* mb = mel + (int64_t)b * sb;
    for (int i = tid; i < n_mels * kMelFrames; i += kMelThreads) {
        const int c = i / kMelFrames, j = i % kMelFrames;
        e[c][j] = j < nv ? expf((float)mb[(int64_t)c * sc + (int64_t)(t0 + j) * st]) : 0.f;
    }
    __syncthreads();
    float* ob = mag + (int64_t)b * ldm + (int64_t)t0 * kBins;
    for (int k = tid; k < kBins; k += kMelThreads) {
        float acc[kMelFrames];
#pragma unroll
        for (int j = 0; j < kMelFrames; ++j) acc[j] = 0.f;
        for (int c = 0; c < n_mels; ++c) {
            const float p = pinv_t[c * kBins + k];
#pragma unroll
            for (int j = 0; j < kMelFrames; ++j) acc[j] = fmaf(p, e[c][j], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < kMelFrames; ++j)
            if (j < nv) ob[j * kBins + k] = fmaxf(acc[j], 0.f);
    }
}

}  // namespace

extern "C" int32_t ispk_griffinlim_tile_samples(void) { return kTile; }

extern "C" int32_t ispk_mel_to_linear_f32(const void* mel, int32_t mel_f16, int64_t mel_sb, int64_t mel_sc, int64_t mel_st,
                                          const int64_t* mel_len, const float* pinv_t, float* mag, int64_t ld_mag, int32_t B,
                                          int32_t n_mels, int32_t T, ispk_stream_t stream) {
    if (B == 0 || T == 0) return 0;
    ISPK_REQUIRE(mel && pinv_t && mag, ISPK_E_NULL, "ispk_mel_to_linear_f32: null pointer");
    ISPK_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= kMaxFrames && n_mels >= 1 && n_mels <= kMaxMels, ISPK_E_SHAPE,
                 "ispk_mel_to_linear_f32: bad shape B=%d n_mels=%d T=%d (B <= 65535, n_mels <= 128, T <= %d)", B, n_mels, T,
                 kMaxFrames);
    ISPK_REQUIRE(ld_mag >= (int64_t)T * kBins, ISPK_E_SHAPE,
                 "ispk_mel_to_linear_f32: leading stride ld_mag=%lld shorter than T * 513 = %lld", (long long)ld_mag,
                 (long long)T * kBins);
    const dim3 grid((T + kMelFrames - 1) / kMelFrames, B);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (mel_f16)
        hipLaunchKernelGGL(mel_to_linear_kernel<_Float16>, grid, dim3(kMelThreads), 0, s, static_cast<const _Float16*>(mel),
                           mel_sb, mel_sc, mel_st, mel_len, pinv_t, mag, ld_mag, n_mels, T);
    else
        hipLaunchKernelGGL(mel_to_linear_kernel<float>, grid, dim3(kMelThreads), 0, s, static_cast<const float*>(mel), mel_sb,
                           mel_sc, mel_st, mel_len, pinv_t, mag, ld_mag, n_mels, T);
    return ispk_launch_status();
}

extern "C" int32_t ispk_griffinlim_step_f32(const float* audio, int64_t ld_audio, const float* mag, int64_t ld_mag,
                                            const int64_t* mel_len, const float* tables, float* out, int64_t ld_out,
                                            int64_t* audio_len, int32_t B, int32_t T, int32_t mode, uint64_t seed,
                                            ispk_stream_t stream) {
    ISPK_REQUIRE(mode == ISPK_GRIFFINLIM_STEP || mode == ISPK_GRIFFINLIM_INIT, ISPK_E_UNSUPPORTED,
                 "ispk_griffinlim_step_f32: mode %d (0 = step, 1 = init)", mode);
    if (B == 0 || T == 0) return 0;
    const bool init = mode == ISPK_GRIFFINLIM_INIT;
    ISPK_REQUIRE((init || audio) && mag && tables && out, ISPK_E_NULL, "ispk_griffinlim_step_f32: null pointer");
    ISPK_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= kMaxFrames, ISPK_E_SHAPE,
                 "ispk_griffinlim_step_f32: bad shape B=%d T=%d (B <= 65535, T <= %d)", B, T, kMaxFrames);
    const int64_t S = (int64_t)T * kHop;
    ISPK_REQUIRE((init || ld_audio >= S) && ld_out >= S && ld_mag >= (int64_t)T * kBins, ISPK_E_SHAPE,
                 "ispk_griffinlim_step_f32: row strides ld_audio=%lld ld_out=%lld ld_mag=%lld shorter than the rows (T=%d)",
                 (long long)ld_audio, (long long)ld_out, (long long)ld_mag, T);
    ISPK_REQUIRE(init || out != audio, ISPK_E_SHAPE,
                 "ispk_griffinlim_step_f32: out may not be audio (neighbouring tiles read the halo)");
    const dim3 grid((unsigned)((S + kTile - 1) / kTile), B);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (init) {
        ISPK_RESERVE_LDS(griffinlim_kernel<true>, kLds, "ispk_griffinlim_step_f32");
        hipLaunchKernelGGL(griffinlim_kernel<true>, grid, dim3(kThreads), kLds, s, audio, ld_audio, (const float*)nullptr,
                           (int64_t)0, 0.f, mag, ld_mag, mel_len, tables, out, ld_out, audio_len, T, mix_seed(seed));
    } else {
        ISPK_RESERVE_LDS(griffinlim_kernel<false>, kLds, "ispk_griffinlim_step_f32");
        hipLaunchKernelGGL(griffinlim_kernel<false>, grid, dim3(kThreads), kLds, s, audio, ld_audio, (const float*)nullptr,
                           (int64_t)0, 0.f, mag, ld_mag, mel_len, tables, out, ld_out, audio_len, T, mix_seed(seed));
    }
    return ispk_launch_status();
}

extern "C" int32_t ispk_griffinlim_fast_step_f32(const float* audio, int64_t ld_audio, const float* prev, int64_t ld_prev,
                                                 float alpha, const float* mag, int64_t ld_mag, const int64_t* mel_len,
                                                 const float* tables, float* out, int64_t ld_out, int64_t* audio_len,
                                                 int32_t B, int32_t T, ispk_stream_t stream) {
    if (B == 0 || T == 0) return 0;
    ISPK_REQUIRE(audio && prev && mag && tables && out, ISPK_E_NULL, "ispk_griffinlim_fast_step_f32: null pointer");
    ISPK_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= kMaxFrames, ISPK_E_SHAPE,
                 "ispk_griffinlim_fast_step_f32: bad shape B=%d T=%d (B <= 65535, T <= %d)", B, T, kMaxFrames);
    const int64_t S = (int64_t)T * kHop;
    ISPK_REQUIRE(ld_audio >= S && ld_prev >= S && ld_out >= S && ld_mag >= (int64_t)T * kBins, ISPK_E_SHAPE,
                 "ispk_griffinlim_fast_step_f32: row strides ld_audio=%lld ld_prev=%lld ld_out=%lld ld_mag=%lld shorter than "
                 "the rows (T=%d)", (long long)ld_audio, (long long)ld_prev, (long long)ld_out, (long long)ld_mag, T);
    ISPK_REQUIRE(out != audio && out != prev, ISPK_E_SHAPE,
                 "ispk_griffinlim_fast_step_f32: out may not be audio or prev (neighbouring tiles read the halo)");
    ISPK_REQUIRE(alpha >= 0.f && alpha < 1.f, ISPK_E_SHAPE, "ispk_griffinlim_fast_step_f32: alpha %g outside [0, 1)",
                 (double)alpha);
    const dim3 grid((unsigned)((S + kTile - 1) / kTile), B);
    auto kernel = griffinlim_kernel<false, true>;
    ISPK_RESERVE_LDS(kernel, kLds, "ispk_griffinlim_fast_step_f32");
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), kLds, reinterpret_cast<hipStream_t>(stream), audio, ld_audio, prev, ld_prev,
                       alpha, mag, ld_mag, mel_len, tables, out, ld_out, audio_len, T, (uint64_t)0);
    return ispk_launch_status();
}

extern "C" int32_t ispk_griffinlim_error_f32(const float* audio, int64_t ld_audio, const float* mag, int64_t ld_mag,
                                             const int64_t* mel_len, const float* tables, float* work, int64_t ld_work,
                                             float* err, int32_t B, int32_t T, ispk_stream_t stream) {
    if (B == 0 || T == 0) return 0;
    ISPK_REQUIRE(audio && mag && tables && work && err, ISPK_E_NULL, "ispk_griffinlim_error_f32: null pointer");
    ISPK_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= kMaxFrames, ISPK_E_SHAPE,
                 "ispk_griffinlim_error_f32: bad shape B=%d T=%d (B <= 65535, T <= %d)", B, T, kMaxFrames);
    ISPK_REQUIRE(ld_audio >= (int64_t)T * kHop && ld_mag >= (int64_t)T * kBins && ld_work >= 2 * (int64_t)T, ISPK_E_SHAPE,
                 "ispk_griffinlim_error_f32: row strides ld_audio=%lld ld_mag=%lld ld_work=%lld shorter than the rows (T=%d)",
                 (long long)ld_audio, (long long)ld_mag, (long long)ld_work, T);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(griffinlim_error_kernel, dim3((T + kErrFrames - 1) / kErrFrames, B), dim3(kThreads), kErrLds, s, audio,
                       ld_audio, mag, ld_mag, mel_len, tables, work, ld_work, T);
    hipLaunchKernelGGL(griffinlim_error_sum_kernel, dim3(B), dim3(kSumThreads), 0, s, work, ld_work, mel_len, err, T);
    return ispk_launch_status();
}
