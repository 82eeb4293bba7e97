// Acoustic features from waveforms (the reference's data providers, tts/data/providers.py:35-111, 178-188, 280-348 with
// tts/data/pitch.py:17-100 and the pitch pad of tts/data/dataset.py:152): slaney log-mel, energy and torch-yin pitch of a
// zero-padded batch, in the collator's layout, in ONE launch.
//
//   features_kernel  grid (ceil(M / kFrames), B), 512 threads = two halves of 256.  A workgroup stages the padded samples of
//                    its kFrames frames once (STFT frame t and YIN frame t both start at padded sample 256 t), then runs the
//                    frames in pairs, one frame per half:
//                      STFT   1024-point real FFT of the Hann-windowed frame (a 512-point complex Stockham FFT + the split)
//                             -> |X_k|, k <= 512 -> sparse mel product, log(max(., 1e-5)); log1p(sqrt(sum |X_k|^2))
//                      YIN    2048-point real FFT of the 2 tau_max samples (zero-padded; 3 tau_max <= 2048, so no lag below
//                             tau_max wraps) -> |X_k|^2 -> inverse real FFT -> the linear autocorrelation r(t), t < tau_max;
//                             torch-yin's difference function and cmdf from in-workgroup scans; the first-index searches as
//                             min-reductions; tau -> Hz with torch's reciprocal-then-multiply; (pitch - mean) / std.
//                    Every FFT pass is radix 4 (one radix-2 pass for 512 points) in LDS with a float64-made twiddle table
//                    (fft.h, shared with the vocoder's ISTFT head).
// Every sum runs in a fixed order and there are no atomics: repeated calls and graph replays give the same bits.
#include <algorithm>

#include "common.h"
#include "fft.h"

namespace {

constexpr int kFrames = 8;                          // STFT frames per workgroup (even: frames run in pairs)
constexpr int kHop = 256;
constexpr int kPadL = 384;                          // int((n_fft - hop) / 2), both providers
constexpr int kBins = 513;                          // n_fft / 2 + 1
constexpr int kThreads = 512;
constexpr int kHalf = 256;                          // threads per frame
constexpr int kMaxTauMax = 682;                     // 3 tau_max <= 2048
constexpr int kStage = (kFrames - 1) * kHop + 2 * kMaxTauMax;   // 3156 padded samples per workgroup (a multiple of 4)
constexpr int kMaxMels = 128;
constexpr int kMaxFbWeights = 2 * kBins;            // a bin lies inside at most two adjacent triangles
constexpr int kTw = 2048;                           // twiddle table: W_2048^m, m < 2048
constexpr int kTableHead = 2 * kTw + 1024;          // tables: twiddles, then the window, then the filterbank weights
constexpr float kClip = 1e-5f;                      // F.dynamic_range_compression clip_val; also pitch.py:85's floor

// Inclusive scan of v[0, n) by the 256 threads of one half (wave `hw` of 4 within it): consecutive chunks per thread, a
// shuffle scan per wave, the wave totals in order.  Fixed order throughout.  Ends with a barrier.
__device__ __forceinline__ void scan_inclusive(float* v, int n, int lt, float* wsum) {
    const int per = (n + kHalf - 1) / kHalf;
    const int lo = min(n, lt * per), hi = min(n, lo + per);
    const int lane = lt % kWave, hw = lt / kWave;
    float s = 0.f;
    for (int i = lo; i < hi; ++i) s += v[i];
    float x = s;
    for (int o = 1; o < kWave; o <<= 1) {
        const float y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == kWave - 1) wsum[hw] = x;
    __syncthreads();
    float off = x - s;
    for (int w = 0; w < hw; ++w) off += wsum[w];
    for (int i = lo; i < hi; ++i) {
        off += v[i];
        v[i] = off;
    }
    __syncthreads();
}

// Sum of one value per thread over the half, in a fixed order (xor butterfly per wave, then the 4 waves in order).
__device__ __forceinline__ float half_sum(float x, int lt, float* wsum) {
    for (int o = kWave / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if (lt % kWave == 0) wsum[lt / kWave] = x;
    __syncthreads();
    const float r = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ int half_min(int x, int lt, int* wmin) {
    for (int o = kWave / 2; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o));
    if (lt % kWave == 0) wmin[lt / kWave] = x;
    __syncthreads();
    const int r = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
    __syncthreads();
    return r;
}

struct YinArgs {
    int tau_min, tau_max;
    float sample_rate, threshold, mean, std;
};

// pitch.py:55-59 then providers.py:348, operation by operation: sample_rate / tensor is torch's reciprocal(tensor) *
// sample_rate (two fp32 roundings, not one division); unvoiced (tau = 0) is 0 Hz; then (p - mean) / std.  Uncontracted.
__device__ __forceinline__ float pitch_value(int tau, const YinArgs& y) {
#pragma clang fp contract(off)
    const float hz = tau > 0 ? __fmul_rn(__frcp_rn((float)(tau + y.tau_min + 1)), y.sample_rate) : 0.f;
    return __fdiv_rn(__fsub_rn(hz, y.mean), y.std);
}

__global__ void __launch_bounds__(kThreads) features_kernel(const float* __restrict__ audio, int64_t ld, bool vec,
                                                            const int64_t* __restrict__ audio_len, const float* __restrict__ tables,
                                                            int max_fb, const int32_t* __restrict__ fb_index, int n_mels, float* __restrict__ mel,
                                                            int64_t* __restrict__ mel_len_out, float* __restrict__ pitch,
                                                            float* __restrict__ energy, int S, int M, YinArgs y) {
    extern __shared__ float4 lds_raw[];
    cf* tw = reinterpret_cast<cf*>(lds_raw);                         // [kTw]
    cf* buf = tw + kTw;                                              // [2 halves][2][1024]
    float* smp = reinterpret_cast<float*>(buf + 4 * 1024);           // [kStage]
    float* fbw = smp + kStage;                                       // [kMaxFbWeights]
    float* mel_s = fbw + kMaxFbWeights;                              // [kMaxMels][kFrames]
    int* fb_lo = reinterpret_cast<int*>(mel_s + kMaxMels * kFrames); // [kMaxMels]
    int* fb_off = fb_lo + kMaxMels;                                  // [kMaxMels + 1]
    __shared__ float wsum[2][4];
    __shared__ int wmin[2][4];
    __shared__ float en_s[kFrames], pitch_s[kFrames];

    const int b = blockIdx.y, t0 = blockIdx.x * kFrames;
    const int tid = threadIdx.x, h = tid / kHalf, lt = tid % kHalf;

    // ---- lengths (device data: out of range -> no frames)
    const int64_t L64 = audio_len[b];
    const bool ok = L64 >= kHop && L64 <= S;
    const int L = ok ? (int)L64 : 0;
    const int n_mel = ok ? (L - kHop) / kHop + 1 : 0;                            // (S + 768 - 1024) // 256 + 1
    const int FL = 2 * y.tau_max;
    const int n_pitch = ok ? min(n_mel, (max(L + 2 * kPadL, FL) - FL) / kHop + 1) : 0;   // pitch.py:62-66, then dataset.py:152
    if (blockIdx.x == 0 && tid == 0 && mel_len_out) mel_len_out[b] = n_mel;
    const int nvalid = max(0, min(kFrames, n_mel - t0));

    if (nvalid > 0) {
        // ---- tables and samples: padded sample 256 t0 + i is audio[256 t0 - 384 + i] inside [0, L), zero elsewhere
        for (int i = tid; i < kTw; i += kThreads) tw[i] = reinterpret_cast<const cf*>(tables)[i];
        if (mel) {
            for (int m = tid; m < n_mels; m += kThreads) {
                const int lo = min(max(fb_index[m], 0), kBins);
                fb_lo[m] = lo;
                fb_off[m] = min(max(fb_index[n_mels + m], 0), max_fb);
            }
            if (tid == 0) fb_off[n_mels] = min(max(fb_index[2 * n_mels], 0), max_fb);
            const int nnz = min(max(fb_index[2 * n_mels], 0), max_fb);      // (never past the table)
            for (int i = tid; i < nnz; i += kThreads) fbw[i] = tables[kTableHead + i];
        }
        const float* row = audio + (int64_t)b * ld;
        const int a0 = t0 * kHop - kPadL;
        for (int i = 4 * tid; i < kStage; i += 4 * kThreads) {
            const int a = a0 + i;
            if (vec && a >= 0 && a + 3 < L) {
                *reinterpret_cast<f32x4*>(smp + i) = *reinterpret_cast<const f32x4*>(row + a);
            } else {
                for (int j = 0; j < 4; ++j) smp[i + j] = (a + j >= 0 && a + j < L) ? row[a + j] : 0.f;
            }
        }
        __syncthreads();

        const float* win = tables + 2 * kTw;
        cf* A = buf + h * 2048;
        cf* Bf = A + 1024;
        float* Af = reinterpret_cast<float*>(A);
        float* Bff = reinterpret_cast<float*>(Bf);
        for (int p = 0; 2 * p < nvalid; ++p) {
            const int f = 2 * p + h;                 // this half's frame in the block (f >= nvalid: computed, not kept)
            const float* x = smp + f * kHop;
            if (mel || energy) {
                // ---- STFT: 1024-point real FFT of the windowed frame
                for (int n = lt; n < 512; n += kHalf)
                    A[n] = make_float2(win[2 * n] * x[2 * n], win[2 * n + 1] * x[2 * n + 1]);
                __syncthreads();
                fft<false, kHalf, kTw>(A, Bf, 512, lt, tw);
                float e2 = 0.f;
                for (int k = lt; k < kBins; k += kHalf) {
                    const cf X = real_split(Bf, k, 512, tw[2 * k]);
                    const float mag = sqrtf(X.x * X.x + X.y * X.y);
                    Af[k] = mag;
                    e2 += mag * mag;
                }
                const float etot = half_sum(e2, lt, wsum[h]);       // (its barriers also publish Af)
                if (lt == 0) en_s[f] = log1pf(sqrtf(etot));
                if (mel) {
                    for (int m = lt; m < n_mels; m += kHalf) {
                        const int lo = fb_lo[m], o0 = fb_off[m];
                        const int w = min(max(fb_off[m + 1] - o0, 0), kBins - lo);
                        float acc = 0.f;
                        for (int k = 0; k < w; ++k) acc += Af[lo + k] * fbw[o0 + k];
                        mel_s[m * kFrames + f] = logf(fmaxf(acc, kClip));
                    }
                }
                __syncthreads();
            }
            if (pitch && 2 * p < n_pitch - t0) {
                // ---- YIN: autocorrelation by a 2048-point real FFT of the FL samples, zero-padded
                for (int n = lt; n < 1024; n += kHalf)
                    A[n] = make_float2(2 * n < FL ? x[2 * n] : 0.f, 2 * n + 1 < FL ? x[2 * n + 1] : 0.f);
                __syncthreads();
                fft<false, kHalf, kTw>(A, Bf, 1024, lt, tw);
                for (int k = lt; k <= 1024; k += kHalf) {
                    const cf X = real_split(Bf, k, 1024, tw[k]);
                    Af[k] = X.x * X.x + X.y * X.y;                  // |X_k|^2, real and even in k
                }
                __syncthreads();
                for (int k = lt; k < 1024; k += kHalf) {            // the half-length inverse: Z_k = E_k + i O_k
                    const float pk = Af[k], pm = Af[1024 - k];
                    const float e = 0.5f * (pk + pm), od = 0.5f * (pk - pm);
                    const cf o = ctw<true>(make_float2(od, 0.f), tw[k]);
                    Bf[k] = make_float2(e - o.y, o.x);
                }
                __syncthreads();
                fft<true, kHalf, kTw>(Bf, A, 1024, lt, tw);         // A[n] = 1024 (r[2n] + i r[2n+1])
                // squares -> prefix sums (Bff[0, FL)); the difference function from lag 1 (Bff[FL, FL + tau_max - 1))
                for (int i = lt; i < FL; i += kHalf) Bff[i] = x[i] * x[i];
                __syncthreads();
                scan_inclusive(Bff, FL, lt, wsum[h]);
                const float c0 = Bff[FL - 1];                       // sqrcs[-1]
                float* d = Bff + FL;
                const int nd = y.tau_max - 1;
                for (int t = 1 + lt; t < y.tau_max; t += kHalf) {
                    const float ct = Bff[FL - t - 1] - Bff[t - 1];  // sqrcs.flip(-1)[t] - sqrcs[t]: sum_{j=t}^{FL-1-t} x_j^2
                    const float r = Af[t] * (1.f / 1024.f);
                    d[t - 1] = (c0 + ct) - 2.f * r;
                }
                __syncthreads();
                // cmdf[j] = d[j] (j + 1) / max(cumsum(d)[j], 1e-5): keep d, scan a copy in Af (r is no longer needed)
                float* cs = Af;
                for (int j = lt; j < nd; j += kHalf) cs[j] = d[j];
                __syncthreads();
                scan_inclusive(cs, nd, lt, wsum[h]);
                for (int j = lt; j < nd; j += kHalf) d[j] = d[j] * (float)(j + 1) / fmaxf(cs[j], kClip);
                __syncthreads();
                // ---- search over c[i] = cmdf[tau_min + i], i < nc (pitch.py:89-100)
                const float* c = d + y.tau_min;
                const int nc = nd - y.tau_min;
                int first = nc;
                for (int i = lt; i < nc; i += kHalf)
                    if (c[i] < y.threshold) first = min(first, i);
                first = half_min(first, lt, wmin[h]);
                // argmax 0 (none below, or index 0 below) means "none": then no index qualifies and tau = 0
                const int from = first > 0 ? first : nc;
                int best = nc;
                for (int i = from + lt; i < nc; i += kHalf)
                    if (i == nc - 1 || c[i + 1] - c[i] >= 0.f) best = min(best, i);
                best = half_min(best, lt, wmin[h]);
                if (lt == 0) pitch_s[f] = pitch_value(best < nc ? best : 0, y);
                __syncthreads();
            }
        }
        __syncthreads();
    }

    // ---- the block's columns, zero past mel_len (pitch: past the YIN frame count too)
    if (mel) {
        float* mb = mel + (int64_t)b * n_mels * M;
        for (int i = tid; i < n_mels * kFrames; i += kThreads) {
            const int m = i / kFrames, f = i % kFrames, t = t0 + f;
            if (t < M) mb[(int64_t)m * M + t] = f < nvalid ? mel_s[m * kFrames + f] : 0.f;
        }
    }
    if (tid < kFrames && t0 + tid < M) {
        const int t = t0 + tid;
        if (energy) energy[(int64_t)b * M + t] = tid < nvalid ? en_s[tid] : 0.f;
        if (pitch) pitch[(int64_t)b * M + t] = t < n_pitch ? pitch_s[tid] : 0.f;
    }
}

}  // namespace

extern "C" int32_t ispk_audio_features_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables,
                                           int64_t table_floats, const int32_t* fb_index, int32_t n_mels, float* mel, int64_t* mel_len, float* pitch,
                                           float* energy, int32_t B, int32_t S, int32_t M, int32_t tau_min, int32_t tau_max,
                                           float sample_rate, float threshold, float pitch_mean, float pitch_std,
                                           ispk_stream_t stream) {
    ISPK_REQUIRE(audio && audio_len && tables, -1, "ispk_audio_features_f32: null pointer");
    ISPK_REQUIRE(!mel || fb_index, -1, "ispk_audio_features_f32: null filterbank index");
    ISPK_REQUIRE(table_floats >= kTableHead, -2, "ispk_audio_features_f32: tables hold %lld floats, need at least %d",
                 (long long)table_floats, kTableHead);
    const int max_fb = (int)std::min<int64_t>(kMaxFbWeights, table_floats - kTableHead);
    ISPK_REQUIRE(B >= 1 && B <= 65535 && S >= 0 && ld_audio >= S, -2, "ispk_audio_features_f32: bad shape B=%d S=%d ld=%lld",
                 B, S, (long long)ld_audio);
    const int frames = S >= kHop ? (S - kHop) / kHop + 1 : 0;
    ISPK_REQUIRE(M >= frames && M <= 0x7fffffff / kMaxMels, -2, "ispk_audio_features_f32: M=%d below the %d frames of S=%d", M,
                 frames, S);
    ISPK_REQUIRE(!mel || (n_mels >= 1 && n_mels <= kMaxMels), -2, "ispk_audio_features_f32: n_mels=%d not in [1, %d]", n_mels,
                 kMaxMels);
    ISPK_REQUIRE(!pitch || (tau_min >= 1 && tau_max - 1 - tau_min >= 1 && 3 * tau_max <= 2048 && 2 * tau_max >= 2 * kPadL + kHop),
                 -2, "ispk_audio_features_f32: tau_min=%d tau_max=%d outside 1 <= tau_min < tau_max - 1, 3 tau_max <= 2048, "
                 "2 tau_max >= 1024", tau_min, tau_max);
    ISPK_REQUIRE(!pitch || pitch_std != 0.f, -2, "ispk_audio_features_f32: pitch std is 0");
    const bool vec = ld_audio % 4 == 0 && ispk_aligned(audio, 16);
    const size_t lds = sizeof(cf) * (kTw + 4 * 1024) + sizeof(float) * (kStage + kMaxFbWeights + kMaxMels * kFrames) +
                       sizeof(int) * (2 * kMaxMels + 1);
    ISPK_RESERVE_LDS(features_kernel, lds, "ispk_audio_features_f32");
    const YinArgs y{tau_min, tau_max, sample_rate, threshold, pitch_mean, pitch_std};
    const int nblk = M > 0 ? (M + kFrames - 1) / kFrames : 1;
    hipLaunchKernelGGL(features_kernel, dim3(nblk, B), dim3(kThreads), lds, reinterpret_cast<hipStream_t>(stream), audio,
                       ld_audio, vec, audio_len, tables, max_fb, fb_index, n_mels, mel, mel_len, pitch, energy, S, M, y);
    return ispk_launch_status();
}
