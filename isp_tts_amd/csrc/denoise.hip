// Vocoder denoiser (isp_tts_amd/denoiser.py): STFT, spectral bias subtraction and ISTFT of a padded mono batch in ONE launch.
// n_fft = win = 1024, hop 256, periodic Hann, center = true with reflect padding: what torch.stft / torch.istft(length = n)
// and the conv-basis STFT of the FastPitch-family Denoiser compute (include/ispk.h has the definition).
//
//   denoise_kernel   grid (ceil(S / 4096), B), 512 threads = 4 groups of 128.  A workgroup writes 16 hop segments (4096
//                    samples) of ONE utterance of n samples.  Sample s takes frames floor((s + 512) / 256) - 3 .. floor((s +
//                    512) / 256), so the tile at hop q0 needs the up-to-19 frames q0 - 1 .. q0 + 17 within [0, F), F = 1 +
//                    n / 256: the 3 frames it shares with a neighbouring tile are transformed by both (no atomics, no second
//                    pass, nothing in HBM between analysis and synthesis).  Frames run 4 at a time, one per group:
//                      gather    1024 samples x[r(256 f - 512 + j)], r the reflection at 0 and n - 1 (applied on load, never an
//                                index at or past n), times the window, as z[m] = x[2m] + i x[2m+1] into the group's ping buffer;
//                      forward   512-point complex Stockham FFT (fft.h) into the frame's 4 KB slot;
//                      shrink    per bin pair (k, 512 - k): X by real_split, g = |X|^2 > t^2 ? 1 - t / sqrt(|X|^2) : 0 with
//                                t = strength bias[k] (IEEE sqrt and division, no rsq), Y = X g / 1024, packed straight into
//                                the inverse's half-length spectrum Z_k = (Y_k + conj Y_{512-k}) + i (Y_k - conj Y_{512-k})
//                                conj(W_1024^k) in the ping buffer (imaginary parts of bins 0 and 512 dropped, as irfft);
//                      inverse   512-point FFT back into the slot: the frame's 1024 real samples in order;
//                    then per output sample the window-weighted overlap-add of its <= 4 frames and the division by the sum of
//                    their w^2, both in ascending frame order.  Samples at or past n are written as 0; an utterance below 513
//                    samples (reflect padding undefined) is copied.  LDS: 80 KB of frame slots + 16 KB of ping buffers + 8 KB
//                    twiddles + 4 KB window + 2 KB of thresholds, as the ISTFT head lays its own out.
// A frame's arithmetic depends on (n, f) alone and a sample's on (n, s) alone - not on the tile, on B, on S or on the row's
// neighbours - and there are no atomics: a ragged batch gives each utterance the bits it gets alone, and repeated calls and
// graph replays repeat theirs.  Every wave belongs to one transform, so running four side by side changes no LDS access
// pattern: the float2 passes read conflict-free (32 consecutive float2 = the 64 banks) and the stores of the first two
// radix-4 passes (strides of 4 and 16 float2 inside a 16-lane group, banks modulo 32) are 4-way; the later passes store runs of
// 16 consecutive float2.  Four groups keep two waves per SIMD to overlap those stores with the other groups' arithmetic.
//
// gfx950 resources (csrc/resource_report.py denoise.hip; no spills, no scratch):
//   denoise_kernel   72 VGPRs, LDS 112,656 B dynamic (one workgroup per CU)
#include <math.h>

#include "common.h"
#include "fft.h"

namespace {

constexpr int kHop = 256;
constexpr int kNfft = 1024;
constexpr int kHalf = kNfft / 2;                   // 512: center padding, and the complex transform's length
constexpr int kBins = kHalf + 1;                   // 513
constexpr int kSegs = 16;                          // hop segments written per workgroup
constexpr int kTile = kSegs * kHop;                // 4096 samples
constexpr int kSlots = kSegs + 4;                  // frame slots: 19 frames touch a tile, rounded up to whole rounds
constexpr int kGroups = 4;                         // transforms side by side
constexpr int kGT = 128;                           // threads per transform
constexpr int kThreads = kGroups * kGT;
constexpr int kTw = 1024;                          // W_1024^m: the 512-point FFT's twiddles and the split's
constexpr int kThr = 516;                          // 513 thresholds, padded to whole float4s
constexpr int kMinLen = kHalf + 1;                 // below this the reflection is undefined: copy
constexpr size_t kLds = sizeof(cf) * (kTw + kGroups * kHalf) + sizeof(float) * (kNfft + kThr + kSlots * kNfft);

__device__ __forceinline__ int valid_len(const int64_t* audio_len, int b, int S) {
    if (!audio_len) return S;
    const int64_t l = audio_len[b];
    return (l >= 0 && l <= S) ? (int)l : 0;
}

// Y = X max(1 - t / |X|, 0) / 1024, 0 where |X| <= t (so also where |X| = 0)
__device__ __forceinline__ cf shrink(cf X, float t) {
    const float m2 = X.x * X.x + X.y * X.y;
    const float g = m2 > t * t ? (1.0f - t / sqrtf(m2)) * (1.0f / kNfft) : 0.f;
    return make_float2(X.x * g, X.y * g);
}

__global__ void __launch_bounds__(kThreads) denoise_kernel(const float* __restrict__ audio, int64_t lda,
                                                           const int64_t* __restrict__ audio_len,
                                                           const float* __restrict__ tables, const float* __restrict__ bias,
                                                           const float* __restrict__ strength_item, float strength,
                                                           float* __restrict__ out, int64_t ldo, int S) {
    extern __shared__ float4 lds_raw[];
    cf* tw = reinterpret_cast<cf*>(lds_raw);                          // [kTw]
    cf* ping = tw + kTw;                                              // [kGroups][512]
    float* win = reinterpret_cast<float*>(ping + kGroups * kHalf);    // [1024]
    float* thr = win + kNfft;                                         // [kThr]: t_k = strength bias[k], k <= 512
    float* frames = thr + kThr;                                       // [kSlots][1024]

    const int b = blockIdx.y, tid = threadIdx.x, g = tid / kGT, lt = tid % kGT;
    const int n = valid_len(audio_len, b, S);
    const int m0 = blockIdx.x * kTile, m1 = min(S, m0 + kTile);
    const int mv = max(m0, min(n, m1));                               // [m0, mv) are the tile's samples inside the utterance
    const float* xrow = audio + (int64_t)b * lda;
    float* orow = out + (int64_t)b * ldo;

    if (n < kMinLen) {
        for (int m = m0 + tid; m < mv; m += kThreads) orow[m] = xrow[m];
    } else if (mv > m0) {
        const int q0 = blockIdx.x * kSegs, F = 1 + n / kHop;
        const int f_lo = max(0, q0 - 1), f_hi = min(F, (mv - 1 + kHalf) / kHop + 1), nf = f_hi - f_lo;
        float st = strength_item ? strength_item[b] : strength;
        st = st >= 0.f ? st : 0.f;                                    // device data: a negative or NaN strength counts as 0
        const cf* tw2048 = reinterpret_cast<const cf*>(tables);
        for (int i = tid; i < kTw; i += kThreads) tw[i] = tw2048[2 * i];
        for (int i = tid; i < kNfft; i += kThreads) win[i] = tables[2 * 2048 + i];
        for (int i = tid; i < kBins; i += kThreads) thr[i] = st * bias[i];
        __syncthreads();
        cf* A = ping + g * kHalf;
        for (int r = 0; r * kGroups < nf; ++r) {
            const int fs = r * kGroups + g;                           // slot; fs >= nf: transformed, never read
            cf* Bf = reinterpret_cast<cf*>(frames + fs * kNfft);
            if (fs < nf) {
                const int i0 = (f_lo + fs) * kHop - kHalf;            // the frame's first sample, before reflection
                for (int m = lt; m < kHalf; m += kGT) {
                    int ia = i0 + 2 * m, ib = ia + 1;
                    ia = ia < 0 ? -ia : ia >= n ? 2 * (n - 1) - ia : ia;
                    ib = ib < 0 ? -ib : ib >= n ? 2 * (n - 1) - ib : ib;
                    A[m] = make_float2(xrow[ia] * win[2 * m], xrow[ib] * win[2 * m + 1]);
                }
            } else {
                for (int m = lt; m < kHalf; m += kGT) A[m] = make_float2(0.f, 0.f);
            }
            __syncthreads();
            fft<false, kGT, kTw>(A, Bf, kHalf, lt, tw);
            for (int k = lt; k <= 256; k += kGT) {
                const int m = kHalf - k;
                cf xk = shrink(real_split(Bf, k, kHalf, tw[k]), thr[k]);
                cf xm = k == 256 ? xk : shrink(real_split(Bf, m, kHalf, tw[m]), thr[m]);
                if (k == 0) {                                         // irfft drops the imaginary parts of DC and Nyquist
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
            __syncthreads();
            fft<true, kGT, kTw>(A, Bf, kHalf, lt, tw);
        }
        // ---- window, overlap-add over the utterance's own frames, envelope division (frame order, no atomics)
        for (int m = m0 + tid; m < mv; m += kThreads) {
            const int u = m + kHalf;                                  // position in the padded signal
            const int fmin = u >= kNfft ? (u - kNfft) / kHop + 1 : 0, fmax = min(F - 1, u / kHop);
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
    for (int m = mv + tid; m < m1; m += kThreads) orow[m] = 0.f;
}

}  // namespace

extern "C" int32_t ispk_denoise_tile_samples(void) { return kTile; }

extern "C" int32_t ispk_denoise_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables,
                                    const float* bias, const float* strength_item, float strength, float* out, int64_t ld_out,
                                    int32_t B, int32_t S, ispk_stream_t stream) {
    if (B == 0 || S == 0) return 0;
    ISPK_REQUIRE(audio && tables && bias && out, ISPK_E_NULL, "ispk_denoise_f32: null pointer");
    ISPK_REQUIRE(B >= 1 && B <= 65535 && S >= 1 && S <= INT32_MAX - 2 * kTile, ISPK_E_SHAPE,
                 "ispk_denoise_f32: bad shape B=%d S=%d (B <= 65535, S <= 2^31 - 8193)", B, S);
    ISPK_REQUIRE(ld_audio >= S && ld_out >= S, ISPK_E_SHAPE,
                 "ispk_denoise_f32: row strides ld_audio=%lld ld_out=%lld shorter than the rows (S=%d)", (long long)ld_audio,
                 (long long)ld_out, S);
    ISPK_REQUIRE(out != audio, ISPK_E_SHAPE, "ispk_denoise_f32: out may not be audio (neighbouring tiles read the halo)");
    ISPK_REQUIRE(strength >= 0.f, ISPK_E_SHAPE, "ispk_denoise_f32: strength %g is negative or NaN", (double)strength);
    ISPK_RESERVE_LDS(denoise_kernel, kLds, "ispk_denoise_f32");
    hipLaunchKernelGGL(denoise_kernel, dim3((S + kTile - 1) / kTile, B), dim3(kThreads), kLds,
                       reinterpret_cast<hipStream_t>(stream), audio, ld_audio, audio_len, tables, bias, strength_item, strength,
                       out, ld_out, S);
    return ispk_launch_status();
}
