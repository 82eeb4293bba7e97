// Vocoder denoiser (isp_tts_amd/denoiser.py): STFT, spectral bias subtraction and ISTFT of a padded mono batch in ONE launch.
// n_fft = win = 1024, hop 256, periodic Hann, center = true with reflect padding: what torch.stft / torch.istft(length = n)
// and the conv-basis STFT of the FastPitch-family Denoiser compute (include/ispk.h has the definition).
//
//   denoise_kernel   the 1024 / 256 tile of stft_tile.h (geometry, LDS, bank and bit-reproducibility notes are there) with 512
//                    samples of reflect padding in front: sample s takes frames floor((s + 512) / 256) - 3 .. floor((s + 512) /
//                    256), so the tile at hop q0 needs the up-to-19 frames q0 - 1 .. q0 + 17 within [0, F), F = 1 + n / 256.
//                    Per frame:
//                      gather    1024 samples x[r(256 f - 512 + j)], r the reflection at 0 and n - 1 (applied on load, never an
//                                index at or past n), times the window, as z[m] = x[2m] + i x[2m+1] into the group's ping buffer;
//                      forward   512-point FFT into the frame's slot;
//                      shrink    per bin pair (k, 512 - k): X by real_split, g = |X|^2 > t^2 ? 1 - t / sqrt(|X|^2) : 0 with
//                                t = strength bias[k] (IEEE sqrt and division, no rsq), Y = X g / 1024, packed straight into
//                                the inverse's half-length spectrum (pack_pairs);
//                      inverse   512-point FFT back into the slot;
//                    then the overlap-add over the utterance's F frames.  Samples at or past n are written as 0; an utterance
//                    below 513 samples (reflect padding undefined) is copied.  LDS: the tile's, plus 2 KB of thresholds between
//                    the window and the frame slots.  A frame's arithmetic depends on (n, f, strength) alone.
//
// gfx950 resources (csrc/resource_report.py denoise.hip; no spills, no scratch):
//   denoise_kernel   72 VGPRs, LDS 112,656 B dynamic (one workgroup per CU)
#include <math.h>

#include "common.h"
#include "stft_tile.h"

namespace {

constexpr int kThr = 516;                          // 513 thresholds, padded to whole float4s
constexpr int kMinLen = kHalf + 1;                 // below this the reflection is undefined: copy
constexpr size_t kDenoiseLds = kLds + sizeof(float) * kThr;
static_assert(kThr % 4 == 0, "the frame slots after the thresholds are read and written as float2 / float4");

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
    const TileLds tile = carve_tile(lds_raw, kThr);
    float* thr = tile.win + kNfft;                                       // [kThr]: t_k = strength bias[k], k <= 512

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
        load_tables(tile.tw, tile.win, tables, tid);
        for (int i = tid; i < kBins; i += kThreads) thr[i] = st * bias[i];
        __syncthreads();
        cf* A = tile.ping + g * kHalf;
        for (int r = 0; r * kGroups < nf; ++r) {
            const int fs = r * kGroups + g;                           // slot; fs >= nf: transformed, never read
            cf* Bf = reinterpret_cast<cf*>(tile.frames + fs * kNfft);
            if (fs < nf) {
                const int i0 = (f_lo + fs) * kHop - kHalf;            // the frame's first sample, before reflection
                for (int m = lt; m < kHalf; m += kGT) {
                    int ia = i0 + 2 * m, ib = ia + 1;
                    ia = ia < 0 ? -ia : ia >= n ? 2 * (n - 1) - ia : ia;
                    ib = ib < 0 ? -ib : ib >= n ? 2 * (n - 1) - ib : ib;
                    A[m] = make_float2(xrow[ia] * tile.win[2 * m], xrow[ib] * tile.win[2 * m + 1]);
                }
            } else {
                clear_frame(A, lt);
            }
            __syncthreads();
            fft<false, kGT, kTw>(A, Bf, kHalf, lt, tile.tw);
            pack_pairs(A, lt, tile.tw, [&](int k, int m, cf& xk, cf& xm) {
                xk = shrink(real_split(Bf, k, kHalf, tile.tw[k]), thr[k]);
                xm = k == 256 ? xk : shrink(real_split(Bf, m, kHalf, tile.tw[m]), thr[m]);
            });
            __syncthreads();
            fft<true, kGT, kTw>(A, Bf, kHalf, lt, tile.tw);
        }
        overlap_add(orow, tile.frames, tile.win, m0, mv, kHalf, f_lo, F, tid);   // pad 512: center = true
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
    ISPK_RESERVE_LDS(denoise_kernel, kDenoiseLds, "ispk_denoise_f32");
    hipLaunchKernelGGL(denoise_kernel, dim3((S + kTile - 1) / kTile, B), dim3(kThreads), kDenoiseLds,
                       reinterpret_cast<hipStream_t>(stream), audio, ld_audio, audio_len, tables, bias, strength_item, strength,
                       out, ld_out, S);
    return ispk_launch_status();
}
