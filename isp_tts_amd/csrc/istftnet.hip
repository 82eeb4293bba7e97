// iSTFTNet output layer (isp_tts_amd/istftnet.py): leaky-ReLU, ReflectionPad1d((1, 0)), the 7-tap C -> n_fft + 2 convolution,
// exp / sin, polar -> rectangular, an n_fft-point inverse real DFT per frame and the windowed overlap-add with the envelope
// division, in ONE kernel: nothing but the stage tensor is read and nothing but audio is written.
//
// An utterance of n valid rows x[0 .. n) has F = n + 1 frames: p[0] = x[1], p[i] = x[i - 1] (the reflection), conv_post runs
// on p with 3 zero rows on both sides, and torch.istft(center = True) of F frames gives hop (F - 1) = hop n samples.  With
// N = n_fft, hop = N / 4, H = N / 2 and the periodic Hann window w, output sample s of the utterance is
//   audio[s] = sum_f w[t_f] g_f[t_f] / sum_f w[t_f]^2,   t_f = s + H - f hop,   over the frames 0 <= f <= n with 0 <= t_f < N
//   g_f[t]   = (1 / N) (Re_0 + (-1)^t Re_H + 2 sum_{k=1}^{H-1} (Re_k cos(2 pi k t / N) - Im_k sin(2 pi k t / N)))
//   Re_k + i Im_k = exp(y_f[k]) exp(i phase_scale sin(y_f[H + 1 + k]))
// (Im_0 and Im_H do not enter, as in irfft), so s in hop block o = s / hop sums the frames o - 1 .. o + 2, in ascending f.
//
//   istftnet_head_kernel<N>   grid (ceil(S / (125 hop)), B), 128 threads, ONE FRAME PER THREAD.  A workgroup owns 125 hop
//       blocks o0 .. o0 + 124 of ONE utterance and computes the 128 frames o0 - 1 .. o0 + 126 they sum (the 3 frames shared with
//       the neighbouring tile are computed by both, bit for bit alike).  Per chunk of 32 channels the 134 padded rows the
//       frames read are staged in LDS (leaky-ReLU applied, the reflection resolved, rows outside [0, F) replaced by zeros with
//       a select; row pitch 33, so the 64 lanes of a wave read 64 banks); thread f runs, per output channel, two fp32 fma
//       chains in (chunk, tap, channel) order - one over the even and one over the odd channels, the two halves of a
//       v_pk_fma_f32 - with the weights as wave-uniform scalar operands, loaded 8 at a time straight from the
//       [7][N + 2][C] image; y = (even + odd) + bias.
//       Then expf / sinf / cosf / sinf per bin, the direct DFT with twiddles cos, sin(2 pi m / N) and the window w / N from
//       the table (made in float64 on the host), the windowed frame into LDS over the dead row window, and every output
//       sample sums its <= 4 frames and its envelope (w^2 from the table) in ascending f and divides.
// Vector FMAs, not MFMA: on gfx950 the exact-fp32 MFMA issues at the fp32 vector peak (64 FLOP / clk / SIMD), so it wins only
// by tile utilisation.  N + 2 = 18 output channels fill 18 / 32 of the two 16-wide MFMA column tiles they need (56 %), while
// v_pk_fma_f32 has no tile to fill, needs no operand layout and no weight staging (the weights are SGPR pairs), reads LDS once
// per 18 packed FMAs, and leaves the kernel one thread per frame from the first tap to the frame's last sample.
// The frame sums are in an order fixed by the position inside the utterance, so a sample's bits depend neither on B, nor on
// the neighbours, nor on the tile it fell into.  No atomics.
//
// gfx950 resources (csrc/resource_report.py istftnet.hip; no spills, no scratch in any instantiation):
//   istftnet_head_kernel<16>   83 VGPRs (5 waves / SIMD), LDS 17,688 B static;  <8> 50,  <20> 118,  <32> 154 VGPRs (3)
#include "common.h"

namespace {

constexpr int kTF = 128;                // frames per workgroup = threads
constexpr int kKC = 32;                 // channels per LDS chunk
constexpr int kMaxC = 512;
constexpr int kWinRows = kTF + 6;       // the frames' rows and the 3-row halo of the 7 taps on both sides
constexpr int kPitch = kKC + 1;         // odd row pitch: consecutive frames read distinct banks
constexpr int kOut = kTF - 3;           // hop blocks a workgroup owns: a block sums 4 consecutive frames

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// table: cos(2 pi m / N) [N], sin(2 pi m / N) [N], w[t] / N [N], w[t]^2 [N]
template <int N>
__global__ __launch_bounds__(kTF) void istftnet_head_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ table,
                                                            const int64_t* __restrict__ len, int len_mul,
                                                            float* __restrict__ audio, int64_t lda,
                                                            int64_t* __restrict__ audio_len, int T, int S, int C, float slope,
                                                            float phase_scale) {
    constexpr int NO = N + 2, H = N / 2, HOP = N / 4, FP = N + 1;
    static_assert(kTF * FP <= kWinRows * kPitch, "the frames reuse the row window");
    __shared__ float smem[kWinRows * kPitch];
    const int b = blockIdx.y, tid = threadIdx.x, o0 = blockIdx.x * kOut;
    int n = valid_len(len, b, T, len_mul);
    if (n < 2) n = 0;                                  // one row has no reflection: counts as empty
    if (blockIdx.x == 0 && tid == 0 && audio_len) audio_len[b] = (int64_t)HOP * n;
    float* arow = audio + (int64_t)b * lda;
    const int s0 = o0 * HOP;
    if (o0 >= n) {
        for (int i = tid; i < kOut * HOP; i += kTF)
            if (s0 + i < S) arow[s0 + i] = 0.f;
        return;
    }
    const float* xb = x + (int64_t)b * T * ldx;
    const int fa = o0 - 1;                             // the tile's first frame; thread tid has frame fa + tid
    f32x2 acc[NO];                                     // per output channel: the sums over its even and its odd channels
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[o] = f32x2{0.f, 0.f};
    for (int c0 = 0; c0 < C; c0 += kKC) {
        __syncthreads();
        for (int idx = tid; idx < kWinRows * 8; idx += kTF) {
            const int wr = idx >> 3, c4 = (idx & 7) * 4, pi = fa - 3 + wr;      // padded row pi = x row (pi ? pi - 1 : 1)
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pi >= 0 && pi <= n) {
                v = *reinterpret_cast<const float4*>(xb + (int64_t)(pi == 0 ? 1 : pi - 1) * ldx + c0 + c4);
                v.x = lrelu(v.x, slope); v.y = lrelu(v.y, slope); v.z = lrelu(v.z, slope); v.w = lrelu(v.w, slope);
            }
            float* d = smem + wr * kPitch + c4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        __syncthreads();
#pragma unroll 1
        for (int j = 0; j < 7; ++j) {
            const float* wj = w + (int64_t)j * NO * C + c0;
            const float* xr = smem + (tid + j) * kPitch;
#pragma unroll 1
            for (int c = 0; c < kKC; c += 8) {
                f32x2 xv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { xv[i].x = xr[c + 2 * i]; xv[i].y = xr[c + 2 * i + 1]; }
#pragma unroll
                for (int o = 0; o < NO; ++o) {
                    const float* wo = wj + o * C + c;          // 8 consecutive weights: one scalar load, 4 SGPR pairs
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        f32x2 wv;
                        wv.x = wo[2 * i]; wv.y = wo[2 * i + 1];
                        acc[o] = __builtin_elementwise_fma(xv[i], wv, acc[o]);
                    }
                }
            }
        }
    }
    __syncthreads();                                   // every frame has read its rows: the window becomes the frames
    float y[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) y[o] = (acc[o].x + acc[o].y) + bias[o];

    // bins: Re_k, Im_k, doubled for 0 < k < H
    float re[H + 1], im[H + 1];
#pragma unroll
    for (int k = 0; k <= H; ++k) {
        const float mag = expf(y[k]);
        const float ph = phase_scale * sinf(y[H + 1 + k]);
        const float two = (k == 0 || k == H) ? 1.f : 2.f;
        re[k] = two * (mag * cosf(ph));
        im[k] = two * (mag * sinf(ph));
    }
    float* fr = smem + tid * FP;
#pragma unroll
    for (int t = 0; t < N; ++t) {
        float v = (t & 1) ? re[0] - re[H] : re[0] + re[H];
#pragma unroll
        for (int k = 1; k < H; ++k) {
            const int m = (k * t) % N;
            v = fmaf(re[k], table[m], v);
            v = fmaf(-im[k], table[N + m], v);
        }
        fr[t] = v * table[2 * N + t];
    }
    __syncthreads();

    const int n_out = HOP * n;
    for (int i = tid; i < kOut * HOP; i += kTF) {
        const int s = s0 + i;
        if (s >= S) break;
        float v = 0.f;
        if (s < n_out) {
            const int lo = i / HOP, r = i - lo * HOP;          // local hop block: frames lo .. lo + 3 of the tile
            float sum = 0.f, env = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int f = fa + lo + q, t = r + (3 - q) * HOP;
                if (f >= 0 && f <= n) {
                    sum += smem[(lo + q) * FP + t];
                    env += table[3 * N + t];
                }
            }
            v = sum / env;
        }
        arow[s] = v;
    }
}

template <int N>
void launch(dim3 grid, hipStream_t s, const float* x, int64_t ldx, const float* w, const float* bias, const float* table,
            const int64_t* len, int len_mul, float* audio, int64_t lda, int64_t* audio_len, int T, int S, int C, float slope,
            float phase_scale) {
    hipLaunchKernelGGL(istftnet_head_kernel<N>, grid, dim3(kTF), 0, s, x, ldx, w, bias, table, len, len_mul, audio, lda, audio_len,
                       T, S, C, slope, phase_scale);
}

}  // namespace

extern "C" int32_t ispk_istftnet_tile_frames(void) { return kTF; }

extern "C" int32_t ispk_istftnet_head_f32(const float* x, int64_t ldx, const float* w, const float* bias, const float* table,
                                          int32_t table_floats, const int64_t* len, int32_t len_mul, float* audio,
                                          int64_t ld_audio, int64_t* audio_len, int32_t B, int32_t T, int32_t S, int32_t C,
                                          int32_t n_fft, int32_t hop, float slope, float phase_scale, ispk_stream_t stream) {
    const char* what = "ispk_istftnet_head_f32";
    if (B == 0) return 0;
    ISPK_REQUIRE(x && w && bias && table && audio, ISPK_E_NULL, "%s: null pointer", what);
    ISPK_REQUIRE(n_fft >= 8 && n_fft <= 32 && n_fft % 4 == 0 && hop * 4 == n_fft, ISPK_E_UNSUPPORTED,
                 "%s: unsupported geometry n_fft=%d hop=%d (n_fft a multiple of 4 from 8 to 32 with hop = n_fft / 4 is built)",
                 what, n_fft, hop);
    ISPK_REQUIRE(B >= 1 && B <= 65535 && T >= 2 && T <= INT32_MAX / hop && S >= hop * T && ld_audio >= S && len_mul >= 1 &&
                     table_floats >= 4 * n_fft,
                 ISPK_E_SHAPE,
                 "%s: bad shape B=%d T=%d S=%d ld_audio=%lld len_mul=%d table_floats=%d (T >= 2, S >= hop T, ld_audio >= S, "
                 "table >= 4 n_fft floats)",
                 what, B, T, S, (long long)ld_audio, len_mul, table_floats);
    ISPK_REQUIRE(C >= 32 && C <= kMaxC && C % 32 == 0, ISPK_E_UNSUPPORTED,
                 "%s: unsupported channel count C=%d (multiples of 32 up to %d are built)", what, C, kMaxC);
    ISPK_REQUIRE(ldx >= C && ldx % 4 == 0 && ispk_aligned(x, 16), ISPK_E_ALIGN,
                 "%s: x needs 16-byte aligned rows of at least C floats (ldx=%lld)", what, (long long)ldx);
    const dim3 grid((S + kOut * hop - 1) / (kOut * hop), B);
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define ISPK_ISTFTNET_CASE(N)                                                                                            \
    case N:                                                                                                              \
        launch<N>(grid, s, x, ldx, w, bias, table, len, len_mul, audio, ld_audio, audio_len, T, S, C, slope, phase_scale); \
        break;
    switch (n_fft) {
        ISPK_ISTFTNET_CASE(8)
        ISPK_ISTFTNET_CASE(12)
        ISPK_ISTFTNET_CASE(16)
        ISPK_ISTFTNET_CASE(20)
        ISPK_ISTFTNET_CASE(24)
        ISPK_ISTFTNET_CASE(28)
        ISPK_ISTFTNET_CASE(32)
    }
#undef ISPK_ISTFTNET_CASE
    return ispk_launch_status();
}
