// HiFi-GAN generator (isp_tts_amd/hifigan.py): the dense dilated Conv1d, the ConvTranspose1d and the output layer.  conv_pre
// runs through ispk_vocoder_unfold + ispk_gemm_{f32,bf16}.
//
// Activations are fp32 rows [B * T][C] (row b*T + t = sample t of utterance b).  A convolution is an implicit GEMM with
// M = time, N = C_out, K = taps x C_in: nothing is unfolded in memory.
//
//   hifigan_conv_kernel<BF, WN, TNT>   grid (ceil(T / 128), (C_out / BN) * u, B), 256 threads = 4 waves as (4 / WN) x WN, a
//       wave TMT x TNT accumulator tiles of 32 x 32: a workgroup owns 128 input-time positions of ONE utterance x
//       BN = 32 WN TNT output channels (128, 64 or 32, the largest that divides C_out) [x one output phase].  Per chunk of 32
//       input channels the window of 128 + span input rows (the tile plus its halo) is staged ONCE in LDS - leaky-ReLU
//       applied, rows outside [0, len_b) replaced by zeros with a select, rounded to bf16 on the bf16 path - and every tap
//       reads it at its own row offset; the tap's [BN][32] weight tile is register-staged and double-buffered, one barrier
//       per (chunk, tap) step.  fp32: v_mfma_f32_32x32x2_f32 (exact fp32 products, rows padded to 36 dwords and read as
//       4 consecutive k per lane exactly as gemm_f32_kernel does); bf16: v_mfma_f32_32x32x16_bf16 (rows padded to 80 B).
//       Both modes are one tap schedule  tap_m = tap0 + m tapstep,  row offset off_m = off0 + m offstep:
//         Conv1d(k, dilation d, padding (k-1)d/2)        taps 0 .. k-1, offsets (m - (k-1)/2) d, output row t
//         ConvTranspose1d(k, stride u, padding p=(k-u)/2) phase r = blockIdx.y % u writes output rows t u + r from the taps
//                                                         j = q0 + m u (q0 = (r + p) mod u, j < k) at offsets
//                                                         floor((r + p) / u) - m: every output row has one owner, no atomics
//       Epilogue: + bias, + residual row, then out = scale * v or out = fma(scale, v, out) (the MRF mean accumulated by the
//       last unit of each ResBlock); output rows at or past the utterance's length are written as zeros.  A tile that lies
//       wholly past the length writes its zeros and leaves.
//   hifigan_post_kernel<CLAMP>         grid (ceil(S / 256), B), 256 threads, one output sample each: leaky-ReLU -> 7-tap
//       C -> 1 convolution (fp32 fma chain in channel-chunk, tap, channel order over an LDS window of 262 rows x 32 channels,
//       row pitch 33) -> + bias -> tanhf, or clamp to [-1, 1] (BigVGAN's use_tanh_at_final = false); zeros at and past the
//       utterance's length; audio_len.
// Sums run in a fixed order that depends only on the position inside the utterance: a ragged batch gives each utterance the
// bits it gets alone, and repeated calls and graph replays give the same bits.  A device length outside [0, T] counts as 0.
//
// gfx950 resources (csrc/resource_report.py hifigan.hip; no spills, no scratch in any).  LDS of the convolution kernel is
// dynamic, (2 BN + 128 + span) rows of 144 B (fp32) or 80 B (bf16), span = (k - 1) d <= 120:
//   hifigan_conv_kernel<f32, 2, 2>   BN 128   96 VGPRs + 64 AGPRs (3 waves / SIMD)   LDS <= 72,576 B
//   hifigan_conv_kernel<f32, 2, 1>   BN 64    66 VGPRs + 33 AGPRs (4)                    <= 54,144 B
//   hifigan_conv_kernel<f32, 1, 1>   BN 32    42 VGPRs + 16 AGPRs (8)                    <= 44,928 B
//   hifigan_conv_kernel<bf16, 2, 2>  BN 128   94 VGPRs + 64 AGPRs (3)                    <= 40,320 B
//   hifigan_conv_kernel<bf16, 2, 1>  BN 64    50 VGPRs + 33 AGPRs (5)                    <= 30,080 B
//   hifigan_conv_kernel<bf16, 1, 1>  BN 32    42 VGPRs + 16 AGPRs (8)                    <= 24,960 B
//   hifigan_post_kernel                       28 VGPRs, LDS 34,584 B static
#include "common.h"

namespace {

constexpr int kTM = 128;          // time positions per workgroup
constexpr int kKC = 32;           // input channels per LDS chunk
constexpr int kMaxC = 512;

struct ConvParams {
    const float* x;
    int64_t ldx;
    const void* w;                // [k][C_out][C_in], fp32 or bf16
    const float* bias;
    const float* resid;
    int64_t ldr;
    float* out;
    int64_t ldo;
    const int64_t* len;
    int len_mul;
    int B, T, C_in, C_out;
    int k, dil, up, pad, transposed;
    float slope, scale;
    int accumulate;
};

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

template <bool BF, int WN, int TNT>
__global__ __launch_bounds__(256) void hifigan_conv_kernel(ConvParams p) {
    constexpr int WM = 4 / WN, TMT = 4 / WM;
    constexpr int BN = 32 * WN * TNT;
    constexpr int PX = BF ? 80 : 144;                 // bytes per LDS row: 32 channels + 16 B
    constexpr int VPR = BF ? 4 : 8;                   // 16-byte vectors per weight row
    constexpr int NW = (BN * VPR + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* Ws = smem_raw;                              // [2][BN] rows
    char* Xs = smem_raw + 2 * BN * PX;                // [kTM + span] rows

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, t0 = blockIdx.x * kTM;
    const int nt = blockIdx.y / p.up, ph = blockIdx.y - nt * p.up, n0 = nt * BN;
    const int len = valid_len(p.len, b, p.T, p.len_mul);
    const int64_t row0 = (int64_t)b * p.T;

    if (t0 >= len) {                                  // nothing valid in this tile: its rows are zeros
        const int nrows = min(kTM, p.T - t0);
        for (int idx = tid; idx < nrows * (BN / 4); idx += 256) {
            const int i = idx / (BN / 4), c4 = (idx % (BN / 4)) * 4;
            *reinterpret_cast<float4*>(p.out + ((row0 + t0 + i) * p.up + ph) * p.ldo + n0 + c4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }

    int tap0, tapstep, off0, offstep, ntaps;
    if (!p.transposed) {
        tap0 = 0; tapstep = 1; ntaps = p.k; off0 = -((p.k - 1) / 2) * p.dil; offstep = p.dil;
    } else {
        const int q0 = (ph + p.pad) % p.up;
        tap0 = q0; tapstep = p.up; ntaps = (p.k - q0 + p.up - 1) / p.up; off0 = (ph + p.pad) / p.up; offstep = -1;
    }
    const int last = off0 + (ntaps - 1) * offstep;
    const int lo = min(off0, last), nwin = kTM + max(off0, last) - lo;
    const int nchunks = p.C_in / kKC, total = nchunks * ntaps;
    const int esz = BF ? 2 : 4;

    u32x4 rw[NW];
    auto gload_w = [&](int ci, int m) {
        const int tap = tap0 + m * tapstep;
#pragma unroll
        for (int q = 0; q < NW; ++q) {
            const int idx = tid + 256 * q;
            if (idx < BN * VPR) {
                const int n = idx / VPR, v = idx % VPR;
                const char* src = static_cast<const char*>(p.w) +
                                  (((int64_t)tap * p.C_out + n0 + n) * p.C_in + ci * kKC) * esz + v * 16;
                rw[q] = *reinterpret_cast<const u32x4*>(src);
            }
        }
    };
    auto swrite_w = [&](int buf) {
#pragma unroll
        for (int q = 0; q < NW; ++q) {
            const int idx = tid + 256 * q;
            if (idx < BN * VPR) *reinterpret_cast<u32x4*>(Ws + (buf * BN + idx / VPR) * PX + (idx % VPR) * 16) = rw[q];
        }
    };
    auto stage_x = [&](int ci) {
        const float* xb = p.x + row0 * p.ldx + ci * kKC;
#pragma unroll 4
        for (int idx = tid; idx < nwin * 8; idx += 256) {
            const int wr = idx >> 3, c4 = (idx & 7) * 4, ti = t0 + lo + wr;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ti >= 0 && ti < len) {
                v = *reinterpret_cast<const float4*>(xb + (int64_t)ti * p.ldx + c4);
                if (p.slope != 1.0f) {
                    v.x = lrelu(v.x, p.slope); v.y = lrelu(v.y, p.slope); v.z = lrelu(v.z, p.slope); v.w = lrelu(v.w, p.slope);
                }
            }
            if (BF) {
                u32x2 o;
                o.x = pack_bf16x2(v.x, v.y);
                o.y = pack_bf16x2(v.z, v.w);
                *reinterpret_cast<u32x2*>(Xs + wr * PX + c4 * 2) = o;
            } else {
                *reinterpret_cast<float4*>(Xs + wr * PX + c4 * 4) = v;
            }
        }
    };

    f32x16 acc[TMT][TNT];
#pragma unroll
    for (int mi = 0; mi < TMT; ++mi)
#pragma unroll
        for (int ni = 0; ni < TNT; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    gload_w(0, 0);
    swrite_w(0);
    int step = 0;
    for (int ci = 0; ci < nchunks; ++ci) {
        stage_x(ci);
        __syncthreads();
        for (int m = 0; m < ntaps; ++m, ++step) {
            const int buf = step & 1;
            if (step + 1 < total) {
                if (m + 1 < ntaps) gload_w(ci, m + 1); else gload_w(ci + 1, 0);
            }
            const int shift = off0 + m * offstep - lo;
            const char* Ab = Xs + (wm * 32 * TMT + l31 + shift) * PX + h * 16;
            const char* Bb = Ws + (buf * BN + wn * 32 * TNT + l31) * PX + h * 16;
            if (BF) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    bf16x8 a[TMT], bb[TNT];
#pragma unroll
                    for (int mi = 0; mi < TMT; ++mi) a[mi] = *reinterpret_cast<const bf16x8*>(Ab + mi * 32 * PX + ks * 32);
#pragma unroll
                    for (int ni = 0; ni < TNT; ++ni) bb[ni] = *reinterpret_cast<const bf16x8*>(Bb + ni * 32 * PX + ks * 32);
#pragma unroll
                    for (int mi = 0; mi < TMT; ++mi)
#pragma unroll
                        for (int ni = 0; ni < TNT; ++ni)
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], bb[ni], acc[mi][ni], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int kq = 0; kq < 4; ++kq) {
                    f32x4 a[TMT], bb[TNT];
#pragma unroll
                    for (int mi = 0; mi < TMT; ++mi) a[mi] = *reinterpret_cast<const f32x4*>(Ab + mi * 32 * PX + kq * 32);
#pragma unroll
                    for (int ni = 0; ni < TNT; ++ni) bb[ni] = *reinterpret_cast<const f32x4*>(Bb + ni * 32 * PX + kq * 32);
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int mi = 0; mi < TMT; ++mi)
#pragma unroll
                            for (int ni = 0; ni < TNT; ++ni)
                                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi][s], bb[ni][s], acc[mi][ni], 0, 0, 0);
                }
            }
            if (step + 1 < total) swrite_w(buf ^ 1);
            __syncthreads();
        }
    }

    // C/D fragment: column (output channel) = lane & 31, row (time) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int mi = 0; mi < TMT; ++mi)
#pragma unroll
        for (int ni = 0; ni < TNT; ++ni) {
            const int j = n0 + (wn * TNT + ni) * 32 + l31;
            const float bj = p.bias ? p.bias[j] : 0.f;
            const int ib = t0 + (wm * TMT + mi) * 32 + 4 * h;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int t = ib + (r & 3) + 8 * (r >> 2);
                if (t >= p.T) continue;
                const int64_t orow = (row0 + t) * p.up + ph;
                float v = acc[mi][ni][r] + bj;
                if (t < len) {
                    if (p.resid) v += p.resid[orow * p.ldr + j];
                    v = p.accumulate ? fmaf(p.scale, v, p.out[orow * p.ldo + j]) : p.scale * v;
                } else {
                    v = 0.f;
                }
                p.out[orow * p.ldo + j] = v;
            }
        }
}

template <bool BF, int WN, int TNT>
int32_t launch_conv(const ConvParams& p, int span, hipStream_t s) {
    constexpr int BN = 32 * WN * TNT, PX = BF ? 80 : 144;
    const size_t lds = (size_t)(2 * BN + kTM + span) * PX;
    ISPK_RESERVE_LDS((&hifigan_conv_kernel<BF, WN, TNT>), lds, "hifigan conv");
    const dim3 grid((p.T + kTM - 1) / kTM, (p.C_out / BN) * p.up, p.B);
    hipLaunchKernelGGL((hifigan_conv_kernel<BF, WN, TNT>), grid, dim3(256), lds, s, p);
    return ispk_launch_status();
}

template <bool BF>
int32_t dispatch_conv(const ConvParams& p, int span, hipStream_t s) {
    if (p.C_out % 128 == 0) return launch_conv<BF, 2, 2>(p, span, s);
    if (p.C_out % 64 == 0) return launch_conv<BF, 2, 1>(p, span, s);
    return launch_conv<BF, 1, 1>(p, span, s);
}

// what the dilated and the transposed entry share: pointers, shapes, layout
int32_t check_common(const char* what, const ConvParams& p) {
    ISPK_REQUIRE(p.x && p.w && p.out, -1, "%s: null pointer", what);
    ISPK_REQUIRE(p.B >= 1 && p.B <= 65535 && p.T >= 1 && p.len_mul >= 1, -2, "%s: bad shape B=%d T=%d len_mul=%d", what, p.B,
                 p.T, p.len_mul);
    ISPK_REQUIRE(p.C_in >= 32 && p.C_in <= kMaxC && p.C_in % 32 == 0 && p.C_out >= 32 && p.C_out <= kMaxC && p.C_out % 32 == 0,
                 -4, "%s: unsupported channel count C_in=%d C_out=%d (multiples of 32 up to %d are built)", what, p.C_in,
                 p.C_out, kMaxC);
    ISPK_REQUIRE(p.ldx >= p.C_in && p.ldo >= p.C_out && (!p.resid || p.ldr >= p.C_out), -2,
                 "%s: row strides ldx=%lld ldo=%lld ldr=%lld shorter than the rows", what, (long long)p.ldx, (long long)p.ldo,
                 (long long)p.ldr);
    ISPK_REQUIRE(p.ldx % 4 == 0 && p.ldo % 4 == 0 && ispk_aligned(p.x, 16) && ispk_aligned(p.w, 16) && ispk_aligned(p.out, 16),
                 -3, "%s: x, w and out need 16-byte aligned rows (ldx=%lld ldo=%lld)", what, (long long)p.ldx, (long long)p.ldo);
    return 0;
}

int32_t conv_entry(bool bf16, const char* what, const float* x, int64_t ldx, const void* w, const float* bias,
                   const float* resid, int64_t ldr, float* out, int64_t ldo, const int64_t* len, int32_t len_mul, int32_t B,
                   int32_t T, int32_t C_in, int32_t C_out, int32_t k, int32_t dilation, float slope, float scale,
                   int32_t accumulate, ispk_stream_t stream) {
    if (B == 0 || T == 0) return 0;
    ConvParams p{x, ldx, w, bias, resid, ldr, out, ldo, len, len_mul, B, T, C_in, C_out, k, dilation, 1, 0, 0, slope, scale,
                 accumulate != 0};
    if (int32_t rc = check_common(what, p)) return rc;
    ISPK_REQUIRE(k >= 1 && k <= 11 && k % 2 == 1 && dilation >= 1 && dilation <= 12, -4,
                 "%s: k=%d dilation=%d: odd k up to 11 and dilations 1 .. 12 are built", what, k, dilation);
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return bf16 ? dispatch_conv<true>(p, (k - 1) * dilation, s) : dispatch_conv<false>(p, (k - 1) * dilation, s);
}

int32_t upsample_entry(bool bf16, const char* what, const float* x, int64_t ldx, const void* w, const float* bias, float* out,
                       int64_t ldo, const int64_t* len, int32_t len_mul, int32_t B, int32_t T, int32_t C_in, int32_t C_out,
                       int32_t k, int32_t u, float slope, ispk_stream_t stream) {
    if (B == 0 || T == 0) return 0;
    ConvParams p{x, ldx, w, bias, nullptr, 0, out, ldo, len, len_mul, B, T, C_in, C_out, k, 1, u, (k - u) / 2, 1, slope, 1.0f, 0};
    if (int32_t rc = check_common(what, p)) return rc;
    ISPK_REQUIRE(u >= 1 && u <= 64 && k >= u && k <= 128 && (k - u) % 2 == 0, -4,
                 "%s: k=%d stride=%d: k >= stride with k - stride even is built (stride <= 64, k <= 128)", what, k, u);
    ISPK_REQUIRE((int64_t)T * u <= INT32_MAX, -2, "%s: T=%d x stride %d output rows per utterance overflow", what, T, u);
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int span = (k + u - 1) / u - 1;
    return bf16 ? dispatch_conv<true>(p, span, s) : dispatch_conv<false>(p, span, s);
}

// ------------------------------------------------------------------------------------------------------ output layer
constexpr int kPostS = 256;                       // samples per workgroup
constexpr int kPostWin = kPostS + 6;
constexpr int kPostPitch = kKC + 1;               // odd row pitch: consecutive samples read distinct banks

template <bool CLAMP>
__global__ __launch_bounds__(kPostS) void hifigan_post_kernel(const float* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              const int64_t* __restrict__ len, int len_mul,
                                                              float* __restrict__ audio, int64_t lda,
                                                              int64_t* __restrict__ audio_len, int T, int S, int C, float slope) {
    __shared__ float win[kPostWin * kPostPitch];
    const int b = blockIdx.y, tid = threadIdx.x, s0 = blockIdx.x * kPostS;
    const int n = valid_len(len, b, T, len_mul);
    if (blockIdx.x == 0 && tid == 0 && audio_len) audio_len[b] = n;
    float* arow = audio + (int64_t)b * lda;
    const int s = s0 + tid;
    if (s0 >= n) {
        if (s < S) arow[s] = 0.f;
        return;
    }
    const float* xb = x + (int64_t)b * T * ldx;
    float acc = 0.f;
    for (int c0 = 0; c0 < C; c0 += kKC) {
        __syncthreads();
        for (int idx = tid; idx < kPostWin * 8; idx += kPostS) {
            const int wr = idx >> 3, c4 = (idx & 7) * 4, ti = s0 - 3 + wr;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ti >= 0 && ti < n) {
                v = *reinterpret_cast<const float4*>(xb + (int64_t)ti * ldx + c0 + c4);
                v.x = lrelu(v.x, slope); v.y = lrelu(v.y, slope); v.z = lrelu(v.z, slope); v.w = lrelu(v.w, slope);
            }
            float* d = win + wr * kPostPitch + c4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const float* wj = w + j * C + c0;
            const float* xr = win + (tid + j) * kPostPitch;
#pragma unroll 8
            for (int c = 0; c < kKC; ++c) acc = fmaf(xr[c], wj[c], acc);
        }
    }
    if (s < S) {
        const float v = acc + bias[0];
        if (CLAMP) arow[s] = s < n ? (v < -1.f ? -1.f : v > 1.f ? 1.f : v) : 0.f;
        else arow[s] = s < n ? tanhf(v) : 0.f;
    }
}

int32_t post_entry(bool clamp, const char* what, const float* x, int64_t ldx, const float* w, const float* bias,
                   const int64_t* len, int32_t len_mul, float* audio, int64_t ld_audio, int64_t* audio_len, int32_t B, int32_t T,
                   int32_t S, int32_t C, float slope, ispk_stream_t stream) {
    if (B == 0) return 0;
    ISPK_REQUIRE(audio && ((x && w && bias) || T == 0), -1, "%s: null pointer", what);
    ISPK_REQUIRE(B >= 1 && B <= 65535 && T >= 0 && S >= T && ld_audio >= S && len_mul >= 1, -2,
                 "%s: bad shape B=%d T=%d S=%d ld_audio=%lld len_mul=%d (S >= T, ld_audio >= S)", what, B, T, S,
                 (long long)ld_audio, len_mul);
    if (S == 0 && !audio_len) return 0;
    ISPK_REQUIRE(T == 0 || (C >= 32 && C <= kMaxC && C % 32 == 0), -4,
                 "%s: unsupported channel count C=%d (multiples of 32 up to %d are built)", what, C, kMaxC);
    ISPK_REQUIRE(T == 0 || (ldx >= C && ldx % 4 == 0 && ispk_aligned(x, 16)), -3,
                 "%s: x needs 16-byte aligned rows of at least C floats (ldx=%lld)", what, (long long)ldx);
    const int nblk = S > 0 ? (S + kPostS - 1) / kPostS : 1;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (clamp)
        hipLaunchKernelGGL(hifigan_post_kernel<true>, dim3(nblk, B), dim3(kPostS), 0, s, x, ldx, w, bias, len, len_mul, audio,
                           ld_audio, audio_len, T, S, C, slope);
    else
        hipLaunchKernelGGL(hifigan_post_kernel<false>, dim3(nblk, B), dim3(kPostS), 0, s, x, ldx, w, bias, len, len_mul, audio,
                           ld_audio, audio_len, T, S, C, slope);
    return ispk_launch_status();
}

}  // namespace

extern "C" int32_t ispk_hifigan_tile_rows(void) { return kTM; }

extern "C" int32_t ispk_hifigan_conv_f32(const float* x, int64_t ldx, const float* w, const float* bias, const float* resid,
                                         int64_t ldr, float* out, int64_t ldo, const int64_t* len, int32_t len_mul, int32_t B,
                                         int32_t T, int32_t C_in, int32_t C_out, int32_t k, int32_t dilation, float slope,
                                         float scale, int32_t accumulate, ispk_stream_t stream) {
    return conv_entry(false, "ispk_hifigan_conv_f32", x, ldx, w, bias, resid, ldr, out, ldo, len, len_mul, B, T, C_in, C_out, k,
                      dilation, slope, scale, accumulate, stream);
}

extern "C" int32_t ispk_hifigan_conv_bf16(const float* x, int64_t ldx, const uint16_t* w, const float* bias, const float* resid,
                                          int64_t ldr, float* out, int64_t ldo, const int64_t* len, int32_t len_mul, int32_t B,
                                          int32_t T, int32_t C_in, int32_t C_out, int32_t k, int32_t dilation, float slope,
                                          float scale, int32_t accumulate, ispk_stream_t stream) {
    return conv_entry(true, "ispk_hifigan_conv_bf16", x, ldx, w, bias, resid, ldr, out, ldo, len, len_mul, B, T, C_in, C_out, k,
                      dilation, slope, scale, accumulate, stream);
}

extern "C" int32_t ispk_hifigan_upsample_f32(const float* x, int64_t ldx, const float* w, const float* bias, float* out,
                                             int64_t ldo, const int64_t* len, int32_t len_mul, int32_t B, int32_t T,
                                             int32_t C_in, int32_t C_out, int32_t k, int32_t stride, float slope,
                                             ispk_stream_t stream) {
    return upsample_entry(false, "ispk_hifigan_upsample_f32", x, ldx, w, bias, out, ldo, len, len_mul, B, T, C_in, C_out, k,
                          stride, slope, stream);
}

extern "C" int32_t ispk_hifigan_upsample_bf16(const float* x, int64_t ldx, const uint16_t* w, const float* bias, float* out,
                                              int64_t ldo, const int64_t* len, int32_t len_mul, int32_t B, int32_t T,
                                              int32_t C_in, int32_t C_out, int32_t k, int32_t stride, float slope,
                                              ispk_stream_t stream) {
    return upsample_entry(true, "ispk_hifigan_upsample_bf16", x, ldx, w, bias, out, ldo, len, len_mul, B, T, C_in, C_out, k,
                          stride, slope, stream);
}

extern "C" int32_t ispk_hifigan_post_f32(const float* x, int64_t ldx, const float* w, const float* bias, const int64_t* len,
                                         int32_t len_mul, float* audio, int64_t ld_audio, int64_t* audio_len, int32_t B,
                                         int32_t T, int32_t S, int32_t C, float slope, ispk_stream_t stream) {
    return post_entry(false, "ispk_hifigan_post_f32", x, ldx, w, bias, len, len_mul, audio, ld_audio, audio_len, B, T, S, C, slope,
                      stream);
}

extern "C" int32_t ispk_hifigan_post_clamp_f32(const float* x, int64_t ldx, const float* w, const float* bias,
                                               const int64_t* len, int32_t len_mul, float* audio, int64_t ld_audio,
                                               int64_t* audio_len, int32_t B, int32_t T, int32_t S, int32_t C, float slope,
                                               ispk_stream_t stream) {
    return post_entry(true, "ispk_hifigan_post_clamp_f32", x, ldx, w, bias, len, len_mul, audio, ld_audio, audio_len, B, T, S, C,
                      slope, stream);
}
