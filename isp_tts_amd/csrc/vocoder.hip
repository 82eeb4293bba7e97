// Vocos vocoder (mel variant: VocosBackbone + ISTFTHead with padding="same", n_fft 1024, hop 256): the three kernels that are
// not a GEMM or a LayerNorm.  The rest of the network runs through ispk_gemm_{f32,bf16} and ispk_layernorm_f32[_bf16]
// (isp_tts_amd/vocoder.py):
//
//   vocoder_unfold_kernel  grid (ceil(T / 32), B), 256 threads.  The embedding Conv1d(n_mels -> dim, 7, padding 3) as GEMM
//                          rows: row b*T + t, column j*C + c = mel[b][c][t + j - 3] (tap-major), zero outside [0, len_b) and
//                          in the K padding; rows at or past len_b all zero.  A workgroup stages mel[b][:, t0 - 3, t0 + 35)
//                          once in LDS (frame-contiguous global reads for a [B][C][T] mel), then writes its 32 rows along
//                          K.  Also writes the byte row mask (t < len_b) the LayerNorms and the residual GEMMs take.
//   dwconv7_ln_kernel<NC>  grid (ceil(T / 32), B), 256 threads = 4 waves, each wave a run of 8 consecutive frames of one
//                          utterance; lane l holds channels l + 64 i, i < NC = dim / 64.  The depthwise Conv1d(dim, 7,
//                          padding 3, groups dim) + bias, then LayerNorm(dim) (two-pass mean / variance, wave butterflies),
//                          out fp32 or bf16; rows at or past len_b written as zeros.  The 7 taps slide through REGISTERS:
//                          a wave keeps the 7 input rows of its current frame and loads one new row per frame (the next
//                          one prefetched a frame ahead), so each residual row is read once per wave plus a 6-row halo per
//                          8-frame run.  The halo rows are the neighbouring waves' rows, read at about the same time, so
//                          they come from L2: staging in LDS would save only those L2 reads, and would cost a barrier and
//                          up to 4 KB of LDS per frame at dim 1024.  The bound is HBM: read the fp32 residual once, write
//                          the normalised rows once.
//   istft_head_kernel      the 1024 / 256 tile of stft_tile.h (geometry, LDS, bank and bit-reproducibility notes are there)
//                          with the framing of padding="same": 384 samples trimmed in front, so the tile at frame s0
//                          transforms the up-to-20 frames s0 - 2 .. s0 + 17 of the utterance.  Per frame, the prologue
//                          exp, clip at 100 (a compare that keeps NaN, as torch.clip), sincos (range-reduced libm sincosf:
//                          p is an unbounded Linear output), x 1/1024 (irfft's norm) for the bin pair (k, 512 - k), packed
//                          straight into the inverse's half-length spectrum (pack_pairs); the inverse FFT into the frame's
//                          slot; then the overlap-add over the frames within [0, len_b).  Samples at or past len_b * 256 are
//                          written as 0.
// Every sum runs in a fixed order and there are no atomics: repeated calls and graph replays give the same bits.  A device
// mel_len outside [0, T] is treated as 0 by all three kernels (zero rows, audio_len 0, nothing read).
//
// gfx950 resources (hipcc -Rpass-analysis=kernel-resource-usage, no scratch in any):
//   vocoder_unfold_kernel<f32|f16, f32|bf16>   14 VGPRs, LDS 19,968 B static
//   dwconv7_ln_kernel<NC, f32|bf16>            no LDS; 131 VGPRs at dim 384 (occupancy 3), 176 at dim 512 (2), 256 + 81
//                                              AGPRs at dim 1024 (1)
//   istft_head_kernel                           72 VGPRs, LDS 110,592 B dynamic (one workgroup per CU)
#include <hip/hip_fp16.h>

#include "common.h"
#include "stft_tile.h"

namespace {

constexpr int kPad = (kNfft - kHop) / 2;          // 384: Vocos ISTFT padding="same"
constexpr int kMaxMels = 128;

// ------------------------------------------------------------------------------------------------------------ unfold
constexpr int kUfFrames = 32;
constexpr int kUfCols = kUfFrames + 6;
constexpr int kUfPitch = kUfCols + 1;             // odd row pitch: channel-strided LDS reads fall on distinct banks

template <bool kInF16, bool kOutBf16>
__global__ void __launch_bounds__(256) vocoder_unfold_kernel(const void* __restrict__ mel, int64_t sb, int64_t sc, int64_t st,
                                                            const int64_t* __restrict__ mel_len, void* __restrict__ rows,
                                                            int64_t ldr, uint8_t* __restrict__ row_mask, int C, int T, int K) {
    __shared__ float tile[kMaxMels * kUfPitch];
    const int b = blockIdx.y, t0 = blockIdx.x * kUfFrames, tid = threadIdx.x;
    const int len = valid_len(mel_len, b, T);
    for (int i = tid; i < C * kUfCols; i += 256) {
        const int c = i / kUfCols, j = i % kUfCols, t = t0 - 3 + j;
        float v = 0.f;
        if (t >= 0 && t < len) {
            const int64_t off = (int64_t)b * sb + (int64_t)c * sc + (int64_t)t * st;
            v = kInF16 ? __half2float(reinterpret_cast<const __half*>(mel)[off]) : reinterpret_cast<const float*>(mel)[off];
        }
        tile[c * kUfPitch + j] = v;
    }
    __syncthreads();
    const int nrows = min(kUfFrames, T - t0), kc = 7 * C;
    for (int r = 0; r < nrows; ++r) {
        const int t = t0 + r;
        const bool ok = t < len;
        const int64_t row = (int64_t)b * T + t;
        for (int k = tid; k < K; k += 256) {
            const int j = k / C, c = k - j * C;
            const float v = (ok && k < kc) ? tile[c * kUfPitch + r + j] : 0.f;
            if (kOutBf16)
                reinterpret_cast<uint16_t*>(rows)[row * ldr + k] = f32_to_bf16(v);
            else
                reinterpret_cast<float*>(rows)[row * ldr + k] = v;
        }
        if (row_mask && tid == 0) row_mask[row] = ok ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------------- dwconv + LN
constexpr int kDwFrames = 8;                      // frames per wave
constexpr int kDwWaves = 4;

template <int NC, bool kOutBf16>
__global__ void __launch_bounds__(256) dwconv7_ln_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                         const float* __restrict__ bias, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps,
                                                         const int64_t* __restrict__ mel_len, void* __restrict__ y,
                                                         int64_t ldy, int T) {
    constexpr int D = NC * kWave;
    const int b = blockIdx.y, lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
    const int tb = (blockIdx.x * kDwWaves + wv) * kDwFrames;
    if (tb >= T) return;
    const int len = valid_len(mel_len, b, T);
    const float* xb = x + (int64_t)b * T * ldx;
    float wt[NC][7], bs[NC], g[NC], be[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + kWave * i;
#pragma unroll
        for (int j = 0; j < 7; ++j) wt[i][j] = w[c * 7 + j];
        bs[i] = bias[c];
        g[i] = gamma[c];
        be[i] = beta[c];
    }
    auto load = [&](float (&dst)[NC], int t) {
        const bool ok = t >= 0 && t < len;
#pragma unroll
        for (int i = 0; i < NC; ++i) dst[i] = ok ? xb[(int64_t)t * ldx + lane + kWave * i] : 0.f;
    };
    float win[7][NC], nxt[NC];
#pragma unroll
    for (int j = 0; j < 6; ++j) load(win[j], tb - 3 + j);
    load(nxt, tb + 3);
    const int nf = min(kDwFrames, T - tb);
    for (int f = 0; f < nf; ++f) {
        const int t = tb + f;
#pragma unroll
        for (int i = 0; i < NC; ++i) win[6][i] = nxt[i];
        load(nxt, t + 4);
        const int64_t row = (int64_t)b * T + t;
        float v[NC];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            float a = bs[i];
#pragma unroll
            for (int j = 0; j < 7; ++j) a = fmaf(wt[i][j], win[j][i], a);
            v[i] = a;
            s += a;
        }
        const float mean = wave_sum(s) * (1.0f / D);
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const float d = v[i] - mean;
            ss = fmaf(d, d, ss);
        }
        const float rstd = 1.0f / sqrtf(wave_sum(ss) * (1.0f / D) + eps);
        const bool ok = t < len;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const float o = ok ? fmaf((v[i] - mean) * rstd, g[i], be[i]) : 0.f;
            if (kOutBf16)
                reinterpret_cast<uint16_t*>(y)[row * ldy + lane + kWave * i] = f32_to_bf16(o);
            else
                reinterpret_cast<float*>(y)[row * ldy + lane + kWave * i] = o;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int i = 0; i < NC; ++i) win[j][i] = win[j + 1][i];
    }
}

template <int NC>
int32_t launch_dwconv(bool bf16, const float* x, int64_t ldx, const float* w, const float* bias, const float* gamma,
                      const float* beta, float eps, const int64_t* mel_len, void* y, int64_t ldy, int B, int T, hipStream_t s) {
    const dim3 grid((T + kDwWaves * kDwFrames - 1) / (kDwWaves * kDwFrames), B);
    if (bf16)
        hipLaunchKernelGGL((dwconv7_ln_kernel<NC, true>), grid, dim3(256), 0, s, x, ldx, w, bias, gamma, beta, eps, mel_len, y,
                           ldy, T);
    else
        hipLaunchKernelGGL((dwconv7_ln_kernel<NC, false>), grid, dim3(256), 0, s, x, ldx, w, bias, gamma, beta, eps, mel_len,
                           y, ldy, T);
    return ispk_launch_status();
}

// -------------------------------------------------------------------------------------------------------- ISTFT head
// X_k / 1024 = clip(exp(lm), max=100) (cos p + i sin p) / 1024
__device__ __forceinline__ cf head_bin(const float* hrow, int k) {
    float mag = expf(hrow[k]);
    mag = mag > 100.f ? 100.f : mag;               // torch.clip: NaN stays NaN (not fminf)
    float sn, cs;
    sincosf(hrow[kBins + k], &sn, &cs);
    mag *= 1.0f / kNfft;
    return make_float2(mag * cs, mag * sn);
}

__global__ void __launch_bounds__(kThreads) istft_head_kernel(const float* __restrict__ h, int64_t ldh,
                                                              const int64_t* __restrict__ mel_len,
                                                              const float* __restrict__ tables, float* __restrict__ audio,
                                                              int64_t lda, int64_t* __restrict__ audio_len, int T, int S) {
    extern __shared__ float4 lds_raw[];
    const TileLds tile = carve_tile(lds_raw);

    const int b = blockIdx.y, tid = threadIdx.x, g = tid / kGT, lt = tid % kGT;
    const int s0 = blockIdx.x * kSegs;
    const int Tb = valid_len(mel_len, b, T);
    if (blockIdx.x == 0 && tid == 0 && audio_len) audio_len[b] = (int64_t)Tb * kHop;
    const int nseg = max(0, min(kSegs, Tb - s0));
    float* arow = audio + (int64_t)b * lda;
    const int m0 = s0 * kHop, m1 = min(S, m0 + kTile), mv = m0 + nseg * kHop;   // [m0, mv): the tile's samples of the utterance

    if (nseg > 0) {
        const int f_lo = max(0, s0 - 2), f_hi = min(Tb, s0 + nseg + 2), nf = f_hi - f_lo;
        load_tables(tile.tw, tile.win, tables, tid);
        __syncthreads();
        cf* Z = tile.ping + g * kHalf;
        for (int r = 0; r * kGroups < nf; ++r) {
            const int fs = r * kGroups + g;                           // slot; fs >= nf: transformed, never read
            if (fs < nf) {
                const float* hrow = h + ((int64_t)b * T + f_lo + fs) * ldh;
                pack_pairs(Z, lt, tile.tw, [&](int k, int m, cf& xk, cf& xm) {
                    xk = head_bin(hrow, k);
                    xm = k == 256 ? xk : head_bin(hrow, m);
                });
            } else {
                clear_frame(Z, lt);
            }
            __syncthreads();
            fft<true, kGT, kTw>(Z, reinterpret_cast<cf*>(tile.frames + fs * kNfft), kHalf, lt, tile.tw);
        }
        overlap_add(arow, tile.frames, tile.win, m0, mv, kPad, f_lo, Tb, tid);
    }
    for (int m = mv + tid; m < m1; m += kThreads) arow[m] = 0.f;
}

}  // namespace

extern "C" int32_t ispk_vocoder_unfold(const void* mel, int32_t mel_f16, int64_t sb, int64_t sc, int64_t st,
                                       const int64_t* mel_len, void* rows, int32_t rows_bf16, int64_t ldr, uint8_t* row_mask,
                                       int32_t B, int32_t C, int32_t T, int32_t K, ispk_stream_t stream) {
    if (B == 0 || T == 0) return 0;
    ISPK_REQUIRE(mel && rows, -1, "ispk_vocoder_unfold: null pointer");
    ISPK_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && C >= 1 && C <= kMaxMels, -2,
                 "ispk_vocoder_unfold: bad shape B=%d C=%d T=%d (1 <= C <= %d)", B, C, T, kMaxMels);
    ISPK_REQUIRE(K >= 7 * C && K % 8 == 0 && ldr >= K, -2, "ispk_vocoder_unfold: K=%d ldr=%lld: need K >= 7 C = %d, K %% 8 == 0, "
                 "ldr >= K", K, (long long)ldr, 7 * C);
    const dim3 grid((T + kUfFrames - 1) / kUfFrames, B);
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define ISPK_UF(F16, BF16) \
    hipLaunchKernelGGL((vocoder_unfold_kernel<F16, BF16>), grid, dim3(256), 0, s, mel, sb, sc, st, mel_len, rows, ldr, row_mask, C, T, K)
    if (mel_f16) {
        if (rows_bf16) ISPK_UF(true, true); else ISPK_UF(true, false);
    } else {
        if (rows_bf16) ISPK_UF(false, true); else ISPK_UF(false, false);
    }
#undef ISPK_UF
    return ispk_launch_status();
}

extern "C" int32_t ispk_dwconv7_ln_f32(const float* x, int64_t ldx, const float* w, const float* bias, const float* gamma,
                                       const float* beta, float eps, const int64_t* mel_len, void* y, int32_t y_bf16,
                                       int64_t ldy, int32_t B, int32_t T, int32_t D, ispk_stream_t stream) {
    if (B == 0 || T == 0) return 0;
    ISPK_REQUIRE(x && w && bias && gamma && beta && y, -1, "ispk_dwconv7_ln_f32: null pointer");
    ISPK_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && D % 64 == 0 && D >= 64 && D <= 1024 && ldx >= D && ldy >= D, -2,
                 "ispk_dwconv7_ln_f32: bad shape B=%d T=%d D=%d ldx=%lld ldy=%lld (D %% 64 == 0, D <= 1024)", B, T, D,
                 (long long)ldx, (long long)ldy);
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool bf = y_bf16 != 0;
    switch (D / 64) {
#define ISPK_DW(N) \
    case N: return launch_dwconv<N>(bf, x, ldx, w, bias, gamma, beta, eps, mel_len, y, ldy, B, T, s);
        ISPK_DW(1) ISPK_DW(2) ISPK_DW(3) ISPK_DW(4) ISPK_DW(5) ISPK_DW(6) ISPK_DW(7) ISPK_DW(8)
        ISPK_DW(9) ISPK_DW(10) ISPK_DW(11) ISPK_DW(12) ISPK_DW(13) ISPK_DW(14) ISPK_DW(15) ISPK_DW(16)
#undef ISPK_DW
    }
    return -2;
}

extern "C" int32_t ispk_istft_head_f32(const float* h, int64_t ldh, const int64_t* mel_len, const float* tables,
                                       int64_t table_floats, float* audio, int64_t ld_audio, int64_t* audio_len, int32_t B,
                                       int32_t T, int32_t S, ispk_stream_t stream) {
    if (B == 0) return 0;
    ISPK_REQUIRE(audio && tables && (h || T == 0), -1, "ispk_istft_head_f32: null pointer");
    ISPK_REQUIRE(table_floats >= kTableFloats, -2, "ispk_istft_head_f32: tables hold %lld floats, need %d", (long long)table_floats,
                 kTableFloats);
    ISPK_REQUIRE(B >= 1 && B <= 65535 && T >= 0 && ldh >= 2 * kBins && S >= 0 && (int64_t)S >= (int64_t)T * kHop &&
                 ld_audio >= S, -2, "ispk_istft_head_f32: bad shape B=%d T=%d S=%d ldh=%lld ld_audio=%lld (ldh >= 1026, "
                 "S >= 256 T, ld_audio >= S)", B, T, S, (long long)ldh, (long long)ld_audio);
    ISPK_RESERVE_LDS(istft_head_kernel, kLds, "ispk_istft_head_f32");
    const int nblk = S > 0 ? (S + kTile - 1) / kTile : 1;
    hipLaunchKernelGGL(istft_head_kernel, dim3(nblk, B), dim3(kThreads), kLds, reinterpret_cast<hipStream_t>(stream), h,
                       ldh, mel_len, tables, audio, ld_audio, audio_len, T, S);
    return ispk_launch_status();
}
