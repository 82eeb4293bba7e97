// The audio front end in front of features.hip: what tts/data/providers.py:203-212 (AudioProvider: torchaudio's Resample, then
// the mean over channels) and tts/data/dataset.py:174-221 (AcousticDataset.compute_stats with functions.py:27-32,
// remove_outliers) compute on the CPU.
//
//   resample_kernel       grid (ceil(blocks / QB), B), 256 threads.  Polyphase windowed-sinc resampling o -> n (the reduced
//                         rates): output m = q n + p is sum_t k[p][t] x[q o + first[p] + t - width] over the compact run of
//                         phase p's non-zero taps.  A workgroup owns QB whole output blocks (n outputs from o inputs each) of
//                         one utterance: it stages the tap table and the input span [q0 o - width, (q0 + QB) o + width) in
//                         LDS - the channel mean and the audio_len mask are applied while staging, float4 loads where the
//                         layout allows - and every thread accumulates its outputs in ascending tap order.
//   feature_stats_kernel  grid (B, 2), 512 threads: one workgroup per (utterance, feature).  The utterance's mel_len values go
//                         to LDS as order-preserving integer keys, a bitonic sort puts them in order (a NaN anywhere empties
//                         the utterance, as every comparison with torch.quantile's NaN is false), the two quantiles and the
//                         IQR bounds are taken in float64, and the kept values (strictly inside the bounds; pitch also > 0)
//                         are reduced in a fixed tree order in float64 to (count, mean, M2, min, max).
//   stats_fold_kernel     one workgroup: folds the [B][2][5] partials in utterance order into the running state with Chan's
//                         merge in float64.
// Every sum runs in a fixed order and there are no atomics: repeated calls and graph replays give the same bits.
#include <algorithm>

#include "chunk_grid.h"

namespace {

// ------------------------------------------------------------------------------------------------------------- resampling
constexpr int kRsThreads = 256;
constexpr int kRsMaxTable = 12288;    // floats of taps in LDS (48 KiB); the seven-rate pairs need at most 8,320
constexpr int kRsMaxPhases = 1024;
constexpr int kRsSpan = 8192;         // floats of staged input per workgroup (32 KiB)
constexpr int kRsOutTarget = 4096;    // output samples a workgroup aims for

struct ResampleArgs {
    int o, n, width, T, QB, C;
    int64_t ld_b, ld_c, ld_out;
    int S, S_out, vec;
};

__global__ __launch_bounds__(kRsThreads) void resample_kernel(const float* __restrict__ audio, const int64_t* __restrict__ audio_len,
                                                              const float* __restrict__ taps, const int32_t* __restrict__ first,
                                                              float* __restrict__ out, int64_t* __restrict__ out_len,
                                                              const ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int o = a.o, n = a.n, T = a.T;
    const int span4 = (a.QB * o + 2 * a.width + 3 + 3) / 4 * 4;       // the span plus up to 3 floats of alignment shift
    float* xs = rs_lds;                                               // [span4]
    float* ks = xs + span4;                                           // [n T]
    int* fs = reinterpret_cast<int*>(ks + n * T);                     // [n]

    int64_t len = audio_len[b];
    if (len < 0 || len > a.S) len = 0;
    const int64_t olen = (len * n + o - 1) / o;                       // ceil(n len / o) <= S_out
    if (blockIdx.x == 0 && tid == 0 && out_len) out_len[b] = olen;

    const int64_t q0 = (int64_t)blockIdx.x * a.QB;
    const int64_t m0 = q0 * n;
    const int n_out = (int)std::min<int64_t>((int64_t)a.QB * n, (int64_t)a.S_out - m0);
    float* orow = out + (int64_t)b * a.ld_out + m0;
    if (m0 >= olen) {                                                 // past the utterance: zeros, nothing read
        for (int i = tid; i < n_out; i += kRsThreads) orow[i] = 0.f;
        return;
    }

    for (int i = tid; i < n * T; i += kRsThreads) ks[i] = taps[i];
    for (int i = tid; i < n; i += kRsThreads) fs[i] = min(max(first[i], 0), 2 * a.width + o - T);   // (device data: kept inside the span)

    // xs[s] = x(g0 + s), g0 = the span's first sample rounded down to a multiple of 4; x is 0 outside [0, len)
    const int64_t start = q0 * o - a.width;
    const int64_t g0 = start >= 0 ? start / 4 * 4 : -((-start + 3) / 4 * 4);
    const int shift = (int)(start - g0);
    const float* xb = audio + (int64_t)b * a.ld_b;
    for (int s4 = tid * 4; s4 < span4; s4 += kRsThreads * 4) {
        const int64_t g = g0 + s4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (g >= 0 && g + 4 <= len && a.vec) {
            for (int c = 0; c < a.C; ++c) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(xb + c * a.ld_c + g);
                v[0] += w.x, v[1] += w.y, v[2] += w.z, v[3] += w.w;
            }
        } else {
            for (int e = 0; e < 4; ++e)
                if (g + e >= 0 && g + e < len)
                    for (int c = 0; c < a.C; ++c) v[e] += xb[c * a.ld_c + g + e];
        }
        if (a.C != 1) {
            const float fc = (float)a.C;
            for (int e = 0; e < 4; ++e) v[e] = v[e] / fc;
        }
        f32x4 w;
        w.x = v[0], w.y = v[1], w.z = v[2], w.w = v[3];
        *reinterpret_cast<f32x4*>(xs + s4) = w;
    }
    __syncthreads();

    for (int i = tid; i < n_out; i += kRsThreads) {
        float acc = 0.f;
        if (m0 + i < olen) {
            const int q = i / n, p = i - q * n;
            const float* k = ks + p * T;
            const float* x = xs + shift + q * o + fs[p];
            for (int t = 0; t < T; ++t) acc = fmaf(k[t], x[t], acc);
        }
        orow[i] = acc;
    }
}

// ------------------------------------------------------------------------------------------------------------- statistics
constexpr int kStThreads = 512;
constexpr int kStMaxM = 4096;

__device__ __forceinline__ uint32_t sort_key(float v) {
    if (v != v) return 0xffffffffu;                                  // NaNs last
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(kStThreads) void feature_stats_kernel(const float* __restrict__ pitch, int64_t ld_pitch,
                                                                   const float* __restrict__ energy, int64_t ld_energy,
                                                                   const int64_t* __restrict__ mel_len, double* __restrict__ partial,
                                                                   int M) {
    __shared__ uint32_t keys[kStMaxM];
    __shared__ double red[kStThreads];
    __shared__ float fred[2 * kStThreads];
    const int tid = threadIdx.x, b = blockIdx.x, f = blockIdx.y;
    const float* row = f == 0 ? pitch + (int64_t)b * ld_pitch : energy + (int64_t)b * ld_energy;
    int64_t len = mel_len[b];
    if (len < 0 || len > M) len = 0;
    const int nv = (int)len;
    int N = 2;
    while (N < nv) N <<= 1;
    int nan_here = 0;
    for (int i = tid; i < N; i += kStThreads) {
        uint32_t k = 0xffffffffu;
        if (i < nv) {
            const float v = row[i];
            nan_here |= v != v;
            k = sort_key(v);
        }
        keys[i] = k;
    }
    const int has_nan = __syncthreads_or(nan_here);
    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < N / 2; t += kStThreads) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint32_t x = keys[lo], y = keys[hi];
                if ((x > y) == up) {
                    keys[lo] = y;
                    keys[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    double lower = 0.0, upper = 0.0;
    const bool live = nv >= 1 && !has_nan;
    if (live) {
#pragma clang fp contract(off)   // the fences as written (no fused multiply-add): the same roundings as a host float64 restatement
        // torch.quantile's "linear": position q (n - 1), the two neighbours interpolated.  4 q is an integer, so the
        // position and its fraction are exact.
        const int r25 = nv - 1, r75 = 3 * (nv - 1);
        const double a25 = key_value(keys[r25 / 4]), b25 = key_value(keys[min(r25 / 4 + 1, nv - 1)]);
        const double a75 = key_value(keys[r75 / 4]), b75 = key_value(keys[min(r75 / 4 + 1, nv - 1)]);
        const double p25 = a25 + 0.25 * (r25 % 4) * (b25 - a25), p75 = a75 + 0.25 * (r75 % 4) * (b75 - a75);
        lower = p25 - 1.5 * (p75 - p25);
        upper = p75 + 1.5 * (p75 - p25);
    }
    double cnt = 0.0, sum = 0.0;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    if (live)
        for (int i = tid; i < nv; i += kStThreads) {
            const float v = key_value(keys[i]);
            if ((double)v > lower && (double)v < upper && (f != 0 || v > 0.f)) {
                cnt += 1.0;
                sum += (double)v;
                mn = fminf(mn, v);
                mx = fmaxf(mx, v);
            }
        }
    const double count = block_sum<kStThreads>(cnt, tid, red);
    const double total = block_sum<kStThreads>(sum, tid, red);
    const double mean = count > 0.0 ? total / count : 0.0;
    double m2 = 0.0;
    if (live)
        for (int i = tid; i < nv; i += kStThreads) {
            const float v = key_value(keys[i]);
            if ((double)v > lower && (double)v < upper && (f != 0 || v > 0.f)) m2 += ((double)v - mean) * ((double)v - mean);
        }
    const double M2 = block_sum<kStThreads>(m2, tid, red);
    fred[tid] = mn;
    fred[kStThreads + tid] = mx;
    __syncthreads();
    for (int s = kStThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            fred[tid] = fminf(fred[tid], fred[tid + s]);
            fred[kStThreads + tid] = fmaxf(fred[kStThreads + tid], fred[kStThreads + tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* p = partial + ((int64_t)b * 2 + f) * 5;
        p[0] = count, p[1] = mean, p[2] = M2, p[3] = (double)fred[0], p[4] = (double)fred[kStThreads];
    }
}

// state [2][5] = (count, mean, M2, min, max) per feature; thread f folds feature f's partials in utterance order.  The
// partials pass through LDS, kFoldChunk utterances at a time, so that the serial fold does not wait on global memory.
constexpr int kFoldThreads = 256;
constexpr int kFoldChunk = 256;

__global__ __launch_bounds__(kFoldThreads) void stats_fold_kernel(const double* __restrict__ partial, double* __restrict__ state,
                                                                  int B, int reset) {
    __shared__ double buf[kFoldChunk * 10];
    const int f = threadIdx.x;
    double n = 0.0, mean = 0.0, M2 = 0.0, mn = (double)__builtin_inff(), mx = -(double)__builtin_inff();
    if (f < 2 && !reset) {
        const double* s = state + f * 5;
        n = s[0], mean = s[1], M2 = s[2], mn = s[3], mx = s[4];
    }
    for (int b0 = 0; b0 < B; b0 += kFoldChunk) {
        const int nb = min(kFoldChunk, B - b0);
        for (int i = threadIdx.x; i < nb * 10; i += kFoldThreads) buf[i] = partial[(int64_t)b0 * 10 + i];
        __syncthreads();
        if (f < 2)
            for (int b = 0; b < nb; ++b) {
                const double* p = buf + (b * 2 + f) * 5;
                const double cnt = p[0];
                if (cnt > 0.0) {
                    const double tot = n + cnt, d = p[1] - mean;
                    mean += d * (cnt / tot);
                    M2 += p[2] + d * d * (n * cnt / tot);
                    n = tot;
                    mn = fmin(mn, p[3]);
                    mx = fmax(mx, p[4]);
                }
            }
        __syncthreads();
    }
    if (f < 2) {
        double* s = state + f * 5;
        s[0] = n, s[1] = mean, s[2] = M2, s[3] = mn, s[4] = mx;
    }
}

}  // namespace

extern "C" int32_t ispk_resample_f32(const float* audio, int64_t ld_b, int64_t ld_c, const int64_t* audio_len, const float* taps,
                                     int64_t tap_floats, const int32_t* first, float* out, int64_t ld_out, int64_t* out_len,
                                     int32_t B, int32_t C, int32_t S, int32_t S_out, int32_t orig, int32_t dest, int32_t width,
                                     int32_t T, ispk_stream_t stream) {
    ISPK_REQUIRE(audio && audio_len && taps && first && out, ISPK_E_NULL, "ispk_resample_f32: null pointer");
    ISPK_REQUIRE(orig >= 1 && dest >= 1 && dest <= kRsMaxPhases && width >= 0 && T >= 1 && T <= 2 * width + orig, ISPK_E_SHAPE,
                 "ispk_resample_f32: bad filter o=%d n=%d width=%d T=%d (1 <= n <= %d, 1 <= T <= 2 width + o)", orig, dest, width,
                 T, kRsMaxPhases);
    ISPK_REQUIRE((int64_t)dest * T <= kRsMaxTable && tap_floats == (int64_t)dest * T, ISPK_E_UNSUPPORTED,
                 "ispk_resample_f32: a tap table of %lld floats (n T = %lld) is not supported: at most %d", (long long)tap_floats,
                 (long long)dest * T, kRsMaxTable);
    ISPK_REQUIRE(orig + 2 * width <= kRsSpan - 8, ISPK_E_UNSUPPORTED,
                 "ispk_resample_f32: one output block spans %d input samples, at most %d are staged", orig + 2 * width, kRsSpan - 8);
    ISPK_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && C <= 64 && S >= 0, ISPK_E_SHAPE, "ispk_resample_f32: bad shape B=%d C=%d S=%d", B,
                 C, S);
    const int64_t want = ((int64_t)S * dest + orig - 1) / orig;
    ISPK_REQUIRE(S_out == want && want <= 0x7fffffff, ISPK_E_SHAPE, "ispk_resample_f32: S_out=%d, ceil(n S / o) = %lld", S_out,
                 (long long)want);
    ISPK_REQUIRE(ld_out >= S_out && (C == 1 || ld_c >= S) && ld_b >= (C == 1 ? (int64_t)S : ld_c), ISPK_E_SHAPE,
                 "ispk_resample_f32: strides ld_b=%lld ld_c=%lld ld_out=%lld too small for S=%d S_out=%d", (long long)ld_b,
                 (long long)ld_c, (long long)ld_out, S, S_out);
    if (S_out == 0) return 0;
    ResampleArgs a;
    a.o = orig, a.n = dest, a.width = width, a.T = T, a.C = C;
    a.QB = std::max(1, std::min(kRsOutTarget / dest, (kRsSpan - 8 - 2 * width) / orig));
    a.ld_b = ld_b, a.ld_c = C == 1 ? 0 : ld_c, a.ld_out = ld_out;
    a.S = S, a.S_out = S_out;
    a.vec = ld_b % 4 == 0 && (C == 1 || ld_c % 4 == 0) && ispk_aligned(audio, 16);
    const int span4 = (a.QB * orig + 2 * width + 6) / 4 * 4;
    const size_t lds = sizeof(float) * ((size_t)span4 + (size_t)dest * T) + sizeof(int) * dest;
    ISPK_RESERVE_LDS(resample_kernel, lds, "ispk_resample_f32");
    const int64_t blocks = ((int64_t)S_out + dest - 1) / dest;
    const int64_t gx = (blocks + a.QB - 1) / a.QB;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)gx, B), dim3(kRsThreads), lds, reinterpret_cast<hipStream_t>(stream), audio,
                       audio_len, taps, first, out, out_len, a);
    return ispk_launch_status();
}

extern "C" int32_t ispk_feature_stats_f64(const float* pitch, int64_t ld_pitch, const float* energy, int64_t ld_energy,
                                          const int64_t* mel_len, double* partial, double* state, int32_t B, int32_t M,
                                          int32_t reset, ispk_stream_t stream) {
    ISPK_REQUIRE(state, ISPK_E_NULL, "ispk_feature_stats_f64: null state");
    ISPK_REQUIRE(B == 0 || (pitch && energy && mel_len && partial), ISPK_E_NULL, "ispk_feature_stats_f64: null pointer");
    ISPK_REQUIRE(B >= 0 && B <= 65535 && M >= 0 && M <= kStMaxM, ISPK_E_SHAPE,
                 "ispk_feature_stats_f64: bad shape B=%d M=%d (M <= %d)", B, M, kStMaxM);
    ISPK_REQUIRE(B == 0 || (ld_pitch >= M && ld_energy >= M), ISPK_E_SHAPE, "ispk_feature_stats_f64: row strides %lld, %lld below M=%d",
                 (long long)ld_pitch, (long long)ld_energy, M);
    if (B == 0 && !reset) return 0;
    if (B > 0)
        hipLaunchKernelGGL(feature_stats_kernel, dim3(B, 2), dim3(kStThreads), 0, reinterpret_cast<hipStream_t>(stream), pitch,
                           ld_pitch, energy, ld_energy, mel_len, partial, M);
    hipLaunchKernelGGL(stats_fold_kernel, dim3(1), dim3(kFoldThreads), 0, reinterpret_cast<hipStream_t>(stream), partial, state, B, reset);
    return ispk_launch_status();
}
