// Hard durations (FlowTemporalAdaptor with soft_duration off, the reference's constructor default: the FastPitch arrangement).
//   ispk_hard_regulate_f32      LengthRegulator without an alignment (temporal_adaptor.py:422-436): every token row repeated
//                               reps = (float(dur) + 0.5).long() times - a row gather, bit-exact
//   ispk_hard_regulate_bwd_f32  its backward: d x[b][l] = the sum of the token's d out rows, in frame order, one owner per value
//   ispk_hard_average_f32       TemporalAverager without an alignment (:451-465) for pitch and energy, plus log1p(duration), in
//                               ispk_soft_average_f32's layout
// All three need the running sums of one utterance's repeats (L <= 512, MAS's limit): every workgroup scans them into LDS for
// itself - 100 .. 512 integers, cheaper than a launch of its own with a workspace.
#include "common.h"
#include "dec_len.h"

namespace {

constexpr int kHdMaxL = 512;
constexpr int kHdThreads = 256;
constexpr int kHdRows = 32;                 // frames per workgroup of the regulator: 8 per wave
// (kHdRepMax, hd_reps: dec_len.h)

// cum[l] = reps[0] + .. + reps[l] (inclusive), cut at INT32_MAX for the frame searches; returns the full sum.  256 threads,
// 256 tokens per trip: a shuffle scan inside each wave, the four wave totals through LDS, the carry in a register.
template <bool kRound>
__device__ __forceinline__ int64_t hd_scan(const float* __restrict__ dur_f, const int64_t* __restrict__ dur_i, int64_t row, int L,
                                           int* __restrict__ cum, int64_t* __restrict__ wave_tot) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int64_t carry = 0;
    for (int base = 0; base < L; base += kHdThreads) {
        const int l = base + t;
        int64_t v = l < L ? hd_reps<kRound>(dur_f, dur_i, row + l) : 0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t up = __shfl_up(v, off, 64);
            if (lane >= off) v += up;
        }
        if (lane == 63) wave_tot[w] = v;
        __syncthreads();
        int64_t before = carry;
        for (int k = 0; k < w; ++k) before += wave_tot[k];
        carry += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        v += before;
        if (l < L) cum[l] = (int)(v > INT32_MAX ? INT32_MAX : v);
        __syncthreads();                                                   // wave_tot is rewritten by the next trip
    }
    return carry;
}

// the token that owns frame y < cum[L - 1]: the first l with cum[l] > y (an upper bound: tokens without frames are skipped)
__device__ __forceinline__ int hd_token(const int* __restrict__ cum, int L, int y) {
    int lo = 0, hi = L - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] <= y) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// grid (ceil(frames / 32), B).  A wave copies one row per trip with 16-byte loads and stores: D / 4 = 64 or 96 float4, lane
// and lane + 64; four rows' loads are issued before the first store.
__global__ __launch_bounds__(kHdThreads) void hard_regulate_kernel(const float* __restrict__ dur_f, const int64_t* __restrict__ dur_i,
                                                                   const float* __restrict__ x, int64_t ldx, float* __restrict__ out,
                                                                   int64_t* __restrict__ dec_len, uint8_t* __restrict__ dec_mask,
                                                                   int frames, int L, int D, int max_len) {
    __shared__ int cum[kHdMaxL];
    __shared__ int64_t wave_tot[4];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
    int64_t total = hd_scan<true>(dur_f, dur_i, (int64_t)b * L, L, cum, wave_tot);
    if (max_len >= 0 && total > max_len) total = max_len;
    const int valid = (int)(total < frames ? total : frames);             // rows below it have a token
    const int y0 = blockIdx.x * kHdRows;
    if (blockIdx.x == 0 && t == 0) dec_len[b] = total;
    if (dec_mask && t < kHdRows && y0 + t < frames) dec_mask[(int64_t)b * frames + y0 + t] = (y0 + t) < total ? 1 : 0;
    const int d4 = D >> 2;
    const bool second = lane + 64 < d4;
    const float* xb = x + (int64_t)b * L * ldx;
    float* ob = out + (int64_t)b * frames * D;
#pragma unroll
    for (int g = 0; g < kHdRows / 16; ++g) {
        f32x4 v0[4], v1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int y = y0 + (g * 4 + u) * 4 + w;
            v0[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            v1[u] = v0[u];
            if (y < valid) {                                               // wave-uniform
                const f32x4* src = reinterpret_cast<const f32x4*>(xb + (int64_t)hd_token(cum, L, y) * ldx);
                v0[u] = src[lane];
                if (second) v1[u] = src[lane + 64];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int y = y0 + (g * 4 + u) * 4 + w;
            if (y < frames) {
                f32x4* dst = reinterpret_cast<f32x4*>(ob + (int64_t)y * D);
                dst[lane] = v0[u];
                if (second) dst[lane + 64] = v1[u];
            }
        }
    }
}

// grid (ceil(L / 4), B): a wave owns one token and adds its frames' gradient rows one after the other in fp32 (frame order, no
// atomics: the same bits every run); four rows' loads in flight.  Rows at or above min(dec_len, rows) belong to nobody.
__global__ __launch_bounds__(kHdThreads) void hard_regulate_bwd_kernel(const float* __restrict__ dur_f, const int64_t* __restrict__ dur_i,
                                                                       const float* __restrict__ d_out, float* __restrict__ d_x,
                                                                       int rows, int L, int D, int max_len) {
    __shared__ int cum[kHdMaxL];
    __shared__ int64_t wave_tot[4];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
    int64_t total = hd_scan<true>(dur_f, dur_i, (int64_t)b * L, L, cum, wave_tot);
    if (max_len >= 0 && total > max_len) total = max_len;
    const int valid = (int)(total < rows ? total : rows);
    const int l = blockIdx.x * 4 + w;
    if (l >= L) return;
    const int begin = min(l ? cum[l - 1] : 0, valid), end = min(cum[l], valid);
    const int d4 = D >> 2;
    const bool second = lane + 64 < d4;
    const float* gb = d_out + (int64_t)b * rows * D;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
    int y = begin;
    for (; y + 4 <= end; y += 4) {
        f32x4 v0[4], v1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const f32x4* src = reinterpret_cast<const f32x4*>(gb + (int64_t)(y + u) * D);
            v0[u] = src[lane];
            v1[u] = second ? src[lane + 64] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a0 += v0[u];
            a1 += v1[u];
        }
    }
    for (; y < end; ++y) {
        const f32x4* src = reinterpret_cast<const f32x4*>(gb + (int64_t)y * D);
        a0 += src[lane];
        if (second) a1 += src[lane + 64];
    }
    f32x4* dst = reinterpret_cast<f32x4*>(d_x + ((int64_t)b * L + l) * D);
    dst[lane] = a0;
    if (second) dst[lane + 64] = a1;
}

// grid (ceil(L / 4), B): a wave owns one token; its lanes stride the token's frames (ends cut at M), then a butterfly over
// the wave - a direct sum per segment, not the reference's difference of two fp32 running sums.
__global__ __launch_bounds__(kHdThreads) void hard_average_kernel(const float* __restrict__ pitch, const float* __restrict__ energy,
                                                                  const int64_t* __restrict__ dur, const int64_t* __restrict__ text_len,
                                                                  float* __restrict__ feats, int M, int L) {
    __shared__ int cum[kHdMaxL];
    __shared__ int64_t wave_tot[4];
    const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    hd_scan<false>(nullptr, dur, (int64_t)b * L, L, cum, wave_tot);
    const int l = blockIdx.x * 4 + w;
    if (l >= L) return;
    const int begin = min(l ? cum[l - 1] : 0, M), end = min(cum[l], M);
    const float* pb = pitch + (int64_t)b * M;
    const float* eb = energy + (int64_t)b * M;
    float sp = 0.f, se = 0.f;
    int np = 0, ne = 0;
    for (int y = begin + lane; y < end; y += 64) {
        const float p = pb[y], e = eb[y];
        sp += p;
        se += e;
        np += p != 0.0f;
        ne += e != 0.0f;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sp += __shfl_xor(sp, off, 64);
        se += __shfl_xor(se, off, 64);
        np += __shfl_xor(np, off, 64);
        ne += __shfl_xor(ne, off, 64);
    }
    if (lane == 0) {
        const bool on = l < (int)text_len[b];
        float* f = feats + ((int64_t)b * L + l) * 3;
        f[0] = log1pf((float)dur[(int64_t)b * L + l]);
        f[1] = on && np ? sp / (float)np : 0.0f;
        f[2] = on && ne ? se / (float)ne : 0.0f;
    }
}

int32_t hard_regulate_check(const char* what, const float* dur_f32, const int64_t* dur_i64, const void* x, const void* out,
                            int32_t B, int32_t frames, int32_t L, int32_t D, int64_t ldx) {
    ISPK_REQUIRE(x && out, ISPK_E_NULL, "%s: null pointer", what);
    ISPK_REQUIRE((dur_f32 != nullptr) != (dur_i64 != nullptr), ISPK_E_NULL, "%s: exactly one of dur_f32 / dur_i64 must be given", what);
    ISPK_REQUIRE(B >= 0 && B <= 65535 && frames >= 1 && L >= 1, ISPK_E_SHAPE, "%s: bad shape B=%d frames=%d L=%d", what, B, frames, L);
    ISPK_REQUIRE(L <= kHdMaxL, ISPK_E_SHAPE, "%s: L=%d tokens (at most %d, the aligner's limit)", what, L, kHdMaxL);
    ISPK_REQUIRE(D == 256 || D == 384, ISPK_E_UNSUPPORTED, "%s: dim %d (built for 256 / 384)", what, D);
    ISPK_REQUIRE(ldx >= D, ISPK_E_SHAPE, "%s: row stride %lld below dim %d", what, (long long)ldx, D);
    ISPK_REQUIRE(ispk_aligned(x, 16) && ispk_aligned(out, 16) && ldx % 4 == 0, ISPK_E_ALIGN,
                 "%s: x / out must be 16-byte aligned, the row stride a multiple of 4", what);
    return 0;
}

}  // namespace

extern "C" int32_t ispk_hard_regulate_f32(const float* dur_f32, const int64_t* dur_i64, const float* x, int64_t ldx, float* out,
                                          int64_t* dec_len, uint8_t* dec_mask, int32_t B, int32_t frames, int32_t L, int32_t D,
                                          int32_t max_len, ispk_stream_t stream) {
    ISPK_REQUIRE(dec_len, ISPK_E_NULL, "hard_regulate: null pointer");
    if (int32_t rc = hard_regulate_check("hard_regulate", dur_f32, dur_i64, x, out, B, frames, L, D, ldx)) return rc;
    if (B == 0) return 0;
    hipLaunchKernelGGL(hard_regulate_kernel, dim3((frames + kHdRows - 1) / kHdRows, B), dim3(kHdThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), dur_f32, dur_i64, x, ldx, out, dec_len, dec_mask, frames, L, D, max_len);
    return ispk_launch_status();
}

extern "C" int32_t ispk_hard_regulate_bwd_f32(const float* dur_f32, const int64_t* dur_i64, const float* d_out, float* d_x, int32_t B,
                                              int32_t rows, int32_t L, int32_t D, int32_t max_len, ispk_stream_t stream) {
    if (int32_t rc = hard_regulate_check("hard_regulate_bwd", dur_f32, dur_i64, d_out, d_x, B, rows, L, D, D)) return rc;
    if (B == 0) return 0;
    hipLaunchKernelGGL(hard_regulate_bwd_kernel, dim3((L + 3) / 4, B), dim3(kHdThreads), 0, reinterpret_cast<hipStream_t>(stream),
                       dur_f32, dur_i64, d_out, d_x, rows, L, D, max_len);
    return ispk_launch_status();
}

extern "C" int32_t ispk_hard_average_f32(const float* pitch, const float* energy, const int64_t* duration, const int64_t* text_len,
                                         float* feats, int32_t B, int32_t M, int32_t L, ispk_stream_t stream) {
    ISPK_REQUIRE(pitch && energy && duration && text_len && feats, ISPK_E_NULL, "hard_average: null pointer");
    ISPK_REQUIRE(B >= 0 && B <= 65535 && M >= 1 && L >= 1, ISPK_E_SHAPE, "hard_average: bad shape B=%d M=%d L=%d", B, M, L);
    ISPK_REQUIRE(L <= kHdMaxL, ISPK_E_SHAPE, "hard_average: L=%d tokens (at most %d, the aligner's limit)", L, kHdMaxL);
    if (B == 0) return 0;
    hipLaunchKernelGGL(hard_average_kernel, dim3((L + 3) / 4, B), dim3(kHdThreads), 0, reinterpret_cast<hipStream_t>(stream), pitch,
                       energy, duration, text_len, feats, M, L);
    return ispk_launch_status();
}
