// BigVGAN generator (isp_tts_amd/bigvgan.py): the anti-aliased periodic activation.  The convolutions are the HiFi-GAN ones
// (csrc/hifigan.hip, slope 1 = no activation on load); the activation is a stencil over time, so it is a pass of its own.
//
// Per utterance of n valid rows, channel c, output row t in [0, n)  (fu = taps[0..12), fd = taps[12..24)):
//   u[s] = 2 sum_{i = ceil((s+4)/2)}^{floor((s+15)/2)} fu[s + 15 - 2 i] x[clamp(i - 5, 0, n-1)]      s in [0, 2n): 6 taps
//   a[s] = u[s] + inv_b[c] sin(al[c] u[s])^2
//   y[t] = sum_{j=0}^{11} fd[j] a[clamp(2 t + j - 5, 0, 2n-1)]
// which is replicate-pad 5 -> 2x transposed-conv upsampling -> snake -> replicate-pad (5, 6) -> stride-2 low-pass.  In terms of
// the pair P(m) = (a[2m], a[2m+1]), which reads x[clamp(m-3 .. m+3)]:
//   a[2m]   = A(2 (fu[11] x[m-3] + fu[9] x[m-2] + fu[7] x[m-1] + fu[5] x[m] + fu[3] x[m+1] + fu[1] x[m+2]))
//   a[2m+1] = A(2 (fu[10] x[m-2] + fu[8] x[m-1] + fu[6] x[m] + fu[4] x[m+1] + fu[2] x[m+2] + fu[0] x[m+3]))
//   y[t]    = fd[0] a[2(t-3)+1] + fd[1] a[2(t-2)] + fd[2] a[2(t-2)+1] + ... + fd[10] a[2(t+2)+1] + fd[11] a[2(t+3)]
// and P(m) for m < 0 is (a[0], a[0]), for m >= n (a[2n-1], a[2n-1]).
//
//   snake_aa_kernel   grid (ceil(T / 512), C / 32, B), 256 threads: 8 lanes x float4 cover 32 channels of a row (128 B, one
//       cache line), the 32 lane groups of a workgroup own 32 consecutive tiles of kRows = 16 rows of ONE utterance.  A thread
//       walks m from t0 - 3 to its last row + 3 with the 7-row x window and 7 partial sums y[m-3 .. m+3] in registers: every
//       pair is evaluated once per tile (two accurate sinf per element: the argument is not range-limited) and scattered into
//       the partial sums in ascending j, so a row's sum runs in the same order wherever the tile lies; the 3 pairs (5 x rows)
//       on either side of a tile are recomputed, 22 / 16 of the sinf work.  Rows at or past n are never read and are written
//       as zeros.  Nothing depends on the neighbours of an utterance or on B.
//
// gfx950 resources (csrc/resource_report.py bigvgan.hip): snake_aa_kernel 128 VGPRs (4 waves / SIMD), no LDS, no spills.
#include "common.h"

namespace {

constexpr int kRows = 16;                 // rows per thread tile
constexpr int kTiles = 32;                // thread tiles per workgroup
constexpr int kWgRows = kRows * kTiles;   // 512 rows of one utterance per workgroup
constexpr int kMaxC = 512;

struct Taps {
    float fu[12], fd[12];
};

__device__ __forceinline__ float snake(float u, float al, float inv_b) {
    const float s = sinf(al * u);
    return fmaf(inv_b * s, s, u);
}

__global__ __launch_bounds__(256) void snake_aa_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ al,
                                                       const float* __restrict__ inv_b, const float* __restrict__ taps,
                                                       float* __restrict__ out, int64_t ldo, const int64_t* __restrict__ len,
                                                       int len_mul, int T) {
    const int b = blockIdx.z, tid = threadIdx.x;
    const int c = blockIdx.y * 32 + (tid & 7) * 4;
    const int t0 = blockIdx.x * kWgRows + (tid >> 3) * kRows;
    if (t0 >= T) return;
    const int n = valid_len(len, b, T, len_mul);
    const int64_t row0 = (int64_t)b * T;
    const float* xc = x + row0 * ldx + c;
    float* oc = out + row0 * ldo + c;
    const int tend = min(t0 + kRows, n);                     // rows [t0, tend) are computed
    for (int t = max(t0, n); t < min(t0 + kRows, T); ++t)    // rows at or past the length: zeros
        *reinterpret_cast<float4*>(oc + (int64_t)t * ldo) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t0 >= n) return;

    Taps f;
#pragma unroll
    for (int j = 0; j < 12; ++j) { f.fu[j] = taps[j]; f.fd[j] = taps[12 + j]; }
    const float4 al4 = *reinterpret_cast<const float4*>(al + c), ib4 = *reinterpret_cast<const float4*>(inv_b + c);
    const float alv[4] = {al4.x, al4.y, al4.z, al4.w}, ibv[4] = {ib4.x, ib4.y, ib4.z, ib4.w};

    auto load = [&](int r, float (&d)[4]) {                  // x[clamp(r, 0, n-1)]: never a row at or past n
        const float4 v = *reinterpret_cast<const float4*>(xc + (int64_t)min(max(r, 0), n - 1) * ldx);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    };

    float w[7][4];                                           // x[clamp(mc - 3 .. mc + 3)]
    float acc[7][4];                                         // partial y[m - 3 .. m + 3]
    float ae[4], ao[4];                                      // P(mc)
    int mc = min(max(t0 - 3, 0), n - 1);
#pragma unroll
    for (int q = 0; q < 7; ++q) load(mc - 3 + q, w[q]);
#pragma unroll
    for (int q = 0; q < 7; ++q)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[q][v] = 0.f;
    bool fresh = true;

    for (int m = t0 - 3; m < tend + 3; ++m) {
        const int want = min(max(m, 0), n - 1);
        if (want != mc) {                                    // the clamped position advances by one row at a time
            mc = want;
#pragma unroll
            for (int q = 0; q < 6; ++q)
#pragma unroll
                for (int v = 0; v < 4; ++v) w[q][v] = w[q + 1][v];
            load(mc + 3, w[6]);
            fresh = true;
        }
        if (fresh) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                float ue = f.fu[11] * w[0][v];
                ue = fmaf(f.fu[9], w[1][v], ue);
                ue = fmaf(f.fu[7], w[2][v], ue);
                ue = fmaf(f.fu[5], w[3][v], ue);
                ue = fmaf(f.fu[3], w[4][v], ue);
                ue = fmaf(f.fu[1], w[5][v], ue);
                float uo = f.fu[10] * w[1][v];
                uo = fmaf(f.fu[8], w[2][v], uo);
                uo = fmaf(f.fu[6], w[3][v], uo);
                uo = fmaf(f.fu[4], w[4][v], uo);
                uo = fmaf(f.fu[2], w[5][v], uo);
                uo = fmaf(f.fu[0], w[6][v], uo);
                ae[v] = snake(2.f * ue, alv[v], ibv[v]);
                ao[v] = snake(2.f * uo, alv[v], ibv[v]);
            }
            fresh = false;
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const float e = m >= n ? ao[v] : ae[v], o = m < 0 ? ae[v] : ao[v];
            // y[m + d] (acc[d + 3]) takes fd[5 - 2d] a[2m] and fd[6 - 2d] a[2m + 1]: j ascends as m does
            acc[6][v] = f.fd[0] * o;
#pragma unroll
            for (int d = 2; d >= -2; --d) acc[d + 3][v] = fmaf(f.fd[6 - 2 * d], o, fmaf(f.fd[5 - 2 * d], e, acc[d + 3][v]));
            acc[0][v] = fmaf(f.fd[11], e, acc[0][v]);
        }
        const int t = m - 3;                                 // complete with this step
        if (t >= t0)
            *reinterpret_cast<float4*>(oc + (int64_t)t * ldo) = make_float4(acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[q][v] = acc[q + 1][v];
    }
}

}  // namespace

extern "C" int32_t ispk_snake_aa_tile_rows(void) { return kWgRows; }

extern "C" int32_t ispk_snake_aa_f32(const float* x, int64_t ldx, const float* al, const float* inv_b, const float* taps,
                                     float* out, int64_t ldo, const int64_t* len, int32_t len_mul, int32_t B, int32_t T,
                                     int32_t C, ispk_stream_t stream) {
    if (B == 0 || T == 0) return 0;
    ISPK_REQUIRE(x && al && inv_b && taps && out, ISPK_E_NULL, "ispk_snake_aa_f32: null pointer");
    ISPK_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && len_mul >= 1, ISPK_E_SHAPE, "ispk_snake_aa_f32: bad shape B=%d T=%d len_mul=%d",
                 B, T, len_mul);
    ISPK_REQUIRE(C >= 32 && C <= kMaxC && C % 32 == 0, ISPK_E_UNSUPPORTED,
                 "ispk_snake_aa_f32: unsupported channel count C=%d (multiples of 32 up to %d are built)", C, kMaxC);
    ISPK_REQUIRE(ldx >= C && ldo >= C, ISPK_E_SHAPE, "ispk_snake_aa_f32: row strides ldx=%lld ldo=%lld shorter than the rows",
                 (long long)ldx, (long long)ldo);
    ISPK_REQUIRE(ldx % 4 == 0 && ldo % 4 == 0 && ispk_aligned(x, 16) && ispk_aligned(out, 16) && ispk_aligned(al, 16) &&
                     ispk_aligned(inv_b, 16),
                 ISPK_E_ALIGN, "ispk_snake_aa_f32: x, out, al and inv_b need 16-byte aligned rows (ldx=%lld ldo=%lld)",
                 (long long)ldx, (long long)ldo);
    ISPK_REQUIRE(x != out, ISPK_E_SHAPE, "ispk_snake_aa_f32: out may not be x (the rows around the one written are read)");
    const dim3 grid((T + kWgRows - 1) / kWgRows, C / 32, B);
    hipLaunchKernelGGL(snake_aa_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, ldx, al, inv_b, taps, out,
                       ldo, len, len_mul, T);
    return ispk_launch_status();
}
