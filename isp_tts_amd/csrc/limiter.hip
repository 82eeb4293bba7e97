// True-peak look-ahead limiter (isp_tts_amd/data/condition.py: Limiter; no counterpart in the reference): the last fp32 stage in
// front of PCM16.  One launch, no host read.  include/ispk.h has the definition (the interpolator h, the envelope e, the required
// gain r, the held minimum m, the smoothed gain s); the names below are its names.
//
//   limit_kernel   grid (ceil(S / 4096), B), 256 threads; a workgroup owns 4,096 output samples of one item.  With Ha = 2 L rounded
//                  up to a multiple of four it stages g x over the tile -(Ha + 8) .. +(Ha + 8) in LDS (16-byte loads where the
//                  item's first kept sample is 16-byte aligned, one float at a time otherwise; zeros outside the item), computes e
//                  and r over the tile +-Ha (a lane takes four consecutive samples: five 16-byte LDS reads, 36 FMAs a sample in
//                  tap order, phase 0 is the sample itself), and keeps its own sixteen g x in registers.  A tile in which no r is
//                  below 1 - the common one - is done: s = 1.  Otherwise the sliding minimum runs by doubling between the two LDS
//                  buffers (A_(k+1)[j] = min(A_k[j], A_k[j + 2^k]), p = floor(log2(2 L + 1)) passes, then m[j] = min(A_p[j - L],
//                  A_p[j + L - 2^p + 1]): two reads a sample whatever L), the deficits 1 - m go back to LDS as float64 over both
//                  buffers, and the smoothing sum runs in float64, a lane's four groups of four consecutive samples side by
//                  side: per four taps four weights (a broadcast) and eight 16-byte reads of deficits feed 64 FMAs.  The weights
//                  cos^2(pi k / (2 (L + 1))) / (L + 1) - their sum over |k| <= L is exactly L + 1 - are made in float64 by the
//                  workgroup.  out = clamp(fp32((double)(g x) s), -c, c): where s is 1 that is g x, the bits of cond_apply_kernel.
// true_peak and reduction of an item are a max and a min over non-negative floats, so the order of the tiles does not matter: a
// tile folds its own in a fixed tree and sends one integer atomic max / min on the bit pattern; the entry point sets both arrays
// (0 and 1.0f) with two 32-bit memsets on the stream in front of the launch, which a graph capture records as memset nodes.
// An item's bits depend on that item alone.  Every LDS index is formed from the tile, L and the thread, never from device data.
//
// gfx950 resources (csrc/resource_report.py limiter.hip): 134 VGPRs, no spills, no scratch; dynamic LDS 8 NW + 8 (4,096 + 2 Ha +
// 16) bytes with NW = 2 L + 4 rounded up to a multiple of four: 34.5 KB at L = 33, 45.2 KB at L = 256.  Inside a captured graph,
// 64 items of 131,072 samples at L = 33 (tools/time_limiter.py): 40 us when nothing is limited, 63 us with a peak in every 16,384
// samples, 85 us when every tile is limited, beside a traffic floor of 10.7 us; DESIGN.md 4.27 says what that appears bound by
// and what was tried.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int kLimTile = 4096;                      // output samples per workgroup: 16 per thread
constexpr int kLimThreads = 256;
constexpr int kLimMaxL = 256;
constexpr int kLimGroups = kLimTile / (4 * kLimThreads);
constexpr int kLimReach = 8;                        // staged samples on each side of the r range: the taps reach -5 .. +6
constexpr int kLimMaxNA = kLimTile + 4 * kLimMaxL;  // r values of a tile at the largest L
constexpr int kLimRGroups = kLimMaxNA / (4 * kLimThreads);      // 5
constexpr int kLimMGroups = (kLimTile + 2 * kLimMaxL + 8 + kLimThreads - 1) / kLimThreads;      // 19 values of m a lane at most
typedef double f64x2 __attribute__((ext_vector_type(2)));
constexpr int kLimXGroups =(kLimMaxNA + 2 * kLimReach + 4 * kLimThreads - 1) / (4 * kLimThreads);      // 6 staged groups a lane

struct LimArgs {
    const float* audio;
    int64_t ld;
    const int64_t* audio_len;
    const int64_t* bounds;
    const float* gain;
    const float* taps;
    float* out;
    int64_t ld_out;
    int64_t* out_len;
    unsigned int* true_peak;
    unsigned int* reduction;
    float c;
    int L, S, vec_in, vec_out, smooth;
};

__host__ __device__ constexpr int lim_halo(int L) { return (2 * L + 3) & ~3; }

__global__ __launch_bounds__(kLimThreads) void limit_kernel(const LimArgs a) {
#pragma clang fp contract(off)   // g x is the rounded product (cond_apply_kernel's); every FMA below is written as one
    extern __shared__ __attribute__((aligned(16))) unsigned char lim_lds[];
    __shared__ float red[2 * (kLimThreads / 64)];
    const int tid = threadIdx.x, b = blockIdx.y, L = a.L;
    const int Ha = lim_halo(L), Hx = Ha + kLimReach, NA = kLimTile + 2 * Ha, NX = NA + 2 * kLimReach, NW = (2 * L + 4 + 3) & ~3;
    double* W = reinterpret_cast<double*>(lim_lds);                        // NW weights, W[t] = w[t - L], 0 from 2 L + 1 on
    float* bufA = reinterpret_cast<float*>(lim_lds + 8 * (size_t)NW);       // NX floats each
    float* bufB = bufA + NX;

    // what is kept of the item: x[0, n) = audio[lo, hi)
    int64_t len = a.S;
    if (a.audio_len) {
        len = a.audio_len[b];
        if (len < 0 || len > a.S) len = 0;
    }
    int64_t lo = 0, hi = len;
    if (a.bounds) {
        lo = a.bounds[2 * b], hi = a.bounds[2 * b + 1];
        if (!(0 <= lo && lo <= hi && hi <= a.S)) lo = hi = 0;             // (device data)
        hi = hi < len ? hi : len;
        lo = lo < hi ? lo : hi;
    }
    const int64_t n = hi - lo, n0 = (int64_t)blockIdx.x * kLimTile;
    if (blockIdx.x == 0 && tid == 0 && a.out_len) a.out_len[b] = n;
    float* orow = a.out ? a.out + (int64_t)b * a.ld_out : nullptr;
    if (n0 >= n) {                                                         // (uniform) silence: nothing to read or measure
        if (orow) {
#pragma unroll
            for (int u = 0; u < kLimGroups; ++u) {
                const int64_t i = n0 + 4 * (u * kLimThreads + tid);
                if (a.vec_out && i + 4 <= a.S) {
                    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                    *reinterpret_cast<f32x4*>(orow + i) = z;
                } else {
                    for (int q = 0; q < 4; ++q)
                        if (i + q < a.S) orow[i + q] = 0.f;
                }
            }
        }
        return;
    }
    const float g = a.gain ? a.gain[b] : 1.f, c = a.c;
    const float* x = a.audio + (int64_t)b * a.ld + lo;
    const bool v4 = a.vec_in && lo % 4 == 0;

    // g x over [n0 - Hx, n0 - Hx + NX), zeros outside [0, n): nothing outside the kept range is read
    // (all of a lane's loads are issued before the first is used: one round trip, not six)
    f32x4 xv[kLimXGroups];
#pragma unroll
    for (int u = 0; u < kLimXGroups; ++u) {
        const int gi = u * kLimThreads + tid;
        const int64_t i = n0 - Hx + 4 * gi;
        xv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (gi < NX / 4) {
            if (v4 && i >= 0 && i + 4 <= n) {
                xv[u] = *reinterpret_cast<const f32x4*>(x + i);
            } else {
                if (i >= 0 && i < n) xv[u].x = x[i];
                if (i + 1 >= 0 && i + 1 < n) xv[u].y = x[i + 1];
                if (i + 2 >= 0 && i + 2 < n) xv[u].z = x[i + 2];
                if (i + 3 >= 0 && i + 3 < n) xv[u].w = x[i + 3];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kLimXGroups; ++u) {
        const int gi = u * kLimThreads + tid;
        if (gi < NX / 4) {
            f32x4 v = xv[u];
            v.x = g * v.x, v.y = g * v.y, v.z = g * v.z, v.w = g * v.w;
            *reinterpret_cast<f32x4*>(bufA + 4 * gi) = v;
        }
    }
    __syncthreads();

    // e and r over [n0 - Ha, n0 - Ha + NA) into bufB; r is 1 outside [0, n)
    float h[3][12];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int t = 0; t < 12; ++t) h[p][t] = a.taps[12 * (p + 1) + t];
    float pk = 0.f;
    int limited = 0;
#pragma unroll 1
    for (int u = 0; u < kLimRGroups; ++u) {
        const int q0 = 4 * (u * kLimThreads + tid);
        if (q0 >= NA) break;
        float v[20];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(bufA + q0 + 4 * j);
            v[4 * j] = t.x, v[4 * j + 1] = t.y, v[4 * j + 2] = t.z, v[4 * j + 3] = t.w;
        }
        float r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float e = fabsf(v[q + kLimReach]);                             // phase 0: the sample itself
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                float acc = 0.f;
#pragma unroll
                for (int t = 0; t < 12; ++t) acc = fmaf(h[p][t], v[q + 3 + t], acc);
                e = fmaxf(e, fabsf(acc));
            }
            const int64_t k = n0 - Ha + q0 + q;
            const bool inside = k >= 0 && k < n;
            r[q] = inside && e > c ? c / e : 1.f;
            pk = inside ? fmaxf(pk, e) : pk;
            limited |= r[q] < 1.f;
        }
        const f32x4 rv = {r[0], r[1], r[2], r[3]};
        *reinterpret_cast<f32x4*>(bufB + q0) = rv;
    }
    // the lane's own sixteen g x, before bufA is used again
    float y[kLimGroups][4];
#pragma unroll
    for (int u = 0; u < kLimGroups; ++u) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(bufA + Hx + 4 * (u * kLimThreads + tid));
        y[u][0] = t.x, y[u][1] = t.y, y[u][2] = t.z, y[u][3] = t.w;
    }
    pk = wave_max(pk);
    if ((tid & 63) == 0) red[tid >> 6] = pk;
    const int any = __syncthreads_or(limited);                             // (also: bufB is written, bufA and red are read)
    if (tid == 0) {
        pk = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        if (pk > 0.f) atomicMax(a.true_peak + b, __builtin_bit_cast(unsigned int, pk));
    }
    if (!a.smooth) return;                                                 // (uniform) the launch only measures

    double s[kLimGroups][4];
#pragma unroll
    for (int u = 0; u < kLimGroups; ++u) s[u][0] = s[u][1] = s[u][2] = s[u][3] = 1.0;
    if (any) {                                                             // (uniform)
        for (int t = tid; t < NW; t += kLimThreads) {
            const double cs = cos(M_PI * (double)(t - L) / (double)(2 * (L + 1)));
            W[t] = t <= 2 * L ? cs * cs / (double)(L + 1) : 0.0;
        }
        // the minimum over 2^p consecutive r, by doubling between the two buffers
        const int p = 31 - __clz(2 * L + 1);
        float* src = bufB;
        float* dst = bufA;
        for (int k = 0; k < p; ++k) {
            const int span = 1 << k;
#pragma unroll 4
            for (int j = tid; j < NA; j += kLimThreads) dst[j] = j + span < NA ? fminf(src[j], src[j + span]) : src[j];
            __syncthreads();
            float* t = src;
            src = dst, dst = t;
        }
        // m over [n0 - L, n0 + 4096 + L), 1 in the padding that only zero weights meet
        // The deficits 1 - m go back to LDS as float64, over BOTH buffers (NM doubles <= NX): a value of m meets (2 L + 1) / 4
        // lanes, and converting it in each of them was a third of the sum's float64 instructions.
        const int NM = kLimTile + NW;
        float mv[kLimMGroups];
#pragma unroll
        for (int v = 0; v < kLimMGroups; ++v) {
            const int u = v * kLimThreads + tid;
            mv[v] = u < kLimTile + 2 * L ? fminf(src[u + Ha - 2 * L], src[u + Ha - (1 << p) + 1]) : 1.f;
        }
        __syncthreads();                                                   // every A_p is read
        double* D = reinterpret_cast<double*>(bufA);
#pragma unroll
        for (int v = 0; v < kLimMGroups; ++v) {
            const int u = v * kLimThreads + tid;
            if (u < NM) D[u] = 1.0 - (double)mv[v];
        }
        __syncthreads();
        // the lane's four groups side by side: four independent reads of deficits and sixteen chains of FMAs behind one read of W
        const double* m = D + 4 * tid;
        double acc[kLimGroups][4];
#pragma unroll
        for (int u = 0; u < kLimGroups; ++u) acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.0;
        double wp0 = 0.0, wp1 = 0.0, wp2 = 0.0;                            // W[t - 1], W[t - 2], W[t - 3]
#pragma unroll 2
        for (int t = 0; t < NW; t += 4) {
            const double w0 = W[t], w1 = W[t + 1], w2 = W[t + 2], w3 = W[t + 3];
#pragma unroll
            for (int u = 0; u < kLimGroups; ++u) {
                const f64x2 da = *reinterpret_cast<const f64x2*>(m + 4 * u * kLimThreads + t);
                const f64x2 db = *reinterpret_cast<const f64x2*>(m + 4 * u * kLimThreads + t + 2);
                const double d0 = da.x, d1 = da.y, d2 = db.x, d3 = db.y;
                double a0 = acc[u][0], a1 = acc[u][1], a2 = acc[u][2], a3 = acc[u][3];
                a0 = fma(w0, d0, a0), a1 = fma(wp0, d0, a1), a2 = fma(wp1, d0, a2), a3 = fma(wp2, d0, a3);
                a0 = fma(w1, d1, a0), a1 = fma(w0, d1, a1), a2 = fma(wp0, d1, a2), a3 = fma(wp1, d1, a3);
                a0 = fma(w2, d2, a0), a1 = fma(w1, d2, a1), a2 = fma(w0, d2, a2), a3 = fma(wp0, d2, a3);
                a0 = fma(w3, d3, a0), a1 = fma(w2, d3, a1), a2 = fma(w1, d3, a2), a3 = fma(w0, d3, a3);
                acc[u][0] = a0, acc[u][1] = a1, acc[u][2] = a2, acc[u][3] = a3;
            }
            wp0 = w3, wp1 = w2, wp2 = w1;
        }
#pragma unroll
        for (int u = 0; u < kLimGroups; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) s[u][q] = fmax(1.0 - acc[u][q], 0.0);
    }

    float lowest = 1.f;
#pragma unroll
    for (int u = 0; u < kLimGroups; ++u) {
        const int64_t i = n0 + 4 * (u * kLimThreads + tid);
        if (i >= a.S) break;
        float o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            o[q] = 0.f;
            if (i + q < n) {
                o[q] = fminf(fmaxf((float)((double)y[u][q] * s[u][q]), -c), c);
                lowest = fminf(lowest, (float)s[u][q]);
            }
        }
        if (!orow) continue;
        if (a.vec_out && i + 4 <= a.S) {
            const f32x4 v = {o[0], o[1], o[2], o[3]};
            *reinterpret_cast<f32x4*>(orow + i) = v;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (i + q < a.S) orow[i + q] = o[q];
        }
    }
    if (!any || !a.reduction) return;                                      // (uniform) untouched: the 1.0f of the memset stands
    lowest = -wave_max(-lowest);
    if ((tid & 63) == 0) red[4 + (tid >> 6)] = lowest;
    __syncthreads();
    if (tid == 0) {
        lowest = fminf(fminf(red[4], red[5]), fminf(red[6], red[7]));
        if (lowest < 1.f) atomicMin(a.reduction + b, __builtin_bit_cast(unsigned int, lowest));
    }
}

bool lim_overlap(const void* p, int64_t pb, const void* q, int64_t qb) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}

}  // namespace

extern "C" int32_t ispk_limit_tile_samples(void) { return kLimTile; }

extern "C" int32_t ispk_limit_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const int64_t* bounds,
                                  const float* gain, const float* taps, float ceiling, int32_t lookahead, float* out, int64_t ld_out,
                                  int64_t* out_len, float* true_peak, float* reduction, int32_t B, int32_t S, ispk_stream_t stream) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= (1 << 24), ISPK_E_SHAPE,
                 "ispk_limit_f32: bad shape B=%d S=%d (B <= 65535, S <= 2^24)", B, S);
    ISPK_REQUIRE(lookahead >= 1 && lookahead <= kLimMaxL, ISPK_E_SHAPE, "ispk_limit_f32: lookahead %d outside 1 .. %d samples", lookahead,
                 kLimMaxL);
    ISPK_REQUIRE(ceiling > 0.f && ceiling <= 3.0e38f, ISPK_E_SHAPE, "ispk_limit_f32: the ceiling %g is not positive and finite",
                 (double)ceiling);
    if (B == 0) return 0;
    ISPK_REQUIRE(audio && taps && true_peak, ISPK_E_NULL, "ispk_limit_f32: null pointer (audio, taps, true_peak)");
    ISPK_REQUIRE(!out || reduction, ISPK_E_NULL, "ispk_limit_f32: null pointer (reduction goes with out)");
    ISPK_REQUIRE(out || !out_len, ISPK_E_NULL, "ispk_limit_f32: null pointer (out_len without out)");
    ISPK_REQUIRE(ld_audio >= S && (!out || ld_out >= S), ISPK_E_SHAPE, "ispk_limit_f32: row strides %lld, %lld below S=%d",
                 (long long)ld_audio, (long long)ld_out, S);
    ISPK_REQUIRE(ispk_aligned(true_peak, 4) && ispk_aligned(reduction, 4), ISPK_E_ALIGN,
                 "ispk_limit_f32: true_peak and reduction are updated as 32-bit words and need 4-byte alignment");
    ISPK_REQUIRE(!out || !lim_overlap(audio, 4 * ((int64_t)(B - 1) * ld_audio + S), out, 4 * ((int64_t)(B - 1) * ld_out + S)), ISPK_E_SHAPE,
                 "ispk_limit_f32: out may not alias audio (a tile reads its neighbours' samples)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(true_peak), 0, (size_t)B, st);
    if (e == hipSuccess && reduction)
        e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(reduction), 0x3f800000, (size_t)B, st);
    if (e != hipSuccess) ISPK_FAIL((int32_t)e, "ispk_limit_f32: cannot initialise the per-item results: %s", hipGetErrorString(e));
    LimArgs a;
    a.audio = audio, a.ld = ld_audio, a.audio_len = audio_len, a.bounds = bounds, a.gain = gain, a.taps = taps;
    a.out = out, a.ld_out = ld_out, a.out_len = out_len;
    a.true_peak = reinterpret_cast<unsigned int*>(true_peak), a.reduction = reinterpret_cast<unsigned int*>(reduction);
    a.c = ceiling, a.L = lookahead, a.S = S;
    a.vec_in = ld_audio % 4 == 0 && ispk_aligned(audio, 16);
    a.vec_out = out && ld_out % 4 == 0 && ispk_aligned(out, 16);
    a.smooth = out || reduction;
    const int Ha = lim_halo(lookahead), NW = (2 * lookahead + 4 + 3) & ~3;
    const size_t lds = 8 * (size_t)NW + 8 * (size_t)(kLimTile + 2 * Ha + 2 * kLimReach);
    const unsigned gx = (unsigned)std::max<int64_t>(1, ((int64_t)S + kLimTile - 1) / kLimTile);        // (S = 0: out_len alone)
    hipLaunchKernelGGL(limit_kernel, dim3(gx, B), dim3(kLimThreads), lds, st, a);
    return ispk_launch_status();
}
