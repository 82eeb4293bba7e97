// The acoustic model's evaluation metrics (models/acoustic/evaluator.py:14-67 of the reference): mel-cepstral distortion over
// a DCT-II basis and the alignment length / strength of the soft attention, all three in two launches.
//
//   metrics_chunk_kernel  grid (ceil(T / kChunk), B): one workgroup per (item, 32-frame chunk).  It stages the chunk's mel
//                         difference columns in LDS, projects them on the DCT basis (coefficients 1 .. n_mfcc - 1), and takes
//                         the first-index argmax / max of its attention rows plus the row just before the chunk, so that the
//                         step across the chunk boundary needs no communication.  Three partial sums per (item, chunk) go to
//                         the workspace, each summed in a fixed order.
//   metrics_final_kernel  one workgroup: per item, the partials in chunk order; then the batch means in a fixed tree order.
// No floating-point atomics anywhere: repeated calls and graph replays give the same bits.
#include "common.h"

namespace {

constexpr int kChunk = 32;            // frames per workgroup
constexpr int kThreads = 256;
constexpr int kMaxC = 128;            // mel channels (LDS tile kChunk x (kMaxC + 1))
constexpr int kFinalThreads = 256;
// 10 sqrt(2) / ln 10 (MCD._logdb_const, evaluator.py:19), rounded once to fp32
constexpr float kLogDb = 6.14185781393705f;

// (v, i) beats (bv, bi) under torch's argmax rule: NaN is the largest value, ties go to the smaller index
__device__ __forceinline__ bool beats(float v, int i, float bv, int bi) {
    const bool n = v != v, bn = bv != bv;
    if (n != bn) return n;
    if (!n && v != bv) return v > bv;
    return i < bi;
}

struct MelView {
    const float* p;
    int64_t sb, sc, st;
};

// d[f][c] = x[c][t0 + f] - y[c][t0 + f] for the chunk's frames < T (0 elsewhere)
__device__ __forceinline__ void stage_diff(float* d, const MelView x, const MelView y, int b, int t0, int C, int T, bool vec_t,
                                           bool vec_c) {
    const float* xb = x.p + (int64_t)b * x.sb;
    const float* yb = y.p + (int64_t)b * y.sb;
    const int ld = C + 1;
    if (vec_t) {            // unit frame stride: 4 consecutive frames of one channel per float4
        for (int i = threadIdx.x; i < C * (kChunk / 4); i += kThreads) {
            const int c = i / (kChunk / 4), f = (i % (kChunk / 4)) * 4, t = t0 + f;
            if (t + 3 < T) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(xb + c * x.sc + t);
                const f32x4 e = *reinterpret_cast<const f32x4*>(yb + c * y.sc + t);
                d[(f + 0) * ld + c] = a.x - e.x;
                d[(f + 1) * ld + c] = a.y - e.y;
                d[(f + 2) * ld + c] = a.z - e.z;
                d[(f + 3) * ld + c] = a.w - e.w;
            } else {
                for (int j = 0; j < 4; ++j)
                    d[(f + j) * ld + c] = t + j < T ? xb[c * x.sc + t + j] - yb[c * y.sc + t + j] : 0.f;
            }
        }
    } else if (vec_c) {     // unit channel stride, C % 4 == 0: 4 consecutive channels of one frame per float4
        const int c4 = C / 4;
        for (int i = threadIdx.x; i < kChunk * c4; i += kThreads) {
            const int f = i / c4, c = (i % c4) * 4, t = t0 + f;
            if (t < T) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(xb + t * x.st + c);
                const f32x4 e = *reinterpret_cast<const f32x4*>(yb + t * y.st + c);
                d[f * ld + c + 0] = a.x - e.x;
                d[f * ld + c + 1] = a.y - e.y;
                d[f * ld + c + 2] = a.z - e.z;
                d[f * ld + c + 3] = a.w - e.w;
            } else {
                d[f * ld + c + 0] = d[f * ld + c + 1] = d[f * ld + c + 2] = d[f * ld + c + 3] = 0.f;
            }
        }
    } else {                // any strides: one element per thread, frames fastest
        for (int i = threadIdx.x; i < C * kChunk; i += kThreads) {
            const int c = i / kChunk, f = i % kChunk, t = t0 + f;
            d[f * ld + c] = t < T ? xb[c * x.sc + (int64_t)t * x.st] - yb[c * y.sc + (int64_t)t * y.st] : 0.f;
        }
    }
}

__global__ void __launch_bounds__(kThreads) metrics_chunk_kernel(MelView x, MelView y, const float* __restrict__ dct,
                                                                 const float* __restrict__ attn, int64_t attn_sb, int64_t attn_st,
                                                                 const int64_t* __restrict__ mel_len, float* __restrict__ part, int B, int C, int T, int L, int n_mfcc,
                                                                 bool vec_t, bool vec_c, bool vec_l) {
    __shared__ float diff[kChunk * (kMaxC + 1)];
    __shared__ float sq[kChunk][kMaxC + 1];
    extern __shared__ float dct_s[];      // [C][n_mfcc] (dynamic: C * n_mfcc floats when the mels are given)
    __shared__ float rowmax[kChunk + 1];
    __shared__ int rowarg[kChunk + 1];
    const int chunk = blockIdx.x, b = blockIdx.y, nch = gridDim.x;
    const int t0 = chunk * kChunk;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int nf = min(kChunk, T - t0);

    // ---- alignment: rows t0 - 1 .. t0 + nf - 1 (slot 0 = the row before the chunk), one wavefront per row
    if (attn) {
        for (int r = wave; r <= kChunk; r += kThreads / kWave) {
            const int t = t0 - 1 + r;
            if (t < 0 || t >= T) continue;
            const float* row = attn + (int64_t)b * attn_sb + (int64_t)t * attn_st;
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            if (vec_l) {    // L % 4 == 0, 16-byte aligned rows: lane reads l = 4 lane + 256 j .. + 3, in increasing order
                for (int l = 4 * lane; l < L; l += 4 * kWave) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(row + l);
                    if (beats(v.x, l, bv, bi)) bv = v.x, bi = l;
                    if (beats(v.y, l + 1, bv, bi)) bv = v.y, bi = l + 1;
                    if (beats(v.z, l + 2, bv, bi)) bv = v.z, bi = l + 2;
                    if (beats(v.w, l + 3, bv, bi)) bv = v.w, bi = l + 3;
                }
            } else {
                for (int l = lane; l < L; l += kWave) {
                    const float v = row[l];
                    if (beats(v, l, bv, bi)) bv = v, bi = l;
                }
            }
            for (int o = kWave / 2; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o);
                const int oi = __shfl_xor(bi, o);
                if (beats(ov, oi, bv, bi)) bv = ov, bi = oi;
            }
            if (lane == 0) {
                rowmax[r] = bv;
                rowarg[r] = bi;
            }
        }
    }

    // ---- MCD: sq[f][k] = ((x - y) . D[:, k])^2 for k = 1 .. n_mfcc - 1
    if (x.p) {
        for (int i = threadIdx.x; i < C * n_mfcc; i += kThreads) dct_s[i] = dct[i];
        stage_diff(diff, x, y, b, t0, C, T, vec_t, vec_c);
        __syncthreads();
        const int nk = n_mfcc - 1;
        for (int i = threadIdx.x; i < nf * nk; i += kThreads) {
            const int f = i / nk, k = 1 + i % nk;
            const float* dr = diff + f * (C + 1);
            float acc = 0.f;
            for (int c = 0; c < C; ++c) acc = fmaf(dr[c], dct_s[c * n_mfcc + k], acc);
            sq[f][k - 1] = acc * acc;
        }
    }
    __syncthreads();

    // ---- the three partials of this (item, chunk): lane f of wave 0 takes frame t0 + f, then a fixed butterfly over the lanes
    if (wave == 0) {
        const int f = lane;
        float e_mcd = 0.f, e_len = 0.f, e_str = 0.f;
        if (f < nf) {
            if (x.p) {
                float e = 0.f;
                for (int k = 0; k < n_mfcc - 1; ++k) e += sq[f][k];
                e_mcd = sqrtf(e);
            }
            if (attn) {
                // the step INTO frame t counts for 1 <= t <= mel_len - 1; the maximum of every frame, padding included
                const int t = t0 + f;
                if (t >= 1 && t < mel_len[b]) {
                    const float dd = (float)(rowarg[f + 1] - rowarg[f]);
                    e_len = sqrtf(1.f + dd * dd);
                }
                e_str = rowmax[f + 1];
            }
        }
        for (int o = kWave / 2; o > 0; o >>= 1) {
            e_mcd += __shfl_xor(e_mcd, o);
            e_len += __shfl_xor(e_len, o);
            e_str += __shfl_xor(e_str, o);
        }
        if (lane == 0) {
            const int64_t o = (int64_t)b * nch + chunk, plane = (int64_t)B * nch;
            if (x.p) part[o] = e_mcd;
            if (attn) {
                part[plane + o] = e_len;
                part[2 * plane + o] = e_str;
            }
        }
    }
}

__global__ void __launch_bounds__(kFinalThreads) metrics_final_kernel(const float* __restrict__ part, const int64_t* __restrict__ mel_len,
                                                                      const int64_t* __restrict__ text_len, float* __restrict__ out,
                                                                      int B, int T, int nch, bool mcd, bool align) {
    __shared__ float red[3][kFinalThreads];
    __shared__ long long lens[kFinalThreads];
    __shared__ int bad[kFinalThreads];
    const int64_t plane = (int64_t)B * nch;
    float m = 0.f, a = 0.f, s = 0.f;
    long long n = 0;
    int invalid = 0;
    for (int b = threadIdx.x; b < B; b += kFinalThreads) {
        const int64_t ml = mel_len[b];
        invalid |= ml < 1 || ml > T;
        n += ml;
        const float* pm = part + (int64_t)b * nch;
        float sm = 0.f, sa = 0.f, ss = 0.f;
        for (int c = 0; c < nch; ++c) {
            if (mcd) sm += pm[c];
            if (align) {
                sa += pm[plane + c];
                ss += pm[2 * plane + c];
            }
        }
        const float fl = (float)ml;
        if (mcd) m += kLogDb * sm / fl;
        if (align) {
            const float tl = (float)text_len[b];
            a += sa / sqrtf(tl * tl + fl * fl);
            s += ss;
        }
    }
    red[0][threadIdx.x] = m;
    red[1][threadIdx.x] = a;
    red[2][threadIdx.x] = s;
    lens[threadIdx.x] = n;
    bad[threadIdx.x] = invalid;
    __syncthreads();
    for (int w = kFinalThreads / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            for (int j = 0; j < 3; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + w];
            lens[threadIdx.x] += lens[threadIdx.x + w];
            bad[threadIdx.x] |= bad[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float nan = __builtin_nanf("");
        const float fb = (float)B;
        if (mcd) out[0] = bad[0] ? nan : red[0][0] / fb;
        if (align) {
            out[1] = bad[0] ? nan : red[1][0] / fb;
            out[2] = bad[0] ? nan : red[2][0] / (float)lens[0];
        }
    }
}

}  // namespace

extern "C" int32_t ispk_acoustic_metrics_f32(const float* mel_out, int64_t out_sb, int64_t out_sc, int64_t out_st,
                                             const float* mel_target, int64_t tgt_sb, int64_t tgt_sc, int64_t tgt_st,
                                             const int64_t* mel_len, const int64_t* text_len, const float* attn_soft,
                                             int64_t attn_sb, int64_t attn_st, const float* dct, float* workspace,
                                             int64_t workspace_floats, float* out, int32_t B, int32_t C, int32_t T, int32_t L,
                                             int32_t n_mfcc, ispk_stream_t stream) {
    const bool mcd = mel_out || mel_target, align = attn_soft != nullptr;
    ISPK_REQUIRE(mel_len && workspace && out && (mcd || align), -1, "ispk_acoustic_metrics_f32: null pointer");
    ISPK_REQUIRE(!mcd || (mel_out && mel_target && dct), -1, "ispk_acoustic_metrics_f32: null mel or DCT pointer");
    ISPK_REQUIRE(!align || text_len, -1, "ispk_acoustic_metrics_f32: null text_len");
    ISPK_REQUIRE(B >= 1 && B <= 65535 && T >= 1, -2, "ispk_acoustic_metrics_f32: bad shape B=%d T=%d", B, T);
    ISPK_REQUIRE(!align || L >= 1, -2, "ispk_acoustic_metrics_f32: bad shape L=%d", L);
    ISPK_REQUIRE(!mcd || (C >= 1 && C <= kMaxC && n_mfcc >= 1 && n_mfcc <= C), -2,
                 "ispk_acoustic_metrics_f32: need 1 <= n_mfcc <= C <= %d (C=%d n_mfcc=%d)", kMaxC, C, n_mfcc);
    const int nch = (T + kChunk - 1) / kChunk;
    const int64_t need = 3 * (int64_t)B * nch;
    ISPK_REQUIRE(workspace_floats >= need, -3, "ispk_acoustic_metrics_f32: workspace needs %lld floats", (long long)need);
    const bool vec_t = mcd && out_st == 1 && tgt_st == 1 && out_sb % 4 == 0 && out_sc % 4 == 0 && tgt_sb % 4 == 0 &&
                       tgt_sc % 4 == 0 && ispk_aligned(mel_out, 16) && ispk_aligned(mel_target, 16);
    const bool vec_c = mcd && !vec_t && out_sc == 1 && tgt_sc == 1 && C % 4 == 0 && out_sb % 4 == 0 && out_st % 4 == 0 &&
                       tgt_sb % 4 == 0 && tgt_st % 4 == 0 && ispk_aligned(mel_out, 16) && ispk_aligned(mel_target, 16);
    const bool vec_l = align && L % 4 == 0 && attn_sb % 4 == 0 && attn_st % 4 == 0 && ispk_aligned(attn_soft, 16);
    const size_t lds = mcd ? sizeof(float) * (size_t)C * n_mfcc : 0;
    ISPK_RESERVE_LDS(metrics_chunk_kernel, lds + sizeof(float) * (kChunk * (2 * kMaxC + 1) + 2 * (kChunk + 1) + kChunk),
                     "ispk_acoustic_metrics_f32");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(metrics_chunk_kernel, dim3(nch, B), dim3(kThreads), lds, s, MelView{mel_out, out_sb, out_sc, out_st},
                       MelView{mel_target, tgt_sb, tgt_sc, tgt_st}, dct, attn_soft, attn_sb, attn_st, mel_len, workspace, B, C, T, L,
                       n_mfcc, vec_t, vec_c, vec_l);
    hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(kFinalThreads), 0, s, workspace, mel_len, text_len, out, B, T, nch,
                       mcd, align);
    return ispk_launch_status();
}
