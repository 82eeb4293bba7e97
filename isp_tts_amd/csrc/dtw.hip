// Dynamic time warping for gfx950: scoring free-running synthesis against a recording (MCD-DTW, F0 RMSE and
// voiced / unvoiced error along the warping path, length ratio).  DESIGN.md 4.15.
//
//   D[0][0] = c[0][0];  D[i][j] = c[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]);
//   ties go to the diagonal, then to (i-1, j), then to (i, j-1); the backtrace runs from (n_len-1, m_len-1).
//
//   dtw_kernel          one workgroup of 4 waves per item.  Lane g of the 256 owns R consecutive rows (R = 1, 2, 4 or 8, picked
//                       on the device from the item's own n_len) and walks the columns; lane l of a wave is l columns behind
//                       lane 0, so that one step of the wave is one anti-diagonal of its 64 R rows.  Inside a lane the left
//                       and diagonal neighbours are registers; the row above a lane's first row comes from the lane before
//                       through one DPP wave shift per step; the row above a wave's first row comes from the wave before
//                       through an LDS row buffer.  Waves run two 64-step blocks apart with one barrier per block, which is
//                       what makes every value of that buffer written one barrier before it is read.  The costs come from a
//                       skewed copy in the workspace (one row of it = one step of a wave, 64 R consecutive floats), prefetched
//                       one group of 64 cells per lane ahead; the 2-bit back-pointers of a lane's R rows are packed over
//                       16 / R columns into one word of the workspace.
//                       Backtrace: the back-pointers of a 64 x 64 window ending at the current cell are decoded into LDS by the
//                       whole workgroup, one thread walks the window (>= 64 steps), until (0, 0).  The path is kept in LDS in
//                       reverse, written out forwards, and the pitch terms are summed along it in a fixed order.
//   cepstra_kernel      the cepstral coefficients 1 .. n_mfcc - 1 of every frame of both mels, once per frame.
//   cost_kernel         c[i][j] = |cep_out[i] - cep_target[j]|, written straight into the skewed layout.
//   skew_kernel         ispk_dtw_f32's row-major cost matrix into the skewed layout.
//   dtw_means_kernel    the batch means in a fixed tree order.
// No floating-point atomics anywhere: repeated calls and graph replays give the same bits.
#include "common.h"

namespace {

constexpr int kMaxLen = 2048;         // N and M limit
constexpr int kThreads = 256;         // 4 waves per item
constexpr int kWaves = kThreads / kWave;
constexpr int kWin = 64;              // backtrace window (cells per side)
constexpr int kMaxC = 128;
constexpr int kFrames = 32;           // frames per workgroup of cepstra_kernel
constexpr int kTile = 64, kKc = 32;   // cost_kernel: cells per side, coefficients per pass
// 10 sqrt(2) / ln 10 (MCD._logdb_const), rounded once to fp32 as in metrics.hip
constexpr float kLogDb = 6.14185781393705f;

__host__ __device__ constexpr int rows_per_lane(int n) { return n <= 256 ? 1 : (n <= 512 ? 2 : (n <= 1024 ? 4 : 8)); }
// back-pointer words of one item: 256 lanes x ceil(M / (16 / R)) words of 16 / R columns x R rows x 2 bits
__host__ __device__ constexpr int64_t bp_words(int rows, int M) {
    const int cpw = 16 / rows_per_lane(rows);
    return (int64_t)kThreads * ((M + cpw - 1) / cpw);
}

// The skewed cost layout the forward pass reads: cell (i, j) of an item whose lanes own R rows each sits at
// (j + i / R) * 256 R + i.  Lane g = i / R reaches column j at step j + g - 64 (g / 64) of its wave, so one step of a wave reads
// ONE row of this layout: 64 R consecutive floats, R per lane.  M + 255 rows; the cells outside n x m are never written and
// whatever they hold never reaches a cell inside.
__host__ __device__ constexpr int64_t skew_floats(int rows, int M) { return (int64_t)(M + kThreads - 1) * kThreads * rows_per_lane(rows); }

struct DtwArgs {
    const float* skew;     // the costs in the skewed layout, skew_item floats per item
    int64_t skew_item;
    const int64_t* n_len;
    const int64_t* m_len;
    float* total;          // [B]
    int32_t* steps;        // [B]
    int16_t* path;         // [B][N + M - 1][2] or null
    uint32_t* bp;          // back-pointer words, bp_item per item
    int64_t bp_item;
    const float* pitch_out;     // [B][>= N] Hz or null
    const float* pitch_tgt;     // [B][>= M]
    int64_t po_sb, pt_sb;
    float* per_item;       // [4][B] or null
    int B, N, M;
};

// Rows d0 .. d0 + G - 1 of the skewed layout: the lane's R rows at its next G columns (0 past the layout's last row).
template <int R, int G>
__device__ __forceinline__ void fetch(float (&dst)[G][R], const float* __restrict__ sk, int d0, int nd) {
    const float* p = sk + (int64_t)d0 * (kThreads * R) + threadIdx.x * R;
#pragma unroll
    for (int q = 0; q < G; ++q, p += kThreads * R) {
        if (d0 + q < nd) {
            if constexpr (R >= 4) {
#pragma unroll
                for (int r = 0; r < R; r += 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(p + r);
                    dst[q][r] = v.x, dst[q][r + 1] = v.y, dst[q][r + 2] = v.z, dst[q][r + 3] = v.w;
                }
            } else if constexpr (R == 2) {
                const f32x2 v = *reinterpret_cast<const f32x2*>(p);
                dst[q][0] = v.x, dst[q][1] = v.y;
            } else {
                dst[q][0] = p[0];
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) dst[q][r] = 0.f;
        }
    }
}

// The forward pass of one item with R rows per lane: fills the back-pointer words and *total_s.
template <int R>
__device__ void dtw_forward(const float* __restrict__ sk, int nd, int n, int m, uint32_t* __restrict__ bp, int wp,
                            float* __restrict__ bnd, float* total_s) {
    constexpr int G = 64 / R;        // steps per prefetch group (64 cells per lane in flight)
    constexpr int CPW = 16 / R;      // columns per back-pointer word
    const int g = threadIdx.x, w = g / kWave, l = g % kWave;
    const int i0 = g * R;
    const int nblk = (m + 2 * kWave - 2) / kWave;                // 64-step blocks of one wave: steps 0 .. m + 62
    const int nwav = (n + kWave * R - 1) / (kWave * R);          // waves that own a row < n
    const int nt = nblk + 2 * (nwav - 1);
    float prev[R];
#pragma unroll
    for (int r = 0; r < R; ++r) prev[r] = INFINITY;
    float diag = g == 0 ? 0.f : INFINITY;     // D[i0 - 1][j - 1]; the 0 makes D[0][0] = c[0][0]
    float bottom = INFINITY;                  // D[i0 + R - 1][j] of the lane's last step
    uint32_t acc = 0;
    float cur[G][R], nxt[G][R];
    for (int t = 0; t < nt; ++t) {
        const int tl = t - 2 * w;
        if (w < nwav && tl >= 0 && tl < nblk) {
            // the row above this wave's first row, for the 64 columns lane 0 takes in this block
            float above = INFINITY;
            if (w > 0 && tl * kWave + l < m) above = bnd[(w - 1) * kMaxLen + tl * kWave + l];
            if (tl == 0) fetch<R, G>(cur, sk, w * kWave, nd);
            for (int grp = 0; grp < kWave / G; ++grp) {
                const int s0 = tl * kWave + grp * G;
                fetch<R, G>(nxt, sk, s0 + G + w * kWave, nd);
#pragma unroll
                for (int q = 0; q < G; ++q) {
                    const int j = s0 + q - l;
                    float recv = dpp_shr1(bottom, INFINITY);
                    const float first = __builtin_bit_cast(
                        float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, above), grp * G + q));
                    if (l == 0) recv = first;
                    if (j >= 0 && j < m) {
                        float up = recv, dg = diag;
                        uint32_t bits = 0;
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const float left = prev[r];
                            const bool d0 = dg <= up && dg <= left;
                            const bool d1 = up <= left;
                            const float val = cur[q][r] + (d0 ? dg : (d1 ? up : left));
                            bits |= (d0 ? 0u : (d1 ? 1u : 2u)) << (2 * r);
                            dg = left;
                            up = val;
                            prev[r] = val;
                        }
                        diag = recv;
                        bottom = up;
                        if (l == kWave - 1 && w < kWaves - 1) bnd[w * kMaxLen + j] = bottom;
                        const int ph = j % CPW;
                        acc = ph == 0 ? bits : (acc | (bits << (ph * 2 * R)));
                        if (ph == CPW - 1 || j == m - 1) bp[(int64_t)g * wp + j / CPW] = acc;
                    }
                }
#pragma unroll
                for (int q = 0; q < G; ++q)
#pragma unroll
                    for (int r = 0; r < R; ++r) cur[q][r] = nxt[q][r];
            }
        }
        __syncthreads();
    }
    // a lane stops at column m - 1, so prev[] still holds that column: D[n - 1][m - 1] is with the owner of row n - 1
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (i0 + r == n - 1) *total_s = prev[r];
}

__global__ void __launch_bounds__(kThreads) dtw_kernel(DtwArgs a) {
    __shared__ float bnd[(kWaves - 1) * kMaxLen];
    __shared__ uint32_t pth[2 * kMaxLen];
    __shared__ uint8_t win[kWin][kWin];
    __shared__ int ctl[4];
    __shared__ float total_s;
    __shared__ float red[3][kThreads];
    const int b = blockIdx.x, t = threadIdx.x;
    const int64_t nl = a.n_len[b], ml = a.m_len[b];
    const int plen = a.N + a.M - 1;
    int16_t* path = a.path ? a.path + (int64_t)b * plen * 2 : nullptr;
    if (nl < 1 || nl > a.N || ml < 1 || ml > a.M) {      // the lengths are device data: NaN, no path
        if (t == 0) {
            const float nan = __builtin_nanf("");
            if (a.total) a.total[b] = nan;
            if (a.steps) a.steps[b] = 0;
            if (a.per_item) {
                a.per_item[b] = nan;
                if (a.pitch_out) a.per_item[a.B + b] = a.per_item[2 * a.B + b] = nan;
                a.per_item[3 * a.B + b] = nan;
            }
        }
        if (path)
            for (int k = t; k < 2 * plen; k += kThreads) path[k] = -1;
        return;
    }
    const int n = (int)nl, m = (int)ml;
    const int R = rows_per_lane(n), cpw = 16 / R, wp = (a.M + cpw - 1) / cpw;
    uint32_t* bp = a.bp + (int64_t)b * a.bp_item;
    const float* sk = a.skew + (int64_t)b * a.skew_item;
    const int nd = a.M + kThreads - 1;
    if (R == 1) dtw_forward<1>(sk, nd, n, m, bp, wp, bnd, &total_s);
    else if (R == 2) dtw_forward<2>(sk, nd, n, m, bp, wp, bnd, &total_s);
    else if (R == 4) dtw_forward<4>(sk, nd, n, m, bp, wp, bnd, &total_s);
    else dtw_forward<8>(sk, nd, n, m, bp, wp, bnd, &total_s);

    // ---- backtrace (the forward pass ended with a barrier: the back-pointer words are visible to the workgroup)
    if (t == 0) ctl[0] = n - 1, ctl[1] = m - 1, ctl[2] = 0, ctl[3] = 0;
    __syncthreads();
    for (;;) {
        const int ci = ctl[0], cj = ctl[1];
        const int wi0 = ci - (kWin - 1), wj0 = cj - (kWin - 1);
        {
            const int rr = t >> 2, i = wi0 + rr;
            if (i >= 0) {
                const uint32_t* row = bp + (int64_t)(i / R) * wp;
                const int sh = 2 * (i % R);
                for (int c = 0; c < kWin / 4; ++c) {
                    const int cc = (t & 3) * (kWin / 4) + c, j = wj0 + cc;
                    if (j >= 0) win[rr][cc] = (uint8_t)((row[j / cpw] >> ((j % cpw) * 2 * R + sh)) & 3u);
                }
            }
        }
        __syncthreads();
        if (t == 0) {
            int i = ci, j = cj, k = ctl[2], done = 0;
            while (i >= wi0 && j >= wj0) {
                pth[k++] = (uint32_t)i | ((uint32_t)j << 16);
                if (i == 0 && j == 0) {
                    done = 1;
                    break;
                }
                int d = win[i - wi0][j - wj0];
                if (i == 0) d = 2;               // (the edges have one predecessor whatever the cost held)
                else if (j == 0) d = 1;
                if (d == 0) --i, --j;
                else if (d == 1) --i;
                else --j;
            }
            ctl[0] = i, ctl[1] = j, ctl[2] = k, ctl[3] = done;
        }
        __syncthreads();
        if (ctl[3]) break;
    }
    const int K = ctl[2];
    if (t == 0) {
        if (a.total) a.total[b] = total_s;
        if (a.steps) a.steps[b] = K;
    }
    if (path) {
        for (int k = t; k < plen; k += kThreads) {
            const uint32_t v = k < K ? pth[K - 1 - k] : 0xffffffffu;
            path[2 * k] = (int16_t)(v & 0xffffu);
            path[2 * k + 1] = (int16_t)(v >> 16);
        }
    }
    if (!a.per_item) return;

    // ---- the scores along the path: thread t takes pairs t, t + 256, ... in order, then a fixed tree
    float sq = 0.f, both = 0.f, diff = 0.f;
    if (a.pitch_out) {
        const float* fo = a.pitch_out + (int64_t)b * a.po_sb;
        const float* ft = a.pitch_tgt + (int64_t)b * a.pt_sb;
        for (int k = t; k < K; k += kThreads) {
            const uint32_t v = pth[K - 1 - k];
            const float x = fo[v & 0xffffu], y = ft[v >> 16];
            const bool vx = x > 0.f, vy = y > 0.f;
            if (vx && vy) {
                const float c = 1200.f * log2f(x / y);
                sq = fmaf(c, c, sq);
                both += 1.f;
            }
            diff += vx != vy ? 1.f : 0.f;
        }
        red[0][t] = sq, red[1][t] = both, red[2][t] = diff;
        __syncthreads();
        for (int s = kThreads / 2; s > 0; s >>= 1) {
            if (t < s)
                for (int q = 0; q < 3; ++q) red[q][t] += red[q][t + s];
            __syncthreads();
        }
    }
    if (t == 0) {
        const float fk = (float)K;
        a.per_item[b] = kLogDb * total_s / fk;
        if (a.pitch_out) {
            a.per_item[a.B + b] = red[1][0] > 0.f ? sqrtf(red[0][0] / red[1][0]) : __builtin_nanf("");
            a.per_item[2 * a.B + b] = red[2][0] / fk;
        }
        a.per_item[3 * a.B + b] = (float)n / (float)m;
    }
}

struct MelView {
    const float* p;
    int64_t sb, sc, st;
};

// cep[b][t][k - 1] = mel[b][:, t] . dct[:, k] for k = 1 .. n_mfcc - 1, zero up to kp; blockIdx.z picks the mel
__global__ void __launch_bounds__(kThreads) cepstra_kernel(MelView x, MelView y, const float* __restrict__ dct, float* __restrict__ cx,
                                                           float* __restrict__ cy, int C, int N, int M, int n_mfcc, int kp) {
    __shared__ float fr[kFrames][kMaxC + 1];
    const MelView v = blockIdx.z ? y : x;
    const int T = blockIdx.z ? M : N;
    float* out = blockIdx.z ? cy : cx;
    const int b = blockIdx.y, t0 = blockIdx.x * kFrames;
    if (t0 >= T) return;
    const int nf = min(kFrames, T - t0);
    const float* vb = v.p + (int64_t)b * v.sb;
    if (v.st == 1) {        // frames fastest
        for (int i = threadIdx.x; i < C * kFrames; i += kThreads) {
            const int c = i / kFrames, f = i % kFrames;
            if (f < nf) fr[f][c] = vb[c * v.sc + t0 + f];
        }
    } else {                // channels fastest
        for (int i = threadIdx.x; i < C * kFrames; i += kThreads) {
            const int f = i / C, c = i % C;
            if (f < nf) fr[f][c] = vb[c * v.sc + (int64_t)(t0 + f) * v.st];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nf * kp; i += kThreads) {
        const int f = i / kp, k = 1 + i % kp;
        float acc = 0.f;
        if (k < n_mfcc)
            for (int c = 0; c < C; ++c) acc = fmaf(fr[f][c], dct[c * n_mfcc + k], acc);
        out[((int64_t)b * T + t0 + f) * kp + k - 1] = acc;
    }
}

// c[i][j] = sqrt(sum_k (cx[b][i][k] - cy[b][j][k])^2), k ascending, written straight into the skewed layout (and row-major into
// cost_out when given): a tile of 64 rows i x 64 layout rows d = j + i / R per workgroup, thread t takes row i0 + t % 64 at 16 d's.
__global__ void __launch_bounds__(kThreads) cost_kernel(const float* __restrict__ cx, const float* __restrict__ cy,
                                                        const int64_t* __restrict__ n_len, const int64_t* __restrict__ m_len,
                                                        float* __restrict__ skew, int64_t skew_item, float* __restrict__ cost_out,
                                                        int N, int M, int kp) {
    __shared__ float as[kTile][kKc + 1], bs[2 * kTile][kKc + 1];
    const int b = blockIdx.z, i0 = blockIdx.y * kTile, d0 = blockIdx.x * kTile;
    const int64_t nl = n_len[b], ml = m_len[b];
    if (nl < 1 || nl > N || ml < 1 || ml > M || i0 >= nl) return;
    const int n = (int)nl, m = (int)ml, R = rows_per_lane(n);
    const int jbase = d0 - (i0 + kTile - 1) / R;             // the tile's columns: jbase .. d0 + 63 - i0 / R (at most 127)
    if (jbase >= m || d0 + kTile - 1 - i0 / R < 0) return;
    const int il = threadIdx.x % kTile, dl = threadIdx.x / kTile, i = i0 + il;
    const int jl = dl - i / R - jbase + d0;                  // this thread's first column, relative to jbase; then + 4 per q
    float acc[16] = {};
    for (int kc = 0; kc < kp; kc += kKc) {
        for (int e = threadIdx.x; e < 3 * kTile * kKc; e += kThreads) {
            const int r = e / kKc, k = e % kKc;
            const bool kin = kc + k < kp;
            if (r < kTile) {
                as[r][k] = (kin && i0 + r < N) ? cx[((int64_t)b * N + i0 + r) * kp + kc + k] : 0.f;
            } else {
                const int j = jbase + r - kTile;
                bs[r - kTile][k] = (kin && j >= 0 && j < M) ? cy[((int64_t)b * M + j) * kp + kc + k] : 0.f;
            }
        }
        __syncthreads();
        for (int k = 0; k < kKc; ++k) {
            const float av = as[il][k];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float d = av - bs[jl + 4 * q][k];
                acc[q] = fmaf(d, d, acc[q]);
            }
        }
        __syncthreads();
    }
    float* sk = skew + (int64_t)b * skew_item;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int d = d0 + dl + 4 * q, j = d - i / R;
        if (i < n && j >= 0 && j < m) {
            const float v = sqrtf(acc[q]);
            sk[(int64_t)d * (kThreads * R) + i] = v;
            if (cost_out) cost_out[((int64_t)b * N + i) * M + j] = v;
        }
    }
}

// A row-major cost matrix into the skewed layout: the same tiles; a thread walks along one row of the matrix, so the 64 rows
// of a tile stay in the L1 while their lines are used up, and the writes are 256-byte runs.
__global__ void __launch_bounds__(kThreads) skew_kernel(const float* __restrict__ cost, int64_t sb, int64_t sn,
                                                        const int64_t* __restrict__ n_len, const int64_t* __restrict__ m_len,
                                                        float* __restrict__ skew, int64_t skew_item, int N, int M) {
    const int b = blockIdx.z, i = blockIdx.y * kTile + threadIdx.x % kTile;
    const int64_t nl = n_len[b], ml = m_len[b];
    if (nl < 1 || nl > N || ml < 1 || ml > M || i >= nl) return;
    const int m = (int)ml, R = rows_per_lane((int)nl);
    const float* row = cost + (int64_t)b * sb + (int64_t)i * sn;
    float* sk = skew + (int64_t)b * skew_item;
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
        const int d = blockIdx.x * kTile + threadIdx.x / kTile + 4 * q, j = d - i / R;
        if (j >= 0 && j < m) sk[(int64_t)d * (kThreads * R) + i] = row[j];
    }
}

// means[q] = mean_b per_item[q][b]: per thread b = t, t + 256, ... in order, then a fixed tree
__global__ void __launch_bounds__(kThreads) dtw_means_kernel(const float* __restrict__ per_item, float* __restrict__ means, int B,
                                                             bool pitch) {
    __shared__ float red[4][kThreads];
    const int t = threadIdx.x;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = t; b < B; b += kThreads)
        for (int q = 0; q < 4; ++q)
            if (pitch || q == 0 || q == 3) s[q] += per_item[(int64_t)q * B + b];
    for (int q = 0; q < 4; ++q) red[q][t] = s[q];
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w)
            for (int q = 0; q < 4; ++q) red[q][t] += red[q][t + w];
        __syncthreads();
    }
    if (t < 4 && (pitch || t == 0 || t == 3)) means[t] = red[t][0] / (float)B;
}

}  // namespace

extern "C" int32_t ispk_dtw_f32(const float* cost, int64_t cost_sb, int64_t cost_sn, const int64_t* n_len, const int64_t* m_len,
                                float* total, int32_t* steps, int16_t* path, float* workspace, int64_t workspace_floats,
                                int32_t B, int32_t N, int32_t M, ispk_stream_t stream) {
    ISPK_REQUIRE(cost && n_len && m_len && total && steps && workspace, ISPK_E_NULL, "ispk_dtw_f32: null pointer");
    ISPK_REQUIRE(B >= 0 && B <= 65535, ISPK_E_SHAPE, "ispk_dtw_f32: bad shape B=%d", B);
    ISPK_REQUIRE(N >= 1 && N <= kMaxLen && M >= 1 && M <= kMaxLen, ISPK_E_SHAPE,
                 "ispk_dtw_f32: need 1 <= N, M <= %d (N=%d M=%d)", kMaxLen, N, M);
    ISPK_REQUIRE(ispk_aligned(workspace, 16), ISPK_E_ALIGN, "ispk_dtw_f32: the workspace must be 16-byte aligned");
    if (B == 0) return 0;
    const int64_t item = bp_words(N, M), sk_item = skew_floats(N, M), need = (int64_t)B * (item + sk_item);
    ISPK_REQUIRE(workspace_floats >= need, ISPK_E_ALIGN, "ispk_dtw_f32: workspace needs %lld floats", (long long)need);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(skew_kernel, dim3((M + kThreads - 1 + kTile - 1) / kTile, (N + kTile - 1) / kTile, B), dim3(kThreads), 0, s,
                       cost, cost_sb, cost_sn, n_len, m_len, workspace, sk_item, N, M);
    DtwArgs a{workspace, sk_item, n_len, m_len, total, steps, path, reinterpret_cast<uint32_t*>(workspace + B * sk_item), item,
              nullptr, nullptr, 0, 0, nullptr, B, N, M};
    hipLaunchKernelGGL(dtw_kernel, dim3(B), dim3(kThreads), 0, s, a);
    return ispk_launch_status();
}

extern "C" int32_t ispk_mcd_dtw_f32(const float* mel_out, int64_t out_sb, int64_t out_sc, int64_t out_st, const float* mel_target,
                                    int64_t tgt_sb, int64_t tgt_sc, int64_t tgt_st, const float* dct, const int64_t* n_len,
                                    const int64_t* m_len, const float* pitch_out, int64_t pitch_out_sb, const float* pitch_target,
                                    int64_t pitch_target_sb, float* workspace, int64_t workspace_floats, float* per_item,
                                    float* means, float* cost_out, int32_t B, int32_t C, int32_t N, int32_t M, int32_t n_mfcc,
                                    ispk_stream_t stream) {
    ISPK_REQUIRE(mel_out && mel_target && dct && n_len && m_len && workspace && per_item && means, ISPK_E_NULL,
                 "ispk_mcd_dtw_f32: null pointer");
    ISPK_REQUIRE((pitch_out != nullptr) == (pitch_target != nullptr), ISPK_E_NULL,
                 "ispk_mcd_dtw_f32: null pitch pointer (give both tracks or neither)");
    ISPK_REQUIRE(B >= 0 && B <= 65535, ISPK_E_SHAPE, "ispk_mcd_dtw_f32: bad shape B=%d", B);
    ISPK_REQUIRE(N >= 1 && N <= kMaxLen && M >= 1 && M <= kMaxLen, ISPK_E_SHAPE,
                 "ispk_mcd_dtw_f32: need 1 <= N, M <= %d (N=%d M=%d)", kMaxLen, N, M);
    ISPK_REQUIRE(C >= 1 && C <= kMaxC && n_mfcc >= 1 && n_mfcc <= C, ISPK_E_SHAPE,
                 "ispk_mcd_dtw_f32: need 1 <= n_mfcc <= C <= %d (C=%d n_mfcc=%d)", kMaxC, C, n_mfcc);
    ISPK_REQUIRE(ispk_aligned(workspace, 16), ISPK_E_ALIGN, "ispk_mcd_dtw_f32: the workspace must be 16-byte aligned");
    if (B == 0) return 0;
    const int kp = (n_mfcc - 1 + 3) / 4 * 4;
    const int64_t item = bp_words(N, M), sk_item = skew_floats(N, M);
    const int64_t n_sk = (int64_t)B * sk_item, n_cx = (int64_t)B * N * kp, n_cy = (int64_t)B * M * kp;
    const int64_t need = n_sk + n_cx + n_cy + 2 * (int64_t)B + (int64_t)B * item;
    ISPK_REQUIRE(workspace_floats >= need, ISPK_E_ALIGN, "ispk_mcd_dtw_f32: workspace needs %lld floats", (long long)need);
    float* skew = workspace;
    float* cx = skew + n_sk;
    float* cy = cx + n_cx;
    float* total = cy + n_cy;
    int32_t* steps = reinterpret_cast<int32_t*>(total + B);
    uint32_t* bp = reinterpret_cast<uint32_t*>(total + 2 * (int64_t)B);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (kp > 0) {
        const int nch = (max(N, M) + kFrames - 1) / kFrames;
        hipLaunchKernelGGL(cepstra_kernel, dim3(nch, B, 2), dim3(kThreads), 0, s, MelView{mel_out, out_sb, out_sc, out_st},
                           MelView{mel_target, tgt_sb, tgt_sc, tgt_st}, dct, cx, cy, C, N, M, n_mfcc, kp);
    }
    hipLaunchKernelGGL(cost_kernel, dim3((M + kThreads - 1 + kTile - 1) / kTile, (N + kTile - 1) / kTile, B), dim3(kThreads), 0, s,
                       cx, cy, n_len, m_len, skew, sk_item, cost_out, N, M, kp);
    DtwArgs a{skew, sk_item, n_len, m_len, total, steps, nullptr, bp, item,
              pitch_out, pitch_target, pitch_out_sb, pitch_target_sb, per_item, B, N, M};
    hipLaunchKernelGGL(dtw_kernel, dim3(B), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(dtw_means_kernel, dim3(1), dim3(kThreads), 0, s, per_item, means, B, pitch_out != nullptr);
    return ispk_launch_status();
}
