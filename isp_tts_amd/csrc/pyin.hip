// PitchTracker (isp_tts_amd/data/pitch.py; no counterpart in the reference, whose only pitch is torch-yin): probabilistic YIN
// (Mauch & Dixon 2014, as librosa.pyin states it) in two stages.  include/ispk.h has the definition.
//
//   pyin_observe_kernel  grid (ceil(M / 8), B), 512 threads = two halves of 256, one frame per half, frames in pairs (the
//                        layout of features_kernel).  A workgroup stages the 3,840 samples of its 8 frames once (frame t
//                        starts at item sample 256 t - 384, zeros outside [0, n)).  Per frame:
//                          cross-correlation  c(tau) = sum_{j<1024} x[j] x[j+tau] as irfft(conj(rfft(first half, zero-padded))
//                                             rfft(frame)) with 2,048 points (j + tau < 2048: nothing wraps) = three
//                                             1,024-point complex transforms of fft.h in fp32 (two half-length splits forward,
//                                             one back);
//                          energies           the inclusive prefix sums of x^2 in float64 (chunks of 8 per lane, a shuffle scan
//                                             per wave, the four waves in order);
//                          d, cmnd            d(tau) = (S[1023] + (S[tau+1023] - S[tau-1])) - 2 c(tau) in float64, four lags
//                                             per lane in registers, the running sum by the same scan, cmnd = d / (sum / tau
//                                             + tiny);
//                          troughs            flags from the neighbours, compacted in lag order by a count scan (at most 511:
//                                             two troughs are never adjacent); per trough the parabolic shift, the bin, the
//                                             first threshold above its height (s_j) and the lowest trough by a (height,
//                                             position) min-reduction;
//                          probabilities      the rank of trough j among the troughs below threshold s is the number of
//                                             earlier troughs with s_j' <= s: per threshold a bit mask over the troughs that
//                                             BEGIN at it (wave ballots, no atomics) and its popcount prefix per 64-trough word,
//                                             so lane j walks s = 0 .. 99 once, adds the count of earlier troughs beginning at
//                                             s, and from s_j on adds prior[s] e2[k] inv[N_s] in ascending s, in float64;
//                          row                bins fall as lags rise, so the troughs of one bin are neighbours in the list and
//                                             the last of each run writes the LDS row, which goes out with unit stride.
//                        LDS: twiddles 16 KB + samples 15 KB + 2 x 32 KB + the prior table 10.4 KB = 107,888 B dynamic, one
//                        workgroup per CU (8 waves).
//   pyin_decode_kernel   grid (B), 512 threads; one workgroup owns an item and its scores stay in LDS.  A first pass (prob
//                        input only) gives every frame its voiced sum, one wave per frame, into the workspace.  Then per frame
//                        lane b scans the 2 h + 1 voiced and the 2 h + 1 unvoiced predecessors of bin b in ascending order
//                        (first maximum wins; the arrays carry h entries of -inf on either side, so the loop has no bounds
//                        test) and forms both targets of bin b from the two block maxima: the banded maximum of 2 x width
//                        predecessors serves two states.  One barrier per frame (scores are double-buffered), one
//                        backpointer byte per (frame, state): voiced / unvoiced source times the offset in the band.  The
//                        last frame leaves the raw scores; a (value, lowest index) max-reduction picks the end, lane 0 walks
//                        back, then all lanes write f0, flags and the normalised contour.
// Every sum and maximum runs in a fixed order, there are no atomics and no host reads: an item's results depend on that item
// alone and repeat bit for bit, and both entries can be captured in a graph.
//
// gfx950 resources (csrc/resource_report.py pyin.hip; no spills, no scratch):
//   pyin_observe_kernel  169 VGPRs, LDS 107,888 B dynamic + 192 B static (one workgroup of 8 waves per CU)
//   pyin_decode_kernel   87 VGPRs, LDS 46,176 B static
#include <float.h>
#include <math.h>

#include <algorithm>

#include "common.h"
#include "fft.h"

namespace {

constexpr int kPyFrames = 8;                        // frames per workgroup of the observation (even: frames run in pairs)
constexpr int kPyHop = 256;
constexpr int kPyPadL = 384;                        // frame t starts at item sample 256 t + 128 - 512
constexpr int kPyWin = 1024;                        // the YIN window: the first half of a frame
constexpr int kPyFrame = 2048;
constexpr int kPyThreads = 512;
constexpr int kPyHalf = 256;                        // threads per frame
constexpr int kPyTw = 2048;                         // twiddle table: W_2048^m, m < 2048 (data.features.twiddles())
constexpr int kPyStage = (kPyFrames - 1) * kPyHop + kPyFrame;    // 3,840 samples per workgroup
constexpr int kPyMaxPeriod = 1022;                  // tau + 1023 < 2047 and tau < 4 * 256
constexpr int kPyMaxBins = ISPK_PYIN_MAX_BINS;
constexpr int kPyThr = ISPK_PYIN_THRESHOLDS;
constexpr int kPyMaxTroughs = 512;
constexpr int kPyWords = kPyMaxTroughs / 64;
constexpr int kPyRegion = 32768;                    // LDS bytes of one half
constexpr double kPyNoTrough = 0.01;
// the host table (data.pitch.observation_table): thresholds, their prior, its running sum, the Boltzmann pieces
constexpr int kPyTabThr = 0, kPyTabPrior = kPyThr, kPyTabCum = 2 * kPyThr, kPyTabE2 = 3 * kPyThr + 1,
              kPyTabInv = kPyTabE2 + kPyMaxTroughs;
static_assert(kPyTabInv + kPyMaxTroughs + 1 == ISPK_PYIN_TABLE_DOUBLES, "include/ispk.h quotes the table's size");
constexpr size_t kPyObsLds = sizeof(cf) * kPyTw + 2 * kPyRegion + sizeof(float) * kPyStage + sizeof(double) * ISPK_PYIN_TABLE_DOUBLES;
static_assert(kPyObsLds == 107888 && kPyObsLds <= 160 * 1024, "the header above and DESIGN.md 4.34 quote this");

constexpr int kDecThreads = 512;
constexpr int kDecMaxHalf = 63;                     // h: 2 (2 h + 1) backpointer codes fit a byte
constexpr int kDecRow = kPyMaxBins + 2 * kDecMaxHalf + 2;        // one block of scores with its -inf margins

struct ObsArgs {
    const int64_t* audio_len;
    const double* table;
    float* obs;
    int64_t* frames;
    int S, M, NB, min_period, max_period;
    double sample_rate, f_min, bins_per_octave;
};

// Inclusive scan over the 256 lanes of one half of kN consecutive values per lane, in registers: the lane's own running sums,
// a shuffle scan of the lane totals per wave, the wave totals in order.  Fixed order.  Ends with a barrier.
template <int kN>
__device__ __forceinline__ void scan_chunks(double (&v)[kN], int lt, double* wsum) {
    const int lane = lt % kWave, hw = lt / kWave;
#pragma unroll
    for (int q = 1; q < kN; ++q) v[q] += v[q - 1];
    double x = v[kN - 1];
    for (int o = 1; o < kWave; o <<= 1) {
        const double y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == kWave - 1) wsum[hw] = x;
    __syncthreads();
    double off = x - v[kN - 1];
    for (int w = 0; w < hw; ++w) off += wsum[w];
#pragma unroll
    for (int q = 0; q < kN; ++q) v[q] += off;
    __syncthreads();
}

__global__ void __launch_bounds__(kPyThreads) pyin_observe_kernel(const float* __restrict__ audio, int64_t ld,
                                                                  const float* __restrict__ tables, ObsArgs a) {
    extern __shared__ float4 lds_raw[];
    cf* tw = reinterpret_cast<cf*>(lds_raw);                                        // [kPyTw]
    char* regions = reinterpret_cast<char*>(tw + kPyTw);                            // [2 halves][kPyRegion]
    float* smp = reinterpret_cast<float*>(regions + 2 * kPyRegion);                 // [kPyStage]
    double* tb = reinterpret_cast<double*>(smp + kPyStage);                         // [ISPK_PYIN_TABLE_DOUBLES]
    __shared__ double wsum[2][4];
    __shared__ double wmin_h[2][4];
    __shared__ int wmin_j[2][4];
    __shared__ int wcnt[2][4];

    const int b = blockIdx.y, t0 = blockIdx.x * kPyFrames;
    const int tid = threadIdx.x, h = tid / kPyHalf, lt = tid % kPyHalf;
    const int lane = lt % kWave, hw = lt / kWave;

    // ---- lengths (device data: out of range -> no frames), as ispk_audio_features_f32 counts them
    const int64_t L64 = a.audio_len[b];
    const bool ok = L64 >= kPyHop && L64 <= a.S;
    const int L = ok ? (int)L64 : 0;
    const int n_frames = ok ? (L - kPyHop) / kPyHop + 1 : 0;
    if (blockIdx.x == 0 && tid == 0 && a.frames) a.frames[b] = n_frames;
    const int nvalid = max(0, min(kPyFrames, min(n_frames, a.M) - t0));
    const int NB = a.NB;
    float* orow = a.obs + ((int64_t)b * a.M + t0) * NB;

    if (nvalid > 0) {
        for (int i = tid; i < kPyTw; i += kPyThreads) tw[i] = reinterpret_cast<const cf*>(tables)[i];
        for (int i = tid; i < ISPK_PYIN_TABLE_DOUBLES; i += kPyThreads) tb[i] = a.table[i];
        const float* row = audio + (int64_t)b * ld;
        const int a0 = t0 * kPyHop - kPyPadL;
        for (int i = tid; i < kPyStage; i += kPyThreads) {
            const int s = a0 + i;
            smp[i] = (s >= 0 && s < L) ? row[s] : 0.f;
        }
        __syncthreads();

        char* reg = regions + h * kPyRegion;
        cf* A = reinterpret_cast<cf*>(reg);                          // ping; then cmnd, float64 [1024]
        cf* C = reinterpret_cast<cf*>(reg + 8192);                   // ping, then 1024 c; then the masks and their prefixes
        cf* Bf = reinterpret_cast<cf*>(reg + 16384);                 // the frame's spectrum; with D the energy prefix sums;
        cf* D = reinterpret_cast<cf*>(reg + 24576);                  // the window's spectrum; then the lists (Bf) and the row (D)
        double* Y = reinterpret_cast<double*>(reg);
        const float* cfl = reinterpret_cast<const float*>(C);
        unsigned long long* mask = reinterpret_cast<unsigned long long*>(reg + 8192);     // [kPyThr][kPyWords]
        uint16_t* wpre = reinterpret_cast<uint16_t*>(reg + 8192 + 8 * kPyThr * kPyWords);  // [kPyThr][kPyWords]
        double* Sq = reinterpret_cast<double*>(reg + 16384);         // [2048]
        uint8_t* l_s = reinterpret_cast<uint8_t*>(reg + 16384);      // [512] first threshold above the trough (100: none)
        int16_t* l_bin = reinterpret_cast<int16_t*>(reg + 16384 + 512);    // [512]
        float* l_p = reinterpret_cast<float*>(reg + 16384 + 1536);   // [512]
        float* rowp = reinterpret_cast<float*>(reg + 24576);         // [kPyMaxBins]
        int* tot = reinterpret_cast<int*>(reg + 24576 + 4096);       // [kPyThr] troughs beginning at s, then N_s
        int* ncum = tot + kPyThr;                                    // [kPyThr]

        const int n_lag = a.max_period - a.min_period + 1;

        for (int p = 0; 2 * p < nvalid; ++p) {
            const int f = 2 * p + h;                 // this half's frame in the block (f >= nvalid: computed, not kept)
            const float* x = smp + f * kPyHop;
            // ---- the two forward transforms: the frame, and its first half zero-padded
            for (int n = lt; n < 1024; n += kPyHalf) {
                const cf v = make_float2(x[2 * n], x[2 * n + 1]);
                A[n] = v;
                C[n] = n < kPyWin / 2 ? v : make_float2(0.f, 0.f);
            }
            __syncthreads();
            fft<false, kPyHalf, kPyTw>(A, Bf, 1024, lt, tw);
            fft<false, kPyHalf, kPyTw>(C, D, 1024, lt, tw);
            // ---- P_k = conj(W_k) X_k, k <= 1024 (Hermitian), as the half-length inverse's input Z_k = E_k + i O_k
            for (int k = lt; k < 1024; k += kPyHalf) {
                const int m = 1024 - k;
                const cf xk = real_split(Bf, k, 1024, tw[k]), wk = real_split(D, k, 1024, tw[k]);
                const cf xm = real_split(Bf, m, 1024, tw[m]), wm = real_split(D, m, 1024, tw[m]);
                const cf pk = make_float2(wk.x * xk.x + wk.y * xk.y, wk.x * xk.y - wk.y * xk.x);
                const cf pm = make_float2(wm.x * xm.x + wm.y * xm.y, wm.x * xm.y - wm.y * xm.x);
                // P_{k+1024} = conj(P_{1024-k})
                const cf e = make_float2(0.5f * (pk.x + pm.x), 0.5f * (pk.y - pm.y));
                const cf od = make_float2(0.5f * (pk.x - pm.x), 0.5f * (pk.y + pm.y));
                const cf o = ctw<true>(od, tw[k]);
                A[k] = make_float2(e.x - o.y, e.y + o.x);
            }
            __syncthreads();
            fft<true, kPyHalf, kPyTw>(A, C, 1024, lt, tw);           // C[n] = 1024 (c[2n] + i c[2n+1])
            // ---- energies: S[i] = sum_{j<=i} x[j]^2 in float64
            {
                double v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const double s = (double)x[8 * lt + q];
                    v[q] = s * s;
                }
                scan_chunks<8>(v, lt, wsum[h]);
#pragma unroll
                for (int q = 0; q < 8; ++q) Sq[8 * lt + q] = v[q];
            }
            __syncthreads();
            // ---- difference function, its running sum, cmnd: lags 4 lt .. 4 lt + 3
            {
                double d[4], keep[4];
                const double e0 = Sq[kPyWin - 1];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int tau = 4 * lt + q;
                    double v = 0.0;
                    if (tau >= 1 && tau <= a.max_period)
                        v = (e0 + (Sq[tau + kPyWin - 1] - Sq[tau - 1])) - 2.0 * ((double)cfl[tau] * (1.0 / 1024.0));
                    d[q] = keep[q] = v;
                }
                scan_chunks<4>(d, lt, wsum[h]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int tau = 4 * lt + q;
                    Y[tau] = tau >= 1 && tau <= a.max_period ? keep[q] / (d[q] / (double)tau + DBL_MIN) : 0.0;
                }
            }
            for (int i = lt; i < NB; i += kPyHalf) rowp[i] = 0.f;
            __syncthreads();
            // ---- troughs of y[i] = cmnd[min_period + i], i < n_lag, in lag order
            int T;
            {
                bool is[4];
                int cnt = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = 4 * lt + q - a.min_period;
                    bool t = false;
                    if (i >= 0 && i < n_lag - 1) {
                        const double y0 = Y[a.min_period + i], y1 = Y[a.min_period + i + 1];
                        t = i == 0 ? y0 < y1 : (y0 < Y[a.min_period + i - 1] && y0 <= y1);
                    }
                    is[q] = t;
                    cnt += t;
                }
                int xs = cnt;
                for (int o = 1; o < kWave; o <<= 1) {
                    const int y = __shfl_up(xs, o);
                    if (lane >= o) xs += y;
                }
                if (lane == kWave - 1) wcnt[h][hw] = xs;
                __syncthreads();
                int pos = xs - cnt;
                for (int w = 0; w < hw; ++w) pos += wcnt[h][w];
                T = min(kPyMaxTroughs, wcnt[h][0] + wcnt[h][1] + wcnt[h][2] + wcnt[h][3]);
                double best_h = INFINITY;
                int best_j = kPyMaxTroughs;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (!is[q] || pos >= kPyMaxTroughs) continue;
                    const int i = 4 * lt + q - a.min_period;
                    const double y0 = Y[a.min_period + i];
                    double shift = 0.0;
                    if (i > 0) {
                        const double ym = Y[a.min_period + i - 1], yp = Y[a.min_period + i + 1];
                        const double ca = yp + ym - 2.0 * y0, cb = (yp - ym) / 2.0;
                        if (fabs(cb) < fabs(ca)) shift = -cb / ca;
                    }
                    const double f0 = a.sample_rate / ((double)(a.min_period + i) + shift);
                    const double v = rint(a.bins_per_octave * log2(f0 / a.f_min));
                    l_bin[pos] = (int16_t)(int)fmin(fmax(v, 0.0), (double)(NB - 1));
                    int s = min(kPyThr, max(0, (int)(y0 * 100.0) - 1));
                    while (s < kPyThr && tb[kPyTabThr + s] <= y0) ++s;
                    l_s[pos] = (uint8_t)s;
                    if (y0 < best_h) best_h = y0, best_j = pos;      // (ascending positions: the first of equal heights stays)
                    ++pos;
                }
                // the lowest trough, the first among equals
                for (int o = kWave / 2; o > 0; o >>= 1) {
                    const double oh = __shfl_xor(best_h, o);
                    const int oj = __shfl_xor(best_j, o);
                    if (oh < best_h || (oh == best_h && oj < best_j)) best_h = oh, best_j = oj;
                }
                if (lane == 0) wmin_h[h][hw] = best_h, wmin_j[h][hw] = best_j;
            }
            __syncthreads();
            int gmin = kPyMaxTroughs;
            {
                double gh = INFINITY;
                for (int w = 0; w < 4; ++w)
                    if (wmin_h[h][w] < gh || (wmin_h[h][w] == gh && wmin_j[h][w] < gmin)) gh = wmin_h[h][w], gmin = wmin_j[h][w];
            }
            const int nwords = (T + 63) / 64;
            // ---- per threshold the troughs that begin at it: wave hw makes words hw and hw + 4; lane l keeps s = l and 64 + l
            for (int w = hw; w < nwords; w += 4) {
                const int j = 64 * w + lane;
                const int my = j < T ? l_s[j] : 255;
                unsigned long long m0 = 0, m1 = 0;
                for (int s = 0; s < kPyThr; ++s) {
                    const unsigned long long m = __ballot(my == s);
                    if (lane == (s & 63)) (s < 64 ? m0 : m1) = m;
                }
                mask[lane * kPyWords + w] = m0;
                if (lane + 64 < kPyThr) mask[(lane + 64) * kPyWords + w] = m1;
            }
            __syncthreads();
            if (lt < kPyThr) {
                int run = 0;
                for (int w = 0; w < nwords; ++w) {
                    wpre[lt * kPyWords + w] = (uint16_t)run;
                    run += __popcll(mask[lt * kPyWords + w]);
                }
                tot[lt] = run;
            }
            __syncthreads();
            if (lt < kPyThr) {
                int run = 0;
                for (int s = 0; s <= lt; ++s) run += tot[s];
                ncum[lt] = run;                      // N_s: the troughs below threshold s
            }
            __syncthreads();
            // ---- the probability of trough j
            for (int j = lt; j < T; j += kPyHalf) {
                const int w = j / 64, sj = l_s[j];
                const unsigned long long below = (1ull << (j % 64)) - 1ull;
                int k = 0;
                double acc = 0.0;
                for (int s = 0; s < kPyThr; ++s) {
                    k += wpre[s * kPyWords + w] + __popcll(mask[s * kPyWords + w] & below);
                    if (s >= sj) acc += tb[kPyTabPrior + s] * tb[kPyTabE2 + k] * tb[kPyTabInv + ncum[s]];
                }
                if (j == gmin) acc += kPyNoTrough * tb[kPyTabCum + sj];
                l_p[j] = (float)acc;
            }
            __syncthreads();
            for (int j = lt; j < T; j += kPyHalf)
                if (j == T - 1 || l_bin[j + 1] != l_bin[j]) rowp[l_bin[j]] = l_p[j];
            __syncthreads();
            if (f < nvalid) {
                float* o = orow + (int64_t)f * NB;
                for (int i = lt; i < NB; i += kPyHalf) o[i] = rowp[i];
            }
            __syncthreads();
        }
    }
    // ---- zero rows past the item's frames
    for (int f = nvalid; f < kPyFrames && t0 + f < a.M; ++f) {
        float* o = orow + (int64_t)f * NB;
        for (int i = tid; i < NB; i += kPyThreads) o[i] = 0.f;
    }
}

struct DecArgs {
    const void* obs;
    const int64_t* obs_len;
    const double* trans;             // logtri [W], lognorm [NB], log stay, log switch, log init
    int32_t* state;
    float* f0;
    int32_t* voiced;
    float* voiced_prob;
    float* pitch;
    int64_t* frames;
    double* log_prob;
    double* ws_sum;                  // [B][M][2]: the voiced probability and the unvoiced log-observation
    uint8_t* ws_bp;                  // [B][M][2 NB]
    int M, NB, W, is_log;
    double f_min, bins_per_octave;
    float mean, std;
};

__global__ void __launch_bounds__(kDecThreads) pyin_decode_kernel(DecArgs a) {
    __shared__ double sc[2][2][kDecRow];             // [buffer][voiced, unvoiced][h margin + NB + margin]
    __shared__ double lnorm[kPyMaxBins];
    __shared__ double ltri[2 * kDecMaxHalf + 1];
    __shared__ double wbest[kDecThreads / kWave];
    __shared__ int wbest_j[kDecThreads / kWave];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid % kWave, wv = tid / kWave;
    const int M = a.M, NB = a.NB, W = a.W, hb = (W - 1) / 2;
    const int n = valid_len(a.obs_len, b, M);
    const double lstay = a.trans[W + NB], lswitch = a.trans[W + NB + 1], linit = a.trans[W + NB + 2];
    const float* pobs = reinterpret_cast<const float*>(a.obs) + (int64_t)b * M * NB;
    const double* lobs = reinterpret_cast<const double*>(a.obs) + (int64_t)b * M * 2 * NB;
    double* wsum = a.ws_sum + (int64_t)b * M * 2;
    uint8_t* bp = a.ws_bp + (int64_t)b * M * 2 * NB;
    int32_t* st = a.state + (int64_t)b * M;

    if (n > 0) {
        for (int i = tid; i < W; i += kDecThreads) ltri[i] = a.trans[i];
        for (int i = tid; i < NB; i += kDecThreads) lnorm[i] = a.trans[W + i];
        for (int i = tid; i < 4 * kDecRow; i += kDecThreads) (&sc[0][0][0])[i] = -INFINITY;
        if (!a.is_log) {
            // ---- voiced sums: one wave per frame, lanes over the bins in ascending order, a butterfly
            for (int t = wv; t < n; t += kDecThreads / kWave) {
                double s = 0.0;
                for (int i = lane; i < NB; i += kWave) s += (double)pobs[(int64_t)t * NB + i];
                for (int o = kWave / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
                if (lane == 0) {
                    const double vp = fmin(fmax(s, 0.0), 1.0);
                    wsum[2 * t] = vp;
                    wsum[2 * t + 1] = log((1.0 - vp) / (double)NB + DBL_MIN);
                }
            }
        }
        __syncthreads();
        // ---- frame 0: the uniform start
        for (int i = tid; i < NB; i += kDecThreads) {
            double ov, ou;
            if (a.is_log) {
                ov = lobs[i], ou = lobs[NB + i];
            } else {
                ov = log((double)fmaxf(pobs[i], 0.f) + DBL_MIN), ou = wsum[1];
            }
            const double dv = linit + ov, du = linit + ou;
            const bool last = n == 1;
            sc[0][0][hb + i] = last ? dv : dv - lnorm[i];
            sc[0][1][hb + i] = last ? du : du - lnorm[i];
        }
        __syncthreads();
        int cur = 0;
        // the next frame's observations are fetched before the banded maximum of this one, so that their latency hides behind it
        constexpr int kPer = kPyMaxBins / kDecThreads;
        float pn[kPer] = {};
        double lvn[kPer] = {}, lun[kPer] = {};
        auto fetch = [&](int t) {
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
                const int i = tid + q * kDecThreads;
                if (i >= NB) continue;
                if (a.is_log) {
                    lvn[q] = lobs[(int64_t)t * 2 * NB + i], lun[q] = lobs[(int64_t)t * 2 * NB + NB + i];
                } else {
                    pn[q] = pobs[(int64_t)t * NB + i], lun[q] = wsum[2 * t + 1];
                }
            }
        };
        if (n > 1) fetch(1);
        for (int t = 1; t < n; ++t) {
            const bool last = t == n - 1;
            float pc[kPer];
            double lvc[kPer], luc[kPer];
#pragma unroll
            for (int q = 0; q < kPer; ++q) pc[q] = pn[q], lvc[q] = lvn[q], luc[q] = lun[q];
            if (!last) fetch(t + 1);
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
                const int i = tid + q * kDecThreads;
                if (i >= NB) continue;
                const double ov = a.is_log ? lvc[q] : log((double)fmaxf(pc[q], 0.f) + DBL_MIN), ou = luc[q];
                // predecessor i - hb + k, k = 0 .. W - 1, sits at sc[..][i + k]; its window reaches bin i at logtri[W - 1 - k]
                const double* pv = &sc[cur][0][i];
                const double* pu = &sc[cur][1][i];
                double bv = -INFINITY, bu = -INFINITY;
                int kv = hb, ku = hb;
#pragma unroll 4
                for (int k = 0; k < W; ++k) {
                    const double lt = ltri[W - 1 - k];
                    const double v = pv[k] + lt, u = pu[k] + lt;
                    if (v > bv) bv = v, kv = k;
                    if (u > bu) bu = u, ku = k;
                }
                // both targets of bin i; a voiced source (the lower state index) wins a tie
                const double vv = bv + lstay, uv = bu + lswitch;
                const double vu = bv + lswitch, uu = bu + lstay;
                const bool tv = uv > vv, tu = uu > vu;
                const double nv = (tv ? uv : vv) + ov, nu = (tu ? uu : vu) + ou;
                bp[(int64_t)t * 2 * NB + i] = (uint8_t)(tv ? W + ku : kv);
                bp[(int64_t)t * 2 * NB + NB + i] = (uint8_t)(tu ? W + ku : kv);
                sc[cur ^ 1][0][hb + i] = last ? nv : nv - lnorm[i];
                sc[cur ^ 1][1][hb + i] = last ? nu : nu - lnorm[i];
            }
            cur ^= 1;
            __syncthreads();
        }
        // ---- the best final state, the lowest index among equals
        double best = -INFINITY;
        int best_j = 2 * NB;
        for (int j = tid; j < 2 * NB; j += kDecThreads) {
            const double v = j < NB ? sc[cur][0][hb + j] : sc[cur][1][hb + j - NB];
            if (v > best || best_j == 2 * NB) best = v, best_j = j;
        }
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const double ov = __shfl_xor(best, o);
            const int oj = __shfl_xor(best_j, o);
            if (oj < 2 * NB && (best_j == 2 * NB || ov > best || (ov == best && oj < best_j))) best = ov, best_j = oj;
        }
        if (lane == 0) wbest[wv] = best, wbest_j[wv] = best_j;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kDecThreads / kWave; ++w) {
                const double ov = wbest[w];
                const int oj = wbest_j[w];
                if (oj < 2 * NB && (best_j == 2 * NB || ov > best || (ov == best && oj < best_j))) best = ov, best_j = oj;
            }
            a.log_prob[b] = best;
            int s = best_j;
            for (int t = n - 1; t >= 1; --t) {
                st[t] = s;
                const int code = bp[(int64_t)t * 2 * NB + s];
                const int u = code >= W, k = code - u * W;
                const int bin = s >= NB ? s - NB : s;
                const int src = min(max(bin - hb + k, 0), NB - 1);
                s = u * NB + src;
            }
            st[0] = s;
        }
        __syncthreads();
    } else if (tid == 0) {
        a.log_prob[b] = 0.0;
    }
    if (tid == 0 && a.frames) a.frames[b] = n;
    // ---- per frame: f0, flags, the normalised contour; zeros (state -1) past the item's frames
    for (int t = tid; t < M; t += kDecThreads) {
        const int64_t o = (int64_t)b * M + t;
        float hz = 0.f, vp = 0.f, norm = 0.f;
        int s = -1, vo = 0;
        if (t < n) {
            s = st[t];
            vo = s < NB;
            if (vo) hz = (float)(a.f_min * exp2((double)s / a.bins_per_octave));
            if (!a.is_log) vp = (float)wsum[2 * t];
            norm = __fdiv_rn(__fsub_rn(hz, a.mean), a.std);
        } else {
            st[t] = -1;
        }
        a.f0[o] = hz;
        a.voiced[o] = vo;
        a.voiced_prob[o] = vp;
        if (a.pitch) a.pitch[o] = norm;
    }
}

int64_t pyin_ws_bytes(int64_t B, int64_t M, int64_t NB) { return 16 * B * M + ((2 * B * M * NB + 7) / 8) * 8; }

}  // namespace

extern "C" int32_t ispk_pyin_frames_per_block(void) { return kPyFrames; }

extern "C" int32_t ispk_pyin_workspace_bytes(int32_t B, int32_t M, int32_t NB, int64_t* bytes) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && M >= 0 && M <= (1 << 22) && NB >= 1 && NB <= kPyMaxBins, ISPK_E_SHAPE,
                 "ispk_pyin_workspace_bytes: bad shape B=%d M=%d NB=%d (B <= 65535, M <= 2^22, 1 <= NB <= %d)", B, M, NB, kPyMaxBins);
    ISPK_REQUIRE(bytes, ISPK_E_NULL, "ispk_pyin_workspace_bytes: null pointer");
    *bytes = pyin_ws_bytes(B, M, NB);
    return 0;
}

extern "C" int32_t ispk_pyin_observe_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables,
                                         const double* prior, float* obs, int64_t* frames, int32_t B, int32_t S, int32_t M,
                                         int32_t NB, int32_t min_period, int32_t max_period, double sample_rate, double f_min,
                                         int32_t bins_per_semitone, ispk_stream_t stream) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= (1 << 30) && ld_audio >= S, ISPK_E_SHAPE,
                 "ispk_pyin_observe_f32: bad shape B=%d S=%d ld=%lld", B, S, (long long)ld_audio);
    const int frames_s = S >= kPyHop ? (S - kPyHop) / kPyHop + 1 : 0;
    ISPK_REQUIRE(M >= frames_s && NB >= 1 && NB <= kPyMaxBins && (int64_t)M * NB <= 0x7fffffff, ISPK_E_SHAPE,
                 "ispk_pyin_observe_f32: M=%d below the %d frames of S=%d, or NB=%d outside [1, %d]", M, frames_s, S, NB, kPyMaxBins);
    ISPK_REQUIRE(min_period >= 1 && max_period <= kPyMaxPeriod && max_period - min_period >= 2, ISPK_E_SHAPE,
                 "ispk_pyin_observe_f32: periods %d .. %d outside 1 <= min, min + 2 <= max <= %d", min_period, max_period,
                 kPyMaxPeriod);
    ISPK_REQUIRE(sample_rate > 0.0 && f_min > 0.0 && bins_per_semitone >= 1 && bins_per_semitone <= 100, ISPK_E_SHAPE,
                 "ispk_pyin_observe_f32: sample_rate %g, f_min %g, bins_per_semitone %d", sample_rate, f_min, bins_per_semitone);
    if (B == 0 || M == 0) return 0;
    ISPK_REQUIRE(audio && audio_len && tables && prior && obs, ISPK_E_NULL, "ispk_pyin_observe_f32: null pointer");
    ISPK_RESERVE_LDS(pyin_observe_kernel, kPyObsLds, "ispk_pyin_observe_f32");
    ObsArgs a;
    a.audio_len = audio_len, a.table = prior, a.obs = obs, a.frames = frames;
    a.S = S, a.M = M, a.NB = NB, a.min_period = min_period, a.max_period = max_period;
    a.sample_rate = sample_rate, a.f_min = f_min, a.bins_per_octave = 12.0 * bins_per_semitone;
    hipLaunchKernelGGL(pyin_observe_kernel, dim3((M + kPyFrames - 1) / kPyFrames, B), dim3(kPyThreads), kPyObsLds,
                       reinterpret_cast<hipStream_t>(stream), audio, ld_audio, tables, a);
    return ispk_launch_status();
}

extern "C" int32_t ispk_pyin_decode_f64(const void* obs, int32_t obs_is_log, const int64_t* obs_len, const double* trans,
                                        int32_t width, double f_min, int32_t bins_per_semitone, float pitch_mean, float pitch_std,
                                        int32_t* state, float* f0, int32_t* voiced, float* voiced_prob, float* pitch,
                                        int64_t* frames, double* log_prob, void* workspace, int64_t workspace_bytes, int32_t B,
                                        int32_t M, int32_t NB, ispk_stream_t stream) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && M >= 0 && M <= (1 << 22) && NB >= 1 && NB <= kPyMaxBins, ISPK_E_SHAPE,
                 "ispk_pyin_decode_f64: bad shape B=%d M=%d NB=%d (B <= 65535, M <= 2^22, 1 <= NB <= %d)", B, M, NB, kPyMaxBins);
    ISPK_REQUIRE(width >= 1 && width % 2 == 1 && width <= 2 * kDecMaxHalf + 1, ISPK_E_SHAPE,
                 "ispk_pyin_decode_f64: width=%d is odd and in [1, %d] (two codes per offset fit one backpointer byte)", width,
                 2 * kDecMaxHalf + 1);
    ISPK_REQUIRE(f_min > 0.0 && bins_per_semitone >= 1 && bins_per_semitone <= 100 && (!pitch || pitch_std != 0.f), ISPK_E_SHAPE,
                 "ispk_pyin_decode_f64: f_min %g, bins_per_semitone %d, pitch std %g", f_min, bins_per_semitone, (double)pitch_std);
    if (B == 0) return 0;
    ISPK_REQUIRE(log_prob, ISPK_E_NULL, "ispk_pyin_decode_f64: null pointer");
    ISPK_REQUIRE(M == 0 || (obs && trans && state && f0 && voiced && voiced_prob && workspace), ISPK_E_NULL,
                 "ispk_pyin_decode_f64: null pointer");
    ISPK_REQUIRE(M == 0 || (workspace_bytes >= pyin_ws_bytes(B, M, NB) && ispk_aligned(workspace, 8)), ISPK_E_ALIGN,
                 "ispk_pyin_decode_f64: the workspace needs %lld bytes at an 8-byte boundary, got %lld",
                 (long long)pyin_ws_bytes(B, M, NB), (long long)workspace_bytes);
    DecArgs a;
    a.obs = obs, a.obs_len = obs_len, a.trans = trans, a.state = state, a.f0 = f0, a.voiced = voiced, a.voiced_prob = voiced_prob;
    a.pitch = pitch, a.frames = frames, a.log_prob = log_prob;
    a.ws_sum = reinterpret_cast<double*>(workspace);
    a.ws_bp = reinterpret_cast<uint8_t*>(workspace) + 16 * (int64_t)B * M;
    a.M = M, a.NB = NB, a.W = width, a.is_log = obs_is_log != 0;
    a.f_min = f_min, a.bins_per_octave = 12.0 * bins_per_semitone, a.mean = pitch_mean, a.std = pitch_std;
    hipLaunchKernelGGL(pyin_decode_kernel, dim3(B), dim3(kDecThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
    return ispk_launch_status();
}
