// Segmenter (no counterpart in the reference, whose recordings arrive as utterances): long recordings cut into utterances at
// their pauses and gathered into a padded batch, on a padded mono batch fp32 [B][S] with int64 audio_len [B] (a length below 0
// or above S counts as 0).  include/ispk.h has the definitions; in short, all integers, `/` floors:
//   Frames      the trim frames of chunk_grid.h, which the conditioner and the noise profile share: hop sums h_t of 256 samples
//               in float64, p_t = (((h_t + h_t+1) + h_t+2) + h_t+3) / 1024 over T = ceil(len / 256) frames, active when p_t > thr.
//   Ends        first / last from the first and last active frames f, l as the conditioner's start / end with pad_frames = pad.
//   Candidates  every maximal inactive run u .. v-1 strictly between f and l of at least min_silence_frames frames:
//               M = 256 ((u + 3 + v) / 2), e = min(256 (u + 3 + pad), M), s = max(256 (v - pad), M).
//   Choice      one greedy pass over the candidates (seg_choose below is the loop of the header, verbatim).
//   Levels      per stored segment the counts and float64 means of p_t over its active / inactive frames.
//   Gather      the stored segments without a dropped flag, in (item, index) order, copied bit for bit into rows.
//
//   hop_sums_kernel    chunk_grid.h's: grid (ceil(S / 8192), B), the hop sums into the item's workspace.  Its staging and the
//                      order of its sums are the header's, so the conditioner's hop sums have the same bits.
//   seg_plan_kernel    grid (B), one workgroup of 1,024 lanes per item (its passes are bound by the latency of one CU's loads:
//                      the more of them in flight, the better).  p_t into the workspace and their max; f and l; then over
//                      [f, l] in chunks of 8,192 frames (8 consecutive frames a lane): an exclusive max-scan hands every lane
//                      the last active frame before its strip, a sum-scan the number of candidates before it, and the lanes
//                      write (e, s) of their candidates in frame order.  Lane 0 runs the choice over the candidates, staged 128
//                      at a time in LDS.  One wave per stored segment sums the levels (lane-strided, then a butterfly: the
//                      order depends on the segment alone).  Slots at or past count are written as zeros.
//   seg_rows_kernel    one workgroup: a thread per item counts its kept segments, an exclusive scan over 256 items at a time
//                      gives the item's first row, the thread writes its rows (item, index, bounds, out_len, row_flags).  The
//                      row table IS the gather's per-row output, so the copy needs no other plan.
//   seg_copy_kernel    grid (ceil(S_out / 4096), R).  Reads its row's (item, start, out_len), copies, zero-fills; 16-byte loads
//                      and stores where the row allows (segment starts are multiples of 256).
// Every sum runs in an order that depends only on the item (never on B or on another item); no atomics, no host read.
#include <algorithm>

#include "chunk_grid.h"

namespace {

constexpr int kSgThreads = 256;                     // seg_rows_kernel: items per round of its scan
constexpr int kSgPlanThreads = 1024;                // the per-item workgroup: one CU's worth of loads in flight
constexpr int kSgStrip = 8;                         // consecutive frames per lane of the candidate pass: chunks of 8,192 frames
constexpr int kSgCandTile = 128;                    // candidates staged in LDS for the choice
constexpr int kSgMaxK = 4096, kSgMaxPad = 1 << 16, kSgMaxRows = 65535;
constexpr int kCpThreads = 256, kCpPer = 16;        // the copy: 4,096 samples per workgroup

struct SegLayout {
    int NH, NC;                                     // hops (and frames) and candidates an item can have
    int64_t per_item;                               // in 8-byte words: hop [NH], p [NH], e [NC], s [NC]
};

SegLayout seg_layout(int S) {
    SegLayout l;
    l.NH = std::max(1, (int)(((int64_t)S + kGridHop - 1) / kGridHop));
    l.NC = l.NH / 5 + 1;                            // a candidate is >= 4 inactive frames behind an active one
    l.per_item = 2 * (int64_t)l.NH + 2 * (int64_t)l.NC;
    return l;
}

struct SegArgs {
    int S, NH, NC, K, ref_mode, pad, msf;
    int64_t per_item, target, max, min;
    double factor, ref;
    double* ws;
    int64_t* segments;
    int32_t *flags, *count, *wanted, *frames, *speech_frames;
    double *speech_power, *noise_power;
};

// The choice's state, held by lane 0.
struct SegChoice {
    int64_t cur, pe, ps;
    bool have;
    int wanted;
};

__device__ __forceinline__ void seg_emit(const SegArgs& a, int b, SegChoice& c, int64_t s, int64_t e) {
    if (c.wanted < a.K) {
        const int64_t o = (int64_t)b * a.K + c.wanted;
        a.segments[2 * o] = s, a.segments[2 * o + 1] = e;
        a.flags[o] = (e - s > a.max ? 1 : 0) | (e - s < a.min ? 2 : 0);
    }
    ++c.wanted;
}

// Boundary j with (e_j, s_j); `virt`: the virtual one, j == n.  A boundary is looked at again after a cut at its predecessor.
__device__ __forceinline__ void seg_choose(const SegArgs& a, int b, SegChoice& c, int64_t ej, int64_t sj, bool virt) {
    for (;;) {
        const int64_t L = ej - c.cur;
        if (L > a.max && c.have) {                                      // the previous pause still fitted: cut there
            seg_emit(a, b, c, c.cur, c.pe);
            c.cur = c.ps, c.have = false;
            continue;
        }
        if (virt || L >= a.target || L > a.max) {
            seg_emit(a, b, c, c.cur, ej);
            c.cur = sj, c.have = false;
        } else {
            c.have = true, c.pe = ej, c.ps = sj;
        }
        return;
    }
}

__global__ __launch_bounds__(kSgPlanThreads) void seg_plan_kernel(const int64_t* __restrict__ audio_len, const SegArgs a) {
    constexpr int kNT = kSgPlanThreads;
    __shared__ double red[kNT];
    __shared__ int ired[2 * kNT];
    __shared__ int64_t ce_s[kSgCandTile], cs_s[kSgCandTile];
    __shared__ int sh_count;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t len = valid_len(audio_len, b, a.S);
    const int T = (int)((len + kGridHop - 1) / kGridHop);
    double* hop = a.ws + (int64_t)b * a.per_item;
    double* pw = hop + a.NH;
    int64_t* ce = reinterpret_cast<int64_t*>(pw + a.NH);
    int64_t* cs = ce + a.NC;

    // frame powers, their max, the threshold
    double mx = 0.0;
    for (int t = tid; t < T; t += 4 * kNT) {                            // four frames a round: their loads go out together
        double p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = t + u * kNT < T ? frame_power(hop, t + u * kNT, T) : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (t + u * kNT < T) {
                pw[t + u * kNT] = p[u];
                mx = fmax(mx, p[u]);
            }
    }
    const double thr = frame_threshold<kNT>(mx, a.ref_mode == 0, a.ref, a.factor, tid, red);

    // the first and last active frames
    int f = 0x7fffffff, l = -1;
#pragma unroll 4
    for (int t = tid; t < T; t += kNT)
        if (pw[t] > thr) {
            f = min(f, t);
            l = max(l, t);
        }
    active_range<kNT>(f, l, tid, ired);

    int count = 0;
    if (l >= 0) {                                                       // (uniform)
        // candidates, compacted in frame order: a run ends at an active frame t whose predecessor is inactive
        int n = 0, carry = -1;                                          // candidates so far; the last active frame before the chunk
        for (int64_t c0 = f; c0 <= l; c0 += (int64_t)kNT * kSgStrip) {
            const int64_t t0 = c0 + (int64_t)tid * kSgStrip;
            uint32_t bits = 0;
            for (int q = 0; q < kSgStrip; ++q)
                if (t0 + q <= l && pw[t0 + q] > thr) bits |= 1u << q;
            int total;
            const int mine = bits ? (int)t0 + 31 - __clz(bits) : -1;
            const int prev = max(carry, block_scan_excl<true, kNT>(mine, -1, tid, ired, total));
            carry = max(carry, total);
            int cnt = 0, pa = prev;
            for (int q = 0; q < kSgStrip; ++q)
                if (bits >> q & 1) {
                    const int t = (int)t0 + q;
                    cnt += t > f && t - (pa + 1) >= a.msf;
                    pa = t;
                }
            int k = n + block_scan_excl<false, kNT>(cnt, 0, tid, ired, total);
            n += total;
            pa = prev;
            for (int q = 0; q < kSgStrip; ++q)
                if (bits >> q & 1) {
                    const int t = (int)t0 + q;
                    if (t > f && t - (pa + 1) >= a.msf) {
                        const int64_t u = pa + 1, v = t;
                        const int64_t M = kGridHop * ((u + 3 + v) / 2);
                        if (k < a.NC) {
                            ce[k] = std::min<int64_t>(kGridHop * (u + 3 + a.pad), M);
                            cs[k] = std::max<int64_t>(kGridHop * (v - a.pad), M);
                        }
                        ++k;
                    }
                    pa = t;
                }
        }
        n = min(n, a.NC);

        // the choice, by lane 0
        SegChoice c;
        c.cur = trim_start(f, a.pad);
        c.pe = c.ps = 0, c.have = false, c.wanted = 0;
        const int64_t last = trim_end(l, a.pad, len);
        for (int j0 = 0; j0 < n; j0 += kSgCandTile) {
            __syncthreads();                                            // the candidates are written; the tile is free
            const int m = min(kSgCandTile, n - j0);
            for (int j = tid; j < m; j += kNT) ce_s[j] = ce[j0 + j], cs_s[j] = cs[j0 + j];
            __syncthreads();
            if (tid == 0)
                for (int j = 0; j < m; ++j) seg_choose(a, b, c, ce_s[j], cs_s[j], false);
        }
        if (tid == 0) {
            seg_choose(a, b, c, last, last, true);
            sh_count = min(c.wanted, a.K);
            a.count[b] = sh_count, a.wanted[b] = c.wanted;
        }
        __syncthreads();                                                // (also: the segments are written)
        count = sh_count;

        // levels: one wave per stored segment
        const int wave = tid / kWave, lane = tid % kWave;
        for (int k = wave; k < count; k += kNT / kWave) {
            const int64_t o = (int64_t)b * a.K + k;
            const int64_t s = a.segments[2 * o], e = a.segments[2 * o + 1];
            const int t0 = (int)((s + kGridHop - 1) / kGridHop), t1 = (int)std::min<int64_t>(T, (e + kGridHop - 1) / kGridHop);
            double sp = 0.0, np = 0.0;
            int ns = 0, ni = 0;
            for (int t = t0 + lane; t < t1; t += kWave) {
                const double p = pw[t];
                if (p > thr) sp += p, ++ns;
                else np += p, ++ni;
            }
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) {
                sp += __shfl_xor(sp, off, kWave);
                np += __shfl_xor(np, off, kWave);
                ns += __shfl_xor(ns, off, kWave);
                ni += __shfl_xor(ni, off, kWave);
            }
            if (lane == 0) {
                a.frames[o] = ns + ni, a.speech_frames[o] = ns;
                a.speech_power[o] = ns ? sp / (double)ns : 0.0;
                a.noise_power[o] = ni ? np / (double)ni : 0.0;
            }
        }
    } else if (tid == 0) {
        a.count[b] = 0, a.wanted[b] = 0;
    }
    for (int k = count + tid; k < a.K; k += kNT) {                      // slots at or past count: zeros
        const int64_t o = (int64_t)b * a.K + k;
        a.segments[2 * o] = 0, a.segments[2 * o + 1] = 0;
        a.flags[o] = 0, a.frames[o] = 0, a.speech_frames[o] = 0;
        a.speech_power[o] = 0.0, a.noise_power[o] = 0.0;
    }
}

// ------------------------------------------------------------------------------------------------------------ gather
struct RowArgs {
    int B, S, K, R, S_out, drop;
    const int64_t* segments;
    const int32_t *flags, *count;
    int64_t *out_len, *bounds;
    int32_t *item, *index, *row_flags, *rows, *rows_wanted;
};

__global__ __launch_bounds__(kSgThreads) void seg_rows_kernel(const RowArgs a) {
    __shared__ int buf[kSgThreads];
    const int tid = threadIdx.x;
    int done = 0;                                                       // kept segments of the items before this chunk
    for (int b0 = 0; b0 < a.B; b0 += kSgThreads) {
        const int b = b0 + tid;
        int n = 0, kept = 0;
        if (b < a.B) {
            n = min(max(a.count[b], 0), a.K);                           // (device data)
#pragma unroll 8
            for (int k = 0; k < n; ++k) kept += !(a.flags[(int64_t)b * a.K + k] & a.drop);
        }
        int total;
        int r = done + block_scan_excl<false, kSgThreads>(kept, 0, tid, buf, total);
        done += total;
        for (int k = 0; k < n && r < a.R; ++k) {
            const int64_t o = (int64_t)b * a.K + k;
            const int fl = a.flags[o];
            if (fl & a.drop) continue;
            int64_t s = a.segments[2 * o], e = a.segments[2 * o + 1];
            if (!(0 <= s && s <= e && e <= a.S)) s = e = 0;             // (device data) a pair outside the row copies nothing
            const int64_t m = std::min<int64_t>(e - s, a.S_out);
            a.out_len[r] = m, a.item[r] = b, a.index[r] = k;
            a.bounds[2 * r] = s, a.bounds[2 * r + 1] = e;
            a.row_flags[r] = fl | (e - s > a.S_out ? 4 : 0);
            ++r;
        }
    }
    const int used = min(done, a.R);
    for (int r = used + tid; r < a.R; r += kSgThreads) {
        a.out_len[r] = 0, a.item[r] = -1, a.index[r] = 0;
        a.bounds[2 * r] = 0, a.bounds[2 * r + 1] = 0;
        a.row_flags[r] = 0;
    }
    if (tid == 0) a.rows[0] = used, a.rows_wanted[0] = done;
}

__global__ __launch_bounds__(kCpThreads) void seg_copy_kernel(const float* __restrict__ audio, int64_t ld, const int32_t* __restrict__ item,
                                                              const int64_t* __restrict__ bounds, const int64_t* __restrict__ out_len,
                                                              float* __restrict__ out, int64_t ld_out, int B, int S, int S_out, int vin,
                                                              int vout) {
    const int r = blockIdx.y;
    const int b = item[r];
    int64_t s = bounds[2 * r], n = out_len[r];
    if (!(0 <= b && b < B && 0 <= s && 0 <= n && n <= S_out && s + n <= S)) s = n = 0;     // (seg_rows_kernel's; checked all the same)
    const float* x = audio + (int64_t)max(b, 0) * ld + s;
    float* o = out + (int64_t)r * ld_out;
    const bool v4 = vin && s % 4 == 0;
    const int64_t i0 = ((int64_t)blockIdx.x * kCpThreads * kCpPer / 4 + threadIdx.x) * 4;
#pragma unroll
    for (int q = 0; q < kCpPer / 4; ++q) {
        const int64_t i = i0 + (int64_t)q * kCpThreads * 4;
        if (i >= S_out) break;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (v4 && i + 4 <= n) {
            v = *reinterpret_cast<const f32x4*>(x + i);
        } else {
            if (i < n) v.x = x[i];
            if (i + 1 < n) v.y = x[i + 1];
            if (i + 2 < n) v.z = x[i + 2];
            if (i + 3 < n) v.w = x[i + 3];
        }
        if (vout && i + 4 <= S_out) {
            *reinterpret_cast<f32x4*>(o + i) = v;
        } else {
            const float e[4] = {v.x, v.y, v.z, v.w};
            for (int k = 0; k < 4 && i + k < S_out; ++k) o[i + k] = e[k];
        }
    }
}

bool seg_overlap(const void* p, int64_t pb, const void* q, int64_t qb) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}

}  // namespace

extern "C" int32_t ispk_segment_workspace_bytes(int32_t B, int32_t S, int64_t* bytes) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0, ISPK_E_SHAPE, "ispk_segment_workspace_bytes: bad shape B=%d S=%d (B <= 65535, 0 <= S < 2^31)",
                 B, S);
    ISPK_REQUIRE(bytes, ISPK_E_NULL, "ispk_segment_workspace_bytes: null pointer");
    *bytes = 8 * (int64_t)B * seg_layout(S).per_item;
    return 0;
}

extern "C" int32_t ispk_segment_plan(const float* audio, int64_t ld_audio, const int64_t* audio_len, double factor, int32_t ref_mode,
                                     double ref, int32_t pad, int32_t min_silence_frames, int64_t target_samples, int64_t max_samples,
                                     int64_t min_samples, int64_t* segments, int32_t* flags, int32_t* count, int32_t* wanted,
                                     int32_t* frames, int32_t* speech_frames, double* speech_power, double* noise_power, void* workspace,
                                     int64_t workspace_bytes, int32_t B, int32_t S, int32_t K, ispk_stream_t stream) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0, ISPK_E_SHAPE, "ispk_segment_plan: bad shape B=%d S=%d (B <= 65535, 0 <= S < 2^31)", B, S);
    ISPK_REQUIRE(K >= 1 && K <= kSgMaxK, ISPK_E_SHAPE, "ispk_segment_plan: K=%d segments per item, 1 .. %d", K, kSgMaxK);
    ISPK_REQUIRE(min_silence_frames >= 4, ISPK_E_SHAPE, "ispk_segment_plan: min_silence_frames %d below 4 (a pause must clear one frame)",
                 min_silence_frames);
    ISPK_REQUIRE(pad >= 0 && pad <= kSgMaxPad, ISPK_E_SHAPE, "ispk_segment_plan: pad %d outside 0 .. %d frames", pad, kSgMaxPad);
    ISPK_REQUIRE(max_samples >= 1 && target_samples >= 0 && min_samples >= 0, ISPK_E_SHAPE,
                 "ispk_segment_plan: bad budget target %lld, max %lld, min %lld samples (max >= 1, the others >= 0)", (long long)target_samples,
                 (long long)max_samples, (long long)min_samples);
    ISPK_REQUIRE((ref_mode == 0 || ref_mode == 1) && factor >= 0.0 && (ref_mode == 0 || ref >= 0.0), ISPK_E_SHAPE,
                 "ispk_segment_plan: bad ref mode %d, factor %g or ref %g", ref_mode, factor, ref);
    if (B == 0) return 0;
    ISPK_REQUIRE(audio && audio_len && segments && flags && count && wanted && frames && speech_frames && speech_power && noise_power &&
                     workspace,
                 ISPK_E_NULL, "ispk_segment_plan: null pointer");
    ISPK_REQUIRE(ld_audio >= S, ISPK_E_SHAPE, "ispk_segment_plan: row stride %lld below S=%d", (long long)ld_audio, S);
    const SegLayout l = seg_layout(S);
    ISPK_REQUIRE(workspace_bytes >= 8 * (int64_t)B * l.per_item && ispk_aligned(workspace, 8), ISPK_E_ALIGN,
                 "ispk_segment_plan: the workspace needs %lld bytes at an 8-byte boundary, got %lld", (long long)(8 * (int64_t)B * l.per_item),
                 (long long)workspace_bytes);
    SegArgs a;
    a.S = S, a.NH = l.NH, a.NC = l.NC, a.K = K, a.ref_mode = ref_mode, a.pad = pad, a.msf = min_silence_frames;
    a.per_item = l.per_item, a.target = target_samples, a.max = max_samples, a.min = min_samples;
    a.factor = factor, a.ref = ref;
    a.ws = reinterpret_cast<double*>(workspace);
    a.segments = segments, a.flags = flags, a.count = count, a.wanted = wanted, a.frames = frames, a.speech_frames = speech_frames;
    a.speech_power = speech_power, a.noise_power = noise_power;
    const int vec = ld_audio % 4 == 0 && ispk_aligned(audio, 16);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned W = (unsigned)(((int64_t)S + kGridSeg - 1) / kGridSeg);
    if (W)
        hipLaunchKernelGGL(hop_sums_kernel<>, dim3(W, B), dim3(kGridThreads), 0, st, audio, ld_audio, audio_len, S, vec, a.ws, a.per_item);
    hipLaunchKernelGGL(seg_plan_kernel, dim3(B), dim3(kSgPlanThreads), 0, st, audio_len, a);
    return ispk_launch_status();
}

extern "C" int32_t ispk_segment_gather_f32(const float* audio, int64_t ld_audio, const int64_t* segments, const int32_t* flags,
                                           const int32_t* count, int32_t drop, float* out, int64_t ld_out, int64_t* out_len, int32_t* item,
                                           int32_t* index, int64_t* bounds, int32_t* row_flags, int32_t* rows, int32_t* rows_wanted,
                                           int32_t B, int32_t S, int32_t K, int32_t R, int32_t S_out, ispk_stream_t stream) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S_out >= 0, ISPK_E_SHAPE,
                 "ispk_segment_gather_f32: bad shape B=%d S=%d S_out=%d (B <= 65535, 0 <= S, S_out < 2^31)", B, S, S_out);
    ISPK_REQUIRE(K >= 1 && K <= kSgMaxK, ISPK_E_SHAPE, "ispk_segment_gather_f32: K=%d segments per item, 1 .. %d", K, kSgMaxK);
    ISPK_REQUIRE(R >= 0 && R <= kSgMaxRows, ISPK_E_SHAPE, "ispk_segment_gather_f32: R=%d rows, 0 .. %d", R, kSgMaxRows);
    ISPK_REQUIRE(drop >= 0 && drop <= 3, ISPK_E_SHAPE, "ispk_segment_gather_f32: drop %d is not a mask of the flags 1 (over) and 2 (short)", drop);
    ISPK_REQUIRE(rows && rows_wanted, ISPK_E_NULL, "ispk_segment_gather_f32: null pointer");
    ISPK_REQUIRE(B == 0 || (audio && segments && flags && count), ISPK_E_NULL, "ispk_segment_gather_f32: null pointer");
    ISPK_REQUIRE(R == 0 || (out_len && item && index && bounds && row_flags && (out || S_out == 0)), ISPK_E_NULL,
                 "ispk_segment_gather_f32: null pointer");
    ISPK_REQUIRE((B == 0 || ld_audio >= S) && ld_out >= S_out, ISPK_E_SHAPE,
                 "ispk_segment_gather_f32: row strides %lld, %lld below S=%d, S_out=%d", (long long)ld_audio, (long long)ld_out, S, S_out);
    ISPK_REQUIRE(B == 0 || R == 0 || S == 0 || S_out == 0 ||
                     !seg_overlap(audio, 4 * ((int64_t)(B - 1) * ld_audio + S), out, 4 * ((int64_t)(R - 1) * ld_out + S_out)),
                 ISPK_E_SHAPE, "ispk_segment_gather_f32: out overlaps audio");
    RowArgs a;
    a.B = B, a.S = S, a.K = K, a.R = R, a.S_out = S_out, a.drop = drop;
    a.segments = segments, a.flags = flags, a.count = count;
    a.out_len = out_len, a.bounds = bounds, a.item = item, a.index = index, a.row_flags = row_flags, a.rows = rows,
    a.rows_wanted = rows_wanted;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(seg_rows_kernel, dim3(1), dim3(kSgThreads), 0, st, a);
    if (R > 0 && S_out > 0) {
        const int vin = ld_audio % 4 == 0 && ispk_aligned(audio, 16), vout = ld_out % 4 == 0 && ispk_aligned(out, 16);
        const int64_t per_block = (int64_t)kCpThreads * kCpPer;
        const unsigned gx = (unsigned)(((int64_t)S_out + per_block - 1) / per_block);
        hipLaunchKernelGGL(seg_copy_kernel, dim3(gx, R), dim3(kCpThreads), 0, st, audio, ld_audio, item, bounds, out_len, out, ld_out, B, S,
                           S_out, vin, vout);
    }
    return ispk_launch_status();
}
