// Equalizer: a cascade of up to eight biquads in float64 on a padded mono batch (no counterpart in the reference, whose audio
// path never changes the spectrum): pre- / de-emphasis around a vocoder, a rumble high-pass in front of the meter, shelves,
// presence peaks and a telephone band.  The stage of the audio chain that changes the spectrum; every other one changes level
// or timing.
//
// Definition.
//   audio fp32 [B][S], unit stride on S, row stride ld_audio >= S.  len = audio_len[b], int64; a length below 0 or above S
//   counts as 0, as everywhere in the audio kernels.  sos float64 [N][5] = (b0, b1, b2, a1, a2) with a0 = 1, 1 <= N <= 8.
//   Each section is transposed direct form II in float64, in the operation order of kw_step (condition.hip):
//       y  = fma(b0, x, s0)
//       s0 = fma(-a1, y, fma(b1, x, s1))
//       s1 = fma(-a2, y, b2 * x)
//   All states are zero at sample 0 of every item; the sections run in order; values between sections stay float64.
//   out[b][i] = fp32(y_N[i]) for i < len, exactly 0 for len <= i < S; out_len[b] = len: the ringing past the end is cut.
//
// The recurrence is linear in its state, so it runs as a chunked scan on a grid fixed to sample 0, as the loudness meter does
// (DESIGN.md 4.16): a chunk is 32 samples = one lane, a segment 256 chunks = 8,192 samples = one workgroup, grid (W, B) with
// W = ceil(S / 8192).  Inside a segment the cascade runs section by section, so the scan only needs 2 x 2 matrices: for a
// section every lane runs its chunk from zero state, a Hillis-Steele scan across the lanes with the host's A_k^(32 2^j),
// j = 0 .. 7, gives every lane its true entry state, the chunk is rerun from it, and the 32 float64 outputs stay in registers
// as the next section's input.  Across segments the carry is the joint 2 N state vector:
//   eq_state_kernel   grid (W - 1, B), not launched when W = 1.  Segment w from zero state: writes its final joint state
//                     (2 N doubles).  A segment at or past len writes nothing; nothing reads it.
//   eq_apply_kernel   grid (W, B).  Folds the states of the segments before it in segment order with the host's joint
//                     A^8192 (2 N x 2 N, row i by lane i), reruns the segment from the true entry state, rounds to fp32 and
//                     stores through LDS: float4 when out's base and row stride allow, scalars otherwise - the same values.
//                     A segment at or past len is written as zeros.
// Every sum and scan runs in an order that is a function of the sample index alone: an item's bits depend on that item, not
// on B, on the row strides or on the alignment; no atomics, no host read, no workgroup waits on another.  A workgroup reads
// only its own segment of audio and stages it in LDS before it stores, and the first launch has read everything it needs
// before the second stores anything: out may be audio itself (same base, same row stride).
//
// LDS: the segment as 256 chunks of 36 floats, staged and read back by chunk_grid.h (the meter's grid; the bank reasoning is
// there).  With the scan's exchange buffer that is 40 KiB a workgroup, four workgroups to a CU; the four spare floats behind chunk k hold the
// entry state of section k, and the kernels are held to 128 registers so that four waves fit a SIMD as well.
#include <math.h>

#include <algorithm>

#include "chunk_grid.h"

namespace {

constexpr int kEqMaxSections = 8;
constexpr int kEqPowers = 8;                        // A_k^(32 2^j), j = 0 .. 7
constexpr int kEqCoef = 8;                          // doubles per section at the head of the table: b0, b1, b2, a1, a2, three unused

// Table, float64: [0, 8 N) the coefficients; [8 N, 40 N) section k's power j as a row-major 2 x 2 at 8 N + 4 (8 k + j);
// [40 N, 40 N + 4 N^2) the joint A^8192, row-major 2 N x 2 N, over the states (s0, s1) of section 0, then section 1, ...
__host__ __device__ constexpr int eq_table_doubles(int n) { return 40 * n + 4 * n * n; }

struct Sos {
    double b0, b1, b2, a1, a2;
};

__device__ __forceinline__ Sos sos_load(const double* __restrict__ tab, int k) {
    const double* c = tab + kEqCoef * k;
    Sos s;
    s.b0 = c[0], s.b1 = c[1], s.b2 = c[2], s.a1 = c[3], s.a2 = c[4];
    return s;
}

// One sample through one section, transposed direct form II; returns the output.
__device__ __forceinline__ double sos_step(const Sos& c, double x, double& s0, double& s1) {
    const double y = fma(c.b0, x, s0);
    s0 = fma(-c.a1, y, fma(c.b1, x, s1));
    s1 = fma(-c.a2, y, c.b2 * x);
    return y;
}

// Inclusive scan over the workgroup's lanes of S_c = A^32 S_(c-1) + v_c (Hillis-Steele, in registers; st is the exchange
// buffer, pw the section's eight 2 x 2 powers: uniform addresses, scalar loads).  Ends with every lane's result also in
// st[.][tid], after a barrier.
__device__ __forceinline__ void eq_scan(double (*st)[kGridThreads], const double* __restrict__ pw, int tid, double& v0, double& v1) {
#pragma unroll 1
    for (int j = 0; j < kEqPowers; ++j) {
        st[0][tid] = v0, st[1][tid] = v1;
        __syncthreads();
        const int src = tid - (1 << j);
        if (src >= 0) {
            const double u0 = st[0][src], u1 = st[1][src];
            const double* P = pw + 4 * j;
            v0 = fma(P[1], u1, fma(P[0], u0, v0));
            v1 = fma(P[3], u1, fma(P[2], u0, v1));
        }
        __syncthreads();
    }
    st[0][tid] = v0, st[1][tid] = v1;
    __syncthreads();
}

// One section over the segment: x holds the lane's 32 inputs and, with `rerun`, its 32 outputs afterwards.  (e0, e1) is the
// section's state at the segment's first sample.  Returns the state behind the segment's last sample in (f0, f1) of the last
// lane.  Ends with a barrier behind the last read of st.
__device__ __forceinline__ void eq_section(const double* __restrict__ tab, int n, int k, double (*st)[kGridThreads], int tid,
                                           double e0, double e1, bool rerun, double x[kGridChunk], double& f0, double& f1) {
    const Sos c = sos_load(tab, k);
    const double* pw = tab + kEqCoef * n + 4 * kEqPowers * k;
    double v0 = 0.0, v1 = 0.0;
#pragma unroll
    for (int i = 0; i < kGridChunk; ++i) sos_step(c, x[i], v0, v1);
    if (tid == 0) {                                                     // the segment's entry state, carried through chunk 0
        v0 = fma(pw[1], e1, fma(pw[0], e0, v0));
        v1 = fma(pw[3], e1, fma(pw[2], e0, v1));
    }
    eq_scan(st, pw, tid, v0, v1);
    f0 = v0, f1 = v1;
    const int p = max(tid - 1, 0);
    double s0 = tid ? st[0][p] : e0, s1 = tid ? st[1][p] : e1;
    __syncthreads();                                                    // (the next section's scan writes st)
    if (rerun) {
#pragma unroll
        for (int i = 0; i < kGridChunk; ++i) x[i] = sos_step(c, x[i], s0, s1);
    }
}

struct EqArgs {
    int64_t ld, ld_out;
    int S, W, n, vec, vec_out;
    double* seg;                                    // [B][W][2 n]: every segment's final joint state from zero entry
};

__global__ __launch_bounds__(kGridThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void eq_state_kernel(const float* __restrict__ audio, const int64_t* __restrict__ audio_len,
                                                                const double* __restrict__ tab, const EqArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[kGridThreads * kGridPad];
    __shared__ double st[2][kGridThreads];
    const int tid = threadIdx.x, w = blockIdx.x, b = blockIdx.y;
    const int64_t len = valid_len(audio_len, b, a.S);
    const int64_t segb = (int64_t)w * kGridSeg;
    if (segb >= len) return;                                            // (uniform) no later segment holds a sample
    stage_chunks(xs, audio + (int64_t)b * a.ld, segb, len, a.vec, tid);
    __syncthreads();
    double x[kGridChunk];
    load_chunk(xs, tid, x);
    double* g = a.seg + ((int64_t)b * a.W + w) * 2 * a.n;
#pragma unroll 1
    for (int k = 0; k < a.n; ++k) {
        double f0, f1;
        eq_section(tab, a.n, k, st, tid, 0.0, 0.0, k + 1 < a.n, x, f0, f1);
        if (tid == kGridThreads - 1) g[2 * k] = f0, g[2 * k + 1] = f1;
    }
}

__global__ __launch_bounds__(kGridThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void eq_apply_kernel(const float* __restrict__ audio, const int64_t* __restrict__ audio_len,
                                                                const double* __restrict__ tab, float* __restrict__ out,
                                                                int64_t* __restrict__ out_len, const EqArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[kGridThreads * kGridPad];
    __shared__ double st[2][kGridThreads];
    const int tid = threadIdx.x, w = blockIdx.x, b = blockIdx.y;
    const int64_t len = valid_len(audio_len, b, a.S);
    const int64_t segb = (int64_t)w * kGridSeg;
    if (w == 0 && tid == 0 && out_len) out_len[b] = len;
    float* xo = xs + tid * kGridPad;
    if (segb < len) {                                                   // (uniform)
        // the joint state at this segment's first sample: E <- A^8192 E + (segment u from zero), u = 0 .. w - 1, row i by lane i,
        // back and forth between the two rows of st; then section k's pair into the four spare floats behind chunk k of xs
        const int n2 = 2 * a.n;
        const double* J = tab + eq_table_doubles(a.n) - n2 * n2;
        if (tid < n2) st[0][tid] = 0.0;
        int cur = 0;
        __syncthreads();
#pragma unroll 1
        for (int u = 0; u < w; ++u) {
            if (tid < n2) {
                double acc = a.seg[((int64_t)b * a.W + u) * n2 + tid];
                for (int j = 0; j < n2; ++j) acc = fma(J[tid * n2 + j], st[cur][j], acc);
                st[cur ^ 1][tid] = acc;
            }
            cur ^= 1;
            __syncthreads();
        }
        if (tid < n2) reinterpret_cast<double*>(xs + (tid >> 1) * kGridPad + kGridChunk)[tid & 1] = st[cur][tid];
        stage_chunks(xs, audio + (int64_t)b * a.ld, segb, len, a.vec, tid);
        __syncthreads();
        double x[kGridChunk];
        load_chunk(xs, tid, x);
#pragma unroll 1
        for (int k = 0; k < a.n; ++k) {
            const double* e = reinterpret_cast<const double*>(xs + k * kGridPad + kGridChunk);
            double f0, f1;
            eq_section(tab, a.n, k, st, tid, e[0], e[1], true, x, f0, f1);
        }
        const int64_t cb = segb + (int64_t)tid * kGridChunk;
#pragma unroll
        for (int k4 = 0; k4 < kGridChunk / 4; ++k4) {
            f32x4 v;
            v.x = cb + 4 * k4 < len ? (float)x[4 * k4] : 0.f;
            v.y = cb + 4 * k4 + 1 < len ? (float)x[4 * k4 + 1] : 0.f;
            v.z = cb + 4 * k4 + 2 < len ? (float)x[4 * k4 + 2] : 0.f;
            v.w = cb + 4 * k4 + 3 < len ? (float)x[4 * k4 + 3] : 0.f;
            *reinterpret_cast<f32x4*>(xo + 4 * k4) = v;                 // (the lane's own chunk: every lane has read its inputs)
        }
    } else {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k4 = 0; k4 < kGridChunk / 4; ++k4) *reinterpret_cast<f32x4*>(xo + 4 * k4) = z;
    }
    __syncthreads();
    float* o = out + (int64_t)b * a.ld_out;
    for (int g = tid; g < kGridSeg / 4; g += kGridThreads) {
        const int64_t i = segb + 4 * (int64_t)g;
        if (i >= a.S) break;
        const f32x4 v = *reinterpret_cast<const f32x4*>(xs + (g >> 3) * kGridPad + (g & 7) * 4);
        if (a.vec_out && i + 4 <= a.S) {
            *reinterpret_cast<f32x4*>(o + i) = v;
        } else {
            o[i] = v.x;
            if (i + 1 < a.S) o[i + 1] = v.y;
            if (i + 2 < a.S) o[i + 2] = v.z;
            if (i + 3 < a.S) o[i + 3] = v.w;
        }
    }
}

}  // namespace

extern "C" int32_t ispk_equalize_segment_samples(void) { return kGridSeg; }

extern "C" int32_t ispk_equalize_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const double* table,
                                     int64_t table_doubles, int32_t sections, float* out, int64_t ld_out, int64_t* out_len,
                                     double* workspace, int64_t workspace_doubles, int32_t B, int32_t S, ispk_stream_t stream) {
    ISPK_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= (1 << 24), ISPK_E_SHAPE,
                 "ispk_equalize_f32: bad shape B=%d S=%d (B <= 65535, S <= 2^24)", B, S);
    ISPK_REQUIRE(sections >= 1 && sections <= kEqMaxSections, ISPK_E_SHAPE, "ispk_equalize_f32: %d sections, expected 1 .. %d",
                 sections, kEqMaxSections);
    if (B == 0) return 0;
    ISPK_REQUIRE(audio && audio_len && table && out && workspace, ISPK_E_NULL, "ispk_equalize_f32: null pointer");
    ISPK_REQUIRE(table_doubles == eq_table_doubles(sections), ISPK_E_SHAPE,
                 "ispk_equalize_f32: a table of %lld doubles, expected %d for %d sections", (long long)table_doubles,
                 eq_table_doubles(sections), sections);
    ISPK_REQUIRE(ld_audio >= S && ld_out >= S, ISPK_E_SHAPE, "ispk_equalize_f32: row strides %lld, %lld below S=%d",
                 (long long)ld_audio, (long long)ld_out, S);
    if (!(out == audio && (ld_out == ld_audio || B == 1))) {               // in place, or apart
        const uintptr_t a0 = (uintptr_t)audio, o0 = (uintptr_t)out;
        const uintptr_t a1 = a0 + 4 * (uintptr_t)((int64_t)(B - 1) * ld_audio + S), o1 = o0 + 4 * (uintptr_t)((int64_t)(B - 1) * ld_out + S);
        ISPK_REQUIRE(a1 <= o0 || o1 <= a0, ISPK_E_SHAPE,
                     "ispk_equalize_f32: out overlaps audio without being audio (same base and row stride)");
    }
    const int W = std::max(1, (S + kGridSeg - 1) / kGridSeg);
    const int64_t need = (int64_t)B * W * 2 * sections;
    ISPK_REQUIRE(workspace_doubles >= need && ispk_aligned(workspace, 8) && ispk_aligned(table, 8), ISPK_E_ALIGN,
                 "ispk_equalize_f32: the workspace needs %lld doubles at an 8-byte boundary, got %lld", (long long)need,
                 (long long)workspace_doubles);
    EqArgs a;
    a.ld = ld_audio, a.ld_out = ld_out, a.S = S, a.W = W, a.n = sections, a.seg = workspace;
    a.vec = ld_audio % 4 == 0 && ispk_aligned(audio, 16);
    a.vec_out = ld_out % 4 == 0 && ispk_aligned(out, 16);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (W > 1) hipLaunchKernelGGL(eq_state_kernel, dim3(W - 1, B), dim3(kGridThreads), 0, st, audio, audio_len, table, a);
    hipLaunchKernelGGL(eq_apply_kernel, dim3(W, B), dim3(kGridThreads), 0, st, audio, audio_len, table, out, out_len, a);
    return ispk_launch_status();
}
