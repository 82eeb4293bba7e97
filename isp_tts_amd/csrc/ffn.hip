// The four-wave fused feed-forward kernel, its W2 packer, launcher and entry points (ispk_ffn_pack_w2_bf16, ispk_ffn_bf16,
// ispk_ffn_bf16_prenorm).  The one-wave-per-SIMD successor the decoder layers call is csrc/ffn2.hip.
#include "gemm_common.h"

// Fused feed-forward block (bf16):  out = mask * ( resid + gelu(x · W1ᵀ + b1) · W2ᵀ + b2 )     feedforward.py:33-40 plus
// the residual add and row mask of transformer.py:105-110 — ONE kernel, the [rows, inner] hidden activations never
// leave the CU (unfused they cost 2 x rows x inner x 2 B of HBM traffic: 200 MB per decoder layer at the benchmark shape,
// more than everything else the layer moves).
//
// A workgroup owns 128 rows (4 waves x 32 rows, one wave per SIMD with the whole 512-register file):
//   xf   : the wave's 32 input rows x D as MFMA fragments, loaded once                            (D/16 x 4 VGPRs)
//   acc2 : the wave's 32 rows x D outputs, transposed (feature on the row axis, row on the lane)   (D/32 x 16 regs)
// and walks the inner dimension in chunks of 32 hidden units, software-pipelined by one chunk.  Iteration c:
//   phase A  acc1' = W1[chunk c+1] · xfᵀ   (D/16 MFMAs; W1 chunk [32][D] streamed through LDS)  - and, in the gaps
//            between those MFMAs, the GELU of chunk c's accumulators, packed pairwise to bf16: which IS the B operand
//            of phase B (register 8s+j of lane half h = hidden 16s + 8(j>>2) + 4h + (j&3): accumulator-as-operand)
//   phase B  acc2[nt] += W2[nt-th 32 features][chunk c] · Pᵀ   (D/32 x 2 MFMAs; W2 chunk [D][32] in LDS, its 32 hidden
//            columns in that same permuted order so that each fragment is ONE conflict-free ds_read_b128)
// With one wave per SIMD nothing else hides anything, so every non-MFMA instruction is placed by hand in an MFMA gap
// (measured with in-kernel stamps, tools/stamp_ffn.py: unscheduled, GELU and the weight staging bursts each took as
// long as a 24-MFMA phase):
//   * GELU: 8 register pairs x 3 stages of ~7 packed-fp32 instructions, one stage per phase-A gap;
//   * LDS stores of the prefetched W1 chunk c+2 / W2 chunk c+1 (already in registers): one per gap at the start of
//     phase A; they retire in order with the operand reads, so the hand-counted lgkmcnt waits count them as younger
//     operations instead of draining them;
//   * the global loads of W1 chunk c+3 / W2 chunk c+2 into those registers: one per gap at the start of phase B (a
//     burst of 12 loads blocks the wave's issue for 12 x 16 cycles x 4 waves on the CU's one address path).
// The operand reads of both phases run as ONE stream through an RD-deep ring of opaque asm reads.  One barrier per chunk.
// Epilogue: the row-coalescing transpose (store_rows_f32) with residual and mask.
// LX: the input is the fp32 residual stream and the kernel applies the LayerNorm that precedes the block itself.
template <int KC, bool B1, bool PK, int EP = kEpDyn, bool ST = false, bool LN = false, bool LX = false>  // D = 64 KC; B1: Linear 1 bias; PK: packed W2; LN: + LayerNorm of the result
__global__ __launch_bounds__(256, 1) void ffn_bf16_kernel(GemmParams p, const uint16_t* __restrict__ W2, int64_t ldw2,
                                                          const float* __restrict__ bias1, int F) {
    [[maybe_unused]] uint64_t tk0 = 0;
    if constexpr (ST) tk0 = __builtin_readcyclecounter();
    constexpr int D = 64 * KC, KS = D / 16, NT = D / 32, HC = 32;
    constexpr int LD1 = D + 8, LD2 = HC + 8;         // padded LDS rows (bf16 elements)
    constexpr int C1 = HC * (D / 8) / 256;            // 16-B pieces per thread: W1 chunk (32 rows x D/8)
    constexpr int C2 = D * (HC / 8) / 256;            //                          W2 chunk (D rows x 4)
    constexpr int W2OPS = PK ? 1 : 2;                 // LDS stores per W2 piece
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    uint16_t* W1s = reinterpret_cast<uint16_t*>(smem_raw);   // [2][HC][LD1]
    uint16_t* W2s = W1s + 2 * HC * LD1;                      // [2][D][LD2]
    char* stage = smem_raw + (size_t)(2 * HC * LD1 + 2 * D * LD2) * 2 + (threadIdx.x >> 6) * kStageBytes;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int mw0 = blockIdx.x * 128 + wave * 32;
    const int m = mw0 + l31;
    [[maybe_unused]] const uint16_t* X = static_cast<const uint16_t*>(p.A);
    const uint16_t* W1 = static_cast<const uint16_t*>(p.W);
    const int nchunks = F / HC;

    // Weight staging: ONE set of C = D/64 16-byte registers per thread alternates between the two operands - in phase A
    // gap i it holds W2 piece i of chunk c+1 (stored to LDS there, then reloaded with W1 piece i of chunk c+2), in phase
    // B gap i that W1 piece (stored, then reloaded with W2 piece i of chunk c+2): each load has one 24-MFMA phase to
    // land (the weights are L2-resident), and only C x 4 registers are tied up instead of 2C x 4 - this kernel sits at
    // the edge of the 256 + 256 register file.  Addresses are "uniform base + one lane offset" (W1 rows are contiguous,
    // ldw1 == D, checked by the launcher): piece i of a chunk is 16-byte unit tid + 256 i.
    constexpr int C = C1;
    static_assert(C1 == C2, "D/64 pieces of either operand per thread");
    u32x4 R[C];
    const uint32_t lane_off1 = tid * 8;                                                    // elements
    const uint32_t lane_off2 = PK ? tid * 8 : (tid >> 2) * (uint32_t)ldw2 + (tid & 3) * 8;
    const int step1 = HC * D;
    const int step2 = PK ? D * HC : HC;              // packed: chunk c is one contiguous [D][32] block
    const int pstep2 = PK ? 2048 : 64 * (int)ldw2;   // piece i -> i + 1 (uniform)
    auto load1 = [&](int i, int c) {      // chunk indices past the end re-read the last chunk (never consumed)
        c = c < nchunks ? c : nchunks - 1;
        R[i] = *reinterpret_cast<const u32x4*>(W1 + ((int64_t)c * step1 + i * 2048) + lane_off1);
    };
    auto load2 = [&](int i, int c) {
        c = c < nchunks ? c : nchunks - 1;
        R[i] = *reinterpret_cast<const u32x4*>(W2 + ((int64_t)c * step2 + (int64_t)i * pstep2) + lane_off2);
    };
    uint32_t s1off[C];   // LDS byte offset of W1 piece i inside a buffer: row (tid + 256 i) / (D/8), 16-byte column
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const int id = tid + 256 * i, r = id / (D / 8), cc = id - r * (D / 8);
        s1off[i] = (r * LD1 + cc * 8) * 2;
    }
    auto store1 = [&](int i, int buf) {
        *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(W1s) + buf * (HC * LD1 * 2) + s1off[i]) = R[i];
    };
    // Row-major W2: chunk rows are stored PERMUTED into the hidden order of the accumulator fragment (LDS position
    // 16s + 8h + j holds hidden 16s + 8(j>>2) + 4h + (j&3)), so a lane's k-step fragment is one aligned 16-byte run: the
    // global 16-byte piece cc (hidden 8cc .. 8cc+7; s = cc>>1, a = cc&1) lands as two 8-byte halves at 16s + 4a (h = 0)
    // and 16s + 8 + 4a (h = 1).  The packed image is already in that order.
    const int s2cc = tid & 3;
    uint16_t* const s2row = W2s + (tid >> 2) * LD2 + (PK ? s2cc * 8 : 16 * (s2cc >> 1) + 4 * (s2cc & 1));
    auto store2 = [&](int i, int buf) {
        uint16_t* row = s2row + (buf * D + 64 * i) * LD2;
        if constexpr (PK) {
            *reinterpret_cast<u32x4*>(row) = R[i];
        } else {
            uint2 lo, hi;
            lo.x = R[i][0]; lo.y = R[i][1]; hi.x = R[i][2]; hi.y = R[i][3];
            *reinterpret_cast<uint2*>(row) = lo;
            *reinterpret_cast<uint2*>(row + 8) = hi;
        }
    };

    // ---- prologue: W1 chunk 0 on its way, then the wave's 32 rows x D as MFMA fragments through a wave-private LDS
    // patch (coalesced 16-byte loads; see gemm_bf16_panel_kernel), one D-half at a time
    bf16x8 xf[KS];
    if constexpr (LX) {
#pragma unroll
        for (int i = 0; i < C; ++i) load1(i, 0);
        // Pre-norm in the prologue (ispk_ffn_bf16_prenorm; transformer.py:101-105: feed_forward(feed_forward_norm(x))):
        // a wave owns whole rows, so it computes their LayerNorm statistics itself - the 32 rows x D fp32 stay in
        // registers (D/2 VGPRs; the accumulators are not live yet) through two passes in fixed summation order (each
        // lane's float4 partial -> a wave-private LDS table -> one lane per row half adds them up: deterministic), then
        // (x - mean) * rstd * gamma + beta is rounded to bf16 on the way into the fragment patch, a K-quarter at a time.
        constexpr int KQ = D / 4, CPQ = KQ / 4, XQ = 32 * CPQ / 64, XLQ = KQ * 2 + 16;     // per K-quarter; XLQ in bytes
        constexpr int GC = (64 % CPQ == 0) ? CPQ : (CPQ == 24 ? 8 : 1), NG = CPQ / GC;       // gcd(64, CPQ); groups per lane
        constexpr int PLD = 4 * CPQ + 1;                                                     // partials per row, padded
        static_assert(4 * 32 * XLQ + 4 * 32 * PLD * 4 + 4 * 64 * 4 <= (2 * HC * LD1 + 2 * D * LD2) * 2,
                      "pre-norm staging aliases the weight buffers");
        const float* Xf = static_cast<const float*>(p.A);
        char* xs = smem_raw + wave * (32 * XLQ);
        float* part = reinterpret_cast<float*>(smem_raw + 4 * (32 * XLQ)) + wave * (32 * PLD);
        float* sst = reinterpret_cast<float*>(smem_raw + 4 * (32 * XLQ) + 4 * 32 * PLD * 4) + wave * 64;
        float4 t[4][XQ];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < XQ; ++j) {
                const int id = lane + 64 * j, r = id / CPQ, c = id - r * CPQ;
                const int row = mw0 + r < p.M ? mw0 + r : p.M - 1;
                t[q][j] = *reinterpret_cast<const float4*>(Xf + (int64_t)row * p.lda + q * KQ + c * 4);
            }
        auto row_total = [&]() {   // sum of this lane's row (l31) over the partial table; both halves end with the total
            float a = 0.f;
#pragma unroll
            for (int i = 0; i < 2 * CPQ; ++i) a += part[l31 * PLD + h * (2 * CPQ) + i];
            return a + __shfl_xor(a, 32, 64);
        };
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < XQ; ++j) {
                const int id = lane + 64 * j, r = id / CPQ, c = id - r * CPQ;
                const float4 v = t[q][j];
                part[r * PLD + q * CPQ + c] = (v.x + v.y) + (v.z + v.w);
            }
        const float mean_l = row_total() * (1.0f / (float)D);
        if (h == 0) sst[2 * l31] = mean_l;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < XQ; ++j) {
                const int id = lane + 64 * j, r = id / CPQ, c = id - r * CPQ;
                const float mu = sst[2 * r];
                const float4 v = t[q][j];
                const float a = v.x - mu, b = v.y - mu, cc = v.z - mu, d = v.w - mu;
                part[r * PLD + q * CPQ + c] = (a * a + b * b) + (cc * cc + d * d);
            }
        const float rstd_l = 1.0f / sqrtf(row_total() * (1.0f / (float)D) + p.lx_eps);
        if (h == 0) sst[2 * l31 + 1] = rstd_l;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 g[NG], be[NG];
#pragma unroll
            for (int u = 0; u < NG; ++u) {
                const int c = (lane + 64 * u) % CPQ;
                g[u] = *reinterpret_cast<const float4*>(p.lx_gamma + q * KQ + c * 4);
                be[u] = *reinterpret_cast<const float4*>(p.lx_beta + q * KQ + c * 4);
            }
#pragma unroll
            for (int j = 0; j < XQ; ++j) {
                const int id = lane + 64 * j, r = id / CPQ, c = id - r * CPQ;
                const float mean = sst[2 * r], rstd = sst[2 * r + 1];
                const float4 v = t[q][j], gg = g[j % NG], bb = be[j % NG];
                uint2 o;
                o.x = pack_bf16x2((v.x - mean) * rstd * gg.x + bb.x, (v.y - mean) * rstd * gg.y + bb.y);
                o.y = pack_bf16x2((v.z - mean) * rstd * gg.z + bb.z, (v.w - mean) * rstd * gg.w + bb.w);
                *reinterpret_cast<uint2*>(xs + r * XLQ + c * 8) = o;
            }
#pragma unroll
            for (int ks = 0; ks < KS / 4; ++ks)
                xf[q * (KS / 4) + ks] = *reinterpret_cast<const bf16x8*>(xs + l31 * XLQ + ks * 32 + h * 16);
        }
    } else {
#pragma unroll
        for (int i = 0; i < C; ++i) load1(i, 0);
        constexpr int KH = D / 2, CPH = KH / 8, XCH = 32 * CPH / 64, XLD = KH * 2 + 16;
        static_assert(4 * 32 * XLD <= (2 * HC * LD1 + 2 * D * LD2) * 2, "x staging patches alias the weight buffers");
        char* xs = smem_raw + wave * (32 * XLD);
        u32x4 t[2][XCH];
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
            for (int j = 0; j < XCH; ++j) {
                const int id = lane + 64 * j, r = id / CPH, c = id - r * CPH;
                const int row = mw0 + r < p.M ? mw0 + r : p.M - 1;
                t[half][j] = *reinterpret_cast<const u32x4*>(X + (int64_t)row * p.lda + half * KH + c * 8);
            }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int j = 0; j < XCH; ++j) {
                const int id = lane + 64 * j, r = id / CPH, c = id - r * CPH;
                *reinterpret_cast<u32x4*>(xs + r * XLD + c * 16) = t[half][j];
            }
#pragma unroll
            for (int ks = 0; ks < KS / 2; ++ks)
                xf[half * (KS / 2) + ks] = *reinterpret_cast<const bf16x8*>(xs + l31 * XLD + ks * 32 + h * 16);
        }
    }
    __syncthreads();   // the patches alias the weight buffers
    // LDS <- W1 chunks 0 and 1, W2 chunk 0; R <- W2 chunk 1 (stored in phase A of iteration 0)
#pragma unroll
    for (int i = 0; i < C; ++i) store1(i, 0);
#pragma unroll
    for (int i = 0; i < C; ++i) load2(i, 0);
#pragma unroll
    for (int i = 0; i < C; ++i) store2(i, 0);
#pragma unroll
    for (int i = 0; i < C; ++i) load1(i, 1);
#pragma unroll
    for (int i = 0; i < C; ++i) store1(i, 1);
#pragma unroll
    for (int i = 0; i < C; ++i) load2(i, 1);
    f32x16 acc2[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[t][r] = 0.f;
    __syncthreads();

    const uint32_t w1base = lds_addr(W1s + l31 * LD1 + 8 * h);
    const uint32_t w2base = lds_addr(W2s + l31 * LD2 + 8 * h);

    // GELU of one accumulator register pair in three stages of ~7 packed-fp32 instructions (= gelu_fast2, same operation
    // order): stage 0 reads the accumulators, stage 2 writes the packed bf16 pair into the next phase's B operand.
    union Frag { uint32_t u[4]; bf16x8 f; };
    f32x16 acc1;
    Frag pfC[2], pfN[2];                  // B operand of the running phase B / being produced for the next one
    f32x2 gx[8], gax[8], gz[8], gq[8];   // per-pair state between stages (one or two pairs live at a time)
    auto gelu_stage = [&](auto gc, int c) __attribute__((always_inline)) {
        constexpr int g = decltype(gc)::value, pr = g / 3, sg = g % 3;   // register pair, stage
        constexpr int r0 = 8 * (pr >> 2) + 2 * (pr & 3);                  // accumulator registers r0, r0 + 1
        if constexpr (sg == 0) {
            f32x2 v;
            v.x = acc1[r0]; v.y = acc1[r0 + 1];
            if constexpr (B1) {
                const int hid = c * HC + (r0 & 3) + 8 * (r0 >> 2) + 4 * h;
                v.x += bias1[hid]; v.y += bias1[hid + 1];
            }
            gx[pr] = v;
            f32x2 ax;
            ax.x = fabsf(v.x); ax.y = fabsf(v.y);
            gax[pr] = ax;
            const f32x2 z = ax * 0.70710678118654752440f;
            gz[pr] = z;
            f32x2 qq = z * 0.0000430638f + 0.0002765672f;
            qq = qq * z + 0.0001520143f;
            qq = qq * z + 0.0092705272f;
            gq[pr] = qq * z + 0.0422820123f;
        } else if constexpr (sg == 1) {
            const f32x2 z = gz[pr];
            f32x2 qq = gq[pr] * z + 0.0705230784f;
            qq = qq * z + 1.0f;
            qq = qq * qq; qq = qq * qq; qq = qq * qq; qq = qq * qq;
            f32x2 r;
            r.x = __builtin_amdgcn_rcpf(qq.x); r.y = __builtin_amdgcn_rcpf(qq.y);
            gq[pr] = r;
        } else {
            const f32x2 hx = gax[pr] * 0.5f;                  // max(x, 0) = 0.5 x + 0.5 |x|
            const f32x2 o = gx[pr] * 0.5f + (hx - hx * gq[pr]);
            pfN[pr >> 2].u[pr & 3] = pack_bf16x2(o.x, o.y);
        }
    };

    {   // pipeline fill: acc1 = W1[chunk 0] · xfᵀ and its GELU (plain reads, no overlap)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(W1s + l31 * LD1 + 8 * h + 16 * ks);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xf[ks], acc1, 0, 0, 0);
        }
        static_for<0, 24>([&](auto gc) { gelu_stage(gc, 0); });
        pfC[0].f = pfN[0].f;
        pfC[1].f = pfN[1].f;
    }
    __syncthreads();   // iteration 1 overwrites W1s[0]

    // Iteration c = 1 .. nchunks:  phase A  acc1 = W1[chunk c] · xfᵀ            (reads W1s[c & 1]; chunk nchunks: a re-run
    //                                                                           of the last chunk, never consumed)
    //                              phase B  acc2 += W2[chunk c-1] · pfCᵀ        (reads W2s[(c-1) & 1]) + GELU(chunk c) -> pfN
    constexpr int RD = 4, NB = 2 * NT, NS = KS + NB;
    static_assert(C <= KS && C <= NB && RD - 1 + RD * W2OPS <= 15, "staging slots / lgkmcnt range");
    [[maybe_unused]] uint64_t tsum[5] = {0, 0, 0, 0, 0}, t0 = 0, tA = 0, tB = 0;
    if constexpr (ST) tsum[3] = __builtin_readcyclecounter() - tk0;
    for (int c = 1; c <= nchunks; ++c) {
        if constexpr (ST) t0 = __builtin_readcyclecounter();
        const int pc = c & 1;
        const uint32_t a1 = w1base + pc * (HC * LD1 * 2);
        const uint32_t a2 = w2base + (pc ^ 1) * (D * LD2 * 2);
        bf16x8 q[RD];
        auto issue = [&](auto ic) {
            constexpr int st = decltype(ic)::value;
            if constexpr (st < KS) {
                lds_read_b128_asm_acc<st * 32>(q[st % RD], a1);
            } else {
                constexpr int nt = (st - KS) / 2, s2 = (st - KS) % 2;
                lds_read_b128_asm_acc<(nt * 32 * LD2 + 16 * s2) * 2>(q[st % RD], a2);
            }
        };
        static_for<0, RD>(issue);
        static_for<0, NS>([&](auto ic) {
            constexpr int st = decltype(ic)::value;
            if constexpr (ST && st == KS) { __builtin_amdgcn_sched_barrier(0); tA = __builtin_readcyclecounter(); }
            // LDS operations younger than read(st): the later reads of the ring plus the stores of gaps st-RD .. st-1
            // (W2 pieces in phase-A gaps 0 .. C-1, W1 pieces in phase-B gaps KS .. KS+C-1)
            constexpr int reads_after = (NS - 1 - st) < (RD - 1) ? (NS - 1 - st) : (RD - 1);
            constexpr int g0 = st - RD < 0 ? 0 : st - RD;
            constexpr int n2 = (st < C ? st : C) - (g0 < C ? g0 : C);
            constexpr int hi1 = st < KS ? KS : (st < KS + C ? st : KS + C), lo1 = g0 < KS ? KS : (g0 < KS + C ? g0 : KS + C);
            lds_wait<reads_after + n2 * W2OPS + (hi1 - lo1)>();
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (st == 0) {
                f32x16 z;
#pragma unroll
                for (int r = 0; r < 16; ++r) z[r] = 0.f;
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(q[st % RD], xf[st], z, 0, 0, 0);
            } else if constexpr (st < KS) {
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(q[st % RD], xf[st], acc1, 0, 0, 0);
            } else {
                constexpr int nt = (st - KS) / 2, s2 = (st - KS) % 2;
                acc2[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(q[st % RD], pfC[s2].f, acc2[nt], 0, 0, 0);
            }
            if constexpr (st + RD < NS) issue(std::integral_constant<int, st + RD>{});
            // ---- gap work
            if constexpr (st < C) {                        // phase A: W2 chunk c -> LDS, W1 chunk c+1 -> register
                store2(st, pc);
                load1(st, c + 1);
            }
            if constexpr (st >= KS && st - KS < C) {        // phase B: W1 chunk c+1 -> LDS, W2 chunk c+1 -> register
                store1(st - KS, pc ^ 1);
                load2(st - KS, c + 1);
            }
            if constexpr (st >= KS) {                      // phase B: the GELU stages that fall into this gap (the first
                static_for<0, 24>([&](auto gc) {           // gap is left to the last phase-A MFMA's latency)
                    constexpr int g = decltype(gc)::value;
                    constexpr int gap = (g * NB / 24 + 1) < NB ? (g * NB / 24 + 1) : NB - 1;
                    if constexpr (gap == st - KS) gelu_stage(gc, c);
                });
            }
        });
        pfC[0].f = pfN[0].f;
        pfC[1].f = pfN[1].f;
        if constexpr (ST) { __builtin_amdgcn_sched_barrier(0); tB = __builtin_readcyclecounter(); }
        __syncthreads();
        if constexpr (ST) {
            const uint64_t tE = __builtin_readcyclecounter();
            tsum[0] += tA - t0; tsum[1] += tB - tA; tsum[2] += tE - tB;
        }
    }
    if constexpr (ST) tk0 = __builtin_readcyclecounter();

    float mk = 1.0f;
    if (EP < 0 || ((uint32_t)EP & (ISPK_EP_MASK_ACC | ISPK_EP_MASK_OUT))) mk = (p.mask && m < p.M) ? (p.mask[m] ? 1.0f : 0.0f) : 1.0f;
    // epilogue: the residual rows of tile nt+PF are requested while tile nt is transposed and stored
    constexpr int PF = LN ? 1 : 3;   // (the LayerNorm variant keeps all final values in registers)
    float mo4[4];
    mask_rows<EP>(p, mw0, lane, mo4);
    float4 rres[PF + 1][4];
    static_for<0, PF>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        if constexpr (t < NT) resid_prefetch<EP>(p, mw0, t * 32, lane, rres[t]);
    });
    if constexpr (!LN) {
        static_for<0, NT>([&](auto tc) {
            constexpr int nt = decltype(tc)::value;
            if constexpr (nt + PF < NT) resid_prefetch<EP>(p, mw0, (nt + PF) * 32, lane, rres[(nt + PF) % (PF + 1)]);
            store_rows_f32<EP>(p, stage, mw0, nt * 32, acc2[nt], mk, lane, nullptr, rres[nt % (PF + 1)], mo4);
        });
    } else {
        // + LayerNorm of the finished rows for the next Linear (normalization.py:20-27; transformer.py:79 of the next
        // layer, or :205-206 after the last): a wave holds ALL D features of its 32 rows, so the statistics need no LDS
        // or barrier - two passes in fp32 over the final values kept in registers (D/32 x 4 float4, the accumulators
        // they replace die tile by tile), reduced over the 8 lanes that share a row.  Saves the separate LayerNorm
        // launch and its 50-MB re-read of the residual stream per decoder layer.
        float4 yv[NT][4];
        float rs[4] = {0.f, 0.f, 0.f, 0.f};
        static_for<0, NT>([&](auto tc) {
            constexpr int nt = decltype(tc)::value;
            if constexpr (nt + PF < NT) resid_prefetch<EP>(p, mw0, (nt + PF) * 32, lane, rres[(nt + PF) % (PF + 1)]);
            store_rows_f32<EP>(p, stage, mw0, nt * 32, acc2[nt], mk, lane, yv[nt], rres[nt % (PF + 1)], mo4);
#pragma unroll
            for (int i = 0; i < 4; ++i) rs[i] += (yv[nt][i].x + yv[nt][i].y) + (yv[nt][i].z + yv[nt][i].w);
        });
        auto row_total = [&](float (&v)[4]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] += __shfl_xor(v[i], 1, 64);
                v[i] += __shfl_xor(v[i], 2, 64);
                v[i] += __shfl_xor(v[i], 4, 64);
            }
        };
        row_total(rs);
        float mean[4], qs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            mean[i] = rs[i] * (1.0f / (float)D);
            qs[i] = 0.f;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float a = yv[t][i].x - mean[i], b = yv[t][i].y - mean[i], c = yv[t][i].z - mean[i],
                            d = yv[t][i].w - mean[i];
                qs[i] += (a * a + b * b) + (c * c + d * d);
            }
        row_total(qs);
        const int c4 = (lane & 7) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mr = mw0 + 8 * i + (lane >> 3);
            if (mr >= p.M) continue;
            const float rstd = 1.0f / sqrtf(qs[i] * (1.0f / (float)D) + p.ln_eps);
            if (p.ln_flags & 4u) {   // statistics only: the consumer GEMM normalises in its prologue (ispk_gemm_bf16_lnin)
                if ((lane & 7) == 0)
                    *reinterpret_cast<float2*>(static_cast<float*>(p.ln_out) + 2 * (int64_t)mr) = make_float2(mean[i], rstd);
                continue;
            }
            const float mo = ((p.ln_flags & 1u) && p.mask) ? (p.mask[mr] ? 1.0f : 0.0f) : 1.0f;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int n = t * 32 + c4;
                const float4 g = *reinterpret_cast<const float4*>(p.ln_gamma + n);
                const float4 be = *reinterpret_cast<const float4*>(p.ln_beta + n);
                float4 o;
                o.x = ((yv[t][i].x - mean[i]) * rstd * g.x + be.x) * mo;
                o.y = ((yv[t][i].y - mean[i]) * rstd * g.y + be.y) * mo;
                o.z = ((yv[t][i].z - mean[i]) * rstd * g.z + be.z) * mo;
                o.w = ((yv[t][i].w - mean[i]) * rstd * g.w + be.w) * mo;
                const int64_t off = (int64_t)mr * p.ln_ld + n;
                if (p.ln_flags & 2u) {
                    uint2 pk;
                    pk.x = pack_bf16x2(o.x, o.y);
                    pk.y = pack_bf16x2(o.z, o.w);
                    *reinterpret_cast<uint2*>(static_cast<uint16_t*>(p.ln_out) + off) = pk;
                } else {
                    *reinterpret_cast<float4*>(static_cast<float*>(p.ln_out) + off) = o;
                }
            }
        }
    }
    if constexpr (ST) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tsum[4] = __builtin_readcyclecounter() - tk0;
        if (lane == 0) {
            uint64_t* dbg = static_cast<uint64_t*>(p.ln_out) + (blockIdx.x * 4 + wave) * 5;
            for (int i = 0; i < 5; ++i) dbg[i] = tsum[i];
        }
    }
}

// W2 [D][F] (nn.Linear layout) -> [F/32][D][32] with each chunk's 32 hidden units in accumulator-fragment order
// (position 16s + 8h + 4a + b holds hidden 16s + 8a + 4h + b): a chunk becomes ONE contiguous 64*D-byte block, so the
// fused kernel streams it with full-line loads spread over every L2 channel (the [D][F] layout reads 64 bytes from each
// of D rows 2*F bytes apart) and stages it with straight 16-byte LDS stores.
__global__ void ffn_pack_w2_kernel(const uint16_t* __restrict__ W2, int64_t ldw2, uint16_t* __restrict__ out, int D, int F) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // one output element
    if (idx >= (int64_t)D * F) return;
    const int pos = idx & 31, n = (idx >> 5) % D, c = (idx >> 5) / D;
    const int hid = (pos & 16) | ((pos & 4) << 1) | ((pos & 8) >> 1) | (pos & 3);
    out[idx] = W2[(int64_t)n * ldw2 + c * 32 + hid];
}

extern "C" int32_t ispk_ffn_pack_w2_bf16(const uint16_t* W2, int64_t ldw2, int32_t D, int32_t F, uint16_t* packed,
                                         ispk_stream_t stream) {
    ISPK_REQUIRE(W2 && packed, ISPK_E_NULL, "ffn_pack_w2: null pointer");
    ISPK_REQUIRE(D >= 1 && F >= 32 && F % 32 == 0 && ldw2 >= F, ISPK_E_SHAPE, "ffn_pack_w2: bad shape D=%d inner=%d", D, F);
    const int64_t n = (int64_t)D * F;
    hipLaunchKernelGGL(ffn_pack_w2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), W2, ldw2, packed, D, F);
    return ispk_launch_status();
}

namespace {
struct FfnLn {   // optional LayerNorm of the result; ispk_ffn_bf16_prenorm asks for the statistics only (flags = 4)
    const float* gamma = nullptr;
    const float* beta = nullptr;
    float eps = 0.f;
    void* out = nullptr;
    int64_t ld = 0;
    uint32_t flags = 0;
};
struct FfnLx {   // LayerNorm applied to the (fp32) input in the prologue
    const float* gamma = nullptr;
    const float* beta = nullptr;
    float eps = 1e-5f;
};
int32_t ffn_launch(const void* x, int64_t ldx, const uint16_t* W1, int64_t ldw1, const float* bias1,
                   const uint16_t* W2, int64_t ldw2, const float* bias2, const float* resid, int64_t ldr,
                   const uint8_t* mask, float* out, int64_t ldo, int32_t rows, int32_t D, int32_t F, uint32_t flags,
                   const FfnLn* ln, ispk_stream_t stream, const FfnLx* lx = nullptr) {
    ISPK_REQUIRE(x && W1 && W2 && out, ISPK_E_NULL, "ffn: null pointer");
    ISPK_REQUIRE(D == 384 || D == 256, ISPK_E_UNSUPPORTED, "ffn: dim %d (built for 256 / 384)", D);
    ISPK_REQUIRE(rows >= 0 && F >= 64 && F % 32 == 0, ISPK_E_SHAPE, "ffn: bad shape rows=%d inner=%d", rows, F);
    ISPK_REQUIRE((flags & ~(ISPK_EP_MASK_OUT | ISPK_EP_MASK_ACC)) == 0, ISPK_E_UNSUPPORTED, "ffn: unsupported flags");
    ISPK_REQUIRE(!((flags & (ISPK_EP_MASK_OUT | ISPK_EP_MASK_ACC)) && !mask), ISPK_E_NULL, "ffn: mask flag without mask");
    ISPK_REQUIRE(ldx % (lx ? 4 : 8) == 0 && ldw1 % 8 == 0 && ldw2 % 8 == 0 && ldo % 4 == 0 && (!resid || ldr % 4 == 0) && ldx >= D &&
                     ldw1 >= D && (ldw2 >= F || ldw2 == 0) && ldo >= D,
                 ISPK_E_ALIGN, "ffn: leading strides must be multiples of 8 (bf16) / 4 (fp32)");
    ISPK_REQUIRE(ispk_aligned(x, 16) && ispk_aligned(W1, 16) && ispk_aligned(W2, 16) && ispk_aligned(out, 16) &&
                     (!resid || ispk_aligned(resid, 16)) && (!bias2 || ispk_aligned(bias2, 16)),
                 ISPK_E_ALIGN, "ffn: pointers must be 16-byte aligned");
    if (rows == 0) return 0;
    GemmParams p{x, ldx, W1, ldw1, out, ldo, bias2, resid, ldr, mask, rows, D, D, flags & ~ISPK_EP_GELU, 0, 0};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((rows + 127) / 128);
    ISPK_REQUIRE((int64_t)F * ldw1 < (1ll << 30) && (int64_t)D * ldw2 < (1ll << 30), ISPK_E_SHAPE, "ffn: weights too large");
    ISPK_REQUIRE(ldw1 == D, ISPK_E_UNSUPPORTED, "ffn: W1 rows must be contiguous (ldw1 == dim)");
    constexpr int kHot = ISPK_EP_MASK_OUT | kEpResid;   // the transformer layer's call (transformer.py:105-110), no bias2
    const bool hot = ep_key(p) == kHot && ispk_knob("ISPK_EP_DYN") == nullptr;
    const bool packed = ldw2 == 0;   // W2 laid out by ispk_ffn_pack_w2_bf16
    ISPK_REQUIRE(lx || !ln, ISPK_E_UNSUPPORTED, "ffn: a LayerNorm of the result needs the pre-norm prologue (ispk_ffn_bf16_prenorm)");
    if (ln) {
        const bool stats_only = ln->flags & 4u;   // ln_out = float [rows][2] (mean, rstd); gamma / beta unused
        ISPK_REQUIRE(ln->out && (stats_only || (ln->gamma && ln->beta)), ISPK_E_NULL, "ffn_ln: null LayerNorm argument");
        ISPK_REQUIRE(stats_only ? ispk_aligned(ln->out, 8)
                                : (ln->ld % 4 == 0 && ln->ld >= D && ispk_aligned(ln->out, (ln->flags & 2u) ? 8 : 16) &&
                                   ispk_aligned(ln->gamma, 16) && ispk_aligned(ln->beta, 16)),
                     ISPK_E_ALIGN, "ffn_ln: LayerNorm buffers must be 16-byte aligned, ln_ld a multiple of 4");
        ISPK_REQUIRE(!((ln->flags & 1u) && !mask), ISPK_E_NULL, "ffn_ln: ln mask flag set but mask is NULL");
        ISPK_REQUIRE(packed && !bias1, ISPK_E_UNSUPPORTED, "ffn_ln: needs the packed W2 image and no first-Linear bias");
        p.ln_gamma = ln->gamma; p.ln_beta = ln->beta; p.ln_out = ln->out; p.ln_ld = ln->ld; p.ln_eps = ln->eps;
        p.ln_flags = ln->flags;
    }
    if (lx) {
        ISPK_REQUIRE(lx->gamma && lx->beta, ISPK_E_NULL, "ffn_prenorm: null LayerNorm argument");
        ISPK_REQUIRE(ispk_aligned(lx->gamma, 16) && ispk_aligned(lx->beta, 16), ISPK_E_ALIGN,
                     "ffn_prenorm: gamma / beta must be 16-byte aligned");
        ISPK_REQUIRE(packed && !bias1, ISPK_E_UNSUPPORTED, "ffn_prenorm: needs the packed W2 image and no first-Linear bias");
        p.lx_gamma = lx->gamma; p.lx_beta = lx->beta; p.lx_eps = lx->eps;
    }
    void* stamp = nullptr;
#ifdef ISPK_EXPERIMENTS
    if (const char* e = ispk_knob("ISPK_FFN_STAMP")) {   // experiments only: per-wave phase cycle sums -> uint64[grid*4][3]
        stamp = reinterpret_cast<void*>(strtoull(e, nullptr, 16));
        ISPK_REQUIRE(D == 384 && packed && !bias1 && hot && !ln && !lx, ISPK_E_UNSUPPORTED, "ffn stamps: the hot instance only");
        p.ln_out = stamp;
    }
#endif
#define ISPK_FFN_GO(KC_, B1_, PK_, EP_, ST_)                                                                          \
    do {                                                                                                              \
        constexpr size_t lds = (size_t)(2 * 32 * (64 * KC_ + 8) + 2 * 64 * KC_ * 40) * 2 + 4 * kStageBytes;             \
        ISPK_RESERVE_LDS((&ffn_bf16_kernel<KC_, B1_, PK_, EP_, ST_>), lds, "ffn");                                    \
        hipLaunchKernelGGL((ffn_bf16_kernel<KC_, B1_, PK_, EP_, ST_>), grid, dim3(256), lds, s, p, W2, ldw2, bias1, F); \
        return ispk_launch_status();                                                                                  \
    } while (0)
#define ISPK_FFN_GO_LX(KC_, EP_, LN_)                                                                                 \
    do {                                                                                                              \
        constexpr size_t lds = (size_t)(2 * 32 * (64 * KC_ + 8) + 2 * 64 * KC_ * 40) * 2 + 4 * kStageBytes;             \
        ISPK_RESERVE_LDS((&ffn_bf16_kernel<KC_, false, true, EP_, false, LN_, true>), lds, "ffn");                    \
        hipLaunchKernelGGL((ffn_bf16_kernel<KC_, false, true, EP_, false, LN_, true>), grid, dim3(256), lds, s, p, W2,  \
                           ldw2, bias1, F);                                                                           \
        return ispk_launch_status();                                                                                  \
    } while (0)
#ifdef ISPK_EXPERIMENTS
#define ISPK_FFN_STAMPED() do { if (stamp) ISPK_FFN_GO(6, false, true, kHot, true); } while (0)
#else
#define ISPK_FFN_STAMPED() (void)stamp
#endif
#define ISPK_FFN_KC(KC_)                                                   \
    do {                                                                   \
        if (lx && ln && hot) ISPK_FFN_GO_LX(KC_, kHot, true);              \
        if (lx && ln) ISPK_FFN_GO_LX(KC_, kEpDyn, true);                   \
        if (lx && hot) ISPK_FFN_GO_LX(KC_, kHot, false);                   \
        if (lx) ISPK_FFN_GO_LX(KC_, kEpDyn, false);                        \
        ISPK_FFN_STAMPED();                                                \
        if (!bias1 && packed && hot) ISPK_FFN_GO(KC_, false, true, kHot, false);  \
        if (!bias1 && packed) ISPK_FFN_GO(KC_, false, true, kEpDyn, false);  \
        if (!bias1) ISPK_FFN_GO(KC_, false, false, kEpDyn, false);          \
        if (packed) ISPK_FFN_GO(KC_, true, true, kEpDyn, false);            \
        ISPK_FFN_GO(KC_, true, false, kEpDyn, false);                       \
    } while (0)
    if (D == 384) ISPK_FFN_KC(6); else ISPK_FFN_KC(4);
#undef ISPK_FFN_KC
#undef ISPK_FFN_STAMPED
#undef ISPK_FFN_GO_LX
#undef ISPK_FFN_GO
    return ispk_launch_status();
}
}  // namespace

extern "C" int32_t ispk_ffn_bf16(const uint16_t* x, int64_t ldx, const uint16_t* W1, int64_t ldw1, const float* bias1,
                                 const uint16_t* W2, int64_t ldw2, const float* bias2, const float* resid, int64_t ldr,
                                 const uint8_t* mask, float* out, int64_t ldo, int32_t rows, int32_t D, int32_t F,
                                 uint32_t flags, ispk_stream_t stream) {
    return ffn_launch(x, ldx, W1, ldw1, bias1, W2, ldw2, bias2, resid, ldr, mask, out, ldo, rows, D, F, flags, nullptr, stream);
}

extern "C" int32_t ispk_ffn_bf16_prenorm(const float* x, int64_t ldx, const float* norm_gamma, const float* norm_beta,
                                         float norm_eps, const uint16_t* W1, int64_t ldw1, const uint16_t* W2_packed,
                                         const float* bias2, const uint8_t* mask, float* out, int64_t ldo, int32_t rows,
                                         int32_t D, int32_t F, uint32_t flags, float* row_stats, float stats_eps,
                                         ispk_stream_t stream) {
    ISPK_REQUIRE(x && ispk_aligned(x, 16), ISPK_E_ALIGN, "ffn_prenorm: x must be a 16-byte aligned fp32 pointer");
    FfnLx lx{norm_gamma, norm_beta, norm_eps};
    FfnLn ln{nullptr, nullptr, stats_eps, row_stats, 0, 4u};
    return ffn_launch(x, ldx, W1, ldw1, nullptr, W2_packed, 0, bias2, x, ldx, mask, out, ldo, rows, D, F, flags,
                      row_stats ? &ln : nullptr, stream, &lx);
}
