// The per-key-block device code of the bf16 ALiBi multi-query attention kernels: one 32-key x 32-query block of a wave -
// score MFMAs with the bias in the accumulator init, key-length mask, lazily rescaled online softmax, P·V MFMAs.
// attention.hip (attn_bf16_kernel) and attn_block.hip (attn_block_short_kernel) both run exactly this code, so their
// rows agree bit for bit.  The layout it expects of K, V and Q is described in attention.hip.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float xhalf_max(float v) { return fmaxf(v, __shfl_xor(v, 32, 64)); }
__device__ __forceinline__ float xhalf_sum(float v) { return v + __shfl_xor(v, 32, 64); }

// max over the two 32-lane halves without the LDS round trip of a bpermute: v_permlane32_swap exchanges the upper half
// of one register with the lower half of another (gfx950).  (Inline asm: the builtin's second result was miscompiled.)
// v_max3_f32 without the canonicalising v_max x, x that fmaxf() puts in front of every operand (scores are never sNaN)
__device__ __forceinline__ float max3_raw(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// exchange the upper half (lanes 32-63) of x with the lower half (lanes 0-31) of y
__device__ __forceinline__ void half_swap(uint32_t& x, uint32_t& y) {
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
}
__device__ __forceinline__ float xhalf_max_swap(float v) {
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
}

// Two adjacent 32-feature accumulator tiles of the wave's 32 rows (register 4g + e of tile t = feature 32t + 8g + 4h + e of the
// lane's row), times `scale`, rounded to bf16: pk[t][g] = the lane's 4-feature group g of tile t.
__device__ __forceinline__ void pack_rows_bf16(const f32x16& a0, const f32x16& a1, float scale, uint2 (&pk)[2][4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        pk[0][g].x = pack_bf16x2(a0[4 * g] * scale, a0[4 * g + 1] * scale);
        pk[0][g].y = pack_bf16x2(a0[4 * g + 2] * scale, a0[4 * g + 3] * scale);
        pk[1][g].x = pack_bf16x2(a1[4 * g] * scale, a1[4 * g + 1] * scale);
        pk[1][g].y = pack_bf16x2(a1[4 * g + 2] * scale, a1[4 * g + 3] * scale);
    }
}
// The two halves of a row trade groups: afterwards (pk[t][2gp], pk[t][2gp + 1]) are the 16 bytes of features
// 32t + 16gp + 8h .. + 7 of the lane's row - a 16-byte row piece, and the MFMA operand fragment of k-step 2t + gp.
__device__ __forceinline__ void swap_row_halves(uint2 (&pk)[2][4]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
            // x = group 2gp, y = group 2gp+1: afterwards half 0 holds (its x, the partner's x), half 1 (the partner's y, its y)
            half_swap(pk[t][2 * gp].x, pk[t][2 * gp + 1].x);
            half_swap(pk[t][2 * gp].y, pk[t][2 * gp + 1].y);
        }
}

constexpr float kAttnLazy = 16.0f;   // a block raises the lazy reference maximum when it exceeds it by more than 2^kAttnLazy

// One key block [key0, key0 + 32) against the wave's 32 queries (q0w .. q0w + 31; this lane: qi, half h).
//   qf: the Q fragments; koff / voff: the lane's LDS byte addresses of its K fragments / transposing V reads inside a slot,
//   blk: byte offset of the block's first row from the slot base; cpos / cneg, nsl, nsl2, scale2s: see attn_bf16_kernel;
//   o0 / o1, mref2, l2a / l2b: the running output, reference maximum (negated, exp2 units) and row sums;
//   mid(): called once after the V reads are issued (the caller's prefetch slot); ST / ts / ta: phase stamps (experiments).
template <bool kResidentC, bool ST, typename Mid>
__device__ __forceinline__ void attn_bf16_key_block(const bf16x8 (&qf)[4], const uint32_t (&koff)[4], const uint32_t (&voff)[2],
                                                    uint32_t blk, int key0, int q0w, int qi, int h, int klen, float nsl,
                                                    float nsl2, float scale2s, const f32x16& cpos, const f32x16& cneg,
                                                    f32x16& o0, f32x16& o1, float& mref2, float& l2a, float& l2b, Mid&& mid,
                                                    [[maybe_unused]] uint64_t (&ts)[6]) {
    constexpr float kLazy = kAttnLazy;
    const float ninf = -__builtin_huge_valf();
    [[maybe_unused]] uint64_t ta = 0, tb = 0, tc = 0, td = 0;

    if constexpr (ST) { ta = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); }
    // the 4 K fragments are requested together (opaque asm reads: hipcc would sink each next to its MFMA and wait
    // for it there); the 8 transposed V reads follow the score MFMAs and land during the softmax
    bf16x8 kf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) lds_read_b128_asm<0>(kf[ks], koff[ks] + blk);
    f32x16 s;
    float base2;                                   // exp2 argument = fma(s, scale2, base2)
    const float d0 = (float)(key0 + 4 * h - qi);   // key - query of accumulator register 0
    if constexpr (kResidentC) {
        lds_wait<0>();
        __builtin_amdgcn_sched_barrier(0);
        if (key0 == q0w) {                          // wave-uniform: the one block that straddles the diagonal
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = fabsf(d0 + (float)((r & 3) + 8 * (r >> 2))) * nsl;
            base2 = mref2;
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[0], qf[0], s, 0, 0, 0);
        } else if (key0 < q0w) {                    // keys before the queries: |d| = -(d0 + c_r)
            base2 = fmaf(-nsl2, d0, mref2);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[0], qf[0], cneg, 0, 0, 0);
        } else {
            base2 = fmaf(nsl2, d0, mref2);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[0], qf[0], cpos, 0, 0, 0);
        }
#pragma unroll
        for (int ks = 1; ks < 4; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], s, 0, 0, 0);
    } else {
        if (key0 == q0w) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = fabsf(d0 + (float)((r & 3) + 8 * (r >> 2))) * nsl;
            base2 = mref2;
        } else if (key0 < q0w) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = cneg[r];
            base2 = fmaf(-nsl2, d0, mref2);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = cpos[r];
            base2 = fmaf(nsl2, d0, mref2);
        }
        lds_wait<0>();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], s, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    u32x2 vr[2][2][2];   // [st][dim tile][run]: keys key0 + 16st + 4h + 0..3 (run 0) and + 8 (run 1) of this lane's dim
    static_for<0, 8>([&](auto ic) {
        constexpr int i8 = decltype(ic)::value, st = i8 >> 2, dt = (i8 >> 1) & 1, run = i8 & 1;
        lds_read_b64_tr_b16_asm<(16 * st + 8 * run) * 128>(vr[st][dt][run], voff[dt] + blk);
    });
    mid();
    if constexpr (ST) { __builtin_amdgcn_sched_barrier(0); tb = __builtin_readcyclecounter(); ts[2] += tb - ta; }
    if (key0 + 32 > klen) {   // the one block that straddles key_len (wave-uniform test)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = key0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            s[r] = key < klen ? s[r] : ninf;
        }
    }
    float bmax = max3_raw(s[0], s[1], s[2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) bmax = max3_raw(bmax, s[r], s[r + 1]);
    // this lane half's block maximum in exp2 units relative to m_ref (the base differs between the halves), then the row's
    bmax = xhalf_max_swap(fmaf(fmaxf(bmax, s[15]), scale2s, base2));
    const bool first = key0 == 0;
    if (first || __builtin_amdgcn_ballot_w64(bmax > kLazy) != 0) {   // wave-uniform
        // raise the reference to this block's row maximum (block 0: set it), rescale what was accumulated
        const float delta = first ? bmax : fmaxf(bmax, 0.f);
        const float alpha = first ? 1.0f : __builtin_amdgcn_exp2f(-delta);
        mref2 -= delta;
        base2 -= delta;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            o0[r] *= alpha;
            o1[r] *= alpha;
        }
        l2a *= alpha;
        l2b *= alpha;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        s[2 * j] = __builtin_amdgcn_exp2f(fmaf(s[2 * j], scale2s, base2));
        s[2 * j + 1] = __builtin_amdgcn_exp2f(fmaf(s[2 * j + 1], scale2s, base2));
        l2a += s[2 * j];
        l2b += s[2 * j + 1];
    }
    // P -> bf16 B-operand fragments (k-step st = registers 8st .. 8st+7)
    union { uint32_t u[4]; bf16x8 f; } pf[2];
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int e = 0; e < 4; ++e) pf[st].u[e] = pack_bf16x2(s[8 * st + 2 * e], s[8 * st + 2 * e + 1]);
    if constexpr (ST) { __builtin_amdgcn_sched_barrier(0); tc = __builtin_readcyclecounter(); ts[3] += tc - tb; }
    lds_wait<0>();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        union { uint32_t u[4]; bf16x8 f; } a0, a1;
        a0.u[0] = vr[st][0][0][0]; a0.u[1] = vr[st][0][0][1]; a0.u[2] = vr[st][0][1][0]; a0.u[3] = vr[st][0][1][1];
        a1.u[0] = vr[st][1][0][0]; a1.u[1] = vr[st][1][0][1]; a1.u[2] = vr[st][1][1][0]; a1.u[3] = vr[st][1][1][1];
        o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.f, pf[st].f, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1.f, pf[st].f, o1, 0, 0, 0);
    }
    if constexpr (ST) { __builtin_amdgcn_sched_barrier(0); td = __builtin_readcyclecounter(); ts[4] += td - tc; }
}

}  // namespace
