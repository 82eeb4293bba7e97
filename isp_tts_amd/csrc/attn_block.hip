// One attention block of the bf16 no-tape forward at N <= 128 positions per batch item, in ONE kernel:
//     q/kv = rows [Wq; Wkv]^T  ->  ALiBi multi-query attention  ->  out = residual + mask * (attn Wo^T)
// It replaces three launches (ispk_gemm_bf16 with a bf16 output, ispk_alibi_mqa_attn_bf16, ispk_gemm_bf16 with the
// ISPK_EP_MASK_ACC + residual epilogue) and computes, bit for bit, what they compute:
//   * every projection accumulates its K/16 k-steps in order from zero with v_mfma_f32_32x32x16_bf16, weights as the A
//     operand and rows as the B operand, k = 16 ks + 8 h + j in lane half h - the panel GEMM's order (gemm.hip);
//   * q/kv and the attention output are rounded to bf16 exactly where the three launches store them;
//   * the key blocks run through attn_core.h, the code attn_bf16_kernel runs;
//   * the output goes through store_rows_f32 (gemm_common.h), the panel GEMM's epilogue.
//
// A workgroup owns one (batch item, 64-query tile) for all H heads: 2 H waves, wave w = head w % H, query half w / H.
//   phase 0  the batch item's rows (<= 128 x dim bf16) are staged in LDS once;
//   phase A  every projection is "one 32-feature tile x two 32-row blocks" per wave, so that a weight fragment is read from
//            memory once per workgroup (the workgroup is bound by the weight bytes its CU can pull in, not by its MFMAs).
//            Weights come straight from memory as operand fragments: in the k-step chunked image (ispk_chunk_k16_bf16) a
//            wave's fragment load is one contiguous KB.  Wave w projects 32 of its head's 64 Q features for the tile's 64
//            rows, keeps the piece of its own query half in registers (the score MFMA's operand) and hands the other to the
//            head's other wave through LDS; waves 0 .. 7 then project one of the four K / V feature tiles for one 64-row
//            group, written to LDS in the swizzled layout the key-block code reads.  The q/kv rows also go to memory (the
//            layer returns them): Q rows by their tile, K/V rows by the tile whose index is their 64-row group;
//   phase B  attention over the <= 4 key blocks in LDS; the normalised output, rounded to bf16, goes to an LDS tile;
//   phase C  wave w multiplies the tile's 64 rows with Wo's output features 32 w .. + 31 and applies the epilogue.
// With finished q/kv rows as the input (x == NULL) phase 0 / A only copy K/V into LDS and load the Q fragments.
#include "attn_core.h"
#include "gemm_common.h"

namespace {

constexpr int kAbKeys = 128;                     // N <= 128: the whole key range is one resident chunk
constexpr int kAbKvBytes = kAbKeys * 128;        // K (and V): [128 keys][128 B], swizzled as attention.hip's ring slot

struct AttnBlockParams {
    const uint16_t* x;        // normalised rows [B * N][ldx], or nullptr: qkv holds finished rows
    int64_t ldx;
    const uint16_t* wqkv_c;   // [dim / 16][64 H + 128][16]
    uint16_t* qkv;            // [B * N][ld_qkv]: written (x given) or read
    int64_t ld_qkv;
    const float* slopes;
    const int64_t* key_len;
    const uint16_t* wo_c;     // [dim / 16][dim][16]
    const float* resid;
    int64_t ldr;
    const uint8_t* mask;      // [B * N] or nullptr
    float* out;
    int64_t ldo;
    int N;
};

template <int H> struct AbLayout {
    static constexpr int D = 64 * H, KS = D / 16, W = D + 128;
    static constexpr int XLD = D * 2 + 16;                      // staged row: 16 B of padding keeps fragment reads conflict-free
    static constexpr int kRows = kAbKeys * XLD;                 // phase 0 / A: the batch item's rows
    static constexpr int kQx = 2 * H * 2048;                    // phase A -> B: 2 x 64 x 16 B of Q pieces per wave, behind the rows
    static constexpr int kOut = 64 * XLD + 2 * H * kStageBytes; // phase B / C: attention output tile + epilogue patches
    static constexpr size_t kLds = 2 * kAbKvBytes + (kRows + kQx > kOut ? kRows + kQx : kOut);
    static_assert(kLds <= 160 * 1024, "LDS budget");
};

// The chunked weight's operand fragments of one 32-feature tile, all k-steps: KS loads of 16 bytes a lane (one contiguous KB
// a wave each), issued together.  wc: [KS][wrows][16].
template <int KS>
__device__ __forceinline__ void load_w_tile(bf16x8 (&wf)[KS], const uint16_t* __restrict__ wc, int wrows, int feat0, int l31, int h) {
    const uint16_t* wp = wc + ((int64_t)(feat0 + l31) * 16 + 8 * h);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wf[ks] = *reinterpret_cast<const bf16x8*>(wp + (int64_t)ks * wrows * 16);
}

// acc0 / acc1 = one 32-feature tile of two 32-row blocks: sum over k-steps, in order from zero, of W fragment x row fragment.
// wf: the tile's weight fragments (each is read from memory ONCE for both row blocks); rows0 / rows1: the lane's row of each
// block in LDS (+ 16 h), row-major bf16.  next(ks, wf[ks]) may refill the fragment just used with a later projection's.
template <int KS, typename Next>
__device__ __forceinline__ void project_rows2(bf16x8 (&wf)[KS], const char* rows0, const char* rows1, f32x16& acc0, f32x16& acc1,
                                              Next&& next) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(rows0 + ks * 32);
        const bf16x8 x1 = *reinterpret_cast<const bf16x8*>(rows1 + ks * 32);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[ks], x0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[ks], x1, acc1, 0, 0, 0);
        next(ks, wf[ks]);
    }
}

// The 16-byte piece gp of tile t after swap_row_halves: features 16 gp + 8 h .. + 7 of the tile, the lane's row
__device__ __forceinline__ u32x4 row_piece(const uint2 (&pk)[2][4], int t, int gp) {
    u32x4 v;
    v.x = pk[t][2 * gp].x; v.y = pk[t][2 * gp].y; v.z = pk[t][2 * gp + 1].x; v.w = pk[t][2 * gp + 1].y;
    return v;
}
__device__ __forceinline__ u32x4 pick(bool second, const u32x4& a, const u32x4& b) {   // wave-uniform choice, per register
    u32x4 v;
    v.x = second ? b.x : a.x; v.y = second ? b.y : a.y; v.z = second ? b.z : a.z; v.w = second ? b.w : a.w;
    return v;
}

template <int H>
__global__ __launch_bounds__(128 * H) void attn_block_short_kernel(AttnBlockParams p) {
    using L = AbLayout<H>;
    constexpr int D = L::D, KS = L::KS, W = L::W, XLD = L::XLD, NT = 128 * H;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* const Kl = smem_raw;                       // [128 rows][128 B]
    char* const Vl = smem_raw + kAbKvBytes;
    char* const Xs = smem_raw + 2 * kAbKvBytes;      // phase 0 / A: [128][XLD]; phase B / C: [64][XLD] output tile + patches
    char* const Os = Xs;
    char* const Qx = Xs + L::kRows;                  // phase A -> B: the Q pieces a wave hands to its head's other wave

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int head = wave % H, qhalf = wave / H;
    const int l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, qt = blockIdx.x, N = p.N;
    const int q0 = qt * 64 + qhalf * 32, qi = q0 + l31;      // q0 + 31 <= 127
    const bool active = q0 < N;                              // wave-uniform: the wave has at least one query row
    int klen = p.key_len ? (int)p.key_len[b] : N;
    klen = klen < 1 ? 1 : (klen > N ? N : klen);
    const int64_t row0 = (int64_t)b * N;

    bf16x8 qf[4];
    bf16x8 wf[KS];
    if (p.x) {
        // ---- phase 0: rows 0 .. 127 of the batch item (rows >= N: row N - 1 again, a valid row that is never stored); the
        // weight fragments of the wave's Q tile are requested behind them and land while the rows are staged
        constexpr int CPR = D / 8, PER = kAbKeys * CPR / NT;   // 16-byte chunks per row; per thread (8)
        static_assert(kAbKeys * CPR % NT == 0, "row staging");
        u32x4 t[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int id = tid + NT * i, r = id / CPR, c = id - r * CPR;
            const int row = r < N ? r : N - 1;
            t[i] = *reinterpret_cast<const u32x4*>(p.x + (row0 + row) * p.ldx + c * 8);
        }
        // Q: wave (head, qhalf) projects features head * 64 + 32 qhalf .. + 31 of BOTH 32-row halves of the tile
        load_w_tile<KS>(wf, p.wqkv_c, W, head * 64 + qhalf * 32, l31, h);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int id = tid + NT * i, r = id / CPR, c = id - r * CPR;
            *reinterpret_cast<u32x4*>(Xs + r * XLD + c * 16) = t[i];
        }
        __syncthreads();

        // ---- phase A.  K / V: wave w < 8 projects feature tile w & 3 (K 0..31, K 32..63, V 0..31, V 32..63) of the 64-row
        // group w >> 2; its weight fragments replace the Q tile's as those are used up.
        const int kvf = wave & 3, kvg = wave >> 2;
        const bool kv = wave < 8 && kvg * 64 < N;
        f32x16 a0, a1;
        uint2 pk[2][4];
        const char* xq = Xs + (qt * 64 + l31) * XLD + h * 16;
        if (kv) {
            const uint16_t* wp = p.wqkv_c + ((int64_t)(D + 32 * kvf + l31) * 16 + 8 * h);
            project_rows2<KS>(wf, xq, xq + 32 * XLD, a0, a1, [&](int ks, bf16x8& w) {
                w = *reinterpret_cast<const bf16x8*>(wp + (int64_t)ks * W * 16);
            });
        } else {
            project_rows2<KS>(wf, xq, xq + 32 * XLD, a0, a1, [](int, bf16x8&) {});
        }
        pack_rows_bf16(a0, a1, 1.0f, pk);   // pk[rh]: row half rh
        swap_row_halves(pk);
        // the wave keeps the pieces of its own query half (k-steps 2 qhalf, 2 qhalf + 1 of its head's score product) and
        // hands the other half's to the head's other wave; all four go to memory
        u32x4 own[2], oth[2];    // (selects, not indexing by qhalf: a run-time index would put the arrays in scratch)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
            const u32x4 v0 = row_piece(pk, 0, gp), v1 = row_piece(pk, 1, gp);
            uint16_t* qdst = p.qkv + (row0 + qt * 64 + l31) * p.ld_qkv + head * 64 + qhalf * 32 + gp * 16 + 8 * h;
            if (qt * 64 + l31 < N) *reinterpret_cast<u32x4*>(qdst) = v0;
            if (qt * 64 + 32 + l31 < N) *reinterpret_cast<u32x4*>(qdst + 32 * p.ld_qkv) = v1;
            own[gp] = pick(qhalf, v0, v1);
            *reinterpret_cast<u32x4*>(Qx + ((wave * 2 + gp) * 64 + lane) * 16) = pick(qhalf, v1, v0);
        }
        if (kv) {
            const char* xk = Xs + (kvg * 64 + l31) * XLD + h * 16;
            project_rows2<KS>(wf, xk, xk + 32 * XLD, a0, a1, [](int, bf16x8&) {});
            pack_rows_bf16(a0, a1, 1.0f, pk);
            swap_row_halves(pk);
            const int isv = kvf >> 1;
#pragma unroll
            for (int rh = 0; rh < 2; ++rh) {
                const int r = kvg * 64 + rh * 32 + l31;
                const int sw = isv ? ((r >> 1) & 1) << 2 : (r >> 1) & 7;
                char* dst = (isv ? Vl : Kl) + r * 128;
                const bool mine = kvg == qt && r < N;       // K/V rows are stored by the tile that owns their 64-row group
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) {
                    const u32x4 v = row_piece(pk, rh, gp);
                    const int c = 4 * (kvf & 1) + 2 * gp + h;   // logical 16-byte chunk: features 8 c .. 8 c + 7
                    *reinterpret_cast<u32x4*>(dst + ((c ^ sw) << 4)) = v;
                    if (mine) *reinterpret_cast<u32x4*>(p.qkv + (row0 + r) * p.ld_qkv + D + 64 * isv + 8 * c) = v;
                }
            }
        }
        __syncthreads();   // K / V and the handed-over Q pieces are complete; the staged rows are dead
        const int other = (1 - qhalf) * H + head;             // the head's other wave holds feature tile 1 - qhalf
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) oth[gp] = *reinterpret_cast<const u32x4*>(Qx + ((other * 2 + gp) * 64 + lane) * 16);
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {      // k-steps 2 t + gp of the score product: feature tile t of the head
            qf[gp] = __builtin_bit_cast(bf16x8, pick(qhalf, own[gp], oth[gp]));
            qf[2 + gp] = __builtin_bit_cast(bf16x8, pick(qhalf, oth[gp], own[gp]));
        }
    } else {
        // ---- finished q/kv rows: K / V into LDS (rows >= N: row N - 1 again, masked by key_len <= N), Q fragments from memory
        constexpr int PER = (kAbKeys * 16 + NT - 1) / NT;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int id = tid + NT * i;
            if (id < kAbKeys * 16) {
                const int r = id >> 4, isv = (id >> 3) & 1, c = id & 7;
                const int row = r < N ? r : N - 1;
                const int sw = isv ? ((r >> 1) & 1) << 2 : (r >> 1) & 7;
                const u32x4 v = *reinterpret_cast<const u32x4*>(p.qkv + (row0 + row) * p.ld_qkv + D + 64 * isv + 8 * c);
                *reinterpret_cast<u32x4*>((isv ? Vl : Kl) + r * 128 + ((c ^ sw) << 4)) = v;
            }
        }
        const int qrow = qi < N ? qi : N - 1;
        const uint16_t* qp = p.qkv + (row0 + qrow) * p.ld_qkv + head * 64 + h * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 16);
        __syncthreads();   // K / V are complete
    }

    // ---- phase B: attention (attn_core.h), the wave's 32 queries against the key blocks below key_len
    if (active) {
        constexpr float kLog2e = 1.4426950408889634f;
        const float scale2 = 0.125f * kLog2e;
        const float nsl = -8.0f * p.slopes[head];
        const float nsl2 = nsl * scale2;
        f32x16 cpos, cneg;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            cpos[r] = nsl * (float)((r & 3) + 8 * (r >> 2));
            cneg[r] = -cpos[r];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(cpos[r]), "+v"(cneg[r]));
        const float scale2s = [&] { float c = scale2; asm volatile("" : "+s"(c)); return c; }();
        const uint32_t kl_base = lds_addr(Kl), vl_base = lds_addr(Vl);
        uint32_t koff[4], voff[2];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) koff[ks] = kl_base + l31 * 128 + (((2 * ks + h) ^ ((l31 >> 1) & 7)) << 4);
        const int qq = (lane & 15) >> 2, pp = lane & 3, dh = (lane >> 4) & 1;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
            voff[dt] = vl_base + (4 * h + qq) * 128 + (((4 * dt + 2 * dh + (pp >> 1)) ^ ((qq >> 1) << 2)) << 4) + 8 * (pp & 1);

        f32x16 o0, o1;
#pragma unroll
        for (int r = 0; r < 16; ++r) o0[r] = o1[r] = 0.f;
        float mref2 = 0.f, l2a = 0.f, l2b = 0.f;
        uint64_t ts[6] = {};
#pragma unroll 1
        for (int kblk = 0; kblk < kAbKeys / 32; ++kblk) {
            const int key0 = kblk * 32;
            if (key0 >= klen) break;  // wave-uniform
            attn_bf16_key_block<true, false>(qf, koff, voff, (uint32_t)(kblk * 32 * 128), key0, q0, qi, h, klen, nsl, nsl2, scale2s,
                                             cpos, cneg, o0, o1, mref2, l2a, l2b, [] {}, ts);
        }
        const float inv = 1.0f / xhalf_sum(l2a + l2b);
        uint2 pk[2][4];
        pack_rows_bf16(o0, o1, inv, pk);
        swap_row_halves(pk);
        char* orow = Os + (qhalf * 32 + l31) * XLD + (head * 64 + 8 * h) * 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(orow + 32 * i) = row_piece(pk, i >> 1, i & 1);
    }
    // ---- phase C: to_out.  Wave w: output features 32 w .. + 31 of both 32-row halves of the tile (Wo's fragments are read
    // once, and requested before the barrier), then the panel GEMM's epilogue.
    load_w_tile<KS>(wf, p.wo_c, D, wave * 32, l31, h);
    __syncthreads();   // the output tile is complete
    {
        f32x16 a0, a1;
        const char* xo = Os + l31 * XLD + h * 16;
        project_rows2<KS>(wf, xo, xo + 32 * XLD, a0, a1, [](int, bf16x8&) {});
        GemmParams g{};
        g.C = p.out; g.ldc = p.ldo; g.resid = p.resid; g.ldr = p.ldr; g.mask = p.mask;
        g.M = (int)(row0 + N);                 // rows of later batch items are not this workgroup's
        g.N = D; g.K = D;
        const int mw0 = (int)(row0 + qt * 64), n0 = wave * 32;
        char* stage = Os + 64 * XLD + wave * kStageBytes;
        auto epilogue = [&](auto epc) {
            constexpr int EP = decltype(epc)::value;
#pragma unroll
            for (int rh = 0; rh < 2; ++rh) {
                if (qt * 64 + rh * 32 >= N) break;       // wave-uniform: no row of this half exists
                const int mh = mw0 + 32 * rh, m = mh + l31;
                const float mk = (EP & ISPK_EP_MASK_ACC) && m < g.M ? (p.mask[m] ? 1.0f : 0.0f) : 1.0f;
                float mo4[4];
                mask_rows<EP>(g, mh, lane, mo4);
                float4 r4[4];
                resid_prefetch<EP>(g, mh, n0, lane, r4);
                store_rows_f32<EP>(g, stage, mh, n0, rh ? a1 : a0, mk, lane, nullptr, r4, mo4);
            }
        };
        if (p.mask) {
            g.flags = ISPK_EP_MASK_ACC;
            epilogue(std::integral_constant<int, ISPK_EP_MASK_ACC | kEpResid>{});
        } else {
            epilogue(std::integral_constant<int, kEpResid>{});
        }
    }
}

template <int H>
int32_t launch_attn_block(const AttnBlockParams& p, int B, hipStream_t st) {
    constexpr size_t lds = AbLayout<H>::kLds;
    ISPK_RESERVE_LDS(&attn_block_short_kernel<H>, lds, "attn_block");
    hipLaunchKernelGGL(attn_block_short_kernel<H>, dim3((p.N + 63) / 64, B), dim3(128 * H), lds, st, p);
    return ispk_launch_status();
}

}  // namespace

extern "C" int32_t ispk_attn_block_short_bf16(const uint16_t* x, int64_t ldx, const uint16_t* Wqkv_chunks, uint16_t* qkv,
                                              int64_t ld_qkv, const float* slopes, const int64_t* key_len,
                                              const uint16_t* Wo_chunks, const float* resid, int64_t ldr, const uint8_t* mask,
                                              float* out, int64_t ldo, int32_t B, int32_t N, int32_t H, ispk_stream_t stream) {
    ISPK_REQUIRE(qkv && slopes && Wo_chunks && resid && out && (!x || Wqkv_chunks), ISPK_E_NULL, "attn_block: null pointer");
    ISPK_REQUIRE(H == 4 || H == 6, ISPK_E_UNSUPPORTED, "attn_block: H=%d (built for 4 heads / dim 256 and 6 heads / dim 384)", H);
    ISPK_REQUIRE(B >= 0 && N >= 1 && N <= kAbKeys, ISPK_E_SHAPE, "attn_block: bad shape B=%d N=%d (1 <= N <= 128)", B, N);
    ISPK_REQUIRE(B <= 65535, ISPK_E_SHAPE, "attn_block: B=%d exceeds the grid limit 65535", B);
    ISPK_REQUIRE((int64_t)B * N <= INT32_MAX, ISPK_E_SHAPE, "attn_block: B * N exceeds int32");
    const int D = 64 * H;
    ISPK_REQUIRE((!x || ldx >= D) && ld_qkv >= D + 128 && ldr >= D && ldo >= D, ISPK_E_SHAPE, "attn_block: leading strides too small");
    ISPK_REQUIRE((!x || ldx % 8 == 0) && ld_qkv % 8 == 0 && ldr % 4 == 0 && ldo % 4 == 0, ISPK_E_ALIGN,
                 "attn_block: ldx / ld_qkv must be multiples of 8, ldr / ldo of 4");
    ISPK_REQUIRE(ispk_aligned(x, 16) && ispk_aligned(Wqkv_chunks, 16) && ispk_aligned(qkv, 16) && ispk_aligned(Wo_chunks, 16) &&
                     ispk_aligned(resid, 16) && ispk_aligned(out, 16),
                 ISPK_E_ALIGN, "attn_block: pointers must be 16-byte aligned");
    if (B == 0) return 0;
    const AttnBlockParams p{x, ldx, Wqkv_chunks, qkv, ld_qkv, slopes, key_len, Wo_chunks, resid, ldr, mask, out, ldo, N};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return H == 6 ? launch_attn_block<6>(p, B, st) : launch_attn_block<4>(p, B, st);
}
