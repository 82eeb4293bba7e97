// The small steps between the transformer stacks of AcousticModel.forward / .infer, as gfx950 kernels (SURVEY rows a13,
// a15, f3): token embedding + key mask, the flow predictor's time embedding, soft length regulation (optionally from a
// soft path generated on the fly) with the decoder lengths and mask.  In the reference each is a handful of ATen
// element-wise launches or a library bmm; here every one is a single launch on the caller's stream.
#include "common.h"
#include "dec_len.h"

namespace {

// ------------------------------------------------------------------------------------------------ token embedding + mask
// models/acoustic/model.py:131-134: emb = Embedding(text) (a row gather; row 0 of the table is the padding row and is
// simply read), enc_mask = arange(L) < text_len[:, None] (utils/functions.py:61-65).
// One wave per token row: D/4 float4 loads of the table row, same stores.  Ids outside [0, vocab) cannot raise on the
// device like F.embedding does on the host; they read the padding row (row 0).
__global__ __launch_bounds__(256) void embed_tokens_kernel(const int64_t* __restrict__ text, const float* __restrict__ table,
                                                           int64_t ld_table, int vocab, const int64_t* __restrict__ text_len,
                                                           float* __restrict__ emb, uint8_t* __restrict__ mask, int rows,
                                                           int L, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    int64_t id = text[row];
    id = (id < 0 || id >= vocab) ? 0 : id;
    const f32x4* src = reinterpret_cast<const f32x4*>(table + id * ld_table);
    f32x4* dst = reinterpret_cast<f32x4*>(emb + (int64_t)row * D);
    for (int c = lane; c < D / 4; c += 64) dst[c] = src[c];
    if (mask && lane == 0) {
        const int b = row / L, l = row - b * L;
        mask[row] = text_len ? (uint8_t)(l < text_len[b]) : (uint8_t)1;
    }
}

// The same lookup with the first layer's q/kv rows gathered beside it (ispk_embed_tokens_qkv): the text encoder's first
// attention_norm + [to_q; to_kv] projection reads nothing but Embedding(text), so its result is one of `vocab` distinct rows -
// staged once per weight version as qkv_table bf16 [vocab][N] - and the LayerNorm and GEMM launches become this second gather.
// Same id clamping, same mask; each lane moves 16-byte vectors of both rows.
__global__ __launch_bounds__(256) void embed_tokens_qkv_kernel(const int64_t* __restrict__ text, const float* __restrict__ table,
                                                               int64_t ld_table, int vocab, const int64_t* __restrict__ text_len,
                                                               float* __restrict__ emb, uint8_t* __restrict__ mask,
                                                               const uint16_t* __restrict__ qkv_table, int64_t ld_qkv_table,
                                                               uint16_t* __restrict__ qkv, int rows, int L, int D, int N) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    int64_t id = text[row];
    id = (id < 0 || id >= vocab) ? 0 : id;
    const f32x4* src = reinterpret_cast<const f32x4*>(table + id * ld_table);
    f32x4* dst = reinterpret_cast<f32x4*>(emb + (int64_t)row * D);
    for (int c = lane; c < D / 4; c += 64) dst[c] = src[c];
    const f32x4* qsrc = reinterpret_cast<const f32x4*>(qkv_table + id * ld_qkv_table);
    f32x4* qdst = reinterpret_cast<f32x4*>(qkv + (int64_t)row * N);
    for (int c = lane; c < N / 8; c += 64) qdst[c] = qsrc[c];
    if (mask && lane == 0) {
        const int b = row / L, l = row - b * L;
        mask[row] = text_len ? (uint8_t)(l < text_len[b]) : (uint8_t)1;
    }
}

// ------------------------------------------------------------------------------------------------ speaker embedding
// models/acoustic/model.py:205-207 (`infer`): enc_out = enc_out + speaker_embedding(speaker) - nn.Embedding rows broadcast
// over the text axis.  In place, every row of the utterance (padded ones too: the reference adds before any re-masking).
// One wave per row; speaker ids at stride `id_stride` (0: one id for the whole batch).  Ids outside [0, speakers) are
// clamped (the host-side F.embedding would raise).
__device__ __forceinline__ int64_t speaker_row(const int64_t* __restrict__ speaker, int b, int id_stride, int speakers) {
    const int64_t id = speaker[(int64_t)b * id_stride];
    return id < 0 ? 0 : (id >= speakers ? speakers - 1 : id);
}

__global__ __launch_bounds__(256) void add_speaker_kernel(float* __restrict__ x, const float* __restrict__ table, int64_t ld_table,
                                                          int speakers, const int64_t* __restrict__ speaker, int id_stride,
                                                          int rows, int L, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int64_t id = speaker_row(speaker, row / L, id_stride, speakers);
    const f32x4* src = reinterpret_cast<const f32x4*>(table + id * ld_table);
    f32x4* dst = reinterpret_cast<f32x4*>(x + (int64_t)row * D);
    for (int c = lane; c < D / 4; c += 64) {
        f32x4 v = dst[c];
        const f32x4 e = src[c];
        v[0] += e[0]; v[1] += e[1]; v[2] += e[2]; v[3] += e[3];
        dst[c] = v;
    }
}

// The same sum into a second buffer, for the teacher-forced forward (model.py:138-146 with `speaker_encoder` read as
// `speaker_embedding`): the aligner takes the un-added encoder output - and keeps it for its backward - so x must survive.
__global__ __launch_bounds__(256) void add_speaker_out_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                              const float* __restrict__ table, int64_t ld_table, int speakers,
                                                              const int64_t* __restrict__ speaker, int id_stride, int rows,
                                                              int L, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int64_t id = speaker_row(speaker, row / L, id_stride, speakers);
    const f32x4* src = reinterpret_cast<const f32x4*>(table + id * ld_table);
    const f32x4* in = reinterpret_cast<const f32x4*>(x + (int64_t)row * D);
    f32x4* dst = reinterpret_cast<f32x4*>(out + (int64_t)row * D);
    for (int c = lane; c < D / 4; c += 64) {
        f32x4 v = in[c];
        const f32x4 e = src[c];
        v[0] += e[0]; v[1] += e[1]; v[2] += e[2]; v[3] += e[3];
        dst[c] = v;
    }
}

// Its backward for the table: d_table[s][:] = sum over the utterances b with id_b == s, in batch order, of the sum over the
// rows l < text_len[b], in row order, of d_x[b][l][:] (nn.Embedding's backward under the broadcast; the reference's gradient is
// exactly zero on padded rows, so leaving them out changes nothing - and what other backward kernels leave there is never read).
// Two stages, one owner per value, no atomics:
//   1. a workgroup owns kSgRows rows of one utterance x 256 columns; wave w adds rows w, w + 4, ... of the chunk, wave 0 then
//      adds the four waves' sums in wave order -> part[b][chunk][:].  Chunks at or past text_len[b] are neither read nor written.
//   2. a workgroup owns one table row x 256 columns: wave w adds, for the utterances b = w, w + 4, ... of that speaker in batch
//      order, their chunks in row order; wave 0 then adds the four waves' sums in wave order.
constexpr int kSgRows = 16;
__device__ __forceinline__ int speaker_grad_len(const int64_t* __restrict__ text_len, int b, int L) {
    if (!text_len) return L;
    const int64_t n = text_len[b];
    return n < 0 ? 0 : (n > L ? L : (int)n);
}

__global__ __launch_bounds__(256) void speaker_grad_stage1_kernel(const float* __restrict__ d_x, const int64_t* __restrict__ text_len,
                                                                  float* __restrict__ part, int L, int D, int chunks) {
    __shared__ f32x4 sums[3][64];
    const int b = blockIdx.z, chunk = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = speaker_grad_len(text_len, b, L), r0 = chunk * kSgRows;
    if (r0 >= n) return;                                            // (uniform over the workgroup: before any barrier)
    const int r1 = r0 + kSgRows < n ? r0 + kSgRows : n, c = blockIdx.x * 64 + lane;
    const bool live = c < D / 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (live)
        for (int r = r0 + wave; r < r1; r += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(d_x + ((int64_t)b * L + r) * D + 4 * c);
            s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
        }
    if (wave > 0) sums[wave - 1][lane] = s;
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const f32x4 v = sums[w][lane];
            s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
        }
        *reinterpret_cast<f32x4*>(part + ((int64_t)b * chunks + chunk) * D + 4 * c) = s;
    }
}

__global__ __launch_bounds__(256) void speaker_grad_stage2_kernel(const float* __restrict__ part, const int64_t* __restrict__ speaker,
                                                                  int id_stride, const int64_t* __restrict__ text_len,
                                                                  float* __restrict__ d_table, int64_t ld_table, int speakers,
                                                                  int B, int L, int D, int chunks, int accumulate) {
    __shared__ f32x4 sums[3][64];
    const int s = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = blockIdx.y * 64 + lane;
    const bool live = c < D / 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // wave w takes the utterances w, w + 4, ... (the tests on b are wave-uniform); an utterance's chunks are fetched eight at a
    // time, independent loads, and added in row order: with few speakers a row's sum is a chain of B / 4 round trips, not B * chunks
    for (int b = wave; b < B; b += 4) {
        if (speaker_row(speaker, b, id_stride, speakers) != s) continue;
        const int nk = (speaker_grad_len(text_len, b, L) + kSgRows - 1) / kSgRows;
        const float* src = part + (int64_t)b * chunks * D + 4 * c;
        for (int k0 = 0; k0 < nk && live; k0 += 8) {
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k0 + u < nk) v[u] = *reinterpret_cast<const f32x4*>(src + (int64_t)(k0 + u) * D);
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k0 + u < nk) { acc[0] += v[u][0]; acc[1] += v[u][1]; acc[2] += v[u][2]; acc[3] += v[u][3]; }
        }
    }
    if (wave > 0) sums[wave - 1][lane] = acc;
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const f32x4 v = sums[w][lane];
            acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
        }
        f32x4* dst = reinterpret_cast<f32x4*>(d_table + (int64_t)s * ld_table + 4 * c);
        if (accumulate) {
            const f32x4 old = *dst;
            acc[0] += old[0]; acc[1] += old[1]; acc[2] += old[2]; acc[3] += old[3];
        }
        *dst = acc;
    }
}

// ------------------------------------------------------------------------------------------------ time embedding
// modules/transformer/embeddings.py:131-157 as built at temporal_adaptor.py:87-89 (freq_dim 64, with_steps):
//   f = [t, sin(t * freq_scale * inv_freq[0..H)), cos(...)]  (1 + 2H values; the reference multiplies in this order)
//   out = W1 silu(W0 f + b0) + b1
// One wave per time value; lane j < E owns hidden unit j, then output j (E <= 64).
__global__ __launch_bounds__(64) void time_embedding_kernel(const float* __restrict__ t, const float* __restrict__ inv_freq,
                                                            const float* __restrict__ freq_scale, int H,
                                                            const float* __restrict__ w0, const float* __restrict__ b0,
                                                            const float* __restrict__ w1, const float* __restrict__ b1,
                                                            int E, float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ float f[1 + 2 * 64];
    __shared__ float h[64];
    const int n = blockIdx.x, j = threadIdx.x;
    const float pos = t[n], fs = freq_scale[0];
    if (j == 0) f[0] = pos;
    for (int i = j; i < H; i += 64) {
        const float a = pos * fs * inv_freq[i];
        f[1 + i] = sinf(a);
        f[1 + H + i] = cosf(a);
    }
    __syncthreads();
    const int K0 = 1 + 2 * H;
    if (j < E) {
        float acc = b0[j];
        for (int k = 0; k < K0; ++k) acc = fmaf(f[k], w0[(int64_t)j * K0 + k], acc);
        h[j] = acc / (1.0f + expf(-acc));   // SiLU
    }
    __syncthreads();
    if (j < E) {
        float acc = b1[j];
        for (int k = 0; k < E; ++k) acc = fmaf(h[k], w1[(int64_t)j * E + k], acc);
        out[(int64_t)n * E + j] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ length regulation
// models/acoustic/modules/temporal_adaptor.py:411-436 (LengthRegulator, soft branch) and :468-478 (generate_soft_path):
//   out[b][y][:] = sum_t A[b][y][t] * x[b][t][:]        A = the aligner's attn_soft (forward), or the soft path
//   dec_len[b]   = (sum_t dur[b][t] + 0.5).long()  [clamped to max_len in forward]
//   soft path (infer): cum = cumsum(dur);  P[t][y] = clamp(cum[t] - y, 0, 1) - clamp(cum[t-1] - y, 0, 1), cum[-1] -> 0 row,
//                      A[y][t] = P[t][y] * (t < enc_len[b]) * (y < dec_len[b])
// A workgroup owns 64 frames x all D features of one utterance; wave w the features [w*D/4, (w+1)*D/4).  Exact fp32
// products on v_mfma_f32_32x32x2_f32 (this feeds the fp32 parity path too).  The token axis streams through LDS in chunks
// of 16; the next chunk is fetched into registers while the current one multiplies.
constexpr int kLrRows = 64, kLrChunk = 16, kLrAld = kLrChunk + 1;

// kSplit (ispk_length_regulate_split_bf16, the bf16 compute path): every fp32 operand value v is split in registers into
// hi = bf16(v) and lo = bf16(v - hi), and a product is three v_mfma_f32_32x32x16_bf16 (hi hi + hi lo + lo hi; the lo lo term
// is below 2^-16 of the product) instead of eight v_mfma_f32_32x32x2_f32: 18 MFMAs of 32 cycles per 16-token chunk and wave
// against 48 of 64 cycles, at ~2^-16 relative error per product - three decimal digits finer than the bf16 GEMMs the result
// feeds.  The fp32 parity path keeps the exact fp32 MFMAs.
// kSplit == 2 (ispk_length_regulate_split_f16, the split-fp16 parity path): the same three products over fp16 terms - 22
// significant bits per operand, fp32-grade results (csrc/split.hip) - on v_mfma_f32_32x32x16_f16.
typedef uint32_t lr_u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 lr_f16x8 __attribute__((ext_vector_type(8)));
template <int kSplit>
__device__ __forceinline__ void lr_split8(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    union { lr_u32x4 u; bf16x8 f; } h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f2 a;
        a.x = v[2 * e]; a.y = v[2 * e + 1];
        if constexpr (kSplit == 2) {
            typedef _Float16 h2 __attribute__((ext_vector_type(2)));
            a.x = __builtin_amdgcn_fmed3f(a.x, -65504.0f, 65504.0f);
            a.y = __builtin_amdgcn_fmed3f(a.y, -65504.0f, 65504.0f);
            h2 ph, pl;
            ph.x = (_Float16)a.x; ph.y = (_Float16)a.y;
            pl.x = (_Float16)(a.x - (float)ph.x); pl.y = (_Float16)(a.y - (float)ph.y);
            h.u[e] = __builtin_bit_cast(uint32_t, ph);
            l.u[e] = __builtin_bit_cast(uint32_t, pl);
        } else {
            typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
            const uint32_t ph = __builtin_bit_cast(uint32_t, __builtin_convertvector(a, bf2));
            f2 r;
            r.x = a.x - __builtin_bit_cast(float, ph << 16);
            r.y = a.y - __builtin_bit_cast(float, ph & 0xffff0000u);
            h.u[e] = ph;
            l.u[e] = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, bf2));
        }
    }
    hi = h.f;
    lo = l.f;
}
template <int kSplit>
__device__ __forceinline__ f32x16 lr_mfma(const bf16x8& a, const bf16x8& b, const f32x16& c) {
    if constexpr (kSplit == 2)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(lr_f16x8, a), __builtin_bit_cast(lr_f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// kQkv (ispk_length_regulate_qkv_bf16): the decoder's first attention_norm + [to_q; to_kv] projection as the epilogue.  The
// finished rows are stored as without it; then their two-pass LayerNorm statistics come from the accumulators (a butterfly over
// the 32 lanes of a row, the four waves' partial sums through LDS), the normalised rows pass through LDS as bf16 - a frame's 384
// features live in four waves, the projection sums over them - and wave w multiplies the 64 frames by columns [128 w, 128 w + 128)
// of the weight, read as MFMA fragments straight from the k-step chunk image (ispk_chunk_k16_bf16: a wave's fragment of one
// step and column tile is 1 KiB contiguous), three steps ahead; the first three are requested before the statistics.  The q/kv
// tile goes back through LDS so that a wave stores whole 1-KiB rows.
struct LrQkv {
    const float* gamma;       // attention_norm of the consuming layer
    const float* beta;
    float eps;
    const uint16_t* w;        // [D / 16][512][16] bf16
    uint16_t* qkv;            // bf16 [B * M][512] at ld elements between rows
    int64_t ld;
};
constexpr int kLrQkvN = 512, kLrQkvLd = kLrQkvN + 8, kLrQkvDepth = 3;
constexpr size_t kLrQkvLds = 16 + (size_t)kLrRows * kLrQkvLd * 2 + (4 * kLrRows + 2 * kLrRows) * sizeof(float);

template <int NT, int kSplit, bool kQkv>   // D = 128 * NT: a wave owns NT 32-feature tiles; kSplit: 0 exact fp32, 1 bf16 terms, 2 fp16 terms
__device__ __forceinline__ void length_regulate_body(const float* __restrict__ align, const float* __restrict__ dur_f,
                                                     const int64_t* __restrict__ dur_i, const int64_t* __restrict__ enc_len,
                                                     const float* __restrict__ x, int64_t ldx, float* __restrict__ out,
                                                     int64_t* __restrict__ dec_len, uint8_t* __restrict__ dec_mask, int M, int L,
                                                     int max_len, int dur_cols, const LrQkv& q) {
    constexpr int D = 128 * NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int64_t& s_dec = *reinterpret_cast<int64_t*>(smem);                      // (all LDS in the dynamic region: a static
    float* As = reinterpret_cast<float*>(smem + 16);                         //  object would shift its 16-byte alignment)
    float* Xs = As + kLrRows * kLrAld;                                       // [16][D]   (As: [64][17] = 4352 B)
    float* cum = Xs + kLrChunk * D;                                          // [L + 1]   (soft path only): cum[t] = sum_{u<t}
    int b = blockIdx.y, bx = blockIdx.x;
    if constexpr (kQkv) {
        // XCD-aware (utterance, frame tile) mapping, as csrc/attention.hip's: workgroups are dealt to the 8 XCDs round-robin in
        // linear order, so the frame tiles of one utterance - which all read its [L][D] rows - would land on 8 different L2s.
        // Within each run of 8 * gridDim.x workgroups, utterance = 8 * run + (linear % 8), tile = (linear / 8) % gridDim.x.
        const int gx = gridDim.x, lin = blockIdx.y * gx + blockIdx.x, run = lin / (8 * gx);
        if ((run + 1) * 8 <= (int)gridDim.y) {            // (a ragged last run keeps the plain mapping)
            const int r = lin - run * 8 * gx;
            b = run * 8 + (r & 7);
            bx = r >> 3;
        }
    }
    const int y0 = bx * kLrRows, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool soft = align == nullptr;

    // ---- decoder length of this utterance (every workgroup of the utterance computes the same value; tile 0 stores it)
    if (wave == 0) {
        int64_t dl;
        if (dur_i) {
            int64_t s = 0;
            for (int t = lane; t < dur_cols; t += 64) s += dur_i[(int64_t)b * dur_cols + t];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            dl = soft_dec_len((float)s);
        } else {
            // sequential fp32 sum in index order (soft_dur_sum, dec_len.h); lane 0 only
            float s = 0.f;
            if (lane == 0) {
                cum[0] = 0.f;
                s = soft_dur_sum<true>(dur_f + (int64_t)b * L, L, 0.f, cum);
            }
            s = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, s)));
            dl = soft_dec_len(s);
        }
        if (max_len >= 0 && dl > max_len) dl = max_len;
        if (lane == 0) {
            s_dec = dl;
            if (bx == 0) dec_len[b] = dl;
        }
    }
    __syncthreads();
    const int64_t dl = s_dec;
    if (dec_mask)
        for (int r = tid; r < kLrRows; r += 256)
            if (y0 + r < M) dec_mask[(int64_t)b * M + y0 + r] = (uint8_t)(y0 + r < dl);
    const int el = enc_len ? (int)enc_len[b] : L;

    f32x16 acc[2][NT];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rt][ct][i] = 0.f;

    const float* xb = x + (int64_t)b * L * ldx;
    const float* ab = soft ? nullptr : align + (int64_t)b * M * L;
    // staging registers: A chunk 64 x 16 = 4 values per thread (thread -> row tid/4, k (tid%4)*4 ..+3); X chunk 16 x D:
    // D/64 float4 per thread (thread -> token tid/16, 4-feature groups (tid%16) + 16*i)
    float ar[4];
    f32x4 xr[D / 64];
    const int a_row = tid >> 2, a_k = (tid & 3) * 4, x_t = tid >> 4, x_c = tid & 15;
    auto fetch = [&](int t0) {
        const int y = y0 + a_row;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + a_k + u;
            float v = 0.f;
            if (y < M && t < L) {
                if (!soft) {
                    v = ab[(int64_t)y * L + t];
                } else {
                    const float fy = (float)y;
                    const float hi = fminf(fmaxf(cum[t + 1] - fy, 0.f), 1.f), lo = fminf(fmaxf(cum[t] - fy, 0.f), 1.f);
                    v = (t < el && y < dl) ? hi - lo : 0.f;
                }
            }
            ar[u] = v;
        }
        const int t = t0 + x_t;
#pragma unroll
        for (int i = 0; i < D / 64; ++i) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (t < L) v = *reinterpret_cast<const f32x4*>(xb + (int64_t)t * ldx + (x_c + 16 * i) * 4);
            xr[i] = v;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int u = 0; u < 4; ++u) As[a_row * kLrAld + a_k + u] = ar[u];
#pragma unroll
        for (int i = 0; i < D / 64; ++i) *reinterpret_cast<f32x4*>(Xs + x_t * D + (x_c + 16 * i) * 4) = xr[i];
    };

    fetch(0);
    for (int t0 = 0; t0 < L; t0 += kLrChunk) {
        __syncthreads();          // everyone is done reading the previous chunk
        stash();
        __syncthreads();
        if (t0 + kLrChunk < L) fetch(t0 + kLrChunk);
        const int r = lane & 31, kh = lane >> 5;
        if constexpr (kSplit != 0) {
            // lane half kh takes tokens 8 kh .. 8 kh + 7 of the chunk in both operands
            bf16x8 ah[2], al[2];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                float av[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) av[e] = As[(32 * rt + r) * kLrAld + 8 * kh + e];
                lr_split8<kSplit>(av, ah[rt], al[rt]);
            }
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                float bv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) bv[e] = Xs[(8 * kh + e) * D + wave * (32 * NT) + ct * 32 + r];
                bf16x8 bh, bl;
                lr_split8<kSplit>(bv, bh, bl);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    acc[rt][ct] = lr_mfma<kSplit>(al[rt], bh, acc[rt][ct]);
                    acc[rt][ct] = lr_mfma<kSplit>(ah[rt], bl, acc[rt][ct]);
                    acc[rt][ct] = lr_mfma<kSplit>(ah[rt], bh, acc[rt][ct]);
                }
            }
            continue;
        }
#pragma unroll
        for (int kk = 0; kk < kLrChunk; kk += 2) {
            const float a0 = As[r * kLrAld + kk + kh], a1 = As[(32 + r) * kLrAld + kk + kh];
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                const float bv = Xs[(kk + kh) * D + wave * (32 * NT) + ct * 32 + r];
                acc[0][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc[0][ct], 0, 0, 0);
                acc[1][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc[1][ct], 0, 0, 0);
            }
        }
    }
    // C/D layout of 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float* ob = out + (int64_t)b * M * D;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int y = y0 + rt * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                if (y < M) ob[(int64_t)y * D + wave * (32 * NT) + ct * 32 + (lane & 31)] = acc[rt][ct][i];
            }

    if constexpr (kQkv) {
        static_assert(NT == 3 && kSplit == 1, "the q/kv epilogue is built for dim 384 on the bf16 path");
        constexpr int kSteps = D / 16, kAld = D + 8, kRing = kLrQkvDepth + 1;
        uint16_t* An = reinterpret_cast<uint16_t*>(smem + 16);               // [64][D + 8] bf16: the normalised rows
        uint16_t* Qs = An;                                                   // [64][520] bf16: the q/kv tile (after the product)
        float* red = reinterpret_cast<float*>(smem + 16 + kLrRows * kLrQkvLd * 2);     // [4 waves][64 rows]
        float* stat = red + 4 * kLrRows;                                     // mean[64], rstd[64]
        const int r = lane & 31, kh = lane >> 5;
        // the weight fragments of this wave's 128 columns: lane (column r, half kh) of column tile ct, step s_
        const uint16_t* wl = q.w + ((int64_t)(wave * 128 + r) * 16 + 8 * kh);
        bf16x8 bq[kRing][4];
        auto wload = [&](int s_, bf16x8 (&dst)[4]) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
                dst[ct] = *reinterpret_cast<const bf16x8*>(wl + ((int64_t)s_ * kLrQkvN + ct * 32) * 16);
        };
        // sum over the 32 lanes of a half-wave of 32 values each, in 31 exchanges: at distance h a lane keeps the half of its
        // values that its bit h selects and adds the partner's; lane l ends with the sum of value l & 31 in v[0]
        auto butterfly = [&](float (&v)[32]) {
            static_for<0, 5>([&](auto st) {
                constexpr int h = 16 >> decltype(st)::value;
                const bool up = (lane & h) != 0;
#pragma unroll
                for (int k = 0; k < h; ++k) {
                    const float keep = up ? v[k + h] : v[k], send = up ? v[k] : v[k + h];
                    v[k] = keep + __shfl_xor(send, h, 64);
                }
            });
        };
        // value k = 16 rt + i of a lane is row 32 rt + (i & 3) + 8 (i >> 2) + 4 kh of the tile; the row whose sum lane l holds:
        const int own = 32 * (r >> 4) + (r & 3) + 8 * ((r & 15) >> 2) + 4 * kh;
        float v[32];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i) v[16 * rt + i] = (acc[rt][0][i] + acc[rt][1][i]) + acc[rt][2][i];
        butterfly(v);
        __syncthreads();          // every wave is done with the token loop's LDS
        red[wave * kLrRows + own] = v[0];
        __syncthreads();
        if (tid < kLrRows) stat[tid] = ((red[tid] + red[kLrRows + tid]) + (red[2 * kLrRows + tid] + red[3 * kLrRows + tid])) * (1.0f / D);
        __syncthreads();
        // (the 4 rows of registers 4 g .. 4 g + 3 are consecutive: one 16-byte read)
        auto rows4 = [&](const float* p, int rt, int g) { return *reinterpret_cast<const f32x4*>(p + 32 * rt + 8 * g + 4 * kh); };
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 m = rows4(stat, rt, g);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * g + e;
                    const float d0 = acc[rt][0][i] - m[e], d1 = acc[rt][1][i] - m[e], d2 = acc[rt][2][i] - m[e];
                    v[16 * rt + i] = (d0 * d0 + d1 * d1) + d2 * d2;
                }
            }
        butterfly(v);
#pragma unroll
        for (int s_ = 0; s_ < kLrQkvDepth; ++s_) wload(s_, bq[s_]);      // (in flight across the rest of the LayerNorm)
        red[wave * kLrRows + own] = v[0];      // (its readers of the first pass are behind the barrier above)
        __syncthreads();
        if (tid < kLrRows) {
            const float var = ((red[tid] + red[kLrRows + tid]) + (red[2 * kLrRows + tid] + red[3 * kLrRows + tid])) * (1.0f / D);
            stat[kLrRows + tid] = 1.0f / sqrtf(var + q.eps);
        }
        __syncthreads();
        float ga[NT], be[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            ga[ct] = q.gamma[wave * (32 * NT) + ct * 32 + r];
            be[ct] = q.beta[wave * (32 * NT) + ct * 32 + r];
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 m = rows4(stat, rt, g), rs = rows4(stat + kLrRows, rt, g);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * g + e, row = 32 * rt + 8 * g + 4 * kh + e;
#pragma unroll
                    for (int ct = 0; ct < NT; ++ct)
                        An[row * kAld + wave * (32 * NT) + ct * 32 + r] = f32_to_bf16((acc[rt][ct][i] - m[e]) * rs[e] * ga[ct] + be[ct]);
                }
            }
        __syncthreads();
        f32x16 qa[2][4];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int i = 0; i < 16; ++i) qa[rt][ct][i] = 0.f;
        static_assert(kSteps % kRing == 0, "the ring is walked in whole turns");
#pragma unroll 1
        for (int s0 = 0; s0 < kSteps; s0 += kRing)
            static_for<0, kRing>([&](auto s_) {
                constexpr int S = decltype(s_)::value;
                if (s0 + S + kLrQkvDepth < kSteps) wload(s0 + S + kLrQkvDepth, bq[(S + kLrQkvDepth) % kRing]);
                const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(An + r * kAld + 16 * (s0 + S) + 8 * kh);
                const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(An + (32 + r) * kAld + 16 * (s0 + S) + 8 * kh);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    qa[0][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bq[S][ct], qa[0][ct], 0, 0, 0);
                    qa[1][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bq[S][ct], qa[1][ct], 0, 0, 0);
                }
            });
        __syncthreads();          // every wave has read its last fragment of An: the q/kv tile takes its place
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    Qs[(32 * rt + (i & 3) + 8 * (i >> 2) + 4 * kh) * kLrQkvLd + wave * 128 + ct * 32 + r] = f32_to_bf16(qa[rt][ct][i]);
        __syncthreads();
        uint16_t* qb = q.qkv + (int64_t)b * M * q.ld;
        for (int row = wave; row < kLrRows; row += 4)       // a wave stores one whole 1-KiB row per instruction
            if (y0 + row < M)
                *reinterpret_cast<u32x4*>(qb + (int64_t)(y0 + row) * q.ld + lane * 8) =
                    *reinterpret_cast<const u32x4*>(Qs + row * kLrQkvLd + lane * 8);
    }
}

template <int NT, int kSplit = 0>
__global__ __launch_bounds__(256) void length_regulate_kernel(const float* __restrict__ align, const float* __restrict__ dur_f,
                                                              const int64_t* __restrict__ dur_i,
                                                              const int64_t* __restrict__ enc_len,
                                                              const float* __restrict__ x, int64_t ldx,
                                                              float* __restrict__ out, int64_t* __restrict__ dec_len,
                                                              uint8_t* __restrict__ dec_mask, int M, int L, int max_len,
                                                              int dur_cols) {
    length_regulate_body<NT, kSplit, false>(align, dur_f, dur_i, enc_len, x, ldx, out, dec_len, dec_mask, M, L, max_len, dur_cols,
                                            LrQkv{});
}

// two workgroups per CU (the second argument is waves per SIMD): 256 registers a lane, 68 KB of LDS
__global__ __launch_bounds__(256, 2) void length_regulate_qkv_kernel(const float* __restrict__ align, const float* __restrict__ dur_f,
                                                                     const int64_t* __restrict__ dur_i,
                                                                     const int64_t* __restrict__ enc_len,
                                                                     const float* __restrict__ x, int64_t ldx,
                                                                     float* __restrict__ out, int64_t* __restrict__ dec_len,
                                                                     uint8_t* __restrict__ dec_mask, int M, int L, int max_len,
                                                                     int dur_cols, LrQkv q) {
    length_regulate_body<3, 1, true>(align, dur_f, dur_i, enc_len, x, ldx, out, dec_len, dec_mask, M, L, max_len, dur_cols, q);
}

}  // namespace

extern "C" int32_t ispk_embed_tokens_f32(const int64_t* text, const float* table, int64_t ld_table, int32_t vocab,
                                         const int64_t* text_len, float* emb, uint8_t* mask, int32_t B, int32_t L,
                                         int32_t D, ispk_stream_t stream) {
    ISPK_REQUIRE(text && table && emb, ISPK_E_NULL, "embed_tokens: null pointer");
    ISPK_REQUIRE(B >= 0 && L >= 1 && D >= 4 && vocab >= 1, ISPK_E_SHAPE, "embed_tokens: bad shape B=%d L=%d D=%d V=%d", B, L,
                 D, vocab);
    ISPK_REQUIRE(D % 4 == 0 && ld_table % 4 == 0 && ld_table >= D && ispk_aligned(table, 16) && ispk_aligned(emb, 16),
                 ISPK_E_ALIGN, "embed_tokens: D / ld_table must be multiples of 4 and table / emb 16-byte aligned");
    if (B == 0) return 0;
    const int rows = B * L;
    hipLaunchKernelGGL(embed_tokens_kernel, dim3((rows + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), text,
                       table, ld_table, vocab, text_len, emb, mask, rows, L, D);
    return ispk_launch_status();
}

extern "C" int32_t ispk_embed_tokens_qkv(const int64_t* text, const float* table, int64_t ld_table, int32_t vocab,
                                         const int64_t* text_len, float* emb, uint8_t* mask, const uint16_t* qkv_table,
                                         int64_t ld_qkv_table, uint16_t* qkv, int32_t B, int32_t L, int32_t D, int32_t N,
                                         ispk_stream_t stream) {
    ISPK_REQUIRE(text && table && emb && qkv_table && qkv, ISPK_E_NULL, "embed_tokens_qkv: null pointer");
    ISPK_REQUIRE(B >= 0 && L >= 1 && D >= 4 && N >= 8 && vocab >= 1, ISPK_E_SHAPE,
                 "embed_tokens_qkv: bad shape B=%d L=%d D=%d N=%d V=%d", B, L, D, N, vocab);
    ISPK_REQUIRE((int64_t)B * L <= INT32_MAX, ISPK_E_SHAPE, "embed_tokens_qkv: B * L = %lld rows exceed int32",
                 (long long)B * L);
    ISPK_REQUIRE(D % 4 == 0 && ld_table % 4 == 0 && ld_table >= D && ispk_aligned(table, 16) && ispk_aligned(emb, 16),
                 ISPK_E_ALIGN, "embed_tokens_qkv: D / ld_table must be multiples of 4 and table / emb 16-byte aligned");
    ISPK_REQUIRE(N % 8 == 0 && ld_qkv_table % 8 == 0 && ld_qkv_table >= N && ispk_aligned(qkv_table, 16) && ispk_aligned(qkv, 16),
                 ISPK_E_ALIGN, "embed_tokens_qkv: N / ld_qkv_table must be multiples of 8 and qkv_table / qkv 16-byte aligned");
    if (B == 0) return 0;
    const int rows = B * L;
    hipLaunchKernelGGL(embed_tokens_qkv_kernel, dim3((rows + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), text,
                       table, ld_table, vocab, text_len, emb, mask, qkv_table, ld_qkv_table, qkv, rows, L, D, N);
    return ispk_launch_status();
}

extern "C" int32_t ispk_add_speaker_f32(float* x, const float* table, int64_t ld_table, int32_t speakers, const int64_t* speaker,
                                        int32_t id_stride, int32_t B, int32_t L, int32_t D, ispk_stream_t stream) {
    ISPK_REQUIRE(x && table && speaker, ISPK_E_NULL, "add_speaker: null pointer");
    ISPK_REQUIRE(B >= 0 && L >= 1 && D >= 4 && speakers >= 1 && (id_stride == 0 || id_stride == 1), ISPK_E_SHAPE,
                 "add_speaker: bad shape B=%d L=%d D=%d speakers=%d id_stride=%d", B, L, D, speakers, id_stride);
    ISPK_REQUIRE(D % 4 == 0 && ld_table % 4 == 0 && ld_table >= D && ispk_aligned(table, 16) && ispk_aligned(x, 16),
                 ISPK_E_ALIGN, "add_speaker: D / ld_table must be multiples of 4 and table / x 16-byte aligned");
    if (B == 0) return 0;
    const int rows = B * L;
    hipLaunchKernelGGL(add_speaker_kernel, dim3((rows + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, table,
                       ld_table, speakers, speaker, id_stride, rows, L, D);
    return ispk_launch_status();
}

extern "C" int32_t ispk_add_speaker_out_f32(const float* x, float* out, const float* table, int64_t ld_table, int32_t speakers,
                                            const int64_t* speaker, int32_t id_stride, int32_t B, int32_t L, int32_t D,
                                            ispk_stream_t stream) {
    ISPK_REQUIRE(x && out && table && speaker, ISPK_E_NULL, "add_speaker_out: null pointer");
    ISPK_REQUIRE(B >= 0 && L >= 1 && D >= 4 && speakers >= 1 && (id_stride == 0 || id_stride == 1), ISPK_E_SHAPE,
                 "add_speaker_out: bad shape B=%d L=%d D=%d speakers=%d id_stride=%d", B, L, D, speakers, id_stride);
    ISPK_REQUIRE(D % 4 == 0 && ld_table % 4 == 0 && ld_table >= D && ispk_aligned(table, 16) && ispk_aligned(x, 16) &&
                     ispk_aligned(out, 16),
                 ISPK_E_ALIGN, "add_speaker_out: D / ld_table must be multiples of 4 and table / x / out 16-byte aligned");
    ISPK_REQUIRE(x != out, ISPK_E_UNSUPPORTED, "add_speaker_out: x and out are the same buffer (ispk_add_speaker_f32 works in place)");
    if (B == 0) return 0;
    const int rows = B * L;
    hipLaunchKernelGGL(add_speaker_out_kernel, dim3((rows + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, out,
                       table, ld_table, speakers, speaker, id_stride, rows, L, D);
    return ispk_launch_status();
}

extern "C" int32_t ispk_speaker_grad_f32(const float* d_x, const int64_t* speaker, int32_t id_stride, const int64_t* text_len,
                                         float* workspace, int64_t workspace_floats, float* d_table, int64_t ld_table,
                                         int32_t speakers, int32_t B, int32_t L, int32_t D, int32_t accumulate,
                                         ispk_stream_t stream) {
    ISPK_REQUIRE(d_x && speaker && workspace && d_table, ISPK_E_NULL, "speaker_grad: null pointer");
    ISPK_REQUIRE(B >= 0 && B <= 65535 && L >= 1 && L <= 512 && D >= 4 && speakers >= 1 && (id_stride == 0 || id_stride == 1),
                 ISPK_E_SHAPE, "speaker_grad: bad shape B=%d L=%d (<= 512) D=%d speakers=%d id_stride=%d", B, L, D, speakers,
                 id_stride);
    ISPK_REQUIRE(D % 4 == 0 && ld_table % 4 == 0 && ld_table >= D && ispk_aligned(d_table, 16) && ispk_aligned(d_x, 16) &&
                     ispk_aligned(workspace, 16),
                 ISPK_E_ALIGN, "speaker_grad: D / ld_table must be multiples of 4 and d_x / d_table / workspace 16-byte aligned");
    const int chunks = (L + kSgRows - 1) / kSgRows;
    ISPK_REQUIRE(workspace_floats >= (int64_t)B * chunks * D, ISPK_E_SHAPE, "speaker_grad: workspace needs %lld floats (B * ceil(L / %d) * D)",
                 (long long)B * chunks * D, kSgRows);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (B > 0)
        hipLaunchKernelGGL(speaker_grad_stage1_kernel, dim3((D / 4 + 63) / 64, chunks, B), dim3(256), 0, s, d_x, text_len, workspace,
                           L, D, chunks);
    hipLaunchKernelGGL(speaker_grad_stage2_kernel, dim3(speakers, (D / 4 + 63) / 64), dim3(256), 0, s, workspace, speaker, id_stride, text_len, d_table,
                       ld_table, speakers, B, L, D, chunks, accumulate);
    return ispk_launch_status();
}

extern "C" int32_t ispk_time_embedding_f32(const float* t, int32_t n, const float* inv_freq, const float* freq_scale,
                                           int32_t half_dim, const float* w0, const float* b0, const float* w1,
                                           const float* b1, int32_t emb_dim, float* out, ispk_stream_t stream) {
    ISPK_REQUIRE(t && inv_freq && freq_scale && w0 && b0 && w1 && b1 && out, ISPK_E_NULL, "time_embedding: null pointer");
    ISPK_REQUIRE(n >= 0 && half_dim >= 1 && half_dim <= 64 && emb_dim >= 1 && emb_dim <= 64, ISPK_E_SHAPE,
                 "time_embedding: bad shape n=%d half_dim=%d emb_dim=%d (both <= 64)", n, half_dim, emb_dim);
    if (n == 0) return 0;
    hipLaunchKernelGGL(time_embedding_kernel, dim3(n), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), t, inv_freq,
                       freq_scale, half_dim, w0, b0, w1, b1, emb_dim, out);
    return ispk_launch_status();
}

static int32_t length_regulate_launch(const float* alignment, const float* dur_f32, const int64_t* dur_i64, const int64_t* enc_len,
                                      const float* x, int64_t ldx, float* out, int64_t* dec_len, uint8_t* dec_mask, int32_t B,
                                      int32_t M, int32_t L, int32_t D, int32_t max_len, int32_t dur_cols, ispk_stream_t stream,
                                      int split, const LrQkv* qkv = nullptr) {
    ISPK_REQUIRE(x && out && dec_len, ISPK_E_NULL, "length_regulate: null pointer");
    ISPK_REQUIRE((dur_f32 != nullptr) != (dur_i64 != nullptr), ISPK_E_NULL,
                 "length_regulate: exactly one of dur_f32 / dur_i64 must be given");
    ISPK_REQUIRE(alignment || dur_f32, ISPK_E_NULL, "length_regulate: the soft path (alignment NULL) needs fp32 durations");
    ISPK_REQUIRE(dur_cols == L || (dur_i64 && dur_cols >= 1), ISPK_E_SHAPE,
                 "length_regulate: dur_cols=%d (L, or any width >= 1 for int64 durations that are only summed)", dur_cols);
    ISPK_REQUIRE(B >= 0 && M >= 1 && L >= 1 && L <= 4096 && B <= 65535, ISPK_E_SHAPE,
                 "length_regulate: bad shape B=%d M=%d L=%d", B, M, L);
    ISPK_REQUIRE(D == 256 || D == 384, ISPK_E_UNSUPPORTED, "length_regulate: dim %d (built for 256 / 384)", D);
    ISPK_REQUIRE(ldx % 4 == 0 && ldx >= D && ispk_aligned(x, 16) && ispk_aligned(out, 16), ISPK_E_ALIGN,
                 "length_regulate: x / out must be 16-byte aligned, ldx a multiple of 4");
    if (B == 0) return 0;
    const size_t lds = 16 + (size_t)(kLrRows * kLrAld + kLrChunk * D + L + 1) * sizeof(float);
    const dim3 grid((M + kLrRows - 1) / kLrRows, B);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define ISPK_LR(NT_, SP_)                                                                                              \
    do {                                                                                                               \
        ISPK_RESERVE_LDS((&length_regulate_kernel<NT_, SP_>), lds, "length_regulate");                                 \
        hipLaunchKernelGGL((length_regulate_kernel<NT_, SP_>), grid, dim3(256), lds, s, alignment, dur_f32, dur_i64, enc_len, x, \
                           ldx, out, dec_len, dec_mask, M, L, max_len, dur_cols);                                      \
    } while (0)
    if (qkv) {
        ISPK_REQUIRE(qkv->gamma && qkv->beta && qkv->w && qkv->qkv, ISPK_E_NULL, "length_regulate_qkv: null pointer");
        ISPK_REQUIRE(D == 384 && split == 1, ISPK_E_UNSUPPORTED, "length_regulate_qkv: dim %d (built for 384, bf16 terms)", D);
        ISPK_REQUIRE(qkv->ld >= kLrQkvN && qkv->ld % 8 == 0 && ispk_aligned(qkv->qkv, 16) && ispk_aligned(qkv->w, 16), ISPK_E_ALIGN,
                     "length_regulate_qkv: ld_qkv must be a multiple of 8 and >= 512, qkv / Wqkv_chunks 16-byte aligned");
        const size_t lds_q = lds > kLrQkvLds ? lds : kLrQkvLds;
        ISPK_RESERVE_LDS((&length_regulate_qkv_kernel), lds_q, "length_regulate_qkv");
        hipLaunchKernelGGL(length_regulate_qkv_kernel, grid, dim3(256), lds_q, s, alignment, dur_f32, dur_i64, enc_len, x, ldx, out,
                           dec_len, dec_mask, M, L, max_len, dur_cols, *qkv);
        return ispk_launch_status();
    }
    if (D == 384) { if (split == 2) ISPK_LR(3, 2); else if (split) ISPK_LR(3, 1); else ISPK_LR(3, 0); }
    else { if (split == 2) ISPK_LR(2, 2); else if (split) ISPK_LR(2, 1); else ISPK_LR(2, 0); }
#undef ISPK_LR
    return ispk_launch_status();
}

extern "C" int32_t ispk_length_regulate_f32(const float* alignment, const float* dur_f32, const int64_t* dur_i64,
                                            const int64_t* enc_len, const float* x, int64_t ldx, float* out,
                                            int64_t* dec_len, uint8_t* dec_mask, int32_t B, int32_t M, int32_t L, int32_t D,
                                            int32_t max_len, int32_t dur_cols, ispk_stream_t stream) {
    return length_regulate_launch(alignment, dur_f32, dur_i64, enc_len, x, ldx, out, dec_len, dec_mask, B, M, L, D, max_len, dur_cols,
                                  stream, 0);
}

extern "C" int32_t ispk_length_regulate_split_bf16(const float* alignment, const float* dur_f32, const int64_t* dur_i64,
                                                   const int64_t* enc_len, const float* x, int64_t ldx, float* out,
                                                   int64_t* dec_len, uint8_t* dec_mask, int32_t B, int32_t M, int32_t L,
                                                   int32_t D, int32_t max_len, int32_t dur_cols, ispk_stream_t stream) {
    return length_regulate_launch(alignment, dur_f32, dur_i64, enc_len, x, ldx, out, dec_len, dec_mask, B, M, L, D, max_len, dur_cols,
                                  stream, 1);
}

extern "C" int32_t ispk_length_regulate_qkv_bf16(const float* alignment, const float* dur_f32, const int64_t* dur_i64,
                                                 const int64_t* enc_len, const float* x, int64_t ldx, float* out,
                                                 int64_t* dec_len, uint8_t* dec_mask, const float* norm_gamma,
                                                 const float* norm_beta, float norm_eps, const uint16_t* Wqkv_chunks, uint16_t* qkv,
                                                 int64_t ld_qkv, int32_t B, int32_t M, int32_t L, int32_t D, int32_t max_len,
                                                 int32_t dur_cols, ispk_stream_t stream) {
    const LrQkv q{norm_gamma, norm_beta, norm_eps, Wqkv_chunks, qkv, ld_qkv};
    return length_regulate_launch(alignment, dur_f32, dur_i64, enc_len, x, ldx, out, dec_len, dec_mask, B, M, L, D, max_len, dur_cols,
                                  stream, 1, &q);
}

extern "C" int32_t ispk_length_regulate_split_f16(const float* alignment, const float* dur_f32, const int64_t* dur_i64,
                                                  const int64_t* enc_len, const float* x, int64_t ldx, float* out,
                                                  int64_t* dec_len, uint8_t* dec_mask, int32_t B, int32_t M, int32_t L,
                                                  int32_t D, int32_t max_len, int32_t dur_cols, ispk_stream_t stream) {
    return length_regulate_launch(alignment, dur_f32, dur_i64, enc_len, x, ldx, out, dec_len, dec_mask, B, M, L, D, max_len, dur_cols,
                                  stream, 2);
}
