/* ispk.h — C ABI of libispk.so: the MI355X (gfx950) kernels behind the isp-tts acoustic-model forward path.
 *
 * The reference (ilya16/isp-tts) has no FFI layer: its operator surface is Python nn.Modules plus one
 * numba-compiled function.  This header is the boundary a drop-in binds instead (ctypes stub: INTEGRATION.md);
 * every entry point names the reference interface it replaces (paths relative to the reference's `tts/`).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch/HIP types except the opaque stream handle.
 *   - All pointers are DEVICE pointers (caller-allocated, e.g. tensor.data_ptr()); row-major; strides in ELEMENTS.
 *   - No allocation, no ownership transfer, no host synchronisation: launches are asynchronous on `stream`
 *     (NULL = the legacy default stream) and are graph-capturable.
 *   - Return value: 0 ok; < 0 argument error (ISPK_E_*), message via ispk_last_error_string() (thread-local);
 *     > 0 a hipError_t from the launch.
 *   - Thread-safe and re-entrant: no mutable global state.
 *   - `lengths` are int64 on device, as the reference's collator produces them (data/collator.py:36,45).
 *   - `row_mask` is a byte per row (torch.bool storage): nonzero = valid.
 */
#ifndef ISPK_H
#define ISPK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* ispk_stream_t; /* == hipStream_t */

#define ISPK_ABI_VERSION 2 /* 2: round 3 - entry points removed (fused variants, _amp attention pair) and added (split fp16, util, graph support) */

#define ISPK_E_NULL (-1)        /* required pointer is NULL */
#define ISPK_E_SHAPE (-2)       /* size out of the supported range */
#define ISPK_E_ALIGN (-3)       /* pointer / stride alignment */
#define ISPK_E_UNSUPPORTED (-4) /* combination not implemented */

int32_t ispk_abi_version(void);
const char* ispk_last_error_string(void);
/* Fills name[cap] with the device's gcnArchName; returns CU count (>0) or a negative/hip error. */
int32_t ispk_device_info(char* name, int32_t cap);

/* ---------------------------------------------------------------------------------------------------------------
 * Monotonic Alignment Search.
 * Replaces: modules/aligner/mas.py:29-35 `b_mas` (numba CPU) and modules/aligner/cuda_mas.py:11-46 `cuda_b_mas`
 * (numba CUDA), as dispatched by models/acoustic/modules/alignment.py:291-331.
 *   logits    [B][M_max][L_max] fp32, element strides (stride_b, stride_m, 1); NOT modified
 *   text_len  [B] int64 (reference `in_lens`),  1 <= text_len[b] <= L_max <= 512
 *   mel_len   [B] int64 (reference `out_lens`), 1 <= mel_len[b]  <= M_max <= 4096
 *   attn_hard [B][M_max][L_max] int16, contiguous: one-hot rows, zero outside (mel_len, text_len)  (fully written)
 *   dur       [B][L_max] int64 or NULL: column sums of attn_hard (alignment.py:275 `attn_hard.sum(dim=1)`) with the
 *             reference's fix-up applied (alignment.py:278-282: mel_len[b] - sum goes to column 0; zero for valid lengths)
 *   path      [B][M_max] int16 or NULL: chosen text index per mel row, -1 for rows >= mel_len
 * One wavefront runs the DP of one utterance; ties go to the diagonal predecessor exactly as mas.py:17.
 */
int32_t ispk_mas_f32(const float* logits, const int64_t* text_len, const int64_t* mel_len, int16_t* attn_hard,
                     int64_t* dur, int16_t* path, int32_t B, int32_t M_max, int32_t L_max, int64_t stride_b,
                     int64_t stride_m, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * LayerNorm / AdaptiveLayerNorm (+ row mask).
 * Replaces: modules/transformer/normalization.py:20-27 (LayerNorm) and :37-61 (AdaptiveLayerNorm), plus the
 * `out * mask` of transformer.py:101-102 / :205-206 when row_mask is given.
 *   y[r][:] = mask[r] * ( scale * ((x[r][:] - mean) / sqrt(var + eps)) + shift ),   biased variance
 *   plain   : scale = gamma[D], shift = beta[D]                       (ada_scale == NULL)
 *   adaptive: scale = ada_scale[b][D], shift = ada_shift[b][D], b = r / rows_per_batch, row stride ada_stride
 *             (ada_stride = 0 broadcasts one condition row over the whole batch: the [1,1,C] case of :57)
 * D must be a multiple of 64 and <= 1024.  x_f32 in, y in the named dtype.
 */
int32_t ispk_layernorm_f32(const float* x, int64_t ldx, const float* gamma, const float* beta, const float* ada_scale,
                           const float* ada_shift, int64_t ada_stride, int32_t rows_per_batch,
                           const uint8_t* row_mask, float* y, int64_t ldy, int32_t rows, int32_t D, float eps,
                           ispk_stream_t stream);
int32_t ispk_layernorm_f32_bf16(const float* x, int64_t ldx, const float* gamma, const float* beta,
                                const float* ada_scale, const float* ada_shift, int64_t ada_stride,
                                int32_t rows_per_batch, const uint8_t* row_mask, uint16_t* y, int64_t ldy, int32_t rows,
                                int32_t D, float eps, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Linear layers on MFMA:  C[i][j] = epilogue( sum_k A[i][k] * W[j][k] ),  A [M][K], W [N][K] (nn.Linear layout).
 * Replaces: nn.Linear call sites attention.py:105,111,168 (to_q / to_kv / to_out), feedforward.py:33-36
 * (Linear -> GELU(erf) -> Linear), transformer.py:170 (project_emb), model.py:167-168 (to_mel + transpose + mask),
 * and the residual / mask arithmetic of transformer.py:91,105,110 and attention.py:172 through `flags`.
 *
 *   v = acc (+ bias)                      bias indexed by column j, or by row i with ISPK_EP_BIAS_ROW
 *   v = gelu_erf(v) | silu(v)             ISPK_EP_GELU | ISPK_EP_SILU
 *   v = mask * v                          ISPK_EP_MASK_ACC   (mask BEFORE the residual add: attention.py:172)
 *   v = v + resid[i][j]                   resid != NULL (same indexing as C, leading stride ldr)
 *   v = mask * v                          ISPK_EP_MASK_OUT   (mask AFTER the residual add: transformer.py:110)
 *   mask indexed by row i, or by column j with ISPK_EP_MASK_COL
 *   store: C[i*ldc + j], or with cols_per_batch > 0:  C[(j / cpb) * batch_stride + i*ldc + (j % cpb)]
 *          (to_mel: A = weight [80][384], "W" = activations [B*M][384], cpb = M, ldc = M, batch_stride = 80*M
 *           -> mel[B][80][M] written with consecutive lanes along the mel-frame axis)
 *
 * Requirements: K % 8 == 0; lda, ldw % 4 == 0 (fp32) / % 8 (bf16); A, W 16-byte aligned.  lda may be SMALLER than K:
 * rows then overlap in memory (the sliding-window view that turns a padded channel-last Conv1d into a GEMM, see below).
 * _f32      : fp32 in, v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate), fp32 out.
 * _bf16     : bf16 in, v_mfma_f32_32x32x16_bf16 (fp32 accumulate), epilogue in fp32; C/resid dtype per flags.
 */
#define ISPK_EP_GELU 1u
#define ISPK_EP_SILU 2u
#define ISPK_EP_MASK_ACC 4u
#define ISPK_EP_MASK_OUT 8u
#define ISPK_EP_BIAS_ROW 16u
#define ISPK_EP_MASK_COL 32u
#define ISPK_EP_OUT_BF16 64u   /* _bf16 entry only: C is bf16 (default fp32) */
#define ISPK_EP_RESID_BF16 128u /* _bf16 entry only: resid is bf16 (default fp32) */
#define ISPK_EP_DUAL_GELU 1024u /* ispk_gemm_bf16_gelu_train only: second output = dropout(gelu(C)) */
#define ISPK_EP_GELU_BWD 2048u  /* ispk_gemm_bf16_gelu_bwd only: C = (A W^T) gelu'(u) [dropout] */
#define ISPK_EP_OUT_SPLIT 512u  /* _split_f16 entry only: C is a pair of fp16 planes (hi at C, lo c_plane elements behind) */
#define ISPK_EP_ROWS_T 256u     /* _bf16 entry, K = 256 / 384, fp32 C, no resid: the M rows are [batch][T] frames with
                                   T = cols_per_batch and C is stored transposed per batch,
                                   C[(i / T) * batch_stride + j * ldc + (i % T)]  (bias by column j, mask by row i): the
                                   Linear + transpose(1, 2) of model.py:167-168 with frame-contiguous 128-B stores */

/* Which block tile ispk_gemm_f32 will use for (M, N, K): TM*10 + TN, block = 64*TM x 64*TN (22 -> 128x128).  Lets a
 * profiler label a launch with the kernel instance rocprof will report. */
int32_t ispk_gemm_f32_tile(int32_t M, int32_t N, int32_t K);
int32_t ispk_gemm_f32(const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc, const float* bias,
                      const float* resid, int64_t ldr, const uint8_t* mask, int32_t M, int32_t N, int32_t K,
                      uint32_t flags, int32_t cols_per_batch, int64_t batch_stride, ispk_stream_t stream);
/* C[z] = A[z] . W[z]^T for z < batch (fp32, no epilogue): element strides stride_a / stride_w / stride_c between batch items.
 * The alignment gradient of the length regulator, d A[b] = d out[b] x[b]^T (temporal_adaptor.py:419-421), as ONE launch. */
int32_t ispk_gemm_f32_batched(const float* A, int64_t lda, int64_t stride_a, const float* W, int64_t ldw, int64_t stride_w,
                              float* C, int64_t ldc, int64_t stride_c, int32_t batch, int32_t M, int32_t N, int32_t K,
                              ispk_stream_t stream);
/* The feed-forward block's first Linear of a TRAINING step under autocast (feedforward.py:33-35: Linear -> GELU -> Dropout)
 * with both tensors the backward needs from ONE launch: u = A W^T (bf16, the pre-activation) and a = dropout(gelu(u)) (bf16;
 * the mask of ispk_gelu_bf16 with the same dropout_p / seed: hash(seed, row * N + feature)) - and its mirror in the backward:
 * du = (dY W2) gelu'(u) [keep / (1 - p)] straight from the GEMM's epilogue (row mask: dY's padded rows).  K = 256 / 384,
 * N % 8 == 0, contiguous-row bf16 tensors, 16-byte aligned. */
int32_t ispk_gemm_bf16_gelu_train(const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw, uint16_t* u, int64_t ldu,
                                  uint16_t* a, int64_t ld_a, int32_t M, int32_t N, int32_t K, float dropout_p, uint64_t seed,
                                  ispk_stream_t stream);
int32_t ispk_gemm_bf16_gelu_bwd(const uint16_t* dY, int64_t lddy, const uint16_t* W2t, int64_t ldw, const uint16_t* u,
                                int64_t ldu, uint16_t* du, int64_t lddu, const uint8_t* row_mask, int32_t M, int32_t N,
                                int32_t K, float dropout_p, uint64_t seed, ispk_stream_t stream);
/* Kernel instance dispatched by this thread's last ispk_gemm_bf16 call (profiler labels): 1000+KC panel<KC>,
 * 2000+10*TN+WM wide<TN,WM>, 3000+10*TM+TN generic<TM,TN>. */
int32_t ispk_gemm_bf16_last_variant(void);
int32_t ispk_gemm_bf16(const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw, void* C, int64_t ldc,
                       const float* bias, const void* resid, int64_t ldr, const uint8_t* mask, int32_t M, int32_t N,
                       int32_t K, uint32_t flags, int32_t cols_per_batch, int64_t batch_stride, ispk_stream_t stream);
/* Few rows, long reduction (a rank's share under strong scaling: the text-side stacks at 8 - 16 utterances per GPU): the same
 * product with K cut into `ksplit` slices that run as separate workgroups into fp32 slabs of `workspace` (ksplit * M * N
 * floats), then one pass adds the slabs in slice order and applies ispk_gemm_bf16's epilogue.  ispk_gemm_bf16_splitk_plan
 * returns the ksplit to use for a shape (1: call ispk_gemm_bf16).  Same reference sites as ispk_gemm_bf16
 * (feedforward.py:36 at K = inner, alignment.py:69-83 convolutions as GEMMs). */
int32_t ispk_gemm_bf16_splitk_plan(int32_t M, int32_t N, int32_t K, uint32_t flags);
int32_t ispk_gemm_bf16_splitk(const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw, void* C, int64_t ldc,
                              const float* bias, const void* resid, int64_t ldr, const uint8_t* mask, int32_t M, int32_t N,
                              int32_t K, uint32_t flags, float* workspace, int32_t ksplit, ispk_stream_t stream);

/* The whole feed-forward block in one kernel (bf16 operands, fp32 accumulation):
 *   out[i][:] = [mask[i]] * ( resid[i][:] + gelu_erf( x[i][:]·W1ᵀ + bias1 )·W2ᵀ + bias2 )
 * Replaces: feedforward.py:33-40 (Linear -> GELU -> Linear; W1 [inner][dim], W2 [dim][inner] as nn.Linear stores them)
 * with the residual add and row mask of transformer.py:105-110.  The [rows][inner] hidden activations never reach HBM.
 * x bf16 [rows][dim]; resid / out fp32 [rows][dim]; dim 256 or 384; inner % 32 == 0; flags: ISPK_EP_MASK_OUT (mask after
 * the residual add) or ISPK_EP_MASK_ACC (before).
 * ldw2 == 0: W2 is the packed image written by ispk_ffn_pack_w2_bf16 (every inner chunk of W2 one contiguous block in
 * fragment order: full-line loads and straight 16-byte LDS stores; ~2 % faster than the row-major layout). */
int32_t ispk_ffn_bf16(const uint16_t* x, int64_t ldx, const uint16_t* W1, int64_t ldw1, const float* bias1,
                      const uint16_t* W2, int64_t ldw2, const float* bias2, const float* resid, int64_t ldr,
                      const uint8_t* mask, float* out, int64_t ldo, int32_t rows, int32_t dim, int32_t inner, uint32_t flags,
                      ispk_stream_t stream);

/* The pre-norm feed-forward block of a transformer layer in one kernel, LayerNorm included:
 *   out[i][:] = [mask[i]] * ( x[i][:] + gelu_erf( LN(x[i][:])·W1ᵀ )·W2ᵀ + bias2 ),   LN = (x - mean_i) * rstd_i * gamma + beta
 * Replaces: transformer.py:101-110 (feed_forward_norm -> feed_forward -> residual add -> mask) = normalization.py:20-27 +
 * feedforward.py:33-40: the separate LayerNorm launch, its bf16 copy of the rows and that copy's re-read disappear.
 * x fp32 [rows][dim] is both the LayerNorm input and the residual; a wave owns whole rows and computes their statistics
 * itself (two-pass fp32, fixed summation order).  The reference also multiplies LN(x) by the row mask (:102); with the
 * same mask applied to the output (flags: ISPK_EP_MASK_OUT / ISPK_EP_MASK_ACC) that product cannot reach any kept value
 * and is skipped.  ISPK_EP_MASK_ACC masks the block's product (bias2 included) before x is added, out = x + mask * (...), so a
 * masked row comes out as x; both flags may be set.  W2 packed (ispk_ffn_pack_w2_bf16), no first-Linear bias.
 * row_stats (optional): float [rows][2] = (mean, rstd with stats_eps) of the OUTPUT rows, for ispk_gemm_bf16_lnin to apply
 * the next LayerNorm while it stages them. */
int32_t ispk_ffn_bf16_prenorm(const float* x, int64_t ldx, const float* norm_gamma, const float* norm_beta, float norm_eps,
                              const uint16_t* W1, int64_t ldw1, const uint16_t* W2_packed, const float* bias2,
                              const uint8_t* mask, float* out, int64_t ldo, int32_t rows, int32_t dim, int32_t inner,
                              uint32_t flags, float* row_stats, float stats_eps, ispk_stream_t stream);

/* Second-generation kernel for the same block (dim 384 only; what the module mirror calls by default):
 *   out[i][:] = [mask[i]] * ( x[i][:] + gelu_erf( LN(x[i][:])·W1ᵀ )·W2ᵀ )          transformer.py:101-110 as above
 * 128 rows per workgroup on EIGHT waves, two per SIMD: the two waves that share a SIMD own the same 32 rows and split both
 * products (K-halves of the first, output-feature halves of the second), so one wave's GELU runs beside the other's
 * MFMAs (csrc/ffn2.hip).  GELU by Abramowitz-Stegun 7.1.27 (|gelu error| <= 2.5e-4 |x|, below the bf16 rounding of the
 * value it feeds).  W1 bf16 [inner][384] contiguous; W2_chunks = ispk_ffn_chunk_w2_bf16(W2): [inner/32][384][32], hidden
 * units in natural order; no biases.  flags / mask / row_stats as ispk_ffn_bf16_prenorm. */
int32_t ispk_ffn_chunk_w2_bf16(const uint16_t* W2, int64_t ldw2, int32_t dim, int32_t inner, uint16_t* out,
                               ispk_stream_t stream);
/* The same block for SMALL batches (the 6,400-row text encoder: 50 row blocks leave most of the 256 CUs idle, and every
 * workgroup streams all 2.4 MB of weights): the inner dimension is split over `splits` workgroups per row block
 * (ispk_ffn_bf16_prenorm2_split: parts[s][i][:] = gelu_erf(LN(x[i][:]) W1_s^T) W2_s^T, raw fp32, split s = hidden units
 * [s * inner / splits, (s + 1) * inner / splits)), then ispk_ffn_combine_ln_f32 adds them in split order:
 *   y[i][:] = [mask[i]] * (x[i][:] + sum_s parts[s][i][:])                              transformer.py:105-110
 *   (x may be NULL: the residual is then inside parts[0], ispk_attn_out_ffn_split_bf16)
 *   ln_out[i][:] = LN(y[i][:]) [* mask[i] if ln_mask]  (optional: the norm that consumes y - next layer's transformer.py:79
 *   or the final :205-206; fp32 or bf16), two-pass statistics.  parts: [splits] blocks at part_stride floats, rows x 384 each. */
int32_t ispk_ffn_bf16_prenorm2_split(const float* x, int64_t ldx, const float* norm_gamma, const float* norm_beta,
                                     float norm_eps, const uint16_t* W1, const uint16_t* W2_chunks, float* parts,
                                     int64_t part_stride, int32_t splits, int32_t rows, int32_t dim, int32_t inner,
                                     ispk_stream_t stream);
int32_t ispk_ffn_combine_ln_f32(const float* x, int64_t ldx, const float* parts, int64_t part_stride, int32_t splits,
                                const uint8_t* mask, float* y, int64_t ldy, const float* ln_gamma, const float* ln_beta,
                                float ln_eps, int32_t ln_mask, void* ln_out, int64_t ld_ln, int32_t ln_bf16, int32_t rows,
                                int32_t dim, ispk_stream_t stream);
int32_t ispk_ffn_bf16_prenorm2(const float* x, int64_t ldx, const float* norm_gamma, const float* norm_beta, float norm_eps,
                               const uint16_t* W1, const uint16_t* W2_chunks, const uint8_t* mask, float* out, int64_t ldo,
                               int32_t rows, int32_t dim, int32_t inner, uint32_t flags, float* row_stats, float stats_eps,
                               ispk_stream_t stream);
/* Second half of a pre-norm TransformerLayer in ONE kernel: the attention block's output projection and the feed-forward block,
 *   x1[i][:]  = x[i][:] + [mask[i] if ISPK_EP_MASK_ACC] * (attn_out[i][:] Wo^T)            attention.py:172-173, transformer.py:91
 *   out[i][:] = [mask[i] if ISPK_EP_MASK_OUT] * (x1[i][:] + gelu_erf(LN(x1[i][:]) W1^T) W2^T)   transformer.py:97-110
 * Replaces: `to_out` (attention.py:69, :172) + the residual add (transformer.py:91) + feed_forward_norm + FeedForward + the
 * second residual add and mask (transformer.py:97-110) - i.e. ispk_gemm_bf16(to_out, residual) followed by
 * ispk_ffn_bf16_prenorm2 - for decoder-sized batches with heads * 64 = dim = 384.  x1 never reaches memory: the row block's
 * residual rows are loaded INTO the accumulators of the kernel's second product, the projection is twelve more steps of that
 * product on top of them (Wo_chunks = ispk_ffn_chunk_w2_bf16(Wo): [384/32][384][32]; attn_out bf16 [rows][384] rows are the
 * B operands, zeroed for masked rows), the LayerNorm is taken from the accumulators, and the feed-forward block accumulates
 * onto them - one read of x, one of attn_out, one write of out per row (per layer: 50 + 25 + 50 MB at 32,768 rows instead
 * of 125 MB for the projection + 170 MB measured for the feed-forward kernel).  Everything else as ispk_ffn_bf16_prenorm2
 * (W1, W2_chunks, row_stats = (mean, rstd) of the output rows for the next layer's q/kv GEMM). */
int32_t ispk_attn_out_ffn_bf16(const float* x, int64_t ldx, const uint16_t* attn_out, int64_t ld_attn,
                               const uint16_t* Wo_chunks, const float* norm_gamma, const float* norm_beta, float norm_eps,
                               const uint16_t* W1, const uint16_t* W2_chunks, const uint8_t* mask, float* out, int64_t ldo,
                               int32_t rows, int32_t dim, int32_t inner, uint32_t flags, float* row_stats, float stats_eps,
                               ispk_stream_t stream);

/* The same kernel with the NEXT layer's attention_norm and fused [to_q; to_kv] projection as its epilogue:
 *   qkv[i][:] = bf16( LN_next(out[i][:]) ) [Wq; Wkv]^T        transformer.py:79-80, attention.py:63-64 of the next TransformerLayer
 * Replaces, in addition: that layer's ispk_gemm_bf16_lnin launch (its re-read of the fp32 rows and 393 KB of weights per
 * workgroup) - between two decoder layers the residual stream is written once and read once.  The finished rows are normalised
 * from the registers that store them (two-pass statistics, next_eps), kept as a bf16 tile in LDS, and multiplied with the weight
 * streamed as 24 k-step chunks: Wqkv_chunks = ispk_chunk_k16_bf16([Wq; Wkv]): [384/16][512][16].  qkv bf16 [rows][512]
 * (6 heads x 64 query features, then 64 key and 64 value features), ld_qkv elements between rows.  No row_stats. */
/* ispk_attn_out_ffn_bf16 for the LAST layer of a stack: the stack's final LayerNorm (transformer.py:205-206, row-masked if ln_mask)
 * of the finished rows as a second output from the same registers, ln_out bf16 (ln_bf16) or fp32 [rows][dim] at ld_ln - the separate
 * LayerNorm launch and its re-read of the rows disappear; `out` may be NULL when only the normalised rows are consumed (the decoder:
 * its output goes through `norm` into to_mel, model.py:168-171) and the fp32 rows are then not stored at all.  ln_mask needs the mask
 * pointer only: it masks ln_out whatever the mask flags say about x1 and out. */
int32_t ispk_attn_out_ffn_norm_bf16(const float* x, int64_t ldx, const uint16_t* attn_out, int64_t ld_attn,
                                    const uint16_t* Wo_chunks, const float* norm_gamma, const float* norm_beta, float norm_eps,
                                    const uint16_t* W1, const uint16_t* W2_chunks, const uint8_t* mask, float* out, int64_t ldo,
                                    int32_t rows, int32_t dim, int32_t inner, uint32_t flags, const float* final_gamma,
                                    const float* final_beta, float final_eps, int32_t ln_mask, void* ln_out, int64_t ld_ln,
                                    int32_t ln_bf16, ispk_stream_t stream);
/* The SMALL-batch form (text encoder) of the projection prologue: ispk_ffn_bf16_prenorm2_split whose every split first forms
 * x1 = x + [mask if ISPK_EP_MASK_ACC] * (attn_out Wo^T) in its accumulators (each needs LN(x1)); split 0's partial product keeps
 * x1, the others start from zero:  parts[0] = x1 + ffn_0(LN(x1)),  parts[s] = ffn_s(LN(x1)).  ispk_ffn_combine_ln_f32 then runs
 * with x = NULL (y = [mask] * sum_s parts[s]).  Replaces the to_out GEMM launch of an encoder layer (attention.py:172-173,
 * transformer.py:91). */
int32_t ispk_attn_out_ffn_split_bf16(const float* x, int64_t ldx, const uint16_t* attn_out, int64_t ld_attn,
                                     const uint16_t* Wo_chunks, const float* norm_gamma, const float* norm_beta, float norm_eps,
                                     const uint16_t* W1, const uint16_t* W2_chunks, const uint8_t* mask, uint32_t flags,
                                     float* parts, int64_t part_stride, int32_t splits, int32_t rows, int32_t dim, int32_t inner,
                                     ispk_stream_t stream);
int32_t ispk_chunk_k16_bf16(const uint16_t* W, int64_t ldw, int32_t N, int32_t K, uint16_t* out, ispk_stream_t stream);
int32_t ispk_attn_out_ffn_qkv_bf16(const float* x, int64_t ldx, const uint16_t* attn_out, int64_t ld_attn,
                                   const uint16_t* Wo_chunks, const float* norm_gamma, const float* norm_beta, float norm_eps,
                                   const uint16_t* W1, const uint16_t* W2_chunks, const uint8_t* mask, float* out, int64_t ldo,
                                   int32_t rows, int32_t dim, int32_t inner, uint32_t flags, const float* next_gamma,
                                   const float* next_beta, float next_eps, const uint16_t* Wqkv_chunks, uint16_t* qkv,
                                   int64_t ld_qkv, ispk_stream_t stream);

/* Linear whose input is LayerNorm(x), with the row statistics supplied by the kernel that produced x:
 *   C[i][n] = epilogue( sum_k bf16( (x[i][k] - mean_i) * rstd_i * ln_gamma[k] + ln_beta[k] ) * W[n][k] )
 * Replaces: normalization.py:20-27 + the Linear that follows it (transformer.py:79-80, attention.py:63-64: attention_norm
 * -> to_q / to_kv) on the bf16 path - the separate LayerNorm launch, its re-read of the fp32 residual stream and the
 * bf16 copy it writes disappear.  x fp32 [M][K] (the residual stream), row_stats float [M][2] = (mean, rstd) from
 * ispk_ffn_bf16_prenorm / ispk_ffn_bf16_prenorm2, or NULL: the kernel computes the statistics itself (its waves
 * own whole rows; two-pass fp32 with ln_eps, fixed summation order) - then any LayerNorm -> Linear pair qualifies
 * (transformer.py:79-80 of a stack's first layer, :101-105 + feedforward.py:33 on the unfused path).
 * K 256 or 384; flags / bias / resid / mask / C as ispk_gemm_bf16 (row-major outputs). */
int32_t ispk_gemm_bf16_lnin(const float* x, int64_t ldx, const float* row_stats, const float* ln_gamma, const float* ln_beta,
                            float ln_eps, const uint16_t* W, int64_t ldw, void* C, int64_t ldc, const float* bias, const void* resid,
                            int64_t ldr, const uint8_t* mask, int32_t M, int32_t N, int32_t K, uint32_t flags,
                            ispk_stream_t stream);

/* One-time weight staging for ispk_ffn_bf16: W2 [dim][inner] (nn.Linear layout, feedforward.py:27) ->
 * packed [inner/32][dim][32], each chunk's 32 hidden units in MFMA accumulator-fragment order.  packed holds
 * dim*inner bf16 elements; inner % 32 == 0. */
int32_t ispk_ffn_pack_w2_bf16(const uint16_t* W2, int64_t ldw2, int32_t dim, int32_t inner, uint16_t* packed,
                              ispk_stream_t stream);

/* Small / odd-shaped Linear (any K, N): one thread per output, fp32 FMA chain in k order.
 * Replaces the tiny nn.Linear sites: embeddings.py:149-153 (time MLP 65->32->32), normalization.py:43-51 (AdaLN
 * condition projections 32->D), temporal_adaptor.py:43,98 (linear_layer D->3), transformer.py:170 with
 * emb_dim 2 / the 3 flow channels of the 387-wide predictor input.
 *   out[i][j] = act( sum_k a[i][k]*w[j][k] + bias[j] ) + resid[i][j];  act: 0 none, ISPK_EP_GELU, ISPK_EP_SILU */
int32_t ispk_linear_small_f32(const float* a, int64_t lda, const float* w, int64_t ldw, const float* bias,
                              const float* resid, int64_t ldr, float* out, int64_t ldo, int32_t M, int32_t N, int32_t K,
                              uint32_t act, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * ALiBi-biased multi-query attention (one shared K/V head, head_dim 64).
 * Replaces: modules/transformer/attend.py:49-122 (`Attend.efficient_attn`: SDPA with a materialised
 * [B,H,N,N] fp32 bias) together with the bias construction of embeddings.py:51-72 and the key-mask assembly of
 * attention.py:128-152.  Nothing of size N*N touches HBM here.
 *   out[b][i][h*64 + d] = sum_j softmax_j( q[b][i][h]·k[b][j] / 8 - slopes[h] * |i - j| ) * v[b][j][d],
 *   j restricted to j < key_len[b] (masked keys get weight exactly 0, as the reference's min/2 fill does)
 *   q   [B][N][H*64] leading stride ldq;  k, v [B][N][64] leading stride ldkv (k and v may alias one
 *   [B][N][128] `to_kv` buffer: k = kv, v = kv + 64);  out [B][N][H*64] leading stride ldo
 *   slopes [H] fp32 = exp(learned_logslopes) (embeddings.py:81-82);  key_len [B] int64 or NULL (= N)
 *   1 <= H <= 8.  Rows i >= key_len[b] are computed like the reference (finite values; zeroed later by the
 *   caller's row mask, attention.py:172).
 *   Every attention entry (these, the split and both training pairs) clamps key_len[b] to [1, N]: 0 (an empty utterance)
 *   attends to key 0 alone, values above N mean N.  key_len values must fit in int32.
 */
int32_t ispk_alibi_mqa_attn_f32(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv,
                                const float* slopes, const int64_t* key_len, float* out, int64_t ldo, int32_t B,
                                int32_t N, int32_t H, ispk_stream_t stream);
int32_t ispk_alibi_mqa_attn_bf16(const uint16_t* q, int64_t ldq, const uint16_t* k, const uint16_t* v, int64_t ldkv,
                                 const float* slopes, const int64_t* key_len, uint16_t* out, int64_t ldo, int32_t B,
                                 int32_t N, int32_t H, ispk_stream_t stream);
/* Same kernel with the work split chosen by the caller: `q_tiles_per_workgroup` 64-query tiles of one batch item share
 * one K/V fetch (only while the whole key range fits the LDS ring, N <= 512; else 1).  0 = automatic (what
 * ispk_alibi_mqa_attn_bf16 uses: as many as still leave >= 256 workgroups).  Results are identical bit for bit. */
int32_t ispk_alibi_mqa_attn_bf16_tiles(const uint16_t* q, int64_t ldq, const uint16_t* k, const uint16_t* v, int64_t ldkv,
                                       const float* slopes, const int64_t* key_len, uint16_t* out, int64_t ldo, int32_t B,
                                       int32_t N, int32_t H, int32_t q_tiles_per_workgroup, ispk_stream_t stream);

/* One attention block of the bf16 forward at N <= 128 positions per batch item in ONE launch (csrc/attn_block.hip):
 *   qkv = x [Wq; Wkv]^T (bf16)   ->   attention as ispk_alibi_mqa_attn_bf16   ->   out = resid + mask * (attn Wo^T) (fp32)
 * bit for bit what ispk_gemm_bf16 (ISPK_EP_OUT_BF16), ispk_alibi_mqa_attn_bf16 and ispk_gemm_bf16 (ISPK_EP_MASK_ACC, resid)
 * give when called in sequence; the attention output itself is not stored.
 *   x      bf16 [B * N][64 H] at ldx: the layer's normalised rows; or NULL: `qkv` already holds the finished q/kv rows
 *   qkv    bf16 [B * N][64 H + 128] at ld_qkv = [Q | K | V]: written (x given; every row exactly once) or read (x NULL)
 *   Wqkv_chunks = ispk_chunk_k16_bf16([Wq; Wkv]): [4 H][64 H + 128][16] (unused when x is NULL);
 *   Wo_chunks   = ispk_chunk_k16_bf16(Wo): [4 H][64 H][16]
 *   slopes [H], key_len [B] int64 or NULL as for the attention entries;  mask [B * N] uint8 or NULL (= all rows valid)
 *   resid, out fp32 [B * N][64 H] at ldr / ldo.   H = 4 or 6 (dim 256 / 384). */
int32_t ispk_attn_block_short_bf16(const uint16_t* x, int64_t ldx, const uint16_t* Wqkv_chunks, uint16_t* qkv, int64_t ld_qkv,
                                   const float* slopes, const int64_t* key_len, const uint16_t* Wo_chunks, const float* resid,
                                   int64_t ldr, const uint8_t* mask, float* out, int64_t ldo, int32_t B, int32_t N, int32_t H,
                                   ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Aligner front-end (the ConvAttention that produces the MAS input), fp32, channel-last padded layout.
 * Replaces: models/acoustic/modules/alignment.py:69-83 (ConvBlock1D), :159-208 (ConvAttention.forward), :18-37
 * (batch_diagonal_prior) and modules/normalization.py:160-208 (_masked_norm "instance").
 *
 * Layout: activations are [B][T+4][C] — channel-last, two zero rows before and after every utterance.  A Conv1d with
 * kernel 5 / padding 2 over such a buffer is ONE ispk_gemm_f32 call over overlapping rows (lda = C, K = 5*C,
 * M = B*(T+4) - 4, weight [O][5*C] = conv.weight.permute(0,2,1)); output row b*(T+4)+t is frame t.
 *
 * Both kernels read fp32 and write fp32 (out_bf16 == 0), bf16 (1: the bf16 throughput path then runs the conv GEMMs on
 * ispk_gemm_bf16 with fp32 outputs, so statistics and scores stay fp32) or split fp16 planes (2: hi plane at `out`, lo plane
 * B*(T+4)*C elements behind - the operand format of ispk_gemm_split_f16, the parity-grade fast path).
 * ispk_pad_rows_f32        out[b][t+2][c] = t < len[b] ? x[b*sb + t*st + c*sc] : 0, pad rows zero
 *                          (x*mask of alignment.py:75 plus the layout change; strides in elements, so a channel-first
 *                           mel [B][C][T] is read with st = 1, sc = T).
 * ispk_masked_instnorm_f32 y: conv output [B][T+4][C] (row t = frame t); per (b, c) mean / biased variance over frames
 *                          t < len[b]; out[b][t+2][c] = t < len[b] ? (y - mean)/sqrt(var + eps)*weight[c] + bias[c] : 0,
 *                          pad rows zero — i.e. the norm, the affine AND the next block's `x * input_mask`.
 * ispk_aligner_scores_f32  q_enc [B][..][128] (frame rows at q_stride_b per utterance), k_enc likewise (text rows):
 *                          S = q·k / sqrt(128) clamped to fp32 max; attn_logits = log_softmax(S over all L columns)
 *                          + log(prior + 1e-6) with the diagonal prior evaluated analytically (gamma 0.1, rows normalised
 *                          with +1e-5, entries < 1e-4 zeroed, zero outside the lengths); attn_soft = softmax over the
 *                          keys < text_len of attn_logits, zero for keys >= text_len and frames >= mel_len.
 *                          Both outputs [B][M][L] fp32 contiguous.  L <= 320, attention_dim 128.
 * ispk_soft_average_f32    TemporalAverager soft branch for pitch and energy plus log1p(duration)
 *                          (models/acoustic/modules/temporal_adaptor.py:257-269, :446-449):
 *                          feats[b][l] = { log1p(dur[b][l]), mask*sum_m pitch[b][m] A[b][m][l] / (sum_m A + 1e-5), same for
 *                          energy }, feats [B][L][3].  duration may be NULL (column 0 is then written as 0): the pitch /
 *                          energy targets need only attn_soft, so they can be had before MAS has finished.
 */
int32_t ispk_pad_rows_f32(const float* x, int64_t stride_b, int64_t stride_t, int64_t stride_c, const int64_t* len,
                          void* out, int32_t out_bf16, int32_t B, int32_t T, int32_t C, ispk_stream_t stream);
int32_t ispk_masked_instnorm_f32(const float* y, const float* weight, const float* bias, const int64_t* len, void* out,
                                 int32_t out_bf16, int32_t B, int32_t T, int32_t C, float eps, ispk_stream_t stream);
int32_t ispk_aligner_scores_f32(const float* q_enc, int64_t q_stride_b, const float* k_enc, int64_t k_stride_b,
                                const int64_t* text_len, const int64_t* mel_len, float* attn_logits, float* attn_soft,
                                int32_t B, int32_t M, int32_t L, int32_t D, ispk_stream_t stream);
/* The same operator for the bf16 compute path (its q_enc / k_enc carry the convolutions' bf16 rounding): score products as
 * three bf16 MFMAs over hi / lo splits of the fp32 operands (~2^-16 relative), v_exp_f32 / v_log_f32 instead of libm. */
int32_t ispk_aligner_scores_fast_f32(const float* q_enc, int64_t q_stride_b, const float* k_enc, int64_t k_stride_b,
                                const int64_t* text_len, const int64_t* mel_len, float* attn_logits, float* attn_soft,
                                int32_t B, int32_t M, int32_t L, int32_t D, ispk_stream_t stream);
int32_t ispk_soft_average_f32(const float* attn_soft, const float* pitch, const float* energy, const int64_t* duration,
                              const int64_t* text_len, float* feats, int32_t B, int32_t M, int32_t L,
                              ispk_stream_t stream);

/* Flow-matching algebra of the adaptor's predictor, FlowTransformerTemporalModule.forward (temporal_adaptor.py:120-147): [B][L][C]
 * fp32 tensors (C = 3 flow channels), t [B].
 * ispk_flow_mix_f32     x_t = (1 - (1 - sigma) t_b) x0 + t_b x1 ;  flow = x1 - (1 - sigma) x0      (:123-126; each operation
 *                       rounded once, in the reference's order)
 * ispk_flow_finish_f32  pf = pred_raw * mask ;  pred = (x0 + pf) * mask (:145) ;  duration = max(exp(pred[..., 0]) - 1, 0)
 *                       (the adaptor's duration estimate, :221 of this repo's mirror / temporal_adaptor.py:276) ;
 *                       loss_ratio[b] = sum over valid (l, c) of (pf - flow)^2 / max(C * valid_l, 1e-5): masked_mean of the
 *                       MSE (:146, utils/functions.py:44-58) before its final mean over the batch; loss_mean[0] (or NULL)
 *                       = that mean, the flow loss itself.  mask uint8 [B][L]. */
/* infer (temporal_adaptor.py:140-170, :351-384):
 * ispk_flow_euler_f32      one Euler step of FlowTransformerTemporalModule.infer: out = x_t + velocity * dt (:166-168; product and
 *                          sum each rounded once), times the [B][L] row mask when given (the `* mask` after the last step, :170).
 *                          dt is a host value: the warped time grid (:150-156) depends only on (steps, step_factor).
 * ispk_infer_features_f32  FlowTemporalAdaptor.infer between predictor and embedding stack (:351-384), pred [B][L][3]:
 *                          duration[b][l] = max(duration_factor * (exp(pred[..,0]) - 1), 0), replaced by the duration target
 *                          (fp32 or int64, at most one given) wherever that is >= 0 (:355-362); features [B][L][2] =
 *                          { (pitch_target | pred[..,1]) * pitch_factor + pitch_delta, (energy_target | pred[..,2]) *
 *                          energy_factor + energy_delta } (:366-381) - the embedding stack's input. */
/* ispk_flow_head_f32    what ends FlowTransformerTemporalModule.forward behind the stack's last layer, in one call: the stack's
 *                       final LayerNorm with its row mask (transformer.py:205-206) on the raw rows y [B][L][256], linear_layer
 *                       (256 -> 3, temporal_adaptor.py:98, :131) and ispk_flow_finish_f32's algebra (:133-147) - pred, duration
 *                       estimate, per-utterance loss ratios and their mean (loss_mean may be NULL).  workspace: 2 * B *
 *                       ceil(L / 16) floats (per-block partial sums, added in block order: deterministic). */
int32_t ispk_flow_head_f32(const float* y, int64_t ldy, const float* norm_gamma, const float* norm_beta, float norm_eps,
                           const float* W, const float* bias, const float* flow, const float* x0, const uint8_t* mask,
                           float* pred, float* duration, float* loss_ratio, float* loss_mean, float* workspace, int32_t B,
                           int32_t L, int32_t D, int32_t C, ispk_stream_t stream);
int32_t ispk_flow_euler_f32(const float* x_t, const float* velocity, float dt, const uint8_t* mask, float* out, int32_t B,
                            int32_t L, int32_t C, ispk_stream_t stream);
int32_t ispk_infer_features_f32(const float* pred, const float* duration_target_f32, const int64_t* duration_target_i64,
                                const float* pitch_target, const float* energy_target, float duration_factor, float pitch_factor,
                                float pitch_delta, float energy_factor, float energy_delta, float* duration, float* features,
                                int32_t B, int32_t L, ispk_stream_t stream);
/* The same with hard durations (soft_duration off, :355-357): the predicted duration is rounded half to even (torch.round)
 * before the clamp, duration = max(rint(duration_factor * (exp(pred[..,0]) - 1)), 0); targets >= 0 replace it unrounded. */
int32_t ispk_infer_features_round_f32(const float* pred, const float* duration_target_f32, const int64_t* duration_target_i64,
                                      const float* pitch_target, const float* energy_target, float duration_factor,
                                      float pitch_factor, float pitch_delta, float energy_factor, float energy_delta,
                                      float* duration, float* features, int32_t B, int32_t L, ispk_stream_t stream);
/* The same with one control set per utterance, read from the device: controls fp32 [B][5], row b = (duration_factor,
 * pitch_factor, pitch_delta, energy_factor, energy_delta) of utterance b; `round` != 0 selects the hard-duration rounding.  A
 * batch whose rows all equal the scalars gives the bits of the two entry points above.  frames_wanted int64 [B] (or NULL):
 * the decoder length the regulator reports for duration[b][0, L) without a clamp - round == 0: (int64)(s + 0.5f), s the
 * fp32 sum taken sequentially in token order (ispk_length_regulate_f32's soft path); round != 0: the sum over the row of
 * (duration + 0.5f) truncated, 0 below 1 (ispk_hard_regulate_f32's repeats).  One workgroup per utterance. */
int32_t ispk_infer_features_items_f32(const float* pred, const float* duration_target_f32, const int64_t* duration_target_i64,
                                      const float* pitch_target, const float* energy_target, const float* controls,
                                      int32_t round, float* duration, float* features, int64_t* frames_wanted, int32_t B,
                                      int32_t L, ispk_stream_t stream);
/* The same with one control set per TOKEN (word-level prosody): controls fp32 [B][L][5], row (b, l) = (duration_factor,
 * pitch_factor, pitch_delta, energy_factor, energy_delta) of token l of utterance b.  The same per-token expression under the
 * same contraction setting, the same frames_wanted (the sequential fp32 sum, or the integer repeats with round != 0), the same
 * refusals and the same no-op at B = 0.  If every row of an utterance equals that utterance's [5] row, duration, features and
 * frames_wanted have the bits of ispk_infer_features_items_f32. */
int32_t ispk_infer_features_tokens_f32(const float* pred, const float* duration_target_f32, const int64_t* duration_target_i64,
                                       const float* pitch_target, const float* energy_target, const float* controls,
                                       int32_t round, float* duration, float* features, int64_t* frames_wanted, int32_t B,
                                       int32_t L, ispk_stream_t stream);
int32_t ispk_flow_mix_f32(const float* x0, const float* x1, const float* t, float sigma, float* x_t, float* flow, int32_t B,
                          int32_t L, int32_t C, ispk_stream_t stream);
int32_t ispk_flow_finish_f32(const float* pred_raw, const float* flow, const float* x0, const uint8_t* mask, float* pred,
                             float* duration, float* loss_ratio, float* loss_mean, int32_t B, int32_t L, int32_t C,
                             ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The steps between the transformer stacks, one launch each instead of ATen glue / a library bmm.
 *
 * ispk_embed_tokens_f32     models/acoustic/model.py:131-134: emb[b][l][:] = table[text[b][l]][:] (nn.Embedding lookup, row
 *                           0 = padding row) and mask[b][l] = l < text_len[b] (utils/functions.py:61-65; mask / text_len may
 *                           be NULL).  Ids outside [0, vocab) read row 0 (the host-side F.embedding would raise).
 * ispk_add_speaker_f32      models/acoustic/model.py:93-97, :205-207 (`infer` of a multi-speaker model): x[b][l][:] +=
 *                           table[speaker[b * id_stride]][:] in place on the encoder output, EVERY row of the utterance (the
 *                           reference adds before any re-masking); id_stride 1 = one id per utterance (the collator's
 *                           [B, 1] field), 0 = one id for the batch (the notebook's `torch.tensor([speaker])`).  Ids outside
 *                           [0, speakers) are clamped (the host-side F.embedding would raise).
 * ispk_add_speaker_out_f32  the same sum into a second buffer: out[b][l][:] = x[b][l][:] + table[id_b][:], x untouched (x != out),
 *                           same id clamp, bit for bit the in-place result.  The teacher-forced forward (model.py:138-146 with
 *                           `speaker_encoder` read as `speaker_embedding`) adds AFTER the aligner took the encoder output, and
 *                           the aligner's backward keeps that tensor.
 * ispk_speaker_grad_f32     the table's gradient under that broadcast: d_table[s][:] = sum over the utterances b with id_b == s
 *                           (ids clamped as above) of the sum over the rows l < text_len[b] (NULL: every row; values outside
 *                           [0, L] are clamped) of d_x[b][l][:], in an order fixed by the shapes.  The reference's gradient is
 *                           exactly zero on padded rows, so leaving them out is the same sum - and rows at or past text_len[b]
 *                           are never read.  One owner per value, fixed order, no atomics: the same bits every run.  Rows of
 *                           speakers absent from the batch are written as zeros; `accumulate` != 0 adds the sums to d_table's
 *                           content instead (absent rows then keep theirs).  d_x fp32 [B][L][D] contiguous, L <= 512, D a
 *                           multiple of 4; d_table [speakers] rows at stride ld_table; workspace >= B * ceil(L / 16) * D floats.
 * ispk_time_embedding_f32   modules/transformer/embeddings.py:131-157 with `with_steps` (temporal_adaptor.py:87-89):
 *                           f = [t, sin(t * freq_scale * inv_freq), cos(..)] (1 + 2*half_dim values),
 *                           out[n][:] = W1 silu(W0 f + b0) + b1; w0 [emb_dim][1 + 2*half_dim], w1 [emb_dim][emb_dim];
 *                           freq_scale is the module's 1-element buffer (device pointer: no host read).
 * ispk_length_regulate_f32  models/acoustic/modules/temporal_adaptor.py:411-436 (LengthRegulator, soft branch):
 *                           out[b][y][:] = sum_t A[b][y][t] * x[b][t][:], dec_len[b] = (sum_t dur[b][t] + 0.5).long()
 *                           clamped to max_len when max_len >= 0, dec_mask[b][y] = y < dec_len[b] (or NULL).
 *                           A = `alignment` fp32 [B][M][L] (forward: the aligner's attn_soft) or, with alignment NULL, the
 *                           soft path of :468-478 generated on the fly from the fp32 durations (infer, :388-397):
 *                           P[t][y] = clamp(cum[t] - y, 0, 1) - clamp(cum[t-1] - y, 0, 1), cum = cumsum(dur) in index order,
 *                           masked by t < enc_len[b] (NULL: L) and y < dec_len[b].  Exactly one of dur_f32 / dur_i64
 *                           is given: fp32 [B][L], or int64 [B][dur_cols] (the MAS durations, dur_cols = L; they are only
 *                           summed, so any [B][dur_cols] array with the same row sums serves - the teacher-forced forward
 *                           passes mel_len as [B][1], which equals the sum of the MAS durations by construction, and so
 *                           does not wait for MAS).  x fp32 [B][L][D] rows at stride ldx, D 256 / 384;
 *                           exact fp32 products (v_mfma_f32_32x32x2_f32). */
int32_t ispk_embed_tokens_f32(const int64_t* text, const float* table, int64_t ld_table, int32_t vocab,
                              const int64_t* text_len, float* emb, uint8_t* mask, int32_t B, int32_t L, int32_t D,
                              ispk_stream_t stream);
/* ispk_embed_tokens_f32 plus a second gather with the same (clamped) ids: qkv[b][l][:] = qkv_table[text[b][l]][:], bf16 rows of
 * N elements (N % 8 == 0) - the text encoder's first attention_norm + [to_q; to_kv] projection, staged once per weight version
 * over the vocab's rows, since its input is Embedding(text) alone. */
int32_t ispk_embed_tokens_qkv(const int64_t* text, const float* table, int64_t ld_table, int32_t vocab, const int64_t* text_len,
                              float* emb, uint8_t* mask, const uint16_t* qkv_table, int64_t ld_qkv_table, uint16_t* qkv,
                              int32_t B, int32_t L, int32_t D, int32_t N, ispk_stream_t stream);
int32_t ispk_add_speaker_f32(float* x, const float* table, int64_t ld_table, int32_t speakers, const int64_t* speaker,
                             int32_t id_stride, int32_t B, int32_t L, int32_t D, ispk_stream_t stream);
int32_t ispk_add_speaker_out_f32(const float* x, float* out, const float* table, int64_t ld_table, int32_t speakers,
                                 const int64_t* speaker, int32_t id_stride, int32_t B, int32_t L, int32_t D, ispk_stream_t stream);
int32_t ispk_speaker_grad_f32(const float* d_x, const int64_t* speaker, int32_t id_stride, const int64_t* text_len,
                              float* workspace, int64_t workspace_floats, float* d_table, int64_t ld_table, int32_t speakers,
                              int32_t B, int32_t L, int32_t D, int32_t accumulate, ispk_stream_t stream);
int32_t ispk_time_embedding_f32(const float* t, int32_t n, const float* inv_freq, const float* freq_scale, int32_t half_dim,
                                const float* w0, const float* b0, const float* w1, const float* b1, int32_t emb_dim,
                                float* out, ispk_stream_t stream);
int32_t ispk_length_regulate_f32(const float* alignment, const float* dur_f32, const int64_t* dur_i64, const int64_t* enc_len,
                                 const float* x, int64_t ldx, float* out, int64_t* dec_len, uint8_t* dec_mask, int32_t B,
                                 int32_t M, int32_t L, int32_t D, int32_t max_len, int32_t dur_cols, ispk_stream_t stream);
/* The same operator for the bf16 compute path: each fp32 operand value is split into two bf16 terms in registers and a product
 * is three bf16 MFMAs (hi hi + hi lo + lo hi, ~2^-16 relative error) instead of eight exact fp32 ones. */
int32_t ispk_length_regulate_split_bf16(const float* alignment, const float* dur_f32, const int64_t* dur_i64, const int64_t* enc_len,
                                 const float* x, int64_t ldx, float* out, int64_t* dec_len, uint8_t* dec_mask, int32_t B,
                                 int32_t M, int32_t L, int32_t D, int32_t max_len, int32_t dur_cols, ispk_stream_t stream);
/* ispk_length_regulate_split_bf16 with the consuming layer's attention_norm + [to_q; to_kv] projection as its epilogue (dim 384):
 * out, dec_len and dec_mask as without it, bit for bit; qkv bf16 [B * M][512] (ld_qkv elements between rows, every row of every
 * frame tile, rows past dec_len included) = bf16(LayerNorm(out row; norm_gamma, norm_beta, norm_eps), two-pass statistics) times
 * Wqkv_chunks = ispk_chunk_k16_bf16([Wq; Wkv]): [384/16][512][16], fp32 accumulation - what ispk_gemm_bf16_lnin computes from
 * `out` with its own statistics.  An utterance's frame tiles are mapped to one XCD (a speed choice: no result depends on it). */
int32_t ispk_length_regulate_qkv_bf16(const float* alignment, const float* dur_f32, const int64_t* dur_i64, const int64_t* enc_len,
                                      const float* x, int64_t ldx, float* out, int64_t* dec_len, uint8_t* dec_mask,
                                      const float* norm_gamma, const float* norm_beta, float norm_eps, const uint16_t* Wqkv_chunks,
                                      uint16_t* qkv, int64_t ld_qkv, int32_t B, int32_t M, int32_t L, int32_t D, int32_t max_len,
                                      int32_t dur_cols, ispk_stream_t stream);
/* ... and for the split-fp16 parity path: the same three products over fp16 terms (22 significant bits per operand: fp32-grade). */
int32_t ispk_length_regulate_split_f16(const float* alignment, const float* dur_f32, const int64_t* dur_i64, const int64_t* enc_len,
                                const float* x, int64_t ldx, float* out, int64_t* dec_len, uint8_t* dec_mask, int32_t B,
                                int32_t M, int32_t L, int32_t D, int32_t max_len, int32_t dur_cols, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Hard durations: FlowTemporalAdaptor with soft_duration off, the reference's constructor default (csrc/hard_duration.hip).
 * L <= 512 tokens (the aligner's limit), B <= 65535; durations outside the operators' domain (negative, NaN) count as 0.
 *
 * ispk_hard_regulate_f32      LengthRegulator without an alignment (temporal_adaptor.py:422-436): reps[b][l] = (float(dur[b][l])
 *                             + 0.5) truncated, over EVERY token column (the reference applies no enc_len mask here);
 *                             dec_len[b] = sum_l reps, clamped to max_len when max_len >= 0; out[b][y][:] = x[b][l][:] for the
 *                             one l with cum[l] <= y < cum[l + 1], zero for y >= dec_len[b]; dec_mask[b][y] = y < dec_len[b]
 *                             (or NULL).  Exactly one of dur_f32 / dur_i64 [B][L] is given.  x fp32 [B][L][D] rows at stride
 *                             ldx, D 256 / 384; out [B][frames][D].  A row copy: bit-exact, whatever the compute path.
 * ispk_hard_regulate_bwd_f32  d_x[b][l][:] = sum of d_out[b][y][:] over the token's frames below min(dec_len[b], rows), added
 *                             in frame order in fp32 by one owner per value (no atomics: the same bits every run); zero rows
 *                             for tokens without frames.  d_out [B][rows][D], d_x [B][L][D], both contiguous.
 * ispk_hard_average_f32       TemporalAverager without an alignment (:451-465) in ispk_soft_average_f32's layout:
 *                             feats[b][l] = { log1p(dur[b][l]), mask * mean of the NON-ZERO pitch[b][y] over the token's
 *                             frames cum[l] <= y < cum[l + 1] (0 when there is none), same for energy }, feats [B][L][3], mask =
 *                             l < text_len[b], cum the running sum of the int64 durations with segment ends cut at M.  Each
 *                             segment is summed directly (the reference differences two fp32 running sums). */
int32_t ispk_hard_regulate_f32(const float* dur_f32, const int64_t* dur_i64, const float* x, int64_t ldx, float* out,
                               int64_t* dec_len, uint8_t* dec_mask, int32_t B, int32_t frames, int32_t L, int32_t D,
                               int32_t max_len, ispk_stream_t stream);
int32_t ispk_hard_regulate_bwd_f32(const float* dur_f32, const int64_t* dur_i64, const float* d_out, float* d_x, int32_t B,
                                   int32_t rows, int32_t L, int32_t D, int32_t max_len, ispk_stream_t stream);
int32_t ispk_hard_average_f32(const float* pitch, const float* energy, const int64_t* duration, const int64_t* text_len,
                              float* feats, int32_t B, int32_t M, int32_t L, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Training step (BASELINE config 5): fp32 kernels with the recipes' dropout; under AMP the Linear GEMMs and
 * their weight gradients take bf16 operands.  The reference has no backward code of its own (autograd of the modules above);
 * what these replace is cited per entry.
 *
 * ispk_transpose_f32           y[c][r] = x[r][c]: weights for dX = dY . W through the NT GEMM (ispk_gemm_f32 wants W^T rows).
 * ispk_gemm_tn_f32             C[N1][N2] (+)= sum_m mask[m] A[m][N1-slice] B[m][N2-slice]: dW = dY^T . X of every nn.Linear
 *                              (autograd of F.linear).  Rows are split into ranges whose partial products go to `workspace`
 *                              (>= N1*N2 floats; more = more ranges, up to 256) and are added in range order: deterministic.
 *                              row_mask uint8 [M] or NULL; accumulate != 0 adds to C.  N1, N2, lda, ldb multiples of 4,
 *                              A and B 16-byte aligned; ldb < N2 is allowed (overlapping rows: the windows of a padded
 *                              convolution input, for the convolution's weight gradient).
 * ispk_gemm_tn_bf16            the same product, operands rounded to bf16 in flight (autocast's weight gradient), fp32 sums.
 * ispk_alibi_mqa_attn_train_bf16 / ispk_alibi_mqa_attn_bwd_bf16   the attention pair below on bf16 tensors (the step under autocast).
 * ispk_layernorm_bwd_f32       backward of modules/transformer/normalization.py:20-31 followed by `* mask` (transformer.py:102):
 *                              dx (=) or (+=, add_to_dx) rstd (g - mean(g) - xhat mean(g xhat)), g = dy mask gamma;
 *                              dgamma = sum_rows dy mask xhat, dbeta = sum_rows dy mask (either may be NULL; both NULL needs no
 *                              workspace, else ceil(rows / 64) * 2 * dim floats).  dim 256 or 384; statistics are recomputed
 *                              from x (two-pass, as the forward kernel).
 * ispk_gelu_f32                a = gelu(u), exact erf (modules/layers.py:29), as a pass of its own: the training forward keeps
 *                              the pre-activation u for the backward (the inference GEMMs apply GELU in their epilogue).
 * ispk_gelu_bwd_f32            du = da * (Phi(u) + u phi(u)): exact-erf GELU (modules/layers.py:29), n % 4 == 0.
 *                              Dropout (feedforward.py:35, nn.Dropout after the activation; attend.py:118, SDPA dropout_p on the
 *                              attention probabilities): with dropout_p > 0 ispk_gelu_f32 returns gelu(u) keep / (1 - p),
 *                              ispk_gelu_bwd_f32 routes the gradient through the same mask, ispk_alibi_mqa_attn_train_f32 is the
 *                              attention forward with dropped probabilities (it also returns the rows' log-sum-exp, which the
 *                              backward takes as lse_in instead of recomputing it) and ispk_alibi_mqa_attn_bwd_f32 differentiates
 *                              through the same mask.  keep = hash(seed, element index) >= p 2^32, a pure function of the seed
 *                              (element index modulo 2^32: flat index of u; ((b H + h) N + query) N + key for attention), so nothing is
 *                              stored; the draw sequence differs from torch's Philox stream (same Bernoulli(1 - p) law).
 *                              ispk_dropout_mask_u8 writes keep for indices 0 .. n-1 (tests).
 * ispk_alibi_mqa_attn_bwd_f32  backward of ispk_alibi_mqa_attn_f32 (attend.py:49-122, embeddings.py:51-82, attention.py:128-152):
 *                              qkv / dqkv fp32 [B][N][H*64 + 128] = [Q heads | K | V] at row stride ld_qkv, o / d_o fp32
 *                              [B][N][H*64] at ld_o, slopes [H] = exp(learned_logslopes), key_len int64 [B] or NULL.
 *                              dQ per head; dK, dV summed over the H heads that share them; dlogslopes[h] = slope_h *
 *                              sum_ij dS_ij (-|i - j|) (or NULL).  The softmax statistics are recomputed (no state is
 *                              kept from the forward).  workspace >= 2*B*H*N + H*B*ceil(N/32) floats.  Every query row is
 *                              differentiated, rows i >= key_len[b] included: d_o there flows into dQ, dK, dV and d log-slope
 *                              like any other row's (training zeroes it first, as the forward's row mask does).  Both
 *                              backwards (this and _bwd_bf16) take o as given for delta_i = sum_d o_id dO_id.
 * ispk_mel_loss_f32            models/acoustic/loss.py:22-35 (MelLoss, weight folded into grad_out by the caller):
 *                              ratio[b] = sum over (c, t < mel_len[b]) of (out - target)^2 / max(C * len_b, 1e-5)
 *                              (utils/functions.py:44-58), loss[0] = mean_b ratio[b]; grad (or NULL) = d loss / d mel_out *
 *                              grad_out, zero on padded frames.  mel fp32 [B][C][T].
 * ispk_aligner_scores_bwd_f32  backward of ispk_aligner_scores_f32 (alignment.py:187-208) from d attn_soft and / or d attn_logits
 *                              (either may be NULL): the gradient of the UNSCALED q . k products, as dS [B][M][ld_s] and its
 *                              transpose dSt [B][L][ld_t] (padding columns must arrive zeroed) - the operands of the two batched
 *                              products d q_enc = dS k_enc, d k_enc = dS^T q_enc.  The diagonal prior is recomputed.
 * ispk_masked_instnorm_bwd_f32 backward of ispk_masked_instnorm_f32 (modules/normalization.py:160-208): y / d_out / d_y are
 *                              [B][T+4][C] with row t = frame t; d_y is zero past each utterance's length; d_weight / d_bias
 *                              summed over utterances in order.  workspace >= 2 B C floats.
 * ispk_soft_average_bwd_f32    d attn_soft (=) or (+=) from d feats [B][L][3] of ispk_soft_average_f32 (temporal_adaptor.py:446-449;
 *                              column 0, the log1p duration, carries no gradient).  workspace >= 3 B L floats.
 * ispk_flow_loss_bwd_f32       d (flow loss) / d pred_raw of ispk_flow_finish_f32 (temporal_adaptor.py:145-146): go 2 m (raw m - flow) /
 *                              (max(C n_b, 1e-5) B), n_b = valid positions of utterance b.
 * ispk_adaln_bwd_f32           backward of AdaptiveLayerNorm (normalization.py:37-61) as ispk_layernorm_f32 applies it with per-
 *                              utterance scale / shift rows: dx (=) or (+=), dscale[b][:] = sum_rows dy mask xhat, dshift[b][:] =
 *                              sum_rows dy mask (rows of utterance b: rows_per_batch consecutive rows); dim 256 / 384.
 * ispk_time_embedding_bwd_f32  backward of ispk_time_embedding_f32 for its four parameters (the time value gets no gradient):
 *                              dw0 [emb_dim][1 + 2 half_dim], db0, dw1 [emb_dim][emb_dim], db1 from d_out [n][emb_dim].
 * ispk_attn_ctc_loss_f32       models/acoustic/loss.py:39-77 (AttentionCTCLoss, weight folded into grad_out): attn_logits fp32
 *                              [B][M][L] -> a blank class with logit blank_logprob in front, log-softmax over the L + 1 classes,
 *                              nn.CTCLoss(blank 0, zero_infinity, reduction "mean") against the targets 1 .. text_len[b] with
 *                              mel_len[b] frames: loss[0] = mean_b nll_b / max(text_len[b], 1) (inf -> 0); grad (or NULL) =
 *                              d loss / d attn_logits * grad_out (what autograd gives through the pad and the log-softmax).
 *                              workspace >= B*M + B + 2*B*M*S floats, S = 2L + 1 rounded up to a multiple of 64.
 * ispk_attn_bin_loss_f32       models/acoustic/loss.py:90-107 (AttentionBinarizationLoss, weight folded into grad_out):
 *                              loss[0] = -sum over the cells of the hard alignment of log(clamp(attn_soft, eps)) / loss[1],
 *                              loss[1] = the number of such cells; attn_hard = the int16 one-hot MAS output [B][M][L].  grad
 *                              (or NULL; must arrive zeroed) = d loss / d attn_soft * grad_out.  workspace: 2048 floats.
 * ispk_mel_grad_rows_f32       first step of the backward of `to_mel` (Linear + transpose + mask, model.py:167-168):
 *                              g[(b, t)][c] = mask[b][t] * dmel[b][c][t], frames as rows for the two GEMMs that follow
 *                              (d dec = g W through ispk_gemm_f32 on W^T, dW = g^T dec through ispk_gemm_tn_f32).
 * ispk_colsum_f32              out[c] = sum_r [mask[r]] x[r][c] (bias gradients), fixed summation order; workspace >= 256 * cols floats.
 * ispk_smallk_wgrad_f32        out[n][k] = sum_r g[r][n] x[r][k], k < K <= 8: weight gradient of a Linear with a handful of input
 *                              features (the adaptor's 2 -> 256 embedding projection, transformer.py:170); workspace >= 256 N K.
 * ispk_embedding_bwd_f32       backward of nn.Embedding (model.py:131): d_table[v][:] = sum of d_emb rows whose id is v, in row order;
 *                              row padding_idx gets zeros.
 * ispk_grad_sqnorm_f32         out[0] = sum g[i]^2 over a flat gradient arena (what clip_grad_norm_ needs,
 *                              experiments/optimizers.py:236-237); partial = 2048 floats (8 KB, 8-byte aligned) of scratch;
 *                              fp64 accumulation in a fixed order.  n = 0 (g may then be NULL) gives 0.
 * ispk_adamw_f32               one torch.optim.AdamW step (optimizers.py:72-74; amsgrad off) over flat arenas p, g, m, v of n
 *                              floats.  Elements [0, n_decay) are the weight-decay group of optimizers.py:15-20 (tensors
 *                              with >= 2 non-unit dimensions): they get `weight_decay` and, when grad_sqnorm (device, the
 *                              sum of squares of that group's UNSCALED gradients) is given, the clip coefficient
 *                              min(1, max_norm / (grad_scale * sqrt(sqnorm) + 1e-6)) - the reference clips group 0 only.
 *                              Every gradient is first multiplied by grad_scale (1 / world size after a summing
 *                              reduce-scatter).  step >= 1 is the 1-based step count of the bias corrections. */
int32_t ispk_transpose_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int32_t rows, int32_t cols,
                           ispk_stream_t stream);
int32_t ispk_gemm_tn_f32(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int32_t M,
                         int32_t N1, int32_t N2, const uint8_t* row_mask, int32_t accumulate, float* workspace,
                         int64_t workspace_floats, ispk_stream_t stream);
/* The same product with the fp32 operands rounded to bf16 on their way to the MFMAs, fp32 accumulation: the weight gradient of a
 * Linear under autocast (recipes/default.yaml:56; torch's Linear backward multiplies bf16 copies of dY and X). */
int32_t ispk_gemm_tn_bf16(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int32_t M,
                          int32_t N1, int32_t N2, const uint8_t* row_mask, int32_t accumulate, float* workspace,
                          int64_t workspace_floats, ispk_stream_t stream);
/* ... and with operands that ARE bf16 in memory (the activations an AMP step keeps in bf16 as their producers wrote them: half
 * the operand bytes of a kernel that is bound by them).  lda, ldb multiples of 4, A and B 8-byte aligned. */
int32_t ispk_gemm_tn_b16(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, float* C, int64_t ldc, int32_t M,
                         int32_t N1, int32_t N2, const uint8_t* row_mask, int32_t accumulate, float* workspace,
                         int64_t workspace_floats, ispk_stream_t stream);
/* Plan of this thread's last weight-gradient launch (ispk_gemm_tn_f32 / _bf16 / _b16 / _batched_f32; tests and profiler labels):
 * returns the kernel that ran - 1 fp32, 2 bf16 in flight, 3 bf16 operands staged through registers, 4 bf16 operands by LDS-DMA
 * (no row mask, batch 1, N1 and N2 multiples of 8); 0 = none yet - and writes the number of row ranges and the rows per range
 * (a multiple of 32; the last range may be shorter) through the pointers that are not NULL. */
int32_t ispk_gemm_tn_last_plan(int32_t* splits, int32_t* rows_per_split);
/* The same product for `batch` independent pairs (A_b, B_b) at element strides stride_a / stride_b, C_b at stride_c - e.g. the
 * backward of the length regulator (temporal_adaptor.py:419-421: out_b = A_b x_b): d x_b = A_b^T d out_b per utterance.
 * row_mask (or NULL) is [batch][M]; workspace >= batch * N1 * N2 floats. */
int32_t ispk_gemm_tn_batched_f32(const float* A, int64_t lda, int64_t stride_a, const float* B, int64_t ldb, int64_t stride_b,
                                 float* C, int64_t ldc, int64_t stride_c, int32_t batch, int32_t M, int32_t N1, int32_t N2,
                                 const uint8_t* row_mask, int32_t accumulate, float* workspace, int64_t workspace_floats,
                                 ispk_stream_t stream);
int32_t ispk_layernorm_bwd_f32(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* gamma,
                               const uint8_t* row_mask, float* dx, int64_t lddx, int32_t add_to_dx, float* dgamma,
                               float* dbeta, float* workspace, int64_t workspace_floats, int64_t rows, int32_t dim,
                               float eps, ispk_stream_t stream);
/* ispk_layernorm_bwd_f32 that also writes dx as bf16 rows (an AMP step: the next dX GEMM and weight gradient read that copy) */
int32_t ispk_layernorm_bwd_dual_f32(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* gamma,
                                    const uint8_t* row_mask, float* dx, int64_t lddx, int32_t add_to_dx, float* dgamma,
                                    float* dbeta, float* workspace, int64_t workspace_floats, int64_t rows, int32_t dim,
                                    float eps, uint16_t* dx_bf16, int64_t ld_dx_bf16, ispk_stream_t stream);
int32_t ispk_gelu_f32(const float* u, float* a, int64_t n, float dropout_p, uint64_t seed, ispk_stream_t stream);
int32_t ispk_gelu_bwd_f32(const float* da, const float* u, float* du, int64_t n, float dropout_p, uint64_t seed,
                          ispk_stream_t stream);
/* The AMP step's forms (recipes/default.yaml:56: under autocast the feed-forward activation and its gradient are bf16 GEMM
 * operands): a / da / du in bf16 as their consumers take them, the pre-activation u stays fp32; same arithmetic, same mask. */
int32_t ispk_gelu_f32_bf16(const float* u, uint16_t* a, int64_t n, float dropout_p, uint64_t seed, ispk_stream_t stream);
int32_t ispk_gelu_bwd_bf16(const uint16_t* da, const float* u, uint16_t* du, int64_t n, float dropout_p, uint64_t seed,
                           ispk_stream_t stream);
/* ... and with the pre-activation u stored in bf16 too (under autocast the first Linear's output is bf16) */
int32_t ispk_gelu_bf16(const uint16_t* u, uint16_t* a, int64_t n, float dropout_p, uint64_t seed, ispk_stream_t stream);
int32_t ispk_gelu_bwd_b16(const uint16_t* da, const uint16_t* u, uint16_t* du, int64_t n, float dropout_p, uint64_t seed,
                          ispk_stream_t stream);
int32_t ispk_dropout_mask_u8(uint8_t* out, int64_t n, float dropout_p, uint64_t seed, ispk_stream_t stream);
int32_t ispk_alibi_mqa_attn_train_f32(const float* qkv, int64_t ld_qkv, const float* slopes, const int64_t* key_len, float* o,
                                      int64_t ld_o, float* lse, int32_t B, int32_t N, int32_t H, float dropout_p, uint64_t seed,
                                      ispk_stream_t stream);
int32_t ispk_alibi_mqa_attn_bwd_f32(const float* qkv, int64_t ld_qkv, const float* o, const float* d_o, int64_t ld_o,
                                    const float* slopes, const int64_t* key_len, float* dqkv, float* dlogslopes,
                                    float* workspace, int64_t workspace_floats, int32_t B, int32_t N, int32_t H,
                                    const float* lse_in, float dropout_p, uint64_t seed, ispk_stream_t stream);
/* The attention of a step under autocast (recipes/default.yaml:56: SDPA and its backward see bf16 q / k / v / dO and return
 * bf16): qkv / o / d_o / dqkv are bf16 (uint16 bit patterns) in the layouts of the fp32 pair, products on bf16 MFMAs with
 * fp32 accumulation and statistics, K / V (forward, dQ) and the heads' Q / dO tiles (dK / dV) staged once per workgroup in
 * LDS (csrc/attention_train.hip).  lse fp32 [B][H][N] is written by the forward and read by the backward: use them as a pair,
 * with the same dropout_p and seed.  workspace: B H N + 2 H B ceil(N / 64) floats.  H <= 6, ld_qkv and ld_o multiples of 8. */
int32_t ispk_alibi_mqa_attn_train_bf16(const uint16_t* qkv, int64_t ld_qkv, const float* slopes, const int64_t* key_len,
                                       uint16_t* o, int64_t ld_o, float* lse, int32_t B, int32_t N, int32_t H, float dropout_p,
                                       uint64_t seed, ispk_stream_t stream);
int32_t ispk_alibi_mqa_attn_bwd_bf16(const uint16_t* qkv, int64_t ld_qkv, const uint16_t* o, const uint16_t* d_o, int64_t ld_o,
                                     const float* slopes, const int64_t* key_len, const float* lse, uint16_t* dqkv,
                                     float* dlogslopes, float* workspace, int64_t workspace_floats, int32_t B, int32_t N,
                                     int32_t H, float dropout_p, uint64_t seed, ispk_stream_t stream);
int32_t ispk_mel_loss_f32(const float* mel_out, const float* mel_target, const int64_t* mel_len, float* ratio, float* loss,
                          float* grad, float grad_out, int32_t B, int32_t C, int32_t T, ispk_stream_t stream);
/* ispk_acoustic_metrics_f32    models/acoustic/evaluator.py:14-67 (MCD, AlignmentMetric; AcousticModelEvaluator.__call__ makes
 *                              all three in one call): out[0] = mcd_{n_mfcc}, out[1] = alignment_length, out[2] =
 *                              alignment_strength, each what the reference's 0-dim result holds.
 *   mel_out, mel_target        fp32 element (b, c, t) at b*sb + c*sc + t*st, c < C channels, t < T frames: [B][C][T] and
 *                              [B][T][C] are a swap of the two strides (the reference's `_mfcc` picks the layout by size(-1)
 *                              == n_mel_channels; the caller resolves it).  Vector loads when the unit-stride axis is the
 *                              frame or (C % 4 == 0) the channel axis, the other strides are multiples of 4 and both bases
 *                              are 16-byte aligned; element loads otherwise.  Both NULL: out[0] is not computed or written.
 *   dct                        [C][n_mfcc] fp32, the DCT-II basis of torchaudio's create_dct(n_mfcc, C, "ortho").
 *                              out[0] = 10 sqrt(2) / ln 10 * mean_b (sum over ALL t < T of |((x - y)[:, t] . D)[1:n_mfcc]|)
 *                              / mel_len[b]  (padded frames included, coefficient 0 dropped, as evaluator.py:25-38).
 *   attn_soft                  fp32 [B][T][L] at (attn_sb, attn_st, 1), or NULL (out[1], out[2] not computed or written).
 *                              a[b][t] = argmax_l (first index on ties, NaN largest: torch's argmax);
 *                              out[1] = mean_b (sum_{t=1}^{mel_len-1} sqrt(1 + (a[t] - a[t-1])^2)) / sqrt(text_len^2 + mel_len^2)
 *                              out[2] = (sum over all B*T frames of max_l attn_soft) / sum_b mel_len[b].
 *   mel_len, text_len          int64 [B] (text_len may be NULL without attn_soft).  1 <= mel_len[b] <= T is required; the
 *                              lengths are device data, so a violation cannot be refused by the return code: it makes every
 *                              written output NaN.
 *   workspace                  >= 3 * B * ceil(T / 32) floats (per-(item, 32-frame chunk) partial sums).
 * Refused (out untouched): a NULL required pointer, B < 1 or B > 65535, T < 1, L < 1 with attn_soft, and with the mels
 * C < 1, C > 128, n_mfcc < 1 or n_mfcc > C; a short workspace (-3).  Two launches, every sum in a fixed order and no
 * floating-point atomics: repeated calls and graph replays are bit-identical. */
int32_t ispk_acoustic_metrics_f32(const float* mel_out, int64_t out_sb, int64_t out_sc, int64_t out_st, const float* mel_target,
                                  int64_t tgt_sb, int64_t tgt_sc, int64_t tgt_st, const int64_t* mel_len, const int64_t* text_len,
                                  const float* attn_soft, int64_t attn_sb, int64_t attn_st, const float* dct, float* workspace,
                                  int64_t workspace_floats, float* out, int32_t B, int32_t C, int32_t T, int32_t L,
                                  int32_t n_mfcc, ispk_stream_t stream);
/* ispk_dtw_f32                 Dynamic time warping of a given cost matrix (no counterpart in the reference, whose evaluator is
 *                              teacher-forced only): D[0][0] = c[0][0], D[i][j] = c[i][j] + min(D[i-1][j-1], D[i-1][j],
 *                              D[i][j-1]); ties go to the diagonal, then to (i-1, j), then to (i, j-1); the backtrace runs from
 *                              (n_len - 1, m_len - 1) to (0, 0).
 *   cost                       fp32 element (b, i, j) at b*cost_sb + i*cost_sn + j, i < N, j < M.  Only the cells i < n_len[b],
 *                              j < m_len[b] are read.
 *   n_len, m_len               int64 [B].  1 <= n_len <= N and 1 <= m_len <= M are required; the lengths are device data, so a
 *                              violation cannot be refused by the return code: that item gets total = NaN, steps = 0 and a
 *                              path of -1.
 *   total, steps               fp32 [B] D[n_len-1][m_len-1] and int32 [B] the number K of cells on the path.
 *   path                       int16 [B][N + M - 1][2] or NULL: the cells (i, j) from (0, 0) to (n_len-1, m_len-1), -1 past K.
 *   workspace                  16-byte aligned, >= B * 256 * ((M + 255) * R + ceil(M * R / 16)) floats with R = 1, 2, 4, 8 for
 *                              N <= 256, 512, 1024, 2048: a skewed copy of the cost matrix (one row of it is what one wave reads
 *                              in one step) and the 2-bit back-pointers.
 * Refused (nothing written): a NULL required pointer, B < 0 or B > 65535, N or M outside 1 .. 2048, a short or misaligned
 * workspace (-3).  B = 0 is a no-op.  Two launches, one workgroup per item in the second; bit-identical across calls and
 * graph replays.
 *
 * ispk_mcd_dtw_f32             Scores free-running synthesis against a recording: MCD after DTW, and F0 RMSE / voicing error
 *                              along the same path.  c[i][j] = |cep_out[i] - cep_target[j]| over the cepstral coefficients
 *                              1 .. n_mfcc - 1 (cep = mel frame . dct, computed once per frame), then ispk_dtw_f32's recurrence.
 *   mel_out, mel_target        as for ispk_acoustic_metrics_f32 (element (b, c, t) at b*sb + c*sc + t*st), with N frames of
 *                              the output and M frames of the target; dct [C][n_mfcc].
 *   pitch_out, pitch_target    fp32 Hz, 0 = unvoiced, frame i of item b at b*sb + i; both or neither.
 *   per_item                   fp32 [4][B]: [0] mcd_dtw = 10 sqrt(2) / ln 10 * total / K; [1] f0_rmse_cents = the RMS of
 *                              1200 log2(f_i / f_j) over the path's pairs with both frames voiced, NaN when there is none;
 *                              [2] vuv_error = the share of the path's pairs whose voicing differs; [3] length_ratio =
 *                              n_len / m_len.  Rows 1 and 2 are written only with the pitch tracks.  An item whose lengths
 *                              are out of range gets NaN in every written row.
 *   means                      fp32 [4]: the plain batch means of the rows of per_item that were written.
 *   cost_out                   NULL, or fp32 [B][N][M]: the cost matrix as the dynamic programme saw it, cells i < n_len, j < m_len
 *                              only (ispk_dtw_f32 on it gives the path the scores were taken along).
 *   workspace                  16-byte aligned: ispk_dtw_f32's, plus B (N + M) kp floats of cepstra with kp = n_mfcc - 1 rounded
 *                              up to 4, plus 2 B floats.  The costs go straight into the skewed layout.
 * Refused as ispk_dtw_f32, and C < 1, C > 128, n_mfcc < 1 or n_mfcc > C.  Four launches. */
int32_t ispk_dtw_f32(const float* cost, int64_t cost_sb, int64_t cost_sn, const int64_t* n_len, const int64_t* m_len,
                     float* total, int32_t* steps, int16_t* path, float* workspace, int64_t workspace_floats, int32_t B,
                     int32_t N, int32_t M, ispk_stream_t stream);
int32_t ispk_mcd_dtw_f32(const float* mel_out, int64_t out_sb, int64_t out_sc, int64_t out_st, const float* mel_target,
                         int64_t tgt_sb, int64_t tgt_sc, int64_t tgt_st, const float* dct, const int64_t* n_len,
                         const int64_t* m_len, const float* pitch_out, int64_t pitch_out_sb, const float* pitch_target,
                         int64_t pitch_target_sb, float* workspace, int64_t workspace_floats, float* per_item, float* means,
                         float* cost_out, int32_t B, int32_t C, int32_t N, int32_t M, int32_t n_mfcc, ispk_stream_t stream);
/* ispk_audio_features_f32     data/providers.py:35-64 (SpectrogramProvider), :70-111 (MelScaleProvider with
 *                              functions.py:19-20), :178-188 (EnergyProvider), :280-348 (PitchProvider, torch-yin, with
 *                              data/pitch.py:17-100), the pitch pad of data/dataset.py:152 and the collator's zero padding
 *                              (data/collator.py:27-95), for n_fft = win_length = 1024, hop 256, pad 384, center=False, power 1.
 *   audio, ld_audio            fp32 [B][S] at row stride ld_audio >= S; utterance b is audio[b][0, audio_len[b]): nothing at or
 *                              past audio_len[b] is read (the reference pads with zeros).  float4 loads when ld_audio % 4 == 0
 *                              and the base is 16-byte aligned.
 *   audio_len                  int64 [B] on the device.  mel_len[b] = (audio_len + 768 - 1024) / 256 + 1.  A length below 256
 *                              (where torch.stft raises) or above S gives mel_len 0 and all-zero rows: lengths are device data,
 *                              so they cannot be refused by the return code.
 *   tables                     fp32: [0, 4096) W_2048^m = exp(-2 pi i m / 2048) as (re, im), m < 2048, made in float64;
 *                              [4096, 5120) the periodic Hann window; [5120, ...) the non-zero filterbank weights, filter by
 *                              filter, each over its contiguous bin range.
 *   table_floats               the length of `tables`, >= 5120: no weight at or past it is read, whatever fb_index says.
 *   fb_index                   int32 [2 n_mels + 1]: first bin lo[m] of filter m, then offsets off[0..n_mels] of its weights
 *                              in tables[5120 + ...]: mel[m] = log(max(sum_{k < off[m+1] - off[m]} |X_{lo+k}| w[off[m]+k], 1e-5)).
 *                              off[n_mels] <= 1026.  May be NULL without mel.
 *   mel                        fp32 [B][n_mels][M] (contiguous), 1 <= n_mels <= 128, or NULL.
 *   mel_len                    int64 [B], or NULL.
 *   pitch                      fp32 [B][M], or NULL: (hz - pitch_mean) / pitch_std for t < (max(len + 768, 2 tau_max) -
 *                              2 tau_max) / 256 + 1 frames, then 0 (dataset.py:152 pads the normalised pitch with 0).  hz is
 *                              torch-yin's: lags tau_min + 1 .. tau_max - 1 of its cumulative-mean-normalised difference
 *                              function, its first-index search against `threshold`, and reciprocal(lag) * sample_rate.
 *                              1 <= tau_min < tau_max - 1, 512 <= tau_max and 3 tau_max <= 2048 (the autocorrelation by a
 *                              2048-point FFT does not wrap).
 *   energy                     fp32 [B][M], or NULL: log1p(sqrt(sum_k |X_k|^2)).
 *   M                          output frames, >= the frame count of S.  Every output is written in full: zero past mel_len.
 * Refused: NULL audio, audio_len or tables (-1), fb_index with mel (-1); table_floats < 5120, B < 1, B > 65535, S < 0, ld_audio < S, M below the
 * frame count of S, n_mels out of range, tau bounds out of range, pitch_std == 0 (-2).  No workspace: one launch, every sum
 * in a fixed order and no atomics, so repeated calls and graph replays are bit-identical. */
int32_t ispk_audio_features_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables,
                                int64_t table_floats, const int32_t* fb_index, int32_t n_mels, float* mel, int64_t* mel_len, float* pitch, float* energy,
                                int32_t B, int32_t S, int32_t M, int32_t tau_min, int32_t tau_max, float sample_rate,
                                float threshold, float pitch_mean, float pitch_std, ispk_stream_t stream);
/* ispk_resample_f32            data/providers.py:203-212 (AudioProvider): torchaudio.transforms.Resample ("sinc_interp_hann")
 *                              and the mean over channels, as one polyphase kernel.  With o = orig and n = dest the REDUCED
 *                              rates (divided by their gcd), output sample m = q n + p of utterance b is
 *                                sum_{t < T} taps[p][t] * x(q o + first[p] + t - width),  x(i) = mean_c audio[b][c][i] inside
 *                              [0, audio_len[b]) and 0 outside it (the reference's zero padding of width and width + o), for
 *                              m < out_len[b] = ceil(n audio_len[b] / o); 0 for out_len[b] <= m < S_out.
 *   audio, ld_b, ld_c          fp32 [B][C][S] at batch stride ld_b and channel stride ld_c (ignored for C = 1), unit stride on
 *                              S.  Nothing at or past audio_len[b] is read.  float4 loads when the strides are multiples of 4
 *                              and the base is 16-byte aligned.
 *   audio_len                  int64 [B] on the device; a length below 0 or above S counts as 0 (a zero row, out_len 0).
 *   taps, tap_floats, first    fp32 [n][T] and int32 [n]: phase p's compact run of non-zero taps and the index of its first tap
 *                              in the dense 2 width + o (data.Resampler builds both in float64, rounded once).  first[p] is
 *                              device data: it is clamped to [0, 2 width + o - T].  tap_floats = n T <= 12288.
 *   out, ld_out, out_len       fp32 [B][S_out] at row stride ld_out, S_out = ceil(n S / o), written in full; int64 [B] or NULL.
 * Refused: a NULL required pointer (-1); n < 1, n > 1024, o < 1, T < 1, T > 2 width + o, B < 1, B > 65535, C < 1, C > 64,
 * S < 0, S_out != ceil(n S / o), short strides (-2); a tap table above 12288 floats or an output block wider than the
 * 8184 staged samples (-4).  One launch, ascending tap order, no atomics: repeats and graph replays are bit-identical.
 *
 * ispk_feature_stats_f64       data/dataset.py:174-221 (AcousticDataset.compute_stats) with functions.py:27-32 (remove_outliers).
 *                              For utterance b and feature f (0 pitch, 1 energy), v = x[b][0, mel_len[b]): p25 / p75 the
 *                              linear-interpolation quantiles at q (n - 1) of the sorted values, kept where
 *                              p25 - 1.5 IQR < v < p75 + 1.5 IQR (strict) and, for pitch, v > 0; any NaN in v keeps nothing.
 *   pitch, energy              fp32 [B][M] at row strides ld_pitch, ld_energy >= M; M <= 4096.
 *   mel_len                    int64 [B] on the device; a length below 0 or above M counts as 0.
 *   partial                    float64 [B][2][5]: (count, mean, M2, min, max) of the kept values of each (utterance, feature),
 *                              (0, 0, 0, +inf, -inf) when nothing is kept.  Quantiles, bounds and sums are float64.
 *   state                      float64 [2][5], the running pooled (count, mean, M2, min, max) per feature: the partials are
 *                              folded into it in utterance order with Chan's merge.  reset != 0 starts from the empty state
 *                              instead of reading it; B = 0 with reset only writes the empty state.
 * Refused: NULL state, or another NULL pointer with B > 0 (-1); B < 0, B > 65535, M < 0, M > 4096, short row strides (-2).
 * Two launches, fixed-order sums, no atomics, no host read. */
int32_t ispk_resample_f32(const float* audio, int64_t ld_b, int64_t ld_c, const int64_t* audio_len, const float* taps,
                          int64_t tap_floats, const int32_t* first, float* out, int64_t ld_out, int64_t* out_len, int32_t B,
                          int32_t C, int32_t S, int32_t S_out, int32_t orig, int32_t dest, int32_t width, int32_t T,
                          ispk_stream_t stream);
int32_t ispk_feature_stats_f64(const float* pitch, int64_t ld_pitch, const float* energy, int64_t ld_energy,
                               const int64_t* mel_len, double* partial, double* state, int32_t B, int32_t M, int32_t reset,
                               ispk_stream_t stream);
/* Audio conditioning (no counterpart in the reference): silence trimming, ITU-R BS.1770-4 loudness and PCM16, on a padded
 * mono batch fp32 [B][S] at row stride ld_audio >= S with int64 audio_len [B] on the device (a length below 0 or above S
 * counts as 0).  Nothing at or past audio_len[b] is read.  float4 loads when the row stride is a multiple of 4 and the
 * base is 16-byte aligned.  B = 0 is a no-op; B > 65535 and S > 2^24 are refused (-2).
 *
 * ispk_audio_measure_f64     bounds int64 [B][2] = (start, end), loudness float64 [B] (LKFS, -inf when no block passes the
 *                            gates), peak fp32 [B] = max |x| over [start, end), gain fp32 [B].
 *   Trim                     frames t = 0 .. ceil(len / 256) - 1, frame t = x[256 t, 256 t + 1024) cut at len, p_t = (sum of
 *                            squares) / 1024 in float64; active when p_t > thr, thr = trim_threshold * max_t p_t (trim_mode 1)
 *                            or trim_threshold itself (trim_mode 2: the caller's constant reference, already multiplied in).
 *                            No active frame: start = end = 0.  Otherwise, f and l the first and last active frames,
 *                            start = max(0, 256 (f - pad_frames)), end = min(len, 256 (l + pad_frames) + 1024).
 *                            trim_mode 0: start = 0, end = len.
 *   Loudness                 of x[start, end) with zero filter state at start.  table float64 [152]: [0, 7) = b0, b1, b2, a1,
 *                            a2 of the K-weighting shelf and a1, a2 of its high-pass (numerator 1, -2, 1) at sample_rate, [7]
 *                            unused, then nine row-major 4 x 4 matrices A^(32 2^k), k = 0 .. 8, A the state transition of the
 *                            cascade in transposed direct form II (states: shelf s1, s2, high-pass s1, s2), made by the host
 *                            in float64 (data.AudioConditioner).  Blocks of 4 steps of sample_rate / 10 samples, one every
 *                            step, only those wholly inside [start, end); z_j = the block's mean square, l_j = -0.691 +
 *                            10 log10 z_j; gates l_j > -70 and l_j > -0.691 + 10 log10(mean z over the first gate's blocks)
 *                            - 10; L = -0.691 + 10 log10(mean z over the blocks passing both).  Filter, sums and gates are
 *                            float64.
 *   Gain                     gain_mode 0: 1.  Otherwise 10^((target_lufs - L) / 20), capped at peak_limit / peak when
 *                            peak > 0; 1 when L = -inf.
 *   workspace                8-byte aligned, >= 2 (B (NH + 1041 W + NS)) floats with W = max(1, ceil(S / 8192)), NH =
 *                            max(1, ceil(S / 256)), NS = S / step + 1 (runtime.audio_measure_workspace_floats): 256-sample
 *                            square sums, the final state of every 32-sample chunk and 8,192-sample segment, per-segment step
 *                            partials and peaks, step sums.
 * Refused: a NULL pointer (-1); sample_rate % 10 != 0, a table of another size, trim_mode outside 0 .. 2, pad_frames outside
 * 0 .. 65536, a negative threshold, peak_limit <= 0 with gain_mode (-2); a short or misaligned workspace (-3); sample_rate
 * outside 8000 .. 768000 (-4).  Three launches.  An item's results depend on that item alone (not on B): every sum runs in
 * a fixed order, no atomics, no host read - repeated calls and graph replays are bit-identical.
 *
 * ispk_audio_apply_f32       out[b][i] = gain[b] * audio[b][start_b + i] (one fp32 product) for i < n_b = min(end_b - start_b,
 *                            S_out), 0 for n_b <= i < S_out; out_len[b] = n_b (may be NULL).  bounds int64 [B][2] is device
 *                            data: a pair outside 0 <= start <= end <= S counts as (0, 0).  gain may be NULL (1).  out fp32
 *                            [B][S_out] at row stride ld_out; it may not overlap audio (-2).  One launch.
 * ispk_pcm16                 out int16 [B][S] at row stride ld_out: q = clamp(rint(32768 x + d), -32768, 32767) (half to
 *                            even, a NaN gives 0) for i < audio_len[b], 0 past it.  dither 0: d = 0.  Otherwise the TPDF
 *                            d = (h(2 i) - h(2 i + 1)) 2^-32, h(k) = mix32(k ^ lo(r)) ^ hi(r) (csrc/dropout.h) with r =
 *                            splitmix64(splitmix64(seed) + b): a pure function of (seed, b, i), so a captured graph repeats
 *                            its dither on every replay.  One launch. */
int32_t ispk_audio_measure_f64(const float* audio, int64_t ld_audio, const int64_t* audio_len, const double* table,
                               int64_t table_doubles, int64_t* bounds, double* loudness, float* peak, float* gain,
                               float* workspace, int64_t workspace_floats, int32_t B, int32_t S, int32_t sample_rate,
                               int32_t trim_mode, double trim_threshold, int32_t pad_frames, int32_t gain_mode,
                               double target_lufs, double peak_limit, ispk_stream_t stream);
int32_t ispk_audio_apply_f32(const float* audio, int64_t ld_audio, const int64_t* bounds, const float* gain, float* out,
                             int64_t ld_out, int64_t* out_len, int32_t B, int32_t S, int32_t S_out, ispk_stream_t stream);
int32_t ispk_pcm16(const float* audio, int64_t ld_audio, const int64_t* audio_len, int16_t* out, int64_t ld_out, int32_t B,
                   int32_t S, int32_t dither, uint64_t seed, ispk_stream_t stream);
/* Vocos vocoder (mel variant, VocosBackbone + ISTFTHead, padding "same", n_fft 1024, hop 256; isp_tts_amd/vocoder.py): the
 * three kernels besides ispk_gemm_* and ispk_layernorm_*.  Utterance b is frames [0, len_b) of [B][.][T] rows, len_b =
 * mel_len[b] (mel_len NULL: every utterance has all T frames).  A device mel_len outside [0, T] counts as 0: zero rows,
 * audio_len 0, nothing read.  Rows are r = b T + t.  B = 0 is a no-op.  One launch each, every sum in a fixed order, no
 * atomics: repeated calls and graph replays are bit-identical.
 *
 * ispk_vocoder_unfold        the embedding Conv1d(C -> dim, kernel 7, padding 3) as GEMM rows:
 *                            rows[r][j C + c] = mel(b, c, t + j - 3) inside [0, len_b), 0 outside it, at k >= 7 C (K padding)
 *                            and on rows t >= len_b.  mel fp32 (mel_f16 = 0) or fp16 at element (b, c, t) = b sb + c sc + t st
 *                            (any strides: a transposed view works); rows fp32 or bf16 (rows_bf16) at row stride ldr >= K.
 *                            K % 8 == 0, K >= 7 C, 1 <= C <= 128.  row_mask (may be NULL): byte [B T], 1 where t < len_b.
 *                            Nothing at or past len_b is read, so padding may hold NaN.
 * ispk_dwconv7_ln_f32        y[r] = LayerNorm(dwconv7(x)[r]) for t < len_b, 0 for t >= len_b: the depthwise Conv1d(D, 7,
 *                            padding 3, groups D) with taps w [D][7] and bias [D] over rows t - 3 .. t + 3 of the same
 *                            utterance (0 outside [0, len_b)), then LayerNorm over D (biased variance, gamma / beta, eps).
 *                            x fp32 [B T][ldx]; y fp32 or bf16 (y_bf16) [B T][ldy].  D % 64 == 0, 64 <= D <= 1024.
 * ispk_istft_head_f32        audio from the head Linear's rows h [B T][ldh >= 1026] (fp32, bias added): bins k <= 512,
 *                            S_k = min(exp(h[r][k]), 100) (cos + i sin)(h[r][513 + k]) (NaN stays NaN), frame t = irfft_1024(S)
 *                            (imaginary parts of bins 0 and 512 ignored) times the window, overlap-added at stride 256 over
 *                            the utterance's own len_b frames, divided by the overlap-added window^2 of those frames, and
 *                            trimmed by 384 samples at both ends: audio[b][m], m < 256 len_b; 0 for 256 len_b <= m < S.
 *                            audio_len[b] = 256 len_b (may be NULL).  tables: fp32 [4096] W_2048^m (re, im) made in float64
 *                            (data.features.twiddles()), then the 1024-point window; table_floats >= 5120.  S >= 256 T,
 *                            ld_audio >= S.
 * Refused: NULL required pointers (-1); shapes out of range (-2). */
int32_t ispk_vocoder_unfold(const void* mel, int32_t mel_f16, int64_t sb, int64_t sc, int64_t st, const int64_t* mel_len,
                            void* rows, int32_t rows_bf16, int64_t ldr, uint8_t* row_mask, int32_t B, int32_t C, int32_t T,
                            int32_t K, ispk_stream_t stream);
int32_t ispk_dwconv7_ln_f32(const float* x, int64_t ldx, const float* w, const float* bias, const float* gamma,
                            const float* beta, float eps, const int64_t* mel_len, void* y, int32_t y_bf16, int64_t ldy,
                            int32_t B, int32_t T, int32_t D, ispk_stream_t stream);
int32_t ispk_istft_head_f32(const float* h, int64_t ldh, const int64_t* mel_len, const float* tables, int64_t table_floats,
                            float* audio, int64_t ld_audio, int64_t* audio_len, int32_t B, int32_t T, int32_t S,
                            ispk_stream_t stream);
int32_t ispk_aligner_scores_bwd_f32(const float* attn_logits, const float* attn_soft, const float* d_soft, const float* d_logits,
                                    const int64_t* text_len, const int64_t* mel_len, float* dS, int64_t ld_s, float* dSt,
                                    int64_t ld_t, int32_t B, int32_t M, int32_t L, float scale, ispk_stream_t stream);
int32_t ispk_masked_instnorm_bwd_f32(const float* y, const float* d_out, const float* weight, const int64_t* lengths, float* d_y,
                                     float* d_weight, float* d_bias, float* workspace, int64_t workspace_floats, int32_t B,
                                     int32_t T, int32_t C, float eps, ispk_stream_t stream);
int32_t ispk_soft_average_bwd_f32(const float* attn_soft, const float* pitch, const float* energy, const float* d_feats,
                                  const int64_t* text_len, float* workspace, int64_t workspace_floats, float* d_attn,
                                  int32_t accumulate, int32_t B, int32_t M, int32_t L, ispk_stream_t stream);
int32_t ispk_flow_loss_bwd_f32(const float* pred_raw, const float* flow, const uint8_t* mask, float grad_out, float* d_raw, int32_t B,
                               int32_t L, int32_t C, ispk_stream_t stream);
int32_t ispk_adaln_bwd_f32(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* scale, int64_t ld_scale,
                           const uint8_t* row_mask, float* dx, int64_t lddx, int32_t add_to_dx, float* dscale, float* dshift,
                           int64_t ld_out, int32_t B, int32_t rows_per_batch, int32_t dim, float eps, ispk_stream_t stream);
int32_t ispk_time_embedding_bwd_f32(const float* t, int32_t n, const float* inv_freq, const float* freq_scale, int32_t half_dim,
                                    const float* w0, const float* b0, const float* w1, int32_t emb_dim, const float* d_out,
                                    float* dw0, float* db0, float* dw1, float* db1, ispk_stream_t stream);
int32_t ispk_attn_ctc_loss_f32(const float* attn_logits, const int64_t* text_len, const int64_t* mel_len, float blank_logprob,
                               float* workspace, int64_t workspace_floats, float* loss, float* grad, float grad_out, int32_t B,
                               int32_t M, int32_t L, ispk_stream_t stream);
int32_t ispk_attn_bin_loss_f32(const float* attn_soft, const int16_t* attn_hard, float eps, float* workspace, float* loss,
                               float* grad, float grad_out, int32_t B, int32_t M, int32_t L, ispk_stream_t stream);
int32_t ispk_mel_grad_rows_f32(const float* dmel, const uint8_t* mask, float* g, int32_t B, int32_t C, int32_t T,
                               ispk_stream_t stream);
int32_t ispk_colsum_f32(const float* x, int64_t ldx, int64_t rows, int32_t cols, const uint8_t* row_mask, float* workspace,
                        int64_t workspace_floats, float* out, ispk_stream_t stream);
int32_t ispk_smallk_wgrad_f32(const float* g, int64_t ldg, const float* x, int64_t ldx, int64_t rows, int32_t N, int32_t K,
                              float* workspace, int64_t workspace_floats, float* out, ispk_stream_t stream);
int32_t ispk_embedding_bwd_f32(const int64_t* ids, const float* d_emb, int64_t rows, int32_t dim, int32_t vocab,
                               int32_t padding_idx, float* d_table, int64_t ld_table, ispk_stream_t stream);
int32_t ispk_grad_sqnorm_f32(const float* g, int64_t n, float* partial, float* out, ispk_stream_t stream);
int32_t ispk_adamw_f32(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_decay, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int32_t step, const float* grad_sqnorm, float max_norm,
                       float grad_scale, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The fp32-grade fast path ("split fp16"): every fp32 operand value v is carried as two fp16 terms, hi = fp16(v) and
 * lo = fp16(v - hi) (22 significant bits), and a product is three fp16 MFMAs, hi hi + hi lo + lo hi, fp32 accumulation:
 * 5.3x the rate of the exact-fp32 MFMAs at fp32-grade results (mel L-inf vs the reference stays < 1e-4; csrc/split.hip).
 * Replaces, on the parity path, the same reference call sites as ispk_gemm_f32 / ispk_alibi_mqa_attn_f32: every nn.Linear
 * of the stacks (attention.py:105,111,168; feedforward.py:33-36; transformer.py:170; model.py:167-168), the aligner's Conv1d
 * as a GEMM (alignment.py:69-83) and Attend.efficient_attn (attend.py:49-122).
 *
 * "Split planes": a [rows][cols] matrix as two fp16 matrices of the same leading stride, the lo plane `*_plane` ELEMENTS
 * behind the hi plane.  Domain |v| <= 65504 (values beyond are clamped).
 * ispk_split_f16            x fp32 [rows][cols] (stride ldx) -> hi / lo planes (stride ldy); cols % 4 == 0.
 * ispk_gemm_split_f16       C = epilogue(A W^T) as ispk_gemm_f32, A [M][K] and W [N][K] as split planes (lda < K allowed: the
 *                           sliding-window Conv1d view).  Epilogue: bias by column, GELU (A&S 7.1.28 erf, |err| <= 3e-7) /
 *                           SILU, MASK_ACC, fp32 residual, MASK_OUT; C fp32 row-major, or ISPK_EP_OUT_SPLIT: C is a pair of
 *                           planes (c_plane; no residual), or ISPK_EP_ROWS_T (cols_per_batch = T, batch_stride): rows are
 *                           [batch][T] frames and C[b][n][t] is written (Linear + transpose(1, 2) of model.py:167-168; bias
 *                           + MASK_OUT only).  K % 8 == 0, N % 4 == 0.
 * ispk_gemm_split_f16_tile  which tile ispk_gemm_split_f16 uses for (M, N, K): TN * 100 + WM * 10 + RT = 64 TN features x 32 WM RT rows.
 * ispk_layernorm_f32_split  ispk_layernorm_f32 with the result written as split planes (y_hi, lo y_plane behind).
 * ispk_alibi_mqa_attn_split_f16   ispk_alibi_mqa_attn_f32 on split terms: q / k / v fp32 as there (K / V are split once per
 *                           workgroup while staged, Q and the probabilities in registers); out fp32 [B][N][H*64] (o_plane
 *                           == 0) or split planes (uint16 elements, lo o_plane behind) for the out-projection GEMM. */
int32_t ispk_split_f16(const float* x, int64_t ldx, uint16_t* hi, uint16_t* lo, int64_t ldy, int32_t rows, int32_t cols,
                       ispk_stream_t stream);
int32_t ispk_gemm_split_f16_tile(int32_t M, int32_t N, int32_t K);
int32_t ispk_gemm_split_f16(const uint16_t* A, int64_t lda, int64_t a_plane, const uint16_t* W, int64_t ldw, int64_t w_plane,
                            void* C, int64_t ldc, int64_t c_plane, const float* bias, const float* resid, int64_t ldr,
                            const uint8_t* mask, int32_t M, int32_t N, int32_t K, uint32_t flags, int32_t cols_per_batch,
                            int64_t batch_stride, ispk_stream_t stream);
int32_t ispk_layernorm_f32_split(const float* x, int64_t ldx, const float* gamma, const float* beta, const float* ada_scale,
                                 const float* ada_shift, int64_t ada_stride, int32_t rows_per_batch, const uint8_t* row_mask,
                                 uint16_t* y_hi, int64_t ldy, int64_t y_plane, int32_t rows, int32_t D, float eps,
                                 ispk_stream_t stream);
int32_t ispk_alibi_mqa_attn_split_f16(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv,
                                      const float* slopes, const int64_t* key_len, void* out, int64_t ldo, int64_t o_plane,
                                      int32_t B, int32_t N, int32_t H, ispk_stream_t stream);

/* fp32 -> bf16 conversion (round-to-nearest-even) of a [rows][cols] matrix; used to stage weights/activations. */
int32_t ispk_cast_f32_bf16(const float* x, int64_t ldx, uint16_t* y, int64_t ldy, int32_t rows, int32_t cols,
                           ispk_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Data movement of a training step (csrc/util.hip), so that a step issues no PyTorch kernel: what the reference does with
 * autograd's AccumulateGrad, torch.cat / .to(bfloat16) on weights, zero fills and scalar algebra on the losses
 * (tts/experiments/trainer.py:538-579, tts/models/acoustic/loss.py:140-182).
 *
 * ispk_segments_f32     up to any number of contiguous fp32 segments in one call (32 per launch): mode 0 dst = src (a
 *                       concatenation), 1 dst += src (gradient delivery into an optimizer arena), 2 dst = bf16(src).
 * ispk_fill_zero        bytes of zeros (4-byte aligned buffer).
 * ispk_scale_f32        x *= s_dev[0] * s_host (s_dev NULL: s_host only): a loss gradient times the incoming scalar gradient.
 * ispk_sum_scalars_f32  out[0] = sum_i weights[i] * terms[i][0] in index order (n <= 8; weights NULL = ones): the total loss.
 * ispk_exp_pad_f32      dst[i] = exp(src[i]) (i < n), 0 (n <= i < total): ALiBi slopes from learned_logslopes.
 * ispk_sqrt_scale_f32   dst[i] = sqrt(src[i]) * scale: the clipped group's gradient norm from its square.
 * ispk_copy2d_f32       rows x cols with leading strides.
 * ispk_permute021_f32   dst[a][c][b] = src[a][b][c]: Conv1d weights [O][C][k] <-> GEMM weights [O][k][C].
 * ispk_conv_weight_flip_f32   wf[c][(K-1-k) O + o] = w[o][c][k]: the GEMM weight of a convolution's input gradient. */
/* A captured (HIP-graph) training step freezes its launch arguments; two things must still change from replay to replay:
 *   ispk_set_dropout_seed_source   while the PROCESS has a source (a DEVICE address of one uint64), every dropout
 *                                  kernel launched from any of its threads - the GELU / attention forward and backward pairs,
 *                                  the mask export - folds that word into its seed when it RUNS; the host rewrites the word
 *                                  between replays.  NULL switches it off.  Process-wide on purpose: an autograd engine
 *                                  launches the backward kernels from a worker thread, and they must draw the forward's masks.
 *   ispk_adam_args_f32 / ispk_adamw_f32_dev   the AdamW step's scalar factors (bias corrections of step t, lr, decay) as a
 *                                  40-byte record: computed on the host exactly as ispk_adamw_f32 computes them, copied to the
 *                                  device by the caller, read by the kernel when it runs. */
typedef struct { float f[10]; } ispk_adam_args_t;
int32_t ispk_set_dropout_seed_source(const uint64_t* device_word);
int32_t ispk_adam_args_f32(float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, float max_norm,
                           float grad_scale, ispk_adam_args_t* out);
int32_t ispk_adamw_f32_dev(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_decay,
                           const ispk_adam_args_t* args_dev, const float* grad_sqnorm, ispk_stream_t stream);

/* ispk_stage_weights   kernel-ready images of fp32 [rows][cols] parameters, 16 per launch: flags 1 = transposed (dst[c][r]: the
 *                       W^T rows the NT GEMM wants for dX = dY W), 2 = bf16 output, 4 = exp of the values; dst rows ld_dst
 *                       elements apart (so that [to_q; to_kv] lands in one fused image).  What the reference does with
 *                       torch.cat / .t() / autocast's weight casts after every optimizer step. */
typedef struct { const float* src; void* dst; int32_t rows, cols; int64_t ld_dst; int32_t flags; } ispk_stage_t;
int32_t ispk_stage_weights(const ispk_stage_t* segs, int32_t nseg, ispk_stream_t stream);
typedef struct { const float* src; void* dst; int64_t n; int32_t mode; } ispk_segment_t;
int32_t ispk_segments_f32(const ispk_segment_t* segs, int32_t nseg, ispk_stream_t stream);
int32_t ispk_fill_zero(void* p, int64_t bytes, ispk_stream_t stream);
int32_t ispk_scale_f32(float* x, int64_t n, const float* s_dev, float s_host, ispk_stream_t stream);
int32_t ispk_sum_scalars_f32(const float* const* terms, const float* weights, int32_t n, float* out, ispk_stream_t stream);
int32_t ispk_exp_pad_f32(const float* src, float* dst, int32_t n, int32_t total, ispk_stream_t stream);
int32_t ispk_sqrt_scale_f32(const float* src, float* dst, int32_t n, float scale, ispk_stream_t stream);
int32_t ispk_copy2d_f32(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int32_t rows, int32_t cols,
                        ispk_stream_t stream);
int32_t ispk_permute021_f32(const float* src, float* dst, int32_t A, int32_t B, int32_t C, ispk_stream_t stream);
int32_t ispk_conv_weight_flip_f32(const float* w, float* wf, int32_t O, int32_t C, int32_t K, ispk_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * HiFi-GAN generator (csrc/hifigan.hip; isp_tts_amd/hifigan.py).  Activations are fp32 rows [B * T][C] with unit column
 * stride (row b*T + t = sample t of utterance b); weights are images [k][C_out][C_in] (tap-major, C_in contiguous), fp32 for
 * the _f32 entries (exact-fp32 MFMA) and bf16 for the _bf16 entries (activations rounded to bf16 on their way into LDS, fp32
 * accumulation, fp32 rows in and out).  The valid length of utterance b is len[b] * len_mul input rows (len NULL: T; a value
 * outside [0, T] counts as 0): input rows at or past it, and halo rows outside [0, length), read as zeros (a select: NaN in
 * the padding does not propagate), output rows at or past the output length are written as zeros.  C_in and C_out are
 * multiples of 32 up to 512 (anything else: E_UNSUP).  x, w and out 16-byte aligned, ldx and ldo multiples of 4.
 *
 * ispk_hifigan_tile_rows      time positions per workgroup of the two convolution kernels (128): the tests' tile edges.
 * ispk_hifigan_conv_*         v = bias + Conv1d(C_in, C_out, k, dilation, padding (k-1) dilation / 2)(leaky_relu(x, slope))
 *                             [+ resid];  out = scale * v, or with accumulate != 0 out = fma(scale, v, out).  slope 1 = no
 *                             activation.  k odd, 1 .. 11; dilation 1 .. 12.  resid may be out (same rows), not x.
 * ispk_hifigan_upsample_*     out [B * T * stride][C_out] = bias + ConvTranspose1d(C_in, C_out, k, stride,
 *                             padding (k - stride) / 2)(leaky_relu(x, slope)); w[j][o][c] = weight[c][o][j].  Any k >= stride
 *                             with k - stride even (stride <= 64, k <= 128); output length stride * input length.
 * ispk_hifigan_post_f32       audio[b][s] = tanh(bias[0] + sum_j sum_c w[j][c] leaky_relu(x[b*T + s + j - 3][c], slope)), the
 *                             7-tap C -> 1 output convolution in fp32, for s < len[b] * len_mul, 0 from there to S (S >= T,
 *                             ld_audio >= S); audio_len[b] = len[b] * len_mul (may be NULL).  w fp32 [7][C].
 * ispk_hifigan_post_clamp_f32 the same with clamp(v, -1, 1) in place of tanh(v) (BigVGAN's use_tanh_at_final = false): the
 *                             same kernel under a template parameter, ispk_hifigan_post_f32's results are unchanged. */
int32_t ispk_hifigan_tile_rows(void);
int32_t ispk_hifigan_conv_f32(const float* x, int64_t ldx, const float* w, const float* bias, const float* resid, int64_t ldr,
                              float* out, int64_t ldo, const int64_t* len, int32_t len_mul, int32_t B, int32_t T, int32_t C_in,
                              int32_t C_out, int32_t k, int32_t dilation, float slope, float scale, int32_t accumulate,
                              ispk_stream_t stream);
int32_t ispk_hifigan_conv_bf16(const float* x, int64_t ldx, const uint16_t* w, const float* bias, const float* resid,
                               int64_t ldr, float* out, int64_t ldo, const int64_t* len, int32_t len_mul, int32_t B, int32_t T,
                               int32_t C_in, int32_t C_out, int32_t k, int32_t dilation, float slope, float scale,
                               int32_t accumulate, ispk_stream_t stream);
int32_t ispk_hifigan_upsample_f32(const float* x, int64_t ldx, const float* w, const float* bias, float* out, int64_t ldo,
                                  const int64_t* len, int32_t len_mul, int32_t B, int32_t T, int32_t C_in, int32_t C_out,
                                  int32_t k, int32_t stride, float slope, ispk_stream_t stream);
int32_t ispk_hifigan_upsample_bf16(const float* x, int64_t ldx, const uint16_t* w, const float* bias, float* out, int64_t ldo,
                                   const int64_t* len, int32_t len_mul, int32_t B, int32_t T, int32_t C_in, int32_t C_out,
                                   int32_t k, int32_t stride, float slope, ispk_stream_t stream);
int32_t ispk_hifigan_post_f32(const float* x, int64_t ldx, const float* w, const float* bias, const int64_t* len,
                              int32_t len_mul, float* audio, int64_t ld_audio, int64_t* audio_len, int32_t B, int32_t T,
                              int32_t S, int32_t C, float slope, ispk_stream_t stream);
int32_t ispk_hifigan_post_clamp_f32(const float* x, int64_t ldx, const float* w, const float* bias, const int64_t* len,
                                    int32_t len_mul, float* audio, int64_t ld_audio, int64_t* audio_len, int32_t B, int32_t T,
                                    int32_t S, int32_t C, float slope, ispk_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * iSTFTNet generator (csrc/istftnet.hip; isp_tts_amd/istftnet.py): the output layer.  conv_pre, the stages and the blocks are
 * the HiFi-GAN entries above.  Rows, lengths and limits are those of ispk_hifigan_post_f32: x is fp32 rows [B * T][C] with
 * unit column stride, 16-byte aligned, ldx a multiple of 4; the valid length of utterance b is n_b = len[b] * len_mul rows
 * (len NULL: T; a value outside [0, T] counts as 0, and so does n_b = 1, which has no reflection); rows at or past it, and
 * halo rows, read as zeros through a select (NaN in the padding does not propagate); C is a multiple of 32 up to 512.
 *
 * ispk_istftnet_tile_frames   frames per workgroup (128): the tests' tile edge.  A workgroup owns 125 hop blocks of one
 *                             utterance and recomputes the 3 frames it shares with its neighbour.
 * ispk_istftnet_head_f32      with N = n_fft, H = N / 2, F = n_b + 1 frames, p[0] = x[1], p[i] = x[i - 1] (ReflectionPad1d((1, 0))):
 *                               y_f[o]  = bias[o] + sum_j sum_c w[j][o][c] leaky_relu(p[f + j - 3][c], slope)   (p = 0 outside [0, F))
 *                               Z_f[k]  = exp(y_f[k]) exp(i phase_scale sin(y_f[H + 1 + k])),  k = 0 .. H
 *                               audio[b] = torch.istft(Z, N, hop, N, hann_window(N, periodic), center = True): hop n_b samples
 *                             (the imaginary parts of Z[0] and Z[H] do not enter; the envelope sum_f w^2 runs over the F frames
 *                             of the utterance), zeros from hop n_b to S; audio_len[b] = hop n_b (may be NULL).  S >= hop T,
 *                             ld_audio >= S, T >= 2 (else E_SHAPE).  n_fft a multiple of 4 from 8 to 32 with hop = n_fft / 4
 *                             (else E_UNSUPPORTED).  w fp32 [7][N + 2][C], bias fp32 [N + 2].  table: 4 N floats made in
 *                             float64 - cos(2 pi m / N) [N], sin(2 pi m / N) [N], hann[t] / N [N], hann[t]^2 [N].  All
 *                             arithmetic fp32 with accurate expf / sinf / cosf; no atomics: a sample's bits depend neither on
 *                             B, nor on the neighbouring utterances, nor on the tile it fell into. */
int32_t ispk_istftnet_tile_frames(void);
int32_t ispk_istftnet_head_f32(const float* x, int64_t ldx, const float* w, const float* bias, const float* table,
                               int32_t table_floats, const int64_t* len, int32_t len_mul, float* audio, int64_t ld_audio,
                               int64_t* audio_len, int32_t B, int32_t T, int32_t S, int32_t C, int32_t n_fft, int32_t hop,
                               float slope, float phase_scale, ispk_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * BigVGAN generator (csrc/bigvgan.hip; isp_tts_amd/bigvgan.py): the anti-aliased periodic activation.  The convolutions
 * are the HiFi-GAN entries above with slope 1.  Rows, lengths and limits are exactly those of the HiFi-GAN entries: x and out
 * are fp32 rows [B * T][C] with unit column stride, 16-byte aligned, ldx and ldo multiples of 4; the valid length of
 * utterance b is len[b] * len_mul rows (len NULL: T; a value outside [0, T] counts as 0); rows at or past it are never read
 * and are written as zeros; C is a multiple of 32 up to 512 (anything else: E_UNSUP).  A workgroup never spans two
 * utterances and the result of utterance b depends neither on its neighbours nor on B.
 *
 * ispk_snake_aa_tile_rows     rows of one utterance per workgroup (512): the tests' tile edges.
 * ispk_snake_aa_f32           per utterance of n valid rows, channel c, row t < n, with fu = taps[0 .. 12), fd = taps[12 .. 24):
 *                               u[s] = 2 sum_{i = ceil((s+4)/2)}^{floor((s+15)/2)} fu[s + 15 - 2 i] x[clamp(i - 5, 0, n-1)][c]
 *                               a[s] = u[s] + inv_b[c] sin(al[c] u[s])^2                                   s in [0, 2n)
 *                               out[t][c] = sum_{j=0}^{11} fd[j] a[clamp(2 t + j - 5, 0, 2n-1)]
 *                             = replicate-pad 5, 2x transposed-convolution upsampling with fu, snake, replicate-pad (5, 6),
 *                             stride-2 convolution with fd.  al, inv_b fp32 [C] (16-byte aligned) and taps fp32 [24] are
 *                             device memory.  Out of place only: out == x is E_SHAPE (the rows around t are read).  fp32
 *                             throughout, accurate sinf (the argument is not range-limited). */
int32_t ispk_snake_aa_tile_rows(void);
int32_t ispk_snake_aa_f32(const float* x, int64_t ldx, const float* al, const float* inv_b, const float* taps, float* out,
                          int64_t ldo, const int64_t* len, int32_t len_mul, int32_t B, int32_t T, int32_t C,
                          ispk_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Vocoder denoiser (csrc/denoise.hip; isp_tts_amd/denoiser.py): STFT, spectral bias subtraction, ISTFT in one launch, on a
 * padded mono batch fp32 [B][S] at row stride ld_audio >= S with int64 audio_len [B] on the device (NULL: every utterance has
 * S samples; a length below 0 or above S counts as 0).  N = 1024, hop 256, K = 513 bins, w the periodic Hann window.
 *
 * ispk_denoise_tile_samples   output samples of one utterance per workgroup (4096): the tests' tile edges.
 * ispk_denoise_f32            per utterance x[0, n), n = audio_len[b] >= 513:
 *                               xp[p] = x[r(p - 512)], p < n + 1024, r(i) = -i (i < 0), 2 (n - 1) - i (i >= n), else i
 *                               X_f[k] = sum_j xp[256 f + j] w[j] exp(-2 pi i j k / 1024)    f < F = 1 + n / 256, k <= 512
 *                               Y_f[k] = X_f[k] max(1 - t_k / |X_f[k]|, 0), 0 where |X_f[k]| = 0;  t_k = strength bias[k]
 *                               y_f    = irfft_1024(Y_f) (1 / 1024; imaginary parts of bins 0 and 512 dropped)
 *                               out[s] = (sum_f w[j] y_f[j]) / (sum_f w[j]^2), j = s + 512 - 256 f, over the frames f < F
 *                                        with 0 <= j < 1024, both sums in ascending f; 0 for n <= s < S
 *                             = torch.stft(center, reflect), the shrink, torch.istft(center, length = n).  With n < 513 (no
 *                             reflection) out[s] = x[s] for s < n, bit for bit.  bias fp32 [513] >= 0 and tables fp32 [5120] =
 *                             W_2048^m as (re, im), then w, both made in float64 and rounded once, are device memory.
 *                             strength_item (may be NULL): fp32 [B] on the device, replaces `strength` per utterance (a negative
 *                             or NaN device value counts as 0).  Nothing at or past n is read.  An utterance's samples depend on
 *                             that utterance alone, every sum runs in a fixed order, no atomics: a ragged batch, repeated calls
 *                             and graph replays are bit-identical.  Scalar loads and stores: no alignment requirement.
 * Refused: NULL audio, tables, bias or out (E_NULL); B > 65535, S > 2^31 - 8193, ld_audio or ld_out < S, out == audio (the
 * neighbouring tiles read the halo), strength negative or NaN (E_SHAPE).  B = 0 or S = 0 is a no-op. */
int32_t ispk_denoise_tile_samples(void);
int32_t ispk_denoise_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables,
                         const float* bias, const float* strength_item, float strength, float* out, int64_t ld_out, int32_t B,
                         int32_t S, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Document join (csrc/join.hip, isp_tts_amd/longform.py): the sentences of a padded batch put back together, per document
 * and in reading order, with pauses, crossfades and fades - no host read.  All integers, `/` floors:
 *   len_b = audio_len[b] if 0 <= audio_len[b] <= S else 0; (s_b, e_b) = (0, len_b), or with bounds [B][2] = (start, end):
 *   s_b = clamp(start, 0, len_b), e_b = clamp(end, s_b, len_b); n_b = e_b - s_b.  Item b is valid when 0 <= doc[b] < D; the
 *   valid items are ordered by (doc, pos, b), next(b) / prev(b) its neighbours in the same document.
 *   ov_b = min(-pause[b], n_b / 2, n_next(b) / 2) when pause[b] < 0 and next(b) exists, else 0 (pause NULL: all 0);
 *   adv_b = n_b + min(pause[b], S_out) when pause[b] >= 0, else n_b - ov_b; off_b = the sum of adv over the items before b
 *   in its document, wanted_d the sum over all of them, doc_len_d = min(wanted_d, S_out).
 *   tail t_b = ov_b if ov_b > 0 else min(fade, n_b / 2); head h_b = ov_prev(b) if that is > 0, else min(fade, n_b / 2);
 *   w_b(i) = head(i) tail(i) in fp32, head(i) = (2 i + 1) / (2 h_b) for i < h_b else 1, tail(i) = (2 (n_b - 1 - i) + 1) /
 *   (2 t_b) for i >= n_b - t_b else 1.
 *   out[d][o] = sum over the items of d with off_b <= o < off_b + n_b, in document order (at most two), of
 *   (g_b w_b(o - off_b)) audio[b][s_b + o - off_b] for o < doc_len_d (g_b = gain[b], 1 for NULL); 0 elsewhere below S_out.
 * ispk_join_plan        one workgroup: ranks the items by counting, writes item_offset int64 [B] (off_b, -1 for a dropped
 *                       item), item_len int64 [B] (n_b, 0 for a dropped item), doc_len and wanted_len int64 [D], and the plan
 *                       (ispk_join_plan_bytes() bytes, 16-byte aligned) that ispk_join_f32 reads.  Integers only, no atomics.
 *                       1 <= B, D <= 1024, 0 <= S, S_out < 2^31, 0 <= fade < 2^23.
 * ispk_join_f32         grid (ceil(S_out / ispk_join_tile_samples()), D): gathers out fp32 [D][S_out] at ld_out from audio
 *                       fp32 [B][S] at ld_audio.  Nothing at or past len_b is read, nothing at or past column S_out written.
 * Both are pure functions of their inputs: a document's bits do not depend on the other documents or on the order of b. */
int32_t ispk_join_tile_samples(void);
int32_t ispk_join_plan_bytes(void);
int32_t ispk_join_plan(const int64_t* audio_len, const int64_t* doc, const int64_t* pos, const int64_t* pause,
                       const int64_t* bounds, void* plan, int64_t plan_bytes, int64_t* item_offset, int64_t* item_len,
                       int64_t* doc_len, int64_t* wanted_len, int32_t B, int32_t S, int32_t D, int32_t S_out, int32_t fade,
                       ispk_stream_t stream);
int32_t ispk_join_f32(const float* audio, int64_t ld_audio, const float* gain, const void* plan, const int64_t* doc_len,
                      float* out, int64_t ld_out, int32_t B, int32_t S, int32_t D, int32_t S_out, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Speech marks (csrc/marks.hip, isp_tts_amd/longform.py): where every token and word of item b lies, in samples of the item's
 * own audio or - with the join group - of its joined document.  One launch, one workgroup per item, integers out, no host read.
 * duration fp32 [B][L] at row stride ld_duration >= L (what the regulator consumed); n = text_len[b] valid tokens (NULL: L; a
 * value outside [0, L] counts as 0); len = audio_len[b] (a value outside [0, S] counts as 0, as in ispk_join_plan); hop =
 * samples per frame.  clamp(v, lo, hi) = lo if v < lo, else hi if v > hi, else v.  The boundary m_t before token t, t in [0, n]:
 *   1. round != 0 (hard durations): r_t = hd_reps<true> of csrc/dec_len.h = (d_t + 0.5f) truncated, 0 below 1 (and for NaN),
 *      cut at 2^30; C_t = r_0 + .. + r_{t-1} in int64; m_t = hop C_t.
 *   2. round == 0 (soft durations): s_0 = 0, s_{t+1} = s_t + d'_t in fp32, sequentially in token order, d'_t = d_t if d_t > 0
 *      else 0 (NaN: 0); v = (double)s_t hop + 0.5; m_t = len where v >= len + 1, else floor(v).  For durations >= 0 the s_t
 *      are soft_dur_sum's sequence bit for bit, so (int64)(s_n + 0.5f) is the frames_wanted of ispk_infer_features_items_f32;
 *      a boundary is where the soft path hands the weight from one token to the next.
 *   3. m_t = clamp(m_t, 0, len).
 *   4. bounds int64 [B][2] (may be NULL: (0, len)): s_b = clamp(start, 0, len), e_b = clamp(end, s_b, len) as in the join;
 *      m_t = clamp(m_t, s_b, e_b) - s_b.
 *   5. the join group item_offset int64 [B], doc int64 [B], doc_len int64 [D] (all given or all NULL): an item with
 *      item_offset[b] < 0 or doc[b] outside [0, D) is dropped and every mark of it is -1; else with d = doc[b] and
 *      dl = max(doc_len[d], 0): m_t = clamp(m_t + item_offset[b], 0, dl)  (item_offset below 2^62).
 *   6. doc_bounds int64 [D][2] (may be NULL, only with the join group): ds = clamp(start_d, 0, dl), de = clamp(end_d, ds, dl);
 *      m_t = clamp(m_t, ds, de) - ds.
 *   token_marks int64 [B][L][2] = (m_t, m_{t+1}) for t < n and (-1, -1) for n <= t < L.
 *   word_marks int64 [B][W][2] (NULL allowed when W == 0): over the tokens t < n whose word_id[b][t] = w lies in [0, W),
 *   (min m_t, max m_{t+1}); (-1, -1) for a word without a token; any other word_id is ignored (word_id int64 [B][L]
 *   contiguous, NULL: no words).
 * Starts are at most ends, consecutive tokens tile ([m_t, m_{t+1}) then [m_{t+1}, m_{t+2})), and without a join an item's first
 * start is 0.  Under a crossfade an item begins before its predecessor ends, so the marks of neighbouring ITEMS overlap there by
 * the overlap of their audio: that is where both are heard, and it is left so.  The fp32 sum of the soft mode is one thread's
 * loop - its order is the contract with the regulator; the hard sums are integers (a block scan).  Plain vector stores, no
 * global atomics; a pure function of its inputs: repeated calls and graph replays give identical bits.
 * Refused: NULL duration, audio_len or token_marks, a partial join group, doc_bounds without the join group, W > 0 (with or
 * without word_id) but no word_marks (E_NULL); L > 4096, W outside [0, 1024], B > 65535, hop outside [1, 2^20], S outside [0, 2^31),
 * ld_duration < L, D outside [1, 1024] with the join group (E_SHAPE).  B = 0 or L = 0 is a no-op. */
int32_t ispk_speech_marks(const float* duration, int64_t ld_duration, const int64_t* text_len, const int64_t* audio_len,
                          const int64_t* bounds, const int64_t* item_offset, const int64_t* doc, const int64_t* doc_len,
                          const int64_t* doc_bounds, const int64_t* word_id, int64_t* token_marks, int64_t* word_marks,
                          int32_t hop, int32_t round, int32_t B, int32_t L, int32_t S, int32_t D, int32_t W,
                          ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Gain envelope (csrc/prosody.hip, isp_tts_amd/longform.py): a linear gain per token on the items' waveforms, with short
 * linear ramps at the token boundaries - the volume part of word-level prosody.  One launch, no atomics, no host read.
 * audio fp32 [B][S] at ld_audio; len = audio_len[b] (a value outside [0, S] counts as 0); token_marks int64 [B][L][2] as
 * ispk_speech_marks writes them in ITEM coordinates (no bounds, no join group); token_gain fp32 [B][L], linear; ramp in samples.
 *   A token with a negative start or end (the marks' -1) is dead.  The others have start and end clamped to [0, len] and are
 *   live when start < end then (a token cut to nothing holds no sample and lends nothing).  The live tokens in index order
 *   tile [0, E), E <= len: each starts where its live predecessor ends, which is how the kernel finds its start.
 *   tok(n) = the live token that holds n; for n >= E the last live token; without a live token e[n] = 1.
 *   At every boundary p between consecutive live tokens j < k: h = min(ramp, (end_j - start_j) / 2, (end_k - start_k) / 2),
 *   `/` floors.  For n in [p - h, p + h), in fp32 without contraction: i = n - p + h, w = (float)(2 i + 1) / (float)(4 h),
 *   e[n] = g_j + (g_k - g_j) w.  Elsewhere e[n] = g_tok(n).  A token lends at most half of itself to each side, so ramps never
 *   overlap, and h = 0 is a step.
 *   out[b][n] = audio[b][n] e[n] for n < len, 0 for len <= n < S  (out fp32 [B][S] at ld_out).
 * Nothing at or past len is read.  Marks that do not tile may give any finite envelope and never cause an access outside the
 * item's rows.  out may be exactly audio (same base, same row stride); otherwise the two must not overlap.  An item's bits
 * depend on that item alone; repeated calls and graph replays repeat theirs.  With all gains equal to g, out has the bits of
 * audio g below len.  Grid (ceil(S / ispk_gain_envelope_tile_samples()), B); 16 bytes per lane when both bases are 16-byte
 * aligned and both strides multiples of four floats.
 * Refused: NULL audio, audio_len, token_marks, token_gain or out (E_NULL); L outside [1, 4096], B > 65535, S outside [0, 2^31),
 * a row stride below S, ramp outside [0, 2^22), out overlapping audio without being audio (E_SHAPE).  B = 0 (or S = 0) is a
 * no-op. */
int32_t ispk_gain_envelope_tile_samples(void);
int32_t ispk_gain_envelope_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const int64_t* token_marks,
                               const float* token_gain, int32_t ramp, float* out, int64_t ld_out, int32_t B, int32_t L,
                               int32_t S, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * True-peak look-ahead limiter (csrc/limiter.hip, isp_tts_amd/data/condition.py): the last fp32 stage in front of ispk_pcm16.
 * One kernel launch behind two 32-bit memsets of true_peak and reduction on the stream; no host read.
 * audio fp32 [B][S] at ld_audio.  len = audio_len[b] (NULL: S; a value outside [0, S] counts as 0).  With bounds int64 [B][2]
 * the kept samples are x[0, n) = audio[b][start, min(end, len)) (a pair that is not 0 <= start <= end <= S keeps nothing),
 * without them audio[b][0, len).  Samples outside count as zero; nothing outside the kept range is read.  g = gain[b] (NULL: 1),
 * c = ceiling > 0 (linear), L = lookahead in samples.  taps fp32 [4][12], made in float64 by the host (data.true_peak_taps):
 *   h[p][k] = sinc(t) cos^2(pi t / 12) for |t| < 6, else 0, with t = k - p / 4, k = -5 .. 6 (column k + 5); phase 0 is the identity.
 *   y[4 i + p] = sum_k h[p][k] fp32(g x[i + k]), fp32 FMAs in the order k = -5 .. 6;  e[i] = max_p |y[4 i + p]|
 *   r[i] = c / e[i] where e[i] > c, else 1; 1 outside [0, n)
 *   m[j] = min over |k| <= L of r[j + k], j in [-L, n + L)   (the minimum itself is extended, not padded with ones: a padded m
 *          lets the gain rise above r within L samples of an item's edges)
 *   s[i] = 1 - sum over |k| <= L of w[k] (1 - m[i + k]), w[k] = cos^2(pi k / (2 (L + 1))) / (L + 1), which sum to 1; the sum
 *          runs in float64.  s is exactly 1 where no r < 1 lies within 2 L samples, and s[i] <= r[i] everywhere.
 *   out[b][i] = clamp(fp32(fp32(g x[i]) s[i]), -c, c) for i < n, 0 for n <= i < S  (out fp32 [B][S] at ld_out); out_len[b] = n
 *   true_peak[b] = max_i e[i], of the gained input, 0 for an empty item;  reduction[b] = fp32(min_i s[i]), 1 when untouched or empty
 * Where s[i] is 1 the output has the bits of ispk_audio_apply_f32 with the same bounds and gain.  out NULL (then out_len NULL
 * too): the launch only measures; with reduction NULL as well it stops behind the envelope.  Both per-item results are folded
 * across an item's tiles with integer atomic max / min on the bit patterns of non-negative floats: the order does not matter,
 * an item's bits depend on that item alone, repeated calls and graph replays repeat theirs.  Grid (ceil(S /
 * ispk_limit_tile_samples()), B); 16-byte loads for an item whose first kept sample is 16-byte aligned (base, row stride and
 * start), 16-byte stores when out's base is and its stride is a multiple of four floats.
 * Refused: B > 65535, S outside [0, 2^24], lookahead outside 1 .. 256, a ceiling that is not positive and finite, a row stride
 * below S, out overlapping audio (E_SHAPE); NULL audio, taps or true_peak, out without reduction, out_len without out (E_NULL);
 * true_peak or reduction off a 4-byte boundary (E_ALIGN).  B = 0 is a no-op. */
int32_t ispk_limit_tile_samples(void);
int32_t ispk_limit_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const int64_t* bounds, const float* gain,
                       const float* taps, float ceiling, int32_t lookahead, float* out, int64_t ld_out, int64_t* out_len,
                       float* true_peak, float* reduction, int32_t B, int32_t S, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Equalizer (csrc/equalizer.hip, isp_tts_amd/data/equalize.py): a cascade of 1 <= N <= 8 biquads in float64, the stage of the
 * audio chain that changes the spectrum.  At most two kernel launches, no atomics, no host read.
 * audio fp32 [B][S], unit stride on S, row stride ld_audio >= S.  len = audio_len[b], int64; a length below 0 or above S
 * counts as 0.  sos float64 [N][5] = (b0, b1, b2, a1, a2) with a0 = 1.  Each section is transposed direct form II in float64:
 *   y  = fma(b0, x, s0)
 *   s0 = fma(-a1, y, fma(b1, x, s1))
 *   s1 = fma(-a2, y, b2 * x)
 * All states are zero at sample 0 of every item; the sections run in order; values between sections stay float64.
 *   out[b][i] = fp32(y_N[i]) for i < len, exactly 0 for len <= i < S  (out fp32 [B][S] at ld_out >= S)
 *   out_len[b] = len (out_len may be NULL): the ringing past the end is cut.  Nothing at or past len is read.
 * table float64 [40 N + 4 N^2], made by the host (data.equalize.equalizer_table):
 *   [0, 8 N)             section k's b0, b1, b2, a1, a2 at 8 k, three unused
 *   [8 N, 40 N)          A_k^(32 2^j), j = 0 .. 7, row-major 2 x 2 at 8 N + 4 (8 k + j); A_k = [[-a1, 1], [-a2, 0]] is the
 *                        section's state transition s' = A_k s + B_k x
 *   [40 N, 40 N + 4 N^2) the joint A^8192, row-major 2 N x 2 N over (s0, s1) of section 0, then of section 1, ...: block
 *                        lower-triangular, read off the update above with x = 0
 * The recurrence runs as a chunked scan on a grid fixed to sample 0: a chunk is 32 samples (one lane), a segment
 * ispk_equalize_segment_samples() = 8192 samples (one workgroup), W = max(1, ceil(S / 8192)).  The first launch (grid (W - 1, B),
 * skipped when W = 1) writes every segment's final joint state from zero entry into workspace (float64 [B][W][2 N]); the second
 * (grid (W, B)) folds the earlier segments' states in segment order with the joint matrix, reruns its segment and stores fp32,
 * 16 bytes at a time when out's base and row stride allow - the same values either way.  Every sum and scan runs in an order
 * that is a function of the sample index alone: an item's bits depend on that item alone, not on B, the row strides or the
 * alignment; repeated calls and graph replays repeat theirs.  A section with a1 = a2 = 0 (FIR) has nilpotent matrices whose
 * powers are exactly zero: its output is fp32 of the serial float64 recurrence, bit for bit.
 * out may be exactly audio (same base, same row stride); otherwise the two must not overlap.
 * Refused before any launch: B > 65535, S outside [0, 2^24], sections outside 1 .. 8, a table of another size, a row stride
 * below S, out overlapping audio without being audio (E_SHAPE); NULL audio, audio_len, table, out or workspace (E_NULL); a
 * workspace below B W 2 N doubles or off an 8-byte boundary (E_ALIGN).  B = 0 is a no-op. */
int32_t ispk_equalize_segment_samples(void);
int32_t ispk_equalize_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const double* table,
                          int64_t table_doubles, int32_t sections, float* out, int64_t ld_out, int64_t* out_len,
                          double* workspace, int64_t workspace_doubles, int32_t B, int32_t S, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Segmenter (csrc/segment.hip, isp_tts_amd/data/segment.py): long recordings cut into utterances at their pauses and gathered
 * into a padded batch - the inverse of the document join.  No atomics, no host read.  audio fp32 [B][S], unit stride on S, row
 * stride ld_audio >= S.  All integers, `/` floors.
 *   Frames.  The trim frames of ispk_audio_measure_f64.  len = audio_len[b] if 0 <= audio_len[b] <= S, else 0; T = ceil(len /
 *     256); hop sum h_t = the float64 sum of squares of x[256 t, min(256 t + 256, len)); p_t = (((h_t + h_{t+1}) + h_{t+2}) +
 *     h_{t+3}) / 1024 with hops at or past T left out; frame t is active when p_t > thr, thr = (max_t p_t) factor (ref_mode 0) or
 *     ref factor (ref_mode 1), factor = 10^(-top_db / 10) made on the host.  No active frame: no segment.
 *   Ends.  With f, l the first and last active frames: first = max(0, 256 (f - pad)), last = min(len, 256 (l + pad) + 1024): the
 *     (start, end) of ispk_audio_measure_f64 with pad_frames = pad.
 *   Candidates.  Every maximal run of inactive frames u .. v-1 with f < u, v <= l and v - u >= min_silence_frames (>= 4, so
 *     that 256 (u + 3) <= M <= 256 v: the cut lies where no active frame reaches): M = 256 ((u + 3 + v) / 2),
 *     e_j = min(256 (u + 3 + pad), M) where the piece before ends, s_j = max(256 (v - pad), M) where the piece after starts;
 *     j = 0 .. n-1 in frame order, and the virtual boundary e_n = last.
 *   Choice.  One pass, each j looked at at most twice:
 *       cur = first; have = false; j = 0
 *       while j <= n:
 *           L = e_j - cur
 *           if L > max_samples and have:        (the previous pause still fitted: cut there and look at j again)
 *               emit(cur, e_{j-1}); cur = s_{j-1}; have = false; continue
 *           if j == n or L >= target_samples or L > max_samples:
 *               emit(cur, e_j); cur = s_j; have = false
 *           else: have = true
 *           j += 1
 *     emit(s, e) appends the segment (s, e) with flags (e - s > max_samples ? 1 : 0) | (e - s < min_samples ? 2 : 0): 1 "over", a
 *     stretch without a usable pause; 2 "short".  wanted[b] counts every emit, count[b] = min(wanted[b], K) are stored.
 *   Levels of a stored segment, F = {t < T : s <= 256 t < e}: frames = |F|, speech_frames = |F and active|, speech_power /
 *     noise_power = the float64 mean of p_t over the active / inactive frames of F, 0 where that set is empty (their ratio is
 *     the SNR estimate that curation filters on).  Every slot k >= count[b] of the [B][K] outputs is written as zeros.
 *   Gather.  The stored segments of all items in (b, k) order, those with flags & drop left out; the first R of the rest are the
 *     rows r = 0, 1, ..: out[r][i] = audio[b][s + i] for i < n_r = min(e - s, S_out), zeros up to S_out, bit for bit; out_len[r]
 *     = n_r, item[r] = b, index[r] = k, bounds[r] = (s, e), row_flags[r] = flags | (4 when e - s > S_out).  Unused rows:
 *     out_len 0, item -1, index 0, bounds (0, 0), row_flags 0, zeros in out.  rows[0] = the rows used, rows_wanted[0] = what an
 *     unbounded R would have used.  A stored pair that is not 0 <= s <= e <= S (device data) copies nothing: bounds (0, 0).
 * ispk_segment_workspace_bytes  *bytes (HOST memory) = what ispk_segment_plan needs for (B, S): per item the hop sums and frame
 *                       powers (float64 [max(1, ceil(S / 256))] each) and (e_j, s_j) int64 of up to NH / 5 + 1 candidates.
 * ispk_segment_plan     two launches.  Grid (ceil(S / 8192), B): the hop sums, 16-byte loads when audio is 16-byte aligned
 *                       and ld_audio a multiple of four floats - the same values either way; nothing at or past len is read;
 *                       every hop is summed in an order that is a function of the sample index alone (32 samples in order,
 *                       eight such sums in order: ispk_audio_measure_f64's, so the frames are its frames bit for bit).  Grid
 *                       (B), one workgroup per item: frame powers, their max, the candidates compacted in frame order with
 *                       workgroup scans, the choice by one lane, the level sums by one wave per segment in a fixed order; all
 *                       passes stride over the workspace, so T is not bounded by LDS.
 *                       segments int64 [B][K][2]; flags, frames, speech_frames int32 [B][K]; count, wanted int32 [B];
 *                       speech_power, noise_power float64 [B][K]; all contiguous.
 * ispk_segment_gather_f32  two launches.  One workgroup writes the row table - which IS out_len / item / index / bounds /
 *                       row_flags - from count and flags (a thread per item, an exclusive scan over 256 items at a time);
 *                       then grid (ceil(S_out / 4096), R) copies, every workgroup reading its row's (item, start, out_len);
 *                       16-byte loads and stores where bases, strides and the start allow.  out fp32 [R][S_out] at ld_out;
 *                       out_len int64 [R]; item, index, row_flags int32 [R]; bounds int64 [R][2]; rows, rows_wanted int32 [1].
 * An item's plan depends on that item alone - not on B, its place in the batch, the row stride or the alignment; repeated
 * calls and graph replays repeat their bits.
 * Refused before any launch: B > 65535, S (or S_out) outside [0, 2^31), K outside 1 .. 4096, R outside 0 .. 65535,
 * min_silence_frames < 4, pad outside 0 .. 65536, max_samples < 1, target_samples < 0, min_samples < 0, ref_mode not 0 or 1, a
 * negative or NaN factor or ref, drop outside 0 .. 3, a row stride below S (S_out), out overlapping audio (E_SHAPE); NULLs
 * (E_NULL); a workspace below ispk_segment_workspace_bytes or off an 8-byte boundary (E_ALIGN).  B = 0 is a no-op for the plan;
 * the gather then writes its rows as unused. */
int32_t ispk_segment_workspace_bytes(int32_t B, int32_t S, int64_t* bytes);
int32_t ispk_segment_plan(const float* audio, int64_t ld_audio, const int64_t* audio_len, double factor, int32_t ref_mode,
                          double ref, int32_t pad, int32_t min_silence_frames, int64_t target_samples, int64_t max_samples,
                          int64_t min_samples, int64_t* segments, int32_t* flags, int32_t* count, int32_t* wanted,
                          int32_t* frames, int32_t* speech_frames, double* speech_power, double* noise_power, void* workspace,
                          int64_t workspace_bytes, int32_t B, int32_t S, int32_t K, ispk_stream_t stream);
int32_t ispk_segment_gather_f32(const float* audio, int64_t ld_audio, const int64_t* segments, const int32_t* flags,
                                const int32_t* count, int32_t drop, float* out, int64_t ld_out, int64_t* out_len, int32_t* item,
                                int32_t* index, int64_t* bounds, int32_t* row_flags, int32_t* rows, int32_t* rows_wanted,
                                int32_t B, int32_t S, int32_t K, int32_t R, int32_t S_out, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Screen (csrc/screen.hip, isp_tts_amd/data/screen.py): per item of a padded mono batch the measurements that decide whether a
 * piece is fit to train on, and a word of flags.  Four launches, no atomics, no host read.  audio fp32 [B][S], unit stride on S,
 * row stride ld_audio >= S; n = audio_len[b] if 0 <= audio_len[b] <= S, else 0.  x is the item with every non-finite sample
 * read as 0; all integers, `/` floors.
 *   nonfinite int32      the NaN and Inf samples among the item's n.
 *   peak fp32            max |x|, exact.
 *   dc, power float64    (sum x) / n and (sum x^2) / n, summed in float64; 0 at n = 0.
 *   Runs.  A run is a maximal stretch of consecutive samples of one class.
 *     Rail: thr = the fp32 product peak * rail_ratio (rail_mode 0) or rail (rail_mode 1); class + where thr > 0 and x >= thr,
 *       class - where thr > 0 and x <= -thr.  clip_runs int32 = the runs of at least min_run samples, clip_samples int64 = their
 *       samples, clip_first int64 = the start of the first of them or -1, clip_longest int64 = the longest run of any length.
 *     Zero: x == 0.  A dropout is a zero run of at least min_dropout samples that neither starts at sample 0 nor ends at
 *       n - 1 (digital silence in front and behind is padding).  dropout_runs int32, dropout_samples int64, dropout_longest
 *       int64 = their number, their samples and the longest of them (0: none).
 *   ltas float64 [B][513]  the long-term average spectrum: F = max(0, (n - 1024) / 256 + 1) frames, frame f = x[256 f, 256 f +
 *     1024) times the window, no padding; ltas[k] = (1 / F) sum_f |X_f[k]|^2 with the transform and |X|^2 in fp32 and the sum
 *     over the frames in float64, ascending f within a tile of 16 frames, then the tiles in order.  Zeros at F = 0.  tables fp32
 *     [5120]: W_2048^m as (re, im), then the window (the head of ispk_audio_features_f32's tables).
 *   band_bin int32       with top = max ltas[2 .. 512]: the largest k in 0 .. 512 with ltas[k] >= top * band_factor (float64;
 *     band_factor = 10^(-band_db / 10) made on the host); -1 when F = 0 or top = 0.
 *   flags int32          1 clipped: clip_runs > 0;  2 narrow: min_band_bin >= 0 and 0 <= band_bin < min_band_bin;  4 dc: |dc| >
 *     max_dc;  8 dropout: dropout_runs > 0;  16 nonfinite: nonfinite > 0;  32 quiet: peak <= min_peak;  64 short: F = 0.
 *   parts               1 levels and runs, 2 spectrum, 3 both.  Without 1 no runs are looked for (the six run outputs read as
 *     none, clip_first -1); without 2 ltas is zeros and band_bin -1.  The flags follow the outputs.
 * ispk_screen_tile_samples      samples of one item per workgroup (4096; 16 frames start in them): the tests' tile edges.
 * ispk_screen_workspace_bytes   *bytes (HOST memory) = what ispk_screen_f64 needs for (B, S): per item and tile of 4,096 samples a
 *                       spectrum partial (float64 [513]), the tile's statistics and two run summaries (88 B), and 8 B per item.
 * ispk_screen_f64       grid (ceil(S / 4096), B): stages the tile and the 768 samples its last frame reads (16-byte loads where
 *                       base and stride allow - the same values either way; nothing at or past n is read), statistics, zero-run
 *                       summary, the tile's frames through the 1024 / 256 FFT of csrc/stft_tile.h.  Grid (B): the item's
 *                       statistics, ltas, band_bin, dropouts, thr.  Grid (ceil(S / 4096), B): the rail-run summaries.  Grid (B):
 *                       the clip outputs and the flags.  All outputs contiguous.
 * An item's results depend on that item alone - not on B, S, the row stride, the alignment or what lies behind n; repeated
 * calls and graph replays repeat their bits.
 * Refused before any launch: B > 65535, S outside [0, 2^24], parts outside 1 .. 3, rail_mode not 0 or 1, rail_ratio outside
 * (0, 1] (mode 0), a rail that is not positive and finite (mode 1), min_run or min_dropout below 1, band_factor outside (0, 1),
 * min_band_bin outside -1 .. 513, a negative or NaN max_dc or min_peak, a row stride below S (E_SHAPE); NULLs (E_NULL); a
 * workspace below ispk_screen_workspace_bytes or off an 8-byte boundary (E_ALIGN).  B = 0 is a no-op. */
int32_t ispk_screen_tile_samples(void);
int32_t ispk_screen_workspace_bytes(int32_t B, int32_t S, int64_t* bytes);
int32_t ispk_screen_f64(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables, int32_t parts,
                        int32_t rail_mode, float rail, float rail_ratio, int32_t min_run, int32_t min_dropout, double band_factor,
                        int32_t min_band_bin, double max_dc, double min_peak, int32_t* nonfinite, float* peak, double* dc,
                        double* power, int32_t* clip_runs, int64_t* clip_samples, int64_t* clip_longest, int64_t* clip_first,
                        int32_t* dropout_runs, int64_t* dropout_samples, int64_t* dropout_longest, double* ltas, int32_t* band_bin,
                        int32_t* flags, void* workspace, int64_t workspace_bytes, int32_t B, int32_t S, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Declipper (csrc/declip.hip, isp_tts_amd/data/declip.py): the clipped samples that the screen finds, restored by Janssen's AR
 * interpolation (Janssen, Veldhuis & Vries 1986) in float64.  Four launches, no atomics, no host read.  audio fp32 [B][S], unit
 * stride on S, row stride ld_audio >= S; n = audio_len[b] if 0 <= audio_len[b] <= S, else 0.  x is the item with every
 * non-finite sample read as 0 (such a sample is copied through unchanged); all integers, `/` floors.
 *   peak, thr, runs      the screen's, value for value: thr = the fp32 product max|x| * rail_ratio (rail_mode 0) or rail
 *     (rail_mode 1); a sample is at the rail when |x| >= thr > 0; a run is a maximal stretch of at-rail samples of one sign.
 *     The UNKNOWN samples are those of the runs of at least min_run samples; clip_samples int64 counts them.
 *   Segments.  Segment j = [512 j, 512 j + 512) within [0, n), solved in its window [512 j - 256, 512 j + 768) within [0, n)
 *     (N <= 1024 samples): every unknown of the window is solved jointly, the segment's own are kept.  A segment without an
 *     unknown of its own is a copy and counts nowhere.  A segment whose window holds more than ispk_declip_max_unknowns() = 256
 *     unknowns, or in which a non-finite intermediate appears (a prediction error or a pivot that is not > 0, a solution that is
 *     not finite), is left as it is and counted in dense.
 *   A pass over the window w (float64; the unknowns start at their clipped values), `iterations` times:
 *     r[k] = sum_i w[i] w[i + k], k = 0 .. order; r[0] *= 1 + 1e-9; r[0] == 0 ends the passes.  Levinson-Durbin gives a[0 ..
 *     order], a[0] = 1.  b[k] = sum_i a[i] a[i + k].  B[s][t] = b[|s - t|] for |s - t| <= order, else 0; U the window's unknown
 *     positions, K the rest: solve B_UU x_U = -B_UK x_K (banded Cholesky, two triangular solves).  Then w[u] = s max(s x_u, s
 *     orig_u), s the sign of the run: a restored sample never lies inside the rail.
 *   out fp32 [B][S] (row stride ld_out >= S): the restored samples are the float64 values rounded once; every other sample
 *     below n keeps its bits; zeros from n on.  out_len int64 = n.  peak fp32 = max |out| (it may exceed 1).  restored int64 =
 *     the samples replaced; windows, dense int32 = the segments solved and left.  flags int32: 1 restored (restored > 0), 2 dense
 *     (dense > 0), 4 skipped.  in_flags int32 [B] or NULL: the screen's flags; an item without bit 1 there is copied bit for
 *     bit, gets flag 4 and zeros in clip_samples, restored, windows and dense.
 * ispk_declip_max_unknowns     256.
 * ispk_declip_workspace_bytes  *bytes (HOST memory) = what ispk_declip_f64 needs for (B, S): per item 16 B per segment of 512
 *                       samples and 4 B per tile of 4,096, rounded up to 8 B.
 * ispk_declip_f64       grid (ceil(S / 4096), B): the tiles' peaks.  Grid (B): thr.  Grid (ceil(S / 512), B): the segments (81,408
 *                       B of LDS, two workgroups per CU; a segment with nothing at the rail is an 8-byte-wide copy).  Grid (B): the
 *                       counts, the output's peak, the flags.  All outputs but out contiguous.
 * An item's results depend on that item alone - not on B, S, the row strides, the alignment or what lies behind n; repeated
 * calls and graph replays repeat their bits.
 * Refused before any launch: B > 65535, S outside [0, 2^24], rail_mode not 0 or 1, rail_ratio outside (0, 1] (mode 0), a rail
 * that is not positive and finite (mode 1), min_run outside 1 .. 64, order outside 1 .. 32, iterations outside 1 .. 8, a row
 * stride below S, out overlapping audio (E_SHAPE); NULLs other than in_flags (E_NULL); a workspace below
 * ispk_declip_workspace_bytes or off an 8-byte boundary (E_ALIGN).  B = 0 is a no-op. */
int32_t ispk_declip_max_unknowns(void);
int32_t ispk_declip_workspace_bytes(int32_t B, int32_t S, int64_t* bytes);
int32_t ispk_declip_f64(const float* audio, int64_t ld_audio, const int64_t* audio_len, const int32_t* in_flags, int32_t rail_mode,
                        float rail, float rail_ratio, int32_t min_run, int32_t order, int32_t iterations, float* out, int64_t ld_out,
                        int64_t* out_len, float* thr, float* peak, int64_t* clip_samples, int64_t* restored, int32_t* windows,
                        int32_t* dense, int32_t* flags, void* workspace, int64_t workspace_bytes, int32_t B, int32_t S,
                        ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * NoiseReducer (csrc/noise.hip, isp_tts_amd/data/noise.py): stationary noise reduction.  The noise spectrum of an item is
 * learnt from its own pauses (the profile), then every frame is attenuated with a Wiener gain smoothed over time and frequency
 * (the reduce).  audio fp32 [B][S], unit stride on S, row stride ld_audio >= S; n = audio_len[b] if 0 <= audio_len[b] <= S,
 * else 0.  All integers, `/` floors.
 *   STFT.  ispk_denoise_f32's: N = 1024, hop 256, K = 513 bins, w the periodic Hann window made in float64 and rounded once,
 *     xp[p] = x[r(p - 512)] (reflect padding), X_f[k] = sum_j xp[256 f + j] w[j] exp(-2 pi i j k / 1024), f < F = 1 + n / 256.
 *     Defined for n >= 513; a shorter item has frames = 0, the flag 2 "short", and is copied bit for bit by the reduce.
 *   Noise frames.  The trim frames of ispk_audio_measure_f64 / ispk_segment_plan: T = ceil(n / 256), the float64 hop sums h_t in
 *     that fixed order, p_t = (((h_t + h_{t+1}) + h_{t+2}) + h_{t+3}) / 1024 with hops at or past T left out, frame t active
 *     when p_t > thr, thr = (max_t p_t) factor (ref_mode 0) or ref factor (ref_mode 1), factor = 10^(-top_db / 10) made on the
 *     host.  STFT frame f and trim frame t = f - 2 cover the same samples [256 t, 256 t + 1024).  Frame f is a noise frame when
 *     2 <= f <= n / 256 - 2 (no reflection; the frame lies wholly inside the item) and every trim frame u with |u - t| <= guard
 *     and 0 <= u < T is inactive.
 *   Profile.  noise[b][k] = the float64 mean over the item's noise frames of |X_f[k]|^2, the transform and |X|^2 in fp32 and
 *     the sum in float64: ascending f within a tile of the 16 frames [16 w, 16 w + 16), then the tiles in order.  noise_frames
 *     [b] = their number, frames[b] = F (0 when short).  flags[b] = (noise_frames < min_noise_frames ? 1 : 0) | (n < 513 ? 2 :
 *     0): 1 "no_profile" - the row is zeros.
 *   Raw gain.  g_f[k] = max(1 - over noise[k] / |X_f[k]|^2, g_min) where |X_f[k]|^2 > 0, else g_min; g_min = 10^(-reduce_db /
 *     20) in (0, 1] made on the host.  In fp32 with nb[k] = the fp32 rounding of the float64 product over noise[k], IEEE
 *     division; a quotient that is infinite or NaN gives g_min.
 *   Smoothed gain.  Triangular weights w_t[d] = Tt + 1 - |d|, |d| <= Tt, and w_k[e] = Fk + 1 - |e|, |e| <= Fk:
 *     h_f[k] = (sum_e w_k[e] g_f[k+e]) / (sum_e w_k[e]) over the bins 0 <= k + e <= 512 that exist, then G_f[k] = (sum_d w_t[d]
 *     h_{f+d}[k]) / (sum_d w_t[d]) over the frames 0 <= f + d < F that exist; e and d ascending, with fma.  The cells that exist
 *     form a rectangle, so this is sum w_t w_k g / sum w_t w_k over them.
 *   Output.  Y_f[k] = X_f[k] G_f[k], y_f = irfft_1024(Y_f), out[s] = (sum_f w[j] y_f[j]) / (sum_f w[j]^2), j = s + 512 - 256 f,
 *     exactly as ispk_denoise_f32; 0 for n <= s < S.
 * ispk_noise_tile_samples     output samples of one item per workgroup of the reduce (4096): the tests' tile edges.
 * ispk_noise_workspace_bytes  *bytes (HOST memory) = what ispk_noise_profile_f64 needs for (B, S): per item the hop sums
 *                       (float64 [NH], NH = max(1, ceil(S / 256))), two int32 [NH + 1] (the active frames before t; the noise
 *                       frame mask), a float64 [513] partial per tile of 16 frames (S / 4096 + 1 of them) and one word.
 * ispk_noise_profile_f64  four launches, no atomics.  Grid (ceil(S / 8192), B): the hop sums.  Grid (B): frame powers, thr, the
 *                       mask, noise_frames, frames, flags.  Grid (S / 4096 + 1, B): each workgroup transforms the noise frames
 *                       among its 16 (the 1024 / 256 FFT of csrc/stft_tile.h) and writes its float64 partial.  Grid (B): noise.
 *                       noise float64 [B][513]; noise_frames, frames, flags int32 [B]; all contiguous.  tables fp32 [5120]:
 *                       ispk_denoise_f32's.  16-byte loads where base and stride allow - the same values either way; nothing
 *                       at or past n is read.
 * ispk_noise_reduce_f32   one launch: the tile of ispk_denoise_f32 with the smoothed gain between analysis and synthesis; the
 *                       raw gains of the Tt frames on either side of a tile's frames come from extra forward transforms,
 *                       nothing lies in HBM in between.  noise float64 [P][513]; item b takes row index[b] (int32 [B]; NULL: row
 *                       b).  flags int32 [B] (NULL: none): the profile's.  An item is copied bit for bit (zeros from n on) when
 *                       n < 513, when its flag has bit 1 or 2 set, or when its row lies outside [0, P).  audio_len may be NULL
 *                       (every item has S samples).  out fp32 [B][S] at ld_out >= S may not be audio.  Scalar loads and
 *                       stores: no alignment requirement.
 * An item's results depend on that item (and its profile row) alone - not on B, S, the row strides, the alignment or what lies
 * behind n; every sum runs in a fixed order; repeated calls and graph replays repeat their bits.
 * Refused before any launch.  Profile: B > 65535, S outside [0, 2^24], ref_mode not 0 or 1, a negative or NaN factor or ref,
 * guard outside 0 .. 65536, min_noise_frames < 1, a row stride below S (E_SHAPE); NULLs (E_NULL); a workspace below
 * ispk_noise_workspace_bytes or off an 8-byte boundary (E_ALIGN).  Reduce: NULL audio, tables, noise or out (E_NULL); B > 65535,
 * S > 2^31 - 8193, P < 1, a row stride below S, out == audio, over negative or not finite, g_min outside (0, 1], smooth_frames
 * outside 0 .. 2, smooth_bins outside 0 .. 8 (E_SHAPE).  B = 0 or S = 0 is a no-op for both. */
int32_t ispk_noise_tile_samples(void);
int32_t ispk_noise_workspace_bytes(int32_t B, int32_t S, int64_t* bytes);
int32_t ispk_noise_profile_f64(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables, double factor,
                               int32_t ref_mode, double ref, int32_t guard, int32_t min_noise_frames, double* noise,
                               int32_t* noise_frames, int32_t* frames, int32_t* flags, void* workspace, int64_t workspace_bytes,
                               int32_t B, int32_t S, ispk_stream_t stream);
int32_t ispk_noise_reduce_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables,
                              const double* noise, int32_t P, const int32_t* index, const int32_t* flags, double over,
                              double g_min, int32_t smooth_frames, int32_t smooth_bins, float* out, int64_t ld_out, int32_t B,
                              int32_t S, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * TimeStretch (csrc/stretch.hip, isp_tts_amd/data/stretch.py): tempo without pitch, the phase vocoder of torchaudio / librosa.
 * (data.PitchShift is this followed by ispk_resample_f32.)  audio fp32 [B][S], unit stride on S, row stride ld_audio >= S;
 * n = audio_len[b] if 0 <= audio_len[b] <= S, else 0; r = rates[b] (float64 [B], device memory) or, with rates NULL, the scalar
 * `rate`; 0.5 <= r <= 2.  Integers, `/` floors, unless said otherwise.
 *   Analysis.  ispk_denoise_f32's STFT: N = 1024, hop 256, K = 513 bins, w the periodic Hann window made in float64 and rounded
 *     once, xp[p] = x[r(p - 512)] (reflect padding), X_i[k] = sum_j xp[256 i + j] w[j] exp(-2 pi i j k / 1024), i < F = 1 + n /
 *     256, transforms in fp32.  X_F = X_{F+1} = 0.
 *   Output frames.  t_j = j r (a float64 product, not a running sum); Fo = the smallest j >= 0 with j r >= F; i_j = floor(t_j),
 *     a_j = t_j - i_j.
 *   Magnitude.  M_j[k] = (1 - a_j) |X_{i_j}[k]| + a_j |X_{i_j + 1}[k]|.
 *   Phase.  P_0[k] = arg X_0[k], P_{j+1}[k] = P_j[k] + w_k + wrap(arg X_{i_j + 1}[k] - arg X_{i_j}[k] - w_k), w_k = pi k / 2 the
 *     expected advance per hop, wrap(d) = d - 2 pi round(d / (2 pi)), arg 0 = 0.  Only exp(i P) is used and w_k + wrap(d - w_k)
 *     = d modulo 2 pi, so the kernels multiply unit phasors instead, in float64 from the fp32 spectra: e_0 = u(X_0), e_{j+1} =
 *     e_j u(X_{i_j + 1}) conj(u(X_{i_j})), u(z) = z / |z|, u(0) = 1, ascending j.  Nothing is accumulated in fp32.
 *   Synthesis.  Y_j[k] = M_j[k] exp(i P_j[k]), y_j = irfft_1024(Y_j), out[s] = (sum_j w[q] y_j[q]) / (sum_j w[q]^2), q = s + 512
 *     - 256 j, over the frames j < Fo in ascending order, exactly as ispk_denoise_f32; 0 <= s < out_len, zeros behind.
 *   Length.  wanted = round-half-even(n / r), an int64 from the float64 quotient; out_len = min(wanted, out_samples).  Every
 *     s < wanted lies under at least one output frame, since 256 F > n.
 *   flags[b], int32: 1 "short" (n < 513, no reflection), 4 "bad_rate" (a device rate that is NaN or outside [0.5, 2]) - such an
 *     item is copied bit for bit with wanted = n and out_len = min(n, out_samples); 2 "truncated" (wanted > out_samples).
 * ispk_stretch_tile_samples     output samples of one item per workgroup of the synthesis (4096): the tests' tile edges.
 * ispk_stretch_workspace_bytes  *bytes (HOST memory) = what ispk_stretch_f32 needs for (B, S, out_samples): per item and output
 *                       tile (max(1, ceil(out_samples / 4096)) of them) one phasor row, float64 re [513] then im [513].
 * ispk_stretch_f32      three launches, no atomics, nothing per (frame, bin) in HBM.  Grid (tiles - 1, B): chunk w = the output
 *                       frames [max(0, 16 w - 1), 16 w + 15), from the first that touches output tile w to the first that touches
 *                       tile w + 1; the workgroup transforms the analysis frames they read (forward only, four at a time through a
 *                       ring of 8 spectra) and writes the product of their steps per bin (chunk 0: times u(X_0)).  Grid (B): the
 *                       exclusive product over the chunks in order, in place; out_len, wanted (int64 [B]) and flags (int32 [B]).
 *                       Grid (tiles, B): the tile of ispk_denoise_f32 - the output frames that touch it, started from the chunk's
 *                       prefix, the analysis frames through the same ring, Y_j / 1024 into the frame's slot, the inverses, the
 *                       overlap-add.  tables fp32 [5120]: ispk_denoise_f32's.  out fp32 [B][out_samples] at ld_out >=
 *                       out_samples may not be audio.  Scalar loads and stores: no alignment requirement on audio or out.
 * An item's results depend on its samples, n and r alone - not on B, S, the row strides, out_samples (where it is at least
 * wanted), its neighbours or what lies behind n; every product and sum runs in a fixed order; repeated calls and graph replays
 * repeat their bits.
 * Refused before any launch: B > 65535, S or out_samples outside [1, 2^24] (workspace_bytes: [0, 2^24]), with rates NULL a scalar
 * rate that is NaN or outside [0.5, 2], a row stride below the row, out == audio (E_SHAPE); NULLs other than rates (E_NULL); a
 * workspace below ispk_stretch_workspace_bytes or off an 8-byte boundary (E_ALIGN).  B = 0 is a no-op. */
int32_t ispk_stretch_tile_samples(void);
int32_t ispk_stretch_workspace_bytes(int32_t B, int32_t S, int32_t out_samples, int64_t* bytes);
int32_t ispk_stretch_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables, double rate,
                         const double* rates, float* out, int64_t ld_out, int32_t out_samples, int64_t* out_len, int64_t* wanted,
                         int32_t* flags, void* workspace, int64_t workspace_bytes, int32_t B, int32_t S, ispk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * PitchTracker (csrc/pyin.hip, isp_tts_amd/data/pitch.py): probabilistic YIN (Mauch & Dixon 2014) as librosa.pyin states it, with
 * center = True framing on the hop of ispk_audio_features_f32, then a Viterbi decode.  audio fp32 [B][S], unit stride on S, row
 * stride ld_audio >= S; n = audio_len[b] if 256 <= audio_len[b] <= S, else no frames; Tb = (n - 256) / 256 + 1 frames (the
 * extractor's mel_len).  Integers, `/` floors, tiny = DBL_MIN.
 *   Frame t: x[j] = audio[256 t + 128 - 512 + j], j < 2048, 0 outside [0, n): its YIN window x[0, 1024) is centred where mel frame
 *     t is centred.
 *   d(tau) = sum_{j<1024} (x[j] - x[j + tau])^2 = (S[1023] + S[tau + 1023] - S[tau - 1]) - 2 c(tau), S the inclusive prefix sums of
 *     x^2 (float64), c(tau) = sum_{j<1024} x[j] x[j + tau] by 2,048-point transforms in fp32 (nothing wraps: j + tau < 2048).
 *   y[i] = d(tau) / (sum_{k=1..tau} d(k) / tau + tiny), tau = min_period + i, i < n_lag = max_period - min_period + 1 (float64).
 *   Troughs: i = 0 if y[0] < y[1]; 0 < i < n_lag - 1 if y[i] < y[i-1] and y[i] <= y[i+1]; never the last lag.
 *   Shift: 0 at i = 0, else -b / a with a = y[i+1] + y[i-1] - 2 y[i], b = (y[i+1] - y[i-1]) / 2 where |b| < |a|, else 0.
 *   Probability of trough j (in lag order): sum over the thresholds s (ascending) with y_j < thr[s] of prior[s] (1 - e^-2) e^(-2 k)
 *     / (1 - e^(-2 N)), N the troughs below thr[s], k the number of them in front of j; the lowest trough (the first of equal
 *     heights) also gets 0.01 times the prior of the thresholds it does not lie below.
 *   Bin of trough j: clip(rint(12 bps log2(sample_rate / (tau + shift) / f_min)), 0, NB - 1), rint half to even; the troughs of one
 *     bin are taken in lag order and the last one's probability stands (also when it is 0).
 *   `prior` float64 [ISPK_PYIN_TABLE_DOUBLES], device memory: thr [100], prior [100], its exclusive running sum [101], (1 - e^-2)
 *     e^(-2 k) for k < 512, 1 / (1 - e^(-2 N)) for N <= 512 (entry 0 unused) - data.pitch.observation_table().
 *   `tables` fp32, at least 4,096 values: W_2048^m as (re, im), made in float64 and rounded once (ispk_audio_features_f32's).
 * ispk_pyin_frames_per_block  frames of one item per workgroup of the observation (8): the tests' tile edge.
 * ispk_pyin_observe_f32   one launch, grid (ceil(M / 8), B).  obs fp32 [B][M][NB], contiguous: row t of item b holds the voiced
 *                       probabilities of frame t, zeros for Tb <= t < M; frames int64 [B] (may be NULL) receives Tb.  M >= the
 *                       frames of S.  Nothing at or past n is read.
 * Decode: Viterbi over 2 NB states, voiced bins then unvoiced bins, for item b over its n = obs_len[b] frames (int64 [B]; NULL: M;
 *   a value outside [0, M] counts as 0).
 *   Observations.  obs_is_log = 0: obs fp32 [B][M][NB] as above; vp = clip(sum of the row, 0, 1) in float64; logobs[j] = log(max(p_j,
 *     0) + tiny) for j < NB and log((1 - vp) / NB + tiny) for every j >= NB.  obs_is_log != 0: obs float64 [B][M][2 NB] holds logobs
 *     itself (voiced_prob is then written as 0).
 *   `trans` float64 [width + NB + 3], device memory: logtri [width] (the log of the triangular window, centre at (width - 1) / 2),
 *     lognorm [NB] (the log of each source row's window sum inside [0, NB)), log stay, log switch, log init - data.pitch.
 *     transition_table().  h = (width - 1) / 2.
 *   Recursion, float64, plain additions (no fused multiply-add occurs): delta_0[j] = log init + logobs_0[j]; delta'[i] = delta[i] -
 *     lognorm[bin(i)]; per target bin c and per source block (voiced, unvoiced) m = max over the source bins i = c - h .. c + h
 *     inside [0, NB), ascending, first maximum, of delta'[i] + logtri[h + c - i]; the voiced target takes max(m_voiced + stay,
 *     m_unvoiced + switch), the unvoiced one max(m_voiced + switch, m_unvoiced + stay), the voiced source on a tie; new[j] = that +
 *     logobs[j].  This is max_i(delta'[i] + logtri[..] + (stay | switch)) over the predecessors in ascending state order with the
 *     first maximum winning, the constant added after the block maximum.  The path ends in the lowest-index maximum of the last
 *     frame; log_prob is that maximum.
 *   Outputs, all [B][M] contiguous: state int32 (-1 past n); f0 fp32 = (float)(f_min 2^(bin / (12 bps))) where voiced, 0 where
 *     unvoiced or past n; voiced int32 (1 / 0); voiced_prob fp32 = vp; pitch fp32 (may be NULL) = (f0 - pitch_mean) / pitch_std in
 *     fp32 for t < n, 0 past n; frames int64 [B] (may be NULL) = n; log_prob float64 [B] (0 for n = 0).
 * ispk_pyin_workspace_bytes  *bytes (HOST memory) = what ispk_pyin_decode_f64 needs: two float64 per (item, frame) and one
 *                       backpointer byte per (item, frame, state), rounded up to 8.
 * ispk_pyin_decode_f64  one launch, grid (B): one workgroup owns an item, its scores stay in LDS, one lane walks back.
 * Both entries: no atomics, no host read, every sum and maximum in a fixed order - an item's results depend on that item alone
 * (not on B, S, M or its neighbours) and repeated calls and graph replays repeat their bits.
 * Refused before any launch.  Observe: B > 65535, S outside [0, 2^30], ld_audio < S, M below the frames of S, NB outside [1, 1024],
 * M NB >= 2^31, periods outside 1 <= min_period, min_period + 2 <= max_period <= 1022, sample_rate or f_min not positive,
 * bins_per_semitone outside [1, 100] (E_SHAPE); NULLs other than frames (E_NULL).  Decode: B > 65535, M > 2^22, NB outside [1,
 * 1024], width even or outside [1, 127], f_min not positive, bins_per_semitone outside [1, 100], pitch given with pitch_std 0
 * (E_SHAPE); NULLs other than obs_len, pitch and frames (E_NULL); a workspace below ispk_pyin_workspace_bytes or off an 8-byte
 * boundary (E_ALIGN).  B = 0 is a no-op for both, M = 0 for the observation. */
#define ISPK_PYIN_THRESHOLDS 100
#define ISPK_PYIN_MAX_BINS 1024
#define ISPK_PYIN_TABLE_DOUBLES 1326
int32_t ispk_pyin_frames_per_block(void);
int32_t ispk_pyin_workspace_bytes(int32_t B, int32_t M, int32_t NB, int64_t* bytes);
int32_t ispk_pyin_observe_f32(const float* audio, int64_t ld_audio, const int64_t* audio_len, const float* tables,
                              const double* prior, float* obs, int64_t* frames, int32_t B, int32_t S, int32_t M, int32_t NB,
                              int32_t min_period, int32_t max_period, double sample_rate, double f_min,
                              int32_t bins_per_semitone, ispk_stream_t stream);
int32_t ispk_pyin_decode_f64(const void* obs, int32_t obs_is_log, const int64_t* obs_len, const double* trans, int32_t width,
                             double f_min, int32_t bins_per_semitone, float pitch_mean, float pitch_std, int32_t* state,
                             float* f0, int32_t* voiced, float* voiced_prob, float* pitch, int64_t* frames, double* log_prob,
                             void* workspace, int64_t workspace_bytes, int32_t B, int32_t M, int32_t NB, ispk_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Griffin-Lim mel inversion (csrc/griffinlim.hip; isp_tts_amd/griffinlim.py): waveforms from mel without a vocoder checkpoint,
 * in the framing of ispk_audio_features_f32: N = 1024, hop 256, K = 513 bins, w the periodic Hann window, 384 zeros on both
 * sides, no centring.  Utterance b has Tb = mel_len[b] frames (NULL: T; a value outside [0, T] counts as 0) and n = 256 Tb
 * samples.  Audio is a padded mono batch fp32 [B][256 T] at a row stride >= 256 T; the magnitude is fp32 [B][T][513] with
 * contiguous frame rows (stride 513) and a leading stride ld_mag >= 513 T.
 *
 * ispk_griffinlim_tile_samples  output samples of one utterance per workgroup (4096): the tests' tile edges.
 * ispk_mel_to_linear_f32      mag[b][f][k] = max(sum_m P[k][m] exp(mel[b][m][f]), 0) for f < Tb, the sum in ascending m with
 *                             fma, accurate expf.  mel fp32 or fp16 (mel_f16 != 0) [B][n_mels][T] at element strides mel_sb,
 *                             mel_sc, mel_st; pinv_t fp32 [n_mels][513] = P transposed (P the pseudo-inverse of the mel
 *                             filterbank, made in float64 and rounded once), device memory.  Frames at or past Tb are neither
 *                             read nor written.  Refused: NULL mel, pinv_t or mag (E_NULL); B > 65535, n_mels outside 1 .. 128,
 *                             T > 8388575, ld_mag < 513 T (E_SHAPE).  B = 0 or T = 0 is a no-op.
 * ispk_griffinlim_step_f32    one launch.  With xp[p] = x[p - 384] inside [0, n) and 0 elsewhere:
 *                               mode ISPK_GRIFFINLIM_STEP (one projection of the iteration, x = audio):
 *                                 X_f[k] = sum_j xp[256 f + j] w[j] exp(-2 pi i j k / 1024)          f < Tb, k <= 512
 *                                 Y_f[k] = M_f[k] X_f[k] / |X_f[k]|, M_f[k] where |X_f[k]|^2 = 0 in fp32; M = mag[b][f][k]
 *                               mode ISPK_GRIFFINLIM_INIT (the initial waveform; audio is not read and may be NULL):
 *                                 Y_f[k] = M_f[k] exp(2 pi i u), u = (h >> 8) 2^-24, h = drop_hash(mix_seed(seed), 513 f + k)
 *                                          of csrc/dropout.h (32-bit index), by an accurate sincospif: a function of
 *                                          (seed, f, k) alone
 *                               then in both modes
 *                                 y_f    = irfft_1024(Y_f) (1 / 1024; imaginary parts of bins 0 and 512 dropped)
 *                                 out[s] = (sum_f w[j] y_f[j]) / (sum_f w[j]^2), j = s + 384 - 256 f, over the frames f < Tb
 *                                          with 0 <= j < 1024, both sums in ascending f; 0 for n <= s < 256 T
 *                             IEEE square root and division; M = 0 gives Y = 0 exactly.  The w^2 sum is positive for every
 *                             s < n and every Tb >= 1.  audio_len (may be NULL): int64 [B] on the device, receives 256 Tb.
 *                             tables fp32 [5120] = W_2048^m as (re, im), then w, both made in float64 and rounded once
 *                             (ispk_denoise_f32's).  Nothing at or past n (audio) or Tb (mag) is read.  An utterance's samples
 *                             depend on that utterance and the seed alone, every sum runs in a fixed order, no atomics: a
 *                             ragged batch, repeated calls and graph replays are bit-identical.  Scalar loads and stores: no
 *                             alignment requirement.  Refused: a mode other than the two (E_UNSUP); NULL mag, tables or out,
 *                             or NULL audio in mode STEP (E_NULL); B > 65535, T > 8388575, a row stride shorter than its
 *                             row, out == audio in mode STEP (the neighbouring tiles read the halo) (E_SHAPE).  B = 0 or
 *                             T = 0 is a no-op.
 * ispk_griffinlim_fast_step_f32  one launch: mode STEP applied to x[i] = fma(-alpha, prev[i], audio[i]) for i in [0, n), the
 *                             fast (momentum) iteration with alpha = momentum / (1 + momentum).  The textbook form takes the
 *                             phase of STFT(x_n) - alpha STFT(x_{n-1}); the STFT is linear, so that is STFT(x_n - alpha
 *                             x_{n-1}) and no spectrum is kept between launches.  prev is a second batch like audio at its own
 *                             row stride ld_prev; nothing at or past n is read from either.  Everything else, the bit-identity
 *                             guarantees included, is mode STEP's; ispk_griffinlim_step_f32 itself runs the code it ran
 *                             before (the difference is a compile-time variant of the kernel).  Refused: NULL audio, prev,
 *                             mag, tables or out (E_NULL); B > 65535, T > 8388575, a row stride (ld_prev included) shorter
 *                             than its row, out == audio or out == prev (the neighbouring tiles read the halo), alpha
 *                             outside [0, 1) or NaN (E_SHAPE).  B = 0 or T = 0 is a no-op.
 * ispk_griffinlim_error_f32   two launches, no atomics: err[b] = || |X| - M ||_F / || M ||_F over the frames f < Tb and the
 *                             513 bins, X the analysis of x = audio above (the spectral convergence).  The first launch (16
 *                             frames per workgroup, each frame in exactly one) writes work[b][f] = (num_f, den_f) =
 *                             (sum_k (sqrt(|X_f[k]|^2) - M_f[k])^2, sum_k M_f[k]^2) for f < Tb in fp32: per-thread partials over
 *                             k = t, t + 128, .. in ascending k with fma, then a fixed tree; frames at or past Tb are not
 *                             written.  The second (one workgroup per utterance) sums work[b][0 .. Tb) in float64 in a fixed
 *                             order and writes err[b] = (float)sqrt(num / den); Tb = 0 gives 0, den = 0 gives 0 if num = 0
 *                             and +inf otherwise.  work is fp32 [B][T][2] scratch at a row stride ld_work >= 2 T, err fp32
 *                             [B], both device memory.  A frame's two numbers depend on (n, f) alone: a ragged batch gives
 *                             each utterance the bits it gets alone.  Refused: NULL audio, mag, tables, work or err (E_NULL);
 *                             B > 65535, T > 8388575, a row stride shorter than its row (E_SHAPE).  B = 0 or T = 0 is a
 *                             no-op (err is not written). */
#define ISPK_GRIFFINLIM_STEP 0
#define ISPK_GRIFFINLIM_INIT 1
int32_t ispk_griffinlim_tile_samples(void);
int32_t ispk_mel_to_linear_f32(const void* mel, int32_t mel_f16, int64_t mel_sb, int64_t mel_sc, int64_t mel_st,
                               const int64_t* mel_len, const float* pinv_t, float* mag, int64_t ld_mag, int32_t B,
                               int32_t n_mels, int32_t T, ispk_stream_t stream);
int32_t ispk_griffinlim_step_f32(const float* audio, int64_t ld_audio, const float* mag, int64_t ld_mag,
                                 const int64_t* mel_len, const float* tables, float* out, int64_t ld_out, int64_t* audio_len,
                                 int32_t B, int32_t T, int32_t mode, uint64_t seed, ispk_stream_t stream);
int32_t ispk_griffinlim_fast_step_f32(const float* audio, int64_t ld_audio, const float* prev, int64_t ld_prev, float alpha,
                                      const float* mag, int64_t ld_mag, const int64_t* mel_len, const float* tables,
                                      float* out, int64_t ld_out, int64_t* audio_len, int32_t B, int32_t T, ispk_stream_t stream);
int32_t ispk_griffinlim_error_f32(const float* audio, int64_t ld_audio, const float* mag, int64_t ld_mag,
                                  const int64_t* mel_len, const float* tables, float* work, int64_t ld_work, float* err,
                                  int32_t B, int32_t T, ispk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ISPK_H */
