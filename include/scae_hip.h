/*
 * scae_hip.h -- C ABI of libscae_hip.so: the MI355X (gfx950) kernels of the
 * SCAE forward/backward hot path.
 *
 * Drop-in boundary.  The reference (bdsaglam/torch-scae) has no FFI of its
 * own -- every op on the path is a stock ATen call made from Python
 * (SURVEY.md section 8b).  The entry points below are therefore what a
 * maintainer of the reference would bind (ctypes / cffi stub in
 * INTEGRATION.md) to replace each ATen op cluster, one launcher per cluster,
 * each citing the reference lines it replaces (paths relative to the
 * reference checkout).
 *
 * Conventions
 *   - plain pointers + sizes only; no torch types, no exceptions, no
 *     allocation, no global state (the one stateful object, a launch list,
 *     is a handle the caller holds), no implicit synchronisation;
 *   - every pointer is a DEVICE pointer to densely packed (contiguous,
 *     row-major, last index fastest) float32 unless stated otherwise; the
 *     caller owns every buffer, including the "saved"/"partial" workspaces;
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it
 *     and the call returns immediately (safe under hipGraph capture);
 *   - launchers are re-entrant (autograd calls the *_bwd ones from its own
 *     worker thread);
 *   - return value: 0 on success, SCAE_ERR_* (negative) for rejected
 *     arguments, otherwise the positive hipError_t of the failed launch;
 *   - pointers documented "nullable" select a mode of the reference op.
 */
#ifndef SCAE_HIP_H
#define SCAE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: scae_launch_list_begin(stream) -> handle; scae_conv3x3_relayout* write the packed
 * fragment-major filter copy behind wf (scae_conv3x3_wf_floats); scae_mlp_chain_desc has
 * row_tile / bf16; scae_decoder_desc has bwd_resident; scae_first_layer_desc has out_h /
 * rwfh / rwdh
 * 3: launch lists record one stream -- scae_launch_list_side_stream / _order / _run2 /
 * _side_size are gone; scae_decoder_desc loses bwd_resident
 * 4: the library reads no environment variable -- scae_gemm_desc has form,
 * scae_likelihood_bwd_desc has separate, scae_conv3x3_bwd_pair_forms_f32 is new and
 * scae_conv3x3_bwd_pair_{reduce,fold}_f32 take dgrad_forms
 * (4, added since, no signature changed: scae_conv3x3_bwd_pair_tile_f32,
 * scae_conv3x3_wgrad_tile_f32 and scae_conv3x3_wgrad_tile_plan -- the weight gradient's tile
 * form as an argument) */
#define SCAE_ABI_VERSION 4

#define SCAE_OK 0
#define SCAE_ERR_BAD_ARG (-1)      /* null pointer / non-positive size     */
#define SCAE_ERR_UNSUPPORTED (-2)  /* shape outside the kernels' limits    */

/* limits of this build (checked by the launchers) */
#define SCAE_MAX_CHANNELS 4        /* image channels C                     */
#define SCAE_ATTN_MAX_SET 64       /* queries N and keys M per attention   */
#define SCAE_RENDER_MAX_TEMPLATE_ELEMS 4096 /* C*th*tw + th*tw per template */

int scae_abi_version(void);
const char *scae_error_string(int code);

/* Launch lists: a training step as the library's own record of its kernel launches.
 * scae_launch_list_begin(stream) opens a recording and returns its handle (NULL: out of
 * memory).  Until scae_launch_list_end(list) every kernel launch that an entry point of
 * this library SUCCESSFULLY issues on exactly that `stream` (from any host thread --
 * autograd's backward worker launches there too; also into the stream while it is being
 * captured) is appended to the list: kernel, grid, block, LDS bytes, a copy of the argument
 * bytes.  Launches on other streams are not seen, and any number of recordings -- one per
 * stream -- may be open at once: the recording is the only state, and the caller holds it.
 * scae_launch_list_run re-issues the launches, in order, on `stream`: what replaying a
 * captured HIP graph of the same launches does, with a hipLaunchKernel per launch on the
 * host and without the graph's end-of-launch cost on the device.  The list holds pointers,
 * not buffers: the caller keeps every buffer the recorded launches use alive and unmoved.
 * Only this library's kernels are recorded -- a graph captured over the same region may
 * hold other nodes (memsets, another library's kernels); whoever replays a list in place
 * of a graph checks scae_launch_list_size against the graph's node count. */
void *scae_launch_list_begin(void *stream);
int scae_launch_list_end(void *list); /* stops recording; SCAE_ERR_BAD_ARG if not open */
int scae_launch_list_size(const void *list); /* kernel launches recorded */
int scae_launch_list_run(const void *list, void *stream);
void scae_launch_list_free(void *list); /* (also ends a recording that is still open) */
int scae_launch_list_lane(const void *list, int i); /* 0 for launch i, -1 past the end */
/* Diagnostic: one run with a timing event in front of and behind every launch, on `stream`;
 * out_us[2 i], out_us[2 i + 1] = start / end of launch i in microseconds after the first
 * (n_out >= 2 * size).  side_stream: NULL or `stream` (else SCAE_ERR_BAD_ARG).  Synchronises
 * the stream.  A kernel trace serialises the dispatches of a process; this shows the
 * launches as they run in the replayed step. */
int scae_launch_list_timeline(const void *list, void *stream, void *side_stream, float *out_us,
                              int n_out);

/* ------------------------------------------------------------------------
 * Presence-logit noise     replaces torch.rand_like (part_encoder.py:106,
 *     object_decoder.py:201): out[0..n) ~ U[0,1), Philox4x32-10 keyed by
 *     state[0] (seed) and counted by state[1] (launches so far), which the
 *     kernel itself advances -- so a replayed HIP graph draws fresh noise.
 *     state: 3 uint64 of device memory {seed, 0, 0} owned by the caller; one
 *     state per stream of concurrent use.
 * ---------------------------------------------------------------------- */
int scae_uniform_f32(float *out, int64_t n, uint64_t *state, void *stream);

/* ------------------------------------------------------------------------
 * K5  geometric_transform            replaces cv_ops.py:20-76
 *   pose (n,6) -> out (n,6), or (n,9) when as_matrix (third row 0,0,1).
 *   similarity / nonlinear / as_matrix: the reference's three flags.
 * ---------------------------------------------------------------------- */
int scae_geometric_transform_fwd_f32(const float *pose, float *out, int64_t n,
                                     int similarity, int nonlinear,
                                     int as_matrix, void *stream);
/* gout has the forward's output layout; gpose (n,6). */
int scae_geometric_transform_bwd_f32(const float *pose, const float *gout,
                                     float *gpose, int64_t n, int similarity,
                                     int nonlinear, int as_matrix,
                                     void *stream);

/* 3 x 3 products of the hierarchical CapsuleLayer.forward (object_decoder.py:184-191:
 * torch.matmul(cvr.repeat(1, 1, n_votes, 1, 1), cpr)): out[c][v] = left[c] right[c][v]
 *   left (n_caps,3,3)  right (n_caps,V,3,3)  out (n_caps,V,3,3); backward: gleft
 *   (n_caps,3,3) nullable (the parent's transform may be a constant), gright like right. */
int scae_mat3_mul_fwd_f32(const float *left, const float *right, float *out, int64_t n_caps,
                          int V, void *stream);
int scae_mat3_mul_bwd_f32(const float *left, const float *right, const float *gout,
                          float *gleft, float *gright, int64_t n_caps, int V, void *stream);

/* ------------------------------------------------------------------------
 * K2  qkv_attention                  replaces set_transformer.py:24-47
 *   q (HB,N,dk)  k (HB,M,dk)  v (HB,M,dv)  presence (HB,M) nullable
 *   out (HB,N,dv);  probs (HB,N,M) = softmax((q k^T - (1-presence) 1e32) /
 *   sqrt_dk) is written for the backward pass.  QK^T and PV run on the fp32
 *   MFMA (v_mfma_f32_16x16x4_f32).  N, M <= SCAE_ATTN_MAX_SET.
 *   sqrt_dk: the divisor, float(np.sqrt(dk)) in the reference (:43).
 * ---------------------------------------------------------------------- */
int scae_qkv_attention_fwd_f32(const float *q, const float *k, const float *v,
                               const float *presence, float *out, float *probs,
                               int HB, int N, int M, int dk, int dv,
                               float sqrt_dk, void *stream);
/* gq (HB,N,dk) gk (HB,M,dk) gv (HB,M,dv); gpresence (HB,M) nullable. */
/* bf16 forward (BASELINE.json configs[2]): q, k, v, out as bf16 bit patterns
 * (what torch.autocast hands the attention), both contractions on the bf16
 * matrix cores with fp32 accumulation, mask / scale / softmax in fp32; probs
 * (HB,N,M) stays fp32 -- the backward pass is scae_qkv_attention_bwd_f32 on
 * upcast operands. */
int scae_qkv_attention_fwd_bf16(const uint16_t *q, const uint16_t *k, const uint16_t *v,
                                const float *presence, uint16_t *out, float *probs, int HB,
                                int N, int M, int dk, int dv, float sqrt_dk, void *stream);
int scae_qkv_attention_bwd_f32(const float *q, const float *k, const float *v,
                               const float *probs, const float *gout,
                               float *gq, float *gk, float *gv,
                               float *gpresence, int HB, int N, int M, int dk,
                               int dv, float sqrt_dk, void *stream);

/* ------------------------------------------------------------------------
 * K2b  fused set-transformer trunk   replaces set_transformer.py:212-219
 *      (fc1 -> n_layers x SAB(x, x, presence) -> fc2; SAB/MAB :107-142 with
 *      n_heads = 1), forward and backward in one launch each.
 *   input x (B,N,Din) is given as 1..4 column segments (so the caller never
 *   materialises the reference's torch.cat, stacked_capsule_auto_encoder.py
 *   :105-124): segment s holds element (b,n,j) at seg_ptr[s][b*batch_stride +
 *   n*row_stride + j], j < seg_width[s]; sum of widths = Din.
 *   presence (B,N) nullable.  params: ONE packed buffer,
 *     [W1 (D,Din), b1 (D)] + per layer [Wq,bq,Wk,bk,Wv,bv,Wo,bo,
 *     (ln0.weight, ln0.bias), Wf,bf, (ln1.weight, ln1.bias)] + [W2 (Dout,D),
 *     b2 (Dout)], every matrix row-major (out,in) like nn.Linear.weight;
 *     scae_set_encoder_param_count() gives its length.
 *   z (B,N,Dout) = fc2 output; hsave (B,L+1,N,D) workspace kept for backward.
 *   Dout = 0 selects "trunk only": no W2/b2 in params, z (B,N,D) receives the
 *   last block's output (the caller folds fc2 into the output attention, K2c).
 *   Limits: N <= 64, D in {8,16,32}, n_heads = 1.
 *   backward: gz (B,N,Dout) -> seg_grad[s] (B,N,width) contiguous, nullable
 *   per segment; pg_partial (scae_set_encoder_grid(B), P) per-workgroup
 *   parameter gradients in the packed layout (caller sums over dim 0).
 * ---------------------------------------------------------------------- */
int scae_set_encoder_param_count(int D, int Din, int Dout, int L, int layer_norm);
int scae_set_encoder_grid(int B);
/* 1 if the shape fits the kernels (LDS budget of the backward pass), else 0 */
int scae_set_encoder_supported(int N, int D, int Din, int Dout, int L, int layer_norm);
int scae_set_encoder_fwd_f32(int nseg, const float *const *seg_ptr, const int *seg_width,
                             const int *seg_row_stride, const int64_t *seg_batch_stride,
                             const float *presence, const float *params, float *z,
                             float *hsave, int B, int N, int D, int Din, int Dout, int L,
                             int layer_norm, void *stream);
int scae_set_encoder_bwd_f32(int nseg, const float *const *seg_ptr, const int *seg_width,
                             const int *seg_row_stride, const int64_t *seg_batch_stride,
                             float *const *seg_grad, const float *presence,
                             const float *params, const float *hsave, const float *gz,
                             float *pg_partial, int B, int N, int D, int Din, int Dout,
                             int L, int layer_norm, void *stream);
/* BASELINE.json configs[2] ("bf16 ... MFMA attention path"): the same two passes with the
 * attention products of every block -- Q K^T, P V (set_transformer.py:24-47) and, in the
 * backward, dO V^T, dS K, dS^T Q, P^T dO -- on v_mfma_f32_16x16x16_bf16 (operands rounded
 * to bf16, fp32 accumulate); mask / scale / softmax, projections, LayerNorm and the saved
 * activations stay fp32.  scae_set_encoder_bf16_supported: the shapes the matrix-core
 * (one wave per 16-row tile) kernels cover; others return SCAE_ERR_UNSUPPORTED. */
int scae_set_encoder_bf16_supported(int N, int D, int Din, int Dout, int L, int layer_norm);
int scae_set_encoder_fwd_bf16(int nseg, const float *const *seg_ptr, const int *seg_width,
                              const int *seg_row_stride, const int64_t *seg_batch_stride,
                              const float *presence, const float *params, float *z,
                              float *hsave, int B, int N, int D, int Din, int Dout, int L,
                              int layer_norm, void *stream);
int scae_set_encoder_bwd_bf16(int nseg, const float *const *seg_ptr, const int *seg_width,
                              const int *seg_row_stride, const int64_t *seg_batch_stride,
                              float *const *seg_grad, const float *presence,
                              const float *params, const float *hsave, const float *gz,
                              float *pg_partial, int B, int N, int D, int Din, int Dout,
                              int L, int layer_norm, void *stream);

/* ------------------------------------------------------------------------
 * K2c  output attention with folded projections
 *      replaces set_transformer.py:218-223 (fc2 + MultiHeadQKVAttention(seeds,
 *      z, z, presence), n_heads = 1) given the trunk output h (B,N,D):
 *        K' = h wk^T + bk,  V' = h wv^T + bv   (wk = Wk W2 etc., folded by the
 *        caller; bo and the value bias ride inside bv because softmax rows sum
 *        to one),  out = softmax((q K'^T - (1-presence) 1e32)/sqrt(C)) V'
 *   q (O,C) = q_projector(seeds) (batch invariant); wk, wv (C,D); bk, bv (C);
 *   out (B,O,C); probs (B,O,N) nullable (inspection only).
 *   A set is shared out over S = scae_seed_attention_splits(B,O) workgroups
 *   (groups of queries).  backward: gout (B,O,C) -> gh (S,B,N,D), one slab
 *   per query group (caller sums over dim 0); partial
 *   (scae_seed_attention_grid(B,O), O*C + 2*C*D + 2*C) = per-workgroup
 *   [gq | gwk | gbk | gwv | gbv] (caller sums over dim 0).
 *   Limits: N, O <= 64, D in {8,16,32}, C % 8 == 0, LDS.
 * ---------------------------------------------------------------------- */
int scae_seed_attention_splits(int B, int O);
int scae_seed_attention_grid(int B, int O);
int scae_seed_attention_supported(int N, int O, int D, int C);
int scae_seed_attention_fwd_f32(const float *h, const float *q, const float *wk,
                                const float *bk, const float *wv, const float *bv,
                                const float *presence, float *out, float *probs, int B,
                                int N, int O, int D, int C, void *stream);
int scae_seed_attention_bwd_f32(const float *h, const float *q, const float *wk,
                                const float *bk, const float *wv, const float *bv,
                                const float *presence, const float *gout, float *gh,
                                float *partial, int B, int N, int O, int D, int C,
                                void *stream);

/* The same output attention on the matrix cores (seed_attention_wave.hip; D = 16,
 * N, O <= 64, C a multiple of 64), with two more steps of algebra: the logits contract
 * over D through qk = q wk (the q bk term is constant along the keys and drops out of
 * the softmax), and out = (P h) wv^T + bv.  bk is therefore not an input, and its
 * gradient is the exact zero the softmax's shift invariance implies.
 *   fwd : out (B,O,C)
 *   bwd : gh (B,N,16) and, per workgroup, one row of `partial`
 *         (scae_seed_attention_mfma_rows(B), O*16 + C*16 + C) = [d(qk) | dwv | dbv]
 *   reduce: the column sums of `partial`, expanded to the gradients of the operands
 *         of scae_seed_attention_fwd_f32: gq (O,C) = d(qk) wk^T, gwk (C,16) = q^T d(qk),
 *         gbk (C) = 0, gwv (C,16), gbv (C) -- one launch (it replaces the column-sum
 *         launch behind scae_seed_attention_bwd_f32). */
int scae_seed_attention_mfma_supported(int N, int O, int D, int C);
int scae_seed_attention_mfma_rows(int B);
int scae_seed_attention_mfma_fwd_f32(const float *h, const float *q, const float *wk,
                                     const float *wv, const float *bv, const float *presence,
                                     float *out, int B, int N, int O, int C, void *stream);
int scae_seed_attention_mfma_bwd_f32(const float *h, const float *q, const float *wk,
                                     const float *wv, const float *presence, const float *gout,
                                     float *gh, float *partial, int B, int N, int O, int C,
                                     void *stream);
/* BASELINE.json configs[2]: the attention products of the output attention (logits q.wkf h^T,
 * P h; backward dT h^T, dS h, P^T dT + dS^T qk) on v_mfma_f32_16x16x16_bf16, everything else
 * (folded projections, softmax, the C-wide output product) fp32.  Same arguments. */
int scae_seed_attention_mfma_fwd_bf16(const float *h, const float *q, const float *wk,
                                      const float *wv, const float *bv, const float *presence,
                                      float *out, int B, int N, int O, int C, void *stream);
int scae_seed_attention_mfma_bwd_bf16(const float *h, const float *q, const float *wk,
                                      const float *wv, const float *presence,
                                      const float *gout, float *gh, float *partial, int B,
                                      int N, int O, int C, void *stream);
int scae_seed_attention_mfma_reduce_f32(const float *partial, int rows, const float *q,
                                        const float *wk, float *gq, float *gwk, float *gbk,
                                        float *gwv, float *gbv, int O, int C, void *stream);

/* ------------------------------------------------------------------------
 * K2d  batch-invariant weight folding feeding K2c
 *      replaces the per-element fc2 / q,k,v,o projector Linear layers of
 *      set_transformer.py:218-223, :36-75 by parameter-only products:
 *        q   = seeds Wq^T + bq                   (O,C)
 *        wkf = Wk W2,       bkf = Wk b2 + bk     (C,D), (C)
 *        wvf = Wo Wv W2,    bvf = Wo (Wv b2 + bv) + bo
 *      wv2e (C,D+1) = [Wv W2 | Wv b2 + bv] and wowv (C,C) = Wo Wv are kept for the
 *      backward pass.
 *      backward: gradients of (q, wkf, bkf, wvf, bvf) -> gradients of all
 *      eleven parameters; gv2e, t1: unused (the workspaces of an earlier two-launch
 *      form; may be NULL).
 *      Limits: C % 64 == 0, C <= 1024, D in {8,16,32}, O <= 64
 *      (scae_seed_fold_supported).
 * ---------------------------------------------------------------------- */
typedef struct scae_seed_fold_desc {
  const float *seeds;                   /* (O,C) */
  const float *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo; /* (C,C) / (C) */
  const float *w2, *b2;                 /* fc2: (C,D), (C) */
  float *q, *wkf, *bkf, *wvf, *bvf;     /* outputs */
  float *wv2e;                          /* (C,D+1) output kept for backward */
  float *wowv;                          /* (C,C) Wo Wv, kept for backward (NULL: not kept;
                                           scae_seed_fold_bwd_f32 needs it) */
  int O, C, D;
} scae_seed_fold_desc;
typedef struct scae_seed_fold_grads {
  const float *g_q, *g_wkf, *g_bkf, *g_wvf, *g_bvf; /* incoming gradients */
  float *d_seeds, *d_wq, *d_bq, *d_wk, *d_bk, *d_wv, *d_bv, *d_wo, *d_bo, *d_w2, *d_b2;
  float *gv2e, *t1;                     /* unused, may be NULL */
} scae_seed_fold_grads;
int scae_seed_fold_supported(int O, int C, int D);
int scae_seed_fold_fwd_f32(const scae_seed_fold_desc *desc, void *stream);
int scae_seed_fold_bwd_f32(const scae_seed_fold_desc *desc, const scae_seed_fold_grads *grads,
                           void *stream);

/* ------------------------------------------------------------------------
 * LayerNorm over the last dimension      replaces nn.LayerNorm(d) of MAB
 *     (set_transformer.py:114-131) where the blocks run module by module.
 *     x, y, gy, gx: (rows, d); weight / bias (d) nullable; mean, rstd (rows)
 *     saved for the backward; d <= 1024.  bwd: gx (nullable) and, when
 *     `partial` is given, scae_layer_norm_rows(rows) partial rows [gw (d) |
 *     gb (d)] for the caller to sum (scae_sum_rows_f32).
 * ---------------------------------------------------------------------- */
int scae_layer_norm_rows(int64_t rows);
int scae_layer_norm_fwd_f32(const float *x, const float *weight, const float *bias, float *y,
                            float *mean, float *rstd, int64_t rows, int d, float eps,
                            void *stream);
int scae_layer_norm_bwd_f32(const float *x, const float *weight, const float *mean,
                            const float *rstd, const float *gy, float *gx, float *partial,
                            int64_t rows, int d, void *stream);

/* ------------------------------------------------------------------------
 * K7  batched fp32 MFMA GEMM with fused epilogue -- the per-capsule MLPs of
 *     CapsuleLayer (object_decoder.py:86-107, :137-158: a Python loop of 4*O
 *     tiny GEMMs in the reference), forward and backward:
 *       C[g][m][n] = epi( sum_k A[g](m,k) * B[g](n,k) ),   g < batch
 *     A(m,k) = A[g*a_batch + (a_kcontig ? m*lda + k : k*lda + m)], B likewise;
 *     C[g*c_batch + m*ldc + n].  epi: + bias[g*bias_batch + n*bias_ld]
 *     (nullable), ReLU if relu, then zeroed where mask[g*mask_batch +
 *     m*ldmask + n] <= 0 (nullable; the ReLU gate of the backward pass).
 *     asum (nullable, needs a_kcontig == 0): asum[g*asum_batch + m*asum_ld] =
 *     sum_k A[g](m,k), the bias gradient that goes with a weight-gradient GEMM
 *     (asum_ld <= 0 means 1; a stride lets it land in a column of C).
 *     Also serves the 1x1 attention convolution of part_encoder.py:71-73.
 * ---------------------------------------------------------------------- */
int scae_gemm_f32(const float *A, const float *B, float *C, const float *bias,
                  const float *mask, float *asum, int batch, int M, int N, int K,
                  int a_kcontig, int lda, int64_t a_batch, int b_kcontig, int ldb,
                  int64_t b_batch, int ldc, int64_t c_batch, int bias_ld, int64_t bias_batch,
                  int ldmask, int64_t mask_batch, int64_t asum_batch, int asum_ld, int relu,
                  void *stream);

/* Two independent GEMMs of the kind above in ONE launch (e.g. the weight- and
 * the data-gradient GEMM of a layer, which wait for the same incoming
 * gradient and are each too small to fill the device).  Fields as the
 * arguments of scae_gemm_f32. */
typedef struct scae_gemm_desc {
  const float *A, *B;
  float *C;
  const float *bias, *mask;
  float *asum;
  int batch, M, N, K;
  int a_kcontig, lda;
  int64_t a_batch;
  int b_kcontig, ldb;
  int64_t b_batch;
  int ldc;
  int64_t c_batch;
  int bias_ld;
  int64_t bias_batch;
  int ldmask;
  int64_t mask_batch, asum_batch;
  int relu, asum_ld;
  float *c_nomask; /* nullable, layout of C: the values before the mask gate */
  int form;        /* 0 = chosen by the launcher from the shapes (the production setting);
                      SCAE_GEMM_TILES forces the register-staged tiles of gemm_mfma.hip even
                      where the wave-private K-split pipelines (gemm_ksplit.hip) would take the
                      list (tests, measurements); anything else: SCAE_ERR_BAD_ARG */
} scae_gemm_desc;
#define SCAE_GEMM_TILES 1
int scae_gemm_pair_f32(const scae_gemm_desc *first, const scae_gemm_desc *second, void *stream);
/* Up to 4 independent GEMMs of that kind in ONE launch (the four weight-gradient
 * GEMMs of a capsule's MLP chain once the data-gradient chain has run). */
int scae_gemm_multi_f32(const scae_gemm_desc *descs, int n, void *stream);
/* scae_seed_attention_mfma_bwd_{f32,bf16} and scae_gemm_multi_f32(descs, n) in ONE launch
 * (csrc/seed_bwd_gemm.hip): in a training step the output attention's backward and the
 * weight-gradient GEMMs of the capsule MLPs both wait for the MLPs' data-gradient chain
 * only and neither fills the device.  SCAE_ERR_UNSUPPORTED unless the GEMMs take the
 * 32 x 32 split-K tiles (then they fill the device alone: launch them separately). */
int scae_seed_attention_mfma_bwd_gemm_f32(const float *h, const float *q, const float *wk,
                                          const float *wv, const float *presence,
                                          const float *gout, float *gh, float *partial, int B,
                                          int N, int O, int C, const scae_gemm_desc *descs,
                                          int n, void *stream);
int scae_seed_attention_mfma_bwd_gemm_bf16(const float *h, const float *q, const float *wk,
                                           const float *wv, const float *presence,
                                           const float *gout, float *gh, float *partial, int B,
                                           int N, int O, int C, const scae_gemm_desc *descs,
                                           int n, void *stream);
/* ... and scae_set_encoder_bwd_{f32,bf16} in the same launch (csrc/seed_bwd_gemm.hip): the
 * trunk's backward reads of the attention's backward only row b of gh, which the workgroup of
 * set b writes, so each attention workgroup goes on with the trunk's backward of its set --
 * the gradient handed over in registers -- while the GEMM tiles fill the rest of the grid.
 * Arguments: those of scae_seed_attention_mfma_bwd_gemm_* (gh and partial are written as
 * there), then those of scae_set_encoder_bwd_* without gz (trunk_B = B, trunk_N = N; h is the
 * trunk's output z).  Same bits as the two launches.
 * scae_object_encoder_bwd_supported: B <= 512 (one set per workgroup), N, O <= 32, C a
 * multiple of 64, D = 16, Dout = 0 and a trunk on the matrix-core kernels
 * (scae_set_encoder_bf16_supported); otherwise -- or when the GEMMs do not take the 32 x 32
 * split-K tiles -- the launchers return SCAE_ERR_UNSUPPORTED and launch nothing. */
int scae_object_encoder_bwd_supported(int B, int N, int O, int C, int D, int Din, int Dout,
                                      int L, int layer_norm);
int scae_object_encoder_bwd_gemm_f32(
    const float *h, const float *q, const float *wk, const float *wv, const float *presence,
    const float *gout, float *gh, float *partial, int B, int N, int O, int C,
    const scae_gemm_desc *descs, int n, int nseg, const float *const *seg_ptr,
    const int *seg_width, const int *seg_row_stride, const int64_t *seg_batch_stride,
    float *const *seg_grad, const float *trunk_presence, const float *params,
    const float *hsave, float *pg_partial, int trunk_B, int trunk_N, int D, int Din, int Dout,
    int L, int layer_norm, void *stream);
int scae_object_encoder_bwd_gemm_bf16(
    const float *h, const float *q, const float *wk, const float *wv, const float *presence,
    const float *gout, float *gh, float *partial, int B, int N, int O, int C,
    const scae_gemm_desc *descs, int n, int nseg, const float *const *seg_ptr,
    const int *seg_width, const int *seg_row_stride, const int64_t *seg_batch_stride,
    float *const *seg_grad, const float *trunk_presence, const float *params,
    const float *hsave, float *pg_partial, int trunk_B, int trunk_N, int D, int Din, int Dout,
    int L, int layer_norm, void *stream);


/* ------------------------------------------------------------------------
 * K7b a chain of up to 4 per-group layers in ONE launch -- the two ReLU MLPs
 *     CapsuleLayer runs back to back per object capsule (object_decoder.py:
 *     86-107 `mlps`, :137-158 `caps_mlps`, the `cat([.., caps_exist])` of :149
 *     between them as an implicit ones column), forward and the data-gradient
 *     half of their backward.  A workgroup carries 16 batch rows of one group
 *     through all layers (activations in LDS, weights as MFMA fragments from L2).
 *     in: element (b, g, k) at in[g*in_gs + b*in_bs + k], k < in_dim.
 *   fwd: layer i: y = x W_i^T (W_i rows = N outputs, K = width of x, row
 *     stride ldw, group stride w_gs) + bias[g*bias_gs + n*bias_ld] (nullable),
 *     ReLU if relu; stored (nullable except for the last layer) at
 *     out[g*out_gs + b*out_bs + n].
 *   bwd: layer i: y = x W_i (W_i rows = the K contraction entries, N columns
 *     used), zeroed where gate[g*gate_gs + b*gate_bs + n] <= 0 (nullable);
 *     out as above.  Pass the layers in backward order; x of the first = the
 *     gradient w.r.t. the last pre-activation.
 *     Each layer's K must equal its predecessor's N (in_dim for the first);
 *     widths <= scae_mlp_chain_max_width().
 * ---------------------------------------------------------------------- */
typedef struct scae_mlp_chain_layer {
  const float *w;
  int64_t w_gs;
  int ldw, K, N;
  const float *bias;
  int64_t bias_gs;
  int bias_ld;
  const float *gate;
  int64_t gate_gs, gate_bs;
  float *out;
  int64_t out_gs, out_bs;
  int relu;
} scae_mlp_chain_layer;
typedef struct scae_mlp_chain_desc {
  scae_mlp_chain_layer layer[4];
  int n_layers;
  const float *in;
  int64_t in_gs, in_bs;
  int in_dim, B, G;
  int row_tile; /* batch rows per workgroup: 0 = chosen by the launcher from the shape
                   (the production setting); 16 | 32 force one (tests, measurements) */
  int bf16;     /* != 0: the layer products on v_mfma_f32_16x16x16_bf16 -- both operands rounded
                   to bf16 (nearest even) on their way into the matrix core, fp32 accumulate,
                   fp32 tensors in memory, epilogues unchanged (BASELINE.json configs[2]) */
} scae_mlp_chain_desc;
int scae_mlp_chain_max_width(void);
int scae_mlp_chain_fwd_f32(const scae_mlp_chain_desc *desc, void *stream);
int scae_mlp_chain_bwd_f32(const scae_mlp_chain_desc *desc, void *stream);

/* The chain with the vote kernel (K3, scae_capsule_votes_*_f32 below) riding in
 * the same launch: CapsuleLayer.forward (object_decoder.py:120-236) from the
 * object encoding to the votes as ONE launch, and the first half of its backward
 * (vote gradients -> parameter-row gradients -> the data-gradient chain) as one.
 *   fwd: the last layer's output rows (B, G, ld_param), N = 8V+7, are the vote
 *     kernel's all_param; outputs as scae_capsule_votes_fwd_f32.
 *   bwd: desc->in is ignored -- the chain's input block is the vote kernel's
 *     gall_param_gated (or gall_param when that is NULL), computed in the launch
 *     from the vote gradients and also written out (the weight-gradient GEMM of
 *     the last layer and the bias sums read them); all_param = the saved rows.
 * Fields as the arguments of scae_capsule_votes_fwd/bwd_f32; B and O are the
 * chain's B and G. */
typedef struct scae_votes_desc {
  const float *all_param; /* bwd only */
  const float *cpr_static, *bias_cvr, *bias_caps, *bias_vote, *bias_scale;
  const float *noise_caps, *noise_vote; /* nullable */
  float noise_scale;
  int V, ld_param, similarity, learn_vote_scale, allow_deformations;
  /* forward outputs */
  float *vote, *scale, *vote_presence, *logit_caps, *logit_vote, *reg_partial;
  float *caps_presence; /* nullable together with caps_arg */
  int *caps_arg;
  /* backward: incoming gradients (nullable), outputs */
  const float *gvote, *gscale, *gvote_presence, *glogit_caps, *glogit_vote, *greg;
  const float *gcaps_presence;
  float *gall_param, *gcpr_in, *gall_param_gated;
} scae_votes_desc;
int scae_mlp_chain_votes_fwd_f32(const scae_mlp_chain_desc *desc, const scae_votes_desc *votes,
                                 void *stream);
int scae_mlp_chain_votes_bwd_f32(const scae_mlp_chain_desc *desc, const scae_votes_desc *votes,
                                 void *stream);
/* The form the launchers above take for these descriptors (`votes` nullable: the plain
 * chain; bwd != 0: the backward launchers); launches nothing.  rows: batch rows per
 * workgroup, 16 | 32; narrow: each LDS activation buffer is as wide as what it holds, not
 * both as wide as the widest layer; scratch_in_weights: the vote blocks take their LDS
 * scratch in the weight tiles, not in an activation buffer. */
typedef struct scae_mlp_chain_form {
  int rows, narrow, scratch_in_weights;
} scae_mlp_chain_form;
int scae_mlp_chain_get_form(const scae_mlp_chain_desc *desc, const scae_votes_desc *votes, int bwd,
                            scae_mlp_chain_form *form);

/* bf16-operand forms of the GEMM-shaped launchers (BASELINE.json configs[2], "bs=1024
 * bf16"): same arguments, same fp32 tensors in memory; the operands are rounded to bf16
 * (nearest even) on their way into LDS and multiplied on v_mfma_f32_32x32x16_bf16 with fp32
 * accumulation, in 128 x 128 tiles.  Problems too small for those tiles (a side shorter
 * than 32; convolutions whose channel counts are not multiples of 128 or that have too few
 * pixels to fill the device) run the fp32 kernels unchanged.  Epilogues (bias, ReLU,
 * gates, column sums -- those of the values as they arrive, rounded) are identical. */
int scae_gemm_bf16(const float *A, const float *B, float *C, const float *bias,
                   const float *mask, float *asum, int batch, int M, int N, int K,
                   int a_kcontig, int lda, int64_t a_batch, int b_kcontig, int ldb,
                   int64_t b_batch, int ldc, int64_t c_batch, int bias_ld, int64_t bias_batch,
                   int ldmask, int64_t mask_batch, int64_t asum_batch, int asum_ld, int relu,
                   void *stream);
int scae_gemm_pair_bf16(const scae_gemm_desc *first, const scae_gemm_desc *second, void *stream);
/* scae_gemm_multi_f32 on the bf16 tiles when every problem has both sides >= 32 (else the
 * fp32 tiles, unchanged) */
int scae_gemm_multi_bf16(const scae_gemm_desc *descs, int n, void *stream);
/* scae_conv3x3_fwd_f32 (the 32 x 64 second-generation tiles: Cin % 32 == 0, Cout % 64 == 0)
 * with the workgroups of scae_seed_fold_fwd_f32(fold) as the tail of its grid: in a training
 * step the parameter-only folding products hide behind an early, large launch instead of
 * lengthening the prologue.  SCAE_ERR_UNSUPPORTED: launch the two separately. */
int scae_conv3x3_fwd_fold_f32(const float *in, const float *wf, const float *bias, float *out,
                              const float *post_bias, float *out_post, int B, int IH, int IW,
                              int Cin, int Cout, int stride, const scae_seed_fold_desc *fold,
                              void *stream);
/* K8r: the forward with the input images resident in LDS (csrc/conv_resident.hip), for the
 * small layers of the encoder: a workgroup owns `group` images x 32 or 64 output channels, stages
 * their input pixels once as three bf16 planes (6 bytes per element), reads the filter from its
 * fragment-major copy `wp` (see relayout) straight into MFMA fragments.  Same contract as
 * scae_conv3x3_fwd_f32 otherwise (results agree to fp32 round-off: the K sum is split by
 * input-channel block).  Cin % 128 == 0, Cout % 32 == 0, the group's planes <= 80 KiB of LDS
 * (two workgroups per CU; a forced group: 150 KiB): scae_conv3x3_fwd_res_supported, else
 * SCAE_ERR_UNSUPPORTED.  group: 0 = by shape; > 0 forces a group size (tests). */
int scae_conv3x3_fwd_res_supported(int B, int IH, int IW, int Cin, int Cout, int stride);
int scae_conv3x3_fwd_res_f32(const float *in, const float *wp, const float *bias, float *out,
                             const float *post_bias, float *out_post, int B, int IH, int IW,
                             int Cin, int Cout, int stride, int group, void *stream);
int scae_conv3x3_fwd_bf16(const float *in, const float *wf, const float *bias, float *out,
                          const float *post_bias, float *out_post, int B, int IH, int IW, int Cin,
                          int Cout, int stride, void *stream);
int scae_conv3x3_bwd_pair_bf16(const float *dpre, const float *wd, const float *in, float *din,
                               float *partial, int B, int IH, int IW, int Cin, int Cout,
                               int stride, void *stream);

/* ------------------------------------------------------------------------
 * K8  3x3 "valid" convolutions of the CNN encoder as implicit GEMMs on the
 *     fp32 matrix cores      replaces part_encoder.py:26-44 / nn_ext.py:34-59
 *     (Conv2d(k=3, stride, padding=0) + ReLU) and their autograd backward.
 *   Activations NHWC: in (B,IH,IW,Cin) -> out (B,OH,OW,Cout), OH=(IH-3)/s+1.
 *   relayout: w (Cout,Cin,3,3) -> wf, wd (Cin,9,Cout).  `wf` holds scae_conv3x3_wf_floats(Cout,Cin)
 *     floats: the (Cout,9,Cin) layout the tile kernels read (`wf` of fwd / fwd_fold: a caller may
 *     fill that block by hand), followed -- when Cin, Cout % 32 == 0 -- by the fragment-major copy
 *     `wp` = wf + Cout*9*Cin of the image-resident forward (fwd_res): the filter split into the
 *     three bf16 planes of its exact fp32 products (csrc/bf16x6.h), 1.5 * Cout*9*Cin floats.
 *   first_*: direct kernels for the image layer (NCHW image, small Cin; w in
 *     the reference layout, Cout % 64 == 0); first_wgrad writes
 *     scae_conv3x3_first_wgrad_rows(B,Cout) partial rows, each
 *     [dW (Cout,Cin*9) | db (Cout)], for the caller to sum over the rows.
 *   fwd:   out = relu(conv(in, wf) + bias)        Cin, Cout % 64 == 0, s <= 2
 *          out_post (nullable, NHWC like out) = out + post_bias, post_bias
 *          (Cout,OH,OW) = img_embedding_bias of part_encoder.py:87 (the sum
 *          the 1x1 attention convolution reads)
 *   dgrad: din = conv^T(dpre, wd), zeroed where gate <= 0 (gate (B,IH,IW,Cin)
 *          = the producing layer's ReLU output, nullable)
 *   wgrad: dw (Cout,Cin,3,3) = sum_pixels dpre x in and (db nullable) db (Cout)
 *          = sum_pixels dpre; partial is a workspace of
 *          scae_conv3x3_wgrad_splits(B,OH,OW,Cin,Cout) * (9*Cout*Cin + Cout) floats.
 *          dw == NULL leaves the partials unreduced; wgrad_reduce_batch then
 *          reduces the partials of up to 8 layers in one launch (HOST arrays).
 * ---------------------------------------------------------------------- */
/* floats a `wf` buffer of relayout / relayout_batch / first_fwd_relayout / the step prologue
 * must hold for a (Cout, Cin) layer: Cout*9*Cin, x 2.5 when the packed copy is written */
int64_t scae_conv3x3_wf_floats(int Cout, int Cin);
int scae_conv3x3_relayout_f32(const float *w, float *wf, float *wd, int Cout, int Cin,
                              void *stream);

/* K8 with bf16-RESIDENT operands (BASELINE configs[2]; csrc/conv_bf16.hip): the same three
 * passes of part_encoder.py:26-44 / nn_ext.py:34-59 with every GEMM operand stored as bf16
 * (uint16_t bit patterns, round-to-nearest-even of the fp32 values) -- NHWC activations,
 * pre-activation gradients, the re-laid-out filters wf (Cout,9,Cin) / wd (Cin,9,Cout) --
 * multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Cin, Cout % 128 == 0,
 * stride 1 or 2, tensors below 2 GiB (scae_conv3x3_bf16r_supported).
 *   cvt_bf16_batch: dst[a][0..n[a]) = bf16(src[a]) for up to 8 arrays (n[a] % 8 == 0) in one
 *     launch; the three arrays are HOST arrays.
 *   fwd:   out_h (bf16) = relu(conv(in, wf) + bias); out_f (nullable, fp32): the same values
 *          unrounded; out_post (nullable, fp32) = relu(.) + post_bias (Cout,OH,OW).
 *   dgrad: din = conv^T(dpre, wd), zeroed where gate <= 0 (gate: bf16 (B,IH,IW,Cin),
 *          nullable), written as bf16 (din_h) and / or fp32 (din_f).
 *   wgrad: partial = scae_conv3x3_wgrad_bf16r_splits(..) x (9*Cout*Cin + Cout) fp32 partials
 *          in the layout of scae_conv3x3_wgrad_f32's (dw == NULL): the fp32 reduction
 *          launches (wgrad_reduce_batch, first_wgrad_reduce) sum them. */
int scae_conv3x3_bf16r_supported(int B, int IH, int IW, int Cin, int Cout, int stride);
/* scae_conv3x3_first_fwd_relayout_f32 for the bf16-resident encoder: the image layer's output
 * as bf16 (out_h), the re-laid-out filters as fp32 (rwf / rwd, as there) AND as bf16 (rwfh / rwdh) */
int scae_conv3x3_first_fwd_relayout_bf16(const float *img, const float *w, const float *bias,
                                         uint16_t *out_h, int B, int Cin, int IH, int IW,
                                         int Cout, int stride, int n_layers,
                                         const float *const *rw, float *const *rwf,
                                         float *const *rwd, uint16_t *const *rwfh,
                                         uint16_t *const *rwdh, const int *rCout,
                                         const int *rCin, void *stream);
int scae_cvt_bf16_batch(int n_arrays, const float *const *src, uint16_t *const *dst,
                        const int64_t *n, void *stream);
int scae_conv3x3_fwd_bf16r(const uint16_t *in, const uint16_t *wf, const float *bias,
                           uint16_t *out_h, float *out_f, const float *post_bias,
                           float *out_post, int B, int IH, int IW, int Cin, int Cout, int stride,
                           void *stream);
int scae_conv3x3_dgrad_bf16r(const uint16_t *dpre, const uint16_t *wd, const uint16_t *gate,
                             uint16_t *din_h, float *din_f, int B, int IH, int IW, int Cin,
                             int Cout, int stride, void *stream);
int scae_conv3x3_wgrad_bf16r_splits(int B, int OH, int OW, int Cin, int Cout);
int scae_conv3x3_wgrad_bf16r(const uint16_t *dpre, const uint16_t *x, float *partial, int B,
                             int IH, int IW, int Cin, int Cout, int stride, void *stream);
/* the same for n_layers <= 8 layers in one launch; the five arrays are HOST arrays */
int scae_conv3x3_relayout_batch_f32(int n_layers, const float *const *w, float *const *wf,
                                    float *const *wd, const int *Cout, const int *Cin,
                                    void *stream);
int scae_conv3x3_first_fwd_f32(const float *img, const float *w, const float *bias,
                               float *out, int B, int Cin, int IH, int IW, int Cout,
                               int stride, void *stream);
int scae_conv3x3_first_wgrad_rows(int B, int Cout);
int scae_conv3x3_first_wgrad_f32(const float *dpre, const float *img, float *partial, int B,
                                 int Cin, int IH, int IW, int Cout, int stride, void *stream);
/* first_fwd / first_wgrad with riders: the parameter-only filter re-layouts of the
 * following n_layers layers (arguments of scae_conv3x3_relayout_batch_f32), resp.
 * the split reductions of their weight-gradient partials (arguments of
 * scae_conv3x3_wgrad_reduce_batch_f32), run as extra workgroups of the same
 * launch -- they are independent of the image layer.  n_layers = 0: no riders. */
int scae_conv3x3_first_fwd_relayout_f32(const float *img, const float *w, const float *bias,
                                        float *out, int B, int Cin, int IH, int IW, int Cout,
                                        int stride, int n_layers, const float *const *rw,
                                        float *const *rwf, float *const *rwd, const int *rCout,
                                        const int *rCin, void *stream);
int scae_conv3x3_first_wgrad_reduce_f32(const float *dpre, const float *img, float *partial,
                                        int B, int Cin, int IH, int IW, int Cout, int stride,
                                        int n_layers, const float *const *rpartial,
                                        float *const *rdw, float *const *rdb, const int *rCout,
                                        const int *rCin, const int *rsplits, void *stream);
int scae_conv3x3_fwd_f32(const float *in, const float *wf, const float *bias, float *out,
                         const float *post_bias, float *out_post, int B, int IH, int IW,
                         int Cin, int Cout, int stride, void *stream);
int scae_conv3x3_dgrad_f32(const float *dpre, const float *wd, const float *gate, float *din,
                           int B, int IH, int IW, int Cin, int Cout, int stride, void *stream);
/* dgrad (gated by `in`, the layer's input = the producing layer's ReLU output)
 * and the weight-gradient partials (as scae_conv3x3_wgrad_f32 with dw == NULL)
 * of one layer in ONE launch: both only wait for dpre. */
int scae_conv3x3_bwd_pair_f32(const float *dpre, const float *wd, const float *in, float *din,
                              float *partial, int B, int IH, int IW, int Cin, int Cout,
                              int stride, void *stream);
/* ... with the data gradient's tile form chosen by the caller (tests, measurements).
 * dgrad_forms is a set of the bits below; SCAE_DGRAD_BY_SHAPE is the production setting and
 * what scae_conv3x3_bwd_pair_f32, _bf16 and scae_conv3x3_dgrad_f32 use.  SCAE_DGRAD_TILE with
 * SCAE_DGRAD_NO_TILE, or any other bit: SCAE_ERR_BAD_ARG. */
#define SCAE_DGRAD_BY_SHAPE 0
#define SCAE_DGRAD_NO_TILE 1   /* never the DMA-fed 64 x 128 tile                        */
#define SCAE_DGRAD_NO_KSPLIT 2 /* never the K-split tile                                 */
#define SCAE_DGRAD_TILE 4      /* the DMA-fed tile wherever its shape limits hold,
                                  whatever the tile count                                */
int scae_conv3x3_bwd_pair_forms_f32(const float *dpre, const float *wd, const float *in,
                                    float *din, float *partial, int B, int IH, int IW, int Cin,
                                    int Cout, int stride, int dgrad_forms, void *stream);
/* scae_conv3x3_bwd_pair_f32 with the workgroups of scae_seed_fold_bwd_f32(fold, fold_grads) as
 * the head of its grid: the folding products' backward writes parameter gradients only, so in
 * a training step it may wait for this launch (256-thread workgroups, tens of microseconds
 * of MFMA tiles to hide behind).  Same results, bit for bit, as the launch of its own.
 * scae_conv3x3_bwd_pair_reduce_f32: the same for scae_seed_attention_mfma_reduce_f32
 * (arguments rpartial .. C), whose outputs only the folding products' backward reads.
 * SCAE_ERR_UNSUPPORTED (folding width != 256, another tile form of the pair): launch both.
 * dgrad_forms: as for scae_conv3x3_bwd_pair_forms_f32 (0 in production; tests, measurements). */
int scae_conv3x3_bwd_pair_reduce_f32(const float *dpre, const float *wd, const float *in,
                                     float *din, float *partial, int B, int IH, int IW, int Cin,
                                     int Cout, int stride, const float *rpartial, int rows,
                                     const float *q, const float *wk, float *gq, float *gwk,
                                     float *gbk, float *gwv, float *gbv, int O, int C,
                                     int dgrad_forms, void *stream);
int scae_conv3x3_bwd_pair_fold_f32(const float *dpre, const float *wd, const float *in,
                                   float *din, float *partial, int B, int IH, int IW, int Cin,
                                   int Cout, int stride, const scae_seed_fold_desc *fold,
                                   const scae_seed_fold_grads *fold_grads, int dgrad_forms,
                                   void *stream);
int scae_conv3x3_wgrad_splits(int B, int OH, int OW, int Cin, int Cout);
int scae_conv3x3_wgrad_f32(const float *dpre, const float *in, float *partial, float *dw,
                           float *db, int B, int IH, int IW, int Cin, int Cout, int stride,
                           void *stream);
int scae_conv3x3_wgrad_reduce_batch_f32(int n_layers, const float *const *partial,
                                        float *const *dw, float *const *db, const int *Cout,
                                        const int *Cin, const int *splits, void *stream);
/* The weight gradient's tile form chosen by the caller (tests, measurements): output x input
 * channels of one workgroup's tile, plus SCAE_WGRAD_HEAD for a pair launch whose
 * weight-gradient workgroups lead the grid instead of following the data gradient's.  Every
 * form runs on the splits of scae_conv3x3_wgrad_splits and writes the same partial slabs bit
 * for bit; 128 x 64 with output channels that 128 does not divide falls back to 64 x 64.
 * SCAE_WGRAD_TILE_BY_SHAPE is the production setting: what the entry points without this
 * argument use, the pair launches with a rider among them, and what
 * scae_conv3x3_wgrad_tile_plan returns for a layer's pair launch under dgrad_forms (a shape
 * code, + SCAE_WGRAD_HEAD; or a negative SCAE_ERR_*).  Anything else: SCAE_ERR_BAD_ARG.
 * These two are not launchers of a training step: the selector follows the stream, and the
 * binding's launch recorder, which takes a launcher's last argument for its stream, leaves
 * them alone. */
#define SCAE_WGRAD_TILE_BY_SHAPE 0
#define SCAE_WGRAD_TILE_64x64 1
#define SCAE_WGRAD_TILE_128x64 2
#define SCAE_WGRAD_HEAD 64
int scae_conv3x3_bwd_pair_tile_f32(const float *dpre, const float *wd, const float *in,
                                   float *din, float *partial, int B, int IH, int IW, int Cin,
                                   int Cout, int stride, int dgrad_forms, void *stream,
                                   int wgrad_tile);
int scae_conv3x3_wgrad_tile_f32(const float *dpre, const float *in, float *partial, float *dw,
                                float *db, int B, int IH, int IW, int Cin, int Cout, int stride,
                                void *stream, int wgrad_tile);
int scae_conv3x3_wgrad_tile_plan(int B, int IH, int IW, int Cin, int Cout, int stride,
                                 int dgrad_forms);

/* ------------------------------------------------------------------------
 * K9  attention pooling of the part-capsule head
 *     replaces nn_ext.py:76-101 (multiple_soft_attention +
 *     multiple_attention_pooling_2d) as used by part_encoder.py:74.
 *   y (B,HW,A*P): NHWC output of the 1x1 attention conv (K7 GEMM); per capsule
 *   a the channels a*P .. a*P+P-2 are features, a*P+P-1 the attention logit.
 *   out (B,A,P-1) = sum_pix y[pix][a*P+p] * softmax_pix(logit)[pix]
 *   backward: g (B,A,P-1) -> dy (B,HW,A*P).
 * ---------------------------------------------------------------------- */
int scae_attention_pool_supported(int HW, int A, int P);
/* Host only: the capsule groups per image every K9 launcher below splits (B, A) into -- one
 * workgroup per (image, group of A / groups capsules); 0 for B or A <= 0.  (K10's:
 * scae_template_color_partial_rows(B, M) / B.) */
int scae_attention_pool_groups(int B, int A);
int scae_attention_pool_fwd_f32(const float *y, float *out, int B, int HW, int A, int P,
                                void *stream);
int scae_attention_pool_bwd_f32(const float *y, const float *g, float *dy, int B, int HW,
                                int A, int P, void *stream);
/* The same pooling with the rest of CapsuleImageEncoder.forward fused behind it
 * (part_encoder.py:75-92, n_poses = 6): the pooled row of capsule a is
 * [pose (6) | presence logit | special features (P-8)];
 *   pose (B,A,6)   = geometric_transform(pooled[..., :6], similarity) (K5 math)
 *   presence (B,A) = sigmoid(pooled[..., 6] + (noise_u - .5) * noise_scale)
 *   feature (B,A,P-8) (nullable when P == 8); noise_u (B,A) U[0,1) or NULL;
 *   absence (B,A) = 1 - presence (nullable; the set-transformer input of
 *   stacked_capsule_auto_encoder.py:113);
 *   pooled (B,A,P-1) is kept for the backward pass, whose incoming gradients
 *   g_pose / g_presence / g_feature may each be NULL (= zeros); g_feature2
 *   (nullable) is added to g_feature -- the feature feeds both the template
 *   colours and the set transformer (stacked_capsule_auto_encoder.py:103,:119),
 *   and summing here saves the caller an accumulate launch. */
int scae_capsule_head_fwd_f32(const float *y, const float *noise_u, float noise_scale,
                              int similarity, float *pooled, float *pose, float *presence,
                              float *feature, float *absence, int B, int HW, int A, int P,
                              void *stream);
/* The 1x1 attention conv (part_encoder.py:70-73) fused into the head's forward:
 * y (B,HW,A*P) = x (B,HW,C) w^T (A*P,C) + bias is computed slab by slab inside the
 * pooling workgroups (fp32 MFMA) and written to y for the backward; everything else
 * as scae_capsule_head_fwd_f32.  Supported for HW <= 32 and C a multiple of 64
 * and at most 256
 * (scae_capsule_head_conv_supported); x and w 16-byte aligned. */
int scae_capsule_head_conv_supported(int HW, int A, int P, int C);
/* ... and faster than GEMM + scae_capsule_head_fwd_f32: the fused form re-reads the
 * weights per image, so it pays for small batches only (see attention_pool.hip). */
int scae_capsule_head_conv_preferred(int B, int HW, int A, int P, int C);
int scae_capsule_head_conv_fwd_f32(const float *x, const float *w, const float *bias, int C,
                                   float *y, const float *noise_u, float noise_scale,
                                   int similarity, float *pooled, float *pose, float *presence,
                                   float *feature, float *absence, int B, int HW, int A, int P,
                                   void *stream);
/* scae_capsule_head_conv_fwd_f32 with scae_template_color_fwd_f32 (TemplateGenerator.forward,
 * part_decoder.py:78-110; arguments logits .. color_nonlin, M = A, its `feature` input is
 * this launch's `feature` output) behind it, workgroup by workgroup: the colour MLP of an
 * (image, capsule group) needs the special features of its own capsules only.
 * SCAE_ERR_UNSUPPORTED (F != P - 8, different grouping, one group per image): launch the two
 * in turn. */
int scae_capsule_head_conv_fwd_tc_f32(
    const float *x, const float *w, const float *bias, int C, float *y, const float *noise_u,
    float noise_scale, int similarity, float *pooled, float *pose, float *presence,
    float *feature, float *absence, int B, int HW, int A, int P, const float *logits,
    const float *w1, const float *b1, const float *w2, const float *b2, float *raw,
    float *templates, float *color, int Ct, int hw, int F, int H1, int template_nonlin,
    int color_nonlin, void *stream);
int scae_capsule_head_bwd_f32(const float *y, const float *pooled, const float *noise_u,
                              float noise_scale, int similarity, const float *g_pose,
                              const float *g_presence, const float *g_feature,
                              const float *g_feature2, float *dy, int B, int HW, int A, int P,
                              void *stream);
/* scae_capsule_head_bwd_f32 with scae_template_color_bwd_f32 (arguments logits ..
 * color_nonlin, M = A; tc_g_feature is both that kernel's g_feature output and this one's
 * g_feature2) in front of it, workgroup by workgroup: both run one workgroup per (image,
 * capsule group) over the same groups, and the head only needs the colour MLP's feature
 * gradient of its own capsules.  SCAE_ERR_UNSUPPORTED (F != P - 8, different grouping):
 * launch the two in turn. */
int scae_capsule_head_bwd_tc_f32(
    const float *y, const float *pooled, const float *noise_u, float noise_scale, int similarity,
    const float *g_pose, const float *g_presence, const float *g_feature, float *dy, int B,
    int HW, int A, int P, const float *logits, const float *feature, const float *w1,
    const float *b1, const float *w2, const float *b2, const float *color,
    const float *g_templates, const float *g_raw, float *g_logits, float *tc_g_feature,
    float *partial, int C, int hw, int F, int H1, int template_nonlin, int color_nonlin,
    void *stream);

/* ------------------------------------------------------------------------
 * Optimiser step on the flat parameter buffer
 *     replaces torch.optim.RMSprop(lr, momentum, eps) of
 *     base_experiment.py:44-77 (alpha = 0.99, weight_decay = 0, not centered):
 *       v <- alpha v + (1-alpha) g^2;  buf <- momentum buf + g/(sqrt(v)+eps);
 *       p <- p - lr buf        (momentum == 0: p <- p - lr g/(sqrt(v)+eps),
 *       buf may be NULL); g <- grad_scale * g + weight_decay p first (grad_scale:
 *       e.g. 1/world_size after a SUM all-reduce).  lr_dev (nullable):
 *       the learning rate in device memory, read instead of `lr` -- lets the
 *       per-epoch ExponentialLR schedule (:73-76) change it under graph replay.
 *       All buffers n floats, at the same offset within a 16-byte line
 *       (slices of identically laid out flat buffers).
 * ---------------------------------------------------------------------- */
int scae_rmsprop_step_f32(float *param, const float *grad, float *square_avg, float *buf,
                          int64_t n, float lr, const float *lr_dev, float alpha, float eps,
                          float momentum, float weight_decay, float grad_scale, void *stream);

/* A training step's last column sums (scae_sum_rows_multi_f32 over `jobs`, whose destinations
 * are parameter-gradient slots of `grad`) and the RMSprop pass above as ONE launch: the sum
 * workgroups apply the update of the elements they produce, the streaming workgroups skip
 * them; bit for bit the two launches' results.  No weight decay in this form. */
struct scae_sum_job;
int scae_rmsprop_sums_step_f32(float *param, float *grad, float *square_avg, float *buf,
                               int64_t n, float lr, const float *lr_dev, float alpha, float eps,
                               float momentum, float grad_scale, const struct scae_sum_job *jobs,
                               int n_jobs, void *stream);

/* Adam / RAdam / RMSprop step on the flat parameter buffers, LookAhead optionally fused in
 *     replaces the reference's other two optimiser choices (base_experiment.py:44-77) and its
 *     LookAhead wrapper over any of the three:
 *     kind 0 = torch.optim.Adam(lr, betas, eps, weight_decay) (coupled L2: g <- g + wd p):
 *       m <- m + (1-b1)(g-m);  v <- b2 v + (1-b2) g^2;
 *       p <- p - lr/(1-b1^t) m / (sqrt(v)/sqrt(1-b2^t) + eps)
 *     kind 1 = RAdam of torch_scae/optimizers.py:36-102 (degenerated_to_sgd; decoupled decay
 *       p <- p - wd lr p first): the same moments (m <- b1 m + (1-b1) g); with
 *       N_sma = N_max - 2t b2^t/(1-b2^t), N_max = 2/(1-b2) - 1: N_sma >= 5:
 *       p <- p - lr rect(t) sqrt(1-b2^t)/(1-b1^t) m/(sqrt(v) + eps), else p <- p - lr/(1-b1^t) m.
 *     kind 2 = the RMSprop of scae_rmsprop_step_f32, bit for bit, with beta1 = momentum,
 *       beta2 = alpha, exp_avg = its momentum buffer, exp_avg_sq = square_avg (the form that
 *       carries a step count: for LookAhead).
 *     look_ahead_k > 0: LookAhead(k, alpha) of optimizers.py:105-190 after the update on every
 *       step t with t % k == 0: the first such step sets slow := p (p unchanged), every later
 *       one slow <- slow + alpha (p - slow), p := slow.  `slow` is read and written on those
 *       steps only (may be NULL with look_ahead_k == 0).
 *     g <- grad_scale g first.  The learning rate is read from lr_dev (device memory: the
 *     per-epoch ExponentialLR of :73-76 under replay).  step_state: SCAE_FLAT_OPT_STATE_INTS
 *     device ints -- [0] the steps taken so far (t - 1 of this step), [1] the slow buffer has
 *     been made, the rest arrival counters that must be 0 (zeroed once; every launch leaves
 *     them so).  The step's scalars come from
 *     [0] in fp64, and with `advance` set the launch's last workgroup writes [0] + 1 (and
 *     [1] = 1 on a sync step): one launch per optimiser step may advance, the last one when a
 *     step is issued as several launches over parameter ranges.  Betas are doubles: their
 *     powers are taken in fp64 (by repeated squaring), as torch takes them.  All buffers n floats, at the same offset
 *     within a 16-byte line. */
#define SCAE_FLAT_OPT_STATE_INTS 2112
int scae_flat_opt_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                           float *slow, int64_t n, const float *lr_dev, int32_t *step_state,
                           int kind, double beta1, double beta2, float eps, float weight_decay,
                           float grad_scale, int look_ahead_k, float look_ahead_alpha,
                           int advance, void *stream);

/* The step's last column sums riding in the launch above, as scae_rmsprop_sums_step_f32 does
 * for plain RMSprop: bit for bit scae_sum_rows_multi_f32 followed by
 * scae_flat_opt_step_f32(..., advance = 1).  No weight decay in this form. */
int scae_flat_opt_sums_step_f32(float *param, float *grad, float *exp_avg, float *exp_avg_sq,
                                float *slow, int64_t n, const float *lr_dev,
                                int32_t *step_state, int kind, double beta1, double beta2,
                                float eps, float grad_scale, int look_ahead_k,
                                float look_ahead_alpha, const struct scae_sum_job *jobs,
                                int n_jobs, void *stream);

/* Gradient clipping by global norm -- torch.nn.utils.clip_grad_norm_(params, max_norm), which
 * Lightning's Trainer(gradient_clip_val) applies between backward and the optimiser step:
 *   total = || g ||_2 over every parameter gradient,  coef = min(1, max_norm / (total + 1e-6)),
 *   g <- coef g.
 * In two launches: scae_grad_sq_partials_f32 writes *n_partials (<= max_partials; a function
 * of n -- and of the jobs -- only) fp64 partial sums of g^2 over the n floats of `grad` (any
 * 4-byte aligned start) into `partials`; the clip forms of the optimiser passes below reduce
 * them in every workgroup in one fixed order (fp64), form total = grad_scale sqrt(sum) and
 * coef in fp32 and apply g <- coef (grad_scale g) before the weight decay.  No atomics: the
 * same inputs give the same bits.  With coef == 1 (max_norm above the norm) the clip forms
 * equal the plain passes bit for bit. */
#define SCAE_GRAD_SQ_MAX_PARTIALS 4096
int scae_grad_sq_partials_f32(const float *grad, int64_t n, double *partials, int max_partials,
                              int *n_partials, void *stream);

/* The step's last column sums riding in the norm launch (as scae_rmsprop_sums_step_f32 hosts
 * them in the optimiser pass): the sums equal scae_sum_rows_multi_f32's bit for bit, and those
 * whose destinations lie in `grad` are counted in the partials. */
int scae_grad_sq_partials_sums_f32(float *grad, int64_t n, double *partials, int max_partials,
                                   int *n_partials, const struct scae_sum_job *jobs, int n_jobs,
                                   void *stream);

/* scae_rmsprop_step_f32 / scae_flat_opt_step_f32 with g scaled by the clip coefficient of the
 * norm launch's `partials` (max_norm > 0).  `norm_out` (device float, may be NULL): the
 * norm before clipping, written by the launch's first workgroup. */
int scae_rmsprop_clip_step_f32(float *param, const float *grad, float *square_avg, float *buf,
                               int64_t n, float lr, const float *lr_dev, float alpha, float eps,
                               float momentum, float weight_decay, float grad_scale,
                               const double *partials, int n_partials, float max_norm,
                               float *norm_out, void *stream);
int scae_flat_opt_clip_step_f32(float *param, const float *grad, float *exp_avg,
                                float *exp_avg_sq, float *slow, int64_t n, const float *lr_dev,
                                int32_t *step_state, int kind, double beta1, double beta2,
                                float eps, float weight_decay, float grad_scale,
                                int look_ahead_k, float look_ahead_alpha, int advance,
                                const double *partials, int n_partials, float max_norm,
                                float *norm_out, void *stream);

/* Gradient accumulation over k batches -- Lightning's Trainer(accumulate_grad_batches=k):
 * the optimiser steps on the gradient of a group of batches.  acc: a flat fp32 buffer laid out
 * like `grad` (n floats at grad's offset within a 16-byte line).
 *   scae_grad_accumulate_f32: acc <- acc + grad (fp32, one add per element: adding the
 *   group's gradients in batch order gives acc = g_1 + g_2 + ... bit for bit).
 *   scae_grad_accumulate_sums_f32: the step's last column sums riding in that launch: the sums
 *   equal scae_sum_rows_multi_f32's bit for bit, and those whose destinations lie in `grad`
 *   are added into acc there.
 * The accumulate forms of the optimiser passes and of the norm launch below are the passes
 * above with g = acc + grad in place of grad (then g <- grad_scale g, clipping, weight decay,
 * the update; the norm launch sums (acc + grad)^2); the optimiser passes leave acc = 0 in the
 * elements they update.  With acc == 0 they equal the plain passes bit for bit. */
int scae_grad_accumulate_f32(float *acc, const float *grad, int64_t n, void *stream);
int scae_grad_accumulate_sums_f32(float *acc, float *grad, int64_t n,
                                  const struct scae_sum_job *jobs, int n_jobs, void *stream);
int scae_grad_sq_acc_partials_f32(const float *grad, const float *acc, int64_t n,
                                  double *partials, int max_partials, int *n_partials,
                                  void *stream);
int scae_grad_sq_acc_partials_sums_f32(float *grad, const float *acc, int64_t n,
                                       double *partials, int max_partials, int *n_partials,
                                       const struct scae_sum_job *jobs, int n_jobs,
                                       void *stream);
int scae_rmsprop_acc_step_f32(float *param, const float *grad, float *acc, float *square_avg,
                              float *buf, int64_t n, float lr, const float *lr_dev, float alpha,
                              float eps, float momentum, float weight_decay, float grad_scale,
                              void *stream);
int scae_rmsprop_acc_sums_step_f32(float *param, float *grad, float *acc, float *square_avg,
                                   float *buf, int64_t n, float lr, const float *lr_dev,
                                   float alpha, float eps, float momentum, float grad_scale,
                                   const struct scae_sum_job *jobs, int n_jobs, void *stream);
int scae_rmsprop_acc_clip_step_f32(float *param, const float *grad, float *acc,
                                   float *square_avg, float *buf, int64_t n, float lr,
                                   const float *lr_dev, float alpha, float eps, float momentum,
                                   float weight_decay, float grad_scale, const double *partials,
                                   int n_partials, float max_norm, float *norm_out,
                                   void *stream);
int scae_flat_opt_acc_step_f32(float *param, const float *grad, float *acc, float *exp_avg,
                               float *exp_avg_sq, float *slow, int64_t n, const float *lr_dev,
                               int32_t *step_state, int kind, double beta1, double beta2,
                               float eps, float weight_decay, float grad_scale,
                               int look_ahead_k, float look_ahead_alpha, int advance,
                               void *stream);
int scae_flat_opt_acc_sums_step_f32(float *param, float *grad, float *acc, float *exp_avg,
                                    float *exp_avg_sq, float *slow, int64_t n,
                                    const float *lr_dev, int32_t *step_state, int kind,
                                    double beta1, double beta2, float eps, float grad_scale,
                                    int look_ahead_k, float look_ahead_alpha,
                                    const struct scae_sum_job *jobs, int n_jobs, void *stream);
int scae_flat_opt_acc_clip_step_f32(float *param, const float *grad, float *acc,
                                    float *exp_avg, float *exp_avg_sq, float *slow, int64_t n,
                                    const float *lr_dev, int32_t *step_state, int kind,
                                    double beta1, double beta2, float eps, float weight_decay,
                                    float grad_scale, int look_ahead_k, float look_ahead_alpha,
                                    int advance, const double *partials, int n_partials,
                                    float max_norm, float *norm_out, void *stream);

/* The non-finite guard -- the form of Lightning's Trainer(terminate_on_nan) that skips: an
 * optimiser step whose gradient (acc + grad in the accumulate forms) holds a NaN or +-Inf
 * element writes nothing.  The guarded forms below are the clip forms above behind one
 * decision, with the same arguments plus `guard_state` after `norm_out`.
 *   The rule: every workgroup reduces the norm launch's `partials` in one fixed order, as the
 *   clip forms do, and the step is skipped iff that fp64 sum is not finite.  The norm launch
 *   squares in fp64, so the sum is NaN or +Inf exactly when an element is NaN or +-Inf: finite
 *   fp32 gradients cannot overflow it (the fp32 norm can, and does not decide).  The sum has
 *   the same bits in every workgroup of every launch of the step (one launch per active
 *   range, all on the same partials), so all of them decide alike, with no synchronisation.
 *   A skipped launch, per buffer:
 *     param, both moments / square_avg, buf, slow    no store
 *     step_state (scae_flat_opt)                     no store, no arrival: [0], [1] keep their
 *                                                    values, every counter stays 0
 *     acc (the accumulate forms)                     0 over the launch's n elements
 *     norm_out                                       written as on a taken step: NaN or +Inf
 *   A step that is taken equals the clip form's bit for bit.
 *   max_norm = +inf: the guard without clipping.  The coefficient is then the constant 1 (not
 *   max_norm / (total + 1e-6), which is NaN once a finite gradient's fp32 norm overflows),
 *   and a step that is taken equals the plain pass's (the plain accumulate pass's) bit for bit.
 *   guard_state (device int64[4], 8-byte aligned, may be NULL): {skipped, first, last,
 *   attempts}, initialised by the caller to {0, -1, -1, 0}.  Thread 0 of the first workgroup
 *   of a launch that is handed the pointer counts: t = attempts; on a skip skipped += 1,
 *   first = t if first < 0, last = t; always attempts = t + 1.  Plain loads and stores: hand
 *   the pointer (and norm_out) to ONE launch of a step, its first range's; the launches of
 *   the other ranges take NULL and decide without counting. */
int scae_rmsprop_guard_step_f32(float *param, const float *grad, float *square_avg, float *buf,
                                int64_t n, float lr, const float *lr_dev, float alpha, float eps,
                                float momentum, float weight_decay, float grad_scale,
                                const double *partials, int n_partials, float max_norm,
                                float *norm_out, int64_t *guard_state, void *stream);
int scae_rmsprop_acc_guard_step_f32(float *param, const float *grad, float *acc,
                                    float *square_avg, float *buf, int64_t n, float lr,
                                    const float *lr_dev, float alpha, float eps, float momentum,
                                    float weight_decay, float grad_scale, const double *partials,
                                    int n_partials, float max_norm, float *norm_out,
                                    int64_t *guard_state, void *stream);
int scae_flat_opt_guard_step_f32(float *param, const float *grad, float *exp_avg,
                                 float *exp_avg_sq, float *slow, int64_t n, const float *lr_dev,
                                 int32_t *step_state, int kind, double beta1, double beta2,
                                 float eps, float weight_decay, float grad_scale,
                                 int look_ahead_k, float look_ahead_alpha, int advance,
                                 const double *partials, int n_partials, float max_norm,
                                 float *norm_out, int64_t *guard_state, void *stream);
int scae_flat_opt_acc_guard_step_f32(float *param, const float *grad, float *acc,
                                     float *exp_avg, float *exp_avg_sq, float *slow, int64_t n,
                                     const float *lr_dev, int32_t *step_state, int kind,
                                     double beta1, double beta2, float eps, float weight_decay,
                                     float grad_scale, int look_ahead_k, float look_ahead_alpha,
                                     int advance, const double *partials, int n_partials,
                                     float max_norm, float *norm_out, int64_t *guard_state,
                                     void *stream);

/* Per-parameter gradient norms -- Lightning's Trainer(track_grad_norm=p): one p-norm per
 * segment of a flat buffer, and their total, as one row of a device ring.
 *   A segment is a run of elements [offset, offset + length) of src[0, n), length >= 1;
 *   segments are disjoint and ascending and need not tile the buffer.  Segment s yields
 *   scale * || x ||_p over its elements, x = src or (acc != NULL) acc + src (one fp32 add, as
 *   the accumulate forms above):  p = 2: exact fp64 squares summed in fp64, then sqrt;  p = 1:
 *   the fp64 sum of |x|;  p = inf: max |x| (NaN if any element is NaN, as
 *   torch.linalg.vector_norm); rounded once to fp32.  row[n_segs]: the p-norm of the segment
 *   values, formed in fp64 from their unrounded fp64 values.
 * The caller cuts the segments into chunks once per segment table (a chunk: at most
 * SCAE_NORM_CHUNK elements of ONE segment, chunks ascending) and packs consecutive chunks
 * into groups, one workgroup each (at most SCAE_NORM_GROUP_CHUNKS chunks and
 * 4 * SCAE_NORM_CHUNK elements, unless a single chunk):
 *   chunks      (n_chunks, 2) int32 device: first element, length;
 *   group_first (n_groups + 1) int32 device: the groups' first chunks, then n_chunks;
 *   seg_first   (n_segs + 1) int32 device: the segments' first chunks, then n_chunks.
 * Two launches: every chunk's fp64 partial into `partials` (n_chunks doubles; a wave per
 * chunk, a chunk outside [0, n) yields NaN and reads nothing), then one workgroup that
 * reduces each segment's partials in chunk order and writes the row
 *   ring + (*cursor % capacity) * (n_segs + 1)
 * and then advances *cursor (device int64: a replayed launch writes successive rows); cursor
 * NULL: row 0.  No atomics and no arrival counter; every order of summation is a function of
 * the tables and of src's phase in a 16-byte line, so two runs give the same bits.  A
 * non-finite element changes its own segment's value and the total only.
 * acc: n floats at src's phase in a 16-byte line.  scale >= 0.  n < 2^31. */
#define SCAE_NORM_CHUNK 2048
#define SCAE_NORM_GROUP_CHUNKS 16
#define SCAE_NORM_INF 0 /* norm_kind: 1, 2 or this */
int scae_segment_norms_chunk(void); /* SCAE_NORM_CHUNK of this build */
int scae_segment_norms_f32(const float *src, const float *acc, int64_t n, const int32_t *chunks,
                           int n_chunks, const int32_t *group_first, int n_groups,
                           const int32_t *seg_first, int n_segs, int norm_kind, float scale,
                           double *partials, float *ring, int64_t *cursor, int capacity,
                           void *stream);

/* The batch hand-over of a training step (base_experiment.py:109-112): n_image
 * floats and n_label int64 labels (device memory) into the step's resident
 * input buffers, in one launch. */
int scae_stage_batch(float *dst_image, const float *src_image, int64_t n_image,
                     int64_t *dst_label, const int64_t *src_label, int64_t n_label,
                     void *stream);

/* Prologue of a training step: the three jobs that depend on nothing but the
 * previous step's parameter update, as block ranges of ONE launch ahead of the
 * (replayed) step --
 *   the batch hand-over of scae_stage_batch (base_experiment.py:109-112),
 *   the presence-noise draws of scae_uniform_f32 (part_encoder.py:106,
 *   object_decoder.py:201: n_noise floats, same generator state, same values),
 *   the parameter-only folding products of scae_seed_fold_fwd_f32
 *   (set_transformer.py:218-223; `fold` as there).
 * A part is left out with n_image == 0 / n_noise == 0 / fold == NULL. */
int scae_step_prologue_f32(float *dst_image, const float *src_image, int64_t n_image,
                           int64_t *dst_label, const int64_t *src_label, int64_t n_label,
                           float *noise, int64_t n_noise, uint64_t *noise_state,
                           const scae_seed_fold_desc *fold, void *stream);

/* ... with a fourth job: the image layer of the CNN encoder and the filter re-layouts
 * of its other layers (the arguments of scae_conv3x3_first_fwd_relayout_f32;
 * part_encoder.py:26-44).  `img` is the batch wherever the caller holds it (the
 * hand-over's source or its destination: the layer does not wait for the copy).
 * first == NULL: scae_step_prologue_f32. */
typedef struct scae_first_layer_desc {
  const float *img;   /* (B, Cin, IH, IW) */
  const float *w;     /* (Cout, Cin, 3, 3) */
  const float *bias;  /* (Cout) */
  float *out;         /* (B, OH, OW, Cout) NHWC, ReLU applied */
  int B, Cin, IH, IW, Cout, stride;
  int n_layers;       /* re-layouts riding along (0..8) */
  const float *rw[8]; /* (rCout, rCin, 3, 3) each */
  float *rwf[8];      /* (rCout, 9, rCin) */
  float *rwd[8];      /* (rCin, 9, rCout) */
  int rCout[8], rCin[8];
  /* bf16-resident encoder (scae_conv3x3_*_bf16r): out_h non-NULL -> the layer's output is
   * written as bf16 to out_h INSTEAD of `out` (which must still be a valid pointer), and bf16
   * copies of the re-laid-out filters go to rwfh / rwdh */
  uint16_t *out_h;    /* (B, OH, OW, Cout) bf16, nullable */
  uint16_t *rwfh[8];  /* (rCout, 9, rCin) bf16 */
  uint16_t *rwdh[8];  /* (rCin, 9, rCout) bf16 */
} scae_first_layer_desc;
int scae_step_prologue_first_f32(float *dst_image, const float *src_image, int64_t n_image,
                                 int64_t *dst_label, const int64_t *src_label,
                                 int64_t n_label, float *noise, int64_t n_noise,
                                 uint64_t *noise_state, const scae_seed_fold_desc *fold,
                                 const scae_first_layer_desc *first, void *stream);

/* A batch source: a dataset held in device memory, read through the epoch's order with the
 * reference's MNIST transform applied on the way in (Pad + RandomAffine(translate):
 * mnist/experiment.py:23-40; base_experiment.py:79-93 for the loaders).  Device code:
 * csrc/batch_source_dev.h; torch_scae_amd/data.py holds the CPU form of every draw.
 *   Slot b of rank `rank`'s batch of B is epoch position p = position + rank*B + b (a step's
 *   global batch is world*B positions from `position`); p -> view row perm(p) -> dataset
 *   row index[perm(p)] (index NULL: the view row itself).
 *   shuffle 0: perm = identity (the reference's loaders do not shuffle); 1: a keyed
 *   pseudo-random permutation of [0, n) (4-round Feistel network, Philox round keys of
 *   (seed, epoch, round), cycle-walked) -- not a uniform draw over all n! orders.
 *   translate 1: per-example shifts (dy, dx) = round-half-even(U(-pad, pad)) per axis,
 *   pad = (H - h) / 2, drawn by Philox from (seed; p, epoch); 0: centred padding.
 *   out[b, c, i, j] = x[row, c, i - top, j - left] where that pixel exists, else 0,
 *   top = (H - h)/2 + dy, left = (W - w)/2 + dx; uint8 pixels / 255.0f (correctly rounded).
 *   Labels (uint8 or int64) are written as int64.  C <= 4 (else SCAE_ERR_UNSUPPORTED),
 *   h <= H, w <= W, n < 2^31, position + (rank + 1) * B <= n.
 *   wrap 1 (a drop_last=False epoch's short last step, DistributedSampler's padding): a
 *   position p >= n reads view row perm(p - n) -- the epoch's first examples again -- while
 *   its shift is still drawn from p itself; then position + (rank + 1) * B <= 2n instead.
 *   wrap 0 (ctypes' zero): no position may reach n.
 *   affine non-NULL: the rest of the reference's transform -- RandomAffine(degrees, translate,
 *   scale, shear) with nearest-neighbour resampling, as Pillow's fixed-point AFFINE path
 *   samples it.  Row p of `affine` (affine_rows, 6) int32 holds position p's inverse map
 *   k0..k5 in 16.16 fixed point; the host builds the table once per epoch
 *   (data.affine_coefficients) and this launch only reads it:
 *     one Philox draw (the generator's key schedule, 10 rounds, key = seed) at counter
 *     (p, epoch_lo, epoch_hi, TAG_AFFINE); its words 0..3 >> 8 are 24-bit r for angle, scale,
 *     shear-x, shear-y, value = lo + (hi - lo) * r / 2^24 in fp64 (degrees; scale 1 and
 *     shear 0 where not asked for); (ty, tx) = the shift (dy, dx) above, acting on the
 *     padded (H, W) image; under wrap the draw uses the unwrapped p, as the shift does;
 *     with rot, sx, sy in radians and (cx, cy) = (W * 0.5, H * 0.5), in fp64:
 *       a = cos(rot - sy) / cos(sy)     b = -cos(rot - sy) * tan(sx) / cos(sy) - sin(rot)
 *       c = sin(rot - sy) / cos(sy)     d = -sin(rot - sy) * tan(sx) / cos(sy) + cos(rot)
 *       M = [d, -b, 0, -c, a, 0] / scale
 *       M[2] += M[0] * (-cx - tx) + M[1] * (-cy - ty) + cx
 *       M[5] += M[3] * (-cx - tx) + M[4] * (-cy - ty) + cy
 *     (torchvision's _get_inverse_affine_matrix); FIX(v) = floor(v * 65536 + 0.5),
 *       k0, k1, k3, k4 = FIX(M[0]), FIX(M[1]), FIX(M[3]), FIX(M[4])
 *       k2 = FIX(M[2] + M[0] * 0.5 + M[1] * 0.5)    k5 = FIX(M[5] + M[3] * 0.5 + M[4] * 0.5)
 *   Sampling is pure integers (int64, arithmetic shifts): for pixel (i, j) of the padded image
 *     xin = (k2 + k1 * i + k0 * j) >> 16      yin = (k5 + k4 * i + k3 * j) >> 16
 *     out[b, c, i, j] = x[row, c, yin - (H - h)/2, xin - (W - w)/2] inside the example, else 0
 *   (degrees = 0 without scale and shear gives the bits of affine = NULL); `translate` is
 *   no switch then -- the table holds the shift -- but the sampling mode: 0 or 1 the nearest
 *   form above, 2 bilinear.  position + (rank + 1) * B <= affine_rows.
 *   Bilinear (translate = 2, affine non-NULL), int64 with arithmetic shifts as above:
 *     U = k2 + k1 * i + k0 * j - 32768           V = k5 + k4 * i + k3 * j - 32768
 *     x0 = (U >> 16) - (W - w)/2   fx = (U >> 8) & 255
 *     y0 = (V >> 16) - (H - h)/2   fy = (V >> 8) & 255
 *     t00 = x[row, c, y0, x0]  t01 = x[.., y0, x0 + 1]  t10 = x[.., y0 + 1, x0]  t11 = x[.., y0 + 1, x0 + 1]
 *   each tap 0 where it falls outside the example or the row outside the dataset.
 *   uint8: acc = (256 - fy) * ((256 - fx) * t00 + fx * t01) + fy * ((256 - fx) * t10 + fx * t11)
 *   (an integer < 2^24), out = (float)acc / 16711680.0f, correctly rounded.  fp32: weights
 *   fx / 256, (256 - fx) / 256, ... (exact); top = w_x0 * t00 + w_x1 * t01, bot likewise,
 *   out = w_y0 * top + w_y1 * bot, every product and sum rounded to fp32 on its own.  At
 *   integer coordinates (fx = fy = 0) these are the nearest form's bits.  A horizontal flip
 *   or a shift range other than the pads is composed into the table's rows by the host
 *   (data.affine_coefficients: flip=, max_shift=); the launch does not know of them.
 *   affine NULL (ctypes' zero): translation alone, as above; translate must be 0 or 1.
 *   Any other translate value (< 0, > 2, or 2 without a table) is refused (-1) before any
 *   HIP call. */
typedef struct scae_batch_source_desc {
  const void *images;     /* (rows, C, h, w) uint8 (image_u8 = 1) or fp32 in [0, 1] */
  const void *labels;     /* (rows) uint8 (label_u8 = 1) or int64; nullable without labels out */
  const int32_t *index;   /* (n) dataset rows of the view, nullable: rows 0 .. n-1 */
  int64_t rows;           /* examples in the dataset (rows outside it read as zeros) */
  int64_t n;              /* examples in the view */
  int image_u8, label_u8;
  int C, h, w, H, W;
  int shuffle, translate;
  uint64_t seed;
  int64_t epoch, position;
  int rank, world;
  int wrap;               /* 1: positions in [n, 2n) read rows of p - n (see above) */
  const int32_t *affine;  /* (affine_rows, 6) k0..k5 of each epoch position, nullable */
  int64_t affine_rows;    /* positions the table covers */
} scae_batch_source_desc;
/* The rank's batch of B from `src` into dst_image (B, C, H, W) fp32 and dst_label (B) int64
 * (nullable), one launch. */
int scae_gather_batch_f32(float *dst_image, int64_t *dst_label, int B,
                          const scae_batch_source_desc *src, void *stream);
/* scae_step_prologue_first_f32 with the batch hand-over taken from `src`: its staging
 * workgroups gather the rank's batch of B into dst_image / dst_label (as
 * scae_gather_batch_f32), and the image layer's workgroups (first, nullable) build their LDS
 * copy of each image from `src` through the same device code -- first->img is not read; first
 * must describe B images of src's (C, H, W).  Noise, folding products and re-layouts as
 * there. */
int scae_step_prologue_source_f32(float *dst_image, int64_t *dst_label, int B,
                                  const scae_batch_source_desc *src, float *noise,
                                  int64_t n_noise, uint64_t *noise_state,
                                  const scae_seed_fold_desc *fold,
                                  const scae_first_layer_desc *first, void *stream);

/* ------------------------------------------------------------------------
 * K10  coloured templates      replaces TemplateGenerator.forward,
 *      part_decoder.py:78-110 (colorize_templates = True):
 *        raw (M,C,hw)        = nonlin_t(logits)
 *        colour (B,M,C)      = nonlin_c'(relu(W2 relu(W1 feature + b1) + b2))
 *                              (nonlin_c' = sigmoid, or relu1(. + .99))
 *        templates (B,M,C,hw) = raw * colour
 *      nonlin codes: 0 sigmoid, 1 relu1 (nn_ext.py:139-140).
 *      w1 (H1,F), b1 (H1), w2 (C,H1), b2 (C); feature (B,M,F).
 *      backward: g_templates (B,M,C,hw), g_raw (M,C,hw, nullable) ->
 *      g_logits (M,C,hw), g_feature (B,M,F), partial
 *      (scae_template_color_partial_rows(B,M), H1*F + H1 + C*H1 + C) =
 *      per-workgroup [dW1 | db1 | dW2 | db2] for the caller to sum over dim 0.
 * ---------------------------------------------------------------------- */
int scae_template_color_supported(int M, int C, int F, int H1);
int scae_template_color_partial_rows(int B, int M);
int scae_template_color_fwd_f32(const float *logits, const float *feature, const float *w1,
                                const float *b1, const float *w2, const float *b2, float *raw,
                                float *templates, float *color, int B, int M, int C, int hw,
                                int F, int H1, int template_nonlin, int color_nonlin,
                                void *stream);
int scae_template_color_bwd_f32(const float *logits, const float *feature, const float *w1,
                                const float *b1, const float *w2, const float *b2,
                                const float *color, const float *g_templates,
                                const float *g_raw, float *g_logits, float *g_feature,
                                float *partial, int B, int M, int C, int hw, int F, int H1,
                                int template_nonlin, int color_nonlin, void *stream);

/* ------------------------------------------------------------------------
 * Column sums of a (rows, cols) matrix of partial gradients, written to up to
 * 8 contiguous destinations: column j in [begin, end) of segment i goes to
 * segments[i].dst[j - begin]; with period > 0 the window [begin, end) of
 * every period-wide block of columns is gathered instead:
 * dst[(j / period) * (end - begin) + j % period - begin] (cols must be a
 * multiple of period: SCAE_ERR_BAD_ARG otherwise).  period = -W < 0:
 * the window is an (n x W) matrix whose TRANSPOSE is written,
 * dst[((j - begin) % W) * n + (j - begin) / W] (an NHWC batch sum landing in
 * a (C,H,W) parameter).  Columns in no
 * segment are dropped; segments may overlap.  `segments` is a HOST array.  Replaces `partial.sum(0)` + per-parameter slice copies
 * behind the partial-gradient outputs of K1, K2b, K2c, K3, K8, K9 and K10.
 * ---------------------------------------------------------------------- */
typedef struct scae_sum_segment {
  float *dst;
  int64_t begin, end, period;
} scae_sum_segment;
int scae_sum_rows_f32(const float *src, int64_t rows, int64_t cols,
                      const scae_sum_segment *segments, int n_segments, void *stream);
/* Up to 16 such column-sum jobs (different matrices) in ONE launch: a backward
 * pass usually leaves two or three partial matrices behind at the same time,
 * and the sums that only feed the optimiser (parameter gradients) of a whole
 * training step can wait for one launch at its end.
 * `jobs` and the segment arrays it points to are HOST memory. */
typedef struct scae_sum_job {
  const float *src;
  int64_t rows, cols;
  const scae_sum_segment *segments;
  int n_segments;
} scae_sum_job;
int scae_sum_rows_multi_f32(const scae_sum_job *jobs, int n_jobs, void *stream);

/* Up to 8 scaled full sums in ONE launch: dst[i][0] = scale[i] * sum(src[i][0..n[i]))
 * (one workgroup each, fixed order).  The scalar outputs of the forward pass:
 * cpr_dynamic_reg_loss = sum(reg_partial)/2/B (object_decoder.py:170) and
 * log_prob = sum(log_prob_per_point)/B (:301-306). */
typedef struct scae_scaled_sum {
  const float *src;
  int64_t n;
  float scale;
  float *dst;
} scae_scaled_sum;
int scae_scaled_sums_f32(const scae_scaled_sum *jobs, int n_jobs, void *stream);

/* ------------------------------------------------------------------------
 * K3  capsule votes                  replaces object_decoder.py:160-225
 *     (+ cv_ops.py:20-76 on OPR/OVR, the batched 3x3 product :189-191)
 *   all_param (B,O,A), A = 6V+6+1+2V, the output of the per-capsule MLPs,
 *     split as [cpr_dynamic 6V | cvr 6 | caps logit 1 | vote logit V |
 *     scale V] (:160-162); consecutive capsule rows are ld_param >= A floats
 *     apart (0 = A; a multiple of 4 lets the MLP GEMMs on either side use
 *     16-byte accesses), the gradients of the backward pass likewise.
 *   cpr_static (O,V,6); bias_cvr (O,6); bias_caps (O); bias_vote (O,V);
 *   bias_scale (O,V)  (caps_bias_list, :108-111).
 *   noise_caps (B,O) / noise_vote (B,O,V): U[0,1) draws, nullable (no noise);
 *     the kernel adds (u-0.5)*noise_scale (:201).
 *   outputs: vote (B,O,V,6) = top two rows of OVR x OPR (:189-191, :413),
 *     scale (B,O,V) (:225), vote_presence (B,O,V) (:217-219),
 *     logit_caps (B,O), logit_vote (B,O,V) (noised logits, :211-212),
 *     reg_partial (B,O): per-(b,o) sum of cpr_dynamic^2 (caller: sum/2/B,
 *     :170); caps_presence (B,O) = max_v vote_presence with its first
 *     maximiser caps_arg (B,O) int32 (object_decoder.py:411; both nullable).
 * ---------------------------------------------------------------------- */
int scae_capsule_votes_fwd_f32(const float *all_param, const float *cpr_static,
                               const float *bias_cvr, const float *bias_caps,
                               const float *bias_vote, const float *bias_scale,
                               const float *noise_caps, const float *noise_vote,
                               float noise_scale, float *vote, float *scale,
                               float *vote_presence, float *logit_caps,
                               float *logit_vote, float *reg_partial,
                               float *caps_presence, int *caps_arg, int B, int O, int V,
                               int ld_param, int similarity, int learn_vote_scale,
                               int allow_deformations, void *stream);
/* incoming grads (all nullable = zero): gvote (B,O,V,6) gscale (B,O,V)
 * gvote_presence (B,O,V) glogit_caps (B,O) glogit_vote (B,O,V);
 * greg: d loss / d cpr_dynamic_reg_loss, a DEVICE scalar, nullable;
 * gcaps_presence (B,O) nullable, routed to vote caps_arg of each capsule.
 * outputs: gall_param (B,O,A); gcpr_in (B,O,V,6) = grad wrt
 * (cpr_dynamic + cpr_static) (caller sums over B for cpr_static; the bias
 * grads are the batch sums of the matching gall_param slices);
 * gall_param_gated (B,O,A), nullable: gall_param zeroed where all_param <= 0,
 * i.e. the gradient w.r.t. the pre-activation of the ReLU that produced
 * all_param (saves the caller a threshold_backward launch). */
int scae_capsule_votes_bwd_f32(const float *all_param, const float *cpr_static,
                               const float *bias_cvr, const float *bias_caps,
                               const float *bias_vote, const float *bias_scale,
                               const float *noise_caps, const float *noise_vote,
                               float noise_scale, const float *gvote,
                               const float *gscale, const float *gvote_presence,
                               const float *glogit_caps, const float *glogit_vote,
                               const float *greg, const float *gcaps_presence,
                               const int *caps_arg, float *gall_param, float *gcpr_in,
                               float *gall_param_gated, int B, int O, int V, int ld_param,
                               int similarity, int learn_vote_scale,
                               int allow_deformations, void *stream);

/* ------------------------------------------------------------------------
 * K4  capsule likelihood             replaces object_decoder.py:257-372
 *   vote (B,O,M,6) scale (B,O,M) vote_presence (B,O,M) dummy_vote (M,6)
 *   x (B,M,6) presence (B,M) nullable
 *   outputs: log_prob_per_point (B,M) (:296-300; caller: sum/B -> log_prob),
 *     vote_presence_binary (B,O,M), winner (B,M,6), winner_presence (B,M),
 *     winner_idx (B,M) int64 (:310), is_from_capsule (B,M) int64 (:334),
 *     soft_winner (B,M,6), soft_winner_presence (B,M),
 *     posterior (B,O+1,M) (softmax of :338 incl. the dummy row),
 *     mixing_log_prob (B,O+1,M), mixing_logit (B,O+1,M).
 * ---------------------------------------------------------------------- */
int scae_capsule_likelihood_fwd_f32(
    const float *vote, const float *scale, const float *vote_presence,
    const float *dummy_vote, const float *x, const float *presence,
    float *log_prob_per_point, float *vote_presence_binary, float *winner,
    float *winner_presence, int64_t *winner_idx, int64_t *is_from_capsule,
    float *soft_winner, float *soft_winner_presence, float *posterior,
    float *mixing_log_prob, float *mixing_logit, int B, int O, int M,
    void *stream);
/* incoming grads, each nullable: g_lpp (B,M), g_winner (B,M,6),
 * g_winner_presence (B,M), g_soft_winner (B,M,6), g_soft_winner_presence
 * (B,M), g_posterior (B,O+1,M), g_mixing_log_prob (B,O+1,M), g_mixing_logit
 * (B,O+1,M).  outputs: gvote, gscale, gvote_presence, gx (B,M,6),
 * gpresence (B,M) (nullable), gdummy_partial (B,M,6) (caller sums over B). */
int scae_capsule_likelihood_bwd_f32(
    const float *vote, const float *scale, const float *vote_presence,
    const float *dummy_vote, const float *x, const float *presence,
    const float *posterior, const int64_t *winner_idx, const float *g_lpp,
    const float *g_winner, const float *g_winner_presence,
    const float *g_soft_winner, const float *g_soft_winner_presence,
    const float *g_posterior, const float *g_mixing_log_prob,
    const float *g_mixing_logit, float *gvote, float *gscale,
    float *gvote_presence, float *gx, float *gpresence, float *gdummy_partial,
    int B, int O, int M, void *stream);

/* ------------------------------------------------------------------------
 * Class probabilities of SCAE.forward
 *     replaces stacked_capsule_auto_encoder.py:205-212:
 *     prior_prob (B,ncls) = softmax(w caps_presence + bias),
 *     post_prob  (B,ncls) = softmax(w sum_m posterior[:, :O, m] + bias)
 *     with caps_presence (B,O), posterior (B,O+1,M), w (ncls,O), bias (ncls)
 *     = prior_classifier.0 (the reference routes both through it).
 *     Limits: O <= 64, ncls <= 32.
 *     extra_sums (HOST array, n_extra <= 8, nullable): scaled full sums (see
 *     scae_scaled_sums_f32) that ride in the same launch -- this is the last
 *     kernel of SCAE.forward, and the forward's scalar outputs (log_prob,
 *     cpr_dynamic_reg_loss) are not read before it.
 * ---------------------------------------------------------------------- */
int scae_class_probs_supported(int O, int ncls);
int scae_class_probs_f32(const float *caps_presence, const float *posterior, const float *w,
                         const float *bias, float *prior_prob, float *post_prob, int B, int O,
                         int M, int ncls, const scae_scaled_sum *extra_sums, int n_extra,
                         void *stream);

/* ------------------------------------------------------------------------
 * K6  fused tail of SCAE.loss        replaces stacked_capsule_auto_encoder.py
 *     :238-285 + object_decoder.py:433-493 (+ math_ops.py) and their backward
 *   lpp (B,M) log_prob_per_point; posterior (B,O+1,M); caps_presence (B,O);
 *   cls_w (ncls,O), cls_b (ncls): prior_classifier.0 (both classification
 *   terms go through it, like the reference :207-212); label (B) int64
 *   nullable (no classification terms).
 *   prior_type / post_type: 0 'l2', 1 'entropy', 2 'kl'; sparsity_on: the
 *   reference's gate (prior weights > 0, :243/:258); weights5 (HOST array) =
 *   [caps_ll, prior_within, prior_between, posterior_within,
 *   posterior_between]; within_const: prior_within_example_constant or NaN
 *   (= n_caps/n_classes); n_classes_cfg: SCAE.n_classes (l2 constants).
 *   out12: [loss, log_prob, prior_within, prior_between, post_within,
 *   post_between, prior_cls_xe, posterior_cls_xe, rec_ll, -rec_ll, -log_prob,
 *   reg]; loss = -w0*log_prob + w1*pw + w2*pb + w3*qw + w4*qb + xe + xe
 *                - rec_ll + w_reg*reg.
 *   extras (nullable): the remaining terms of the training loss, so that the
 *   whole scalar (:217-287) leaves one kernel -- rec_sums (n_rec) = K1's tile
 *   sums of the reconstruction log-likelihood (rec_ll = sum / B, :222-224), reg
 *   (1) = cpr_dynamic_reg_loss with its weight w_reg (:270-272); g_rec_sums /
 *   g_reg receive their gradients in the backward pass.
 *   backward: gout12 (12) -> g_lpp, g_posterior, g_caps_presence, g_cls_w,
 *   g_cls_b (classifier inputs are detached in the reference).
 *   workspace: scae_loss_tail_workspace_floats(B,O,ncls) floats owned by the
 *   caller; the forward leaves the per-image / per-column statistics there and
 *   the backward of the same inputs reads them.
 * ---------------------------------------------------------------------- */
/* The training log: a nullable descriptor that makes the loss tail's batch combine (wherever
 * it runs: the deferred workgroup of scae_loss_tail_bwd_f32 or the standalone combine) end in
 * an epilogue -- the replayed step's `log` of BaseExperiment.training_step
 * (base_experiment.py:109-126) with no launch of its own.  The epilogue
 *   - forms both heads' accuracies from prior_prob / post_prob (B, ncls), which
 *     scae_loss_tail_fwd_class_probs_f32 wrote in the same batch, as the evaluation epilogue
 *     does (torch.argmax: first maximal index, NaN maximal; count / B in fp32; zero without a
 *     label; the batch value is the max of the two heads);
 *   - writes one row of SCAE_TRAIN_LOG_ROW floats at rows + (step[0] % capacity) * ROW:
 *       [0] loss  [1] accuracy  [2] prior accuracy  [3] posterior accuracy
 *       [4 + i] out12[i], i < 12  [16] learning rate (lr[0]; NaN when lr is NULL)
 *       [17] mse  [18] part-capsule L1 (scae_train_log_f32's extra2 only; else zero);
 *   - advances the device step counter step[0] by one (ONE thread, in stream order: a captured
 *     launch follows the count, as the optimisers' step count does);
 *   - adds the batch into acc (nullable), laid out as SCAE_EVAL_ACC_DOUBLES, in stream order
 *     with one writer per entry and no atomics: the sums are reproducible bit for bit.
 * The descriptor itself is host memory, read when the launch is issued; the pointers in it
 * are device memory. */
/* The evaluation feature sink: DEVICE memory that a captured launch reaches by its address, so
 * that pointing it at another output needs no new capture.  Batch rows [cursor, cursor + B)
 * of an (capacity, 2, O) fp32 matrix receive each image's two classifier inputs: [.., 0, o]
 * the prior presence caps_presence[b, o] and [.., 1, o] the posterior mass
 * sum_m posterior[b, o, m] (summed as scae_class_probs_f32 sums it).  A row at or beyond
 * capacity is dropped and sets overflow; the batch's last launch advances cursor by B (ONE
 * thread, in stream order).  capacity 0: the sink is off -- nothing is written and the cursor
 * stays. */
typedef struct scae_eval_sink {
  float *rows;
  int64_t capacity;
  int64_t cursor;
  int64_t overflow;
} scae_eval_sink;
/* The evaluation records: DEVICE memory that a captured launch reaches by its address, like
 * the feature sink.  Batch rows [cursor, cursor + B) of a (capacity, SCAE_EVAL_RECORD_FLOATS)
 * fp32 matrix receive one record per image, written by the batch's last launch:
 *   [0] label as a float (-1 without labels)
 *   [1] prior-head class  [2] posterior-head class: argmax over the head's class probabilities
 *       as torch.argmax takes it (first maximal index, NaN maximal), the rule of the accuracies
 *   [3] [4] the two heads' probability of their own predicted class
 *   [5] [6] the two heads' probability of the label's class (0 without labels, or for a label
 *       outside [0, ncls))
 *   [7] the image's reconstruction log-likelihood, rec_ll_per_pixel.view(B, -1).sum(-1)[b]: its
 *       tile sums added in tile order (or, from a per-pixel map, one wave's strided sum)
 *   [8] the image's capsule log-likelihood sum_m lpp[b, m], summed as the loss tail sums it.
 * Without class probabilities (ncls = 0) entries [1..6] are -1, -1, 0, 0, 0, 0.
 * confusion is a (2, ncls, ncls) int64 matrix indexed [head, label, predicted], head 0 the
 * prior and head 1 the posterior: the batch's two histograms are built on chip and added by
 * ONE workgroup in stream order, one writer per cell and no global atomics, so repeated runs
 * give the same counts.  Images without a label, or with one outside [0, ncls), are not
 * counted.  ncls here must equal the launch's ncls, or nothing is counted.
 * labelled 0: the labels the launches carry are placeholders (a step always stages some) --
 * the rows are written as without labels and nothing is counted.
 * A row at or beyond capacity is dropped, is not counted either (confusion is always the
 * histogram of the rows written) and sets overflow; cursor advances by B after everything
 * else (ONE thread, in stream order).  capacity 0: the records are off -- nothing is written
 * and the cursor stays. */
#define SCAE_EVAL_RECORD_FLOATS 9
#define SCAE_EVAL_RECORDS_MAX_CLASSES 64
typedef struct scae_eval_records {
  float *rows;
  int64_t capacity;
  int64_t cursor;
  int64_t overflow;
  int64_t *confusion;
  int64_t ncls;
  int64_t labelled;
} scae_eval_records;
#define SCAE_TRAIN_LOG_ROW 19
typedef struct scae_train_log_desc {
  float *rows;      /* (capacity, SCAE_TRAIN_LOG_ROW) ring */
  int64_t *step;    /* (1) rows written so far */
  int capacity;
  double *acc;      /* nullable: SCAE_EVAL_ACC_DOUBLES epoch accumulator */
  const float *prior_prob, *post_prob;  /* (B, ncls); unused without a label */
  const int64_t *label;                 /* (B) nullable: no accuracies */
  int ncls;
  const float *lr;  /* nullable: the learning rate the optimiser reads in this step */
} scae_train_log_desc;
typedef struct scae_loss_extras {
  const float *rec_sums;
  int n_rec;
  const float *reg;
  float w_reg;
  float *g_rec_sums, *g_reg;
  float *loss;          /* forward: also receives out12[0] (a separate scalar) */
  const float *g_loss;  /* backward: gradient of that scalar, added to gout12[0];
                           gout12 may then be NULL (= zeros) */
  /* A training step in which nothing reads the forward's scalars before the backward has
   * run: with defer_combine the forward launches its per-image kernel only, and the batch
   * combine (out12, loss) is one more workgroup of the BACKWARD launch, which then needs
   * out12 (and loss) here.  scae_loss_tail_combine_f32 is that combine on its own, for a
   * deferred forward that no backward followed. */
  int defer_combine;
  float *out12;
  /* nullable: the training log's epilogue after the combine (scae_train_log_desc); ignored by
   * the evaluation epilogue and by a forward whose combine is deferred */
  const scae_train_log_desc *train_log;
} scae_loss_extras;
int scae_loss_tail_supported(int B, int O, int ncls);
int64_t scae_loss_tail_workspace_floats(int B, int O, int ncls);
int scae_loss_tail_fwd_f32(const float *lpp, const float *posterior,
                           const float *caps_presence, const float *cls_w,
                           const float *cls_b, const int64_t *label,
                           const scae_loss_extras *extras, float *out12, float *workspace,
                           int B, int O, int M, int ncls, int n_classes_cfg, int prior_type,
                           int post_type, int sparsity_on, const float *weights5,
                           float within_const, void *stream);
/* defer_combine costs B^2 2 O extra loads in the backward: worth it for small batches only */
int scae_loss_tail_defer_preferred(int B, int O);
int scae_loss_tail_combine_f32(const float *lpp, const float *posterior,
                               const float *caps_presence, const float *cls_w,
                               const float *cls_b, const int64_t *label,
                               const scae_loss_extras *extras, float *out12, float *workspace,
                               int B, int O, int M, int ncls, int n_classes_cfg, int prior_type,
                               int post_type, int sparsity_on, const float *weights5,
                               float within_const, void *stream);
/* scae_loss_tail_fwd_f32 with the workgroups of scae_class_probs_f32 (arguments cp_* ..
 * n_extra, same meaning) riding in its per-image launch: both are one wave per image and
 * independent, and in a training step nothing reads the class probabilities in between. */
int scae_loss_tail_fwd_class_probs_f32(
    const float *lpp, const float *posterior, const float *caps_presence, const float *cls_w,
    const float *cls_b, const int64_t *label, const scae_loss_extras *extras, float *out12,
    float *workspace, int B, int O, int M, int ncls, int n_classes_cfg, int prior_type,
    int post_type, int sparsity_on, const float *weights5, float within_const,
    const float *cp_caps_presence, const float *cp_posterior, const float *cp_w,
    const float *cp_bias, float *prior_prob, float *post_prob, int cp_B, int cp_O, int cp_M,
    int cp_ncls, const scae_scaled_sum *extra_sums, int n_extra, void *stream);
/* The same with the evaluation feature sink (scae_eval_sink, DEVICE memory, nullable): the
 * riding image workgroups store their classifier inputs at rows cursor + b.  The cursor is
 * advanced by the batch's last launch (scae_eval_tail_sink_f32). */
int scae_loss_tail_fwd_class_probs_sink_f32(
    const float *lpp, const float *posterior, const float *caps_presence, const float *cls_w,
    const float *cls_b, const int64_t *label, const scae_loss_extras *extras, float *out12,
    float *workspace, int B, int O, int M, int ncls, int n_classes_cfg, int prior_type,
    int post_type, int sparsity_on, const float *weights5, float within_const,
    const float *cp_caps_presence, const float *cp_posterior, const float *cp_w,
    const float *cp_bias, float *prior_prob, float *post_prob, int cp_B, int cp_O, int cp_M,
    int cp_ncls, const scae_scaled_sum *extra_sums, int n_extra, scae_eval_sink *sink,
    void *stream);
int scae_loss_tail_bwd_f32(const float *lpp, const float *posterior,
                           const float *caps_presence, const float *cls_w,
                           const float *cls_b, const int64_t *label,
                           const scae_loss_extras *extras, const float *gout12,
                           const float *workspace, float *g_lpp, float *g_posterior,
                           float *g_caps_presence, float *g_cls_w,
                           float *g_cls_b, int B, int O, int M, int ncls, int n_classes_cfg,
                           int prior_type, int post_type, int sparsity_on,
                           const float *weights5, float within_const, void *stream);

/* ------------------------------------------------------------------------
 * Evaluation epilogue (csrc/eval_tail.hip): the last launch of an evaluation batch.
 *   replaces SCAE.calculate_accuracy (stacked_capsule_auto_encoder.py:289-297) and the
 *   per-batch outputs plus epoch means of BaseExperiment.validation_step /
 *   validation_epoch_end / test_step / test_epoch_end (base_experiment.py:128-202)
 * ------------------------------------------------------------------------ */
/* The fp64 accumulator (zero it to start an epoch):
 *   [0] batches  [1] sum loss  [2] sum accuracy (max of the heads)  [3] sum prior accuracy
 *   [4] sum posterior accuracy  [5 + i] sum of out12[i], i < 12 (scae_loss_tail_fwd_f32's
 *   12-vector; zero when out12 is not given).  ONE thread adds a batch, in stream order:
 * the sums are reproducible bit for bit.  batch3 (nullable) receives the batch's {accuracy,
 * prior accuracy, posterior accuracy}.  Accuracy of a head: argmax over its class
 * probabilities (torch.argmax: first maximal index, NaN maximal) == label, count / B in fp32;
 * zero without a label. */
#define SCAE_EVAL_ACC_DOUBLES 17
/* The loss tail's batch combine -- the same bits as scae_loss_tail_combine_f32 for the same
 * arguments (extras->defer_combine ignored) -- plus the accuracies from prior_prob / post_prob
 * (B, ncls), which scae_loss_tail_fwd_class_probs_f32 wrote in the same batch, plus the
 * accumulation.  One workgroup.  Follows a forward launched with defer_combine. */
int scae_eval_tail_f32(const float *lpp, const float *posterior, const float *caps_presence,
                       const float *cls_w, const float *cls_b, const int64_t *label,
                       const scae_loss_extras *extras, float *out12, float *workspace, int B,
                       int O, int M, int ncls, int n_classes_cfg, int prior_type,
                       int post_type, int sparsity_on, const float *weights5,
                       float within_const, const float *prior_prob, const float *post_prob,
                       double *acc, float *batch3, void *stream);
/* The same, ending the batch of a feature sink (nullable): thread 0 advances its cursor by B
 * after the accumulation. */
int scae_eval_tail_sink_f32(const float *lpp, const float *posterior, const float *caps_presence,
                            const float *cls_w, const float *cls_b, const int64_t *label,
                            const scae_loss_extras *extras, float *out12, float *workspace,
                            int B, int O, int M, int ncls, int n_classes_cfg, int prior_type,
                            int post_type, int sparsity_on, const float *weights5,
                            float within_const, const float *prior_prob, const float *post_prob,
                            double *acc, float *batch3, scae_eval_sink *sink, void *stream);
/* The same, also writing the batch's evaluation records (scae_eval_records, nullable like the
 * sink): the combine workgroup, which reads every image's class probabilities, tile sums
 * (extras->rec_sums as (B, n_rec / B); column [7] is zero without them) and per-image
 * workspace entry, writes the rows and the confusion counts before the combine and advances
 * the records' cursor last.  out12, acc and batch3 get the bits scae_eval_tail_sink_f32 gives.
 * At most SCAE_EVAL_RECORDS_MAX_CLASSES classes (the tail itself takes 32). */
int scae_eval_tail_records_f32(const float *lpp, const float *posterior,
                               const float *caps_presence, const float *cls_w,
                               const float *cls_b, const int64_t *label,
                               const scae_loss_extras *extras, float *out12, float *workspace,
                               int B, int O, int M, int ncls, int n_classes_cfg, int prior_type,
                               int post_type, int sparsity_on, const float *weights5,
                               float within_const, const float *prior_prob,
                               const float *post_prob, double *acc, float *batch3,
                               scae_eval_sink *sink, scae_eval_records *records, void *stream);
/* The records of one batch and the cursor's advance as a launch of its own, for a model outside
 * the fused tail.  prior_prob / post_prob (B, ncls) nullable together (ncls = 0), label (B)
 * nullable, lpp (B, M) nullable (column [8] zero).  The reconstruction term comes from
 * rec_sums (B, n_rec), added in tile order, or else from rec_pixels (B, n_rec), a per-pixel
 * log-likelihood map that one wave per image sums; both NULL: column [7] zero.  One
 * workgroup.  SCAE_ERR_UNSUPPORTED beyond SCAE_EVAL_RECORDS_MAX_CLASSES classes. */
int scae_eval_records_f32(const float *prior_prob, const float *post_prob, const int64_t *label,
                          const float *lpp, const float *rec_sums, const float *rec_pixels,
                          int B, int ncls, int M, int n_rec, scae_eval_records *records,
                          void *stream);
/* Accuracies + accumulation only, for a loss other launches computed (a model outside the
 * fused tail: recon_mse_weight > 0, part_caps_sparsity_weight > 0, more than 32 classes):
 * loss (1), out12 (12, nullable), prior_prob / post_prob (B, ncls) and label (nullable
 * together: n_classes=None; any ncls > 0). */
int scae_eval_accumulate_f32(const float *loss, const float *out12, const float *prior_prob,
                             const float *post_prob, const int64_t *label, int B, int ncls,
                             double *acc, float *batch3, void *stream);
/* The feature sink's rows of one batch and the cursor's advance as a launch of its own, for a
 * batch whose class probabilities did not ride in the loss tail (O > 64, no classes, a model
 * outside the fused tail): caps_presence (B, O), posterior (B, O + 1, M) -- only its first O
 * rows are read.  One workgroup. */
int scae_eval_features_f32(const float *caps_presence, const float *posterior, int B, int O,
                           int M, scae_eval_sink *sink, void *stream);
/* The training log's epilogue alone (scae_train_log_desc, B images), for a loss other launches
 * computed (a model outside the fused tail, or a step whose plan holds no class probabilities):
 * loss (1), out12 (12, nullable: zeros), extra2 (2, nullable: zeros) = {mse, part-capsule L1}.
 * One workgroup. */
int scae_train_log_f32(const float *loss, const float *out12, const float *extra2,
                       const scae_train_log_desc *log, int B, void *stream);

/* ------------------------------------------------------------------------
 * K1  template render + Gaussian-mixture image likelihood
 *     replaces part_decoder.py:174-237 (affine_grid + 2x grid_sample +
 *     background + presence), distributions.py:34-47 (mixture log_prob) and
 *     the rec term of stacked_capsule_auto_encoder.py:220.
 *
 * Decoder description shared by the K1 entry points:
 *   templates (B,M,C,th,tw); pose (B,M,6) = row-major 2x3 affine;
 *   presence (B,M) nullable;
 *   templates_alpha (M,th,tw) -- non-null selects the alpha-channel mode
 *     (mixing logits have ONE channel, Cm = 1), null selects the temperature
 *     mode (logits = transformed/temperature, Cm = C) and then
 *     temperature_logit (1) must be given;
 *   bg_image (B,C,H,W) nullable; when null bg_value (1) must be given;
 *   bg_mixing_logit (1) (alpha mode only);
 *   out_scale (1) nullable: sigma = softplus(out_scale)+1e-4, else sigma = 1.
 *   K = M+1 mixture components, the last one is the background.
 * ---------------------------------------------------------------------- */
typedef struct scae_decoder_desc {
  const float *templates;
  const float *templates_alpha;
  const float *pose;
  const float *presence;
  const float *bg_image;
  const float *bg_value;
  const float *bg_mixing_logit;
  const float *temperature_logit;
  const float *out_scale;
  int B, M, C, th, tw, H, W;
  int template_repeat; /* > 1: templates is (B / template_repeat, M, C, th, tw) and images
                          r*k .. r*k + r-1 share template set k (forward only) */
} scae_decoder_desc;

/* materialise transformed_templates (B,K,C,H,W) and mixing_logits
 * (B,K,Cm,H,W): part_decoder.py:174-231. */
int scae_template_render_fwd_f32(const scae_decoder_desc *d,
                                 float *transformed_templates,
                                 float *mixing_logits, void *stream);

/* fused path: log_prob (B,C,H,W) of image x (B,C,H,W) under the mixture,
 * straight from the compact decoder inputs (nothing (B,K,..)-sized touches
 * HBM).  lse_post (B,C,H,W) and lse_prior (B,Cm,H,W) are saved for the
 * backward pass; log_prob = lse_post - lse_prior. */
int scae_render_gmm_logprob_fwd_f32(const scae_decoder_desc *d, const float *x,
                                    float *log_prob, float *lse_post,
                                    float *lse_prior, void *stream);

/* backward of either path.
 *   fused (g_tt == NULL): g_logprob (B,C,H,W) with x / lse_post / lse_prior of
 *     the forward;
 *   materialised (g_tt != NULL): g_tt (B,K,C,H,W), g_ml (B,K,Cm,H,W) (either
 *     may be NULL = zero, not both) -- x, lse_*, g_logprob ignored.
 * outputs: g_templates (B,M,C,th,tw), g_alpha_partial (B,M,th,tw) (alpha mode;
 *   caller sums over B), g_pose (B,M,6), g_presence (B,M) (nullable),
 *   g_bg_image (B,C,H,W) (nullable),
 *   g_scalar_partial (B,K,4): per-(b,k) partial grads of [bg_value,
 *   bg_mixing_logit, temperature_logit, out_scale] with the sigmoid/softplus
 *   chain already applied (caller sums over (B,K)). */
int scae_render_gmm_bwd_f32(const scae_decoder_desc *d, const float *x,
                            const float *lse_post, const float *lse_prior,
                            const float *g_logprob, const float *g_tt,
                            const float *g_ml, float *g_templates,
                            float *g_alpha_partial, float *g_pose,
                            float *g_presence, float *g_bg_image,
                            float *g_scalar_partial, void *stream);
/* Tile-sum variant for the training loss (stacked_capsule_auto_encoder.py:222-224
 * only ever needs rec_ll = mean_b sum_{c,h,w} log_prob): the forward emits one
 * partial sum per (image, pixel tile) -- tile_sums (B, scae_render_gmm_logprob_tiles(d)),
 * summed in a fixed order -- instead of the per-pixel map, and the backward
 * takes the gradient of those sums (B, tiles). */
int scae_render_gmm_logprob_tiles(const scae_decoder_desc *d);
int scae_render_gmm_logprob_sums_fwd_f32(const scae_decoder_desc *d, const float *x,
                                         float *tile_sums, float *lse_post, float *lse_prior,
                                         void *stream);
int scae_render_gmm_sums_bwd_f32(const scae_decoder_desc *d, const float *x,
                                 const float *lse_post, const float *lse_prior,
                                 const float *g_tile_sums, float *g_templates,
                                 float *g_alpha_partial, float *g_pose, float *g_presence,
                                 float *g_bg_image, float *g_scalar_partial, void *stream);
/* Which kernel form the K1 entry points take for `d` (host only, launches nothing; the
 * launchers' own predicates).  fused: the backward gets the gradient of log_prob or of its
 * tile sums (scae_render_gmm_bwd_f32 without g_tt / g_ml, scae_render_gmm_sums_bwd_f32), not
 * of the materialised tensors; tt / ml: the addresses scae_template_render_fwd_f32 would
 * write (their alignment picks its form).
 *   out[0] likelihood forward: SCAE_K1_FWD_*      out[1] its lanes per pixel (KSPLIT)
 *   out[2] classic forward: 1 = zero-padded planes out[3] render: SCAE_K1_RENDER_*
 *   out[4] backward: SCAE_K1_BWD_*                out[5] gather: image rows per pass
 *   out[6] cell-gather: image rows per chunk      out[7] pixels per forward tile
 *   out[8] cell-gather: (cell, row slice) items per workgroup (its budget)
 *   out[9] cell-gather: item slots in LDS -- above the budget when the template has more
 *          cells, (th + 1)(tw + 1), than the budget      out[10], out[11] 0 (reserved) */
#define SCAE_K1_FWD_WAVE 0
#define SCAE_K1_FWD_CLASSIC 1
#define SCAE_K1_RENDER_WAVE 0
#define SCAE_K1_RENDER_CLASSIC 1
#define SCAE_K1_BWD_CELL 0
#define SCAE_K1_BWD_SCATTER 1
#define SCAE_K1_BWD_GATHER 2
int scae_render_gmm_forms(const scae_decoder_desc *d, int fused, const void *tt,
                          const void *ml, int out[12]);


/* scae_set_encoder_fwd_f32 and scae_render_gmm_logprob_sums_fwd_f32 as ONE launch:
 * the two forward kernels are independent -- both only read the part encoder's outputs
 * (stacked_capsule_auto_encoder.py:105-124 and :146-162 / :220) -- and the trunk leaves three
 * quarters of the SIMDs idle, so the likelihood's workgroups ride as a second block range of
 * its launch.  Falls back to the two launches where the shapes do not fit; identical results. */
int scae_set_encoder_fwd_logprob_f32(int nseg, const float *const *seg_ptr,
                                     const int *seg_width, const int *seg_row_stride,
                                     const int64_t *seg_batch_stride, const float *presence,
                                     const float *params, float *z, float *hsave, int B, int N,
                                     int D, int Din, int Dout, int L, int layer_norm,
                                     const scae_decoder_desc *d, const float *x,
                                     float *tile_sums, float *lse_post, float *lse_prior,
                                     void *stream);

/* ... with the bf16 attention products of scae_set_encoder_fwd_bf16 in the trunk */
int scae_set_encoder_fwd_logprob_bf16(int nseg, const float *const *seg_ptr,
                                      const int *seg_width, const int *seg_row_stride,
                                      const int64_t *seg_batch_stride, const float *presence,
                                      const float *params, float *z, float *hsave, int B, int N,
                                      int D, int Din, int Dout, int L, int layer_norm,
                                      const scae_decoder_desc *d, const float *x,
                                      float *tile_sums, float *lse_post, float *lse_prior,
                                      void *stream);

/* scae_render_gmm_sums_bwd_f32 and scae_capsule_likelihood_bwd_f32 as ONE launch: both
 * backward kernels only wait for the loss tail's (stacked_capsule_auto_encoder.py:217-287)
 * and are independent of each other; the capsule likelihood's one-workgroup-per-image kernel
 * rides as the first block range of the reconstruction likelihood's launch.  `k` holds the
 * arguments of scae_capsule_likelihood_bwd_f32 (same names).  Two launches where the shapes do
 * not fit; identical results. */
typedef struct scae_likelihood_bwd_desc {
  const float *vote, *scale, *vote_presence, *dummy_vote, *x, *presence, *posterior;
  const int64_t *winner_idx;
  const float *g_lpp, *g_winner, *g_winner_presence, *g_soft_winner, *g_soft_winner_presence,
      *g_posterior, *g_mixing_log_prob, *g_mixing_logit;
  float *gvote, *gscale, *gvote_presence, *gx, *gpresence, *gdummy_partial;
  int B, O, M;
  int separate; /* 0 = one launch where the shapes fit (the production setting); != 0 forces
                   the two launches (tests, measurements) */
} scae_likelihood_bwd_desc;
int scae_render_gmm_sums_bwd_likelihood_f32(
    const scae_decoder_desc *d, const float *x, const float *lse_post, const float *lse_prior,
    const float *g_tile_sums, float *g_templates, float *g_alpha_partial, float *g_pose,
    float *g_presence, float *g_bg_image, float *g_scalar_partial,
    const scae_likelihood_bwd_desc *k, void *stream);

/* generic mixture over materialised tensors: distributions.py:34-47.
 *   loc (B,K,C,P), mixing_logits (B,K,Cm,P) with Cm in {1,C}, sigma (1) device
 *   scalar (the Normal's scale), x (B,C,P) -> log_prob (B,C,P). */
int scae_gmm_log_prob_fwd_f32(const float *loc, const float *mixing_logits,
                              const float *sigma, const float *x,
                              float *log_prob, int B, int K, int C, int Cm,
                              int64_t P, void *stream);
/* g_loc (B,K,C,P), g_ml (B,K,Cm,P), g_sigma_partial (B) (caller sums),
 * g_x (B,C,P) nullable. */
int scae_gmm_log_prob_bwd_f32(const float *loc, const float *mixing_logits,
                              const float *sigma, const float *x,
                              const float *g_logprob, float *g_loc,
                              float *g_ml, float *g_sigma_partial, float *g_x,
                              int B, int K, int C, int Cm, int64_t P,
                              void *stream);
/* mean (distributions.py:37-39) and mode (:50-77, one-hot argmax over K of
 * log_softmax(logits) [+ component log-prob at its own mean when `maximum`])
 * -> out (B,C,P).  mode: Cm == 1 with C > 1 and maximum is rejected like the
 * reference (its in-place add cannot broadcast). */
int scae_gmm_mean_f32(const float *loc, const float *mixing_logits, float *out,
                      int B, int K, int C, int Cm, int64_t P, void *stream);
int scae_gmm_mode_f32(const float *loc, const float *mixing_logits,
                      const float *sigma, float *out, int maximum, int B,
                      int K, int C, int Cm, int64_t P, void *stream);

/* distributions.py:37-39 (mean) / :50-77 (mode) of the mixture part_decoder.py:174-237 builds,
 * from the compact inputs: no (B,K,C,H,W) tensor exists.  Images [first, first + count) of
 * d->B only (the grid is sized by count).  out: (count, C, H, W) dense.  what: 0 = mode,
 * 1 = mean.  The bits are those of the materialising entry point followed by the generic
 * mode / mean over its tensors: each component's value and mixing logit in the arithmetic of
 * the render form that entry point takes for d, the first largest logit wins (mode), two-pass
 * softmax in component order (mean).  Every shape the descriptor check accepts is served: the
 * image's template planes are staged in LDS whole, or in chunks of templates (one template's
 * padded planes are at most 5 x SCAE_RENDER_MAX_TEMPLATE_ELEMS floats plus their corners,
 * 82 KB, for a one-texel-wide template: inside a CU's LDS). */
int scae_render_gmm_mode_f32(const scae_decoder_desc *d, float *out, int what, int first,
                             int count, void *stream);

/* The mixture's E-step from the compact inputs (csrc/render_gmm_parts.hip): which component owns
 * each pixel of images [first, first + count).  Per pixel p and channel c, K = M + 1 components
 * with values loc[k,c,p] and mixing logits ml[k,cm,p] in the arithmetic of
 * scae_render_gmm_mode_f32 (cm = 0 in alpha mode, c in temperature mode), sigma the Normal scale:
 *   j[k,c,p] = ml[k,cm,p] - 0.5 (x[c,p] - loc[k,c,p])^2 / sigma^2    (x null: ml[k,cm,p] alone)
 *   r[k,c,p] = softmax_k j[.,c,p]   two passes (max, then sum) in component order
 *   R[k,p]   = (1/C) sum_c r[k,c,p]
 *   part[p]  = first k with the largest R[k,p] (k = M: background),  conf[p] = R[part[p],p]
 *   mass[k]  = sum_p R[k,p]: wave sums, waves, pixel rounds and tiles each in a fixed order, no
 *              atomics -- the same bits on every run of a call (and of another slice of the
 *              batch while both take the same pixel tiling)
 *   group[p] = part_group[b, part[p]] for part[p] < M, else -1
 *   rgb[:,p] = t palette[id mod P] (id = part[p] / group[p]) with t = mean_c loc[part[p],c,p];
 *              t (1, 1, 1) on a background pixel
 * x: (B, C, H, W) or null.  part_group: (B, M) int32 or null (then group and rgb_group must be
 * null).  palette: (P, 3).  part, group: (count, H, W) int32; conf: (count, H, W); mass:
 * (count, M + 1); mass_partial: (count, tiles, M + 1) workspace, tiles from
 * scae_render_gmm_parts_geometry; rgb_part, rgb_group: (count, 3, H, W) or null.  Two launches:
 * the E-step, then the tiles' sums. */
int scae_render_gmm_parts_f32(const scae_decoder_desc *d, const float *x, const int *part_group,
                              const float *palette, int P, int *part, float *conf, float *mass,
                              float *mass_partial, int *group, float *rgb_part,
                              float *rgb_group, int first, int count, void *stream);
/* out[0..2] = {pixel tiles per image, pixels per tile, templates staged at a time} of that call
 * (and of scae_render_gmm_mode_f32) for `count` images; templates staged < d->M: chunked. */
int scae_render_gmm_parts_geometry(const scae_decoder_desc *d, int count, int *out);

/* ------------------------------------------------------------------------
 * Image sheets (csrc/image_sheet.hip): up to 4 sources (n[i], C, H, W), taken as one batch of
 * N = sum n[i] images in source order, laid into sheet (3, Hs, Ws) in one launch.
 *   N > 1: xmaps = min(nrow, N) images per row, ymaps = ceil(N / xmaps) rows, cells of
 *     (H + padding, W + padding); Hs = ymaps (H + padding) + padding, Ws = xmaps (W + padding)
 *     + padding; image k at row (k / xmaps)(H + padding) + padding, column
 *     (k % xmaps)(W + padding) + padding; everything else, cells beyond N included, is
 *     pad_value.
 *   N = 1: the image itself, Hs = H, Ws = W.
 *   C = 1 is repeated to the 3 channels, C = 3 copied; any other C is rejected.
 * src and n are host arrays of nsrc entries.
 * ------------------------------------------------------------------------ */
int scae_image_sheet_f32(int nsrc, const float *const *src, const int *n, int C, int H, int W,
                         int nrow, int padding, float pad_value, float *sheet, void *stream);

/* ------------------------------------------------------------------------
 * k-means (csrc/kmeans.hip): Lloyd iterations of n_init restarts in one grid, no float atomics.
 *   distance sum_f (x_f - c_f)^2 in f order, ties to the lowest cluster; update the mean of the
 *   assigned points (an empty cluster keeps its centroid); a restart stops when no assignment
 *   changed or after max_iter assignments -- the update of that last assignment is skipped, so
 *   centroids, labels and inertia always belong together.
 * ------------------------------------------------------------------------ */
#define SCAE_KMEANS_MAX_K 256
#define SCAE_KMEANS_MAX_F 256
#define SCAE_KMEANS_MAX_KF 16384
#define SCAE_KMEANS_STATE_INTS 4   /* per restart: done, iterations, converged, last changed */
int scae_kmeans_supported(int k, int F);
/* the workgroups per restart of an assignment launch (the partials' G) */
int scae_kmeans_groups(int64_t N, int R);
typedef struct scae_kmeans_desc {
  const float *x;        /* (N, F) */
  int64_t N;
  int F, k, R;           /* features, clusters, restarts */
  int G;                 /* scae_kmeans_groups(N, R) */
  int max_iter;
  float *centroids;      /* (R, k, F): the init in, the result out */
  int64_t *labels;       /* (R, N): -1 before the first assignment */
  float *part_sum;       /* (R, G, k F) */
  int *part_count;       /* (R, G, k) */
  int *part_changed;     /* (R, G) */
  double *part_inertia;  /* (R, G) */
  int *state;            /* R * SCAE_KMEANS_STATE_INTS + 1 zeros; the last int counts the
                          * restarts that have stopped (the host's one read per chunk) */
  double *inertia;       /* (R): of the last assignment */
} scae_kmeans_desc;
/* n_iters Lloyd iterations (two launches each: assignment, then a fixed-order reduction and
 * update); launches of a stopped restart exit at once. */
int scae_kmeans_lloyd_f32(const scae_kmeans_desc *d, int n_iters, void *stream);
/* k-means++ (D^2 sampling) of R restarts, one workgroup each: centre j of restart r takes the
 * uniform u of Philox4x32-10 keyed (seed, r) at counter (j, 0, 0, 0x4B4D5050), 24 bits -> [0, 1),
 * and picks the first point whose running D^2 sum exceeds u * total (centre 0: every weight 1).
 * centroids (R, k, F), d2 (R, N) workspace, chosen (R, k) the picked rows. */
int scae_kmeans_pp_f32(const float *x, int64_t N, int F, int k, int R, uint32_t seed,
                       float *centroids, float *d2, int64_t *chosen, void *stream);
/* nearest-centroid labels (N) of x (N, F) under centroids (k, F) */
int scae_kmeans_assign_f32(const float *x, int64_t N, int F, int k, const float *centroids,
                           int64_t *labels, void *stream);
/* table (k, ncls) += counts of (cluster_ids[n], labels[n]) pairs; pairs outside the table
 * count into *outside.  Integer atomics: any order gives the same counts. */
int scae_kmeans_contingency(const int64_t *cluster_ids, const int64_t *labels, int64_t N, int k,
                            int ncls, int *table, int *outside, void *stream);

/* ------------------------------------------------------------------------
 * Linear probe (csrc/linear_probe.hip): multinomial logistic regression with L2 on the weights
 * (not the bias) on standardised features z = (x - mean) * scale with a trailing 1, R values of
 * l2 solved side by side.  Objective per problem, V of shape (C, F + 1):
 *   J(V) = (1/N) sum_n [logsumexp_c(V_c . z_n) - V_{y_n} . z_n] + (l2/2) sum_{c, f<F} V_{c,f}^2
 * FISTA with gradient restart from the state (W, V, t): g = grad J(V); W' = V - step g; if
 * sum g (W' - W) > 0 (fp64) t = 1; t' = (1 + sqrt(1 + 4 t^2)) / 2; V = W' + ((t - 1)/t')
 * (W' - W); W = W', t = t'.  The iteration that measures max|g| <= tol ends its problem as
 * converged with W = V (the point the gradient belongs to, no step taken); a problem also ends
 * after max_iter iterations.  No float atomics, fixed-order sums.
 * ------------------------------------------------------------------------ */
#define SCAE_PROBE_MAX_F 256
#define SCAE_PROBE_MAX_C 256
#define SCAE_PROBE_MAX_CF 16384    /* C * (F + 1): one problem's V in LDS */
#define SCAE_PROBE_MAX_R 16
#define SCAE_PROBE_STATE_INTS 4    /* per problem: done, iterations, converged, restarts */
int scae_probe_supported(int F, int C, int R);
/* the row groups of the moments and gradient launches: whole 64-row tiles, a contiguous row
 * range each; a function of (N, F) alone (0 for arguments out of range) */
int scae_probe_groups(int64_t N, int F);
/* the workgroups (= cross-entropy partials) of a prediction launch over N rows */
int scae_probe_predict_blocks(int64_t N);
/* moments (F + 1, F + 1) fp64 = [x 1]^T [x 1] of x (N, F): per-group partials in part
 * (scae_probe_groups(N, F), (F + 1)^2), added in group order.  With y, *outside += the labels
 * outside [0, C) (an integer count). */
int scae_probe_moments_f64(const float *x, const int64_t *y, int64_t N, int F, int C,
                           double *part, double *moments, int *outside, void *stream);
typedef struct scae_probe_desc {
  const float *x;        /* (N, F) raw features */
  const int64_t *y;      /* (N) labels in [0, C) */
  int64_t N;
  int F, C, R;           /* features, classes, problems */
  int G;                 /* scae_probe_groups(N, F) */
  int max_iter;
  const float *mean;     /* (F) */
  const float *scale;    /* (F): 1 / standard deviation, 0 for a constant column */
  const double *l2;      /* (R) */
  const double *step;    /* (R): 1 / L */
  const double *tol;     /* (R) */
  float *W, *V;          /* (R, C, F + 1): the state in, the result out */
  float *grad;           /* (R, C, F + 1): grad J(V) of the last iteration */
  double *t;             /* (R): the momentum scalar, 1 at the start */
  float *part_grad;      /* (R, G, C (F + 1)) */
  double *part_loss;     /* (R, G) */
  double *history;       /* (R, max_iter, 3): J(V), max|g|, restarted, one row per iteration */
  int *state;            /* R * SCAE_PROBE_STATE_INTS + 1 zeros; the last int counts the
                          * problems that have stopped (the host's one read per chunk) */
} scae_probe_desc;
/* n_iters iterations of every running problem, two launches each: the gradient partials of
 * all problems from one pass over x, then per problem the fixed-order reduction, the update,
 * a history row and the stop decision.  A stopped problem's state is left untouched. */
int scae_probe_fit_f32(const scae_probe_desc *d, int n_iters, void *stream);
/* pred (N) = arg max_c of weight (C, F) . x + bias (C), ties to the lowest class; log_prob (N)
 * the row's log-probability of that class.  With y: *mean_ce = the fp64 mean of the rows'
 * cross-entropy, from part_ce (scae_probe_predict_blocks(N)) partials added in block order. */
int scae_probe_predict_f32(const float *x, int64_t N, int F, int C, const float *weight,
                           const float *bias, const int64_t *y, int64_t *pred, float *log_prob,
                           double *part_ce, double *mean_ce, void *stream);

/* ------------------------------------------------------------------------
 * t-SNE (csrc/tsne.hip): exact 2-D t-SNE of x (N, F) -- dense joint affinities P (N, N) from a
 * per-row bandwidth search, then gradient iterations with gains and momentum.  No float
 * atomics, every sum in a fixed order: two runs give the same bits.
 *   d_ij = sum_f (x_if - x_jf)^2 in f order.  For j != i p_{j|i} = e_j / S with
 *   e_j = exp(-beta_i (d_ij - min_{k != i} d_ik)), S = sum_j e_j; beta_i by bisection on
 *   H = log S + beta sum_j (d e) / S from beta = 1, both bounds open (double / halve while the
 *   side is open, else the midpoint), until |H - log(perplexity)| <= 1e-5 or 100 evaluations.
 *   P_ij = (p_{j|i} + p_{i|j}) / (2 N), P_ii = 0: symmetric bit for bit.
 *   q_ij = 1 / (1 + |y_i - y_j|^2), q_ii = 0; Z = sum q (fp64 over the rows' sums);
 *   g_i = 4 (exaggeration sum_j P_ij q_ij (y_i - y_j) - (1/Z) sum_j q_ij^2 (y_i - y_j));
 *   per coordinate gain = max(g velocity < 0 ? gain + 0.2 : gain * 0.8, 0.01),
 *   velocity = momentum velocity - learning_rate gain g, y += velocity; then Y loses its column
 *   means (fp64 sums).  Iteration it < exaggeration_iter runs with early_exaggeration and
 *   momentum 0.5, a later one with exaggeration 1 and momentum 0.8.
 *   KL = sum P log P + sum_ij P_ij log1p(|y_i - y_j|^2) + log Z (fp64 over the rows' sums).
 * ------------------------------------------------------------------------ */
#define SCAE_TSNE_MAX_N 32768      /* one row of fp32 distances (128 KiB) in a CU's LDS */
#define SCAE_TSNE_MAX_F 256
#define SCAE_TSNE_HISTORY_COLS 3   /* iteration, KL, the gradient's 2-norm */
#define SCAE_TSNE_BLOCK_DOUBLES 640   /* the update launches' per-workgroup partials */
/* 1 for 2 <= N <= SCAE_TSNE_MAX_N and 1 <= F <= SCAE_TSNE_MAX_F, else 0 */
int scae_tsne_supported(int N, int F);
/* the column groups of a gradient launch (the partials' G): 256 columns each up to N = 2048,
 * 1024 above, so that the (row block, column group) grid covers the CUs from N of about 10^3
 * on; a function of N alone (0 for N out of range) */
int scae_tsne_groups(int N);
/* x (N, F) -> P (N, N), beta (N) and *plogp = the fp64 sum of P log P over P > 0, from part
 * (T (T + 1) / 2 doubles, T = ceil(N / 32): one per pair of mirrored 32 x 32 tiles) added in
 * index order.  P holds the distances, then the conditional affinities, on the way. */
int scae_tsne_affinities_f32(const float *x, int N, int F, float perplexity, float *P,
                             float *beta, double *part, double *plogp, void *stream);
typedef struct scae_tsne_desc {
  int N;
  int G;                     /* scae_tsne_groups(N) */
  int n_iter;                /* the run's length: nothing stops early */
  int exaggeration_iter;
  int check_every;
  float early_exaggeration;
  float learning_rate;
  const float *P;            /* (N, N) */
  float *Y, *velocity, *gains;   /* (N, 2): the state in, the result out */
  float *part;               /* (6, G, N): attraction (2), repulsion (2), Z, KL per column group */
  float *rows;               /* (6, N): the same, the groups added in g order */
  double *block;             /* (SCAE_TSNE_BLOCK_DOUBLES) */
  const double *plogp;       /* (1) */
  double *history;           /* (ceil(n_iter / check_every), SCAE_TSNE_HISTORY_COLS) */
} scae_tsne_desc;
/* iterations first_iter .. first_iter + n - 1, four launches each: the gradient's partials per
 * (row block, column group), the rows' sums in g order, the update, and the recentring on
 * the update's grid.  An iteration it > 0 that is a multiple of check_every also records
 * (it, KL, |g|) of the Y it starts from in history row it / check_every - 1 (its gradient
 * launch is the form that adds P log1p(d)); when first_iter + n == n_iter a last evaluation
 * without an update records (n_iter, KL, |g|) of the result in the last row.  Nothing is read
 * back: the host enqueues a whole run. */
int scae_tsne_run_f32(const scae_tsne_desc *d, int first_iter, int n, void *stream);

/* ------------------------------------------------------------------------
 * k nearest neighbours (csrc/knn.hip): the exact, brute-force search for the k nearest rows of a
 * base (Nb, F) for every query row (Nq, F), the k-NN vote on the lists, and the neighbour ranks
 * behind trustworthiness.  The result is defined by a total order, so its bits do not depend on
 * how the base is split over workgroups; no float atomics, no global atomics.
 *   d_ij = sum_f (q_if - b_jf)^2 in f order from 0, the difference, the product and the sum each
 *   rounded to fp32 (no fused multiply-add: numpy's float32 reproduces it exactly).
 *   Neighbours ascend by the pair (d_ij, j): equal distances go to the lower base index.  In
 *   self mode the base is the queries and row i is not its own neighbour.
 *   Inputs are finite (not checked).
 * ------------------------------------------------------------------------ */
#define SCAE_KNN_MAX_K 64
#define SCAE_KNN_MAX_F 256
#define SCAE_KNN_MAX_KS 8
/* 1 for 1 <= Nq, Nb < 2^31, 1 <= F <= SCAE_KNN_MAX_F and 1 <= k <= min(SCAE_KNN_MAX_K, Nb),
 * else 0 (self mode needs k <= Nb - 1 besides: scae_knn_f32 checks it) */
int scae_knn_supported(int64_t Nq, int64_t Nb, int F, int k);
/* base groups G of a search launch: a function of (Nq, Nb) alone -- enough (query tile, base
 * group) workgroups to cover the CUs when Nq is small, at least 512 base rows each, at most 64;
 * 0 for sizes out of range */
int scae_knn_groups(int64_t Nq, int64_t Nb);
/* q (Nq, F), base (Nb, F) -> d2 (Nq, k) fp32 and idx (Nq, k) int64, ascending by (d2, idx).
 * self_mode: base must be q and Nb == Nq.  part: (Nq, G, k) 64-bit words, G =
 * scae_knn_groups(Nq, Nb) -- each group's sorted list as (bits of d2) << 32 | idx, merged by a
 * second launch; with G == 1 the search writes d2 / idx itself and part may be NULL. */
int scae_knn_f32(const float *q, int64_t Nq, const float *base, int64_t Nb, int F, int k,
                 int self_mode, uint64_t *part, float *d2, int64_t *idx, void *stream);
/* The vote on neighbour lists idx / d2 (Nq, k) of a base with labels base_labels (Nb):
 * pred (Nq, n_ks) int64, column i the prediction from the first ks[i] neighbours (ks ascending,
 * ks[n_ks - 1] == k, n_ks <= SCAE_KNN_MAX_KS; a host array).  Walking the list m = 0, 1, ...:
 * w_m = 1, or with `weighted` 1 / sqrt(d2_m) (both correctly rounded) -- unless d2_0 == 0, then
 * w_m = 1 where d2_m == 0 and 0 elsewhere; the tally of neighbour m is the fp32 sum in list order
 * of w_n over n <= m with label_n == label_m, and the running best becomes (tally, label_m) when
 * the tally is greater, or equal with a lower label.  No per-class array: any int64 labels. */
int scae_knn_vote_f32(const int64_t *idx, const float *d2, int64_t Nq, int k,
                      const int64_t *base_labels, int64_t Nb, const int *ks, int n_ks,
                      int weighted, int64_t *pred, void *stream);
/* Self-mode ranks of listed neighbours: for x (N, F) and idx (N, k) (rows j != i of x; values
 * outside [0, N) are clamped into it) rank (N, k) int32 = 1 + #{ l != i : (d_il, l) < (d_ij, j) }
 * and *penalty = sum max(0, rank - k), an exact int64.  part_count: (N, G, k) int32 with G =
 * scae_knn_groups(N, N); part: ceil(N / 256) int64 per-workgroup penalties, added in index
 * order by a last launch. */
int scae_knn_ranks_f32(const float *x, int64_t N, int F, const int64_t *idx, int k, int *rank,
                       int *part_count, int64_t *part, int64_t *penalty, void *stream);

/* ------------------------------------------------------------------------
 * Sparse t-SNE (csrc/tsne_sparse.hip, the wide search in csrc/knn.hip): t-SNE past
 * SCAE_TSNE_MAX_N rows.  P lives on each row's K nearest neighbours (CSR after the
 * symmetrisation, which the caller assembles: embed.py does it with integer sorts on the
 * device); the repulsion is still exact over every pair, an N-body pass over Y with no N^2
 * memory.  The rules are the dense ones term for term, with these differences:
 *   the neighbour lists are the k-NN search's (d, j)-ordered lists in self mode;
 *   the bandwidth search runs over the row's K listed distances, shifted by the first;
 *   p_{j|i} = 0 off the list, P_ij = (p_{j|i} + p_{i|j}) / (2 N) on the union of the edges;
 *   the attraction and KL sums run over row i's stored entries in column order.
 * No float atomics, every sum in a fixed order: two runs give the same bits.
 * ------------------------------------------------------------------------ */
#define SCAE_TSNE_MAX_NEIGHBORS 128      /* the search's lists at k = 128: 144 KiB of LDS */
#define SCAE_TSNE_SPARSE_MAX_N 262144
#define SCAE_TSNE_SPARSE_BLOCK_DOUBLES 5120   /* 5 x (SCAE_TSNE_SPARSE_MAX_N / 256) partials */
/* scae_knn_f32 in self mode for 1 <= k <= min(SCAE_TSNE_MAX_NEIGHBORS, N - 1): the same
 * kernels, the same lists (part as there: (N, G, k) words with G = scae_knn_groups(N, N)) */
int scae_knn_wide_f32(const float *x, int64_t N, int F, int k, uint64_t *part, float *d2,
                      int64_t *idx, void *stream);
/* 1 for 2 <= N <= SCAE_TSNE_SPARSE_MAX_N, 1 <= F <= SCAE_TSNE_MAX_F and
 * 1 <= K <= min(SCAE_TSNE_MAX_NEIGHBORS, N - 1), else 0 */
int scae_tsne_sparse_supported(int N, int F, int K);
/* the column groups of a repulsion launch (the partials' G): a function of N alone -- about
 * 1024 (512-row block, column group) workgroups, whole 512-column tiles each, at most 64; 0 for
 * N out of range */
int scae_tsne_sparse_groups(int N);
/* d2 (N, K), a row ascending (the search's lists) -> beta (N) and the conditional rows cond
 * (N, K): p_{j|i} of the listed neighbours.  One row per wave, two entries per lane. */
int scae_tsne_knn_bandwidths_f32(const float *d2, int N, int K, float perplexity, float *cond,
                                 float *beta, void *stream);
typedef struct scae_tsne_sparse_desc {
  int N;
  int G;                     /* scae_tsne_sparse_groups(N) */
  int n_iter;
  int exaggeration_iter;
  int check_every;
  float early_exaggeration;
  float learning_rate;
  const int64_t *indptr;     /* (N + 1): CSR of the joint affinities, */
  const int *cols;           /* (nnz) a row's columns ascending, no diagonal, */
  const float *vals;         /* (nnz) symmetric */
  int64_t nnz;
  float *Y, *velocity, *gains;   /* (N, 2): the state in, the result out */
  float *part;               /* (3, G, N): repulsion (2) and Z per column group */
  float *rows;               /* (6, N): attraction (2), repulsion (2), Z, KL */
  double *block;             /* (SCAE_TSNE_SPARSE_BLOCK_DOUBLES) */
  const double *plogp;       /* (1) */
  double *history;           /* (ceil(n_iter / check_every), SCAE_TSNE_HISTORY_COLS) */
} scae_tsne_sparse_desc;
/* scae_tsne_run_f32 for the sparse form, five launches an iteration: the attraction (a CSR row
 * per wave; the recorded iterations' form adds P log1p(d)), the repulsion's partials per (row
 * block, column group), the rows' sums in g order, the update, the recentring.  The same
 * schedule, history rows and final evaluation; nothing is read back. */
int scae_tsne_sparse_run_f32(const scae_tsne_sparse_desc *d, int first_iter, int n, void *stream);

/* ------------------------------------------------------------------------
 * Cluster quality (csrc/cluster_quality.hip): the exact silhouette of a labelling of x (N, F) and
 * the per-cluster tables behind the Calinski-Harabasz and Davies-Bouldin indices.  No float
 * atomics, every sum in a fixed order that no launch geometry changes: two runs give the same
 * bits.  The caller sorts the rows by (label, row) with a stable integer sort: xs (N, F) the
 * sorted rows, ls (N) their clusters, order (N) their original rows, off (k + 1) the clusters'
 * first positions (cluster_quality.py does it on the device).
 *   d_ij = sqrt(sum_f (x_if - x_jf)^2): the squared distance by the k-NN search's rule (f order,
 *   the difference, the product and the sum each rounded to fp32, no fused multiply-add), the
 *   correctly rounded fp32 root, then widened to fp64.
 *   D_i(c) = the fp64 sum of d_ij over cluster c's rows j != i in ascending row order;
 *   a_i = D_i(c(i)) / (n_c(i) - 1); b_i = min over non-empty c != c(i) of D_i(c) / n_c, nearest_i
 *   the lowest c that attains it; s_i = (b_i - a_i) / max(a_i, b_i).  s_i = 0 when n_c(i) = 1
 *   (then a_i = 0), when no other cluster is non-empty (then b_i = +inf, nearest_i = -1) or when
 *   max(a_i, b_i) = 0.  The self pair is skipped by row, not by d = 0.
 * ------------------------------------------------------------------------ */
#define SCAE_CLUSTER_QUALITY_MAX_F 256
/* 1 for 1 <= N < 2^31, 1 <= F <= SCAE_CLUSTER_QUALITY_MAX_F and 1 <= k < 2^31 - 1, else 0 */
int scae_cluster_quality_supported(int64_t N, int F, int64_t k);
/* labels (N) int64 -> lab32 (N) int32 clamped into [0, k); *outside (zeroed by the caller) counts
 * the labels that were outside */
int scae_cluster_quality_labels(const int64_t *labels, int64_t N, int64_t k, int *lab32,
                                int *outside, void *stream);
/* -> values, a, b (N) fp64 and nearest (N) int64 in the original row order, sorted_values (N)
 * the values in sorted order (workspace), scores (k + 1): the mean of each cluster's values (the
 * fp64 sum in row order over n_c; NaN for an empty cluster) and, last, the mean of all values
 * (the fp64 sum in row order over N).  One row per lane, the sorted rows streamed through LDS;
 * a second launch for the scores. */
int scae_cluster_quality_silhouette_f32(const float *xs, const int *ls, const int64_t *off,
                                        const int64_t *order, int64_t N, int F, int64_t k,
                                        double *values, double *a, double *b, int64_t *nearest,
                                        double *sorted_values, double *scores, void *stream);
/* -> table (k, F + 3) fp64, row c = (n_c, the mean m_c (F), W_c = sum |x_i - m_c|^2,
 * S_c = the mean of |x_i - m_c|), fp64 sums in a fixed order; an empty cluster's row is
 * (0, NaN.., 0, NaN).  One workgroup per cluster. */
int scae_cluster_quality_dispersion_f32(const float *xs, const int64_t *off, int64_t N, int F,
                                        int64_t k, double *table, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SCAE_HIP_H */
