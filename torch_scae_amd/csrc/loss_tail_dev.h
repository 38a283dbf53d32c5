// Batch combine of the loss tail (loss_tail.hip), shared with the evaluation epilogue
// (eval_tail.hip): the argument block, the workspace layout and the one-workgroup body
// that forms the batch sums, the between-example terms, the training scalar and the
// 12-vector.  One copy, so both kernels give the same bits for the same inputs.
#pragma once
#include "common.h"

namespace scae_tail {
constexpr int NTI = 64;    // tail_image_kernel: one wave per image
// Workgroup sizes of the combine (ONE workgroup: its batch / column sums are chains of L2
// loads, more waves keep more of them in flight) and of the backward: at small batches
// (scae_loss_tail_defer_preferred) both run NT_SMALL threads, so that the combine can be a
// workgroup of the backward launch and an image's workgroup can form the column sums
// exactly as the combine does; at large batches 1024 and 256 (measured best at B = 1024).
// (A 1024-thread form of the small-batch backward took 16 us instead of 10.)
constexpr int NT_SMALL = 512, NTC_LARGE = 1024, NTB_LARGE = 256;

struct TailArgs {
  const float *lpp;        // (B,M)   log_prob_per_point
  const float *posterior;  // (B,O+1,M)
  const float *cp;         // (B,O)   caps_presence
  const float *cls_w;      // (ncls,O) nullable
  const float *cls_b;      // (ncls)
  const int64_t *label;    // (B) nullable
  int B, O, M, ncls;
  int prior_type, post_type;  // 0 l2, 1 entropy, 2 kl
  int sparsity_on;            // reference gate: prior weights > 0
  float w_ll, w_pw, w_pb, w_qw, w_qb;  // loss weights
  float l2_within_const, l2_between_const, l2_within_const_post, l2_between_const_post;
};

// workspace (floats): part (B,8) | mass (B,O) | gl (B,2,ncls) | col (2,O)
//   part[b] = {sum_m lpp, prior within_b, posterior within_b, prior xe_b,
//              posterior xe_b, row sum of caps_presence, row sum of mass / M, -}
//   mass[b][o] = sum_m posterior[b,o,m]  (un-normalised)
//   gl[b][which][c] = d xe_b / d logit_c (which: 0 prior, 1 posterior input)
//   col[0][o] = sum_b caps_presence, col[1][o] = sum_b mass / M
struct Ws {
  float *part, *mass, *gl, *col;
};
__host__ __device__ inline Ws carve_ws(float *w, int B, int O, int ncls) {
  Ws s;
  s.part = w;
  s.mass = s.part + (size_t)B * 8;
  s.gl = s.mass + (size_t)B * O;
  s.col = s.gl + (size_t)B * 2 * (ncls > 0 ? ncls : 1);
  return s;
}
inline size_t ws_floats(int B, int O, int ncls) {
  return (size_t)B * 8 + (size_t)B * O + (size_t)B * 2 * (ncls > 0 ? ncls : 1) + 2 * (size_t)O;
}

// -sum p log_safe(p*k) terms: value
__device__ __forceinline__ float ent_term(float p, float k) {
  return -p * scae::log_safe(p * k);
}
// between-example term from the column sums in LDS (first wave; result in all lanes)
__device__ __forceinline__ float between_term(const float *col, int O, int type, float cb,
                                              int lane) {
  float t = 0.f;
  if (type == 0) {
    for (int o = lane; o < O; o += 64) t += (col[o] - cb) * (col[o] - cb);
    return scae::wave_sum(t) / O;
  }
  const float k = type == 2 ? (float)O : 1.f;
  float tot = 0.f;
  for (int o = 0; o < O; ++o) tot += col[o];
  for (int o = lane; o < O; o += 64) t += ent_term(col[o] / (tot + 1e-8f), k);
  return -scae::wave_sum(t);
}

// out: [0] loss  [1] log_prob  [2] prior_within [3] prior_between [4] post_within
//      [5] post_between [6] prior_cls_xe [7] posterior_cls_xe [8] rec_ll [9] -rec_ll
//      [10] -log_prob [11] reg
// column sums over the batch into col[2 O] (LDS; also published to ws.col when asked): 16
// lanes per column, each takes every 16th image: the summation order -- and the result, bit
// for bit -- does not depend on who forms it (nor on NTC).
template <int NTC>
__device__ __forceinline__ void column_sums(const TailArgs &a, const Ws &ws, float *col, int tid,
                                            bool publish) {
  const int B = a.B, O = a.O;
  for (int e = tid; e < ((2 * O * 16 + NTC - 1) / NTC) * NTC; e += NTC) {
    const int c = e >> 4, l = e & 15, which = c / O, o = c - which * O;
    float t = 0.f;
    if (c < 2 * O) {  // (loads kept in flight: four independent partial sums)
      auto at = [&](int b) {
        return which == 0 ? a.cp[(size_t)b * O + o] : ws.mass[(size_t)b * O + o] / a.M;
      };
      float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
      int b = l;
      for (; b + 48 < B; b += 64) {
        const float u0 = at(b), u1 = at(b + 16), u2 = at(b + 32), u3 = at(b + 48);
        t0 += u0, t1 += u1, t2 += u2, t3 += u3;
      }
      for (; b < B; b += 16) t0 += at(b);
      t = (t0 + t1) + (t2 + t3);
    }
    t = scae::row_sum16(t);
    if (c < 2 * O && l == 0) {
      col[c] = t;
      if (publish) ws.col[c] = t;
    }
  }
}

// out: [0] loss  [1] log_prob  [2] prior_within [3] prior_between [4] post_within
//      [5] post_between [6] prior_cls_xe [7] posterior_cls_xe [8] rec_ll [9] -rec_ll
//      [10] -log_prob [11] reg
template <int NTC>
__device__ __forceinline__ void combine_body(const TailArgs &a, const scae_loss_extras &x,
                                             const Ws &ws, float *out, float *smem) {
  const int B = a.B, O = a.O, tid = threadIdx.x;
  float *col = smem, *red = smem + 2 * O;  // red: 6 * (NTC/64) floats
  float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b = tid; b < B; b += NTC) {
    const float4 p = *reinterpret_cast<const float4 *>(ws.part + (size_t)b * 8);
    v[0] += p.x, v[1] += p.y, v[2] += p.z, v[3] += p.w;
    v[4] += ws.part[(size_t)b * 8 + 4];
  }
  if (x.rec_sums)
    for (int i = tid; i < x.n_rec; i += NTC) v[5] += x.rec_sums[i];
  column_sums<NTC>(a, ws, col, tid, true);
  scae::block_sum<6, NTC>(v, red);  // (contains the barriers that publish col[])
  if (tid >= 64) return;
  float pb = 0.f, qb = 0.f;
  if (a.sparsity_on) {
    pb = between_term(col, O, a.prior_type, a.l2_between_const, tid);
    qb = between_term(col + O, O, a.post_type, a.l2_between_const_post, tid);
  }
  if (tid != 0) return;
  const float log_prob = v[0] / B, pw = v[1] / B, qw = v[2] / B, xe1 = v[3] / B, xe2 = v[4] / B;
  const float rec = x.rec_sums ? v[5] / B : 0.f, reg = x.reg ? x.reg[0] : 0.f;
  out[1] = log_prob, out[2] = pw, out[3] = pb, out[4] = qw, out[5] = qb;
  out[6] = xe1, out[7] = xe2, out[8] = rec, out[9] = -rec, out[10] = -log_prob, out[11] = reg;
  const float loss = -a.w_ll * log_prob + a.w_pw * pw + a.w_pb * pb + a.w_qw * qw +
                     a.w_qb * qb + xe1 + xe2 - rec + x.w_reg * reg;
  out[0] = loss;
  if (x.loss) x.loss[0] = loss;
}

// -- accuracies and the fp64 epoch accumulator: the evaluation epilogue (eval_tail.hip) and
// the training log (scae_train_log_desc, loss_tail.hip) ------------------------------------

// torch.argmax over one row: the first maximal index; the first NaN wins.  The row is read
// 16 classes at a time, the loads of a chunk in flight together.
__device__ __forceinline__ int row_argmax(const float *p, int n) {
  float v = 0.f;
  int best = 0;
  for (int c0 = 0; c0 < n; c0 += 16) {
    float x[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = c0 + j < n ? p[c0 + j] : 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int c = c0 + j;
      if (c >= n) break;
      if (x[j] != x[j]) return c;
      if (c == 0 || x[j] > v) v = x[j], best = c;
    }
  }
  return best;
}

// the two heads' correct counts, complete in thread 0 (all threads must call: barrier)
template <int NT>
__device__ __forceinline__ void accuracy_counts(const float *prior_prob, const float *post_prob,
                                                const int64_t *label, int B, int ncls,
                                                float &n_prior, float &n_post) {
  __shared__ float red[2][NT / 64];
  float cp = 0.f, cq = 0.f;  // (integers: exact in fp32 up to 2^24 images)
  if (label && ncls > 0) {
    for (int b = threadIdx.x; b < B; b += NT) {
      const int64_t l = label[b];
      cp += row_argmax(prior_prob + (size_t)b * ncls, ncls) == l ? 1.f : 0.f;
      cq += row_argmax(post_prob + (size_t)b * ncls, ncls) == l ? 1.f : 0.f;
    }
  }
  cp = scae::wave_sum(cp);
  cq = scae::wave_sum(cq);
  const int w = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) red[0][w] = cp, red[1][w] = cq;
  __syncthreads();
  n_prior = n_post = 0.f;
  if (threadIdx.x == 0)
    for (int i = 0; i < NT / 64; ++i) n_prior += red[0][i], n_post += red[1][i];
}

// count / B per head (zero without a label) and the batch value max(prior, posterior)
__device__ __forceinline__ void batch_accuracies(bool labelled, int B, float n_prior,
                                                 float n_post, float acc3[3]) {
  float pa = 0.f, qa = 0.f;
  if (labelled) pa = n_prior / (float)B, qa = n_post / (float)B;
  acc3[0] = qa > pa ? qa : pa, acc3[1] = pa, acc3[2] = qa;
}

// one thread: the batch into an SCAE_EVAL_ACC_DOUBLES accumulator (out12 nullable: zeros)
__device__ __forceinline__ void accumulate_batch(double *A, float loss, const float *out12,
                                                 const float acc3[3]) {
  A[0] += 1.0;
  A[1] += (double)loss;
  A[2] += (double)acc3[0];
  A[3] += (double)acc3[1];
  A[4] += (double)acc3[2];
  if (out12)
    for (int i = 0; i < 12; ++i) A[5 + i] += (double)out12[i];
}

// The training log (include/scae_hip.h, scae_train_log_desc) as a kernel argument
struct TrainLogArgs {
  float *rows;                          // (capacity, SCAE_TRAIN_LOG_ROW)
  int64_t *step;                        // device step counter
  double *acc;                          // nullable
  const float *prior_prob, *post_prob;  // (B, ncls)
  const int64_t *label;                 // nullable: no accuracies
  const float *lr;                      // nullable: NaN
  int capacity, B, ncls;
};

// After the batch's loss and 12-vector exist (stores of this workgroup before a barrier, or
// another launch's): the accuracies, one row of the ring at the step counter's slot, the
// counter advanced, the batch added to the accumulator.  All threads call (barrier); the
// first wave writes, lane i the row's entry i and the accumulator's entry i -- the same fp64
// adds as accumulate_batch, with all of their loads in flight at once.
template <int NT>
__device__ __forceinline__ void train_log_epilogue(const TrainLogArgs &g, const float *loss,
                                                   const float *out12, const float *extra) {
  float n_prior, n_post;
  accuracy_counts<NT>(g.prior_prob, g.post_prob, g.label, g.B, g.ncls, n_prior, n_post);
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  n_prior = __shfl(n_prior, 0), n_post = __shfl(n_post, 0);
  float acc3[3];
  batch_accuracies(g.label && g.ncls > 0, g.B, n_prior, n_post, acc3);
  const int64_t s = g.step[0];
  const float l = loss[0];
  const float o = out12 && lane >= 4 && lane < 16 ? out12[lane - 4] : 0.f;
  const float lr = g.lr ? g.lr[0] : __builtin_nanf("");
  const float e = extra && lane >= 17 && lane < 19 ? extra[lane - 17] : 0.f;
  const double a = g.acc && lane < SCAE_EVAL_ACC_DOUBLES ? g.acc[lane] : 0.0;
  const float v = lane == 0 ? l : lane == 1 ? acc3[0] : lane == 2 ? acc3[1]
                : lane == 3 ? acc3[2] : lane < 16 ? o : lane == 16 ? lr : e;
  float *r = g.rows + (size_t)((uint64_t)s % (uint64_t)g.capacity) * SCAE_TRAIN_LOG_ROW;
  if (lane < SCAE_TRAIN_LOG_ROW) r[lane] = v;
  // the accumulator's entry i >= 1 is the row's entry i - 1: [1] loss, [2..4] accuracies,
  // [5 + i] out12[i]; [0] counts batches
  const float u = __shfl(v, lane > 0 ? lane - 1 : 0);
  if (g.acc && lane < SCAE_EVAL_ACC_DOUBLES && (lane < 5 || out12))
    g.acc[lane] = a + (lane == 0 ? 1.0 : (double)u);
  if (lane == 0) g.step[0] = s + 1;
}

// LDS of the combine workgroup (either size)
inline size_t combine_lds(int O) { return (2 * O + 6 * (NTC_LARGE / 64)) * sizeof(float); }

// TailArgs from the entry points' arguments (loss_tail.hip): SCAE_ERR_* on bad ones
int fill_tail(TailArgs &a, const float *lpp, const float *posterior, const float *cp,
              const float *cls_w, const float *cls_b, const int64_t *label, int B, int O, int M,
              int ncls, int n_classes_cfg, int prior_type, int post_type, int sparsity_on,
              const float *weights /*5*/, float within_const);
// TrainLogArgs from a descriptor (loss_tail.hip): SCAE_ERR_* on bad ones
int fill_train_log(TrainLogArgs &g, const scae_train_log_desc &d, int B);
}  // namespace scae_tail
