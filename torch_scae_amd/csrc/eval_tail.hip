// Evaluation epilogue for gfx950: the one launch that ends an evaluation batch
// (BaseExperiment.validation_step / test_step, base_experiment.py:128-202, and their
// *_epoch_end means).  One workgroup:
//   (a) the loss tail's batch combine (loss_tail_dev.h::combine_body, the code
//       tail_combine_kernel runs: the same bits for the same inputs);
//   (b) SCAE.calculate_accuracy (stacked_capsule_auto_encoder.py:289-297) from the class
//       probabilities the tail's per-image launch wrote: argmax per image and head as
//       torch.argmax (first maximal index, NaN maximal), compared with the int64 label,
//       count / B per head, the batch value max(prior, posterior);
//   (c) the batch added into a device-resident fp64 accumulator by ONE thread, in
//       stream order: no atomics, so N replays give the same epoch sums bit for bit.
// scae_eval_accumulate_f32 is (b) + (c) alone, for a loss computed by other launches.
#include "common.h"
#include "loss_tail_dev.h"

namespace {
using namespace scae_tail;

struct EvalArgs {
  const float *prior_prob, *post_prob;  // (B, ncls); unused when ncls == 0 or no label
  const int64_t *label;                 // (B) nullable: no accuracies
  int B, ncls;
  double *acc;     // SCAE_EVAL_ACC_DOUBLES
  float *batch3;   // nullable: this batch's {best, prior, posterior} accuracy
};

// torch.argmax over one row: the first maximal index; the first NaN wins
__device__ __forceinline__ int row_argmax(const float *p, int n) {
  float v = p[0];
  if (v != v) return 0;
  int best = 0;
  for (int c = 1; c < n; ++c) {
    const float x = p[c];
    if (x != x) return c;
    if (x > v) v = x, best = c;
  }
  return best;
}

// the two heads' correct counts, complete in thread 0 (all threads must call: barrier)
template <int NT>
__device__ __forceinline__ void accuracy_counts(const EvalArgs &e, float &n_prior,
                                                float &n_post) {
  __shared__ float red[2][NT / 64];
  float cp = 0.f, cq = 0.f;  // (integers: exact in fp32 up to 2^24 images)
  if (e.label && e.ncls > 0) {
    for (int b = threadIdx.x; b < e.B; b += NT) {
      const int64_t l = e.label[b];
      cp += row_argmax(e.prior_prob + (size_t)b * e.ncls, e.ncls) == l ? 1.f : 0.f;
      cq += row_argmax(e.post_prob + (size_t)b * e.ncls, e.ncls) == l ? 1.f : 0.f;
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

// thread 0: the batch into the accumulator
__device__ __forceinline__ void accumulate(const EvalArgs &e, float loss, const float *out12,
                                           float n_prior, float n_post) {
  float pa = 0.f, qa = 0.f;
  if (e.label && e.ncls > 0) pa = n_prior / (float)e.B, qa = n_post / (float)e.B;
  const float best = qa > pa ? qa : pa;
  double *A = e.acc;
  A[0] += 1.0;
  A[1] += (double)loss;
  A[2] += (double)best;
  A[3] += (double)pa;
  A[4] += (double)qa;
  if (out12)
    for (int i = 0; i < 12; ++i) A[5 + i] += (double)out12[i];
  if (e.batch3) e.batch3[0] = best, e.batch3[1] = pa, e.batch3[2] = qa;
}

template <int NTC>
__global__ __launch_bounds__(NTC) void eval_tail_kernel(TailArgs a, scae_loss_extras x, Ws ws,
                                                       float *out12, EvalArgs e) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float n_prior, n_post;
  accuracy_counts<NTC>(e, n_prior, n_post);
  combine_body<NTC>(a, x, ws, out12, smem);
  if (threadIdx.x != 0) return;
  accumulate(e, out12[0], out12, n_prior, n_post);  // (out12: this thread's own stores)
}

constexpr int NT_ACC = 256;
__global__ __launch_bounds__(NT_ACC) void eval_accumulate_kernel(const float *loss,
                                                                const float *out12, EvalArgs e) {
  float n_prior, n_post;
  accuracy_counts<NT_ACC>(e, n_prior, n_post);
  if (threadIdx.x != 0) return;
  accumulate(e, loss[0], out12, n_prior, n_post);
}

int fill_eval(EvalArgs &e, const float *prior_prob, const float *post_prob,
              const int64_t *label, int B, int ncls, double *acc, float *batch3) {
  if (!acc || B <= 0 || ncls < 0) return SCAE_ERR_BAD_ARG;
  if (label && (ncls <= 0 || !prior_prob || !post_prob)) return SCAE_ERR_BAD_ARG;
  e = EvalArgs{prior_prob, post_prob, label, B, ncls, acc, batch3};
  return SCAE_OK;
}
}  // namespace

extern "C" int scae_eval_tail_f32(const float *lpp, const float *posterior,
                                  const float *caps_presence, const float *cls_w,
                                  const float *cls_b, const int64_t *label,
                                  const scae_loss_extras *extras, float *out12, float *workspace,
                                  int B, int O, int M, int ncls, int n_classes_cfg,
                                  int prior_type, int post_type, int sparsity_on,
                                  const float *weights5, float within_const,
                                  const float *prior_prob, const float *post_prob, double *acc,
                                  float *batch3, void *stream) {
  TailArgs a;
  int rc = fill_tail(a, lpp, posterior, caps_presence, cls_w, cls_b, label, B, O, M, ncls,
                     n_classes_cfg, prior_type, post_type, sparsity_on, weights5, within_const);
  if (rc) return rc;
  SCAE_REQUIRE(out12 && workspace);
  EvalArgs e;
  rc = fill_eval(e, prior_prob, post_prob, label, B, ncls, acc, batch3);
  if (rc) return rc;
  scae_loss_extras x{};
  if (extras) x = *extras;
  if (x.rec_sums && x.n_rec <= 0) return SCAE_ERR_BAD_ARG;
  x.defer_combine = 0;
  const Ws ws = carve_ws(workspace, B, O, ncls);
  hipStream_t st = (hipStream_t)stream;
  // the combine's workgroup size as launch_combine (loss_tail.hip) picks it: the block sums'
  // order depends on it
  if (scae_loss_tail_defer_preferred(B, O))
    scae::launch(eval_tail_kernel<NT_SMALL>, dim3(1), dim3(NT_SMALL), combine_lds(O), st, a, x,
                 ws, out12, e);
  else
    scae::launch(eval_tail_kernel<NTC_LARGE>, dim3(1), dim3(NTC_LARGE), combine_lds(O), st, a,
                 x, ws, out12, e);
  return scae_launch_status();
}

extern "C" int scae_eval_accumulate_f32(const float *loss, const float *out12,
                                        const float *prior_prob, const float *post_prob,
                                        const int64_t *label, int B, int ncls, double *acc,
                                        float *batch3, void *stream) {
  SCAE_REQUIRE(loss);
  EvalArgs e;
  int rc = fill_eval(e, prior_prob, post_prob, label, B, ncls, acc, batch3);
  if (rc) return rc;
  scae::launch(eval_accumulate_kernel, dim3(1), dim3(NT_ACC), 0, (hipStream_t)stream, loss,
               out12, e);
  return scae_launch_status();
}
