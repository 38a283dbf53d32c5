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
// The training log (scae_train_log_desc) shares (b) and (c) (loss_tail_dev.h); its epilogue
// rides in the training step's combine workgroup (loss_tail.hip), and scae_train_log_f32
// below is that epilogue alone, for a loss computed by other launches.
#include "class_probs_dev.h"
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
  scae_eval_sink *sink;  // nullable: the feature sink whose cursor this batch advances
};

// the two heads' correct counts, complete in thread 0 (all threads must call: barrier)
template <int NT>
__device__ __forceinline__ void accuracy_counts(const EvalArgs &e, float &n_prior,
                                                float &n_post) {
  scae_tail::accuracy_counts<NT>(e.prior_prob, e.post_prob, e.label, e.B, e.ncls, n_prior,
                                 n_post);
}

// thread 0: the batch into the accumulator
__device__ __forceinline__ void accumulate(const EvalArgs &e, float loss, const float *out12,
                                           float n_prior, float n_post) {
  float acc3[3];
  batch_accuracies(e.label && e.ncls > 0, e.B, n_prior, n_post, acc3);
  accumulate_batch(e.acc, loss, out12, acc3);
  if (e.sink) scae_cp::sink_advance(e.sink, e.B);
  if (e.batch3) e.batch3[0] = acc3[0], e.batch3[1] = acc3[1], e.batch3[2] = acc3[2];
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

// the training log's epilogue for a loss, 12-vector and class probabilities of other launches
__global__ __launch_bounds__(NT_ACC) void train_log_kernel(const float *loss, const float *out12,
                                                          const float *extra2,
                                                          TrainLogArgs g) {
  train_log_epilogue<NT_ACC>(g, loss, out12, extra2);
}

// the feature sink's rows of a batch and the cursor's advance, one workgroup: thread i takes
// (image, capsule) pairs i, i + NT_ACC, ..., the mass summed as scae_cp::body sums it
__global__ __launch_bounds__(NT_ACC) void eval_features_kernel(const float *cp,
                                                              const float *posterior, int B,
                                                              int O, int M,
                                                              scae_eval_sink *sink) {
  for (int i = threadIdx.x; i < B * O; i += NT_ACC) {
    const int b = i / O, o = i - b * O;
    const float *p = posterior + ((size_t)b * (O + 1) + o) * M;
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
    int m = 0;
    for (; m + 4 <= M; m += 4) m0 += p[m], m1 += p[m + 1], m2 += p[m + 2], m3 += p[m + 3];
    for (; m < M; ++m) m0 += p[m];
    scae_cp::sink_store(sink, b, O, o, cp[(size_t)b * O + o], (m0 + m1) + (m2 + m3));
  }
  __syncthreads();  // every thread has read the cursor
  if (threadIdx.x == 0) scae_cp::sink_advance(sink, B);
}

int fill_eval(EvalArgs &e, const float *prior_prob, const float *post_prob,
              const int64_t *label, int B, int ncls, double *acc, float *batch3) {
  if (!acc || B <= 0 || ncls < 0) return SCAE_ERR_BAD_ARG;
  if (label && (ncls <= 0 || !prior_prob || !post_prob)) return SCAE_ERR_BAD_ARG;
  e = EvalArgs{prior_prob, post_prob, label, B, ncls, acc, batch3, nullptr};
  return SCAE_OK;
}
}  // namespace

extern "C" int scae_eval_tail_sink_f32(const float *lpp, const float *posterior,
                                       const float *caps_presence, const float *cls_w,
                                       const float *cls_b, const int64_t *label,
                                       const scae_loss_extras *extras, float *out12,
                                       float *workspace, int B, int O, int M, int ncls,
                                       int n_classes_cfg, int prior_type, int post_type,
                                       int sparsity_on, const float *weights5,
                                       float within_const, const float *prior_prob,
                                       const float *post_prob, double *acc, float *batch3,
                                       scae_eval_sink *sink, void *stream) {
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
  e.sink = sink;
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

extern "C" int scae_eval_tail_f32(const float *lpp, const float *posterior,
                                  const float *caps_presence, const float *cls_w,
                                  const float *cls_b, const int64_t *label,
                                  const scae_loss_extras *extras, float *out12, float *workspace,
                                  int B, int O, int M, int ncls, int n_classes_cfg,
                                  int prior_type, int post_type, int sparsity_on,
                                  const float *weights5, float within_const,
                                  const float *prior_prob, const float *post_prob, double *acc,
                                  float *batch3, void *stream) {
  return scae_eval_tail_sink_f32(lpp, posterior, caps_presence, cls_w, cls_b, label, extras,
                                 out12, workspace, B, O, M, ncls, n_classes_cfg, prior_type,
                                 post_type, sparsity_on, weights5, within_const, prior_prob,
                                 post_prob, acc, batch3, nullptr, stream);
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

extern "C" int scae_eval_features_f32(const float *caps_presence, const float *posterior,
                                      int B, int O, int M, scae_eval_sink *sink,
                                      void *stream) {
  SCAE_REQUIRE(caps_presence && posterior && sink && B > 0 && O > 0 && M > 0);
  scae::launch(eval_features_kernel, dim3(1), dim3(NT_ACC), 0, (hipStream_t)stream,
               caps_presence, posterior, B, O, M, sink);
  return scae_launch_status();
}

extern "C" int scae_train_log_f32(const float *loss, const float *out12, const float *extra2,
                                  const scae_train_log_desc *log, int B, void *stream) {
  SCAE_REQUIRE(loss && log);
  TrainLogArgs g;
  const int rc = fill_train_log(g, *log, B);
  if (rc) return rc;
  scae::launch(train_log_kernel, dim3(1), dim3(NT_ACC), 0, (hipStream_t)stream, loss, out12,
               extra2, g);
  return scae_launch_status();
}
