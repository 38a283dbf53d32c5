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
// With evaluation records (scae_eval_records) the same workgroup first writes one row per
// image -- label, both heads' class and its probability, the label's probability, the image's
// reconstruction and capsule log-likelihoods -- and adds the batch's two confusion histograms,
// built in LDS, into the global matrix: scae_eval_tail_records_f32; (a) is untouched, (b) comes
// out of the same loop.  scae_eval_records_f32 is the records alone.
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

// ---- the evaluation records (include/scae_hip.h, scae_eval_records) ---------------------
struct RecordArgs {
  scae_eval_records *rec;
  const float *part;        // (B, 8) loss-tail workspace rows, [0] = sum_m lpp: column [8]
  const float *lpp;         // (B, M): column [8] by records_wave_sums instead
  const float *rec_sums;    // (B, n_rec) tile sums: column [7], added in tile order
  const float *rec_pixels;  // (B, n_rec) per-pixel map: column [7] by records_wave_sums
  int M, n_rec;
};
constexpr int NT_REC = 512;
constexpr int REC_ROW = SCAE_EVAL_RECORD_FLOATS;

// LDS of the records (ints) behind the combine's: the accuracy counts' scratch, then the
// batch's two ncls x ncls histograms
inline size_t records_lds_offset(int O) { return (combine_lds(O) + 15) / 16 * 16; }
inline size_t records_lds(int ncls) {
  return (2 * (NTC_LARGE / 64) + 2 * (size_t)ncls * ncls) * sizeof(int);
}

// Columns [7] / [8] from per-element maps, one wave per image: lpp as tail_image_kernel sums
// it (lane-strided, then wave_sum: the same bits), a per-pixel map with four loads in flight.
template <int NT>
__device__ __forceinline__ void records_wave_sums(const RecordArgs &r, int B) {
  const int64_t cap = r.rec->capacity, cursor = r.rec->cursor;
  const int lane = threadIdx.x & 63;
  for (int b = threadIdx.x >> 6; b < B; b += NT / 64) {  // (wave-uniform)
    if (cursor + b >= cap) break;
    float lp = 0.f, rl = 0.f;
    if (r.lpp) {
      for (int m = lane; m < r.M; m += 64) lp += r.lpp[(size_t)b * r.M + m];
      lp = scae::wave_sum(lp);
    }
    if (r.rec_pixels) {
      const float *p = r.rec_pixels + (size_t)b * r.n_rec;
      float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
      int i = lane;
      for (; i + 192 < r.n_rec; i += 256)
        t0 += p[i], t1 += p[i + 64], t2 += p[i + 128], t3 += p[i + 192];
      for (; i < r.n_rec; i += 64) t0 += p[i];
      rl = scae::wave_sum((t0 + t1) + (t2 + t3));
    }
    if (lane == 0) {
      float *row = r.rec->rows + (size_t)(cursor + b) * REC_ROW;
      row[8] = lp;
      if (!r.rec_sums) row[7] = rl;
    }
  }
}

// The batch's rows and confusion counts, and the two heads' correct counts as
// accuracy_counts forms them (integers: the same values), complete in thread 0.  All threads
// call (barriers).  lds: 2 * (NT / 64) + 2 * ncls^2 ints.  The cursor is read here by every
// thread and advanced by records_advance after a later barrier.
template <int NT>
__device__ __forceinline__ void records_body(const EvalArgs &e, const RecordArgs &r, int *lds,
                                             float &n_prior, float &n_post) {
  const int tid = threadIdx.x, B = e.B, ncls = e.ncls;
  scae_eval_records *k = r.rec;
  const int64_t cap = k->capacity, cursor = k->cursor;
  const bool labelled = e.label && k->labelled;
  const bool counting = cap > 0 && labelled && ncls > 0 && k->confusion && k->ncls == ncls;
  const int cells = counting ? 2 * ncls * ncls : 0;
  int *red = lds, *hist = lds + 2 * (NT / 64);
  for (int i = tid; i < cells; i += NT) hist[i] = 0;
  __syncthreads();
  int cp = 0, cq = 0;
  for (int b = tid; b < B; b += NT) {
    const int64_t l = e.label ? e.label[b] : -1;
    int pc = -1, qc = -1;
    float pconf = 0.f, qconf = 0.f, pl = 0.f, ql = 0.f;
    const bool row_on = cursor + b < cap;
    if (ncls > 0) {
      const float *pp = e.prior_prob + (size_t)b * ncls, *qp = e.post_prob + (size_t)b * ncls;
      pc = row_argmax(pp, ncls), qc = row_argmax(qp, ncls);
      pconf = pp[pc], qconf = qp[qc];
      if (e.label) cp += pc == l, cq += qc == l;
      if (labelled && l >= 0 && l < ncls) {
        pl = pp[l], ql = qp[l];
        if (counting && row_on) {
          atomicAdd(&hist[(int)l * ncls + pc], 1);
          atomicAdd(&hist[(ncls + (int)l) * ncls + qc], 1);
        }
      }
    }
    if (!row_on) continue;
    float *row = k->rows + (size_t)(cursor + b) * REC_ROW;
    row[0] = labelled ? (float)l : -1.f;
    row[1] = (float)pc, row[2] = (float)qc, row[3] = pconf, row[4] = qconf;
    row[5] = pl, row[6] = ql;
    if (r.rec_sums) {
      float rl = 0.f;
      for (int t = 0; t < r.n_rec; ++t) rl += r.rec_sums[(size_t)b * r.n_rec + t];
      row[7] = rl;
    } else if (!r.rec_pixels) {
      row[7] = 0.f;
    }
    if (r.part) row[8] = r.part[(size_t)b * 8];
  }
  for (int o = 32; o > 0; o >>= 1) cp += __shfl_xor(cp, o), cq += __shfl_xor(cq, o);
  if ((tid & 63) == 0) red[tid >> 6] = cp, red[NT / 64 + (tid >> 6)] = cq;
  __syncthreads();  // (also: the histograms are complete)
  n_prior = n_post = 0.f;
  if (tid == 0) {
    int np = 0, nq = 0;
    for (int i = 0; i < NT / 64; ++i) np += red[i], nq += red[NT / 64 + i];
    n_prior = (float)np, n_post = (float)nq;
  }
  // one writer per cell, in stream order: no global atomics
  for (int i = tid; i < cells; i += NT) {
    const int h = hist[i];
    if (h) k->confusion[i] += (int64_t)h;
  }
}

// thread 0, after a barrier that follows records_body: rows [cursor, cursor + B) are done
__device__ __forceinline__ void records_advance(scae_eval_records *k, int B) {
  const int64_t cap = k->capacity;
  if (cap <= 0) return;
  const int64_t end = k->cursor + B;
  if (end > cap) k->overflow = 1;
  k->cursor = end;
}

// eval_tail_kernel with the records: rows and counts first (LDS behind the combine's), the
// combine untouched, the cursors last
template <int NTC>
__global__ __launch_bounds__(NTC) void eval_tail_records_kernel(TailArgs a, scae_loss_extras x,
                                                               Ws ws, float *out12, EvalArgs e,
                                                               RecordArgs r, int lds_offset) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float n_prior, n_post;
  records_body<NTC>(e, r, reinterpret_cast<int *>(smem) + lds_offset / 4, n_prior, n_post);
  combine_body<NTC>(a, x, ws, out12, smem);  // (its barriers: every thread has read the cursor)
  if (threadIdx.x != 0) return;
  accumulate(e, out12[0], out12, n_prior, n_post);
  records_advance(r.rec, e.B);
}

__global__ __launch_bounds__(NT_REC) void eval_records_kernel(EvalArgs e, RecordArgs r) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float n_prior, n_post;
  if (r.rec->capacity > 0) records_wave_sums<NT_REC>(r, e.B);
  records_body<NT_REC>(e, r, reinterpret_cast<int *>(smem), n_prior, n_post);
  __syncthreads();  // every thread has read the cursor
  if (threadIdx.x == 0) records_advance(r.rec, e.B);
}
}  // namespace

extern "C" int scae_eval_tail_records_f32(
    const float *lpp, const float *posterior, const float *caps_presence, const float *cls_w,
    const float *cls_b, const int64_t *label, const scae_loss_extras *extras, float *out12,
    float *workspace, int B, int O, int M, int ncls, int n_classes_cfg, int prior_type,
    int post_type, int sparsity_on, const float *weights5, float within_const,
    const float *prior_prob, const float *post_prob, double *acc, float *batch3,
    scae_eval_sink *sink, scae_eval_records *records, void *stream) {
  if (!records)
    return scae_eval_tail_sink_f32(lpp, posterior, caps_presence, cls_w, cls_b, label, extras,
                                   out12, workspace, B, O, M, ncls, n_classes_cfg, prior_type,
                                   post_type, sparsity_on, weights5, within_const, prior_prob,
                                   post_prob, acc, batch3, sink, stream);
  TailArgs a;
  int rc = fill_tail(a, lpp, posterior, caps_presence, cls_w, cls_b, label, B, O, M, ncls,
                     n_classes_cfg, prior_type, post_type, sparsity_on, weights5, within_const);
  if (rc) return rc;
  SCAE_REQUIRE(out12 && workspace);
  EvalArgs e;
  rc = fill_eval(e, prior_prob, post_prob, label, B, ncls, acc, batch3);
  if (rc) return rc;
  SCAE_REQUIRE(ncls == 0 || (prior_prob && post_prob));
  if (ncls > SCAE_EVAL_RECORDS_MAX_CLASSES) return SCAE_ERR_UNSUPPORTED;
  scae_loss_extras x{};
  if (extras) x = *extras;
  if (x.rec_sums && (x.n_rec <= 0 || x.n_rec % B)) return SCAE_ERR_BAD_ARG;
  x.defer_combine = 0;
  e.sink = sink;
  const Ws ws = carve_ws(workspace, B, O, ncls);
  const RecordArgs r{records, ws.part, nullptr, x.rec_sums, nullptr, M, x.n_rec / B};
  const int off = (int)records_lds_offset(O);
  const size_t lds = off + records_lds(ncls);
  hipStream_t st = (hipStream_t)stream;
  if (scae_loss_tail_defer_preferred(B, O))
    scae::launch(eval_tail_records_kernel<NT_SMALL>, dim3(1), dim3(NT_SMALL), lds, st, a, x, ws,
                 out12, e, r, off);
  else
    scae::launch(eval_tail_records_kernel<NTC_LARGE>, dim3(1), dim3(NTC_LARGE), lds, st, a, x,
                 ws, out12, e, r, off);
  return scae_launch_status();
}

extern "C" int scae_eval_records_f32(const float *prior_prob, const float *post_prob,
                                     const int64_t *label, const float *lpp,
                                     const float *rec_sums, const float *rec_pixels, int B,
                                     int ncls, int M, int n_rec, scae_eval_records *records,
                                     void *stream) {
  SCAE_REQUIRE(records && B > 0 && ncls >= 0);
  SCAE_REQUIRE(ncls == 0 || (prior_prob && post_prob));
  SCAE_REQUIRE(!lpp || M > 0);
  SCAE_REQUIRE(!(rec_sums || rec_pixels) || n_rec > 0);
  if (ncls > SCAE_EVAL_RECORDS_MAX_CLASSES) return SCAE_ERR_UNSUPPORTED;
  const EvalArgs e{prior_prob, post_prob, label, B, ncls, nullptr, nullptr, nullptr};
  const RecordArgs r{records, nullptr, lpp, rec_sums, rec_sums ? nullptr : rec_pixels, M, n_rec};
  scae::launch(eval_records_kernel, dim3(1), dim3(NT_REC), records_lds(ncls),
               (hipStream_t)stream, e, r);
  return scae_launch_status();
}

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
