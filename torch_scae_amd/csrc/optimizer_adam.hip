// Adam and RAdam on the flat parameter buffers, with LookAhead fused into the same pass -- the
// reference's other two optimisers (base_experiment.py:44-77: torch.optim.Adam and
// torch_scae/optimizers.py's RAdam, optionally wrapped in its LookAhead) as one pass over
// (param, grad, exp_avg, exp_avg_sq[, slow]) each, laid out as optimizer.hip's RMSprop pass.
// RMSprop wrapped in LookAhead runs here too (the arithmetic of optimizer.hip's update(), with
// momentum_buffer and square_avg in the places of exp_avg and exp_avg_sq); plain RMSprop keeps
// optimizer.hip's kernels.
//   Adam (torch.optim.Adam, coupled L2 decay):  g <- g + wd p
//     m <- m + (1-b1)(g - m);  v <- b2 v + (1-b2) g^2
//     p <- p - (lr / (1-b1^t)) m / (sqrt(v) / sqrt(1-b2^t) + eps)
//   RAdam (optimizers.py:36-102, degenerated_to_sgd): decoupled decay p <- p - wd lr p first;
//     v <- b2 v + (1-b2) g^2;  m <- b1 m + (1-b1) g
//     N_sma >= 5: p <- p - lr rect(t) sqrt(1-b2^t)/(1-b1^t) m / (sqrt(v) + eps)
//     otherwise:  p <- p - lr/(1-b1^t) m                      (SGD with momentum)
//   LookAhead (optimizers.py:105-190) on every k-th step, after the update: the first sync
//     creates slow := p (p unchanged), every later one slow <- slow + alpha (p - slow), p := slow.
// The step count t lives in device memory (step_state[0]: steps taken so far), so that the bias
// corrections, N_sma and the LookAhead sync follow the step under graph / launch-list replay:
// every workgroup derives the step's scalars from it in fp64 (identical values everywhere), and
// the last workgroup to arrive writes t + 1.  Non-sync steps move 28 bytes per parameter, like
// RMSprop with momentum; a sync step 8 more.
// The clip form (scae_flat_opt_clip_step_f32) scales g by clip_grad_norm_'s coefficient from
// the norm launch's partials (grad_clip_dev.h) after grad_scale, before the weight decay.
// The accumulate forms (scae_flat_opt_acc_*: gradient accumulation, grad_accumulate.hip) read
// g = acc + grad in place of grad and leave acc = 0 behind.
// The guarded forms (scae_flat_opt[_acc]_guard_step_f32: the non-finite guard) are the clip
// forms behind a decision on the partials' fp64 sum: not finite, and the launch stores nothing
// and makes no arrival (the accumulate form: acc = 0); finite, and it is the clip form bit
// for bit.
#include "grad_clip_dev.h"

namespace {
enum { ADAM = 0, RADAM = 1, RMSPROP = 2 };   // scae_flat_opt_step_f32's `kind`

struct AdamArgs {
  float *p, *m, *v, *slow;
  const float *g;
  const float *lr_dev;
  int *state;        // [0] steps taken, [1] slow buffer made, [2] + sub-counters: arrivals
  long n;
  double b1, b2;     // RMSprop: momentum, alpha
  float eps, weight_decay, grad_scale, la_alpha;
  int la_k, advance;
};

// what every element of one step shares
struct StepScalars {
  float b1, omb1, b2, omb2;  // betas and 1 - betas, each rounded once from fp64 (as torch does)
  float step;                // Adam: lr / (1-b1^t);  RAdam: lr x its step size;  RMSprop: lr
  float bc2;                 // Adam: sqrt(1 - b2^t)
  float decay;               // RAdam: wd x lr
  int t;                     // steps taken before this one
  float coef;                // clip_grad_norm_'s coefficient (the clip form only)
  bool rect, sync, init;     // RAdam's regime; LookAhead: a sync step, slow already made
};

// b^t for an integer t >= 1 by repeated squaring: ~2 log2(t) fp64 products instead of pow()'s
// few hundred fp64 instructions
__device__ __forceinline__ double ipow(double b, int t) {
  double r = 1.0;
  for (; t > 0; t >>= 1, b *= b)
    if (t & 1) r *= b;
  return r;
}

template <int K>
__device__ __forceinline__ StepScalars step_scalars(const AdamArgs &a) {
  StepScalars s;
  s.t = a.state[0];
  const double t = s.t + 1.0, lr = a.lr_dev[0];
  const double b1t = ipow(a.b1, s.t + 1), b2t = ipow(a.b2, s.t + 1);
  s.b1 = (float)a.b1, s.omb1 = (float)(1.0 - a.b1);
  s.b2 = (float)a.b2, s.omb2 = (float)(1.0 - a.b2);
  s.bc2 = (float)sqrt(1.0 - b2t);
  s.decay = (float)((double)a.weight_decay * lr);
  s.rect = false;
  if (K == RMSPROP) {
    s.omb2 = 1.f - s.b2;   // (as optimizer.hip: 1 - alpha in fp32)
    s.step = a.lr_dev[0];
  } else if (K == ADAM) {
    s.step = (float)(lr / (1.0 - b1t));
  } else {   // optimizers.py:70-85, the same expressions in the same order
    const double n_max = 2.0 / (1.0 - a.b2) - 1.0;
    const double n_sma = n_max - 2.0 * t * b2t / (1.0 - b2t);
    s.rect = n_sma >= 5.0;
    const double size =
        s.rect ? sqrt((1.0 - b2t) * (n_sma - 4.0) / (n_max - 4.0) * (n_sma - 2.0) / n_sma * n_max /
                      (n_max - 2.0)) /
                     (1.0 - b1t)
               : 1.0 / (1.0 - b1t);
    s.step = (float)(size * lr);
  }
  s.sync = a.la_k > 0 && (s.t + 1) % a.la_k == 0;
  s.init = a.state[1] != 0;
  return s;
}

// ... computed by one thread of the workgroup, read by all (the same values in every workgroup);
// CLIP: with the clip coefficient, reduced from the norm launch's partials by the whole workgroup
template <int K, bool CLIP = false>
__device__ __forceinline__ StepScalars shared_scalars(const AdamArgs &a,
                                                      const scae_clip::Clip *clip = nullptr) {
  __shared__ StepScalars sh;
  float coef = 1.f;
  if (CLIP) coef = scae_clip::clip_coef(*clip, a.grad_scale);
  if (threadIdx.x == 0) {
    sh = step_scalars<K>(a);
    if (CLIP) sh.coef = coef;
  }
  __syncthreads();
  return sh;
}

// (no FMA contraction: the update is compiled into three kernels -- vector, scalar edge, the sum
// workgroups of adam_sums_kernel -- that must round alike, bit for bit; the fmaf calls are the
// fused multiply-adds of torch's CPU kernels)
#pragma clang fp contract(off)
template <int K, bool CLIP = false>
__device__ __forceinline__ void update(float &p, float &m, float &v, float g, const AdamArgs &a,
                                       const StepScalars &s) {
  g *= a.grad_scale;  // e.g. 1/world_size after a SUM all-reduce
  if (CLIP) g *= s.coef;   // clip_grad_norm_ (exact for coef == 1: the unclipped pass's bits)
  if (K == RMSPROP) {   // optimizer.hip's update(): b1 = momentum, b2 = alpha
    if (a.weight_decay != 0.f) g = fmaf(a.weight_decay, p, g);
    v = s.b2 * v + s.omb2 * g * g;
    const float step = g / (sqrtf(v) + a.eps);
    if (s.b1 > 0.f) {
      m = s.b1 * m + step;
      p -= s.step * m;
    } else {
      p -= s.step * step;
    }
  } else if (K == ADAM) {
    if (a.weight_decay != 0.f) g = fmaf(a.weight_decay, p, g);  // grad.add(param, alpha=wd)
    m = fmaf(s.omb1, g - m, m);                                 // exp_avg.lerp_(grad, 1-b1)
    v = s.b2 * v + s.omb2 * g * g;
    p -= s.step * m / (sqrtf(v) / s.bc2 + a.eps);
  } else {
    v = s.b2 * v + s.omb2 * g * g;
    m = fmaf(s.omb1, g, s.b1 * m);
    if (a.weight_decay != 0.f) p = fmaf(-s.decay, p, p);        // p.add_(-wd lr, p)
    if (s.rect)
      p -= s.step * m / (sqrtf(v) + a.eps);
    else
      p = fmaf(-s.step, m, p);                                  // p.add_(-step lr, exp_avg)
  }
}

// LookAhead's sync (sync steps only)
__device__ __forceinline__ void look_ahead(float &p, float &slow, const AdamArgs &a,
                                           const StepScalars &s) {
  if (s.init) {
    slow = fmaf(a.la_alpha, p - slow, slow);   // slow.add_(alpha, fast - slow)
    p = slow;
  } else {
    slow = p;                                  // the lazily created slow buffer
  }
}

// one element in place (scalar edges, sum workgroups); ACC: g = acc + grad, acc zeroed
template <int K, bool CLIP = false, bool ACC = false>
__device__ __forceinline__ void update_at(const AdamArgs &a, const StepScalars &s, long i,
                                          float g, float *acc = nullptr) {
  if (ACC) g = acc[i] + g, acc[i] = 0.f;
  float p = a.p[i], m = a.m[i], v = a.v[i];
  update<K, CLIP>(p, m, v, g, a, s);
  if (s.sync) {
    float sl = a.slow[i];
    look_ahead(p, sl, a, s);
    a.slow[i] = sl;
  }
  a.p[i] = p, a.m[i] = m, a.v[i] = v;
}

// The last workgroup of the launch to get here advances the step count (every workgroup has
// read it by then: its value was consumed before the barrier in shared_scalars); the next launch
// sees it as it sees any kernel's output.  The arrival goes in two levels -- SUBS counters, each
// on a 256-byte line of its own, then one -- because 2048 device-scope atomics on ONE address
// serialise: 18 us of a 30 us pass at cfg-2's size.  (No __threadfence() either: a device-scope
// fence writes the XCD's L2 back, and one per workgroup made the pass 78 us.)  Every counter is
// back at 0 when the launch ends.
constexpr int SUBS = 32, LINE = 64;   // sub-counter k at state[LINE * (k + 1)]
static_assert(LINE * (SUBS + 1) == SCAE_FLAT_OPT_STATE_INTS, "step_state layout");
__device__ __forceinline__ void arrive(const AdamArgs &a, const StepScalars &s) {
  if (!a.advance) return;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int grid = (int)gridDim.x, k = (int)blockIdx.x % SUBS;
  const int members = grid / SUBS + (k < grid % SUBS);   // workgroups that share counter k
  int *sub = a.state + LINE * (k + 1);
  if (atomicAdd(sub, 1) != members - 1) return;
  atomicExch(sub, 0);
  if (atomicAdd(&a.state[2], 1) != min(grid, SUBS) - 1) return;
  atomicExch(&a.state[2], 0);
  a.state[0] = s.t + 1;
  if (s.sync) a.state[1] = 1;
}

// the float4 lanes of elements [head + 4 i, head + 4 i + 4): `own` bit u set = element u is
// not this workgroup's to write; ACC: g = acc + grad, acc zeroed
template <int K, bool CLIP = false, bool ACC = false>
__device__ __forceinline__ void update_quad(const AdamArgs &a, const StepScalars &s, int head,
                                            long i, int own, float *acc = nullptr) {
  float *p4 = a.p + head, *m4 = a.m + head, *v4 = a.v + head, *s4 = a.slow + head;
  float4 p = reinterpret_cast<float4 *>(p4)[i], m = reinterpret_cast<float4 *>(m4)[i],
         v = reinterpret_cast<float4 *>(v4)[i];
  float4 g = reinterpret_cast<const float4 *>(a.g + head)[i];
  float *a4 = acc + head;
  if (ACC) {
    const float4 ac = reinterpret_cast<float4 *>(a4)[i];
    g = make_float4(ac.x + g.x, ac.y + g.y, ac.z + g.z, ac.w + g.w);
  }
  update<K, CLIP>(p.x, m.x, v.x, g.x, a, s);
  update<K, CLIP>(p.y, m.y, v.y, g.y, a, s);
  update<K, CLIP>(p.z, m.z, v.z, g.z, a, s);
  update<K, CLIP>(p.w, m.w, v.w, g.w, a, s);
  float4 sl;
  if (s.sync) {   // (workgroup-uniform)
    sl = reinterpret_cast<float4 *>(s4)[i];
    look_ahead(p.x, sl.x, a, s);
    look_ahead(p.y, sl.y, a, s);
    look_ahead(p.z, sl.z, a, s);
    look_ahead(p.w, sl.w, a, s);
  }
  if (own == 0) {
    reinterpret_cast<float4 *>(p4)[i] = p;
    reinterpret_cast<float4 *>(m4)[i] = m;
    reinterpret_cast<float4 *>(v4)[i] = v;
    if (s.sync) reinterpret_cast<float4 *>(s4)[i] = sl;
    if (ACC) reinterpret_cast<float4 *>(a4)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {   // (rare: a quad that straddles the edge of a range the sum workgroups own)
    const float pe[4] = {p.x, p.y, p.z, p.w}, me[4] = {m.x, m.y, m.z, m.w},
                ve[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (!((own >> u) & 1)) {
        p4[4 * i + u] = pe[u], m4[4 * i + u] = me[u], v4[4 * i + u] = ve[u];
        if (ACC) a4[4 * i + u] = 0.f;
      }
    if (s.sync) {
      const float se[4] = {sl.x, sl.y, sl.z, sl.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (!((own >> u) & 1)) s4[4 * i + u] = se[u];
    }
  }
}

// `head` leading elements bring the (equally misaligned) buffers to a 16-byte boundary; then
// float4 lanes; then the tail
template <int K, bool CLIP, bool ACC = false>
__device__ __forceinline__ void adam_pass(const AdamArgs &a, int head, const StepScalars &s,
                                          float *acc = nullptr) {
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n4 = (a.n - head) >> 2;
  for (long i = tid; i < n4; i += stride) update_quad<K, CLIP, ACC>(a, s, head, i, 0, acc);
  const long tail0 = head + (n4 << 2), edge = head + (a.n - tail0);
  for (long e = tid; e < edge; e += stride) {
    const long i = e < head ? e : tail0 + (e - head);
    update_at<K, CLIP, ACC>(a, s, i, a.g[i], acc);
  }
  arrive(a, s);
}
template <int K>
__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a, int head) {
  adam_pass<K, false>(a, head, shared_scalars<K>(a));
}
// the clip form: every workgroup first reduces the norm launch's partials to the coefficient
// (the same bits in every workgroup)
template <int K>
__global__ __launch_bounds__(256) void adam_clip_kernel(AdamArgs a, int head,
                                                        scae_clip::Clip clip) {
  adam_pass<K, true>(a, head, shared_scalars<K, true>(a, &clip));
}
// the accumulate forms of the two above
template <int K>
__global__ __launch_bounds__(256) void adam_acc_kernel(AdamArgs a, int head, float *acc) {
  adam_pass<K, false, true>(a, head, shared_scalars<K>(a), acc);
}
template <int K>
__global__ __launch_bounds__(256) void adam_acc_clip_kernel(AdamArgs a, int head,
                                                            scae_clip::Clip clip, float *acc) {
  adam_pass<K, true, true>(a, head, shared_scalars<K, true>(a, &clip), acc);
}
// the guarded forms of the two clip forms (the non-finite guard, grad_clip_dev.h): a workgroup
// that finds the partials' fp64 sum not finite returns before the pass and before arrive() --
// nothing is stored to p, m, v or slow, step_state keeps every int (the count, the slow-made
// flag, the arrival counters at 0); the accumulate form leaves acc = 0 over its elements
template <int K, bool ACC>
__device__ __forceinline__ void adam_guard(const AdamArgs &a, int head,
                                           const scae_clip::Clip &clip,
                                           const scae_clip::Guard &guard, float *acc) {
  __shared__ StepScalars sh;
  bool skip;
  const float coef = scae_clip::guard_coef(clip, guard, a.grad_scale, skip);
  if (skip) {   // workgroup-uniform, after the sum's barrier
    if (ACC) scae_clip::zero_acc(acc, a.n, head);
    return;
  }
  if (threadIdx.x == 0) {   // (as shared_scalars<K, true>)
    sh = step_scalars<K>(a);
    sh.coef = coef;
  }
  __syncthreads();
  const StepScalars s = sh;
  adam_pass<K, true, ACC>(a, head, s, acc);
}
template <int K>
__global__ __launch_bounds__(256) void adam_guard_kernel(AdamArgs a, int head,
                                                         scae_clip::Clip clip,
                                                         scae_clip::Guard guard) {
  adam_guard<K, false>(a, head, clip, guard, nullptr);
}
template <int K>
__global__ __launch_bounds__(256) void adam_acc_guard_kernel(AdamArgs a, int head,
                                                             scae_clip::Clip clip,
                                                             scae_clip::Guard guard, float *acc) {
  adam_guard<K, true>(a, head, clip, guard, acc);
}

// The step's last column sums and the optimiser in one launch, as optimizer.hip's
// rmsprop_sums_kernel: the sum workgroups (the head of the grid) update the elements they
// produce, the streaming workgroups behind them skip exactly those (the segments' destination
// ranges, rebuilt from the job table into LDS by every workgroup).  Same arithmetic per element:
// the results equal the two launches' bit for bit.
// ACC: the accumulate form.
using scae_sums::MAXR;
template <int K, bool ACC>
__device__ __forceinline__ void adam_sums(const AdamArgs &a, int head,
                                          const scae_sums::Jobs &jobs, int sum_blocks,
                                          float *acc) {
  __shared__ float red[scae_sums::NT];
  __shared__ int r_lo[MAXR], r_hi[MAXR];
  __shared__ int r_n;
  const StepScalars s = shared_scalars<K>(a);
  if ((int)blockIdx.x < sum_blocks) {   // workgroup-uniform
    scae_sums::sum_block(jobs, blockIdx.x, red, [&](float *dst, float v) {
      *dst = v;
      const long off = dst - a.g;
      if (off >= 0 && off < a.n) update_at<K, false, ACC>(a, s, off, v, acc);
    });
    arrive(a, s);
    return;
  }
  // the ranges of the flat buffers the sum workgroups own
  const int nr = scae_sums::owned_ranges(jobs, a.g, a.n, r_lo, r_hi, &r_n);
  const long stride = (long)(gridDim.x - sum_blocks) * blockDim.x;
  const long tid = (long)(blockIdx.x - sum_blocks) * blockDim.x + threadIdx.x;
  const long n4 = (a.n - head) >> 2;
  for (long i = tid; i < n4; i += stride) {
    const int e0 = head + 4 * (int)i;
    // bit u: element e0 + u belongs to a sum workgroup
    const int own = scae_sums::quad_owned(e0, r_lo, r_hi, nr);
    if (own != 15) update_quad<K, false, ACC>(a, s, head, i, own, acc);
  }
  const long tail0 = head + (n4 << 2), edge = head + (a.n - tail0);
  for (long e = tid; e < edge; e += stride) {
    const long i = e < head ? e : tail0 + (e - head);
    if (!scae_sums::owned(i, r_lo, r_hi, nr)) update_at<K, false, ACC>(a, s, i, a.g[i], acc);
  }
  arrive(a, s);
}
template <int K>
__global__ __launch_bounds__(256) void adam_sums_kernel(AdamArgs a, int head, scae_sums::Jobs jobs,
                                                        int sum_blocks) {
  adam_sums<K, false>(a, head, jobs, sum_blocks, nullptr);
}
template <int K>
__global__ __launch_bounds__(256) void adam_acc_sums_kernel(AdamArgs a, int head,
                                                            scae_sums::Jobs jobs, int sum_blocks,
                                                            float *acc) {
  adam_sums<K, true>(a, head, jobs, sum_blocks, acc);
}

// the checks both entry points share; -> head, or < 0
int prepare(AdamArgs &a, float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
            float *slow, int64_t n, const float *lr_dev, int32_t *step_state, int kind,
            double beta1, double beta2, float eps, float weight_decay, float grad_scale,
            int look_ahead_k, float look_ahead_alpha, int advance) {
  if (!(param && grad && exp_avg && exp_avg_sq && lr_dev && step_state && n > 0 &&
        (kind == ADAM || kind == RADAM || kind == RMSPROP) && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 &&
        beta2 < 1.0 && look_ahead_k >= 0 && (look_ahead_k == 0 || slow) && n < (1l << 31)))
    return -1;
  // all buffers slices of equally laid out flat buffers: same phase within a 16-byte line
  const size_t phase = (size_t)param & 15;
  if ((phase & 3) || ((size_t)grad & 15) != phase || ((size_t)exp_avg & 15) != phase ||
      ((size_t)exp_avg_sq & 15) != phase || (look_ahead_k > 0 && ((size_t)slow & 15) != phase))
    return -1;
  a = AdamArgs{param,       exp_avg,   exp_avg_sq,   look_ahead_k > 0 ? slow : nullptr,
               grad,        lr_dev,    step_state,   (long)n,
               beta1,       beta2,     eps,          weight_decay,
               grad_scale,  look_ahead_alpha, look_ahead_k, advance != 0};
  int head = (int)((16 - phase) & 15) / 4;
  return head > n ? (int)n : head;
}
}  // namespace

template <template <int> class F, class... T>
void launch_kind(int kind, dim3 grid, hipStream_t st, T... args) {
  scae::launch(kind == ADAM ? F<ADAM>::fn : kind == RADAM ? F<RADAM>::fn : F<RMSPROP>::fn, grid,
               dim3(256), 0, st, args...);
}
template <int K> struct Plain { static constexpr auto fn = adam_kernel<K>; };
template <int K> struct Sums { static constexpr auto fn = adam_sums_kernel<K>; };
template <int K> struct Clipped { static constexpr auto fn = adam_clip_kernel<K>; };
template <int K> struct AccPlain { static constexpr auto fn = adam_acc_kernel<K>; };
template <int K> struct AccSums { static constexpr auto fn = adam_acc_sums_kernel<K>; };
template <int K> struct AccClipped { static constexpr auto fn = adam_acc_clip_kernel<K>; };
template <int K> struct Guarded { static constexpr auto fn = adam_guard_kernel<K>; };
template <int K> struct AccGuarded { static constexpr auto fn = adam_acc_guard_kernel<K>; };

extern "C" int scae_flat_opt_step_f32(float *param, const float *grad, float *exp_avg,
                                      float *exp_avg_sq, float *slow, int64_t n,
                                      const float *lr_dev, int32_t *step_state, int kind,
                                      double beta1, double beta2, float eps, float weight_decay,
                                      float grad_scale, int look_ahead_k, float look_ahead_alpha,
                                      int advance, void *stream) {
  AdamArgs a;
  const int head = prepare(a, param, grad, exp_avg, exp_avg_sq, slow, n, lr_dev, step_state,
                           kind, beta1, beta2, eps, weight_decay, grad_scale, look_ahead_k,
                           look_ahead_alpha, advance);
  if (head < 0) return SCAE_ERR_BAD_ARG;
  long blocks = (n / 4 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  launch_kind<Plain>(kind, dim3((unsigned)blocks), (hipStream_t)stream, a, head);
  return scae_launch_status();
}

extern "C" int scae_flat_opt_sums_step_f32(float *param, float *grad, float *exp_avg,
                                           float *exp_avg_sq, float *slow, int64_t n,
                                           const float *lr_dev, int32_t *step_state, int kind,
                                           double beta1, double beta2, float eps,
                                           float grad_scale, int look_ahead_k,
                                           float look_ahead_alpha, const scae_sum_job *jobs,
                                           int n_jobs, void *stream) {
  AdamArgs a;
  const int head = prepare(a, param, grad, exp_avg, exp_avg_sq, slow, n, lr_dev, step_state,
                           kind, beta1, beta2, eps, 0.f, grad_scale, look_ahead_k,
                           look_ahead_alpha, 1);
  if (head < 0) return SCAE_ERR_BAD_ARG;
  scae_sums::Jobs js;
  const int sum_blocks = scae_sums::fill_jobs(js, jobs, n_jobs);
  SCAE_REQUIRE(sum_blocks > 0);
  // the whole grid resident at once, as scae_rmsprop_sums_step_f32
  long blocks = (n / 4 + 255) / 256;
  const long room = 2048 - sum_blocks;
  const long cap = room > 512 ? room : 512;
  blocks = blocks < 1 ? 1 : (blocks > cap ? cap : blocks);
  launch_kind<Sums>(kind, dim3((unsigned)(sum_blocks + blocks)), (hipStream_t)stream, a, head,
                    js, sum_blocks);
  return scae_launch_status();
}

// scae_flat_opt[_acc]_clip_step_f32 and scae_flat_opt[_acc]_guard_step_f32 behind one set of
// checks and one grid; acc: the accumulate forms; GUARD: the guarded kernels, which also take
// guard_state
namespace {
template <bool GUARD>
int clip_launch(float *param, const float *grad, float *acc, float *exp_avg, float *exp_avg_sq,
                float *slow, int64_t n, const float *lr_dev, int32_t *step_state, int kind,
                double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                int look_ahead_k, float look_ahead_alpha, int advance, const double *partials,
                int n_partials, float max_norm, float *norm_out, int64_t *guard_state,
                bool with_acc, void *stream) {
  AdamArgs a;
  const int head = prepare(a, param, grad, exp_avg, exp_avg_sq, slow, n, lr_dev, step_state,
                           kind, beta1, beta2, eps, weight_decay, grad_scale, look_ahead_k,
                           look_ahead_alpha, advance);
  if (head < 0 || ((size_t)guard_state & 7)) return SCAE_ERR_BAD_ARG;
  if (with_acc && !(acc && ((size_t)acc & 15) == ((size_t)param & 15))) return SCAE_ERR_BAD_ARG;
  SCAE_REQUIRE(partials && n_partials > 0 && n_partials <= SCAE_GRAD_SQ_MAX_PARTIALS &&
               max_norm > 0.f);
  long blocks = (n / 4 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  const dim3 grid((unsigned)blocks);
  const hipStream_t st = (hipStream_t)stream;
  const scae_clip::Clip clip{partials, n_partials, max_norm, norm_out};
  if constexpr (GUARD) {
    const scae_clip::Guard guard{(long long *)guard_state};
    if (with_acc)
      launch_kind<AccGuarded>(kind, grid, st, a, head, clip, guard, acc);
    else
      launch_kind<Guarded>(kind, grid, st, a, head, clip, guard);
  } else {
    if (with_acc)
      launch_kind<AccClipped>(kind, grid, st, a, head, clip, acc);
    else
      launch_kind<Clipped>(kind, grid, st, a, head, clip);
  }
  return scae_launch_status();
}
}  // namespace

// scae_flat_opt_step_f32 with g scaled by clip_grad_norm_'s coefficient (grad_clip_dev.h)
extern "C" int scae_flat_opt_clip_step_f32(float *param, const float *grad, float *exp_avg,
                                           float *exp_avg_sq, float *slow, int64_t n,
                                           const float *lr_dev, int32_t *step_state, int kind,
                                           double beta1, double beta2, float eps,
                                           float weight_decay, float grad_scale,
                                           int look_ahead_k, float look_ahead_alpha, int advance,
                                           const double *partials, int n_partials,
                                           float max_norm, float *norm_out, void *stream) {
  return clip_launch<false>(param, grad, nullptr, exp_avg, exp_avg_sq, slow, n, lr_dev,
                            step_state, kind, beta1, beta2, eps, weight_decay, grad_scale,
                            look_ahead_k, look_ahead_alpha, advance, partials, n_partials,
                            max_norm, norm_out, nullptr, false, stream);
}

// scae_flat_opt_clip_step_f32 behind the non-finite guard (max_norm = +inf: the guard alone)
extern "C" int scae_flat_opt_guard_step_f32(float *param, const float *grad, float *exp_avg,
                                            float *exp_avg_sq, float *slow, int64_t n,
                                            const float *lr_dev, int32_t *step_state, int kind,
                                            double beta1, double beta2, float eps,
                                            float weight_decay, float grad_scale,
                                            int look_ahead_k, float look_ahead_alpha,
                                            int advance, const double *partials,
                                            int n_partials, float max_norm, float *norm_out,
                                            int64_t *guard_state, void *stream) {
  return clip_launch<true>(param, grad, nullptr, exp_avg, exp_avg_sq, slow, n, lr_dev,
                           step_state, kind, beta1, beta2, eps, weight_decay, grad_scale,
                           look_ahead_k, look_ahead_alpha, advance, partials, n_partials,
                           max_norm, norm_out, guard_state, false, stream);
}

// ---- the accumulate forms (gradient accumulation): the three entry points above with
// g = acc + grad; acc (n floats at the buffers' phase in a 16-byte line) is 0 afterwards -----
static bool acc_ok(const float *acc, const float *param) {
  return acc && ((size_t)acc & 15) == ((size_t)param & 15);
}

extern "C" int scae_flat_opt_acc_step_f32(float *param, const float *grad, float *acc,
                                          float *exp_avg, float *exp_avg_sq, float *slow,
                                          int64_t n, const float *lr_dev, int32_t *step_state,
                                          int kind, double beta1, double beta2, float eps,
                                          float weight_decay, float grad_scale, int look_ahead_k,
                                          float look_ahead_alpha, int advance, void *stream) {
  AdamArgs a;
  const int head = prepare(a, param, grad, exp_avg, exp_avg_sq, slow, n, lr_dev, step_state,
                           kind, beta1, beta2, eps, weight_decay, grad_scale, look_ahead_k,
                           look_ahead_alpha, advance);
  if (head < 0 || !acc_ok(acc, param)) return SCAE_ERR_BAD_ARG;
  long blocks = (n / 4 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  launch_kind<AccPlain>(kind, dim3((unsigned)blocks), (hipStream_t)stream, a, head, acc);
  return scae_launch_status();
}

extern "C" int scae_flat_opt_acc_sums_step_f32(float *param, float *grad, float *acc,
                                               float *exp_avg, float *exp_avg_sq, float *slow,
                                               int64_t n, const float *lr_dev,
                                               int32_t *step_state, int kind, double beta1,
                                               double beta2, float eps, float grad_scale,
                                               int look_ahead_k, float look_ahead_alpha,
                                               const scae_sum_job *jobs, int n_jobs,
                                               void *stream) {
  AdamArgs a;
  const int head = prepare(a, param, grad, exp_avg, exp_avg_sq, slow, n, lr_dev, step_state,
                           kind, beta1, beta2, eps, 0.f, grad_scale, look_ahead_k,
                           look_ahead_alpha, 1);
  if (head < 0 || !acc_ok(acc, param)) return SCAE_ERR_BAD_ARG;
  scae_sums::Jobs js;
  const int sum_blocks = scae_sums::fill_jobs(js, jobs, n_jobs);
  SCAE_REQUIRE(sum_blocks > 0);
  long blocks = (n / 4 + 255) / 256;
  const long room = 2048 - sum_blocks;
  const long cap = room > 512 ? room : 512;
  blocks = blocks < 1 ? 1 : (blocks > cap ? cap : blocks);
  launch_kind<AccSums>(kind, dim3((unsigned)(sum_blocks + blocks)), (hipStream_t)stream, a, head,
                       js, sum_blocks, acc);
  return scae_launch_status();
}

extern "C" int scae_flat_opt_acc_clip_step_f32(float *param, const float *grad, float *acc,
                                               float *exp_avg, float *exp_avg_sq, float *slow,
                                               int64_t n, const float *lr_dev,
                                               int32_t *step_state, int kind, double beta1,
                                               double beta2, float eps, float weight_decay,
                                               float grad_scale, int look_ahead_k,
                                               float look_ahead_alpha, int advance,
                                               const double *partials, int n_partials,
                                               float max_norm, float *norm_out, void *stream) {
  return clip_launch<false>(param, grad, acc, exp_avg, exp_avg_sq, slow, n, lr_dev, step_state,
                            kind, beta1, beta2, eps, weight_decay, grad_scale, look_ahead_k,
                            look_ahead_alpha, advance, partials, n_partials, max_norm, norm_out,
                            nullptr, true, stream);
}

extern "C" int scae_flat_opt_acc_guard_step_f32(float *param, const float *grad, float *acc,
                                                float *exp_avg, float *exp_avg_sq, float *slow,
                                                int64_t n, const float *lr_dev,
                                                int32_t *step_state, int kind, double beta1,
                                                double beta2, float eps, float weight_decay,
                                                float grad_scale, int look_ahead_k,
                                                float look_ahead_alpha, int advance,
                                                const double *partials, int n_partials,
                                                float max_norm, float *norm_out,
                                                int64_t *guard_state, void *stream) {
  return clip_launch<true>(param, grad, acc, exp_avg, exp_avg_sq, slow, n, lr_dev, step_state,
                           kind, beta1, beta2, eps, weight_decay, grad_scale, look_ahead_k,
                           look_ahead_alpha, advance, partials, n_partials, max_norm, norm_out,
                           guard_state, true, stream);
}
