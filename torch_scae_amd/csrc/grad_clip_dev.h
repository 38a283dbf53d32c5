// Device code of gradient clipping by global norm (torch.nn.utils.clip_grad_norm_, as
// Lightning's Trainer(gradient_clip_val) applies it between backward and the optimiser step):
// the norm launch of grad_clip.hip writes a few hundred fp64 partial sums of g^2, and every
// workgroup of the clip forms of the optimiser passes (optimizer.hip, optimizer_adam.hip)
// reduces them itself -- in one fixed order, so every workgroup of every launch of the step
// holds the same coefficient bit for bit, with no inter-workgroup synchronisation.  The guarded
// forms (the non-finite guard) take their decision on that same sum.
#pragma once
#include "sum_rows_dev.h"

namespace scae_clip {
struct Clip {
  const double *partials;   // scae_grad_sq_partials_f32's output
  int n_partials;
  float max_norm;
  float *norm_out;          // the norm before clipping (workgroup 0 writes it) or NULL
};

// the sum over a workgroup of 256 threads (4 waves of 64) in a fixed order: a butterfly within
// each wave (partner sums are commutative: every lane ends on the same bits), then the four
// wave sums in order; every thread returns it.  `red`: 4 doubles of LDS.
__device__ __forceinline__ double block_sum_f64(double s, double *red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// the fp64 sum of the norm launch's partials, in one fixed order: the same bits in every
// workgroup of every launch of the step.  Every thread of the workgroup calls it (one barrier).
__device__ __forceinline__ double partials_sum(const Clip &c) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < c.n_partials; i += 256) s += c.partials[i];
  return block_sum_f64(s, red);
}

// clip_grad_norm_'s coefficient min(1, max_norm / (total + 1e-6)) in fp32, total =
// grad_scale sqrt(sum of the partials) (the norm of the scaled gradient; the sum in fp64).
// Every thread of the workgroup calls it (one barrier).  A NaN total gives a NaN coefficient,
// an infinite one 0, as in torch.
__device__ __forceinline__ float clip_coef(const Clip &c, float grad_scale) {
  const double sum = partials_sum(c);
  const float total = (float)((double)grad_scale * sqrt(sum));
  if (c.norm_out && blockIdx.x == 0 && threadIdx.x == 0) *c.norm_out = total;
  const float r = c.max_norm / (total + 1e-6f);
  return r > 1.f ? 1.f : r;
}

// The non-finite guard (the guarded forms of the optimiser passes): the step is skipped iff
// that fp64 sum is not finite -- a NaN or +-Inf element makes it NaN or +Inf, and finite fp32
// elements cannot overflow it (the fp32 `total` can: it does not decide).  The same bits
// everywhere, so every workgroup of every launch of the step decides alike; taken after the
// sum's barrier, workgroup-uniform.  state: int64 {skipped, first, last, attempts} or NULL
// (the launch decides but does not count); one writer a step -- thread 0 of workgroup 0 of
// the launch that is handed the pointer -- so plain loads and stores do.
struct Guard {
  long long *state;
};

// -> the coefficient of a step that is taken: clip_coef's, or the constant 1 when max_norm is
// +inf (the guard without clipping: inf / (total + 1e-6) is NaN once a finite gradient's fp32
// norm overflows).  `skip`: the decision.  norm_out is written either way.
__device__ __forceinline__ float guard_coef(const Clip &c, const Guard &gd, float grad_scale,
                                            bool &skip) {
  const double sum = partials_sum(c);
  const float total = (float)((double)grad_scale * sqrt(sum));
  skip = !(fabs(sum) < __builtin_inf());   // NaN or Inf
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (c.norm_out) *c.norm_out = total;
    if (gd.state) {
      const long long t = gd.state[3];
      if (skip) {
        gd.state[0] += 1;
        if (gd.state[1] < 0) gd.state[1] = t;
        gd.state[2] = t;
      }
      gd.state[3] = t + 1;
    }
  }
  if (c.max_norm == __builtin_inff()) return 1.f;
  const float r = c.max_norm / (total + 1e-6f);
  return r > 1.f ? 1.f : r;
}

// what a skipped accumulate form leaves behind: acc = 0 over the n elements of the launch
// (`head` leading elements up to the 16-byte boundary, float4 lanes, the tail)
__device__ __forceinline__ void zero_acc(float *acc, long n, int head) {
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n4 = (n - head) >> 2;
  for (long i = tid; i < n4; i += stride)
    reinterpret_cast<float4 *>(acc + head)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const long tail0 = head + (n4 << 2), edge = head + (n - tail0);
  for (long e = tid; e < edge; e += stride) acc[e < head ? e : tail0 + (e - head)] = 0.f;
}
}  // namespace scae_clip
