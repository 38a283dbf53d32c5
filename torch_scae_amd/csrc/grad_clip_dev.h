// Device code of gradient clipping by global norm (torch.nn.utils.clip_grad_norm_, as
// Lightning's Trainer(gradient_clip_val) applies it between backward and the optimiser step):
// the norm launch of grad_clip.hip writes a few hundred fp64 partial sums of g^2, and every
// workgroup of the clip forms of the optimiser passes (optimizer.hip, optimizer_adam.hip)
// reduces them itself -- in one fixed order, so every workgroup of every launch of the step
// holds the same coefficient bit for bit, with no inter-workgroup synchronisation.
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

// clip_grad_norm_'s coefficient min(1, max_norm / (total + 1e-6)) in fp32, total =
// grad_scale sqrt(sum of the partials) (the norm of the scaled gradient; the sum in fp64).
// Every thread of the workgroup calls it (one barrier).  A NaN total gives a NaN coefficient,
// an infinite one 0, as in torch.
__device__ __forceinline__ float clip_coef(const Clip &c, float grad_scale) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < c.n_partials; i += 256) s += c.partials[i];
  const double sum = block_sum_f64(s, red);
  const float total = (float)((double)grad_scale * sqrt(sum));
  if (c.norm_out && blockIdx.x == 0 && threadIdx.x == 0) *c.norm_out = total;
  const float r = c.max_norm / (total + 1e-6f);
  return r > 1.f ? 1.f : r;
}
}  // namespace scae_clip
