// The ordered sums of the analysis kernels (kmeans, linear_probe, tsne, tsne_sparse): these
// bodies ARE the order of every fp64 sum behind the inertia, the probe's loss, Z, KL, the column
// means and |g|, so there is one copy.  (scae_clip::block_sum_f64 of grad_clip_dev.h pairs the
// waves as (r0 + r1) + (r2 + r3): another order, the training step's.)
#pragma once
#include "common.h"

namespace scae_reduce {
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the block's fp64 sum of one value per thread: waves by shuffle, then in wave order; valid in
// thread 0.  red: NT / 64 doubles; contains barriers
template <int NT>
__device__ __forceinline__ double block_sum_f64(double v, double *red) {
  static_assert(NT == 4 * SCAE_WAVE, "the wave order below is written out for four waves");
  v = wave_sum_f64(v);
  __syncthreads();   // (red may still be read from the call before)
  if (threadIdx.x % SCAE_WAVE == 0) red[threadIdx.x / SCAE_WAVE] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ double ordered_sum(const double *p, int n) {
  double s = 0.0;
  for (int b = 0; b < n; ++b) s += p[b];
  return s;
}
}  // namespace scae_reduce
