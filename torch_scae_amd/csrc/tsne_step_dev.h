// The part of a t-SNE iteration that does not depend on how the gradient was summed, for
// tsne.hip (dense P) and tsne_sparse.hip (CSR P, N-body repulsion).  Either path leaves
// rows (6, N) = attraction (2), repulsion (2), Z, KL per row and then shares
//   tsne_block_z_kl    the tail of its rows kernel: the workgroup's fp64 sums of z | kl;
//   tsne_update_kernel Z, gradient, gains, velocity, position; fp64 column-sum and |g|^2 partials;
//   tsne_finish_kernel the update's grid again: the column means leave Y, and the history row;
//   tsne_run           the schedule: exaggeration and momentum by iteration, which iterations
//                      record, and the evaluation without an update after the last one.
// block holds five rows of per-workgroup partials -- z, kl, y0, y1, |g|^2 -- block_stride
// apart: the path's largest N over NU.  Every fp64 sum is reduce_f64_dev.h's, every
// product-sum an explicit fmaf, and each body here turns contraction off for itself.
//
// The kernels sit in an anonymous namespace: each including file gets its own, internal, copy.
#pragma once
#include "common.h"
#include "reduce_f64_dev.h"

namespace {
using scae_reduce::block_sum_f64;
using scae_reduce::ordered_sum;
constexpr int NU = 256;   // rows / update / finish workgroup: one row per thread

struct TsneState {
  int N;
  float learning_rate;
  float *Y, *velocity, *gains;   // (N, 2)
  const float *rows;             // (6, N)
  double *block;                 // (5, block_stride)
  int block_stride;
  const double *plogp;
  double *history;
};

template <class Desc>
TsneState tsne_state(const Desc &d, int block_stride) {
  return {d.N,     d.learning_rate, d.Y,     d.velocity, d.gains, d.rows,
          d.block, block_stride,    d.plogp, d.history};
}

// block (0 | 1, b) = the workgroup's fp64 sum of z | kl.  red: NU / 64 doubles; barriers
template <bool KL>
__device__ __forceinline__ void tsne_block_z_kl(float z, float kl, double *block,
                                                int block_stride, double *red) {
#pragma clang fp contract(off)
  const double zs = block_sum_f64<NU>((double)z, red);
  if (threadIdx.x == 0) block[blockIdx.x] = zs;
  if constexpr (KL) {
    const double ks = block_sum_f64<NU>((double)kl, red);
    if (threadIdx.x == 0) block[block_stride + blockIdx.x] = ks;
  }
}

// grid (ceil(N / NU)).  apply = 0: the gradient's norm alone (the evaluation after the last
// iteration); block (2 | 3 | 4, b) = the workgroup's fp64 sums of y0 | y1 | g0^2 + g1^2
__global__ __launch_bounds__(NU) void tsne_update_kernel(TsneState d, float exaggeration,
                                                         float momentum, int apply) {
#pragma clang fp contract(off)
  __shared__ double red[NU / SCAE_WAVE];
  const int i = blockIdx.x * NU + threadIdx.x, N = d.N, MAXB = d.block_stride;
  const float zinv = (float)(1.0 / ordered_sum(d.block, gridDim.x));
  double s0 = 0.0, s1 = 0.0, gg = 0.0;
  if (i < N) {
    float y[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float att = d.rows[(size_t)k * N + i], rep = d.rows[(size_t)(2 + k) * N + i];
      const float g = 4.f * (exaggeration * att - rep * zinv);
      gg += (double)g * (double)g;
      y[k] = d.Y[2 * (size_t)i + k];
      if (apply) {
        float vel = d.velocity[2 * (size_t)i + k], gain = d.gains[2 * (size_t)i + k];
        gain = fmaxf(g * vel < 0.f ? gain + 0.2f : gain * 0.8f, 0.01f);
        vel = momentum * vel - (d.learning_rate * gain) * g;
        y[k] += vel;
        d.gains[2 * (size_t)i + k] = gain, d.velocity[2 * (size_t)i + k] = vel;
        d.Y[2 * (size_t)i + k] = y[k];
      }
    }
    s0 = (double)y[0], s1 = (double)y[1];
  }
  s0 = block_sum_f64<NU>(s0, red);
  s1 = block_sum_f64<NU>(s1, red);
  gg = block_sum_f64<NU>(gg, red);
  if (threadIdx.x == 0) {
    d.block[2 * MAXB + blockIdx.x] = s0;
    d.block[3 * MAXB + blockIdx.x] = s1;
    d.block[4 * MAXB + blockIdx.x] = gg;
  }
}

// grid (ceil(N / NU)), a row per thread.  apply: Y loses its column means (every workgroup adds
// the update's partials in the same order; one workgroup walking all of Y took 54 us at
// N = 60 000); row >= 0: workgroup 0 writes the history row (it, KL, |g|)
__global__ __launch_bounds__(NU) void tsne_finish_kernel(TsneState d, int it, int apply,
                                                         int row) {
#pragma clang fp contract(off)
  __shared__ float mean[2];
  const int i = blockIdx.x * NU + threadIdx.x, N = d.N, nb = gridDim.x, MAXB = d.block_stride;
  if (apply) {
    if (threadIdx.x < 2)
      mean[threadIdx.x] =
          (float)(ordered_sum(d.block + (2 + threadIdx.x) * MAXB, nb) / (double)N);
    __syncthreads();
    if (i < N) d.Y[2 * (size_t)i] -= mean[0], d.Y[2 * (size_t)i + 1] -= mean[1];
  }
  if (row >= 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    const double Z = ordered_sum(d.block, nb);
    double *h = d.history + (size_t)row * SCAE_TSNE_HISTORY_COLS;
    h[0] = (double)it;
    h[1] = *d.plogp + ordered_sum(d.block + MAXB, nb) + log(Z);
    h[2] = sqrt(ordered_sum(d.block + 4 * MAXB, nb));
  }
}

// Iterations first_iter .. first_iter + n - 1 of the run d describes (either descriptor), and
// when they end it the evaluation of the result.  sum_gradient(kl) enqueues the path's
// launches that leave the gradient's sums in rows and z (| kl) in block; kl: a recorded
// iteration, the form that adds P log1p(d).
template <class Desc, class SumGradient>
void tsne_run(const Desc &d, int block_stride, int first_iter, int n, hipStream_t st,
              SumGradient sum_gradient) {
  const TsneState s = tsne_state(d, block_stride);
  const int nb = (d.N + NU - 1) / NU;
  // the launches of iteration it (apply) or of the evaluation at it (no update)
  auto iteration = [&](int it, bool apply, int row) {
    const bool early = it < d.exaggeration_iter;
    sum_gradient(row >= 0);
    scae::launch(tsne_update_kernel, dim3(nb), dim3(NU), 0, st, s,
                 early ? d.early_exaggeration : 1.f, early ? 0.5f : 0.8f, (int)apply);
    scae::launch(tsne_finish_kernel, dim3(nb), dim3(NU), 0, st, s, it, (int)apply, row);
  };
  for (int it = first_iter; it < first_iter + n; ++it)
    iteration(it, true, it > 0 && it % d.check_every == 0 ? it / d.check_every - 1 : -1);
  if (n > 0 && first_iter + n == d.n_iter)
    iteration(d.n_iter, false, (d.n_iter + d.check_every - 1) / d.check_every - 1);
}
}  // namespace
