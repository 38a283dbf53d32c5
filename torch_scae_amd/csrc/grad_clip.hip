// The gradient's sum of squares for clipping by global norm (torch.nn.utils.clip_grad_norm_,
// Lightning's Trainer(gradient_clip_val)): fp64 partial sums of g^2 over the flat gradient
// buffer, one per workgroup, into a small device workspace that every workgroup of the clip
// forms of the optimiser passes reduces in a fixed order (grad_clip_dev.h).  No atomics and no
// arrival counter: the partials are a function of the grid and the data, the grid a function
// of n (and of the riding sum jobs), so two runs give the same bits.  Squares of fp32 values
// are exact in fp64 and summed in fp64.
// The sums form hosts the step's last column sums (scae_sums::Jobs), as the optimiser's
// rmsprop_sums_kernel does: the sum workgroups head the grid, write their gradient slots and
// add the squares of what they write into their own partials; the streaming workgroups behind
// them skip exactly those destination ranges (scae_sums::owned_ranges).
// The accumulate forms (gradient accumulation, grad_accumulate.hip) take the squares of
// acc + g: the gradient of a group of batches that the accumulate forms of the optimiser
// passes then apply.
#include "grad_clip_dev.h"

namespace {
constexpr int MAX_STREAM = 512;   // streaming workgroups: at most this many partials
constexpr int UNROLL = 8;         // float4 loads in flight per thread

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

__device__ __forceinline__ double sq4(float4 v) {
  return ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
}

// this thread's share of the sum of squares of g[0, n) (workgroup `blk` of `nblk`): `head`
// leading elements bring g to a 16-byte boundary, then float4 lanes, then the tail; SKIP:
// without the elements of the nr ranges [r_lo, r_hi); ACC: of acc + g (acc laid out as g)
template <bool SKIP, bool ACC = false>
__device__ __forceinline__ double stream_sq(const float *g, long n, int head, int blk, int nblk,
                                            const int *r_lo, const int *r_hi, int nr,
                                            const float *acc = nullptr) {
  const long stride = (long)nblk * blockDim.x, tid = (long)blk * blockDim.x + threadIdx.x;
  const long n4 = (n - head) >> 2;
  const float4 *g4 = reinterpret_cast<const float4 *>(g + head);
  const float4 *a4 = reinterpret_cast<const float4 *>(acc + head);
  double s = 0.0;
  long i = tid;
  for (; i + (UNROLL - 1) * stride < n4; i += UNROLL * stride) {
    float4 v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) v[u] = g4[i + u * stride];
    if (ACC) {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) v[u] = add4(a4[i + u * stride], v[u]);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (SKIP) {
        const int own = scae_sums::quad_owned(head + 4 * (int)(i + u * stride), r_lo, r_hi, nr);
        if (own & 1) v[u].x = 0.f;
        if (own & 2) v[u].y = 0.f;
        if (own & 4) v[u].z = 0.f;
        if (own & 8) v[u].w = 0.f;
      }
      s += sq4(v[u]);
    }
  }
  for (; i < n4; i += stride) {
    float4 v = g4[i];
    if (ACC) v = add4(a4[i], v);
    if (SKIP) {
      const int own = scae_sums::quad_owned(head + 4 * (int)i, r_lo, r_hi, nr);
      if (own & 1) v.x = 0.f;
      if (own & 2) v.y = 0.f;
      if (own & 4) v.z = 0.f;
      if (own & 8) v.w = 0.f;
    }
    s += sq4(v);
  }
  // scalar edges: [0, head) and [head + 4*n4, n)
  const long tail0 = head + (n4 << 2), edge = head + (n - tail0);
  for (long e = tid; e < edge; e += stride) {
    const long k = e < head ? e : tail0 + (e - head);
    if (SKIP && scae_sums::owned(k, r_lo, r_hi, nr)) continue;
    const double x = ACC ? acc[k] + g[k] : g[k];
    s += x * x;
  }
  return s;
}

__global__ __launch_bounds__(256) void grad_sq_kernel(const float *g, long n, int head,
                                                      double *partials) {
  __shared__ double red[4];
  const double s = stream_sq<false>(g, n, head, blockIdx.x, gridDim.x, nullptr, nullptr, 0);
  const double tot = scae_clip::block_sum_f64(s, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

// the accumulate form: the squares of acc + g
__global__ __launch_bounds__(256) void grad_sq_acc_kernel(const float *g, const float *acc,
                                                          long n, int head, double *partials) {
  __shared__ double red[4];
  const double s =
      stream_sq<false, true>(g, n, head, blockIdx.x, gridDim.x, nullptr, nullptr, 0, acc);
  const double tot = scae_clip::block_sum_f64(s, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

template <bool ACC>
__device__ __forceinline__ void grad_sq_sums(float *g, long n, int head, double *partials,
                                             const scae_sums::Jobs &jobs, int sum_blocks,
                                             const float *acc) {
  __shared__ float red[scae_sums::NT];
  __shared__ int r_lo[scae_sums::MAXR], r_hi[scae_sums::MAXR];
  __shared__ int r_n;
  __shared__ double red2[4];
  double s = 0.0;
  if ((int)blockIdx.x < sum_blocks) {   // workgroup-uniform
    scae_sums::sum_block(jobs, blockIdx.x, red, [&](float *dst, float v) {
      *dst = v;
      const long off = dst - g;
      if (off >= 0 && off < n) {
        const double x = ACC ? acc[off] + v : v;
        s += x * x;
      }
    });
  } else {
    const int nr = scae_sums::owned_ranges(jobs, g, n, r_lo, r_hi, &r_n);
    s = stream_sq<true, ACC>(g, n, head, blockIdx.x - sum_blocks, gridDim.x - sum_blocks, r_lo,
                             r_hi, nr, acc);
  }
  const double tot = scae_clip::block_sum_f64(s, red2);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void grad_sq_sums_kernel(float *g, long n, int head,
                                                           double *partials,
                                                           scae_sums::Jobs jobs, int sum_blocks) {
  grad_sq_sums<false>(g, n, head, partials, jobs, sum_blocks, nullptr);
}
__global__ __launch_bounds__(256) void grad_sq_sums_acc_kernel(float *g, long n, int head,
                                                               double *partials,
                                                               scae_sums::Jobs jobs,
                                                               int sum_blocks, const float *acc) {
  grad_sq_sums<true>(g, n, head, partials, jobs, sum_blocks, acc);
}

// -> the streaming workgroups for n elements (a function of n only), or < 0
int stream_blocks(int64_t n, const float *grad, int &head) {
  if (!(grad && n > 0 && n < (1l << 31) && ((size_t)grad & 3) == 0)) return -1;
  head = (int)((16 - ((size_t)grad & 15)) & 15) / 4;
  if (head > n) head = (int)n;
  const long per = 256l * UNROLL;   // float4 per workgroup and round
  long blocks = ((n - head) / 4 + per - 1) / per;
  return (int)(blocks < 1 ? 1 : (blocks > MAX_STREAM ? MAX_STREAM : blocks));
}
}  // namespace

extern "C" int scae_grad_sq_partials_f32(const float *grad, int64_t n, double *partials,
                                         int max_partials, int *n_partials, void *stream) {
  int head = 0;
  const int blocks = stream_blocks(n, grad, head);
  SCAE_REQUIRE(blocks > 0 && partials && n_partials && blocks <= max_partials);
  *n_partials = blocks;
  scae::launch(grad_sq_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grad,
               (long)n, head, partials);
  return scae_launch_status();
}

extern "C" int scae_grad_sq_partials_sums_f32(float *grad, int64_t n, double *partials,
                                              int max_partials, int *n_partials,
                                              const scae_sum_job *jobs, int n_jobs,
                                              void *stream) {
  int head = 0;
  const int blocks = stream_blocks(n, grad, head);
  SCAE_REQUIRE(blocks > 0 && partials && n_partials);
  scae_sums::Jobs js;
  const int sum_blocks = scae_sums::fill_jobs(js, jobs, n_jobs);
  SCAE_REQUIRE(sum_blocks > 0 && sum_blocks + blocks <= max_partials);
  *n_partials = sum_blocks + blocks;
  scae::launch(grad_sq_sums_kernel, dim3((unsigned)(sum_blocks + blocks)), dim3(256), 0,
               (hipStream_t)stream, grad, (long)n, head, partials, js, sum_blocks);
  return scae_launch_status();
}

// the accumulate forms: the squares of acc + g (acc: n floats at grad's phase in a 16-byte line)
extern "C" int scae_grad_sq_acc_partials_f32(const float *grad, const float *acc, int64_t n,
                                             double *partials, int max_partials, int *n_partials,
                                             void *stream) {
  int head = 0;
  const int blocks = stream_blocks(n, grad, head);
  SCAE_REQUIRE(blocks > 0 && acc && ((size_t)acc & 15) == ((size_t)grad & 15) && partials &&
               n_partials && blocks <= max_partials);
  *n_partials = blocks;
  scae::launch(grad_sq_acc_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
               grad, acc, (long)n, head, partials);
  return scae_launch_status();
}

extern "C" int scae_grad_sq_acc_partials_sums_f32(float *grad, const float *acc, int64_t n,
                                                  double *partials, int max_partials,
                                                  int *n_partials, const scae_sum_job *jobs,
                                                  int n_jobs, void *stream) {
  int head = 0;
  const int blocks = stream_blocks(n, grad, head);
  SCAE_REQUIRE(blocks > 0 && acc && ((size_t)acc & 15) == ((size_t)grad & 15) && partials &&
               n_partials);
  scae_sums::Jobs js;
  const int sum_blocks = scae_sums::fill_jobs(js, jobs, n_jobs);
  SCAE_REQUIRE(sum_blocks > 0 && sum_blocks + blocks <= max_partials);
  *n_partials = sum_blocks + blocks;
  scae::launch(grad_sq_sums_acc_kernel, dim3((unsigned)(sum_blocks + blocks)), dim3(256), 0,
               (hipStream_t)stream, grad, (long)n, head, partials, js, sum_blocks, acc);
  return scae_launch_status();
}
