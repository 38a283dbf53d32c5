// Gradient accumulation over several batches (Lightning's Trainer(accumulate_grad_batches=k)):
// on a batch that does not end its group the training step's last launch is acc += g over the
// flat gradient buffer instead of the optimiser pass; the group's last batch ends in the
// accumulate forms of the optimiser passes (optimizer.hip, optimizer_adam.hip), which read
// g_eff = grad_scale (acc + g) and leave acc = 0 behind -- so no batch needs a "first of its
// group" form of this pass.  fp32 adds in batch order: acc = g_1 + g_2 + ..., the same bits
// however the grid is cut.
// The sums form hosts the step's last column sums (scae_sums::Jobs), as the optimiser's
// rmsprop_sums_kernel does: the sum workgroups head the grid, write their gradient slots and
// add what they write into acc; the streaming workgroups behind them skip exactly those
// destination ranges (scae_sums::owned_ranges).
#include "sum_rows_dev.h"

namespace {
constexpr int MAX_STREAM = 1024;  // streaming workgroups
constexpr int UNROLL = 4;         // float4 loads of each stream in flight per thread

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// this workgroup's share (`blk` of `nblk`) of acc[0, n) += g[0, n): `head` leading elements
// bring both (equally misaligned) buffers to a 16-byte boundary, then float4 lanes, then the
// tail; SKIP: without the elements of the nr ranges [r_lo, r_hi)
template <bool SKIP>
__device__ __forceinline__ void stream_add(float *acc, const float *g, long n, int head, int blk,
                                           int nblk, const int *r_lo, const int *r_hi, int nr) {
  const long stride = (long)nblk * blockDim.x, tid = (long)blk * blockDim.x + threadIdx.x;
  const long n4 = (n - head) >> 2;
  float4 *a4 = reinterpret_cast<float4 *>(acc + head);
  const float4 *g4 = reinterpret_cast<const float4 *>(g + head);
  long i = tid;
  if (!SKIP) {
    for (; i + (UNROLL - 1) * stride < n4; i += UNROLL * stride) {
      float4 a[UNROLL], v[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) a[u] = a4[i + u * stride], v[u] = g4[i + u * stride];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) a4[i + u * stride] = add4(a[u], v[u]);
    }
  }
  for (; i < n4; i += stride) {
    const float4 a = a4[i], v = g4[i];
    const int own = SKIP ? scae_sums::quad_owned(head + 4 * (int)i, r_lo, r_hi, nr) : 0;
    if (own == 0) {
      a4[i] = add4(a, v);
    } else if (own != 15) {   // (rare: a quad that straddles the edge of an owned range)
      const float ae[4] = {a.x, a.y, a.z, a.w}, ve[4] = {v.x, v.y, v.z, v.w};
      float *q = acc + head + 4 * i;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (!((own >> u) & 1)) q[u] = ae[u] + ve[u];
    }
  }
  // scalar edges: [0, head) and [head + 4*n4, n)
  const long tail0 = head + (n4 << 2), edge = head + (n - tail0);
  for (long e = tid; e < edge; e += stride) {
    const long k = e < head ? e : tail0 + (e - head);
    if (SKIP && scae_sums::owned(k, r_lo, r_hi, nr)) continue;
    acc[k] = acc[k] + g[k];
  }
}

__global__ __launch_bounds__(256) void accumulate_kernel(float *acc, const float *g, long n,
                                                         int head) {
  stream_add<false>(acc, g, n, head, blockIdx.x, gridDim.x, nullptr, nullptr, 0);
}

__global__ __launch_bounds__(256) void accumulate_sums_kernel(float *acc, float *g, long n,
                                                              int head, scae_sums::Jobs jobs,
                                                              int sum_blocks) {
  __shared__ float red[scae_sums::NT];
  __shared__ int r_lo[scae_sums::MAXR], r_hi[scae_sums::MAXR];
  __shared__ int r_n;
  if ((int)blockIdx.x < sum_blocks) {   // workgroup-uniform
    scae_sums::sum_block(jobs, blockIdx.x, red, [&](float *dst, float v) {
      *dst = v;
      const long off = dst - g;
      if (off >= 0 && off < n) acc[off] = acc[off] + v;
    });
    return;
  }
  const int nr = scae_sums::owned_ranges(jobs, g, n, r_lo, r_hi, &r_n);
  stream_add<true>(acc, g, n, head, blockIdx.x - sum_blocks, gridDim.x - sum_blocks, r_lo, r_hi,
                   nr);
}

// -> the streaming workgroups for n elements, or < 0 (bad arguments); `head` as stream_add's
int stream_blocks(const float *acc, const float *grad, int64_t n, int &head) {
  if (!(acc && grad && n > 0 && n < (1l << 31))) return -1;
  const size_t phase = (size_t)grad & 15;
  if ((phase & 3) || ((size_t)acc & 15) != phase) return -1;
  head = (int)((16 - phase) & 15) / 4;
  if (head > n) head = (int)n;
  const long per = 256l * UNROLL;   // float4 per workgroup and round
  const long blocks = ((n - head) / 4 + per - 1) / per;
  return (int)(blocks < 1 ? 1 : (blocks > MAX_STREAM ? MAX_STREAM : blocks));
}
}  // namespace

extern "C" int scae_grad_accumulate_f32(float *acc, const float *grad, int64_t n, void *stream) {
  int head = 0;
  const int blocks = stream_blocks(acc, grad, n, head);
  SCAE_REQUIRE(blocks > 0);
  scae::launch(accumulate_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, acc,
               grad, (long)n, head);
  return scae_launch_status();
}

extern "C" int scae_grad_accumulate_sums_f32(float *acc, float *grad, int64_t n,
                                             const scae_sum_job *jobs, int n_jobs,
                                             void *stream) {
  int head = 0;
  const int blocks = stream_blocks(acc, grad, n, head);
  SCAE_REQUIRE(blocks > 0);
  scae_sums::Jobs js;
  const int sum_blocks = scae_sums::fill_jobs(js, jobs, n_jobs);
  SCAE_REQUIRE(sum_blocks > 0);
  scae::launch(accumulate_sums_kernel, dim3((unsigned)(sum_blocks + blocks)), dim3(256), 0,
               (hipStream_t)stream, acc, grad, (long)n, head, js, sum_blocks);
  return scae_launch_status();
}
