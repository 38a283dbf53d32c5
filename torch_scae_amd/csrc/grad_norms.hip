// Per-parameter gradient norms (Lightning's Trainer(track_grad_norm=p)): one p-norm per segment
// of a flat buffer and their total, written as one row of a device ring (scae_hip.h,
// scae_segment_norms_f32).  Two launches.  The chunk launch: a wave per chunk (at most
// SCAE_NORM_CHUNK elements of one segment), four waves a workgroup, each workgroup a group of
// consecutive chunks from the caller's tables; a lane reads float4 on the 16-byte aligned
// interior of its chunk and the first lanes the scalar head and tail, every term goes to fp64
// (a square of an fp32 value is exact there), a butterfly sums the wave, lane 0 writes the
// chunk's partial.  The finish launch: one workgroup, sixteen lanes a segment, reduces each
// segment's partials in chunk order, writes the row and advances the ring's cursor.  No atomics,
// no arrival counter, no fence: the order of every sum is a function of the tables, so two runs
// give the same bits, and a non-finite element stays in its own segment's partials.
#include "common.h"

namespace {
constexpr int CH = SCAE_NORM_CHUNK;
constexpr int QUADS = CH / 4 / 64;   // float4 loads in flight per lane
static_assert(CH == QUADS * 4 * 64, "a chunk is a whole number of float4 per lane");

// KIND: 2, 1 or SCAE_NORM_INF.  term: one element's share; join: of two partial results (a
// NaN on either side stays: fmax would drop it)
template <int KIND>
__device__ __forceinline__ double term(float x) {
  if (KIND == 2) return (double)x * (double)x;
  return (double)fabsf(x);
}
template <int KIND>
__device__ __forceinline__ double join(double a, double b) {
  if (KIND != SCAE_NORM_INF) return a + b;
  return (b > a || b != b) ? b : a;
}
template <int KIND>
__device__ __forceinline__ double term4(float4 v) {
  return join<KIND>(join<KIND>(term<KIND>(v.x), term<KIND>(v.y)),
                    join<KIND>(term<KIND>(v.z), term<KIND>(v.w)));
}
template <int KIND>
__device__ __forceinline__ double finish(double raw, float scale) {
  return (double)scale * (KIND == 2 ? sqrt(raw) : raw);
}

template <int KIND, bool ACC>
__global__ __launch_bounds__(256) void norm_chunks_kernel(const float *src, const float *acc,
                                                          long n, const int2 *chunks,
                                                          int n_chunks, const int *group_first,
                                                          double *partials) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int c0 = group_first[blockIdx.x], c1 = group_first[blockIdx.x + 1];
  c0 = c0 < 0 ? 0 : c0;
  c1 = c1 > n_chunks ? n_chunks : c1;
  for (int c = c0 + wave; c < c1; c += 4) {   // (wave-uniform)
    const int2 ch = chunks[c];
    const long b = ch.x;
    const int len = ch.y;
    double s = 0.0;
    if (b < 0 || len < 1 || len > CH || b + len > n) {
      s = __builtin_nan("");   // a chunk outside the buffer: nothing read, visibly wrong
    } else {
      const float *g = src + b, *a = ACC ? acc + b : nullptr;
      int head = (int)((16 - ((size_t)g & 15)) & 15) / 4;
      head = head > len ? len : head;
      const int n4 = (len - head) >> 2, tail = len - head - (n4 << 2);
      const float4 *g4 = reinterpret_cast<const float4 *>(g + head);
      const float4 *a4 = reinterpret_cast<const float4 *>(a + head);
      float4 v[QUADS];
#pragma unroll
      for (int u = 0; u < QUADS; ++u) {
        const int i = lane + 64 * u;
        v[u] = i < n4 ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      if (ACC) {
#pragma unroll
        for (int u = 0; u < QUADS; ++u) {
          const int i = lane + 64 * u;
          if (i < n4) {
            const float4 w = a4[i];
            v[u] = make_float4(w.x + v[u].x, w.y + v[u].y, w.z + v[u].z, w.w + v[u].w);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < QUADS; ++u) s = join<KIND>(s, term4<KIND>(v[u]));
      // scalar edges: lanes [0, head) the head, the next `tail` lanes the tail
      if (lane < head + tail) {
        const int k = lane < head ? lane : head + (n4 << 2) + (lane - head);
        s = join<KIND>(s, term<KIND>(ACC ? a[k] + g[k] : g[k]));
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s = join<KIND>(s, __shfl_xor(s, m, 64));
    if (lane == 0) partials[c] = s;
  }
}

// one workgroup of 64 sub-groups of 16 lanes; sub-group g takes segments g, g + 64, ...
template <int KIND>
__global__ __launch_bounds__(1024) void norm_finish_kernel(const double *partials, int n_chunks,
                                                           const int *seg_first, int n_segs,
                                                           float scale, float *ring,
                                                           long long *cursor, int capacity) {
  __shared__ double tot[64];
  __shared__ long long at;
  if (threadIdx.x == 0) at = cursor ? *cursor : 0;
  __syncthreads();
  const long long count = at;
  float *out = ring + (count % capacity) * (long long)(n_segs + 1);
  const int sub = threadIdx.x >> 4, j = threadIdx.x & 15;
  double t = 0.0;
  for (int s = sub; s < n_segs; s += 64) {
    int c0 = seg_first[s], c1 = seg_first[s + 1];
    c0 = c0 < 0 ? 0 : c0;
    c1 = c1 > n_chunks ? n_chunks : c1;
    double v = 0.0;
    for (int c = c0 + j; c < c1; c += 16) v = join<KIND>(v, partials[c]);
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v = join<KIND>(v, __shfl_xor(v, m, 64));
    t = join<KIND>(t, v);
    if (j == 0) out[s] = (float)finish<KIND>(v, scale);
  }
  if (j == 0) tot[sub] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = tot[0];
    for (int i = 1; i < 64; ++i) a = join<KIND>(a, tot[i]);
    out[n_segs] = (float)finish<KIND>(a, scale);
    if (cursor) *cursor = count + 1;
  }
}

template <int KIND>
void launch_kind(const float *src, const float *acc, long n, const int2 *chunks, int n_chunks,
                 const int *group_first, int n_groups, const int *seg_first, int n_segs,
                 float scale, double *partials, float *ring, long long *cursor, int capacity,
                 hipStream_t st) {
  if (acc)
    scae::launch(norm_chunks_kernel<KIND, true>, dim3((unsigned)n_groups), dim3(256), 0, st, src,
                 acc, n, chunks, n_chunks, group_first, partials);
  else
    scae::launch(norm_chunks_kernel<KIND, false>, dim3((unsigned)n_groups), dim3(256), 0, st,
                 src, acc, n, chunks, n_chunks, group_first, partials);
  scae::launch(norm_finish_kernel<KIND>, dim3(1), dim3(1024), 0, st,
               (const double *)partials, n_chunks, seg_first, n_segs, scale, ring, cursor,
               capacity);
}
}  // namespace

extern "C" int scae_segment_norms_chunk(void) { return SCAE_NORM_CHUNK; }

extern "C" int scae_segment_norms_f32(const float *src, const float *acc, int64_t n,
                                      const int32_t *chunks, int n_chunks,
                                      const int32_t *group_first, int n_groups,
                                      const int32_t *seg_first, int n_segs, int norm_kind,
                                      float scale, double *partials, float *ring,
                                      int64_t *cursor, int capacity, void *stream) {
  SCAE_REQUIRE(src && ((size_t)src & 3) == 0 && n > 0 && n < (1ll << 31));
  SCAE_REQUIRE(!acc || ((size_t)acc & 15) == ((size_t)src & 15));
  SCAE_REQUIRE(chunks && ((size_t)chunks & 7) == 0 && group_first && seg_first && partials &&
               ring);
  SCAE_REQUIRE(n_chunks > 0 && n_groups > 0 && n_groups <= n_chunks && n_segs > 0 &&
               n_segs <= n_chunks && capacity > 0);
  SCAE_REQUIRE(scale >= 0.f);
  const int2 *ch = reinterpret_cast<const int2 *>(chunks);
  long long *cur = reinterpret_cast<long long *>(cursor);
  hipStream_t st = (hipStream_t)stream;
  switch (norm_kind) {
    case 2:
      launch_kind<2>(src, acc, (long)n, ch, n_chunks, group_first, n_groups, seg_first, n_segs,
                     scale, partials, ring, cur, capacity, st);
      break;
    case 1:
      launch_kind<1>(src, acc, (long)n, ch, n_chunks, group_first, n_groups, seg_first, n_segs,
                     scale, partials, ring, cur, capacity, st);
      break;
    case SCAE_NORM_INF:
      launch_kind<SCAE_NORM_INF>(src, acc, (long)n, ch, n_chunks, group_first, n_groups,
                                 seg_first, n_segs, scale, partials, ring, cur, capacity, st);
      break;
    default:
      return SCAE_ERR_BAD_ARG;
  }
  return scae_launch_status();
}
