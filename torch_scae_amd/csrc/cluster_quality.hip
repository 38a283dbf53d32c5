// Cluster quality for gfx950 (cluster_quality.py): the exact silhouette of a labelling -- an
// all-pairs pass over the features -- its mean per cluster and overall, and the per-cluster
// centroid / scatter tables behind the Calinski-Harabasz and Davies-Bouldin indices.
//
// MUST BE COMPILED WITH -ffp-contract=off (csrc/Makefile gives this file the flag): the fp64
// sums and quotients below are each rounded once, which is what numpy does; under HIP's default
// -ffp-contract=fast the backend would fuse products into sums.  The squared distance is
// row_dist_dev.h's, which keeps contraction off for itself.
// sqrtf / sqrt / the fp64 divide are the correctly rounded ones (hipcc's default, no fast-math).
//
// The rows arrive sorted by (label, row) (a stable integer sort, cluster_quality.py): cluster c
// is the positions off[c] .. off[c + 1] - 1 and a position's original row is order[p].
//
//   cq_labels_kernel      labels -> int32 clamped into [0, k), the ones outside counted (an
//                         integer atomic, as the contingency table counts them);
//   cq_silhouette_kernel  row_dist_dev.h's tile and distance with one row i per lane over
//                         every sorted row (the tile rows' clusters staged beside it), d_ij =
//                         sqrtf(d2) widened to fp64 and added to the lane's ONE running sum
//                         of the cluster being streamed.
//                         Every lane meets the same row at the same time, so the end of a
//                         cluster is wave-uniform: there the sum becomes a's numerator (own
//                         cluster) or, over n_c, a candidate for the running (b, nearest) minimum
//                         (strictly less: clusters ascend, ties stay with the lowest).  The self
//                         pair is skipped by position.  No per-cluster array, no atomics, no
//                         (N, k) table; the base is never split, so D_i(c) is the sum in
//                         ascending row order whatever the grid;
//   cq_score_kernel       workgroup c < k: the mean of cluster c's values in row order (they are
//                         contiguous in the sorted copy); workgroup k: the mean of all values in
//                         row order.  One thread adds, the others stage 256 values at a time;
//   cq_dispersion_kernel  workgroup c: n_c, the mean m_c (fp64; row r of the cluster goes to
//                         slice r mod S, S = 256 / F, a slice adds its rows in order, the slices
//                         are added in order), then W_c = sum |x_i - m_c|^2 and S_c = the mean of
//                         |x_i - m_c| (row r to thread r mod 256, the threads added in order).
#include "common.h"
#include "row_dist_dev.h"

namespace {
using namespace scae_rows;
constexpr int TQ = 64;             // rows of a silhouette workgroup, one per lane: one wave, so
                                   // that N = 10^4 still gives 157 workgroups
constexpr int TILE_ROWS = TILE_FLOATS / 4;   // rows of a tile at most (F4 = 4)
constexpr int FXR = 32;            // features held in registers by the register form
constexpr int TR = 256;            // score / dispersion / label workgroup

__global__ __launch_bounds__(TR) void cq_labels_kernel(const int64_t *labels, int64_t N, int k,
                                                       int *lab32, int *outside) {
  for (int64_t n = (int64_t)blockIdx.x * TR + threadIdx.x; n < N; n += (int64_t)gridDim.x * TR) {
    const int64_t l = labels[n];
    const bool ok = l >= 0 && l < k;
    lab32[n] = ok ? (int)l : (l < 0 ? 0 : k - 1);
    if (!ok) atomicAdd(outside, 1);
  }
}

// grid ceil(N / TQ)
template <int FX>
__global__ __launch_bounds__(TQ) void cq_silhouette_kernel(
    const float *xs, const int *ls, const int64_t *off, const int64_t *order, int64_t N, int F,
    double *values, double *a_out, double *b_out, int64_t *nearest, double *sorted_values) {
  __shared__ __attribute__((aligned(16))) float tile[TILE_FLOATS];
  __shared__ int tl[TILE_ROWS + 1];   // the tile rows' clusters and the next row's (-1: the end)
  const int t = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * TQ + t;
  const bool active = p < N;
  const TileGeom tg = tile_geom(F);
  const float *xp = xs + (active ? p : 0) * F;
  float xr[FX > 0 ? FX : 1];
  if constexpr (FX > 0) {
#pragma unroll
    for (int f = 0; f < FX; ++f) xr[f] = f < F ? xp[f] : 0.f;
  }
  const int own = ls[active ? p : 0];
  double run = 0.0, own_sum = 0.0, b = __longlong_as_double(0x7FF0000000000000ll);
  int near = -1;
  for (int64_t row0 = 0; row0 < N; row0 += tg.TB) {
    const int64_t left = N - row0;
    const int rows = left < tg.TB ? (int)left : tg.TB;
    __syncthreads();   // (the previous tile has been read)
    // (row_dist_dev.h's load_tile writes the same tile; this 32-bit row test is 2 % faster here)
    for (int e = t; e < tg.TB * tg.F4; e += TQ) {
      const int r = e / tg.F4, f = e - r * tg.F4;
      tile[e] = (f < F && r < rows) ? xs[(row0 + r) * F + f] : 0.f;
    }
    for (int r = t; r <= rows; r += TQ) tl[r] = row0 + r < N ? ls[row0 + r] : -1;
    __syncthreads();
    if (!active) continue;
    for (int r = 0; r < rows; r += 4) {
      // four rows at a time: independent sums (rows past the end are zeros in LDS)
      float d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) d[u] = dist2<FX>(xr, xp, tile + (r + u) * tg.F4, F, tg.F4);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (r + u >= rows) break;
        const double e = (double)sqrtf(d[u]);
        if (row0 + r + u != p) run += e;
        const int c = tl[r + u];
        if (tl[r + u + 1] != c) {   // the cluster ends here: the same for every lane
          if (c == own) {
            own_sum = run;
          } else {
            const double m = run / (double)(off[c + 1] - off[c]);
            if (m < b) b = m, near = c;
          }
          run = 0.0;
        }
      }
    }
  }
  if (!active) return;
  const int64_t n_own = off[own + 1] - off[own];
  const double a = n_own > 1 ? own_sum / (double)(n_own - 1) : 0.0;
  double s = 0.0;
  if (n_own > 1 && near >= 0) {
    const double mx = a > b ? a : b;
    if (mx > 0.0) s = (b - a) / mx;
  }
  const int64_t i = order[p];
  values[i] = s;
  a_out[i] = a;
  b_out[i] = b;
  nearest[i] = near;
  sorted_values[p] = s;
}

// grid k + 1: scores[c] = the mean of cluster c's values (NaN when empty), scores[k] = the mean
// of all values; both sums in row order from 0
__global__ __launch_bounds__(TR) void cq_score_kernel(const double *values,
                                                      const double *sorted_values,
                                                      const int64_t *off, int64_t N, int k,
                                                      double *scores) {
  __shared__ double buf[TR];
  const int t = threadIdx.x, c = blockIdx.x;
  const double *src = c < k ? sorted_values : values;
  const int64_t lo = c < k ? off[c] : 0, hi = c < k ? off[c + 1] : N;
  double sum = 0.0;
  for (int64_t r0 = lo; r0 < hi; r0 += TR) {
    __syncthreads();
    if (r0 + t < hi) buf[t] = src[r0 + t];
    __syncthreads();
    if (t == 0) {
      const int n = hi - r0 < TR ? (int)(hi - r0) : TR;
      for (int u = 0; u < n; ++u) sum += buf[u];
    }
  }
  if (t == 0)
    scores[c] = hi > lo ? sum / (double)(hi - lo) : __longlong_as_double(0x7FF8000000000000ll);
}

// grid k: table row c = (n_c, m_c (F), W_c, S_c); an empty cluster gets (0, NaN.., 0, NaN)
__global__ __launch_bounds__(TR) void cq_dispersion_kernel(const float *xs, const int64_t *off,
                                                           int F, double *table) {
  __shared__ double part[TR], part2[TR], mean[TR];
  const int t = threadIdx.x, c = blockIdx.x;
  const int64_t lo = off[c], hi = off[c + 1], n = hi - lo;
  double *row = table + (int64_t)c * (F + 3);
  if (n == 0) {
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    if (t < F) row[1 + t] = nan;
    if (t == 0) row[0] = 0.0, row[F + 1] = 0.0, row[F + 2] = nan;
    return;
  }
  const int S = TR / F, sl = t / F, f = t - sl * F;
  double sum = 0.0;
  if (sl < S)
    for (int64_t r = lo + sl; r < hi; r += S) sum += (double)xs[r * F + f];
  part[t] = sum;
  __syncthreads();
  if (t < F) {
    double all = 0.0;
    for (int u = 0; u < S; ++u) all += part[u * F + t];
    mean[t] = all / (double)n;
    row[1 + t] = mean[t];
  }
  __syncthreads();
  double w = 0.0, sd = 0.0;
  for (int64_t r = lo + t; r < hi; r += TR) {
    double d2 = 0.0;
    for (int g = 0; g < F; ++g) {
      const double u = (double)xs[r * F + g] - mean[g];
      d2 += u * u;
    }
    w += d2;
    sd += sqrt(d2);
  }
  part[t] = w;
  part2[t] = sd;
  __syncthreads();
  if (t == 0) {
    double W = 0.0, Sd = 0.0;
    for (int u = 0; u < TR; ++u) W += part[u], Sd += part2[u];
    row[0] = (double)n;
    row[F + 1] = W;
    row[F + 2] = Sd / (double)n;
  }
}
}  // namespace

extern "C" int scae_cluster_quality_supported(int64_t N, int F, int64_t k) {
  const int64_t lim = (int64_t)1 << 31;
  return N >= 1 && N < lim && F >= 1 && F <= SCAE_CLUSTER_QUALITY_MAX_F && k >= 1 && k < lim - 1;
}

extern "C" int scae_cluster_quality_labels(const int64_t *labels, int64_t N, int64_t k,
                                           int *lab32, int *outside, void *stream) {
  SCAE_REQUIRE(labels && lab32 && outside);
  if (!scae_cluster_quality_supported(N, 1, k)) return SCAE_ERR_UNSUPPORTED;
  const int64_t blocks = (N + TR - 1) / TR;
  scae::launch(cq_labels_kernel, dim3(blocks < 1024 ? (unsigned)blocks : 1024u), dim3(TR), 0,
               (hipStream_t)stream, labels, N, (int)k, lab32, outside);
  return scae_launch_status();
}

extern "C" int scae_cluster_quality_silhouette_f32(const float *xs, const int *ls,
                                                   const int64_t *off, const int64_t *order,
                                                   int64_t N, int F, int64_t k, double *values,
                                                   double *a, double *b, int64_t *nearest,
                                                   double *sorted_values, double *scores,
                                                   void *stream) {
  SCAE_REQUIRE(xs && ls && off && order && values && a && b && nearest && sorted_values &&
               scores);
  if (!scae_cluster_quality_supported(N, F, k)) return SCAE_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((N + TQ - 1) / TQ));
  if (F <= FXR)
    scae::launch(cq_silhouette_kernel<FXR>, grid, dim3(TQ), 0, st, xs, ls, off, order, N, F,
                 values, a, b, nearest, sorted_values);
  else
    scae::launch(cq_silhouette_kernel<0>, grid, dim3(TQ), 0, st, xs, ls, off, order, N, F,
                 values, a, b, nearest, sorted_values);
  scae::launch(cq_score_kernel, dim3((unsigned)(k + 1)), dim3(TR), 0, st, (const double *)values,
               (const double *)sorted_values, off, N, (int)k, scores);
  return scae_launch_status();
}

extern "C" int scae_cluster_quality_dispersion_f32(const float *xs, const int64_t *off,
                                                   int64_t N, int F, int64_t k, double *table,
                                                   void *stream) {
  SCAE_REQUIRE(xs && off && table);
  if (!scae_cluster_quality_supported(N, F, k)) return SCAE_ERR_UNSUPPORTED;
  scae::launch(cq_dispersion_kernel, dim3((unsigned)k), dim3(TR), 0, (hipStream_t)stream, xs,
               off, F, table);
  return scae_launch_status();
}
