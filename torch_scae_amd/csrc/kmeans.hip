// k-means for gfx950 (cluster.py): the unsupervised classification of SCAE's capsule
// activations -- Lloyd iterations of all restarts in one grid (grid.y = restart), k-means++
// seeding, nearest-centroid assignment and the cluster/class contingency table.
//
// One Lloyd iteration is two launches:
//   km_assign_kernel   one point per lane, the restart's centroids in LDS (every lane reads the
//                      same address: a broadcast); the tile's points are ordered by label
//                      (counting sort in LDS) and each thread adds the points of its
//                      (cluster, feature) pairs into LDS in point order, so the workgroup's
//                      partial sums, counts, changed count and fp64 inertia have a fixed order;
//   km_update_kernel   one workgroup per restart: the G partials summed in g order, the stop
//                      decision (no assignment changed, or max_iter reached) and the new means.
// No float atomics: two runs give the same bits.  A stopped restart's launches exit at once,
// so the host can enqueue several iterations and read one counter per chunk.  The wave sums
// are reduce_f64_dev.h's.
#include "common.h"
#include "noise_dev.h"
#include "reduce_f64_dev.h"

namespace {
constexpr int TP = 256;    // points per tile = lanes of an assignment workgroup
constexpr int NTU = 1024;  // update workgroup
constexpr int NTP = 1024;  // k-means++ workgroup
constexpr int MAX_GROUPS = 2048;  // assignment workgroups of all restarts together
constexpr uint32_t TAG_KMPP = 0x4B4D5050u;
constexpr int ST = SCAE_KMEANS_STATE_INTS;

using scae_reduce::wave_sum_f64;
using scae_reduce::wave_sum_i32;

// squared distance of the point whose features sit in xr (FX > 0: registers) or at xp (FX == 0)
// to the centroid at cc (LDS), in f order.  An fmaf accumulation: NOT row_dist_dev.h's
// three-roundings rule, and the labels' bits depend on it -- the two are not to be unified
template <int FX>
__device__ __forceinline__ float dist2_fma(const float (&xr)[FX > 0 ? FX : 1], const float *xp,
                                           const float *cc, int F) {
  float d = 0.f;
  if constexpr (FX > 0) {
#pragma unroll
    for (int f = 0; f < FX; ++f)
      if (f < F) {
        const float u = xr[f] - cc[f];
        d = fmaf(u, u, d);
      }
  } else {
    for (int f = 0; f < F; ++f) {
      const float u = xp[f] - cc[f];
      d = fmaf(u, u, d);
    }
  }
  return d;
}

// nearest centroid of point xp: (index, distance); ties to the lowest index
template <int FX>
__device__ __forceinline__ int nearest(const float *xp, const float *cs, int k, int F,
                                       float &best_d) {
  float xr[FX > 0 ? FX : 1];
  if constexpr (FX > 0) {
#pragma unroll
    for (int f = 0; f < FX; ++f) xr[f] = f < F ? xp[f] : 0.f;
  }
  int best = 0;
  float bd = INFINITY;
  for (int c = 0; c < k; ++c) {
    const float d = dist2_fma<FX>(xr, xp, cs + c * F, F);
    if (d < bd) bd = d, best = c;
  }
  best_d = bd;
  return best;
}

size_t assign_lds(int k, int F) {
  return (size_t)2 * k * F * sizeof(float) + (size_t)(3 * TP + 2 * k + 2) * sizeof(int) +
         (TP / SCAE_WAVE) * sizeof(double);
}

// grid (G, R): workgroup g of restart r takes tiles g, g + G, ...  Without part_sum (assign
// only) it writes labels alone.
template <int FX>
__global__ __launch_bounds__(TP) void km_assign_kernel(scae_kmeans_desc d) {
  const int r = blockIdx.y, g = blockIdx.x, t = threadIdx.x;
  if (d.state && d.state[r * ST]) return;  // this restart has stopped
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int F = d.F, k = d.k, kF = k * F, G = d.G;
  const int64_t N = d.N;
  const bool parts = d.part_sum != nullptr;
  float *cs = smem;                 // (k, F) centroids
  float *acc = cs + kF;             // (k, F) this workgroup's sums
  int *cnt = reinterpret_cast<int *>(acc + kF);  // (k) its counts
  int *tcnt = cnt + k;              // (k) the tile's counts
  int *lab = tcnt + k;              // (TP) the tile's labels (-1: no point)
  int *order = lab + TP;            // (TP) the tile's points by label
  int *start = order + TP;          // (TP) where each cluster's points begin in order
  int *s_changed = start + TP;
  double *red = reinterpret_cast<double *>(s_changed + 2);
  const float *C = d.centroids + (size_t)r * kF;
  for (int i = t; i < kF; i += TP) cs[i] = C[i], acc[i] = 0.f;
  for (int c = t; c < k; c += TP) cnt[c] = 0;
  if (t == 0) *s_changed = 0;
  __syncthreads();
  int changed = 0;
  double inertia = 0.0;
  int64_t *labels = d.labels + (size_t)r * N;
  const int64_t ntiles = (N + TP - 1) / TP;
  for (int64_t tile = g; tile < ntiles; tile += G) {
    const int64_t n = tile * TP + t;
    int best = -1;
    if (n < N) {
      float bd;
      best = nearest<FX>(d.x + n * F, cs, k, F, bd);
      if (parts) {
        changed += labels[n] != best;
        inertia += (double)bd;
      }
      labels[n] = best;
    }
    if (!parts) continue;
    lab[t] = best;
    __syncthreads();
    // counting sort of the tile by label, stable: thread c counts, then places, in point order
    for (int c = t; c < k; c += TP) {
      int m = 0;
      for (int i = 0; i < TP; ++i) m += lab[i] == c;
      tcnt[c] = m;
    }
    __syncthreads();
    if (t == 0) {
      int s = 0;
      for (int c = 0; c < k; ++c) start[c] = s, s += tcnt[c];
    }
    __syncthreads();
    for (int c = t; c < k; c += TP) {
      int at = start[c];
      for (int i = 0; i < TP; ++i)
        if (lab[i] == c) order[at++] = i;
      cnt[c] += tcnt[c];
    }
    __syncthreads();
    // thread-owned (cluster, feature) pairs: the cluster's points in point order
    const float *xt = d.x + tile * TP * F;
    for (int p = t; p < kF; p += TP) {
      const int c = p / F, f = p - c * F;
      const int b = start[c], e = b + tcnt[c];
      float s = acc[p];
      for (int j = b; j < e; ++j) s += xt[(size_t)order[j] * F + f];
      acc[p] = s;
    }
    __syncthreads();  // (lab / order / start are rewritten by the next tile)
  }
  if (!parts) return;
  // the workgroup's partials: changed (integer: any order), inertia (waves in a fixed tree,
  // then wave order)
  changed = wave_sum_i32(changed);
  inertia = wave_sum_f64(inertia);
  const int wid = t / SCAE_WAVE, lane = t % SCAE_WAVE;
  if (lane == 0) {
    atomicAdd(s_changed, changed);
    red[wid] = inertia;
  }
  __syncthreads();
  const size_t rg = (size_t)r * G + g;
  float *ps = d.part_sum + rg * kF;
  for (int i = t; i < kF; i += TP) ps[i] = acc[i];
  for (int c = t; c < k; c += TP) d.part_count[rg * k + c] = cnt[c];
  if (t == 0) {
    double s = 0.0;
    for (int w = 0; w < TP / SCAE_WAVE; ++w) s += red[w];
    d.part_inertia[rg] = s;
    d.part_changed[rg] = *s_changed;
  }
}

// grid (R): the restart's partials in g order, the stop decision, the new means
__global__ __launch_bounds__(NTU) void km_update_kernel(scae_kmeans_desc d) {
  const int r = blockIdx.x, t = threadIdx.x;
  int *st = d.state + r * ST;
  if (st[0]) return;
  __shared__ int s_stop;
  const int G = d.G, k = d.k, F = d.F, kF = k * F;
  const size_t r0 = (size_t)r * G;
  if (t < SCAE_WAVE) {
    int ch = 0;
    double in = 0.0;
    for (int g = t; g < G; g += SCAE_WAVE) ch += d.part_changed[r0 + g], in += d.part_inertia[r0 + g];
    ch = wave_sum_i32(ch);
    in = wave_sum_f64(in);
    if (t == 0) {
      const int it = st[1] + 1;
      const int stop = ch == 0 || it >= d.max_iter;
      st[1] = it;
      st[3] = ch;
      d.inertia[r] = in;
      if (stop) {
        st[0] = 1;
        st[2] = ch == 0;
        atomicAdd(d.state + d.R * ST, 1);
      }
      s_stop = stop;
    }
  }
  __syncthreads();
  if (s_stop) return;  // the centroids stay those the last assignment used
  float *C = d.centroids + (size_t)r * kF;
  for (int p = t; p < kF; p += NTU) {
    const int c = p / F;
    float s = 0.f;
    int n = 0;
    for (int g = 0; g < G; ++g) {
      s += d.part_sum[(r0 + g) * kF + p];
      n += d.part_count[(r0 + g) * k + c];
    }
    if (n > 0) C[p] = s / (float)n;  // (an empty cluster keeps its centroid)
  }
}

__device__ __forceinline__ float pp_uniform(uint32_t seed, int r, int j) {
  uint32_t c[4] = {(uint32_t)j, 0u, 0u, TAG_KMPP};
  uint32_t k0 = seed, k1 = (uint32_t)r;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    scae_noise::philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return (float)(c[0] >> 8) * (1.0f / 16777216.0f);
}

// grid (R): thread t owns points [t * chunk, (t + 1) * chunk)
__global__ __launch_bounds__(NTP) void km_pp_kernel(const float *x, int64_t N, int F, int k,
                                                    uint32_t seed, float *cent, float *d2,
                                                    int64_t *chosen) {
  const int r = blockIdx.x, t = threadIdx.x;
  __shared__ double tsum[NTP];
  __shared__ float cj[SCAE_KMEANS_MAX_F];
  __shared__ int s_owner;
  __shared__ double s_before, s_target;
  __shared__ int64_t s_idx;
  float *D = d2 + (size_t)r * N;
  const int64_t chunk = (N + NTP - 1) / NTP;
  const int64_t lo = t * chunk < N ? t * chunk : N, hi = lo + chunk < N ? lo + chunk : N;
  for (int64_t n = lo; n < hi; ++n) D[n] = 1.f;
  for (int j = 0; j < k; ++j) {
    double s = 0.0;
    for (int64_t n = lo; n < hi; ++n) s += (double)D[n];
    tsum[t] = s;
    __syncthreads();
    if (t == 0) {
      double total = 0.0;
      for (int i = 0; i < NTP; ++i) total += tsum[i];
      const double target = (double)pp_uniform(seed, r, j) * total;
      double run = 0.0;
      int owner = -1;
      for (int i = 0; i < NTP; ++i) {
        if (run + tsum[i] > target) {
          owner = i;
          break;
        }
        run += tsum[i];
      }
      s_owner = owner, s_before = run, s_target = target, s_idx = N - 1;
    }
    __syncthreads();
    if (t == s_owner) {
      double run = s_before;
      int64_t idx = hi - 1;  // (rounding: the chunk's last point)
      for (int64_t n = lo; n < hi; ++n) {
        run += (double)D[n];
        if (run > s_target) {
          idx = n;
          break;
        }
      }
      s_idx = idx;
    }
    __syncthreads();
    const int64_t idx = s_idx;
    for (int f = t; f < F; f += NTP) {
      cj[f] = x[idx * F + f];
      cent[((size_t)r * k + j) * F + f] = cj[f];
    }
    if (t == 0) chosen[(size_t)r * k + j] = idx;
    __syncthreads();
    if (j + 1 < k) {
      for (int64_t n = lo; n < hi; ++n) {
        const float *xp = x + n * F;
        float dd = 0.f;
        for (int f = 0; f < F; ++f) {
          const float u = xp[f] - cj[f];
          dd = fmaf(u, u, dd);
        }
        D[n] = j == 0 ? dd : fminf(D[n], dd);
      }
    }
    __syncthreads();  // (tsum, cj are rewritten)
  }
}

__global__ __launch_bounds__(256) void km_contingency_kernel(const int64_t *cid, const int64_t *lab,
                                                             int64_t N, int k, int ncls,
                                                             int *table, int *outside) {
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < N;
       n += (int64_t)gridDim.x * 256) {
    const int64_t c = cid[n], l = lab[n];
    if (c >= 0 && c < k && l >= 0 && l < ncls)
      atomicAdd(&table[c * ncls + l], 1);
    else
      atomicAdd(outside, 1);
  }
}

template <int FX>
int launch_assign(const scae_kmeans_desc &d, dim3 grid, hipStream_t st) {
  const size_t lds = assign_lds(d.k, d.F);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(km_assign_kernel<FX>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  scae::launch(km_assign_kernel<FX>, grid, dim3(TP), lds, st, d);
  return SCAE_OK;
}

int assign(const scae_kmeans_desc &d, dim3 grid, hipStream_t st) {
  if (d.F <= 32) return launch_assign<32>(d, grid, st);
  if (d.F <= 64) return launch_assign<64>(d, grid, st);
  if (d.F <= 128) return launch_assign<128>(d, grid, st);
  return launch_assign<0>(d, grid, st);
}
}  // namespace

extern "C" int scae_kmeans_supported(int k, int F) {
  return k > 0 && F > 0 && k <= SCAE_KMEANS_MAX_K && F <= SCAE_KMEANS_MAX_F &&
         k * F <= SCAE_KMEANS_MAX_KF;
}

extern "C" int scae_kmeans_groups(int64_t N, int R) {
  if (N <= 0 || R <= 0) return 0;
  const int64_t tiles = (N + TP - 1) / TP;
  int64_t g = MAX_GROUPS / R;
  if (g < 1) g = 1;
  return (int)(tiles < g ? tiles : g);
}

extern "C" int scae_kmeans_lloyd_f32(const scae_kmeans_desc *dp, int n_iters, void *stream) {
  SCAE_REQUIRE(dp && n_iters >= 0);
  const scae_kmeans_desc d = *dp;
  SCAE_REQUIRE(d.x && d.centroids && d.labels && d.part_sum && d.part_count && d.part_changed &&
               d.part_inertia && d.state && d.inertia && d.N > 0 && d.N < ((int64_t)1 << 31) &&
               d.R > 0 && d.max_iter > 0);
  if (!scae_kmeans_supported(d.k, d.F)) return SCAE_ERR_UNSUPPORTED;
  SCAE_REQUIRE(d.G == scae_kmeans_groups(d.N, d.R));
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < n_iters; ++i) {
    const int rc = assign(d, dim3(d.G, d.R), st);
    if (rc) return rc;
    scae::launch(km_update_kernel, dim3(d.R), dim3(NTU), 0, st, d);
  }
  return scae_launch_status();
}

extern "C" int scae_kmeans_pp_f32(const float *x, int64_t N, int F, int k, int R, uint32_t seed,
                                  float *centroids, float *d2, int64_t *chosen, void *stream) {
  SCAE_REQUIRE(x && centroids && d2 && chosen && N > 0 && N < ((int64_t)1 << 31) && R > 0);
  if (!scae_kmeans_supported(k, F)) return SCAE_ERR_UNSUPPORTED;
  scae::launch(km_pp_kernel, dim3(R), dim3(NTP), 0, (hipStream_t)stream, x, N, F, k, seed,
               centroids, d2, chosen);
  return scae_launch_status();
}

extern "C" int scae_kmeans_assign_f32(const float *x, int64_t N, int F, int k,
                                      const float *centroids, int64_t *labels, void *stream) {
  SCAE_REQUIRE(x && centroids && labels && N > 0 && N < ((int64_t)1 << 31));
  if (!scae_kmeans_supported(k, F)) return SCAE_ERR_UNSUPPORTED;
  scae_kmeans_desc d{};
  d.x = x, d.N = N, d.F = F, d.k = k, d.R = 1, d.G = scae_kmeans_groups(N, 1);
  d.centroids = const_cast<float *>(centroids), d.labels = labels;
  const int rc = assign(d, dim3(d.G, 1), (hipStream_t)stream);
  if (rc) return rc;
  return scae_launch_status();
}

extern "C" int scae_kmeans_contingency(const int64_t *cluster_ids, const int64_t *labels,
                                       int64_t N, int k, int ncls, int *table, int *outside,
                                       void *stream) {
  SCAE_REQUIRE(cluster_ids && labels && table && outside && N > 0 && k > 0 && ncls > 0);
  const int64_t blocks = (N + 255) / 256;
  scae::launch(km_contingency_kernel, dim3(blocks < 1024 ? (int)blocks : 1024), dim3(256), 0,
               (hipStream_t)stream, cluster_ids, labels, N, k, ncls, table, outside);
  return scae_launch_status();
}
