// Exact k nearest neighbours for gfx950 (neighbors.py): the brute-force search, the k-NN vote and
// the neighbour ranks behind trustworthiness.
//
// The distance, the row tile and its geometry are row_dist_dev.h's, which states the
// rounding rule and keeps contraction off for itself; csrc/Makefile also gives this file
// -ffp-contract=off, for the vote's tallies.
//
// A neighbour is the 64-bit key (bits of d) << 32 | j.  d is a sum of squares from +0, so its
// bits order as unsigned integers the way the floats do, and the keys of one query are distinct:
// comparing keys is comparing the pairs (d, j), a total order.  Whatever way the base is split,
// the k least keys are the same.
//
//   knn_search_kernel  grid (query tiles, G base groups), one query per lane (its features in
//                      registers up to F = 32), the group's base rows streamed through LDS in
//                      tiles and read as a broadcast; each lane keeps its k best keys sorted in
//                      LDS as [slot][lane] (a wave's accesses to one slot fall in distinct
//                      banks) and the k-th in a register: a candidate touches the list only when
//                      it beats that threshold.  G == 1 writes the result, else the group's list;
//   knn_merge_kernel   one query per thread: the G sorted lists merged by key;
//   knn_vote_kernel    one query per thread, O(k^2 / 2) label compares;
//   knn_rank_count_kernel  the same streaming with one row i per lane: the k target keys
//                      (d_ij, j) in LDS, then for every streamed row l one d_il and k compares
//                      into register counters (skipped when the key is above all targets);
//   knn_rank_finish_kernel / knn_penalty_kernel  the groups' counts added, the ranks written,
//                      the penalties summed per workgroup and then in index order.
#include "common.h"
#include "row_dist_dev.h"

namespace {
using namespace scae_rows;
constexpr int TQ = 128;            // queries of a search workgroup, one per lane
constexpr int FXR = 32;            // features held in registers by the register form
constexpr int MAX_G = 64;          // base groups at most
constexpr int MIN_GROUP_ROWS = 512;
constexpr int TARGET_WG = 512;     // workgroups a search aims for: two per CU
constexpr int TM = 64;             // merge / vote workgroup
constexpr int TF = 256;            // rank finish / penalty workgroup
constexpr uint64_t EMPTY = ~0ull;  // no finite distance has these bits

__device__ __forceinline__ uint64_t make_key(float d, int64_t j) {
  return ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)j;
}

// key into the lane's sorted list (stride TQ), which it is known to beat; -> the new k-th key
__device__ __forceinline__ uint64_t list_insert(uint64_t *list, int k, uint64_t key) {
  int s = k - 1;
  while (s > 0) {
    const uint64_t p = list[(s - 1) * TQ];
    if (p < key) break;
    list[s * TQ] = p;
    --s;
  }
  list[s * TQ] = key;
  return list[(k - 1) * TQ];
}

struct Range {
  int64_t begin, end;
};
__device__ __forceinline__ Range group_range(int64_t Nb, int G, int g) {
  const int64_t chunk = (Nb + G - 1) / G;
  const int64_t b = g * chunk < Nb ? g * chunk : Nb;
  return {b, b + chunk < Nb ? b + chunk : Nb};
}

size_t search_lds(int k) { return (size_t)k * TQ * sizeof(uint64_t) + TILE_FLOATS * sizeof(float); }

template <int FX>
__global__ __launch_bounds__(TQ) void knn_search_kernel(const float *q, int64_t Nq,
                                                        const float *base, int64_t Nb, int F,
                                                        int k, int self_mode, int G,
                                                        uint64_t *part, float *d2, int64_t *idx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  uint64_t *list = reinterpret_cast<uint64_t *>(smem_raw) + threadIdx.x;   // [slot][lane]
  float *tile = reinterpret_cast<float *>(smem_raw + (size_t)k * TQ * sizeof(uint64_t));
  const int t = threadIdx.x, g = blockIdx.y;
  const int64_t qi = (int64_t)blockIdx.x * TQ + t;
  const bool active = qi < Nq;
  const TileGeom tg = tile_geom(F);
  const float *xp = q + (active ? qi : 0) * F;
  float xr[FX > 0 ? FX : 1];
  if constexpr (FX > 0) {
#pragma unroll
    for (int f = 0; f < FX; ++f) xr[f] = f < F ? xp[f] : 0.f;
  }
  for (int s = 0; s < k; ++s) list[s * TQ] = EMPTY;
  uint64_t thr = EMPTY;
  const int64_t skip = self_mode ? qi : -1;
  const Range rg = group_range(Nb, G, g);
  for (int64_t row0 = rg.begin; row0 < rg.end; row0 += tg.TB) {
    __syncthreads();   // (the previous tile has been read)
    load_tile<TQ>(tile, base, row0, rg.end, tg.TB, F, tg.F4);
    __syncthreads();
    if (!active) continue;
    const int64_t left = rg.end - row0;
    const int rows = left < tg.TB ? (int)left : tg.TB;
    for (int r = 0; r < rows; r += 4) {
      // four rows at a time: independent sums (rows past the end are zeros in LDS)
      float d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) d[u] = dist2<FX>(xr, xp, tile + (r + u) * tg.F4, F, tg.F4);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t j = row0 + r + u;
        const uint64_t key = make_key(d[u], j);
        if (r + u < rows && j != skip && key < thr) thr = list_insert(list, k, key);
      }
    }
  }
  if (!active) return;
  if (G == 1) {
    for (int s = 0; s < k; ++s) {
      const uint64_t key = list[s * TQ];
      d2[qi * k + s] = __uint_as_float((uint32_t)(key >> 32));
      idx[qi * k + s] = (int64_t)(uint32_t)key;
    }
  } else {
    uint64_t *p = part + (qi * G + g) * k;
    for (int s = 0; s < k; ++s) p[s] = list[s * TQ];
  }
}

// grid ceil(Nq / TM): the G sorted lists of a query merged by key (a short group's list ends in
// EMPTY keys; k <= Nb says the result has none)
__global__ __launch_bounds__(TM) void knn_merge_kernel(const uint64_t *part, int64_t Nq, int G,
                                                       int k, float *d2, int64_t *idx) {
  __shared__ unsigned char pos[MAX_G * TM];   // [group][lane]: the list's next entry
  const int t = threadIdx.x;
  const int64_t qi = (int64_t)blockIdx.x * TM + t;
  if (qi >= Nq) return;
  for (int g = 0; g < G; ++g) pos[g * TM + t] = 0;
  const uint64_t *p = part + qi * G * k;
  for (int s = 0; s < k; ++s) {
    uint64_t best = EMPTY;
    int bg = 0;
    for (int g = 0; g < G; ++g) {
      const int at = pos[g * TM + t];
      const uint64_t key = at < k ? p[g * k + at] : EMPTY;
      if (key < best) best = key, bg = g;
    }
    if (best != EMPTY) ++pos[bg * TM + t];
    d2[qi * k + s] = __uint_as_float((uint32_t)(best >> 32));
    idx[qi * k + s] = (int64_t)(uint32_t)best;
  }
}

struct Ks {
  int v[SCAE_KNN_MAX_KS];
};

__global__ __launch_bounds__(TM) void knn_vote_kernel(const int64_t *idx, const float *d2,
                                                      int64_t Nq, int k, const int64_t *labels,
                                                      int64_t Nb, Ks ks, int n_ks, int weighted,
                                                      int64_t *pred) {
  const int64_t qi = (int64_t)blockIdx.x * TM + threadIdx.x;
  if (qi >= Nq) return;
  const int64_t *ix = idx + qi * k;
  const float *dd = d2 + qi * k;
  const bool zeros = weighted && dd[0] == 0.f;
  auto label_of = [&](int n) {
    int64_t j = ix[n];
    j = j < 0 ? 0 : (j >= Nb ? Nb - 1 : j);
    return labels[j];
  };
  auto weight_of = [&](int n) {
    if (!weighted) return 1.f;
    if (zeros) return dd[n] == 0.f ? 1.f : 0.f;
    return 1.f / sqrtf(dd[n]);   // (both correctly rounded: the compiler's default for HIP)
  };
  float best_t = 0.f;
  int64_t best_l = 0;
  for (int m = 0; m < k; ++m) {
    const int64_t lm = label_of(m);
    float tally = 0.f;
    for (int n = 0; n <= m; ++n)
      if (label_of(n) == lm) tally = __fadd_rn(tally, weight_of(n));
    if (m == 0 || tally > best_t || (tally == best_t && lm < best_l)) best_t = tally, best_l = lm;
#pragma unroll
    for (int i = 0; i < SCAE_KNN_MAX_KS; ++i)
      if (i < n_ks && ks.v[i] == m + 1) pred[qi * n_ks + i] = best_l;
  }
}

size_t rank_lds(int k) { return search_lds(k); }

// grid (row tiles, G): counts of the group's rows l != i whose key is below each target's
template <int FX, int KX>
__global__ __launch_bounds__(TQ) void knn_rank_count_kernel(const float *x, int64_t N, int F,
                                                            const int64_t *idx, int k, int G,
                                                            int *part_count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  uint64_t *tk = reinterpret_cast<uint64_t *>(smem_raw) + threadIdx.x;   // [slot][lane]
  float *tile = reinterpret_cast<float *>(smem_raw + (size_t)k * TQ * sizeof(uint64_t));
  const int t = threadIdx.x, g = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * TQ + t;
  const bool active = i < N;
  const TileGeom tg = tile_geom(F);
  const float *xp = x + (active ? i : 0) * F;
  float xr[FX > 0 ? FX : 1];
  if constexpr (FX > 0) {
#pragma unroll
    for (int f = 0; f < FX; ++f) xr[f] = f < F ? xp[f] : 0.f;
  }
  uint64_t tmax = 0;
  if (active)
    for (int m = 0; m < k; ++m) {
      int64_t j = idx[i * k + m];
      j = j < 0 ? 0 : (j >= N ? N - 1 : j);
      const uint64_t key = make_key(dist2_rows(xp, x + j * F, F), j);
      tk[m * TQ] = key;
      tmax = key > tmax ? key : tmax;
    }
  int cnt[KX];
#pragma unroll
  for (int m = 0; m < KX; ++m) cnt[m] = 0;
  const Range rg = group_range(N, G, g);
  for (int64_t row0 = rg.begin; row0 < rg.end; row0 += tg.TB) {
    __syncthreads();
    load_tile<TQ>(tile, x, row0, rg.end, tg.TB, F, tg.F4);
    __syncthreads();
    if (!active) continue;
    const int64_t left = rg.end - row0;
    const int rows = left < tg.TB ? (int)left : tg.TB;
    for (int r = 0; r < rows; r += 4) {
      float d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) d[u] = dist2<FX>(xr, xp, tile + (r + u) * tg.F4, F, tg.F4);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t l = row0 + r + u;
        const uint64_t key = make_key(d[u], l);
        if (r + u < rows && l != i && key < tmax) {
#pragma unroll
          for (int m = 0; m < KX; ++m)
            if (m < k) cnt[m] += key < tk[m * TQ];
        }
      }
    }
  }
  if (!active) return;
  int *pc = part_count + (i * G + g) * k;
#pragma unroll
  for (int m = 0; m < KX; ++m)
    if (m < k) pc[m] = cnt[m];
}

// grid ceil(N / TF): rank = 1 + the groups' counts; the workgroup's penalty in thread order
__global__ __launch_bounds__(TF) void knn_rank_finish_kernel(const int *part_count, int64_t N,
                                                             int G, int k, int *rank,
                                                             int64_t *part) {
  __shared__ int64_t pen[TF];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * TF + t;
  int64_t mine = 0;
  if (i < N)
    for (int m = 0; m < k; ++m) {
      int c = 0;
      for (int g = 0; g < G; ++g) c += part_count[(i * G + g) * k + m];
      rank[i * k + m] = 1 + c;
      mine += 1 + c > k ? 1 + c - k : 0;
    }
  pen[t] = mine;
  __syncthreads();
  if (t == 0) {
    int64_t s = 0;
    for (int u = 0; u < TF; ++u) s += pen[u];
    part[blockIdx.x] = s;
  }
}

// one workgroup: the partials in index order
__global__ __launch_bounds__(TF) void knn_penalty_kernel(const int64_t *part, int64_t n,
                                                         int64_t *penalty) {
  __shared__ int64_t pen[TF];
  const int t = threadIdx.x;
  int64_t s = 0;
  for (int64_t u = t; u < n; u += TF) s += part[u];
  pen[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t all = 0;
    for (int u = 0; u < TF; ++u) all += pen[u];
    *penalty = all;
  }
}

template <class K>
int big_lds(K kernel, size_t lds) {
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  return SCAE_OK;
}

template <int FX>
int launch_search(dim3 grid, hipStream_t st, const float *q, int64_t Nq, const float *base,
                  int64_t Nb, int F, int k, int self_mode, int G, uint64_t *part, float *d2,
                  int64_t *idx) {
  const size_t lds = search_lds(k);
  const int rc = big_lds(knn_search_kernel<FX>, lds);
  if (rc) return rc;
  scae::launch(knn_search_kernel<FX>, grid, dim3(TQ), lds, st, q, Nq, base, Nb, F, k, self_mode,
               G, part, d2, idx);
  return SCAE_OK;
}

template <int FX, int KX>
int launch_rank(dim3 grid, hipStream_t st, const float *x, int64_t N, int F, const int64_t *idx,
                int k, int G, int *part_count) {
  const size_t lds = rank_lds(k);
  const int rc = big_lds(knn_rank_count_kernel<FX, KX>, lds);
  if (rc) return rc;
  scae::launch(knn_rank_count_kernel<FX, KX>, grid, dim3(TQ), lds, st, x, N, F, idx, k, G,
               part_count);
  return SCAE_OK;
}
}  // namespace

extern "C" int scae_knn_supported(int64_t Nq, int64_t Nb, int F, int k) {
  const int64_t lim = (int64_t)1 << 31;
  return Nq >= 1 && Nb >= 1 && Nq < lim && Nb < lim && F >= 1 && F <= SCAE_KNN_MAX_F && k >= 1 &&
         k <= SCAE_KNN_MAX_K && k <= Nb;
}

extern "C" int scae_knn_groups(int64_t Nq, int64_t Nb) {
  const int64_t lim = (int64_t)1 << 31;
  if (Nq < 1 || Nb < 1 || Nq >= lim || Nb >= lim) return 0;
  const int64_t tiles = (Nq + TQ - 1) / TQ;
  int64_t g = (TARGET_WG + tiles - 1) / tiles;
  const int64_t by_rows = Nb / MIN_GROUP_ROWS;
  if (g > by_rows) g = by_rows;
  if (g > MAX_G) g = MAX_G;
  return g < 1 ? 1 : (int)g;
}

extern "C" int scae_knn_f32(const float *q, int64_t Nq, const float *base, int64_t Nb, int F,
                            int k, int self_mode, uint64_t *part, float *d2, int64_t *idx,
                            void *stream) {
  SCAE_REQUIRE(q && base && d2 && idx);
  if (!scae_knn_supported(Nq, Nb, F, k)) return SCAE_ERR_UNSUPPORTED;
  if (self_mode) {
    SCAE_REQUIRE(base == q && Nb == Nq);
    if (k > Nb - 1) return SCAE_ERR_UNSUPPORTED;
  }
  const int G = scae_knn_groups(Nq, Nb);
  SCAE_REQUIRE(G == 1 || part);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((Nq + TQ - 1) / TQ), G);
  const int rc = F <= FXR ? launch_search<FXR>(grid, st, q, Nq, base, Nb, F, k, self_mode, G,
                                               part, d2, idx)
                          : launch_search<0>(grid, st, q, Nq, base, Nb, F, k, self_mode, G, part,
                                             d2, idx);
  if (rc) return rc;
  if (G > 1)
    scae::launch(knn_merge_kernel, dim3((unsigned)((Nq + TM - 1) / TM)), dim3(TM), 0, st,
                 (const uint64_t *)part, Nq, G, k, d2, idx);
  return scae_launch_status();
}

// the self-mode search of sparse t-SNE: the same launches up to k = SCAE_TSNE_MAX_NEIGHBORS (the
// lists of a workgroup then take 128 KiB of LDS, one workgroup a CU; the merge's byte cursors
// end at k <= 128)
extern "C" int scae_knn_wide_f32(const float *x, int64_t N, int F, int k, uint64_t *part,
                                 float *d2, int64_t *idx, void *stream) {
  SCAE_REQUIRE(x && d2 && idx);
  static_assert(SCAE_TSNE_MAX_NEIGHBORS <= 255, "knn_merge_kernel's cursors are bytes");
  if (N < 2 || N >= ((int64_t)1 << 31) || F < 1 || F > SCAE_KNN_MAX_F || k < 1 ||
      k > SCAE_TSNE_MAX_NEIGHBORS || k > N - 1)
    return SCAE_ERR_UNSUPPORTED;
  const int G = scae_knn_groups(N, N);
  SCAE_REQUIRE(G == 1 || part);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((N + TQ - 1) / TQ), G);
  const int rc = F <= FXR ? launch_search<FXR>(grid, st, x, N, x, N, F, k, 1, G, part, d2, idx)
                          : launch_search<0>(grid, st, x, N, x, N, F, k, 1, G, part, d2, idx);
  if (rc) return rc;
  if (G > 1)
    scae::launch(knn_merge_kernel, dim3((unsigned)((N + TM - 1) / TM)), dim3(TM), 0, st,
                 (const uint64_t *)part, N, G, k, d2, idx);
  return scae_launch_status();
}

extern "C" int scae_knn_vote_f32(const int64_t *idx, const float *d2, int64_t Nq, int k,
                                 const int64_t *base_labels, int64_t Nb, const int *ks, int n_ks,
                                 int weighted, int64_t *pred, void *stream) {
  SCAE_REQUIRE(idx && d2 && base_labels && ks && pred && Nq >= 1 && Nq < ((int64_t)1 << 31) &&
               Nb >= 1 && k >= 1 && k <= SCAE_KNN_MAX_K && n_ks >= 1 && n_ks <= SCAE_KNN_MAX_KS);
  Ks kv{};
  for (int i = 0; i < n_ks; ++i) {
    SCAE_REQUIRE(ks[i] >= 1 && (i == 0 || ks[i] > ks[i - 1]));
    kv.v[i] = ks[i];
  }
  SCAE_REQUIRE(ks[n_ks - 1] == k);
  scae::launch(knn_vote_kernel, dim3((unsigned)((Nq + TM - 1) / TM)), dim3(TM), 0,
               (hipStream_t)stream, idx, d2, Nq, k, base_labels, Nb, kv, n_ks, weighted, pred);
  return scae_launch_status();
}

extern "C" int scae_knn_ranks_f32(const float *x, int64_t N, int F, const int64_t *idx, int k,
                                  int *rank, int *part_count, int64_t *part, int64_t *penalty,
                                  void *stream) {
  SCAE_REQUIRE(x && idx && rank && part_count && part && penalty);
  if (!scae_knn_supported(N, N, F, k) || k > N - 1) return SCAE_ERR_UNSUPPORTED;
  const int G = scae_knn_groups(N, N);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((N + TQ - 1) / TQ), G);
  int rc;
  if (F <= FXR)
    rc = k <= 16 ? launch_rank<FXR, 16>(grid, st, x, N, F, idx, k, G, part_count)
                 : launch_rank<FXR, SCAE_KNN_MAX_K>(grid, st, x, N, F, idx, k, G, part_count);
  else
    rc = k <= 16 ? launch_rank<0, 16>(grid, st, x, N, F, idx, k, G, part_count)
                 : launch_rank<0, SCAE_KNN_MAX_K>(grid, st, x, N, F, idx, k, G, part_count);
  if (rc) return rc;
  const int64_t blocks = (N + TF - 1) / TF;
  scae::launch(knn_rank_finish_kernel, dim3((unsigned)blocks), dim3(TF), 0, st,
               (const int *)part_count, N, G, k, rank, part);
  scae::launch(knn_penalty_kernel, dim3(1), dim3(TF), 0, st, (const int64_t *)part, blocks,
               penalty);
  return scae_launch_status();
}
