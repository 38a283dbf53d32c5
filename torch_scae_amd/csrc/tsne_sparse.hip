// Sparse t-SNE for gfx950 (embed.py, neighbors="auto" | K): the dense rules of tsne.hip with P
// kept on each row's K nearest neighbours and the repulsion still exact over every pair.  The
// rules are in include/scae_hip.h.
//
// Affinities, once per run (the lists come from knn.hip's search, the CSR from integer sorts):
//   tsne_knn_beta_kernel  one row per wave, lane l holds the list's entries l and l + 64: the
//                         bisection of the dense path, S and sum d e reduced by DPP, so every
//                         lane decides from the same two sums; the conditional row written.
// One iteration is five launches:
//   tsne_att_kernel    a CSR row per wave: lane l takes the row's entries l, l + 64, ... in
//                      order, gathers y_j (Y is 8 N bytes: it stays in L2), and the wave reduces
//                      sum P q dy (and sum P log1p(d) in the recorded form) by DPP.  A hub row
//                      of N - 1 entries is one wave's loop: correct, not fast;
//   tsne_rep_kernel    grid (512-row blocks, G column groups), the all-pairs pass.  A thread
//                      keeps two rows' y_i and their q^2 dy and q sums in registers, the
//                      group's columns go through LDS in tiles of 256 and are read as a
//                      broadcast, two columns a read.  No P, no log1p.  q = 1 / (1 + d) is
//                      the hardware reciprocal and one Newton step (the division's expansion
//                      would double the loop); the compiler packs the two rows' arithmetic
//                      into v_pk_*_f32, 35 of them and 8 v_rcp_f32 for 8 pairs, and the issue
//                      of those bounds the pass (the quarter-rate reciprocal is close to half
//                      of it).  Only a tile that holds the block's own rows or columns past N
//                      pays for the j != i / j < N test;
//   tsne_srows_kernel  the repulsion's partials added in g order (the attraction launch has
//                      written its rows), then tsne_step_dev.h's update, finish and schedule: the
//                      dense path's, with block's rows SCAE_TSNE_SPARSE_MAX_N / 256 apart.
// Nothing crosses workgroups inside a launch; every product-sum is an explicit fmaf and
// contraction is off, so the recorded form of the attraction gives the bits of the plain one.
#pragma clang fp contract(off)
#include "common.h"
#include "tsne_step_dev.h"

namespace {
constexpr int NW = 4;              // rows (waves) of a bandwidth / attraction workgroup
constexpr int RT = 256;            // repulsion workgroup
constexpr int RR = 2;              // rows per thread there
constexpr int RB = RT * RR;        // rows per workgroup
constexpr int TJ = 256;            // columns per LDS tile: one per thread to load
constexpr int TARGET_WG = 1024;    // workgroups a repulsion launch aims for: four per CU
constexpr int MAX_G = 64;
// NU, the rows / update / finish workgroup (one row per thread), is tsne_step_dev.h's
constexpr int MAXB = SCAE_TSNE_SPARSE_MAX_N / NU;   // block's stride
static_assert(5 * MAXB == SCAE_TSNE_SPARSE_BLOCK_DOUBLES, "block partials: z, kl, y0, y1, |g|^2");
static_assert(SCAE_TSNE_MAX_NEIGHBORS == 2 * SCAE_WAVE, "two list entries per lane");

// grid ceil(N / NW): wave w of workgroup b takes row NW b + w (no barrier: a wave past N leaves)
__global__ __launch_bounds__(NW * SCAE_WAVE) void tsne_knn_beta_kernel(const float *d2, int N,
                                                                       int K, float log_perp,
                                                                       float *cond,
                                                                       float *beta_out) {
  const int lane = threadIdx.x % SCAE_WAVE;
  const int i = blockIdx.x * NW + __builtin_amdgcn_readfirstlane(threadIdx.x / SCAE_WAVE);
  if (i >= N) return;
  const float *di = d2 + (size_t)i * K;
  const bool in0 = lane < K, in1 = lane + SCAE_WAVE < K;
  const float first = di[0];
  const float a0 = in0 ? di[lane] - first : 0.f;
  const float a1 = in1 ? di[lane + SCAE_WAVE] - first : 0.f;
  float beta = 1.f, lo = 0.f, hi = 0.f, S = 1.f, e0 = 0.f, e1 = 0.f;
  bool lo_open = true, hi_open = true;
  for (int step = 0; step < 100; ++step) {
    e0 = in0 ? expf(-beta * a0) : 0.f;
    e1 = in1 ? expf(-beta * a1) : 0.f;
    S = scae::wave_sum(e0 + e1);
    const float U = scae::wave_sum(fmaf(a1, e1, a0 * e0));
    const float diff = (logf(S) + beta * U / S) - log_perp;
    if (fabsf(diff) <= 1e-5f || step == 99) break;
    if (diff > 0.f) {   // too flat: a larger beta
      lo = beta, lo_open = false;
      beta = hi_open ? beta * 2.f : (beta + hi) * 0.5f;
    } else {
      hi = beta, hi_open = false;
      beta = lo_open ? beta * 0.5f : (beta + lo) * 0.5f;
    }
  }
  float *ci = cond + (size_t)i * K;
  if (in0) ci[lane] = e0 / S;
  if (in1) ci[lane + SCAE_WAVE] = e1 / S;
  if (lane == 0) beta_out[i] = beta;
}

// grid ceil(N / NW): rows (0 | 1 | 5, i) = the row's sums of P q dy0 | P q dy1 | P log1p(d)
template <bool KL>
__global__ __launch_bounds__(NW * SCAE_WAVE) void tsne_att_kernel(scae_tsne_sparse_desc d) {
  const int lane = threadIdx.x % SCAE_WAVE, N = d.N;
  const int i = blockIdx.x * NW + __builtin_amdgcn_readfirstlane(threadIdx.x / SCAE_WAVE);
  if (i >= N) return;
  const float2 *Y2 = reinterpret_cast<const float2 *>(d.Y);
  const float2 yi = Y2[i];
  int64_t b = d.indptr[i], e = d.indptr[i + 1];
  b = b < 0 ? 0 : b, e = e > d.nnz ? d.nnz : e;   // (a broken CSR reads nothing out of bounds)
  float a0 = 0.f, a1 = 0.f, kl = 0.f;
  for (int64_t p = b + lane; p < e; p += SCAE_WAVE) {
    int j = d.cols[p];
    j = j < 0 ? 0 : (j >= N ? N - 1 : j);
    const float pv = d.vals[p];
    const float2 yj = Y2[j];
    const float dy0 = yi.x - yj.x, dy1 = yi.y - yj.y;
    const float dd = fmaf(dy1, dy1, dy0 * dy0);
    const float pq = pv * (1.f / (1.f + dd));
    a0 = fmaf(pq, dy0, a0), a1 = fmaf(pq, dy1, a1);
    if constexpr (KL) kl = fmaf(pv, log1pf(dd), kl);
  }
  a0 = scae::wave_sum(a0), a1 = scae::wave_sum(a1);
  if constexpr (KL) kl = scae::wave_sum(kl);
  if (lane == 0) {
    d.rows[i] = a0, d.rows[(size_t)N + i] = a1;
    if constexpr (KL) d.rows[(size_t)5 * N + i] = kl;
  }
}

// 1 / x for x >= 1: v_rcp_f32 (1 ulp) and one Newton step.  (x = +inf, |y| beyond 1e19, would
// give NaN where the division gives 0: no embedding gets there)
__device__ __forceinline__ float recip(float x) {
  const float r = __builtin_amdgcn_rcpf(x);
  return fmaf(fmaf(-x, r, 1.f), r, r);
}

// the tile's TJ columns (LDS, two a float4) against the thread's RR rows; MASK: q = 0 for the
// row itself and for columns past N
template <bool MASK>
__device__ __forceinline__ void rep_tile(const float4 *tile, int j0, int N, const int (&irow)[RR],
                                         const float (&yi0)[RR], const float (&yi1)[RR],
                                         float (&b0)[RR], float (&b1)[RR], float (&z)[RR]) {
#pragma unroll 2
  for (int p = 0; p < TJ / 2; ++p) {
    const float4 v = tile[p];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float yj0 = h ? v.z : v.x, yj1 = h ? v.w : v.y;
      const int j = j0 + 2 * p + h;
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        const float dy0 = yi0[r] - yj0, dy1 = yi1[r] - yj1;
        const float dd = fmaf(dy1, dy1, dy0 * dy0);
        float q = recip(1.f + dd);
        if constexpr (MASK) q = (j == irow[r] || j >= N) ? 0.f : q;
        const float q2 = q * q;
        b0[r] = fmaf(q2, dy0, b0[r]), b1[r] = fmaf(q2, dy1, b1[r]);
        z[r] += q;
      }
    }
  }
}

// grid (ceil(N / RB), G); group g takes columns [g chunk, (g + 1) chunk), chunk a multiple of TJ;
// part (0 | 1 | 2, g, i) = the group's sums of q^2 dy0 | q^2 dy1 | q in column order
__global__ __launch_bounds__(RT) void tsne_rep_kernel(const float *Y, int N, int G, int chunk,
                                                      float *part) {
  __shared__ float4 tile[TJ / 2];
  const int t = threadIdx.x, i0 = blockIdx.x * RB, g = blockIdx.y;
  const float2 *Y2 = reinterpret_cast<const float2 *>(Y);
  int irow[RR];
  float yi0[RR], yi1[RR], b0[RR], b1[RR], z[RR];
#pragma unroll
  for (int r = 0; r < RR; ++r) {
    irow[r] = i0 + r * RT + t;
    const float2 v = irow[r] < N ? Y2[irow[r]] : make_float2(0.f, 0.f);
    yi0[r] = v.x, yi1[r] = v.y, b0[r] = 0.f, b1[r] = 0.f, z[r] = 0.f;
  }
  const int jb = g * chunk, je = jb + chunk < N ? jb + chunk : N;
  for (int j0 = jb; j0 < je; j0 += TJ) {
    __syncthreads();   // (the previous tile has been read)
    reinterpret_cast<float2 *>(tile)[t] = j0 + t < N ? Y2[j0 + t] : make_float2(0.f, 0.f);
    __syncthreads();
    if ((j0 < i0 + RB && j0 + TJ > i0) || j0 + TJ > N)   // (uniform over the workgroup)
      rep_tile<true>(tile, j0, N, irow, yi0, yi1, b0, b1, z);
    else
      rep_tile<false>(tile, j0, N, irow, yi0, yi1, b0, b1, z);
  }
#pragma unroll
  for (int r = 0; r < RR; ++r)
    if (irow[r] < N) {
      part[((size_t)0 * G + g) * N + irow[r]] = b0[r];
      part[((size_t)1 * G + g) * N + irow[r]] = b1[r];
      part[((size_t)2 * G + g) * N + irow[r]] = z[r];
    }
}

// grid (ceil(N / NU)): rows (2 + c, i) = sum_g part (c, g, i) in g order; block (0 | 1, b) = the
// workgroup's fp64 sum of z | kl (the attraction launch has written rows 0, 1 and 5).  The loads
// of GU groups are issued together (a thread's G dependent round trips were the launch's time at
// N = 10 000, 40 workgroups and G = 40); the additions keep the g order
template <bool KL>
__global__ __launch_bounds__(NU) void tsne_srows_kernel(scae_tsne_sparse_desc d) {
  constexpr int GU = 8;
  __shared__ double red[NU / SCAE_WAVE];
  const int i = blockIdx.x * NU + threadIdx.x, N = d.N, G = d.G;
  float z = 0.f, kl = 0.f;
  if (i < N) {
    float s[3] = {0.f, 0.f, 0.f};
    for (int g0 = 0; g0 < G; g0 += GU) {
      float v[3][GU];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int u = 0; u < GU; ++u)
          v[c][u] = g0 + u < G ? d.part[((size_t)c * G + g0 + u) * N + i] : 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int u = 0; u < GU; ++u)
          if (g0 + u < G) s[c] += v[c][u];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) d.rows[(size_t)(2 + c) * N + i] = s[c];
    z = s[2];
    if constexpr (KL) kl = d.rows[(size_t)5 * N + i];
  }
  tsne_block_z_kl<KL>(z, kl, d.block, MAXB, red);
}

// columns of a repulsion group: whole tiles, about TARGET_WG workgroups over the row blocks
int group_chunk(int N) {
  const int rb = (N + RB - 1) / RB;
  int want = (TARGET_WG + rb - 1) / rb;
  want = want > MAX_G ? MAX_G : want;
  const int cols = (N + want - 1) / want;
  return (cols + TJ - 1) / TJ * TJ;
}

// the gradient's sums of one iteration into rows (kl: the recorded form)
void sum_gradient(const scae_tsne_sparse_desc &d, bool kl, hipStream_t st) {
  const int nb = (d.N + NU - 1) / NU, nw = (d.N + NW - 1) / NW;
  if (kl)
    scae::launch(tsne_att_kernel<true>, dim3(nw), dim3(NW * SCAE_WAVE), 0, st, d);
  else
    scae::launch(tsne_att_kernel<false>, dim3(nw), dim3(NW * SCAE_WAVE), 0, st, d);
  scae::launch(tsne_rep_kernel, dim3((d.N + RB - 1) / RB, d.G), dim3(RT), 0, st,
               (const float *)d.Y, d.N, d.G, group_chunk(d.N), d.part);
  if (kl)
    scae::launch(tsne_srows_kernel<true>, dim3(nb), dim3(NU), 0, st, d);
  else
    scae::launch(tsne_srows_kernel<false>, dim3(nb), dim3(NU), 0, st, d);
}
}  // namespace

extern "C" int scae_tsne_sparse_supported(int N, int F, int K) {
  return N >= 2 && N <= SCAE_TSNE_SPARSE_MAX_N && F >= 1 && F <= SCAE_TSNE_MAX_F && K >= 1 &&
         K <= SCAE_TSNE_MAX_NEIGHBORS && K <= N - 1;
}

extern "C" int scae_tsne_sparse_groups(int N) {
  if (N < 2 || N > SCAE_TSNE_SPARSE_MAX_N) return 0;
  const int chunk = group_chunk(N);
  return (N + chunk - 1) / chunk;
}

extern "C" int scae_tsne_knn_bandwidths_f32(const float *d2, int N, int K, float perplexity,
                                            float *cond, float *beta, void *stream) {
  SCAE_REQUIRE(d2 && cond && beta);
  if (!scae_tsne_sparse_supported(N, 1, K)) return SCAE_ERR_UNSUPPORTED;
  SCAE_REQUIRE(perplexity > 0.f && 3.f * perplexity <= (float)K);
  scae::launch(tsne_knn_beta_kernel, dim3((N + NW - 1) / NW), dim3(NW * SCAE_WAVE), 0,
               (hipStream_t)stream, d2, N, K, logf(perplexity), cond, beta);
  return scae_launch_status();
}

extern "C" int scae_tsne_sparse_run_f32(const scae_tsne_sparse_desc *dp, int first_iter, int n,
                                        void *stream) {
  SCAE_REQUIRE(dp && first_iter >= 0 && n >= 0);
  const scae_tsne_sparse_desc d = *dp;
  SCAE_REQUIRE(d.indptr && d.cols && d.vals && d.Y && d.velocity && d.gains && d.part &&
               d.rows && d.block && d.plogp && d.history && d.nnz >= 0 && d.n_iter > 0 &&
               d.check_every > 0 && d.exaggeration_iter >= 0 && first_iter + n <= d.n_iter);
  if (!scae_tsne_sparse_supported(d.N, 1, 1)) return SCAE_ERR_UNSUPPORTED;
  SCAE_REQUIRE(d.G == scae_tsne_sparse_groups(d.N));
  hipStream_t st = (hipStream_t)stream;
  tsne_run(d, MAXB, first_iter, n, st, [&](bool kl) { sum_gradient(d, kl, st); });
  return scae_launch_status();
}
