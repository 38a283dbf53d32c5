// Exact t-SNE for gfx950 (embed.py): the 2-D embedding of SCAE's capsule features the paper
// shows next to its k-means and linear-probe figures.  The rules are in include/scae_hip.h.
//
// Affinities, once per run:
//   tsne_dist_kernel   64 x 64 tiles of squared distances over 32-feature LDS chunks, f order;
//   tsne_beta_kernel   one workgroup per row, the row in LDS: minimum, then the bisection -- each
//                      evaluation sums S and sum d e per thread in j order, per wave by DPP, the
//                      waves in order -- and the conditional row written in place;
//   tsne_sym_kernel    one workgroup per pair of mirrored 32 x 32 tiles, both through LDS,
//                      (p_j|i + p_i|j) / 2N to both and the pair's fp64 share of sum P log P;
//   tsne_sum_kernel    those shares in index order.
// One iteration is four launches:
//   tsne_grad_kernel   grid (row blocks, column groups).  A wave keeps the y_j of its 64 M
//                      columns in registers (lane l: columns l, l + 64, ...), walks its rows with
//                      y_i wave-uniform and P's row segment read coalesced, and reduces the
//                      row's five sums (six in the KL form) across lanes by DPP;
//   tsne_rows_kernel   the G partials of every row in g order, per-workgroup fp64 sums of Z, KL;
//   tsne_update_kernel, tsne_finish_kernel  tsne_step_dev.h's, shared with tsne_sparse.hip, as is
//                      the schedule: the update, then the column means leave Y and the history row.
// P is read once per iteration (N^2 floats: the pass is bound by that stream above N of a few
// thousand); nothing crosses workgroups inside a launch, so stream order is the only ordering.
// Every product-sum is an explicit fmaf and contraction is off: the KL form of the gradient
// kernel gives the bits of the plain one.
#pragma clang fp contract(off)
#include "common.h"
#include "tsne_step_dev.h"

namespace {
constexpr int DT = 64, DF = 32;   // distance tile, feature chunk
constexpr int NB = 256;           // bandwidth-search workgroup
constexpr int ST = 32;            // symmetrise tile
constexpr int NS = 1024;          // one-workgroup reductions
constexpr int SMALL_N = 2048;     // up to here 256-column groups, above 1024
constexpr int NC = 6;             // att0, att1, rep0, rep1, z, kl
// NU, the rows / update / finish workgroup (one row per thread), is tsne_step_dev.h's
constexpr int MAXB = SCAE_TSNE_MAX_N / NU;   // 128 update workgroups at most: block's stride
static_assert(5 * MAXB == SCAE_TSNE_BLOCK_DOUBLES, "block partials: z, kl, y0, y1, |g|^2");

using scae_reduce::wave_sum_f64;

__global__ __launch_bounds__(256) void tsne_dist_kernel(const float *x, int N, int F, float *D) {
  __shared__ float xi[DT][DF + 1], xj[DT][DF + 1];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int i0 = blockIdx.y * DT, j0 = blockIdx.x * DT;
  float acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
  for (int f0 = 0; f0 < F; f0 += DF) {
    for (int e = t; e < DT * DF; e += 256) {
      const int r = e / DF, f = e % DF;
      const bool fok = f0 + f < F;
      xi[r][f] = fok && i0 + r < N ? x[(size_t)(i0 + r) * F + f0 + f] : 0.f;
      xj[r][f] = fok && j0 + r < N ? x[(size_t)(j0 + r) * F + f0 + f] : 0.f;
    }
    __syncthreads();
    const int fn = F - f0 < DF ? F - f0 : DF;
    for (int f = 0; f < fn; ++f) {
      float a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = xi[ty + 16 * u][f], b[u] = xj[tx + 16 * u][f];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const float df = a[u] - b[v];
          acc[u][v] = fmaf(df, df, acc[u][v]);
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = i0 + ty + 16 * u, j = j0 + tx + 16 * v;
      if (i < N && j < N) D[(size_t)i * N + j] = acc[u][v];
    }
}

// grid (N); dynamic LDS: the row, N floats
__global__ __launch_bounds__(NB) void tsne_beta_kernel(float *P, int N, float log_perp,
                                                       float *beta_out) {
  extern __shared__ __attribute__((aligned(16))) float row[];
  __shared__ float red[2 * NB / SCAE_WAVE];
  const int i = blockIdx.x, t = threadIdx.x, wid = t / SCAE_WAVE, lane = t % SCAE_WAVE;
  float *Pi = P + (size_t)i * N;
  float mn = INFINITY;
  for (int j = t; j < N; j += NB) {
    const float d = Pi[j];
    row[j] = d;
    if (j != i) mn = fminf(mn, d);
  }
  mn = -scae::wave_max(-mn);
  if (lane == 0) red[wid] = mn;
  __syncthreads();
  mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  for (int j = t; j < N; j += NB) row[j] -= mn;   // (this thread's own entries)
  __syncthreads();                                // (red is rewritten)
  // every thread keeps the same (beta, lo, hi): they all see the same sums
  float beta = 1.f, lo = 0.f, hi = 0.f, S = 1.f;
  bool lo_open = true, hi_open = true;
  for (int step = 0; step < 100; ++step) {
    float s = 0.f, u = 0.f;
    for (int j = t; j < N; j += NB)
      if (j != i) {
        const float d = row[j], e = expf(-beta * d);
        s += e;
        u = fmaf(d, e, u);
      }
    s = scae::wave_sum(s);
    u = scae::wave_sum(u);
    if (lane == 0) red[wid] = s, red[NB / SCAE_WAVE + wid] = u;
    __syncthreads();
    S = ((red[0] + red[1]) + red[2]) + red[3];
    const float U = ((red[4] + red[5]) + red[6]) + red[7];
    __syncthreads();
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
  for (int j = t; j < N; j += NB) Pi[j] = j != i ? expf(-beta * row[j]) / S : 0.f;
  if (t == 0) beta_out[i] = beta;
}

__host__ __device__ inline size_t pair_index(int I, int J, int T) {   // I <= J
  return (size_t)I * T - (size_t)I * (I - 1) / 2 + (J - I);
}

// grid (T, T), T = ceil(N / 32); the workgroups below the diagonal have nothing to do
__global__ __launch_bounds__(256) void tsne_sym_kernel(float *P, int N, double *part) {
  const int I = blockIdx.y, J = blockIdx.x;
  if (J < I) return;
  __shared__ float A[ST][ST + 1], B[ST][ST + 1];
  __shared__ double red[256 / SCAE_WAVE];
  const int t = threadIdx.x, c = t & 31, r0 = t >> 5;
  for (int r = r0; r < ST; r += 8) {
    const int i = I * ST + r, j = J * ST + c, i2 = J * ST + r, j2 = I * ST + c;
    A[r][c] = i < N && j < N ? P[(size_t)i * N + j] : 0.f;
    B[r][c] = i2 < N && j2 < N ? P[(size_t)i2 * N + j2] : 0.f;
  }
  __syncthreads();
  const float two_n = 2.f * (float)N;
  double s = 0.0;
  for (int r = r0; r < ST; r += 8) {
    const int i = I * ST + r, j = J * ST + c, i2 = J * ST + r, j2 = I * ST + c;
    if (i < N && j < N) {
      const float v = (A[r][c] + B[c][r]) / two_n;
      P[(size_t)i * N + j] = v;
      if (v > 0.f) s += (double)v * log((double)v);
    }
    if (I != J && i2 < N && j2 < N) P[(size_t)i2 * N + j2] = (A[c][r] + B[r][c]) / two_n;
  }
  if (I != J) s *= 2.0;   // (the mirrored tile holds the same values)
  s = wave_sum_f64(s);
  if (t % SCAE_WAVE == 0) red[t / SCAE_WAVE] = s;
  __syncthreads();
  if (t == 0) part[pair_index(I, J, gridDim.x)] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup: out = sum of part[0, n), thread t its entries t, t + NS, ... in order, the
// waves by shuffle, then in wave order
__global__ __launch_bounds__(NS) void tsne_sum_kernel(const double *part, int64_t n, double *out) {
  __shared__ double red[NS / SCAE_WAVE];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int64_t k = t; k < n; k += NS) s += part[k];
  s = wave_sum_f64(s);
  if (t % SCAE_WAVE == 0) red[t / SCAE_WAVE] = s;
  __syncthreads();
  if (t == 0) {
    double a = 0.0;
    for (int w = 0; w < NS / SCAE_WAVE; ++w) a += red[w];
    *out = a;
  }
}

// grid (ceil(N / (4 RW)), G), 4 waves; wave w of workgroup b takes rows (4 b + w) RW ...
template <int M, int RW, bool KL>
__global__ __launch_bounds__(256) void tsne_grad_kernel(const float *P, const float *Y, int N,
                                                        int G, float *part) {
  const int lane = threadIdx.x % SCAE_WAVE;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / SCAE_WAVE);
  const int g = blockIdx.y, jb = g * (SCAE_WAVE * M) + lane;
  const float2 *Y2 = reinterpret_cast<const float2 *>(Y);
  float yj0[M], yj1[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int j = jb + SCAE_WAVE * m;
    const float2 v = j < N ? Y2[j] : make_float2(0.f, 0.f);
    yj0[m] = v.x, yj1[m] = v.y;
  }
  const int r0 = (blockIdx.x * 4 + w) * RW;
  float keep[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) keep[c] = 0.f;
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    const int i = r0 + r;   // wave-uniform
    if (i < N) {
      const float2 yi = Y2[i];
      const float *Pi = P + (size_t)i * N + jb;
      float pv[M];
#pragma unroll
      for (int m = 0; m < M; ++m) pv[m] = jb + SCAE_WAVE * m < N ? Pi[SCAE_WAVE * m] : 0.f;
      float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f, z = 0.f, kl = 0.f;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const int j = jb + SCAE_WAVE * m;
        const float dy0 = yi.x - yj0[m], dy1 = yi.y - yj1[m];
        const float d = fmaf(dy1, dy1, dy0 * dy0);
        const float q = j < N && j != i ? 1.f / (1.f + d) : 0.f;
        const float pq = pv[m] * q, q2 = q * q;
        a0 = fmaf(pq, dy0, a0), a1 = fmaf(pq, dy1, a1);
        b0 = fmaf(q2, dy0, b0), b1 = fmaf(q2, dy1, b1);
        z += q;
        if constexpr (KL) kl = fmaf(pv[m], log1pf(d), kl);   // (P = 0 on the diagonal and past N)
      }
      a0 = scae::wave_sum(a0), a1 = scae::wave_sum(a1);
      b0 = scae::wave_sum(b0), b1 = scae::wave_sum(b1);
      z = scae::wave_sum(z);
      if constexpr (KL) kl = scae::wave_sum(kl);
      if (lane == r) keep[0] = a0, keep[1] = a1, keep[2] = b0, keep[3] = b1, keep[4] = z, keep[5] = kl;
    }
  }
  if (lane < RW && r0 + lane < N) {
#pragma unroll
    for (int c = 0; c < (KL ? NC : NC - 1); ++c)
      part[((size_t)c * G + g) * N + r0 + lane] = keep[c];
  }
}

// grid (ceil(N / NU)): rows (c, i) = sum_g part (c, g, i) in g order; block (0 | 1, b) = the
// workgroup's fp64 sum of z | kl
template <bool KL>
__global__ __launch_bounds__(NU) void tsne_rows_kernel(scae_tsne_desc d) {
  __shared__ double red[NU / SCAE_WAVE];
  const int i = blockIdx.x * NU + threadIdx.x, N = d.N, G = d.G;
  float z = 0.f, kl = 0.f;
  if (i < N) {
#pragma unroll
    for (int c = 0; c < (KL ? NC : NC - 1); ++c) {
      float s = 0.f;
      for (int g = 0; g < G; ++g) s += d.part[((size_t)c * G + g) * N + i];
      d.rows[(size_t)c * N + i] = s;
      if (c == 4) z = s;
      if (c == 5) kl = s;
    }
  }
  tsne_block_z_kl<KL>(z, kl, d.block, MAXB, red);
}

template <int M, int RW>
void launch_grad(const scae_tsne_desc &d, bool kl, hipStream_t st) {
  const dim3 grid((d.N + 4 * RW - 1) / (4 * RW), d.G);
  if (kl)
    scae::launch(tsne_grad_kernel<M, RW, true>, grid, dim3(256), 0, st, d.P, d.Y, d.N, d.G, d.part);
  else
    scae::launch(tsne_grad_kernel<M, RW, false>, grid, dim3(256), 0, st, d.P, d.Y, d.N, d.G, d.part);
}

// the gradient's sums of one iteration into rows (kl: the recorded form)
void sum_gradient(const scae_tsne_desc &d, bool kl, hipStream_t st) {
  const int nb = (d.N + NU - 1) / NU;
  if (d.N <= SMALL_N)
    launch_grad<4, 4>(d, kl, st);
  else
    launch_grad<16, 8>(d, kl, st);
  if (kl)
    scae::launch(tsne_rows_kernel<true>, dim3(nb), dim3(NU), 0, st, d);
  else
    scae::launch(tsne_rows_kernel<false>, dim3(nb), dim3(NU), 0, st, d);
}
}  // namespace

extern "C" int scae_tsne_supported(int N, int F) {
  return N >= 2 && N <= SCAE_TSNE_MAX_N && F >= 1 && F <= SCAE_TSNE_MAX_F;
}

extern "C" int scae_tsne_groups(int N) {
  if (N < 2 || N > SCAE_TSNE_MAX_N) return 0;
  const int cols = SCAE_WAVE * (N <= SMALL_N ? 4 : 16);
  return (N + cols - 1) / cols;
}

extern "C" int scae_tsne_affinities_f32(const float *x, int N, int F, float perplexity, float *P,
                                        float *beta, double *part, double *plogp, void *stream) {
  SCAE_REQUIRE(x && P && beta && part && plogp);
  if (!scae_tsne_supported(N, F)) return SCAE_ERR_UNSUPPORTED;
  SCAE_REQUIRE(perplexity > 0.f && 3.f * perplexity <= (float)(N - 1));
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)((N + 3) / 4 * 4) * sizeof(float);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(tsne_beta_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const int TD = (N + DT - 1) / DT, T = (N + ST - 1) / ST;
  scae::launch(tsne_dist_kernel, dim3(TD, TD), dim3(256), 0, st, x, N, F, P);
  scae::launch(tsne_beta_kernel, dim3(N), dim3(NB), lds, st, P, N, logf(perplexity), beta);
  scae::launch(tsne_sym_kernel, dim3(T, T), dim3(256), 0, st, P, N, part);
  scae::launch(tsne_sum_kernel, dim3(1), dim3(NS), 0, st, (const double *)part,
               (int64_t)pair_index(T - 1, T - 1, T) + 1, plogp);
  return scae_launch_status();
}

extern "C" int scae_tsne_run_f32(const scae_tsne_desc *dp, int first_iter, int n, void *stream) {
  SCAE_REQUIRE(dp && first_iter >= 0 && n >= 0);
  const scae_tsne_desc d = *dp;
  SCAE_REQUIRE(d.P && d.Y && d.velocity && d.gains && d.part && d.rows && d.block && d.plogp &&
               d.history && d.n_iter > 0 && d.check_every > 0 && d.exaggeration_iter >= 0 &&
               first_iter + n <= d.n_iter);
  if (!scae_tsne_supported(d.N, 1)) return SCAE_ERR_UNSUPPORTED;
  SCAE_REQUIRE(d.G == scae_tsne_groups(d.N));
  hipStream_t st = (hipStream_t)stream;
  tsne_run(d, MAXB, first_iter, n, st, [&](bool kl) { sum_gradient(d, kl, st); });
  return scae_launch_status();
}
