// Linear probe for gfx950 (probe.py): multinomial logistic regression on the standardised
// capsule features, FISTA with gradient restart, R regularisation strengths side by side.
//
// Rows are cut into G = scae_probe_groups(N, F) groups of whole 64-row tiles; group g owns one
// contiguous row range, whatever R is.
//   pb_moments_kernel   grid (G): the group's fp64 partial of [x 1]^T [x 1], labels outside
//                       [0, C) counted (integer atomic); pb_moments_reduce_kernel adds the
//                       partials in g order.
// One iteration is two launches:
//   pb_grad_kernel      grid (G): each tile is standardised into LDS once and serves every
//                       running problem in turn -- the problem's V in LDS, logits, a
//                       max-subtracted softmax, the rows' losses (fp64) and the tile's
//                       (P - Y)^T Z in row order, added to the group's partial;
//   pb_update_kernel    grid (R): the G partials in g order (fp64), the FISTA update, one
//                       history row and the stop decision.  It runs as a launch of its own and
//                       not as the last-arriving workgroup of the gradient launch: the stream
//                       orders the two, so no workgroup reads another's partials inside a
//                       launch.
// No float atomics, every sum in a fixed order: two runs give the same bits, and a problem's
// bits do not depend on the problems solved beside it.  The launches of a stopped problem
// leave its state untouched.  The fp64 wave sum is reduce_f64_dev.h's.
#include "common.h"
#include "reduce_f64_dev.h"

namespace {
constexpr int TR = 64;     // rows per tile
constexpr int NT = 256;    // gradient / moments / predict workgroup
constexpr int NTU = 1024;  // update workgroup
constexpr int ST = SCAE_PROBE_STATE_INTS;
constexpr int PREDICT_BLOCKS = 1024;
constexpr size_t LDS_MAX = 160 * 1024;

using scae_reduce::wave_sum_f64;
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

__host__ __device__ inline int odd_stride(int F) { return (F + 1) | 1; }  // (bank spread)
__host__ __device__ inline int pad4(int n) { return (n + 3) & ~3; }

int64_t tiles_of(int64_t N) { return (N + TR - 1) / TR; }
int64_t tiles_per_group(int64_t N, int F) {
  int64_t gmax = SCAE_PROBE_MAX_CF / (F + 1);
  gmax = gmax < 64 ? 64 : gmax > 256 ? 256 : gmax;
  const int64_t tiles = tiles_of(N);
  return (tiles + gmax - 1) / gmax;
}

// ---- moments ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void pb_moments_kernel(const float *x, const int64_t *y,
                                                        int64_t N, int F, int C, int tpg,
                                                        double *part, int *outside) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int g = blockIdx.x, t = threadIdx.x, F1 = F + 1, XS = odd_stride(F);
  const int64_t tiles = (N + TR - 1) / TR;
  const int64_t t0 = (int64_t)g * tpg, t1 = t0 + tpg < tiles ? t0 + tpg : tiles;
  double *pg = part + (size_t)g * F1 * F1;
  int bad = 0;
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t row0 = tile * TR;
    const int rows = N - row0 < TR ? (int)(N - row0) : TR;
    for (int i = t; i < TR * F1; i += NT) {
      const int row = i / F1, f = i - row * F1;
      float v = 0.f;
      if (row < rows) v = f < F ? x[(row0 + row) * F + f] : 1.f;
      smem[row * XS + f] = v;
    }
    if (y && t < rows) {
      const int64_t l = y[row0 + t];
      bad += l < 0 || l >= C;
    }
    __syncthreads();
    for (int p = t; p < F1 * F1; p += NT) {
      const int i = p / F1, j = p - i * F1;
      double s = 0.0;
      for (int row = 0; row < TR; ++row)
        s = fma((double)smem[row * XS + i], (double)smem[row * XS + j], s);
      pg[p] = tile == t0 ? s : pg[p] + s;
    }
    __syncthreads();  // (the tile is rewritten)
  }
  if (bad) atomicAdd(outside, bad);
}

__global__ __launch_bounds__(NT) void pb_moments_reduce_kernel(const double *part, int G, int n,
                                                               double *out) {
  const int p = blockIdx.x * NT + threadIdx.x;
  if (p >= n) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += part[(size_t)g * n + p];
  out[p] = s;
}

// ---- one iteration ---------------------------------------------------------------------------
size_t grad_lds(int F, int C, int R) {
  const int ZS = odd_stride(F);
  return (size_t)R * TR * sizeof(double) +
         (size_t)(2 * pad4(F) + TR * ZS + pad4(C * ZS) + C * TR + TR) * sizeof(float);
}

__global__ __launch_bounds__(NT) void pb_grad_kernel(scae_probe_desc d, int tpg) {
  const int *state = d.state;
  const int R = d.R;
  if (state[R * ST] >= R) return;  // every problem has stopped
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int g = blockIdx.x, t = threadIdx.x, F = d.F, C = d.C, F1 = F + 1, CF = C * F1;
  const int ZS = odd_stride(F), G = d.G;
  const int64_t N = d.N;
  double *lacc = reinterpret_cast<double *>(smem);          // (R, TR) the rows' losses
  float *ms = reinterpret_cast<float *>(lacc + R * TR);     // (F) means
  float *ds = ms + pad4(F);                                 // (F) scales
  float *Zt = ds + pad4(F);                                 // (TR, ZS) the standardised tile
  float *Vs = Zt + TR * ZS;                                 // (C, ZS) the problem's V
  float *Lg = Vs + pad4(C * ZS);                            // (C, TR) logits, then P - Y
  int *ys = reinterpret_cast<int *>(Lg + C * TR);           // (TR) labels
  for (int f = t; f < F; f += NT) ms[f] = d.mean[f], ds[f] = d.scale[f];
  for (int i = t; i < R * TR; i += NT) lacc[i] = 0.0;
  __syncthreads();
  const int64_t tiles = (N + TR - 1) / TR;
  const int64_t t0 = (int64_t)g * tpg, t1 = t0 + tpg < tiles ? t0 + tpg : tiles;
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t row0 = tile * TR;
    const int rows = N - row0 < TR ? (int)(N - row0) : TR;
    for (int i = t; i < TR * F1; i += NT) {
      const int row = i / F1, f = i - row * F1;
      float v = 0.f;
      if (row < rows) v = f < F ? (d.x[(row0 + row) * F + f] - ms[f]) * ds[f] : 1.f;
      Zt[row * ZS + f] = v;
    }
    if (t < TR) {  // (labels were counted by the moments launch; a stray one stays inside Lg)
      const int64_t l = t < rows ? d.y[row0 + t] : 0;
      ys[t] = l < 0 ? 0 : l >= C ? C - 1 : (int)l;
    }
    // (Zt / ys are first read behind the barrier that follows the V load)
    for (int r = 0; r < R; ++r) {
      if (state[r * ST]) continue;  // stopped: uniform over the workgroup
      const float *V = d.V + (size_t)r * CF;
      for (int i = t; i < CF; i += NT) {
        const int c = i / F1, f = i - c * F1;
        Vs[c * ZS + f] = V[i];
      }
      __syncthreads();
      {  // logits: a wave takes one class at a time (V broadcast), a lane one row
        const int row = t & (TR - 1);
        const float *z = Zt + row * ZS;
        for (int c = t / TR; c < C; c += NT / TR) {
          const float *v = Vs + c * ZS;
          float s = 0.f;
          for (int f = 0; f < F1; ++f) s = fmaf(z[f], v[f], s);
          Lg[c * TR + row] = s;
        }
      }
      __syncthreads();
      if (t < TR) {
        if (t < rows) {
          float mx = Lg[t];
          for (int c = 1; c < C; ++c) mx = fmaxf(mx, Lg[c * TR + t]);
          float sum = 0.f;
          for (int c = 0; c < C; ++c) {
            const float e = expf(Lg[c * TR + t] - mx);
            sum += e;
          }
          const int yy = ys[t];
          const float ly = Lg[yy * TR + t];
          lacc[r * TR + t] += (double)((mx + logf(sum)) - ly);
          for (int c = 0; c < C; ++c) {
            const float p = expf(Lg[c * TR + t] - mx) / sum;
            Lg[c * TR + t] = c == yy ? p - 1.f : p;
          }
        } else {
          for (int c = 0; c < C; ++c) Lg[c * TR + t] = 0.f;
        }
      }
      __syncthreads();
      float *pg = d.part_grad + ((size_t)r * G + g) * CF;
      for (int p = t; p < CF; p += NT) {
        const int c = p / F1, f = p - c * F1;
        const float *dd = Lg + c * TR;
        float s = 0.f;
        for (int row = 0; row < TR; ++row) s = fmaf(dd[row], Zt[row * ZS + f], s);
        pg[p] = tile == t0 ? s : pg[p] + s;
      }
      __syncthreads();  // (Vs / Lg are rewritten by the next problem, Zt by the next tile)
    }
    __syncthreads();  // (every problem may have been skipped)
  }
  if (t < TR) {  // one wave: the rows' sums in a fixed tree
    for (int r = 0; r < R; ++r) {
      if (state[r * ST]) continue;
      const double s = wave_sum_f64(lacc[r * TR + t]);
      if (t == 0) d.part_loss[(size_t)r * G + g] = s;
    }
  }
}

__global__ __launch_bounds__(NTU) void pb_update_kernel(scae_probe_desc d) {
  const int r = blockIdx.x, t = threadIdx.x;
  int *st = d.state + r * ST;
  if (st[0]) return;
  constexpr int NW = NTU / SCAE_WAVE;
  __shared__ double s_dot[NW], s_pen[NW];
  __shared__ float s_max[NW];
  __shared__ int s_conv;
  __shared__ float s_beta;
  const int F1 = d.F + 1, CF = d.C * F1, G = d.G;
  const double N = (double)d.N, l2 = d.l2[r];
  const float l2f = (float)l2, stepf = (float)d.step[r];
  float *W = d.W + (size_t)r * CF, *V = d.V + (size_t)r * CF, *grad = d.grad + (size_t)r * CF;
  const float *part = d.part_grad + (size_t)r * G * CF;
  double dot = 0.0, pen = 0.0;
  float mx = 0.f;
  for (int p = t; p < CF; p += NTU) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += (double)part[(size_t)g * CF + p];
    const float v = V[p];
    float gf = (float)(s / N);
    if (p % F1 < d.F) {  // (the bias takes no penalty)
      gf = fmaf(l2f, v, gf);
      pen += (double)v * (double)v;
    }
    grad[p] = gf;
    const float wn = fmaf(-stepf, gf, v);
    dot += (double)gf * (double)(wn - W[p]);
    mx = fmaxf(mx, fabsf(gf));
  }
  dot = wave_sum_f64(dot);
  pen = wave_sum_f64(pen);
  mx = wave_max_f32(mx);
  const int wid = t / SCAE_WAVE;
  if (t % SCAE_WAVE == 0) s_dot[wid] = dot, s_pen[wid] = pen, s_max[wid] = mx;
  __syncthreads();
  if (t == 0) {
    double sd = 0.0, sp = 0.0, loss = 0.0;
    float m = 0.f;
    for (int w = 0; w < NW; ++w) sd += s_dot[w], sp += s_pen[w], m = fmaxf(m, s_max[w]);
    for (int g = 0; g < G; ++g) loss += d.part_loss[(size_t)r * G + g];
    const int it = st[1] + 1;
    const int conv = (double)m <= d.tol[r];
    const int stop = conv || it >= d.max_iter;
    const int restart = !conv && sd > 0.0;
    double *h = d.history + ((size_t)r * d.max_iter + (it - 1)) * 3;
    h[0] = loss / N + 0.5 * l2 * sp;
    h[1] = (double)m;
    h[2] = (double)restart;
    st[1] = it;
    st[3] += restart;
    float beta = 0.f;
    if (!conv) {
      const double tt = restart ? 1.0 : d.t[r];
      const double tn = 0.5 * (1.0 + sqrt(1.0 + 4.0 * tt * tt));
      beta = (float)((tt - 1.0) / tn);
      d.t[r] = tn;
    }
    if (stop) {
      st[0] = 1;
      st[2] = conv;
      atomicAdd(d.state + d.R * ST, 1);
    }
    s_conv = conv;
    s_beta = beta;
  }
  __syncthreads();
  if (s_conv) {  // the point whose gradient was measured is the result
    for (int p = t; p < CF; p += NTU) W[p] = V[p];
    return;
  }
  const float beta = s_beta;
  for (int p = t; p < CF; p += NTU) {
    const float v = V[p], w = W[p];
    const float wn = fmaf(-stepf, grad[p], v);
    V[p] = fmaf(beta, wn - w, wn);
    W[p] = wn;
  }
}

// ---- prediction --------------------------------------------------------------------------------
// block b takes rows b * NT + t, + gridDim.x * NT, ...; weight and bias in LDS as (C, F + 1)
__global__ __launch_bounds__(NT) void pb_predict_kernel(const float *x, int64_t N, int F, int C,
                                                        const float *weight, const float *bias,
                                                        const int64_t *y, int64_t *pred,
                                                        float *logp, double *part_ce) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ double red[NT / SCAE_WAVE];
  const int t = threadIdx.x, F1 = F + 1;
  for (int i = t; i < C * F1; i += NT) {
    const int c = i / F1, f = i - c * F1;
    smem[i] = f < F ? weight[c * F + f] : bias[c];
  }
  __syncthreads();
  double ce = 0.0;
  for (int64_t n = (int64_t)blockIdx.x * NT + t; n < N; n += (int64_t)gridDim.x * NT) {
    const float *xp = x + n * F;
    const int64_t yy = y ? y[n] : -1;
    float mx = -INFINITY, ly = 0.f;
    int best = 0;
    for (int c = 0; c < C; ++c) {
      const float *w = smem + c * F1;
      float s = 0.f;
      for (int f = 0; f < F; ++f) s = fmaf(xp[f], w[f], s);
      s += w[F];
      if (s > mx) mx = s, best = c;  // (ties to the lowest class)
      if (c == yy) ly = s;
    }
    float sum = 0.f;
    for (int c = 0; c < C; ++c) {
      const float *w = smem + c * F1;
      float s = 0.f;
      for (int f = 0; f < F; ++f) s = fmaf(xp[f], w[f], s);
      s += w[F];
      sum += expf(s - mx);
    }
    const float lse = logf(sum);  // (log sum exp, less the largest logit)
    pred[n] = best;
    logp[n] = -lse;
    if (yy >= 0 && yy < C) ce += (double)((mx - ly) + lse);
  }
  if (!part_ce) return;
  ce = wave_sum_f64(ce);
  if (t % SCAE_WAVE == 0) red[t / SCAE_WAVE] = ce;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int w = 0; w < NT / SCAE_WAVE; ++w) s += red[w];
    part_ce[blockIdx.x] = s;
  }
}

__global__ void pb_mean_kernel(const double *part, int n, int64_t N, double *out) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += part[i];
  *out = s / (double)N;
}

template <class K>
int allow_lds(K kernel, size_t lds) {
  if (lds <= 48 * 1024) return SCAE_OK;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  return e == hipSuccess ? SCAE_OK : (int)e;
}
}  // namespace

extern "C" int scae_probe_supported(int F, int C, int R) {
  return F > 0 && C > 0 && R > 0 && F <= SCAE_PROBE_MAX_F && C <= SCAE_PROBE_MAX_C &&
         C * (F + 1) <= SCAE_PROBE_MAX_CF && R <= SCAE_PROBE_MAX_R;
}

extern "C" int scae_probe_groups(int64_t N, int F) {
  if (N <= 0 || F <= 0 || F > SCAE_PROBE_MAX_F || N >= ((int64_t)1 << 31)) return 0;
  const int64_t tpg = tiles_per_group(N, F);
  return (int)((tiles_of(N) + tpg - 1) / tpg);
}

extern "C" int scae_probe_predict_blocks(int64_t N) {
  if (N <= 0) return 0;
  const int64_t b = (N + NT - 1) / NT;
  return (int)(b < PREDICT_BLOCKS ? b : PREDICT_BLOCKS);
}

extern "C" int scae_probe_moments_f64(const float *x, const int64_t *y, int64_t N, int F, int C,
                                      double *part, double *moments, int *outside,
                                      void *stream) {
  SCAE_REQUIRE(x && part && moments && N > 0 && N < ((int64_t)1 << 31) && F > 0 &&
               F <= SCAE_PROBE_MAX_F && (!y || (outside && C > 0)));
  const int G = scae_probe_groups(N, F), n = (F + 1) * (F + 1);
  const size_t lds = (size_t)TR * odd_stride(F) * sizeof(float);
  const int rc = allow_lds(pb_moments_kernel, lds);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  scae::launch(pb_moments_kernel, dim3(G), dim3(NT), lds, st, x, y, N, F, C,
               (int)tiles_per_group(N, F), part, outside);
  scae::launch(pb_moments_reduce_kernel, dim3((n + NT - 1) / NT), dim3(NT), 0, st, part, G, n,
               moments);
  return scae_launch_status();
}

extern "C" int scae_probe_fit_f32(const scae_probe_desc *dp, int n_iters, void *stream) {
  SCAE_REQUIRE(dp && n_iters >= 0);
  const scae_probe_desc d = *dp;
  SCAE_REQUIRE(d.x && d.y && d.mean && d.scale && d.l2 && d.step && d.tol && d.W && d.V &&
               d.grad && d.t && d.part_grad && d.part_loss && d.history && d.state &&
               d.N > 0 && d.N < ((int64_t)1 << 31) && d.max_iter > 0);
  if (!scae_probe_supported(d.F, d.C, d.R)) return SCAE_ERR_UNSUPPORTED;
  SCAE_REQUIRE(d.G == scae_probe_groups(d.N, d.F));
  const size_t lds = grad_lds(d.F, d.C, d.R);
  if (lds > LDS_MAX) return SCAE_ERR_UNSUPPORTED;
  const int rc = allow_lds(pb_grad_kernel, lds);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int tpg = (int)tiles_per_group(d.N, d.F);
  for (int i = 0; i < n_iters; ++i) {
    scae::launch(pb_grad_kernel, dim3(d.G), dim3(NT), lds, st, d, tpg);
    scae::launch(pb_update_kernel, dim3(d.R), dim3(NTU), 0, st, d);
  }
  return scae_launch_status();
}

extern "C" int scae_probe_predict_f32(const float *x, int64_t N, int F, int C,
                                      const float *weight, const float *bias, const int64_t *y,
                                      int64_t *pred, float *log_prob, double *part_ce,
                                      double *mean_ce, void *stream) {
  SCAE_REQUIRE(x && weight && bias && pred && log_prob && N > 0 && N < ((int64_t)1 << 31) &&
               (!y || (part_ce && mean_ce)));
  if (!scae_probe_supported(F, C, 1)) return SCAE_ERR_UNSUPPORTED;
  const size_t lds = (size_t)C * (F + 1) * sizeof(float);
  const int rc = allow_lds(pb_predict_kernel, lds);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = scae_probe_predict_blocks(N);
  scae::launch(pb_predict_kernel, dim3(blocks), dim3(NT), lds, st, x, N, F, C, weight, bias, y,
               pred, log_prob, y ? part_ce : (double *)nullptr);
  if (y) scae::launch(pb_mean_kernel, dim3(1), dim3(1), 0, st, part_ce, blocks, N, mean_ce);
  return scae_launch_status();
}
