// K1, fused mode / mean: distributions.py:37-39 / :50-77 of the mixture part_decoder.py:174-237
// builds, straight from the compact decoder inputs -- the reconstruction image without the two
// (B,K,.,H,W) tensors of the materialising path (render_gmm.hip / render_gmm_wave.hip, then
// gmm_mean_mode_kernel), and with its bits.
//
// MUST BE COMPILED WITH -ffp-contract=off (csrc/Makefile gives this file the flag; any other
// build of it has to as well).  Under HIP's default -ffp-contract=fast the backend fuses products
// into sums whatever a `#pragma clang fp contract(off)` says, and the bitwise contract with the
// materialising kernels rests on every rounding below happening as written: only an explicit
// fmaf is an fma here.
//
// What is restated below -- the contraction choices in render_fwd_kernel / render_wave_kernel /
// gmm_mean_mode_kernel and the device library's expf / logf sequences inside them -- was read
// from the code ROCm 7.2.0 (AMD clang 22.0.0git, roc-7.2.0) generates for those translation
// units.  Another compiler release, or an edit of those kernels that changes how they are
// contracted, can move their bits; tests/test_image_log_gpu.py (mode and mean bit for bit
// against the materialising path, and a sweep of the scalar parameters) is the check that this
// file still follows them.
#include "common.h"
#include "render_gmm_dev.h"

namespace {

using namespace scae_k1;

constexpr int NT = 256;

// ---------------------------------------------------------------------------
// fused mode / mean: the reconstruction image straight from the compact inputs.
// One workgroup per (pixel tile, image); a lane owns a pixel and walks the M templates and the
// background in component order, so the result has the bits of render + gmm_mean_mode_kernel
// without the two (B,K,.,H,W) tensors: the components' values and logits come from the same
// arithmetic as the materialising kernel the launcher would pick -- LERP: render_gmm_wave.hip's
// nested-fma blend, else render_fwd_kernel's four weighted taps.
// The planes of `kchunk` templates are staged at a time (all M when they fit: one staging per
// workgroup, several pixel rounds; else one round and a restaging per chunk, and the mean's
// second pass stages them again rather than rescale a running sum -- same bits either way).
// ---------------------------------------------------------------------------
// The compiler contracts the shared helpers differently from kernel to kernel (the affine map
// is fma(a1, yn, a0 xn) in render_fwd_kernel and two rounded products in the quad-store form;
// a template tap sum is an fma chain, the alpha tap sum four rounded products), so what the two
// materialising kernels execute is spelled out here with explicit roundings: nothing in
// mode_ptaps / mode_sample / ModeState is left for contraction to decide (this file is
// compiled with -ffp-contract=off, csrc/Makefile: the rounding intrinsics are plain operators to
// the compiler, only an explicit fmaf is an fma here).
template <bool LERP>
__device__ __forceinline__ void mode_ptaps(const float *a, int p, int W, int H, int tw, int th,
                                           PTaps &t) {
  const float inv_w = 1.f / (float)W;
  const int i = (int)(((float)p + 0.5f) * inv_w), j = p - i * W;  // exact for p < 2^22
  t.xn = fmaf((float)(2 * j + 1), inv_w, -1.f);
  t.yn = fmaf((float)(2 * i + 1), 1.f / (float)H, -1.f);
  float gx, gy;
  if (LERP) {
    gx = __fadd_rn(__fadd_rn(__fmul_rn(a[0], t.xn), __fmul_rn(a[1], t.yn)), a[2]);
    gy = __fadd_rn(__fadd_rn(__fmul_rn(a[3], t.xn), __fmul_rn(a[4], t.yn)), a[5]);
  } else {
    gx = __fadd_rn(fmaf(a[1], t.yn, __fmul_rn(a[0], t.xn)), a[2]);
    gy = __fadd_rn(fmaf(a[4], t.yn, __fmul_rn(a[3], t.xn)), a[5]);
  }
  float ix = __fmul_rn(fmaf(__fadd_rn(gx, 1.f), (float)tw, -1.f), 0.5f);
  float iy = __fmul_rn(fmaf(__fadd_rn(gy, 1.f), (float)th, -1.f), 0.5f);
  ix = fminf(fmaxf(ix, -2.f), (float)tw);  // fmaxf(NaN, -2) = -2
  iy = fminf(fmaxf(iy, -2.f), (float)th);
  const float x0f = floorf(ix), y0f = floorf(iy);
  t.fx = ix - x0f;
  t.fy = iy - y0f;
  t.base = ((int)y0f + 2) * pad_w(tw) + (int)x0f + 2;
}

// ALPHA: the plane is the alpha plane (render_fwd_kernel sums its four products unfused)
template <bool LERP, bool ALPHA>
__device__ __forceinline__ float mode_sample(const float *plane, const PTaps &t, int pw) {
  const float *q0 = plane + t.base, *q1 = q0 + pw;
  const float v00 = q0[0], v01 = q0[1], v10 = q1[0], v11 = q1[1];
  if (LERP) {
    const float t0 = fmaf(t.fx, v01 - v00, v00), t1 = fmaf(t.fx, v11 - v10, v10);
    return fmaf(t.fy, t1 - t0, t0);
  }
  const float wx1 = t.fx, wx0 = 1.f - t.fx, wy1 = t.fy, wy0 = 1.f - t.fy;
  const float w00 = __fmul_rn(wx0, wy0), w01 = __fmul_rn(wx1, wy0);
  const float w10 = __fmul_rn(wx0, wy1), w11 = __fmul_rn(wx1, wy1);
  if (ALPHA)
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(v00, w00), __fmul_rn(v01, w01)),
                               __fmul_rn(v10, w10)),
                     __fmul_rn(v11, w11));
  return fmaf(v11, w11, fmaf(v10, w10, fmaf(v00, w00, __fmul_rn(v01, w01))));
}

// expf as the device library evaluates it inside gmm_mean_mode_kernel (whose translation unit
// contracts its products): two-term log2 e split, round to nearest, v_exp_f32, ldexp, and the
// underflow / overflow selects.  tests/test_image_log_gpu.py holds the mean to that kernel's bits.
__device__ __forceinline__ float mode_expf(float x) {
  const float c = __int_as_float(0x3fb8aa3b), cc = __int_as_float(0x32a5705f);
  const float ph = x * c, e = rintf(ph);
  const float pl = fmaf(cc, x, fmaf(x, c, -ph));
  float r = ldexpf(__builtin_amdgcn_exp2f((ph - e) + pl), (int)e);
  r = __int_as_float(0xc2ce8ed0) > x ? 0.f : r;
  return __int_as_float(0x42b17218) < x ? INFINITY : r;
}

// log_safe likewise, as the render kernels' translation units evaluate its logf (their last
// step is contracted: fma(y, ln 2, low part)).  The library scales denormal arguments by 2^32
// first; log_safe never takes the logarithm below kLogSafeEps, so that branch is not restated.
static_assert(scae::kLogSafeEps >= 1.17549435e-38f,
              "mode_log_safe omits logf's denormal scaling: kLogSafeEps must be a normal number");
__device__ __forceinline__ float mode_log_safe(float x) {
  if (x < scae::kLogSafeEps) return scae::kLogSafeFloor;
  const float c = __int_as_float(0x3f317217), cl = __int_as_float(0x3377d1cf);
  const float y = __builtin_amdgcn_logf(x), ph = y * c;
  const float r = fmaf(y, c, fmaf(y, cl, fmaf(y, c, -ph)));
  return fabsf(y) < INFINITY ? r : y;
}

template <int C>
struct ModeState {
  float best[C], val[C];     // mode: largest logit so far and its component's value
  float m[C], s[C], acc[C];  // mean: max logit (pass 0), sum of exp and weighted sum (pass 1)
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      best[c] = m[c] = -INFINITY;
      val[c] = s[c] = acc[c] = 0.f;
    }
  }
  // component k with values v and logits ml (ml[0] alone when the logits have one channel)
  __device__ __forceinline__ void add(int k, const float (&v)[C], const float (&ml)[C],
                                      bool one_logit, bool mean, int pass) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float l = ml[one_logit ? 0 : c];
      if (!mean) {  // strict >, the lowest k wins; component 0 when no logit compares greater
        const bool take = l > best[c];
        if (take) best[c] = l;
        if (take || k == 0) val[c] = v[c];
      } else if (pass == 0) {
        m[c] = fmaxf(m[c], l);
      } else {
        const float e = mode_expf(l - m[c]);
        s[c] += e;
        acc[c] = __fadd_rn(acc[c], __fmul_rn(e, v[c]));  // (the generic kernel does not fuse)
      }
    }
  }
};

template <int C, bool LERP>
__global__ __launch_bounds__(NT) void render_mode_kernel(scae_decoder_desc d,
                                                         float *__restrict__ out, int mean,
                                                         int first, int tiles, int ppb,
                                                         int kchunk) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int img = blockIdx.x / tiles, tile = blockIdx.x - img * tiles;
  const int b = first + img, tid = threadIdx.x;
  const int M = d.M, HW = d.H * d.W, tsz = d.th * d.tw;
  const bool alpha_mode = d.templates_alpha != nullptr;
  const Scalars sc = load_scalars(d);
  const int psz = pad_elems(d.th, d.tw), pw = pad_w(d.tw);
  float *s_tmpl = smem;                                       // kchunk * C planes
  float *s_alpha = s_tmpl + (size_t)kchunk * C * psz;         // kchunk planes (alpha mode)
  float *s_pose = s_alpha + (alpha_mode ? kchunk * psz : 0);  // kchunk * 6
  float *s_lsp = s_pose + kchunk * 6;                         // kchunk
  const bool one_stage = kchunk >= M;
  const int p_begin = tile * ppb, p_end = min(p_begin + ppb, HW);
  const int passes = mean ? 2 : 1;

  for (int r0 = p_begin; r0 < p_end; r0 += NT) {  // (one round when the templates are chunked)
    const int p = r0 + tid;
    const bool live = p < p_end;
    const int pc = live ? p : p_begin;
    ModeState<C> st;
    st.init();
    for (int pass = 0; pass < passes; ++pass) {
      for (int k0 = 0; k0 < M; k0 += kchunk) {
        const int nk = min(kchunk, M - k0);
        if (!one_stage || (r0 == p_begin && pass == 0)) {
          __syncthreads();  // every lane is done with the planes staged before
          stage_padded<NT>(s_tmpl, d.templates + ((size_t)tb(d, b) * M + k0) * C * tsz, nk * C,
                           d.th, d.tw);
          if (alpha_mode)
            stage_padded<NT>(s_alpha, d.templates_alpha + (size_t)k0 * tsz, nk, d.th, d.tw);
          for (int i = tid; i < nk * 6; i += NT)
            s_pose[i] = d.pose[((size_t)b * M + k0) * 6 + i];
          for (int i = tid; i < nk; i += NT)
            s_lsp[i] = d.presence ? mode_log_safe(d.presence[(size_t)b * M + k0 + i]) : 0.f;
          __syncthreads();
        }
        for (int kl = 0; kl < nk; ++kl) {
          PTaps t;
          mode_ptaps<LERP>(s_pose + kl * 6, pc, d.W, d.H, d.tw, d.th, t);
          const float lsp = s_lsp[kl];
          float v[C], ml[C];
          if (alpha_mode)
            ml[0] = __fadd_rn(mode_sample<LERP, true>(s_alpha + kl * psz, t, pw), lsp);
#pragma unroll
          for (int c = 0; c < C; ++c) {
            v[c] = mode_sample<LERP, false>(s_tmpl + (kl * C + c) * psz, t, pw);
            if (!alpha_mode) ml[c] = __fadd_rn(__fdiv_rn(v[c], sc.temperature), lsp);
          }
          st.add(k0 + kl, v, ml, alpha_mode, mean, pass);
        }
      }
      {  // background component (k = M), part_decoder.py:189-195, :210-213
        float v[C], ml[C];
        if (alpha_mode) ml[0] = sc.bg_ml;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          v[c] = d.bg_image ? d.bg_image[((size_t)b * C + c) * HW + pc] : sc.bg_val;
          if (!alpha_mode) ml[c] = __fdiv_rn(v[c], sc.temperature);
        }
        st.add(M, v, ml, alpha_mode, mean, pass);
      }
    }
    if (live) {
#pragma unroll
      for (int c = 0; c < C; ++c)
        out[((size_t)img * C + c) * HW + p] = mean ? st.acc[c] / st.s[c] : st.val[c];
    }
  }
}

}  // namespace

// ---- fused mode / mean -------------------------------------------------------------------
namespace {
#ifndef SCAE_MODE_LDS_KB
#define SCAE_MODE_LDS_KB 64   // planes staged per workgroup: two workgroups share a CU's LDS
#endif
template <int C>
int launch_render_mode(const scae_decoder_desc *d, float *out, int mean, int first, int count,
                       hipStream_t st) {
  const int HW = d->H * d->W;
  // floats per staged template: its C (+ alpha) padded planes, pose and log presence
  const size_t per_k =
      (size_t)(d->C + (d->templates_alpha ? 1 : 0)) * pad_elems(d->th, d->tw) + 7;
  size_t kchunk = (size_t)SCAE_MODE_LDS_KB * 1024 / sizeof(float) / per_k;
  kchunk = kchunk < 1 ? 1 : (kchunk > (size_t)d->M ? (size_t)d->M : kchunk);
  const size_t lds = sizeof(float) * kchunk * per_k;
  // pixel tiles: one 256-pixel round per workgroup while the slice alone cannot fill the
  // CUs (or the templates are chunked), else the whole image behind one staging
  const int rounds = (HW + NT - 1) / NT;
  int tiles = rounds;
  if ((int)kchunk >= d->M) {
    const int want = (512 + count - 1) / count;
    tiles = want < rounds ? want : rounds;
  }
  const int ppb = ((HW + tiles - 1) / tiles + NT - 1) / NT * NT;
  tiles = (HW + ppb - 1) / ppb;
  // the arithmetic of the materialising form scae_template_render_fwd_f32 takes for d (its
  // output tensors are 16-byte aligned allocations)
  bool lerp = false;
#ifndef SCAE_K1_NO_WAVE
  lerp = render_wave_lds(d) && (!d->bg_image || ((size_t)d->bg_image & 15) == 0);
#endif
  int rc;
#define SCAE_LAUNCH_MODE(LP)                                                                \
  rc = set_lds(render_mode_kernel<C, LP>, lds);                                             \
  if (rc) return rc;                                                                        \
  scae::launch((render_mode_kernel<C, LP>), dim3((unsigned)count * tiles), dim3(NT), lds, st, \
               *d, out, mean, first, tiles, ppb, (int)kchunk)
  if (lerp) {
    SCAE_LAUNCH_MODE(true);
  } else {
    SCAE_LAUNCH_MODE(false);
  }
#undef SCAE_LAUNCH_MODE
  return scae_launch_status();
}
}  // namespace

extern "C" int scae_render_gmm_mode_f32(const scae_decoder_desc *d, float *out, int what,
                                        int first, int count, void *stream) {
  int rc = check_decoder_desc(d);
  if (rc) return rc;
  SCAE_REQUIRE(out && (what == 0 || what == 1));
  SCAE_REQUIRE(first >= 0 && count > 0 && first <= d->B - count);
#define CALL(CC) launch_render_mode<CC>(d, out, what, first, count, (hipStream_t)stream)
  switch (d->C) {
    case 1: return CALL(1);
    case 2: return CALL(2);
    case 3: return CALL(3);
    case 4: return CALL(4);
    default: return SCAE_ERR_UNSUPPORTED;
  }
#undef CALL
}
