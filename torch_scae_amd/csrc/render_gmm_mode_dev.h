// Component arithmetic and launch geometry shared by the kernels that walk the decoder's
// mixture per pixel straight from its compact inputs: render_gmm_mode.hip (mode / mean) and
// render_gmm_parts.hip (the E-step: per-pixel responsibilities, owners, per-part mass).
//
// EVERY TRANSLATION UNIT THAT INCLUDES THIS MUST BE COMPILED WITH -ffp-contract=off
// (csrc/Makefile gives both files the flag).  Under HIP's default -ffp-contract=fast the backend
// fuses products into sums whatever a `#pragma clang fp contract(off)` says, and the bitwise
// contract with the materialising kernels rests on every rounding below happening as written:
// only an explicit fmaf is an fma here.
//
// What is restated below -- the contraction choices in render_fwd_kernel / render_wave_kernel /
// gmm_mean_mode_kernel and the device library's expf / logf sequences inside them -- was read
// from the code ROCm 7.2.0 (AMD clang 22.0.0git, roc-7.2.0) generates for those translation
// units.  Another compiler release, or an edit of those kernels that changes how they are
// contracted, can move their bits; tests/test_image_log_gpu.py (mode and mean bit for bit
// against the materialising path, and a sweep of the scalar parameters) is the check that this
// file still follows them.
#pragma once
#include "common.h"
#include "render_gmm_dev.h"

namespace scae_k1 {

// The compiler contracts the shared helpers differently from kernel to kernel (the affine map
// is fma(a1, yn, a0 xn) in render_fwd_kernel and two rounded products in the quad-store form;
// a template tap sum is an fma chain, the alpha tap sum four rounded products), so what the two
// materialising kernels execute is spelled out here with explicit roundings: nothing in
// mode_ptaps / mode_sample is left for contraction to decide (the rounding intrinsics are plain
// operators to the compiler under -ffp-contract=off, only an explicit fmaf is an fma).
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

// ---- launch geometry ------------------------------------------------------------------
#ifndef SCAE_MODE_LDS_KB
#define SCAE_MODE_LDS_KB 64   // planes staged per workgroup: two workgroups share a CU's LDS
#endif
constexpr int kModeThreads = 256;

struct ModeGeom {
  int kchunk;   // templates staged at a time (>= M: the image's planes are staged once)
  size_t lds;   // bytes of the staged planes, poses and log presences
  int tiles;    // workgroups per image
  int ppb;      // pixels per workgroup, a multiple of kModeThreads
  bool lerp;    // the quad-store render form's arithmetic (else the four weighted taps)
};

inline ModeGeom mode_geom(const scae_decoder_desc *d, int count) {
  ModeGeom g;
  const int HW = d->H * d->W, NT = kModeThreads;
  // floats per staged template: its C (+ alpha) padded planes, pose and log presence
  const size_t per_k =
      (size_t)(d->C + (d->templates_alpha ? 1 : 0)) * pad_elems(d->th, d->tw) + 7;
  size_t kchunk = (size_t)SCAE_MODE_LDS_KB * 1024 / sizeof(float) / per_k;
  kchunk = kchunk < 1 ? 1 : (kchunk > (size_t)d->M ? (size_t)d->M : kchunk);
  g.kchunk = (int)kchunk;
  g.lds = sizeof(float) * kchunk * per_k;
  // pixel tiles: one 256-pixel round per workgroup while the slice alone cannot fill the
  // CUs (or the templates are chunked), else the whole image behind one staging
  const int rounds = (HW + NT - 1) / NT;
  int tiles = rounds;
  if (g.kchunk >= d->M) {
    const int want = (512 + count - 1) / count;
    tiles = want < rounds ? want : rounds;
  }
  g.ppb = ((HW + tiles - 1) / tiles + NT - 1) / NT * NT;
  g.tiles = (HW + g.ppb - 1) / g.ppb;
  // the arithmetic of the materialising form scae_template_render_fwd_f32 takes for d (its
  // output tensors are 16-byte aligned allocations)
  g.lerp = false;
#ifndef SCAE_K1_NO_WAVE
  g.lerp = render_wave_lds(d) && (!d->bg_image || ((size_t)d->bg_image & 15) == 0);
#endif
  return g;
}

}  // namespace scae_k1
