// The output attention's backward (K2c, seed_attention_wave.hip) and the weight-gradient
// GEMMs of the capsule MLPs (K7, gemm_mfma.hip) in ONE launch.
//
// Both only wait for the data-gradient chain of the capsule MLPs (set_transformer.py:212-223
// backward needs the gradient of the object encoding; object_decoder.py:137-158 backward
// needs the pre-activation gradients), neither reads what the other writes, and kernels do
// not overlap on this stack.  Alone, the attention backward is one workgroup per set -- 128
// workgroups at B = 128, each a 15 us dependent chain on a quarter of the CUs -- and the four
// GEMMs are ~1.4 k short 32 x 32 split-K tiles that would fill the rest.  Here the
// attention workgroups are the head of the grid and the GEMM tiles its tail: 15.6 + 17.3 us
// as two launches.  Launch-uniform resources are the attention's (160 VGPRs, 47 KB of LDS
// at N, O <= 32 -- the only shape merged): the GEMM tiles (108 VGPRs, 18 KB on their own)
// still fit three workgroups per CU.
//
// Both device bodies come from their own files, compiled here without their kernels and
// entry points (SCAE_DEVICE_ONLY); each sits in a namespace of its own because the two tile
// vocabularies (scae_wave / scae_tile) share names.
#include <algorithm>

#include "mfma_tile.h"
#include "set_encoder_args.h"
#include "wave_mfma.h"

#define SCAE_DEVICE_ONLY
namespace scae_saw {
#include "seed_attention_wave.hip"
}
namespace scae_gemm {
#include "gemm_mfma.hip"
}
#include "set_encoder_wave.hip"   // (namespace scae_st)
#undef SCAE_DEVICE_ONLY

namespace {
constexpr int NTH = 256;
static_assert(scae_tile::NT == NTH, "one block size for both parts");

template <int NT, bool BF>
__global__ __launch_bounds__(NTH) void saw_bwd_gemm_kernel(scae_saw::SwArgs a, int n_saw,
                                                           scae_gemm::GemmMulti p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if ((int)blockIdx.x < n_saw)   // (the long dependent chains first)
    scae_saw::saw_bwd_body<NT, BF>(a, smem, blockIdx.x, n_saw);
  else
    scae_gemm::gemm_multi_body<1>(p, smem, (int)blockIdx.x - n_saw);
}

template <int NT, bool BF>
int launch(const scae_saw::SwArgs &a, const scae_gemm::GemmMulti &p, hipStream_t st) {
  const size_t lds = sizeof(float) * std::max<size_t>(scae_saw::Geo<NT>::LDS_FLOATS,
                                                      scae_tile::Tile<1>::SMEM);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(
        reinterpret_cast<const void *>(saw_bwd_gemm_kernel<NT, BF>),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const int n_saw = a.B < 512 ? a.B : 512;   // = scae_seed_attention_mfma_rows(B)
  scae::launch((saw_bwd_gemm_kernel<NT, BF>), dim3(n_saw + p.first[p.n]), dim3(NTH), lds,
                     st, a, n_saw, p);
  return scae_launch_status();
}

int impl(const float *h, const float *q, const float *wk, const float *wv,
         const float *presence, const float *gout, float *gh, float *partial, int B, int N,
         int O, int C, const scae_gemm_desc *descs, int n, int bf16, void *stream) {
  SCAE_REQUIRE(h && q && wk && wv && gout && gh && partial && descs);
  scae_saw::SwArgs a{h,  q,       wk, wv, nullptr, presence, nullptr, gout,
                     gh, partial, B,  N,  O,       C,        1.f / sqrtf((float)C), bf16};
  int rc = scae_saw::check(a);
  if (rc) return rc;
  scae_gemm::GemmMulti p;
  int T;
  rc = scae_gemm::plan_multi(p, T, descs, n);
  if (rc) return rc;
  if (T != 32) return SCAE_ERR_UNSUPPORTED;   // (large problems fill the device on their own)
  // sets of more than 32 elements: the attention's 4-tile form holds 268 VGPRs -- one GEMM
  // workgroup per SIMD instead of four; the two launches are faster apart
  if (N > 32 || O > 32) return SCAE_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  return bf16 ? launch<2, true>(a, p, st) : launch<2, false>(a, p, st);
}

// ---- ... and the trunk's backward (K2b, set_encoder_wave.hip) of the same set behind it ----
// The trunk's backward reads one thing the attention's writes: row b of gh, written by the
// workgroup of set b and read by the workgroup of set b.  With one set per workgroup (B <= 512)
// the head workgroups go on with the trunk's backward of their set: wave u of the attention
// ends holding key tile u of dh in the layout wave u of the trunk starts from, so the
// gradient is handed over in registers, the trunk's set-up and cold first touches sit behind
// the attention instead of behind a kernel boundary, and the GEMM tiles have a chain of two
// kernels' length to finish under.  The trunk's LDS image aliases the attention's tiles.
// NTS: the trunk's tile count (= waves); the attention's other waves leave before the trunk's
// first barrier, which then synchronises the waves that are left.
// Registers are launch-uniform: left alone the compiler spreads the trunk over 208 of them,
// and every GEMM workgroup is allocated as many.  Two workgroups per SIMD is what the LDS
// allows at NTS = 2 (57.6 KB); NTS = 1 fits three (156 registers, 47.1 KB).
template <int NTS, bool BF>
__global__ __launch_bounds__(NTH) __attribute__((amdgpu_waves_per_eu(2)))
void saw_stw_bwd_gemm_kernel(scae_saw::SwArgs a, int n_saw,
                                                               scae_gemm::GemmMulti p,
                                                               scae_st::StArgs t,
                                                               int trunk_lds_floats) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if ((int)blockIdx.x >= n_saw) {
    scae_gemm::gemm_multi_body<1>(p, smem, (int)blockIdx.x - n_saw);
    return;
  }
  // (n_saw = B: the body's loop runs once, and ends with a barrier behind its last LDS read)
  const scae_wave::f32x4 gh = scae_saw::saw_bwd_body<2, BF>(a, smem, blockIdx.x, n_saw);
  scae_st::lds_zero(smem, trunk_lds_floats, threadIdx.x, NTH);
  scae_wave::lds_fence();
  __syncthreads();
  if (threadIdx.x >= 64 * NTS) return;   // whole waves
  scae_st::stw_bwd_body<NTS, BF, true>(t, smem, blockIdx.x, n_saw, gh);
}

template <int NTS, bool BF>
int launch_trunk(const scae_saw::SwArgs &a, const scae_gemm::GemmMulti &p,
                 const scae_st::StArgs &t, hipStream_t st) {
  const size_t trunk = scae_st::stw_bwd_lds_floats<NTS>(t.Din);
  const size_t lds =
      sizeof(float) * std::max<size_t>({scae_saw::Geo<2>::LDS_FLOATS, scae_tile::Tile<1>::SMEM, trunk});
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(
        reinterpret_cast<const void *>(saw_stw_bwd_gemm_kernel<NTS, BF>),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  scae::launch((saw_stw_bwd_gemm_kernel<NTS, BF>), dim3(a.B + p.first[p.n]), dim3(NTH), lds, st,
               a, a.B, p, t, (int)trunk);
  return scae_launch_status();
}

bool trunk_rides(int B, int N, int O, int C, int D, int Din, int Dout, int L, int layer_norm) {
  return B > 0 && B <= 512 && N > 0 && N <= 32 && O > 0 && O <= 32 && C > 0 && (C & 63) == 0 &&
         D == scae_wave::D && Dout == 0 && scae_st::wave_bwd_shape(N, D, Din, Dout, L, layer_norm);
}

int impl_trunk(const float *h, const float *q, const float *wk, const float *wv,
               const float *presence, const float *gout, float *gh, float *partial, int B, int N,
               int O, int C, const scae_gemm_desc *descs, int n, int nseg,
               const float *const *seg_ptr, const int *seg_width, const int *seg_row_stride,
               const int64_t *seg_batch_stride, float *const *seg_grad,
               const float *trunk_presence, const float *params, const float *hsave,
               float *pg_partial, int B2, int N2, int D, int Din, int Dout, int L, int layer_norm,
               int bf16, void *stream) {
  SCAE_REQUIRE(h && q && wk && wv && gout && gh && partial && descs);
  if (B2 != B || N2 != N) return SCAE_ERR_BAD_ARG;
  scae_saw::SwArgs a{h,  q,       wk, wv, nullptr, presence, nullptr, gout,
                     gh, partial, B,  N,  O,       C,        1.f / sqrtf((float)C), bf16};
  int rc = scae_saw::check(a);
  if (rc) return rc;
  scae_st::StArgs t;
  rc = scae_st::wave_bwd_args(t, bf16 != 0, nseg, seg_ptr, seg_width, seg_row_stride,
                              seg_batch_stride, seg_grad, trunk_presence, params, hsave,
                              pg_partial, B, N, D, Din, Dout, L, layer_norm);
  if (rc) return rc;
  scae_gemm::GemmMulti p;
  int T;
  rc = scae_gemm::plan_multi(p, T, descs, n);
  if (rc) return rc;
  if (T != 32) return SCAE_ERR_UNSUPPORTED;
  if (!trunk_rides(B, N, O, C, D, Din, Dout, L, layer_norm)) return SCAE_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (N <= 16) return bf16 ? launch_trunk<1, true>(a, p, t, st) : launch_trunk<1, false>(a, p, t, st);
  return bf16 ? launch_trunk<2, true>(a, p, t, st) : launch_trunk<2, false>(a, p, t, st);
}
}  // namespace

extern "C" int scae_object_encoder_bwd_supported(int B, int N, int O, int C, int D, int Din,
                                                 int Dout, int L, int layer_norm) {
  return trunk_rides(B, N, O, C, D, Din, Dout, L, layer_norm) ? 1 : 0;
}
#define SCAE_OBJECT_ENCODER_BWD(SUFFIX, BF)                                                      \
  extern "C" int scae_object_encoder_bwd_gemm_##SUFFIX(                                          \
      const float *h, const float *q, const float *wk, const float *wv, const float *presence,   \
      const float *gout, float *gh, float *partial, int B, int N, int O, int C,                  \
      const scae_gemm_desc *descs, int n, int nseg, const float *const *seg_ptr,                 \
      const int *seg_width, const int *seg_row_stride, const int64_t *seg_batch_stride,          \
      float *const *seg_grad, const float *trunk_presence, const float *params,                  \
      const float *hsave, float *pg_partial, int trunk_B, int trunk_N, int D, int Din, int Dout, \
      int L, int layer_norm, void *stream) {                                                     \
    return impl_trunk(h, q, wk, wv, presence, gout, gh, partial, B, N, O, C, descs, n, nseg,     \
                      seg_ptr, seg_width, seg_row_stride, seg_batch_stride, seg_grad,            \
                      trunk_presence, params, hsave, pg_partial, trunk_B, trunk_N, D, Din, Dout, \
                      L, layer_norm, BF, stream);                                                \
  }
SCAE_OBJECT_ENCODER_BWD(f32, 0)
SCAE_OBJECT_ENCODER_BWD(bf16, 1)
#undef SCAE_OBJECT_ENCODER_BWD

extern "C" int scae_seed_attention_mfma_bwd_gemm_f32(
    const float *h, const float *q, const float *wk, const float *wv, const float *presence,
    const float *gout, float *gh, float *partial, int B, int N, int O, int C,
    const scae_gemm_desc *descs, int n, void *stream) {
  return impl(h, q, wk, wv, presence, gout, gh, partial, B, N, O, C, descs, n, 0, stream);
}
extern "C" int scae_seed_attention_mfma_bwd_gemm_bf16(
    const float *h, const float *q, const float *wk, const float *wv, const float *presence,
    const float *gout, float *gh, float *partial, int B, int N, int O, int C,
    const scae_gemm_desc *descs, int n, void *stream) {
  return impl(h, q, wk, wv, presence, gout, gh, partial, B, N, O, C, descs, n, 1, stream);
}
