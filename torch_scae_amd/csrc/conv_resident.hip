// K8r -- the forward of a small 3x3 "valid" convolution layer (part_encoder.py:26-44,
// nn_ext.py:34-59: Conv2d(k=3, stride s, padding 0) + ReLU) with the INPUT IMAGES RESIDENT in
// LDS, for layers whose whole problem is a few microseconds of matrix time (the encoder's
// 9x9 -> 7x7 and 7x7 -> 5x5 layers at B = 128: 1.85 / 0.94 GFLOP on 256 CUs).
//
// What bounds the ring-pipelined tiles of conv_mfma.hip there (phase stamps, tools/fwd_prof.py)
// is not the matrix pipe: every K chunk costs a workgroup barrier and three LDS-DMA
// instructions per wave, each of which holds the wave's issue for 60-180 cycles that no MFMA
// covers, and 200 / 392 tiles on 256 CUs leave a quarter of the chip idle.  Here
//   * a workgroup owns a GROUP OF IMAGES x 32 NJ output channels (NJ = 2 column tiles where the
//     plan allows, else 1): the images' input pixels (G x IH x IW x Cin elements as three bf16
//     planes, 37-61 KB) are staged ONCE for all of them; the nine taps of the implicit GEMM are
//     nine offsets into that LDS image -- no operand of A is ever re-fetched, and none is split
//     more than once;
//   * the weights come straight from global memory into MFMA fragments: the filter is kept
//     in a FRAGMENT-MAJOR copy (scae_conv3x3_relayout*: the second half of the `wf` buffer),
//     where the 64 lanes x 16 bytes of one fragment quad are 1 KiB contiguous -- one fully
//     coalesced `global_load_dwordx4`, no LDS, a chunk ahead of its use;
//   * the four waves of a column tile split K by input-channel block and never meet inside the
//     main loop: no barrier, no DMA, no counted waits -- ds_read_b128 +
//     v_mfma_f32_32x32x16_bf16 only; they sum their accumulators through LDS once at the end
//     (fixed order: deterministic, and the same order for NJ = 1 and 2: the same bits);
//   * the grid is B / G x Cout / (32 NJ) workgroups of 4 NJ waves: 256 of eight waves for either
//     layer at B = 128, one per CU, equal work each.
// The image's layout and the swizzle that keeps the row-per-lane fragment reads free of bank
// conflicts are described at the kernel.
#include "bf16x6.h"
#include "mfma_pipe.h"
#include "conv_first_dev.h"

namespace {
namespace pipe = scae_pipe;
using scae_first::ConvGeom;
constexpr int NT = 256;

struct ResArgs {
  const float *in, *wp, *bias, *post_bias;
  float *out, *out_post;
  ConvGeom g;
  int G;   // images per workgroup
};

// The products run on the bf16 matrix cores as six exact partial products of a three-way split
// of the fp32 operands (bf16x6.h): fp32 results at 6 / 16 of the fp32 MFMA time.  Both operands
// arrive at the main loop already split: the filter's fragment-major copy holds its three bf16
// planes, and the staging cuts every pixel into its planes ONCE -- not once per tap and column
// tile on the fragments -- so the loop is ds_read_b128 + MFMA only.
//
// The LDS image: a pixel is Cin / 8 UNITS of 8 channels; a unit is 48 bytes, its hi, mid and lo
// bf16x8 side by side (the three fragment reads share one address and differ by an immediate
// offset).  Unit s of pixel p sits in place s ^ (key(p) & 15) of the pixel's row, where
//     key(p) = n * OH * OW + (ih / stride) * OW + iw / stride        (p = (n, ih, iw)):
// lane `li` of a fragment read, at any tap, holds the key  r + const  of its output row r, so the
// 16 lanes that share an LDS cycle of a ds_read_b128 (MI355X: {0-3, 12-15, 20-27}, {4-11, 16-19,
// 28-31} and the same + 32) hold 16 different keys mod 16.  A row is a multiple of 16 x 48 bytes
// and 3 is odd, so 16 different places are 16 different 16-byte bank columns: no conflicts at any
// stride or group (the fp32 image's  slot ^ (p & 15)  collided 2-way wherever two rows of the
// lane group were 16 input pixels apart).  The staging stores of 8 consecutive lanes are the 8
// units of an aligned block, permuted: 8 different columns of the 32 store banks as well.
constexpr int SU = 6;          // units a thread loads before it splits the first
constexpr int UNIT_BYTES = 48;

// p / d for 0 <= p < 2^20: (p + 0.5) / d is at least 0.5 / d away from an integer, the product's
// error is below p / d * 2^-22
__device__ __forceinline__ int small_div(int p, float rd) { return (int)(((float)p + 0.5f) * rd); }

template <int MI, int NJ>
__global__ __launch_bounds__(NT * NJ, 2 / NJ) void conv_res_fwd_kernel(ResArgs a) {
  constexpr int NTH = NT * NJ;
  extern __shared__ __attribute__((aligned(1024))) float smem[];
  char *const simg = reinterpret_cast<char *>(smem);
  const int tid = threadIdx.x, wid = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63,
            li = lane & 31, lk = lane >> 5;
  const ConvGeom &g = a.g;
  // wave `wid` is K part `kp` of the workgroup's column tile `nj`
  const int kp = wid & 3, nj = wid >> 2;
  const int ntiles = g.Cout / (32 * NJ);
  const int nt = (blockIdx.x % ntiles) * NJ + nj, img0 = (blockIdx.x / ntiles) * a.G;
  const int nimg = min(a.G, g.B - img0);
  const int ipix = g.IH * g.IW, opix = g.OH * g.OW;
  const int UP = g.Cin / 8;             // units per pixel (a multiple of 16)
  const int rowb = UP * UNIT_BYTES;     // bytes of a pixel's row of units
  const int sh = g.stride - 1;          // stride 1 or 2
  const int CB = g.Cin / 32;         // 32-channel blocks per tap
  const int CPT = CB / 4;            // ... per wave
  const int NCW = 9 * CPT;           // this wave's chunks
  // (per 32-channel chunk: 2 pairs of quads x 3 planes x 64 lanes x 16 bytes)
  const uint4 *wq = reinterpret_cast<const uint4 *>(a.wp) + (size_t)nt * (9 * CB) * 384 + lane;
  uint4 bq[2][2][3];   // [buffer][pair][plane]
  auto load_b = [&](int c, int buf) {
    const int tap = c / CPT, cb = kp + 4 * (c - tap * CPT);
    const uint4 *src = wq + (size_t)(tap * CB + cb) * 384;
#pragma unroll
    for (int qp = 0; qp < 2; ++qp)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) bq[buf][qp][pl] = src[(qp * 3 + pl) * 64];
  };
  load_b(0, 0);   // (in flight under the staging)
  // ---- 1. the group's input pixels -> LDS, split into their planes --------------------------
  {
    const pipe::rsrc_t rin =
        pipe::make_rsrc(a.in, (unsigned)((size_t)g.B * ipix * g.Cin * 4));
    const int units = a.G * ipix * UP, valid = nimg * ipix;
    const float ripix = 1.f / (float)ipix, riw = 1.f / (float)g.IW;
    // unit u = tid + k * NTH is unit s of pixel p: stepped, not divided
    const int dp = NTH / UP, ds = NTH - dp * UP;
    int p = tid / UP, s = tid - p * UP;
    for (int ub = 0; ub < units; ub += SU * NTH) {   // (ub: wave-uniform)
      const int u0 = ub + tid;
      scae_x6::u32x4 v[SU][2];
      int dst[SU];
      // pixels past the group's images (a ragged last group) read an offset no descriptor
      // covers: zeros, and nothing past the B images is touched
#pragma unroll
      for (int k = 0; k < SU; ++k) {
        if (ub + k * NTH >= units) break;   // rounds no thread has a unit in
        const bool in = u0 + k * NTH < units;
        const int vo = in && p < valid ? ((img0 * ipix + p) * g.Cin + s * 8) * 4 : pipe::DMA_ZERO;
        v[k][0] = __builtin_amdgcn_raw_buffer_load_b128(rin, vo, 0, 0);
        v[k][1] = __builtin_amdgcn_raw_buffer_load_b128(rin, vo, 16, 0);
        const int n = small_div(p, ripix), rem = p - n * ipix;
        const int ih = small_div(rem, riw), iw = rem - ih * g.IW;
        const int key = n * opix + (ih >> sh) * g.OW + (iw >> sh);
        // (a last pass's idle lanes store to the spare unit behind the image: no branch)
        dst[k] = in ? p * rowb + (s ^ (key & 15)) * UNIT_BYTES : units * UNIT_BYTES;
        s += ds, p += dp;
        if (s >= UP) s -= UP, ++p;
      }
#pragma unroll
      for (int k = 0; k < SU; ++k) {
        if (ub + k * NTH >= units) break;
        const scae_x6::Split3 sp = scae_x6::split3(__builtin_bit_cast(float4, v[k][0]),
                                                   __builtin_bit_cast(float4, v[k][1]));
        uint4 *d = reinterpret_cast<uint4 *>(simg + dst[k]);
        d[0] = __builtin_bit_cast(uint4, sp.hi);
        d[1] = __builtin_bit_cast(uint4, sp.mid);
        d[2] = __builtin_bit_cast(uint4, sp.lo);
      }
    }
  }
  // ---- this lane's rows: output pixel r of the group -> its window's first input pixel -----
  const int rows = nimg * opix;
  int pbase[MI], kbase[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int r = min(mi * 32 + li, rows - 1);
    const int n = r / opix, rem = r - n * opix, oh = rem / g.OW, ow = rem - oh * g.OW;
    pbase[mi] = n * ipix + oh * g.stride * g.IW + ow * g.stride;
    kbase[mi] = r;   // key of that pixel
  }
  // ---- 2. main loop: the wave contracts the channel blocks kp, kp + 4, .. of every tap -------
  // NS small-product accumulators per tile -- with one tile per wave three, so that two MFMAs
  // on the same accumulator are three instructions apart (a dependent MFMA waits ~64 cycles);
  // with more tiles the tiles themselves interleave
  constexpr int NS = MI == 1 ? 3 : 1;
  pipe::f32x16 acc[MI], accl[MI][NS];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      acc[mi][e] = 0.f;
#pragma unroll
      for (int n = 0; n < NS; ++n) accl[mi][n][e] = 0.f;
    }
  __syncthreads();   // the image is whole
  auto chunk = [&](int c, int buf) {
    if (c + 1 < NCW) load_b(c + 1, buf ^ 1);
    const int tap = c / CPT, cb = kp + 4 * (c - tap * CPT);
    const int kh = tap / 3, kw = tap - 3 * kh;
    const int unit0 = cb * 4 + lk * 2;
    const char *ap[MI];
    int sw[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      ap[mi] = simg + (pbase[mi] + kh * g.IW + kw) * rowb;
      sw[mi] = (kbase[mi] + (kh >> sh) * g.OW + (kw >> sh)) & 15;
    }
    // two units = the lane's eight k of each of two bf16 MFMAs (the same eight for A and B)
#pragma unroll
    for (int qp = 0; qp < 2; ++qp) {
      scae_x6::Split3 bs;
      bs.hi = __builtin_bit_cast(scae_x6::bf16x8, bq[buf][qp][0]);
      bs.mid = __builtin_bit_cast(scae_x6::bf16x8, bq[buf][qp][1]);
      bs.lo = __builtin_bit_cast(scae_x6::bf16x8, bq[buf][qp][2]);
      scae_x6::Split3 as[MI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        const uint4 *src =
            reinterpret_cast<const uint4 *>(ap[mi] + ((unit0 + qp) ^ sw[mi]) * UNIT_BYTES);
        as[mi].hi = __builtin_bit_cast(scae_x6::bf16x8, src[0]);
        as[mi].mid = __builtin_bit_cast(scae_x6::bf16x8, src[1]);
        as[mi].lo = __builtin_bit_cast(scae_x6::bf16x8, src[2]);
      }
      // the six products, product by product over the tiles: consecutive MFMAs write
      // different accumulators (smallest products first within an accumulator)
#define SCAE_X6_STEP(AP, BP, N)                                                                   \
  _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) accl[mi][(N) % NS] =                          \
      __builtin_amdgcn_mfma_f32_32x32x16_bf16(as[mi].AP, bs.BP, accl[mi][(N) % NS], 0, 0, 0);
      SCAE_X6_STEP(hi, lo, 0)
      SCAE_X6_STEP(lo, hi, 1)
      SCAE_X6_STEP(mid, mid, 2)
      SCAE_X6_STEP(hi, mid, 0)
      SCAE_X6_STEP(mid, hi, 1)
#undef SCAE_X6_STEP
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as[mi].hi, bs.hi, acc[mi], 0, 0, 0);
    }
  };
  for (int c = 0; c < NCW; c += 2) {
    chunk(c, 0);
    if (c + 1 < NCW) chunk(c + 1, 1);
  }
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    pipe::f32x16 small = accl[mi][0];
#pragma unroll
    for (int n = 1; n < NS; ++n) small += accl[mi][n];
    acc[mi] += small;
  }
  // ---- 3. a tile's four K parts meet in LDS (the staged pixels are dead), fixed order -------
  __syncthreads();
  // slab [wave][mi][reg][lane]
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int e = 0; e < 16; ++e) smem[((wid * MI + mi) * 16 + e) * 64 + lane] = acc[mi][e];
  const int col = nt * 32 + li;
  const float bn = a.bias[col];
  float pb[MI][4];
  // the wave finishes registers 4 kp .. 4 kp + 3 of its column tile: these rows of a tile
  const int row0 = 8 * kp + 4 * lk;
  if (a.out_post) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = min(mi * 32 + row0 + e, rows - 1);
        pb[mi][e] = a.post_bias[(size_t)col * opix + r % opix];
      }
  }
  __syncthreads();
  const unsigned obytes = (unsigned)((size_t)g.B * opix * g.Cout * 4);
  const pipe::rsrc_t ro = pipe::make_rsrc(a.out, obytes);
  const pipe::rsrc_t rp = pipe::make_rsrc(a.out_post ? a.out_post : a.out, obytes);
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        v += smem[(((nj * 4 + w) * MI + mi) * 16 + 4 * kp + e) * 64 + lane];
      const int r = mi * 32 + row0 + e;
      const float o = fmaxf(v + bn, 0.f);
      // rows past the group's last output pixel: an offset no descriptor covers (dropped)
      const int off = r < rows ? ((img0 * opix + r) * g.Cout + col) * 4 : pipe::DMA_ZERO;
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, o), ro, off, 0, 0);
      if (a.out_post)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, o + pb[mi][e]), rp, off, 0, 0);
    }
}

struct ResPlan {
  int G, MI, NJ;
  size_t lds;
};
// images per workgroup: the best row use of the 32-row MFMA tiles among the groups that fit
// (<= 4 tiles, LDS for two workgroups per CU); ties go to the smaller group (more workgroups).
// Column tiles per workgroup: two (eight waves on one staged image: measured faster than two
// workgroups of four at both of the encoder's shapes) where Cout allows
// and the meeting slabs of 2 x 4 waves stay within the image's LDS class (<= 2 row tiles)
bool res_plan(const ConvGeom &g, ResPlan &p, int force_g) {
  if (g.stride < 1 || g.stride > 2 || g.Cin % 128 || g.Cout % 32) return false;
  const int opix = g.OH * g.OW, ipix = g.IH * g.IW;
  double best = 0.;
  p.G = 0;
  for (int G = 1; G <= 8 && G <= g.B; ++G) {
    if (force_g > 0 && G != force_g) continue;
    const int MI = (G * opix + 31) / 32;
    // (three bf16 planes: 6 bytes per element, and the spare unit the staging's idle lanes hit)
    const size_t stage = ((size_t)G * ipix * (g.Cin / 8) + 1) * UNIT_BYTES;
    const int NJ = g.Cout % 64 == 0 && MI <= 2 ? 2 : 1;
    const size_t lds = std::max(stage, (size_t)4 * NJ * MI * 16 * 64 * 4);
    // two workgroups per CU can stay resident: half of the CU's 160 KiB each
    if (MI > 4 || lds > (force_g > 0 ? 150 : 80) * 1024) break;
    const double use = (double)G * opix / (32. * MI);
    if (use > best + 1e-9) best = use, p.G = G, p.MI = MI, p.NJ = NJ, p.lds = lds;
  }
  return p.G > 0;
}
}  // namespace

extern "C" int scae_conv3x3_fwd_res_supported(int B, int IH, int IW, int Cin, int Cout, int stride) {
  if (B <= 0 || IH < 3 || IW < 3 || Cin <= 0 || Cout <= 0 || stride <= 0) return 0;
  ConvGeom g{B, IH, IW, (IH - 3) / stride + 1, (IW - 3) / stride + 1, Cin, Cout, stride};
  ResPlan p;
  return res_plan(g, p, 0) ? 1 : 0;
}

// `group`: images per workgroup (0: chosen by shape -- the production setting; > 0: forced,
// tests and measurements)
extern "C" int scae_conv3x3_fwd_res_f32(const float *in, const float *wp, const float *bias,
                                        float *out, const float *post_bias, float *out_post, int B,
                                        int IH, int IW, int Cin, int Cout, int stride, int group,
                                        void *stream) {
  SCAE_REQUIRE(in && wp && bias && out && (!out_post || post_bias) && B > 0 && IH >= 3 && IW >= 3 &&
               Cin > 0 && Cout > 0 && stride > 0 && group >= 0);
  ConvGeom g{B, IH, IW, (IH - 3) / stride + 1, (IW - 3) / stride + 1, Cin, Cout, stride};
  ResPlan p;
  if (!res_plan(g, p, group)) return SCAE_ERR_UNSUPPORTED;
  ResArgs a{in, wp, bias, post_bias, out, out_post, g, p.G};
  const dim3 grid((Cout / (32 * p.NJ)) * ((B + p.G - 1) / p.G));
  hipStream_t st = (hipStream_t)stream;
#define SCAE_RES(M, J)                                                                           \
  case M * 2 + J - 1: {                                                                          \
    if (p.lds > 48 * 1024) {                                                                     \
      hipError_t e =                                                                             \
          hipFuncSetAttribute(reinterpret_cast<const void *>(conv_res_fwd_kernel<M, J>),         \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);           \
      if (e != hipSuccess) return (int)e;                                                        \
    }                                                                                            \
    scae::launch(conv_res_fwd_kernel<M, J>, grid, dim3(NT * J), p.lds, st, a);                   \
    break;                                                                                       \
  }
  switch (p.MI * 2 + p.NJ - 1) {
    SCAE_RES(1, 1) SCAE_RES(2, 1) SCAE_RES(3, 1) SCAE_RES(4, 1) SCAE_RES(1, 2) SCAE_RES(2, 2)
    default: return SCAE_ERR_UNSUPPORTED;
  }
#undef SCAE_RES
  return scae_launch_status();
}
