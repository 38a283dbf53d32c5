// Device side of a batch source (include/scae_hip.h, scae_batch_source_desc): slot b of a
// rank's batch is epoch position p = position + rank * B + b; p maps to view row perm_e(p)
// and that to dataset row index[perm_e(p)]; the example is zero-padded to (H, W) and shifted
// by (dy, dx) on the way in -- the reference's MNIST transform (Pad + RandomAffine(translate),
// mnist/experiment.py:23-40), data.pad_and_translate's convention exactly.  Shared by the
// standalone gather (batch_source.hip) and the step prologue (step_prologue.hip), whose
// staging AND image-layer workgroups build their copy of an image through gather_image: the
// two hold the same bits.  data.py mirrors every draw below in integer torch ops.
//
// Epoch order (shuffle = 1): a keyed pseudo-random permutation of [0, n) -- a 4-round Feistel
// network over the smallest even bit width k with 2^k >= n, cycle-walked into [0, n) (fewer
// than 4 walks on average: 2^k < 4n).  Round r's key is a Philox draw of (seed, epoch, r); its
// round function is 3 Philox rounds of the right half under that key.  It is NOT a uniform
// draw over all n! orders.  shuffle = 0: the identity (the reference's DataLoaders).
// wrap = 1: a position p in [n, 2n) -- the padding of a drop_last=False epoch's short last
// step -- takes the row of p - n (both orders) and keeps p for its shift draw.
// Shifts: two 24-bit uniforms r of one Philox draw keyed by seed at counter (p, epoch, tag);
// shift = round half to even of 2*pad*r / 2^24 - pad, in integers (torchvision's
// round(U(-pad, pad))), pad = (H - h) / 2 per axis; translate = 0: no shift.
// affine != NULL: the example is resampled through position p's inverse affine map instead
// (rotation, scale, shear and the shift above: RandomAffine with nearest-neighbour sampling).
// Its six 16.16 fixed-point coefficients are row p of a table the host builds once per epoch
// (include/scae_hip.h has the definition; data.affine_coefficients computes it in fp64); the
// device only reads them and samples in integers, so every copy of an image holds the same
// bits as data.affine_warp's.  With a table the `translate` word is not a switch (the table
// holds the shift) but the sampling mode: 0 / 1 nearest, 2 bilinear -- the four taps around
// the map's point moved half a pixel back, weighted with the 8 fraction bits below the integer
// part (U = k2 + k1 i + k0 j - 32768: x0 = U >> 16, fx = (U >> 8) & 255; likewise V), a tap
// outside the example 0.  uint8 data: the weighted sum of the bytes as an integer (< 2^24),
// one correctly rounded division by 255 * 65536; fp32 data: weights n / 256 (exact), every
// product and sum rounded on its own, no contraction.  At integer coordinates it is the nearest
// form's bits.  Horizontal flips and shift ranges other than the pads (data.py: flip=,
// max_shift=) are composed into the table's rows on the host: nothing here reads them.
#pragma once
#include "common.h"
#include "noise_dev.h"

namespace scae_src {
constexpr uint32_t TAG_PERM = 0x5045524Du, TAG_SHIFT = 0x53484654u;
// (data.py draws the affine parameters on the host at TAG_AFFINE = 0x4146464E)
constexpr int FEISTEL_ROUNDS = 4, F_PHILOX_ROUNDS = 3, KEY_PHILOX_ROUNDS = 10;

// Philox4x32 with the generator's key schedule (noise_dev.h), `rounds` rounds
__device__ __forceinline__ void philox(uint32_t (&c)[4], uint32_t k0, uint32_t k1, int rounds) {
  for (int r = 0; r < rounds; ++r) {
    scae_noise::philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

struct Draw {
  int64_t row;     // dataset row (-1: outside the dataset -- zeros)
  int top, left;   // placement of the example's (0, 0) in the padded image
  int k[6];        // (affine) xin = (k2 + k1 i + k0 j) >> 16, yin = (k5 + k4 i + k3 j) >> 16
};

__device__ __forceinline__ int shift_of(uint32_t r24, int pad) {
  // round half to even of (2 pad r - pad 2^24) / 2^24, exactly
  const int64_t num = 2 * (int64_t)pad * r24;
  const int64_t f = (num >> 24) - pad, rem = num & 0xFFFFFF;
  return (int)(rem > 0x800000 ? f + 1 : rem < 0x800000 ? f : f + (f & 1));
}

// The draw of epoch position p.  Every lane of the calling wave must be active (the round
// keys and the shift are drawn on lanes 0-4 and broadcast).
__device__ __forceinline__ Draw draw(const scae_batch_source_desc &s, int64_t p) {
  const int lane = threadIdx.x & 63;
  const uint32_t e_lo = (uint32_t)s.epoch, e_hi = (uint32_t)((uint64_t)s.epoch >> 32);
  uint32_t c[4] = {(uint32_t)lane, e_lo, e_hi, TAG_PERM};
  if (lane == 4) c[0] = (uint32_t)p, c[3] = TAG_SHIFT;
  scae_src::philox(c, (uint32_t)s.seed, (uint32_t)(s.seed >> 32), KEY_PHILOX_ROUNDS);
  Draw d;
  // (wrap: p mod n for the row, the unwrapped p for the shift above -- check() bounds p < 2n)
  uint32_t x = (uint32_t)(s.wrap && p >= s.n ? p - s.n : p);
  if (s.shuffle && s.n > 1) {
    int k = 0;
    while ((1ll << k) < s.n) k += 2;
    const int h = k / 2;
    const uint32_t m = (1u << h) - 1;
    uint32_t key0[FEISTEL_ROUNDS], key1[FEISTEL_ROUNDS];
#pragma unroll
    for (int r = 0; r < FEISTEL_ROUNDS; ++r)
      key0[r] = (uint32_t)__shfl((int)c[0], r), key1[r] = (uint32_t)__shfl((int)c[1], r);
    do {   // cycle walk: ends at the latest when the cycle returns to p < n
      uint32_t L = x >> h, R = x & m;
#pragma unroll
      for (int r = 0; r < FEISTEL_ROUNDS; ++r) {
        uint32_t f[4] = {R, 0u, 0u, 0u};
        scae_src::philox(f, key0[r], key1[r], F_PHILOX_ROUNDS);
        const uint32_t nl = R;
        R = L ^ (f[0] & m);
        L = nl;
      }
      x = (L << h) | R;
    } while ((int64_t)x >= s.n);
  }
  d.row = s.index ? (int64_t)s.index[x] : (int64_t)x;
  if (d.row < 0 || d.row >= s.rows) d.row = -1;
  const int ph = (s.H - s.h) / 2, pw = (s.W - s.w) / 2;
  const uint32_t ry = (uint32_t)__shfl((int)c[0], 4) >> 8, rx = (uint32_t)__shfl((int)c[1], 4) >> 8;
  d.top = ph + (s.translate ? shift_of(ry, ph) : 0);
  d.left = pw + (s.translate ? shift_of(rx, pw) : 0);
#pragma unroll
  for (int i = 0; i < 6; ++i) d.k[i] = s.affine ? s.affine[p * 6 + i] : 0;   // (p < affine_rows)
  return d;
}

// a * x + b * y with both products and the sum rounded to fp32 (the bilinear form's fp32 rule,
// data.affine_warp's torch ops).  The rounding intrinsics are plain operators to the compiler,
// and under HIP's default -ffp-contract=fast the backend fuses a product into the sum whatever
// a contract pragma says once this is inlined into a kernel (it did: v_pk_fma_f32).  The files
// that include this header must keep their flags -- the prologue's other arithmetic holds its
// bits under them -- so each product passes through an empty asm statement, which emits
// nothing and leaves the backend no product to fuse.
__device__ __forceinline__ float blend(float a, float x, float b, float y) {
  float ax = __fmul_rn(a, x), by = __fmul_rn(b, y);
  asm volatile("" : "+v"(ax));
  asm volatile("" : "+v"(by));
  return __fadd_rn(ax, by);
}

// dst[0 .. C*H*W) = the padded, shifted example of position p (all threads of a 256-thread
// workgroup; no barrier).  Returns the draw.
__device__ __forceinline__ Draw gather_image(const scae_batch_source_desc &s, int64_t p,
                                             float *dst) {
  const Draw d = draw(s, p);
  const int HW = s.H * s.W, count = s.C * HW, hw = s.h * s.w;
  const uint8_t *img8 = static_cast<const uint8_t *>(s.images);
  const float *imgf = static_cast<const float *>(s.images);
  const size_t base = d.row < 0 ? 0 : (size_t)d.row * s.C * hw;
  if (s.affine && s.translate == 2) {   // bilinear: 8-bit weights of the same fixed-point map
    const int ph = (s.H - s.h) / 2, pw = (s.W - s.w) / 2;
    for (int e = threadIdx.x; e < count; e += 256) {
      const int ch = e / HW, rr = e - ch * HW, i = rr / s.W, j = rr - i * s.W;
      const int64_t U = d.k[2] + (int64_t)d.k[1] * i + (int64_t)d.k[0] * j - 32768;
      const int64_t V = d.k[5] + (int64_t)d.k[4] * i + (int64_t)d.k[3] * j - 32768;
      const int64_t x0 = (U >> 16) - pw, y0 = (V >> 16) - ph;
      const int fx = (int)((U >> 8) & 255), fy = (int)((V >> 8) & 255);
      // the four taps' validity; a tap outside the example (or the dataset) is 0
      const bool r0 = d.row >= 0 && y0 >= 0 && y0 < s.h, r1 = d.row >= 0 && y0 >= -1 && y0 < s.h - 1;
      const bool c0 = x0 >= 0 && x0 < s.w, c1 = x0 >= -1 && x0 < s.w - 1;
      // (clamped so that every formed offset lies inside the example; read only where valid)
      const size_t ya = (size_t)(y0 < 0 ? 0 : y0 >= s.h ? s.h - 1 : y0);
      const size_t yb = (size_t)(y0 + 1 < 0 ? 0 : y0 + 1 >= s.h ? s.h - 1 : y0 + 1);
      const size_t xa = (size_t)(x0 < 0 ? 0 : x0 >= s.w ? s.w - 1 : x0);
      const size_t xb = (size_t)(x0 + 1 < 0 ? 0 : x0 + 1 >= s.w ? s.w - 1 : x0 + 1);
      const size_t plane = base + (size_t)ch * hw;
      const size_t o00 = plane + ya * s.w + xa, o01 = plane + ya * s.w + xb;
      const size_t o10 = plane + yb * s.w + xa, o11 = plane + yb * s.w + xb;
      float v;
      if (s.image_u8) {   // acc <= 255 * 65536 < 2^24: exact in fp32; one rounding, the division
        const int t00 = r0 && c0 ? img8[o00] : 0, t01 = r0 && c1 ? img8[o01] : 0;
        const int t10 = r1 && c0 ? img8[o10] : 0, t11 = r1 && c1 ? img8[o11] : 0;
        const int acc = (256 - fy) * ((256 - fx) * t00 + fx * t01) +
                        fy * ((256 - fx) * t10 + fx * t11);
        v = __fdiv_rn((float)acc, 16711680.0f);   // 255 * 65536
      } else {            // exact weights, every product and sum rounded on its own
        const float t00 = r0 && c0 ? imgf[o00] : 0.f, t01 = r0 && c1 ? imgf[o01] : 0.f;
        const float t10 = r1 && c0 ? imgf[o10] : 0.f, t11 = r1 && c1 ? imgf[o11] : 0.f;
        const float wx1 = (float)fx * 0.00390625f, wx0 = (float)(256 - fx) * 0.00390625f;
        const float wy1 = (float)fy * 0.00390625f, wy0 = (float)(256 - fy) * 0.00390625f;
        v = blend(wy0, blend(wx0, t00, wx1, t01), wy1, blend(wx0, t10, wx1, t11));
      }
      dst[e] = v;
    }
    return d;
  }
  if (s.affine) {   // nearest-neighbour through the inverse map, in integers
    const int ph = (s.H - s.h) / 2, pw = (s.W - s.w) / 2;
    for (int e = threadIdx.x; e < count; e += 256) {
      const int ch = e / HW, rr = e - ch * HW, i = rr / s.W, j = rr - i * s.W;
      const int64_t sj = ((d.k[2] + (int64_t)d.k[1] * i + (int64_t)d.k[0] * j) >> 16) - pw;
      const int64_t si = ((d.k[5] + (int64_t)d.k[4] * i + (int64_t)d.k[3] * j) >> 16) - ph;
      float v = 0.f;
      if (d.row >= 0 && si >= 0 && si < s.h && sj >= 0 && sj < s.w) {
        const size_t off = base + (size_t)ch * hw + (size_t)si * s.w + (size_t)sj;
        v = s.image_u8 ? __fdiv_rn((float)img8[off], 255.0f) : imgf[off];   // ToTensor
      }
      dst[e] = v;
    }
    return d;
  }
  for (int e = threadIdx.x; e < count; e += 256) {
    const int ch = e / HW, rr = e - ch * HW, i = rr / s.W, j = rr - i * s.W;
    const int si = i - d.top, sj = j - d.left;
    float v = 0.f;
    if (d.row >= 0 && si >= 0 && si < s.h && sj >= 0 && sj < s.w) {
      const size_t off = base + (size_t)ch * hw + si * s.w + sj;
      v = s.image_u8 ? __fdiv_rn((float)img8[off], 255.0f) : imgf[off];   // ToTensor
    }
    dst[e] = v;
  }
  return d;
}

__device__ __forceinline__ int64_t label_of(const scae_batch_source_desc &s, const Draw &d) {
  if (d.row < 0) return 0;
  return s.label_u8 ? (int64_t) static_cast<const uint8_t *>(s.labels)[d.row]
                    : static_cast<const int64_t *>(s.labels)[d.row];
}

// host: the checks both entry points make before any HIP call (B: the rank's batch)
inline int check(const scae_batch_source_desc *s, int B) {
  SCAE_REQUIRE(s && s->images && B > 0);
  const scae_batch_source_desc &a = *s;
  SCAE_REQUIRE(a.n > 0 && a.n < (1ll << 31) && a.rows > 0 && (a.index || a.n <= a.rows));
  SCAE_REQUIRE(a.C > 0 && a.h > 0 && a.w > 0 && a.h <= a.H && a.w <= a.W);
  SCAE_REQUIRE(a.world > 0 && a.rank >= 0 && a.rank < a.world && a.epoch >= 0 &&
               a.position >= 0);
  SCAE_REQUIRE(a.wrap == 0 || a.wrap == 1);
  SCAE_REQUIRE(a.position + (int64_t)(a.rank + 1) * B <= (a.wrap ? 2 * a.n : a.n));
  SCAE_REQUIRE((a.image_u8 == 0 || a.image_u8 == 1) && (a.label_u8 == 0 || a.label_u8 == 1));
  SCAE_REQUIRE(a.affine ? a.position + (int64_t)(a.rank + 1) * B <= a.affine_rows
                        : a.affine_rows == 0);
  // (with a table `translate` is the sampling mode: 0 / 1 nearest, 2 bilinear)
  SCAE_REQUIRE(a.translate >= 0 && a.translate <= (a.affine ? 2 : 1));
  if (a.C > 4) return SCAE_ERR_UNSUPPORTED;
  return 0;
}
}  // namespace scae_src
