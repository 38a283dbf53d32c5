// The exact fp32 row distance and the streamed row tile of the all-pairs analysis kernels
// (knn.hip's search and rank count, cluster_quality.hip's silhouette).
//
// d = sum_f (x_f - b_f)^2 in f order from +0 rounds the difference, the product and the sum each
// to fp32, which is what numpy's float32 does; under HIP's default -ffp-contract=fast the backend
// would fuse the product into the sum.  Every function body here turns contraction off for
// itself, so the rule does not rest on the flags of the file that includes it.  The rounding
// intrinsics are plain operators to the compiler; they mark the places that rely on this.
// (kmeans.hip's dist2_fma is another rule: an fmaf accumulation.)
//
// One row i per lane (its features in registers up to FX, read from memory above); the base
// rows go through LDS in tiles of TILE_FLOATS and are read as a broadcast, four rows a step.
// The streaming loop and the load of the lane's row into xr stay in the three kernels; the
// silhouette also fills its tile itself (a 32-bit row test).
#pragma once
#include "common.h"

namespace scae_rows {
constexpr int TILE_FLOATS = 4096;  // the base tile in LDS (16 KiB)

// a tile's rows are padded with zeros to F4 floats; TB rows a tile: a multiple of four, >= 16
struct TileGeom {
  int F4, TB;
};
__device__ __forceinline__ TileGeom tile_geom(int F) {
#pragma clang fp contract(off)
  const int F4 = (F + 3) & ~3;
  return {F4, (TILE_FLOATS / F4) & ~3};
}

__device__ __forceinline__ float sq_add(float d, float a, float b) {
#pragma clang fp contract(off)
  const float u = __fsub_rn(a, b);
  return __fadd_rn(d, __fmul_rn(u, u));
}

// squared distance of the row (registers xr, FX > 0, zero above F; or global row xp) to the
// base row at b in LDS: rows there are padded with zeros to F4 = 4 * ceil(F / 4) floats (a
// zero pair adds +0 to d: nothing changes), so the register form runs in whole groups of four
template <int FX>
__device__ __forceinline__ float dist2(const float (&xr)[FX > 0 ? FX : 1], const float *xp,
                                       const float *b, int F, int F4) {
#pragma clang fp contract(off)
  float d = 0.f;
  if constexpr (FX > 0) {
#pragma unroll
    for (int f = 0; f < FX; f += 4)
      if (f < F4) {
        const float4 v = *reinterpret_cast<const float4 *>(b + f);
        d = sq_add(d, xr[f], v.x);
        d = sq_add(d, xr[f + 1], v.y);
        d = sq_add(d, xr[f + 2], v.z);
        d = sq_add(d, xr[f + 3], v.w);
      }
  } else {
    for (int f = 0; f < F; ++f) d = sq_add(d, xp[f], b[f]);
  }
  return d;
}

// two rows of global memory, the same arithmetic
__device__ __forceinline__ float dist2_rows(const float *a, const float *b, int F) {
#pragma clang fp contract(off)
  float d = 0.f;
  for (int f = 0; f < F; ++f) d = sq_add(d, a[f], b[f]);
  return d;
}

// base rows [row0, row0 + rows) -> tile (rows, F4), zeros for the padding and past `end`
template <int NT>
__device__ __forceinline__ void load_tile(float *tile, const float *base, int64_t row0,
                                          int64_t end, int rows, int F, int F4) {
#pragma clang fp contract(off)
  for (int e = threadIdx.x; e < rows * F4; e += NT) {
    const int r = e / F4, f = e - r * F4;
    const int64_t j = row0 + r;
    tile[e] = (f < F && j < end) ? base[j * F + f] : 0.f;
  }
}
}  // namespace scae_rows
