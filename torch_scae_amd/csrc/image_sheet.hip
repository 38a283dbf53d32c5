// Image sheets for logging: a batch of (C, H, W) images laid out as one (3, Hs, Ws) grid with
// `padding` pixels of `pad_value` around every image -- what validation_epoch_end
// (base_experiment.py:152-182) hands to add_image.  Up to 4 sources are taken as one batch in
// source order (the reference concatenates its rows of images first); one launch, one thread per
// sheet element, every element written exactly once (a pure copy: nothing to reduce).
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_SOURCES = 4;

struct SheetArgs {
  const float *src[MAX_SOURCES];
  int end[MAX_SOURCES];  // images before the end of source i (cumulative counts)
  int nsrc, N, C, H, W, xmaps, ymaps, padding, Hs, Ws;
  float pad_value;
};

__global__ __launch_bounds__(NT) void image_sheet_kernel(SheetArgs a, float *__restrict__ sheet) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int64_t plane = (int64_t)a.Hs * a.Ws;
  if (i >= 3 * plane) return;
  const int ch = (int)(i / plane);
  const int r = (int)(i - ch * plane), y = r / a.Ws, x = r - y * a.Ws;
  int k, py, px;  // image and the pixel inside it
  if (a.N == 1) {
    k = 0, py = y, px = x;
  } else {
    const int ch_h = a.H + a.padding, ch_w = a.W + a.padding;
    const int cy = y / ch_h, cx = x / ch_w;
    py = y - cy * ch_h - a.padding;
    px = x - cx * ch_w - a.padding;
    k = cy * a.xmaps + cx;
    // the padding lines, the closing line / column of the sheet, cells beyond the last image
    if (py < 0 || px < 0 || cy >= a.ymaps || cx >= a.xmaps || k >= a.N) {
      sheet[i] = a.pad_value;
      return;
    }
  }
  int s = 0, begin = 0;
#pragma unroll
  for (int j = 0; j < MAX_SOURCES - 1; ++j)
    if (j + 1 < a.nsrc && k >= a.end[j]) s = j + 1, begin = a.end[j];
  const int c = a.C == 1 ? 0 : ch;
  sheet[i] = a.src[s][(((size_t)(k - begin) * a.C + c) * a.H + py) * a.W + px];
}

}  // namespace

extern "C" int scae_image_sheet_f32(int nsrc, const float *const *src, const int *n, int C, int H,
                                    int W, int nrow, int padding, float pad_value, float *sheet,
                                    void *stream) {
  SCAE_REQUIRE(nsrc >= 1 && nsrc <= MAX_SOURCES && src && n && sheet);
  SCAE_REQUIRE((C == 1 || C == 3) && H > 0 && W > 0 && nrow > 0 && padding >= 0);
  SheetArgs a = {};
  int64_t N = 0;
  for (int i = 0; i < nsrc; ++i) {
    SCAE_REQUIRE(src[i] && n[i] > 0);
    N += n[i];
    SCAE_REQUIRE(N < (1 << 24));
    a.src[i] = src[i];
    a.end[i] = (int)N;
  }
  a.nsrc = nsrc, a.N = (int)N, a.C = C, a.H = H, a.W = W, a.padding = padding;
  a.pad_value = pad_value;
  a.xmaps = nrow < a.N ? nrow : a.N;
  a.ymaps = (a.N + a.xmaps - 1) / a.xmaps;
  const int64_t Hs = a.N == 1 ? H : (int64_t)a.ymaps * (H + padding) + padding;
  const int64_t Ws = a.N == 1 ? W : (int64_t)a.xmaps * (W + padding) + padding;
  SCAE_REQUIRE(Hs * Ws < ((int64_t)1 << 30));
  a.Hs = (int)Hs, a.Ws = (int)Ws;
  const int64_t total = 3 * Hs * Ws;
  scae::launch(image_sheet_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0,
               (hipStream_t)stream, a, sheet);
  return scae_launch_status();
}
