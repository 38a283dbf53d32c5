// A batch drawn from a device-resident dataset (batch_source_dev.h) on its own: one workgroup
// per image of the rank's batch writes the padded, shifted example and its int64 label.  The
// step prologue (step_prologue.hip) does the same in its staging workgroups; this launch is
// for steps without a prologue, an evaluation's remainder batch and the tests.
#include "common.h"
#include "batch_source_dev.h"

namespace {
constexpr int NT = 256;

__global__ __launch_bounds__(NT) void gather_batch_kernel(float *__restrict__ dst_image,
                                                          int64_t *__restrict__ dst_label, int B,
                                                          scae_batch_source_desc s) {
  const int b = blockIdx.x;
  const scae_src::Draw d =
      scae_src::gather_image(s, s.position + (int64_t)s.rank * B + b,
                             dst_image + (size_t)b * s.C * s.H * s.W);
  if (dst_label && threadIdx.x == 0) dst_label[b] = scae_src::label_of(s, d);
}
}  // namespace

extern "C" int scae_gather_batch_f32(float *dst_image, int64_t *dst_label, int B,
                                     const scae_batch_source_desc *src, void *stream) {
  SCAE_REQUIRE(dst_image);
  const int rc = scae_src::check(src, B);
  if (rc) return rc;
  SCAE_REQUIRE(!dst_label || src->labels);
  scae::launch(gather_batch_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, dst_image,
               dst_label, B, *src);
  return scae_launch_status();
}
