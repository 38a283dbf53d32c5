// K1, fused mode / mean: distributions.py:37-39 / :50-77 of the mixture part_decoder.py:174-237
// builds, straight from the compact decoder inputs -- the reconstruction image without the two
// (B,K,.,H,W) tensors of the materialising path (render_gmm.hip / render_gmm_wave.hip, then
// gmm_mean_mode_kernel), and with its bits.
//
// Compiled with -ffp-contract=off, as render_gmm_mode_dev.h requires of every file that includes
// it: that header holds the component arithmetic (mode_ptaps, mode_sample, mode_expf,
// mode_log_safe) and the launch geometry this file shares with render_gmm_parts.hip.
#include "common.h"
#include "render_gmm_dev.h"
#include "render_gmm_mode_dev.h"

namespace {

using namespace scae_k1;

constexpr int NT = kModeThreads;

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
template <int C>
int launch_render_mode(const scae_decoder_desc *d, float *out, int mean, int first, int count,
                       hipStream_t st) {
  const ModeGeom g = mode_geom(d, count);
  const size_t lds = g.lds;
  const int tiles = g.tiles, ppb = g.ppb, kchunk = g.kchunk;
  int rc;
#define SCAE_LAUNCH_MODE(LP)                                                                \
  rc = set_lds(render_mode_kernel<C, LP>, lds);                                             \
  if (rc) return rc;                                                                        \
  scae::launch((render_mode_kernel<C, LP>), dim3((unsigned)count * tiles), dim3(NT), lds, st, \
               *d, out, mean, first, tiles, ppb, kchunk)
  if (g.lerp) {
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
