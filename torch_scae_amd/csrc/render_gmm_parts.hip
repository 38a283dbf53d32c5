// K1, fused E-step: which component of the mixture part_decoder.py:174-237 builds explains each
// pixel -- the per-pixel posterior over the M templates and the background given the observed
// image (or the prior, without one), its arg-max, its per-part sums and a coloured rendering,
// straight from the compact decoder inputs: no (B,K,.,H,W) tensor exists.
//
// Compiled with -ffp-contract=off, as render_gmm_mode_dev.h requires: every component's value
// and mixing logit comes from that header's arithmetic, i.e. has the bits of the materialising
// render (and of render_mode_kernel).  On top of them, per pixel p and channel c
//   j[k,c] = ml[k,cm] - (0.5 (x[c] - loc[k,c])^2) / sigma^2        (ml[k,cm] alone without x)
//   r[k,c] = softmax_k j[.,c]     two passes: max, then sum of exp, in component order
//   R[k]   = (r[k,0] + ... + r[k,C-1]) (1/C)
//   part   = first k with the largest R[k],  conf = R[part],  mass[k] = sum_p R[k,p]
#include "common.h"
#include "render_gmm_dev.h"
#include "render_gmm_mode_dev.h"

namespace {

using namespace scae_k1;

constexpr int NT = kModeThreads;
constexpr int WAVES = NT / 64;

// One walk over the M templates and the background in component order for pixel `pc` of image
// b: f(k, v, ml) gets component k's C values and its logits (ml[0] alone in alpha mode).  The
// planes of `kchunk` templates are staged at a time; `restage` = false: the workgroup's planes
// (all M) are in LDS already.  Every lane of the workgroup takes the same path through here.
template <int C, bool LERP, typename F>
__device__ __forceinline__ void walk_components(const scae_decoder_desc &d, const Scalars &sc,
                                                float *smem, int kchunk, int b, int pc,
                                                bool restage, F &&f) {
  const int tid = threadIdx.x, M = d.M, HW = d.H * d.W, tsz = d.th * d.tw;
  const bool alpha_mode = d.templates_alpha != nullptr;
  const int psz = pad_elems(d.th, d.tw), pw = pad_w(d.tw);
  float *s_tmpl = smem;                                       // kchunk * C planes
  float *s_alpha = s_tmpl + (size_t)kchunk * C * psz;         // kchunk planes (alpha mode)
  float *s_pose = s_alpha + (alpha_mode ? kchunk * psz : 0);  // kchunk * 6
  float *s_lsp = s_pose + kchunk * 6;                         // kchunk
  for (int k0 = 0; k0 < M; k0 += kchunk) {
    const int nk = min(kchunk, M - k0);
    if (restage) {
      __syncthreads();  // every lane is done with the planes staged before
      stage_padded<NT>(s_tmpl, d.templates + ((size_t)tb(d, b) * M + k0) * C * tsz, nk * C,
                       d.th, d.tw);
      if (alpha_mode)
        stage_padded<NT>(s_alpha, d.templates_alpha + (size_t)k0 * tsz, nk, d.th, d.tw);
      for (int i = tid; i < nk * 6; i += NT) s_pose[i] = d.pose[((size_t)b * M + k0) * 6 + i];
      for (int i = tid; i < nk; i += NT)
        s_lsp[i] = d.presence ? mode_log_safe(d.presence[(size_t)b * M + k0 + i]) : 0.f;
      __syncthreads();
    }
    for (int kl = 0; kl < nk; ++kl) {
      PTaps t;
      mode_ptaps<LERP>(s_pose + kl * 6, pc, d.W, d.H, d.tw, d.th, t);
      const float lsp = s_lsp[kl];
      float v[C], ml[C];
      if (alpha_mode) ml[0] = __fadd_rn(mode_sample<LERP, true>(s_alpha + kl * psz, t, pw), lsp);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        v[c] = mode_sample<LERP, false>(s_tmpl + (kl * C + c) * psz, t, pw);
        if (!alpha_mode) ml[c] = __fadd_rn(__fdiv_rn(v[c], sc.temperature), lsp);
      }
      f(k0 + kl, v, ml);
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
    f(M, v, ml);
  }
}

struct PartsOut {
  const float *x;         // (B, C, H, W) or null
  const int *part_group;  // (B, M) or null
  const float *palette;   // (P, 3)
  int P;
  int *part;              // (count, H, W)
  float *conf;            // (count, H, W)
  float *mass_partial;    // (count, tiles, M + 1)
  int *group;             // (count, H, W) or null
  float *rgb_part;        // (count, 3, H, W) or null
  float *rgb_group;       // (count, 3, H, W) or null
};

// One workgroup per (pixel tile, image), one lane per pixel, as render_mode_kernel.  Three walks
// per pixel round: the per-channel maximum of the joint logits, the per-channel sum of
// exponentials, then R[k] with its arg-max and the workgroup's per-component sums.  When the
// templates are chunked each walk restages them (one round per workgroup then).
template <int C, bool LERP>
__global__ __launch_bounds__(NT) void render_parts_kernel(scae_decoder_desc d, PartsOut o,
                                                          int first, int tiles, int ppb,
                                                          int kchunk) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int img = blockIdx.x / tiles, tile = blockIdx.x - img * tiles;
  const int b = first + img, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = d.M, K = M + 1, HW = d.H * d.W;
  const bool alpha_mode = d.templates_alpha != nullptr;
  const Scalars sc = load_scalars(d);
  const float inv_c = 1.f / (float)C;
  const size_t per_k = (size_t)(C + (alpha_mode ? 1 : 0)) * pad_elems(d.th, d.tw) + 7;
  float *s_mass = smem + (size_t)kchunk * per_k;  // WAVES * K: per wave, summed over the rounds
  const bool one_stage = kchunk >= M;
  const int p_begin = tile * ppb, p_end = min(p_begin + ppb, HW);

  for (int i = tid; i < WAVES * K; i += NT) s_mass[i] = 0.f;
  // (the first staging's barriers order these stores before any wave adds to them)

  for (int r0 = p_begin; r0 < p_end; r0 += NT) {  // (one round when the templates are chunked)
    const int p = r0 + tid;
    const bool live = p < p_end;
    const int pc = live ? p : p_begin;
    float xr[C];
#pragma unroll
    for (int c = 0; c < C; ++c) xr[c] = o.x ? o.x[((size_t)b * C + c) * HW + pc] : 0.f;
    // joint logit of one component and channel
    auto joint = [&](const float (&v)[C], const float (&ml)[C], int c) {
      const float l = ml[alpha_mode ? 0 : c];
      if (!o.x) return l;
      const float dx = xr[c] - v[c];
      return l - (0.5f * (dx * dx)) * sc.inv_var;
    };

    float m[C], s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      m[c] = -INFINITY;
      s[c] = 0.f;
    }
    walk_components<C, LERP>(d, sc, smem, kchunk, b, pc, !one_stage || r0 == p_begin,
                             [&](int, const float (&v)[C], const float (&ml)[C]) {
#pragma unroll
                               for (int c = 0; c < C; ++c) m[c] = fmaxf(m[c], joint(v, ml, c));
                             });
    walk_components<C, LERP>(d, sc, smem, kchunk, b, pc, !one_stage,
                             [&](int, const float (&v)[C], const float (&ml)[C]) {
#pragma unroll
                               for (int c = 0; c < C; ++c)
                                 s[c] += mode_expf(joint(v, ml, c) - m[c]);
                             });
    int part = 0;
    float conf = 0.f, tone = 0.f;
    walk_components<C, LERP>(
        d, sc, smem, kchunk, b, pc, !one_stage,
        [&](int k, const float (&v)[C], const float (&ml)[C]) {
          float R = 0.f, t = 0.f;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            R += mode_expf(joint(v, ml, c) - m[c]) / s[c];
            t += v[c];
          }
          R *= inv_c;
          // strict >: the lowest k wins a tie; component 0 when nothing compares greater
          if (k == 0 || R > conf) {
            part = k;
            conf = R;
            tone = t * inv_c;
          }
          // the wave's sum over its pixels, the same butterfly on every run; dead lanes add 0
          float w = live ? R : 0.f;
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) w += __shfl_xor(w, off);
          if (lane == 0) s_mass[wave * K + k] += w;  // (rounds in order)
        });

    if (live) {
      const size_t q = (size_t)img * HW + p;
      o.part[q] = part;
      o.conf[q] = conf;
      const bool bg = part == M;
      int grp = -1;
      if (o.part_group && !bg) grp = o.part_group[(size_t)b * M + part];
      if (o.group) o.group[q] = grp;
      const int pi = part % o.P, gi = ((grp % o.P) + o.P) % o.P;  // (any table entry is in range)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const size_t qc = ((size_t)img * 3 + ch) * HW + p;
        if (o.rgb_part)
          o.rgb_part[qc] = bg ? tone : tone * o.palette[pi * 3 + ch];
        if (o.rgb_group)
          o.rgb_group[qc] = bg ? tone : tone * o.palette[gi * 3 + ch];
      }
    }
  }
  __syncthreads();
  // the waves in index order
  for (int k = tid; k < K; k += NT) {
    float a = s_mass[k];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) a += s_mass[w * K + k];
    o.mass_partial[((size_t)img * tiles + tile) * K + k] = a;
  }
}

// mass[img, k] = the tiles' partials in index order
__global__ void parts_mass_kernel(const float *__restrict__ partial, float *__restrict__ mass,
                                  int tiles, int K) {
  const int img = blockIdx.x;
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    float a = 0.f;
    for (int t = 0; t < tiles; ++t) a += partial[((size_t)img * tiles + t) * K + k];
    mass[(size_t)img * K + k] = a;
  }
}

template <int C>
int launch_render_parts(const scae_decoder_desc *d, const PartsOut &o, float *mass, int first,
                        int count, hipStream_t st) {
  const ModeGeom g = mode_geom(d, count);
  const int K = d->M + 1;
  const size_t lds = g.lds + sizeof(float) * WAVES * K;
  int rc;
#define SCAE_LAUNCH_PARTS(LP)                                                                 \
  rc = set_lds(render_parts_kernel<C, LP>, lds);                                              \
  if (rc) return rc;                                                                          \
  scae::launch((render_parts_kernel<C, LP>), dim3((unsigned)count * g.tiles), dim3(NT), lds,  \
               st, *d, o, first, g.tiles, g.ppb, g.kchunk)
  if (g.lerp) {
    SCAE_LAUNCH_PARTS(true);
  } else {
    SCAE_LAUNCH_PARTS(false);
  }
#undef SCAE_LAUNCH_PARTS
  rc = scae_launch_status();
  if (rc) return rc;
  scae::launch(parts_mass_kernel, dim3((unsigned)count), dim3(64), 0, st,
               (const float *)o.mass_partial, mass, g.tiles, K);
  return scae_launch_status();
}

}  // namespace

extern "C" int scae_render_gmm_parts_geometry(const scae_decoder_desc *d, int count, int *out) {
  int rc = check_decoder_desc(d);
  if (rc) return rc;
  SCAE_REQUIRE(out && count > 0 && count <= d->B);
  const ModeGeom g = mode_geom(d, count);
  out[0] = g.tiles;
  out[1] = g.ppb;
  out[2] = g.kchunk;
  return SCAE_OK;
}

extern "C" int scae_render_gmm_parts_f32(const scae_decoder_desc *d, const float *x,
                                         const int *part_group, const float *palette, int P,
                                         int *part, float *conf, float *mass,
                                         float *mass_partial, int *group, float *rgb_part,
                                         float *rgb_group, int first, int count, void *stream) {
  int rc = check_decoder_desc(d);
  if (rc) return rc;
  SCAE_REQUIRE(part && conf && mass && mass_partial);
  SCAE_REQUIRE(first >= 0 && count > 0 && first <= d->B - count);
  SCAE_REQUIRE(!(rgb_part || rgb_group) || (palette && P > 0));
  SCAE_REQUIRE(!(group || rgb_group) || part_group);
  const PartsOut o{x, part_group, palette, P, part, conf, mass_partial, group, rgb_part,
                   rgb_group};
#define CALL(CC) launch_render_parts<CC>(d, o, mass, first, count, (hipStream_t)stream)
  switch (d->C) {
    case 1: return CALL(1);
    case 2: return CALL(2);
    case 3: return CALL(3);
    case 4: return CALL(4);
    default: return SCAE_ERR_UNSUPPORTED;
  }
#undef CALL
}
