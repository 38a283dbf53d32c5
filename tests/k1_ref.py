"""fp64 reference of the part decoder (K1: csrc/render_gmm.hip, render_gmm_wave.hip,
render_gmm_wave_dev.h, render_gmm_mode.hip) that also says how far an fp32 evaluation may be
from it.  CPU only; no GPU import.  The role tests/lk_ref.py plays for K4.

``forward`` restates ``oracle.bilinear_warp``, ``image_decoder``, ``gmm_log_prob``, ``gmm_mean``
and ``gmm_mode`` in explicit fp64 formulas on the fp32 inputs as given (no ``grid_sample``);
``log_safe`` and its gradient decide their floor on the fp32 value, as the kernels do.
``backward`` is the hand-written fp64 backward of every gradient the ABI returns --
g_templates, g_alpha_partial and g_scalar_partial per (image, component), g_pose,
g_presence, g_bg_image -- for a per-pixel ``g_logprob`` (a per-tile gradient is spread over
its pixels by ``spread_tiles``) or for the unfused pair ``g_tt`` / ``g_ml``.
``autograd_backward`` is the same through fp64 autograd of ``forward``'s formulas;
tests/test_k1_ref.py holds one against the other and both against the oracle run in fp64.

Every float entry comes with a companion magnitude: the sum of the absolute values of the
terms that are added to make it, with the companion of each factor carried along by the
chain rule --

    sample position   ix = ((a0 xn + a1 yn + a2 + 1) tw - 1) / 2:
                      m_ix = ((|a0 xn| + |a1 yn| + |a2| + 1) tw + 1) / 2
    bilinear sample   v = sum_taps t w:   m_v = sum |t| w + |dv/dix| m_ix + |dv/diy| m_iy
    log-sum-exp       |max| + |log sum| + sum_k p_k m_k                    (as lk_ref._lse)
    exp(a - lse)      value (1 + m_a + m_lse) + FLOOR
    texel gradient    sum_pixels m_g w + |g| (wy m_ix + wx m_iy)
      cell-gather     + sum_pixels |g| {1 + fx + fy + fx fy, fx + fx fy, fy + fx fy, fx fy} for
                      the cell's four corners: that form (render_gmm_wave_dev.h) adds a cell's
                      moment sums S = sum g {1, fx, fy, fx fy} and forms the corners as
                      S0 - S1 - S2 + S3, S1 - S3, S2 - S3, S3 -- these are the terms its
                      arithmetic really adds, whatever the bilinear weight they combine to
                      (``backward(..., moments=True)``)
    pose gradient     sum_pixels (m_g |dv/dix| + |g| m_(dv/dix)) |xn| tw / 2
    a scalar's        sum over the pixels of the component, the same way

and the bound of an entry is c 2^-24 magnitude.  Nothing is masked out of a comparison: d/d pose
jumps where a sample position crosses a texel-cell boundary, so every case is cleared of them
in fp64 (``clear_of_cell_boundaries``, margin 8e-6) and ``checked_case`` asserts that.

Measured (tests/test_k1_ref.py::test_constants_come_from_the_fp32_oracle re-measures and
prints them): the fp32 oracle on the CPU (ATen's affine_grid / grid_sample, autograd) against
this reference, worst |fp32 - fp64| / (2^-24 magnitude) over every case of ``all_cases()``:

    outputs    tt 2.50  ml 2.28  log_prob 0.89  tile_sums 0.56  mean 1.03
    gradients  templates 1.42  alpha 1.21  pose 0.16  presence 0.37  bg_image 0.88
               scalars 0.20
    (gradients: per-pixel g_logprob, g_tt alone, g_ml alone, both; lse_post and lse_prior
    are not oracle outputs -- they are the two terms of log_prob and share its constant)

Each kind has its own constant, 4 x its measured ratio rounded up to one digit (C_OUT[kind],
C_GRAD[kind] below).  Cases of B M >= 3000 are measured on log_prob and its tile sums only, and
the "init" pose regime is a stand-in on the CPU (``make_case``).  The factor 4 is for what
the kernels do differently from ATen: wave shuffles, segmented runs and row slices instead of
serial sums, fmaf lerps, and the hardware exp / log / rcp.  c is never tuned against a kernel.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
# worst ratio of the fp32 oracle against this reference, per kind (test_k1_ref.py prints them)
MEASURED_OUT = dict(tt=2.50, ml=2.28, log_prob=0.89, tile_sums=0.56, mean=1.03)
MEASURED_GRAD = dict(templates=1.42, alpha=1.21, pose=0.16, presence=0.37, bg_image=0.88,
                     scalars=0.20)


def _four_times(v):
    """4 x the measured ratio, rounded up to one significant digit"""
    x = 4.0 * v
    e = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / e - 1e-9) * e


# one constant per kind of output and of gradient.  lse_post and lse_prior are not oracle outputs:
# they are the two terms of log_prob and take its constant; the alpha and scalar partials take
# the constants of their sums
C_OUT = {k: _four_times(v) for k, v in MEASURED_OUT.items()}
C_OUT["lse_post"] = C_OUT["lse_prior"] = C_OUT["log_prob"]
C_GRAD = {k: _four_times(v) for k, v in MEASURED_GRAD.items()}
C_GRAD["alpha_partial"], C_GRAD["scalar_partial"] = C_GRAD["alpha"], C_GRAD["scalars"]
HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)
EPS32 = float(np.float32(1e-16))
FLOOR = 2.0 ** -102   # times 2^-24: the smallest normal fp32 -- what an underflow may lose
CHUNK_ELEMS = 300000  # (image, component, channel, pixel) entries per pass over the batch


def _d(t):
    return None if t is None else t.detach().double()


def _softplus(v):
    return torch.where(v > 20, v, torch.log1p(torch.exp(torch.clamp(v, max=20.0))))


def _scalars(ins, leaves=None):
    """sigma, temperature, bg value, bg mixing logit with companions and the derivative of
    each with respect to its parameter.  ``leaves``: (b, K) fp64 leaves that stand for the
    parameters per (image, component) -- autograd then returns the per-component partials."""
    z = torch.zeros((), dtype=torch.float64)
    val = {k: (_d(ins[k]).reshape(()) if ins.get(k) is not None else None)
           for k in ("bg_value", "bg_mixing_logit", "temperature_logit", "scale")}
    raw = val if leaves is None else {k: (leaves[k] if val[k] is not None else None) for k in val}
    alpha_mode = ins.get("alpha") is not None
    s = {}
    if val["scale"] is not None:
        s["sigma"] = _softplus(raw["scale"]) + 1e-4
        s["m_sigma"] = (_softplus(val["scale"]) + 1e-4) * (2 + val["scale"].abs())
        s["d_sigma"] = torch.sigmoid(val["scale"])
    else:
        s["sigma"], s["m_sigma"], s["d_sigma"] = z + 1.0, z, z
    if alpha_mode:
        s["T"], s["m_T"], s["d_T"] = z + 1.0, z, z
        s["bg_ml"] = _softplus(raw["bg_mixing_logit"])
        s["m_bg_ml"] = _softplus(val["bg_mixing_logit"]) * (2 + val["bg_mixing_logit"].abs())
        s["d_bg_ml"] = torch.sigmoid(val["bg_mixing_logit"])
    else:
        tl = val["temperature_logit"] + 0.5
        s["T"] = _softplus(raw["temperature_logit"] + 0.5) + 1e-4
        s["m_T"] = (_softplus(tl) + 1e-4) * (2 + tl.abs())
        s["d_T"] = torch.sigmoid(tl)
    if ins.get("bg_image") is None:
        bv = torch.sigmoid(val["bg_value"])
        s["bg_val"] = torch.sigmoid(raw["bg_value"])
        s["m_bg_val"] = bv * (2 + val["bg_value"].abs())
        s["d_bg_val"] = bv * (1 - bv)
    return s


def _geometry(pose, HW, ts):
    """sample positions of every (image, component, pixel), their companions and the four
    bilinear taps as (texel index, inside mask, wx, wy, d wx / d ix, d wy / d iy)"""
    H, W = HW
    th, tw = ts
    xs = (2 * torch.arange(W, dtype=torch.float64) + 1) / W - 1
    ys = (2 * torch.arange(H, dtype=torch.float64) + 1) / H - 1
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    xn, yn = gx.reshape(-1), gy.reshape(-1)                               # (P,)
    a = pose.unsqueeze(-1)                                                # (b,M,6,1)
    ix = ((a[:, :, 0] * xn + a[:, :, 1] * yn + a[:, :, 2] + 1) * tw - 1) / 2
    iy = ((a[:, :, 3] * xn + a[:, :, 4] * yn + a[:, :, 5] + 1) * th - 1) / 2
    ad = a.detach().abs()
    m_ix = ((ad[:, :, 0] * xn.abs() + ad[:, :, 1] * yn.abs() + ad[:, :, 2] + 1) * tw + 1) / 2
    m_iy = ((ad[:, :, 3] * xn.abs() + ad[:, :, 4] * yn.abs() + ad[:, :, 5] + 1) * th + 1) / 2
    x0, y0 = torch.floor(ix.detach()), torch.floor(iy.detach())
    fx, fy = ix - x0, iy - y0
    taps = []
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        xi, yi = x0 + dx, y0 + dy
        ok = ((xi >= 0) & (xi < tw) & (yi >= 0) & (yi < th)).double()
        idx = (yi.clamp(0, th - 1) * tw + xi.clamp(0, tw - 1)).long()
        taps.append((idx, ok, fx if dx else 1 - fx, fy if dy else 1 - fy,
                     1.0 if dx else -1.0, 1.0 if dy else -1.0))
    return dict(xn=xn, yn=yn, ix=ix, iy=iy, m_ix=m_ix, m_iy=m_iy, taps=taps)


def _sample(planes, geo):
    """planes (b,M,c,th*tw) -> value, d/dix, d/diy (b,M,c,P) and the companions of the three"""
    b, M, c, _ = planes.shape
    P = geo["xn"].numel()
    v = dvx = dvy = av = adx = ady = across = 0.0
    for idx, ok, wx, wy, sx, sy in geo["taps"]:
        t = torch.gather(planes, 3, idx.unsqueeze(2).expand(b, M, c, P)) * ok.unsqueeze(2)
        wx, wy = wx.unsqueeze(2), wy.unsqueeze(2)
        v = v + t * wx * wy
        dvx = dvx + t * sx * wy
        dvy = dvy + t * sy * wx
        at, wxd, wyd = t.detach().abs(), wx.detach(), wy.detach()
        av, adx, ady, across = av + at * wxd * wyd, adx + at * wyd, ady + at * wxd, across + at
    m_ix, m_iy = geo["m_ix"].unsqueeze(2), geo["m_iy"].unsqueeze(2)
    m_v = av + dvx.detach().abs() * m_ix + dvy.detach().abs() * m_iy
    return v, dvx, dvy, m_v, adx + across * m_iy, ady + across * m_ix


def _lsp(presence32):
    """log_safe(presence) on the fp32 value, its companion, and log_safe's gradient"""
    small = presence32 < EPS32
    p = presence32.double()
    safe = torch.where(small, torch.ones_like(p), p)
    lsp = torch.where(small, torch.full_like(p, -1e8), safe.log())
    lsg = torch.where(small, torch.zeros_like(p), 1 / safe)
    return lsp, lsp.abs() + 1, lsg, small


def _lse(a, m_a):
    """log-sum-exp over dim 1 with its companion"""
    mx = a.max(1, keepdim=True)[0]
    sm = torch.exp(a - mx).sum(1, keepdim=True)
    lse = mx + sm.log()
    p = torch.exp(a - lse).detach()
    m = mx.detach().abs() + sm.detach().log().abs() + (p * m_a).sum(1, keepdim=True)
    return lse, m


def _chunk_forward(ins, HW, lo, hi, leaves=None, sc_leaves=None):
    """images [lo, hi): every forward quantity as differentiable fp64 tensors (of ``leaves``
    where given) plus the detached companions"""
    t32 = ins["templates"]
    B0, M, C, th, tw = t32.shape
    B = ins["pose"].shape[0]
    rep = B // B0
    b = hi - lo
    P = HW[0] * HW[1]
    alpha_mode = ins.get("alpha") is not None
    if leaves is not None:
        templates, pose, alpha = leaves["templates"], leaves["pose"], leaves.get("alpha")
        bg_image = leaves.get("bg_image")
    else:
        tsel = torch.arange(lo, hi) // rep
        templates = _d(t32)[tsel]
        pose = _d(ins["pose"])[lo:hi]
        alpha = _d(ins["alpha"]).unsqueeze(0).expand(b, M, th, tw) if alpha_mode else None
        bg_image = _d(ins["bg_image"])[lo:hi] if ins.get("bg_image") is not None else None
    sc = _scalars(ins, sc_leaves)

    def per(v, k0, k1):     # a scalar, or its (b, K) per-component leaf, as (b, k1 - k0, 1, 1)
        return v if v.dim() == 0 else v[:, k0:k1].reshape(b, k1 - k0, 1, 1)
    geo = _geometry(pose, HW, (th, tw))
    tv, tdx, tdy, m_tv, m_tdx, m_tdy = _sample(templates.reshape(b, M, C, th * tw), geo)
    if bg_image is not None:
        bg = bg_image.reshape(b, 1, C, P)
        m_bg = torch.zeros_like(bg.detach())
    else:
        bg = per(sc["bg_val"], M, M + 1) * torch.ones(b, 1, C, P, dtype=torch.float64)
        m_bg = sc["m_bg_val"] * torch.ones(b, 1, C, P, dtype=torch.float64)
    tt = torch.cat([tv, bg], 1)                                           # (b,K,C,P)
    m_tt = torch.cat([m_tv, m_bg], 1)
    if ins.get("presence") is not None:
        lsp, m_lsp, lsg, _ = _lsp(ins["presence"][lo:hi])
        if leaves is not None and leaves.get("presence") is not None:
            # log_safe as a function of the leaf: log where live, the constant where floored
            lsp = torch.where(lsg > 0, leaves["presence"].clamp_min(1e-300).log(), lsp)
    else:
        lsp = m_lsp = lsg = torch.zeros(b, M, dtype=torch.float64)
    lsp4 = torch.cat([lsp, torch.zeros(b, 1, dtype=torch.float64)], 1).reshape(b, M + 1, 1, 1)
    m_lsp4 = torch.cat([m_lsp, torch.zeros(b, 1, dtype=torch.float64)], 1).reshape(b, M + 1, 1, 1)
    out = dict(geo=geo, sc=sc, tdx=tdx, tdy=tdy, m_tdx=m_tdx, m_tdy=m_tdy, lsg=lsg)
    if alpha_mode:
        aval, adx, ady, m_a, m_adx, m_ady = _sample(alpha.reshape(b, M, 1, th * tw), geo)
        bgml = per(sc["bg_ml"], M, M + 1) * torch.ones(b, 1, 1, P, dtype=torch.float64)
        ml = torch.cat([aval + lsp4[:, :M], bgml], 1)                     # (b,K,1,P)
        m_ml = torch.cat([m_a + m_lsp4[:, :M],
                          sc["m_bg_ml"] * torch.ones(b, 1, 1, P, dtype=torch.float64)], 1)
        out.update(adx=adx, ady=ady, m_adx=m_adx, m_ady=m_ady)
    else:
        T = per(sc["T"], 0, M + 1)
        ml = tt / T + lsp4
        Td = T.detach()
        m_ml = (m_tt + tt.detach().abs()) / Td + tt.detach().abs() / (Td * Td) * sc["m_T"] + m_lsp4
    out.update(tt=tt, ml=ml, m_tt=m_tt, m_ml=m_ml)
    return out


def _chunk_likelihood(f, x, ins):
    """adds log_prob, lse_post, lse_prior (b,C|Cm,P) and companions to a chunk's forward"""
    b, K = f["tt"].shape[:2]
    sc = f["sc"]
    sg = sc["sigma"] if sc["sigma"].dim() == 0 else sc["sigma"].reshape(b, K, 1, 1)
    d = x.unsqueeze(1) - f["tt"]
    iv = 1 / (sg * sg)
    n = -(d * d) * (0.5 * iv) - sg.log() - HALF_LOG_2PI
    dd, ivd, sgd = d.detach(), iv.detach(), sg.detach()
    m_n = dd * dd * 0.5 * ivd + dd.abs() * ivd * f["m_tt"] + \
        (dd * dd * ivd / sgd + 1 / sgd) * sc["m_sigma"] + sgd.log().abs() + HALF_LOG_2PI
    post = f["ml"] + n
    m_post = f["m_ml"] + m_n
    lse_post, m_lse_post = _lse(post, m_post)
    lse_prior, m_lse_prior = _lse(f["ml"], f["m_ml"])
    f.update(d=d, iv=iv, post=post, m_post=m_post,
             lse_post=lse_post.squeeze(1), m_lse_post=m_lse_post.squeeze(1),
             lse_prior=lse_prior.squeeze(1), m_lse_prior=m_lse_prior.squeeze(1))
    f["log_prob"] = f["lse_post"] - f["lse_prior"]
    f["m_log_prob"] = f["m_lse_post"] + f["m_lse_prior"]
    return f


def _chunks(ins, HW):
    B0, M, C = ins["templates"].shape[:3]
    B = ins["pose"].shape[0]
    nb = max(1, CHUNK_ELEMS // ((M + 1) * C * HW[0] * HW[1]))
    return [(lo, min(B, lo + nb)) for lo in range(0, B, nb)]


def _cat(parts):
    keys = parts[0].keys()
    return {k: torch.cat([p[k] for p in parts], 0) for k in keys}


def forward(ins, HW, want=("tt", "ml", "log_prob", "lse_post", "lse_prior", "mean")):
    """-> {name: fp64 tensor, "m_" + name: its companion} for the names in ``want``:
    tt (B,K,C,P), ml (B,K,Cm,P), log_prob / lse_post (B,C,P), lse_prior (B,Cm,P), mean (B,C,P)."""
    parts = []
    with torch.no_grad():
        for lo, hi in _chunks(ins, HW):
            f = _chunk_forward(ins, HW, lo, hi)
            if any(k in want for k in ("log_prob", "lse_post", "lse_prior")):
                C = f["tt"].shape[2]
                _chunk_likelihood(f, _d(ins["x"])[lo:hi].reshape(hi - lo, C, -1), ins)
            if "mean" in want:
                _, m_lse = _lse(f["ml"], f["m_ml"])
                p = torch.softmax(f["ml"], 1)
                m_p = p * (1 + f["m_ml"] + m_lse) + FLOOR
                f["mean"] = (p * f["tt"]).sum(1)
                f["m_mean"] = (p * f["m_tt"] + m_p * f["tt"].abs()).sum(1)
            parts.append({k: f[k] for w in want for k in (w, "m_" + w)})
    return _cat(parts)


def tile_sums(log_prob, m_log_prob, tiles, ppb):
    """(B,C,P) per-pixel log-probs -> (B,tiles) sums over channels and the ppb pixels of a
    tile, with companions (the terms that are added, and what each carries)"""
    B, C, P = log_prob.shape
    pad = tiles * ppb - P
    assert 0 <= pad < ppb
    s = F.pad(log_prob, (0, pad)).reshape(B, C, tiles, ppb).sum((1, 3))
    m = F.pad(m_log_prob + log_prob.abs(), (0, pad)).reshape(B, C, tiles, ppb).sum((1, 3))
    return s, m


def spread_tiles(g_tile, ppb, C, P):
    """(B,tiles) gradient of the tile sums -> the (B,C,P) per-pixel gradient it stands for"""
    return g_tile.double().repeat_interleave(ppb, 1)[:, :P].unsqueeze(1).expand(-1, C, -1)


def mode_error(out, ins, HW):
    """worst |out - tt[k]| / bound over the pixels, the best over every component k whose fp64
    mixing logit is within the two logits' own fp32 bounds of the maximum (the arg-max of a
    near tie is decided by rounding, in the fp32 oracle as in the kernel)"""
    f = forward(ins, HW, want=("tt", "ml"))
    ml, m_ml, tt, m_tt = f["ml"], f["m_ml"], f["tt"], f["m_tt"]
    top, at = ml.max(1, keepdim=True)
    near = (top - ml) <= C_OUT["ml"] * U * (m_ml + torch.gather(m_ml, 1, at))   # (B,K,Cm,P)
    err = (out.detach().double().cpu().reshape(tt.shape[0], 1, tt.shape[2], -1) - tt).abs()
    r = err / (C_OUT["tt"] * U * m_tt).clamp_min(1e-300)    # (a companion of 0: exact or nothing)
    r = torch.where(near.expand_as(r), r, torch.full_like(r, math.inf))
    return float(r.min(1)[0].max())


def mixture_mean(loc, ml):
    """gmm_mean of given tensors (B,K,C,P), (B,K,Cm,P), taken as exact -> (mean, companion)"""
    loc, ml = loc.detach().double().cpu(), ml.detach().double().cpu()
    _, m_lse = _lse(ml, ml.abs())
    p = torch.softmax(ml, 1)
    m_p = p * (1 + ml.abs() + m_lse) + FLOOR
    return (p * loc).sum(1), ((p + m_p) * loc.abs()).sum(1)


def mixture_mode_ok(out, loc, ml, slack=0.0):
    """gmm_mode of given fp32 tensors: every output entry is, bit for bit, the value of a
    component whose logit is the largest (``slack``: or within slack (|max| + 1) of it) --
    with slack 0 and the first such component, torch.argmax's choice"""
    loc, ml = loc.detach().cpu(), ml.detach().double().cpu()
    B, K, C, P = loc.shape
    top = ml.max(1, keepdim=True)[0]
    if slack == 0.0:
        pick = ml.argmax(1, keepdim=True).expand(B, 1, C, P)
        return torch.equal(out.detach().cpu().reshape(B, C, P), torch.gather(loc, 1, pick)[:, 0])
    near = ((top - ml) <= slack * (top.abs() + 1)).expand(B, K, C, P)
    hit = (out.detach().cpu().reshape(B, 1, C, P) == loc) & near
    return bool(hit.any(1).all())


def _incoming(grads, f, x, lo, hi):
    """the per-component gradients on tt and ml (with companions) that a chunk's backward
    starts from, plus the sigma partials; fused (g_logprob) or unfused (g_tt / g_ml)"""
    tt, ml = f["tt"], f["ml"]
    b, K, C, P = tt.shape
    sc = f["sc"]
    z = torch.zeros_like(tt)
    if grads.get("g_logprob") is not None:
        g = _d(grads["g_logprob"])[lo:hi].reshape(b, 1, C, P)
        ga = g.abs()
        sg, iv, d = sc["sigma"], f["iv"], f["d"]
        w = torch.exp(f["post"] - f["lse_post"].unsqueeze(1))
        m_w = w * (1 + f["m_post"] + f["m_lse_post"].unsqueeze(1)) + FLOOR
        spr = torch.exp(ml - f["lse_prior"].unsqueeze(1))
        m_spr = spr * (1 + f["m_ml"] + f["m_lse_prior"].unsqueeze(1)) + FLOOR
        gtt = g * w * d * iv
        m_gtt = ga * (m_w * d.abs() * iv + w * f["m_tt"] * iv
                      + w * d.abs() * iv * 2 * sc["m_sigma"] / sg)
        gml = g * (w - spr)
        m_gml = ga * (m_w + m_spr)
        gsig = (g * w * (d * d * iv - 1) / sg).sum((2, 3))
        m_gsig = (ga * (m_w * (d * d * iv + 1) / sg + w * 2 * d.abs() * f["m_tt"] * iv / sg
                        + w * (3 * d * d * iv + 1) / (sg * sg) * sc["m_sigma"])).sum((2, 3))
    else:
        gtt = _d(grads["g_tt"])[lo:hi].reshape(b, K, C, P) if grads.get("g_tt") is not None else z
        gml = _d(grads["g_ml"])[lo:hi].reshape(ml.shape) if grads.get("g_ml") is not None \
            else torch.zeros_like(ml)
        m_gtt, m_gml = gtt.abs(), gml.abs()
        gsig = m_gsig = torch.zeros(b, K, dtype=torch.float64)
    return gtt, m_gtt, gml, m_gml, gsig, m_gsig


def _chunk_backward(ins, HW, grads, lo, hi, moments=False):
    t32 = ins["templates"]
    B0, M, C, th, tw = t32.shape
    b, K, P, tsz = hi - lo, M + 1, HW[0] * HW[1], th * tw
    alpha_mode = ins.get("alpha") is not None
    f = _chunk_forward(ins, HW, lo, hi)
    x = _d(ins["x"])[lo:hi].reshape(b, C, P) if ins.get("x") is not None else None
    if grads.get("g_logprob") is not None:
        _chunk_likelihood(f, x, ins)
    sc, geo = f["sc"], f["geo"]
    gtt, m_gtt, gml, m_gml, gsig, m_gsig = _incoming(grads, f, x, lo, hi)
    gT = m_gT = torch.zeros(b, K, dtype=torch.float64)
    if alpha_mode:
        gmla, m_gmla = gml.sum(2, keepdim=True), m_gml.sum(2, keepdim=True)   # (b,K,1,P)
        gpres_sum, m_gpres_sum = gmla.sum((2, 3)), m_gmla.sum((2, 3))
    else:
        T, tt, m_tt = sc["T"], f["tt"], f["m_tt"]
        gT = (-gml * tt / (T * T)).sum((2, 3))
        m_gT = ((m_gml * tt.abs() + gml.abs() * m_tt) / (T * T)
                + 2 * (gml * tt).abs() / (T * T * T) * sc["m_T"]).sum((2, 3))
        gpres_sum, m_gpres_sum = gml.sum((2, 3)), m_gml.sum((2, 3))
        m_gtt = m_gtt + m_gml / T + gml.abs() / (T * T) * sc["m_T"]
        gtt = gtt + gml / T
    # ---- texel gradients: every pixel's four taps, scattered
    g_t = torch.zeros(b, M, C, tsz, dtype=torch.float64)
    m_g_t = torch.zeros_like(g_t)
    g_a = m_g_a = None
    if alpha_mode:
        g_a = torch.zeros(b, M, 1, tsz, dtype=torch.float64)
        m_g_a = torch.zeros_like(g_a)
    m_ix, m_iy = geo["m_ix"].unsqueeze(2), geo["m_iy"].unsqueeze(2)
    fx, fy = geo["taps"][1][2].unsqueeze(2), geo["taps"][2][3].unsqueeze(2)
    # the cell-gather form's terms per corner (module docstring): S0 - S1 - S2 + S3, S1 - S3,
    # S2 - S3, S3 with S = sum g {1, fx, fy, fx fy}
    mom = (1 + fx + fy + fx * fy, fx + fx * fy, fy + fx * fy, fx * fy)
    for (idx, ok, wx, wy, sx, sy), mo in zip(geo["taps"], mom):
        i4, ok, wx, wy = idx.unsqueeze(2), ok.unsqueeze(2), wx.unsqueeze(2), wy.unsqueeze(2)
        pos = ok * (wy * m_ix + wx * m_iy)
        if moments:
            pos = pos + ok * mo
        g_t.scatter_add_(3, i4.expand(b, M, C, P), gtt[:, :M] * wx * wy * ok)
        m_g_t.scatter_add_(3, i4.expand(b, M, C, P),
                           m_gtt[:, :M] * wx * wy * ok + gtt[:, :M].abs() * pos)
        if alpha_mode:
            g_a.scatter_add_(3, i4, gmla[:, :M] * wx * wy * ok)
            m_g_a.scatter_add_(3, i4, m_gmla[:, :M] * wx * wy * ok + gmla[:, :M].abs() * pos)
    # ---- pose
    gix = (gtt[:, :M] * f["tdx"]).sum(2)
    giy = (gtt[:, :M] * f["tdy"]).sum(2)
    m_gix = (m_gtt[:, :M] * f["tdx"].abs() + gtt[:, :M].abs() * f["m_tdx"]).sum(2)
    m_giy = (m_gtt[:, :M] * f["tdy"].abs() + gtt[:, :M].abs() * f["m_tdy"]).sum(2)
    if alpha_mode:
        gix = gix + (gmla[:, :M] * f["adx"]).sum(2)
        giy = giy + (gmla[:, :M] * f["ady"]).sum(2)
        m_gix = m_gix + (m_gmla[:, :M] * f["adx"].abs() + gmla[:, :M].abs() * f["m_adx"]).sum(2)
        m_giy = m_giy + (m_gmla[:, :M] * f["ady"].abs() + gmla[:, :M].abs() * f["m_ady"]).sum(2)
    hx, hy = 0.5 * tw, 0.5 * th
    xn, yn = geo["xn"], geo["yn"]
    one = torch.ones_like(xn)
    g_pose = torch.stack([(gix * v).sum(-1) * hx for v in (xn, yn, one)]
                         + [(giy * v).sum(-1) * hy for v in (xn, yn, one)], -1)
    m_g_pose = torch.stack([(m_gix * v.abs()).sum(-1) * hx for v in (xn, yn, one)]
                           + [(m_giy * v.abs()).sum(-1) * hy for v in (xn, yn, one)], -1)
    out = dict(templates=g_t.reshape(b, M, C, th, tw), pose=g_pose)
    mag = dict(templates=m_g_t.reshape(b, M, C, th, tw), pose=m_g_pose)
    if alpha_mode:
        out["alpha_partial"], mag["alpha_partial"] = g_a.reshape(b, M, th, tw), m_g_a.reshape(b, M, th, tw)
    if ins.get("presence") is not None:
        out["presence"] = gpres_sum[:, :M] * f["lsg"]
        mag["presence"] = m_gpres_sum[:, :M] * f["lsg"].abs()
    # ---- background and the four scalars' per-(image, component) partials
    sp = torch.zeros(b, K, 4, dtype=torch.float64)
    m_sp = torch.zeros_like(sp)
    if ins.get("bg_image") is not None:
        out["bg_image"], mag["bg_image"] = gtt[:, M], m_gtt[:, M]
    else:
        sp[:, M, 0] = gtt[:, M].sum((1, 2)) * sc["d_bg_val"]
        m_sp[:, M, 0] = m_gtt[:, M].sum((1, 2)) * sc["d_bg_val"]
    if alpha_mode:
        sp[:, M, 1] = gmla[:, M].sum((1, 2)) * sc["d_bg_ml"]
        m_sp[:, M, 1] = m_gmla[:, M].sum((1, 2)) * sc["d_bg_ml"]
    else:
        sp[:, :, 2], m_sp[:, :, 2] = gT * sc["d_T"], m_gT * sc["d_T"]
    if ins.get("scale") is not None:
        sp[:, :, 3], m_sp[:, :, 3] = gsig * sc["d_sigma"], m_gsig * sc["d_sigma"]
    out["scalar_partial"], mag["scalar_partial"] = sp, m_sp
    return out, mag


def backward(ins, HW, grads, moments=False):
    """``grads``: {"g_logprob": (B,C,H,W)} (fused) or any of {"g_tt": (B,K,C,H,W), "g_ml":
    (B,K,Cm,H,W)} (unfused) -> (gradients, companions): templates (B,M,C,th,tw),
    alpha_partial (B,M,th,tw), pose (B,M,6), presence (B,M), bg_image (B,C,P),
    scalar_partial (B,K,4: bg_value, bg_mixing_logit, temperature_logit, scale) -- the
    names a mode does not have are absent.  ``moments``: the texel gradients' companions for
    the cell-gather form, which adds the four moment sums of a cell (module docstring)."""
    assert ins["pose"].shape[0] == ins["templates"].shape[0], "no backward under template_repeat"
    outs, mags = [], []
    with torch.no_grad():
        for lo, hi in _chunks(ins, HW):
            o, m = _chunk_backward(ins, HW, grads, lo, hi, moments)
            outs.append(o)
            mags.append({k: v + FLOOR for k, v in m.items()})
    return _cat(outs), _cat(mags)


def autograd_backward(ins, HW, grads):
    """the same gradients by fp64 autograd through this module's forward formulas: the scalar
    parameters enter as (B, K) leaves, so that their gradients are the per-component partials"""
    B, M, C, th, tw = ins["templates"].shape
    K, P = M + 1, HW[0] * HW[1]
    alpha_mode = ins.get("alpha") is not None
    leaf = lambda t: _d(t).clone().requires_grad_(True)      # noqa: E731
    lv = dict(templates=leaf(ins["templates"]), pose=leaf(ins["pose"]))
    if alpha_mode:
        lv["alpha"] = leaf(ins["alpha"].unsqueeze(0).expand(B, M, th, tw))
    for k in ("presence", "bg_image"):
        if ins.get(k) is not None:
            lv[k] = leaf(ins[k])
    scl = {k: leaf(ins[k].reshape(1, 1).expand(B, K)) for k in
           ("bg_value", "bg_mixing_logit", "temperature_logit", "scale") if ins.get(k) is not None}
    f = _chunk_forward(ins, HW, 0, B, leaves=lv, sc_leaves=scl)
    if grads.get("g_logprob") is not None:
        _chunk_likelihood(f, _d(ins["x"]).reshape(B, C, P), ins)
        tot = (f["log_prob"] * _d(grads["g_logprob"]).reshape(B, C, P)).sum()
    else:
        tot = 0.0
        if grads.get("g_tt") is not None:
            tot = tot + (f["tt"] * _d(grads["g_tt"]).reshape(f["tt"].shape)).sum()
        if grads.get("g_ml") is not None:
            tot = tot + (f["ml"] * _d(grads["g_ml"]).reshape(f["ml"].shape)).sum()
    names = list(lv) + list(scl)
    gs = torch.autograd.grad(tot, [dict(lv, **scl)[k] for k in names], allow_unused=True)
    g = {k: (torch.zeros_like(dict(lv, **scl)[k]) if v is None else v) for k, v in zip(names, gs)}
    out = dict(templates=g["templates"], pose=g["pose"])
    if alpha_mode:
        out["alpha_partial"] = g["alpha"]
    if "presence" in g:
        out["presence"] = g["presence"]
    if "bg_image" in g:
        out["bg_image"] = g["bg_image"].reshape(B, C, P)
    sp = torch.zeros(B, K, 4, dtype=torch.float64)
    for i, k in enumerate(("bg_value", "bg_mixing_logit", "temperature_logit", "scale")):
        if k in g and not (k == "bg_value" and "bg_image" in g) \
                and not (k == "bg_mixing_logit" and not alpha_mode) \
                and not (k == "temperature_logit" and alpha_mode):
            sp[:, :, i] = g[k]
    out["scalar_partial"] = sp
    return out


def ratio(got, ref, magnitude, c):
    """worst |got - ref| / (c 2^-24 magnitude); an entry with magnitude 0 must be exact."""
    dlt = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    bound = c * U * magnitude
    r = torch.where(bound > 0, dlt / bound.clamp_min(1e-300),
                    torch.where(dlt > 0, torch.full_like(dlt, math.inf), torch.zeros_like(dlt)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------ cell boundaries
def near_cell_boundary(pose, HW, ts, margin=8e-6):
    """(B,M) bool: some pixel's fp64 sample position lies within ``margin`` of a texel-cell
    boundary that matters (inside the template or one cell around it)"""
    H, W = HW
    th, tw = ts
    xs = (2 * torch.arange(W, dtype=torch.float64) + 1) / W - 1
    ys = (2 * torch.arange(H, dtype=torch.float64) + 1) / H - 1
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    gx, gy = gx.reshape(-1), gy.reshape(-1)
    a = pose.double()[..., None]                           # (B, M, 6, 1)
    ix = ((a[:, :, 0] * gx + a[:, :, 1] * gy + a[:, :, 2] + 1) * tw - 1) / 2
    iy = ((a[:, :, 3] * gx + a[:, :, 4] * gy + a[:, :, 5] + 1) * th - 1) / 2
    near = lambda v, n: ((v - v.round()).abs() < margin) \
        & (v > -1.5) & (v < n + 0.5)                       # noqa: E731
    return (near(ix, tw) | near(iy, th)).any(-1)


def clear_of_cell_boundaries(pose, HW, ts, g, margin=8e-6):
    """d log_prob / d pose jumps where a pixel's sample position crosses a
    texel-cell boundary: a pixel within fp32 round-off of one has two valid
    one-sided derivatives (the golden poses are
    'irrational' for the same reason).  Round-off of a position is a few ulp
    of ~10 texels, ~1e-6; capsules with a pixel within 8e-6 get their
    translation nudged until none is left."""
    pose = pose.clone()
    for _ in range(60):
        bad = near_cell_boundary(pose, HW, ts, margin)     # (B, M)
        if not bool(bad.any()):
            return pose
        nudge = torch.randn(pose.shape[0], pose.shape[1], 2, generator=g) * 2e-2
        pose[..., 2] += torch.where(bad, nudge[..., 0], torch.zeros(()))
        pose[..., 5] += torch.where(bad, nudge[..., 1], torch.zeros(()))
    raise AssertionError("poses could not be cleared of cell boundaries")


# ---------------------------------------------------------------------------------------- cases
# forms a case expects (what scae_render_gmm_forms reports)
WAVE, CLASSIC = 0, 1
CELL, SCATTER, GATHER = 0, 1, 2


def _case(name, B, M, C, HW, ts, alpha=True, poses="unit", presence="rand", bg_image=False,
          scale=False, repeat=1, fwd=None, render=None, bwd=None, bwd_unfused=None,
          checks="RFBU", **extra):
    """checks: R render, F likelihood forward (+ sums, mean / mode), B fused backward,
    U unfused backward.  fwd: (form, ksplit, pad); render: form; bwd / bwd_unfused: form."""
    return dict(name=name, B=B, M=M, C=C, HW=HW, ts=ts, alpha=alpha, poses=poses,
                presence=presence, bg_image=bg_image, scale=scale, repeat=repeat, fwd=fwd,
                render=render, bwd=bwd, bwd_unfused=bwd_unfused, checks=checks, **extra)


def all_cases():
    """every case tests/test_part_decoder_vs_fp64.py runs, each with the kernel forms it is
    there for (asserted against the library's own dispatch before anything is compared)"""
    c = [
        # ---- likelihood forward, wave form
        _case("wave-1wave-tiles", 2, 24, 1, (40, 40), (11, 11), fwd=(WAVE, 1, 0), render=WAVE,
              bwd=CELL, bwd_unfused=SCATTER, ppb=64, chunk_rows=20),
        _case("wave-B128", 128, 24, 1, (40, 40), (11, 11), fwd=(WAVE, 1, 0), render=WAVE,
              checks="F", ppb=256),
        _case("wave-B160-7wave-wgs", 160, 4, 1, (40, 40), (11, 11), fwd=(WAVE, 1, 0),
              render=WAVE, checks="F", ppb=448),
        _case("wave-ragged-C3", 4, 5, 3, (17, 23), (7, 9), scale=True, fwd=(WAVE, 1, 0),
              render=CLASSIC, bwd=CELL, bwd_unfused=SCATTER),
        _case("wave-C4", 2, 3, 4, (9, 16), (4, 3), scale=True, fwd=(WAVE, 1, 0), render=WAVE,
              bwd=CELL, bwd_unfused=SCATTER),
        # ---- likelihood forward, classic form (temperature mode)
        _case("classic-ks4-pad", 4, 5, 3, (17, 23), (7, 9), alpha=False, scale=True,
              fwd=(CLASSIC, 4, 1), render=CLASSIC, bwd=SCATTER, bwd_unfused=SCATTER),
        _case("classic-ks2", 256, 3, 1, (32, 32), (5, 5), alpha=False, fwd=(CLASSIC, 2, 1),
              render=CLASSIC, checks="F"),
        _case("classic-ks1", 1024, 2, 1, (32, 32), (5, 5), alpha=False, fwd=(CLASSIC, 1, 1),
              render=CLASSIC, checks="F"),
        _case("classic-ks2-unpadded", 256, 10, 1, (32, 32), (44, 44), alpha=False,
              fwd=(CLASSIC, 2, 0), render=CLASSIC, checks="F"),
        _case("classic-ks1-unpadded", 1024, 10, 1, (32, 32), (44, 44), alpha=False,
              fwd=(CLASSIC, 1, 0), render=CLASSIC, checks="F"),
        _case("classic-unpadded", 2, 40, 3, (12, 18), (11, 11), alpha=False,
              fwd=(CLASSIC, 4, 0), render=CLASSIC, bwd=GATHER, bwd_unfused=GATHER),
        _case("classic-in-alpha-mode", 2, 70, 3, (12, 12), (11, 11), fwd=(CLASSIC, 4, 0),
              render=WAVE, bwd=CELL, bwd_unfused=GATHER, checks="RFB"),
        # ---- render
        _case("render-9x15", 3, 7, 2, (9, 15), (5, 6), fwd=(WAVE, 1, 0), render=CLASSIC,
              bwd=CELL, bwd_unfused=GATHER),
        # ---- backward, cell-gather
        _case("cell-32x32-C3", 2, 6, 3, (32, 32), (11, 11), fwd=(WAVE, 1, 0), render=WAVE,
              bwd=CELL, bwd_unfused=GATHER, chunk_rows=32, checks="FBU"),
        _case("cell-collapsed", 4, 8, 1, (40, 40), (11, 11), poses="collapsed",
              fwd=(WAVE, 1, 0), render=WAVE, bwd=CELL, bwd_unfused=SCATTER, checks="FB"),
        _case("cell-5x6-template", 2, 4, 1, (24, 24), (5, 6), fwd=(WAVE, 1, 0), render=WAVE,
              bwd=CELL, bwd_unfused=SCATTER, checks="FB"),
        _case("cell-17x17-template", 2, 3, 1, (24, 24), (17, 17), fwd=(WAVE, 1, 0),
              render=WAVE, bwd=CELL, bwd_unfused=GATHER, checks="FBU"),
        # ---- backward, scatter and gather
        _case("scatter-W16", 2, 4, 1, (12, 16), (7, 7), alpha=False, fwd=(CLASSIC, 4, 1),
              render=CLASSIC, bwd=SCATTER, bwd_unfused=SCATTER),
        _case("gather-W15", 2, 4, 1, (12, 15), (7, 7), alpha=False, fwd=(CLASSIC, 4, 1),
              render=CLASSIC, bwd=GATHER, bwd_unfused=GATHER),
        _case("gather-two-passes", 1, 3, 3, (48, 64), (11, 11), alpha=False,
              fwd=(CLASSIC, 4, 1), render=CLASSIC, bwd=GATHER, bwd_unfused=GATHER,
              gather_rows=40, checks="FB"),
        _case("fallback-no-cell", 1, 2, 1, (16, 16), (36, 36), fwd=(WAVE, 1, 0),
              render=WAVE, bwd=GATHER, bwd_unfused=GATHER, checks="FB"),
        # ---- regimes
        _case("regime-init", 8, 8, 1, (40, 40), (11, 11), poses="init", fwd=(WAVE, 1, 0),
              render=WAVE, bwd=CELL, bwd_unfused=SCATTER, checks="RFBU"),
        _case("regime-mixed", 8, 8, 1, (40, 40), (11, 11), poses="mixed", fwd=(WAVE, 1, 0),
              render=WAVE, bwd=CELL, bwd_unfused=SCATTER, checks="RFBU"),
        _case("regime-collapsed-C3", 8, 6, 3, (32, 32), (11, 11), poses="collapsed",
              fwd=(WAVE, 1, 0), render=WAVE, bwd=CELL, bwd_unfused=GATHER, checks="RFBU"),
        _case("outside-template", 2, 4, 1, (16, 16), (7, 7), poses="outside", fwd=(WAVE, 1, 0),
              render=WAVE, bwd=CELL, bwd_unfused=SCATTER),
        _case("presence-0-1e-18-1", 3, 6, 1, (16, 16), (7, 7), presence="edges",
              fwd=(WAVE, 1, 0), render=WAVE, bwd=CELL, bwd_unfused=SCATTER),
        _case("presence-0-1e-18-1-temperature", 3, 6, 1, (16, 16), (7, 7), alpha=False,
              presence="edges", fwd=(CLASSIC, 4, 1), render=CLASSIC, bwd=SCATTER,
              bwd_unfused=SCATTER),
        _case("no-presence", 2, 4, 2, (16, 16), (7, 7), presence=None, fwd=(WAVE, 1, 0),
              render=WAVE, bwd=CELL, bwd_unfused=SCATTER),
        _case("bg-image", 2, 4, 3, (16, 16), (7, 7), bg_image=True, scale=True,
              fwd=(WAVE, 1, 0), render=WAVE, bwd=CELL, bwd_unfused=SCATTER),
        _case("bg-image-temperature", 2, 4, 3, (17, 23), (7, 9), alpha=False, bg_image=True,
              scale=True, fwd=(CLASSIC, 4, 1), render=CLASSIC, bwd=SCATTER,
              bwd_unfused=SCATTER),
        _case("template-repeat-3", 6, 4, 1, (16, 16), (7, 7), repeat=3, fwd=(WAVE, 1, 0),
              render=WAVE, checks="RF"),
    ]
    return c


def case_id(c):
    return c["name"]


def _unit_poses(B, M, g):
    pose = torch.randn(B, M, 6, generator=g) * 0.5
    pose[:, :, 0] += 1.0
    pose[:, :, 4] += 1.0
    return pose


def _small_poses(B, M, g):
    small = torch.randn(B, M, 6, generator=g) * 0.003
    small[:, :, 0] += 0.01
    small[:, :, 4] += 0.01
    small[:, :, 2] = torch.rand(B, M, generator=g) * 2.4 - 1.2
    small[:, :, 5] = torch.rand(B, M, generator=g) * 2.4 - 1.2
    return small


def make_case(c, reseed=0, inputs=None):
    """-> (ins: fp32 tensors, HW).  The pose regimes restate ``_regime_inputs`` of
    tests/test_hip_ops.py; its "init" regime runs a freshly initialised part encoder on the
    GPU, so here it is a stand-in (small random affine maps) and the GPU module passes the
    real (pose, presence) as ``inputs``."""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(c["name"])) + 7919 * reseed
    g = torch.Generator().manual_seed(seed)
    B, M, C, HW, ts = c["B"], c["M"], c["C"], c["HW"], c["ts"]
    B0 = B // c["repeat"]
    ins = dict(templates=torch.rand(B0, M, C, *ts, generator=g),
               alpha=torch.randn(M, *ts, generator=g) * 0.5 if c["alpha"] else None,
               x=torch.rand(B, C, *HW, generator=g),
               bg_value=torch.randn(1, generator=g) * 0.5,
               bg_mixing_logit=torch.randn(1, generator=g) * 0.5,
               temperature_logit=torch.randn(1, generator=g) * 0.5,
               scale=torch.randn(1, generator=g) * 0.5 if c["scale"] else None,
               bg_image=torch.rand(B, C, *HW, generator=g) if c["bg_image"] else None)
    unit, small = _unit_poses(B, M, g), _small_poses(B, M, g)
    presence = torch.rand(B, M, generator=g)
    kind = c["poses"]
    if kind == "unit":
        pose = unit
    elif kind == "init":
        pose = torch.randn(B, M, 6, generator=g) * 0.3
        pose[:, :, 0] += 0.25
        pose[:, :, 4] += 0.25
    elif kind == "collapsed":
        pose = small
        presence = torch.where(presence < 0.5, torch.full_like(presence, 1e-18),
                               torch.zeros_like(presence))
        presence[:, 0] = torch.rand(B, generator=g)
    elif kind == "mixed":
        pick = torch.rand(B, M, generator=g)
        pose = torch.where((pick < 0.5)[..., None], small, unit)
        one_axis = (pick >= 0.5) & (pick < 0.65)
        pose[..., 0] = torch.where(one_axis, small[..., 0], pose[..., 0])
        pose[..., 1] = torch.where(one_axis, small[..., 1], pose[..., 1])
        presence = torch.where(pick < 0.25, torch.full_like(presence, 1e-18), presence)
    elif kind == "outside":
        pose = unit
        pose[:, 1, 2] = 5.0          # capsule 1: every sample position beyond the template
    else:
        raise ValueError(kind)
    if inputs is not None:
        pose, presence = inputs[0].clone().float(), inputs[1].clone().float()
    if c["presence"] == "edges":
        presence[:, 0], presence[:, 1], presence[:, 2] = 0.0, 1e-18, 1.0
    ins["pose"] = clear_of_cell_boundaries(pose, HW, ts, g)
    ins["presence"] = None if c["presence"] is None else presence
    return ins, tuple(HW)


def checked_case(c, inputs=None):
    """``make_case``; asserts that no (capsule, pixel) is within 8e-6 of a cell boundary"""
    ins, HW = make_case(c, inputs=inputs)
    assert not bool(near_cell_boundary(ins["pose"], HW, c["ts"]).any()), c["name"]
    return ins, HW


def make_grads(c, seed=0):
    """incoming gradients, seeded (fp32): per-pixel g_logprob, g_tt, g_ml"""
    g = torch.Generator().manual_seed(4242 + seed + c["B"] * 31 + c["M"] * 7)
    B, K, C, HW = c["B"], c["M"] + 1, c["C"], c["HW"]
    Cm = 1 if c["alpha"] else C
    return dict(g_logprob=torch.randn(B, C, *HW, generator=g),
                g_tt=torch.randn(B, K, C, *HW, generator=g),
                g_ml=torch.randn(B, K, Cm, *HW, generator=g))
