"""fp64 reference of the object-capsule votes (K3: csrc/capsule_votes.hip, the stand-alone
wave-per-capsule form, and csrc/capsule_votes_dev.h ``fwd_block`` / ``bwd_block``, the form
that rides in the K7b chain launches) that also says how far an fp32 evaluation may be from
it.  CPU only; no GPU import.

``forward`` restates ``oracle.scae_oracle.capsule_layer`` from ``all_param`` onwards (the
non-hierarchical form) in fp64: the split of the 8V+7 parameters, the two pose transforms of
cv_ops.py:20-76 and their 2x3 product, the presence logits with their uniform noise, the vote
presences, the vote scale, and -- what the kernel adds -- the per-capsule partial of the
deformation regulariser ``reg_partial = sum dyn^2`` and ``caps_presence = max_v
vote_presence`` with its first maximiser ``caps_arg``.  The constants are the fp32 values the
fp32 oracle and the kernel both hold (``K32``: 2 pi and 1e-2 rounded to fp32; .5 and the
softplus threshold 20 are exact); ``K64`` has the doubles, with which the reference equals
the fp64 oracle to 1e-12.  ``backward`` is a hand-written fp64 backward for any subset of the
seven incoming gradients; it takes ``caps_arg``: the gradient of caps_presence goes to the
vote the forward reported.

Every float entry comes with a companion magnitude (``res["scale_of"][name]``, for outputs and
gradients): the same formula with every summand replaced by its absolute value and every
function value f(x) by |f(x)| + |f'(x)| * companion(x) -- 1 - tanh^2 has 1 + tanh^2,
s (1 - s) has s (1 + s), cos(2 pi p) carries |sin| |2 pi p| for the rounding of its argument,
a sum over votes is the sum of its |terms|; ``FLOOR`` (lk_ref's) is added for what an
underflow loses.  A bound is then, entry by entry,

    |fp32 - fp64| <= c * 2^-24 * scale

Measured (tests/test_votes_ref.py::test_constants_come_from_the_fp32_oracle re-measures and
prints them): the fp32 oracle on the CPU against this reference, worst
|fp32 - fp64| / (2^-24 scale) over every case of tests/test_capsule_votes_vs_fp64.py:

    outputs    vote 2.56  scale 1.45  vote_presence 2.31  logit_caps 1.67  logit_vote 1.72
               reg_partial 2.82
    gradients  gall_param 2.43  gall_param_gated 2.32  gcpr_in 2.18
    batch sums cpr_static 0.39  bias_cvr 0.36  bias_caps 0.79  bias_vote 1.31
               bias_scale 1.57
    (gradients: each incoming gradient alone and all seven together; the caps_presence
    gradient routed at the fp64 arg-max where the gap is clear, at the fp32 oracle's own
    first maximum otherwise)

    C_OUT = 20 (4 x 2.82 = 11.3, rounded up to one digit)   C_GRAD = 10 (4 x 2.43 = 9.7)

The factor 4 is for what the kernels do differently from the oracle: 64-lane, 16-lane and
4-way summation trees instead of torch's sums, fused multiply-adds, and a device expf / tanhf
/ sinf / cosf of a couple of ulp where the host's are one.  c is never tuned against a kernel.

``_forward`` / ``_backward`` take a set of mutant names (``MUTANTS``): each plants one
mistake of the kind the lane arithmetic invites, for test_votes_ref.py to show that the bar
and the cases see it.
"""
import collections
import math

import numpy as np
import torch

from tests.lk_ref import FLOOR, U, gamma, ratio  # noqa: F401  (re-exported)

C_OUT = 20.0
C_GRAD = 10.0
Consts = collections.namedtuple("Consts", "two_pi off")
K32 = Consts(float(np.float32(2 * math.pi)), float(np.float32(1e-2)))
K64 = Consts(2 * math.pi, 1e-2)

GRAD_NAMES = ("gvote", "gscale", "gvote_presence", "glogit_caps", "glogit_vote", "greg",
              "gcaps_presence")
FLOAT_OUTS = ("vote", "scale", "vote_presence", "logit_caps", "logit_vote", "reg_partial")
GRAD_OUTS = ("gall_param", "gall_param_gated", "gcpr_in")
PARAM_NAMES = ("cpr_static", "bias_cvr", "bias_caps", "bias_vote", "bias_scale")
MUTANTS = ("reg_tail16", "reg_tail64", "last_max", "lane_ties16", "lane_ties64", "quarter",
           "no_gcaps", "reg_no_B", "gate_ge", "sim_leak", "no_noise_bwd", "bias_div")


def _d(t):
    return None if t is None else t.detach().double().cpu()


def _sig(x, cx):
    s = torch.sigmoid(x)
    return s, s + s * torch.sigmoid(-x) * cx + FLOOR


def _tanh5(p, cp):
    t = torch.tanh(5 * p)
    sech2 = 1 / torch.cosh((5 * p).clamp(-300, 300)) ** 2
    return t, t.abs() + sech2 * 5 * cp + FLOOR, 5 * sech2


def _xf(p, cp, sim, K):
    """the pose transform of cv_ops.py:20-76 on (..., 6) with its local derivatives (Xf of
    capsule_votes_dev.h); every value v comes with its companion c_v"""
    x = {}
    ex, x["c_ex"] = _sig(p[..., 0], cp[..., 0])
    ey, x["c_ey"] = _sig(p[..., 1], cp[..., 1])
    x["sx"], x["c_sx"] = ex + K.off, x["c_ex"] + K.off
    x["sy"], x["c_sy"] = ey + K.off, x["c_ey"] + K.off
    # s (1 - s): s (1 + s), and what the round-off of s itself adds (|1 - 2 s| <= 1)
    x["dsx"], x["c_dsx"] = ex * torch.sigmoid(-p[..., 0]), ex * (1 + ex) + (x["c_ex"] - ex)
    x["dsy"], x["c_dsy"] = ey * torch.sigmoid(-p[..., 1]), ey * (1 + ey) + (x["c_ey"] - ey)
    for name, j in (("sh", 3), ("tx", 4), ("ty", 5)):
        t, c_t, x["d" + name] = _tanh5(p[..., j], cp[..., j])
        x[name], x["c_" + name] = t, c_t
        # 5 (1 - t^2): 5 (1 + t^2), and 2 |t| times the round-off of t
        x["c_d" + name] = 5 * (1 + t * t + 2 * t.abs() * (c_t - t.abs()))
    th, c_th = p[..., 2] * K.two_pi, cp[..., 2] * K.two_pi
    x["c"], x["s"] = torch.cos(th), torch.sin(th)
    x["c_c"] = x["c"].abs() + x["s"].abs() * c_th
    x["c_s"] = x["s"].abs() + x["c"].abs() * c_th
    sx, sy, sh, c, s = x["sx"], x["sy"], x["sh"], x["c"], x["s"]
    c_sx, c_sy, c_sh, c_c, c_s = x["c_sx"], x["c_sy"], x["c_sh"], x["c_c"], x["c_s"]
    if sim:
        o = [sx * c, -sx * s, x["tx"], sx * s, sx * c, x["ty"]]
        c_o = [c_sx * c_c, c_sx * c_s, x["c_tx"], c_sx * c_s, c_sx * c_c, x["c_ty"]]
    else:
        o = [sx * c + sh * sy * s, -sx * s + sh * sy * c, x["tx"], sy * s, sy * c, x["ty"]]
        c_o = [c_sx * c_c + c_sh * c_sy * c_s, c_sx * c_s + c_sh * c_sy * c_c, x["c_tx"],
               c_sy * c_s, c_sy * c_c, x["c_ty"]]
    x["o"], x["c_o"] = o, c_o
    return x


def _xf_backward(x, sim, go, c_go, K, leak=False):
    """go, c_go: lists of 6 -> (gp (..., 6), c_gp): xf_backward of capsule_votes_dev.h"""
    sx, sy, sh, c, s = x["sx"], x["sy"], x["sh"], x["c"], x["s"]
    c_sx, c_sy, c_sh, c_c, c_s = x["c_sx"], x["c_sy"], x["c_sh"], x["c_c"], x["c_s"]
    z = torch.zeros_like(go[0] * c)
    if sim:
        gsx = go[0] * c - go[1] * s + go[3] * s + go[4] * c
        a_gsx = c_go[0] * c_c + c_go[1] * c_s + c_go[3] * c_s + c_go[4] * c_c
        gsy, a_gsy, gsh, a_gsh = z, z, z, z
        gth = sx * (-go[0] * s - go[1] * c + go[3] * c - go[4] * s)
        a_gth = c_sx * (c_go[0] * c_s + c_go[1] * c_c + c_go[3] * c_c + c_go[4] * c_s)
    if not sim or leak:
        gsy = go[0] * sh * s + go[1] * sh * c + go[3] * s + go[4] * c
        a_gsy = c_go[0] * c_sh * c_s + c_go[1] * c_sh * c_c + c_go[3] * c_s + c_go[4] * c_c
        gsh = go[0] * sy * s + go[1] * sy * c
        a_gsh = c_go[0] * c_sy * c_s + c_go[1] * c_sy * c_c
    if not sim:
        gsx = go[0] * c - go[1] * s
        a_gsx = c_go[0] * c_c + c_go[1] * c_s
        gth = go[0] * (-sx * s + sh * sy * c) + go[1] * (-sx * c - sh * sy * s) + \
            go[3] * sy * c - go[4] * sy * s
        a_gth = c_go[0] * (c_sx * c_s + c_sh * c_sy * c_c) + \
            c_go[1] * (c_sx * c_c + c_sh * c_sy * c_s) + c_go[3] * c_sy * c_c + \
            c_go[4] * c_sy * c_s
    gp = [gsx * x["dsx"], gsy * x["dsy"], gth * K.two_pi, gsh * x["dsh"], go[2] * x["dtx"],
          go[5] * x["dty"]]
    c_gp = [a_gsx * x["c_dsx"], a_gsy * x["c_dsy"], a_gth * K.two_pi, a_gsh * x["c_dsh"],
            c_go[2] * x["c_dtx"], c_go[5] * x["c_dty"]]
    return torch.stack(torch.broadcast_tensors(*gp), -1), \
        torch.stack(torch.broadcast_tensors(*c_gp), -1)


def _pieces(ins, mut=frozenset(), K=K32, noise=True):
    """what forward and backward share"""
    ap = _d(ins["all_param"])
    B, O, A = ap.shape
    V = (A - 7) // 8
    assert A == 8 * V + 7
    sim, lvs, adef = (bool(ins[k]) for k in ("similarity", "learn_vote_scale",
                                             "allow_deformations"))
    ns = float(ins["noise_scale"])

    def per_o(t, *shape):
        t = _d(t).reshape(O, *shape)
        if "bias_div" in mut:     # the row of capsule (b O + o) / O = b, not of (b O + o) % O
            return t[torch.arange(B) % O].unsqueeze(1).expand(B, O, *shape)
        return t.unsqueeze(0).expand(B, O, *shape)
    cpr_static = _d(ins["cpr_static"]).reshape(1, O, V, 6)
    b_cvr, b_caps = per_o(ins["bias_cvr"], 1, 6), per_o(ins["bias_caps"])
    b_vote, b_scale = per_o(ins["bias_vote"], V), per_o(ins["bias_scale"], V)
    dyn = ap[..., :6 * V].reshape(B, O, V, 6)
    if not adef:
        dyn = torch.zeros_like(dyn)
    pr, c_pr = dyn + cpr_static, dyn.abs() + cpr_static.abs()
    cv_in = ap[..., 6 * V:6 * V + 6].reshape(B, O, 1, 6)
    cv, c_cv = cv_in + b_cvr, cv_in.abs() + b_cvr.abs()
    P, C = _xf(pr, c_pr, sim, K), _xf(cv, c_cv, sim, K)
    lc_in, lv_in = ap[..., 6 * V + 6], ap[..., 6 * V + 7:7 * V + 7]
    lc, c_lc = lc_in + b_caps, lc_in.abs() + b_caps.abs()
    lv, c_lv = lv_in + b_vote, lv_in.abs() + b_vote.abs()
    if noise and ins.get("noise_caps") is not None:
        n = _d(ins["noise_caps"]).reshape(B, O)
        lc, c_lc = lc + (n - 0.5) * ns, c_lc + (n.abs() + 0.5) * abs(ns)
    if noise and ins.get("noise_vote") is not None:
        n = _d(ins["noise_vote"]).reshape(B, O, V)
        lv, c_lv = lv + (n - 0.5) * ns, c_lv + (n.abs() + 0.5) * abs(ns)
    pc, c_pc = _sig(lc, c_lc)
    pv, c_pv = _sig(lv, c_lv)
    sc_in = ap[..., 7 * V + 7:]
    sx, c_sx = sc_in + b_scale + .5, sc_in.abs() + b_scale.abs() + .5
    return dict(ap=ap, B=B, O=O, V=V, A=A, sim=sim, lvs=lvs, adef=adef, dyn=dyn, P=P, C=C, lc=lc,
                c_lc=c_lc, lv=lv, c_lv=c_lv, pc=pc, c_pc=c_pc, pv=pv, c_pv=c_pv, sx=sx,
                c_sx=c_sx)


def _argmax(vp, mut=frozenset()):
    """the first maximiser over the last dim (the mutants': the last one / the one in the
    lowest lane of a 16- or 64-lane stride loop)"""
    V = vp.shape[-1]
    idx = torch.arange(V).expand_as(vp)
    hit = vp == vp.max(-1, keepdim=True)[0]
    if "last_max" in mut:
        return torch.where(hit, idx, torch.full_like(idx, -1)).max(-1)[0]
    key = idx
    for name, n in (("lane_ties16", 16), ("lane_ties64", 64)):
        if name in mut:
            key = (idx % n) * V + idx
    best = torch.where(hit, key, torch.full_like(idx, V * V + V)).min(-1)[0]
    return best % V if key is not idx else best


def _forward(ins, mut=frozenset(), K=K32):
    p = _pieces(ins, mut, K)
    B, O, V, P, C = p["B"], p["O"], p["V"], p["P"], p["C"]
    Co, Po, cC, cP = C["o"], P["o"], C["c_o"], P["c_o"]
    vote = torch.stack([
        Co[0] * Po[0] + Co[1] * Po[3], Co[0] * Po[1] + Co[1] * Po[4],
        Co[0] * Po[2] + Co[1] * Po[5] + Co[2],
        Co[3] * Po[0] + Co[4] * Po[3], Co[3] * Po[1] + Co[4] * Po[4],
        Co[3] * Po[2] + Co[4] * Po[5] + Co[5]], -1)
    s_vote = torch.stack([
        cC[0] * cP[0] + cC[1] * cP[3], cC[0] * cP[1] + cC[1] * cP[4],
        cC[0] * cP[2] + cC[1] * cP[5] + cC[2],
        cC[3] * cP[0] + cC[4] * cP[3], cC[3] * cP[1] + cC[4] * cP[4],
        cC[3] * cP[2] + cC[4] * cP[5] + cC[5]], -1)
    vp = p["pc"].unsqueeze(-1) * p["pv"]
    s_vp = p["c_pc"].unsqueeze(-1) * p["c_pv"] + FLOOR
    if p["lvs"]:
        x, cx = p["sx"], p["c_sx"]
        soft = torch.where(x > 20, x, torch.log1p(torch.exp(x.clamp_max(20))))
        scale = soft + K.off
        s_scale = torch.where(x > 20, cx, soft + torch.sigmoid(x) * cx) + K.off + FLOOR
    else:
        scale, s_scale = torch.ones(B, O, V, dtype=torch.float64), torch.zeros(B, O, V).double()
    terms = (p["dyn"] ** 2).sum(-1)                                   # (B,O,V)
    keep = torch.ones(V, dtype=torch.float64)
    if "reg_tail16" in mut:
        keep[16 * (V // 16):] = 0
    if "reg_tail64" in mut:
        keep[64:] = 0
    arg = _argmax(vp, mut)
    res = dict(vote=vote, scale=scale, vote_presence=vp, logit_caps=p["lc"].unsqueeze(-1),
               logit_vote=p["lv"], reg_partial=(terms * keep).sum(-1),
               caps_presence=vp.gather(-1, arg.unsqueeze(-1)).squeeze(-1), caps_arg=arg)
    res["scale_of"] = dict(vote=s_vote, scale=s_scale, vote_presence=s_vp,
                        logit_caps=p["c_lc"].unsqueeze(-1), logit_vote=p["c_lv"],
                        reg_partial=terms.sum(-1), caps_presence=s_vp.gather(
                            -1, arg.unsqueeze(-1)).squeeze(-1))
    return res


def _backward(ins, grads, caps_arg=None, mut=frozenset(), K=K32):
    p = _pieces(ins, mut, K, noise="no_noise_bwd" not in mut)
    B, O, V, A, P, C, sim = p["B"], p["O"], p["V"], p["A"], p["P"], p["C"], p["sim"]
    g = {k: _d(grads.get(k)) for k in GRAD_NAMES}
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    gv = g["gvote"].reshape(B, O, V, 6) if g["gvote"] is not None else z(B, O, V, 6)
    gv, a_gv = [gv[..., k] for k in range(6)], [gv[..., k].abs() for k in range(6)]
    Co, Po, cC, cP = C["o"], P["o"], C["c_o"], P["c_o"]
    # per vote: its terms of the gradient on the capsule's pose matrix, and its own matrix's
    part = [gv[0] * Po[0] + gv[1] * Po[1] + gv[2] * Po[2],
            gv[0] * Po[3] + gv[1] * Po[4] + gv[2] * Po[5], gv[2],
            gv[3] * Po[0] + gv[4] * Po[1] + gv[5] * Po[2],
            gv[3] * Po[3] + gv[4] * Po[4] + gv[5] * Po[5], gv[5]]
    a_part = [a_gv[0] * cP[0] + a_gv[1] * cP[1] + a_gv[2] * cP[2],
              a_gv[0] * cP[3] + a_gv[1] * cP[4] + a_gv[2] * cP[5], a_gv[2],
              a_gv[3] * cP[0] + a_gv[4] * cP[1] + a_gv[5] * cP[2],
              a_gv[3] * cP[3] + a_gv[4] * cP[4] + a_gv[5] * cP[5], a_gv[5]]
    gP = [gv[0] * Co[0] + gv[3] * Co[3], gv[1] * Co[0] + gv[4] * Co[3],
          gv[2] * Co[0] + gv[5] * Co[3], gv[0] * Co[1] + gv[3] * Co[4],
          gv[1] * Co[1] + gv[4] * Co[4], gv[2] * Co[1] + gv[5] * Co[4]]
    a_gP = [a_gv[0] * cC[0] + a_gv[3] * cC[3], a_gv[1] * cC[0] + a_gv[4] * cC[3],
            a_gv[2] * cC[0] + a_gv[5] * cC[3], a_gv[0] * cC[1] + a_gv[3] * cC[4],
            a_gv[1] * cC[1] + a_gv[4] * cC[4], a_gv[2] * cC[1] + a_gv[5] * cC[4]]
    leak = "sim_leak" in mut
    gin, a_gin = _xf_backward(P, sim, gP, a_gP, K, leak)             # (B,O,V,6)
    reg_w = 0.0
    if g["greg"] is not None:
        reg_w = float(g["greg"]) if "reg_no_B" in mut else float(g["greg"]) / B
    if p["adef"]:
        gdyn, a_gdyn = gin + reg_w * p["dyn"], a_gin + abs(reg_w) * p["dyn"].abs()
    else:
        gdyn, a_gdyn = z(B, O, V, 6), z(B, O, V, 6)
    g_vp = g["gvote_presence"].reshape(B, O, V) if g["gvote_presence"] is not None \
        else z(B, O, V)
    a_gvp = g_vp.abs()
    if g["gcaps_presence"] is not None and "no_gcaps" not in mut:
        arg = _forward(ins, K=K)["caps_arg"] if caps_arg is None else caps_arg.long().cpu()
        hot = z(B, O, V).scatter_(-1, arg.reshape(B, O, 1), 1.0)
        gcp = g["gcaps_presence"].reshape(B, O, 1)
        g_vp, a_gvp = g_vp + hot * gcp, a_gvp + hot * gcp.abs()
    pc, c_pc, pv, c_pv = p["pc"].unsqueeze(-1), p["c_pc"].unsqueeze(-1), p["pv"], p["c_pv"]
    keep = torch.ones(V, dtype=torch.float64)
    if "quarter" in mut:
        keep[3::4] = 0
    gC = [(t * keep).sum(-1, keepdim=True) for t in part]           # sums over the votes
    a_gC = [t.sum(-1, keepdim=True) for t in a_part]
    gpc = (g_vp * pv * keep).sum(-1)
    a_gpc = (a_gvp * c_pv).sum(-1)
    g_lv = g_vp * pc * pv * torch.sigmoid(-p["lv"])
    a_glv = a_gvp * c_pc * c_pv * (1 + c_pv)
    if g["glogit_vote"] is not None:
        t = g["glogit_vote"].reshape(B, O, V)
        g_lv, a_glv = g_lv + t, a_glv + t.abs()
    g_sc, a_gsc = z(B, O, V), z(B, O, V)
    if p["lvs"] and g["gscale"] is not None:
        x, cx, t = p["sx"], p["c_sx"], g["gscale"].reshape(B, O, V)
        sg = torch.sigmoid(x)
        g_sc = t * torch.where(x > 20, torch.ones_like(x), sg)
        a_gsc = t.abs() * (torch.where(x > 20, torch.ones_like(x),
                                       sg + sg * torch.sigmoid(-x) * cx) + FLOOR)
    gcv, a_gcv = _xf_backward(C, sim, gC, a_gC, K, leak)            # (B,O,1,6)
    g_lc = gpc * p["pc"] * torch.sigmoid(-p["lc"])
    a_glc = a_gpc * p["c_pc"] * (1 + p["c_pc"])
    if g["glogit_caps"] is not None:
        t = g["glogit_caps"].reshape(B, O)
        g_lc, a_glc = g_lc + t, a_glc + t.abs()
    gall = torch.cat([gdyn.reshape(B, O, 6 * V), gcv.reshape(B, O, 6), g_lc.unsqueeze(-1),
                      g_lv, g_sc], -1)
    a_gall = torch.cat([a_gdyn.reshape(B, O, 6 * V), a_gcv.reshape(B, O, 6),
                        a_glc.unsqueeze(-1), a_glv, a_gsc], -1)
    assert gall.shape == (B, O, A)
    live = p["ap"] >= 0 if "gate_ge" in mut else p["ap"] > 0
    out = dict(gall_param=gall, gall_param_gated=gall * live, gcpr_in=gin)
    s = dict(gall_param=a_gall + FLOOR, gall_param_gated=(a_gall + FLOOR) * (p["ap"] > 0),
             gcpr_in=a_gin + FLOOR)
    # the parameter gradients: batch sums of gcpr_in and of column blocks of gall_param
    cols = dict(bias_cvr=(6 * V, 6 * V + 6, (1, O, 1, 6)), bias_caps=(6 * V + 6, 6 * V + 7,
                                                                       (1, O, 1)),
                bias_vote=(6 * V + 7, 7 * V + 7, (1, O, V)), bias_scale=(7 * V + 7, A, (1, O, V)))
    out["cpr_static"], s["cpr_static"] = gin.sum(0, keepdim=True), s["gcpr_in"].sum(0, keepdim=True)
    for k, (lo, hi, shape) in cols.items():
        out[k] = gall[..., lo:hi].sum(0).reshape(shape)
        s[k] = s["gall_param"][..., lo:hi].sum(0).reshape(shape)
    out["scale_of"] = s
    return out


def forward(ins):
    """``ins``: all_param (B,O,8V+7), cpr_static (1,O,V,6), bias_cvr (1,O,1,6), bias_caps
    (1,O,1), bias_vote / bias_scale (1,O,V), noise_caps (B,O,1) / noise_vote (B,O,V) or
    None, noise_scale, similarity, learn_vote_scale, allow_deformations.  -> vote (B,O,V,6),
    scale, vote_presence, logit_caps (B,O,1), logit_vote, reg_partial (B,O), caps_presence,
    caps_arg (int64), and ``scale_of``: the companion magnitude of every float entry."""
    return _forward(ins)


def backward(ins, grads, caps_arg=None):
    """``grads``: any subset of GRAD_NAMES -> tensor (absent or None: no gradient).
    -> gall_param, gall_param_gated (zero where all_param <= 0), gcpr_in, the parameter
    gradients (PARAM_NAMES: their batch sums) and ``scale_of``: the companions.
    ``caps_arg``: where the caps_presence gradient goes (None: this reference's own)."""
    return _backward(ins, grads, caps_arg)


def presence_gap(res):
    """best minus second-best fp64 vote presence per capsule ((B,O); inf at V = 1)"""
    vp = res["vote_presence"]
    if vp.shape[-1] == 1:
        return torch.full_like(vp[..., 0], math.inf)
    top = vp.topk(2, dim=-1)[0]
    return top[..., 0] - top[..., 1]


def presence_bar(res):
    """(B,O): 2 C_OUT 2^-24 of the largest companion among a capsule's vote presences --
    above it two fp32 presences, each within the bar, keep their fp64 order"""
    return 2 * C_OUT * U * res["scale_of"]["vote_presence"].max(-1)[0]


# ------------------------------------------------------------------------------------ cases
REGIMES = ("benign", "saturated", "relu", "wrap", "ties")
NOISE_SCALE = 4.0


def tie_groups(V):
    """the planted groups of tied votes (their lowest member is the expected arg-max):
    adjacent across a 16-lane boundary, 16 apart, 64 apart and across 64 where V allows,
    each kind also with the last vote; pairs and triples"""
    out = []
    if V > 16:
        out += [(0, 16, V - 1), (15, 16), (1, 17)]
    if V > 64:
        out += [(63, 64), (0, 64), (5, 21, V - 1)]
    if V >= 4:
        out += [(2, 3), (V - 2, V - 1), (0, V - 1), (1, 2, V - 1)]
    return [g for g in out if len(set(g)) == len(g) and max(g) < V]


def _seed(regime, B, O, V):
    return REGIMES.index(regime) * 1000003 + B * 10007 + O * 101 + V


def make_case(regime, B, O, V, sim=True, lvs=True, adef=True, noise="both", reseed=0):
    """-> (ins: fp32 tensors and the flags, meta).  meta["tie"] (B,O) int64: the lowest vote
    of a planted group of bit-identical vote logits that is the capsule's maximum, or -1."""
    g = torch.Generator().manual_seed(_seed(regime, B, O, V) + 7919 * reseed)
    r = lambda *s: torch.rand(*s, generator=g)     # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g)    # noqa: E731
    A = 8 * V + 7
    ap = n(B, O, A)
    cpr, b_cvr = n(1, O, V, 6) * 0.3, n(1, O, 1, 6) * 0.3
    b_caps, b_vote, b_scale = n(1, O, 1), n(1, O, V), n(1, O, V)
    n_caps, n_vote = r(B, O, 1), r(B, O, V)
    tie = torch.full((B, O), -1, dtype=torch.int64)
    pm = lambda *s: torch.sign(n(*s))              # noqa: E731
    if regime == "saturated":
        # the magnitudes sit in the biases, so that they survive a ReLU in front of
        # all_param; one vote per capsule is on, the others off -- except in the capsules
        # (b O + o) % 23 == 22, where three are (sigmoids that are all exactly 1 in fp32), and
        # (b O + o) % 29 == 28, whose capsule presence is exactly 0 in fp32: every vote ties
        b_cvr = pm(1, O, 1, 6) * (2 + 28 * r(1, O, 1, 6))
        cpr = pm(1, O, V, 6) * (2 + 28 * r(1, O, V, 6))
        b_cvr[..., 2], cpr[..., 2] = n(1, O, 1), n(1, O, V)          # (theta: not here)
        b_caps = pm(1, O, 1) * (30 + 45 * r(1, O, 1))
        b_caps[0, 0, 0] = 45.0
        if O > 1:
            b_caps[0, 1, 0] = -35.0
        b_vote = -(30 + 70 * r(1, O, V))
        b_vote[0, 0, 0] = -100.0                      # expf overflows: a sigmoid of exactly 0
        for o in range(O):
            b_vote[0, o, (3 * o + 1) % V] = 30 + 70 * float(r(1))
        kind = torch.randint(0, 3, (1, O, V), generator=g)
        b_scale = torch.where(kind == 0, torch.full((1, O, V), 19.0),     # both sides of 20
                              torch.where(kind == 1, -(100.5 + 20 * r(1, O, V)), b_scale))
        ap = ap * 2
        for bo in range(B * O):
            b, o = divmod(bo, O)
            if bo % 23 == 22:
                ap[b, o, 6 * V + 7 + (o + 2) % V] = 200.0
                ap[b, o, 6 * V + 7 + V - 1] = 200.0
            if bo % 29 == 28:
                ap[b, o, 6 * V + 6] = -200.0
    elif regime == "relu":
        ap = torch.where(r(B, O, A) < 0.5, torch.zeros(B, O, A), ap)
    elif regime == "wrap":
        for t in (cpr, b_cvr):
            t[..., 2] = (r(*t.shape[:-1]) * 2 - 1) * 25
        th = (r(B, O, V + 1) * 2 - 1) * 25
        ap[..., 2:6 * V:6] = th[..., :V]
        ap[..., 6 * V + 2] = th[..., V]
    elif regime == "ties":
        groups = tie_groups(V)
        assert groups, V
        lv_col = 6 * V + 7
        for b in range(B):
            for o in range(O):
                if (b + o) % 5 == 4:
                    continue                                         # some capsules stay plain
                grp = groups[(b * O + o) % len(groups)]
                lo = grp[0]
                ap[b, o, lv_col + lo] = 12.0                         # above every other logit
                for hi in grp[1:]:
                    ap[b, o, lv_col + hi] = ap[b, o, lv_col + lo]
                    n_vote[b, o, hi] = n_vote[b, o, lo]
                tie[b, o] = lo
        # the same bias for every vote a group may hold
        b_vote[0, :, sorted({v for grp in groups for v in grp})] = 0.25
    elif regime != "benign":
        raise ValueError(regime)
    ins = dict(all_param=ap.contiguous(), cpr_static=cpr, bias_cvr=b_cvr, bias_caps=b_caps,
               bias_vote=b_vote, bias_scale=b_scale,
               noise_caps=n_caps if noise in ("both", "caps") else None,
               noise_vote=n_vote if noise in ("both", "vote") else None,
               noise_scale=NOISE_SCALE, similarity=int(sim), learn_vote_scale=int(lvs),
               allow_deformations=int(adef))
    return ins, dict(tie=tie, regime=regime, shape=(B, O, V))


def clear(res):
    """(B,O) bool: the fp64 gap between best and second best exceeds ``presence_bar``"""
    return presence_gap(res) > presence_bar(res)


def well_separated(ins, meta):
    """outside the planted ties at least 90 % of the capsules are ``clear``"""
    plain = meta["tie"] < 0
    if not bool(plain.any()):
        return True
    return float(clear(forward(ins))[plain].double().mean()) >= 0.9


def checked_case(regime, B, O, V, sim=True, lvs=True, adef=True, noise="both"):
    """``make_case``, reseeded until ``well_separated`` holds."""
    for k in range(20):
        ins, meta = make_case(regime, B, O, V, sim, lvs, adef, noise, reseed=k)
        if well_separated(ins, meta):
            meta["reseed"] = k
            return ins, meta
    raise AssertionError(("no well separated draw", regime, B, O, V))


def relu_case(ins):
    """the case as a one-layer identity chain hands it to the votes: all_param = relu(x)"""
    return dict(ins, all_param=torch.relu(ins["all_param"]))


def make_grads(B, O, V, seed=0):
    """the seven incoming gradients, seeded (fp32)"""
    g = torch.Generator().manual_seed(4242 + seed + B * 31 + O * 7 + V)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(gvote=n(B, O, V, 6), gscale=n(B, O, V), gvote_presence=n(B, O, V),
                glogit_caps=n(B, O, 1), glogit_vote=n(B, O, V), greg=n(()),
                gcaps_presence=n(B, O))


def subsets(grads):
    return [(k, {k: grads[k]}) for k in GRAD_NAMES] + [("all", dict(grads))]


V_MAX = (704 - 7) // 8     # the largest V with 8 V + 7 <= scae_mlp_chain_max_width()
SHAPES = [(5, 3, 1), (17, 5, 7), (33, 2, 17), (3, 2, 65), (37, 6, 24), (2, 1, V_MAX)]
FLAG_SHAPE = (17, 5, 7)
REGIME_SHAPES = dict(saturated=[(17, 5, 7), (3, 2, 65), (37, 6, 24)],
                     relu=[(17, 5, 7), (33, 2, 17), (37, 6, 24)],
                     wrap=[(17, 5, 7), (3, 2, 65)],
                     ties=[(17, 5, 7), (33, 2, 17), (3, 2, 65), (37, 6, 24), (2, 1, V_MAX)])


def all_cases():
    """(regime, B, O, V, similarity, learn_vote_scale, allow_deformations, noise) of every
    case the GPU module runs"""
    out = [("benign", *s, i % 2, 1, 1, "both") for i, s in enumerate(SHAPES)]
    out += [("benign", *FLAG_SHAPE, sim, lvs, adef, "both")
            for sim in (0, 1) for lvs in (0, 1) for adef in (0, 1)
            if (sim, lvs, adef) != (1, 1, 1)]
    out += [("benign", *FLAG_SHAPE, 1, 1, 1, nz) for nz in ("caps", "vote", "none")]
    for regime, shapes in REGIME_SHAPES.items():
        out += [(regime, *s, (i + 1) % 2, 1, 1, "both") for i, s in enumerate(shapes)]
    out += [("saturated", *FLAG_SHAPE, 0, 0, 0, "none"), ("relu", *FLAG_SHAPE, 0, 1, 0, "both")]
    return out


def case_id(c):
    flags = ("s" if c[4] else "a") + ("l" if c[5] else "-") + ("d" if c[6] else "-")
    return f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-{flags}-{c[7]}"
