"""fp64 reference of the part-capsule head (K9: csrc/attention_pool.hip -- 1x1 attention
conv, softmax pooling over pixels, split, noise, sigmoid and pose non-linearity -- in its
pool-only form, its form from a given y and its fused conv forms) and of the coloured
templates (K10: csrc/template_color.hip) that also says how far an fp32 evaluation may be
from it.  CPU only; no GPU import.

``forward`` restates part_encoder.py:70-92 in fp64: ``y = x w^T + b``, per capsule a
``mask = softmax over pixels of y[.., a P + P - 1]``, ``pooled`` (B,A,P-1), and -- the head --
``pose = geometric_transform(pooled[..., :6])`` (``votes_ref._xf``, which carries the
companions), ``presence = sigmoid(pooled[..., 6] + (u - .5) scale)``, ``absence = 1 -
presence`` and ``feature = pooled[..., 7:]``.  ``ins`` without ``x`` starts from a given
``y``; ``head=False`` is the pool-only form (P >= 2).  ``backward`` is hand-written, for any
subset of (g_pose, g_presence, g_feature, g_feature2) or ``g`` of the pool-only form, and
returns dy and, through the conv, dx, dw and db.  ``tc_forward`` / ``tc_backward`` restate
TemplateGenerator.forward (part_decoder.py:78-110) and its backward: raw, color and
templates from the template logits and the colour MLP [F, H1, C] (ReLU after both layers),
both non-linearities for templates and colour, relu1 evaluated as written (relu6(6 x) / 6);
g_logits (with and without g_raw), g_feature and the batch sums dW1, db1, dW2, db2.  The
constants are the fp32 values the fp32 oracle and the kernels hold (``K32``: 2 pi, 1e-2 and
the colour's .99 rounded to fp32); with ``K64`` the reference equals the fp64 oracle to 1e-12.

Every float entry comes with a companion magnitude (``res["scale_of"][name]``): the same
formula with every summand replaced by its absolute value and every function value f(x) by
|f(x)| + |f'(x)| * companion(x) -- exp(l - mx) has e (1 + c_l + c_mx), a mask e / s has
c_e / s + m c_s / s, the softmax-backward term m (t - sa) has c_m (c_t + c_sa) with c_sa =
sum c_m c_t, so that the cancellation at saturation is accounted for; ``FLOOR`` (lk_ref's) is
added for what an underflow loses.  A bound is then, entry by entry,

    |fp32 - fp64| <= c * 2^-24 * scale

Measured (tests/test_head_ref.py::test_constants_come_from_the_fp32_oracle re-measures and
prints them): the fp32 oracle on the CPU (F.conv2d + multiple_attention_pooling_2d +
geometric_transform + sigmoid with autograd for K9, from x and from the given y;
template_generator for K10) against this reference, worst |fp32 - fp64| / (2^-24 scale) over
every case of tests/test_capsule_head_vs_fp64.py:

    K9  outputs    pooled 1.17  pose 0.74  presence 1.08  absence 0.63  feature 1.17
        gradients  dy 4.21   (through the conv: dx 0.61  dw 1.15  db 15.1)
        (gradients: each incoming gradient alone, g_feature + g_feature2, all four; g of the
        pool-only form)
    K10 outputs    raw 1.85  color 1.57  templates 3.51
        gradients  g_logits 2.90  g_feature 1.79   (with and without g_raw)
        batch sums dW1 1.53  db1 1.01  dW2 1.04  db2 0.85

    C_OUT = 5 (4 x 1.17 = 4.7, rounded up to one digit)   C_GRAD = 20 (4 x 4.21 = 16.9)
    TC_C_OUT = 20 (4 x 3.51 = 14.1)   TC_C_GRAD = 20 (4 x 2.90 = 11.6)

The conv's own output y is not held by a measured constant but by ``y_bound``: gamma(C + 1) of
its companion, whatever the summation order (the fp32 oracle's own y is 15.5 x 2^-24 of the
companion off at C = 256).  dx, dw and db are left out of C_GRAD: they are n-term GEMM sums,
whose error is the summation's (gamma(n) of the summed |terms|), not the head's, and their
from-x companions compound through the conv, the exponential and the softmax backward until
they exceed the values themselves -- a bound from them sees neither a zeroed nor a doubled
gradient.  The op-level test therefore runs on ``exact_conv`` cases, whose conv is exact in
fp32 in any summation order, takes dy and its sharp companions from the from-y reference
(c_y = |y|) and pushes them through the conv (``conv_backward``): C_GRAD 2^-24 of the pushed
companions plus gamma(n) of the summed |terms|.  test_head_ref.py shows per (shape, loss,
tensor) that a zeroed, a doubled and a misrouted gradient exceed that bar and that the fp32
oracle stays within it.  K10's batch sums over B M terms add gamma(n) the same way.

The factor 4 is for what the kernels do differently from the oracle: MFMA, lane-tree and fma
summation orders instead of torch's sums, and a device expf of a couple of ulp where the
host's is one.  c is never tuned against a kernel.

``_forward`` / ``_backward`` / ``_tc_forward`` / ``_tc_backward`` take a set of mutant names
(``MUTANTS``): each plants one mistake of the kind the lane arithmetic invites, for
test_head_ref.py to show that the bar and the cases see it.  The mutants that drop the
softmax's maximum evaluate their exponentials in fp32, where they overflow.  ``raw_from_b1``
changes no value -- raw does not depend on the image -- except that at B = 1 nobody writes raw
(NaN here, the sentinels on the device): it shows that the list has a B = 1 case, not that the
bar sees a wrong raw; that is ``group_m0``'s part.
"""
import collections
import math

import numpy as np
import torch

from tests.lk_ref import FLOOR, U, gamma, ratio  # noqa: F401  (re-exported)
from tests.votes_ref import _sig, _xf, _xf_backward

C_OUT = 5.0
C_GRAD = 20.0
TC_C_OUT = 20.0
TC_C_GRAD = 20.0
Consts = collections.namedtuple("Consts", "two_pi off c99")
K32 = Consts(float(np.float32(2 * math.pi)), float(np.float32(1e-2)), float(np.float32(.99)))
K64 = Consts(2 * math.pi, 1e-2, .99)

GRAD_NAMES = ("g_pose", "g_presence", "g_feature", "g_feature2")
HEAD_OUTS = ("pooled", "pose", "presence", "absence", "feature")
CONV_GRADS = ("dx", "dw", "db")
TC_OUTS = ("raw", "color", "templates")
TC_GRADS = ("g_logits", "g_feature")
TC_SUMS = ("dW1", "db1", "dW2", "db2")
K9_MUTANTS = ("max16", "no_max", "one_trip", "pix32", "sa_half", "logit_col", "no_noise_bwd",
              "gf2_dropped", "absence_from_logit")
K10_MUTANTS = ("colour_window_unshifted", "relu1_ge", "h1_gate_pre", "bwdB_per", "raw_from_b1",
               "group_m0")
MUTANTS = K9_MUTANTS + K10_MUTANTS


def _d(t):
    return None if t is None else t.detach().double().cpu()


def y_bound(c_y, C):
    """the conv output against the fp64 conv: gamma(C + 1) of sum |x| |w| + |b| -- what C
    products and a bias may lose in ANY summation order (an MFMA chain, a GEMM's k-split), so
    no measured constant.  (A logit of 40 + 255 small terms is 15 x 2^-24 of its companion off
    in the fp32 oracle itself: each small addition rounds at the ulp of 40.)"""
    return gamma(C + 1) * c_y


def groups(B, A):
    """capsule groups per image (``pool_splits`` / ``tc_splits``): the largest divisor of A up
    to 8, or the first one with B d >= 512.  The GPU module asserts it against the library's
    own answer for every case."""
    s = 1
    for d in range(1, min(A, 8) + 1):
        if A % d == 0:
            s = d
            if B * d >= 512:
                break
    return s


# ------------------------------------------------------------------------------------- K9
def _pieces(ins, mut=frozenset(), K=K32, noise=True):
    """what forward and backward share: y, the masks, pooled and the head's values"""
    A = int(ins["A"])
    if ins.get("x") is not None:
        x, w = _d(ins["x"]), _d(ins["w"])
        b = _d(ins["bias"]) if ins.get("bias") is not None else torch.zeros(w.shape[0]).double()
        y, c_y = x @ w.t() + b, x.abs() @ w.abs().t() + b.abs()
    else:
        y = _d(ins["y"])
        c_y = y.abs()
    B, HW, AP = y.shape
    P = AP // A
    assert AP == A * P and P >= 2
    Ag = A // groups(B, A)
    y4, c_y4 = y.view(B, HW, A, P), c_y.view(B, HW, A, P)
    col = P - 2 if "logit_col" in mut else P - 1
    l, c_l = y4[..., col], c_y4[..., col]                              # (B,HW,A)
    pix = torch.arange(HW).view(1, HW, 1)
    live = (pix < 32) if "pix32" in mut else torch.ones(1, HW, 1, dtype=torch.bool)
    inmax = live & (pix % 32 < 16) if "max16" in mut else live
    mx, arg = torch.where(inmax, l, torch.full_like(l, -math.inf)).max(1, keepdim=True)
    c_mx = c_l.gather(1, arg)
    if "no_max" in mut:
        mx = torch.zeros_like(mx)
    d = l - mx
    e = torch.exp(d.float()).double() if mut & {"max16", "no_max"} else torch.exp(d)
    e = e * live
    s = e.sum(1, keepdim=True)
    m = e / s
    c_e = e * (1 + c_l + c_mx)
    c_m = c_e / s + m * c_e.sum(1, keepdim=True) / s + FLOOR
    if "one_trip" in mut:
        m = m * (torch.arange(A) % Ag < 16)
    pooled = (y4[..., :P - 1] * m.unsqueeze(-1)).sum(1)                # (B,A,P-1)
    c_pooled = (c_y4[..., :P - 1] * c_m.unsqueeze(-1)).sum(1) + FLOOR
    p = dict(B=B, HW=HW, A=A, P=P, y=y, c_y=c_y, y4=y4, c_y4=c_y4, m=m, c_m=c_m, pooled=pooled,
             c_pooled=c_pooled, head=bool(ins.get("head", True)))
    if not p["head"]:
        return p
    assert P >= 8
    p["sim"] = bool(ins["similarity"])
    p["X"] = _xf(pooled[..., :6], c_pooled[..., :6], p["sim"], K)
    lg, c_lg = pooled[..., 6], c_pooled[..., 6]
    p["logit_clean"] = lg
    if noise and ins.get("noise_u") is not None:
        ns, u = float(ins["noise_scale"]), _d(ins["noise_u"])
        lg, c_lg = lg + (u - .5) * ns, c_lg + (u.abs() + .5) * abs(ns)
    p["logit"], p["c_logit"] = lg, c_lg
    p["pr"], p["c_pr"] = _sig(lg, c_lg)
    return p


def _forward(ins, mut=frozenset(), K=K32):
    p = _pieces(ins, mut, K)
    res = dict(y=p["y"], mask=p["m"], pooled=p["pooled"])
    s = dict(y=p["c_y"], mask=p["c_m"], pooled=p["c_pooled"])
    if p["head"]:
        X = p["X"]
        res["pose"] = torch.stack(torch.broadcast_tensors(*X["o"]), -1)
        s["pose"] = torch.stack(torch.broadcast_tensors(*X["c_o"]), -1)
        res["presence"], s["presence"] = p["pr"], p["c_pr"]
        res["absence"], s["absence"] = 1 - p["pr"], 1 + p["c_pr"]
        if "absence_from_logit" in mut:
            res["absence"] = 1 - torch.sigmoid(p["logit_clean"])
        res["feature"], s["feature"] = p["pooled"][..., 7:], p["c_pooled"][..., 7:]
    res["scale_of"] = s
    return res


def _backward(ins, grads, mut=frozenset(), K=K32):
    p = _pieces(ins, mut, K, noise="no_noise_bwd" not in mut)
    B, HW, A, P = p["B"], p["HW"], p["A"], p["P"]
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    if p["head"]:
        g = {k: _d(grads.get(k)) for k in GRAD_NAMES}
        gpo = g["g_pose"] if g["g_pose"] is not None else z(B, A, 6)
        go, c_go = [gpo[..., k] for k in range(6)], [gpo[..., k].abs() for k in range(6)]
        gp, c_gp = _xf_backward(p["X"], p["sim"], go, c_go, K)
        gpr = g["g_presence"] if g["g_presence"] is not None else z(B, A)
        g6 = gpr * p["pr"] * torch.sigmoid(-p["logit"])
        c_g6 = gpr.abs() * p["c_pr"] * (1 + p["c_pr"])
        gf, c_gf = z(B, A, P - 8), z(B, A, P - 8)
        for k in ("g_feature", "g_feature2"):
            if g[k] is None or (k == "g_feature2" and "gf2_dropped" in mut):
                continue
            gf, c_gf = gf + g[k], c_gf + g[k].abs()
        gs = torch.cat([gp, g6.unsqueeze(-1), gf], -1)
        c_gs = torch.cat([c_gp, c_g6.unsqueeze(-1), c_gf], -1)
    else:
        gs = _d(grads["g"])
        c_gs = gs.abs()
    y4, c_y4, m, c_m = p["y4"], p["c_y4"], p["m"], p["c_m"]
    t = (gs.unsqueeze(1) * y4[..., :P - 1]).sum(-1)                    # (B,HW,A)
    c_t = (c_gs.unsqueeze(1) * c_y4[..., :P - 1]).sum(-1)
    keep = torch.ones(1, HW, 1, dtype=torch.float64)
    if "sa_half" in mut:
        keep = (torch.arange(HW).view(1, HW, 1) % 32 < 16).double()
    sa, c_sa = (m * t * keep).sum(1, keepdim=True), (c_m * c_t).sum(1, keepdim=True)
    dy4 = torch.cat([gs.unsqueeze(1) * m.unsqueeze(-1), (m * (t - sa)).unsqueeze(-1)], -1)
    c_dy4 = torch.cat([c_gs.unsqueeze(1) * c_m.unsqueeze(-1),
                       (c_m * (c_t + c_sa)).unsqueeze(-1)], -1) + FLOOR
    dy, c_dy = dy4.reshape(B, HW, A * P), c_dy4.reshape(B, HW, A * P)
    out, s = dict(dy=dy), dict(dy=c_dy)
    if ins.get("x") is not None:
        x, w = _d(ins["x"]), _d(ins["w"])
        out["dx"], s["dx"] = dy @ w, c_dy @ w.abs()
        out["dw"] = torch.einsum("bhk,bhc->kc", dy, x)
        s["dw"] = torch.einsum("bhk,bhc->kc", c_dy, x.abs())
        out["db"], s["db"] = dy.sum((0, 1)), c_dy.sum((0, 1))
    out["scale_of"] = s
    return out


def forward(ins):
    """``ins``: x (B,HW,C), w (A P,C), bias -- or y (B,HW,A P) --, A, noise_u (B,A) or None,
    noise_scale, similarity, head (False: the pool-only form).  -> y, mask (B,HW,A), pooled
    (B,A,P-1), pose (B,A,6), presence, absence (B,A), feature (B,A,P-8) and ``scale_of``: the
    companion magnitude of every entry."""
    return _forward(ins)


def backward(ins, grads):
    """``grads``: any subset of GRAD_NAMES (absent or None: no gradient), or ``g`` (B,A,P-1)
    of the pool-only form.  -> dy (B,HW,A P), with ``x`` in ``ins`` also dx, dw, db, and
    ``scale_of``."""
    return _backward(ins, grads)


def from_y(ins):
    """the case from the y an exact conv rounded to fp32 hands over"""
    y = _forward(ins)["y"].float()
    return {k: v for k, v in dict(ins, y=y).items() if k not in ("x", "w", "bias")}


def exact_conv(ins):
    """the case with x on a grid of 1/8 in [-4, 4], w of 1/64 in [-.5, .5] and the bias of
    1/512 in [-4, 4]: every product is a multiple of 1/512 and every partial sum stays below
    2^24 / 512, so the conv is exact in fp32 in ANY summation order (and every operand has at
    most 6 significant bits: exact in a bf16 split, too).  The y an op computes for itself is
    then the fp64 y, bit for bit, and the sharp from-y reference applies at the op level."""
    x = (ins["x"] * 8).round().clamp(-32, 32) / 8
    w = (ins["w"] * 64).round().clamp(-32, 32) / 64
    b = (ins["bias"] * 512).round().clamp(-2048, 2048) / 512
    assert (x.shape[-1] * 4 * 0.5 + 4) * 512 < 2 ** 24
    return dict(ins, x=x, w=w, bias=b)


def conv_backward(res, x, w):
    """dy of ``backward`` (from a given y) pushed through the 1x1 conv -> (dx, dw, db, and
    ``bound``: per entry C_GRAD 2^-24 of dy's companions pushed through the same sums, plus
    gamma(n) of the summed |terms| for the n-term sum itself, n = A P for dx and B HW for dw
    and db -- any summation order)"""
    dy, c_dy, x, w = res["dy"], res["scale_of"]["dy"], _d(x), _d(w)
    B, HW, AP = dy.shape
    out = dict(dx=dy @ w, dw=torch.einsum("bhk,bhc->kc", dy, x), db=dy.sum((0, 1)))
    comp = dict(dx=c_dy @ w.abs(), dw=torch.einsum("bhk,bhc->kc", c_dy, x.abs()),
                db=c_dy.sum((0, 1)))
    parts = dict(dx=dy.abs() @ w.abs(), dw=torch.einsum("bhk,bhc->kc", dy.abs(), x.abs()),
                 db=dy.abs().sum((0, 1)))
    n = dict(dx=AP, dw=B * HW, db=B * HW)
    out["bound"] = {k: C_GRAD * U * comp[k] + gamma(n[k]) * parts[k] for k in comp}
    return out


# the op-level cases: ``exact_conv`` of these
OP_SHAPES = [("benign", 5, 16, 8, 9, 128), ("benign", 7, 33, 42, 9, 8)]


# ------------------------------------------------------------------------------------ K10
def _relu1(x):
    return (x * 6).clamp(0, 6) / 6


def _nonlin(x, c_x, kind):
    """-> (f, companion, f', companion of f')"""
    if kind == 0:
        s, c_s = _sig(x, c_x)
        return s, c_s, s * torch.sigmoid(-x), s * (1 + s) + (c_s - s)
    inside = ((x > 0) & (x < 1)).double()
    return _relu1(x), torch.where(x >= 1, torch.ones_like(x), c_x * inside), inside, inside


def _tc_pieces(ins, mut=frozenset(), K=K32):
    lg, ft = _d(ins["logits"]), _d(ins["feature"])
    w1, b1, w2, b2 = (_d(ins[k]) for k in ("w1", "b1", "w2", "b2"))
    tnl, cnl = int(ins["tnl"]), int(ins["cnl"])
    B, M, F = ft.shape
    s1, c_s1 = ft @ w1.t() + b1, ft.abs() @ w1.abs().t() + b1.abs()    # (B,M,H1)
    on1 = s1 > 0
    h1, c_h1 = s1 * on1, c_s1 * on1
    pre2, c_pre2 = h1 @ w2.t() + b2, c_h1 @ w2.abs().t() + b2.abs()    # (B,M,C)
    on2 = pre2 > 0
    r, c_r = pre2 * on2, c_pre2 * on2
    if cnl == 0:
        color, c_color, dcol, c_dcol = _nonlin(r, c_r, 0)
    else:
        zc = r + K.c99
        color = _relu1(zc)
        c_color = torch.where(zc >= 1, torch.ones_like(zc), c_r + K.c99)
        win = pre2 if "colour_window_unshifted" in mut else zc
        dcol = ((win >= 0) & (win <= 1) if "relu1_ge" in mut else (win > 0) & (win < 1)).double()
        c_dcol = dcol
    dcol, c_dcol = dcol * on2, c_dcol * on2
    raw, c_raw, draw, c_draw = _nonlin(lg, lg.abs(), tnl)
    if tnl == 1 and "relu1_ge" in mut:
        draw = ((lg >= 0) & (lg <= 1)).double()
    return dict(B=B, M=M, F=F, lg=lg, ft=ft, w1=w1, w2=w2, on1=on1, h1=h1, c_h1=c_h1, s1=s1,
                c_s1=c_s1, pre2=pre2, c_pre2=c_pre2, color=color, c_color=c_color + FLOOR,
                dcol=dcol, c_dcol=c_dcol, raw=raw, c_raw=c_raw + FLOOR * (c_raw > 0), draw=draw,
                c_draw=c_draw, cnl=cnl, tnl=tnl)


def _by_group(t, B, M, mut):
    """(M, ...) per-capsule rows as the workgroup of capsule m reads them (``group_m0``: the
    rows of the first group)"""
    if "group_m0" not in mut:
        return t
    return t[torch.arange(M) % (M // groups(B, M))]


def _tc_forward(ins, mut=frozenset(), K=K32):
    p = _tc_pieces(ins, mut, K)
    B, M = p["B"], p["M"]
    raw_used, c_raw_used = _by_group(p["raw"], B, M, mut), p["c_raw"]
    tm = raw_used.unsqueeze(0) * p["color"].unsqueeze(-1)
    raw = raw_used
    if "raw_from_b1" in mut and B < 2:
        raw = torch.full_like(raw, math.nan)            # (no image but the first: not written)
    return dict(raw=raw, color=p["color"], templates=tm, pre2=p["pre2"], s1=p["s1"],
                scale_of=dict(raw=c_raw_used, color=p["c_color"], pre2=p["c_pre2"], s1=p["c_s1"],
                              templates=c_raw_used.unsqueeze(0) * p["c_color"].unsqueeze(-1)))


def _tc_backward(ins, g_templates, g_raw=None, mut=frozenset(), K=K32):
    p = _tc_pieces(ins, mut, K)
    B, M = p["B"], p["M"]
    gt, gr = _d(g_templates), _d(g_raw)
    raw, c_raw = _by_group(p["raw"], B, M, mut), p["c_raw"]
    gc, c_gc = (gt * raw).sum(-1), (gt.abs() * c_raw).sum(-1)         # (B,M,C)
    g2, c_g2 = gc * p["dcol"], c_gc * p["c_dcol"]
    s = g2 @ p["w2"]
    gate = (s > 0) if "h1_gate_pre" in mut else p["on1"]
    g1, c_g1 = s * gate, (c_g2 @ p["w2"].abs()) * p["on1"]
    out = dict(g_feature=g1 @ p["w1"], dW1=torch.einsum("bmj,bmf->jf", g1, p["ft"]),
               db1=g1.sum((0, 1)), dW2=torch.einsum("bmc,bmj->cj", g2, p["h1"]),
               db2=g2.sum((0, 1)))
    sc = dict(g_feature=c_g1 @ p["w1"].abs() + FLOOR,
              dW1=torch.einsum("bmj,bmf->jf", c_g1, p["ft"].abs()) + FLOOR,
              db1=c_g1.sum((0, 1)) + FLOOR,
              dW2=torch.einsum("bmc,bmj->cj", c_g2, p["c_h1"]) + FLOOR,
              db2=c_g2.sum((0, 1)) + FLOOR)
    keep = torch.ones(B, dtype=torch.float64)
    if "bwdB_per" in mut:
        keep[4 * (B // 4):] = 0
    tot = (gt * p["color"].unsqueeze(-1) * keep.view(B, 1, 1, 1)).sum(0)
    c_tot = (gt.abs() * p["c_color"].unsqueeze(-1)).sum(0)
    if gr is not None:
        tot, c_tot = tot + gr, c_tot + gr.abs()
    out["g_logits"] = tot * _by_group(p["draw"], B, M, mut)
    sc["g_logits"] = c_tot * p["c_draw"] + FLOOR * (p["c_draw"] > 0)
    out["scale_of"] = sc
    return out


def tc_forward(ins):
    """``ins``: logits (M,C,hw), feature (B,M,F), w1 (H1,F), b1, w2 (C,H1), b2, tnl, cnl (0
    sigmoid, 1 relu1).  -> raw (M,C,hw), color (B,M,C), templates (B,M,C,hw), the
    pre-activations s1 and pre2, and ``scale_of``."""
    return _tc_forward(ins)


def tc_backward(ins, g_templates, g_raw=None):
    """-> g_logits (M,C,hw), g_feature (B,M,F), the batch sums dW1, db1, dW2, db2 and
    ``scale_of``."""
    return _tc_backward(ins, g_templates, g_raw)


# ------------------------------------------------------------------------------ K9 cases
REGIMES = ("benign", "saturated", "ties", "presence", "wrap", "posesat")
NOISE_SCALE = 4.0
N_IND = 8     # indicator channels of x that plant a capsule's winning pixel


def winner_pixel(b, c, HW):
    """where indicator channel c of image b is on: by turns in lanes 16-31 of the first 32
    pixels, at an index >= 32, in the last pixels (>= 64 where there are that many) and in
    lanes 0-15"""
    k, r = (b + c) % 4, (3 * b + 5 * c) % 16
    if k == 0:
        return min(16 + r, HW - 1)
    if k == 1:
        return min(32 + r, HW - 1)
    if k == 2:
        return HW - 1 - (r % 2)
    return r % HW


def _seed(regime, B, HW, A, P, C):
    return REGIMES.index(regime) * 1000003 + B * 10007 + HW * 1009 + A * 101 + P * 7 + C


def make_case(regime, B, HW, A, P, C, sim=True, noise=True, head=True, reseed=0):
    """-> (ins: fp32 tensors and the flags, meta)"""
    g = torch.Generator().manual_seed(_seed(regime, B, HW, A, P, C) + 7919 * reseed)
    r = lambda *s: torch.rand(*s, generator=g)     # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g)    # noqa: E731
    x, w, bias = n(B, HW, C), n(A, P, C) / C ** 0.5, n(A, P)
    u = r(B, A)
    ni = min(N_IND, C)
    pm = lambda *s: torch.sign(n(*s))              # noqa: E731
    if regime == "saturated":
        # per capsule one pixel's logit at least 60 above all others (up to 120: past expf's
        # range, so that a maximum over half the lanes overflows), offsets of +90 and -90
        x[..., :ni] = 0
        for b in range(B):
            for c in range(ni):
                x[b, winner_pixel(b, c, HW), c] = 1.0
        w[:, P - 1, :ni] = 0
        for a in range(A):
            w[a, P - 1, a % ni] = 70 + 50 * float(r(1))
            bias[a, P - 1] = 90.0 if a % 2 == 0 else -90.0
    elif regime == "ties":
        # even capsules: all logits equal (the bias itself); odd ones: two equal maxima 40
        # above the rest, at two pixels whose x rows are the same
        x[..., 0] = 0
        for b in range(B):
            p1, p2 = (5 * b + 1) % HW, (5 * b + 1 + max(HW // 2, 1)) % HW
            x[b, p2] = x[b, p1]
            x[b, p1, 0] = x[b, p2, 0] = 1.0
        w[0::2, P - 1] = 0
        w[1::2, P - 1] *= 0.1
        w[1::2, P - 1, 0] = 40.0
    elif regime == "presence" and P >= 8:
        bias[:, 6] = torch.where(torch.arange(A) % 2 == 0, 30.0, -30.0) + bias[:, 6]
    elif regime == "wrap" and P >= 8:
        bias[:, 2] = (r(A) * 2 - 1) * 25
    elif regime == "posesat" and P >= 8:
        for j in (0, 1, 3, 4, 5):
            bias[:, j] = pm(A) * (2 + 28 * r(A))
    elif regime != "benign":
        raise ValueError(regime)
    ins = dict(x=x, w=w.reshape(A * P, C).contiguous(), bias=bias.reshape(A * P).contiguous(),
               A=A, noise_u=u if noise else None, noise_scale=NOISE_SCALE, similarity=int(sim),
               head=bool(head))
    return ins, dict(regime=regime, shape=(B, HW, A, P, C))


def conditions(ins, meta):
    """the regime's conditions on the fp64 values -> list of violations"""
    regime, (B, HW, A, P, C) = meta["regime"], meta["shape"]
    res = forward(ins)
    l = res["y"].view(B, HW, A, P)[..., P - 1]
    bad = []
    if regime == "saturated" and HW > 1:
        top = l.topk(2, dim=1)[0]
        if float((top[:, 0] - top[:, 1]).min()) < 60:
            bad.append("gap below 60")
        if not (float(l.max()) > 150 and float(l.max(1)[0].min()) < -10):
            bad.append("offsets")
    if regime == "ties":
        if not torch.equal(l[..., 0::2].float(), ins["bias"].view(A, P)[0::2, P - 1].expand(
                B, HW, -1)):
            bad.append("even capsules: logits are not the bias")
        if HW > 1 and A > 1:
            top = l[..., 1::2].topk(min(3, HW), dim=1)[0]
            if not torch.equal(top[:, 0], top[:, 1]):
                bad.append("odd capsules: maxima differ")
            if HW > 2 and float((top[:, 1] - top[:, 2]).min()) < 30:
                bad.append("odd capsules: rest too close")
    if regime == "presence" and ins["head"]:
        lg = _pieces(ins)["logit"]
        if float(lg.abs().min()) < 20:
            bad.append("presence logit below 20")
    return bad


def checked_case(regime, B, HW, A, P, C, sim=True, noise=True, head=True):
    """``make_case``, reseeded until ``conditions`` hold; asserts that it ended clean."""
    for k in range(20):
        ins, meta = make_case(regime, B, HW, A, P, C, sim, noise, head, reseed=k)
        if not conditions(ins, meta):
            meta["reseed"] = k
            return ins, meta
    raise AssertionError(("no clean draw", regime, B, HW, A, P, C, conditions(ins, meta)))


def make_grads(B, A, P, seed=0):
    g = torch.Generator().manual_seed(4243 + seed + B * 31 + A * 7 + P)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    F = max(P - 8, 0)
    return dict(g_pose=n(B, A, 6), g_presence=n(B, A), g_feature=n(B, A, F),
                g_feature2=n(B, A, F), g=n(B, A, P - 1))


def subsets(grads, P):
    """each incoming gradient alone, g_feature + g_feature2, all four"""
    names = GRAD_NAMES if P > 8 else GRAD_NAMES[:2]
    out = [(k, {k: grads[k]}) for k in names]
    if P > 8:
        out.append(("g_feature+g_feature2", {k: grads[k] for k in GRAD_NAMES[2:]}))
    return out + [("all", {k: grads[k] for k in names})]


# (B, HW, A, P, C): groups x size, what the shape is there for
SHAPES = [
    (3, 1, 1, 8, 64),      # 1 x 1 at A = 1; HW = 1; P = 8 (no feature); group AP = 8: idle waves
    (5, 16, 8, 9, 128),    # 8 x 1; P odd: misaligned group offsets, both stage_y paths; HW = 16
    (2, 17, 128, 8, 64),   # 8 x 16; group AP = 128 exactly: 8 column tiles; aligned; HW = 17
    (3, 32, 17, 9, 192),   # 1 x 17 (prime): the second softmax trip, half-filled last wave;
                           # AP = 153: a second conv trip, ragged, A P % 4 != 0; HW = 32
    (2, 25, 37, 8, 256),   # 1 x 37: three softmax trips; AP = 296: three conv trips
    (7, 33, 42, 9, 8),     # 7 x 6; HW = 33
    (3, 64, 16, 12, 8),    # 8 x 2; group AP = 24, aligned offsets: the vector path; HW = 64
    (2, 65, 17, 10, 12),   # 1 x 17; HW = 65: three pixel trips per lane
    (256, 16, 4, 24, 64),  # 2 x 2: the early break at B d >= 512; P = 24
    (4, 25, 24, 24, 128),  # 8 x 3: the step's own shape at a small batch
]
DECOMPOSITION = {(3, 1): (1, 1), (5, 8): (8, 1), (2, 128): (8, 16), (3, 17): (1, 17),
                 (2, 37): (1, 37), (7, 42): (7, 6), (3, 16): (8, 2), (2, 17): (1, 17),
                 (256, 4): (2, 2), (4, 24): (8, 3), (6, 5): (5, 1), (3, 4): (4, 1),
                 (4, 17): (1, 17), (5, 6): (6, 1), (2, 40): (8, 5)}
REGIME_SHAPES = dict(saturated=[1, 2, 3, 4, 5, 6, 7, 9], ties=[1, 3, 4, 6, 7],
                     presence=[1, 4, 9], wrap=[1, 5], posesat=[3, 9])
# pool-only form (B, HW, A, P, C): P in {2, 5, 9}
POOL_SHAPES = [(6, 12, 5, 9, 8), (3, 1, 4, 2, 20), (4, 36, 17, 5, 8), (5, 65, 6, 2, 8),
               (2, 32, 40, 5, 8)]


def all_cases():
    """(regime, B, HW, A, P, C, similarity, noise, head) of every K9 case the GPU module runs"""
    out = [("benign", *s, i % 2, (i + 1) % 3 != 0, True) for i, s in enumerate(SHAPES)]
    for regime, idx in REGIME_SHAPES.items():
        out += [(regime, *SHAPES[i], (i + k + 1) % 2, k % 2 == 0, True)       # (noise by turns)
                for k, i in enumerate(idx)]
    out += [("benign", *s, 0, False, False) for s in POOL_SHAPES]
    out += [(regime, *POOL_SHAPES[i], 0, False, False)
            for regime, idx in (("saturated", [2, 3, 4]), ("ties", [3, 4])) for i in idx]
    return out


def find_case(regime, B, HW, A, P, C):
    (c,) = [c for c in all_cases() if c[:6] == (regime, B, HW, A, P, C) and c[8]]
    return c


# the forms that run K10 inside the head's workgroups: (head case, C, hw, H1, template_nonlin,
# color_nonlin) with M = A and F = P - 8; the colour MLP is built (``kinks``) around the
# reference's own features
FUSED_TC = [
    (("benign", 5, 16, 8, 9, 128), 3, 16, 32, 1, 1),     # M C hw = 384 > 256 at B = 5: ragged
                                                         # batch parts in the 512-thread bwdB
    (("benign", 4, 25, 24, 24, 128), 1, 121, 32, 0, 1),  # groups of 3, F = 16
    (("saturated", 4, 25, 24, 24, 128), 3, 63, 7, 1, 0),
    (("benign", 256, 16, 4, 24, 64), 1, 16, 32, 1, 1),   # 2 x 2 behind the early break
]
DECLINED_TC = (("benign", 3, 32, 17, 9, 192), 3, 16, 32, 1, 1)    # one group per image


def fused_tc_case(spec, feature=None):
    """-> (head case, its ins, the K10 ins around ``feature`` (None: the reference's))"""
    shape, C, hw, H1, tnl, cnl = spec
    c = find_case(*shape)
    ins, _ = checked_case(*c)
    B, A, P = c[1], c[3], c[4]
    if feature is None:
        feature = _forward(ins)["feature"].float()
    tins, _ = tc_checked_case("kinks", B, A, C, hw, P - 8, H1, tnl, cnl, feature=feature)
    return c, ins, tins


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}x{c[3]}x{c[4]}-C{c[5]}-" + \
        ("s" if c[6] else "a") + ("n" if c[7] else "-") + ("" if c[8] else "-pool")


def fusable(c):
    """the fused conv forms take the case (HW <= 32, C a multiple of 64, the head)"""
    return c[8] and c[2] <= 32 and c[5] % 64 == 0 and c[5] <= 256


# ----------------------------------------------------------------------------- K10 cases
TC_REGIMES = ("benign", "kinks")
NL = ("sigmoid", "relu1")
# (B, M, C, hw, F, H1): groups x size
TC_SHAPES = [
    (1, 6, 1, 1, 1, 7),       # 6 x 1; M C hw = 6: one ragged texel block; B = 1: three empty parts
    (2, 9, 3, 16, 5, 32),     # 3 x 3; M C hw = 432: two texel blocks, the last ragged
    (3, 42, 3, 63, 16, 32),   # 7 x 6
    (5, 9, 1, 64, 5, 7),      # 3 x 3; per = 2: a ragged last batch part
    (8, 6, 3, 65, 16, 32),    # 6 x 1; even batch parts; a second lane trip in bwdA
    (5, 42, 1, 121, 5, 32),   # 7 x 6
]
TC_DECOMPOSITION = {(1, 6): (6, 1), (2, 9): (3, 3), (3, 42): (7, 6), (5, 9): (3, 3),
                    (8, 6): (6, 1), (5, 42): (7, 6), (5, 8): (8, 1), (4, 24): (8, 3),
                    (256, 4): (2, 2), (3, 17): (1, 17)}


def tc_make_case(regime, B, M, C, hw, F, H1, tnl, cnl, reseed=0, feature=None):
    """``feature``: the (B,M,F) features to build the case around (the head's own, for the
    forms that run the colour MLP inside the head's workgroups)"""
    g = torch.Generator().manual_seed(TC_REGIMES.index(regime) * 1000003 + B * 10007 + M * 1009 +
                                      C * 101 + hw * 7 + F + 13 * H1 + 7919 * reseed)
    r = lambda *s: torch.rand(*s, generator=g)     # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g)    # noqa: E731
    ft = n(B, M, F)
    if feature is not None:
        ft = feature.detach().float().cpu().reshape(B, M, F)
    w1, b1 = n(H1, F) / F ** 0.5, n(H1) * 0.3
    w2, b2 = n(C, H1) / H1 ** 0.5, n(C) * 0.3
    if regime == "benign":
        lg = n(M, C, hw) * 1.6 - 0.3
    else:
        lg = r(M, C, hw) * 2 - 0.5                  # over (-0.5, 1.5): all three pieces of relu1
        if tnl == 1 and lg.numel() >= 4:
            lg.view(-1)[0::max(lg.numel() // 3, 2)] = 0.0     # ... and the kinks themselves:
            lg.view(-1)[1::max(lg.numel() // 3, 2)] = 1.0     # exact inputs, gradient 0
        # each hidden unit's bias at a middle quantile of its products: on for 35 to 65 % of
        # the (b, m) rows
        pr = (ft.double() @ w1.double().t()).reshape(B * M, H1).sort(0)[0]
        at = ((0.35 + 0.3 * r(H1)) * (B * M - 1)).long()
        b1 = -(pr[at, torch.arange(H1)] + pr[at + 1, torch.arange(H1)]).float() / 2
        # scale and shift each colour's second layer so that a third of its pre-activations
        # is below 0, a third inside the relu1 colour's window (0, 0.01) and a third above
        h1 = torch.relu(ft.double() @ w1.double().t() + b1.double())
        for c in range(C):
            q = (h1 @ w2[c].double()).flatten().sort()[0]
            k = q.numel() // 3
            lo, hi = (q[k - 1] + q[k]) / 2, (q[-k - 1] + q[-k]) / 2
            if not float(hi - lo) > 0:
                continue                            # (``tc_conditions`` then asks for a reseed)
            al = 0.01 / float(hi - lo)
            w2[c], b2[c] = w2[c] * al, -al * float(lo)
    ins = dict(logits=lg, feature=ft, w1=w1, b1=b1, w2=w2, b2=b2, tnl=int(tnl), cnl=int(cnl))
    return ins, dict(regime=regime, shape=(B, M, C, hw, F, H1))


def tc_kink_margins(ins):
    """distance of every pre-activation from its kinks over the bound c 2^-24 scale there
    (> 1: an fp32 evaluation within the bar takes the fp64 branch): ReLU at 0 for s1 and pre2,
    the relu1 colour's window ends, relu1 at 0 and 1 for the template logits (the planted
    exact 0 and 1 apart: inputs, whose products 6 x are exact) -> dict of the smallest"""
    res = tc_forward(ins)
    s, out = res["scale_of"], {}
    out["s1"] = float((res["s1"].abs() / (TC_C_OUT * U * s["s1"])).min())
    out["pre2"] = float((res["pre2"].abs() / (TC_C_OUT * U * s["pre2"])).min())
    if ins["cnl"] == 1:
        d = (res["pre2"] + K32.c99 - 1).abs() / (TC_C_OUT * U * (s["pre2"] + K32.c99))
        out["window"] = float(d.min())
    if ins["tnl"] == 1:
        lg = _d(ins["logits"])
        d = torch.minimum(lg.abs(), (lg - 1).abs())
        d = d[(lg != 0) & (lg != 1)]
        out["logits"] = float((d / (TC_C_OUT * U * 1.5)).min()) if d.numel() else math.inf
    return out


def tc_shares(ins):
    """-> (shares of pre2 <= 0, inside (0, .01), above; the smallest on- and off-share of a
    hidden ReLU over (b, m))"""
    res = tc_forward(ins)
    p2, win = res["pre2"], res["pre2"] + K32.c99
    inside = ((p2 > 0) & (win < 1)).double().mean()
    on = (res["s1"] > 0).double().mean((0, 1))
    return (float((p2 <= 0).double().mean()), float(inside), float((win >= 1).double().mean()),
            float(on.min()), float((1 - on).min()))


def tc_conditions(ins, meta):
    bad = [f"margin {k} {v:.3g}" for k, v in tc_kink_margins(ins).items() if v <= 1]
    if meta["regime"] == "kinks":
        below, inside, above, on, off = tc_shares(ins)
        if min(below, inside, above) < 0.25:
            bad.append(f"pre2 shares {below:.2f} {inside:.2f} {above:.2f}")
        if min(on, off) < 0.25:
            bad.append(f"hidden ReLU shares {on:.2f} {off:.2f}")
        lg = ins["logits"]
        if ins["tnl"] == 1 and lg.numel() >= 16 and not (
                bool((lg < 0).any()) and bool((lg > 1).any()) and bool(((lg > 0) & (lg < 1)).any())):
            bad.append("relu1 pieces")
    return bad


def tc_checked_case(regime, B, M, C, hw, F, H1, tnl, cnl, feature=None):
    """``tc_make_case``, reseeded until ``tc_conditions`` hold; asserts that it ended clean."""
    for k in range(200):
        ins, meta = tc_make_case(regime, B, M, C, hw, F, H1, tnl, cnl, reseed=k, feature=feature)
        if not tc_conditions(ins, meta):
            meta["reseed"] = k
            return ins, meta
    raise AssertionError(("no clean draw", regime, B, M, C, hw, F, H1, tc_conditions(ins, meta)))


def tc_make_grads(B, M, C, hw, seed=0):
    g = torch.Generator().manual_seed(977 + seed + B * 31 + M * 7 + C + hw)
    return torch.randn(B, M, C, hw, generator=g), torch.randn(M, C, hw, generator=g)


def tc_all_cases():
    """(regime, B, M, C, hw, F, H1, template_nonlin, color_nonlin) of every K10 case"""
    out = []
    for i, s in enumerate(TC_SHAPES):
        combos = [(t, c) for t in (0, 1) for c in (0, 1)] if i in (1, 3) else \
            [(i % 2, 1), ((i + 1) % 2, (i // 2) % 2)]
        out += [("kinks", *s, t, c) for t, c in combos]
    out += [("benign", *TC_SHAPES[i], t, c) for i, t, c in ((1, 1, 1), (4, 0, 0), (5, 1, 0))]
    return out


def tc_case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}x{c[3]}x{c[4]}-F{c[5]}-H{c[6]}-{NL[c[7]]}-{NL[c[8]]}"
