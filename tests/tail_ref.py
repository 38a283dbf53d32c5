"""fp64 reference of the fused loss tail (K6: csrc/loss_tail.hip, csrc/loss_tail_dev.h) that
also says how far an fp32 evaluation may be from it.  CPU only; no GPU import.  The role
tests/lk_ref.py plays for K4 and tests/k1_ref.py for K1.

``compose`` is the tail written with the oracle's own pieces (``O.sparsity_loss`` and with it
``O.log_safe`` / ``O.normalize``, ``F.cross_entropy`` over softmax probabilities with detached
classifier inputs) in whatever dtype its leaves have; ``forward`` is ``compose`` in fp64 and
returns the 12-vector of loss_tail_dev.h, ``backward`` is fp64 autograd over it, contracted with
``gout12`` on the 12-vector and ``g_loss`` on the scalar.  The weights, ``within_const``,
``n_classes_cfg``, ``sparsity_on``, ``rec_sums``, ``reg`` and ``w_reg`` are taken exactly as the
ABI takes them (``n_classes_cfg`` <= 0 counts as 1; the posterior call never sees
``within_const``).

``hand`` restates both by hand, formula by formula as the kernels form them, and with every
value returns a companion magnitude: the same expression with every addend replaced by its
absolute value, each factor's own magnitude carried along by the chain rule --

    batch mean          sum |v| / B
    l2 term             (sum |x| + |c|)^2 (mean over images / columns)
    -p log_safe(p k)    p (|L| + 1): L = log(p k) or the floor -1e8; the 1 is the relative
                        error of the argument
    its derivative e    |L| + 2 (the +1 of d/dp(-p log p k) by absolute value), 1e8 below the floor
    within gradient     (m_e + sum_o m_e p) / (r + 1e-8) / B, between the same over the columns
    softmax p           p (1 + m_z + m_lse) + FLOOR, m_z = sum |x w| + |b|, m_lse as lk_ref._lse
    xe                  |max p| + |log sum exp(p - max)| + p_label + sum_c m_dq m_p,
                        m_dq = softmax(p) + [c = label]
    d xe / d logit      m_p (m_dq + sum p m_dq) + p sum m_p m_dq
    the incoming        m_g0 = |gout12[0]| + |g_loss|; w g0 + gout12[i]: |w| m_g0 + |gout12[i]|

-- and the bar of an entry is ``C[kind] * 2**-24 * magnitude`` (``ratio``).  An entry whose
magnitude is zero must be exact: the sparsity terms and their gradients with ``sparsity_on = 0``,
the cross-entropies without a label, the posterior's dummy row.

Measured (tests/test_tail_ref.py::test_constants_come_from_the_fp32_oracle re-measures and prints
them): ``compose`` in fp32 on the CPU with fp32 autograd against this reference, worst
|fp32 - fp64| / (2^-24 magnitude) over every case of ``all_cases()``, every one of the twelve
``gout12`` entries alone, all together, ``g_loss`` alone and ``g_loss`` with ``gout12``: MEASURED
below.  Each kind has its own constant, 4 x its ratio rounded up to one digit (the project's
convention: the factor 4 is for what the kernels do differently from ATen -- 16-lane, 4-lane and
wave summation trees instead of ATen's, fmaf chains, the device's expf / logf / division).  No
constant is tuned against a kernel.

Conditions on the inputs (``checked_case``), so that fp32 and fp64 may not legitimately
disagree: no argument ``q = p k`` of ``log_safe`` lies within a relative 2^-16 of its threshold
1e-16 (exact zeros and values <= 1e-20 are wanted and are far from it).  The tail takes no
arg-max.  Nothing is masked out of a comparison.

``hand(..., mut=...)`` plants one mistake of the kind this kernel's arithmetic invites
(``MUTANTS``), for tests/test_tail_ref.py to show that the bars and the cases see it.
"""
import math

import torch
import torch.nn.functional as F

from oracle import scae_oracle as O

U = 2.0 ** -24
EPS = 1e-16
FLOOR = 2.0 ** -102   # times 2^-24: the smallest normal fp32 -- what an underflow may lose
TYPES = ("l2", "entropy", "kl")
WEIGHTS = (1.0, 2.0, 0.35, 0.7, 0.2)
W_REG = 0.37
NT_SMALL, NTC_LARGE, NTB_LARGE, MAXCLS = 512, 1024, 256, 32   # loss_tail_dev.h / loss_tail.hip

# kinds of entry.  outputs: the 12-vector's index -> kind; gradients: by tensor
OUT_KIND = ("loss", "mean", "mean", "between", "mean", "between", "xe", "xe", "mean", "mean",
            "mean", "mean")
OUT_NAMES = ("loss", "log_prob", "prior_within", "prior_between", "post_within", "post_between",
             "prior_cls_xe", "post_cls_xe", "rec_ll", "neg_rec_ll", "neg_log_prob", "reg")
GRAD_KIND = dict(lpp="bcast", rec_sums="bcast", reg="bcast", caps_presence="g_cp",
                 posterior="g_posterior", cls_w="g_cls", cls_b="g_cls")
GRAD_NAMES = tuple(GRAD_KIND)
# worst ratio of the fp32 composition against this reference, per kind (test_tail_ref.py prints)
MEASURED = dict(mean=1.36, between=1.29, loss=0.90, xe=1.00, g_cp=4.40, g_posterior=4.72,
                bcast=1.21, g_cls=0.50)


def _four_times(v):
    """4 x the measured ratio, rounded up to one significant digit"""
    x = 4.0 * v
    e = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / e - 1e-9) * e


C = {k: _four_times(v) for k, v in MEASURED.items()}

MUTANTS = ("colsum_tail", "gpost_no_M", "post_between_prior_cols", "kl_k1", "no_dot_w",
           "gw_cp_both", "no_pdq_dot", "g10_sign", "grec_unwritten")


def defer_preferred(B, O_):
    """scae_loss_tail_defer_preferred's formula: the small form while B B 2 O 4 <= 8 MiB"""
    return B > 0 and O_ > 0 and B * B * 2 * O_ * 4 <= (8 << 20)


# ------------------------------------------------------------------------- oracle composition
def leaves(ins, dtype, grad=False):
    out = {}
    for k, v in ins.items():
        if v is None or k == "label":
            out[k] = v
        else:
            out[k] = v.detach().to(dtype).requires_grad_(grad)
    return out


def compose(lv, cfg):
    """the 12-vector from the oracle's pieces, in the dtype of the leaves"""
    lpp, post, cp = lv["lpp"], lv["posterior"], lv["caps_presence"]
    B, M = lpp.shape
    nc = cfg["n_classes_cfg"] if cfg["n_classes_cfg"] and cfg["n_classes_cfg"] > 0 else 1
    w = cfg["weights"]
    zero = torch.zeros((), dtype=lpp.dtype)
    log_prob = lpp.sum() / B
    mass = post[:, :-1].sum(-1)
    pw = pb = qw = qb = zero
    if cfg["sparsity_on"]:
        pw, pb = O.sparsity_loss(cfg["prior"], cp, n_classes=nc,
                                 within_example_constant=cfg["within_const"])
        qw, qb = O.sparsity_loss(cfg["post"], mass / M, n_classes=nc)
    xe1 = xe2 = zero
    if lv["label"] is not None:
        p1 = torch.softmax(F.linear(cp.detach(), lv["cls_w"], lv["cls_b"]), -1)
        p2 = torch.softmax(F.linear(mass.detach(), lv["cls_w"], lv["cls_b"]), -1)
        xe1, xe2 = F.cross_entropy(p1, lv["label"]), F.cross_entropy(p2, lv["label"])
    rec = lv["rec_sums"].sum() / B if lv.get("rec_sums") is not None else zero
    reg = lv["reg"].reshape(()) if lv.get("reg") is not None else zero
    loss = -w[0] * log_prob + w[1] * pw + w[2] * pb + w[3] * qw + w[4] * qb + xe1 + xe2 - rec \
        + cfg["w_reg"] * reg
    return torch.stack([loss, log_prob, pw, pb, qw, qb, xe1, xe2, rec, -rec, -log_prob, reg])


def forward(ins, cfg):
    """-> (12,) fp64: loss, log_prob, the four sparsity terms, the two cross-entropies over
    probabilities, rec_ll, -rec_ll, -log_prob, reg"""
    return compose(leaves(ins, torch.float64), cfg).detach()


def autograd(ins, cfg, gout12, g_loss, dtype):
    """gradients of <gout12, out12> + g_loss * out12[0] through ``compose`` in ``dtype`` ->
    dict over GRAD_NAMES (None: the ABI writes nothing there)"""
    lv = leaves(ins, dtype, grad=True)
    out = compose(lv, cfg)
    tot = torch.zeros((), dtype=dtype)
    if gout12 is not None:
        tot = tot + (out * gout12.to(dtype)).sum()
    if g_loss is not None:
        tot = tot + out[0] * g_loss.to(dtype).reshape(())
    names = [k for k in GRAD_NAMES if lv.get(k) is not None]
    gs = torch.autograd.grad(tot, [lv[k] for k in names], allow_unused=True)
    res = {k: None for k in GRAD_NAMES}
    for k, g in zip(names, gs):
        res[k] = torch.zeros_like(lv[k]) if g is None else g
    return res


def backward(ins, cfg, gout12=None, g_loss=None):
    """fp64 autograd over ``forward``: gradients for lpp, posterior (dummy row zero),
    caps_presence, cls_w, cls_b, rec_sums and reg"""
    return autograd(ins, cfg, gout12, g_loss, torch.float64)


# --------------------------------------------------------------------------- the hand-written
def _ent(x, k):
    """f = sum_o -p log_safe(p k), p = x / (sum x + 1e-8), over the last dim -> value, its
    companion, d value / d x (without the dot projection: e / (r+eps), and the dot), companions"""
    r = x.sum(-1, keepdim=True)
    rinv = 1.0 / (r + 1e-8)
    p = x * rinv
    q = p * k
    small = q < EPS
    L = torch.where(small, torch.full_like(q, -1e8),
                    torch.where(small, torch.ones_like(q), q).log())
    val = (-p * L).sum(-1)
    m_val = (p * (L.abs() + 1)).sum(-1)
    e = torch.where(small, torch.full_like(q, 1e8), -(L + 1))
    m_e = torch.where(small, torch.full_like(q, 1e8), L.abs() + 2)
    dot = (e * p).sum(-1, keepdim=True)
    m_dot = (m_e * p).sum(-1, keepdim=True)
    return dict(val=val, m_val=m_val, e=e, m_e=m_e, dot=dot, m_dot=m_dot, rinv=rinv, q=q)


def _sparsity(x, col, kind, cw, cb, gw, m_gw, gb, m_gb, mut):
    """within / between terms of x (B,O) >= 0 with the column sums ``col`` (O,) -> pw, m_pw, pb,
    m_pb, g_x (B,O), m_g_x"""
    B, Oc = x.shape
    if kind == "l2":
        r, m_r = x.sum(1), x.abs().sum(1)
        pw, m_pw = ((r - cw) ** 2).mean(), ((m_r + abs(cw)) ** 2).mean()
        m_col = col.abs()       # (column sums of non-negative entries)
        pb, m_pb = ((col - cb) ** 2).mean(), ((m_col + abs(cb)) ** 2).mean()
        g = gw * 2 * (r - cw).unsqueeze(1) / B + gb * 2 * (col - cb).unsqueeze(0) / Oc
        m_g = m_gw * 2 * (m_r + abs(cw)).unsqueeze(1) / B \
            + m_gb * 2 * (m_col + abs(cb)).unsqueeze(0) / Oc
        return pw, m_pw, pb, m_pb, g, m_g
    k = float(Oc) if kind == "kl" and "kl_k1" not in mut else 1.0
    w, b = _ent(x, k), _ent(col, k)
    pw, m_pw = w["val"].mean(), w["m_val"].mean()
    pb, m_pb = -b["val"], b["m_val"]
    dw = (w["e"] - (0.0 if "no_dot_w" in mut else w["dot"])) * w["rinv"] / B
    m_dw = (w["m_e"] + w["m_dot"]) * w["rinv"] / B
    db = -(b["e"] - b["dot"]) * b["rinv"]
    m_db = (b["m_e"] + b["m_dot"]) * b["rinv"]
    return pw, m_pw, pb, m_pb, gw * dw + gb * db.unsqueeze(0), \
        m_gw * m_dw + m_gb * m_db.unsqueeze(0)


def _cls(X, W, b, label, mut):
    """softmax(X W^T + b), cross_entropy over the probabilities -> per-image xe, companion,
    d xe_b / d logit (B, ncls), companion"""
    z = X @ W.t() + b
    m_z = X.abs() @ W.abs().t() + b.abs()
    mx = z.max(1, keepdim=True)[0]
    ez = torch.exp(z - mx)
    sm = ez.sum(1, keepdim=True)
    p = ez / sm
    m_lse = mx.abs() + sm.log().abs() + (p * m_z).sum(1, keepdim=True)
    m_p = p * (1 + m_z + m_lse) + FLOOR
    mx2 = p.max(1, keepdim=True)[0]
    q = torch.exp(p - mx2)
    s2 = q.sum(1, keepdim=True)
    hot = F.one_hot(label, p.shape[1]).double()
    pl = (p * hot).sum(1)
    xe = mx2.squeeze(1) + s2.log().squeeze(1) - pl
    dq, m_dq = q / s2 - hot, q / s2 + hot
    m_xe = mx2.abs().squeeze(1) + s2.log().abs().squeeze(1) + pl + (m_dq * m_p).sum(1)
    dot = (p * dq).sum(1, keepdim=True)
    m_dot = (m_p * m_dq).sum(1, keepdim=True)
    if "no_pdq_dot" in mut:
        dot = torch.zeros_like(dot)
    gl = p * (dq - dot)
    m_gl = m_p * (m_dq + (p * m_dq).sum(1, keepdim=True)) + p * m_dot
    return xe, m_xe, gl, m_gl


def hand(ins, cfg, gout12=None, g_loss=None, mut=frozenset()):
    """-> dict(out (12), m_out (12), grads {name: tensor | None}, m_grads): the tail and its
    backward as the kernels form them, in fp64, with the companion of every entry"""
    mut = frozenset(mut)
    d = lambda t: None if t is None else t.detach().double()   # noqa: E731
    lpp, post, cp = d(ins["lpp"]), d(ins["posterior"]), d(ins["caps_presence"])
    W, bias, label = d(ins["cls_w"]), d(ins["cls_b"]), ins["label"]
    rec_in, reg_in = d(ins.get("rec_sums")), d(ins.get("reg"))
    B, M = lpp.shape
    Oc = cp.shape[1]
    nc = float(cfg["n_classes_cfg"]) if cfg["n_classes_cfg"] and cfg["n_classes_cfg"] > 0 else 1.0
    w_ll, w_pw, w_pb, w_qw, w_qb = [float(v) for v in cfg["weights"]]
    w_reg = float(cfg["w_reg"])
    G = torch.zeros(12, dtype=torch.float64) if gout12 is None else d(gout12).clone()
    m_G = G.abs()
    if g_loss is not None:
        G[0] = G[0] + float(g_loss)
        m_G[0] = m_G[0] + abs(float(g_loss))
    g0, m_g0 = G[0], m_G[0]
    z = torch.zeros((), dtype=torch.float64)

    log_prob, m_log_prob = lpp.sum() / B, lpp.abs().sum() / B
    mass = post[:, :Oc].sum(-1)                   # (B,O) un-normalised: the classifier's input
    xq = mass / M
    keep = B - B % 64 if "colsum_tail" in mut else B
    col_p, col_q = cp[:keep].sum(0), xq[:keep].sum(0)
    if "post_between_prior_cols" in mut:
        col_q = col_p
    pw = pb = qw = qb = m_pw = m_pb = m_qw = m_qb = z
    g_cp = torch.zeros(B, Oc, dtype=torch.float64)
    g_xq, m_g_cp, m_g_xq = g_cp.clone(), g_cp.clone(), g_cp.clone()
    if cfg["sparsity_on"]:
        cw = float(Oc) / nc if cfg["within_const"] is None else float(cfg["within_const"])
        pw, m_pw, pb, m_pb, g_cp, m_g_cp = _sparsity(
            cp, col_p, cfg["prior"], cw, B / nc, w_pw * g0 + G[2], abs(w_pw) * m_g0 + m_G[2],
            w_pb * g0 + G[3], abs(w_pb) * m_g0 + m_G[3], mut)
        qw, m_qw, qb, m_qb, g_xq, m_g_xq = _sparsity(
            xq, col_q, cfg["post"], float(Oc) / nc, B / nc, w_qw * g0 + G[4],
            abs(w_qw) * m_g0 + m_G[4], w_qb * g0 + G[5], abs(w_qb) * m_g0 + m_G[5], mut)
    div = 1.0 if "gpost_no_M" in mut else float(M)
    g_post = torch.zeros_like(post)
    m_g_post = torch.zeros_like(post)
    g_post[:, :Oc] = (g_xq / div).unsqueeze(-1)
    m_g_post[:, :Oc] = (m_g_xq / M).unsqueeze(-1)

    xe1 = xe2 = m_xe1 = m_xe2 = z
    g_w = g_b = m_g_w = m_g_b = None
    if label is not None:
        x1, m_x1, gl1, m_gl1 = _cls(cp, W, bias, label, mut)
        x2, m_x2, gl2, m_gl2 = _cls(mass, W, bias, label, mut)
        xe1, m_xe1, xe2, m_xe2 = x1.mean(), m_x1.mean(), x2.mean(), m_x2.mean()
        gx1, gx2 = (g0 + G[6]) / B, (g0 + G[7]) / B
        m_gx1, m_gx2 = (m_g0 + m_G[6]) / B, (m_g0 + m_G[7]) / B
        X2 = cp if "gw_cp_both" in mut else mass
        g_w = gx1 * (gl1.t() @ cp) + gx2 * (gl2.t() @ X2)
        m_g_w = m_gx1 * (m_gl1.t() @ cp.abs()) + m_gx2 * (m_gl2.t() @ mass.abs())
        g_b = gx1 * gl1.sum(0) + gx2 * gl2.sum(0)
        m_g_b = m_gx1 * m_gl1.sum(0) + m_gx2 * m_gl2.sum(0)

    rec, m_rec = (rec_in.sum() / B, rec_in.abs().sum() / B) if rec_in is not None else (z, z)
    reg, m_reg = (reg_in.reshape(()), reg_in.abs().reshape(())) if reg_in is not None else (z, z)
    loss = -w_ll * log_prob + w_pw * pw + w_pb * pb + w_qw * qw + w_qb * qb + xe1 + xe2 - rec \
        + w_reg * reg
    m_loss = abs(w_ll) * m_log_prob + abs(w_pw) * m_pw + abs(w_pb) * m_pb + abs(w_qw) * m_qw \
        + abs(w_qb) * m_qb + m_xe1 + m_xe2 + m_rec + abs(w_reg) * m_reg
    out = torch.stack([loss, log_prob, pw, pb, qw, qb, xe1, xe2, rec, -rec, -log_prob, reg])
    m_out = torch.stack([m_loss, m_log_prob, m_pw, m_pb, m_qw, m_qb, m_xe1, m_xe2, m_rec, m_rec,
                         m_log_prob, m_reg])

    s10 = 1.0 if "g10_sign" in mut else -1.0
    g_lp = (-w_ll * g0 + G[1] + s10 * G[10]) / B
    m_g_lp = (abs(w_ll) * m_g0 + m_G[1] + m_G[10]) / B
    grads = dict(lpp=torch.full_like(lpp, float(g_lp)), posterior=g_post, caps_presence=g_cp,
                 cls_w=g_w, cls_b=g_b, rec_sums=None, reg=None)
    m_grads = dict(lpp=torch.full_like(lpp, float(m_g_lp)), posterior=m_g_post,
                   caps_presence=m_g_cp, cls_w=m_g_w, cls_b=m_g_b, rec_sums=None, reg=None)
    if rec_in is not None:
        gr = torch.full_like(rec_in, float((-g0 + G[8] - G[9]) / B))
        if "grec_unwritten" in mut:
            gr[B * (rec_in.numel() // B):] = 0.0
        grads["rec_sums"] = gr
        m_grads["rec_sums"] = torch.full_like(rec_in, float((m_g0 + m_G[8] + m_G[9]) / B))
    if reg_in is not None:
        grads["reg"] = (w_reg * g0 + G[11]).reshape(reg_in.shape)
        m_grads["reg"] = (abs(w_reg) * m_g0 + m_G[11]).reshape(reg_in.shape)
    return dict(out=out, m_out=m_out, grads=grads, m_grads=m_grads)


def ratio(got, ref, scale, c):
    """worst |got - ref| / (c 2^-24 scale); an entry with scale 0 must be exact."""
    dlt = (got.detach().double().cpu() - ref).abs()
    bound = c * U * scale
    r = torch.where(bound > 0, dlt / bound.clamp_min(1e-300),
                    torch.where(dlt > 0, torch.full_like(dlt, math.inf), torch.zeros_like(dlt)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


def out_ratios(got12, ref12, m12, unit=False):
    """per entry of the 12-vector: |got - ref| / bar (``unit``: bar with c = 1)"""
    return [ratio(got12[i:i + 1], ref12[i:i + 1], m12[i:i + 1], 1.0 if unit else C[OUT_KIND[i]])
            for i in range(12)]


def grad_ratios(got, ref, m, unit=False):
    """per gradient tensor that the reference has: |got - ref| / bar"""
    return {k: ratio(got[k], ref[k], m[k], 1.0 if unit else C[GRAD_KIND[k]])
            for k in GRAD_NAMES if ref[k] is not None}


def log_safe_args(ins, cfg):
    """every q = p k the case's entropy / kl terms feed to ``log_safe`` (fp64), one tensor"""
    if not cfg["sparsity_on"]:
        return torch.zeros(0, dtype=torch.float64)
    cp = ins["caps_presence"].double()
    Oc = cp.shape[1]
    xq = ins["posterior"].double()[:, :Oc].sum(-1) / ins["lpp"].shape[1]
    qs = []
    for x, kind in ((cp, cfg["prior"]), (xq, cfg["post"])):
        if kind == "l2":
            continue
        k = float(Oc) if kind == "kl" else 1.0
        qs += [_ent(x, k)["q"].flatten(), _ent(x.sum(0), k)["q"].flatten()]
    return torch.cat(qs) if qs else torch.zeros(0, dtype=torch.float64)


def clear_of_threshold(ins, cfg):
    q = log_safe_args(ins, cfg)
    return bool(((q / EPS - 1).abs() > 2.0 ** -16).all())


# ------------------------------------------------------------------------------------ cases
REGIMES = ("benign", "sparse", "saturated", "cancelling")
N_REC = ("7B", "B-3", "B+5", "1")


def _case(B, O_, M, ncls, prior, post, regime="benign", n_rec="7B", within_const=None,
          sparsity_on=True, n_classes_cfg=None):
    return dict(B=B, O=O_, M=M, ncls=ncls, prior=prior, post=post, regime=regime, n_rec=n_rec,
                within_const=within_const, sparsity_on=sparsity_on,
                n_classes_cfg=(ncls if n_classes_cfg is None else n_classes_cfg))


def all_cases():
    """every case the GPU module runs: (B, O, M, ncls) at the smallest shapes that take each
    path of the kernels, the nine (prior, posterior) type pairs, the regimes, ``sparsity_on``,
    ``within_const`` and the four ``n_rec`` spread over them"""
    c = _case
    nine = [(p, q) for p in TYPES for q in TYPES]
    spread = ["benign", "sparse", "cancelling", "saturated", "sparse", "cancelling", "sparse",
              "benign", "saturated"]
    out = [
        c(1, 1, 1, 1, "l2", "l2", n_rec="1"),                          # degenerate sizes
        c(5, 3, 5, 2, "entropy", "kl", n_rec="B+5"),                   # B < 16, O < 4, scalar M
        c(17, 7, 7, 10, "kl", "entropy", "sparse", n_rec="B-3"),       # O tail of 3
        c(17, 7, 7, 10, "entropy", "kl", "benign", n_rec="B+5", sparsity_on=False),
        c(63, 24, 24, 10, "l2", "entropy"),                            # the b + 48 < B boundary
        c(64, 24, 24, 10, "entropy", "l2", n_rec="B+5", within_const=1.5),
        c(67, 24, 24, 10, "kl", "kl", "sparse", n_rec="B-3"),
    ]
    for i, (p, q) in enumerate(nine):                                  # the existing shape
        out.append(c(128, 24, 24, 10, p, q, spread[i], n_rec=N_REC[i % 4],
                     within_const=1.5 if p == "l2" and i % 2 == 0 else None))
    out += [
        c(33, 65, 70, 32, "kl", "l2", n_rec="B-3"),                    # O, M > 64, MAXCLS, rounds
        c(33, 65, 70, 32, "entropy", "kl", "sparse", n_rec="B+5"),
        c(515, 1, 4, 3, "l2", "kl", n_rec="1"),                        # stride loop B > 512
        c(40, 24, 24, 0, "l2", "l2", within_const=1.5, n_classes_cfg=10),   # no label
        # ---- large form
        c(210, 24, 24, 10, "l2", "entropy", n_rec="B+5"),              # first large B at O = 24
        c(210, 24, 24, 10, "entropy", "kl", "sparse"),
        c(210, 24, 24, 10, "kl", "l2", "saturated", n_rec="B-3"),
        c(131, 70, 5, 10, "entropy", "entropy", "cancelling", n_rec="B+5"),  # O > 64, 64-blocks
        c(131, 70, 5, 10, "l2", "kl", n_rec="1", sparsity_on=False),
        c(95, 130, 8, 4, "kl", "kl", "sparse", n_rec="B-3"),           # 2 O 16 > 1024
        c(95, 130, 8, 4, "l2", "l2", n_rec="7B", within_const=1.5),
        c(1030, 3, 5, 2, "l2", "kl"),                                  # stride loop B > 1024
        c(1030, 3, 5, 2, "entropy", "l2", "sparse", n_rec="1"),
        c(210, 24, 24, 0, "kl", "entropy", n_rec="B+5", n_classes_cfg=10),   # no label
    ]
    return out


def form(c):
    return "small" if defer_preferred(c["B"], c["O"]) else "large"


def case_id(c):
    s = f"{form(c)}-{c['B']}x{c['O']}x{c['M']}x{c['ncls']}-{c['prior']}-{c['post']}-{c['regime']}"
    s += f"-nrec{c['n_rec']}"
    if c["within_const"] is not None:
        s += "-wc"
    if not c["sparsity_on"]:
        s += "-off"
    return s


def n_rec_of(c):
    B = c["B"]
    return max(1, {"7B": 7 * B, "B-3": B - 3, "B+5": B + 5, "1": 1}[c["n_rec"]])


def cfg_of(c):
    return dict(prior=c["prior"], post=c["post"], weights=WEIGHTS, within_const=c["within_const"],
                n_classes_cfg=c["n_classes_cfg"], sparsity_on=c["sparsity_on"], w_reg=W_REG)


def make_case(c, reseed=0):
    """-> ins: fp32 tensors (label int64; cls_w, cls_b, label None without classes)"""
    B, Oc, M, ncls = c["B"], c["O"], c["M"], c["ncls"]
    seed = REGIMES.index(c["regime"]) * 1000003 + B * 10007 + Oc * 101 + M * 7 + ncls \
        + 31 * TYPES.index(c["prior"]) + 57 * TYPES.index(c["post"]) + 7919 * reseed
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)     # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g)    # noqa: E731
    regime = c["regime"]
    lpp = n(B, M)
    post = torch.softmax(n(B, Oc + 1, M), 1)
    cp = r(B, Oc)
    rec = n(n_rec_of(c))
    W = b = label = None
    if ncls > 0:
        W, b = n(ncls, Oc) * 0.3, n(ncls) * 0.1
        label = torch.randint(0, ncls, (B,), generator=g)
        label[0], label[-1] = 0, ncls - 1          # (B = 1: the last assignment holds)
    if regime == "sparse":
        tiny = torch.tensor([1e-20, 1e-25, 1e-30])
        u = r(B, Oc)
        cp = torch.where(u < 0.3, torch.zeros_like(cp), cp)
        cp = torch.where((u >= 0.3) & (u < 0.5),
                         tiny[torch.randint(0, 3, (B, Oc), generator=g)], cp)
        cp[0] = 0.0                                  # a whole zero row
        if B > 2:
            cp[2] = tiny[torch.randint(0, 3, (Oc,), generator=g)]   # a row of tiny values only
        if Oc > 1:
            cp[:, 1] = 0.0                           # a whole zero column
        # posteriors: one-hot parts (all mass on one capsule), dummy-dominated parts (real rows
        # 1e-22), and a capsule that explains nothing anywhere (a zero column of the mass)
        for bi in range(B):
            kind = bi % 4
            if kind == 0:
                hot = torch.randint(0, Oc, (M,), generator=g)
                post[bi] = 0.0
                post[bi, hot, torch.arange(M)] = 1.0
            elif kind == 1:
                post[bi, :Oc] = 1e-22
                post[bi, Oc] = 1.0
        if Oc > 2:
            post[:, 2] = 0.0
        if B > 3:
            post[3, :Oc] = 0.0                       # an image whose mass is exactly zero
            post[3, Oc] = 1.0
    elif regime == "saturated":
        W = n(ncls, Oc) * (30.0 / math.sqrt(Oc / 3.0))
        b = n(ncls) * 3.0
    elif regime == "cancelling":
        lpp = -1e4 + 100.0 * n(B, M)
        rec = n(n_rec_of(c)) * 1e4
    elif regime != "benign":
        raise ValueError(regime)
    return dict(lpp=lpp, posterior=post.contiguous(), caps_presence=cp, cls_w=W, cls_b=b,
                label=label, rec_sums=rec, reg=r(1))


def checked_case(c):
    """``make_case``, reseeded until no ``log_safe`` argument is near its threshold"""
    cfg = cfg_of(c)
    for k in range(20):
        ins = make_case(c, reseed=k)
        if clear_of_threshold(ins, cfg):
            return ins, cfg
    raise AssertionError(("no draw clear of log_safe's threshold", case_id(c)))


def make_gouts(c):
    """the incoming gradients of a case: [(name, gout12 | None, g_loss | None)] -- each of the
    twelve entries alone (one-hot, value not 1), all together, g_loss alone, g_loss + gout12"""
    g = torch.Generator().manual_seed(4242 + c["B"] * 31 + c["O"] * 7 + c["M"])
    full = torch.randn(12, generator=g) * 0.8 + torch.sign(torch.randn(12, generator=g)) * 0.3
    gl = torch.tensor([1.3])
    sets = []
    for i in range(12):
        one = torch.zeros(12)
        one[i] = full[i]
        sets.append((f"gout[{i}]", one, None))
    sets += [("gout all", full, None), ("g_loss", None, gl), ("g_loss + gout", full, gl)]
    return sets
