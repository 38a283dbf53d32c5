"""fp64 reference of the capsule likelihood (K4: csrc/capsule_likelihood_dev.h) that also says
how far an fp32 evaluation may be from it.  CPU only; no GPU import.

``forward`` restates ``oracle.scae_oracle.capsule_likelihood`` line by line in fp64 (dummy
row, ``log_safe``'s floor, ``is_from_capsule = win // M``; the dummy logit is log(0.01)
rounded to fp32, which is what the oracle's float32 ``zeros + log001`` and the kernel's
``kLog001`` both hold).  ``backward`` is a hand-written fp64 backward for any subset of the
eight incoming gradients.

Every float entry comes with a companion magnitude (``res["scale"][name]``): the same formula
with every summand replaced by its absolute value -- |max| + |log sum| plus the weighted input
magnitudes for a log-sum-exp, the magnitude of the exponent (+1) times the value for an
exponential, the sum of |chain-rule terms| for a gradient.  A bound is then, entry by entry,

    |fp32 - fp64| <= c * 2^-24 * scale

which serves a mixing logit of -1e8 (spacing 8) and a posterior of 1e-9 alike.  (``FLOOR`` is
added to every companion: 2^-24 of it is the smallest normal fp32, what an underflow loses.)

Derived, not measured: ``winner_gap`` returns G = gamma(24) * S per part, with
gamma(n) = n 2^-24 / (1 - n 2^-24) and S the largest, over the capsules o of the part, of
|ml| + sum_i d_i^2 / (2 s^2) + 6 |log s| + 6 * 0.5 log 2 pi: phase A's posterior logit is a
sum of 19 such terms formed with fewer than 24 roundings each, so an fp32 posterior logit is
within G of the fp64 one, an fp32 arg-max is within G of the fp64 maximum, and where the
fp64 gap between best and second best exceeds 2 G it IS the fp64 arg-max.  Where every capsule
of a part is below log_safe's 1e-16 the logits are -1e8 + vote_lp, fp32 spacing 8: the arg-max
is decided by rounding (G ~ 140), in the fp32 oracle as in the kernel.

Measured (tests/test_lk_ref.py::test_constant_c_comes_from_the_fp32_oracle re-measures and
prints them): the fp32 oracle on the CPU against this reference, worst
|fp32 - fp64| / (2^-24 scale) over every case of tests/test_capsule_likelihood_vs_fp64.py:

    outputs    log_prob_per_point 1.35  soft_winner 0.72  soft_winner_presence 2.11
               posterior 3.42  mixing_log_prob 3.15  mixing_logit 1.00
    gradients  vote 3.40  scale 3.15  vote_presence 3.34  dummy_vote 0.90  x 2.09
               presence 1.14
    (gradients: each incoming gradient alone and all eight together; in the floored parts
    the winner gradients are scattered at the fp32 oracle's own winner)

    C_OUT = 20 (4 x 3.42 = 13.7, rounded up to one digit)   C_GRAD = 20 (4 x 3.40 = 13.6)

The factor 4 is for what the kernel does differently from the oracle: 16-lane and 4-lane
summation trees instead of serial sums, and a device expf / logf / division of a couple of
ulp where the host's are one.  c is never tuned against the kernel.

``_forward`` / ``_backward`` take a set of mutant names (``MUTANTS``): each plants one
mistake of the kind the lane arithmetic invites, for test_lk_ref.py to show that the bar and
the cases see it.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
C_OUT = 20.0
C_GRAD = 20.0
LOG001 = float(np.float32(np.log(0.01)))
HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)
EPS = 1e-16
FLOOR = 2.0 ** -102   # times 2^-24: the smallest normal fp32 -- what an underflow may lose

GRAD_NAMES = ("log_prob_per_point", "winner", "winner_presence", "soft_winner",
              "soft_winner_presence", "posterior", "mixing_log_prob", "mixing_logit")
IN_NAMES = ("vote", "scale", "vote_presence", "dummy_vote", "x", "presence")
FLOAT_OUTS = ("log_prob_per_point", "soft_winner", "soft_winner_presence", "posterior",
              "mixing_log_prob", "mixing_logit")
MUTANTS = ("last_max", "no_dummy_post", "no_o64_sums", "soft_winner_mod4", "gx_mod4",
           "gmlp_no_dummy", "gmlp_o16", "gwinner_plus1", "log_safe_grad", "no_presence_grad",
           "gdummy_last_real")


def gamma(n):
    return n * U / (1 - n * U)


def f64(ins):
    return {k: None if v is None else v.detach().double() for k, v in ins.items()}


def _lse(a, s_a, keep=None):
    """log-sum-exp over dim 1 of ``a`` (entries with keep == False left out of the sum), its
    companion magnitude and the weights exp(a - lse)."""
    mx = a.max(1, keepdim=True)[0]
    e = torch.exp(a - mx)
    if keep is not None:
        e = e * keep
    sm = e.sum(1, keepdim=True)
    p = e / sm
    lse = mx + sm.log()
    s = mx.abs() + sm.log().abs() + (p * s_a).sum(1, keepdim=True)
    return lse, s, mx, sm


def _pieces(ins, mut=frozenset()):
    """what forward and backward share"""
    i = f64(ins)
    vote, sc, vp, x = i["vote"], i["scale"], i["vote_presence"], i["x"]
    B, O, M, _ = vote.shape
    d = x.unsqueeze(1) - vote                                        # (B,O,M,6)
    var2 = 2 * sc * sc
    vlp = (-(d * d) / var2.unsqueeze(-1) - sc.log().unsqueeze(-1) - HALF_LOG_2PI).sum(-1)
    s_vlp = ((d * d) / var2.unsqueeze(-1)).sum(-1) + 6 * sc.log().abs() + 6 * HALF_LOG_2PI
    small = vp < EPS
    ml_real = torch.where(small, torch.full_like(vp, -1e8),
                          torch.where(small, torch.ones_like(vp), vp).log())
    row = torch.full((B, 1, M), LOG001, dtype=torch.float64)
    ml = torch.cat([ml_real, row], 1)                                # (B,O+1,M)
    post = ml + torch.cat([vlp, row], 1)
    s_ml = ml.abs()
    s_post = s_ml + torch.cat([s_vlp, row.abs()], 1)
    keep_ml = keep_post = None
    if "no_o64_sums" in mut:
        keep_ml = torch.ones(1, O + 1, 1, dtype=torch.float64)
        keep_ml[:, 64:O] = 0
        keep_post = keep_ml
    if "no_dummy_post" in mut:
        keep_post = torch.ones(1, O + 1, 1, dtype=torch.float64) if keep_post is None \
            else keep_post.clone()
        keep_post[:, O] = 0
    lse_ml, s_lse_ml, _, _ = _lse(ml, s_ml, keep_ml)
    if "no_dummy_post" in mut:      # the maximum, too, is taken without the dummy
        pm = torch.cat([post[:, :O], torch.full((B, 1, M), -math.inf, dtype=torch.float64)], 1)
        mx = pm.max(1, keepdim=True)[0]
        sm = (torch.exp(post - mx) * keep_post).sum(1, keepdim=True)
        lse_post, s_lse_post = mx + sm.log(), mx.abs() + sm.log().abs()
    else:
        lse_post, s_lse_post, _, _ = _lse(post, s_post, keep_post)
    pp = torch.exp(post - lse_post)                                  # :338, dummy row included
    rel = s_post + s_lse_post + 1                                    # |exponent| + the exp itself
    return dict(i=i, B=B, O=O, M=M, d=d, ml=ml, post=post, s_ml=s_ml, s_post=s_post,
                lse_ml=lse_ml, s_lse_ml=s_lse_ml, lse_post=lse_post, s_lse_post=s_lse_post,
                pp=pp, rel=rel, small=small)


def _argmax(post_real, last=False):
    """torch.argmax over dim 1: the first maximum (``last``: the mutant's last one)."""
    O = post_real.shape[1]
    mx = post_real.max(1, keepdim=True)[0]
    idx = torch.arange(O).view(1, O, 1).expand_as(post_real)
    hit = post_real == mx
    if last:
        return torch.where(hit, idx, torch.full_like(idx, -1)).max(1)[0]
    return torch.where(hit, idx, torch.full_like(idx, O)).min(1)[0]


def _gather(t, win):
    """t[b, win[b, m], m]"""
    B, M = win.shape
    bi = torch.arange(B).unsqueeze(1).expand(B, M)
    mi = torch.arange(M).unsqueeze(0).expand(B, M)
    return t[bi, win, mi]


def _forward(ins, mut=frozenset()):
    p = _pieces(ins, mut)
    i, B, O, M = p["i"], p["B"], p["O"], p["M"]
    vote, vp, pres = i["vote"], i["vote_presence"], i["presence"]
    ml, post, pp, rel = p["ml"], p["post"], p["pp"], p["rel"]
    mlp = ml - p["lse_ml"]                                           # :286
    binary = (ml[:, :-1] > ml[:, -1:]).double()                      # :289
    lpp, s_lpp = p["lse_post"].squeeze(1), p["s_lse_post"].squeeze(1)
    if pres is not None:
        lpp, s_lpp = lpp * pres, s_lpp * pres.abs()                  # :296-300
    win = _argmax(post[:, :-1], "last_max" in mut)                   # :310-311
    s_pp = pp * rel + FLOOR
    votes = torch.cat([vote, i["dummy_vote"].expand(B, 1, M, 6)], 1)
    vps = torch.cat([vp, torch.zeros(B, 1, M, dtype=torch.float64)], 1)
    w = pp
    if "soft_winner_mod4" in mut:
        keep = torch.ones(O + 1, dtype=torch.float64)
        keep[3:O:4] = 0
        w = pp * keep.view(1, O + 1, 1)
    res = dict(
        log_prob_per_point=lpp, log_prob=lpp.sum(1).mean(), vote_presence_binary=binary,
        winner=_gather(vote, win), winner_presence=_gather(vp, win), winner_idx=win,
        is_from_capsule=win // M,                                    # :334 (reference quirk)
        soft_winner=(w.unsqueeze(-1) * votes).sum(1),                # :350
        soft_winner_presence=(pp * vps).sum(1),                      # :354
        posterior=pp, posterior_mixing_prob=pp[:, :-1], mixing_log_prob=mlp, mixing_logit=ml,
        post=post[:, :-1])
    res["scale"] = dict(
        log_prob_per_point=s_lpp, log_prob=s_lpp.sum(1).mean(),
        soft_winner=(s_pp.unsqueeze(-1) * votes.abs()).sum(1),
        soft_winner_presence=(s_pp * vps.abs()).sum(1),
        posterior=s_pp, posterior_mixing_prob=s_pp[:, :-1],
        mixing_log_prob=p["s_ml"] + p["s_lse_ml"], mixing_logit=p["s_ml"])
    return res


def _backward(ins, grads, winner_idx=None, mut=frozenset()):
    p = _pieces(ins)
    i, B, O, M = p["i"], p["B"], p["O"], p["M"]
    vote, sc, vp, pres = i["vote"], i["scale"], i["vote_presence"], i["presence"]
    d, ml, pp, rel = p["d"], p["ml"], p["pp"], p["rel"]
    g = {k: None if grads.get(k) is None else grads[k].detach().double() for k in GRAD_NAMES}
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    win = _argmax(p["post"][:, :-1]) if winner_idx is None else winner_idx.long().cpu()
    votes = torch.cat([vote, i["dummy_vote"].expand(B, 1, M, 6)], 1)
    vps = torch.cat([vp, z(B, 1, M)], 1)
    g_sw = g["soft_winner"] if g["soft_winner"] is not None else z(B, M, 6)
    g_swp = g["soft_winner_presence"] if g["soft_winner_presence"] is not None else z(B, M)
    g_post = g["posterior"] if g["posterior"] is not None else z(B, O + 1, M)
    g_mlp = g["mixing_log_prob"] if g["mixing_log_prob"] is not None else z(B, O + 1, M)
    g_mlogit = g["mixing_logit"] if g["mixing_logit"] is not None else z(B, O + 1, M)
    g_lpp = g["log_prob_per_point"] if g["log_prob_per_point"] is not None else z(B, M)
    # incoming gradient on every posterior probability (dummy row included)
    gpp = g_post + (g_sw.unsqueeze(1) * votes).sum(-1) + g_swp.unsqueeze(1) * vps
    s_gpp = g_post.abs() + (g_sw.abs().unsqueeze(1) * votes.abs()).sum(-1) + \
        g_swp.abs().unsqueeze(1) * vps.abs()
    w = pp * (1 + rel) + FLOOR                # a posterior and what its own round-off adds
    dot = (pp * gpp).sum(1, keepdim=True)
    s_dot = (w * s_gpp).sum(1, keepdim=True)
    glse = g_lpp if pres is None or "no_presence_grad" in mut else g_lpp * pres
    glse = glse.unsqueeze(1)
    gpost = (pp * (gpp - dot) + glse * pp)[:, :O]
    s_gpost = (w * (s_gpp + s_dot + glse.abs()))[:, :O]
    # mixing logits: the log-softmax's backward takes the column sum over all O + 1 rows
    col, s_col = g_mlp, g_mlp.abs()
    if "gmlp_no_dummy" in mut:
        col = col[:, :O]
    if "gmlp_o16" in mut:
        col = col[:, :16]
    gs, s_gs = col.sum(1, keepdim=True), s_col.sum(1, keepdim=True)
    mlp = ml - p["lse_ml"]
    s_mlp = p["s_ml"] + p["s_lse_ml"]
    gml = gpost + g_mlogit[:, :O] + g_mlp[:, :O] - (mlp.exp() * gs)[:, :O]
    s_gml = s_gpost + g_mlogit[:, :O].abs() + g_mlp[:, :O].abs() + \
        ((mlp.exp() * (1 + s_mlp) + FLOOR) * s_gs)[:, :O]
    small = p["small"]
    if "log_safe_grad" in mut:
        lsg = 1 / vp
    else:
        lsg = torch.where(small, torch.zeros_like(vp),
                          1 / torch.where(small, torch.ones_like(vp), vp))
    gvp = gml * lsg + g_swp.unsqueeze(1) * pp[:, :O]
    s_gvp = s_gml * lsg.abs() + g_swp.abs().unsqueeze(1) * w[:, :O]
    iv = (1 / (sc * sc)).unsqueeze(-1)
    gvote = gpost.unsqueeze(-1) * d * iv + g_sw.unsqueeze(1) * pp[:, :O].unsqueeze(-1)
    s_gvote = s_gpost.unsqueeze(-1) * d.abs() * iv + \
        g_sw.abs().unsqueeze(1) * w[:, :O].unsqueeze(-1)
    hot = torch.zeros(B, O, M, dtype=torch.float64)
    hot.scatter_(1, win.unsqueeze(1), 1.0)
    if g["winner_presence"] is not None:
        gvp = gvp + hot * g["winner_presence"].unsqueeze(1)
        s_gvp = s_gvp + hot * g["winner_presence"].abs().unsqueeze(1)
    if g["winner"] is not None:
        hw = hot
        if "gwinner_plus1" in mut:
            hw = torch.zeros_like(hot)
            hw.scatter_(1, ((win + 1) % O).unsqueeze(1), 1.0)
        gvote = gvote + hw.unsqueeze(-1) * g["winner"].unsqueeze(1)
        s_gvote = s_gvote + hw.unsqueeze(-1) * g["winner"].abs().unsqueeze(1)
    gscale = (gpost.unsqueeze(-1) * (d * d * iv - 1) / sc.unsqueeze(-1)).sum(-1)
    s_gscale = (s_gpost.unsqueeze(-1) * (d * d * iv + 1) / sc.unsqueeze(-1)).sum(-1)
    gx_terms = -(gpost.unsqueeze(-1) * d * iv)
    if "gx_mod4" in mut:
        gx_terms = gx_terms.clone()
        gx_terms[:, 3::4] = 0
    gx = gx_terms.sum(1)
    s_gx = (s_gpost.unsqueeze(-1) * d.abs() * iv).sum(1)
    ppd = pp[:, O - 1] if "gdummy_last_real" in mut else pp[:, O]
    gdp = g_sw * ppd.unsqueeze(-1)                                   # (B,M,6) per-image partials
    s_gdp = g_sw.abs() * w[:, O].unsqueeze(-1)
    has_dummy = g["soft_winner"] is not None or g["winner"] is not None
    out = dict(vote=gvote, scale=gscale, vote_presence=gvp, x=gx, dummy_partial=gdp,
               dummy_vote=gdp.sum(0).view(1, 1, M, 6) if has_dummy else None, presence=None)
    s = dict(vote=s_gvote, scale=s_gscale, vote_presence=s_gvp, x=s_gx, dummy_partial=s_gdp,
             dummy_vote=s_gdp.sum(0).view(1, 1, M, 6), presence=None)
    if pres is not None:
        lse, s_lse = p["lse_post"].squeeze(1), p["s_lse_post"].squeeze(1)
        out["presence"] = g_lpp * lse
        s["presence"] = g_lpp.abs() * s_lse
    out["scale_of"] = {k: None if v is None else v + FLOOR for k, v in s.items()}
    return out


def forward(ins):
    """-> dict of the eleven outputs (``posterior`` with its dummy row, (B,O+1,M), and the
    oracle's ``posterior_mixing_prob`` without), ``log_prob``, the real posterior logits
    ``post`` (B,O,M), and ``scale``: the companion magnitude of every float entry."""
    return _forward(ins)


def backward(ins, grads, winner_idx=None):
    """``grads``: any subset of GRAD_NAMES -> tensor (an absent or None one is no gradient,
    as autograd passes it).  -> gradients for vote, scale, vote_presence, dummy_vote (None
    unless a (soft) winner gradient came in), x, presence (None without ``presence``);
    ``dummy_partial`` (B,M,6): the per-image terms of dummy_vote's; ``scale_of``: the
    companions.  ``winner_idx``: scatter the winner gradients there, not at this
    reference's own arg-max."""
    return _backward(ins, grads, winner_idx)


def winner_gap(ins):
    """G (B,M): an fp32 posterior logit is within G of the fp64 one (module docstring)."""
    p = _pieces(ins)
    return gamma(24) * p["s_post"][:, :-1].max(1)[0]


def gap(post):
    """best minus second best real posterior logit, per part ((B,M); inf with one capsule)"""
    if post.shape[1] == 1:
        return torch.full_like(post[:, 0], math.inf)
    top = post.topk(2, dim=1)[0]
    return top[:, 0] - top[:, 1]


def ratio(got, ref, scale, c):
    """worst |got - ref| / (c 2^-24 scale); an entry with scale 0 must be exact."""
    dlt = (got.detach().double().cpu() - ref).abs()
    bound = c * U * scale
    r = torch.where(bound > 0, dlt / bound.clamp_min(1e-300),
                    torch.where(dlt > 0, torch.full_like(dlt, math.inf), torch.zeros_like(dlt)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------ cases
REGIMES = ("benign", "dominant", "near-dummy", "floored", "ties")


def _seed(regime, B, O, M):
    return REGIMES.index(regime) * 1000003 + B * 10007 + O * 101 + M


def make_case(regime, B, O, M, presence=True, reseed=0):
    """-> (ins: fp32 tensors, meta).  meta["floored"] (B,M) bool: parts holding a capsule below
    log_safe's floor (their G is ~140: the arg-max among floored capsules is decided by
    rounding); meta["tie"] (B,M) int64: the lower index of a planted bit-identical pair that is
    the part's maximum, or -1."""
    g = torch.Generator().manual_seed(_seed(regime, B, O, M) + 7919 * reseed)
    r = lambda *s: torch.rand(*s, generator=g)     # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g)    # noqa: E731
    vote, x = n(B, O, M, 6), n(B, M, 6)
    scale, vp = r(B, O, M) + 0.1, r(B, O, M)
    dummy, pres = n(1, 1, M, 6) * 0.1, r(B, M)
    floored = torch.zeros(B, M, dtype=torch.bool)
    tie = torch.full((B, M), -1, dtype=torch.int64)
    bi = torch.arange(B).unsqueeze(1).expand(B, M)
    mi = torch.arange(M).unsqueeze(0).expand(B, M)
    if regime == "dominant":
        # one capsule per part within 0.01 of x at scale 0.02; every other vote is many
        # sigma away, so its term underflows in expf
        scale = torch.full((B, O, M), 0.02)
        vote = x.unsqueeze(1) + (n(B, O, M, 6) + 3 * torch.sign(n(B, O, M, 6)))
        dom = torch.randint(0, O, (B, M), generator=g)
        vote[bi, dom, mi] = x + (r(B, M, 6) * 2 - 1) * 0.01 / math.sqrt(6)
    elif regime == "near-dummy":
        # the dummy carries most of the mass, the real components still matter
        vp = 0.011 + 0.009 * r(B, O, M)
        scale = 0.7 + 0.4 * r(B, O, M)
        dirs = n(B, O, M, 6)
        dirs = dirs / dirs.norm(dim=-1, keepdim=True)
        vote = x.unsqueeze(1) + 3 * scale.unsqueeze(-1) * dirs * (0.9 + 0.2 * r(B, O, M, 1))
    elif regime == "floored":
        tiny = torch.tensor([0.0, 1e-20, 9e-17])
        pick = tiny[torch.randint(0, 3, (B, O, M), generator=g)]
        all_floored = (torch.arange(M) % 2 == 0).view(1, 1, M).expand(B, O, M)
        some = r(B, O, M) < 0.5
        some[:, 0] = torch.arange(M).view(1, M) % 4 == 1      # at least one live, one floored
        if O > 1:
            some[:, 1] = ~some[:, 0]
        vp = torch.where(all_floored | some, pick, vp)
        floored = (vp < EPS).any(1)
    elif regime == "ties":
        # bit-identical pairs (same vote, scale, presence: equal logits in any precision),
        # their vote on x at a small scale so that the pair is the part's maximum
        kinds = [(o, o + 16) for o in (1,) if o + 16 < O]              # same lane
        kinds += [(o, o + 1) for o in (5,) if o + 1 < O]               # neighbouring lanes
        kinds += [(o, o2) for o, o2 in ((37, 70), (63, 64)) if o2 < O]  # across 64
        kinds += [(o, O - 1) for o in (0, O - 2) if 0 <= o < O - 1]    # the last capsule
        for m in range(M):
            for b in range(B):
                lo, hi = kinds[(m + b * 3) % len(kinds)]
                if (m + b) % 5 == 4:
                    continue                                          # some parts stay plain
                vote[b, lo, m] = x[b, m]
                scale[b, lo, m] = 0.05
                vp[b, lo, m] = 0.9
                vote[b, hi, m], scale[b, hi, m], vp[b, hi, m] = \
                    vote[b, lo, m], scale[b, lo, m], vp[b, lo, m]
                tie[b, m] = lo
    elif regime != "benign":
        raise ValueError(regime)
    # vote_presence_binary is ml > log(0.01): not decided by the rounding of logf
    band = (vp >= 0.0099) & (vp <= 0.0101)
    vp = torch.where(band, torch.full_like(vp, 0.0105), vp)
    ins = dict(vote=vote.contiguous(), scale=scale, vote_presence=vp, dummy_vote=dummy, x=x,
               presence=pres if presence else None)
    return ins, dict(floored=floored, tie=tie, regime=regime, shape=(B, O, M))


def well_separated(ins, meta):
    """(B,M) bool: outside the floored parts and the planted ties the fp64 gap between the best
    and the second-best posterior logit exceeds 2 G."""
    res = forward(ins)
    ok = gap(res["post"]) > 2 * winner_gap(ins)
    return ok | meta["floored"] | (meta["tie"] >= 0)


def checked_case(regime, B, O, M, presence=True):
    """``make_case``, reseeded until ``well_separated`` holds everywhere."""
    for k in range(20):
        ins, meta = make_case(regime, B, O, M, presence, reseed=k)
        if bool(well_separated(ins, meta).all()):
            meta["reseed"] = k
            return ins, meta
    raise AssertionError(("no well separated draw", regime, B, O, M))


def make_grads(B, O, M, seed=0):
    """the eight incoming gradients, seeded (fp32)"""
    g = torch.Generator().manual_seed(4242 + seed + B * 31 + O * 7 + M)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(log_prob_per_point=n(B, M), winner=n(B, M, 6), winner_presence=n(B, M),
                soft_winner=n(B, M, 6), soft_winner_presence=n(B, M), posterior=n(B, O + 1, M),
                mixing_log_prob=n(B, O + 1, M), mixing_logit=n(B, O + 1, M))


SHAPES = [(2, 1, 1), (2, 3, 5), (3, 15, 37), (3, 16, 36), (3, 17, 37), (2, 63, 64), (2, 64, 65),
          (2, 65, 65), (2, 80, 24), (2, 130, 100), (2, 200, 60), (1030, 3, 2)]
REGIME_SHAPES = [(3, 17, 37), (2, 64, 65), (2, 65, 65), (2, 130, 100)]
TIE_SHAPES = [(2, 64, 65), (2, 130, 100)]
NOPRES_SHAPES = [(3, 17, 37), (2, 65, 65)]


def all_cases():
    """(regime, B, O, M, presence) of every case the GPU module runs"""
    out = [("benign", *s, True) for s in SHAPES]
    out += [(r, *s, True) for r in ("dominant", "near-dummy", "floored") for s in REGIME_SHAPES]
    out += [("ties", *s, True) for s in TIE_SHAPES]
    out += [("benign", *s, False) for s in NOPRES_SHAPES]
    return out


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" + ("" if c[4] else "-nopres")
