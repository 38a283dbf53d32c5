"""tests/lk_ref.py proven on the CPU: the fp64 reference is the oracle's capsule likelihood,
its hand-written backward is autograd's, the constant c of the bar comes from the fp32 oracle,
the cases satisfy the conditions the winner checks rest on, and the bar with these cases
sees each of the mistakes the kernel's lane arithmetic invites (``lk_ref.MUTANTS``).
Run with -s for the measured ratios."""
import functools
import math

import pytest
import torch

from oracle import scae_oracle as O
from tests import lk_ref as R
from tests.golden_util import assert_close, load, sub

CASES = R.all_cases()
IDS = [R.case_id(c) for c in CASES]


@functools.lru_cache(maxsize=None)
def case(c):
    ins, meta = R.checked_case(*c)
    return ins, meta, R.forward(ins)


class _Keep(torch.Tensor):
    """``presence.float()`` (object_decoder.py:298) is the identity on fp32 inputs; it stays
    the identity in the fp64 run of the oracle."""

    def float(self):
        return self


def _oracle(ins, dtype, grad=False):
    """the oracle on ``ins`` in ``dtype`` -> (leaves, result)"""
    lv = {k: None if v is None else v.detach().to(dtype).requires_grad_(grad)
          for k, v in ins.items()}
    pres = lv["presence"]
    if pres is not None and dtype == torch.float64:
        pres = pres.as_subclass(_Keep)
    return lv, O.capsule_likelihood(lv["vote"], lv["scale"], lv["vote_presence"],
                                    lv["dummy_vote"], lv["x"], pres)


def _per_point(lv):
    """object_decoder.py:263-300 with the oracle's own pieces, for log_prob_per_point (the
    oracle returns only its mean)"""
    B, M, _ = lv["x"].shape
    vlp = O.normal_log_prob(lv["x"].unsqueeze(1), lv["vote"], lv["scale"].unsqueeze(-1)).sum(-1)
    log001 = float(math.log(0.01))
    row = torch.zeros(B, 1, M) + log001
    post = torch.cat([O.log_safe(lv["vote_presence"]), row], 1) + torch.cat([vlp, row], 1)
    pp = post.logsumexp(1)
    return pp if lv["presence"] is None else pp * lv["presence"]


def _weighted(res, lv, grads, ins):
    """sum of <incoming gradient, output> on an oracle result (log_prob_per_point through
    ``_per_point``, the posterior's dummy row as one minus the real rows)"""
    tot = 0.0
    for k, g in grads.items():
        g = g.to(lv["vote"].dtype)
        if k == "log_prob_per_point":
            tot = tot + (_per_point(lv) * g).sum()
        elif k == "posterior":
            pm = res.posterior_mixing_prob
            tot = tot + (pm * g[:, :-1]).sum() + ((1 - pm.sum(1)) * g[:, -1]).sum()
        else:
            tot = tot + (res[k] * g).sum()
    return tot


def _oracle_grads(ins, grads, dtype):
    lv, res = _oracle(ins, dtype, grad=True)
    _weighted(res, lv, grads, ins).backward()
    return {k: None if v is None else v.grad for k, v in lv.items()}, res


def _winner_idx(res, vote):
    """the oracle returns ``winner`` and ``win // M`` only: the index whose vote it gathered"""
    hit = (vote == res.winner.unsqueeze(1)).all(-1)                   # (B,O,M)
    O_ = vote.shape[1]
    idx = torch.arange(O_).view(1, O_, 1).expand_as(hit)
    return torch.where(hit, idx, torch.full_like(idx, O_)).min(1)[0]


def _subsets(grads):
    return [(k, {k: grads[k]}) for k in R.GRAD_NAMES] + [("all", dict(grads))]


# ----------------------------------------------------------------------- the reference is right
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_forward_equals_the_fp64_oracle(c):
    ins, meta, res = case(c)
    lv, ro = _oracle(ins, torch.float64)
    # 1e-12 relative -- of the companion magnitude, which is the entry's own size for every
    # tensor but the posterior family: exp(-600) carries the round-off of its exponent
    ro = dict(ro, log_prob_per_point=_per_point(lv))
    for k in ("log_prob", "log_prob_per_point", "soft_winner", "soft_winner_presence",
              "posterior_mixing_prob", "mixing_log_prob", "mixing_logit"):
        assert R.ratio(res[k], ro[k], res["scale"][k], 1e-12 / R.U) <= 1.0, k
    for k in ("winner", "winner_presence", "vote_presence_binary", "is_from_capsule"):
        assert torch.equal(res[k], ro[k].to(res[k].dtype)), k
    B, Oc, M = c[1:4]
    assert res["post"].shape == (B, Oc, M) and res["posterior"].shape == (B, Oc + 1, M)
    assert_close(res["posterior"].sum(1), torch.ones(B, M, dtype=torch.float64), 1e-12, 0, "sum")


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_backward_equals_autograd_through_the_fp64_oracle(c):
    ins, meta, res = case(c)
    B, Oc, M = c[1:4]
    worst = 0.0
    for name, gs in _subsets(R.make_grads(B, Oc, M)):
        got = R.backward(ins, gs)
        ref, _ = _oracle_grads(ins, gs, torch.float64)
        for k in R.IN_NAMES:
            if ref[k] is None:
                # no path from these outputs (autograd: None; the kernel's partials: zeros)
                assert got[k] is None or float(got[k].abs().max()) == 0.0, (name, k)
                continue
            r = R.ratio(got[k], ref[k], got["scale_of"][k], 1e-11 / R.U)
            worst = max(worst, r)
            assert r <= 1.0, (name, k, r)
    print(f"{R.case_id(c)}: worst |hand - autograd| / (1e-11 scale) {worst:.3g}")


@pytest.mark.parametrize("name", ["a", "b", "nopres"])
def test_forward_equals_the_committed_golden_vectors(name):
    blob, _ = load("op_capsule_likelihood")
    cs = sub(blob, name + "/")
    ins = dict(sub(cs, "in/"))
    ins.setdefault("presence", None)
    res = R.forward(ins)
    clear = R.gap(res["post"]) > 2 * R.winner_gap(ins)     # (a, b hold parts floored throughout)
    for k, ref in sub(cs, "out/").items():
        got = res[k]
        if k in ("winner", "winner_presence", "is_from_capsule"):
            got, ref = got[clear], ref[clear]
        assert_close(got.to(ref.dtype), ref, 1e-5, 1e-5, "out " + k)


# ------------------------------------------------------------------------------ the constant c
def test_constant_c_comes_from_the_fp32_oracle():
    """worst |fp32 oracle - fp64| / (2^-24 scale) per tensor over every case of the GPU
    module; C_OUT and C_GRAD are 4 x the worst, rounded up to one digit (a little room below
    for another host's libm)."""
    outs = {k: (0.0, "") for k in R.FLOAT_OUTS}
    grs = {k: (0.0, "") for k in R.IN_NAMES}
    for c in CASES:
        ins, meta, res = case(c)
        B, Oc, M = c[1:4]
        lv, r32 = _oracle(ins, torch.float32)
        win32 = _winner_idx(r32, ins["vote"])
        win = torch.where(meta["floored"], win32, res["winner_idx"])
        got = dict(log_prob_per_point=_per_point(lv), soft_winner=r32.soft_winner,
                   soft_winner_presence=r32.soft_winner_presence,
                   posterior=r32.posterior_mixing_prob, mixing_log_prob=r32.mixing_log_prob,
                   mixing_logit=r32.mixing_logit)
        for k in outs:
            ref, sc = res[k], res["scale"][k]
            if k == "posterior":
                ref, sc = ref[:, :-1], sc[:, :-1]
            r = R.ratio(got[k], ref, sc, 1.0)
            if r > outs[k][0]:
                outs[k] = (r, R.case_id(c))
        for name, gs in _subsets(R.make_grads(B, Oc, M)):
            g32, _ = _oracle_grads(ins, gs, torch.float32)
            ref = R.backward(ins, gs, winner_idx=win)
            for k in grs:
                if g32[k] is None:
                    continue
                r = R.ratio(g32[k], ref[k], ref["scale_of"][k], 1.0)
                if r > grs[k][0]:
                    grs[k] = (r, f"{R.case_id(c)} {name}")
    for k, (r, where) in outs.items():
        print(f"output   {k:22s} worst ratio {r:.3f}  ({where})")
    for k, (r, where) in grs.items():
        print(f"gradient {k:22s} worst ratio {r:.3f}  ({where})")
    for what, c_used, table in (("C_OUT", R.C_OUT, outs), ("C_GRAD", R.C_GRAD, grs)):
        worst = max(r for r, _ in table.values())
        print(f"{what} = {c_used}: 4 x worst = {4 * worst:.3f}")
        assert 4 * worst <= c_used <= 8 * worst, (what, worst)


# ---------------------------------------------------------- the conditions hold for the cases
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_cases_are_well_separated_and_ties_are_the_maximum(c):
    ins, meta, res = case(c)
    assert bool(R.well_separated(ins, meta).all())
    tie = meta["tie"]
    if c[0] == "ties":
        assert int((tie >= 0).sum()) > tie.numel() // 2
        post, on = res["post"], tie >= 0
        mx = post.max(1)[0]
        lo = R._gather(post, tie.clamp_min(0))
        assert torch.equal(lo[on], mx[on])                      # the pair is the maximum ...
        assert int(((post == mx.unsqueeze(1)).sum(1)[on] != 2).sum()) == 0   # ... and a pair
        assert torch.equal(res["winner_idx"][on], tie[on])      # first maximum: the lower one
        kinds = set()
        for b, m in on.nonzero().tolist():
            hi = int((post[b, :, m] == mx[b, m]).nonzero()[-1])
            lo_ = int(tie[b, m])
            kinds.add("lane" if hi - lo_ == 16 else "next" if hi - lo_ == 1 else "far")
            kinds.add("last" if hi == c[2] - 1 else "inner")
            if lo_ < 64 <= hi:
                kinds.add("across64")
        assert {"lane", "next", "last"} <= kinds and ("across64" in kinds) == (c[2] > 64)
    if c[0] == "floored":
        fl = meta["floored"]
        small = ins["vote_presence"] < R.EPS
        assert bool(small.all(1).any()) and bool((small.any(1) & ~small.all(1)).any())
        assert torch.equal(fl, small.any(1))
    band = (ins["vote_presence"] >= 0.0099) & (ins["vote_presence"] <= 0.0101)
    assert not bool(band.any())


@pytest.mark.parametrize("regime", ["benign", "dominant"])
@pytest.mark.parametrize("shape", [(3, 17, 37), (2, 65, 65), (2, 130, 100)])
def test_fp32_and_fp64_argmax_agree_where_the_gap_says_so(regime, shape):
    ins, meta, res = case((regime, *shape, True))
    _, r32 = _oracle(ins, torch.float32)
    assert torch.equal(_winner_idx(r32, ins["vote"]), res["winner_idx"])
    G = R.winner_gap(ins)
    print(f"{regime} {shape}: smallest gap / 2G {float((R.gap(res['post']) / (2 * G)).min()):.3g}")


def test_the_regimes_are_what_they_say():
    ins, _, res = case(("dominant", 3, 17, 37, True))
    assert float(res["posterior"][:, :-1].max(1)[0].min()) > 0.999
    second = res["post"].topk(2, dim=1)[0][:, 1] - res["post"].max(1)[0]
    assert float(second.max()) < -104          # expf underflows to zero below -103.97
    ins, _, res = case(("near-dummy", 3, 17, 37, True))
    dummy = res["posterior"][:, -1]
    assert float(dummy.mean()) > 0.5 and float((1 - dummy).min()) > 1e-3
    ins, meta, res = case(("floored", 2, 130, 100, True))
    small = ins["vote_presence"] < R.EPS
    dead = small.all(1)
    assert float(res["posterior"][:, -1][dead].min()) == 1.0
    assert float(R.winner_gap(ins)[dead].min()) > 100   # fp32 cannot order these logits


# ----------------------------------------------------------------------- the bar sees mistakes
MUTANT_CASES = [("benign", 3, 17, 37, True), ("near-dummy", 3, 17, 37, True),
                ("benign", 2, 65, 65, True), ("near-dummy", 2, 130, 100, True),
                ("floored", 3, 17, 37, True), ("ties", 2, 64, 65, True),
                ("ties", 2, 130, 100, True)]


def _mutant_excess(mutant, c):
    """-> (worst ratio against the bar, which tensor) of the mutant on one case;
    inf for a changed discrete output."""
    ins, meta, res = case(c)
    B, Oc, M = c[1:4]
    mut = frozenset([mutant])
    worst, where = 0.0, ""
    bad = R._forward(ins, mut)
    for k in ("winner_idx", "is_from_capsule", "vote_presence_binary"):
        if not torch.equal(bad[k], res[k]):
            return math.inf, k
    for k in R.FLOAT_OUTS:
        r = R.ratio(bad[k], res[k], res["scale"][k], R.C_OUT)
        if r > worst:
            worst, where = r, k
    for name, gs in _subsets(R.make_grads(B, Oc, M)):
        ref = R.backward(ins, gs)
        badg = R._backward(ins, gs, None, mut)
        for k in R.IN_NAMES + ("dummy_partial",):
            if ref[k] is None:
                continue
            r = R.ratio(badg[k], ref[k], ref["scale_of"][k], R.C_GRAD)
            if r > worst:
                worst, where = r, f"grad {k} ({name})"
    return worst, where


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_bar_sees_the_mutant(mutant):
    best = (0.0, "", "")
    for c in MUTANT_CASES:
        r, where = _mutant_excess(mutant, c)
        if r > best[0]:
            best = (r, R.case_id(c), where)
    print(f"mutant {mutant:18s} exceeds the bar {best[0]:.3g} x on {best[1]}: {best[2]}")
    assert best[0] >= 4.0, best


def test_the_reference_itself_is_no_mutant():
    for c in MUTANT_CASES[:2]:
        ins, _, res = case(c)
        again = R._forward(ins, frozenset())
        assert all(torch.equal(again[k], res[k]) for k in R.FLOAT_OUTS)
