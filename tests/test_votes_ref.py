"""tests/votes_ref.py proven on the CPU: the fp64 reference is the oracle's capsule layer from
``all_param`` onwards, its hand-written backward is autograd's, the constants of the bar come
from the fp32 oracle, the cases satisfy the conditions the arg-max checks rest on, and the bar
with these cases sees each of the mistakes the kernels' lane arithmetic invites
(``votes_ref.MUTANTS``).  Run with -s for the measured ratios."""
import functools
import math
from unittest import mock

import pytest
import torch

from oracle import scae_oracle as O
from tests import votes_ref as R

CASES = R.all_cases()
IDS = [R.case_id(c) for c in CASES]


@functools.lru_cache(maxsize=None)
def case(c):
    ins, meta = R.checked_case(*c)
    return ins, meta, R.forward(ins)


def _oracle(ins, dtype, grad=False):
    """``oracle.scae_oracle.capsule_layer`` in ``dtype`` as a function of ``all_param``: its
    ``mlp`` is patched so that the ``caps_mlps.i`` calls hand out ``all_param[:, i]`` of a
    leaf.  cpr_static is a per-example leaf, so that its gradient is the kernel's gcpr_in.
    -> (leaves, outputs)"""
    ap = ins["all_param"].detach().to(dtype).requires_grad_(grad)
    B, Oc, A = ap.shape
    V = (A - 7) // 8
    lv = dict(all_param=ap, cpr_static=ins["cpr_static"].detach().to(dtype).expand(
        B, Oc, V, 6).clone().requires_grad_(grad))
    for k in R.PARAM_NAMES[1:]:
        lv[k] = ins[k].detach().to(dtype).requires_grad_(grad)
    P = {"p.cpr_static": lv["cpr_static"]}
    for j, k in enumerate(R.PARAM_NAMES[1:]):
        P[f"p.caps_bias_list.{j}"] = lv[k]
    noisy = ins["noise_caps"] is not None or ins["noise_vote"] is not None
    cfg = dict(n_caps=Oc, n_votes=V, allow_deformations=bool(ins["allow_deformations"]),
               similarity_transform=bool(ins["similarity"]),
               learn_vote_scale=bool(ins["learn_vote_scale"]),
               noise_type="uniform" if noisy else None, noise_scale=ins["noise_scale"])
    # (an absent draw: 0.5, whose term (0.5 - 0.5) * noise_scale is exactly 0)
    nc = ins["noise_caps"] if ins["noise_caps"] is not None else torch.full((B, Oc, 1), 0.5)
    nv = ins["noise_vote"] if ins["noise_vote"] is not None else torch.full((B, Oc, V), 0.5)

    def fake_mlp(P_, prefix, x, n_linear):
        if ".caps_mlps." in prefix:
            return ap[:, int(prefix.rsplit(".", 1)[1])]
        return torch.zeros(x.shape[0], 1, dtype=dtype)
    with mock.patch.object(O, "mlp", fake_mlp):
        res = O.capsule_layer(P, "p", torch.zeros(B, Oc, 1, dtype=dtype), cfg,
                              noise_caps=nc.to(dtype), noise_vote=nv.to(dtype))
    dyn = ap[..., :6 * V] if ins["allow_deformations"] else torch.zeros(B, Oc, 6 * V, dtype=dtype)
    out = dict(vote=res.vote[..., :2, :].reshape(B, Oc, V, 6), scale=res.scale,
               vote_presence=res.vote_presence, logit_caps=res.presence_logit_per_caps,
               logit_vote=res.presence_logit_per_vote, reg=res.cpr_dynamic_reg_loss,
               reg_partial=(dyn ** 2).sum(-1))         # (object_decoder.py:170, per capsule)
    assert out["logit_caps"].shape == (B, Oc, 1) and out["scale"].shape == (B, Oc, V)
    return lv, out


def _oracle_grads(ins, grads, dtype, caps_arg):
    """autograd through the oracle of sum <incoming gradient, output>; caps_presence is the
    vote presence at ``caps_arg``.  -> gradients named as votes_ref.backward's"""
    lv, out = _oracle(ins, dtype, grad=True)
    tot = torch.zeros((), dtype=dtype)
    for k, g in grads.items():
        g = g.to(dtype)
        if k == "greg":
            tot = tot + out["reg"] * g
        elif k == "gcaps_presence":
            tot = tot + (out["vote_presence"].gather(-1, caps_arg.unsqueeze(-1)).squeeze(-1)
                         * g).sum()
        else:
            name = dict(gvote="vote", gscale="scale", gvote_presence="vote_presence",
                        glogit_caps="logit_caps", glogit_vote="logit_vote")[k]
            tot = tot + (out[name] * g.reshape(out[name].shape)).sum()
    if tot.requires_grad:
        tot.backward()
    gr = {k: v.grad if v.grad is not None else torch.zeros_like(v) for k, v in lv.items()}
    live = (ins["all_param"] > 0).to(dtype)
    res = dict(gall_param=gr["all_param"], gall_param_gated=gr["all_param"] * live,
               gcpr_in=gr["cpr_static"], cpr_static=gr["cpr_static"].sum(0, keepdim=True))
    for k in R.PARAM_NAMES[1:]:
        res[k] = gr[k]
    return res


GRAD_KEYS = R.GRAD_OUTS + R.PARAM_NAMES


# ----------------------------------------------------------------------- the reference is right
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_forward_equals_the_fp64_oracle(c):
    ins, meta, _ = case(c)
    res = R._forward(ins, K=R.K64)
    _, ro = _oracle(ins, torch.float64)
    for k in R.FLOAT_OUTS:
        assert res[k].shape == ro[k].shape, k
        assert R.ratio(res[k], ro[k], res["scale_of"][k], 1e-12 / R.U) <= 1.0, k
    B = c[1]
    reg = res["reg_partial"].sum() / 2 / B
    assert abs(float(reg - ro["reg"])) <= 1e-12 * float(res["scale_of"]["reg_partial"].sum())
    arg = R._argmax(ro["vote_presence"])
    sure = R.clear(res) | (meta["tie"] >= 0)
    assert torch.equal(res["caps_arg"][sure], arg[sure])
    cp = ro["vote_presence"].gather(-1, res["caps_arg"].unsqueeze(-1)).squeeze(-1)
    assert R.ratio(res["caps_presence"], cp, res["scale_of"]["caps_presence"], 1e-12 / R.U) <= 1.0
    assert torch.equal(res["caps_presence"], res["vote_presence"].max(-1)[0])


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_backward_equals_autograd_through_the_fp64_oracle(c):
    ins, meta, _ = case(c)
    arg = R._forward(ins, K=R.K64)["caps_arg"]
    worst = 0.0
    for name, gs in R.subsets(R.make_grads(*c[1:4])):
        got = R._backward(ins, gs, arg, K=R.K64)
        ref = _oracle_grads(ins, gs, torch.float64, arg)
        for k in GRAD_KEYS:
            assert got[k].shape == ref[k].shape, (name, k)
            r = R.ratio(got[k], ref[k], got["scale_of"][k], 1e-11 / R.U)
            worst = max(worst, r)
            assert r <= 1.0, (name, k, r)
    print(f"{R.case_id(c)}: worst |hand - autograd| / (1e-11 scale) {worst:.3g}")


# ------------------------------------------------------------------------------ the constants
def test_constants_come_from_the_fp32_oracle():
    """worst |fp32 oracle - fp64| / (2^-24 scale) per tensor over every case of the GPU
    module; C_OUT and C_GRAD are 4 x the worst, rounded up to one digit (a little room below
    for another host's libm)."""
    outs = {k: (0.0, "") for k in R.FLOAT_OUTS}
    grs = {k: (0.0, "") for k in GRAD_KEYS}
    for c in CASES:
        ins, meta, res = case(c)
        _, r32 = _oracle(ins, torch.float32)
        for k in outs:
            r = R.ratio(r32[k], res[k], res["scale_of"][k], 1.0)
            if r > outs[k][0]:
                outs[k] = (r, R.case_id(c))
        sure = R.clear(res) | (meta["tie"] >= 0)
        arg = torch.where(sure, res["caps_arg"], R._argmax(r32["vote_presence"]))
        for name, gs in R.subsets(R.make_grads(*c[1:4])):
            g32 = _oracle_grads(ins, gs, torch.float32, arg)
            ref = R.backward(ins, gs, arg)
            for k in grs:
                r = R.ratio(g32[k], ref[k], ref["scale_of"][k], 1.0)
                if r > grs[k][0]:
                    grs[k] = (r, f"{R.case_id(c)} {name}")
    for k, (r, where) in outs.items():
        print(f"output   {k:18s} worst ratio {r:.3f}  ({where})")
    for k, (r, where) in grs.items():
        print(f"gradient {k:18s} worst ratio {r:.3f}  ({where})")
    # (the parameter gradients are batch sums: the op-level test adds gamma(B) for them)
    for what, c_used, table in (("C_OUT", R.C_OUT, outs),
                                ("C_GRAD", R.C_GRAD, {k: grs[k] for k in R.GRAD_OUTS})):
        worst = max(r for r, _ in table.values())
        print(f"{what} = {c_used}: 4 x worst = {4 * worst:.3f}")
        assert 4 * worst <= c_used <= 8 * worst, (what, worst)


# ---------------------------------------------------------- the conditions hold for the cases
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_conditions(c):
    ins, meta, res = case(c)
    regime, B, Oc, V = c[:4]
    ap, tie, vp = ins["all_param"], meta["tie"], res["vote_presence"]
    plain = tie < 0
    if bool(plain.any()):
        frac = float(R.clear(res)[plain].double().mean())
        if frac < 1:
            print(f"{R.case_id(c)}: {100 * frac:.1f} % of the plain capsules are clear")
        assert frac >= 0.9
    # the same conditions on what a one-layer identity chain hands the vote blocks
    assert R.well_separated(R.relu_case(ins), meta)
    if regime == "ties":
        on = tie >= 0
        assert int(on.sum()) > tie.numel() // 2
        for variant in (ins, R.relu_case(ins)):
            r = R.forward(variant)
            for dt in (torch.float64, torch.float32):
                p = _oracle(variant, dt)[1]["vote_presence"]
                mx = p.max(-1, keepdim=True)[0]
                n_max = (p == mx).sum(-1)
                assert bool(((n_max[on] == 2) | (n_max[on] == 3)).all())
                assert torch.equal(R._argmax(p)[on], tie[on])       # the lowest tied vote
            assert torch.equal(r["caps_arg"][on], tie[on])
        kinds = set()
        for b, o in on.nonzero().tolist():
            hit = (vp[b, o] == vp[b, o].max()).nonzero().flatten().tolist()
            kinds.add("triple" if len(hit) == 3 else "pair")
            for lo, hi in zip(hit, hit[1:]):
                kinds.add({1: "next", 16: "lane16", 64: "lane64"}.get(hi - lo, "far"))
                if lo < 64 <= hi:
                    kinds.add("across64")
                if lo // 16 != hi // 16 and hi - lo == 1:
                    kinds.add("across16")
            if hit[-1] == V - 1:
                kinds.add("last")
        want = {"next", "last", "pair"}
        if V > 16 and B * Oc >= 3:
            want |= {"lane16", "across16", "triple"}
        if V > 64 and B * Oc >= 6:
            want |= {"lane64", "across64"}
        assert want <= kinds, (want, kinds)
    if regime == "saturated":
        for variant in (ins, R.relu_case(ins)):
            o32 = _oracle(variant, torch.float32)[1]
            sv = torch.sigmoid(o32["logit_vote"])
            sc = torch.sigmoid(o32["logit_caps"])
            assert bool((sv == 0).any()) and bool((sv == 1).any()) and bool((sc == 1).any())
            assert float(o32["logit_vote"].abs().min()) > 15
            if ins["learn_vote_scale"]:
                x = R._pieces(variant)["sx"]
                assert bool((x > 20).any()) and bool(((x < 20) & (x > 15)).any())
                assert bool((x <= -100).any())
        assert bool((torch.sigmoid(_oracle(ins, torch.float32)[1]["logit_caps"]) == 0).any()) \
            or B * Oc < 29
    if regime == "relu":
        assert 0.4 < float((ap == 0).float().mean()) < 0.6 and bool((ap < 0).any())
    if regime == "wrap":
        p2 = ap[..., 2:6 * V:6].reshape(B, Oc, V) + ins["cpr_static"][..., 2]
        c2 = ap[..., 6 * V + 2] + ins["bias_cvr"][0, :, 0, 2]
        assert 30 < float(p2.abs().max()) <= 50 and 15 < float(c2.abs().max()) <= 50


def test_fp32_and_fp64_argmax_agree_where_the_gap_says_so():
    for c in CASES:
        ins, meta, res = case(c)
        _, r32 = _oracle(ins, torch.float32)
        sure = R.clear(res)
        assert torch.equal(R._argmax(r32["vote_presence"])[sure], res["caps_arg"][sure]), c


# ----------------------------------------------------------------------- the bar sees mistakes
MUTANT_CASES = [("benign", 17, 5, 7, 1, 1, 1, "both"), ("benign", 33, 2, 17, 0, 1, 1, "both"),
                ("benign", 3, 2, 65, 1, 1, 1, "both"), ("relu", 17, 5, 7, 1, 1, 1, "both"),
                ("ties", 17, 5, 7, 1, 1, 1, "both"), ("ties", 33, 2, 17, 0, 1, 1, "both"),
                ("ties", 3, 2, 65, 1, 1, 1, "both")]
assert all(c in CASES for c in MUTANT_CASES)


def _mutant_excess(mutant, c):
    """-> (worst ratio against the bar, which tensor) of the mutant on one case; inf for an
    arg-max that changed where the GPU module pins it (clear capsules, planted ties)."""
    ins, meta, res = case(c)
    mut = frozenset([mutant])
    worst, where = 0.0, ""
    bad = R._forward(ins, mut)
    sure = R.clear(res) | (meta["tie"] >= 0)
    if not torch.equal(bad["caps_arg"][sure], res["caps_arg"][sure]):
        return math.inf, "caps_arg"
    for k in R.FLOAT_OUTS + ("caps_presence",):
        r = R.ratio(bad[k], res[k], res["scale_of"][k], R.C_OUT)
        if r > worst:
            worst, where = r, k
    for name, gs in R.subsets(R.make_grads(*c[1:4])):
        ref = R.backward(ins, gs, res["caps_arg"])
        badg = R._backward(ins, gs, res["caps_arg"], mut)
        for k in R.GRAD_OUTS:
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
    print(f"mutant {mutant:14s} exceeds the bar {best[0]:.3g} x on {best[1]}: {best[2]}")
    assert best[0] >= 4.0, best


def test_the_reference_itself_is_no_mutant():
    for c in MUTANT_CASES[:2]:
        ins, _, res = case(c)
        again = R._forward(ins, frozenset())
        assert all(torch.equal(again[k], res[k]) for k in R.FLOAT_OUTS + ("caps_arg",))
        gs = R.make_grads(*c[1:4])
        a, b = R.backward(ins, gs), R._backward(ins, gs, None, frozenset())
        assert all(torch.equal(a[k], b[k]) for k in GRAD_KEYS)
