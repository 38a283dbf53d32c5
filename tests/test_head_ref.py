"""tests/head_ref.py proven on the CPU: the fp64 reference is the composition of the oracle's
ops (F.conv2d + multiple_attention_pooling_2d + geometric_transform + sigmoid for K9,
template_generator for K10), its hand-written backward is autograd's, the constants of the
bar come from the fp32 oracle, the cases satisfy their regimes' conditions with no entry left
out, and the bar with these cases sees each of the mistakes the kernels' lane arithmetic
invites (``head_ref.MUTANTS``).  Run with -s for the measured ratios."""
import functools
import math
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import scae_oracle as O
from tests import head_ref as R

CASES = R.all_cases()
IDS = [R.case_id(c) for c in CASES]
TC_CASES = R.tc_all_cases()
TC_IDS = [R.tc_case_id(c) for c in TC_CASES]


@functools.lru_cache(maxsize=None)
def case(c):
    ins, meta = R.checked_case(*c)
    return ins, meta, R.forward(ins)


@functools.lru_cache(maxsize=None)
def tc_case(c):
    ins, meta = R.tc_checked_case(*c)
    return ins, meta, R.tc_forward(ins)


def _grad_sets(c):
    gs = R.make_grads(c[1], c[3], c[4])
    return R.subsets(gs, c[4]) if c[8] else [("g", dict(g=gs["g"]))]


@functools.lru_cache(maxsize=None)
def _ref_backward(c, name):
    return R.backward(case(c)[0], dict(_grad_sets(c))[name])


def _oracle(ins, dtype, grads=None):
    """the composed oracle ops in ``dtype`` (from x, or from the given y) -> outputs, and with
    ``grads`` the autograd gradients dy (and dx, dw, db)"""
    A, lv = int(ins["A"]), {}
    if ins.get("x") is not None:
        for k in ("x", "w", "bias"):
            lv[k] = ins[k].detach().to(dtype).requires_grad_(grads is not None)
        B, HW, C = lv["x"].shape
        fm = F.conv2d(lv["x"].permute(0, 2, 1).reshape(B, C, HW, 1),
                      lv["w"].view(-1, C, 1, 1), lv["bias"])              # (B,AP,HW,1)
    else:
        lv["y"] = ins["y"].detach().to(dtype).requires_grad_(grads is not None)
        B, HW, _ = lv["y"].shape
        fm = lv["y"].permute(0, 2, 1).unsqueeze(-1).contiguous()
    if grads is not None:
        fm.retain_grad()
    P = fm.shape[1] // A
    pooled = O.multiple_attention_pooling_2d(fm, A).view(B, A, P - 1)
    out = dict(y=fm[..., 0].permute(0, 2, 1), pooled=pooled,
               mask=F.softmax(fm.view(B, A, P, HW)[:, :, -1], -1).permute(0, 2, 1))
    if ins.get("head", True):
        out["pose"] = O.geometric_transform(pooled[..., :6], similarity=bool(ins["similarity"]))
        lg = pooled[..., 6]
        if ins.get("noise_u") is not None:
            lg = lg + (ins["noise_u"].to(dtype) - .5) * ins["noise_scale"]
        out["presence"] = torch.sigmoid(lg)
        out["absence"] = 1 - out["presence"]
        out["feature"] = pooled[..., 7:]
    if grads is None:
        return out
    tot = torch.zeros((), dtype=dtype)
    for k, g in grads.items():
        name = dict(g_pose="pose", g_presence="presence", g_feature="feature",
                    g_feature2="feature", g="pooled")[k]
        tot = tot + (out[name] * g.to(dtype)).sum()
    tot.backward()
    gr = dict(dy=fm.grad[..., 0].permute(0, 2, 1))
    if "x" in lv:
        gr.update(dx=lv["x"].grad, dw=lv["w"].grad, db=lv["bias"].grad)
    return gr


def _tc_oracle(ins, dtype, g_templates=None, g_raw=None):
    M, C, hw = ins["logits"].shape
    lv = {k: ins[k].detach().to(dtype).requires_grad_(g_templates is not None)
          for k in ("logits", "feature", "w1", "b1", "w2", "b2")}
    P = {"tg.template_logits": lv["logits"].view(1, M, C, hw, 1),
         "tg.templates_color_mlp.0.weight": lv["w1"], "tg.templates_color_mlp.0.bias": lv["b1"],
         "tg.templates_color_mlp.2.weight": lv["w2"], "tg.templates_color_mlp.2.bias": lv["b2"]}
    cfg = dict(template_nonlin=R.NL[ins["tnl"]], color_nonlin=R.NL[ins["cnl"]],
               colorize_templates=True)
    res = O.template_generator(P, "tg", lv["feature"], lv["feature"].shape[0], cfg)
    B = lv["feature"].shape[0]
    tm, raw = res.templates.view(B, M, C, hw), res.raw_templates.view(M, C, hw)
    if g_templates is None:
        h = torch.relu(F.linear(lv["feature"], lv["w1"], lv["b1"]))
        col = torch.relu(F.linear(h, lv["w2"], lv["b2"]))
        col = O.relu1(col + .99) if ins["cnl"] == 1 else torch.sigmoid(col)
        return dict(raw=raw, templates=tm, color=col)
    tot = (tm * g_templates.to(dtype)).sum()
    if g_raw is not None:
        tot = tot + (raw * g_raw.to(dtype)).sum()
    tot.backward()
    return dict(g_logits=lv["logits"].grad, g_feature=lv["feature"].grad, dW1=lv["w1"].grad,
                db1=lv["b1"].grad, dW2=lv["w2"].grad, db2=lv["b2"].grad)


def _outs(ins):
    return (("y",) if ins.get("x") is not None else ()) + \
        (R.HEAD_OUTS if ins.get("head", True) else ("pooled",))


# ----------------------------------------------------------------------- the reference is right
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_forward_equals_the_fp64_oracle(c):
    ins = case(c)[0]
    for variant in (ins, R.from_y(ins)):
        res = R._forward(variant, K=R.K64)
        ro = _oracle(variant, torch.float64)
        for k in _outs(variant) + ("mask",):
            assert res[k].shape == ro[k].shape, k
            assert R.ratio(ro[k], res[k], res["scale_of"][k], 1e-12 / R.U) <= 1.0, k


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_backward_equals_autograd_through_the_fp64_oracle(c):
    ins = case(c)[0]
    worst = 0.0
    for variant in (ins, R.from_y(ins)):
        for name, gs in _grad_sets(c):
            got = R._backward(variant, gs, K=R.K64)
            ref = _oracle(variant, torch.float64, gs)
            for k, t in ref.items():
                assert got[k].shape == t.shape, (name, k)
                r = R.ratio(t, got[k], got["scale_of"][k], 1e-11 / R.U)
                worst = max(worst, r)
                assert r <= 1.0, (name, k, r)
    print(f"{R.case_id(c)}: worst |hand - autograd| / (1e-11 scale) {worst:.3g}")


@pytest.mark.parametrize("c", TC_CASES, ids=TC_IDS)
def test_tc_reference_equals_the_fp64_oracle(c):
    ins = tc_case(c)[0]
    res = R._tc_forward(ins, K=R.K64)
    ro = _tc_oracle(ins, torch.float64)
    for k in R.TC_OUTS:
        assert res[k].shape == ro[k].shape, k
        assert R.ratio(ro[k], res[k], res["scale_of"][k], 1e-12 / R.U) <= 1.0, k
    gt, gr = R.tc_make_grads(*c[1:5])
    for g_raw in (gr, None):
        got = R._tc_backward(ins, gt, g_raw, K=R.K64)
        ref = _tc_oracle(ins, torch.float64, gt, g_raw)
        for k in R.TC_GRADS + R.TC_SUMS:
            assert got[k].shape == ref[k].shape, k
            assert R.ratio(ref[k], got[k], got["scale_of"][k], 1e-11 / R.U) <= 1.0, k


# ------------------------------------------------------------------------------ the constants
def one_digit_up(v):
    e = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / e - 1e-9) * e


def _bump(table, k, r, where):
    if r > table.get(k, (0.0, ""))[0]:
        table[k] = (r, where)


@functools.lru_cache(maxsize=None)
def _measured():
    k9o, k9g, k10o, k10g = {}, {}, {}, {}
    for c in CASES:
        ins, _, res = case(c)
        for tag, variant in (("x", ins), ("y", R.from_y(ins))):
            ref = res if tag == "x" else R.forward(variant)
            r32 = _oracle(variant, torch.float32)
            for k in _outs(variant):
                _bump(k9o, k, R.ratio(r32[k], ref[k], ref["scale_of"][k], 1.0),
                      f"{R.case_id(c)} from {tag}")
            for name, gs in _grad_sets(c):
                g32 = _oracle(variant, torch.float32, gs)
                gref = _ref_backward(c, name) if tag == "x" else R.backward(variant, gs)
                for k, t in g32.items():
                    _bump(k9g, k, R.ratio(t, gref[k], gref["scale_of"][k], 1.0),
                          f"{R.case_id(c)} from {tag} {name}")
    for shape in R.OP_SHAPES:                    # the op-level cases: exact conv, from its y
        c = R.find_case(*shape)
        variant = R.from_y(R.exact_conv(case(c)[0]))
        ref, r32 = R.forward(variant), _oracle(variant, torch.float32)
        for k in _outs(variant):
            _bump(k9o, k, R.ratio(r32[k], ref[k], ref["scale_of"][k], 1.0),
                  f"{R.case_id(c)} exact conv")
        for name, gs in _grad_sets(c):
            g32, gref = _oracle(variant, torch.float32, gs), R.backward(variant, gs)
            _bump(k9g, "dy", R.ratio(g32["dy"], gref["dy"], gref["scale_of"]["dy"], 1.0),
                  f"{R.case_id(c)} exact conv {name}")
    tcs = [(R.tc_case_id(c), tc_case(c)[0]) for c in TC_CASES]
    for spec in R.FUSED_TC:
        c, _, tins = R.fused_tc_case(spec)
        tcs.append((R.case_id(c) + " colours", tins))
    for name, ins in tcs:
        res, r32 = R.tc_forward(ins), _tc_oracle(ins, torch.float32)
        for k in R.TC_OUTS:
            _bump(k10o, k, R.ratio(r32[k], res[k], res["scale_of"][k], 1.0), name)
        M, C, hw = ins["logits"].shape
        gt, gr = R.tc_make_grads(ins["feature"].shape[0], M, C, hw)
        for g_raw in (gr, None):
            g32, gref = _tc_oracle(ins, torch.float32, gt, g_raw), R.tc_backward(ins, gt, g_raw)
            for k in R.TC_GRADS + R.TC_SUMS:
                _bump(k10g, k, R.ratio(g32[k], gref[k], gref["scale_of"][k], 1.0),
                      name + (" g_raw" if g_raw is not None else ""))
    return k9o, k9g, k10o, k10g


def test_constants_come_from_the_fp32_oracle():
    """worst |fp32 oracle - fp64| / (2^-24 scale) per tensor over every case of the GPU
    module; each constant is 4 x the worst of its tensors, rounded up to one digit.  (dx, dw,
    db and the K10 batch sums are GEMMs and batch sums: the op-level tests add gamma(n).)"""
    k9o, k9g, k10o, k10g = _measured()
    for what, table in (("K9 output", k9o), ("K9 gradient", k9g), ("K10 output", k10o),
                        ("K10 gradient", k10g)):
        for k, (r, where) in table.items():
            print(f"{what:13s} {k:10s} worst ratio {r:.3f}  ({where})")
    for what, c_used, table in (
            ("C_OUT", R.C_OUT, {k: k9o[k] for k in R.HEAD_OUTS}), ("C_GRAD", R.C_GRAD, {"dy": k9g["dy"]}),
            ("TC_C_OUT", R.TC_C_OUT, k10o),
            ("TC_C_GRAD", R.TC_C_GRAD, {k: k10g[k] for k in R.TC_GRADS})):
        worst = max(r for r, _ in table.values())
        print(f"{what} = {c_used}: 4 x worst = {4 * worst:.3f}")
        assert c_used == one_digit_up(4 * worst), (what, worst)
        assert re.search(rf"(?<![A-Z_]){what} = {c_used:g} ", R.__doc__), what
        # the unmutated fp32 oracle is within the bar everywhere
        assert worst * 4 <= c_used
    # y is held by gamma(C + 1), whatever the summation order: the oracle's own conv within it
    for c in CASES:
        ins, _, res = case(c)
        y32 = _oracle(ins, torch.float32)["y"]
        assert R.ratio(y32, res["y"], R.y_bound(res["scale_of"]["y"], c[5]), 1 / R.U) <= 1.0


# ---------------------------------------------------------- the conditions hold for the cases
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_conditions(c):
    ins, meta, res = case(c)
    regime, B, HW, A, P, C = c[:6]
    assert R.conditions(ins, meta) == []
    s = R.groups(B, A)
    assert R.DECOMPOSITION[(B, A)] == (s, A // s)
    r32 = _oracle(ins, torch.float32)
    if regime == "saturated" and HW > 1:
        win = res["mask"].argmax(1)                                   # (B,A)
        assert float(res["mask"].max(1)[0].min()) >= 1 - 1e-20
        if HW > 32:
            assert bool((win >= 32).any()) and bool(((win < 32) & (win >= 16)).any())
        if HW > 16:
            assert bool((win % 32 >= 16).any()) and bool((win % 32 < 16).any())
        l = res["y"].view(B, HW, A, P)[..., P - 1]
        assert bool(torch.isinf(torch.exp(l.float())).any())          # no maximum: overflow
        assert float(torch.exp(l.float()).min()) < 2.0 ** -126        # ... and denormals
    if regime == "ties":
        if HW & (HW - 1) == 0:            # a power of two: exp(0) = 1, the sum HW, 1 / HW exact
            for m in (res["mask"], r32["mask"]):
                even = m[..., 0::2]
                assert bool((even == 1.0 / HW).all())
        if HW > 1 and A > 1:
            odd = res["mask"][..., 1::2]
            assert float((odd.max(1)[0] - 0.5).abs().max()) < 1e-12
            assert bool(((odd > 0.25).sum(1) == 2).all())
    if regime == "presence":
        ab = r32["absence"]
        assert bool((ab == 0).any()) and bool((ab == 1).any())
        assert bool(((ab == 0) | (ab == 1)).all())
        sg = r32["presence"]
        assert bool((sg * (1 - sg) == 0).any())                       # gradient underflow
    if regime == "wrap":
        assert 15 < float(res["pooled"][..., 2].abs().max()) <= 50
    if regime == "posesat":
        assert float(res["pooled"][..., :2].abs().min()) > 1


@pytest.mark.parametrize("c", TC_CASES, ids=TC_IDS)
def test_tc_case_conditions(c):
    ins, meta, res = tc_case(c)
    assert R.tc_conditions(ins, meta) == []
    B, M = c[1:3]
    s = R.groups(B, M)
    assert R.TC_DECOMPOSITION[(B, M)] == (s, M // s)
    margins = R.tc_kink_margins(ins)
    print(f"{R.tc_case_id(c)}: reseed {meta['reseed']}, kink margins / bound " +
          " ".join(f"{k} {v:.3g}" for k, v in margins.items()) +
          "; shares " + " ".join(f"{v:.2f}" for v in R.tc_shares(ins)))
    assert min(margins.values()) > 1
    # the fp32 oracle takes the fp64 branch everywhere: no entry is left out of a comparison
    s1 = F.linear(ins["feature"], ins["w1"], ins["b1"])
    pre2 = F.linear(torch.relu(s1), ins["w2"], ins["b2"])
    assert torch.equal(s1 > 0, res["s1"] > 0) and torch.equal(pre2 > 0, res["pre2"] > 0)
    assert torch.equal((pre2 + .99) * 6. < 6., res["pre2"] + R.K32.c99 < 1)
    if c[0] == "kinks":
        below, inside, above, on, off = R.tc_shares(ins)
        assert min(below, inside, above, on, off) >= 0.25
        lg = ins["logits"]
        if c[7] == 1 and lg.numel() >= 4:
            assert bool((lg == 0).any()) and bool((lg == 1).any())


@pytest.mark.parametrize("spec", R.FUSED_TC + [R.DECLINED_TC],
                         ids=lambda s: "x".join(map(str, s[0][1:])))
def test_fused_tc_case_conditions(spec):
    """the colour MLP built around the head reference's own features meets the kinks
    conditions, and both kernels split the case into the same groups"""
    c, ins, tins = R.fused_tc_case(spec)
    assert R.tc_conditions(tins, dict(regime="kinks")) == []
    B, A, P = c[1], c[3], c[4]
    assert tins["feature"].shape == (B, A, P - 8)
    assert R.DECOMPOSITION[(B, A)] == R.TC_DECOMPOSITION[(B, A)]
    assert (R.groups(B, A) == 1) == (spec is R.DECLINED_TC)


# ----------------------------------------------------------------------- the bar sees mistakes
def _mutant_excess(mutant, c):
    """-> (worst ratio against the bar, which tensor) of a K9 mutant on one case"""
    ins, _, res = case(c)
    mut = frozenset([mutant])
    worst, where = 0.0, ""
    bad = R._forward(ins, mut)
    for k in _outs(ins)[1:]:
        r = R.ratio(bad[k], res[k], res["scale_of"][k], R.C_OUT)
        if r > worst:
            worst, where = r, k
    for name, gs in _grad_sets(c):
        ref = _ref_backward(c, name)
        r = R.ratio(R._backward(ins, gs, mut)["dy"], ref["dy"], ref["scale_of"]["dy"], R.C_GRAD)
        if r > worst:
            worst, where = r, f"dy ({name})"
    return worst, where


def _tc_mutant_excess(mutant, c):
    ins, _, res = tc_case(c)
    mut = frozenset([mutant])
    worst, where = 0.0, ""
    bad = R._tc_forward(ins, mut)
    for k in R.TC_OUTS:
        r = R.ratio(bad[k], res[k], res["scale_of"][k], R.TC_C_OUT)
        if r > worst:
            worst, where = r, k
    gt, gr = R.tc_make_grads(*c[1:5])
    for g_raw in (gr, None):
        ref, badg = R.tc_backward(ins, gt, g_raw), R._tc_backward(ins, gt, g_raw, mut)
        for k in R.TC_GRADS + R.TC_SUMS:
            r = R.ratio(badg[k], ref[k], ref["scale_of"][k], R.TC_C_GRAD)
            if r > worst:
                worst, where = r, f"grad {k}"
    return worst, where


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_bar_sees_the_mutant(mutant):
    k9 = mutant in R.K9_MUTANTS
    caught = []
    for c in (CASES if k9 else TC_CASES):
        r, where = _mutant_excess(mutant, c) if k9 else _tc_mutant_excess(mutant, c)
        if r > 1.0:
            caught.append((R.case_id(c) if k9 else R.tc_case_id(c), r, where))
    print(f"mutant {mutant}: caught by {len(caught)} cases: " +
          "; ".join(f"{i} {r:.3g} x ({w})" for i, r, w in caught[:6]) +
          (" ..." if len(caught) > 6 else ""))
    assert caught, mutant


@functools.lru_cache(maxsize=None)
def _op_reference(shape, only):
    ins = R.exact_conv(case(R.find_case(*shape))[0])
    B, A, P = shape[1], shape[3], shape[4]
    gs = {"g_" + only: R.make_grads(B, A, P)["g_" + only]}
    return ins, gs, R.conv_backward(R.backward(R.from_y(ins), gs), ins["x"], ins["w"])


@pytest.mark.parametrize("only", ["pose", "presence", "feature"])
@pytest.mark.parametrize("shape", R.OP_SHAPES, ids=lambda s: "x".join(map(str, s[1:])))
def test_the_op_level_bar_sees_a_zeroed_doubled_or_misrouted_gradient(shape, only):
    """the bound of the GPU module's op-level test, per tensor: the conv of the case is exact
    in fp32, the fp32 oracle through autograd is within the bar, and zeros, twice the gradient
    and the gradient of a loss on another output are not"""
    ins, gs, want = _op_reference(shape, only)
    y = R.forward(ins)["y"]
    assert torch.equal(y.float().double(), y)
    y32 = F.linear(ins["x"], ins["w"], ins["bias"])
    assert torch.equal(y32.double(), y)                        # ... and torch's own order
    g32 = _oracle(ins, torch.float32, gs)
    other = _op_reference(shape, "presence" if only == "pose" else "pose")[2]
    for k in R.CONV_GRADS:
        bar = lambda t: R.ratio(t, want[k], want["bound"][k], 1 / R.U)  # noqa: E731
        rs = dict(oracle=bar(g32[k]), zeros=bar(torch.zeros_like(want[k])), twice=bar(2 * want[k]),
                  misrouted=bar(other[k]))
        print(f"{'x'.join(map(str, shape[1:]))} loss on {only}: {k} / bound " +
              " ".join(f"{n} {r:.3g}" for n, r in rs.items()))
        assert rs["oracle"] <= 1.0, (k, rs)
        assert min(rs["zeros"], rs["twice"], rs["misrouted"]) > 1.0, (k, rs)


def test_the_reference_itself_is_no_mutant():
    for c in CASES[:3]:
        assert _mutant_excess("", c)[0] == 0.0
    for c in TC_CASES[:3]:
        assert _tc_mutant_excess("", c)[0] == 0.0
