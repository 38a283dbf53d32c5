"""K9, the part-capsule head, and K10, the coloured templates, entry by entry against the fp64
reference of tests/head_ref.py: every output and every gradient within c 2^-24 of its
companion magnitude (c from the fp32 oracle's own distance, tests/test_head_ref.py), every
incoming gradient alone and together, at the ABI level with every output buffer starting as
sentinels and a sentinel tail behind it.

Every entry point: the pool-only pair, the head from a given y, the head with the 1x1 conv
inside its workgroups (whose written y is held against the fp64 conv and, fed back to the
head from y, must reproduce every output bit for bit), the step's own forms with K10 inside
the head's workgroups (bitwise equal to the separate launches; a shape they decline leaves
every output untouched), the head's backward, and K10's stand-alone pair.  The cases
(head_ref.SHAPES, POOL_SHAPES, TC_SHAPES, FUSED_TC: the smallest shapes that reach each
path, listed there with what each is for) assert their group decomposition through
``scae_attention_pool_groups`` / ``scae_template_color_partial_rows``.

Run with -s: each check prints its worst ratio against the bar."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import head_ref as R

pytestmark = pytest.mark.gpu
P_ = ctypes.c_void_p
SENT = 7.0
PAD = 37
CASES = R.all_cases()
HEAD = [c for c in CASES if c[8]]
POOL = [c for c in CASES if not c[8]]
FUSABLE = [c for c in HEAD if R.fusable(c)]
TC_CASES = R.tc_all_cases()


def _st():
    return P_(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else P_(t.data_ptr())


def _padded(*shape):
    """-> (buffer with PAD sentinel entries behind it, view of the tensor); the tensor itself
    starts out as sentinels, too"""
    n = int(np.prod(shape))
    buf = torch.full((n + PAD,), SENT, dtype=torch.float32, device="cuda")
    return buf, buf[:n].view(*shape)


def _tails_untouched(bufs):
    for name, (buf, view) in bufs.items():
        assert bool((buf[view.numel():] == SENT).all()), name


def _all_sentinels(bufs):
    for name, (buf, _) in bufs.items():
        assert bool((buf == SENT).all()), name


def _views(bufs):
    return {k: v[1] for k, v in bufs.items()}


def _cuda(t):
    return None if t is None else t.contiguous().cuda()


def _decomposition(B, A, table=R.DECOMPOSITION, tc=False):
    """the case's groups x group size, asserted through the library's own answer"""
    from torch_scae_amd import _lib
    lib = _lib.load()
    s = lib.scae_template_color_partial_rows(B, A) // B if tc else \
        lib.scae_attention_pool_groups(B, A)
    assert s == R.groups(B, A) and table[(B, A)] == (s, A // s), (B, A, s)
    return s


@functools.lru_cache(maxsize=None)
def case(c):
    """-> (ins from x, its reference, ins from the y an exact conv hands over, its reference)"""
    ins, meta = R.checked_case(*c)
    yins = R.from_y(ins)
    return ins, R.forward(ins), yins, R.forward(yins)


def _line(what, rs):
    print(f"{what}: |err| / bound " + " ".join(f"{k} {r:.2g}" for k, r in rs.items()))


def _new_head_outs(B, A, P):
    f = dict(pooled=_padded(B, A, P - 1), pose=_padded(B, A, 6), presence=_padded(B, A),
             absence=_padded(B, A))
    if P > 8:
        f["feature"] = _padded(B, A, P - 8)
    return f


def _head_args(ins, f, c):
    B, HW, A, P = c[1:5]
    return (_p(_cuda(ins["noise_u"])), float(ins["noise_scale"]), int(ins["similarity"]),
            _p(f["pooled"][1]), _p(f["pose"][1]), _p(f["presence"][1]),
            _p(f["feature"][1]) if P > 8 else None, _p(f["absence"][1]), B, HW, A, P)


def _head_fwd(ins, y, c):
    from torch_scae_amd import _lib
    f = _new_head_outs(c[1], c[3], c[4])
    _lib.call("scae_capsule_head_fwd_f32", _p(y), *_head_args(ins, f, c), _st())
    torch.cuda.synchronize()
    _tails_untouched(f)
    return _views(f)


def _check_head(out, ref, what):
    rs = {k: R.ratio(out[k], ref[k], ref["scale_of"][k], R.C_OUT) for k in R.HEAD_OUTS
          if k in out}
    _line(what, rs)
    assert max(rs.values()) <= 1.0, (what, rs)
    assert torch.equal(out["absence"], 1.0 - out["presence"])     # of its own presence


# --------------------------------------------------------------------- the pool-only pair
@pytest.mark.parametrize("c", POOL, ids=R.case_id)
def test_attention_pool_forward_and_backward_vs_fp64(c):
    from torch_scae_amd import _lib
    _, _, yins, ref = case(c)
    regime, B, HW, A, P = c[:5]
    _decomposition(B, A)
    y = yins["y"].cuda()
    out = _padded(B, A, P - 1)
    _lib.call("scae_attention_pool_fwd_f32", _p(y), _p(out[1]), B, HW, A, P, _st())
    g = R.make_grads(B, A, P)["g"]
    dy = _padded(B, HW, A * P)
    _lib.call("scae_attention_pool_bwd_f32", _p(y), _p(g.cuda()), _p(dy[1]), B, HW, A, P, _st())
    torch.cuda.synchronize()
    _tails_untouched(dict(out=out, dy=dy))
    want = R.backward(yins, dict(g=g))
    rs = dict(pooled=R.ratio(out[1], ref["pooled"], ref["scale_of"]["pooled"], R.C_OUT),
              dy=R.ratio(dy[1], want["dy"], want["scale_of"]["dy"], R.C_GRAD))
    _line(R.case_id(c), rs)
    assert max(rs.values()) <= 1.0, rs
    if regime == "ties" and HW & (HW - 1) == 0:
        # all logits equal: the mask is exactly 1 / HW, so dy's feature columns are g / HW
        got = dy[1].view(B, HW, A, P)[:, :, 0::2, :P - 1].cpu()
        assert torch.equal(got, (g[:, 0::2] * (1.0 / HW)).unsqueeze(1).expand_as(got))


# ------------------------------------------------------------------ the head from a given y
@pytest.mark.parametrize("c", HEAD, ids=R.case_id)
def test_head_forward_from_y_vs_fp64(c):
    _, _, yins, ref = case(c)
    _decomposition(c[1], c[3])
    out = _head_fwd(yins, yins["y"].cuda(), c)
    _check_head(out, ref, R.case_id(c))


def _head_bwd(ins, y, pooled, grads, c):
    from torch_scae_amd import _lib
    B, HW, A, P = c[1:5]
    dy = _padded(B, HW, A * P)
    g = [_cuda(grads.get(k)) for k in R.GRAD_NAMES]
    _lib.call("scae_capsule_head_bwd_f32", _p(y), _p(pooled), _p(_cuda(ins["noise_u"])),
              float(ins["noise_scale"]), int(ins["similarity"]), *[_p(t) for t in g], _p(dy[1]),
              B, HW, A, P, _st())
    torch.cuda.synchronize()
    _tails_untouched(dict(dy=dy))
    return dy[1]


@pytest.mark.parametrize("c", HEAD, ids=R.case_id)
def test_head_backward_each_incoming_gradient_alone_and_together_vs_fp64(c):
    _, _, yins, ref = case(c)
    regime, B, HW, A, P = c[:5]
    _decomposition(B, A)
    y = yins["y"].cuda()
    pooled = _head_fwd(yins, y, c)["pooled"]
    grads = R.make_grads(B, A, P)
    acc = {}
    for name, gs in R.subsets(grads, P):
        dy = _head_bwd(yins, y, pooled, gs, c)
        want = R.backward(yins, gs)
        r = R.ratio(dy, want["dy"], want["scale_of"]["dy"], R.C_GRAD)
        acc[name] = r
        assert r <= 1.0, (R.case_id(c), name, r)
        if regime == "ties" and HW & (HW - 1) == 0 and name == "g_feature":
            got = dy.view(B, HW, A, P)[:, :, 0::2, 7:P - 1].cpu()
            assert torch.equal(got, (gs[name][:, 0::2] * (1.0 / HW)).unsqueeze(1).expand_as(got))
    _line(f"{R.case_id(c)} dy per incoming", acc)
    # no gradient at all: zeros, exactly
    assert float(_head_bwd(yins, y, pooled, {}, c).abs().max()) == 0.0


# ------------------------------------------------- the 1x1 conv inside the head's workgroups
def _conv_fwd(ins, c):
    from torch_scae_amd import _lib
    B, HW, A, P, C = c[1:6]
    x, w, b = (_cuda(ins[k]) for k in ("x", "w", "bias"))
    assert _lib.load().scae_capsule_head_conv_supported(HW, A, P, C)
    f = _new_head_outs(B, A, P)
    f["y"] = _padded(B, HW, A * P)
    _lib.call("scae_capsule_head_conv_fwd_f32", _p(x), _p(w), _p(b), C, _p(f["y"][1]),
              *_head_args(ins, f, c), _st())
    torch.cuda.synchronize()
    _tails_untouched(f)
    return _views(f), (x, w, b)


@pytest.mark.parametrize("c", FUSABLE, ids=R.case_id)
def test_head_with_the_conv_inside_vs_fp64(c):
    ins, ref, _, _ = case(c)
    _decomposition(c[1], c[3])
    out, _ = _conv_fwd(ins, c)
    ry = R.ratio(out["y"], ref["y"], R.y_bound(ref["scale_of"]["y"], c[5]), 1 / R.U)
    print(f"{R.case_id(c)}: y |err| / (gamma(C + 1) scale) {ry:.2g}")
    assert ry <= 1.0
    _check_head(out, ref, R.case_id(c))
    # the same code on the same values: the head from the y just written, bit for bit
    again = _head_fwd(ins, out["y"], c)
    for k in again:
        assert torch.equal(again[k], out[k]), k


# ------------------------------------------------------ K10 inside the head's workgroups
def _tc_dev(tins):
    return {k: _cuda(tins[k]) for k in ("logits", "feature", "w1", "b1", "w2", "b2")}


def _tc_new_outs(B, M, C, hw):
    return dict(raw=_padded(M, C, hw), templates=_padded(B, M, C, hw), color=_padded(B, M, C))


def _tc_dims(tins):
    M, C, hw = tins["logits"].shape
    B, _, F = tins["feature"].shape
    return B, M, C, hw, F, tins["w1"].shape[0]


def _tc_fwd(tins, feature=None):
    from torch_scae_amd import _lib
    B, M, C, hw, F, H1 = _tc_dims(tins)
    d = _tc_dev(tins)
    f = _tc_new_outs(B, M, C, hw)
    _lib.call("scae_template_color_fwd_f32", _p(d["logits"]),
              _p(d["feature"] if feature is None else feature),
              *[_p(d[k]) for k in ("w1", "b1", "w2", "b2")], _p(f["raw"][1]),
              _p(f["templates"][1]), _p(f["color"][1]), B, M, C, hw, F, H1, tins["tnl"],
              tins["cnl"], _st())
    torch.cuda.synchronize()
    _tails_untouched(f)
    return _views(f)


def _check_tc_forward(out, tins, regime, what):
    """against the reference on ``tins`` (whose conditions must hold: no entry is left out)"""
    assert R.tc_conditions(tins, dict(regime=regime)) == [], what
    ref = R.tc_forward(tins)
    rs = {k: R.ratio(out[k], ref[k], ref["scale_of"][k], R.TC_C_OUT) for k in R.TC_OUTS}
    _line(what, rs)
    assert max(rs.values()) <= 1.0, (what, rs)


def _conv_tc_args(ins, tins, f, c, xwb):
    B, M, C, hw, F, H1 = _tc_dims(tins)
    d = _tc_dev(tins)
    return (*[_p(t) for t in xwb], c[5], _p(f["y"][1]), *_head_args(ins, f, c),
            _p(d["logits"]), *[_p(d[k]) for k in ("w1", "b1", "w2", "b2")], _p(f["raw"][1]),
            _p(f["templates"][1]), _p(f["color"][1]), C, hw, F, H1, tins["tnl"], tins["cnl"],
            _st()), d


@pytest.mark.parametrize("spec", R.FUSED_TC, ids=lambda s: "x".join(map(str, s[0][1:])))
def test_head_conv_with_the_colour_mlp_behind_vs_fp64_and_the_separate_launches(spec):
    from torch_scae_amd import _lib
    c, ins, tins = R.fused_tc_case(spec)
    ref = case(c)[1]
    B, HW, A, P = c[1:5]
    s = _decomposition(B, A)
    assert s > 1 and _decomposition(B, A, R.TC_DECOMPOSITION, tc=True) == s
    sep, xwb = _conv_fwd(ins, c)
    B, M, C, hw, F, H1 = _tc_dims(tins)
    f = _new_head_outs(B, A, P)
    f.update(_tc_new_outs(B, M, C, hw), y=_padded(B, HW, A * P))
    args, alive = _conv_tc_args(ins, tins, f, c, xwb)
    _lib.call("scae_capsule_head_conv_fwd_tc_f32", *args)
    torch.cuda.synchronize()
    del alive                                  # (the device copies the arguments point to)
    _tails_untouched(f)
    out = _views(f)
    _check_head(out, ref, R.case_id(c) + " +tc")
    # the reference of K10 on the features the head itself wrote
    tins = dict(tins, feature=out["feature"].cpu())
    _check_tc_forward(out, tins, "kinks", f"{R.case_id(c)} +tc {M}x{C}x{hw}")
    # every sum has one owner: the bits of the separate launches
    sep.update(_tc_fwd(tins, feature=sep["feature"]))
    for k in out:
        assert torch.equal(out[k], sep[k]), k


def test_head_conv_with_the_colour_mlp_declines_one_group_per_image():
    from torch_scae_amd import _lib
    c, ins, tins = R.fused_tc_case(R.DECLINED_TC)
    B, HW, A, P = c[1:5]
    assert _decomposition(B, A) == 1
    B, M, C, hw, F, H1 = _tc_dims(tins)
    xwb = tuple(_cuda(ins[k]) for k in ("x", "w", "bias"))
    f = _new_head_outs(B, A, P)
    f.update(_tc_new_outs(B, M, C, hw), y=_padded(B, HW, A * P))
    args, alive = _conv_tc_args(ins, tins, f, c, xwb)
    rc = _lib.load().scae_capsule_head_conv_fwd_tc_f32(*args)
    torch.cuda.synchronize()
    del alive
    assert rc == _lib.ERR_UNSUPPORTED
    _all_sentinels(f)


def _tc_bwd_bufs(B, M, C, hw, F, H1):
    from torch_scae_amd import _lib
    rows = _lib.load().scae_template_color_partial_rows(B, M)
    return dict(g_logits=_padded(M, C, hw), g_feature=_padded(B, M, F),
                partial=_padded(rows, H1 * F + H1 + C * H1 + C))


def _check_tc_backward(got, tins, gt, g_raw, what):
    B, M, C, hw, F, H1 = _tc_dims(tins)
    want = R.tc_backward(tins, gt, g_raw)
    rs = {k: R.ratio(got[k], want[k], want["scale_of"][k], R.TC_C_GRAD) for k in R.TC_GRADS}
    # the partial rows [dW1 | db1 | dW2 | db2], summed in fp64: a row is an fp32 sum over its
    # group's capsules (gamma(group size) of the summed companions on top of the bar)
    sums = got["partial"].double().sum(0).cpu()
    Mg = M // R.groups(B, M)
    pos = 0
    for k in R.TC_SUMS:
        n = want[k].numel()
        bound = (R.TC_C_GRAD * R.U + R.gamma(Mg)) * want["scale_of"][k]
        rs[k] = R.ratio(sums[pos:pos + n].view(want[k].shape), want[k], bound, 1 / R.U)
        pos += n
    assert pos == sums.numel()
    _line(what, rs)
    assert max(rs.values()) <= 1.0, (what, rs)


@pytest.mark.parametrize("spec", R.FUSED_TC, ids=lambda s: "x".join(map(str, s[0][1:])))
def test_head_backward_with_the_colour_mlp_in_front_vs_fp64(spec):
    from torch_scae_amd import _lib
    c, ins, tins = R.fused_tc_case(spec)
    yins = case(c)[2]
    B, HW, A, P = c[1:5]
    s = _decomposition(B, A)
    assert s > 1 and _decomposition(B, A, R.TC_DECOMPOSITION, tc=True) == s
    y = yins["y"].cuda()
    head = _head_fwd(yins, y, c)
    tins = dict(tins, feature=head["feature"].cpu())
    B, M, C, hw, F, H1 = _tc_dims(tins)
    fwd = _tc_fwd(tins)
    _check_tc_forward(fwd, tins, "kinks", f"{R.case_id(c)} colours {M}x{C}x{hw}")
    gt, gr = R.tc_make_grads(B, M, C, hw)
    grads = {k: v for k, v in R.make_grads(B, A, P).items() if k in R.GRAD_NAMES[:3]}
    d = _tc_dev(tins)
    for g_raw in (gr, None):
        f = _tc_bwd_bufs(B, M, C, hw, F, H1)
        f["dy"] = _padded(B, HW, A * P)
        dev = [_cuda(grads[k]) for k in R.GRAD_NAMES[:3]] + [gt.cuda(), _cuda(g_raw)]
        _lib.call("scae_capsule_head_bwd_tc_f32", _p(y), _p(head["pooled"]),
                  _p(_cuda(yins["noise_u"])), float(yins["noise_scale"]),
                  int(yins["similarity"]), *[_p(t) for t in dev[:3]], _p(f["dy"][1]), B, HW, A,
                  P, _p(d["logits"]), _p(d["feature"]),
                  *[_p(d[k]) for k in ("w1", "b1", "w2", "b2")], _p(fwd["color"]), _p(dev[3]),
                  _p(dev[4]), _p(f["g_logits"][1]), _p(f["g_feature"][1]), _p(f["partial"][1]),
                  C, hw, F, H1, tins["tnl"], tins["cnl"], _st())
        torch.cuda.synchronize()
        _tails_untouched(f)
        got = _views(f)
        what = f"{R.case_id(c)} bwd_tc" + (" g_raw" if g_raw is not None else "")
        _check_tc_backward(got, tins, gt, g_raw, what)
        # the head's part: its g_feature2 is the colour MLP's feature gradient, as written
        want = R.backward(yins, dict(grads, g_feature2=got["g_feature"].cpu()))
        r = R.ratio(got["dy"], want["dy"], want["scale_of"]["dy"], R.C_GRAD)
        print(f"{what}: dy |err| / bound {r:.2g}")
        assert r <= 1.0, (what, r)


def test_head_backward_with_the_colour_mlp_declines_one_group_per_image():
    from torch_scae_amd import _lib
    c, ins, tins = R.fused_tc_case(R.DECLINED_TC)
    yins, ref = case(c)[2:]
    B, HW, A, P = c[1:5]
    assert _decomposition(B, A) == 1
    B, M, C, hw, F, H1 = _tc_dims(tins)
    d = _tc_dev(tins)
    y, pooled = yins["y"].cuda(), ref["pooled"].float().cuda()
    color = R.tc_forward(tins)["color"].float().cuda()
    gt = R.tc_make_grads(B, M, C, hw)[0].cuda()
    f = _tc_bwd_bufs(B, M, C, hw, F, H1)
    f["dy"] = _padded(B, HW, A * P)
    rc = _lib.load().scae_capsule_head_bwd_tc_f32(
        _p(y), _p(pooled), None, 0.0, int(yins["similarity"]), None, None, None,
        _p(f["dy"][1]), B, HW, A, P, _p(d["logits"]), _p(d["feature"]),
        *[_p(d[k]) for k in ("w1", "b1", "w2", "b2")], _p(color), _p(gt), None,
        _p(f["g_logits"][1]), _p(f["g_feature"][1]), _p(f["partial"][1]), C, hw, F, H1,
        tins["tnl"], tins["cnl"], _st())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED
    _all_sentinels(f)


# ------------------------------------------------------------------ K10's stand-alone pair
@functools.lru_cache(maxsize=None)
def tc_case(c):
    return R.tc_checked_case(*c)[0]


@pytest.mark.parametrize("c", TC_CASES, ids=R.tc_case_id)
def test_template_color_forward_vs_fp64(c):
    tins = tc_case(c)
    _decomposition(c[1], c[2], R.TC_DECOMPOSITION, tc=True)
    _check_tc_forward(_tc_fwd(tins), tins, c[0], R.tc_case_id(c))


@pytest.mark.parametrize("c", TC_CASES, ids=R.tc_case_id)
def test_template_color_backward_with_and_without_g_raw_vs_fp64(c):
    from torch_scae_amd import _lib
    tins = tc_case(c)
    B, M, C, hw, F, H1 = _tc_dims(tins)
    _decomposition(B, M, R.TC_DECOMPOSITION, tc=True)
    d = _tc_dev(tins)
    color = _tc_fwd(tins)["color"]
    gt, gr = R.tc_make_grads(B, M, C, hw)
    for g_raw in (gr, None):
        f = _tc_bwd_bufs(B, M, C, hw, F, H1)
        dev = (gt.cuda(), _cuda(g_raw))
        _lib.call("scae_template_color_bwd_f32", _p(d["logits"]), _p(d["feature"]),
                  *[_p(d[k]) for k in ("w1", "b1", "w2", "b2")], _p(color), _p(dev[0]),
                  _p(dev[1]), _p(f["g_logits"][1]), _p(f["g_feature"][1]), _p(f["partial"][1]),
                  B, M, C, hw, F, H1, tins["tnl"], tins["cnl"], _st())
        torch.cuda.synchronize()
        _tails_untouched(f)
        _check_tc_backward(_views(f), tins, gt, g_raw,
                           R.tc_case_id(c) + (" g_raw" if g_raw is not None else ""))


# ---------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("only", ["pose", "presence", "feature"])
@pytest.mark.parametrize("shape", R.OP_SHAPES, ids=lambda s: "x".join(map(str, s[1:])))
def test_op_capsule_head_with_a_loss_on_one_output_vs_fp64(shape, only):
    """autograd hands None for the other two outputs.  The case is ``exact_conv``: the y the op
    computes for itself is the fp64 y bit for bit in any summation order, so the outputs and dy
    are held by the sharp from-y reference, and dx, dw, db by dy's companions pushed through
    the conv plus gamma(n) for the n-term sums (``head_ref.conv_backward``;
    test_head_ref.py shows that zeros, a doubled and a misrouted gradient exceed this bar for
    every shape, loss and tensor)."""
    from torch_scae_amd import ops
    c = R.find_case(*shape)
    ins = R.exact_conv(R.checked_case(*c)[0])
    yins = R.from_y(ins)
    ref = R.forward(yins)
    assert torch.equal(yins["y"].double(), R.forward(ins)["y"])
    B, HW, A, P, C = c[1:6]
    _decomposition(B, A)
    lv = {k: ins[k].clone().cuda().requires_grad_() for k in ("x", "w", "bias")}
    pose, pres, feat, absence = ops.capsule_head(lv["x"], lv["w"], lv["bias"], A,
                                                 _cuda(ins["noise_u"]), ins["noise_scale"],
                                                 bool(ins["similarity"]))
    out = dict(pose=pose, presence=pres, feature=feat)
    rs = {k: R.ratio(t, ref[k], ref["scale_of"][k], R.C_OUT) for k, t in out.items()}
    assert torch.equal(absence.view(B, A), 1.0 - pres.detach())
    grads = R.make_grads(B, A, P)
    (out[only] * grads["g_" + only].cuda()).sum().backward()
    torch.cuda.synchronize()
    want = R.conv_backward(R.backward(yins, {"g_" + only: grads["g_" + only]}), ins["x"], ins["w"])
    for k, name in (("dx", "x"), ("dw", "w"), ("db", "bias")):
        rs[k] = R.ratio(lv[name].grad, want[k], want["bound"][k], 1 / R.U)
    _line(f"ops.capsule_head {R.case_id(c)} loss on {only}", rs)
    assert max(rs.values()) <= 1.0, rs


def test_op_template_generator_parameter_gradients_at_group_size_six_vs_fp64():
    from torch_scae_amd.part_decoder import TemplateGenerator
    c = ("kinks", 3, 42, 3, 63, 16, 32, 1, 1)
    assert c in TC_CASES
    tins = tc_case(c)
    B, M, C, hw, F, H1 = _tc_dims(tins)
    assert _decomposition(B, M, R.TC_DECOMPOSITION, tc=True) == 7
    tg = TemplateGenerator(M, C, (7, 9), template_nonlin="relu1", dim_feature=F,
                           colorize_templates=True, color_nonlin="relu1")
    with torch.no_grad():
        tg.template_logits.copy_(tins["logits"].view(1, M, C, 7, 9))
        for i, (w, b) in ((0, ("w1", "b1")), (2, ("w2", "b2"))):
            tg.templates_color_mlp[i].weight.copy_(tins[w])
            tg.templates_color_mlp[i].bias.copy_(tins[b])
    tg = tg.cuda()
    feature = tins["feature"].cuda().requires_grad_()
    out = tg(feature=feature)
    gt, gr = R.tc_make_grads(B, M, C, hw)
    ((out.templates.view(B, M, C, hw) * gt.cuda()).sum() +
     (out.raw_templates.view(M, C, hw) * gr.cuda()).sum()).backward()
    torch.cuda.synchronize()
    want = R.tc_backward(tins, gt, gr)
    mlp = tg.templates_color_mlp
    got = dict(g_logits=tg.template_logits.grad.view(M, C, hw), g_feature=feature.grad,
               dW1=mlp[0].weight.grad, db1=mlp[0].bias.grad, dW2=mlp[2].weight.grad,
               db2=mlp[2].bias.grad)
    rs = {}
    for k, g in got.items():
        # (the batch sums: B M fp32 terms in the partial rows and their sum)
        extra = R.gamma(B * M) if k in R.TC_SUMS else 0.0
        rs[k] = R.ratio(g, want[k], (R.TC_C_GRAD * R.U + extra) * want["scale_of"][k], 1 / R.U)
    _line("TemplateGenerator " + R.tc_case_id(c), rs)
    assert max(rs.values()) <= 1.0, rs
