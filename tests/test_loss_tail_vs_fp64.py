"""K6, the fused loss tail (csrc/loss_tail.hip, csrc/loss_tail_dev.h), entry by entry against
the fp64 reference of tests/tail_ref.py, at the ABI level with a sentinel tail behind every
output buffer and behind the workspace: the 12-vector and the scalar, and every gradient for
each of the twelve ``gout12`` entries alone, all together, ``g_loss`` alone (``gout12`` NULL)
and both, within c[kind] 2^-24 of the entry's companion magnitude (c from the fp32
composition's own distance, tests/test_tail_ref.py) -- in the small form
(``scae_loss_tail_defer_preferred``: 512-thread combine and backward) and the large one (1024 /
256 threads, classifier-gradient blocks of 64), at the shapes where the kernels' loops change
path, for all nine (prior, posterior) sparsity-type pairs, with ``sparsity_on = 0``, without a
label, and on benign, sparse (zeros, values <= 1e-20, zero rows and columns, one-hot and
dummy-dominated posteriors), saturated-classifier and cancelling inputs.  Each case asserts the
form its id names.  The deferred form (combine inside the backward launch) and the combine on
its own must give the bits of the three-launch form.

Run with -s: each check prints its worst ratio against the bar."""
import ctypes
import functools

import pytest
import torch

from tests import tail_ref as R

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
SENT = 7.0
PAD = 37
CASES = R.all_cases()
IDS = [R.case_id(c) for c in CASES]
BY_ID = dict(zip(IDS, CASES))
SMALL = [i for i in IDS if i.startswith("small-")]
# the ABI allows the deferred form in the large form, too: one case (B and n_rec <= 512, so that
# the 512-thread combine inside the backward adds the same partial sums as the 1024-thread one)
DEFERRED = SMALL + ["large-210x24x24x10-l2-entropy-benign-nrecB+5"]
REPEAT = ["small-67x24x24x10-kl-kl-sparse-nrecB-3",
          "large-131x70x5x10-entropy-entropy-cancelling-nrecB+5"]
OP_CASES = ["small-17x7x7x10-kl-entropy-sparse-nrecB-3",
            "large-210x24x24x10-kl-l2-saturated-nrecB-3"]


def _st():
    return P(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else P(t.data_ptr())


def _padded(*shape):
    """-> (buffer with PAD sentinel entries behind it, view of the tensor); sentinels all over"""
    n = 1
    for s in shape:
        n *= int(s)
    buf = torch.full((n + PAD,), SENT, dtype=torch.float32, device="cuda")
    return buf, buf[:n].view(*shape)


def _tails_untouched(bufs):
    for name, (buf, view) in bufs.items():
        assert bool((buf[view.numel():] == SENT).all()), name


@functools.lru_cache(maxsize=None)
def case(cid):
    c = BY_ID[cid]
    ins, cfg = R.checked_case(c)
    dev = {k: None if v is None else v.contiguous().cuda() for k, v in ins.items()}
    h = R.hand(ins, cfg)
    return c, ins, cfg, dev, R.forward(ins, cfg), h["m_out"]


def _tail_args(c, cfg, dev):
    w5 = (ctypes.c_float * 5)(*cfg["weights"])
    wc = float("nan") if cfg["within_const"] is None else float(cfg["within_const"])
    ints = (c["B"], c["O"], c["M"], c["ncls"], int(cfg["n_classes_cfg"] or 0),
            R.TYPES.index(cfg["prior"]), R.TYPES.index(cfg["post"]), int(cfg["sparsity_on"]))
    ptrs = (_p(dev["lpp"]), _p(dev["posterior"]), _p(dev["caps_presence"]), _p(dev["cls_w"]),
            _p(dev["cls_b"]), _p(dev["label"]))
    return ptrs, ints, w5, wc


def _extras(cfg, dev, f):
    from torch_scae_amd import _lib
    ex = _lib.LossExtras()
    ex.rec_sums, ex.n_rec = dev["rec_sums"].data_ptr(), dev["rec_sums"].numel()
    ex.reg, ex.w_reg = dev["reg"].data_ptr(), float(cfg["w_reg"])
    ex.loss = f["loss"][1].data_ptr()
    return ex


def _forward(cid, defer=False, combine_after=False):
    """scae_loss_tail_fwd_f32 (``defer``: with defer_combine = 1; ``combine_after``: then
    scae_loss_tail_combine_f32 on its own) -> padded buffers out12, loss, ws"""
    from torch_scae_amd import _lib
    c, ins, cfg, dev, ref, m_out = case(cid)
    lib = _lib.load()
    nws = lib.scae_loss_tail_workspace_floats(c["B"], c["O"], c["ncls"])
    assert nws == c["B"] * 8 + c["B"] * c["O"] + c["B"] * 2 * max(c["ncls"], 1) + 2 * c["O"]
    f = dict(out12=_padded(12), loss=_padded(1), ws=_padded(nws))
    ptrs, ints, w5, wc = _tail_args(c, cfg, dev)
    ex = _extras(cfg, dev, f)
    ex.defer_combine = int(defer)
    _lib.call("scae_loss_tail_fwd_f32", *ptrs, ctypes.byref(ex), _p(f["out12"][1]),
              _p(f["ws"][1]), *ints, w5, wc, _st())
    torch.cuda.synchronize()
    if defer:      # nothing of the scalars exists yet
        assert bool((f["out12"][0] == SENT).all()) and bool((f["loss"][0] == SENT).all())
    if combine_after:
        ex.defer_combine = 0
        _lib.call("scae_loss_tail_combine_f32", *ptrs, ctypes.byref(ex), _p(f["out12"][1]),
                  _p(f["ws"][1]), *ints, w5, wc, _st())
        torch.cuda.synchronize()
    _tails_untouched(f)
    return f


@functools.lru_cache(maxsize=None)
def fwd_of(cid):
    return _forward(cid)


def _backward(cid, fw, gout, g_loss, defer=False):
    """scae_loss_tail_bwd_f32 on the workspace of ``fw`` (``defer``: carrying the combine, which
    writes fw's out12 and loss) -> dict of gradient tensors (cls_w / cls_b: None without label)"""
    from torch_scae_amd import _lib
    c, ins, cfg, dev, ref, m_out = case(cid)
    B, Oc, M, ncls = c["B"], c["O"], c["M"], c["ncls"]
    f = dict(lpp=_padded(B, M), posterior=_padded(B, Oc + 1, M), caps_presence=_padded(B, Oc),
             cls_w=_padded(max(ncls, 1), Oc), cls_b=_padded(max(ncls, 1)),
             rec_sums=_padded(dev["rec_sums"].numel()), reg=_padded(1))
    ptrs, ints, w5, wc = _tail_args(c, cfg, dev)
    ex = _extras(cfg, dev, fw)
    ex.g_rec_sums, ex.g_reg = f["rec_sums"][1].data_ptr(), f["reg"][1].data_ptr()
    gl = None if g_loss is None else g_loss.cuda()
    go = None if gout is None else gout.cuda()
    if gl is not None:
        ex.g_loss = gl.data_ptr()
    if defer:
        ex.defer_combine, ex.out12 = 1, fw["out12"][1].data_ptr()
    _lib.call("scae_loss_tail_bwd_f32", *ptrs, ctypes.byref(ex), _p(go), _p(fw["ws"][1]),
              _p(f["lpp"][1]), _p(f["posterior"][1]), _p(f["caps_presence"][1]),
              _p(f["cls_w"][1]), _p(f["cls_b"][1]), *ints, w5, wc, _st())
    torch.cuda.synchronize()
    _tails_untouched(f)
    _tails_untouched(fw)
    res = {k: v[1] for k, v in f.items()}
    if ncls == 0:   # without a label the classifier gradients are not written at all
        assert bool((f["cls_w"][0] == SENT).all()) and bool((f["cls_b"][0] == SENT).all())
        res["cls_w"] = res["cls_b"] = None
    return res


def _assert_form(cid):
    from torch_scae_amd import _lib
    c = BY_ID[cid]
    small = bool(_lib.load().scae_loss_tail_defer_preferred(c["B"], c["O"]))
    assert small == cid.startswith("small-") and small == R.defer_preferred(c["B"], c["O"])


def _check_out(cid, out12, what):
    c, ins, cfg, dev, ref, m_out = case(cid)
    rs = R.out_ratios(out12, ref, m_out)
    worst = max(range(12), key=lambda i: rs[i])
    print(f"{cid} {what}: worst |err| / bound {rs[worst]:.3g} ({R.OUT_NAMES[worst]}, kind "
          f"{R.OUT_KIND[worst]})")
    assert rs[worst] <= 1.0, (what, dict(zip(R.OUT_NAMES, rs)))
    o = out12.cpu()
    assert float(o[9]) == -float(o[8]) and float(o[10]) == -float(o[1])
    if not cfg["sparsity_on"]:
        assert all(float(o[i]) == 0.0 for i in (2, 3, 4, 5))
    if c["ncls"] == 0:
        assert float(o[6]) == 0.0 and float(o[7]) == 0.0
    assert float(o[11]) == float(ins["reg"][0])


def _check_grads(cid, got, gout, g_loss, what):
    c, ins, cfg, dev, ref, m_out = case(cid)
    want = R.backward(ins, cfg, gout, g_loss)
    m = R.hand(ins, cfg, gout, g_loss)["m_grads"]
    rs = R.grad_ratios(got, want, m)
    assert set(rs) == {k for k in R.GRAD_NAMES if c["ncls"] > 0 or not k.startswith("cls_")}
    k = max(rs, key=rs.get)
    print(f"{cid} {what}: worst |err| / bound {rs[k]:.3g} (g_{k}, kind {R.GRAD_KIND[k]})")
    assert rs[k] <= 1.0, (what, rs)
    # exactly zero: the posterior's dummy row; without sparsity g_cp and g_posterior
    assert float(got["posterior"][:, c["O"]].abs().max()) == 0.0
    if not cfg["sparsity_on"]:
        assert float(got["posterior"].abs().max()) == 0.0
        assert float(got["caps_presence"].abs().max()) == 0.0
    return rs


# ------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("cid", IDS)
def test_forward_vs_fp64(cid):
    _assert_form(cid)
    f = fwd_of(cid)
    _check_out(cid, f["out12"][1], "out12")
    # extras.loss receives the bits of out[0]
    assert torch.equal(f["loss"][1].view(torch.int32), f["out12"][1][:1].view(torch.int32))


# ----------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("cid", IDS)
def test_backward_each_gout_entry_alone_all_together_and_g_loss_vs_fp64(cid):
    _assert_form(cid)
    fw = fwd_of(cid)
    before = fw["out12"][0].clone()
    worst = {}
    for name, gout, g_loss in R.make_gouts(BY_ID[cid]):
        got = _backward(cid, fw, gout, g_loss)
        for k, r in _check_grads(cid, got, gout, g_loss, f"incoming {name}").items():
            worst[R.GRAD_KIND[k]] = max(worst.get(R.GRAD_KIND[k], 0.0), r)
    print(f"{cid} backward, worst share of the bar per kind: "
          + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    assert torch.equal(fw["out12"][0], before)        # the three-launch backward writes no scalar


# ------------------------------------------------------------------------------ deferred form
def _bits_equal(a, b, what):
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), what


@pytest.mark.parametrize("cid", DEFERRED)
def test_deferred_combine_gives_the_bits_of_the_three_launch_form(cid):
    _assert_form(cid)
    assert cid in IDS
    plain = fwd_of(cid)
    sets = R.make_gouts(BY_ID[cid])
    for name, gout, g_loss in (sets[-1], sets[-2]):       # g_loss + gout12; g_loss alone
        want = _backward(cid, plain, gout, g_loss)
        fw = _forward(cid, defer=True)
        got = _backward(cid, fw, gout, g_loss, defer=True)
        _bits_equal(fw["out12"][1], plain["out12"][1], (name, "out12"))
        _bits_equal(fw["loss"][1], plain["loss"][1], (name, "loss"))
        _bits_equal(fw["ws"][1], plain["ws"][1], (name, "workspace"))
        for k in R.GRAD_NAMES:
            if want[k] is None:
                assert got[k] is None
                continue
            _bits_equal(got[k], want[k], (name, k))
        _check_out(cid, fw["out12"][1], f"deferred out12 ({name})")
        _check_grads(cid, got, gout, g_loss, f"deferred, incoming {name}")
    # the combine on its own after a deferred forward
    alone = _forward(cid, defer=True, combine_after=True)
    _bits_equal(alone["out12"][1], plain["out12"][1], "combine alone: out12")
    _bits_equal(alone["loss"][1], plain["loss"][1], "combine alone: loss")


@pytest.mark.parametrize("cid", REPEAT)
def test_repeated_runs_are_bit_equal(cid):
    _assert_form(cid)
    name, gout, g_loss = R.make_gouts(BY_ID[cid])[-1]
    runs = []
    for _ in range(2):
        fw = _forward(cid)
        runs.append((fw, _backward(cid, fw, gout, g_loss)))
    (f0, g0), (f1, g1) = runs
    for k in ("out12", "loss", "ws"):
        _bits_equal(f0[k][1], f1[k][1], k)
    for k in R.GRAD_NAMES:
        _bits_equal(g0[k], g1[k], k)


# ------------------------------------------------------------- through the op and autograd
@pytest.mark.parametrize("cid", OP_CASES)
def test_loss_tail_scalar_and_autograd_vs_fp64(cid):
    """a weighted sum of the scalar and all twelve outputs through ops.loss_tail_scalar against
    fp64 autograd of the same expression: the wrapper's gout12 / g_loss plumbing"""
    from torch_scae_amd import ops
    _assert_form(cid)
    assert cid in IDS
    c, ins, cfg, dev, ref, m_out = case(cid)
    name, gout, g_loss = R.make_gouts(c)[-1]
    names = ("lpp", "posterior", "caps_presence", "cls_w", "cls_b", "rec_sums", "reg")
    lv = {k: ins[k].detach().clone().cuda().requires_grad_(True) for k in names}
    loss, out = ops.loss_tail_scalar(
        lv["lpp"], lv["posterior"], lv["caps_presence"], lv["cls_w"], lv["cls_b"], dev["label"],
        cfg["n_classes_cfg"], cfg["prior"], cfg["post"], cfg["sparsity_on"], list(cfg["weights"]),
        cfg["within_const"], rec_sums=lv["rec_sums"], reg=lv["reg"], w_reg=cfg["w_reg"])
    (loss * g_loss.cuda()[0] + (out * gout.cuda()).sum()).backward()
    torch.cuda.synchronize()
    _check_out(cid, out.detach(), "op out12")
    assert float(loss.detach()) == float(out.detach()[0])
    _check_grads(cid, {k: v.grad for k, v in lv.items()}, gout, g_loss, "op, scalar + all twelve")
