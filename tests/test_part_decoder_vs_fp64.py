"""K1, the part decoder (csrc/render_gmm.hip, render_gmm_wave.hip, render_gmm_wave_dev.h,
render_gmm_mode.hip), entry by entry against the fp64 reference of tests/k1_ref.py: every
output and every gradient the ABI returns within c 2^-24 of its companion magnitude (c from
the fp32 oracle's own distance, tests/test_k1_ref.py), at the ABI level, in every form the
dispatch takes -- each case names the forms it is there for and asserts them against
scae_render_gmm_forms before anything is compared.  Every output buffer carries a sentinel
tail.  Nothing is masked out of a comparison.

Run with -s: each check prints its worst ratio against the bar."""
import ctypes
import functools

import pytest
import torch

from tests import k1_ref as R
from tests.test_capsule_likelihood_vs_fp64 import P, _p, _padded, _st, _tails_untouched

pytestmark = pytest.mark.gpu
CASES = R.all_cases()


def _ids(flag):
    return [c["name"] for c in CASES if flag in c["checks"]]


@functools.lru_cache(maxsize=2)
def setup(name):
    """-> (case, fp32 inputs, HW, device tensors, descriptor)"""
    from torch_scae_amd import _lib
    c = next(c for c in CASES if c["name"] == name)
    inputs = None
    if c["poses"] == "init":
        from tests.test_hip_ops import _regime_inputs
        inputs = _regime_inputs("init", c["B"], c["M"], c["C"], c["HW"],
                                torch.Generator().manual_seed(17))
    ins, HW = R.checked_case(c, inputs=inputs)
    dev = {k: None if v is None else v.contiguous().cuda() for k, v in ins.items()}
    B0, M, C, th, tw = ins["templates"].shape
    B = ins["pose"].shape[0]
    d = _lib.DecoderDesc(_p(dev["templates"]), _p(dev["alpha"]), _p(dev["pose"]),
                         _p(dev["presence"]), _p(dev["bg_image"]), _p(dev["bg_value"]),
                         _p(dev["bg_mixing_logit"]), _p(dev["temperature_logit"]),
                         _p(dev["scale"]), B, M, C, th, tw, HW[0], HW[1], B // B0)
    return c, ins, HW, dev, d


def _forms(d, fused, tt=None, ml=None):
    from torch_scae_amd import _lib
    out = (ctypes.c_int * 12)()
    rc = _lib.load().scae_render_gmm_forms(ctypes.byref(d), fused, _p(tt) or P(4096),
                                           _p(ml) or P(4096), out)
    assert rc == 0, rc
    return dict(fwd=(out[0], out[1], out[2]), render=out[3], bwd=out[4], gather_rows=out[5],
                chunk_rows=out[6], ppb=out[7], item_budget=out[8], max_items=out[9])


def _check(name, what, got, ref, mag, c):
    r = R.ratio(got, ref, mag, c)
    print(f"{name} {what}: worst |err| / bound {r:.3g}")
    assert r <= 1.0, (name, what, r)


# ------------------------------------------------------------------------------------- render
def _render(d, dev, c, HW, offset=0):
    from torch_scae_amd import _lib
    B, K, C, Pn = c["B"], c["M"] + 1, c["C"], HW[0] * HW[1]
    Cm = 1 if c["alpha"] else C
    n_tt, n_ml = B * K * C * Pn, B * K * Cm * Pn
    # ``offset`` floats in front of tt: the view is then off 16-byte alignment
    buf = torch.full((offset + n_tt + 37,), 7.0, device="cuda")
    tt = buf[offset:offset + n_tt].view(B, K, C, Pn)
    mlb, ml = _padded(B, K, Cm, Pn)
    assert _forms(d, 1, tt, ml)["render"] == (R.CLASSIC if offset % 4 else c["render"])
    _lib.call("scae_template_render_fwd_f32", ctypes.byref(d), _p(tt), _p(ml), _st())
    torch.cuda.synchronize()
    _tails_untouched(dict(ml=(mlb, ml)))
    assert bool((buf[:offset] == 7.0).all()) and bool((buf[offset + n_tt:] == 7.0).all())
    return tt, ml


@pytest.mark.parametrize("name", _ids("R"))
def test_render_vs_fp64(name):
    c, ins, HW, dev, d = setup(name)
    ref = R.forward(ins, HW, want=("tt", "ml"))
    for offset in (0, 1) if name == "wave-1wave-tiles" else (0,):
        tt, ml = _render(d, dev, c, HW, offset)
        tag = "" if not offset else " (output off 16-byte alignment)"
        _check(name, "transformed_templates" + tag, tt, ref["tt"], ref["m_tt"], R.C_OUT["tt"])
        _check(name, "mixing_logits" + tag, ml, ref["ml"], ref["m_ml"], R.C_OUT["ml"])


# --------------------------------------------------------------------------------- likelihood
def _logprob(d, dev, c, HW):
    from torch_scae_amd import _lib
    B, C, Pn = c["B"], c["C"], HW[0] * HW[1]
    Cm = 1 if c["alpha"] else C
    f = dict(log_prob=_padded(B, C, Pn), lse_post=_padded(B, C, Pn), lse_prior=_padded(B, Cm, Pn))
    _lib.call("scae_render_gmm_logprob_fwd_f32", ctypes.byref(d), _p(dev["x"]),
              *[_p(f[k][1]) for k in f], _st())
    torch.cuda.synchronize()
    _tails_untouched(f)
    return {k: v[1] for k, v in f.items()}


def _logprob_sums(d, dev, c, HW):
    from torch_scae_amd import _lib
    B, C, Pn = c["B"], c["C"], HW[0] * HW[1]
    Cm = 1 if c["alpha"] else C
    tiles = _lib.load().scae_render_gmm_logprob_tiles(ctypes.byref(d))
    f = dict(tile_sums=_padded(B, tiles), lse_post=_padded(B, C, Pn), lse_prior=_padded(B, Cm, Pn))
    _lib.call("scae_render_gmm_logprob_sums_fwd_f32", ctypes.byref(d), _p(dev["x"]),
              *[_p(f[k][1]) for k in f], _st())
    torch.cuda.synchronize()
    _tails_untouched(f)
    return {k: v[1] for k, v in f.items()}, tiles


@pytest.mark.parametrize("name", _ids("F"))
def test_likelihood_forward_vs_fp64(name):
    from torch_scae_amd import _lib
    c, ins, HW, dev, d = setup(name)
    B, C, Pn = c["B"], c["C"], HW[0] * HW[1]
    form = _forms(d, 1)
    assert form["fwd"] == c["fwd"], form
    if "ppb" in c:
        assert form["ppb"] == c["ppb"], form
    ref = R.forward(ins, HW, want=("log_prob", "lse_post", "lse_prior", "mean"))
    out = _logprob(d, dev, c, HW)
    for k in ("log_prob", "lse_post", "lse_prior"):
        _check(name, k, out[k], ref[k], ref["m_" + k], R.C_OUT[k])
    sums, tiles = _logprob_sums(d, dev, c, HW)
    assert tiles == -(-Pn // form["ppb"])
    s, m = R.tile_sums(ref["log_prob"], ref["m_log_prob"], tiles, form["ppb"])
    _check(name, "tile sums", sums["tile_sums"], s, m, R.C_OUT["tile_sums"])
    for k in ("lse_post", "lse_prior"):
        _check(name, k + " (sums call)", sums[k], ref[k], ref["m_" + k], R.C_OUT[k])
    # mean and mode from the compact inputs
    for what in (1, 0):
        buf, o = _padded(B, C, Pn)
        _lib.call("scae_render_gmm_mode_f32", ctypes.byref(d), _p(o), what, 0, B, _st())
        torch.cuda.synchronize()
        _tails_untouched(dict(o=(buf, o)))
        if what:
            _check(name, "mean", o, ref["mean"], ref["m_mean"], R.C_OUT["mean"])
        else:
            r = R.mode_error(o, ins, HW)
            print(f"{name} mode: worst |err| / bound {r:.3g}")
            assert r <= 1.0, (name, "mode", r)


@pytest.mark.parametrize("name", ["wave-ragged-C3", "classic-ks4-pad", "presence-0-1e-18-1"])
def test_generic_mean_and_mode_vs_fp64(name):
    """scae_gmm_mean_f32 / scae_gmm_mode_f32 (and maximum=True where the reference allows it)
    on the rendered tensors"""
    from torch_scae_amd import _lib
    c, ins, HW, dev, d = setup(name)
    B, K, C, Pn = c["B"], c["M"] + 1, c["C"], HW[0] * HW[1]
    Cm = 1 if c["alpha"] else C
    tt, ml = _render(d, dev, c, HW)
    # the reference is taken on the kernel's own rendered fp32 tensors: they are this entry
    # point's inputs, exact as given
    mean, m_mean = R.mixture_mean(tt, ml)
    sigma = torch.ones(1, device="cuda")
    buf, o = _padded(B, C, Pn)
    _lib.call("scae_gmm_mean_f32", _p(tt), _p(ml), _p(o), B, K, C, Cm, Pn, _st())
    torch.cuda.synchronize()
    _tails_untouched(dict(o=(buf, o)))
    _check(name, "generic mean", o, mean, m_mean, R.C_OUT["mean"])
    for maximum in (0, 1):
        if maximum and Cm == 1 and C > 1:
            continue          # the reference raises there, and so does the entry point
        buf, o = _padded(B, C, Pn)
        _lib.call("scae_gmm_mode_f32", _p(tt), _p(ml), _p(sigma), _p(o), maximum, B, K, C, Cm,
                  Pn, _st())
        torch.cuda.synchronize()
        _tails_untouched(dict(o=(buf, o)))
        # maximum=False: torch.argmax's component, bit for bit.  maximum=True adds
        # log N(loc; loc, sigma) = -log sigma - log sqrt(2 pi), the same for every component
        # (the reference has one sigma): the arg-max can only move between logits that the
        # fp32 sum ml + constant rounds together, 2 roundings of 2^-24 (|ml| + 1)
        assert R.mixture_mode_ok(o, tt, ml, slack=4 * R.U if maximum else 0.0), (name, maximum)
        print(f"{name} generic mode(maximum={bool(maximum)}): the arg-max component's bits")


# ----------------------------------------------------------------------------------- backward
def _bwd(d, dev, c, HW, saved, g_logprob=None, g_tt=None, g_ml=None, g_tile=None):
    from torch_scae_amd import _lib
    B, M, C = c["B"], c["M"], c["C"]
    th, tw = c["ts"]
    f = dict(templates=_padded(B, M, C, th, tw), pose=_padded(B, M, 6),
             scalar_partial=_padded(B, M + 1, 4))
    if c["alpha"]:
        f["alpha_partial"] = _padded(B, M, th, tw)
    if dev["presence"] is not None:
        f["presence"] = _padded(B, M)
    if dev["bg_image"] is not None:
        f["bg_image"] = _padded(B, C, HW[0] * HW[1])
    o = lambda k: _p(f[k][1]) if k in f else None       # noqa: E731
    outs = (o("templates"), o("alpha_partial"), o("pose"), o("presence"), o("bg_image"),
            o("scalar_partial"))
    fused = g_tt is None and g_ml is None
    sv = [_p(dev["x"]), _p(saved["lse_post"]), _p(saved["lse_prior"])] if fused else [None] * 3
    if g_tile is not None:
        _lib.call("scae_render_gmm_sums_bwd_f32", ctypes.byref(d), *sv, _p(g_tile), *outs, _st())
    else:
        _lib.call("scae_render_gmm_bwd_f32", ctypes.byref(d), *sv, _p(g_logprob), _p(g_tt),
                  _p(g_ml), *outs, _st())
    torch.cuda.synchronize()
    _tails_untouched(f)
    return {k: v[1] for k, v in f.items()}


def _compare_grads(name, what, got, ref, mag):
    assert set(got) == set(ref), (set(got), set(ref))
    rs = {k: R.ratio(got[k], ref[k], mag[k], R.C_GRAD[k]) for k in ref}
    print(f"{name} {what}: worst |err| / bound "
          + "  ".join(f"{k} {v:.3g}" for k, v in rs.items()))
    assert max(rs.values()) <= 1.0, (name, what, rs)


def _same_bits(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", _ids("B"))
def test_fused_backward_vs_fp64(name):
    c, ins, HW, dev, d = setup(name)
    B, C, Pn = c["B"], c["C"], HW[0] * HW[1]
    form = _forms(d, 1)
    assert form["bwd"] == c["bwd"], form
    for k in ("chunk_rows", "gather_rows"):
        if k in c:
            assert form[k] == c[k], form
    saved = _logprob(d, dev, c, HW)
    g = R.make_grads(c)["g_logprob"]
    cell = form["bwd"] == R.CELL      # (its texel gradients are sums of cell moments)
    ref, mag = R.backward(ins, HW, dict(g_logprob=g), moments=cell)
    got = _bwd(d, dev, c, HW, saved, g_logprob=g.cuda())
    _compare_grads(name, "per-pixel g_logprob", got, ref, mag)
    again = _bwd(d, dev, c, HW, saved, g_logprob=g.cuda())
    assert _same_bits(got, again), "a second run returns other bits"
    # the gradient of the tile sums, non-uniform weights
    sums, tiles = _logprob_sums(d, dev, c, HW)
    gen = torch.Generator().manual_seed(77)
    g_tile = 0.5 + torch.rand(B, tiles, generator=gen)
    ref, mag = R.backward(ins, HW, dict(g_logprob=R.spread_tiles(g_tile, form["ppb"], C, Pn)),
                          moments=cell)
    got = _bwd(d, dev, c, HW, sums, g_tile=g_tile.cuda())
    _compare_grads(name, "per-tile g_tile", got, ref, mag)


@pytest.mark.parametrize("name", _ids("U"))
def test_unfused_backward_vs_fp64(name):
    c, ins, HW, dev, d = setup(name)
    form = _forms(d, 0)
    assert form["bwd"] == c["bwd_unfused"], form
    g = R.make_grads(c)
    first = None
    for what, gs in (("g_tt alone", dict(g_tt=g["g_tt"])), ("g_ml alone", dict(g_ml=g["g_ml"])),
                     ("g_tt and g_ml", dict(g_tt=g["g_tt"], g_ml=g["g_ml"]))):
        ref, mag = R.backward(ins, HW, gs)
        dv = {k: v.cuda() for k, v in gs.items()}
        got = _bwd(d, dev, c, HW, None, **dv)
        _compare_grads(name, "unfused " + what, got, ref, mag)
        first = (got, dv)
    again = _bwd(d, dev, c, HW, None, **first[1])
    assert _same_bits(first[0], again), "a second run returns other bits"


def test_backward_under_template_repeat_is_unsupported():
    from torch_scae_amd import _lib
    c, ins, HW, dev, d = setup("template-repeat-3")
    B, M, C = c["B"], c["M"], c["C"]
    z = lambda *s: torch.zeros(*s, device="cuda")     # noqa: E731
    args = (_p(dev["x"]), _p(z(B, C, *HW)), _p(z(B, 1, *HW)), _p(z(B, C, *HW)), None, None,
            _p(z(B, M, C, *c["ts"])), _p(z(B, M, *c["ts"])), _p(z(B, M, 6)), _p(z(B, M)), None,
            _p(z(B, M + 1, 4)), _st())
    assert _lib.load().scae_render_gmm_bwd_f32(ctypes.byref(d), *args) == _lib.ERR_UNSUPPORTED
    tiles = _lib.load().scae_render_gmm_logprob_tiles(ctypes.byref(d))
    sums_args = args[:3] + (_p(z(B, tiles)),) + args[6:]
    assert _lib.load().scae_render_gmm_sums_bwd_f32(ctypes.byref(d), *sums_args) \
        == _lib.ERR_UNSUPPORTED
