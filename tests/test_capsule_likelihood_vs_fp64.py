"""K4, the capsule likelihood (csrc/capsule_likelihood_dev.h), entry by entry against the fp64
reference of tests/lk_ref.py: every output and every gradient within c 2^-24 of its companion
magnitude (c from the fp32 oracle's own distance, tests/test_lk_ref.py), every incoming
gradient alone and all together, in the register form (O <= 64), the LDS two-pass form
(O > 64) and with the grid's stride loop (B > 1024), on benign, dominant, near-dummy, floored
and tied inputs.  The winner is held by a rule that is valid in every regime: its fp64
posterior logit is within G of the maximum (lk_ref.winner_gap), it IS the fp64 arg-max where
the fp64 gap exceeds 2 G, the lower index on planted ties, and the gathered outputs are the
bits of the vote it names.

The 256-thread form (the backward riding in the part decoder's likelihood backward,
csrc/render_bwd_likelihood.hip): its group sums are 16- and 4-lane whatever the block size,
so it must equal the 1024-thread launch bit for bit.  test_timed_path.py
``test_likelihood_riding_in_the_trunk_launch_changes_nothing`` pins that at cfg-2 (O = M = 24:
M * 16 = 384, no multiple of 256); here the shape where it is one (M = 16), with the ride
switched off by scae_likelihood_bwd_desc.separate as the only difference, and the launch count to show
that the ride was taken.

Run with -s: each check prints its worst ratio against the bar."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import lk_ref as R

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
SENT = 7.0
PAD = 37
CASES = R.all_cases()
IDS = [R.case_id(c) for c in CASES]


def _st():
    return P(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else P(t.data_ptr())


def _padded(*shape, dtype=torch.float32):
    """-> (buffer with PAD sentinel entries behind it, view of the tensor)"""
    n = int(np.prod(shape))
    buf = torch.full((n + PAD,), -7 if dtype == torch.int64 else SENT, dtype=dtype,
                     device="cuda")
    return buf, buf[:n].view(*shape)


def _tails_untouched(bufs):
    for name, (buf, view) in bufs.items():
        tail = buf[view.numel():]
        assert bool((tail == (-7 if buf.dtype == torch.int64 else SENT)).all()), name


@functools.lru_cache(maxsize=None)
def case(c):
    ins, meta = R.checked_case(*c)
    dev = {k: None if v is None else v.contiguous().cuda() for k, v in ins.items()}
    return ins, meta, R.forward(ins), R.winner_gap(ins), dev


def _fwd(dev, B, O, M):
    from torch_scae_amd import _lib
    f = dict(log_prob_per_point=_padded(B, M), vote_presence_binary=_padded(B, O, M),
             winner=_padded(B, M, 6), winner_presence=_padded(B, M),
             winner_idx=_padded(B, M, dtype=torch.int64),
             is_from_capsule=_padded(B, M, dtype=torch.int64), soft_winner=_padded(B, M, 6),
             soft_winner_presence=_padded(B, M), posterior=_padded(B, O + 1, M),
             mixing_log_prob=_padded(B, O + 1, M), mixing_logit=_padded(B, O + 1, M))
    _lib.call("scae_capsule_likelihood_fwd_f32", _p(dev["vote"]), _p(dev["scale"]),
              _p(dev["vote_presence"]), _p(dev["dummy_vote"]), _p(dev["x"]),
              _p(dev["presence"]), *[_p(f[k][1]) for k in f], B, O, M, _st())
    torch.cuda.synchronize()
    _tails_untouched(f)
    return {k: v[1] for k, v in f.items()}


@functools.lru_cache(maxsize=None)
def fwd_of(c):
    return _fwd(case(c)[4], *c[1:4])


def _bwd(dev, out, grads, B, O, M):
    from torch_scae_amd import _lib
    f = dict(vote=_padded(B, O, M, 6), scale=_padded(B, O, M), vote_presence=_padded(B, O, M),
             x=_padded(B, M, 6))
    if dev["presence"] is not None:
        f["presence"] = _padded(B, M)
    f["dummy_partial"] = _padded(B, M, 6)
    gin = [None if grads.get(k) is None else grads[k].contiguous().cuda() for k in R.GRAD_NAMES]
    _lib.call("scae_capsule_likelihood_bwd_f32", _p(dev["vote"]), _p(dev["scale"]),
              _p(dev["vote_presence"]), _p(dev["dummy_vote"]), _p(dev["x"]),
              _p(dev["presence"]), _p(out["posterior"]), _p(out["winner_idx"]),
              *[_p(g) for g in gin], _p(f["vote"][1]), _p(f["scale"][1]),
              _p(f["vote_presence"][1]), _p(f["x"][1]),
              _p(f["presence"][1]) if "presence" in f else None, _p(f["dummy_partial"][1]),
              B, O, M, _st())
    torch.cuda.synchronize()
    _tails_untouched(f)
    return {k: v[1] for k, v in f.items()}


def _winner_for_reference(c, out):
    """the fp64 reference scatters the winner gradients at its own arg-max; in the floored
    parts, where fp32 decides the arg-max by rounding, at the kernel's"""
    ins, meta, ref, G, dev = case(c)
    return torch.where(meta["floored"], out["winner_idx"].cpu(), ref["winner_idx"])


# ------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_forward_outputs_vs_fp64(c):
    ins, meta, ref, G, dev = case(c)
    B, O, M = c[1:4]
    out = fwd_of(c)
    for k in R.FLOAT_OUTS:
        r = R.ratio(out[k], ref[k], ref["scale"][k], R.C_OUT)
        print(f"{R.case_id(c)} {k}: worst |err| / bound {r:.3g}")
        assert r <= 1.0, (k, r)
    assert torch.equal(out["vote_presence_binary"].cpu().double(), ref["vote_presence_binary"])
    row = out["mixing_logit"][:, O].cpu()
    assert torch.equal(row, torch.full((B, M), R.LOG001, dtype=torch.float32))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_winner_in_every_regime(c):
    ins, meta, ref, G, dev = case(c)
    B, O, M = c[1:4]
    out = fwd_of(c)
    win = out["winner_idx"].cpu()
    assert int(win.min()) >= 0 and int(win.max()) < O
    post = ref["post"]
    short = post.max(1)[0] - R._gather(post, win)          # how far below the fp64 maximum
    print(f"{R.case_id(c)}: worst (max - post[winner]) / G {float((short / G).max()):.3g}; "
          f"{int((win != ref['winner_idx']).sum())} of {win.numel()} differ from the fp64 arg-max")
    assert bool((short <= G).all())
    assert torch.equal(out["winner"].cpu(), R._gather(ins["vote"], win))
    assert torch.equal(out["winner_presence"].cpu(), R._gather(ins["vote_presence"], win))
    assert torch.equal(out["is_from_capsule"].cpu(), win // M)
    clear = R.gap(post) > 2 * G
    assert torch.equal(win[clear], ref["winner_idx"][clear])
    assert bool((clear | meta["floored"] | (meta["tie"] >= 0)).all())
    tied = meta["tie"] >= 0
    assert torch.equal(win[tied], meta["tie"][tied])


# ----------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_backward_each_incoming_gradient_alone_and_all_together_vs_fp64(c):
    ins, meta, ref, G, dev = case(c)
    B, O, M = c[1:4]
    out = fwd_of(c)
    win = _winner_for_reference(c, out)
    grads = R.make_grads(B, O, M)
    subsets = [(k, {k: grads[k]}) for k in R.GRAD_NAMES] + [("all", grads)]
    for name, gs in subsets:
        got = _bwd(dev, out, gs, B, O, M)
        want = R.backward(ins, gs, winner_idx=win)
        rs = {k: R.ratio(g, want[k], want["scale_of"][k], R.C_GRAD) for k, g in got.items()}
        worst = max(rs.values())
        print(f"{R.case_id(c)} incoming {name}: worst |err| / bound {worst:.3g}")
        assert worst <= 1.0, (name, rs)
        if c[4]:
            assert "presence" in got
        else:
            assert "presence" not in got and want["presence"] is None


# ------------------------------------------------------------- through the op and autograd
OUT_ORDER = ("log_prob_per_point", "vote_presence_binary", "winner", "winner_presence",
             "winner_idx", "is_from_capsule", "soft_winner", "soft_winner_presence",
             "posterior", "mixing_log_prob", "mixing_logit", "log_prob")


def _op(c, weights):
    """ops.capsule_likelihood on leaves, backward of the weighted sum -> (outputs, leaves)"""
    from torch_scae_amd import ops
    ins = case(c)[0]
    lv = {k: None if v is None else v.detach().clone().cuda().requires_grad_(True)
          for k, v in ins.items()}
    res = dict(zip(OUT_ORDER, ops.capsule_likelihood(
        lv["vote"], lv["scale"], lv["vote_presence"], lv["dummy_vote"], lv["x"],
        lv["presence"])))
    tot = sum((res[k] * w.cuda()).sum() for k, w in weights.items())
    tot.backward()
    torch.cuda.synchronize()
    return res, lv


def _check_op_grads(c, res, lv, weights, what):
    ins, meta, ref, G, dev = case(c)
    B = c[1]
    gs = {k: w for k, w in weights.items() if k != "log_prob"}
    extra = None
    if "log_prob" in weights:
        # log_prob = sum(log_prob_per_point) / B: the op forms g_log_prob / B and adds it to
        # the per-point gradient in fp32 -- two roundings of the incoming gradient itself,
        # each 2^-24 of |g_log_prob / B| + |g_per_point| (which may cancel in the sum).  They
        # reach every output like a per-point gradient of that size: 2 units of its companion
        # on top of the bar
        spread = (weights["log_prob"].double() / B).expand(B, c[3])
        own = gs["log_prob_per_point"].double() if "log_prob_per_point" in gs else 0.0 * spread
        gs["log_prob_per_point"] = spread + own
        extra = R.backward(ins, {"log_prob_per_point": spread.abs() + own.abs()})["scale_of"]
    win = torch.where(meta["floored"], res["winner_idx"].cpu(), ref["winner_idx"])
    want = R.backward(ins, gs, winner_idx=win)
    for k in R.IN_NAMES:
        if lv[k] is None or want[k] is None:
            continue
        scale = want["scale_of"][k]
        if extra is not None and extra[k] is not None:
            scale = scale + (2.0 / R.C_GRAD) * extra[k]
        r = R.ratio(lv[k].grad, want[k], scale, R.C_GRAD)
        print(f"{R.case_id(c)} {what} grad {k}: worst |err| / bound {r:.3g}")
        assert r <= 1.0, (what, k, r)


@pytest.mark.parametrize("c", [("benign", 3, 17, 37, True), ("benign", 2, 65, 65, True)],
                         ids=R.case_id)
def test_op_and_autograd_vs_fp64(c):
    ins, meta, ref, G, dev = case(c)
    B, O, M = c[1:4]
    w = dict(R.make_grads(B, O, M, seed=1), log_prob=torch.tensor(1.7))
    res, lv = _op(c, w)
    for k in R.FLOAT_OUTS + ("log_prob",):
        r = R.ratio(res[k], ref[k], ref["scale"][k], R.C_OUT)
        print(f"{R.case_id(c)} op {k}: worst |err| / bound {r:.3g}")
        assert r <= 1.0, (k, r)
    assert torch.equal(res["winner_idx"].cpu(), ref["winner_idx"])
    _check_op_grads(c, res, lv, w, "all nine")
    assert lv["dummy_vote"].grad is not None
    # log_prob alone: the dummy vote is not reached at all, as in the reference
    w = dict(log_prob=torch.tensor(-0.6))
    res, lv = _op(c, w)
    assert lv["dummy_vote"].grad is None
    _check_op_grads(c, res, lv, w, "log_prob alone")
    # winner alone: the dummy vote's partials are zeros, and so is their sum (_sum_rows)
    w = dict(winner=R.make_grads(B, O, M, seed=2)["winner"])
    res, lv = _op(c, w)
    g = lv["dummy_vote"].grad
    assert g is not None and g.shape == ins["dummy_vote"].shape and float(g.abs().max()) == 0.0
    _check_op_grads(c, res, lv, w, "winner alone")


def test_beyond_the_lds_limit_is_an_error_and_nothing_is_launched():
    """(3 O + 14) M floats of LDS in the backward: (2, 200, 67) is 41 138 > 40 960."""
    from torch_scae_amd import _lib, ops
    from torch_scae_amd.ops import ScaeHipError
    B, O, M = 2, 200, 67
    assert (3 * O + 14) * M > 40960 >= (3 * 200 + 14) * 60
    g = torch.Generator().manual_seed(5)
    vote = torch.randn(B, O, M, 6, generator=g).cuda()
    args = (vote, torch.ones(B, O, M, device="cuda"),
            torch.rand(B, O, M, generator=g).cuda(), torch.zeros(1, 1, M, 6, device="cuda"),
            torch.randn(B, M, 6, generator=g).cuda(), None)
    lib = _lib.load()
    torch.cuda.synchronize()
    lst = lib.scae_launch_list_begin(_st())
    assert lst
    try:
        with pytest.raises(ScaeHipError):
            ops.capsule_likelihood(*args)
        assert lib.scae_launch_list_end(P(lst)) == 0
        assert lib.scae_launch_list_size(P(lst)) == 0
    finally:
        lib.scae_launch_list_free(P(lst))


# ------------------------------------------------------------------- the 256-thread riding form
def test_backward_riding_in_the_decoder_launch_equals_its_own_launch_bitwise(monkeypatch):
    """A medium-config TrainStep with an encoder-fed decoder and 16 part capsules
    (M * 16 = 256: every pass of the 256-thread loops is full; O = 6): K4's backward as the
    first block range of scae_render_gmm_sums_bwd_likelihood_f32's launch (256 threads)
    against the same entry point splitting into its two launches (ops._K1_K4_SEPARATE, the
    descriptor's ``separate``: K4 on 1024 threads) and against fuse_kernels off -- the likelihood's four incoming
    gradients (log_prob_per_point, posterior, mixing_log_prob, mixing_logit) and all that
    follows from them, bit for bit in every parameter gradient."""
    from tests.test_step_plan import _eager_step, _filled_state, _flat_grads, _medium_cfg
    from torch_scae_amd import _lib, ops
    cfg = dict(_medium_cfg(vote_type="enc", presence_type="enc"), n_part_caps=16)
    sd, g = _filled_state(cfg)
    B = 8
    image = torch.rand(B, *cfg["image_shape"], generator=g).cuda()
    label = torch.randint(0, cfg["n_classes"], (B,), generator=g).cuda()
    lib = _lib.load()
    runs = {}
    for mode in ("ride", "split", "unfused"):
        monkeypatch.setattr(ops, "_K1_K4_SEPARATE", mode == "split")
        torch.manual_seed(99)       # (the noise streams: the same draws in every run)
        ops.reset_noise()
        model, step = _eager_step(cfg, sd, B, fuse_kernels=mode != "unfused")
        calls, real = [], ops._lib.call

        def spy(name, *a):
            calls.append(name)
            return real(name, *a)
        torch.cuda.synchronize()
        lst = lib.scae_launch_list_begin(_st())
        assert lst
        ops._lib.call = spy
        try:
            loss = step(image, label)
            torch.cuda.synchronize()
        finally:
            ops._lib.call = real
            lib.scae_launch_list_end(P(lst))
        n = lib.scae_launch_list_size(P(lst))
        lib.scae_launch_list_free(P(lst))
        runs[mode] = (float(loss), {k: v.detach().clone() for k, v in _flat_grads(step).items()},
                      calls, n)
    monkeypatch.setattr(ops, "_K1_K4_SEPARATE", False)
    assert "scae_render_gmm_sums_bwd_likelihood_f32" in runs["ride"][2]
    assert "scae_render_gmm_sums_bwd_likelihood_f32" in runs["split"][2]
    assert "scae_capsule_likelihood_bwd_f32" in runs["unfused"][2]
    # the same calls, one kernel launch fewer: the ride was taken
    assert runs["ride"][2] == runs["split"][2] and runs["ride"][3] + 1 == runs["split"][3]
    l0, g0 = runs["ride"][:2]
    assert len(g0) > 50 and any(float(v.abs().max()) > 0 for v in g0.values())
    for mode in ("split", "unfused"):
        l1, g1 = runs[mode][:2]
        assert l1 == l0, (mode, l0, l1)
        for k in g0:
            assert torch.equal(g0[k], g1[k]), (mode, k)
    print(f"ride {runs['ride'][3]} launches, split {runs['split'][3]}, "
          f"unfused {runs['unfused'][3]}; loss {l0:.6f}; {len(g0)} gradients bit-equal")
