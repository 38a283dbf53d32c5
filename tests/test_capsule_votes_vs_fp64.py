"""K3, the object-capsule votes, entry by entry against the fp64 reference of
tests/votes_ref.py: every output and every gradient within c 2^-24 of its companion magnitude
(c from the fp32 oracle's own distance, tests/test_votes_ref.py), every incoming gradient
alone and all together, at the ABI level with a sentinel tail behind every output buffer.

Both forms: the stand-alone one (csrc/capsule_votes.hip: one wave per capsule, a lane loop
over the votes that takes a second trip at V > 64) and the fused one (``fwd_block`` /
``bwd_block`` of csrc/capsule_votes_dev.h inside the K7b chain launches: 16 capsules per
call, 16-lane and 4-way reductions, scratch in an activation buffer or in the weight tiles,
twice per workgroup at 32 rows) -- the latter in each of the launcher's three forms, which
``scae_mlp_chain_get_form`` names and every fused case asserts.  The fused cases feed the vote
blocks through a one-layer chain with an identity weight, whose output is relu(x) bit for
bit (products with 0 and 1 are exact), and the reference is evaluated on the all_param the
chain itself wrote.

The arg-max is held without a tolerance: ``caps_arg`` is the first index of the maximum of
the kernel's own vote_presence and ``caps_presence`` that entry's bits; it is the fp64
arg-max where the fp64 gap exceeds the bar of two presences, and the lowest tied vote on the
planted ties.

Run with -s: each check prints its worst ratio against the bar."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import votes_ref as R

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
SENT = 7.0
ISENT = -7
PAD = 37
CASES = R.all_cases()
IDS = [R.case_id(c) for c in CASES]
BIAS = ("cpr_static", "bias_cvr", "bias_caps", "bias_vote", "bias_scale")
OUTS = R.FLOAT_OUTS + ("caps_presence", "caps_arg")


def _st():
    return P(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else P(t.data_ptr())


def _padded(*shape, dtype=torch.float32):
    """-> (buffer with PAD sentinel entries behind it, view of the tensor); the tensor itself
    starts out as sentinels, too"""
    n = int(np.prod(shape))
    buf = torch.full((n + PAD,), ISENT if dtype == torch.int32 else SENT, dtype=dtype,
                     device="cuda")
    return buf, buf[:n].view(*shape)


def _tails_untouched(bufs):
    for name, (buf, view) in bufs.items():
        tail = buf[view.numel():]
        assert bool((tail == (ISENT if buf.dtype == torch.int32 else SENT)).all()), name


def _rows(B, O, A, ldp, fill=None):
    """(B, O, ldp) rows behind a sentinel tail, their padding columns [A, ldp) sentinels;
    -> (bufs entry, the (B, O, A) view)"""
    buf, full = _padded(B, O, ldp)
    if fill is not None:
        full[..., :A] = fill
    return (buf, full), full[..., :A]


def _padding_untouched(entry, A, name):
    _tails_untouched({name: entry})
    assert bool((entry[1][..., A:] == SENT).all()), name + ": padding columns"


@functools.lru_cache(maxsize=None)
def case(c):
    ins, meta = R.checked_case(*c)
    dev = {k: v.contiguous().cuda() if torch.is_tensor(v) else v for k, v in ins.items()}
    return ins, meta, R.forward(ins), dev


def _flags(ins):
    return int(ins["similarity"]), int(ins["learn_vote_scale"]), int(ins["allow_deformations"])


def _new_outs(B, O, V, with_caps=True):
    f = dict(vote=_padded(B, O, V, 6), scale=_padded(B, O, V), vote_presence=_padded(B, O, V),
             logit_caps=_padded(B, O, 1), logit_vote=_padded(B, O, V),
             reg_partial=_padded(B, O))
    if with_caps:
        f["caps_presence"] = _padded(B, O)
        f["caps_arg"] = _padded(B, O, dtype=torch.int32)
    return f


# ------------------------------------------------------------------------- stand-alone form
def _fwd(dev, B, O, V, ldp=None, with_caps=True):
    from torch_scae_amd import _lib
    A = 8 * V + 7
    ldp = ldp or A
    rows, _ = _rows(B, O, A, ldp, dev["all_param"])
    f = _new_outs(B, O, V, with_caps)
    _lib.call("scae_capsule_votes_fwd_f32", _p(rows[1]), *[_p(dev[k]) for k in BIAS],
              _p(dev["noise_caps"]), _p(dev["noise_vote"]), float(dev["noise_scale"]),
              *[_p(f[k][1]) if k in f else None for k in OUTS], B, O, V, ldp, *_flags(dev),
              _st())
    torch.cuda.synchronize()
    _tails_untouched(f)
    return {k: v[1] for k, v in f.items()}, rows


def _bwd(dev, rows, grads, caps_arg, B, O, V, ldp=None, gated=True):
    from torch_scae_amd import _lib
    A = 8 * V + 7
    ldp = ldp or A
    ga, gg = _rows(B, O, A, ldp), _rows(B, O, A, ldp)
    gin = _padded(B, O, V, 6)
    g = [None if grads.get(k) is None else grads[k].contiguous().cuda() for k in R.GRAD_NAMES]
    _lib.call("scae_capsule_votes_bwd_f32", _p(rows[1]), *[_p(dev[k]) for k in BIAS],
              _p(dev["noise_caps"]), _p(dev["noise_vote"]), float(dev["noise_scale"]),
              *[_p(t) for t in g], _p(caps_arg), _p(ga[0][1]), _p(gin[1]),
              _p(gg[0][1]) if gated else None, B, O, V, ldp, *_flags(dev), _st())
    torch.cuda.synchronize()
    _padding_untouched(ga[0], A, "gall_param")
    _padding_untouched(gg[0], A, "gall_param_gated")
    _tails_untouched(dict(gcpr_in=gin))
    got = dict(gall_param=ga[1], gcpr_in=gin[1])
    if gated:
        got["gall_param_gated"] = gg[1]
    else:
        assert bool((gg[1] == SENT).all())
    return got


def _check_forward(out, ins, meta, ref, what):
    B, O, V = ref["vote_presence"].shape
    rs = {}
    for k in R.FLOAT_OUTS:
        assert out[k].shape == ref[k].shape, k
        rs[k] = R.ratio(out[k], ref[k], ref["scale_of"][k], R.C_OUT)
    line = f"{what}: |err| / bound " + " ".join(f"{k} {r:.2g}" for k, r in rs.items())
    if "caps_arg" not in out:
        print(line)
    assert max(rs.values()) <= 1.0, (what, rs)
    if not ins["allow_deformations"]:
        assert float(out["reg_partial"].abs().max()) == 0.0
    if not ins["learn_vote_scale"]:
        assert bool((out["scale"] == 1.0).all())
    if "caps_arg" not in out:
        return
    vp, arg = out["vote_presence"].cpu(), out["caps_arg"].cpu().long()
    sure = R.clear(ref)
    print(f"{line}; {int(sure.sum())}/{sure.numel()} clear, "
          f"{int((arg != ref['caps_arg']).sum())} off the fp64 arg-max")
    assert int(arg.min()) >= 0 and int(arg.max()) < V
    assert torch.equal(arg, R._argmax(vp)), what          # the first maximum of its own output
    assert torch.equal(out["caps_presence"].cpu(), vp.gather(-1, arg.unsqueeze(-1)).squeeze(-1))
    assert torch.equal(arg[sure], ref["caps_arg"][sure]), what
    tied = meta["tie"] >= 0
    assert torch.equal(arg[tied], meta["tie"][tied]), what


def _check_backward(got, want, ins, what, acc=None):
    """``acc``: collect the worst ratio per tensor (and which incoming gradient gave it) for
    one line from ``_report``, not a line per call"""
    V = want["gcpr_in"].shape[2]
    rs = {k: R.ratio(g, want[k], want["scale_of"][k], R.C_GRAD) for k, g in got.items()}
    if acc is None:
        print(f"{what}: |err| / bound " + " ".join(f"{k} {r:.2g}" for k, r in rs.items()))
    else:
        for k, r in rs.items():
            if r >= acc.get(k, (-1.0, ""))[0]:
                acc[k] = (r, what.rsplit(" ", 1)[-1])
    assert max(rs.values()) <= 1.0, (what, rs)
    for k in ("gall_param", "gall_param_gated"):
        if k not in got:
            continue
        if not ins["allow_deformations"]:
            assert float(got[k][..., :6 * V].abs().max()) == 0.0, (what, k)
        if not ins["learn_vote_scale"]:
            assert float(got[k][..., 7 * V + 7:].abs().max()) == 0.0, (what, k)


def _report(what, acc):
    print(f"{what}: worst |err| / bound " +
          " ".join(f"{k} {r:.2g} ({name})" for k, (r, name) in acc.items()))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_standalone_forward_vs_fp64(c):
    ins, meta, ref, dev = case(c)
    out, _ = _fwd(dev, *c[1:4])
    _check_forward(out, ins, meta, ref, R.case_id(c))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_standalone_backward_each_incoming_gradient_alone_and_all_together_vs_fp64(c):
    ins, meta, ref, dev = case(c)
    B, O, V = c[1:4]
    out, rows = _fwd(dev, B, O, V)
    arg = out["caps_arg"]
    acc = {}
    for name, gs in R.subsets(R.make_grads(B, O, V)):
        got = _bwd(dev, rows, gs, arg, B, O, V)
        want = R.backward(ins, gs, arg.cpu())
        _check_backward(got, want, ins, f"{R.case_id(c)} incoming {name}", acc)
    _report(R.case_id(c), acc)


@pytest.mark.parametrize("extra", [1, 2, 3, 4])
@pytest.mark.parametrize("c", [("benign", 17, 5, 7, 1, 1, 1, "both"),
                               ("relu", 17, 5, 7, 0, 1, 0, "both"),
                               ("ties", 3, 2, 65, 1, 1, 1, "both")], ids=R.case_id)
def test_standalone_row_stride(c, extra):
    """ld_param = A + 1 .. A + 4: the same bits as with dense rows, and the padding columns
    of both gradient copies keep their sentinels (``_bwd`` asserts it)."""
    ins, meta, ref, dev = case(c)
    B, O, V = c[1:4]
    ldp = 8 * V + 7 + extra
    dense, drows = _fwd(dev, B, O, V)
    out, rows = _fwd(dev, B, O, V, ldp=ldp)
    assert bool((rows[1][..., 8 * V + 7:] == SENT).all())
    for k in OUTS:
        assert torch.equal(out[k], dense[k]), k
    _check_forward(out, ins, meta, ref, f"{R.case_id(c)} ld {ldp}")
    gs = R.make_grads(B, O, V)
    got = _bwd(dev, rows, gs, out["caps_arg"], B, O, V, ldp=ldp)
    gd = _bwd(dev, drows, gs, dense["caps_arg"], B, O, V)
    for k in got:
        assert torch.equal(got[k], gd[k]), k
    _check_backward(got, R.backward(ins, gs, out["caps_arg"].cpu()), ins,
                    f"{R.case_id(c)} ld {ldp} incoming all")


@pytest.mark.parametrize("c", [("benign", 17, 5, 7, 1, 1, 1, "both"),
                               ("relu", 33, 2, 17, 0, 1, 1, "both"),
                               ("benign", 3, 2, 65, 1, 1, 1, "both")], ids=R.case_id)
def test_standalone_nullable_outputs(c):
    """caps_presence / caps_arg both NULL, gall_param_gated NULL: nothing else changes."""
    ins, meta, ref, dev = case(c)
    B, O, V = c[1:4]
    full, rows = _fwd(dev, B, O, V)
    bare, _ = _fwd(dev, B, O, V, with_caps=False)
    assert "caps_arg" not in bare
    for k in R.FLOAT_OUTS:
        assert torch.equal(bare[k], full[k]), k
    _check_forward(bare, ins, meta, ref, f"{R.case_id(c)} no caps_presence")
    # without gcaps_presence the backward needs no caps_arg either
    gs = {k: v for k, v in R.make_grads(B, O, V).items() if k != "gcaps_presence"}
    both = _bwd(dev, rows, gs, None, B, O, V)
    one = _bwd(dev, rows, gs, None, B, O, V, gated=False)
    assert "gall_param_gated" not in one
    for k in one:
        assert torch.equal(one[k], both[k]), k
    _check_backward(one, R.backward(ins, gs), ins, f"{R.case_id(c)} no gated copy")


# -------------------------------------------------------------------------------- fused form
FORMS = {(16, 0, 0): "16a",    # 16 rows, one stride, the vote scratch in an activation buffer
         (16, 1, 1): "16w",    # 16 rows, narrow buffers, the scratch in the weight tiles
         (32, 1, 1): "32"}     # 32 rows (narrow buffers, the scratch in the weight tiles)
SMALL = {0: ("16a", "16a"), 16: ("16a", "16a"), 32: ("32", "32")}
# V = 65 (A = 527, one stride 532): 16 rows of two such buffers and the weight tiles are above
# 80 KiB.  Forward, both buffers hold 527 columns: not narrow, and 32 rows would take 167 KiB.
# Backward, buffer 1 holds nothing: narrow (68.5 KiB), 32 rows 103 KiB.
V65 = {0: ("16a", "16w"), 16: ("16a", "16w"), 32: ("16a", "32")}
# V = 87: 16 * 7 V floats of backward scratch do not fit the weight tiles (8704 floats), so
# neither a narrow form nor 32 rows is taken, whatever row_tile asks for
V87 = {0: ("16a", "16a"), 16: ("16a", "16a"), 32: ("16a", "16a")}
FUSED = [(c, V87 if c[3] == R.V_MAX else V65 if c[3] == 65 else SMALL) for c in (
    [("benign", *s, i % 2, 1, 1, "both") for i, s in enumerate(R.SHAPES)] +
    [("benign", 17, 5, 7, 0, 0, 0, "both"), ("benign", 17, 5, 7, 1, 0, 1, "both"),
     ("benign", 17, 5, 7, 0, 1, 0, "both"), ("benign", 17, 5, 7, 1, 1, 1, "none"),
     ("saturated", 17, 5, 7, 1, 1, 1, "both"), ("saturated", 37, 6, 24, 1, 1, 1, "both"),
     ("relu", 33, 2, 17, 0, 1, 1, "both"), ("wrap", 17, 5, 7, 1, 1, 1, "both"),
     ("wrap", 3, 2, 65, 0, 1, 1, "both")] +
    [("ties", *s, (i + 1) % 2, 1, 1, "both") for i, s in enumerate(R.REGIME_SHAPES["ties"])])]
assert all(c in CASES for c, _ in FUSED)
FUSED_PARAMS = [
    pytest.param(c, tile, forms[tile],
                 id=f"{R.case_id(c)}-tile{tile}-fwd{forms[tile][0]}-bwd{forms[tile][1]}")
    for c, forms in FUSED for tile in (0, 16, 32)]


def _form(d, v, bwd):
    from torch_scae_amd import _lib
    f = _lib.MlpChainForm()
    _lib.call("scae_mlp_chain_get_form", ctypes.byref(d), ctypes.byref(v), int(bwd),
              ctypes.byref(f))
    return FORMS[(f.rows, f.narrow, f.scratch_in_weights)]


def _votes_desc(dev, V, ldp):
    from torch_scae_amd import _lib
    v = _lib.VotesDesc()
    for k in BIAS + ("noise_caps", "noise_vote"):
        setattr(v, k, None if dev[k] is None else dev[k].data_ptr())
    v.noise_scale, v.V, v.ld_param = float(dev["noise_scale"]), V, ldp
    v.similarity, v.learn_vote_scale, v.allow_deformations = _flags(dev)
    return v


def _chain_fwd(x, ws, dev, V, ldp, tile, with_caps=True):
    """the chain relu(W_n .. relu(W_0 x)) with the vote blocks at its end, one launch
    -> (outputs, all_param rows entry, hidden activations, the form taken)"""
    from torch_scae_amd import _lib
    B, G, Kin = x.shape
    A = 8 * V + 7
    d = _lib.MlpChainDesc()
    d.n_layers, d.in_, d.in_gs, d.in_bs, d.in_dim, d.B, d.G, d.row_tile, d.bf16 = \
        len(ws), x.data_ptr(), x.stride(1), x.stride(0), Kin, B, G, tile, 0
    rows, _ = _rows(B, G, A, ldp)
    acts = []
    for l, w in enumerate(ws):
        N, K = w.shape[1:]
        y = d.layer[l]
        y.w, y.w_gs, y.ldw, y.K, y.N, y.relu = w.data_ptr(), N * K, K, K, N, 1
        if l == len(ws) - 1:
            y.out, y.out_gs, y.out_bs = rows[1].data_ptr(), ldp, G * ldp
        else:
            acts.append(torch.empty(G, B, N, device="cuda"))
            y.out, y.out_gs, y.out_bs = acts[-1].data_ptr(), B * N, N
    v = _votes_desc(dev, V, ldp)
    f = _new_outs(B, G, V, with_caps)
    for k, (_, t) in f.items():
        setattr(v, k, t.data_ptr())
    form = _form(d, v, False)
    _lib.call("scae_mlp_chain_votes_fwd_f32", ctypes.byref(d), ctypes.byref(v), _st())
    torch.cuda.synchronize()
    _tails_untouched(f)
    _padding_untouched(rows, A, "all_param")
    return {k: t[1] for k, t in f.items()}, rows, acts, form


def _chain_bwd(x, ws, acts, rows, dev, grads, caps_arg, V, ldp, tile, gated=True):
    """the vote blocks' backward at the head of the data-gradient chain, one launch
    -> (gradients with gx, the form taken)"""
    from torch_scae_amd import _lib
    B, G, Kin = x.shape
    A = 8 * V + 7
    d = _lib.MlpChainDesc()
    d.n_layers, d.in_dim, d.B, d.G, d.row_tile, d.bf16 = len(ws), A, B, G, tile, 0
    gx = _padded(B, G, Kin)
    hidden = []
    for i, l in enumerate(range(len(ws) - 1, -1, -1)):
        N, K = ws[l].shape[1:]
        y = d.layer[i]
        y.w, y.w_gs, y.ldw, y.K, y.N = ws[l].data_ptr(), N * K, K, N, K
        if l > 0:
            hidden.append(torch.empty(G, B, K, device="cuda"))
            y.gate, y.gate_gs, y.gate_bs = acts[l - 1].data_ptr(), B * K, K
            y.out, y.out_gs, y.out_bs = hidden[-1].data_ptr(), B * K, K
        else:
            y.out, y.out_gs, y.out_bs = gx[1].data_ptr(), Kin, G * Kin
    v = _votes_desc(dev, V, ldp)
    v.all_param = rows[1].data_ptr()
    g = {k: None if grads.get(k) is None else grads[k].contiguous().cuda()
         for k in R.GRAD_NAMES}
    for k, t in g.items():
        setattr(v, k, None if t is None else t.data_ptr())
    v.caps_arg = None if caps_arg is None else caps_arg.data_ptr()
    ga, gg = _rows(B, G, A, ldp), _rows(B, G, A, ldp)
    gin = _padded(B, G, V, 6)
    v.gall_param, v.gcpr_in = ga[0][1].data_ptr(), gin[1].data_ptr()
    v.gall_param_gated = gg[0][1].data_ptr() if gated else None
    form = _form(d, v, True)
    _lib.call("scae_mlp_chain_votes_bwd_f32", ctypes.byref(d), ctypes.byref(v), _st())
    torch.cuda.synchronize()
    _padding_untouched(ga[0], A, "gall_param")
    _padding_untouched(gg[0], A, "gall_param_gated")
    _tails_untouched(dict(gcpr_in=gin, gx=gx))
    got = dict(gall_param=ga[1], gcpr_in=gin[1])
    if gated:
        got["gall_param_gated"] = gg[1]
    else:
        assert bool((gg[1] == SENT).all())
    return got, gx[1], form


@functools.lru_cache(maxsize=None)
def relu_case(c):
    """the case behind a one-layer identity chain: all_param = relu(x)"""
    ins, meta, _, dev = case(c)
    rins = R.relu_case(ins)
    A = ins["all_param"].shape[2]
    eye = torch.eye(A).expand(c[2], A, A).contiguous().cuda()
    return rins, meta, R.forward(rins), dev, eye


@functools.lru_cache(maxsize=None)
def _relu_backward(c, name, arg_bytes):
    rins = relu_case(c)[0]
    B, O, V = c[1:4]
    arg = torch.frombuffer(bytearray(arg_bytes), dtype=torch.int32).view(B, O)
    gs = dict(R.subsets(R.make_grads(B, O, V)))[name]
    return R.backward(rins, gs, arg)


def _ld(V, tile):
    """rows padded to a multiple of 4 floats, as ops.chain_votes hands them over; dense (odd,
    unaligned) rows at row_tile 16"""
    A = 8 * V + 7
    return A if tile == 16 else (A + 3) // 4 * 4


@pytest.mark.parametrize("c,tile,forms", FUSED_PARAMS)
def test_fused_forward_vs_fp64(c, tile, forms):
    rins, meta, ref, dev, eye = relu_case(c)
    B, O, V = c[1:4]
    out, rows, _, form = _chain_fwd(dev["all_param"], [eye], dev, V, _ld(V, tile), tile)
    assert form == forms[0]
    # the chain wrote relu(x), bit for bit: the reference is evaluated on just that
    assert torch.equal(rows[1][..., :8 * V + 7].cpu(), rins["all_param"])
    _check_forward(out, rins, meta, ref, f"{R.case_id(c)} tile {tile} ({form})")
    # caps_presence / caps_arg both NULL: nothing else changes
    bare = _chain_fwd(dev["all_param"], [eye], dev, V, _ld(V, tile), tile, with_caps=False)[0]
    assert "caps_arg" not in bare
    for k in R.FLOAT_OUTS:
        assert torch.equal(bare[k], out[k]), k


@pytest.mark.parametrize("c,tile,forms", FUSED_PARAMS)
def test_fused_backward_each_incoming_gradient_alone_and_all_together_vs_fp64(c, tile, forms):
    rins, meta, ref, dev, eye = relu_case(c)
    B, O, V = c[1:4]
    x, ldp = dev["all_param"], _ld(V, tile)
    out, rows, acts, _ = _chain_fwd(x, [eye], dev, V, ldp, tile)
    arg = out["caps_arg"]
    key = arg.cpu().numpy().tobytes()
    acc = {}
    for name, gs in R.subsets(R.make_grads(B, O, V)):
        got, gx, form = _chain_bwd(x, [eye], acts, rows, dev, gs, arg, V, ldp, tile)
        assert form == forms[1]
        _check_backward(got, _relu_backward(c, name, key), rins,
                        f"{R.case_id(c)} tile {tile} ({form}) incoming {name}", acc)
        # the LDS rows the data-gradient chain consumed are the global gated copy
        assert torch.equal(gx, got["gall_param_gated"]), name
    _report(f"{R.case_id(c)} tile {tile} ({form})", acc)
    # without the gated copy the chain consumes the ungated rows
    gs = R.make_grads(B, O, V)
    one, gx, _ = _chain_bwd(x, [eye], acts, rows, dev, gs, arg, V, ldp, tile, gated=False)
    assert torch.equal(one["gall_param"], got["gall_param"])
    assert torch.equal(one["gcpr_in"], got["gcpr_in"])
    assert torch.equal(gx, one["gall_param"])


# a two-layer chain whose one-stride LDS at 16 rows, 16 (2 * 388) + 8704 floats = 82.5 KiB, is
# above 80 KiB and whose narrow LDS, 16 (388 + 20) + 8704 floats = 59.5 KiB, is not: 16 -> 16
# -> 375 (V = 46; the backward chain 375 -> 16 -> 16 has the same two widths); and a small one
RANDOM_CHAINS = [
    pytest.param((19, 2, 46, 16, 16), tile, form, id=f"narrow-19x2x46-tile{tile}-{form}")
    for tile, form in ((0, "16w"), (16, "16w"), (32, "32"))] + [
    pytest.param((19, 3, 7, 20, 24), tile, form, id=f"small-19x3x7-tile{tile}-{form}")
    for tile, form in ((0, "16a"), (16, "16a"), (32, "32"))]


@functools.lru_cache(maxsize=None)
def _random_chain(shape):
    B, O, V, Kin, H = shape
    ins, meta = R.checked_case("benign", B, O, V, 0, 1, 1, "both")
    g = torch.Generator().manual_seed(B * O * V + Kin)
    x = torch.randn(B, O, Kin, generator=g)
    ws = [torch.randn(O, H, Kin, generator=g) / Kin ** 0.5,
          torch.randn(O, 8 * V + 7, H, generator=g) / H ** 0.5 * 2]
    dev = {k: v.contiguous().cuda() if torch.is_tensor(v) else v for k, v in ins.items()}
    return ins, x.cuda(), [w.cuda() for w in ws], dev


@pytest.mark.parametrize("shape,tile,form", RANDOM_CHAINS)
def test_fused_behind_a_random_two_layer_chain_vs_fp64(shape, tile, form):
    """Nothing rests on the identity: the reference on the all_param a random chain wrote."""
    B, O, V, Kin, H = shape
    ins, x, ws, dev = _random_chain(shape)
    A, ldp = 8 * V + 7, _ld(V, tile)
    out, rows, acts, f = _chain_fwd(x, ws, dev, V, ldp, tile)
    assert f == form
    ap = rows[1][..., :A].cpu()
    assert float((ap > 0).float().mean()) > 0.3 and float((ap == 0).float().mean()) > 0.3
    rins = dict(ins, all_param=ap)
    ref = R.forward(rins)
    meta = dict(tie=torch.full((B, O), -1, dtype=torch.int64))
    _check_forward(out, rins, meta, ref, f"random chain {shape} tile {tile} ({f})")
    gs = R.make_grads(B, O, V)
    got, gx, f = _chain_bwd(x, ws, acts, rows, dev, gs, out["caps_arg"], V, ldp, tile)
    assert f == form
    want = R.backward(rins, gs, out["caps_arg"].cpu())
    _check_backward(got, want, rins, f"random chain {shape} tile {tile} ({f}) incoming all")
    # the data-gradient chain behind it, from the kernel's own gated rows (K7b's products
    # have their own module, test_mlp_chain_vs_fp64, and its bar: 1e-4 of the largest entry)
    gg = got["gall_param_gated"].double().cpu()
    gh = torch.einsum("bga,gah->bgh", gg, ws[1].double().cpu()) * \
        (acts[0].transpose(0, 1).cpu() > 0)
    gx_ref = torch.einsum("bgh,ghk->bgk", gh, ws[0].double().cpu())
    assert float((gx.cpu() - gx_ref).abs().max()) <= 1e-4 * float(gx_ref.abs().max())


# ------------------------------------------------------------ op level, parameter gradients
def _op_param_grads(which, B, O, V):
    """ops.capsule_votes on contiguous all_param (ldp = A: odd, unaligned rows) /
    ops.chain_votes behind the identity chain (rows padded to a multiple of 4): the gradients
    of cpr_static and the four biases -- batch sums of gcpr_in and of column blocks of
    gall_param, made by ``_sum_rows_multi`` with period ldp -- against the fp64 sums."""
    from torch_scae_amd import ops
    c = ("benign", B, O, V, 1, 1, 1, "both")
    ins, meta = R.checked_case(*c)
    A = 8 * V + 7
    if which == "chain":
        ins = R.relu_case(ins)
    ref = R.forward(ins)
    lv = {k: ins[k].clone().cuda().requires_grad_() for k in ("all_param",) + BIAS}
    kw = dict(noise_caps=ins["noise_caps"].cuda(), noise_vote=ins["noise_vote"].cuda(),
              noise_scale=ins["noise_scale"], similarity=True, learn_vote_scale=True,
              allow_deformations=True)
    if which == "chain":
        eye = torch.eye(A).expand(O, A, A).contiguous().cuda().requires_grad_()
        outs = ops.chain_votes(lv["all_param"], [(eye, None, False)],
                               *[lv[k] for k in BIAS], **kw)
    else:
        outs = ops.capsule_votes(lv["all_param"], *[lv[k] for k in BIAS], **kw)
    names = ("vote", "scale", "vote_presence", "logit_caps", "logit_vote")
    for k, t in zip(names, outs):
        r = R.ratio(t, ref[k], ref["scale_of"][k], R.C_OUT)
        assert r <= 1.0, (which, k, r)
    vp, cp = outs[2].detach().cpu(), outs[6].detach().cpu()
    assert torch.equal(cp, vp.max(-1)[0])
    arg = R._argmax(vp)                      # where the kernel routes caps_presence's gradient
    gs = R.make_grads(B, O, V, seed=3)
    torch.autograd.backward(list(outs[:7]), [gs[k].cuda() for k in R.GRAD_NAMES])
    torch.cuda.synchronize()
    want = R.backward(ins, gs, arg)
    parts = dict(cpr_static=want["gcpr_in"].abs().sum(0, keepdim=True))
    for k, (lo, hi) in dict(bias_cvr=(6 * V, 6 * V + 6), bias_caps=(6 * V + 6, 6 * V + 7),
                            bias_vote=(6 * V + 7, 7 * V + 7), bias_scale=(7 * V + 7, A)).items():
        parts[k] = want["gall_param"][..., lo:hi].abs().sum(0).reshape(ins[k].shape)
    rs = {}
    for k in BIAS:
        assert lv[k].grad.shape == ins[k].shape
        # C_GRAD 2^-24 of the summed companions, and gamma(B) of the summed |terms|
        bound = R.C_GRAD * R.U * want["scale_of"][k] + R.gamma(B) * parts[k]
        r = R.ratio(lv[k].grad, want[k], bound, 1.0 / R.U)
        rs[k] = r
    print(f"ops.{which} {B}x{O}x{V}: |err| / bound " +
          " ".join(f"{k} {r:.2g}" for k, r in rs.items()))
    assert max(rs.values()) <= 1.0, (which, rs)
    r = R.ratio(lv["all_param"].grad, want["gall_param_gated" if which == "chain"
                                           else "gall_param"],
                want["scale_of"]["gall_param"], R.C_GRAD)
    assert r <= 1.0, (which, "all_param", r)


@pytest.mark.parametrize("B,O,V", [(37, 5, 7), (19, 3, 65)])
@pytest.mark.parametrize("which", ["votes", "chain"])
def test_op_parameter_gradients_vs_fp64(which, B, O, V):
    _op_param_grads(which, B, O, V)
