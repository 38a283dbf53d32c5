"""The exact-split fp32 kernels (csrc/bf16x6.h: six bf16 partial products per fp32 product)
entry by entry against fp64 that sums the same six kinds, within the bound derived in
tests/x6_emulate.py.  A dropped kind, a lost ``mid`` or ``lo`` plane, or a kind read from the
wrong plane moves an entry by about 2^-16 of its size -- far outside that bound on the sparse-K
operand families used here (tests/test_x6_emulate.py: >= 4x on the worst entry, measured
19x .. 10^6x), where the 1e-4 and 2e-6-of-max bars of test_hip_ops.py cannot see it.

Operand families: every value a full 24-bit mantissa (all three planes nonzero; one draw with
some ``mid`` / ``lo`` planes exactly zero), magnitudes 2^[-8, 8), random signs; one operand
dense, the other sparse along K -- each output entry has a few nonzero products, each in a
different 32-deep K chunk (asserted per case by ``x6_emulate.chunk_counts_ok``), so that no
MFMA adds two of them.  Both sides are made sparse in turn: the filter (K8r's is pre-split in
``wp``, the tiles split it in registers) and the activations / pre-activation gradient.

Forms and how each is reached (conv_mfma.hip ``plan_dgrad`` / ``conv_bwd_pair_impl``,
restated by ``x6_emulate.dgrad_mode`` and asserted there):
  * forward: conv_fwd_pipe_kernel<PipeC2> is the only fp32 form of scae_conv3x3_fwd_f32;
  * data gradient: DMODE 4 where (Cin/128) x 64-pixel tiles >= 500 (forced by SCAE_DGRAD_TILE
    in scae_conv3x3_bwd_pair_forms_f32's dgrad_forms, barred by SCAE_DGRAD_NO_TILE), else
    DMODE 5 (barred by SCAE_DGRAD_NO_KSPLIT), else the first-generation
    tiles on fp32 MFMAs (v_mfma_f32_16x16x4_f32, mfma_tile.h): DMODE 0 when (Cin/64) x
    64-pixel tiles >= 1024, DMODE 2 when (Cin/64) x 32-pixel tiles >= 600, else DMODE 1;
  * weight gradient: scae_conv3x3_wgrad_f32 always takes PipeW (32-pixel ring); inside the
    pair launch PipeW16 (16-pixel ring) when the data gradient is not DMODE 5 and
    B*OH*OW < SCAE_WGRAD_SHORT_CHUNK_PIXELS (8192), else PipeW;
  * gemm_ksplit.hip (x6k) by shape (scae_gemm_desc.form = 0), gemm_mfma.hip's fp32 tiles
    with form = SCAE_GEMM_TILES.
Where a selector switches the form, the two runs must differ in their bits.
fwd_fold, bwd_pair_reduce and bwd_pair_fold equal separate launches bit for bit
(test_hip_ops.py), so the rows here cover them.
"""
import ctypes

import pytest
import torch

from tests import x6_emulate as E

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
SENT = 7.0


def _st():
    return P(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else P(t.data_ptr())


def _check(got, ref, bound, what):
    """every entry within its bound (entries with bound 0 -- no product -- exactly)."""
    d = (got.double().cpu() - ref).abs()
    ratio = torch.where(bound > 0, d / bound.clamp_min(1e-300),
                        torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    worst = float(ratio.max())
    print(f"{what}: worst |err| / bound {worst:.3g}  ({int((bound > 0).sum())} entries)")
    assert worst <= 1.0, what
    return worst


def _call(name, *args):
    from torch_scae_amd import _lib
    _lib.call(name, *args)


def _dev(t):
    return t.contiguous().cuda()


# --------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("B,IH,IW,Ci,Co,s,post", [
    (3, 9, 9, 128, 64, 1, True),      # one ragged tile (147 rows), the embedding bias output
    (2, 21, 19, 64, 128, 2, False),   # stride 2, two channel tiles, two chunks per tap
    (5, 6, 7, 64, 64, 2, True),       # stride 2, one ragged 32-row tile
])
@pytest.mark.parametrize("side", ["filter", "input", "filter-zero-planes"])
def test_conv_forward_pipe_vs_fp64(B, IH, IW, Ci, Co, s, post, side):
    """scae_conv3x3_fwd_f32 (PipeC2: 32 x 64 tiles, the 2 k-halves meet in LDS: x = 1), with
    the filter and its negation: every entry is checked unclipped by the ReLU in one run."""
    g = torch.Generator().manual_seed(B * 1000 + IH * 10 + Ci)
    OH, OW = (IH - 3) // s + 1, (IW - 3) // s + 1
    lz = 0.5 if side.endswith("zero-planes") else 0.0
    if side.startswith("filter"):
        x, w = E.full_mantissa(g, (B, IH, IW, Ci)), E.sparse_filter(g, Co, Ci, "fwd", lo_zero=lz)
    else:
        x, w = E.sparse_pixels(g, B, IH, IW, Ci), E.full_mantissa(g, (Co, Ci, 3, 3))
    assert "fwd" in E.chunk_counts_ok(x, w, None, s)
    bias, pb = E.full_mantissa(g, (Co,), 4), E.full_mantissa(g, (Co, OH, OW), 4)
    t = E.kind_terms(E.op_fwd(s), x, w)
    M = B * OH * OW
    xd, bd, pbd = _dev(x), _dev(bias), _dev(pb)             # (alive across the launches)
    for sign in (1.0, -1.0):
        wf = _dev((sign * w).permute(0, 2, 3, 1))             # (co, tap, ci)
        out = torch.full((M + 5, Co), SENT, device="cuda")
        outp = torch.full((M + 5, Co), SENT, device="cuda") if post else None
        _call("scae_conv3x3_fwd_f32", _p(xd), _p(wf), _p(bd), _p(out), _p(pbd) if post else None,
              _p(outp), B, IH, IW, Ci, Co, s, _st())
        torch.cuda.synchronize()
        assert bool((out[M:] == SENT).all()) and (outp is None or bool((outp[M:] == SENT).all()))
        ts = dict(t, P=sign * t["P"])
        ref, bound = E.x6_ref(ts, x=1, extra=1, bias=bias.double())
        ref = ref.relu()
        _check(out[:M].view(B, OH, OW, Co), ref, bound, f"fwd {side} sign {sign:+.0f}")
        if post:
            refp = ref + pb.double().permute(1, 2, 0)
            boundp = bound + E.gamma(1) * (ref.abs() + bound + pb.double().abs().permute(1, 2, 0))
            _check(outp[:M].view(B, OH, OW, Co), refp, boundp, f"fwd post {side} {sign:+.0f}")


# --------------------------------------------------------- K8r: the image-resident forward
def _relayout(w):
    from torch_scae_amd import _lib
    Co, Ci = w.shape[:2]
    n = _lib.load().scae_conv3x3_wf_floats(Co, Ci)
    wf = torch.full((n,), SENT, device="cuda")
    wd = torch.full((Ci, 9, Co), SENT, device="cuda")
    return wf, wd


def _packed_planes(wf, Co, Ci):
    """the three bf16 planes as the fragment-major copy holds them (conv_first_dev.h
    ``packed_index``), read back as (3, Co, 9, Ci) int32 bit patterns."""
    raw = wf[Co * 9 * Ci:].cpu().view(torch.int16).to(torch.int32) & 0xFFFF
    co = torch.arange(Co)[:, None, None]
    tap = torch.arange(9)[None, :, None]
    ci = torch.arange(Ci)[None, None, :]
    chunk = (co >> 5) * (9 * (Ci >> 5)) + tap * (Ci >> 5) + (ci >> 5)
    out = []
    for p in range(3):
        idx = ((((chunk * 2 + ((ci & 15) >> 3)) * 3 + p) * 64 + ((ci & 31) >> 4) * 32 +
                (co & 31)) << 3) + (ci & 7)
        out.append(raw[idx])
    return torch.stack(out)


@pytest.mark.parametrize("B,IH,Ci,Co,s,group,post", [
    (5, 7, 128, 128, 1, 0, True),      # the launcher's own group
    (7, 7, 128, 64, 1, 3, False),      # a forced group of three images, a last group of one
    (3, 9, 256, 96, 2, 1, True),       # stride 2, one image per workgroup, two channel blocks
])
@pytest.mark.parametrize("side", ["filter", "input"])
def test_conv_resident_forward_vs_fp64(B, IH, Ci, Co, s, group, post, side):
    """scae_conv3x3_fwd_res_f32 (K8r: filter planes pre-split in ``wp``, four K parts meet in
    LDS: x = 3).  ``wp`` from scae_conv3x3_relayout_f32; relayout_batch_f32 and the image
    layer's riding relayout write the same bits, and the planes in ``wp`` are split3(w)."""
    from torch_scae_amd import _lib
    lib = _lib.load()
    if group == 0:
        assert lib.scae_conv3x3_fwd_res_supported(B, IH, IH, Ci, Co, s) == 1
    g = torch.Generator().manual_seed(B * 100 + Ci + Co + s)
    OH = (IH - 3) // s + 1
    if side == "filter":
        x, w = E.full_mantissa(g, (B, IH, IH, Ci)), E.sparse_filter(g, Co, Ci, "fwd", lo_zero=0.3)
    else:
        x, w = E.sparse_pixels(g, B, IH, IH, Ci), E.full_mantissa(g, (Co, Ci, 3, 3))
    assert "fwd" in E.chunk_counts_ok(x, w, None, s)
    bias, pb = E.full_mantissa(g, (Co,), 4), E.full_mantissa(g, (Co, OH, OH), 4)
    t = E.kind_terms(E.op_fwd(s), x, w)
    xd, bd, pbd = _dev(x), _dev(bias), _dev(pb)
    for sign in (1.0, -1.0):
        wd_ = _dev(sign * w)
        wf, wd = _relayout(w)
        _call("scae_conv3x3_relayout_f32", _p(wd_), _p(wf), _p(wd), Co, Ci, _st())
        if sign > 0:
            wf2, wd2 = _relayout(w)
            _call("scae_conv3x3_relayout_batch_f32", 1, (P * 1)(wd_.data_ptr()),
                  (P * 1)(wf2.data_ptr()), (P * 1)(wd2.data_ptr()), (ctypes.c_int * 1)(Co),
                  (ctypes.c_int * 1)(Ci), _st())
            wf3, wd3 = _relayout(w)
            img = torch.rand(1, 1, 8, 8).cuda()
            w1, b1 = torch.rand(64, 1, 3, 3).cuda(), torch.rand(64).cuda()
            o1 = torch.empty(1, 6, 6, 64, device="cuda")
            _call("scae_conv3x3_first_fwd_relayout_f32", _p(img), _p(w1), _p(b1), _p(o1), 1, 1,
                  8, 8, 64, 1, 1, (P * 1)(wd_.data_ptr()), (P * 1)(wf3.data_ptr()),
                  (P * 1)(wd3.data_ptr()), (ctypes.c_int * 1)(Co), (ctypes.c_int * 1)(Ci), _st())
            torch.cuda.synchronize()
            for a, b in ((wf, wf2), (wf, wf3), (wd, wd2), (wd, wd3)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            planes = _packed_planes(wf, Co, Ci)
            want = torch.stack([E.bf16_bits(p) for p in E.split3(w.permute(0, 2, 3, 1).reshape(Co, 9, Ci))])
            assert torch.equal(planes, want)
            assert torch.equal(wf[:Co * 9 * Ci].cpu(), w.permute(0, 2, 3, 1).reshape(-1))
        out = torch.full((B, OH, OH, Co), SENT, device="cuda")
        outp = torch.full((B, OH, OH, Co), SENT, device="cuda") if post else None
        wp = P(wf.data_ptr() + 4 * Co * 9 * Ci)                # the fragment-major planes
        _call("scae_conv3x3_fwd_res_f32", _p(xd), wp, _p(bd), _p(out), _p(pbd) if post else None,
              _p(outp), B, IH, IH, Ci, Co, s, group, _st())
        torch.cuda.synchronize()
        ref, bound = E.x6_ref(dict(t, P=sign * t["P"]), x=3, extra=1, bias=bias.double())
        ref = ref.relu()
        _check(out, ref, bound, f"K8r {side} sign {sign:+.0f}")
        if post:
            refp = ref + pb.double().permute(1, 2, 0)
            boundp = bound + E.gamma(1) * (ref.abs() + bound + pb.double().abs().permute(1, 2, 0))
            _check(outp, refp, boundp, f"K8r post {side} {sign:+.0f}")


# ------------------------------------------------------------------- backward pair launch
def _wgrad_ref(dpre, x, s):
    t = E.kind_terms(E.op_wgrad(s), dpre, x)               # (Co, Ci, 3, 3)
    return t


def _check_partials(part, t, dpre, splits, Co, Ci, what):
    """the weight-gradient partials of every split summed in fp64 (no fp32 split sum: x = 0)
    and the bias partials."""
    n = 9 * Co * Ci
    pw = part[:splits * n].view(splits, 9, Co, Ci).double().cpu().sum(0)
    ref, bound = E.x6_ref(t)
    w = _check(pw, ref.permute(2, 3, 0, 1).reshape(9, Co, Ci),
               bound.permute(2, 3, 0, 1).reshape(9, Co, Ci), f"{what} dW partials")
    pb = part[splits * n:splits * (n + Co)].view(splits, Co).double().cpu().sum(0)
    d = dpre.double().reshape(-1, Co)
    cnt = (d != 0).sum(0)
    _check(pb, d.sum(0), E.gamma(cnt + 1) * d.abs().sum(0), f"{what} db partials")
    return w


PAIR = [
    # form, B, IH, IW, Ci, Co, stride, dgrad_forms
    ("DMODE 0 + PipeW16", 48, 19, 19, 256, 64, 2, E.NO_TILE | E.NO_KSPLIT),
    ("DMODE 2 + PipeW16 (cfg-2 layer 3)", 128, 9, 9, 128, 128, 1, E.NO_KSPLIT),
    ("DMODE 1 + PipeW16 (cfg-2 layer 4)", 128, 7, 7, 128, 128, 1, E.NO_KSPLIT),
    ("DMODE 4 + PipeW16", 3, 9, 11, 128, 64, 2, E.TILE),
    ("DMODE 5 + PipeW", 2, 10, 12, 256, 64, 2, 0),
]


@pytest.mark.parametrize("form,B,IH,IW,Ci,Co,s,forms", PAIR, ids=[p[0] for p in PAIR])
@pytest.mark.parametrize("side", ["dpre", "input"])
def test_conv_backward_pair_vs_fp64(form, B, IH, IW, Ci, Co, s, forms, side):
    """scae_conv3x3_bwd_pair_forms_f32: the gated input gradient (gate = the input > 0) and the
    weight-gradient partials.  side 'dpre': the pre-activation gradient sparse (both passes'
    premise), the input positive (gate open everywhere) -- and one shape with a signed input
    (a gate); side 'input': the input sparse and positive, dpre dense: the partials only (the
    data gradient's premise does not hold)."""
    from torch_scae_amd import _lib
    lib = _lib.load()
    OH, OW = (IH - 3) // s + 1, (IW - 3) // s + 1
    M = B * OH * OW
    assert (E.NO_TILE, E.NO_KSPLIT, E.TILE) == (_lib.DGRAD_NO_TILE, _lib.DGRAD_NO_KSPLIT,
                                                _lib.DGRAD_TILE)
    mode = E.dgrad_mode(B, IH, IW, Ci, Co, s, pair=True, forms=forms)
    assert f"DMODE {mode} " in form + " "
    w16 = mode != 5 and M < 8192
    assert ("PipeW16" in form) == w16
    g = torch.Generator().manual_seed(B * 31 + IH + Ci)
    gated = side == "dpre" and mode == 5
    if side == "dpre":
        x = E.full_mantissa(g, (B, IH, IW, Ci))
        x = x if gated else x.abs()
        dpre, w = E.sparse_dpre(g, B, OH, OW, Co), E.full_mantissa(g, (Co, Ci, 3, 3))
        assert {"dgrad", "wgrad"} <= E.chunk_counts_ok(x, w, dpre, s)
    else:
        x = E.sparse_input(g, B, IH, IW, Ci, s).abs()
        dpre, w = E.full_mantissa(g, (B, OH, OW, Co)), E.full_mantissa(g, (Co, Ci, 3, 3))
        assert "wgrad" in E.chunk_counts_ok(x, w, dpre, s)
    splits = lib.scae_conv3x3_wgrad_splits(B, OH, OW, Ci, Co)
    wd = _dev(w.permute(1, 2, 3, 0))                       # (ci, tap, co)
    xd, dd = _dev(x), _dev(dpre)
    outs = {}
    # the other run: the first-generation tiles (DMODE 4 / 5), or the default form (0 - 2)
    alt = E.NO_TILE | E.NO_KSPLIT if mode >= 4 else 0
    for run, dgrad_forms in (("form", forms), ("other", alt)):
        din = torch.full((B * IH * IW + 5, Ci), SENT, device="cuda")
        part = torch.full((splits * (9 * Co * Ci + Co) + 5,), SENT, device="cuda")
        _call("scae_conv3x3_bwd_pair_forms_f32", _p(dd), _p(wd), _p(xd), _p(din), _p(part),
              B, IH, IW, Ci, Co, s, dgrad_forms, _st())
        torch.cuda.synchronize()
        assert bool((din[-5:] == SENT).all()) and bool((part[-5:] == SENT).all())
        outs[run] = (din, part)
    assert not torch.equal(outs["form"][0], outs["other"][0])   # the selector switched the form
    din, part = outs["form"]
    if side == "dpre":
        t = E.kind_terms(E.op_dgrad(s, (IH, IW)), dpre, w, fp32=mode < 4)
        ref, bound = E.x6_ref(t, x=3) if mode >= 4 else E.fp32_ref(t, extra=3)
        open_ = x > 0
        ref = torch.where(open_, ref, torch.zeros_like(ref))
        bound = torch.where(open_, bound, torch.zeros_like(bound))
        _check(din[:-5].view(B, IH, IW, Ci), ref, bound, f"{form} din ({side})")
    _check_partials(part, _wgrad_ref(dpre, x, s), dpre, splits, Co, Ci, f"{form} ({side})")


@pytest.mark.parametrize("side,gate", [("filter", False), ("dpre", False), ("filter", True)])
def test_conv_dgrad_standalone_vs_fp64(side, gate):
    """scae_conv3x3_dgrad_f32 in its default form at this shape (DMODE 5: 50 tiles of 64 x 128
    < 500), with the sparse filter (Wd rows) and the sparse dpre, and
    one run with a gate."""
    B, IH, IW, Ci, Co, s = 2, 9, 9, 128, 128, 1
    assert E.dgrad_mode(B, IH, IW, Ci, Co, s, pair=False) == 5
    OH, OW = IH - 2, IW - 2
    g = torch.Generator().manual_seed(77 + gate)
    if side == "filter":
        dpre, w = E.full_mantissa(g, (B, OH, OW, Co)), E.sparse_filter(g, Co, Ci, "dgrad")
    else:
        dpre, w = E.sparse_dpre(g, B, OH, OW, Co), E.full_mantissa(g, (Co, Ci, 3, 3))
    assert "dgrad" in E.chunk_counts_ok(None, w, dpre, s)
    gt = E.full_mantissa(g, (B, IH, IW, Ci)) if gate else None
    din = torch.full((B * IH * IW + 5, Ci), SENT, device="cuda")
    dd, wdd, gd = _dev(dpre), _dev(w.permute(1, 2, 3, 0)), _dev(gt) if gate else None
    _call("scae_conv3x3_dgrad_f32", _p(dd), _p(wdd), _p(gd), _p(din), B, IH, IW, Ci, Co, s, _st())
    torch.cuda.synchronize()
    assert bool((din[-5:] == SENT).all())
    ref, bound = E.x6_ref(E.kind_terms(E.op_dgrad(s, (IH, IW)), dpre, w), x=3)
    if gate:
        ref = torch.where(gt > 0, ref, torch.zeros_like(ref))
        bound = torch.where(gt > 0, bound, torch.zeros_like(bound))
    _check(din[:-5].view(B, IH, IW, Ci), ref, bound, f"dgrad {side} gate={gate}")


@pytest.mark.parametrize("B,IH,Ci,Co,s,side", [
    (8, 9, 128, 64, 1, "dpre"),
    (8, 9, 128, 64, 1, "input"),
    (128, 19, 128, 128, 2, "dpre"),    # cfg-2's layer 2 (10 368 pixels)
    (128, 9, 128, 128, 1, "input"),    # cfg-2's layer 3
    (128, 7, 128, 128, 1, "dpre"),     # cfg-2's layer 4
])
def test_conv_wgrad_pipe_and_reduce_vs_fp64(B, IH, Ci, Co, s, side):
    """scae_conv3x3_wgrad_f32 (always PipeW, the 32-pixel ring) + scae_conv3x3_wgrad_reduce_
    batch_f32: dW and db after the fp32 sum over the splits (x = splits - 1)."""
    from torch_scae_amd import _lib
    lib = _lib.load()
    OH = (IH - 3) // s + 1
    g = torch.Generator().manual_seed(B + IH * 7 + (side == "dpre"))
    if side == "dpre":
        x, dpre = E.full_mantissa(g, (B, IH, IH, Ci)), E.sparse_dpre(g, B, OH, OH, Co)
    else:
        x, dpre = E.sparse_input(g, B, IH, IH, Ci, s), E.full_mantissa(g, (B, OH, OH, Co))
    assert "wgrad" in E.chunk_counts_ok(x, torch.zeros(Co, Ci, 3, 3), dpre, s)
    splits = lib.scae_conv3x3_wgrad_splits(B, OH, OH, Ci, Co)
    part = torch.full((splits * (9 * Co * Ci + Co) + 5,), SENT, device="cuda")
    dd = _dev(dpre)
    xd = _dev(x)
    _call("scae_conv3x3_wgrad_f32", _p(dd), _p(xd), _p(part), None, None,
          B, IH, IH, Ci, Co, s, _st())
    dw = torch.full((Co * Ci * 9 + 5,), SENT, device="cuda")
    db = torch.full((Co + 5,), SENT, device="cuda")
    _call("scae_conv3x3_wgrad_reduce_batch_f32", 1, (P * 1)(part.data_ptr()),
          (P * 1)(dw.data_ptr()), (P * 1)(db.data_ptr()), (ctypes.c_int * 1)(Co),
          (ctypes.c_int * 1)(Ci), (ctypes.c_int * 1)(splits), _st())
    torch.cuda.synchronize()
    assert bool((part[-5:] == SENT).all() and (dw[-5:] == SENT).all() and (db[-5:] == SENT).all())
    t = _wgrad_ref(dpre, x, s)
    _check_partials(part, t, dpre, splits, Co, Ci, f"PipeW B={B} {side}")
    ref, bound = E.x6_ref(t, x=splits - 1)
    _check(dw[:-5].view(Co, Ci, 3, 3), ref, bound, f"PipeW B={B} {side} dW, {splits} splits")
    d = dpre.double().reshape(-1, Co)
    _check(db[:-5], d.sum(0), E.gamma((d != 0).sum(0) + splits) * d.abs().sum(0), "db")


# -------------------------------------------------------------------------- image layer
@pytest.mark.parametrize("C0,s", [(1, 1), (1, 2), (3, 1), (3, 2)])
def test_conv_first_layer_vs_fp64(C0, s):
    """scae_conv3x3_first_fwd_f32 / first_wgrad_f32: fmaf chains (one rounding per term) and,
    in the weight gradient, the waves' partial rows summed in LDS (<= 4) -- exact fp64
    products and gamma(n + extra) sum |a b|."""
    from torch_scae_amd import _lib
    lib = _lib.load()
    B, IH, Co = 5, 17, 64
    OH = (IH - 3) // s + 1
    g = torch.Generator().manual_seed(C0 * 10 + s)
    img = E.full_mantissa(g, (B, C0, IH, IH)).abs()
    w, bias = E.full_mantissa(g, (Co, C0, 3, 3)), E.full_mantissa(g, (Co,), 4)
    M = B * OH * OH
    out = torch.full((M + 5, Co), SENT, device="cuda")
    imd, wdd, bd = _dev(img), _dev(w), _dev(bias)
    _call("scae_conv3x3_first_fwd_f32", _p(imd), _p(wdd), _p(bd), _p(out),
          B, C0, IH, IH, Co, s, _st())
    dpre = E.full_mantissa(g, (B, OH, OH, Co))
    rows = lib.scae_conv3x3_first_wgrad_rows(B, Co)
    part = torch.full((rows * Co * (C0 * 9 + 1) + 5,), SENT, device="cuda")
    dd = _dev(dpre)
    _call("scae_conv3x3_first_wgrad_f32", _p(dd), _p(imd), _p(part), B, C0, IH,
          IH, Co, s, _st())
    torch.cuda.synchronize()
    assert bool((out[M:] == SENT).all()) and bool((part[-5:] == SENT).all())
    xn = img.permute(0, 2, 3, 1)
    t = E.kind_terms(E.op_fwd(s), xn, w, fp32=True)
    ref, bound = E.fp32_ref(t, extra=1, bias=bias.double())
    _check(out[:M].view(B, OH, OH, Co), ref.relu(), bound, f"first fwd C0={C0} s={s}")
    K1 = C0 * 9
    pr = part[:-5].view(rows, Co * (K1 + 1)).double().cpu().sum(0)
    tw = E.kind_terms(E.op_wgrad(s), dpre, xn, fp32=True)
    ref, bound = E.fp32_ref(tw, extra=4)
    _check(pr[:Co * K1].view(Co, C0, 3, 3), ref, bound, f"first dW C0={C0} s={s}")
    d = dpre.double().reshape(-1, Co)
    _check(pr[Co * K1:], d.sum(0), E.gamma(d.shape[0] + 4) * d.abs().sum(0), "first db")


# ------------------------------------------------------------------- capsule-head GEMMs
@pytest.mark.parametrize("B,HW,C,AP,gsz", [
    (128, 25, 128, 576, 32),    # cfg-2's capsule head: K = 576 and 800
    (64, 9, 128, 160, 32),      # five K chunks: waves with one and with two
])
@pytest.mark.parametrize("side", ["dy", "operands"])
def test_gemm_pair_x6k_and_fp32_tiles_vs_fp64(B, HW, C, AP, gsz, side):
    """scae_gemm_pair_f32 on the 1 x 1 attention convolution's backward: dx = dy W gated (+ the
    ungated copy), dW per group = dy^T x (+ bias sums) -- x6k (form = 0, mode "1": four
    wave-private pipelines summed in LDS, x = 3) against the kind sum, gemm_mfma.hip's fp32
    tiles (form = SCAE_GEMM_TILES, mode "0") against the exact product; the two differ in their bits.  side 'dy': dy sparse
    (one term per row, 1 .. 4 per column in different 32-row blocks); 'operands': W and x
    sparse, dy dense."""
    from torch_scae_amd import _lib, ops
    g = torch.Generator().manual_seed(B + HW + (side == "dy"))
    S, kper, slab = B // gsz, HW * gsz, AP * C + AP
    if side == "dy":
        dy = E.sparse_dpre(g, 1, B * HW, 1, AP).view(B * HW, AP)
        w, x = E.full_mantissa(g, (AP, C)), E.full_mantissa(g, (B * HW, C))
    else:
        dy = E.full_mantissa(g, (B * HW, AP))
        w = E.sparse_rows(g, C, AP).T.contiguous()
        x = E.sparse_dpre(g, 1, B * HW, 1, C).view(B * HW, C)
    gate = E.full_mantissa(g, (B * HW, C))
    d_dy, d_w, d_x, d_g = _dev(dy), _dev(w), _dev(x), _dev(gate)
    outs = {}
    for mode in ("1", "0"):
        part = torch.full((S * slab + 5,), SENT, device="cuda")
        dx = torch.full((B * HW * C + 5,), SENT, device="cuda")
        raw = torch.full((B * HW * C + 5,), SENT, device="cuda")
        dgrad = ops._gemm_desc(ops._p(d_dy), ops._p(d_w), ops._p(dx), 1, B * HW, C, AP, True, AP,
                               0, False, C, 0, C, 0)
        dgrad.mask, dgrad.ldmask, dgrad.c_nomask = d_g.data_ptr(), C, raw.data_ptr()
        wgrad = ops._gemm_desc(ops._p(d_dy), ops._p(d_x), ops._p(part), S, AP, C, kper, False,
                               AP, kper * AP, False, C, kper * C, C, slab,
                               asum=ops._off(part, AP * C), asum_b=slab)
        wgrad.form = dgrad.form = 0 if mode == "1" else _lib.GEMM_TILES
        ops._gemm_pair(wgrad, dgrad, d_x)
        torch.cuda.synchronize()
        for t in (part, dx, raw):
            assert bool((t[-5:] == SENT).all())
        outs[mode] = (dx[:-5], raw[:-5], part[:-5])
    assert not any(torch.equal(a, b) for a, b in zip(outs["1"], outs["0"]))
    td = E.kind_terms(E.op_gemm, dy[None], w.T[None], fp32=False)
    tw = E.kind_terms(E.op_gemm, dy.view(S, kper, AP).transpose(1, 2), x.view(S, kper, C).transpose(1, 2))
    db_ref = dy.double().view(S, kper, AP).sum(1)
    db_bound = E.gamma(kper + 4) * dy.double().abs().view(S, kper, AP).sum(1)
    for mode in ("1", "0"):
        dx, raw, part = (t.double().cpu() for t in outs[mode])
        rd, bd = E.x6_ref(td, x=3) if mode == "1" else E.fp32_ref(td, extra=4)
        rw, bw = E.x6_ref(tw, x=3) if mode == "1" else E.fp32_ref(tw, extra=4)
        rd, bd = rd[0], bd[0]
        _check(raw.view(B * HW, C), rd, bd, f"KSPLIT={mode} {side} dx raw")
        open_ = gate.double() > 0
        _check(dx.view(B * HW, C), torch.where(open_, rd, 0 * rd), torch.where(open_, bd, 0 * bd),
               f"KSPLIT={mode} {side} dx gated")
        pv = part.view(S, slab)
        _check(pv[:, :AP * C].view(S, AP, C), rw, bw, f"KSPLIT={mode} {side} dW")
        _check(pv[:, AP * C:], db_ref, db_bound, f"KSPLIT={mode} {side} db")


@pytest.mark.parametrize("nprob", [1, 3, 4])
def test_gemm_multi_x6k_vs_fp64(nprob):
    """scae_gemm_multi_f32 with 1, 3 and 4 weight-gradient problems of the capsule head's form
    (both operands k-strided, groups of images): x6k at form = 0 (mode "1"), the fp32 tiles at
    form = SCAE_GEMM_TILES (mode "0"), each problem against its own reference."""
    from torch_scae_amd import _lib, ops
    g = torch.Generator().manual_seed(40 + nprob)
    shapes = [(4, 96, 64, 800), (2, 64, 128, 288), (3, 32, 64, 224), (1, 128, 64, 128)][:nprob]
    probs = []
    for G, n, k, rows in shapes:
        a, b = E.sparse_dpre(g, 1, G * rows, 1, n).view(G, rows, n), E.full_mantissa(g, (G, rows, k))
        probs.append((G, n, k, rows, a, b))
    outs = {}
    for mode in ("1", "0"):
        descs = (_lib.GemmDesc * nprob)()
        keep = []
        for i, (G, n, k, rows, a, b) in enumerate(probs):
            da, db_ = _dev(a), _dev(b)
            c = torch.full((G * n * k + 5,), SENT, device="cuda")
            keep += [da, db_, c]
            descs[i] = ops._gemm_desc(ops._p(da), ops._p(db_), ops._p(c), G, n, k, rows, False,
                                      n, rows * n, False, k, rows * k, k, n * k)
            descs[i].form = 0 if mode == "1" else _lib.GEMM_TILES
        _call("scae_gemm_multi_f32", descs, nprob, _st())
        torch.cuda.synchronize()
        outs[mode] = [keep[3 * i + 2] for i in range(nprob)]
    for i, (G, n, k, rows, a, b) in enumerate(probs):
        assert bool((outs["1"][i][-5:] == SENT).all() and (outs["0"][i][-5:] == SENT).all())
        t = E.kind_terms(E.op_gemm, a.transpose(1, 2), b.transpose(1, 2))
        for mode in ("1", "0"):
            ref, bound = E.x6_ref(t, x=3) if mode == "1" else E.fp32_ref(t, extra=4)
            _check(outs[mode][i][:-5].view(G, n, k), ref, bound, f"multi {i}/{nprob} KSPLIT={mode}")
    assert not all(torch.equal(a, b) for a, b in zip(outs["1"], outs["0"]))
