"""The weight gradient's tile forms (scae_hip.h: SCAE_WGRAD_TILE_*) write the partial slabs of
the 64 x 64 form bit for bit: an output element's chain of products depends on the split's
pixel range, the chunk order, the order of the 16-k batches and the six bf16 products, none of
which the tile shape enters.  The reference of every case is the 64 x 64 form of the same build
(pinned to fp64 by test_x6_kernels_vs_fp64.py); the comparison is equality of bits over the whole
partial buffer (splits x 9 x Cout x Cin slab entries and splits x Cout bias rows) and, for the
pair launches, the input gradient."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p

# (B, IH = IW, Cin, Cout, stride)
ONE_SPLIT_RAGGED = (2, 7, 128, 128, 1)       # M = 50: one split, the second chunk ragged
TWO_SPLITS_RAGGED = (8, 19, 128, 128, 2)     # M = 648: per = 352 and 296, the last chunk ragged
SHORT_RING = (30, 9, 128, 128, 1)            # M = 1470 < 8192 pixels: per = 304 there, 320 alone
FALLBACK = [(8, 19, 64, 128, 2), (8, 19, 128, 64, 2)]
RIDER = (128, 9, 128, 128, 1)                # the encoder's third layer at B = 128


def _lib_():
    from torch_scae_amd import _lib
    return _lib


def _tiles():
    L = _lib_()
    return {"64x64": L.WGRAD_TILE_64x64, "128x64": L.WGRAD_TILE_128x64}


# every code the library offers beside the plain 64 x 64 form: (shape, SCAE_WGRAD_HEAD or not)
OFFERED = [("128x64", 0), ("128x64", 1), ("64x64", 1)]


def _code(shape, head=0):
    return _tiles()[shape] + (_lib_().WGRAD_HEAD if head else 0)


def _st():
    return P(torch.cuda.current_stream().cuda_stream)


_OPERANDS = {}


def _operands(shape):
    """seeded operands of a layer, made once per shape and never written"""
    if shape not in _OPERANDS:
        B, IH, Ci, Co, s = shape
        OH = (IH - 3) // s + 1
        g = torch.Generator().manual_seed(sum(shape))
        x = torch.relu(torch.randn(B, IH, IH, Ci, generator=g)).cuda()
        wd = (torch.randn(Ci, 9, Co, generator=g) * 0.05).cuda()
        dpre = torch.randn(B, OH, OH, Co, generator=g).cuda()
        splits = _lib_().load().scae_conv3x3_wgrad_splits(B, OH, OH, Ci, Co)
        _OPERANDS[shape] = (x, wd, dpre, splits)
    return _OPERANDS[shape]


def _pair(shape, forms, tile):
    """scae_conv3x3_bwd_pair_tile_f32 -> (din, partial)"""
    B, IH, Ci, Co, s = shape
    x, wd, dpre, splits = _operands(shape)
    din = torch.full((B, IH, IH, Ci), 7.0, device="cuda")
    part = torch.full((splits * (9 * Co * Ci + Co),), 7.0, device="cuda")
    _lib_().call("scae_conv3x3_bwd_pair_tile_f32", P(dpre.data_ptr()), P(wd.data_ptr()),
                 P(x.data_ptr()), P(din.data_ptr()), P(part.data_ptr()), B, IH, IH, Ci, Co, s,
                 forms, _st(), tile)
    torch.cuda.synchronize()
    return din, part


def _alone(shape, tile):
    """scae_conv3x3_wgrad_tile_f32 (dw == NULL) -> partial"""
    B, IH, Ci, Co, s = shape
    x, wd, dpre, splits = _operands(shape)
    part = torch.full((splits * (9 * Co * Ci + Co),), 7.0, device="cuda")
    _lib_().call("scae_conv3x3_wgrad_tile_f32", P(dpre.data_ptr()), P(x.data_ptr()),
                 P(part.data_ptr()), None, None, B, IH, IH, Ci, Co, s, _st(), tile)
    torch.cuda.synchronize()
    return part


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


_REF = {}


def _ref_pair(shape, forms):
    if (shape, forms) not in _REF:
        _REF[shape, forms] = _pair(shape, forms, _code("64x64"))
    return _REF[shape, forms]


def _ref_alone(shape):
    if shape not in _REF:
        _REF[shape] = _alone(shape, _code("64x64"))
    return _REF[shape]


@pytest.mark.parametrize("shape", [ONE_SPLIT_RAGGED, TWO_SPLITS_RAGGED],
                         ids=["one split", "two splits"])
@pytest.mark.parametrize("tile", [t for t in OFFERED if not t[1]], ids=str)
def test_the_stand_alone_weight_gradient_of_every_tile_equals_the_64x64_form(shape, tile):
    B, IH, Ci, Co, s = shape
    OH = (IH - 3) // s + 1
    splits = _operands(shape)[3]
    assert splits == (1 if shape == ONE_SPLIT_RAGGED else 2)
    if shape == TWO_SPLITS_RAGGED:   # per = 352: the second split has 296 pixels, 8 in its last chunk
        assert B * OH * OH == 648 and (324 + 31) // 32 * 32 == 352 and (648 - 352) % 32 == 8
    ref = _ref_alone(shape)
    assert not bool((ref == 7.0).any())
    assert _same_bits(_alone(shape, _code(*tile)), ref)


@pytest.mark.parametrize("tile", OFFERED, ids=str)
def test_the_16_pixel_ring_of_a_short_layer_equals_the_64x64_form(tile):
    """a layer below SCAE_WGRAD_SHORT_CHUNK_PIXELS whose data-gradient form is not the K-split
    tile: its weight-gradient tiles walk 16-pixel chunks (and `per` is a multiple of 16, not 32)"""
    B, IH, Ci, Co, s = SHORT_RING
    OH = (IH - 3) // s + 1
    splits = _operands(SHORT_RING)[3]
    per16 = ((B * OH * OH + splits - 1) // splits + 15) // 16 * 16
    assert B * OH * OH < 8192 and per16 % 32 == 16, (splits, per16)
    forms = _lib_().DGRAD_TILE
    din, part = _ref_pair(SHORT_RING, forms)
    # the pair's slabs differ from the stand-alone launch's (32-pixel quantum): the short ring ran
    assert not _same_bits(part, _ref_alone(SHORT_RING))
    d, p = _pair(SHORT_RING, forms, _code(*tile))
    assert _same_bits(p, part) and _same_bits(d, din)


@pytest.mark.parametrize("shape", FALLBACK, ids=["64 -> 128", "128 -> 64"])
@pytest.mark.parametrize("tile", ["128x64"])
def test_a_tile_the_channels_do_not_divide_falls_back_and_equals_the_64x64_form(shape, tile):
    """64 -> 128 takes the 128 x 64 tile (one column of tiles), 128 -> 64 falls back"""
    assert _same_bits(_alone(shape, _code(tile)), _ref_alone(shape))
    din, part = _ref_pair(shape, 0)
    d, p = _pair(shape, 0, _code(tile, head=1))
    assert _same_bits(p, part) and _same_bits(d, din)


@pytest.mark.parametrize("forms", [0, 1, 2, 3, 4, 6],
                         ids=["by shape", "NO_TILE", "NO_KSPLIT", "NO_TILE|NO_KSPLIT", "TILE",
                              "TILE|NO_KSPLIT"])
@pytest.mark.parametrize("tile", OFFERED, ids=str)
def test_the_pair_launch_of_every_tile_and_data_gradient_form_equals_the_64x64_form(forms, tile):
    L = _lib_()
    assert (L.DGRAD_NO_TILE, L.DGRAD_NO_KSPLIT, L.DGRAD_TILE) == (1, 2, 4)
    din, part = _ref_pair(TWO_SPLITS_RAGGED, forms)
    assert not bool((part == 7.0).any()) and not bool((din == 7.0).all())
    d, p = _pair(TWO_SPLITS_RAGGED, forms, _code(*tile))
    assert _same_bits(p, part) and _same_bits(d, din)
    # by shape: the planner's own choice writes the same bits
    d, p = _pair(TWO_SPLITS_RAGGED, forms, L.WGRAD_TILE_BY_SHAPE)
    assert _same_bits(p, part) and _same_bits(d, din)


def test_rider_launches_by_shape_equal_the_plain_pair_launch_of_the_planned_tile():
    """scae_conv3x3_bwd_pair_reduce_f32 / _fold_f32 take the planner's tile: din and the partial
    slabs equal scae_conv3x3_bwd_pair_tile_f32 of that tile, and of the 64 x 64 form"""
    from torch_scae_amd import ops
    L = _lib_()
    lib = L.load()
    B, IH, Ci, Co, s = RIDER
    planned = lib.scae_conv3x3_wgrad_tile_plan(B, IH, IH, Ci, Co, s, 0)
    assert planned == _code("128x64", head=1)   # a layer that takes the new tile
    x, wd, dpre, splits = _operands(RIDER)
    g = torch.Generator().manual_seed(34)
    rnd = lambda *shape: torch.randn(*shape, generator=g).cuda()   # noqa: E731
    new = lambda *shape: torch.empty(*shape, device="cuda")        # noqa: E731
    O, C, D, rows = 24, 256, 16, 128
    partial_rows, q, wk = rnd(rows, O * D + C * D + C), rnd(O, C), rnd(C, D)
    shapes = [(O, C), (C, C), (C,), (C, C), (C,), (C, C), (C,), (C, C), (C,), (C, D), (C,)]
    vals = [rnd(*sh) / sh[-1] ** .5 for sh in shapes]
    fold_outs = (new(O, C), new(C, D), new(C), new(C, D), new(C), new(C, D + 1), new(C, C))
    L.call("scae_seed_fold_fwd_f32", ctypes.byref(ops._fold_desc(vals, fold_outs, O, C, D)), _st())
    red_out = [new(O, C), new(C, D), new(C), new(C, D), new(C)]
    outs = {}
    for which in ("reduce", "fold"):
        din = torch.full((B, IH, IH, Ci), 7.0, device="cuda")
        part = torch.full((splits * (9 * Co * Ci + Co),), 7.0, device="cuda")
        pair = (P(dpre.data_ptr()), P(wd.data_ptr()), P(x.data_ptr()), P(din.data_ptr()),
                P(part.data_ptr()), B, IH, IH, Ci, Co, s)
        if which == "reduce":
            L.call("scae_conv3x3_bwd_pair_reduce_f32", *pair, ops._p(partial_rows), rows,
                   ops._p(q), ops._p(wk), *[ops._p(t) for t in red_out], O, C, 0, _st())
        else:
            desc, gr = ops._fold_desc(vals, fold_outs, O, C, D), L.SeedFoldGrads()
            for name, t in zip(("g_q", "g_wkf", "g_bkf", "g_wvf", "g_bvf"), red_out):
                setattr(gr, name, t.data_ptr())
            grads = [torch.empty_like(v) for v in vals]
            for name, t in zip(ops._FOLD_INPUTS, grads):
                setattr(gr, "d_" + name, t.data_ptr())
            L.call("scae_conv3x3_bwd_pair_fold_f32", *pair, ctypes.byref(desc), ctypes.byref(gr),
                   0, _st())
        torch.cuda.synchronize()
        outs[which] = (din, part)
    for tile in (planned, _code("64x64")):
        din, part = _pair(RIDER, 0, tile)
        for which in ("reduce", "fold"):
            assert _same_bits(outs[which][0], din) and _same_bits(outs[which][1], part), \
                (which, tile)


def _rejected_without_a_launch(fn, *args):
    """rc of fn(*args[:-1], stream, args[-1]) -- the tile selector follows the stream -- and the
    number of launches a recording around it saw"""
    lib = _lib_().load()
    torch.cuda.synchronize()
    lst = lib.scae_launch_list_begin(_st())
    assert lst
    try:
        rc = getattr(lib, fn)(*args[:-1], _st(), args[-1])
        assert lib.scae_launch_list_end(P(lst)) == 0
        return rc, lib.scae_launch_list_size(P(lst))
    finally:
        lib.scae_launch_list_free(P(lst))


@pytest.mark.parametrize("tile", [3, 4, 8 + 2, 32 + 2, 64, 128 + 2, -1],
                         ids=["shape 3", "shape 4", "bit 8", "bit 32", "head without a shape",
                              "bit 128", "negative"])
def test_a_wgrad_tile_outside_its_set_is_an_error_and_nothing_is_launched(tile):
    L = _lib_()
    B, IH, Ci, Co, s = TWO_SPLITS_RAGGED
    x, wd, dpre, splits = _operands(TWO_SPLITS_RAGGED)
    din = torch.full((B, IH, IH, Ci), 7.0, device="cuda")
    part = torch.full((splits * (9 * Co * Ci + Co),), 7.0, device="cuda")
    pair = (P(dpre.data_ptr()), P(wd.data_ptr()), P(x.data_ptr()), P(din.data_ptr()),
            P(part.data_ptr()), B, IH, IH, Ci, Co, s, 0)
    alone = (P(dpre.data_ptr()), P(x.data_ptr()), P(part.data_ptr()), None, None, B, IH, IH, Ci,
             Co, s)
    assert _rejected_without_a_launch("scae_conv3x3_bwd_pair_tile_f32", *pair, tile) == \
        (L.ERR_BAD_ARG, 0)
    assert _rejected_without_a_launch("scae_conv3x3_wgrad_tile_f32", *alone, tile) == \
        (L.ERR_BAD_ARG, 0)
    torch.cuda.synchronize()
    assert bool((din == 7.0).all()) and bool((part == 7.0).all())
    good = _code("128x64")           # the same arguments with a tile of the set
    assert _rejected_without_a_launch("scae_conv3x3_bwd_pair_tile_f32", *pair, good) == (0, 1)
    assert _rejected_without_a_launch("scae_conv3x3_wgrad_tile_f32", *alone, good) == (0, 1)
