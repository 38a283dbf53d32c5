"""``affine=`` views of a resident dataset on the CPU path: RandomAffine's degrees / scale /
shear with nearest-neighbour resampling.  ``degrees=0`` alone is the view without ``affine``
bit for bit; ``affine_warp`` agrees with Pillow's fixed-point AFFINE path on every pixel
(live, and against the recorded fixture tests/golden/affine_nearest_pil.npz); the draws stay
in their ranges and depend on (seed, epoch, position) alone; a wrapped position keeps its own
draw; bad arguments are refused; ``state_dict`` carries the argument."""
import math
import os

import numpy as np
import pytest
import torch

from torch_scae_amd import data as D

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "affine_nearest_pil.npz")
FULL = dict(degrees=25, scale=(0.8, 1.2), shear=(-10, 10, -5, 5))


def _dataset(n, C=1, h=28, out=40, u8=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (n, C, h, h), generator=g, dtype=torch.uint8)
    if not u8:
        imgs = torch.rand(n, C, h, h, generator=g)
    labels = torch.randint(0, 10, (n,), generator=g)
    return D.ResidentDataset(imgs, labels, out_size=(out, out), device="cpu")


# -- 1. degrees = 0 is the view without affine -----------------------------------------------
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("drop_last", [True, False])
@pytest.mark.parametrize("u8, C, h, out", [(True, 1, 28, 40), (False, 3, 32, 32),
                                           (True, 3, 27, 40)])
def test_zero_degrees_equals_the_view_without_affine(shuffle, drop_last, u8, C, h, out):
    ds = _dataset(101, C, h, out, u8)
    args = dict(shuffle=shuffle, seed=9, drop_last=drop_last)
    plain, warped = ds.view(**args), ds.view(affine=dict(degrees=0), **args)
    B = 16
    assert warped.steps_in_epoch(B) == plain.steps_in_epoch(B) == (6 if drop_last else 7)
    for epoch in (0, 1, 5):
        for step in range(plain.steps_in_epoch(B)):
            wi, wl = warped.batch(epoch, step, B)
            pi, pl = plain.batch(epoch, step, B)
            assert wi.dtype == torch.float32 and torch.equal(wi, pi), (epoch, step)
            assert torch.equal(wl, pl), (epoch, step)
    # (an untranslated view likewise: the identity map)
    a = ds.view(translate=False, affine=dict(degrees=0), **args).batch(2, 1, B)[0]
    assert torch.equal(a, ds.view(translate=False, **args).batch(2, 1, B)[0])


# -- 2. Pillow, live ---------------------------------------------------------------------------
def _pil_matrix(k):
    k = [float(v) for v in k]
    return (k[0] / 65536, k[1] / 65536, (k[2] - 0.5 * k[0] - 0.5 * k[1]) / 65536,
            k[3] / 65536, k[4] / 65536, (k[5] - 0.5 * k[3] - 0.5 * k[4]) / 65536)


def _pil_warp(images, coeffs, out_size):
    from PIL import Image
    N, C, h, w = images.shape
    H, W = out_size
    ph, pw = (H - h) // 2, (W - w) // 2
    out = np.zeros((N, C, H, W), np.uint8)
    for n in range(N):
        for c in range(C):
            padded = np.zeros((H, W), np.uint8)
            padded[ph:ph + h, pw:pw + w] = images[n, c]
            got = Image.fromarray(padded).transform(
                (W, H), Image.AFFINE, data=_pil_matrix(coeffs[n]), resample=Image.NEAREST,
                fillcolor=0)
            out[n, c] = np.asarray(got)
    return out


PIL_CASES = [
    # affine, translate, C, h -> H
    (dict(degrees=30), True, 1, 28, 40),
    (dict(degrees=(-180, 180), scale=(0.6, 1.5)), True, 1, 28, 40),
    (FULL, True, 1, 28, 40),
    (dict(degrees=15, shear=20), False, 1, 28, 40),
    (dict(degrees=(10, 45), scale=(0.9, 1.1), shear=(0, 0, -15, 15)), True, 3, 32, 32),
    (dict(degrees=0), True, 1, 28, 40),                  # (translation only)
    (dict(degrees=0, shear=(5, 25)), True, 1, 30, 40),
]


@pytest.mark.parametrize("case", PIL_CASES)
def test_affine_warp_equals_pillow_nearest(case):
    pytest.importorskip("PIL")
    affine, translate, C, h, H = case
    N = 300
    g = torch.Generator().manual_seed(h + H + C)
    images = torch.randint(0, 256, (N, C, h, h), generator=g, dtype=torch.uint8)
    k = D.affine_coefficients(torch.arange(N), 3, 1234, ((H - h) // 2,) * 2, (H, H), affine,
                              translate)
    # the comparison's ground: an off-diagonal term, or the identity linear part (Pillow
    # resamples pure scale on another path)
    keep = (k[:, 1] != 0) | (k[:, 3] != 0) | ((k[:, 0] == 65536) & (k[:, 4] == 65536))
    assert int(keep.sum()) >= N - 5
    images, k = images[keep], k[keep]
    got = D.affine_warp(images, k, (H, H))
    want = torch.from_numpy(_pil_warp(images.numpy(), k.numpy(), (H, H)))
    assert torch.equal(got, want.to(torch.float32) / 255.0)
    differing = int((got != want.to(torch.float32) / 255.0).sum())
    assert differing == 0
    if affine != dict(degrees=0):
        assert not torch.equal(got, D.pad_and_translate(images, (H, H),
                                                        shifts=torch.zeros(len(k), 2).long()))


# -- 3. the recorded fixture -------------------------------------------------------------------
def test_golden_fixture_is_small_and_within_the_comparison():
    assert os.path.getsize(GOLDEN) < 1 << 20
    z = np.load(GOLDEN)
    assert z["coeffs_a"].shape[0] + z["coeffs_b"].shape[0] <= 64
    for g in "ab":
        k = z["coeffs_" + g].astype(np.int64)
        assert ((k[:, 1] != 0) | (k[:, 3] != 0) | ((k[:, 0] == 65536) & (k[:, 4] == 65536))).all()
        assert (k[:, 1] != 0).sum() >= len(k) - 4    # (mostly rotations and shears)


@pytest.mark.parametrize("group, out", [("a", 40), ("b", 32)])
def test_affine_warp_equals_the_recorded_pillow_pixels(group, out):
    z = np.load(GOLDEN)
    images = torch.from_numpy(z["images_" + group])
    coeffs = torch.from_numpy(z["coeffs_" + group])
    want = torch.from_numpy(z["pil_" + group])
    got = D.affine_warp(images, coeffs, (out, out))
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got, want.to(torch.float32) / 255.0)
    # float datasets take the same texels
    gotf = D.affine_warp(images.to(torch.float32) / 255.0, coeffs, (out, out))
    assert torch.equal(gotf, got)


# -- 4. draws, determinism, wrap, validation, state -------------------------------------------
def _decompose(k):
    """(angle in degrees, scale, shear-x in degrees) back out of k0, k1, k3, k4 of draws with
    shear-y = 0: M = [d, -b; -c, a] / s with a = cos r, c = sin r, b = -cos r tan sx - sin r,
    d = -sin r tan sx + cos r, hence a b + c d = -tan sx."""
    m0, m1, m3, m4 = (k[:, i].to(torch.float64) / 65536 for i in (0, 1, 3, 4))
    s = 1.0 / torch.sqrt(m3 * m3 + m4 * m4)
    a, b, c, d = m4 * s, -m1 * s, -m3 * s, m0 * s
    return torch.rad2deg(torch.atan2(c, a)), s, torch.rad2deg(torch.atan(-(a * b + c * d)))


def test_draws_stay_in_their_ranges_and_fill_them():
    N, H = 4000, 40
    p = torch.arange(N)
    k = D.affine_coefficients(p, 0, 5, (6, 6), (H, H),
                              dict(degrees=(-20, 40), scale=(0.7, 1.3), shear=(-8, 12)))
    rot, s, sx = _decompose(k)
    tol = 0.02                                      # (16.16 quantisation of the matrix)
    assert rot.min() >= -20 - tol and rot.max() <= 40 + tol
    assert rot.min() < -19 and rot.max() > 39 and abs(float(rot.mean()) - 10) < 1.5
    assert s.min() >= 0.7 - 1e-3 and s.max() <= 1.3 + 1e-3
    assert s.min() < 0.71 and s.max() > 1.29 and abs(float(s.mean()) - 1.0) < 0.02
    assert sx.min() >= -8 - tol and sx.max() <= 12 + tol
    assert sx.min() < -7.5 and sx.max() > 11.5
    # a number d means (-d, d); missing scale is exactly 1, missing shear exactly 0
    k = D.affine_coefficients(p, 0, 5, (6, 6), (H, H), dict(degrees=10))
    rot, s, sx = _decompose(k)
    assert rot.min() >= -10 - tol and rot.max() <= 10 + tol and rot.min() < -9.5
    assert (s - 1).abs().max() < 1e-4 and sx.abs().max() < 0.01
    # shear-y alone: k4 = a / s = cos(rot - sy) / cos(sy) with rot = 0 is exactly 1
    k = D.affine_coefficients(p, 0, 5, (6, 6), (H, H),
                              dict(degrees=0, shear=(0, 0, -15, 15)))
    assert bool((k[:, 4] == 65536).all()) and bool((k[:, 1] == 0).all())
    sy = torch.rad2deg(torch.atan(k[:, 3].to(torch.float64) / 65536))   # -c = tan sy
    assert sy.min() >= -15 - tol and sy.max() <= 15 + tol and sy.min() < -14.5 < 14.5 < sy.max()


def test_translation_is_the_existing_shift_draw():
    """With the identity linear part k2, k5 hold exactly the view's own shifts."""
    p = torch.arange(500)
    k = D.affine_coefficients(p, 2, 77, (6, 4), (40, 36), dict(degrees=0))
    sh = D.translate_shifts(p, 2, 77, (6, 4))
    assert torch.equal(k[:, 2], -sh[:, 1] * 65536 + 32768)
    assert torch.equal(k[:, 5], -sh[:, 0] * 65536 + 32768)
    k0 = D.affine_coefficients(p, 2, 77, (6, 4), (40, 36), dict(degrees=0), translate=False)
    assert bool((k0 == torch.tensor([65536, 0, 32768, 0, 65536, 32768])).all())


def test_coefficients_depend_on_seed_epoch_and_position_alone():
    args = ((6, 6), (40, 40), FULL)
    p = torch.arange(257)
    k = D.affine_coefficients(p, 3, 11, *args)
    assert k.dtype == torch.int64 and tuple(k.shape) == (257, 6)
    assert torch.equal(k, D.affine_coefficients(p, 3, 11, *args))
    # position by position, and in another order: the same rows
    for q in (0, 1, 100, 256):
        assert torch.equal(D.affine_coefficients(torch.tensor([q]), 3, 11, *args)[0], k[q])
    perm = torch.randperm(257, generator=torch.Generator().manual_seed(0))
    assert torch.equal(D.affine_coefficients(perm, 3, 11, *args), k[perm])
    # another seed, epoch (low or high word) or position: another draw
    assert not torch.equal(k, D.affine_coefficients(p, 3, 12, *args))
    assert not torch.equal(k, D.affine_coefficients(p, 4, 11, *args))
    assert not torch.equal(k, D.affine_coefficients(p, 3 + (1 << 32), 11, *args))
    assert not torch.equal(k, D.affine_coefficients(p, 3, 11 + (1 << 32), *args))
    assert len({tuple(r) for r in k[:, [0, 1, 3, 4]].tolist()}) == 257
    # its own Philox stream: the angle is not the shift draw's word
    sh = D.affine_coefficients(p, 3, 11, (6, 6), (40, 40), dict(degrees=0))
    assert not torch.equal(sh[:, 2], k[:, 2])


def test_the_definition_on_one_position_in_python_floats():
    """One row recomputed with the math module from the specification's text."""
    H, W, pads, seed, epoch, q = 40, 36, (6, 4), 99, 7, 13
    rng = dict(degrees=(-30.0, 50.0), scale=(0.75, 1.5), shear=(-10.0, 20.0, -5.0, 8.0))
    pt = torch.tensor([q])
    c = D._philox([pt, D._word(epoch, pt), D._word(epoch >> 32, pt),
                   D._word(0x4146464E, pt)], seed & 0xFFFFFFFF, seed >> 32, 10)
    r = [int(w) >> 8 for w in c]
    val = [lo + (hi - lo) * rr / 2 ** 24 for rr, (lo, hi) in zip(
        r, (rng["degrees"], rng["scale"], rng["shear"][:2], rng["shear"][2:]))]
    rot, sx, sy, scale = math.radians(val[0]), math.radians(val[2]), math.radians(val[3]), val[1]
    ty, tx = D.translate_shifts(pt, epoch, seed, pads)[0].tolist()
    cx, cy = W * 0.5, H * 0.5
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    cc = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    M = [v / scale for v in (d, -b, 0.0, -cc, a, 0.0)]
    M[2] += M[0] * (-cx - tx) + M[1] * (-cy - ty) + cx
    M[5] += M[3] * (-cx - tx) + M[4] * (-cy - ty) + cy

    def fix(v):
        return math.floor(v * 65536 + 0.5)
    want = [fix(M[0]), fix(M[1]), fix(M[2] + M[0] * 0.5 + M[1] * 0.5),
            fix(M[3]), fix(M[4]), fix(M[5] + M[3] * 0.5 + M[4] * 0.5)]
    got = D.affine_coefficients(pt, epoch, seed, pads, (H, W), rng)[0].tolist()
    # (libm and the tensor library may round sin / cos / tan differently in the last place --
    # a few 1e-16 on a matrix term, below 1e-14 on M[2] / M[5] after the centre's factor of at
    # most 26: FIX's floor can then fall either side of an integer, one unit and no more)
    assert all(abs(g - w) <= 1 for g, w in zip(got, want)), (got, want)


def test_sampling_is_the_integer_rule_pixel_by_pixel():
    g = torch.Generator().manual_seed(4)
    img = torch.randint(0, 256, (3, 2, 5, 7), generator=g, dtype=torch.uint8)
    H, W, ph, pw = 9, 12, 2, 2
    k = torch.tensor([[60000, -30000, 123456, 25000, 70000, -200000],
                      [-65536, 0, 12 * 65536 - 1, 0, -65536, 9 * 65536 - 1],   # (180 degrees)
                      [131072, 0, 0, 0, 32768, 65536]])
    got = D.affine_warp(img, k, (H, W))
    for n in range(3):
        k0, k1, k2, k3, k4, k5 = k[n].tolist()
        for i in range(H):
            for j in range(W):
                xin, yin = (k2 + k1 * i + k0 * j) >> 16, (k5 + k4 * i + k3 * j) >> 16
                y, x = yin - ph, xin - pw
                for c in range(2):
                    want = float(img[n, c, y, x].float() / 255.0) \
                        if 0 <= y < 5 and 0 <= x < 7 else 0.0
                    assert float(got[n, c, i, j]) == want, (n, c, i, j)
    with pytest.raises(ValueError):
        D.affine_warp(img, k[:2], (H, W))
    with pytest.raises(ValueError):
        D.affine_warp(img, k, (4, 12))


def test_a_wrapped_position_reads_the_row_of_p_minus_n_and_keeps_its_own_draw():
    ds = _dataset(70)
    B = 16
    for shuffle in (False, True):
        v4 = ds.view(shuffle=shuffle, seed=3, drop_last=False, affine=FULL, world=4, rank=3)
        assert v4.remainder(B) == 2     # 70 - 64 = 6 -> ceil(6 / 4) = 2: 8 positions, 2 padded
        pos = v4.positions(v4.steps_per_epoch(B), B)
        assert pos.tolist() == [70, 71]
        image, label = v4.batch(1, v4.steps_per_epoch(B), B)
        rows, _ = v4.rows_and_shifts(1, pos)
        rows0, _ = v4.rows_and_shifts(1, pos - 70)
        assert torch.equal(rows, rows0)
        k_own = v4.coefficients(1, pos)
        k_first = v4.coefficients(1, pos - 70)
        assert not torch.equal(k_own, k_first)
        assert torch.equal(image, D.affine_warp(ds.images[rows], k_own, (40, 40)))
        assert not torch.equal(image, D.affine_warp(ds.images[rows], k_first, (40, 40)))
        assert torch.equal(label, ds.labels[rows])


def test_affine_batches_differ_from_translated_ones_and_change_per_epoch():
    ds = _dataset(64, 3, 32, 32)
    plain, warped = ds.view(seed=1), ds.view(seed=1, affine=dict(degrees=20))
    a, la = warped.batch(0, 0, 32)
    assert torch.equal(plain.batch(0, 0, 32)[0], ds.images[:32].float() / 255.0)  # (no-op)
    assert not torch.equal(a, plain.batch(0, 0, 32)[0])     # (32 -> 32 is augmented now)
    assert torch.equal(la, plain.batch(0, 0, 32)[1])
    assert not torch.equal(a, warped.batch(1, 0, 32)[0])
    assert torch.equal(a, warped.batch(0, 0, 32)[0])
    im, lb = warped.materialise(0)
    assert torch.equal(im[:32], a) and tuple(im.shape) == (64, 3, 32, 32)
    views = ds.split([40, 24], generator=torch.Generator().manual_seed(0),
                     affine=dict(degrees=5, scale=(0.9, 1.1)))
    assert all(v.affine == D.affine_ranges(dict(degrees=5, scale=(0.9, 1.1))) for v in views)


@pytest.mark.parametrize("bad", [
    dict(degrees=-5), dict(degrees=(10, -10)), dict(degrees=float("nan")),
    dict(degrees=(0, float("inf"))), dict(degrees=(1, 2, 3)), dict(degrees="x"),
    dict(degrees=0, scale=(0, 1)), dict(degrees=0, scale=(-1, 1)), dict(degrees=0, scale=1.0),
    dict(degrees=0, scale=(1.2, 0.8)), dict(degrees=0, scale=(1, float("nan"))),
    dict(degrees=0, shear=-3), dict(degrees=0, shear=(5, -5)), dict(degrees=0, shear=(1, 2, 3)),
    dict(degrees=0, shear=(0, 1, 5, 4)), dict(degrees=0, shear=(0, float("inf"))),
    dict(degrees=0, rotate=3), (10, 20), 15.0,
])
def test_bad_arguments_are_refused(bad):
    with pytest.raises(ValueError):
        _dataset(8).view(affine=bad)


def test_accepted_argument_forms():
    r = D.affine_ranges
    assert r(None) is None
    assert r(dict(degrees=10)) == dict(degrees=(-10.0, 10.0), scale=(1.0, 1.0),
                                       shear=(0.0, 0.0, 0.0, 0.0))
    assert r({}) == r(dict(degrees=0))
    assert r(dict(degrees=(5, 7), scale=(0.5, 2), shear=4))["shear"] == (-4.0, 4.0, 0.0, 0.0)
    assert r(dict(degrees=0, shear=(1, 2)))["shear"] == (1.0, 2.0, 0.0, 0.0)
    assert r(dict(degrees=0, shear=[1, 2, -3, 4]))["shear"] == (1.0, 2.0, -3.0, 4.0)
    assert r(dict(degrees=0, scale=None, shear=None)) == r(dict(degrees=0))
    assert r(r(FULL)) == r(FULL)
    # a map that leaves 16.16 fixed point in int32 is refused where the table is built
    with pytest.raises(ValueError):
        D.affine_coefficients(torch.arange(4), 0, 0, (6, 6), (40, 40),
                              dict(degrees=0, scale=(1e-6, 1e-6)))
    with pytest.raises(ValueError):
        D.affine_coefficients(torch.arange(4), 0, 0, (6, 6), (40, 40),
                              dict(degrees=0, shear=(90, 90)))


def test_state_dict_carries_the_argument():
    ds = _dataset(70)
    v = ds.view(shuffle=True, seed=5, affine=FULL, drop_last=False)
    for _ in range(7):
        v.take_step(16)
    sd = v.state_dict()
    assert sd["affine"] == {k: list(x) for k, x in D.affine_ranges(FULL).items()}
    w = ds.view()
    assert w.affine is None and w.state_dict()["affine"] is None
    w.load_state_dict(sd)
    assert w.affine == v.affine and (w.epoch, w.cursor) == (v.epoch, v.cursor)
    assert torch.equal(w.batch(1, 2, 16)[0], v.batch(1, 2, 16)[0])
    w.load_state_dict(ds.view().state_dict())
    assert w.affine is None
    # a state written before the argument existed leaves the view's own
    old = {k: x for k, x in sd.items() if k != "affine"}
    u = ds.view(affine=dict(degrees=3))
    u.load_state_dict(old)
    assert u.affine == D.affine_ranges(dict(degrees=3))
    # the state survives a checkpoint's serialisation
    import io
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    assert torch.load(buf)["affine"] == sd["affine"]


def test_descriptor_fields_without_a_gpu():
    """affine = NULL / affine_rows = 0 is today's descriptor; the entry points refuse a table
    that does not cover the batch before any HIP call."""
    import ctypes
    from torch_scae_amd import _lib
    lib = _lib.load()
    T = _lib.BatchSourceDesc
    assert T.affine.offset >= T.wrap.offset + 4 and T.affine_rows.offset == T.affine.offset + 8
    assert ctypes.sizeof(T) == T.affine_rows.offset + 8
    d = _dataset(10).view().desc(0, 0)
    assert not d.affine and d.affine_rows == 0

    def desc(**kw):
        d = T()
        d.images, d.labels, d.rows, d.n = 0x1000, 0x1000, 100, 100
        d.C, d.h, d.w, d.H, d.W, d.world = 1, 28, 28, 40, 40, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    fake = ctypes.c_void_p(0x1000)
    for bad in (dict(affine=0x1000, affine_rows=0), dict(affine=0x1000, affine_rows=99, position=96),
                dict(affine=0x1000, affine_rows=103, position=100, wrap=1),
                dict(affine=0x1000, affine_rows=99, position=92, rank=1, world=2),
                dict(affine_rows=100)):
        assert lib.scae_gather_batch_f32(fake, fake, 4, ctypes.byref(desc(**bad)), None) == -1, bad
        assert lib.scae_step_prologue_source_f32(fake, fake, 4, ctypes.byref(desc(**bad)), None,
                                                 0, None, None, None, None) == -1, bad
