"""``flip=``, ``max_shift=`` and ``interpolation="bilinear"`` views of a resident dataset on the
CPU path: a flipped position reads its example mirrored about the example itself (asymmetric
padding included), by ``flip_bits``; the coefficient mirror's integer identity; ``max_shift``
replaces the pads as the shift range and crops what leaves the frame; a degrees-0 bilinear view
is the nearest one bit for bit, and ``affine_warp(..., "bilinear")`` stays within a derived
bound of an fp64 bilinear with the real-valued matrix (and of ``grid_sample``); bad arguments
are refused; ``state_dict`` and ``factory.make_train_view`` carry the arguments; the
descriptor of a default view is today's, and the entry points refuse an unknown sampling mode
before any HIP call."""
import ctypes
import io

import numpy as np
import pytest
import torch

from torch_scae_amd import data as D

N, C, h, w, B = 21, 3, 6, 5, 4
SIZES = [(6, 5), (9, 8)]         # unpadded; pads (1, 1) with an odd W - w (right pad 2)
WARP = dict(degrees=30, scale=(0.7, 1.3), shear=10)


def _images(u8, seed=0):
    g = torch.Generator().manual_seed(seed)
    if u8:
        return torch.randint(0, 256, (N, C, h, w), generator=g, dtype=torch.uint8)
    return torch.rand(N, C, h, w, generator=g)


def _dataset(u8=True, out=(9, 8), images=None):
    labels = torch.arange(N) % 10
    return D.ResidentDataset(_images(u8) if images is None else images, labels, out_size=out,
                             device="cpu")


# -- 1. flip ------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [None, dict(degrees=0)])
@pytest.mark.parametrize("out", SIZES)
@pytest.mark.parametrize("u8", [True, False])
def test_flip_mirrors_the_example_where_flip_bits_says(u8, out, affine):
    seed = 3
    images = _images(u8)
    ds, mirrored = _dataset(u8, out, images), _dataset(u8, out, images.flip(-1))
    args = dict(shuffle=False, translate=False, seed=seed, affine=affine)
    plain = ds.view(**args).materialise()[0]
    want_flipped = mirrored.view(**args).materialise()[0]     # (mirrored about the example)
    got, labels = ds.view(flip=True, **args).materialise()
    bits = D.flip_bits(torch.arange(N), 0, seed)
    assert bits.dtype == torch.bool and 0 < int(bits.sum()) < N
    for p in range(N):
        assert torch.equal(got[p], want_flipped[p] if bits[p] else plain[p]), p
        assert not torch.equal(want_flipped[p], plain[p])
    assert torch.equal(labels, torch.arange(N) % 10)
    # another epoch: another draw of the bits
    assert not torch.equal(D.flip_bits(torch.arange(N), 1, seed), bits)


def test_flip_bits_is_word_two_of_the_shift_draw_and_keeps_the_unwrapped_position():
    seed, epoch = (5 << 32) + 77, (1 << 32) + 2
    p = torch.arange(64)
    c = D._philox([p, D._word(epoch, p), D._word(epoch >> 32, p), D._word(0x53484654, p)],
                  seed & 0xFFFFFFFF, seed >> 32, 10)
    assert torch.equal(D.flip_bits(p, epoch, seed), (c[2] >> 31) == 1)
    sh = D.translate_shifts(p, epoch, seed, (6, 4))
    assert torch.equal(sh[:, 0], D.shift_rule(c[0] >> 8, 6))
    # a wrapped position (drop_last=False) reads the row of p - n and flips by p itself
    ds = _dataset(True, (9, 8))
    v = ds.view(flip=True, translate=False, seed=9, world=2, rank=1, drop_last=False)
    spe, b = v.steps_per_epoch(B), v.remainder(B)
    pos = v.positions(spe, B)
    assert b == 3 and pos.tolist() == [19, 20, 21]
    got = v.batch(0, spe, B)[0]
    unflipped = ds.view(translate=False).materialise()[0]
    bits = D.flip_bits(pos, 0, 9)
    flipped = _dataset(True, (9, 8), _images(True).flip(-1)).view(translate=False) \
        .materialise()[0]
    for s, q in enumerate(pos.tolist()):
        row = q - N if q >= N else q
        assert torch.equal(got[s], (flipped if bits[s] else unflipped)[row]), q


def test_the_coefficient_mirror_is_the_integer_mirror():
    g = torch.Generator().manual_seed(0)
    K = torch.randint(-(1 << 40), 1 << 40, (100000,), generator=g)
    K = torch.cat([K, torch.tensor([0, -1, 1, 65535, 65536, -65536, -65537])])
    for pw, ww in ((0, 5), (1, 5), (6, 28), (0, 32)):
        a1 = 2 * pw + ww
        assert torch.equal((a1 - 1) - (K >> 16), (a1 * 65536 - 1 - K) >> 16)
    # as affine_coefficients composes it: rows with the bit set, x coefficients only
    p = torch.arange(200)
    args = (p, 1, 4, (1, 1), (9, 8), WARP)
    k = D.affine_coefficients(*args)
    kf = D.affine_coefficients(*args, flip=True, width=5)
    m = D.flip_bits(p, 1, 4)
    a1 = 2 * 1 + 5
    assert torch.equal(kf[~m], k[~m]) and torch.equal(kf[:, 3:], k[:, 3:])
    assert torch.equal(kf[m][:, 0], -k[m][:, 0]) and torch.equal(kf[m][:, 1], -k[m][:, 1])
    assert torch.equal(kf[m][:, 2], a1 * 65536 - 1 - k[m][:, 2])
    # the default width is W - 2 pad_w: right where W - w is even
    assert torch.equal(D.affine_coefficients(*args, flip=True),
                       D.affine_coefficients(*args, flip=True, width=6))


# -- 2. max_shift -------------------------------------------------------------------------------
def _place(images, out, shifts):
    """pad_and_translate's placement with cropping, pixel block by pixel block."""
    H, W = out
    ph, pw = (H - h) // 2, (W - w) // 2
    x = images.to(torch.float32)
    if images.dtype == torch.uint8:
        x = x / 255.0
    res = torch.zeros(images.shape[0], C, H, W)
    for n, (dy, dx) in enumerate(shifts.tolist()):
        top, left = ph + dy, pw + dx
        i0, i1, j0, j1 = max(top, 0), min(top + h, H), max(left, 0), min(left + w, W)
        if i0 < i1 and j0 < j1:
            res[n, :, i0:i1, j0:j1] = x[n, :, i0 - top:i1 - top, j0 - left:j1 - left]
    return res


@pytest.mark.parametrize("out", SIZES)
@pytest.mark.parametrize("u8", [True, False])
def test_max_shift_replaces_the_pads_and_crops(u8, out):
    ds = _dataset(u8, out)
    v = ds.view(shuffle=True, seed=6, max_shift=(2, 3))
    sh = D.translate_shifts(torch.arange(2000), 0, 6, (2, 3))
    assert torch.equal(v.rows_and_shifts(0, torch.arange(N))[1], sh[:N])
    assert sorted(set(sh[:, 0].tolist())) == [-2, -1, 0, 1, 2]
    assert sorted(set(sh[:, 1].tolist())) == [-3, -2, -1, 0, 1, 2, 3]
    cropped = 0
    for epoch in (0, 2):
        for step in range(v.steps_per_epoch(B)):
            rows, shifts = v.indices_and_shifts(epoch, step, B)
            got, labels = v.batch(epoch, step, B)
            assert torch.equal(got, _place(ds.images[rows], out, shifts)), (epoch, step)
            assert torch.equal(labels, ds.labels[rows])
            cropped += int((shifts.abs() > torch.tensor(ds.pads)).any(1).sum())
    assert cropped > 0
    # translate=False: no shift, whatever the range
    a = ds.view(translate=False, max_shift=(2, 3)).materialise()[0]
    assert torch.equal(a, ds.view(translate=False).materialise()[0])


def test_no_max_shift_is_todays_view_and_the_pads_as_range_give_its_bits():
    ds = _dataset(True, (9, 8))
    plain = ds.view(shuffle=True, seed=6)
    assert plain.max_shift is None and not plain.uses_table
    same = ds.view(shuffle=True, seed=6, max_shift=None)
    via_table = ds.view(shuffle=True, seed=6, max_shift=ds.pads)
    assert via_table.uses_table
    for epoch in (0, 1):
        for step in range(plain.steps_per_epoch(B)):
            want = D.pad_and_translate(
                ds.images[plain.indices_and_shifts(epoch, step, B)[0]], (9, 8),
                shifts=D.translate_shifts(plain.positions(step, B), epoch, 6, ds.pads))
            assert torch.equal(plain.batch(epoch, step, B)[0], want)
            assert torch.equal(same.batch(epoch, step, B)[0], want)
            assert torch.equal(via_table.batch(epoch, step, B)[0], want)


# -- 3. bilinear ----------------------------------------------------------------------------------
@pytest.mark.parametrize("out", SIZES)
@pytest.mark.parametrize("u8", [True, False])
def test_bilinear_at_zero_degrees_is_the_nearest_view_bit_for_bit(u8, out):
    ds = _dataset(u8, out)
    # (without flip: a mirrored position samples 2^-16 of a pixel beside the integer point)
    for extra in (dict(), dict(max_shift=(2, 3)), dict(affine=dict(degrees=0))):
        args = dict(shuffle=True, seed=8, drop_last=False, **extra)
        near, bil = ds.view(**args), ds.view(interpolation="bilinear", **args)
        for epoch in (0, 1):
            for step in range(near.steps_in_epoch(B)):
                assert torch.equal(bil.batch(epoch, step, B)[0], near.batch(epoch, step, B)[0])


def test_bilinear_is_the_rule_pixel_by_pixel():
    g = torch.Generator().manual_seed(4)
    k = torch.tensor([[60000, -30000, 123456, 25000, 70000, -200000],
                      [-65536, 0, 8 * 65536 - 1, 0, -65536, 9 * 65536 - 1],
                      [40000, 1000, -70000, -900, 32768, 65536 + 77]])
    H, W, ph, pw = 9, 8, 1, 1
    for u8 in (True, False):
        img = torch.randint(0, 256, (3, 2, h, w), generator=g, dtype=torch.uint8) if u8 \
            else torch.rand(3, 2, h, w, generator=g)
        got = D.affine_warp(img, k, (H, W), "bilinear")
        assert got.dtype == torch.float32
        f32 = np.float32

        def tap(n, c, y, x):
            inside = 0 <= y < h and 0 <= x < w
            return (int(img[n, c, y, x]) if u8 else f32(img[n, c, y, x])) if inside \
                else (0 if u8 else f32(0))
        for n in range(3):
            k0, k1, k2, k3, k4, k5 = k[n].tolist()
            for i in range(H):
                for j in range(W):
                    U, V = k2 + k1 * i + k0 * j - 32768, k5 + k4 * i + k3 * j - 32768
                    x0, fx, y0, fy = (U >> 16) - pw, (U >> 8) & 255, (V >> 16) - ph, (V >> 8) & 255
                    for c in range(2):
                        t = [tap(n, c, y0, x0), tap(n, c, y0, x0 + 1),
                             tap(n, c, y0 + 1, x0), tap(n, c, y0 + 1, x0 + 1)]
                        if u8:
                            acc = (256 - fy) * ((256 - fx) * t[0] + fx * t[1]) + \
                                fy * ((256 - fx) * t[2] + fx * t[3])
                            want = f32(acc) / f32(16711680.0)
                        else:
                            wx1, wx0 = f32(fx) / f32(256), f32(256 - fx) / f32(256)
                            wy1, wy0 = f32(fy) / f32(256), f32(256 - fy) / f32(256)
                            top = f32(f32(wx0 * t[0]) + f32(wx1 * t[1]))
                            bot = f32(f32(wx0 * t[2]) + f32(wx1 * t[3]))
                            want = f32(f32(wy0 * top) + f32(wy1 * bot))
                        assert got[n, c, i, j].item() == float(want), (u8, n, c, i, j)
    with pytest.raises(ValueError):
        D.affine_warp(img, k, (H, W), "bicubic")


def _real_matrices(p, epoch, seed, pads, size, rng, shift_lim):
    """Each position's inverse map as real numbers (fp64), from the definition's text."""
    H, W = size
    pt = torch.as_tensor(p)
    c = D._philox([pt, D._word(epoch, pt), D._word(epoch >> 32, pt), D._word(0x4146464E, pt)],
                  seed & 0xFFFFFFFF, seed >> 32, 10)
    a = D.affine_ranges(rng)
    spans = (a["degrees"], a["scale"], a["shear"][:2], a["shear"][2:])
    val = [lo + (hi - lo) * (wd >> 8).numpy().astype(np.float64) / 2 ** 24
           for wd, (lo, hi) in zip(c, spans)]
    rot, scale, sx, sy = np.radians(val[0]), val[1], np.radians(val[2]), np.radians(val[3])
    sh = D.translate_shifts(pt, epoch, seed, shift_lim).numpy().astype(np.float64)
    ty, tx = sh[:, 0], sh[:, 1]
    cx, cy = W * 0.5, H * 0.5
    ma = np.cos(rot - sy) / np.cos(sy)
    mb = -np.cos(rot - sy) * np.tan(sx) / np.cos(sy) - np.sin(rot)
    mc = np.sin(rot - sy) / np.cos(sy)
    md = -np.sin(rot - sy) * np.tan(sx) / np.cos(sy) + np.cos(rot)
    M = np.stack([md, -mb, 0 * md, -mc, ma, 0 * md], 1) / scale[:, None]
    M[:, 2] = M[:, 0] * (-cx - tx) + M[:, 1] * (-cy - ty) + cx
    M[:, 5] = M[:, 3] * (-cx - tx) + M[:, 4] * (-cy - ty) + cy
    return M


def _bilinear_fp64(padded, M):
    """fp64 bilinear of zero-padded images (n, C, H, W) through real-valued inverse maps: output
    pixel (i, j) has its centre at (j + 0.5, i + 0.5); real weights; taps outside are zero."""
    n, Cn, H, W = padded.shape
    ii, jj = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    out = np.zeros((n, Cn, H, W))
    for b in range(n):
        u = M[b, 0] * jj + M[b, 1] * ii + M[b, 2] - 0.5       # pixel-index coordinates
        v = M[b, 3] * jj + M[b, 4] * ii + M[b, 5] - 0.5
        x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
        fx, fy = u - x0, v - y0

        def tap(y, x):
            inside = (y >= 0) & (y < H) & (x >= 0) & (x < W)
            return padded[b][:, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)] * inside
        out[b] = (1 - fy) * ((1 - fx) * tap(y0, x0) + fx * tap(y0, x0 + 1)) + \
            fy * ((1 - fx) * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1))
    return out


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("out", SIZES)
@pytest.mark.parametrize("u8", [True, False])
def test_bilinear_stays_within_the_derived_bound_of_an_fp64_bilinear(u8, out, flip):
    """The interpolant of values in [0, 1] is 1-Lipschitz per axis; the 8-bit weights truncate
    each coordinate by < 2^-8; FIX moves each of a coordinate's three coefficients by <= 2^-17,
    the coordinate by <= 2^-17 (H + W) per axis; the mirror adds 2^-16:
    |err| <= 2^-7 + (H + W + 1) 2^-15, plus 2^-20 against fp32 grid_sample."""
    H, W = out
    seed, epoch = 12, 1
    ds = _dataset(u8, out)
    v = ds.view(seed=seed, affine=WARP, flip=flip, max_shift=(1, 2),
                interpolation="bilinear")
    got = v.materialise(epoch)[0].numpy().astype(np.float64)
    p = torch.arange(N)
    M = _real_matrices(p, epoch, seed, ds.pads, out, WARP, (1, 2))
    images = ds.images.clone()
    bits = D.flip_bits(p, epoch, seed) if flip else torch.zeros(N, dtype=torch.bool)
    images[bits] = images[bits].flip(-1)
    padded = D.pad_and_translate(images, out, shifts=torch.zeros(N, 2, dtype=torch.int64))
    want = _bilinear_fp64(padded.numpy().astype(np.float64), M)
    bound = 2.0 ** -7 + (H + W + 1) * 2.0 ** -15
    err = np.abs(got - want).max()
    print(f"bilinear vs fp64: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    # (the test is not vacuous: the nearest form is far outside the bound)
    near = ds.view(seed=seed, affine=WARP, flip=flip, max_shift=(1, 2)).materialise(epoch)[0]
    assert np.abs(near.numpy() - want).max() > 10 * bound
    try:
        from torch.nn.functional import grid_sample
    except ImportError:
        return
    ii, jj = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    Mt = torch.from_numpy(M).view(N, 6, 1, 1)
    u = Mt[:, 0] * jj + Mt[:, 1] * ii + Mt[:, 2]              # pixel-edge coordinates in [0, W]
    vv = Mt[:, 3] * jj + Mt[:, 4] * ii + Mt[:, 5]
    grid = torch.stack([2 * u / W - 1, 2 * vv / H - 1], -1).to(torch.float32)
    gs = grid_sample(padded, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    err = float((torch.from_numpy(got) - gs.to(torch.float64)).abs().max())
    print(f"bilinear vs grid_sample: max err {err:.3e}")
    assert err <= bound + 2.0 ** -20


# -- 4. arguments ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [
    dict(flip=1), dict(flip=None), dict(flip="yes"),
    dict(max_shift=(-1, 2)), dict(max_shift=(1.0, 2)), dict(max_shift=3), dict(max_shift=(1, 2, 3)),
    dict(max_shift=(True, 1)), dict(max_shift="ab"),
    dict(interpolation="bicubic"), dict(interpolation=None), dict(interpolation="BILINEAR"),
    dict(affine=dict(degrees=5, interpolation="bilinear")),
])
def test_bad_arguments_are_refused(bad):
    ds = _dataset()
    with pytest.raises(ValueError):
        ds.view(**bad)
    with pytest.raises(ValueError):
        ds.split([N - 5, 5], **bad)


def test_bad_arguments_of_the_functions_are_refused():
    args = (torch.arange(4), 0, 0, (1, 1), (9, 8), dict(degrees=0))
    with pytest.raises(ValueError):
        D.affine_coefficients(*args, flip=1)
    with pytest.raises(ValueError):
        D.affine_coefficients(*args, max_shift=(-1, 0))
    assert D.affine_coefficients(*args, max_shift=[0, 2]).shape == (4, 6)


def test_state_dict_carries_the_arguments():
    ds = _dataset()
    v = ds.view(shuffle=True, seed=5, flip=True, max_shift=(2, 3), interpolation="bilinear",
                affine=WARP, drop_last=False)
    for _ in range(7):
        v.take_step(B)
    sd = v.state_dict()
    assert (sd["flip"], sd["max_shift"], sd["interpolation"]) == (True, [2, 3], "bilinear")
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    loaded = torch.load(buf)
    assert loaded == sd
    u = ds.view()
    assert (u.flip, u.max_shift, u.interpolation) == (False, None, "nearest")
    plain_sd = u.state_dict()
    assert (plain_sd["flip"], plain_sd["max_shift"], plain_sd["interpolation"]) == \
        (False, None, "nearest")
    u.load_state_dict(loaded)
    assert (u.flip, u.max_shift, u.interpolation) == (True, (2, 3), "bilinear")
    assert (u.epoch, u.cursor) == (v.epoch, v.cursor)
    assert torch.equal(u.batch(1, 2, B)[0], v.batch(1, 2, B)[0])
    u.load_state_dict(plain_sd)
    assert (u.flip, u.max_shift, u.interpolation) == (False, None, "nearest")
    # a state written before the arguments existed: today's behaviour on a view built without them
    old = {k: x for k, x in plain_sd.items() if k not in ("flip", "max_shift", "interpolation")}
    t = ds.view(shuffle=True, seed=5)
    t.load_state_dict(old)
    assert (t.flip, t.max_shift, t.interpolation) == (False, None, "nearest")
    assert not t.uses_table
    assert torch.equal(t.batch(0, 1, B)[0], ds.view().batch(0, 1, B)[0])   # (u's order, seed)
    with pytest.raises(ValueError):
        t.load_state_dict(dict(sd, interpolation="cubic"))


def test_the_table_is_rebuilt_when_an_option_changes():
    ds = _dataset()
    v = ds.view(seed=2, flip=True)
    t0 = v._affine_table(0)
    assert v._affine_table(0) is t0 and tuple(t0.shape) == (N, 6) and t0.dtype == torch.int32
    assert torch.equal(t0.to(torch.int64), v.coefficients(0, torch.arange(N)))
    v.max_shift = (0, 2)
    t1 = v._affine_table(0)
    assert t1 is not t0 and torch.equal(t1.to(torch.int64), v.coefficients(0, torch.arange(N)))
    v.flip = False
    assert v._affine_table(0) is not t1
    v.interpolation = "bilinear"
    assert len(v._tables) == 2


def test_make_train_view_reads_the_config():
    from torch_scae_amd import factory
    ds = _dataset()
    v = factory.make_train_view(ds, dict(seed=7))
    assert isinstance(v, D.DatasetView) and v.shuffle and v.translate and v.seed == 7
    assert v.affine is None and not v.uses_table and v.drop_last
    assert factory.make_train_view(ds, dict(dataset=dict(name="mnist"))).seed == 0
    full = dict(translate=True, max_shift=[2, 3], flip=True, affine=dict(degrees=15),
                interpolation="bilinear")
    v = factory.make_train_view(ds, dict(seed=1, dataset=dict(augment=full)), rank=1, world=2,
                                drop_last=False)
    assert (v.flip, v.max_shift, v.interpolation) == (True, (2, 3), "bilinear")
    assert v.affine == D.affine_ranges(dict(degrees=15)) and v.shuffle and v.seed == 1
    assert (v.rank, v.world, v.drop_last) == (1, 2, False)
    want = ds.view(shuffle=True, seed=1, rank=1, world=2, drop_last=False, **full)
    assert torch.equal(v.batch(0, 1, B)[0], want.batch(0, 1, B)[0])
    v = factory.make_train_view(ds, dict(dataset=dict(augment=dict(translate=False))))
    assert not v.translate and v.shuffle
    assert not factory.make_train_view(ds, dict(seed=3), shuffle=False).shuffle
    for bad in (dict(colour_jitter=0.1), dict(flip=True, degrees=5), "flip"):
        with pytest.raises(ValueError):
            factory.make_train_view(ds, dict(dataset=dict(augment=bad)))


# -- 5. the descriptor ------------------------------------------------------------------------------
def test_descriptor_of_a_default_view_is_todays_and_the_mode_rides_in_translate():
    from torch_scae_amd import _lib
    lib = _lib.load()
    T = _lib.BatchSourceDesc
    assert ctypes.sizeof(T) == T.affine_rows.offset + 8 == 136
    ds = _dataset(True, (9, 8))
    v = ds.view(shuffle=True, seed=(3 << 32) + 1, rank=1, world=2, drop_last=False)
    want = T()
    want.images, want.labels, want.index = ds.images.data_ptr(), ds.labels.data_ptr(), None
    want.rows = want.n = N
    want.image_u8, want.label_u8 = 1, 0
    want.C, want.h, want.w, want.H, want.W = C, h, w, 9, 8
    want.shuffle, want.translate = 1, 1
    want.seed, want.epoch, want.position = (3 << 32) + 1, 5, 8
    want.rank, want.world, want.wrap = 1, 2, 1
    want.affine, want.affine_rows = None, 0
    assert bytes(v.desc(5, 8)) == bytes(want)
    assert ds.view(translate=False).desc(0, 0).translate == 0
    # nearest table views keep the word as it was; a bilinear view says 2 and has a table
    for extra in (dict(flip=True), dict(max_shift=(2, 2)), dict(affine=dict(degrees=5))):
        for translate in (False, True):
            d = ds.view(translate=translate, **extra).desc(0, 0)
            assert d.translate == int(translate) and d.affine and d.affine_rows == N
    for translate in (False, True):
        d = ds.view(translate=translate, interpolation="bilinear").desc(0, 0)
        assert d.translate == 2 and d.affine and d.affine_rows == N

    def desc(**kw):
        d = T()
        d.images, d.labels, d.rows, d.n = 0x1000, 0x1000, 100, 100
        d.C, d.h, d.w, d.H, d.W, d.world = 1, 28, 28, 40, 40, 1
        for k, x in kw.items():
            setattr(d, k, x)
        return d
    fake = ctypes.c_void_p(0x1000)
    for bad in (dict(translate=2), dict(translate=3), dict(translate=-1),
                dict(translate=3, affine=0x1000, affine_rows=100),
                dict(translate=-1, affine=0x1000, affine_rows=100)):
        assert lib.scae_gather_batch_f32(fake, fake, 4, ctypes.byref(desc(**bad)), None) == -1, bad
        assert lib.scae_step_prologue_source_f32(fake, fake, 4, ctypes.byref(desc(**bad)), None,
                                                 0, None, None, None, None) == -1, bad
