"""Input formats either side of the hot path.

``pad_and_translate`` is the MNIST training transform of the reference
(torch_scae_experiments/mnist/experiment.py:23-40): 28x28 digits are
zero-padded to the model's 40x40 input and shifted by a random whole number of
pixels of at most the padding in each direction
(``Pad(6)`` + ``RandomAffine(degrees=0, translate=(6/40, 6/40))`` + ``ToTensor``)
-- done here for a whole batch on the device instead of per sample on the
host.

``stroke_batches`` is a structured synthetic stand-in for MNIST where no
dataset can be fetched: ten glyph classes, each a fixed set of pen strokes,
rendered under a random affine warp per sample -- images with parts that recur
under pose changes, which is what the part capsules model.  (U[0,1) noise
images have no such structure: trained on them the capsules switch off within
a few hundred steps)

``ResidentDataset`` holds a dataset in device memory once; its views
(``split`` / ``view``) are the reference's loaders and ``random_split``
(torch_scae_experiments/base_experiment.py:79-93, mnist/experiment.py:23-55)
with the transform applied on the device: a training step gathers its batch
in its prologue launch (csrc/batch_source_dev.h, ``TrainStep.step_from``).
Every view also has a CPU path that computes the same order and shifts in
integer torch ops.  A view's ``affine=`` adds the transform's other arguments
(``degrees``, ``scale``, ``shear``) with nearest-neighbour resampling:
``affine_coefficients`` draws them and builds each position's fixed-point
inverse map on the host, ``affine_warp`` is the CPU path of the sampling.  ``flip=`` and
``max_shift=`` (RandomHorizontalFlip; a shift range other than the pads, as RandomCrop with
padding) are composed into the same maps, and ``interpolation="bilinear"`` samples them with
four taps and 8-bit weights."""
import gzip
import math

import torch


def pad_and_translate(images, out_size=(40, 40), generator=None, shifts=None):
    """images (B, C, h, w) uint8 or float -> (B, C, H, W) float32 in [0, 1].

    ``shifts`` (B, 2) integer (dy, dx) overrides the random draw; otherwise
    each is round(U(-pad, pad)) like torchvision's RandomAffine.get_params
    with the padding of that axis as the maximal shift."""
    B, C, h, w = images.shape
    H, W = out_size
    if H < h or W < w:
        raise ValueError("output smaller than the images")
    x = images.to(torch.float32)
    if not images.dtype.is_floating_point:
        x = x / 255.0                         # ToTensor
    ph, pw = (H - h) // 2, (W - w) // 2
    if shifts is None:
        u = torch.rand(B, 2, generator=generator, device="cpu")
        lim = torch.tensor([ph, pw], dtype=torch.float32)
        shifts = torch.round((u * 2 - 1) * lim).to(torch.int64)
    shifts = shifts.to(images.device)
    # out[b, :, i, j] = x[b, :, i - top_b, j - left_b] where that exists
    top = (ph + shifts[:, 0]).view(B, 1, 1)
    left = (pw + shifts[:, 1]).view(B, 1, 1)
    ii = torch.arange(H, device=images.device).view(1, H, 1) - top   # (B,H,1)
    jj = torch.arange(W, device=images.device).view(1, 1, W) - left  # (B,1,W)
    valid = (ii >= 0) & (ii < h) & (jj >= 0) & (jj < w)              # (B,H,W)
    flat = ii.clamp(0, h - 1) * w + jj.clamp(0, w - 1)                # (B,H,W)
    out = torch.gather(x.reshape(B, C, h * w), 2,
                       flat.view(B, 1, H * W).expand(B, C, H * W))
    return (out.view(B, C, H, W) * valid.unsqueeze(1)).contiguous()


def stroke_batches(n_batches, batch, image_shape, seed=0, device="cpu",
                   n_classes=10, strokes=4, glyph_seed=None):
    """-> (images (n_batches, B, C, H, W) float32 in [0, 1], labels
    (n_batches, B) int64).  Class c is a fixed glyph of ``strokes`` line
    segments (drawn once from ``seed``, or from ``glyph_seed`` when given: a
    held-out set is the same ``glyph_seed`` under another ``seed``); a sample is its glyph under a random
    rotation (+-25 degrees), scale (0.75 .. 1.1), shear and translation
    (+-0.2), drawn with a soft pen (Gaussian profile, sigma 0.07 of the half
    image) -- evaluated analytically per pixel on ``device``."""
    C, H, W = image_shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    # glyphs: endpoints in [-0.75, 0.75]^2, consecutive strokes share an endpoint
    gg = g if glyph_seed is None else torch.Generator(device="cpu").manual_seed(glyph_seed)
    pts = torch.rand(n_classes, strokes + 1, 2, generator=gg) * 1.5 - 0.75
    N = n_batches * batch
    labels = torch.randint(0, n_classes, (N,), generator=g)
    ang = (torch.rand(N, generator=g) * 2 - 1) * math.radians(25.0)
    scale = 0.75 + 0.35 * torch.rand(N, generator=g)
    shear = (torch.rand(N, generator=g) * 2 - 1) * 0.2
    shift = (torch.rand(N, 2, generator=g) * 2 - 1) * 0.2
    colour = 0.6 + 0.4 * torch.rand(N, C, generator=g)
    cos, sin = torch.cos(ang) * scale, torch.sin(ang) * scale
    A = torch.stack([torch.stack([cos, -sin + shear * cos], -1),
                     torch.stack([sin, cos + shear * sin], -1)], -2)   # (N,2,2)
    P = torch.einsum("nij,nkj->nki", A, pts[labels]) + shift[:, None, :]
    P, colour = P.to(device), colour.to(device)
    ys = (2 * torch.arange(H, device=device, dtype=torch.float32) + 1) / H - 1
    xs = (2 * torch.arange(W, device=device, dtype=torch.float32) + 1) / W - 1
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    q = torch.stack([gx, gy], -1).view(1, 1, H * W, 2)         # pixel centres
    a, b = P[:, :-1, None, :], P[:, 1:, None, :]               # (N,S,1,2)
    ab = b - a
    t = ((q - a) * ab).sum(-1) / (ab * ab).sum(-1).clamp_min(1e-8)
    d2 = ((q - (a + t.clamp(0, 1).unsqueeze(-1) * ab)) ** 2).sum(-1)  # (N,S,HW)
    ink = torch.exp(-d2.amin(1) / (2 * 0.07 ** 2)).view(N, 1, H, W)
    images = (ink * colour.view(N, C, 1, 1)).clamp(0, 1)
    return (images.view(n_batches, batch, C, H, W).contiguous(),
            labels.view(n_batches, batch).to(device))


# -- device-resident datasets ---------------------------------------------------------------
# The draws of csrc/batch_source_dev.h in integer torch ops (int64 tensors holding uint32
# values): Philox4x32 with the device generator's constants and key schedule (noise_dev.h).
_M32 = 0xFFFFFFFF
_TAG_PERM, _TAG_SHIFT, _TAG_AFFINE = 0x5045524D, 0x53484654, 0x4146464E
_FEISTEL_ROUNDS, _F_PHILOX_ROUNDS, _KEY_PHILOX_ROUNDS = 4, 3, 10


def _mulhilo(a, m):
    """(hi, lo) 32-bit words of a * m (a: uint32 values, m: a uint32 constant), in 16-bit
    limbs so that no int64 product overflows."""
    pl, ph = a * (m & 0xFFFF), a * (m >> 16)
    s = (pl & _M32) + ((ph & 0xFFFF) << 16)
    return ((pl >> 32) + (ph >> 16) + (s >> 32)) & _M32, s & _M32


def _philox(c, k0, k1, rounds):
    c = list(c)
    for _ in range(rounds):
        hi0, lo0 = _mulhilo(c[0], 0xD2511F53)
        hi1, lo1 = _mulhilo(c[2], 0xCD9E8D57)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c


def _word(v, like):
    return torch.full_like(like, v & _M32)


def _round_keys(seed, epoch):
    r = torch.arange(_FEISTEL_ROUNDS, dtype=torch.int64)
    c = _philox([r, _word(epoch, r), _word(epoch >> 32, r), _word(_TAG_PERM, r)],
                seed & _M32, (seed >> 32) & _M32, _KEY_PHILOX_ROUNDS)
    return list(zip(c[0].tolist(), c[1].tolist()))


def feistel_order(positions, n, seed, epoch):
    """View rows of epoch positions (int64 tensor, values in [0, n)) under the shuffled
    order: a keyed pseudo-random permutation of [0, n) -- a 4-round Feistel network over the
    smallest even bit width k with 2^k >= n, round keys drawn by Philox from (seed, epoch,
    round), cycle-walked into [0, n).  Not a uniform draw over all n! orders."""
    x = positions.to(torch.int64).clone()
    if n <= 1:
        return x
    k = 0
    while (1 << k) < n:
        k += 2
    h, m = k // 2, (1 << (k // 2)) - 1
    keys = _round_keys(seed, epoch)
    todo = torch.ones_like(x, dtype=torch.bool)
    while bool(todo.any()):
        v = x[todo]
        L, R = v >> h, v & m
        zero = torch.zeros_like(R)
        for k0, k1 in keys:
            f = _philox([R, zero, zero, zero], k0, k1, _F_PHILOX_ROUNDS)[0]
            L, R = R, L ^ (f & m)
        x[todo] = (L << h) | R
        todo = x >= n
    return x


def shift_rule(r24, pad):
    """round-half-to-even(2 pad r / 2^24 - pad) of 24-bit uniforms r, exactly in integers
    (torchvision's RandomAffine translation: round(U(-pad, pad)))."""
    num = 2 * pad * r24.to(torch.int64)
    f, rem = (num >> 24) - pad, num & 0xFFFFFF
    half = 0x800000
    return torch.where(rem > half, f + 1, torch.where(rem < half, f, f + (f & 1)))


def translate_shifts(positions, epoch, seed, pads):
    """(len, 2) int64 (dy, dx) of epoch positions: two 24-bit uniforms of one Philox draw
    keyed by ``seed`` at counter (position, epoch, tag); ``pads`` = (pad_h, pad_w)."""
    p = positions.to(torch.int64)
    c = _philox([p & _M32, _word(epoch, p), _word(epoch >> 32, p), _word(_TAG_SHIFT, p)],
                seed & _M32, (seed >> 32) & _M32, _KEY_PHILOX_ROUNDS)
    return torch.stack([shift_rule(c[0] >> 8, pads[0]), shift_rule(c[1] >> 8, pads[1])], 1)


def flip_bits(positions, epoch, seed):
    """(len,) bool of epoch positions: True where ``flip=True`` mirrors the example
    (RandomHorizontalFlip, p = 0.5) -- the top bit of word 2 of the Philox draw whose words 0
    and 1 give the shifts (``translate_shifts``: counter (position, epoch, TAG_SHIFT), key =
    ``seed``)."""
    p = torch.as_tensor(positions).to(torch.int64)
    c = _philox([p & _M32, _word(epoch, p), _word(epoch >> 32, p), _word(_TAG_SHIFT, p)],
                seed & _M32, (seed >> 32) & _M32, _KEY_PHILOX_ROUNDS)
    return (c[2] >> 31) == 1


def shift_ranges(max_shift):
    """``max_shift``: None, or (sy, sx) non-negative ints -- validated; -> None or (sy, sx).
    ValueError on anything else."""
    if max_shift is None:
        return None
    try:
        sy, sx = max_shift
    except (TypeError, ValueError):
        raise ValueError(f"max_shift: (sy, sx) expected, got {max_shift!r}") from None
    for v in (sy, sx):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"max_shift: non-negative ints expected, got {max_shift!r}")
    return sy, sx


INTERPOLATIONS = ("nearest", "bilinear")
_IDENTITY = {"degrees": 0.0}     # (the table route of a view without ``affine``)


def _range(v, name, symmetric=False):
    """(lo, hi) floats of a range argument; a number d means (-d, d) where ``symmetric``."""
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        if not symmetric:
            raise ValueError(f"{name}: a (lo, hi) pair expected, got {v!r}")
        if v < 0:
            raise ValueError(f"{name}: a single number must be non-negative, got {v!r}")
        v = (-v, v)
    try:
        lo, hi = (float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: a (lo, hi) pair expected, got {v!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"{name}: finite lo <= hi expected, got {v!r}")
    return lo, hi


def affine_ranges(affine):
    """``affine = dict(degrees=d | (lo, hi), scale=(lo, hi) | None, shear=s | (lo, hi) |
    (xlo, xhi, ylo, yhi) | None)`` -- torchvision's RandomAffine arguments; a number d means
    (-d, d), a missing scale 1, a missing shear 0 -- validated and normalised to
    ``dict(degrees=(lo, hi), scale=(lo, hi), shear=(xlo, xhi, ylo, yhi))`` of floats.
    None stays None.  ValueError on anything else."""
    if affine is None:
        return None
    if not isinstance(affine, dict) or set(affine) - {"degrees", "scale", "shear"}:
        raise ValueError(f"affine: a dict of degrees / scale / shear expected, got {affine!r}")
    deg = _range(affine.get("degrees", 0.0), "degrees", symmetric=True)
    scale = affine.get("scale")
    scale = (1.0, 1.0) if scale is None else _range(scale, "scale")
    if scale[0] <= 0:
        raise ValueError(f"scale: positive values expected, got {scale!r}")
    shear = affine.get("shear")
    if shear is None:
        shear = (0.0, 0.0, 0.0, 0.0)
    elif isinstance(shear, (int, float)) or len(shear) == 2:
        shear = _range(shear, "shear", symmetric=True) + (0.0, 0.0)
    elif len(shear) == 4:
        shear = _range(shear[:2], "shear") + _range(shear[2:], "shear")
    else:
        raise ValueError(f"shear: 1, 2 or 4 values expected, got {shear!r}")
    return {"degrees": deg, "scale": scale, "shear": shear}


def affine_coefficients(positions, epoch, seed, pads, size, affine, translate=True, *,
                        max_shift=None, flip=False, width=None):
    """(len, 6) int64 k0..k5 of epoch positions: each position's inverse affine map in 16.16
    fixed point, as Pillow's nearest-neighbour AFFINE path holds it (include/scae_hip.h,
    scae_batch_source_desc, has the definition).  One Philox draw keyed by ``seed`` at
    counter (position, epoch, TAG_AFFINE) gives 24-bit r for angle, scale, shear-x and
    shear-y, value = lo + (hi - lo) r / 2^24 in the ranges of ``affine`` (``affine_ranges``
    form or its input); the translation is ``translate_shifts`` of the same position
    (``translate``; else none) on the padded image of ``size`` = (H, W); the matrix is
    torchvision's ``_get_inverse_affine_matrix`` about (W / 2, H / 2) in fp64 and
    FIX(v) = floor(v 65536 + 0.5).  Every value is a function of (seed, epoch, position)
    alone.  ValueError where a coefficient leaves int32 (a scale too small, a shear too
    close to 90 degrees).

    ``max_shift`` = (sy, sx) replaces the pads as the translation's range (``shift_ranges``;
    None: the pads).  ``flip``: positions whose ``flip_bits`` is set read the example mirrored
    left to right -- composed into the map after FIX: with A1 = 2 pad_w + w (``width`` = w,
    the example's width; default W - 2 pad_w, right where W - w is even),
    k0' = -k0, k1' = -k1, k2' = 65536 A1 - 1 - k2, since for every integer K
    (A1 - 1) - (K >> 16) == (65536 A1 - 1 - K) >> 16: exactly the mirrored column for the
    nearest form, and the mirrored point less 2^-16 of a pixel for the bilinear one."""
    a = affine_ranges(affine)
    max_shift = shift_ranges(max_shift)
    if not isinstance(flip, bool):
        raise ValueError(f"flip: a bool expected, got {flip!r}")
    p = torch.as_tensor(positions, dtype=torch.int64)
    H, W = size
    c = _philox([p & _M32, _word(epoch, p), _word(epoch >> 32, p), _word(_TAG_AFFINE, p)],
                seed & _M32, (seed >> 32) & _M32, _KEY_PHILOX_ROUNDS)

    def value(word, lo, hi):
        return lo + (hi - lo) * (word >> 8).to(torch.float64) / float(1 << 24)
    rad = math.pi / 180.0                     # (math.radians' factor)
    rot = value(c[0], *a["degrees"]) * rad
    scale = value(c[1], *a["scale"])
    sx = value(c[2], *a["shear"][:2]) * rad
    sy = value(c[3], *a["shear"][2:]) * rad
    shifts = translate_shifts(p, epoch, seed, pads if max_shift is None else max_shift) \
        if translate else torch.zeros(p.numel(), 2, dtype=torch.int64)
    ty, tx = shifts[:, 0].to(torch.float64), shifts[:, 1].to(torch.float64)
    cx, cy = W * 0.5, H * 0.5
    ma = torch.cos(rot - sy) / torch.cos(sy)
    mb = -torch.cos(rot - sy) * torch.tan(sx) / torch.cos(sy) - torch.sin(rot)
    mc = torch.sin(rot - sy) / torch.cos(sy)
    md = -torch.sin(rot - sy) * torch.tan(sx) / torch.cos(sy) + torch.cos(rot)
    m0, m1, m3, m4 = md / scale, -mb / scale, -mc / scale, ma / scale
    m2 = m0 * (-cx - tx) + m1 * (-cy - ty) + cx
    m5 = m3 * (-cx - tx) + m4 * (-cy - ty) + cy
    k = torch.stack([m0, m1, m2 + m0 * 0.5 + m1 * 0.5, m3, m4, m5 + m3 * 0.5 + m4 * 0.5], 1)
    k = torch.floor(k * 65536.0 + 0.5)
    if flip:
        a1 = float(2 * pads[1] + (W - 2 * pads[1] if width is None else int(width)))
        m = flip_bits(p, epoch, seed)
        k[:, 0] = torch.where(m, -k[:, 0], k[:, 0])
        k[:, 1] = torch.where(m, -k[:, 1], k[:, 1])
        k[:, 2] = torch.where(m, a1 * 65536.0 - 1.0 - k[:, 2], k[:, 2])
    if not bool((torch.isfinite(k) & (k.abs() < float(1 << 31))).all()):
        raise ValueError("affine: a coefficient does not fit 16.16 fixed point in int32 "
                         "(scale too small or shear too close to 90 degrees)")
    return k.to(torch.int64)


def _affine_warp_bilinear(images, k, out_size):
    """``affine_warp``'s bilinear form (k: (B, 6, 1, 1) int64)."""
    B, C, h, w = images.shape
    H, W = out_size
    ph, pw = (H - h) // 2, (W - w) // 2
    i = torch.arange(H, device=images.device).view(1, H, 1)
    j = torch.arange(W, device=images.device).view(1, 1, W)
    U = k[:, 2] + k[:, 1] * i + k[:, 0] * j - 32768                     # (B,H,W)
    V = k[:, 5] + k[:, 4] * i + k[:, 3] * j - 32768
    x0, fx = (U >> 16) - pw, (U >> 8) & 255
    y0, fy = (V >> 16) - ph, (V >> 8) & 255
    u8 = not images.dtype.is_floating_point
    src = (images.to(torch.int64) if u8 else images.to(torch.float32)).reshape(B, C, h * w)

    def tap(y, x):
        valid = (y >= 0) & (y < h) & (x >= 0) & (x < w)
        flat = y.clamp(0, h - 1) * w + x.clamp(0, w - 1)
        t = torch.gather(src, 2, flat.view(B, 1, H * W).expand(B, C, H * W))
        return t.view(B, C, H, W) * valid.unsqueeze(1)
    t00, t01, t10, t11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    fx, fy = fx.unsqueeze(1), fy.unsqueeze(1)
    if u8:      # an integer < 2^24: exact in fp32, then one correctly rounded division
        acc = (256 - fy) * ((256 - fx) * t00 + fx * t01) + fy * ((256 - fx) * t10 + fx * t11)
        return (acc.to(torch.float32) / 16711680.0).contiguous()        # 255 * 65536
    wx1, wx0 = fx.to(torch.float32) / 256.0, (256 - fx).to(torch.float32) / 256.0
    wy1, wy0 = fy.to(torch.float32) / 256.0, (256 - fy).to(torch.float32) / 256.0
    top, bot = wx0 * t00 + wx1 * t01, wx0 * t10 + wx1 * t11   # (each op rounds on its own)
    return (wy0 * top + wy1 * bot).contiguous()


def affine_warp(images, coeffs, out_size, interpolation="nearest"):
    """images (B, C, h, w) uint8 or float, ``coeffs`` (B, 6) integer k0..k5
    (``affine_coefficients``) -> (B, C, H, W) float32: the example, zero-padded to
    ``out_size`` = (H, W), resampled through its inverse map with nearest-neighbour sampling
    in pure integers -- pixel (i, j) reads padded-image pixel (yin, xin) =
    ((k5 + k4 i + k3 j) >> 16, (k2 + k1 i + k0 j) >> 16), zero outside the example --
    then ToTensor's division for uint8.  The CPU path of the device gather's affine form.

    ``interpolation="bilinear"``: the four taps around the same fixed-point point moved half
    a pixel back, U = k2 + k1 i + k0 j - 32768 (x0 = (U >> 16) - pad_w, fx = (U >> 8) & 255;
    V, y0, fy likewise), a tap outside the example 0, weighted with the 8-bit fractions:
    uint8 data as an integer sum divided once by 255 * 65536, fp32 data with the exact weights
    n / 256 and every product and sum rounded to fp32 on its own (include/scae_hip.h has the
    rule) -- the device form's bits, and at integer coordinates the nearest form's.  Not
    Pillow's bilinear, which computes in fp64 per pixel and treats edges differently."""
    B, C, h, w = images.shape
    H, W = out_size
    if H < h or W < w:
        raise ValueError("output smaller than the images")
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f"interpolation: one of {INTERPOLATIONS} expected, "
                         f"got {interpolation!r}")
    k = torch.as_tensor(coeffs).to(images.device, torch.int64)
    if tuple(k.shape) != (B, 6):
        raise ValueError(f"coeffs ({B}, 6) expected, got {tuple(k.shape)}")
    if interpolation == "bilinear":
        return _affine_warp_bilinear(images, k.view(B, 6, 1, 1), out_size)
    x = images.to(torch.float32)
    if not images.dtype.is_floating_point:
        x = x / 255.0                         # ToTensor
    ph, pw = (H - h) // 2, (W - w) // 2
    k = k.view(B, 6, 1, 1)
    i = torch.arange(H, device=images.device).view(1, H, 1)
    j = torch.arange(W, device=images.device).view(1, 1, W)
    jj = ((k[:, 2] + k[:, 1] * i + k[:, 0] * j) >> 16) - pw            # (B,H,W)
    ii = ((k[:, 5] + k[:, 4] * i + k[:, 3] * j) >> 16) - ph
    valid = (ii >= 0) & (ii < h) & (jj >= 0) & (jj < w)
    flat = ii.clamp(0, h - 1) * w + jj.clamp(0, w - 1)
    out = torch.gather(x.reshape(B, C, h * w), 2,
                       flat.view(B, 1, H * W).expand(B, C, H * W))
    return (out.view(B, C, H, W) * valid.unsqueeze(1)).contiguous()


class ResidentDataset:
    """A dataset held in device memory once: ``images`` (N, C, h, w) or (N, h, w), uint8
    (pixels / 255, as ToTensor) or floating in [0, 1] (kept as fp32); ``labels`` (N,) uint8 or
    any integer type (kept as int64).  Batches come out as (B, C, H, W) fp32 with ``out_size``
    = (H, W) >= (h, w): zero padding of (H - h) // 2 per side, plus the training transform's
    random translation where a view asks for it.  C <= 4."""

    def __init__(self, images, labels, out_size=(40, 40), device="cuda"):
        images, labels = torch.as_tensor(images), torch.as_tensor(labels)
        if images.dim() == 3:
            images = images.unsqueeze(1)
        if images.dim() != 4 or labels.dim() != 1 or labels.shape[0] != images.shape[0]:
            raise ValueError("images (N, C, h, w) or (N, h, w) and labels (N,) expected")
        if images.shape[0] == 0 or images.shape[0] >= 2 ** 31:
            raise ValueError("a dataset holds 1 .. 2^31 - 1 examples")
        if images.dtype != torch.uint8:
            if not images.dtype.is_floating_point:
                raise ValueError("images must be uint8 or floating point")
            images = images.to(torch.float32)
        if labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise ValueError("labels must be integers")
        if labels.dtype != torch.uint8:
            labels = labels.to(torch.int64)
        self.n, self.C, self.h, self.w = images.shape
        self.H, self.W = (int(v) for v in out_size)
        if not (1 <= self.C <= 4 and self.h <= self.H and self.w <= self.W):
            raise ValueError(f"C <= 4 and out_size >= (h, w) needed, got C={self.C}, "
                             f"(h, w)=({self.h}, {self.w}), out_size={tuple(out_size)}")
        self.device = torch.device(device)
        self.images = images.to(self.device).contiguous()
        self.labels = labels.to(self.device).contiguous()

    @property
    def pads(self):
        return (self.H - self.h) // 2, (self.W - self.w) // 2

    def __len__(self):
        return self.n

    def view(self, shuffle=False, translate=True, seed=0, rank=0, world=1, drop_last=True,
             affine=None, flip=False, max_shift=None, interpolation="nearest"):
        """The whole dataset as one view (``DatasetView``)."""
        return DatasetView(self, None, shuffle, translate, seed, rank, world, drop_last,
                           affine, flip, max_shift, interpolation)

    def split(self, lengths, generator=None, **view_args):
        """Views over the rows ``torch.utils.data.random_split(range(N), lengths,
        generator)`` gives (``torch.randperm(N, generator=generator)`` cut in turn); lengths
        are integers summing to N.  ``view_args`` (shuffle, translate, seed, rank, world,
        drop_last, affine, flip, max_shift, interpolation) apply to every view; a view's
        attributes can be changed afterwards."""
        lengths = [int(v) for v in lengths]
        if sum(lengths) != self.n or any(v <= 0 for v in lengths):
            raise ValueError("lengths must be positive and sum to the dataset's size")
        perm = torch.randperm(self.n, generator=generator)
        views, off = [], 0
        for v in lengths:
            views.append(DatasetView(self, perm[off:off + v], **view_args))
            off += v
        return views


class DatasetView:
    """A view of a ``ResidentDataset``: ``index`` (its dataset rows, None: all), read in the
    epoch's order (``shuffle``: a keyed pseudo-random permutation per epoch, ``feistel_order``;
    else the identity -- the reference's loaders do not shuffle) with per-example shifts
    (``translate``; else centred padding).  The reference's validation split inherits the
    training transform (``random_split`` shares the dataset object), so translate it too for
    parity; its test set is not padded at all, which does not fit a 40 x 40 model: give the
    test view ``translate=False`` for centred padding.

    Rank sharding: step s of an epoch takes the global batch of world*B positions from
    s*world*B; rank r takes slots [r*B, (r+1)*B).  An epoch has spe = n // (world*B) such
    full steps.  ``drop_last`` (the default) ends it there: the r = n - spe*world*B last
    positions are not trained -- without shuffling the same examples every epoch.
    ``drop_last=False`` -- the reference's loaders (base_experiment.py:79-82) -- adds one
    short step when r > 0: each rank takes b = ceil(r / world) positions, rank k those from
    spe*world*B + k*b, and a position p >= n reads the row of p - n (the epoch's first
    examples again, as DistributedSampler pads) with a shift drawn from p itself.  A
    ``TrainStep`` runs that step on its remainder step of batch b.

    ``affine`` (``dict(degrees=, scale=, shear=)``, ``affine_ranges``): the other arguments
    of the reference's ``RandomAffine`` -- every example is resampled, nearest neighbour,
    through a rotation / scale / shear about the padded image's centre drawn per epoch
    position, composed with the shift above (``affine_coefficients``; the shift acts on the
    padded image, so unlike without ``affine`` it can augment an unpadded 32 x 32 dataset
    too).  ``degrees=0`` alone gives the bits of ``affine=None``.  The positions' fixed-point
    coefficients are built on the host and uploaded once per (view, epoch) -- (positions, 6)
    int32, about 1.4 MB for 60 000 examples, this epoch's table and the previous one kept
    alive for launches still in flight -- so the first device read of an epoch pays one
    host-to-device copy, and every other step of the epoch stays "prologue launch + replay,
    no torch operator, no copy".  An affinely warped test view (affNIST-style viewpoint
    checks) is ``ds.view(translate=False, affine=...)``.

    Three more arguments ride in the same table (without ``affine`` it is built with degrees
    0, scale 1, shear 0) and cost the device nothing of their own:
    ``flip=True`` is RandomHorizontalFlip(p = 0.5): the positions whose ``flip_bits`` is set
    read their example mirrored left to right, before padding, shift or warp.
    ``max_shift=(sy, sx)`` (non-negative ints) replaces the pads as the translation's range
    where ``translate`` is on: dy = ``shift_rule(r, sy)``, dx = ``shift_rule(r, sx)`` of the
    same draw; a range beyond the pad cuts off what leaves the frame and fills with zeros.
    On an unpadded 32 x 32 dataset ``max_shift=(4, 4)`` is RandomCrop(32, padding=4) up to
    the endpoint rule: ``shift_rule`` is round(U(-s, s)), so -s and +s each come up half as
    often as the values between, where RandomCrop draws uniform integers.
    ``interpolation="bilinear"`` samples the four neighbours with 8-bit weights instead of
    the nearest pixel (``affine_warp`` has the rule; smooth strokes under rotation); at
    integer coordinates -- ``degrees=0`` -- it is the nearest form bit for bit.
    ``epoch`` / ``cursor`` (steps taken in the epoch) advance with ``TrainStep.step_from``;
    ``state_dict`` carries them so that a resumed run continues in the same order."""

    def __init__(self, dataset, index=None, shuffle=False, translate=True, seed=0, rank=0,
                 world=1, drop_last=True, affine=None, flip=False, max_shift=None,
                 interpolation="nearest"):
        self.dataset = dataset
        if index is not None:
            index = torch.as_tensor(index).to("cpu", torch.int64).contiguous()
            if index.dim() != 1 or index.numel() == 0 or \
                    int(index.min()) < 0 or int(index.max()) >= dataset.n:
                raise ValueError("index must hold dataset rows")
        self.index = index
        self.n = dataset.n if index is None else index.numel()
        self.index_dev = None if index is None else \
            index.to(torch.int32).to(dataset.device)
        if not (isinstance(world, int) and world >= 1 and 0 <= rank < world):
            raise ValueError(f"rank {rank} of world {world}")
        self.shuffle, self.translate = bool(shuffle), bool(translate)
        self.seed = int(seed) & ((1 << 64) - 1)
        self.rank, self.world = int(rank), int(world)
        self.drop_last = bool(drop_last)
        if not self.drop_last and self.n < self.world:
            raise ValueError(f"{self.n} examples cannot give each of {self.world} ranks one")
        self.affine = affine_ranges(affine)
        self.flip, self.max_shift, self.interpolation = \
            self._options(flip, max_shift, interpolation)
        self._tables = {}               # (device coefficient tables: ``_affine_table``)
        self.epoch = self.cursor = 0

    @staticmethod
    def _options(flip, max_shift, interpolation):
        if not isinstance(flip, bool):
            raise ValueError(f"flip: a bool expected, got {flip!r}")
        if interpolation not in INTERPOLATIONS:
            raise ValueError(f"interpolation: one of {INTERPOLATIONS} expected, "
                             f"got {interpolation!r}")
        return flip, shift_ranges(max_shift), interpolation

    @property
    def uses_table(self):
        """The view's examples are sampled through the epoch's coefficient table."""
        return self.affine is not None or self.flip or self.max_shift is not None \
            or self.interpolation != "nearest"

    def __len__(self):
        return self.n

    # -- the order ------------------------------------------------------------------------
    def steps_per_epoch(self, batch):
        """Full steps of ``batch`` per rank in an epoch."""
        return self.n // (self.world * batch)

    def remainder(self, batch):
        """Each rank's batch in the epoch's short last step: ceil(r / world) of the r
        positions the full steps leave; 0 with ``drop_last`` or when nothing is left."""
        if self.drop_last:
            return 0
        r = self.n - self.steps_per_epoch(batch) * self.world * batch
        return -(-r // self.world)

    def steps_in_epoch(self, batch):
        """The epoch's steps: the full ones, plus the short one when there is one."""
        return self.steps_per_epoch(batch) + (self.remainder(batch) > 0)

    def positions(self, step, batch):
        """Epoch positions of this rank's slots in step ``step`` (``step`` =
        ``steps_per_epoch(batch)`` with a remainder: the short step's, unwrapped -- they may
        reach past n)."""
        b = self.remainder(batch) if step == self.steps_per_epoch(batch) else 0
        if b:
            return step * self.world * batch + self.rank * b + torch.arange(b)
        return step * self.world * batch + self.rank * batch + torch.arange(batch)

    def rows_and_shifts(self, epoch, positions):
        """(dataset rows, (len, 2) shifts) of epoch positions -- the CPU path.  Without
        ``drop_last`` a position p >= n takes the row of p - n and keeps p for its shift."""
        p = torch.as_tensor(positions, dtype=torch.int64)
        q = p if self.drop_last else torch.where(p >= self.n, p - self.n, p)
        vr = feistel_order(q, self.n, self.seed, epoch) if self.shuffle else q
        rows = vr if self.index is None else self.index[vr]
        ds = self.dataset
        lim = ds.pads if self.max_shift is None else self.max_shift
        shifts = translate_shifts(p, epoch, self.seed, lim) if self.translate \
            else torch.zeros(p.numel(), 2, dtype=torch.int64)
        return rows, shifts

    def indices_and_shifts(self, epoch, step, batch):
        return self.rows_and_shifts(epoch, self.positions(step, batch))

    def coefficients(self, epoch, positions):
        """(len, 6) int64 inverse-map coefficients of epoch positions (views that use the
        table: ``affine``, ``flip``, ``max_shift``, bilinear; a position p >= n keeps p for
        its draws, as for its shift) -- the CPU path."""
        ds = self.dataset
        return affine_coefficients(positions, epoch, self.seed, ds.pads, (ds.H, ds.W),
                                   _IDENTITY if self.affine is None else self.affine,
                                   self.translate, max_shift=self.max_shift, flip=self.flip,
                                   width=ds.w)

    def _cpu_batch(self, epoch, positions):
        rows, shifts = self.rows_and_shifts(epoch, positions)
        ds = self.dataset
        src = ds.images[rows.to(ds.device)].cpu()
        if self.uses_table:
            image = affine_warp(src, self.coefficients(epoch, positions), (ds.H, ds.W),
                                self.interpolation)
        else:
            image = pad_and_translate(src, (ds.H, ds.W), shifts=shifts)
        return image, ds.labels[rows.to(ds.device)].cpu().to(torch.int64)

    def batch(self, epoch, step, batch):
        """This rank's batch of step ``step`` of ``epoch`` on the CPU: (image (B, C, H, W)
        fp32, label (B,) int64) -- what the device gather writes, bit for bit.  ``step`` =
        ``steps_per_epoch(batch)`` without ``drop_last``: the short step's (b, ...)."""
        return self._cpu_batch(epoch, self.positions(step, batch))

    def materialise(self, epoch=None):
        """Every example of the view in epoch position order (CPU): what an evaluation of
        the view reads."""
        return self._cpu_batch(self.epoch if epoch is None else epoch, torch.arange(self.n))

    # -- the device side --------------------------------------------------------------------
    def _affine_table(self, epoch):
        """The epoch's (positions, 6) int32 coefficient table on the device: every position
        a step of the epoch can read -- n, plus the world - 1 a short step's padding can add
        without ``drop_last``.  Built by the CPU path and uploaded on first use; the two
        most recent tables stay alive (launches reading the previous epoch's may still be
        in flight)."""
        ds = self.dataset
        count = self.n + (0 if self.drop_last else self.world - 1)
        key = (int(epoch), self.seed, self.translate, count,
               None if self.affine is None else tuple(sorted(self.affine.items())),
               self.flip, self.max_shift, self.interpolation)
        table = self._tables.get(key)
        if table is None:
            table = self.coefficients(epoch, torch.arange(count)).to(torch.int32) \
                .contiguous().to(ds.device)
            while len(self._tables) >= 2:
                del self._tables[next(iter(self._tables))]
            self._tables[key] = table
        return table

    def desc(self, epoch, position, rank=None):
        """struct scae_batch_source_desc of this rank's batch at epoch position
        ``position`` (of the step's global batch).  An ``affine`` view's descriptor points
        at the epoch's coefficient table (uploaded here the first time the epoch is
        asked for)."""
        from . import _lib
        ds = self.dataset
        d = _lib.BatchSourceDesc()
        d.images, d.labels = ds.images.data_ptr(), ds.labels.data_ptr()
        d.index = None if self.index_dev is None else self.index_dev.data_ptr()
        d.rows, d.n = ds.n, self.n
        d.image_u8, d.label_u8 = int(ds.images.dtype == torch.uint8), \
            int(ds.labels.dtype == torch.uint8)
        d.C, d.h, d.w, d.H, d.W = ds.C, ds.h, ds.w, ds.H, ds.W
        d.shuffle, d.translate = int(self.shuffle), int(self.translate)
        d.seed, d.epoch, d.position = self.seed, int(epoch), int(position)
        d.rank, d.world = self.rank if rank is None else rank, self.world
        d.wrap = int(not self.drop_last)
        if self.uses_table:
            table = self._affine_table(epoch)
            d.affine, d.affine_rows = table.data_ptr(), table.shape[0]
            if self.interpolation == "bilinear":
                d.translate = 2         # (with a table: the sampling mode)
        return d

    def check(self, batch, image_shape):
        ds = self.dataset
        if tuple(image_shape) != (ds.C, ds.H, ds.W):
            raise ValueError(f"the view gives ({ds.C}, {ds.H}, {ds.W}) images, the step "
                             f"takes {tuple(image_shape)}")
        if ds.device.type != "cuda":
            raise ValueError("a step reads a dataset held on the device")
        if self.steps_in_epoch(batch) == 0:
            raise ValueError(f"{self.n} examples make no batch of {batch} x {self.world} ranks")

    def gather(self, batch, epoch=None, step=None, image=None, label=None, rank=None,
               position=None):
        """This rank's batch on the device in one launch (scae_gather_batch_f32) -- by default
        the batch the next ``TrainStep.step_from`` takes; into ``image`` / ``label`` when
        given.  -> (image, label)."""
        import ctypes
        from . import _lib
        ds = self.dataset
        epoch = self.epoch if epoch is None else epoch
        if position is None:
            position = (self.cursor if step is None else step) * self.world * batch
        if image is None:
            image = torch.empty(batch, ds.C, ds.H, ds.W, device=ds.device)
        if label is None:
            label = torch.empty(batch, dtype=torch.int64, device=ds.device)
        _lib.call("scae_gather_batch_f32", ctypes.c_void_p(image.data_ptr()),
                  ctypes.c_void_p(label.data_ptr()), batch,
                  ctypes.byref(self.desc(epoch, position, rank)),
                  ctypes.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream))
        return image, label

    def take_step(self, batch):
        """(epoch, position) of the next step's global batch, with ``.size`` the rank's
        batch in it (``batch``, or ``remainder(batch)`` for the short step); advances the
        cursor, wrapping to the next epoch after ``steps_in_epoch(batch)`` steps."""
        spe, last = self.steps_per_epoch(batch), self.steps_in_epoch(batch)
        if self.cursor >= last:         # (a state loaded for another batch size)
            self.epoch, self.cursor = self.epoch + 1, 0
        size = batch if self.cursor < spe else self.remainder(batch)
        out = StepAt(self.epoch, self.cursor * self.world * batch, size)
        self.cursor += 1
        if self.cursor == last:
            self.epoch, self.cursor = self.epoch + 1, 0
        return out

    def state_dict(self):
        """The cursor says where the epoch stands: with ``drop_last=False`` a cursor of
        ``steps_per_epoch(B)`` is a short step still to come."""
        return {"epoch": self.epoch, "cursor": self.cursor, "seed": self.seed,
                "shuffle": self.shuffle, "translate": self.translate, "n": self.n,
                "rank": self.rank, "world": self.world, "drop_last": self.drop_last,
                "affine": None if self.affine is None else
                {k: list(v) for k, v in self.affine.items()},
                "flip": self.flip, "interpolation": self.interpolation,
                "max_shift": None if self.max_shift is None else list(self.max_shift)}

    def load_state_dict(self, sd):
        if sd.get("n", self.n) != self.n or sd.get("world", self.world) != self.world:
            raise ValueError("state of a view of another size / world")
        self.seed = int(sd.get("seed", self.seed))
        self.shuffle = bool(sd.get("shuffle", self.shuffle))
        self.translate = bool(sd.get("translate", self.translate))
        self.drop_last = bool(sd.get("drop_last", self.drop_last))
        if "affine" in sd:
            self.affine = affine_ranges(sd["affine"])
        # (a state written before these arguments existed leaves the view's own)
        self.flip, self.max_shift, self.interpolation = self._options(
            sd.get("flip", self.flip), sd.get("max_shift", self.max_shift),
            sd.get("interpolation", self.interpolation))
        self.epoch, self.cursor = int(sd["epoch"]), int(sd["cursor"])


class StepAt(tuple):
    """(epoch, position) of a step's global batch, as ``DatasetView.take_step`` hands it out;
    ``size``: the rank's batch in that step."""

    def __new__(cls, epoch, position, size):
        out = super().__new__(cls, (epoch, position))
        out.size = size
        return out


_IDX_TYPES = {0x08: torch.uint8, 0x09: torch.int8, 0x0B: torch.int16, 0x0C: torch.int32,
              0x0D: torch.float32, 0x0E: torch.float64}


def read_idx(path):
    """An IDX file (MNIST's format: train-images-idx3-ubyte, ...), plain or gzip-compressed
    (``.gz``), from local disk -> a CPU tensor of its type and shape."""
    import numpy as np
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as f:
        raw = f.read()
    if len(raw) < 4 or raw[0] != 0 or raw[1] != 0 or raw[2] not in _IDX_TYPES:
        raise ValueError(f"{path}: not an IDX file")
    nd = raw[3]
    dims = [int.from_bytes(raw[4 + 4 * i:8 + 4 * i], "big") for i in range(nd)]
    dtype = _IDX_TYPES[raw[2]]
    np_t = {torch.uint8: ">u1", torch.int8: ">i1", torch.int16: ">i2", torch.int32: ">i4",
            torch.float32: ">f4", torch.float64: ">f8"}[dtype]
    count = math.prod(dims)
    data = np.frombuffer(raw, dtype=np_t, count=count, offset=4 + 4 * nd)
    return torch.from_numpy(data.astype(np_t[1:]).reshape(dims).copy())
