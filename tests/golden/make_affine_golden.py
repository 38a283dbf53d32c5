"""Writes affine_nearest_pil.npz: what Pillow's nearest-neighbour AFFINE transform gives for
recorded inputs and coefficients -- the yardstick of data.affine_warp and of the device
gather's affine form (tests/test_affine_view.py, tests/test_affine_view_gpu.py).

    python tests/golden/make_affine_golden.py

Two groups of cases, random uint8 pixels: ``a`` 40 x (1, 28, 28) -> 40 x 40 and ``b``
16 x (3, 32, 32) -> 32 x 32.  Per group: ``images_*`` (N, C, h, w) uint8, ``coeffs_*`` (N, 6)
int32 k0..k5 (data.affine_coefficients: rotation, scale, shear and translation; the last
four of each group translation only), ``pil_*`` (N, C, H, W) uint8 Pillow's pixels of the
zero-padded image under ``Image.transform(AFFINE, NEAREST, fillcolor=0)`` with the matrix
the coefficients stand for.  Pure scale (k1 = k3 = 0 with k0 or k4 != 65536) is left out:
Pillow resamples it on another, double-accumulating path.  Before writing, the script
compares ``pil_*`` with data.affine_warp and reports the images that differ (0 expected)."""
import os
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from torch_scae_amd import data as D  # noqa: E402

FULL = dict(degrees=30, scale=(0.8, 1.25), shear=(-12, 12, -6, 6))
ROTATE = dict(degrees=(-180, 180))


def pil_matrix(k):
    """The fp64 matrix whose Pillow fixed-point form is exactly k0..k5."""
    k = [float(v) for v in k]
    return (k[0] / 65536, k[1] / 65536, (k[2] - 0.5 * k[0] - 0.5 * k[1]) / 65536,
            k[3] / 65536, k[4] / 65536, (k[5] - 0.5 * k[3] - 0.5 * k[4]) / 65536)


def pil_warp(images, coeffs, out_size):
    """(N, C, h, w) uint8 -> (N, C, H, W) uint8 through Pillow, channel by channel."""
    N, C, h, w = images.shape
    H, W = out_size
    ph, pw = (H - h) // 2, (W - w) // 2
    out = np.zeros((N, C, H, W), np.uint8)
    for n in range(N):
        for c in range(C):
            padded = np.zeros((H, W), np.uint8)
            padded[ph:ph + h, pw:pw + w] = images[n, c]
            got = Image.fromarray(padded).transform(
                (W, H), Image.AFFINE, data=pil_matrix(coeffs[n]), resample=Image.NEAREST,
                fillcolor=0)
            out[n, c] = np.asarray(got)
    return out


def in_pillow_comparison(coeffs):
    """Rows whose matrix Pillow samples on its fixed-point path, or exactly: an off-diagonal
    term, or the identity linear part."""
    k = torch.as_tensor(coeffs)
    return (k[:, 1] != 0) | (k[:, 3] != 0) | ((k[:, 0] == 65536) & (k[:, 4] == 65536))


def group(seed, N, C, h, out):
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (N, C, h, h), generator=g, dtype=torch.uint8)
    pads, size = ((out - h) // 2,) * 2, (out, out)
    p = torch.arange(N)
    half = (N - 4) // 2
    k = torch.cat([
        D.affine_coefficients(p[:half], 0, seed, pads, size, FULL),
        D.affine_coefficients(p[half:N - 4], 1, seed, pads, size, ROTATE),
        D.affine_coefficients(p[N - 4:], 2, seed, pads, size, dict(degrees=0))])
    assert bool(in_pillow_comparison(k).all())
    pil = pil_warp(images.numpy(), k.numpy(), size)
    mine = (D.affine_warp(images, k, size) * 255).round().to(torch.uint8).numpy()
    differ = int((pil != mine).reshape(N, -1).any(1).sum())
    print(f"{N} x ({C}, {h}, {h}) -> {out}: {differ} images differ from Pillow")
    return images.numpy(), k.to(torch.int32).numpy(), pil


def main():
    ia, ka, pa = group(11, 40, 1, 28, 40)
    ib, kb, pb = group(12, 16, 3, 32, 32)
    np.savez_compressed(os.path.join(HERE, "affine_nearest_pil.npz"), images_a=ia,
                        coeffs_a=ka, pil_a=pa, images_b=ib, coeffs_b=kb, pil_b=pb)


if __name__ == "__main__":
    main()
