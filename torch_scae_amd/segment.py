"""Part segmentation maps: which part template, and which object capsule through it, owns
each pixel of a reconstruction.

The decoder explains an image as a per-pixel mixture of its M transformed templates and a
background (part_decoder.py:174-237).  The mixture's E-step -- the posterior over components
given the observed pixel -- says which part explains which pixel; its arg-max is the
segmentation people look at first, its per-part sums say how much of an image each part
covers.  ``segment`` takes both from the fused kernel (``ops.render_gmm_parts``: nothing of
the size of the rendered (B, M+1, C, H, W) tensors is made); ``segment_host`` is the same
definitions written plainly in numpy over materialised tensors, for CPU use and as the tests'
reference.

The part-to-object owner comes from ``posterior_mixing_prob``: the reference's
``is_from_capsule`` is ``winning_vote_idx // n_input_points`` (object_decoder.py:334), 0 almost
everywhere, and no usable owner table.

Definitions, for one image with K = M + 1 components, values loc[k, c, p], mixing logits
ml[k, cm, p] (cm = 0 for one logit channel, else c), Normal scale sigma and target x[c, p]:

  j[k,c,p] = ml[k,cm,p] - 0.5 (x[c,p] - loc[k,c,p])^2 / sigma^2      (x None: ml[k,cm,p])
  r[k,c,p] = softmax_k j[.,c,p]           two passes (max, then sum) in component order
  R[k,p]   = (1/C) sum_c r[k,c,p]         channels added in order
  part[p]  = first k with the largest R[k,p]   (k = M: the background)
  conf[p]  = R[part[p], p]
  mass[k]  = sum_p R[k,p]
  group[p] = part_group[part[p]] for part[p] < M, else -1
  rgb[:,p] = t[p] palette[id mod P], id = part[p] or group[p], t[p] = mean_c loc[part[p],c,p];
             t[p] (1, 1, 1) on a background pixel
"""
import collections
import colorsys
import math

import numpy as np
import torch

from . import ops

__all__ = ["palette", "part_owner", "segment", "segment_host", "part_usage", "Segmentation",
           "PartUsage"]

# (part, conf, mass, group, rgb_part, rgb_group): the kernel's result tuple
Segmentation = ops.GmmParts
PartUsage = collections.namedtuple(
    "PartUsage", ["part_share", "capsule_share", "class_part_share", "class_capsule_share",
                  "class_count"])

_GOLDEN = (3.0 - math.sqrt(5.0)) / 2.0       # the golden angle as a share of the circle


def palette(n):
    """(n, 3) fp32 colours, the same on every call: hue i * golden angle (any run of
    consecutive ids gets well separated hues), saturation 0.75, value 1; HSV -> RGB in fp64,
    rounded to fp32 once."""
    if not isinstance(n, int) or isinstance(n, bool) or n <= 0:
        raise ValueError(f"palette size must be a positive int, got {n!r}")
    rows = [colorsys.hsv_to_rgb((i * _GOLDEN) % 1.0, 0.75, 1.0) for i in range(n)]
    return torch.from_numpy(np.asarray(rows, dtype=np.float64).astype(np.float32))


_default_palette = palette      # (``palette`` is also an argument name below)


def part_owner(res):
    """(B, M) int32: the object capsule that owns each part, the first largest of
    ``res.posterior_mixing_prob[b, :, m]`` (B, O, M)."""
    post = res["posterior_mixing_prob"].detach()
    if post.dim() != 3:
        raise ValueError(f"posterior_mixing_prob must be (B, O, M), got {tuple(post.shape)}")
    return _first_argmax(post, 1).to(torch.int32)


def _first_argmax(t, dim):
    """arg-max along dim, the lowest index among equals (torch.argmax does not promise it)."""
    n = t.shape[dim]
    shape = [1] * t.dim()
    shape[dim] = n
    idx = torch.arange(n, device=t.device).view(shape)
    top = t == t.amax(dim, keepdim=True)
    return torch.where(top, idx, n).amin(dim).clamp_(max=n - 1)


def segment(res, image=None, first=0, count=None, palette=None):
    """Segmentation of images [first, first + count) of a model result: ``res.rec``'s
    mixture given ``image`` (B, C, H, W; None: prior ownership), parts grouped by
    ``part_owner(res)``.  -> Segmentation of device tensors (ops.render_gmm_parts)."""
    pdf = res["rec"].pdf
    inputs = getattr(pdf, "_decoder_inputs", None)
    if inputs is None:
        raise ops.ScaeHipError("segment runs on the library's kernels and needs the compact "
                               "decoder inputs of a model on the HIP device; segment_host "
                               "serves materialised CPU tensors")
    if palette is not None:
        palette = palette.to(inputs.pose.device)
    with torch.no_grad():
        return ops.render_gmm_parts(inputs, x=image, part_group=part_owner(res),
                                    palette=palette, first=first, count=count)


def segment_host(loc, mixing_logits, sigma, x=None, part_group=None, palette=None,
                 dtype=np.float64):
    """The definitions at the top of this module, literally, in numpy at ``dtype`` for one
    image: loc (K, C, P), mixing_logits (K, Cm, P) with Cm in {1, C}, sigma a number, x
    (C, P) or None, part_group (M,) ints or None, palette (Q, 3) or None (then
    ``palette(M)``).  Trailing pixel dimensions may be any shape ((K, C, H, W) ...): they are
    kept.  -> (Segmentation, R) with R (K, pixels...) the responsibilities themselves."""
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)  # noqa
    loc = as_np(loc).astype(dtype)
    ml = as_np(mixing_logits).astype(dtype)
    K, C = loc.shape[:2]
    M, pix = K - 1, loc.shape[2:]
    if ml.shape[0] != K or ml.shape[1] not in (1, C) or ml.shape[2:] != pix:
        raise ValueError(f"logits {ml.shape} do not fit components {loc.shape}")
    loc, ml = loc.reshape(K, C, -1), ml.reshape(K, ml.shape[1], -1)
    P = loc.shape[2]
    j = np.broadcast_to(ml, loc.shape).copy()
    if x is not None:
        x = as_np(x).astype(dtype).reshape(C, -1)
        if x.shape[1] != P:
            raise ValueError(f"target of {x.shape[1]} pixels for components of {P}")
        var = dtype(float(sigma)) * dtype(float(sigma))
        d = x[None] - loc
        j = j - (dtype(0.5) * (d * d)) / var
    m = np.full((C, P), -np.inf, dtype)
    for k in range(K):                      # pass 1: the maximum, in component order
        m = np.maximum(m, j[k])
    e = np.exp(j - m[None]).astype(dtype)
    s = np.zeros((C, P), dtype)
    for k in range(K):                      # pass 2: the sum, in component order
        s = s + e[k]
    r = e / s[None]
    R = np.zeros((K, P), dtype)
    for c in range(C):                      # channels in order
        R = R + r[:, c]
    R = R * (dtype(1) / dtype(C))
    part = np.zeros(P, np.int32)
    conf = R[0].copy()
    for k in range(1, K):                   # strict >: the first largest
        take = R[k] > conf
        part[take] = k
        conf[take] = R[k][take]
    mass = R.sum(1, dtype=dtype)
    bg = part == M
    tone = np.zeros(P, dtype)
    for c in range(C):
        tone = tone + loc[part, c, np.arange(P)]
    tone = tone * (dtype(1) / dtype(C))
    pal = as_np(_default_palette(max(M, 1)) if palette is None else palette).astype(dtype)

    def colour(ids):
        rgb = tone[None] * pal[ids % pal.shape[0]].T
        rgb[:, bg] = tone[bg]
        return rgb.reshape(3, *pix)
    group = rgb_group = None
    if part_group is not None:
        table = as_np(part_group).astype(np.int64).reshape(-1)
        if table.shape[0] != M:
            raise ValueError(f"part_group must list the {M} parts, got {table.shape[0]}")
        group = np.where(bg, -1, table[np.minimum(part, M - 1)]).astype(np.int32)
        rgb_group = colour(group)
        group = group.reshape(pix)
    seg = Segmentation(part.reshape(pix), conf.reshape(pix), mass, group, colour(part),
                       rgb_group)
    return seg, R.reshape(K, *pix)


def part_usage(model, images, labels=None, batch_size=128, n_classes=None):
    """How much of an image each part, and each object capsule through its parts, covers on
    average over ``images`` (N, C, H, W): eager no_grad forwards in batches of ``batch_size``
    (the last may be short), the posterior mass per part from the kernel, its share of the
    H W pixels accumulated on the device in fp64; one host read at the end (and the labels'
    range checked before the first batch).

    -> PartUsage(part_share (M+1,), capsule_share (O+1,): the last entry is the background;
    with ``labels`` (N,) also class_part_share (n_classes, M+1), class_capsule_share
    (n_classes, O+1) -- the mean over each class's images, zero rows for absent classes --
    and class_count (n_classes,); else None), as fp64 numpy arrays."""
    if images.dim() != 4 or images.shape[0] == 0:
        raise ValueError("images must be a non-empty (N, C, H, W) tensor")
    if not isinstance(batch_size, int) or batch_size <= 0:
        raise ValueError(f"batch_size must be a positive int, got {batch_size!r}")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise ops.ScaeHipError("part_usage runs on the library's kernels: the model is on "
                               "the CPU")
    N = images.shape[0]
    if labels is not None:
        if tuple(labels.shape) != (N,):
            raise ValueError(f"labels must be ({N},), got {tuple(labels.shape)}")
        lo, hi = int(labels.min()), int(labels.max())     # (an argument check, before any work)
        if n_classes is None:
            n_classes = getattr(model, "n_classes", None) or hi + 1
        if lo < 0 or hi >= n_classes:
            raise ValueError(f"labels must lie in [0, {n_classes}), got [{lo}, {hi}]")
    HW = images.shape[2] * images.shape[3]
    was = model.training
    model.eval()
    acc = None
    try:
        with torch.no_grad():
            for i in range(0, N, batch_size):
                image = images[i:i + batch_size].to(dev)
                res = model(image)
                owner = part_owner(res)
                O = res["posterior_mixing_prob"].shape[1]
                seg = ops.render_gmm_parts(res["rec"].pdf._decoder_inputs, x=image,
                                           part_group=owner)
                share = seg.mass.double() / HW                       # (b, M+1)
                M = share.shape[1] - 1
                caps = torch.zeros(share.shape[0], O + 1, device=dev, dtype=torch.float64)
                caps.scatter_add_(1, owner.long(), share[:, :M])
                caps[:, O] = share[:, M]
                both = torch.cat([share, caps], 1)                   # (b, M+1 + O+1)
                if acc is None:
                    rows = 1 if labels is None else 1 + n_classes
                    acc = torch.zeros(rows, both.shape[1] + 1, device=dev,
                                      dtype=torch.float64)          # (last column: images)
                both = torch.cat([both, torch.ones_like(both[:, :1])], 1)
                acc[0] += both.sum(0)
                if labels is not None:
                    acc[1:].index_add_(0, labels[i:i + batch_size].to(dev).long(), both)
    finally:
        model.train(was)
    acc = acc.cpu().numpy()                                          # the one host read
    mean = acc[:, :-1] / np.maximum(acc[:, -1:], 1.0)
    cut = M + 1
    if labels is None:
        return PartUsage(mean[0, :cut], mean[0, cut:], None, None, None)
    return PartUsage(mean[0, :cut], mean[0, cut:], mean[1:, :cut], mean[1:, cut:],
                     acc[1:, -1].astype(np.int64))
