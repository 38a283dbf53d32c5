"""Time the part segmentation (torch_scae_amd.segment) two ways, HIP-event timed, and print one
JSON line per way and slice:

    python tools/segment_time.py CONFIG [--reps N]

CONFIG: cfg2 (MNIST 40x40, 24 templates of 11x11, B=128) or cfg3 (configs[2]'s shape, 48
templates, B=1024), on random decoder inputs at those shapes (alpha mode, one channel, presence
given).  Slices: the 8 logged images and the whole batch.  Ways: (a) "materialising" --
``ops.render_templates`` of the slice's images (a descriptor of those images alone), then the
E-step in torch ops on the device: joint logits, softmax over components, channel mean, max /
arg-max, per-part sums, owner gather and the two coloured images; (b) "render_gmm_parts" -- the
fused kernel from the compact inputs.  Reported per way: the median ms of a call (each call
synchronised) and ``torch.cuda.max_memory_allocated`` above what was allocated before the call.
Both ways run in this one process on the same inputs; owners are compared first (a few may
differ where two responsibilities are within rounding of each other: the count is printed).
Run each CONFIG in a process of its own under its own time limit."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from torch_scae_amd import ops, segment  # noqa: E402

CONFIGS = {"cfg2": dict(B=128, M=24, O=24), "cfg3": dict(B=1024, M=48, O=64)}
C, H, W, TH, TW = 1, 40, 40, 11, 11
PER_IMAGE = ("templates", "pose", "presence", "bg_image")


def make_inputs(B, M, O):
    g = torch.Generator().manual_seed(0)
    pose = torch.tensor([1.6, 0.0, 0.0, 0.0, 1.6, 0.0]) + \
        torch.randn(B, M, 6, generator=g) * torch.tensor([0.4, 0.3, 0.5, 0.3, 0.4, 0.5])
    t = dict(templates=torch.rand(B, M, C, TH, TW, generator=g),
             templates_alpha=torch.randn(1, M, 1, TH, TW, generator=g) * 2, pose=pose,
             presence=0.7 + 0.3 * torch.rand(B, M, generator=g),
             bg_value=torch.randn(1, generator=g) - 1.5,
             bg_mixing_logit=torch.randn(1, generator=g))
    inputs = ops.DecoderInputs((H, W), **{k: v.cuda() for k, v in t.items()})
    x = torch.rand(B, C, H, W, generator=g).cuda()
    table = torch.randint(0, O, (B, M), generator=g, dtype=torch.int32).cuda()
    return inputs, x, table


def head(inputs, n):
    """The decoder inputs of the first n images alone."""
    return ops.DecoderInputs(inputs.output_size, **{
        f: (getattr(inputs, f)[:n] if f in PER_IMAGE and getattr(inputs, f) is not None
            else getattr(inputs, f)) for f in ops.DecoderInputs.FIELDS})


def materialising(inputs, x, table, pal, n):
    """Render the n images' (n, M+1, ., H, W) tensors, then the E-step in torch ops."""
    tt, ml = ops.render_templates(head(inputs, n))              # sigma = 1: no out_scale
    M = tt.shape[1] - 1
    j = ml - 0.5 * (x[:n, None] - tt) ** 2
    R = torch.softmax(j, 1).mean(2)                             # (n, K, H, W)
    conf, part = R.max(1)
    mass = R.sum((2, 3))
    tone = tt.gather(1, part[:, None, None].expand(-1, 1, tt.shape[2], -1, -1))[:, 0].mean(1)
    bg = part == M
    group = table[:n].long().gather(1, part.clamp(max=M - 1).flatten(1)).view_as(part)
    group = torch.where(bg, -1, group)

    def colour(ids):
        rgb = tone[:, None] * pal[ids % pal.shape[0]].movedim(-1, 1)
        return torch.where(bg[:, None], tone[:, None].expand_as(rgb), rgb)
    return segment.Segmentation(part.int(), conf, mass, group.int(), colour(part),
                                colour(group))


def fused(inputs, x, table, pal, n):
    return ops.render_gmm_parts(inputs, x=x, part_group=table, palette=pal, first=0, count=n)


def measure(fn, args, reps):
    ms, peak = [], 0
    for i in range(reps + 3):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        out = fn(*args)
        e[1].record()
        torch.cuda.synchronize()
        if i >= 3:          # (warm-up calls dropped)
            ms.append(e[0].elapsed_time(e[1]))
            peak = max(peak, torch.cuda.max_memory_allocated() - base)
        del out
    return statistics.median(ms), peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    B, M = cfg["B"], cfg["M"]
    inputs, x, table = make_inputs(**cfg)
    pal = segment.palette(max(M, cfg["O"])).cuda()
    with torch.no_grad():
        for n in (8, B):
            a, b = materialising(inputs, x, table, pal, n), fused(inputs, x, table, pal, n)
            differ = int((a.part != b.part).sum())
            mass_gap = float((a.mass - b.mass).abs().max())
            del a, b
            tag = dict(config=args.config, batch=B, images=n, owners_differing=differ,
                       pixels=n * H * W, max_mass_gap=mass_gap,
                       one_rendered_tensor_bytes=n * (M + 1) * C * H * W * 4)
            for way, fn in (("materialising", materialising), ("render_gmm_parts", fused)):
                ms, peak = measure(fn, (inputs, x, table, pal, n), args.reps)
                print(json.dumps(dict(tag, way=way, ms_per_call=round(ms, 4),
                                      peak_bytes=int(peak))), flush=True)


if __name__ == "__main__":
    main()
