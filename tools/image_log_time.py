"""Time the validation image sheets (validation_epoch_end, base_experiment.py:152-182) two
ways, HIP-event timed, and print one JSON line per way:

    python tools/image_log_time.py CONFIG [--reps N] [--alternatives]

CONFIG: cfg2 (MNIST 40x40, 24/24, B=128) or cfg3 (configs[2]'s shape, 48/64, B=1024).
Ways: (a) "materialising" -- what a caller did before EvalStep.validation_images: an eager
no_grad forward of the staged batch, ``.mode()`` of every reconstruction over its rendered
(B, M+1, C, H, W) tensors, and the three sheets laid out by torch ops on the device;
(b) "validation_images" -- the same eager forward, the fused render-and-mode kernel for the 8
logged images, image 0's components alone, the sheet kernel.  Reported per way: the median ms
of a call (each call synchronised), the share of it spent after the forward, and
``torch.cuda.max_memory_allocated`` above what was allocated before the call.  Both ways run
in this one process on the same model and batch; the sheets are compared bit for bit first.
Run each CONFIG in a process of its own under its own time limit."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from torch_scae_amd import EvalStep, factory  # noqa: E402
from torch_scae_amd.distributions import GaussianMixture  # noqa: E402

CONFIGS = {
    "cfg2": (dict(image_shape=(1, 40, 40), n_classes=10, n_part_caps=24, n_obj_caps=24), 128),
    "cfg3": (dict(image_shape=(1, 40, 40), n_classes=10, n_part_caps=48, n_obj_caps=64), 1024),
}


def torch_sheet(t, nrow, padding=1, pad_value=0.0):
    """The sheet layout in torch ops on t's device (t: (N, C, H, W), N > 1)."""
    N, C, H, W = t.shape
    t = t.expand(N, 3, H, W)
    xmaps = min(nrow, N)
    ymaps = -(-N // xmaps)
    sheet = t.new_full((3, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding),
                       pad_value)
    for k in range(N):
        y = (k // xmaps) * (H + padding) + padding
        x = (k % xmaps) * (W + padding) + padding
        sheet[:, y:y + H, x:x + W] = t[k]
    return sheet


def materialising(step, res, n=8):
    """The three sheets with every mixture's mode taken over its rendered tensors."""
    keys = ["rec"] + (["bottom_up_rec", "top_down_rec"]
                      if step.model.reconstruct_alternatives else [])
    unfused = GaussianMixture._fused_image
    GaussianMixture._fused_image = lambda self: False     # the path before the fused kernel
    try:
        with torch.no_grad():
            rows = [step.image[:n]] + [res[k].pdf.mode()[:n] for k in keys]
    finally:
        GaussianMixture._fused_image = unfused
    templates = res.templates[0]
    nrow = int(templates.shape[0] ** 0.5)
    return {"recons": torch_sheet(torch.cat(rows, 0), n),
            "templates": torch_sheet(templates, nrow),
            "transformed_templates": torch_sheet(res.transformed_templates[0], nrow)}


def measure(fn, step, reps):
    """-> (median ms of forward + sheets, median ms of the sheets alone, peak bytes above
    the allocation before the call)."""
    total, tail, peak = [], [], 0
    for i in range(reps + 3):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        res = step._eager_result()
        e[1].record()
        out = fn(step, res)
        e[2].record()
        torch.cuda.synchronize()
        if i >= 3:          # (warm-up calls dropped)
            total.append(e[0].elapsed_time(e[2]))
            tail.append(e[1].elapsed_time(e[2]))
            peak = max(peak, torch.cuda.max_memory_allocated() - base)
        del res, out
    return statistics.median(total), statistics.median(tail), peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--alternatives", action="store_true")
    args = ap.parse_args()
    cfg, B = CONFIGS[args.config]
    cfg = dict(cfg, scae_params=dict(reconstruct_alternatives=args.alternatives))
    torch.manual_seed(0)
    model = factory.make_scae(cfg).cuda().train()
    with torch.no_grad():
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.normal_(0, 0.05)
    g = torch.Generator().manual_seed(1)
    image = torch.rand(B, *cfg["image_shape"], generator=g).cuda()
    label = torch.randint(0, 10, (B,), generator=g).cuda()
    step = EvalStep(model, B, cfg["image_shape"])
    step(image, label)

    res = step._eager_result()
    fused = step.validation_images(res)
    old = materialising(step, res)
    same = all(torch.equal(fused[k], old[k]) for k in old)
    del res, fused, old

    M, (C, H, W) = cfg["n_part_caps"], cfg["image_shape"]
    tag = dict(config=args.config, batch=B, alternatives=args.alternatives,
               one_rendered_tensor_bytes=B * (M + 1) * C * H * W * 4, sheets_equal=same)
    for way, fn in (("materialising", materialising),
                    ("validation_images", lambda s, r: s.validation_images(r))):
        ms, tail, peak = measure(fn, step, args.reps)
        print(json.dumps(dict(tag, way=way, ms_per_call=round(ms, 4),
                              ms_after_forward=round(tail, 4), peak_bytes=int(peak))),
              flush=True)


if __name__ == "__main__":
    main()
