"""Time cfg-2's training step (MNIST 40x40, 24/24 capsules, B=128, RMSprop, graph replay) fed
by ``step_from`` from four views of the same resident dataset, HIP-event timed, and print one
JSON line per way:

    python tools/augment_time.py [--steps N] [--n EXAMPLES] [--rounds R] [--ways a,b,...]

(a) "translate": a shuffled, translated view -- the default path (tools/affine_time.py's
    "source");
(b) "flip_shift": the same with ``flip=True, max_shift=(8, 8)``: the table route with the
    identity map, nearest sampling;
(c) "affine": ``affine=dict(degrees=15, scale=(0.9, 1.1), shear=5)``, nearest;
(d) "bilinear": (c) with ``interpolation="bilinear"`` and ``flip=True``: four taps per pixel.
Each timed window starts at the head of an epoch whose table is already on the device and ends
inside it (``--steps`` + 20 warm-up steps must fit an epoch).  Reported per way: the best and
the worst of ``--rounds`` alternated rounds from the same parameter snapshot -- their gap is the
run-to-run spread a difference has to exceed.  ``--ways translate,affine`` runs on a commit
from before (b) and (d) existed, for the default path's figure there.  The dataset is synthetic
uint8 28x28 noise, 60 000 examples."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torch_scae_amd import data, factory  # noqa: E402
from torch_scae_amd.train_step import TrainStep  # noqa: E402

CFG2 = dict(image_shape=(1, 40, 40), n_classes=10, n_part_caps=24, n_obj_caps=24,
            scae_params=dict(reconstruct_alternatives=False))
B = 128
AFFINE = dict(degrees=15, scale=(0.9, 1.1), shear=5)
WAYS = {"translate": dict(),
        "flip_shift": dict(flip=True, max_shift=(8, 8)),
        "affine": dict(affine=AFFINE),
        "bilinear": dict(affine=AFFINE, interpolation="bilinear", flip=True)}


def timed(fn, steps):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ways", default=",".join(WAYS))
    args = ap.parse_args()
    names = args.ways.split(",")
    if (args.steps + 20) * B > args.n or set(names) - set(WAYS):
        ap.error("--steps + 20 warm-up steps must fit one epoch of --n examples; --ways of "
                 + ",".join(WAYS))
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(CFG2).cuda().train()
    step = TrainStep(model, B, CFG2["image_shape"])
    snap = step.snapshot()
    g = torch.Generator().manual_seed(1)
    digits = torch.randint(0, 256, (args.n, 1, 28, 28), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (args.n,), generator=g)
    ds = data.ResidentDataset(digits, labels, out_size=(40, 40), device="cuda")
    views = {name: ds.view(shuffle=True, translate=True, seed=2, **WAYS[name]) for name in names}
    ms = {name: [] for name in views}
    for _ in range(args.rounds):        # alternated
        for name, view in views.items():
            step.restore(snap)          # (a live, not a diverged, model)
            view.epoch, view.cursor = 0, 0
            view.desc(0, 0)             # (the epoch's table, outside the window)
            ms[name].append(timed(lambda: step.step_from(view), args.steps))
    for name in views:
        best, worst = min(ms[name]), max(ms[name])
        print(json.dumps(dict(way=name, workload="cfg2 bs128 rmsprop graph replay",
                              ms_per_step=round(best, 4), worst_round_ms=round(worst, 4),
                              spread_us=round(1e3 * (worst - best), 2),
                              images_per_s=round(B / best * 1e3, 1),
                              steps=args.steps, rounds=args.rounds)), flush=True)
    base = min(ms[names[0]])
    print(json.dumps({f"{name}_minus_{names[0]}_us": round(1e3 * (min(ms[name]) - base), 2)
                      for name in names[1:]}))


if __name__ == "__main__":
    main()
