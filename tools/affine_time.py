"""Time cfg-2's training step (MNIST 40x40, 24/24 capsules, B=128, RMSprop, graph replay) fed
by ``step_from`` from a translate-only view and from an ``affine=`` view of the same resident
dataset, HIP-event timed, and print one JSON line per way:

    python tools/affine_time.py [--steps N] [--n EXAMPLES] [--rounds R]

(a) "source": a shuffled, translated view (tools/source_time.py's way (c));
(b) "affine": the same view with ``affine=dict(degrees=15, scale=(0.9, 1.1), shear=5)``: every
    staging and image-layer workgroup resamples its example through the position's
    fixed-point inverse map, read from the epoch's coefficient table;
(c) "affine_identity": ``affine=dict(degrees=0)`` -- the affine code path on the bits of (a).
Each timed window starts at the head of an epoch whose table is already on the device and
ends inside it (``--steps`` + 20 warm-up steps must fit an epoch), so the ways compare the
launches alone; "table_ms" is the once-per-epoch cost, on the host clock: the draws and
matrices of all positions in fp64 torch ops plus the one upload.  Reported per way: the best
and the worst of ``--rounds`` alternated rounds from the same parameter snapshot -- their gap
is the run-to-run spread a difference has to exceed.  The dataset is synthetic uint8 28x28
noise, 60 000 examples."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torch_scae_amd import data, factory  # noqa: E402
from torch_scae_amd.train_step import TrainStep  # noqa: E402

CFG2 = dict(image_shape=(1, 40, 40), n_classes=10, n_part_caps=24, n_obj_caps=24,
            scae_params=dict(reconstruct_alternatives=False))
B = 128
AFFINE = dict(degrees=15, scale=(0.9, 1.1), shear=5)


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
    args = ap.parse_args()
    if (args.steps + 20) * B > args.n:
        ap.error("--steps + 20 warm-up steps must fit one epoch of --n examples")
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(CFG2).cuda().train()
    step = TrainStep(model, B, CFG2["image_shape"])
    snap = step.snapshot()
    g = torch.Generator().manual_seed(1)
    digits = torch.randint(0, 256, (args.n, 1, 28, 28), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (args.n,), generator=g)
    ds = data.ResidentDataset(digits, labels, out_size=(40, 40), device="cuda")
    views = {"source": ds.view(shuffle=True, translate=True, seed=2),
             "affine": ds.view(shuffle=True, translate=True, seed=2, affine=AFFINE),
             "affine_identity": ds.view(shuffle=True, translate=True, seed=2,
                                        affine=dict(degrees=0))}
    table_ms = []
    for epoch in range(3):              # (the host's share of an epoch's first step)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        views["affine"].desc(epoch + 100, 0)
        torch.cuda.synchronize()
        table_ms.append(1e3 * (time.perf_counter() - t0))
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
    print(json.dumps(dict(
        affine_minus_source_us=round(1e3 * (min(ms["affine"]) - min(ms["source"])), 2),
        identity_minus_source_us=round(
            1e3 * (min(ms["affine_identity"]) - min(ms["source"])), 2),
        table_ms=round(min(table_ms), 2), table_positions=args.n,
        table_us_per_step_of_an_epoch=round(1e3 * min(table_ms) / (args.n // B), 2))))


if __name__ == "__main__":
    main()
