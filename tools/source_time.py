"""Time cfg-2's training step (MNIST 40x40, 24/24 capsules, B=128, RMSprop, graph replay) fed
three ways, HIP-event timed, and print one JSON line per way:

    python tools/source_time.py [--steps N] [--n EXAMPLES]

(a) "staged": bench.py's pre-staged device batches -- ``step(image, label)`` on fp32 batches
    already on the device (the prologue copies 800 KB of fp32 per step);
(b) "aten": today's way to train on data -- index a device-resident uint8 dataset,
    ``data.pad_and_translate`` (ATen ops, host RNG and a host-to-device copy), ``step``;
(c) "source": ``step.step_from(view)`` on a shuffled, translated ResidentDataset view: the
    batch gathered in the step's prologue launch (100 KB of uint8 read per step);
(a') "staged_view": (a) on 64 batches of that same view gathered ahead of time -- the step's
    time depends on the data it trains on, so (c) - (a') is the cost of the feed itself.
Reported: ms per step, images/s, each way's best of ``--rounds`` alternated rounds from the
same parameter snapshot.  The dataset is synthetic uint8 28x28 noise, 60 000 examples."""
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
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(CFG2).cuda().train()
    step = TrainStep(model, B, CFG2["image_shape"])
    snap = step.snapshot()
    g = torch.Generator().manual_seed(1)
    digits = torch.randint(0, 256, (args.n, 1, 28, 28), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (args.n,), generator=g)
    ds = data.ResidentDataset(digits, labels, out_size=(40, 40), device="cuda")
    view = ds.view(shuffle=True, translate=True, seed=2)
    staged_i = torch.rand(8, B, 1, 40, 40, generator=g).cuda()
    staged_l = torch.randint(0, 10, (8, B), generator=g).cuda()
    pre = ds.view(shuffle=True, translate=True, seed=2)
    pre_b = [pre.gather(B, step=s) for s in range(64)]
    k = [0]

    def staged_view():
        k[0] = (k[0] + 1) % 64
        step(*pre_b[k[0]])

    def staged():
        k[0] = (k[0] + 1) % 8
        step(staged_i[k[0]], staged_l[k[0]])

    def aten():
        rows = torch.randint(0, ds.n, (B,), device="cuda")
        step(data.pad_and_translate(ds.images[rows], (40, 40)), ds.labels[rows])

    def source():
        step.step_from(view)
    ways = [("staged", staged), ("staged_view", staged_view), ("aten", aten),
            ("source", source)]
    best = {}
    for _ in range(args.rounds):        # alternated, the best round of each kept
        for name, fn in ways:
            step.restore(snap)          # (a live, not a diverged, model)
            ms = timed(fn, args.steps)
            best[name] = min(best.get(name, ms), ms)
    for name, _ in ways:
        print(json.dumps(dict(way=name, workload="cfg2 bs128 rmsprop graph replay",
                              ms_per_step=round(best[name], 4),
                              images_per_s=round(B / best[name] * 1e3, 1),
                              steps=args.steps, rounds=args.rounds)), flush=True)
    print(json.dumps(dict(
        source_minus_staged_us=round(1e3 * (best["source"] - best["staged"]), 2),
        source_minus_staged_view_us=round(1e3 * (best["source"] - best["staged_view"]), 2))))


if __name__ == "__main__":
    main()
