"""Time cfg-2's training step (MNIST 40x40, 24/24 capsules, B=128, RMSprop, graph replay) fed
from a shuffled, translated ResidentDataset view, with and without its log, HIP-event timed,
and print one JSON line per way:

    python tools/train_log_time.py [--steps N] [--rounds R]

(a) "step_from": ``step.step_from(view)``, no log (bench.py's step, fed from the view);
(b) "step_from_logged": the same on a ``TrainStep(log_steps=1024)``: the log's row written by
    the loss tail's combine workgroup, the epoch sums added;
(c) "training_step": today's way to get the log -- ``view.batch`` (the view's CPU path) and
    ``training_step(image, label)`` (host-to-device copy, torch kernels for the accuracy and
    the log copies in the captured graph);
(c') "training_step_device": ``training_step`` on batches of the same view gathered on the
    device ahead of time: (c) without the CPU feed.
Each way has its own step built from ONE parameter snapshot; reported: ms per step, the best
of ``--rounds`` alternated rounds (each from the snapshot), the captured graph's nodes /
kernel nodes / library launches, and (b) - (a), (c) - (a) in us per step."""
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
    sd = {k: v.clone() for k, v in factory.make_scae(CFG2).state_dict().items()}

    def build(**kw):
        model = factory.make_scae(CFG2)
        model.load_state_dict(sd)
        return TrainStep(model.cuda().train(), B, CFG2["image_shape"], **kw)
    g = torch.Generator().manual_seed(1)
    digits = torch.randint(0, 256, (args.n, 1, 28, 28), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (args.n,), generator=g)
    ds = data.ResidentDataset(digits, labels, out_size=(40, 40), device="cuda")
    plain, logged, today, today_dev = build(), build(log_steps=1024), build(), build()
    views = {name: ds.view(shuffle=True, translate=True, seed=2)
             for name in ("a", "b", "c")}
    pre = ds.view(shuffle=True, translate=True, seed=2)
    pre_b = [pre.gather(B, step=s) for s in range(64)]
    k = [0]

    def cpu_batch(view):
        epoch, pos = view.take_step(B)
        return view.batch(epoch, pos // B, B)

    def today_way():
        today.training_step(*cpu_batch(views["c"]))

    def today_device():
        k[0] = (k[0] + 1) % 64
        today_dev.training_step(*pre_b[k[0]])
    ways = [("step_from", plain, lambda: plain.step_from(views["a"])),
            ("step_from_logged", logged, lambda: logged.step_from(views["b"])),
            ("training_step", today, today_way),
            ("training_step_device", today_dev, today_device)]
    # capture every step first (training_step builds its graph with the log), then snapshot
    plain.step_from(views["a"])
    logged.step_from(views["b"])
    today_way()
    today_device()
    torch.cuda.synchronize()
    snaps = {name: st.snapshot() for name, st, _ in ways}
    best = {}
    for _ in range(args.rounds):        # alternated, the best round of each kept
        for name, st, fn in ways:
            st.restore(snaps[name])     # (a live, not a diverged, model)
            ms = timed(fn, args.steps)
            best[name] = min(best.get(name, ms), ms)
    # the captured graphs' make-up: the same steps once more under replay="launches" (which
    # keeps the graph readable), one step each
    counts = {}
    for name, kw, fn in (("step_from", {}, lambda st: st.step_from(views["a"])),
                         ("step_from_logged", dict(log_steps=1024),
                          lambda st: st.step_from(views["b"])),
                         ("training_step", {}, lambda st: st.training_step(*pre_b[0])),
                         ("training_step_device", {},
                          lambda st: st.training_step(*pre_b[0]))):
        st = build(replay="launches", **kw)
        fn(st)
        torch.cuda.synchronize()
        counts[name] = dict(zip(("graph_nodes", "kernel_nodes", "library_launches"),
                                st.graph_nodes or (None,) * 3),
                            launch_list_taken=bool(st._klist))
        del st
    for name, st, _ in ways:
        print(json.dumps(dict(way=name, workload="cfg2 bs128 rmsprop graph replay",
                              ms_per_step=round(best[name], 4),
                              images_per_s=round(B / best[name] * 1e3, 1),
                              **counts[name], steps=args.steps,
                              rounds=args.rounds)), flush=True)
    print(json.dumps(dict(
        logged_minus_plain_us=round(1e3 * (best["step_from_logged"] - best["step_from"]), 2),
        training_step_minus_plain_us=round(1e3 * (best["training_step"] - best["step_from"]),
                                           2),
        training_step_device_minus_plain_us=round(
            1e3 * (best["training_step_device"] - best["step_from"]), 2),
        log_rows=int(logged.train_log.step))))


if __name__ == "__main__":
    main()
