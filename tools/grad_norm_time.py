"""Time cfg-2's training step (MNIST 40x40, 24/24 capsules, B=128, RMSprop) with and without
tracked gradient norms (TrainStep(track_grad_norm=2)), without and with clipping by global
norm, HIP-event timed as bench.py times a step, and print one JSON line per way:

    python tools/grad_norm_time.py [--steps N] [--rounds R] [--replay graph|launches]

(a) "untracked" / "tracked": bench.py's step against the same step with the norms: the last
    column sums launch on their own instead of riding in the RMSprop pass, then the two launches
    of scae_segment_norms_f32;
(b) "clipped" / "clipped tracked": gradient_clip_val at half the first step's norm; the column
    sums keep riding in the clip's norm launch, the two launches follow it.
All four steps are built from ONE parameter snapshot and replay the same staged batch;
reported: ms per step, the best of ``--rounds`` alternated rounds (each from the snapshot), the
library launches each step records, tracked - untracked in us per step for (a) and (b), and
the two new launches' own duration: scae_segment_norms_f32 on the step's flat gradient, issued
back to back ``--steps`` times between two events (us per call, both launches)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torch_scae_amd import _lib, factory  # noqa: E402
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replay", default="launches", choices=("graph", "launches"))
    args = ap.parse_args()
    np.random.seed(0)
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in factory.make_scae(CFG2).state_dict().items()}
    g = torch.Generator().manual_seed(1)
    image = torch.rand(B, *CFG2["image_shape"], generator=g).cuda()
    label = torch.randint(0, 10, (B,), generator=g).cuda()

    def build(**kw):
        model = factory.make_scae(CFG2)
        model.load_state_dict(sd)
        return TrainStep(model.cuda().train(), B, CFG2["image_shape"], lr=3e-5,
                         replay=args.replay, **kw)
    probe = build(track_grad_norm=2)
    probe(image, label)
    first = float(probe.last_grad_norm())
    del probe
    clip = 0.5 * first
    ways = [("untracked", build()), ("tracked", build(track_grad_norm=2)),
            ("clipped", build(gradient_clip_val=clip)),
            ("clipped tracked", build(gradient_clip_val=clip, track_grad_norm=2))]
    for _, st in ways:
        st.prepare(image, label)
    torch.cuda.synchronize()
    snaps = {name: st.snapshot() for name, st in ways}
    best = {}
    for _ in range(args.rounds):        # alternated, the best round of each kept
        for name, st in ways:
            st.restore(snaps[name])
            ms = timed(lambda: st(image, label), args.steps)
            best[name] = min(best.get(name, ms), ms)
    lib = _lib.load()
    for name, st in ways:
        print(json.dumps(dict(
            way=name, workload=f"cfg2 bs128 rmsprop {args.replay} replay",
            ms_per_step=round(best[name], 4), images_per_s=round(B / best[name] * 1e3, 1),
            library_launches=lib.scae_launch_list_size(st._klist) if st._klist else None,
            graph_nodes=st.graph_nodes, steps=args.steps, rounds=args.rounds)), flush=True)
    tracked = ways[1][1]
    trk = tracked.grad_norms
    row = torch.empty(1, len(trk.segments) + 1, device="cuda")
    alone = timed(lambda: trk.launch(tracked.flat.flat_grad, None, 1.0, into=row), args.steps)
    print(json.dumps(dict(
        tracked_minus_untracked_us=round(1e3 * (best["tracked"] - best["untracked"]), 2),
        clipped_tracked_minus_clipped_us=round(
            1e3 * (best["clipped tracked"] - best["clipped"]), 2),
        norm_launches_alone_us=round(1e3 * alone, 2), segments=len(trk.segments),
        chunks=int(trk.tables[0].shape[0]), workgroups=int(trk.tables[1].numel()) - 1,
        total_norm=round(float(tracked.last_grad_norm()), 4), first_norm=round(first, 4))))


if __name__ == "__main__":
    main()
