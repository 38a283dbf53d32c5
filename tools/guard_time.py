"""Time cfg-2's training step (MNIST 40x40, 24/24 capsules, B=128, RMSprop) with and without
the non-finite guard (TrainStep(nonfinite="skip")) and clipping by global norm, HIP-event
timed as bench.py and tools/clip_time.py time it, and print one JSON line per way:

    python tools/guard_time.py [--steps N] [--rounds R] [--replay graph|launches] [--out FILE]

(a) "unguarded": bench.py's step (the last column sums ride in the RMSprop pass);
(b) "guarded": nonfinite="skip" -- one launch more, the norm launch clipping uses (the last
    column sums ride in it), and the guarded form of the pass with max_norm = +inf;
(c) "clipped": gradient_clip_val at half the first step's norm (clipping active);
(d) "clipped+guarded": both -- the launches of (c), the pass in its guarded form.
The four steps are built from ONE parameter snapshot and replay the same staged batch (every
gradient is finite: the guarded steps are taken); reported: ms per step, the best of
``--rounds`` rounds in which the four ways alternate (each from the snapshot), the library
launches each step records, and the differences in us per step: (b) - (a), (c) - (a),
(d) - (c).  ``--out``: the lines are also written to that file."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replay", default="launches", choices=("graph", "launches"))
    ap.add_argument("--out", default=None)
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
    probe = build(gradient_clip_val=1e30)
    probe(image, label)
    first = float(probe.last_grad_norm())
    del probe
    clip = 0.5 * first
    ways = [("unguarded", build()), ("guarded", build(nonfinite="skip")),
            ("clipped", build(gradient_clip_val=clip)),
            ("clipped+guarded", build(gradient_clip_val=clip, nonfinite="skip"))]
    for _, st in ways:
        st.prepare(image, label)
    torch.cuda.synchronize()
    snaps = {name: st.snapshot() for name, st in ways}
    best, rounds = {}, {name: [] for name, _ in ways}
    for _ in range(args.rounds):        # alternated, the best round of each kept
        for name, st in ways:
            st.restore(snaps[name])
            ms = timed(lambda: st(image, label), args.steps)
            rounds[name].append(round(ms, 4))
            best[name] = min(best.get(name, ms), ms)
    lib = _lib.load()
    lines = []
    for name, st in ways:
        lines.append(dict(
            way=name, workload=f"cfg2 bs128 rmsprop {args.replay} replay",
            ms_per_step=round(best[name], 4), images_per_s=round(B / best[name] * 1e3, 1),
            rounds_ms=rounds[name],
            library_launches=lib.scae_launch_list_size(st._klist) if st._klist else None,
            graph_nodes=st.graph_nodes, steps=args.steps, rounds=args.rounds))
    us = lambda a, b: round(1e3 * (best[a] - best[b]), 2)   # noqa: E731
    guarded = dict(ways)["clipped+guarded"]
    lines.append(dict(
        guarded_minus_unguarded_us=us("guarded", "unguarded"),
        clipped_minus_unguarded_us=us("clipped", "unguarded"),
        clipped_guarded_minus_clipped_us=us("clipped+guarded", "clipped"),
        first_norm=round(first, 4), last_norm=round(float(guarded.last_grad_norm()), 4),
        gradient_clip_val=round(clip, 4),
        nonfinite_steps={name: st.nonfinite_steps() for name, st in ways if st.nonfinite}))
    text = "\n".join(json.dumps(x) for x in lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
