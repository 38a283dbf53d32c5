"""What an epoch's short last batch costs (``drop_last=False`` views, ``TrainStep``'s
remainder step), and print one JSON line per measurement:

    python tools/remainder_time.py [--rounds R] [--steps N] [--skip-bf16]

(a) "first_call": building and capturing the remainder step (three warm-ups and the
    capture) plus its first replay, host wall time, at cfg-2 (B = 128, b = 88 -- 55 000 mod
    128); each round builds it afresh;
(b) "replay": the source-fed remainder step against the full step (prologue gather +
    replay, HIP-event timed over ``--steps`` steps), ms per step;
(c) "epoch": one 55 000-image epoch of ``train_epoch`` with ``drop_last`` True (429 steps)
    and False (429 + the short one), HIP-event timed, each round from one snapshot;
(d) "memory": the device memory the remainder step's capture adds (allocated and reserved,
    MiB), at cfg-2 and at BASELINE configs[2]'s shape in bf16 (B = 1024, b = 728).
Timings are reported as min / median / max over ``--rounds`` alternated rounds."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torch_scae_amd import data, factory  # noqa: E402
from torch_scae_amd.train_step import TrainStep  # noqa: E402

CFG2 = dict(image_shape=(1, 40, 40), n_classes=10, n_part_caps=24, n_obj_caps=24,
            scae_params=dict(reconstruct_alternatives=False))
CFG3 = dict(CFG2, n_part_caps=48, n_obj_caps=64)
N = 55000


def spread(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4),
                max=round(max(xs), 4), n=len(xs))


def events(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def build(cfg, B, **kw):
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(cfg).cuda().train()
    return TrainStep(model, B, cfg["image_shape"], **kw)


def dataset(n):
    g = torch.Generator().manual_seed(1)
    digits = torch.randint(0, 256, (n, 1, 28, 28), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (n,), generator=g)
    return data.ResidentDataset(digits, labels, out_size=(40, 40), device="cuda")


def memory(cfg, B, **kw):
    """MiB the remainder step's capture adds to a step whose own graph is built."""
    b = N % B
    step = build(cfg, B, **kw)
    step.capture()
    torch.cuda.synchronize()
    # (a capture empties the allocator's cache as it starts: empty it for the baseline too)
    torch.cuda.empty_cache()
    a0, r0 = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
    step.remainder_step(b).capture()
    torch.cuda.synchronize()
    a1, r1 = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
    out = dict(B=B, b=b, allocated_mib=round((a1 - a0) / 2 ** 20, 2),
               reserved_mib=round((r1 - r0) / 2 ** 20, 2),
               full_step_reserved_mib=round(r0 / 2 ** 20, 2))
    del step
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--skip-bf16", action="store_true")
    args = ap.parse_args()
    B, b = 128, N % 128
    ds = dataset(N)

    # (a) first call
    step = build(CFG2, B)
    step.capture()
    view = ds.view(shuffle=True, seed=2, drop_last=False)
    done = view.steps_per_epoch(B) * B
    first = []
    for _ in range(args.rounds):
        step._rem = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rem = step.remainder_step(b)
        rem._stage_source(view, 0, done)
        rem._step_staged()
        torch.cuda.synchronize()
        first.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps(dict(what="first_call", workload="cfg2 B=128 b=88 rmsprop graph",
                          ms=spread(first))), flush=True)

    # (b) replay: the short step against the full one, both source-fed
    snap = step.snapshot()

    def full():
        step._stage_source(view, 0, 0)
        step._step_staged()

    def short():
        rem._stage_source(view, 0, done)
        rem._step_staged()
    per = {"full": [], "short": []}
    for _ in range(args.rounds):
        for name, fn in (("full", full), ("short", short)):
            step.restore(snap)
            for _ in range(10):
                fn()
            per[name].append(events(lambda: [fn() for _ in range(args.steps)]) / args.steps)
    print(json.dumps(dict(what="replay", workload="cfg2 source-fed, graph replay",
                          full_ms=spread(per["full"]), short_ms=spread(per["short"]),
                          steps=args.steps)), flush=True)

    # (c) one epoch, drop_last True / False
    views = {True: ds.view(shuffle=True, seed=2), False: ds.view(shuffle=True, seed=2,
                                                                  drop_last=False)}
    ep = {True: [], False: []}
    for _ in range(args.rounds):
        for drop in (True, False):
            step.restore(snap)
            v = views[drop]
            ep[drop].append(events(lambda: step.train_epoch(v)))
    print(json.dumps(dict(what="epoch", workload=f"cfg2 n={N} train_epoch",
                          steps_drop_last=views[True].steps_in_epoch(B),
                          steps_keep_last=views[False].steps_in_epoch(B),
                          drop_last_ms=spread(ep[True]), keep_last_ms=spread(ep[False]),
                          median_extra_ms=round(statistics.median(ep[False]) -
                                                statistics.median(ep[True]), 4))), flush=True)
    del step, rem
    torch.cuda.empty_cache()

    # (d) memory
    print(json.dumps(dict(what="memory", workload="cfg2 fp32", **memory(CFG2, 128))),
          flush=True)
    if not args.skip_bf16:
        print(json.dumps(dict(what="memory", workload="configs[2] shape bf16",
                              **memory(CFG3, 1024, autocast_dtype=torch.bfloat16))),
              flush=True)


if __name__ == "__main__":
    main()
