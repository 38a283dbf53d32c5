"""Time cfg-2's training step (MNIST 40x40, 24/24 capsules, B=128, RMSprop) with gradient
accumulation (TrainStep(accumulate_grad_batches=4)), HIP-event timed, and print one JSON line
per way:

    python tools/accumulate_time.py [--steps N] [--rounds R] [--replay graph|launches]

(a) "k1": bench.py's step (the last column sums ride in the RMSprop pass);
(b) "accumulate form": the k = 4 step on a batch that does not end its group -- the
    accumulate pass (acc += g, the last column sums riding in it) in the optimiser's place;
(c) "update form": the k = 4 step on a group's last batch -- the accumulate form of the
    RMSprop pass (g = acc + g, acc -> 0);
(d) "k4": the k = 4 step as training runs it, three (b) and one (c) per group.
Every way is a call ``step(image, label)`` -- staging launch, host bookkeeping, replay -- so the
ways are timed alike; (b) and (c) set the step's count of pending batches before each call so
that it picks that form.  All steps are built from ONE parameter snapshot and replay the same
staged batch.  Reported: ms per batch, the best of ``--rounds`` alternated rounds, the
snapshot put back every 20 batches inside the timed region (as bench.py does); the host's
time to issue one call (when it exceeds the device time per batch
the loop is host-bound); the device span of one replay of each captured form
and each launch's time in it (scae_launch_list_timeline: an event in front of and
behind every launch); the library
launches each form records; the differences to (a) in us; and the device memory the second
captured form adds (it shares the first form's pool).  The new kernels' own times: run this
under ``rocprofv3 --kernel-trace --stats -- python tools/accumulate_time.py --steps 100
--rounds 1`` (accumulate_sums_kernel, rmsprop_acc_sums_kernel)."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torch_scae_amd import _lib, factory  # noqa: E402
from torch_scae_amd.train_step import TrainStep  # noqa: E402

CFG2 = dict(image_shape=(1, 40, 40), n_classes=10, n_part_caps=24, n_obj_caps=24,
            scae_params=dict(reconstruct_alternatives=False))
B = 128


def timed(fn, steps, reset):
    """-> (device ms per call, host us to issue one call).  ``reset()`` (the snapshot put
    back) runs before every 20 calls, inside the timed region as in bench.py: the steps then
    stay within 20 optimiser updates of the snapshot, where every capsule is live.  Left to
    train on a fixed noise batch the capsules switch off within a few hundred updates and the
    likelihood backward skips them, so a way that updates more often would run faster."""
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for i in range(steps):
        if i % 20 == 0:
            reset()
        fn()
    host = (time.perf_counter() - t0) / steps * 1e6
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, host


def device_span_us(lib, st):
    """-> (device span of one replay of the step's launch list, [(launch, us)]): the best of 7
    replays (first launch's start to the last one's end), an event on each side of every
    launch."""
    klist = st._klist
    n = lib.scae_launch_list_size(klist)
    out = (ctypes.c_float * (2 * n))()
    best = None
    for _ in range(7):
        if lib.scae_launch_list_timeline(
                klist, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), None, out,
                2 * n) != 0:
            return None, None
        t = list(out)
        if best is None or t[-1] - t[0] < best[-1] - best[0]:
            best = t
    names = [getattr(fn, "__name__", "?") for fn, _, _ in st._launches] \
        if st._launches and len(st._launches) == n else ["?"] * n
    return round(best[-1] - best[0], 2), [(names[i], round(best[2 * i + 1] - best[2 * i], 2))
                                          for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
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
    k1, k4 = build(), build(accumulate_grad_batches=4)
    k1.prepare(image, label)
    k4.prepare(image, label)            # (the update form)
    torch.cuda.synchronize()
    mem0 = torch.cuda.memory_reserved()
    k4._use_form("acc")
    k4.capture()                        # the second form
    torch.cuda.synchronize()
    added = torch.cuda.memory_reserved() - mem0
    k4._use_form("update")

    def form(pending):
        def run():
            k4._acc_state["pending"] = pending    # 0: the accumulate form, 3: the update form
            k4(image, label)
        return run
    ways = [("k1", k1, lambda: k1(image, label)), ("accumulate form", k4, form(0)),
            ("update form", k4, form(3)), ("k4", k4, lambda: k4(image, label))]
    snaps = {name: st.snapshot() for name, st, _ in ways}
    best, host = {}, {}
    for _ in range(args.rounds):        # alternated, the best round of each kept
        for name, st, fn in ways:
            ms, us = timed(fn, args.steps, lambda: st.restore(snaps[name]))
            if ms < best.get(name, float("inf")):
                best[name], host[name] = ms, us
    lib = _lib.load()

    def launches(st, name):
        st.restore(snaps["k1" if st is k1 else "k4"])     # (live capsules, as timed)
        st._use_form(name)
        if not st._klist:
            return None, None, None
        return (lib.scae_launch_list_size(st._klist),) + device_span_us(lib, st)
    counts = {"k1": launches(k1, "update"), "accumulate form": launches(k4, "acc"),
              "update form": launches(k4, "update"), "k4": (None, None, None)}
    for name, st, _ in ways:
        print(json.dumps(dict(
            way=name, workload=f"cfg2 bs128 rmsprop {args.replay} replay",
            ms_per_batch=round(best[name], 4), images_per_s=round(B / best[name] * 1e3, 1),
            host_us_per_call=round(host[name], 1), library_launches=counts[name][0],
            device_span_us=counts[name][1], steps=args.steps, rounds=args.rounds,
            launch_us=counts[name][2])), flush=True)
    print(json.dumps({f"{name}_minus_k1_us": round(1e3 * (best[name] - best["k1"]), 2)
                      for name in ("accumulate form", "update form", "k4")}
                     | dict(second_form_bytes=added)))


if __name__ == "__main__":
    main()
