"""The optimisers' passes alone at cfg-2's flat size (2 414 879 parameters) and cfg-2's
replayed step with each optimiser, HIP-event timed.

    python tools/optimizer_time.py [reps]

Launch alone: RMSprop (scae_rmsprop_step_f32 / _sums_), Adam and RAdam
(scae_flat_opt_step_f32 / _sums_), plain and with the step's last column sums riding (a
synthetic job table of the riding test's shapes), and LookAhead on a non-sync and on a
sync step; back-to-back launches, the mean per launch, GB/s from the bytes the pass must
move (28 per parameter, 36 on a LookAhead sync step).  Replayed step: bench.py's cfg-2
step built with each optimiser, graph and launch-list replay, the mean over `reps`
steps on the bench's synthetic batches."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from torch_scae_amd import _lib  # noqa: E402

N = 2414879
P = ctypes.c_void_p
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200


def timed(fn, n=reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def launches_alone():
    g = torch.Generator().manual_seed(0)
    p, grad, m, slow = (torch.randn(N, generator=g).cuda() * 0.1 for _ in range(4))
    v = torch.rand(N, generator=g).cuda()
    lr = torch.full((1,), 3e-5, device="cuda")
    state = torch.zeros(_lib.FLAT_OPT_STATE_INTS, dtype=torch.int32, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)
    # a job table like the step's last column sums (destinations inside the gradient)
    parts = [torch.randn(22, 9 * 40, generator=g).cuda(), torch.randn(128, 5 * 12, generator=g).cuda(),
             torch.randn(7, 333, generator=g).cuda(), torch.randn(300, 6, generator=g).cuda()]
    layout = [(1, [(0, 360, -40, 360)]), (3001, [(0, 5, 12, 50), (5, 12, 12, 70)]),
              (7002, [(0, 100, 0, 100), (120, 333, 0, 213)]), (N - 10, [(0, 6, 0, 6)])]
    jobs, keep = (_lib.SumJob * len(parts))(), []
    for job, part, (off, segs) in zip(jobs, parts, layout):
        arr = (_lib.SumSegment * len(segs))()
        pos = off
        for a, (b, e, per, length) in zip(arr, segs):
            a.dst, a.begin, a.end, a.period = grad.data_ptr() + 4 * pos, b, e, per
            pos += length
        keep.append(arr)
        job.src, job.rows, job.cols = part.data_ptr(), part.shape[0], part.shape[1]
        job.segments, job.n_segments = arr, len(segs)
    eps = 1e-2 / 128 ** 2
    ptrs = (P(p.data_ptr()), P(grad.data_ptr()), P(m.data_ptr()), P(v.data_ptr()))

    def rms(sums):
        if sums:
            return lambda: _lib.call("scae_rmsprop_sums_step_f32", *ptrs[:2], ptrs[3], ptrs[2], N,
                                     3e-5, P(lr.data_ptr()),
                                     0.99, eps, 0.9, 1.0, jobs, len(parts), st)
        return lambda: _lib.call("scae_rmsprop_step_f32", *ptrs[:2], ptrs[3], ptrs[2], N, 3e-5,
                                 P(lr.data_ptr()), 0.99, eps, 0.9, 0.0, 1.0, st)

    def opt(kind, sums, k=0, advance=1):
        common = (*ptrs, P(slow.data_ptr()), N, P(lr.data_ptr()), P(state.data_ptr()), kind,
                  0.9, 0.999, eps)
        if sums:
            return lambda: _lib.call("scae_flat_opt_sums_step_f32", *common, 1.0, k, 0.5, jobs,
                                     len(parts), st)
        return lambda: _lib.call("scae_flat_opt_step_f32", *common, 0.0, 1.0, k, 0.5, advance, st)

    rows = [("RMSprop", rms(False), 28), ("RMSprop riding", rms(True), 28)]
    for name, kind in (("Adam", 0), ("RAdam", 1)):
        rows += [(name, opt(kind, False), 28), (name + " riding", opt(kind, True), 28)]
    # what the step count's advance costs: the same pass with no workgroup arriving
    rows += [("Adam, count not advanced", opt(0, False, advance=0), 28)]
    # LookAhead: k = 1 makes every step a sync (slow weights made), a huge k none
    rows += [("Adam + LookAhead, non-sync step", opt(0, False, 1 << 30), 28),
             ("Adam + LookAhead, sync step", opt(0, False, 1), 36),
             ("Adam + LookAhead riding, sync step", opt(0, True, 1), 36)]
    print(f"launch alone, n = {N}:")
    for name, fn, bytes_per in rows:
        us = timed(fn)
        print(f"  {name:38s} {us:7.2f} us  {bytes_per * N / us / 1e3:7.0f} GB/s")


def replayed_steps():
    import bench
    cfg = bench.CONFIGS["mnist_24_24_bs128"]
    dev = torch.device("cuda", 0)
    images, labels = bench.synthetic_batches(cfg, dev, 1000)
    print(f"cfg-2 replayed step (B = {cfg['batch']}), mean over {reps} steps:")
    for replay in ("graph", "launches"):
        for kind, la in (("rmsprop", False), ("adam", False), ("radam", False),
                         ("adam", True)):
            torch.manual_seed(1234)
            step = bench.make_step(cfg, dev, optimizer=kind, look_ahead=la, replay=replay)
            step.capture()
            i = [0]

            def one():
                step(images[i[0] % 8], labels[i[0] % 8])
                i[0] += 1
            us = timed(one)
            name = kind + (" + LookAhead" if la else "")
            print(f"  {replay:8s} {name:18s} {us / 1e3:.4f} ms/step")
            del step
            torch.cuda.empty_cache()


if __name__ == "__main__":
    launches_alone()
    replayed_steps()
