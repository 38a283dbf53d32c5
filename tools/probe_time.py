"""Time the linear probe at the cfg-2 feature shapes, (60 000, 24) and (60 000, 48) with 10
classes, on synthetic capsule-like features (no model is trained), HIP-event timed after
warm-up, one JSON line per measurement:

    python tools/probe_time.py [--n 60000] [--reps 3] [--no-host] [--wide]

- ``probe.fit`` (l2 = 1e-3), the same algorithm as a torch-op loop on the device (matmul /
  softmax, one host read of the stop test per iteration: float-atomic-free but bound by
  launches) and ``probe.fit_host`` (fp64 numpy);
- the regularisation path: ``probe.fit`` with R = 8 values of l2 in one grid against eight
  single fits;
- ``--wide`` adds the largest shape, F = 256 with C = 64 (``probe.fit`` alone): with F = 48,
  C = 10 the pair at which a matrix-core form of the two products would be judged.
Iteration counts are printed with every line.  Run it in a process of its own under its own
time limit."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torch_scae_amd import probe  # noqa: E402

L2_PATH = [1e-5, 1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 1e-1, 1.0]


def synthetic(N, F, C, seed=0):
    rng = np.random.default_rng(seed)
    proto = (rng.random((C, F)) < 0.3).astype(np.float64)
    y = rng.integers(0, C, N)
    x = np.clip(proto[y] * rng.random((N, F)) + 0.15 * rng.random((N, F)), 0, 1)
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.int64))


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def torch_fit(x, y, C, l2, mean, scale, L, max_iter=2000, tol=1e-5):
    """The probe's iteration in torch ops on the device, fp32."""
    N, F = x.shape
    Z = torch.cat([(x - mean) * scale, torch.ones(N, 1, device=x.device)], 1)
    Y = torch.nn.functional.one_hot(y, C).to(Z.dtype)
    W = torch.zeros(C, F + 1, device=x.device)
    V, t, step = W.clone(), 1.0, 1.0 / L
    mask = torch.ones(F + 1, device=x.device)
    mask[F] = 0.0
    for it in range(max_iter):
        D = torch.softmax(Z @ V.T, 1) - Y
        g = D.T @ Z / N + l2 * V * mask
        if float(g.abs().max()) <= tol:
            return V, it + 1, True
        Wn = V - step * g
        if float((g.double() * (Wn - W).double()).sum()) > 0:
            t = 1.0
        tn = 0.5 * (1.0 + math.sqrt(1.0 + 4.0 * t * t))
        V = Wn + ((t - 1.0) / tn) * (Wn - W)
        W, t = Wn, tn
    return W, max_iter, False


def line(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--wide", action="store_true")
    args = ap.parse_args()
    shapes = [(24, 10), (48, 10)] + ([(256, 64)] if args.wide else [])
    for F, C in shapes:
        xc, yc = synthetic(args.n, F, C)
        x, y = xc.cuda(), yc.cuda()
        N = x.shape[0]
        ms, res = timed(lambda: probe.fit(x, y, C, l2=1e-3), args.reps)
        line(what="fit", way="probe.fit", N=N, F=F, C=C, ms=round(ms, 3), n_iter=res.n_iter,
             converged=res.converged, us_per_iter=round(1e3 * ms / res.n_iter, 2),
             loss=res.loss)
        if F == 256:
            continue
        p = probe.DeviceProblems(x, y, C, [1e-3], [1e-5], 1)
        mean, scale = p.mean_d, p.scale_d
        ms, out = timed(lambda: torch_fit(x, y, C, 1e-3, mean, scale, p.L[0]), 1)
        line(what="fit", way="torch-op loop", N=N, F=F, C=C, ms=round(ms, 3), n_iter=out[1],
             converged=out[2])
        ms, path = timed(lambda: probe.fit(x, y, C, l2=L2_PATH), args.reps)
        line(what="path", way="probe.fit R=8 in one grid", N=N, F=F, C=C, ms=round(ms, 3),
             n_iter=[r.n_iter for r in path])
        ms, singles = timed(lambda: [probe.fit(x, y, C, l2=v) for v in L2_PATH], args.reps)
        line(what="path", way="eight single probe.fit", N=N, F=F, C=C, ms=round(ms, 3),
             n_iter=[r.n_iter for r in singles])
        if not args.no_host:
            t0 = time.perf_counter()
            res = probe.fit_host(xc, yc, C, l2=1e-3)
            line(what="fit", way="fit_host (fp64 numpy)", N=N, F=F, C=C,
                 ms=round(1e3 * (time.perf_counter() - t0), 1), n_iter=res.n_iter,
                 converged=res.converged, loss=res.loss)


if __name__ == "__main__":
    main()
