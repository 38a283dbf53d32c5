"""Time t-SNE (torch_scae_amd/embed.py, csrc/tsne.hip) on synthetic (N, 24) capsule-like features
with 10 classes, at N = 10 000 and N = 32 768, HIP-event timed after a warm-up, one JSON line:

    python tools/tsne_time.py [--n 10000 32768] [--iters 1000] [--host-n 2000] [--no-host]
                              [--neighbors auto|K]

- ``embed.affinities``; ``embed.tsne`` for ``--iters`` iterations (affinities and the PCA
  initialisation included) and the iterations alone; the same iteration as a torch-op loop on the
  device (dense (N, N) temporaries, no host read), ``--torch-iters`` of them, scaled per iteration;
- ``embed.tsne_host`` (fp64 numpy) at a size it finishes, ``--host-n``;
- scikit-learn's ``TSNE(method="exact")`` at ``--host-n`` and ``"barnes_hut"`` at the first N, if
  ``sklearn`` imports; silent otherwise.
- with ``--neighbors`` the sparse form (csrc/tsne_sparse.hip) instead: ``embed.affinities_knn``,
  ``embed.tsne(neighbors=...)`` and its iterations alone, no torch loop; and, at the first N when
  the dense form takes it, the trustworthiness at k = 12 of the sparse and the dense embedding
  from the same initialisation ("quality").  The split of an iteration into its launches is a
  kernel trace's to give: run ``--child tsne`` under a profiler;
Every GPU measurement runs in a child process of its own under its own time limit; a child that
fails or runs out of time leaves an "error" entry and ends the measurements."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402


def synthetic(N, F=24, C=10, seed=0):
    rng = np.random.default_rng(seed)
    proto = (rng.random((C, F)) < 0.3).astype(np.float64)
    y = rng.integers(0, C, N)
    x = np.clip(proto[y] * rng.random((N, F)) + 0.15 * rng.random((N, F)), 0, 1)
    return x.astype(np.float32), y


def timed(fn, reps=1, warm=1):
    import torch
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


def torch_iteration(P, Y, vel, gains, ex, mom, lr):
    """The rules' iteration in torch ops, fp32 (float sums in torch's own order)."""
    import torch
    dy = Y[:, None, :] - Y[None, :, :]
    q = 1.0 / (1.0 + (dy * dy).sum(-1))
    q.fill_diagonal_(0.0)
    Z = q.sum(dtype=torch.float64)
    att = ((P * q)[:, :, None] * dy).sum(1)
    rep = ((q * q)[:, :, None] * dy).sum(1)
    g = 4.0 * (ex * att - rep * (1.0 / Z).float())
    gains = torch.clamp_min(torch.where(g * vel < 0, gains + 0.2, gains * 0.8), 0.01)
    vel = mom * vel - lr * gains * g
    Y = Y + vel
    return Y - Y.mean(0), vel, gains


def child(what, N, iters, nb=None):
    import torch
    from torch_scae_amd import embed
    x = torch.from_numpy(synthetic(N)[0]).cuda()
    out = dict(what=what, N=N)
    if nb is not None:
        out.update(neighbors=nb)
    if what == "affinities" and nb is not None:
        ms, res = timed(lambda: embed.affinities_knn(x, 30.0, nb))
        out.update(ms=round(ms, 3), nnz=res[1].numel())
    elif what == "tsne" and nb is not None:
        ms, res = timed(lambda: embed.tsne(x, n_iter=iters, neighbors=nb))
        csr, _, plogp = embed._affinities_knn_device(x, 30.0, embed._check_sparse(x, 30.0, nb))
        p = embed._SparseProblem(csr, plogp, res.y, iters, 12.0, 250, max(N / 48.0, 50.0), 50)
        ms_it, _ = timed(lambda: p.run(0, iters), warm=0)
        out.update(ms=round(ms, 3), iterations=iters, kl=res.kl,
                   iterations_ms=round(ms_it, 3), us_per_iteration=round(1e3 * ms_it / iters, 2))
    elif what == "quality":
        from torch_scae_amd.neighbors import trustworthiness
        for name, arg in (("sparse", nb), ("dense", None)):
            res = embed.tsne(x, n_iter=iters, neighbors=arg)
            out[name] = dict(kl=res.kl, trustworthiness_12=trustworthiness(x, res.y, 12))
    elif what == "affinities":
        ms, _ = timed(lambda: embed.affinities(x, 30.0))
        out.update(ms=round(ms, 3))
    elif what == "tsne":
        ms, res = timed(lambda: embed.tsne(x, n_iter=iters))
        P, _, plogp = embed._affinities_device(x, 30.0)
        p = embed._TsneProblem(P, plogp, res.y, iters, 12.0, 250, max(N / 48.0, 50.0), 50)
        ms_it, _ = timed(lambda: p.run(0, iters), warm=0)
        out.update(ms=round(ms, 3), iterations=iters, kl=res.kl,
                   iterations_ms=round(ms_it, 3), us_per_iteration=round(1e3 * ms_it / iters, 2))
    elif what == "torch":
        P, _, _ = embed._affinities_device(x, 30.0)
        Y = embed.init_pca(x).cuda()
        state = [Y, torch.zeros_like(Y), torch.ones_like(Y)]

        def loop():
            for _ in range(iters):
                state[:] = torch_iteration(P, *state, 12.0, 0.5, max(N / 48.0, 50.0))
        ms, _ = timed(loop)
        out.update(iterations=iters, us_per_iteration=round(1e3 * ms / iters, 2))
    print(json.dumps(out), flush=True)


def run_child(what, N, iters, limit, nb=None):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
           "--child", what, "--n", str(N), "--iters", str(iters)]
    if nb is not None:
        cmd += ["--neighbors", str(nb)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return dict(what=what, N=N, error=f"exit {r.returncode}"), False
    return json.loads(r.stdout.strip().splitlines()[-1]), True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10000, 32768])
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--torch-iters", type=int, default=20)
    ap.add_argument("--host-n", type=int, default=2000)
    ap.add_argument("--host-iters", type=int, default=1000)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--neighbors", type=lambda v: v if v == "auto" else int(v))
    ap.add_argument("--child")
    args = ap.parse_args()
    nb = args.neighbors
    if args.child:
        return child(args.child, args.n[0], args.iters, nb)
    results, ok = [], True
    for N in args.n:
        for what, iters in (("affinities", 0), ("tsne", args.iters), ("torch", args.torch_iters)):
            if what == "torch" and (N > 16384 or nb is not None):
                continue                      # (its (N, N, 2) temporaries: 8 GiB each at 32 768)
            if ok:
                r, ok = run_child(what, N, iters, args.limit, nb)
                results.append(r)
    if ok and nb is not None and args.n[0] <= 32768:
        r, ok = run_child("quality", args.n[0], args.iters, args.limit, nb)
        results.append(r)
    if nb is not None:
        args.no_host = True
    if not args.no_host:
        import torch
        from torch_scae_amd import embed
        xh = torch.from_numpy(synthetic(args.host_n)[0])
        t0 = time.perf_counter()
        res = embed.tsne_host(xh, n_iter=args.host_iters)
        results.append(dict(what="tsne_host (fp64 numpy)", N=args.host_n,
                            iterations=args.host_iters, kl=res.kl,
                            ms=round(1e3 * (time.perf_counter() - t0), 1)))
        try:
            from sklearn.manifold import TSNE
        except ImportError:
            TSNE = None
        if TSNE is not None:
            for method, N in (("exact", args.host_n), ("barnes_hut", args.n[0])):
                t0 = time.perf_counter()
                TSNE(method=method, init="pca", perplexity=30.0).fit_transform(synthetic(N)[0])
                results.append(dict(what=f"sklearn TSNE {method}", N=N,
                                    ms=round(1e3 * (time.perf_counter() - t0), 1)))
    print(json.dumps(dict(tool="tsne_time", results=results)), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
