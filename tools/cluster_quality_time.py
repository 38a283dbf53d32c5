"""Time the cluster-quality tools (torch_scae_amd/cluster_quality.py, csrc/cluster_quality.hip) on
synthetic capsule-like features with 10 classes, HIP-event timed after a warm-up, one JSON line:

    python tools/cluster_quality_time.py [--sizes 10000 60000] [--k 10] [--select-n 10000]
                                         [--sklearn-sizes 60000 30000 10000] [--no-sklearn]

- ``cluster_quality.silhouette`` at (N, 24) for every N of ``--sizes`` under the generating
  classes as labels (the sort, both launches and the one read), and ``dispersion``;
- the same quantity in torch ops on the device: ``torch.cdist`` over chunks of ``--torch-rows``
  rows times a one-hot (N, k) matrix, fp32 sums in torch's own order, so its values are compared
  only loosely and its time is what counts;
- ``select_k`` over k = 2 .. 20 at N = ``--select-n`` (``--n-init`` restarts a fit);
- scikit-learn's ``silhouette_samples`` on the CPU (skipped if it does not import): the first N
  of ``--sklearn-sizes`` that finishes within ``--sklearn-limit`` seconds.
Every measurement runs in a child process of its own under its own time limit; a GPU child that
fails or runs out of time leaves an "error" entry and ends the GPU measurements."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tools.tsne_time import synthetic, timed  # noqa: E402


def torch_silhouette(x, lab, k, rows):
    import torch
    N = x.shape[0]
    onehot = torch.nn.functional.one_hot(lab, k).to(x.dtype)
    n = onehot.sum(0)
    out = []
    for lo in range(0, N, rows):
        D = torch.cdist(x[lo:lo + rows], x) @ onehot                 # (rows, k) sums
        own = onehot[lo:lo + rows].bool()
        a = D[own] / (n[lab[lo:lo + rows]] - 1).clamp_min(1)
        b = (D / n).masked_fill(own | (n == 0), float("inf")).min(1).values
        out.append(torch.where(n[lab[lo:lo + rows]] > 1, (b - a) / torch.maximum(a, b), 0 * a))
    return torch.cat(out).nan_to_num(0.0)


def child(what, args):
    N = args.n
    xs, ys = synthetic(N, seed=0)
    if what == "sklearn":
        from sklearn.metrics import silhouette_samples
        t0 = time.perf_counter()
        s = silhouette_samples(xs.astype("float64"), ys)
        print(json.dumps(dict(what="sklearn silhouette_samples (CPU)", N=N, F=xs.shape[1],
                              k=args.k, ms=round(1e3 * (time.perf_counter() - t0), 1),
                              score=float(s.mean()))), flush=True)
        return 0
    import torch
    from torch_scae_amd import cluster_quality as Q
    x, lab = torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda()
    out = dict(what=what, N=N, F=x.shape[1], k=args.k)
    if what == "silhouette":
        ms, res = timed(lambda: Q.silhouette(x, lab, args.k), reps=3)
        out.update(ms=round(ms, 3), score=res.score)
    elif what == "dispersion":
        ms, res = timed(lambda: Q.dispersion(x, lab, args.k), reps=3)
        out.update(ms=round(ms, 3), calinski_harabasz=res.calinski_harabasz,
                   davies_bouldin=res.davies_bouldin)
    elif what == "torch":
        ms, s = timed(lambda: torch_silhouette(x, lab, args.k, args.torch_rows), reps=3)
        ours = Q.silhouette(x, lab, args.k).values
        out.update(ms=round(ms, 3), rows_per_chunk=args.torch_rows,
                   max_abs_difference_to_silhouette=float((s.double() - ours).abs().max()))
    elif what == "select_k":
        ks = range(2, 21)
        ms, res = timed(lambda: Q.select_k(x, ks, n_init=args.n_init), reps=1)
        out = dict(what=what, N=N, F=x.shape[1], ks=[2, 20], n_init=args.n_init,
                   ms=round(ms, 1), chosen=res.k)
    print(json.dumps(out), flush=True)


def run_child(what, args, n, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
           "--child", what, "--n", str(n), "--k", str(args.k), "--n-init", str(args.n_init),
           "--torch-rows", str(args.torch_rows)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return dict(what=what, N=n, error=f"exit {r.returncode}"), False
    return json.loads(r.stdout.strip().splitlines()[-1]), True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[10000, 60000])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--select-n", type=int, default=10000)
    ap.add_argument("--n-init", type=int, default=3)
    ap.add_argument("--torch-rows", type=int, default=2048)
    ap.add_argument("--sklearn-sizes", type=int, nargs="*", default=[60000, 30000, 10000])
    ap.add_argument("--sklearn-limit", type=int, default=90)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--child")
    ap.add_argument("--n", type=int, default=10000)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args)
    results, ok = [], True
    if not args.no_gpu:
        jobs = [(w, n) for n in args.sizes for w in ("silhouette", "dispersion", "torch")]
        for what, n in jobs + [("select_k", args.select_n)]:
            if ok:
                r, ok = run_child(what, args, n, args.limit)
                results.append(r)
    if not args.no_sklearn:
        try:
            import sklearn  # noqa: F401
        except ImportError:
            results.append(dict(what="sklearn", skipped="scikit-learn does not import"))
        else:
            for n in args.sklearn_sizes:
                r, done = run_child("sklearn", args, n, args.sklearn_limit)
                results.append(r)
                if done:
                    break
    print(json.dumps(dict(tool="cluster_quality_time", results=results)), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
