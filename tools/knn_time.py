"""Time the k-NN tools (torch_scae_amd/neighbors.py, csrc/knn.hip) on synthetic capsule-like
features with 10 classes -- (10 000, 24) queries against (60 000, 24) base rows at k = 20, the
shape of MNIST test against train -- HIP-event timed after a warm-up, one JSON line:

    python tools/knn_time.py [--nq 10000] [--nb 60000] [--k 20] [--trust-n 10000] [--no-host]

- ``neighbors.knn``; ``neighbors.classify`` (the search and the vote, ks = (1, 5, k));
  ``neighbors.trustworthiness`` of a random 2-D embedding at N = ``--trust-n``, k = 12;
- the same search in torch ops on the device: ``torch.cdist`` and ``topk`` over chunks of
  ``--torch-rows`` query rows (the whole (Nq, Nb) matrix would be 2.4 GB); its distances are
  rounded otherwise and its ties fall where the sort leaves them, so only its time is compared;
- ``neighbors.knn_host`` (float32 numpy) on ``--host-nq`` of the queries, scaled to all of them.
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

from tools.tsne_time import synthetic, timed  # noqa: E402


def torch_search(q, b, k, rows):
    import torch
    d2, idx = [], []
    for lo in range(0, q.shape[0], rows):
        d, i = torch.cdist(q[lo:lo + rows], b).topk(k, dim=1, largest=False)
        d2.append(d * d)
        idx.append(i)
    return torch.cat(idx), torch.cat(d2)


def child(what, args):
    import torch
    from torch_scae_amd import neighbors as NB
    xq, _ = synthetic(args.nq, seed=1)
    xb, yb = synthetic(args.nb, seed=0)
    q, b = torch.from_numpy(xq).cuda(), torch.from_numpy(xb).cuda()
    lab = torch.from_numpy(yb).cuda()
    out = dict(what=what, Nq=args.nq, Nb=args.nb, F=q.shape[1], k=args.k)
    if what == "knn":
        ms, _ = timed(lambda: NB.knn(q, args.k, b), reps=3)
        out.update(ms=round(ms, 3), groups=NB._lib.load().scae_knn_groups(args.nq, args.nb))
    elif what == "classify":
        ks = tuple(sorted({1, min(5, args.k), args.k}))
        ms, _ = timed(lambda: NB.classify(q, b, lab, ks), reps=3)
        out.update(ms=round(ms, 3), ks=ks)
    elif what == "trustworthiness":
        N = args.trust_n
        x = torch.from_numpy(synthetic(N, seed=2)[0]).cuda()
        y = np.random.default_rng(3).standard_normal((N, 2)).astype(np.float32)
        y = torch.from_numpy(y).cuda()
        ms, t = timed(lambda: NB.trustworthiness(x, y, 12), reps=3)
        out = dict(what=what, N=N, F=x.shape[1], k=12, ms=round(ms, 3), value=t)
    elif what == "torch":
        ms, (idx, _) = timed(lambda: torch_search(q, b, args.k, args.torch_rows), reps=3)
        ours = NB.knn(q, args.k, b).idx
        out.update(ms=round(ms, 3), rows_per_chunk=args.torch_rows,
                   lists_equal_to_knn=float((idx == ours).all(1).float().mean()))
    print(json.dumps(out), flush=True)


def run_child(what, args):
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
           "--child", what, "--nq", str(args.nq), "--nb", str(args.nb), "--k", str(args.k),
           "--trust-n", str(args.trust_n), "--torch-rows", str(args.torch_rows)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return dict(what=what, error=f"exit {r.returncode}"), False
    return json.loads(r.stdout.strip().splitlines()[-1]), True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--nb", type=int, default=60000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--trust-n", type=int, default=10000)
    ap.add_argument("--torch-rows", type=int, default=2048)
    ap.add_argument("--host-nq", type=int, default=10000)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args)
    results, ok = [], True
    for what in ("knn", "classify", "trustworthiness", "torch"):
        if ok:
            r, ok = run_child(what, args)
            results.append(r)
    if not args.no_host:
        import torch
        from torch_scae_amd import neighbors as NB
        n = min(args.host_nq, args.nq)
        q = torch.from_numpy(synthetic(args.nq, seed=1)[0][:n])
        b = torch.from_numpy(synthetic(args.nb, seed=0)[0])
        t0 = time.perf_counter()
        NB.knn_host(q, args.k, b)
        ms = 1e3 * (time.perf_counter() - t0)
        results.append(dict(what="knn_host (float32 numpy)", Nq=n, Nb=args.nb, k=args.k,
                            ms=round(ms, 1), ms_scaled_to_all_queries=round(ms * args.nq / n, 1)))
    print(json.dumps(dict(tool="knn_time", results=results)), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
