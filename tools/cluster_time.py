"""Time the unsupervised-classification pipeline at cfg-2 (B = 128) on 60 000
``data.stroke_batches`` images, HIP-event timed after warm-up, one JSON line per measurement:

    python tools/cluster_time.py [--n 60000] [--reps 3]

- encode: ``EvalStep.encode`` (replayed batches, features stored by the loss tail's per-image
  launch) against an eager no_grad loop that gathers the same two tensors
  (``caps_presence``, ``posterior_mixing_prob.sum(-1)``) batch by batch;
- k-means with k = 10 on the (N, 24) prior features: ``cluster.kmeans`` with n_init = 10,
  the same with n_init = 1, a torch-op Lloyd on the device (cdist / argmin / index_add_,
  n_init = 10 restarts one after the other, the same iteration rules) and ``kmeans_host``
  (fp64 numpy, n_init = 10).
Run it in a process of its own under its own time limit."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from torch_scae_amd import EvalStep, cluster, data, factory  # noqa: E402

CFG = dict(image_shape=(1, 40, 40), n_classes=10, n_part_caps=24, n_obj_caps=24,
           scae_params=dict(reconstruct_alternatives=False))
B = 128


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


def torch_lloyd(x, init, max_iter=300):
    """Lloyd in torch ops on the device, one restart (float-atomic sums: not reproducible)."""
    c = init.clone()
    prev = torch.full((x.shape[0],), -1, device=x.device, dtype=torch.int64)
    k = c.shape[0]
    for it in range(max_iter):
        lab = torch.cdist(x, c).argmin(1)
        if bool((lab == prev).all()):
            break
        s = torch.zeros_like(c).index_add_(0, lab, x)
        n = torch.bincount(lab, minlength=k).to(x.dtype)
        c = torch.where(n[:, None] > 0, s / n.clamp(min=1)[:, None], c)
        prev = lab
    return c, lab, it + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    torch.manual_seed(0)
    model = factory.make_scae(CFG).cuda().train()
    nb = (args.n + B - 1) // B
    imgs, labs = data.stroke_batches(nb, B, CFG["image_shape"], seed=0)
    images = imgs.flatten(0, 1)[:args.n].cuda()
    labels = labs.flatten()[:args.n].cuda()
    N = images.shape[0]
    step = EvalStep(model, B, CFG["image_shape"])

    ms, enc = timed(lambda: step.encode(images, labels), args.reps)
    print(json.dumps({"what": "encode", "way": "EvalStep.encode", "N": N, "ms": round(ms, 3),
                      "us_per_batch": round(1e3 * ms / nb, 2), "fused": bool(step.fused)}))

    def eager():
        pres, mass = [], []
        with step._eval_mode():
            for i in range(0, N, B):
                res = model(images[i:i + B])
                pres.append(res.caps_presence)
                mass.append(res.posterior_mixing_prob.sum(-1))
        return torch.cat(pres), torch.cat(mass)
    ms, _ = timed(eager, args.reps)
    print(json.dumps({"what": "encode", "way": "eager no_grad loop", "N": N,
                      "ms": round(ms, 3), "us_per_batch": round(1e3 * ms / nb, 2)}))

    x = enc["prior"].contiguous()
    for n_init in (10, 1):
        ms, res = timed(lambda: cluster.kmeans(x, 10, n_init=n_init, seed=0), args.reps)
        print(json.dumps({"what": "kmeans", "way": f"cluster.kmeans n_init={n_init}",
                          "N": N, "F": x.shape[1], "ms": round(ms, 3), "n_iter": res.n_iter,
                          "converged": res.converged, "inertia": res.inertia}))
    inits = cluster.kmeans_pp_host(x.cpu(), 10, n_init=10, seed=0)[0]
    inits = torch.from_numpy(inits).float().cuda()

    def torch_all():
        best = None
        for r in range(10):
            c, lab, it = torch_lloyd(x, inits[r])
            inertia = float(((x - c[lab]) ** 2).sum(1).double().sum())
            if best is None or inertia < best[0]:
                best = (inertia, it)
        return best
    ms, best = timed(torch_all, 1)
    print(json.dumps({"what": "kmeans", "way": "torch-op Lloyd n_init=10", "N": N,
                      "ms": round(ms, 3), "n_iter": best[1], "inertia": best[0]}))
    xc = x.cpu()
    t0 = time.perf_counter()
    res = cluster.kmeans_host(xc, 10, n_init=10, seed=0)
    ms = 1e3 * (time.perf_counter() - t0)
    print(json.dumps({"what": "kmeans", "way": "kmeans_host n_init=10 (fp64 numpy)", "N": N,
                      "ms": round(ms, 1), "n_iter": res.n_iter, "inertia": res.inertia}))


if __name__ == "__main__":
    main()
