"""Time per-example predictions over a whole split three ways, host clock around work that
ends in a device synchronise, and print one JSON line per way and one for the difference:

    python tools/predict_time.py [CONFIG] [--images N] [--reps R]

CONFIG: cfg2 (MNIST 40x40, 24/24, B=128; the default), cfg5 or cfg3 (tools/eval_time.py's).
Ways, over the same N images (default 60000, with a remainder batch):
  - ``predict``: EvalStep.predict -- every batch replayed, the records and the confusion
    matrices written by the epilogue's combine workgroup, one read at the end;
  - ``evaluate``: EvalStep.evaluate on a step that never had records attached: the launches of
    the commit before the records existed (SCAE_HIP_LIB=<a build of that commit> times that
    build's library instead; this tool then skips ``predict``);
  - ``eager``: what a script did without ``predict`` -- per batch an eager no-grad forward,
    both heads' argmax, the per-image sum of the materialised per-pixel log-likelihood, a
    bincount per head and a host read.
The ways are run in turn, R rounds (default 5) after one warm-up round; reported: the median
and the spread of the rounds in ms per split, ms per batch, and ``predict - evaluate`` per
batch.  The parameters lie in flat buffers, as a training run's TrainStep puts them.  Run it
in a process of its own under its own time limit."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from torch_scae_amd import EvalStep, factory  # noqa: E402
from torch_scae_amd.data_parallel import FlatParameters  # noqa: E402
from eval_time import CONFIGS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="cfg2", choices=sorted(CONFIGS))
    ap.add_argument("--images", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_time.py measures on the GPU: none is visible")
    cfg, B = CONFIGS[args.config]
    cfg = dict(cfg, scae_params=dict(reconstruct_alternatives=False))
    torch.manual_seed(0)
    model = factory.make_scae(cfg).cuda().train()
    flat = FlatParameters(model)  # noqa: F841
    g = torch.Generator().manual_seed(1)
    N = args.images
    images = torch.rand(N, *cfg["image_shape"], generator=g).cuda()
    labels = torch.randint(0, 10, (N,), generator=g).cuda()
    n_batches = -(-N // B)
    ncls = cfg["n_classes"]

    def eager():
        was = model.training
        model.eval()
        conf = torch.zeros(2, ncls * ncls, dtype=torch.int64)
        with torch.no_grad():
            for lo in range(0, N, B):
                x, y = images[lo:lo + B], labels[lo:lo + B]
                res = model(x)
                pc, qc = res.prior_cls_prob.argmax(-1), res.posterior_cls_prob.argmax(-1)
                rec = res.rec.pdf.log_prob(x).view(x.shape[0], -1).sum(-1)  # noqa: F841
                cells = torch.stack([torch.bincount(y * ncls + pc, minlength=ncls * ncls),
                                     torch.bincount(y * ncls + qc, minlength=ncls * ncls)])
                conf += cells.cpu()              # the host read per batch
        model.train(was)
        return conf

    ways = {}
    if not os.environ.get("SCAE_HIP_LIB"):
        pstep = EvalStep(model, B, cfg["image_shape"])
        out = torch.empty(N, 9, device="cuda")
        ways["predict"] = lambda: pstep.predict(images, labels, out=out)
    estep = EvalStep(model, B, cfg["image_shape"])
    ways["evaluate"] = lambda: estep.evaluate(images, labels)
    ways["eager"] = eager

    times = {k: [] for k in ways}
    for r in range(args.reps + 1):
        for name, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:                                # (round 0: captures and warm-up)
                times[name].append((time.perf_counter() - t0) * 1e3)
    tag = dict(config=args.config, batch=B, images=N, batches=n_batches, reps=args.reps)
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        print(json.dumps(dict(tag, way=name, ms_per_split=round(med[name], 3),
                              ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
                              ms_per_batch=round(med[name] / n_batches, 5),
                              images_per_s=round(N / med[name] * 1e3))), flush=True)
    if "predict" in med:
        d = (med["predict"] - med["evaluate"]) / n_batches
        print(json.dumps(dict(tag, way="predict - evaluate",
                              us_per_batch=round(d * 1e3, 3))), flush=True)


if __name__ == "__main__":
    main()
