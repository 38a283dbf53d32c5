"""Time one evaluation batch (forward + SCAE.loss + calculate_accuracy under eval() and
no_grad) three ways, HIP-event timed, and print one JSON line per way:

    python tools/eval_time.py CONFIG [--bf16] [--reps N]

CONFIG: cfg2 (MNIST 40x40, 24/24, B=128), cfg5 (CIFAR shape, 32/32, B=256) or cfg3
(configs[2]'s shape, 48/64, B=1024).  Ways: EvalStep with graph replay, EvalStep with
launch-list replay, and the eager path a training script used before EvalStep (an eager
``model(x)`` + ``model.loss`` + ``calculate_accuracy`` and a host read of the loss per
batch, tools/train_strokes.py).  Reported: ms per batch, images/s, and launches per
batch -- the kernel nodes of the captured graph for EvalStep, the library's launches
(ATen kernels not counted) for the eager path.  The parameters lie in flat buffers, as a
training run's TrainStep puts them.  Run each CONFIG in a process of its own
under its own time limit."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from torch_scae_amd import EvalStep, _lib, factory  # noqa: E402
from torch_scae_amd.data_parallel import FlatParameters  # noqa: E402

CONFIGS = {
    "cfg2": (dict(image_shape=(1, 40, 40), n_classes=10, n_part_caps=24, n_obj_caps=24), 128),
    "cfg5": (dict(image_shape=(3, 32, 32), n_classes=10, n_part_caps=32, n_obj_caps=32), 256),
    "cfg3": (dict(image_shape=(1, 40, 40), n_classes=10, n_part_caps=48, n_obj_caps=64), 1024),
}


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=sorted(CONFIGS))
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    cfg, B = CONFIGS[args.config]
    cfg = dict(cfg, scae_params=dict(reconstruct_alternatives=False))
    torch.manual_seed(0)
    model = factory.make_scae(cfg).cuda().train()
    # the parameters in flat buffers, as the TrainStep of a training run lays them out
    flat = FlatParameters(model)  # noqa: F841
    g = torch.Generator().manual_seed(1)
    n_batches = 8
    images = torch.rand(n_batches * B, *cfg["image_shape"], generator=g).cuda()
    labels = torch.randint(0, 10, (n_batches * B,), generator=g).cuda()
    batches = [(images[i * B:(i + 1) * B], labels[i * B:(i + 1) * B])
               for i in range(n_batches)]
    dt = torch.bfloat16 if args.bf16 else None
    tag = dict(config=args.config, batch=B, dtype="bf16" if args.bf16 else "fp32")

    def report(way, ms, launches):
        print(json.dumps(dict(tag, way=way, ms_per_batch=round(ms, 4),
                              images_per_s=round(B / ms * 1e3), launches=launches)),
              flush=True)

    for replay in ("graph", "launches"):
        step = EvalStep(model, B, cfg["image_shape"], replay=replay, autocast_dtype=dt)
        step(*batches[0])
        it = iter(range(1 << 30))
        ms = timed(lambda: step(*batches[next(it) % n_batches]), args.reps)
        report(f"EvalStep {replay}", ms, step.graph_nodes[1] if step.graph_nodes else None)
        del step

    calls = []
    real = _lib.call

    def eager(x, y):
        was = model.training
        model.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=args.bf16):
            res = model(x)
            loss, _ = model.loss(res, x, y)
            acc = model.calculate_accuracy(res, y)
        model.train(was)
        return float(loss), acc

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    _lib.call = spy
    try:
        eager(*batches[0])
    finally:
        _lib.call = real
    it = iter(range(1 << 30))
    ms = timed(lambda: eager(*batches[next(it) % n_batches]), args.reps)
    report("eager no_grad", ms, len(calls))


if __name__ == "__main__":
    main()
