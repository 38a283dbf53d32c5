"""Capture optimiser trajectories from the REAL reference (bdsaglam/torch-scae) into
tests/golden/optim_trajectories.npz.

    python tests/golden/make_optimizer_golden.py <reference checkout>

Needs a checkout of the reference (its ``torch_scae/optimizers.py``: RAdam and
LookAhead, imported from there, not restated) and stock ``torch.optim`` (Adam,
RMSprop, ExponentialLR).  Only the output file is used by the tests.

Three fp32 tensors of awkward sizes (1, 13, 37 elements: scalar heads, float4 lanes and
tails at every phase once laid back to back) take 12 steps of one recorded gradient
sequence under each optimiser the reference offers (base_experiment.py:44-77:
RMSprop(momentum 0.9), Adam, RAdam; eps = 1e-2 / 128**2), each with weight decay 0 and
1e-2, each wrapped in LookAhead(k=5, alpha=0.5) without weight decay and Adam also with
it (CASES), with ONE ExponentialLR(0.9) step between steps 6 and 7.  (Sizes and cases
are what the coverage needs and no more: the file stays small.)  12 steps
cover RAdam's switch from SGD to the rectified update (t = 6 at b2 = 0.999) and
LookAhead's first sync (t = 5, which only creates the slow weights) and its
first real one (t = 10).

Keys: ``grad{j}`` (12, n_j); ``init{j}`` (n_j,); per case ``{case}/param{j}``
(12, n_j) after every step and ``{case}/{state}{j}`` (12, n_j) for each state
tensor (exp_avg, exp_avg_sq | square_avg, momentum_buffer; slow_buffer from the
first sync on, zeros before); ``{case}/lr`` (12,) the learning rate each step
used.  Case names: ``{rmsprop|adam|radam}_wd{0|0.01}[_la]``.
"""
import os
import sys
import warnings

import numpy as np
import torch

SIZES = (1, 13, 37)
# (optimiser, weight decay, LookAhead)
CASES = [(kind, wd, False) for kind in ("rmsprop", "adam", "radam") for wd in (0.0, 1e-2)] + \
    [(kind, 0.0, True) for kind in ("rmsprop", "adam", "radam")] + [("adam", 1e-2, True)]
STEPS = 12
LR, GAMMA, DECAY_AFTER = 1e-2, 0.9, 6
EPS = 1e-2 / 128.0 ** 2
LA_K, LA_ALPHA = 5, 0.5
STATE_KEYS = {"rmsprop": ("square_avg", "momentum_buffer"),
              "adam": ("exp_avg", "exp_avg_sq"), "radam": ("exp_avg", "exp_avg_sq")}


def main(ref):
    sys.path.insert(0, ref)
    warnings.simplefilter("ignore")      # (the reference's deprecated add_ / addcmul_ forms)
    from torch_scae.optimizers import LookAhead, RAdam

    g = torch.Generator().manual_seed(20)
    init = [torch.randn(n, generator=g) for n in SIZES]
    # gradients of three scales: one near eps (6.1e-7), where eps matters to Adam / RAdam
    scales = (1.0, 1e-3, 1e-6)
    grads = [torch.stack([torch.randn(n, generator=g) * s for _ in range(STEPS)])
             for n, s in zip(SIZES, scales)]
    out = {f"grad{j}": gr.numpy() for j, gr in enumerate(grads)}
    out.update({f"init{j}": p.numpy() for j, p in enumerate(init)})
    for kind, wd, la in CASES:
        case = f"{kind}_wd{wd:g}" + ("_la" if la else "")
        params = [p.clone().requires_grad_(True) for p in init]
        if kind == "rmsprop":
            opt = torch.optim.RMSprop(params, lr=LR, momentum=0.9, eps=EPS,
                                      weight_decay=wd)
        elif kind == "adam":
            opt = torch.optim.Adam(params, lr=LR, eps=EPS, weight_decay=wd)
        else:
            opt = RAdam(params, lr=LR, eps=EPS, weight_decay=wd)
        base = opt
        if la:
            opt = LookAhead(opt, k=LA_K, alpha=LA_ALPHA)
        sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=GAMMA)
        rec = {}
        lrs = []
        for s in range(STEPS):
            for p, gr in zip(params, grads):
                p.grad = gr[s].clone()
            lrs.append(opt.param_groups[0]["lr"])
            opt.step()
            for j, p in enumerate(params):
                rec.setdefault(f"{case}/param{j}", []).append(p.detach().clone())
                st = base.state[p]
                for key in STATE_KEYS[kind]:
                    rec.setdefault(f"{case}/{key}{j}", []).append(st[key].clone())
                if la:
                    slow = opt.state[p].get("slow_buffer")
                    rec.setdefault(f"{case}/slow_buffer{j}", []).append(
                        slow.clone() if slow is not None else torch.zeros_like(p))
            if s + 1 == DECAY_AFTER:
                sched.step()
        out.update({k: torch.stack(v).numpy() for k, v in rec.items()})
        out[f"{case}/lr"] = np.array(lrs)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "optim_trajectories.npz")
    np.savez_compressed(dst, **out)
    print(f"wrote {dst}: {len(out)} arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
