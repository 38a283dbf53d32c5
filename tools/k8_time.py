"""K8 timings per layer (forward, data gradient, backward pair, weight gradient) at a
bench workload's shapes.

    k8_time.py [WORKLOAD]                       the production forms (bench.time_k8_kernels)
    k8_time.py [WORKLOAD] --tiles 1,65,2,66     the backward pair and the stand-alone weight
                                                gradient of every layer per wgrad_tile code
                                                (scae_hip.h: SCAE_WGRAD_TILE_*), us, with the
                                                operand bytes the form's tiles stage (MB)
"""
import argparse, ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench

ap = argparse.ArgumentParser()
ap.add_argument("workload", nargs="?", default="mnist_24_24_bs128")
ap.add_argument("--tiles", default="")
ap.add_argument("--reps", type=int, default=30)
args = ap.parse_args()
cfg = bench.CONFIGS[args.workload]
dev = torch.device("cuda", 0)


def best_us(fn, reps, rounds=5):
    for _ in range(5):
        assert fn() == 0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(rounds):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    return round(min(ts), 2), round(sorted(ts)[len(ts) // 2], 2)


def tile_forms(codes):
    from torch_scae_amd import _lib, ops
    lib, B = _lib.load(), cfg["batch"]
    p, I = ops._p, ctypes.c_int
    shapes = {_lib.WGRAD_TILE_64x64: (64, 64), _lib.WGRAD_TILE_128x64: (128, 64)}
    HEAD = _lib.WGRAD_HEAD
    for li, (IH, Ci, Co, s) in enumerate(bench.conv_layers(cfg)):
        OH = (IH - 3) // s + 1
        f = lambda *sh: torch.randn(*sh, device=dev)   # noqa: E731
        x, wd = torch.relu(f(B, IH, IH, Ci)), f(Ci, 9, Co)
        dy, dx = f(B, OH, OH, Co), f(B, IH, IH, Ci)
        st = ops._stream(x)
        splits = lib.scae_conv3x3_wgrad_splits(B, OH, OH, Ci, Co)
        part = f(splits * (9 * Co * Ci + Co))
        geo = (I(B), I(IH), I(IH), I(Ci), I(Co), I(s))
        planned = lib.scae_conv3x3_wgrad_tile_plan(*geo, 0)
        ref = None
        for code in codes:
            eff = code or planned
            ta, tb = shapes[eff & ~HEAD]
            if Co % ta:
                ta = 64
            per = (((B * OH * OH + splits - 1) // splits) + 31) // 32 * 32
            # every tile stages (ta + tb) operand rows of 4 bytes per pixel of its split
            staged = (Co // ta) * (Ci // tb) * 9 * splits * per * (ta + tb) * 4 / 1e6
            pair = best_us(lambda: lib.scae_conv3x3_bwd_pair_tile_f32(
                p(dy), p(wd), p(x), p(dx), p(part), *geo, 0, st, code), args.reps)
            torch.cuda.synchronize()
            bits = part.clone()
            alone = best_us(lambda: lib.scae_conv3x3_wgrad_tile_f32(
                p(dy), p(x), p(part), None, None, *geo, st, code & ~HEAD), args.reps)
            ref = bits if ref is None else ref
            print("tile", json.dumps(dict(
                layer=li + 2, code=code, planned=planned, tile=[ta, tb],
                head=bool(eff & HEAD), splits=splits, staged_mb=round(staged, 1),
                pair_us_best_median=pair, wgrad_us_best_median=alone,
                same_bits_as_first=bool(torch.equal(bits.view(torch.int32),
                                                    ref.view(torch.int32))))), flush=True)


if args.tiles:
    tile_forms([int(c) for c in args.tiles.split(",")])
else:
    k8 = bench.time_k8_kernels(cfg, dev, reps=args.reps)
    out = {}
    for name, ls in k8.items():
        out[name] = [round(l["seconds"] * 1e6, 1) for l in ls] + \
            [round(sum(l["flops"] for l in ls) / sum(l["seconds"] for l in ls) / 1e12, 1)]
    print("auto", json.dumps(out), flush=True)
