"""K8 timings per layer (forward, data gradient, backward pair, weight gradient) at a
bench workload's shapes."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
wl = sys.argv[1] if len(sys.argv) > 1 else "mnist_24_24_bs128"
cfg = bench.CONFIGS[wl]
dev = torch.device("cuda", 0)
k8 = bench.time_k8_kernels(cfg, dev, reps=30)
out = {}
for name, ls in k8.items():
    out[name] = [round(l["seconds"] * 1e6, 1) for l in ls] + \
        [round(sum(l["flops"] for l in ls) / sum(l["seconds"] for l in ls) / 1e12, 1)]
print("auto", json.dumps(out), flush=True)
