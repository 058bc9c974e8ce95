"""A/B: the LM woProg ablation (PoseNet_GNNskip_ABwoProg) against the LM PoseNet_GNNskip on the same box, in alternating runs --
crops/s of the eval forward (hipGraph replay) at B = 256 bf16 and at B = 1 (fp32), shipped config values, deterministic weights.

    python tools/woprog_ab.py [--rounds R] [--iters I] [--out profiles/woprog_ab.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from checkerpose_amd.synthetic import build_net, build_woprog, det_image  # noqa: E402


def timed(net, img, obj, iters):
    with torch.no_grad():
        for _ in range(3):
            net(img, None, obj)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            net(img, None, obj)
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nets = {"lm": build_net(seed=0, lm=True).to(dev), "woprog": build_woprog(seed=0).to(dev)}
    res = {}
    for B, dtype in ((256, "bf16"), (1, "fp32")):
        for n in nets.values():
            n.set_compute_dtype(dtype)
        img = det_image(B, seed=1).to(dev)
        obj = torch.tensor([i % 13 + 1 for i in range(B)], device=dev)
        ms = {k: [] for k in nets}
        for _ in range(a.rounds):
            for k, n in nets.items():           # alternating: lm, woprog, lm, woprog, ...
                ms[k].append(timed(n, img, obj, a.iters))
        best = {k: min(v) for k, v in ms.items()}
        key = "B%d_%s" % (B, dtype)
        res[key] = dict(ms=ms, crops_per_s={k: B * 1e3 / v for k, v in best.items()}, woprog_over_lm=best["lm"] / best["woprog"])
        print(json.dumps({key: res[key]}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
