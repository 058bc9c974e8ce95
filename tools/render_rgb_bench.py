#!/usr/bin/env python3
"""Row N14: what a shaded frame costs beside the depth render it is built on.

  python tools/render_rgb_bench.py [--quick] [--out profiles/render_rgb_bench.json]

Times whole Python calls of render.render_rgb: device events around `calls` (100) calls after `warmup` (10) warm-ups, every
configuration alike; the calls are timed in four consecutive blocks, the mean over all of them is the figure and (slowest block -
fastest block) / median block is the run-to-run spread.  640 x 480 frames of icospheres with 1 280 and 20 480 triangles, B = 1 / 32 /
256, flat and phong, ssaa 1 and 4 (`--faces` restricts a run to one mesh; rows of such runs are merged by hand into one file).  Comparator: metric.render_depth on the same poses -- the same walk without shading, present before
this row.  No pass / fail ratio is fixed: nobody had measured one.  No time of the reference's OpenGL path is claimed (it runs nowhere
this project runs)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from checkerpose_amd import metric, render  # noqa: E402
from tests import vsd_stages as S  # noqa: E402

LM_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
W, H = 640, 480


def rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def timed(fn, calls, warmup, blocks=4):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = [calls // blocks + (1 if k < calls % blocks else 0) for k in range(blocks)]
    per = [n for n in per if n > 0]
    out = []
    for n in per:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    each = sorted(ms / n for ms, n in zip(out, per))
    return sum(out) / sum(per), (each[-1] - each[0]) / each[len(each) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_rgb_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--faces", type=int, choices=(1280, 20480), default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    R = np.stack([rotation(rng) for _ in range(256)])
    t = np.stack([rng.uniform(-200, 200, 256), rng.uniform(-150, 150, 256), rng.uniform(350, 600, 256)], 1)
    levels = {1280: 3, 20480: 5}
    shapes = [(B, F) for F in (1280, 20480) for B in (1, 32, 256) if a.faces in (None, F)]
    calls, warmup = a.calls, a.warmup
    if a.quick:
        shapes, calls, warmup = [(256, 1280)], 3, 1
    rows = []
    for B, F in shapes:
        v, f = S._icosphere(levels[F], 50.0)
        col = np.round(30.0 + 220.0 * (v - v.min(0)) / (v.max(0) - v.min(0))).astype(np.uint8)
        ms = metric.MeshSet.from_arrays([v.astype(np.float32)], diameters=[100.0], faces=[f], colors=[col], normals=[(v / 50.0).astype(np.float32)])
        Rd = torch.from_numpy(np.ascontiguousarray(R[:B])).to(dev)
        td = torch.from_numpy(np.ascontiguousarray(t[:B].reshape(B, 3, 1))).to(dev)
        t_d, s_d = timed(lambda: metric.render_depth(Rd, td, LM_K, ms, (W, H)), calls, warmup)
        row = {"B": B, "F": F, "V": int(v.shape[0]), "render_depth_ms": t_d, "render_depth_spread": s_d}
        for shading in ("flat", "phong"):
            for ssaa in (1, 4):
                out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
                t_r, s_r = timed(lambda: render.render_rgb(Rd, td, LM_K, ms, (W, H), shading=shading, ssaa=ssaa, out=out), calls, warmup)
                row["%s_ssaa%d" % (shading, ssaa)] = {"ms": t_r, "spread": s_r, "ratio_to_render_depth": t_r / t_d, "ms_per_pose": t_r / B}
                print("B=%3d F=%5d %-5s ssaa %d: %.3f ms (spread %.3f), render_depth %.3f ms, ratio %.2f" % (B, F, shading, ssaa, t_r, s_r, t_d, t_r / t_d),
                      flush=True)
                del out
        rows.append(row)
        torch.cuda.empty_cache()
    res = {"bench": "render_rgb", "device": torch.cuda.get_device_name(0), "calls": calls, "warmup": warmup, "blocks": 4, "frame": [W, H],
           "comparator": "metric.render_depth on the same poses (the same tile walk without shading; it stores 4 bytes per pixel, the frame 3)",
           "rows": rows}
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
