"""micro-benchmark of metric.mask_errors (cp_mask_errors: both silhouettes rasterised per tile, BOP's cus / cou_bb_proj counted in
registers) against the composition a user could already make: metric.render_depth of both sides with the images stored, then torch
logical operations and reductions.  tools/vsd_bench.py's method.

  python tools/mask_error_bench.py [--out profiles/mask_error_bench.json] [--calls 100] [--warmup 10] [--repeats 3] [--quick]

Device: events around `--calls` calls after `--warmup` warm-ups, repeated `--repeats` times (median, min and max are recorded: the
run-to-run spread), 640 x 480 frames, B in {1, 32, 256} pairs of an icosphere of 1 280 and 20 480 triangles (radius 50 mm at
350 - 600 mm), the estimate a few mm off the ground truth.  The time is that of the whole Python call (outputs and scratch
allocated), as a user pays it.  The composition computes cus only (counts by sum over the frame, the quotient with torch.where);
mask_errors is timed for cus alone and for cus + cou_bb_proj.  The two give the same cus bits: asserted before timing.
The share of the pose / vertex / tile / finish launches comes from a kernel trace of the `--quick` run (rocprofv3 --kernel-trace
--stats), not from this script.  No host figure exists for the reference's render path (its OpenGL renderers run nowhere this
project runs), so NO ratio against the reference is given."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from checkerpose_amd import _abi, metric  # noqa: E402
from tests import vsd_stages as S  # noqa: E402
from tools.bop_error_bench import timed  # noqa: E402
from tools.vsd_bench import LM_K, H, W, poses  # noqa: E402


def composed_cus(R_est, t_est, R_gt, t_gt, K, ms):
    """cus from two stored renders: what the parent commit offers"""
    me = metric.render_depth(R_est, t_est, K, ms, (W, H)) > 0
    mg = metric.render_depth(R_gt, t_gt, K, ms, (W, H)) > 0
    inter = (me & mg).sum((1, 2))
    union = (me | mg).sum((1, 2))
    return torch.where(union > 0, 1.0 - inter.double() / union.clamp(min=1).double(), torch.ones_like(inter, dtype=torch.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_error_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    R, t_est, t_gt = poses(rng, 256)
    levels = {1280: 3, 20480: 5}
    shapes = [(B, F) for F in (1280, 20480) for B in (1, 32, 256)]
    calls, warmup, repeats = a.calls, a.warmup, a.repeats
    if a.quick:
        shapes, calls, warmup, repeats = [(32, 1280), (256, 20480)], 3, 1, 1
    rows = []
    for B, F in shapes:
        v, f = S._icosphere(levels[F], 50.0)
        ms = metric.MeshSet.from_arrays([v.astype(np.float32)], diameters=[100.0], faces=[f])
        up = lambda x, s: torch.from_numpy(np.ascontiguousarray(x[:B].reshape(s))).to(dev)   # noqa: E731
        args = (up(R, (B, 3, 3)), up(t_est, (B, 3, 1)), up(R, (B, 3, 3)), up(t_gt, (B, 3, 1)), LM_K, ms)
        once = metric.mask_errors(*args, (W, H), return_counts=True)
        assert torch.equal(once["cus"], composed_cus(*args)), "the composition and mask_errors disagree"
        paths = {"mask_errors_cus": lambda: metric.mask_errors(*args, (W, H), kinds=("cus",)),
                 "mask_errors_both": lambda: metric.mask_errors(*args, (W, H)),
                 "composed_cus": lambda: composed_cus(*args)}
        row = {"B": B, "F": F, "V": int(v.shape[0]), "union_pixels_pair0": int(once["counts"][0, 1])}
        for name, fn in paths.items():
            ts = sorted(timed(fn, calls, warmup) for _ in range(repeats))
            row[name + "_ms"] = {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}
        new, old = row["mask_errors_cus_ms"], row["composed_cus_ms"]
        row["not_slower_beyond_spread"] = bool(new["min"] <= old["max"])
        rows.append(row)
        print("B=%3d F=%5d: mask_errors cus %.3f ms [%.3f, %.3f], both kinds %.3f ms, composed %.3f ms [%.3f, %.3f]"
              % (B, F, new["median"], new["min"], new["max"], row["mask_errors_both_ms"]["median"], old["median"], old["min"], old["max"]), flush=True)
    res = {"bench": "mask_errors", "device": torch.cuda.get_device_name(0), "calls": calls, "warmup": warmup, "repeats": repeats,
           "frame": [W, H], "lib_version": int(_abi.load().cp_version()),
           "comparison": "composed_cus = metric.render_depth twice with the images stored + torch logical operations and reductions "
                         "(what the parent commit offers); no ratio against the reference's OpenGL path is claimed", "rows": rows}
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
