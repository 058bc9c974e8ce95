"""micro-benchmark of metric.vsd_errors (cp_vsd_errors: depth rasteriser + BOP's VSD counting), tools/bop_error_bench.py's method.

  python tools/vsd_bench.py [--out profiles/vsd_bench.json] [--calls 100] [--warmup 10] [--quick]

Device: events around `--calls` calls after `--warmup` warm-ups, 640 x 480 frames, B in {1, 32, 256} poses of an icosphere of 1 280,
20 480 and 81 920 triangles (radius 50 mm at 350 - 600 mm: 95 - 165 pixels across), the estimate a few mm off the ground truth, a
seeded test depth.  The time is that of the whole Python call (outputs and scratch allocated), as a user pays it.
`tri_tile_tests_per_s` = sum over poses and sides of (triangles x 32-pixel tiles its rectangle reaches) / time: every tile sets up
every triangle of the mesh once -- the unit of the tile launch's work; the tiles are counted from the depth images a separate call
returns.  The share of the pose / vertex / tile / sum launches comes from a kernel trace of the `--quick` run
(rocprofv3 --kernel-trace --stats), not from this script.
No host figure exists for the reference's render path (its OpenGL renderers run nowhere this project runs), so NO ratio is given.
What is timed on the host, one pose, and named for what it is: `host_numpy_scoring_ms` -- the numpy counting of pose_error.vsd given
the two depth images (tests/vsd_stages.score); `host_oracle_render_ms` -- tests/vsd_stages.oracle_render of ONE side, an untuned
float64 numpy loop that also computes its dilated / eroded depths: NOT the reference's OpenGL render."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from checkerpose_amd import metric  # noqa: E402
from tests import vsd_stages as S  # noqa: E402
from tools.bop_error_bench import timed  # noqa: E402

LM_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
W, H = 640, 480


def poses(rng, n):
    R = np.stack([S_rot(rng) for _ in range(n)])
    t_gt = np.stack([rng.uniform(-120, 120, n), rng.uniform(-80, 80, n), rng.uniform(350, 600, n)], 1)
    t_est = t_gt + rng.normal(size=(n, 3)) * 4.0
    return R, t_est, t_gt


def S_rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def tiles_of(depth):
    """32-pixel tiles the bounding rectangle of the covered pixels reaches"""
    ys, xs = np.nonzero(depth > 0)
    if not ys.size:
        return 0
    return (xs.max() // 32 - xs.min() // 32 + 1) * (ys.max() // 32 - ys.min() // 32 + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vsd_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    R, t_est, t_gt = poses(rng, 256)
    test = (300.0 + 400.0 * rng.random((4, H, W))).astype(np.float32)
    test[rng.random(test.shape) < 0.1] = 0.0
    test_dev = torch.from_numpy(test).to(dev)
    levels = {1280: 3, 20480: 5, 81920: 6}
    shapes = [(B, F) for F in (1280, 20480, 81920) for B in (1, 32, 256)]
    calls, warmup = a.calls, a.warmup
    if a.quick:
        shapes, calls, warmup = [(32, 1280), (256, 20480)], 3, 1
    rows, host = [], {}
    for B, F in shapes:
        v, f = S._icosphere(levels[F], 50.0)
        ms = metric.MeshSet.from_arrays([v.astype(np.float32)], diameters=[100.0], faces=[f])
        up = lambda x, s: torch.from_numpy(np.ascontiguousarray(x[:B].reshape(s))).to(dev)   # noqa: E731
        args = (up(R, (B, 3, 3)), up(t_est, (B, 3, 1)), up(R, (B, 3, 3)), up(t_gt, (B, 3, 1)), LM_K, ms, test_dev)
        ids = torch.arange(B, dtype=torch.int32, device=dev) % 4
        once = metric.vsd_errors(*args, image_ids=ids, return_depth=True, return_counts=True)
        depth = once["depth"].cpu().numpy()
        work = float(sum(F * tiles_of(depth[b, s]) for b in range(B) for s in range(2)))
        if F not in host and not a.quick:
            t0 = time.perf_counter()
            S.score(test[0], depth[0, 0], depth[0, 1], LM_K, 15.0, S.TAUS, True, 100.0)
            t1 = time.perf_counter()
            S.oracle_render(R[0], t_gt[0], LM_K, v, f, (W, H))
            host[F] = ((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3)
        t = timed(lambda: metric.vsd_errors(*args, image_ids=ids), calls, warmup)
        row = {"B": B, "F": F, "V": int(v.shape[0]), "device_ms": t, "ms_per_pose": t / B, "tri_tile_tests": work, "tri_tile_tests_per_s": work / (t * 1e-3),
               "inter_pixels_pose0": int(once["counts"][0, 1])}
        if F in host:
            row["host_numpy_scoring_ms_per_pose"], row["host_oracle_render_ms_per_side"] = host[F]
        rows.append(row)
        print("B=%3d F=%5d: %.3f ms per call (%.4f per pose), %.3g triangle-tile tests/s; host numpy scoring %s ms / pose, oracle render %s ms / side"
              % (B, F, t, t / B, row["tri_tile_tests_per_s"], "%.1f" % host[F][0] if F in host else "-", "%.0f" % host[F][1] if F in host else "-"), flush=True)
    res = {"bench": "vsd_errors", "device": torch.cuda.get_device_name(0), "calls": calls, "warmup": warmup, "frame": [W, H],
           "host_threads": os.environ.get("OMP_NUM_THREADS"),
           "host_paths": "numpy counting of vsd given depth images (one pose); the float64 oracle rasteriser of tests/vsd_stages.py (one side) "
                         "-- an untuned numpy loop, NOT the reference's OpenGL render: no ratio is claimed", "rows": rows}
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
