"""micro-benchmark of gt_info.gt_info (cp_gt_info: the 3W x 3H canvas render fused with BOP's ground-truth counting), tools/vsd_bench.py's
method.

  python tools/gt_info_bench.py [--out profiles/gt_info_bench.json] [--calls 100] [--warmup 10] [--quick]

Device: events around `--calls` calls after `--warmup` warm-ups, 640 x 480 frames, B in {1, 32, 256} poses of an icosphere of 1 280 and
20 480 triangles (radius 50 mm at 350 - 600 mm), some of them cut by the frame's edge, a seeded sensor depth.  The time is that of
the whole Python call (outputs and scratch allocated), as a user pays it.
Baseline `composed_ms`: what a user could already compose from existing pieces -- metric.render_depth on the 3W x 3H canvas (the
principal point moved by (W, H)) followed by torch's elementwise operations and reductions for the distances, the visibility test,
the three counts and the two boxes (`composed` below; it returns what gt_info returns without the images).  `ratio` =
composed_ms / fused_ms.  The composition holds a (B,3H,3W) float image: at B = 256 that is 2.8 GB for the depth alone.
The share of the pose / vertex / tile / finish launches comes from a kernel trace of the `--quick` run (rocprofv3 --kernel-trace
--stats), not from this script.  No host figure exists for the reference's OpenGL path, so NO ratio against it is given."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from checkerpose_amd import gt_info as GI, metric  # noqa: E402
from tests import vsd_stages as S  # noqa: E402
from tools.bop_error_bench import timed  # noqa: E402
from tools.vsd_bench import LM_K, S_rot  # noqa: E402

W, H = 640, 480


def composed(R, t, K, ms, depth, image_ids, delta=15.0):
    """gt_info's counts, fraction and boxes from metric.render_depth on the canvas + torch operations"""
    dev = R.device
    B = R.shape[0]
    Kc = torch.as_tensor(K, dtype=torch.float64).clone()
    Kc[0, 2] += W
    Kc[1, 2] += H
    large = metric.render_depth(R, t, Kc, ms, (3 * W, 3 * H))
    dg = large[:, H:2 * H, W:2 * W].to(torch.float64)
    dt = depth[image_ids.long()].to(torch.float64)
    xs = (torch.arange(W, device=dev, dtype=torch.float64) - K[0, 2]) / K[0, 0]
    ys = (torch.arange(H, device=dev, dtype=torch.float64) - K[1, 2]) / K[1, 1]
    r = torch.sqrt(xs[None, :] ** 2 + ys[:, None] ** 2 + 1.0)
    t_gt, t_im = dg * r, dt * r
    mask = t_gt > 0
    visib = ((t_gt.float() - t_im.float() <= delta) | (t_im == 0)) & mask
    obj = large > 0
    n_all, n_valid, n_visib = obj.sum((1, 2)), (mask & (t_im > 0)).sum((1, 2)), visib.sum((1, 2))
    fract = torch.where(n_all > 0, n_visib.double() / n_all.double().clamp(min=1), torch.zeros_like(n_all, dtype=torch.float64))

    def box(m, ox, oy):
        cols, rows = m.any(1), m.any(2)
        nx, ny = cols.shape[1], rows.shape[1]
        ix, iy = torch.arange(nx, device=dev), torch.arange(ny, device=dev)
        x0 = torch.where(cols, ix, nx).amin(1) - ox
        x1 = torch.where(cols, ix, -1).amax(1) - ox
        y0 = torch.where(rows, iy, ny).amin(1) - oy
        y1 = torch.where(rows, iy, -1).amax(1) - oy
        b = torch.stack([x0, y0, x1 - x0, y1 - y0], 1)
        return torch.where((n_visib > 0)[:, None], b, torch.full_like(b, -1))

    return {"px_count_all": n_all, "px_count_valid": n_valid, "px_count_visib": n_visib, "visib_fract": fract, "bbox_obj": box(obj, W, H),
            "bbox_visib": box(visib, 0, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_info_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    R = np.stack([S_rot(rng) for _ in range(256)])
    t = np.stack([rng.uniform(-260, 260, 256), rng.uniform(-190, 190, 256), rng.uniform(350, 600, 256)], 1)     # some cut by the frame's edge
    depth = (300.0 + 400.0 * rng.random((4, H, W))).astype(np.float32)
    depth[rng.random(depth.shape) < 0.1] = 0.0
    depth_dev = torch.from_numpy(depth).to(dev)
    K = torch.from_numpy(LM_K)
    levels = {1280: 3, 20480: 5}
    shapes = [(B, F) for F in (1280, 20480) for B in (1, 32, 256)]
    calls, warmup = a.calls, a.warmup
    if a.quick:
        shapes, calls, warmup = [(32, 1280), (256, 20480)], 3, 1
    rows = []
    for B, F in shapes:
        v, f = S._icosphere(levels[F], 50.0)
        ms = metric.MeshSet.from_arrays([v.astype(np.float32)], diameters=[100.0], faces=[f])
        up = lambda x, s: torch.from_numpy(np.ascontiguousarray(x[:B].reshape(s))).to(dev)   # noqa: E731
        Rd, td = up(R, (B, 3, 3)), up(t, (B, 3, 1))
        ids = torch.arange(B, dtype=torch.int32, device=dev) % 4
        fused = GI.gt_info(Rd, td, LM_K, ms, depth_dev, image_ids=ids)
        comp = composed(Rd, td, K, ms, depth_dev, ids)
        agree = {k: int((fused[k].to(comp[k].dtype) == comp[k]).reshape(B, -1).all(1).sum()) for k in comp}
        t_f = timed(lambda: GI.gt_info(Rd, td, LM_K, ms, depth_dev, image_ids=ids), calls, warmup)
        t_m = timed(lambda: GI.gt_info(Rd, td, LM_K, ms, depth_dev, image_ids=ids, return_masks=True), calls, warmup)
        t_c = timed(lambda: composed(Rd, td, K, ms, depth_dev, ids), calls if B < 256 else max(3, calls // 10), warmup if B < 256 else 2)
        row = {"B": B, "F": F, "V": int(v.shape[0]), "fused_ms": t_f, "fused_with_masks_ms": t_m, "composed_ms": t_c, "ratio": t_c / t_f,
               "ms_per_pose": t_f / B, "poses_agreeing_with_composition": agree, "visible_pixels_pose0": int(fused["px_count_visib"][0])}
        rows.append(row)
        print("B=%3d F=%5d: fused %.3f ms (%.3f with masks), composed %.3f ms, ratio %.2f; poses agreeing %s"
              % (B, F, t_f, t_m, t_c, t_c / t_f, agree), flush=True)
        del comp
        torch.cuda.empty_cache()
    res = {"bench": "gt_info", "device": torch.cuda.get_device_name(0), "calls": calls, "warmup": warmup, "frame": [W, H],
           "baseline": "metric.render_depth on the 3W x 3H canvas + torch elementwise operations and reductions (tools/gt_info_bench.py: composed); "
                       "at B = 256 it is timed over calls / 10 calls", "rows": rows}
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
