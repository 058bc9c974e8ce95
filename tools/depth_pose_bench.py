"""micro-benchmark of postprocess.solve_pose_depth (cp_pose_depth_ransac) beside solve_pnp_ransac on the SAME
correspondences, tools/icp_bench.py's method.

  python tools/depth_pose_bench.py [--out profiles/depth_pose_bench.json] [--windows 3] [--warmup 1] [--crops 256] [--points 512]
  python tools/depth_pose_bench.py --resources     (only where hipcc is: adds the compiler's figures of the new kernels to the file)

Time: device events around the WHOLE Python call (buffers allocated, the lift included), after `--warmup` warm-up calls; the figure is
the median of `--windows` windows of one call each, the windows are kept.  Both solvers at 150 iterations, B = 256 crops of N = 512
keypoints on 640 x 480 frames.
The set: 8 images, each one object (farthest-point keypoints of three LM objects in turn) at a random pose about 700 mm away; the p2d
are the true projections quantised to the 64-cell grid of the object's box, as `correspondences` gives them; 30 % of a crop's
correspondences carry a wrong code (a random cell of the box), 80 % are valid; the sensor's depth is a z-buffer of the keypoints' own
depths over a 3 x 3 footprint in front of a plane at twice the distance.  dist_threshold = 6 (mm), reproj_threshold = 2 (pixels).
Accuracy: the median ADD over the keypoints and the median translation error along the viewing ray |(t - t_gt) . t_gt / |t_gt||, for
both solvers.  NOTHING is required of this row and nothing is fixed in advance; the file holds what was measured."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("pose_depth_lift_kernel", "pose_depth_ransac_kernel")


def kernel_resources():
    src = os.path.join(ROOT, "checkerpose_amd", "csrc", "pose_depth.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c", src, "-o", os.devnull,
                              "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900).stderr
    except (OSError, subprocess.SubprocessError):
        return "UNMEASURED"
    res = {}
    for block in out.split("Function Name: ")[1:]:
        name = next((k for k in KERNELS if k in block.split()[0]), None)
        if name is None:
            continue
        fig = {}
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                         ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"), ("static_lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, block)
            fig[key] = int(m.group(1)) if m else "UNMEASURED"
        res[name] = fig
    return res or "UNMEASURED"


def build_set(B, N, n_img, W, H, K, seed=25):
    """-> (p3d (B,N,3) f32, p2d (B,N,2) f32, valid (B,N,3) uint8, depth (n_img,H,W) f32, image_ids (B,), R_gt (B,3,3), t_gt (B,3))"""
    from tests import depth_pose_stages as D
    rng = np.random.default_rng(seed)
    depth = np.zeros((n_img, H, W), np.float32)
    models = [D.model(o, N) for o in (0, 7, 14)]
    poses, clean, boxes = [], [], []
    for i in range(n_img):
        X = models[i % 3].astype(np.float64)
        R = D._rotation(rng)
        t = np.array([rng.uniform(-120, 120), rng.uniform(-80, 80), rng.uniform(650, 750)])
        C = X @ R.T + t
        uv = np.stack([K[0, 0] * C[:, 0] / C[:, 2] + K[0, 2], K[1, 1] * C[:, 1] / C[:, 2] + K[1, 2]], 1)
        q = D.quantise(uv)
        depth[i] = np.float32(2.0 * t[2])
        zbuf = np.full((H, W), np.inf, np.float32)
        for (u, v), z in zip(q, C[:, 2].astype(np.float32)):
            x, y = int(np.floor(u)), int(np.floor(v))
            zbuf[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = np.minimum(zbuf[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2], z)
        depth[i][np.isfinite(zbuf)] = zbuf[np.isfinite(zbuf)]
        poses.append((R, t))
        clean.append(q)
        boxes.append((q[:, 0].min(), q[:, 1].min(), q[:, 0].max(), q[:, 1].max()))
    image_ids = np.arange(B) % n_img
    p3d = np.stack([models[i % 3] for i in image_ids])
    p2d = np.stack([clean[i] for i in image_ids]).copy()
    valid = np.zeros((B, N, 3), np.uint8)
    for b in range(B):
        wrong = rng.random(N) < 0.3
        x0, y0, x1, y1 = boxes[image_ids[b]]
        cells = rng.integers(0, 64, size=(int(wrong.sum()), 2))
        p2d[b, wrong, 0] = (x0 + (x1 - x0) * cells[:, 0] / 63.0).astype(np.float32)
        p2d[b, wrong, 1] = (y0 + (y1 - y0) * cells[:, 1] / 63.0).astype(np.float32)
        valid[b, :, 0] = rng.random(N) < 0.8
    return (p3d, p2d, valid, depth, image_ids, np.stack([poses[i][0] for i in image_ids]), np.stack([poses[i][1] for i in image_ids]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_pose_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--crops", type=int, default=256)
    ap.add_argument("--points", type=int, default=512)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "pose_depth", "timing": "UNMEASURED", "accuracy": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from pnp_gc_bench import device_call_ms
    from checkerpose_amd import _abi
    from checkerpose_amd.postprocess import lift_correspondences, solve_pnp_ransac, solve_pose_depth
    from tests.pnp_stages import K_LMO
    lib = _abi.load()
    dev = torch.device("cuda:0")
    W, H, n_img, B, N = 640, 480, 8, a.crops, a.points
    K = K_LMO.astype(np.float32)
    p3d, p2d, valid, depth, image_ids, Rg, tg = build_set(B, N, n_img, W, H, K.astype(np.float64))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)            # noqa: E731
    d3, d2, dv, dd, dK = up(p3d), up(p2d), up(valid), up(depth), up(K)
    thr, rthr, iters = 6.0, 2.0, 150
    calls = (("solve_pose_depth", lambda: solve_pose_depth(d3, d2, dv, dK, dd, thr, image_ids=image_ids, iterations=iters, seed=1)),
             ("solve_pnp_ransac", lambda: solve_pnp_ransac(d3, d2, dv, dK, reproj_threshold=rthr, iterations=iters, seed=1)),
             ("lift_correspondences", lambda: lift_correspondences(d2, dv, dK, dd, image_ids=image_ids)))
    timing = {"B": B, "N": N, "frame": [W, H], "images": n_img, "iterations": iters}
    for label, fn in calls:
        for _ in range(a.warmup):
            fn()
        wins = [device_call_ms(fn) for _ in range(a.windows)]
        timing[label + "_ms"], timing[label + "_windows_ms"] = float(np.median(wins)), wins
    accuracy = {"dist_threshold": thr, "reproj_threshold": rthr, "wrong_codes": 0.3, "valid": 0.8}
    ray = tg / np.linalg.norm(tg, axis=1, keepdims=True)
    for label, fn in calls[:2]:
        R, t, inl, status = [x.cpu().numpy() for x in fn()[:4]]
        t = t[:, :, 0]
        add = np.array([np.linalg.norm((p3d[b].astype(np.float64) @ R[b].T + t[b]) - (p3d[b].astype(np.float64) @ Rg[b].T + tg[b]), axis=1).mean() for b in range(B)])
        along = np.abs(((t - tg) * ray).sum(1))
        accuracy[label] = {"solved": int((status == 1).sum()), "median_add": float(np.median(add)), "p90_add": float(np.quantile(add, 0.9)),
                           "median_error_along_ray": float(np.median(along)), "p90_error_along_ray": float(np.quantile(along, 0.9)),
                           "median_inliers": float(np.median(inl.sum(1)))}
    n_lifted = lift_correspondences(d2, dv, dK, dd, image_ids=image_ids)[2].cpu().numpy()
    accuracy["median_lifted"] = float(np.median(n_lifted))
    print("B %d N %d: solve_pose_depth %.3f ms %s, solve_pnp_ransac %.3f ms %s, lift alone %.3f ms" % (
        B, N, timing["solve_pose_depth_ms"], timing["solve_pose_depth_windows_ms"], timing["solve_pnp_ransac_ms"], timing["solve_pnp_ransac_windows_ms"],
        timing["lift_correspondences_ms"]), flush=True)
    print("accuracy: %s" % json.dumps(accuracy), flush=True)
    res = {"bench": "pose_depth", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()),
           "method": "device events around the whole call (allocations and the lift included), median of one-call windows after warm-ups; both "
                     "solvers on the same correspondences at 150 iterations; units of the errors: the keypoints' (mm)",
           "timing": timing, "accuracy": accuracy, "kernel_resources": "UNMEASURED"}
    if os.path.exists(a.out):
        old = json.load(open(a.out))
        if old.get("kernel_resources", "UNMEASURED") != "UNMEASURED":
            res["kernel_resources"] = old["kernel_resources"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
