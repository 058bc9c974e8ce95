"""micro-benchmark of postprocess.refine_poses_icp (cp_surface_samples + cp_icp_refine), tools/pnp_refine_bench.py's method.

  python tools/icp_bench.py [--out profiles/icp_bench.json] [--windows 3] [--warmup 1] [--poses 256]
  python tools/icp_bench.py --resources          (only where hipcc is: adds the compiler's figures of the new kernels to the file)

Time: device events around the WHOLE Python call (the render of the samples, buffers allocated, the poses packed), after `--warmup`
warm-up calls; the figure is the median of `--windows` windows of one call each, the windows are kept.  refine_poses_icp at its defaults
(20 iterations, step_tol 1e-6, inertia 1e-2) with grid 32 and 64 on P = 256 poses, 640 x 480 frames: 8 images, each the device's own
render of one object (torus, ico1280, box, halfbox in turn) at a random pose about 700 mm away with a far plane behind it; every pose
starts 4 degrees and 4 % of the distance along the ray off its image's truth; max_dist = 0.3 diameters.  The call with `samples=` given
(stages B and C alone) and surface_samples alone are timed beside it.
For orientation only, the numpy restatement's (tests/icp_stages.refine) time per pose on the host, over the device's own samples of
the first poses.  Accuracy: the median ADD in % of the diameter before and after, the status counts, the iterations.
NOTHING is required of this row and nothing is fixed in advance; the file holds what was measured."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("icp_pose_kernel", "icp_vertex_kernel", "icp_tile_kernel", "icp_finish_kernel", "icp_refine_kernel")


def kernel_resources():
    src = os.path.join(ROOT, "checkerpose_amd", "csrc", "icp_refine.hip")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--host-poses", type=int, default=4)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "icp_refine", "timing": "UNMEASURED", "accuracy": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from pnp_gc_bench import device_call_ms
    from checkerpose_amd import _abi, metric
    from checkerpose_amd.postprocess import refine_poses_icp, surface_samples
    from tests import icp_stages as I
    from tests.pnp_stages import K_LMO
    lib = _abi.load()
    dev = torch.device("cuda:0")
    W, H, n_img, P = 640, 480, 8, a.poses
    names = ("torus", "ico1280", "box", "halfbox")
    v, f = I.mesh_arrays(names)
    diam = I.diameters(names)
    ms = metric.MeshSet.from_arrays(v, diameters=diam, faces=f)
    rng = np.random.default_rng(24)
    Rt = np.stack([I._random_rotation(rng) for _ in range(n_img)])
    tt = np.stack([[rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(650, 750)] for _ in range(n_img)])
    img_mesh = np.arange(n_img) % len(names)
    K = torch.from_numpy(K_LMO).to(dev)
    depth = metric.render_depth(torch.from_numpy(Rt).to(dev), torch.from_numpy(tt).to(dev), K, ms, (W, H), mesh_ids=img_mesh)
    depth = torch.where(depth > 0, depth, torch.full_like(depth, 2000.0))
    image_ids = np.arange(P) % n_img
    mesh_ids = img_mesh[image_ids]
    R0 = np.stack([I._rodrigues(rng.normal(size=3), np.radians(4.0)) @ Rt[i] for i in image_ids])
    t0 = np.stack([tt[i] * (1.0 + 0.04 * (1.0 if rng.random() < 0.5 else -1.0)) for i in image_ids])
    R0d, t0d = torch.from_numpy(R0).to(dev), torch.from_numpy(t0).to(dev)
    max_dist = torch.from_numpy(0.3 * diam[mesh_ids]).to(dev)
    kw = dict(image_ids=image_ids, mesh_ids=mesh_ids)

    def add_percent(R, t):
        e = metric.pose_errors(R, t, Rt[image_ids], tt[image_ids], ms, mesh_ids=mesh_ids, kinds=("add",))["add"].cpu().numpy()
        return 100.0 * e / diam[mesh_ids]

    timing = []
    for grid in (32, 64):
        smp = surface_samples(R0d, t0d, K, ms, (W, H), mesh_ids=mesh_ids, grid=grid)
        row = {"P": P, "frame": [W, H], "images": n_img, "grid": grid, "median_samples": float(np.median((smp["face"] >= 0).sum(1).cpu().numpy()))}
        for label, fn in (("refine_poses_icp", lambda: refine_poses_icp(R0d, t0d, K, ms, depth, max_dist, grid=grid, **kw)),
                          ("refine_poses_icp_samples_given", lambda: refine_poses_icp(R0d, t0d, K, ms, depth, max_dist, samples=smp, **kw)),
                          ("surface_samples", lambda: surface_samples(R0d, t0d, K, ms, (W, H), mesh_ids=mesh_ids, grid=grid))):
            for _ in range(a.warmup):
                fn()
            wins = [device_call_ms(fn) for _ in range(a.windows)]
            row[label + "_ms"], row[label + "_windows_ms"] = float(np.median(wins)), wins
        R, t, st, info = refine_poses_icp(R0d, t0d, K, ms, depth, max_dist, samples=smp, **kw)
        row["status_counts"] = {str(k): int((st == k).sum()) for k in range(4)}
        iters = info["iters"].cpu().numpy()
        row["iterations_histogram"] = {str(k): int((iters == k).sum()) for k in sorted(set(iters.tolist()))}
        row["median_pairs"] = float(np.median(info["n"].cpu().numpy()))
        row["median_add_percent_of_diameter"] = {"before": float(np.median(add_percent(R0d, t0d))), "after": float(np.median(add_percent(R, t)))}
        # the numpy restatement on the host, over the device's own samples of the first poses
        host = {k: smp[k][:a.host_poses].cpu().numpy() for k in ("X", "N", "face")}
        dep = depth.cpu().numpy()
        t_host = time.perf_counter()
        for b in range(a.host_poses):
            I.refine(host["X"][b], host["N"][b], host["face"][b], K_LMO, R0[b], t0[b], dep[image_ids[b]], float(max_dist[b]), diam[mesh_ids[b]] / 2.0)
        row["numpy_restatement_ms_per_pose"] = 1e3 * (time.perf_counter() - t_host) / a.host_poses
        print("grid %d: refine_poses_icp %.3f ms %s, samples given %.3f ms, surface_samples %.3f ms; numpy %.1f ms per pose; ADD %% %s status %s" % (
            grid, row["refine_poses_icp_ms"], row["refine_poses_icp_windows_ms"], row["refine_poses_icp_samples_given_ms"], row["surface_samples_ms"],
            row["numpy_restatement_ms_per_pose"], row["median_add_percent_of_diameter"], row["status_counts"]), flush=True)
        timing.append(row)
    res = {"bench": "icp_refine", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()),
           "method": "device events around the whole call (render of the samples, allocations, packing of the poses), median of one-call windows "
                     "after warm-ups; refine_poses_icp at its defaults; the numpy figure is tests/icp_stages.refine on the host, for orientation only",
           "timing": timing, "kernel_resources": "UNMEASURED"}
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
