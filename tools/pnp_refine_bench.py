"""micro-benchmark of postprocess.refine_poses_lm (cp_pnp_refine_lm) beside solve_pnp_ransac (row N4), tools/pnp_gc_bench.py's method.

  python tools/pnp_refine_bench.py [--out profiles/pnp_refine_bench.json] [--windows 3] [--warmup 1] [--crops 64]
  python tools/pnp_refine_bench.py --resources          (only where hipcc is: adds the compiler's figures of the new kernel to the file)

Time: device events around the WHOLE Python call (buffers allocated, the pose packed), after `--warmup` warm-up calls; the figure is the
median of `--windows` windows of one call each, the windows are kept.  refine_poses_lm at its defaults (20 iterations, step_tol 1e-10) over
the inliers of solve_pnp_ransac at its defaults, both on the same batches: B = 32, N = 512 on the LM-O ape, and B = 8, N = 4096 on LM
object 8.  Crops: 0.5 px noise, 30 % outliers, all keypoints valid.
Accuracy: pnp_gc_bench.make_crops' scattered and clustered sets (`--crops` seeded crops, N = 512, ape, 0.5 px noise, 30 % outliers):
median rotation error (degrees) and translation error (% of |t|) of solve_pnp_ransac before and after the refinement, the status counts
and the histogram of iterations run.
No speed and no accuracy gain is required of this row and nothing is fixed in advance; the file holds what was measured."""
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

KERNELS = ("pnp_refine_lm_kernel",)


def kernel_resources():
    src = os.path.join(ROOT, "checkerpose_amd", "csrc", "pnp_refine.hip")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_refine_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--crops", type=int, default=64)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "pnp_refine", "timing": "UNMEASURED", "accuracy": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from pnp_gc_bench import device_call_ms, make_crops, pose_errors
    from checkerpose_amd import _abi
    from checkerpose_amd.postprocess import refine_poses_lm, solve_pnp_ransac
    from tests.pnp_stages import DATA, K_LMO, lmo_model
    lib = _abi.load()
    dev = torch.device("cuda:0")
    K = torch.from_numpy(K_LMO).float().to(dev)
    models = {"lmo_ape_512": lmo_model(512), "lm_obj8_4096": np.load(os.path.join(DATA, "fps_lm_15x4096.npy"))[7].astype(np.float32).astype(np.float64)}
    timing = []
    for name, B in (("lmo_ape_512", 32), ("lm_obj8_4096", 8)):
        xyz = models[name]
        N = len(xyz)
        p2d, _, _ = make_crops(np.random.default_rng(5), xyz, K_LMO, B, False)
        p3 = torch.from_numpy(xyz).float().to(dev)
        p2 = torch.from_numpy(p2d).to(dev)
        valid = torch.ones(B, N, 3, dtype=torch.uint8, device=dev)
        R, t, inl, status = solve_pnp_ransac(p3, p2, valid, K)
        row = {"model": name, "B": B, "N": N, "median_inliers": float(np.median(inl.sum(1).cpu().numpy()))}
        for label, fn in (("refine_lm", lambda: refine_poses_lm(p3, p2, inl, K, R, t, status=status)),
                          ("epnp", lambda: solve_pnp_ransac(p3, p2, valid, K))):
            for _ in range(a.warmup):
                fn()
            wins = [device_call_ms(fn) for _ in range(a.windows)]
            row[label + "_ms"], row[label + "_windows_ms"] = float(np.median(wins)), wins
        out = refine_poses_lm(p3, p2, inl, K, R, t, status=status)
        row["refine_lm_status_counts"] = {str(k): int((out[2] == k).sum()) for k in range(4)}
        row["refine_lm_iterations"] = out[3]["iters"].cpu().tolist()
        print("%s B=%d N=%d: refine_lm %.3f ms %s, epnp %.3f ms %s" % (name, B, N, row["refine_lm_ms"], row["refine_lm_windows_ms"], row["epnp_ms"],
                                                                        row["epnp_windows_ms"]), flush=True)
        timing.append(row)
    accuracy = []
    xyz = models["lmo_ape_512"]
    p3 = torch.from_numpy(xyz).float().to(dev)
    for kind in ("scattered", "clustered"):
        p2d, Rt, tt = make_crops(np.random.default_rng(6), xyz, K_LMO, a.crops, kind == "clustered")
        p2 = torch.from_numpy(p2d).to(dev)
        valid = torch.ones(a.crops, 512, 3, dtype=torch.uint8, device=dev)
        R, t, inl, status = solve_pnp_ransac(p3, p2, valid, K)
        R2, t2, st2, info = refine_poses_lm(p3, p2, inl, K, R, t, status=status)
        row = {"outliers": kind, "crops": a.crops, "N": 512, "noise_px": 0.5, "outlier_fraction": 0.3,
               "identity_fallbacks": int((status == 0).sum()), "median_inliers": float(np.median(inl.sum(1).cpu().numpy()))}
        for label, (Rx, tx) in (("epnp", (R, t)), ("epnp_refine_lm", (R2, t2))):
            eR, et = pose_errors(Rx.cpu().numpy(), tx.cpu().numpy()[:, :, 0], Rt, tt)
            row[label] = {"median_rotation_error_deg": float(np.median(eR)), "median_translation_error_percent": float(np.median(et))}
        iters = info["iters"].cpu().numpy()
        row["refine_status_counts"] = {str(k): int((st2 == k).sum()) for k in range(4)}
        row["iterations_histogram"] = {str(k): int((iters == k).sum()) for k in sorted(set(iters.tolist()))}
        ok = (st2 != 0).cpu().numpy()
        row["median_cost_before_px2"] = float(np.median(info["cost0"].cpu().numpy()[ok])) if ok.any() else "UNMEASURED"
        row["median_cost_after_px2"] = float(np.median(info["cost"].cpu().numpy()[ok])) if ok.any() else "UNMEASURED"
        print(kind, json.dumps({k: v for k, v in row.items() if isinstance(v, dict)}), flush=True)
        accuracy.append(row)
    res = {"bench": "pnp_refine", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()),
           "method": "device events around the whole call (allocations, packing of the pose), median of one-call windows after warm-ups; "
                     "refine_poses_lm at its defaults over the inliers of solve_pnp_ransac at its defaults, on the same batches",
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
