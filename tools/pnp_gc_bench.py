"""micro-benchmark of postprocess.solve_pnp_gc (cp_pnp_gc) beside solve_pnp_ransac (row N4), tools/visibility_bench.py's method.

  python tools/pnp_gc_bench.py [--out profiles/pnp_gc_bench.json] [--windows 3] [--warmup 1] [--crops 64]
  python tools/pnp_gc_bench.py --resources          (only where hipcc is: adds the compiler's figures of the new kernels to the file)

Time: device events around the WHOLE Python call (scratch allocated, the status read back), after `--warmup` warm-up calls; the figure
is the median of `--windows` windows of one call each, the windows are kept.  Both solvers on the same batches at their defaults
(gc: 400 iterations, lambda 0.1, radius 20; epnp: 150 iterations): B = 32, N = 512 on the LM-O ape's graph, and B = 8, N = 4096 on LM
object 8's.  Crops: 0.5 px noise, 30 % outliers, all keypoints valid.
Accuracy: `--crops` seeded crops (N = 512, ape), 0.5 px noise, 30 % outliers -- once scattered over the model, once clustered on one
patch of it (the keypoints nearest to a random keypoint) -- median rotation error (degrees) and translation error (% of |t|) of both
solvers over the crops, identity fallbacks (status 0) included as the reference scores them, and the number of fallbacks.
The graph-cut solver is recorded twice: at its default spatial_coherence_weight 0.1 ("gc") and at `--lam-extra` (0.02).
No speed or accuracy is required of this row and nothing is fixed in advance; the file holds what was measured."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("radius_graph_count_kernel", "radius_graph_fill_kernel", "graphcut_label_kernel", "gc_hypotheses_kernel", "gc_select_lo_kernel")


def kernel_resources():
    src = os.path.join(ROOT, "checkerpose_amd", "csrc", "pnp_gc.hip")
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


def device_call_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def make_crops(rng, xyz, K, B, clustered, outlier_frac=0.3, noise=0.5):
    """-> (p2d (B,N,2) f32, R (B,3,3), t (B,3))"""
    from tests.pnp_stages import _pose
    from oracle.pnp_oracle import project
    n = len(xyz)
    p2d, Rs, ts = [], [], []
    for _ in range(B):
        R, t = _pose(rng)
        uv = project(xyz, K, R, t) + rng.normal(scale=noise, size=(n, 2))
        k = int(round(outlier_frac * n))
        if clustered:
            out = np.argsort(((xyz - xyz[rng.integers(n)]) ** 2).sum(1))[:k]
        else:
            out = rng.permutation(n)[:k]
        uv[out] += rng.uniform(20, 80, size=(k, 2)) * rng.choice([-1, 1], size=(k, 2))
        p2d.append(uv)
        Rs.append(R)
        ts.append(t)
    return np.stack(p2d).astype(np.float32), np.stack(Rs), np.stack(ts)


def pose_errors(R, t, Rt, tt):
    cos = np.clip((np.einsum("bij,bij->b", R, Rt) - 1.0) / 2.0, -1.0, 1.0)
    return np.degrees(np.arccos(cos)), 100.0 * np.linalg.norm(t - tt, axis=1) / np.linalg.norm(tt, axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_gc_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--crops", type=int, default=64)
    ap.add_argument("--lam-extra", type=float, default=0.02, help="a second spatial_coherence_weight, recorded beside the default 0.1")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "pnp_gc", "timing": "UNMEASURED", "accuracy": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from checkerpose_amd import _abi
    from checkerpose_amd.postprocess import radius_graph, solve_pnp_gc, solve_pnp_ransac
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
        graph_ms = device_call_ms(lambda: radius_graph(p3, 20.0))          # first touch included: once per object
        graph = radius_graph(p3, 20.0)
        row = {"model": name, "B": B, "N": N, "directed_edges": graph.totals[0], "radius_graph_first_call_ms": graph_ms,
               "radius_graph_ms": device_call_ms(lambda: radius_graph(p3, 20.0))}
        for label, fn in (("gc", lambda: solve_pnp_gc(p3, p2, valid, K, graph)),
                          ("gc_lam_%g" % a.lam_extra, lambda: solve_pnp_gc(p3, p2, valid, K, graph, spatial_coherence_weight=a.lam_extra)),
                          ("epnp", lambda: solve_pnp_ransac(p3, p2, valid, K))):
            for _ in range(a.warmup):
                fn()
            wins = [device_call_ms(fn) for _ in range(a.windows)]
            row[label + "_ms"], row[label + "_windows_ms"] = float(np.median(wins)), wins
            row[label + "_status1"] = int(fn()[3].sum())
        print("%s B=%d N=%d: gc %.2f ms %s, epnp %.2f ms %s" % (name, B, N, row["gc_ms"], row["gc_windows_ms"], row["epnp_ms"], row["epnp_windows_ms"]), flush=True)
        lx = "gc_lam_%g" % a.lam_extra
        print("   gc at lambda %g: %.2f ms %s, status 1 on %d" % (a.lam_extra, row[lx + "_ms"], row[lx + "_windows_ms"], row[lx + "_status1"]), flush=True)
        timing.append(row)
    accuracy = []
    xyz = models["lmo_ape_512"]
    p3 = torch.from_numpy(xyz).float().to(dev)
    graph = radius_graph(p3, 20.0)
    for kind in ("scattered", "clustered"):
        p2d, Rt, tt = make_crops(np.random.default_rng(6), xyz, K_LMO, a.crops, kind == "clustered")
        p2 = torch.from_numpy(p2d).to(dev)
        valid = torch.ones(a.crops, 512, 3, dtype=torch.uint8, device=dev)
        row = {"outliers": kind, "crops": a.crops, "N": 512, "noise_px": 0.5, "outlier_fraction": 0.3}
        for label, fn in (("gc", lambda: solve_pnp_gc(p3, p2, valid, K, graph)),
                          ("gc_lam_%g" % a.lam_extra, lambda: solve_pnp_gc(p3, p2, valid, K, graph, spatial_coherence_weight=a.lam_extra)),
                          ("epnp", lambda: solve_pnp_ransac(p3, p2, valid, K))):
            R, t, inl, status = fn()
            eR, et = pose_errors(R.cpu().numpy(), t.cpu().numpy()[:, :, 0], Rt, tt)
            row[label] = {"median_rotation_error_deg": float(np.median(eR)), "median_translation_error_percent": float(np.median(et)),
                          "identity_fallbacks": int((status == 0).sum()), "median_inliers": float(np.median(inl.sum(1).cpu().numpy()))}
        print(kind, json.dumps({k: v for k, v in row.items() if isinstance(v, dict)}), flush=True)
        accuracy.append(row)
    res = {"bench": "pnp_gc", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()),
           "method": "device events around the whole solver call (allocations, the status read-back), median of one-call windows after warm-ups; "
                     "both solvers at their defaults on the same batches", "timing": timing, "accuracy": accuracy, "kernel_resources": "UNMEASURED"}
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
