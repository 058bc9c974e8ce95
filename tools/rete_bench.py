"""micro-benchmark of targets.pose_re_te_sym (cp_pose_rete) beside the numpy restatement of the reference's
get_closest_rot loop on the host, tools/pnp_refine_bench.py's method.

  python tools/rete_bench.py [--out profiles/rete_bench.json] [--windows 3] [--warmup 1] [--host-pairs 32]
  python tools/rete_bench.py --resources          (only where hipcc is: adds the compiler's figures of the two kernels to the file)

P = 4096 pose pairs (the estimate within a few hundredths of a radian of a symmetric copy of the ground truth) against ONE symmetry
set per run, S = 1 (the identity), 2 (a half turn), 314 (a continuous axis), 628 (a continuous axis and a flip): the sets of
SymmetrySet.from_models_info(rotations_as=np.float32).  Time: device events around the WHOLE Python call (packing of the poses, the
output buffers; the set is already on the device), after `--warmup` warm-up calls; the figure is the median of `--windows` windows of
one call each, the windows are kept.  Host: what test_lm.py does per pose -- a loop over the set with one np.linalg.inv and one
trace per member, strict `<` -- restated here in numpy, wall clock over the first `--host-pairs` of the same pairs, scaled to per
pose.  Nothing is required of these numbers; the file holds what was measured."""
import argparse
import json
import math
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("pose_rete_kernel", "rete_pass_counts_kernel")
INFOS = {1: {"diameter": 100.0},
         2: {"diameter": 100.0, "symmetries_discrete": [[-1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0]]},
         314: {"diameter": 100.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [3.5, -2.0, 0.0]}]},
         628: {"diameter": 100.0, "symmetries_continuous": [{"axis": [0, 1, 0], "offset": [0, 0, 0]}],
               "symmetries_discrete": [[1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, -1.0, 1.5, 0, 0, 0, 1.0]]}}


def kernel_resources():
    src = os.path.join(ROOT, "checkerpose_amd", "csrc", "rete.hip")
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


def host_closest_re(R_est, R_gt, syms):
    """test_lm.py's per-pose work, restated: re against the plain ground truth, then one inverse and one trace per member"""
    def re_of(Re, Rg):
        c = float(0.5 * (np.trace(Re.dot(np.linalg.inv(Rg))) - 1.0))
        return 180.0 * math.acos(min(1.0, max(-1.0, c))) / np.pi
    best = re_of(R_est, R_gt)
    for S in syms:
        cur = re_of(R_est, R_gt.dot(S))
        if cur < best:
            best = cur
    return best


def _uniform_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def _small_rotation(rng):
    a = rng.normal(size=3)
    th = rng.uniform(0.01, 0.06)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rete_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--host-pairs", type=int, default=32)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "rete", "timing": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from pnp_gc_bench import device_call_ms
    from checkerpose_amd import _abi
    from checkerpose_amd.scene import SymmetrySet
    from checkerpose_amd.targets import pose_re_te_sym
    lib = _abi.load()
    dev = torch.device("cuda:0")
    P = a.pairs
    timing = []
    for S, info in INFOS.items():
        ss = SymmetrySet.from_models_info([info], rotations_as=np.float32)
        syms = ss.table.numpy()[:, :9].reshape(-1, 3, 3)
        assert len(syms) == S
        rng = np.random.default_rng(S)
        R_gt = np.stack([_uniform_rotation(rng) for _ in range(P)])
        R_est = np.stack([_small_rotation(rng) @ R_gt[p].dot(syms[int(rng.integers(S))]) for p in range(P)])
        t_gt = rng.uniform(-100, 100, size=(P, 3)) + np.array([0.0, 0.0, 800.0])
        t_est = t_gt + rng.normal(size=(P, 3)) * 10.0
        d = [torch.from_numpy(x).to(dev) for x in (R_est, t_est, R_gt, t_gt)]
        ss.on(dev)
        fn = lambda: pose_re_te_sym(*d, symmetries=ss)               # noqa: E731
        for _ in range(a.warmup):
            fn()
        wins = [device_call_ms(fn) for _ in range(a.windows)]
        re_dev = fn()[0].cpu().numpy()
        n = min(a.host_pairs, P)
        t0 = time.perf_counter()
        re_host = np.array([host_closest_re(R_est[p], R_gt[p], syms) for p in range(n)])
        host_s = time.perf_counter() - t0
        row = {"S": S, "P": P, "device_ms": float(np.median(wins)), "device_windows_ms": wins, "device_us_per_pose": 1e3 * float(np.median(wins)) / P,
               "host_pairs": n, "host_ms_per_pose": 1e3 * host_s / n, "max_abs_re_difference_deg_on_host_pairs": float(np.abs(re_dev[:n] - re_host).max())}
        print("S=%d P=%d: device %.3f ms %s (%.3f us per pose), host %.3f ms per pose over %d" % (
            S, P, row["device_ms"], wins, row["device_us_per_pose"], row["host_ms_per_pose"], n), flush=True)
        timing.append(row)
    res = {"bench": "rete", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()),
           "method": "device events around the whole pose_re_te_sym call (poses packed, outputs allocated; the set already on the device), "
                     "median of one-call windows after warm-ups; host: the per-pose loop of get_closest_rot restated in numpy, wall clock "
                     "over the first host_pairs pairs", "timing": timing, "kernel_resources": "UNMEASURED"}
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
