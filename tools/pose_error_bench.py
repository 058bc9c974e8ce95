"""micro-benchmark of metric.pose_errors (cp_pose_errors) against the host path a user has today: numpy + scipy.spatial.cKDTree,
one pose at a time (the restatement of bop_toolkit_lib.pose_error.add / .adi in tests/test_pose_error.py), threads as the box sets them.

  python tools/pose_error_bench.py [--out profiles/pose_error_bench.json] [--host-poses 8]

Device: events around 5 calls after 2 warm-ups, for B in {1, 32, 256} x V in {4096, 20480, 61440} (vertices: the LM surface samples
of checkerpose_amd/data/fps_lm_15x4096.npy, the first V rows).  Host: at V = 4096 all 256 poses of the batch are timed; at the larger
meshes the mean over `--host-poses` poses, SCALED to B (the loop is one independent call per pose) -- `host_adi_poses_timed` in every
row says which.  Writes both times, their ratio and the achieved pair evaluations per second, and prints the JSON line.  No speed-up is promised: the parent commit has no device path, so the host path
is the comparison."""
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
from tests.test_pose_error import host_add, host_adi, lm_table  # noqa: E402


def poses(rng, B):
    R_gt = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(B)])
    R_gt *= np.sign(np.linalg.det(R_gt))[:, None, None]
    t_gt = np.stack([rng.uniform(-100, 100, B), rng.uniform(-100, 100, B), rng.uniform(400, 1500, B)], 1)
    ax = rng.normal(size=(B, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    Kx = np.zeros((B, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    th = np.deg2rad(2.0)                                  # estimates 2 degrees and about 5 mm off: the regime the metric is used in
    small = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    return small @ R_gt, t_gt + rng.normal(scale=3.0, size=(B, 3)), R_gt, t_gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_error_bench.json"))
    ap.add_argument("--host-poses", type=int, default=8)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    table = lm_table()
    rng = np.random.default_rng(0)
    rows = []
    for V in (4096, 20480, 61440):
        pts = np.ascontiguousarray(table[:V])
        ms = metric.MeshSet.from_arrays([pts], diameters=[1.0])
        Re, te, Rg, tg = poses(rng, 256)
        host_adi(Re[0], te[0], Rg[0], tg[0], pts)                # warm-up: imports scipy, touches the pages
        t0 = time.perf_counter()
        n_host = 256 if V == 4096 else a.host_poses
        for b in range(n_host):
            host_adi(Re[b], te[b], Rg[b], tg[b], pts)
        host_adi_ms = (time.perf_counter() - t0) * 1e3 / n_host
        t0 = time.perf_counter()
        for b in range(a.host_poses):
            host_add(Re[b], te[b], Rg[b], tg[b], pts)
        host_add_ms = (time.perf_counter() - t0) * 1e3 / a.host_poses
        for B in (1, 32, 256):
            up = lambda x, s: torch.from_numpy(np.ascontiguousarray(x[:B].reshape(s))).to(dev)   # noqa: E731
            args = (up(Re, (B, 3, 3)), up(te, (B, 3, 1)), up(Rg, (B, 3, 3)), up(tg, (B, 3, 1)), ms)
            row = {"B": B, "V": V, "host_adi_ms_per_pose": host_adi_ms, "host_add_ms_per_pose": host_add_ms, "host_adi_poses_timed": n_host}
            for kinds, name in ((("adi",), "adi"), (("add",), "add"), (("add", "adi"), "both")):
                for _ in range(2):
                    metric.pose_errors(*args, kinds=kinds)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    metric.pose_errors(*args, kinds=kinds)
                e1.record()
                torch.cuda.synchronize()
                row["device_%s_ms" % name] = e0.elapsed_time(e1) / a.calls
            row["host_adi_ms"] = host_adi_ms * B
            row["adi_host_over_device"] = row["host_adi_ms"] / row["device_adi_ms"]
            row["add_host_over_device"] = host_add_ms * B / row["device_add_ms"]
            row["adi_pairs_per_s"] = B * float(V) * V / (row["device_adi_ms"] * 1e-3)
            rows.append(row)
            print("B=%3d V=%5d: ADI device %.3f ms, host %.1f ms (%s; x%.0f), %.3g pairs/s; ADD device %.3f ms" %
                  (B, V, row["device_adi_ms"], row["host_adi_ms"], "timed" if n_host >= B else "mean of %d poses x B" % n_host, row["adi_host_over_device"], row["adi_pairs_per_s"], row["device_add_ms"]), flush=True)
    res = {"bench": "pose_errors", "device": torch.cuda.get_device_name(0), "calls": a.calls, "warmup": 2, "host_poses": a.host_poses,
           "host_threads": os.environ.get("OMP_NUM_THREADS"), "host_path": "numpy + scipy.spatial.cKDTree, one pose at a time, float64",
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
