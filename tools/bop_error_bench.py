"""micro-benchmark of metric.bop_errors (cp_bop_errors: MSSD / MSPD / proj) against the host path a user has today: the float64 numpy
restatement of bop_toolkit_lib.pose_error.mssd / .mspd / .proj (tests/test_bop_error.py), one pose at a time, threads as the box sets them.

  python tools/bop_error_bench.py [--out profiles/bop_error_bench.json] [--calls 100] [--warmup 10] [--quick]

Device: events around `--calls` calls after `--warmup` warm-ups, for B in {1, 256} x V in {4096, 20480} x S in {1, 2, 8, 628, 1256}, each
kind alone and all three together (vertices: the first V rows of checkerpose_amd/data/fps_lm_15x4096.npy; symmetry sets: S rotations
about one axis).  The time is that of the whole Python call (allocation of the outputs and the scratch included), as a user pays it.
`evals_per_s` = B * S * V / time; `vector_fraction` = evals_per_s * (VALU instructions per evaluation, an ESTIMATE counted from the
source's arithmetic, not from the compiled ISA: 13 MSSD, 18 MSPD, 31 both) over the chip's fp32 vector issue rate (compute units x 128
lanes x clock; `clock_source` says whether the clock came from the device properties or is the 2.4 GHz assumed without them).  Host: ONE pose per (S, V), scaled to B.
Crossover: B = 256, V = 4096, all three kinds, both mappings forced, over S = 4 .. 128 -- `crossover_S` is the first S at which the
large-S mapping is not slower.  `--quick` runs a handful of calls of a few shapes (for a kernel trace).  No time is asserted: the parent
commit has no device path, so the host path is the comparison."""
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
from tests.test_bop_error import restate  # noqa: E402
from tests.test_pose_error import lm_table  # noqa: E402
from tools.pose_error_bench import poses  # noqa: E402

LM_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
INSTR = {"mssd": 13, "mspd": 18, "proj": 0, "all": 31}
KIND_SETS = (("mssd", ("mssd",)), ("mspd", ("mspd",)), ("proj", ("proj",)), ("all", ("mssd", "mspd", "proj")))


def sym_table(S):
    """S rotations about one axis (the first is the identity), as an (S,12) table"""
    a = np.array([0.0, 0.6, 0.8])
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    rows = []
    for i in range(S):
        th = 2.0 * np.pi * i / S
        rows.append(np.concatenate([(np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx).reshape(9), np.zeros(3)]))
    return np.stack(rows)


def sym_set(T):
    return metric.SymmetrySet.from_transforms([[{"R": r[:9].reshape(3, 3), "t": r[9:]} for r in T]])


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bop_error_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(0)
    clock_khz = getattr(prop, "clock_rate", None)
    clock_source = "torch.cuda.get_device_properties().clock_rate" if clock_khz else "assumed 2.4 GHz (the property is missing)"
    clock_hz = float(clock_khz or 2400000) * 1e3
    vector_rate = prop.multi_processor_count * 128 * clock_hz
    table = lm_table()
    rng = np.random.default_rng(0)
    Re, te, Rg, tg = poses(rng, 256)
    K = torch.from_numpy(LM_K).to(dev)

    def args_for(B, ms):
        up = lambda x, s: torch.from_numpy(np.ascontiguousarray(x[:B].reshape(s))).to(dev)   # noqa: E731
        return (up(Re, (B, 3, 3)), up(te, (B, 3, 1)), up(Rg, (B, 3, 3)), up(tg, (B, 3, 1)), K, ms)

    shapes = [(B, V, S) for V in (4096, 20480) for S in (1, 2, 8, 628, 1256) for B in (1, 256)]
    calls, warmup = a.calls, a.warmup
    if a.quick:
        shapes, calls, warmup = [(256, 4096, 8), (256, 4096, 628), (1, 20480, 1256)], 3, 1
    rows, host_ms = [], {}
    for B, V, S in shapes:
        pts = np.ascontiguousarray(table[:V])
        ms = metric.MeshSet.from_arrays([pts], diameters=[1.0])
        T = sym_table(S)
        ss = sym_set(T)
        if (V, S) not in host_ms and not a.quick:
            restate(Re[0], te[0], Rg[0], tg[0], LM_K, pts[:64], T[:1], np.float64)
            t0 = time.perf_counter()
            restate(Re[0], te[0], Rg[0], tg[0], LM_K, pts, T, np.float64)
            host_ms[(V, S)] = (time.perf_counter() - t0) * 1e3
        args = args_for(B, ms)
        row = {"B": B, "V": V, "S": S, "host_all_ms_per_pose": host_ms.get((V, S))}
        for name, kinds in KIND_SETS:
            t = timed(lambda: metric.bop_errors(*args, symmetries=ss, kinds=kinds), calls, warmup)
            row["device_%s_ms" % name] = t
            if name != "proj":
                row["%s_evals_per_s" % name] = B * float(S) * V / (t * 1e-3)
                row["%s_vector_fraction" % name] = row["%s_evals_per_s" % name] * INSTR[name] / vector_rate
        if row["host_all_ms_per_pose"] is not None:
            row["host_all_ms"] = row["host_all_ms_per_pose"] * B
            row["all_host_over_device"] = row["host_all_ms"] / row["device_all_ms"]
        rows.append(row)
        print("B=%3d V=%5d S=%4d: all %.3f ms (mssd %.3f, mspd %.3f, proj %.3f), %.3g evals/s = %.2f of the vector rate; host %s ms" %
              (B, V, S, row["device_all_ms"], row["device_mssd_ms"], row["device_mspd_ms"], row["device_proj_ms"], row["all_evals_per_s"],
               row["all_vector_fraction"], "%.1f" % row["host_all_ms"] if "host_all_ms" in row else "-"), flush=True)
    cross, crossover = [], None
    if not a.quick:
        pts = np.ascontiguousarray(table[:4096])
        ms = metric.MeshSet.from_arrays([pts], diameters=[1.0])
        args = args_for(256, ms)
        for S in (4, 8, 12, 16, 24, 32, 48, 64, 96, 128):
            ss = sym_set(sym_table(S))
            t_small = timed(lambda: metric.bop_errors(*args, symmetries=ss, _mapping="small"), calls, warmup)
            t_large = timed(lambda: metric.bop_errors(*args, symmetries=ss, _mapping="large"), calls, warmup)
            cross.append({"S": S, "small_ms": t_small, "large_ms": t_large})
            if crossover is None and t_large <= t_small:
                crossover = S
            print("crossover B=256 V=4096 S=%3d: small %.3f ms, large %.3f ms" % (S, t_small, t_large), flush=True)
    res = {"bench": "bop_errors", "device": torch.cuda.get_device_name(0), "calls": calls, "warmup": warmup,
           "host_threads": os.environ.get("OMP_NUM_THREADS"), "host_path": "numpy float64 restatement of pose_error.mssd + .mspd + .proj, one pose, scaled to B",
           "vector_rate_lane_instr_per_s": vector_rate, "compute_units": prop.multi_processor_count, "clock_hz": clock_hz, "clock_source": clock_source,
           "instr_per_eval_estimate": INSTR, "rows": rows, "crossover": cross, "crossover_S": crossover}
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
