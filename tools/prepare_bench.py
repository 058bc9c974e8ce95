"""micro-benchmark of checkerpose_amd.prepare (cp_fps, cp_pts_diameter), tools/vsd_bench.py's method.

  python tools/prepare_bench.py [--out profiles/prepare_bench.json] [--calls 10] [--warmup 2] [--quick]
  python tools/prepare_bench.py --host-reference [--out ...]      (only where the reference tree is: adds its own functions' times)

Device: events around `--calls` calls after `--warmup` warm-ups; the time is that of the whole Python call (clouds uploaded, outputs
and scratch allocated), as a user pays it.
  FPS: uniform clouds of V = 5 000 / 50 000 / 250 000 points, npoint = 4096, M = 1 and M = 21 clouds per call.
  `enqueue` rows: the 4097-launch chain enqueued directly (what the package does) against the same chain captured once into a
  linear graph and replayed (cp_graph_*): `graph_build_ms` is the host time of capture + instantiation, paid per (shape, buffers),
  `graph_replay_ms` a replay.  Object preparation runs once per object, so a graph would have to be built per call.
  Diameter: V = 4 096 / 20 480 / 100 000, M = 1.
Host figures of THIS box (numpy, OMP_NUM_THREADS as set): `host_rule_ms` = tests/prepare_cases.fps_rule, a numpy restatement of the rule
with the reference's passes per step, timed over `host_steps` samples of ONE cloud and scaled to npoint (a step's cost does not
depend on the step); `host_metric_ms` = metric.calc_pts_diameter (the package's pruned host function).  The reference's own functions
can only be timed where its tree is (--host-reference, a different box, stated in the file): farthest_point_sample_init_center over
`steps` samples scaled to 4096, misc.calc_pts_diameter in full.
No ratio is fixed in advance; the file holds what was measured."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from checkerpose_amd import _abi, metric, prepare  # noqa: E402
from tests import prepare_cases as P  # noqa: E402
from tools.bop_error_bench import timed  # noqa: E402

NPOINT = 4096


def cloud(V, seed=0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (V, 3)) * np.array([100.0, 60.0, 30.0])


def graph_times(clouds, calls, warmup):
    """the cp_fps chain of `clouds` captured into one graph: (host ms of capture + instantiation, ms per replay), ids checked"""
    lib = _abi.load()
    dev, pts, off_dev, off = prepare._upload(clouds, "cuda:0")
    M, sizes = off.shape[0] - 1, np.diff(off)
    scratch = torch.empty(lib.cp_fps_scratch_bytes(M, int(off[-1]), int(sizes.max()), 0), dtype=torch.uint8, device=dev)
    ids = torch.empty((M, NPOINT), dtype=torch.int32, device=dev)
    xyz = torch.empty((M, NPOINT, 3), dtype=torch.float64, device=dev)
    lane = torch.cuda.Stream(dev)
    lane.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _abi.check(lib.cp_graph_begin_capture(lane.cuda_stream), "graph capture begin")
    rc = lib.cp_fps(lane.cuda_stream, pts.data_ptr(), off_dev.data_ptr(), off.ctypes.data, M, NPOINT, 0, ids.data_ptr(), xyz.data_ptr(),
                    scratch.data_ptr())
    gx = C.c_void_p()
    rc2 = lib.cp_graph_end_capture(lane.cuda_stream, C.byref(gx))
    _abi.check(rc, "cp_fps under capture")
    _abi.check(rc2, "graph capture end")
    build = (time.perf_counter() - t0) * 1e3
    cur = torch.cuda.current_stream(dev).cuda_stream
    t = timed(lambda: _abi.check(lib.cp_graph_launch(gx, cur), "graph launch"), calls, warmup)
    direct, _ = prepare.fps_batch(clouds, NPOINT)
    same = bool(torch.equal(direct, ids))
    lib.cp_graph_destroy(gx)
    return build, t, same


def host_reference(out):
    ref = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
    sys.path.insert(0, os.path.join(ref, "bop_toolkit"))
    sys.path.insert(0, os.path.join(ref, "checkerpose", "preprocess_data"))
    import types
    for stub in ("plyfile", "mmcv"):
        sys.modules.setdefault(stub, types.ModuleType(stub))
    sys.modules["plyfile"].PlyData = None
    import get_fps_points as G
    from bop_toolkit_lib import misc
    rows = {"box": "the CPU box that holds the reference tree (not the GPU box)", "host_threads": os.environ.get("OMP_NUM_THREADS"), "fps": [], "diameter": []}
    for V in (5000, 50000, 250000):
        pts, steps = cloud(V), 256
        t0 = time.perf_counter()
        G.farthest_point_sample_init_center(pts, steps)
        ms = (time.perf_counter() - t0) * 1e3
        rows["fps"].append({"V": V, "steps_timed": steps, "ms_timed": ms, "ms_scaled_to_4096": ms * NPOINT / steps})
        print("reference FPS V=%6d: %.1f ms for %d samples -> %.0f ms for 4096" % (V, ms, steps, ms * NPOINT / steps), flush=True)
    for V in (4096, 20480, 100000):
        pts = cloud(V)
        t0 = time.perf_counter()
        misc.calc_pts_diameter(pts)
        ms = (time.perf_counter() - t0) * 1e3
        rows["diameter"].append({"V": V, "ms": ms})
        print("reference diameter V=%6d: %.1f ms" % (V, ms), flush=True)
    res = json.load(open(out)) if os.path.exists(out) else {"bench": "prepare"}
    res["reference_functions"] = rows
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepare_bench.json"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--host-reference", action="store_true")
    a = ap.parse_args()
    if a.host_reference:
        return host_reference(a.out)
    calls, warmup = a.calls, a.warmup
    fps_shapes = [(M, V) for V in (5000, 50000, 250000) for M in (1, 21)]
    diam_shapes, host_steps = [4096, 20480, 100000], 64
    if a.quick:
        fps_shapes, diam_shapes, calls, warmup, host_steps = [(1, 5000), (21, 50000)], [4096, 20480], 2, 1, 8
    fps_rows, enq_rows, diam_rows, host = [], [], [], {}
    for M, V in fps_shapes:
        clouds = [cloud(V, seed=m) for m in range(M)]
        if V not in host:
            t0 = time.perf_counter()
            P.fps_rule(clouds[0], host_steps)
            host[V] = (time.perf_counter() - t0) * 1e3 * NPOINT / host_steps
        t = timed(lambda: prepare.fps_batch(clouds, NPOINT), calls, warmup)
        dev, pts, off_dev, off = prepare._upload(clouds, "cuda:0")
        t_dev = timed(lambda: prepare._fps(dev, pts, off_dev, off, NPOINT), calls, warmup)       # without the upload
        fps_rows.append({"M": M, "V": V, "npoint": NPOINT, "device_ms": t, "device_ms_without_upload": t_dev, "ms_per_object": t / M,
                         "us_per_step": t_dev * 1e3 / (NPOINT + 2), "host_rule_ms_per_object": host[V], "host_steps": host_steps})
        print("fps  M=%2d V=%6d: %.2f ms per call (%.2f without the upload, %.2f us per launch), %.2f ms per object; host rule %.0f ms per object"
              % (M, V, t, t_dev, t_dev * 1e3 / (NPOINT + 2), t / M, host[V]), flush=True)
        if M == 1 or a.quick:
            build, replay, same = graph_times(clouds, calls, warmup)
            enq_rows.append({"M": M, "V": V, "direct_ms": t_dev, "graph_build_ms": build, "graph_replay_ms": replay, "ids_equal": same})
            print("     enqueue: direct %.2f ms, graph replay %.2f ms after %.1f ms of capture + instantiation, ids equal %s" % (t_dev, replay, build, same), flush=True)
    for V in diam_shapes:
        pts = cloud(V)
        t0 = time.perf_counter()
        ref = metric.calc_pts_diameter(pts)
        host_ms = (time.perf_counter() - t0) * 1e3
        t = timed(lambda: prepare.pts_diameters([pts]), calls, warmup)
        dev, tab, off_dev, off = prepare._upload([pts], "cuda:0")
        t_dev = timed(lambda: prepare._diameters(dev, tab, off_dev, off), calls, warmup)
        same = prepare.calc_pts_diameter(pts) == ref
        diam_rows.append({"V": V, "device_ms": t, "device_ms_without_upload": t_dev, "pairs_per_s": V * (V + 1) / 2 / (t_dev * 1e-3),
                          "host_metric_ms": host_ms, "equal_to_host": bool(same)})
        print("diam V=%6d: %.3f ms per call (%.3f without the upload, %.3g pairs/s); host metric.calc_pts_diameter %.1f ms; equal %s"
              % (V, t, t_dev, diam_rows[-1]["pairs_per_s"], host_ms, same), flush=True)
    res = {"bench": "prepare", "device": torch.cuda.get_device_name(0), "calls": calls, "warmup": warmup, "host_threads": os.environ.get("OMP_NUM_THREADS"),
           "host_paths": "host_rule_ms: tests/prepare_cases.fps_rule (numpy restatement, %d samples timed, scaled to 4096); host_metric_ms: "
                         "metric.calc_pts_diameter; both on the GPU box.  reference_functions (if present): the reference's own, on another box" % host_steps,
           "fps": fps_rows, "enqueue": enq_rows, "diameter": diam_rows}
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        if os.path.exists(a.out):
            old = json.load(open(a.out))
            if "reference_functions" in old:
                res["reference_functions"] = old["reference_functions"]
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
