"""micro-benchmark of checkerpose_amd.visibility (cp_hpr_visibility), tools/prepare_bench.py's method.

  python tools/visibility_bench.py [--out profiles/visibility_bench.json] [--views 2562] [--windows 3] [--warmup 1] [--budget 150]
  python tools/visibility_bench.py --host-reference [--host-views 8]     (only where the reference tree, scipy and hipcc are)

Device: device events around the WHOLE Python call (cloud and poses uploaded, outputs and scratch allocated, the status read back),
as a user pays it, after `--warmup` warm-up calls; the figure is the median of `--windows` windows of one call each.
Shapes: a seeded noisy blob (`cloud`) of V = 5 000 / 20 000 / 50 000 vertices, `--views` poses (2 562: render.sample_views' default
set), t = (0, 0, 400).  A shape is first probed with one view per automatic workgroup; if the full call, by that probe, would not fit
`--budget` seconds with its warm-ups and windows, the full figure is recorded as "UNMEASURED" and the probe's own figure stays, with
its number of views.  No speed is required of this row and no ratio is fixed in advance; the file holds what was measured.
--host-reference: the reference's OWN compute_vis_hpr loop (compiled from its source with `ast`, scipy's qhull), ONE thread, the same
clouds, `--host-views` views each, scaled to 2 562 -- on the box that holds the reference tree (not the GPU box), stated in the file;
and the compiler's resource figures of hpr_visibility_kernel (hipcc -Rpass-analysis=kernel-resource-usage)."""
import argparse
import ast
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (5000, 20000, 50000)
N_VIEWS = 2562
HOST_STARTING_RECORD_MS = {5000: 6.0, 20000: 21.0, 50000: 57.0}      # one view, scipy 1.15.3, one thread (the row's starting record)


def cloud(V, seed=0):
    """a noisy blob: a sphere of radius 60 squeezed to an ellipsoid, with 10 % radial noise"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(V, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return d * (60.0 * (1.0 + 0.1 * rng.normal(size=V)))[:, None] * np.array([1.0, 0.7, 0.5])


def rotations(n):
    from checkerpose_amd.render import sample_views
    views, _ = sample_views(N_VIEWS)
    R = np.stack([np.asarray(v["R"], dtype=np.float64).reshape(3, 3) for v in views])
    return R[np.arange(n) % R.shape[0]]


def kernel_resources():
    src = os.path.join(ROOT, "checkerpose_amd", "csrc", "visibility.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c", src, "-o", os.devnull,
                              "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600).stderr
    except (OSError, subprocess.SubprocessError):
        return "UNMEASURED"
    fig = {}
    for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                     ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgpr_spills", r"VGPRs Spill: (\d+)"),
                     ("lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
        m = re.search(pat, out)
        fig[key] = int(m.group(1)) if m else "UNMEASURED"
    return fig


def host_reference(out, host_views):
    from scipy.spatial import ConvexHull
    import scipy
    ref = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
    rel = os.path.join("checkerpose", "preprocess_data", "get_overall_visibility.py")
    tree = ast.parse(open(os.path.join(ref, rel)).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("compute_vis_hpr", "transform_pts_Rt")]
    ns = {"np": np, "ConvexHull": ConvexHull}
    exec(compile(ast.Module(body=fns, type_ignores=[]), rel, "exec"), ns)
    R, trans = rotations(host_views), np.array([0.0, 0.0, 400.0]).reshape((3, 1))
    rows = []
    for V in SHAPES:
        pts = cloud(V)
        per_view, visible = [], 0.0
        for k in range(host_views):
            t0 = time.perf_counter()
            vis = ns["compute_vis_hpr"](ns["transform_pts_Rt"](pts, R[k], trans), radius_param=2.0)
            per_view.append((time.perf_counter() - t0) * 1e3)
            visible += float(vis.mean())
        ms = float(np.median(per_view))
        rows.append({"V": V, "views_timed": host_views, "ms_per_view": ms, "s_scaled_to_2562_views": ms * N_VIEWS / 1e3,
                     "visible_share": visible / host_views, "starting_record_ms_per_view": HOST_STARTING_RECORD_MS[V]})
        print("reference loop V=%6d: %.1f ms per view (median of %d) -> %.0f s for 2562 views" % (V, ms, host_views, ms * N_VIEWS / 1e3), flush=True)
    res = json.load(open(out)) if os.path.exists(out) else {"bench": "visibility", "device_rows": "UNMEASURED"}
    res["reference_functions"] = {"box": "the CPU box that holds the reference tree (not the GPU box)", "threads": 1,
                                  "scipy": scipy.__version__, "rows": rows}
    res["kernel_resources"] = kernel_resources()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def device_call_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility_bench.json"))
    ap.add_argument("--views", type=int, default=N_VIEWS)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--budget", type=float, default=150.0, help="seconds a shape's full calls may take, by its probe")
    ap.add_argument("--shapes", type=int, nargs="*", default=list(SHAPES))
    ap.add_argument("--host-reference", action="store_true")
    ap.add_argument("--host-views", type=int, default=8)
    a = ap.parse_args()
    if a.host_reference:
        os.environ.setdefault("OMP_NUM_THREADS", "1")
        return host_reference(a.out, a.host_views)
    import torch
    from checkerpose_amd import _abi, visibility
    lib = _abi.load()
    R = rotations(a.views)
    rows = []
    for V in a.shapes:
        pts = cloud(V)
        slab = lib.cp_hpr_visibility_scratch_bytes(1, V, 0)
        groups = lib.cp_hpr_visibility_scratch_bytes(a.views, V, 0) // slab
        n_probe = int(min(groups, a.views))
        visibility.hpr_visibility(pts, R[:min(4, n_probe)])                               # first touch: library load, allocator
        probe_ms = device_call_ms(lambda: visibility.hpr_visibility(pts, R[:n_probe]))
        rounds = -(-a.views // n_probe)
        row = {"V": V, "n_views": a.views, "workgroups": int(groups), "slab_bytes": int(slab), "probe_views": n_probe, "probe_ms": probe_ms,
               "estimated_full_ms": probe_ms * rounds}
        if probe_ms * rounds * (a.warmup + a.windows) / 1e3 > a.budget:
            row.update({"device_ms": "UNMEASURED", "windows": 0, "why": "the probe puts warm-ups + windows beyond --budget %.0f s" % a.budget})
            print("V=%6d: probe of %d views %.1f ms -> about %.1f s per full call: full call UNMEASURED" % (V, n_probe, probe_ms, probe_ms * rounds / 1e3), flush=True)
        else:
            for _ in range(a.warmup):
                visibility.hpr_visibility(pts, R)
            wins = [device_call_ms(lambda: visibility.hpr_visibility(pts, R)) for _ in range(a.windows)]
            counts = visibility.hpr_visibility(pts, R)
            row.update({"device_ms": float(np.median(wins)), "windows_ms": wins, "windows": a.windows, "warmup": a.warmup,
                        "ms_per_view": float(np.median(wins)) / a.views, "mean_visibility": float(counts.double().mean()) / a.views})
            print("V=%6d: %d views in %.1f ms (median of %d windows), %.3f ms per view; probe of %d views %.1f ms"
                  % (V, a.views, row["device_ms"], a.windows, row["ms_per_view"], n_probe, probe_ms), flush=True)
        rows.append(row)
    res = {"bench": "visibility", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()),
           "method": "device events around the whole hpr_visibility call (uploads, allocations, status read-back), median of one-call windows "
                     "after warm-ups; probe = one call with one view per automatic workgroup",
           "host_starting_record_ms_per_view": {str(k): v for k, v in HOST_STARTING_RECORD_MS.items()}, "device_rows": rows,
           "reference_functions": "UNMEASURED", "kernel_resources": "UNMEASURED"}
    if os.path.exists(a.out):
        old = json.load(open(a.out))
        for key in ("reference_functions", "kernel_resources"):
            if old.get(key, "UNMEASURED") != "UNMEASURED":
                res[key] = old[key]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
