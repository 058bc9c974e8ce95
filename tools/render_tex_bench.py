"""micro-benchmark of row N20 (UV texture sampling; csrc/render_shade.h): what the feature costs the untextured calls, and what a
textured render costs beside a vertex-coloured one.  tools/scene_bench.py's method.

  python tools/render_tex_bench.py [--out profiles/render_tex_bench.json] [--windows 3] [--warmup 1] [--calls 1]
                                   [--parent-lib PATH/libcheckerpose_hip.so]
  python tools/render_tex_bench.py --resources        (only where hipcc is: adds the compiler's figures of the tile kernels' two instantiations to the file)

Time: device events around the WHOLE Python call (scratch and outputs allocated), after `--warmup` warm-up calls; the figure is the
median of `--windows` windows of `--calls` calls each (per call), the windows are kept.  The sides of a pair run in the SAME process,
alternating window by window.

  "untextured"   render_rgb (256 poses, phong, ssaa 1: tools/render_rgb_bench.py's shape), vis_poses and render_scene (64 images x 8 poses:
                 tools/vis_bench.py's and tools/scene_bench.py's), 640 x 480, ico1280, vertex colours -- through THIS tree's library
                 against the library built from the parent commit (--parent-lib; without it this part reads "not measured").  Both run
                 the same Python; the parent's library has no _tex entry points, so its side calls the plain ones with the same arguments.
                 The bar: this tree's median within the parent's own window spread.
  "textured"     render_rgb of 64 poses of ico1280 with spherical UVs and a 1024 x 1024 texture, "nearest" and "linear", ssaa 1 and 4,
                 beside the same mesh vertex-coloured; the ratio is recorded.  No speed is required of it."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {"render_rgb.hip": "rgb_tile_kernel", "vis_poses.hip": "vis_scene_tile_kernel", "scene_labels.hip": "scene_tile_kernel"}
K_LM = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
W, H = 640, 480


def kernel_resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    res = {}
    for src, kernel in KERNELS.items():
        try:
            out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c", os.path.join(ROOT, "checkerpose_amd", "csrc", src),
                                  "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900).stderr
        except (OSError, subprocess.SubprocessError):
            return "not measured"
        for block in out.split("Function Name: ")[1:]:
            sym = block.split()[0]
            m = re.search(r"\d%sILb([01])E" % kernel, sym)                # the mangled name holds <length><name>I<bool>E
            if m is None:
                continue
            name = "%s<%s>" % (kernel, "true" if m.group(1) == "1" else "false")
            fig = {}
            for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                             ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"), ("static_lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)"),
                             ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
                m = re.search(pat, block)
                fig[key] = int(m.group(1)) if m else "not measured"
            res[name] = fig
    return res or "not measured"


class ParentLib:
    """the parent commit's library behind this tree's Python: a _tex entry point it lacks is its plain one without the five texture
    arguments (which are null in every call made here)"""

    def __init__(self, path, signatures):
        self._lib = C.CDLL(path)
        for name, (res, args) in signatures.items():
            if hasattr(self._lib, name):
                fn = getattr(self._lib, name)
                fn.restype, fn.argtypes = res, args

    def __getattr__(self, name):
        if name.endswith("_tex"):
            fn = getattr(self._lib, name[:-4])
            return lambda *a: fn(*a[:-5])
        return getattr(self._lib, name)


def window_ms(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def alternate(sides, windows, warmup, calls):
    """sides: {name: (setup or None, fn)} -> {name: [per-call ms of each window]}, the sides alternating window by window"""
    for setup, fn in sides.values():
        if setup:
            setup()
        for _ in range(warmup):
            fn()
    wins = {k: [] for k in sides}
    for w in range(windows):
        for k, (setup, fn) in (list(sides.items()) if w % 2 == 0 else list(sides.items())[::-1]):      # the order flips: no side always runs first
            if setup:
                setup()
            wins[k].append(window_ms(fn, calls))
    return wins


def spherical_uvs(v):
    d = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    return np.stack([np.arctan2(d[:, 1], d[:, 0]) / (2.0 * np.pi) + 0.5, np.arccos(np.clip(d[:, 2], -1.0, 1.0)) / np.pi], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_tex_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "render_tex", "untextured": "not measured", "textured": "not measured"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from checkerpose_amd import _abi, metric, render, vis
    from tests import render_rgb_stages as RS
    lib = _abi.load()
    dev = torch.device("cuda:0")
    v, f, c, n = RS.meshes()["ico1280"]                                   # radius 50: 100 mm across
    ms = metric.MeshSet.from_arrays([v], faces=[f], colors=[c], normals=[n], diameters=[100.0])
    rng = np.random.default_rng(20)

    def poses(P, z):
        Rs = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(P)])
        Rs *= np.sign(np.linalg.det(Rs))[:, None, None]
        ts = np.stack([rng.uniform(-200, 200, P), rng.uniform(-150, 150, P), rng.uniform(*z, P)], 1).reshape(P, 3, 1)
        return torch.from_numpy(Rs).to(dev), torch.from_numpy(ts).to(dev)

    # ---- the untextured calls, this tree against the parent commit
    untextured = "not measured"
    if a.parent_lib:
        parent = ParentLib(a.parent_lib, _abi.SIGNATURES)
        use = lambda which: (lambda: setattr(_abi, "_lib", which))      # noqa: E731
        R1, t1 = poses(256, (350, 600))
        out1 = torch.empty((256, H, W, 3), dtype=torch.uint8, device=dev)
        n_img, per = 64, 8
        R2, t2 = poses(n_img * per, (600, 1000))
        ids = np.arange(n_img * per) % n_img
        frames = torch.from_numpy(rng.integers(0, 256, size=(n_img, H, W, 3), dtype=np.uint8)).to(dev)
        calls = {"render_rgb": lambda: render.render_rgb(R1, t1, K_LM, ms, (W, H), shading="phong", ssaa=1, out=out1),
                 "vis_poses": lambda: vis.vis_poses(R2, t2, K_LM, ms, frames, image_ids=ids),
                 "render_scene": lambda: render.render_scene(R2, t2, K_LM, ms, (W, H), ids, n_images=n_img)}
        untextured = {}
        for name, fn in calls.items():
            use(lib)()
            mine = fn()
            use(parent)()
            theirs = fn()
            equal = bool(all(torch.equal(mine[k], theirs[k]) for k in mine if mine[k].dtype != torch.float64))
            wins = alternate({"this": (use(lib), fn), "parent": (use(parent), fn)}, a.windows, a.warmup, a.calls)
            use(lib)()
            spread = max(wins["parent"]) - min(wins["parent"])
            med = {k: float(np.median(w)) for k, w in wins.items()}
            untextured[name] = {"this_ms": med["this"], "parent_ms": med["parent"], "this_windows_ms": wins["this"], "parent_windows_ms": wins["parent"],
                                "parent_window_spread_ms": spread, "within_parent_spread": bool(med["this"] <= med["parent"] + spread),
                                "outputs_equal": equal}
            print("untextured %-12s this %.3f ms %s, parent %.3f ms %s, equal %s" % (name, med["this"], wins["this"], med["parent"], wins["parent"], equal),
                  flush=True)
            del mine, theirs

    # ---- the textured path beside the vertex-coloured one
    tex = rng.integers(0, 256, size=(1024, 1024, 3), dtype=np.uint8)
    uv = spherical_uvs(v)
    sets = {filt: metric.MeshSet.from_arrays([v], faces=[f], normals=[n], diameters=[100.0], uvs=[uv], textures=[tex], tex_filter=filt)
            for filt in ("nearest", "linear")}
    R3, t3 = poses(64, (350, 600))
    out3 = torch.empty((64, H, W, 3), dtype=torch.uint8, device=dev)
    textured = []
    for ssaa in (1, 4):
        sides = {"vertex_colours": (None, lambda: render.render_rgb(R3, t3, K_LM, ms, (W, H), shading="phong", ssaa=ssaa, out=out3))}
        for filt, mset in sets.items():
            sides[filt] = (None, lambda mset=mset: render.render_rgb(R3, t3, K_LM, mset, (W, H), shading="phong", ssaa=ssaa, out=out3))
        wins = alternate(sides, a.windows, a.warmup, a.calls)
        med = {k: float(np.median(w)) for k, w in wins.items()}
        row = {"ssaa": ssaa, "poses": 64, "frame": [W, H], "mesh": "ico1280, spherical UVs", "texture": [1024, 1024]}
        for k in sides:
            row[k + "_ms"], row[k + "_windows_ms"] = med[k], wins[k]
        for filt in sets:
            row[filt + "_ratio_to_vertex_colours"] = med[filt] / med["vertex_colours"]
        textured.append(row)
        print("textured ssaa %d: vertex colours %.3f ms, nearest %.3f ms (x %.2f), linear %.3f ms (x %.2f)"
              % (ssaa, med["vertex_colours"], med["nearest"], row["nearest_ratio_to_vertex_colours"], med["linear"], row["linear_ratio_to_vertex_colours"]),
              flush=True)
    res = {"bench": "render_tex", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()), "windows": a.windows, "warmup": a.warmup,
           "calls_per_window": a.calls,
           "method": "device events around the whole Python call, median of the windows (per call) after warm-ups, the sides alternating in one process, their order flipping from window to window",
           "untextured": untextured, "textured": textured, "kernel_resources": "not measured"}
    if os.path.exists(a.out):
        old = json.load(open(a.out))
        if old.get("kernel_resources", "not measured") != "not measured":
            res["kernel_resources"] = old["kernel_resources"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
