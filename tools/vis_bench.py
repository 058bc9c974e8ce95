"""micro-benchmark of vis.vis_poses (cp_vis_poses) beside the composition it replaces, tools/pnp_gc_bench.py's method.

  python tools/vis_bench.py [--out profiles/vis_bench.json] [--windows 3] [--warmup 1] [--images 64] [--poses-per-image 8]
  python tools/vis_bench.py --resources          (only where hipcc is: adds the compiler's figures of the new kernels to the file)

Time: device events around the WHOLE Python call (scratch and outputs allocated), after `--warmup` warm-up calls; the figure is the
median of `--windows` windows of one call each, the windows are kept.  The two sides run in the SAME process, alternating window by
window:  "scene" = one vis_poses call;  "composed" = render_rgb(return_depth=True) over all P poses (P full frames of 7 bytes per
pixel) followed by the composition in torch ops per image (the depth test, the masked copy, the boxes from the colour mask, the
outline, the blend).  Setup: frame 640 x 480, 64 images x 8 poses, mesh ico1280 scaled to 100 mm, phong, resolve_visib.
torch.cuda.max_memory_allocated of both sides is recorded.  No speed is required of this row and nothing is fixed in advance; the file
holds what was measured, and a figure that was not measured reads "not measured"."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("vis_pose_kernel", "vis_vertex_kernel", "vis_scene_tile_kernel", "vis_finish_kernel", "dd_init_kernel", "dd_reduce_kernel",
           "dd_second_kernel", "dd_stats_kernel", "dd_colour_kernel")


def kernel_resources():
    src = os.path.join(ROOT, "checkerpose_amd", "csrc", "vis_poses.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c", src, "-o", os.devnull,
                              "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900).stderr
    except (OSError, subprocess.SubprocessError):
        return "not measured"
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
            fig[key] = int(m.group(1)) if m else "not measured"
        res[name] = fig
    return res or "not measured"


def device_call_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def composed(render, R, t, K, ms, frames, image_ids, size, box_value):
    """the composition vis_poses replaces: every pose's full frame, then torch ops per image (resolve_visib, boxes drawn)"""
    import torch
    r = render.render_rgb(R, t, K, ms, size, shading="phong", bg_color=(0, 0, 0), return_depth=True)
    n_img, H, W = frames.shape[:3]
    ys = torch.arange(H, device=frames.device)[:, None]
    xs = torch.arange(W, device=frames.device)[None, :]
    vis = torch.empty_like(frames)
    for img in range(n_img):
        ren_rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=frames.device)
        ren_depth = torch.zeros((H, W), dtype=torch.float32, device=frames.device)
        layer = torch.zeros((H, W), dtype=torch.bool, device=frames.device)
        for b in image_ids[img]:
            m_rgb, m_depth = r["rgb"][b], r["depth"][b]
            m = (m_depth != 0) & ((ren_depth == 0) | (m_depth < ren_depth))
            ren_depth = torch.where(m, m_depth, ren_depth)
            ren_rgb = torch.where(m[..., None], m_rgb, ren_rgb)
            obj = (m_rgb > 0).any(2)
            cols, rows = obj.any(0), obj.any(1)
            x0, x1 = torch.where(cols, xs[0], W).min(), torch.where(cols, xs[0], -1).max()
            y0, y1 = torch.where(rows, ys[:, 0], H).min(), torch.where(rows, ys[:, 0], -1).max()
            layer |= (((xs == x0) | (xs == x1)) & (ys >= y0) & (ys <= y1)) | (((ys == y0) | (ys == y1)) & (xs >= x0) & (xs <= x1))
        v = (frames[img].to(torch.int32) + ren_rgb.to(torch.int32)) // 2 + layer[..., None].to(torch.int32) * box_value
        vis[img] = v.clamp(max=255).to(torch.uint8)
    return vis


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vis_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--poses-per-image", type=int, default=8)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "vis_poses", "timing": "not measured"}
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
    W, H, n_img, per = 640, 480, a.images, a.poses_per_image
    v, f, c, n = RS.meshes()["ico1280"]                                   # radius 50: 100 mm across
    ms = metric.MeshSet.from_arrays([v], faces=[f], colors=[c], normals=[n], diameters=[100.0])
    rng = np.random.default_rng(18)
    P = n_img * per
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    Rs = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(P)])
    Rs *= np.sign(np.linalg.det(Rs))[:, None, None]
    ts = np.stack([rng.uniform(-220, 220, P), rng.uniform(-150, 150, P), rng.uniform(600, 1000, P)], 1).reshape(P, 3, 1)
    ids = np.arange(P) % n_img                                            # interleaved
    R, t = torch.from_numpy(Rs).to(dev), torch.from_numpy(ts).to(dev)
    frames = torch.from_numpy(rng.integers(0, 256, size=(n_img, H, W, 3), dtype=np.uint8)).to(dev)
    per_image = [[int(b) for b in np.nonzero(ids == i)[0]] for i in range(n_img)]
    sides = {"scene": lambda: vis.vis_poses(R, t, K, ms, frames, image_ids=ids)["vis"],
             "composed": lambda: composed(render, R, t, K, ms, frames, per_image, (W, H), 76)}
    equal = bool(torch.equal(sides["scene"](), sides["composed"]()))
    for fn in sides.values():
        for _ in range(a.warmup):
            fn()
    wins, mem = {k: [] for k in sides}, {}
    for _ in range(a.windows):                                            # alternating
        for k, fn in sides.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            wins[k].append(device_call_ms(fn))
            mem[k] = int(torch.cuda.max_memory_allocated(dev) - base)
    row = {"frame": [W, H], "images": n_img, "poses": P, "mesh": "ico1280 (1280 faces, 100 mm)", "shading": "phong", "pictures_equal": equal}
    for k in sides:
        row[k + "_ms"], row[k + "_windows_ms"], row[k + "_peak_bytes_above_inputs"] = float(np.median(wins[k])), wins[k], mem[k]
    print("scene %.2f ms %s, composed %.2f ms %s, equal %s" % (row["scene_ms"], wins["scene"], row["composed_ms"], wins["composed"], equal), flush=True)
    res = {"bench": "vis_poses", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()),
           "method": "device events around the whole Python call, median of one-call windows after warm-ups, the two sides alternating in one "
                     "process; peak = torch.cuda.max_memory_allocated above what was allocated before the call", "timing": [row],
           "kernel_resources": "not measured"}
    if os.path.exists(a.out):
        old = json.load(open(a.out))
        if old.get("kernel_resources", "not measured") != "not measured":
            res["kernel_resources"] = old["kernel_resources"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
