"""micro-benchmark of render.render_scene and render.scene_training_batch (cp_render_scene, cp_crop_mask_bits)
beside the composition they replace, tools/vis_bench.py's method.

  python tools/scene_bench.py [--out profiles/scene_bench.json] [--windows 3] [--warmup 1] [--images 64] [--poses-per-image 8]
  python tools/scene_bench.py --resources        (only where hipcc is: adds the compiler's figures of the new kernels to the file)

Time: device events around the WHOLE Python call (scratch and outputs allocated), after `--warmup` warm-up calls; the figure is the
median of `--windows` windows of one call each, the windows are kept.  The sides of a pair run in the SAME process, alternating window
by window:
  "scene"          render_scene                     against  "composed": vis_poses(zeros frames, draw_boxes=False) +
                                                             gt_info(depth=ren_depth, return_masks=True)
  "scene_batch"    scene_training_batch(is_train=False)  against  "composed_batch": that composition + make_training_batch on the poses kept
Setup: frame 640 x 480, 64 images x 8 poses with interleaved image ids, mesh ico1280 scaled to 100 mm, phong.
torch.cuda.max_memory_allocated above the inputs is recorded for every side.  The mask memory is derived, not measured: two uint32
planes per image = 8 I H W bytes against 2 P H W bytes of mask images.  No speed is required of this row and nothing is fixed in
advance; the file holds what was measured, and a figure that was not measured reads "not measured"."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {"scene_labels.hip": ("scene_pose_kernel", "scene_vertex_kernel", "scene_tile_kernel", "scene_finish_kernel"),
           "preprocess.hip": ("crop_mask_bits_kernel",)}


def kernel_resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    res = {}
    for src, kernels in KERNELS.items():
        try:
            out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c", os.path.join(ROOT, "checkerpose_amd", "csrc", src),
                                  "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900).stderr
        except (OSError, subprocess.SubprocessError):
            return "not measured"
        for block in out.split("Function Name: ")[1:]:
            name = next((k for k in kernels if k in block.split()[0]), None)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--poses-per-image", type=int, default=8)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "render_scene", "timing": "not measured"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from checkerpose_amd import _abi, gt_info, metric, render, targets, vis
    from tests import render_rgb_stages as RS
    lib = _abi.load()
    dev = torch.device("cuda:0")
    W, H, n_img, per = 640, 480, a.images, a.poses_per_image
    v, f, c, n = RS.meshes()["ico1280"]                                   # radius 50: 100 mm across
    ms = metric.MeshSet.from_arrays([v], faces=[f], colors=[c], normals=[n], diameters=[100.0])
    rng = np.random.default_rng(19)
    P = n_img * per
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    Rs, ts, ids, _ = render.sample_scene_poses(rng, n_img, per, K, (W, H), (600.0, 1000.0), 1)      # interleaved image ids
    R, t = torch.from_numpy(Rs).to(dev), torch.from_numpy(ts).to(dev)
    zeros = torch.zeros((n_img, H, W, 3), dtype=torch.uint8, device=dev)
    p3 = rng.uniform(-45.0, 45.0, size=(512, 3))

    def composed():
        vp = vis.vis_poses(R, t, K, ms, zeros, image_ids=ids, resolve_visib=True, draw_boxes=False)
        return vp, gt_info.gt_info(R, t, K, ms, vp["ren_depth"], image_ids=ids, return_masks=True)

    def composed_batch():
        # make_training_batch addresses frames and masks through ONE img_index: the frames are expanded per sample, as a caller must
        vp, g = composed()
        kept = render.scene_kept(g["ok"].cpu().numpy(), g["visib_fract"].cpu().numpy(), 0.1)
        kd = torch.from_numpy(kept).to(dev)
        frames = vp["ren_rgb"][torch.from_numpy(ids[kept].astype(np.int64)).to(dev)]
        return targets.make_training_batch(frames, g["mask_visib"][kd], g["mask"][kd], R[kd], t[kd], K, list(g["bbox_visib"].cpu().numpy()[kept]), p3,
                                           is_train=False)

    pairs = {"scene": lambda: render.render_scene(R, t, K, ms, (W, H), ids, n_images=n_img), "composed": composed,
             "scene_batch": lambda: render.scene_training_batch(ms, None, R, t, K, (W, H), ids, p3, is_train=False, n_images=n_img),
             "composed_batch": composed_batch}
    s, (vp, g) = pairs["scene"](), composed()
    equal = bool(torch.equal(s["depth"], vp["ren_depth"]) and torch.equal(s["rgb"], vp["ren_rgb"]) and all(torch.equal(s[k], g[k]) for k in gt_info.KEYS)
                 and torch.equal(render.scene_masks(s["visib_bits"], ids, s["slot"]), g["mask_visib"])
                 and torch.equal(render.scene_masks(s["full_bits"], ids, s["slot"]), g["mask"]))
    (b1, kept), b2 = pairs["scene_batch"](), pairs["composed_batch"]()
    batch_equal = bool(len(b1) == len(b2) and all(torch.equal(x, y) for x, y in zip(b1, b2)))
    del s, vp, g, b1, b2
    for fn in pairs.values():
        for _ in range(a.warmup):
            fn()
    wins, mem = {k: [] for k in pairs}, {}
    for _ in range(a.windows):                                            # alternating
        for k, fn in pairs.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            wins[k].append(device_call_ms(fn))
            mem[k] = int(torch.cuda.max_memory_allocated(dev) - base)
    row = {"frame": [W, H], "images": n_img, "poses": P, "samples_kept": int(len(kept)), "mesh": "ico1280 (1280 faces, 100 mm)", "shading": "phong",
           "outputs_equal": equal, "batches_equal": batch_equal,
           "mask_bytes_derived": {"bit_planes_8_I_H_W": 8 * n_img * H * W, "mask_images_2_P_H_W": 2 * P * H * W}}
    for k in pairs:
        row[k + "_ms"], row[k + "_windows_ms"], row[k + "_peak_bytes_above_inputs"] = float(np.median(wins[k])), wins[k], mem[k]
    print("scene %.2f ms %s, composed %.2f ms %s, equal %s; scene_batch %.2f ms %s, composed_batch %.2f ms %s, equal %s"
          % (row["scene_ms"], wins["scene"], row["composed_ms"], wins["composed"], equal, row["scene_batch_ms"], wins["scene_batch"],
             row["composed_batch_ms"], wins["composed_batch"], batch_equal), flush=True)
    res = {"bench": "render_scene", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()),
           "method": "device events around the whole Python call, median of one-call windows after warm-ups, the sides alternating in one "
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
