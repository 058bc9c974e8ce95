"""micro-benchmark of postprocess.verify_poses_mask (cp_verify_poses_mask), tools/verify_bench.py's scene.

  python tools/verify_mask_bench.py [--out profiles/verify_mask_bench.json] [--rounds 5] [--reps 5] [--warmup 2] [--poses 256]
  python tools/verify_mask_bench.py --resources     (only where hipcc is: adds the compiler's figures of the new kernels to the file)

Time: device events around `--reps` repeated calls of the WHOLE Python call (buffers allocated, the poses packed), per call; `--rounds`
rounds after `--warmup` warm-up calls of every variant, the variants in alternating order from round to round; per variant the median, the
rounds and spread = max - min.  The scene: P = 256 poses of LM-sized meshes (torus, ico1280, box, halfbox in turn) on 640 x 480 frames,
about 700 mm away; 8 masks, each the device's own silhouette of one object's truth pose (the full mask) and the same with a slab of
columns cut out (the visible mask); every pose starts 4 degrees and 4 % of the distance along the ray off its mask's truth.
  verify_poses_mask            the fused call: full masks alone, with the visible masks, with the visible masks and the label map
  composition                  what it replaces at the parent commit: metric.render_depth (a (P,H,W) float frame), the threshold,
                               coco_eval.pack_masks, coco_eval.mask_ious against the full masks (and, "with visible", against the
                               visible ones too); its n_model and iou are compared with the fused ones
NOTHING is required of this row and nothing is fixed in advance; the file holds what was measured."""
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

KERNELS = ("pose_verify_mask_pose_kernel", "pose_verify_mask_vertex_kernel", "pose_verify_mask_tile_kernel", "pose_verify_mask_finish_kernel")


def kernel_resources():
    src = os.path.join(ROOT, "checkerpose_amd", "csrc", "pose_verify_mask.hip")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_mask_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "pose_verify_mask", "timing": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from checkerpose_amd import _abi, coco_eval, metric
    from checkerpose_amd.postprocess import verify_poses_mask
    from tests import icp_stages as I
    from tests.pnp_stages import K_LMO
    lib = _abi.load()
    dev = torch.device("cuda:0")
    W, H, n_masks, P = 640, 480, 8, a.poses
    names = ("torus", "ico1280", "box", "halfbox")
    v, f = I.mesh_arrays(names)
    ms = metric.MeshSet.from_arrays(v, diameters=I.diameters(names), faces=f)
    rng = np.random.default_rng(28)
    Rt = np.stack([I._random_rotation(rng) for _ in range(n_masks)])
    tt = np.stack([[rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(650, 750)] for _ in range(n_masks)])
    mask_mesh = np.arange(n_masks) % len(names)
    K = torch.from_numpy(K_LMO).to(dev)
    truth = metric.render_depth(torch.from_numpy(Rt).to(dev), torch.from_numpy(tt).to(dev), K, ms, (W, H), mesh_ids=mask_mesh) > 0
    seen = truth.clone()
    for n in range(n_masks):                                                     # a slab of 12 columns through each silhouette's middle
        xs = torch.nonzero(truth[n].any(0)).flatten()
        if len(xs):
            x0 = int(xs[len(xs) // 2])
            seen[n, :, x0:x0 + 12] = False
    full, visible = coco_eval.pack_masks(truth.to(torch.uint8)), coco_eval.pack_masks(seen.to(torch.uint8))
    mask_ids = np.arange(P) % n_masks
    mesh_ids = mask_mesh[mask_ids]
    R0 = np.stack([I._rodrigues(rng.normal(size=3), np.radians(4.0)) @ Rt[i] for i in mask_ids])
    t0 = np.stack([tt[i] * (1.0 + 0.04 * (1.0 if rng.random() < 0.5 else -1.0)) for i in mask_ids])
    R0d, t0d = torch.from_numpy(R0).to(dev), torch.from_numpy(t0).to(dev).reshape(P, 3, 1)
    mask_t, mesh_t = torch.from_numpy(mask_ids.astype(np.int32)).to(dev), torch.from_numpy(mesh_ids.astype(np.int32)).to(dev)
    pairs = torch.stack([torch.arange(P, device=dev, dtype=torch.int32), mask_t], 1)

    def composed(with_visible):
        """the parent commit's pieces: a full depth frame per pose, the threshold, the pack, the overlaps -> (n_model, iou[, iou with visible])"""
        D = metric.render_depth(R0d, t0d, K, ms, (W, H), mesh_ids=mesh_t)
        sil = coco_eval.pack_masks((D > 0).to(torch.uint8))
        out = (sil.area, coco_eval.mask_ious(sil, full, pairs))
        return out + (coco_eval.mask_ious(sil, visible, pairs),) if with_visible else out

    kw = dict(mask_ids=mask_t, mesh_ids=mesh_t)
    variants = (("verify_poses_mask", lambda: verify_poses_mask(R0d, t0d, K, ms, full, **kw)),
                ("verify_poses_mask_with_visible", lambda: verify_poses_mask(R0d, t0d, K, ms, full, visible=visible, **kw)),
                ("verify_poses_mask_with_visible_and_labels", lambda: verify_poses_mask(R0d, t0d, K, ms, full, visible=visible, return_labels=True, **kw)),
                ("composition", lambda: composed(False)),
                ("composition_with_visible", lambda: composed(True)),
                ("render_depth_alone", lambda: metric.render_depth(R0d, t0d, K, ms, (W, H), mesh_ids=mesh_t)))

    def per_call_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    for _, fn in variants:
        for _ in range(a.warmup):
            fn()
    rounds = {label: [] for label, _ in variants}
    for r in range(a.rounds):
        for label, fn in (variants if r % 2 == 0 else variants[::-1]):           # alternating order
            rounds[label].append(per_call_ms(fn))
    timing = {"P": P, "frame": [W, H], "masks": n_masks, "rounds": a.rounds, "reps_per_round": a.reps, "warmup_calls": a.warmup}
    for label, _ in variants:
        timing[label] = {"median_ms": float(np.median(rounds[label])), "rounds_ms": rounds[label], "spread_ms": float(max(rounds[label]) - min(rounds[label]))}
        print("%-44s %.3f ms per call  (spread %.3f)  %s" % (label, timing[label]["median_ms"], timing[label]["spread_ms"], np.round(rounds[label], 3).tolist()), flush=True)
    score, info = verify_poses_mask(R0d, t0d, K, ms, full, visible=visible, **kw)
    n_model, iou = composed(False)
    timing["composition_n_model_equal_fused"] = bool(torch.equal(n_model, info["n_model"]))
    timing["composition_iou_bits_equal_fused"] = bool(torch.equal(iou.view(torch.int64), score.view(torch.int64)))
    timing["median_n_model"] = float(np.median(info["n_model"].cpu().numpy()))
    timing["median_iou"] = float(np.nanmedian(score.cpu().numpy()))
    timing["depth_frame_bytes_not_allocated"] = P * H * W * 4
    gap = timing["composition"]["median_ms"] - timing["verify_poses_mask"]["median_ms"]
    timing["fused_faster_than_composition_by_more_than_the_spread"] = bool(gap > max(timing["composition"]["spread_ms"], timing["verify_poses_mask"]["spread_ms"]))
    print("n_model equal: %s, iou bits equal: %s, fused faster by more than the spread: %s" % (
        timing["composition_n_model_equal_fused"], timing["composition_iou_bits_equal_fused"], timing["fused_faster_than_composition_by_more_than_the_spread"]), flush=True)
    res = {"bench": "pose_verify_mask", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()),
           "method": "device events around repeated whole calls (allocations, packing of the poses), per call; rounds in alternating order after "
                     "warm-ups, median and spread = max - min over the rounds; the composition is metric.render_depth, the threshold, "
                     "coco_eval.pack_masks and coco_eval.mask_ious, what the fused call replaces",
           "timing": timing, "kernel_resources": "UNMEASURED"}
    if os.path.exists(a.out):
        old = json.load(open(a.out))
        if old.get("kernel_resources", "UNMEASURED") != "UNMEASURED":
            res["kernel_resources"] = old["kernel_resources"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
