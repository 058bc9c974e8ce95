"""micro-benchmark of postprocess.verify_scene_mask (cp_verify_scene_mask).

  python tools/scene_verify_bench.py [--out profiles/scene_verify_bench.json] [--rounds 5] [--reps 5] [--warmup 2]
  python tools/scene_verify_bench.py --resources     (only where hipcc is: adds the compiler's figures of the new kernels to the file)

Time: device events around `--reps` repeated calls of the WHOLE Python call (buffers allocated, the poses packed), per call; `--rounds`
rounds after `--warmup` warm-up calls of every variant, the variants in alternating order from round to round; per variant the median, the
rounds and spread = max - min.  The scene: P = 256 poses of LM-sized meshes (torus, ico1280, box, halfbox in turn) as 32 images x 8 poses
on 640 x 480 frames, about 700 mm away, the eight objects of an image clustered so that they hide each other; the masks are the truth
scenes' own (render_scene's planes, packed); every estimate starts 4 degrees and 4 % of the distance along the ray off its truth.
  verify_scene_mask            the fused call, without and with the two planes
  composition                  what it replaces at the parent commit: render.render_scene (colours, a depth frame and two planes per
                               image), render.scene_masks twice (two dense (P,H,W) byte arrays), coco_eval.pack_masks twice, the
                               word overlaps (and, popcount) and coco_eval.mask_ious of the predicted-visible silhouettes against the
                               visible masks; its n_model, n_pvis, n_pvis_in and iou_vis are compared with the fused ones (iou_vis
                               where the union is not empty: there the fused call gives NaN with ok = 0)
  verify_poses_mask            row N28 on the same poses and masks: the per-pose score this row extends
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

KERNELS = ("scene_verify_table_kernel", "scene_verify_pose_kernel", "scene_verify_vertex_kernel", "scene_verify_tile_kernel", "scene_verify_finish_kernel")


def kernel_resources():
    src = os.path.join(ROOT, "checkerpose_amd", "csrc", "scene_verify_mask.hip")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_verify_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "scene_verify_mask", "timing": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from checkerpose_amd import _abi, coco_eval, metric, render
    from checkerpose_amd.postprocess import verify_poses_mask, verify_scene_mask
    from tests import icp_stages as I
    from tests.pnp_stages import K_LMO
    lib = _abi.load()
    dev = torch.device("cuda:0")
    W, H, n_img, per, delta = 640, 480, 32, 8, 15.0
    P = n_img * per
    names = ("torus", "ico1280", "box", "halfbox")
    v, f = I.mesh_arrays(names)
    ms = metric.MeshSet.from_arrays(v, diameters=I.diameters(names), faces=f)
    rng = np.random.default_rng(31)
    image_ids = np.repeat(np.arange(n_img), per).astype(np.int32)
    mesh_ids = (np.arange(P) % len(names)).astype(np.int32)
    Rt = np.stack([I._random_rotation(rng) for _ in range(P)])
    centre = np.stack([[rng.uniform(-60, 60), rng.uniform(-40, 40), 0.0] for _ in range(n_img)])[image_ids]
    tt = centre + np.stack([[rng.uniform(-90, 90), rng.uniform(-70, 70), rng.uniform(620, 780)] for _ in range(P)])
    K = torch.from_numpy(K_LMO).to(dev)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    ids_t, mesh_t = up(image_ids), up(mesh_ids)

    def scene_packed(R, t):
        """the parent commit's pieces: the shaded scene render, the two dense mask stacks, the two packs"""
        sc = render.render_scene(R, t, K, ms, (W, H), image_ids, mesh_ids=mesh_ids, n_images=n_img, shading="flat", delta=delta)
        return (sc, coco_eval.pack_masks(render.scene_masks(sc["full_bits"], ids_t, sc["slot"])),
                coco_eval.pack_masks(render.scene_masks(sc["visib_bits"], ids_t, sc["slot"])))

    _, full, visible = scene_packed(up(Rt), up(tt).reshape(P, 3, 1))               # the truth scenes' masks
    R0 = np.stack([I._rodrigues(rng.normal(size=3), np.radians(4.0)) @ Rt[i] for i in range(P)])
    t0 = np.stack([tt[i] * (1.0 + 0.04 * (1.0 if rng.random() < 0.5 else -1.0)) for i in range(P)])
    R0d, t0d = up(R0), up(t0).reshape(P, 3, 1)
    pairs = torch.stack([torch.arange(P, device=dev, dtype=torch.int32)] * 2, 1)

    def popcount(x):
        """set bits per int32 word -> int64"""
        x = x.to(torch.int64) & 0xFFFFFFFF
        x = x - ((x >> 1) & 0x55555555)
        x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
        x = (x + (x >> 4)) & 0x0F0F0F0F
        return ((x * 0x01010101) & 0xFFFFFFFF) >> 24

    def composed():
        """-> (n_model, n_pvis, n_pvis_in, iou_vis) by the parent commit's calls: the word overlaps and mask_ious"""
        _, sil, pvis = scene_packed(R0d, t0d)
        return sil.area, pvis.area, popcount(pvis.bits & visible.bits).sum((1, 2)), coco_eval.mask_ious(pvis, visible, pairs)

    kw = dict(mesh_ids=mesh_t, n_images=n_img)
    variants = (("verify_scene_mask", lambda: verify_scene_mask(R0d, t0d, K, ms, full, visible, ids_t, delta, **kw)),
                ("verify_scene_mask_with_planes", lambda: verify_scene_mask(R0d, t0d, K, ms, full, visible, ids_t, delta, return_planes=True, **kw)),
                ("composition", composed),
                ("verify_poses_mask", lambda: verify_poses_mask(R0d, t0d, K, ms, full, visible=visible, mesh_ids=mesh_t)))

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
    timing = {"P": P, "images": n_img, "poses_per_image": per, "frame": [W, H], "delta": delta, "rounds": a.rounds, "reps_per_round": a.reps,
              "warmup_calls": a.warmup}
    for label, fn in variants:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        timing[label] = {"median_ms": float(np.median(rounds[label])), "rounds_ms": rounds[label], "spread_ms": float(max(rounds[label]) - min(rounds[label])),
                         "peak_allocation_bytes": int(torch.cuda.max_memory_allocated() - base)}
        print("%-32s %.3f ms per call  (spread %.3f)  peak %.1f MB  %s" % (label, timing[label]["median_ms"], timing[label]["spread_ms"],
                                                                          timing[label]["peak_allocation_bytes"] / 1e6, np.round(rounds[label], 3).tolist()), flush=True)
    score, info = verify_scene_mask(R0d, t0d, K, ms, full, visible, ids_t, delta, **kw)
    n_model, n_pvis, n_pvis_in, iou_vis = composed()
    s28, i28 = verify_poses_mask(R0d, t0d, K, ms, full, visible=visible, mesh_ids=mesh_t)
    timing["composition_n_model_equal_fused"] = bool(torch.equal(n_model, info["n_model"]))
    timing["composition_n_pvis_equal_fused"] = bool(torch.equal(n_pvis, info["n_pvis"]))
    timing["composition_n_pvis_in_equal_fused"] = bool(torch.equal(n_pvis_in, info["n_pvis_in"].to(torch.int64)))
    live = info["ok"]                                                              # where the union is 0 the fused call gives NaN with ok = 0
    timing["composition_iou_vis_bits_equal_fused_where_ok"] = bool(torch.equal(iou_vis[live].view(torch.int64), score[live].view(torch.int64)))
    timing["poses_with_empty_union"] = int((~live).sum())
    timing["composition_iou_vis_at_empty_union"] = [float(x) for x in iou_vis[~live].cpu().numpy()[:8]]
    timing["verify_poses_mask_iou_bits_equal_fused"] = bool(torch.equal(s28.view(torch.int64), info["iou"].view(torch.int64)))
    timing["median_silhouette_px"] = float(np.median(info["n_model"].cpu().numpy()))
    timing["median_visib_fract"] = float(np.nanmedian(info["visib_fract"].cpu().numpy()))
    timing["median_iou_vis"] = float(np.nanmedian(score.cpu().numpy()))
    timing["median_iou"] = float(np.nanmedian(info["iou"].cpu().numpy()))
    timing["poses_with_hidden_seen"] = int((info["n_hidden_seen"] > 0).sum())
    timing["dense_mask_bytes_not_allocated"] = 2 * P * H * W
    spread = max(timing["composition"]["spread_ms"], timing["verify_scene_mask"]["spread_ms"])
    timing["fused_faster_than_composition_by_more_than_the_spread"] = bool(timing["composition"]["median_ms"] - timing["verify_scene_mask"]["median_ms"] > spread)
    print("n_model equal: %s, n_pvis equal: %s, n_pvis_in equal: %s, iou_vis bits equal where ok: %s (%d poses with an empty union: %s), N28 iou bits "
          "equal: %s, fused faster by more than the spread: %s" % (
              timing["composition_n_model_equal_fused"], timing["composition_n_pvis_equal_fused"], timing["composition_n_pvis_in_equal_fused"],
              timing["composition_iou_vis_bits_equal_fused_where_ok"], timing["poses_with_empty_union"], timing["composition_iou_vis_at_empty_union"],
              timing["verify_poses_mask_iou_bits_equal_fused"], timing["fused_faster_than_composition_by_more_than_the_spread"]), flush=True)
    print("median silhouette %.0f px, median visib_fract %.3f, median iou %.3f, median iou_vis %.3f, poses with n_hidden_seen > 0: %d" % (
        timing["median_silhouette_px"], timing["median_visib_fract"], timing["median_iou"], timing["median_iou_vis"], timing["poses_with_hidden_seen"]), flush=True)
    res = {"bench": "scene_verify_mask", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()),
           "method": "device events around repeated whole calls (allocations, packing of the poses), per call; rounds in alternating order after "
                     "warm-ups, median and spread = max - min over the rounds; peak allocation = torch's peak above the resident inputs over one "
                     "call; the composition is render.render_scene, render.scene_masks twice, coco_eval.pack_masks twice and coco_eval.mask_ious",
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
