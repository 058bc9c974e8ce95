"""micro-benchmark of postprocess.mask_extents / contour_samples / refine_poses_mask (csrc/mask_refine.hip),
tools/verify_mask_bench.py's scene.

  python tools/mask_refine_bench.py [--out profiles/mask_refine_bench.json] [--rounds 5] [--reps 5] [--warmup 2] [--poses 256]
  python tools/mask_refine_bench.py --resources     (only where hipcc is: adds the compiler's figures of the new kernels to the file)

Time: device events around `--reps` repeated calls of the WHOLE Python call (buffers allocated, the poses packed), per call; `--rounds`
rounds after `--warmup` warm-up calls of every variant, the variants in alternating order from round to round; per variant the median, the
rounds and spread = max - min.  The scene: P = 256 poses of LM-sized meshes (torus, ico1280, box, halfbox in turn) on 640 x 480 frames,
about 700 mm away; 8 masks, each the device's own silhouette of one object's truth pose; every pose starts 3 degrees, 1 % of the distance
sideways on each axis and 3 % along the ray off its mask's truth.
  mask_extents                 cp_mask_extents over the 8 packed masks, and over 256 (one per pose)
  mask_extents_torch           the torch composition it must beat to stay: coco_eval.unpack_masks, then where / amin / amax per axis
  contour_samples              stage A alone (grid 32)
  refine_poses_mask            the whole call (extents, stage A, the one-launch LM), dof "rt" and "t", max_dist 24 px, 20 iterations
  refine_poses_icp             row N24 on the same poses against the truths' depth renders: the yardstick with depth
  render_depth_alone           one raster pass that stores the frame: the yardstick of stage A
NOTHING is required of the refinement's time and nothing is fixed in advance; the file holds what was measured."""
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

KERNELS = ("mask_extents_kernel", "contour_pose_kernel", "contour_vertex_kernel", "contour_tile_kernel", "contour_finish_kernel", "mask_refine_kernel")


def kernel_resources():
    src = os.path.join(ROOT, "checkerpose_amd", "csrc", "mask_refine.hip")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_refine_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "mask_refine", "timing": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from checkerpose_amd import _abi, coco_eval, metric
    from checkerpose_amd import postprocess as Q
    from tests import icp_stages as I
    from tests.pnp_stages import K_LMO
    lib = _abi.load()
    dev = torch.device("cuda:0")
    W, H, n_masks, P = 640, 480, 8, a.poses
    names = ("torus", "ico1280", "box", "halfbox")
    v, f = I.mesh_arrays(names)
    diam = I.diameters(names)
    ms = metric.MeshSet.from_arrays(v, diameters=diam, faces=f)
    rng = np.random.default_rng(30)
    Rt = np.stack([I._random_rotation(rng) for _ in range(n_masks)])
    tt = np.stack([[rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(650, 750)] for _ in range(n_masks)])
    mask_mesh = np.arange(n_masks) % len(names)
    K = torch.from_numpy(K_LMO).to(dev)
    depth = metric.render_depth(torch.from_numpy(Rt).to(dev), torch.from_numpy(tt).to(dev), K, ms, (W, H), mesh_ids=mask_mesh)
    truth = depth > 0
    sensor = torch.where(truth, depth, torch.full_like(depth, 2000.0))           # row N24's image: the object before a far plane
    full = coco_eval.pack_masks(truth.to(torch.uint8))
    mask_ids = np.arange(P) % n_masks
    mesh_ids = mask_mesh[mask_ids]
    full_p = coco_eval.pack_masks(truth[torch.from_numpy(mask_ids).to(dev)].to(torch.uint8))      # one mask per pose
    sg = lambda: 1.0 if rng.random() < 0.5 else -1.0      # noqa: E731
    R0 = np.stack([I._rodrigues(rng.normal(size=3), np.radians(3.0)) @ Rt[i] for i in mask_ids])
    t0 = np.stack([tt[i] + tt[i][2] * np.array([0.01 * sg(), 0.01 * sg(), 0.03 * sg()]) for i in mask_ids])
    R0d, t0d = torch.from_numpy(R0).to(dev), torch.from_numpy(t0).to(dev).reshape(P, 3, 1)
    mask_t, mesh_t = torch.from_numpy(mask_ids.astype(np.int32)).to(dev), torch.from_numpy(mesh_ids.astype(np.int32)).to(dev)
    icp_dist = float(0.2 * diam.min())
    xs, ys = torch.arange(W, device=dev, dtype=torch.int32), torch.arange(H, device=dev, dtype=torch.int32)

    def extents_torch(packed):
        """the composition on unpack_masks' dense masks -> (row (N,H,2), col (N,W,2)) int32"""
        m = coco_eval.unpack_masks(packed).bool()
        r0, r1 = torch.where(m, xs[None, None, :], W).amin(2), torch.where(m, xs[None, None, :], -1).amax(2)
        c0, c1 = torch.where(m, ys[None, :, None], H).amin(1), torch.where(m, ys[None, :, None], -1).amax(1)
        return torch.stack([torch.where(r1 < 0, r1, r0), r1], 2).int(), torch.stack([torch.where(c1 < 0, c1, c0), c1], 2).int()

    kw = dict(mask_ids=mask_t, mesh_ids=mesh_t)
    variants = (("mask_extents_8", lambda: Q.mask_extents(full)),
                ("mask_extents_torch_8", lambda: extents_torch(full)),
                ("mask_extents_256", lambda: Q.mask_extents(full_p)),
                ("mask_extents_torch_256", lambda: extents_torch(full_p)),
                ("contour_samples", lambda: Q.contour_samples(R0d, t0d, K, ms, (W, H), mesh_ids=mesh_t, grid=32)),
                ("refine_poses_mask_rt", lambda: Q.refine_poses_mask(R0d, t0d, K, ms, full, 24.0, "rt", **kw)),
                ("refine_poses_mask_t", lambda: Q.refine_poses_mask(R0d, t0d, K, ms, full, 24.0, "t", **kw)),
                ("refine_poses_icp", lambda: Q.refine_poses_icp(R0d, t0d, K, ms, sensor, icp_dist, image_ids=mask_t, mesh_ids=mesh_t)),
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
    timing = {"P": P, "frame": [W, H], "masks": n_masks, "grid": 32, "max_dist_px": 24.0, "max_iters": 20, "rounds": a.rounds, "reps_per_round": a.reps,
              "warmup_calls": a.warmup}
    for label, _ in variants:
        timing[label] = {"median_ms": float(np.median(rounds[label])), "rounds_ms": rounds[label], "spread_ms": float(max(rounds[label]) - min(rounds[label]))}
        print("%-28s %.3f ms per call  (spread %.3f)  %s" % (label, timing[label]["median_ms"], timing[label]["spread_ms"], np.round(rounds[label], 3).tolist()), flush=True)
    for n, packed in (("8", full), ("256", full_p)):
        ext, (row, col) = Q.mask_extents(packed), extents_torch(packed)
        timing["mask_extents_equal_torch_%s" % n] = bool(torch.equal(ext["row"], row) and torch.equal(ext["col"], col))
        k, c = timing["mask_extents_%s" % n], timing["mask_extents_torch_%s" % n]
        timing["mask_extents_faster_than_torch_by_more_than_the_spread_%s" % n] = bool(c["median_ms"] - k["median_ms"] > max(k["spread_ms"], c["spread_ms"]))
    truth_t = torch.from_numpy(tt[mask_ids]).to(dev)
    err = lambda t: float((t.reshape(P, 3) - truth_t).norm(dim=1).median())      # noqa: E731
    timing["median_translation_error_mm"] = {"input": err(t0d)}
    for label, dof in (("refine_poses_mask_rt", "rt"), ("refine_poses_mask_t", "t")):
        R1, t1, st, info = Q.refine_poses_mask(R0d, t0d, K, ms, full, 24.0, dof, **kw)
        timing["median_translation_error_mm"][label] = err(t1)
        timing[label]["status_counts"] = np.bincount(st.cpu().numpy(), minlength=4).tolist()
        timing[label]["median_iters"] = float(info["iters"].double().median())
        timing[label]["median_pairs"] = float(info["n"].double().median())
    R1, t1, st, info = Q.refine_poses_icp(R0d, t0d, K, ms, sensor, icp_dist, image_ids=mask_t, mesh_ids=mesh_t)
    timing["median_translation_error_mm"]["refine_poses_icp"] = err(t1)
    print(json.dumps({k: timing[k] for k in timing if k.startswith("mask_extents_equal") or k.startswith("mask_extents_faster") or k == "median_translation_error_mm"}), flush=True)
    res = {"bench": "mask_refine", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()),
           "method": "device events around repeated whole calls (allocations, packing of the poses), per call; rounds in alternating order after "
                     "warm-ups, median and spread = max - min over the rounds; mask_extents_torch is coco_eval.unpack_masks, then where / amin / "
                     "amax per axis, what cp_mask_extents must beat to stay",
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
