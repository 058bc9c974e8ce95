"""micro-benchmark of postprocess.verify_poses_photo (cp_verify_poses_photo_tex).

  python tools/photo_verify_bench.py [--out profiles/photo_verify_bench.json] [--rounds 5] [--reps 5] [--warmup 2] [--poses 256]
  python tools/photo_verify_bench.py --resources     (only where hipcc is: adds the compiler's figures of the new kernels to the file)

Time: device events around `--reps` repeated calls of the WHOLE Python call (buffers allocated, the poses packed), per call; `--rounds`
rounds after `--warmup` warm-up calls of every variant, the variants in alternating order from round to round; per variant the median, the
rounds and spread = max - min.  Memory: torch.cuda.max_memory_allocated over one call of each variant after reset_peak_memory_stats, less
what was allocated before the call.  The scene: P = 256 poses of YCB-V-sized meshes (a 100 mm sphere of 1280 faces under a 512 x 512
texture, the 100 mm can of tests/photo_stages.py, an 80 mm box with vertex colours, in turn) on 8 frames of 640 x 480 under YCB-V's
camera, 0.5 to 0.9 m away.
  verify_poses_photo        the fused call, without masks and with visible masks
  composition               what it replaces on the same build: render.render_rgb with depth (a (P,H,W,3) colour and a (P,H,W) depth frame),
                            then torch ops: the two lumas, the pixel set, the six integer sums, the finish in float64; its sums and its
                            ncc are compared with the fused ones
Also the worst distance in units in the last place between the device's ncc / gain / offset and the numpy rule over the cases of
tests/photo_stages.py (the tests' bound is 4).  NOTHING is required of the time; the file holds what was measured."""
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

KERNELS = ("photo_pose_kernel", "photo_vertex_kernel", "photo_tile_kernelILb0", "photo_tile_kernelILb1", "photo_finish_kernel")
K_YCBV = np.array([[1066.778, 0.0, 312.9869], [0.0, 1067.487, 241.3109], [0.0, 0.0, 1.0]])


def kernel_resources():
    src = os.path.join(ROOT, "checkerpose_amd", "csrc", "pose_verify_photo.hip")
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
        res[name.replace("ILb0", "<false>").replace("ILb1", "<true>")] = fig
    return res or "UNMEASURED"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photo_verify_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "pose_verify_photo", "timing": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from checkerpose_amd import _abi, coco_eval, metric, render
    from checkerpose_amd.postprocess import verify_poses_photo
    from tests import icp_stages as I
    from tests import photo_stages as PS
    from tests import render_rgb_stages as RS
    lib = _abi.load()
    dev = torch.device("cuda:0")
    W, H, n_img, P, min_pixels = 640, 480, 8, a.poses, 64
    rng = np.random.default_rng(35)
    sv, sf, scol, sn = RS.meshes()["ico1280"]
    d = sv.astype(np.float64) / np.linalg.norm(sv.astype(np.float64), axis=1, keepdims=True)
    suv = np.stack([np.arctan2(d[:, 1], d[:, 0]) / (2.0 * np.pi) + 0.5, np.arccos(np.clip(d[:, 2], -1.0, 1.0)) / np.pi], 1)
    can, box = PS.mesh_table()["can"], PS.mesh_table()["cbox"]
    ms = metric.MeshSet.from_arrays([sv, can["verts"], box["verts"]], faces=[sf, can["faces"], box["faces"]], normals=[sn, can["normals"], box["normals"]],
                                    colors=[None, None, box["colors"]], uvs=[suv, can["uvs"], None],
                                    textures=[rng.integers(0, 256, (512, 512, 3), dtype=np.uint8), can["tex"], None], diameters=[100.0, 120.0, 108.0])
    Rm = np.stack([I._random_rotation(rng) for _ in range(P)])
    tm = np.stack([[rng.uniform(-120, 120), rng.uniform(-90, 90), rng.uniform(500, 900)] for _ in range(P)])
    Rd, td = torch.from_numpy(Rm).to(dev), torch.from_numpy(tm).to(dev).reshape(P, 3, 1)
    K = torch.from_numpy(K_YCBV).to(dev)
    mesh_t = torch.from_numpy((np.arange(P) % 3).astype(np.int32)).to(dev)
    img_t = torch.from_numpy((np.arange(P) % n_img).astype(np.int32)).to(dev)
    frames = torch.from_numpy(rng.integers(0, 256, (n_img, H, W, 3), dtype=np.uint8)).to(dev)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.stack([((xx + 3 * k) // 40 + (yy + 5 * k) // 40) % 3 != 0 for k in range(n_img)])      # two thirds of every frame, in blocks
    visible = coco_eval.pack_masks(torch.from_numpy(masks.astype(np.uint8)).to(dev))
    dense = torch.from_numpy(masks).to(dev)
    wts = torch.tensor([77, 150, 29], dtype=torch.int32, device=dev)

    def composed(with_visible):
        """render_rgb's frames, then torch ops -> (n_model, n, sums (P,5), ncc)"""
        res = render.render_rgb(Rd, td, K, ms, (W, H), mesh_ids=mesh_t, shading="phong", return_depth=True)
        ya = ((res["rgb"].to(torch.int32) * wts).sum(-1, dtype=torch.int32) + 128) >> 8
        yb = (((frames.to(torch.int32) * wts).sum(-1, dtype=torch.int32) + 128) >> 8)[img_t.long()]
        model = res["depth"] > 0
        om = model & dense[img_t.long()] if with_visible else model
        ya, yb = ya * om, yb * om                                             # (int32 per pixel: 255^2 fits; the sums are int64)
        n = om.sum((1, 2))
        tot = lambda x: x.sum((1, 2), dtype=torch.int64)      # noqa: E731
        s = torch.stack([tot(ya), tot(yb), tot(ya * ya), tot(yb * yb), tot(ya * yb)], 1)
        cov, va, vb = n * s[:, 4] - s[:, 0] * s[:, 1], n * s[:, 2] - s[:, 0] * s[:, 0], n * s[:, 3] - s[:, 1] * s[:, 1]
        ncc = cov.double() / torch.sqrt(va.double() * vb.double())
        return model.sum((1, 2)), n, s, ncc

    kw = dict(image_ids=img_t, mesh_ids=mesh_t, shading="phong")
    variants = (("verify_poses_photo", lambda: verify_poses_photo(Rd, td, K, ms, frames, min_pixels, **kw)),
                ("verify_poses_photo_with_visible", lambda: verify_poses_photo(Rd, td, K, ms, frames, min_pixels, visible=visible, mask_ids=img_t, **kw)),
                ("composition", lambda: composed(False)),
                ("composition_with_visible", lambda: composed(True)),
                ("render_rgb_with_depth_alone", lambda: render.render_rgb(Rd, td, K, ms, (W, H), mesh_ids=mesh_t, shading="phong", return_depth=True)))

    def per_call_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    def peak_bytes(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        del out
        return int(peak)

    for _, fn in variants:
        for _ in range(a.warmup):
            fn()
    rounds = {label: [] for label, _ in variants}
    for r in range(a.rounds):
        for label, fn in (variants if r % 2 == 0 else variants[::-1]):           # alternating order
            rounds[label].append(per_call_ms(fn))
    timing = {"P": P, "frame": [W, H], "frames": n_img, "meshes": "ico1280 textured 512 x 512, can (24 segments, 16 x 8), box with vertex colours",
              "rounds": a.rounds, "reps_per_round": a.reps, "warmup_calls": a.warmup}
    for label, fn in variants:
        timing[label] = {"median_ms": float(np.median(rounds[label])), "rounds_ms": rounds[label], "spread_ms": float(max(rounds[label]) - min(rounds[label])),
                         "peak_allocated_bytes": peak_bytes(fn)}
        print("%-36s %.3f ms per call  (spread %.3f)  peak %.1f MiB  %s" % (label, timing[label]["median_ms"], timing[label]["spread_ms"],
                                                                           timing[label]["peak_allocated_bytes"] / 2 ** 20, np.round(rounds[label], 3).tolist()), flush=True)
    for vis, fused, comp in ((False, "verify_poses_photo", "composition"), (True, "verify_poses_photo_with_visible", "composition_with_visible")):
        score, info = variants[1 if vis else 0][1]()
        n_model, n, s, ncc = composed(vis)
        tag = "_with_visible" if vis else ""
        timing["composition_sums_equal_fused" + tag] = bool(torch.equal(n_model.int(), info["n_model"]) and torch.equal(n.int(), info["n"]) and all(
            torch.equal(s[:, i], info[k]) for i, k in enumerate(PS.SUMS)))
        okm = info["ok"].cpu().numpy()
        timing["composition_ncc_worst_ulp" + tag] = int(max(PS.ulp_distance(ncc.cpu().numpy()[okm], score.cpu().numpy()[okm])))
        timing["poses_ok" + tag] = int(okm.sum())
        timing["median_n" + tag] = float(np.median(info["n"].cpu().numpy()))
        timing["fused_peak_below_composition" + tag] = bool(timing[fused]["peak_allocated_bytes"] < timing[comp]["peak_allocated_bytes"])
        gap = timing[comp]["median_ms"] - timing[fused]["median_ms"]
        timing["fused_faster_than_composition_by_more_than_the_spread" + tag] = bool(gap > max(timing[comp]["spread_ms"], timing[fused]["spread_ms"]))
    timing["frames_not_allocated_bytes"] = P * H * W * (3 + 4)
    print({k: v for k, v in timing.items() if not isinstance(v, dict)}, flush=True)
    # the rule: the worst distance of the device's quotients from numpy's over the tests' cases
    import tests.test_gpu_verify_photo as G
    worst = {}
    for name in PS.CASES:
        _, _, out, want = G._run(name)
        worst[name] = int(G._check(out, want, what=name))
    print("worst ulp distance from the numpy rule per case: %s" % worst, flush=True)
    res = {"bench": "pose_verify_photo", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()),
           "method": "device events around repeated whole calls (allocations, packing of the poses), per call; rounds in alternating order after "
                     "warm-ups, median and spread = max - min over the rounds; peak = torch.cuda.max_memory_allocated over one call less what was "
                     "allocated before it; the composition is render.render_rgb with depth followed by torch ops on the same build",
           "timing": timing, "rule_worst_ulp": {"bound_in_tests": 4, "worst": max(worst.values()), "per_case": worst}, "kernel_resources": "UNMEASURED"}
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
