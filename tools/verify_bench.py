"""micro-benchmark of postprocess.verify_poses / select_poses (cp_verify_poses, cp_select_poses), tools/icp_bench.py's method.

  python tools/verify_bench.py [--out profiles/verify_bench.json] [--windows 3] [--warmup 1] [--poses 256]
  python tools/verify_bench.py --resources          (only where hipcc is: adds the compiler's figures of the new kernels to the file)

Time: device events around the WHOLE Python call (buffers allocated, the poses packed), after `--warmup` warm-up calls; the figure is the
median of `--windows` windows of one call each, the windows are kept.  tools/icp_bench.py's scene: P = 256 poses on 640 x 480 frames, 8
images, each the device's own render of one object (torus, ico1280, box, halfbox in turn) about 700 mm away with a far plane behind it;
every pose starts 4 degrees and 4 % of the distance along the ray off its image's truth.
  verify_poses                 the fused call, with and without the label map
  composition                  what it replaces at the parent commit: metric.render_depth (a (P,H,W) float frame), a gather of each pose's
                               sensor image, the torch elementwise passes of the rule and the sums; its counts are compared with the fused ones
  selection                    C = 2 candidates per crop, the start pose and refine_poses_icp's (N24 at its defaults, max_dist 0.3 diameters):
                               one verify_poses over 2 P poses + select_poses, against the same in torch with argmax; and the share of crops
                               on which the chosen candidate has the smaller ADD (equal ADDs count as right), per tau
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

KERNELS = ("pose_verify_pose_kernel", "pose_verify_vertex_kernel", "pose_verify_tile_kernel", "pose_verify_finish_kernel", "pose_select_kernel")


def kernel_resources():
    src = os.path.join(ROOT, "checkerpose_amd", "csrc", "pose_verify.hip")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "pose_verify", "timing": "UNMEASURED", "selection": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from pnp_gc_bench import device_call_ms
    from checkerpose_amd import _abi, metric
    from checkerpose_amd.postprocess import VERIFY_COUNTS, refine_poses_icp, select_poses, verify_poses
    from tests import icp_stages as I
    from tests.pnp_stages import K_LMO
    lib = _abi.load()
    dev = torch.device("cuda:0")
    W, H, n_img, P = 640, 480, 8, a.poses
    names = ("torus", "ico1280", "box", "halfbox")
    v, f = I.mesh_arrays(names)
    diam = I.diameters(names)
    ms = metric.MeshSet.from_arrays(v, diameters=diam, faces=f)
    rng = np.random.default_rng(24)
    Rt = np.stack([I._random_rotation(rng) for _ in range(n_img)])
    tt = np.stack([[rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(650, 750)] for _ in range(n_img)])
    img_mesh = np.arange(n_img) % len(names)
    K = torch.from_numpy(K_LMO).to(dev)
    depth = metric.render_depth(torch.from_numpy(Rt).to(dev), torch.from_numpy(tt).to(dev), K, ms, (W, H), mesh_ids=img_mesh)
    depth = torch.where(depth > 0, depth, torch.full_like(depth, 2000.0))
    image_ids = np.arange(P) % n_img
    mesh_ids = img_mesh[image_ids]
    R0 = np.stack([I._rodrigues(rng.normal(size=3), np.radians(4.0)) @ Rt[i] for i in image_ids])
    t0 = np.stack([tt[i] * (1.0 + 0.04 * (1.0 if rng.random() < 0.5 else -1.0)) for i in image_ids])
    R0d, t0d = torch.from_numpy(R0).to(dev), torch.from_numpy(t0).to(dev).reshape(P, 3, 1)
    img_t, mesh_t = torch.from_numpy(image_ids).to(dev), torch.from_numpy(mesh_ids.astype(np.int32)).to(dev)

    def composed(R, t, tau, weight=1.0, n=1):
        """the rule as the parent commit's pieces compose it: a full depth frame per pose, then torch passes.  n: the poses are n stacked
        candidate sets -> (counts (P', 6), score (P',))"""
        ids = img_t.repeat(n)
        D = metric.render_depth(R, t, K, ms, (W, H), mesh_ids=mesh_t.repeat(n))
        S = depth[ids]
        tau32 = torch.tensor(tau, dtype=torch.float32, device=dev)
        model = D > 0
        valid = torch.isfinite(S) & (S > 0)
        d = S - D
        ad = d.abs()
        live = model & valid
        match = live & (ad <= tau32)
        occluded = live & ~match & (d < -tau32)
        through = live & ~match & ~occluded
        q = torch.clamp((64.0 * (ad / tau32)).to(torch.int32), max=63) * match
        counts = torch.stack([x.sum((1, 2), dtype=torch.int32) for x in (model, model & ~valid, match, occluded, through, q)], 1)
        c = counts.double()
        den = (c[:, 2] + c[:, 4]) + weight * c[:, 3]
        return counts, torch.where(den != 0, (c[:, 2] - c[:, 5] / 64.0) / den, torch.full_like(den, float("nan")))

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        wins = [device_call_ms(fn) for _ in range(a.windows)]
        return float(np.median(wins)), wins

    tau = 20.0
    kw = dict(image_ids=img_t, mesh_ids=mesh_t)
    timing = {"P": P, "frame": [W, H], "images": n_img, "tau": tau}
    for label, fn in (("verify_poses", lambda: verify_poses(R0d, t0d, K, ms, depth, tau, **kw)),
                      ("verify_poses_with_labels", lambda: verify_poses(R0d, t0d, K, ms, depth, tau, return_labels=True, **kw)),
                      ("composition", lambda: composed(R0d, t0d, tau)),
                      ("render_depth_alone", lambda: metric.render_depth(R0d, t0d, K, ms, (W, H), mesh_ids=mesh_t))):
        timing[label + "_ms"], timing[label + "_windows_ms"] = timed(fn)
    score, info = verify_poses(R0d, t0d, K, ms, depth, tau, **kw)
    c_counts, c_score = composed(R0d, t0d, tau)
    fused_counts = torch.stack([info[k] for k in VERIFY_COUNTS], 1)
    timing["composition_counts_equal_fused"] = bool(torch.equal(fused_counts, c_counts))
    timing["composition_score_max_abs_diff"] = float(torch.nan_to_num(score - c_score).abs().max())
    timing["median_n_model"] = float(np.median(info["n_model"].cpu().numpy()))
    print("P = %d on %d x %d: verify_poses %.3f ms %s (with labels %.3f ms), composition %.3f ms %s (render_depth alone %.3f ms), counts equal: %s" % (
        P, W, H, timing["verify_poses_ms"], timing["verify_poses_windows_ms"], timing["verify_poses_with_labels_ms"], timing["composition_ms"],
        timing["composition_windows_ms"], timing["render_depth_alone_ms"], timing["composition_counts_equal_fused"]), flush=True)

    # ---- the selection: the start pose against N24's refinement of it
    max_dist = torch.from_numpy(0.3 * diam[mesh_ids]).to(dev)
    R1, t1, st, _ = refine_poses_icp(R0d, t0d, K, ms, depth, max_dist, image_ids=image_ids, mesh_ids=mesh_ids)
    Rc, tc = torch.stack([R0d, R1]), torch.stack([t0d, t1])

    def add_of(R, t):
        return metric.pose_errors(R, t, Rt[image_ids], tt[image_ids], ms, mesh_ids=mesh_ids, kinds=("add",))["add"].cpu().numpy()

    add = np.stack([add_of(R0d, t0d), add_of(R1, t1)])
    kw2 = dict(image_ids=img_t.repeat(2), mesh_ids=mesh_t.repeat(2))

    def fused_select(tau_):
        s, i = verify_poses(Rc.reshape(2 * P, 3, 3), tc.reshape(2 * P, 3, 1), K, ms, depth, tau_, **kw2)
        return select_poses(s.view(2, P), i["ok"].view(2, P), Rc, tc)

    def composed_select(tau_):
        _, s = composed(Rc.reshape(2 * P, 3, 3), tc.reshape(2 * P, 3, 1), tau_, n=2)
        choice = torch.argmax(torch.nan_to_num(s.view(2, P), nan=-1.0), 0)
        cols = torch.arange(P, device=dev)
        return choice, Rc[choice, cols], tc[choice, cols]

    selection = {"candidates": ["start", "icp"], "icp_status_counts": {str(k): int((st == k).sum()) for k in range(4)},
                 "share_icp_has_smaller_add": float((add[1] < add[0]).mean()), "median_add_percent_of_diameter": {
                     "start": float(np.median(100.0 * add[0] / diam[mesh_ids])), "icp": float(np.median(100.0 * add[1] / diam[mesh_ids]))}, "per_tau": []}
    selection["verify_and_select_ms"], selection["verify_and_select_windows_ms"] = timed(lambda: fused_select(tau))
    selection["composition_and_argmax_ms"], selection["composition_and_argmax_windows_ms"] = timed(lambda: composed_select(tau))
    for tau_ in (5.0, 10.0, 20.0, 40.0):
        choice = fused_select(tau_)[0].cpu().numpy()
        chosen = add[choice, np.arange(P)]
        row = {"tau": tau_, "share_chosen_has_smaller_or_equal_add": float((chosen <= add.min(0)).mean()), "share_icp_chosen": float((choice == 1).mean()),
               "choice_equals_composition": bool(np.array_equal(choice, composed_select(tau_)[0].cpu().numpy())),
               "median_add_percent_of_diameter_chosen": float(np.median(100.0 * chosen / diam[mesh_ids]))}
        selection["per_tau"].append(row)
        print("tau %g: %s" % (tau_, row), flush=True)
    print("selection at tau %g: verify + select %.3f ms, composition + argmax %.3f ms; icp better on %.3f of the crops" % (
        tau, selection["verify_and_select_ms"], selection["composition_and_argmax_ms"], selection["share_icp_has_smaller_add"]), flush=True)
    res = {"bench": "pose_verify", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()),
           "method": "device events around the whole call (allocations, packing of the poses), median of one-call windows after warm-ups; the "
                     "composition is metric.render_depth plus torch passes, what the fused call replaces",
           "timing": timing, "selection": selection, "kernel_resources": "UNMEASURED"}
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
