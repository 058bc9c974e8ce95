#!/usr/bin/env python3
"""Row N6 (ground-truth side: keypoint codes, box jitter, the code / mask report, re / te) pinned by the REFERENCE's own statements.

Runs ONLY where the reference tree is (CHECKERPOSE_REFERENCE, default /root/reference; nothing of it travels, only the recorded
arrays in targets.npz are committed):

  python tests/golden/make_golden_targets.py

`bop_dataset_pytorch.py`, `test.py` and `test_network_with_test_data.py` import modules this image lacks, so the pieces used are
compiled from their source with `ast` while generating: the functions `project_pts`, `aug_Bbox`, `get_final_Bbox`,
`mapping_pixel_position_to_original_position_2d`, `class_id_vec_to_class_code_vecs`, `compute_mask_pixelwise_error`,
`compute_mask_iou`, the statements of `__getitem__` that discretise the projections (from `roi_mask_bit = ...` to `pixel_y_code = ...`,
:356-373, run with a stub `self`), and the statements of test.py's inner loop from `npoint_in_roi = ...` to `full_iou_arr[...] = ...`
(:432-457).  `bop_toolkit_lib.pose_error.re` / `.te` import directly.

Keypoints are NOT stored: rows of checkerpose_amd/data/fps_lm_15x4096.npy (float32, cast to float64) -- `enc_obj` names the object
(1-based), the first `enc_N` rows are the keypoints.
  groups   0: N = 512 shared (object 1), S = 64, crop_square_resize, tall and wide boxes, boxes off the frame, a box that misses the
              object (no keypoint in the RoI) and one "no detection" crop (the loader's dummy: zeros, :328-338)
           1: N = 512 shared, S = 128, crop_resize with w != h (clamped to the 640 x 480 frame)
           2: the LM twin: N = 4096, objects 1-3 mixed (`obj_ids`), S = 64
  asserted while generating (the crop is redrawn otherwise): depth > 0; every quotient (u - bx) / (bw / S) lies >= 1e-6 from an
  integer and every u - bx, v - by >= 1e-6 px from zero, so no label hinges on rounding; over the fixture every out-of-RoI cause
  occurs (left, above, right, below) and 10 % - 90 % of the keypoints are inside.
  report   groups 0 and 1 as batches: logits made from the labels (sign = bit, |logit| a power of two in [2^-9, 4], stored as
           float16 and read as float32) with a seeded 10 % of the bits flipped, the leading nb bits of them (nb = 6 and 5 for group 0, 6 for group 1); seg logits from GT disc masks shifted by a
           few pixels, at the seg sizes 64 and 32; the "no detection" crop has empty masks and all-negative seg logits (empty union).
           Recorded: the reference's figures and the integer counts they are quotients of, taken from the reference's own arrays.
  aug      32 boxes, each under its own np.random.seed, through the reference's aug_Bbox.
  re / te  of the poses of pose_error.npz (same order)."""
import ast
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "bop_toolkit"))
sys.path.insert(0, ROOT)

from bop_toolkit_lib import pose_error  # noqa: E402

K_LM = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
IMG_W, IMG_H = 640, 480
MARGIN = 1e-6


def _tree(rel):
    return ast.parse(open(os.path.join(REF, "checkerpose", rel)).read())


def _functions(rel, names, ns):
    fns = [n for n in _tree(rel).body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(f.name for f in fns) == sorted(names), (rel, names)
    exec(compile(ast.Module(body=fns, type_ignores=[]), rel, "exec"), ns)


def _assigns(stmt):
    out = []
    for t in getattr(stmt, "targets", []):
        for n in ast.walk(t):
            if isinstance(n, ast.Name):
                out.append(n.id)
    return out


def _span(body, first_name, last_name, rel):
    """the statements of `body` from the first that assigns `first_name` to the next one that assigns (an element of) `last_name`"""
    i0 = next(i for i, s in enumerate(body) if first_name in _assigns(s))
    i1 = next(i for i, s in enumerate(body) if i > i0 and last_name in _assigns(s))
    assert i0 < i1
    return compile(ast.Module(body=body[i0:i1 + 1], type_ignores=[]), rel, "exec")


def reference_pieces():
    ns = {"np": np, "math": math, "torch": torch}
    _functions("bop_dataset_pytorch.py", ["project_pts", "aug_Bbox", "get_final_Bbox", "mapping_pixel_position_to_original_position_2d"], ns)
    _functions("binary_code_helper/class_id_encoder_decoder.py", ["class_id_vec_to_class_code_vecs"], ns)
    _functions("test_network_with_test_data.py", ["compute_mask_pixelwise_error", "compute_mask_iou"], ns)
    cls = [n for n in _tree("bop_dataset_pytorch.py").body if isinstance(n, ast.ClassDef) and n.name == "bop_dataset_single_obj_pytorch_code2d"][0]
    getitem = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__getitem__"][0]
    discretise = _span(getitem.body, "roi_mask_bit", "pixel_y_code", "bop_dataset_pytorch.py")
    loops = [n for n in ast.walk(_tree("test.py")) if isinstance(n, ast.For) and any("npoint_in_roi" in _assigns(s) for s in n.body)]
    assert len(loops) == 1
    report = _span(loops[0].body, "npoint_in_roi", "full_iou_arr", "test.py")
    return ns, discretise, report


def rodrigues(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def encode_one(ns, discretise, pts, K, R, t, Bbox, method, S):
    """the loader's path for one sample: project_pts, get_final_Bbox, then the statements :356-373 -> dict, or None on a margin violation"""
    proj_xy, depth = ns["project_pts"](pts, K, R, t.reshape(3, 1))
    final = ns["get_final_Bbox"](np.array(Bbox), method, IMG_W, IMG_H)
    if final[2] <= 0 or final[3] <= 0:
        return None
    roi_x = np.linspace(0, S - 1, S)
    self = types.SimpleNamespace(num_p3d=pts.shape[0], crop_size_gt=S, roi_xy=np.asarray(np.meshgrid(roi_x, roi_x)).transpose((1, 2, 0)))
    env = dict(ns, self=self, proj_xy=proj_xy, Bbox=final, num_code_dir_bit=int(math.log2(S)))
    exec(discretise, env)
    if not (depth > 0).all():
        return None
    for k in (0, 1):
        d = proj_xy[:, k] - final[k]
        q = d / (final[2 + k] / S)
        if (np.abs(d) < MARGIN).any() or (np.abs(q - np.round(q)) < MARGIN).any():
            return None
    return {"final": final, "proj_xy": proj_xy, "depth": depth, "roi": env["roi_mask_bit"][:, 0], "x_code": env["pixel_x_code"],
            "y_code": env["pixel_y_code"], "x_id": env["pixel_x_id"], "y_id": env["pixel_y_id"], "roi_xy_ori": env["roi_xy_ori"],
            "left": (proj_xy[:, 0] < final[0]).any(), "above": (proj_xy[:, 1] < final[1]).any(),
            "right": ((proj_xy[:, 0] - final[0]) / (final[2] / S) >= S).any(), "below": ((proj_xy[:, 1] - final[1]) / (final[3] / S) >= S).any()}


def draw_crop(rng, ns, discretise, pts, method, S, shape, place):
    """shape: "tall" | "wide" | "any"; place: "centre" | "edge" (object near the frame's corner: the final box leaves the frame) |
    "miss" (the box lies beside the object)"""
    for _ in range(200):
        R = rodrigues(rng.normal(size=3), rng.uniform(0, 180))
        z = rng.uniform(600, 1200)
        if place == "edge":
            t = np.array([-325.0 * z / 572.4 + rng.uniform(0, 40), -242.0 * z / 573.6 + rng.uniform(0, 40), z])
        else:
            t = np.array([rng.uniform(-120, 120), rng.uniform(-80, 80), z])
        uv, _ = ns["project_pts"](pts, K_LM, R, t.reshape(3, 1))
        lo, hi = uv.min(0), uv.max(0)
        ext = hi - lo
        w, h = ext * rng.uniform(0.5, 1.5, size=2)
        if shape == "tall":
            h = max(h, 1.4 * w)
        elif shape == "wide":
            w = max(w, 1.4 * h)
        c = 0.5 * (lo + hi) + ext * rng.uniform(-0.3, 0.3, size=2)
        if place == "miss":
            c = c + np.array([2.5 * ext[0] + w, 0.0])
        Bbox = [int(c[0] - w / 2), int(c[1] - h / 2), int(w), int(h)]
        if Bbox[2] < 8 or Bbox[3] < 8 or Bbox[2] == Bbox[3]:
            continue
        e = encode_one(ns, discretise, pts, K_LM, R, t, Bbox, method, S)
        if e is None:
            continue
        if place == "edge" and not ((Bbox[0] < 0 and Bbox[1] < 0) if method == "crop_resize" else (e["final"][0] < 0 and e["final"][1] < 0)):
            continue
        if place == "miss" and e["roi"].sum() != 0:
            continue
        e.update(R=R, t=t, Bbox=np.array(Bbox))
        return e
    raise AssertionError("no crop clear of the margins for %r" % ((method, S, shape, place),))


def disc_masks(rng, S, empty):
    """(visible, full) GT mask crops, float 0 / 1 as transform_pre leaves them (mask / 255); visible = full minus an occluding half plane"""
    yy, xx = np.mgrid[0:S, 0:S]
    if empty:
        return np.zeros((S, S), np.float32), np.zeros((S, S), np.float32)
    cx, cy, r = rng.uniform(0.35, 0.65) * S, rng.uniform(0.35, 0.65) * S, rng.uniform(0.2, 0.4) * S
    full = ((xx - cx) ** 2 + (yy - cy) ** 2 <= r * r)
    vis = full & (xx + 0.5 * yy < cx + 0.9 * r)
    return vis.astype(np.float32), full.astype(np.float32)


def seg_logits(rng, vis, full, size, empty):
    """seg logits at (size, size) from the GT masks shifted by a few pixels; |logit| >= 1e-3"""
    out = []
    for m in (vis, full):
        sh = np.roll(m, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), (0, 1))
        sm = F.interpolate(torch.from_numpy(sh)[None, None], size=(size, size), mode="nearest")[0, 0].numpy()
        mag = 2.0 ** rng.integers(-9, 3, size=sm.shape)
        out.append(np.where(empty, -mag, np.where(sm > 0.5, mag, -mag)))
    return np.stack(out).astype(np.float16)


def report_batch(ns, report, rng, crops, S, nb, seg_size):
    """test.py:294-323 for one batch (the sigmoid decisions, the transposes to (batch, #keypoint, #bits), the GT masks brought to the
    seg size), then the reference's statements :432-457 per crop"""
    B, N, bits = len(crops), crops[0]["roi"].shape[0], int(math.log2(S))
    gt_roi = np.stack([c["roi"][None] for c in crops]).astype(np.float32)                      # (B,1,N) as the loader returns it
    gt_x = np.stack([c["x_code"].T for c in crops]).astype(np.float32)                         # (B,bits,N)
    gt_y = np.stack([c["y_code"].T for c in crops]).astype(np.float32)
    logits = []
    for g in (gt_roi, gt_x[:, :nb], gt_y[:, :nb]):
        flip = rng.random(g.shape) < 0.1
        logits.append((np.where((g > 0.5) ^ flip, 1.0, -1.0) * 2.0 ** rng.integers(-9, 3, size=g.shape)).astype(np.float16))
    masks = [disc_masks(rng, S, c["no_det"]) for c in crops]
    m_vis, m_full = np.stack([m[0] for m in masks]), np.stack([m[1] for m in masks])
    seg = np.stack([seg_logits(rng, m[0], m[1], seg_size, c["no_det"]) for m, c in zip(masks, crops)])
    assert all(a.dtype == np.float16 and np.abs(a.astype(np.float32)).min() >= 1e-3 for a in logits + [seg])
    f16 = {"logit_roi": logits[0], "logit_x": logits[1], "logit_y": logits[2], "seg": seg}
    logits, seg = [a.astype(np.float32) for a in logits], seg.astype(np.float32)       # the reference sees float32, as from the network
    dec = lambda z: torch.where(torch.sigmoid(torch.from_numpy(z)) > 0.5, 1.0, 0.0).numpy()     # noqa: E731
    tr = lambda a: a.transpose(0, 2, 1)                                                       # noqa: E731
    pred_seg = dec(seg)
    near = lambda m: F.interpolate(torch.from_numpy(m)[:, None], size=(seg_size, seg_size), mode="nearest").squeeze(1).numpy()   # noqa: E731
    env = dict(ns, num_p3d=N, num_proj_bits=nb, batch_idx=0,
               gt_roi_bit=tr(gt_roi), pred_roi_bit=tr(dec(logits[0])), gt_x_bits=tr(gt_x[:, :nb]), pred_x_bits=tr(dec(logits[1])),
               gt_y_bits=tr(gt_y[:, :nb]), pred_y_bits=tr(dec(logits[2])), pred_seg_visib=pred_seg[:, 0], pred_seg_full=pred_seg[:, 1],
               gt_seg_visib=near(m_vis), gt_seg_full=near(m_full))
    names = ("roi_bit_acc", "reproj_x_acc", "reproj_y_acc", "visib_pixel_acc", "visib_iou", "full_pixel_acc", "full_iou")
    fig = {k: np.zeros(B) for k in names}
    fig["bit_err_arr"] = np.zeros((B, 2 * nb + 1))
    cnt = {k: np.zeros(B, np.int64) for k in ("n_in_roi", "roi_bit_mismatch", "x_id_abs_diff", "y_id_abs_diff", "visib_mismatch",
                                                "visib_intersection", "visib_union", "full_mismatch", "full_intersection", "full_union")}
    cnt["x_bit_mismatch"], cnt["y_bit_mismatch"] = np.zeros((B, nb), np.int64), np.zeros((B, nb), np.int64)
    w = 2.0 ** np.arange(nb - 1, -1, -1)
    for b in range(B):
        env.update({k + "_arr": np.zeros(1) for k in names})
        env.update(counter=b, bit_err_arr=np.zeros((1, 2 * nb + 1)))
        exec(report, env)
        for k in names:
            fig[k][b] = env[k + "_arr"][0]
        fig["bit_err_arr"][b] = env["bit_err_arr"][0]
        # the integer counts behind those figures, from the reference's own arrays
        exact = lambda v: int(round(float(v)))                                              # noqa: E731
        cnt["n_in_roi"][b] = exact(env["gt_roi_bit"][b].sum())
        cnt["roi_bit_mismatch"][b] = exact(np.abs(env["gt_roi_bit"][b] - env["pred_roi_bit"][b]).sum())
        cnt["x_bit_mismatch"][b] = np.abs(env["diff_x_bits"]).sum(0)
        cnt["y_bit_mismatch"][b] = np.abs(env["diff_y_bits"]).sum(0)
        cnt["x_id_abs_diff"][b] = exact(np.abs(env["diff_x_bits"].astype(np.float64) @ w).sum())
        cnt["y_id_abs_diff"][b] = exact(np.abs(env["diff_y_bits"].astype(np.float64) @ w).sum())
        for m in ("visib", "full"):
            p, g = env["pred_seg_" + m][b], env["gt_seg_" + m][b]
            cnt[m + "_mismatch"][b] = exact(np.abs(p - g).sum())
            cnt[m + "_intersection"][b] = exact(np.logical_and(p, g).sum())
            cnt[m + "_union"][b] = exact(np.logical_or(p, g).sum())
        # ... and they do reproduce the reference's figures (float32 roundings of the reference aside)
        npt = max(cnt["n_in_roi"][b], 1)
        assert abs(fig["roi_bit_acc"][b] - (1 - cnt["roi_bit_mismatch"][b] / N)) <= 1e-6
        assert abs(fig["reproj_x_acc"][b] - (1 - cnt["x_id_abs_diff"][b] / npt / 2 ** nb)) <= 1e-6
        assert abs(fig["visib_pixel_acc"][b] - (1 - cnt["visib_mismatch"][b] / seg_size ** 2)) <= 1e-6
    out = dict(f16, mask_visib=(m_vis * 255).astype(np.uint8), mask_full=(m_full * 255).astype(np.uint8))
    out.update(fig)
    out.update({k: v.astype(np.int32) for k, v in cnt.items()})
    return out


def main():
    rng = np.random.default_rng(20240711)
    ns, discretise, report = reference_pieces()
    table = np.load(os.path.join(ROOT, "checkerpose_amd", "data", "fps_lm_15x4096.npy")).astype(np.float64)
    plan = [(0, 1, 512, "crop_square_resize", 64, s, p) for s, p in (("tall", "centre"), ("wide", "centre"), ("any", "centre"), ("tall", "edge"),
                                                                    ("wide", "edge"), ("any", "miss"), ("any", "centre"))]
    plan += [(1, 1, 512, "crop_resize", 128, s, p) for s, p in (("tall", "centre"), ("wide", "centre"), ("any", "edge"), ("any", "centre"))]
    plan += [(2, o, 4096, "crop_square_resize", 64, s, "centre") for o, s in ((2, "tall"), (1, "wide"), (3, "any"), (2, "any"))]
    crops = []
    for g, obj, N, method, S, shape, place in plan:
        e = draw_crop(rng, ns, discretise, table[obj - 1, :N], method, S, shape, place)
        e.update(group=g, obj=obj, N=N, method=method, S=S, no_det=False)
        crops.append(e)
        print("group %d obj %d N=%4d %-18s S=%3d %-4s %-6s box %-22s final %-22s in RoI %.3f" %
              (g, obj, N, method, S, shape, place, e["Bbox"].tolist(), e["final"].tolist(), e["roi"].mean()), flush=True)
    # the "no detection" sample of group 0 (bop_dataset_pytorch.py:328-338): dummy box, zero labels
    nd = dict(crops[0], group=0, no_det=True, Bbox=np.zeros(4, int), final=np.zeros(4, int), roi=np.zeros(512), x_code=np.zeros((512, 6)),
              y_code=np.zeros((512, 6)), x_id=np.zeros(512, int), y_id=np.zeros(512, int), proj_xy=np.zeros((512, 2)), depth=np.zeros(512),
              roi_xy_ori=np.zeros((64, 64, 2)), left=False, above=False, right=False, below=False)
    crops.insert(7, nd)
    real = [c for c in crops if not c["no_det"]]
    assert all(any(c[k] for c in real) for k in ("left", "above", "right", "below"))
    frac = sum(c["roi"].sum() for c in real) / sum(c["N"] for c in real)
    assert 0.1 <= frac <= 0.9, frac
    assert any(c["final"][0] < 0 for c in real) and any(c["final"][1] < 0 for c in real)
    assert any(c["final"][2] != c["final"][3] for c in real if c["method"] == "crop_resize")
    print("keypoints in the RoI over the fixture: %.3f" % frac)
    out = {"enc_group": np.array([c["group"] for c in crops]), "enc_obj": np.array([c["obj"] for c in crops]),
           "enc_N": np.array([c["N"] for c in crops]), "enc_S": np.array([c["S"] for c in crops]),
           "enc_method": np.array([c["method"] for c in crops]), "enc_no_det": np.array([c["no_det"] for c in crops]),
           "enc_K": K_LM, "enc_R": np.stack([c["R"] for c in crops]), "enc_t": np.stack([c["t"] for c in crops]),
           "enc_Bbox": np.stack([c["Bbox"] for c in crops]).astype(np.int32), "enc_final": np.stack([c["final"] for c in crops]).astype(np.int32),
           "img_wh": np.array([IMG_W, IMG_H])}
    for i, c in enumerate(crops):
        step = 8 if c["N"] == 4096 else 1                     # projections of the 4096-keypoint crops: every 8th keypoint
        out["enc%02d_roi" % i] = np.packbits(c["roi"].astype(np.uint8))
        out["enc%02d_x_code" % i] = np.packbits(c["x_code"].astype(np.uint8), axis=0)          # (ceil(N/8), bits)
        out["enc%02d_y_code" % i] = np.packbits(c["y_code"].astype(np.uint8), axis=0)
        out["enc%02d_x_id" % i] = c["x_id"].astype(np.int16)
        out["enc%02d_y_id" % i] = c["y_id"].astype(np.int16)
        out["enc%02d_proj_xy" % i] = c["proj_xy"][::step]
        out["enc%02d_depth" % i] = c["depth"][::step]
        out["enc%02d_roi_xy_corners" % i] = c["roi_xy_ori"][[0, 0, -1, -1], [0, -1, 0, -1]].astype(np.float32)   # the grid's 4 corners
    g0, g1 = [c for c in crops if c["group"] == 0], [c for c in crops if c["group"] == 1]
    for name, (cs, S, nb, seg_size) in {"rep0": (g0, 64, 6, 64), "rep1": (g0, 64, 5, 32), "rep2": (g1, 128, 6, 64)}.items():
        r = report_batch(ns, report, rng, cs, S, nb, seg_size)
        assert name != "rep0" or (r["visib_union"].min() == 0 and r["n_in_roi"].min() == 0)
        out.update({"%s_%s" % (name, k): v for k, v in r.items()})
        out[name + "_meta"] = np.array([cs[0]["group"], S, nb, seg_size])
        print(name, "roi_bit_acc", np.round(r["roi_bit_acc"], 4), "visib_iou", np.round(r["visib_iou"], 4))
    # aug_Bbox under fixed seeds
    boxes, ratios, seeds, res = [], [], [], []
    for i in range(32):
        gt = np.array([int(rng.integers(-40, 560)), int(rng.integers(-40, 400)), int(rng.integers(12, 300)), int(rng.integers(12, 300))])
        ratio = (1.5, 1.2, 1.0)[i % 3]
        np.random.seed(1000 + i)
        res.append(ns["aug_Bbox"](gt, ratio))
        boxes.append(gt); ratios.append(ratio); seeds.append(1000 + i)
    out.update(aug_in=np.array(boxes, dtype=np.int32), aug_ratio=np.array(ratios), aug_seed=np.array(seeds), aug_out=np.array(res, dtype=np.int32))
    # re / te of the pose-error fixture's poses
    pe = np.load(os.path.join(HERE, "pose_error.npz"))
    out["pose_re"] = np.array([pose_error.re(pe["R_est"][c], pe["R_gt"][c]) for c in range(len(pe["add"]))])
    out["pose_te"] = np.array([pose_error.te(pe["t_est"][c].reshape(3, 1), pe["t_gt"][c].reshape(3, 1)) for c in range(len(pe["add"]))])
    path = os.path.join(HERE, "targets.npz")
    np.savez_compressed(path, **out)
    print("wrote targets.npz: %d crops, %d bytes" % (len(crops), os.path.getsize(path)))


if __name__ == "__main__":
    main()
