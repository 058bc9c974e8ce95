"""On-device pose scoring: the twin of the reference's metric.py and of the scoring block of its test
scripts (test.py:378-427, test_lm.py:300-321, compute_auc_posecnn test.py:37-57).

  pose_errors(...)                       batched ADD / ADD-S (ADI) on device tensors -- takes what solve_pnp_ransac returns
  Calculate_ADD_Error_BOP / _ADI_        the reference's names and numpy-in, float-out signatures (one pose; B = 1 of the above)
  compute_auc_posecnn, summarize         pass rates at 2 / 5 / 10 % of the diameter and the PoseCNN AUC (host: one float per image)
  bop_errors, mssd / mspd / proj, bop_recall, summarize_bop                   BOP's MSSD / MSPD / projection error (row N7): below
  vsd_errors, vsd, render_depth, vsd_from_depth, vsd_taus                     BOP's VSD with its depth rasteriser (row N8): below
  mask_errors, mask_overlap, box_overlap, cus / cou_bb_proj / cou_mask / cou_bb   BOP's overlap errors (row N12): at the end

This module holds the error functions, the recall and summary functions and the one-pose wrappers under the reference's names.  The
containers (MeshSet, SymmetrySet, symmetry_transformations, the host calc_pts_diameter) live in checkerpose_amd/scene.py and are
importable from here as before; the handling of poses, camera, mesh / image ids, frame size and kinds is scene's too, and every
launch goes through _abi.call.

ADI is an all-pairs search: V^2 distance evaluations per pose and no spatial index.  Measured on one MI355X (tools/pose_error_bench.py,
profiles/pose_error_bench.json): one pose takes 0.16 / 0.36 / 1.44 ms at 4 096 / 20 480 / 61 440 vertices, 256 poses 0.60 / 11.6 / 101 ms
(about 9e12 pairs/s when the chip is full); beyond about 1e5 vertices subsample the mesh (the reference's own LM tables are 4 096
farthest-point samples per object).  There is no CPU fallback."""
import ctypes as C

import numpy as np
import torch

from . import _abi, scene
from .scene import MeshSet, SymmetrySet, calc_pts_diameter, symmetry_transformations   # noqa: F401  (their public home was here)

KINDS = {"add": _abi.POSE_ERR_ADD, "adi": _abi.POSE_ERR_ADI}


def pose_errors(R_est, t_est, R_gt, t_gt, vertices, mesh_ids=None, kinds=("add", "adi")):
    """ADD and / or ADD-S (ADI) of B poses against their ground truth, on the device (cp_pose_errors).
      R_est, t_est: (B,3,3) / (B,3,1) CUDA tensors, e.g. straight from solve_pnp_ransac; R_gt, t_gt: the same shapes (tensors on the
      same device, or host arrays, which are uploaded: 96 bytes per pose);
      vertices: one (V,3) array / tensor for every pose, a list of them, or a MeshSet; with several meshes `mesh_ids` (B,) names
      each pose's mesh;  kinds: any of "add", "adi".
    R_est is taken as ORTHONORMAL (the solver's poses and its identity fallback are): the kernel works in the model frame with the
    relative pose I + R_est^T (R_gt - R_est), which is the reference's rigid change of frame only then -- with a sheared or scaled
    estimate neither the reference's ADD nor R_est^T R_gt is what comes out.  A pose with a NaN / inf entry scores NaN in both errors.
    -> dict kind -> (B,) float64 CUDA tensor, in the vertices' units.  ADI costs V^2 per pose (module docstring)."""
    scene.require_cuda("metric", R_est, t_est)
    dev = R_est.device
    mask = scene.kinds_mask(kinds, KINDS, "kinds is empty: ask for \"add\", \"adi\" or both")
    est = scene.pack_poses(R_est, t_est)
    B = est.shape[0]
    if B == 0:
        raise ValueError("no poses")
    gt = scene.pack_poses(R_gt, t_gt, B, dev)
    ms = scene.as_meshset(vertices)
    verts, offsets = ms.on(dev)
    ids, (vmax,) = scene.mesh_ids_on(mesh_ids, B, dev, ms.sizes)
    out = {k: torch.empty(B, dtype=torch.float64, device=dev) for k, bit in KINDS.items() if mask & bit}
    scratch = None
    if mask & KINDS["adi"]:
        scratch = torch.empty(_abi.load().cp_pose_errors_scratch_bytes(B, vmax), dtype=torch.uint8, device=dev)
    _abi.call("cp_pose_errors", dev, est, gt, verts, offsets, len(ms), ids, B, vmax, mask, out.get("add"), out.get("adi"), scratch)
    return out


def _one_pose(kind, R_GT, t_GT, R_predict, t_predict, vertices, device):
    dev = scene.cuda_device("metric", device)
    out = pose_errors(*scene.upload_pose(R_predict, t_predict, dev), *scene.upload_pose(R_GT, t_GT, dev), vertices, kinds=(kind,))
    return float(out[kind][0])


def Calculate_ADD_Error_BOP(R_GT, t_GT, R_predict, t_predict, vertices, device="cuda:0"):
    """the reference's metric.py:8-12 (numpy arrays of one pose -> float), scored on the device"""
    return _one_pose("add", R_GT, t_GT, R_predict, t_predict, vertices, device)


def Calculate_ADI_Error_BOP(R_GT, t_GT, R_predict, t_predict, vertices, device="cuda:0"):
    """the reference's metric.py:14-18 (numpy arrays of one pose -> float), scored on the device"""
    return _one_pose("adi", R_GT, t_GT, R_predict, t_predict, vertices, device)


def compute_auc_posecnn(errors):
    """Area under the accuracy-threshold curve up to 0.1 (errors in metres), as test.py:37-57 computes it after the YCB-Video
    toolbox: errors above 0.1 count as misses; nan when there is no error or none within 0.1."""
    d = np.sort(np.asarray(errors, dtype=np.float64).reshape(-1))
    n = d.shape[0]
    hit = d <= 0.1
    if n == 0 or not hit.any():
        return np.nan
    rec = d[hit]
    prec = (np.arange(1, n + 1, dtype=np.float64) / n)[hit]
    mrec = np.concatenate(([0.0], rec, [0.1]))
    mpre = np.maximum.accumulate(np.concatenate(([0.0], prec, [prec[-1]])))
    step = np.nonzero(mrec[1:] != mrec[:-1])[0] + 1
    return float(((mrec[step] - mrec[step - 1]) * mpre[step]).sum() * 10)


def _to_numpy(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _summary(err, diam):
    """err (n,), diam (n,): pass rates with the strict `<` of test.py:382-386 and the AUC of err / 1000 (test.py:480)"""
    err = np.where(np.isnan(err), 10000.0, err)             # test.py:379-380
    n = err.shape[0]
    out = {"count": int(n)}
    for pct, f in ((2, 0.02), (5, 0.05), (10, 0.1)):
        out["passed_%d" % pct] = float((err < f * diam).sum()) / n if n else float("nan")
    out["auc_posecnn"] = compute_auc_posecnn(err / 1000.0)
    return out


def summarize(errors, diameters, symmetric=None, mesh_ids=None):
    """The numbers test.py / test_lm.py print from the per-image errors (in mm).
      errors: the dict pose_errors() returns (or {"add": ..., "adi": ...} arrays); diameters: a float, one per pose, or -- with
      mesh_ids -- one per mesh (MeshSet.diameters); symmetric: bool or per-mesh bools: ADI is the main metric of a symmetric object
      and ADD the supplementary one, the other way round otherwise (test.py:127-136).
    -> {"passed_2", "passed_5", "passed_10", "auc_posecnn", "count"} of the main metric (+ "supp_*" of the other one when both
    errors are given); with mesh_ids also "per_mesh": {mesh id -> the same dict for that mesh's poses} (test_lm.py:319-321)."""
    err = {k: _to_numpy(v).astype(np.float64).reshape(-1) for k, v in errors.items()}
    if not err or set(err) - set(KINDS):
        raise ValueError("errors must hold \"add\" and / or \"adi\"")
    n = next(iter(err.values())).shape[0]
    ids = None if mesh_ids is None else _to_numpy(mesh_ids).astype(np.int64).reshape(-1)
    diam = np.asarray(diameters, dtype=np.float64).reshape(-1)
    sym = np.zeros(1, bool) if symmetric is None else np.asarray(symmetric, dtype=bool).reshape(-1)
    if ids is not None:
        diam = diam[ids] if diam.shape[0] != 1 else np.broadcast_to(diam, (n,))
        sym = sym[ids] if sym.shape[0] != 1 else np.broadcast_to(sym, (n,))
    else:
        diam, sym = np.broadcast_to(diam, (n,)), np.broadcast_to(sym, (n,))
    for k in ("adi" if sym.any() else None, "add" if (~sym).any() else None):
        if k is not None and k not in err:
            raise ValueError("the main metric of %s objects is %r: it is not among the errors given"
                             % ("symmetric" if k == "adi" else "non-symmetric", k))
    both = len(err) == 2

    def block(sel):
        main = np.where(sym[sel], err["adi"][sel] if "adi" in err else 0.0, err["add"][sel] if "add" in err else 0.0)
        out = _summary(main, diam[sel])
        if both:
            supp = np.where(sym[sel], err["add"][sel], err["adi"][sel])
            out.update({"supp_" + k: v for k, v in _summary(supp, diam[sel]).items() if k != "count"})
        return out

    res = block(np.ones(n, bool))
    if ids is not None:
        res["per_mesh"] = {int(m): block(ids == m) for m in np.unique(ids)}
    return res


# ---- BOP's MSSD / MSPD / projection error (cp_bop_errors) ---------------------------------------------------------
# The twin of the three renderer-free functions of bop_toolkit_lib/pose_error.py (mssd :96-118, mspd :121-144, proj :217-232) and of
# the recall eval_bop19_pose.py / eval_calc_scores.py compute from them (misc.get_symmetry_transformations: scene.SymmetrySet).
#   bop_errors(...)                        batched, on device tensors -- takes what solve_pnp_ransac returns
#   mssd / mspd / proj                     bop_toolkit's names and numpy-in, float-out signatures (B = 1 of the above)
#   bop_recall, summarize_bop              recall per threshold and its mean (AR_MSSD / AR_MSPD); host: one float per pose
BOP_KINDS = {"mssd": _abi.BOP_ERR_MSSD, "mspd": _abi.BOP_ERR_MSPD, "proj": _abi.BOP_ERR_PROJ}
_BOP_MAPS = {None: 0, "small": _abi.BOP_MAP_SMALL, "large": _abi.BOP_MAP_LARGE}


def bop_errors(R_est, t_est, R_gt, t_gt, cam_K, vertices, symmetries=None, mesh_ids=None, kinds=("mssd", "mspd", "proj"), _mapping=None):
    """BOP's MSSD, MSPD and / or projection error of B poses against their ground truth, on the device (cp_bop_errors).
      R_est, t_est: (B,3,3) / (B,3,1) CUDA tensors, e.g. straight from solve_pnp_ransac; R_gt, t_gt: the same shapes (tensors on the
      same device, or host arrays, which are uploaded);  cam_K: (3,3) for every pose or (B,3,3), tensor or array;
      vertices: one (V,3) array / tensor for every pose, a list of them, or a MeshSet; with several meshes `mesh_ids` (B,), on the
      host or on the device, names each pose's mesh;  symmetries: a SymmetrySet in the same mesh order, a list of bop_toolkit `syms`
      lists, or None = the identity alone for every mesh;  kinds: any of "mssd", "mspd", "proj".
    MSSD comes in the vertices' units, MSPD and proj in pixels of cam_K.  A pose with a NaN / inf entry (either pose, or K), or a
    device-side mesh id outside 0..M-1, scores NaN in every kind.  `_mapping` ("small" / "large") forces one of the kernel's two
    mappings (measurement and tests: results are bit-identical).
    -> dict kind -> (B,) float64 CUDA tensor."""
    scene.require_cuda("metric", R_est, t_est)
    dev = R_est.device
    mask = scene.kinds_mask(kinds, BOP_KINDS, "kinds is empty: ask for \"mssd\", \"mspd\" and / or \"proj\"")
    if _mapping not in _BOP_MAPS:
        raise ValueError("_mapping must be None, \"small\" or \"large\"")
    est = scene.pack_poses(R_est, t_est)
    B = est.shape[0]
    if B == 0:
        raise ValueError("no poses")
    gt = scene.pack_poses(R_gt, t_gt, B, dev)
    K, k_stride = scene.camera(cam_K, B, dev)
    ms = scene.as_meshset(vertices)
    M = len(ms)
    ss = scene.as_symmetries(symmetries, M)
    verts, v_off = ms.on(dev)
    table, s_off = ss.on(dev)
    ids, (vmax, smax) = scene.mesh_ids_on(mesh_ids, B, dev, ms.sizes, ss.sizes)
    out = {k: torch.empty(B, dtype=torch.float64, device=dev) for k, bit in BOP_KINDS.items() if mask & bit}
    scratch = torch.empty(_abi.load().cp_bop_errors_map_scratch_bytes(B, smax, vmax, _BOP_MAPS[_mapping]), dtype=torch.uint8, device=dev)
    _abi.call("cp_bop_errors", dev, est, gt, K, k_stride, verts, v_off, table, s_off, M, ids, B, vmax, smax, mask | _BOP_MAPS[_mapping],
              out.get("mssd"), out.get("mspd"), out.get("proj"), scratch)
    return out


def _one_bop(kind, R_est, t_est, R_gt, t_gt, K, pts, syms, device):
    dev = scene.cuda_device("metric", device)
    out = bop_errors(*scene.upload_pose(R_est, t_est, dev), *scene.upload_pose(R_gt, t_gt, dev),
                     np.eye(3) if K is None else np.asarray(K, dtype=np.float64).reshape(3, 3), pts,
                     symmetries=None if syms is None else [list(syms)], kinds=(kind,))
    return float(out[kind][0])


def mssd(R_est, t_est, R_gt, t_gt, pts, syms, device="cuda:0"):
    """bop_toolkit_lib.pose_error.mssd (numpy arrays of one pose -> float), scored on the device"""
    return _one_bop("mssd", R_est, t_est, R_gt, t_gt, None, pts, syms, device)


def mspd(R_est, t_est, R_gt, t_gt, K, pts, syms, device="cuda:0"):
    """bop_toolkit_lib.pose_error.mspd (numpy arrays of one pose -> float), scored on the device"""
    return _one_bop("mspd", R_est, t_est, R_gt, t_gt, K, pts, syms, device)


def proj(R_est, t_est, R_gt, t_gt, K, pts, device="cuda:0"):
    """bop_toolkit_lib.pose_error.proj (numpy arrays of one pose -> float), scored on the device"""
    return _one_bop("proj", R_est, t_est, R_gt, t_gt, K, pts, None, device)


def bop_thresholds(kind):
    """eval_bop19_pose.py:46,51: the ten thresholds of correctness of MSSD (fractions of the diameter) and MSPD (pixels at width 640)"""
    if kind == "mssd":
        return np.arange(0.05, 0.51, 0.05)
    if kind == "mspd":
        return np.arange(5, 51, 5)
    if kind == "vsd":                                      # eval_bop19_pose.py:31,34: vsd_taus and its correct_th are the same ten values
        return np.arange(0.05, 0.51, 0.05)
    if kind == "cus":                                      # eval_calc_scores.py:43
        return np.array([0.5])
    if kind in ("re", "te"):                               # eval_calc_scores.py:45-46: degrees, centimetres
        return np.array([5.0])
    if kind == "rete":                                     # eval_calc_scores.py:44: one two-element threshold [deg, cm]
        return np.array([[5.0, 5.0]])
    raise ValueError("%r has no default thresholds (BOP'19 scores \"mssd\" and \"mspd\"): pass `thresholds`" % (kind,))


def bop_recall(errors, kind, diameters=None, im_width=None, thresholds=None, mesh_ids=None):
    """Recall of one error kind over its thresholds, with ONE estimate per target as test.py produces (then BOP's greedy matching is
    the comparison alone): eval_calc_scores.py:246-263 + pose_matching.py:68.
      errors: (n,) tensor / array of `kind` ("mssd", "mspd", "proj" or "cus");  MSSD is divided by the diameter (`diameters`: a float,
      one per pose, or -- with mesh_ids -- one per mesh), MSPD is multiplied by 640 / im_width, proj and cus are taken as they are;  thresholds:
      default bop_thresholds(kind).  A pose is correct when error < threshold, STRICT; NaN is a miss.
    -> {"thresholds", "correct": (n, T) bool, "recall": (T,), "AR_<KIND>": their mean, "count"} and, with mesh_ids,
       "per_mesh": {mesh id -> {"recall", "AR_<KIND>", "count"}}.
    Several estimates or instances per target, or a targets file: checkerpose_amd.bop_eval does the matching (row N11)."""
    if kind == "vsd":
        return _vsd_recall(errors, thresholds, mesh_ids)
    if kind not in BOP_KINDS and kind != "cus":
        raise ValueError("kind must be among %s, got %r" % (sorted(BOP_KINDS) + ["cus", "vsd"], kind))
    e = _to_numpy(errors).astype(np.float64).reshape(-1)
    n = e.shape[0]
    ids = None if mesh_ids is None else _to_numpy(mesh_ids).astype(np.int64).reshape(-1)
    if kind == "mssd":
        if diameters is None:
            raise ValueError("MSSD is scored relative to the object diameter: pass `diameters`")
        diam = np.asarray(diameters, dtype=np.float64).reshape(-1)
        diam = diam[ids] if (ids is not None and diam.shape[0] != 1) else np.broadcast_to(diam, (n,))
        e = e / diam
    elif kind == "mspd":
        if im_width is None:
            raise ValueError("MSPD is scored at an image width of 640: pass `im_width`")
        e = (640.0 / float(im_width)) * e
    th = bop_thresholds(kind) if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    correct = e[:, None] < th[None, :]
    name = "AR_" + kind.upper()

    def block(sel):
        c = correct[sel]
        rec = c.mean(0) if c.shape[0] else np.full(th.shape[0], np.nan)
        return {"recall": rec, name: float(rec.mean()), "count": int(c.shape[0])}

    res = block(np.ones(n, bool))
    res.update({"thresholds": th, "correct": correct})
    if ids is not None:
        res["per_mesh"] = {int(m): block(ids == m) for m in np.unique(ids)}
    return res


def _vsd_recall(errors, thresholds, mesh_ids):
    """bop_recall(.., "vsd"): errors (n, T), one column per tau (vsd_errors' "vsd"); a pose is correct for the pair (tau, threshold)
    when its error at that tau < threshold, STRICT; NaN is a miss (eval_calc_scores.py:246-263 run once per tau).
    -> {"thresholds", "correct": (n, T, Th) bool, "recall": (T, Th), "AR_VSD": their mean over all pairs, "count"} (+ "per_mesh")"""
    e = _to_numpy(errors).astype(np.float64)
    if e.ndim != 2:
        raise ValueError("VSD errors must be (n, T), one column per tau; got %r" % (e.shape,))
    th = bop_thresholds("vsd") if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    correct = e[:, :, None] < th[None, None, :]
    ids = None if mesh_ids is None else _to_numpy(mesh_ids).astype(np.int64).reshape(-1)

    def block(sel):
        c = correct[sel]
        rec = c.mean(0) if c.shape[0] else np.full(correct.shape[1:], np.nan)
        return {"recall": rec, "AR_VSD": float(rec.mean()), "count": int(c.shape[0])}

    res = block(np.ones(e.shape[0], bool))
    res.update({"thresholds": th, "correct": correct})
    if ids is not None:
        res["per_mesh"] = {int(m): block(ids == m) for m in np.unique(ids)}
    return res


def summarize_bop(errors, diameters=None, im_width=None, mesh_ids=None, thresholds=None):
    """bop_recall of every kind in `errors` (the dict bop_errors returns; other keys, e.g. "add", are ignored; "proj" only when
    `thresholds` names it).  thresholds: optional dict kind -> thresholds.
    -> {kind: bop_recall's dict} plus "AR_MSSD" / "AR_MSPD" at the top.  With "vsd" in `errors` (vsd_errors' (n, T) array) also
    "vsd" / "AR_VSD", and -- when all three are there -- "AR" = mean(AR_VSD, AR_MSSD, AR_MSPD) (eval_bop19_pose.py:243).
    One estimate per target is assumed; checkerpose_amd.bop_eval.evaluate_results matches several to several (row N11)."""
    thresholds = thresholds or {}
    res = {}
    for kind in BOP_KINDS:
        if kind not in errors or (kind == "proj" and "proj" not in thresholds):
            continue
        res[kind] = bop_recall(errors[kind], kind, diameters=diameters, im_width=im_width, thresholds=thresholds.get(kind), mesh_ids=mesh_ids)
        res["AR_" + kind.upper()] = res[kind]["AR_" + kind.upper()]
    if "vsd" in errors:
        res["vsd"] = bop_recall(errors["vsd"], "vsd", thresholds=thresholds.get("vsd"), mesh_ids=mesh_ids)
        res["AR_VSD"] = res["vsd"]["AR_VSD"]
        if "AR_MSSD" in res and "AR_MSPD" in res:
            res["AR"] = float(np.mean([res["AR_VSD"], res["AR_MSSD"], res["AR_MSPD"]]))
    if not res:
        raise ValueError("errors holds none of \"mssd\", \"mspd\", \"vsd\" (or \"proj\" with thresholds)")
    return res


def score_poses(R_est, t_est, R_gt, t_gt, cam_K, vertices, mesh_ids=None, kinds=("add", "adi"), symmetries=None, depth_test=None,
                image_ids=None, size=None, **vsd_kwargs):
    """pose_errors, bop_errors, vsd_errors and / or mask_errors by the kinds asked (postprocess.evaluate_poses, targets.evaluate_batch):
    kinds of "add" / "adi" alone are exactly pose_errors -- nothing else is launched.  "vsd" needs `depth_test` (and a MeshSet with
    faces); vsd_kwargs (delta, taus, normalized_by_diameter, sphere_check) go to vsd_errors; its (B, T) errors come back under "vsd".
    "cus" / "cou_bb_proj" need `size` = (W, H) (and a MeshSet with faces): mask_errors, without the sphere shortcut."""
    names = [kinds] if isinstance(kinds, str) else list(kinds)
    want_vsd = "vsd" in names
    masks = [k for k in names if k in MASK_KINDS]
    names = [k for k in names if k != "vsd" and k not in MASK_KINDS]
    if want_vsd and depth_test is None:
        raise ValueError("kind \"vsd\" needs depth_test")
    if masks and size is None:
        raise ValueError("kinds \"cus\" / \"cou_bb_proj\" need size=(W, H)")
    bop = [k for k in names if k in BOP_KINDS]
    if not bop and not want_vsd and not masks:
        return pose_errors(R_est, t_est, R_gt, t_gt, vertices, mesh_ids=mesh_ids, kinds=kinds)
    rest = [k for k in names if k not in BOP_KINDS]
    out = pose_errors(R_est, t_est, R_gt, t_gt, vertices, mesh_ids=mesh_ids, kinds=rest) if rest else {}
    if bop:
        out.update(bop_errors(R_est, t_est, R_gt, t_gt, cam_K, vertices, symmetries=symmetries, mesh_ids=mesh_ids, kinds=bop))
    if want_vsd:
        out["vsd"] = vsd_errors(R_est, t_est, R_gt, t_gt, cam_K, vertices, depth_test, image_ids=image_ids, mesh_ids=mesh_ids,
                                **vsd_kwargs)["vsd"]
    if masks:
        out.update(mask_errors(R_est, t_est, R_gt, t_gt, cam_K, vertices, size, mesh_ids=mesh_ids, kinds=masks))
    return out


# ---- BOP's VSD (cp_vsd_errors) ------------------------------------------------------------------------------------
# The twin of bop_toolkit_lib/pose_error.py:17-93 (vsd) with the renderer it asks for: a depth rasteriser in HIP fused with the
# reference's pixel counting.  The reference's own renderers (vispy / OpenGL / the C++ bop_renderer) do not run here.
#   vsd_errors(...)                        batched, on device tensors -- takes what solve_pnp_ransac returns, and depth images
#   vsd                                    bop_toolkit's name and signature (one pose; `renderer` is a MeshSet with faces)
#   render_depth                           the rasteriser alone
#   bop_recall(.., "vsd"), summarize_bop   recall per (tau, threshold) pair, AR_VSD and BOP'19's AR
def vsd_taus(taus):
    """the misalignment tolerances of VSD (default bop_thresholds("vsd")) -> (float64 (T,) array, the same as a ctypes double[T])"""
    tv = bop_thresholds("vsd") if taus is None else np.asarray(taus, dtype=np.float64).reshape(-1)
    if not 1 <= tv.shape[0] <= 16 or not np.isfinite(tv).all():
        raise ValueError("taus: 1 to 16 finite values")
    return tv, (C.c_double * tv.shape[0])(*tv.tolist())


def vsd_errors(R_est, t_est, R_gt, t_gt, cam_K, meshes, depth_test, image_ids=None, delta=15.0, taus=None, normalized_by_diameter=True,
               mesh_ids=None, sphere_check=True, return_counts=False, return_depth=False):
    """BOP's VSD of B poses against their ground truth, rendered and counted on the device (cp_vsd_errors).
      R_est, t_est: (B,3,3) / (B,3,1) CUDA tensors; R_gt, t_gt: the same shapes (tensors or host arrays); cam_K: (3,3) or (B,3,3);
      meshes: a MeshSet built with faces (with several meshes, mesh_ids (B,) names each pose's);  depth_test: (H,W) or (I,H,W) depth
      images in the vertices' units (mm; 0 = no measurement), image_ids (B,) names each pose's image (default: the one image, or
      image b for pose b when I == B);  delta: the visibility tolerance (15 mm for lm / lmo / ycbv);  taus: default
      bop_thresholds("vsd");  sphere_check: the shortcut of bop_toolkit's caller (eval_calc_errors.py:299-318) -- a pose whose
      sphere projection does not overlap the ground truth's is not rendered and scores 1.0 at every tau.
    A pose with a NaN / inf entry, a device-side mesh / image id out of range, or any vertex at Z <= 0 scores NaN (a miss).
    -> {"vsd": (B,T) float64 CUDA tensor} (+ "counts": (B,T+2) int32 = union, inter, cost count per tau; + "depth": (B,2,H,W)
    float32 = the estimate's and the ground truth's render).  The counts are the same bits with or without the depth output."""
    dev, est, B = scene.mesh_poses(R_est, t_est, meshes)
    K, k_stride = scene.camera(cam_K, B, dev)
    ids, (vmax,) = scene.mesh_ids_on(mesh_ids, B, dev, meshes.sizes)
    gt = scene.pack_poses(R_gt, t_gt, B, dev)
    d, img, n_img = scene.depth_images(depth_test, image_ids, B, dev)
    H, W = int(d.shape[1]), int(d.shape[2])
    tv, ctaus = vsd_taus(taus)
    T = tv.shape[0]
    verts, v_off = meshes.on(dev)
    faces, f_off, diam = meshes.faces_on(dev)
    err = torch.empty((B, T), dtype=torch.float64, device=dev)
    counts = torch.empty((B, T + 2), dtype=torch.int32, device=dev)
    depth = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev) if return_depth else None
    scratch = torch.empty(_abi.load().cp_vsd_errors_scratch_bytes(B, vmax, H, W), dtype=torch.uint8, device=dev)
    _abi.call("cp_vsd_errors", dev, est, gt, K, k_stride, verts, v_off, faces, f_off, len(meshes), ids, d, img, n_img, H, W, float(delta),
              diam, ctaus, T, 1 if normalized_by_diameter else 0, 1 if sphere_check else 0, B, vmax, err, counts, depth, scratch)
    out = {"vsd": err}
    if return_counts:
        out["counts"] = counts
    if return_depth:
        out["depth"] = depth
    return out


def vsd_from_depth(depth_est, depth_gt, depth_test, cam_K, diameters, image_ids=None, delta=15.0, taus=None, normalized_by_diameter=True):
    """vsd_errors' counting on caller-supplied renders (cp_vsd_from_depth): depth_est, depth_gt (B,H,W) float32 CUDA tensors;
    diameters: a float or one per pose.  -> {"vsd": (B,T) f64, "counts": (B,T+2) int32}"""
    scene.require_cuda("metric", depth_est, depth_gt)
    if depth_est.dim() != 3 or depth_est.shape != depth_gt.shape:
        raise ValueError("depth_est and depth_gt must both be (B,H,W)")
    dev = depth_est.device
    de = depth_est.to(torch.float32).contiguous()
    dg = depth_gt.to(device=dev, dtype=torch.float32).contiguous()
    B, H, W = (int(v) for v in de.shape)
    if B == 0:
        raise ValueError("no poses")
    d, img, n_img = scene.depth_images(depth_test, image_ids, B, dev)
    if tuple(d.shape[1:]) != (H, W):
        raise ValueError("depth_test is %r, the renders are %r" % (tuple(d.shape[1:]), (H, W)))
    K, k_stride = scene.camera(cam_K, B, dev)
    diam = np.asarray(diameters, dtype=np.float64).reshape(-1)
    if diam.shape[0] not in (1, B):
        raise ValueError("diameters: a float or one per pose")
    diam = torch.from_numpy(np.array(np.broadcast_to(diam, (B,)), dtype=np.float64)).to(dev)
    tv, ctaus = vsd_taus(taus)
    T = tv.shape[0]
    err = torch.empty((B, T), dtype=torch.float64, device=dev)
    counts = torch.empty((B, T + 2), dtype=torch.int32, device=dev)
    scratch = torch.empty(_abi.load().cp_vsd_errors_scratch_bytes(B, 0, H, W), dtype=torch.uint8, device=dev)
    _abi.call("cp_vsd_from_depth", dev, de, dg, K, k_stride, d, img, n_img, H, W, float(delta), diam, ctaus, T,
              1 if normalized_by_diameter else 0, B, err, counts, scratch)
    return {"vsd": err, "counts": counts}


def render_depth(R, t, cam_K, meshes, size, mesh_ids=None):
    """Depth images of B poses of `meshes` (a MeshSet with faces), rendered on the device (cp_render_depth): depth[b, y, x] is the
    eye-space Z of the front-most surface on the ray through image point (x + 0.5, y + 0.5), 0 where there is none -- what
    bop_toolkit's renderer.render_object(...)['depth'] holds.  size: (width, height), as bop_toolkit's renderers take it.
    A pose with a non-finite entry or any vertex at Z <= 0 renders nothing (zeros).  -> (B,H,W) float32 CUDA tensor"""
    dev, poses, B = scene.mesh_poses(R, t, meshes)
    K, k_stride = scene.camera(cam_K, B, dev)
    ids, (vmax,) = scene.mesh_ids_on(mesh_ids, B, dev, meshes.sizes)
    W, H = scene.frame_size(size)
    verts, v_off = meshes.on(dev)
    faces, f_off, _ = meshes.faces_on(dev)
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    scratch = torch.empty(_abi.load().cp_vsd_errors_scratch_bytes(B, vmax, H, W), dtype=torch.uint8, device=dev)
    _abi.call("cp_render_depth", dev, poses, K, k_stride, verts, v_off, faces, f_off, len(meshes), ids, H, W, B, vmax, depth, scratch)
    return depth


def vsd(R_est, t_est, R_gt, t_gt, depth_test, K, delta, taus, normalized_by_diameter, diameter, renderer, obj_id, cost_type="step",
        device="cuda:0"):
    """bop_toolkit_lib.pose_error.vsd (numpy arrays of one pose -> list of floats, one per tau), rendered and scored on the device.
    `renderer` is a MeshSet with faces and `obj_id` the index of the object's mesh in it; `diameter` is the one the distances are
    normalised by (it replaces the MeshSet's for this call).  Only the 'step' cost exists.  No sphere shortcut: that is the caller's."""
    if cost_type != "step":
        raise ValueError("only the 'step' pixel-wise matching cost is implemented")
    dev = scene.cuda_device("metric", device)
    if not isinstance(renderer, MeshSet) or renderer.faces is None:
        raise ValueError("renderer must be a MeshSet built with faces")
    m = int(obj_id)
    if not 0 <= m < len(renderer):
        raise ValueError("obj_id must be a mesh index in 0..%d" % (len(renderer) - 1))
    v0, v1 = int(renderer.offsets[m]), int(renderer.offsets[m + 1])
    f0, f1 = int(renderer.face_offsets[m]), int(renderer.face_offsets[m + 1])
    one = MeshSet.from_arrays([renderer.verts[v0:v1]], diameters=[float(diameter)], faces=[renderer.faces[f0:f1]])
    out = vsd_errors(*scene.upload_pose(R_est, t_est, dev), *scene.upload_pose(R_gt, t_gt, dev),
                     np.asarray(K, dtype=np.float64).reshape(3, 3), one, np.asarray(depth_test, dtype=np.float32), delta=delta, taus=taus,
                     normalized_by_diameter=normalized_by_diameter, sphere_check=False)
    return [float(v) for v in out["vsd"][0].cpu()]


# ---- BOP's overlap errors (cp_mask_errors / cp_mask_overlap / cp_box_overlap) ------------------------------------
# The twin of the last four functions of bop_toolkit_lib/pose_error.py: cou_mask :235-253, cus :256-286, cou_bb :289-297, cou_bb_proj
# :300-330 (with misc.calc_2d_bbox / misc.iou).  With them every error of that file runs on the device.
#   mask_errors(...)                       batched cus / cou_bb_proj: both silhouettes rasterised per tile, nothing stored unless asked
#   mask_overlap(...)                      the counting half on caller-supplied masks: cou_mask, and cou_bb of the masks' boxes
#   box_overlap(...)                       1 - iou of box pairs
#   cou_mask, cou_bb, cus, cou_bb_proj     bop_toolkit's names and argument order (one pair)
MASK_KINDS = ("cus", "cou_bb_proj")
OVERLAP_KINDS = ("cou_mask", "cou_bb")


def mask_errors(R_est, t_est, R_gt, t_gt, cam_K, meshes, size, mesh_ids=None, kinds=("cus", "cou_bb_proj"), sphere_check=False,
                return_counts=False, return_boxes=False, return_masks=False):
    """BOP's 'cus' (complement over union of the projected silhouettes) and / or 'cou_bb_proj' (of their bounding boxes) of B poses
    against their ground truth, rendered and counted on the device (cp_mask_errors).
      R_est, t_est: (B,3,3) / (B,3,1) CUDA tensors, e.g. straight from solve_pnp_ransac; R_gt, t_gt: the same shapes (tensors or host
      arrays); cam_K: (3,3) or (B,3,3); meshes: a MeshSet built with faces (with several meshes, mesh_ids (B,) names each pair's);
      size: (width, height) of the frame, as bop_toolkit's renderers take it;  kinds: any of "cus", "cou_bb_proj";
      sphere_check: the shortcut of bop_toolkit's caller (eval_calc_errors.py:299-302,357-362), which belongs to 'cus' ALONE -- a pair
      whose sphere projections do not overlap scores cus = 1.0 unrendered; cou_bb_proj is computed whatever the check says.
    A silhouette pixel is set exactly where render_depth(..., size) > 0.  cus = 1 - inter / union, 1.0 when the union is empty.
    cou_bb_proj = 1 - iou of the boxes (xmin, ymin, xmax - xmin, ymax - ymin): no + 1, not clipped; where a side's silhouette is
    EMPTY (e.g. wholly outside the frame) the reference raises (xs.min() of nothing) -- here cou_bb_proj is NaN, a miss under the
    strict `<` of the matching.  A pair with a NaN / inf entry, a device-side mesh id out of range, or any vertex at Z <= 0 on
    either side scores NaN in both kinds.
    -> dict kind -> (B,) float64 CUDA tensor; + "counts": (B,4) int32 = inter, union, n_est, n_gt and "ok": (B,) bool
    (return_counts); + "boxes": (B,2,4) int32 = the estimate's and the ground truth's x, y, w, h, -1 where empty (return_boxes);
    + "masks": (B,2,H,W) bool (return_masks).  A sphere-skipped pair that is not rendered (no "cou_bb_proj" among the kinds) has
    counts 0, boxes -1 and empty masks.  The errors are the same bits with or without the optional outputs.
    return_masks forfeits the early leave: every tile of every pair then walks its pixels to store them (zeros where nothing is
    rendered), which is the stored-image cost the fused call otherwise avoids -- ask for masks only when they are wanted."""
    mask = scene.kinds_mask(kinds, MASK_KINDS, "kinds is empty: ask for \"cus\", \"cou_bb_proj\" or both")
    dev, est, B = scene.mesh_poses(R_est, t_est, meshes)
    K, k_stride = scene.camera(cam_K, B, dev)
    ids, (vmax,) = scene.mesh_ids_on(mesh_ids, B, dev, meshes.sizes)
    gt = scene.pack_poses(R_gt, t_gt, B, dev)
    if size is None:
        raise ValueError("size=(width, height) is required: a MeshSet has no frame")
    W, H = scene.frame_size(size)
    verts, v_off = meshes.on(dev)
    faces, f_off, diam = meshes.faces_on(dev)
    out = {k: torch.empty(B, dtype=torch.float64, device=dev) for n, k in enumerate(MASK_KINDS) if mask >> n & 1}
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev) if return_counts else None
    ok = torch.empty(B, dtype=torch.uint8, device=dev) if return_counts else None
    boxes = torch.empty((B, 2, 4), dtype=torch.int32, device=dev) if return_boxes else None
    masks = torch.empty((B, 2, H, W), dtype=torch.uint8, device=dev) if return_masks else None
    scratch = torch.empty(_abi.load().cp_mask_errors_scratch_bytes(B, vmax), dtype=torch.uint8, device=dev)
    _abi.call("cp_mask_errors", dev, est, gt, K, k_stride, verts, v_off, faces, f_off, len(meshes), ids, diam, H, W, 1 if sphere_check else 0,
              B, vmax, out.get("cus"), out.get("cou_bb_proj"), counts, boxes, ok, masks, scratch)
    if return_counts:
        out["counts"], out["ok"] = counts, ok.view(torch.bool)
    if return_boxes:
        out["boxes"] = boxes
    if return_masks:
        out["masks"] = masks.view(torch.bool)
    return out


def _as_masks(m, dev=None):
    m = torch.as_tensor(m)
    if dev is not None:
        m = m.to(dev)
    if m.dim() == 2:
        m = m[None]
    if m.dim() != 3:
        raise ValueError("masks must be (H,W) or (B,H,W), got %r" % (tuple(m.shape),))
    if m.dtype == torch.bool:
        return m.contiguous().view(torch.uint8)
    if m.dtype == torch.uint8:
        return m.contiguous()
    return (m != 0).view(torch.uint8)                         # astype(bool) of any other type


def mask_overlap(mask_est, mask_gt, kinds=("cou_mask", "cou_bb"), return_counts=False, return_boxes=False):
    """pose_error.cou_mask of B mask pairs and / or cou_bb of the masks' bounding boxes, on the device in ONE launch (cp_mask_overlap).
      mask_est, mask_gt: (B,H,W) (or (H,W)) CUDA tensors, bool or uint8 (any other dtype is compared with 0 first): nonzero = set,
      as the reference's astype(bool) -- e.g. the network's predicted segmentation against mask_visib.
    cou_mask = 1 - inter / union, 1.0 when the union is empty;  cou_bb = 1 - iou of the boxes (xmin, ymin, xmax - xmin, ymax - ymin)
    of the two masks, NaN where a mask is empty (misc.calc_2d_bbox raises there).
    -> dict kind -> (B,) float64 CUDA tensor (+ "counts": (B,4) int32 = inter, union, n_est, n_gt; + "boxes": (B,2,4) int32, -1 where empty)"""
    mask = scene.kinds_mask(kinds, OVERLAP_KINDS, None if return_counts or return_boxes else
                            "kinds is empty: ask for \"cou_mask\", \"cou_bb\" or both")
    scene.require_cuda("metric", mask_est)
    dev = mask_est.device
    me, mg = _as_masks(mask_est), _as_masks(mask_gt, dev)
    if me.shape != mg.shape:
        raise ValueError("mask_est is %r, mask_gt %r" % (tuple(me.shape), tuple(mg.shape)))
    B, H, W = (int(v) for v in me.shape)
    if B == 0 or H == 0 or W == 0:
        raise ValueError("no masks")
    out = {k: torch.empty(B, dtype=torch.float64, device=dev) for n, k in enumerate(OVERLAP_KINDS) if mask >> n & 1}
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev) if return_counts else None
    boxes = torch.empty((B, 2, 4), dtype=torch.int32, device=dev) if return_boxes else None
    _abi.call("cp_mask_overlap", dev, me, mg, H, W, B, out.get("cou_mask"), out.get("cou_bb"), counts, boxes)
    if return_counts:
        out["counts"] = counts
    if return_boxes:
        out["boxes"] = boxes
    return out


def box_overlap(bb_est, bb_gt):
    """pose_error.cou_bb = 1 - misc.iou of B box pairs (x, y, w, h), on the device (cp_box_overlap): bb_est (B,4) CUDA tensor (any
    real dtype; computed in float64), bb_gt the same shape (tensor or host array).  -> (B,) float64 CUDA tensor"""
    scene.require_cuda("metric", bb_est)
    dev = bb_est.device
    a = bb_est.reshape(-1, 4).to(torch.float64).contiguous()
    c = torch.as_tensor(bb_gt).to(device=dev, dtype=torch.float64).reshape(-1, 4).contiguous()
    if a.shape != c.shape or a.shape[0] == 0:
        raise ValueError("bb_est and bb_gt must both be (B,4), B > 0")
    B = int(a.shape[0])
    out = torch.empty(B, dtype=torch.float64, device=dev)
    _abi.call("cp_box_overlap", dev, a, c, B, out)
    return out


def cou_mask(mask_est, mask_gt, device="cuda:0"):
    """bop_toolkit_lib.pose_error.cou_mask (two hxw arrays -> float), counted on the device"""
    dev = scene.cuda_device("metric", device)
    f = lambda m: torch.from_numpy(np.ascontiguousarray(np.asarray(m).astype(bool))).to(dev)   # noqa: E731
    return float(mask_overlap(f(mask_est), f(mask_gt), kinds=("cou_mask",))["cou_mask"][0])


def cou_bb(bb_est, bb_gt, device="cuda:0"):
    """bop_toolkit_lib.pose_error.cou_bb (two boxes x, y, w, h -> float), on the device"""
    dev = scene.cuda_device("metric", device)
    f = lambda b: torch.from_numpy(np.asarray(b, dtype=np.float64).reshape(1, 4)).to(dev)   # noqa: E731
    return float(box_overlap(f(bb_est), f(bb_gt))[0])


def _one_mask_error(kind, R_est, t_est, R_gt, t_gt, K, renderer, obj_id, size, device):
    dev = scene.cuda_device("metric", device)
    if not isinstance(renderer, MeshSet) or renderer.faces is None:
        raise ValueError("renderer must be a MeshSet built with faces")
    if size is None:
        raise ValueError("size=(width, height) is required: a MeshSet has no frame")
    m = int(obj_id)
    if not 0 <= m < len(renderer):
        raise ValueError("obj_id must be a mesh index in 0..%d" % (len(renderer) - 1))
    out = mask_errors(*scene.upload_pose(R_est, t_est, dev), *scene.upload_pose(R_gt, t_gt, dev),
                      np.asarray(K, dtype=np.float64).reshape(3, 3), renderer, size, mesh_ids=None if len(renderer) == 1 else [m],
                      kinds=(kind,))
    return float(out[kind][0])


def cus(R_est, t_est, R_gt, t_gt, K, renderer, obj_id, size=None, device="cuda:0"):
    """bop_toolkit_lib.pose_error.cus (numpy arrays of one pose -> float), rendered and counted on the device.  `renderer` is a
    MeshSet with faces and `obj_id` the index of the object's mesh in it; size=(W, H) is required, because a MeshSet has no frame.
    No sphere shortcut: that is the caller's."""
    return _one_mask_error("cus", R_est, t_est, R_gt, t_gt, K, renderer, obj_id, size, device)


def cou_bb_proj(R_est, t_est, R_gt, t_gt, K, renderer, obj_id, size=None, device="cuda:0"):
    """bop_toolkit_lib.pose_error.cou_bb_proj, with cus' arguments.  NaN where the reference raises (a silhouette with no pixel)."""
    return _one_mask_error("cou_bb_proj", R_est, t_est, R_gt, t_gt, K, renderer, obj_id, size, device)
