"""Poses refined against the network's own predicted masks on the device (csrc/mask_refine.hip).

Rows N24 - N26 refine and verify against the sensor's depth; CheckerPose is an RGB method and BOP's RGB track forbids depth.  An RGB-only
pose is weakest along the viewing ray: the keypoints' p2d sit on a 64-cell RoI grid and EPnP / row N22 minimise over those alone.  The
extent of the predicted mask fixes the scale of the projection, and so the depth.  Here the contour of a pose's render (ONE raster pass
at the input pose: the first / last covered pixel of lattice rows, the topmost / bottommost of lattice columns) is pulled onto the
extents of a packed mask -- coco_eval.PackedMasks bit rows, as paste_masks (row N27) leaves the full (amodal) mask, channel 1 -- by a
Levenberg-Marquardt iteration over translation alone (dof="t") or rotation and translation (dof="rt").  mask_extents and
contour_samples are the two operands, refine_poses_mask the refinement, estimate_poses_mask_refined is postprocess.estimate_poses that
offers the refined pose as one more candidate ("sil") to row N28's verification, which can discard a refinement that made the pose
worse.  All four are reached through postprocess.  The rule is the project's own (the reference never refines), stated at the top of the
kernel file and restated in numpy by tests/mask_refine_stages.py.  Nothing has been measured on the network's own masks, which are
pasted from 64 x 64 cells.  No CPU fallback: CPU tensors raise."""
import numpy as np
import torch

from . import _abi
from .verify_mask import _check_packed, _check_verify_mask

MASK_REFINE_MAX_ITERS, MASK_REFINE_GRID_MAX, MASK_REFINE_RECORD, MASK_REFINE_INFO = 64, 64, 18, 42        # csrc/mask_refine.hip
MASK_REFINE_DOF = {"t": 0, "rt": 1}
_CONTOUR_KEYS = ("rect", "shape", "pixel", "depth", "X", "ok")


def _check_grid(grid):
    grid = int(grid)
    if not 1 <= grid <= MASK_REFINE_GRID_MAX:
        raise ValueError("grid must be in 1..%d, got %r" % (MASK_REFINE_GRID_MAX, grid))
    return grid


def mask_extents(masks):
    """Per mask of a coco_eval.PackedMasks on the device: row (N,H,2) int32 = (first, last) set column of every row, col (N,W,2) int32 =
    (first, last) set row of every column, (-1, -1) where there is none (cp_mask_extents: one launch, integer only).
    -> dict(row, col)"""
    from . import scene
    N, H, W = _check_packed(masks, "masks")
    if N < 1:
        raise ValueError("masks holds no masks")
    scene.require_cuda("refine_mask", masks.bits)
    dev = masks.bits.device
    bits = masks.bits.contiguous()
    row = torch.empty((N, H, 2), dtype=torch.int32, device=dev)
    col = torch.empty((N, W, 2), dtype=torch.int32, device=dev)
    _abi.call("cp_mask_extents", dev, bits, N, H, W, row, col)
    return dict(row=row, col=col)


def contour_samples(R, t, cam_K, meshes, size, mesh_ids=None, grid=32):
    """Stage A of refine_poses_mask (row N30) on its own: ONE raster pass of the P poses of `meshes` (a MeshSet with faces) on a frame of
    size = (width, height), then per pose the contour pixels on row N24's lattice lines (csrc/mask_refine.hip states the rule).
    S = 4 * grid slots per pose: slot 2 j / 2 j + 1 the first / last covered pixel of lattice row j, slot 2 grid + 2 i / + 1 the topmost /
    bottommost covered pixel of lattice column i.  -> dict of device tensors:
      rect (P,4) int32 x0 y0 x1 y1 (-1 four times when empty); shape (P,2) int32 nx ny; pixel (P,S,2) int32 (-1 -1 = empty slot: no
      covered pixel on its line, or the pixel lies on the frame's border); depth (P,S) f32: metric.render_depth's value at the pixel (0
      in an empty slot); X (P,S,3) f64 the model-space point (NaN in an empty slot); ok (P,) int32: 0 where the pose was not rendered
      (a non-finite entry, a vertex at Z <= 0, a mesh id out of range)."""
    from . import scene
    grid = _check_grid(grid)
    dev, poses, P = scene.mesh_poses(R, t, meshes)
    K, k_stride = scene.camera(cam_K, P, dev, "P")
    ids, (vmax,) = scene.mesh_ids_on(mesh_ids, P, dev, meshes.sizes)
    W, H = scene.frame_size(size)
    verts, v_off = meshes.on(dev)
    faces, f_off, _ = meshes.faces_on(dev)
    S = 4 * grid
    out = dict(rect=torch.empty((P, 4), dtype=torch.int32, device=dev), shape=torch.empty((P, 2), dtype=torch.int32, device=dev),
               pixel=torch.empty((P, S, 2), dtype=torch.int32, device=dev), depth=torch.empty((P, S), dtype=torch.float32, device=dev),
               X=torch.empty((P, S, 3), dtype=torch.float64, device=dev), ok=torch.empty((P,), dtype=torch.int32, device=dev))
    scratch = torch.empty(_abi.load().cp_contour_samples_scratch_bytes(P, vmax, grid), dtype=torch.uint8, device=dev)
    _abi.call("cp_contour_samples", dev, poses, K, k_stride, verts, v_off, faces, f_off, len(meshes), ids, H, W, P, vmax, grid,
              *[out[k] for k in _CONTOUR_KEYS], scratch)
    return out


def refine_poses_mask(R, t, cam_K, meshes, full, max_dist, dof, mask_ids=None, mesh_ids=None, status=None, grid=32, max_iters=20, step_tol=1e-6,
                      min_pairs=6, return_records=False):
    """Silhouette refinement of poses against predicted masks on the device (row N30; opt-in -- the reference does not refine): what a
    user WITHOUT depth runs after an RGB-only estimate, whose error is largest along the viewing ray.  The rule is this project's own
    (csrc/mask_refine.hip states it, tests/mask_refine_stages.py restates it): contour samples of each mesh rendered ONCE at the input
    pose (contour_samples), re-associated after every accepted step with the mask's extent on the row (column) they project to, one
    axis-aligned residual per sample, Levenberg-Marquardt in row N22's form.
      R (P,3,3), t (P,3,1) / (P,3): the poses to start from (CUDA/HIP tensors); cam_K (3,3) / (P,3,3); meshes: a MeshSet with faces; full:
      the coco_eval.PackedMasks of the full (amodal) masks -- paste_masks(seg, ..., channel=1); mask_ids (P,) or None: each pose's mask
      row (None needs len(full) == P: pose p reads mask p); mesh_ids (P,) with several meshes; status (P,) or None: poses whose entry
      is 0 are left alone.
      max_dist: a number or a (P,) tensor in PIXELS, NO default: a sample farther than this from its mask extent is dropped.  About a
      twelfth of the frame's width worked in the restatement's experiment (8 px on 96 x 80, 24 px on 288 x 240); it is the caller's choice.
      dof: "t" or "rt", NO default: "t" moves the translation only and returns R bitwise; "rt" moves the rotation too.  On an object some
      30 px across three degrees move the contour by less than a pixel and the rotation drifts: prefer "t" there.
      grid in 1..64: lattice lines per axis; max_iters in 1..64; step_tol > 0; min_pairs >= 6.
    Masks clipped by their crop window, occlusion and symmetry are not handled: the full mask is taken as the object's silhouette.
    -> (R (P,3,3) f64, t (P,3,1) f64, refine_status (P,) int32, info[, records])
       refine_status: 1 = an accepted step below step_tol, 2 = max_iters ran out, 3 = lambda passed 1e8 or fewer than min_pairs pairs
       were left after a step, 0 = pass-through (the input pose, bitwise: status 0 given, a non-finite pose or cam_K, a pose that is not
       rendered, a mask id outside 0..len(full)-1, fewer than min_pairs pairs under the input pose);
       info: dict of device tensors -- cost0, cost (P,) f64: sums of squared pixel residuals at the input / returned pose; n_samples,
       n0, n (P,) int64: samples, pairs at the input pose, pairs at the returned pose; iters (P,) int64; H (P,6,6) f64: the undamped
       J^T J at the returned pose over its pairs (rotation then translation); status = refine_status; samples: contour_samples' dict;
       extents: mask_extents' dict.  Pass-through rows hold NaN in cost0, cost and H.
       records (return_records=True): (P, max_iters, 18) f64, [lambda, n, c, c', accepted, s, R' (9), t' (3)] per executed iteration,
       NaN where none ran."""
    from . import scene
    if dof not in MASK_REFINE_DOF:
        raise ValueError('dof must be "t" or "rt", got %r' % (dof,))
    max_iters, min_pairs, step_tol = int(max_iters), int(min_pairs), float(step_tol)
    if not 1 <= max_iters <= MASK_REFINE_MAX_ITERS:
        raise ValueError("max_iters must be in 1..%d for cp_mask_refine, got %r" % (MASK_REFINE_MAX_ITERS, max_iters))
    if not 0.0 < step_tol < float("inf"):
        raise ValueError("step_tol must be a finite number > 0, got %r" % (step_tol,))
    if min_pairs < 6:
        raise ValueError("min_pairs must be >= 6, got %r" % (min_pairs,))
    grid = _check_grid(grid)
    n_masks, H, W = _check_packed(full, "full")
    if n_masks < 1:
        raise ValueError("full holds no masks")
    if not torch.is_tensor(max_dist) and not 0.0 < float(max_dist) < float("inf"):
        raise ValueError("max_dist must be a finite number > 0 (in pixels), got %r" % (max_dist,))
    dev, poses, P = scene.mesh_poses(R, t, meshes)
    scene.require_cuda("refine_mask", full.bits, full.area)
    if torch.is_tensor(max_dist):
        scene.require_cuda("refine_mask", max_dist)
        if max_dist.numel() != P:
            raise ValueError("max_dist must be a number or a (P,) tensor")
        md = max_dist.reshape(P).to(device=dev, dtype=torch.float64).contiguous()
    else:
        md = torch.full((P,), float(max_dist), dtype=torch.float64, device=dev)
    if status is not None and (not torch.is_tensor(status) or tuple(status.shape) != (P,)):
        raise ValueError("status must be a (P,) tensor or None")
    if status is not None:
        scene.require_cuda("refine_mask", status)
    if mask_ids is None:
        if n_masks != P:
            raise ValueError("%d masks for %d poses need mask_ids" % (n_masks, P))
        m_ids = None
    elif torch.is_tensor(mask_ids) and mask_ids.is_cuda:              # resident ids stay there unread: an id outside 0..N-1 passes through
        if mask_ids.numel() != P:
            raise ValueError("mask_ids must be (P,)")
        m_ids = mask_ids.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    else:                                                           # host ids are checked
        host = np.asarray(mask_ids).reshape(-1).astype(np.int64)
        if host.shape[0] != P or host.min() < 0 or host.max() >= n_masks:
            raise ValueError("mask_ids must be (P,) with values in 0..%d" % (n_masks - 1))
        m_ids = torch.from_numpy(host.astype(np.int32)).to(dev)
    K, k_stride = scene.camera(cam_K, P, dev, "P")
    extents = mask_extents(full)
    samples = contour_samples(R, t, cam_K, meshes, (W, H), mesh_ids=mesh_ids, grid=grid)
    st_in = None if status is None else status.to(device=dev, dtype=torch.int32).contiguous()
    pose = torch.empty(P, 12, dtype=torch.float64, device=dev)
    rstatus = torch.empty(P, dtype=torch.int32, device=dev)
    info = torch.empty(P, MASK_REFINE_INFO, dtype=torch.float64, device=dev)
    rec = torch.full((P, max_iters, MASK_REFINE_RECORD), float("nan"), dtype=torch.float64, device=dev) if return_records else None
    _abi.call("cp_mask_refine", dev, poses, K, k_stride, samples["X"], samples["pixel"], samples["ok"], grid, extents["row"], extents["col"], m_ids,
              n_masks, H, W, md, st_in, MASK_REFINE_DOF[dof], max_iters, step_tol, min_pairs, P, pose, rstatus, info, rec)
    out_info = dict(cost0=info[:, 0], cost=info[:, 1], n_samples=info[:, 2].long(), n0=info[:, 3].long(), n=info[:, 4].long(),
                    iters=info[:, 5].long(), H=info[:, 6:].view(P, 6, 6), status=rstatus, samples=samples, extents=extents)
    out = (pose[:, :9].view(P, 3, 3), pose[:, 9:].view(P, 3, 1), rstatus, out_info)
    if return_records:
        out += (rec,)
    return out


def _check_refine_mask(refine_mask):
    """estimate_poses_mask_refined's `refine_mask` argument: a dict with max_dist and dof (optionally grid, max_iters, step_tol, min_pairs)"""
    if not isinstance(refine_mask, dict) or "max_dist" not in refine_mask or "dof" not in refine_mask:
        raise ValueError("refine_mask must be dict(max_dist=..., dof=...[, grid=..., max_iters=..., step_tol=..., min_pairs=...])")
    extra = [k for k in refine_mask if k not in ("max_dist", "dof", "grid", "max_iters", "step_tol", "min_pairs")]
    if extra:
        raise ValueError("refine_mask: unknown key(s) %r (the meshes are verify's, the masks the crops' own, the status the solver's)" % (extra,))


def estimate_poses_mask_refined(net, frames, Bboxes, p3d_xyz, cam_K, refine_mask, verify, return_verify=False, **estimate_kwargs):
    """estimate_poses_mask_verified with one more candidate (row N30; RGB-only): the same call (estimate_kwargs are estimate_poses'
    keywords) with ONE forward, whose `seg` output goes through paste_masks as there; the pose after the LAST stage the call runs goes
    through refine_poses_mask against the crops' full masks and is appended as the candidate "sil"; ONE verify_poses_mask scores all
    candidates and ONE select_poses keeps per crop the one its predicted mask supports -- so a refinement that made the pose worse is
    discarded.  A crop whose refinement passed through (refine status 0) offers no "sil" candidate: the result is then
    estimate_poses_mask_verified's.
      refine_mask: a dict with `max_dist` and `dof` (refine_poses_mask's, no defaults) and optionally `grid`, `max_iters`, `step_tol`,
      `min_pairs`; verify: estimate_poses_mask_verified's dict (`meshes`, optionally `mesh_ids` and `use_visible`).
    -> (R, t, inliers, status, final boxes) as estimate_poses; return_verify=True appends estimate_poses_mask_verified's dict, its
       stages ending with "sil", plus refine = (refine_status, info) of refine_poses_mask."""
    from . import paste, postprocess
    _check_refine_mask(refine_mask)
    _check_verify_mask(verify)
    method = estimate_kwargs.get("resize_method", "crop_square_resize")
    paste._check_paste_method(method)
    keep = {}
    stages, inl, status, final = postprocess._estimate_stages(net, frames, Bboxes, p3d_xyz, cam_K, keep=keep, **estimate_kwargs)
    H, W = (int(v) for v in frames.shape[-3:-1])
    full = postprocess.paste_masks(keep["seg"], keep["padded"], (H, W), method, 1)
    visible = postprocess.paste_masks(keep["seg"], keep["padded"], (H, W), method, 0) if verify.get("use_visible", True) else None
    B = int(stages[0][1].shape[0])
    mesh_ids = verify.get("mesh_ids")
    _, R_last, t_last = stages[-1]
    Rs, ts, rstatus, rinfo = postprocess.refine_poses_mask(R_last.reshape(B, 3, 3), t_last.reshape(B, 3, 1), cam_K, verify["meshes"], full,
                                                           refine_mask["max_dist"], refine_mask["dof"], mesh_ids=mesh_ids, status=status.reshape(-1),
                                                           **{k: v for k, v in refine_mask.items() if k not in ("max_dist", "dof")})
    stages = list(stages) + [("sil", Rs, ts)]
    C_ = len(stages)
    Rc = torch.stack([r.reshape(B, 3, 3) for _, r, _ in stages])
    tc = torch.stack([x.reshape(B, 3, 1) for _, _, x in stages])
    K = cam_K if torch.is_tensor(cam_K) else np.asarray(cam_K)
    if K.ndim == 3:
        K = K.repeat(C_, 1, 1) if torch.is_tensor(K) else np.tile(K, (C_, 1, 1))
    if mesh_ids is not None:
        mesh_ids = mesh_ids.reshape(-1).repeat(C_) if torch.is_tensor(mesh_ids) else np.tile(np.asarray(mesh_ids).reshape(-1), C_)
    # a pass-through "sil" (refine status 0) is the last stage's pose over again: no candidate
    st = status.reshape(-1).to(torch.int32)
    cand_status = torch.cat([st.repeat(C_ - 1), torch.where(rstatus != 0, st, torch.zeros_like(st))])
    score, info = postprocess.verify_poses_mask(Rc.reshape(C_ * B, 3, 3), tc.reshape(C_ * B, 3, 1), K, verify["meshes"], full, visible=visible,
                                                mask_ids=np.tile(np.arange(B), C_), mesh_ids=mesh_ids, status=cand_status)
    score = score.view(C_, B)
    choice, R, t = postprocess.select_poses(score, info["ok"].view(C_, B), Rc, tc)
    if not return_verify:
        return R, t, inl, status, final
    return R, t, inl, status, final, dict(score=score, choice=choice, stages=tuple(n for n, _, _ in stages), info=info, full=full, visible=visible,
                                          refine=(rstatus, rinfo))
