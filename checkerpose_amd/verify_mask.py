"""Poses verified against the network's own predicted masks on the device (csrc/pose_verify_mask.hip).

Row N26 (postprocess.verify_poses) needs the sensor's depth; CheckerPose is an RGB method and BOP's RGB track forbids depth.  Here a
candidate pose's rendered silhouette is compared with a packed mask -- coco_eval.PackedMasks bit rows, as paste_masks (row N27) leaves
the network's `seg` output: channel 1 the full (amodal) mask, what a render of the object alone should look like, channel 0 the visible
one -- inside the raster tile: no depth frame and no dense mask exists, the outputs are integer counts.  verify_poses_mask scores poses,
estimate_poses_mask_verified is postprocess.estimate_poses that keeps per crop the stage's pose the masks of its ONE forward support
best; the choice is postprocess.select_poses, unchanged.  Both are reached as postprocess.verify_poses_mask and
postprocess.estimate_poses_mask_verified.  The rule is the project's own (the reference never verifies), stated at the top of the kernel
file and restated in numpy by tests/verify_mask_stages.py.  No CPU fallback: CPU tensors raise."""
import numpy as np
import torch

from . import _abi

VERIFY_MASK_MAX_PIXELS = 1 << 24                    # csrc/pose_verify_mask.hip: the sums are int32, as cp_verify_poses'
VERIFY_MASK_COUNTS = ("n_model", "n_inter", "n_vis_in", "n_mask", "n_vis")
VERIFY_MASK_LABELS = {"model": 1, "full": 2, "visible": 4}        # the label map's bits


def _check_packed(masks, name):
    from . import coco_eval
    if not isinstance(masks, coco_eval.PackedMasks):
        raise ValueError("%s must be a coco_eval.PackedMasks (paste_masks, pack_masks), got %r" % (name, type(masks).__name__))
    N, H, W = len(masks), int(masks.H), int(masks.W)
    if not (torch.is_tensor(masks.bits) and torch.is_tensor(masks.area)) or masks.bits.dtype != torch.int32 or masks.area.dtype != torch.int32 \
            or tuple(masks.bits.shape) != (N, H, (W + 31) // 32) or tuple(masks.area.shape) != (N,):
        raise ValueError("%s: bits must be (N,H,ceil(W/32)) int32 and area (N,) int32" % name)
    return N, H, W


def verify_poses_mask(R, t, cam_K, meshes, full, visible=None, mask_ids=None, mesh_ids=None, status=None, return_labels=False):
    """Hypothesis verification of poses against predicted masks on the device (row N28; opt-in -- the reference does not verify): each
    pose is rendered and its silhouette compared with its mask inside one tile kernel -- no depth frame and no dense mask is stored.
    The rule is this project's own (csrc/pose_verify_mask.hip states it, tests/verify_mask_stages.py restates it).  With D the pose's
    render (metric.render_depth's bits) over the masks' frame, a pixel with D > 0 is a model pixel;
      n_model = |D > 0|, n_inter = |model and full|, n_vis_in = |model and visible|, n_mask = full.area[m], n_vis = visible.area[m]
      (the areas are read, not recounted); iou = n_inter / (n_model + n_mask - n_inter), cover = n_vis_in / n_vis, score = iou.
    cover is reported and not folded into the score: how to combine the two stays the caller's choice.
      R (P,3,3), t (P,3,1) / (P,3): CUDA/HIP tensors; cam_K (3,3) / (P,3,3); meshes: a MeshSet with faces; full: the
      coco_eval.PackedMasks of the full (amodal) masks -- paste_masks(seg, ..., channel=1) --, H W <= 2^24; visible: None, or the
      PackedMasks of the visible masks (channel=0), of full's frame size and length; mask_ids (P,) or None: each pose's mask row (None
      needs len(full) == P: pose p reads mask p); mesh_ids (P,) with several meshes; status (P,) or None: a pose whose entry is 0 (the
      solvers' identity fallback) is no candidate.
    -> (score (P,) f64, info[, labels (P,H,W) uint8: model | full << 1 | visible << 2 per pixel])
       info: dict of device tensors -- n_model, n_inter, n_vis_in, n_mask, n_vis (P,) int32; box (P,4) int32 xmin ymin xmax ymax of the
       silhouette, -1s when n_model == 0; ok (P,) bool; iou, cover (P,) f64.  score and iou are NaN with ok False when the union is 0 or
       the pose is not counted (its sums 0, its box -1s): a non-finite pose or cam_K, a vertex at Z <= 0, a mesh id out of range, a mask
       id outside 0..len(full)-1, status 0.  cover is NaN when n_vis == 0, without `visible`, or when the pose is not counted.  An empty
       full mask under a non-empty render scores exactly 0 with ok True.  A pose that is not counted still gets its mask bits in the
       labels.  Every output is a function of integer sums: bitwise the same for a pose alone or in a batch, with or without labels."""
    from . import scene
    n_masks, H, W = _check_packed(full, "full")
    if visible is not None and _check_packed(visible, "visible") != (n_masks, H, W):
        raise ValueError("visible must hold as many masks of the same frame size as full (%d of %d x %d)" % (n_masks, H, W))
    if n_masks < 1:
        raise ValueError("full holds no masks")
    if H * W > VERIFY_MASK_MAX_PIXELS:
        raise ValueError("masks: H * W must be <= 2^24 for cp_verify_poses_mask (its sums are int32), got %d x %d" % (H, W))
    dev, poses, P = scene.mesh_poses(R, t, meshes)
    scene.require_cuda("verify_mask", full.bits, full.area, *([visible.bits, visible.area] if visible is not None else []))
    if status is not None and (not torch.is_tensor(status) or tuple(status.shape) != (P,)):
        raise ValueError("status must be a (P,) tensor or None")
    if status is not None:
        scene.require_cuda("verify_mask", status)
    if mask_ids is None:
        if n_masks != P:
            raise ValueError("%d masks for %d poses need mask_ids" % (n_masks, P))
        m_ids = None
    elif torch.is_tensor(mask_ids) and mask_ids.is_cuda:              # resident ids stay there unread: an id outside 0..N-1 scores NaN
        if mask_ids.numel() != P:
            raise ValueError("mask_ids must be (P,)")
        m_ids = mask_ids.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    else:                                                           # host ids are checked
        host = np.asarray(mask_ids).reshape(-1).astype(np.int64)
        if host.shape[0] != P or host.min() < 0 or host.max() >= n_masks:
            raise ValueError("mask_ids must be (P,) with values in 0..%d" % (n_masks - 1))
        m_ids = torch.from_numpy(host.astype(np.int32)).to(dev)
    K, k_stride = scene.camera(cam_K, P, dev, "P")
    ids, (vmax,) = scene.mesh_ids_on(mesh_ids, P, dev, meshes.sizes)
    verts, v_off = meshes.on(dev)
    faces, f_off, _ = meshes.faces_on(dev)
    st_in = None if status is None else status.to(device=dev, dtype=torch.int32).contiguous()
    f_bits, f_area = full.bits.to(dev).contiguous(), full.area.to(dev).contiguous()
    v_bits, v_area = (None, None) if visible is None else (visible.bits.to(dev).contiguous(), visible.area.to(dev).contiguous())
    counts = torch.empty((P, len(VERIFY_MASK_COUNTS)), dtype=torch.int32, device=dev)
    box = torch.empty((P, 4), dtype=torch.int32, device=dev)
    score, iou, cover = (torch.empty((P,), dtype=torch.float64, device=dev) for _ in range(3))
    ok = torch.empty((P,), dtype=torch.uint8, device=dev)
    labels = torch.empty((P, H, W), dtype=torch.uint8, device=dev) if return_labels else None
    scratch = torch.empty(_abi.load().cp_verify_poses_mask_scratch_bytes(P, vmax), dtype=torch.uint8, device=dev)
    _abi.call("cp_verify_poses_mask", dev, poses, K, k_stride, verts, v_off, faces, f_off, len(meshes), ids, f_bits, f_area, v_bits, v_area,
              m_ids, n_masks, H, W, st_in, P, vmax, counts, box, score, iou, cover, ok, labels, scratch)
    info = {k: counts[:, i] for i, k in enumerate(VERIFY_MASK_COUNTS)}
    info.update(box=box, ok=ok.bool(), iou=iou, cover=cover)
    return (score, info, labels) if return_labels else (score, info)


def _check_verify_mask(verify):
    """estimate_poses_mask_verified's `verify` argument: a dict with meshes (optionally mesh_ids and use_visible)"""
    if not isinstance(verify, dict) or "meshes" not in verify:
        raise ValueError("verify must be dict(meshes=...[, mesh_ids=..., use_visible=...])")
    if "image_ids" in verify or "status" in verify or "mask_ids" in verify:
        raise ValueError("verify must not name image_ids, status or mask_ids: the masks are the crops' own and the status is the solver's")
    extra = [k for k in verify if k not in ("meshes", "mesh_ids", "use_visible")]
    if extra:
        raise ValueError("verify: unknown key(s) %r" % (extra,))


def estimate_poses_mask_verified(net, frames, Bboxes, p3d_xyz, cam_K, verify, return_verify=False, **estimate_kwargs):
    """estimate_poses with hypothesis verification against the network's own masks (row N28; RGB-only, where estimate_poses_verified
    needs depth): the same call (estimate_kwargs are estimate_poses' keywords) with ONE forward, whose `seg` output goes through
    paste_masks -- channel 1, the full mask, and channel 0, the visible one, unless use_visible is False -- with the crops' own padded
    boxes and resize_method; the poses after each stage the call runs (the solver's, then after "lm", then after "icp": 1, 2 or 3
    candidates per crop, candidate-major, crop b's mask for each of its candidates) are scored by ONE verify_poses_mask and ONE
    select_poses keeps per crop the one its predicted mask supports.
      verify: a dict with `meshes` (a MeshSet with faces, in the units of p3d_xyz) and optionally `mesh_ids` and `use_visible` (default
      True: the visible masks are pasted too and `cover` is reported; it never changes the score); `image_ids`, `status` and `mask_ids`
      are refused.  resize_method="crop_resize_by_warp_affine" raises paste_masks' NotImplementedError.
    -> (R, t, inliers, status, final boxes) as estimate_poses: R, t the chosen candidates' (their bits), inliers and status still the
       solver's; return_verify=True appends a dict: score (C,B), choice (B,) int32, stages (a tuple of "solver" / "lm" / "icp"), info
       (verify_poses_mask's dict over the C * B poses, candidate-major), full and visible (the pasted PackedMasks; visible None
       without use_visible)."""
    from . import paste, postprocess
    _check_verify_mask(verify)
    method = estimate_kwargs.get("resize_method", "crop_square_resize")
    paste._check_paste_method(method)
    keep = {}
    stages, inl, status, final = postprocess._estimate_stages(net, frames, Bboxes, p3d_xyz, cam_K, keep=keep, **estimate_kwargs)
    H, W = (int(v) for v in frames.shape[-3:-1])
    full = postprocess.paste_masks(keep["seg"], keep["padded"], (H, W), method, 1)
    visible = postprocess.paste_masks(keep["seg"], keep["padded"], (H, W), method, 0) if verify.get("use_visible", True) else None
    C_, B = len(stages), int(stages[0][1].shape[0])
    Rc = torch.stack([r.reshape(B, 3, 3) for _, r, _ in stages])
    tc = torch.stack([x.reshape(B, 3, 1) for _, _, x in stages])
    K = cam_K if torch.is_tensor(cam_K) else np.asarray(cam_K)
    if K.ndim == 3:
        K = K.repeat(C_, 1, 1) if torch.is_tensor(K) else np.tile(K, (C_, 1, 1))
    mesh_ids = verify.get("mesh_ids")
    if mesh_ids is not None:
        mesh_ids = mesh_ids.reshape(-1).repeat(C_) if torch.is_tensor(mesh_ids) else np.tile(np.asarray(mesh_ids).reshape(-1), C_)
    score, info = postprocess.verify_poses_mask(Rc.reshape(C_ * B, 3, 3), tc.reshape(C_ * B, 3, 1), K, verify["meshes"], full, visible=visible,
                                                mask_ids=np.tile(np.arange(B), C_), mesh_ids=mesh_ids, status=status.reshape(-1).repeat(C_))
    score = score.view(C_, B)
    choice, R, t = postprocess.select_poses(score, info["ok"].view(C_, B), Rc, tc)
    if not return_verify:
        return R, t, inl, status, final
    return R, t, inl, status, final, dict(score=score, choice=choice, stages=tuple(n for n, _, _ in stages), info=info, full=full, visible=visible)
