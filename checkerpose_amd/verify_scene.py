"""The poses of an image verified together against the network's visible masks on the device (SURVEY.md 8f row N31;
csrc/scene_verify_mask.hip).

Row N28 (postprocess.verify_poses_mask) scores every pose as if its object stood alone: its `iou` compares the unoccluded silhouette
with the full mask, its `cover` the unoccluded silhouette with the visible mask.  Here the estimates of one image occlude each other --
the front-most composite and the BOP'19 visibility test of row N19 (render.render_scene) -- and what the scene predicts to be visible of
a pose is counted against the pose's visible mask (`seg` channel 0, as paste_masks leaves it) inside the raster tile: depth only, no
frame and no dense mask is stored.  verify_scene_mask scores poses, estimate_poses_scene_verified is postprocess.estimate_poses that
keeps per crop the stage's pose whose scene the masks of its ONE forward support best; the choice is postprocess.select_poses,
unchanged.  Both are reached as postprocess.verify_scene_mask and postprocess.estimate_poses_scene_verified.  The rule is the project's
own (the reference never verifies), stated at the top of the kernel file and restated in numpy by tests/scene_verify_stages.py.  It has
been exercised on rendered truth masks only: its behaviour on the network's own masks is not measured.  No CPU fallback: CPU tensors
raise."""
import math

import numpy as np
import torch

from . import _abi
from .verify_mask import _check_packed

VERIFY_SCENE_MAX_PIXELS = 1 << 24                   # csrc/scene_verify_mask.hip: the sums are int32, as cp_verify_poses_mask's
VERIFY_SCENE_MAX_POSES = 32                         # per image: one bit of the planes each
VERIFY_SCENE_COUNTS = ("n_model", "n_pvis", "n_inter", "n_vis_in", "n_pvis_in", "n_mask", "n_vis", "n_hidden_seen")


def verify_scene_mask(R, t, cam_K, meshes, full, visible, image_ids, delta, mask_ids=None, mesh_ids=None, status=None, n_images=None,
                      return_planes=False):
    """Hypothesis verification of the poses of an image TOGETHER against predicted masks on the device (row N31; opt-in -- the reference
    does not verify).  The rule is this project's own (csrc/scene_verify_mask.hip states it, tests/scene_verify_stages.py restates it).
    With D_p pose p's render (metric.render_depth's bits) over the masks' frame, a pixel with D_p > 0 is a model pixel of p; ren = the
    smallest positive D_p over the counted poses of p's image; a model pixel is PREDICTED VISIBLE where render_scene's 'bop19' test holds
    with ren as the sensor depth: f32(dist_p) - f32(dist_ren) <= delta (distances under pose p's cam_K).  Per pose
      n_model, n_pvis (predicted visible), n_inter = |model and full|, n_vis_in = |model and visible|, n_pvis_in = |pvis and visible|,
      n_mask = full.area[m], n_vis = visible.area[m] (read, not recounted), n_hidden_seen = n_vis_in - n_pvis_in (pixels the network
      sees of p that another estimate hides);
      iou = n_inter / (n_model + n_mask - n_inter), cover = n_vis_in / n_vis (verify_poses_mask's), iou_vis = n_pvis_in / (n_pvis + n_vis
      - n_pvis_in), visib_fract = n_pvis / n_model, score = iou_vis.  How to combine iou and iou_vis stays the caller's choice.
      R (P,3,3), t (P,3,1) / (P,3): CUDA/HIP tensors; cam_K (3,3) / (P,3,3); meshes: a MeshSet with faces; full, visible: the
      coco_eval.PackedMasks of the full and the visible masks -- paste_masks(seg, ..., channel=1) and channel=0 --, of one frame size and
      length, H W <= 2^24; image_ids (P,): each pose's image, required -- host ids are checked (values in 0..n_images-1, at most 32 poses
      per image: ValueError), resident ids stay on the device unread (n_images is then required; an id out of range and a pose beyond its
      image's 32nd slot are not counted); delta: a finite number >= 0 in the unit of the meshes and t, no default; mask_ids (P,) or None
      (None needs len(full) == P); mesh_ids (P,) with several meshes; status (P,) or None: a pose whose entry is 0 is not counted;
      n_images: I (default: the largest host image id + 1).
    The slot of a pose is its rank among the poses of its image in the order given, counted or not.
    -> (score (P,) f64, info[, planes]): info is a dict of device tensors -- VERIFY_SCENE_COUNTS (P,) int32; box, box_pvis (P,4) int32
       xmin ymin xmax ymax of the model / predicted-visible pixels, -1s without any; ok (P,) bool; slot (P,) int32; iou, cover, iou_vis,
       visib_fract (P,) f64.  A pose that is not counted (a non-finite pose or cam_K, a vertex at Z <= 0, a mesh, mask or image id out
       of range, status 0, a slot >= 32) occludes nothing: its sums are 0, its boxes -1s, ok False, its quotients NaN.  score and iou_vis
       are NaN with ok False also when their union is 0.  planes: dict(full_bits, visib_bits) int32 (I,H,W), bit s set where the pose
       at slot s has a model / predicted-visible pixel (render_scene's layout; render.scene_masks expands them).
       Every output is a function of integer sums and per-pixel values: bitwise the same for an image alone or in a batch, with or
       without planes."""
    from . import scene
    n_masks, H, W = _check_packed(full, "full")
    if _check_packed(visible, "visible") != (n_masks, H, W):
        raise ValueError("visible must hold as many masks of the same frame size as full (%d of %d x %d)" % (n_masks, H, W))
    if n_masks < 1:
        raise ValueError("full holds no masks")
    if H * W > VERIFY_SCENE_MAX_PIXELS:
        raise ValueError("masks: H * W must be <= 2^24 for cp_verify_scene_mask (its sums are int32), got %d x %d" % (H, W))
    if isinstance(delta, bool) or not isinstance(delta, (int, float, np.integer, np.floating)) or not math.isfinite(float(delta)) or float(delta) < 0:
        raise ValueError("delta must be a finite number >= 0 (the unit of the meshes and t; no default), got %r" % (delta,))
    if image_ids is None:
        raise ValueError("verify_scene_mask needs image_ids: each pose's image")
    dev, poses, P = scene.mesh_poses(R, t, meshes)
    scene.require_cuda("verify_scene", full.bits, full.area, visible.bits, visible.area)
    if status is not None and (not torch.is_tensor(status) or tuple(status.shape) != (P,)):
        raise ValueError("status must be a (P,) tensor or None")
    if status is not None:
        scene.require_cuda("verify_scene", status)
    if torch.is_tensor(image_ids) and image_ids.is_cuda:              # resident ids stay there unread
        if image_ids.numel() != P:
            raise ValueError("image_ids must be (P,)")
        if n_images is None:
            raise ValueError("resident image_ids are not read: give n_images")
        n_img = int(n_images)
        i_ids = image_ids.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    else:                                                           # host ids are checked
        host = np.asarray(image_ids.cpu() if torch.is_tensor(image_ids) else image_ids).reshape(-1).astype(np.int64)
        if host.shape[0] != P:
            raise ValueError("image_ids must be (P,)")
        n_img = int(n_images) if n_images is not None else int(host.max()) + 1
        if n_img <= 0 or host.min() < 0 or host.max() >= n_img:
            raise ValueError("image_ids must be (P,) with values in 0..n_images-1 (n_images = %d)" % n_img)
        per = np.bincount(host, minlength=n_img)
        if int(per.max()) > VERIFY_SCENE_MAX_POSES:
            raise ValueError("image_ids: image %d holds %d poses: at most %d per image" % (int(per.argmax()), int(per.max()), VERIFY_SCENE_MAX_POSES))
        i_ids = torch.from_numpy(host.astype(np.int32)).to(dev)
    if n_img <= 0:
        raise ValueError("n_images must be positive")
    if mask_ids is None:
        if n_masks != P:
            raise ValueError("%d masks for %d poses need mask_ids" % (n_masks, P))
        m_ids = None
    elif torch.is_tensor(mask_ids) and mask_ids.is_cuda:              # resident ids stay there unread: an id outside 0..N-1 is not counted
        if mask_ids.numel() != P:
            raise ValueError("mask_ids must be (P,)")
        m_ids = mask_ids.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    else:
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
    v_bits, v_area = visible.bits.to(dev).contiguous(), visible.area.to(dev).contiguous()
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)      # noqa: E731
    counts, boxes, slot = i32(P, len(VERIFY_SCENE_COUNTS)), i32(P, 2, 4), i32(P)
    score, iou, cover, iou_vis, fract = (torch.empty((P,), dtype=torch.float64, device=dev) for _ in range(5))
    ok = torch.empty((P,), dtype=torch.uint8, device=dev)
    pl_full, pl_visib = (i32(n_img, H, W), i32(n_img, H, W)) if return_planes else (None, None)
    scratch = torch.empty(_abi.load().cp_verify_scene_mask_scratch_bytes(P, vmax, n_img), dtype=torch.uint8, device=dev)
    _abi.call("cp_verify_scene_mask", dev, poses, K, k_stride, verts, v_off, faces, f_off, len(meshes), ids, f_bits, f_area, v_bits, v_area,
              m_ids, n_masks, H, W, i_ids, n_img, st_in, float(delta), P, vmax, counts, boxes, slot, score, iou, cover, iou_vis, fract, ok,
              pl_full, pl_visib, scratch)
    info = {k: counts[:, i] for i, k in enumerate(VERIFY_SCENE_COUNTS)}
    info.update(box=boxes[:, 0], box_pvis=boxes[:, 1], ok=ok.bool(), slot=slot, iou=iou, cover=cover, iou_vis=iou_vis, visib_fract=fract)
    return (score, info, dict(full_bits=pl_full, visib_bits=pl_visib)) if return_planes else (score, info)


def _check_verify_scene(verify):
    """estimate_poses_scene_verified's `verify` argument: a dict with meshes and delta (optionally mesh_ids)"""
    if not isinstance(verify, dict) or "meshes" not in verify or "delta" not in verify:
        raise ValueError("verify must be dict(meshes=..., delta=...[, mesh_ids=...])")
    if "image_ids" in verify or "status" in verify or "mask_ids" in verify:
        raise ValueError("verify must not name image_ids, status or mask_ids: the images are the call's img_index, the masks the crops' own "
                         "and the status is the solver's")
    extra = [k for k in verify if k not in ("meshes", "delta", "mesh_ids")]
    if extra:
        raise ValueError("verify: unknown key(s) %r" % (extra,))


def estimate_poses_scene_verified(net, frames, Bboxes, p3d_xyz, cam_K, verify, return_verify=False, **estimate_kwargs):
    """estimate_poses with scene-level hypothesis verification against the network's own masks (row N31; RGB-only): the same call
    (estimate_kwargs are estimate_poses' keywords) with ONE forward, whose `seg` output goes through paste_masks twice -- channel 1, the
    full masks, and channel 0, the visible ones -- as in estimate_poses_mask_verified.  The poses after each stage the call runs (the
    solver's, then after "lm", then after "icp": C = 1, 2 or 3 candidates per crop) are laid out candidate-major, and stage c of every
    crop forms scene c of its frame: image_ids = c * n_frames + img_index, n_images = C * n_frames, crop b's masks for each of its
    candidates.  ONE verify_scene_mask scores them and ONE select_poses on `score` (iou_vis) keeps per crop the stage whose scene its
    visible mask supports best: the choice is per crop, within scenes of equal stages; a joint search over mixed stages is not built.
      verify: a dict with `meshes` (a MeshSet with faces, in the units of p3d_xyz) and `delta` (verify_scene_mask's, no default), and
      optionally `mesh_ids`; `image_ids`, `status` and `mask_ids` are refused.  More than 32 crops of one frame raise ValueError.
      resize_method="crop_resize_by_warp_affine" raises paste_masks' NotImplementedError.
    -> (R, t, inliers, status, final boxes) as estimate_poses: R, t the chosen candidates' (their bits), inliers and status still the
       solver's; return_verify=True appends a dict: score (C,B), choice (B,) int32, stages (a tuple of "solver" / "lm" / "icp"), info
       (verify_scene_mask's dict over the C * B poses, candidate-major), image_ids (C * B,) as passed on, full and visible (the pasted
       PackedMasks).  With one crop per frame iou, cover and the counts they are made of are estimate_poses_mask_verified's bits."""
    from . import paste, postprocess
    _check_verify_scene(verify)
    method = estimate_kwargs.get("resize_method", "crop_square_resize")
    paste._check_paste_method(method)
    n_frames = 1 if frames.dim() == 3 else int(frames.shape[0])
    B = len(Bboxes)
    img_index = estimate_kwargs.get("img_index")
    if img_index is None:
        img = np.zeros(B, np.int64) if n_frames == 1 else np.arange(B, dtype=np.int64)      # get_roi_batch's default: crop b from frame b
    else:
        img = np.asarray(img_index.cpu() if torch.is_tensor(img_index) else img_index).reshape(-1).astype(np.int64)
    if img.shape[0] != B or (B and (img.min() < 0 or img.max() >= n_frames)):
        raise ValueError("img_index must be (B,) = (%d,) with values in 0..%d" % (B, n_frames - 1))
    if B and int(np.bincount(img, minlength=n_frames).max()) > VERIFY_SCENE_MAX_POSES:
        raise ValueError("frame %d holds %d crops: at most %d per frame can be verified as one scene"
                         % (int(np.bincount(img).argmax()), int(np.bincount(img).max()), VERIFY_SCENE_MAX_POSES))
    keep = {}
    stages, inl, status, final = postprocess._estimate_stages(net, frames, Bboxes, p3d_xyz, cam_K, keep=keep, **estimate_kwargs)
    H, W = (int(v) for v in frames.shape[-3:-1])
    full = postprocess.paste_masks(keep["seg"], keep["padded"], (H, W), method, 1)
    visible = postprocess.paste_masks(keep["seg"], keep["padded"], (H, W), method, 0)
    C_ = len(stages)
    Rc = torch.stack([r.reshape(B, 3, 3) for _, r, _ in stages])
    tc = torch.stack([x.reshape(B, 3, 1) for _, _, x in stages])
    K = cam_K if torch.is_tensor(cam_K) else np.asarray(cam_K)
    if K.ndim == 3:
        K = K.repeat(C_, 1, 1) if torch.is_tensor(K) else np.tile(K, (C_, 1, 1))
    mesh_ids = verify.get("mesh_ids")
    if mesh_ids is not None:
        mesh_ids = mesh_ids.reshape(-1).repeat(C_) if torch.is_tensor(mesh_ids) else np.tile(np.asarray(mesh_ids).reshape(-1), C_)
    image_ids = (np.arange(C_, dtype=np.int64)[:, None] * n_frames + img[None, :]).reshape(-1)
    score, info = postprocess.verify_scene_mask(Rc.reshape(C_ * B, 3, 3), tc.reshape(C_ * B, 3, 1), K, verify["meshes"], full, visible, image_ids,
                                                verify["delta"], mask_ids=np.tile(np.arange(B), C_), mesh_ids=mesh_ids,
                                                status=status.reshape(-1).repeat(C_), n_images=C_ * n_frames)
    score = score.view(C_, B)
    choice, R, t = postprocess.select_poses(score, info["ok"].view(C_, B), Rc, tc)
    if not return_verify:
        return R, t, inl, status, final
    return R, t, inl, status, final, dict(score=score, choice=choice, stages=tuple(n for n, _, _ in stages), info=info, image_ids=image_ids,
                                          full=full, visible=visible)
