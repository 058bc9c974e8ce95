"""Poses verified against the photograph on the device (csrc/pose_verify_photo.hip).

Rows N26 (the sensor's depth), N28 (the predicted full mask) and N31 (an image's visible masks) see geometry only: a silhouette, and a
depth render, does not change when a geometrically symmetric object -- a can, a box, a bottle -- turns about its axis; the printed label
does.  Here a candidate pose's shaded render (render.render_rgb's bits, textures of row N20 included) is correlated with the frame's own
uint8 pixels inside the raster tile: no frame, render or dense mask is stored, the outputs are integer sums and the zero-mean normalised
cross-correlation of the two lumas, which a gain and an offset of the brightness leave unchanged.  verify_poses_photo scores poses,
estimate_poses_photo_verified is postprocess.estimate_poses that keeps per crop the stage's pose the photograph supports best; the choice
is postprocess.select_poses, unchanged.  Both are reached as postprocess.verify_poses_photo and
postprocess.estimate_poses_photo_verified.  The rule is the project's own (the reference never verifies), stated at the top of the kernel
file and restated in numpy by tests/photo_stages.py.  Opt-in, RGB-only.  No CPU fallback: CPU tensors raise."""
import numpy as np
import torch

from . import _abi

VERIFY_PHOTO_MAX_PIXELS = 1 << 22                   # csrc/pose_verify_photo.hip: a tile's sums are int32, a pose's products int64
VERIFY_PHOTO_SUMS = ("Sa", "Sb", "Saa", "Sbb", "Sab")
VERIFY_PHOTO_KEYS = ("meshes", "min_pixels", "mesh_ids", "use_visible", "shading", "ambient_weight", "light_cam_pos", "surf_color", "bgr")


def _check_frames(frames):
    """frames uint8 (n_img,H,W,3) or (H,W,3) -> (n_img, H, W); float frames and frames beyond H W <= 2^22 raise"""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or int(frames.shape[-1]) != 3:
        raise ValueError("frames must be a uint8 (n_img,H,W,3) or (H,W,3) tensor -- the photograph's own bytes, not a normalised float image"
                         "; got %s" % ("%s %r" % (frames.dtype, tuple(frames.shape)) if torch.is_tensor(frames) else type(frames).__name__))
    n_img = 1 if frames.dim() == 3 else int(frames.shape[0])
    H, W = int(frames.shape[-3]), int(frames.shape[-2])
    if n_img < 1 or H < 1 or W < 1:
        raise ValueError("frames are empty: %r" % (tuple(frames.shape),))
    if H * W > VERIFY_PHOTO_MAX_PIXELS:
        raise ValueError("frames: H * W must be <= 2^22 for cp_verify_poses_photo (a tile's sums are int32, a pose's products int64), "
                         "got %d x %d" % (H, W))
    return n_img, H, W


def _check_min_pixels(min_pixels):
    if isinstance(min_pixels, bool) or not isinstance(min_pixels, (int, np.integer)) or int(min_pixels) < 2 or int(min_pixels) >= 1 << 31:
        raise ValueError("min_pixels must be an integer >= 2 (no default: nothing fixes how few pixels make a correlation meaningful), "
                         "got %r" % (min_pixels,))
    return int(min_pixels)


def verify_poses_photo(R, t, cam_K, meshes, frames, min_pixels, image_ids=None, visible=None, mask_ids=None, mesh_ids=None, status=None,
                       shading="phong", ambient_weight=0.5, light_cam_pos=(0, 0, 0), surf_color=None, bgr=False):
    """Hypothesis verification of poses against the photograph on the device (row N35; opt-in, RGB-only -- the reference does not
    verify): each pose is rendered and shaded as render.render_rgb renders it at ssaa 1 and correlated with its frame inside one tile
    kernel -- no frame, render or dense mask is stored.  The rule is this project's own (csrc/pose_verify_photo.hip states it,
    tests/photo_stages.py restates it).  With C, D the pose's colour and depth render, Y = (77 R + 150 G + 29 B + 128) >> 8 the luma of the
    render (a) and of the frame (b), over the pixels D > 0 -- with `visible` also inside the pose's visible mask --:
      n, Sa, Sb, Saa, Sbb, Sab as integers; cov = n Sab - Sa Sb, va = n Saa - Sa^2, vb = n Sbb - Sb^2 (exact int64);
      ncc = cov / sqrt(va * vb), score = ncc, gain = cov / va, offset = (Sb - gain Sa) / n.
    Equal images give exactly 1.0; a frame 2 Y + 3 gives exactly 1.0 with gain exactly 2.0.
      R (P,3,3), t (P,3,1) / (P,3): CUDA/HIP tensors; cam_K (3,3) / (P,3,3); meshes: a MeshSet with faces (and colors / normals /
      textures as the shading needs them); frames: uint8 (n_img,H,W,3) or (H,W,3), resident, H W <= 2^22; min_pixels: an integer >= 2,
      NO default; image_ids (P,) or None: each pose's frame (None: the one frame, or frame p for pose p when n_img == P); visible: None,
      or the coco_eval.PackedMasks of the visible masks over the frames' size (paste_masks(seg, ..., channel=0)); mask_ids (P,) or None:
      each pose's mask row (None needs len(visible) == P); mesh_ids (P,) with several meshes; status (P,) or None: a pose whose entry is
      0 (the solvers' identity fallback) is no candidate; shading, ambient_weight, light_cam_pos, surf_color: render.render_rgb's;
      bgr: the FRAMES' bytes are B G R (what cv2.imread gives the loaders) -- the render's are not touched.
    -> (score (P,) f64, info): a dict of device tensors -- n_model (|D > 0|), n (P,) int32; Sa, Sb, Saa, Sbb, Sab (P,) int64; ncc, gain,
       offset (P,) f64; ok (P,) bool.  ok is False and score, ncc, gain, offset are NaN when va == 0 (a flat render), vb == 0 (a flat
       frame patch), n < min_pixels, or the pose is not counted at all (zero sums): a non-finite pose or cam_K, a singular R, a vertex at
       Z <= 0, a mesh, image or mask id out of range, status 0.  Every output is a function of integer sums: bitwise the same for a pose
       alone or in a batch."""
    from . import scene
    shade, amb, light_c = scene.lighting(shading, ambient_weight, light_cam_pos)
    min_pixels = _check_min_pixels(min_pixels)
    n_img, H, W = _check_frames(frames)
    n_masks = 0
    if visible is not None:
        from .verify_mask import _check_packed
        n_masks, Hm, Wm = _check_packed(visible, "visible")
        if (Hm, Wm) != (H, W) or n_masks < 1:
            raise ValueError("visible must hold masks of the frames' size %d x %d, got %d of %d x %d" % (H, W, n_masks, Hm, Wm))
    elif mask_ids is not None:
        raise ValueError("mask_ids belong to visible=...")
    scene.check_shaded_meshes(meshes, shading, "verify_poses_photo")
    dev, poses, P = scene.mesh_poses(R, t, meshes)
    scene.require_cuda("verify_photo", frames, *([visible.bits] if visible is not None else []))
    if status is not None and (not torch.is_tensor(status) or tuple(status.shape) != (P,)):
        raise ValueError("status must be a (P,) tensor or None")
    if status is not None:
        scene.require_cuda("verify_photo", status)
    m_ids = None
    if visible is not None:
        if mask_ids is None:
            if n_masks != P:
                raise ValueError("%d masks for %d poses need mask_ids" % (n_masks, P))
        elif torch.is_tensor(mask_ids) and mask_ids.is_cuda:          # resident ids stay there unread: an id outside 0..N-1 scores NaN
            if mask_ids.numel() != P:
                raise ValueError("mask_ids must be (P,)")
            m_ids = mask_ids.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        else:                                                       # host ids are checked
            host = np.asarray(mask_ids).reshape(-1).astype(np.int64)
            if host.shape[0] != P or host.min() < 0 or host.max() >= n_masks:
                raise ValueError("mask_ids must be (P,) with values in 0..%d" % (n_masks - 1))
            m_ids = torch.from_numpy(host.astype(np.int32)).to(dev)
    if torch.is_tensor(image_ids) and image_ids.is_cuda:              # resident ids stay there unread: an id outside 0..n_img-1 scores NaN
        i_ids = scene.image_ids_on(image_ids, P, n_img, dev)
    else:                                                           # scene.py's one default rule; host ids are checked
        host = scene.image_ids_host(image_ids, P, n_img, "frames", "P")
        i_ids = None if host is None else torch.from_numpy(host.astype(np.int32)).to(dev)
    K, k_stride = scene.camera(cam_K, P, dev, "P")
    ids, (vmax,) = scene.mesh_ids_on(mesh_ids, P, dev, meshes.sizes)
    verts, v_off = meshes.on(dev)
    faces, f_off, _ = meshes.faces_on(dev)
    colors, normals = meshes.shading_on(dev)
    if surf_color is not None:
        surf_c, colors = scene.vec3(surf_color, "surf_color"), None
    else:
        surf_c = scene.vec3((0.5, 0.5, 0.5), "surf_color")
    tex = meshes.textures_on(dev, use=surf_color is None)
    fr = frames.to(dev).contiguous()
    st_in = None if status is None else status.to(device=dev, dtype=torch.int32).contiguous()
    v_bits = None if visible is None else visible.bits.to(dev).contiguous()
    counts = torch.empty((P, 2), dtype=torch.int32, device=dev)
    sums = torch.empty((P, len(VERIFY_PHOTO_SUMS)), dtype=torch.int64, device=dev)
    ncc, score, gain, offset = (torch.empty((P,), dtype=torch.float64, device=dev) for _ in range(4))
    ok = torch.empty((P,), dtype=torch.uint8, device=dev)
    scratch = torch.empty(_abi.load().cp_verify_poses_photo_scratch_bytes(P, vmax), dtype=torch.uint8, device=dev)
    _abi.call("cp_verify_poses_photo_tex", dev, poses, K, k_stride, verts, v_off, faces, f_off, len(meshes), ids, colors, normals, surf_c, light_c,
              amb, shade, fr, i_ids, n_img, H, W, 1 if bgr else 0, v_bits, m_ids, n_masks, st_in, min_pixels, P, vmax, counts, sums, ncc, score,
              gain, offset, ok, scratch, *tex)
    info = dict(n_model=counts[:, 0], n=counts[:, 1])
    info.update({k: sums[:, i] for i, k in enumerate(VERIFY_PHOTO_SUMS)})
    info.update(ncc=ncc, gain=gain, offset=offset, ok=ok.bool())
    return score, info


def _check_verify_photo(verify):
    """estimate_poses_photo_verified's `verify` argument: a dict with meshes and min_pixels (optionally VERIFY_PHOTO_KEYS' others)"""
    if not isinstance(verify, dict) or "meshes" not in verify or "min_pixels" not in verify:
        raise ValueError("verify must be dict(meshes=..., min_pixels=...[, mesh_ids, use_visible, shading, ambient_weight, light_cam_pos, "
                         "surf_color, bgr])")
    if "image_ids" in verify or "status" in verify or "mask_ids" in verify:
        raise ValueError("verify must not name image_ids, status or mask_ids: the images are the call's img_index, the masks the crops' own "
                         "and the status is the solver's")
    extra = [k for k in verify if k not in VERIFY_PHOTO_KEYS]
    if extra:
        raise ValueError("verify: unknown key(s) %r" % (extra,))
    _check_min_pixels(verify["min_pixels"])


def estimate_poses_photo_verified(net, frames, Bboxes, p3d_xyz, cam_K, verify, return_verify=False, **estimate_kwargs):
    """estimate_poses with hypothesis verification against the photograph (row N35; RGB-only): the same call (estimate_kwargs are
    estimate_poses' keywords) with ONE forward; the poses after each stage the call runs (the solver's, then after "lm", then after
    "icp": 1, 2 or 3 candidates per crop, candidate-major) are rendered and correlated with the call's own uint8 frames -- each crop's
    frame is the call's img_index -- by ONE verify_poses_photo, and ONE select_poses keeps per crop the one the photograph supports.  With
    use_visible (default True) the forward's `seg` channel 0, the visible mask, is pasted (paste_masks, row N27) with the crops' own
    padded boxes and resize_method and restricts the comparison to where the object is seen.
      frames: uint8 (n_img,H,W,3) or (H,W,3), H W <= 2^22 -- float frames raise;
      verify: a dict with `meshes` (a MeshSet with faces, in the units of p3d_xyz) and `min_pixels` (no default), and optionally `mesh_ids`,
      `use_visible`, `shading`, `ambient_weight`, `light_cam_pos`, `surf_color`, `bgr` (verify_poses_photo's); `image_ids`, `status` and
      `mask_ids` are refused.  With use_visible, resize_method="crop_resize_by_warp_affine" raises paste_masks' NotImplementedError.
    -> (R, t, inliers, status, final boxes) as estimate_poses: R, t the chosen candidates' (their bits), inliers and status still the
       solver's; return_verify=True appends a dict: score (C,B), choice (B,) int32, stages (a tuple of "solver" / "lm" / "icp"), info
       (verify_poses_photo's dict over the C * B poses, candidate-major), image_ids (C * B,) as passed on (None with one frame), visible
       (the pasted PackedMasks; None without use_visible)."""
    from . import paste, postprocess
    _check_verify_photo(verify)
    n_frames, H, W = _check_frames(frames)
    use_visible = bool(verify.get("use_visible", True))
    method = estimate_kwargs.get("resize_method", "crop_square_resize")
    if use_visible:
        paste._check_paste_method(method)
    B = len(Bboxes)
    img_index = estimate_kwargs.get("img_index")
    if img_index is None:
        img = None if n_frames == 1 else np.arange(B, dtype=np.int64)      # get_roi_batch's default: crop b from frame b
    else:
        img = np.asarray(img_index.cpu() if torch.is_tensor(img_index) else img_index).reshape(-1).astype(np.int64)
    if img is not None and (img.shape[0] != B or (B and (img.min() < 0 or img.max() >= n_frames))):
        raise ValueError("img_index must be (B,) = (%d,) with values in 0..%d" % (B, n_frames - 1))
    keep = {}
    stages, inl, status, final = postprocess._estimate_stages(net, frames, Bboxes, p3d_xyz, cam_K, keep=keep, **estimate_kwargs)
    visible = postprocess.paste_masks(keep["seg"], keep["padded"], (H, W), method, 0) if use_visible else None
    C_ = len(stages)
    Rc = torch.stack([r.reshape(B, 3, 3) for _, r, _ in stages])
    tc = torch.stack([x.reshape(B, 3, 1) for _, _, x in stages])
    K = cam_K if torch.is_tensor(cam_K) else np.asarray(cam_K)
    if K.ndim == 3:
        K = K.repeat(C_, 1, 1) if torch.is_tensor(K) else np.tile(K, (C_, 1, 1))
    mesh_ids = verify.get("mesh_ids")
    if mesh_ids is not None:
        mesh_ids = mesh_ids.reshape(-1).repeat(C_) if torch.is_tensor(mesh_ids) else np.tile(np.asarray(mesh_ids).reshape(-1), C_)
    image_ids = None if img is None else np.tile(img, C_)
    kw = {k: verify[k] for k in ("shading", "ambient_weight", "light_cam_pos", "surf_color", "bgr") if k in verify}
    score, info = postprocess.verify_poses_photo(Rc.reshape(C_ * B, 3, 3), tc.reshape(C_ * B, 3, 1), K, verify["meshes"], frames,
                                                 verify["min_pixels"], image_ids=image_ids, visible=visible,
                                                 mask_ids=np.tile(np.arange(B), C_) if use_visible else None, mesh_ids=mesh_ids,
                                                 status=status.reshape(-1).repeat(C_), **kw)
    score = score.view(C_, B)
    choice, R, t = postprocess.select_poses(score, info["ok"].view(C_, B), Rc, tc)
    if not return_verify:
        return R, t, inl, status, final
    return R, t, inl, status, final, dict(score=score, choice=choice, stages=tuple(n for n, _, _ in stages), info=info, image_ids=image_ids,
                                          visible=visible)
