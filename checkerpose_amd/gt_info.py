"""BOP ground-truth info and masks on the device (row N10; csrc/gt_info.hip).

What bop_toolkit's scripts/calc_gt_info.py and scripts/calc_gt_masks.py write for every ground-truth pose of a scene -- the pixel
counts, visib_fract, bbox_obj, bbox_visib of scene_gt_info.json and the mask / mask_visib images -- computed for a batch of poses
in one call.  The reference renders each pose through OpenGL on a 3W x 3H canvas and makes full-frame numpy passes; here the
canvas is rendered tile by tile by metric.render_depth's rasteriser and counted in the same kernel.  Poses, camera, mesh and image ids
are handled by checkerpose_amd/scene.py, as for metric.vsd_errors.

  gt_info(...)              poses + meshes + sensor depth -> counts, fraction, boxes (+ masks, + the in-frame render)
  gt_info_from_depth(...)   the same counting on a caller's canvas render (B,3H,3W)
  scene_gt_info(...)        bop_toolkit's scene_gt / scene_camera dicts -> the structure of scene_gt_info.json, one device call
  save_scene_gt_info(...)   that structure as JSON

The `mask_visib`, `mask` and `bbox_visib` returned here are exactly what targets.make_training_batch takes as `masks_visib`,
`masks_full` and `Bboxes` (one mask pair per pose: pass img_index = the pose's own row): a scene that ships neither scene_gt_info.json
nor the mask folders can be trained on.  There is no CPU fallback."""
import json

import numpy as np
import torch

from . import _abi, scene

KEYS = ("px_count_all", "px_count_valid", "px_count_visib", "visib_fract", "bbox_obj", "bbox_visib")


def _outputs(B, H, W, dev, return_masks):
    """the output tensors both entry points fill: counts, fraction, boxes, ok (+ the two masks)"""
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)      # noqa: E731
    return (torch.empty((B, 3), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.float64, device=dev),
            torch.empty((B, 2, 4), dtype=torch.int32, device=dev), u8(B), u8(B, H, W) if return_masks else None,
            u8(B, H, W) if return_masks else None)


def label_dict(counts, fract, boxes, ok, mask, visib):
    """the result dict of the entry points from their output tensors (render.render_scene fills the same ones: mask, visib None)"""
    out = {"px_count_all": counts[:, 0], "px_count_valid": counts[:, 1], "px_count_visib": counts[:, 2], "visib_fract": fract,
           "bbox_obj": boxes[:, 0], "bbox_visib": boxes[:, 1], "ok": ok.to(torch.bool)}
    if mask is not None:
        out["mask"], out["mask_visib"] = mask, visib
    return out


def gt_info(R, t, cam_K, meshes, depth, image_ids=None, mesh_ids=None, delta=15.0, return_masks=False, return_depth=False):
    """calc_gt_info.py / calc_gt_masks.py for B ground-truth poses, rendered and counted on the device (cp_gt_info).
      R, t: (B,3,3) / (B,3,1) CUDA tensors; cam_K: (3,3) or (B,3,3); meshes: a MeshSet built with faces (with several meshes, mesh_ids
      (B,) names each pose's); depth: (H,W) or (I,H,W) sensor depth in the vertices' units (mm; 0 = no measurement), image_ids (B,)
      names each pose's image (default: the one image, or image b for pose b when I == B); delta: the visibility tolerance (15 mm;
      5 for itodd) -- the argument handling is metric.vsd_errors' (scene.py).
    -> dict of CUDA tensors: px_count_all (the silhouette on the 3W x 3H canvas, truncated part included), px_count_valid,
    px_count_visib int32 (B,); visib_fract float64 (B,); bbox_obj (the canvas silhouette in frame coordinates, not clipped: may be
    negative or exceed the frame), bbox_visib int32 (B,4) = x, y, xmax - xmin, ymax - ymin, BOTH -1 unless px_count_visib > 0;
    ok bool (B,) -- False for a pose that is not rendered (a NaN / inf entry, a device-side mesh / image id out of range, any vertex
    at Z <= 0): counts 0, fraction 0, boxes -1;  with return_masks "mask" and "mask_visib" uint8 (B,H,W) holding 0 / 255 (the
    mask files' content);  with return_depth "depth" float32 (B,H,W), the in-frame render -- the same bits as metric.render_depth
    at (W,H).  The other outputs are the same bits with or without the images.
    mask_visib, mask and bbox_visib are what targets.make_training_batch takes as masks_visib, masks_full and Bboxes."""
    dev, poses, B = scene.mesh_poses(R, t, meshes)
    K, k_stride = scene.camera(cam_K, B, dev)
    ids, (vmax,) = scene.mesh_ids_on(mesh_ids, B, dev, meshes.sizes)
    d, img, n_img = scene.depth_images(depth, image_ids, B, dev)
    H, W = int(d.shape[1]), int(d.shape[2])
    verts, v_off = meshes.on(dev)
    faces, f_off, _ = meshes.faces_on(dev)
    counts, fract, boxes, ok, mask, visib = _outputs(B, H, W, dev, return_masks)
    render = torch.empty((B, H, W), dtype=torch.float32, device=dev) if return_depth else None
    scratch = torch.empty(_abi.load().cp_gt_info_scratch_bytes(B, vmax), dtype=torch.uint8, device=dev)
    _abi.call("cp_gt_info", dev, poses, K, k_stride, verts, v_off, faces, f_off, len(meshes), ids, d, img, n_img, H, W, float(delta), B, vmax,
              counts, fract, boxes, ok, mask, visib, render, scratch)
    out = label_dict(counts, fract, boxes, ok, mask, visib)
    if return_depth:
        out["depth"] = render
    return out


def gt_info_from_depth(depth_gt_large, depth, cam_K, image_ids=None, delta=15.0, return_masks=False):
    """gt_info's counting on caller-supplied canvas renders (cp_gt_info_from_depth): depth_gt_large (B,3H,3W) float32 CUDA tensor, the
    object on the 3W x 3H canvas with the principal point moved by (W, H) -- frame pixel (x, y) is [y + H, x + W]; depth: (H,W) or
    (I,H,W) sensor depth.  -> gt_info's dict (ok is False only for a non-finite K or a device-side image id out of range)."""
    scene.require_cuda("gt_info", depth_gt_large)
    if depth_gt_large.dim() != 3 or depth_gt_large.shape[0] == 0:
        raise ValueError("depth_gt_large must be (B,3H,3W) with B >= 1, got %r" % (tuple(depth_gt_large.shape),))
    dev = depth_gt_large.device
    large = depth_gt_large.to(torch.float32).contiguous()
    B = int(large.shape[0])
    d, img, n_img = scene.depth_images(depth, image_ids, B, dev)
    H, W = int(d.shape[1]), int(d.shape[2])
    if tuple(large.shape[1:]) != (3 * H, 3 * W):
        raise ValueError("depth is %r, so depth_gt_large must be %r; got %r" % ((H, W), (3 * H, 3 * W), tuple(large.shape[1:])))
    K, k_stride = scene.camera(cam_K, B, dev)
    counts, fract, boxes, ok, mask, visib = _outputs(B, H, W, dev, return_masks)
    scratch = torch.empty(_abi.load().cp_gt_info_scratch_bytes(B, 0), dtype=torch.uint8, device=dev)
    _abi.call("cp_gt_info_from_depth", dev, large, K, k_stride, d, img, n_img, H, W, float(delta), B, counts, fract, boxes, ok, mask, visib,
              scratch)
    return label_dict(counts, fract, boxes, ok, mask, visib)


def scene_gt_info(scene_gt, scene_camera, depths, meshes, obj_index, delta=15.0, device="cuda:0", return_masks=False, _call=None):
    """calc_gt_info.py for one scene, in ONE device call.
      scene_gt: {im_id: [{"obj_id", "cam_R_m2c", "cam_t_m2c"}, ...]} and scene_camera: {im_id: {"cam_K", "depth_scale"}} as
      bop_toolkit's inout.load_scene_gt / load_scene_camera return them;  depths: {im_id: (H,W) array}, the depth images as stored
      (all of one size) -- multiplied by the image's depth_scale here, as the scripts do;  meshes: a MeshSet built with faces;
      obj_index: {obj_id: index of its mesh in `meshes`}.
    -> {im_id: [{"px_count_all": int, "px_count_valid": int, "px_count_visib": int, "visib_fract": float, "bbox_obj": [int x 4],
    "bbox_visib": [int x 4]}, ...]}, one entry per ground truth in scene_gt's order: the content of scene_gt_info.json.
    With return_masks -> (that, {(im_id, gt_id): (mask, mask_visib)}) with the uint8 (H,W) arrays of the mask files -- what
    targets.make_training_batch takes as masks_full / masks_visib, with bbox_visib as its Bboxes."""
    im_ids = sorted(scene_gt.keys())
    rows = [(i, im_id, gt_id, gt) for i, im_id in enumerate(im_ids) for gt_id, gt in enumerate(scene_gt[im_id])]
    if not rows:
        return ({im_id: [] for im_id in im_ids}, {}) if return_masks else {im_id: [] for im_id in im_ids}
    for _, _, _, gt in rows:
        if gt["obj_id"] not in obj_index:
            raise ValueError("obj_id %r is not in obj_index" % (gt["obj_id"],))
    stack = []
    for im_id in im_ids:
        d = np.asarray(depths[im_id], dtype=np.float32)
        if d.ndim != 2 or (stack and d.shape != stack[0].shape):
            raise ValueError("every depth image must be (H,W) of one size")
        stack.append(d * np.float32(scene_camera[im_id].get("depth_scale", 1.0)))       # inout.load_depth gives float32; `depth *= scale`
    R = np.stack([np.asarray(gt["cam_R_m2c"], dtype=np.float64).reshape(3, 3) for _, _, _, gt in rows])
    t = np.stack([np.asarray(gt["cam_t_m2c"], dtype=np.float64).reshape(3, 1) for _, _, _, gt in rows])
    K = np.stack([np.asarray(scene_camera[im_id]["cam_K"], dtype=np.float64).reshape(3, 3) for _, im_id, _, _ in rows])
    call = gt_info if _call is None else _call
    dev = torch.device(device)
    out = call(torch.from_numpy(R).to(dev), torch.from_numpy(t).to(dev), K, meshes, np.stack(stack),
               image_ids=[i for i, _, _, _ in rows], mesh_ids=[int(obj_index[gt["obj_id"]]) for _, _, _, gt in rows], delta=delta,
               return_masks=return_masks)
    host = {k: out[k].cpu().numpy() for k in KEYS}
    info = {im_id: [] for im_id in im_ids}
    for j, (_, im_id, _, _) in enumerate(rows):
        info[im_id].append({"px_count_all": int(host["px_count_all"][j]), "px_count_valid": int(host["px_count_valid"][j]),
                            "px_count_visib": int(host["px_count_visib"][j]), "visib_fract": float(host["visib_fract"][j]),
                            "bbox_obj": [int(e) for e in host["bbox_obj"][j]], "bbox_visib": [int(e) for e in host["bbox_visib"][j]]})
    if not return_masks:
        return info
    m, mv = out["mask"].cpu().numpy(), out["mask_visib"].cpu().numpy()
    return info, {(im_id, gt_id): (m[j], mv[j]) for j, (_, im_id, gt_id, _) in enumerate(rows)}


def save_scene_gt_info(path, info):
    """scene_gt_info's result as scene_gt_info.json: one line per image, keys as strings in ascending order (inout.save_json's
    layout for a dict of lists)"""
    with open(path, "w") as f:
        f.write("{\n")
        keys = sorted(info.keys())
        for n, k in enumerate(keys):
            f.write('  "%d": %s%s\n' % (int(k), json.dumps(info[k], sort_keys=True), "," if n + 1 < len(keys) else ""))
        f.write("}")
