"""Poses drawn over the photograph, on the device (csrc/vis_poses.hip).

  vis_poses         P poses on I frames -> per image the composite of its poses, their 2-D boxes, the blend with the frame, cp_vis_poses
  depth_diff_vis    the depth-difference picture of any render against a sensor depth, cp_depth_diff_vis
  select_estimates  the choice of estimates scripts/vis_est_poses.py:151-181 makes (host)
  vis_est_poses     scripts/vis_est_poses.py without the files: ONE vis_poses call for a scene's estimates
  vis_gt_poses      scripts/vis_gt_poses.py without the files: ONE vis_poses call for a scene's ground truths

The rule (bop_toolkit_lib/visualization.py:90-235, vis_object_poses, read as a rule; stated per pixel in csrc/vis_poses.hip).  Per
image, poses in the order given: m_rgb and m_depth of a pose are render.render_rgb(ssaa=1, bg_color=(0, 0, 0), return_depth=True) of
that pose alone, bit for bit, with the pose's own surface colour or the mesh's colours.  ren_rgb = 0, ren_depth = 0;
m = m_depth != 0 and (ren_depth == 0 or m_depth < ren_depth) on the float32 depths, strict; ren_depth[m] = m_depth;
resolve_visib: ren_rgb[m] = m_rgb, otherwise ren_rgb = min(255, ren_rgb + m_rgb).  The box of a pose covers the pixels where any
channel of m_rgb is > 0 (the reference's obj_mask: a black surface occludes but has no box): x, y, xmax - xmin, ymax - ymin, or -1.
A pixel on the one-pixel outline through (x, y), (x + w, y + h) of any box of its image holds int(c * 255) of box_color;
vis = min(255, (frame + ren_rgb) // 2 + outline), as integers -- the reference's float32 0.5 a + 0.5 b + 1.0 c, clipped and truncated.
A pose that render_rgb does not render (a non-finite entry, a singular R, any vertex at Z <= 0) is skipped and reported in `ok`; the
reference would show clipped geometry.

Depth difference (visualization.py:206-235 with depth_for_vis): valid = depth > 0 and ren_depth > 0; dd = valid ? ren_depth - depth : 0
in float32; red = 255 where valid and dd < delta; m0 = min dd over ALL pixels; x = dd - m0; over x > 0, in float64,
n = (x - min x) / (max (x - min x) / (1.0 - 0.2)) + 0.2; green = blue = uint8(255 n) by truncation; 0 where not valid.  An image whose dd
holds fewer than three distinct values gets diff_ok = 0 and zeros (the reference raises or divides 0 by 0).

UNPINNED / out of scope: the text the reference writes on both pictures (its font call does not exist in the Pillow at hand; `boxes`
are returned for a caller who annotates), JPEG / PNG writing, dataset folders, SSAA in the composite.  A textured MeshSet (row N20) is drawn with its textures, by render_rgb's rule.  OpenGL's own output
is unpinned as for render_rgb.  There is no CPU fallback.

Poses, camera (per IMAGE here), mesh ids, the grouping of the poses by image (scene.group_by_image) and the light are handled by
checkerpose_amd/scene.py, which render.render_rgb shares."""
import ctypes as C
import math

import numpy as np
import torch

from . import _abi, scene

_S = 1.0 - 0.2      # depth_for_vis' valid_end - valid_start, as Python forms it


def _frames_checked(frames):
    if not (torch.is_tensor(frames) or isinstance(frames, np.ndarray)):
        raise ValueError("frames must be a uint8 (I,H,W,3) tensor")
    f = torch.as_tensor(frames)
    if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3 or min(f.shape[:3]) <= 0:
        raise ValueError("frames must be uint8 (I,H,W,3), got %s %r" % (f.dtype, tuple(f.shape)))
    return f


def _depth_checked(depth, shape):
    if not (torch.is_tensor(depth) or isinstance(depth, np.ndarray)):
        raise ValueError("depth must be an (I,H,W) tensor")
    d = torch.as_tensor(depth)
    if d.dim() == 2:
        d = d[None]
    if tuple(d.shape) != tuple(shape):
        raise ValueError("depth must be %r, got %r" % (tuple(shape), tuple(d.shape)))
    return d


def depth_diff_vis(ren_depth, depth, image_ids=None, delta=15.0):
    """The reference's depth-difference picture (module docstring) of B renders ren_depth (B,H,W) float32 CUDA against sensor depths
    depth (H,W) or (I,H,W) in the same units (0 = no measurement); image_ids (B,) names each render's depth image (default: the one
    image, or image b for render b when I == B).
    -> {"depth_diff": uint8 (B,H,W,3), "diff_stats": float64 (B,3) = min, max, mean of the difference over the valid pixels (NaN
    when none is valid), "diff_ok": uint8 (B,) -- 0 where the difference holds fewer than three distinct values: an all-zero picture}.
    Five launches (cp_depth_diff_vis), integer atomics only: bit-identical from call to call, for an image alone or in a batch."""
    if not (torch.is_tensor(ren_depth) or isinstance(ren_depth, np.ndarray)):
        raise ValueError("ren_depth must be a (B,H,W) tensor")
    r = torch.as_tensor(ren_depth)
    if r.dim() == 2:
        r = r[None]
    if r.dim() != 3 or min(r.shape) <= 0:
        raise ValueError("ren_depth must be (B,H,W), got %r" % (tuple(r.shape),))
    if not math.isfinite(float(delta)):
        raise ValueError("delta must be finite")
    B, H, W = (int(v) for v in r.shape)
    if not (torch.is_tensor(depth) or isinstance(depth, np.ndarray)):
        raise ValueError("depth must be an (H,W) or (I,H,W) tensor")
    dshape = tuple(torch.as_tensor(depth).shape)
    if len(dshape) not in (2, 3) or tuple(dshape[-2:]) != (H, W):
        raise ValueError("depth must be (H,W) or (I,H,W) with H, W = %d, %d; got %r" % (H, W, dshape))
    scene.require_cuda("vis", r)
    dev = r.device
    r = r.to(torch.float32).contiguous()
    d, img, n_img = scene.depth_images(depth, image_ids, B, dev)
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    stats = torch.empty((B, 3), dtype=torch.float64, device=dev)
    ok = torch.empty((B,), dtype=torch.uint8, device=dev)
    scratch = torch.empty(_abi.load().cp_depth_diff_vis_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    _abi.call("cp_depth_diff_vis", dev, r, d, img, n_img, float(delta), _S, H, W, B, out, stats, ok, scratch)
    return {"depth_diff": out, "diff_stats": stats, "diff_ok": ok}


def vis_poses(R, t, cam_K, meshes, frames, image_ids=None, mesh_ids=None, surf_colors=None, resolve_visib=True, draw_boxes=True,
              box_color=(0.3, 0.3, 0.3), shading="phong", ambient_weight=0.5, light_cam_pos=(0, 0, 0), depth=None, depth_diff=False,
              delta=15.0):
    """P poses drawn over I frames, as bop_toolkit's visualization.vis_object_poses draws them (module docstring), on the device.
      R, t: (P,3,3) / (P,3,1) or (P,3) -- device tensors, or host arrays; cam_K: (3,3) or (I,3,3), PER IMAGE;
      meshes: a MeshSet built with faces (colors / normals as the shading needs them), mesh_ids (P,) with several meshes;
      frames: uint8 (I,H,W,3) CUDA tensor, the photographs (RGB);  image_ids (P,): each pose's frame (default: the one frame, or
      frame b for pose b when I == P) -- the poses of a frame are drawn in the order given;
      surf_colors: (P,3) or one colour, RGB in [0, 1] (None: the mesh's colours, or grey);  resolve_visib: the front-most object per
      pixel, otherwise a saturating sum;  draw_boxes, box_color: the 2-D boxes' outline;  shading, ambient_weight, light_cam_pos:
      render_rgb's;  depth (I,H,W) or (H,W) with I == 1: the sensor depth, needed with depth_diff only;  delta: its tolerance.
    -> {"vis", "ren_rgb": uint8 (I,H,W,3), "ren_depth": float32 (I,H,W), "boxes": int32 (P,4) x, y, w, h (-1 without a coloured
    pixel), "ok": uint8 (P,)} on the device; with depth_diff also depth_diff_vis' "depth_diff", "diff_stats", "diff_ok" of ren_depth.
    Four launches whatever the data (cp_vis_poses); bit-identical from call to call, for an image alone or in a batch."""
    shade, amb, light_c = scene.lighting(shading, ambient_weight, light_cam_pos)
    box_c = scene.vec3(box_color, "box_color")
    fr = _frames_checked(frames)
    n_img, H, W = (int(v) for v in fr.shape[:3])
    scene.check_shaded_meshes(meshes, shading, "vis_poses")
    P = int((R.shape if hasattr(R, "shape") else np.asarray(R).shape)[0])
    if P <= 0:
        raise ValueError("no poses")
    ids, off, order = scene.group_by_image(image_ids, P, n_img)
    surf = scene.surf_colors_host(surf_colors, P)
    if depth_diff:
        if depth is None:
            raise ValueError("depth_diff needs the sensor depth")
        depth = _depth_checked(depth, (n_img, H, W))
    scene.require_cuda("vis", fr)
    dev = fr.device
    fr = fr.contiguous()
    _, poses, B = scene.mesh_poses(*scene.poses_to_device("vis", torch.as_tensor(R).to(dev), torch.as_tensor(t).to(dev)), meshes)
    mids, (vmax,) = scene.mesh_ids_on(mesh_ids, B, dev, meshes.sizes)
    K, k_stride = scene.camera(cam_K, n_img, dev, "I")
    verts, v_off = meshes.on(dev)
    faces, f_off, _ = meshes.faces_on(dev)
    colors, normals = meshes.shading_on(dev)
    surf_d = None if surf is None else torch.from_numpy(np.ascontiguousarray(surf)).to(dev)
    ids_d, off_d, order_d = (torch.from_numpy(a).to(dev) for a in (ids, off, order))
    res = {"vis": torch.empty((n_img, H, W, 3), dtype=torch.uint8, device=dev),
           "ren_rgb": torch.empty((n_img, H, W, 3), dtype=torch.uint8, device=dev),
           "ren_depth": torch.empty((n_img, H, W), dtype=torch.float32, device=dev),
           "boxes": torch.empty((P, 4), dtype=torch.int32, device=dev), "ok": torch.empty((P,), dtype=torch.uint8, device=dev)}
    scratch = torch.empty(_abi.load().cp_vis_poses_scratch_bytes(P, vmax, n_img), dtype=torch.uint8, device=dev)
    _abi.call("cp_vis_poses_tex", dev, poses, K, k_stride, verts, v_off, faces, f_off, len(meshes), mids, colors, normals, surf_d, ids_d, off_d,
              order_d, off.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p), fr, shade, amb, light_c, box_c,
              1 if resolve_visib else 0, 1 if draw_boxes else 0, H, W, P, n_img, vmax, res["vis"], res["ren_rgb"], res["ren_depth"],
              res["boxes"], res["ok"], scratch, *meshes.textures_on(dev, use=surf is None))
    if depth_diff:
        res.update(depth_diff_vis(res["ren_depth"], depth.to(dev), delta=delta))
    return res


# ---- the two scripts, host dict work only ---------------------------------------------------------------------------------------------
def select_estimates(ests, n_top=1, scene_gt=None):
    """scripts/vis_est_poses.py:151-181: ests, a list of {"im_id", "obj_id", "score", "R", "t"} of ONE scene, organised by image and
    object in first-appearance order; per (image, object) sorted by score descending (stable: ties keep the input order) and cut to
    n_top -- 0 = all, -1 = the number of that object's ground truths in scene_gt[im_id], otherwise n_top.
    -> {im_id: {obj_id: [est, ...]}} (dicts keep insertion order)."""
    n_top = int(n_top)
    if n_top < -1:
        raise ValueError("n_top must be -1, 0 or positive")
    if n_top == -1 and scene_gt is None:
        raise ValueError("n_top = -1 counts the ground truths: pass scene_gt")
    org = {}
    for est in ests:
        org.setdefault(est["im_id"], {}).setdefault(est["obj_id"], []).append(est)
    out = {}
    for im_id, im_ests in org.items():
        out[im_id] = {}
        for obj_id, obj_ests in im_ests.items():
            ranked = sorted(obj_ests, key=lambda e: e["score"], reverse=True)
            if n_top == 0:
                cut = None
            elif n_top == -1:
                cut = sum(gt["obj_id"] == obj_id for gt in scene_gt[im_id])
            else:
                cut = n_top
            out[im_id][obj_id] = ranked[slice(0, cut)]
    return out


def _scene_call(groups, scene_camera, frames, meshes, obj_index, palette, device, vis_kw):
    """groups: [(vis_name, im_id, [(obj_id, R, t), ...])] -> {vis_name: one image's slice of ONE vis_poses call}"""
    if not groups:
        return {}
    for k in ("image_ids", "mesh_ids", "surf_colors"):
        if k in vis_kw:
            raise ValueError("%s is set from the scene" % k)
    rows = [(g, obj_id, R, t) for g, (_, _, poses) in enumerate(groups) for obj_id, R, t in poses]
    for _, obj_id, _, _ in rows:
        if obj_id not in obj_index:
            raise ValueError("obj_id %r is not in obj_index" % (obj_id,))
    stack = []
    for _, im_id, _ in groups:
        f = np.asarray(frames[im_id])
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or (stack and f.shape != stack[0].shape):
            raise ValueError("every frame must be uint8 (H,W,3) of one size")
        stack.append(f)
    depth = vis_kw.pop("depth", None)
    if depth is not None:
        depth = np.stack([np.asarray(depth[im_id], dtype=np.float32) * np.float32(scene_camera[im_id].get("depth_scale", 1.0))
                          for _, im_id, _ in groups])
    K = np.stack([np.asarray(scene_camera[im_id]["cam_K"], dtype=np.float64).reshape(3, 3) for _, im_id, _ in groups])
    dev = torch.device(device)
    fr = torch.from_numpy(np.stack(stack)).to(dev)
    if not rows:
        raise ValueError("no pose to draw in any image")
    Rs = np.stack([np.asarray(R, dtype=np.float64).reshape(3, 3) for _, _, R, _ in rows])
    ts = np.stack([np.asarray(t, dtype=np.float64).reshape(3, 1) for _, _, _, t in rows])
    surf = None if palette is None else np.asarray([palette[(int(obj_id) - 1) % len(palette)] for _, obj_id, _, _ in rows], dtype=np.float64)
    out = vis_poses(torch.from_numpy(Rs).to(dev), torch.from_numpy(ts).to(dev), K, meshes, fr, image_ids=[g for g, _, _, _ in rows],
                    mesh_ids=[int(obj_index[obj_id]) for _, obj_id, _, _ in rows], surf_colors=surf, depth=depth, **vis_kw)
    res = {}
    for g, (name, _, _) in enumerate(groups):
        mine = [j for j, r in enumerate(rows) if r[0] == g]
        one = {k: out[k][g] for k in ("vis", "ren_rgb", "ren_depth", "depth_diff", "diff_stats", "diff_ok") if k in out}
        one["boxes"], one["ok"] = out["boxes"][mine], out["ok"][mine]
        res[name] = one
    return res


def vis_est_poses(ests, scene_camera, frames, meshes, obj_index, palette=None, vis_per_obj_id=True, n_top=1, scene_gt=None,
                  device="cuda:0", **vis_kw):
    """scripts/vis_est_poses.py for one scene without the files, in ONE vis_poses call.  ests: [{"im_id", "obj_id", "score", "R", "t"}]
    (inout.load_bop_results' entries of the scene); scene_camera: {im_id: {"cam_K", "depth_scale"}}; frames: {im_id: uint8 (H,W,3)};
    meshes, obj_index: {obj_id: index of its mesh}; palette: a list of RGB colours in [0, 1] (the reference's colors.json) --
    palette[(obj_id - 1) % len(palette)] is the object's surface colour, None = the mesh's own colours (vis_orig_color);
    select_estimates(ests, n_top, scene_gt) chooses; vis_per_obj_id: one picture per (im_id, obj_id), otherwise one per im_id with
    the objects' estimates chained.  vis_kw goes to vis_poses (defaults as the script: phong, resolve_visib); depth={im_id: (H,W)}
    as stored (multiplied by depth_scale here) with depth_diff=True.
    -> {(im_id, obj_id) or im_id: {"vis", "ren_rgb", "ren_depth", "boxes", "ok" (+ the depth-difference entries)}}."""
    chosen = select_estimates(ests, n_top, scene_gt)
    groups = []
    for im_id, im_ests in chosen.items():
        per_obj = [(obj_id, [(obj_id, e["R"], e["t"]) for e in obj_ests]) for obj_id, obj_ests in im_ests.items()]
        if vis_per_obj_id:
            groups += [((im_id, obj_id), im_id, poses) for obj_id, poses in per_obj]
        else:
            groups.append((im_id, im_id, [p for _, poses in per_obj for p in poses]))
    return _scene_call(groups, scene_camera, frames, meshes, obj_index, palette, device, dict(vis_kw))


def vis_gt_poses(scene_gt, scene_camera, frames, meshes, obj_index, palette=None, gt_ids=None, device="cuda:0", **vis_kw):
    """scripts/vis_gt_poses.py for one scene without the files, in ONE vis_poses call: per image (ascending im_id) its ground truths
    in gt order (gt_ids: only those indices), flat shading as the script sets it.  Arguments as vis_est_poses.
    -> {im_id: {"vis", "ren_rgb", "ren_depth", "boxes", "ok" (+ the depth-difference entries)}}."""
    vis_kw = dict(vis_kw)
    vis_kw.setdefault("shading", "flat")
    groups = []
    for im_id in sorted(scene_gt.keys()):
        keep = range(len(scene_gt[im_id])) if not gt_ids else sorted(set(range(len(scene_gt[im_id]))).intersection(gt_ids))
        groups.append((im_id, im_id, [(scene_gt[im_id][g]["obj_id"], scene_gt[im_id][g]["cam_R_m2c"], scene_gt[im_id][g]["cam_t_m2c"])
                                      for g in keep]))
    return _scene_call(groups, scene_camera, frames, meshes, obj_index, palette, device, vis_kw)
