"""Shaded RGB training frames of coloured meshes, rendered on the device (csrc/render_rgb.hip).

  render_rgb        B poses of a MeshSet -> uint8 (B,H,W,3) frames (+ depth, mask, boxes, ok), cp_render_rgb
  sample_views      the host twin of bop_toolkit_lib.view_sampler.sample_views (float64 numpy; both modes)
  render_views      the loop of bop_toolkit's scripts/render_train_imgs.py:128-214 without the files
  synthetic_batch   render_rgb -> targets.make_training_batch: a training batch of an object nobody photographed
  render_scene      P poses on I images -> per image the occluded composite over a background, per pose gt_info's labels, the masks
                    as two bit planes per image (row N19; csrc/scene_labels.hip, cp_render_scene)
  scene_masks       a bit plane back as the uint8 (P,H,W) mask images it stands for (plain torch)
  scene_training_batch   render_scene -> bop_io's visibility filter -> the loader's tuple, the mask crops cut from the bit planes
  sample_scene_poses     the project's own placement of several objects per image (host, UNPINNED)

Render rule (renderer_py.py:24-105, 422-518 and renderer.py:23-29 read as a rule; stated per sample in csrc/render_rgb.hip):
coverage and the front-most surface are metric.render_depth's; over the winning triangle (the smallest face index among equal
1 / Z) v_color, v_L = normalize(light - eye_pos) per VERTEX and v_normal are interpolated perspective-correctly;
light_w = min(1, ambient_weight + max(dot(normalize(v_L), normalize(n)), 0)); the pixel is np.round(255 * light_w * v_color).
  shading "flat":  n = normalize(cross(dFdx(eye_pos), dFdy(eye_pos))), the face normal turned towards the viewer whatever the winding;
  shading "phong": n = the interpolated v_normal, taken as the shader writes it -- normalize(u_nm * vec4(a_normal, 1.0)).xyz, a
                   FOUR-vector normalisation before .xyz: the per-vertex lengths differ (the fourth component is 1 - t . (R n), far
                   from 0 at working distances) and weight the interpolation.  The quirk is kept, not corrected.
Vertex colours are divided by 255 when the mesh's largest value is > 1, a mesh without colours is 0.5 grey, `surf_color` replaces
both (renderer_py.add_object:313-352).

ssaa f in {1, 2, 4}: samples on the f-times finer grid under K * f (render_train_imgs.py:98-103), each sample quantised to uint8,
then f x f samples averaged per pixel as integers -- (s + 2) >> 2 for f = 2, round-half-even of s / 16 for f = 4.  This is the
project's statement of cv2.resize(INTER_AREA)'s integer-factor path on 8-bit images.

UNPINNED: (1) OpenGL's own output -- the shaders are GLSL and run nowhere this project runs, so the shading is pinned to the rule
read from them (tests/render_rgb_stages.py, float64), as the depth render of row N8 is; (2) cv2's INTER_AREA -- cv2 is not
available to the tests, as for the resize of row N3.  Specular terms, the C++ and vispy renderers, PLY reading and PNG writing are
not here.

Textures (row N20; stated in csrc/render_shade.h): a MeshSet built with textures= / uvs= colours a textured mesh's sample by its
texel -- (u, v) interpolated perspective-correctly like v_color, then the OpenGL specification's sampler rule with clamp-to-edge and no
mipmaps: "nearest" texel = T[Ht - 1 - clamp(floor(v Ht))][clamp(floor(u Wt))] (the reference uploads np.flipud(image)), "linear" the
bilinear blend about (u Wt - 0.5, v Ht - 0.5) -- and colour = light_w * (texel / 255).  add_object's order holds: surf_color, then the
texture, then vertex colours, then grey.  The filter lives on the MeshSet.  UNPINNED: which filter vispy selects for its Texture2D,
a driver's fixed-point filtering (GL implementations blend with a few fractional bits), OpenGL's own output, and the quantisation
of float textures to bytes (MeshSet.from_arrays).

The MeshSet and the handling of poses, camera, mesh ids, frame size and the light are checkerpose_amd/scene.py's (shared with
vis.vis_poses); the depth rasteriser alone is metric.render_depth.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _abi, gt_info, metric, scene
from .scene import SHADINGS   # noqa: F401  (public here since row N14)


def render_rgb(R, t, cam_K, meshes, size, mesh_ids=None, shading="phong", ambient_weight=0.5, light_cam_pos=(0, 0, 0),
               bg_color=(0, 0, 0), surf_color=None, ssaa=1, bgr=False, return_depth=False, return_mask=False, return_boxes=False,
               out=None):
    """uint8 frames of B poses of `meshes` (a MeshSet built with faces, and colors / normals as the shading needs them), shaded as
    bop_toolkit's RendererPython(mode='rgb') shades (module docstring), on the device (cp_render_rgb).
      R, t: (B,3,3) / (B,3,1) or (B,3) -- solve_pnp_ransac's tensors, or host arrays; cam_K: (3,3) or (B,3,3);
      size: (width, height); mesh_ids (B,) with several meshes;  shading "phong" (needs the MeshSet's normals) or "flat";
      ambient_weight, light_cam_pos: renderer.py:23-29 -- the light in the reference's camera frame (x right, y UP, z towards the
      viewer: OpenGL's), default at the camera;  bg_color, surf_color: RGB in [0, 1] (surf_color None: the mesh's colours, or grey);
      ssaa 1, 2 or 4;  bgr: store the channels reversed (what cv2.imread gives the loaders);
      out: a uint8 (B,H,W,3) contiguous tensor on the poses' device to write into.
    return_depth / return_mask / return_boxes (ssaa == 1 only: they belong to the sample grid, and a caller who wants depth beside an
    anti-aliased frame renders it with metric.render_depth, as render_train_imgs.py does): depth float32 (B,H,W), the same bits
    as metric.render_depth; mask uint8 (B,H,W) = 255 where depth > 0; boxes int32 (B,4) = misc.calc_2d_bbox of the mask (x, y, w, h),
    -1 where the mask is empty.
    A pose with a non-finite entry, a singular R or any vertex at Z <= 0 is not rendered: ok = 0, background only.
    -> {"rgb": uint8 (B,H,W,3), "ok": uint8 (B,)} (+ "depth", "mask", "boxes"), all on the device.  Four launches whatever the data."""
    shade, amb, light_c = scene.lighting(shading, ambient_weight, light_cam_pos)
    ssaa = int(ssaa)
    if ssaa not in (1, 2, 4):
        raise ValueError("ssaa must be 1, 2 or 4, got %r" % (ssaa,))
    if ssaa != 1 and (return_depth or return_mask or return_boxes):
        raise ValueError("depth, mask and boxes are made at ssaa=1 only: render them in a call of their own")
    bg_c = scene.vec3(bg_color, "bg_color")
    scene.check_shaded_meshes(meshes, shading, "render_rgb")
    W, H = scene.frame_size(size)
    dev, poses, B = scene.mesh_poses(*scene.poses_to_device("render", R, t), meshes)
    K, k_stride = scene.camera(cam_K, B, dev)
    ids, (vmax,) = scene.mesh_ids_on(mesh_ids, B, dev, meshes.sizes)
    verts, v_off = meshes.on(dev)
    faces, f_off, _ = meshes.faces_on(dev)
    colors, normals = meshes.shading_on(dev)
    if surf_color is not None:
        surf_c, colors = scene.vec3(surf_color, "surf_color"), None
    else:
        surf_c = scene.vec3((0.5, 0.5, 0.5), "surf_color")
    tex = meshes.textures_on(dev, use=surf_color is None)
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    elif not (torch.is_tensor(out) and out.device == dev and out.dtype == torch.uint8 and tuple(out.shape) == (B, H, W, 3)
              and out.is_contiguous()):
        raise ValueError("out must be a contiguous uint8 (%d,%d,%d,3) tensor on %s" % (B, H, W, dev))
    res = {"rgb": out, "ok": torch.empty(B, dtype=torch.uint8, device=dev)}
    if return_depth:
        res["depth"] = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    if return_mask:
        res["mask"] = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    if return_boxes:
        res["boxes"] = torch.empty((B, 4), dtype=torch.int32, device=dev)
    scratch = torch.empty(_abi.load().cp_render_rgb_scratch_bytes(B, vmax), dtype=torch.uint8, device=dev)
    _abi.call("cp_render_rgb_tex", dev, poses, K, k_stride, verts, v_off, faces, f_off, len(meshes), ids, colors, normals, surf_c, light_c, amb,
              bg_c, shade, ssaa, 1 if bgr else 0, H, W, B, vmax, out, res.get("depth"), res.get("mask"), res.get("boxes"), res["ok"], scratch,
              *tex)
    return res


# ---- view sampling (host, float64) -------------------------------------------------------------------------------------------------
def fibonacci_sampling(n_pts, radius=1.0):
    """view_sampler.fibonacci_sampling: an odd number of points of the Fibonacci lattice on the sphere -> list of [x, y, z]"""
    if n_pts % 2 != 1:
        raise ValueError("fibonacci_sampling needs an odd number of points")
    half = int(n_pts / 2)
    golden = (math.sqrt(5.0) + 1.0) / 2.0
    step = 2.0 * math.pi * (golden - 1.0)
    pts = []
    for i in range(-half, half + 1):
        lat = math.asin((2 * i) / float(2 * half + 1))
        lon = (step * i) % (2 * math.pi)
        s = math.cos(lat) * radius
        pts.append([math.cos(lon) * s, math.sin(lon) * s, math.tan(lat) * s])
    return pts


_ICO_FACES = ((0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
              (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1))


def hinter_sampling(min_n_pts, radius=1.0):
    """view_sampler.hinter_sampling: the icosahedron subdivided (edge midpoints, four faces per face) until it has at least
    `min_n_pts` vertices, projected onto the sphere, ordered from the top vertex outwards ring by ring, each ring by azimuth
    -> (points (n,3) float64, the subdivision level that created each point).  The ring order of points with EQUAL azimuth follows
    the iteration order of Python sets of small integers, as the reference's does."""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    pts = [(-1.0, g, 0.0), (1.0, g, 0.0), (-1.0, -g, 0.0), (1.0, -g, 0.0), (0.0, -1.0, g), (0.0, 1.0, g), (0.0, -1.0, -g), (0.0, 1.0, -g),
           (g, 0.0, -1.0), (g, 0.0, 1.0), (-g, 0.0, -1.0), (-g, 0.0, 1.0)]
    faces = list(_ICO_FACES)
    level_of = [0] * len(pts)
    level = 0
    while len(pts) < min_n_pts:
        level += 1
        mid, split = {}, []
        for face in faces:
            corner = list(face)
            for i in range(3):
                a, b = face[i], face[(i + 1) % 3]
                key = (a, b) if a < b else (b, a)
                if key not in mid:
                    mid[key] = len(pts)
                    pts.append((0.5 * (np.array(pts[key[0]]) + np.array(pts[key[1]]))).tolist())
                    level_of.append(level)
                corner.append(mid[key])
            split += [(corner[0], corner[3], corner[5]), (corner[3], corner[1], corner[4]), (corner[3], corner[4], corner[5]),
                      (corner[5], corner[4], corner[2])]
        faces = split
    pts = np.array(pts)
    pts *= np.reshape(radius / np.linalg.norm(pts, axis=1), (pts.shape[0], 1))
    linked = {}
    for face in faces:
        for i in range(3):
            linked.setdefault(face[i], set()).add(face[(i + 1) % 3])
            linked[face[i]].add(face[(i + 2) % 3])

    def azimuth(i):
        return (math.atan2(pts[i][1], pts[i][0]) + 2.0 * math.pi) % (2.0 * math.pi)

    order, ring, done = [], [int(np.argmax(pts[:, 2]))], [False] * pts.shape[0]
    while len(order) != pts.shape[0]:
        ring = sorted(ring, key=azimuth)
        reached = []
        for i in ring:
            order.append(i)
            done[i] = True
            reached += [j for j in linked[i]]
        ring = [j for j in set(reached) if not done[j]]
    return pts[np.array(order), :], [level_of[i] for i in order]


def sample_views(min_n_views, radius=1.0, azimuth_range=(0, 2 * math.pi), elev_range=(-0.5 * math.pi, 0.5 * math.pi),
                 mode="hinterstoisser"):
    """bop_toolkit_lib.view_sampler.sample_views on the host: viewpoints on a sphere of `radius` looking at its centre, those outside
    the azimuth / elevation ranges dropped -> (list of {'R': (3,3), 't': (3,1)} float64, views_level).  As in the reference,
    views_level has one entry per SAMPLED point (before the ranges cut any), and "fibonacci" rounds an even count up to odd."""
    if mode == "hinterstoisser":
        pts, levels = hinter_sampling(min_n_views, radius=radius)
    elif mode == "fibonacci":
        n = min_n_views if min_n_views % 2 == 1 else min_n_views + 1
        pts = fibonacci_sampling(n, radius=radius)
        levels = [0] * len(pts)
    else:
        raise ValueError("Unknown view sampling mode.")
    c, s = math.cos(math.pi), math.sin(math.pi)             # the half turn about x, as a rotation matrix of angle pi is formed
    flip = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    views = []
    for pt in pts:
        az = math.atan2(pt[1], pt[0])
        if az < 0:
            az += 2.0 * math.pi
        elev = math.acos(np.linalg.norm([pt[0], pt[1], 0]) / np.linalg.norm(pt))
        if pt[2] < 0:
            elev = -elev
        if not (azimuth_range[0] <= az <= azimuth_range[1] and elev_range[0] <= elev <= elev_range[1]):
            continue
        fwd = -np.array(pt)                                  # gluLookAt: forward, side, up
        fwd /= np.linalg.norm(fwd)
        side = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
        if np.count_nonzero(side) == 0:                      # looking along the z axis
            side = np.array([1.0, 0.0, 0.0])
        side /= np.linalg.norm(side)
        up = np.cross(side, fwd)
        R = flip.dot(np.array([[side[0], side[1], side[2]], [up[0], up[1], up[2]], [-fwd[0], -fwd[1], -fwd[2]]]))
        views.append({"R": R, "t": -R.dot(np.array(pt).reshape((3, 1)))})
    return views, levels


def render_views(meshes, obj_ids, cam_K, size, radii, min_n_views, azimuth_range=(0, 2 * math.pi),
                 elev_range=(-0.5 * math.pi, 0.5 * math.pi), depth_scale=1.0, ssaa=4, shading="phong", ambient_weight=0.5, batch=256,
                 mode="hinterstoisser", device=None):
    """The loop of scripts/render_train_imgs.py:128-214 without the files.  meshes: a MeshSet (faces, colours, normals) whose mesh m
    is object obj_ids[m]; per object and radius the views of sample_views are rendered in batches of `batch` poses: the frame with
    render_rgb (ssaa, shading, ambient_weight) and the depth with metric.render_depth at the frame's own K, divided by depth_scale.
    mode: sample_views' (the script fixes "hinterstoisser"); device: where to render (default: the current CUDA/HIP device).
    -> {obj_id: {"rgb": uint8 (n,H,W,3), "depth": float32 (n,H,W) (device tensors), "scene_gt": {im_id: [{'cam_R_m2c', 'cam_t_m2c',
    'obj_id'}]}, "scene_camera": {im_id: {'cam_K', 'depth_scale', 'view_level'}}}} in bop_toolkit's structure."""
    obj_ids = [int(o) for o in obj_ids]
    if len(obj_ids) != len(meshes):
        raise ValueError("need one object id per mesh")
    if int(batch) <= 0:
        raise ValueError("batch must be positive")
    K = np.asarray(cam_K, dtype=np.float64).reshape(3, 3)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    result = {}
    for m, obj_id in enumerate(obj_ids):
        scene_camera, scene_gt, Rs, ts = {}, {}, [], []
        for radius in radii:
            views, levels = sample_views(min_n_views, radius, azimuth_range, elev_range, mode)
            for view_id, view in enumerate(views):
                im_id = len(Rs)
                scene_camera[im_id] = {"cam_K": K, "depth_scale": depth_scale, "view_level": int(levels[view_id])}
                scene_gt[im_id] = [{"cam_R_m2c": view["R"], "cam_t_m2c": view["t"], "obj_id": obj_id}]
                Rs.append(view["R"])
                ts.append(view["t"])
        rgb, depth = [], []
        for i0 in range(0, len(Rs), int(batch)):
            Rb = torch.from_numpy(np.stack(Rs[i0:i0 + int(batch)])).to(device)
            tb = torch.from_numpy(np.stack(ts[i0:i0 + int(batch)])).to(device)
            ids = None if len(meshes) == 1 else torch.full((Rb.shape[0],), m, dtype=torch.int32, device=device)
            rgb.append(render_rgb(Rb, tb, K, meshes, size, mesh_ids=ids, shading=shading, ambient_weight=ambient_weight, ssaa=ssaa)["rgb"])
            depth.append(metric.render_depth(Rb, tb, K, meshes, size, mesh_ids=ids) / float(depth_scale))
        H, W = int(size[1]), int(size[0])
        result[obj_id] = {"rgb": torch.cat(rgb) if rgb else torch.empty((0, H, W, 3), dtype=torch.uint8, device=device),
                          "depth": torch.cat(depth) if depth else torch.empty((0, H, W), dtype=torch.float32, device=device),
                          "scene_gt": scene_gt, "scene_camera": scene_camera}
    return result


def synthetic_batch(meshes, mesh_ids, R, t, cam_K, size, p3d_xyz, augment=None, backgrounds=None, **render_kw):
    """A training batch of rendered frames: render_rgb(..., return_mask=True, return_boxes=True), then targets.make_training_batch
    with frame b for sample b, the mask as both masks_visib and masks_full (one object, nothing occludes it) and the boxes as the
    ground-truth boxes -- exactly that composition, bit for bit.  render_kw goes to render_rgb (ssaa must stay 1: the mask belongs to
    the sample grid); every sample must be rendered with a non-empty mask (ValueError otherwise: a sample needs its box).
    The boxes (16 bytes per sample) pass through the host, where make_training_batch grows them; no frame does.
    Several objects in one frame, hiding each other, with visible and full masks that differ: scene_training_batch."""
    from . import targets
    for k in ("return_depth", "return_mask", "return_boxes", "out"):
        if k in render_kw:
            raise ValueError("synthetic_batch sets %s itself" % k)
    Rt, tt = scene.poses_to_device("render", R, t)
    r = render_rgb(Rt, tt, cam_K, meshes, size, mesh_ids=mesh_ids, return_mask=True, return_boxes=True, **render_kw)
    boxes = r["boxes"].cpu().numpy()
    if (boxes[:, 0] < 0).any():
        raise ValueError("samples %r render nothing inside the frame: no box to crop" % (np.nonzero(boxes[:, 0] < 0)[0].tolist(),))
    B = boxes.shape[0]
    return targets.make_training_batch(r["rgb"], r["mask"], r["mask"], Rt, tt, cam_K, boxes, p3d_xyz, img_index=np.arange(B),
                                       augment=augment, backgrounds=backgrounds)


# ---- occluded scenes of several objects (row N19) --------------------------------------------------------------------------------------
MAX_SCENE_POSES = 32        # per image: one bit of the planes each


def _scene_backgrounds(backgrounds, bg_index, n_img, H, W):
    """the checks of render_scene's background arguments that need no device -> (backgrounds or None, host int32 ids or None)"""
    if backgrounds is None:
        if bg_index is not None:
            raise ValueError("bg_index without backgrounds")
        return None, None
    if not (torch.is_tensor(backgrounds) and backgrounds.dtype == torch.uint8 and backgrounds.dim() in (3, 4)):
        raise ValueError("backgrounds must be a uint8 (n_bg,H,W,3) tensor")
    bg = backgrounds.unsqueeze(0) if backgrounds.dim() == 3 else backgrounds
    if tuple(bg.shape[1:]) != (H, W, 3) or bg.shape[0] < 1:
        raise ValueError("backgrounds must be (n_bg,%d,%d,3), at the frame size; got %r" % (H, W, tuple(bg.shape)))
    n_bg = int(bg.shape[0])
    if bg_index is None:
        if n_bg not in (1, n_img):
            raise ValueError("%d backgrounds for %d images need bg_index" % (n_bg, n_img))
        return bg, None
    idx = np.asarray(bg_index.cpu() if torch.is_tensor(bg_index) else bg_index).reshape(-1).astype(np.int64)
    if idx.shape[0] != n_img or (n_img and (idx.min() < 0 or idx.max() >= n_bg)):
        raise ValueError("bg_index must be (I,) = (%d,) with values in 0..%d" % (n_img, n_bg - 1))
    return bg, idx.astype(np.int32)


def render_scene(R, t, cam_K, meshes, size, image_ids, mesh_ids=None, n_images=None, surf_colors=None, shading="phong",
                 ambient_weight=0.5, light_cam_pos=(0, 0, 0), bg_color=(0, 0, 0), backgrounds=None, bg_index=None, delta=15.0, bgr=False):
    """Occluded scenes of several objects with their labels, on the device (cp_render_scene): what vis.vis_poses(resolve_visib=True)
    followed by gt_info.gt_info(depth=ren_depth, return_masks=True) computes, bit for bit, in four launches, over a background.
      R, t: (P,3,3) / (P,3,1) or (P,3) -- device tensors, or host arrays; cam_K: (3,3) or (I,3,3), PER IMAGE; meshes: a MeshSet built
      with faces (colors / normals as the shading needs them), mesh_ids (P,) with several meshes; size: (width, height);
      image_ids (P,): each pose's image -- the poses of an image are composed in the order given, at most 32 of them (ValueError);
      n_images: I (default: the largest image id + 1; an image may have no pose);  surf_colors, shading, ambient_weight,
      light_cam_pos: vis_poses';  backgrounds: uint8 (n_bg,H,W,3) CUDA tensor behind the objects, image i showing row bg_index[i]
      (default: row i, or the only row), or None: bg_color, RGB in [0, 1];  delta: gt_info's visibility tolerance;  bgr: store the
      channels reversed (what cv2.imread gives the loaders).
    The slot of a pose is its rank among the poses of its image, in the order given; a pose that is not rendered keeps its slot.
    -> dict of device tensors: "rgb" uint8 (I,H,W,3) and "depth" float32 (I,H,W) -- vis_poses' ren_rgb (where depth > 0; the
    background elsewhere) and ren_depth; "full_bits", "visib_bits" int32 (I,H,W): bit s is set where the mask / mask_visib image of
    the pose at slot s would be 255 (scene_masks expands them; preprocess.get_roi_mask_bits crops them) -- 8 bytes per pixel whatever
    P is, against 2 P; "slot" int32 (P,); gt_info.KEYS as gt_info gives them with "depth" as the sensor depth; "ok" bool (P,) --
    False for a pose vis_poses does not render (a non-finite entry, a singular R, any vertex at Z <= 0): counts 0, boxes -1, no bit.
    Bit-identical from call to call, for an image alone or in a batch; the labels with or without backgrounds."""
    shade, amb, light_c = scene.lighting(shading, ambient_weight, light_cam_pos)
    bg_c = scene.vec3(bg_color, "bg_color")
    scene.check_shaded_meshes(meshes, shading, "render_scene")
    W, H = scene.frame_size(size)
    if not math.isfinite(float(delta)):
        raise ValueError("delta must be finite")
    P = int((R.shape if hasattr(R, "shape") else np.asarray(R).shape)[0])
    if P <= 0:
        raise ValueError("no poses")
    if image_ids is None:
        raise ValueError("render_scene needs image_ids: each pose's image")
    flat = np.asarray(image_ids.cpu() if torch.is_tensor(image_ids) else image_ids).reshape(-1)
    n_img = int(n_images) if n_images is not None else (int(flat.max()) + 1 if flat.size else 0)
    if n_img <= 0:
        raise ValueError("n_images must be positive")
    ids, off, order = scene.group_by_image(flat, P, n_img)
    if int(np.diff(off).max()) > MAX_SCENE_POSES:
        raise ValueError("image %d holds %d poses: at most %d per image (one bit of the planes each)"
                         % (int(np.diff(off).argmax()), int(np.diff(off).max()), MAX_SCENE_POSES))
    surf = scene.surf_colors_host(surf_colors, P)
    bg, bg_idx = _scene_backgrounds(backgrounds, bg_index, n_img, H, W)
    if bg is not None:
        scene.require_cuda("render", bg)
    dev, poses, _ = scene.mesh_poses(*scene.poses_to_device("render", R, t), meshes)
    if bg is not None and bg.device != dev:
        raise ValueError("backgrounds must live on the poses' device")
    mids, (vmax,) = scene.mesh_ids_on(mesh_ids, P, dev, meshes.sizes)
    K, k_stride = scene.camera(cam_K, n_img, dev, "I")
    verts, v_off = meshes.on(dev)
    faces, f_off, _ = meshes.faces_on(dev)
    colors, normals = meshes.shading_on(dev)
    surf_d = None if surf is None else torch.from_numpy(np.ascontiguousarray(surf)).to(dev)
    ids_d, off_d, order_d = (torch.from_numpy(a).to(dev) for a in (ids, off, order))
    bg_d = None if bg is None else bg.contiguous()
    bg_idx_d = None if bg_idx is None else torch.from_numpy(bg_idx).to(dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)      # noqa: E731
    rgb, depth = torch.empty((n_img, H, W, 3), dtype=torch.uint8, device=dev), torch.empty((n_img, H, W), dtype=torch.float32, device=dev)
    full, visib, slot, counts, boxes = i32(n_img, H, W), i32(n_img, H, W), i32(P), i32(P, 3), i32(P, 2, 4)
    fract, ok = torch.empty((P,), dtype=torch.float64, device=dev), torch.empty((P,), dtype=torch.uint8, device=dev)
    scratch = torch.empty(_abi.load().cp_render_scene_scratch_bytes(P, vmax, n_img), dtype=torch.uint8, device=dev)
    _abi.call("cp_render_scene_tex", dev, poses, K, k_stride, verts, v_off, faces, f_off, len(meshes), mids, colors, normals, surf_d, ids_d, off_d,
              order_d, off.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p), bg_d, 0 if bg_d is None else int(bg_d.shape[0]),
              bg_idx_d, bg_c, shade, amb, light_c, float(delta), 1 if bgr else 0, H, W, P, n_img, vmax, rgb, depth, full, visib, slot, counts,
              fract, boxes, ok, scratch, *meshes.textures_on(dev, use=surf is None))
    out = {"rgb": rgb, "depth": depth, "full_bits": full, "visib_bits": visib, "slot": slot}
    out.update(gt_info.label_dict(counts, fract, boxes, ok, None, None))
    return out


def scene_masks(bits, image_ids, slot):
    """The mask images a bit plane of render_scene stands for: bits int32 (I,H,W) ("full_bits" or "visib_bits"), image_ids (P,) and
    slot (P,) ("slot") -> uint8 (P,H,W) holding 0 / 255, gt_info's "mask" / "mask_visib".  A slot outside 0..31 gives zeros.
    Plain torch on the planes' device (a CPU tensor works): for callers and tests; the training path crops the planes directly."""
    bits = torch.as_tensor(bits)
    if bits.dim() != 3 or bits.dtype != torch.int32:
        raise ValueError("bits must be an int32 (I,H,W) tensor, got %s %r" % (bits.dtype, tuple(bits.shape)))
    ids = torch.as_tensor(image_ids).reshape(-1).to(device=bits.device, dtype=torch.int64)
    s = torch.as_tensor(slot).reshape(-1).to(device=bits.device, dtype=torch.int32)
    if ids.numel() != s.numel():
        raise ValueError("image_ids and slot must both be (P,)")
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= bits.shape[0]):
        raise ValueError("image_ids must name planes 0..%d" % (bits.shape[0] - 1))
    have = ((s >= 0) & (s < 32))[:, None, None]
    bit = torch.bitwise_right_shift(bits[ids], s.clamp(0, 31)[:, None, None]) & 1        # (arithmetic shift: the bit asked for is kept)
    return ((bit != 0) & have).to(torch.uint8) * 255


def _no_swap(augment):
    if augment is not None and (np.asarray(augment.bg_index) >= 0).any():
        raise ValueError("scene_training_batch: the plan swaps backgrounds (bg_index >= 0), which would erase the occluders -- "
                         "render_scene composites the background itself: pass backgrounds / bg_index to it")


def scene_training_batch(meshes, mesh_ids, R, t, cam_K, size, image_ids, p3d_xyz, visib_threshold=0.1, obj_ids=None, is_train=True,
                         padding_ratio=1.5, crop_size_img=256, crop_size_gt=64, resize_method="crop_square_resize", augment=None,
                         **scene_kw):
    """A training batch of occluded synthetic scenes: render_scene(R, t, cam_K, meshes, size, image_ids, mesh_ids, **scene_kw), the
    loader's filter visib_fract > visib_threshold (tools_for_BOP/bop_io.py:173-180, strict) over the rendered poses, then
    targets.make_training_batch's body for the poses kept -- sample b's frame is its image's "rgb", its box its "bbox_visib", and the
    two mask crops are cut from the bit planes (preprocess.get_roi_mask_bits): exactly make_training_batch on the expanded masks,
    bit for bit, without the 2 P mask images.
      cam_K (3,3) or (I,3,3) PER IMAGE; p3d_xyz (N,3) shared, (P,N,3) per pose, or with obj_ids (P,) the object table (n_obj,N,3);
      augment: an augment.AugmentPlan of P samples, one per POSE (rows of the poses kept are used), whose samples ask for no
      background swap (ValueError otherwise: the scene call composites the background itself -- scene_kw's backgrounds / bg_index);
      is_train, padding_ratio, crop sizes, resize_method: make_training_batch's (is_train draws the box jitter from np.random).
    -> (batch, kept): make_training_batch's 11 / 12 entries for the poses kept, and their indices (int64 numpy, ascending).
    Only the per-pose ok, fractions and boxes pass through the host."""
    from . import preprocess as PP
    from . import targets
    _no_swap(augment)
    P = int((R.shape if hasattr(R, "shape") else np.asarray(R).shape)[0])
    if augment is not None and augment.B != P:
        raise ValueError("augment: a plan of one sample per pose (%d), got %d" % (P, augment.B))
    Rt, tt = scene.poses_to_device("render", R, t)
    sc = render_scene(Rt, tt, cam_K, meshes, size, image_ids, mesh_ids=mesh_ids, **scene_kw)
    kept = scene_kept(sc["ok"].cpu().numpy(), sc["visib_fract"].cpu().numpy(), visib_threshold)
    img = np.asarray(image_ids.cpu() if torch.is_tensor(image_ids) else image_ids).reshape(-1).astype(np.int64)[kept]
    boxes = sc["bbox_visib"].cpu().numpy()[kept]
    slot = sc["slot"].cpu().numpy()[kept]
    dev, kept_d = Rt.device, torch.from_numpy(kept).to(Rt.device)
    K = torch.as_tensor(cam_K).to(device=dev, dtype=torch.float64)
    if K.dim() == 3:
        K = K[torch.from_numpy(img).to(dev)]
    p3 = p3d_xyz
    if obj_ids is None and torch.as_tensor(p3d_xyz).dim() == 3:
        p3 = torch.as_tensor(p3d_xyz)[kept_d.to(torch.as_tensor(p3d_xyz).device)]
    oid = None if obj_ids is None else np.asarray(obj_ids.cpu() if torch.is_tensor(obj_ids) else obj_ids).reshape(-1)[kept]
    plan = None if augment is None else augment.select(kept)
    crop_masks = lambda grown: (PP.get_roi_mask_bits(sc["visib_bits"], slot, grown, crop_size_gt, resize_method, img_index=img),      # noqa: E731
                                PP.get_roi_mask_bits(sc["full_bits"], slot, grown, crop_size_gt, resize_method, img_index=img))
    batch = targets.batch_from_frames(sc["rgb"], crop_masks, Rt[kept_d], tt[kept_d], K, list(boxes), p3, is_train, padding_ratio,
                                      crop_size_img, crop_size_gt, resize_method, img, oid, plan, None, None)
    return batch, kept


def scene_kept(ok, visib_fract, visib_threshold):
    """bop_io's sample filter on render_scene's host-side labels: the ascending int64 indices of the poses that were rendered (ok) and
    whose visib_fract is STRICTLY above the threshold (`visib_fract > train_obj_visible_theshold`, bop_io.py:173-180)"""
    ok, fract = np.asarray(ok).reshape(-1).astype(bool), np.asarray(visib_fract, dtype=np.float64).reshape(-1)
    return np.nonzero(ok & (fract > float(visib_threshold)))[0].astype(np.int64)


def sample_scene_poses(rng, n_images, objects_per_image, cam_K, size, z_range, n_meshes):
    """Poses for render_scene: objects_per_image objects in each of n_images images.
    UNPINNED -- this is the project's OWN placement rule, not a restatement of any reference code (the reference trains on scenes that
    BlenderProc / the BOP datasets placed): per pose, independently, the projected centre (u, v) is uniform in the frame [0, W) x
    [0, H), Z is uniform in z_range = (near, far), t = Z K^-1 (u, v, 1), the rotation is uniform on SO(3) (a normalised Gaussian
    quaternion), the mesh uniform among n_meshes.  Nothing keeps the objects from intersecting: the composite resolves depth per pixel.
      rng: a numpy.random.Generator; cam_K (3,3) shared or (n_images,3,3); size: (width, height).
    -> R (P,3,3), t (P,3,1) float64, image_ids (P,), mesh_ids (P,) int32 numpy arrays, P = n_images * objects_per_image, poses
    interleaved across images (pose j lies in image j % n_images) -- the same seed gives the same arrays."""
    n_img, per, M = int(n_images), int(objects_per_image), int(n_meshes)
    W, H = scene.frame_size(size)
    if n_img <= 0 or M <= 0 or not 1 <= per <= MAX_SCENE_POSES:
        raise ValueError("n_images and n_meshes must be positive, objects_per_image in 1..%d" % MAX_SCENE_POSES)
    z0, z1 = (float(v) for v in z_range)
    if not (0.0 < z0 <= z1 and math.isfinite(z1)):
        raise ValueError("z_range must be (near, far) with 0 < near <= far")
    K = np.asarray(cam_K, dtype=np.float64)
    if K.shape not in ((3, 3), (n_img, 3, 3)):
        raise ValueError("cam_K must be (3,3) or (n_images,3,3)")
    P = n_img * per
    image_ids = (np.arange(P) % n_img).astype(np.int32)
    Kp = np.broadcast_to(K, (n_img, 3, 3))[image_ids]
    q = rng.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                  2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
    u, v, Z = rng.uniform(0.0, W, size=P), rng.uniform(0.0, H, size=P), rng.uniform(z0, z1, size=P)
    t = Z[:, None] * np.linalg.solve(Kp, np.stack([u, v, np.ones(P)], 1)[:, :, None])[:, :, 0]
    mesh_ids = rng.integers(0, M, size=P).astype(np.int32)
    return R, t.reshape(P, 3, 1), image_ids, mesh_ids
