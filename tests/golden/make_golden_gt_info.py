#!/usr/bin/env python3
"""Row N10 (BOP ground-truth info and masks) pinned by the REFERENCE's own scripts after the render.

Runs ONLY where the reference tree is (CHECKERPOSE_REFERENCE, default /root/reference; nothing of it travels, only the recorded
numbers in gt_info.npz are committed):

  python tests/golden/make_golden_gt_info.py

The reference's own scripts bop_toolkit/scripts/calc_gt_info.py and calc_gt_masks.py are RUN, whole, under runpy -- once per scene
of SCENES.  They cannot reach a dataset or an OpenGL context here, so what they import is given stand-ins before they start:
  renderer.create_renderer      -> a stub whose render_object(...)['depth'] is the float32 depth of tests/vsd_stages.oracle_render (the
                                   render rule in float64) at the canvas size and principal point the script asks for.  calc_gt_masks.py
                                   asks for the frame-sized render: it gets the in-frame part of the same canvas render, so both
                                   scripts see one surface;
  dataset_params.get_split_params / get_model_params / get_present_scene_ids -> the scene's size and path templates that only the
                                   stubs below read.  get_split_params also sets the script's own PARAMETERS entry p['delta'] (the
                                   knob its comment says to edit: "5 for ITODD, 15 for the other datasets") to the scene's delta;
  inout.load_scene_gt / load_scene_camera / load_depth -> the poses, intrinsics and depth images drawn here (load_depth returns
                                   the stored image, the scripts multiply by depth_scale themselves); misc.Precomputer is reset
                                   there, i.e. before every image;
  inout.save_json / save_im, misc.ensure_dir, misc.log -> capture what the scripts save; nothing is written.
  (imageio / png, which inout imports for the loaders that are replaced, are empty modules.)
Everything between the render and the saved values is the scripts' own code: depth_im_to_dist_im_fast, estimate_visib_mask_gt, the
counts, the fraction, calc_2d_bbox, 255 * mask.  depth_gt_large is taken from the stub renderer's record of what it handed in.

Every recorded visibility decision (the fp32 difference against delta) lies at least 1e-6 (relative) from its boundary -- except a
few pixels of the "straddle64" image, moved float by float to where the fp32 and the fp64 difference fall on opposite sides of delta -- and at most
5 % of a case's covered canvas pixels are undecided in the oracle: a case that fails either is redrawn with the next seed.  The pose
with a vertex behind the camera is outside the render rule (the oracle refuses it): it is recorded with the project's own answer for
it, ok = 0, and does not pass through the scripts."""
import os
import runpy
import sys
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "bop_toolkit"))
sys.path.insert(0, ROOT)
for name in ("imageio", "png"):
    if name not in sys.modules:
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)

from bop_toolkit_lib import dataset_params, inout, misc, renderer  # noqa: E402
from tests import gt_info_stages as G  # noqa: E402
from tests import vsd_stages as S  # noqa: E402

LM_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])

# scene id -> ((W, H), delta, depth_scale)
SCENES = {1: ((67, 45), 15, 1.0), 2: ((33, 31), 15, 1.0), 3: ((160, 120), 15, 1.0), 4: ((64, 64), 5, 1.0), 5: ((96, 80), 5, 0.5)}
# (scene, image, mesh, depth kind of the image (its first entry's counts), shift of the centre in frame widths / heights, K group, placement)
CASES = [
    (1, 0, "box", "plane", (0.0, 0.0), 0, "centre"),              # wholly in the frame
    (1, 1, "box", "plane", (-0.5, 0.0), 0, "centre"),             # straddling the left edge
    (1, 2, "ico80", "noise", (0.05, -0.5), 0, "centre"),          # the top edge
    (1, 3, "torus", "plane", (0.5, 0.0), 0, "centre"),            # the right edge
    (1, 4, "halfbox", "plane", (0.0, 0.5), 0, "open"),            # the bottom edge
    (1, 5, "box", "holes", (-0.5, -0.5), 0, "centre"),            # a corner
    (1, 6, "box", "plane", (1.0, 0.1), 0, "centre"),              # wholly in the canvas margin
    (1, 7, "ico1280", "plane", (-1.5, 0.2), 0, "centre"),         # cut by the canvas edge
    (1, 8, "box", "plane", (3.0, 0.0), 0, "centre"),              # wholly off the canvas
    (1, 9, "box", "wall", (0.0, 0.0), 0, "centre"),               # behind an occluder entirely
    (1, 10, "torus", "occluder", (0.0, 0.0), 0, "centre"),        # behind an occluder partly
    (1, 11, "ico1280", "holes", (0.0, 0.0), 0, "centre"),         # zeros are visible, not valid
    (1, 12, "zeroarea", "zeros", (0.0, 0.0), 0, "centre"),        # all-zero depth
    (1, 13, "triangle", "noise", (-0.25, -0.1), 0, "centre"),     # three objects, one depth image
    (1, 13, "box", "noise", (0.1, 0.1), 0, "centre"),
    (1, 13, "ico80", "noise", (0.3, -0.15), 0, "centre"),
    (1, 14, "triangle", "plane", (0.1, 0.1), 0, "pixel"),         # a one-pixel silhouette
    (1, 15, "box", "straddle", (0.0, 0.0), 1, "centre"),          # per-image K; differences straddling delta
    (1, 16, "torus", "noise", (-0.4, 0.3), 2, "centre"),
    (2, 0, "triangle", "plane", (0.0, 0.0), 0, "centre"),
    (2, 1, "ico80", "straddle", (0.5, 0.5), 0, "centre"),
    (3, 0, "ico20480", "noise", (-0.2, 0.0), 0, "centre"),
    (3, 0, "box", "noise", (0.25, 0.05), 0, "centre"),
    (4, 0, "box", "straddle64", (0.0, 0.0), 0, "centre"),         # ... and a few pixels where fp32 and fp64 differences part
    (4, 1, "torus", "occluder", (0.5, -0.1), 0, "centre"),
    (5, 0, "halfbox", "straddle", (-0.1, 0.0), 3, "open"),
]
BEHIND = (1, "box", (0.0, 0.0))                                     # scene, mesh: a vertex at Z <= 0


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def small_rotation(rng, angle):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def draw(case, seed, diam):
    scene, im, mesh, kind, shift, kgroup, place = case
    (W, H), delta, scale = SCENES[scene]
    rng = np.random.default_rng(seed)
    K = LM_K.copy()
    K[:2] *= W / 640.0
    if kgroup:
        K[0, 0] *= 1.0 + 0.03 * kgroup
        K[1, 1] *= 1.0 - 0.02 * kgroup
        K[0, 2] += 1.7 * kgroup
        K[1, 2] -= 0.9 * kgroup
    D = diam[mesh]
    zc = D * K[0, 0] / (0.45 * min(W, H))                    # the object spans about 45 % of the short side
    if place == "pixel":
        zc = D * K[0, 0] / 1.6                               # ... or about a pixel
    R = rotation(rng)
    if place == "open":
        R = small_rotation(rng, 0.3) @ np.array([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]])
    c = np.array([(W / 2 - K[0, 2]) / K[0, 0], (H / 2 - K[1, 2]) / K[1, 1], 1.0]) * zc
    t = c + rng.normal(size=3) * 0.03 * D
    t[0] += shift[0] * W / K[0, 0] * zc
    t[1] += shift[1] * H / K[1, 1] * zc
    return dict(K=K, R=R, t=t, zc=zc, D=D)


def sensor_depth(kind, renders, far, near, delta, rng):
    """the image's depth: a plane behind the objects (at `far`), the objects in front of it, then `kind` (`near`: in front of them all)"""
    plane = np.float32(far)
    t = np.full(renders[0].shape, plane, dtype=np.float32)
    for d in renders:
        t = np.where((d > 0) & (d < t), d, t).astype(np.float32)
    H, W = t.shape
    if kind == "zeros":
        return np.zeros_like(t)
    if kind == "wall":
        t[:] = np.float32(near)
    if kind == "occluder":                                   # a slab in front of the left 45 % of the image
        t[:, :int(0.45 * W)] = np.float32(near)
    if kind == "holes":
        t[rng.random((H, W)) < 0.2] = 0.0
    if kind == "noise":
        t = (t + rng.uniform(-4.0, 4.0, size=(H, W)).astype(np.float32)).astype(np.float32)
        t[rng.random((H, W)) < 0.05] = 0.0
    if kind in ("straddle", "straddle64"):                                   # the sensor sees a surface about delta in front: the test is a coin's toss
        t = (t - np.float32(delta) + rng.uniform(-4.0, 4.0, size=(H, W)).astype(np.float32)).astype(np.float32)
        t[rng.random((H, W)) < 0.05] = 0.0
    return t


class StubRenderer(object):
    """render_object(obj_id, R, t, fx, fy, cx, cy)['depth']: the oracle's float32 depth on the canvas; the frame-sized renderer
    returns the in-frame part of the same canvas render"""
    oracles = {}                                             # (obj, R, t, K) -> oracle_canvas' dict, shared by both scripts
    handed = []                                              # (obj_id, depth) in call order, canvas-sized renders only

    def __init__(self, width, height, meshes, frame):
        self.size, self.meshes, self.frame = (width, height), meshes, frame

    def add_object(self, obj_id, path):
        pass

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        W, H = self.frame
        large = self.size == (3 * W, 3 * H)
        assert large or self.size == (W, H)
        Kc = np.array([[fx, 0.0, cx + (0 if large else W)], [0.0, fy, cy + (0 if large else H)], [0.0, 0.0, 1.0]])       # the canvas's
        key = (obj_id, np.asarray(R).tobytes(), np.asarray(t).tobytes(), Kc.tobytes())
        if key not in StubRenderer.oracles:
            v, f = self.meshes[S.MESH_NAMES[obj_id]]
            StubRenderer.oracles[key] = S.oracle_render(R, np.asarray(t).reshape(3), Kc, v, f, (3 * W, 3 * H))
        d = StubRenderer.oracles[key]["d"]
        if large:
            StubRenderer.handed.append((obj_id, d))
            return {"depth": d}
        return {"depth": np.ascontiguousarray(G.frame_of(d, (W, H)))}


def reset_precomputer():
    misc.Precomputer.xs = misc.Precomputer.ys = misc.Precomputer.pre_Xs = misc.Precomputer.pre_Ys = None
    misc.Precomputer.depth_im_shape = misc.Precomputer.K = None


def run_scripts(scene, scene_gt, scene_camera, stored_depth, meshes):
    """both scripts on one scene -> (scene_gt_info as saved, {(im_id, gt_id): (mask, mask_visib)}, the canvas renders handed in)"""
    (W, H), delta, _ = SCENES[scene]
    saved = {"json": None, "im": {}}
    StubRenderer.handed = []

    def get_split_params(datasets_path, dataset, split, split_type=None):
        sys._getframe(1).f_globals["p"]["delta"] = delta     # the script's own PARAMETERS entry
        return {"im_size": (W, H), "scene_camera_tpath": "camera|{scene_id}", "scene_gt_tpath": "gt|{scene_id}",
                "depth_tpath": "depth|{scene_id}|{im_id}|.tif", "scene_gt_info_tpath": "info|{scene_id}",
                "mask_tpath": "mask|{scene_id}|{im_id}|{gt_id}", "mask_visib_tpath": "mask_visib|{scene_id}|{im_id}|{gt_id}"}

    def load_depth(path):
        reset_precomputer()
        return stored_depth[int(path.split("|")[2])].copy()

    def save_im(path, im):
        kind, _, im_id, gt_id = path.split("|")
        saved["im"][(kind, int(im_id), int(gt_id))] = np.array(im)

    def save_json(path, content):
        saved["json"] = content

    patches = [(dataset_params, "get_split_params", get_split_params),
               (dataset_params, "get_model_params", lambda *a, **k: {"obj_ids": list(range(len(S.MESH_NAMES))), "model_tpath": "{obj_id}"}),
               (dataset_params, "get_present_scene_ids", lambda dp: [scene]),
               (renderer, "create_renderer", lambda w, h, renderer_type="vispy", mode="rgb+depth", **k: StubRenderer(w, h, meshes, (W, H))),
               (inout, "load_scene_gt", lambda path: scene_gt), (inout, "load_scene_camera", lambda path: scene_camera),
               (inout, "load_depth", load_depth), (inout, "save_im", save_im), (inout, "save_json", save_json),
               (misc, "ensure_dir", lambda path: None), (misc, "log", lambda s: None)]
    old = [(m, n, getattr(m, n)) for m, n, _ in patches]
    try:
        for m, n, fn in patches:
            setattr(m, n, fn)
        runpy.run_path(os.path.join(REF, "bop_toolkit", "scripts", "calc_gt_info.py"), run_name="__main__")
        handed = list(StubRenderer.handed)
        runpy.run_path(os.path.join(REF, "bop_toolkit", "scripts", "calc_gt_masks.py"), run_name="__main__")
    finally:
        for m, n, fn in old:
            setattr(m, n, fn)
    masks = {(im, gt): (saved["im"][("mask", im, gt)], saved["im"][("mask_visib", im, gt)]) for kind, im, gt in saved["im"] if kind == "mask"}
    return saved["json"], masks, handed


def tune(depth, large, K, delta, size, want=8):
    """move up to `want` sensor pixels, float by float, to where the reference's fp32 difference and the fp64 difference fall on
    opposite sides of delta -> (depth, the pixels moved)"""
    dg = G.frame_of(large, size)
    depth = depth.copy()
    moved = np.zeros(depth.shape, dtype=bool)
    ys, xs = np.nonzero((dg > 0) & (depth > 0))
    for y, x in zip(ys[::7], xs[::7]):
        if moved.sum() >= want:
            break
        px, py = (x - K[0, 2]) / np.float64(K[0, 0]), (y - K[1, 2]) / np.float64(K[1, 1])
        r = np.sqrt(px * px + py * py + 1.0)
        v = np.float32(dg[y, x] - delta / r)                 # dist_gt - dist_im is about delta here
        cand = [v]
        for _ in range(60):
            cand.append(np.nextafter(cand[-1], np.float32(0)))
        cand = np.asarray(cand, dtype=np.float32)
        t_im = np.sqrt((px * cand) ** 2 + (py * cand) ** 2 + cand.astype(np.float64) ** 2)
        t_gt = np.sqrt((px * dg[y, x]) ** 2 + (py * dg[y, x]) ** 2 + np.float64(dg[y, x]) ** 2)
        d32 = np.float32(t_gt) - t_im.astype(np.float32)
        hit = np.nonzero((d32 <= np.float32(delta)) != (t_gt - t_im <= delta))[0]
        if hit.size:
            depth[y, x] = cand[hit[0]]
            moved[y, x] = True
    assert moved.sum() >= 3, moved.sum()
    return depth, moved


def margin_of(large, depth, K, delta, size, skip=None):
    dg = G.frame_of(large, size)
    t_gt, t_im = S.dist_image(dg, K), S.dist_image(depth, K)
    sel = (t_gt > 0) & (t_im != 0)
    if skip is not None:
        sel &= ~skip
    diff = (t_gt.astype(np.float32) - t_im.astype(np.float32))[sel].astype(np.float64)
    return float(np.abs(diff - delta).min()) / delta if diff.size else np.inf


def main():
    meshes = S.meshes()
    diam = {k: S.diameter(v) for k, (v, f) in meshes.items() if f is not None}
    seeds = [1000 * ci for ci in range(len(CASES))]
    made = {}
    while True:
        poses = [draw(case, seeds[ci], diam) for ci, case in enumerate(CASES)]
        oracles = []
        for ci, (case, pose) in enumerate(zip(CASES, poses)):
            if (ci, seeds[ci]) not in made:
                v, f = meshes[case[2]]
                made[(ci, seeds[ci])] = G.oracle_canvas(pose["R"], pose["t"], pose["K"], v, f, SCENES[case[0]][0])
            oracles.append(made[(ci, seeds[ci])])
        # the images: composited from every ground truth of the image; the kind and the generator are the first entry's
        images, redo, tuned = {}, set(), {}
        for ci, case in enumerate(CASES):
            key = (case[0], case[1])
            if key in images:
                continue
            (W, H), delta, scale = SCENES[case[0]]
            group = [cj for cj, c in enumerate(CASES) if (c[0], c[1]) == key]
            rng = np.random.default_rng(seeds[ci] + 500)
            depth = sensor_depth(case[3], [G.frame_of(oracles[cj]["d"], (W, H)) for cj in group], max(poses[cj]["zc"] + 0.8 * poses[cj]["D"] for cj in group),
                                 min(poses[cj]["zc"] - 0.9 * poses[cj]["D"] for cj in group), delta, rng)
            if case[3] == "straddle64":
                depth, tuned[key] = tune(depth, oracles[ci]["d"], poses[ci]["K"], delta, (W, H))
            images[key] = depth
        for ci, case in enumerate(CASES):
            (W, H), delta, scale = SCENES[case[0]]
            share = S.undecided_share(oracles[ci])
            margin = margin_of(oracles[ci]["d"], images[(case[0], case[1])], poses[ci]["K"], delta, (W, H), tuned.get((case[0], case[1])))
            n_all = int((oracles[ci]["d"] > 0).sum())
            want_pixel = case[6] == "pixel" and not (n_all == 1 and int(oracles[ci]["covered_lo"].sum()) == 1)
            if margin < 1e-6 or share > 0.05 or want_pixel:
                print("case %d: margin %.2e, undecided %.3f, canvas pixels %d -> redrawn" % (ci, margin, share, n_all))
                redo.add(ci)
        if not redo:
            break
        for ci in redo:                                      # (an image's entries are redrawn together: the image is the first one's)
            seeds[ci] += 1

    rec = {k: [] for k in ("R", "t", "K", "mesh", "scene", "image", "W", "H", "delta", "kgroup", "seed", "undecided", "ok") + G.INFO_KEYS}
    out, image_index = {}, {}
    for scene in sorted(SCENES):
        (W, H), delta, scale = SCENES[scene]
        idx = [ci for ci, c in enumerate(CASES) if c[0] == scene]
        im_ids = sorted({CASES[ci][1] for ci in idx})
        # bop_toolkit's own im_id / gt_id numbering: im_id = 100 * image (so that calc_gt_masks' log line fires too)
        scene_gt = {100 * im: [{"obj_id": S.MESH_NAMES.index(CASES[ci][2]), "cam_R_m2c": poses[ci]["R"].copy(),
                                "cam_t_m2c": poses[ci]["t"].reshape(3, 1).copy()} for ci in idx if CASES[ci][1] == im] for im in im_ids}
        first = {im: [ci for ci in idx if CASES[ci][1] == im][0] for im in im_ids}
        scene_camera = {100 * im: {"cam_K": poses[first[im]]["K"].copy(), "depth_scale": scale} for im in im_ids}
        for im in im_ids:                                    # one K per image: every entry of an image was drawn with it
            assert all(np.array_equal(poses[ci]["K"], poses[first[im]]["K"]) for ci in idx if CASES[ci][1] == im)
        stored = {100 * im: (images[(scene, im)] / np.float32(scale)).astype(np.float32) for im in im_ids}
        for im in im_ids:
            assert np.array_equal(stored[100 * im] * np.float32(scale), images[(scene, im)])
        info, masks, handed = run_scripts(scene, scene_gt, scene_camera, stored, meshes)
        n = 0
        for im in im_ids:
            image_index[(scene, im)] = len(image_index)
            out["depth_%d" % image_index[(scene, im)]] = images[(scene, im)]
            for gt_id, ci in enumerate([c for c in idx if CASES[c][1] == im]):
                e = info[100 * im][gt_id]
                mask, mask_visib = masks[(100 * im, gt_id)]
                obj, large = handed[n]
                n += 1
                assert obj == S.MESH_NAMES.index(CASES[ci][2]) and np.array_equal(large, oracles[ci]["d"]) and large.dtype == np.float32
                assert mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 255} and set(np.unique(mask_visib)) <= {0, 255}
                assert int((mask_visib > 0).sum()) == e["px_count_visib"] and all(type(e[k]) is int for k in G.INFO_KEYS[:3])
                mine = G.count(large, images[(scene, im)], poses[ci]["K"], delta)
                assert G.same_info(mine, e) and np.array_equal(mine["mask"], mask > 0) and np.array_equal(mine["mask_visib"], mask_visib > 0), ci
                for k in G.INFO_KEYS:
                    rec[k].append(e[k])
                for k, val in (("R", poses[ci]["R"]), ("t", poses[ci]["t"]), ("K", poses[ci]["K"]), ("mesh", S.MESH_NAMES.index(CASES[ci][2])),
                               ("scene", scene), ("image", image_index[(scene, im)]), ("W", W), ("H", H), ("delta", float(delta)),
                               ("kgroup", CASES[ci][5]), ("seed", seeds[ci]), ("undecided", S.undecided_share(oracles[ci])), ("ok", True)):
                    rec[k].append(val)
                c = len(rec["ok"]) - 1
                out["large_%d" % c], out["mask_%d" % c], out["visib_%d" % c] = large, G.pack(mask > 0), G.pack(mask_visib > 0)
                print("case %2d scene %d im %2d %-9s %-8s all %5d valid %5d visib %5d fract %.4f obj %s visib %s undecided %.4f"
                      % (c, scene, im, CASES[ci][2], CASES[ci][3], e["px_count_all"], e["px_count_valid"], e["px_count_visib"], e["visib_fract"],
                         e["bbox_obj"], e["bbox_visib"], rec["undecided"][-1]))
    # the pose with a vertex behind the camera: the project's rule, not the scripts'
    scene, mesh, shift = BEHIND
    pose = draw((scene, 0, mesh, "plane", shift, 0, "centre"), 77, diam)
    pose["t"][2] = 10.0
    u, v, Z, _ = S.screen(pose["R"], pose["t"], pose["K"], meshes[mesh][0])
    assert (Z <= 0).any() and (Z > 0).any()
    (W, H), delta, _ = SCENES[scene]
    for k, val in (("R", pose["R"]), ("t", pose["t"]), ("K", pose["K"]), ("mesh", S.MESH_NAMES.index(mesh)), ("scene", scene),
                   ("image", image_index[(scene, 0)]), ("W", W), ("H", H), ("delta", float(delta)), ("kgroup", 0), ("seed", 77), ("undecided", 0.0),
                   ("ok", False), ("px_count_all", 0), ("px_count_valid", 0), ("px_count_visib", 0), ("visib_fract", 0.0),
                   ("bbox_obj", [-1] * 4), ("bbox_visib", [-1] * 4)):
        rec[k].append(val)
    out.update({k: np.asarray(v) for k, v in rec.items()})
    out["mesh_names"] = np.asarray(S.MESH_NAMES)
    out["mesh_crc"] = np.asarray([zlib.crc32(meshes[k][0].tobytes() + meshes[k][1].tobytes()) if meshes[k][1] is not None else 0
                                  for k in S.MESH_NAMES], dtype=np.int64)
    out["worst_undecided"] = np.float64(max(rec["undecided"]))
    path = os.path.join(HERE, "gt_info.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes), %d cases, worst undecided share %.4f" % (path, os.path.getsize(path), len(rec["ok"]), max(rec["undecided"])))
    assert os.path.getsize(path) < 500000


if __name__ == "__main__":
    main()
