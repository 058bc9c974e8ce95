#!/usr/bin/env python3
"""Row N8 (BOP's VSD) pinned by the REFERENCE's own code after the render.

Runs ONLY where the reference tree is (CHECKERPOSE_REFERENCE, default /root/reference; nothing of it travels, only the recorded
numbers in vsd.npz are committed):

  python tests/golden/make_golden_vsd.py

The reference's renderers (vispy / glumpy / OpenGL / bop_renderer) run nowhere this project runs, so `pose_error.vsd`
(pose_error.py:17-93) is called with a STUB renderer whose render_object(...)['depth'] returns the float32 depth of
tests/vsd_stages.oracle_render -- the render rule stated in float64.  Everything after the render is then the reference's own:
misc.depth_im_to_dist_im_fast (with its Precomputer cache, reset before every case; the whole list is evaluated a second time in
reverse order and must give the same numbers), visibility.estimate_visib_mask_gt / _est, the counting and the quotients.  The
counts the reference does not return (union, inter, cost per tau) are taken with the same functions.  misc.overlapping_sphere_projections
gives the sphere bit.

Cases (tests/vsd_stages.meshes for the meshes; "hull" is scipy's ConvexHull of checkerpose_amd/data/fps_lmo_obj01.npy, its faces are
recorded): see CASES.  Test depth = the ground truth's render over a plane behind it, optionally with an occluder in front of part
of it, holes of 0, all zeros, and +- a few mm of noise.  Every recorded decision (the fp32 difference against delta, |dist_gt -
dist_est| (/ diameter) against every tau) lies at least 1e-6 (relative) from its boundary: a case that does not is redrawn with the
next seed."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "bop_toolkit"))
sys.path.insert(0, ROOT)

from bop_toolkit_lib import misc, pose_error, visibility  # noqa: E402
from tests import vsd_stages as S  # noqa: E402

LM_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
TAUS = np.arange(0.05, 0.51, 0.05)

# (mesh, (W, H), est offset as a fraction of the diameter, test depth kind, delta, normalized, placement, K group)
CASES = [
    ("triangle", (33, 31), 0.0, "plane", 15, True, "centre", 0),
    ("triangle", (67, 45), 0.10, "plane", 5, True, "centre", 0),
    ("box", (67, 45), 0.0, "plane", 15, True, "centre", 0),
    ("box", (67, 45), 0.02, "occluder", 15, True, "centre", 0),
    ("box", (160, 120), 0.10, "noise", 15, True, "centre", 0),
    ("box", (67, 45), 0.40, "holes", 15, True, "centre", 0),
    ("halfbox", (67, 45), 0.02, "plane", 15, True, "open", 0),
    ("halfbox", (96, 80), 0.10, "noise", 15, False, "open", 0),
    ("ico80", (33, 31), 0.10, "plane", 15, True, "centre", 0),
    ("ico1280", (67, 45), 0.02, "zeros", 15, True, "centre", 0),
    ("ico1280", (96, 80), 0.40, "occluder", 15, True, "centre", 0),
    ("ico20480", (160, 120), 0.02, "noise", 15, True, "centre", 0),
    ("torus", (67, 45), 0.0, "occluder", 15, True, "centre", 0),
    ("torus", (96, 80), 0.10, "noise", 5, True, "centre", 0),
    ("hull", (67, 45), 0.02, "plane", 15, True, "centre", 0),
    ("hull", (67, 45), 0.10, "holes", 5, False, "centre", 0),
    ("zeroarea", (67, 45), 0.02, "plane", 15, True, "centre", 0),
    ("box", (67, 45), 0.10, "plane", 15, True, "partly", 0),
    ("box", (67, 45), 0.02, "plane", 15, True, "outside", 0),
    ("ico80", (67, 45), 0.0, "plane", 15, True, "disjoint", 0),
    ("box", (67, 45), 0.0, "plane", 15, True, "far", 0),
    ("box", (67, 45), 0.02, "noise", 15, True, "centre", 1),
    ("torus", (67, 45), 0.10, "plane", 15, True, "centre", 2),
    ("ico80", (67, 45), 0.40, "occluder", 15, True, "centre", 3),
]


class StubRenderer(object):
    """render_object(obj_id, R, t, fx, fy, cx, cy)['depth'] = the oracle's float32 depth of mesh `obj_id`"""

    def __init__(self, meshes, size):
        self.meshes, self.size, self.made = meshes, size, []

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        v, f = self.meshes[obj_id]
        K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        d = S.oracle_render(R, t, K, v, f, self.size)["d"]
        self.made.append(d)
        return {"depth": d}


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


def draw(case, seed, meshes, diam):
    mesh, size, frac, kind, delta, norm, place, kgroup = case
    rng = np.random.default_rng(seed)
    W, H = size
    K = LM_K.copy()
    K[:2] *= W / 640.0
    if kgroup:
        K[0, 0] *= 1.0 + 0.03 * kgroup
        K[1, 1] *= 1.0 - 0.02 * kgroup
        K[0, 2] += 1.7 * kgroup
        K[1, 2] -= 0.9 * kgroup
    D = diam[mesh]
    zc = D * K[0, 0] / (0.45 * min(W, H))                    # the object spans about 45 % of the short side
    R_gt = rotation(rng)
    if place == "open":                                      # the half box's missing +y / +z faces towards the camera: inner faces show
        R_gt = small_rotation(rng, 0.3) @ np.array([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]])
    c = np.array([(W / 2 - K[0, 2]) / K[0, 0], (H / 2 - K[1, 2]) / K[1, 1], 1.0]) * zc
    t_gt = c + rng.normal(size=3) * 0.03 * D
    if place == "partly":
        t_gt[0] -= 0.5 * W / K[0, 0] * zc
    if place == "outside":
        t_gt[0] += 2.0 * W / K[0, 0] * zc
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    R_est = small_rotation(rng, 2.0 * frac) @ R_gt if frac else R_gt.copy()
    t_est = t_gt + frac * D * d
    if place == "disjoint":                                  # both inside the frame, the rectangles apart
        t_gt[0] -= 0.27 * W / K[0, 0] * zc
        t_est = t_gt.copy()
        t_est[0] += 0.55 * W / K[0, 0] * zc
    if place == "far":                                       # the sphere projections do not overlap
        t_est = t_gt.copy()
        t_est[0] += 0.6 * W / K[0, 0] * zc
        t_est[2] *= 1.5
    return dict(K=K, R_gt=R_gt, t_gt=t_gt, R_est=R_est, t_est=t_est, rng=rng, zc=zc)


def test_depth(kind, d_gt, zc, D, rng):
    H, W = d_gt.shape
    plane = np.float32(zc + 0.8 * D)
    t = np.where(d_gt > 0, d_gt, plane).astype(np.float32)
    if kind == "zeros":
        return np.zeros_like(t)
    if kind == "occluder":                                   # a slab in front of the left 40 % of the image
        t[:, :int(0.4 * W)] = np.float32(zc - 0.9 * D)
    if kind == "holes":
        t[rng.random((H, W)) < 0.2] = 0.0
    if kind == "noise":
        t = (t + rng.uniform(-4.0, 4.0, size=(H, W)).astype(np.float32)).astype(np.float32)
        t[rng.random((H, W)) < 0.05] = 0.0
    return t


def reference_counts(depth_test, d_est, d_gt, K, delta, taus, norm, D):
    """the counts pose_error.vsd forms, with the reference's own functions; and the smallest relative margin of its decisions"""
    dist_test = misc.depth_im_to_dist_im_fast(depth_test, K)
    dist_gt = misc.depth_im_to_dist_im_fast(d_gt, K)
    dist_est = misc.depth_im_to_dist_im_fast(d_est, K)
    vg = visibility.estimate_visib_mask_gt(dist_test, dist_gt, delta, visib_mode="bop19")
    ve = visibility.estimate_visib_mask_est(dist_test, dist_est, vg, delta, visib_mode="bop19")
    inter, union = np.logical_and(vg, ve), np.logical_or(vg, ve)
    dists = np.abs(dist_gt[inter] - dist_est[inter])
    if norm:
        dists /= D
    counts = [int(union.sum()), int(inter.sum())] + [int((dists >= tau).sum()) for tau in taus]
    margin = np.inf
    for dm in (dist_gt, dist_est):
        sel = (dm > 0) & (dist_test != 0)
        diff = (dm.astype(np.float32) - dist_test.astype(np.float32))[sel].astype(np.float64)
        if diff.size:
            margin = min(margin, float(np.abs(diff - delta).min()) / delta)
    for tau in taus:
        if dists.size:
            margin = min(margin, float(np.abs(dists - tau).min()) / tau)
    return np.array(counts, dtype=np.int64), margin


def reset_precomputer():
    misc.Precomputer.xs = misc.Precomputer.ys = misc.Precomputer.pre_Xs = misc.Precomputer.pre_Ys = None
    misc.Precomputer.depth_im_shape = misc.Precomputer.K = None


def evaluate(case, pose, depth, meshes, diam):
    mesh, size, frac, kind, delta, norm, place, kgroup = case
    reset_precomputer()
    stub = StubRenderer(meshes, size)
    e = pose_error.vsd(pose["R_est"], pose["t_est"].reshape(3, 1), pose["R_gt"], pose["t_gt"].reshape(3, 1), depth, pose["K"], delta,
                       list(TAUS), norm, diam[mesh], stub, mesh, "step")
    d_est, d_gt = stub.made
    counts, margin = reference_counts(depth, d_est, d_gt, pose["K"], delta, TAUS, norm, diam[mesh])
    return np.asarray(e, dtype=np.float64), counts, margin, d_est, d_gt


def main():
    from scipy.spatial import ConvexHull
    pts = np.load(os.path.join(ROOT, "checkerpose_amd", "data", "fps_lmo_obj01.npy")).reshape(-1, 3)
    hull_faces = np.sort(ConvexHull(pts).simplices.astype(np.int32), axis=1)
    hull_faces = hull_faces[np.lexsort(hull_faces.T[::-1])]
    meshes = S.meshes(hull_faces)
    diam = {k: S.diameter(v) for k, (v, f) in meshes.items()}
    rec = {k: [] for k in ("R_est", "t_est", "R_gt", "t_gt", "K", "mesh", "W", "H", "delta", "norm", "kgroup", "errors", "counts", "sphere",
                           "seed", "undecided")}
    images, poses = [], []
    for ci, case in enumerate(CASES):
        mesh, size, frac, kind, delta, norm, place, kgroup = case
        seed = 1000 * ci
        while True:
            pose = draw(case, seed, meshes, diam)
            v, f = meshes[mesh]
            o_gt = S.oracle_render(pose["R_gt"], pose["t_gt"], pose["K"], v, f, size)
            o_est = S.oracle_render(pose["R_est"], pose["t_est"], pose["K"], v, f, size)
            depth = test_depth(kind, o_gt["d"], pose["zc"], diam[mesh], pose["rng"])
            e, counts, margin, d_est, d_gt = evaluate(case, pose, depth, meshes, diam)
            share = max(S.undecided_share(o_gt), S.undecided_share(o_est))
            if margin >= 1e-6 and share <= 0.05:
                break
            print("case %d: margin %.2e, undecided %.3f -> redrawn" % (ci, margin, share))
            seed += 1
        assert np.array_equal(d_est, o_est["d"]) and np.array_equal(d_gt, o_gt["d"])
        assert np.array_equal(e, S.errors_of(counts)), (ci, e, counts)
        sphere = bool(misc.overlapping_sphere_projections(0.5 * diam[mesh], pose["t_est"], pose["t_gt"]))
        for k in ("R_est", "t_est", "R_gt", "t_gt", "K"):
            rec[k].append(pose[k])
        for k, val in (("mesh", S.MESH_NAMES.index(mesh)), ("W", size[0]), ("H", size[1]), ("delta", float(delta)), ("norm", bool(norm)),
                       ("kgroup", kgroup), ("errors", e), ("counts", counts), ("sphere", sphere), ("seed", seed), ("undecided", share)):
            rec[k].append(val)
        images.append((depth, d_est, d_gt))
        poses.append(pose)
        print("case %2d %-9s %3dx%-3d %-8s union %5d inter %5d cost %s  e[0] %.4f e[9] %.4f sphere %d margin %.1e undecided %.4f"
              % (ci, mesh, size[0], size[1], kind, counts[0], counts[1], counts[2:].tolist(), e[0], e[9], sphere, margin, share))
    # the recorded values must not depend on the order of the cases (Precomputer's cache across K and shape changes)
    for ci in reversed(range(len(CASES))):
        e, counts, _, _, _ = evaluate(CASES[ci], poses[ci], images[ci][0], meshes, diam)
        assert np.array_equal(e, rec["errors"][ci]) and np.array_equal(counts, rec["counts"][ci]), ci
    out = {k: np.asarray(v) for k, v in rec.items()}
    out["taus"] = TAUS
    out["hull_faces"] = hull_faces.astype(np.int16)
    out["mesh_names"] = np.asarray(S.MESH_NAMES)
    out["mesh_diameter"] = np.asarray([diam[k] for k in S.MESH_NAMES])
    for ci, (depth, d_est, d_gt) in enumerate(images):
        out["test_%d" % ci], out["est_%d" % ci], out["gt_%d" % ci] = depth, d_est, d_gt
    path = os.path.join(HERE, "vsd.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
