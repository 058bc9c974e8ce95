#!/usr/bin/env python3
"""Fixture of the self-occlusion measure (cp_hpr_visibility): tests/golden/visibility.npz.

Runs ONLY where the reference tree is (CHECKERPOSE_REFERENCE, default /root/reference; nothing of it travels, only the recorded
results) and where scipy is installed:

  python tests/golden/make_golden_visibility.py

`compute_vis_hpr` and `transform_pts_Rt` are compiled from checkerpose/preprocess_data/get_overall_visibility.py with `ast` (the
script's top level parses arguments and imports mmcv) and run with scipy.spatial.ConvexHull (qhull): every recorded mask is what the
REFERENCE's own function returned for the REFERENCE's own transform of the cloud.  Clouds and views are regenerated from seeds
(tests/visibility_stages.py), not stored.  Per case:
  mask__<name>    (n_views, V) uint8
  crc__<name>     CRC-32 of the cloud's, the rotations' and the translations' float64 bytes
  margin__<name>  the smallest decision margin over the case's views, in cloud units: for a point that is not a hull vertex its
                  depth below the hull (from hull.equations); for a hull vertex its distance outside the hull of the OTHER points.
                  The maker REFUSES a case whose margin is under 1e-6: three orders above fp64 noise on a plane value at coordinates
                  of 1e5, so a recorded cell never hinges on rounding or on qhull's merging.  A condition of the fixture, not a
                  tolerance of the tests.
  mean__<name>, stat__<name>   the script's statistic over the case's views (lines 113-122): mean (V,), then [min, max, below x 9]"""
import ast
import os
import sys

import numpy as np
from scipy.spatial import ConvexHull

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

from tests import visibility_stages as S  # noqa: E402


def reference_pieces():
    rel = os.path.join("checkerpose", "preprocess_data", "get_overall_visibility.py")
    tree = ast.parse(open(os.path.join(REF, rel)).read())
    want = ["compute_vis_hpr", "transform_pts_Rt"]
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert sorted(f.name for f in fns) == sorted(want)
    ns = {"np": np, "ConvexHull": ConvexHull}
    exec(compile(ast.Module(body=fns, type_ignores=[]), rel, "exec"), ns)
    return ns["compute_vis_hpr"], ns["transform_pts_Rt"]


def margin(P, vis):
    """P (N,3): the flipped points with the viewpoint in row 0; vis (N,) the hull's vertex flags -> the smallest decision margin"""
    hull = ConvexHull(P)
    flags = np.zeros(P.shape[0], dtype=bool)
    flags[hull.vertices] = True
    assert np.array_equal(flags, vis)
    eq = hull.equations
    depth = -(P @ eq[:, :3].T + eq[:, 3]).max(axis=1)                  # >= 0 for every point; the depth of the non-vertices
    worst = depth[~flags].min() if (~flags).any() else np.inf
    for i in np.nonzero(flags)[0]:
        rest = np.delete(P, i, axis=0)
        if rest.shape[0] < 4:
            continue
        e = ConvexHull(rest).equations
        worst = min(worst, (e[:, :3] @ P[i] + e[:, 3]).max())
    return worst


def main():
    compute_vis_hpr, transform_pts_Rt = reference_pieces()
    out = {}
    for name in S.names():
        c = S.CASES[name]
        pts = S.cloud(name)
        R, t = S.views(name)
        assert pts.shape == (c["V"], 3) and pts.dtype == np.float64
        mask = np.zeros((c["n_views"], c["V"]), dtype=np.uint8)
        worst = np.inf
        for k in range(c["n_views"]):
            tk = S.view_t(t, k)
            cam = transform_pts_Rt(pts, R[k], tk.reshape((3, 1)))
            vis = compute_vis_hpr(cam, radius_param=c["radius_param"])
            assert vis.shape == (c["V"],) and vis.dtype == np.float64 and np.isin(vis, (0.0, 1.0)).all()
            mask[k] = vis.astype(np.uint8)
            P = S.flip(pts, R[k], tk, c["radius_param"])
            flags = np.concatenate([[True], vis > 0])                  # (the viewpoint is a hull vertex: margin() asserts it)
            worst = min(worst, margin(P, flags))
        if not worst >= S.MARGIN_FLOOR:
            raise SystemExit("%s: decision margin %.3e is under the floor %.1e -- change the case's seed" % (name, worst, S.MARGIN_FLOOR))
        mean, lo, hi, below = S.statistic(mask.sum(axis=0, dtype=np.int64), c["n_views"])
        out["mask__" + name] = mask
        out["crc__" + name] = np.uint32(S.crc(pts, R, t))
        out["margin__" + name] = np.float64(worst)
        out["mean__" + name] = mean
        out["stat__" + name] = np.concatenate([[lo, hi], below])
        print("%-20s V=%5d views=%2d visible %5.1f%%  margin %.3e" % (name, c["V"], c["n_views"], 100.0 * mask.mean(), worst), flush=True)
    np.savez_compressed(S.GOLDEN, **out)
    print("wrote", S.GOLDEN, os.path.getsize(S.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
