"""The tile-raster scaffold that rows N8, N10, N12 and N14 share (csrc/vsd_raster.h), through all four entry points on ONE small scene:
a shared helper that is wrong for one of its callers shows here as a disagreement between them.

  mesh    the first 257 faces of vsd_stages' "ico1280": one full chunk of 256 triangles plus one; an open surface (no culling)
  frame   45 x 37: a 2 x 2 tile grid with partial tiles on both axes
  batch   an ordinary pose whose silhouette meets all four tiles, one whose silhouette crosses the frame's left and top edge, and
          one with vertices behind the camera (not rendered)

With d = render_depth(...): gt_info's depth and render_rgb's (ssaa = 1) are d's bits, render_rgb's mask is 255 * (d > 0), mask_errors
(est = gt) returns d > 0 on both sides and cus == 0; the third pose is not-ok / NaN everywhere and leaves its neighbours' results equal
to a B = 2 call without it; d passes the interval check of the float64 oracle rasteriser (tests/vsd_stages.py)."""
import numpy as np
import pytest
import torch

from tests import vsd_stages as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = (45, 37)                                                  # (W, H)
K = np.array([[150.0, 0.0, 22.3], [0.0, 148.0, 18.9], [0.0, 0.0, 1.0]])
_SHARED = {}


def _rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    k = w / th
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)


def _scene():
    v, f = S.meshes()["ico1280"]
    f = np.ascontiguousarray(f[:257])
    R = np.stack([_rodrigues([0.3, -1.9, 0.4]), _rodrigues([1.1, 0.5, -0.7]), _rodrigues([0.2, 0.1, 0.3])])
    t = np.array([[18.0, -2.0, 440.0], [-50.0, -38.0, 330.0], [5.0, -4.0, 30.0]])
    return v, f, R, t


def _run(n):
    """the four rows on the first n poses, once, shared: name -> numpy array"""
    if n not in _SHARED:
        from checkerpose_amd import gt_info, metric, render
        v, f, R, t = _scene()
        ms = metric.MeshSet.from_arrays([v], faces=[f], diameters=[100.0])
        Rd, td = torch.from_numpy(R[:n]).to(DEV), torch.from_numpy(t[:n, :, None]).to(DEV)
        sensor = np.full((SIZE[1], SIZE[0]), 400.0, dtype=np.float32)
        out = {"d": metric.render_depth(Rd, td, K, ms, SIZE)}
        for k, a in gt_info.gt_info(Rd, td, K, ms, sensor, return_masks=True, return_depth=True).items():
            out["gi_" + k] = a
        for k, a in render.render_rgb(Rd, td, K, ms, SIZE, shading="flat", ssaa=1, return_depth=True, return_mask=True, return_boxes=True).items():
            out["rr_" + k] = a
        for k, a in metric.mask_errors(Rd, td, Rd, td, K, ms, SIZE, return_counts=True, return_boxes=True, return_masks=True).items():
            out["me_" + k] = a
        _SHARED[n] = {k: a.cpu().numpy() for k, a in out.items()}
    return _SHARED[n]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_the_scene_is_what_the_docstring_says():
    v, f, R, t = _scene()
    assert f.shape == (257, 3)
    cov = [S.oracle_render(R[b], t[b], K, v, f, SIZE)["d"] > 0 for b in range(2)]
    assert all(c.any() for c in (cov[0][:32, :32], cov[0][:32, 32:], cov[0][32:, :32], cov[0][32:, 32:]))
    assert not (cov[0][0].any() or cov[0][-1].any() or cov[0][:, 0].any() or cov[0][:, -1].any())
    assert cov[1][:, 0].any() and cov[1][0].any()
    assert (S.screen(R[2], t[2], K, v)[2] <= 0).any()


def test_the_four_rows_render_the_same_depth_and_silhouette():
    r = _run(3)
    d = r["d"]
    assert d.shape == (3, SIZE[1], SIZE[0]) and d.dtype == np.float32
    assert (d[0] > 0).any() and (d[1] > 0).any()
    assert np.array_equal(_bits(r["gi_depth"]), _bits(d))
    assert np.array_equal(_bits(r["rr_depth"]), _bits(d))
    assert np.array_equal(r["rr_mask"], 255 * (d > 0).astype(np.uint8))
    assert np.array_equal(r["me_masks"][:, 0], d > 0) and np.array_equal(r["me_masks"][:, 1], d > 0)
    assert np.array_equal(r["me_cus"][:2], np.zeros(2))
    n = (d > 0).reshape(3, -1).sum(1)
    assert np.array_equal(r["me_counts"], np.stack([n, n, n, n], 1))


def test_a_pose_behind_the_camera_is_refused_and_leaves_its_neighbours_alone():
    r, two = _run(3), _run(2)
    assert not r["d"][2].any()
    assert not r["gi_ok"][2] and r["gi_ok"][:2].all()
    assert not r["rr_ok"][2] and r["rr_ok"][:2].all()
    assert not r["me_ok"][2] and r["me_ok"][:2].all()
    assert np.isnan(r["me_cus"][2]) and np.isnan(r["me_cou_bb_proj"][2])
    assert not r["gi_depth"][2].any() and not r["rr_mask"][2].any() and not r["me_masks"][2].any()
    assert set(two) == set(r)
    for k in r:
        assert np.array_equal(_bits(r[k][:2]), _bits(two[k])), k


def test_the_depth_passes_the_oracle_interval_check():
    v, f, R, t = _scene()
    d = _run(3)["d"]
    for b in range(2):
        ok, ratio, nbad = S.check_render(d[b], S.oracle_render(R[b], t[b], K, v, f, SIZE))
        print("pose %d worst |diff| / tol_d on decided pixels %.4f, pixels outside their interval %d" % (b, ratio, nbad))
        assert ok, (b, ratio, nbad)
