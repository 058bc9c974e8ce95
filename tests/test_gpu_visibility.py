"""Row N16 on the device: cp_hpr_visibility and checkerpose_amd.visibility against what the reference's own compute_vis_hpr returned with
qhull (tests/golden/visibility.npz, tests/golden/make_golden_visibility.py).  Nothing here has a tolerance: every recorded mask is
EQUAL, counts are the masks' column sums, every status is 0, and the outputs do not depend on the call, the batch, the order of the
views or the number of workgroups."""
import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, render, visibility
from tests import visibility_stages as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g():
    return np.load(S.GOLDEN)


@pytest.fixture(scope="module")
def device_results():
    """every case through ONE hpr_visibility call: name -> (counts (V,), mask (n_views,V)) on the host"""
    out = {}
    for name in S.names():
        R, t = S.views(name)
        counts, mask = visibility.hpr_visibility(S.cloud(name), R, t, S.CASES[name]["radius_param"], DEV, return_mask=True)
        assert counts.dtype == torch.int32 and mask.dtype == torch.uint8 and counts.is_cuda and mask.is_cuda
        out[name] = (counts.cpu().numpy(), mask.cpu().numpy())
    return out


@pytest.mark.parametrize("name", S.names())
def test_every_recorded_mask_is_equal_and_counts_are_the_column_sums(g, device_results, name):
    counts, mask = device_results[name]
    ref = g["mask__" + name]
    wrong = int((mask != ref).sum())
    print("%-20s V=%5d views=%2d cells differing: %d of %d" % (name, ref.shape[1], ref.shape[0], wrong, ref.size))
    assert mask.shape == ref.shape and wrong == 0, (name, wrong)
    assert np.array_equal(counts, ref.sum(axis=0, dtype=np.int64)), name


def test_every_status_is_zero_and_the_mask_is_optional(g, device_results):
    lib = _abi.load()
    dev = torch.device(DEV)
    for name in ("sphere_v2000", "box_v4", "torus_v300_tview"):
        pts, (R, t) = S.cloud(name), S.views(name)
        n, V = R.shape[0], pts.shape[0]
        d_pts, d_R, d_t = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pts, R, t))
        counts = torch.full((V,), -7, dtype=torch.int32, device=dev)                      # the call zeroes counts itself
        status = torch.full((n,), -7, dtype=torch.int32, device=dev)
        scratch = torch.empty(lib.cp_hpr_visibility_scratch_bytes(n, V, 0), dtype=torch.uint8, device=dev)
        lib.cp_kernel_log_begin()
        with torch.cuda.device(dev):
            rc = lib.cp_hpr_visibility(torch.cuda.current_stream(dev).cuda_stream, d_pts.data_ptr(), d_R.data_ptr(), d_t.data_ptr(),
                                       0 if t.ndim == 1 else 3, n, V, S.CASES[name]["radius_param"], 0, counts.data_ptr(), None,
                                       status.data_ptr(), scratch.data_ptr())
        assert rc == 0 and lib.cp_kernel_log().decode() == "hpr_visibility_kernel"
        assert status.cpu().tolist() == [0] * n, name
        assert np.array_equal(counts.cpu().numpy(), device_results[name][0]), name


def test_compute_vis_hpr_on_single_views_matches_the_recorded_arrays(g):
    for name, ks in (("sphere_v300", (0, 7)), ("torus_v65", (3,)), ("tetra_centroid_v5", (0, 15)), ("sphere_v300_r15", (5,)),
                     ("torus_v300_tview", (2,))):
        pts, (R, t) = S.cloud(name), S.views(name)
        for k in ks:
            cam = (R[k].dot(pts.T) + S.view_t(t, k).reshape((3, 1))).T                     # the reference's transform_pts_Rt
            vis = visibility.compute_vis_hpr(cam, radius_param=S.CASES[name]["radius_param"], device=DEV)
            assert type(vis) is np.ndarray and vis.dtype == np.float64 and vis.shape == (pts.shape[0],)
            assert np.array_equal(vis, g["mask__" + name][k].astype(np.float64)), (name, k)
    pts, (R, t) = S.cloud("box_v64"), S.views("box_v64")
    cam = (R[1].dot(pts.T) + t.reshape((3, 1))).T
    eye = np.array([12.5, -40.0, 3.0])
    assert np.array_equal(visibility.compute_vis_hpr(cam + eye, viewpoint=eye, device=DEV), g["mask__box_v64"][1].astype(np.float64))


def test_overall_visibility_matches_the_recorded_statistic(g):
    for name in ("sphere_v300", "box_v65", "torus_v300_tview"):
        R, t = S.views(name)
        out = visibility.overall_visibility(S.cloud(name), R, t, device=DEV)
        assert sorted(out) == ["below", "max", "mean", "min", "n_views"] and out["n_views"] == 16
        assert out["mean"].dtype == np.float64 and np.array_equal(out["mean"], g["mean__" + name]), name
        assert np.array_equal(np.concatenate([[out["min"], out["max"]], out["below"]]), g["stat__" + name]), name
    pts = S.cloud("sphere_v65")                                                           # R=None: the rotations of sample_views
    out = visibility.overall_visibility(pts, min_n_views=12, device=DEV)
    views, _ = render.sample_views(12)
    Rs = np.stack([v["R"] for v in views])
    counts = visibility.hpr_visibility(pts, Rs, device=DEV).cpu().numpy()
    assert out["n_views"] == len(views) == 12 and np.array_equal(out["mean"], counts / 12)
    assert 0.0 <= out["min"] <= out["max"] <= 1.0 and out["below"].shape == (9,) and (np.diff(out["below"]) >= 0).all()


def test_outputs_are_bitwise_the_same_across_calls_batches_orders_and_workgroups(device_results):
    for name in ("sphere_v300", "torus_v300_tview", "sphere_v2000", "box_v5"):
        pts, (R, t), rp = S.cloud(name), S.views(name), S.CASES[name]["radius_param"]
        counts, mask = device_results[name]
        n = R.shape[0]
        c2, m2 = visibility.hpr_visibility(pts, R, t, rp, DEV, return_mask=True)          # two calls
        assert np.array_equal(c2.cpu().numpy(), counts) and np.array_equal(m2.cpu().numpy(), mask), name
        k = n - 2                                                                         # a view alone against the same view in its batch
        c1, m1 = visibility.hpr_visibility(pts, R[k:k + 1], S.view_t(t, k), rp, DEV, return_mask=True)
        assert np.array_equal(m1.cpu().numpy()[0], mask[k]) and np.array_equal(c1.cpu().numpy(), mask[k].astype(np.int32)), name
        perm = np.random.default_rng(5).permutation(n)                                    # views in shuffled order: the permuted mask
        cp, mp = visibility.hpr_visibility(pts, R[perm], t if t.ndim == 1 else t[perm], rp, DEV, return_mask=True)
        assert np.array_equal(mp.cpu().numpy(), mask[perm]) and np.array_equal(cp.cpu().numpy(), counts), name
        for wg in (1, 3, 64):
            cw, mw = visibility.hpr_visibility(pts, R, t, rp, DEV, return_mask=True, _workgroups=wg)
            assert np.array_equal(cw.cpu().numpy(), counts) and np.array_equal(mw.cpu().numpy(), mask), (name, wg)


def test_four_coincident_points_raise_with_status_1():
    with pytest.raises(RuntimeError, match="view 0 failed with status 1"):
        visibility.hpr_visibility(np.ones((4, 3)), np.eye(3)[None], device=DEV)
    with pytest.raises(RuntimeError, match="status 1"):
        visibility.compute_vis_hpr(np.full((4, 3), 25.0), device=DEV)
    R = np.stack([np.eye(3), np.zeros((3, 3)), np.zeros((3, 3))])                         # the FIRST failing view is named
    with pytest.raises(RuntimeError, match="view 1 failed with status 1.*2 of 3 views"):  # (R = 0 sends every point to t)
        visibility.hpr_visibility(S.cloud("tetra_v4"), R, device=DEV)
