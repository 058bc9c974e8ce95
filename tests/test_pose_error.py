"""Row N5 (pose errors: ADD / ADD-S, pass rates, AUC), host side.  tests/golden/pose_error.npz holds what the REFERENCE's own
bop_toolkit_lib.pose_error.add / .adi, misc.calc_pts_diameter and test.py's compute_auc_posecnn returned (make_golden_pose_error.py);
the numpy + cKDTree restatement below -- the yardstick of tests/test_gpu_pose_error.py, which cannot read the reference -- reproduces
those numbers, and so do the package's host functions (diameter, AUC, summarize).  cp_pose_errors' argument checks return before any
launch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, metric
from checkerpose_amd.synthetic import DATA
from tests.common import golden


def lm_table():
    return np.load(os.path.join(DATA, "fps_lm_15x4096.npy")).reshape(-1, 3)             # (61440, 3) float32


def mesh_of(g, table, mi):
    s, n = int(g["mesh_start"][mi]), int(g["mesh_count"][mi])
    return table[s:s + n]


def host_add(R_est, t_est, R_gt, t_gt, pts):
    """pose_error.add restated (float64): mean distance of the vertices under the two poses"""
    pts = np.asarray(pts, dtype=np.float64)
    pe = pts @ np.asarray(R_est, dtype=np.float64).T + np.asarray(t_est, dtype=np.float64).reshape(1, 3)
    pg = pts @ np.asarray(R_gt, dtype=np.float64).T + np.asarray(t_gt, dtype=np.float64).reshape(1, 3)
    return float(np.linalg.norm(pe - pg, axis=1).mean())


def host_adi(R_est, t_est, R_gt, t_gt, pts):
    """pose_error.adi restated (float64): a k-d tree over the vertices in the estimated pose, queried with those in the true pose"""
    from scipy.spatial import cKDTree
    pts = np.asarray(pts, dtype=np.float64)
    pe = pts @ np.asarray(R_est, dtype=np.float64).T + np.asarray(t_est, dtype=np.float64).reshape(1, 3)
    pg = pts @ np.asarray(R_gt, dtype=np.float64).T + np.asarray(t_gt, dtype=np.float64).reshape(1, 3)
    return float(cKDTree(pe).query(pg, k=1)[0].mean())


def tolerance(R_est, t_est, R_gt, t_gt, pts, ref):
    """the fp32 model-frame bound: 16 * 2^-24 * (largest vertex norm + |relative translation| + error)"""
    tr = np.asarray(R_est, dtype=np.float64).T @ (np.asarray(t_gt, dtype=np.float64).reshape(3) - np.asarray(t_est, dtype=np.float64).reshape(3))
    r_max = float(np.linalg.norm(np.asarray(pts, dtype=np.float64), axis=1).max())
    return 16.0 * 2.0 ** -24 * (r_max + float(np.linalg.norm(tr)) + ref)


def test_restatement_reproduces_the_reference():
    g, table = golden("pose_error"), lm_table()
    assert len(g["add"]) >= 35
    for c in range(len(g["add"])):
        pts = mesh_of(g, table, g["mesh"][c])
        a = host_add(g["R_est"][c], g["t_est"][c], g["R_gt"][c], g["t_gt"][c], pts)
        s = host_adi(g["R_est"][c], g["t_est"][c], g["R_gt"][c], g["t_gt"][c], pts)
        assert abs(a - g["add"][c]) <= 1e-9 * g["add"][c], (c, a, g["add"][c])
        assert abs(s - g["adi"][c]) <= 1e-9 * g["adi"][c], (c, s, g["adi"][c])
        if str(g["tag"][c]) == "0":
            assert g["add"][c] == 0.0 and g["adi"][c] == 0.0
        assert g["adi"][c] <= g["add"][c] * (1 + 1e-12)
    half = [c for c in range(len(g["tag"])) if str(g["tag"][c]) == "half"]
    assert half and all(g["adi"][c] < 0.5 * g["add"][c] for c in half)                  # the symmetric-looking case: ADI far below ADD
    assert max(g["add"]) > 1000.0                                                       # the identity fallback: beyond a metre


def test_diameters_match_the_reference():
    g, table = golden("pose_error"), lm_table()
    for mi in range(len(g["mesh_count"])):
        d = metric.calc_pts_diameter(mesh_of(g, table, mi))
        assert abs(d - g["mesh_diameter"][mi]) <= 1e-12 * max(1.0, g["mesh_diameter"][mi]), (mi, d, g["mesh_diameter"][mi])
    rng = np.random.default_rng(0)                                                       # and brute force on clouds without structure
    for n in (2, 7, 300):
        p = rng.normal(size=(n, 3)) * rng.uniform(1, 50, size=3)
        brute = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1).max())
        assert abs(metric.calc_pts_diameter(p) - brute) <= 1e-12 * brute


def test_auc_matches_the_reference_and_its_edge_cases():
    g = golden("pose_error")
    groups = sorted(set(g["group"].tolist()))
    sel = [g["group"] == k for k in groups] + [np.ones(len(g["group"]), bool)]
    assert len(sel) == len(g["auc_add"])
    for m, ra, ri in zip(sel, g["auc_add"], g["auc_adi"]):
        for got, ref in ((metric.compute_auc_posecnn(g["add"][m] / 1000.0), ra), (metric.compute_auc_posecnn(g["adi"][m] / 1000.0), ri)):
            assert (np.isnan(got) and np.isnan(ref)) or abs(got - ref) <= 1e-12, (got, ref)
    assert np.isfinite(g["auc_add"][-1]) and 0.0 < g["auc_add"][-1] < 100.0
    assert np.isnan(metric.compute_auc_posecnn(np.array([])))                            # empty
    assert np.isnan(metric.compute_auc_posecnn(np.array([0.11, 0.5, 3.0])))              # nothing within 0.1 m
    assert abs(metric.compute_auc_posecnn(np.zeros(4)) - 1.0) <= 1e-12                   # all perfect: the whole area (0.1 * 1 * 10)
    assert abs(metric.compute_auc_posecnn(np.array([0.05, 0.05, 0.05, 0.05])) - 0.625) <= 1e-12   # ties: the step at 0.05 counts once, at its first tie's height
    assert abs(metric.compute_auc_posecnn(np.array([0.05, 0.05, 0.2, 0.2])) - 0.375) <= 1e-12     # half of them missed
    assert abs(metric.compute_auc_posecnn(np.array([0.1])) - 1.0) <= 1e-12               # 0.1 itself still counts (the curve is read at a step's right end)
    e = np.array([0.02, 0.07, 0.07, 0.3])
    keep = e.copy()
    assert abs(metric.compute_auc_posecnn(e) - (0.02 * 0.25 + (0.07 - 0.02) * 0.5 + (0.1 - 0.07) * 0.75) * 10) <= 1e-12
    assert np.array_equal(e, keep)                                                       # the input is not modified


def test_summarize_counts_what_the_goldens_imply():
    g = golden("pose_error")
    diam = g["mesh_diameter"]
    for k in sorted(set(g["group"].tolist())):
        m = g["group"] == k
        ids = g["mesh"][m]
        err = {"add": g["add"][m], "adi": g["adi"][m]}
        s = metric.summarize(err, diam, mesh_ids=ids)
        n = int(m.sum())
        assert s["count"] == n
        for pct, f in ((2, 0.02), (5, 0.05), (10, 0.1)):
            assert s["passed_%d" % pct] * n == pytest.approx(sum(e < f * diam[i] for e, i in zip(err["add"], ids)), abs=1e-9)
            assert s["supp_passed_%d" % pct] * n == pytest.approx(sum(e < f * diam[i] for e, i in zip(err["adi"], ids)), abs=1e-9)
        ref = g["auc_add"][sorted(set(g["group"].tolist())).index(k)]
        assert (np.isnan(s["auc_posecnn"]) and np.isnan(ref)) or abs(s["auc_posecnn"] - ref) <= 1e-12
        assert sorted(s["per_mesh"]) == sorted(set(ids.tolist()))
        sym = metric.summarize(err, diam, symmetric=np.ones(len(diam), bool), mesh_ids=ids)      # symmetric objects: ADI is the main metric
        assert sym["passed_10"] == s["supp_passed_10"] and sym["supp_passed_10"] == s["passed_10"]
    # the strict `<` of test.py:382-386: an error equal to the threshold fails
    s = metric.summarize({"add": np.array([2.0, 5.0, 10.0, 1.0])}, 100.0)
    assert (s["passed_2"], s["passed_5"], s["passed_10"]) == (0.25, 0.5, 0.75)
    assert metric.summarize({"add": np.array([np.nan])}, 100.0)["passed_10"] == 0.0                 # nan counts as 10 000 (:379-380)
    with pytest.raises(ValueError):
        metric.summarize({"add": np.array([1.0])}, 100.0, symmetric=True)                            # main metric ADI not given
    per = metric.summarize({"add": np.array([1.0, 50.0, 1.0])}, np.array([100.0, 200.0]), mesh_ids=[0, 1, 1])["per_mesh"]
    assert per[0]["passed_2"] == 1.0 and per[1]["passed_2"] == 0.5 and per[1]["count"] == 2


def test_meshset_packing_and_offsets():
    a = np.arange(12, dtype=np.float64).reshape(4, 3)
    b = torch.arange(6, dtype=torch.float32).reshape(2, 3) + 100
    ms = metric.MeshSet.from_arrays([a, b, a[:1]])
    assert len(ms) == 3 and ms.offsets.tolist() == [0, 4, 6, 7] and ms.offsets.dtype == torch.int32
    assert ms.verts.dtype == torch.float32 and tuple(ms.verts.shape) == (7, 3) and ms.verts.is_contiguous()
    assert np.array_equal(ms.verts.numpy(), np.concatenate([a, b.numpy(), a[:1]]).astype(np.float32))
    assert ms.sizes.tolist() == [4, 2, 1]
    assert ms.diameters[0] == pytest.approx(np.linalg.norm(a[3] - a[0]), abs=1e-12) and ms.diameters[2] == 0.0
    assert metric.MeshSet.from_arrays(a, diameters=[7.5]).diameters.tolist() == [7.5]               # one bare array; given diameters kept
    for bad in ([], [np.zeros((0, 3))], [np.zeros((4, 2))]):
        with pytest.raises(ValueError):
            metric.MeshSet.from_arrays(bad)
    with pytest.raises(ValueError):
        metric.MeshSet.from_arrays([a, a], diameters=[1.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ms.on("cpu")


def test_no_cpu_fallback():
    R, t = torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3, 1, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.pose_errors(R, t, R, t, np.zeros((4, 3), np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.Calculate_ADD_Error_BOP(np.eye(3), np.zeros(3), np.eye(3), np.zeros(3), np.zeros((4, 3)), device="cpu")
    from checkerpose_amd import postprocess
    assert callable(postprocess.evaluate_poses)


def test_cp_pose_errors_rejects_bad_arguments_before_any_launch(lib):
    p = C.c_void_p(4096)                                    # fake, aligned; never dereferenced: every call returns before a launch
    both = _abi.POSE_ERR_ADD | _abi.POSE_ERR_ADI
    call = lib.cp_pose_errors
    assert call(None, None, p, p, p, 1, p, 2, 8, both, p, p, p) == -1          # null poses
    assert call(None, p, None, p, p, 1, p, 2, 8, both, p, p, p) == -1
    assert call(None, p, p, None, p, 1, p, 2, 8, both, p, p, p) == -1          # null vertex table
    assert call(None, p, p, p, p, 1, p, 2, 8, 0, p, p, p) == -1                # empty kinds mask
    assert call(None, p, p, p, p, 1, p, 2, 8, 4, p, p, p) == -1                # unknown kind bit
    assert call(None, p, p, p, p, 1, p, 2, 8, both, None, p, p) == -1          # an output that was asked for is missing
    assert call(None, p, p, p, p, 1, p, 2, 8, both, p, None, p) == -1
    assert call(None, p, p, p, p, 1, p, 2, 8, both, p, p, None) == -1          # ADI needs the scratch
    assert call(None, p, p, p, None, 1, p, 2, 8, both, p, p, p) == -1          # mesh_id without offsets
    assert call(None, p, p, p, p, 0, p, 2, 8, both, p, p, p) == -1             # offsets of no mesh
    assert call(None, p, p, p, p, 1, p, 0, 8, both, p, p, p) == -1             # B, Vmax
    assert call(None, p, p, p, p, 1, p, 2, 0, both, p, p, p) == -1
    assert call(None, p, p, C.c_void_p(4096 + 4), p, 1, p, 2, 8, both, p, p, p) == -3      # misaligned vertex table
    assert call(None, C.c_void_p(4096 + 4), p, p, p, 1, p, 2, 8, both, p, p, p) == -3      # misaligned fp64 poses
    assert call(None, p, p, p, C.c_void_p(4096 + 2), 1, p, 2, 8, both, p, p, p) == -3      # misaligned offsets
    assert call(None, p, p, p, p, 1, p, 20000, 1000000, both, p, p, p) == -4               # 20 000 x 977 query tiles: beyond 2^24 - 1 workgroups
    assert lib.cp_pose_errors_scratch_bytes(0, 8) == 0
    for B, V in ((1, 1), (1, 4096), (256, 4096), (1, 61440), (13, 4096)):
        n = lib.cp_pose_errors_scratch_bytes(B, V)
        assert n >= 4 * B * V and n % (4 * B * V) == 0                         # one float per pose, vertex and candidate split
    assert lib.cp_version() >= 206
