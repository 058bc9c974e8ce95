"""Row N16 (self-occlusion measure: hidden-point-removal visibility over views), host side.  tests/golden/visibility.npz holds what the
REFERENCE's own compute_vis_hpr returned with scipy's qhull for the reference's own transform of each cloud
(tests/golden/make_golden_visibility.py); the numpy restatement of the device rule (tests/visibility_stages.py) reproduces every
recorded mask EXACTLY.  The statistic, the wrapper's refusals, cp_hpr_visibility's argument checks (which return before any launch)
and the scratch query need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import checkerpose_amd
from checkerpose_amd import _abi, visibility
from tests import visibility_stages as S


@pytest.fixture(scope="module")
def g():
    return np.load(S.GOLDEN)


@pytest.fixture(scope="module")
def replay(g):
    """every case through the restatement, once: name -> (masks (n_views,V), statuses, per-view stats)"""
    out = {}
    for name in S.names():
        c, pts = S.CASES[name], S.cloud(name)
        R, t = S.views(name)
        rows = [S.hpr_rule(pts, R[k], S.view_t(t, k), c["radius_param"]) for k in range(c["n_views"])]
        out[name] = (np.stack([r[0] for r in rows]), [r[1] for r in rows], [r[2] for r in rows])
    return out


def test_fixture_holds_every_case_and_the_generators_have_not_drifted(g):
    assert len(S.names()) == 24
    kinds = {}
    for name in S.names():
        c, pts = S.CASES[name], S.cloud(name)
        R, t = S.views(name)
        assert int(g["crc__" + name]) == S.crc(pts, R, t), name
        m = g["mask__" + name]
        assert m.dtype == np.uint8 and m.shape == (c["n_views"], c["V"]) and set(np.unique(m)) <= {0, 1}, name
        assert float(g["margin__" + name]) >= S.MARGIN_FLOOR, name                       # the fixture's condition, not a tolerance
        assert np.allclose(np.einsum("nij,nkj->nik", R, R), np.eye(3), atol=1e-12) and np.linalg.det(R).min() > 0.99
        kinds.setdefault(c["kind"], []).append(c["V"])
    for kind in ("sphere", "box", "torus"):
        assert set(S.SIZES) <= set(kinds[kind])
    assert 2000 in kinds["sphere"] and g["mask__sphere_v2000"].shape == (4, 2000)
    assert sorted(c["radius_param"] for c in S.CASES.values())[0] == 1.5 and sum(c["tview"] for c in S.CASES.values()) == 1
    assert S.views("torus_v300_tview")[1].shape == (16, 3)
    for name in ("sphere_v300", "torus_v300", "sphere_v2000"):                            # the cases are not trivial: points ARE hidden
        assert 0.15 < g["mask__" + name].mean() < 0.6, name


@pytest.mark.parametrize("name", S.names())
def test_rule_restatement_reproduces_every_recorded_mask(g, replay, name):
    masks, statuses, _ = replay[name]
    assert statuses == [0] * len(statuses), name
    assert np.array_equal(masks, g["mask__" + name]), (name, int((masks != g["mask__" + name]).sum()))


def test_restatement_reports_faces_iterations_and_visible_sets(replay):
    worst_vis, faces, verts = 0, 0, 0
    for name in S.names():
        masks, _, stats = replay[name]
        V = S.CASES[name]["V"]
        for k, s in enumerate(stats):
            hull_vertices = int(masks[k].sum()) + 1                                      # + the viewpoint
            assert s["iterations"] == hull_vertices - 4, (name, k)                       # every inserted point is a final hull vertex
            assert s["faces_created"] >= 4 + 3 * s["iterations"]                         # a horizon holds at least 3 edges
            assert 4 + 2 * s["iterations"] <= 2 * (V + 1) - 4                            # the live faces fit the table
            assert 1 <= s["max_visible"] or s["iterations"] == 0
            worst_vis = max(worst_vis, s["max_visible"])
            faces += s["faces_created"]
            verts += hull_vertices
    print("largest visible set %d, faces created per hull vertex %.2f" % (worst_vis, faces / verts))
    assert worst_vis > 6            # the lists' global-memory spill (beyond 4 faces / 6 edges in LDS) is reached by the cases
    assert faces / verts < 5.2
    big = replay["sphere_v2000"][2]
    assert min(s["iterations"] for s in big) > 200                                       # hundreds of insertions per view


def test_restatement_status_codes():
    same = np.ones((4, 3))
    assert S.hpr_rule(same, np.eye(3), np.array(S.T_DEFAULT))[1] == 1                    # coincident points
    line = np.stack([np.zeros(6), np.zeros(6), np.linspace(100.0, 200.0, 6)], axis=1)
    assert S.hpr_rule(line, np.eye(3), np.zeros(3))[1] == 1                              # on one ray through the viewpoint: collinear


def test_statistic_counts_over_views_strict_thresholds(g):
    counts = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
    mean, lo, hi, below = S.statistic(counts, 10)
    assert np.array_equal(mean, counts / 10) and lo == 0.0 and hi == 1.0
    expect = [np.mean(counts / 10 < i * 0.1) for i in range(1, 10)]
    assert below.tolist() == expect
    assert below[0] == 1 / 11                                                            # 0.1 < 1 * 0.1 is False: strict
    assert below[2] == 4 / 11                                                            # 3 / 10 < 3 * 0.1 = 0.30000000000000004: the script's thresholds
    for name in ("sphere_v300", "torus_v65"):
        m = g["mask__" + name]
        mean, lo, hi, below = S.statistic(m.sum(axis=0), m.shape[0])
        assert np.array_equal(mean, g["mean__" + name]) and np.array_equal(np.concatenate([[lo, hi], below]), g["stat__" + name])


def test_names_are_reachable_from_the_package():
    assert checkerpose_amd.compute_vis_hpr is visibility.compute_vis_hpr
    assert checkerpose_amd.hpr_visibility is visibility.hpr_visibility
    assert checkerpose_amd.overall_visibility is visibility.overall_visibility
    assert "UNPINNED" in visibility.__doc__ and "UNPINNED" in visibility.overall_visibility.__doc__


def test_wrapper_refuses_bad_input_before_any_launch():
    pts, R = S.cloud("sphere_v5"), np.eye(3)[None]
    for bad in (pts[:3], np.zeros((5, 2)), np.zeros((0, 3))):                            # V < 4 (the reference's V = 3 is not rebuilt)
        with pytest.raises(ValueError):
            visibility.hpr_visibility(bad, R, device="cpu")
    for val in (np.nan, np.inf, -np.inf):
        a = pts.copy()
        a[2, 1] = val
        with pytest.raises(ValueError):
            visibility.hpr_visibility(a, R, device="cpu")
        with pytest.raises(ValueError):
            visibility.compute_vis_hpr(a, device="cpu")
        with pytest.raises(ValueError):
            visibility.hpr_visibility(pts, np.full((1, 3, 3), val), device="cpu")
        with pytest.raises(ValueError):
            visibility.hpr_visibility(pts, R, t=(0.0, val, 400.0), device="cpu")
        with pytest.raises(ValueError):
            visibility.hpr_visibility(pts, R, radius_param=val, device="cpu")
    with pytest.raises(ValueError):
        visibility.hpr_visibility(pts, np.zeros((0, 3, 3)), device="cpu")                # n_views < 1
    with pytest.raises(ValueError):
        visibility.hpr_visibility(pts, np.eye(4)[None], device="cpu")
    with pytest.raises(ValueError):
        visibility.hpr_visibility(pts, np.stack([np.eye(3)] * 2), t=np.zeros((3, 3)), device="cpu")
    for rp in (-0.5, 8.5, 300.0):                                                        # absurd radius parameters
        with pytest.raises(ValueError):
            visibility.hpr_visibility(pts, R, radius_param=rp, device="cpu")
        with pytest.raises(ValueError):
            visibility.compute_vis_hpr(pts, radius_param=rp, device="cpu")
    with pytest.raises(ValueError):
        visibility.hpr_visibility(pts, R, device="cpu", _workgroups=-1)
    with pytest.raises(ValueError):
        visibility.hpr_visibility(pts, R, device="cpu", _workgroups=65536)
    # a vertex at the viewpoint (norm 0): in a single view, in one view of a batch, through compute_vis_hpr's viewpoint
    a = pts.copy()
    a[3] = (0.0, 0.0, -400.0)
    with pytest.raises(ValueError, match="viewpoint in view 0"):
        visibility.hpr_visibility(a, R, device="cpu")
    Rs, ts = S.rotations(5, 3), np.array(S.T_DEFAULT) + np.arange(15.0).reshape(5, 3)
    a[3] = np.linalg.solve(Rs[4], -ts[4])
    hit = visibility._camera(a, Rs[4], ts[4])[3]
    if (hit == 0).all():                                                                 # (the solve may land an ulp off: then no view hits)
        with pytest.raises(ValueError, match="viewpoint in view 4"):
            visibility.hpr_visibility(a, Rs, ts, device="cpu")
    with pytest.raises(ValueError, match="viewpoint"):
        visibility.compute_vis_hpr(pts + 7.0, viewpoint=pts[2] + 7.0, device="cpu")
    with pytest.raises(ValueError):
        visibility.compute_vis_hpr(pts, viewpoint=(0.0, np.nan, 0.0), device="cpu")
    # well-formed input on the host: no fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        visibility.hpr_visibility(pts, R, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        visibility.compute_vis_hpr(pts, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        visibility.overall_visibility(pts, R, device="cpu")
    assert visibility._vertex_at_viewpoint(pts, S.rotations(16, 1), np.array(S.T_DEFAULT)) is None


def test_cp_hpr_visibility_rejects_bad_arguments_before_any_launch(lib):
    p = C.c_void_p(4096)                                    # fake, aligned; never dereferenced: every call returns before a launch
    call = lib.cp_hpr_visibility

    def args(**kw):
        a = dict(pts=p, R=p, t=p, t_stride=0, n_views=3, V=9, rp=2.0, wg=0, counts=p, mask=p, status=p, scratch=p)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = call(None, a["pts"], a["R"], a["t"], a["t_stride"], a["n_views"], a["V"], a["rp"], a["wg"], a["counts"], a["mask"],
                  a["status"], a["scratch"])
        assert lib.cp_kernel_log() == b"", kw
        return rc
    for name in ("pts", "R", "t", "counts", "status", "scratch"):
        assert args(**{name: None}) == -1, name
    assert args(n_views=0) == -1 and args(n_views=-2) == -1
    assert args(V=3) == -1 and args(V=0) == -1 and args(V=-7) == -1
    assert args(t_stride=1) == -1 and args(t_stride=-3) == -1 and args(t_stride=6) == -1
    for rp in (float("nan"), float("inf"), -float("inf"), -0.25, 8.25):
        assert args(rp=rp) == -1, rp
    assert args(wg=-1) == -1
    odd8, odd4 = C.c_void_p(4096 + 4), C.c_void_p(4096 + 2)
    for name in ("pts", "R", "t", "scratch"):
        assert args(**{name: odd8}) == -3, name
    for name in ("counts", "status"):
        assert args(**{name: odd4}) == -3, name
    assert args(V=(1 << 22) + 1) == -4 and args(wg=65536) == -4
    assert lib.cp_version() >= 217


def test_scratch_query_is_per_workgroup_and_zero_for_bad_shapes(lib):
    q = lib.cp_hpr_visibility_scratch_bytes
    assert q(0, 9, 0) == 0 and q(-1, 9, 0) == 0 and q(3, 3, 0) == 0 and q(3, 0, 0) == 0 and q(3, (1 << 22) + 1, 0) == 0
    assert q(3, 9, -1) == 0 and q(3, 9, 65536) == 0

    def slab(V):                                            # N points, Fcap face slots, Hcap staged faces
        N, F = V + 1, 2 * V - 2
        H = F + 2
        return (8 * (3 * N + 4 * F + 4 * H) + 4 * (2 * N + 5 * F + 2 * H) + 15) // 16 * 16
    for V in (4, 5, 64, 2000, 50000):
        one = q(1, V, 0)
        assert one == slab(V), V
        assert q(2562, V, 1) == one and q(2562, V, 7) == 7 * one and q(3, V, 64) == 3 * one      # never more workgroups than views
        auto = q(2562, V, 0)
        assert auto % one == 0 and 1 <= auto // one <= 512 and (auto <= 2 << 30 or auto == one)
    assert q(1, 50000, 0) == 10799936                      # 10.8 MB per workgroup at V = 50 000, whatever the number of views
    assert q(16, 300, 0) == 16 * q(1, 300, 0)
