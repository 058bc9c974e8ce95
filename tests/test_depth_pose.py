"""CPU: row N25's rule (tests/depth_pose_stages.py) against independent arithmetic -- the fit against numpy.linalg.svd's Kabsch, the
rank-2 completion, the sampler against oracle/pnp_oracle.py --; check_case's power: tamperings of the records, each caught; the
committed cases: no decision near its boundary, the converging crops near their truth; refusals and defaults of the new entry points;
estimate_poses' new keywords with stubs; every existing default unchanged."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import depth_pose_stages as D


def _kabsch(X, Q):
    """the textbook solution by LAPACK's SVD: R = U diag(1, 1, det(U V^T)) V^T of H = sum (Q - q)(X - x)^T"""
    x, q = X.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - q).T @ (X - x))
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    return R, q - R @ x


def _pose(rng):
    R = D._rotation(rng)
    return R, rng.uniform(-50, 50, 3) + np.array([0, 0, 400.0])


# ---------------------------------------------------------------------------------------------------------------- the arithmetic
@pytest.mark.parametrize("n,noise", [(3, 0.0), (4, 0.5), (17, 0.0), (300, 1.0), (1000, 3.0)])
def test_fit_is_kabsch(n, noise):
    rng = np.random.default_rng(n)
    for trial in range(8):
        X = rng.normal(scale=40.0, size=(n, 3))
        R, t = _pose(rng)
        Q = X @ R.T + t + rng.normal(scale=noise, size=(n, 3)) if noise else X @ R.T + t
        for sums in (D.device_sum, D.permuted_sum):
            P = D.fit(X, Q, np.ones(n, bool), sums)
            Rk, tk = _kabsch(X, Q)
            assert np.abs(P[:9].reshape(3, 3) - Rk).max() < 1e-11 and np.abs(P[9:] - tk).max() < 1e-9
            assert abs(np.linalg.det(P[:9].reshape(3, 3)) - 1.0) < 1e-12
        if not noise:
            assert np.abs(P[:9].reshape(3, 3) - R).max() < 1e-11
    # the mask: rows outside it play no part
    mask = rng.random(n) < 0.6
    mask[:3] = True
    P = D.fit(X, Q, mask)
    Rk, tk = _kabsch(X[mask], Q[mask])
    assert np.abs(P[:9].reshape(3, 3) - Rk).max() < 1e-11 and np.abs(P[9:] - tk).max() < 1e-9


def test_minimal_pose_is_the_fit_of_three():
    rng = np.random.default_rng(5)
    for trial in range(50):
        X = rng.normal(scale=40.0, size=(3, 3))
        R, t = _pose(rng)
        Q = X @ R.T + t
        P = D.minimal_pose(X, Q)
        assert np.abs(P[:9].reshape(3, 3) - R).max() < 1e-10 and np.abs(P[9:] - t).max() < 1e-8           # rank 2: completed, det +1
        assert D.residual2(P, X, Q).max() < 1e-18 * 400.0 ** 2
        Q = Q + rng.normal(scale=2.0, size=(3, 3))                   # incongruent triangles: still the least-squares pose
        Rk, tk = _kabsch(X, Q)
        P = D.minimal_pose(X, Q)
        assert np.abs(P[:9].reshape(3, 3) - Rk).max() < 1e-10 and np.abs(P[9:] - tk).max() < 1e-8


def test_rank2_completion_and_reflection():
    rng = np.random.default_rng(6)
    for trial in range(20):
        X = rng.normal(scale=40.0, size=(200, 3))
        X[:, 2] = 0.0                                                # coplanar model points: H has rank 2
        R, t = _pose(rng)
        Q = X @ R.T + t
        H = (Q - Q.mean(0)).T @ (X - X.mean(0))
        Rn, rank = D.nearest_rotation(H)
        assert rank == 2 and np.abs(np.reshape(Rn, (3, 3)) - R).max() < 1e-11 and abs(np.linalg.det(np.reshape(Rn, (3, 3))) - 1.0) < 1e-12
        # a reflected cloud: the nearest PROPER rotation flips the weakest direction (LAPACK's Kabsch does the same)
        X = rng.normal(scale=(40.0, 25.0, 3.0), size=(200, 3))
        Q = (X * np.array([1.0, 1.0, -1.0])) @ R.T + t
        P = D.fit(X, Q, np.ones(200, bool))
        Rk, tk = _kabsch(X, Q)
        assert np.abs(P[:9].reshape(3, 3) - Rk).max() < 1e-10 and abs(np.linalg.det(P[:9].reshape(3, 3)) - 1.0) < 1e-12
    # rank < 2: no rotation
    line = np.outer(np.linspace(-1, 1, 9), [1.0, 2.0, -0.5])
    assert D.nearest_rotation(line.T @ line)[0] is None and D.nearest_rotation(np.zeros((3, 3)))[0] is None
    assert D.nearest_rotation(np.full((3, 3), np.nan))[0] is None
    assert D.fit(line, line + 1.0, np.ones(9, bool)) is None
    assert D.minimal_pose(line[:3], line[:3] + 1.0) is None                                      # collinear sample: degenerate
    assert D.minimal_pose(np.eye(3), np.ones((3, 3))) is None                                    # identical lifted points: rank 0


def test_sampler_is_the_oracles():
    from oracle.pnp_oracle import _hash32, sample_indices
    rng = np.random.default_rng(7)
    for _ in range(300):
        seed, crop, hyp, n = int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 64)), int(rng.integers(0, 256)), int(rng.integers(3, 4097))
        assert D.sample3(seed, crop, hyp, n) == sample_indices(seed, crop, hyp, n, 3)
        assert D.hash32(seed, crop, hyp, 5) == _hash32(seed, crop, hyp, 5)
    assert sorted(D.sample3(1, 0, 0, 3)) == [0, 1, 2]


def test_device_sum_is_a_sum():
    rng = np.random.default_rng(8)
    for n in (1, 63, 256, 257, 1000, 4096):
        v = rng.normal(size=(n, 5)) * 10.0 ** rng.integers(-3, 4, size=(n, 1))
        ref = np.array([float(np.sum(v[:, k].astype(np.longdouble))) for k in range(5)])
        for sums in (D.device_sum, D.permuted_sum):
            assert np.abs(sums(v) - ref).max() <= 1e-12 * np.abs(v).sum(0).max()


def test_needed_iters_is_opencvs():
    assert D.needed_iters(2, 100, 3, 150)[0] == 150 and D.needed_iters(100, 100, 3, 150)[0] == 0
    assert D.needed_iters(50, 100, 3, 256)[0] == int(np.rint(np.log(0.01) / np.log(1 - 0.125))) == 34
    assert D.needed_iters(10, 100, 3, 150)[0] == 150


def test_lift_rule():
    K = D.K_A
    depth = np.zeros((2, 80, 96), np.float32)
    depth[0, 10, 20], depth[0, 79, 95], depth[1, 10, 20] = 300.0, 250.0, 123.0
    depth[0, 11, 20], depth[0, 12, 20], depth[0, 13, 20] = np.nan, np.inf, -5.0
    p2d = np.array([[20.75, 10.25], [95.99, 79.5], [96.0, 40.0], [-0.01, 3.0], [20.0, 11.0], [20.0, 12.0], [20.0, 13.0], [20.5, 14.0], [20.9, 10.9],
                    [np.nan, 10.0], [20.75, 10.25]], np.float32)
    valid = np.ones(len(p2d), bool)
    valid[-1] = False
    Q, lf = D.lift(p2d, valid, K, depth, 0)
    assert lf.tolist() == [True, True] + [False] * 6 + [True, False, False]
    assert Q[0, 2] == 300.0 and Q[8, 2] == 300.0 and Q[1, 2] == 250.0 and not Q[~lf].any()
    # the ray goes through (u, v) as given, not through the pixel centre: one rounding from fp64
    u, v = np.float64(p2d[0, 0]), np.float64(p2d[0, 1])
    assert Q[0, 0] == np.float32((u - np.float64(K[0, 2])) / np.float64(K[0, 0]) * 300.0) and Q[0, 1] == np.float32((v - np.float64(K[1, 2])) / np.float64(K[1, 1]) * 300.0)
    assert Q[0, 0] != Q[8, 0]
    assert D.lift(p2d, valid, K, depth, 1)[0][0, 2] == 123.0
    assert not D.lift(p2d, valid, K, depth, 2)[1].any() and not D.lift(p2d, valid, K, depth, -1)[1].any()
    # p2d as `correspondences` gives them: corners of the 64-cell grid over the integer box, fp32
    uv = np.array([[10.2, 20.7], [40.9, 33.1], [25.0, 25.0]])
    q = D.quantise(uv)
    assert q.dtype == np.float32 and np.array_equal(q[0], np.float32([9 + 33 / 64 * 2, 19 + 16 / 64 * 6])) and (np.abs(q - uv) < [33 / 64, 16 / 64]).all() and (q <= uv).all()


# ---------------------------------------------------------------------------------------------------------------- the cases
CPU_CASES = list(D.CASES)


def test_case_set_covers_the_issue():
    cases = [D.make(n) for n in D.CASES]
    assert {c.N for c in cases} >= {3, 5, 64, 512, 4096} and any(c.N == 4096 and c.B == 2 for c in cases)
    assert {c.B for c in cases} >= {1, 3, 5} and any(c.image_ids is not None and len(set(c.image_ids.tolist())) < c.B for c in cases)
    assert any(c.K.ndim == 3 for c in cases) and any(c.K.ndim == 2 for c in cases) and any(c.p3d.ndim == 3 for c in cases)
    assert {c.iterations for c in cases} >= {1, 64, 65, 256} and {c.column for c in cases} == {0, 1, 2}
    assert any(np.ndim(c.thr) == 1 for c in cases) and any(np.ndim(c.thr) == 0 for c in cases)
    assert all(c.depth.shape[1:] == (80, 96) for c in cases)
    assert any(np.isnan(c.depth).any() and np.isinf(c.depth).any() and (c.depth < 0).any() and (c.depth == 0).any() for c in cases)
    assert any(((c.p2d[..., 0] >= 96) | (c.p2d[..., 0] < 0)).any() for c in cases)
    lifted = {n: [int(D.make(n).lifted(b)[1].sum()) for b in range(D.make(n).B)] for n in D.CASES}
    assert lifted["three_lifted"] == [3, 3] and lifted["two_lifted"] == [2, 0] and lifted["n3"] == [3]
    assert len(D.converging()) >= 20


@pytest.mark.parametrize("name", CPU_CASES)
def test_cases_have_no_decision_near_its_boundary(name):
    case = D.make(name)
    out = D.restatement_outputs(case)
    res = D.check_case(case, out)
    assert res["near"] == [] and res["seen"] == (0.0, 0.0)
    if name == "collinear":
        assert out["status"].tolist() == [0] and (out["hypotheses"][0, :, 0] == -1).all()            # every hypothesis degenerate
    if name == "two_lifted":
        assert out["status"].tolist() == [0, 0] and np.isnan(out["hypotheses"]).all()
    if name == "three_lifted":
        assert sorted(out["status"].tolist()) == [0, 1]              # three pairs: solved when the triangles agree within the threshold
    if name == "coplanar":
        assert (out["steps"][:, 0, 1] == 1).all()                    # the rank-2 refit succeeds
    if name == "n512_slab_half":                                     # the occluder: 30 - 50 % of the lifted keypoints are outliers
        assert 0.3 <= 1.0 - out["inliers"][0].sum() / out["n_lifted"][0] <= 0.5


def test_free_running_rule_reaches_the_truth():
    for name, b in D.converging(CPU_CASES):
        case = D.make(name)
        out = D.restatement_outputs(case)
        X = case.crop(b)[0]
        add = D.add_error(X, out["R"][b], out["t"][b], *case.truth[b])
        assert out["status"][b] == 1 and add < 0.05 * np.linalg.norm(X, axis=1).max(), (name, b, add)
        P = np.concatenate([out["R"][b].reshape(9), out["t"][b]])
        idx = np.nonzero(out["lifted"][b])[0]
        L = out["inliers"][b, idx]
        assert np.array_equal(_bits(D.fit(X[idx], out["Q"][b, idx].astype(np.float64), L)), _bits(P))      # the pose IS the fit over the returned inliers


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_local_optimisation_pays():
    """stage C against the winner's first fit alone, after ONE mediocre hypothesis: several times the inliers, nearer the truth"""
    case = D.make("grow")
    full, bare = D.restatement_outputs(case), D.restatement_outputs(case, tamper=("no_lo",))
    assert (full["inliers"].sum(1) > 3 * bare["inliers"].sum(1)).all()
    assert np.array_equal(full["steps"][:, :, 1], [[1, 1, 0, np.nan], [1, 1, 1, 1]], equal_nan=True)        # a stop by the count, and all 3 used
    for b in range(case.B):
        X = case.crop(b)[0]
        assert D.add_error(X, full["R"][b], full["t"][b], *case.truth[b]) < D.add_error(X, bare["R"][b], bare["t"][b], *case.truth[b])


TAMPERINGS = {
    "count": lambda o: o["hypotheses"].__setitem__((0, 3, 0), o["hypotheses"][0, 3, 0] + 1),
    "degenerate_flag": lambda o: o["hypotheses"].__setitem__((0, 5, 0), -1.0),
    "hypothesis_pose": lambda o: o["hypotheses"].__setitem__((0, 2, 13), o["hypotheses"][0, 2, 13] * (1 + 1e-9)),
    "record_behind_the_stop": lambda o: o["hypotheses"].__setitem__((0, -1, 0), 7.0),
    "missing_record": lambda o: o["hypotheses"].__setitem__((0, 9), np.nan),
    "step_flag": lambda o: o["steps"].__setitem__((0, 0, 1), 0.0),
    "step_count": lambda o: o["steps"].__setitem__((0, 0, 0), o["steps"][0, 0, 0] - 1),
    "step_pose": lambda o: o["steps"].__setitem__((0, 0, 2), o["steps"][0, 0, 2] + 1e-7),
    "extra_step": lambda o: o["steps"].__setitem__((0, 3), o["steps"][0, 0]),
    "returned_pose": lambda o: o["t"].__setitem__((0, 2), np.nextafter(o["t"][0, 2], np.inf)),
    "inlier_bit": lambda o: o["inliers"].__setitem__((0, int(np.nonzero(o["lifted"][0])[0][0])), ~o["inliers"][0, int(np.nonzero(o["lifted"][0])[0][0])]),
    "inlier_not_lifted": lambda o: o["inliers"].__setitem__((0, int(np.nonzero(o["lifted"][0] == 0)[0][0])), True),
    "status": lambda o: o["status"].__setitem__(0, 0),
    "lifted": lambda o: o["lifted"].__setitem__((0, int(np.nonzero(o["lifted"][0])[0][0])), 0),
    "Q_bit": lambda o: o["Q"].__setitem__((0, int(np.nonzero(o["lifted"][0])[0][0]), 0), np.nextafter(o["Q"][0, int(np.nonzero(o["lifted"][0])[0][0]), 0], np.float32(1e9))),
    "n_lifted": lambda o: o["n_lifted"].__setitem__(0, o["n_lifted"][0] + 1),
}


@pytest.mark.parametrize("what", list(TAMPERINGS))
def test_tampered_records_are_caught(what):
    case = D.make("column_2")                                        # 150 iterations of which one round runs; holes, so some keypoints are not lifted
    out = {k: v.copy() for k, v in D.restatement_outputs(case).items()}
    assert np.isnan(out["hypotheses"][0, 64:]).all() and np.isnan(out["steps"][0, 3]).all() and not out["lifted"][0].all()
    D.check_case(case, out)
    TAMPERINGS[what](out)
    with pytest.raises(D.StageError):
        D.check_case(case, out)


@pytest.mark.parametrize("rule", ["strict", "no_stop", "no_lo"])
def test_another_rule_is_caught(rule):
    """records made under a rule that differs in one decision do not replay"""
    caught = 0
    for name in ("n64_b3", "n512_slab_half", "column_1", "coplanar", "grow"):
        case = D.make(name)
        out = D.restatement_outputs(case, tamper=(rule,))
        same = all(np.array_equal(out[k], D.restatement_outputs(case)[k], equal_nan=True) for k in out if k != "winner")     # (what a device returns)
        try:
            D.check_case(case, out)
            assert same, (rule, name)                                # it replays only where the other rule decided nothing differently
        except D.StageError:
            assert not same
            caught += 1
    assert caught >= 1 or rule == "strict"                           # (r^2 == thr^2 exactly does not occur in the cases: "strict" decides alike)


# ------------------------------------------------------------------------------------------------------- refusals and defaults
def _host_args():
    case = D.make("n64_b3")
    t = torch.from_numpy
    return dict(p3d_xyz=t(case.p3d), p2d=t(case.p2d), valid=t(case.valid), cam_K=t(case.K), depth=t(case.depth), dist_threshold=8.0,
                image_ids=case.image_ids)


def test_refusals_and_defaults():
    from checkerpose_amd import postprocess as PP
    sig = inspect.signature(PP.solve_pose_depth).parameters
    assert list(sig) == ["p3d_xyz", "p2d", "valid", "cam_K", "depth", "dist_threshold", "image_ids", "column", "iterations", "seed", "return_hypotheses"]
    assert sig["dist_threshold"].default is inspect.Parameter.empty                  # NO default
    assert [sig[k].default for k in ("image_ids", "column", "iterations", "seed", "return_hypotheses")] == [None, 0, 150, 0, False]
    sig = inspect.signature(PP.lift_correspondences).parameters
    assert list(sig) == ["p2d", "valid", "cam_K", "depth", "image_ids", "column"] and [sig[k].default for k in ("image_ids", "column")] == [None, 0]
    a = _host_args()
    for name, bad in (("iterations", 0), ("iterations", 257), ("dist_threshold", 0.0), ("dist_threshold", -2.0), ("dist_threshold", float("nan")),
                      ("dist_threshold", float("inf")), ("dist_threshold", None)):
        with pytest.raises((ValueError, RuntimeError), match=name if name != "dist_threshold" else "dist_threshold|no CPU fallback"):
            PP.solve_pose_depth(**dict(a, **{name: bad}))
    with pytest.raises(ValueError, match="iterations"):
        PP.solve_pose_depth(**dict(a, iterations=257))
    with pytest.raises(ValueError, match="column"):
        PP.solve_pose_depth(**dict(a, column=3))
    with pytest.raises(ValueError, match="valid"):
        PP.solve_pose_depth(**dict(a, valid=a["valid"][:, :, 0]))
    with pytest.raises(ValueError, match="p2d"):
        PP.lift_correspondences(a["p2d"][0], a["valid"], a["cam_K"], a["depth"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                       # well-formed arguments on the host: still no fallback
        PP.solve_pose_depth(**a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.lift_correspondences(a["p2d"], a["valid"], a["cam_K"], a["depth"], image_ids=a["image_ids"])
    with pytest.raises(TypeError):
        PP.solve_pose_depth(a["p3d_xyz"], a["p2d"], a["valid"], a["cam_K"], a["depth"])           # dist_threshold is required


def test_existing_signatures_are_prefixes():
    """nothing existing changes: every public call keeps its parameters, order and defaults; estimate_poses gains two at the end"""
    from checkerpose_amd import postprocess as PP
    want = {
        "correspondences": "(outputs, roi_xy_ori=None, discard_bd_pixel=0, Bboxes=None)",
        "solve_pnp_ransac": "(p3d_xyz, p2d, valid, cam_K, column=0, reproj_threshold=2.0, iterations=150, seed=0, return_hypotheses=False)",
        "solve_pnp_gc": "(p3d_xyz, p2d, valid, cam_K, graph, graph_ids=None, column=0, reproj_threshold=2.0, spatial_coherence_weight=0.1, "
                        "iterations=400, min_inliers=6, seed=0, return_stages=False)",
        "refine_poses_lm": "(p3d_xyz, p2d, mask, cam_K, R, t, status=None, max_iters=20, step_tol=1e-10, return_records=False)",
        "refine_poses_icp": "(R, t, cam_K, meshes, depth, max_dist, image_ids=None, mesh_ids=None, status=None, grid=32, max_iters=20, step_tol=1e-06, "
                            "min_pairs=6, inertia=0.01, samples=None, return_records=False)",
        "surface_samples": "(R, t, cam_K, meshes, size, mesh_ids=None, grid=32)",
        "evaluate_poses": "(net, frames, Bboxes, p3d_xyz, cam_K, R_gt, t_gt, vertices, mesh_ids=None, kinds=('add', 'adi'), symmetries=None, "
                          "depth_test=None, image_ids=None, size=None, **estimate_kwargs)",
        "from_id_to_pose": "(p3d_xyz, roi_xy_ori, cam_K, roi_mask_bit, pixel_x_id, pixel_y_id, check_seg=False, seg_mask=None, use_progressivex=False, "
                           "neighborhood_ball_radius=20, spatial_coherence_weight=0.1, prog_max_iters=400, discard_bd_pixel=0, return_inliers=False, "
                           "reprojErr_thresh=2, cv_max_iters=150, device='cuda:0', seed=0, progx_backend=None, refine=None)",
    }
    for name, sig in want.items():
        assert str(inspect.signature(getattr(PP, name))) == sig, name
    before = ("(net, frames, Bboxes, p3d_xyz, cam_K, img_index=None, obj_ids=None, padding_ratio=1.5, crop_size=256, resize_method='crop_square_resize', "
              "check_seg=False, discard_bd_pixel=0, reproj_threshold=2.0, iterations=150, seed=0, solver='epnp', graph=None, spatial_coherence_weight=0.1, "
              "prog_max_iters=400, refine=None, icp=None")
    assert str(inspect.signature(PP.estimate_poses)) == before + ", depth=None, dist_threshold=None)"
    assert "depth" not in inspect.signature(PP.from_id_to_pose).parameters       # it has no depth and keeps refusing
    z = np.zeros
    with pytest.raises(TypeError):
        PP.from_id_to_pose(z((8, 3), np.float32), z((1, 8, 2), np.float32), np.eye(3, dtype=np.float32), z((8, 1), np.float32), np.arange(8),
                           z(8, np.int64), solver="depth")


def test_estimate_poses_keywords():
    from checkerpose_amd import postprocess as PP
    frames, p3d, K = torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(8, 3), torch.eye(3)
    with pytest.raises(ValueError, match="solver"):
        PP.estimate_poses(None, frames, [], p3d, K, solver="kabsch")
    for kw in (dict(), dict(depth="D"), dict(dist_threshold=5.0)):               # both are required with "depth"
        with pytest.raises(ValueError, match="dist_threshold"):
            PP.estimate_poses(None, frames, [], p3d, K, solver="depth", **kw)
    for solver in ("epnp", "gc"):                                                # and refused with the other solvers
        for kw in (dict(depth="D"), dict(dist_threshold=5.0), dict(depth="D", dist_threshold=5.0)):
            with pytest.raises(ValueError, match="solver='depth'"):
                PP.estimate_poses(None, frames, [], p3d, K, solver=solver, graph="G", **kw)


def test_estimate_poses_routes_depth(monkeypatch):
    """the solver call and what follows it, with stubs in place of every device call"""
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import preprocess as PRE
    calls = []
    monkeypatch.setattr(PRE, "get_roi_batch", lambda *a, **k: "crops")
    monkeypatch.setattr(PP, "correspondences", lambda out, **k: ("p2d", "valid", None))
    monkeypatch.setattr(PP, "solve_pnp_ransac", lambda *a, **k: ("R0", "t0", "inl", "status"))

    def depth_solver(p3d, p2d, valid, K, depth, thr, **kw):
        calls.append(("depth", p3d, p2d, valid, K, depth, thr, kw))
        return "Rd", "td", "inld", "std"

    def lm(p3d, p2d, mask, K, R, t, status=None):
        calls.append(("lm", R, t, mask, status))
        return R + "+lm", t + "+lm", None, None

    def icp(R, t, K, meshes, depth, max_dist, **kw):
        calls.append(("icp", R, t, depth, max_dist, kw))
        return R + "+icp", t + "+icp", None, None

    monkeypatch.setattr(PP, "solve_pose_depth", depth_solver)
    monkeypatch.setattr(PP, "refine_poses_lm", lm)
    monkeypatch.setattr(PP, "refine_poses_icp", icp)
    frames = torch.zeros(2, 40, 40, 3, dtype=torch.uint8)
    args = (lambda crops, _: "out", frames, [[5, 5, 10, 10]], "p3d", "K")
    assert PP.estimate_poses(*args, img_index=[1])[:4] == ("R0", "t0", "inl", "status") and calls == []        # the default is unchanged
    want = ("depth", "p3d", "p2d", "valid", "K", "D", 5.0, dict(image_ids=[1], column=0, iterations=77, seed=4))
    assert PP.estimate_poses(*args, img_index=[1], solver="depth", depth="D", dist_threshold=5.0, iterations=77, seed=4)[:4] == ("Rd", "td", "inld", "std")
    assert calls == [want]
    del calls[:]
    out = PP.estimate_poses(*args, img_index=[1], solver="depth", depth="D", dist_threshold=5.0, iterations=77, seed=4, check_seg=True, refine="lm")
    assert out[:4] == ("Rd+lm", "td+lm", "inld", "std")                          # "lm" polishes over the returned inliers
    assert calls == [want[:7] + (dict(want[7], column=1),), ("lm", "Rd", "td", "inld", "std")]
    del calls[:]
    spec = dict(meshes="M", depth="D2", max_dist=7.0)                            # "icp" still takes its own dict (its own depth)
    out = PP.estimate_poses(*args, img_index=[1], solver="depth", depth="D", dist_threshold=5.0, iterations=77, seed=4, refine="icp", icp=spec)
    assert out[:4] == ("Rd+icp", "td+icp", "inld", "std") and calls == [want, ("icp", "Rd", "td", "D2", 7.0, dict(image_ids=[1], status="std"))]
    # evaluate_poses reaches it through the keywords it already forwards
    from checkerpose_amd import metric
    monkeypatch.setattr(metric, "score_poses", lambda R, t, *a, **k: {"add": (R, t)})
    del calls[:]
    E = PP.evaluate_poses(*args, "Rgt", "tgt", "V", img_index=[1], solver="depth", depth="D", dist_threshold=5.0, iterations=77, seed=4)
    assert E[0] == {"add": ("Rd", "td")} and E[1:5] == ("Rd", "td", "inld", "std") and calls == [want]


def test_abi():
    """the library on a CPU box: the new symbols resolve, the constants, the refusals with fake pointers (nothing launches)"""
    from checkerpose_amd import _abi
    from checkerpose_amd import postprocess as PP
    lib = _abi.load()
    assert lib.cp_version() >= 235
    assert lib.cp_pose_depth_record_doubles() == D.RECORD == PP.DEPTH_POSE_RECORD == 14
    assert (PP.DEPTH_POSE_MAX_ITERS, PP.DEPTH_POSE_NMAX, PP.DEPTH_POSE_STEPS) == (D.MAX_ITERS, D.NMAX, D.STEPS) == (256, 4096, 4)
    assert lib.cp_pose_depth_ransac_scratch_bytes(2, 64, 150) == 2 * 150 * 112 + 2 * 4 * 112 + 2 * 64 * 12 + 8 + 128
    assert [lib.cp_pose_depth_ransac_scratch_bytes(*a) for a in ((0, 64, 150), (2, 0, 150), (2, 4097, 150), (2, 64, 0), (2, 64, 257))] == [0] * 5
    buf = C.create_string_buffer(4096 + 16)
    p = (C.addressof(buf) + 15) & ~15
    ok_l = [None, p, p, 3, p, 0, p, None, 1, 80, 96, 2, 64, p, p, p]
    ok_s = [None, p, 0, p, p, 3, p, 9, p, None, 2, 80, 96, 2, 512, 5.0, None, 150, 7, p, p, p, p]

    def l_with(i, v):
        a = list(ok_l)
        a[i] = v
        return lib.cp_lift_correspondences(*a)

    def s_with(*pairs):
        a = list(ok_s)
        for i, v in pairs:
            a[i] = v
        return lib.cp_pose_depth_ransac(*a)

    INVALID, ALIGN = l_with(1, None), l_with(1, p + 2)
    assert INVALID != 0 and ALIGN not in (0, INVALID)
    assert [l_with(12, 0), l_with(12, 4097), l_with(3, 0), l_with(5, 8), l_with(8, 0), l_with(8, 3), l_with(9, 0), l_with(10, 0), l_with(11, -1),
            l_with(13, None), l_with(14, None), l_with(15, None), l_with(6, None)] == [INVALID] * 13
    assert [l_with(13, p + 2), l_with(15, p + 2), l_with(7, p + 2)] == [ALIGN] * 3
    assert l_with(11, 0) == 0                                                     # B == 0 returns without a launch
    assert [s_with((17, 0)), s_with((17, 257)), s_with((14, 4097)), s_with((14, 0)), s_with((15, 0.0)), s_with((15, -1.0)), s_with((15, float("nan"))),
            s_with((15, float("inf"))), s_with((1, None)), s_with((19, None)), s_with((20, None)), s_with((21, None)), s_with((22, None)),
            s_with((2, 3 * 512 - 1)), s_with((10, 3)), s_with((13, -1))] == [INVALID] * 16
    assert [s_with((19, p + 4)), s_with((22, p + 4)), s_with((16, p + 4)), s_with((21, p + 2))] == [ALIGN] * 4
    assert s_with((13, 0)) == 0 and s_with((13, 0), (15, float("nan")), (16, p)) == 0
