"""CPU: row N26's rule in numpy (tests/verify_stages.py) -- its tamperings, score_of and select on hand-made inputs, what the committed
cases cover, the selection cases' gaps --, the library's host halves with fake pointers, and the Python layer's refusals, defaults and
estimate_poses_verified's routing with stubs (no device)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import icp_stages as I
from tests import verify_stages as VS
from tests.pnp_stages import StageError


def _run(name):
    """a committed case on the CPU: (case, render_f32 renders, the rule's outputs); both cached by verify_stages, left unchanged"""
    case = VS.make(name)
    D = VS.cpu_renders(case)
    return case, D, VS.reference(case, D)


# ------------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("tamper", VS.TAMPERINGS)
def test_tamperings_are_caught(tamper):
    """ONE rule changed: some committed case's counts or choice change, and check_case refuses the changed outputs"""
    changed = []
    for name in VS.CASES:
        case, D, good = _run(name)
        bad = VS.reference(case, D, (tamper,))
        if not np.array_equal(good["counts"], bad["counts"]) or (good["choice"] is not None and not np.array_equal(good["choice"], bad["choice"])):
            changed.append(name)
            with pytest.raises(StageError):
                VS.check_case(case, D, bad)
    assert changed, tamper
    print(tamper, "changes", changed)


def test_tamperings_listed():
    assert len(VS.TAMPERINGS) >= 6 and set(VS.TAMPERINGS) >= {"strict", "swap", "nan_zero", "round", "no_weight", "last_tie"}


@pytest.mark.parametrize("name", list(VS.CASES) + list(VS.SELECTION))
def test_classes_partition_the_model_pixels(name):
    """every pixel with D > 0 is in exactly one class, none other is; `through` is d > tau; q lies in 0..63 and is 0 off the matches"""
    case, D, out = _run(name)
    VS.check_case(case, D, out)
    S = case.sensor(D)
    for b in range(case.P):
        lab, n = out["labels"][b], out["counts"][b]
        if not case.counted(b):
            assert not lab.any() and not n.any() and np.isnan(out["score"][b]) and not out["ok"][b]
            continue
        assert np.array_equal(lab != 0, D[b] > 0)
        assert n[0] == n[1] + n[2] + n[3] + n[4] == (D[b] > 0).sum()
        with np.errstate(invalid="ignore"):
            d = S[case.image_of(b)].astype(np.float32) - D[b]
            tau = np.float32(case.tau_of(b))
            assert np.array_equal(lab == VS.THROUGH, (D[b] > 0) & (d > tau) & np.isfinite(S[case.image_of(b)]))
            assert np.array_equal(lab == VS.OCCLUDED, (D[b] > 0) & (d < -tau) & (S[case.image_of(b)] > 0))
        _, q = VS.classify(D[b], S[case.image_of(b)], case.tau_of(b))
        assert q.min() >= 0 and q.max() <= 63 and not q[lab != VS.MATCH].any() and q.sum() == n[5]
        if out["ok"][b]:
            assert 0.0 <= out["score"][b] <= 1.0


def test_classify_by_hand():
    D = np.array([[0.0, 100.0, 100.0, 100.0, 100.0, 100.0, 100.0, 100.0, 100.0, 100.0]], np.float32)
    S = np.array([[50.0, 100.0, 104.0, 96.0, 104.5, 90.0, 0.0, np.nan, np.inf, -3.0]], np.float32)
    lab, q = VS.classify(D, S, 4.0)
    assert lab.tolist() == [[0, 1, 1, 1, 3, 2, 4, 4, 4, 4]]
    assert q.tolist() == [[0, 0, 63, 63, 0, 0, 0, 0, 0, 0]]                    # a == tau: 64 clamped to 63
    lab, q = VS.classify(np.full((1, 4), 100.0), np.array([[101.0, 99.0, 102.99, 103.0]]), 4.0)
    assert lab.tolist() == [[1, 1, 1, 1]] and q.tolist() == [[16, 16, 47, 48]]      # truncated: 2.99 / 4 * 64 = 47.8
    assert VS.classify(np.full((1, 1), 100.0), np.array([[102.99]]), 4.0, ("round",))[1].tolist() == [[48]]
    assert VS.classify(D, S, 4.0, ("strict",))[0].tolist() == [[0, 1, 3, 3, 3, 2, 4, 4, 4, 4]]
    assert VS.classify(D, S, 4.0, ("swap",))[0].tolist() == [[0, 1, 1, 1, 2, 3, 4, 4, 4, 4]]
    assert VS.classify(D, S, 4.0, ("nan_zero",))[0].tolist() == [[0, 1, 1, 1, 3, 2, 4, 2, 4, 4]]
    assert VS.counts_of(*VS.classify(D, S, 4.0)).tolist() == [9, 4, 3, 1, 1, 126]


def test_score_of_hand_made_counts():
    s, fit, den, ok = VS.score_of([10, 1, 4, 2, 3, 64], 1.0)
    assert (fit, den, ok) == (3.0, 9.0, True) and s == 3.0 / 9.0
    s, fit, den, ok = VS.score_of([10, 1, 4, 2, 3, 64], 0.5)
    assert (fit, den, s) == (3.0, 8.0, 0.375)
    assert VS.score_of([10, 1, 4, 2, 3, 64], 0.0)[0] == 3.0 / 7.0 and VS.score_of([10, 1, 4, 2, 3, 64], 0.0, tamper=("no_weight",))[0] == 3.0 / 9.0
    assert VS.score_of([5, 0, 5, 0, 0, 0])[0] == 1.0 and VS.score_of([5, 0, 5, 0, 0, 5 * 63])[0] == 1.0 / 64.0
    for counts, w in (([0] * 6, 1.0), ([7, 7, 0, 0, 0, 0], 1.0), ([7, 0, 0, 7, 0, 0], 0.0)):      # nothing, all missing, all occluded at weight 0
        s, fit, den, ok = VS.score_of(counts, w)
        assert np.isnan(s) and den == 0.0 and fit == 0.0 and not ok
    s, fit, den, ok = VS.score_of([7, 0, 0, 7, 0, 0], 1.0)
    assert (s, den, ok) == (0.0, 7.0, True)
    s, fit, den, ok = VS.score_of([10, 1, 4, 2, 3, 64], 1.0, counted=False)
    assert np.isnan(s) and not ok and den == 9.0
    big = [1 << 24, 0, 1 << 24, 0, 0, 63 << 24]                                  # the largest sums a 2^24-pixel frame allows: exact in float64
    assert VS.score_of(big)[1] == float((1 << 24) - 63 * (1 << 24) // 64) and 63 << 24 < 2 ** 31


def test_select_ties_nan_and_fallback():
    nan = float("nan")
    score = np.array([[0.5, 0.2, nan, 0.9, nan, 0.3],
                      [0.7, 0.2, 0.1, 0.9, nan, 0.3],
                      [0.7, 0.1, 0.4, 0.1, nan, 0.8]])
    ok = np.ones((3, 6), bool)
    ok[2, 5] = False
    assert VS.select(score, ok).tolist() == [1, 0, 2, 0, 0, 0]                   # first of the equals; NaN never wins; none: 0; ok = 0: out
    assert VS.select(score, ok, ("last_tie",)).tolist() == [2, 1, 2, 1, 0, 1]
    assert VS.select(score[:1], ok[:1]).tolist() == [0] * 6
    assert VS.select(np.array([[-np.inf], [np.inf]]), np.ones((2, 1), bool)).tolist() == [1]
    assert VS.select(np.array([[0.9], [0.1]]), np.array([[False], [True]])).tolist() == [1]
    assert VS.select(np.array([[0.9], [0.1]]), np.zeros((2, 1), bool)).tolist() == [0]


def test_what_the_cases_cover():
    cases = [VS.make(n) for n in VS.CASES]
    assert {c.P for c in cases} >= {1, 3, 5}
    assert any(c.K.ndim == 3 for c in cases) and any(c.K.ndim == 2 for c in cases)
    assert any(np.ndim(c.tau) for c in cases) and any(not np.ndim(c.tau) for c in cases)
    assert {c.occlusion_weight for c in cases} >= {1.0, 0.5, 0.0}
    assert any(c.mesh_ids is not None and c.image_ids is not None and len(set(c.image_ids)) < c.P and len(set(c.mesh_ids)) < c.P for c in cases)
    assert {m for c in cases for m in c.meshes} >= {"torus", "ico80", "box"} and all(c.size == I.SIZE == (96, 80) for c in cases)
    d = VS.make("mixed_3").depth
    assert np.isnan(d).any() and np.isinf(d).any() and (d == 0).any() and (d < 0).any() and (d == 150).any() and (d == 900).any()
    out = _run("mixed_5")[2]["counts"]
    assert (out[:, 1] > 0).any()                                                # missing
    assert (out[:, 3] > 0).any() and (out[:, 4] > 100).any() and (out[:, 5] > 0).any()      # occluded (the slab), through (the far plane), q
    # the edge cases, pose by pose
    case, D, e = _run("edges_8")
    xs = np.nonzero((D[0] > 0).any(0))[0]
    assert xs.max() == I.SIZE[0] - 1 and e["ok"][0]                              # partly off the frame: cut at the right edge
    assert VS.rendered(case, 1) and not D[1].any() and e["counts"][1, 0] == 0    # wholly off the frame: rendered, n_model = 0
    assert not VS.rendered(case, 2) and VS.rendered(case, 3) and case.status[3] == 0 and case.image_ids[4] >= case.n_img
    assert not VS.rendered(case, 5) and case.tau[6] == 0.0
    assert np.isnan(e["score"][1:7]).all() and not e["ok"][1:7].any() and not e["counts"][1:7].any() and e["ok"][7]
    # the exact ties: nearly every model pixel, on both sides
    case, D, t = _run("tie_1")
    S = case.sensor(D)[0]
    on = D[0] > 0
    assert (np.abs(S - D[0])[on] == np.float32(4.0)).mean() > 0.9 and ((S - D[0])[on] > 0).any() and ((S - D[0])[on] < 0).any()
    assert t["counts"][0, 2] == t["counts"][0, 0] and t["counts"][0, 5] >= 63 * 0.9 * t["counts"][0, 0]
    assert VS.reference(case, D, ("strict",))["counts"][0, 2] < 0.1 * t["counts"][0, 0]
    # the selections
    assert _run("occluder_weight")[2]["choice"].tolist() == [0]
    ow = VS.make("occluder_weight")
    assert VS.reference(ow, VS.cpu_renders(ow), ("no_weight",))["choice"].tolist() == [1]
    ts = _run("tie_select")[2]
    assert ts["choice"].tolist() == [1, 0] and ts["score"][2] == ts["score"][4] > ts["score"][0]


def test_selection_cases():
    """tests/icp_stages.py's CPU refinement against its start pose under the numpy rule alone: the refined pose of the converging cases
    leads by at least 0.05 on every crop; on the triangle cases the start pose scores at least as high -- by at least 0.05 where the
    two poses differ at all (triangle_1_g8 is passed through by N24: equal scores, the tie goes to candidate 0)"""
    seen = set()
    for name, (icp_name, idx, tau, want) in VS.SELECTION.items():
        case, D, out = _run(name)
        s = out["score"].reshape(case.cand)
        gap = s[1] - s[0]
        print("%-24s tau %5.1f start %s refined %s gap %s choice %s" % (name, tau, np.round(s[0], 4).tolist(), np.round(s[1], 4).tolist(),
                                                                        np.round(gap, 4).tolist(), out["choice"].tolist()))
        assert out["ok"].all() and out["choice"].tolist() == [want] * len(idx)
        if icp_name in I.CONVERGING:
            assert want == 1 and (gap >= 0.05).all()
            seen.add("converging")
        else:
            assert want == 0 and icp_name.startswith("triangle") and (s[0] >= s[1]).all()
            same = np.array([np.array_equal(case.R[b], case.R[b + len(idx)]) and np.array_equal(case.t[b], case.t[b + len(idx)]) for b in range(len(idx))])
            assert (gap[~same] <= -0.05).all() and (gap[same] == 0.0).all()
            seen.add("same" if same.all() else "drifting")
    assert seen == {"converging", "drifting", "same"}


# ------------------------------------------------------------------------------------------------------------- the library
def test_abi_refusals():
    """the library on a CPU box: the new symbols resolve, the scratch sizing, refusals with fake pointers (nothing launches)"""
    from checkerpose_amd import _abi
    from checkerpose_amd import postprocess as PP
    lib = _abi.load()
    assert lib.cp_version() >= 236
    assert lib.cp_verify_poses_scratch_bytes(3, 64) == 384 + 3 * 64 * 16 and lib.cp_verify_poses_scratch_bytes(0, 64) == 0
    assert lib.cp_verify_poses_scratch_bytes(3, -1) == 0 and lib.cp_verify_poses_scratch_bytes(1, 0) == 128
    assert PP.VERIFY_COUNTS == VS.COUNTS and PP.VERIFY_MAX_PIXELS == 1 << 24 and PP.VERIFY_CMAX == 64
    buf = C.create_string_buffer(4096 + 16)
    p = (C.addressof(buf) + 15) & ~15
    #       0     1  2  3  4  5  6  7  8  9     10 11    12 13  14  15 16    17   18 19 20 21 22 23 24 25    26
    ok_a = [None, p, p, 0, p, p, p, p, 1, None, p, None, 1, 80, 96, p, None, 1.0, 3, 8, p, p, p, p, p, None, p]
    ok_b = [None, p, p, 3, 5, p]

    def a_with(*pairs):
        a = list(ok_a)
        for i, v in pairs:
            a[i] = v
        lib.cp_kernel_log_begin()
        rc = lib.cp_verify_poses(*a)
        assert lib.cp_kernel_log() == b""
        return rc

    def b_with(i, v):
        lib.cp_kernel_log_begin()
        rc = lib.cp_select_poses(*(ok_b[:i] + [v] + ok_b[i + 1:]))
        assert lib.cp_kernel_log() == b""
        return rc

    INVALID, ALIGN, RANGE = a_with((1, None)), a_with((1, p + 4)), a_with((13, 4097), (14, 4096))
    assert len({0, INVALID, ALIGN, RANGE}) == 4
    assert [a_with((i, None)) for i in (2, 4, 5, 6, 7, 10, 15, 20, 21, 22, 23, 24, 26)] == [INVALID] * 13
    assert [a_with((8, 0)), a_with((8, 2)), a_with((19, 0)), a_with((3, 4)), a_with((13, 0)), a_with((14, 0)), a_with((18, 0)), a_with((12, 0)),
            a_with((12, 2))] == [INVALID] * 9
    assert [a_with((17, w)) for w in (-0.5, 1.0001, float("nan"), float("inf"))] == [INVALID] * 4
    assert [a_with((26, p + 8)), a_with((2, p + 4)), a_with((15, p + 4)), a_with((21, p + 4)), a_with((22, p + 4)), a_with((23, p + 4)), a_with((4, p + 2)),
            a_with((9, p + 2)), a_with((10, p + 2)), a_with((11, p + 2)), a_with((16, p + 2)), a_with((20, p + 2))] == [ALIGN] * 12
    assert a_with((13, 0), (26, p + 8)) == INVALID and a_with((13, 4097), (14, 4096), (26, p + 8)) == ALIGN      # the classes' order
    assert [a_with((13, 1), (14, (1 << 24) + 1)), a_with((13, 4096), (14, 4096), (18, 1 << 12)), a_with((18, 1 << 20), (19, 1 << 12))] == [RANGE] * 3
    assert [b_with(1, None), b_with(5, None), b_with(3, 0), b_with(3, 65), b_with(4, 0), b_with(4, -1)] == [INVALID] * 6
    assert [b_with(1, p + 4), b_with(5, p + 2)] == [ALIGN] * 2
    lib.cp_kernel_log_begin()
    assert lib.cp_select_poses(None, p, p, 64, 1 << 25, p) == RANGE and lib.cp_kernel_log() == b""


# ------------------------------------------------------------------------------------------------------------- the Python layer
def _host_args():
    from checkerpose_amd.metric import MeshSet
    v, f = I.mesh_arrays(("box",))
    ms = MeshSet.from_arrays(v, faces=f)
    return dict(R=torch.eye(3, dtype=torch.float64)[None], t=torch.tensor([[0.0, 0.0, 300.0]], dtype=torch.float64), cam_K=torch.from_numpy(I.K_A),
                meshes=ms, depth=torch.full((80, 96), 300.0), tau=8.0)


def test_defaults_and_refusals():
    from checkerpose_amd import postprocess as PP
    sig = inspect.signature(PP.verify_poses).parameters
    assert list(sig) == ["R", "t", "cam_K", "meshes", "depth", "tau", "image_ids", "mesh_ids", "status", "occlusion_weight", "return_labels"]
    assert sig["tau"].default is inspect.Parameter.empty                        # NO default
    assert [sig[k].default for k in ("image_ids", "mesh_ids", "status", "occlusion_weight", "return_labels")] == [None, None, None, 1.0, False]
    assert str(inspect.signature(PP.select_poses)) == "(score, ok=None, R=None, t=None)"
    assert str(inspect.signature(PP.estimate_poses_verified)) == "(net, frames, Bboxes, p3d_xyz, cam_K, verify, return_verify=False, **estimate_kwargs)"
    a = _host_args()
    for name, bad in (("occlusion_weight", -0.1), ("occlusion_weight", 1.5), ("occlusion_weight", float("nan")), ("tau", 0.0), ("tau", -1.0),
                      ("tau", float("inf")), ("tau", float("nan")), ("tau", None)):
        with pytest.raises(ValueError, match=name):
            PP.verify_poses(**dict(a, **{name: bad}))
    with pytest.raises(TypeError):
        PP.verify_poses(a["R"], a["t"], a["cam_K"], a["meshes"], a["depth"])    # tau is required
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # well-formed arguments on the host: still no fallback
        PP.verify_poses(**a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.verify_poses(**dict(a, tau=torch.tensor([8.0])))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.select_poses(torch.zeros(2, 3, dtype=torch.float64))
    for bad in (torch.zeros(3), torch.zeros(65, 2), torch.zeros(0, 2), np.zeros((2, 3))):
        with pytest.raises(ValueError, match="score"):
            PP.select_poses(bad)
    s = torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="ok"):
        PP.select_poses(s, ok=torch.ones(3, 2, dtype=torch.bool))
    with pytest.raises(ValueError, match="ok"):
        PP.select_poses(s, ok=torch.ones(2, 3))
    with pytest.raises(ValueError, match="both"):
        PP.select_poses(s, R=torch.zeros(2, 3, 3, 3))
    with pytest.raises(ValueError, match="R must be"):
        PP.select_poses(s, R=torch.zeros(2, 3, 3, 3), t=torch.zeros(2, 3, 3))


PARENT_SIGNATURES = {         # every public function of postprocess at the parent commit: nothing lost, nothing reordered, no default changed
    "correspondences": "(outputs, roi_xy_ori=None, discard_bd_pixel=0, Bboxes=None)",
    "estimate_poses": "(net, frames, Bboxes, p3d_xyz, cam_K, img_index=None, obj_ids=None, padding_ratio=1.5, crop_size=256, resize_method='crop_square_resize', check_seg=False, discard_bd_pixel=0, reproj_threshold=2.0, iterations=150, seed=0, solver='epnp', graph=None, spatial_coherence_weight=0.1, prog_max_iters=400, refine=None, icp=None, depth=None, dist_threshold=None)",
    "evaluate_poses": "(net, frames, Bboxes, p3d_xyz, cam_K, R_gt, t_gt, vertices, mesh_ids=None, kinds=('add', 'adi'), symmetries=None, depth_test=None, image_ids=None, size=None, **estimate_kwargs)",
    "from_id_to_pose": "(p3d_xyz, roi_xy_ori, cam_K, roi_mask_bit, pixel_x_id, pixel_y_id, check_seg=False, seg_mask=None, use_progressivex=False, neighborhood_ball_radius=20, spatial_coherence_weight=0.1, prog_max_iters=400, discard_bd_pixel=0, return_inliers=False, reprojErr_thresh=2, cv_max_iters=150, device='cuda:0', seed=0, progx_backend=None, refine=None)",
    "graphcut_label": "(cin, offsets, indices, w)",
    "lift_correspondences": "(p2d, valid, cam_K, depth, image_ids=None, column=0)",
    "pose_covariance": "(info, sigma=None)",
    "radius_graph": "(p3d_xyz, radius=20.0, device='cuda:0')",
    "refine_poses_icp": "(R, t, cam_K, meshes, depth, max_dist, image_ids=None, mesh_ids=None, status=None, grid=32, max_iters=20, step_tol=1e-06, min_pairs=6, inertia=0.01, samples=None, return_records=False)",
    "refine_poses_lm": "(p3d_xyz, p2d, mask, cam_K, R, t, status=None, max_iters=20, step_tol=1e-10, return_records=False)",
    "solve_pnp_gc": "(p3d_xyz, p2d, valid, cam_K, graph, graph_ids=None, column=0, reproj_threshold=2.0, spatial_coherence_weight=0.1, iterations=400, min_inliers=6, seed=0, return_stages=False)",
    "solve_pnp_ransac": "(p3d_xyz, p2d, valid, cam_K, column=0, reproj_threshold=2.0, iterations=150, seed=0, return_hypotheses=False)",
    "solve_pose_depth": "(p3d_xyz, p2d, valid, cam_K, depth, dist_threshold, image_ids=None, column=0, iterations=150, seed=0, return_hypotheses=False)",
    "surface_samples": "(R, t, cam_K, meshes, size, mesh_ids=None, grid=32)",
}


def test_existing_signatures_are_unchanged():
    from checkerpose_amd import postprocess as PP
    for name, old in PARENT_SIGNATURES.items():
        assert str(inspect.signature(getattr(PP, name))) == old, name
    public = {n for n, f in vars(PP).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == PP.__name__}
    assert public == set(PARENT_SIGNATURES) | {"verify_poses", "select_poses", "estimate_poses_verified"}


def test_verify_values():
    from checkerpose_amd import postprocess as PP
    frames, p3d, K = torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(8, 3), torch.eye(3)
    for bad in (None, "yes", dict(meshes=None, depth=None), dict(meshes=None, tau=1.0), dict(depth=None, tau=1.0)):
        with pytest.raises(ValueError, match="verify"):
            PP.estimate_poses_verified(None, frames, [], p3d, K, bad)
    for key in ("image_ids", "status"):
        with pytest.raises(ValueError, match="img_index"):
            PP.estimate_poses_verified(None, frames, [], p3d, K, {"meshes": None, "depth": None, "tau": 1.0, key: [0]})
    with pytest.raises(ValueError, match="unknown"):
        PP.estimate_poses_verified(None, frames, [], p3d, K, dict(meshes=None, depth=None, tau=1.0, grid=8))
    ok = dict(meshes=None, depth=None, tau=1.0)
    with pytest.raises(ValueError, match="refine"):                              # estimate_poses' own refusals hold
        PP.estimate_poses_verified(None, frames, [], p3d, K, ok, refine="gn")
    with pytest.raises(TypeError):
        PP.estimate_poses_verified(None, frames, [], p3d, K, ok, no_such_keyword=1)
    with pytest.raises(TypeError):                                               # estimate_poses itself is as it was
        PP.estimate_poses(None, frames, [], p3d, K, verify=ok)
    with pytest.raises(ValueError, match="return_verify"):
        PP.evaluate_poses(None, frames, [], p3d, K, None, None, None, verify=ok, return_verify=True)
    assert "verify" not in inspect.signature(PP.from_id_to_pose).parameters       # no depth there: unchanged


def test_estimate_poses_verified_routes(monkeypatch):
    """the candidates' order, the ONE verify_poses and ONE select_poses call with their arguments and the gather, with stubs in place of
    every device call; estimate_poses runs what ran before"""
    from checkerpose_amd import metric
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import preprocess as PRE
    B = 2
    calls = []
    base_R = torch.arange(B * 9, dtype=torch.float64).reshape(B, 3, 3)
    base_t = torch.arange(B * 3, dtype=torch.float64).reshape(B, 3, 1)
    status = torch.tensor([1, 0], dtype=torch.int32)
    monkeypatch.setattr(PRE, "get_roi_batch", lambda *a, **k: "crops")
    monkeypatch.setattr(PP, "correspondences", lambda out, **k: ("p2d", "valid", None))
    monkeypatch.setattr(PP, "solve_pnp_ransac", lambda *a, **k: (base_R, base_t, "inl", status))

    def lm(p3d, p2d, mask, K, R, t, status=None):
        calls.append(("lm", R, t))
        return R + 100.0, t + 100.0, None, None

    def icp(R, t, K, meshes, depth, max_dist, **kw):
        calls.append(("icp", R, t))
        return R + 1000.0, t.reshape(-1, 3) + 1000.0, None, None             # (a (B,3) t: the stack reshapes it)

    def verify(R, t, K, meshes, depth, tau, **kw):
        calls.append(("verify", R, t, K, meshes, depth, tau, kw))
        P = R.shape[0]
        return torch.arange(P, dtype=torch.float64), dict(ok=torch.ones(P, dtype=torch.bool), marker="info")

    def select(score, ok, R, t):
        calls.append(("select", score, ok, R, t))
        choice = torch.tensor([score.shape[0] - 1, 0], dtype=torch.int32)
        return choice, R[choice.long(), torch.arange(B)], t[choice.long(), torch.arange(B)]

    monkeypatch.setattr(PP, "refine_poses_lm", lm)
    monkeypatch.setattr(PP, "refine_poses_icp", icp)
    monkeypatch.setattr(PP, "verify_poses", verify)
    monkeypatch.setattr(PP, "select_poses", select)
    frames = torch.zeros(2, 40, 40, 3, dtype=torch.uint8)
    K = np.stack([I.K_A, I.K_B])
    args = (lambda crops, _: "out", frames, [[5, 5, 10, 10], [6, 6, 10, 10]], "p3d", K)
    icp_spec = dict(meshes="M", depth="D", max_dist=7.0)
    spec = dict(meshes="VM", depth="VD", tau=torch.tensor([3.0, 4.0]), mesh_ids=[1, 0], occlusion_weight=0.25)

    # estimate_poses: exactly the calls of before, the last stage's pose
    out = PP.estimate_poses(*args, img_index=[1, 0], refine="lm+icp", icp=icp_spec)
    assert len(out) == 5 and [c[0] for c in calls] == ["lm", "icp"] and torch.equal(out[0], base_R + 1100.0)
    for refine, names, shift in ((None, ("solver",), (0.0,)), ("lm", ("solver", "lm"), (0.0, 100.0)), ("icp", ("solver", "icp"), (0.0, 1000.0)),
                                 ("lm+icp", ("solver", "lm", "icp"), (0.0, 100.0, 1100.0))):
        del calls[:]
        out = PP.estimate_poses_verified(*args, spec, return_verify=True, img_index=[1, 0], refine=refine, icp=icp_spec)
        R, t, inl, st, final, rep = out
        C_ = len(names)
        assert [c[0] for c in calls] == list(names[1:]) + ["verify", "select"]
        v, s = calls[-2], calls[-1]
        want_R = torch.cat([base_R + x for x in shift])
        want_t = torch.cat([base_t + x for x in shift])
        assert torch.equal(v[1], want_R) and torch.equal(v[2], want_t) and v[2].shape == (C_ * B, 3, 1)      # candidate-major, the stages' order
        assert np.array_equal(v[3], np.concatenate([K] * C_)) and v[4:6] == ("VM", "VD") and torch.equal(v[6], spec["tau"].repeat(C_))
        kw = v[7]
        assert sorted(kw) == ["image_ids", "mesh_ids", "occlusion_weight", "status"] and kw["occlusion_weight"] == 0.25
        assert list(kw["image_ids"]) == [1, 0] * C_ and list(kw["mesh_ids"]) == [1, 0] * C_ and torch.equal(kw["status"], status.repeat(C_))
        assert s[1].shape == (C_, B) and s[2].shape == (C_, B) and torch.equal(s[3], want_R.view(C_, B, 3, 3)) and torch.equal(s[4], want_t.view(C_, B, 3, 1))
        # the gather: crop 0 takes the last candidate, crop 1 the first
        assert torch.equal(R[0], base_R[0] + shift[-1]) and torch.equal(R[1], base_R[1]) and torch.equal(t[0], base_t[0] + shift[-1]) and torch.equal(t[1], base_t[1])
        assert inl == "inl" and st is status                                       # still the solver's
        assert rep["stages"] == names and rep["choice"].tolist() == [C_ - 1, 0] and rep["score"].shape == (C_, B) and rep["info"]["marker"] == "info"
        assert len(PP.estimate_poses_verified(*args, spec, img_index=[1, 0], refine=refine, icp=icp_spec)) == 5
    assert sorted(spec) == ["depth", "mesh_ids", "meshes", "occlusion_weight", "tau"]      # the caller's dict is left alone

    # without img_index and with one depth image per crop, the default rule is said before the crops are stacked; a number tau stays one
    del calls[:]
    PP.estimate_poses_verified(*args, dict(meshes="VM", depth=np.zeros((B, 4, 4), np.float32), tau=5.0), refine="lm")
    v = calls[-2]
    assert list(v[7]["image_ids"]) == [0, 1, 0, 1] and v[6] == 5.0 and v[7]["mesh_ids"] is None and v[7]["occlusion_weight"] == 1.0

    # evaluate_poses reaches it through its `verify` keyword and scores the chosen poses; without it, the last stage's
    seen = {}
    monkeypatch.setattr(metric, "score_poses", lambda R, t, *a, **k: seen.update(R=R) or "errors")
    res = PP.evaluate_poses(*args, "Rgt", "tgt", "verts", img_index=[1, 0], refine="lm", verify=spec)
    assert res[0] == "errors" and len(res) == 6 and torch.equal(seen["R"][0], base_R[0] + 100.0) and torch.equal(seen["R"][1], base_R[1])
    del calls[:]
    res = PP.evaluate_poses(*args, "Rgt", "tgt", "verts", img_index=[1, 0], refine="lm")
    assert [c[0] for c in calls] == ["lm"] and torch.equal(seen["R"], base_R + 100.0)
