"""CPU: row N17 (graph-cut RANSAC pose solver).  The numpy restatement of tests/gc_stages.py against scipy's exact max-flow and
cKDTree, the stage checker on the restatement's own run (and that it catches what it claims to), the wrapper's refusals and the ABI's
argument checks (they return before any launch: no device is needed to reach them)."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

from tests import gc_stages as G
from tests.pnp_stages import StageError, lmo_model


def _random_graph(rng, n, p):
    adj = np.triu(rng.random((n, n)) < p, 1)
    adj = adj | adj.T
    return np.concatenate([[0], np.cumsum(adj.sum(1))]).astype(np.int32), np.nonzero(adj)[1].astype(np.int32)


def _random_problem(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    off, idx = _random_graph(rng, n, rng.choice([0.0, 0.1, 0.3, 1.0]))
    cin = rng.integers(0, 3 * G.Q, size=n)
    cin[rng.random(n) < 0.15] = -1
    cin[rng.random(n) < 0.1] = G.Q                            # ties between the two unary terms
    w = int(rng.choice([0, 1, G.weight(0.1), G.Q, 3 * G.Q]))
    return cin, off, idx, w


@pytest.mark.parametrize("seed", range(40))
def test_label_is_the_minimal_source_side_of_a_minimum_cut(seed):
    cin, off, idx, w = _random_problem(seed)
    lab, fv = G.label(cin, off, idx, w)
    assert not lab[cin < 0].any()
    assert G.cut_value(cin, off, idx, w, lab) == fv           # a cut of the flow's value: a minimum cut
    for v in np.nonzero(cin >= 0)[0]:                         # v is on the minimal source side iff more capacity v -> t means more flow
        more = cin.copy()
        more[v] += 1
        assert (G.label(more, off, idx, w)[1] > fv) == bool(lab[v]), v
    # the device's procedure on one lane ends on the same set and value
    lab2, fv2, sweeps = G.count_sweeps(cin, off, idx, w)
    assert np.array_equal(lab2, lab) and fv2 == fv and 16 * sweeps <= G.MAX_SWEEPS


def test_label_known_answers():
    off, idx = np.array([0, 0, 0, 0], np.int32), np.zeros(0, np.int32)
    lab, fv = G.label(np.array([0, G.Q, G.Q - 1]), off, idx, G.weight(0.1))
    assert lab.tolist() == [True, False, True] and fv == 0 + G.Q + G.Q - 1      # cin == Q: an outlier
    # a star: the centre alone would be an outlier (cin = 1.5 Q), its 8 inlier leaves (w = 0.1 Q each) flip it
    n = 9
    off = np.array([0, 8] + list(range(9, 17)), np.int32)
    idx = np.array(list(range(1, 9)) + [0] * 8, np.int32)
    cin = np.array([G.Q + G.Q // 2] + [0] * 8)
    assert G.label(cin, off, idx, G.weight(0.1))[0].all()
    assert G.label(cin, off, idx, G.weight(0.05))[0].tolist() == [False] + [True] * 8
    assert G.label(cin, off, idx, 0)[0].tolist() == [False] + [True] * 8
    assert n == len(cin)


def test_hand_built_label_cases_on_one_lane():
    """the inputs of the device's labelling tests: the device's procedure, restated on one lane, ends on scipy's cut within a
    sixteenth of the kernel's sweep bound; the named cases do what their names say"""
    cases = G.label_cases()
    worst = 0
    for name, (cin, off, idx, w) in cases.items():
        for b in range(len(cin)):
            lab, fv = G.label(cin[b], off, idx, w)
            if name != "n4096_deg8":
                lab2, fv2, sweeps = G.count_sweeps(cin[b], off, idx, w)
                assert np.array_equal(lab, lab2) and fv == fv2, (name, b)
                worst = max(worst, sweeps)
        if name == "star_flipped":
            assert lab.all()
        if name == "star_kept":
            assert not lab[0] and lab[1:].all()
        if name == "all_inlier":
            assert lab.all()
        if name == "all_outlier":
            assert not lab.any()
        if name == "cin_equals_Q":
            assert lab.tolist() == [i % 3 != 0 for i in range(64)]
    assert np.diff(cases["n4096_deg8"][1]).mean() > 6 and np.diff(cases["ape_512"][1]).max() == 56
    print("largest sweep count over the hand-built cases: %d" % worst)
    assert 16 * worst <= G.MAX_SWEEPS


def _cloud(seed, n, radius):
    rng = np.random.default_rng(seed)
    while True:                                               # refuse any pair within 1e-9 relative of radius^2
        x = rng.uniform(-40, 40, size=(n, 3)).astype(np.float32)
        if n < 2 or G.min_margin(x, radius) > 1e-9:
            return x


@pytest.mark.parametrize("n,radius", [(1, 20.0), (2, 20.0), (65, 20.0), (300, 20.0), (300, 0.0), (64, 1000.0)])
def test_radius_graph_restatement_equals_ckdtree(n, radius):
    x = _cloud(n, n, radius)
    off, idx = G.radius_graph_np(x, radius)
    tree = cKDTree(x.astype(np.float64))
    for i, nb in enumerate(tree.query_ball_point(x.astype(np.float64), radius)):
        assert idx[off[i]:off[i + 1]].tolist() == sorted(j for j in nb if j != i), i
    assert off[-1] == len(idx)
    if radius == 0.0:
        assert len(idx) == 0
    if radius == 1000.0:
        assert len(idx) == n * (n - 1)


def test_ape_graph_matches_the_issue_table():
    off, idx = G.radius_graph_np(lmo_model(512), 20.0)
    deg = np.diff(off)
    assert (deg.min(), deg.max(), len(idx)) == (23, 56, 18320) and round(deg.mean()) == 36


@pytest.mark.parametrize("name", list(G.CASES) + list(G.EDGE_CASES))
def test_committed_cases_keep_the_makers_promises(name):
    """what the stage checker presumes of a case, from the oracle alone: every four-point sample well posed (stage A), the unary
    term decisive under the true pose (stage G); the degenerate clouds promise nothing"""
    gc = G.CASES[name]() if name in G.CASES else G.EDGE_CASES[name]()
    if name in G.CASES:
        gc.assert_well_posed()
        gc.assert_unary_decides()
    assert gc.N <= 4096 and all(len(idx) <= 1 << 21 for _, idx in gc.graphs)


def test_well_posed_refuses_a_near_multiple_root():
    gc = G.GcCase(S_columns_seed_40(0), G.EXACT_LAM)
    p3, p2, va, K = gc.case.crop(1)
    vid = np.nonzero(va)[0]
    from oracle import pnp_oracle as P
    assert not G.well_posed(p3, p2, K, vid[P.sample_indices(40, 1, 25, len(vid), 4)])
    assert G.well_posed(p3, p2, K, vid[P.sample_indices(40, 1, 24, len(vid), 4)])


def S_columns_seed_40(column):
    from tests import pnp_stages
    return pnp_stages._columns(column)


@pytest.fixture(scope="module")
def small_run():
    gc = G.CASES["shape_4x33"]()
    outs = G.restatement_outputs(gc)
    stages = {k: np.stack([o[4][k] for o in outs]) for k in ("hypotheses", "steps", "cin", "labels")}
    return gc, stages, np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs]), np.array([o[3] for o in outs])


def test_checker_passes_on_the_restatement(small_run):
    gc, stages, R, t, inl, status = small_run
    total = G.check_case(gc, stages, R, t, inl, status)
    assert total["status1"] == gc.B and total["all_inlier"] > 0 and total["steps"] >= gc.B


@pytest.mark.parametrize("stage,tamper", [
    ("A", lambda s, R, t, i: s["hypotheses"].__setitem__((0, 70, 0), 3.0)),                    # a record behind the stopping rule
    ("B", lambda s, R, t, i: s["hypotheses"].__setitem__((0, 1, 1), s["hypotheses"][0, 1, 1] * (1 + 1e-6))),
    ("C", lambda s, R, t, i: s["steps"].__setitem__((0, 0, 13), s["steps"][0, 0, 13] + 1.0)),
    ("D", lambda s, R, t, i: s["cin"].__setitem__((0, 0, 3), s["cin"][0, 0, 3] + 2)),
    ("E", lambda s, R, t, i: s["labels"].__setitem__((0, 1, 0), 1 - s["labels"][0, 1, 0])),
    ("F", lambda s, R, t, i: s["steps"].__setitem__((0, 0, 27), s["steps"][0, 0, 27] * (1 + 1e-5))),
    ("C", lambda s, R, t, i: t.__setitem__((0, 2), t[0, 2] + 1e-9)),
])
def test_checker_catches(small_run, stage, tamper):
    gc, stages, R, t, inl, status = small_run
    stages = {k: v.copy() for k, v in stages.items()}
    R, t, inl = R.copy(), t.copy(), inl.copy()
    tamper(stages, R, t, inl)
    with pytest.raises(StageError) as e:
        G.check_case(gc, stages, R, t, inl, status)
    assert e.value.stage == stage and e.value.crop == 0


def test_abi_argument_checks_return_before_any_launch(lib):
    assert lib.cp_version() >= 218
    one, N = C.c_void_p(64), 512

    def logged(fn, *a):
        lib.cp_kernel_log_begin()
        rc = fn(*a)
        assert lib.cp_kernel_log() == b"", a
        return rc
    # cp_radius_graph_count / _fill
    cnt = lambda **k: logged(lib.cp_radius_graph_count, None, k.get("pts", one), k.get("M", 1), k.get("N", N), k.get("r", 20.0),
                             k.get("off", one), k.get("tot", one))                                                   # noqa: E731
    assert cnt(N=0) == -1 and cnt(N=4097) == -1 and cnt(M=0) == -1 and cnt(r=-1.0) == -1 and cnt(r=float("nan")) == -1 and cnt(r=float("inf")) == -1
    for name in ("pts", "off", "tot"):
        assert cnt(**{name: None}) == -1, name
    assert cnt(off=C.c_void_p(66)) == -3
    fill = lambda **k: logged(lib.cp_radius_graph_fill, None, k.get("pts", one), k.get("M", 1), k.get("N", N), k.get("r", 20.0),
                              k.get("off", one), k.get("base", one), k.get("idx", one), k.get("n", 100))             # noqa: E731
    assert fill(N=0) == -1 and fill(N=4097) == -1 and fill(M=0) == -1 and fill(r=-1.0) == -1 and fill(n=-1) == -1 and fill(n=(1 << 21) + 1) == -1
    for name in ("pts", "off", "base", "idx"):
        assert fill(**{name: None}) == -1, name
    assert fill(base=C.c_void_p(68)) == -3
    # cp_graphcut_label
    lab = lambda **k: logged(lib.cp_graphcut_label, None, k.get("cin", one), k.get("off", one), k.get("idx", one), k.get("B", 2), k.get("N", N),
                             k.get("E", 1000), k.get("w", 6554), k.get("lab", one), k.get("flow", one), k.get("st", one), k.get("sw", one),
                             k.get("scr", one), k.get("nb", 2 * 1000 * 4))                                           # noqa: E731
    assert lab(B=0) == -1 and lab(N=0) == -1 and lab(N=4097) == -1 and lab(E=-1) == -1 and lab(E=(1 << 21) + 1) == -1
    assert lab(w=-1) == -1 and lab(w=(1 << 28) + 1) == -1 and lab(nb=2 * 1000 * 4 - 1) == -1
    for name in ("cin", "off", "idx", "lab", "flow", "st", "scr"):
        assert lab(**{name: None}) == -1, name
    assert lab(flow=C.c_void_p(68)) == -3 and lab(st=C.c_void_p(66)) == -3
    # cp_pnp_gc
    def gc(**k):
        a = dict(p3d=one, p3d_bs=0, p2d=one, valid=one, vs=3, K=one, K_bs=0, off=one, idx=one, base=one, gid=None, M=1, me=18320, ni=18320,
                 B=2, N=N, thr=2.0, w=6554, it=400, mi=6, pose=one, inl=one, status=one, scratch=one)
        a.update(k)
        return logged(lib.cp_pnp_gc, None, a["p3d"], a["p3d_bs"], a["p2d"], a["valid"], a["vs"], a["K"], a["K_bs"], a["off"], a["idx"], a["base"],
                      a["gid"], a["M"], a["me"], a["ni"], a["B"], a["N"], a["thr"], a["w"], a["it"], a["mi"], 1, a["pose"], a["inl"], a["status"],
                      a["scratch"])
    assert gc(N=4097) == -1 and gc(N=0) == -1 and gc(B=0) == -1 and gc(vs=0) == -1
    assert gc(it=0) == -1 and gc(it=513) == -1 and gc(it=-5) == -1
    assert gc(thr=0.0) == -1 and gc(thr=float("nan")) == -1 and gc(w=-1) == -1 and gc(mi=3) == -1
    assert gc(M=0) == -1 and gc(M=2) == -1 and gc(me=-1) == -1 and gc(me=(1 << 21) + 1) == -1 and gc(ni=-1) == -1
    assert gc(p3d_bs=3 * N - 1) == -1 and gc(K_bs=8) == -1
    for name in ("p3d", "p2d", "valid", "K", "off", "idx", "base", "pose", "inl", "status", "scratch"):
        assert gc(**{name: None}) == -1, name
    assert gc(pose=C.c_void_p(68)) == -3 and gc(scratch=C.c_void_p(68)) == -3 and gc(status=C.c_void_p(66)) == -3 and gc(M=2, gid=C.c_void_p(66)) == -3
    # the scratch query: hypothesis records, step records, cin, labels, flows
    B, E = 3, 18320
    want = B * 512 * 14 * 8 + B * 9 * 30 * 8 + B * 9 * N * 4 + B * 9 * N
    assert lib.cp_pnp_gc_scratch_bytes(B, N, E) == (want + 7) // 8 * 8 + B * E * 4
    assert lib.cp_pnp_gc_scratch_bytes(B, N, 0) == (want + 7) // 8 * 8 + B * 4
    assert lib.cp_pnp_gc_scratch_bytes(0, N, E) == 0 and lib.cp_pnp_gc_scratch_bytes(B, 4097, E) == 0 and lib.cp_pnp_gc_scratch_bytes(B, N, (1 << 21) + 1) == 0


def test_wrapper_refusals():
    from checkerpose_amd import postprocess as PP
    p3, p2, va, K = torch.zeros(8, 3), torch.zeros(2, 8, 2), torch.ones(2, 8, 3, dtype=torch.uint8), torch.eye(3)
    z = torch.zeros
    graph = PP.RadiusGraph(z(1, 9, dtype=torch.int32), z(1, dtype=torch.int32), z(1, dtype=torch.int64), [0], 20.0)
    two = PP.RadiusGraph(z(2, 9, dtype=torch.int32), z(1, dtype=torch.int32), z(2, dtype=torch.int64), [0, 0], 20.0)
    for bad in (dict(iterations=0), dict(iterations=513), dict(iterations=-1), dict(column=3), dict(column=-1), dict(min_inliers=3),
                dict(spatial_coherence_weight=-0.1), dict(spatial_coherence_weight=float("nan")), dict(reproj_threshold=0.0)):
        with pytest.raises(ValueError):
            PP.solve_pnp_gc(p3, p2, va, K, graph, **bad)
    for bad_valid in (va[:, :, :2], va[:, :7], va[:1], va.float()):
        with pytest.raises(ValueError):
            PP.solve_pnp_gc(p3, p2, bad_valid, K, graph)
    with pytest.raises(ValueError, match="RadiusGraph"):
        PP.solve_pnp_gc(p3, p2, va, K, None)
    with pytest.raises(ValueError, match="graph_ids"):
        PP.solve_pnp_gc(p3, p2, va, K, two)
    with pytest.raises(ValueError, match="keypoints"):
        PP.solve_pnp_gc(torch.zeros(7, 3), p2[:, :7], va[:, :7], K, graph)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # well-formed arguments on the host: still no fallback
        PP.solve_pnp_gc(p3, p2, va, K, graph)
    for bad in (torch.zeros(8, 2), torch.zeros(4097, 3), torch.zeros(0, 3)):
        with pytest.raises(ValueError):
            PP.radius_graph(bad)
    with pytest.raises(ValueError):
        PP.radius_graph(p3, radius=-1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.radius_graph(p3, device="cpu")
    with pytest.raises(ValueError, match="solver"):
        PP.estimate_poses(None, torch.zeros(4, 4, 3, dtype=torch.uint8), [], p3, K, solver="progx")
    with pytest.raises(ValueError, match="graph"):
        PP.estimate_poses(None, torch.zeros(4, 4, 3, dtype=torch.uint8), [], p3, K, solver="gc")


def test_from_id_to_pose_without_a_backend_still_refuses_progressivex():
    from checkerpose_amd.postprocess import from_id_to_pose
    xyz = np.zeros((8, 3), np.float32)
    roi_xy, bit, ids = np.zeros((4, 4, 2), np.float32), np.ones((8, 1), np.float32), np.zeros(8, np.int64)
    with pytest.raises(ValueError, match="progx_backend"):
        from_id_to_pose(xyz, roi_xy, np.eye(3), bit, ids, ids, use_progressivex=True)
    with pytest.raises(ValueError, match="progx_backend"):
        from_id_to_pose(xyz, roi_xy, np.eye(3), bit, ids, ids, use_progressivex=True, progx_backend="flann")
    R, t = from_id_to_pose(xyz, roi_xy, np.eye(3), np.zeros((8, 1), np.float32), ids, ids, use_progressivex=True, progx_backend="device")
    assert np.array_equal(R, np.eye(3)) and not t.any()             # fewer than 6 valid points: the identity, no device touched
