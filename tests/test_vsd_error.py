"""Row N8 (BOP's VSD), host side.  tests/golden/vsd.npz holds what the REFERENCE's own bop_toolkit_lib.pose_error.vsd returned when its
renderer was a stub handing it the float64 oracle's depth (tests/golden/make_golden_vsd.py), the counts its visibility / distance
functions give, and misc.overlapping_sphere_projections' bit.  The stages of tests/vsd_stages.py are checked here against those
records and against each other -- they are the yardsticks of tests/test_gpu_vsd_error.py, which cannot read the reference:

  score(...)            reproduces every recorded count EXACTLY and the errors as the float64 quotients of the counts;
  oracle_render(...)    its nominal depth equals the recorded renders bit for bit; at most 5 % of the covered pixels are undecided;
  render_f32(...)       the fp32 restatement of the device's rasteriser stays within ONE QUARTER of the derived bounds
                        (vsd_stages' module docstring: eps = 32 * 2^-24 * (S + max(W, H)) pixels for an edge distance,
                        tol_d = 16 * 2^-24 * Z + 3 eps Zspan sum 1 / h for a depth).

Worst float32-restatement / bound ratios over the fixture (printed by test_float32_restatement_stays_within_a_quarter_of_the_bounds):
edge distance 0.053 of eps (at the samples that project onto the edge's segment, within min(2 px, the edge's length) of it), depth
0.032 of tol_d on the decided pixels; no pixel outside its interval; the largest undecided share of the covered pixels is 0.0079."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, metric
from tests import vsd_stages as S
from tests.common import golden

_CACHE = {}


def fixture():
    """(golden arrays, {mesh name: (verts, faces)}) -- built once, never modified"""
    if "g" not in _CACHE:
        g = golden("vsd")
        _CACHE["g"] = (g, S.meshes(g["hull_faces"].astype(np.int32)))
    return _CACHE["g"]


def mesh_of(c):
    g, meshes = fixture()
    return meshes[str(g["mesh_names"][g["mesh"][c]])]


def oracle(c, side):
    """oracle_render of fixture case c, side "est" / "gt": computed once, shared by every test that needs it"""
    if (c, side) not in _CACHE:
        g, _ = fixture()
        v, f = mesh_of(c)
        _CACHE[(c, side)] = S.oracle_render(g["R_" + side][c], g["t_" + side][c], g["K"][c], v, f, (int(g["W"][c]), int(g["H"][c])))
    return _CACHE[(c, side)]


def mesh_set():
    """the fixture's nine meshes as one MeshSet with faces, in vsd.npz's mesh order"""
    if "ms" not in _CACHE:
        g, meshes = fixture()
        names = [str(n) for n in g["mesh_names"]]
        _CACHE["ms"] = metric.MeshSet.from_arrays([meshes[n][0] for n in names], diameters=g["mesh_diameter"], faces=[meshes[n][1] for n in names])
    return _CACHE["ms"]


def n_cases():
    return len(fixture()[0]["mesh"])


def score_case(c, est=None, gt=None, **mut):
    g, _ = fixture()
    return S.score(g["test_%d" % c], g["est_%d" % c] if est is None else est, g["gt_%d" % c] if gt is None else gt, g["K"][c],
                   float(g["delta"][c]), g["taus"], bool(g["norm"][c]), float(g["mesh_diameter"][g["mesh"][c]]), **mut)


def test_fixture_covers_what_the_issue_lists():
    g, meshes = fixture()
    n = n_cases()
    assert n >= 24 and set(g["mesh"].tolist()) == set(range(9)) and [str(x) for x in g["mesh_names"]] == list(S.MESH_NAMES)
    assert [meshes[k][1].shape[0] for k in ("triangle", "box", "halfbox", "ico80", "ico1280", "ico20480")] == [1, 12, 8, 80, 1280, 20480]
    sizes = {(int(w), int(h)) for w, h in zip(g["W"], g["H"])}
    assert {(67, 45), (160, 120), (33, 31)} <= sizes and all(w <= 160 and h <= 120 and (w % 32 or h % 32) for w, h in sizes)
    assert set(g["delta"].tolist()) == {5.0, 15.0} and set(g["norm"].tolist()) == {True, False}
    assert len(set(g["kgroup"].tolist())) >= 3 and not g["sphere"].all() and g["sphere"].any()
    assert (g["counts"][:, 0] == 0).any()                                               # fully outside the frame: union 0 -> 1.0
    assert any(len(set(g["counts"][c, 2:].tolist())) >= 5 for c in range(n))            # cost counts that differ across the taus
    assert any((g["test_%d" % c] == 0).all() for c in range(n))                         # an all-zero test depth
    assert np.array_equal(g["taus"], np.arange(0.05, 0.51, 0.05))
    tri = meshes["zeroarea"]
    assert (tri[1][:, 0] == tri[1][:, 1]).any()                                         # a triangle of zero area


def test_scoring_restatement_reproduces_the_reference_exactly():
    g, _ = fixture()
    for c in range(n_cases()):
        counts, errors = score_case(c)
        assert np.array_equal(counts, g["counts"][c]), (c, counts, g["counts"][c])
        assert np.array_equal(errors, g["errors"][c]) and np.array_equal(S.errors_of(g["counts"][c]), g["errors"][c]), c
        if g["counts"][c, 0] == 0:
            assert (g["errors"][c] == 1.0).all()
        R = 0.5 * float(g["mesh_diameter"][g["mesh"][c]])
        assert S.sphere_overlap(R, g["t_est"][c], g["t_gt"][c]) == bool(g["sphere"][c]), c


def test_oracle_equals_the_recorded_renders_and_is_mostly_decided():
    g, _ = fixture()
    worst = 0.0
    for c in range(n_cases()):
        for side in ("est", "gt"):
            o = oracle(c, side)
            assert o["d"].dtype == np.float32 and np.array_equal(o["d"], g[side + "_%d" % c]), (c, side)
            share = S.undecided_share(o)
            worst = max(worst, share)
            assert share <= 0.05, (c, side, share)
            ok, ratio, nbad = S.check_render(o["d"], o)                                 # the oracle passes its own interval check
            assert ok and ratio == 0.0
    print("largest undecided share of the covered pixels: %.4f" % worst)


def test_float32_restatement_stays_within_a_quarter_of_the_bounds():
    g, _ = fixture()
    worst_d, worst_e = 0.0, 0.0
    for c in range(n_cases()):
        v, f = mesh_of(c)
        for side in ("est", "gt"):
            o = oracle(c, side)
            depth, dist_err = S.render_f32(g["R_" + side][c], g["t_" + side][c], g["K"][c], v, f, (int(g["W"][c]), int(g["H"][c])), want_dist=True)
            ok, ratio, nbad = S.check_render(depth, o)
            worst_d, worst_e = max(worst_d, ratio), max(worst_e, dist_err / o["eps"])
            assert nbad == 0 and ratio <= 0.25 and dist_err <= 0.25 * o["eps"], (c, side, nbad, ratio, dist_err / o["eps"])
    print("float32 restatement: worst |diff| / bound  edge distance %.4f  depth %.4f" % (worst_e, worst_d))


def test_mutations_of_the_checker_are_caught_under_their_stage():
    g, _ = fixture()
    hit = {"sample": 0, "cull": 0, "bop18": 0, "strict": 0}
    for c in range(n_cases()):
        v, f = mesh_of(c)
        size = (int(g["W"][c]), int(g["H"][c]))
        if c in (3, 6, 7):                                                              # render stage (a few cases: the oracle is slow)
            args = (g["R_gt"][c], g["t_gt"][c], g["K"][c], v, f, size)
            hit["sample"] += not np.array_equal(S.oracle_render(*args, sample=0.0)["d"], g["gt_%d" % c])
            hit["cull"] += not np.array_equal(S.oracle_render(*args, cull=True)["d"], g["gt_%d" % c])
        hit["bop18"] += not np.array_equal(score_case(c, mode="bop18")[0], g["counts"][c])  # scoring stage
        hit["strict"] += not np.array_equal(score_case(c, strict=True)[0], g["counts"][c])
    print("mutations caught (cases):", hit)
    assert hit["sample"] == 3 and hit["cull"] == 2 and hit["bop18"] >= 3           # culling: the open half box alone shows back faces
    assert not S.check_render(S.oracle_render(g["R_gt"][7], g["t_gt"][7], g["K"][7], *mesh_of(7), (96, 80), cull=True)["d"], oracle(7, "gt"))[0]
    assert not S.check_render(S.oracle_render(g["R_gt"][3], g["t_gt"][3], g["K"][3], *mesh_of(3), (67, 45), sample=0.0)["d"], oracle(3, "gt"))[0]
    # `>` instead of `>=` at tau: no recorded distance sits ON a tau (the fixture keeps 1e-6 away), so the stage is shown directly
    d = np.full((4, 4), 500.0, dtype=np.float32)
    K = np.array([[100.0, 0, 2.0], [0, 100.0, 2.0], [0, 0, 1.0]])
    e = d.copy()
    e[2, 2] = 750.0                                                                     # pixel (2, 2) is the principal point: dist = depth
    assert S.score(np.zeros_like(d), e, d, K, 15.0, [250.0], False, 1.0)[0].tolist() == [16, 16, 1]
    assert S.score(np.zeros_like(d), e, d, K, 15.0, [250.0], False, 1.0, strict=True)[0].tolist() == [16, 16, 0]


def test_thresholds_recall_and_ar():
    g, _ = fixture()
    assert np.array_equal(metric.bop_thresholds("vsd"), np.arange(0.05, 0.51, 0.05)) and len(metric.bop_thresholds("vsd")) == 10
    e = np.concatenate([g["errors"], np.full((1, 10), np.nan)], 0)
    r = metric.bop_recall(torch.from_numpy(e), "vsd")
    rec, ar = S.ar_vsd(e)
    assert r["recall"].shape == (10, 10) and np.array_equal(r["recall"], rec) and r["AR_VSD"] == ar and r["count"] == len(e)
    assert not r["correct"][-1].any()                                                   # NaN is a miss
    on = metric.bop_recall(np.array([[metric.bop_thresholds("vsd")[3]] * 10]), "vsd")   # an error exactly ON a threshold: strict
    assert on["correct"][0, 0].tolist() == [False] * 4 + [True] * 6
    ids = np.arange(len(e)) % 3
    pm = metric.bop_recall(e, "vsd", mesh_ids=ids)["per_mesh"]
    assert pm[1]["AR_VSD"] == S.ar_vsd(e[ids == 1])[1]
    with pytest.raises(ValueError):
        metric.bop_recall(e[:, 0], "vsd")
    n = len(e)
    rng = np.random.default_rng(3)
    mssd, mspd = rng.uniform(0, 60, n), rng.uniform(0, 60, n)
    s = metric.summarize_bop({"mssd": mssd, "mspd": mspd, "vsd": e}, diameters=100.0, im_width=640)
    assert sorted(s) == ["AR", "AR_MSPD", "AR_MSSD", "AR_VSD", "mspd", "mssd", "vsd"]
    assert s["AR_VSD"] == ar and s["AR"] == float(np.mean([ar, s["AR_MSSD"], s["AR_MSPD"]]))
    s2 = metric.summarize_bop({"mssd": mssd, "vsd": e}, diameters=100.0)
    assert sorted(s2) == ["AR_MSSD", "AR_VSD", "mssd", "vsd"]                            # no "AR" unless all three are there
    plain = metric.summarize_bop({"mssd": mssd, "mspd": mspd, "proj": mspd, "add": mspd}, diameters=100.0, im_width=640)
    assert sorted(plain) == ["AR_MSPD", "AR_MSSD", "mspd", "mssd"]                       # without "vsd": the keys it returned before
    assert plain["AR_MSSD"] == s["AR_MSSD"] and plain["AR_MSPD"] == s["AR_MSPD"]


def test_meshset_faces_and_argument_checks_without_a_device():
    ms = mesh_set()
    assert len(ms) == 9 and ms.faces.dtype == torch.int32 and ms.face_offsets.tolist()[:4] == [0, 1, 13, 21]
    plain = metric.MeshSet.from_arrays([np.ones((4, 3), np.float32)], diameters=[1.0])
    assert plain.faces is None and plain.face_offsets is None
    with pytest.raises(ValueError):
        metric.MeshSet.from_arrays([np.ones((4, 3))], diameters=[1.0], faces=[np.array([[0, 1, 4]])])       # an index past the mesh
    with pytest.raises(ValueError):
        metric.MeshSet.from_arrays([np.ones((4, 3))], diameters=[1.0], faces=[np.array([[0.0, 1.0, 2.0]])])
    with pytest.raises(ValueError):
        metric.MeshSet.from_arrays([np.ones((4, 3))] * 2, diameters=[1.0, 1.0], faces=[np.array([[0, 1, 2]])])
    with pytest.raises(ValueError, match="no faces"):
        plain.faces_on("cuda:0")
    R, t = torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3, 1, dtype=torch.float64)
    d = np.zeros((8, 8), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.vsd_errors(R, t, R, t, np.eye(3), ms, d, mesh_ids=[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.render_depth(R, t, np.eye(3), ms, (8, 8), mesh_ids=[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.vsd(np.eye(3), np.zeros(3), np.eye(3), np.zeros(3), d, np.eye(3), 15, [0.1], True, 100.0, ms, 1, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.vsd_from_depth(torch.zeros(1, 8, 8), torch.zeros(1, 8, 8), d, np.eye(3), 1.0)
    with pytest.raises(ValueError, match="step"):
        metric.vsd(np.eye(3), np.zeros(3), np.eye(3), np.zeros(3), d, np.eye(3), 15, [0.1], True, 100.0, ms, 1, cost_type="tlinear")
    with pytest.raises(ValueError, match="depth_test"):
        metric.score_poses(R, t, R, t, np.eye(3), ms, kinds=("vsd",))
    sig = inspect.signature(metric.vsd_errors)
    assert list(sig.parameters) == ["R_est", "t_est", "R_gt", "t_gt", "cam_K", "meshes", "depth_test", "image_ids", "delta", "taus",
                                    "normalized_by_diameter", "mesh_ids", "sphere_check", "return_counts", "return_depth"]
    assert sig.parameters["delta"].default == 15.0 and sig.parameters["sphere_check"].default is True
    assert list(inspect.signature(metric.vsd).parameters)[:13] == ["R_est", "t_est", "R_gt", "t_gt", "depth_test", "K", "delta", "taus",
                                                                   "normalized_by_diameter", "diameter", "renderer", "obj_id", "cost_type"]
    from checkerpose_amd import postprocess, targets
    for fn in (postprocess.evaluate_poses, targets.evaluate_batch, metric.score_poses):
        p = inspect.signature(fn).parameters
        assert p["depth_test"].default is None and p["image_ids"].default is None and p["kinds"].default == ("add", "adi")


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    p = C.c_void_p(4096)                                    # fake, aligned; never dereferenced: every call returns before a launch
    taus = (C.c_double * 10)(*np.arange(0.05, 0.51, 0.05).tolist())

    def vsd(est=p, gt=p, K=p, ks=9, verts=p, voff=p, faces=p, foff=p, M=2, ids=p, test=p, img=p, n_img=2, H=48, W=64, delta=15.0,
            diam=p, taus=taus, T=10, norm=1, sphere=1, B=2, Vmax=8, err=p, cnt=p, depth=None, scr=p):
        return lib.cp_vsd_errors(None, est, gt, K, ks, verts, voff, faces, foff, M, ids, test, img, n_img, H, W, delta, diam, taus, T, norm,
                                 sphere, B, Vmax, err, cnt, depth, scr)

    for name in ("est", "gt", "K", "verts", "voff", "faces", "foff", "test", "diam", "taus", "err", "cnt", "scr"):
        assert vsd(**{name: None}) == -1, name
    assert vsd(B=0) == -1 and vsd(M=0) == -1 and vsd(Vmax=0) == -1 and vsd(H=0) == -1 and vsd(W=-1) == -1 and vsd(n_img=0) == -1
    assert vsd(T=0) == -1 and vsd(T=17) == -1 and vsd(ks=3) == -1 and vsd(delta=float("nan")) == -1
    assert vsd(ids=None) == -1 and vsd(img=None) == -1                                  # several meshes / images need ids
    assert vsd(est=C.c_void_p(4100)) == -3 and vsd(scr=C.c_void_p(4104)) == -3 and vsd(faces=C.c_void_p(4098)) == -3
    assert vsd(depth=C.c_void_p(4098)) == -3
    assert vsd(B=1 << 20, H=480, W=640) == -4                                           # 2^20 x 300 tiles

    def fd(est=p, gt=p, K=p, ks=0, test=p, img=p, n_img=2, H=48, W=64, delta=15.0, diam=p, taus=taus, T=10, norm=1, B=2, err=p, cnt=p, scr=p):
        return lib.cp_vsd_from_depth(None, est, gt, K, ks, test, img, n_img, H, W, delta, diam, taus, T, norm, B, err, cnt, scr)

    for name in ("est", "gt", "K", "test", "diam", "taus", "err", "cnt", "scr"):
        assert fd(**{name: None}) == -1, name
    assert fd(B=0) == -1 and fd(T=17) == -1 and fd(ks=5) == -1 and fd(img=None) == -1 and fd(H=0) == -1
    assert fd(est=C.c_void_p(4098)) == -3 and fd(scr=C.c_void_p(4100)) == -3 and fd(B=1 << 20, H=480, W=640) == -4

    def rd(poses=p, K=p, ks=0, verts=p, voff=p, faces=p, foff=p, M=2, ids=p, H=48, W=64, B=2, Vmax=8, out=p, scr=p):
        return lib.cp_render_depth(None, poses, K, ks, verts, voff, faces, foff, M, ids, H, W, B, Vmax, out, scr)

    for name in ("poses", "K", "verts", "voff", "faces", "foff", "out", "scr"):
        assert rd(**{name: None}) == -1, name
    assert rd(B=0) == -1 and rd(Vmax=0) == -1 and rd(ids=None) == -1 and rd(ks=1) == -1 and rd(W=0) == -1
    assert rd(out=C.c_void_p(4098)) == -3 and rd(B=1 << 20, H=480, W=640) == -4
    assert lib.cp_vsd_errors_scratch_bytes(0, 8, 48, 64) == 0 and lib.cp_vsd_errors_scratch_bytes(1, -1, 48, 64) == 0
    assert lib.cp_vsd_errors_scratch_bytes(1, 8, 0, 64) == 0
    for B, V, H, W in ((1, 0, 31, 33), (1, 3, 31, 33), (2, 10242, 480, 640), (256, 10242, 480, 640)):
        n = lib.cp_vsd_errors_scratch_bytes(B, V, H, W)
        tiles = ((H + 31) // 32) * ((W + 31) // 32)
        assert n % 16 == 0 and n >= 160 * B + 32 * B * V + 72 * B * tiles
    assert lib.cp_version() >= 209
    for name in ("cp_vsd_errors", "cp_vsd_errors_scratch_bytes", "cp_vsd_from_depth", "cp_render_depth"):
        assert name in _abi.SIGNATURES
