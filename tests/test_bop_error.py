"""Row N7 (BOP's MSSD / MSPD / projection error and their recall), host side.  tests/golden/bop_error.npz holds what the REFERENCE's own
bop_toolkit_lib.pose_error.mssd / .mspd / .proj, misc.get_symmetry_transformations and pose_matching.match_poses returned
(make_golden_bop_error.py).  Two numpy restatements of cp_bop_errors' arithmetic live here -- the yardsticks of
tests/test_gpu_bop_error.py, which cannot read the reference:

  restate(..., np.float64)   must reproduce the recorded values within 64 * 2^-53 of the scales below;
  restate(..., np.float32)   (the per-(pose, symmetry) matrices rounded to fp32, the vertex loop in fp32) must stay within ONE QUARTER
                             of the device's bounds on every fixture case -- if it did not, the bounds would be wrong.

Bounds (derived, not tuned; eps = 2^-24):
  MSSD          |got - ref| <= 16 eps (2 r_max + max_s |d_s| + ref): N5's bound with the two terms the difference form has -- the
                entries of D_s = R_est - R_gs are each rounded once (|D_s p| error <= a few eps r_max, twice: the rounding of D_s and
                the fma chain), d_s = t_est - t_gs is rounded once, the norm a few eps of itself.
  MSPD / proj   |got - ref| <= 64 eps max_{P, v} (A_u + |u| A_z + A_v + |v| A_z) / |z| + 16 eps ref, with A_u, A_v, A_z the sums of
                absolute products in the three rows of P p_h, (u, v) the projection and z the third row: N6's projection bound at
                fp32.  A projection's error is a few eps of (A_u + |u| A_z) / |z| per coordinate, the difference of two projections
                carries two of them, and min_s max_v moves by at most the largest error of any (symmetry, vertex) pair -- so the
                maximum runs over the estimate's matrix and EVERY K [R_gs | t_gs] of the set (for proj: the estimate's and the
                ground truth's), not over the winning symmetry alone.
Worst float32-restatement / bound ratio over the fixture (printed by test_float32_restatement_stays_within_a_quarter_of_the_bounds):
MSSD 0.020, MSPD 0.015, proj 0.0070; the float64 one reaches 0.20 of its 64 * 2^-53 bound."""
import ctypes as C
import inspect
import json

import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, metric
from tests.common import golden
from tests.test_pose_error import lm_table, mesh_of

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
SET_SIZES = [1, 2, 4, 63, 64, 65, 628, 1256]
_CACHE = {}


def fixture():
    """(golden arrays, vertex table, the twin's symmetry sets as (S,12) float64 tables) -- built once, never modified"""
    if not _CACHE:
        g = golden("bop_error")
        sets = [metric.symmetry_transformations(json.loads(str(info)), float(step)) for info, step in zip(g["set_info"], g["set_step"])]
        tables = [np.stack([np.concatenate([t["R"].reshape(9), t["t"].reshape(3)]) for t in s]) for s in sets]
        _CACHE["v"] = (g, lm_table(), tables)
    return _CACHE["v"]


def compose(R_est, t_est, R_gt, t_gt, K, T):
    """the per-(pose, symmetry) numbers of bop_compose_kernel, in float64: D (S,3,3), d (S,3), Pe (3,4), Pg (S,3,4), Pgt (3,4)"""
    R_est, R_gt, K = (np.asarray(a, dtype=np.float64).reshape(3, 3) for a in (R_est, R_gt, K))
    t_est, t_gt = (np.asarray(a, dtype=np.float64).reshape(3) for a in (t_est, t_gt))
    Rs, ts = T[:, :9].reshape(-1, 3, 3), T[:, 9:]
    Rgs = R_gt[None] @ Rs
    tgs = ts @ R_gt.T + t_gt
    Pe = K @ np.concatenate([R_est, t_est[:, None]], 1)
    Pgt = K @ np.concatenate([R_gt, t_gt[:, None]], 1)
    Pg = K[None] @ np.concatenate([Rgs, tgs[:, :, None]], 2)
    return R_est[None] - Rgs, t_est[None] - tgs, Pe, Pg, Pgt


def _project(P, pts):
    q = pts @ P[..., :3].swapaxes(-1, -2) + P[..., None, :, 3]              # (..., V, 3)
    return q[..., :2] / q[..., 2:]


def restate(R_est, t_est, R_gt, t_gt, K, pts, T, dtype):
    """cp_bop_errors' arithmetic in numpy: compose in float64, cast to `dtype`, the vertex loop in `dtype`, maxima of squared
    distances, square roots / proj's sum in float64 -> (mssd, mspd, proj)"""
    D, d, Pe, Pg, Pgt = (a.astype(dtype) for a in compose(R_est, t_est, R_gt, t_gt, K, T))
    p = np.asarray(pts).astype(dtype)
    ue = _project(Pe, p)
    a2, c2 = [], []
    for s0 in range(0, T.shape[0], 64):                                     # chunks of symmetries: bounded temporaries
        e = p[None] @ D[s0:s0 + 64].swapaxes(1, 2) + d[s0:s0 + 64, None, :]
        a2.append((e * e).sum(2).max(1))
        du = _project(Pg[s0:s0 + 64], p) - ue[None]
        c2.append((du * du).sum(2).max(1))
    dg = _project(Pgt, p) - ue
    pr = np.sqrt((dg * dg).sum(1).astype(np.float64)).mean()
    return (float(np.sqrt(np.concatenate(a2).astype(np.float64)).min()), float(np.sqrt(np.concatenate(c2).astype(np.float64)).min()), float(pr))


def _px_scale(P, pts):
    """max_v (A_u + |u| A_z + A_v + |v| A_z) / |z| of one or a stack of 3x4 matrices, in float64"""
    ph = np.concatenate([pts, np.ones((pts.shape[0], 1))], 1)
    A = np.abs(ph) @ np.abs(P).swapaxes(-1, -2)                             # (..., V, 3): sums of absolute products
    q = ph @ P.swapaxes(-1, -2)
    u, v, z = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2], np.abs(q[..., 2])
    return float(((A[..., 0] + np.abs(u) * A[..., 2] + A[..., 1] + np.abs(v) * A[..., 2]) / z).max())


def scales(R_est, t_est, R_gt, t_gt, K, pts, T):
    """the three scales the bounds multiply: (2 r_max + max_s |d_s|, px scale of MSPD, px scale of proj) -- add `ref` yourself"""
    pts = np.asarray(pts, dtype=np.float64)
    D, d, Pe, Pg, Pgt = compose(R_est, t_est, R_gt, t_gt, K, T)
    r_max = float(np.linalg.norm(pts, axis=1).max())
    pe = _px_scale(Pe, pts)
    return 2.0 * r_max + float(np.linalg.norm(d, axis=1).max()), max(pe, _px_scale(Pg, pts)), max(pe, _px_scale(Pgt, pts))


def tolerances(sc, ref, eps=EPS32):
    """(MSSD, MSPD, proj) bounds of the module docstring from sc = scales(...) and the references ref = (mssd, mspd, proj);
    eps = 2^-53 gives the float64 check: 64 eps of the same scales"""
    s3, sp, sj = sc
    k = 4.0 if eps == EPS64 else 1.0
    return (16.0 * k * eps * (s3 + ref[0]), 64.0 * eps * sp + 16.0 * k * eps * ref[1], 64.0 * eps * sj + 16.0 * k * eps * ref[2])


def case_args(g, table, tables, c):
    return (g["R_est"][c], g["t_est"][c], g["R_gt"][c], g["t_gt"][c], g["K"][c], mesh_of(g, table, g["mesh"][c]), tables[g["set"][c]])


def case_tolerances(c, ref, eps=EPS32):
    """tolerances() of fixture case c, its scales computed once and shared by every test that needs them"""
    if ("scales", c) not in _CACHE:
        _CACHE[("scales", c)] = scales(*case_args(*fixture(), c))
    return tolerances(_CACHE[("scales", c)], ref, eps)


def test_fixture_covers_what_the_issue_lists():
    g, _, _ = fixture()
    assert g["set_size"].tolist() == SET_SIZES
    assert sorted(set(g["mesh_count"][:9].tolist())) == [1, 3, 63, 65, 1000, 4095, 4096, 9001, 20480]
    assert len(set(g["mesh_count"][9:].tolist())) == 13
    assert set(g["set"].tolist()) == set(range(8)) and len(g["mssd"]) >= 80
    for si, S in enumerate(SET_SIZES[1:], start=1):                          # every symmetric set: first, last, around 64 and the middle
        ks = set(g["k"][(g["set"] == si) & (g["k"] >= 0)].tolist())
        assert {k for k in (0, S - 1, 63, 64, S // 2 - 1, S // 2) if k < S} <= ks, (si, ks)
    own = g["group"] == 12
    assert len({tuple(k.reshape(-1)) for k in g["K"][own]}) == own.sum() > 1   # a per-pose K group
    for c in range(len(g["mssd"])):                                          # no recorded error near a threshold
        e = g["mssd"][c] / g["mesh_diameter"][g["mesh"][c]]
        assert (np.abs(e - g["th_mssd"]) >= 1e-3 * g["th_mssd"]).all() and (np.abs(g["mspd"][c] - g["th_mspd"]) >= 1e-3 * g["th_mspd"]).all()


def test_float64_restatement_reproduces_the_reference():
    g, table, tables = fixture()
    worst = 0.0
    for c in range(len(g["mssd"])):
        args = case_args(g, table, tables, c)
        ref = (g["mssd"][c], g["mspd"][c], g["proj"][c])
        got = restate(*args, np.float64)
        tol = case_tolerances(c, ref, eps=EPS64)
        for name, a, r, t in zip(("mssd", "mspd", "proj"), got, ref, tol):
            worst = max(worst, abs(a - r) / t)
            assert abs(a - r) <= t, (c, str(g["tag"][c]), name, a, r, t)
        if str(g["tag"][c]) == "0" and g["set"][c] in (0, 1, 2):
            assert got == (0.0, 0.0, 0.0) and ref == (0.0, 0.0, 0.0)
    print("float64 restatement: worst |diff| / bound %.3f" % worst)


def test_float32_restatement_stays_within_a_quarter_of_the_bounds():
    g, table, tables = fixture()
    worst = {"mssd": 0.0, "mspd": 0.0, "proj": 0.0}
    for c in range(len(g["mssd"])):
        args = case_args(g, table, tables, c)
        ref = (g["mssd"][c], g["mspd"][c], g["proj"][c])
        got = restate(*args, np.float32)
        tol = case_tolerances(c, ref)
        for name, a, r, t in zip(("mssd", "mspd", "proj"), got, ref, tol):
            worst[name] = max(worst[name], abs(a - r) / t)
            assert abs(a - r) <= 0.25 * t, (c, str(g["tag"][c]), name, a, r, t)
    print("float32 restatement: worst |diff| / bound  mssd %.4f  mspd %.4f  proj %.4f" % (worst["mssd"], worst["mspd"], worst["proj"]))


def test_symmetry_twin_sizes_and_the_missing_identity():
    g, _, tables = fixture()
    assert [t.shape[0] for t in tables] == g["set_size"].tolist() == SET_SIZES
    eye = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    for si, t in enumerate(tables):
        info = json.loads(str(g["set_info"][si]))
        has_identity = bool((np.abs(t - eye).max(1) < 1e-9).any())
        if "symmetries_continuous" in info:                                  # i = 1 .. count - 1: the identity is NOT in the set
            count = int(np.ceil(np.pi / float(g["set_step"][si])))
            assert t.shape[0] == (count - 1) * (1 + len(info.get("symmetries_discrete", ())))
            assert not has_identity, si
        else:
            assert has_identity and np.array_equal(t[0], eye)
    ss = metric.SymmetrySet.from_models_info([json.loads(str(i)) for i in g["set_info"][:3]])       # the default step
    assert ss.sizes.tolist() == [1, 2, 4] and ss.offsets.tolist() == [0, 1, 3, 7] and ss.table.dtype == torch.float64
    assert metric.SymmetrySet.from_models_info([json.loads(str(g["set_info"][6]))]).sizes.tolist() == [628]     # step 0.01 by default
    back = metric.SymmetrySet.from_transforms([ss.transforms(2)])
    assert torch.equal(back.table, ss.table[3:7])
    with pytest.raises(ValueError):
        metric.SymmetrySet.from_transforms([[]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ss.on("cpu")


def test_symmetry_twin_entries():
    g, _, tables = fixture()
    for si in (2, 5, 6):
        ref = g["set_T_%d" % si]
        info = json.loads(str(g["set_info"][si]))
        off = max([float(np.linalg.norm(c["offset"])) for c in info.get("symmetries_continuous", ())] + [0.0])
        assert ref.shape == tables[si].shape
        worst = float(np.abs(tables[si] - ref).max())
        print("set %d (S = %d): max |twin - reference| = %.3e" % (si, ref.shape[0], worst))
        assert worst <= 8.0 * EPS64 * (1.0 + off), (si, worst)


def test_recall_bits_equal_the_recorded_ones():
    g, _, _ = fixture()
    diam = g["mesh_diameter"]
    r3 = metric.bop_recall(g["mssd"], "mssd", diameters=diam, mesh_ids=g["mesh"])
    rp = metric.bop_recall(torch.from_numpy(g["mspd"]), "mspd", im_width=640)
    assert np.array_equal(r3["correct"], g["bits_mssd"]) and np.array_equal(rp["correct"], g["bits_mspd"])
    assert np.array_equal(r3["recall"], g["bits_mssd"].mean(0)) and r3["AR_MSSD"] == float(g["bits_mssd"].mean(0).mean())
    assert rp["AR_MSPD"] == float(g["bits_mspd"].mean(0).mean()) and r3["count"] == len(g["mssd"])
    for m, blk in r3["per_mesh"].items():
        sel = g["mesh"] == m
        assert blk["count"] == sel.sum() and np.array_equal(blk["recall"], g["bits_mssd"][sel].mean(0))
    per_pose = metric.bop_recall(g["mssd"], "mssd", diameters=diam[g["mesh"]])                       # one diameter per pose
    assert np.array_equal(per_pose["correct"], g["bits_mssd"])
    s = metric.summarize_bop({"mssd": g["mssd"], "mspd": g["mspd"], "proj": g["proj"], "add": g["proj"]}, diameters=diam, im_width=640,
                             mesh_ids=g["mesh"])
    assert sorted(s) == ["AR_MSPD", "AR_MSSD", "mspd", "mssd"] and s["AR_MSSD"] == r3["AR_MSSD"] and s["AR_MSPD"] == rp["AR_MSPD"]
    s = metric.summarize_bop({"proj": g["proj"]}, thresholds={"proj": [5.0]})
    assert s["AR_PROJ"] == float((g["proj"] < 5.0).mean())


def test_threshold_expressions():
    assert np.array_equal(metric.bop_thresholds("mssd"), np.arange(0.05, 0.51, 0.05)) and len(metric.bop_thresholds("mssd")) == 10
    assert np.array_equal(metric.bop_thresholds("mspd"), np.arange(5, 51, 5)) and len(metric.bop_thresholds("mspd")) == 10
    src = inspect.getsource(metric.bop_thresholds)
    assert "np.arange(0.05, 0.51, 0.05)" in src and "np.arange(5, 51, 5)" in src
    with pytest.raises(ValueError):
        metric.bop_thresholds("proj")
    with pytest.raises(ValueError):
        metric.bop_recall([1.0], "proj")


def test_strict_comparison_nan_and_the_width_factor():
    th = np.arange(0.05, 0.51, 0.05)
    r = metric.bop_recall(np.array([th[3], np.nan, 0.0]), "mssd", diameters=1.0)                    # an error exactly ON a threshold
    assert r["correct"][0].tolist() == [False] * 4 + [True] * 6
    assert not r["correct"][1].any() and r["correct"][2].all()                                        # NaN is a miss
    assert np.allclose(r["recall"], (r["correct"].sum(0)) / 3.0) and r["count"] == 3
    r = metric.bop_recall([10.0, 19.999], "mspd", im_width=640)
    assert r["correct"][0].tolist() == [False, False] + [True] * 8 and r["correct"][1].tolist() == [False] * 3 + [True] * 7
    r = metric.bop_recall([12.0, 20.0], "mspd", im_width=1280)                                        # 640 / 1280: scored as 6 and 10 pixels
    assert r["correct"][0].tolist() == [False] + [True] * 9 and r["correct"][1].tolist() == [False, False] + [True] * 8
    r = metric.bop_recall([12.0], "mssd", diameters=[100.0, 24.0], mesh_ids=[1])                      # 12 / 24 = 0.5: the last threshold, strict
    assert not r["correct"][0].any()
    with pytest.raises(ValueError):
        metric.bop_recall([1.0], "mssd")
    with pytest.raises(ValueError):
        metric.bop_recall([1.0], "mspd")


def test_no_cpu_fallback():
    R, t = torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3, 1, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.bop_errors(R, t, R, t, np.eye(3), np.zeros((4, 3), np.float32))
    ident = [{"R": np.eye(3), "t": np.zeros((3, 1))}]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.mssd(np.eye(3), np.zeros(3), np.eye(3), np.zeros(3), np.ones((4, 3)), ident, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.mspd(np.eye(3), np.zeros(3), np.eye(3), np.zeros(3), np.eye(3), np.ones((4, 3)), ident, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.proj(np.eye(3), np.zeros(3), np.eye(3), np.zeros(3), np.eye(3), np.ones((4, 3)), device="cpu")
    sig = inspect.signature(metric.bop_errors)
    assert list(sig.parameters)[:9] == ["R_est", "t_est", "R_gt", "t_gt", "cam_K", "vertices", "symmetries", "mesh_ids", "kinds"]
    assert sig.parameters["kinds"].default == ("mssd", "mspd", "proj")
    from checkerpose_amd import postprocess, targets
    assert inspect.signature(postprocess.evaluate_poses).parameters["symmetries"].default is None
    assert inspect.signature(targets.evaluate_batch).parameters["symmetries"].default is None
    assert inspect.signature(postprocess.evaluate_poses).parameters["kinds"].default == ("add", "adi")


def test_cp_bop_errors_rejects_bad_arguments_before_any_launch(lib):
    p = C.c_void_p(4096)                                    # fake, aligned; never dereferenced: every call returns before a launch
    all3 = _abi.BOP_ERR_MSSD | _abi.BOP_ERR_MSPD | _abi.BOP_ERR_PROJ

    def call(est=p, gt=p, K=p, ks=9, verts=p, voff=p, syms=p, soff=p, M=2, ids=p, B=2, Vmax=8, Smax=4, kinds=all3, o1=p, o2=p, o3=p, scr=p):
        return lib.cp_bop_errors(None, est, gt, K, ks, verts, voff, syms, soff, M, ids, B, Vmax, Smax, kinds, o1, o2, o3, scr)

    for name in ("est", "gt", "K", "verts", "syms", "soff", "scr"):
        assert call(**{name: None}) == -1, name                                # null inputs
    assert call(kinds=0) == -1 and call(kinds=8) == -1 and call(kinds=_abi.BOP_MAP_SMALL) == -1      # no kind / unknown bit / a mapping bit alone
    assert call(kinds=all3 | _abi.BOP_MAP_SMALL | _abi.BOP_MAP_LARGE) == -1
    assert call(o1=None) == -1 and call(o2=None) == -1 and call(o3=None) == -1                      # an output that was asked for is missing
    assert call(B=0) == -1 and call(M=0) == -1 and call(Vmax=0) == -1 and call(Smax=0) == -1 and call(B=-3) == -1
    assert call(ks=3) == -1 and call(ks=12) == -1                                                     # k_stride is 0 or 9
    assert call(ids=None) == -1 and call(voff=None) == -1                                             # several meshes need ids and offsets
    assert call(est=C.c_void_p(4100)) == -3 and call(scr=C.c_void_p(4104)) == -3 and call(soff=C.c_void_p(4098)) == -3
    assert call(B=1 << 22, Smax=1256) == -4                                                           # 2^22 x 1256 / 256 compose workgroups
    assert call(B=1 << 20, Smax=1, Vmax=1 << 20, kinds=all3 | _abi.BOP_MAP_SMALL) == -4
    assert lib.cp_bop_errors_scratch_bytes(0, 1, 8) == 0 and lib.cp_bop_errors_scratch_bytes(1, 0, 8) == 0
    assert lib.cp_bop_errors_map_scratch_bytes(1, 1, 8, 7) == 0
    for B, S, V in ((1, 1, 1), (1, 8, 4096), (256, 628, 20480), (13, 65, 4096), (256, 1256, 20480)):
        n = lib.cp_bop_errors_scratch_bytes(B, S, V)
        assert n >= 4 * (24 * B * S + 32 * B) + 8 * B * S and n % 16 == 0
        assert n == lib.cp_bop_errors_map_scratch_bytes(B, S, V, 0)
        assert n in (lib.cp_bop_errors_map_scratch_bytes(B, S, V, _abi.BOP_MAP_SMALL), lib.cp_bop_errors_map_scratch_bytes(B, S, V, _abi.BOP_MAP_LARGE))
    assert lib.cp_version() >= 208
