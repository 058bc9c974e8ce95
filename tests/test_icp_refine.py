"""CPU: row N24's restatement and checker (tests/icp_stages.py) against independent statements -- numpy.linalg.lstsq and
scipy.optimize.least_squares for the step, the lattice rule by enumeration --, the checker's own tamperings, the selection of the
converging cases, the measured constants, and the Python layer's refusals, defaults and `refine` values (no device)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import icp_stages as I
from tests.pnp_stages import StageError

_RUNS = {}


def _run(name):
    """a committed case free-running on the CPU: (case, samples, (records, R, t, status, info)); computed once, left unchanged"""
    if name not in _RUNS:
        case = I.make(name)
        smp = I.case_samples(case)
        _RUNS[name] = (case, smp, I.restatement_outputs(case, smp))
    return _RUNS[name]


def _inner_problem(name="torus_3_g17", b=0):
    case, smp, _ = _run(name)
    s = smp[b]
    a = I.associate(s["X"], s["N"], s["face"], case.K_of(b), case.R0[b], case.t0[b], case.depth[case.image_of(b)], case.max_dist_of(b))
    k = a["pair"]
    return case, s, a, k


def test_gauss_newton_step_is_lstsq():
    """lambda -> 0, inertia = 0: the restatement's step solves J d = -r in the least-squares sense (J, r written out here again)"""
    for name, b in (("torus_3_g17", 0), ("ico80_3_g32", 1), ("box_3_g17", 2)):
        case, s, a, k = _inner_problem(name, b)
        Y, C, Q, Np = a["Y"][k], a["C"][k], a["Q"][k], a["Np"][k]
        J = np.concatenate([np.cross(Y, Np), Np], 1)
        r = ((C - Q) * Np).sum(1)
        want = np.linalg.lstsq(J, -r, rcond=None)[0]
        state = I.numpy_sum(I.pair_terms(a))
        kind, d, Rn, tn, sstep = I.trial(state, case.R0[b], case.t0[b], 0.0, 0.0, case.rho_of(b), np.inf)
        assert kind == 1
        # normal equations square the condition number: cond(H) eps bounds the relative difference
        cond = np.linalg.cond(J) ** 2
        assert np.abs(d - want).max() <= 64 * cond * np.finfo(float).eps * np.abs(want).max(), (name, np.abs(d - want).max(), cond)
        assert sstep == max(np.abs(d[:3]).max(), np.abs(d[3:]).max() / np.linalg.norm(case.t0[b]))


def test_inner_problem_against_scipy():
    """ONE association's inner problem (Q, Np frozen): the rule's undamped steps reach scipy.optimize.least_squares' minimiser"""
    so = pytest.importorskip("scipy.optimize")
    case, s, a, k = _inner_problem("ico80_3_g32", 0)
    X, Q, Np = s["X"][k], a["Q"][k], a["Np"][k]
    R0, t0 = case.R0[0], case.t0[0]

    def pose(x):
        return I._rodrigues(x[:3], np.linalg.norm(x[:3])) @ R0 if np.linalg.norm(x[:3]) > 0 else R0, t0 + x[3:]

    def resid(x):
        R, t = pose(x)
        return (((X @ R.T + t) - Q) * Np).sum(1)

    ref = so.least_squares(resid, np.zeros(6), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    R, t = R0, t0
    for _ in range(12):                                      # the rule's own step with lambda = 0, inertia = 0 and no bound, always taken
        frozen = dict(a, Y=np.where(k[:, None], np.where(k[:, None], s["X"], 0.0) @ R.T, 0.0))
        frozen["C"] = frozen["Y"] + t
        kind, d, R, t, _ = I.trial(I.numpy_sum(I.pair_terms(frozen)), R, t, 0.0, 0.0, case.rho_of(0), np.inf)
        assert kind == 1
    Rs, ts = pose(ref.x)
    # both minimise the same smooth cost.  MINPACK differentiates forward: its Jacobian, hence the gradient whose zero it finds, is off by
    # about sqrt(eps) = 1.5e-8 relative, which the conditioning of H (the sphere-like ico80 constrains its rotation only through its
    # facets: up to 1e2) amplifies in the pose: 1e-6.  The cost itself is flat there: the rule's point must not be the worse one.
    assert np.abs(R - Rs).max() <= 1e-6 and np.linalg.norm(t - ts) / np.linalg.norm(ts) <= 1e-6, (np.abs(R - Rs).max(), np.linalg.norm(t - ts))
    cost = lambda R_, t_: float(((((X @ R_.T + t_) - Q) * Np).sum(1) ** 2).sum())      # noqa: E731
    assert cost(R, t) <= cost(Rs, ts) * (1.0 + 1e-9)


def test_lattice_rule():
    for x0, w, grid in ((0, 1, 8), (3, 7, 8), (3, 8, 8), (3, 9, 8), (10, 31, 17), (0, 96, 64), (5, 64, 64), (2, 65, 64), (7, 1000, 33), (0, 4096, 64)):
        n = min(grid, w)
        cols = I.lattice_axis(x0, w, n)
        assert len(cols) == n and cols[0] >= x0 and cols[-1] <= x0 + w - 1
        assert all(b > a for a, b in zip(cols, cols[1:]))
        if n == w:
            assert cols == list(range(x0, x0 + w))
        assert all(x0 + (i * w) // n <= c < x0 + -((-(i + 1) * w) // n) for i, c in enumerate(cols))      # column i inside its own cell
    lat = I.lattice((-2, 5, 30, 97), I.SIZE, 17)
    assert lat == (0, 5, 31, 75, 17, 17)
    assert I.lattice((96, 0, 99, 5), I.SIZE, 8) is None and I.lattice((-5, -9, -1, -1), I.SIZE, 8) is None
    pix = I.lattice_pixels(I.lattice((10, 20, 14, 60), I.SIZE, 8), 8)          # narrower than the grid: nx = w = 5
    assert (pix[:40, 0].reshape(8, 5) == np.arange(10, 15)).all() and (pix[40:] == -1).all() and len(set(pix[:40:5, 1])) == 8


@pytest.mark.parametrize("name", list(I.CASES))
def test_restatement_replays_and_converges(name):
    """every committed case: the checker accepts the restatement's own free-running outputs; a case committed as converging ends, on
    the CPU alone, below a quarter of its starting ADD with status 1 or 2 on every refined pose; the others assert only the replay"""
    case, smp, out = _run(name)
    I.check_case(case, smp, *out)
    rec, R, t, status, info = out
    if name in I.CONVERGING:
        assert I.converges(case, R, t, status), (I.add_ratios(case, R, t), status)
    refined = status != 0
    assert (info[refined, 1] <= info[refined, 0]).all()


def test_converging_selection():
    assert set(I.CONVERGING) <= set(I.CASES) and len(I.CONVERGING) >= 8
    meshes = set()
    for name in I.CONVERGING:
        case, _, (_, _, _, status, _) = _run(name)
        meshes |= {case.meshes[case.mesh_of(b)] for b in range(case.P) if status[b]}
    assert len(meshes) >= 3, meshes
    # what the committed cases cover
    grids = {I.make(n).grid for n in I.CASES}
    assert {8, 17, 32, 64} <= grids
    assert {I.make(n).P for n in I.CASES} >= {1, 3, 5} and {I.make(n).max_iters for n in I.CASES} >= {1, 2, 20}
    assert any(I.make(n).K.ndim == 3 for n in I.CASES) and any(np.ndim(I.make(n).max_dist) for n in I.CASES)
    assert any(I.make(n).mesh_ids is not None and I.make(n).image_ids is not None for n in I.CASES)
    _, smp, _ = _run("narrow_triangle")
    assert smp[0]["shape"][0] < 32                                               # its rectangle is narrower than the grid: nx = w
    _, smp, _ = _run("torus_off_frame")
    assert smp[0]["rect"][2] == I.SIZE[0] - 1                                    # partly outside the frame: clipped at the right edge
    case, smp, _ = _run("ico80_1_g64")
    assert (smp[0]["face"] >= 0).sum() > 256 and case.grid ** 2 == 4096
    d = I.make("torus_3_g17").depth
    assert np.isnan(d).any() and (d == 0).any() and (d == 150).any() and (d == 900).any()


def test_measured_constants():
    tau = [0.0, 0.0]
    for name in I.CASES:
        case, smp, (rec, *_r) = _run(name)
        tau = [max(a, b) for a, b in zip(tau, I.measure_tau(case, smp, rec))]
    for seen, kept in zip(tau, I.MEASURED_TAU):
        assert kept / 4 < seen <= kept, (tau, I.MEASURED_TAU)
    assert I.taus()[0] < 1e-12 and I.taus()[1] < 1e-12


def _tampered(case, smp, tamper):
    if tamper == "no_flip":
        smp = []
        for b, s in enumerate(I.case_samples(case)):
            v, f = case.geometry(b)
            X, N, face = I.samples_from(s["pixel"], s["depth"], s["face"], case.K_of(b), case.R0[b], case.t0[b], v, f, flip=False)
            smp.append(dict(s, X=X, N=N, face=face))
    return smp, I.restatement_outputs(case, smp, tamper=(tamper,))


@pytest.mark.parametrize("tamper", [t for t in I.TAMPERINGS if t != "strict"])
def test_tamperings_are_caught(tamper):
    """a recorded run of the restatement with ONE rule changed is refused by check_case, at the stage the change shows in"""
    stage = dict(rot_sign="T", pixel_centre="C", round="n", no_inertia="T", no_flip="N", rerotate="C")[tamper]
    caught = 0
    # (a closed mesh wound outwards shows only faces whose normal already points at the camera: the flip shows on the open ones)
    for name in ("halfbox_3_g32", "triangle_3_g17") if tamper == "no_flip" else ("torus_3_g17", "box_3_g17"):
        case, smp, _ = _run(name)
        smp_t, out = _tampered(case, smp, tamper)
        try:
            I.check_case(case, smp_t, *out)
        except StageError as e:
            caught += 1
            assert e.stage in (stage, "n", "C"), (tamper, e)
    assert caught == 2, tamper


def _tie_case():
    """a fronto-parallel 7 x 7 patch at Z = 512 in front of a sensor plane at 516 -- 520 at the centre pixel, whose sample lies ON the
    optical axis: |C - Q| = 8 = max_dist EXACTLY there (512 * (520 / 512) is exact), about 4.03 elsewhere"""
    K = np.array([[120.0, 0.0, 47.5], [0.0, 118.0, 40.5], [0.0, 0.0, 1.0]])
    pix = np.array([(x, y) for y in range(37, 44) for x in range(44, 51)])
    X = np.stack([(pix[:, 0] + 0.5 - 47.5) * 512.0 / 120.0, (pix[:, 1] + 0.5 - 40.5) * 512.0 / 118.0, np.zeros(49)], 1)
    N = np.tile([0.0, 0.0, -1.0], (49, 1))
    depth = np.full((80, 96), 516.0, np.float32)
    depth[40, 47] = 520.0
    case = I.IcpCase("tie", ("box",), None, K, None, [(0, np.eye(3), np.array([0.0, 0.0, 516.0]), K)], np.eye(3)[None], np.array([[0.0, 0.0, 512.0]]),
                     depth[None], 8.0, grid=7, max_iters=3)
    return case, [dict(pixel=pix, depth=np.full(49, 512.0, np.float32), face=np.zeros(49, np.int64), X=X, N=N)]


def test_strict_comparison_is_caught():
    """`<` instead of `<=` at max_dist shows only where |C - Q| == max_dist exactly: the rule's own comparison decides that pair"""
    case, smp = _tie_case()
    a = I.associate(smp[0]["X"], smp[0]["N"], smp[0]["face"], case.K, case.R0[0], case.t0[0], case.depth[0], 8.0)
    assert a["n"] == 49 and a["margin"] == 0.0
    good = I.restatement_outputs(case, smp)
    assert good[3][0] != 0 and good[0][0, 0, 1] == 49
    I.check_case(case, smp, *good, stage_a=False, allow_exact=True)
    with pytest.raises(StageError) as e:                     # without the allowance the tie is reported AS a tie, first
        I.check_case(case, smp, *good, stage_a=False)
    assert e.value.stage == "B"
    bad = I.restatement_outputs(case, smp, tamper=("strict",))
    assert bad[0][0, 0, 1] == 48
    with pytest.raises(StageError) as e:
        I.check_case(case, smp, *bad, stage_a=False, allow_exact=True)
    assert e.value.stage == "n"


def test_checker_catches_edits_of_the_outputs():
    case, smp, out = _run("torus_3_g17")
    rec, R, t, status, info = [x.copy() for x in out]
    for stage, edit in (("L", lambda: rec.__setitem__((0, 1, 0), rec[0, 1, 0] * 10)), ("R", lambda: t.__setitem__((1, 2), np.nextafter(t[1, 2], 0))),
                        ("E", lambda: status.__setitem__(2, 1)), ("I", lambda: info.__setitem__((0, 4), info[0, 4] + 1)),
                        ("A", lambda: rec.__setitem__((2, 0, 4), 1.0 - rec[2, 0, 4]))):
        rec, R, t, status, info = [x.copy() for x in out]
        edit()
        with pytest.raises(StageError) as e:
            I.check_case(case, smp, rec, R, t, status, info)
        assert e.value.stage == stage, (stage, e.value)


# ------------------------------------------------------------------------------------------------------------- the Python layer
def _host_args():
    from checkerpose_amd.metric import MeshSet
    v, f = I.mesh_arrays(("box",))
    ms = MeshSet.from_arrays(v, faces=f)
    return dict(R=torch.eye(3, dtype=torch.float64)[None], t=torch.tensor([[0.0, 0.0, 300.0]], dtype=torch.float64), cam_K=torch.from_numpy(I.K_A),
                meshes=ms, depth=torch.full((80, 96), 300.0), max_dist=10.0)


def test_defaults_and_refusals():
    from checkerpose_amd import postprocess as PP
    sig = inspect.signature(PP.refine_poses_icp).parameters
    assert sig["max_dist"].default is inspect.Parameter.empty                   # NO default
    assert [sig[k].default for k in ("grid", "max_iters", "step_tol", "min_pairs", "inertia", "samples", "return_records")] == [32, 20, 1e-6, 6, 1e-2, None, False]
    assert inspect.signature(PP.surface_samples).parameters["grid"].default == 32
    assert inspect.signature(PP.estimate_poses).parameters["refine"].default is None and inspect.signature(PP.estimate_poses).parameters["icp"].default is None
    a = _host_args()
    for name, bad in (("min_pairs", 5), ("inertia", -1e-3), ("inertia", float("nan")), ("grid", 0), ("grid", 65), ("max_iters", 0), ("max_iters", 65),
                      ("step_tol", 0.0), ("step_tol", float("inf"))):
        with pytest.raises(ValueError, match=name):
            PP.refine_poses_icp(**dict(a, **{name: bad}))
    for bad in (0, 65):
        with pytest.raises(ValueError, match="grid"):
            PP.surface_samples(a["R"], a["t"], a["cam_K"], a["meshes"], (96, 80), grid=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # well-formed arguments on the host: still no fallback
        PP.refine_poses_icp(**a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.surface_samples(a["R"], a["t"], a["cam_K"], a["meshes"], (96, 80))
    with pytest.raises(TypeError):
        PP.refine_poses_icp(a["R"], a["t"], a["cam_K"], a["meshes"], a["depth"])                 # max_dist is required


def test_refine_values():
    from checkerpose_amd import postprocess as PP
    frames, p3d, K = torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(8, 3), torch.eye(3)
    for bad in ("gn", "icp+lm", "ICP", ""):
        with pytest.raises(ValueError, match="refine"):
            PP.estimate_poses(None, frames, [], p3d, K, refine=bad)
    for refine in ("icp", "lm+icp"):
        with pytest.raises(ValueError, match="icp"):
            PP.estimate_poses(None, frames, [], p3d, K, refine=refine)
        with pytest.raises(ValueError, match="icp"):
            PP.estimate_poses(None, frames, [], p3d, K, refine=refine, icp=dict(meshes=None, depth=None))             # no max_dist
        with pytest.raises(ValueError, match="img_index"):
            PP.estimate_poses(None, frames, [], p3d, K, refine=refine, icp=dict(meshes=None, depth=None, max_dist=1.0, image_ids=[0]))
    z = np.zeros
    for bad in ("icp", "lm+icp"):                            # from_id_to_pose has no depth: it keeps refusing anything but None / "lm"
        with pytest.raises(ValueError, match="refine"):
            PP.from_id_to_pose(z((8, 3), np.float32), z((1, 8, 2), np.float32), np.eye(3, dtype=np.float32), z((8, 1), np.float32), np.arange(8),
                               z(8, np.int64), refine=bad)


def test_estimate_poses_routes_refine(monkeypatch):
    """the order and the arguments of the refinement calls, with stubs in place of every device call"""
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import preprocess as PRE
    calls = []
    monkeypatch.setattr(PRE, "get_roi_batch", lambda *a, **k: "crops")
    monkeypatch.setattr(PP, "correspondences", lambda out, **k: ("p2d", "valid", None))
    monkeypatch.setattr(PP, "solve_pnp_ransac", lambda *a, **k: ("R0", "t0", "inl", "status"))

    def lm(p3d, p2d, mask, K, R, t, status=None):
        calls.append(("lm", R, t, mask, status))
        return R + "+lm", t + "+lm", None, None

    def icp(R, t, K, meshes, depth, max_dist, **kw):
        calls.append(("icp", R, t, meshes, depth, max_dist, kw))
        return R + "+icp", t + "+icp", None, None

    monkeypatch.setattr(PP, "refine_poses_lm", lm)
    monkeypatch.setattr(PP, "refine_poses_icp", icp)
    frames = torch.zeros(2, 40, 40, 3, dtype=torch.uint8)
    args = (lambda crops, _: "out", frames, [[5, 5, 10, 10]], "p3d", "K")
    spec = dict(meshes="M", depth="D", max_dist=7.0, mesh_ids=[0], grid=8)
    want_kw = dict(image_ids=[1], status="status", mesh_ids=[0], grid=8)
    assert PP.estimate_poses(*args, img_index=[1])[:4] == ("R0", "t0", "inl", "status") and calls == []
    assert PP.estimate_poses(*args, img_index=[1], refine=None, icp=spec)[:2] == ("R0", "t0") and calls == []
    assert PP.estimate_poses(*args, img_index=[1], refine="lm")[:4] == ("R0+lm", "t0+lm", "inl", "status")
    assert calls == [("lm", "R0", "t0", "inl", "status")]
    del calls[:]
    assert PP.estimate_poses(*args, img_index=[1], refine="icp", icp=spec)[:4] == ("R0+icp", "t0+icp", "inl", "status")
    assert calls == [("icp", "R0", "t0", "M", "D", 7.0, want_kw)]
    del calls[:]
    assert PP.estimate_poses(*args, img_index=[1], refine="lm+icp", icp=spec)[:4] == ("R0+lm+icp", "t0+lm+icp", "inl", "status")
    assert calls == [("lm", "R0", "t0", "inl", "status"), ("icp", "R0+lm", "t0+lm", "M", "D", 7.0, want_kw)]
    assert spec == dict(meshes="M", depth="D", max_dist=7.0, mesh_ids=[0], grid=8)          # the caller's dict is left alone


def test_abi_refusals():
    """the library on a CPU box: the new symbols resolve, the constants, a few refusals with fake pointers (nothing launches)"""
    from checkerpose_amd import _abi
    from checkerpose_amd import postprocess as PP
    lib = _abi.load()
    assert lib.cp_version() >= 234
    assert lib.cp_icp_refine_record_doubles() == I.REC == PP.ICP_RECORD == 18 and lib.cp_icp_refine_info_doubles() == I.INFO == PP.ICP_INFO == 42
    assert lib.cp_surface_samples_scratch_bytes(3, 64) == 288 + 3 * 64 * 16 and lib.cp_surface_samples_scratch_bytes(0, 64) == 0
    buf = C.create_string_buffer(4096 + 16)
    p = (C.addressof(buf) + 15) & ~15
    ok_a = [None, p, p, 0, p, p, p, p, 1, None, 80, 96, 1, 8, 8, p, p, p, p, p, p, p, p, p]
    ok_b = [None, p, p, 0, p, p, p, 64, p, None, 1, 80, 96, p, p, 1, None, None, 20, 1e-6, 6, 1e-2, 1, p, p, p, None]

    def a_with(i, v):
        return lib.cp_surface_samples(*(ok_a[:i] + [v] + ok_a[i + 1:]))

    def b_with(i, v):
        return lib.cp_icp_refine(*(ok_b[:i] + [v] + ok_b[i + 1:]))

    INVALID, ALIGN = a_with(1, None), a_with(1, p + 4)                           # a null pose table; a misaligned one
    assert INVALID != 0 and ALIGN not in (0, INVALID)
    assert [a_with(14, 0), a_with(14, 65), a_with(8, 2), a_with(12, 0), a_with(23, None)] == [INVALID] * 5
    assert [a_with(20, p + 4), a_with(19, p + 2)] == [ALIGN] * 2
    assert [b_with(7, 0), b_with(7, 4097), b_with(18, 65), b_with(19, 0.0), b_with(20, 5), b_with(21, -1.0), b_with(10, 2), b_with(15, 2), b_with(22, 0),
            b_with(13, None)] == [INVALID] * 10
    assert [b_with(4, p + 4), b_with(6, p + 2), b_with(26, p + 4)] == [ALIGN] * 3
