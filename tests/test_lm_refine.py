"""CPU: row N22 (Levenberg-Marquardt polish of solved poses).  The numpy restatement of tests/lm_stages.py against its own checker, its
own properties (decreasing cost, a stationary end point) and scipy.optimize.least_squares; the checker against tampering, one named
mutation per stage; the measured constants re-derived; the wrapper's and the ABI's refusals (they return before any launch: no
device is needed to reach them)."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.optimize import least_squares

from tests import lm_stages as L
from tests.pnp_stages import StageError

REFINED = [k for k in L.CASES if k not in ("behind_camera",)]


@pytest.fixture(scope="module")
def runs():
    """every committed case with the restatement's own outputs, computed once and left unchanged"""
    out = {}
    for name in L.CASES:
        case = L.make(name)
        out[name] = (case,) + L.restatement_outputs(case)
    return out


@pytest.mark.parametrize("name", list(L.CASES))
def test_checker_passes_on_the_restatement(runs, name):
    case, rec, R, t, status, info = runs[name]
    total = L.check_case(case, rec, R, t, status, info, log=print)
    if name.startswith("exact") and case.max_iters == 20:
        assert (status == 1).all() and total["accepted"] >= 3 * case.B          # 5 degrees off: several accepted steps, then the step rule
    if name in ("exact_it1", "exact_it2", "noisy_it1", "noisy_it2", "origin_it5"):
        assert (status == 2).all() and (info[:, 3] == case.max_iters).all()
    if name == "origin":
        assert (status == 3).all() and (info[:, 3] == 12).all() and total["accepted"] == 0
    if name == "exact_it64":
        assert (status == 3).all()                                               # step_tol 1e-300: it ends by lambda, not by the step rule


def test_measured_constants(runs):
    tau, e = [0.0, 0.0], [0.0, 0.0]
    for name, (case, rec, R, t, status, info) in runs.items():
        a, b = L.measure_tau(case, rec), L.measure_e(case, R, t, status)
        tau, e = [max(x, y) for x, y in zip(tau, a)], [max(x, y) for x, y in zip(e, b)]
    print("MEASURED_TAU = (%.3e, %.3e)  MEASURED_E = (%.3e, %.3e)" % (tau[0], tau[1], e[0], e[1]))
    for got, kept in zip(tau + e, L.MEASURED_TAU + L.MEASURED_E):
        assert kept / 4 < got <= kept, (got, kept)
    assert L.taus()[0] < 1e-6 and L.taus()[1] < 1e-5                             # the caps of pnp_stages are not what binds


def _tamper_flag(rec, R, t, info):
    it = int(np.nonzero(rec[0, :, 3] == 1.0)[0][0])
    rec[0, it, 3] = 0.0


def _tamper_trial(rec, R, t, info):
    rec[0, 0, 5] += 1e-6


def _tamper_cost(rec, R, t, info):
    rec[0, 1, 1] *= 1.0 + 1e-6


def _tamper_trial_cost(rec, R, t, info):
    rec[0, 0, 2] *= 1.0 - 1e-6


def _tamper_lambda(rec, R, t, info):
    rec[0, 1, 0] *= 10.0


def _tamper_pose(rec, R, t, info):
    acc = np.nonzero(rec[0, :, 3] == 1.0)[0]
    R[0] = rec[0, acc[-2], 5:14].reshape(3, 3)                                   # an accepted trial, but not the last


def _tamper_status(rec, R, t, info, status=None):
    rec[0, int(info[0, 3])] = rec[0, int(info[0, 3]) - 1]                        # a record behind the stop


def _tamper_info(rec, R, t, info):
    info[0, 4 + 7] *= 1.0 + 1e-6


@pytest.mark.parametrize("stage,tamper", [("A", _tamper_flag), ("T", _tamper_trial), ("S", _tamper_cost), ("C", _tamper_trial_cost),
                                          ("L", _tamper_lambda), ("R", _tamper_pose), ("E", _tamper_status), ("I", _tamper_info)],
                         ids=["flag", "trial_pose", "cost", "trial_cost", "lambda", "returned_pose", "stop", "info_H"])
def test_checker_catches(runs, stage, tamper):
    case, rec, R, t, status, info = runs["exact_3x256"]
    rec, R, t, info = rec.copy(), R.copy(), t.copy(), info.copy()
    tamper(rec, R, t, info)
    with pytest.raises(StageError) as e:
        L.check_case(case, rec, R, t, status, info)
    assert e.value.stage == stage and e.value.crop == 0


def test_checker_catches_a_cost_that_only_the_restatement_contradicts(runs):
    """c off by 1e-6 relative in the FIRST record (no earlier c' to compare with): stage C, against numpy's cost"""
    case, rec, R, t, status, info = runs["exact_3x256"]
    rec, info = rec.copy(), info.copy()
    rec[0, 0, 1] *= 1.0 + 1e-6
    info[0, 0] = rec[0, 0, 1]
    with pytest.raises(StageError) as e:
        L.check_case(case, rec, R, t, status, info)
    assert e.value.stage == "C"


@pytest.mark.parametrize("name", REFINED)
def test_accepted_costs_strictly_decrease(runs, name):
    case, rec, R, t, status, info = runs[name]
    for b in range(case.B):
        if status[b] == 0:
            continue
        costs = [rec[b, 0, 1]] + [r[2] for r in rec[b] if r[3] == 1.0]
        assert all(y < x for x, y in zip(costs, costs[1:])), (name, b, costs)
        assert info[b, 1] == costs[-1] and info[b, 0] == costs[0] and info[b, 1] <= info[b, 0]


@pytest.mark.parametrize("name", [k for k in REFINED if k.startswith(("exact", "noisy", "passthrough"))])
def test_final_pose_is_stationary(runs, name):
    """what the stop rule implies: the last step solves (H + lambda D) d = -g with |d| <= b = (step_tol x 3, step_tol |t| x 3), so
    |g_i| <= ((|H| + lambda diag H) b)_i at the state before it, and at the state after it up to the step's own second-order change:
    a factor 2, plus the rounding of g's sum, 1e-12 sum_k |J_ki| |r_k|"""
    case, rec, R, t, status, info = runs[name]
    seen = 0
    for b in range(case.B):
        if status[b] != 1:
            continue
        p3, p2, mk, K = case.crop(b)
        sel = np.nonzero(mk)[0]
        X, p = p3[sel], p2[sel]
        J0, J1, r0, r1, _ = L.jacobian(X, p, K, R[b], t[b])
        sums, _ = L.evaluate(X, p, K, R[b], t[b])
        H, g = L.unpack_H(sums), sums[21:27]
        lam = rec[b, int(info[b, 3]) - 1, 0]
        bound = np.concatenate([np.full(3, case.step_tol), np.full(3, case.step_tol * np.linalg.norm(t[b]))])
        noise = np.array([(np.abs(J0[i]) * np.abs(r0) + np.abs(J1[i]) * np.abs(r1)).sum() for i in range(6)])
        lim = 2.0 * (np.abs(H) + lam * np.diag(np.diag(H))) @ bound + 1e-12 * noise
        assert (np.abs(g) <= lim).all(), (name, b, np.abs(g) / lim)
        seen += 1
    assert seen or case.max_iters != 20


def _scipy_pose(case, b):
    p3, p2, mk, K = case.crop(b)
    sel = np.nonzero(mk)[0]
    X, p = p3[sel], p2[sel]
    R0, t0 = case.R0[b], case.t0[b]

    def pose(x):
        return L._rodrigues(x[:3], np.linalg.norm(x[:3])) @ R0 if np.linalg.norm(x[:3]) > 0 else R0, t0 + x[3:]

    def res(x):
        Rx, tx = pose(x)
        _, _, r0, r1, _ = L.jacobian(X, p, K, Rx, tx)
        return np.concatenate([r0, r1])
    sol = least_squares(res, np.zeros(6), method="trf", jac="3-point", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=np.array([1, 1, 1, 1e3, 1e3, 1e3]))
    return pose(sol.x)


def test_scipy_least_squares_ends_at_the_same_pose(runs):
    worst = [0.0, 0.0]
    for name in ("exact_3x7", "exact_3x256", "exact_per_crop_K", "noisy_3x512", "noisy_1x4096"):
        case, rec, R, t, status, info = runs[name]
        for b in range(case.B):
            assert status[b] == 1
            Rs, ts = _scipy_pose(case, b)
            worst[0] = max(worst[0], float(np.abs(Rs - R[b]).max()))
            worst[1] = max(worst[1], float(np.linalg.norm(ts - t[b]) / np.linalg.norm(t[b])))
    print("MEASURED_SCIPY = (%.3e, %.3e)" % tuple(worst))
    assert worst[0] <= L.scipy_margins()[0] and worst[1] <= L.scipy_margins()[1], worst


def test_pass_through_cases_pass_through(runs):
    case, rec, R, t, status, info = runs["passthrough"]
    assert status.tolist() == [1, 0, 0, 0, 0, 0, 1]
    for b in range(1, 6):
        assert np.array_equal(R[b].view(np.uint64), case.R0[b].view(np.uint64)) and np.array_equal(t[b].view(np.uint64), case.t0[b].view(np.uint64))
        assert np.isnan(rec[b]).all() and info[b, 3] == 0 and info[b, 2] == case.mask[b].sum()
    assert info[2, 2] == 5
    case, rec, R, t, status, info = runs["behind_camera"]
    assert status.tolist() == [0, 0] and np.array_equal(R, case.R0) and np.array_equal(t, case.t0) and np.isnan(rec).all()
    for b in range(2):                                                           # it IS the edge it is named after
        assert not L.point_terms(case.p3d, case.p2d[b], case.K, case.R0[b], case.t0[b])[1].all()


def test_kernel_order_sum_is_a_sum():
    rng = np.random.default_rng(0)
    for n in (1, 6, 63, 64, 65, 255, 256, 257, 700, 4096):
        T = rng.normal(size=(n, 28)) * 10.0 ** rng.integers(-3, 4, size=(n, 1))
        assert np.allclose(L.kernel_sum(T), T.sum(0), rtol=0, atol=1e-12 * np.abs(T).sum(0))
    ints = rng.integers(-1000, 1000, size=(777, 28)).astype(np.float64)          # exact in any order
    assert np.array_equal(L.kernel_sum(ints), ints.sum(0))


def test_abi_argument_checks_return_before_any_launch(lib):
    assert lib.cp_version() >= 232
    assert lib.cp_pnp_refine_lm_record_doubles() == L.REC == 17 and lib.cp_pnp_refine_lm_info_doubles() == L.INFO == 40
    one, two, N = C.c_void_p(4096), C.c_void_p(8192), 512

    def call(**kw):
        a = dict(p3d=one, p3d_bs=0, p2d=one, mask=one, ms=1, K=one, K_bs=0, B=2, N=N, pin=one, sin=None, it=20, tol=1e-10, pout=two, sout=one,
                 info=one, rec=None)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = lib.cp_pnp_refine_lm(None, a["p3d"], a["p3d_bs"], a["p2d"], a["mask"], a["ms"], a["K"], a["K_bs"], a["B"], a["N"], a["pin"], a["sin"],
                                  a["it"], a["tol"], a["pout"], a["sout"], a["info"], a["rec"])
        assert lib.cp_kernel_log() == b"", kw
        return rc
    for name in ("p3d", "p2d", "mask", "K", "pin", "pout", "sout", "info"):
        assert call(**{name: None}) == -1, name
        assert call(B=0, **{name: None}) == -1, name
    assert call(B=-1) == -1 and call(N=0) == -1 and call(N=4097) == -1 and call(N=-1) == -1 and call(ms=0) == -1
    assert call(it=0) == -1 and call(it=65) == -1 and call(it=-3) == -1
    for tol in (0.0, -1e-10, float("nan"), float("inf")):
        assert call(tol=tol) == -1, tol
    for bs in (1, 3 * N - 1, -3 * N):
        assert call(p3d_bs=bs) == -1, bs
    assert call(K_bs=8) == -1 and call(K_bs=-9) == -1
    for name in ("pin", "pout", "info", "rec"):
        assert call(**{name: C.c_void_p(4100)}) == -3, name
    assert call(sout=C.c_void_p(4098)) == -3 and call(sin=C.c_void_p(4098)) == -3
    assert call(pout=C.c_void_p(4096 + 96)) == -1 and call(pout=C.c_void_p(4096 + 8)) == -1 and call(pout=C.c_void_p(4096 - 184)) == -1   # partial overlap
    assert call(B=0) == 0 and call(B=0, pout=one) == 0                           # nothing to do: no launch (the log stayed empty)


def test_wrapper_refusals():
    from checkerpose_amd import postprocess as PP
    B, N = 2, 8
    a = dict(p3d_xyz=torch.zeros(N, 3), p2d=torch.zeros(B, N, 2), mask=torch.ones(B, N, dtype=torch.bool), cam_K=torch.eye(3),
             R=torch.eye(3, dtype=torch.float64).expand(B, 3, 3).contiguous(), t=torch.ones(B, 3, 1, dtype=torch.float64))
    for name, bad in (("max_iters", 0), ("max_iters", 65), ("max_iters", -1), ("step_tol", 0.0), ("step_tol", -1.0), ("step_tol", float("nan")),
                      ("step_tol", float("inf"))):
        with pytest.raises(ValueError, match=name):
            PP.refine_poses_lm(**dict(a, **{name: bad}))
    for name, bad in (("mask", a["mask"][:, :7]), ("mask", a["mask"].float()), ("mask", a["mask"][:1]), ("R", a["R"][:1]), ("t", torch.ones(B, 4)),
                      ("p2d", torch.zeros(B, N, 3)), ("status", torch.ones(3, dtype=torch.int32))):
        with pytest.raises(ValueError, match=name):
            PP.refine_poses_lm(**dict(a, **{name: bad}))
    with pytest.raises(ValueError, match="N must be"):
        PP.refine_poses_lm(torch.zeros(4097, 3), torch.zeros(1, 4097, 2), torch.ones(1, 4097, dtype=torch.bool), torch.eye(3), a["R"][:1], a["t"][:1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # well-formed arguments on the host: still no fallback
        PP.refine_poses_lm(**a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.refine_poses_lm(**dict(a, mask=a["mask"].to(torch.uint8), status=torch.ones(B, dtype=torch.int32)))
    with pytest.raises(ValueError, match="refine"):
        PP.estimate_poses(None, torch.zeros(4, 4, 3, dtype=torch.uint8), [], a["p3d_xyz"], a["cam_K"], refine="gn")
    z = np.zeros
    with pytest.raises(ValueError, match="refine"):
        PP.from_id_to_pose(z((N, 3), np.float32), z((1, N, 2), np.float32), np.eye(3, dtype=np.float32), z((N, 1), np.float32), np.arange(N),
                           z(N, np.int64), refine="LM")


def test_pose_covariance_on_the_host():
    """plain torch: runs on CPU tensors too"""
    from checkerpose_amd.postprocess import pose_covariance
    rng = np.random.default_rng(3)
    A = rng.normal(size=(4, 9, 6))
    H = torch.from_numpy(np.einsum("bki,bkj->bij", A, A))
    info = dict(H=H.clone(), n=torch.tensor([10, 3, 8, 8]), cost=torch.tensor([28.0, 1.0, 5.0, 5.0], dtype=torch.float64),
                status=torch.tensor([1, 1, 0, 2], dtype=torch.int32))
    info["H"][2] = float("nan")
    cov = pose_covariance(info)
    assert tuple(cov.shape) == (4, 6, 6) and cov.dtype == torch.float64
    assert torch.isnan(cov[1]).all() and torch.isnan(cov[2]).all()             # 2 n <= 6; status 0
    assert torch.allclose(cov[0], 2.0 * torch.linalg.inv(H[0]), rtol=1e-12, atol=0) and torch.allclose(cov[3], 0.5 * torch.linalg.inv(H[3]), rtol=1e-12, atol=0)
    cov = pose_covariance(info, sigma=0.5)
    assert torch.allclose(cov[0], 0.25 * torch.linalg.inv(H[0]), rtol=1e-12, atol=0) and torch.isnan(cov[2]).all()


def test_package_exports_the_new_names():
    import checkerpose_amd
    from checkerpose_amd import postprocess as PP
    assert checkerpose_amd.refine_poses_lm is PP.refine_poses_lm and checkerpose_amd.pose_covariance is PP.pose_covariance
    import inspect
    assert inspect.signature(PP.estimate_poses).parameters["refine"].default is None
    assert inspect.signature(PP.from_id_to_pose).parameters["refine"].default is None
    assert list(inspect.signature(PP.refine_poses_lm).parameters) == ["p3d_xyz", "p2d", "mask", "cam_K", "R", "t", "status", "max_iters", "step_tol",
                                                                      "return_records"]
