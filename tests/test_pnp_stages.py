"""CPU: the stage checker of tests/pnp_stages.py is shown to catch what it claims to.  It passes on the oracle's own run of every
committed case (records in the device's layout: oracle.hypothesis_records) with zero undecided pairs, it raises under the right
stage on each mutation of such a run, and the constants it carries (TAU, the stage-E margin) are re-measured here."""
import numpy as np
import pytest

from oracle import pnp_oracle as P
from tests import pnp_stages as S

_runs = {}


def _run(name):
    if name not in _runs:
        case = S.CASES[name]()
        _runs[name] = (case, S.oracle_outputs(case))
    return _runs[name]


@pytest.mark.parametrize("name", list(S.CASES))
def test_checker_passes_on_the_oracles_own_records(name):
    case, out = _run(name)
    total = S.check_case(case, *out, log=print)
    assert total["undecided"] == 0
    rec, R, t, inl, status = out
    for b in case.full_oracle:                              # what the GPU test compares with must be a solved crop with a known answer
        assert status[b] == 1 and case.truth[b] is not None, (name, b)
        assert np.abs(R[b] - case.truth[b][0]).max() < 1e-5 and np.array_equal(inl[b], case.crop(b)[2] & ~case.truth[b][2])
    if name.startswith("shape") or name.startswith("column") or name == "per_crop_K":
        assert total["all_inlier"] >= case.B                # stage E has something to check on every such case


def test_measured_constants():
    """TAU and the stage-E margin come from these measurements: the constants in tests/pnp_stages.py bound them, and not loosely
    (a quarter of each would miss), so a change of the cases or of the oracle that moves them is noticed"""
    tau, e = [0.0, 0.0], [0.0, 0.0]
    for name in S.CASES:
        case, (rec, R, t, inl, status) = _run(name)
        tau = [max(a, b) for a, b in zip(tau, S.measure_tau(case, inl, status))]
        e = [max(a, b) for a, b in zip(e, S.measure_e(case, rec))]
    print("measured tau %.3e %.3e, E %.3e %.3e" % (tau[0], tau[1], e[0], e[1]))
    for got, const in zip(tau + e, S.MEASURED_TAU + S.MEASURED_E):
        assert 0.25 * const < got <= const, (tau, e)
    assert S.taus() == (16 * S.MEASURED_TAU[0], 16 * S.MEASURED_TAU[1]) and S.taus()[0] < 1e-6 and S.taus()[1] < 1e-5      # below the caps
    assert S.e_margins() == (8 * S.MEASURED_E[0], 8 * S.MEASURED_E[1])


def test_kernel_jacobi_is_an_eigen_solver():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(40, 12))
    A = A.T @ A
    w, V = S.kernel_jacobi(A)
    assert np.all(np.diff(w) >= 0) and np.allclose(w, np.linalg.eigvalsh(A), rtol=1e-12, atol=1e-12 * w[-1])
    assert np.abs(V.T @ V - np.eye(12)).max() < 1e-13 and np.abs(A @ V - V * w).max() < 1e-11 * w[-1]


def test_oracle_refactoring_left_the_results_alone():
    """hypothesis_records + solve_pnp_ransac: the counts a run visits decide where it stops; a run restricted to 64 iterations
    equals the first round of a longer one; records given from outside are used as they are"""
    case, (rec, R, t, inl, status) = _run("outliers_0.6")
    p3, p2, va, K = case.crop(0)
    r64 = P.hypothesis_records(p3, p2, va, K, case.thr, 64, case.seed, 0)
    assert np.array_equal(r64, rec[0, :64], equal_nan=True)
    assert not np.isnan(rec[0, :, 0]).any()                 # 60 % outliers: the rule never stops a run of 150
    case3, (rec3, *_) = _run("outliers_0.3")
    assert np.isnan(rec3[:, 64:]).all() and not np.isnan(rec3[:, :64, 0]).any()
    again = P.solve_pnp_ransac(p3, p2, va, K, case.thr, case.iterations, case.seed, 0)
    assert np.array_equal(again[0], R[0]) and np.array_equal(again[1], t[0]) and np.array_equal(again[2], inl[0])


# ---------------------------------------------------------------------------------------------------------------- the mutations
def _crop_args(name, b):
    case, (rec, R, t, inl, status) = _run(name)
    p3, p2, va, K = case.crop(b)
    return case, dict(p3d=p3, p2d=p2, valid=va, K=K, thr=case.thr, iterations=case.iterations, seed=case.seed, crop=b,
                      records=rec[b].copy(), R=R[b].copy(), t=t[b].copy(), inliers=inl[b].copy(), status=int(status[b]), truth=case.truth[b])


def _raises(stage, kw):
    with pytest.raises(S.StageError) as e:
        S.check_crop(**kw)
    assert e.value.stage == stage, str(e.value)
    assert "stage %s, crop %d" % (stage, kw["crop"]) in str(e.value)
    return e.value


def test_mutation_count_off_by_one():
    for d in (1, -1):
        case, kw = _crop_args("shape_6x512", 2)
        c = kw["records"][:64, 0]
        h = int(np.nonzero((c >= 1) & (c < c.max() - 1))[0][0])      # not the winner, and no influence on the stopping rule
        kw["records"][h, 0] += d
        assert _raises("B", kw).hyp == h


def test_mutation_record_beyond_the_stopping_rule_and_missing_within():
    case, kw = _crop_args("shape_6x512", 1)
    assert np.isnan(kw["records"][64:]).all()               # 30 % outliers: one round
    kw["records"][64] = kw["records"][0]
    assert _raises("A", kw).hyp == 64
    case, kw = _crop_args("shape_6x512", 1)
    kw["records"][10] = np.nan
    assert _raises("A", kw).hyp == 10
    case, kw = _crop_args("outliers_0.6", 0)                # three rounds demanded: the last one dropped
    kw["records"][128:] = np.nan
    assert _raises("A", kw).hyp == 128
    case, kw = _crop_args("shape_6x512", 1)                 # a stale word in an otherwise unwritten record
    kw["records"][100, 5] = 0.0
    assert _raises("A", kw).hyp == 100


def test_mutation_winner_replaced_by_a_later_tie():
    """needs two hypotheses that tie at the largest count with DIFFERENT inlier sets (with equal sets nothing observable changes):
    noisy 33-point crops are searched in a fixed order for one"""
    xyz = S.lmo_model(33)
    rng = np.random.default_rng(70)
    for crop in range(60):
        p2d, valid, _ = S._crop(rng, xyz, S.K_LMO, 0.2, 0.7, 0.9)
        rec = P.hypothesis_records(xyz, p2d, valid, S.K_LMO, 2.0, 64, 70, crop)
        c = rec[:, 0]
        ties = np.nonzero(c == c.max())[0]
        if c.max() < 5 or len(ties) < 2:
            continue
        vid = np.nonzero(valid)[0]
        sets = [S._sq_errors(xyz[vid], p2d[vid], S.K_LMO, rec[h:h + 1, 2:11].reshape(1, 3, 3), rec[h:h + 1, 11:14])[0] <= 4.0 for h in ties]
        later = [k for k in range(1, len(ties)) if not np.array_equal(sets[k], sets[0])]
        if later:
            break
    else:
        raise AssertionError("no crop with a tie of different inlier sets")
    R, t, inl, status = P.solve_pnp_ransac(xyz, p2d, valid, S.K_LMO, 2.0, 64, 70, crop, records=rec)
    kw = dict(p3d=xyz, p2d=p2d, valid=valid, K=S.K_LMO, thr=2.0, iterations=64, seed=70, crop=crop, records=rec, R=R, t=t, inliers=inl, status=status)
    S.check_crop(**kw)                                      # the first of the ties: passes
    sel = vid[sets[later[0]]]
    kw["inliers"] = np.zeros(33, bool)
    kw["inliers"][sel] = True
    kw["R"], kw["t"], _ = P.epnp(xyz[sel], p2d[sel], S.K_LMO)      # everything else consistent with the later tie
    assert _raises("C", kw).hyp == int(ties[0])


def test_mutation_inlier_bit_flipped():
    case, kw = _crop_args("shape_6x512", 0)
    for k in (np.nonzero(kw["inliers"])[0][3], np.nonzero(kw["valid"] & ~kw["inliers"])[0][0]):
        m = dict(kw, inliers=kw["inliers"].copy())
        m["inliers"][k] ^= True
        assert str(int(k)) in str(_raises("C", m))


def test_mutation_inlier_outside_the_valid_column():
    case, kw = _crop_args("shape_6x512", 0)
    k = int(np.nonzero(~kw["valid"] & ~case.truth[0][2])[0][0])      # a true correspondence, but not in the column
    kw["inliers"][k] = True
    assert "valid column" in str(_raises("C", kw))


def test_mutation_refit_pose_moved_by_ten_tau():
    tau_R, tau_t = S.taus()
    case, kw = _crop_args("shape_6x512", 0)
    a = 10 * tau_R
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    assert "|dR|" in str(_raises("D", dict(kw, R=rot @ kw["R"])))
    _raises("D", dict(kw, t=kw["t"] * (1 + 10 * tau_t)))
    S.check_crop(**dict(kw, t=kw["t"] * (1 + 0.1 * tau_t)))          # ... and a tenth of tau passes
    # a degenerate refit keeps the winner's record bitwise
    case, kw = _crop_args("shape_6x512", 0)
    win = int(np.argmax(kw["records"][:, 0]))
    assert not np.array_equal(kw["R"].reshape(9), kw["records"][win, 2:11])


def test_mutation_reflection():
    case, kw = _crop_args("shape_6x512", 3)
    h = int(np.nonzero(kw["records"][:, 0] >= 0)[0][5])
    kw["records"][h, 8:11] *= -1                            # third row of R negated: orthonormal, det -1
    assert "proper rotation" in str(_raises("B", kw)) and _raises("B", kw).hyp == h
    case, kw = _crop_args("shape_6x512", 3)
    kw["R"][2] *= -1
    _raises("D", kw)


def test_mutation_status_flipped():
    case, kw = _crop_args("shape_6x512", 0)
    _raises("C", dict(kw, status=0))
    case, kw = _crop_args("outliers_0.85", 0)               # no hypothesis with 5 inliers: identity, status 0
    assert kw["status"] == 0
    _raises("C", dict(kw, status=1))
    few = kw["valid"].copy()
    few[np.nonzero(few)[0][3:]] = False                     # 3 valid points: nothing may be written, identity
    S.check_crop(**dict(kw, valid=few, records=np.full_like(kw["records"], np.nan), truth=None))
    _raises("A", dict(kw, valid=few, truth=None))


def test_mutation_known_answer():
    """stage E: an all-inlier hypothesis whose pose is off the true one (but consistent with its own count) is reported"""
    case, kw = _crop_args("shape_2x6", 0)
    a = 1e-3                                                # ~0.05 px at 46 mm / 900 mm: every point stays an inlier, counts unchanged
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    h = 7
    kw["records"][h, 2:11] = (kw["records"][h, 2:11].reshape(3, 3) @ rot).reshape(9)
    assert _raises("E", kw).hyp == h
