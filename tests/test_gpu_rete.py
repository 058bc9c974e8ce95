"""Row N23 on the device: cp_pose_rete / cp_rete_pass_counts through checkerpose_amd.targets and bop_eval, against the numpy restatement
(tests/rete_stages.py) and what the reference's own functions recorded (tests/golden/rete.npz).

Tolerances (none tuned on the device's output; EPS = 2^-53 as in tests/test_gpu_targets.py):
  cos   |device - reference| <= 64 EPS, the project's bound for the cofactor cosine.  The 3 x 3 product in front of it is three
        products and two sums per entry of a matrix with entries of magnitude <= 1: at most 3 EPS per entry, nine entries weighted by
        cofactors of magnitude <= 1 -- 27 EPS in the worst case, inside the 64.
  re    degrees(d / sqrt(1 - cos^2)) with d = 64 EPS; degrees(acos(1 - d)) where |cos| > 1 - 1e-9; exactly 0.0 for bitwise-equal matrices
  te    8 EPS (|t_a| + |t_b|)
  index equal to the restatement's / the reference's, except where the device's candidate lies within 2 tol of the best one (then the
        value alone is compared); at most 5 % of the symmetric pairs may do so.  Bitwise-equal candidates are decided by "first wins".
Flags, counts, rates, matches and the report text are exact: the maker keeps every recorded error clear of its thresholds."""
import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, bop_eval as BE, scene, targets
from tests import bop_eval_stages as S
from tests import rete_stages as RS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_SHARED = {}


def _up(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int64) if a.dtype == np.float64 else a


def case_tables():
    """the fixture's four sets as (S,12) tables: from_models_info(rotations_as=np.float32), once"""
    if "tables" not in _SHARED:
        fx = RS.fixture()
        info = RS.models_info(fx)
        ss = scene.SymmetrySet.from_models_info([info[int(o)] for o in fx["case_objs"]], rotations_as=np.float32)
        t, off = ss.table.numpy(), ss.offsets.numpy()
        _SHARED["tables"] = (ss, [t[off[m]:off[m + 1]] for m in range(len(ss))])
    return _SHARED["tables"]


def set_of(tables):
    """a SymmetrySet of the given (S,12) tables (S = 0 allowed: from_transforms refuses an empty set, the kernel does not)"""
    off = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int32)
    return scene.SymmetrySet(torch.from_numpy(np.ascontiguousarray(np.concatenate(tables, 0))), torch.from_numpy(off))


def device(R_est, t_est, R_gt, t_gt, tables=None, mesh_ids=None):
    out = targets.pose_re_te_sym(_up(R_est), t_est, R_gt, t_gt, symmetries=None if tables is None else set_of(tables), mesh_ids=mesh_ids,
                                 return_cos=True, return_index=True, return_closest=True)
    return [o.cpu().numpy() for o in out]


def compare(got, R_est, t_est, R_gt, t_gt, tables, mesh_ids, ref=None):
    """the device's (re, te, cos, index, closest) against the restatement (and, with ref = (re, cos, te, index, gap), the recording)
    -> the number of pairs whose index was compared by value only"""
    re, te, cs, idx, closest = got
    r_re, r_te, r_cs, r_idx = RS.rete_batch(R_est, t_est, R_gt, t_gt, tables, mesh_ids)
    if ref is not None:
        assert (np.abs(r_re - ref[0]) <= RS.tol_re(ref[1])).all()
        r_re, r_cs, r_te = ref[0], ref[1], ref[2]
    tol = RS.tol_re(r_cs)
    assert (np.abs(te - r_te) <= RS.tol_te(t_est, t_gt)).all()
    loose = 0
    for p in range(len(re)):
        T = None if tables is None else tables[0 if mesh_ids is None else int(mesh_ids[p])]
        Sm = None if T is None else T[:, :9].reshape(-1, 3, 3)
        assert abs(re[p] - r_re[p]) <= tol[p], (p, re[p], r_re[p], tol[p])
        assert -1 <= idx[p] < (0 if T is None else len(T))
        want = r_idx[p] if ref is None else ref[3][p]
        if idx[p] != want:
            if ref is not None:                                      # the reference's own two best distinct candidates are this close
                assert ref[4][p] <= 2.0 * tol[p], (p, idx[p], want)
            res = RS.candidate_res(R_est[p], R_gt[p], Sm)
            assert res[idx[p] + 1] - res.min() <= 2.0 * tol[p], (p, idx[p], want)
            cand = RS.candidates(R_gt[p], Sm)
            assert not np.array_equal(cand[idx[p] + 1], cand[want + 1]), (p, "bitwise-equal candidates: the first wins")
            loose += 1
        else:
            assert abs(cs[p] - r_cs[p]) <= RS.tol_cos(), (p, cs[p], r_cs[p])
        mat = R_gt[p] if idx[p] < 0 else R_gt[p].dot(Sm[idx[p]])
        assert np.abs(closest[p] - mat).max() <= 16 * RS.EPS, p      # R_gt . S on either side: 3 roundings of sums <= sqrt(3) each, x 2, fused or not
    return loose


def test_fixture_cases_in_one_call():
    fx = RS.fixture()
    _, tables = case_tables()
    a = (fx["case_R_est"], fx["case_t_est"], fx["case_R_gt"], fx["case_t_gt"])
    got = device(*a, tables, fx["case_mesh"])
    loose = compare(got, *a, tables, fx["case_mesh"], ref=(fx["case_re"], fx["case_cos"], fx["case_te"], fx["case_index"], fx["case_gap"]))
    sym = int((fx["case_mesh"] > 0).sum())
    print("%d pairs, %d symmetric, %d indices compared by value only" % (len(got[0]), sym, loose))
    assert loose <= 0.05 * sym
    equal = fx["case_kind"] == 2
    assert (got[0][equal] == 0.0).all() and (got[3][equal] == -1).all() and (got[2][equal] == 1.0).all()
    disc = fx["case_mesh"] == 1                                      # plain ground truth against the identity member: exactly decided
    assert np.array_equal(got[3][disc], fx["case_index"][disc]) and (got[3][disc] == -1).sum() > 10


@pytest.mark.parametrize("S_size", [0, 1, 2, 63, 64, 65, 314, 628])
def test_grid_against_the_restatement(S_size):
    fx = RS.fixture()
    _, (t1, t2, t314, t628) = case_tables()
    first = {0: t628[:0], 1: t1, 2: t2, 314: t314, 628: t628}.get(S_size, t628[:S_size])
    tables = [first, t2, t314[:40]]                                  # pairs of one call mix sets of different sizes
    loose = total = 0
    for P in (1, 3, 4, 5, 257):
        rng = np.random.default_rng(1000 * S_size + P)
        pick = rng.integers(0, len(fx["case_re"]), size=P)
        mesh = np.where(rng.random(P) < 0.7, 0, rng.integers(1, 3, size=P)).astype(np.int64)
        mesh[0] = 0
        R_gt, t_gt, t_est = fx["case_R_gt"][pick], fx["case_t_gt"][pick], fx["case_t_est"][pick]
        R_est = fx["case_R_est"][pick].copy()
        for p in range(P):                                           # near a symmetric copy of the pair's own set, or as drawn
            T = tables[mesh[p]]
            if len(T) and rng.random() < 0.6:
                R_est[p] = RS.candidates(R_gt[p], T[:, :9].reshape(-1, 3, 3))[1 + int(rng.integers(len(T)))] @ _small(rng)
        got = device(R_est, t_est, R_gt, t_gt, tables, mesh)
        loose += compare(got, R_est, t_est, R_gt, t_gt, tables, mesh)
        total += P
        if S_size == 0 and P == 5:                                   # without a table: the same bits as an empty set
            plain = device(R_est, t_est, R_gt, t_gt)
            m0 = mesh == 0
            assert all(np.array_equal(_bits(a[m0]), _bits(b[m0])) for a, b in zip(got, plain)) and (plain[3] == -1).all()
    assert loose <= 0.05 * total


def _small(rng, angle=None):
    a = rng.normal(size=3)
    a *= (rng.uniform(0.01, 0.06) if angle is None else angle) / np.linalg.norm(a)
    th = np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]) / th
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def test_exact_ties_and_the_identity():
    fx = RS.fixture()
    _, (t1, t2, t314, t628) = case_tables()
    R = fx["case_R_gt"][:6]
    t = fx["case_t_gt"][:6]
    re, te, cs, idx, closest = device(R, t, R, t, [t2], None)        # R_est = R_gt, the identity is a member
    assert (re == 0.0).all() and (idx == -1).all() and (cs == 1.0).all() and (te == 0.0).all() and np.array_equal(closest, R)
    twice = np.concatenate([t314[5:6], t314[9:10], t314[9:10], t314[5:6], t314[9:10]], 0)      # the same rotation several times
    for k, want in ((5, 0), (9, 1)):
        R_est = np.stack([RS.product(r, t314[k, :9].reshape(3, 3)) for r in R])      # the candidate's own bits (numpy's dot may fuse)
        re, _, cs, idx, _ = device(R_est, t, R, t, [twice], None)
        assert (re == 0.0).all() and (cs == 1.0).all() and (idx == want).all()      # an exact copy: 0 degrees, the lower index
        # 0.005 rad off the copy: the two rotations of the table are four steps of the continuous axis (0.08 rad) apart
        re, _, _, idx, _ = device(np.stack([r @ _small(np.random.default_rng(k), 0.005) for r in R_est]), t, R, t, [twice], None)
        assert (idx == want).all() and (re > 0.1).all()


def test_nan_and_singular_input_stay_in_their_pair():
    fx = RS.fixture()
    _, tables = case_tables()
    n = 9
    a = [fx[k][60:60 + n].copy() for k in ("case_R_est", "case_t_est", "case_R_gt", "case_t_gt")]
    mesh = np.array([0, 1, 2, 3, 0, 1, 2, 3, 2])
    clean = device(*a, tables, mesh)
    a[2][1, 0, 0] = np.nan                                           # a NaN in R_gt
    a[2][3] = 0.0                                                    # a singular R_gt
    a[0][5, 2, 1] = np.nan                                           # a NaN in R_est
    a[2][7] = np.ones((3, 3))                                        # singular, not zero
    re, te, cs, idx, _ = device(*a, tables, mesh)
    bad = np.array([1, 3, 5, 7])
    good = np.array([0, 2, 4, 6, 8])
    assert np.isnan(re[bad]).all() and (idx[bad] == -1).all() and not np.isfinite(cs[bad]).any()
    assert np.array_equal(_bits(te), _bits(clean[1]))                # te does not look at the rotations
    for x, y in zip((re, cs, idx), (clean[0], clean[2], clean[3])):
        assert np.array_equal(_bits(x[good]), _bits(y[good]))
    # a mesh id outside the sets: refused on the host, NaN / -1 from ids that live on the device
    with pytest.raises(ValueError, match="mesh_ids"):
        targets.pose_re_te_sym(_up(a[0]), a[1], a[2], a[3], symmetries=set_of(tables), mesh_ids=np.array([0, 1, 2, 3, 4, 1, 2, 3, 2]))
    with pytest.raises(ValueError, match="mesh_ids"):
        targets.pose_re_te_sym(_up(a[0]), a[1], a[2], a[3], symmetries=set_of(tables))
    with pytest.raises(ValueError, match="mesh_ids"):
        targets.pose_re_te_sym(_up(a[0]), a[1], a[2], a[3], symmetries=set_of(tables), mesh_ids=mesh[:4])
    with pytest.raises(ValueError, match="mesh_ids"):
        targets.pose_re_te_sym(_up(a[0]), a[1], a[2], a[3], mesh_ids=mesh)
    ids = _up(np.array([0, 4, 2, 3, -1, 1, 2, 3, 2], dtype=np.int32))
    re2, te2, idx2 = targets.pose_re_te_sym(_up(clean_inputs(fx, n)[0]), *clean_inputs(fx, n)[1:], symmetries=set_of(tables), mesh_ids=ids, return_index=True)
    re2, idx2 = re2.cpu().numpy(), idx2.cpu().numpy()
    assert np.isnan(re2[[1, 4]]).all() and (idx2[[1, 4]] == -1).all()
    keep = np.array([0, 2, 3, 5, 6, 7, 8])
    assert np.array_equal(_bits(re2[keep]), _bits(clean[0][keep])) and np.array_equal(_bits(te2), _bits(clean[1]))


def clean_inputs(fx, n):
    return [fx[k][60:60 + n] for k in ("case_R_est", "case_t_est", "case_R_gt", "case_t_gt")]


def test_without_symmetries_equals_the_entry_point_with_no_table():
    fx = RS.fixture()
    Re, te_, Rg, tg = (fx[k] for k in ("case_R_est", "case_t_est", "case_R_gt", "case_t_gt"))
    P = len(Re)
    re, te, cs, idx = targets.pose_re_te_sym(_up(Re), te_, Rg, tg, return_cos=True, return_index=True)
    A, B = _up(np.concatenate([Re.reshape(P, 9), te_], 1)), _up(np.concatenate([Rg.reshape(P, 9), tg], 1))
    out = [torch.empty(P, dtype=torch.float64, device=DEV) for _ in range(3)] + [torch.empty(P, dtype=torch.int32, device=DEV)]
    _abi.call("cp_pose_rete", A.device, A, B, P, None, None, None, 0, None, None, *out)
    for x, y in zip((re, te, cs, idx), out):
        assert np.array_equal(_bits(x), _bits(y))
    assert (idx.cpu().numpy() == -1).all()
    re2, te2 = targets.pose_re_te_sym(_up(Re), te_, Rg, tg)          # the optional outputs change nothing
    assert torch.equal(re2, re) and torch.equal(te2, te)
    ref_re, ref_te = targets.pose_re_te(_up(Re), te_, Rg, tg)        # the torch expression: the same quantity, its own rounding
    assert (np.abs(re.cpu().numpy() - ref_re.cpu().numpy()) <= 2.0 * RS.tol_re(cs.cpu().numpy())).all()
    assert (np.abs(te.cpu().numpy() - ref_te.cpu().numpy()) <= 2.0 * RS.tol_te(te_, tg)).all()


def _world_b():
    if "B" not in _SHARED:
        b = S.fixture()["B"]
        _SHARED["B"] = (b, S.evalset_of(b, poses=True), S.b_ests(b), {int(o): k for k, o in enumerate(b["obj_ids"])})
    return _SHARED["B"]


def test_calc_errors_and_match_reproduce_the_references_matches():
    fx = RS.fixture()
    b, es, ests, obj_index = _world_b()
    n_top, visib_gt_min = int(fx["match_params"][0]), float(fx["match_params"][1])
    pairs = BE.expand_pairs(es, ests, n_top)
    key = np.stack([pairs.est_scene[pairs.pair_est], pairs.est_im[pairs.pair_est], pairs.est_obj[pairs.pair_est], pairs.est_id[pairs.pair_est],
                    es.gt_id[pairs.pair_gt]], 1)
    assert np.array_equal(key, fx["match_key"])
    both = BE.calc_errors(pairs, ests, "rete", None, obj_index)
    e_re, e_te = BE.calc_errors(pairs, ests, "re", None, obj_index), BE.calc_errors(pairs, ests, "te", None, obj_index)
    assert tuple(both.shape) == (len(key), 2) and tuple(e_re.shape) == (len(key), 1) == tuple(e_te.shape)
    assert torch.equal(both, torch.cat([e_re, e_te], 1))
    got, rec = both.cpu().numpy(), fx["match_err"]
    rows, prs = S.expand(b, n_top)
    args = list(S._b_pair_args(b, rows, prs))
    cos = np.array([RS.cos_cof(a[0], a[2]) for a in args])
    assert (np.abs(got[:, 0] - rec[:, 0]) <= RS.tol_re(cos)).all()
    assert (np.abs(got[:, 1] - rec[:, 1]) <= RS.tol_te(np.stack([a[1] for a in args]), np.stack([a[3] for a in args]))).all()
    valid = BE.gt_valid(es, visib_gt_min)
    assert np.array_equal(valid, fx["match_m_valid"])
    m = BE.match(pairs, both, fx["match_th"], n_top=n_top, valid=valid)
    sc = BE.localization_scores(es, m, valid, n_top)
    assert np.array_equal(m["est_id"].cpu().numpy(), fx["match_m_est"])
    assert np.array_equal(_bits(m["score"]), _bits(fx["match_m_score"]))
    assert np.array_equal(np.stack([es.gt_scene, es.gt_im, es.gt_obj, es.gt_id], 1), fx["match_m_key"])
    assert np.array_equal(sc["tp_count"], fx["match_s_counts"][:, 2]) and np.array_equal(_bits(np.asarray(sc["recall"])), _bits(fx["match_s_recall"]))
    res = BE.evaluate_results(es, ests, None, obj_index, None, im_width=int(b["width"]), kinds=("re", "te", "rete"))
    assert set(k for k in res if k.startswith("AR")) == {"AR_RE", "AR_TE", "AR_RETE"}
    assert res["AR_RETE"] == float(fx["match_s_recall"][0])          # the first recorded column is eval_calc_scores.py's [5.0, 5.0]
    assert res["AR_RETE"] <= min(res["AR_RE"], res["AR_TE"])


def test_evaluate_batch_keyword():
    from checkerpose_amd import metric
    from tests.common import build_net
    from tests.test_gpu_targets import _scene
    from tests.test_targets import lm_keypoints
    B = 2
    frames, vis, full, Rs, ts, K, boxes = _scene(B, seed=9)
    pts = lm_keypoints(1, 512).astype(np.float32)
    net = build_net(seed=1).cuda().eval()
    ms = metric.MeshSet.from_arrays([pts], diameters=[100.0])
    args = (net, _up(frames), _up(vis), _up(full), boxes, pts, K, Rs, ts, ms)
    base = targets.evaluate_batch(*args)
    none = targets.evaluate_batch(*args, re_symmetries=None)
    _, (t1, t2, t314, t628) = case_tables()
    sym = targets.evaluate_batch(*args, re_symmetries=set_of([t314]))
    for name in targets.COLUMNS:
        assert set(none[name]) == set(base[name]) and "re_index" not in base[name]
        for k in ("re", "te", "R", "t", "status"):
            assert torch.equal(none[name][k], base[name][k]), (name, k)
        assert all(torch.equal(none[name]["errors"][k], base[name]["errors"][k]) for k in base[name]["errors"])
        re, te, idx = targets.pose_re_te_sym(base[name]["R"], base[name]["t"], Rs, ts, symmetries=set_of([t314]), return_index=True)
        assert torch.equal(sym[name]["re"], re) and torch.equal(sym[name]["te"], te) and torch.equal(sym[name]["re_index"], idx)
        assert sym[name]["re_index"].dtype == torch.int32


def _on_threshold(P, n_obj, seed):
    """errors drawn from a few values, the thresholds themselves and NaN among them"""
    rng = np.random.default_rng(seed)
    diam = rng.choice([100.0, 250.0, 64.0], size=P)
    adx = diam * rng.choice([0.01, 0.02, 0.03, 0.05, 0.07, 0.1, 0.2], size=P)
    adx[rng.random(P) < 0.1] = np.nan
    re = rng.choice([0.5, 2.0, np.nextafter(2.0, 0.0), 3.0, 5.0, np.nextafter(5.0, 0.0), 9.0, np.nan], size=P)
    te = rng.choice([3.0, 20.0, np.nextafter(20.0, 0.0), 30.0, 50.0, np.nextafter(50.0, 0.0), 70.0, np.nan], size=P)
    return re, te, adx, diam, rng.integers(0, n_obj, size=P)


@pytest.mark.parametrize("n_obj", [1, 13])
def test_pass_counts_are_the_restatements_integers(n_obj):
    for P in (1, 255, 256, 257, 4099):
        re, te, adx, diam, slot = _on_threshold(P, n_obj, 7 * P + n_obj)
        want = RS.pass_counts(re, te, adx, diam, slot, n_obj)
        got = targets.rete_pass_counts(_up(re), te, adx, diam, slot, n_obj)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (n_obj, P)
        again = targets.rete_pass_counts(_up(re), _up(te), _up(adx), _up(diam), _up(slot.astype(np.int32)), n_obj)     # slots on the device
        assert torch.equal(got, again)
    on = RS.pass_flags(np.array([2.0, 5.0]), np.array([20.0, 50.0]), np.array([2.0, 10.0]), np.array([100.0, 100.0]))
    assert on[:, 4:].sum() == 3 and on[0, 1:4].tolist() == [0, 1, 1]   # ON a threshold fails it (strict): only re 2 < 5, te 20 < 50 pass
    with pytest.raises(ValueError, match="slots"):
        targets.rete_pass_counts(_up(re), te, adx, diam, np.full(len(re), n_obj), n_obj)
    with pytest.raises(ValueError, match="n_obj"):
        targets.rete_pass_counts(_up(re), te, adx, diam, slot, 257)
    stray = targets.rete_pass_counts(_up(re[:5]), te[:5], adx[:5], diam[:5], _up(np.array([0, n_obj, -1, 0, 0], dtype=np.int32)), n_obj)
    assert int(stray[0, 0]) == 3 and int(stray[:, 0].sum()) == 3     # a stray slot that lives on the device is skipped


def test_summarize_report_lm_gives_the_recorded_text():
    fx = RS.fixture()
    lm13 = fx["rep_lm13"].tolist()
    info = RS.models_info(fx)
    syms = scene.SymmetrySet.from_models_info([info[o] for o in lm13], rotations_as=np.float32)
    slot = np.array([lm13.index(o) for o in fx["rep_obj"].tolist()])
    n = len(slot)
    re, te, idx = targets.pose_re_te_sym(_up(fx["rep_R_est"]), fx["rep_t_est"], fx["rep_R_gt"], fx["rep_t_gt"], symmetries=syms, mesh_ids=slot,
                                         return_index=True)
    asym = ~np.isin(fx["rep_obj"], fx["rep_symmetry_ids"])
    assert (idx.cpu().numpy()[asym] == -1).all() and (idx.cpu().numpy()[~asym] >= 0).any()
    noise = torch.full((n,), 1e6, dtype=torch.float64, device=DEV)
    batches = []
    for lo, hi in ((0, 50), (50, n)):                                # two batches, as a test loop accumulates them
        col = {"re": re[lo:hi], "te": te[lo:hi], "errors": {"add": _up(fx["rep_add"][lo:hi]), "adi": _up(fx["rep_adi"][lo:hi])}}
        other = {"re": noise[lo:hi], "te": noise[lo:hi], "errors": {"add": noise[lo:hi], "adi": noise[lo:hi]}}
        rep = {k: _up(fx["rep_fig_" + k][lo:hi]) for k in targets.FIGURES}
        rep["bit_err_arr"] = _up(fx["rep_fig_bit_err_arr"][lo:hi])
        batches.append({"all": col, "full": other, "visib": other, "report": rep})
    diam = {int(o): float(info[int(o)]["diameter"]) for o in lm13}
    res, text = targets.summarize_report_lm(batches, fx["rep_obj"], diam)
    assert text == str(fx["rep_text"])
    assert np.array_equal(res["counts"][:, 1:], np.stack([fx["rep_flags"][slot == k].sum(0) for k in range(13)]))
    assert np.array_equal(np.stack([res["per_object"][k] for k in targets.RETE_COUNTS[1:]], 1), fx["rep_rates"])
    assert [res[k] for k in targets.RETE_COUNTS[1:]] == fx["rep_overall"].tolist()
    _, text_d = targets.summarize_report_lm(batches, fx["rep_obj"], fx["rep_diam"])          # one diameter per crop
    assert text_d == text
    _, other_text = targets.summarize_report_lm(batches, fx["rep_obj"], diam, adx_type="visib")
    assert other_text.startswith("adx_type visib\nacc 0.0000\n") and other_text != text
