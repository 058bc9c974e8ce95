"""Row N11 (BOP's matching and recall scores), host side.  tests/golden/bop_eval.npz holds what the REFERENCE's own scripts saved
when they were run whole (runpy; tests/golden/make_golden_bop_eval.py): stage A, eval_calc_scores.py once per threshold column on
drawn error tables; stage B, eval_calc_errors.py for "mssd", "mspd", "proj", "add", "adi" and "ad" on a drawn world of closed-form
meshes, and eval_calc_scores.py on the errors it saved.  Checked here, without a GPU:

  - the float64 restatement tests/bop_eval_stages.py reproduces every recorded est_id, gt_id, validity, count and recall, and the
    bits of score, error and error_norm -- it is what tests/test_gpu_bop_eval.py builds its inputs with;
  - stage B: the restatement's expansion gives the recorded (scene, image, object, est_id, gt_id) list of every kind, its float64
    errors are the recorded ones to 1e-9 (inf where they are inf), and matching and scoring the recorded errors gives the recorded
    matches and scores; the maker's guards hold on the recording;
  - every mutation of bop_eval_stages.MUTATIONS (arg-min instead of the scan for E = 2, `<=` instead of `<`, the last index on
    ties, an unstable sort, validity ignored, targets without min(n_top, .), the mean over objects with targets only, n_top applied
    after pairing) changes at least one recorded value; the number of changed entries is printed;
  - the host half of checkerpose_amd.bop_eval: EvalSet.from_dicts keeps the script's row order and drops unnamed images, gt_valid
    equals the recorded validity, pairs_from_errors / expand_pairs build the tables the kernel reads (n_top before pairing, the
    script's ValueError, equal to the recorded lists of stage B), the results CSV round-trips; cp_bop_match / cp_bop_scores refuse
    bad arguments before any launch."""
import ctypes as C

import numpy as np
import pytest

from checkerpose_amd import bop_eval as BE
from tests import bop_eval_stages as S
from tests.bop_eval_stages import bits, evalset_of as _evalset, fixture

_CACHE = {}
A_CASES = ["big_c1", "big_c10", "big_rete", "small_c65", "small_c100", "scan_order"]


def restated(name):
    """rows, validity, matches and scores of a case by the restatement, once, shared"""
    if name not in _CACHE:
        fx = fixture()[name]
        rows = S.rows_of(fx["targets"], fx["gt"])
        valid = S.valid_mask(fx["targets"], fx["gt"], fx["visib"], rows, float(fx["params"][1]))
        m = S.match_all(fx, rows, valid)
        _CACHE[name] = (rows, valid, m, S.scores(fx, rows, valid, m[0]))
    return _CACHE[name]


def stage_b(kind):
    """the recorded lists of a stage B kind as (rows, pairs, err, the stage-A-shaped case, its ground-truth rows and validity)"""
    if ("B", kind) not in _CACHE:
        b = fixture()["B"]
        rows, pairs = S.expand(b, int(b[kind + "_params"][0]))
        fx = S.b_case(b, kind, rows, pairs, b[kind + "_err"])
        gt_rows = S.rows_of(fx["targets"], fx["gt"])
        _CACHE[("B", kind)] = (rows, pairs, fx, gt_rows, S.valid_mask(fx["targets"], fx["gt"], fx["visib"], gt_rows, float(fx["params"][1])))
    return _CACHE[("B", kind)]


def test_fixture_covers_what_the_issue_lists():
    f = {k: v for k, v in fixture().items() if k != "B"}
    assert sorted(fx["col_th"].shape[0] for fx in f.values()) == [1, 1, 10, 10, 65, 100]
    assert {int(fx["params"][0]) for fx in f.values()} == {1, 2, 0, -1} and {float(fx["params"][1]) for fx in f.values()} == {-1.0, 0.1}
    b = fixture()["B"]                                                       # stage B: 3 scenes of 2 - 4 images, several instances / estimates
    ims = {}
    for s, i in b["cam"].tolist():
        ims[s] = ims.get(s, 0) + 1
    assert sorted(ims.values()) == [2, 3, 4]
    n_g, n_e = {}, {}
    for k in map(tuple, b["gt"][:, :3].tolist()):
        n_g[k] = n_g.get(k, 0) + 1
    for k in map(tuple, b["est"].tolist()):
        n_e[k] = n_e.get(k, 0) + 1
    assert max(n_g.values()) >= 3 and sum(v > 1 for v in n_g.values()) >= 5 and sum(v > 1 for v in n_e.values()) >= 5
    assert any(k not in n_g for k in n_e) and any(tuple(t[:3]) not in n_e for t in b["targets"].tolist())
    for kind in ("mssd", "add", "adi", "ad"):                                # both sides of the sphere shortcut
        assert np.isinf(b[kind + "_err"]).any() and np.isfinite(b[kind + "_err"]).any()
    assert {int(b[k + "_params"][0]) for k in S.B_KINDS} == {-1, 0, 1, 2}
    big = f["big_rete"]
    key = big["m_key"]
    sizes = {}
    for k in map(tuple, key[:, :3]):
        sizes[k] = sizes.get(k, 0) + 1
    n_e = {}
    for k in map(tuple, big["est"][:, :3]):
        n_e[k] = n_e.get(k, 0) + 1
    assert {1, 2, 63, 64, 65, 130} <= set(sizes.values())
    shapes = {(n, n_e.get(k, 0)) for k, n in sizes.items()}
    assert {(1, 0), (1, 1), (63, 5), (63, 70), (64, 64), (65, 66), (130, 140), (130, 4)} <= shapes
    assert any(k not in sizes for k in n_e)                                  # estimates of an object absent from the image
    assert np.isnan(big["err"]).any() and np.isinf(big["err"]).any()
    c10 = f["big_c10"]
    assert np.isin(c10["err"], c10["col_th"]).any()                          # values equal to a threshold
    assert (key[:, 1] != 9).all() and (big["gt"][:, 1] == 9).any()           # the image no target names is dropped
    assert not big["m_valid"].all() and big["m_valid"].any()
    tg = {tuple(t[:3]): t[3] for t in big["targets"]}
    assert any(tg[k] < n for k, n in sizes.items() if k in tg)               # inst_count below the instance count
    assert (big["s_obj"][-1] == 0).all() and (big["s_scene"][-1] == 0).all()  # an object and a scene without targets


@pytest.mark.parametrize("name", A_CASES)
def test_restatement_reproduces_the_reference(name):
    fx = fixture()[name]
    rows, valid, (est, score, err, norm), sc = restated(name)
    assert np.array_equal(fx["gt"][rows], fx["m_key"])
    assert np.array_equal(valid, fx["m_valid"])
    assert np.array_equal(est, fx["m_est"])
    assert np.array_equal(bits(score), bits(fx["m_score"]))
    assert np.array_equal(bits(err), bits(fx["m_err"])) and np.array_equal(bits(norm), bits(fx["m_norm"]))
    assert np.array_equal(sc["counts"], fx["s_counts"])
    for a, b in (("recall", "s_recall"), ("obj", "s_obj"), ("scene", "s_scene"), ("mobj", "s_mobj"), ("mscene", "s_mscene")):
        assert np.array_equal(bits(sc[a]), bits(fx[b])), a


def test_scan_order_case_is_what_its_comment_says():
    fx = fixture()["scan_order"]
    assert fx["m_est"][:, 0].tolist() == [0, -1, 0, -1, -1]                 # A is kept over B; B' is kept over A' and C'
    assert fx["m_err"][0, 0].tolist() == [3.0, 3.0] and fx["m_err"][2, 0].tolist() == [4.0, 1.0]


@pytest.mark.parametrize("kind", S.B_KINDS)
def test_restatement_reproduces_stage_b(kind):
    b = fixture()["B"]
    rows, pairs, fx, gt_rows, valid = stage_b(kind)
    assert np.array_equal(rows[:, :4], b[kind + "_est"])
    assert np.array_equal(np.concatenate([rows[pairs[:, 0], :4], pairs[:, 1:]], 1), b[kind + "_key"])
    rec = b[kind + "_err"]
    host, bound = S.host_errors(b, kind, rows, pairs, want_bounds=True)
    fin = np.isfinite(rec)
    assert np.array_equal(np.isinf(host), ~fin) and (np.abs(host[fin] - rec[fin]) <= 1e-9 * rec[fin]).all()
    # the maker's guards: 4 bounds from every threshold, 1e-9 diameters from the diameter
    div, factor = S.b_scale(b, kind, rows, pairs)
    gap = np.abs(fx["err"][fin] - fx["col_th"][:, 0][None, :]).min(1)
    assert (gap >= 4.0 * (factor * bound[fin] if kind == "mspd" else bound[fin] / div[fin])).all()
    if kind in ("mssd", "add", "adi", "ad"):
        dist = np.array([np.linalg.norm(a[1] - a[3]) for a in S._b_pair_args(b, rows, pairs)])
        assert (np.abs(dist - div) >= 1e-9 * div).all() and np.array_equal(dist < div, fin)
    assert np.array_equal(fx["gt"][gt_rows], b[kind + "_m_key"]) and np.array_equal(valid, b[kind + "_m_valid"])
    est, score, err, norm = S.match_all(fx, gt_rows, valid)
    assert np.array_equal(est, b[kind + "_m_est"]) and np.array_equal(bits(score), bits(b[kind + "_m_score"]))
    assert np.array_equal(bits(err), bits(b[kind + "_m_err"])) and np.array_equal(bits(norm), bits(b[kind + "_m_norm"]))
    sc = S.scores(fx, gt_rows, valid, est)
    assert np.array_equal(sc["counts"], b[kind + "_s_counts"])
    for a, c in (("recall", "s_recall"), ("obj", "s_obj"), ("scene", "s_scene"), ("mobj", "s_mobj"), ("mscene", "s_mscene")):
        assert np.array_equal(bits(sc[a]), bits(b[kind + "_" + c])), a


def test_expand_pairs_equals_the_recorded_lists():
    b = fixture()["B"]
    es = S.evalset_of(b, poses=True)
    ests = S.b_ests(b)
    for kind in S.B_KINDS:
        p = BE.expand_pairs(es, ests, int(b[kind + "_params"][0]))
        assert np.array_equal(np.stack([p.est_scene, p.est_im, p.est_obj, p.est_id], 1), b[kind + "_est"]), kind
        key = np.stack([p.est_scene[p.pair_est], p.est_im[p.pair_est], p.est_obj[p.pair_est], p.est_id[p.pair_est], es.gt_id[p.pair_gt]], 1)
        assert np.array_equal(key, b[kind + "_key"]), kind
        assert np.array_equal(b["est"][p.est_src], b[kind + "_est"][:, :3])


@pytest.mark.parametrize("mut", S.MUTATIONS)
def test_every_mutation_is_caught(mut):
    total = 0
    if mut == "ntop_after_pairing":                                          # the expansion: stage B's recorded lists and matches
        b = fixture()["B"]
        for kind in S.B_KINDS:
            rows, pairs = S.expand(b, int(b[kind + "_params"][0]), mut)
            key = np.concatenate([rows[pairs[:, 0], :4], pairs[:, 1:]], 1)
            recorded = {tuple(k): e for k, e in zip(b[kind + "_key"].tolist(), b[kind + "_err"])}
            assert all(tuple(k) in recorded for k in key.tolist())           # it keeps fewer pairs, never others
            fx = S.b_case(b, kind, rows, pairs, np.array([recorded[tuple(k)] for k in key.tolist()]))
            _, _, _, gt_rows, valid = stage_b(kind)
            changed = int((S.match_all(fx, gt_rows, valid)[0] != b[kind + "_m_est"]).sum())
            print("mutation %-24s %-5s keeps %d of %d recorded pairs, changes %d recorded matches" % (mut, kind, len(key), len(recorded), changed))
            total += changed
        assert total >= 1
        return
    for name in ("big_c1", "big_c10", "big_rete", "scan_order"):
        fx = fixture()[name]
        rows, valid, m0, _ = restated(name)
        if mut in ("targets_no_min", "mean_with_targets_only"):
            sc = S.scores(fx, rows, valid, fx["m_est"], mut)
            total += int((sc["counts"] != fx["s_counts"]).sum() + (bits(sc["mobj"]) != bits(fx["s_mobj"])).sum()
                         + (bits(sc["recall"]) != bits(fx["s_recall"])).sum())
        else:
            if mut == "argmin" and fx["col_th"].shape[1] != 2:
                continue
            est = S.match_all(fx, rows, valid, mut)[0]
            total += int((est != fx["m_est"]).sum())
    print("mutation %-24s changes %d recorded entries" % (mut, total))
    assert total >= 1


@pytest.mark.parametrize("name", ["big_c10", "big_rete", "small_c100"])
def test_evalset_rows_validity_and_tables(name):
    fx = fixture()[name]
    es = _evalset(fx)
    assert np.array_equal(np.stack([es.gt_scene, es.gt_im, es.gt_obj, es.gt_id], 1), fx["m_key"])
    assert np.array_equal(BE.gt_valid(es, float(fx["params"][1])), fx["m_valid"])
    assert np.array_equal(BE.gt_valid(es, 0.3), S.valid_mask(fx["targets"], fx["gt"], fx["visib"], S.rows_of(fx["targets"], fx["gt"]), 0.3))
    pairs, table = BE.pairs_from_errors(es, S.scene_errs_of(fx))
    n_g = np.diff(es.grp_off)
    n_e = np.diff(pairs.k_est_off)
    assert np.array_equal(np.diff(pairs.k_pair_off), n_e * n_g) and pairs.k_pair_off[-1] == pairs.k_pair.shape[0]
    assert (pairs.est_group == -1).any()                                     # absent object / unnamed image: no group
    for g in (0, es.n_groups // 2, es.n_groups - 1):                         # the block of a group is estimate-major, gt_id ascending
        rows = es.grp_rows[es.grp_off[g]:es.grp_off[g + 1]]
        assert (np.diff(es.gt_id[rows]) > 0).all()
        blk = pairs.k_pair[pairs.k_pair_off[g]:pairs.k_pair_off[g + 1]].reshape(n_e[g], n_g[g])
        assert (pairs.pair_gt[blk] == rows[None, :]).all()
        assert (pairs.pair_est[blk] == pairs.k_rows[pairs.k_est_off[g]:pairs.k_est_off[g + 1]][:, None]).all()
    assert table.shape == (pairs.pair_est.shape[0], fx["err"].shape[1])


def test_expand_pairs_selects_before_pairing_and_raises_like_the_script():
    targets = [{"scene_id": 1, "im_id": 0, "obj_id": 7, "inst_count": 2}, {"scene_id": 1, "im_id": 0, "obj_id": 8, "inst_count": 1}]
    scene_gt = {1: {0: [{"obj_id": 7}, {"obj_id": 9}, {"obj_id": 7}]}}
    es = BE.EvalSet.from_dicts(targets, scene_gt, None, [1], [7, 8, 9])
    ests = [{"scene_id": 1, "im_id": 0, "obj_id": 7, "score": s} for s in (0.2, 0.9, 0.9, 0.5)]
    ests += [{"scene_id": 1, "im_id": 0, "obj_id": 9, "score": 1.0}, {"scene_id": 1, "im_id": 0, "obj_id": 8, "score": 1.0}]
    for n_top, want in ((1, [1]), (2, [1, 2]), (-1, [1, 2]), (0, [1, 2, 3, 0])):     # stable by descending score, est_id = list index
        p = BE.expand_pairs(es, ests, n_top)
        sel = p.est_obj == 7
        assert p.est_id[sel].tolist() == want, n_top
        assert p.pair_est.shape[0] == 2 * len(want)                          # n_top estimates x BOTH ground truths, not n_top pairs
        assert p.pair_gt.reshape(-1, 2).tolist() == [[0, 2]] * len(want)
        assert (p.est_obj == 9).sum() == 0 and (p.est_obj == 8).sum() == 1   # targets' estimates only; object 8 has no ground truth
    with pytest.raises(ValueError, match="Not enough estimates"):
        BE.expand_pairs(es, ests[:1] + ests[4:], -1, skip_missing=False)


def test_results_csv_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    res = [{"scene_id": 2, "im_id": 3 + k, "obj_id": 5, "score": float(rng.random()), "R": rng.normal(size=(3, 3)),
            "t": rng.normal(size=(3, 1)) * 100, "time": 0.25} for k in range(3)]
    path = str(tmp_path / "m_lmo-test.csv")
    BE.save_bop_results(path, res)
    assert open(path).readline().strip() == "scene_id,im_id,obj_id,score,R,t,time"
    back = BE.load_bop_results(path)
    for a, b in zip(res, back):
        assert (a["scene_id"], a["im_id"], a["obj_id"], a["score"], a["time"]) == (b["scene_id"], b["im_id"], b["obj_id"], b["score"], b["time"])
        assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and b["t"].shape == (3, 1)


def test_no_cpu_fallback():
    """a "cpu" device is refused whether or not the machine has a GPU: nothing is computed on the host instead"""
    fx = fixture()["scan_order"]
    targets, scene_gt, info = S.dicts_of(fx)
    es = BE.EvalSet.from_dicts(targets, scene_gt, info, fx["scene_ids"].tolist(), fx["obj_ids"].tolist(), device="cpu")
    pairs, table = BE.pairs_from_errors(es, S.scene_errs_of(fx))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BE.match(pairs, table, fx["col_th"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BE.localization_scores(es, np.zeros((es.n_gt, 1), dtype=np.int32), None, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BE.match_poses([{"est_id": 0, "score": 1.0, "errors": {0: [1.0]}}], [2.0], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BE.calc_localization_scores([1], [1], [{"scene_id": 1, "im_id": 0, "obj_id": 1, "gt_id": 0, "est_id": 0, "valid": True}], 1, device="cpu")


def test_scores_refuse_a_valid_ground_truth_outside_the_lists():
    """score.calc_localization_scores raises KeyError for a valid ground truth whose object or scene is not listed"""
    fx = fixture()["scan_order"]
    targets, scene_gt, info = S.dicts_of(fx)
    es = BE.EvalSet.from_dicts(targets, scene_gt, info, [1, 2], [2], device="cpu")   # object 1 is not listed
    with pytest.raises(KeyError):
        BE.localization_scores(es, np.zeros((es.n_gt, 1), dtype=np.int32), None, 0)


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    assert lib.cp_version() >= 212
    A = C.c_void_p(0x10000)

    def call(**kw):
        a = dict(errs=A, P=4, C_err=1, score=A, ids=A, NE=2, eoff=A, goff=A, poff=A, G=1, rows=None, valid=None, NG=2, cerr=A, cth=A,
                 C=3, E=1, max_ests=0, moff=None, words=0, flags=0, oe=A, osc=A, oer=A, on=A, scratch=A)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = lib.cp_bop_match(None, a["errs"], a["P"], a["C_err"], a["score"], a["ids"], a["NE"], a["eoff"], a["goff"], a["poff"], a["G"],
                              a["rows"], a["valid"], a["NG"], a["cerr"], a["cth"], a["C"], a["E"], a["max_ests"], a["moff"], a["words"],
                              a["flags"], a["oe"], a["osc"], a["oer"], a["on"], a["scratch"])
        assert lib.cp_kernel_log() == b"", kw
        return rc
    for bad in (dict(E=0), dict(E=3), dict(C=0), dict(G=0), dict(NG=0), dict(C_err=0), dict(NE=-1), dict(P=-1), dict(flags=4),
                dict(errs=None), dict(score=None), dict(ids=None), dict(eoff=None), dict(goff=None), dict(poff=None), dict(cerr=None),
                dict(cth=None), dict(oe=None), dict(osc=None), dict(oer=None), dict(on=None), dict(scratch=None), dict(words=2)):
        assert call(**bad) == -1, bad
    for bad in (dict(scratch=C.c_void_p(0x10008)), dict(errs=C.c_void_p(0x10004)), dict(poff=C.c_void_p(0x10004)), dict(oe=C.c_void_p(0x10002))):
        assert call(**bad) == -3, bad
    assert lib.cp_bop_match_scratch_bytes(5, 3, 10) == 32 + 240 + 16 and lib.cp_bop_match_scratch_bytes(0, 0, 0) == 0
    lib.cp_kernel_log_begin()
    assert lib.cp_bop_scores(None, A, None, A, A, 2, A, None, 1, 3, 0, 1, 1, 0, A) == -1          # no objects listed
    assert lib.cp_bop_scores(None, A, None, A, A, 2, A, None, 1, 3, 2, 1, 1, 2, A) == -1          # unknown flag
    assert lib.cp_bop_scores(None, None, None, A, A, 2, A, None, 1, 3, 2, 1, 1, 0, A) == -1
    assert lib.cp_bop_scores(None, A, None, A, A, 2, A, None, 1, 3, 2, 1, 1, 0, C.c_void_p(0x10002)) == -3
    assert lib.cp_kernel_log() == b""
