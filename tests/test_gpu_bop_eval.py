"""Row N11 on the device: cp_bop_match / cp_bop_scores through checkerpose_amd.bop_eval against tests/golden/bop_eval.npz (what the
reference's eval_calc_errors.py and eval_calc_scores.py saved, run whole; fixture and restatement: tests/bop_eval_stages.py).

  exact        every est_id, score, error, error_norm (bits), count and recall of every stage A case equals the recording
  stage B      expand_pairs gives the recorded pair lists; calc_errors' "mssd" / "mspd" / "proj" / "add" / "adi" / "ad" lie within
               rows N7's / N5's bounds of the recorded errors (inf where they are inf); the matches, counts and recalls after them
               equal the recording exactly (the maker's guards keep every error 4 bounds from every threshold); evaluate_results
               on the multi-estimate world gives the recorded MSSD and MSPD recalls
  structures   match_poses, match_poses_scene and calc_localization_scores return the reference's lists / dicts
  invariance   the same bits from two calls, for an image alone or in the batch, columns alone or together, the error block staged
               through LDS or read from global memory, the matched set in a register or in scratch (n_g = 64 and 65 are among the
               groups), the counts through LDS bins or global integer atomics
  errors       calc_errors(kind="vsd") equals metric.vsd_errors on the expanded pairs bit for bit; the sphere shortcut of "mssd" / "add"
  end to end   evaluate_results on a one-estimate-per-target set equals metric.summarize_bop on the same errors"""
import numpy as np
import pytest
import torch

from checkerpose_amd import bop_eval as BE, metric
from tests import bop_eval_stages as S
from tests import vsd_stages as V
from tests.bop_eval_stages import bits, evalset_of as _evalset, fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ["big_c1", "big_c10", "big_rete", "small_c65", "small_c100", "scan_order"]
_RUNS = {}


def run(name, **kw):
    """a stage A case through match + localization_scores (numpy back), once per variant, shared"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _RUNS:
        fx = fixture()[name]
        es = _evalset(fx)
        pairs, table = BE.pairs_from_errors(es, S.scene_errs_of(fx))
        valid = BE.gt_valid(es, float(fx["params"][1]))
        bins = kw.pop("_bins", None)
        m = BE.match(pairs, table, fx["col_th"], err_cols=fx["col_err"], n_top=int(fx["params"][0]), valid=valid, **kw)
        torch.cuda.synchronize()
        sc = BE.localization_scores(es, m, valid, int(fx["params"][0]), _bins=bins)
        _RUNS[key] = ({k: m[k].cpu().numpy() for k in ("est_id", "score", "error", "error_norm")}, sc, es)
    return _RUNS[key]


def same(a, b):
    return all(np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k], b[k].view(np.int64) if b[k].dtype == np.float64 else b[k])
               for k in ("est_id", "score", "error", "error_norm"))


@pytest.mark.parametrize("name", CASES)
def test_stage_a_is_exact(name):
    fx = fixture()[name]
    m, sc, es = run(name)
    assert np.array_equal(m["est_id"], fx["m_est"])
    assert np.array_equal(bits(m["score"]), bits(fx["m_score"]))
    assert np.array_equal(bits(m["error"]), bits(fx["m_err"])) and np.array_equal(bits(m["error_norm"]), bits(fx["m_norm"]))
    assert sc["gt_count"] == fx["s_counts"][0, 0] and sc["targets_count"] == fx["s_counts"][0, 1]
    assert np.array_equal(sc["tp_count"], fx["s_counts"][:, 2])
    for a, b in (("recall", "s_recall"), ("obj_recalls", "s_obj"), ("scene_recalls", "s_scene"), ("mean_obj_recall", "s_mobj"),
                 ("mean_scene_recall", "s_mscene")):
        assert np.array_equal(bits(sc[a]), bits(fx[b])), a
    one = BE.scores_of_column(sc, es, 0)
    assert one["obj_recalls"][int(fx["obj_ids"][0])] == fx["s_obj"][0, 0] and one["tp_count"] == fx["s_counts"][0, 2]


@pytest.mark.parametrize("name", ["big_c10", "big_rete", "small_c100"])
def test_paths_and_calls_give_the_same_bits(name):
    base = run(name)
    fx = fixture()[name]
    for kw in (dict(_stage="global"), dict(_mask="scratch"), dict(_stage="global", _mask="scratch"), dict(_stage="lds", _bins="global")):
        other = run(name, **kw)
        assert same(base[0], other[0]), kw
        assert np.array_equal(base[1]["tp_count"], other[1]["tp_count"]) and np.array_equal(base[1]["obj_tp"], other[1]["obj_tp"])
        assert np.array_equal(base[1]["scene_tp"], other[1]["scene_tp"]) and np.array_equal(base[1]["obj_targets"], other[1]["obj_targets"])
    _RUNS.pop((name, ()))
    assert same(base[0], run(name)[0])                                       # a second call
    es = base[2]
    pairs, table = BE.pairs_from_errors(es, S.scene_errs_of(fx))
    valid = BE.gt_valid(es, float(fx["params"][1]))
    for cols in ([0], [fx["col_th"].shape[0] - 1], list(range(1, fx["col_th"].shape[0], 3))):       # columns alone or together
        m = BE.match(pairs, table, fx["col_th"][cols], err_cols=fx["col_err"][cols], n_top=int(fx["params"][0]), valid=valid)
        for k in ("est_id", "score", "error", "error_norm"):
            assert np.array_equal(m[k].cpu().numpy(), base[0][k][:, cols]), (k, cols)


def test_an_image_alone_equals_the_image_in_the_batch():
    fx = fixture()["big_rete"]
    base = run("big_rete")[0]
    for scene, im in ((2, 1), (1, 2), (2, 2)):                               # the images with the 64-, 65- and 130-instance groups
        sub = dict(fx)
        sub["targets"] = fx["targets"][(fx["targets"][:, 0] == scene) & (fx["targets"][:, 1] == im)]
        es = _evalset(sub)
        errs = {scene: [e for e in S.scene_errs_of(fx)[scene] if e["im_id"] == im]}
        pairs, table = BE.pairs_from_errors(es, errs)
        m = BE.match(pairs, table, fx["col_th"], err_cols=fx["col_err"], n_top=int(fx["params"][0]), valid=BE.gt_valid(es, -1))
        rows = np.nonzero((fx["m_key"][:, 0] == scene) & (fx["m_key"][:, 1] == im))[0]
        assert max(np.bincount(es.gt_obj)) >= 63
        for k in ("est_id", "score", "error", "error_norm"):
            assert np.array_equal(m[k].cpu().numpy(), base[k][rows]), (k, scene, im)


def test_bop_toolkit_structures():
    fx = fixture()["big_c10"]
    c = 3
    th = fx["col_th"][c].tolist()
    n_top = int(fx["params"][0])
    scene_errs = S.scene_errs_of(fx, fx["col_err"][c].tolist())
    all_matches = []
    for scene in (1, 2):
        rows = np.nonzero(fx["m_key"][:, 0] == scene)[0]
        scene_gt, scene_valid = {}, {}
        for r in rows:
            scene_gt.setdefault(int(fx["m_key"][r, 1]), []).append({"obj_id": int(fx["m_key"][r, 2])})
            scene_valid.setdefault(int(fx["m_key"][r, 1]), []).append(bool(fx["m_valid"][r]))
        got = BE.match_poses_scene(scene, scene_gt, scene_valid, scene_errs[scene], th, n_top)
        assert len(got) == len(rows)
        for m, r in zip(got, rows):
            assert [m["scene_id"], m["im_id"], m["obj_id"], m["gt_id"]] == fx["m_key"][r].tolist() and m["valid"] == bool(fx["m_valid"][r])
            assert m["est_id"] == fx["m_est"][r, c]
            if m["est_id"] == -1:
                assert (m["score"], m["error"], m["error_norm"]) == (-1, -1, -1)
            else:
                assert m["score"] == fx["m_score"][r, c] and m["error"] == fx["m_err"][r, c].tolist() and m["error_norm"] == fx["m_norm"][r, c].tolist()
        all_matches += got
    sc = BE.calc_localization_scores(fx["scene_ids"].tolist(), fx["obj_ids"].tolist(), all_matches, n_top)
    assert sc["recall"] == fx["s_recall"][c] and sc["mean_obj_recall"] == fx["s_mobj"][c] and sc["mean_scene_recall"] == fx["s_mscene"][c]
    assert [sc["gt_count"], sc["targets_count"], sc["tp_count"]] == fx["s_counts"][c].tolist()
    assert list(sc["obj_recalls"].values()) == fx["s_obj"][:, c].tolist() and list(sc["scene_recalls"].keys()) == fx["scene_ids"].tolist()
    # match_poses: the scan-order group; the list comes in matching order
    errs = [{"est_id": 4, "score": 0.2, "errors": {0: [3.0, 3.0], 1: [1.0, 4.0]}}, {"est_id": 9, "score": 0.8, "errors": {0: [4.0, 4.5], 1: [6.0, 1.0]}}]
    got = BE.match_poses(errs, [5.0, 5.0])
    assert got == [{"est_id": 9, "gt_id": 0, "score": 0.8, "error": [4.0, 4.5], "error_norm": [0.8, 0.9]},
                   {"est_id": 4, "gt_id": 1, "score": 0.2, "error": [1.0, 4.0], "error_norm": [0.2, 0.8]}]
    assert BE.match_poses(errs, [5.0, 5.0], max_ests_count=1) == got[:1]
    assert [m["gt_id"] for m in BE.match_poses(errs, [5.0, 5.0], gt_valid_mask=[False, True])] == [1]
    back = [dict(e, errors=dict(reversed(list(e["errors"].items())))) for e in errs]          # the dicts' own order is the scan order
    assert [(m["est_id"], m["gt_id"]) for m in BE.match_poses(back, [7.0, 5.0])] == [(9, 1), (4, 0)]
    assert [(m["est_id"], m["gt_id"]) for m in BE.match_poses(errs, [7.0, 5.0])] == [(9, 0), (4, 1)]
    assert BE.match_poses(errs, [4.0, 4.5]) == [{"est_id": 4, "gt_id": 0, "score": 0.2, "error": [3.0, 3.0], "error_norm": [0.75, 3.0 / 4.5]}]


def _world_b():
    """stage B's world on the device, once: (b, evalset, estimates, MeshSet, obj_index, SymmetrySet, scene_camera)"""
    if "B" not in _RUNS:
        b = fixture()["B"]
        verts, info = S.b_models(b)
        objs = [int(o) for o in b["obj_ids"]]
        ms = metric.MeshSet.from_arrays([verts[o] for o in objs], diameters=[info[o]["diameter"] for o in objs])
        cam = {}
        for (s, i), K in zip(b["cam"].tolist(), b["K"]):
            cam.setdefault(s, {})[i] = {"cam_K": K}
        _RUNS["B"] = (b, S.evalset_of(b, poses=True), S.b_ests(b), ms, {o: k for k, o in enumerate(objs)},
                      metric.SymmetrySet.from_models_info([info[o] for o in objs]), cam)
    return _RUNS["B"]


@pytest.mark.parametrize("kind", S.B_KINDS)
def test_stage_b_errors_within_the_rows_bounds_matches_and_scores_exact(kind):
    b, es, ests, ms, obj_index, syms, cam = _world_b()
    n_top, visib_gt_min = int(b[kind + "_params"][0]), float(b[kind + "_params"][1])
    pairs = BE.expand_pairs(es, ests, n_top)
    key = np.stack([pairs.est_scene[pairs.pair_est], pairs.est_im[pairs.pair_est], pairs.est_obj[pairs.pair_est], pairs.est_id[pairs.pair_est],
                    es.gt_id[pairs.pair_gt]], 1)
    assert np.array_equal(key, b[kind + "_key"])
    errs = BE.calc_errors(pairs, ests, kind, ms, obj_index, scene_camera=cam, symmetries=syms, symmetric_obj_ids=b["sym_obj_ids"].tolist())
    got, rec = errs[:, 0].cpu().numpy(), b[kind + "_err"]
    rows, prs = S.expand(b, n_top)
    _, bound = S.host_errors(b, kind, rows, prs, want_bounds=True)
    fin = np.isfinite(rec)
    assert np.array_equal(np.isinf(got), ~fin) and not np.isnan(got).any()
    ratio = np.abs(got[fin] - rec[fin]) / bound[fin]
    print("%s: %d pairs, %d inf, worst |device - reference| / bound %.4f" % (kind, len(rec), int((~fin).sum()), float(ratio.max())))
    assert (ratio <= 1.0).all()
    div, factor = S.b_scale(b, kind, rows, prs)
    norm = factor * errs if kind == "mspd" else errs / torch.from_numpy(div).to(errs.device)[:, None]
    valid = BE.gt_valid(es, visib_gt_min)
    assert np.array_equal(valid, b[kind + "_m_valid"])
    m = BE.match(pairs, norm, b[kind + "_th"], n_top=n_top, valid=valid)
    sc = BE.localization_scores(es, m, valid, n_top)
    est = m["est_id"].cpu().numpy()
    assert np.array_equal(est, b[kind + "_m_est"])
    assert np.array_equal(bits(m["score"].cpu().numpy()), bits(b[kind + "_m_score"]))
    at = {tuple(k): p for p, k in enumerate(key.tolist())}                   # a match carries the device's own error of its pair
    mk, dev_norm, m_err = b[kind + "_m_key"], norm[:, 0].cpu().numpy(), m["error"].cpu().numpy()[:, :, 0]
    assert np.array_equal(np.stack([es.gt_scene, es.gt_im, es.gt_obj, es.gt_id], 1), mk)
    for r, c in np.argwhere(est >= 0).tolist():
        assert bits(m_err[r, c]) == bits(dev_norm[at[(mk[r, 0], mk[r, 1], mk[r, 2], est[r, c], mk[r, 3])]]), (r, c)
    assert [sc["gt_count"], sc["targets_count"]] == b[kind + "_s_counts"][0, :2].tolist() and np.array_equal(sc["tp_count"], b[kind + "_s_counts"][:, 2])
    for a, c in (("recall", "s_recall"), ("obj_recalls", "s_obj"), ("scene_recalls", "s_scene"), ("mean_obj_recall", "s_mobj"),
                 ("mean_scene_recall", "s_mscene")):
        assert np.array_equal(bits(sc[a]), bits(b[kind + "_" + c])), a


def test_evaluate_results_on_the_multi_estimate_world():
    b, es, ests, ms, obj_index, syms, cam = _world_b()
    res = BE.evaluate_results(es, ests, ms, obj_index, cam, im_width=int(b["width"]), symmetries=syms, kinds=("mssd", "mspd"))
    for kind in ("mssd", "mspd"):                                            # recorded with eval_bop19_pose.py's parameters
        assert np.array_equal(b[kind + "_th"], metric.bop_thresholds(kind)) and b[kind + "_params"].tolist() == [-1.0, -1.0]
        assert np.array_equal(bits(res["recall"][kind]), bits(b[kind + "_s_recall"])), kind
        assert res["AR_" + kind.upper()] == float(np.mean(list(b[kind + "_s_recall"])))
    assert "AR" not in res and np.array_equal(res["valid"], b["mssd_m_valid"])


def _scene(rng, n_im, size, diam):
    """a small scene: one box per image in front of a plane, estimates near the ground truth"""
    W, H = size
    K = np.array([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1.0]])
    gts, ests, depths = {}, [], {}
    for im in range(n_im):
        R = np.eye(3)
        t = np.array([[rng.uniform(-5, 5)], [rng.uniform(-5, 5)], [6.0 * diam + rng.uniform(0, 20)]])
        gts[im] = [{"obj_id": 3, "cam_R_m2c": R, "cam_t_m2c": t}]
        depths[im] = np.full((H, W), 9.0 * diam, dtype=np.float32)
        shift = np.array([[[0.5, 4.0, 15.0, 3.0 * diam][im % 4]], [0.0], [rng.uniform(-2, 2)]])
        ests.append({"scene_id": 1, "im_id": im, "obj_id": 3, "score": float(rng.random()), "R": R, "t": t + shift})
    return K, gts, ests, depths


def test_calc_errors_vsd_shortcuts_and_evaluate_results():
    rng = np.random.default_rng(5)
    verts, faces = V.meshes()["box"]
    diam = V.diameter(verts)
    ms = metric.MeshSet.from_arrays([verts], diameters=[diam], faces=[faces])
    W, H = 64, 48
    K, gts, ests, depths = _scene(rng, 6, (W, H), diam)
    targets = [{"scene_id": 1, "im_id": im, "obj_id": 3, "inst_count": 1} for im in gts]
    es = BE.EvalSet.from_dicts(targets, {1: gts}, None, [1], [3])
    cam = {1: {im: {"cam_K": K} for im in gts}}
    pairs = BE.expand_pairs(es, ests, -1)
    Re = torch.from_numpy(np.stack([e["R"] for e in ests])).to(DEV)
    te = torch.from_numpy(np.stack([e["t"] for e in ests])).to(DEV)
    Rg, tg = np.stack([gts[im][0]["cam_R_m2c"] for im in gts]), np.stack([gts[im][0]["cam_t_m2c"] for im in gts])
    stack = np.stack([depths[im] for im in gts])
    vsd = BE.calc_errors(pairs, ests, "vsd", ms, {3: 0}, scene_camera=cam, depths={1: depths})
    direct = metric.vsd_errors(Re, te, Rg, tg, K, ms, stack, image_ids=list(range(6)))["vsd"]
    assert torch.equal(vsd, direct) and tuple(vsd.shape) == (6, 10)
    # the sphere shortcut: inf exactly where |t_e - t_g| >= diameter (the 3-diameter shifts), the row's own error elsewhere
    dist = np.linalg.norm((te.cpu().numpy() - tg).reshape(-1, 3), axis=1)
    assert (dist >= diam).any() and (dist < diam).any()
    bop = metric.bop_errors(Re, te, Rg, tg, K, ms, kinds=("mssd", "mspd"))
    add = metric.pose_errors(Re, te, Rg, tg, ms, kinds=("add", "adi"))
    far = torch.from_numpy(dist >= diam).to(DEV)
    inf = torch.full((6,), float("inf"), dtype=torch.float64, device=DEV)
    assert torch.equal(BE.calc_errors(pairs, ests, "mssd", ms, {3: 0})[:, 0], torch.where(far, inf, bop["mssd"]))
    assert torch.equal(BE.calc_errors(pairs, ests, "add", ms, {3: 0})[:, 0], torch.where(far, inf, add["add"]))
    assert torch.equal(BE.calc_errors(pairs, ests, "ad", ms, {3: 0}, symmetric_obj_ids=[3])[:, 0], torch.where(far, inf, add["adi"]))
    assert torch.equal(BE.calc_errors(pairs, ests, "mspd", ms, {3: 0}, scene_camera=cam)[:, 0], bop["mspd"])
    # one estimate per target, every ground truth valid: BOP's matching is the comparison alone, and the recall is summarize_bop's
    res = BE.evaluate_results(es, ests, ms, {3: 0}, cam, im_width=W, depths={1: depths})
    errors = {"mssd": torch.where(far, inf, bop["mssd"]), "mspd": bop["mspd"], "vsd": direct}
    want = metric.summarize_bop(errors, diameters=diam, im_width=W)
    assert res["valid"].all() and res["scores"]["mssd"]["targets_count"] == 6
    assert np.array_equal(bits(res["recall"]["mssd"]), bits(want["mssd"]["recall"]))
    assert np.array_equal(bits(res["recall"]["mspd"]), bits(want["mspd"]["recall"]))
    assert np.array_equal(bits(res["recall"]["vsd"].reshape(10, 10)), bits(want["vsd"]["recall"]))
    for k in ("AR_MSSD", "AR_MSPD", "AR_VSD", "AR"):
        print("%s %.6f (summarize_bop %.6f)" % (k, res[k], want[k]))
        assert res[k] == want[k], k
    assert 0.0 < res["AR"] < 1.0
