"""Row N12 on the device: cp_mask_errors / cp_mask_overlap / cp_box_overlap against tests/golden/mask_error.npz and the stages of
tests/mask_error_stages.py (fixture and restatement: tests/test_mask_error.py).

  exact        mask_overlap on the recorded renders gives every count, both boxes and the float64 bits of all four recorded errors;
               box_overlap the recorded cou_bb of the hand-made box pairs; mask_errors' masks EQUAL render_depth(...) > 0, its counts
               and boxes the numpy counting on those masks; identical poses score 0.0;
  bitwise      two calls, a pair alone against in its batch, with / without the optional outputs, shared against repeated K, the
               kinds asked singly against together, the bop_toolkit-named twins;
  sphere       a pair the shortcut skips scores cus exactly 1.0 and is not rendered; the launch list does not depend on it; the
               shortcut never reaches cou_bb_proj;
  band         against the recorded reference values: counts inside the interval the undecided pixels (possibly but not surely
               set in the float64 oracle) allow, cus between the quotients of its ends, boxes between the inner and outer boxes,
               cou_bb_proj within what those boxes allow.  The number of cases that equal the recorded value outright is printed;
  stage B      bop_eval.calc_errors("cus") on the drawn world: the pair list is eval_calc_errors.py's, the skipped pairs are exactly 1.0,
               every other error lies within its pair's recorded interval, the errors equal metric.mask_errors on the expanded
               pairs bit for bit, and the matches and scores at 0.5 equal what eval_calc_scores.py saved exactly (the maker keeps
               every interval clear of 0.5); evaluate_results reports it as AR_CUS, outside AR, and is unchanged without it."""
import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, metric
from tests import mask_error_stages as M
from tests import vsd_stages as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_SHARED = {}
LAUNCHES = "mask_error_pose_kernel + mask_error_vertex_kernel + mask_error_tile_kernel + mask_error_finish_kernel"


def _dev(a, shape):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))).to(DEV)


def mesh_set():
    if "ms" not in _SHARED:
        g, meshes = M.fixture()
        names = [str(n) for n in g["mesh_names"]]
        _SHARED["ms"] = metric.MeshSet.from_arrays([meshes[n][0] for n in names], diameters=g["mesh_diameter"], faces=[meshes[n][1] for n in names])
    return _SHARED["ms"]


def _groups():
    """fixture cases that can share one call: the same frame"""
    g, _ = M.fixture()
    out = {}
    for c in range(len(g["names"])):
        out.setdefault((int(g["W"][c]), int(g["H"][c])), []).append(c)
    return out


def _poses(idx):
    g, _ = M.fixture()
    n = len(idx)
    return (_dev(g["R_est"][idx], (n, 3, 3)), _dev(g["t_est"][idx], (n, 3, 1)), _dev(g["R_gt"][idx], (n, 3, 3)), _dev(g["t_gt"][idx], (n, 3, 1)),
            _dev(g["K"][idx], (n, 3, 3)))


def _call(idx, size, **kw):
    g, _ = M.fixture()
    out = metric.mask_errors(*_poses(idx), mesh_set(), size, mesh_ids=g["mesh"][idx], **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _run(key):
    """group `key` through mask_errors (both kinds, no sphere check, every optional output), once, shared"""
    if key not in _SHARED:
        idx = _groups()[key]
        out = metric.mask_errors(*_poses(idx), mesh_set(), key, mesh_ids=M.fixture()[0]["mesh"][idx], return_counts=True, return_boxes=True,
                                 return_masks=True)
        assert out["cus"].dtype == torch.float64 and tuple(out["cus"].shape) == (len(idx),) and out["counts"].dtype == torch.int32
        assert tuple(out["masks"].shape) == (len(idx), 2, key[1], key[0]) and out["masks"].dtype == torch.bool
        assert tuple(out["boxes"].shape) == (len(idx), 2, 4) and tuple(out["counts"].shape) == (len(idx), 4)
        _SHARED[key] = (idx, {k: v.cpu().numpy() for k, v in out.items()})
    return _SHARED[key]


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def test_mask_overlap_on_the_recorded_renders_equals_the_reference():
    g, _ = M.fixture()
    for key, idx in _groups().items():
        idx = [c for c in idx if not g["behind"][c]]
        me = np.stack([M.layers(c)[0] for c in idx])
        mg = np.stack([M.layers(c)[1] for c in idx])
        ys, xs = np.mgrid[0:key[1], 0:key[0]]
        mixed = (1 + (xs + 2 * ys) % 255).astype(np.uint8)
        variants = [(torch.from_numpy(me), torch.from_numpy(mg)),                                                      # bool
                    (torch.from_numpy(me.astype(np.uint8) * 255), torch.from_numpy(mg.astype(np.uint8))),             # 0 / 255 against 0 / 1
                    (torch.from_numpy(me * mixed[None]), torch.from_numpy(mg.astype(np.int32) * 7))]                  # 0 / 1..255; another dtype
        first = None
        for a, b in variants:
            out = metric.mask_overlap(a.to(DEV), b.to(DEV), return_counts=True, return_boxes=True)
            out = {k: v.cpu().numpy() for k, v in out.items()}
            if first is None:
                first = out
            for k in out:
                assert np.array_equal(_bits(out[k]) if out[k].dtype == np.float64 else out[k], _bits(first[k]) if out[k].dtype == np.float64 else first[k]), k
        for j, c in enumerate(idx):
            print("case %2d %-14s counts %s boxes %s" % (c, g["names"][c], first["counts"][j].tolist(), first["boxes"][j].tolist()))
            assert np.array_equal(first["counts"][j], g["counts"][c]) and np.array_equal(first["boxes"][j], g["boxes"][c]), c
            assert np.array_equal(_bits(first["cou_mask"][j]), _bits(g["cou_mask"][c])) and np.array_equal(_bits(first["cou_mask"][j]), _bits(g["cus"][c])), c
            assert M.same(first["cou_bb"][j], g["cou_bb"][c]) and M.same(first["cou_bb"][j], g["cou_bb_proj"][c]), c
        # a pair alone, (H, W) inputs, one kind; the bop_toolkit-named twin
        one = metric.mask_overlap(torch.from_numpy(me[0]).to(DEV), torch.from_numpy(mg[0]).to(DEV), kinds="cou_mask")
        assert sorted(one) == ["cou_mask"] and _bits(one["cou_mask"].cpu().numpy())[0] == _bits(first["cou_mask"])[0]
        assert metric.cou_mask(me[-1].astype(np.uint8) * 255, mg[-1]) == first["cou_mask"][-1]
    # misaligned rows: a view that starts one byte into its storage takes the byte path and counts the same
    c = M.case("offset_box")
    me, mg = M.layers(c)[:2]
    raw = torch.zeros(me.size + 1, dtype=torch.uint8, device=DEV)
    raw[1:] = torch.from_numpy(me.reshape(-1).astype(np.uint8)).to(DEV)
    out = metric.mask_overlap(raw[1:].view(1, *me.shape), torch.from_numpy(mg[None]).to(DEV), return_counts=True)
    assert out["counts"].cpu().numpy()[0].tolist() == g["counts"][c].tolist()


def test_box_overlap_equals_the_reference():
    g, _ = M.fixture()
    got = metric.box_overlap(torch.from_numpy(g["bb_est"]).to(DEV), g["bb_gt"]).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(g["bb_cou"])), (got, g["bb_cou"])
    idx = [c for c in range(len(g["names"])) if not g["raises"][c] and not g["behind"][c]]
    got = metric.box_overlap(torch.from_numpy(g["boxes"][idx, 0]).to(DEV), torch.from_numpy(g["boxes"][idx, 1]).to(DEV)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(g["cou_bb"][idx]))
    assert metric.cou_bb(g["bb_est"][4].tolist(), g["bb_gt"][4].tolist()) == g["bb_cou"][4]


def test_masks_equal_render_depth_and_counts_equal_the_counting_on_them():
    g, _ = M.fixture()
    for key in _groups():
        idx, out = _run(key)
        R_est, t_est, R_gt, t_gt, K = _poses(idx)
        ids = np.concatenate([g["mesh"][idx], g["mesh"][idx]])
        d = metric.render_depth(torch.cat([R_est, R_gt]), torch.cat([t_est, t_gt]), torch.cat([K, K]), mesh_set(), key, mesh_ids=ids).cpu().numpy()
        n = len(idx)
        for j, c in enumerate(idx):
            me, mg = out["masks"][j]
            if g["behind"][c]:                                # ok = 0: nothing is scored, nothing is stored
                assert not out["ok"][j] and not me.any() and not mg.any() and (out["counts"][j] == 0).all() and (out["boxes"][j] == -1).all()
                assert np.isnan(out["cus"][j]) and np.isnan(out["cou_bb_proj"][j])
                continue
            assert out["ok"][j]
            assert np.array_equal(me, d[j] > 0) and np.array_equal(mg, d[n + j] > 0), c
            counts = M.counts_of(me, mg)
            be, bg = M.box_of(me), M.box_of(mg)
            assert out["counts"][j].tolist() == counts and out["boxes"][j].tolist() == [be or [-1] * 4, bg or [-1] * 4], c
            assert _bits(out["cus"][j]) == _bits(M.cou(counts)) and M.same(out["cou_bb_proj"][j], M.cou_box(be, bg)), c
            assert np.array_equal(_bits(out["cou_bb_proj"][j]), _bits(M.cou_box(be, bg))) or np.isnan(out["cou_bb_proj"][j])
    for name in ("identical_box", "identical_ico", "column_both"):
        c = M.case(name)
        idx, out = _run((int(g["W"][c]), int(g["H"][c])))
        assert out["cus"][idx.index(c)] == 0.0 and _bits(out["cus"][idx.index(c)]) == 0


def test_results_are_bitwise_the_same_however_they_are_asked():
    g, _ = M.fixture()
    key = (67, 45)
    idx, ref = _run(key)
    eq = lambda a, b: np.array_equal(_bits(a), _bits(b))      # noqa: E731
    again = _call(idx, key, return_counts=True, return_boxes=True, return_masks=True)
    for k in ref:
        assert np.array_equal(again[k], ref[k], equal_nan=ref[k].dtype == np.float64), k
    plain = _call(idx, key)                                   # without the optional outputs
    assert sorted(plain) == ["cou_bb_proj", "cus"] and eq(plain["cus"], ref["cus"]) and eq(plain["cou_bb_proj"], ref["cou_bb_proj"])
    for kind in ("cus", "cou_bb_proj"):                       # asked singly
        single = _call(idx, key, kinds=(kind,))
        assert sorted(single) == [kind] and eq(single[kind], ref[kind])
    for j in (0, 2, len(idx) - 1):                            # a pair alone, under one shared K
        c = idx[j]
        one = metric.mask_errors(_dev(g["R_est"][c], (1, 3, 3)), _dev(g["t_est"][c], (1, 3, 1)), g["R_gt"][c][None], g["t_gt"][c].reshape(1, 3, 1),
                                 g["K"][c], mesh_set(), key, mesh_ids=[int(g["mesh"][c])], return_counts=True)
        assert eq(one["cus"].cpu().numpy(), ref["cus"][j:j + 1]) and eq(one["cou_bb_proj"].cpu().numpy(), ref["cou_bb_proj"][j:j + 1])
        assert np.array_equal(one["counts"].cpu().numpy()[0], ref["counts"][j])
    same_k = [c for c in idx if g["kgroup"][c] == 0]          # shared K against the same K repeated per pair
    R_est, t_est, R_gt, t_gt, K = _poses(same_k)
    a = metric.mask_errors(R_est, t_est, R_gt, t_gt, K, mesh_set(), key, mesh_ids=g["mesh"][same_k])
    b = metric.mask_errors(R_est, t_est, R_gt, t_gt, g["K"][same_k[0]], mesh_set(), key, mesh_ids=g["mesh"][same_k])
    assert np.array_equal(g["K"][same_k], np.broadcast_to(g["K"][same_k[0]], (len(same_k), 3, 3)))
    for kind in ("cus", "cou_bb_proj"):
        assert eq(a[kind].cpu().numpy(), b[kind].cpu().numpy()) and eq(a[kind].cpu().numpy(), ref[kind][[idx.index(c) for c in same_k]])
    # the bop_toolkit-named twins: one pair, host arrays in, a float out
    c = M.case("offset_box")
    ms = mesh_set()
    args = (g["R_est"][c], g["t_est"][c], g["R_gt"][c], g["t_gt"][c], g["K"][c], ms, int(g["mesh"][c]))
    assert metric.cus(*args, size=key) == ref["cus"][idx.index(c)] and metric.cou_bb_proj(*args, size=key) == ref["cou_bb_proj"][idx.index(c)]
    with pytest.raises(ValueError, match="size"):
        metric.cus(*args)
    scored = metric.score_poses(*_poses(idx)[:4], _poses(idx)[4], ms, mesh_ids=g["mesh"][idx], kinds=("add", "cus", "cou_bb_proj"), size=key)
    assert sorted(scored) == ["add", "cou_bb_proj", "cus"] and eq(scored["cus"].cpu().numpy(), ref["cus"])


def test_sphere_shortcut_is_cus_alone_and_the_launch_list_is_fixed():
    g, _ = M.fixture()
    lib = _abi.load()
    for key in ((67, 45), (96, 80)):
        idx, ref = _run(key)
        skipped = [j for j, c in enumerate(idx) if not g["sphere"][c] and not g["behind"][c]]
        assert skipped
        lib.cp_kernel_log_begin()
        both = _call(idx, key, sphere_check=True, return_counts=True, return_masks=True)
        assert lib.cp_kernel_log().decode() == LAUNCHES
        lib.cp_kernel_log_begin()
        only = _call(idx, key, kinds=("cus",), sphere_check=True, return_counts=True, return_masks=True)
        assert lib.cp_kernel_log().decode() == LAUNCHES
        lib.cp_kernel_log_begin()
        keep = [j for j in range(len(idx)) if j not in skipped]
        _call([idx[j] for j in keep], key, sphere_check=True)                      # no pair is skipped: the same launches
        assert lib.cp_kernel_log().decode() == LAUNCHES
        for j, c in enumerate(idx):
            if g["behind"][c]:
                assert np.isnan(both["cus"][j]) and np.isnan(only["cus"][j])
            elif j in skipped:
                assert both["cus"][j] == 1.0 and only["cus"][j] == 1.0, c
                assert not only["masks"][j].any() and (only["counts"][j] == 0).all(), c          # cus alone: not rendered
                assert np.array_equal(both["masks"][j], ref["masks"][j]) and np.array_equal(both["counts"][j], ref["counts"][j])
            else:
                assert _bits(both["cus"][j]) == _bits(ref["cus"][j]) and _bits(only["cus"][j]) == _bits(ref["cus"][j]), c
                assert np.array_equal(only["masks"][j], ref["masks"][j])
            assert M.same(both["cou_bb_proj"][j], ref["cou_bb_proj"][j]), c           # never touched by the shortcut
    idx, ref = _run((96, 80))
    j = idx.index(M.case("diagonal"))
    assert ref["cou_bb_proj"][j] < 1.0 and ref["cus"][j] == 1.0


def test_device_lies_within_the_band_of_the_recorded_reference_values():
    g, _ = M.fixture()
    exact, total = 0, 0
    for key in _groups():
        idx, out = _run(key)
        for j, c in enumerate(idx):
            if g["behind"][c]:
                continue
            total += 1
            counts, boxes, cus, bbp = out["counts"][j].tolist(), out["boxes"][j].tolist(), float(out["cus"][j]), float(out["cou_bb_proj"][j])
            same = (counts == g["counts"][c].tolist() and boxes == g["boxes"][c].tolist() and M.same(cus, g["cus"][c])
                    and M.same(bbp, g["cou_bb_proj"][c]))
            exact += int(same)
            low, high = M.count_interval(c)
            print("case %2d %-14s counts %s in [%s, %s] cus %.6f (recorded %.6f) cou_bb_proj %.6f (recorded %.6f) %s"
                  % (c, g["names"][c], counts, low, high, cus, g["cus"][c], bbp, g["cou_bb_proj"][c], "exact" if same else "within band"))
            assert all(lo <= v <= hi for lo, v, hi in zip(low, counts, high)), c
            lo, hi = M.cus_interval(c)
            assert lo <= cus <= hi, c
            for side in (0, 1):
                assert M.box_within(boxes[side], *M.box_interval(c, side)), (c, side)
            lo, hi = M.cou_bb_proj_interval(c)
            if g["raises"][c]:
                assert np.isnan(bbp), c                           # the reference raises: NaN here
            elif not np.isnan(lo):
                assert lo <= bbp <= hi, c
    print("device equals the recorded reference value outright in %d of %d cases" % (exact, total))


def _world_b():
    """stage B's world on the device, once: (b, evalset, estimates, MeshSet with faces, obj_index, SymmetrySet, scene_camera, size)"""
    if "B" not in _SHARED:
        from tests import bop_eval_stages as BS
        b = M.world_b()
        _, info = BS.b_models(b)                              # (checks the meshes' CRC)
        meshes = S.meshes()
        objs = [int(o) for o in b["obj_ids"]]
        names = [str(n) for n in b["mesh"]]
        ms = metric.MeshSet.from_arrays([meshes[n][0] for n in names], diameters=[info[o]["diameter"] for o in objs], faces=[meshes[n][1] for n in names])
        cam = {}
        for (s, i), K in zip(b["cam"].tolist(), b["K"]):
            cam.setdefault(s, {})[i] = {"cam_K": K}
        _SHARED["B"] = (b, BS.evalset_of(b, poses=True), BS.b_ests(b), ms, {o: k for k, o in enumerate(objs)},
                        metric.SymmetrySet.from_models_info([info[o] for o in objs]), cam, (int(b["width"]), int(b["height"])))
    return _SHARED["B"]


def test_stage_b_calc_errors_within_the_intervals_matches_and_scores_exact():
    from checkerpose_amd import bop_eval as BE
    from tests import bop_eval_stages as BS
    b, es, ests, ms, obj_index, _, cam, size = _world_b()
    n_top, visib_gt_min = int(b["cus_params"][0]), float(b["cus_params"][1])
    pairs = BE.expand_pairs(es, ests, n_top)
    key = np.stack([pairs.est_scene[pairs.pair_est], pairs.est_im[pairs.pair_est], pairs.est_obj[pairs.pair_est], pairs.est_id[pairs.pair_est],
                    es.gt_id[pairs.pair_gt]], 1)
    assert np.array_equal(key, b["cus_key"])
    lib = _abi.load()
    lib.cp_kernel_log_begin()
    errs = BE.calc_errors(pairs, ests, "cus", ms, obj_index, scene_camera=cam, size=size)          # sphere_check defaults to True
    assert lib.cp_kernel_log().decode() == LAUNCHES
    assert tuple(errs.shape) == (len(key), 1) and errs.dtype == torch.float64
    got, rec, lo, hi, skip = errs[:, 0].cpu().numpy(), b["cus_err"], b["cus_lo"], b["cus_hi"], b["cus_skip"]
    assert not np.isnan(got).any() and (got[skip] == 1.0).all() and skip.any() and (~skip).any()
    print("stage B: %d pairs, %d skipped by the sphere check, %d of the %d rendered ones equal the recorded error outright"
          % (len(rec), int(skip.sum()), int((got[~skip] == rec[~skip]).sum()), int((~skip).sum())))
    assert ((lo <= got) & (got <= hi)).all(), np.nonzero(~((lo <= got) & (got <= hi)))[0]
    # the same pairs through metric.mask_errors, poses and K gathered pair by pair from the world's own tables
    rows, prs = BS.expand(b, n_top)
    args = list(BS._b_pair_args(b, rows, prs))
    f = lambda k, shape: _dev(np.stack([a[k] for a in args]), (len(args),) + shape)     # noqa: E731
    direct = metric.mask_errors(f(0, (3, 3)), f(1, (3, 1)), f(2, (3, 3)), f(3, (3, 1)), f(4, (3, 3)), ms, size,
                                mesh_ids=[obj_index[a[5]] for a in args], kinds=("cus",), sphere_check=True)["cus"]
    assert torch.equal(errs[:, 0], direct)
    unchecked = BE.calc_errors(pairs, ests, "cus", ms, obj_index, scene_camera=cam, size=size, sphere_check=False)[:, 0].cpu().numpy()
    assert np.array_equal(_bits(unchecked[~skip]), _bits(got[~skip]))              # the check changes nothing but the skipped pairs
    with pytest.raises(ValueError, match="size"):
        BE.calc_errors(pairs, ests, "cus", ms, obj_index, scene_camera=cam)
    # matching and scores at 0.5: exactly what eval_calc_scores.py saved
    valid = BE.gt_valid(es, visib_gt_min)
    assert np.array_equal(valid, b["cus_m_valid"])
    m = BE.match(pairs, errs, b["cus_th"], n_top=n_top, valid=valid)
    sc = BE.localization_scores(es, m, valid, n_top)
    est = m["est_id"].cpu().numpy()
    assert np.array_equal(est, b["cus_m_est"])
    assert np.array_equal(_bits(m["score"].cpu().numpy()), _bits(b["cus_m_score"]))
    assert np.array_equal(np.stack([es.gt_scene, es.gt_im, es.gt_obj, es.gt_id], 1), b["cus_m_key"])
    assert [sc["gt_count"], sc["targets_count"]] == b["cus_s_counts"][0, :2].tolist() and np.array_equal(sc["tp_count"], b["cus_s_counts"][:, 2])
    for a, c in (("recall", "s_recall"), ("obj_recalls", "s_obj"), ("scene_recalls", "s_scene"), ("mean_obj_recall", "s_mobj"),
                 ("mean_scene_recall", "s_mscene")):
        assert np.array_equal(_bits(sc[a]), _bits(b["cus_" + c])), a
    r = metric.bop_recall(torch.tensor([0.2, 0.5, float("nan"), 1.0], device=DEV), "cus")
    assert r["recall"].tolist() == [0.25]


def test_evaluate_results_reports_cus_outside_ar_and_is_unchanged_without_it():
    from checkerpose_amd import bop_eval as BE
    b, es, ests, ms, obj_index, syms, cam, size = _world_b()
    before = BE.evaluate_results(es, ests, ms, obj_index, cam, im_width=int(b["width"]), symmetries=syms, kinds=("mssd", "mspd"))
    assert sorted(before) == ["AR_MSPD", "AR_MSSD", "recall", "scores", "valid"] and sorted(before["recall"]) == ["mspd", "mssd"]
    res = BE.evaluate_results(es, ests, ms, obj_index, cam, im_width=int(b["width"]), symmetries=syms, kinds=("mssd", "mspd", "cus"), size=size)
    assert sorted(res) == ["AR_CUS", "AR_MSPD", "AR_MSSD", "recall", "scores", "valid"] and "AR" not in res
    assert np.array_equal(_bits(res["recall"]["cus"]), _bits(b["cus_s_recall"])) and res["AR_CUS"] == float(b["cus_s_recall"][0])
    for kind in ("mssd", "mspd"):                             # the other kinds: the same bits with and without "cus"
        assert np.array_equal(_bits(res["recall"][kind]), _bits(before["recall"][kind])) and res["AR_" + kind.upper()] == before["AR_" + kind.upper()]
    assert np.array_equal(res["valid"], before["valid"])
