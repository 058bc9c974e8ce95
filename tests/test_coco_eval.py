"""CPU: row N15 (BOP'22 COCO detection / segmentation scores).  The ground-truth side of tests/coco_stages.py against the values
recorded from bop_toolkit_lib/pycoco_utils.py (tests/golden/coco_eval.npz); the two restatements of the score side against each other
and against closed forms; one named case per rule that a slip would break; the host half of checkerpose_amd/coco_eval.py (index plan,
scene merge, RLE decoding, result checks) and the argument checks of the cp_coco_* entry points."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import coco_stages as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coco_eval.npz")
FRAMES = ((31, 33), (50, 70), (120, 160))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def fixture_masks(gold, H, W):
    tag = "%dx%d" % (H, W)
    bits = np.unpackbits(gold["masks_" + tag], axis=1)[:, :H * W].reshape(-1, H, W)
    return bits.astype(np.uint8) * gold["values_" + tag][:, None, None].astype(np.uint8), tag


# ---- the pinned side --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", FRAMES)
def test_restatement_reproduces_recorded_rle_boxes_and_annotations(gold, H, W):
    masks, tag = fixture_masks(gold, H, W)
    counts, offsets = gold["rle_counts_" + tag], gold["rle_offsets_" + tag]
    infos = json.loads(str(gold["infos_" + tag]))
    assert len(infos) == len(masks) == 14 and infos[0] is None                  # the empty mask: create_annotation_info gives None
    for n, m in enumerate(masks):
        rle = S.binary_mask_to_rle(m)
        assert rle["counts"] == counts[offsets[n]:offsets[n + 1]].tolist() and rle["size"] == [H, W], n
        back = np.unpackbits(gold["roundtrip_" + tag][n])[:H * W].reshape(H, W).astype(bool)
        assert np.array_equal(S.rle_to_binary_mask(rle), back) and np.array_equal(back, m != 0), n
        if m.any():
            assert S.bbox_from_binary_mask(m) == gold["bbox_" + tag][n].tolist(), n
        box = gold["bbox_" + tag][n].tolist()
        assert S.create_annotation_info(n + 1, 100 + n, 5, m, box, ignore=bool(n % 3 == 0)) == infos[n], n
    assert counts[offsets[1]:offsets[2]].tolist() == [0, H * W]                # the full mask: a leading 0
    assert counts[offsets[4]:offsets[5]].tolist() == [3 * H + H - 2, 4, H * W - 4 * H - 2]      # one run across the column boundary


def test_host_rle_decoder_and_scene_merge_reproduce_the_recorded_values(gold):
    from checkerpose_amd import coco_eval as CE
    for H, W in FRAMES:
        masks, tag = fixture_masks(gold, H, W)
        rles = [S.binary_mask_to_rle(m) for m in masks]
        assert np.array_equal(CE.rle_decode(rles), (masks != 0).astype(np.uint8))
    spec = json.loads(str(gold["merge_scenes"]))
    merged, offs = S.merge_scenes(spec["scenes"])
    assert [im["id"] for im in merged["images"]] == gold["merge_image_ids"].tolist()
    assert [[a["id"], a["image_id"]] for a in merged["annotations"]] == gold["merge_ann_ids"].tolist()
    assert offs == gold["merge_offsets"].tolist() == [0, 8, 18]
    # the module's twin of the script's loop: every image is a target, every result carries a box
    anns = {10 + i: s for i, s in enumerate(spec["scenes"])}
    targets = [{"scene_id": 10 + i, "im_id": im["id"]} for i, s in enumerate(spec["scenes"]) for im in s["images"]]
    results = [dict(r, scene_id=10 + i, bbox=[0, 0, 1, 1], segmentation={}) for i, rs in enumerate(spec["results"]) for r in rs]
    before = json.dumps([anns, results], sort_keys=True)
    ann, res = CE.merge_scenes(anns, results, targets, "bbox")
    assert json.dumps([anns, results], sort_keys=True) == before                # the inputs are left as they were
    assert [im["id"] for im in ann["images"]] == gold["merge_image_ids"].tolist()
    assert [[a["id"], a["image_id"]] for a in ann["annotations"]] == gold["merge_ann_ids"].tolist()
    assert [r["image_id"] for r in res] == gold["merge_result_image_ids"].tolist()
    # images, annotations and results outside the target list are dropped BEFORE the offsets are made
    ann2, res2 = CE.merge_scenes(anns, results, [t for t in targets if not (t["scene_id"] == 10 and t["im_id"] == 7)], "bbox")
    assert [im["id"] for im in ann2["images"]] == [0, 3, 4 + 1, 4 + 2, 4 + 9, 14 + 0, 14 + 4]
    assert [r["image_id"] for r in res2] == [3, 4 + 9, 4 + 1, 14 + 4]
    assert CE.merge_scenes(anns, results, targets, "segm")[1] == []            # every segmentation is empty


# ---- the two restatements -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drawn():
    return S.draw_world(31, 33, seed=3)


@pytest.mark.parametrize("ann_type", ["segm", "bbox"])
def test_the_two_restatements_agree_bit_for_bit_on_the_drawn_world(drawn, ann_type):
    a, b = S.evaluate(drawn, ann_type), S.evaluate_brute(drawn, ann_type)
    assert a["precision"].tobytes() == b["precision"].tobytes() and a["recall"].tobytes() == b["recall"].tobytes()
    assert a["stats"] == b["stats"]
    sizes = {(len(g["scores"]), g["ious"].shape[1]) for g in a["groups"].values()}
    assert {d for d, _ in sizes} == {0, 1, 7, 100} and {g for _, g in sizes} == {0, 1, 7}      # 103 detections were cut to 100
    assert (a["precision"] > 0).any() and (a["precision"][:, :, 3] == -1).all() and (a["precision"][:, :, 4] == -1).all()
    assert 0 < a["stats"]["AP"] < 1 and a["stats"]["AR1"] < a["stats"]["AR100"]


def box_world(gts, dts, image_ids=None, category_ids=None):
    """gts: (image, category, [x, y, w, h], ignore[, area]); dts: (image, category, [x, y, w, h], score)"""
    G = [{"image_id": g[0], "category_id": g[1], "bbox": list(g[2]), "ignore": bool(g[3]), "iscrowd": 0,
          "area": g[4] if len(g) > 4 else g[2][2] * g[2][3]} for g in gts]
    D = [{"image_id": d[0], "category_id": d[1], "bbox": list(d[2]), "score": d[3]} for d in dts]
    return {"image_ids": image_ids or sorted({x["image_id"] for x in G + D}),
            "category_ids": category_ids or sorted({x["category_id"] for x in G + D}), "size": None, "gts": G, "dts": D}


def both(world, **kw):
    a, b = S.evaluate(world, "bbox", **kw), S.evaluate_brute(world, "bbox", **kw)
    assert a["precision"].tobytes() == b["precision"].tobytes() and a["recall"].tobytes() == b["recall"].tobytes()
    return a


A, B_, FAR = [0, 0, 10, 10], [20, 0, 10, 10], [50, 50, 10, 10]


def test_closed_forms():
    # TP, FP, TP on two ground truths: rc = .5 .5 1, pr = 1 2/3 2/3 from the right: 51 thresholds at 1, 50 at 2/3 -- at every IoU threshold
    r = both(box_world([(1, 1, A, 0), (1, 1, B_, 0)], [(1, 1, A, .9), (1, 1, FAR, .8), (1, 1, B_, .7)]))
    want = (51 * 1 + 50 * 2 / 3) / 101
    for k in ("AP", "AP50", "AP75", "AP_small"):
        assert abs(r["stats"][k] - want) <= 1e-12, k
    assert np.abs(r["precision"][:, :, 0, 0, 2].mean(1) - want).max() <= 1e-12
    assert r["stats"]["AR1"] == 0.5 and r["stats"]["AR10"] == 1.0 and r["stats"]["AR100"] == 1.0 and r["stats"]["AR_small"] == 1.0
    assert r["stats"]["AP_medium"] == -1.0 and r["stats"]["AP_large"] == -1.0 and r["stats"]["AR_large"] == -1.0
    assert r["precision"][0, 0, 0, 0, 2] == 1 / (1 + EPS) and r["precision"][0, 100, 0, 0, 2] == 2 / (3 + EPS)
    # all correct
    r = both(box_world([(1, 1, A, 0), (2, 1, B_, 0)], [(1, 1, A, .9), (2, 1, B_, .7)]))
    assert abs(r["stats"]["AP"] - 1) <= 1e-12 and r["stats"]["AR100"] == 1.0 and r["stats"]["AR1"] == 1.0
    # no detections: AP 0, AR 0
    r = both(box_world([(1, 1, A, 0)], []))
    assert r["stats"]["AP"] == 0.0 and r["stats"]["AR100"] == 0.0 and r["stats"]["AR1"] == 0.0 and r["stats"]["AP_large"] == -1.0
    # no unignored ground truth: -1
    r = both(box_world([(1, 1, A, 1)], [(1, 1, A, .9)]))
    assert all(v == -1.0 for v in r["stats"].values()) and (r["precision"] == -1).all() and (r["recall"] == -1).all()


# ---- one named case per rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num,den", [(1, 2), (3, 5), (3, 4), (9, 10)])
def test_iou_exactly_at_a_threshold_matches_when_it_is_not_below(num, den):
    """`iou < threshold` skips: an IoU equal to the threshold's float64 matches (with `<=` it would not)"""
    thrs = S.iou_thrs()
    det = [0, 0, 100, 100 * num // den] if (100 * num) % den == 0 else None
    r = both(box_world([(1, 1, [0, 0, 100, 100], 0)], [(1, 1, det, .9)]))
    iou = S.box_iou(det, [0, 0, 100, 100])
    assert iou == num / den
    hit = np.array([not (iou < t) for t in thrs])
    t_eq = int(round((num / den - .5) / .05))
    if thrs[t_eq] == iou:                                                    # .5 and .75 are hit exactly by np.linspace(.5, .95, 10)
        assert hit[t_eq]
    assert (num, den) not in ((1, 2), (3, 4)) or thrs[t_eq] == iou
    assert r["recall"][:, 0, 0, 2].tolist() == hit.astype(float).tolist()
    assert r["groups"][(1, 1)]["dtm"][0, :, 0].tolist() == hit.astype(int).tolist()


def test_the_later_ground_truth_wins_an_iou_tie():
    g0, g1 = [0, 0, 10, 8], [0, 2, 10, 8]
    r = both(box_world([(1, 1, g0, 0), (1, 1, g1, 0)], [(1, 1, [0, 0, 10, 10], .9), (1, 1, g1, .8)]))
    assert S.box_iou([0, 0, 10, 10], g0) == S.box_iou([0, 0, 10, 10], g1) == 0.8 and S.box_iou(g1, g0) == 0.6
    dtm = r["groups"][(1, 1)]["dtm"][0]
    assert dtm[:6, 0].tolist() == [2] * 6 and dtm[7:, 0].tolist() == [0] * 3          # the first detection takes g1, the LATER one
    assert dtm[5, 1] == 0 and dtm[0, 1] == 1                                     # so the second is left with g0 (IoU .6)
    assert abs(r["stats"]["AP75"] - 51 / 101) <= 1e-12                           # (first-wins would give both a match: AP75 = 1)


def test_the_walk_stops_at_the_first_ignored_ground_truth_once_an_unignored_one_matched():
    world = box_world([(1, 1, [0, 0, 100, 92], 1), (1, 1, [0, 0, 100, 72], 0)], [(1, 1, [0, 0, 100, 100], .9)])
    r = both(world)
    assert r["groups"][(1, 1)]["ious"].tolist() == [[0.92, 0.72]]
    # thresholds up to .70: the unignored one (IoU .72) is walked first and kept, although the ignored one overlaps more
    assert r["groups"][(1, 1)]["dtm"][0, :, 0].tolist() == [2] * 5 + [1] * 4 + [0]
    assert r["groups"][(1, 1)]["dtIg"][0, :, 0].tolist() == [False] * 5 + [True] * 4 + [False]
    assert r["recall"][:, 0, 0, 2].tolist() == [1.0] * 5 + [0.0] * 5 and r["stats"]["AR100"] == 0.5
    assert abs(r["stats"]["AP50"] - 1) <= 1e-12


def test_an_ignored_ground_truth_absorbs_its_detection():
    r = both(box_world([(1, 1, A, 1), (1, 1, B_, 0)], [(1, 1, A, .95), (1, 1, B_, .9)]))
    assert r["groups"][(1, 1)]["dtIg"][0, :, 0].all() and not r["groups"][(1, 1)]["dtIg"][0, :, 1].any()
    assert abs(r["stats"]["AP"] - 1) <= 1e-12                                    # (counted as a false positive it would give .5)


@pytest.mark.parametrize("side,stats", [(32, ("small", "medium")), (96, ("medium", "large"))])
def test_areas_exactly_on_a_range_border_belong_to_both_ranges(side, stats):
    box = [0, 0, side, side]
    r = both(box_world([(1, 1, box, 0)], [(1, 1, box, .9)]))
    for name in ("small", "medium", "large"):
        want = 1.0 if name in stats else -1.0
        assert abs(r["stats"]["AP_" + name] - want) <= 1e-12 and r["stats"]["AR_" + name] == want, name
    # a detection of exactly that area without a ground truth in range is not ignored either
    r = both(box_world([(1, 1, [200, 200, 40, 40], 0)], [(1, 1, box, .9), (1, 1, [200, 200, 40, 40], .8)]))
    assert not r["groups"][(1, 1)]["dtIg"][1 if side == 32 else 2, :, 0].any()


def test_score_ties_across_images_keep_the_image_order():
    r = both(box_world([(1, 1, A, 0), (2, 1, A, 0)], [(2, 1, A, .5), (1, 1, FAR, .5)]))
    assert abs(r["stats"]["AP"] - 51 * (1 / (2 + EPS)) / 101) <= 1e-12           # FP (image 1) first, then TP; the reverse gives 51 / 101


def test_103_detections_are_cut_to_100():
    noise = [(1, 1, [100 + 20 * i, 0, 10, 10], 1.0 - i / 1000.0) for i in range(102)]
    kept = both(box_world([(1, 1, A, 0)], noise[:50] + [(1, 1, A, 1.0 - 98.5 / 1000.0)] + noise[50:]))      # rank 99: the last one kept
    assert kept["stats"]["AR100"] == 1.0 and abs(kept["stats"]["AP"] - 1 / (100 + EPS)) <= 1e-12
    cut = both(box_world([(1, 1, A, 0)], noise[:50] + [(1, 1, A, 1.0 - 99.5 / 1000.0)] + noise[50:]))       # rank 100: cut
    assert cut["stats"]["AR100"] == 0.0 and cut["stats"]["AP"] == 0.0
    assert len(cut["groups"][(1, 1)]["scores"]) == 100


def test_maxdet_1_takes_the_first_detection_of_every_image_from_the_100_greedy():
    r = both(box_world([(1, 1, A, 0), (2, 1, A, 0)], [(1, 1, A, .3), (2, 1, FAR, .9), (2, 1, A, .8)]))
    assert r["stats"]["AR1"] == 0.5 and r["stats"]["AR10"] == 1.0               # per image, not the best score overall (that gives 0)


def test_a_category_with_detections_and_no_ground_truth_scores_minus_one():
    r = both(box_world([(1, 1, A, 0)], [(1, 1, A, .9), (1, 2, A, .9)]))
    assert (r["precision"][:, :, 1] == -1).all() and (r["recall"][:, 1] == -1).all()
    assert abs(r["stats"]["AP"] - 1) <= 1e-12 and r["stats"]["AR100"] == 1.0    # (as zeros it would halve both)


def test_an_image_with_neither_changes_nothing():
    gts, dts = [(1, 1, A, 0), (2, 1, B_, 0)], [(1, 1, A, .9), (2, 1, FAR, .95)]
    with_empty, without = both(box_world(gts, dts, image_ids=[1, 2, 99])), both(box_world(gts, dts))
    assert with_empty["precision"].tobytes() == without["precision"].tobytes() and with_empty["stats"] == without["stats"]
    with pytest.raises(ValueError, match="do not correspond"):
        S.evaluate(box_world(gts, dts + [(7, 1, A, .5)], image_ids=[1, 2]), "bbox")


def test_the_stock_ignore_switch():
    world = box_world([(1, 1, A, 1)], [(1, 1, A, .9)])
    assert both(world)["stats"]["AP"] == -1.0                                    # the fork: the annotation's flag counts
    assert abs(both(world, stock_ignore=True)["stats"]["AP"] - 1) <= 1e-12       # stock pycocotools: iscrowd (0) overwrites it


# ---- the module's host half -------------------------------------------------------------------------------------------------------------
def test_index_plan_agrees_with_the_restatement(drawn):
    from checkerpose_amd import coco_eval as CE
    w = drawn
    ref = S.evaluate(w, "bbox")
    plan = CE.make_plan(np.array(sorted(w["image_ids"])), np.array(sorted(w["category_ids"])), [g["image_id"] for g in w["gts"]],
                        [g["category_id"] for g in w["gts"]], [d["image_id"] for d in w["dts"]], [d["category_id"] for d in w["dts"]],
                        [d["score"] for d in w["dts"]])
    imgs, cats = sorted(w["image_ids"]), sorted(w["category_ids"])
    keys = [(imgs[i], cats[c]) for c, i in zip(plan["group_cat"], plan["group_img"])]
    assert keys == sorted(ref["groups"], key=lambda k: (k[1], k[0])) and plan["n_groups"] == len(keys)
    for n, key in enumerate(keys):
        d0, d1, g0, g1 = plan["det_off"][n], plan["det_off"][n + 1], plan["gt_off"][n], plan["gt_off"][n + 1]
        assert [w["dts"][i]["score"] for i in plan["det_sel"][d0:d1]] == ref["groups"][key]["scores"].tolist()
        assert (d1 - d0, g1 - g0) == ref["groups"][key]["ious"].shape and d1 - d0 <= 100
        assert [id(w["gts"][i]) for i in plan["gt_sel"][g0:g1]] == [id(g) for g in w["gts"] if (g["image_id"], g["category_id"]) == key]
        assert plan["iou_off"][n + 1] - plan["iou_off"][n] == (d1 - d0) * (g1 - g0)
        pairs = plan["pairs"][plan["iou_off"][n]:plan["iou_off"][n + 1]]
        assert pairs.tolist() == [[d, g] for d in range(d0, d1) for g in range(g0, g1)]
    assert plan["cat_det_off"][-1] == len(plan["det_sel"]) and plan["cat_gt_off"][-1] == len(plan["gt_sel"])
    score = np.array([w["dts"][i]["score"] for i in plan["det_sel"]])
    for k in range(len(cats)):
        c0, c1 = plan["cat_det_off"][k], plan["cat_det_off"][k + 1]
        seg = plan["order"][c0:c1]
        assert sorted(seg.tolist()) == list(range(c0, c1))
        assert seg.tolist() == (c0 + np.argsort(-score[c0:c1], kind="stable")).tolist()


def test_summarize_is_the_restatements(drawn):
    from checkerpose_amd import coco_eval as CE
    ref = S.evaluate(drawn, "segm")
    assert CE.summarize(ref["precision"], ref["recall"]) == ref["stats"]
    assert CE.iou_thrs().tobytes() == S.iou_thrs().tobytes() and CE.rec_thrs().tobytes() == S.rec_thrs().tobytes()
    assert np.asarray(CE.AREA_RNG).tolist() == np.asarray(S.AREA_RNG, float).tolist() and list(CE.MAX_DETS) == S.MAX_DETS


def test_result_checks_times_and_no_cpu_fallback(tmp_path):
    import checkerpose_amd
    from checkerpose_amd import coco_eval as CE
    assert checkerpose_amd.eval_bop22_coco is CE.eval_bop22_coco and checkerpose_amd.CocoSet is CE.CocoSet
    good = {"scene_id": 1, "image_id": 2, "category_id": 3, "score": 0.5, "bbox": [0, 0, 1, 1], "segmentation": {"counts": [4], "size": [2, 2]},
            "time": 0.25}
    assert CE.check_coco_results([good]) == (True, "OK")
    for bad in (dict(good, score=1), dict(good, scene_id="1"), dict(good, segmentation=[1, 2]), dict(good, segmentation={"size": [2, 2]}),
                dict(good, time="x"), {k: v for k, v in good.items() if k != "category_id"}):
        assert CE.check_coco_results([bad])[0] is False, bad
    assert CE.check_coco_results([dict(good, segmentation=[1, 2])], ann_type="bbox")[0] is True
    res = [{"scene_id": 1, "im_id": 2, "obj_id": 3, "score": 0.5, "bbox": np.array([1, 2, 3, 4]), "run_time": 0.25},
           {"scene_id": 1, "im_id": 2, "obj_id": 4, "score": 0.25, "segmentation": {"counts": [4], "size": [2, 2]}}]
    path = str(tmp_path / "r.json")
    CE.save_coco_results(path, res)
    assert json.load(open(path)) == [
        {"scene_id": 1, "image_id": 2, "category_id": 3, "score": 0.5, "bbox": [1, 2, 3, 4], "segmentation": {}, "time": 0.25},
        {"scene_id": 1, "image_id": 2, "category_id": 4, "score": 0.25, "bbox": [], "segmentation": {"counts": [4], "size": [2, 2]}, "time": -1}]
    assert CE.check_coco_results(path, ann_type="bbox") == (True, "OK")
    assert CE.check_coco_results(path)[0] is False                              # the empty segmentation of the first result: as inout.py
    assert CE.check_coco_results(str(tmp_path / "missing.json"))[0] is False
    with pytest.raises(ValueError):
        CE.save_coco_results(path, res, version="bop19")
    t = lambda s, i, v: {"scene_id": s, "image_id": i, "time": v}      # noqa: E731
    assert CE.average_time_per_image([t(1, 1, .5), t(1, 1, .5004), t(1, 2, 1.0), t(2, 1, 3.0)]) == 1.5
    assert CE.average_time_per_image([t(1, 1, .5), t(1, 2, -1)]) == -1.0
    with pytest.raises(ValueError, match="different run times"):
        CE.average_time_per_image([t(1, 1, .5), t(1, 1, .502)])
    with pytest.raises(ValueError, match="scene_coco_anns_modal"):      # 'bbox' + 'modal' is scored against the modal annotations
        CE.eval_bop22_coco({}, [], [], "bbox", "modal")
    with pytest.raises(ValueError, match="iscrowd"):
        CE.CocoSet([1], [1], [1], [1], [4.0], iscrowd=[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CE.annotate_masks(np.ones((1, 4, 4), np.uint8), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CE.box_ious(np.zeros((1, 4)), np.zeros((1, 4)), [[0, 0]])
    with pytest.raises(ValueError, match="compressed"):
        CE.rle_decode([{"counts": "abc", "size": [2, 2]}])


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    p = C.c_void_p(4096)                                    # fake, aligned; never dereferenced: every call returns before a launch
    lib.cp_kernel_log_begin()

    def pack(m=p, N=2, H=31, W=33, bits=p, area=p, box=p):
        return lib.cp_coco_pack(None, m, N, H, W, bits, area, box)
    for name in ("m", "bits", "area", "box"):
        assert pack(**{name: None}) == -1, name
    assert pack(N=0) == -1 and pack(H=0) == -1 and pack(W=0) == -1 and pack(W=-3) == -1
    assert pack(bits=C.c_void_p(4098)) == -3 and pack(H=1 << 16, W=1 << 15) == -4 and pack(N=1 << 24) == -4

    def cnt(bits=p, N=2, H=31, W=33, n=p):
        return lib.cp_coco_rle_count(None, bits, N, H, W, n)

    def wr(bits=p, N=2, H=31, W=33, off=p, counts=p, total=10):
        return lib.cp_coco_rle_write(None, bits, N, H, W, off, counts, total)
    assert cnt(bits=None) == -1 and cnt(n=None) == -1 and cnt(N=0) == -1 and cnt(H=0) == -1 and cnt(W=0) == -1 and cnt(n=C.c_void_p(4098)) == -3
    assert wr(bits=None) == -1 and wr(off=None) == -1 and wr(counts=None) == -1 and wr(total=0) == -1 and wr(H=0) == -1 and wr(W=0) == -1
    assert wr(off=C.c_void_p(4100)) == -3 and wr(H=1 << 16, W=1 << 15) == -4

    def mi(db=p, da=p, dx=p, ND=2, gb=p, ga=p, gx=p, NG=2, H=31, W=33, pairs=p, P=3, out=p):
        return lib.cp_coco_mask_iou(None, db, da, dx, ND, gb, ga, gx, NG, H, W, pairs, P, out)
    for name in ("db", "da", "dx", "gb", "ga", "gx", "pairs", "out"):
        assert mi(**{name: None}) == -1, name
    assert mi(ND=0) == -1 and mi(NG=0) == -1 and mi(H=0) == -1 and mi(W=0) == -1 and mi(P=0) == -1 and mi(out=C.c_void_p(4100)) == -3

    def bi(d=p, ND=2, g=p, NG=2, pairs=p, P=3, out=p):
        return lib.cp_coco_box_iou(None, d, ND, g, NG, pairs, P, out)
    assert bi(d=None) == -1 and bi(g=None) == -1 and bi(pairs=None) == -1 and bi(out=None) == -1 and bi(P=0) == -1 and bi(ND=0) == -1
    assert bi(d=C.c_void_p(4100)) == -3

    def offs(*rows):
        a = np.ascontiguousarray(np.concatenate(rows), dtype=np.int32)
        return a, a.ctypes.data_as(C.c_void_p)

    def match(det=(0, 2, 5), gt=(0, 1, 3), iou=(0, 2, 8), ND=5, NGT=3, P=8, dev=p, ngrp=2, **kw):
        keep, host = offs(det, gt, iou)
        a = dict(ious=p, da=p, ga=p, gi=p, thr=p, rng=p, dm=p, di=p, go=p, scr=p, host=host)
        a.update(kw)
        return lib.cp_coco_match(None, a["ious"], a["host"], dev, ngrp, ND, NGT, P, a["da"], a["ga"], a["gi"], a["thr"], a["rng"], a["dm"],
                                 a["di"], a["go"], a["scr"])
    assert match(ND=4) == -1 and match(NGT=4) == -1 and match(P=9) == -1          # the offsets do not end at the totals
    for name in ("ious", "da", "ga", "gi", "thr", "rng", "dm", "di", "go", "scr", "host"):
        assert match(**{name: None}) == -1, name
    assert match(dev=None) == -1 and match(ngrp=0) == -1
    assert match(det=(0, 3, 2), iou=(0, 3, 1), ND=2, P=1) == -1                   # offsets that do not ascend
    assert match(det=(1, 2, 5)) == -1 and match(gt=(0, 2, 3)) == -1               # not from 0; an IoU stretch that is not D x G
    assert match(det=(0, 101, 102), gt=(0, 1, 2), iou=(0, 101, 102), ND=102, NGT=2, P=102) == -1      # more than 100 kept detections
    assert match(ious=C.c_void_p(4100)) == -3 and match(dm=C.c_void_p(4098)) == -3
    assert lib.cp_coco_match_scratch_bytes(0) == 0 and lib.cp_coco_match_scratch_bytes(7) == 280

    def acc(det=(0, 2, 5), gt=(0, 3, 3), ND=5, NGT=3, K=2, dev=p, mds=(1, 10, 100), **kw):
        keep, host = offs(det, gt)
        keep2, mdp = offs(mds)
        a = dict(dm=p, di=p, gi=p, rank=p, order=p, rec=p, pr=p, rc=p, host=host, md=mdp)
        a.update(kw)
        return lib.cp_coco_accumulate(None, a["dm"], a["di"], a["gi"], a["rank"], a["order"], a["host"], dev, K, ND, NGT, a["md"], a["rec"],
                                      a["pr"], a["rc"])
    for name in ("dm", "di", "gi", "rank", "order", "rec", "pr", "rc", "host", "md"):
        assert acc(**{name: None}) == -1, name
    assert acc(dev=None) == -1 and acc(K=0) == -1 and acc(ND=6) == -1 and acc(det=(0, 5, 2), ND=2) == -1 and acc(gt=(0, 3, 2), NGT=2) == -1
    assert acc(mds=(1, 10, 101)) == -1 and acc(mds=(0, 10, 100)) == -1 and acc(pr=C.c_void_p(4100)) == -3
    assert lib.cp_kernel_log() == b""                                           # nothing was launched
