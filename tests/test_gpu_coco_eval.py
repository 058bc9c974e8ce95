"""GPU: row N15 (csrc/coco_eval.hip through checkerpose_amd/coco_eval.py) against tests/coco_stages.py and the values recorded from
bop_toolkit_lib/pycoco_utils.py.  Everything is exact: no tolerance anywhere.

Frames (H x W) 31 x 33, 50 x 70 and 120 x 160: one tail bit, a width that is no multiple of 32, five words per row.  The drawn world
(coco_stages.draw_world) has 6 images and 5 categories -- one empty, one with detections and no ground truth -- and groups of
D in {0, 1, 7, 100, 103} detections and G in {0, 1, 7} ground truths."""
import json
import os

import numpy as np
import pytest
import torch

from checkerpose_amd import coco_eval as CE
from tests import coco_stages as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coco_eval.npz")
FRAMES = ((31, 33), (50, 70), (120, 160))
_WORLDS = {}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def fixture_masks(gold, H, W):
    tag = "%dx%d" % (H, W)
    bits = np.unpackbits(gold["masks_" + tag], axis=1)[:, :H * W].reshape(-1, H, W)
    return bits.astype(np.uint8) * gold["values_" + tag][:, None, None].astype(np.uint8), tag


def to_sets(world, stock_ignore=False, dts=None):
    """a coco_stages world as the module's inputs: (CocoSet with masks and boxes, dets dict)"""
    gts, dts = world["gts"], world["dts"] if dts is None else dts
    cs = CE.CocoSet(world["image_ids"], world["category_ids"], [g["image_id"] for g in gts], [g["category_id"] for g in gts],
                    [g["area"] for g in gts], [g["ignore"] for g in gts], [g["iscrowd"] for g in gts],
                    masks=torch.from_numpy(np.stack([g["mask"] for g in gts])).to(DEV) if gts else None,
                    bbox=torch.tensor([g["bbox"] for g in gts], dtype=torch.float64, device=DEV) if gts else None,
                    stock_ignore=stock_ignore, device=DEV)
    dets = {"image_id": [d["image_id"] for d in dts], "category_id": [d["category_id"] for d in dts], "score": [d["score"] for d in dts]}
    if dts:
        dets["masks"] = torch.from_numpy(np.stack([d["mask"] for d in dts])).to(DEV)
        dets["bbox"] = torch.tensor([d["bbox"] for d in dts], dtype=torch.float64, device=DEV)
    return cs, dets


def shared(H, W):
    """the drawn world of a frame size: the restatement (once) and the device result with its tables, both annotation types"""
    if (H, W) not in _WORLDS:
        world = S.draw_world(H, W, seed=H)
        cs, dets = to_sets(world)
        _WORLDS[(H, W)] = {"world": world, "sets": (cs, dets),
                           "ref": {t: S.evaluate(world, t) for t in ("segm", "bbox")},
                           "got": {t: CE.evaluate(cs, dets, t, return_tables=True) for t in ("segm", "bbox")}}
    return _WORLDS[(H, W)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("H,W", FRAMES)
def test_pack_area_box_and_rle_equal_the_recorded_reference_values(gold, H, W):
    masks, tag = fixture_masks(gold, H, W)
    out = CE.annotate_masks(torch.from_numpy(masks).to(DEV), return_rle=True)
    b = masks != 0
    assert out["area"].dtype == torch.int32 and out["area"].cpu().numpy().tolist() == b.reshape(len(b), -1).sum(1).tolist()
    assert out["bbox"].cpu().numpy().tolist() == gold["bbox_" + tag].tolist()          # -1s for the empty mask
    box = out["box"].cpu().numpy()
    assert box[0].tolist() == [-1] * 4 and (box[1:, 2] - box[1:, 0] + 1 == gold["bbox_" + tag][1:, 2]).all()
    WW = (W + 31) // 32
    padded = np.zeros((len(b), H, WW * 32), np.uint8)
    padded[:, :, :W] = b
    words = np.packbits(padded.reshape(len(b), H, WW, 32), axis=-1, bitorder="little").view("<u4").reshape(len(b), H, WW)
    assert np.array_equal(out["packed"].bits.cpu().numpy().view(np.uint32), words)      # bits past W are zero
    assert out["rle_counts"].dtype == torch.int32 and out["rle_counts"].cpu().numpy().tolist() == gold["rle_counts_" + tag].tolist()
    assert out["rle_offsets"].cpu().numpy().tolist() == gold["rle_offsets_" + tag].tolist()
    infos = json.loads(str(gold["infos_" + tag]))
    for n in range(1, len(b)):
        assert out["rle"][n] == infos[n]["segmentation"] and int(out["area"][n]) == infos[n]["area"], n
    # a mask alone gives the same bits as in its batch; a bool tensor and a second call too
    again = CE.annotate_masks(torch.from_numpy(b).to(DEV), return_rle=True)
    assert torch.equal(again["rle_counts"], out["rle_counts"]) and torch.equal(again["packed"].bits, out["packed"].bits)
    for n in (0, 5, 9):
        one = CE.annotate_masks(torch.from_numpy(masks[n:n + 1]).to(DEV), return_rle=True)
        assert one["rle"][0] == out["rle"][n] and torch.equal(one["box"][0], out["box"][n]) and torch.equal(one["area"][0], out["area"][n])


@pytest.mark.parametrize("ann_type", ["segm", "bbox"])
@pytest.mark.parametrize("H,W", FRAMES)
def test_ious_and_match_tables_equal_the_restatement(H, W, ann_type):
    w = shared(H, W)
    ref, got = w["ref"][ann_type], w["got"][ann_type]
    plan = got["plan"]
    imgs, cats = sorted(w["world"]["image_ids"]), sorted(w["world"]["category_ids"])
    keys = [(imgs[i], cats[c]) for c, i in zip(plan["group_cat"], plan["group_img"])]
    assert sorted(keys) == sorted(ref["groups"]) and got["ious"].dtype == np.float64
    sizes = set()
    for n, key in enumerate(keys):
        r = ref["groups"][key]
        d0, d1, g0, g1 = plan["det_off"][n], plan["det_off"][n + 1], plan["gt_off"][n], plan["gt_off"][n + 1]
        sizes.add((d1 - d0, g1 - g0))
        assert same_bits(got["ious"][plan["iou_off"][n]:plan["iou_off"][n + 1]].reshape(d1 - d0, g1 - g0), r["ious"]), key
        assert np.array_equal(got["dt_match"][d0:d1].transpose(1, 2, 0), r["dtm"]), key
        assert np.array_equal(got["dt_ignore"][d0:d1].transpose(1, 2, 0) != 0, r["dtIg"]), key
        assert np.array_equal(got["gt_ignore"][g0:g1].T, r["gtIg"]), key
    assert {d for d, _ in sizes} == {0, 1, 7, 100} and {g for _, g in sizes} == {0, 1, 7}
    assert (got["ious"] > 0.5).any() and (got["ious"] == 0).any() and (got["dt_match"] > 0).any() and got["dt_ignore"].any()


@pytest.mark.parametrize("ann_type", ["segm", "bbox"])
@pytest.mark.parametrize("H,W", FRAMES)
def test_precision_recall_and_the_twelve_scores_equal_the_restatement(H, W, ann_type):
    w = shared(H, W)
    ref, got = w["ref"][ann_type], w["got"][ann_type]
    assert got["precision"].shape == (10, 101, 5, 4, 3) and got["recall"].shape == (10, 5, 4, 3)
    assert same_bits(got["precision"], ref["precision"]) and same_bits(got["recall"], ref["recall"])
    for name in S.STAT_NAMES:
        assert got[name] == ref["stats"][name], name
    assert (got["precision"][:, :, 3:] == -1).all() and 0 < got["AP"] < 1 and got["AR1"] < got["AR100"]


def test_stock_ignore_switch_and_dict_level_twin():
    w = shared(31, 33)
    world = w["world"]
    cs, dets = to_sets(world, stock_ignore=True)
    got, ref = CE.evaluate(cs, dets, "segm"), S.evaluate(world, "segm", stock_ignore=True)
    assert same_bits(got["precision"], ref["precision"]) and same_bits(got["recall"], ref["recall"])
    assert got["AP"] != w["got"]["segm"]["AP"]
    # eval_bop22_coco: two scenes of three images each; the second scene's image ids are moved by max id + 1 = 6
    scene_of = {2: 1, 3: 1, 5: 1, 8: 2, 13: 2, 15: 2}
    local = {8: 0, 13: 4, 15: 5}
    anns, results = {}, []
    for s in (1, 2):
        ims = [i for i in world["image_ids"] if scene_of[i] == s]
        anns[s] = {"categories": [{"id": c} for c in world["category_ids"]], "images": [{"id": local.get(i, i)} for i in ims], "annotations": []}
    for n, g in enumerate(world["gts"]):
        anns[scene_of[g["image_id"]]]["annotations"].append(
            {"id": n + 1, "image_id": local.get(g["image_id"], g["image_id"]), "category_id": g["category_id"], "iscrowd": 0, "area": g["area"],
             "bbox": g["bbox"], "ignore": g["ignore"], "segmentation": S.binary_mask_to_rle(g["mask"])})
    for d in world["dts"]:
        results.append({"scene_id": scene_of[d["image_id"]], "image_id": local.get(d["image_id"], d["image_id"]), "category_id": d["category_id"],
                        "score": d["score"], "bbox": d["bbox"], "segmentation": S.binary_mask_to_rle(d["mask"]), "time": 0.5})
    targets = [{"scene_id": scene_of[i], "im_id": local.get(i, i)} for i in world["image_ids"]]
    merged_id = {2: 2, 3: 3, 5: 5, 8: 6, 13: 10, 15: 11}
    moved = dict(world, image_ids=[merged_id[i] for i in world["image_ids"]], gts=[dict(g, image_id=merged_id[g["image_id"]]) for g in world["gts"]],
                 dts=[dict(d, image_id=merged_id[d["image_id"]]) for d in world["dts"]])
    for ann_type in ("segm", "bbox"):
        want = S.evaluate(moved, ann_type)["stats"]
        scores = CE.eval_bop22_coco(anns, results, targets, ann_type, device=DEV)
        assert {k: scores[k] for k in S.STAT_NAMES} == want and scores["average_time_per_image"] == 0.5
        assert want == w["ref"][ann_type]["stats"]                              # moving image ids in order changes nothing
    # a target list without image 13 (local id 4 of scene 2): its annotations and results are dropped
    fewer = [t for t in targets if not (t["scene_id"] == 2 and t["im_id"] == 4)]
    less = dict(moved, image_ids=[i for i in moved["image_ids"] if i != 10], gts=[g for g in moved["gts"] if g["image_id"] != 10],
                dts=[d for d in moved["dts"] if d["image_id"] != 10])
    scores = CE.eval_bop22_coco(anns, results, fewer, "segm", device=DEV)
    assert {k: scores[k] for k in S.STAT_NAMES} == S.evaluate(less, "segm")["stats"]


def test_calc_gt_coco_on_the_device_masks_of_scene_gt_info():
    from checkerpose_amd import gt_info as GI
    from tests.test_gt_info import depth_of, fixture, n_cases
    from tests.test_vsd_error import mesh_set
    g, _ = fixture()
    idx = [c for c in range(n_cases()) if int(g["scene"][c]) == 3]              # 160 x 120, two objects in one image
    im = 7
    scene_gt = {im: [{"obj_id": 10 + int(g["mesh"][c]), "cam_R_m2c": g["R"][c], "cam_t_m2c": np.asarray(g["t"][c]).reshape(3, 1)} for c in idx]}
    camera = {im: {"cam_K": g["K"][idx[0]], "depth_scale": 1.0}}
    obj_index = {10 + int(g["mesh"][c]): int(g["mesh"][c]) for c in idx}
    info, masks = GI.scene_gt_info(scene_gt, camera, {im: depth_of(idx[0])}, mesh_set(), obj_index, delta=float(g["delta"][idx[0]]),
                                   device=DEV, return_masks=True)
    assert len(masks) == len(idx) and any(m[1].any() for m in masks.values())
    for bbox_type in ("amodal", "modal"):
        got = CE.calc_gt_coco(scene_gt, info, masks, bbox_type=bbox_type, device=DEV)
        want = S.calc_gt_coco(scene_gt, info, masks, bbox_type)
        assert got["annotations"] == want and len(want) >= 1 and got["images"] == [{"id": im, "width": 160, "height": 120}]
        assert all(a["area"] == int((masks[(im, a["id"] - 1)][1] > 0).sum()) for a in want) or len(want) < len(idx)


@pytest.mark.parametrize("H,W", FRAMES)
def test_calc_gt_coco_skip_rule_ids_and_ignore_flags(gold, H, W):
    masks, _ = fixture_masks(gold, H, W)
    visib = masks[[8, 0, 9, 10, 11, 12, 13]]                                    # the second instance has no visible pixel
    full = masks[[8, 9, 0, 1, 11, 12, 1]]                                       # the third no full mask: skipped with 'amodal' only
    scene_gt = {5: [{"obj_id": 3}, {"obj_id": 4}, {"obj_id": 3}], 2: [{"obj_id": 9}], 11: [], 12: [{"obj_id": 1}, {"obj_id": 1}, {"obj_id": 2}]}
    fr = [0.5, 0.0, 0.3, 0.05, 0.1, 0.0999, 1.0]
    info = {5: [{"visib_fract": f} for f in fr[:3]], 2: [{"visib_fract": fr[3]}], 11: [], 12: [{"visib_fract": f} for f in fr[4:]]}
    rows = [(im, j) for im, insts in scene_gt.items() for j in range(len(insts))]
    as_dict = {key: (full[n], visib[n]) for n, key in enumerate(rows)}
    for bbox_type in ("amodal", "modal"):
        want = S.calc_gt_coco(scene_gt, info, as_dict, bbox_type)
        got = CE.calc_gt_coco(scene_gt, info, torch.from_numpy(visib).to(DEV), torch.from_numpy(full).to(DEV), bbox_type=bbox_type)
        assert got["annotations"] == want and [im["id"] for im in got["images"]] == [5, 2, 11, 12]
        assert [a["id"] for a in want] == list(range(1, len(want) + 1)) and len(want) == (5 if bbox_type == "amodal" else 6)
        assert [a["ignore"] for a in want if a["image_id"] in (2, 12)] == [True, False, True, False]
        assert CE.calc_gt_coco(scene_gt, info, as_dict, bbox_type=bbox_type, device=DEV)["annotations"] == want


def test_bitwise_two_calls_an_image_alone_and_shuffled_detections():
    w = shared(50, 70)
    world, (cs, dets) = w["world"], w["sets"]
    for ann_type in ("segm", "bbox"):
        first = w["got"][ann_type]
        again = CE.evaluate(cs, dets, ann_type, return_tables=True)
        for k in ("precision", "recall", "ious", "dt_match", "dt_ignore", "gt_ignore"):
            assert same_bits(first[k], again[k]), (ann_type, k)
        # image 2 (groups of 103, 7, 1 and 7 detections) alone: its groups' tables are the bits they are in the batch
        alone_world = dict(world, gts=[g for g in world["gts"] if g["image_id"] == 2], dts=[d for d in world["dts"] if d["image_id"] == 2])
        alone = CE.evaluate(*to_sets(alone_world), ann_type, return_tables=True)
        pa, pb = alone["plan"], first["plan"]
        imgs = sorted(world["image_ids"])
        rows = [n for n in range(pb["n_groups"]) if imgs[pb["group_img"][n]] == 2]
        assert len(rows) == pa["n_groups"] == 4
        for na, nb in enumerate(rows):
            for off, keys in (("det_off", ("dt_match", "dt_ignore")), ("gt_off", ("gt_ignore",)), ("iou_off", ("ious",))):
                for k in keys:
                    assert same_bits(alone[k][pa[off][na]:pa[off][na + 1]], first[k][pb[off][nb]:pb[off][nb + 1]]), (ann_type, k, nb)
    # detections with distinct scores in two input orders: the same tables
    world = S.draw_world(50, 70, seed=11, distinct_scores=True)
    assert len({d["score"] for d in world["dts"]}) == len(world["dts"])
    perm = np.random.default_rng(1).permutation(len(world["dts"]))
    for ann_type in ("segm", "bbox"):
        a = CE.evaluate(*to_sets(world), ann_type)
        b = CE.evaluate(*to_sets(world, dts=[world["dts"][i] for i in perm]), ann_type)
        assert same_bits(a["precision"], b["precision"]) and same_bits(a["recall"], b["recall"])
        ref = S.evaluate(world, ann_type)
        assert same_bits(a["precision"], ref["precision"]) and same_bits(a["recall"], ref["recall"])


def test_pairwise_ious_alone_and_refusals():
    w = shared(120, 160)
    world = w["world"]
    gts, dts = world["gts"][:9], world["dts"][:40]
    gm = torch.from_numpy(np.stack([g["mask"] for g in gts])).to(DEV)
    dm = torch.from_numpy(np.stack([d["mask"] for d in dts])).to(DEV)
    pairs = [(d, g) for d in range(len(dts)) for g in range(len(gts))]
    got = CE.mask_ious(dm, gm, pairs).cpu().numpy()
    assert got.tolist() == [S.mask_iou(dts[d]["mask"], gts[g]["mask"]) for d, g in pairs]
    bd, bg = torch.tensor([d["bbox"] for d in dts], dtype=torch.float64, device=DEV), torch.tensor([g["bbox"] for g in gts], dtype=torch.float64, device=DEV)
    gotb = CE.box_ious(bd, bg, pairs).cpu().numpy()
    assert gotb.tolist() == [S.box_iou(dts[d]["bbox"], gts[g]["bbox"]) for d, g in pairs]
    for n in (0, 17, len(pairs) - 1):                                          # a pair alone
        d, g = pairs[n]
        assert float(CE.mask_ious(dm[d:d + 1], gm[g:g + 1], [(0, 0)])[0]) == got[n] and float(CE.box_ious(bd[d], bg[g], [(0, 0)])[0]) == gotb[n]
    assert np.isnan(CE.mask_ious(dm, gm, [(0, 9), (40, 0), (-1, 0)]).cpu().numpy()).all()      # an index out of range: NaN, no read
    assert CE.mask_ious(dm, gm, []).numel() == 0
    with pytest.raises(ValueError, match="ground truth"):
        CE.mask_ious(dm, gm[:, :50], pairs)
    cs, dets = to_sets(world)
    with pytest.raises(ValueError, match="do not correspond"):
        CE.evaluate(cs, dict(dets, image_id=[99] * len(world["dts"])), "segm")
    with pytest.raises(ValueError, match="ann_type"):
        CE.evaluate(cs, dets, "keypoints")
    empty = CE.evaluate(CE.CocoSet([1, 2], [1], [], [], [], device=DEV), {"image_id": [], "category_id": [], "score": []}, "bbox")
    assert (empty["precision"] == -1).all() and empty["AP"] == -1.0


# ---- the named cases of tests/test_coco_eval.py on the device: the drawn worlds hold no IoU tie and hardly an IoU on a threshold ------
from tests.test_coco_eval import A, B_, FAR, box_world  # noqa: E402


def rasterised(world, H=64, W=128):
    """the same world with a mask per integer box (area = its count), for 'segm'"""
    def mask(b):
        m = np.zeros((H, W), bool)
        m[b[1]:b[1] + b[3], b[0]:b[0] + b[2]] = True
        return m
    return dict(world, gts=[dict(g, mask=mask(g["bbox"])) for g in world["gts"]], dts=[dict(d, mask=mask(d["bbox"])) for d in world["dts"]])


def on_device(world, ann_type="bbox", **kw):
    """the world through CE.evaluate; precision, recall and every group's tables must be the restatement's -> (restatement, device)"""
    ref = S.evaluate(world, ann_type, **kw)
    gts, dts = world["gts"], world["dts"]
    segm = ann_type == "segm"
    cs = CE.CocoSet(world["image_ids"], world["category_ids"], [g["image_id"] for g in gts], [g["category_id"] for g in gts],
                    [g["area"] for g in gts], [g["ignore"] for g in gts],
                    masks=torch.from_numpy(np.stack([g["mask"] for g in gts])).to(DEV) if segm else None,
                    bbox=None if segm else torch.tensor([g["bbox"] for g in gts], dtype=torch.float64, device=DEV), device=DEV, **kw)
    dets = {"image_id": [d["image_id"] for d in dts], "category_id": [d["category_id"] for d in dts], "score": [d["score"] for d in dts]}
    if dts:
        dets["masks" if segm else "bbox"] = (torch.from_numpy(np.stack([d["mask"] for d in dts])).to(DEV) if segm else
                                             torch.tensor([d["bbox"] for d in dts], dtype=torch.float64, device=DEV))
    got = CE.evaluate(cs, dets, ann_type, return_tables=True)
    assert same_bits(got["precision"], ref["precision"]) and same_bits(got["recall"], ref["recall"])
    assert all(got[k] == ref["stats"][k] for k in S.STAT_NAMES)
    plan = got["plan"]
    imgs, cats = sorted(world["image_ids"]), sorted(world["category_ids"])
    for n, (c, i) in enumerate(zip(plan["group_cat"], plan["group_img"])):
        r = ref["groups"][(imgs[i], cats[c])]
        d0, d1, g0, g1 = plan["det_off"][n], plan["det_off"][n + 1], plan["gt_off"][n], plan["gt_off"][n + 1]
        assert same_bits(got["ious"][plan["iou_off"][n]:plan["iou_off"][n + 1]].reshape(d1 - d0, g1 - g0), r["ious"])
        assert np.array_equal(got["dt_match"][d0:d1].transpose(1, 2, 0), r["dtm"])
        assert np.array_equal(got["dt_ignore"][d0:d1].transpose(1, 2, 0) != 0, r["dtIg"])
        assert np.array_equal(got["gt_ignore"][g0:g1].T, r["gtIg"])
    return ref, got


@pytest.mark.parametrize("ann_type", ["bbox", "segm"])
def test_device_the_later_ground_truth_wins_an_iou_tie(ann_type):
    g0, g1 = [0, 0, 10, 8], [0, 2, 10, 8]
    world = box_world([(1, 1, g0, 0), (1, 1, g1, 0)], [(1, 1, [0, 0, 10, 10], .9), (1, 1, g1, .8)])
    ref, got = on_device(rasterised(world) if ann_type == "segm" else world, ann_type)
    assert got["ious"].tolist() == [0.8, 0.8, 0.6, 1.0]
    dtm = got["dt_match"][:, 0, :]                                               # (detection, threshold) at the whole area range
    assert dtm[0, :6].tolist() == [2] * 6 and dtm[0, 7:].tolist() == [0] * 3     # the first detection takes g1, the LATER one
    assert dtm[1, 0] == 1 and dtm[1, 5] == 0                                     # so the second is left with g0 (IoU .6)
    assert abs(got["AP75"] - 51 / 101) <= 1e-12                                  # (first-wins would give both a match: AP75 = 1)


@pytest.mark.parametrize("num,den", [(1, 2), (3, 5), (3, 4), (9, 10)])
def test_device_iou_exactly_at_a_threshold_matches_when_it_is_not_below(num, den):
    thrs = S.iou_thrs()
    ref, got = on_device(box_world([(1, 1, [0, 0, 100, 100], 0)], [(1, 1, [0, 0, 100, 100 * num // den], .9)]))
    assert got["ious"].tolist() == [num / den]
    hit = [not (num / den < t) for t in thrs]
    assert (num, den) not in ((1, 2), (3, 4)) or thrs[int(round((num / den - .5) / .05))] == num / den      # hit exactly by the linspace
    assert got["dt_match"][0, 0, :].tolist() == [int(h) for h in hit] and got["recall"][:, 0, 0, 2].tolist() == [float(h) for h in hit]


def test_device_break_at_an_ignored_ground_truth_and_absorbing():
    ref, got = on_device(box_world([(1, 1, [0, 0, 100, 92], 1), (1, 1, [0, 0, 100, 72], 0)], [(1, 1, [0, 0, 100, 100], .9)]))
    assert got["ious"].tolist() == [0.92, 0.72]
    assert got["dt_match"][0, 0, :].tolist() == [2] * 5 + [1] * 4 + [0] and got["dt_ignore"][0, 0, :].tolist() == [0] * 5 + [1] * 4 + [0]
    assert got["AR100"] == 0.5 and abs(got["AP50"] - 1) <= 1e-12
    ref, got = on_device(box_world([(1, 1, A, 1), (1, 1, B_, 0)], [(1, 1, A, .95), (1, 1, B_, .9)]))
    assert got["dt_ignore"][0, 0, :].all() and not got["dt_ignore"][1, 0, :].any() and abs(got["AP"] - 1) <= 1e-12


@pytest.mark.parametrize("side,stats", [(32, ("small", "medium")), (96, ("medium", "large"))])
def test_device_areas_exactly_on_a_range_border(side, stats):
    box = [0, 0, side, side]
    for ann_type in ("bbox", "segm"):
        world = box_world([(1, 1, box, 0)], [(1, 1, box, .9)])
        ref, got = on_device(rasterised(world, 96, 96) if ann_type == "segm" else world, ann_type)
        for name in ("small", "medium", "large"):
            want = 1.0 if name in stats else -1.0
            assert abs(got["AP_" + name] - want) <= 1e-12 and got["AR_" + name] == want, (ann_type, name)
    ref, got = on_device(box_world([(1, 1, [200, 200, 40, 40], 0)], [(1, 1, box, .9), (1, 1, [200, 200, 40, 40], .8)]))
    assert not got["dt_ignore"][0, 1 if side == 32 else 2, :].any()


def test_device_ties_across_images_cut_maxdet_missing_ground_truth_and_stock_ignore():
    eps = 2.0 ** -52
    ref, got = on_device(box_world([(1, 1, A, 0), (2, 1, A, 0)], [(2, 1, A, .5), (1, 1, FAR, .5)]))
    assert abs(got["AP"] - 51 * (1 / (2 + eps)) / 101) <= 1e-12                  # score tie: image 1's false positive stays first
    noise = [(1, 1, [100 + 20 * i, 0, 10, 10], 1.0 - i / 1000.0) for i in range(102)]
    ref, got = on_device(box_world([(1, 1, A, 0)], noise[:50] + [(1, 1, A, 1.0 - 98.5 / 1000.0)] + noise[50:]))
    assert got["AR100"] == 1.0 and abs(got["AP"] - 1 / (100 + eps)) <= 1e-12 and len(got["dt_match"]) == 100
    ref, got = on_device(box_world([(1, 1, A, 0)], noise[:50] + [(1, 1, A, 1.0 - 99.5 / 1000.0)] + noise[50:]))
    assert got["AR100"] == 0.0 and got["AP"] == 0.0                              # rank 100 is cut
    ref, got = on_device(box_world([(1, 1, A, 0), (2, 1, A, 0)], [(1, 1, A, .3), (2, 1, FAR, .9), (2, 1, A, .8)]))
    assert got["AR1"] == 0.5 and got["AR10"] == 1.0                              # maxDet 1: the first of EVERY image
    ref, got = on_device(box_world([(1, 1, A, 0)], [(1, 1, A, .9), (1, 2, A, .9)]))
    assert (got["precision"][:, :, 1] == -1).all() and abs(got["AP"] - 1) <= 1e-12 and got["AR100"] == 1.0
    ref, got = on_device(box_world([(1, 1, A, 0), (1, 1, B_, 0)], [(1, 1, A, .9), (1, 1, FAR, .8), (1, 1, B_, .7)]))
    assert abs(got["AP"] - (51 + 50 * 2 / 3) / 101) <= 1e-12 and got["AR1"] == 0.5
    world = box_world([(1, 1, A, 1)], [(1, 1, A, .9)])
    assert on_device(world)[1]["AP"] == -1.0 and abs(on_device(world, stock_ignore=True)[1]["AP"] - 1) <= 1e-12


def test_calc_gt_coco_keeps_the_callers_keys(gold):
    masks, _ = fixture_masks(gold, 31, 33)
    scene_gt = {"000004": [{"obj_id": 3}, {"obj_id": 5}]}
    info = {"000004": [{"visib_fract": 0.5}, {"visib_fract": 0.01}]}
    m = torch.from_numpy(masks[[8, 9]]).to(DEV)
    got = CE.calc_gt_coco(scene_gt, info, m, m)
    assert [(a["id"], a["image_id"], a["ignore"]) for a in got["annotations"]] == [(1, 4, False), (2, 4, True)] and got["images"][0]["id"] == 4
