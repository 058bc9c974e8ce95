"""The BOP'22 COCO detection / segmentation task restated in float64 numpy: the yardstick of tests/test_coco_eval.py and
tests/test_gpu_coco_eval.py (row N15).  It reads nothing of the reference and nothing of checkerpose_amd.

Ground-truth side (bop_toolkit scripts/calc_gt_coco.py:84-121, bop_toolkit_lib/pycoco_utils.py:34-75,126-141,186-200): PINNED -- the
functions below reproduce the values that tests/golden/make_golden_coco_eval.py recorded from pycoco_utils itself.

Score side (pycocotools' COCO.loadRes + COCOeval.evaluate / accumulate / summarize as scripts/eval_bop22_coco.py:142-154 drives
them): UNPINNED -- pycocotools is not installed, so the published rule is restated twice, in two ways that share nothing but the
IoU helpers' definitions:
  evaluate(world, ann_type)         COCOeval's structure: per (image, category) IoU matrix, evaluateImg per area range with all
                                    thresholds at once, accumulate with numpy sorts / cumsum / searchsorted
  evaluate_brute(world, ann_type)   per (category, area range, maxDet, threshold) from scratch, plain Python loops and lists, its own
                                    sorting (sorted() with a key), IoU from pixel sets / Python floats

A world is a dict: "image_ids", "category_ids" (lists of ints), "size" (H, W), "gts": list of {"image_id", "category_id", "area",
"ignore", "iscrowd", "bbox" [x, y, w, h], "mask" (H,W) bool}, "dts": list of {"image_id", "category_id", "score", "bbox", "mask"}."""
import numpy as np

STAT_NAMES = ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR1", "AR10", "AR100", "AR_small", "AR_medium", "AR_large")
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]


def iou_thrs():
    return np.linspace(.5, .95, 10)


def rec_thrs():
    return np.linspace(0, 1, 101)


# ---- ground-truth side -------------------------------------------------------------------------------------------------------------
def binary_mask_to_rle(mask):
    """column-major run lengths; a leading 0 when the first pixel is set; size = [H, W]"""
    m = np.asarray(mask).astype(bool)
    flat = m.ravel(order="F")
    change = np.nonzero(flat[1:] != flat[:-1])[0] + 1
    edges = np.concatenate([[0], change, [flat.size]])
    counts = np.diff(edges).tolist()
    if flat[0]:
        counts = [0] + counts
    return {"counts": [int(c) for c in counts], "size": [int(m.shape[0]), int(m.shape[1])]}


def rle_to_binary_mask(rle):
    H, W = rle["size"]
    counts = np.asarray(rle["counts"], np.int64)
    flat = np.zeros(H * W, bool)
    values = np.repeat(np.arange(len(counts)) % 2 == 1, counts)
    flat[:len(values)] = values
    return flat.reshape(H, W, order="F")


def bbox_from_binary_mask(mask):
    m = np.asarray(mask).astype(bool)
    ys, xs = np.nonzero(m)
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


def create_annotation_info(annotation_id, image_id, object_id, mask, bounding_box, ignore=None):
    m = np.asarray(mask).astype(bool)
    area = int(m.sum())
    if area < 1:
        return None
    info = {"id": annotation_id, "image_id": image_id, "category_id": object_id, "iscrowd": 0, "area": area, "bbox": bounding_box,
            "segmentation": binary_mask_to_rle(m), "width": int(m.shape[1]), "height": int(m.shape[0])}
    if ignore is not None:
        info["ignore"] = ignore
    return info


def calc_gt_coco(scene_gt, scene_gt_info, masks, bbox_type="amodal"):
    """masks: {(im_id, gt_id): (mask, mask_visib)} -> the annotations list of one scene"""
    annotations, segmentation_id = [], 1
    for im_id, inst_list in scene_gt.items():
        for idx, inst in enumerate(inst_list):
            ignore_gt = bool(scene_gt_info[im_id][idx]["visib_fract"] < 0.1)
            full, visib = (np.asarray(m).astype(bool) for m in masks[(im_id, idx)])
            if visib.sum() < 1:
                continue
            if bbox_type == "amodal":
                if full.sum() < 1:
                    continue
                box = bbox_from_binary_mask(full)
            else:
                box = bbox_from_binary_mask(visib)
            info = create_annotation_info(segmentation_id, int(im_id), inst["obj_id"], visib, box, ignore=ignore_gt)
            if info is not None:
                annotations.append(info)
            segmentation_id += 1
    return annotations


def merge_scenes(scenes):
    """The id rule of pycoco_utils.merge_coco_annotations over a list of {"images", "annotations"}: every scene after the first has its
    image ids moved past the largest image id so far and its annotation ids past the largest annotation id so far (by 0 while there is
    none).  The inputs are left alone.  -> ({"images", "annotations"}, the image shift of each scene)"""
    images, annotations, shifts = [], [], []
    for n, scene in enumerate(scenes):
        by = 1 + max(im["id"] for im in images) if n else 0
        ann_by = 1 + max([a["id"] for a in annotations], default=-1) if n else 0
        images = images + [dict(im, id=im["id"] + by) for im in scene["images"]]
        annotations = annotations + [dict(a, id=a["id"] + ann_by, image_id=a["image_id"] + by) for a in scene["annotations"]]
        shifts.append(by)
    return {"images": images, "annotations": annotations}, shifts


# ---- IoU -----------------------------------------------------------------------------------------------------------------------------
def mask_iou(a, b):
    inter = int(np.logical_and(a, b).sum())
    if inter == 0:
        return 0.0
    return inter / (int(a.sum()) + int(b.sum()) - inter)


def box_iou(T, G):
    """maskApi bbIou, float64, one operation at a time"""
    T, G = np.asarray(T, np.float64), np.asarray(G, np.float64)
    da, ga = T[2] * T[3], G[2] * G[3]
    w = np.minimum(T[2] + T[0], G[2] + G[0]) - np.maximum(T[0], G[0])
    if w <= 0:
        w = np.float64(0)
    h = np.minimum(T[3] + T[1], G[3] + G[1]) - np.maximum(T[1], G[1])
    if h <= 0:
        h = np.float64(0)
    i = w * h
    u = da + ga - i
    return float(i / u)


def det_area(d, ann_type):
    return float(int(np.asarray(d["mask"]).sum())) if ann_type == "segm" else float(np.float64(d["bbox"][2]) * np.float64(d["bbox"][3]))


def gt_ignored(g, stock_ignore):
    """the cocoapi fork BOP installs: the annotation's flag OR iscrowd; stock pycocotools: iscrowd alone"""
    return bool(g["iscrowd"]) if stock_ignore else bool(g.get("ignore", False) or g["iscrowd"])


# ---- restatement 1: COCOeval's structure ------------------------------------------------------------------------------------------------
def _groups(world):
    gts, dts = {}, {}
    for g in world["gts"]:
        gts.setdefault((g["image_id"], g["category_id"]), []).append(g)
    for d in world["dts"]:
        if d["image_id"] not in world["image_ids"]:
            raise ValueError("Results do not correspond to current coco set")
        dts.setdefault((d["image_id"], d["category_id"]), []).append(d)
    return gts, dts


def compute_iou(gt, dt, ann_type):
    """computeIoU: detections in stable descending score order, cut to 100 -> (the kept detections, (D,G) float64)"""
    inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in inds][:MAX_DETS[-1]]
    ious = np.zeros((len(dt), len(gt)), np.float64)
    for i, d in enumerate(dt):
        for j, g in enumerate(gt):
            ious[i, j] = mask_iou(d["mask"], g["mask"]) if ann_type == "segm" else box_iou(d["bbox"], g["bbox"])
    return dt, ious


def evaluate_img(gt, dt, ious, a_rng, ann_type, stock_ignore):
    """evaluateImg at maxDet 100 -> dtm (T,D) = index of the matched ground truth in INPUT order + 1, dtIg (T,D), gtIg (G,) in input
    order, the detections' scores"""
    thrs = iou_thrs()
    G, D, T = len(gt), len(dt), len(thrs)
    g_ig = np.array([1 if (gt_ignored(g, stock_ignore) or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gt], int)
    gtind = np.argsort(g_ig, kind="mergesort")
    gtIg = g_ig[gtind]
    gtm, dtm, dtIg = np.zeros((T, G), int), np.zeros((T, D), int), np.zeros((T, D), int)
    if G and D:
        iou_s = ious[:, gtind]
        for tind, t in enumerate(thrs):
            for dind in range(D):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
                    if gtm[tind, gind] > 0:
                        continue
                    if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                        break
                    if iou_s[dind, gind] < iou:
                        continue
                    iou = iou_s[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dtIg[tind, dind] = gtIg[m]
                dtm[tind, dind] = gtind[m] + 1
                gtm[tind, m] = dind + 1
    a = np.array([det_area(d, ann_type) < a_rng[0] or det_area(d, ann_type) > a_rng[1] for d in dt], bool).reshape(1, D)
    dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return dtm, dtIg, g_ig, np.array([d["score"] for d in dt], np.float64)


def summarize(precision, recall):
    thrs = iou_thrs()

    def stat(ap, thr=None, a=0, m=2):
        s = precision if ap else recall
        if thr is not None:
            s = s[np.where(thr == thrs)[0]]
        s = s[..., a, m]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    vals = [stat(1), stat(1, .5), stat(1, .75), stat(1, a=1), stat(1, a=2), stat(1, a=3),
            stat(0, m=0), stat(0, m=1), stat(0, m=2), stat(0, a=1), stat(0, a=2), stat(0, a=3)]
    return dict(zip(STAT_NAMES, vals))


def evaluate(world, ann_type, stock_ignore=False):
    """-> {"precision" (10,101,K,4,3), "recall" (10,K,4,3), "stats", "groups": {(image_id, category_id): {"ious" (D,G), "dtm" (4,10,D),
    "dtIg" (4,10,D), "gtIg" (4,G), "scores" (D,)}}}"""
    for g in world["gts"]:
        if g["iscrowd"]:
            raise ValueError("iscrowd must be 0")
    thrs, recs = iou_thrs(), rec_thrs()
    img_ids, cat_ids = sorted(set(world["image_ids"])), sorted(set(world["category_ids"]))
    gts, dts = _groups(world)
    T, R, K, A, M = len(thrs), len(recs), len(cat_ids), len(AREA_RNG), len(MAX_DETS)
    groups = {}
    for cat in cat_ids:
        for img in img_ids:
            gt, dt = gts.get((img, cat), []), dts.get((img, cat), [])
            if not gt and not dt:
                continue
            dt, ious = compute_iou(gt, dt, ann_type)
            per_area = [evaluate_img(gt, dt, ious, rng, ann_type, stock_ignore) for rng in AREA_RNG]
            groups[(img, cat)] = {"ious": ious, "dtm": np.stack([p[0] for p in per_area]), "dtIg": np.stack([p[1] for p in per_area]),
                                  "gtIg": np.stack([p[2] for p in per_area]), "scores": per_area[0][3]}
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k, cat in enumerate(cat_ids):
        E = [groups[(img, cat)] for img in img_ids if (img, cat) in groups]
        if not E:
            continue
        for a in range(A):
            for m, max_det in enumerate(MAX_DETS):
                scores = np.concatenate([e["scores"][:max_det] for e in E])
                inds = np.argsort(-scores, kind="mergesort")
                dtm = np.concatenate([e["dtm"][a][:, :max_det] for e in E], axis=1)[:, inds]
                dtIg = np.concatenate([e["dtIg"][a][:, :max_det] for e in E], axis=1)[:, inds]
                gtIg = np.concatenate([e["gtIg"][a] for e in E])
                npig = np.count_nonzero(gtIg == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtIg))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, recs, side="left")
                    try:
                        for ri, pi in enumerate(inds_r):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return {"precision": precision, "recall": recall, "stats": summarize(precision, recall), "groups": groups}


# ---- restatement 2: brute force ---------------------------------------------------------------------------------------------------------
def _brute_iou(d, g, ann_type):
    if ann_type == "segm":
        pa = set(zip(*np.nonzero(d["mask"])))
        pb = set(zip(*np.nonzero(g["mask"])))
        inter = len(pa & pb)
        return 0.0 if inter == 0 else inter / len(pa | pb)
    dx, dy, dw, dh = (float(v) for v in d["bbox"])
    gx, gy, gw, gh = (float(v) for v in g["bbox"])
    w = min(dx + dw, gx + gw) - max(dx, gx)
    h = min(dy + dh, gy + gh) - max(dy, gy)
    w = 0.0 if w <= 0 else w
    h = 0.0 if h <= 0 else h
    i = w * h
    return i / (dw * dh + gw * gh - i)


def evaluate_brute(world, ann_type, stock_ignore=False):
    """-> {"precision", "recall", "stats"}: every (category, area range, threshold) matched from scratch"""
    thrs, recs = [float(t) for t in iou_thrs()], [float(r) for r in rec_thrs()]
    img_ids, cat_ids = sorted(set(world["image_ids"])), sorted(set(world["category_ids"]))
    K = len(cat_ids)
    precision, recall = -np.ones((10, 101, K, 4, 3)), -np.ones((10, K, 4, 3))
    cache = {}
    for k, cat in enumerate(cat_ids):
        per_img = []
        for img in img_ids:
            gt = [g for g in world["gts"] if g["image_id"] == img and g["category_id"] == cat]
            dt = [d for d in world["dts"] if d["image_id"] == img and d["category_id"] == cat]
            if gt or dt:
                dt = sorted(dt, key=lambda d: -d["score"])[:100]
                for d in dt:
                    for g in gt:
                        cache[(id(d), id(g))] = _brute_iou(d, g, ann_type)
                per_img.append((gt, dt))
        if not per_img:
            continue
        for a, (lo, hi) in enumerate(AREA_RNG):
            for t, thr in enumerate(thrs):
                rows, npig = [], 0                       # rows: (score, image position, rank, matched, ignored)
                for pos, (gt, dt) in enumerate(per_img):
                    ign = [gt_ignored(g, stock_ignore) or g["area"] < lo or g["area"] > hi for g in gt]
                    npig += sum(1 for v in ign if not v)
                    walk = [j for j in range(len(gt)) if not ign[j]] + [j for j in range(len(gt)) if ign[j]]
                    taken = set()
                    for rank, d in enumerate(dt):
                        best, m = min(thr, 1 - 1e-10), None
                        for j in walk:
                            if j in taken:
                                continue
                            if m is not None and not ign[m] and ign[j]:
                                break
                            if cache[(id(d), id(gt[j]))] < best:
                                continue
                            best, m = cache[(id(d), id(gt[j]))], j
                        if m is None:
                            ar = det_area(d, ann_type)
                            rows.append((d["score"], pos, rank, False, ar < lo or ar > hi))
                        else:
                            taken.add(m)
                            rows.append((d["score"], pos, rank, True, ign[m]))
                if npig == 0:
                    continue
                for mi, max_det in enumerate(MAX_DETS):
                    lst = sorted([r for r in rows if r[2] < max_det], key=lambda r: (-r[0], r[1], r[2]))
                    tp = fp = 0
                    rc, pr = [], []
                    for r in lst:
                        if not r[4]:
                            if r[3]:
                                tp += 1
                            else:
                                fp += 1
                        rc.append(tp / npig)
                        pr.append(tp / (fp + tp + 2.0 ** -52))
                    recall[t, k, a, mi] = rc[-1] if lst else 0.0
                    for r_i, thr_r in enumerate(recs):
                        reach = [p for c, p in zip(rc, pr) if c >= thr_r]
                        precision[t, r_i, k, a, mi] = max(reach) if reach else 0.0
    return {"precision": precision, "recall": recall, "stats": summarize(precision, recall)}


# ---- the drawn world ------------------------------------------------------------------------------------------------------------------
# (D, G) of every (category, image) group: D in {0, 1, 7, 100, 103}, G in {0, 1, 7}; category 7 has detections and no ground truth,
# category 9 is empty, image 15 has neither
IMAGE_IDS = [2, 3, 5, 8, 13, 15]
CATEGORY_IDS = [1, 3, 4, 7, 9]
LAYOUT = {1: {2: (103, 7), 3: (1, 1), 5: (0, 1), 8: (7, 0), 13: (100, 7)},
          3: {2: (7, 7), 3: (7, 1), 5: (1, 0), 8: (0, 7), 13: (1, 7)},
          4: {2: (1, 1), 5: (7, 7), 8: (7, 1)},
          7: {2: (7, 0), 5: (1, 0)}}


def _blob(rng, H, W, box=None):
    """a rectangle with ragged content (so that runs and tail bits are exercised); never empty"""
    if box is None:
        w, h = int(rng.integers(2, max(3, W // 2))), int(rng.integers(2, max(3, H // 2)))
        x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
    else:
        x, y, w, h = box
        x, y = int(np.clip(x, 0, W - 1)), int(np.clip(y, 0, H - 1))
        w, h = int(np.clip(w, 1, W - x)), int(np.clip(h, 1, H - y))
    m = np.zeros((H, W), bool)
    m[y:y + h, x:x + w] = rng.random((h, w)) > 0.15
    m[y, x] = True
    return m, (x, y, w, h)


def draw_world(H, W, seed=0, distinct_scores=False):
    """6 images, 5 categories, the LAYOUT above on an H x W frame.  Scores are drawn from a coarse grid (ties within and across images)
    unless distinct_scores.  Some ground truths carry the ignore flag; two touch the right and bottom edges."""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for cat, per_img in LAYOUT.items():
        for img, (D, G) in per_img.items():
            mine = []
            for j in range(G):
                box = (W - 4, H - 3, 4, 3) if (j == 0 and G == 7) else None
                mask, box = _blob(rng, H, W, box)
                g = {"image_id": img, "category_id": cat, "area": int(mask.sum()), "ignore": bool(rng.random() < 0.2), "iscrowd": 0,
                     "bbox": bbox_from_binary_mask(mask), "mask": mask, "rect": box}
                mine.append(g)
            for j in range(D):
                if mine and rng.random() < 0.7:
                    x, y, w, h = mine[int(rng.integers(len(mine)))]["rect"]
                    jit = rng.integers(-2, 3, 4)
                    mask, _ = _blob(rng, H, W, (x + jit[0], y + jit[1], w + jit[2], h + jit[3]))
                    if rng.random() < 0.15:
                        mask = mine[int(rng.integers(len(mine)))]["mask"].copy()        # an exact copy: IoU 1, and ties between detections
                else:
                    mask, _ = _blob(rng, H, W)
                tight = bbox_from_binary_mask(mask)
                frac = rng.integers(0, 4, 4) * 0.25
                bbox = [tight[0] + frac[0], tight[1] + frac[1], tight[2] + frac[2], tight[3] + frac[3]]
                score = float(rng.random()) if distinct_scores else float(rng.integers(0, 12)) / 11.0
                dts.append({"image_id": img, "category_id": cat, "score": score, "bbox": [float(v) for v in bbox], "mask": mask})
            gts.extend(mine)
    order = rng.permutation(len(dts))                     # detections arrive in no particular order
    return {"image_ids": list(IMAGE_IDS), "category_ids": list(CATEGORY_IDS), "size": (H, W), "gts": gts, "dts": [dts[i] for i in order]}
