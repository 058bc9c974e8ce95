"""benchmark of row N15 (checkerpose_amd/coco_eval.py: the BOP'22 COCO detection / segmentation scores on the device).

  python tools/coco_eval_bench.py [--out profiles/coco_eval_bench.json] [--calls 60] [--windows 3] [--warmup 3] [--quick]

One seeded world at BOP scale: 900 images of 640 x 480, 6 ground truths each (15 categories), 1 - 100 detections per image, 'segm' and
'bbox'.  Masks are rectangles with a hole pattern, drawn by the same rule with torch on the device and with numpy on the host.

Device (an MI355X; there is no fallback): the host clock around the whole Python call -- `evaluate` ends with the download of the
tables and `calc_gt_coco` with the download of the run lengths, so each call ends synchronised.  `evaluate` starts from packed masks
and is timed in `--windows` windows of `--calls` calls each (about a second per window) after `--warmup` warm-ups; the figure is the
median of all calls, and the medians of the single windows are kept beside it as the spread within the run (the spread between
machines is not covered).  `evaluate_plan_ms` is the host index plan alone (make_plan), which every call includes.  `pack_masks` is
timed on its own: the detections are packed in chunks, 45 000 frames of 640 x 480 do not fit the device as bytes at once.
Host: tests/coco_stages.py's restatement (`evaluate`) on the first `--host-images` images and a Python loop over every pixel of the
column-major mask (the kind of work pycoco_utils.binary_mask_to_rle does) on `--host-rle` masks, each scaled linearly to the whole
world and marked as extrapolated.  pycocotools itself is not installed: no figure for it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from checkerpose_amd import coco_eval as CE  # noqa: E402
from tests import coco_stages as S  # noqa: E402

W, H, N_CAT, PER_IMAGE = 640, 480, 15, 6


def draw(n_img, seed=0):
    """boxes and ids only: gts (image, category, x, y, w, h, visib_fract), dts (image, category, x, y, w, h, score)"""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for im in range(n_img):
        cats = rng.permutation(N_CAT)[:PER_IMAGE] + 1
        mine = []
        for c in cats:
            w, h = int(rng.integers(20, 200)), int(rng.integers(20, 200))
            x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
            mine.append((im, int(c), x, y, w, h, float(rng.random())))
        gts.extend(mine)
        for _ in range(int(rng.integers(1, 101))):
            if rng.random() < 0.6:
                _, c, x, y, w, h, _ = mine[int(rng.integers(PER_IMAGE))]
                j = rng.integers(-8, 9, 4)
                x, y = int(np.clip(x + j[0], 0, W - 2)), int(np.clip(y + j[1], 0, H - 2))
                w, h = int(np.clip(w + j[2], 1, W - x)), int(np.clip(h + j[3], 1, H - y))
            else:
                c = int(rng.integers(1, N_CAT + 1))
                w, h = int(rng.integers(20, 200)), int(rng.integers(20, 200))
                x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
            dts.append((im, c, x, y, w, h, float(rng.random())))
    return gts, dts


def masks_numpy(rows):
    ys, xs = np.mgrid[0:H, 0:W]
    holes = (xs + 2 * ys) % 7 == 0
    return [(xs >= r[2]) & (xs < r[2] + r[4]) & (ys >= r[3]) & (ys < r[3] + r[5]) & ~holes for r in rows]


def masks_torch(rows, dev):
    b = torch.tensor([r[2:6] for r in rows], dtype=torch.int32, device=dev)
    ys, xs = torch.arange(H, device=dev, dtype=torch.int32)[None, :, None], torch.arange(W, device=dev, dtype=torch.int32)[None, None, :]
    x, y, w, h = (b[:, k][:, None, None] for k in range(4))
    return ((xs >= x) & (xs < x + w) & (ys >= y) & (ys < y + h) & ((xs + 2 * ys) % 7 != 0)).to(torch.uint8)


def pack_chunks(rows, dev, chunk=1000):
    parts, ms = [], 0.0
    for i in range(0, len(rows), chunk):
        m = masks_torch(rows[i:i + chunk], dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = CE.pack_masks(m)
        torch.cuda.synchronize()
        ms += (time.perf_counter() - t0) * 1e3
        parts.append(p)
        del m
    return CE.concat_packed(parts), ms


def median_ms(fn, calls, warmup, windows=1):
    """-> (median of all calls, the median of each window)"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(windows):
        win = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            win.append((time.perf_counter() - t0) * 1e3)
        out.append(win)
    return float(np.median(np.concatenate(out))), [round(float(np.median(w)), 3) for w in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_eval_bench.json"))
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=900)
    ap.add_argument("--host-images", type=int, default=12)
    ap.add_argument("--host-rle", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.quick:
        a.images, a.calls, a.windows, a.warmup, a.host_images, a.host_rle = 30, 2, 1, 1, 2, 1
    if not torch.cuda.is_available():
        raise RuntimeError("tools/coco_eval_bench.py measures on an MI355X: no device, no figure")
    dev = torch.device("cuda:0")
    gts, dts = draw(a.images)
    print("world: %d images, %d ground truths, %d detections" % (a.images, len(gts), len(dts)), flush=True)
    gp, gt_pack_ms = pack_chunks(gts, dev)
    dp, dt_pack_ms = pack_chunks(dts, dev)
    col = lambda rows, k: [r[k] for r in rows]      # noqa: E731
    gbox = gp.box.to(torch.float64)
    gt_bbox = torch.cat([gbox[:, :2], gbox[:, 2:] - gbox[:, :2] + 1], 1)
    cs = CE.CocoSet(list(range(a.images)), list(range(1, N_CAT + 1)), col(gts, 0), col(gts, 1), gp.area.cpu().numpy(),
                    [r[6] < 0.1 for r in gts], masks=gp, bbox=gt_bbox, device=dev)
    dets = {"image_id": col(dts, 0), "category_id": col(dts, 1), "score": col(dts, 6), "masks": dp,
            "bbox": torch.tensor([r[2:6] for r in dts], dtype=torch.float64, device=dev)}
    res = {"bench": "coco_eval", "device": torch.cuda.get_device_name(0), "calls": a.calls, "windows": a.windows, "warmup": a.warmup, "frame": [W, H],
           "images": a.images, "ground_truths": len(gts), "detections": len(dts), "categories": N_CAT,
           "pack_ground_truth_ms": gt_pack_ms, "pack_detections_ms": dt_pack_ms}
    scores = {}
    for ann_type in ("segm", "bbox"):
        scores[ann_type] = CE.evaluate(cs, dets, ann_type)
        med, all_ms = median_ms(lambda: CE.evaluate(cs, dets, ann_type), a.calls, a.warmup, a.windows)
        res["evaluate_%s_ms" % ann_type], res["evaluate_%s_window_medians_ms" % ann_type] = med, all_ms
        res["AP_%s" % ann_type] = scores[ann_type]["AP"]
        print("evaluate %s: median %.2f ms %s, AP %.4f" % (ann_type, med, all_ms, scores[ann_type]["AP"]), flush=True)
    t0 = time.perf_counter()
    for _ in range(10):
        CE.make_plan(cs.image_ids, cs.category_ids, cs.image_id, cs.category_id, np.asarray(dets["image_id"]), np.asarray(dets["category_id"]),
                     np.asarray(dets["score"]))
    res["evaluate_plan_ms"] = (time.perf_counter() - t0) * 1e2
    print("index plan alone: %.2f ms" % res["evaluate_plan_ms"], flush=True)
    # calc_gt_coco: one scene holding every image, the masks resident (visible mask = full mask)
    scene_gt = {im: [] for im in range(a.images)}
    info = {im: [] for im in range(a.images)}
    for r in gts:
        scene_gt[r[0]].append({"obj_id": r[1]})
        info[r[0]].append({"visib_fract": r[6]})
    chunk = 600                                            # 100 images of resident masks per call: 184 MB as bytes
    def gt_coco():      # noqa: E306
        out = []
        for i in range(0, len(gts), chunk):
            ims = sorted({r[0] for r in gts[i:i + chunk]})
            m = masks_torch(gts[i:i + chunk], dev)
            out.append(CE.calc_gt_coco({k: scene_gt[k] for k in ims}, info, m, m, device=dev))
        return out
    med, all_ms = median_ms(gt_coco, 2 if a.quick else 5, 1)
    res["calc_gt_coco_ms"] = med
    res["calc_gt_coco_note"] = "whole world in calls of 100 images; includes drawing the masks with torch and building the dicts on the host"
    print("calc_gt_coco: median %.2f ms" % med, flush=True)

    # host: the restatement on the first images, the reference-style RLE on a few masks
    n_h = min(a.host_images, a.images)
    hg, hd = [r for r in gts if r[0] < n_h], [r for r in dts if r[0] < n_h]
    gm, dm = masks_numpy(hg), masks_numpy(hd)
    world = {"image_ids": list(range(n_h)), "category_ids": list(range(1, N_CAT + 1)), "size": (H, W),
             "gts": [{"image_id": r[0], "category_id": r[1], "area": int(m.sum()), "ignore": r[6] < 0.1, "iscrowd": 0,
                      "bbox": S.bbox_from_binary_mask(m), "mask": m} for r, m in zip(hg, gm)],
             "dts": [{"image_id": r[0], "category_id": r[1], "score": r[6], "bbox": [float(v) for v in r[2:6]], "mask": m} for r, m in zip(hd, dm)]}
    for ann_type in ("segm", "bbox"):
        t0 = time.perf_counter()
        ref = S.evaluate(world, ann_type)
        ms = (time.perf_counter() - t0) * 1e3
        sub = CE.evaluate(*subset_sets(world, dev), ann_type)
        res["host_%s_ms_%d_images" % (ann_type, n_h)] = ms
        res["host_%s_ms_extrapolated" % ann_type] = ms * a.images / n_h
        res["ratio_%s_host_extrapolated_over_device" % ann_type] = ms * a.images / n_h / res["evaluate_%s_ms" % ann_type]
        res["subset_equal_%s" % ann_type] = bool(sub["precision"].tobytes() == ref["precision"].tobytes() and
                                                 sub["recall"].tobytes() == ref["recall"].tobytes())
        print("host %s: %.1f ms on %d images -> %.0f ms extrapolated; device tables equal on the subset: %s"
              % (ann_type, ms, n_h, ms * a.images / n_h, res["subset_equal_%s" % ann_type]), flush=True)
    t0 = time.perf_counter()
    for m in gm[:a.host_rle]:
        runs, last, n = [], False, 0                      # runs of 0s and 1s in turn, the first one of 0s (possibly empty)
        for v in m.ravel(order="F").tolist():
            if v != last:
                runs.append(n)
                last, n = v, 0
            n += 1
        runs.append(n)
    ms = (time.perf_counter() - t0) * 1e3 / max(1, a.host_rle)
    res["host_rle_ms_per_mask"], res["host_rle_ms_extrapolated"] = ms, ms * len(gts)
    res["ratio_gt_coco_host_rle_extrapolated_over_device"] = ms * len(gts) / res["calc_gt_coco_ms"]
    res["host"] = "tests/coco_stages.py evaluate on %d images and a per-pixel Python RLE loop on %d masks, scaled linearly" % (n_h, a.host_rle)
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


def subset_sets(world, dev):
    gts, dts = world["gts"], world["dts"]
    cs = CE.CocoSet(world["image_ids"], world["category_ids"], [g["image_id"] for g in gts], [g["category_id"] for g in gts],
                    [g["area"] for g in gts], [g["ignore"] for g in gts], masks=torch.from_numpy(np.stack([g["mask"] for g in gts])).to(dev),
                    bbox=torch.tensor([g["bbox"] for g in gts], dtype=torch.float64, device=dev), device=dev)
    return cs, {"image_id": [d["image_id"] for d in dts], "category_id": [d["category_id"] for d in dts], "score": [d["score"] for d in dts],
                "masks": torch.from_numpy(np.stack([d["mask"] for d in dts])).to(dev),
                "bbox": torch.tensor([d["bbox"] for d in dts], dtype=torch.float64, device=dev)}


if __name__ == "__main__":
    main()
