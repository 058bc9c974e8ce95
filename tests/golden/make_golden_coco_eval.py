"""Records what bop_toolkit_lib/pycoco_utils.py itself gives on the fixture masks of row N15 -> tests/golden/coco_eval.npz.

Runs ONLY where the reference tree is (CHECKERPOSE_REFERENCE, default /root/reference; nothing of it travels, only the recorded
numbers).  pycoco_utils imports skimage at its top for the polygon encoding alone (out of scope here); skimage is not installed, so an
EMPTY stub module stands in for `skimage` / `skimage.measure` in sys.modules -- in this maker only.  The functions that then run, and
are therefore pinned: binary_mask_to_rle, rle_to_binary_mask, bbox_from_binary_mask, create_annotation_info(mask_encoding_format=
'rle'), merge_coco_annotations, merge_coco_results.  pycoco_utils.compute_ious is NOT recorded: nothing calls it and it is wrong
(np.einsum over bool arrays is an OR of ANDs, so every overlapping pair scores 1 / union).

    python tests/golden/make_golden_coco_eval.py
"""
import copy
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(REF, "bop_toolkit"))

for name in ("skimage", "skimage.measure"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["skimage"].measure = sys.modules["skimage.measure"]

from bop_toolkit_lib import pycoco_utils as P  # noqa: E402

FRAMES = ((31, 33), (50, 70), (120, 160))            # (H, W): one tail bit, a width that is no multiple of 32, five words per row


def fixture_masks(H, W, seed):
    """hand-made edge cases + drawn blobs, uint8 (N,H,W) holding 0 / 255 / other nonzero values (nonzero = set)"""
    rng = np.random.default_rng(seed)
    out = []
    z = lambda: np.zeros((H, W), np.uint8)      # noqa: E731
    out.append(z())                                                  # empty: create_annotation_info returns None
    m = z(); m[:] = 255; out.append(m)                               # full: one run with a leading 0
    m = z(); m[0, 0] = 1; out.append(m)                              # the first pixel alone
    m = z(); m[H - 1, W - 1] = 7; out.append(m)                      # the last pixel alone (the tail bit of the last word)
    m = z(); m[H - 2:, 3] = 255; m[:2, 4] = 255; out.append(m)       # a run that goes on across the column boundary
    m = z(); m[::2, ::2] = 255; m[1::2, 1::2] = 255; out.append(m)   # checkerboard: every pixel a run
    m = z(); m[:, W - 1] = 255; out.append(m)                        # the last column
    m = z(); m[H // 2, :] = 255; out.append(m)                       # one row: W runs of one pixel
    for _ in range(6):
        w, h = int(rng.integers(2, W // 2 + 2)), int(rng.integers(2, H // 2 + 2))
        x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        m = z()
        m[y:y + h, x:x + w] = (rng.random((h, w)) > 0.2) * 255
        m[y, x] = 255
        out.append(m)
    return np.stack(out)


def main():
    rec = {}
    for (H, W) in FRAMES:
        tag = "%dx%d" % (H, W)
        masks = fixture_masks(H, W, seed=H * 1000 + W)
        counts, offsets, boxes, infos, decoded = [], [0], [], [], []
        for n, m in enumerate(masks):
            b = m.astype(bool)
            rle = P.binary_mask_to_rle(b)
            assert rle["size"] == [H, W]
            counts.extend(int(c) for c in rle["counts"])
            offsets.append(len(counts))
            back = P.rle_to_binary_mask(rle)
            decoded.append(np.packbits(back.astype(np.uint8).reshape(-1)))
            box = P.bbox_from_binary_mask(b) if b.any() else [-1, -1, -1, -1]
            boxes.append(box)
            info = P.create_annotation_info(n + 1, 100 + n, 5, b, box, tolerance=2, ignore=bool(n % 3 == 0))
            infos.append(None if info is None else {k: (v if k != "segmentation" else {"counts": [int(c) for c in v["counts"]],
                                                                                      "size": v["size"]}) for k, v in info.items()})
        rec["masks_" + tag] = np.packbits(masks.reshape(len(masks), -1) != 0, axis=1)
        rec["values_" + tag] = np.array([int(m.max()) for m in masks], np.int32)          # the nonzero value each mask was drawn with
        rec["rle_counts_" + tag] = np.asarray(counts, np.int32)
        rec["rle_offsets_" + tag] = np.asarray(offsets, np.int64)
        rec["bbox_" + tag] = np.asarray(boxes, np.int32)
        rec["roundtrip_" + tag] = np.stack(decoded)
        rec["infos_" + tag] = np.array(json.dumps(infos))

    # a three-scene merge: the first scene has images and no annotation (annotation_id_offset = 0 in the second merge)
    def scene(im_ids, anns):
        return {"categories": [{"id": 5, "name": "5", "supercategory": "x"}], "images": [{"id": i} for i in im_ids],
                "annotations": [{"id": a, "image_id": i} for a, i in anns]}
    scenes = [scene([0, 3, 7], []), scene([1, 2, 9], [(1, 1), (2, 1), (3, 9)]), scene([0, 4], [(1, 0), (2, 4), (5, 4)])]
    results = [[{"image_id": 3, "k": 0}], [{"image_id": 9, "k": 1}, {"image_id": 1, "k": 2}], [{"image_id": 4, "k": 3}]]
    rec["merge_scenes"] = np.array(json.dumps({"scenes": scenes, "results": results}))
    s, r = copy.deepcopy(scenes), copy.deepcopy(results)
    ann, res, offs = s[0], r[0], [0]
    for i in (1, 2):
        ann, off = P.merge_coco_annotations(ann, s[i])
        res = P.merge_coco_results(res, r[i], off)
        offs.append(int(off))
    rec["merge_image_ids"] = np.asarray([im["id"] for im in ann["images"]], np.int64)
    rec["merge_ann_ids"] = np.asarray([[a["id"], a["image_id"]] for a in ann["annotations"]], np.int64)
    rec["merge_result_image_ids"] = np.asarray([x["image_id"] for x in res], np.int64)
    rec["merge_offsets"] = np.asarray(offs, np.int64)
    path = os.path.join(HERE, "coco_eval.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
