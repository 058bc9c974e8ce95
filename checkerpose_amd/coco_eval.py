"""BOP'22 COCO detection / segmentation scores on the device (row N15; csrc/coco_eval.hip).

bop_toolkit's scripts/calc_gt_coco.py, scripts/eval_bop22_coco.py and bop_toolkit_lib/pycoco_utils.py, with pycocotools'
COCOeval.evaluate / accumulate / summarize as the script drives them, for masks and boxes that are resident on the device:

  annotate_masks(...)       area, box and (optionally) the column-major RLE of N masks
  unpack_masks(...)         PackedMasks back to dense uint8 masks, for callers who want a picture
  rle_unpack / rle_stats    row N29 (csrc/rle_unpack.hip): run lists on the device -> PackedMasks / area, box and status alone
  rle_flatten / pack_rles   RLE dicts (lists or compressed strings: rle_from_string / rle_to_string) -> run lists -> PackedMasks
  segmentation_results(...) row N27: the network's seg logits + the crops' boxes -> the BOP'22 result dicts (postprocess.paste_masks_rle)
  calc_gt_coco(...)         the `images` / `annotations` lists of scene_gt_coco.json (ids, skips, ignore flags, RLE dicts)
  mask_ious / box_ious      IoU of listed (detection, ground truth) pairs, float64
  CocoSet                   the ground truth of an evaluation, built from arrays
  evaluate(...)             AP, AP50, AP75, AP_small/medium/large, AR1/10/100, AR_small/medium/large + the precision / recall tables
  eval_bop22_coco(...)      the dict-level twin of eval_bop22_coco.py's loop (target filter, scene merge, average_time_per_image)
  check_coco_results / save_coco_results    inout.py's

Masks, IoUs, matching and the precision / recall tables are computed on the device; the index plan (which detection belongs to which
(image, category) group, the score orders) is a few integers per detection and is made on the host with numpy, and the last step --
twelve means over the downloaded tables -- is numpy's, as in the reference.  There is no CPU fallback."""
import json

import numpy as np
import torch

from . import _abi, scene

T, R, A, M, KEEP = 10, 101, 4, 3, 100
MAX_DETS = (1, 10, 100)
AREA_RNG = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))
STAT_NAMES = ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR1", "AR10", "AR100", "AR_small", "AR_medium", "AR_large")


def iou_thrs():
    return np.linspace(.5, .95, 10)


def rec_thrs():
    return np.linspace(0, 1, 101)


def _as_masks(masks, dev=None):
    m = masks if torch.is_tensor(masks) else torch.as_tensor(np.asarray(masks))
    if dev is not None:
        m = m.to(dev)
    scene.require_cuda("coco_eval", m)
    if m.dim() == 2:
        m = m[None]
    if m.dim() != 3 or 0 in m.shape:
        raise ValueError("masks must be (N,H,W) with N, H, W >= 1, got %r" % (tuple(m.shape),))
    if m.dtype == torch.bool:
        m = m.to(torch.uint8)
    elif m.dtype != torch.uint8:
        m = (m != 0).to(torch.uint8)
    return m.contiguous()


class PackedMasks:
    """N masks of one frame size as bit rows on the device: bits (N,H,WW) int32 words, area (N) int32, box (N,4) int32 =
    xmin ymin xmax ymax (-1s for an empty mask)"""

    def __init__(self, bits, area, box, H, W):
        self.bits, self.area, self.box, self.H, self.W = bits, area, box, H, W

    def __len__(self):
        return int(self.area.shape[0])

    @property
    def device(self):
        return self.bits.device


def pack_masks(masks, device=None):
    """cp_coco_pack: (N,H,W) bool / uint8 masks (nonzero = set; a host array goes to `device` first) -> PackedMasks"""
    if isinstance(masks, PackedMasks):
        return masks
    m = _as_masks(masks, device)
    N, H, W = (int(v) for v in m.shape)
    dev = m.device
    bits = torch.empty((N, H, (W + 31) // 32), dtype=torch.int32, device=dev)
    area = torch.empty((N,), dtype=torch.int32, device=dev)
    box = torch.empty((N, 4), dtype=torch.int32, device=dev)
    _abi.call("cp_coco_pack", dev, m, N, H, W, bits, area, box)
    return PackedMasks(bits, area, box, H, W)


def unpack_masks(packed):
    """cp_coco_unpack, pack_masks' inverse: PackedMasks -> (N,H,W) uint8 CUDA tensor of 0 / 1"""
    N, dev = len(packed), packed.device
    scene.require_cuda("coco_eval", packed.bits)
    out = torch.empty((N, packed.H, packed.W), dtype=torch.uint8, device=dev)
    if N:
        _abi.call("cp_coco_unpack", dev, packed.bits, N, packed.H, packed.W, out)
    return out


def rle_encode(packed):
    """pycoco_utils.binary_mask_to_rle of every packed mask -> (counts int32 (total,), offsets int64 (N + 1,)) on the device: mask n's
    run lengths are counts[offsets[n]:offsets[n + 1]]"""
    N, dev = len(packed), packed.device
    n_runs = torch.empty((N,), dtype=torch.int32, device=dev)
    _abi.call("cp_coco_rle_count", dev, packed.bits, N, packed.H, packed.W, n_runs)
    offsets = torch.zeros((N + 1,), dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(n_runs, 0)
    total = int(offsets[-1])
    counts = torch.empty((total,), dtype=torch.int32, device=dev)
    _abi.call("cp_coco_rle_write", dev, packed.bits, N, packed.H, packed.W, offsets, counts, total)
    return counts, offsets


def rle_dicts(counts, offsets, H, W, compress=False):
    """the device RLE as pycoco_utils' dicts: [{"counts": [...], "size": [H, W]}, ...] (host); with compress the counts are
    pycocotools' compressed strings (rle_to_string), as cocoapi writers emit them"""
    c, o = counts.cpu().numpy(), offsets.cpu().numpy()
    enc = rle_to_string if compress else (lambda run: [int(v) for v in run])
    return [{"counts": enc(c[o[n]:o[n + 1]]), "size": [int(H), int(W)]} for n in range(len(o) - 1)]


RLE_STATUS = {1: "a negative count", 2: "the counts sum to more than H * W", 3: "the offsets do not fit the counts"}


def _rle_args(counts, offsets, H, W):
    scene.require_cuda("coco_eval", counts, offsets)
    if counts.dtype != torch.int32 or offsets.dtype != torch.int64 or counts.dim() != 1 or offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("counts must be int32 (total,) and offsets int64 (N + 1,), as rle_encode makes them")
    if counts.device != offsets.device:
        raise ValueError("counts are on %s, offsets on %s" % (counts.device, offsets.device))
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("the frame must be at least 1 x 1, got %d x %d" % (H, W))
    return counts.contiguous(), offsets.contiguous(), int(offsets.numel()) - 1, H, W


def _rle_unpack(counts, offsets, H, W, with_bits):
    counts, offsets, N, H, W = _rle_args(counts, offsets, H, W)
    dev = counts.device
    bits = torch.empty((N, H, (W + 31) // 32), dtype=torch.int32, device=dev) if with_bits else None
    area = torch.empty((N,), dtype=torch.int32, device=dev)
    box = torch.empty((N, 4), dtype=torch.int32, device=dev)
    status = torch.empty((N,), dtype=torch.int32, device=dev)
    if N:
        total = int(counts.numel())
        ends = torch.empty((total,), dtype=torch.int32, device=dev)      # cp_coco_rle_unpack_scratch_bytes(total) = 4 * total
        nz = lambda t: t if t.numel() else None      # noqa: E731
        _abi.call("cp_coco_rle_unpack", dev, nz(counts), offsets, N, H, W, total, nz(ends), bits, area, box, status)
    return bits, area, box, status, H, W


def _check_rle_status(status, H, W, first=0):
    """ValueError naming the first mask with a nonzero status (one host read of N integers); `first`: the index of mask 0 in the
    caller's list"""
    st = status.cpu().numpy()
    bad = np.nonzero(st)[0]
    if len(bad):
        raise ValueError("mask %d: RLE counts do not fit %dx%d (%s)" % (first + bad[0], H, W, RLE_STATUS.get(int(st[bad[0]]), "?")))


def rle_unpack(counts, offsets, H, W, check=True, return_status=False):
    """cp_coco_rle_unpack, rle_encode's inverse and pycoco_utils.rle_to_binary_mask on the device: counts int32 (total,), offsets int64
    (N + 1,) CUDA tensors (rle_encode's / postprocess.paste_masks_rle's layout) of H x W masks -> PackedMasks; no dense mask exists on
    either side.  Zero-length runs are taken anywhere, a list that sums to less than H * W leaves the rest background.  A mask whose
    list holds a negative count (status 1), sums to more than H * W (2) or whose offsets do not fit the counts (3) comes out empty;
    with check (one host read of N integers) the first such mask raises ValueError instead.  With return_status -> (PackedMasks,
    status int32 (N,))."""
    bits, area, box, status, H, W = _rle_unpack(counts, offsets, H, W, True)
    if check:
        _check_rle_status(status, H, W)
    packed = PackedMasks(bits, area, box, H, W)
    return (packed, status) if return_status else packed


def rle_stats(counts, offsets, H, W):
    """area int32 (N,), box int32 (N,4) xmin ymin xmax ymax and status int32 (N,) of device run lists, from the runs alone (the same
    entry point without its bits launch): the annotation info of an RLE without decoding it.  A mask with a nonzero status (see
    rle_unpack) has area 0 and a box of -1s."""
    _, area, box, status, _, _ = _rle_unpack(counts, offsets, H, W, False)
    return area, box, status


def rle_from_string(s):
    """pycocotools' rleFrString: the compressed `counts` string of an RLE -> its run lengths (list of int; host).  Each character
    minus 48 carries 5 payload bits, least significant group first; bit 0x20 says that more follow; on a value's last character bit
    0x10 extends the sign.  From the fourth value on a value is stored as its difference against the value two places back."""
    if isinstance(s, str):
        s = s.encode("ascii")
    counts, p, n = [], 0, len(s)
    while p < n:
        x, k, more = 0, 0, True
        while more:
            if p >= n:
                raise ValueError("the compressed RLE string ends inside a value")
            c = s[p] - 48
            if not 0 <= c < 64:
                raise ValueError("character %r is not part of a compressed RLE string" % (chr(s[p]),))
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_to_string(counts):
    """pycocotools' rleToString, rle_from_string's inverse: run lengths -> the compressed `counts` string (str; host)"""
    counts = [int(v) for v in counts]
    out = []
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(c + 48)
    return bytes(out).decode("ascii")


def rle_flatten(rles):
    """a list of RLE dicts of one size -> (counts int32 (total,), offsets int64 (N + 1,), (H, W)) numpy arrays in rle_encode's layout
    (host).  A `counts` that is a str or bytes is a compressed string (rle_from_string).  Negative counts pass (the decoder names
    them); counts outside int32 raise ValueError."""
    if not rles:
        return np.zeros(0, np.int32), np.zeros(1, np.int64), (1, 1)
    H, W = (int(v) for v in rles[0]["size"])
    runs = []
    for rle in rles:
        if [int(v) for v in rle["size"]] != [H, W]:
            raise ValueError("every RLE must have size %r, got %r" % ([H, W], rle["size"]))
        c = rle["counts"]
        try:
            a = np.asarray(rle_from_string(c) if isinstance(c, (str, bytes)) else c, np.int64).reshape(-1)
        except OverflowError:
            a = None
        if a is None or (a.size and (a.max() > 2 ** 31 - 1 or a.min() < -2 ** 31)):
            raise ValueError("RLE counts do not fit int32")
        runs.append(a)
    offsets = np.zeros(len(runs) + 1, np.int64)
    np.cumsum([len(a) for a in runs], out=offsets[1:])
    return np.concatenate(runs).astype(np.int32), offsets, (H, W)


def annotate_masks(masks, return_rle=False, device=None):
    """area, box and RLE of resident masks.  masks: (N,H,W) CUDA tensor, bool or uint8 (nonzero = set, as the reference's astype(bool)).
    -> dict of CUDA tensors: "area" int32 (N,), "box" int32 (N,4) xmin ymin xmax ymax, "bbox" int32 (N,4) =
    pycoco_utils.bbox_from_binary_mask's x y w h (w = xmax - xmin + 1), all -1 for an empty mask (the reference raises there);
    "packed": the PackedMasks (mask_ious / CocoSet take it);  with return_rle "rle_counts" / "rle_offsets" (rle_encode) and "rle",
    the host list of RLE dicts."""
    p = pack_masks(masks, device)
    box = p.box
    out = {"area": p.area, "box": box, "bbox": _xywh(p.area, box), "packed": p}
    if return_rle:
        out["rle_counts"], out["rle_offsets"] = rle_encode(p)
        out["rle"] = rle_dicts(out["rle_counts"], out["rle_offsets"], p.H, p.W)
    return out


def _xywh(area, box):
    """pycoco_utils.bbox_from_binary_mask's x y w h from xmin ymin xmax ymax (w = xmax - xmin + 1); all -1 for an empty mask"""
    wh = box[:, 2:] - box[:, :2] + 1
    return torch.where((area > 0)[:, None], torch.cat([box[:, :2], wh], 1), torch.full_like(box, -1))


def segmentation_results(seg, Bboxes, frame_size, scene_id, image_id, category_id, score, time=None, resize_method="crop_square_resize",
                         channel=0):
    """The BOP'22 segmentation results of one forward (row N27): the network's `seg` logits (B,C,Sh,Sw) and the crops' padded boxes ->
    the host list of result dicts that check_coco_results / eval_bop22_coco / save_coco_results read: scene_id, image_id, category_id,
    score, bbox [x, y, w, h] of the pasted mask, segmentation {"counts", "size": [H, W]} and, when given, time.  Built from
    postprocess.paste_masks_rle (its arguments): no dense mask exists on either side.  scene_id, image_id, category_id, score, time:
    a value for all detections or one per detection.  A detection whose mask is empty is KEPT, with bbox [-1, -1, -1, -1]
    (annotate_masks' convention): dropping it would change the false-positive count."""
    from . import postprocess
    counts, offsets, area, box = postprocess.paste_masks_rle(seg, Bboxes, frame_size, resize_method, channel)
    B = int(area.shape[0])
    H, W = (int(v) for v in frame_size)
    rles = rle_dicts(counts, offsets, H, W)
    bbox = _xywh(area, box).cpu().numpy()

    def per_det(v, name):
        a = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v).reshape(-1)
        if a.shape[0] not in (1, B):
            raise ValueError("%s must be one value or one per detection (%d), got %d" % (name, B, a.shape[0]))
        return np.broadcast_to(a, (B,))
    cols = [per_det(v, k) for k, v in (("scene_id", scene_id), ("image_id", image_id), ("category_id", category_id), ("score", score))]
    times = None if time is None else per_det(time, "time")
    out = []
    for b in range(B):
        row = {"scene_id": int(cols[0][b]), "image_id": int(cols[1][b]), "category_id": int(cols[2][b]), "score": float(cols[3][b]),
               "bbox": [int(v) for v in bbox[b]], "segmentation": rles[b]}
        if times is not None:
            row["time"] = float(times[b])
        out.append(row)
    return out


def calc_gt_coco(scene_gt, scene_gt_info, masks_visib, masks_full=None, bbox_type="amodal", im_size=None, device="cuda:0"):
    """scripts/calc_gt_coco.py:84-121 for one scene.
      scene_gt: {im_id: [{"obj_id", ...}, ...]}, scene_gt_info: {im_id: [{"visib_fract", ...}, ...]} as bop_toolkit loads them;
      masks: EITHER masks_visib = {(im_id, gt_id): (mask, mask_visib)}, gt_info.scene_gt_info(..., return_masks=True)'s second
      result, OR masks_visib / masks_full as (N,H,W) arrays / CUDA tensors with one row per ground truth in scene_gt's iteration order.
    -> {"images": [{"id", "width", "height"}], "annotations": [...]} with the reference's annotation dicts (id, image_id, category_id,
    iscrowd, area, bbox, segmentation = RLE, width, height, ignore): segmentation_id starts at 1 and advances for every instance that
    passes the skip rule (visible mask empty; with 'amodal' also the full mask empty).  The wall-clock fields (date_captured, INFO),
    file names and categories are the caller's to add."""
    if bbox_type not in ("amodal", "modal"):
        raise ValueError("%s is not a valid bounding box type" % (bbox_type,))
    rows = [(im_id, gt_id, inst) for im_id, insts in scene_gt.items() for gt_id, inst in enumerate(insts)]      # keys as the caller has them
    images = [{"id": int(im_id)} for im_id in scene_gt.keys()]
    if isinstance(masks_visib, dict):
        pairs = [masks_visib[(im_id, gt_id)] for im_id, gt_id, _ in rows]
        full = [p[0] for p in pairs]
        visib = [p[1] for p in pairs]
        stack = (lambda xs: torch.stack(list(xs))) if rows and torch.is_tensor(full[0]) else (lambda xs: np.stack(list(xs)))
        masks_full, masks_visib = (stack(full), stack(visib)) if rows else (None, None)
    if not rows:
        return {"images": images, "annotations": []}
    if masks_full is None and bbox_type == "amodal":
        raise ValueError("bbox_type 'amodal' takes the box from the full mask: pass masks_full")
    dev = masks_visib.device if torch.is_tensor(masks_visib) and masks_visib.is_cuda else torch.device(device)
    vis = annotate_masks(masks_visib, return_rle=True, device=dev)
    if len(vis["packed"]) != len(rows):
        raise ValueError("%d masks for %d ground truths" % (len(vis["packed"]), len(rows)))
    H, W = vis["packed"].H, vis["packed"].W
    for im in images:
        im["width"], im["height"] = (W, H) if im_size is None else (int(im_size[0]), int(im_size[1]))
    src = vis
    if bbox_type == "amodal":
        src = annotate_masks(masks_full, device=dev)
        if len(src["packed"]) != len(rows):
            raise ValueError("%d full masks for %d ground truths" % (len(src["packed"]), len(rows)))
    area, bbox, box_area = vis["area"].cpu().numpy(), src["bbox"].cpu().numpy(), src["area"].cpu().numpy()
    annotations, segmentation_id = [], 1
    for j, (im_id, gt_id, inst) in enumerate(rows):
        if area[j] < 1 or (bbox_type == "amodal" and box_area[j] < 1):
            continue
        ignore_gt = bool(scene_gt_info[im_id][gt_id]["visib_fract"] < 0.1)
        annotations.append({"id": segmentation_id, "image_id": int(im_id), "category_id": inst["obj_id"], "iscrowd": 0, "area": int(area[j]),
                            "bbox": [int(v) for v in bbox[j]], "segmentation": vis["rle"][j], "width": W, "height": H,
                            "ignore": ignore_gt})
        segmentation_id += 1
    return {"images": images, "annotations": annotations}


def _pairs(pairs, dev):
    p = torch.as_tensor(pairs).to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
    return p, int(p.shape[0])


def mask_ious(dets, gts, pairs):
    """IoU of the listed pairs of masks (cp_coco_mask_iou): dets, gts: PackedMasks (or (N,H,W) CUDA masks) of one frame size; pairs
    (P,2) = (detection index, ground-truth index).  -> (P,) float64 CUDA tensor: 0.0 when the intersection is empty, else
    inter / union as one float64 quotient."""
    d = pack_masks(dets)
    g = pack_masks(gts, d.device)
    if (d.H, d.W) != (g.H, g.W):
        raise ValueError("detections are %dx%d, ground truth %dx%d" % (d.H, d.W, g.H, g.W))
    dev = d.device
    p, P = _pairs(pairs, dev)
    out = torch.empty((P,), dtype=torch.float64, device=dev)
    if P == 0:
        return out
    _abi.call("cp_coco_mask_iou", dev, d.bits, d.area, d.box, len(d), g.bits, g.area, g.box, len(g), d.H, d.W, p, P, out)
    return out


def _boxes(b, dev=None):
    t = torch.as_tensor(b)
    t = t.to(device=dev if dev is not None else t.device, dtype=torch.float64).reshape(-1, 4).contiguous()
    scene.require_cuda("coco_eval", t)
    return t


def box_ious(dets, gts, pairs):
    """maskApi's bbIou of the listed pairs (cp_coco_box_iou): dets (ND,4) CUDA tensor x y w h, gts (NG,4); computed in float64.
    -> (P,) float64 CUDA tensor"""
    d = _boxes(dets)
    g = _boxes(gts, d.device)
    dev = d.device
    p, P = _pairs(pairs, dev)
    out = torch.empty((P,), dtype=torch.float64, device=dev)
    if P == 0:
        return out
    _abi.call("cp_coco_box_iou", dev, d, int(d.shape[0]), g, int(g.shape[0]), p, P, out)
    return out


def _host(x, dtype):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=dtype)


class CocoSet:
    """The ground truth of an evaluation, from arrays (what COCO(dataset_coco_ann) holds).
      image_ids: every image of the set (also those without annotations); category_ids: the `categories` ids -- evaluation is per
      category, sorted; image_id, category_id, area, ignore (N,): per annotation -- area is the annotation's `area` (BOP: the visible
      mask's count, also for boxes); iscrowd must be 0 (crowd IoU is out of scope);  masks: (N,H,W) CUDA masks or PackedMasks ('segm')
      and / or bbox (N,4) x y w h ('bbox').
      stock_ignore: False (default) is the cocoapi fork BOP installs, where a ground truth is ignored when its `ignore` flag OR iscrowd
      is set; True is stock pycocotools, which overwrites the flag with iscrowd -- with iscrowd = 0 no ground truth is ignored."""

    def __init__(self, image_ids, category_ids, image_id, category_id, area, ignore=None, iscrowd=None, masks=None, bbox=None,
                 stock_ignore=False, device="cuda:0"):
        self.image_ids = np.unique(_host(image_ids, np.int64))
        self.category_ids = np.unique(_host(category_ids, np.int64))
        self.image_id, self.category_id = _host(image_id, np.int64), _host(category_id, np.int64)
        n = len(self.image_id)
        self.area = _host(area, np.float64)
        self.ignore = np.zeros(n, bool) if ignore is None else _host(ignore, np.int64) != 0
        crowd = np.zeros(n, bool) if iscrowd is None else _host(iscrowd, np.int64) != 0
        if crowd.any():
            raise ValueError("iscrowd must be 0: crowd annotations are out of scope")
        if not (len(self.category_id) == len(self.area) == len(self.ignore) == n):
            raise ValueError("image_id, category_id, area and ignore must have one entry per annotation")
        self.stock_ignore = bool(stock_ignore)
        self.device = torch.device(device)
        self.masks = None if masks is None or n == 0 else pack_masks(masks, self.device)
        self.bbox = None if bbox is None or n == 0 else _boxes(bbox, self.device)
        for name, v in (("masks", self.masks), ("bbox", self.bbox)):
            if v is not None and len(v) != n:
                raise ValueError("%s has %d rows for %d annotations" % (name, len(v), n))
        if self.masks is not None:
            self.device = self.masks.device


def make_plan(image_ids, category_ids, g_img, g_cat, d_img, d_cat, d_score):
    """The index plan of an evaluation (host, numpy; a few integers per detection).  Groups are the (category, image) pairs that have a
    ground truth or a detection, ordered by category, then image id.  -> dict:
      gt_sel / det_sel: input rows in plan order (ground truth: by group, input order kept; detections: by group, stable descending
      score, cut to 100 per group);  det_off, gt_off, iou_off (n_groups + 1);  group_cat / group_img: indices into the sorted
      category / image ids;  det_rank;  pairs (P,2) in plan rows, each group's (D,G) matrix row-major;  order: plan rows, each
      category's stretch in stable descending score order;  cat_det_off, cat_gt_off (K + 1)."""
    image_ids, category_ids = np.asarray(image_ids, np.int64), np.asarray(category_ids, np.int64)
    n_img, K = len(image_ids), len(category_ids)

    def keys(img, cat, what, strict):
        img, cat = np.asarray(img, np.int64), np.asarray(cat, np.int64)
        ii = np.searchsorted(image_ids, img).clip(0, max(n_img - 1, 0))
        ci = np.searchsorted(category_ids, cat).clip(0, max(K - 1, 0))
        img_ok = (image_ids[ii] == img) if n_img else np.zeros(len(img), bool)
        cat_ok = (category_ids[ci] == cat) if K else np.zeros(len(cat), bool)
        if strict and not img_ok.all():
            raise ValueError("Results do not correspond to current coco set: %s image ids %r are not in it"
                             % (what, sorted(set(img[~img_ok].tolist()))[:5]))
        keep = np.nonzero(img_ok & cat_ok)[0]
        return keep, ci[keep] * max(n_img, 1) + ii[keep]

    g_keep, g_key = keys(g_img, g_cat, "ground-truth", False)
    d_keep, d_key = keys(d_img, d_cat, "detection", True)
    group_key = np.unique(np.concatenate([g_key, d_key]))
    n_groups = len(group_key)
    g_grp, d_grp = np.searchsorted(group_key, g_key), np.searchsorted(group_key, d_key)
    # (numpy's stable sort of 16-bit keys is a radix sort: the two float sorts below are then what the plan costs)
    small = lambda a, n: a.astype(np.int16) if n < 2 ** 15 else a      # noqa: E731
    g_perm = np.argsort(small(g_grp, n_groups), kind="stable")
    score = np.asarray(d_score, np.float64)[d_keep]
    by_score = np.argsort(-score, kind="stable")
    d_perm = by_score[np.argsort(small(d_grp[by_score], n_groups), kind="stable")]
    first = np.concatenate([[0], np.cumsum(np.bincount(d_grp, minlength=n_groups))])
    rank = np.arange(len(d_perm)) - first[d_grp[d_perm]]
    d_perm = d_perm[rank < KEEP]
    det_grp, gt_grp = d_grp[d_perm], g_grp[g_perm]
    det_off = np.concatenate([[0], np.cumsum(np.bincount(det_grp, minlength=n_groups))])
    gt_off = np.concatenate([[0], np.cumsum(np.bincount(gt_grp, minlength=n_groups))])
    det_rank = np.arange(len(d_perm)) - det_off[det_grp]
    D, G = np.diff(det_off), np.diff(gt_off)
    iou_off = np.concatenate([[0], np.cumsum(D * G)])
    per_det = G[det_grp]
    P = int(per_det.sum())
    row = np.repeat(np.arange(len(d_perm)), per_det)
    col = np.arange(P) - np.repeat(np.cumsum(per_det) - per_det, per_det) + np.repeat(gt_off[det_grp], per_det)
    group_cat, group_img = group_key // max(n_img, 1), group_key % max(n_img, 1)
    cat_grp_off = np.searchsorted(group_cat, np.arange(K + 1))
    plan_score = score[d_perm]
    by_score = np.argsort(-plan_score, kind="stable")
    det_cat = group_cat[det_grp]
    order = by_score[np.argsort(small(det_cat[by_score], K), kind="stable")]
    if max(len(d_perm), len(g_perm), P) >= 2 ** 31:
        raise ValueError("too many detections, ground truths or pairs for 32-bit offsets")
    return {"gt_sel": g_keep[g_perm], "det_sel": d_keep[d_perm], "det_off": det_off, "gt_off": gt_off, "iou_off": iou_off,
            "group_cat": group_cat, "group_img": group_img, "det_rank": det_rank, "pairs": np.stack([row, col], 1).astype(np.int32),
            "order": order, "cat_det_off": det_off[cat_grp_off], "cat_gt_off": gt_off[cat_grp_off], "n_groups": n_groups}


def summarize(precision, recall):
    """COCOeval.summarize's twelve numbers from the tables (numpy, as the reference): the mean of the entries > -1, or -1"""
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


def evaluate(cocoset, dets, ann_type="segm", return_tables=False):
    """COCOeval(cocoGt, cocoGt.loadRes(dets), ann_type).evaluate() / accumulate() / summarize() on the device.
      dets: dict with image_id, category_id, score (N,) and masks ((N,H,W) CUDA masks or PackedMasks; 'segm') or bbox ((N,4) x y w h;
      'bbox').  A detection's area is its mask's count ('segm') or w * h in float64 ('bbox').
    -> dict: the twelve scores (STAT_NAMES), "precision" (10,101,K,4,3) and "recall" (10,K,4,3) float64 host arrays (-1 where a
    category has no unignored ground truth).  With return_tables also "plan" (make_plan's), "ious" (P,), "dt_match" (ND,4,10): index
    of the matched ground truth within its group + 1, "dt_ignore" (ND,4,10), "gt_ignore" (NG,4) as host arrays in plan order."""
    if ann_type not in ("segm", "bbox"):
        raise ValueError("ann_type must be 'segm' or 'bbox', got %r" % (ann_type,))
    cs, dev = cocoset, cocoset.device
    scene.require_cuda("coco_eval", device=dev)
    K = len(cs.category_ids)
    if K == 0:
        raise ValueError("the set has no categories")
    d_img, d_cat, d_score = _host(dets["image_id"], np.int64), _host(dets["category_id"], np.int64), _host(dets["score"], np.float64)
    plan = make_plan(cs.image_ids, cs.category_ids, cs.image_id, cs.category_id, d_img, d_cat, d_score)
    ND, NG, P, n_groups = len(plan["det_sel"]), len(plan["gt_sel"]), len(plan["pairs"]), plan["n_groups"]
    lib = _abi.load()
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))      # noqa: E731
    sel_d, sel_g = torch.from_numpy(plan["det_sel"]).to(dev), torch.from_numpy(plan["gt_sel"]).to(dev)
    pairs = i32(plan["pairs"]).to(dev)
    key = "masks" if ann_type == "segm" else "bbox"
    gt_side = cs.masks if ann_type == "segm" else cs.bbox
    if (NG and gt_side is None) or (ND and dets.get(key) is None):
        raise ValueError("ann_type %r needs %r of the ground truth and of the detections" % (ann_type, key))
    if ann_type == "segm":
        dm = pack_masks(dets["masks"], dev) if ND else None
        det_area = dm.area.to(torch.float64)[sel_d] if ND else torch.empty(0, dtype=torch.float64, device=dev)
        if P:
            ious = mask_ious(dm, gt_side, torch.stack([sel_d[pairs[:, 0].long()], sel_g[pairs[:, 1].long()]], 1))
    else:
        db = _boxes(dets["bbox"], dev) if ND else None
        det_area = (db[:, 2] * db[:, 3])[sel_d] if ND else torch.empty(0, dtype=torch.float64, device=dev)
        if P:
            ious = box_ious(db, gt_side, torch.stack([sel_d[pairs[:, 0].long()], sel_g[pairs[:, 1].long()]], 1))
    if not P:
        ious = torch.empty(0, dtype=torch.float64, device=dev)
    det_area = det_area.contiguous()
    gt_area = torch.from_numpy(cs.area[plan["gt_sel"]]).to(dev)
    flag = np.zeros(NG, np.uint8) if cs.stock_ignore else cs.ignore[plan["gt_sel"]].astype(np.uint8)
    gt_flag = torch.from_numpy(flag).to(dev)
    thrs, recs = torch.from_numpy(iou_thrs()).to(dev), torch.from_numpy(rec_thrs()).to(dev)
    rng = torch.from_numpy(np.asarray(AREA_RNG, np.float64)).to(dev)
    moff_h = i32(np.concatenate([plan["det_off"], plan["gt_off"], plan["iou_off"]]))
    aoff_h = i32(np.concatenate([plan["cat_det_off"], plan["cat_gt_off"]]))
    moff_d, aoff_d = moff_h.to(dev), aoff_h.to(dev)
    dt_match = torch.empty((ND, A, T), dtype=torch.int32, device=dev)
    dt_ignore = torch.empty((ND, A, T), dtype=torch.uint8, device=dev)
    gt_ignore = torch.empty((NG, A), dtype=torch.uint8, device=dev)
    scratch = torch.empty(max(lib.cp_coco_match_scratch_bytes(NG), 1), dtype=torch.uint8, device=dev)
    precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
    rank, order = i32(plan["det_rank"]).to(dev), i32(plan["order"]).to(dev)
    max_dets = i32(np.asarray(MAX_DETS))
    nz = lambda t: t if t.numel() else None      # noqa: E731  (an empty table goes in as a null pointer)
    if n_groups:
        _abi.call("cp_coco_match", dev, nz(ious), moff_h, moff_d, n_groups, ND, NG, P, nz(det_area), nz(gt_area), nz(gt_flag), thrs, rng,
                  nz(dt_match), nz(dt_ignore), nz(gt_ignore), scratch if NG else None)
    _abi.call("cp_coco_accumulate", dev, nz(dt_match), nz(dt_ignore), nz(gt_ignore), nz(rank), nz(order), aoff_h, aoff_d, K, ND, NG,
              max_dets, recs, precision, recall)
    out = {"precision": precision.cpu().numpy(), "recall": recall.cpu().numpy()}
    out.update(summarize(out["precision"], out["recall"]))
    if return_tables:
        out.update({"plan": plan, "ious": ious.cpu().numpy(), "dt_match": dt_match.cpu().numpy(), "dt_ignore": dt_ignore.cpu().numpy(),
                    "gt_ignore": gt_ignore.cpu().numpy()})
    return out


def rle_decode(rles):
    """pycoco_utils.rle_to_binary_mask of a list of RLE dicts of one size, on the host (vectorised numpy) -> (N,H,W) uint8"""
    if not rles:
        return np.zeros((0, 1, 1), np.uint8)
    H, W = (int(v) for v in rles[0]["size"])
    out = np.zeros((len(rles), W, H), np.uint8)
    for n, rle in enumerate(rles):
        if [int(v) for v in rle["size"]] != [H, W]:
            raise ValueError("every RLE must have size %r, got %r" % ([H, W], rle["size"]))
        if isinstance(rle["counts"], (str, bytes)):
            raise ValueError("compressed RLE strings are not supported: pass the uncompressed counts list")
        counts = np.asarray(rle["counts"], np.int64).reshape(-1)
        if (counts < 0).any() or counts.sum() > H * W:
            raise ValueError("RLE counts do not fit %dx%d" % (H, W))
        values = (np.arange(len(counts)) % 2).astype(np.uint8)
        flat = np.repeat(values, counts)
        out[n].reshape(-1)[:len(flat)] = flat
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def concat_packed(parts):
    """several PackedMasks of one frame size as one"""
    sizes = {(p.H, p.W) for p in parts}
    if len(sizes) != 1:
        raise ValueError("masks of %d frame sizes: one set holds one size" % len(sizes))
    (H, W), = sizes
    return PackedMasks(torch.cat([p.bits for p in parts]), torch.cat([p.area for p in parts]), torch.cat([p.box for p in parts]), H, W)


def pack_rles(rles, device, chunk=512):
    """RLE dicts (counts as lists or as pycocotools' compressed strings) -> PackedMasks, `chunk` masks per call: the run lists are
    flattened on the host (rle_flatten), go up in one small upload -- a few KB per mask where the dense mask has H * W bytes -- and are
    decoded on the device (rle_unpack); no dense mask exists on either side.  The same bits, area and box as
    pack_masks(rle_decode(rles)); counts that do not fit the frame raise ValueError as there."""
    dev = torch.device(device)
    scene.require_cuda("coco_eval", device=dev)
    parts = []
    for i in range(0, len(rles), chunk):
        counts, offsets, (H, W) = rle_flatten(rles[i:i + chunk])
        head = offsets.nbytes
        up = torch.from_numpy(np.concatenate([offsets.view(np.uint8), counts.view(np.uint8)])).to(dev)      # offsets first: 8-byte aligned
        packed, status = rle_unpack(up[head:].view(torch.int32), up[:head].view(torch.int64), H, W, check=False, return_status=True)
        _check_rle_status(status, H, W, first=i)
        parts.append(packed)
    return concat_packed(parts)


def merge_scenes(scene_coco_anns, coco_results, targets, ann_type="segm"):
    """What eval_bop22_coco.py:102-139 hands to pycocotools, from dicts.  A result counts when its `bbox` ('bbox') or `segmentation`
    ('segm') is not empty; images, annotations and results of (scene, image) pairs outside `targets` are dropped; then every scene
    after the first has its image ids moved past the largest image id merged so far, and its annotation ids past the largest
    annotation id merged so far (by 0 while no annotation has been merged) -- the shifts of pycoco_utils.merge_coco_annotations /
    merge_coco_results.  The inputs are not modified.
      scene_coco_anns: {scene_id: {"images", "annotations", "categories"}} in the order of the split's scene_ids.
    -> ({"images", "annotations", "categories"}, results)"""
    wanted = {(t["scene_id"], t["im_id"]) for t in targets}
    field = "bbox" if ann_type == "bbox" else "segmentation"
    by_scene = {}
    for r in coco_results:
        if r[field]:
            by_scene.setdefault(r["scene_id"], []).append(r)
    images, annotations, categories, results = [], [], [], []
    for n, (scene_id, ann) in enumerate(scene_coco_anns.items()):
        img_shift = max(im["id"] for im in images) + 1 if n else 0
        ann_shift = max((a["id"] for a in annotations), default=-1) + 1 if n else 0
        images += [dict(im, id=im["id"] + img_shift) for im in ann["images"] if (scene_id, im["id"]) in wanted]
        annotations += [dict(a, id=a["id"] + ann_shift, image_id=a["image_id"] + img_shift) for a in ann["annotations"]
                        if (scene_id, a["image_id"]) in wanted]
        results += [dict(r, image_id=r["image_id"] + img_shift) for r in by_scene.get(scene_id, ()) if (scene_id, r["image_id"]) in wanted]
        categories += [c for c in ann.get("categories", ()) if c not in categories]
    return {"images": images, "annotations": annotations, "categories": categories}, results


def average_time_per_image(coco_results):
    """The script's `average_time_per_image` (eval_bop22_coco.py:156-176): every image counts once, with the time of its first result;
    -1.0 as soon as a result carries a negative time; ValueError when a later result of an image differs from the first by more than
    1 ms.  Results are visited in order, so which of the two endings is met first is the script's."""
    first = {}
    for r in coco_results:
        t = r["time"]
        if t < 0:
            return -1.0
        seen = first.setdefault((r["scene_id"], r["image_id"]), t)
        if abs(seen - t) > 0.001:
            raise ValueError("scene %d, image %d: results carry different run times (%r and %r)" % (r["scene_id"], r["image_id"], seen, t))
    return float(np.mean(list(first.values())))


def eval_bop22_coco(scene_coco_anns, coco_results, targets, ann_type="segm", bbox_type="amodal", scene_coco_anns_modal=None,
                    stock_ignore=False, device="cuda:0"):
    """scripts/eval_bop22_coco.py's loop body on dicts -> the content of scores_bop22_coco_<ann_type>.json: the twelve scores and
    average_time_per_image.  scene_coco_anns: {scene_id: scene_gt_coco dict} in the split's scene order; scene_coco_anns_modal: the
    scene_gt_coco_modal dicts, which the script reads instead when ann_type is 'bbox' and bbox_type is 'modal' (required then).  RLE
    masks (ground truth and results; counts as lists or as pycocotools' compressed strings, which loadRes accepts too) go up as run
    lists 512 masks at a time and are decoded and scored on the device (pack_rles, row N29): no dense mask on either side."""
    if bbox_type not in ("amodal", "modal"):
        raise ValueError("%s is not a valid bounding box type" % (bbox_type,))
    if ann_type == "bbox" and bbox_type == "modal":
        if scene_coco_anns_modal is None:
            raise ValueError("ann_type 'bbox' with bbox_type 'modal' is scored against scene_coco_anns_modal")
        scene_coco_anns = scene_coco_anns_modal
    ann, res = merge_scenes(scene_coco_anns, coco_results, targets, ann_type)
    gts = ann["annotations"]
    segm = ann_type == "segm"
    cs = CocoSet([im["id"] for im in ann["images"]], [c["id"] for c in ann["categories"]], [a["image_id"] for a in gts],
                 [a["category_id"] for a in gts], [a["area"] for a in gts], [a.get("ignore", 0) for a in gts],
                 [a.get("iscrowd", 0) for a in gts], masks=pack_rles([a["segmentation"] for a in gts], device) if segm and gts else None,
                 bbox=np.asarray([a["bbox"] for a in gts], np.float64) if not segm and gts else None, stock_ignore=stock_ignore,
                 device=device)
    dets = {"image_id": [r["image_id"] for r in res], "category_id": [r["category_id"] for r in res], "score": [r["score"] for r in res]}
    if res:
        if segm:
            dets["masks"] = pack_rles([r["segmentation"] for r in res], cs.device)
        else:
            dets["bbox"] = torch.from_numpy(np.asarray([r["bbox"] for r in res], np.float64)).to(cs.device)
    scores = evaluate(cs, dets, ann_type)
    out = {k: scores[k] for k in STAT_NAMES}
    out["average_time_per_image"] = average_time_per_image(coco_results)
    return out


# a 'bop22' result: (key, accepted types, required) -- bool passes as int, as isinstance has it
_RESULT_FIELDS = (("scene_id", int, True), ("image_id", int, True), ("category_id", int, True), ("score", float, True),
                  ("bbox", list, False), ("time", (float, int), False))


def _result_fault(result, ann_type):
    for key, _, required in _RESULT_FIELDS:
        if required and key not in result:
            return "%s key missing" % key
    for key, types, _ in _RESULT_FIELDS:
        if key in result and not isinstance(result[key], types):
            return "%s is %s" % (key, type(result[key]).__name__)
    if ann_type == "segm" and "segmentation" in result:
        seg = result["segmentation"]
        if not isinstance(seg, dict):
            return "segmentation is not an RLE dict"
        if "counts" not in seg or "size" not in seg:
            return "segmentation lacks counts or size"
    return None


def check_coco_results(results, version="bop22", ann_type="segm"):
    """The format check of inout.check_coco_results on a loaded list (or a path to its JSON): the four ids / score present and typed,
    bbox a list and time a number when present, and for 'segm' a segmentation that is a dict with counts and size.  Explicit checks
    (no assert statements: they hold under `python -O` too).  -> (passed, message); other versions pass unchecked, as there."""
    if isinstance(results, str):
        try:
            with open(results) as f:
                results = json.load(f)
        except Exception as e:
            return False, "cannot load the COCO results: %s" % (e,)
    if version == "bop22":
        for n, result in enumerate(results):
            fault = _result_fault(result, ann_type)
            if fault is not None:
                return False, "result %d: %s" % (n, fault)
    return True, "OK"


# BOP's keys of a detection -> the keys of the COCO results file; the optional ones with the value written when absent
_BOP_TO_COCO = (("scene_id", "scene_id"), ("image_id", "im_id"), ("category_id", "obj_id"), ("score", "score"))
_BOP_TO_COCO_OPTIONAL = (("bbox", "bbox", []), ("segmentation", "segmentation", {}), ("time", "run_time", -1))


def coco_results(results, version="bop22"):
    """the list inout.save_coco_results writes: BOP's scene_id / im_id / obj_id / score / bbox (an array) / segmentation / run_time
    renamed to COCO's keys, an absent bbox as [], segmentation as {}, run_time as -1"""
    if version != "bop22":
        raise ValueError("unknown version of BOP detection results: %r" % (version,))
    out = []
    for res in results:
        row = {coco: res[bop] for coco, bop in _BOP_TO_COCO}
        for coco, bop, absent in _BOP_TO_COCO_OPTIONAL:
            row[coco] = type(absent)(absent) if bop not in res else res[bop]
        if "bbox" in res:
            row["bbox"] = np.asarray(res["bbox"]).tolist()
        out.append(row)
    return out


def save_coco_results(path, results, version="bop22"):
    """inout.save_coco_results: coco_results(...) as JSON"""
    out = coco_results(results, version)
    with open(path, "w") as f:
        json.dump(out, f)
