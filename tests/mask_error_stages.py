"""Row N12 (BOP's cus / cou_bb_proj / cou_mask / cou_bb), the stages the device is pinned by.  Nothing here reads the reference;
everything is numpy and Python numbers.

  counts_of, box_of      the four counts (inter, union, n_est, n_gt) and the box (x, y, xmax - xmin, ymax - ymin) of a mask
  cou, cou_box           pose_error.cou_mask / cus after the masks, and 1 - misc.iou, restated; their mutations for the checker's own test
  layers                 a fixture case's six bit-packed masks: est, gt, est possibly / surely set, gt possibly / surely set
  count_interval, ...    what the undecided pixels (possibly but not surely set) of both renders allow"""
import numpy as np

from tests import vsd_stages as S
from tests.common import golden

_CACHE = {}


def fixture():
    """(golden arrays, {mesh name: (verts, faces)}) -- built once, never modified; "hull" takes its faces from vsd.npz"""
    if "g" not in _CACHE:
        _CACHE["g"] = (golden("mask_error"), S.meshes(golden("vsd")["hull_faces"].astype(np.int32)))
    return _CACHE["g"]


def world_b():
    """stage B of the fixture: the drawn world of tests/golden/make_golden_bop_eval.py with what eval_calc_errors.py --error_type=cus
    and eval_calc_scores.py saved on it ("cus_*"), as tests/bop_eval_stages.py's functions read it"""
    if "b" not in _CACHE:
        g, _ = fixture()
        _CACHE["b"] = {k[2:]: g[k] for k in g.files if k.startswith("b_")}
    return _CACHE["b"]


def case(name):
    g, _ = fixture()
    return [str(n) for n in g["names"]].index(name)


def layers(c):
    """(6, H, W) bool of fixture case c: est, gt, est possibly set, est surely set, gt possibly set, gt surely set"""
    if ("bits", c) not in _CACHE:
        g, _ = fixture()
        H, W = int(g["H"][c]), int(g["W"][c])
        _CACHE[("bits", c)] = np.unpackbits(g["bits_%d" % c], axis=1)[:, :H * W].reshape(6, H, W).astype(bool)
    return _CACHE[("bits", c)]


def counts_of(me, mg, one_side=False):
    me, mg = np.asarray(me).astype(bool), np.asarray(mg).astype(bool)
    return [int((me & mg).sum()), int(mg.sum()) if one_side else int((me | mg).sum()), int(me.sum()), int(mg.sum())]


def cou(counts, empty=1.0):
    """1 - inter / float(union); `empty` when the union is empty (the reference: 1.0)"""
    return 1.0 - counts[0] / float(counts[1]) if counts[1] > 0 else empty


def box_of(mask, plus_one=False, clip=None):
    """misc.calc_2d_bbox(xs, ys) of a mask's pixels, None when it has none.  plus_one / clip=(W, H): mutations"""
    ys, xs = np.asarray(mask).nonzero()
    if not xs.size:
        return None
    x0, y0, x1, y1 = int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())
    return clip_box([x0, y0, x1 - x0 + int(plus_one), y1 - y0 + int(plus_one)], clip)


def clip_box(b, size):
    """a box with both corners clipped into the frame, as calc_2d_bbox(clip=True) would (a mutation); size None: unchanged"""
    if size is None:
        return list(b)
    cx = lambda v, n: min(max(v, 0), n - 1)                  # noqa: E731
    x0, y0, x1, y1 = cx(b[0], size[0]), cx(b[1], size[1]), cx(b[0] + b[2], size[0]), cx(b[1] + b[3], size[1])
    return [x0, y0, x1 - x0, y1 - y0]


def cou_box(a, b, or_equal=False):
    """1 - misc.iou(a, b), boxes x, y, w, h; NaN when either is None (the reference's cou_bb_proj raises).  or_equal: the mutation
    `>=` in `w_inter > 0 and h_inter > 0` (0 / 0 then gives NaN)"""
    if a is None or b is None:
        return float("nan")
    tl = max(a[0], b[0]), max(a[1], b[1])
    br = min(a[0] + a[2], b[0] + b[2]), min(a[1] + a[3], b[1] + b[3])
    w, h = br[0] - tl[0], br[1] - tl[1]
    iou = 0.0
    if (w >= 0 and h >= 0) if or_equal else (w > 0 and h > 0):
        inter = w * h
        den = float(a[2] * a[3] + b[2] * b[3] - inter)
        iou = inter / den if den != 0 else float("nan")
    return 1.0 - iou


def same(a, b):
    """float equality with NaN == NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.array_equal(a, b, equal_nan=True))


# ---- what the undecided pixels allow ---------------------------------------------------------------------------------------------------
def count_interval(c):
    """(low, high) of inter, union, n_est, n_gt over every pair of masks between the surely-set and the possibly-set ones"""
    _, _, e_lo, e_hi, g_lo, g_hi = layers(c)          # *_lo = possibly set (dilated), *_hi = surely set (eroded)
    low = [int((e_hi & g_hi).sum()), int((e_hi | g_hi).sum()), int(e_hi.sum()), int(g_hi.sum())]
    high = [int((e_lo & g_lo).sum()), int((e_lo | g_lo).sum()), int(e_lo.sum()), int(g_lo.sum())]
    return low, high


def cus_interval(c):
    """cus is monotone in both counts: between the quotients of the interval's ends"""
    low, high = count_interval(c)
    return cou([high[0], max(low[1], 1)]) if high[1] > 0 else 1.0, cou([low[0], high[1]]) if high[1] > 0 else 1.0


def box_interval(c, side):
    """(inner, outer) boxes as xmin ymin xmax ymax of side 0 / 1: of the surely-set and of the possibly-set pixels (None: no pixel)"""
    lo, hi = layers(c)[2 + 2 * side], layers(c)[3 + 2 * side]
    f = lambda m: None if not m.any() else [int(m.nonzero()[1].min()), int(m.nonzero()[0].min()), int(m.nonzero()[1].max()), int(m.nonzero()[0].max())]   # noqa: E731
    return f(hi), f(lo)


def box_within(box, inner, outer):
    """box x, y, w, h (or -1s = empty) lies between the inner and the outer box"""
    if box[0] == -1 and box[2] == -1:
        return inner is None
    if outer is None:
        return False
    x0, y0, x1, y1 = box[0], box[1], box[0] + box[2], box[1] + box[3]
    ok = outer[0] <= x0 and outer[1] <= y0 and x1 <= outer[2] and y1 <= outer[3]
    if inner is not None:
        ok = ok and x0 <= inner[0] and y0 <= inner[1] and x1 >= inner[2] and y1 >= inner[3]
    return ok


def cou_bb_proj_interval(c):
    """the smallest and largest 1 - iou over every pair of boxes between the inner and outer ones (each coordinate moves over a few
    pixels at most: enumerated).  (nan, nan) when a side can be empty."""
    import itertools
    rng = []
    for side in (0, 1):
        inner, outer = box_interval(c, side)
        if outer is None or inner is None:
            return float("nan"), float("nan")
        rng.append([range(outer[0], inner[0] + 1), range(outer[1], inner[1] + 1), range(inner[2], outer[2] + 1), range(inner[3], outer[3] + 1)])
    vals = []
    for a in itertools.product(*rng[0]):
        for b in itertools.product(*rng[1]):
            vals.append(cou_box([a[0], a[1], a[2] - a[0], a[3] - a[1]], [b[0], b[1], b[2] - b[0], b[3] - b[1]]))
    return min(vals), max(vals)
