"""Row N27 restated in numpy: the rule of csrc/paste_masks.hip (predicted masks pasted into the frame), with integer numpy only.

  threshold(plane)              the pinned `sigmoid(z) > 0.5` in fp32: z > 1.5 * 2^-24 (NaN, -0.0 and +0.0 fail)
  paste(plane, window, H, W)    the dense (H,W) uint8 mask of one seg plane and one window (x1, y1, x2, y2, rw, rh)
  area_box(mask)                (area, [xmin, ymin, xmax, ymax]) -- -1s for an empty mask
  rle(mask)                     the column-major run lengths, through tests/coco_stages.binary_mask_to_rle
  pack(mask)                    cp_coco_pack's bit rows (H, ceil(W / 32)) as int32

The tamperings (`rule=`) are the mistakes the rule excludes; tests/test_paste_masks.py shows that each is caught by a named case."""
import struct

import numpy as np

from tests import coco_stages as CS

Z0 = np.float32(struct.unpack("<f", struct.pack("<I", 0x33C00000))[0])       # include/checkerpose_hip.h CP_SIGMOID_HALF_Z0_BITS


def threshold(plane, rule="pinned"):
    z = np.asarray(plane, np.float32)
    with np.errstate(invalid="ignore"):
        return (z >= Z0) if rule == "ge" else (z > Z0)


def cells(lo, hi, start, S, r, rule="centre"):
    """the cell of every frame coordinate in [lo, hi) of a window axis that starts at `start` with roi size r: integer division"""
    off = np.arange(lo, hi, dtype=np.int64) - np.int64(start)
    if rule == "left_edge":                                # cv2.INTER_NEAREST: floor(rx S / r)
        return (off * np.int64(S)) // np.int64(r)
    return ((2 * off + 1) * np.int64(S)) // (2 * np.int64(r))


def extent(start, end, size, r, rule="centre"):
    """[lo, hi) of a window axis: where the crop read a real pixel"""
    lo = max(int(start), 0)
    hi = min(int(end), int(size)) if rule == "x2_only" else min(int(end), int(size), int(start) + int(r))
    return lo, max(hi, lo)


def paste(plane, window, H, W, rule="centre"):
    """rule: "centre" (THE rule); tamperings: "left_edge", "x2_only", "ge", "swapped" (cx and cy exchanged)"""
    x1, y1, x2, y2, rw, rh = (int(v) for v in window)
    out = np.zeros((H, W), np.uint8)
    if rw <= 0 or rh <= 0:
        return out
    ext = "x2_only" if rule == "x2_only" else "centre"
    lx, hx = extent(x1, x2, W, rw, ext)
    ly, hy = extent(y1, y2, H, rh, ext)
    if hx <= lx or hy <= ly:
        return out
    on = threshold(plane, "ge" if rule == "ge" else "pinned")
    Sh, Sw = on.shape
    cell = "left_edge" if rule == "left_edge" else "centre"
    cx, cy = cells(lx, hx, x1, Sw, rw, cell), cells(ly, hy, y1, Sh, rh, cell)
    if rule == "x2_only":                                  # the tampered extent reaches past the roi: the last cell goes on
        cx, cy = np.minimum(cx, Sw - 1), np.minimum(cy, Sh - 1)
    if rule == "swapped":
        cx, cy = np.minimum(cells(lx, hx, x1, Sh, rw), Sw - 1), np.minimum(cells(ly, hy, y1, Sw, rh), Sh - 1)
    out[ly:hy, lx:hx] = on[np.ix_(cy, cx)]
    return out


def area_box(mask):
    ys, xs = np.nonzero(np.asarray(mask))
    if len(xs) == 0:
        return 0, [-1, -1, -1, -1]
    return int(len(xs)), [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def rle(mask, order="F"):
    """binary_mask_to_rle's counts; order="C" is the tampering (a row-major ravel)"""
    m = np.asarray(mask)
    if order == "C":                                       # (an array whose column-major ravel is m's row-major one)
        return CS.binary_mask_to_rle(m.ravel(order="C").reshape(m.shape, order="F"))["counts"]
    return CS.binary_mask_to_rle(m)["counts"]


def pack(mask):
    m = np.asarray(mask) != 0
    H, W = m.shape
    WW = (W + 31) // 32
    padded = np.zeros((H, WW * 32), np.uint64)
    padded[:, :W] = m
    words = (padded.reshape(H, WW, 32) << np.arange(32, dtype=np.uint64)).sum(2)
    return words.astype(np.uint32).view(np.int32)
