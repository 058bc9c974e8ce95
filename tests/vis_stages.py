"""Row N18 (poses drawn over the photograph), the stages the device is pinned by.  Nothing here reads the reference; everything is numpy.

  compose          the integer restatement of bop_toolkit_lib/visualization.py:90-205 on per-pose frames (m_rgb uint8 (H,W,3), m_depth
                   float32 (H,W)): ren_rgb, ren_depth, the boxes, the boxes layer, the blend.  tests/test_vis_poses.py holds it EQUAL
                   to what the reference's own vis_object_poses saved (tests/golden/vis_poses.npz); tests/test_gpu_vis_poses.py
                   applies it to the device's own per-pose render_rgb frames: the host composition the scene kernel replaces
  depth_diff       the restatement of visualization.py:206-235 with depth_for_vis: the picture, (min, max, mean), ok
  draw_outline     PIL's one-pixel rectangle outline through the inclusive corners (x, y), (x + w, y + h), clipped to the frame

The rule is stated in checkerpose_amd/vis.py's docstring."""
import numpy as np

S = 1.0 - 0.2      # depth_for_vis: valid_end - valid_start


def box_of(m_rgb):
    """x, y, xmax - xmin, ymax - ymin of the pixels where any channel is > 0 (the reference's obj_mask), or -1 four times"""
    ys, xs = np.nonzero((np.asarray(m_rgb) > 0).any(2))
    if ys.size == 0:
        return [-1, -1, -1, -1]
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]


def draw_outline(layer, box, value):
    H, W = layer.shape[:2]
    x0, y0, x1, y1 = box[0], box[1], box[0] + box[2], box[1] + box[3]
    ys, xs = np.mgrid[0:H, 0:W]
    on = (((xs == x0) | (xs == x1)) & (ys >= y0) & (ys <= y1)) | (((ys == y0) | (ys == y1)) & (xs >= x0) & (xs <= x1))
    layer[on] = value
    return layer


def compose(frame, m_rgbs, m_depths, resolve=True, draw_boxes=True, box_color=(0.3, 0.3, 0.3)):
    """one image.  frame uint8 (H,W,3); m_rgbs / m_depths: the poses' frames in drawing order (a pose that is not rendered: all zero)
    -> dict vis, ren_rgb uint8 (H,W,3), ren_depth float32 (H,W), boxes int (n,4)"""
    frame = np.asarray(frame)
    H, W = frame.shape[:2]
    ren_rgb = np.zeros((H, W, 3), dtype=np.int64)
    ren_depth = np.zeros((H, W), dtype=np.float32)
    layer = np.zeros((H, W, 3), dtype=np.int64)
    value = np.array([int(c * 255) for c in box_color], dtype=np.int64)
    boxes = []
    for m_rgb, m_depth in zip(m_rgbs, m_depths):
        m_rgb, m_depth = np.asarray(m_rgb).astype(np.int64), np.asarray(m_depth, dtype=np.float32)
        m = (m_depth != 0) & ((ren_depth == 0) | (m_depth < ren_depth))
        ren_depth[m] = m_depth[m]
        if resolve:
            ren_rgb[m] = m_rgb[m]
        else:
            ren_rgb = np.minimum(255, ren_rgb + m_rgb)
        boxes.append(box_of(m_rgb))
        if draw_boxes and boxes[-1][0] >= 0:
            draw_outline(layer, boxes[-1], value)
    vis = np.minimum(255, (frame.astype(np.int64) + ren_rgb) // 2 + layer)
    return {"vis": vis.astype(np.uint8), "ren_rgb": ren_rgb.astype(np.uint8), "ren_depth": ren_depth,
            "boxes": np.asarray(boxes, dtype=np.int64).reshape(-1, 4)}


def dd_of(ren_depth, depth):
    """(dd float32 with +0 where not valid, valid)"""
    ren_depth, depth = np.asarray(ren_depth, dtype=np.float32), np.asarray(depth, dtype=np.float32)
    valid = (depth > 0) & (ren_depth > 0)
    with np.errstate(invalid="ignore"):
        dd = np.where(valid, ren_depth - depth, np.float32(0)).astype(np.float32)
    return dd + np.float32(0), valid                                 # (-0 + 0 = +0)


def distinct_dd(ren_depth, depth):
    return int(np.unique(dd_of(ren_depth, depth)[0]).size)


def depth_diff(ren_depth, depth, delta=15.0):
    """-> (picture uint8 (H,W,3), stats float64 (3,) = min, max, mean over the valid pixels or NaN, ok)"""
    dd, valid = dd_of(ren_depth, depth)
    H, W = dd.shape
    stats = np.full(3, np.nan)
    if valid.any():
        stats = np.array([float(dd[valid].min()), float(dd[valid].max()), float(dd[valid].astype(np.float64).mean())])
    values = np.unique(dd)
    out = np.zeros((H, W, 3), dtype=np.uint8)
    if values.size < 3:
        return out, stats, 0
    m0 = values[0]
    x = (dd - m0).astype(np.float32)
    mask = x > 0
    x64 = x.astype(np.float64)
    mn = np.float64(np.float32(values[1] - m0))
    mx = np.float64(np.float32(values[-1] - m0)) - mn
    n = np.zeros((H, W))
    n[mask] = (x64[mask] - mn) / (mx / S) + 0.2
    gb = (255 * n).astype(np.uint8)
    out[..., 0] = np.where(valid & (dd < np.float32(delta)), 255, 0)
    out[..., 1] = gb
    out[..., 2] = gb
    out[~valid] = 0
    return out, stats, 1
