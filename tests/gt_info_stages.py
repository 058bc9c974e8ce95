"""Row N10 (BOP ground-truth info and masks), the stages the device is pinned by.  Nothing here reads the reference; everything is
numpy.  The float64 oracle rasteriser, its bounds and the meshes are tests/vsd_stages.py's, unchanged.

  canvas_K / oracle_canvas   the reference's 3W x 3H canvas: the principal point moved by (W, H); the oracle rendered on it
  frame_of                   the in-frame part of a canvas image
  count                      calc_gt_info.py:115-175 and calc_gt_masks.py:106-127 after the render, restated; its mutations for
                             the checker's own test
  intervals                  what the undecided pixels of the oracle allow: per count an interval, per box an inner and an outer
                             box, per mask the pixels that are decided
  check_against_intervals    a result (counts, boxes, masks) against them
  pack / unpack              the fixture's bit-packed masks

A canvas pixel is UNDECIDED when the oracle's dilated and eroded renders disagree there by more than tol_d (vsd_stages'
docstring); a frame pixel's visibility is undecided too when f32(dist_gt) - f32(dist_im) comes within the render's tolerance of
delta (the margin of vsd_stages.count_interval)."""
import numpy as np

from tests import vsd_stages as S

MUTATIONS = ("bop18", "all_on_frame", "valid_on_canvas", "gate_on_all", "plus_one", "clip_obj", "diff64")
INFO_KEYS = ("px_count_all", "px_count_valid", "px_count_visib", "visib_fract", "bbox_obj", "bbox_visib")


def canvas_K(K, size):
    K = np.array(K, dtype=np.float64).reshape(3, 3)
    K[0, 2] += size[0]
    K[1, 2] += size[1]
    return K


def oracle_canvas(R, t, K, verts, faces, size):
    """vsd_stages.oracle_render on the (3W, 3H) canvas; canvas pixel [y + H, x + W] is frame pixel (x, y)"""
    return S.oracle_render(R, t, canvas_K(K, size), verts, faces, (3 * size[0], 3 * size[1]))


def frame_of(canvas, size):
    W, H = size
    return canvas[H:2 * H, W:2 * W]


def _bbox(mask, off=(0, 0), plus_one=False):
    ys, xs = mask.nonzero()
    xs, ys = xs - off[0], ys - off[1]
    e = 1 if plus_one else 0
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()) + e, int(ys.max() - ys.min()) + e]


def count(depth_gt_large, depth, K, delta, mutation=None):
    """-> dict: the six entries of scene_gt_info.json for one ground truth, and mask, mask_visib (bool (H,W)).
    depth_gt_large float32 (3H,3W), depth float32 (H,W) the sensor's (already scaled to mm)."""
    assert mutation is None or mutation in MUTATIONS
    large = np.asarray(depth_gt_large, dtype=np.float32)
    depth = np.asarray(depth, dtype=np.float32)
    H, W = depth.shape
    assert large.shape == (3 * H, 3 * W)
    depth_gt = frame_of(large, (W, H))
    dist_gt, dist_im = S.dist_image(depth_gt, K), S.dist_image(depth, K)
    if mutation == "diff64":
        visib = ((dist_gt - dist_im <= delta) | (dist_im == 0)) & (dist_gt > 0)
    else:
        visib = S._visible(dist_im, dist_gt, delta, "bop18" if mutation == "bop18" else "bop19")
    mask_large = large > 0
    mask = dist_gt > 0
    n_all = int((depth_gt > 0).sum()) if mutation == "all_on_frame" else int(mask_large.sum())
    if mutation == "valid_on_canvas":
        n_valid = int((dist_im[mask] > 0).sum()) + int(mask_large.sum() - (depth_gt > 0).sum())        # the margin's pixels counted as valid
    else:
        n_valid = int((dist_im[mask] > 0).sum())
    n_visib = int(visib.sum())
    fract = n_visib / float(n_all) if n_all > 0 else 0.0
    box_obj, box_visib = [-1, -1, -1, -1], [-1, -1, -1, -1]
    if (n_all if mutation == "gate_on_all" else n_visib) > 0:
        box_obj = _bbox(mask_large, (W, H), mutation == "plus_one")
        if mutation == "clip_obj":
            x0, y0 = min(max(box_obj[0], 0), W - 1), min(max(box_obj[1], 0), H - 1)
            x1, y1 = min(max(box_obj[0] + box_obj[2], 0), W - 1), min(max(box_obj[1] + box_obj[3], 0), H - 1)
            box_obj = [x0, y0, x1 - x0, y1 - y0]
    if n_visib > 0:
        box_visib = _bbox(visib, (0, 0), mutation == "plus_one")
    return {"px_count_all": n_all, "px_count_valid": n_valid, "px_count_visib": n_visib, "visib_fract": float(fract), "bbox_obj": box_obj,
            "bbox_visib": box_visib, "mask": mask, "mask_visib": visib}


def same_info(a, b):
    """the six entries equal (visib_fract as bits)"""
    return all((np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes()) if k == "visib_fract" else (list(np.asarray(a[k]).reshape(-1)) == list(np.asarray(b[k]).reshape(-1)))
               for k in INFO_KEYS)


def intervals(o, depth, K, delta, size):
    """o: oracle_canvas' dict.  -> dict
      all, valid, visib        (low, high) of each count
      set_obj, may_obj         bool (3H,3W): canvas pixels surely / possibly in the silhouette
      set_visib, may_visib     bool (H,W): frame pixels surely / possibly visible
      mask_decided, visib_decided  bool (H,W): where the masks are fixed, and the values there (mask_value, visib_value)"""
    W, H = size
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    depth = np.asarray(depth, dtype=np.float32)
    d = o["d"]
    dec = o["decided"]
    set_obj = (d > 0) & dec
    may_obj = o["covered_lo"]                                          # (the dilated coverage holds the nominal one)
    dg, dec_f, tol_f = frame_of(d, size), frame_of(dec, size), frame_of(o["tol"], size)
    may_f, set_f = frame_of(may_obj, size), frame_of(set_obj, size)
    t_im, t_gt = S.dist_image(depth, K), S.dist_image(dg, K)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    r = np.sqrt(1.0 + ((xs - K[0, 2]) / K[0, 0]) ** 2 + ((ys - K[1, 2]) / K[1, 1]) ** 2)
    mg = r * tol_f + 4.0 * S.EPS32 * (t_gt + t_im)                    # how far dist_gt - dist_im can move (+ its fp32 roundings)
    near = (dg > 0) & (t_im != 0) & (np.abs((t_gt - t_im) - delta) <= mg)
    vis = S._visible(t_im, t_gt, delta, "bop19")
    visib_decided = dec_f & ~near
    set_visib = vis & visib_decided
    may_visib = set_visib | (~visib_decided & may_f)
    valid = t_im > 0
    out = {"all": (int(set_obj.sum()), int(may_obj.sum())), "valid": (int((set_f & valid).sum()), int((may_f & valid).sum())),
           "visib": (int(set_visib.sum()), int(may_visib.sum())), "set_obj": set_obj, "may_obj": may_obj, "set_visib": set_visib,
           "may_visib": may_visib, "mask_decided": dec_f, "mask_value": dg > 0, "visib_decided": visib_decided, "visib_value": vis}
    return out


def _box_between(box, inner, outer, off):
    """box = x, y, w, h lies between the box of `inner` and the box of `outer` (bool images, `inner` a subset of `outer`)"""
    x0, y0, x1, y1 = box[0], box[1], box[0] + box[2], box[1] + box[3]
    if not outer.any():
        return False
    ox0, oy0, ow, oh = _bbox(outer, off)
    ok = ox0 <= x0 and oy0 <= y0 and x1 <= ox0 + ow and y1 <= oy0 + oh
    if inner.any():
        ix0, iy0, iw, ih = _bbox(inner, off)
        ok = ok and x0 <= ix0 and y0 <= iy0 and x1 >= ix0 + iw and y1 >= iy0 + ih
    return bool(ok)


def check_against_intervals(res, iv, size):
    """res: count's dict (or the device's, masks as bool) -> list of complaints (empty = passes)"""
    W, H = size
    bad = []
    for k, key in (("all", "px_count_all"), ("valid", "px_count_valid"), ("visib", "px_count_visib")):
        if not iv[k][0] <= int(res[key]) <= iv[k][1]:
            bad.append("%s %d outside %r" % (key, int(res[key]), iv[k]))
    box_obj, box_visib = [int(v) for v in res["bbox_obj"]], [int(v) for v in res["bbox_visib"]]
    if int(res["px_count_visib"]) > 0:
        if not _box_between(box_obj, iv["set_obj"], iv["may_obj"], (W, H)):
            bad.append("bbox_obj %r" % (box_obj,))
        if not _box_between(box_visib, iv["set_visib"], iv["may_visib"], (0, 0)):
            bad.append("bbox_visib %r" % (box_visib,))
    elif box_obj != [-1] * 4 or box_visib != [-1] * 4:
        bad.append("boxes must be -1 without a visible pixel")
    m, mv = np.asarray(res["mask"]).astype(bool), np.asarray(res["mask_visib"]).astype(bool)
    if (m != iv["mask_value"])[iv["mask_decided"]].any():
        bad.append("mask differs on %d decided pixels" % int((m != iv["mask_value"])[iv["mask_decided"]].sum()))
    if (mv != iv["visib_value"])[iv["visib_decided"]].any():
        bad.append("mask_visib differs on %d decided pixels" % int((mv != iv["visib_value"])[iv["visib_decided"]].sum()))
    return bad


def pack(mask):
    return np.packbits(np.asarray(mask).astype(bool).reshape(-1))


def unpack(bits, size):
    W, H = size
    return np.unpackbits(bits)[:W * H].reshape(H, W).astype(bool)
