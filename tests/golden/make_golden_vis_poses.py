#!/usr/bin/env python3
"""Row N18 (poses drawn over the photograph) pinned by the REFERENCE's own vis_object_poses.

Runs ONLY where the reference tree is (CHECKERPOSE_REFERENCE, default /root/reference; nothing of it travels, only the recorded
numbers in vis_poses.npz are committed):

  python tests/golden/make_golden_vis_poses.py

bop_toolkit_lib.visualization.vis_object_poses renders through a `renderer` object and composes in numpy.  Here it runs as it is, on
seeded per-pose frames served by a fake renderer (render_object returns the case's m_rgb / m_depth of the pose whose obj_id is asked),
with: imageio and png stubbed in sys.modules (inout imports them), np.float = float (removed from numpy), inout.save_im captured,
misc.ensure_dir a no-op, write_text_on_image replaced by the identity that records its txt_list (the font call it needs does not
exist in the Pillow at hand: text is UNPINNED and out of scope).  draw_rect is the reference's own, through Pillow.
Recorded per case: the inputs (frame, the poses' frames, the sensor depth), the saved RGB picture, and for the depth-difference cases
the saved picture and the min / max the reference would print.  A depth-difference case whose difference holds fewer than three
distinct values is REFUSED (the reference raises or divides 0 by 0 there): a condition of the fixture, not a tolerance."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "bop_toolkit"))
sys.path.insert(0, ROOT)

for _name in ("imageio", "png"):
    sys.modules[_name] = types.ModuleType(_name)
if not hasattr(np, "float"):
    np.float = float

from bop_toolkit_lib import inout, misc, visualization  # noqa: E402
from tests import vis_stages as VS  # noqa: E402

SAVED, TEXT = {}, {}
inout.save_im = lambda path, im, jpg_quality=95: SAVED.__setitem__(path, np.array(im))
misc.ensure_dir = lambda path: None


def _identity_text(im, txt_list, loc=(3, 0), color=(1.0, 1.0, 1.0), size=20):
    TEXT["last"] = txt_list
    return im


visualization.write_text_on_image = _identity_text


class FakeRenderer:
    def __init__(self, rgbs, depths):
        self.rgbs, self.depths = rgbs, depths

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        return {"rgb": self.rgbs[obj_id], "depth": self.depths[obj_id]}


def shape(W, H, kind, x0, y0, x1, y1):
    ys, xs = np.mgrid[0:H, 0:W]
    inside = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
    if kind == "ellipse":
        cx, cy, rx, ry = (x0 + x1) / 2.0, (y0 + y1) / 2.0, max((x1 - x0) / 2.0, 0.5), max((y1 - y0) / 2.0, 0.5)
        inside &= ((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1.0
    return inside


def pose(W, H, kind, rect, colour, z0, gx=0.0, gy=0.0, shade=True):
    """a filled shape of `colour` (shaded by a smooth ramp) on the depth plane z0 + gx x + gy y, rounded to quarters of a millimetre"""
    m = shape(W, H, kind, *rect)
    ys, xs = np.mgrid[0:H, 0:W]
    ramp = (0.55 + 0.45 * (xs + ys) / float(W + H)) if shade else np.ones((H, W))
    rgb = np.zeros((H, W, 3), dtype=np.uint8)
    for c in range(3):
        rgb[..., c] = np.where(m, np.round(colour[c] * ramp), 0).astype(np.uint8)
    depth = np.where(m, np.round(4.0 * (z0 + gx * xs + gy * ys)) / 4.0, 0.0).astype(np.float32)
    return rgb, depth


def sensor(rng, W, H, ren_depth, offsets, zero_share=0.15):
    """a sensor depth: the composite's depth minus an offset drawn per pixel from `offsets`, a background plane elsewhere, zeros sprinkled"""
    off = np.asarray(offsets, dtype=np.float32)[rng.integers(0, len(offsets), size=(H, W))]
    d = np.where(ren_depth > 0, ren_depth - off, np.float32(900.0)).astype(np.float32)
    d[rng.random((H, W)) < zero_share] = 0.0
    return d


def build_cases():
    cases = []
    for W, H in ((48, 40), (33, 31)):
        sx, sy = W / 48.0, H / 40.0
        r = lambda a, b, c, d: (int(a * sx), int(b * sy), int(c * sx), int(d * sy))      # noqa: E731
        overlap = [pose(W, H, "ellipse", r(4, 5, 30, 30), (230, 70, 30), 520.0, 0.6, 0.2), pose(W, H, "rect", r(18, 12, 44, 36), (60, 200, 90), 500.0, -0.3, 0.9),
                   pose(W, H, "ellipse", r(10, 18, 38, 39), (40, 90, 240), 540.0, 0.1, -0.8)]
        tie = [pose(W, H, "rect", r(6, 6, 30, 28), (250, 40, 40), 600.0, shade=False), pose(W, H, "rect", r(16, 14, 42, 34), (40, 40, 250), 600.0, shade=False)]
        black = [pose(W, H, "rect", r(8, 8, 36, 30), (120, 220, 60), 640.0, 0.5, 0.0), pose(W, H, "ellipse", r(14, 4, 40, 26), (0, 0, 0), 560.0, 0.0, 0.4)]
        nothing = [pose(W, H, "rect", (W + 5, H + 5, W + 9, H + 9), (200, 200, 200), 500.0), pose(W, H, "ellipse", r(10, 10, 30, 30), (90, 160, 210), 700.0, 0.2, 0.2)]
        border = [pose(W, H, "rect", (0, 0, int(12 * sx), H - 1), (210, 180, 40), 480.0, 0.0, 0.3), pose(W, H, "rect", (0, 0, W - 1, H - 1), (70, 60, 140), 800.0, 0.2, 0.1),
                  pose(W, H, "rect", (W - 1, H - 1, W - 1, H - 1), (255, 255, 255), 300.0)]
        bright = [pose(W, H, "rect", r(4, 4, 34, 30), (240, 200, 130), 500.0, shade=False), pose(W, H, "ellipse", r(12, 10, 44, 38), (200, 130, 250), 450.0, shade=False),
                  pose(W, H, "rect", r(20, 2, 40, 22), (90, 250, 10), 470.0, shade=False)]
        for name, poses, dd in (("overlap", overlap, True), ("tie", tie, False), ("black", black, True), ("nopixel", nothing, False), ("border", border, True),
                                ("saturate", bright, False), ("none", [], False)):
            for resolve in (True, False):
                cases.append({"name": "%s_%s_%dx%d" % (name, "resolve" if resolve else "sum", W, H), "W": W, "H": H, "poses": poses, "resolve": resolve,
                              "dd": dd and resolve})
    return cases


def main():
    rng = np.random.default_rng(18)
    out, meta = {}, []
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    for ci, c in enumerate(build_cases()):
        W, H, poses = c["W"], c["H"], c["poses"]
        frame = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        frame[: H // 4] = 255                                       # a bright band: the blend and the boxes layer reach the clip
        rgbs = np.stack([p[0] for p in poses]) if poses else np.zeros((0, H, W, 3), dtype=np.uint8)
        depths = np.stack([p[1] for p in poses]) if poses else np.zeros((0, H, W), dtype=np.float32)
        ren_depth = VS.compose(frame, rgbs, depths, resolve=True)["ren_depth"]
        # the offsets put dd on both sides of delta = 15 and exactly on it (quarters of a millimetre: every value exact in float32)
        depth = sensor(rng, W, H, ren_depth, (-20.0, -3.25, 0.0, 3.5, 14.75, 15.0, 15.25, 40.0))
        if c["dd"] and VS.distinct_dd(ren_depth, depth) < 3:
            raise SystemExit("case %s: fewer than three distinct depth differences -- refused" % c["name"])
        SAVED.clear()
        TEXT.clear()
        visualization.vis_object_poses(poses=[{"obj_id": j, "R": np.eye(3), "t": np.zeros((3, 1))} for j in range(len(poses))], K=K,
                                       renderer=FakeRenderer(rgbs, depths), rgb=frame, depth=depth, vis_rgb_path="out/rgb.jpg",
                                       vis_depth_diff_path="out/dd.jpg" if c["dd"] else None, vis_rgb_resolve_visib=c["resolve"])
        k = "c%02d_" % ci
        out[k + "frame"], out[k + "m_rgb"], out[k + "m_depth"], out[k + "depth"] = frame, rgbs, depths, depth
        out[k + "vis"] = SAVED["out/rgb.jpg"]
        assert out[k + "vis"].dtype == np.uint8 and out[k + "vis"].shape == (H, W, 3)
        if c["dd"]:
            out[k + "dd_vis"] = SAVED["out/dd.jpg"]
            info = {e["name"]: float(e["val"]) for e in TEXT["last"]}
            out[k + "dd_minmax"] = np.array([info["min diff"], info["max diff"]], dtype=np.float64)
        meta.append({"name": c["name"], "resolve": bool(c["resolve"]), "dd": bool(c["dd"]), "n": len(poses)})
        print("%-28s poses %d  dd %s" % (c["name"], len(poses), c["dd"]))
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "vis_poses.npz")
    np.savez_compressed(path, **out)
    print("%d cases -> %s (%d bytes)" % (len(meta), path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
