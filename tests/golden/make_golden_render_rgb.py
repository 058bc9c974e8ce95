#!/usr/bin/env python3
"""Row N14 (shaded RGB frames) pinned by the REFERENCE's own matrices and view sampler.

Runs ONLY where the reference tree is (CHECKERPOSE_REFERENCE, default /root/reference; nothing of it travels, only the recorded
numbers in render_rgb.npz are committed):

  python tests/golden/make_golden_render_rgb.py

The reference's RGB renderer is GLSL under OpenGL and runs nowhere this project runs, so what it would DRAW is UNPINNED (as the depth
render of row N8 is): the shading is pinned to the rule read from the shaders, stated in float64 by tests/render_rgb_stages.py.
What the reference does compute on the host is taken from its OWN code:
  * renderer_py is imported with glumpy / OpenGL (and the image libraries of inout) stubbed in sys.modules, and per case u_mv, u_nm and
    u_mvp come from its _calc_model_view, _calc_normal_matrix and _calc_calib_proj / _calc_model_view_proj, built from mat_model,
    mat_view and the clipping planes exactly as render_object builds them: the oracle shades with the matrices the shader would get;
  * view_sampler.sample_views, both modes, min_n_views 1, 12, 42, 162, 642, two radii, the full sphere and a restricted azimuth /
    elevation range that cuts views: the views and views_level are recorded.
Meshes are generated in closed form (tests/render_rgb_stages.meshes) and CRC-checked.  Per case at most 5 % of the covered pixels may
be undecided by the oracle: asserted here, a pose that misses it is redrawn with the next seed.  The file is byte-reproducible."""
import json
import math
import os
import sys
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "bop_toolkit"))
sys.path.insert(0, ROOT)

for _name in ("glumpy", "glumpy.log", "OpenGL", "OpenGL.GL", "imageio", "png", "cv2"):
    try:
        __import__(_name)
    except Exception:
        sys.modules[_name] = types.ModuleType(_name)
if not hasattr(sys.modules["glumpy"], "app"):
    sys.modules["glumpy"].app = sys.modules["glumpy"].gloo = sys.modules["glumpy"].gl = types.ModuleType("glumpy.stub")
    sys.modules["glumpy.log"].log = types.SimpleNamespace(setLevel=lambda level: None)

from bop_toolkit_lib import renderer_py, view_sampler  # noqa: E402
from tests import render_rgb_stages as RS  # noqa: E402

LM_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])

# name, mesh, (W, H), shading, ambient, light (reference's camera frame), ssaa, placement, K group, surf_color, bg
CASES = [
    ("tri3_flat", "tri3", (33, 31), "flat", 0.5, (0, 0, 0), 1, "centre", 0, None, (0, 0, 0)),
    ("tri3_phong_s2", "tri3", (67, 45), "phong", 0.5, (0, 0, 0), 2, "centre", 0, None, (0, 0, 0)),
    ("quad_axis", "quad", (64, 64), "flat", 0.2, (0, 0, 0), 1, "axis", 4, None, (0, 0, 0)),
    ("box_phong", "box", (67, 45), "phong", 0.5, (0, 0, 0), 1, "centre", 0, None, (0, 0, 0)),
    ("box_flat_light", "box", (160, 120), "flat", 0.5, (300.0, 200.0, 100.0), 1, "centre", 0, None, (0, 0, 0)),
    ("box_left_a0", "box", (67, 45), "flat", 0.0, (0, 0, 0), 1, "left", 0, None, (0, 0, 0)),
    ("box_top", "box", (67, 45), "flat", 0.5, (0, 0, 0), 1, "top", 0, None, (0, 0, 0)),
    ("box_right", "box", (67, 45), "phong", 0.5, (0, 0, 0), 1, "right", 0, None, (0, 0, 0)),
    ("ico1280_topleft", "ico1280", (67, 45), "flat", 0.5, (0, 0, 0), 1, "topleft", 0, None, (0, 0, 0)),
    ("box_corner_a1", "box", (67, 45), "phong", 1.0, (0, 0, 0), 1, "corner", 0, None, (0, 0, 0)),
    ("box_outside", "box", (67, 45), "flat", 0.5, (0, 0, 0), 1, "outside", 0, None, (0.2, 0.4, 0.6)),
    ("halfbox_flat", "halfbox", (67, 45), "flat", 0.5, (0, 0, 0), 1, "open", 0, None, (0, 0, 0)),
    ("halfbox_phong_light", "halfbox", (96, 80), "phong", 0.3, (-250.0, 150.0, 50.0), 1, "open", 0, None, (0, 0, 0)),
    ("ico80_phong", "ico80", (33, 31), "phong", 0.5, (0, 0, 0), 1, "centre", 0, None, (0, 0, 0)),
    ("ico80_flat_s4", "ico80", (67, 45), "flat", 0.5, (0, 0, 0), 4, "centre", 0, None, (0, 0, 0)),
    ("ico1280_phong", "ico1280", (67, 45), "phong", 0.5, (0, 0, 0), 1, "centre", 0, None, (0, 0, 0)),
    ("ico1280_flat_s2", "ico1280", (96, 80), "flat", 0.5, (0, 0, 0), 2, "centre", 0, None, (0, 0, 0)),
    ("zeroarea_flat", "zeroarea", (67, 45), "flat", 0.5, (0, 0, 0), 1, "centre", 0, None, (0, 0, 0)),
    ("coincident", "coincident", (67, 45), "flat", 1.0, (0, 0, 0), 1, "centre", 0, None, (0, 0, 0)),
    ("grey_phong", "grey", (67, 45), "phong", 0.5, (0, 0, 0), 1, "centre", 0, None, (0, 0, 0)),
    ("box_surf_a1", "box", (67, 45), "flat", 1.0, (0, 0, 0), 1, "centre", 0, (0.25, 0.5, 0.75), (0, 0, 0)),
    ("box_surf_a1_phong", "box", (67, 45), "phong", 1.0, (0, 0, 0), 1, "centre", 0, (0.25, 0.5, 0.75), (0, 0, 0)),
    ("box_surf_tie", "box", (67, 45), "flat", 1.0, (0, 0, 0), 1, "centre", 0, (0.3, 0.1, 0.7), (0, 0, 0)),
    ("icofloat_phong", "icofloat", (67, 45), "phong", 0.5, (0, 0, 0), 1, "centre", 0, None, (0, 0, 0)),
    ("slab_grazing", "slab", (96, 80), "flat", 1.0, (0, 0, 0), 1, "grazing", 0, None, (0, 0, 0)),
    ("ico80_onepixel", "ico80", (33, 31), "flat", 0.5, (0, 0, 0), 1, "far", 0, None, (0, 0, 0)),
    ("box_behind", "box", (67, 45), "flat", 0.5, (0, 0, 0), 1, "behind", 0, None, (0.1, 0.1, 0.1)),
    ("box_k1_phong", "box", (67, 45), "phong", 0.5, (0, 0, 0), 1, "centre", 1, None, (0, 0, 0)),
    ("ico80_bottom_k2", "ico80", (67, 45), "phong", 0.7, (0, 0, 0), 1, "bottom", 2, None, (1.0, 1.0, 1.0)),
]

VIEW_COUNTS = (1, 12, 42, 162, 642)
VIEW_SETTINGS = ((1.0, (0.0, 2.0 * math.pi), (-0.5 * math.pi, 0.5 * math.pi)), (650.0, (0.3, 4.0), (0.1, 1.2)))


def camera(size, group):
    W, H = size
    s = W / 640.0
    K = np.array([[LM_K[0, 0] * s, 0.0, W / 2.0 - 0.3], [0.0, LM_K[1, 1] * s, H / 2.0 + 0.2], [0.0, 0.0, 1.0]])
    if group == 1:
        K[0, 0] *= 1.13; K[1, 1] *= 0.91; K[0, 2] += 2.4; K[1, 2] -= 1.7     # noqa: E702
    elif group == 2:
        K[0, 0] *= 0.8; K[1, 1] *= 0.8; K[0, 2] -= 3.1                        # noqa: E702
    elif group == 4:
        K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    return K


def rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def pose(place, K, size, verts, rng):
    W, H = size
    diam = float(np.linalg.norm(verts.max(0) - verts.min(0)))
    z = K[0, 0] * diam / (0.62 * min(W, H))
    R = rotation(rng)
    at = {"centre": (W / 2.0, H / 2.0), "open": (W / 2.0, H / 2.0), "left": (2.0, H / 2.0), "top": (W / 2.0, 1.5), "right": (W - 2.0, H / 2.0), "topleft": (1.0, 2.0), "corner": (W - 3.0, H - 2.0),
          "outside": (-3.0 * W, H / 2.0), "bottom": (W / 2.0, H - 1.0), "far": (W / 2.0, H / 2.0), "behind": (W / 2.0, H / 2.0),
          "axis": (W / 2.0, H / 2.0), "grazing": (W / 2.0, H / 2.0)}[place]
    if place == "far":
        z = K[0, 0] * diam / 1.1                                           # about one pixel across
    if place == "behind":
        z = 0.3 * diam                                                      # the far side in front, the near side behind the camera
    if place == "axis":
        R = np.eye(3)
    if place == "grazing":
        a = math.radians(80.0) + 0.05 * rng.standard_normal()              # the slab's plane nearly contains the optical axis
        R = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(a), -math.sin(a)], [0.0, math.sin(a), math.cos(a)]])
        z = 1.5 * diam
    if (verts[:, 2] == verts[0, 2]).all() and place not in ("axis", "grazing"):     # a planar mesh: a limited tilt, never edge-on
        a, b, c = rng.uniform(-math.pi, math.pi), rng.uniform(-0.7, 0.7), rng.uniform(-0.7, 0.7)
        rz = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(b), -math.sin(b)], [0.0, math.sin(b), math.cos(b)]])
        ry = np.array([[math.cos(c), 0.0, math.sin(c)], [0.0, 1.0, 0.0], [-math.sin(c), 0.0, math.cos(c)]])
        R = rx @ ry @ rz
    t = z * np.linalg.solve(K, np.array([at[0], at[1], 1.0]))
    if place == "axis":
        t = np.array([0.0, 0.0, z])
    return R, t


def reference_uniforms(R, t, K, size, verts):
    """u_mv, u_nm, u_mvp as RendererPython.render_object / _draw_rgb form them (renderer_py.py:422-495), from the reference's functions"""
    W, H = size
    mat_model = np.eye(4, dtype=np.float32)
    mat_view_cv = np.eye(4, dtype=np.float32)
    mat_view_cv[:3, :3], mat_view_cv[:3, 3] = R, t.squeeze()
    yz_flip = np.eye(4, dtype=np.float32)
    yz_flip[1, 1], yz_flip[2, 2] = -1, -1
    mat_view = yz_flip.dot(mat_view_cv).T
    lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
    corners = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]).T
    eye_z = mat_view_cv[2, :].reshape((1, 4)).dot(corners)
    Kc = np.array([[K[0, 0], 0.0, K[0, 2]], [0.0, K[1, 1], K[1, 2]], [0.0, 0.0, 1.0]])
    mat_proj = renderer_py._calc_calib_proj(Kc, 0, 0, W, H, eye_z.min(), eye_z.max())
    return (renderer_py._calc_model_view(mat_model, mat_view), renderer_py._calc_normal_matrix(mat_model, mat_view),
            renderer_py._calc_model_view_proj(mat_model, mat_view, mat_proj))


def main():
    meshes = RS.meshes()
    out = {}
    crc = 0
    for name in RS.MESH_NAMES:
        v, f, c, n = meshes[name]
        for a in (v, f, n) + ((c,) if c is not None else ()):
            crc = zlib.crc32(np.ascontiguousarray(a).tobytes(), crc)
    out["mesh_crc"] = np.array([crc], dtype=np.int64)
    meta = []
    for ci, (name, mesh, size, shading, amb, light, ssaa, place, kg, surf, bg) in enumerate(CASES):
        v, f, c, n = meshes[mesh]
        K = camera(size, kg)
        for seed in range(64):
            rng = np.random.default_rng(1000 * ci + seed)
            R, t = pose(place, K, size, v, rng)
            if place == "behind":
                share, rendered = 0.0, False
                break
            u_mv, u_nm, u_mvp = reference_uniforms(R, t, K, size, v)
            o = RS.oracle_rgb(R, t, K, v, f, c, n, size, shading, amb, light, bg, surf, ssaa, u_mv, u_nm, want_candidates=False)
            share, rendered = RS.undecided_share(o), True
            if place == "open" and not (o["covered"].sum() > 0.10 * size[0] * size[1]):
                continue
            if share <= 0.05 or name == "coincident":
                break
        else:
            raise SystemExit("case %s: no pose within the 5 %% limit" % name)
        if not rendered:
            u_mv, u_nm, u_mvp = reference_uniforms(R, t, K, size, v)
        else:
            assert share <= 0.05 or name == "coincident", (name, share)
        print("%-22s seed %2d  undecided %.4f  covered %d" % (name, seed, share, int(o["covered"].sum()) if rendered else 0))
        out["R_%02d" % ci], out["t_%02d" % ci], out["K_%02d" % ci] = R, t, K
        out["u_mv_%02d" % ci], out["u_nm_%02d" % ci], out["u_mvp_%02d" % ci] = (np.asarray(m, dtype=np.float64) for m in (u_mv, u_nm, u_mvp))
        meta.append({"name": name, "mesh": mesh, "size": list(size), "shading": shading, "ambient": amb, "light": list(light), "ssaa": ssaa,
                     "place": place, "surf_color": None if surf is None else list(surf), "bg": list(bg), "rendered": rendered,
                     "undecided": round(share, 6)})
    out["cases"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    vmeta = []
    for mode in ("hinterstoisser", "fibonacci"):
        for n in VIEW_COUNTS:
            for si, (radius, az, el) in enumerate(VIEW_SETTINGS):
                views, levels = view_sampler.sample_views(n, radius, az, el, mode)
                key = "views_%s_%d_%d" % (mode[0], n, si)
                out[key + "_R"] = np.array([vw["R"] for vw in views], dtype=np.float64).reshape(-1, 3, 3)
                out[key + "_t"] = np.array([vw["t"] for vw in views], dtype=np.float64).reshape(-1, 3, 1)
                out[key + "_level"] = np.asarray(levels, dtype=np.int64)
                vmeta.append({"key": key, "mode": mode, "n": n, "radius": radius, "azimuth": list(az), "elev": list(el)})
    out["views"] = np.frombuffer(json.dumps(vmeta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "render_rgb.npz")
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:           # fixed member order and timestamps: byte-reproducible
        for k in sorted(out):
            import io
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
