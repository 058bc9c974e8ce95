"""Row N35 (poses verified against the photograph), the rule the device is pinned by.  Nothing here reads the reference (it never verifies);
everything is numpy and Python integers.  The renders the rule is applied to come from elsewhere: tests/render_tex_stages.render_tex_f32 /
tests/render_rgb_stages.render_f32 on the CPU, render.render_rgb's own colour and depth on the device.

The rule (csrc/pose_verify_photo.hip states it), per pose with colour render C (H,W,3) uint8, depth render D (H,W) and frame B (H,W,3) uint8:
  luma      Y = (77 R + 150 G + 29 B + 128) >> 8 of both (weights sum to 256: a grey pixel g gives exactly g); `bgr` swaps the two outer
            weights for the FRAME only
  pixels    Omega = {D > 0}, intersected with the visible mask's bit when there is one (pixel x of a packed row is bit x & 31 of word x >> 5)
  sums      n, Sa, Sb, Saa, Sbb, Sab over Omega (a: the render's luma, b: the frame's) and n_model = |D > 0|, as Python integers
  finish    cov = n Sab - Sa Sb, va = n Saa - Sa^2, vb = n Sbb - Sb^2 as integers, each converted to float64 once;
            ncc = cov / sqrt(va * vb), score = ncc, gain = cov / va, offset = (Sb - gain Sa) / n
  NaN       ok = False and ncc, score, gain, offset NaN when va == 0, vb == 0, n < min_pixels or the pose is not counted (zero sums)

  luma, pack, read, pixel_set, sums_of, finish, reference     the rule
  TAMPERINGS     eight wrong readings of it, for the checker's own test (tests/test_verify_photo.py asserts that each is caught)
  mesh_table     the test meshes: render_tex_stages.tex_meshes() with textures, render_rgb_stages.meshes() with vertex colours, and the "can":
                 a 24-segment cylinder under a 16 x 8 texture whose halves differ -- the object whose silhouette does not see a half turn
  PhotoCase, CASES, make     the cases of the device tests (poses, cameras, frames, masks, ids, shading)
  ulp_distance   the distance of two float64 arrays in units in the last place
"""
import math

import numpy as np

from tests import render_rgb_stages as RS
from tests import render_tex_stages as RT

LUMA = (77, 150, 29)
SUMS = ("Sa", "Sb", "Saa", "Sbb", "Sab")
TAMPERINGS = ("luma_weights", "no_round", "ge_zero", "ignore_mask", "cov_without_n", "split_sqrt", "min_pixels_off_by_one", "bgr_on_render")
MAX_PIXELS = 1 << 22


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def luma(img, swap=False, tamper=()):
    """(…,3) uint8 -> int64 luma; swap: the bytes are B G R"""
    w = (54, 183, 19) if "luma_weights" in tamper else LUMA
    c = np.asarray(img).astype(np.int64)
    r, b = (c[..., 2], c[..., 0]) if swap else (c[..., 0], c[..., 2])
    return (w[0] * r + w[1] * c[..., 1] + w[2] * b + (0 if "no_round" in tamper else 128)) >> 8


def pack(masks):
    """(N,H,W) bool -> (N,H,ceil(W/32)) int32 bit rows: pixel x is bit x & 31 of word x >> 5 (cp_coco_pack's layout)"""
    m = np.asarray(masks).astype(bool)
    N, H, W = m.shape
    WW = (W + 31) // 32
    pad = np.zeros((N, H, WW * 32), dtype=np.uint64)
    pad[:, :, :W] = m
    words = (pad.reshape(N, H, WW, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return words.astype(np.uint32).view(np.int32)


def read(bits, W):
    """pack's inverse: (N,H,WW) int32 -> (N,H,W) bool"""
    b = np.asarray(bits).view(np.uint32)
    x = np.arange(W)
    return ((b[:, :, x >> 5] >> (x & 31).astype(np.uint32)) & 1).astype(bool)


def pixel_set(D, mask=None, tamper=()):
    """-> (model (H,W) bool, Omega (H,W) bool)"""
    model = (np.asarray(D) >= 0) if "ge_zero" in tamper else (np.asarray(D) > 0)
    om = model if mask is None or "ignore_mask" in tamper else model & np.asarray(mask).astype(bool)
    return model, om


def sums_of(C, D, frame, mask=None, bgr=False, tamper=()):
    """the integer sums of one pose -> dict n_model, n, Sa, Sb, Saa, Sbb, Sab (Python integers)"""
    model, om = pixel_set(D, mask, tamper)
    a = luma(C, bgr and "bgr_on_render" in tamper, tamper)[om]
    b = luma(frame, bgr, tamper)[om]
    s = lambda v: int(v.sum(dtype=np.int64))      # noqa: E731
    return dict(n_model=int(model.sum()), n=int(om.sum()), Sa=s(a), Sb=s(b), Saa=s(a * a), Sbb=s(b * b), Sab=s(a * b))


def finish(s, min_pixels, counted=True, tamper=()):
    """sums -> dict n_model .. Sab (zeros when not counted), ncc, score, gain, offset (float64), ok"""
    out = {k: (int(s[k]) if counted else 0) for k in ("n_model", "n") + SUMS}
    n, Sa, Sb, Saa, Sbb, Sab = (out[k] for k in ("n",) + SUMS)
    cov = (Sab if "cov_without_n" in tamper else n * Sab) - Sa * Sb
    va, vb = n * Saa - Sa * Sa, n * Sbb - Sb * Sb
    assert max(abs(cov), abs(va), abs(vb)) < 1 << 63
    need = min_pixels + 1 if "min_pixels_off_by_one" in tamper else min_pixels
    ok = bool(counted and n >= need and va != 0 and vb != 0)
    nan = float("nan")
    if ok:
        dcov, dva, dvb = np.float64(float(cov)), np.float64(float(va)), np.float64(float(vb))      # one correctly rounded conversion each
        den = np.sqrt(dva) * np.sqrt(dvb) if "split_sqrt" in tamper else np.sqrt(dva * dvb)
        ncc = dcov / den
        gain = dcov / dva
        offset = (np.float64(float(Sb)) - gain * np.float64(float(Sa))) / np.float64(float(n))
    else:
        ncc = gain = offset = nan
    out.update(ncc=float(ncc), score=float(ncc), gain=float(gain), offset=float(offset), ok=ok)
    return out


def reference(C, D, frame, min_pixels, mask=None, bgr=False, counted=True, tamper=()):
    """the rule on one pose's renders and its frame"""
    H, W = np.asarray(D).shape
    assert H * W <= MAX_PIXELS
    return finish(sums_of(C, D, frame, mask, bgr, tamper), min_pixels, counted, tamper)


def ulp_distance(a, b):
    """the distance of float64 arrays in units in the last place (0 for two NaNs, a huge number for one)"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    key = lambda x: np.where(x.view(np.int64) < 0, np.int64(-2 ** 63) - x.view(np.int64), x.view(np.int64)).astype(object)      # noqa: E731
    d = np.abs(key(a) - key(b))
    both, one = np.isnan(a) & np.isnan(b), np.isnan(a) ^ np.isnan(b)
    return np.where(both, 0, np.where(one, 2 ** 62, d))


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
CAN_SEGMENTS, CAN_RADIUS, CAN_HALF = 24, 33.0, 50.0


def can_texture():
    """16 x 8, file row order: the left half bright and warm, the right half dark and cold, a faint pattern in each"""
    y, x = np.mgrid[0:8, 0:16]
    p = ((x + y) % 2) * 12 + 3 * y
    left = np.stack([225 - p, 205 - p, 70 + p], -1)
    right = np.stack([35 + p, 55 + p, 150 - p], -1)
    return np.where((x < 8)[..., None], left, right).astype(np.uint8)


def can_mesh():
    """-> (verts (V,3), faces (F,3), uvs (V,2), normals (V,3)): the side as 24 quads over 25 vertex columns (the seam column doubled: u = 0
    and u = 1), u = angle / 2 pi about the z axis, v along it; two caps as fans whose UVs lie inside one texel of each half"""
    n, r, h = CAN_SEGMENTS, CAN_RADIUS, CAN_HALF
    v, uv, nr, f = [], [], [], []
    for j in range(n + 1):
        a = 2.0 * math.pi * j / n
        for z, vv in ((-h, 0.02), (h, 0.98)):
            v.append([r * math.cos(a), r * math.sin(a), z]); uv.append([j / n, vv]); nr.append([math.cos(a), math.sin(a), 0.0])      # noqa: E702
    for j in range(n):
        a0, a1, b0, b1 = 2 * j, 2 * j + 1, 2 * j + 2, 2 * j + 3
        f += [[a0, b0, b1], [a0, b1, a1]]
    for z, u0 in ((-h, 0.22), (h, 0.72)):
        c = len(v)
        v.append([0.0, 0.0, z]); uv.append([u0, 0.5]); nr.append([0.0, 0.0, np.sign(z)])      # noqa: E702
        for j in range(n):
            a = 2.0 * math.pi * j / n
            v.append([r * math.cos(a), r * math.sin(a), z]); uv.append([u0 + 0.01 * math.cos(a), 0.5 + 0.02 * math.sin(a)]); nr.append([0.0, 0.0, np.sign(z)])      # noqa: E702
        f += [[c, c + 1 + j, c + 1 + (j + 1) % n] for j in range(n)]
    return (np.array(v, dtype=np.float32), np.array(f, dtype=np.int32), np.array(uv, dtype=np.float32), np.array(nr, dtype=np.float32))


def can_poses(tilt=0.12, distance=330.0):
    """-> (R_true, R_turned, t): the can upright in the image, its u = 0.5 meridian (the halves' border) towards the camera; R_turned is
    R_true after half a turn about the can's axis: the same silhouette up to boundary pixels, the other label"""
    base = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    Rx, _ = RT._pose(tilt, 0.0, 0.05, (0, 0, 0))
    R = Rx @ base
    half = np.diag([-1.0, -1.0, 1.0])
    return R, R @ half, np.array([2.0, -1.5, distance])


_MESHES = {}


def mesh_table():
    """name -> dict(verts, faces, normals, colors or None, uvs or None, tex or None)"""
    if not _MESHES:
        tm, tx, cm = RT.tex_meshes(), RT.textures(), RS.meshes()
        for name, mesh, tex in (("tquad", "quad", "t5x3"), ("tbox", "box", "check8"), ("tico", "ico80", "grad64x16"), ("tover", "quadover", "t2x2")):
            v, f, uv, n = tm[mesh]
            _MESHES[name] = dict(verts=v, faces=f, normals=n, colors=None, uvs=uv, tex=tx[tex])
        for name, mesh in (("cbox", "box"), ("cico", "ico80"), ("ctri", "tri3"), ("grey", "grey")):
            v, f, c, n = cm[mesh]
            _MESHES[name] = dict(verts=v, faces=f, normals=n, colors=c, uvs=None, tex=None)
        v, f, uv, n = can_mesh()
        _MESHES["can"] = dict(verts=v, faces=f, normals=n, colors=None, uvs=uv, tex=can_texture())
    return _MESHES


def meshset_args(names, tex_filter="nearest"):
    """MeshSet.from_arrays' arguments for the named meshes -> (list of vertex arrays, keyword dict)"""
    ms = [mesh_table()[k] for k in names]
    kw = dict(faces=[m["faces"] for m in ms], normals=[m["normals"] for m in ms], diameters=[1.0] * len(ms))
    if any(m["colors"] is not None for m in ms):
        kw["colors"] = [m["colors"] for m in ms]
    if any(m["tex"] is not None for m in ms):
        kw.update(textures=[m["tex"] for m in ms], uvs=[m["uvs"] for m in ms], tex_filter=tex_filter)
    return [m["verts"] for m in ms], kw


def cpu_render(name, R, t, K, size, tex_filter="nearest", shading="flat", ambient=0.5, surf_color=None):
    """one pose of one mesh through the fp32 restatements of the device's arithmetic -> (C (H,W,3) uint8, D (H,W) float32: 1 where covered)"""
    m = mesh_table()[name]
    if m["tex"] is not None and surf_color is None:
        rgb, face = RT.render_tex_f32(R, t, K, m["verts"], m["faces"], m["uvs"], m["tex"], m["normals"], size, tex_filter, shading, ambient)
        return rgb, (face >= 0).astype(np.float32)
    rgb, depth, _ = RS.render_f32(R, t, K, m["verts"], m["faces"], m["colors"], m["normals"], size, shading, ambient, surf_color=surf_color)
    return rgb, depth


def silhouette_iou(Da, Db):
    a, b = np.asarray(Da) > 0, np.asarray(Db) > 0
    return float((a & b).sum()) / float(max((a | b).sum(), 1))


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
class PhotoCase:
    """One call of verify_poses_photo: P poses of `meshes` over n_img noise frames of `size` = (W, H)."""

    def __init__(self, name, meshes, size, focal, P, seed, n_img=1, tex_filter="nearest", shading="flat", ambient=0.5, light=(0, 0, 0),
                 surf_color=None, bgr=False, masks=0, shared_masks=False, per_pose_K=False, min_pixels=8):
        rng = np.random.default_rng(seed)
        W, H = size
        self.name, self.meshes, self.size, self.P, self.n_img = name, tuple(meshes), size, P, n_img
        self.tex_filter, self.shading, self.ambient, self.light, self.surf_color, self.bgr = tex_filter, shading, ambient, light, surf_color, bgr
        self.min_pixels = min_pixels
        K = RT._cam(size, focal)
        self.K = np.stack([K + np.array([[0.3 * b, 0, 0.2 * b], [0, -0.2 * b, -0.1 * b], [0, 0, 0]]) for b in range(P)]) if per_pose_K else K
        ang = rng.uniform(-1.2, 1.2, (P, 3))
        self.R = np.stack([RT._pose(*a, (0, 0, 0))[0] for a in ang])
        spread = np.array([0.11 * W / focal, 0.11 * H / focal]) * 330.0      # the centre moves by a ninth of the frame at the most
        self.t = np.concatenate([rng.uniform(-1, 1, (P, 2)) * spread, rng.uniform(300.0, 360.0, (P, 1))], 1)
        self.mesh_ids = None if len(self.meshes) == 1 else (np.arange(P) % len(self.meshes)).astype(np.int32)
        self.image_ids = None if n_img == 1 else (rng.integers(0, n_img, P).astype(np.int32) if n_img != P else None)
        # frames: noise of limited bandwidth (blocks of 3 x 3 under pixel noise), so that the frame patches are far from flat
        coarse = rng.integers(0, 256, (n_img, (H + 2) // 3, (W + 2) // 3, 3))
        up = np.repeat(np.repeat(coarse, 3, 1), 3, 2)[:, :H, :W]
        self.frames = np.clip(up + rng.integers(-20, 21, (n_img, H, W, 3)), 0, 255).astype(np.uint8)
        self.masks = self.mask_ids = None
        if masks:
            NM = masks
            yy, xx = np.mgrid[0:H, 0:W]
            m = []
            for k in range(NM):                                     # half planes through the frame with a sprinkle of holes
                a = rng.uniform(0, 2 * math.pi)
                m.append((((xx - W / 2.0) * math.cos(a) + (yy - H / 2.0) * math.sin(a)) > -0.2 * W) & (rng.random((H, W)) < 0.85))
            self.masks = np.stack(m)
            self.mask_ids = (rng.integers(0, NM, P).astype(np.int32) if shared_masks or NM != P else None)
        self.status = None

    def image_of(self, b):
        return 0 if self.n_img == 1 else (b if self.image_ids is None else int(self.image_ids[b]))

    def mask_of(self, b):
        return None if self.masks is None else (b if self.mask_ids is None else int(self.mask_ids[b]))

    def K_of(self, b):
        return self.K[b] if self.K.ndim == 3 else self.K

    def render_kwargs(self):
        return dict(shading=self.shading, ambient_weight=self.ambient, light_cam_pos=self.light, surf_color=self.surf_color)


# frames (W, H): (33, 31) partial tiles on both sides; (64, 64) whole tiles; (96, 40) with three frames: 3 x 2 tiles, the bottom ones partial.
# P = 1, 3 and 257 (past one 256-thread pose block).
CASES = {
    "tex_nearest_33x31_1": lambda: PhotoCase("tex_nearest_33x31_1", ["tbox"], (33, 31), 70.0, 1, 11),
    "tex_nearest_33x31_3": lambda: PhotoCase("tex_nearest_33x31_3", ["tquad", "tbox", "tico"], (33, 31), 70.0, 3, 12, masks=3),
    "tex_linear_64_3": lambda: PhotoCase("tex_linear_64_3", ["tico", "tover", "tbox"], (64, 64), 150.0, 3, 13, tex_filter="linear", shading="phong", bgr=True,
                                         masks=2, shared_masks=True, per_pose_K=True),
    "vcol_96x40_3": lambda: PhotoCase("vcol_96x40_3", ["cbox", "cico", "ctri"], (96, 40), 100.0, 3, 14, n_img=3, shading="phong", ambient=0.3, light=(40.0, 60.0, 100.0)),
    "vcol_flat_64_3": lambda: PhotoCase("vcol_flat_64_3", ["cico", "grey"], (64, 64), 140.0, 3, 15, bgr=True, ambient=0.4),
    "surf_96x40_257": lambda: PhotoCase("surf_96x40_257", ["cbox", "tico"], (96, 40), 100.0, 257, 16, n_img=3, surf_color=(0.9, 0.5, 0.2), masks=5, shared_masks=True,
                                        ambient=0.35),
    "mixed_64_3": lambda: PhotoCase("mixed_64_3", ["tquad", "cbox", "grey"], (64, 64), 150.0, 3, 17, shading="phong", masks=3),
    "mixed_33x31_1": lambda: PhotoCase("mixed_33x31_1", ["tbox", "cico"], (33, 31), 70.0, 1, 18, tex_filter="linear", bgr=True),
    "mixed_96x40_257": lambda: PhotoCase("mixed_96x40_257", ["tbox", "cico", "grey", "tquad"], (96, 40), 100.0, 257, 19, n_img=3, shading="phong"),
}
_CASES = {}


def make(name):
    if name not in _CASES:
        _CASES[name] = CASES[name]()
    return _CASES[name]
