"""Row N20 (UV texture sampling), the stages the device is pinned by.  Nothing here reads the reference; everything is numpy, on top of
tests/render_rgb_stages.py (imported unchanged: coverage, the winning face, the weights, light_w and their tolerances are its).

  tex_meshes        the test meshes with UVs: quad, quadover (UVs from -0.25 to 1.25), box, slab (grazing), ico80 (spherical UVs), faceted
                    (a box whose faces share no vertices; every face's three UVs lie inside ONE texel of the 5 x 3 texture)
  textures          t1x1, t2x2, t5x3 (all texels distinct), check8 (8 x 8 checkerboard), grad64x16; uint8 (Ht, Wt, 3), file row order
  sample            the sampler rule (csrc/render_shade.h) in any dtype;  oracle_tex: the float64 statement on top of oracle_rgb's
                    geometry;  render_tex_f32: the device's arithmetic in numpy float32
  CASES             the cases of the band tests (pose, camera, frame, mesh, texture, shading, ambient)
  MUTATIONS         six mutations of the statement, for the checker's own test

The rule.  Over the winning face (u, v) is interpolated with v_color's perspective-correct weights in v_color's expression form
a + (w1 (c - a) + w2 (d - a)).  The reference uploads np.flipud(image): GL's texel row j is the file's row Ht - 1 - j.
  nearest:  i = clamp(floor(u Wt), 0, Wt - 1),  j = clamp(floor(v Ht), 0, Ht - 1),  texel = T[Ht - 1 - j, i]
  linear:   a = u Wt - 0.5, i0 = floor(a), alpha = a - i0, i1 = i0 + 1 (both clamped); likewise j0, j1, beta;
            texel = lo + beta (hi - lo),  lo = t00 + alpha (t10 - t00),  hi = t01 + alpha (t11 - t01)
  v = 255 * light_w * (texel / 255).

Tolerances (derived, not tuned; e = 2^-24; dw = the weight error of render_rgb_stages' docstring).  The interpolated u carries
du = dw span_u + 4 e |u| (span_u: the face's largest UV difference), so its texel coordinate u Wt carries
    E_u = Wt (dw span_u + 4 e |u|) + e |u Wt|                          (likewise E_v)
nearest: a sample is DECIDED when u Wt lies farther than E_u from every integer in 1..Wt-1 and v Ht farther than E_v from every integer
in 1..Ht-1 (the clamp removes the boundaries at 0 and Wt).  Its texel is then exact and
    tol_c = 255 (d_dot cmax + light_w 4 e + 4 e),   cmax = the texture's largest value / 255, d_dot: render_rgb_stages'.
An undecided sample may take any texel whose index lies within E of its coordinate.
linear: nothing new is undecided; the blend is Lipschitz in its coordinates with constant D = the largest difference between adjacent
texels (/ 255), so tol_c grows by 255 light_w ((E_u + E_v) D + 8 e)."""
import numpy as np

from tests import render_rgb_stages as RS
from tests import vsd_stages as S

EPS32 = RS.EPS32
MUTATIONS = ("noflip", "swapuv", "affineuv", "roundidx", "noclamp", "nohalf")
FILTERS = ("nearest", "linear")


# ---- meshes and textures ----------------------------------------------------------------------------------------------------------
_MESHES = {}


def tex_meshes():
    """name -> (verts float32 (V,3), faces int32 (F,3), uvs float32 (V,2), normals float32 (V,3))"""
    if _MESHES:
        return _MESHES
    base = RS.meshes()
    out = {}
    v, f, _, n = base["quad"]
    out["quad"] = (v, f, np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]), n)
    out["quadover"] = (v, f, np.array([[-0.25, -0.25], [1.25, -0.25], [1.25, 1.25], [-0.25, 1.25]]), n)
    v, f, _, n = base["box"]
    p = (v.astype(np.float64) - v.min(0)) / (v.max(0) - v.min(0))
    out["box"] = (v, f, np.stack([0.05 + 0.6 * p[:, 0] + 0.3 * p[:, 2], 0.05 + 0.6 * p[:, 1] + 0.3 * p[:, 2]], 1), n)
    v, f, _, n = base["slab"]                                          # u along the long axis, seen at a grazing angle
    out["slab"] = (v, f, np.stack([(v[:, 2] + 150.0) / 300.0, (v[:, 0] + 30.0) / 60.0], 1), n)
    v, f, _, n = base["ico80"]
    d = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    out["ico80"] = (v, f, np.stack([np.arctan2(d[:, 1], d[:, 0]) / (2.0 * np.pi) + 0.5, np.arccos(np.clip(d[:, 2], -1.0, 1.0)) / np.pi], 1), n)
    v, f, _, n = base["box"]                                           # faceted: 12 faces x 3 own vertices; face k lies in texel k of 5 x 3
    fv, fn, fuv = v[f.reshape(-1)], n[f.reshape(-1)], []
    for k in range(f.shape[0]):
        i, j = k % 5, k // 5
        fuv += [[(i + 0.3) / 5.0, (j + 0.3) / 3.0], [(i + 0.7) / 5.0, (j + 0.4) / 3.0], [(i + 0.5) / 5.0, (j + 0.7) / 3.0]]
    out["faceted"] = (fv, np.arange(3 * f.shape[0], dtype=np.int32).reshape(-1, 3), np.array(fuv), fn)
    for k, (v, f, uv, n) in out.items():
        _MESHES[k] = (np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32), np.ascontiguousarray(uv, dtype=np.float32),
                      np.ascontiguousarray(n, dtype=np.float32))
    return _MESHES


_TEX = {}


def textures():
    """name -> uint8 (Ht, Wt, 3), rows in file order; every maximum is > 1"""
    if not _TEX:
        _TEX["t1x1"] = np.array([[[200, 120, 40]]], dtype=np.uint8)
        _TEX["t2x2"] = np.array([[[250, 20, 20], [20, 250, 20]], [[20, 20, 250], [240, 240, 30]]], dtype=np.uint8)
        k = np.arange(15).reshape(3, 5)
        _TEX["t5x3"] = np.stack([20 + 15 * k, 250 - 13 * k, 40 + 7 * ((k * 7) % 15)], -1).astype(np.uint8)
        y, x = np.mgrid[0:8, 0:8]
        on = ((x + y) % 2 == 0)[..., None]
        _TEX["check8"] = np.where(on, np.array([230, 210, 30]), np.array([30, 60, 220])).astype(np.uint8)
        y, x = np.mgrid[0:16, 0:64]
        _TEX["grad64x16"] = np.stack([3 + 4 * x, 8 + 16 * y, 255 - 4 * x], -1).astype(np.uint8)
    return _TEX


def face_texel(k):
    """the (file row, column) of the 5 x 3 texel that face k of "faceted" lies in"""
    return 3 - 1 - k // 5, k % 5


def _pose(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx, np.asarray(t, dtype=np.float64)


def _cam(size, f):
    W, H = size
    return np.array([[f, 0.0, W / 2.0 + 0.3], [0.0, 1.01 * f, H / 2.0 - 0.2], [0.0, 0.0, 1.0]])


def _case(name, mesh, tex, size, f, rot, t, shading="flat", ambient=0.5):
    R, tt = _pose(*rot, t)
    return dict(name=name, mesh=mesh, tex=tex, size=size, K=_cam(size, f), R=R, t=tt, shading=shading, ambient=ambient)


# poses chosen so that the oracle alone leaves at most 5 % of the covered pixels undecided (asserted in tests/test_render_tex.py)
CASES = (
    _case("quad_1x1", "quad", "t1x1", (32, 32), 120.0, (0.3, -0.2, 0.1), (2.0, -1.0, 330.0), "phong", 0.4),
    _case("quad_2x2", "quad", "t2x2", (33, 65), 150.0, (0.2, 0.5, 0.7), (1.0, 3.0, 300.0)),
    _case("quad_5x3", "quad", "t5x3", (67, 45), 220.0, (-0.4, 0.3, -0.2), (-3.0, 2.0, 320.0), "phong", 0.5),
    _case("quadover_5x3", "quadover", "t5x3", (67, 45), 220.0, (0.2, -0.3, 0.4), (2.0, -2.0, 330.0), "flat", 1.0),
    _case("quadover_check", "quadover", "check8", (32, 32), 130.0, (0.0, 0.4, -0.3), (0.0, 1.0, 340.0), "flat", 0.6),
    _case("box_check", "box", "check8", (67, 45), 160.0, (0.6, 0.7, 0.2), (3.0, -2.0, 330.0), "phong", 0.5),
    _case("box_grad", "box", "grad64x16", (33, 65), 140.0, (-0.5, 0.4, 1.0), (-1.0, 4.0, 300.0), "flat", 0.3),
    _case("quad_grad", "quad", "grad64x16", (67, 45), 230.0, (0.5, -0.4, 0.3), (1.0, -1.0, 330.0), "phong", 0.5),
    _case("slab_check", "slab", "check8", (67, 45), 120.0, (0.3, 0.0, 0.0), (0.0, 20.0, 400.0), "flat", 1.0),
    _case("ico80_check", "ico80", "check8", (67, 45), 150.0, (0.4, -0.6, 0.3), (-2.0, 1.0, 300.0), "phong", 0.5),
    _case("ico80_5x3", "ico80", "t5x3", (32, 32), 100.0, (1.2, 0.3, -0.8), (1.0, 0.0, 320.0), "flat", 0.5),
    _case("faceted_5x3", "faceted", "t5x3", (67, 45), 170.0, (0.5, -0.7, 0.2), (2.0, 1.0, 340.0), "flat", 1.0),
)


def case_args(c):
    v, f, uv, n = tex_meshes()[c["mesh"]]
    return dict(R=c["R"], t=c["t"], K=c["K"], verts=v, faces=f, uvs=uv, tex=textures()[c["tex"]], normals=n, size=c["size"], shading=c["shading"],
                ambient=c["ambient"])


# ---- the sampler -------------------------------------------------------------------------------------------------------------------
def interp_uv(w, uv, fa):
    """a + (w1 (c - a) + w2 (d - a)) of the faces' UVs (N,2), in uv's dtype"""
    a, c, d = uv[fa[:, 0]], uv[fa[:, 1]], uv[fa[:, 2]]
    return a + (w[1][:, None] * (c - a) + w[2][:, None] * (d - a))


def sample(tex, u, v, filt, f=np.float64, mut=None):
    """the texel (N,3) as bytes in dtype f of texture tex (uint8 (Ht,Wt,3), file row order) at (u, v) (N,)"""
    Ht, Wt = tex.shape[:2]
    if mut == "swapuv":
        u, v = v, u
    su, sv = u * f(Wt), v * f(Ht)
    wrap = mut == "noclamp"
    idx = lambda x, n: (np.mod(x, n) if wrap else np.clip(x, 0, n - 1)).astype(np.int64)      # noqa: E731
    row = lambda j: j if mut == "noflip" else Ht - 1 - j                                       # noqa: E731
    if filt == "nearest":
        fl = (lambda x: np.floor(x + f(0.5))) if mut == "roundidx" else np.floor
        return tex[row(idx(fl(sv), Ht)), idx(fl(su), Wt)].astype(f)
    h = f(0.0) if mut == "nohalf" else f(0.5)
    a, b = su - h, sv - h
    fa, fb = np.floor(a), np.floor(b)
    al, be = (a - fa)[:, None], (b - fb)[:, None]
    i0, i1, j0, j1 = idx(fa, Wt), idx(fa + f(1), Wt), idx(fb, Ht), idx(fb + f(1), Ht)
    T = tex.astype(f)
    t00, t10, t01, t11 = T[row(j0), i0], T[row(j0), i1], T[row(j1), i0], T[row(j1), i1]
    lo, hi = t00 + al * (t10 - t00), t01 + al * (t11 - t01)
    return lo + be * (hi - lo)


def adjacent_difference(tex):
    """D: the largest difference between horizontally or vertically adjacent texels, / 255"""
    T = tex.astype(np.float64)
    d = [np.abs(np.diff(T, axis=a)).max() for a in (0, 1) if T.shape[a] > 1]
    return (max(d) if d else 0.0) / 255.0


def _white_record(dtype, a, light):
    rec = RS.vertex_records(dtype, a["R"], a["t"], a["K"], a["verts"], np.ones((len(a["verts"]), 3)), a["normals"], light)
    rec["uniform"] = np.ones(3)
    return rec


def _face_terms(rec, a, fidx, xs, ys, eps, mut):
    """per sample on faces fidx: light_w, its tolerance term d_dot, (u, v), (E_u, E_v)"""
    e = EPS32
    faces, tex = a["faces"], a["tex"]
    Ht, Wt = tex.shape[:2]
    val, ex = RS.shade_points(rec, faces, fidx, xs, ys, a["shading"], a["ambient"], extras=True)
    tol_w = RS._tolerance(rec, faces, fidx, xs, ys, ex, eps, a["shading"], a["R"], a["t"], a["verts"], a["normals"])
    lw = ex["lw"]
    d_dot = tol_w / 255.0 - lw * 4.0 * e - 4.0 * e                      # white: cmax 1, span 0 -> tol = 255 (d_dot + lw 4 e + 4 e)
    fa = np.asarray(faces, dtype=np.int64)[fidx]
    w = ex["w"]
    if mut == "affineuv":
        w = RS.shade_points(rec, faces, fidx, xs, ys, a["shading"], a["ambient"], mut="affine", extras=True)[1]["w"]
    uv64 = np.asarray(a["uvs"]).astype(np.float64)
    uv = interp_uv(w, uv64, fa)
    x, y, z = rec["u"][fa], rec["v"][fa], 1.0 / rec["iz"][fa]
    area = np.abs((x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0]))
    inv_h = sum(np.sqrt((x[:, q] - x[:, p]) ** 2 + (y[:, q] - y[:, p]) ** 2) for p, q in ((1, 2), (2, 0), (0, 1))) / area
    dw = 6.0 * eps * (z.max(1) / z.min(1)) * inv_h + 8.0 * e             # (render_rgb_stages._tolerance's)
    span = np.abs(uv64[fa][:, :, None, :] - uv64[fa][:, None, :, :]).max((1, 2))      # (N,2)
    dims = np.array([Wt, Ht], dtype=np.float64)
    E = dims * (dw[:, None] * span + 4.0 * e * np.abs(uv)) + e * np.abs(uv * dims)
    if mut == "swapuv":
        E = E[:, ::-1] * (dims / dims[::-1])
    return lw, d_dot, uv, E


def _values(a, filt, lw, d_dot, uv, E, mut):
    """-> (v (N,3), tol (N,), decided (N,), candidates: per sample None or a list of (value (3,), tol))"""
    e = EPS32
    tex = a["tex"]
    Ht, Wt = tex.shape[:2]
    cmax = float(tex.max()) / 255.0
    texel = sample(tex, uv[:, 0], uv[:, 1], filt, np.float64, mut)
    v = lw[:, None] * texel
    tol = 255.0 * (d_dot * cmax + lw * 4.0 * e + 4.0 * e)
    n = len(lw)
    if filt == "linear":
        tol = tol + 255.0 * lw * ((E[:, 0] + E[:, 1]) * adjacent_difference(tex) + 8.0 * e)
        return v, tol, np.ones(n, dtype=bool), [None] * n, texel
    us, vs = (uv[:, 1], uv[:, 0]) if mut == "swapuv" else (uv[:, 0], uv[:, 1])
    shift = 0.5 if mut == "roundidx" else 0.0
    su, sv = us * Wt + shift, vs * Ht + shift
    near = lambda s, E_, n_: (np.abs(s - np.clip(np.round(s), 1, max(n_ - 1, 1))) <= E_) & (n_ > 1)      # noqa: E731
    und = near(su, E[:, 0], Wt) | near(sv, E[:, 1], Ht)
    cands = [None] * n
    for k in np.nonzero(und)[0]:
        lst = []
        for i in range(int(np.floor(su[k] - E[k, 0])), int(np.floor(su[k] + E[k, 0])) + 1):
            for j in range(int(np.floor(sv[k] - E[k, 1])), int(np.floor(sv[k] + E[k, 1])) + 1):
                ii, jj = (i % Wt, j % Ht) if mut == "noclamp" else (min(max(i, 0), Wt - 1), min(max(j, 0), Ht - 1))
                lst.append((lw[k] * tex[jj if mut == "noflip" else Ht - 1 - jj, ii].astype(np.float64), tol[k]))
        cands[k] = lst
    return v, tol, ~und, cands, texel


def oracle_tex(R, t, K, verts, faces, uvs, tex, normals, size, filt="nearest", shading="phong", ambient=0.5, light=(0, 0, 0), mut=None):
    """The float64 statement at (W, H), background 0, ssaa 1 (SSAA and the other backgrounds are pinned by exact equalities on the
    device).  -> render_rgb_stages.check_band's dict (v, decided, tol, covered, candidates, lo, hi) + u8, texel (H,W,3) (the decided
    pixels' texel bytes; nearest), eps."""
    a = dict(R=R, t=t, K=K, verts=verts, faces=faces, uvs=uvs, tex=tex, normals=normals, shading=shading, ambient=ambient)
    W, H = size
    rec = _white_record(np.float64, a, light)
    if not (rec["iz"] > 0).all():
        raise ValueError("a vertex at Z <= 0: outside the render rule")
    o = S.oracle_render(R, t, K, verts, faces, (W, H))
    eps = o["eps"]
    win_iz, win_f, top_iz, top_f, sec_iz, lo_faces = RS._winners(rec, faces, (W, H), eps)
    covered = top_f >= 0
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(sec_iz > 0, 1.0 / sec_iz, np.inf) - np.where(top_iz > 0, 1.0 / top_iz, 0.0)
    decided = o["decided"] & ((~covered & (win_f < 0)) | (covered & (win_f == top_f) & (gap > o["tol"])))
    val, tol, texel = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W, 3))
    cands = {}
    ys, xs = np.nonzero(win_f >= 0)
    if ys.size:
        lw, d_dot, uv, E = _face_terms(rec, a, win_f[ys, xs], xs, ys, eps, mut)
        v, tl, dec, cl, tx = _values(a, filt, lw, d_dot, uv, E, mut)
        val[ys, xs], tol[ys, xs], texel[ys, xs] = np.clip(v, 0.0, 255.0), tl, tx
        for k in np.nonzero(~dec & decided[ys, xs])[0]:                # the geometry is decided, the texel is not
            cands[(ys[k], xs[k])] = cl[k]
        decided[ys, xs] &= dec
    decided &= np.isfinite(tol) & np.isfinite(val).all(-1)
    und = ~decided
    hi_cov = np.isfinite(o["d_hi"])
    for yy, xx in zip(*np.nonzero(und & ~hi_cov)):                     # the background, unless eroded coverage is certain
        cands.setdefault((yy, xx), []).append((np.zeros(3), 0.0))
    for fi, sl, lom in lo_faces:                                       # any face that covers the sample in the dilated sense
        m = lom & und[sl]
        if not m.any():
            continue
        yy, xx = np.nonzero(m)
        yy, xx = yy + sl[0].start, xx + sl[1].start
        lw, d_dot, uv, E = _face_terms(rec, a, np.full(yy.shape, fi), xx, yy, eps, mut)
        v, tl, dec, cl, _ = _values(a, filt, np.nan_to_num(lw), np.nan_to_num(d_dot, nan=1.0, posinf=1.0), np.nan_to_num(uv), np.nan_to_num(E, posinf=1e9), mut)
        tl = np.where(np.isfinite(tl), tl, 255.0)
        for k in range(yy.size):
            cands.setdefault((yy[k], xx[k]), []).extend(cl[k] if cl[k] is not None else [(np.clip(v[k], 0.0, 255.0), tl[k])])
    for key in [k for k in cands if decided[k]]:
        del cands[key]
    return {"v": val, "u8": RS.quantise(val), "decided": decided, "tol": tol, "covered": covered, "candidates": cands, "lo": val - 0.5 - tol[..., None],
            "hi": val + 0.5 + tol[..., None], "eps": eps, "texel": texel}


# ---- the device's arithmetic, restated in fp32 ----------------------------------------------------------------------------------------
def render_tex_f32(R, t, K, verts, faces, uvs, tex, normals, size, filt="nearest", shading="phong", ambient=0.5, light=(0, 0, 0)):
    """cp_render_rgb_tex's arithmetic in numpy float32 (ssaa 1, background 0) -> (rgb uint8 (H,W,3), face (H,W))"""
    f32 = np.float32
    W, H = size
    a = dict(R=R, t=t, K=K, verts=verts, faces=faces, normals=normals)
    rec = _white_record(f32, a, light)
    rec["uniform"] = np.ones(3, dtype=f32)
    best, face = RS.winners_f32(rec, faces, (W, H))
    img = np.zeros((H, W, 3), dtype=np.uint8)
    ys, xs = np.nonzero(face >= 0)
    if ys.size:
        _, ex = RS.shade_points(rec, faces, face[ys, xs], xs, ys, shading, f32(ambient), extras=True)
        fa = np.asarray(faces, dtype=np.int64)[face[ys, xs]]
        uv = interp_uv(ex["w"], np.asarray(uvs, dtype=f32), fa)
        texel = sample(tex, uv[:, 0], uv[:, 1], filt, f32)
        img[ys, xs] = RS.quantise(f32(255) * (ex["lw"][:, None] * (texel / f32(255))))
    return img, face
