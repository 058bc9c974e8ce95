"""Row N14 (shaded RGB frames), the stages the device is pinned by.  Nothing here reads the reference; everything is numpy.

  meshes            the fixture's coloured triangle meshes, built in closed form
  uniforms          u_mv, u_nm as the reference's _calc_model_view / _calc_normal_matrix give them (restated; the fixture records
                    the reference's own and the two are compared in tests/test_render_rgb.py)
  oracle_rgb        the float64 statement of the render rule: per pixel the real value v = 255 * light_w * colour, whether the pixel is
                    DECIDED, the derived tolerance tol_c, and for the other pixels the values some candidate surface allows
  render_f32        the fp32 numpy restatement of the device's arithmetic (csrc/render_rgb.hip), uint8
  ssaa_average      the integer averaging rule;  check_band: a uint8 frame against the oracle
  MUTATIONS         eight mutations of the statement, for the checker's own test

Render rule (renderer_py.py:24-105, 422-518 read as a rule).  Coverage and the front-most surface: tests/vsd_stages.py (sample at
the pixel centre, no culling, zero-area triangles skipped), built on its dilated / eroded edges with the same eps and tol_d.  Over the
winning triangle the shader's varyings are interpolated perspective-correctly (weights E_i / Z_i / sum_j E_j / Z_j, E_i the edge
function opposite vertex i):  v_color;  v_L = normalize(light - eye_pos) per VERTEX;  v_normal = normalize(u_nm * vec4(a_normal, 1)).xyz
(a 4-vector normalisation).  flat: n = the face normal turned towards the viewer;  phong: n = the interpolated v_normal.
light_w = min(1, ambient + max(dot(normalize(v_L), normalize(n)), 0));  v = 255 * light_w * v_color;  uint8 = np.round(v).

A sample is DECIDED when its coverage is decided (vsd_stages), its winner is unambiguous (the runner-up among the triangles that cover
it in the dilated sense is another face only if its depth is further than tol_d away, and the winner is the same in the strict and
in the dilated sense), and -- after SSAA -- every contributing sample is decided.

tol_c (grey levels; derived, not tuned; e = 2^-24).  The device evaluates the weights from fp32 screen coordinates: an error eps of the
edge distances (vsd_stages' eps) moves the screen-affine weight of vertex i by <= 3 eps / h_i (h_i the altitude), the perspective
division by 1 / Z_i and the renormalisation amplify the sum of the moves by <= 2 Zmax / Zmin, and the fp32 products and quotients
of the weights add 8 e:
    dw = 6 eps (Zmax / Zmin) sum_i 1 / h_i + 8 e                                   (sum of |weight errors|)
An interpolated attribute A moves by dw * span(A) (the weights sum to 1) plus its vertices' own errors:
    eye_pos = R p + t in fp32 (three fma):  d_eye = 4 e (|R| |p| + |t|);   v_L: d_eye / |light - eye| + 4 e per vertex;
    v_normal: (4 e (|c| |n| + |n| + 1)) / |u_nm (n, 1)| + 4 e per vertex (c = R^-1 t: the fourth component 1 - c . n cancels);
    the flat normal, from two edges u, v of eye positions: (2 d_eye (|u| + |v|) + 4 e |u| |v|) / |u x v|.
Normalising a vector of length |A| turns an error dA into a direction error <= 2 dA / |A| + 3 e, so with dL, dN the errors of the
interpolated vectors:
    d_dot = 2 dL / |L| + 2 dN / |N| + 10 e;   light_w is 1-Lipschitz in the dot product;
    tol_c = 255 (d_dot max(colour) + light_w (dw span(colour) + 4 e) + 4 e).
With SSAA the band is stated on the integers: a sample may quantise to any integer in [round(v - tol_c), round(v + tol_c)] (one value
unless v lies within tol_c of a rounding boundary); these are summed and sent through the monotone averaging rule, which gives the
interval the pixel must lie in (one value for nearly every pixel).  A pixel is decided when every contributing sample is."""
import numpy as np

from tests import vsd_stages as S

EPS32 = S.EPS32
TILE = S.TILE
MUTATIONS = ("affine", "noflip", "noclamp", "halfup", "no255", "norm3", "pixelL", "avgfirst")


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def _pos_colors(v, lo=30.0, hi=250.0):
    """0..255 colours that vary smoothly with position"""
    v = np.asarray(v, dtype=np.float64)
    span = v.max(0) - v.min(0)
    span[span == 0] = 1.0
    return np.round(lo + (hi - lo) * (v - v.min(0)) / span).astype(np.uint8)


def _radial_normals(v):
    v = np.asarray(v, dtype=np.float64)
    c = v - v.mean(0)
    n = np.linalg.norm(c, axis=1, keepdims=True)
    n[n == 0] = 1.0
    return (c / n).astype(np.float32)


MESH_NAMES = ("tri3", "quad", "box", "halfbox", "ico80", "ico1280", "zeroarea", "coincident", "grey", "icofloat", "slab")
_MESHES = {}


def meshes():
    """name -> (verts float32 (V,3) mm, faces int32 (F,3), colours (V,3) uint8 / float32 / None, normals float32 (V,3))"""
    if not _MESHES:
        out = {}
        v = np.array([[-60.0, -35.0, 0.0], [55.0, -20.0, 0.0], [5.0, 50.0, 0.0]])
        out["tri3"] = (v, np.array([[0, 1, 2]], dtype=np.int32), np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], dtype=np.uint8),
                       np.tile(np.array([[0.2, -0.1, -1.0]]) / np.linalg.norm([0.2, -0.1, -1.0]), (3, 1)))
        v = np.array([[-40.0, -30.0, 0.0], [40.0, -30.0, 0.0], [40.0, 30.0, 0.0], [-40.0, 30.0, 0.0]])
        out["quad"] = (v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), np.array([[200, 120, 40]] * 4, dtype=np.uint8),
                       np.tile(np.array([[0.0, 0.0, -1.0]]), (4, 1)))
        for name, open_top in (("box", False), ("halfbox", True), ("grey", False)):
            v, f = S._box(80.0, 60.0, 40.0, open_top=open_top)
            out[name] = (v, f, None if name == "grey" else _pos_colors(v), _radial_normals(v))
        for name, level in (("ico80", 1), ("ico1280", 3), ("icofloat", 1)):
            v, f = S._icosphere(level, 50.0)
            col = _pos_colors(v)
            out[name] = (v, f, (col.astype(np.float32) / np.float32(256.0)) if name == "icofloat" else col, (v / 50.0).astype(np.float32))
        v, f = S._box(70.0, 50.0, 30.0)
        out["zeroarea"] = (v, np.concatenate([f, np.array([[0, 0, 5], [3, 6, 6], [2, 2, 2]], dtype=np.int32)], 0), _pos_colors(v), _radial_normals(v))
        v = np.array([[-50.0, -40.0, 0.0], [50.0, -30.0, 0.0], [0.0, 45.0, 0.0]])
        out["coincident"] = (np.concatenate([v, v], 0), np.array([[3, 4, 5], [0, 1, 2]], dtype=np.int32),
                             np.array([[250, 20, 20]] * 3 + [[20, 20, 250]] * 3, dtype=np.uint8), np.tile(np.array([[0.0, 0.0, -1.0]]), (6, 1)))
        # a long slab seen at a grazing angle: perspective-correct and screen-affine interpolation differ by many grey levels
        v = np.array([[-30.0, 0.0, -150.0], [30.0, 0.0, -150.0], [30.0, 0.0, 150.0], [-30.0, 0.0, 150.0]])
        out["slab"] = (v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), np.array([[250, 250, 250], [250, 250, 250], [10, 10, 10], [10, 10, 10]], dtype=np.uint8),
                       np.tile(np.array([[0.0, -1.0, 0.0]]), (4, 1)))
        for k, (v, f, c, n) in out.items():
            _MESHES[k] = (np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32), c,
                          np.ascontiguousarray(n, dtype=np.float32))
    return _MESHES


def colors01(colors, n_verts, surf_color=None, no255=False):
    """add_object's colour rule in float64: surf_color, else the mesh's colours (/ 255 when their maximum is > 1), else 0.5 grey"""
    if surf_color is not None:
        return np.tile(np.asarray(surf_color, dtype=np.float64).reshape(1, 3), (n_verts, 1))
    if colors is None:
        return np.full((n_verts, 3), 0.5)
    c = np.asarray(colors).astype(np.float32).astype(np.float64)
    if c.max() > 1.0 and not no255:
        c = c / 255.0
    return c


# ---- the uniforms ---------------------------------------------------------------------------------------------------------------------
def uniforms(R, t):
    """(u_mv, u_nm) as numpy 4x4 arrays in the reference's row-vector layout: eye = [p, 1] @ u_mv, normal4 = [n, 1] @ u_nm.
    mat_view = (yz_flip @ [R t; 0 1])^T in float32 as render_object builds it; u_mv = mat_model @ mat_view; u_nm = inv(u_mv)^T."""
    view_cv = np.eye(4, dtype=np.float32)
    view_cv[:3, :3], view_cv[:3, 3] = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3)
    flip = np.eye(4, dtype=np.float32)
    flip[1, 1], flip[2, 2] = -1, -1
    u_mv = np.dot(np.eye(4, dtype=np.float32), flip.dot(view_cv).T)
    return u_mv, np.linalg.inv(u_mv).T


# ---- shading of a list of (face, sample) points -----------------------------------------------------------------------------------------
def vertex_records(dtype, R, t, K, verts, col01, normals, light_gl, u_mv=None, u_nm=None, mut=None):
    """per-vertex records in `dtype`.  float64: the statement, in the shader's eye frame from u_mv / u_nm.  float32: the device's
    arithmetic (rgb_pose_kernel + rgb_vertex_kernel) in the poses' camera frame."""
    f = dtype
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    rec = {"dtype": f, "sk": 1.0 if (K[0, 0] > 0) == (K[1, 1] > 0) else -1.0}
    if f == np.float64:
        u, v, Z, Sc = S.screen(R, t, K, verts)
        rec.update(u=u, v=v, iz=1.0 / Z, S=Sc)
        if u_mv is None:
            u_mv, u_nm = uniforms(R, t)
        ph = np.concatenate([np.asarray(verts, dtype=np.float64), np.ones((len(verts), 1))], 1)
        eye = (ph @ np.asarray(u_mv, dtype=np.float64))[:, :3]
        light = np.asarray(light_gl, dtype=np.float64).reshape(3)
        n4 = np.concatenate([np.asarray(normals, dtype=np.float64), np.ones((len(verts), 1))], 1) @ np.asarray(u_nm, dtype=np.float64)
        nlen = np.linalg.norm(n4[:, :3] if mut == "norm3" else n4, axis=1, keepdims=True)
        rec.update(n4len=np.linalg.norm(n4, axis=1))
        vn = n4[:, :3] / nlen
    else:
        Kc = np.array([[K[0, 0], 0.0, K[0, 2]], [0.0, K[1, 1], K[1, 2]], [0.0, 0.0, 1.0]])
        P = (Kc @ np.concatenate([R, t[:, None]], 1)).astype(f)
        p = np.asarray(verts, dtype=f)
        row = lambda M, r: ((M[r, 0] * p[:, 0] + M[r, 3]) + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]     # noqa: E731
        pw = row(P, 2)
        rec.update(u=row(P, 0) / pw, v=row(P, 1) / pw, iz=f(1.0) / pw)
        RT = np.concatenate([R, t[:, None]], 1).astype(f)
        eye = np.stack([row(RT, 0), row(RT, 1), row(RT, 2)], 1)
        light = (np.asarray(light_gl, dtype=np.float64).reshape(3) * np.array([1.0, -1.0, -1.0])).astype(f)
        N = np.linalg.inv(R).T
        c = (N.T @ t).astype(f)
        N = N.astype(f)
        nr = np.asarray(normals, dtype=f)
        nx = [(N[r, 0] * nr[:, 0] + N[r, 1] * nr[:, 1]) + N[r, 2] * nr[:, 2] for r in range(3)]
        nw = f(1.0) - ((c[0] * nr[:, 0] + c[1] * nr[:, 1]) + c[2] * nr[:, 2])
        nlen = np.sqrt(((nx[0] * nx[0] + nx[1] * nx[1]) + nx[2] * nx[2]) + nw * nw)
        vn = np.stack(nx, 1) / nlen[:, None]
    Lv = light[None, :] - eye
    rec.update(eye=eye, light=light, L=Lv / np.sqrt((Lv[:, 0] * Lv[:, 0] + Lv[:, 1] * Lv[:, 1]) + Lv[:, 2] * Lv[:, 2])[:, None],
               vn=vn.astype(f), col=np.asarray(col01, dtype=f))
    return rec


def shade_points(rec, faces, fidx, px, py, shading, ambient, mut=None, extras=False):
    """the real value 255 * light_w * colour (N,3) of samples (px, py) (integer sample indices) on faces fidx, in rec's dtype"""
    f = rec["dtype"]
    fa = np.asarray(faces, dtype=np.int64)[fidx]
    i0, i1, i2 = fa[:, 0], fa[:, 1], fa[:, 2]
    fx0 = ((px // TILE) * TILE + 0.5).astype(f)
    fy0 = ((py // TILE) * TILE + 0.5).astype(f)
    qx, qy = (px % TILE).astype(f), (py % TILE).astype(f)
    u, v, iz = rec["u"], rec["v"], rec["iz"]
    ax, ay, cx, cy, dx, dy = u[i0] - fx0, v[i0] - fy0, u[i1] - fx0, v[i1] - fy0, u[i2] - fx0, v[i2] - fy0
    area = (cx - ax) * (dy - ay) - (dx - ax) * (cy - ay)
    e0 = (dx - cx) * (qy - cy) - (dy - cy) * (qx - cx)
    e1 = (ax - dx) * (qy - dy) - (ay - dy) * (qx - dx)
    e2 = (cx - ax) * (qy - ay) - (cy - ay) * (qx - ax)
    if mut == "affine":
        p0, p1, p2 = e0, e1, e2
    else:
        p0, p1, p2 = e0 * iz[i0], e1 * iz[i1], e2 * iz[i2]
    ps = (p0 + p1) + p2
    w = [p0 / ps, p1 / ps, p2 / ps]
    mix = lambda A: (w[0][:, None] * A[i0] + w[1][:, None] * A[i1]) + w[2][:, None] * A[i2]      # noqa: E731
    eye = rec["eye"]
    if mut == "pixelL":
        Lp = rec["light"][None, :] - mix(eye)
    else:
        Lp = mix(rec["L"])
    if shading == "phong":
        Np = mix(rec["vn"])
    else:
        a, b = eye[i1] - eye[i0], eye[i2] - eye[i0]
        Np = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        if mut != "noflip":
            if f == np.float64:
                away = (Np * eye[i0]).sum(1) > 0                          # the viewer is at the origin of the eye frame
            else:
                away = (area > 0) == (rec["sk"] > 0)
            Np = np.where(away[:, None], -Np, Np)
    ll = np.sqrt((Lp[:, 0] * Lp[:, 0] + Lp[:, 1] * Lp[:, 1]) + Lp[:, 2] * Lp[:, 2])
    nl = np.sqrt((Np[:, 0] * Np[:, 0] + Np[:, 1] * Np[:, 1]) + Np[:, 2] * Np[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        dt = ((Lp[:, 0] * Np[:, 0] + Lp[:, 1] * Np[:, 1]) + Lp[:, 2] * Np[:, 2]) / (ll * nl)
    lw = f(ambient) + np.where(dt > 0, dt, f(0))
    if mut != "noclamp":
        lw = np.minimum(lw, f(1))
    # a uniform colour (surf_color, or the grey of a mesh without colours) is a constant of the draw, not interpolated
    # (the device forms a + (w1 (c - a) + w2 (d - a)): three equal colours give that colour exactly)
    C = rec["col"]
    col = (C[i0] + (w[1][:, None] * (C[i1] - C[i0]) + w[2][:, None] * (C[i2] - C[i0]))) if rec.get("uniform") is None else np.tile(np.asarray(rec["uniform"], dtype=f).reshape(1, 3), (len(lw), 1))
    val = f(255) * (lw[:, None] * col)
    if extras:
        return val, {"w": w, "ll": ll, "nl": nl, "lw": lw, "col": col, "i": (i0, i1, i2)}
    return val


def quantise(val, mut=None):
    v = np.asarray(val)
    q = np.floor(v + 0.5) if mut == "halfup" else np.round(v)
    return np.clip(np.nan_to_num(q, nan=0.0), 0, 255).astype(np.uint8)


def ssaa_average(img, f):
    """(fH, fW, 3) uint8 -> (H, W, 3) uint8: f x f samples summed as integers; (s + 2) >> 2, or round-half-even of s / 16"""
    if f == 1:
        return np.asarray(img, dtype=np.uint8)
    a = np.asarray(img).astype(np.int64)
    fh, fw = a.shape[0] // f, a.shape[1] // f
    s = a.reshape(fh, f, fw, f, -1).sum((1, 3))
    if f == 2:
        return ((s + 2) >> 2).astype(np.uint8)
    q, r = s >> 4, s & 15
    return (q + ((r > 8) | ((r == 8) & ((q & 1) == 1)))).astype(np.uint8)


# ---- the float64 statement ------------------------------------------------------------------------------------------------------------
def _winners(rec, faces, size, eps):
    """per sample: the strict winner (smallest index among equal 1 / Z), the dilated top face and the best 1 / Z of ANOTHER dilated face"""
    W, H = size
    u, v, iz = rec["u"], rec["v"], rec["iz"]
    win_iz, win_f = np.zeros((H, W)), np.full((H, W), -1, dtype=np.int64)
    top_iz, top_f, sec_iz = np.zeros((H, W)), np.full((H, W), -1, dtype=np.int64), np.zeros((H, W))
    lo_faces = []
    for fi, (a, b, c) in enumerate(np.asarray(faces, dtype=np.int64)):
        x, y, z = u[[a, b, c]], v[[a, b, c]], iz[[a, b, c]]
        area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
        if area == 0.0:
            continue
        x0, x1 = max(0, int(np.floor(x.min() - 0.5 - eps))), min(W - 1, int(np.ceil(x.max() - 0.5 + eps)))
        y0, y1 = max(0, int(np.floor(y.min() - 0.5 - eps))), min(H - 1, int(np.ceil(y.max() - 0.5 + eps)))
        if x1 < x0 or y1 < y0:
            continue
        X, Y = (np.arange(x0, x1 + 1) + 0.5)[None, :], (np.arange(y0, y1 + 1) + 0.5)[:, None]
        dist, izp = np.full((y1 - y0 + 1, x1 - x0 + 1), np.inf), 0.0
        for i, (p, q) in enumerate(((1, 2), (2, 0), (0, 1))):
            ex, ey = x[q] - x[p], y[q] - y[p]
            E = ex * (Y - y[p]) - ey * (X - x[p])
            dist = np.minimum(dist, E * (np.sign(area) / np.sqrt(ex * ex + ey * ey)))
            izp = izp + E * (z[i] / area)
        sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        strict, lo = (dist >= 0) & (izp > 0), (dist >= -eps) & (izp > 0)
        if not lo.any():
            continue
        lo_faces.append((fi, sl, lo))
        up = strict & (izp > win_iz[sl])
        win_iz[sl] = np.where(up, izp, win_iz[sl])
        win_f[sl] = np.where(up, fi, win_f[sl])
        new_top = lo & (izp > top_iz[sl])
        sec_iz[sl] = np.where(new_top, top_iz[sl], np.where(lo & (izp > sec_iz[sl]), izp, sec_iz[sl]))
        top_iz[sl] = np.where(new_top, izp, top_iz[sl])
        top_f[sl] = np.where(new_top, fi, top_f[sl])
    return win_iz, win_f, top_iz, top_f, sec_iz, lo_faces


def _tolerance(rec, faces, fidx, px, py, ex, eps, shading, R, t, verts, normals):
    """tol_c of the module docstring for the shaded points (N,)"""
    e = EPS32
    fa = np.asarray(faces, dtype=np.int64)[fidx]
    u, v, iz = rec["u"], rec["v"], rec["iz"]
    x, y, z = u[fa], v[fa], 1.0 / iz[fa]                                   # (N,3)
    area = np.abs((x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0]))
    inv_h = sum(np.sqrt((x[:, q] - x[:, p]) ** 2 + (y[:, q] - y[:, p]) ** 2) for p, q in ((1, 2), (2, 0), (0, 1))) / area
    dw = 6.0 * eps * (z.max(1) / z.min(1)) * inv_h + 8.0 * e
    span = lambda A: np.abs(A[fa][:, :, None, :] - A[fa][:, None, :, :]).max((1, 2)).max(-1)      # noqa: E731
    Rm, tv = np.abs(np.asarray(R, dtype=np.float64).reshape(3, 3)), np.abs(np.asarray(t, dtype=np.float64).reshape(3))
    p = np.abs(np.asarray(verts, dtype=np.float64))
    d_eye = 4.0 * e * (np.linalg.norm(Rm) * np.linalg.norm(p, axis=1).max() + np.linalg.norm(tv))
    eye = rec["eye"]
    d_vL = (d_eye / np.linalg.norm(rec["light"][None, :] - eye, axis=1) + 4.0 * e)[fa].max(1)
    dL = dw * np.sqrt(3.0) * span(rec["L"]) + d_vL
    if shading == "phong":
        c = np.linalg.norm(np.linalg.inv(np.asarray(R, dtype=np.float64).reshape(3, 3)) @ np.asarray(t, dtype=np.float64).reshape(3))
        nn = np.linalg.norm(np.asarray(normals, dtype=np.float64), axis=1)
        d_vn = ((4.0 * e * (c * nn + nn + 1.0)) / rec["n4len"] + 4.0 * e)[fa].max(1)
        dN = dw * np.sqrt(3.0) * span(rec["vn"]) + d_vn
    else:
        a, b = eye[fa[:, 1]] - eye[fa[:, 0]], eye[fa[:, 2]] - eye[fa[:, 0]]
        la, lb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
        dN = 2.0 * d_eye * (la + lb) + 4.0 * e * la * lb                 # (absolute, against |u x v| = ex["nl"])
    with np.errstate(divide="ignore", invalid="ignore"):
        d_dot = 2.0 * dL / ex["ll"] + 2.0 * dN / ex["nl"] + 10.0 * e
    cmax = np.abs(rec["col"][fa]).max((1, 2))
    tol = 255.0 * (d_dot * cmax + ex["lw"] * (dw * span(rec["col"]) + 4.0 * e) + 4.0 * e)
    return np.where(np.isfinite(tol), tol, np.inf)


def oracle_rgb(R, t, K, verts, faces, colors, normals, size, shading="phong", ambient=0.5, light=(0, 0, 0), bg=(0, 0, 0), surf_color=None,
               ssaa=1, u_mv=None, u_nm=None, mut=None, want_candidates=True):
    """The statement at output size (W, H).  -> dict: v (H,W,3) float64, the real value of decided pixels at ssaa = 1 / the exact
    expected uint8 value at ssaa > 1;  u8 (H,W,3) the statement's own frame;  decided (H,W) bool;  tol (H,W);  covered (H,W) bool (in
    the dilated sense);  candidates: {(y, x): (values (n,3), tolerances (n,))} for the undecided pixels at ssaa = 1 (None = background
    allowed is flagged by a row of NaN tolerance -1);  lo, hi (H,W,3): the interval any candidate allows (every ssaa)."""
    W, H = size
    f = int(ssaa)
    sw, sh = f * W, f * H
    Kf = np.asarray(K, dtype=np.float64).reshape(3, 3).copy()
    Kf[0, 0] *= f; Kf[1, 1] *= f; Kf[0, 2] *= f; Kf[1, 2] *= f           # noqa: E702
    col = colors01(colors, len(verts), surf_color, no255=(mut == "no255"))
    rec = vertex_records(np.float64, R, t, Kf, verts, col, normals, light, u_mv, u_nm, mut)
    rec["uniform"] = col[0] if (colors is None or surf_color is not None) else None
    if not (rec["iz"] > 0).all():
        raise ValueError("a vertex at Z <= 0: outside the render rule")
    o = S.oracle_render(R, t, Kf, verts, faces, (sw, sh))
    eps = o["eps"]
    win_iz, win_f, top_iz, top_f, sec_iz, lo_faces = _winners(rec, faces, (sw, sh), eps)
    covered = top_f >= 0
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(sec_iz > 0, 1.0 / sec_iz, np.inf) - np.where(top_iz > 0, 1.0 / top_iz, 0.0)
    decided = o["decided"] & ((~covered & (win_f < 0)) | (covered & (win_f == top_f) & (gap > o["tol"])))
    bgq = np.clip(np.round(255.0 * np.asarray(bg, dtype=np.float64)), 0, 255)
    val = np.tile(bgq.reshape(1, 1, 3), (sh, sw, 1)).astype(np.float64)
    tol = np.zeros((sh, sw))
    ys, xs = np.nonzero(win_f >= 0)
    if ys.size:
        vv, ex = shade_points(rec, faces, win_f[ys, xs], xs, ys, shading, ambient, mut, extras=True)
        val[ys, xs] = np.clip(vv, 0.0, 255.0)
        tol[ys, xs] = _tolerance(rec, faces, win_f[ys, xs], xs, ys, ex, eps, shading, R, t, verts, normals)
    decided &= np.isfinite(tol) & np.isfinite(val).all(-1)
    # what the undecided samples may take: the background (unless eroded coverage is certain) or any dilated face's value
    lo, hi = val - 0.5 - tol[..., None], val + 0.5 + tol[..., None]
    cands = {}
    und = ~decided
    if und.any():
        hi_cov = np.isfinite(o["d_hi"])
        lo[und], hi[und] = np.inf, -np.inf
        for yy, xx in zip(*np.nonzero(und & ~hi_cov)):
            lo[yy, xx], hi[yy, xx] = np.minimum(lo[yy, xx], bgq - 0.5), np.maximum(hi[yy, xx], bgq + 0.5)
            cands.setdefault((yy, xx), []).append((bgq, 0.0))
        for fi, sl, lom in lo_faces:
            m = lom & und[sl]
            if not m.any():
                continue
            yy, xx = np.nonzero(m)
            yy, xx = yy + sl[0].start, xx + sl[1].start
            vv, ex = shade_points(rec, faces, np.full(yy.shape, fi), xx, yy, shading, ambient, mut, extras=True)
            vv = np.clip(np.nan_to_num(vv, nan=0.0), 0.0, 255.0)
            tt = _tolerance(rec, faces, np.full(yy.shape, fi), xx, yy, ex, eps, shading, R, t, verts, normals)
            tt = np.where(np.isfinite(tt), tt, 255.0)
            lo[yy, xx] = np.minimum(lo[yy, xx], vv - 0.5 - tt[:, None])
            hi[yy, xx] = np.maximum(hi[yy, xx], vv + 0.5 + tt[:, None])
            if want_candidates and f == 1:
                for k in range(yy.size):
                    cands.setdefault((yy[k], xx[k]), []).append((vv[k], tt[k]))
    if f == 1:
        return {"v": val, "u8": quantise(val, mut), "decided": decided, "tol": tol, "covered": covered, "candidates": cands, "lo": lo, "hi": hi,
                "eps": eps, "depth": o}
    # SSAA: quantise every sample, then the integer rule.  A sample whose v lies within tol_c of a rounding boundary may quantise either
    # way: per sample the integers [round(v - tol_c), round(v + tol_c)], summed, through the (monotone) rule give the pixel's interval.
    if mut == "avgfirst":
        u8 = quantise(val.reshape(H, f, W, f, 3).mean((1, 3)), mut)
    else:
        u8 = ssaa_average(quantise(val, mut), f)
    blk = lambda a, fn: fn(fn(a.reshape((H, f, W, f) + a.shape[2:]), 3), 1)      # noqa: E731
    t3 = np.where(np.isfinite(tol), tol, 255.0)[..., None]
    if mut == "avgfirst":
        ilo = quantise(np.clip(val - t3, 0, 255).reshape(H, f, W, f, 3).mean((1, 3))).astype(np.float64)
        ihi = quantise(np.clip(val + t3, 0, 255).reshape(H, f, W, f, 3).mean((1, 3))).astype(np.float64)
    else:
        ilo = ssaa_average(quantise(np.clip(val - t3, 0, 255), mut), f).astype(np.float64)
        ihi = ssaa_average(quantise(np.clip(val + t3, 0, 255), mut), f).astype(np.float64)
    return {"v": u8.astype(np.float64), "u8": u8, "decided": blk(decided, np.all), "tol": np.zeros((H, W)), "covered": blk(covered, np.any),
            "candidates": {}, "lo": blk(np.floor(lo + 0.5), np.mean) - 1.0, "hi": blk(np.ceil(hi - 0.5), np.mean) + 1.0, "eps": eps, "depth": o,
            "ilo": ilo, "ihi": ihi}


def undecided_share(o):
    n = int(o["covered"].sum())
    return float((~o["decided"] & o["covered"]).sum()) / n if n else 0.0


def check_band(img, o):
    """a uint8 frame (H,W,3) against oracle_rgb's dict -> (ok, worst (|u8 - v| - 0.5) / tol_c over the decided covered pixels with
    tol_c > 0, the share of decided pixels equal to round(v) outright, the number of pixels outside what they may take)"""
    g = np.asarray(img).astype(np.float64)
    dec = o["decided"]
    diff = np.abs(g - o["v"]).max(-1)
    if "ilo" in o:                                                     # SSAA: the integer interval of the module docstring
        bad_dec = dec & ~((g >= o["ilo"]) & (g <= o["ihi"])).all(-1)
    else:
        bad_dec = dec & ~(diff <= 0.5 + o["tol"])
    und_bad = 0
    ys, xs = np.nonzero(~dec)
    for yy, xx in zip(ys, xs):
        c = o["candidates"].get((yy, xx))
        if c is None:
            fits = bool(((g[yy, xx] >= o["lo"][yy, xx]) & (g[yy, xx] <= o["hi"][yy, xx])).all())
        else:
            fits = any((np.abs(g[yy, xx] - vv) <= 0.5 + tt).all() for vv, tt in c)
        und_bad += 0 if fits else 1
    sel = dec & o["covered"] & (o["tol"] > 0)
    ratio = float(((diff[sel] - 0.5) / o["tol"][sel]).max()) if sel.any() else -np.inf
    equal = float((g[dec] == np.round(o["v"][dec])).all(-1).mean()) if dec.any() else 1.0
    nbad = int(bad_dec.sum()) + und_bad
    return nbad == 0, ratio, equal, nbad


# ---- the device's arithmetic, restated in fp32 ----------------------------------------------------------------------------------------
def winners_f32(rec, faces, size):
    """rr_raster_tile in numpy float32 -> (1 / Z (H,W) float32, face (H,W) int64, -1 = background)"""
    f32 = np.float32
    W, H = size
    u, v, iz = rec["u"], rec["v"], rec["iz"]
    f = np.asarray(faces, dtype=np.int64)
    best_all, face_all = np.zeros((H, W), dtype=f32), np.full((H, W), -1, dtype=np.int64)
    for oy in range(0, H, TILE):
        for ox in range(0, W, TILE):
            fx0, fy0 = f32(ox + 0.5), f32(oy + 0.5)
            ax, ay, cx, cy, dx, dy = u[f[:, 0]] - fx0, v[f[:, 0]] - fy0, u[f[:, 1]] - fx0, v[f[:, 1]] - fy0, u[f[:, 2]] - fx0, v[f[:, 2]] - fy0
            xmin, xmax = np.minimum(ax, np.minimum(cx, dx)), np.maximum(ax, np.maximum(cx, dx))
            ymin, ymax = np.minimum(ay, np.minimum(cy, dy)), np.maximum(ay, np.maximum(cy, dy))
            area = (cx - ax) * (dy - ay) - (dx - ax) * (cy - ay)
            k = np.nonzero((area != 0) & (xmax >= 0) & (xmin <= TILE - 1) & (ymax >= 0) & (ymin <= TILE - 1))[0]
            if not k.shape[0]:
                continue
            ax, ay, cx, cy, dx, dy, area = ax[k], ay[k], cx[k], cy[k], dx[k], dy[k], area[k]
            wa, wc, wd = iz[f[k, 0]], iz[f[k, 1]], iz[f[k, 2]]
            sg, ia = np.where(area > 0, f32(1), f32(-1)), f32(1.0) / area
            e = [(-(dy - cy), dx - cx, (dy - cy) * cx - (dx - cx) * cy), (-(ay - dy), ax - dx, (ay - dy) * dx - (ax - dx) * dy),
                 (-(cy - ay), cx - ax, (cy - ay) * ax - (cx - ax) * ay)]
            g1, g2 = (wc - wa) * ia, (wd - wa) * ia
            pa, pb, pc = e[1][0] * g1 + e[2][0] * g2, e[1][1] * g1 + e[2][1] * g2, wa + (e[1][2] * g1 + e[2][2] * g2)
            qx, qy = np.arange(TILE, dtype=f32)[None, None, :], np.arange(TILE, dtype=f32)[None, :, None]
            best, face = np.zeros((TILE, TILE), dtype=f32), np.full((TILE, TILE), -1, dtype=np.int64)
            for c0 in range(0, k.shape[0], 512):
                s = slice(c0, c0 + 512)
                w = [(sg[s] * a[s])[:, None, None] * qx + ((sg[s] * b[s])[:, None, None] * qy + (sg[s] * c[s])[:, None, None]) for a, b, c in e]
                izp = pa[s, None, None] * qx + (pb[s, None, None] * qy + pc[s, None, None])
                m = np.where((w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0) & (izp > 0), izp, f32(0))
                am = m.argmax(0)                                          # the first maximum: the smallest face index of the chunk
                mx = np.take_along_axis(m, am[None], 0)[0]
                up = mx > best                                            # (later chunks hold larger indices: strict)
                best, face = np.where(up, mx, best), np.where(up, k[s][am], face)
            th, tw = min(TILE, H - oy), min(TILE, W - ox)
            best_all[oy:oy + th, ox:ox + tw], face_all[oy:oy + th, ox:ox + tw] = best[:th, :tw], face[:th, :tw]
    return best_all, face_all


def render_f32(R, t, K, verts, faces, colors, normals, size, shading="phong", ambient=0.5, light=(0, 0, 0), bg=(0, 0, 0), surf_color=None,
               ssaa=1, bgr=False):
    """cp_render_rgb's arithmetic in numpy float32 (separately rounded products where the device fuses: the same error model)
    -> (rgb uint8 (H,W,3), depth float32 (sample grid), face (sample grid))"""
    f32 = np.float32
    W, H = size
    f = int(ssaa)
    Kf = np.asarray(K, dtype=np.float64).reshape(3, 3).copy()
    Kf[0, 0] *= f; Kf[1, 1] *= f; Kf[0, 2] *= f; Kf[1, 2] *= f           # noqa: E702
    c = colors01(colors, len(verts), surf_color).astype(f32) if (colors is None or surf_color is not None) else None
    if c is None:                                                         # MeshSet.from_arrays: float32, / 255 when the maximum is > 1
        c = np.asarray(colors).astype(f32)
        if c.max() > 1.0:
            c = c / f32(255.0)
    uniform = colors is None or surf_color is not None
    rec = vertex_records(f32, R, t, Kf, verts, c, normals, light)
    rec["uniform"] = c[0] if uniform else None
    best, face = winners_f32(rec, faces, (f * W, f * H))
    bgq = np.clip(np.round(f32(255.0) * np.asarray(bg, dtype=np.float64).astype(f32)), 0, 255).astype(np.uint8)
    img = np.tile(bgq.reshape(1, 1, 3), (f * H, f * W, 1))
    ys, xs = np.nonzero(face >= 0)
    if ys.size:
        img[ys, xs] = quantise(shade_points(rec, faces, face[ys, xs], xs, ys, shading, f32(ambient)))
    img = ssaa_average(img, f)
    with np.errstate(divide="ignore"):
        depth = np.where(best > 0, f32(1.0) / best, f32(0)).astype(f32)
    return (img[..., ::-1] if bgr else img), depth, face
