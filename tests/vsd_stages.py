"""Row N8 (BOP's VSD), the stages the device is pinned by.  Nothing here reads the reference; everything is numpy.

  oracle_render          float64 statement of the render rule, with the dilated / eroded depths that say where it is DECIDED
  check_render           the interval check of a depth image against the oracle
  render_f32             an fp32 restatement of the device's rasteriser arithmetic (the yardstick of the bounds: <= 1/4)
  score                  the reference's counting (pose_error.vsd after the render) restated; its mutations for the checker's own test
  count_interval         the counts the undecided pixels of both renders allow
  meshes                 the fixture's triangle meshes, built in closed form

Render rule (renderer_py.py:185-226, 422-555 read as a rule): depth[y, x] is the smallest Z > 0 at which the ray through image point
(x + 0.5, y + 0.5) meets a triangle; Z lies on the triangle's plane, i.e. 1 / Z is interpolated linearly in the image; no culling;
background 0; window coordinate = image coordinate u = fx X / Z + cx, v = fy Y / Z + cy.

Bounds (derived, not tuned; e = 2^-24).  A triangle covers a sample when its three signed edge DISTANCES (pixels, positive inside)
are >= 0.  The device evaluates them from fp32 screen coordinates:
  * u = (P p)_0 / (P p)_2 with P = K [R | t] rounded to fp32 and a 3-fma chain per row: |du| <= 5 e S_u,
    S_u = (A_u + |u| A_z) / Z, A_* the sums of absolute products of the rows (tests/test_bop_error.py's projection scale);
  * u - (tile origin + 0.5) is rounded once: e |u|;  the edge function a q_x + b q_y + c with c = dy x_a - dx y_a costs four more
    roundings of products of an edge component and a coordinate: as a distance, 4 e X with X the largest tile-relative coordinate.
  Both |u| and X are at most S + max(W, H) with S = max_v max(S_u, S_v) -- vertices far outside the frame count.  Moving both ends of
  an edge and the sample moves the distance by sqrt(2) times that.  With the constants rounded up:
      eps   = 32 e (S + max(W, H))                                    [pixels]
  * the plane: 1 / Z_i carries 2 e, the interpolation a few more: 16 e Z; the barycentric weight of vertex i is (distance to the
    opposite edge) / h_i with h_i the altitude, so an error eps of the distances moves the weight by <= 3 eps / h_i and Z by
      tol_T = 16 e Z + 3 eps Zspan_T sum_i 1 / h_i,   Zspan_T = Zmax (Zmax - Zmin) / Zmin of the triangle's vertices.
  tol_d of a pixel is the largest tol_T over the triangles that cover it in the dilated sense."""
import numpy as np

EPS32 = 2.0 ** -24
TILE = 32
TAUS = np.arange(0.05, 0.51, 0.05)


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def _icosphere(level, radius):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v) * radius, np.asarray(f, dtype=np.int32)


def _box(sx, sy, sz, open_top=False):
    v = np.array([[x, y, z] for x in (-sx, sx) for y in (-sy, sy) for z in (-sz, sz)], dtype=np.float64) / 2.0
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]      # -x +x -y +y -z +z
    if open_top:
        q = q[:3] + q[4:5]                                                                         # -x +x -y -z: an open half box
    f = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    return v, np.asarray(f, dtype=np.int32)


def _torus(R, r, n, m):
    a, b = np.meshgrid(np.arange(n) * 2 * np.pi / n, np.arange(m) * 2 * np.pi / m, indexing="ij")
    v = np.stack([(R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)], -1).reshape(-1, 3)
    f = []
    for i in range(n):
        for j in range(m):
            p, q, s, t = i * m + j, ((i + 1) % n) * m + j, ((i + 1) % n) * m + (j + 1) % m, i * m + (j + 1) % m
            f += [(p, q, s), (p, s, t)]
    return v, np.asarray(f, dtype=np.int32)


MESH_NAMES = ("triangle", "box", "halfbox", "ico80", "ico1280", "ico20480", "torus", "hull", "zeroarea")
_MESHES = {}


def meshes(hull_faces=None):
    """name -> (verts float32 (V,3) in mm, faces int32 (F,3)); "hull" needs the recorded faces of the convex hull of
    checkerpose_amd/data/fps_lmo_obj01.npy (tests/golden/vsd.npz: scipy made them once)"""
    if not _MESHES:
        import os
        out = {"triangle": (np.array([[-60.0, -35.0, 5.0], [55.0, -20.0, -10.0], [5.0, 50.0, 20.0]]), np.array([[0, 1, 2]], dtype=np.int32)),
               "box": _box(80.0, 60.0, 40.0), "halfbox": _box(80.0, 60.0, 40.0, open_top=True),
               "ico80": _icosphere(1, 50.0), "ico1280": _icosphere(3, 50.0), "ico20480": _icosphere(5, 50.0),
               "torus": _torus(40.0, 15.0, 24, 12)}
        v, f = _box(70.0, 50.0, 30.0)
        out["zeroarea"] = (v, np.concatenate([f, np.array([[0, 0, 5], [3, 6, 6], [2, 2, 2]], dtype=np.int32)], 0))
        pts = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "checkerpose_amd", "data", "fps_lmo_obj01.npy"))
        out["hull"] = (pts.reshape(-1, 3), None)
        for k, (v, f) in out.items():
            _MESHES[k] = (np.ascontiguousarray(v, dtype=np.float32), f)
    if hull_faces is not None and _MESHES["hull"][1] is None:
        _MESHES["hull"] = (_MESHES["hull"][0], np.ascontiguousarray(hull_faces, dtype=np.int32))
    return _MESHES


def diameter(verts):
    from checkerpose_amd.metric import calc_pts_diameter
    return calc_pts_diameter(verts)


# ---- the render rule -----------------------------------------------------------------------------------------------------------------
def screen(R, t, K, verts):
    """float64 (u, v, Z) of the vertices under K' [R | t], K' = fx, fy, cx, cy of K; and the scale S of the module docstring"""
    R, K = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(K, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    Kc = np.array([[K[0, 0], 0.0, K[0, 2]], [0.0, K[1, 1], K[1, 2]], [0.0, 0.0, 1.0]])
    P = Kc @ np.concatenate([R, t[:, None]], 1)
    ph = np.concatenate([np.asarray(verts, dtype=np.float64), np.ones((len(verts), 1))], 1)
    q = ph @ P.T
    A = np.abs(ph) @ np.abs(P).T
    Z = q[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = q[:, 0] / Z, q[:, 1] / Z
        S = float(np.max(np.maximum(A[:, 0] + np.abs(u) * A[:, 2], A[:, 1] + np.abs(v) * A[:, 2]) / np.abs(Z)))
    return u, v, Z, S


def bounds(S, size):
    """eps [px] of the module docstring"""
    return 32.0 * EPS32 * (S + max(size))


def oracle_render(R, t, K, verts, faces, size, sample=0.5, cull=False):
    """-> dict d (float32, 0 = background), d_lo, d_hi (float64, inf = uncovered), tol (float64), eps, decided (bool), covered_lo.
    size = (W, H).  `sample` and `cull` exist for the checker's own mutation tests."""
    W, H = size
    u, v, Z, S = screen(R, t, K, verts)
    if not (Z > 0).all():
        raise ValueError("a vertex at Z <= 0: outside the render rule")
    eps = bounds(S, size)
    f = np.asarray(faces, dtype=np.int64)
    x = np.stack([u[f[:, 0]], u[f[:, 1]], u[f[:, 2]]], 1)               # (F, 3)
    y = np.stack([v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]], 1)
    z = np.stack([Z[f[:, 0]], Z[f[:, 1]], Z[f[:, 2]]], 1)
    area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    keep = area != 0.0
    if cull:                                                             # OpenGL's front face (counter-clockwise, y up) in image coordinates
        keep &= area < 0.0
    x, y, z, area = x[keep], y[keep], z[keep], area[keep]
    # edge i is opposite vertex i: from vertex i+1 to vertex i+2
    ia, ib = np.array([1, 2, 0]), np.array([2, 0, 1])
    ex, ey = x[:, ib] - x[:, ia], y[:, ib] - y[:, ia]
    length = np.sqrt(ex * ex + ey * ey)                                  # (F, 3)
    with np.errstate(divide="ignore"):
        inv_h = length / np.abs(area)[:, None]                           # 1 / altitude
    zspan = z.max(1) * (z.max(1) - z.min(1)) / z.min(1)
    sens = 3.0 * eps * zspan * inv_h.sum(1)                              # (F,)
    sgn = np.sign(area)
    d = np.full((H, W), np.inf)
    d_lo, d_hi, tol = d.copy(), d.copy(), np.zeros((H, W))
    bx0, bx1 = x.min(1) - sample - eps, x.max(1) - sample + eps          # in pixel-index units
    by0, by1 = y.min(1) - sample - eps, y.max(1) - sample + eps
    for oy in range(0, H, TILE):
        for ox in range(0, W, TILE):
            th, tw = min(TILE, H - oy), min(TILE, W - ox)
            idx = np.nonzero((bx1 >= ox) & (bx0 <= ox + tw - 1) & (by1 >= oy) & (by0 <= oy + th - 1))[0]
            X = (ox + np.arange(tw) + sample)[None, None, :]
            Y = (oy + np.arange(th) + sample)[None, :, None]
            for c0 in range(0, idx.shape[0], 512):
                k = idx[c0:c0 + 512]
                E = [ex[k, i, None, None] * (Y - y[k, ia[i], None, None]) - ey[k, i, None, None] * (X - x[k, ia[i], None, None]) for i in range(3)]
                dist = np.stack([E[i] * (sgn[k, None, None] / length[k, i, None, None]) for i in range(3)], 0).min(0)
                iz = sum(E[i] / (area[k, None, None] * z[k, i, None, None]) for i in range(3))
                with np.errstate(divide="ignore", invalid="ignore"):
                    zp = np.where(iz > 0, 1.0 / iz, np.inf)
                tt = 16.0 * EPS32 * np.where(np.isfinite(zp), zp, 0.0) + sens[k, None, None]
                lo = (dist >= -eps) & np.isfinite(zp)
                sl = (slice(oy, oy + th), slice(ox, ox + tw))
                d[sl] = np.minimum(d[sl], np.where((dist >= 0.0) & np.isfinite(zp), zp, np.inf).min(0))
                d_lo[sl] = np.minimum(d_lo[sl], np.where(lo, zp, np.inf).min(0))
                d_hi[sl] = np.minimum(d_hi[sl], np.where((dist >= eps) & np.isfinite(zp), zp, np.inf).min(0))
                tol[sl] = np.maximum(tol[sl], np.where(lo, tt, 0.0).max(0))
    both_inf = np.isinf(d_lo) & np.isinf(d_hi)
    with np.errstate(invalid="ignore"):
        decided = both_inf | ((d_hi - d_lo) <= tol)
    return {"d": np.where(np.isfinite(d), d, 0.0).astype(np.float32), "d_lo": d_lo, "d_hi": d_hi, "tol": tol, "eps": eps,
            "decided": decided, "covered_lo": np.isfinite(d_lo)}


def undecided_share(o):
    n = int(o["covered_lo"].sum())
    return float((~o["decided"] & o["covered_lo"]).sum()) / n if n else 0.0


def check_render(depth, o):
    """the interval check of one depth image (0 = background) against oracle_render's dict
    -> (ok, worst |diff| / tol on the decided covered pixels, number of pixels outside their interval)"""
    g = np.asarray(depth, dtype=np.float64)
    g = np.where(g > 0, g, np.inf)
    ref = np.where(o["d"] > 0, o["d"].astype(np.float64), np.inf)
    dec = o["decided"]
    fin = dec & np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        bad_dec = dec & ~((g == ref) | (np.abs(g - ref) <= o["tol"]))
        bad_und = ~dec & ~((g >= o["d_lo"] - o["tol"]) & (g <= o["d_hi"] + o["tol"]))
        ratio = np.abs(g - ref)[fin] / o["tol"][fin] if fin.any() else np.zeros(1)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    nbad = int(bad_dec.sum() + bad_und.sum())
    return nbad == 0, float(ratio.max()) if ratio.size else 0.0, nbad


# ---- the device's rasteriser arithmetic, restated in fp32 ------------------------------------------------------------------------------
def render_f32(R, t, K, verts, faces, size, want_dist=False):
    """vsd_vertex_kernel + vsd_tile_kernel's render in numpy float32 (separately rounded products where the device fuses: the same
    error model) -> depth (H,W) float32 [, the smallest |edge distance error| material: (device distance - true distance) is
    measured by the caller through edge_distance_error]"""
    f32 = np.float32
    W, H = size
    R, K = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(K, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    Kc = np.array([[K[0, 0], 0.0, K[0, 2]], [0.0, K[1, 1], K[1, 2]], [0.0, 0.0, 1.0]])
    P = (Kc @ np.concatenate([R, t[:, None]], 1)).astype(f32)
    p = np.asarray(verts, dtype=f32)
    row = lambda r: ((P[r, 0] * p[:, 0] + P[r, 3]) + P[r, 1] * p[:, 1]) + P[r, 2] * p[:, 2]     # noqa: E731
    pu, pv, pw = row(0), row(1), row(2)
    u, v, iz = pu / pw, pv / pw, f32(1.0) / pw
    f = np.asarray(faces, dtype=np.int64)
    depth = np.zeros((H, W), dtype=f32)
    dist_err = 0.0
    u64, v64, _, _ = screen(R, t, K, verts)
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
            qx = np.arange(TILE, dtype=f32)[None, None, :]
            qy = np.arange(TILE, dtype=f32)[None, :, None]
            best = np.zeros((TILE, TILE), dtype=f32)
            for c0 in range(0, k.shape[0], 512):
                s = slice(c0, c0 + 512)
                w = [(sg[s] * a[s])[:, None, None] * qx + ((sg[s] * b[s])[:, None, None] * qy + (sg[s] * c[s])[:, None, None]) for a, b, c in e]
                izp = pa[s, None, None] * qx + (pb[s, None, None] * qy + pc[s, None, None])
                inside = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)
                best = np.maximum(best, np.where(inside, izp, f32(0)).max(0))
                if want_dist:                                            # the device's edge distances against the float64 ones, at
                    kk = k[s]                                            # the samples that project onto the edge's segment, within
                    #                                                      min(2 px, the edge's length) of it: where the edge is a boundary
                    th_, tw_ = min(TILE, H - oy), min(TILE, W - ox)
                    X = (ox + 0.5 + np.arange(tw_))[None, None, :]
                    Y = (oy + 0.5 + np.arange(th_))[None, :, None]
                    ar64 = (u64[f[kk, 1]] - u64[f[kk, 0]]) * (v64[f[kk, 2]] - v64[f[kk, 0]]) - (u64[f[kk, 2]] - u64[f[kk, 0]]) * (v64[f[kk, 1]] - v64[f[kk, 0]])
                    ok = ar64 != 0
                    d64 = []
                    for a_, b_ in ((1, 2), (2, 0), (0, 1)):
                        xa, ya = u64[f[kk, a_]][ok], v64[f[kk, a_]][ok]
                        ex_, ey_ = u64[f[kk, b_]][ok] - xa, v64[f[kk, b_]][ok] - ya
                        ln = np.sqrt(ex_ * ex_ + ey_ * ey_)
                        E64 = ex_[:, None, None] * (Y - ya[:, None, None]) - ey_[:, None, None] * (X - xa[:, None, None])
                        along = (ex_[:, None, None] * (X - xa[:, None, None]) + ey_[:, None, None] * (Y - ya[:, None, None])) / ln[:, None, None]
                        d64.append((E64 * (np.sign(ar64[ok]) / ln)[:, None, None], ln, (along >= 0) & (along <= ln[:, None, None])))
                    if ok.any():
                        for i in range(3):
                            dd = np.abs(w[i][ok][:, :th_, :tw_].astype(np.float64) / d64[i][1][:, None, None] - d64[i][0])
                            near = d64[i][2] & (np.abs(d64[i][0]) <= np.minimum(2.0, d64[i][1])[:, None, None])
                            if near.any():
                                dist_err = max(dist_err, float(dd[near].max()))
            th, tw = min(TILE, H - oy), min(TILE, W - ox)
            with np.errstate(divide="ignore"):
                z = np.where(best > 0, f32(1.0) / best, f32(0)).astype(f32)
            depth[oy:oy + th, ox:ox + tw] = z[:th, :tw]
    return (depth, dist_err) if want_dist else depth


# ---- the reference's counting, restated ------------------------------------------------------------------------------------------------
def dist_image(depth, K):
    """misc.depth_im_to_dist_im_fast: integer pixel x, y; float64"""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    H, W = depth.shape
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    pre_x, pre_y = (xs - K[0, 2]) / np.float64(K[0, 0]), (ys - K[1, 2]) / np.float64(K[1, 1])
    return np.sqrt(np.multiply(pre_x, depth) ** 2 + np.multiply(pre_y, depth) ** 2 + depth.astype(np.float64) ** 2)


def _visible(d_test, d_model, delta, mode):
    diff = d_model.astype(np.float32) - d_test.astype(np.float32)
    near = diff <= np.float32(delta)
    if mode == "bop18":
        return near & (d_test > 0) & (d_model > 0)
    return (near | (d_test == 0)) & (d_model > 0)


def score(depth_test, depth_est, depth_gt, K, delta, taus, normalized_by_diameter, diam, mode="bop19", strict=False):
    """pose_error.vsd after its two renders -> (counts int64 (T + 2,) = union, inter, cost per tau; errors float64 (T,)).
    `mode` / `strict` (a `>` at tau) exist for the checker's own mutation tests."""
    t_test, t_est, t_gt = (dist_image(np.asarray(d, dtype=np.float32), K) for d in (depth_test, depth_est, depth_gt))
    vg = _visible(t_test, t_gt, delta, mode)
    ve = _visible(t_test, t_est, delta, mode) | (vg & (t_est > 0))
    inter, union = vg & ve, vg | ve
    n_union, n_inter = int(union.sum()), int(inter.sum())
    dists = np.abs(t_gt[inter] - t_est[inter])
    if normalized_by_diameter:
        dists = dists / diam
    cost = [int((dists > tau).sum() if strict else (dists >= tau).sum()) for tau in taus]
    counts = np.array([n_union, n_inter] + cost, dtype=np.int64)
    return counts, errors_of(counts)


def errors_of(counts):
    """the float64 quotients of the counts: (cost + union - inter) / union, 1.0 when union == 0"""
    counts = np.asarray(counts, dtype=np.int64)
    if counts[0] == 0:
        return np.ones(counts.shape[0] - 2)
    return np.array([(c + (counts[0] - counts[1])) / float(counts[0]) for c in counts[2:]], dtype=np.float64)


def count_interval(depth_test, o_est, o_gt, K, delta, taus, normalized_by_diameter, diam):
    """(lower, upper) int64 (T + 2,): the counts any pair of depth images inside the oracle's intervals can give.  A pixel is SURE
    when both renders are decided there and every comparison the counting makes (the fp32 difference against delta on either
    side, |dist_gt - dist_est| against every tau) clears its boundary by the renders' tolerances; the counts over the sure pixels
    are fixed, every other pixel may or may not enter each count."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    de, dg = o_est["d"], o_gt["d"]
    t_test, t_est, t_gt = (dist_image(np.asarray(d, dtype=np.float32), K) for d in (depth_test, de, dg))
    H, W = de.shape
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    r = np.sqrt(1.0 + ((xs - K[0, 2]) / K[0, 0]) ** 2 + ((ys - K[1, 2]) / K[1, 1]) ** 2)
    me = r * o_est["tol"] + 4.0 * EPS32 * (t_est + t_test)               # how far dist_est - dist_test can move (+ its fp32 roundings)
    mg = r * o_gt["tol"] + 4.0 * EPS32 * (t_gt + t_test)
    sure = o_est["decided"] & o_gt["decided"]
    sure &= ~((de > 0) & (np.abs((t_est - t_test) - delta) <= me)) & ~((dg > 0) & (np.abs((t_gt - t_test) - delta) <= mg))
    dd = np.abs(t_gt - t_est) / (diam if normalized_by_diameter else 1.0)
    mm = (r * (o_est["tol"] + o_gt["tol"])) / (diam if normalized_by_diameter else 1.0) + 8.0 * EPS32 * dd
    both = (de > 0) & (dg > 0)
    for tau in taus:
        sure &= ~(both & (np.abs(dd - tau) <= mm))
    vg = _visible(t_test, t_gt, delta, "bop19")
    ve = _visible(t_test, t_est, delta, "bop19") | (vg & (t_est > 0))
    inter, union = vg & ve & sure, (vg | ve) & sure
    low = np.array([int(union.sum()), int(inter.sum())] + [int((inter & (dd >= tau)).sum()) for tau in taus], dtype=np.int64)
    return low, low + int((~sure).sum())


def sphere_overlap(radius, p1, p2):
    """misc.overlapping_sphere_projections restated (float64)"""
    p1, p2 = np.asarray(p1, dtype=np.float64).reshape(3), np.asarray(p2, dtype=np.float64).reshape(3)
    if p1[2] == 0 or p2[2] == 0:
        return False
    d = (p1 / p1[2])[:2] - (p2 / p2[2])[:2]
    return bool(np.sqrt(d[0] * d[0] + d[1] * d[1]) < radius * (1.0 / p1[2] + 1.0 / p2[2]))


def ar_vsd(errors, taus=TAUS, ths=TAUS):
    """eval_calc_scores' recall restated for one estimate per target: per (tau, threshold) the share of poses with error < threshold
    (strict; NaN misses), then the mean over all pairs -> (recall (T, Th), AR_VSD)"""
    e = np.asarray(errors, dtype=np.float64)
    rec = np.zeros((len(taus), len(ths)))
    for i in range(len(taus)):
        for j, th in enumerate(ths):
            rec[i, j] = sum(1 for x in e[:, i] if x < th) / float(e.shape[0])
    return rec, float(np.mean(rec))
