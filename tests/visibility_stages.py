"""The clouds and views of tests/golden/visibility.npz and a numpy restatement of the device rule of checkerpose_amd/csrc/visibility.hip
(SURVEY.md 8f row N16), shared by the fixture's maker (tests/golden/make_golden_visibility.py) and the CPU / GPU tests.

Clouds and rotations are regenerated from seeds, not stored; the fixture keeps their CRC-32 so that a drifting generator is noticed.
  cases        name -> dict(kind, V, seed, n_views, radius_param, tview)
  cloud(name)  (V,3) float64, object units of millimetres around the origin
  views(name)  (R (n_views,3,3), t (3,) or (n_views,3)): seeded rotations; t = (0, 0, 400) unless the case has a per-view t
  flip         step 1 of the rule: pc = R p + t, the spherical flip, row 0 the viewpoint -- numpy's own unfused expressions
  hull_rule    steps 2-5: -> (vertex flags (N,), status, {"faces_created", "iterations", "max_visible"})
  hpr_rule     both, for one view -> (visible (V,) uint8, status, stats)
  statistic    the script's lines 113-122: mean = counts / n_views, min, max, the nine ratios np.mean(mean < i * 0.1)"""
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visibility.npz")
T_DEFAULT = (0.0, 0.0, 400.0)
MARGIN_FLOOR = 1e-6            # cloud units: the maker refuses a case with a decision closer to a tie than this
SIZES = (4, 5, 63, 64, 65, 300)


def _cases():
    out = {}
    seed = 100
    for kind in ("sphere", "box", "torus"):
        for V in SIZES:
            seed += 1
            out["%s_v%d" % (kind, V)] = dict(kind=kind, V=V, seed=seed, n_views=16, radius_param=2.0, tview=False)
    out["sphere_v2000"] = dict(kind="sphere", V=2000, seed=201, n_views=4, radius_param=2.0, tview=False)
    out["tetra_centroid_v5"] = dict(kind="tetra_centroid", V=5, seed=0, n_views=16, radius_param=2.0, tview=False)
    out["cube_centre_v9"] = dict(kind="cube_centre", V=9, seed=0, n_views=16, radius_param=2.0, tview=False)
    out["tetra_v4"] = dict(kind="tetra", V=4, seed=0, n_views=16, radius_param=2.0, tview=False)
    out["sphere_v300_r15"] = dict(kind="sphere", V=300, seed=301, n_views=16, radius_param=1.5, tview=False)
    out["torus_v300_tview"] = dict(kind="torus", V=300, seed=302, n_views=16, radius_param=2.0, tview=True)
    return out


CASES = _cases()


def names():
    return list(CASES)


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a, dtype=np.float64).tobytes(), c)
    return c & 0xFFFFFFFF


def dented_sphere(V, seed):
    """a sphere of radius 50 with a deep dent towards (0.6, 0, 0.8) and 5 % radial noise"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(V, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    dent = 1.0 - 0.45 * np.exp(-((d - np.array([0.6, 0.0, 0.8])) ** 2).sum(axis=1) / 0.15)
    r = 50.0 * dent * (1.0 + 0.05 * rng.normal(size=V))
    return d * r[:, None]


def box_surface(V, seed):
    """points on the six faces of an 80 x 60 x 40 box"""
    rng = np.random.default_rng(seed)
    half = np.array([40.0, 30.0, 20.0])
    pts = rng.uniform(-1.0, 1.0, size=(V, 3)) * half
    face = rng.integers(0, 6, size=V)
    axis, sign = face // 2, np.where(face % 2 == 0, -1.0, 1.0)
    pts[np.arange(V), axis] = sign * half[axis]
    return pts


def torus(V, seed):
    """points on a torus of radii 45 and 15: every view hides part of the inner ring"""
    rng = np.random.default_rng(seed)
    u, w = rng.uniform(0.0, 2.0 * np.pi, size=V), rng.uniform(0.0, 2.0 * np.pi, size=V)
    ring = 45.0 + 15.0 * np.cos(w)
    return np.stack([ring * np.cos(u), ring * np.sin(u), 15.0 * np.sin(w)], axis=1)


_TETRA = 40.0 * np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])


def cloud(name):
    c = CASES[name]
    kind = c["kind"]
    if kind == "sphere":
        return dented_sphere(c["V"], c["seed"])
    if kind == "box":
        return box_surface(c["V"], c["seed"])
    if kind == "torus":
        return torus(c["V"], c["seed"])
    if kind == "tetra":
        return _TETRA.copy()
    if kind == "tetra_centroid":
        return np.concatenate([_TETRA, _TETRA.mean(axis=0, keepdims=True)], axis=0)
    if kind == "cube_centre":
        corners = 30.0 * np.array([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)])
        return np.concatenate([corners, np.zeros((1, 3))], axis=0)
    raise KeyError(kind)


def rotations(n, seed):
    rng = np.random.default_rng(seed)
    out = np.empty((n, 3, 3))
    for k in range(n):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 2] = -q[:, 2]
        out[k] = q
    return out


def views(name):
    c = CASES[name]
    R = rotations(c["n_views"], 7000 + c["seed"])
    if not c["tview"]:
        return R, np.array(T_DEFAULT)
    rng = np.random.default_rng(9000 + c["seed"])
    t = np.array(T_DEFAULT) + rng.uniform(-60.0, 60.0, size=(c["n_views"], 3))
    return R, t


def view_t(t, k):
    return t if t.ndim == 1 else t[k]


# ---- the rule ------------------------------------------------------------------------------------------------------------------

def flip(vertices, R, t, radius_param=2.0):
    """step 1 -> (N,3) with N = V + 1: row 0 the viewpoint, rows 1.. the flipped points"""
    v = np.asarray(vertices, dtype=np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    pc = np.stack([((R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z) + t[k] for k in range(3)], axis=1)
    nr = np.sqrt((pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]) + pc[:, 2] * pc[:, 2])
    radius = nr.max() * (10 ** radius_param)
    P = np.zeros((v.shape[0] + 1, 3))
    P[1:] = pc + (2 * (radius - nr))[:, None] * (pc / nr[:, None])
    return P


def _plane(P, a, b, c):
    A, e, f = P[a], P[b] - P[a], P[c] - P[a]
    n0, n1, n2 = e[1] * f[2] - e[2] * f[1], e[2] * f[0] - e[0] * f[2], e[0] * f[1] - e[1] * f[0]
    return np.array([n0, n1, n2, -((n0 * A[0] + n1 * A[1]) + n2 * A[2])])


def _val(pl, P):
    """plane value(s): pl (4,) or (F,4) against P (3,) or (n,3), by the device's order of operations"""
    pl, P = np.asarray(pl), np.asarray(P)
    if pl.ndim == 2 and P.ndim == 2:
        pl, P = pl[None, :, :], P[:, None, :]
    return ((pl[..., 0] * P[..., 0] + pl[..., 1] * P[..., 1]) + pl[..., 2] * P[..., 2]) + pl[..., 3]


def hull_rule(P):
    """steps 2-5 on the (N,3) flipped points -> (vertex (N,) bool, status, stats)"""
    N = P.shape[0]
    Fcap = 2 * (N - 1) - 2
    stats = {"faces_created": 0, "iterations": 0, "max_visible": 0}
    vertex = np.zeros(N, dtype=bool)
    i0, i1 = int(np.argmin(P[:, 0])), int(np.argmax(P[:, 0]))
    if not P[i1, 0] > P[i0, 0]:
        return vertex, 1, stats
    e = P[i1] - P[i0]
    d = P - P[i0]
    c = np.stack([d[:, 1] * e[2] - d[:, 2] * e[1], d[:, 2] * e[0] - d[:, 0] * e[2], d[:, 0] * e[1] - d[:, 1] * e[0]], axis=1)
    m = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
    i2 = int(np.argmax(m))
    if not m[i2] > 0:
        return vertex, 1, stats
    f = P[i2] - P[i0]
    n = np.array([e[1] * f[2] - e[2] * f[1], e[2] * f[0] - e[0] * f[2], e[0] * f[1] - e[1] * f[0]])
    m = np.abs((n[0] * d[:, 0] + n[1] * d[:, 1]) + n[2] * d[:, 2])
    i3 = int(np.argmax(m))
    if not m[i3] > 0:
        return vertex, 1, stats
    tv = [i0, i1, i2, i3]
    fv = np.zeros((Fcap, 3), dtype=np.int64)
    fpl = np.zeros((Fcap, 4))
    state = np.zeros(Fcap, dtype=np.int64)                # 0 dead, 1 live
    for k, (a, b, c_, opp) in enumerate(((0, 1, 2, 3), (0, 1, 3, 2), (0, 2, 3, 1), (1, 2, 3, 0))):
        a, b, c_, opp = tv[a], tv[b], tv[c_], tv[opp]
        pl = _plane(P, a, b, c_)
        if _val(pl, P[opp]) > 0:
            b, c_ = c_, b
            pl = _plane(P, a, b, c_)
        if not _val(pl, P[opp]) < 0:
            return vertex, 1, stats
        fv[k], fpl[k], state[k] = (a, b, c_), pl, 1
    vertex[tv] = True
    stats["faces_created"] = 4
    assign = np.full(N, -1, dtype=np.int64)
    above = _val(fpl[:4], P) > 0                          # (N,4)
    has = above.any(axis=1) & ~vertex
    assign[has] = np.argmax(above[has], axis=1)           # the first face it lies above
    nslots, it = 4, 0
    while True:
        pend = np.nonzero(assign >= 0)[0]
        if pend.size == 0:
            return vertex, 0, stats
        if it == N:
            return vertex, 4, stats
        F = assign[pend[0]]
        vals = _val(fpl[F], P)
        p = int(np.argmax(vals))
        if not vals[p] > 0:
            return vertex, 2, stats
        live = np.nonzero(state[:nslots] == 1)[0]
        visf = live[_val(fpl[live], P[p]) > 0]
        v = visf.size
        stats["max_visible"] = max(stats["max_visible"], int(v))
        edges = [(int(fv[g, j]), int(fv[g, (j + 1) % 3])) for g in visf for j in range(3)]
        have = set(edges)
        hz = sorted(ab for ab in edges if (ab[1], ab[0]) not in have)          # by start point: the tie order of the reassignment
        h = len(hz)
        if h < 3 or len(set(a for a, _ in hz)) != h:
            return vertex, 2, stats
        extra = max(0, h - v)
        if nslots + extra > Fcap:
            return vertex, 3, stats
        newpl = np.stack([_plane(P, a, b, p) for a, b in hz])
        slots = np.array([visf[k] if k < v else nslots + (k - v) for k in range(h)], dtype=np.int64)
        move = np.nonzero((assign >= 0) & np.isin(assign, visf))[0]
        if move.size:
            val = _val(newpl, P[move])                                         # (points, h)
            val = np.where(val > 0, val, -np.inf)
            best = np.argmax(val, axis=1)                                      # the largest value; the first = the smallest start point
            assign[move] = np.where(np.isfinite(val[np.arange(move.size), best]), slots[best], -1)
        assign[p] = -1
        vertex[p] = True
        state[visf] = 0
        for k in range(h):
            fv[slots[k]], fpl[slots[k]], state[slots[k]] = (hz[k][0], hz[k][1], p), newpl[k], 1
        nslots += extra
        it += 1
        stats["iterations"] = it
        stats["faces_created"] += h


def hpr_rule(vertices, R, t, radius_param=2.0):
    vertex, status, stats = hull_rule(flip(vertices, R, t, radius_param))
    return vertex[1:].astype(np.uint8), status, stats


def statistic(counts, n_views):
    """get_overall_visibility.py:113-122 -> (mean (V,), min, max, below (9,))"""
    mean = np.asarray(counts, dtype=np.float64) / n_views
    below = np.array([np.mean(mean < i * 0.1) for i in range(1, 10)])
    return mean, mean.min(), mean.max(), below
