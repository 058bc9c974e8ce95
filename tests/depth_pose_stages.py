"""Row N25's rule in numpy (csrc/pose_depth.hip states it), the committed cases, and check_case: the replay of the device's records.

The rule is this project's own: the restatement below IS its definition for the tests.  It follows the kernel's arithmetic operation
for operation (fp64, no contraction): the lift, the sampler, the degeneracy test, the minimal solver, nearest_rotation, the inlier
test.  The sums of a fit take a `sums` function: device_sum is lm_stages.kernel_sum, the kernel's order (thread t adds keypoints t, t + 256, ...,
then block_sum's tree), permuted_sum another order -- the difference between the two is the summation-order difference that check_case
measures per case and compares poses against (margin = 16 x).

check_case replays a device run from its records: every decision (a degenerate sample, an inlier, a round that runs, the winner, a
step that is accepted) is recomputed from the DEVICE's own recorded poses, so that counts, winner, step flags, status and inliers must
be exact, while the poses themselves are compared with the numpy rule's within the margin.  A decision within 1e-9 (relative) of its
boundary is reported in the result's `near` list: the committed cases have none under the numpy rule alone (tests/test_depth_pose.py).

`python -m tests.depth_pose_stages` prints the per-case summation-order differences of the numpy rule."""
import math
import os

import numpy as np

from tests.lm_stages import kernel_sum

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "checkerpose_amd", "data")
SIZE = (96, 80)                                     # (W, H)
RECORD, STEPS, ROUND, MAX_ITERS, NMAX, THREADS = 14, 4, 64, 256, 4096, 256
NEAR = 1e-9
MARGIN_FACTOR = 16.0
K_A = np.array([[120.0, 0.0, 47.3], [0.0, 118.0, 40.6], [0.0, 0.0, 1.0]], np.float32)
K_B = np.array([[124.0, 0.0, 45.7], [0.0, 121.0, 38.2], [0.0, 0.0, 1.0]], np.float32)


class StageError(AssertionError):
    def __init__(self, stage, crop, what):
        super().__init__("stage %s, crop %d: %s" % (stage, crop, what))
        self.stage, self.crop = stage, crop


# --------------------------------------------------------------------------------------------------------------------- the sampler
def hash32(a, b, c, d):
    M = 0xFFFFFFFF
    h = (a * 0x9E3779B1 + 0x7F4A7C15) & M
    for v in (b, c, d):
        h ^= (v + 0x9E3779B9 + ((h << 6) & M) + (h >> 2)) & M
        h = (h * 0x85EBCA6B) & M
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & M
        h ^= h >> 16
    return h


def sample3(seed, crop, hyp, n):
    """3 distinct positions in [0, n): draw k = hash32(seed, crop, hyp, try) % n, duplicates redrawn"""
    out, t = [], 0
    while len(out) < 3:
        r = hash32(seed & 0xFFFFFFFF, crop, hyp, t) % n
        t += 1
        if r not in out:
            out.append(r)
    return out


def needed_iters(best, n, m, iters):
    """OpenCV's RANSACUpdateNumIters at confidence 0.99 (pnp_core.h) -> (iterations, the real number before rounding or None)"""
    if best < m:
        return iters, None
    ep = min(max(1.0 - float(best) / float(n), 0.0), 1.0)
    num = math.log(1.0 - 0.99)
    denom = 1.0 - math.pow(1.0 - ep, float(m))
    if denom < 2.2250738585072014e-308:
        return 0, None
    denom = math.log(denom)
    if denom >= 0.0 or -num >= float(iters) * (-denom):
        return iters, None
    return int(np.rint(num / denom)), num / denom


# -------------------------------------------------------------------------------------------------------------------- stage A
def lift(p2d, valid, K, depth, image=0):
    """one crop: p2d (N,2) f32, valid (N,) bool, K (3,3) f32, depth (I,H,W) f32 -> (Q (N,3) f32, lifted (N,) bool)"""
    p2d, K = np.asarray(p2d, np.float32), np.asarray(K, np.float32)
    N = p2d.shape[0]
    Q, lifted = np.zeros((N, 3), np.float32), np.zeros(N, bool)
    I, H, W = depth.shape
    if not 0 <= image < I:
        return Q, lifted
    u, v = p2d[:, 0].astype(np.float64), p2d[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = np.asarray(valid, bool) & (u >= 0.0) & (v >= 0.0) & (u < float(W)) & (v < float(H))
    x, y = np.floor(np.where(inside, u, 0.0)).astype(np.int64), np.floor(np.where(inside, v, 0.0)).astype(np.int64)
    z = depth[image][y, x]
    with np.errstate(invalid="ignore"):
        ok = inside & np.isfinite(z) & (z > 0)
    fx, fy, cx, cy = (np.float64(K[0, 0]), np.float64(K[1, 1]), np.float64(K[0, 2]), np.float64(K[1, 2]))
    zd = z.astype(np.float64)
    with np.errstate(all="ignore"):
        q0 = ((u - cx) / fx) * zd
        q1 = ((v - cy) / fy) * zd
    Q[ok, 0], Q[ok, 1], Q[ok, 2] = q0[ok].astype(np.float32), q1[ok].astype(np.float32), z[ok]
    lifted[:] = ok
    return Q, lifted


# ------------------------------------------------------------------------------------------------------- the rotation, the fits
def nearest_rotation(m):
    """pnp_core.h's nearest_rotation operation for operation: -> (R (9,) list or None, rank 3 / 2 / 0)"""
    a = [float(x) for x in np.asarray(m, np.float64).reshape(9)]
    v = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    sqrt, fabs = math.sqrt, math.fabs
    if not all(math.isfinite(x) for x in a):
        return None, 0
    PQ = ((0, 1), (0, 2), (1, 2))
    for _ in range(40):
        rotated = False
        for p, q in PQ:
            al = be = ga = 0.0
            for i in range(3):
                al += a[3 * i + p] * a[3 * i + p]
                be += a[3 * i + q] * a[3 * i + q]
                ga += a[3 * i + p] * a[3 * i + q]
            if fabs(ga) <= 1e-16 * sqrt(al * be) or ga == 0.0:
                continue
            rotated = True
            zeta = (be - al) / (2.0 * ga)
            t = (1.0 if zeta >= 0.0 else -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta))
            c = 1.0 / sqrt(1.0 + t * t)
            s = c * t
            for i in range(3):
                aip, aiq = a[3 * i + p], a[3 * i + q]
                a[3 * i + p] = c * aip - s * aiq
                a[3 * i + q] = s * aip + c * aiq
                vip, viq = v[3 * i + p], v[3 * i + q]
                v[3 * i + p] = c * vip - s * viq
                v[3 * i + q] = s * vip + c * viq
        if not rotated:
            break
    sg = [sqrt(a[j] * a[j] + a[3 + j] * a[3 + j] + a[6 + j] * a[6 + j]) for j in range(3)]
    for p, q in PQ:
        if sg[q] > sg[p]:
            sg[p], sg[q] = sg[q], sg[p]
            for i in range(3):
                a[3 * i + p], a[3 * i + q] = a[3 * i + q], a[3 * i + p]
                v[3 * i + p], v[3 * i + q] = v[3 * i + q], v[3 * i + p]
    if not sg[1] > 1e-12 * sg[0]:
        return None, 0
    i0, i1 = 1.0 / sg[0], 1.0 / sg[1]
    u0 = (a[0] * i0, a[3] * i0, a[6] * i0)
    u1 = (a[1] * i1, a[4] * i1, a[7] * i1)
    dv = v[0] * (v[4] * v[8] - v[5] * v[7]) - v[1] * (v[3] * v[8] - v[5] * v[6]) + v[2] * (v[3] * v[7] - v[4] * v[6])
    sgn = 1.0 if dv >= 0.0 else -1.0
    u2 = (sgn * (u0[1] * u1[2] - u0[2] * u1[1]), sgn * (u0[2] * u1[0] - u0[0] * u1[2]), sgn * (u0[0] * u1[1] - u0[1] * u1[0]))
    R = [u0[i] * v[3 * j] + u1[i] * v[3 * j + 1] + u2[i] * v[3 * j + 2] for i in range(3) for j in range(3)]
    return R, (2 if sg[2] <= 1e-12 * sg[0] else 3)


def _pose_from(H9, x, q):
    R, rank = nearest_rotation(H9)
    if R is None:
        return None
    t = [q[a] - ((R[3 * a] * x[0] + R[3 * a + 1] * x[1]) + R[3 * a + 2] * x[2]) for a in range(3)]
    return np.array(R + t, np.float64)


def degeneracy(X3):
    """the collinearity test of a sample's model points (3,3) f64 -> (|e1 x e2|^2, 1e-12 (max squared edge)^2)"""
    e1, e2, e3 = X3[1] - X3[0], X3[2] - X3[0], X3[2] - X3[1]
    c0, c1, c2 = e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]
    l1, l2, l3 = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] for e in (e1, e2, e3))
    lm = max(max(l1, l2), l3)
    return (c0 * c0 + c1 * c1) + c2 * c2, 1e-12 * (lm * lm)


def minimal_pose(X3, Q3, order=(0, 1, 2)):
    """the pose of three pairs (fp64 arrays (3,3)), or None when degenerate; `order`: the order of the three-term sums (the rule's is
    0, 1, 2; another one measures the summation-order difference)"""
    lhs, rhs = degeneracy(X3)
    if lhs <= rhs:
        return None
    i, j, k = order
    x = [((X3[i][c] + X3[j][c]) + X3[k][c]) / 3.0 for c in range(3)]
    q = [((Q3[i][c] + Q3[j][c]) + Q3[k][c]) / 3.0 for c in range(3)]
    H = [((Q3[i][a] - q[a]) * (X3[i][c] - x[c]) + (Q3[j][a] - q[a]) * (X3[j][c] - x[c])) + (Q3[k][a] - q[a]) * (X3[k][c] - x[c])
         for a in range(3) for c in range(3)]
    return _pose_from(H, x, q)


device_sum = kernel_sum      # vals (n, k): row j belongs to thread j % 256; block_sum's order (pnp_core.h)


def permuted_sum(vals):
    """another order: numpy's pairwise sum over the rows reversed"""
    return np.sum(vals[::-1], axis=0)


def fit(X, Q, mask, sums=device_sum):
    """the least-squares pose over the flagged keypoints (X, Q (n,3) f64; rows outside `mask` add 0.0, as the kernel skips them)"""
    cnt = float(mask.sum())
    m = mask[:, None]
    acc = sums(np.where(m, np.concatenate([X, Q], 1), 0.0))
    x, q = acc[:3] / cnt, acc[3:] / cnt
    terms = ((Q - q)[:, :, None] * (X - x)[:, None, :]).reshape(-1, 9)
    H = sums(np.where(m, terms, 0.0))
    return _pose_from(H, [float(c) for c in x], [float(c) for c in q])


def residual2(P, X, Q):
    """|R X + t - Q|^2 in the kernel's order; X, Q (n,3) f64"""
    d = [(((P[3 * a] * X[:, 0] + P[3 * a + 1] * X[:, 1]) + P[3 * a + 2] * X[:, 2]) + P[9 + a]) - Q[:, a] for a in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)


# ------------------------------------------------------------------------------------------------------- the free-running rule
def solve_crop(X, Q, thr, iterations, seed, crop, sums=device_sum, tamper=()):
    """stages B and C over the n lifted keypoints (X, Q (n,3) f64, ascending) -> dict(pose (12,), inliers (n,) bool, status,
    hypotheses (iterations,14), steps (4,14), winner).  NaN where the rule writes nothing.
    tamper (tests only): "strict" = an inlier needs r^2 < thr^2; "no_stop" = the stopping rule never cuts a round; "no_lo" = stage C
    stops after the first fit.  (Which of several hypotheses with the winning count wins shows in the outputs only where their inlier
    sets differ; in the committed cases they never do.)"""
    n = X.shape[0]
    hyp = np.full((iterations, RECORD), np.nan)
    steps = np.full((STEPS, RECORD), np.nan)
    out = dict(pose=IDENTITY.copy(), inliers=np.zeros(n, bool), status=0, hypotheses=hyp, steps=steps, winner=-1)
    if n < 3 or not (thr > 0.0 and math.isfinite(thr)):
        return out
    thr2 = thr * thr
    inl = (lambda P: residual2(P, X, Q) < thr2) if "strict" in tamper else (lambda P: residual2(P, X, Q) <= thr2)
    bc, bh, bp = 2, -1, None
    r = 0
    while ROUND * r < iterations:
        for h in range(ROUND * r, min(ROUND * (r + 1), iterations)):
            s = sample3(seed, crop, h, n)
            P = minimal_pose(X[s], Q[s])
            if P is None:
                hyp[h, 0] = -1.0
                continue
            c = int(inl(P).sum())
            hyp[h, 0], hyp[h, 2:] = c, P
            if c > bc:
                bc, bh, bp = c, h, P
        r += 1
        if "no_stop" not in tamper and not ROUND * r < needed_iters(bc if bh >= 0 else -1, n, 3, iterations)[0]:
            break
    if bh < 0:
        return out
    out["winner"] = bh
    P, L = bp, inl(bp)
    Pn = fit(X, Q, L, sums)
    ok = Pn is not None
    if ok:
        P = Pn
    steps[0, 0], steps[0, 1], steps[0, 2:] = L.sum(), float(ok), P
    for k in range(1, STEPS):
        if not ok or "no_lo" in tamper:
            break
        Ln = inl(P)
        ok = Ln.sum() > L.sum()
        Pn = fit(X, Q, Ln, sums) if ok else None
        ok = ok and Pn is not None
        if ok:
            P, L = Pn, Ln
        steps[k, 0], steps[k, 1], steps[k, 2:] = Ln.sum(), float(ok), P
    out.update(pose=P, inliers=L, status=1)
    return out


# ------------------------------------------------------------------------------------------------------------------ the cases
class Case:
    """p3d (N,3) or (B,N,3) f32; p2d (B,N,2) f32; valid (B,N,3) uint8; K (3,3) or (B,3,3) f32; depth (I,H,W) f32; image_ids None or (B,)
    int; thr a number or (B,) f64; truth: per crop (R, t) or None; converging: the crops whose pose must come out near the truth"""

    def __init__(self, name, p3d, p2d, valid, K, depth, image_ids=None, thr=6.0, column=0, iterations=150, seed=1, truth=None, converging=()):
        self.name, self.p3d, self.p2d, self.valid = name, np.asarray(p3d, np.float32), np.asarray(p2d, np.float32), np.asarray(valid, np.uint8)
        self.K, self.depth, self.image_ids, self.thr = np.asarray(K, np.float32), np.asarray(depth, np.float32), image_ids, thr
        self.column, self.iterations, self.seed = column, iterations, seed
        self.B, self.N = self.p2d.shape[:2]
        self.truth = truth if truth is not None else [None] * self.B
        self.converging = tuple(converging)

    def image_of(self, b):
        if self.image_ids is not None:
            return int(self.image_ids[b])
        return 0 if self.depth.shape[0] == 1 else b

    def thr_of(self, b):
        return float(self.thr[b]) if np.ndim(self.thr) else float(self.thr)

    def crop(self, b):
        """-> (X (N,3) f64 model points, p2d (N,2) f32, valid (N,) bool, K (3,3) f32)"""
        return ((self.p3d[b] if self.p3d.ndim == 3 else self.p3d).astype(np.float64), self.p2d[b], self.valid[b, :, self.column] != 0,
                self.K[b] if self.K.ndim == 3 else self.K)

    def lifted(self, b):
        """-> (Q (N,3) f32, lifted (N,) bool) of crop b under the numpy rule"""
        _, p2d, valid, K = self.crop(b)
        return lift(p2d, valid, K, self.depth, self.image_of(b))


def model(obj, n):
    return np.load(os.path.join(DATA, "fps_lm_15x4096.npy"))[obj, :n].astype(np.float32)


def _rotation(rng):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = rng.uniform(0.2, np.pi - 0.2)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def quantise(uv):
    """true projections (N,2) f64 -> the p2d that `correspondences` gives: the corner of the 64-cell RoI grid cell, over the points'
    integer bounding box (x, y, w, h), evaluated in fp64 and cast to fp32 (csrc/graph_ops.hip)"""
    x0, y0 = math.floor(uv[:, 0].min()) - 1, math.floor(uv[:, 1].min()) - 1
    w, h = math.ceil(uv[:, 0].max()) + 1 - x0, math.ceil(uv[:, 1].max()) + 1 - y0
    xi = np.clip(np.floor((uv[:, 0] - x0) / (w / 64.0)), 0, 63)
    yi = np.clip(np.floor((uv[:, 1] - y0) / (h / 64.0)), 0, 63)
    return np.stack([(float(w) / 64.0 * xi + float(x0)).astype(np.float32), (float(h) / 64.0 * yi + float(y0)).astype(np.float32)], 1)


def _splat(depth, p2d, z, keep):
    """the sensor's depth under the keypoints: a z-buffer of the keypoints' own depths at the pixels their p2d fall in (the nearest
    wins: keypoints on the far side of the object that share a pixel with a nearer one become the natural outliers)"""
    H, W = depth.shape
    for (u, v), zz, k in zip(p2d, z, keep):
        if k and 0 <= u < W and 0 <= v < H:
            x, y = int(math.floor(u)), int(math.floor(v))
            if not depth[y, x] > 0 or zz < depth[y, x]:
                depth[y, x] = zz


def _scene(name, seed, B, N, objs=(0,), n_img=None, image_ids=None, per_crop_K=False, per_crop_model=False, slab=0.0, holes=0.0, junk=False,
           valid_frac=(1.0, 0.7, 0.4), shift=(), planar=None, keep=None, converging=True, **kw):
    """B crops of N keypoints on n_img frames.  slab: the fraction of the object's footprint that an occluder in front of it covers;
    holes: the fraction of depth pixels set to 0; junk: NaN, inf and negative depths as well; shift: crops pushed partly out of the
    frame; planar: "coplanar" / "collinear" model points; keep: only this many keypoints of a crop keep their valid byte."""
    rng = np.random.default_rng(seed)
    W, H = SIZE
    n_img = B if n_img is None else n_img                       # without ids: one image per crop in order, or one image for all
    ids = image_ids
    assert ids is not None or n_img in (1, B)
    depth = np.zeros((n_img, H, W), np.float32)
    models = [model(objs[b % len(objs)], N) for b in range(B)]
    if planar:
        for m in models:
            m[:, 2] = 0.0
            if planar == "collinear":
                m[:, 1] = 0.0
    Ks = np.stack([K_A if b % 2 == 0 else K_B for b in range(B)]) if per_crop_K else K_A
    p2d, valid, truth = np.zeros((B, N, 2), np.float32), np.zeros((B, N, 3), np.uint8), []
    for b in range(B):
        K = (Ks[b] if per_crop_K else Ks).astype(np.float64)
        X = models[b].astype(np.float64)
        rad = np.linalg.norm(X, axis=1).max()
        R = _rotation(rng)
        tz = rad * 120.0 / rng.uniform(26.0, 32.0)              # the footprint's radius: 26 .. 32 pixels
        t = np.array([rng.uniform(-0.03, 0.03) * tz, rng.uniform(-0.02, 0.02) * tz, tz])
        if b in shift:
            t[0] += 0.3 * tz
        C = X @ R.T + t
        uv = np.stack([K[0, 0] * C[:, 0] / C[:, 2] + K[0, 2], K[1, 1] * C[:, 1] / C[:, 2] + K[1, 2]], 1)
        p2d[b] = quantise(uv)
        for c, f in enumerate(valid_frac):
            valid[b, :, c] = rng.random(N) < f
        if keep is not None:
            only = np.zeros(N, bool)
            only[rng.choice(N, keep[b % len(keep)], replace=False)] = True
            valid[b] &= only[:, None]
        img = int(ids[b]) if ids is not None else (0 if n_img == 1 else b)
        _splat(depth[img], p2d[b], C[:, 2].astype(np.float32), np.ones(N, bool))
        truth.append((R, t))
        if slab:                                                # an occluder slab in front of the left part of the footprint
            x1 = int(np.quantile(uv[:, 0], slab))
            region = depth[img, :, :max(x1, 0)]
            region[region > 0] = np.float32(0.45 * tz)
    if holes:
        depth[rng.random(depth.shape) < holes] = 0.0
    if junk:
        m = rng.random(depth.shape)
        depth[m < 0.03] = np.nan
        depth[(m >= 0.03) & (m < 0.05)] = np.inf
        depth[(m >= 0.05) & (m < 0.07)] = -depth[(m >= 0.05) & (m < 0.07)] - 1.0
    p3d = np.stack(models) if per_crop_model or len(objs) > 1 else models[0]
    return Case(name, p3d, p2d, valid, Ks, depth, image_ids=ids, truth=truth, seed=seed, converging=range(B) if converging else (), **kw)


CASES = {
    "n3": lambda: _scene("n3", 11, 1, 3, valid_frac=(1.0, 1.0, 1.0), iterations=64, converging=False),
    "n5": lambda: _scene("n5", 12, 1, 5, valid_frac=(1.0, 1.0, 1.0), iterations=1, converging=False),
    "n64_b3": lambda: _scene("n64_b3", 13, 3, 64, n_img=2, image_ids=np.array([1, 0, 1]), iterations=65, thr=8.0),
    "n512_b5_slab": lambda: _scene("n512_b5_slab", 14, 5, 512, objs=(0, 14), n_img=3, image_ids=np.array([0, 2, 1, 2, 0]), per_crop_K=True,
                                   slab=0.2, holes=0.05, junk=True, thr=np.array([6.0, 8.0, 5.0, 7.0, 6.5]), iterations=256),
    "n512_slab_half": lambda: _scene("n512_slab_half", 15, 1, 512, slab=0.3, holes=0.1, iterations=150),
    "n4096_b2": lambda: _scene("n4096_b2", 16, 2, 4096, objs=(14,), per_crop_model=True, iterations=150, thr=5.0),
    "n512_off_frame": lambda: _scene("n512_off_frame", 17, 2, 512, objs=(14,), shift=(1,), iterations=64),
    "three_lifted": lambda: _scene("three_lifted", 18, 2, 64, keep=(3, 3), iterations=150, converging=False),
    "two_lifted": lambda: _scene("two_lifted", 19, 2, 64, n_img=1, keep=(2, 0), iterations=150, converging=False),
    "collinear": lambda: _scene("collinear", 20, 1, 64, planar="collinear", iterations=65, converging=False),
    "coplanar": lambda: _scene("coplanar", 21, 2, 512, planar="coplanar", iterations=150),
    "grow": lambda: _scene("grow", 43, 2, 512, iterations=1, thr=4.0),       # one mediocre hypothesis: stage C's inlier set grows up to 3 times
    "column_1": lambda: _scene("column_1", 22, 3, 512, column=1, slab=0.3),
    "column_2": lambda: _scene("column_2", 23, 3, 512, column=2, slab=0.3, junk=True),
}
_CASES = {}


def make(name):
    if name not in _CASES:
        _CASES[name] = CASES[name]()
    return _CASES[name]


def converging(names=None):
    """(case name, crop) of every crop that must come out near its truth"""
    return [(n, b) for n in (names or CASES) for b in make(n).converging]


# --------------------------------------------------------------------------------------------------- the restatement of a whole case
def restatement_outputs(case, sums=device_sum, tamper=()):
    """the free-running numpy rule over a case, in the layout of the device's outputs (numpy arrays)"""
    B, N, it = case.B, case.N, case.iterations
    out = dict(R=np.zeros((B, 3, 3)), t=np.zeros((B, 3)), inliers=np.zeros((B, N), bool), status=np.zeros(B, np.int32),
               hypotheses=np.full((B, it, RECORD), np.nan), steps=np.full((B, STEPS, RECORD), np.nan), Q=np.zeros((B, N, 3), np.float32),
               lifted=np.zeros((B, N), np.uint8), n_lifted=np.zeros(B, np.int32), winner=np.zeros(B, np.int64))
    for b in range(B):
        X = case.crop(b)[0]
        Q, lf = case.lifted(b)
        idx = np.nonzero(lf)[0]
        s = solve_crop(X[idx], Q[idx].astype(np.float64), case.thr_of(b), it, case.seed, b, sums, tamper)
        out["R"][b], out["t"][b] = s["pose"][:9].reshape(3, 3), s["pose"][9:]
        out["inliers"][b, idx] = s["inliers"]
        out["status"][b], out["hypotheses"][b], out["steps"][b], out["winner"][b] = s["status"], s["hypotheses"], s["steps"], s["winner"]
        out["Q"][b], out["lifted"][b], out["n_lifted"][b] = Q, lf, lf.sum()
    return out


def add_error(X, R, t, Rt, tt):
    """the mean distance of the model points under two poses (ADD)"""
    return float(np.linalg.norm((X @ np.asarray(R).T + np.reshape(t, 3)) - (X @ Rt.T + tt), axis=1).mean())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32)


def _pose_diff(P, Pn):
    """(max |dR|, |dt| / max(|t|, 1))"""
    return float(np.abs(P[:9] - Pn[:9]).max()), float(np.linalg.norm(P[9:] - Pn[9:]) / max(np.linalg.norm(Pn[9:]), 1.0))


def _near(lhs, rhs):
    with np.errstate(invalid="ignore"):
        return np.abs(lhs - rhs) <= NEAR * np.maximum(np.abs(lhs), np.abs(rhs))


def check_case(case, out, stage_a=True):
    """out: the device's (or a restatement's) outputs as numpy arrays -- R (B,3,3), t (B,3), inliers (B,N), status (B,), hypotheses
    (B,iterations,14), steps (B,4,14), Q, lifted, n_lifted.  Raises StageError at the first difference; -> dict(near: decisions within
    1e-9 of their boundary, order: the case's summation-order difference (dR, dt), seen: the largest pose difference to the numpy
    rule, margin: 16 x order, hyps: hypothesis records replayed)"""
    near, order, seen, pending = [], [0.0, 0.0], [0.0, 0.0], []
    nh = 0
    for b in range(case.B):
        X, _, _, _ = case.crop(b)
        Q, lf = case.lifted(b)
        if stage_a:
            if not np.array_equal(np.asarray(out["lifted"][b]) != 0, lf):
                raise StageError("A", b, "lifted differs at keypoints %r" % (np.nonzero((np.asarray(out["lifted"][b]) != 0) != lf)[0][:8].tolist(),))
            if not np.array_equal(_bits(np.asarray(out["Q"][b], np.float32)), _bits(Q)):
                raise StageError("A", b, "Q differs in its bits")
            if int(out["n_lifted"][b]) != int(lf.sum()):
                raise StageError("A", b, "n_lifted %d, expected %d" % (int(out["n_lifted"][b]), int(lf.sum())))
        idx = np.nonzero(lf)[0]
        n, it, thr = len(idx), case.iterations, case.thr_of(b)
        Xl, Ql = X[idx], Q[idx].astype(np.float64)
        hyp, steps = np.asarray(out["hypotheses"][b]), np.asarray(out["steps"][b])
        pose = np.concatenate([np.asarray(out["R"][b], np.float64).reshape(9), np.asarray(out["t"][b], np.float64).reshape(3)])
        inl, status = np.asarray(out["inliers"][b]).astype(bool), int(out["status"][b])

        def fallback(why):
            if status != 0 or not np.array_equal(_bits(pose), _bits(IDENTITY)) or inl.any():
                raise StageError("B", b, "%s: expected status 0, the identity (bitwise) and no inliers, got status %d" % (why, status))
            if not np.isnan(steps).all():
                raise StageError("C", b, "%s: step records written" % why)

        if n < 3 or not (thr > 0.0 and math.isfinite(thr)):
            fallback("%d lifted keypoints" % n)
            if not np.isnan(hyp).all():
                raise StageError("B", b, "hypothesis records written for a crop that falls back")
            continue
        thr2 = thr * thr

        def inliers_of(P, what):
            r2 = residual2(P, Xl, Ql)
            if _near(r2, thr2).any():
                near.append((b, what, "inlier test"))
            return r2 <= thr2

        def compare(P, Pn, Pp, what):
            o = _pose_diff(Pp, Pn)
            d = _pose_diff(P, Pn)
            for k in range(2):
                order[k], seen[k] = max(order[k], o[k]), max(seen[k], d[k])
            pending.append((b, what, d))

        # ---- stage B: the rounds
        bc, bh, bp = 2, -1, None
        r = 0
        while ROUND * r < it:
            for h in range(ROUND * r, min(ROUND * (r + 1), it)):
                s = sample3(case.seed, b, h, n)
                lhs, rhs = degeneracy(Xl[s])
                if _near(np.float64(lhs), np.float64(rhs)):
                    near.append((b, "hypothesis %d" % h, "degeneracy test"))
                Pn = minimal_pose(Xl[s], Ql[s])
                c = hyp[h, 0]
                if np.isnan(c):
                    raise StageError("B", b, "hypothesis %d of round %d has no record" % (h, r))
                if Pn is None:
                    if c != -1.0:
                        raise StageError("B", b, "hypothesis %d (sample %r) is degenerate, its record says %r" % (h, s, c))
                    continue
                if c < 0:
                    raise StageError("B", b, "hypothesis %d (sample %r) is not degenerate, its record says %r" % (h, s, c))
                P = hyp[h, 2:]
                if not np.isfinite(P).all():
                    raise StageError("B", b, "hypothesis %d: pose not finite" % h)
                compare(P, Pn, minimal_pose(Xl[s], Ql[s], order=(2, 0, 1)), "hypothesis %d" % h)
                cn = int(inliers_of(P, "hypothesis %d" % h).sum())
                if cn != int(c):
                    raise StageError("B", b, "hypothesis %d: %d inliers under its recorded pose, its record says %d" % (h, cn, int(c)))
                nh += 1
                if cn > bc:
                    bc, bh, bp = cn, h, P.copy()
            r += 1
            need, real = needed_iters(bc if bh >= 0 else -1, n, 3, it)
            if real is not None and abs(real - ROUND * r) <= 0.5 + 1e-6 and ROUND * r < it:
                near.append((b, "round %d" % r, "stopping rule"))
            if not ROUND * r < need:
                break
        if not np.isnan(hyp[min(ROUND * r, it):]).all():
            raise StageError("B", b, "records written behind round %d, which the stopping rule cut off" % (r - 1))
        if bh < 0:
            fallback("no hypothesis with 3 inliers")
            continue
        # ---- stage C
        if status != 1:
            raise StageError("C", b, "status %d, expected 1 (winner: hypothesis %d with %d inliers)" % (status, bh, bc))
        P, L = bp, inliers_of(bp, "winner")
        k_ran = 0
        for k in range(STEPS):
            rec = steps[k]
            if k == 0:
                Lk, grow = L, True
            else:
                Lk = inliers_of(P, "step %d" % k)
                grow = Lk.sum() > L.sum()
            Pn = fit(Xl, Ql, Lk) if grow else None
            ok = grow and Pn is not None
            if np.isnan(rec[0]) or int(rec[0]) != int(Lk.sum()) or rec[1] != float(ok):
                raise StageError("C", b, "step %d: expected [%d inliers, accepted %d], the record says [%r, %r]" % (k, Lk.sum(), ok, rec[0], rec[1]))
            if ok:
                compare(rec[2:], Pn, fit(Xl, Ql, Lk, permuted_sum), "step %d" % k)
                P, L = rec[2:].copy(), Lk
            elif not np.array_equal(_bits(rec[2:]), _bits(P)):
                raise StageError("C", b, "step %d was not accepted, but its record's pose is not the state's" % k)
            k_ran = k + 1
            if not ok:
                break
        if not np.isnan(steps[k_ran:]).all():
            raise StageError("C", b, "step records written behind step %d" % (k_ran - 1))
        if not np.array_equal(_bits(pose), _bits(P)):
            raise StageError("C", b, "the returned pose is not the last accepted state")
        want = np.zeros(case.N, bool)
        want[idx] = L
        if not np.array_equal(inl, want):
            raise StageError("C", b, "inliers differ at keypoints %r" % (np.nonzero(inl != want)[0][:8].tolist(),))
    margin = [MARGIN_FACTOR * o for o in order]
    for b, what, d in pending:
        if not (d[0] <= margin[0] and d[1] <= margin[1]):
            raise StageError("P", b, "%s: pose off the numpy rule's by |dR| = %.3e (margin %.3e), |dt|/|t| = %.3e (margin %.3e)"
                             % (what, d[0], margin[0], d[1], margin[1]))
    return dict(near=near, order=tuple(order), seen=tuple(seen), margin=tuple(margin), hyps=nh)


if __name__ == "__main__":
    for name in CASES:
        c = make(name)
        res = check_case(c, restatement_outputs(c))
        o = restatement_outputs(c)
        print("%-16s B %d N %4d lifted %-22s status %-12s winner %-18s order dR %.3e dt %.3e near %d"
              % (name, c.B, c.N, o["n_lifted"].tolist(), o["status"].tolist(), o["winner"].tolist(), res["order"][0], res["order"][1], len(res["near"])))
        for b in c.converging:
            X = c.crop(b)[0]
            print("    crop %d: inliers %d, ADD %.3f" % (b, o["inliers"][b].sum(), add_error(X, o["R"][b], o["t"][b], *c.truth[b])))
