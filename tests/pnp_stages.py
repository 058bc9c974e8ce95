"""TEST INFRASTRUCTURE (not collected): cp_pnp_ransac checked stage by stage by replaying the decisions the device itself recorded.

The device leaves one 14-double record per hypothesis in its scratch ([count, unused, R (9), t (3)] at (b * iterations + h) * 14;
postprocess.solve_pnp_ransac(return_hypotheses=True) pre-fills it with NaN and hands it back).  A 5-point hypothesis' POSE is
ambiguous by nature under noise (M^T M has a two-dimensional null space whose basis the eigen-solver is free to choose), every
other stage is exact given that pose, and `check_crop` checks each of them in numpy float64 against oracle/pnp_oracle.py:

  A  which records exist      the stopping rule (needed_iterations between rounds of 64) replayed on the recorded counts
  B  scoring                  R a proper rotation; count == #valid points with squared reprojection error <= thr^2 under the
                              RECORDED pose; -1 only where the oracle's epnp on the same sample fails too
  C  selection                winner = first record with the largest count >= 5; the returned mask is its inlier set; status
  D  refit                    oracle epnp over the DEVICE's inlier list == the returned pose within TAU_R / TAU_T, for ONE of
                              the 8 orientations of the oracle's control-point axes (below)
  E  known answers            (noise-free crops) a hypothesis whose sample holds no outlier counts exactly the valid non-outlier
                              points and has the true pose within E_MARGIN_R / E_MARGIN_T
  (nv == 4: no RANSAC but P3P -- no records, pose against the oracle's solve_four_points; nv < 4: the identity fallback.)

The band of stage B / C: a (point, hypothesis) pair whose squared error lies within BAND * thr^2 of thr^2 is undecided.  The
error is ~30 fp64 operations on values up to ~1e3 px with a difference of order thr, i.e. a relative evaluation error of order
1e-12; 1e-9 leaves three orders for contraction and ordering differences.  At most UNDECIDED_CAP of a case's pairs may be
undecided (`check_case` asserts it; the inputs are continuous, so the expected number is zero, and it IS zero on the oracle's own
records for every committed case: tests/test_pnp_stages.py).

Stage D and the orientation of the control-point axes.  EPnP puts its control points on the PCA axes of the model points; the sign
of an eigenvector is the eigen-solver's free choice (LAPACK in the oracle, cyclic Jacobi on the device), and EPnP's linearisation
is not invariant to it: the unit-norm constraint on the 12-vector of control points is a different one in each frame.  First run on
an MI355X, refit against oracle.epnp as it is: 3.0e-4 apart on a noisy crop (271 inliers), 1e-8 .. 5e-7 on noise-free ones (the
pixels' fp32 rounding is their noise), against 3.5e-14 / <= 2.7e-11 once the oracle's axes are oriented as the device's were.  So
the refit is unique only up to these 8 orientations, stage D accepts the one that fits, and TAU stays what was measured: a refit
over a wrong index list, a wrong M^T M or a wrong candidate is off by orders more than TAU from all eight.

Measured constants (all on the reference side, on a CPU; re-derived and asserted on every run of tests/test_pnp_stages.py:
`python -m tests.pnp_stages` prints them):
  TAU_R, TAU_T      16 x the largest |R - R'|_max and |t - t'| / |t| between oracle.epnp on a committed case's inlier set with
                    LAPACK's eigenvectors of M^T M and with those of `kernel_jacobi` (numpy restatement of the device's cyclic
                    Jacobi at its stopping criterion), capped at 1e-6 / 1e-5 (the tolerances test_pnp.py uses for exact data).
                    MEASURED_TAU below holds the largest differences seen.
  E_MARGIN_R / _T   8 x the worst deviation from the true pose of the oracle's own all-inlier hypotheses over the noise-free
                    crops of the committed cases.  MEASURED_E below holds that worst deviation.
"""
import os
import sys

import numpy as np

from oracle import pnp_oracle as P

BAND = 1e-9
UNDECIDED_CAP = 1e-6
# largest (dR, dt / |t|) between the LAPACK and the Jacobi refit over the committed cases / worst (dR, dt / |t|) of the oracle's
# all-inlier hypotheses: printed by `python -m tests.pnp_stages`, asserted (as upper bounds that a quarter of them would miss) in
# tests/test_pnp_stages.py::test_measured_constants
MEASURED_TAU = (2.5e-11, 2.7e-11)           # seen: 2.453e-11, 2.667e-11, both on shape_256x512 -> TAU_R = 4.0e-10, TAU_T = 4.3e-10
MEASURED_E = (8.5e-06, 1.9e-06)             # seen: 8.481e-06 (shape_256x512), 1.887e-06 (column_1): the pixels' fp32 rounding
TAU_CAP = (1e-6, 1e-5)

K_LMO = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1.0]]).astype(np.float32).astype(np.float64)
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "checkerpose_amd", "data")


def taus():
    return min(16 * MEASURED_TAU[0], TAU_CAP[0]), min(16 * MEASURED_TAU[1], TAU_CAP[1])


def e_margins():
    return 8 * MEASURED_E[0], 8 * MEASURED_E[1]


class StageError(AssertionError):
    def __init__(self, stage, crop, hyp, what):
        self.stage, self.crop, self.hyp = stage, crop, hyp
        super().__init__("stage %s, crop %d, hypothesis %s: %s" % (stage, crop, "-" if hyp is None else hyp, what))


def kernel_jacobi(A):
    """csrc/pnp.hip:jacobi_eig12_wave in numpy: cyclic Jacobi, at most 30 sweeps, stop when the off-diagonal mass is below 1e-26
    of the diagonal's, a rotation skipped when apq^2 <= 1e-34 |app aqq|.  -> (ascending eigenvalues, eigenvectors in columns)"""
    a = np.array(A, np.float64)
    n = a.shape[0]
    v = np.eye(n)
    for _ in range(30):
        diag = float((np.diag(a) ** 2).sum())
        off = float((np.triu(a, 1) ** 2).sum())
        if off <= 1e-26 * diag or off == 0.0:
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq, app, aqq = a[p, q], a[p, p], a[q, q]
                if apq * apq <= 1e-34 * abs(app * aqq) or apq == 0.0:
                    continue
                theta = (aqq - app) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                akp, akq = a[:, p].copy(), a[:, q].copy()
                a[:, p], a[:, q] = c * akp - s * akq, s * akp + c * akq
                apk, aqk = a[p, :].copy(), a[q, :].copy()
                a[p, :], a[q, :] = c * apk - s * aqk, s * apk + c * aqk
                vkp, vkq = v[:, p].copy(), v[:, q].copy()
                v[:, p], v[:, q] = c * vkp - s * vkq, s * vkp + c * vkq
    order = np.argsort(np.diag(a), kind="stable")
    return np.diag(a)[order], v[:, order]


AXIS_SIGNS = [(a, b, c) for a in (1.0, -1.0) for b in (1.0, -1.0) for c in (1.0, -1.0)]


def _oracle_epnp(pw, uv, K, eig=None, axis_signs=AXIS_SIGNS[0]):
    """oracle.epnp, None where it is degenerate (raises, or no candidate with a finite error)"""
    try:
        with np.errstate(all="ignore"):
            R, t, err = P.epnp(pw, uv, K, eig, axis_signs)
    except np.linalg.LinAlgError:
        return None
    return (R, t) if np.isfinite(err) else None


def _sq_errors(pw, uv, K, Rs, ts):
    """squared reprojection errors (H, n) of n points under H poses (Rs (H,3,3), ts (H,3)); NaN / inf where the projection is"""
    with np.errstate(all="ignore"):
        pc = np.einsum("hij,nj->hni", Rs, pw) + ts[:, None, :]
        u = K[0, 2] + K[0, 0] * pc[..., 0] / pc[..., 2]
        v = K[1, 2] + K[1, 1] * pc[..., 1] / pc[..., 2]
        return (u - uv[None, :, 0]) ** 2 + (v - uv[None, :, 1]) ** 2


def expected_rounds(counts, nv, iterations):
    """how many hypothesis records the stopping rule demands, replayed from the recorded counts (NaN = unwritten: reads as -1)"""
    if nv < 5:
        return 0
    done, best = min(iterations, 64), -1
    r = 1
    while 64 * r < iterations:
        c = counts[64 * (r - 1):64 * r]
        c = c[~np.isnan(c)]
        best = max(best, int(c.max()) if len(c) else -1)
        if 64 * r >= P.needed_iterations(best, nv, 5, iterations):
            break
        done = min(iterations, 64 * (r + 1))
        r += 1
    return done


def check_crop(p3d, p2d, valid, K, thr, iterations, seed, crop, records, R, t, inliers, status, truth=None):
    """Raises StageError (stage, crop, hypothesis in the message) where the device's outputs contradict its own records or the
    oracle.  p3d (N,3), p2d (N,2), valid (N,) (one column), K (3,3): the values the device read (fp32-representable); records
    (iterations, 14); R (3,3), t (3,), inliers (N,), status: what it returned.  truth = (R, t, outlier mask (N,)) switches
    stage E on (noise-free crops only).  Returns the statistics `check_case` sums up."""
    p3d, p2d, K = np.asarray(p3d, np.float64), np.asarray(p2d, np.float64), np.asarray(K, np.float64)
    valid, inliers = np.asarray(valid).astype(bool), np.asarray(inliers).astype(bool)
    records, R, t = np.asarray(records, np.float64), np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    N = len(p3d)
    vid = np.nonzero(valid)[0]
    nv = len(vid)
    thr2 = float(np.float32(thr)) ** 2
    stats = dict(pairs=0, undecided=0, written=0, rounds=0, all_inlier=0, degenerate=0)
    if records.shape != (iterations, P.HYP_DOUBLES):
        raise StageError("A", crop, None, "records have shape %r" % (records.shape,))

    # ---- A: which records exist
    need = expected_rounds(records[:, 0], nv, iterations)
    written = ~np.isnan(records[:, 0])
    for h in range(iterations):
        if h < need and not written[h]:
            raise StageError("A", crop, h, "record missing: the stopping rule demands %d hypotheses (nv = %d)" % (need, nv))
        if h >= need and not np.isnan(records[h]).all():
            raise StageError("A", crop, h, "record written beyond the %d hypotheses the stopping rule demands (nv = %d)" % (need, nv))
    stats["written"], stats["rounds"] = need, (need + 63) // 64
    counts = records[:need, 0]
    if need and not (np.all(counts == np.rint(counts)) and counts.min() >= -1 and counts.max() <= nv):
        raise StageError("A", crop, int(np.argmax((counts != np.rint(counts)) | (counts < -1) | (counts > nv))), "count is no integer in -1..nv")

    def identity_expected(stage, why):
        if status != 0 or not np.array_equal(R, np.eye(3)) or t.any() or inliers.any():
            raise StageError(stage, crop, None, "%s: expected the identity pose, no inliers, status 0; got status %d, %d inliers" % (why, status, inliers.sum()))

    if nv < 4:
        identity_expected("C", "%d valid points" % nv)
        return stats
    if nv == 4:                                                # no RANSAC: P3P on the first three, the fourth one picks
        rt = P.solve_four_points(p3d[vid], p2d[vid], K)
        if rt is None:
            identity_expected("C", "4 valid points without a P3P solution")
            return stats
        if status != 1 or not np.array_equal(inliers, valid):
            raise StageError("C", crop, None, "4 valid points: status %d, inliers != the valid column" % status)
        if not (np.abs(R - rt[0]).max() <= TAU_CAP[0] and np.abs(t - rt[1]).max() <= TAU_CAP[1] * max(1.0, np.linalg.norm(rt[1]))):
            raise StageError("D", crop, None, "P3P pose off the oracle's by %.3e / %.3e" % (np.abs(R - rt[0]).max(), np.abs(t - rt[1]).max()))
        return stats

    # ---- B: scoring under the recorded poses
    posed = np.nonzero(counts >= 0)[0]
    Rs, ts = records[posed, 2:11].reshape(-1, 3, 3), records[posed, 11:14]
    if not np.isfinite(records[posed, 2:14]).all():
        raise StageError("B", crop, int(posed[np.argmax(~np.isfinite(records[posed, 2:14]).all(1))]), "count >= 0 with a non-finite pose")
    for h in np.nonzero(counts < 0)[0]:
        stats["degenerate"] += 1
        s = vid[P.sample_indices(seed, crop, int(h), nv, 5)]
        if _oracle_epnp(p3d[s], p2d[s], K) is not None:
            raise StageError("B", crop, int(h), "count -1, but the oracle's epnp solves the sample %r" % (s.tolist(),))
    if len(posed):
        ortho = np.abs(np.einsum("hji,hjk->hik", Rs, Rs) - np.eye(3)).max((1, 2))
        det = np.abs(np.linalg.det(Rs) - 1.0)
        bad = np.nonzero((ortho > 1e-12) | (det > 1e-12))[0]
        if len(bad):
            raise StageError("B", crop, int(posed[bad[0]]), "R is no proper rotation: |R^T R - I| = %.3e, |det - 1| = %.3e" % (ortho[bad[0]], det[bad[0]]))
        d2 = _sq_errors(p3d[vid], p2d[vid], K, Rs, ts)                     # (H, nv)
        with np.errstate(invalid="ignore"):
            lo, hi = (d2 <= thr2 * (1.0 - BAND)).sum(1), (d2 <= thr2 * (1.0 + BAND)).sum(1)
            und = (d2 <= thr2 * (1.0 + BAND)) & ~(d2 <= thr2 * (1.0 - BAND))
        stats["pairs"] += d2.size
        stats["undecided"] += int(und.sum())
        c = counts[posed]
        bad = np.nonzero((c < lo) | (c > hi))[0]
        if len(bad):
            raise StageError("B", crop, int(posed[bad[0]]), "count %d, but %d..%d valid points lie within thr under the recorded pose"
                             % (c[bad[0]], lo[bad[0]], hi[bad[0]]))

    # ---- C: selection
    if inliers.shape != (N,) or (inliers & ~valid).any():
        raise StageError("C", crop, None, "inliers outside the valid column: %r" % (np.nonzero(inliers & ~valid)[0][:8].tolist(),))
    if not need or counts.max() < 5:
        identity_expected("C", "no hypothesis with 5 inliers")
        return stats
    win = int(np.argmax(counts))                                           # the first of the largest
    if status != 1:
        raise StageError("C", crop, win, "status %d with a winner of %d inliers" % (status, counts[win]))
    w = int(np.nonzero(posed == win)[0][0])
    sure_in, sure_out = d2[w] <= thr2 * (1.0 - BAND), ~(d2[w] <= thr2 * (1.0 + BAND))
    got = inliers[vid]
    if (sure_in & ~got).any() or (sure_out & got).any():
        diff = vid[(sure_in & ~got) | (sure_out & got)]
        raise StageError("C", crop, win, "the returned mask (%d) is not the winner's inlier set (%d): differs at %r"
                         % (got.sum(), sure_in.sum(), diff[:8].tolist()))

    # ---- D: refit over the device's inlier list (the oracle in each orientation of its control-point axes: AXIS_SIGNS)
    sel = np.nonzero(inliers)[0]
    fits = [rt for rt in (_oracle_epnp(p3d[sel], p2d[sel], K, None, sg) for sg in AXIS_SIGNS) if rt is not None]
    if not fits:
        if not (np.array_equal(R.reshape(9), records[win, 2:11]) and np.array_equal(t, records[win, 11:14])):
            raise StageError("D", crop, win, "degenerate refit (%d inliers): the returned pose is not the winner's record" % len(sel))
    else:
        tau_R, tau_t = taus()
        dR, dt = min(((np.abs(R - rt[0]).max(), np.linalg.norm(t - rt[1]) / np.linalg.norm(rt[1])) for rt in fits),
                     key=lambda d: max(d[0] / tau_R, d[1] / tau_t))
        stats["refit_1e15"] = max(stats.get("refit_1e15", 0), int(1e15 * max(dR, dt)))
        if not (dR <= tau_R and dt <= tau_t):
            raise StageError("D", crop, win, "refit over %d inliers off the oracle's: |dR| = %.3e (tau %.3e), |dt|/|t| = %.3e (tau %.3e)"
                             % (len(sel), dR, tau_R, dt, tau_t))

    # ---- E: known answers of the all-inlier samples of a noise-free crop
    if truth is not None:
        Rt, tt, out = np.asarray(truth[0], np.float64), np.asarray(truth[1], np.float64), np.asarray(truth[2]).astype(bool)
        n_true = int((valid & ~out).sum())
        mR, mt = e_margins()
        for h in range(need):
            s = vid[P.sample_indices(seed, crop, h, nv, 5)]
            if out[s].any():
                continue
            stats["all_inlier"] += 1
            if counts[h] != n_true:
                raise StageError("E", crop, h, "all-inlier sample %r counts %d, the crop has %d valid non-outliers" % (s.tolist(), counts[h], n_true))
            dR = np.abs(records[h, 2:11].reshape(3, 3) - Rt).max()
            dt = np.linalg.norm(records[h, 11:14] - tt) / np.linalg.norm(tt)
            if not (dR <= mR and dt <= mt):
                raise StageError("E", crop, h, "all-inlier sample %r: pose off the true one by |dR| = %.3e (margin %.3e), |dt|/|t| = %.3e (%.3e)"
                                 % (s.tolist(), dR, mR, dt, mt))
    return stats


# ------------------------------------------------------------------------------------------------------------- the committed cases
def _pose(rng, tz=(500.0, 1300.0)):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = rng.uniform(0.1, np.pi - 0.1)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx, np.array([rng.uniform(-120, 120), rng.uniform(-90, 90), rng.uniform(*tz)])


def lmo_model(n):
    return np.load(os.path.join(DATA, "fps_lmo_obj01.npy"))[:n].astype(np.float32).astype(np.float64)


def _crop(rng, xyz, K, outlier_frac, noise, valid_frac, pose=None):
    """one crop: (p2d (N,2) fp32-representable, valid (N,), truth (R, t, outlier mask))"""
    n = len(xyz)
    R, t = _pose(rng) if pose is None else pose
    with np.errstate(all="ignore"):
        uv = P.project(xyz, K, R, t)
    out = rng.random(n) < outlier_frac
    uv = uv + rng.normal(scale=noise, size=uv.shape) if noise else uv
    uv[out] += rng.uniform(20, 80, size=(int(out.sum()), 2)) * rng.choice([-1, 1], size=(int(out.sum()), 2))
    valid = rng.random(n) < valid_frac
    return uv.astype(np.float32).astype(np.float64), valid, (R, t, out)


class Case:
    """p3d (N,3) shared or (B,N,3); p2d (B,N,2); valid (B,N,3) uint8; K (3,3) shared or (B,3,3); truth: per crop (R, t, out) or None
    (noisy / degenerate crops: no stage E); full_oracle: the crops whose pose, mask and status must equal the full oracle's;
    min_rounds: stage A must find at least this many rounds written on every crop with >= 5 valid points"""

    def __init__(self, name, p3d, p2d, valid, K=K_LMO, column=0, thr=2.0, iterations=150, seed=1, truth=None, full_oracle=(),
                 min_rounds=1, oracle_status=False):
        self.name, self.p3d, self.p2d, self.valid, self.K = name, p3d, p2d, valid.astype(np.uint8), K
        self.column, self.thr, self.iterations, self.seed = column, thr, iterations, seed
        self.B, self.N = p2d.shape[:2]
        self.truth = truth if truth is not None else [None] * self.B
        self.full_oracle, self.min_rounds, self.oracle_status = tuple(full_oracle), min_rounds, oracle_status

    def crop(self, b):
        return (self.p3d[b] if self.p3d.ndim == 3 else self.p3d, self.p2d[b], self.valid[b, :, self.column].astype(bool),
                self.K[b] if self.K.ndim == 3 else self.K)


def _standard(name, seed, B, N, outlier_frac=0.3, noise=0.0, valid_frac=0.8, model=None, K=K_LMO, full=False, **kw):
    rng = np.random.default_rng(seed)
    xyz = lmo_model(N) if model is None else model
    crops = []
    for b in range(B):
        of = outlier_frac[b % len(outlier_frac)] if isinstance(outlier_frac, tuple) else outlier_frac
        nz = noise[b % len(noise)] if isinstance(noise, tuple) else noise
        crops.append((_crop(rng, xyz[b] if xyz.ndim == 3 else xyz, K[b] if K.ndim == 3 else K, of, nz, valid_frac), nz))
    valid = np.zeros((B, N, 3), np.uint8)
    valid[:, :, 0] = np.stack([c[0][1] for c in crops])
    return Case(name, xyz, np.stack([c[0][0] for c in crops]), valid, K, truth=[None if nz else c[2] for c, nz in crops],
                full_oracle=range(B) if full is True else (full or ()), seed=seed, **kw)


def _lm_models():
    tab = np.load(os.path.join(DATA, "fps_lm_15x4096.npy"))
    return tab[[0, 7, 14]].astype(np.float32).astype(np.float64)                        # mixed objects, one model per crop


def _per_crop_K(B):
    Ks = np.stack([K_LMO] * B)
    for b in range(B):
        Ks[b, 0, 0] *= 1.0 + 0.11 * (b + 1)
        Ks[b, 1, 1] *= 1.0 - 0.07 * (b + 1)
        Ks[b, 0, 2] += 13.0 * (b + 1)
        Ks[b, 1, 2] -= 9.0 * (b + 1)
    return Ks.astype(np.float32).astype(np.float64)


def _columns(column):
    rng = np.random.default_rng(40)
    xyz = lmo_model(512)
    crops = [_crop(rng, xyz, K_LMO, 0.3, 0.0, 1.0) for _ in range(3)]
    valid = np.stack([rng.random((3, 512)) < f for f in (0.9, 0.6, 0.3)], 2)            # three different masks with real content
    return Case("column_%d" % column, xyz, np.stack([c[0] for c in crops]), valid, column=column, truth=[c[2] for c in crops], seed=40)


def _edge(kind):
    rng = np.random.default_rng(50)
    N, B = 512, 2
    xyz = lmo_model(N)
    valid = np.zeros((B, N, 3), np.uint8)
    valid[:, :, 0] = rng.random((B, N)) < 0.8
    pose = [None] * B
    if kind == "coplanar":
        xyz = xyz.copy()
        xyz[:, 2] = 0.0
    elif kind == "collinear":
        xyz = np.stack([xyz[:, 0], np.zeros(N), np.zeros(N)], 1)
    elif kind == "identical":
        xyz = np.repeat(xyz[:1], N, 0)
    elif kind == "behind_camera":                           # t_z small against the model radius (~46 mm): part of the model behind
        pose = [(_pose(rng)[0], np.array([3.0, -2.0, 12.0 + 9.0 * b])) for b in range(B)]
    crops = [_crop(rng, xyz, K_LMO, 0.2, 0.0, 1.0, pose[b]) for b in range(B)]
    p2d = np.stack([c[0] for c in crops])
    if kind == "random_p2d":
        p2d = rng.uniform(0, 640, size=p2d.shape).astype(np.float32).astype(np.float64)
    return Case("edge_" + kind, xyz, p2d, valid, seed=50, oracle_status=True)


EDGES = ("coplanar", "collinear", "identical", "random_p2d", "behind_camera")
ITERATIONS = (1, 5, 63, 64, 65, 128, 150, 256)
CASES = {
    "shape_6x512": lambda: _standard("shape_6x512", 11, 6, 512, full=True),
    "shape_3x4096_lm": lambda: _standard("shape_3x4096_lm", 12, 3, 4096, model=_lm_models(), full=True),
    "shape_4x100": lambda: _standard("shape_4x100", 13, 4, 100, 0.2, valid_frac=0.9, full=True),
    "shape_4x65": lambda: _standard("shape_4x65", 14, 4, 65, 0.2, valid_frac=0.9, full=True),
    "shape_4x33": lambda: _standard("shape_4x33", 15, 4, 33, 0.2, valid_frac=0.9, full=True),
    "shape_2x5": lambda: _standard("shape_2x5", 16, 2, 5, 0.0, valid_frac=1.0, full=True),
    "shape_2x6": lambda: _standard("shape_2x6", 17, 2, 6, 0.0, valid_frac=1.0, full=True),
    "shape_256x512": lambda: _standard("shape_256x512", 18, 256, 512, full=range(0, 256, 32)),
    "per_crop_K": lambda: _standard("per_crop_K", 19, 4, 512, K=_per_crop_K(4), full=True),
    "thr_0.5": lambda: _standard("thr_0.5", 20, 3, 512, noise=(0.5, 0.5, 0.0), thr=0.5),
    "thr_2": lambda: _standard("thr_2", 20, 3, 512, noise=(0.5, 0.5, 0.0), thr=2.0),
    "thr_8": lambda: _standard("thr_8", 20, 3, 512, noise=(0.5, 0.5, 0.0), thr=8.0),
    "outliers_0": lambda: _standard("outliers_0", 30, 3, 512, 0.0),
    "outliers_0.3": lambda: _standard("outliers_0.3", 31, 3, 512, 0.3),
    "outliers_0.6": lambda: _standard("outliers_0.6", 32, 3, 512, 0.6, min_rounds=2),
    "outliers_0.85": lambda: _standard("outliers_0.85", 33, 3, 512, 0.85, min_rounds=2),
}
for _it in ITERATIONS:      # crops alternate between 30 % outliers (the rule stops after one round) and 60 % (it never stops)
    CASES["iterations_%d" % _it] = lambda _it=_it: _standard("iterations_%d" % _it, 60, 4, 512, (0.3, 0.6), iterations=_it)
for _c in range(3):
    CASES["column_%d" % _c] = lambda _c=_c: _columns(_c)
for _k in EDGES:
    CASES["edge_" + _k] = lambda _k=_k: _edge(_k)


def oracle_outputs(case):
    """the oracle's own run of a case in the device's output layout: (records (B,it,14), R (B,3,3), t (B,3), inliers (B,N), status (B,))"""
    rec = np.full((case.B, case.iterations, P.HYP_DOUBLES), np.nan)
    R, t = np.zeros((case.B, 3, 3)), np.zeros((case.B, 3))
    inl, status = np.zeros((case.B, case.N), bool), np.zeros(case.B, np.int32)
    for b in range(case.B):
        p3, p2, va, K = case.crop(b)
        rec[b] = P.hypothesis_records(p3, p2, va, K, case.thr, case.iterations, case.seed, b)
        R[b], t[b], inl[b], status[b] = P.solve_pnp_ransac(p3, p2, va, K, case.thr, case.iterations, case.seed, b, records=rec[b])
    return rec, R, t, inl, status


def check_case(case, records, R, t, inliers, status, log=None):
    """check_crop on every crop of a case + the conditions that hold per case: the undecided cap, min_rounds.  -> summed statistics"""
    total = {}
    for b in range(case.B):
        p3, p2, va, K = case.crop(b)
        st = check_crop(p3, p2, va, K, case.thr, case.iterations, case.seed, b, records[b], R[b], np.asarray(t[b]).reshape(3),
                        inliers[b], int(status[b]), truth=case.truth[b])
        if va.sum() >= 5 and st["rounds"] < case.min_rounds:
            raise StageError("A", b, None, "only %d round(s) written: the case is there to exercise %d" % (st["rounds"], case.min_rounds))
        for k, v in st.items():
            total[k] = max(total.get(k, 0), v) if k == "refit_1e15" else total.get(k, 0) + v
    total["status1"] = int(np.asarray(status).sum())
    if log is not None:
        log("%-18s %s" % (case.name, " ".join("%s=%d" % kv for kv in sorted(total.items()))))
    assert total["undecided"] <= UNDECIDED_CAP * total["pairs"], (case.name, total)
    return total


def measure_tau(case, inliers, status):
    """largest (|dR|, |dt| / |t|) between oracle.epnp with LAPACK's and with the kernel's Jacobi eigenvectors over a case's inlier sets"""
    worst = [0.0, 0.0]
    for b in range(case.B):
        p3, p2, va, K = case.crop(b)
        sel = np.nonzero(inliers[b])[0]
        if not status[b] or va.sum() < 5:
            continue
        a, j = _oracle_epnp(p3[sel], p2[sel], K), _oracle_epnp(p3[sel], p2[sel], K, kernel_jacobi)
        if a is None or j is None:
            assert a is None and j is None, (case.name, b)
            continue
        worst[0] = max(worst[0], float(np.abs(a[0] - j[0]).max()))
        worst[1] = max(worst[1], float(np.linalg.norm(a[1] - j[1]) / np.linalg.norm(a[1])))
    return worst


def measure_e(case, records):
    """worst (|dR|, |dt| / |t|) from the true pose over the oracle's own all-inlier hypotheses of a case's noise-free crops"""
    worst = [0.0, 0.0]
    for b in range(case.B):
        if case.truth[b] is None:
            continue
        p3, p2, va, K = case.crop(b)
        vid = np.nonzero(va)[0]
        Rt, tt, out = case.truth[b]
        for h in np.nonzero(~np.isnan(records[b, :, 0]))[0]:
            if out[vid[P.sample_indices(case.seed, b, int(h), len(vid), 5)]].any() or records[b, h, 0] < 0:
                continue
            worst[0] = max(worst[0], float(np.abs(records[b, h, 2:11].reshape(3, 3) - Rt).max()))
            worst[1] = max(worst[1], float(np.linalg.norm(records[b, h, 11:14] - tt) / np.linalg.norm(tt)))
    return worst


if __name__ == "__main__":
    import time
    tau, e = [0.0, 0.0], [0.0, 0.0]
    for name in (sys.argv[1:] or CASES):
        t0 = time.time()
        case = CASES[name]()
        rec, R, t, inl, status = oracle_outputs(case)
        a, b = measure_tau(case, inl, status), measure_e(case, rec)
        tau, e = [max(x, y) for x, y in zip(tau, a)], [max(x, y) for x, y in zip(e, b)]
        print("%-18s tau %.3e %.3e   E %.3e %.3e   status %s  (%.1f s)" % (name, a[0], a[1], b[0], b[1], status.tolist()[:8], time.time() - t0), flush=True)
    print("MEASURED_TAU = (%.3e, %.3e)\nMEASURED_E = (%.3e, %.3e)" % (tau[0], tau[1], e[0], e[1]))
