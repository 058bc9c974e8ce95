"""TEST INFRASTRUCTURE (not collected): the rule of row N33 (csrc/pnp_conf.hip: ranked set, PROSAC pool, whitened gate) in numpy, and
cp_pnp_conf checked stage by stage by replaying the decisions the device itself recorded -- tests/pnp_stages.py's method, on its
constants: BAND, UNDECIDED_CAP, taus(), e_margins(), the 8 axis orientations of the oracle's EPnP.  No tolerance is invented here.

  rank(sigma2, valid)                     the ranked set: order (N,) int32 (-1 beyond nv), nv, n_dropped
  pool_size(h, nv, iterations, guided)    n_h in exact (Python) integers
  hypothesis_records(...), solve(...)     the solver on oracle.pnp_oracle's epnp / sample_indices / needed_iterations / solve_four_points

`check_crop` stages:
  R  order / n_ranked / n_dropped equal the rule exactly
  P  every written record's slot 1 equals pool_size(h)
  A  which records exist: the stopping rule replayed on the recorded counts (nv = the ranked points)
  B  the recorded R is a proper rotation; count == the whitened gate under the RECORDED pose (a pair within BAND * chi2 of chi2 is
     undecided; at most UNDECIDED_CAP of a case's pairs may be); -1 only where the oracle's epnp on the replayed sample fails too
  C  the winner (first record with the largest count >= 5) and the returned mask; status; inliers inside the ranked set
  D  the oracle's epnp over the DEVICE's inlier list agrees within taus() for one of the 8 orientations
  E  (noise-free crops) a hypothesis whose sample has no outlier counts exactly the non-outlier ranked points, pose within e_margins()
  (nv == 4: P3P on the four ranked points in ascending keypoint order; nv < 4: the identity fallback.)
"""
import functools

import numpy as np

from oracle import pnp_oracle as P
from tests import pnp_stages as S
from tests.pnp_stages import BAND, UNDECIDED_CAP, StageError, _oracle_epnp, expected_rounds, taus

HYP = P.HYP_DOUBLES


# ------------------------------------------------------------------------------------------------------------------- the rule
def rank(sigma2, valid):
    """sigma2 (N,2) f64, valid (N,) -> (order (N,) int32: ranked keypoints by ascending sigma2_x + sigma2_y, ties by ascending index,
    -1 beyond nv; nv; n_dropped = valid keypoints whose variance is not finite and > 0 on both axes)"""
    sigma2, valid = np.asarray(sigma2, np.float64), np.asarray(valid).astype(bool)
    with np.errstate(invalid="ignore"):
        good = np.isfinite(sigma2).all(1) & (sigma2 > 0.0).all(1)
    ranked = np.nonzero(valid & good)[0]
    with np.errstate(all="ignore"):
        key = sigma2[ranked, 0] + sigma2[ranked, 1]
    order = np.full(len(valid), -1, np.int32)
    order[:len(ranked)] = ranked[np.lexsort((ranked, key))]
    return order, len(ranked), int((valid & ~good).sum())


def c5(n):
    return n * (n - 1) * (n - 2) * (n - 3) * (n - 4) // 120


def pool_size(h, nv, iterations, guided=True):
    """the smallest n in [5, nv] with C(n,5) * iterations >= (h + 1) * C(nv,5); nv when not guided"""
    if not guided:
        return nv
    need = (h + 1) * c5(nv)
    n = 5
    while c5(n) * iterations < need:
        n += 1
    return n


def sample(order, seed, crop, h, nh):
    """the five keypoints of hypothesis h: positions from the shared hash sampler over the first nh of the ranking"""
    return order[P.sample_indices(seed, crop, h, nh, 5)]


def whitened(p3d, p2d, sigma2, K, Rs, ts):
    """d2 (H, n) = du^2 / sigma2_x + dv^2 / sigma2_y of n points under H poses"""
    with np.errstate(all="ignore"):
        pc = np.einsum("hij,nj->hni", Rs, p3d) + ts[:, None, :]
        u = K[0, 2] + K[0, 0] * pc[..., 0] / pc[..., 2]
        v = K[1, 2] + K[1, 1] * pc[..., 1] / pc[..., 2]
        return (u - p2d[None, :, 0]) ** 2 / sigma2[None, :, 0] + (v - p2d[None, :, 1]) ** 2 / sigma2[None, :, 1]


def hypothesis_records(p3d, p2d, valid, sigma2, K, chi2, iterations=150, seed=0, crop=0, guided=True):
    """the RANSAC loop in the device's record layout: (iterations, 14), NaN wherever the device writes nothing"""
    p3d, p2d, sigma2 = np.asarray(p3d, np.float64), np.asarray(p2d, np.float64), np.asarray(sigma2, np.float64)
    order, nv, _ = rank(sigma2, valid)
    rec = np.full((iterations, HYP), np.nan)
    if nv < 5:
        return rec
    rid = order[:nv]
    best = -1
    for h in range(iterations):
        if h > 0 and h % 64 == 0 and h >= P.needed_iterations(best, nv, 5, iterations):
            break
        nh = pool_size(h, nv, iterations, guided)
        rec[h, 0], rec[h, 1] = -1, nh
        s = sample(order, seed, crop, h, nh)
        rt = _oracle_epnp(p3d[s], p2d[s], K)
        if rt is None:
            continue
        d2 = whitened(p3d[rid], p2d[rid], sigma2[rid], K, rt[0][None], rt[1][None])[0]
        with np.errstate(invalid="ignore"):
            rec[h, 0] = int((d2 <= chi2).sum())
        rec[h, 2:11], rec[h, 11:14] = rt[0].reshape(9), rt[1]
        best = max(best, int(rec[h, 0]))
    return rec


def solve(p3d, p2d, valid, sigma2, K, chi2, iterations=150, seed=0, crop=0, guided=True, records=None):
    """-> (R, t, inlier mask (N,), status): as oracle.pnp_oracle.solve_pnp_ransac, under the rule of row N33"""
    p3d, p2d, sigma2 = np.asarray(p3d, np.float64), np.asarray(p2d, np.float64), np.asarray(sigma2, np.float64)
    order, nv, _ = rank(sigma2, valid)
    rid = np.sort(order[:nv])
    ident = (np.eye(3), np.zeros(3), np.zeros(len(p3d), bool), 0)
    if nv < 4:
        return ident
    if nv == 4:
        rt = P.solve_four_points(p3d[rid], p2d[rid], np.asarray(K, np.float64))
        if rt is None:
            return ident
        mask = np.zeros(len(p3d), bool)
        mask[rid] = True
        return rt[0], rt[1], mask, 1
    rec = hypothesis_records(p3d, p2d, valid, sigma2, K, chi2, iterations, seed, crop, guided) if records is None else records
    counts = np.where(np.isnan(rec[:, 0]), -1, rec[:, 0])
    win = int(np.argmax(counts))
    if counts[win] < 5:
        return ident
    d2 = whitened(p3d[rid], p2d[rid], sigma2[rid], K, rec[win, 2:11].reshape(1, 3, 3), rec[win, 11:14][None])[0]
    with np.errstate(invalid="ignore"):
        sel = rid[d2 <= chi2]
    rt = _oracle_epnp(p3d[sel], p2d[sel], K)
    R, t = rt if rt is not None else (rec[win, 2:11].reshape(3, 3), rec[win, 11:14])
    mask = np.zeros(len(p3d), bool)
    mask[sel] = True
    return R, t, mask, 1


# ---------------------------------------------------------------------------------------------------------------- the checker
def check_crop(p3d, p2d, valid, sigma2, K, chi2, iterations, seed, crop, guided, records, R, t, inliers, status, order, n_ranked,
               n_dropped, truth=None):
    """Raises StageError where the device's outputs contradict its own records or the rule.  Arguments as pnp_stages.check_crop, plus
    sigma2 (N,2), chi2, guided and the ranking's three outputs.  Returns the statistics `check_case` sums up."""
    p3d, p2d, K = np.asarray(p3d, np.float64), np.asarray(p2d, np.float64), np.asarray(K, np.float64)
    sigma2 = np.asarray(sigma2, np.float64)
    valid, inliers = np.asarray(valid).astype(bool), np.asarray(inliers).astype(bool)
    records, R, t = np.asarray(records, np.float64), np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    order = np.asarray(order)
    N = len(p3d)
    stats = dict(pairs=0, undecided=0, written=0, rounds=0, all_inlier=0, degenerate=0)

    # ---- R: the ranking
    want, nv, nd = rank(sigma2, valid)
    if int(n_ranked) != nv or int(n_dropped) != nd:
        raise StageError("R", crop, None, "n_ranked %d, n_dropped %d; the rule gives %d, %d" % (n_ranked, n_dropped, nv, nd))
    if order.shape != (N,) or not np.array_equal(order, want):
        at = int(np.argmax(order != want)) if order.shape == (N,) else -1
        raise StageError("R", crop, None, "order differs from the rule at position %d: %r, expected %r" % (at, order[at:at + 4].tolist(), want[at:at + 4].tolist()))
    rid = np.sort(want[:nv])
    ranked = np.zeros(N, bool)
    ranked[rid] = True
    if records.shape != (iterations, HYP):
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

    # ---- P: the pool sizes
    pools = [pool_size(h, nv, iterations, guided) for h in range(need)]
    for h in range(need):
        if records[h, 1] != pools[h]:
            raise StageError("P", crop, h, "pool size %r, the rule gives %d (nv = %d, iterations = %d)" % (records[h, 1], pools[h], nv, iterations))

    def identity_expected(stage, why):
        if status != 0 or not np.array_equal(R, np.eye(3)) or t.any() or inliers.any():
            raise StageError(stage, crop, None, "%s: expected the identity pose, no inliers, status 0; got status %d, %d inliers" % (why, status, inliers.sum()))

    if nv < 4:
        identity_expected("C", "%d ranked points" % nv)
        return stats
    if nv == 4:
        rt = P.solve_four_points(p3d[rid], p2d[rid], K)
        if rt is None:
            identity_expected("C", "4 ranked points without a P3P solution")
            return stats
        if status != 1 or not np.array_equal(inliers, ranked):
            raise StageError("C", crop, None, "4 ranked points: status %d, inliers != the ranked set" % status)
        if not (np.abs(R - rt[0]).max() <= S.TAU_CAP[0] and np.abs(t - rt[1]).max() <= S.TAU_CAP[1] * max(1.0, np.linalg.norm(rt[1]))):
            raise StageError("D", crop, None, "P3P pose off the oracle's by %.3e / %.3e" % (np.abs(R - rt[0]).max(), np.abs(t - rt[1]).max()))
        return stats

    # ---- B: scoring under the recorded poses
    posed = np.nonzero(counts >= 0)[0]
    Rs, ts = records[posed, 2:11].reshape(-1, 3, 3), records[posed, 11:14]
    if not np.isfinite(records[posed, 2:14]).all():
        raise StageError("B", crop, int(posed[np.argmax(~np.isfinite(records[posed, 2:14]).all(1))]), "count >= 0 with a non-finite pose")
    for h in np.nonzero(counts < 0)[0]:
        stats["degenerate"] += 1
        s = sample(want, seed, crop, int(h), pools[h])
        if _oracle_epnp(p3d[s], p2d[s], K) is not None:
            raise StageError("B", crop, int(h), "count -1, but the oracle's epnp solves the sample %r" % (s.tolist(),))
    if len(posed):
        ortho = np.abs(np.einsum("hji,hjk->hik", Rs, Rs) - np.eye(3)).max((1, 2))
        det = np.abs(np.linalg.det(Rs) - 1.0)
        bad = np.nonzero((ortho > 1e-12) | (det > 1e-12))[0]
        if len(bad):
            raise StageError("B", crop, int(posed[bad[0]]), "R is no proper rotation: |R^T R - I| = %.3e, |det - 1| = %.3e" % (ortho[bad[0]], det[bad[0]]))
        d2 = whitened(p3d[rid], p2d[rid], sigma2[rid], K, Rs, ts)                  # (H, nv)
        with np.errstate(invalid="ignore"):
            lo, hi = (d2 <= chi2 * (1.0 - BAND)).sum(1), (d2 <= chi2 * (1.0 + BAND)).sum(1)
            und = (d2 <= chi2 * (1.0 + BAND)) & ~(d2 <= chi2 * (1.0 - BAND))
        stats["pairs"] += d2.size
        stats["undecided"] += int(und.sum())
        c = counts[posed]
        bad = np.nonzero((c < lo) | (c > hi))[0]
        if len(bad):
            raise StageError("B", crop, int(posed[bad[0]]), "count %d, but %d..%d ranked points pass the whitened gate under the recorded pose"
                             % (c[bad[0]], lo[bad[0]], hi[bad[0]]))

    # ---- C: selection
    if inliers.shape != (N,) or (inliers & ~ranked).any():
        raise StageError("C", crop, None, "inliers outside the ranked set: %r" % (np.nonzero(inliers & ~ranked)[0][:8].tolist(),))
    if not need or counts.max() < 5:
        identity_expected("C", "no hypothesis with 5 inliers")
        return stats
    win = int(np.argmax(counts))
    if status != 1:
        raise StageError("C", crop, win, "status %d with a winner of %d inliers" % (status, counts[win]))
    w = int(np.nonzero(posed == win)[0][0])
    with np.errstate(invalid="ignore"):
        sure_in, sure_out = d2[w] <= chi2 * (1.0 - BAND), ~(d2[w] <= chi2 * (1.0 + BAND))
    got = inliers[rid]
    if (sure_in & ~got).any() or (sure_out & got).any():
        diff = rid[(sure_in & ~got) | (sure_out & got)]
        raise StageError("C", crop, win, "the returned mask (%d) is not the winner's inlier set (%d): differs at %r"
                         % (got.sum(), sure_in.sum(), diff[:8].tolist()))

    # ---- D: the refit over the device's inlier list
    sel = np.nonzero(inliers)[0]
    fits = [rt for rt in (_oracle_epnp(p3d[sel], p2d[sel], K, None, sg) for sg in S.AXIS_SIGNS) if rt is not None]
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
        n_true = int((ranked & ~out).sum())
        mR, mt = S.e_margins()
        for h in range(need):
            s = sample(want, seed, crop, h, pools[h])
            if out[s].any():
                continue
            stats["all_inlier"] += 1
            if counts[h] != n_true:
                raise StageError("E", crop, h, "all-inlier sample %r counts %d, the crop has %d ranked non-outliers" % (s.tolist(), counts[h], n_true))
            dR = np.abs(records[h, 2:11].reshape(3, 3) - Rt).max()
            dt = np.linalg.norm(records[h, 11:14] - tt) / np.linalg.norm(tt)
            if not (dR <= mR and dt <= mt):
                raise StageError("E", crop, h, "all-inlier sample %r: pose off the true one by |dR| = %.3e (margin %.3e), |dt|/|t| = %.3e (%.3e)"
                                 % (s.tolist(), dR, mR, dt, mt))
    return stats


# ------------------------------------------------------------------------------------------------------------- the committed cases
SIGMA_IN, SIGMA_OUT = (0.25, 4.0), (9.0, 36.0)      # pixels^2 per axis: what looks like an inlier / the large variance of a flagged outlier


def variances(rng, out, informative):
    """(n,2) variances: an outlier gets the large variance with probability `informative`; everything else looks like an inlier.  With
    outliers 20..80 px off per axis (pnp_stages._crop) a flagged outlier's whitened residual is at least 2 * 400 / 36 = 22 > 9.21, an
    unflagged one's at least 200; a noise-free inlier's is ~1e-9: stage E's counts are exact at either quantile."""
    n = len(out)
    s2 = rng.uniform(*SIGMA_IN, size=(n, 2))
    big = out & (rng.random(n) < informative)
    s2[big] = rng.uniform(*SIGMA_OUT, size=(int(big.sum()), 2))
    return s2


class Case(S.Case):
    """pnp_stages.Case plus sigma2 (B,N,2) f64, chi2 and guided"""

    def __init__(self, name, p3d, p2d, valid, sigma2, chi2=9.21, guided=True, **kw):
        super().__init__(name, p3d, p2d, valid, **kw)
        self.sigma2, self.chi2, self.guided = np.asarray(sigma2, np.float64), float(chi2), bool(guided)


def _make(name, seed, B, N, outlier_frac=0.3, informative=0.8, noise=0.0, valid_frac=0.9, model=None, K=S.K_LMO, column=0, sigma2=None,
          nv=None, **kw):
    rng = np.random.default_rng(seed)
    xyz = S.lmo_model(N) if model is None else model
    shares = outlier_frac if isinstance(outlier_frac, tuple) else (outlier_frac,)
    crops = [S._crop(rng, xyz[b] if xyz.ndim == 3 else xyz, K[b] if K.ndim == 3 else K, shares[b % len(shares)], noise, valid_frac)
             for b in range(B)]
    valid = np.zeros((B, N, 3), np.uint8)
    for c in range(3):                                       # three different masks with real content; the case's column is the crop's own
        valid[:, :, c] = rng.random((B, N)) < 0.5
    valid[:, :, column] = np.stack([c[1] for c in crops])
    if nv is not None:                                       # exactly nv valid points per crop, spread over the keypoints
        valid[:, :, column] = 0
        for b in range(B):
            valid[b, rng.choice(N, nv, replace=False), column] = 1
    s2 = np.stack([variances(rng, c[2][2], informative) for c in crops]) if sigma2 is None else sigma2(rng, B, N)
    return Case(name, xyz, np.stack([c[0] for c in crops]), valid, s2, K=K, column=column, seed=seed,
                truth=[None if noise else c[2] for c in crops], **kw)


def _bad_variances(rng, B, N):
    """every kind of bad variance, each on ONE axis only, on a fifth of the points; the rest as inliers look"""
    s2 = rng.uniform(*SIGMA_IN, size=(B, N, 2))
    kinds = (np.nan, np.inf, 0.0, -1.0, -np.inf, -0.0)
    for b in range(B):
        for j, i in enumerate(rng.choice(N, N // 5, replace=False)):
            s2[b, i, j % 2] = kinds[j % len(kinds)]
    return s2


def _edge(kind):
    e = S._edge(kind)
    rng = np.random.default_rng(51)
    return Case("edge_" + kind, e.p3d, e.p2d, e.valid, rng.uniform(*SIGMA_IN, size=(e.B, e.N, 2)), seed=50, iterations=64)


CASES = {}
for _n in (6, 7, 64, 65, 255, 256, 257, 512):
    CASES["shape_1x%d" % _n] = lambda _n=_n: _make("shape_1x%d" % _n, 100 + _n, 1, _n, 0.0 if _n < 64 else 0.3, valid_frac=1.0 if _n < 64 else 0.9,
                                                    iterations=70)
CASES["shape_3x64"] = lambda: _make("shape_3x64", 201, 3, 64, 0.3, iterations=70)
CASES["shape_3x257"] = lambda: _make("shape_3x257", 202, 3, 257, 0.5, iterations=70)
CASES["per_crop_K_p3d"] = lambda: _make("per_crop_K_p3d", 203, 3, 512, 0.3, model=S._lm_models()[:, :512], K=S._per_crop_K(3), iterations=70)
CASES["noisy_3x256"] = lambda: _make("noisy_3x256", 204, 3, 256, 0.4, noise=0.5, iterations=70, chi2=5.99)
for _it in S.ITERATIONS:     # crops alternate between 30 % outliers (the rule stops after one round) and 70 % (it never stops)
    CASES["iterations_%d" % _it] = lambda _it=_it: _make("iterations_%d" % _it, 260, 2, 256, (0.3, 0.7), iterations=_it)
for _nv in (0, 3, 4, 5, 6):
    CASES["nv_%d" % _nv] = lambda _nv=_nv: _make("nv_%d" % _nv, 300 + _nv, 3 if _nv == 4 else 1, 64, 0.0, nv=_nv, iterations=20)
CASES["ties_all"] = lambda: _make("ties_all", 310, 1, 65, 0.3, sigma2=lambda rng, B, N: np.full((B, N, 2), 2.0), iterations=70)
CASES["ties_blocks"] = lambda: _make("ties_blocks", 311, 3, 256, 0.3, iterations=70,
                                     sigma2=lambda rng, B, N: np.repeat(rng.integers(1, 5, size=(B, N, 1)) * 0.5, 2, 2))
CASES["bad_variances"] = lambda: _make("bad_variances", 312, 3, 65, 0.2, sigma2=_bad_variances, iterations=70)
for _c in range(3):
    CASES["column_%d" % _c] = lambda _c=_c: _make("column_%d" % _c, 320, 1, 257, 0.3, column=_c, iterations=70)
CASES["unguided_1x256"] = lambda: _make("unguided_1x256", 330, 1, 256, 0.5, guided=False, iterations=150)
CASES["unguided_3x65"] = lambda: _make("unguided_3x65", 331, 3, 65, 0.3, guided=False, iterations=70)
CASES["guided_hard"] = lambda: _make("guided_hard", 332, 1, 256, 0.7, iterations=150)
for _k in S.EDGES:
    CASES["edge_" + _k] = lambda _k=_k: _edge(_k)


def restated_outputs(case):
    """the restatement's own run of a case in the device's output layout: dict(records (B,it,14), R (B,3,3), t (B,3), inliers (B,N),
    status (B,), order (B,N), n_ranked (B,), n_dropped (B,))"""
    B, N, it = case.B, case.N, case.iterations
    o = dict(records=np.full((B, it, HYP), np.nan), R=np.zeros((B, 3, 3)), t=np.zeros((B, 3)), inliers=np.zeros((B, N), bool),
             status=np.zeros(B, np.int32), order=np.zeros((B, N), np.int32), n_ranked=np.zeros(B, np.int32), n_dropped=np.zeros(B, np.int32))
    for b in range(B):
        p3, p2, va, K = case.crop(b)
        o["order"][b], o["n_ranked"][b], o["n_dropped"][b] = rank(case.sigma2[b], va)
        o["records"][b] = hypothesis_records(p3, p2, va, case.sigma2[b], K, case.chi2, it, case.seed, b, case.guided)
        o["R"][b], o["t"][b], o["inliers"][b], o["status"][b] = solve(p3, p2, va, case.sigma2[b], K, case.chi2, it, case.seed, b, case.guided,
                                                                      records=o["records"][b])
    return o


@functools.lru_cache(maxsize=None)
def cached(name):
    case = CASES[name]()
    return case, restated_outputs(case)


def check_case(case, o, log=None):
    """check_crop on every crop of a case + the undecided cap.  o: a dict as restated_outputs returns.  -> summed statistics"""
    total = {}
    for b in range(case.B):
        p3, p2, va, K = case.crop(b)
        st = check_crop(p3, p2, va, case.sigma2[b], K, case.chi2, case.iterations, case.seed, b, case.guided, o["records"][b], o["R"][b],
                        np.asarray(o["t"][b]).reshape(3), o["inliers"][b], int(o["status"][b]), o["order"][b], int(o["n_ranked"][b]),
                        int(o["n_dropped"][b]), truth=case.truth[b])
        for k, v in st.items():
            total[k] = max(total.get(k, 0), v) if k == "refit_1e15" else total.get(k, 0) + v
    total["status1"] = int(np.asarray(o["status"]).sum())
    if log is not None:
        log("%-18s %s" % (case.name, " ".join("%s=%d" % kv for kv in sorted(total.items()))))
    assert total["undecided"] <= UNDECIDED_CAP * total["pairs"], (case.name, total)
    return total


# ------------------------------------------------------------------------------------------------------------------ tamperings
def _copy(o):
    return {k: np.array(v, copy=True) for k, v in o.items()}


def _winner(o, b):
    c = np.where(np.isnan(o["records"][b, :, 0]), -1, o["records"][b, :, 0])
    return int(np.argmax(c)), c


def t_order_swap(case, o):
    o = _copy(o)
    o["order"][0, [1, 2]] = o["order"][0, [2, 1]]
    return o


def t_tie_wrong(case, o):
    """two neighbours of the ranking with EQUAL keys exchanged: descending index inside the tie"""
    o = _copy(o)
    key = case.sigma2[0].sum(1)
    od = o["order"][0]
    j = next(j for j in range(int(o["n_ranked"][0]) - 1) if key[od[j]] == key[od[j + 1]])
    od[[j, j + 1]] = od[[j + 1, j]]
    return o


def t_pool_off_by_one(case, o):
    o = _copy(o)
    o["records"][0, 3, 1] += 1
    return o


def t_count_off_by_one(case, o):
    o = _copy(o)
    win, c = _winner(o, 0)
    h = next(h for h in range(len(c)) if c[h] >= 0 and h != win and c[h] + 1 < c[win])      # (the winner stays the winner)
    o["records"][0, h, 0] += 1
    return o


def t_second_best_winner(case, o):
    """mask and pose of the best record with FEWER inliers than the winner"""
    o = _copy(o)
    p3, p2, va, K = case.crop(0)
    win, c = _winner(o, 0)
    h = int(np.argmax(np.where(c < c[win], c, -2)))
    rid = np.sort(o["order"][0, :int(o["n_ranked"][0])])
    d2 = whitened(p3[rid], p2[rid], case.sigma2[0][rid], K, o["records"][0, h, 2:11].reshape(1, 3, 3), o["records"][0, h, 11:14][None])[0]
    sel = rid[d2 <= case.chi2]
    o["inliers"][0] = False
    o["inliers"][0, sel] = True
    o["R"][0], o["t"][0] = _oracle_epnp(p3[sel], p2[sel], K)
    return o


def t_mask_bit_flipped(case, o):
    o = _copy(o)
    i = int(np.nonzero(o["inliers"][0])[0][0])
    o["inliers"][0, i] = False
    return o


def t_refit_wrong_list(case, o):
    """the pose refitted over the inlier list without its last three members"""
    o = _copy(o)
    p3, p2, va, K = case.crop(0)
    sel = np.nonzero(o["inliers"][0])[0][:-3]
    o["R"][0], o["t"][0] = _oracle_epnp(p3[sel], p2[sel], K)
    return o


# name -> (case, the stage that must catch it, the tampering)
TAMPERINGS = {
    "order_swap": ("noisy_3x256", "R", t_order_swap),
    "tie_wrong": ("ties_blocks", "R", t_tie_wrong),
    "pool_off_by_one": ("noisy_3x256", "P", t_pool_off_by_one),
    "count_off_by_one": ("noisy_3x256", "B", t_count_off_by_one),
    "second_best_winner": ("noisy_3x256", "C", t_second_best_winner),
    "mask_bit_flipped": ("noisy_3x256", "C", t_mask_bit_flipped),
    "refit_wrong_list": ("noisy_3x256", "D", t_refit_wrong_list),
}


# ------------------------------------------------------------------------------------------- the sample-composition set-up
def probe_crop(seed, nv, outlier_share, informative):
    """one crop of the probe: (outlier flags (nv,), sigma2 (nv,2)) -- outliers get the large variance with probability `informative`"""
    rng = np.random.default_rng(seed)
    out = rng.random(nv) < outlier_share
    return out, variances(rng, out, informative)


def first_all_inlier(out, order, nv, iterations, seed, crop, guided):
    """(the first hypothesis whose sample has no outlier, or `iterations` if none; how many of the `iterations` have none)"""
    first, n = iterations, 0
    for h in range(iterations):
        if not out[sample(order, seed, crop, h, pool_size(h, nv, iterations, guided))].any():
            n += 1
            first = min(first, h)
    return first, n


if __name__ == "__main__":
    import sys
    import time
    for name in (sys.argv[1:] or CASES):
        t0 = time.time()
        case, o = cached(name)
        check_case(case, o, log=print)
        print("    (%.1f s)" % (time.time() - t0), flush=True)
