"""TEST INFRASTRUCTURE (not collected): cp_pnp_refine_lm (row N22) checked one iteration at a time by replaying the device's own records.

THE RULE (csrc/pnp_refine.hip states it; `refine` below is its numpy restatement).  Per crop: S = {k : mask[k] != 0}, n = |S|; model
points X_k and pixels p_k (fp32 values), fu, fv, uc, vc = K[0,0], K[1,1], K[0,2], K[1,2]; the input pose (R, t).  All in float64.
  residual    Y_k = R X_k, C_k = Y_k + t, r_k = (fu C_x / C_z + uc - p_x, fv C_y / C_z + vc - p_y), cost c = sum_k |r_k|^2
  increment   d = (w, v): R' = exp([w]x) R (Rodrigues), t' = t + v
  Jacobian    J_k = P_k [ -[Y_k]x | I ], P_k = [[fu / C_z, 0, -fu C_x / C_z^2], [0, fv / C_z, -fv C_y / C_z^2]]; H = sum J^T J, g = sum J^T r
  iteration   lambda = 1e-3; at most max_iters (1..64) times: solve (H + lambda diag H) d = -g by Cholesky; not positive definite ->
              the trial is rejected with c' = +inf (d, the trial pose and s are NaN); else c' at (R', t'), +inf if a selected point has
              C'_z <= 0 or c' is not finite; accept iff c' < c (the trial becomes the state, lambda = max(lambda / 10, 1e-12)), else
              lambda = 10 lambda; s = max(|w|_inf, |v|_inf / |t|) with t from before the step
  stopping    s <= step_tol (accepted or not): status 1; lambda > 1e8 after a rejection: 3; iterations run out: 2
  pass-through (status 0, the pose returned is bitwise the input): status_in == 0, n < 6, a non-finite input pose or selected pixel,
              a selected point with C_z <= 0 under the input pose
  records     17 doubles per executed iteration: [lambda used, c, c', accepted 0/1, s, R' (9), t' (3)]; NaN elsewhere
  returned    bitwise the last accepted trial pose, or the input pose

`check_crop` replays the records of one crop and raises pnp_stages.StageError (stage, crop, iteration in the message):
  P  pass-through     expected exactly where the rule says; then pose bitwise, no records, info = [NaN, NaN, n, 0, NaN ...]
  L  lambda           reproduced EXACTLY from the accept flags (one IEEE division or multiplication per iteration)
  C  cost             c and c' equal numpy's cost at the replayed state / the recorded trial pose to a relative COST_RTOL = 1e-9: a sum of at
                      most 4096 positive fp64 terms carries a relative error of order 1e-12, which leaves the three orders pnp_stages.BAND
                      leaves; c' = +inf exactly where numpy finds a point not in front, a non-finite cost or no Cholesky factor
  T  trial pose       numpy's trial from the replayed state and the recorded lambda within TAU_R (|dR|_max), TAU_T (|dt| / |t|); s within
                      max(TAU_R, TAU_T)
  A  accept flag      accepted == (c' < c) on the device's own two numbers
  S  state            c of an iteration is bitwise the c' of the last accepted one before it (c of the input pose before any)
  E  stop and status  follow from the device's own s, lambda and iteration count; nothing recorded after the stop, nothing missing before
  R  returned pose    bitwise the last accepted trial (or the input pose)
  I  info             cost0 / cost are the records' first c / last accepted c' bitwise, n, iterations; H equals numpy's at the returned pose
                      to a relative COST_RTOL of sqrt(H_ii H_jj)
  K  known answer     (noise-free crops that stopped by the step rule) the returned pose lies within E_MARGIN of the true one

Measured constants, all on the reference side, on a CPU (`python -m tests.lm_stages` prints them; tests/test_lm_refine.py re-derives
and asserts them on every run):
  TAU_R, TAU_T   16 x the largest difference, over every executed iteration of every committed case, between two versions of the
                 restatement's trial pose from the same state and lambda: one with numpy's (pairwise) sums of the 28 per-point terms,
                 one with the kernel's order (thread i takes points i, i + 256, ... in ascending order; a shuffle tree 32, 16, .. 1 inside
                 each wave of 64; wave 0 + 1 + 2 + 3) -- capped at pnp_stages.TAU_CAP.  MEASURED_TAU holds the largest differences seen.
  E_MARGIN       8 x the restatement's own worst deviation from the true pose on the noise-free cases that stop by the step rule (the
                 pixels' fp32 rounding is their noise).  MEASURED_E holds that worst deviation.
  SCIPY_MARGIN   (tests/test_lm_refine.py) 8 x the largest difference measured between the restatement's final pose and
                 scipy.optimize.least_squares' from the same start.  MEASURED_SCIPY holds the difference seen.
"""
import math
import sys

import numpy as np

from oracle import pnp_oracle as P
from tests import pnp_stages as S
from tests.pnp_stages import StageError

REC, INFO, MAX_ITERS, THREADS = 17, 40, 64, 256
LAMBDA0, LAMBDA_MIN, LAMBDA_STOP = 1e-3, 1e-12, 1e8
COST_RTOL = 1e-9
# (|dR|_max, |dt| / |t|): printed by `python -m tests.lm_stages`, asserted (as upper bounds that a quarter of them would miss) in
# tests/test_lm_refine.py::test_measured_constants
MEASURED_TAU = (4.4e-15, 3.0e-14)             # seen: 4.385e-15, 2.940e-14, both on exact_3x256 -> TAU_R = 7.0e-14, TAU_T = 4.8e-13
MEASURED_E = (3.7e-07, 1.5e-07)               # seen: 3.684e-07, 1.461e-07, both on exact_3x7: the pixels' fp32 rounding on seven points
MEASURED_SCIPY = (6.3e-11, 3.8e-10)           # seen: 6.282e-11 (noisy_3x512), 3.773e-10: scipy's 'trf' with 3-point differences


def taus():
    return min(16 * MEASURED_TAU[0], S.TAU_CAP[0]), min(16 * MEASURED_TAU[1], S.TAU_CAP[1])


def e_margins():
    return 8 * MEASURED_E[0], 8 * MEASURED_E[1]


def scipy_margins():
    return 8 * MEASURED_SCIPY[0], 8 * MEASURED_SCIPY[1]


# ------------------------------------------------------------------------------------------------------------- the restatement
def jacobian(X, p, K, R, t):
    """-> (J0, J1: the two rows of every J_k as lists of six (n,) arrays, r0, r1 (n,), C_z (n,)), in the kernel's operation order
    (numpy's element-wise arithmetic is IEEE, uncontracted)"""
    fu, fv, uc, vc = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    X0, X1, X2 = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(all="ignore"):
        Y0 = R[0, 0] * X0 + R[0, 1] * X1 + R[0, 2] * X2
        Y1 = R[1, 0] * X0 + R[1, 1] * X1 + R[1, 2] * X2
        Y2 = R[2, 0] * X0 + R[2, 1] * X1 + R[2, 2] * X2
        C0, C1, C2 = Y0 + t[0], Y1 + t[1], Y2 + t[2]
        iz = 1.0 / C2
        r0, r1 = fu * C0 * iz + uc - p[:, 0], fv * C1 * iz + vc - p[:, 1]
        a, b = fu * iz, fv * iz
        pu, pv = -(a * C0 * iz), -(b * C1 * iz)
        z = np.zeros_like(a)
        J0 = [pu * Y1, a * Y2 - pu * Y0, -(a * Y1), a, z, pu]
        J1 = [pv * Y1 - b * Y2, -(pv * Y0), b * Y0, z, b, pv]
    return J0, J1, r0, r1, C2


def point_terms(X, p, K, R, t):
    """-> (T (n, 28): per point the 21 upper-triangle entries of J^T J row by row, the 6 of J^T r, |r|^2; front (n,) bool: C_z > 0)"""
    J0, J1, r0, r1, C2 = jacobian(X, p, K, R, t)
    with np.errstate(all="ignore"):
        cols = [J0[i] * J0[j] + J1[i] * J1[j] for i in range(6) for j in range(i, 6)]
        cols += [J0[i] * r0 + J1[i] * r1 for i in range(6)]
        cols.append(r0 * r0 + r1 * r1)
    return np.stack(cols, 1), C2 > 0.0


def numpy_sum(T):
    return T.sum(0)


def kernel_sum(T):
    """the kernel's summation order: thread i adds its points i, i + 256, ... in ascending order to 0; block_sum: a shuffle tree inside
    each wave (x[l] += x[l + o], o = 32, 16, .. 1), then wave 0 + wave 1 + wave 2 + wave 3"""
    part = np.zeros((THREADS, T.shape[1]))
    for j in range(0, len(T), THREADS):
        blk = T[j:j + THREADS]
        part[:len(blk)] = part[:len(blk)] + blk
    x = part.reshape(THREADS // 64, 64, -1).copy()
    o = 32
    while o:
        x[:, :o] = x[:, :o] + x[:, o:2 * o]
        o //= 2
    w = x[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def unpack_H(sums):
    H = np.zeros((6, 6))
    e = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = sums[e]
            e += 1
    return H


def load_lower(sums):
    """csrc/pnp_core.h:lm_load_lower: the 21 upper-triangle sums -> the lower triangle of H as 6 x 6 Python floats"""
    L = [[0.0] * 6 for _ in range(6)]
    e = 0
    for p_ in range(6):
        for q in range(p_, 6):
            L[q][p_] = float(sums[e])
            e += 1
    return L


def solve_step(L, g, R, t):
    """csrc/pnp_core.h:lm_solve_step in Python floats, from the damped lower triangle L (destroyed) and g (6): Cholesky, the two solves,
    Rodrigues -> (pd, d (6), R' (3,3), t' (3), s); NaN everywhere when there is no Cholesky factor"""
    nan = float("nan")
    pd = True
    for j in range(6):
        s = L[j][j]
        for k in range(j):
            s -= L[j][k] * L[j][k]
        if not (s > 0.0) or not math.isfinite(s):
            pd = False
            break
        ljj = math.sqrt(s)
        L[j][j] = ljj
        for i in range(j + 1, 6):
            v = L[i][j]
            for k in range(j):
                v -= L[i][k] * L[j][k]
            L[i][j] = v / ljj
    d = [nan] * 6
    if pd:
        y = [0.0] * 6
        for i in range(6):
            v = -float(g[i])
            for k in range(i):
                v -= L[i][k] * y[k]
            y[i] = v / L[i][i]
        for i in range(5, -1, -1):
            v = y[i]
            for k in range(i + 1, 6):
                v -= L[k][i] * d[k]
            d[i] = v / L[i][i]
        pd = all(math.isfinite(x) for x in d)
    if not pd:
        return False, np.full(6, nan), np.full((3, 3), nan), np.full(3, nan), nan
    th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    if th2 < 1e-16:
        ca, cb = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        th = math.sqrt(th2)
        sh = math.sin(0.5 * th)
        ca, cb = math.sin(th) / th, 2.0 * sh * sh / th2
    W = [[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]]
    E = [[(1.0 if i == j else 0.0) + ca * W[i][j] + cb * (W[i][0] * W[0][j] + W[i][1] * W[1][j] + W[i][2] * W[2][j]) for j in range(3)] for i in range(3)]
    Rn = np.array([[E[i][0] * float(R[0, j]) + E[i][1] * float(R[1, j]) + E[i][2] * float(R[2, j]) for j in range(3)] for i in range(3)])
    tn = np.array([float(t[i]) + d[3 + i] for i in range(3)])
    t0, t1, t2 = float(t[0]), float(t[1]), float(t[2])
    tnorm = math.sqrt(t0 * t0 + t1 * t1 + t2 * t2)
    sw = max(abs(d[0]), abs(d[1]), abs(d[2]))
    with np.errstate(all="ignore"):
        sv = float(np.float64(max(abs(d[3]), abs(d[4]), abs(d[5]))) / np.float64(tnorm))
    s = sv if (sv > sw or sv != sv) else sw
    return True, np.array(d), Rn, tn, s


def trial(sums, R, t, lam):
    """the trial step of csrc/pnp_refine.hip: H + lambda diag H on its own diagonal, then solve_step"""
    L = load_lower(sums)
    for p_ in range(6):
        L[p_][p_] = L[p_][p_] + lam * L[p_][p_]
    return solve_step(L, sums[21:27], R, t)


def evaluate(X, p, K, R, t, sums=numpy_sum):
    """-> (the 28 sums, cost as the rule sees it: +inf with a point not in front or a non-finite sum)"""
    T, front = point_terms(X, p, K, R, t)
    with np.errstate(all="ignore"):
        sm = sums(T)
    c = float(sm[27]) if front.all() and np.isfinite(sm[27]) else float("inf")
    return sm, c


def passes_through(X, p, K, R, t, status_in):
    if status_in == 0 or len(X) < 6 or not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(p).all()):
        return True
    return not point_terms(X, p, K, R, t)[1].all()


def refine(p3d, p2d, mask, K, R, t, status_in=1, max_iters=20, step_tol=1e-10, sums=numpy_sum):
    """the rule on one crop -> dict(R, t, status, info (40,), records (max_iters, 17)) in the device's output layout"""
    sel = np.nonzero(np.asarray(mask))[0]
    X, p = np.asarray(p3d, np.float64)[sel], np.asarray(p2d, np.float64)[sel]
    K, R, t = np.asarray(K, np.float64), np.array(R, np.float64), np.array(t, np.float64).reshape(3)
    rec = np.full((max_iters, REC), np.nan)
    info = np.full(INFO, np.nan)
    info[2], info[3] = len(sel), 0
    if passes_through(X, p, K, R, t, status_in):
        return dict(R=R, t=t, status=0, info=info, records=rec)
    T, _ = point_terms(X, p, K, R, t)
    state = sums(T)
    c = c0 = float(state[27])
    lam, status, iters = LAMBDA0, 2, 0
    for it in range(max_iters):
        pd, d, Rn, tn, s = trial(state, R, t, lam)
        cn, new = float("inf"), None
        if pd:
            new, cn = evaluate(X, p, K, Rn, tn, sums)
        accept = cn < c
        rec[it, :5] = lam, c, cn, 1.0 if accept else 0.0, s
        rec[it, 5:14], rec[it, 14:17] = Rn.reshape(9), tn
        if accept:
            R, t, state, c = Rn, tn, new, cn
            lam = max(lam / 10.0, LAMBDA_MIN)
        else:
            lam = lam * 10.0
        iters = it + 1
        if s <= step_tol:
            status = 1
            break
        if not accept and lam > LAMBDA_STOP:
            status = 3
            break
    info[0], info[1], info[3] = c0, c, iters
    info[4:] = unpack_H(state).reshape(36)
    return dict(R=R, t=t, status=status, info=info, records=rec)


# ------------------------------------------------------------------------------------------------------------- the checker
def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def check_crop(p3d, p2d, mask, K, R_in, t_in, status_in, max_iters, step_tol, crop, records, R_out, t_out, status, info, truth=None):
    """Raises StageError where the outputs of cp_pnp_refine_lm on one crop contradict its own records or the restatement.  p3d (N,3),
    p2d (N,2), mask (N,), K (3,3), R_in (3,3), t_in (3,): the values the device read; records (max_iters, 17), R_out, t_out, status,
    info (40,): what it returned.  truth = (R, t) switches stage K on.  -> statistics (iterations, accepted, worst trial differences)"""
    sel = np.nonzero(np.asarray(mask))[0]
    X, p = np.asarray(p3d, np.float64)[sel], np.asarray(p2d, np.float64)[sel]
    K, R_in, t_in = np.asarray(K, np.float64), np.asarray(R_in, np.float64), np.asarray(t_in, np.float64).reshape(3)
    records, R_out, t_out, info = np.asarray(records, np.float64), np.asarray(R_out, np.float64), np.asarray(t_out, np.float64).reshape(3), np.asarray(info, np.float64)
    status = int(status)
    stats = dict(iters=0, accepted=0, dR_1e18=0, dt_1e18=0, passed=0)
    if records.shape != (max_iters, REC) or info.shape != (INFO,):
        raise StageError("P", crop, None, "records / info have shapes %r / %r" % (records.shape, info.shape))
    bits = lambda a: np.asarray(a, np.float64).reshape(-1).view(np.uint64)                      # noqa: E731

    def same(a, b):
        return np.array_equal(bits(a), bits(b))
    # ---- P
    if passes_through(X, p, K, R_in, t_in, status_in):
        if status != 0:
            raise StageError("P", crop, None, "the rule passes this crop through (n = %d, status_in %r), got status %d" % (len(sel), status_in, status))
        if not (same(R_out, R_in) and same(t_out, t_in)):
            raise StageError("P", crop, None, "pass-through, but the returned pose is not bitwise the input pose")
        if not np.isnan(records).all():
            raise StageError("P", crop, None, "pass-through, but records were written")
        if not (info[2] == len(sel) and info[3] == 0 and np.isnan(info[:2]).all() and np.isnan(info[4:]).all()):
            raise StageError("P", crop, None, "pass-through: info is not [NaN, NaN, n, 0, NaN ...]: %r" % (info[:4].tolist(),))
        stats["passed"] = 1
        return stats
    if status == 0:
        raise StageError("P", crop, None, "status 0 on a crop the rule refines (n = %d)" % len(sel))
    tau_R, tau_t = taus()
    R, t = R_in, t_in
    state, c_np = evaluate(X, p, K, R, t)
    lam, c_dev, last = LAMBDA0, None, None
    want_status, iters = 2, 0
    for it in range(max_iters):
        rec = records[it]
        if np.isnan(rec).all():
            raise StageError("E", crop, it, "no record, but nothing recorded before stops the iteration")
        lam_d, c_d, cn_d, acc_d, s_d = rec[:5]
        Rn_d, tn_d = rec[5:14].reshape(3, 3), rec[14:17]
        # L
        if lam_d != lam:
            raise StageError("L", crop, it, "lambda %.17g, the flags give %.17g" % (lam_d, lam))
        # S, C: the state's cost
        if c_dev is not None and not same(c_d, c_dev):
            raise StageError("S", crop, it, "c = %.17g is not the last accepted c' (or the first c) = %.17g" % (c_d, c_dev))
        if not (np.isfinite(c_d) and _rel(c_d, float(state[27])) <= COST_RTOL):
            raise StageError("C", crop, it, "c = %.17g, numpy at the replayed state: %.17g" % (c_d, float(state[27])))
        c_dev = c_d
        # T
        pd, d, Rn, tn, s = trial(state, R, t, lam)
        if not pd:
            if not (np.isnan(rec[4:]).all() and cn_d == np.inf):
                raise StageError("T", crop, it, "numpy finds no Cholesky factor; the record holds a trial (c' = %r)" % cn_d)
        else:
            if not np.isfinite(rec[4:]).all():
                raise StageError("T", crop, it, "the trial pose or s is not finite, numpy's is")
            dR, dt = float(np.abs(Rn_d - Rn).max()), float(np.linalg.norm(tn_d - tn) / np.linalg.norm(t))
            stats["dR_1e18"], stats["dt_1e18"] = max(stats["dR_1e18"], int(1e18 * dR)), max(stats["dt_1e18"], int(1e18 * dt))
            if not (dR <= tau_R and dt <= tau_t):
                raise StageError("T", crop, it, "trial pose off numpy's: |dR| = %.3e (tau %.3e), |dt|/|t| = %.3e (tau %.3e)" % (dR, tau_R, dt, tau_t))
            if not abs(s_d - s) <= max(tau_R, tau_t):
                raise StageError("T", crop, it, "s = %.17g, numpy's %.17g" % (s_d, s))
            # C: the trial's cost, at the DEVICE's trial pose
            new, cn = evaluate(X, p, K, Rn_d, tn_d)
            if np.isinf(cn) != np.isinf(cn_d) or (np.isfinite(cn) and not _rel(cn_d, cn) <= COST_RTOL):
                raise StageError("C", crop, it, "c' = %.17g, numpy at the recorded trial pose: %.17g" % (cn_d, cn))
        # A
        if acc_d not in (0.0, 1.0) or bool(acc_d) != bool(cn_d < c_d):
            raise StageError("A", crop, it, "accepted = %r with c' = %.17g, c = %.17g" % (acc_d, cn_d, c_d))
        if acc_d:
            R, t, state, c_dev, last = Rn_d.copy(), tn_d.copy(), new, cn_d, (Rn_d.copy(), tn_d.copy())
            lam = max(lam / 10.0, LAMBDA_MIN)
            stats["accepted"] += 1
        else:
            lam = lam * 10.0
        iters = it + 1
        # E
        if s_d <= step_tol:
            want_status = 1
            break
        if not acc_d and lam > LAMBDA_STOP:
            want_status = 3
            break
    stats["iters"] = iters
    if not np.isnan(records[iters:]).all():
        raise StageError("E", crop, iters, "a record behind the stop (status %d after %d iterations by the device's own s and lambda)" % (want_status, iters))
    if status != want_status:
        raise StageError("E", crop, iters - 1, "status %d, the records end with %d" % (status, want_status))
    # R
    want = last if last is not None else (R_in, t_in)
    if not (same(R_out, want[0]) and same(t_out, want[1])):
        raise StageError("R", crop, None, "the returned pose is not bitwise the last accepted trial%s" % ("" if last is not None else " (none: the input pose)"))
    # I
    if not (same(info[0], records[0, 1]) and same(info[1], c_dev) and info[2] == len(sel) and info[3] == iters):
        raise StageError("I", crop, None, "info = %r, the records say cost0 %.17g, cost %.17g, n %d, %d iterations" % (info[:4].tolist(), records[0, 1], c_dev, len(sel), iters))
    H_d, H = info[4:].reshape(6, 6), unpack_H(state)
    scale = np.sqrt(np.outer(np.diag(H), np.diag(H)))
    if not (np.isfinite(H_d).all() and np.array_equal(H_d, H_d.T) and (np.abs(H_d - H) <= COST_RTOL * scale).all()):
        raise StageError("I", crop, None, "H off numpy's at the returned pose by %.3e of sqrt(H_ii H_jj)" % float(np.nanmax(np.abs(H_d - H) / scale)))
    # K
    if truth is not None and status == 1:
        mR, mt = e_margins()
        dR, dt = float(np.abs(R_out - truth[0]).max()), float(np.linalg.norm(t_out - truth[1]) / np.linalg.norm(truth[1]))
        if not (dR <= mR and dt <= mt):
            raise StageError("K", crop, None, "noise-free crop: off the true pose by |dR| = %.3e (margin %.3e), |dt|/|t| = %.3e (%.3e)" % (dR, mR, dt, mt))
    return stats


# ------------------------------------------------------------------------------------------------------------- the committed cases
class LmCase:
    """p3d (N,3) shared or (B,N,3); p2d (B,N,2); mask (B,N) uint8; K (3,3) shared or (B,3,3); R0 (B,3,3), t0 (B,3): the start poses,
    None for the noisy cases, whose start and mask are a RANSAC solver's output over `valid` (B,N,3) (`with_start`); status_in (B,)
    int32 or None; truth: per crop (R, t) or None"""

    def __init__(self, name, p3d, p2d, mask, K, R0=None, t0=None, status_in=None, max_iters=20, step_tol=1e-10, truth=None, valid=None, seed=0):
        self.name, self.p3d, self.p2d, self.K = name, p3d, p2d, K
        self.mask = None if mask is None else mask.astype(np.uint8)
        self.R0, self.t0, self.status_in, self.max_iters, self.step_tol = R0, t0, status_in, max_iters, step_tol
        self.B, self.N = p2d.shape[:2]
        self.truth = truth if truth is not None else [None] * self.B
        self.valid, self.seed = valid, seed

    def crop(self, b):
        return (self.p3d[b] if self.p3d.ndim == 3 else self.p3d, self.p2d[b], self.mask[b], self.K[b] if self.K.ndim == 3 else self.K)

    def with_start(self, R, t, inliers, status):
        """the noisy cases: start from a solver's poses over its inliers"""
        self.R0, self.t0 = np.asarray(R, np.float64).reshape(self.B, 3, 3), np.asarray(t, np.float64).reshape(self.B, 3)
        self.mask, self.status_in = np.asarray(inliers).astype(np.uint8), np.asarray(status).astype(np.int32)
        return self


def _rodrigues(axis, angle):
    a = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def _exact(name, seed, B, N, select=1.0, model=None, K=S.K_LMO, **kw):
    """noise-free crops without outliers, started 5 degrees and 5 % of |t| off the truth"""
    rng = np.random.default_rng(seed)
    xyz = S.lmo_model(N) if model is None else model
    p2d, mask, R0, t0, truth = [], [], [], [], []
    for b in range(B):
        uv, sel, (R, t, _) = S._crop(rng, xyz[b] if xyz.ndim == 3 else xyz, K[b] if K.ndim == 3 else K, 0.0, 0.0, select)
        if sel.sum() < 6:
            sel[:6] = True
        p2d.append(uv); mask.append(sel); truth.append((R, t))
        R0.append(_rodrigues(rng.normal(size=3), np.radians(5.0)) @ R)
        u = rng.normal(size=3)
        t0.append(t + 0.05 * np.linalg.norm(t) * u / np.linalg.norm(u))
    return LmCase(name, xyz, np.stack(p2d), np.stack(mask), K, np.stack(R0), np.stack(t0), truth=truth, seed=seed, **kw)


def _noisy(name, seed, B, N, model=None, K=S.K_LMO, **kw):
    """0.5 px noise, 30 % outliers, every keypoint valid: start and mask come from a RANSAC solver (`with_start`)"""
    rng = np.random.default_rng(seed)
    xyz = S.lmo_model(N) if model is None else model
    crops = [S._crop(rng, xyz[b] if xyz.ndim == 3 else xyz, K[b] if K.ndim == 3 else K, 0.3, 0.5, 1.0) for b in range(B)]
    valid = np.zeros((B, N, 3), np.uint8)
    valid[:, :, 0] = 1
    return LmCase(name, xyz, np.stack([c[0] for c in crops]), None, K, valid=valid, seed=seed, **kw)


def _passthrough():
    """crop 0 is refined (the control); 1: status 0 in; 2: five selected points; 3: NaN in R; 4: inf in t; 5: NaN in a selected pixel;
    6: NaN in a pixel that is NOT selected (refined)"""
    c = _exact("passthrough", 70, 7, 64, select=0.8)
    c.status_in = np.ones(7, np.int32)
    c.status_in[1] = 0
    c.mask[2, np.nonzero(c.mask[2])[0][5:]] = 0
    c.R0[3, 1, 2] = np.nan
    c.t0[4, 0] = np.inf
    c.p2d[5, np.nonzero(c.mask[5])[0][3], 1] = np.nan
    c.mask[6, 0] = 0
    c.p2d[6, 0, 0] = np.nan
    c.truth = [None] * 7
    return c


def _behind_camera():
    """pnp_stages' behind_camera edge (t_z small against the model radius), started AT its true poses: part of the model is behind"""
    rng = np.random.default_rng(50)
    N, B = 512, 2
    xyz = S.lmo_model(N)
    pose =[(S._pose(rng)[0], np.array([3.0, -2.0, 12.0 + 9.0 * b])) for b in range(B)]
    crops = [S._crop(rng, xyz, S.K_LMO, 0.2, 0.0, 1.0, pose[b]) for b in range(B)]
    p2d = np.nan_to_num(np.stack([c[0] for c in crops]), nan=0.0, posinf=1e6, neginf=-1e6).astype(np.float32).astype(np.float64)
    return LmCase("behind_camera", xyz, p2d, np.ones((B, N), np.uint8), S.K_LMO, np.stack([q[0] for q in pose]), np.stack([q[1] for q in pose]))


def _origin():
    """eight model points AT the origin: the rotation block of H is zero, no damping makes it positive definite -> every trial is
    rejected, lambda passes 1e8 after 12 iterations: status 3 (status 2 with max_iters below 12)"""
    t = np.array([10.0, -20.0, 700.0])
    xyz = np.zeros((8, 3))
    uv = (P.project(xyz, S.K_LMO, np.eye(3), t) + 0.25).astype(np.float32).astype(np.float64)
    return LmCase("origin", xyz, np.stack([uv, uv]), np.ones((2, 8), np.uint8), S.K_LMO, np.stack([np.eye(3)] * 2), np.stack([t, t + 1.0]))


def _with(case, **kw):
    for k, v in kw.items():
        setattr(case, k, v)
    return case


CASES = {
    "exact_3x6": lambda: _exact("exact_3x6", 61, 3, 6),
    "exact_3x7": lambda: _exact("exact_3x7", 62, 3, 7),
    "exact_1x255": lambda: _exact("exact_1x255", 63, 1, 255),
    "exact_3x256": lambda: _exact("exact_3x256", 64, 3, 256),
    "exact_1x257": lambda: _exact("exact_1x257", 65, 1, 257),
    "exact_33x512": lambda: _exact("exact_33x512", 66, 33, 512, select=0.8),
    "exact_3x4096_lm": lambda: _exact("exact_3x4096_lm", 67, 3, 4096, model=S._lm_models(), K=S._per_crop_K(3)),
    "exact_per_crop_K": lambda: _exact("exact_per_crop_K", 68, 3, 512, select=0.8, K=S._per_crop_K(3)),
    "exact_it1": lambda: _exact("exact_it1", 69, 3, 512, select=0.8, max_iters=1),
    "exact_it2": lambda: _exact("exact_it2", 69, 3, 512, select=0.8, max_iters=2),
    "exact_it64": lambda: _exact("exact_it64", 69, 3, 512, select=0.8, max_iters=64, step_tol=1e-300),
    "noisy_3x512": lambda: _noisy("noisy_3x512", 7, 3, 512),
    "noisy_it1": lambda: _noisy("noisy_it1", 7, 3, 512, max_iters=1),
    "noisy_it2": lambda: _noisy("noisy_it2", 7, 3, 512, max_iters=2),
    "noisy_it64": lambda: _noisy("noisy_it64", 7, 3, 512, max_iters=64),
    "noisy_1x4096": lambda: _noisy("noisy_1x4096", 8, 1, 4096, model=S._lm_models()[1]),
    "passthrough": _passthrough,
    "behind_camera": _behind_camera,
    "origin": _origin,
    "origin_it5": lambda: _with(_origin(), name="origin_it5", max_iters=5),
}
NOISY = tuple(k for k in CASES if k.startswith("noisy"))


def oracle_start(case, iterations=64):
    """the noisy cases on a CPU: start from oracle/pnp_oracle.solve_pnp_ransac (the device tests start from the device solver's output)"""
    out = [P.solve_pnp_ransac(*(case.p3d[b] if case.p3d.ndim == 3 else case.p3d, case.p2d[b], case.valid[b, :, 0].astype(bool),
                                case.K[b] if case.K.ndim == 3 else case.K), 2.0, iterations, case.seed, b) for b in range(case.B)]
    return case.with_start(np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]), [o[3] for o in out])


def make(name):
    case = CASES[name]()
    return oracle_start(case) if case.mask is None else case


def restatement_outputs(case, sums=numpy_sum):
    """the restatement's own run of a case in the device's output layout: (records (B,it,17), R (B,3,3), t (B,3), status (B,), info (B,40))"""
    outs = []
    for b in range(case.B):
        p3, p2, mk, K = case.crop(b)
        outs.append(refine(p3, p2, mk, K, case.R0[b], case.t0[b], 1 if case.status_in is None else int(case.status_in[b]), case.max_iters,
                           case.step_tol, sums))
    return (np.stack([o["records"] for o in outs]), np.stack([o["R"] for o in outs]), np.stack([o["t"] for o in outs]),
            np.array([o["status"] for o in outs], np.int32), np.stack([o["info"] for o in outs]))


def check_case(case, records, R, t, status, info, log=None):
    total = {}
    for b in range(case.B):
        p3, p2, mk, K = case.crop(b)
        st = check_crop(p3, p2, mk, K, case.R0[b], case.t0[b], 1 if case.status_in is None else int(case.status_in[b]), case.max_iters, case.step_tol,
                        b, records[b], R[b], np.asarray(t[b]).reshape(3), int(status[b]), info[b], truth=case.truth[b])
        for k, v in st.items():
            total[k] = max(total.get(k, 0), v) if k.endswith("_1e18") else total.get(k, 0) + v
    if log is not None:
        log("%-18s status %s %s" % (case.name, np.asarray(status).tolist()[:8], " ".join("%s=%d" % kv for kv in sorted(total.items()))))
    return total


def measure_tau(case, records):
    """largest (|dR|_max, |dt| / |t|) between the trial from numpy's sums and the trial from the kernel-order sums of the same terms, over
    every executed iteration of the restatement's run of a case"""
    worst = [0.0, 0.0]
    for b in range(case.B):
        p3, p2, mk, K = case.crop(b)
        sel = np.nonzero(mk)[0]
        X, p = np.asarray(p3, np.float64)[sel], np.asarray(p2, np.float64)[sel]
        R, t = case.R0[b], case.t0[b]
        for rec in records[b]:
            if np.isnan(rec[0]):
                break
            T, _ = point_terms(X, p, np.asarray(K, np.float64), R, t)
            a, k = trial(numpy_sum(T), R, t, rec[0]), trial(kernel_sum(T), R, t, rec[0])
            assert a[0] == k[0], (case.name, b)
            if a[0]:
                worst[0] = max(worst[0], float(np.abs(a[2] - k[2]).max()))
                worst[1] = max(worst[1], float(np.linalg.norm(a[3] - k[3]) / np.linalg.norm(t)))
            if rec[3]:
                R, t = rec[5:14].reshape(3, 3), rec[14:17]
    return worst


def measure_e(case, R, t, status):
    """the restatement's worst deviation from the true pose over a case's noise-free crops that stopped by the step rule"""
    worst = [0.0, 0.0]
    for b in range(case.B):
        if case.truth[b] is None or status[b] != 1:
            continue
        worst[0] = max(worst[0], float(np.abs(R[b] - case.truth[b][0]).max()))
        worst[1] = max(worst[1], float(np.linalg.norm(t[b] - case.truth[b][1]) / np.linalg.norm(case.truth[b][1])))
    return worst


def measure_all(names=None, log=None):
    tau, e = [0.0, 0.0], [0.0, 0.0]
    for name in (names or CASES):
        case = make(name)
        rec, R, t, status, info = restatement_outputs(case)
        a, b = measure_tau(case, rec), measure_e(case, R, t, status)
        tau, e = [max(x, y) for x, y in zip(tau, a)], [max(x, y) for x, y in zip(e, b)]
        if log is not None:
            log("%-18s tau %.3e %.3e   E %.3e %.3e   status %s iters %s" % (name, a[0], a[1], b[0], b[1], status.tolist()[:8], info[:8, 3].astype(int).tolist()))
    return tau, e


if __name__ == "__main__":
    tau, e = measure_all(sys.argv[1:], log=lambda s: print(s, flush=True))
    print("MEASURED_TAU = (%.3e, %.3e)\nMEASURED_E = (%.3e, %.3e)" % (tau[0], tau[1], e[0], e[1]))
