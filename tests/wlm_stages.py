"""TEST INFRASTRUCTURE (not collected): row N32 -- cp_code_confidence and cp_pnp_refine_wlm -- restated in numpy, the second checked one
iteration at a time by replaying the device's own records, as tests/lm_stages.py does for row N22 (its load_lower, solve_step,
kernel_sum and StageError are used here unchanged).

RULE 1, code_confidence (csrc/code_confidence.hip states it).  bits (B, rows, N) fp32: row 0 the RoI bit, rows 1..r the x bits MSB
first, rows 1+r..2r the y bits; bbox (B,4) int32 (x, y, w, h); grid (Hc, Wc); floor > 0 in cells^2.  All in float64, uncontracted.
  bit j (0 = MSB), logit z: e = exp(-|z|), q_j = e / ((1 + e)(1 + e)) = p (1 - p); +-inf -> 0, NaN -> NaN
  per axis: v = sum_j 4^(r-1-j) q_j, j ascending
  sigma2[b,n,0] = (w / Wc)^2 (floor + v_x), sigma2[b,n,1] = (h / Hc)^2 (floor + v_y); an empty box gives 0 (NaN with a NaN logit)
Tolerance CONF_RTOL = 64 * 2^-52 relative: each q_j carries two exp results good to an ulp and fewer than ten roundings, the sum at
most 30 more.

RULE 2, refine (csrc/pnp_refine_w.hip states it): row N22's rule (tests/lm_stages.py) with
  scale (N,2) fp32 = 1 / sigma per axis: u_{k,a} = scale_{k,a} r_{k,a}, Jacobian rows j_{k,a} = scale_{k,a} J_{k,a}, the scale applied
  before any product (a scale of exactly 1 changes no operand);
  Huber, delta > 0 (+inf allowed), per scalar component: rho(u) = u^2 if |u| <= delta else 2 delta |u| - delta^2, cost c = sum rho,
  omega = 1 if |u| <= delta else delta / |u|, H = sum (omega j) j^T, g = sum (omega j) u (half the gradient of c), accept iff c' < c on
  this cost;
  pass-through also where a selected point's scale is not finite or <= 0;
  info (42): row N22's 40 (H the whitened, omega-weighted matrix), then the number of components with |u| > delta at the input pose,
  then at the returned pose.

`check_crop` replays the records of one crop with stages P, L, C, T, A, S, E, R, I exactly as lm_stages.check_crop does (stage I also
checks the two counts, exactly: they are integers).  The Huber cases are committed under the condition that at every pose the
restatement evaluates, states and trials alike, min | |u| - delta | >= HUBER_GAP = 1e-6, so that device and numpy take the same branch
(tests/test_wlm.py asserts it).

TAMPERINGS, each caught by a named case (TAMPER_CASE; tests/test_wlm.py):
  scale_r_only    the scale applied to r but not to J                hetero_3x7
  omega_squared   omega squared                                      outlier_3x256
  huber_norm      Huber on the point norm instead of per component   outlier_1x255
  lt_at_delta     `<` for `<=` at delta                              at_delta (a CPU-only case: a component sits AT delta)
  accept_unrobust acceptance on the unrobust cost                    unrobust_accept
  swap_xy         x and y scales swapped                             hetero_1x257
  pow_j           4^j for 4^(r-1-j)                                  conf "msb_unsure"
  p_for_q         p in place of p (1 - p)                            conf "random"
  floor_outside   the floor outside the box scale                    conf "random"

Measured constants, on the reference side, on a CPU (`python -m tests.wlm_stages` prints them; tests/test_wlm.py re-derives them):
  TAU_R, TAU_T   16 x the largest difference over every executed iteration of every committed case between the restatement's trial
                 from numpy's sums and from the kernel-order sums (lm_stages.kernel_sum) of the same terms, capped at
                 pnp_stages.TAU_CAP.  MEASURED_TAU holds the largest differences seen.
  SCIPY_MARGIN   8 x the largest difference between the restatement's final pose and scipy.optimize.least_squares' (loss="huber",
                 f_scale=delta; "linear" for delta = +inf) on the whitened residuals from the same start.  MEASURED_SCIPY.
"""
import math
import sys

import numpy as np

from tests import lm_stages as L
from tests import pnp_stages as S
from tests.lm_stages import StageError, kernel_sum, load_lower, solve_step    # noqa: F401

REC, INFO, MAX_ITERS = 17, 42, 64
COST_RTOL = L.COST_RTOL                       # 1e-9: sums of at most 8192 non-negative fp64 terms, by lm_stages' argument
CONF_RTOL = 64 * 2.0 ** -52
HUBER_GAP = 1e-6
CELL_PX = 2.0                                 # the outliers' unit: a cell of a 128-px box on the 64-cell grid
MEASURED_TAU = (5.6e-16, 1.5e-15)             # seen: 5.551e-16, 1.459e-15, both on outlier_3x6 -> TAU_R = 9.0e-15, TAU_T = 2.4e-14
MEASURED_SCIPY = (3.7e-09, 6.8e-10)           # seen: 3.672e-09, 6.777e-10, both on hetero_3x512: scipy's 'trf' with 3-point differences
INF = float("inf")


def taus():
    return min(16 * MEASURED_TAU[0], S.TAU_CAP[0]), min(16 * MEASURED_TAU[1], S.TAU_CAP[1])


def scipy_margins():
    return 8 * MEASURED_SCIPY[0], 8 * MEASURED_SCIPY[1]


# ------------------------------------------------------------------------------------------------------------- rule 1
def code_variance(bits, r, tamper=None):
    """bits (B, rows, N) float32 -> (v_x, v_y) (B,N) float64: the codes' variances in cells^2"""
    z = np.asarray(bits, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(z))
        q = e / ((1.0 + e) * (1.0 + e))
        if tamper == "p_for_q":
            q = 1.0 / (1.0 + np.exp(-z))
        vx, vy = np.zeros(z[:, 0].shape), np.zeros(z[:, 0].shape)
        for j in range(r):
            w = float(4 ** (j if tamper == "pow_j" else r - 1 - j))
            vx = vx + w * q[:, 1 + j]
            vy = vy + w * q[:, 1 + r + j]
    return vx, vy


def code_confidence(bits, bbox, Hc, Wc, r, floor=1.0 / 12.0, tamper=None):
    """bits (B, rows, N) float32, bbox (B,4) int -> sigma2 (B,N,2) float64"""
    bbox = np.asarray(bbox)
    vx, vy = code_variance(bits, r, tamper)
    with np.errstate(all="ignore"):
        sx = (bbox[:, 2].astype(np.float64) / np.float64(Wc))[:, None]
        sy = (bbox[:, 3].astype(np.float64) / np.float64(Hc))[:, None]
        if tamper == "floor_outside":
            return np.stack([sx * sx * vx + floor, sy * sy * vy + floor], 2)
        return np.stack([sx * sx * (floor + vx), sy * sy * (floor + vy)], 2)


CONF_SIDES = ((1, 64), (64, 100), (100, 640), (640, 1), (0, 64), (64, 0))        # boxes of side 1, 64, 100 and 640, empty on either axis


def conf_inputs(B, N, r, rows, seed, shift=0):
    """the device cases' operands: logits random x 4, then (where there are 16 keypoints at least) one keypoint with every logit zero
    and one with every bit certain, then every special value (+-0, +-50, +-800, +-inf, NaN) planted LAST, so that nothing overwrites
    it -- at N = 1 they all meet in keypoint 0, on different rows as far as the 2 r code rows reach; crop b gets box
    CONF_SIDES[(b + shift) % 6]: the shifts 0, B, 2 B, .. below 6 give one (B, N, r) every box"""
    rng = np.random.default_rng(seed)
    bits = (4.0 * rng.normal(size=(B, rows, N))).astype(np.float32)
    special = [0.0, -0.0, 50.0, -50.0, 800.0, -800.0, np.inf, -np.inf, np.nan]
    for b in range(B):
        if N >= 16:
            bits[b, :, 5 + b] = 0.0                                              # a keypoint with every logit zero
            bits[b, :, 11 + b] = -np.inf                                         # ... and with every bit certain
        for i, s in enumerate(special):
            n = (7 * i + 3 * b) % N
            if N >= 16 and n in (5 + b, 11 + b):
                n = (n + 1) % N
            bits[b, 1 + (i + b) % (2 * r), n] = s
    bbox = np.array([[10 * b, 20 + b, CONF_SIDES[(b + shift) % 6][0], CONF_SIDES[(b + shift) % 6][1]] for b in range(B)], np.int32)
    return bits, bbox


CONF_CASES = {
    "random": lambda: conf_inputs(3, 65, 6, 13, 5, shift=5) + (6,),
    "msb_unsure": lambda: _msb_unsure(),
}


def _msb_unsure():
    bits = np.full((1, 13, 8), 9.0, np.float32)
    bits[0, 1, :] = 0.01                                                         # the x code's MSB undecided, everything else certain
    return bits, np.array([[0, 0, 128, 128]], np.int32), 6


# ------------------------------------------------------------------------------------------------------------- rule 2
def point_terms(X, p, sc, K, R, t, delta, tamper=None):
    """-> (T (n, 29): per point the 21 upper-triangle entries of H, the 6 of g, rho_0 + rho_1, the number of components beyond delta;
    front (n,) bool: C_z > 0; plain (n,): u_0^2 + u_1^2), in the kernel's operation order"""
    J0, J1, r0, r1, C2 = L.jacobian(X, p, K, R, t)
    s0, s1 = sc[:, 0], sc[:, 1]
    if tamper == "swap_xy":
        s0, s1 = s1, s0
    with np.errstate(all="ignore"):
        u0, u1 = s0 * r0, s1 * r1
        j0, j1 = [s0 * x for x in J0], [s1 * x for x in J1]
        if tamper == "scale_r_only":
            j0, j1 = J0, J1
        a0, a1 = np.abs(u0), np.abs(u1)
        if tamper == "huber_norm":
            a0 = a1 = np.sqrt(u0 * u0 + u1 * u1)
        k0, k1 = (a0 >= delta, a1 >= delta) if tamper == "lt_at_delta" else (a0 > delta, a1 > delta)
        w0, w1 = np.where(k0, delta / a0, 1.0), np.where(k1, delta / a1, 1.0)
        rho0, rho1 = np.where(k0, 2.0 * delta * a0 - delta * delta, u0 * u0), np.where(k1, 2.0 * delta * a1 - delta * delta, u1 * u1)
        if tamper == "huber_norm":
            rho0, rho1 = np.where(k0, 2.0 * delta * a0 - delta * delta, u0 * u0 + u1 * u1), np.zeros_like(u0)
        if tamper == "omega_squared":
            w0, w1 = w0 * w0, w1 * w1
        m0, m1 = [w0 * x for x in j0], [w1 * x for x in j1]
        cols = [m0[i] * j0[j] + m1[i] * j1[j] for i in range(6) for j in range(i, 6)]
        cols += [m0[i] * u0 + m1[i] * u1 for i in range(6)]
        cols.append(rho0 + rho1)
        cols.append(k0.astype(np.float64) + k1.astype(np.float64))
        plain = u0 * u0 + u1 * u1
    return np.stack(cols, 1), C2 > 0.0, plain


def numpy_sum(T):
    return T.sum(0)


def trial(sums, R, t, lam):
    """the trial step: H + lambda diag H on its own diagonal, then lm_stages.solve_step"""
    Lo = load_lower(sums)
    for q in range(6):
        Lo[q][q] = Lo[q][q] + lam * Lo[q][q]
    return solve_step(Lo, sums[21:27], R, t)


def evaluate(X, p, sc, K, R, t, delta, sums=numpy_sum, tamper=None, gaps=None):
    """-> (the 29 sums, the cost as the rule sees it: +inf with a point not in front or a non-finite sum, the unrobust cost)"""
    T, front, plain = point_terms(X, p, sc, K, R, t, delta, tamper)
    if gaps is not None and np.isfinite(delta):
        with np.errstate(all="ignore"):
            J0, J1, r0, r1, _ = L.jacobian(X, p, K, R, t)
            gaps.append(float(np.min(np.abs(np.abs(np.concatenate([sc[:, 0] * r0, sc[:, 1] * r1])) - delta))))
    with np.errstate(all="ignore"):
        sm = sums(T)
    ok = front.all() and np.isfinite(sm[27])
    return sm, (float(sm[27]) if ok else INF), (float(plain.sum()) if ok else INF)


def _select(p3d, p2d, mask, scale):
    sel = np.nonzero(np.asarray(mask))[0]
    return sel, np.asarray(p3d, np.float64)[sel], np.asarray(p2d, np.float64)[sel], np.asarray(scale, np.float32).astype(np.float64)[sel]


def passes_through(X, p, sc, K, R, t, status_in):
    if status_in == 0 or len(X) < 6 or not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(p).all()):
        return True
    if not (np.isfinite(sc).all() and (sc > 0.0).all()):
        return True
    return not L.point_terms(X, p, K, R, t)[1].all()


def refine(p3d, p2d, mask, scale, K, R, t, delta, status_in=1, max_iters=20, step_tol=1e-10, sums=numpy_sum, tamper=None, gaps=None):
    """the rule on one crop -> dict(R, t, status, info (42,), records (max_iters, 17)) in the device's output layout"""
    sel, X, p, sc = _select(p3d, p2d, mask, scale)
    K, R, t = np.asarray(K, np.float64), np.array(R, np.float64), np.array(t, np.float64).reshape(3)
    rec = np.full((max_iters, REC), np.nan)
    info = np.full(INFO, np.nan)
    info[2], info[3] = len(sel), 0
    if passes_through(X, p, sc, K, R, t, status_in):
        return dict(R=R, t=t, status=0, info=info, records=rec)
    state, _, plain = evaluate(X, p, sc, K, R, t, delta, sums, tamper, gaps)
    c = c0 = float(state[27])
    clip0 = float(state[28])
    lam, status, iters = L.LAMBDA0, 2, 0
    for it in range(max_iters):
        pd, d, Rn, tn, s = trial(state, R, t, lam)
        cn, new, plain_n = INF, None, INF
        if pd:
            new, cn, plain_n = evaluate(X, p, sc, K, Rn, tn, delta, sums, tamper, gaps)
        accept = (plain_n < plain) if tamper == "accept_unrobust" else (cn < c)
        rec[it, :5] = lam, c, cn, 1.0 if accept else 0.0, s
        rec[it, 5:14], rec[it, 14:17] = Rn.reshape(9), tn
        if accept:
            R, t, state, c, plain = Rn, tn, new, cn, plain_n
            lam = max(lam / 10.0, L.LAMBDA_MIN)
        else:
            lam = lam * 10.0
        iters = it + 1
        if s <= step_tol:
            status = 1
            break
        if not accept and lam > L.LAMBDA_STOP:
            status = 3
            break
    info[0], info[1], info[3] = c0, c, iters
    info[4:40] = L.unpack_H(state).reshape(36)
    info[40], info[41] = clip0, float(state[28])
    return dict(R=R, t=t, status=status, info=info, records=rec)


# ------------------------------------------------------------------------------------------------------------- the checker
def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def check_crop(p3d, p2d, mask, scale, K, R_in, t_in, delta, status_in, max_iters, step_tol, crop, records, R_out, t_out, status, info):
    """Raises StageError where the outputs of cp_pnp_refine_wlm on one crop contradict its own records or the restatement; the stages
    are lm_stages.check_crop's.  -> statistics (iterations, accepted, worst trial differences, pass-throughs)"""
    sel, X, p, sc = _select(p3d, p2d, mask, scale)
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
    if passes_through(X, p, sc, K, R_in, t_in, status_in):
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
    state, _, _ = evaluate(X, p, sc, K, R, t, delta)
    clip0 = float(state[28])
    lam, c_dev, last = L.LAMBDA0, None, None
    want_status, iters = 2, 0
    for it in range(max_iters):
        rec = records[it]
        if np.isnan(rec).all():
            raise StageError("E", crop, it, "no record, but nothing recorded before stops the iteration")
        lam_d, c_d, cn_d, acc_d, s_d = rec[:5]
        Rn_d, tn_d = rec[5:14].reshape(3, 3), rec[14:17]
        if lam_d != lam:
            raise StageError("L", crop, it, "lambda %.17g, the flags give %.17g" % (lam_d, lam))
        if c_dev is not None and not same(c_d, c_dev):
            raise StageError("S", crop, it, "c = %.17g is not the last accepted c' (or the first c) = %.17g" % (c_d, c_dev))
        if not (np.isfinite(c_d) and _rel(c_d, float(state[27])) <= COST_RTOL):
            raise StageError("C", crop, it, "c = %.17g, numpy at the replayed state: %.17g" % (c_d, float(state[27])))
        c_dev = c_d
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
            new, cn, _ = evaluate(X, p, sc, K, Rn_d, tn_d, delta)
            if np.isinf(cn) != np.isinf(cn_d) or (np.isfinite(cn) and not _rel(cn_d, cn) <= COST_RTOL):
                raise StageError("C", crop, it, "c' = %.17g, numpy at the recorded trial pose: %.17g" % (cn_d, cn))
        if acc_d not in (0.0, 1.0) or bool(acc_d) != bool(cn_d < c_d):
            raise StageError("A", crop, it, "accepted = %r with c' = %.17g, c = %.17g" % (acc_d, cn_d, c_d))
        if acc_d:
            R, t, state, c_dev, last = Rn_d.copy(), tn_d.copy(), new, cn_d, (Rn_d.copy(), tn_d.copy())
            lam = max(lam / 10.0, L.LAMBDA_MIN)
            stats["accepted"] += 1
        else:
            lam = lam * 10.0
        iters = it + 1
        if s_d <= step_tol:
            want_status = 1
            break
        if not acc_d and lam > L.LAMBDA_STOP:
            want_status = 3
            break
    stats["iters"] = iters
    if not np.isnan(records[iters:]).all():
        raise StageError("E", crop, iters, "a record behind the stop (status %d after %d iterations by the device's own s and lambda)" % (want_status, iters))
    if status != want_status:
        raise StageError("E", crop, iters - 1, "status %d, the records end with %d" % (status, want_status))
    want = last if last is not None else (R_in, t_in)
    if not (same(R_out, want[0]) and same(t_out, want[1])):
        raise StageError("R", crop, None, "the returned pose is not bitwise the last accepted trial%s" % ("" if last is not None else " (none: the input pose)"))
    if not (same(info[0], records[0, 1]) and same(info[1], c_dev) and info[2] == len(sel) and info[3] == iters):
        raise StageError("I", crop, None, "info = %r, the records say cost0 %.17g, cost %.17g, n %d, %d iterations" % (info[:4].tolist(), records[0, 1], c_dev, len(sel), iters))
    H_d, H = info[4:40].reshape(6, 6), L.unpack_H(state)
    scale_ = np.sqrt(np.outer(np.diag(H), np.diag(H)))
    if not (np.isfinite(H_d).all() and np.array_equal(H_d, H_d.T) and (np.abs(H_d - H) <= COST_RTOL * scale_).all()):
        raise StageError("I", crop, None, "H off numpy's at the returned pose by %.3e of sqrt(H_ii H_jj)" % float(np.nanmax(np.abs(H_d - H) / scale_)))
    if not (info[40] == clip0 and info[41] == float(state[28])):
        raise StageError("I", crop, None, "components beyond delta: %r at the input / returned pose, numpy counts %r" % (info[40:].tolist(), [clip0, float(state[28])]))
    return stats


# ------------------------------------------------------------------------------------------------------------- the committed cases
class WlmCase:
    """p3d (N,3) shared or (B,N,3); p2d (B,N,2); mask (B,N) uint8; scale (B,N,2) float32; K (3,3) shared or (B,3,3); R0 (B,3,3), t0 (B,3);
    delta; status_in (B,) int32 or None; inlier (B,N) bool: the points that are no gross outliers; truth: per crop (R, t)"""

    def __init__(self, name, p3d, p2d, mask, scale, K, R0, t0, delta, status_in=None, max_iters=20, step_tol=1e-10, inlier=None, truth=None):
        self.name, self.p3d, self.p2d, self.K = name, p3d, p2d, K
        self.mask, self.scale = mask.astype(np.uint8), np.asarray(scale, np.float32)
        self.R0, self.t0, self.delta, self.status_in, self.max_iters, self.step_tol = R0, t0, float(delta), status_in, max_iters, step_tol
        self.B, self.N = p2d.shape[:2]
        self.inlier = np.ones((self.B, self.N), bool) if inlier is None else inlier
        self.truth = truth

    def crop(self, b):
        return (self.p3d[b] if self.p3d.ndim == 3 else self.p3d, self.p2d[b], self.mask[b], self.scale[b], self.K[b] if self.K.ndim == 3 else self.K)

    def status(self, b):
        return 1 if self.status_in is None else int(self.status_in[b])


def _make(name, seed, B, N, kind, per_crop=False, select=1.0, start=(2.0, 0.02), delta=None, max_iters=20):
    """kind "unit": scales all 1, delta = +inf, 0.5 px noise; "hetero": per-point, per-axis sigma in [0.3, 3] px, the noise drawn with
    it, scale = 1 / sigma, delta = +inf; "outlier": hetero plus 10 % (at least one) gross outliers inside the mask, shifted by 8 to 32
    cells of CELL_PX pixels per axis, delta = 2.5.  per_crop: per-crop models and intrinsics.  The start is `start` = (degrees, fraction
    of |t|) off the truth."""
    rng = np.random.default_rng(seed)
    if per_crop:
        xyz, K = S._lm_models()[:B, :N], S._per_crop_K(B)
    else:
        xyz, K = S.lmo_model(N), S.K_LMO
    p2d, mask, scale, R0, t0, inl, truth = [], [], [], [], [], [], []
    for b in range(B):
        X, Kb = (xyz[b] if xyz.ndim == 3 else xyz), (K[b] if K.ndim == 3 else K)
        R, t = S._pose(rng)
        uv = S.P.project(X, Kb, R, t)
        sigma = np.full((N, 2), 0.5) if kind == "unit" else rng.uniform(0.3, 3.0, size=(N, 2))
        uv = uv + rng.normal(size=(N, 2)) * sigma
        sel = rng.random(N) < select
        if sel.sum() < 6:
            sel[:6] = True
        good = np.ones(N, bool)
        if kind == "outlier":
            idx = np.nonzero(sel)[0]
            out = rng.choice(idx, size=max(1, int(round(0.1 * len(idx)))), replace=False)
            uv[out] += CELL_PX * rng.uniform(8.0, 32.0, size=(len(out), 2)) * rng.choice([-1.0, 1.0], size=(len(out), 2))
            good[out] = False
        p2d.append(uv.astype(np.float32).astype(np.float64)); mask.append(sel); inl.append(good); truth.append((R, t))
        scale.append(np.ones((N, 2), np.float32) if kind == "unit" else (1.0 / sigma).astype(np.float32))
        R0.append(L._rodrigues(rng.normal(size=3), np.radians(start[0])) @ R)
        u = rng.normal(size=3)
        t0.append(t + start[1] * np.linalg.norm(t) * u / np.linalg.norm(u))
    if delta is None:
        delta = 2.5 if kind == "outlier" else INF
    return WlmCase(name, xyz, np.stack(p2d), np.stack(mask), np.stack(scale), K, np.stack(R0), np.stack(t0), delta, inlier=np.stack(inl), truth=truth,
                   max_iters=max_iters)


def _passthrough():
    """crop 0 is refined (the control); 1: status 0 in; 2: five selected points; 3: NaN in R; 4: inf in t; 5: NaN in a selected pixel;
    6: NaN in a pixel that is NOT selected (refined); 7: a selected scale of 0; 8: a negative one; 9: an infinite one; 10: NaN;
    11: a bad scale that is NOT selected (refined); 12: every point behind the camera"""
    c = _make("passthrough", 170, 13, 64, "outlier", select=0.8)
    c.status_in = np.ones(13, np.int32)
    c.status_in[1] = 0
    c.mask[2, np.nonzero(c.mask[2])[0][5:]] = 0
    c.R0[3, 1, 2] = np.nan
    c.t0[4, 0] = np.inf
    c.p2d[5, np.nonzero(c.mask[5])[0][3], 1] = np.nan
    c.mask[6, 0] = 0
    c.p2d[6, 0, 0] = np.nan
    for b, bad in ((7, 0.0), (8, -1.0), (9, np.inf), (10, np.nan)):
        c.scale[b, np.nonzero(c.mask[b])[0][2], b % 2] = bad
    c.mask[11, 1] = 0
    c.scale[11, 1] = (0.0, np.nan)
    c.t0[12, 2] = -c.t0[12, 2]
    return c


PASS_EXPECT = [1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]      # 1 = refined


def _unrobust_accept():
    """started a small step off the Huber fit of an outlier crop: the robust cost falls on the first step, the unrobust one rises"""
    base = _make("unrobust_accept", UNROBUST_SEED, 1, 64, "outlier")
    out = refine(*base.crop(0), base.R0[0], base.t0[0], base.delta, max_iters=40)
    rng = np.random.default_rng(UNROBUST_SEED)
    base.R0 = (L._rodrigues(rng.normal(size=3), np.radians(0.05)) @ out["R"])[None]
    base.t0 = out["t"][None] * (1.0 + 1e-4)
    return base


def _at_delta():
    """CPU only (it breaks the HUBER_GAP condition on purpose): delta is set to the |u| of one component at the input pose, which is
    then AT delta: `<=` leaves it unclipped and uncounted"""
    c = _make("at_delta", 181, 1, 32, "hetero")
    _, X, p, sc = _select(*c.crop(0)[:4])
    _, _, r0, _, _ = L.jacobian(X, p, c.K, c.R0[0], c.t0[0])
    c.delta = float(np.sort(np.abs(sc[:, 0] * r0))[len(r0) // 2])
    return c


UNROBUST_SEED = 0
# the seeds are 200 + 10 i + j but for outlier_3x512: with seed 252 its crop 1 is the rare draw in which row N22 over ALL points lands
# nearer the inlier-only fit than the Huber fit does (ADD 1.52 against 2.58: outliers of random sign leave a plain fit unbiased, only
# noisier), which tests/test_wlm.py asserts per crop; 1252 was the next seed tried (four alternatives gave 12 of 12 crops the usual order)
_SEEDS = {"outlier_3x512": 1252}
_SIZES = ((6, 3), (7, 3), (255, 1), (256, 3), (257, 1), (512, 3))
CASES = {}
for _i, (_n, _b) in enumerate(_SIZES):
    for _j, _kind in enumerate(("unit", "hetero", "outlier")):
        _name = "%s_%dx%d" % (_kind, _b, _n)
        CASES[_name] = (lambda name=_name, seed=_SEEDS.get(_name, 200 + 10 * _i + _j), b=_b, n=_n, kind=_kind, pc=(_n in (7, 256) and _b == 3):
                        _make(name, seed, b, n, kind, per_crop=pc, select=1.0 if n < 255 else 0.8))
CASES["passthrough"] = _passthrough
CASES["unrobust_accept"] = _unrobust_accept
HUBER = tuple(k for k in CASES if k.startswith("outlier")) + ("passthrough", "unrobust_accept")
CPU_ONLY = {"at_delta": _at_delta}
TAMPER_CASE = {"scale_r_only": "hetero_3x7", "omega_squared": "outlier_3x256", "huber_norm": "outlier_1x255", "lt_at_delta": "at_delta",
               "accept_unrobust": "unrobust_accept", "swap_xy": "hetero_1x257"}
CONF_TAMPER_CASE = {"pow_j": "msb_unsure", "p_for_q": "random", "floor_outside": "random"}


def make(name):
    return (CASES[name] if name in CASES else CPU_ONLY[name])()


def restatement_outputs(case, sums=numpy_sum, tamper=None, gaps=None):
    """(records (B,it,17), R (B,3,3), t (B,3), status (B,), info (B,42)) in the device's output layout"""
    outs = [refine(*case.crop(b), case.R0[b], case.t0[b], case.delta, case.status(b), case.max_iters, case.step_tol, sums, tamper, gaps)
            for b in range(case.B)]
    return (np.stack([o["records"] for o in outs]), np.stack([o["R"] for o in outs]), np.stack([o["t"] for o in outs]),
            np.array([o["status"] for o in outs], np.int32), np.stack([o["info"] for o in outs]))


def check_case(case, records, R, t, status, info, log=None):
    total = {}
    for b in range(case.B):
        st = check_crop(*case.crop(b), case.R0[b], case.t0[b], case.delta, case.status(b), case.max_iters, case.step_tol, b, records[b], R[b],
                        np.asarray(t[b]).reshape(3), int(status[b]), info[b])
        for k, v in st.items():
            total[k] = max(total.get(k, 0), v) if k.endswith("_1e18") else total.get(k, 0) + v
    if log is not None:
        log("%-18s status %s %s" % (case.name, np.asarray(status).tolist()[:13], " ".join("%s=%d" % kv for kv in sorted(total.items()))))
    return total


def measure_tau(case, records):
    """largest (|dR|_max, |dt| / |t|) between the trial from numpy's sums and from the kernel-order sums of the same terms, over every
    executed iteration of the restatement's run of a case"""
    worst = [0.0, 0.0]
    for b in range(case.B):
        _, X, p, sc = _select(*case.crop(b)[:4])
        K = np.asarray(case.crop(b)[4], np.float64)
        R, t = case.R0[b], case.t0[b]
        for rec in records[b]:
            if np.isnan(rec[0]):
                break
            T = point_terms(X, p, sc, K, R, t, case.delta)[0]
            a, k = trial(numpy_sum(T), R, t, rec[0]), trial(kernel_sum(T), R, t, rec[0])
            assert a[0] == k[0], (case.name, b)
            if a[0]:
                worst[0] = max(worst[0], float(np.abs(a[2] - k[2]).max()))
                worst[1] = max(worst[1], float(np.linalg.norm(a[3] - k[3]) / np.linalg.norm(t)))
            if rec[3]:
                R, t = rec[5:14].reshape(3, 3), rec[14:17]
    return worst


def measure_all(names=None, log=None):
    tau = [0.0, 0.0]
    for name in (names or CASES):
        case = make(name)
        gaps = []
        rec, R, t, status, info = restatement_outputs(case, gaps=gaps)
        a = measure_tau(case, rec)
        tau = [max(x, y) for x, y in zip(tau, a)]
        if log is not None:
            log("%-18s tau %.3e %.3e   gap %.3e   status %s iters %s clipped %s" % (name, a[0], a[1], min(gaps) if gaps else math.inf, status.tolist()[:13],
                                                                                    info[:13, 3].astype(int).tolist(), np.nan_to_num(info[:13, 41]).astype(int).tolist()))
    return tau


if __name__ == "__main__":
    tau = measure_all(sys.argv[1:], log=lambda s: print(s, flush=True))
    print("MEASURED_TAU = (%.3e, %.3e)" % (tau[0], tau[1]))
