"""Row N34 restated in numpy float64 (csrc/calibrate.hip states the rule): the reliability accumulators, the bracketed-Newton fit of the
inverse temperatures and the whitened-residual histogram, with math.fsum for every floating sum, the committed cases, the checker that
compares a result (the device's, or a tampered oracle's) against the oracle, and the named tamperings.  Not a test file.

What is exact: every integer, asserted with ==.  What is bounded: a floating sum of n terms against its fsum,
|difference| <= (n + 8) * 2^-53 * fsum(|terms|) -- n + 8 roundings of any summation order plus the per-term rounding.  The terms of the
whitened-residual sums use + - x / sqrt alone and are exact per term; the others go through exp / log1p, where two correctly working
libraries differ by an ulp or two per call and (p - y) cancels: the derived bound was measured against them before it was trusted
(MEASURED_RATIO) and holds as it is.  The fit is certified, not replayed: the oracle's gradient brackets zero around the returned scale."""
import math

import numpy as np

U = 2.0 ** -53
# The largest ratio |device - fsum| / ((n + 8) 2^-53 fsum|terms|) seen on an MI355X over the committed cases, for the sums whose terms go
# through exp / log1p (row h of random_B3_N1_r6_M2, n = 3; the next largest 0.43; every case of more than 65 samples below 0.3): below
# 1, so the derived bound stands with the factor 1 and nothing measured enters an assertion.  profiles/calib_bench.json carries the same
# figures per kind of sum.
MEASURED_RATIO = 0.872
TRANSCENDENTAL_FACTOR = 1.0

OK, CAPPED_HIGH, CAPPED_LOW, EMPTY, NOT_CONVERGED = 0, 1, 2, 3, 4


class StageError(AssertionError):
    def __init__(self, stage, row, msg):
        super().__init__("%s (row / crop / group %r): %s" % (stage, row, msg))
        self.stage, self.row = stage, row


def fs(x):
    """math.fsum where it is defined (finite terms), numpy's propagation of inf / NaN otherwise"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if x.size and not np.all(np.isfinite(x)):
        with np.errstate(all="ignore"):
            return float(np.sum(x))
    return math.fsum(x.tolist())


def logit_edges(M):
    return np.array([math.log(k / (M - k)) for k in range(1, M)], dtype=np.float64)


def chi2_edges(M):
    return np.array([-2.0 * math.log(1.0 - k / M) for k in range(1, M)], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------- per-sample terms
def terms(z32, y, s, tamper=None):
    """z32 float32 array (no NaN), y bool array, s float -> dict of float64 arrays t, p, nll, brier, g, h"""
    with np.errstate(all="ignore"):
        z = z32.astype(np.float64)
        t = z * s
        e = np.exp(-np.abs(t))
        p = np.where(t >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))
        d = p - y.astype(np.float64)
        nll = np.log1p(e) + np.where(y, np.maximum(-t, 0.0), np.maximum(t, 0.0))
        g = d if tamper == "g_no_z" else d * z
        return dict(t=t, p=p, nll=nll, brier=d * d, g=g, h=(p * (1.0 - p)) * (z * z))


def row_samples(case, k, tamper=None):
    """the counted samples of logit row k in (b, n) order -> (z32 with NaN still in, y bool)"""
    r = case["r"]
    roi = case["roi"][:, 0, :] > 0.5
    if k == 0:
        lab, sel = roi, np.ones_like(roi)
        if tamper == "roi_masked":
            sel = roi
    else:
        lab = (case["gx"][:, k - 1, :] if k <= r else case["gy"][:, k - 1 - r, :]) > 0.5
        sel = np.ones_like(roi) if tamper == "xy_unmasked" else roi
    z = case["bits"][:, k, :]
    return z[sel], lab[sel]


def bin_of(t, edges, tamper=None):
    """the number of edges <= t"""
    return np.searchsorted(edges, t, side="left" if tamper == "edge_lower" else "right")


# ------------------------------------------------------------------------------------------------------------- reliability
SUM_KEYS = ("nll", "brier", "g", "h")


def reliability(case, tamper=None):
    """-> dict like checkerpose_amd.calibrate.reliability's (numpy), plus abs_<sum> = fsum(|terms|) per floating sum (abs_sum_p per bin)"""
    K, edges, scale = 1 + 2 * case["r"], case["edges"], case["scale"]
    M = len(edges) + 1
    o = dict(count=np.zeros((K, M), np.int64), positives=np.zeros((K, M), np.int64), sum_p=np.zeros((K, M)), abs_sum_p=np.zeros((K, M)),
             n=np.zeros(K, np.int64), n_nan=np.zeros(K, np.int64), n_right=np.zeros(K, np.int64))
    for key in SUM_KEYS:
        o[key], o["abs_" + key] = np.zeros(K), np.zeros(K)
    for k in range(K):
        z, y = row_samples(case, k, tamper)
        nan = np.isnan(z)
        o["n_nan"][k] = int(nan.sum())
        z, y = z[~nan], y[~nan]
        o["n"][k] = z.size
        o["n_right"][k] = int(((z > 0) == y).sum())
        c = terms(z, y, float(scale[k]), tamper)
        b = bin_of(c["p"] if tamper == "bin_p" else c["t"], edges, tamper)
        for m in range(M):
            sel = b == m
            o["count"][k, m], o["positives"][k, m] = int(sel.sum()), int((sel & y).sum())
            o["sum_p"][k, m], o["abs_sum_p"][k, m] = fs(c["p"][sel]), fs(np.abs(c["p"][sel]))
        for key in SUM_KEYS:
            o[key][k] = fs(c[key])
            with np.errstate(all="ignore"):
                o["abs_" + key][k] = fs(np.abs(c[key]))
    return o


def _same_nonfinite(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def check_sum(stage, row, got, want, n, abs_sum, factor, ratios=None):
    """|got - want| <= factor (n + 8) 2^-53 abs_sum; a non-finite oracle value must be met in kind.  ratios: a dict that receives the
    largest |got - want| / ((n + 8) 2^-53 abs_sum) per stage (the measurement behind TRANSCENDENTAL_FACTOR)."""
    got, want = float(got), float(want)
    if not np.isfinite(want):
        if not _same_nonfinite(got, want):
            raise StageError(stage, row, "got %r, the oracle has %r" % (got, want))
        return
    unit = (n + 8) * U * abs_sum
    diff = abs(got - want)
    if ratios is not None and unit > 0:
        ratios[stage] = max(ratios.get(stage, 0.0), diff / unit)
    if not diff <= factor * unit:
        raise StageError(stage, row, "|%r - %r| = %.3g > %.3g = %g (n + 8) 2^-53 fsum|terms| (n = %d)" % (got, want, diff, factor * unit, factor, n))


def check_reliability(case, out, ratios=None):
    """out: a reliability result as numpy arrays (the device's, or an oracle's) against the oracle of `case`"""
    o = case.get("_oracle") or reliability(case)
    case["_oracle"] = o
    K = 1 + 2 * case["r"]
    for key in ("n_nan", "n", "n_right", "count", "positives"):
        got = np.asarray(out[key])
        if got.shape != o[key].shape or got.dtype != np.int64:
            raise StageError(key, None, "shape / dtype %r %r" % (got.shape, got.dtype))
        bad = np.argwhere(got != o[key])
        if len(bad):
            raise StageError(key, int(bad[0][0]), "got %r, the oracle has %r" % (got[tuple(bad[0])], o[key][tuple(bad[0])]))
    for k in range(K):
        for m in range(o["count"].shape[1]):
            check_sum("sum_p", k, out["sum_p"][k, m], o["sum_p"][k, m], int(o["count"][k, m]), o["abs_sum_p"][k, m], TRANSCENDENTAL_FACTOR, ratios)
        for key in SUM_KEYS:
            check_sum(key, k, out[key][k], o[key][k], int(o["n"][k]), o["abs_" + key][k], TRANSCENDENTAL_FACTOR, ratios)


# ------------------------------------------------------------------------------------------------------------- the fit
def group_rows(groups, r):
    K = 1 + 2 * r
    if isinstance(groups, str):
        return {"row": np.arange(K), "significance": np.concatenate([[0], 1 + np.arange(r), 1 + np.arange(r)]),
                "all": np.zeros(K, int)}[groups].astype(np.int32)
    return np.asarray(groups, dtype=np.int32)


def group_eval(case, rows, s):
    """n, nll, g, h of the rows `rows` at the shared s, by fsum; plus fsum |g terms|"""
    n, parts = 0, {k: [] for k in ("nll", "g", "h")}
    for k in rows:
        z, y = row_samples(case, k)
        keep = ~np.isnan(z)
        c = terms(z[keep], y[keep], s)
        n += int(keep.sum())
        for key in parts:
            parts[key].append(c[key])
    cat = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in parts.items()}
    with np.errstate(all="ignore"):
        return n, fs(cat["nll"]), fs(cat["g"]), fs(cat["h"]), fs(np.abs(cat["g"])), fs(np.abs(cat["nll"]))


def fit(case, tamper=None):
    """The committed iteration (csrc/calibrate.hip) with fsum evaluations -> dict(scale (K,), status, iters, nll_before, nll_after, n, s
    per group).  tamper "no_bracket": plain Newton, the bracket never consulted."""
    r, grp = case["r"], group_rows(case["groups"], case["r"])
    s_min, s_max, tol, max_iters = case["s_min"], case["s_max"], case["step_tol"], case["max_iters"]
    G = int(grp.max()) + 1
    o = dict(status=np.zeros(G, np.int32), iters=np.zeros(G, np.int32), nll_before=np.zeros(G), nll_after=np.zeros(G), n=np.zeros(G, np.int64),
             s=np.ones(G), group_of_row=grp)
    for gi in range(G):
        rows = [k for k in range(1 + 2 * r) if grp[k] == gi]
        s, lo, hi, best = 1.0, s_min, s_max, None
        for it in range(1, max_iters + 1):
            n, nll, g, h = group_eval(case, rows, s)[:4]
            o["iters"][gi] = it
            if it == 1:
                o["nll_before"][gi], o["n"][gi] = nll, n
                if n == 0:
                    o["status"][gi], o["nll_after"][gi] = EMPTY, nll
                    break
            if best is None or nll < best[1]:
                best = (s, nll)
            if g < 0.0:
                lo = s
            else:
                hi = s
            with np.errstate(all="ignore"):
                c = s - np.float64(g) / np.float64(h)
            if tamper != "no_bracket" and not (np.isfinite(h) and h > 0.0 and lo < c < hi):
                c = math.sqrt(lo * hi)
            c = float(c)
            if abs(c - s) <= tol * s:
                pending = 0
                if tamper != "no_bracket":
                    if hi == s_max and s_max - lo <= 3.0 * tol * s_max:
                        c, pending = s_max, 1
                    elif lo == s_min and hi - s_min <= 3.0 * tol * s_min:
                        c, pending = s_min, 2
                nll1, g1 = group_eval(case, rows, c)[1:3]
                o["s"][gi], o["nll_after"][gi] = c, nll1
                o["status"][gi] = CAPPED_HIGH if pending == 1 and g1 < 0.0 else CAPPED_LOW if pending == 2 and g1 > 0.0 else OK
                break
            if it >= max_iters:
                o["status"][gi], o["s"][gi], o["nll_after"][gi] = NOT_CONVERGED, best[0], best[1]
                break
            s = c
    o["scale"] = o["s"][grp]
    return o


def check_fit(case, out, ratios=None, report=None):
    """The certificate: for an OK group the oracle's gradient brackets zero within delta = 4 step_tol around the returned s; a capped
    group's gradient has the cap's sign at the cap; EMPTY has no sample; nll_after <= nll_before always; nll_before / nll_after are the
    oracle's NLL at 1 / at the returned s within the bound; scale[k] is its group's s.  report: a list that receives (group, s, n, h)."""
    r, grp = case["r"], group_rows(case["groups"], case["r"])
    G = int(grp.max()) + 1
    delta = 4.0 * case["step_tol"]
    status, s_out = np.asarray(out["status"]), np.asarray(out["s"], dtype=np.float64)
    if status.shape != (G,) or not np.array_equal(np.asarray(out["scale"]), s_out[grp]):
        raise StageError("scale", None, "scale is not the rows' groups' s")
    for gi in range(G):
        rows = [k for k in range(1 + 2 * r) if grp[k] == gi]
        s, st = float(s_out[gi]), int(status[gi])
        n1, nll_at1 = group_eval(case, rows, 1.0)[:2]
        if int(out["n"][gi]) != n1:
            raise StageError("n", gi, "got %r, the oracle counts %r" % (int(out["n"][gi]), n1))
        if (st == EMPTY) != (n1 == 0):
            raise StageError("status", gi, "status %d with %d samples" % (st, n1))
        if st == EMPTY:
            if s != 1.0:
                raise StageError("status", gi, "an empty group must keep s = 1")
            continue
        if not (case["s_min"] <= s <= case["s_max"]):
            raise StageError("certificate", gi, "s = %r outside the bracket" % s)
        nb, na = float(out["nll_before"][gi]), float(out["nll_after"][gi])
        if not na <= nb:
            raise StageError("nll", gi, "nll_after %r > nll_before %r" % (na, nb))
        n, nll_s, g_s, h_s, _, abs_nll = group_eval(case, rows, s)
        if np.isnan(g_s):
            # an infinite logit on the right side: (p - y) z = 0 * inf, the gradient is NaN at every s.  The rule's "otherwise hi = s" and its
            # bisection then walk the bracket down onto s_min, where g > 0 is false: OK at s_min is the rule's only outcome
            if not (st == OK and s == case["s_min"]):
                raise StageError("certificate", gi, "a NaN gradient must end OK at s_min, got status %d at s = %r" % (st, s))
            continue
        check_sum("nll", gi, na, nll_s, n, abs_nll, TRANSCENDENTAL_FACTOR, ratios)
        check_sum("nll", gi, nb, nll_at1, n, group_eval(case, rows, 1.0)[5], TRANSCENDENTAL_FACTOR, ratios)
        if report is not None:
            report.append((gi, s, n, h_s))

        def g_at(x):
            v = group_eval(case, rows, x)
            return v[2], TRANSCENDENTAL_FACTOR * (v[0] + 8) * U * v[4]
        if st == OK:
            (g_lo, e_lo), (g_hi, e_hi) = g_at(s * (1.0 - delta)), g_at(s * (1.0 + delta))
            if not (g_lo <= e_lo and g_hi >= -e_hi):
                raise StageError("certificate", gi, "g(s (1 - d)) = %r (eps %.3g), g(s (1 + d)) = %r (eps %.3g) at s = %r" % (g_lo, e_lo, g_hi, e_hi, s))
        elif st == CAPPED_HIGH:
            if not (s == case["s_max"] and g_at(case["s_max"])[0] < 0.0):
                raise StageError("certificate", gi, "CAPPED_HIGH but g(s_max) is not < 0 or s != s_max")
        elif st == CAPPED_LOW:
            if not (s == case["s_min"] and g_at(case["s_min"])[0] > 0.0):
                raise StageError("certificate", gi, "CAPPED_LOW but g(s_min) is not > 0 or s != s_min")
        elif st != NOT_CONVERGED:
            raise StageError("status", gi, "unknown status %d" % st)
        if st == NOT_CONVERGED:
            if int(out["iters"][gi]) != case["max_iters"]:
                raise StageError("status", gi, "NOT_CONVERGED after %d of %d evaluations" % (int(out["iters"][gi]), case["max_iters"]))
            ref = case.get("_fit") or fit(case)
            case["_fit"] = ref
            if ref["status"][gi] != NOT_CONVERGED and ref["iters"][gi] + 4 <= case["max_iters"]:      # (4 evaluations of slack: ulp-level differences)
                raise StageError("certificate", gi, "NOT_CONVERGED where the committed iteration stops after %d of %d evaluations"
                                 % (ref["iters"][gi], case["max_iters"]))


# ------------------------------------------------------------------------------------------------------------- sigma2 consistency
def pit(case, tamper=None):
    """-> dict(counts (B,E+1) int32, n, n_dropped (B,) int32, sum_d2, sum_u, sum_v (B,), abs_* likewise, d2: list of the counted d2)"""
    p2d, proj, s2, roi, edges = case["p2d"], case["proj"], case["sigma2"], case["roi"][:, 0, :] > 0.5, case["edges"]
    valid = case["valid"][:, :, case["column"]] != 0
    B, N = valid.shape
    o = dict(counts=np.zeros((B, len(edges) + 1), np.int32), n=np.zeros(B, np.int32), n_dropped=np.zeros(B, np.int32), d2=[])
    for key in ("sum_d2", "sum_u", "sum_v"):
        o[key], o["abs_" + key] = np.zeros(B), np.zeros(B)
    with np.errstate(all="ignore"):
        good = valid & roi & np.isfinite(s2).all(2) & (s2 > 0).all(2)
        if tamper == "dropped_counted":
            good = valid & roi
        du = p2d[..., 0].astype(np.float64) - proj[..., 0]
        dv = p2d[..., 1].astype(np.float64) - proj[..., 1]
        den = np.sqrt(s2) if tamper == "pit_sigma" else s2
        d2 = (du * du) / den[..., 0] + (dv * dv) / den[..., 1]
        u, v = du / np.sqrt(s2[..., 0]), dv / np.sqrt(s2[..., 1])
    for b in range(B):
        sel = good[b]
        o["n"][b], o["n_dropped"][b] = int(sel.sum()), int(N - sel.sum())
        o["counts"][b] = np.bincount(np.searchsorted(edges, d2[b][sel], side="right"), minlength=len(edges) + 1)
        o["d2"].append(d2[b][sel])
        for key, x in (("sum_d2", d2), ("sum_u", u), ("sum_v", v)):
            o[key][b], o["abs_" + key][b] = fs(x[b][sel]), fs(np.abs(x[b][sel]))
    return o


def pit_undecided(case, o=None):
    """the counted points whose d2 is within a relative 2^-40 of an edge without being ON it (an on-edge point built from powers of two is
    exact on both sides): the committed cases have none"""
    o = o or pit(case)
    bad = 0
    for d2 in o["d2"]:
        for e in case["edges"]:
            with np.errstate(all="ignore"):
                bad += int(((d2 != e) & (np.abs(d2 - e) <= 2.0 ** -40 * abs(e))).sum())
    return bad


def check_pit(case, out, ratios=None):
    o = case.get("_oracle") or pit(case)
    case["_oracle"] = o
    for key in ("n", "n_dropped", "counts"):
        got = np.asarray(out[key])
        if got.shape != o[key].shape or got.dtype != np.int32:
            raise StageError(key, None, "shape / dtype %r %r" % (got.shape, got.dtype))
        bad = np.argwhere(got != o[key])
        if len(bad):
            raise StageError(key, int(bad[0][0]), "got %r, the oracle has %r" % (got[tuple(bad[0])], o[key][tuple(bad[0])]))
    for b in range(len(o["n"])):
        for key in ("sum_d2", "sum_u", "sum_v"):
            check_sum(key, b, out[key][b], o[key][b], int(o["n"][b]), o["abs_" + key][b], 1.0, ratios)


# ------------------------------------------------------------------------------------------------------------- the committed cases
SPECIAL_LOGITS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e30, -1e30], dtype=np.float32)


def bits_case(B, N, r, M, seed, kind="random", rows_extra=0, scale="mixed"):
    """bits (B, 1 + 2r + rows_extra, N) f32, labels with `r + 1` code rows (one more than predicted), scale, edges.
    kind: random | special (0, -0, +-inf, NaN, +-1e30 and on-edge products sprinkled in) | labels0 | labels1 | separable | antiseparable |
    empty_crop (crop 0's GT RoI bits all 0) | no_roi (every GT RoI bit 0)"""
    rng = np.random.default_rng(seed)
    K = 1 + 2 * r
    bits = (rng.normal(size=(B, K + rows_extra, N)) * 3.0).astype(np.float32)
    roi = (rng.random((B, 1, N)) < 0.7).astype(np.float32)
    gx = (rng.random((B, r + 1, N)) < 0.5).astype(np.float32)
    gy = (rng.random((B, r + 1, N)) < 0.5).astype(np.float32)
    edges = logit_edges(M)
    sc = np.ones(K) if scale == "ones" else np.exp2(rng.integers(-2, 3, size=K).astype(np.float64)) * (1.0 + (rng.random(K) < 0.5) * rng.random(K))
    if kind == "special":
        flat = bits.reshape(-1)
        idx = rng.choice(flat.size, max(1, flat.size // 5), replace=False)
        flat[idx] = SPECIAL_LOGITS[np.arange(idx.size) % len(SPECIAL_LOGITS)]
        if M > 1:                                    # products that land exactly on an edge: z a power of two, s = edge / z (exact)
            for k in range(K):
                e = edges[(k * 3) % (M - 1)]
                if e > 0.0:
                    sc[k] = e / 2.0
                    bits[:, k, :: 3] = 2.0
                elif e < 0.0:
                    sc[k] = -e / 4.0
                    bits[:, k, :: 3] = -4.0
                else:
                    bits[:, k, :: 3] = np.where(np.arange(len(bits[0, k, :: 3])) % 2 == 0, 0.0, -0.0)
    elif kind == "labels0":
        gx[:], gy[:], roi[:, :, ::2] = 0.0, 0.0, 1.0
    elif kind == "labels1":
        gx[:], gy[:], roi[:] = 1.0, 1.0, 1.0
    elif kind in ("separable", "antiseparable"):
        roi[:] = 1.0
        pos = bits[:, :K, :] > 0
        if kind == "antiseparable":
            pos = ~pos
        lab = pos.astype(np.float32)
        gx[:, :r, :], gy[:, :r, :] = lab[:, 1:1 + r, :], lab[:, 1 + r:, :]
        # (the RoI label of row 0 decides which x / y samples count: keep every keypoint in by leaving roi = 1 for the x / y rows;
        #  row 0 is then "all positives", separable only where its logits are positive -- flip them)
        bits[:, 0, :] = np.abs(bits[:, 0, :]) * (1.0 if kind == "separable" else -1.0)
    elif kind == "empty_crop":
        roi[0] = 0.0
    elif kind == "no_roi":
        roi[:] = 0.0
    return dict(bits=bits[:, :K, :], block=bits, r=r, roi=roi, gx=gx, gy=gy, edges=edges, M=M, scale=sc, name="%s_B%d_N%d_r%d_M%d" % (kind, B, N, r, M))


def fit_case(B, N, r, seed, kind="recovery", groups="row", s_min=2.0 ** -6, s_max=2.0 ** 6, step_tol=1e-8, max_iters=60):
    """recovery: z = t_true / s0 with labels drawn from sigmoid(t_true) (s0 per GROUP, so that a shared s has one truth)"""
    rng = np.random.default_rng(seed)
    K = 1 + 2 * r
    grp = group_rows(groups, r)
    if kind in ("recovery", "newton_leaves"):
        s0 = np.exp2(rng.uniform(-1.5, 1.5, size=int(grp.max()) + 1))[grp]
        t_true = rng.normal(size=(B, K, N)) * 2.5
        bits = (t_true / s0[None, :, None]).astype(np.float32)
        prob = 1.0 / (1.0 + np.exp(-bits.astype(np.float64) * s0[None, :, None]))
        lab = (rng.random((B, K, N)) < prob).astype(np.float32)
        if kind == "newton_leaves":      # confident logits, a few of them wrong: at s = 1 the curvature has underflowed, Newton's step is huge
            bits = (np.sign(t_true) * (30.0 + np.abs(t_true))).astype(np.float32)
            lab = (bits > 0).astype(np.float32)
            flip = rng.random((B, K, N)) < 0.05
            lab = np.where(flip, 1.0 - lab, lab).astype(np.float32)
            s0 = np.full(K, np.nan)
        case = dict(bits=bits, block=bits, r=r, roi=lab[:, :1, :].copy(), gx=lab[:, 1:1 + r, :].copy(), gy=lab[:, 1 + r:, :].copy(), s0=s0)
        # the x / y rows count where the GT RoI bit is set: that thins them by the row-0 labels, independent of their own draws
    else:
        c = bits_case(B, N, r, 2, seed, kind=kind)
        case = dict(bits=c["bits"], block=c["block"], r=r, roi=c["roi"], gx=c["gx"], gy=c["gy"], s0=np.full(K, np.nan))
    case.update(groups=groups, s_min=s_min, s_max=s_max, step_tol=step_tol, max_iters=max_iters,
                name="fit_%s_B%d_N%d_r%d_%s" % (kind, B, N, r, groups if isinstance(groups, str) else "array"))
    return case


BAD_VARIANCES = (np.nan, np.inf, 0.0, -0.0, -1.0, -np.inf)


def pit_case(B, N, seed, bins=10, column=0, kind="random"):
    """p2d = proj + sqrt(sigma2) * N(0, 1) * spread; kind: random | bad (variances NaN / inf / 0 / -0 / negative on ONE axis) | on_edge
    (explicit edges with 1.0 among them; points with du = 2, sigma2_x = 4, dv = 0: d2 = 1.0 exactly)"""
    rng = np.random.default_rng(seed)
    proj = rng.uniform(50.0, 400.0, size=(B, N, 2))
    s2 = rng.uniform(0.2, 30.0, size=(B, N, 2))
    p2d = (proj + np.sqrt(s2) * rng.normal(size=(B, N, 2)) * 1.3).astype(np.float32)
    valid = (rng.random((B, N, 3)) < 0.8).astype(np.uint8)
    roi = (rng.random((B, 1, N)) < 0.8).astype(np.float32)
    edges = chi2_edges(bins) if isinstance(bins, int) else np.asarray(bins, dtype=np.float64)
    if kind == "bad":
        for b in range(B):
            for j, i in enumerate(rng.choice(N, max(1, N // 3), replace=False)):
                s2[b, i, j % 2] = BAD_VARIANCES[j % len(BAD_VARIANCES)]
    elif kind == "on_edge":
        edges = np.array([0.25, 1.0, 4.0, 5.99, 9.21])
        proj[:, ::2, :] = np.round(proj[:, ::2, :])                  # integers: the float32 p2d = proj + 2 is exact
        p2d[:, ::2, 0], p2d[:, ::2, 1] = (proj[:, ::2, 0] + 2.0).astype(np.float32), proj[:, ::2, 1].astype(np.float32)
        s2[:, ::2, 0], s2[:, ::2, 1] = 4.0, 0.5
        valid[:, ::2, :], roi[:, 0, ::2] = 1, 1.0
    return dict(p2d=p2d, proj=proj, sigma2=s2, valid=valid, roi=roi, edges=edges, column=column, name="pit_%s_B%d_N%d_c%d" % (kind, B, N, column))


N_LIST, B_LIST = (1, 63, 64, 65, 257, 512), (1, 3, 17)


def reliability_cases():
    """every N with every B once (r and M rotate), plus every kind, every M, a batch stride (rows_extra) -- the smallest that can break"""
    out, i = [], 0
    for N in N_LIST:
        for B in B_LIST:
            out.append(bits_case(B, N, (1, 6)[i % 2], (1, 2, 15, 64)[i % 4], 100 + i, kind=("random", "special")[(i // 2) % 2], rows_extra=i % 3))
            i += 1
    for j, kind in enumerate(("labels0", "labels1", "separable", "antiseparable", "empty_crop", "no_roi", "special")):
        out.append(bits_case(3, 65, 6, (15, 64, 2, 15, 15, 15, 64)[j], 200 + j, kind=kind, rows_extra=j % 2))
    return out


def fit_cases():
    out = [fit_case(3, 257, 6, 300, groups="row"), fit_case(17, 512, 6, 301, groups="significance"), fit_case(3, 65, 1, 302, groups="all"),
           fit_case(1, 512, 6, 303, groups=[0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]), fit_case(1, 1, 1, 304, groups="row"),
           fit_case(3, 64, 6, 305, kind="separable"), fit_case(3, 63, 6, 306, kind="antiseparable"), fit_case(3, 65, 6, 307, kind="empty_crop"),
           fit_case(3, 65, 6, 308, kind="no_roi"), fit_case(3, 65, 6, 309, kind="labels0"), fit_case(3, 65, 6, 310, kind="labels1"),
           fit_case(3, 257, 6, 311, kind="newton_leaves", groups="significance"), fit_case(3, 257, 6, 312, max_iters=2),
           fit_case(3, 65, 6, 313, kind="special", groups="all"), fit_case(3, 257, 1, 314, s_min=0.5, s_max=1.0)]
    return out


def pit_cases():
    out, i = [], 0
    for N in N_LIST:
        for B in B_LIST:
            out.append(pit_case(B, N, 400 + i, bins=(10, 1, 64, 2)[i % 4], column=i % 3, kind=("random", "bad", "on_edge")[i % 3]))
            i += 1
    return out


# ------------------------------------------------------------------------------------------------------------- the named tamperings
# name -> (which checker, a case builder, the tampered oracle, the stage that must catch it)
TAMPERINGS = {
    "edge_to_lower_bin": ("reliability", lambda: bits_case(3, 65, 6, 15, 207, kind="special"), lambda c: reliability(c, "edge_lower"), "count"),
    "xy_rows_unmasked": ("reliability", lambda: bits_case(3, 65, 6, 15, 100), lambda c: reliability(c, "xy_unmasked"), "n"),
    "roi_row_masked": ("reliability", lambda: bits_case(3, 65, 6, 15, 100), lambda c: reliability(c, "roi_masked"), "n"),
    "p_binned_instead_of_t": ("reliability", lambda: bits_case(3, 65, 6, 15, 100), lambda c: reliability(c, "bin_p"), "count"),
    "g_without_z": ("reliability", lambda: bits_case(3, 65, 6, 15, 100), lambda c: reliability(c, "g_no_z"), "g"),
    "newton_without_bracket": ("fit", lambda: fit_case(3, 257, 6, 311, kind="newton_leaves", groups="significance"), lambda c: fit(c, "no_bracket"),
                               "certificate"),
    "pit_sigma_for_sigma2": ("pit", lambda: pit_case(3, 65, 401), lambda c: pit(c, "pit_sigma"), "counts"),
    "dropped_points_counted": ("pit", lambda: pit_case(3, 65, 402, kind="bad"), lambda c: pit(c, "dropped_counted"), "n"),
}
CHECKERS = {"reliability": check_reliability, "fit": check_fit, "pit": check_pit}
ORACLES = {"reliability": reliability, "fit": fit, "pit": pit}
