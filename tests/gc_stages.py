"""TEST INFRASTRUCTURE (not collected): the graph-cut RANSAC pose solver (cp_pnp_gc) restated in numpy and checked
stage by stage by replaying the records the device itself leaves (postprocess.solve_pnp_gc(return_stages=True)), in the style of
tests/pnp_stages.py, whose case makers, BAND / UNDECIDED_CAP, TAU and E margins it reuses.

The rule (this project's own; parity with pyprogressivex is UNPINNED -- the package is not part of the reference's tree):
  hypotheses   rounds of 64; hypothesis h draws oracle.sample_indices(seed, crop, h, nv, 4), oracle.solve_four_points; count = valid
               points with r^2 <= thr^2, score = sum over them of 1 - r^2 / thr^2; oracle.needed_iterations (m = 4) between rounds;
               winner = first record with the largest score among those with count >= 4; nv < min_inliers or no such record: identity
  labelling    Q = 2^16; cin_i = floor(min(r_i^2 / thr^2, 2^14) Q + 0.5), cout = Q, w = floor(lambda Q + 0.5) per direction on every
               graph edge between two valid points; inliers = the MINIMAL source side of a minimum cut of s->i = cout, i->t = cin_i,
               i<->j = w (`label`: scipy.sparse.csgraph.maximum_flow + a BFS over the residual graph)
  LO           P_0 = winner; step k = 0..LO_MAX: L_k = label(P_k); stop if |L_k| < min_inliers; k < LO_MAX: Q_k = EPnP over L_k, stop
               if it fails or score(Q_k) <= score(P_k), else P_{k+1} = Q_k.  Returned: the last P_k and L_k, status 1 -- or the
               identity, status 0, when |L_k| < min_inliers.

`check_crop` stages (issue N17):
  A  which hypothesis records exist (stopping rule replayed on the recorded counts); the four-point pose against
     oracle.solve_four_points on the same sample within pnp_stages.TAU_CAP; count -1 only where the oracle finds no pose either
  B  count exact outside BAND (undecided pairs counted against UNDECIDED_CAP by check_case); every recorded score within 1e-9
     relative of numpy's under the RECORDED pose
  C  the winner and every accept / stop decision replayed on the RECORDED scores: exact; poses handed on bit for bit
  D  |cin_dev - cin_numpy| <= 1 under the recorded pose
  E  labels EQUAL to the canonical cut of the RECORDED capacities
  F  the refit against oracle.epnp over the device's list within pnp_stages.taus(), for one of the 8 axis orientations
  G  known answers on noise-free crops (where a run hypothesis' sample holds no outlier): returned inliers == valid non-outliers,
     pose within pnp_stages.e_margins().  The case maker asserts (`assert_unary_decides`) that under the true pose every valid
     outlier has cin - Q > w * degree and every valid non-outlier Q - cin > w * (its valid outlier neighbours): then the unary
     term alone decides (flipping any set of labels of the true labelling raises the energy).

`count_sweeps` restates the device's max-flow (csrc/pnp_gc.hip:gc_maxflow: cancellation, push-relabel sweeps in node order, a global
relabel every 8 sweeps, labels = reachable from the nodes left with excess) on one lane: it is how the kernel's sweep bound was chosen
(`python -m tests.gc_stages` prints the largest count over the committed cases) and shows on a CPU that this procedure yields the
canonical cut."""
import os
import sys

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import breadth_first_order, maximum_flow

from oracle import pnp_oracle as P
from tests import pnp_stages as S
from tests.pnp_stages import StageError

Q = 1 << 16
CIN_CAP = 1 << 14
LO_MAX = 8
STEP = 30
SCORE_RTOL = 1e-9
SWEEPS_PER_RELABEL, MAX_SWEEPS = 8, 2048          # csrc/pnp_gc.hip
INF = 0x3fffffff


# ---------------------------------------------------------------------------------------------------------------- the graph
def radius_graph_np(xyz, radius):
    """CSR (offsets (N+1,) int32, indices int32, columns ascending) of the pairs i != j with dx*dx + dy*dy + dz*dz <= radius^2, in
    fp64 from the fp32 coordinates"""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    n = len(x)
    r2 = float(radius) * float(radius)
    rows = []
    for i0 in range(0, n, 512):
        d = x[i0:i0 + 512, None, :] - x[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        adj = d2 <= r2
        adj[np.arange(adj.shape[0]), np.arange(i0, i0 + adj.shape[0])] = False
        rows.append(adj)
    adj = np.concatenate(rows, 0)
    offsets = np.concatenate([[0], np.cumsum(adj.sum(1))]).astype(np.int32)
    return offsets, np.nonzero(adj)[1].astype(np.int32)


def min_margin(xyz, radius):
    """smallest | d2 / radius^2 - 1 | over the pairs: a cloud whose margin is below 1e-9 is refused by the makers"""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    r2 = float(radius) ** 2
    return float(np.abs(d2 / r2 - 1.0).min()) if r2 > 0 else np.inf


# ---------------------------------------------------------------------------------------------------------------- the labelling
def _arcs(cin, offsets, indices, w):
    cin = np.asarray(cin, np.int64)
    n = len(cin)
    node = cin >= 0
    rows = np.repeat(np.arange(n), np.diff(offsets))
    cols = np.asarray(indices, np.int64)
    keep = node[rows] & node[cols] if len(cols) else np.zeros(0, bool)
    return cin, n, node, rows[keep], cols[keep]


def label(cin, offsets, indices, w):
    """-> (labels (N,) bool: the minimal source side of a minimum cut, flow value): scipy's exact max-flow + BFS from s over the
    residual arcs.  cin (N,) integers, -1 = not a node."""
    cin, n, node, er, ec = _arcs(cin, offsets, indices, w)
    s, t = n, n + 1
    vid = np.nonzero(node)[0]
    r = np.concatenate([np.full(len(vid), s), vid, er if w > 0 else []]).astype(np.int64)
    c = np.concatenate([vid, np.full(len(vid), t), ec if w > 0 else []]).astype(np.int64)
    v = np.concatenate([np.full(len(vid), Q), cin[vid], np.full(len(er) if w > 0 else 0, w)]).astype(np.int64)
    nz = v > 0
    cap = sp.csr_matrix((v[nz].astype(np.int32), (r[nz], c[nz])), shape=(n + 2, n + 2))
    res = maximum_flow(cap, s, t)
    resid = (cap - res.flow).tocsr()
    resid.data = np.where(resid.data > 0, 1, 0)
    resid.eliminate_zeros()
    reach = np.zeros(n + 2, bool)
    reach[breadth_first_order(resid, s, directed=True, return_predecessors=False)] = True
    return reach[:n] & node, int(res.flow_value)


def cut_value(cin, offsets, indices, w, labels):
    """capacity of the cut ({s} + labels, rest)"""
    cin, n, node, er, ec = _arcs(cin, offsets, indices, w)
    lab = np.asarray(labels, bool)
    return int(Q * (node & ~lab).sum() + cin[lab & node].sum() + w * (lab[er] & ~lab[ec]).sum())


def count_sweeps(cin, offsets, indices, w):
    """csrc/pnp_gc.hip:gc_maxflow on one lane -> (labels, flow value, sweeps); RuntimeError at the kernel's bound"""
    cin = np.asarray(cin, np.int64)
    n = len(cin)
    off = [int(x) for x in offsets]
    idx = [int(x) for x in indices]
    node = [bool(c >= 0) for c in cin]
    ex = [int(Q - c) if 0 <= c < Q else 0 for c in cin]
    sk = [int(c - Q) if c >= Q else 0 for c in cin]
    part = int(sum(min(int(c), Q) for c in cin if c >= 0) + sum(sk))
    flow = [0] * len(idx)
    rev = {}
    for u in range(n):
        for a in range(off[u], off[u + 1]):
            rev[(u, idx[a])] = a
    sweeps, done = 0, False
    h = [INF] * n
    for rnd in range(MAX_SWEEPS // SWEEPS_PER_RELABEL + 1):
        h = [1 if node[i] and sk[i] > 0 else INF for i in range(n)]
        frontier, L = [i for i in range(n) if h[i] == 1], 1
        while frontier:                                      # BFS from the sink over residual arcs v -> u
            nxt = []
            for u in frontier:
                for a in range(off[u], off[u + 1]):
                    v = idx[a]
                    if node[v] and h[v] == INF and w + flow[a] > 0:      # residual of v -> u = w - flow[v -> u] = w + flow[u -> v]
                        h[v] = L + 1
                        nxt.append(v)
            frontier, L = nxt, L + 1
        if not any(ex[i] > 0 and h[i] < INF for i in range(n)):
            done = True
            break
        if rnd == MAX_SWEEPS // SWEEPS_PER_RELABEL:
            break
        for _ in range(SWEEPS_PER_RELABEL):
            for u in range(n):
                e0, hu = ex[u], h[u]
                if e0 <= 0 or hu >= INF:
                    continue
                rem, hmin = e0, INF
                if sk[u] > 0:
                    d = min(rem, sk[u])
                    sk[u] -= d
                    rem -= d
                for a in range(off[u], off[u + 1]):
                    if rem <= 0:
                        break
                    v = idx[a]
                    r = w - flow[a]
                    if not node[v] or r <= 0:
                        continue
                    if h[v] < hu:
                        d = min(rem, r)
                        flow[a] += d
                        flow[rev[(v, u)]] -= d
                        ex[v] += d
                        rem -= d
                    elif h[v] < hmin:
                        hmin = h[v]
                if rem != e0:
                    ex[u] += rem - e0
                else:
                    h[u] = INF if hmin >= INF else hmin + 1
            sweeps += 1
    if not done:
        raise RuntimeError("count_sweeps: %d sweeps did not suffice" % sweeps)
    lab = [node[i] and ex[i] > 0 for i in range(n)]
    stack = [i for i in range(n) if lab[i]]
    while stack:
        u = stack.pop()
        for a in range(off[u], off[u + 1]):
            v = idx[a]
            if node[v] and not lab[v] and w - flow[a] > 0:
                lab[v] = True
                stack.append(v)
    return np.array(lab, bool), part - sum(sk), sweeps


# ---------------------------------------------------------------------------------------------------------------- the solver
def weight(lam):
    return int(np.floor(float(lam) * Q + 0.5))


def sq_errors(p3d, p2d, K, R, t):
    return S._sq_errors(p3d, p2d, K, np.asarray(R, np.float64).reshape(1, 3, 3), np.asarray(t, np.float64).reshape(1, 3))[0]


def msac(d2, thr2):
    with np.errstate(invalid="ignore"):
        inl = d2 <= thr2
    return int(inl.sum()), float((1.0 - d2[inl] / thr2).sum())


def cin_of(d2, valid, thr2):
    with np.errstate(all="ignore"):
        q = d2 / thr2
    q = np.where(q < CIN_CAP, q, float(CIN_CAP))                # the cap, also where the projection is not finite
    return np.where(valid, np.floor(q * Q + 0.5), -1).astype(np.int64)


def expected_rounds(counts, nv, iterations, min_inliers):
    if nv < min_inliers:
        return 0
    done, best, r = min(iterations, 64), -1, 1
    while 64 * r < iterations:
        c = counts[64 * (r - 1):64 * r]
        c = c[~np.isnan(c)]
        best = max(best, int(c.max()) if len(c) else -1)
        if 64 * r >= P.needed_iterations(best, nv, 4, iterations):
            break
        done = min(iterations, 64 * (r + 1))
        r += 1
    return done


def _four(p3d, p2d, K, s):
    with np.errstate(all="ignore"):
        try:
            return P.solve_four_points(p3d[s], p2d[s], K)
        except np.linalg.LinAlgError:
            return None


def well_posed(p3d, p2d, K, s):
    """Is the oracle's four-point answer on sample s its own?  P3P's quartic has near-multiple roots on some samples; there the
    answer (which roots are real, which one the fourth point picks) turns on the last bits of the root finder, np.roots in the oracle
    and Durand-Kerner on the device, and neither is the reference of the other.  The criterion uses the oracle alone: the sample's
    pixels scaled by 1 +- 1e-9 (far below their fp32 spacing) must give the same verdict and a pose within TAU_CAP / 16.  The case
    makers refuse a case that holds an ill-posed sample (`assert_well_posed`), as they refuse a cloud with a pair at the radius."""
    base = _four(p3d, p2d, K, s)
    for sg in (1.0, -1.0):
        q = np.array(p2d, np.float64)
        q[s] = q[s] * (1.0 + sg * 1e-9)
        o = _four(p3d, q, K, s)
        if (o is None) != (base is None):
            return False
        if base is not None and not (np.abs(o[0] - base[0]).max() <= S.TAU_CAP[0] / 16 and
                                     np.abs(o[1] - base[1]).max() <= S.TAU_CAP[1] / 16 * max(1.0, np.linalg.norm(base[1]))):
            return False
    return True


def solve_gc(p3d, p2d, valid, K, offsets, indices, thr=2.0, lam=0.1, iterations=400, min_inliers=6, seed=0, crop=0):
    """the whole rule in numpy, in the device's layouts: -> (R, t (3,), inliers (N,), status, dict(hypotheses (iterations,14),
    steps (9,30), cin (9,N), labels (9,N)))"""
    p3d, p2d, K = np.asarray(p3d, np.float64), np.asarray(p2d, np.float64), np.asarray(K, np.float64)
    valid = np.asarray(valid).astype(bool)
    N = len(p3d)
    vid = np.nonzero(valid)[0]
    nv = len(vid)
    thr2 = float(np.float32(thr)) ** 2
    w = weight(lam)
    rec = np.full((iterations, 14), np.nan)
    steps = np.full((LO_MAX + 1, STEP), np.nan)
    cins, labs = np.full((LO_MAX + 1, N), -2, np.int64), np.full((LO_MAX + 1, N), 255, np.uint8)
    st = dict(hypotheses=rec, steps=steps, cin=cins, labels=labs)
    ident = (np.eye(3), np.zeros(3), np.zeros(N, bool), 0, st)
    if nv < min_inliers:
        return ident
    best = -1
    for h in range(iterations):
        if h > 0 and h % 64 == 0 and h >= P.needed_iterations(best, nv, 4, iterations):
            break
        rec[h, 0] = -1
        rt = _four(p3d, p2d, K, vid[P.sample_indices(seed, crop, h, nv, 4)])
        if rt is None:
            continue
        cnt, sc = msac(sq_errors(p3d[vid], p2d[vid], K, rt[0], rt[1]), thr2)
        rec[h, 0], rec[h, 1], rec[h, 2:11], rec[h, 11:14] = cnt, sc, rt[0].reshape(9), rt[1]
        best = max(best, cnt)
    cand = np.nonzero(np.nan_to_num(rec[:, 0], nan=-1) >= 4)[0]
    if not len(cand):
        return ident
    win = int(cand[np.argmax(rec[cand, 1])])
    Pk, sP = rec[win, 2:14].copy(), rec[win, 1]
    have = False
    for k in range(LO_MAX + 1):
        cin = cin_of(sq_errors(p3d, p2d, K, Pk[:9], Pk[9:]), valid, thr2)
        lab, _ = label(cin, offsets, indices, w)
        steps[k, 0], steps[k, 1:13], steps[k, 13], steps[k, 14] = k, Pk, sP, lab.sum()
        steps[k, 29] = 0                                        # (sweeps: the device's own figure; scipy solves this one)
        cins[k], labs[k] = cin, lab
        have = lab.sum() >= min_inliers
        if not have or k == LO_MAX:
            break
        sel = np.nonzero(lab)[0]
        fit = S._oracle_epnp(p3d[sel], p2d[sel], K)
        steps[k, 15] = 0.0 if fit is None else 1.0
        if fit is None:
            break
        Qk = np.concatenate([fit[0].reshape(9), fit[1]])
        sQ = msac(sq_errors(p3d[vid], p2d[vid], K, Qk[:9], Qk[9:]), thr2)[1]
        steps[k, 16:28], steps[k, 28] = Qk, sQ
        if not sQ > sP:
            break
        Pk, sP = Qk, sQ
    if not have:
        return ident
    return Pk[:9].reshape(3, 3), Pk[9:].copy(), labs[k].astype(bool), 1, st


def check_crop(p3d, p2d, valid, K, offsets, indices, thr, lam, iterations, min_inliers, seed, crop, stages, R, t, inliers, status, truth=None):
    """Raises StageError where the device's outputs contradict its own records or numpy.  stages: dict of this crop's hypotheses
    (iterations,14), steps (9,30), cin (9,N), labels (9,N).  -> statistics (pairs / undecided for check_case's cap, sweeps, ...)"""
    p3d, p2d, K = np.asarray(p3d, np.float64), np.asarray(p2d, np.float64), np.asarray(K, np.float64)
    valid, inliers = np.asarray(valid).astype(bool), np.asarray(inliers).astype(bool)
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    rec, steps = np.asarray(stages["hypotheses"], np.float64), np.asarray(stages["steps"], np.float64)
    cins, labs = np.asarray(stages["cin"]).astype(np.int64), np.asarray(stages["labels"])
    N = len(p3d)
    vid = np.nonzero(valid)[0]
    nv = len(vid)
    thr2 = float(np.float32(thr)) ** 2
    w = weight(lam)
    stats = dict(pairs=0, undecided=0, written=0, rounds=0, degenerate=0, steps=0, sweeps=0, all_inlier=0)
    if rec.shape != (iterations, 14) or steps.shape != (LO_MAX + 1, STEP):
        raise StageError("A", crop, None, "records have shapes %r %r" % (rec.shape, steps.shape))

    def identity_expected(stage, why):
        if status != 0 or not np.array_equal(R, np.eye(3)) or t.any() or inliers.any():
            raise StageError(stage, crop, None, "%s: expected the identity pose, no inliers, status 0; got status %d, %d inliers" % (why, status, inliers.sum()))

    # ---- A: which records exist, the four-point poses
    need = expected_rounds(rec[:, 0], nv, iterations, min_inliers)
    for h in range(iterations):
        if h < need and np.isnan(rec[h, 0]):
            raise StageError("A", crop, h, "record missing: the stopping rule demands %d hypotheses (nv = %d)" % (need, nv))
        if h >= need and not np.isnan(rec[h]).all():
            raise StageError("A", crop, h, "record written beyond the %d hypotheses the stopping rule demands (nv = %d)" % (need, nv))
    stats["written"], stats["rounds"] = need, (need + 63) // 64
    counts = rec[:need, 0]
    if need and not (np.all(counts == np.rint(counts)) and counts.min() >= -1 and counts.max() <= nv):
        raise StageError("A", crop, None, "a count is no integer in -1..nv")
    if nv < min_inliers:
        if not np.isnan(steps).all():
            raise StageError("C", crop, None, "a step ran with %d valid points" % nv)
        identity_expected("C", "%d valid points" % nv)
        return stats
    samples = [vid[P.sample_indices(seed, crop, h, nv, 4)] for h in range(need)]
    for h in range(need):
        assert well_posed(p3d, p2d, K, samples[h]), (crop, h, "the case holds an ill-posed four-point sample (GcCase.assert_well_posed)")
        rt = _four(p3d, p2d, K, samples[h])
        if counts[h] < 0:
            stats["degenerate"] += 1
            if rt is not None:
                raise StageError("A", crop, h, "count -1, but the oracle's solve_four_points solves the sample %r" % (samples[h].tolist(),))
            continue
        if rt is None:
            raise StageError("A", crop, h, "a pose where the oracle's solve_four_points finds none, sample %r" % (samples[h].tolist(),))
        dR, dt = np.abs(rec[h, 2:11].reshape(3, 3) - rt[0]).max(), np.abs(rec[h, 11:14] - rt[1]).max()
        if not (dR <= S.TAU_CAP[0] and dt <= S.TAU_CAP[1] * max(1.0, np.linalg.norm(rt[1]))):
            raise StageError("A", crop, h, "four-point pose off the oracle's by %.3e / %.3e, sample %r" % (dR, dt, samples[h].tolist()))

    # ---- B: counts and scores under the recorded poses
    posed = np.nonzero(counts >= 0)[0]
    if len(posed):
        if not np.isfinite(rec[posed, 1:14]).all():
            raise StageError("B", crop, int(posed[np.argmax(~np.isfinite(rec[posed, 1:14]).all(1))]), "count >= 0 with a non-finite score or pose")
        d2 = S._sq_errors(p3d[vid], p2d[vid], K, rec[posed, 2:11].reshape(-1, 3, 3), rec[posed, 11:14])
        with np.errstate(invalid="ignore"):
            lo, hi = (d2 <= thr2 * (1.0 - S.BAND)).sum(1), (d2 <= thr2 * (1.0 + S.BAND)).sum(1)
            sc = np.where(d2 <= thr2, 1.0 - d2 / thr2, 0.0).sum(1)
        stats["pairs"] += d2.size
        stats["undecided"] += int((hi - lo).sum())
        c = counts[posed]
        bad = np.nonzero((c < lo) | (c > hi))[0]
        if len(bad):
            raise StageError("B", crop, int(posed[bad[0]]), "count %d, but %d..%d valid points lie within thr under the recorded pose"
                             % (c[bad[0]], lo[bad[0]], hi[bad[0]]))
        bad = np.nonzero(~(np.abs(rec[posed, 1] - sc) <= SCORE_RTOL * np.abs(sc)))[0]
        if len(bad):
            raise StageError("B", crop, int(posed[bad[0]]), "score %.17g, numpy's under the recorded pose %.17g" % (rec[posed[bad[0]], 1], sc[bad[0]]))

    # ---- C: the winner
    if inliers.shape != (N,) or (inliers & ~valid).any():
        raise StageError("C", crop, None, "inliers outside the valid column")
    cand = np.nonzero(counts >= 4)[0]
    if not len(cand):
        if not np.isnan(steps).all():
            raise StageError("C", crop, None, "a step ran without a record of count >= 4")
        identity_expected("C", "no hypothesis with 4 inliers")
        return stats
    win = int(cand[np.argmax(rec[cand, 1])])                               # the first of the largest
    Pk, sP = rec[win, 2:14], rec[win, 1]
    k, final = 0, None
    while True:
        st = steps[k]
        # C: this step ran, on the pose and score handed on
        if st[0] != k or not np.array_equal(st[1:13], Pk) or st[13] != sP:
            raise StageError("C", crop, win, "step %d does not start from the pose / score the decisions so far hand it (winner %d)" % (k, win))
        stats["steps"] += 1
        stats["sweeps"] = max(stats["sweeps"], int(st[29]))
        # D: capacities under the recorded pose
        want = cin_of(sq_errors(p3d, p2d, K, Pk[:9], Pk[9:]), valid, thr2)
        if ((cins[k] < 0) != (want < 0)).any() or np.abs(cins[k] - want).max() > 1:
            i = int(np.argmax(np.abs(cins[k] - want)))
            raise StageError("D", crop, win, "step %d: cin[%d] = %d, numpy's %d" % (k, i, cins[k, i], want[i]))
        # E: the labels are the canonical cut of the recorded capacities
        lab, _ = label(cins[k], offsets, indices, w)
        if not np.array_equal(labs[k].astype(bool), lab) or labs[k].max() > 1:
            diff = np.nonzero(labs[k].astype(bool) != lab)[0]
            raise StageError("E", crop, win, "step %d: labels (%d) differ from the canonical cut (%d) at %r" % (k, (labs[k] == 1).sum(), lab.sum(), diff[:8].tolist()))
        if st[14] != lab.sum():
            raise StageError("E", crop, win, "step %d: |L| recorded %r, labels hold %d" % (k, st[14], lab.sum()))
        if lab.sum() < min_inliers:
            if not np.isnan(st[15:29]).all():
                raise StageError("C", crop, win, "step %d: a refit over %d < min_inliers labels" % (k, lab.sum()))
            final = None
            break
        final = (Pk, lab)
        if k == LO_MAX:
            if not np.isnan(st[15:29]).all():
                raise StageError("C", crop, win, "a refit in the last step")
            break
        # F: the refit over the device's list
        sel = np.nonzero(lab)[0]
        fits = [rt for rt in (S._oracle_epnp(p3d[sel], p2d[sel], K, None, sg) for sg in S.AXIS_SIGNS) if rt is not None]
        if st[15] not in (0.0, 1.0):
            raise StageError("C", crop, win, "step %d: refit flag %r" % (k, st[15]))
        if st[15] == 0.0:
            if fits:
                raise StageError("F", crop, win, "step %d: refit failed over %d labels, the oracle's epnp solves them" % (k, len(sel)))
            if not np.isnan(st[16:29]).all():
                raise StageError("C", crop, win, "step %d: a failed refit left a pose" % k)
            break
        Qk, sQ = st[16:28], st[28]
        if not fits:
            raise StageError("F", crop, win, "step %d: a refit where the oracle's epnp is degenerate (%d labels)" % (k, len(sel)))
        tau_R, tau_t = S.taus()
        dR, dt = min(((np.abs(Qk[:9].reshape(3, 3) - rt[0]).max(), np.linalg.norm(Qk[9:] - rt[1]) / np.linalg.norm(rt[1])) for rt in fits),
                     key=lambda d: max(d[0] / tau_R, d[1] / tau_t))
        stats["refit_1e15"] = max(stats.get("refit_1e15", 0), int(1e15 * max(dR, dt)))
        if not (dR <= tau_R and dt <= tau_t):
            raise StageError("F", crop, win, "step %d: refit over %d labels off the oracle's: |dR| = %.3e (tau %.3e), |dt|/|t| = %.3e (tau %.3e)"
                             % (k, len(sel), dR, tau_R, dt, tau_t))
        # B again: the refit's score under the recorded pose
        sc = msac(sq_errors(p3d[vid], p2d[vid], K, Qk[:9], Qk[9:]), thr2)[1]
        if not abs(sQ - sc) <= SCORE_RTOL * abs(sc):
            raise StageError("B", crop, win, "step %d: score(Q) %.17g, numpy's under the recorded pose %.17g" % (k, sQ, sc))
        if not sQ > sP:
            break
        Pk, sP, k = Qk, sQ, k + 1
    if not np.isnan(steps[k + 1:]).all():
        raise StageError("C", crop, win, "steps ran behind step %d, where the decisions end" % k)
    if final is None:
        identity_expected("C", "fewer than min_inliers labels in step %d" % k)
    elif status != 1 or not np.array_equal(R.reshape(9), final[0][:9]) or not np.array_equal(t, final[0][9:]) or not np.array_equal(inliers, final[1]):
        raise StageError("C", crop, win, "the returned pose / inliers / status %d are not those of step %d" % (status, k))

    # ---- G: known answers
    if truth is not None:
        Rt, tt, out = np.asarray(truth[0], np.float64), np.asarray(truth[1], np.float64), np.asarray(truth[2]).astype(bool)
        stats["all_inlier"] = sum(1 for s in samples if not out[s].any())
        if stats["all_inlier"]:
            if status != 1 or not np.array_equal(inliers, valid & ~out):
                raise StageError("G", crop, win, "status %d, %d inliers; the crop has %d valid non-outliers" % (status, inliers.sum(), (valid & ~out).sum()))
            mR, mt = S.e_margins()
            dR, dt = np.abs(R - Rt).max(), np.linalg.norm(t - tt) / np.linalg.norm(tt)
            if not (dR <= mR and dt <= mt):
                raise StageError("G", crop, win, "pose off the true one by |dR| = %.3e (margin %.3e), |dt|/|t| = %.3e (%.3e)" % (dR, mR, dt, mt))
    return stats


# ---------------------------------------------------------------------------------------------------------------- the committed cases
RADIUS = 20.0


class GcCase:
    """a pnp_stages.Case + the solver's own parameters and the graphs: graphs[m] = (offsets, indices) of object m, graph_ids (B,) or None"""

    def __init__(self, case, lam=0.1, min_inliers=6, iterations=400):
        self.case, self.lam, self.min_inliers = case, lam, min_inliers
        case.iterations = iterations
        models = case.p3d if case.p3d.ndim == 3 else case.p3d[None]
        self.models = models
        self.graph_ids = np.arange(case.B, dtype=np.int32) if case.p3d.ndim == 3 else None
        self.graphs = [radius_graph_np(m, RADIUS) for m in models]
        self.name, self.B, self.N = case.name, case.B, case.N

    def graph(self, b):
        return self.graphs[b if self.graph_ids is not None else 0]

    def assert_well_posed(self):
        """every sample any hypothesis of this case can draw is well posed for the oracle (`well_posed`)"""
        for b in range(self.B):
            p3, p2, va, K = self.case.crop(b)
            vid = np.nonzero(va)[0]
            if len(vid) < self.min_inliers:
                continue
            for h in range(self.case.iterations):
                smp = vid[P.sample_indices(self.case.seed, b, h, len(vid), 4)]
                assert well_posed(p3, p2, K, smp), (self.name, b, h, "ill-posed four-point sample: choose another seed")

    def assert_unary_decides(self):
        """stage G's premise, under the true pose of every crop that carries a truth"""
        w = weight(self.lam)
        thr2 = float(np.float32(self.case.thr)) ** 2
        for b in range(self.B):
            if self.case.truth[b] is None:
                continue
            p3, p2, va, K = self.case.crop(b)
            Rt, tt, out = self.case.truth[b]
            off, idx = self.graph(b)
            cin = cin_of(sq_errors(p3, p2, K, Rt, tt), va, thr2)
            deg = np.diff(off)
            rows = np.repeat(np.arange(self.N), deg)
            deg_out = np.bincount(rows, weights=(va & out)[idx], minlength=self.N)
            o, i = va & out, va & ~out
            assert (cin[o] - Q > w * deg[o]).all(), (self.name, b, "an outlier's unary term does not outweigh its edges")
            assert (Q - cin[i] > w * deg_out[i]).all(), (self.name, b, "a non-outlier's unary term does not outweigh its edges to outliers")


def _lm_models():
    """two LM objects whose radius-20 graphs are light at N = 4096 (297 670 and 231 270 directed edges), one model per crop"""
    tab = np.load(os.path.join(S.DATA, "fps_lm_15x4096.npy"))
    return tab[[7, 12]].astype(np.float32).astype(np.float64)


def _columns(column, seed=41):
    """pnp_stages._columns with a seed of its own (that one's seed 40 holds two ill-posed samples)"""
    rng = np.random.default_rng(seed)
    xyz = S.lmo_model(512)
    crops = [S._crop(rng, xyz, S.K_LMO, 0.3, 0.0, 1.0) for _ in range(3)]
    valid = np.stack([rng.random((3, 512)) < f for f in (0.9, 0.6, 0.3)], 2)            # three different masks with real content
    return S.Case("column_%d" % column, xyz, np.stack([c[0] for c in crops]), valid, column=column, truth=[c[2] for c in crops], seed=seed)


def _nv5():
    c = S._standard("nv_5", 21, 2, 33, 0.0, valid_frac=1.0)
    c.valid[:, 5:, :] = 0
    c.truth = [None, None]
    return c


# seeds: pnp_stages' own where the case passes assert_well_posed; per_crop_K (19 -> 119), outliers_0.3 (31 -> 131) and the columns
# (40 -> 41) hold one ill-posed sample each at that seed and take the next one tried
EXACT_LAM = 0.02          # noise-free cases: small enough for assert_unary_decides at the degrees of these models (up to 56 / 126)
EDGES = ("coplanar", "collinear", "identical", "random_p2d")
ITERATIONS = (1, 63, 64, 65, 400, 512)
CASES = {
    "shape_2x6": lambda: GcCase(S._standard("shape_2x6", 17, 2, 6, 0.0, valid_frac=1.0), EXACT_LAM),
    "shape_4x33": lambda: GcCase(S._standard("shape_4x33", 15, 4, 33, 0.2, valid_frac=0.9), EXACT_LAM),
    "shape_4x65": lambda: GcCase(S._standard("shape_4x65", 14, 4, 65, 0.2, valid_frac=0.9), EXACT_LAM),
    "shape_3x512": lambda: GcCase(S._standard("shape_3x512", 11, 3, 512), EXACT_LAM),
    "shape_2x4096_lm": lambda: GcCase(S._standard("shape_2x4096_lm", 12, 2, 4096, model=_lm_models()), 0.01),     # degrees up to 126
    "per_crop_K": lambda: GcCase(S._standard("per_crop_K", 119, 4, 512, K=S._per_crop_K(4)), EXACT_LAM),
    "outliers_0": lambda: GcCase(S._standard("outliers_0", 30, 3, 512, 0.0), EXACT_LAM),
    "outliers_0.3": lambda: GcCase(S._standard("outliers_0.3", 131, 3, 512, 0.3), EXACT_LAM),
    "outliers_0.6": lambda: GcCase(S._standard("outliers_0.6", 32, 3, 512, 0.6), EXACT_LAM),
    "thr_0.5": lambda: GcCase(S._standard("thr_0.5", 20, 3, 512, noise=(0.5, 0.5, 0.5), thr=0.5)),
    "thr_2": lambda: GcCase(S._standard("thr_2", 20, 3, 512, noise=(0.5, 0.5, 0.5), thr=2.0)),
    "thr_8": lambda: GcCase(S._standard("thr_8", 20, 3, 512, noise=(0.5, 0.5, 0.5), thr=8.0)),
    "noise_lam_0.02": lambda: GcCase(S._standard("noise_lam_0.02", 22, 3, 512, (0.3, 0.6, 0.0), noise=(0.5, 0.5, 0.5)), EXACT_LAM),
    "nv_5": lambda: GcCase(_nv5()),
}
for _it in ITERATIONS:      # crops alternate between 30 % and 60 % outliers, 0.5 px noise on the second pair
    CASES["iterations_%d" % _it] = lambda _it=_it: GcCase(S._standard("iterations_%d" % _it, 60, 4, 512, (0.3, 0.6), noise=(0.0, 0.0, 0.5, 0.5)),
                                                          EXACT_LAM, iterations=_it)
for _c in range(3):
    CASES["column_%d" % _c] = lambda _c=_c: GcCase(_columns(_c), EXACT_LAM)
EDGE_CASES = {"edge_" + k: (lambda k=k: GcCase(S._edge(k))) for k in EDGES}


# ---------------------------------------------------------------------------------------------------------------- hand-built labelling problems
def _csr(n, pairs):
    adj = np.zeros((n, n), bool)
    for i, j in pairs:
        adj[i, j] = adj[j, i] = True
    return np.concatenate([[0], np.cumsum(adj.sum(1))]).astype(np.int32), np.nonzero(adj)[1].astype(np.int32)


def _mixed_cin(rng, n):
    """60 % inlier-like (below Q), 30 % outlier-like (up to 6 Q), the rest close to the tie or not a node"""
    cin = np.where(rng.random(n) < 0.6, rng.integers(0, Q, n), rng.integers(Q, 6 * Q, n))
    tie = rng.random(n) < 0.05
    cin[tie] = Q + rng.integers(-2, 3, int(tie.sum()))
    cin[rng.random(n) < 0.05] = -1
    return cin.astype(np.int64)


def label_cases():
    """name -> (cin (B,N), offsets, indices, w): the inputs of cp_graphcut_label's tests"""
    rng = np.random.default_rng(170)
    out = {}
    for n in (1, 6, 63, 64, 65):
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if rng.random() < 0.2]
        out["random_%d" % n] = (np.stack([_mixed_cin(rng, n), _mixed_cin(rng, n)]), *_csr(n, pairs), weight(0.1))
    out["no_edges"] = (_mixed_cin(rng, 64)[None], *_csr(64, []), weight(0.1))
    chain = _csr(65, [(i, i + 1) for i in range(64)])
    out["chain_lam1"] = (np.stack([np.where(np.arange(65) % 2, 3 * Q // 2, Q // 4), np.where(np.arange(65) < 30, 0, 3 * Q)]).astype(np.int64), *chain, weight(1.0))
    out["chain_lam0.1"] = (_mixed_cin(rng, 65)[None], *chain, weight(0.1))
    star = _csr(9, [(0, i) for i in range(1, 9)])
    cs = np.array([Q + Q // 2] + [0] * 8, np.int64)
    out["star_flipped"] = (cs[None], *star, weight(0.1))                 # 8 leaves x 0.1 Q > Q / 2: the centre joins them
    out["star_kept"] = (cs[None], *star, weight(0.05))
    two = _csr(12, [(i, j) for i in range(6) for j in range(i + 1, 6)] + [(i, j) for i in range(6, 12) for j in range(i + 1, 12)])
    out["two_components"] = (np.array([[0, 0, 0, 0, 0, 2 * Q, 3 * Q, 3 * Q, 3 * Q, 3 * Q, 3 * Q, Q // 2]], np.int64), *two, weight(0.3))
    g64 = _csr(64, [(i, j) for i in range(64) for j in range(i + 1, 64) if rng.random() < 0.15])
    out["all_inlier"] = (np.zeros((1, 64), np.int64), *g64, weight(0.1))
    out["all_outlier"] = (np.full((1, 64), 3 * Q, np.int64), *g64, weight(0.1))
    out["cin_equals_Q"] = (np.stack([np.full(64, Q), np.where(np.arange(64) % 3 == 0, Q, Q - 1)]).astype(np.int64), *g64, 0)
    out["lam_0"] = (_mixed_cin(rng, 64)[None], *g64, 0)
    out["lam_1"] = (_mixed_cin(rng, 64)[None], *g64, weight(1.0))
    pts = rng.uniform(0, 100, size=(4096, 3)).astype(np.float32)
    g4096 = radius_graph_np(pts, 7.8)                                   # mean degree ~8
    out["n4096_deg8"] = (_mixed_cin(rng, 4096)[None], *g4096, weight(0.1))
    ape = radius_graph_np(S.lmo_model(512), RADIUS)                     # degrees 23..56
    out["ape_512"] = (np.stack([_mixed_cin(rng, 512), _mixed_cin(rng, 512)]), *ape, weight(0.1))
    return out


def restatement_outputs(gc):
    """the restatement's own run of a case in the device's output layout"""
    out = []
    for b in range(gc.B):
        p3, p2, va, K = gc.case.crop(b)
        off, idx = gc.graph(b)
        out.append(solve_gc(p3, p2, va, K, off, idx, gc.case.thr, gc.lam, gc.case.iterations, gc.min_inliers, gc.case.seed, b))
    return out


def check_case(gc, stages, R, t, inliers, status, log=None):
    """check_crop on every crop + the undecided cap.  stages: dict of (B, ...) arrays"""
    gc.assert_unary_decides()
    total = {}
    for b in range(gc.B):
        p3, p2, va, K = gc.case.crop(b)
        off, idx = gc.graph(b)
        st = check_crop(p3, p2, va, K, off, idx, gc.case.thr, gc.lam, gc.case.iterations, gc.min_inliers, gc.case.seed, b,
                        {k: np.asarray(v[b]) for k, v in stages.items()}, R[b], np.asarray(t[b]).reshape(3), inliers[b], int(status[b]),
                        truth=gc.case.truth[b])
        for k, v in st.items():
            total[k] = max(total.get(k, 0), v) if k in ("refit_1e15", "sweeps") else total.get(k, 0) + v
    total["status1"] = int(np.asarray(status).sum())
    if log is not None:
        log("%-18s %s" % (gc.name, " ".join("%s=%d" % kv for kv in sorted(total.items()))))
    assert total["undecided"] <= S.UNDECIDED_CAP * max(total["pairs"], 1), (gc.name, total)
    assert 16 * total["sweeps"] <= MAX_SWEEPS, (gc.name, total)
    return total


if __name__ == "__main__":
    import time
    worst = 0
    for name in (sys.argv[1:] or CASES):
        t0 = time.time()
        gc = CASES[name]()
        outs = restatement_outputs(gc)
        sw = 0
        for b, o in enumerate(outs):
            off, idx = gc.graph(b)
            for k in range(LO_MAX + 1):
                if o[4]["cin"][k, 0] == -2 and (o[4]["cin"][k] == -2).all():
                    continue
                lab, fv, n = count_sweeps(o[4]["cin"][k], off, idx, weight(gc.lam))
                assert np.array_equal(lab, o[4]["labels"][k].astype(bool)), (name, b, k)
                sw = max(sw, n)
        worst = max(worst, sw)
        print("%-18s status %s  steps %s  sweeps %d  (%.1f s)" % (name, [o[3] for o in outs], [int(np.nansum(~np.isnan(o[4]["steps"][:, 0]))) for o in outs],
                                                                 sw, time.time() - t0), flush=True)
    print("largest sweep count: %d (bound %d)" % (worst, MAX_SWEEPS))
