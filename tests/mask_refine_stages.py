"""TEST INFRASTRUCTURE (not collected): cp_mask_extents / cp_contour_samples / cp_mask_refine (row N30) checked one iteration at a time by
replaying the device's own records.

THE RULE (csrc/mask_refine.hip states it; `extents`, `contour_from_depth`, `associate`, `refine` below are its numpy restatement).  All
in float64 after the render.  fx, fy, cx, cy = K[0,0], K[1,1], K[0,2], K[1,2].
Mask extents   row[y] = (first, last) set column of row y, col[x] = (first, last) set row of column x, (-1, -1) where there is none.
Stage A, contour samples of a pose (one render D at the INPUT pose; the render is tests/vsd_stages.py's rule)
  lattice     row N24's (icp_stages.lattice): rect = the pose's vertex rectangle intersected with the frame, w x h pixels from (x0, y0);
              nx = min(grid, w), ny = min(grid, h); lattice column i is pixel x0 + ((2 i + 1) w) // (2 nx), rows likewise; S = 4 grid slots
  slots       lattice row j at frame row y: slot 2 j = the first covered pixel (D > 0) of row y, slot 2 j + 1 the last; lattice column i at
              frame column x: slot 2 grid + 2 i = the topmost covered pixel of column x, 2 grid + 2 i + 1 the bottommost
  empty       (pixel -1 -1, depth 0, X NaN) when the line holds no covered pixel, or the pixel lies on the frame's first / last column
              (row kinds) or first / last row (column kinds)
  sample      pixel (x, y), d = D[y, x] (float32); Qr = (((x + 0.5 - cx) d) / fx, ((y + 0.5 - cy) d) / fy, d); X = R^T (Qr - t)
Stage B, association under (R, t)
  Y = R X, C = Y + t, reject unless C_z > 0; a_u = (fx C_x) / C_z, u = a_u + cx, a_v = (fy C_y) / C_z, v = a_v + cy; pixel (floor u,
  floor v), reject outside the frame; row kinds: m = row[mask][py][kind], reject when m < 0 or m is the frame's first / last column,
  b = m + 0.5, r = u - b, g = (fx / C_z, 0, -(a_u / C_z)); column kinds: col[mask][px][kind], the frame's first / last row, r = v - b,
  g = (0, fy / C_z, -(a_v / C_z)); reject unless |r| <= max_dist; (axis, b) frozen until the next association; n = the pairs
Stage C, LM over the pairs: d = (w, v): R' = exp([w]x) R, t' = t + v; J_i = [(Y_i x g_i)^T, g_i^T]; H = sum J^T J, g = sum J^T r,
  c = sum r^2; lambda = 1e-3.  At most max_iters times: 1 solve (H + lambda diag H) d = -g by Cholesky -- dof "t": the rotation block is
  the identity, its coupling and gradient zero, w = 0 and R' BITWISE R; 2 no factor: rejected, c' = +inf, the trial NaN; 3 else c' over
  the SAME pairs, a C_z <= 0 or a value that is not finite counts as +inf; 4 accept iff c' < c: the state becomes the trial,
  lambda = max(lambda / 10, 1e-12), stage B again; 5 n < min_pairs then stops with status 3; 6 else lambda *= 10, lambda > 1e8 stops with
  status 3; 7 an ACCEPTED step with s = max(|w|_inf, |v|_inf / |t|) <= step_tol stops with status 1; 8 iterations out: status 2.
  pass-through (status 0, pose bitwise the input, info NaN but for the counts): status_in == 0, a pose or K entry not finite, a mesh or
  mask id out of range, no render, fewer than min_pairs pairs under the input pose.
  records     18 doubles per executed iteration: [lambda, n, c, c', accepted, s, R' (9), t' (3)]
  info        42 doubles: [c0, c, samples, n0, n, iterations, H (36)]

`check_case` replays one case and raises pnp_stages.StageError (stage, pose, iteration in the message):
  N  stage A          pixel and depth EQUAL the restatement's from the render the caller hands over; X to 1e-12 relative
  P  pass-through     expected exactly where the rule says; then pose bitwise, no records, info NaN but for the counts
  n  pairs            n equals the restatement's count exactly (the association runs on the device's own X and recorded poses: the same
                      IEEE operations in the same order, so no tie margin is needed)
  L  lambda           reproduced EXACTLY from the accept flags
  C  cost             c and c' equal numpy's at the replayed state / over the state's pairs at the recorded trial pose to 1e-9 relative
  T  trial pose       numpy's trial from the replayed state within taus() (|dR|_max, |dt| / |t|); dof "t": R' bitwise the state's R
  A  accept flag      accepted == (c' < c) on the device's own two numbers
  E  stop and status  follow from the device's own s, lambda, n and iteration count; nothing recorded after the stop
  R  returned pose    bitwise the last accepted trial (or the input pose)
  I  info             cost0, the counts and the iterations exactly; cost and H to 1e-9 relative

ROUTE.  The replay takes the tolerance route of tests/test_gpu_lm_refine.py, not the bit-for-bit one: lm_solve_step calls sin and sqrt,
whose device and libm roundings are not pinned against each other.  MEASURED_TAU is the largest difference, over every executed
iteration of every committed case free-running on a CPU, between the restatement's trial pose with numpy's sums and with the kernel's
summation order (`kernel_sum`: lm_stages.kernel_sum's scheme over the SLOTS, an empty slot adding zero); taus() = 16 x that, capped at
pnp_stages.TAU_CAP.  It is measured on the restatement, never on the kernel.  `python -m tests.mask_refine_stages` prints it, the
table of DESIGN.md and the bound of the shifted-mask cases."""
import math
import sys

import numpy as np

from tests import icp_stages as I
from tests import lm_stages as L
from tests import pnp_stages as S
from tests import vsd_stages as V
from tests.pnp_stages import StageError

REC, INFO, MAX_ITERS, THREADS = 18, 42, 64, 256
LAMBDA0, LAMBDA_MIN, LAMBDA_STOP = 1e-3, 1e-12, 1e8
COST_RTOL, SAMPLE_RTOL = 1e-9, 1e-12
SIZE_A, SIZE_B = (96, 80), (70, 50)                # (W, H): 3 x 3 tiles; 3 x 2 tiles and a partial last word (70 = 2 * 32 + 6)
MEASURED_TAU = (4.5e-16, 3.4e-16)                  # seen: 4.441e-16, 3.312e-16; printed by `python -m tests.mask_refine_stages`; asserted in tests/test_mask_refine.py
SHIFT_BOUND = 0.008                                # seen: 0.0070 (shift_t_g64 pose 0): |t - the shifted truth| / Z with dof "t" 

numpy_sum = L.numpy_sum
kernel_sum = L.kernel_sum                          # thread i holds slot i; shuffle tree per wave; wave 0 + 1 + 2 + 3

K_A, K_B = I.K_A, I.K_B
K_C = np.array([[90.0, 0.0, 34.6], [0.0, 88.0, 25.3], [0.0, 0.0, 1.0]])      # the (70, 50) frame's camera

TAMPERINGS = ("no_border", "no_half", "right_first", "swap_axes", "no_gate", "no_reassoc", "ignore_mask_ids", "t_moves_R")
# the committed case that catches each tampering (tests/test_mask_refine.py::test_tampering_is_caught)
TAMPER_CASE = {"no_border": "edges_96", "no_half": "near_rt_g64", "right_first": "near_rt_g64", "swap_axes": "near_rt_g64", "no_gate": "masks_70",
               "no_reassoc": "near_rt_g64", "ignore_mask_ids": "near_t_g5", "t_moves_R": "near_t_g5"}


def taus():
    return min(16 * MEASURED_TAU[0], S.TAU_CAP[0]), min(16 * MEASURED_TAU[1], S.TAU_CAP[1])


# --------------------------------------------------------------------------------------------------------------- mask extents
def extents(mask):
    """mask (H, W) bool -> row (H, 2), col (W, 2) int32: (first, last) set column / row, (-1, -1) where there is none"""
    m = np.asarray(mask, bool)
    H, W = m.shape
    xs, ys = np.arange(W), np.arange(H)
    row = np.stack([np.where(m.any(1), np.where(m, xs[None, :], W).min(1), -1), np.where(m, xs[None, :], -1).max(1)], 1)
    col = np.stack([np.where(m.any(0), np.where(m, ys[:, None], H).min(0), -1), np.where(m, ys[:, None], -1).max(0)], 1)
    return row.astype(np.int32), col.astype(np.int32)


def pack_bits(masks, dirty=False):
    """masks (N, H, W) bool -> (N, H, ceil(W / 32)) int32 in cp_coco_pack's layout; dirty: the bits beyond W of the last word are SET
    (the extents must ignore them)"""
    m = np.asarray(masks, bool)
    N, H, W = m.shape
    WW = (W + 31) // 32
    pad = np.zeros((N, H, WW * 32), bool)
    pad[:, :, :W] = m
    pad[:, :, W:] = dirty
    w = (pad.reshape(N, H, WW, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return w.view(np.int32)


# ------------------------------------------------------------------------------------------------------------------- stage A
def contour_from_depth(D, rect, size, grid, K, R, t, tamper=()):
    """stage A from a render D (H, W) float32 and the pose's vertex rectangle (None: no render)
    -> dict(rect (4,), shape (2,), pixel (S,2), depth (S,) float32, X (S,3), ok)"""
    W, H = size
    S_ = 4 * grid
    pixel, depth, X = np.full((S_, 2), -1, np.int64), np.zeros(S_, np.float32), np.full((S_, 3), np.nan)
    lat = None if rect is None else I.lattice(rect, size, grid)
    out = dict(rect=np.array([-1] * 4 if lat is None else [lat[0], lat[1], lat[0] + lat[2] - 1, lat[1] + lat[3] - 1]),
               shape=np.array([0, 0] if lat is None else [lat[4], lat[5]]), pixel=pixel, depth=depth, X=X, ok=int(rect is not None))
    if lat is None:
        return out
    x0, y0, w, h, nx, ny = lat
    cov = np.asarray(D) > 0
    border = "no_border" not in tamper
    for j, y in enumerate(I.lattice_axis(y0, h, ny)):
        xs = np.nonzero(cov[y])[0]
        for side, x in enumerate((xs[:1], xs[-1:])):
            if len(x) and not (border and (x[0] == 0 or x[0] == W - 1)):
                pixel[2 * j + side] = x[0], y
    for i, x in enumerate(I.lattice_axis(x0, w, nx)):
        ys = np.nonzero(cov[:, x])[0]
        for side, y in enumerate((ys[:1], ys[-1:])):
            if len(y) and not (border and (y[0] == 0 or y[0] == H - 1)):
                pixel[2 * grid + 2 * i + side] = x, y[0]
    k = np.nonzero(pixel[:, 0] >= 0)[0]
    depth[k] = np.asarray(D, np.float32)[pixel[k, 1], pixel[k, 0]]
    X[k] = sample_points(pixel[k], depth[k], K, R, t)
    return out


def sample_points(pixel, depth, K, R, t):
    K, R, t = np.asarray(K, np.float64), np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    d = np.asarray(depth, np.float32).astype(np.float64)
    px, py = np.asarray(pixel)[:, 0].astype(np.float64), np.asarray(pixel)[:, 1].astype(np.float64)
    Q = np.stack([((px + 0.5 - cx) * d) / fx, ((py + 0.5 - cy) * d) / fy, d], 1)
    e = Q - t
    return np.stack([(R[0, j] * e[:, 0] + R[1, j] * e[:, 1]) + R[2, j] * e[:, 2] for j in range(3)], 1)


_RENDERS = {}


def render(mesh, R, t, K, size):
    """tests/vsd_stages.py's float32 render of a named mesh (cached by its arguments' bytes; read-only)"""
    key = (mesh, np.asarray(R, np.float64).tobytes(), np.asarray(t, np.float64).tobytes(), np.asarray(K, np.float64).tobytes(), size)
    if key not in _RENDERS:
        v, f = V.meshes()[mesh]
        d = V.render_f32(R, t, K, v, f, size)
        d.setflags(write=False)
        _RENDERS[key] = d
    return _RENDERS[key]


def free_samples(mesh, R, t, K, size, grid, tamper=()):
    """stage A free-running on a CPU for ONE pose of a named mesh (None: a mesh id out of range) -> (contour_from_depth's dict, D)"""
    W, H = size
    D0 = np.zeros((H, W), np.float32)
    if mesh is None or not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(K).all()):
        return contour_from_depth(D0, None, size, grid, K, R, t), D0
    rect = I.vertex_rect(R, t, K, V.meshes()[mesh][0], size)
    if rect is None:
        return contour_from_depth(D0, None, size, grid, K, R, t), D0
    D = render(mesh, R, t, K, size) if I.lattice(rect, size, grid) is not None else D0
    return contour_from_depth(D, rect, size, grid, K, R, t, tamper), D


# ------------------------------------------------------------------------------------------------------------ stages B and C
def associate(X, pixel, grid, K, R, t, row, col, size, max_dist, tamper=(), frozen=None):
    """stage B for every slot -> dict(pair (S,) bool, b (S,), Y (S,3), Cz, a, r (S,), column (S,) bool, n).  frozen: an earlier
    association whose (pair, b) are kept (the checker's own tampering "no_reassoc")"""
    K, R, t = np.asarray(K, np.float64), np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    W, H = size
    S_ = 4 * grid
    slot = np.arange(S_)
    column, far = slot >= 2 * grid, slot & 1
    if "swap_axes" in tamper:
        column = ~column
    live = np.asarray(pixel)[:, 0] >= 0
    Xs = np.where(live[:, None], X, 0.0)
    with np.errstate(all="ignore"):
        Y = np.stack([(R[i, 0] * Xs[:, 0] + R[i, 1] * Xs[:, 1]) + R[i, 2] * Xs[:, 2] for i in range(3)], 1)
        C = Y + t
        front = live & (C[:, 2] > 0.0)
        au, av = (fx * C[:, 0]) / C[:, 2], (fy * C[:, 1]) / C[:, 2]
        u, v = au + cx, av + cy
        inside = front & (u >= 0.0) & (u < W) & (v >= 0.0) & (v < H)
        px = np.clip(np.where(inside, np.floor(u), 0), 0, W - 1).astype(np.int64)
        py = np.clip(np.where(inside, np.floor(v), 0), 0, H - 1).astype(np.int64)
        side = np.zeros_like(far) if "right_first" in tamper else far
        line_c, line_r = np.clip(px, 0, len(col) - 1), np.clip(py, 0, len(row) - 1)
        m = np.where(column, np.asarray(col)[line_c, side], np.asarray(row)[line_r, side]).astype(np.int64)
        lim = np.where(column, H - 1, W - 1)
        have = inside & (m >= 0)
        if "no_border" not in tamper:
            have &= (m != 0) & (m != lim)
        b = m.astype(np.float64) + (0.0 if "no_half" in tamper else 0.5)
        wv = np.where(column, v, u)
        if frozen is not None:
            b = frozen["b"]
        r = wv - b
        pair = have & (np.abs(r) <= max_dist) if "no_gate" not in tamper else have
        if frozen is not None:
            pair = frozen["pair"]
        a = np.where(column, av, au)
    return dict(pair=pair, b=b, Y=Y, Cz=C[:, 2], a=a, r=r, column=column, n=int(pair.sum()), f=np.where(column, fy, fx))


def pair_terms(a):
    """-> T (S, 29): per slot the 21 upper-triangle entries of J^T J row by row, the 6 of J^T r, r^2, 1; zero rows where there is no pair"""
    Y, r, column = a["Y"], a["r"], a["column"]
    with np.errstate(all="ignore"):
        ga, g2 = a["f"] / a["Cz"], -(a["a"] / a["Cz"])
        g0, g1 = np.where(column, 0.0, ga), np.where(column, ga, 0.0)
        J = [Y[:, 1] * g2 - Y[:, 2] * g1, Y[:, 2] * g0 - Y[:, 0] * g2, Y[:, 0] * g1 - Y[:, 1] * g0, g0, g1, g2]
        cols = [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * r for i in range(6)] + [r * r, np.ones_like(r)]
    T = np.stack(cols, 1)
    return np.where(a["pair"][:, None], T, 0.0)


def trial_cost(a, X, K, Rn, tn, sums=numpy_sum):
    """c' of (Rn, tn) over the pairs of association `a` ((axis, b) fixed); +inf when a pair lies behind the camera or c' is not finite"""
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    Xs = np.where(a["pair"][:, None], X, 0.0)
    with np.errstate(all="ignore"):
        C = np.stack([((Rn[i, 0] * Xs[:, 0] + Rn[i, 1] * Xs[:, 1]) + Rn[i, 2] * Xs[:, 2]) + tn[i] for i in range(3)], 1)
        w = np.where(a["column"], (fy * C[:, 1]) / C[:, 2] + cy, (fx * C[:, 0]) / C[:, 2] + cx)
        r = w - a["b"]
        term = np.where(C[:, 2] > 0.0, r * r, np.inf)
        c = float(sums(np.where(a["pair"], term, 0.0)[:, None])[0])
    return c if math.isfinite(c) else float("inf")


def trial(sums, R, t, lam, dof, tamper=()):
    """the trial step of csrc/mask_refine.hip -> (pd, d, R', t', s)"""
    Lm = L.load_lower(sums)
    g = [float(x) for x in sums[21:27]]
    t_only = dof == "t" and "t_moves_R" not in tamper
    if t_only:
        for q in range(6):
            for r_ in range(3):
                Lm[q][r_] = 1.0 if q == r_ else 0.0
        g[:3] = [0.0, 0.0, 0.0]
    for q in range(3 if t_only else 0, 6):
        Lm[q][q] = Lm[q][q] + lam * Lm[q][q]
    pd, d, Rn, tn, s = L.solve_step(Lm, g, np.asarray(R, np.float64).reshape(3, 3), t)
    if pd and t_only:
        d = d.copy()
        d[:3] = 0.0
        Rn = np.array(R, np.float64).reshape(3, 3).copy()
    return pd, d, Rn, tn, s


def passes_before_pairs(K, R, t, status_in, ok, row):
    return status_in == 0 or row is None or not ok or not (np.isfinite(K).all() and np.isfinite(R).all() and np.isfinite(t).all())


def refine(X, pixel, ok, grid, K, R, t, row, col, size, max_dist, dof, status_in=1, max_iters=20, step_tol=1e-6, min_pairs=6, sums=numpy_sum,
           tamper=()):
    """stages B and C on one pose (row / col None: a mask id out of range) -> dict(R, t, status, info (42,), records (max_iters, 18))"""
    K, R, t = np.asarray(K, np.float64), np.array(R, np.float64), np.array(t, np.float64).reshape(3)
    rec = np.full((max_iters, REC), np.nan)
    info = np.full(INFO, np.nan)
    info[2:6] = int((np.asarray(pixel)[:, 0] >= 0).sum()), 0, 0, 0
    if passes_before_pairs(K, R, t, status_in, ok, row):
        return dict(R=R, t=t, status=0, info=info, records=rec)
    args = (X, pixel, grid, K)
    a = associate(*args, R, t, row, col, size, max_dist, tamper)
    info[3] = info[4] = a["n"]
    if a["n"] < min_pairs:
        return dict(R=R, t=t, status=0, info=info, records=rec)
    state = sums(pair_terms(a))
    c = c0 = float(state[27])
    n0 = a["n"]
    lam, status, iters = LAMBDA0, 2, 0
    for it in range(max_iters):
        pd, d, Rn, tn, s = trial(state, R, t, lam, dof, tamper)
        cn = trial_cost(a, X, K, Rn, tn, sums) if pd else float("inf")
        accept = cn < c
        rec[it, :6] = lam, a["n"], c, cn, 1.0 if accept else 0.0, s
        rec[it, 6:15], rec[it, 15:18] = Rn.reshape(9), tn
        iters = it + 1
        if accept:
            R, t = Rn, tn
            lam = max(lam / 10.0, LAMBDA_MIN)
            a = associate(*args, R, t, row, col, size, max_dist, tamper, frozen=a if "no_reassoc" in tamper else None)
            state = sums(pair_terms(a))
            c = float(state[27])
            if a["n"] < min_pairs:
                status = 3
                break
            if s <= step_tol:
                status = 1
                break
        else:
            lam = lam * 10.0
            if lam > LAMBDA_STOP:
                status = 3
                break
    info[0], info[1], info[3], info[4], info[5] = c0, c, n0, a["n"], iters
    info[6:] = L.unpack_H(state).reshape(36)
    return dict(R=R, t=t, status=status, info=info, records=rec)


# ------------------------------------------------------------------------------------------------------------------ the checker
def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def _bits(a):
    return np.asarray(a, np.float64).reshape(-1).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def check_samples(smp, D, size, grid, K, R, t, pose):
    """stage N: the pose's slots against the restatement from the render D and the device's own rectangle"""
    rect = None if not smp["ok"] or smp["rect"][0] < 0 else tuple(int(x) for x in smp["rect"])
    if not smp["ok"] or rect is None:
        if (np.asarray(smp["pixel"]) >= 0).any():
            raise StageError("N", pose, None, "samples of a pose that has no render or no rectangle in the frame")
        return
    want = contour_from_depth(D, rect, size, grid, K, R, t)
    if not np.array_equal(want["pixel"], np.asarray(smp["pixel"])):
        raise StageError("N", pose, None, "the slots' pixels differ from the restatement's in %d slots" % int((want["pixel"] != np.asarray(smp["pixel"])).any(1).sum()))
    if not np.array_equal(want["depth"].view(np.uint32), np.asarray(smp["depth"], np.float32).view(np.uint32)):
        raise StageError("N", pose, None, "a slot's depth is not bitwise the render's")
    k = want["pixel"][:, 0] >= 0
    if not np.isnan(np.asarray(smp["X"])[~k]).all():
        raise StageError("N", pose, None, "an empty slot holds a point")
    if k.any():
        dX = np.abs(np.asarray(smp["X"])[k] - want["X"][k]).max(1) / np.maximum(np.abs(want["X"][k]).max(1), 1.0)
        if not dX.max() <= SAMPLE_RTOL:
            raise StageError("N", pose, None, "X off the restatement's by %.3e (relative)" % dX.max())


def check_pose(smp, grid, K, R_in, t_in, row, col, size, max_dist, dof, status_in, max_iters, step_tol, min_pairs, pose, records, R_out, t_out,
               status, info, D=None):
    """Raises StageError where the outputs of cp_mask_refine on one pose contradict its own records or the restatement.  smp: the
    pose's samples (rect, pixel, depth, X, ok: the values the device read); D: the pose's render, switches stage N on.  -> statistics"""
    K, R_in, t_in = np.asarray(K, np.float64), np.asarray(R_in, np.float64), np.asarray(t_in, np.float64).reshape(3)
    records, R_out, t_out, info = np.asarray(records, np.float64), np.asarray(R_out, np.float64), np.asarray(t_out, np.float64).reshape(3), np.asarray(info, np.float64)
    X, pixel = np.asarray(smp["X"], np.float64), np.asarray(smp["pixel"])
    status = int(status)
    stats = dict(iters=0, accepted=0, dR_1e18=0, dt_1e18=0, passed=0)
    if records.shape != (max_iters, REC) or info.shape != (INFO,):
        raise StageError("P", pose, None, "records / info have shapes %r / %r" % (records.shape, info.shape))
    if D is not None and np.isfinite(K).all() and np.isfinite(R_in).all() and np.isfinite(t_in).all():
        check_samples(smp, D, size, grid, K, R_in, t_in, pose)
    n_samples = int((pixel[:, 0] >= 0).sum())

    def assoc(R, t):
        return associate(X, pixel, grid, K, R, t, row, col, size, max_dist)

    def passed(n0):
        if status != 0:
            raise StageError("P", pose, None, "the rule passes this pose through (%d samples, %d pairs, status_in %r), got status %d" % (n_samples, n0, status_in, status))
        if not (_same(R_out, R_in) and _same(t_out, t_in)):
            raise StageError("P", pose, None, "pass-through, but the returned pose is not bitwise the input pose")
        if not np.isnan(records).all():
            raise StageError("P", pose, None, "pass-through, but records were written")
        if not (info[2] == n_samples and info[3] == n0 and info[4] == n0 and info[5] == 0 and np.isnan(info[:2]).all() and np.isnan(info[6:]).all()):
            raise StageError("P", pose, None, "pass-through: info is not [NaN, NaN, %d, %d, %d, 0, NaN ...]: %r" % (n_samples, n0, n0, info[:6].tolist()))
        stats["passed"] = 1
        return stats

    if passes_before_pairs(K, R_in, t_in, status_in, smp["ok"], row):
        return passed(0)
    a = assoc(R_in, t_in)
    if a["n"] < min_pairs:
        return passed(a["n"])
    if status == 0:
        raise StageError("P", pose, None, "status 0 on a pose the rule refines (%d pairs)" % a["n"])
    tau_R, tau_t = taus()
    R, t = R_in, t_in
    state = numpy_sum(pair_terms(a))
    n0 = a["n"]
    lam, last, want_status, iters = LAMBDA0, None, 2, 0
    for it in range(max_iters):
        rec = records[it]
        if np.isnan(rec).all():
            raise StageError("E", pose, it, "no record, but nothing recorded before stops the iteration")
        lam_d, n_d, c_d, cn_d, acc_d, s_d = rec[:6]
        Rn_d, tn_d = rec[6:15].reshape(3, 3), rec[15:18]
        if n_d != a["n"]:
            raise StageError("n", pose, it, "n = %r, the restatement pairs %d samples" % (n_d, a["n"]))
        if lam_d != lam:
            raise StageError("L", pose, it, "lambda %.17g, the flags give %.17g" % (lam_d, lam))
        if not (np.isfinite(c_d) and _rel(c_d, float(state[27])) <= COST_RTOL):
            raise StageError("C", pose, it, "c = %.17g, numpy at the replayed state: %.17g" % (c_d, float(state[27])))
        pd, d, Rn, tn, s = trial(state, R, t, lam, dof)
        if not pd:
            if not (np.isnan(rec[5:]).all() and cn_d == np.inf):
                raise StageError("T", pose, it, "numpy finds no Cholesky factor; the record holds a trial (c' = %r)" % cn_d)
        else:
            if not np.isfinite(rec[5:]).all():
                raise StageError("T", pose, it, "the trial pose or s is not finite, numpy's is")
            dR, dt = float(np.abs(Rn_d - Rn).max()), float(np.linalg.norm(tn_d - tn) / np.linalg.norm(t))
            stats["dR_1e18"], stats["dt_1e18"] = max(stats["dR_1e18"], int(1e18 * dR)), max(stats["dt_1e18"], int(1e18 * dt))
            if dof == "t" and not _same(Rn_d, R):
                raise StageError("T", pose, it, 'dof "t", but the trial rotation is not bitwise the state\'s')
            if not (dR <= tau_R and dt <= tau_t):
                raise StageError("T", pose, it, "trial pose off numpy's: |dR| = %.3e (tau %.3e), |dt|/|t| = %.3e (tau %.3e)" % (dR, tau_R, dt, tau_t))
            if not abs(s_d - s) <= max(tau_R, tau_t):
                raise StageError("T", pose, it, "s = %.17g, numpy's %.17g" % (s_d, s))
            cn = trial_cost(a, X, K, Rn_d, tn_d)
            if np.isinf(cn) != np.isinf(cn_d) or (np.isfinite(cn) and not _rel(cn_d, cn) <= COST_RTOL):
                raise StageError("C", pose, it, "c' = %.17g, numpy over the state's pairs at the recorded trial pose: %.17g" % (cn_d, cn))
        if acc_d not in (0.0, 1.0) or bool(acc_d) != bool(cn_d < c_d):
            raise StageError("A", pose, it, "accepted = %r with c' = %.17g, c = %.17g" % (acc_d, cn_d, c_d))
        iters = it + 1
        if acc_d:
            R, t, last = Rn_d.copy(), tn_d.copy(), (Rn_d.copy(), tn_d.copy())
            lam = max(lam / 10.0, LAMBDA_MIN)
            stats["accepted"] += 1
            a = assoc(R, t)
            state = numpy_sum(pair_terms(a))
            if a["n"] < min_pairs:
                want_status = 3
                break
            if s_d <= step_tol:
                want_status = 1
                break
        else:
            lam = lam * 10.0
            if lam > LAMBDA_STOP:
                want_status = 3
                break
    stats["iters"] = iters
    if not np.isnan(records[iters:]).all():
        raise StageError("E", pose, iters, "a record behind the stop (status %d after %d iterations by the device's own s, n and lambda)" % (want_status, iters))
    if status != want_status:
        raise StageError("E", pose, iters - 1, "status %d, the records end with %d" % (status, want_status))
    want = last if last is not None else (R_in, t_in)
    if not (_same(R_out, want[0]) and _same(t_out, want[1])):
        raise StageError("R", pose, None, "the returned pose is not bitwise the last accepted trial%s" % ("" if last is not None else " (none: the input pose)"))
    if dof == "t" and not _same(R_out, R_in):
        raise StageError("R", pose, None, 'dof "t", but the returned rotation is not bitwise the input\'s')
    if not (_same(info[0], records[0, 2]) and info[2] == n_samples and info[3] == n0 and info[4] == a["n"] and info[5] == iters):
        raise StageError("I", pose, None, "info = %r, the records say cost0 %.17g, %d samples, %d / %d pairs, %d iterations" % (info[:6].tolist(), records[0, 2], n_samples, n0, a["n"], iters))
    if not _rel(info[1], float(state[27])) <= COST_RTOL or (not records[iters - 1, 4] and not _same(info[1], records[iters - 1, 2])):
        raise StageError("I", pose, None, "cost = %.17g, numpy at the returned pose: %.17g" % (info[1], float(state[27])))
    H_d, H = info[6:].reshape(6, 6), L.unpack_H(state)
    scale = np.sqrt(np.outer(np.diag(H), np.diag(H))) + 1e-300
    if not (np.isfinite(H_d).all() and np.array_equal(H_d, H_d.T) and (np.abs(H_d - H) <= COST_RTOL * scale).all()):
        raise StageError("I", pose, None, "H off numpy's at the returned pose by %.3e of sqrt(H_ii H_jj)" % float(np.nanmax(np.abs(H_d - H) / scale)))
    return stats


# ------------------------------------------------------------------------------------------------------------- the committed cases
class MaskCase:
    """meshes: names into vsd_stages.meshes(); mesh_ids (P,) or None (an id outside the names: out of range); K (3,3) or (P,3,3);
    masks (NM,H,W) bool; mask_ids (P,) or None (mask p for pose p; an id outside 0..NM-1: out of range); truth: per pose (R, t) of the
    pose its mask was made from, or None; kind: per pose "self" / "near" / "shift" / "other"; shift: per pose (dx, dy) or None"""

    def __init__(self, name, size, meshes, mesh_ids, K, R0, t0, masks, mask_ids, truth, kind, shift, max_dist, dof, grid, max_iters=20, step_tol=1e-6,
                 min_pairs=6, status_in=None):
        self.name, self.size, self.meshes, self.mesh_ids, self.K, self.R0, self.t0 = name, size, tuple(meshes), mesh_ids, K, R0, t0
        self.masks, self.mask_ids, self.truth, self.kind, self.shift = masks, mask_ids, truth, kind, shift
        self.max_dist, self.dof, self.grid, self.max_iters, self.step_tol, self.min_pairs, self.status_in = max_dist, dof, grid, max_iters, step_tol, min_pairs, status_in
        self.P = len(R0)
        self._ext = [extents(m) for m in masks]

    def mesh_of(self, b):
        m = 0 if self.mesh_ids is None else int(self.mesh_ids[b])
        return self.meshes[m] if 0 <= m < len(self.meshes) else None

    def mask_of(self, b, tamper=()):
        m = b if self.mask_ids is None or "ignore_mask_ids" in tamper else int(self.mask_ids[b])
        if "ignore_mask_ids" in tamper:
            m = b % len(self.masks)
        return m if 0 <= m < len(self.masks) else None

    def extents_of(self, b, tamper=()):
        m = self.mask_of(b, tamper)
        return (None, None) if m is None else self._ext[m]

    def K_of(self, b):
        return self.K[b] if self.K.ndim == 3 else self.K

    def status_of(self, b):
        return 1 if self.status_in is None else int(self.status_in[b])


def _pose(rng, K, size, distance=(300.0, 360.0)):
    R = I._random_rotation(rng)
    z = rng.uniform(*distance)
    W, H = size
    return R, np.array([z * (W / 2 + rng.uniform(-6, 6) - K[0, 2]) / K[0, 0], z * (H / 2 + rng.uniform(-4, 4) - K[1, 2]) / K[1, 1], z])


def _near(rng, R, t, deg=3.0, side=0.01, ray=0.03):
    sg = lambda: 1.0 if rng.random() < 0.5 else -1.0      # noqa: E731
    return I._rodrigues(rng.normal(size=3), np.radians(deg)) @ R, t + t[2] * np.array([side * sg(), side * sg(), ray * sg()])


def _shifted(mask, dx, dy):
    out = np.zeros_like(mask)
    H, W = mask.shape
    out[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = mask[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    return out


def _build(name, seed, size, K, poses, masks_extra=(), mask_ids=None, per_pose_K=None, **kw):
    """poses: per pose (mesh name, kind, argument): "self" the truth itself; "near" a perturbed start; "shift" (dx, dy): the truth under
    a mask shifted by whole pixels.  Mask p is pose p's truth silhouette (shifted); masks_extra are appended."""
    rng = np.random.default_rng(seed)
    names = []
    for m, _, _ in poses:
        if m not in names:
            names.append(m)
    R0, t0, masks, truth, kind, shift, Ks = [], [], [], [], [], [], []
    for b, (m, kd, arg) in enumerate(poses):
        Kb = K if per_pose_K is None else per_pose_K[b % len(per_pose_K)]
        Ks.append(Kb)
        R, t = _pose(rng, Kb, size)
        sil = render(m, R, t, Kb, size) > 0
        truth.append((R, t))
        kind.append(kd)
        shift.append(arg if kd == "shift" else None)
        if kd == "near":
            Rs, ts = _near(rng, R, t)
        else:
            Rs, ts = R, t
        R0.append(Rs)
        t0.append(ts)
        masks.append(_shifted(sil, *arg) if kd == "shift" else sil)
    masks = np.stack(masks + list(masks_extra))
    mesh_ids = None if len(names) == 1 else np.array([names.index(m) for m, _, _ in poses], np.int32)
    return MaskCase(name, size, names, mesh_ids, K if per_pose_K is None else np.stack(Ks), np.stack(R0), np.stack(t0), masks, mask_ids, truth, kind, shift, **kw)


def _near_t_g5():
    """four poses over TWO masks: poses 2 and 3 start near the truths of poses 1 and 0 and read their masks (shared, permuted ids)"""
    c = _build("near_t_g5", 42, SIZE_A, K_A, [("torus", "near", None), ("box", "near", None)], max_dist=8.0, dof="t", grid=5)
    rng = np.random.default_rng(420)
    extra = [_near(rng, *c.truth[1]), _near(rng, *c.truth[0])]
    c.R0 = np.concatenate([c.R0, np.stack([e[0] for e in extra])])
    c.t0 = np.concatenate([c.t0, np.stack([e[1] for e in extra])])
    c.mesh_ids = np.array([0, 1, 1, 0], np.int32)
    c.mask_ids = np.array([0, 1, 1, 0], np.int32)
    c.truth, c.kind, c.shift, c.P = c.truth + [c.truth[1], c.truth[0]], c.kind + ["near", "near"], c.shift + [None, None], 4
    c.mask_ids = np.array([0, 1, 1, 0], np.int32)
    return c


def _edges():
    """0: the control; 1: partly outside the frame (its border samples are dropped); 2: wholly outside; 3: a vertex behind the camera;
    4: NaN in R; 5: status 0; 6: a mask id out of range; 7: a mesh id out of range"""
    c = _build("edges_96", 43, SIZE_A, K_A, [("torus", "near", None)] * 8, max_dist=8.0, dof="rt", grid=5)
    z = c.truth[1][1][2]
    R1 = c.truth[1][0]
    t1 = np.array([z * (SIZE_A[0] - 6.0 - K_A[0, 2]) / K_A[0, 0], c.truth[1][1][1], z])      # the centre six pixels inside the right edge
    c.masks[1] = render("torus", R1, t1, K_A, SIZE_A) > 0
    c._ext[1] = extents(c.masks[1])
    c.truth[1] = (R1, t1)
    c.R0[1], c.t0[1] = R1, t1 * np.array([1.0, 1.0, 1.03])
    c.kind = ["near", "other", "other", "other", "other", "other", "other", "other"]
    c.t0[2] = c.t0[2] + np.array([900.0, 0.0, 0.0])
    c.t0[3] = np.array([0.0, 0.0, 20.0])
    c.R0[4, 1, 2] = np.nan
    c.status_in = np.ones(8, np.int32)
    c.status_in[5] = 0
    c.mask_ids = np.arange(8, dtype=np.int32)
    c.mask_ids[6] = 8
    c.mesh_ids = np.zeros(8, np.int32)
    c.mesh_ids[7] = 1
    return c


def _masks_70():
    """five torus poses at ONE truth on the (70, 50) frame under: 0 the truth's silhouette, 1 an empty mask, 2 a full-frame mask (all its
    extents on the border: pass-through), 3 a one-pixel mask, 4 a checkerboard"""
    W, H = SIZE_B
    c = _build("masks_70", 44, SIZE_B, K_C, [("torus", "near", None)], max_dist=6.0, dof="rt", grid=5)
    sil = c.masks[0]
    one = np.zeros((H, W), bool)
    ys, xs = np.nonzero(sil)
    one[int(np.median(ys)), int(xs.min()) + 1] = True
    chk = (np.add.outer(np.arange(H), np.arange(W)) % 2 == 0)
    c.masks = np.stack([sil, np.zeros((H, W), bool), np.ones((H, W), bool), one, chk])
    c._ext = [extents(m) for m in c.masks]
    c.R0, c.t0 = np.repeat(c.R0, 5, 0), np.repeat(c.t0, 5, 0)
    c.truth, c.kind, c.shift, c.P = c.truth * 5, ["near", "other", "other", "other", "other"], [None] * 5, 5
    return c


CASES = {
    "self_g5": lambda: _build("self_g5", 40, SIZE_A, K_A, [("torus", "self", None), ("box", "self", None), ("ico80", "self", None)], max_dist=8.0, dof="rt", grid=5),
    "near_rt_g64": lambda: _build("near_rt_g64", 41, SIZE_A, K_A, [("torus", "near", None), ("box", "near", None), ("ico80", "near", None)],
                                  per_pose_K=(K_A, K_B), max_dist=8.0, dof="rt", grid=64),
    "near_t_g5": _near_t_g5,
    "shift_t_g64": lambda: _build("shift_t_g64", 45, SIZE_B, K_C, [("torus", "shift", (2, -1)), ("box", "shift", (-3, 2)), ("ico80", "shift", (1, 1))],
                                  max_dist=6.0, dof="t", grid=64),
    "shift_t_g5": lambda: _build("shift_t_g5", 46, SIZE_A, K_A, [("torus", "shift", (-2, 3)), ("ico80", "shift", (4, 0))], max_dist=8.0, dof="t", grid=5),
    "near_g1": lambda: _build("near_g1", 47, SIZE_B, K_C, [("torus", "near", None), ("box", "near", None)], max_dist=6.0, dof="rt", grid=1),
    "near_it2": lambda: _build("near_it2", 41, SIZE_A, K_A, [("torus", "near", None), ("box", "near", None), ("ico80", "near", None)],
                               per_pose_K=(K_A, K_B), max_dist=8.0, dof="rt", grid=64, max_iters=2),
    "edges_96": _edges,
    "masks_70": _masks_70,
}
_CASES = {}


def make(name):
    if name not in _CASES:
        _CASES[name] = CASES[name]()
    return _CASES[name]


def case_samples(case, tamper=()):
    """stage A free-running for every pose of a case: (a list of per-pose dicts, a list of the renders)"""
    out = [free_samples(case.mesh_of(b), case.R0[b], case.t0[b], case.K_of(b), case.size, case.grid, tamper) for b in range(case.P)]
    return [o[0] for o in out], [o[1] for o in out]


def restatement_outputs(case, samples, sums=numpy_sum, tamper=()):
    """the restatement's own run of a case over `samples` in the device's output layout:
    (records (P,it,18), R (P,3,3), t (P,3), status (P,), info (P,42))"""
    outs = []
    for b in range(case.P):
        s = samples[b]
        row, col = case.extents_of(b, tamper)
        outs.append(refine(s["X"], s["pixel"], s["ok"], case.grid, case.K_of(b), case.R0[b], case.t0[b], row, col, case.size, case.max_dist, case.dof,
                           case.status_of(b), case.max_iters, case.step_tol, case.min_pairs, sums, tamper))
    return (np.stack([o["records"] for o in outs]), np.stack([o["R"] for o in outs]), np.stack([o["t"] for o in outs]),
            np.array([o["status"] for o in outs], np.int32), np.stack([o["info"] for o in outs]))


def check_case(case, samples, records, R, t, status, info, renders=None, log=None):
    """samples: a list of per-pose dicts (rect, pixel, depth, X, ok: what the device read); renders: per pose D, switches stage N on"""
    total = {}
    for b in range(case.P):
        row, col = case.extents_of(b)
        st = check_pose(samples[b], case.grid, case.K_of(b), case.R0[b], case.t0[b], row, col, case.size, case.max_dist, case.dof, case.status_of(b),
                        case.max_iters, case.step_tol, case.min_pairs, b, records[b], R[b], np.asarray(t[b]).reshape(3), int(status[b]), info[b],
                        D=None if renders is None else renders[b])
        for k, x in st.items():
            total[k] = max(total.get(k, 0), x) if k.endswith("_1e18") else total.get(k, 0) + x
    if log is not None:
        log("%-14s status %s %s" % (case.name, np.asarray(status).tolist()[:8], " ".join("%s=%d" % kv for kv in sorted(total.items()))))
    return total


def silhouette_iou(case, b, R, t):
    """IoU of pose b's render under (R, t) with its mask"""
    m = case.masks[case.mask_of(b)]
    sil = render(case.mesh_of(b), R, np.reshape(t, 3), case.K_of(b), case.size) > 0
    return float((sil & m).sum()) / max(float((sil | m).sum()), 1.0)


def shift_error(case, b, t):
    """|t - the translation that moves the truth's projection by the mask's whole-pixel shift| / Z, for a "shift" pose"""
    R, tt = case.truth[b]
    K = case.K_of(b)
    dx, dy = case.shift[b]
    want = tt + tt[2] * np.array([dx / K[0, 0], dy / K[1, 1], 0.0])
    return float(np.linalg.norm(np.reshape(t, 3) - want) / tt[2])


def measure_tau(case, samples, records):
    """largest (|dR|_max, |dt| / |t|) between the trial from numpy's sums and from the kernel-order sums of the same terms, over every
    executed iteration of the restatement's run of a case"""
    worst = [0.0, 0.0]
    for b in range(case.P):
        s = samples[b]
        row, col = case.extents_of(b)
        R, t = case.R0[b], case.t0[b]
        for rec in records[b]:
            if np.isnan(rec[0]):
                break
            T = pair_terms(associate(s["X"], s["pixel"], case.grid, case.K_of(b), R, t, row, col, case.size, case.max_dist))
            x, k = trial(numpy_sum(T), R, t, rec[0], case.dof), trial(kernel_sum(T), R, t, rec[0], case.dof)
            if x[0] and k[0]:
                worst[0] = max(worst[0], float(np.abs(x[2] - k[2]).max()))
                worst[1] = max(worst[1], float(np.linalg.norm(x[3] - k[3]) / np.linalg.norm(t)))
            if rec[4]:
                R, t = rec[6:15].reshape(3, 3), rec[15:18]
    return worst


def _rot_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra @ Rb.T) - 1.0) / 2.0, -1.0, 1.0))))


def measure_all(names=None, log=None):
    tau, shift = [0.0, 0.0], 0.0
    for name in (names or CASES):
        case = make(name)
        smp, _ = case_samples(case)
        rec, R, t, status, info = restatement_outputs(case, smp)
        a = measure_tau(case, smp, rec)
        tau = [max(x, y) for x, y in zip(tau, a)]
        for b in range(case.P):
            if case.kind[b] == "other" or status[b] == 0:
                continue
            Rt, tt = case.truth[b]
            if case.kind[b] == "shift":
                shift = max(shift, shift_error(case, b, t[b]))
            if log is not None:
                log("%-12s pose %d %-5s dof %-2s grid %2d status %d iters %2d n %3d -> %3d IoU %.3f -> %.3f |dt| %6.2f -> %6.2f rot %5.2f -> %5.2f deg%s" % (
                    name, b, case.kind[b], case.dof, case.grid, status[b], info[b, 5], info[b, 3], info[b, 4], silhouette_iou(case, b, case.R0[b], case.t0[b]),
                    silhouette_iou(case, b, R[b], t[b]), np.linalg.norm(case.t0[b] - tt), np.linalg.norm(t[b] - tt), _rot_deg(case.R0[b], Rt), _rot_deg(R[b], Rt),
                    "  shift error / Z %.4f" % shift_error(case, b, t[b]) if case.kind[b] == "shift" else ""))
    return tau, shift


if __name__ == "__main__":
    tau, shift = measure_all(sys.argv[1:], log=lambda s: print(s, flush=True))
    print("MEASURED_TAU = (%.3e, %.3e)\nlargest shift error / Z = %.4f" % (tau[0], tau[1], shift))
