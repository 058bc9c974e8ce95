"""TEST INFRASTRUCTURE (not collected): cp_surface_samples / cp_icp_refine (row N24) checked one iteration at a time by replaying the
device's own records.

THE RULE (csrc/icp_refine.hip states it; `samples_from`, `associate`, `refine` below are its numpy restatement).  All in float64.
Stage A, surface samples of a pose (one render at the INPUT pose; the render is tests/vsd_stages.py's rule)
  lattice     rect = the pose's vertex rectangle intersected with the frame, w x h pixels from (x0, y0); nx = min(grid, w), ny = min(grid, h);
              column i is pixel x0 + ((2 i + 1) w) // (2 nx), rows likewise; slot j * nx + i of S = grid * grid
  sample      a lattice pixel (x, y) the mesh covers: depth = the render's float32 depth, face = the winning face;
              Qr = (((x + 0.5 - cx) depth) / fx, ((y + 0.5 - cy) depth) / fy, depth); X = R^T (Qr - t);
              N = the unit normal of `face` ((v1 - v0) x (v2 - v0), normalised), negated where (R N) . Qr > 0
Stage B, association under (R, t), with depth the SENSOR's image
  Y = R X, C = Y + t, reject unless C_z > 0; u = (fx C_x) / C_z + cx, v likewise; pixel (floor u, floor v), reject outside the frame;
  d = depth[py, px], reject unless finite and > 0; Q = C (d / C_z); reject unless |C - Q|_2 <= max_dist; Np = R N; n = the pairs
Stage C, LM over the pairs: r_i = Np_i . (C_i - Q_i), Q_i and Np_i fixed; d = (w, v): R' = exp([w]x) R, t' = t + v;
  J_i = [(Y_i x Np_i)^T, Np_i^T]; H = sum J^T J, g = sum J^T r, c = sum r^2; lambda = 1e-3; rho = diameter / 2.  At most max_iters times:
  1 solve (H + lambda diag H + inertia n diag(rho^2, rho^2, rho^2, 1, 1, 1)) d = -g by Cholesky; 2 no factor (s, R', t' NaN), |v|_2 > max_dist
  or |w|_2 rho > max_dist: rejected, c' = +inf; 3 else c' over the SAME pairs; 4 accept iff c' < c: the state becomes the trial,
  lambda = max(lambda / 10, 1e-12), stage B again, n < min_pairs stops with status 3; 5 else lambda *= 10, lambda > 1e8 stops with
  status 3; 6 s = max(|w|_inf, |v|_inf / |t|): an ACCEPTED step with s <= step_tol stops with status 1; 7 iterations out: status 2.
  pass-through (status 0, pose bitwise the input, info NaN but for the counts): status_in == 0, a pose or K entry not finite, no render,
  fewer than min_pairs samples, fewer than min_pairs pairs under the input pose.
  records     18 doubles per executed iteration: [lambda, n, c, c', accepted, s, R' (9), t' (3)]
  info        42 doubles: [c0, c, samples, n0, n, iterations, H (36)]

`check_case` replays one case and raises pnp_stages.StageError (stage, pose, iteration in the message):
  N  stage A          X, N equal the restatement from the device's own (pixel, depth, face) to 1e-12 relative
  P  pass-through     expected exactly where the rule says; then pose bitwise, no records, info NaN but for the counts
  B  ties             FIRST: no decision of stage B lies within TIE = 1e-9 of its boundary: frac(u), frac(v) (pixels), C_z (relative to
                      |t|), |C - Q| - max_dist (relative to max_dist); a tie is reported as a tie
  n  pairs            n equals the restatement's count exactly
  L  lambda           reproduced EXACTLY from the accept flags
  C  cost             c and c' equal numpy's at the replayed state / over the state's pairs at the recorded trial pose to 1e-9 relative
  T  trial pose       numpy's trial from the replayed state within taus() (|dR|_max, |dt| / |t|); the kind of rejection equal
  A  accept flag      accepted == (c' < c) on the device's own two numbers
  E  stop and status  follow from the device's own s, lambda, n and iteration count; nothing recorded after the stop
  R  returned pose    bitwise the last accepted trial (or the input pose)
  I  info             cost0, the counts and the iterations exactly; cost and H to 1e-9 relative

MEASURED_TAU: the largest difference, over every executed iteration of every committed case free-running on a CPU, between the
restatement's trial pose with numpy's sums and with the kernel's summation order (`kernel_sum`: lm_stages.kernel_sum's scheme over the
SLOTS, an empty slot adding zero); taus() = 16 x that, capped at pnp_stages.TAU_CAP.  `python -m tests.icp_stages` prints it, the
table of the converging cases and the inertia table of DESIGN.md."""
import math
import sys

import numpy as np

from tests import lm_stages as L
from tests import pnp_stages as S
from tests import vsd_stages as V
from tests.pnp_stages import StageError

REC, INFO, MAX_ITERS, THREADS = 18, 42, 64, 256
LAMBDA0, LAMBDA_MIN, LAMBDA_STOP = 1e-3, 1e-12, 1e8
COST_RTOL, TIE, SAMPLE_RTOL = 1e-9, 1e-9, 1e-12
SIZE = (96, 80)                                    # (W, H): 3 x 3 tiles, the right and bottom ones partial
MEASURED_TAU = (3.7e-15, 3.2e-15)                  # seen: 3.664e-15 (halfbox_3_g32), 3.109e-15 (triangle_3_g17); printed by `python -m tests.icp_stages`; asserted in tests/test_icp_refine.py

numpy_sum = L.numpy_sum
kernel_sum = L.kernel_sum                          # thread i adds slots i, i + 256, ...; shuffle tree per wave; wave 0 + 1 + 2 + 3


def taus():
    return min(16 * MEASURED_TAU[0], S.TAU_CAP[0]), min(16 * MEASURED_TAU[1], S.TAU_CAP[1])


# ------------------------------------------------------------------------------------------------------------------- stage A
def lattice(rect, size, grid):
    """rect = (xmin, ymin, xmax, ymax) of the vertices' pixels -> (x0, y0, w, h, nx, ny), or None when it misses the frame"""
    W, H = size
    x0, y0, x1, y1 = max(int(rect[0]), 0), max(int(rect[1]), 0), min(int(rect[2]), W - 1), min(int(rect[3]), H - 1)
    if x0 > x1 or y0 > y1:
        return None
    w, h = x1 - x0 + 1, y1 - y0 + 1
    return x0, y0, w, h, min(grid, w), min(grid, h)


def lattice_axis(first, extent, n):
    return [first + ((2 * i + 1) * extent) // (2 * n) for i in range(n)]


def lattice_pixels(lat, grid):
    """-> pixel (S, 2) int, -1 beyond nx * ny"""
    pix = np.full((grid * grid, 2), -1, np.int64)
    if lat is not None:
        x0, y0, w, h, nx, ny = lat
        xs, ys = lattice_axis(x0, w, nx), lattice_axis(y0, h, ny)
        for j in range(ny):
            for i in range(nx):
                pix[j * nx + i] = xs[i], ys[j]
    return pix


def samples_from(pixel, depth, face, K, R, t, verts, faces, flip=True):
    """stage A from given (pixel (S,2), depth (S,) float32, face (S,)): -> X (S,3), N (S,3), face (S,) (-1 where the normal is not
    finite); NaN in empty slots.  flip=False is the checker's own tampering (normals not turned towards the camera)"""
    K, R, t = np.asarray(K, np.float64), np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    face = np.array(face, np.int64)
    X, N = np.full((len(face), 3), np.nan), np.full((len(face), 3), np.nan)
    k = np.nonzero(face >= 0)[0]
    if len(k) == 0:
        return X, N, face
    d = np.asarray(depth, np.float32)[k].astype(np.float64)
    px, py = np.asarray(pixel)[k, 0].astype(np.float64), np.asarray(pixel)[k, 1].astype(np.float64)
    Q = np.stack([((px + 0.5 - cx) * d) / fx, ((py + 0.5 - cy) * d) / fy, d], 1)
    e = Q - t
    Xk = np.stack([(R[0, j] * e[:, 0] + R[1, j] * e[:, 1]) + R[2, j] * e[:, 2] for j in range(3)], 1)
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)[face[k]]
    a, c = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    n = np.stack([a[:, 1] * c[:, 2] - a[:, 2] * c[:, 1], a[:, 2] * c[:, 0] - a[:, 0] * c[:, 2], a[:, 0] * c[:, 1] - a[:, 1] * c[:, 0]], 1)
    with np.errstate(all="ignore"):
        n = n / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]
    rn = np.stack([(R[i, 0] * n[:, 0] + R[i, 1] * n[:, 1]) + R[i, 2] * n[:, 2] for i in range(3)], 1)
    away = (rn[:, 0] * Q[:, 0] + rn[:, 1] * Q[:, 1]) + rn[:, 2] * Q[:, 2] > 0.0
    if flip:
        n = np.where(away[:, None], -n, n)
    good = np.isfinite(n).all(1)
    X[k[good]], N[k[good]] = Xk[good], n[good]
    face[k[~good]] = -1
    return X, N, face


def vertex_rect(R, t, K, verts, size):
    """the pixels whose sample can lie at a vertex, merged, as the scaffold's vertex kernel clamps them (float64 here); None with a vertex at Z <= 0"""
    u, v, Z, _ = V.screen(R, t, K, verts)
    if not (Z > 0).all() or not (np.isfinite(u).all() and np.isfinite(v).all()):
        return None
    W, H = size
    cu, cv = np.clip(u - 0.5, -2.0, W + 1.0), np.clip(v - 0.5, -2.0, H + 1.0)
    return int(np.floor(cu).min()), int(np.floor(cv).min()), int(np.ceil(cu).max()), int(np.ceil(cv).max())


def ray_faces(pixel, K, R, t, verts, faces):
    """the face a pixel's ray meets first (float64; the smallest index among equals), -1 where none"""
    K, R, t = np.asarray(K, np.float64), np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    cam = np.asarray(verts, np.float64) @ R.T + t
    f = np.asarray(faces, np.int64)
    v0, e1, e2 = cam[f[:, 0]], cam[f[:, 1]] - cam[f[:, 0]], cam[f[:, 2]] - cam[f[:, 0]]
    out = np.full(len(pixel), -1, np.int64)
    for s, (x, y) in enumerate(np.asarray(pixel)):
        if x < 0:
            continue
        dvec = np.array([(x + 0.5 - K[0, 2]) / K[0, 0], (y + 0.5 - K[1, 2]) / K[1, 1], 1.0])
        pv = np.cross(dvec, e2)
        det = (e1 * pv).sum(1)
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = -v0
            a = (tv * pv).sum(1) * inv
            qv = np.cross(tv, e1)
            b = (qv @ dvec) * inv
            z = (e2 * qv).sum(1) * inv
        hit = (det != 0) & (a >= 0) & (b >= 0) & (a + b <= 1) & (z > 0)
        if hit.any():
            zz = np.where(hit, z, np.inf)
            out[s] = int(np.argmin(zz))
    return out


def free_samples(R, t, K, verts, faces, size, grid):
    """stage A free-running on a CPU: the depth from vsd_stages.oracle_render, the face from the pixel's ray in float64
    -> dict(rect, shape, pixel, depth, face, X, N, ok) of ONE pose in the device's layout"""
    S_ = grid * grid
    rect = vertex_rect(R, t, K, verts, size)
    lat = None if rect is None else lattice(rect, size, grid)
    pixel = lattice_pixels(lat, grid)
    depth, face = np.zeros(S_, np.float32), np.full(S_, -1, np.int64)
    if lat is not None:
        o = V.oracle_render(R, t, K, verts, faces, size)["d"]
        used = lat[4] * lat[5]
        depth[:used] = o[pixel[:used, 1], pixel[:used, 0]]
        fc = ray_faces(pixel[:used], K, R, t, verts, faces)
        face[:used] = np.where((depth[:used] > 0) & (fc >= 0), fc, -1)
        depth[:used] = np.where(face[:used] >= 0, depth[:used], 0.0)
    X, N, face = samples_from(pixel, depth, face, K, R, t, verts, faces)
    return dict(rect=np.array([-1] * 4 if lat is None else [lat[0], lat[1], lat[0] + lat[2] - 1, lat[1] + lat[3] - 1]),
                shape=np.array([0, 0] if lat is None else [lat[4], lat[5]]), pixel=pixel, depth=depth, face=face, X=X, N=N,
                ok=int(rect is not None))


# ------------------------------------------------------------------------------------------------------------ stages B and C
TAMPERINGS = ("rot_sign", "pixel_centre", "round", "strict", "no_inertia", "no_flip", "rerotate")


def associate(X, N, face, K, R, t, depth, max_dist, tamper=()):
    """stage B for every slot -> dict(pair (S,) bool, Y, C, Q, Np (S,3), margin: the smallest distance of a decision from its boundary
    [frac px, C_z / |t|, (|C - Q| - max_dist) / max_dist], exact: whether a margin of exactly 0 occurred)"""
    K, R, t = np.asarray(K, np.float64), np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    H, W = depth.shape
    live = np.asarray(face) >= 0
    Xs = np.where(live[:, None], X, 0.0)
    Ns = np.where(live[:, None], N, 0.0)
    with np.errstate(all="ignore"):
        Y = np.stack([(R[i, 0] * Xs[:, 0] + R[i, 1] * Xs[:, 1]) + R[i, 2] * Xs[:, 2] for i in range(3)], 1)
        C = Y + t
        front = live & (C[:, 2] > 0.0)
        u, v = (fx * C[:, 0]) / C[:, 2] + cx, (fy * C[:, 1]) / C[:, 2] + cy
        inside = front & (u >= 0.0) & (u < W) & (v >= 0.0) & (v < H)
        fl = np.rint if "round" in tamper else np.floor
        px = np.clip(np.where(inside, fl(u), 0), 0, W - 1).astype(np.int64)
        py = np.clip(np.where(inside, fl(v), 0), 0, H - 1).astype(np.int64)
        d = depth[py, px].astype(np.float64)
        seen = inside & np.isfinite(d) & (d > 0.0)
        sc = d / C[:, 2]
        Q = C * sc[:, None]
        if "pixel_centre" in tamper:
            Q = np.stack([((px + 0.5 - cx) * d) / fx, ((py + 0.5 - cy) * d) / fy, d], 1)
        e = C - Q
        dist = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        pair = seen & ((dist < max_dist) if "strict" in tamper else (dist <= max_dist))
        Np = np.stack([(R[i, 0] * Ns[:, 0] + R[i, 1] * Ns[:, 1]) + R[i, 2] * Ns[:, 2] for i in range(3)], 1)
        m = [np.inf]
        if live.any():
            m.append(np.abs(C[live, 2]).min() / np.linalg.norm(t))
        if front.any():
            fu, fv = u[front] - np.floor(u[front]), v[front] - np.floor(v[front])
            m.append(min(np.minimum(fu, 1.0 - fu).min(), np.minimum(fv, 1.0 - fv).min()))
        if seen.any():
            m.append(np.abs(dist[seen] - max_dist).min() / max_dist)
    margin = float(np.nanmin(m))
    return dict(pair=pair, Y=Y, C=C, Q=Q, Np=Np, margin=margin, n=int(pair.sum()))


def pair_terms(a, tamper=()):
    """-> T (S, 29): per slot the 21 upper-triangle entries of J^T J row by row, the 6 of J^T r, r^2, 1; zero rows where there is no pair"""
    Y, C, Q, Np = a["Y"], a["C"], a["Q"], a["Np"]
    with np.errstate(all="ignore"):
        r = (Np[:, 0] * (C[:, 0] - Q[:, 0]) + Np[:, 1] * (C[:, 1] - Q[:, 1])) + Np[:, 2] * (C[:, 2] - Q[:, 2])
        J = [Y[:, 1] * Np[:, 2] - Y[:, 2] * Np[:, 1], Y[:, 2] * Np[:, 0] - Y[:, 0] * Np[:, 2], Y[:, 0] * Np[:, 1] - Y[:, 1] * Np[:, 0],
             Np[:, 0], Np[:, 1], Np[:, 2]]
        if "rot_sign" in tamper:
            J[:3] = [-J[0], -J[1], -J[2]]
        cols = [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * r for i in range(6)] + [r * r, np.ones_like(r)]
    T = np.stack(cols, 1)
    return np.where(a["pair"][:, None], T, 0.0)


def trial_cost(a, X, Rn, tn, sums=numpy_sum, N=None, tamper=()):
    """c' of (Rn, tn) over the pairs of association `a` (Q and Np fixed); +inf when it is not finite"""
    Xs = np.where(a["pair"][:, None], X, 0.0)
    Np = a["Np"]
    with np.errstate(all="ignore"):
        if "rerotate" in tamper:
            Ns = np.where(a["pair"][:, None], N, 0.0)
            Np = np.stack([(Rn[i, 0] * Ns[:, 0] + Rn[i, 1] * Ns[:, 1]) + Rn[i, 2] * Ns[:, 2] for i in range(3)], 1)
        Yn = np.stack([(Rn[i, 0] * Xs[:, 0] + Rn[i, 1] * Xs[:, 1]) + Rn[i, 2] * Xs[:, 2] for i in range(3)], 1)
        Cn = Yn + tn
        r = (Np[:, 0] * (Cn[:, 0] - a["Q"][:, 0]) + Np[:, 1] * (Cn[:, 1] - a["Q"][:, 1])) + Np[:, 2] * (Cn[:, 2] - a["Q"][:, 2])
        c = float(sums(np.where(a["pair"], r * r, 0.0)[:, None])[0])
    return c if math.isfinite(c) else float("inf")


def trial(sums, R, t, lam, damp, rho, max_dist):
    """the trial step of csrc/icp_refine.hip: H + lambda diag H + damp diag(rho^2 x 3, 1 x 3) on its own diagonal, lm_stages.solve_step,
    then the step bound -> (kind 0 no factor | 1 a trial | 2 beyond the step bound, d, R', t', s)"""
    Lm = L.load_lower(sums)
    for p_ in range(6):
        Lm[p_][p_] = (Lm[p_][p_] + lam * Lm[p_][p_]) + damp * (rho * rho if p_ < 3 else 1.0)
    pd, d, Rn, tn, s = L.solve_step(Lm, sums[21:27], R, t)
    if not pd:
        return 0, d, Rn, tn, s
    d0, d1, d2, d3, d4, d5 = (float(x) for x in d)
    th2 = d0 * d0 + d1 * d1 + d2 * d2
    vn = math.sqrt(d3 * d3 + d4 * d4 + d5 * d5)
    kind = 2 if (vn > max_dist or math.sqrt(th2) * rho > max_dist) else 1
    return kind, d, Rn, tn, s


def unpack_H(sums):
    return L.unpack_H(sums)


def passes_before_samples(K, R, t, status_in):
    return status_in == 0 or not (np.isfinite(K).all() and np.isfinite(R).all() and np.isfinite(t).all())


def refine(X, N, face, K, R, t, depth, max_dist, rho, status_in=1, max_iters=20, step_tol=1e-6, min_pairs=6, inertia=1e-2, sums=numpy_sum,
           tamper=()):
    """stages B and C on one pose -> dict(R, t, status, info (42,), records (max_iters, 18)) in the device's output layout"""
    K, R, t = np.asarray(K, np.float64), np.array(R, np.float64), np.array(t, np.float64).reshape(3)
    rec = np.full((max_iters, REC), np.nan)
    info = np.full(INFO, np.nan)
    n_samples = int((np.asarray(face) >= 0).sum())
    info[2:6] = n_samples, 0, 0, 0
    if passes_before_samples(K, R, t, status_in) or n_samples < min_pairs:
        return dict(R=R, t=t, status=0, info=info, records=rec)
    a = associate(X, N, face, K, R, t, depth, max_dist, tamper)
    info[3] = info[4] = a["n"]
    if a["n"] < min_pairs:
        return dict(R=R, t=t, status=0, info=info, records=rec)
    state = sums(pair_terms(a, tamper))
    c = c0 = float(state[27])
    n0 = a["n"]
    lam, status, iters = LAMBDA0, 2, 0
    for it in range(max_iters):
        n = a["n"]
        kind, d, Rn, tn, s = trial(state, R, t, lam, (0.0 if "no_inertia" in tamper else inertia) * n, rho, max_dist)
        cn = trial_cost(a, X, Rn, tn, sums, N, tamper) if kind == 1 else float("inf")
        accept = cn < c
        rec[it, :6] = lam, n, c, cn, 1.0 if accept else 0.0, s
        rec[it, 6:15], rec[it, 15:18] = Rn.reshape(9), tn
        iters = it + 1
        if accept:
            R, t = Rn, tn
            lam = max(lam / 10.0, LAMBDA_MIN)
            a = associate(X, N, face, K, R, t, depth, max_dist, tamper)
            state = sums(pair_terms(a, tamper))
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
    info[6:] = unpack_H(state).reshape(36)
    return dict(R=R, t=t, status=status, info=info, records=rec)


# ------------------------------------------------------------------------------------------------------------------ the checker
def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def _bits(a):
    return np.asarray(a, np.float64).reshape(-1).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def check_samples(smp, K, R, t, verts, faces, pose):
    """stage N: the device's X, N, face against the restatement from its own (pixel, depth, face)"""
    face_in = np.where(np.asarray(smp["depth"]) > 0, np.asarray(smp["face"]), -1)
    if not np.isfinite(R).all() or not np.isfinite(t).all() or not np.isfinite(K).all():
        if (np.asarray(smp["face"]) >= 0).any():
            raise StageError("N", pose, None, "samples of a pose that is not finite")
        return
    X, N, face = samples_from(smp["pixel"], smp["depth"], face_in, K, R, t, verts, faces)
    if not np.array_equal(face, np.asarray(smp["face"])):
        raise StageError("N", pose, None, "the sample slots differ from the restatement's")
    k = face >= 0
    if not (np.isnan(np.asarray(smp["X"])[~k]).all() and np.isnan(np.asarray(smp["N"])[~k]).all()):
        raise StageError("N", pose, None, "an empty slot holds a point or a normal")
    if k.any():
        dX = np.abs(np.asarray(smp["X"])[k] - X[k]).max(1) / np.maximum(np.abs(X[k]).max(1), 1.0)
        dN = np.abs(np.asarray(smp["N"])[k] - N[k]).max(1)
        if not (dX.max() <= SAMPLE_RTOL and dN.max() <= SAMPLE_RTOL):
            raise StageError("N", pose, None, "X / N off the restatement's by %.3e / %.3e (relative)" % (dX.max(), dN.max()))


def check_pose(smp, K, R_in, t_in, depth, max_dist, rho, status_in, max_iters, step_tol, min_pairs, inertia, pose, records, R_out, t_out, status,
               info, verts=None, faces=None, allow_exact=False):
    """Raises StageError where the outputs of cp_icp_refine on one pose contradict its own records or the restatement.  smp: the
    pose's samples (pixel, depth, face, X, N: the values the device read); verts / faces switch stage N on; allow_exact: a decision
    EXACTLY on its boundary is the rule's own comparison, not a tie (the checker's own test of `<=`).  -> statistics"""
    K, R_in, t_in = np.asarray(K, np.float64), np.asarray(R_in, np.float64), np.asarray(t_in, np.float64).reshape(3)
    records, R_out, t_out, info = np.asarray(records, np.float64), np.asarray(R_out, np.float64), np.asarray(t_out, np.float64).reshape(3), np.asarray(info, np.float64)
    X, N, face = np.asarray(smp["X"], np.float64), np.asarray(smp["N"], np.float64), np.asarray(smp["face"])
    status = int(status)
    stats = dict(iters=0, accepted=0, dR_1e18=0, dt_1e18=0, passed=0)
    if records.shape != (max_iters, REC) or info.shape != (INFO,):
        raise StageError("P", pose, None, "records / info have shapes %r / %r" % (records.shape, info.shape))
    if verts is not None:
        check_samples(smp, K, R_in, t_in, verts, faces, pose)
    n_samples = int((face >= 0).sum())

    def assoc(R, t, it):
        a = associate(X, N, face, K, R, t, depth, max_dist)
        if a["margin"] < TIE and not (allow_exact and a["margin"] == 0.0):
            raise StageError("B", pose, it, "a decision of stage B lies %.3e from its boundary: a tie" % a["margin"])
        return a

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

    if passes_before_samples(K, R_in, t_in, status_in) or n_samples < min_pairs:
        return passed(0)
    a = assoc(R_in, t_in, None)
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
        kind, d, Rn, tn, s = trial(state, R, t, lam, inertia * a["n"], rho, max_dist)
        if kind == 0:
            if not (np.isnan(rec[5:]).all() and cn_d == np.inf):
                raise StageError("T", pose, it, "numpy finds no Cholesky factor; the record holds a trial (c' = %r)" % cn_d)
        else:
            if not np.isfinite(rec[5:]).all():
                raise StageError("T", pose, it, "the trial pose or s is not finite, numpy's is")
            dR, dt = float(np.abs(Rn_d - Rn).max()), float(np.linalg.norm(tn_d - tn) / np.linalg.norm(t))
            stats["dR_1e18"], stats["dt_1e18"] = max(stats["dR_1e18"], int(1e18 * dR)), max(stats["dt_1e18"], int(1e18 * dt))
            if not (dR <= tau_R and dt <= tau_t):
                raise StageError("T", pose, it, "trial pose off numpy's: |dR| = %.3e (tau %.3e), |dt|/|t| = %.3e (tau %.3e)" % (dR, tau_R, dt, tau_t))
            if not abs(s_d - s) <= max(tau_R, tau_t):
                raise StageError("T", pose, it, "s = %.17g, numpy's %.17g" % (s_d, s))
            if kind == 2:
                if cn_d != np.inf:
                    raise StageError("T", pose, it, "the step passes the bound max_dist, c' = %r is not +inf" % cn_d)
            else:
                cn = trial_cost(a, X, Rn_d, tn_d)
                if np.isinf(cn) != np.isinf(cn_d) or (np.isfinite(cn) and not _rel(cn_d, cn) <= COST_RTOL):
                    raise StageError("C", pose, it, "c' = %.17g, numpy over the state's pairs at the recorded trial pose: %.17g" % (cn_d, cn))
        if acc_d not in (0.0, 1.0) or bool(acc_d) != bool(cn_d < c_d):
            raise StageError("A", pose, it, "accepted = %r with c' = %.17g, c = %.17g" % (acc_d, cn_d, c_d))
        iters = it + 1
        if acc_d:
            R, t, last = Rn_d.copy(), tn_d.copy(), (Rn_d.copy(), tn_d.copy())
            lam = max(lam / 10.0, LAMBDA_MIN)
            stats["accepted"] += 1
            a = assoc(R, t, it)
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
    if not (_same(info[0], records[0, 2]) and info[2] == n_samples and info[3] == n0 and info[4] == a["n"] and info[5] == iters):
        raise StageError("I", pose, None, "info = %r, the records say cost0 %.17g, %d samples, %d / %d pairs, %d iterations" % (info[:6].tolist(), records[0, 2], n_samples, n0, a["n"], iters))
    if not _rel(info[1], float(state[27])) <= COST_RTOL or (not records[iters - 1, 4] and not _same(info[1], records[iters - 1, 2])):
        raise StageError("I", pose, None, "cost = %.17g, numpy at the returned pose: %.17g" % (info[1], float(state[27])))
    H_d, H = info[6:].reshape(6, 6), unpack_H(state)
    scale = np.sqrt(np.outer(np.diag(H), np.diag(H))) + 1e-300
    if not (np.isfinite(H_d).all() and np.array_equal(H_d, H_d.T) and (np.abs(H_d - H) <= COST_RTOL * scale).all()):
        raise StageError("I", pose, None, "H off numpy's at the returned pose by %.3e of sqrt(H_ii H_jj)" % float(np.nanmax(np.abs(H_d - H) / scale)))
    return stats


# ------------------------------------------------------------------------------------------------------------- the committed cases
K_A = np.array([[120.0, 0.0, 47.3], [0.0, 118.0, 40.6], [0.0, 0.0, 1.0]])
K_B = np.array([[124.0, 0.0, 45.7], [0.0, 121.0, 38.2], [0.0, 0.0, 1.0]])


def _rodrigues(axis, angle):
    return L._rodrigues(np.asarray(axis, np.float64), angle)


def _random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def mesh_arrays(names):
    m = V.meshes()
    return [m[k][0] for k in names], [m[k][1] for k in names]


def diameters(names):
    return np.array([V.diameter(V.meshes()[k][0]) for k in names])


def add_error(verts, R, t, Rt, tt):
    v = np.asarray(verts, np.float64)
    return float(np.linalg.norm((v @ np.asarray(R).T + np.reshape(t, 3)) - (v @ np.asarray(Rt).T + np.reshape(tt, 3)), axis=1).mean())


class IcpCase:
    """meshes: names into vsd_stages.meshes(); mesh_ids (P,) or None; K (3,3) or (P,3,3); image_ids (P,) or None with ONE image;
    truth: per IMAGE (mesh index, R, t, K) of the object the sensor saw; R0 (P,3,3), t0 (P,3): the start poses; depth (I,H,W) float32"""

    def __init__(self, name, meshes, mesh_ids, K, image_ids, truth, R0, t0, depth, max_dist, grid=17, max_iters=20, step_tol=1e-6, min_pairs=6,
                 inertia=1e-2, status_in=None):
        self.name, self.meshes, self.mesh_ids, self.K, self.image_ids, self.truth = name, tuple(meshes), mesh_ids, K, image_ids, truth
        self.R0, self.t0, self.depth, self.max_dist = R0, t0, depth, max_dist
        self.grid, self.max_iters, self.step_tol, self.min_pairs, self.inertia, self.status_in = grid, max_iters, step_tol, min_pairs, inertia, status_in
        self.P = len(R0)
        self.size = SIZE

    def mesh_of(self, b):
        return 0 if self.mesh_ids is None else int(self.mesh_ids[b])

    def image_of(self, b):
        return 0 if self.image_ids is None else int(self.image_ids[b])

    def K_of(self, b):
        return self.K[b] if self.K.ndim == 3 else self.K

    def max_dist_of(self, b):
        return float(self.max_dist[b]) if np.ndim(self.max_dist) else float(self.max_dist)

    def geometry(self, b):
        verts, faces = mesh_arrays(self.meshes)
        return verts[self.mesh_of(b)], faces[self.mesh_of(b)]

    def rho_of(self, b):
        return float(diameters(self.meshes)[self.mesh_of(b)]) / 2.0

    def truth_of(self, b):
        return self.truth[self.image_of(b)]


_RENDERS = {}


def sensor_depth(mesh, R, t, K, seed):
    """what the sensor saw: the oracle render of the truth pose, a far plane behind it, a near occluder slab, a patch of zeros and a
    patch of NaN (cached: the tests share it and leave it unchanged)"""
    key = (mesh, seed)
    if key not in _RENDERS:
        v, f = V.meshes()[mesh]
        d = V.oracle_render(R, t, K, v, f, SIZE)["d"].astype(np.float32)
        W, H = SIZE
        d = np.where(d > 0, d, np.float32(900.0))
        rng = np.random.default_rng(1000 + seed)
        ys, xs = np.nonzero(d < 900.0)
        x_mid, y_mid = (int(np.median(xs)), int(np.median(ys))) if len(xs) else (W // 2, H // 2)
        x_occ = int(np.clip(x_mid + rng.integers(4, 9), 0, W - 4))
        d[:, x_occ:x_occ + 3] = np.float32(150.0)                       # the occluder slab: three columns through the object
        y_z = int(np.clip(y_mid - rng.integers(5, 10), 0, H - 3))
        d[y_z:y_z + 2, max(x_mid - 12, 0):max(x_mid - 12, 0) + 5] = 0.0  # the sensor's holes
        d[min(y_mid + 6, H - 2):min(y_mid + 6, H - 2) + 2, max(x_mid - 10, 0):max(x_mid - 10, 0) + 4] = np.nan
        d.setflags(write=False)
        _RENDERS[key] = d
    return _RENDERS[key]


def _scene(name, seed, layout, K=K_A, per_pose_K=False, off_frame=(), max_dist=0.3, deg=4.0, ray=0.04, distance=(300.0, 360.0), **kw):
    """layout: per pose (mesh name, image).  Every image holds ONE object at a random truth pose; each pose starts `deg` degrees and
    `ray` of the distance along the viewing ray off its image's truth.  off_frame: images whose object lies partly outside the frame.
    max_dist: a fraction of each pose's mesh diameter (a float: the smallest over the poses as ONE number; "tensor": one per pose)"""
    rng = np.random.default_rng(seed)
    names = []
    for m, _ in layout:
        if m not in names:
            names.append(m)
    n_img = 1 + max(i for _, i in layout)
    P = len(layout)
    Ks = np.stack([K_A if b % 2 == 0 else K_B for b in range(P)]) if per_pose_K else K
    truth, depth = [], []
    for i in range(n_img):
        b0 = [b for b, (_, im) in enumerate(layout) if im == i][0]
        Kb = Ks[b0] if per_pose_K else K
        mesh = layout[b0][0]
        R = _random_rotation(rng)
        z = rng.uniform(*distance)
        t = np.array([rng.uniform(-20, 20), rng.uniform(-15, 15), z])
        if i in off_frame:
            t[0] = z * (SIZE[0] - 6.0 - Kb[0, 2]) / Kb[0, 0]               # the object's centre six pixels inside the right edge
        truth.append((names.index(mesh), R, t, Kb))
        depth.append(sensor_depth(mesh, R, t, Kb, seed * 16 + i))
    R0, t0 = [], []
    for b, (m, i) in enumerate(layout):
        _, R, t, _ = truth[i]
        R0.append(_rodrigues(rng.normal(size=3), np.radians(deg)) @ R)
        t0.append(t * (1.0 + ray * (1.0 if rng.random() < 0.5 else -1.0)))
    mesh_ids = None if len(names) == 1 else np.array([names.index(m) for m, _ in layout], np.int32)
    image_ids = None if n_img == 1 else np.array([i for _, i in layout], np.int32)
    diam = diameters(names)
    per = np.array([diam[names.index(m)] for m, _ in layout])
    if max_dist == "tensor":
        md = 0.3 * per
    else:
        md = float(max_dist * per.min())
    return IcpCase(name, names, mesh_ids, Ks, image_ids, truth, np.stack(R0), np.stack(t0), np.stack(depth), md, **kw)


def _passthrough():
    """pose 0 is refined (the control); 1: status 0 in; 2: NaN in R; 3: inf in t; 4: started far to the side (no pair within max_dist)"""
    c = _scene("passthrough", 31, [("torus", 0)] * 5, grid=17)
    c.status_in = np.ones(5, np.int32)
    c.status_in[1] = 0
    c.R0[2, 1, 2] = np.nan
    c.t0[3, 0] = np.inf
    c.t0[4] = c.t0[4] * np.array([1.0, 1.0, 1.6])
    return c


def _narrow():
    """a triangle seen nearly edge-on from far away: its rectangle is narrower than the grid (nx = w < grid)"""
    c = _scene("narrow_triangle", 34, [("triangle", 0)], grid=32, distance=(1400.0, 1500.0), deg=1.0, ray=0.01, max_dist=0.5)
    return c


CASES = {
    "torus_1_g8": lambda: _scene("torus_1_g8", 11, [("torus", 0)], grid=8),
    "torus_3_g17": lambda: _scene("torus_3_g17", 12, [("torus", 0), ("torus", 1), ("torus", 0)], grid=17),
    "ico80_3_g32": lambda: _scene("ico80_3_g32", 13, [("ico80", 0), ("ico80", 1), ("ico80", 2)], grid=32, per_pose_K=True),
    "ico80_1_g64": lambda: _scene("ico80_1_g64", 14, [("ico80", 0)], grid=64),
    "box_3_g17": lambda: _scene("box_3_g17", 15, [("box", 0), ("box", 1), ("box", 1)], grid=17),
    "halfbox_3_g32": lambda: _scene("halfbox_3_g32", 16, [("halfbox", 0), ("halfbox", 1), ("halfbox", 2)], grid=32),
    "mixed_5_g17": lambda: _scene("mixed_5_g17", 17, [("torus", 0), ("box", 1), ("torus", 0), ("box", 1), ("torus", 2)], grid=17, max_dist="tensor"),
    "mixed_5_g64": lambda: _scene("mixed_5_g64", 18, [("ico80", 0), ("torus", 1), ("ico80", 2), ("torus", 1), ("ico80", 0)], grid=64, per_pose_K=True,
                                  max_dist="tensor"),
    "torus_off_frame": lambda: _scene("torus_off_frame", 19, [("torus", 0), ("torus", 1), ("torus", 0)], grid=17, off_frame=(0,)),
    "torus_it1": lambda: _scene("torus_it1", 12, [("torus", 0), ("torus", 1), ("torus", 0)], grid=17, max_iters=1),
    "torus_it2": lambda: _scene("torus_it2", 12, [("torus", 0), ("torus", 1), ("torus", 0)], grid=17, max_iters=2),
    "ico80_inertia0": lambda: _scene("ico80_inertia0", 20, [("ico80", 0), ("ico80", 1), ("ico80", 0)], grid=17, inertia=0.0),
    "triangle_1_g8": lambda: _scene("triangle_1_g8", 21, [("triangle", 0)], grid=8),        # seen edge-on: fewer than 6 samples
    "triangle_3_g17": lambda: _scene("triangle_3_g17", 22, [("triangle", 0), ("triangle", 1), ("triangle", 2)], grid=17),
    "narrow_triangle": _narrow,
    "passthrough": _passthrough,
}
# the cases every refined pose of which the restatement ALONE, free-running on a CPU, brings below a quarter of its starting ADD with
# status 1 or 2 (tests/test_icp_refine.py::test_converging_selection asserts it); the others are "drifting": only the replay is asserted
CONVERGING = ("torus_1_g8", "torus_3_g17", "ico80_3_g32", "ico80_1_g64", "box_3_g17", "halfbox_3_g32", "mixed_5_g17", "mixed_5_g64",
              "torus_off_frame", "torus_it1", "torus_it2", "ico80_inertia0", "narrow_triangle", "passthrough")

_CASES = {}


def make(name):
    if name not in _CASES:
        _CASES[name] = CASES[name]()
    return _CASES[name]


def case_samples(case):
    """stage A free-running for every pose of a case: a list of per-pose dicts"""
    out = []
    for b in range(case.P):
        v, f = case.geometry(b)
        R, t, K = case.R0[b], case.t0[b], case.K_of(b)
        if not (np.isfinite(R).all() and np.isfinite(t).all()):
            S_ = case.grid ** 2
            out.append(dict(rect=np.array([-1] * 4), shape=np.array([0, 0]), pixel=np.full((S_, 2), -1), depth=np.zeros(S_, np.float32),
                            face=np.full(S_, -1), X=np.full((S_, 3), np.nan), N=np.full((S_, 3), np.nan), ok=0))
        else:
            out.append(free_samples(R, t, K, v, f, case.size, case.grid))
    return out


def restatement_outputs(case, samples, sums=numpy_sum, tamper=(), inertia=None):
    """the restatement's own run of a case over `samples` (a list of per-pose dicts) in the device's output layout:
    (records (P,it,18), R (P,3,3), t (P,3), status (P,), info (P,42))"""
    outs = []
    for b in range(case.P):
        s = samples[b]
        outs.append(refine(s["X"], s["N"], s["face"], case.K_of(b), case.R0[b], case.t0[b], case.depth[case.image_of(b)], case.max_dist_of(b),
                           case.rho_of(b), 1 if case.status_in is None else int(case.status_in[b]), case.max_iters, case.step_tol, case.min_pairs,
                           case.inertia if inertia is None else inertia, sums, tamper))
    return (np.stack([o["records"] for o in outs]), np.stack([o["R"] for o in outs]), np.stack([o["t"] for o in outs]),
            np.array([o["status"] for o in outs], np.int32), np.stack([o["info"] for o in outs]))


def check_case(case, samples, records, R, t, status, info, log=None, stage_a=True, allow_exact=False):
    """samples: a list of per-pose dicts (pixel, depth, face, X, N: what the device read)"""
    total = {}
    for b in range(case.P):
        v, f = case.geometry(b)
        st = check_pose(samples[b], case.K_of(b), case.R0[b], case.t0[b], case.depth[case.image_of(b)], case.max_dist_of(b), case.rho_of(b),
                        1 if case.status_in is None else int(case.status_in[b]), case.max_iters, case.step_tol, case.min_pairs, case.inertia, b,
                        records[b], R[b], np.asarray(t[b]).reshape(3), int(status[b]), info[b], verts=v if stage_a else None, faces=f,
                        allow_exact=allow_exact)
        for k, x in st.items():
            total[k] = max(total.get(k, 0), x) if k.endswith("_1e18") else total.get(k, 0) + x
    if log is not None:
        log("%-18s status %s %s" % (case.name, np.asarray(status).tolist()[:8], " ".join("%s=%d" % kv for kv in sorted(total.items()))))
    return total


def add_ratios(case, R, t):
    """per pose (starting ADD, final ADD) against its image's truth"""
    out = []
    for b in range(case.P):
        v, _ = case.geometry(b)
        _, Rt, tt, _ = case.truth_of(b)
        out.append((add_error(v, case.R0[b], case.t0[b], Rt, tt), add_error(v, R[b], np.reshape(t[b], 3), Rt, tt)))
    return out


def converges(case, R, t, status):
    """every refined pose ends below a quarter of its starting ADD with status 1 or 2 (and at least one pose is refined)"""
    ok, any_ = True, False
    for b, (a0, a1) in enumerate(add_ratios(case, R, t)):
        if status[b] == 0:
            continue
        any_ = True
        ok = ok and status[b] in (1, 2) and a1 < 0.25 * a0
    return ok and any_


def measure_tau(case, samples, records):
    """largest (|dR|_max, |dt| / |t|) between the trial from numpy's sums and from the kernel-order sums of the same terms, over every
    executed iteration of the restatement's run of a case"""
    worst = [0.0, 0.0]
    for b in range(case.P):
        s = samples[b]
        R, t = case.R0[b], case.t0[b]
        for rec in records[b]:
            if np.isnan(rec[0]):
                break
            a = associate(s["X"], s["N"], s["face"], case.K_of(b), R, t, case.depth[case.image_of(b)], case.max_dist_of(b))
            T = pair_terms(a)
            args = (R, t, rec[0], case.inertia * a["n"], case.rho_of(b), case.max_dist_of(b))
            x, k = trial(numpy_sum(T), *args), trial(kernel_sum(T), *args)
            if x[0] and k[0]:
                worst[0] = max(worst[0], float(np.abs(x[2] - k[2]).max()))
                worst[1] = max(worst[1], float(np.linalg.norm(x[3] - k[3]) / np.linalg.norm(t)))
            if rec[4]:
                R, t = rec[6:15].reshape(3, 3), rec[15:18]
    return worst


def measure_all(names=None, log=None, inertias=(0.0, 1e-3, 1e-2, 1e-1)):
    tau, conv = [0.0, 0.0], []
    for name in (names or CASES):
        case = make(name)
        smp = case_samples(case)
        rec, R, t, status, info = restatement_outputs(case, smp)
        a = measure_tau(case, smp, rec)
        tau = [max(x, y) for x, y in zip(tau, a)]
        if converges(case, R, t, status):
            conv.append(name)
        if log is not None:
            diam = diameters(case.meshes)
            cols = []
            for w in inertias:
                _, Rw, tw, sw, _ = restatement_outputs(case, smp, inertia=w)
                cols.append(" ".join("%5.1f" % (100.0 * a1 / diam[case.mesh_of(b)]) if sw[b] else "  -  " for b, (_, a1) in enumerate(add_ratios(case, Rw, tw))))
            start = " ".join("%5.1f" % (100.0 * a0 / diam[case.mesh_of(b)]) for b, (a0, _) in enumerate(add_ratios(case, R, t)))
            log("%-16s tau %.2e %.2e status %s iters %s n %s | ADD %% of diameter: start %s | %s" % (
                name, a[0], a[1], status.tolist(), info[:, 5].astype(int).tolist(), info[:, 4].astype(int).tolist(), start,
                " | ".join("inertia %g: %s" % (w, c) for w, c in zip(inertias, cols))))
    return tau, conv


if __name__ == "__main__":
    tau, conv = measure_all(sys.argv[1:], log=lambda s: print(s, flush=True))
    print("MEASURED_TAU = (%.3e, %.3e)\nCONVERGING = %r" % (tau[0], tau[1], tuple(conv)))
