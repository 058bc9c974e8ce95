"""Row N23 (rotation / translation errors against the closest symmetric ground truth, the LM report's pass counts): the rule at the
top of csrc/rete.hip restated in float64 numpy, one pose pair at a time.  Not a test file: tests/test_rete.py checks it against what
the reference's own functions recorded (tests/golden/rete.npz), tests/test_gpu_rete.py compares the device with it.  `mut` names ONE
deliberate mistake (MUTATIONS), so that the CPU test can show that the fixture tells the right rule from the wrong one."""
import json

import numpy as np

MUTATIONS = ("le", "cos_noclamp", "S_Rgt", "te_sym_t")
EPS = 2.0 ** -53                          # the unit roundoff, as tests/test_gpu_targets.py has it
COUNT_COLUMNS = ("n", "adx2", "adx5", "adx10", "rete2", "rete5", "re2", "re5", "te2", "te5")
_CACHE = {}


def fixture():
    if "g" not in _CACHE:
        from tests.common import golden
        g = golden("rete")
        _CACHE["g"] = {k: g[k] for k in g.files}
    return _CACHE["g"]


def models_info(fx=None):
    """the fixture's synthetic models_info: {obj_id (int): entry}"""
    fx = fixture() if fx is None else fx
    return {int(k): v for k, v in json.loads(str(fx["models_info"])).items()}


def cos_cof(Ra, C):
    """(trace(Ra . inv(C)) - 1) / 2 with the inverse from the cofactors, summed row by row: 1 exactly for bitwise-equal matrices.
    C: (3,3) or a stack (n,3,3) -- every candidate by the same operations in the same order"""
    C = np.asarray(C, dtype=np.float64)
    r0, r1, r2 = C[..., 0, :], C[..., 1, :], C[..., 2, :]
    cof = np.stack([np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)], -2)
    det = r0[..., 0] * cof[..., 0, 0] + r0[..., 1] * cof[..., 0, 1] + r0[..., 2] * cof[..., 0, 2]
    prod = ((Ra - C) * cof).reshape(C.shape[:-2] + (9,))
    s = prod[..., 0]
    for k in range(1, 9):
        s = s + prod[..., k]
    return 1.0 + 0.5 * (s / det)


def degrees_of(c):
    """degrees(acos(clamp(c, -1, 1))); NaN where c is not finite"""
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(c), np.arccos(np.minimum(1.0, np.maximum(-1.0, c))) * (180.0 / np.pi), np.nan)


def candidates(R_gt, syms, mut=None):
    """[R_gt] + [R_gt . S_k] as a stack (1 + S, 3, 3); syms: (S,3,3) or None"""
    out = [R_gt]
    for S in (() if syms is None else syms):
        out.append(product(S, R_gt) if mut == "S_Rgt" else product(R_gt, S))
    return np.stack(out)


def product(A, B):
    """A . B as the kernel forms it: per entry a_i0 b_0j + a_i1 b_1j + a_i2 b_2j, left to right, every operation rounded"""
    return A[:, 0:1] * B[0] + A[:, 1:2] * B[1] + A[:, 2:3] * B[2]


def candidate_res(R_est, R_gt, syms):
    """re of every candidate in order (1 + S,): what the winner is chosen from"""
    return degrees_of(cos_cof(R_est, candidates(R_gt, syms)))


def closest(R_est, R_gt, syms, mut=None):
    """-> (re in degrees, the winner's cos before the clamp, the winner's index: -1 = R_gt itself)"""
    cs = cos_cof(R_est, candidates(R_gt, syms, mut))
    if mut == "cos_noclamp":                     # the comparison on cos, the clamp dropped
        with np.errstate(invalid="ignore"):
            res, key = np.degrees(np.arccos(cs)), -cs
    else:
        res = degrees_of(cs)
        key = res
    best = 0
    for k in range(1, len(cs)):                  # the strict `<` keeps the earlier candidate; NaN never replaces
        if (key[k] <= key[best]) if mut == "le" else (key[k] < key[best]):
            best = k
    return float(res[best]), float(cs[best]), best - 1


def te_of(t_est, t_gt, sym_t=None, mut=None):
    d = np.asarray(t_gt, dtype=np.float64).reshape(3) - np.asarray(t_est, dtype=np.float64).reshape(3)
    if mut == "te_sym_t" and sym_t is not None:
        d = d + np.asarray(sym_t, dtype=np.float64).reshape(3)
    return float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))


def rete_batch(R_est, t_est, R_gt, t_gt, tables=None, mesh_ids=None, mut=None):
    """the whole entry point: tables = per-mesh (S,12) arrays [R | t] or None -> (re, te, cos, index) arrays"""
    P = len(R_est)
    re, te, cs, idx = np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P, dtype=np.int32)
    for p in range(P):
        T = None if tables is None else tables[0 if mesh_ids is None else int(mesh_ids[p])]
        S = None if T is None else T[:, :9].reshape(-1, 3, 3)
        re[p], cs[p], idx[p] = closest(R_est[p], R_gt[p], S, mut)
        te[p] = te_of(t_est[p], t_gt[p], T[idx[p], 9:] if (T is not None and idx[p] >= 0) else None, mut)
    return re, te, cs, idx


def tol_cos():
    """the project's bound for the cofactor cosine (tests/test_gpu_targets.py): 64 eps"""
    return 64.0 * EPS


def tol_re(cos):
    """the bound of re that follows from tol_cos: d / sqrt(1 - cos^2) in degrees, acos(1 - d) next to the ends"""
    c = np.clip(np.asarray(cos, dtype=np.float64), -1.0, 1.0)
    d = tol_cos()
    with np.errstate(divide="ignore", invalid="ignore"):
        inner = np.degrees(d / np.sqrt(1.0 - c * c))
    return np.where(np.abs(c) > 1.0 - 1e-9, np.degrees(np.arccos(1.0 - d)), inner)


def tol_te(t_a, t_b):
    return 8.0 * EPS * (np.linalg.norm(np.asarray(t_a).reshape(-1, 3), axis=1) + np.linalg.norm(np.asarray(t_b).reshape(-1, 3), axis=1))


def pass_flags(re, te, adx, diam):
    """(P, 10) 0 / 1: [1, adx < 0.02 d, < 0.05 d, < 0.1 d, re<2 & te<20, re<5 & te<50, re<2, re<5, te<20, te<50]; NaN is 10000 first"""
    f = lambda x: np.where(np.isnan(x), 10000.0, np.asarray(x, dtype=np.float64))      # noqa: E731
    r, t, a, d = f(re), f(te), f(adx), np.asarray(diam, dtype=np.float64)
    return np.stack([np.ones_like(r, dtype=bool), a < d * 0.02, a < d * 0.05, a < d * 0.1, (r < 2) & (t < 20), (r < 5) & (t < 50),
                     r < 2, r < 5, t < 20, t < 50], 1).astype(np.int32)


def pass_counts(re, te, adx, diam, slot, n_obj):
    out = np.zeros((n_obj, len(COUNT_COLUMNS)), dtype=np.int32)
    np.add.at(out, np.asarray(slot, dtype=np.int64), pass_flags(re, te, adx, diam))
    return out


def rates(counts):
    """-> (per-object rates (n_obj, 9), their means over the objects (9,))"""
    c = np.asarray(counts, dtype=np.float64)
    r = c[:, 1:] / c[:, :1]
    return r, np.array([np.mean(r[:, k]) for k in range(r.shape[1])])
