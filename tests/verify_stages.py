"""Row N26 (hypothesis verification against the sensor's depth), the rule the device is pinned by.  Not a test file: the rule of
csrc/pose_verify.hip in numpy, operation for operation, the committed cases, the checker and its tamperings.  Nothing here reads the
reference (it does not verify); the meshes and the CPU render are tests/vsd_stages.py's, the frame and the scenes' make tests/icp_stages.py's.

  classify(D, S, tau)             float32: the label of every pixel (0 none, 1 match, 2 occluded, 3 through, 4 missing) and q
  counts_of, score_of             the six integer sums; fit, den, score, ok in float64
  select(score, ok)               the choice per crop over candidate-major scores
  reference(case, D)              a case's expected outputs from renders D (P,H,W) -- render_f32's on a CPU, metric.render_depth's on the device
  check_case(case, D, out)        every output EQUAL to the reference's (counts, labels, choice) or the same bits (fit, den, score)

The rule.  D: the pose's depth render, S: the sensor depth of the pose's image, tau: the pose's tolerance as float32.  A pixel with D > 0
is a model pixel; it is missing when S is not finite or S <= 0; else with d = S - D (one float32 subtraction) and a = |d| it is a match
when a <= tau, occluded when d < -tau, through when d > tau.  A match adds q = min(63, int(64 * (a / tau))) (float32 division, float32
product, truncation).  fit = n_match - sum_q / 64, den = (n_match + n_through) + occlusion_weight * n_occluded, score = fit / den in
float64; NaN with ok = 0 when den == 0 or the pose is not counted (status 0, an image id out of range, a tau that as float32 is not
positive and finite -- and whatever is not rendered: D is then all zero).  Per crop the eligible candidate with the largest score wins,
the smallest index on equal scores, candidate 0 when none is eligible."""
import numpy as np

from tests import icp_stages as I
from tests import vsd_stages as V
from tests.pnp_stages import StageError

SIZE = I.SIZE                                      # (W, H) = (96, 80): 3 x 3 tiles, the right and bottom ones partial
COUNTS = ("n_model", "n_missing", "n_match", "n_occluded", "n_through", "sum_q")
NONE, MATCH, OCCLUDED, THROUGH, MISSING = 0, 1, 2, 3, 4
TAMPERINGS = ("strict", "swap", "nan_zero", "round", "no_weight", "last_tie")


# ------------------------------------------------------------------------------------------------------------------- the rule
def classify(D, S, tau, tamper=()):
    """-> (labels uint8, q int64), both shaped like D.  tamper: names of TAMPERINGS, for the checker's own test"""
    f32 = np.float32
    D, S, tau = np.asarray(D, f32), np.asarray(S, f32), f32(tau)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        model = D > 0
        if "nan_zero" in tamper:                                                # NaN read as a measured depth of 0
            missing = np.isinf(S) | (S <= 0)
            S = np.where(np.isnan(S), f32(0), S)
        else:
            missing = ~np.isfinite(S) | ~(S > 0)
        d = (S - D).astype(f32)
        a = np.abs(d)
        match = (a < tau) if "strict" in tamper else (a <= tau)
        occluded = ~match & (d < -tau)
        through = ~match & ~occluded
        if "swap" in tamper:
            occluded, through = through, occluded
        r = (a / tau).astype(f32)
        v = (f32(64.0) * r).astype(f32)
        v = np.where(match & model & ~missing, v, f32(0))
        q = np.minimum(63, (np.rint(v) if "round" in tamper else np.trunc(v)).astype(np.int64))
    lab = np.zeros(D.shape, np.uint8)
    live = model & ~missing
    lab[model & missing] = MISSING
    lab[live & match] = MATCH
    lab[live & occluded] = OCCLUDED
    lab[live & through] = THROUGH
    return lab, np.where(lab == MATCH, q, 0)


def counts_of(lab, q):
    """the six sums of one pose -> int64 (6,)"""
    return np.array([int((lab != NONE).sum()), int((lab == MISSING).sum()), int((lab == MATCH).sum()), int((lab == OCCLUDED).sum()),
                     int((lab == THROUGH).sum()), int(q.sum())], np.int64)


def score_of(counts, occlusion_weight=1.0, counted=True, tamper=()):
    """-> (score, fit, den, ok) in float64, every operation rounded on its own"""
    n = [np.float64(int(x)) for x in counts]
    w = np.float64(1.0 if "no_weight" in tamper else occlusion_weight)
    fit = n[2] - n[5] / np.float64(64.0)
    den = (n[2] + n[4]) + w * n[3]
    ok = bool(counted) and den != 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return (fit / den if ok else np.float64(np.nan)), fit, den, ok


def select(score, ok, tamper=()):
    """score, ok (C,B) -> choice int32 (B,)"""
    score, ok = np.asarray(score, np.float64), np.asarray(ok, bool)
    C, B = score.shape
    choice = np.zeros(B, np.int32)
    for b in range(B):
        best = -1
        for c in range(C):
            s = score[c, b]
            if not ok[c, b] or np.isnan(s):
                continue
            if best < 0 or s > score[best, b] or ("last_tie" in tamper and s == score[best, b]):
                best = c
        choice[b] = max(best, 0)
    return choice


# ------------------------------------------------------------------------------------------------------------------- the cases
class VerifyCase:
    """meshes: names into vsd_stages.meshes(); mesh_ids (P,) or None; K (3,3) or (P,3,3); image_ids (P,) or None with ONE image;
    R (P,3,3), t (P,3): the poses, candidate-major when cand = (C, B); depth (I,H,W) float32, or None with tie = True: the sensor depth
    is then built from the poses' OWN renders (tie_depth), whoever made them; tau: a number or (P,); status (P,) int32 or None"""

    def __init__(self, name, meshes, mesh_ids, K, image_ids, R, t, depth, tau, occlusion_weight=1.0, status=None, cand=None, tie=False):
        self.name, self.meshes, self.mesh_ids, self.K, self.image_ids = name, tuple(meshes), mesh_ids, np.asarray(K, np.float64), image_ids
        self.R, self.t, self.depth, self.tau, self.occlusion_weight, self.status, self.cand, self.tie = R, t, depth, tau, occlusion_weight, status, cand, tie
        self.P, self.size = len(R), SIZE
        self.n_img = 1 if depth is None else len(depth)

    def mesh_of(self, b):
        return 0 if self.mesh_ids is None else int(self.mesh_ids[b])

    def image_of(self, b):
        return 0 if self.image_ids is None else int(self.image_ids[b])

    def K_of(self, b):
        return self.K[b] if self.K.ndim == 3 else self.K

    def tau_of(self, b):
        return float(self.tau[b]) if np.ndim(self.tau) else float(self.tau)

    def geometry(self, b):
        verts, faces = I.mesh_arrays(self.meshes)
        return verts[self.mesh_of(b)], faces[self.mesh_of(b)]

    def counted(self, b):
        """what the pose kernel decides without the render: the status, the image id, tau as float32"""
        tau = np.float32(self.tau_of(b))
        return (self.status is None or int(self.status[b]) != 0) and 0 <= self.image_of(b) < self.n_img and bool(tau > 0) and bool(np.isfinite(tau))

    def sensor(self, D):
        """the sensor depth (I,H,W) the case is verified against; D: the renders the caller scores (only a tie case reads them)"""
        return tie_depth(D[0], self.tau_of(0))[None] if self.tie else self.depth


def tie_depth(D, tau):
    """a sensor depth with |S - D| == tau EXACTLY in float32 wherever the render allows it: S = D + tau on even columns, D - tau on odd
    ones, kept only where (D + tau) - D == tau resp. D - (D - tau) == tau holds in float32 (elsewhere, and off the model, S = D)"""
    f32 = np.float32
    D, tau = np.asarray(D, f32), f32(tau)
    up, dn = (D + tau).astype(f32), (D - tau).astype(f32)
    even = (np.arange(D.shape[1]) % 2 == 0)[None, :]
    S = np.where(even, np.where((up - D).astype(f32) == tau, up, D), np.where(((D - dn).astype(f32) == tau) & (dn > 0), dn, D))
    return np.where(D > 0, S, D).astype(f32)


_SENSORS = {}


def sensor_depth(mesh, R, t, K, seed):
    """what the sensor saw of one object: render_f32 of the truth pose, a far plane (900) behind it, an occluder slab (150) of three
    columns through the object, and 2 x 4 patches of holes (0), NaN, inf and negative depths on it (cached, read-only)"""
    key = (mesh, seed)
    if key not in _SENSORS:
        v, f = V.meshes()[mesh]
        d = V.render_f32(R, t, K, v, f, SIZE).copy()
        W, H = SIZE
        ys, xs = np.nonzero(d > 0)
        d = np.where(d > 0, d, np.float32(900.0)).astype(np.float32)
        rng = np.random.default_rng(2000 + seed)
        xm, ym = (int(np.median(xs)), int(np.median(ys))) if len(xs) else (W // 2, H // 2)
        x_occ = int(np.clip(xm + rng.integers(4, 9), 0, W - 4))
        d[:, x_occ:x_occ + 3] = np.float32(150.0)
        for k, val in enumerate((0.0, np.nan, np.inf, -5.0)):
            y0, x0 = int(np.clip(ym - 7 + 4 * k, 0, H - 2)), int(np.clip(xm - 9, 0, W - 4))
            d[y0:y0 + 2, x0:x0 + 4] = val
        d.setflags(write=False)
        _SENSORS[key] = d
    return _SENSORS[key]


def _scene(name, seed, layout, K=I.K_A, per_pose_K=False, off_frame=(), tau=8.0, distance=(300.0, 360.0), **kw):
    """layout: per pose (mesh name, image, kind).  Every image holds ONE object at a random truth pose (off_frame: images whose object
    lies partly outside the frame).  kind: "truth"; "near" = 2 degrees and 1.5 % along the ray off it (about 5 mm: matches with every q); "side" = moved a diameter sideways
    (in front of the far plane: through); "gone" = wholly off the frame; "behind" = vertices at Z <= 0.  tau: a number, or "tensor" =
    6, 8, 10, ... per pose"""
    rng = np.random.default_rng(seed)
    names = []
    for m, _, _ in layout:
        if m not in names:
            names.append(m)
    n_img, P = 1 + max(i for _, i, _ in layout), len(layout)
    Ks = np.stack([I.K_A if b % 2 == 0 else I.K_B for b in range(P)]) if per_pose_K else K
    truth, depth = [], []
    for i in range(n_img):
        b0 = [b for b, (_, im, _) in enumerate(layout) if im == i][0]
        Kb = Ks[b0] if per_pose_K else K
        R = I._random_rotation(rng)
        z = rng.uniform(*distance)
        t = np.array([rng.uniform(-20, 20), rng.uniform(-15, 15), z])
        if i in off_frame:
            t[0] = z * (SIZE[0] - 6.0 - Kb[0, 2]) / Kb[0, 0]                   # the object's centre six pixels inside the right edge
        truth.append((R, t))
        depth.append(sensor_depth(layout[b0][0], R, t, Kb, seed * 16 + i))
    Rs, ts = [], []
    for m, i, kind in layout:
        R, t = truth[i]
        if kind != "truth":
            R = I._rodrigues(rng.normal(size=3), np.radians(2.0)) @ R
            t = t * (1.0 + 0.015 * (1.0 if rng.random() < 0.5 else -1.0))
        if kind == "side":
            t = t + np.array([-float(V.diameter(V.meshes()[m][0])), 0.0, 0.0])
        elif kind == "gone":
            t = t + np.array([4.0 * t[2], 0.0, 0.0])
        elif kind == "behind":
            t = np.array([t[0], t[1], 30.0])
        Rs.append(R)
        ts.append(t)
    mesh_ids = None if len(names) == 1 else np.array([names.index(m) for m, _, _ in layout], np.int32)
    image_ids = None if n_img == 1 else np.array([i for _, i, _ in layout], np.int32)
    if isinstance(tau, str):
        tau = 6.0 + 2.0 * np.arange(P)
    return VerifyCase(name, names, mesh_ids, Ks, image_ids, np.stack(Rs), np.stack(ts), np.stack(depth), tau, **kw)


def _edges():
    """0 truth of an object partly off the frame; 1 wholly off the frame (n_model = 0); 2 a vertex behind the camera; 3 status 0;
    4 an image id out of range; 5 NaN in R; 6 a tau of 0; 7 the control (near)"""
    lay = [("torus", 0, "truth"), ("torus", 1, "gone"), ("torus", 1, "behind"), ("torus", 1, "truth"), ("torus", 1, "truth"), ("torus", 1, "near"),
           ("torus", 1, "near"), ("torus", 1, "near")]
    c = _scene("edges_8", 43, lay, off_frame=(0,), tau="tensor")
    c.status = np.ones(8, np.int32)
    c.status[3] = 0
    c.image_ids = c.image_ids.copy()
    c.image_ids[4] = 7
    c.R[5, 1, 2] = np.nan
    c.tau[6] = 0.0
    return c


def _tie():
    """one torus whose sensor depth is its own render +- tau, tau = 4 a power of two: a == tau exactly on (nearly) every model pixel"""
    c = _scene("tie_1", 44, [("torus", 0, "truth")], tau=4.0)
    c.depth, c.tie = None, True
    return c


def _occluder_weight():
    """C = 2, B = 1, occlusion_weight 0.  Candidate 0: a box seen face-on at 320 (front face at 300) that the sensor saw, but for a slab at
    200 over 70 % of its width.  Candidate 1: the same box at 220, its front face IN the slab's plane.  The slab supports candidate 1
    (about half of its pixels match, the others see through to 300 / 900); candidate 0 matches on the rest and is occluded under the slab:
    at weight 0 it wins (1 against about 0.5), at weight 1 it loses (0.3)"""
    K = I.K_A
    v, f = V.meshes()["box"]
    R, tA, tB = np.eye(3), np.array([2.0, 1.0, 320.0]), np.array([2.0, 1.0, 220.0])
    d = V.render_f32(R, tA, K, v, f, SIZE).copy()
    xs = np.nonzero((d > 0).any(0))[0]
    d = np.where(d > 0, d, np.float32(900.0)).astype(np.float32)
    x0, x1 = int(xs.min()), int(xs.max())
    d[:, x0:x0 + int(round(0.7 * (x1 - x0 + 1)))] = np.float32(200.0)
    return VerifyCase("occluder_weight", ("box",), None, K, None, np.stack([R, R]), np.stack([tA, tB]), d[None], 6.0, occlusion_weight=0.0, cand=(2, 1))


def _tie_select():
    """C = 3, B = 2 over one image: candidates near, truth, truth -- candidates 1 and 2 are the same pose, an exact tie of the best score;
    crop 1 has status 0: no candidate is eligible, candidate 0 it is"""
    s = _scene("tie_select", 45, [("ico80", 0, "near"), ("ico80", 0, "near"), ("ico80", 0, "truth"), ("ico80", 0, "truth"), ("ico80", 0, "truth"),
                                   ("ico80", 0, "truth")])
    s.cand, s.status = (3, 2), np.array([1, 0] * 3, np.int32)
    return s


def _refined(key, name, idx, tau):
    """C = 2 over the poses idx of a tests/icp_stages.py case: its start poses, then the poses its restatement refines them to on a CPU"""
    case = I.make(name)
    smp = I.case_samples(case)
    _, R1, t1, _, _ = I.restatement_outputs(case, smp)
    idx = np.asarray(idx)
    pick = lambda a: None if a is None else np.concatenate([np.asarray(a)[idx]] * 2)                 # noqa: E731
    return VerifyCase(key, case.meshes, pick(case.mesh_ids), np.concatenate([case.K[idx]] * 2) if case.K.ndim == 3 else case.K,
                      pick(case.image_ids), np.concatenate([case.R0[idx], R1[idx]]), np.concatenate([case.t0[idx], t1[idx]]), case.depth, tau,
                      cand=(2, len(idx)))


CASES = {
    "torus_1": lambda: _scene("torus_1", 40, [("torus", 0, "near")]),
    "mixed_3": lambda: _scene("mixed_3", 41, [("torus", 0, "truth"), ("box", 1, "near"), ("torus", 0, "side")], per_pose_K=True, tau="tensor",
                              occlusion_weight=0.5),
    "mixed_5": lambda: _scene("mixed_5", 42, [("ico80", 0, "near"), ("torus", 1, "near"), ("ico80", 0, "truth"), ("box", 2, "side"), ("torus", 1, "truth")],
                              occlusion_weight=0.0),
    "edges_8": _edges,
    "tie_1": _tie,
    "occluder_weight": _occluder_weight,
    "tie_select": _tie_select,
}
# The selection cases (C = 2: the start pose, then tests/icp_stages.py's CPU refinement of it): name -> (icp case, poses, tau, the
# candidate every crop chooses).  In the CONVERGING ones the refined pose outscores the start pose on every crop by at least 0.05 under
# the numpy rule alone; in the triangle (drifting) ones the start pose scores at least as high (tests/test_pose_verify.py asserts both
# and prints the gaps):
#   triangle_3_g17, poses 0 and 2 at tau = 128: a tolerance beyond the triangle's size, so the score is in effect the share of the
#     silhouette the sensor supports -- N24 slid the triangle in its plane, off the silhouette (through 32 -> 89 and 1 -> 59 pixels): the
#     start pose leads by 0.09 and 0.07.  (At tau <= 32 the rule prefers the refined poses, whose ADD is also the lower one: 11.9 against
#     13.3, 9.9 against 13.1 -- "drifting" there means short of a quarter of the start's ADD, not worse than it.  Pose 1 is left out: its
#     refined pose leads at every tau tried.)
#   triangle_1_g8: fewer than six samples, N24 passes the pose through bitwise: the scores are EQUAL and the tie goes to candidate 0.
SELECTION = {
    "select_torus_1_g8": ("torus_1_g8", (0,), 8.0, 1),
    "select_box_3_g17": ("box_3_g17", (0, 1, 2), 8.0, 1),
    "select_halfbox_3_g32": ("halfbox_3_g32", (0, 1, 2), 8.0, 1),
    "select_triangle_3_g17": ("triangle_3_g17", (0, 2), 128.0, 0),
    "select_triangle_1_g8": ("triangle_1_g8", (0,), 8.0, 0),
}
_CASES = {}


def make(name):
    if name not in _CASES:
        _CASES[name] = _refined(name, *SELECTION[name][:3]) if name in SELECTION else CASES[name]()
    return _CASES[name]


# ------------------------------------------------------------------------------------------------------------------- the checker
def rendered(case, b):
    """the render rule's own refusals, in float64: a non-finite pose or K, a mesh id out of range, a vertex at Z <= 0"""
    R, t, K = case.R[b], case.t[b], case.K_of(b)
    if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(K).all()) or not 0 <= case.mesh_of(b) < len(case.meshes):
        return False
    v, _ = case.geometry(b)
    return bool(((v.astype(np.float64) @ R[2] + t[2]) > 0).all())


_RENDERS = {}


def cpu_renders(case):
    """render_f32 of every pose (zeros where the rule renders nothing) -> (P,H,W) float32; cached, read-only"""
    if case.name not in _RENDERS:
        W, H = case.size
        D = np.zeros((case.P, H, W), np.float32)
        for b in range(case.P):
            if rendered(case, b) and case.counted(b):
                v, f = case.geometry(b)
                D[b] = V.render_f32(case.R[b], case.t[b], case.K_of(b), v, f, case.size)
        D.setflags(write=False)
        _RENDERS[case.name] = D
    return _RENDERS[case.name]


def reference(case, D, tamper=()):
    """the rule applied to renders D (P,H,W) -> dict: counts (P,6) int32, score, fit, den (P,) float64, ok (P,) bool, labels (P,H,W)
    uint8, choice (B,) int32 or None"""
    D = np.asarray(D, np.float32)
    S = case.sensor(D)
    out = dict(counts=np.zeros((case.P, 6), np.int32), score=np.zeros(case.P), fit=np.zeros(case.P), den=np.zeros(case.P),
               ok=np.zeros(case.P, bool), labels=np.zeros(D.shape, np.uint8), choice=None)
    for b in range(case.P):
        counted = case.counted(b)
        if counted:
            out["labels"][b], q = classify(D[b], S[case.image_of(b)], case.tau_of(b), tamper)
            out["counts"][b] = counts_of(out["labels"][b], q)
        out["score"][b], out["fit"][b], out["den"][b], out["ok"][b] = score_of(out["counts"][b], case.occlusion_weight, counted, tamper)
    if case.cand is not None:
        out["choice"] = select(out["score"].reshape(case.cand), out["ok"].reshape(case.cand), tamper)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_case(case, D, out, log=None):
    """out: dict as reference() returns it (labels and choice may be None: not checked then), e.g. the device's outputs for the renders D.
    StageError naming the stage -- "counts", "labels", "fit", "den", "ok", "score", "choice" -- and the pose"""
    want = reference(case, D)
    for stage in ("counts", "labels", "ok", "choice"):
        if out.get(stage) is None or want[stage] is None:
            continue
        got = np.asarray(out[stage])
        if got.shape != want[stage].shape or not np.array_equal(got, want[stage]):
            bad = np.nonzero((got != want[stage]).reshape(len(got), -1).any(1))[0] if got.shape == want[stage].shape else [-1]
            b = int(bad[0])
            raise StageError(stage, b, None, "got %s, expected %s" % ((got[b].tolist(), want[stage][b].tolist()) if stage != "labels" and b >= 0
                                                                        else ("%d pixels differ" % int((got != want[stage]).sum()), "none")))
    for stage in ("fit", "den", "score"):
        got = np.asarray(out[stage], np.float64)
        if got.shape != want[stage].shape or not np.array_equal(_bits(got), _bits(want[stage])):
            b = int(np.nonzero(_bits(got) != _bits(want[stage]))[0][0]) if got.shape == want[stage].shape else -1
            raise StageError(stage, b, None, "got %r, expected %r" % (float(got[b]), float(want[stage][b])))
    if log is not None:
        log("%-22s counts %s score %s%s" % (case.name, want["counts"].tolist(), np.round(want["score"], 4).tolist(),
                                           "" if want["choice"] is None else " choice %s" % want["choice"].tolist()))
    return want


if __name__ == "__main__":
    import sys
    for name in (sys.argv[1:] or list(CASES) + list(SELECTION)):
        c = make(name)
        check_case(c, cpu_renders(c), reference(c, cpu_renders(c)), log=lambda s: print(s, flush=True))
