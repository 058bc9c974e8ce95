"""Row N28 (hypothesis verification against predicted masks), the rule the device is pinned by.  Not a test file: the rule of
csrc/pose_verify_mask.hip in numpy, the committed cases, the checker and its tamperings.  Nothing here reads the reference (it does
not verify); the meshes and the CPU render are tests/vsd_stages.py's, the cameras and the pose makers tests/icp_stages.py's.

  pack(masks)                     cp_coco_pack's layout: dense (N,H,W) bool -> int32 words (N,H,WW), WW = ceil(W / 32), pixel x = bit x & 31
                                  of word x >> 5
  read(bits, H, W)                the kernel's reading of those words back into dense masks (where the layout tamperings act)
  counts_of, box_of, finish, labels_of      the integer sums, the silhouette's box, the float64 finish, the label map
  select                          tests/verify_stages.py's (row N26's choice, unchanged)
  reference(case, D)              a case's expected outputs from renders D (P,H,W) -- render_f32's on a CPU, metric.render_depth's on the device
  check_case(case, D, out)        every output EQUAL to the reference's (counts, box, labels, ok, choice) or the same bits (iou, cover, score)

The rule.  Per pose p with mask row m = mask_ids[p] (m = p without ids): D = the pose's depth render over the masks' W x H frame; a pixel
is a model pixel iff D > 0; F = the full mask m, V = the optional visible mask m.  n_model = |D > 0|, n_inter = |model and F|, n_vis_in =
|model and V| (0 without visible); n_mask = full.area[m], n_vis = visible.area[m] are read, not recounted (both 0 for a mask id outside
0..N-1, n_vis 0 without visible); box = xmin ymin xmax ymax of the model pixels, -1 four times when n_model == 0.  In float64: union =
n_model + n_mask - n_inter (integers), iou = n_inter / union, cover = n_vis_in / n_vis, score = iou.  score and iou are NaN with ok = 0
when union == 0 or the pose is not counted (sums 0, box -1s): a non-finite pose or K, a vertex at Z <= 0, a mesh id out of range, a mask
id outside 0..N-1, status 0.  cover is NaN when n_vis == 0, without visible, or when the pose is not counted.  Labels: model | F << 1 |
V << 2; a pose that is not counted still gets its mask bits (zeros for an invalid mask id)."""
import numpy as np

from tests import icp_stages as I
from tests import verify_stages as VS
from tests import vsd_stages as V
from tests.pnp_stages import StageError

SIZE_A = (96, 80)                                  # (W, H): 3 x 3 tiles, the right and bottom ones partial
SIZE_B = (70, 50)                                  # a partial last word (70 = 2 * 32 + 6) and partial tiles on both axes
K_S = np.array([[90.0, 0.0, 34.3], [0.0, 88.0, 25.6], [0.0, 0.0, 1.0]])          # cameras of the small frame
K_T = np.array([[93.0, 0.0, 35.7], [0.0, 91.0, 24.2], [0.0, 0.0, 1.0]])
COUNTS = ("n_model", "n_inter", "n_vis_in", "n_mask", "n_vis")
MODEL, FULL, VISIBLE = 1, 2, 4
TAMPERINGS = ("bit_reverse", "floor_stride", "union_no_inter", "vis_area", "ignore_mask_ids", "ge_zero")
select = VS.select


# ------------------------------------------------------------------------------------------------------------------- the rule
def pack(masks):
    """dense (N,H,W) bool -> (N,H,WW) int32: cp_coco_pack's layout"""
    m = np.asarray(masks, bool)
    N, H, W = m.shape
    WW = (W + 31) // 32
    pad = np.zeros((N, H, WW * 32), np.uint64)
    pad[:, :, :W] = m
    words = (pad.reshape(N, H, WW, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return words.astype(np.uint32).view(np.int32)


def read(bits, H, W, tamper=()):
    """the words as the kernel reads them -> dense (N,H,W) bool.  tamper: "bit_reverse" (bit 31 - (x & 31)), "floor_stride" (rows
    floor(W / 32) words apart), for the checker's own test"""
    bits = np.ascontiguousarray(bits).view(np.uint32)
    N = bits.shape[0]
    WW = (W + 31) // 32
    flat = bits.reshape(-1)
    stride = W // 32 if "floor_stride" in tamper else WW
    n, y, x = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
    word = flat[np.minimum((n * H + y) * stride + (x >> 5), flat.size - 1)] if flat.size else np.zeros(n.shape, np.uint32)
    bit = (31 - (x & 31)) if "bit_reverse" in tamper else (x & 31)
    return ((word >> bit.astype(np.uint32)) & 1).astype(bool)


def counts_of(D, F, Vm=None, tamper=()):
    """-> (n_model, n_inter, n_vis_in) of one pose; D (H,W) float32, F, Vm (H,W) bool"""
    D = np.asarray(D, np.float32)
    model = (D >= 0) if "ge_zero" in tamper else (D > 0)
    return int(model.sum()), int((model & F).sum()), (0 if Vm is None else int((model & Vm).sum()))


def box_of(D, tamper=()):
    D = np.asarray(D, np.float32)
    ys, xs = np.nonzero((D >= 0) if "ge_zero" in tamper else (D > 0))
    return [-1] * 4 if len(xs) == 0 else [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def finish(n_model, n_inter, n_vis_in, n_mask, n_vis, counted=True, tamper=()):
    """-> (score, iou, cover, ok) in float64, every operation rounded on its own"""
    nan = np.float64(np.nan)
    union = int(n_model) + int(n_mask) - (0 if "union_no_inter" in tamper else int(n_inter))
    ok = bool(counted) and union != 0
    iou = np.float64(int(n_inter)) / np.float64(union) if ok else nan
    cover = np.float64(int(n_vis_in)) / np.float64(int(n_vis)) if counted and int(n_vis) != 0 else nan
    return iou, iou, cover, ok


def labels_of(D, F, Vm, counted, tamper=()):
    D = np.asarray(D, np.float32)
    model = ((D >= 0) if "ge_zero" in tamper else (D > 0)) & bool(counted)
    lab = model.astype(np.uint8) * MODEL
    if F is not None:
        lab |= F.astype(np.uint8) * FULL
    if Vm is not None:
        lab |= Vm.astype(np.uint8) * VISIBLE
    return lab


# ------------------------------------------------------------------------------------------------------------------- the cases
class MaskCase:
    """size (W, H); meshes: names into vsd_stages.meshes(); mesh_ids (P,) or None; K (3,3) or (P,3,3); R (P,3,3), t (P,3): the poses,
    candidate-major when cand = (C, B); full: one maker per mask row -- a dense (H,W) bool array, or ("own", p): the silhouette of pose
    p's render, whoever made it --; holes (N,) list of column ranges (x0, x1) cut out of the full mask to give the visible one, or None:
    no visible masks; mask_ids (P,) or None (then N == P); status (P,) int32 or None"""

    def __init__(self, name, size, meshes, mesh_ids, K, R, t, full, holes=None, mask_ids=None, status=None, cand=None):
        self.name, self.size, self.meshes, self.mesh_ids, self.K = name, size, tuple(meshes), mesh_ids, np.asarray(K, np.float64)
        self.R, self.t, self.full, self.holes, self.mask_ids, self.status, self.cand = R, t, list(full), holes, mask_ids, status, cand
        self.P, self.N = len(R), len(full)

    def mesh_of(self, b):
        return 0 if self.mesh_ids is None else int(self.mesh_ids[b])

    def mask_of(self, b, tamper=()):
        return b % self.N if self.mask_ids is None or "ignore_mask_ids" in tamper else int(self.mask_ids[b])

    def K_of(self, b):
        return self.K[b] if self.K.ndim == 3 else self.K

    def geometry(self, b):
        verts, faces = I.mesh_arrays(self.meshes)
        return verts[self.mesh_of(b)], faces[self.mesh_of(b)]

    def rendered(self, b):
        """the render rule's own refusals, in float64: a non-finite pose or K, a mesh id out of range, a vertex at Z <= 0"""
        R, t, K = self.R[b], self.t[b], self.K_of(b)
        if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(K).all()) or not 0 <= self.mesh_of(b) < len(self.meshes):
            return False
        v, _ = self.geometry(b)
        return bool(((v.astype(np.float64) @ R[2] + t[2]) > 0).all())

    def counted(self, b, tamper=()):
        return self.rendered(b) and (self.status is None or int(self.status[b]) != 0) and 0 <= self.mask_of(b, tamper) < self.N

    def masks(self, D):
        """the dense masks (full (N,H,W) bool, visible (N,H,W) bool or None) the case is verified against; D: the renders the caller
        scores (only an "own" row reads them)"""
        full = np.stack([(np.asarray(D[m[1]]) > 0) if isinstance(m, tuple) else np.asarray(m, bool) for m in self.full])
        if self.holes is None:
            return full, None
        vis = full.copy()
        for n, (x0, x1) in enumerate(self.holes):
            vis[n, :, x0:x1] = False
        return full, vis


_SILS = {}


def silhouette(mesh, R, t, K, size):
    """render_f32's silhouette of one pose (cached by its bytes, read-only)"""
    key = (mesh, size, np.asarray(R).tobytes(), np.asarray(t).tobytes(), np.asarray(K).tobytes())
    if key not in _SILS:
        v, f = V.meshes()[mesh]
        s = V.render_f32(R, t, K, v, f, size) > 0
        s.setflags(write=False)
        _SILS[key] = s
    return _SILS[key]


def checkerboard(size, cell=3):
    W, H = size
    y, x = np.mgrid[0:H, 0:W]
    return ((x // cell + y // cell) % 2 == 0)


def _poses(seed, layout, Ks, size, distance=(300.0, 360.0)):
    """layout: per pose (mesh name, object, kind).  Every object has ONE random truth pose; kind: "truth"; "near" = 4 degrees and 6 %
    sideways of the distance off it (a partial overlap with the truth's silhouette); "edge" = the truth moved so that its centre lies six
    pixels inside the right edge; "gone" = wholly off the frame; "behind" = vertices at Z <= 0.  -> (R (P,3,3), t (P,3), truth per object)"""
    rng = np.random.default_rng(seed)
    truth = {}
    Rs, ts = [], []
    for b, (m, obj, kind) in enumerate(layout):
        Kb = Ks[b] if np.ndim(Ks) == 3 else Ks
        if obj not in truth:
            z = rng.uniform(*distance)
            truth[obj] = (I._random_rotation(rng), np.array([rng.uniform(-20, 20), rng.uniform(-12, 12), z]), m, Kb)
        R, t = truth[obj][0], truth[obj][1]
        if kind in ("near", "edge_near"):
            R = I._rodrigues(rng.normal(size=3), np.radians(4.0)) @ R
            t = t + np.array([0.06 * t[2] * (1.0 if rng.random() < 0.5 else -1.0), 0.03 * t[2], 0.0])
        if kind in ("edge", "edge_near"):
            t = t.copy()
            t[0] += t[2] * (size[0] - 6.0 - Kb[0, 2]) / Kb[0, 0] - truth[obj][1][0]
        elif kind == "gone":
            t = t + np.array([4.0 * t[2], 0.0, 0.0])
        elif kind == "behind":
            t = np.array([t[0], t[1], 10.0])                                 # (every committed mesh reaches 15 from its centre on every axis)
        Rs.append(R)
        ts.append(t)
    return np.stack(Rs), np.stack(ts), truth


def _truth_mask(truth, obj, size, shift=(0, 0)):
    R, t, m, K = truth[obj]
    s = silhouette(m, R, t, K, size)
    return np.roll(s, shift, (1, 0)) if shift != (0, 0) else s


def _mixed_a():
    """(96, 80), three meshes with mesh_ids, per-pose K, visible masks, SHARED and PERMUTED mask ids over four masks: 0 the torus's
    truth silhouette, 1 a checkerboard, 2 the full frame, 3 the box's truth silhouette"""
    lay = [("torus", 0, "near"), ("box", 1, "near"), ("ico80", 2, "truth"), ("torus", 0, "truth"), ("box", 1, "truth"), ("ico80", 2, "near")]
    Ks = np.stack([I.K_A if b % 2 == 0 else I.K_B for b in range(len(lay))])
    R, t, truth = _poses(140, lay, Ks, SIZE_A)
    W, H = SIZE_A
    full = [_truth_mask(truth, 0, SIZE_A), checkerboard(SIZE_A), np.ones((H, W), bool), _truth_mask(truth, 1, SIZE_A)]
    return MaskCase("mixed_a_6", SIZE_A, ("torus", "box", "ico80"), np.array([0, 1, 2, 0, 1, 2], np.int32), Ks, R, t, full,
                    holes=[(44, 52), (10, 40), (0, 33), (50, 58)], mask_ids=np.array([0, 3, 1, 2, 3, 1], np.int32))


def _mixed_b():
    """(70, 50), no visible masks, no mask ids (N == P): 0 the pose's OWN silhouette (iou exactly 1), 1 the truth's silhouette under a
    near pose, 2 an EMPTY mask, 3 a ONE-PIXEL mask at the frame's last column (bit 5 of the partial last word), 4 a checkerboard"""
    lay = [("torus", 0, "truth"), ("torus", 0, "near"), ("ico80", 1, "truth"), ("box", 2, "edge"), ("ico80", 1, "near")]
    R, t, truth = _poses(141, lay, K_S, SIZE_B)
    W, H = SIZE_B
    one = np.zeros((H, W), bool)
    ys = np.nonzero(silhouette("box", R[3], t[3], K_S, SIZE_B)[:, W - 1])[0]
    one[int(ys[len(ys) // 2]) if len(ys) else H // 2, W - 1] = True
    full = [("own", 0), _truth_mask(truth, 0, SIZE_B), np.zeros((H, W), bool), one, checkerboard(SIZE_B, 2)]
    return MaskCase("mixed_b_5", SIZE_B, ("torus", "ico80", "box"), np.array([0, 0, 1, 2, 1], np.int32), K_S, R, t, full)


def _edges(name, size, Ks, seed):
    """0 a near pose partly off the frame; 1 wholly off the frame (n_model = 0: iou 0 with ok = 1); 2 a vertex behind the camera; 3
    status 0; 4 a mask id out of range; 5 NaN in R; 6 a mesh id out of range; 7 the control (near); 8 a full-frame mask.  Visible masks."""
    lay = [("torus", 0, "edge_near"), ("torus", 1, "gone"), ("torus", 1, "behind"), ("torus", 1, "truth"), ("torus", 1, "truth"), ("torus", 1, "near"),
           ("torus", 1, "near"), ("torus", 1, "near"), ("torus", 1, "truth")]
    R, t, truth = _poses(seed, lay, Ks, size)
    W, H = size
    te = truth[0][1].copy()
    te[0] = te[2] * (W - 6.0 - Ks[0, 2]) / Ks[0, 0]                                # object 0's truth, its centre six pixels inside the right edge
    edge = silhouette("torus", truth[0][0], te, Ks, size)
    c = MaskCase(name, size, ("torus",), np.zeros(9, np.int32), Ks, R, t, [edge, _truth_mask(truth, 1, size), np.ones((H, W), bool)],
                 holes=[(W - 12, W - 5), (W // 2, W // 2 + 5), (3, 40)], mask_ids=np.array([0, 1, 1, 1, 9, 1, 1, 1, 2], np.int32),
                 status=np.array([1, 1, 1, 0, 1, 1, 1, 1, 1], np.int32))
    c.R[5, 1, 2] = np.nan
    c.mesh_ids[6] = 4
    return c


def _select_a():
    """C = 3, B = 2 on (96, 80): candidates near, truth, truth -- candidates 1 and 2 are the same pose, an exact tie of the best score;
    crop 1 has status 0: no candidate is eligible, candidate 0 it is.  The masks are the crops' truth silhouettes moved one pixel."""
    lay = [("ico80", 0, "near"), ("box", 1, "near"), ("ico80", 0, "truth"), ("box", 1, "truth"), ("ico80", 0, "truth"), ("box", 1, "truth")]
    R, t, truth = _poses(142, lay, I.K_A, SIZE_A)
    full = [_truth_mask(truth, 0, SIZE_A, (1, 0)), _truth_mask(truth, 1, SIZE_A, (0, 1))]
    return MaskCase("select_a", SIZE_A, ("ico80", "box"), np.array([0, 1] * 3, np.int32), I.K_A, R, t, full, holes=[(40, 46), (50, 55)],
                    mask_ids=np.array([0, 1] * 3, np.int32), status=np.array([1, 0] * 3, np.int32), cand=(3, 2))


def _select_b():
    """C = 2, B = 2 on (70, 50), per-pose K: the near pose against the truth, masks = the truths' silhouettes moved one pixel: the truth wins"""
    lay = [("torus", 0, "near"), ("ico80", 1, "truth"), ("torus", 0, "truth"), ("ico80", 1, "near")]
    Ks = np.stack([K_S, K_T, K_S, K_T])
    R, t, truth = _poses(143, lay, Ks, SIZE_B)
    full = [_truth_mask(truth, 0, SIZE_B, (0, 1)), _truth_mask(truth, 1, SIZE_B, (1, 0))]
    return MaskCase("select_b", SIZE_B, ("torus", "ico80"), np.array([0, 1] * 2, np.int32), Ks, R, t, full, mask_ids=np.array([0, 1] * 2, np.int32),
                    cand=(2, 2))


CASES = {
    "mixed_a_6": _mixed_a,
    "mixed_b_5": _mixed_b,
    "edges_a_9": lambda: _edges("edges_a_9", SIZE_A, I.K_A, 144),
    "edges_b_9": lambda: _edges("edges_b_9", SIZE_B, K_S, 145),
    "select_a": _select_a,
    "select_b": _select_b,
}
# the case whose outputs each tampering changes (tests/test_verify_mask.py asserts it): floor_stride needs the frame whose width is no
# multiple of 32, vis_area a case with visible masks, ignore_mask_ids permuted ids, ge_zero any render with background
CAUGHT_BY = {"bit_reverse": "mixed_a_6", "floor_stride": "mixed_b_5", "union_no_inter": "mixed_a_6", "vis_area": "mixed_a_6",
             "ignore_mask_ids": "mixed_a_6", "ge_zero": "mixed_b_5"}
_CASES = {}


def make(name):
    if name not in _CASES:
        _CASES[name] = CASES[name]()
    return _CASES[name]


# ------------------------------------------------------------------------------------------------------------------- the checker
_RENDERS = {}


def cpu_renders(case):
    """render_f32 of every pose (zeros where the rule renders nothing) -> (P,H,W) float32; cached, read-only"""
    if case.name not in _RENDERS:
        W, H = case.size
        D = np.zeros((case.P, H, W), np.float32)
        for b in range(case.P):
            if case.rendered(b):
                v, f = case.geometry(b)
                D[b] = V.render_f32(case.R[b], case.t[b], case.K_of(b), v, f, case.size)
        D.setflags(write=False)
        _RENDERS[case.name] = D
    return _RENDERS[case.name]


def reference(case, D, tamper=()):
    """the rule applied to renders D (P,H,W) -> dict: counts (P,5) int32, box (P,4) int32, score, iou, cover (P,) float64, ok (P,) bool,
    labels (P,H,W) uint8, choice (B,) int32 or None"""
    D = np.asarray(D, np.float32)
    W, H = case.size
    dense_f, dense_v = case.masks(D)
    area_f = dense_f.reshape(case.N, -1).sum(1).astype(np.int64)                  # PackedMasks.area: pinned by rows N15 and N27
    area_v = None if dense_v is None else dense_v.reshape(case.N, -1).sum(1).astype(np.int64)
    F = read(pack(dense_f), H, W, tamper)
    Vm = None if dense_v is None else read(pack(dense_v), H, W, tamper)
    P = case.P
    out = dict(counts=np.zeros((P, 5), np.int32), box=np.full((P, 4), -1, np.int32), score=np.zeros(P), iou=np.zeros(P), cover=np.zeros(P),
               ok=np.zeros(P, bool), labels=np.zeros(D.shape, np.uint8), choice=None)
    for b in range(P):
        m = case.mask_of(b, tamper)
        have = 0 <= m < case.N
        counted = case.counted(b, tamper)
        n = [0, 0, 0]
        if counted:
            n = list(counts_of(D[b], F[m], None if Vm is None else Vm[m], tamper))
            out["box"][b] = box_of(D[b], tamper)
        n_mask = int((area_v if "vis_area" in tamper and area_v is not None else area_f)[m]) if have else 0
        n_vis = int(area_v[m]) if have and area_v is not None else 0
        out["counts"][b] = n + [n_mask, n_vis]
        out["score"][b], out["iou"][b], out["cover"][b], out["ok"][b] = finish(n[0], n[1], n[2], n_mask, n_vis, counted, tamper)
        out["labels"][b] = labels_of(D[b], F[m] if have else None, Vm[m] if have and Vm is not None else None, counted, tamper)
    if case.cand is not None:
        out["choice"] = select(out["score"].reshape(case.cand), out["ok"].reshape(case.cand))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_case(case, D, out, log=None):
    """out: dict as reference() returns it (labels and choice may be None: not checked then), e.g. the device's outputs for the renders D.
    StageError naming the stage -- "counts", "box", "labels", "ok", "choice", "iou", "cover", "score" -- and the pose"""
    want = reference(case, D)
    for stage in ("counts", "box", "labels", "ok", "choice"):
        if out.get(stage) is None or want[stage] is None:
            continue
        got = np.asarray(out[stage])
        if got.shape != want[stage].shape or not np.array_equal(got, want[stage]):
            bad = np.nonzero((got != want[stage]).reshape(len(got), -1).any(1))[0] if got.shape == want[stage].shape else [-1]
            b = int(bad[0])
            raise StageError(stage, b, None, "got %s, expected %s" % ((got[b].tolist(), want[stage][b].tolist()) if stage != "labels" and b >= 0
                                                                        else ("%d pixels differ" % int((got != want[stage]).sum()), "none")))
    for stage in ("iou", "cover", "score"):
        got = np.asarray(out[stage], np.float64)
        if got.shape != want[stage].shape or not np.array_equal(_bits(got), _bits(want[stage])):
            b = int(np.nonzero(_bits(got) != _bits(want[stage]))[0][0]) if got.shape == want[stage].shape else -1
            raise StageError(stage, b, None, "got %r, expected %r" % (float(got[b]), float(want[stage][b])))
    if log is not None:
        log("%-12s counts %s iou %s%s" % (case.name, want["counts"].tolist(), np.round(want["iou"], 4).tolist(),
                                         "" if want["choice"] is None else " choice %s" % want["choice"].tolist()))
    return want


def nontrivial(case, D):
    """the poses with 0 < n_inter < min(n_model, n_mask): a pass cannot come from trivial counts"""
    n = reference(case, D)["counts"].astype(np.int64)
    return np.nonzero((n[:, 1] > 0) & (n[:, 1] < np.minimum(n[:, 0], n[:, 3])))[0]


if __name__ == "__main__":
    import sys
    for name in (sys.argv[1:] or list(CASES)):
        c = make(name)
        check_case(c, cpu_renders(c), reference(c, cpu_renders(c)), log=lambda s: print(s, flush=True))
        print("   nontrivial poses", nontrivial(c, cpu_renders(c)).tolist(), flush=True)
