"""Row N31 (the poses of an image verified together against the visible masks), the rule the device is pinned by.  Not a test file: the
rule of csrc/scene_verify_mask.hip in numpy, the committed cases, the checker and its tamperings.  Nothing here reads the reference (it
does not verify); the meshes, the CPU render, dist_image and the 'bop19' test are tests/vsd_stages.py's, the cameras tests/icp_stages.py's
and tests/verify_mask_stages.py's, the packed layout and row N28's finish tests/verify_mask_stages.py's.

  slots_of(image_ids, I)          the rank of every pose among the poses of its image, in the order given (-1: image id out of range)
  composite(Ds)                   ren and its owner from the renders of an image's counted poses, in slot order
  predicted_visible(D, ren, K, delta)   the model pixels of a pose that the scene leaves visible
  reference(case, D)              a case's expected outputs from renders D (P,H,W) -- render_f32's on a CPU, metric.render_depth's on the device
  check_case(case, D, out)        every output EQUAL to the reference's (integers) or the same bits (the five quotients)

The rule.  Pose p belongs to image image_ids[p] and reads mask row m = mask_ids[p] (m = p without ids) of the full masks F and the
visible masks V.  A pose is COUNTED unless an entry of the pose or of its K is not finite, a vertex is at Z <= 0, its mesh, mask or image
id is out of range, status[p] == 0, or its slot is 32 or more; slot = its rank among the poses of its image in the order given, counted or
not (-1 for an image id out of range).  D_p = the pose's render over the frame; a model pixel has D_p > 0.  ren = the smallest positive
D_p over the counted poses of the image (of equal depths the earlier slot owns the pixel).  A model pixel of p is predicted visible iff
f32(dist_p) - f32(dist_ren) <= f32(delta), both distances vsd_stages.dist_image's under pose p's own K.  n_model = |model|, n_pvis = |pvis|,
n_inter = |model and F|, n_vis_in = |model and V|, n_pvis_in = |pvis and V|, n_mask = area(F_m), n_vis = area(V_m) (read; 0 for a mask id
out of range), n_hidden_seen = n_vis_in - n_pvis_in; box, box_pvis = xmin ymin xmax ymax of the model / pvis pixels, -1s without any.  In
float64, one division each: iou = n_inter / (n_model + n_mask - n_inter) and cover = n_vis_in / n_vis (row N28's, NaN where it gives NaN),
iou_vis = n_pvis_in / (n_pvis + n_vis - n_pvis_in), visib_fract = n_pvis / n_model, score = iou_vis.  iou_vis and score are NaN with ok = 0
when their union is 0 or the pose is not counted; visib_fract is NaN when n_model == 0 or the pose is not counted.  A pose that is not
counted occludes nothing, its sums are 0, its boxes -1s.  Planes (I,H,W) int32: bit s is set where the pose at slot s has a model / a
predicted-visible pixel."""
import numpy as np

from tests import icp_stages as I
from tests import verify_mask_stages as VM
from tests import vsd_stages as V
from tests.pnp_stages import StageError

SIZE_A, SIZE_B, K_S, K_T = VM.SIZE_A, VM.SIZE_B, VM.K_S, VM.K_T
MAX_POSES = 32
COUNTS = ("n_model", "n_pvis", "n_inter", "n_vis_in", "n_pvis_in", "n_mask", "n_vis", "n_hidden_seen")
QUOTIENTS = ("iou", "cover", "iou_vis", "visib_fract", "score")
TAMPERINGS = ("tie_later", "lt_visible", "depth_not_dist", "uncounted_occludes", "swap_fv", "pvis_in_over_model", "ignore_mask_ids",
              "ignore_image_ids")
pack, read, select = VM.pack, VM.read, VM.select


# ------------------------------------------------------------------------------------------------------------------- the rule
def slots_of(image_ids, n_images):
    """-> (P,) int: the number of q < p with image_ids[q] == image_ids[p]; -1 for an image id outside 0..n_images-1"""
    seen, out = {}, []
    for i in (int(v) for v in image_ids):
        if not 0 <= i < n_images:
            out.append(-1)
            continue
        out.append(seen.get(i, 0))
        seen[i] = out[-1] + 1
    return np.array(out, np.int64)


def composite(Ds, tamper=()):
    """Ds: [(slot, D (H,W) float32)] in slot order -> (ren (H,W) float32, owner (H,W) int8: the slot that owns the pixel, -1 none).
    tamper "tie_later": of equal depths the LATER slot owns the pixel"""
    shape = Ds[0][1].shape
    ren, owner = np.zeros(shape, np.float32), np.full(shape, -1, np.int8)
    for s, D in Ds:
        D = np.asarray(D, np.float32)
        take = (D > 0) & ((ren == 0) | ((D <= ren) if "tie_later" in tamper else (D < ren)))
        ren = np.where(take, D, ren)
        owner = np.where(take, np.int8(s), owner)
    return ren, owner


def predicted_visible(D, ren, K, delta, tamper=()):
    """the model pixels of a render D that the composite ren leaves visible: row N19's 'bop19' test on distances.  tamper "lt_visible":
    a strict <; "depth_not_dist": the test on depths"""
    D, ren = np.asarray(D, np.float32), np.asarray(ren, np.float32)
    if "depth_not_dist" in tamper:
        t_own, t_ren = D.astype(np.float64), ren.astype(np.float64)
    else:
        t_own, t_ren = V.dist_image(D, K), V.dist_image(ren, K)
    if "lt_visible" in tamper:
        return ((t_own.astype(np.float32) - t_ren.astype(np.float32) < np.float32(delta)) | (t_ren == 0)) & (t_own > 0)
    return V._visible(t_ren, t_own, delta, "bop19")


def box_of(mask):
    ys, xs = np.nonzero(mask)
    return [-1] * 4 if len(xs) == 0 else [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def finish(n_model, n_pvis, n_inter, n_vis_in, n_pvis_in, n_mask, n_vis, counted=True):
    """-> dict of the five quotients (float64, one division each) and ok"""
    nan = np.float64(np.nan)
    _, iou, cover, _ = VM.finish(n_model, n_inter, n_vis_in, n_mask, n_vis, counted)
    union = int(n_pvis) + int(n_vis) - int(n_pvis_in)
    ok = bool(counted) and union != 0
    iou_vis = np.float64(int(n_pvis_in)) / np.float64(union) if ok else nan
    fract = np.float64(int(n_pvis)) / np.float64(int(n_model)) if counted and int(n_model) != 0 else nan
    return dict(iou=iou, cover=cover, iou_vis=iou_vis, visib_fract=fract, score=iou_vis, ok=ok)


# ------------------------------------------------------------------------------------------------------------------- the cases
class SceneCase:
    """size (W, H); meshes: names into vsd_stages.meshes(); mesh_ids (P,) or None; K (3,3) or (P,3,3); R (P,3,3), t (P,3), candidate-major
    when cand = (C, B); image_ids (P,), n_images; full, visible: dense (N,H,W) bool; mask_ids (P,) or None (then N == P); status (P,) or
    None; delta"""

    def __init__(self, name, size, meshes, mesh_ids, K, R, t, image_ids, n_images, full, visible, delta, mask_ids=None, status=None, cand=None):
        self.name, self.size, self.meshes, self.K = name, size, tuple(meshes), np.asarray(K, np.float64)
        self.mesh_ids = None if mesh_ids is None else np.asarray(mesh_ids, np.int32)
        self.R, self.t = np.array(R, np.float64), np.array(t, np.float64)
        self.image_ids, self.n_images = np.asarray(image_ids, np.int32), int(n_images)
        self.full, self.visible, self.delta = np.asarray(full, bool), np.asarray(visible, bool), float(delta)
        self.mask_ids = None if mask_ids is None else np.asarray(mask_ids, np.int32)
        self.status = None if status is None else np.asarray(status, np.int32)
        self.cand, self.P, self.N = cand, len(self.R), len(self.full)

    def mesh_of(self, b):
        return 0 if self.mesh_ids is None else int(self.mesh_ids[b])

    def mask_of(self, b, tamper=()):
        return b % self.N if self.mask_ids is None or "ignore_mask_ids" in tamper else int(self.mask_ids[b])

    def image_of(self, b, tamper=()):
        return 0 if "ignore_image_ids" in tamper else int(self.image_ids[b])

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

    def slots(self, tamper=()):
        return slots_of([self.image_of(b, tamper) for b in range(self.P)], self.n_images)

    def counted(self, b, tamper=()):
        return (self.rendered(b) and (self.status is None or int(self.status[b]) != 0) and 0 <= self.mask_of(b, tamper) < self.N
                and 0 <= int(self.slots(tamper)[b]) < MAX_POSES)


def _rot(seed):
    return I._random_rotation(np.random.default_rng(seed))


def _near(R, t, seed):
    """4 degrees and 6 % / 3 % of the distance sideways off (R, t)"""
    rng = np.random.default_rng(seed)
    return I._rodrigues(rng.normal(size=3), np.radians(4.0)) @ R, t + np.array([0.06 * t[2], 0.03 * t[2], 0.0])


def _render(mesh, R, t, K, size):
    v, f = V.meshes()[mesh]
    return V.render_f32(R, t, K, v, f, size)


def truth_masks(poses, size, delta):
    """poses: [(mesh, R, t, K)] of ONE image, all counted -> (F (n,H,W) bool: the silhouettes, Vm (n,H,W) bool: what the scene leaves
    visible of each), by the rule itself on render_f32's renders"""
    Ds = [_render(m, R, t, K, size) for m, R, t, K in poses]
    ren, _ = composite(list(enumerate(Ds)))
    return np.stack([D > 0 for D in Ds]), np.stack([predicted_visible(D, ren, p[3], delta) for D, p in zip(Ds, poses)])


def _occlusion(name, size, K, delta, seed):
    """a box at Z = 300 in front of a torus at Z = 340, overlapping; masks = the truth scene's (row 0 the box, row 1 the torus).
    image 0: the truth; image 1: the torus 15 % nearer -- it passes in front of the box; image 2, torus first: the torus 6 % nearer -- still
    behind, interpenetrating"""
    Rb, Rt = _rot(seed), _rot(seed + 1)
    tb, tt = np.array([-8.0, 3.0, 300.0]), np.array([10.0, -4.0, 340.0])
    F, Vm = truth_masks([("box", Rb, tb, K), ("torus", Rt, tt, K)], size, delta)
    R = [Rb, Rt, Rb, Rt, Rt, Rb]
    t = [tb, tt, tb, 0.85 * tt, 0.94 * tt, tb]
    return SceneCase(name, size, ("box", "torus"), [0, 1, 0, 1, 1, 0], K, R, t, [0, 0, 1, 1, 2, 2], 3, F, Vm, delta, mask_ids=[0, 1, 0, 1, 1, 0])


def _hidden_tie():
    """(96, 80), ONE image: a box at Z = 250 twice (identical poses: the tie -- both fully visible, slot 0 owns the composite) and an
    ico80 at Z = 600 twice, wholly behind the boxes: fully hidden, once under an EMPTY visible mask (row 1: iou_vis NaN, ok 0) and once
    under a non-empty one (row 2: iou_vis exactly 0, ok 1)"""
    K = I.K_B
    Rb, tb = I._rodrigues(np.array([0.3, 1.0, 0.2]), 0.25), np.array([2.0, 1.0, 250.0])
    Ri, ti = np.eye(3), np.array([4.0, 2.0, 600.0])
    box, ico = _render("box", Rb, tb, K, SIZE_A) > 0, _render("ico80", Ri, ti, K, SIZE_A) > 0
    return SceneCase("hidden_tie_a", SIZE_A, ("box", "ico80"), [0, 0, 1, 1], K, [Rb, Rb, Ri, Ri], [tb, tb, ti, ti], [0, 0, 0, 0], 1,
                     [box, ico, ico], [box, np.zeros_like(ico), ico], 0.0, mask_ids=[0, 0, 1, 2])


def _crowd(name, extra):
    """(70, 50): image 0 holds EXACTLY 32 small ico80 poses on an 8 x 4 grid (neighbours overlap), image 1 four larger poses; the poses of
    the two images are INTERLEAVED in the order given.  extra: a 33rd pose of image 0 at the end, a box in front of the crowd -- beyond
    the 32nd slot, not counted.  N == P masks without ids: the truth scenes' own"""
    lay, R, t, ids = [], [], [], []
    big = {3: ("box", np.array([-12.0, 4.0, 300.0])), 11: ("torus", np.array([14.0, -3.0, 340.0])), 20: ("box", np.array([30.0, 30.0, 420.0])),
           30: ("torus", np.array([-40.0, -20.0, 500.0]))}
    n = 0
    for b in range(36):
        if b in big:
            lay.append(big[b][0]); R.append(_rot(160 + b)); t.append(big[b][1]); ids.append(1)
            continue
        col, rw = n % 8, n // 8
        z = 1100.0 if (col + rw) % 2 else 1500.0
        u, v = 12.0 + 6.0 * col, 8.0 + 10.0 * rw
        lay.append("ico80"); R.append(_rot(160 + b)); ids.append(0)
        t.append(np.array([(u - K_S[0, 2]) / K_S[0, 0] * z, (v - K_S[1, 2]) / K_S[1, 1] * z, z]))
        n += 1
    F, Vm = np.zeros((36, SIZE_B[1], SIZE_B[0]), bool), np.zeros((36, SIZE_B[1], SIZE_B[0]), bool)
    for img in (0, 1):
        rows = [b for b in range(36) if ids[b] == img]
        F[rows], Vm[rows] = truth_masks([(lay[b], R[b], t[b], K_S) for b in rows], SIZE_B, 15.0)
    if extra:
        lay.append("box"); R.append(_rot(199)); t.append(np.array([0.0, 0.0, 200.0])); ids.append(0)
        s = (_render("box", R[-1], t[-1], K_S, SIZE_B) > 0)[None]
        F, Vm = np.concatenate([F, s]), np.concatenate([Vm, s])
    names = ("ico80", "box", "torus")
    return SceneCase(name, SIZE_B, names, [names.index(m) for m in lay], K_S, R, t, ids, 2, F, Vm, 15.0)


def _mixed():
    """(70, 50), per-pose K, three meshes, SHARED and PERMUTED mask ids over five rows: 0 empty / empty, 1 the full frame / the full frame
    less columns 3..39, 2 ONE pixel at the frame's last column (bit 5 of the partial last word), 3 a checkerboard / its right half, 4 the
    torus's truth silhouette / what image 0's truth leaves visible of it.  Image 0: the torus, a box in front of it, an ico80 partly
    outside the frame, an ico80 wholly outside; image 1: a box and a torus"""
    W, H = SIZE_B
    Ks = np.stack([K_S, K_T, K_S, K_T, K_T, K_S])
    Rt, tt = _rot(171), np.array([6.0, -2.0, 340.0])
    Rb, tb = _rot(172), np.array([-6.0, 4.0, 290.0])
    Ri = _rot(173)
    te = np.array([300.0 * (W - 4.0 - K_S[0, 2]) / K_S[0, 0], 5.0, 300.0])         # its centre four pixels inside the right edge
    tg = np.array([1400.0, 0.0, 300.0])                                            # wholly off the frame
    F4, V4 = truth_masks([("torus", Rt, tt, K_S), ("box", Rb, tb, K_T)], SIZE_B, 15.0)
    one = np.zeros((H, W), bool)
    ys = np.nonzero((_render("ico80", Ri, te, K_S, SIZE_B) > 0)[:, W - 1])[0]
    one[int(ys[len(ys) // 2]) if len(ys) else H // 2, W - 1] = True
    allf, chk = np.ones((H, W), bool), VM.checkerboard(SIZE_B, 2)
    holed, half = allf.copy(), chk.copy()
    holed[:, 3:40] = False
    half[:, :W // 2] = False
    full = [np.zeros((H, W), bool), allf, one, chk, F4[0]]
    vis = [np.zeros((H, W), bool), holed, one, half, V4[0]]
    return SceneCase("mixed_b", SIZE_B, ("torus", "box", "ico80"), [0, 1, 2, 2, 1, 0], Ks, [Rt, Rb, Ri, Ri, _rot(174), _rot(175)],
                     [tt, tb, te, tg, np.array([-4.0, 2.0, 310.0]), np.array([5.0, 0.0, 330.0])], [0, 0, 0, 0, 1, 1], 2, full, vis, 15.0,
                     mask_ids=[4, 3, 1, 2, 0, 3])


WAYS = ("nan_pose", "nan_K", "behind", "mesh_id", "mask_id", "status", "image_id")


def _uncounted():
    """(96, 80), per-pose K.  Image k (k = 0 .. 6): an intruder that is NOT counted in way WAYS[k] -- a box at Z = 200, in FRONT --, then a
    counted torus at Z = 340; image 7: the same torus alone (pose 14).  Every torus must come out as pose 14 does.  The intruder of way
    "image_id" names image 99.  Row 0: the torus's silhouette / the same less columns 44..51, row 1: the box's silhouette"""
    K = I.K_A
    Rt, tt = _rot(181), np.array([4.0, -2.0, 340.0])
    Rb, tb = _rot(182), np.array([0.0, 0.0, 200.0])
    R, t, ids, mesh, mask, status = [], [], [], [], [], []
    for k in range(len(WAYS)):
        R += [Rb.copy(), Rt]; t += [tb.copy(), tt]; ids += [k, k]; mesh += [0, 1]; mask += [1, 0]; status += [1, 1]
    R.append(Rt); t.append(tt); ids.append(7); mesh.append(1); mask.append(0); status.append(1)
    Ks = np.stack([K] * 15)
    R[0][1, 2] = np.nan
    Ks[2, 0, 0] = np.inf
    t[4] = np.array([0.0, 0.0, 10.0])
    mesh[6], mask[8], status[10], ids[12] = 5, 9, 0, 99
    sil_t, sil_b = _render("torus", Rt, tt, K, SIZE_A) > 0, _render("box", Rb, tb, K, SIZE_A) > 0
    vis_t = sil_t.copy()
    vis_t[:, 44:52] = False
    return SceneCase("uncounted_a", SIZE_A, ("box", "torus"), mesh, Ks, R, t, ids, 8, [sil_t, sil_b], [vis_t, sil_b], 15.0, mask_ids=mask, status=status)


def _select():
    """C = 3, B = 2 on (96, 80), ONE frame: stage c of both crops is scene c (image_ids = c).  Candidates near, truth, truth -- candidates
    1 and 2 are the same scene, an exact tie of the best score: the choice is 1 for both crops.  The masks are the truth scene's"""
    K = I.K_A
    Rb, Rt = _rot(191), _rot(192)
    tb, tt = np.array([-8.0, 3.0, 300.0]), np.array([10.0, -4.0, 340.0])
    F, Vm = truth_masks([("box", Rb, tb, K), ("torus", Rt, tt, K)], SIZE_A, 15.0)
    nb, nt = _near(Rb, tb, 193), _near(Rt, tt, 194)
    return SceneCase("select_a", SIZE_A, ("box", "torus"), [0, 1] * 3, K, [nb[0], nt[0], Rb, Rt, Rb, Rt], [nb[1], nt[1], tb, tt, tb, tt],
                     [0, 0, 1, 1, 2, 2], 3, F, Vm, 15.0, mask_ids=[0, 1] * 3, cand=(3, 2))


CASES = {
    "occl_a": lambda: _occlusion("occl_a", SIZE_A, I.K_A, 1.0, 151),
    "occl_b_d0": lambda: _occlusion("occl_b_d0", SIZE_B, K_S, 0.0, 153),
    "occl_b_d15": lambda: _occlusion("occl_b_d15", SIZE_B, K_S, 15.0, 153),
    "occl_b_big": lambda: _occlusion("occl_b_big", SIZE_B, K_S, 1.0e6, 153),
    "hidden_tie_a": _hidden_tie,
    "crowd32_b": lambda: _crowd("crowd32_b", False),
    "crowd33_b": lambda: _crowd("crowd33_b", True),
    "mixed_b": _mixed,
    "uncounted_a": _uncounted,
    "select_a": _select,
}
# the case whose outputs each tampering changes (tests/test_scene_verify.py asserts it): tie_later needs two identical poses, lt_visible
# delta = 0, depth_not_dist pixels whose depth difference lies within a few per cent of delta, uncounted_occludes an uncounted pose in front
CAUGHT_BY = {"tie_later": "hidden_tie_a", "lt_visible": "occl_b_d0", "depth_not_dist": "occl_b_d15", "uncounted_occludes": "uncounted_a",
             "swap_fv": "occl_a", "pvis_in_over_model": "occl_a", "ignore_mask_ids": "mixed_b", "ignore_image_ids": "crowd32_b"}
_CASES, _RENDERS = {}, {}


def make(name):
    if name not in _CASES:
        _CASES[name] = CASES[name]()
    return _CASES[name]


# ------------------------------------------------------------------------------------------------------------------- the checker
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
    """the rule applied to renders D (P,H,W) -> dict: counts (P,8) int32, box, box_pvis (P,4) int32, ok (P,) bool, slot (P,) int32, the five
    quotients (P,) float64, full_bits, visib_bits (I,H,W) int32, owner (I,H,W) int8 (the composite's owner: the device stores none),
    choice (B,) int32 or None"""
    D = np.asarray(D, np.float32)
    W, H = case.size
    P, n_img = case.P, case.n_images
    dense_f, dense_v = (case.visible, case.full) if "swap_fv" in tamper else (case.full, case.visible)
    area_f, area_v = dense_f.reshape(case.N, -1).sum(1).astype(np.int64), dense_v.reshape(case.N, -1).sum(1).astype(np.int64)
    F, Vm = read(pack(dense_f), H, W), read(pack(dense_v), H, W)
    slots = case.slots(tamper)
    counted = [case.counted(b, tamper) for b in range(P)]
    out = dict(counts=np.zeros((P, 8), np.int32), box=np.full((P, 4), -1, np.int32), box_pvis=np.full((P, 4), -1, np.int32), ok=np.zeros(P, bool),
               slot=slots.astype(np.int32), full_bits=np.zeros((n_img, H, W), np.uint32), visib_bits=np.zeros((n_img, H, W), np.uint32),
               owner=np.full((n_img, H, W), -1, np.int8), choice=None)
    out.update({k: np.full(P, np.nan) for k in QUOTIENTS})
    ren = np.zeros((n_img, H, W), np.float32)
    for img in range(n_img):
        rows = [b for b in range(P) if case.image_of(b, tamper) == img and 0 <= slots[b] < MAX_POSES
                and (counted[b] or ("uncounted_occludes" in tamper and case.rendered(b)))]
        if rows:
            ren[img], out["owner"][img] = composite([(int(slots[b]), D[b]) for b in rows], tamper)
    for b in range(P):
        m = case.mask_of(b, tamper)
        have = 0 <= m < case.N
        n_mask, n_vis = (int(area_f[m]), int(area_v[m])) if have else (0, 0)
        n = [0] * 5
        if counted[b]:
            img = case.image_of(b, tamper)
            model = D[b] > 0
            pvis = predicted_visible(D[b], ren[img], case.K_of(b), case.delta, tamper)
            n = [int(model.sum()), int(pvis.sum()), int((model & F[m]).sum()), int((model & Vm[m]).sum()),
                 int(((model if "pvis_in_over_model" in tamper else pvis) & Vm[m]).sum())]
            out["box"][b], out["box_pvis"][b] = box_of(model), box_of(pvis)
            out["full_bits"][img] |= model.astype(np.uint32) << np.uint32(slots[b])
            out["visib_bits"][img] |= pvis.astype(np.uint32) << np.uint32(slots[b])
        out["counts"][b] = n + [n_mask, n_vis, n[3] - n[4]]
        fin = finish(*n, n_mask, n_vis, counted[b])
        for k in QUOTIENTS + ("ok",):
            out[k][b] = fin[k]
    out["full_bits"], out["visib_bits"] = out["full_bits"].view(np.int32), out["visib_bits"].view(np.int32)
    if case.cand is not None:
        out["choice"] = select(out["score"].reshape(case.cand), out["ok"].reshape(case.cand))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_case(case, D, out, log=None):
    """out: dict as reference() returns it (full_bits, visib_bits, owner and choice may be missing or None: not checked then), e.g. the
    device's outputs for the renders D.  StageError naming the stage and the pose (or the image, for a plane)"""
    want = reference(case, D)
    for stage in ("slot", "counts", "box", "box_pvis", "ok", "full_bits", "visib_bits", "owner", "choice"):
        if out.get(stage) is None or want[stage] is None:
            continue
        got = np.asarray(out[stage])
        if got.shape != want[stage].shape or not np.array_equal(got, want[stage]):
            bad = np.nonzero((got != want[stage]).reshape(len(got), -1).any(1))[0] if got.shape == want[stage].shape else [-1]
            b = int(bad[0])
            plane = stage in ("full_bits", "visib_bits", "owner")
            raise StageError(stage, b, None, "got %s, expected %s" % (("%d pixels differ" % int((got != want[stage]).sum()), "none") if plane or b < 0
                                                                        else (got[b].tolist(), want[stage][b].tolist())))
    for stage in QUOTIENTS:
        got = np.asarray(out[stage], np.float64)
        if got.shape != want[stage].shape or not np.array_equal(_bits(got), _bits(want[stage])):
            b = int(np.nonzero(_bits(got) != _bits(want[stage]))[0][0]) if got.shape == want[stage].shape else -1
            raise StageError(stage, b, None, "got %r, expected %r" % (float(got[b]), float(want[stage][b])))
    if log is not None:
        log("%-12s n_model %s n_pvis %s iou_vis %s%s" % (case.name, want["counts"][:, 0].tolist(), want["counts"][:, 1].tolist(),
                                                         np.round(want["iou_vis"], 4).tolist(),
                                                         "" if want["choice"] is None else " choice %s" % want["choice"].tolist()))
    return want


def partly_hidden(case, D):
    """the poses with 0 < n_pvis < n_model: a pass cannot come from scenes without occlusion"""
    n = reference(case, D)["counts"].astype(np.int64)
    return np.nonzero((n[:, 1] > 0) & (n[:, 1] < n[:, 0]))[0]


if __name__ == "__main__":
    import sys
    for name in (sys.argv[1:] or list(CASES)):
        c = make(name)
        check_case(c, cpu_renders(c), reference(c, cpu_renders(c)), log=lambda s: print(s, flush=True))
        print("   partly hidden poses", partly_hidden(c, cpu_renders(c)).tolist(), flush=True)
