#!/usr/bin/env python3
"""Row N12 (BOP's cus / cou_bb_proj / cou_mask / cou_bb) pinned by the REFERENCE's own functions after the render.

Runs ONLY where the reference tree is (CHECKERPOSE_REFERENCE, default /root/reference; nothing of it travels, only the recorded
numbers in mask_error.npz are committed):

  python tests/golden/make_golden_mask_error.py

The method is make_golden_vsd.py's: the reference's renderers run nowhere this project runs, so `pose_error.cus` and
`pose_error.cou_bb_proj` (pose_error.py:256-330) are called with the STUB renderer whose render_object(...)['depth'] is the float32
depth of tests/vsd_stages.oracle_render.  `pose_error.cou_mask` runs on the two renders' masks (given as bool, as 0 / 255 and as
0 / 1..255 uint8: one value), `pose_error.cou_bb` on their boxes (misc.calc_2d_bbox) and on the hand-made box pairs of BOXES.
Where cou_bb_proj raises (a silhouette with no pixel: xs.min() of an empty array) NaN is recorded with raises = 1.  A pose with a
vertex at Z <= 0 is outside the render rule: nothing is called, NaN is recorded with behind = 1.

Per case the fixture holds both renders' masks and the oracle's dilated ("possibly set": inside by -eps) and eroded ("surely set":
inside by +eps) masks, bit-packed.  A pixel is undecided where they differ; a side may leave at most 5 % of its covered pixels
undecided (row N8's limit): asserted here, the worst share is printed.

Meshes: tests/vsd_stages.meshes (closed form; "hull" with the faces recorded in vsd.npz); their CRC-32 is recorded.

Stage B: bop_toolkit/scripts/eval_calc_errors.py is RUN, whole, under runpy with --error_type=cus on the drawn world of
make_golden_bop_eval.py (draw_b: box, icosphere and torus as objects 1..3, 3 scenes of 2, 3 and 4 images of 320 x 240 with a camera
matrix per image, several instances and estimates per object, estimates near an instance, between two, or beyond the diameter), with
that file's stand-ins for dataset_params / inout and `renderer.create_renderer` -> the stub renderer, as make_golden_gt_info.py
stubs it.  Then eval_calc_scores.py is run whole on what it saved, at correct_th = 0.5 (make_golden_bop_eval.record).  Per saved
pair the fixture holds the error, whether the script's sphere shortcut skipped it, and the interval [lo, hi] of cus that the
undecided pixels of its two renders allow.  The world is redrawn with the next seed unless: pairs on both sides of the shortcut
occur; no sphere decision lies within 1e-9 (relative) of its boundary; no render leaves more than 5 % of its covered pixels undecided;
no pair's interval contains 0.5; and the intervals of two pairs of one estimate that both lie below 0.5 are disjoint (the greedy
matching compares them) -- so every error inside its interval gives the recorded matches and scores exactly."""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
if not hasattr(np, "bool"):                                      # pose_error.cou_mask spells astype(np.bool)
    np.bool = bool

import make_golden_vsd as V  # noqa: E402  (puts the reference's bop_toolkit and the repository on sys.path)
from bop_toolkit_lib import misc, pose_error  # noqa: E402
from tests import vsd_stages as S  # noqa: E402

# (name, mesh, (W, H), est offset as a fraction of the diameter, placement, K group)
CASES = [
    ("identical_box", "box", (67, 45), 0.0, "centre", 0),
    ("identical_ico", "ico80", (33, 31), 0.0, "centre", 0),
    ("offset_box", "box", (67, 45), 0.10, "centre", 0),
    ("disjoint", "ico80", (67, 45), 0.0, "disjoint", 0),
    ("inside", "ico1280", (67, 45), 0.0, "inside", 0),
    ("crosstile", "torus", (96, 80), 0.10, "centre", 0),
    ("outside_est", "box", (67, 45), 0.0, "outside_est", 0),
    ("outside_both", "box", (67, 45), 0.02, "outside", 0),
    ("pixel", "triangle", (67, 45), 0.0, "pixel", 0),
    ("column", "triangle", (67, 45), 0.0, "column", 0),
    ("column_both", "triangle", (67, 45), 0.0, "column_both", 0),
    ("touch", "box", (96, 80), 0.0, "touch", 0),
    ("zeroarea", "zeroarea", (67, 45), 0.05, "centre", 0),
    ("halfbox_small", "halfbox", (67, 45), 0.02, "open", 0),
    ("halfbox_large", "halfbox", (96, 80), 0.10, "open", 0),
    ("behind", "box", (67, 45), 0.0, "behind", 0),
    ("k1", "box", (67, 45), 0.05, "centre", 1),
    ("k2", "torus", (67, 45), 0.10, "centre", 2),
    ("k3", "ico80", (67, 45), 0.20, "centre", 3),
    ("diagonal", "ico80", (96, 80), 0.0, "diagonal", 0),
    ("far", "box", (67, 45), 0.0, "far", 0),
    ("partly", "box", (67, 45), 0.10, "partly", 0),
    ("hull", "hull", (96, 80), 0.05, "centre", 0),
    ("triangle_small", "triangle", (33, 31), 0.10, "centre", 0),
    ("ico20480", "ico20480", (160, 120), 0.02, "centre", 0),
    ("ico1280_large", "ico1280", (160, 120), 0.20, "centre", 0),
]

# box pairs (x, y, w, h) for cou_bb: integer and fractional, outside a 67 x 45 frame, touching, nested, empty-width
BOXES = [
    ([10, 5, 20, 12], [14, 8, 20, 12]), ([10, 5, 20, 12], [10, 5, 20, 12]), ([0, 0, 10, 10], [10, 0, 10, 10]),
    ([0, 0, 10, 10], [0, 10, 10, 10]), ([-15, -8, 40, 30], [5, 4, 100, 60]), ([60, 40, 30, 30], [50, 30, 25, 25]),
    ([3, 3, 0, 9], [0, 0, 10, 12]), ([3, 3, 0, 9], [3, 3, 0, 9]), ([2, 2, 30, 30], [10, 10, 5, 5]),
    ([1.5, 2.25, 10.5, 7.75], [4.0, 3.5, 9.25, 8.0]), ([0, 0, 5, 5], [20, 20, 5, 5]), ([-30, -30, 10, 10], [-25, -25, 10, 10]),
]

_BASE = {"outside_est": "centre", "inside": "centre", "pixel": "centre", "column": "centre", "column_both": "centre", "touch": "centre",
         "behind": "centre", "diagonal": "centre"}


def box_of(mask):
    ys, xs = mask.nonzero()
    return [int(v) for v in misc.calc_2d_bbox(xs, ys, im_size=None, clip=False)] if xs.size else None


def draw(case, seed, meshes, diam):
    name, mesh, size, frac, place, kgroup = case
    pose = V.draw((mesh, size, frac, "plane", 15, True, _BASE.get(place, place), kgroup), seed, meshes, diam)
    W, H = size
    K, zc, D, rng = pose["K"], pose["zc"], diam[mesh], pose["rng"]
    if place == "outside_est":
        pose["t_est"] = pose["t_est"] + np.array([2.0 * W / K[0, 0] * zc, 0.0, 0.0])
    if place == "inside":                                        # further along the same ray: a smaller, concentric silhouette
        pose["t_est"] = pose["t_gt"] * 1.7
    if place == "diagonal":                                      # discs apart (the sphere projections do not overlap), their boxes overlap
        pose["t_gt"] = pose["t_gt"] - np.array([0.375 * D, 0.375 * D, 0.0])
        pose["t_est"] = pose["t_gt"] + np.array([0.75 * D, 0.75 * D, 0.0])
    if place == "behind":
        pose["t_est"] = np.array([pose["t_gt"][0], pose["t_gt"][1], 10.0])
    if place == "pixel":                                         # the triangle about 1.3 pixels wide
        pose["t_est"] = pose["t_gt"] * (0.45 * min(W, H) / 1.3)
    if place in ("column", "column_both"):                       # the triangle seen nearly edge-on, about 5 pixels tall
        a = rng.uniform(0, 2 * np.pi)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
        Ry = np.array([[0, 0, 1.0], [0, 1.0, 0], [-1.0, 0, 0]])
        pose["R_est"] = V.small_rotation(rng, 0.01) @ Ry @ Rz
        pose["t_est"] = pose["t_gt"] * (0.45 * min(W, H) / 5.0)
        if place == "column_both":
            pose["R_gt"], pose["t_gt"] = pose["R_est"].copy(), pose["t_est"].copy()
    return pose


def accept(case, o_est, o_gt):
    """the property the case is named after (a seed that misses it is skipped)"""
    place = case[4]
    me, mg = o_est["d"] > 0, o_gt["d"] > 0
    be, bg = box_of(me), box_of(mg)
    if place == "pixel":
        return int(me.sum()) == 1 and bool((me & mg).any())
    if place == "column":
        return be is not None and be[2] == 0 and be[3] > 0 and bool((me & mg).any())
    if place == "column_both":
        return be is not None and be[2] == 0 and be[3] > 0
    if place == "touch":
        return be is not None and be[0] + be[2] == bg[0]
    return True


def evaluate(case, pose, meshes):
    """the reference's four functions on one case -> (cus, cou_bb_proj, raises, cou_mask, cou_bb, renders)"""
    name, mesh, size = case[0], case[1], case[2]
    args = (pose["R_est"], pose["t_est"].reshape(3, 1), pose["R_gt"], pose["t_gt"].reshape(3, 1), pose["K"])
    stub = V.StubRenderer(meshes, size)
    cus = float(pose_error.cus(*args, stub, mesh))
    d_est, d_gt = stub.made
    stub = V.StubRenderer(meshes, size)
    try:
        bbp, raises = float(pose_error.cou_bb_proj(*args, stub, mesh)), False
    except ValueError:
        bbp, raises = float("nan"), True
    assert len(stub.made) == 2 and np.array_equal(stub.made[0], d_est) and np.array_equal(stub.made[1], d_gt)
    me, mg = d_est > 0, d_gt > 0
    ys, xs = np.mgrid[0:me.shape[0], 0:me.shape[1]]
    mixed = (1 + (xs + 2 * ys) % 255).astype(np.uint8)
    cm = [float(pose_error.cou_mask(a, b)) for a, b in ((me, mg), (me.astype(np.uint8) * 255, mg.astype(np.uint8) * 255),
                                                        (me * mixed, mg.astype(np.uint8)))]
    assert cm[0] == cm[1] == cm[2] == cus, (name, cm, cus)
    be, bg = box_of(me), box_of(mg)
    cbb = float(pose_error.cou_bb(be, bg)) if be is not None and bg is not None else float("nan")
    assert raises == (be is None or bg is None) and (raises or cbb == bbp), (name, cbb, bbp)
    return cus, bbp, raises, cm[0], cbb, d_est, d_gt


def save_npz(path, arrays):
    """np.savez_compressed with a fixed timestamp and order: the same arrays give the same bytes on every run"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


class WorldRenderer(object):
    """what renderer.create_renderer hands eval_calc_errors.py in stage B: render_object(...)['depth'] = the oracle's float32 depth"""

    def __init__(self, size, meshes_of):
        self.size, self.meshes_of, self.made = size, meshes_of, {}

    def add_object(self, obj_id, model_path, **kwargs):
        assert obj_id in self.meshes_of

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        key = (obj_id, np.asarray(R).tobytes(), np.asarray(t).tobytes(), fx, fy, cx, cy)
        if key not in self.made:
            v, f = self.meshes_of[obj_id]
            self.made[key] = S.oracle_render(R, np.asarray(t).reshape(3), np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]), v, f, self.size)
        return {"depth": self.made[key]["d"]}


def run_errors_cus(E, b, n_top, ren):
    """eval_calc_errors.py --error_type=cus on the world b -> {scene_id: the list it saved}"""
    import copy
    import runpy
    from bop_toolkit_lib import dataset_params, inout, renderer
    from tests import bop_eval_stages as BS
    targets, scene_gt, _ = BS.dicts_of(b, poses=True)
    _, info = BS.b_models(b)
    ests = BS.b_ests(b)
    cams = {}
    for (s, i), K in zip(b["cam"].tolist(), b["K"]):
        cams.setdefault(s, {})[i] = {"cam_K": K.copy(), "depth_scale": 1.0}
    saved = {}

    def load_json(path, keys_to_int=False):
        if path == "models_info":
            return copy.deepcopy(info)
        if path.endswith("targets.json"):
            return copy.deepcopy(targets)
        raise AssertionError(path)

    def save_json(path, content):
        saved[int(os.path.basename(path)[len("errors_"):-len(".json")])] = content

    patches = [(dataset_params, "get_split_params", lambda *a, **k: {"base_path": "base", "scene_gt_tpath": "gt|{scene_id}", "im_size": ren.size,
                                                                      "scene_camera_tpath": "cam|{scene_id}", "depth_tpath": "depth",
                                                                      "scene_ids": [int(s) for s in b["scene_ids"]]}),
               (dataset_params, "get_model_params", lambda *a, **k: {"obj_ids": [int(o) for o in b["obj_ids"]], "models_info_path": "models_info",
                                                                      "symmetric_obj_ids": [int(o) for o in b["sym_obj_ids"]], "model_tpath": "{obj_id}"}),
               (renderer, "create_renderer", lambda w, h, renderer_type="vispy", mode="rgb+depth", **k: ren),
               (inout, "load_json", load_json), (inout, "load_bop_results", lambda path, version="bop19": copy.deepcopy(ests)),
               (inout, "load_scene_gt", lambda path: copy.deepcopy(scene_gt[int(path.split("|")[1])])),
               (inout, "load_scene_camera", lambda path: copy.deepcopy(cams[int(path.split("|")[1])])),
               (inout, "save_json", save_json), (misc, "log", lambda s: None), (misc, "ensure_dir", lambda path: None)]
    old = [(m, n, getattr(m, n)) for m, n, _ in patches]
    argv = sys.argv
    try:
        for m, n, fn in patches:
            setattr(m, n, fn)
        sys.argv = ["eval_calc_errors.py", "--n_top=%d" % n_top, "--error_type=cus", "--result_filenames=m_ds-test.csv", "--results_path=res",
                    "--eval_path=eval", "--targets_filename=targets.json"]
        runpy.run_path(os.path.join(V.REF, "bop_toolkit", "scripts", "eval_calc_errors.py"), run_name="__main__")
    finally:
        sys.argv = argv
        for m, n, fn in old:
            setattr(m, n, fn)
    return saved


def cus_interval(o_est, o_gt):
    """the smallest and largest cus over every pair of masks between the surely-set and the possibly-set pixels of two renders"""
    e_lo, e_hi, g_lo, g_hi = (np.isfinite(o[k]) for o in (o_est, o_gt) for k in ("d_lo", "d_hi"))
    i_min, i_max, u_min, u_max = int((e_hi & g_hi).sum()), int((e_lo & g_lo).sum()), int((e_hi | g_hi).sum()), int((e_lo | g_lo).sum())
    if u_max == 0:
        return 1.0, 1.0
    return (1.0 - i_max / float(max(u_min, 1)), 1.0 - i_min / float(u_max))


def stage_b(meshes):
    import make_golden_bop_eval as E
    from tests import bop_eval_stages as BS
    n_top, visib_gt_min, size = -1, -1, (E.B_WIDTH, 240)
    seed = 3100
    while True:
        b = E.draw_b(np.random.default_rng(seed))
        meshes_of = {int(o): meshes[str(n)] for o, n in zip(b["obj_ids"], b["mesh"])}
        _, info = BS.b_models(b)
        ren = WorldRenderer(size, meshes_of)
        saved = run_errors_cus(E, b, n_top, ren)
        est_rows = np.array([(scene, e["im_id"], e["obj_id"], e["est_id"]) for scene, lst in saved.items() for e in lst], dtype=np.int64).reshape(-1, 4)
        key = np.array([(scene, e["im_id"], e["obj_id"], e["est_id"], g) for scene, lst in saved.items() for e in lst for g in e["errors"]],
                       dtype=np.int64).reshape(-1, 5)
        err = np.array([v[0] for lst in saved.values() for e in lst for v in e["errors"].values()], dtype=np.float64)
        rows, pairs = BS.expand(b, n_top)
        assert np.array_equal(rows[:, :4], est_rows) and np.array_equal(pairs[:, 1], key[:, 4]) and len(err) == len(pairs)
        lo, hi, skip, why, worst = np.ones(len(err)), np.ones(len(err)), np.zeros(len(err), bool), None, 0.0
        for p, (Re, te, Rg, tg, K, o) in enumerate(BS._b_pair_args(b, rows, pairs)):
            r = 0.5 * info[o]["diameter"]
            d = np.linalg.norm((te / te[2])[:2] - (tg / tg[2])[:2])
            th = r * (1.0 / te[2] + 1.0 / tg[2])
            skip[p] = not misc.overlapping_sphere_projections(r, te, tg)
            if abs(d - th) <= 1e-9 * th:
                why = "a sphere decision on its boundary"
            if skip[p]:
                assert err[p] == 1.0
                continue
            o_e = ren.made[(o, Re.tobytes(), te.reshape(3, 1).tobytes(), K[0, 0], K[1, 1], K[0, 2], K[1, 2])]
            o_g = ren.made[(o, Rg.tobytes(), tg.reshape(3, 1).tobytes(), K[0, 0], K[1, 1], K[0, 2], K[1, 2])]
            worst = max(worst, S.undecided_share(o_e), S.undecided_share(o_g))
            lo[p], hi[p] = cus_interval(o_e, o_g)
            assert lo[p] <= err[p] <= hi[p]
            if lo[p] <= 0.5 <= hi[p]:
                why = "an error within its interval of 0.5"
        if worst > 0.05:
            why = "a render with more than 5 %% of its covered pixels undecided (%.3f)" % worst
        if not (skip.any() and (~skip).any() and (err < 0.5).any() and ((err >= 0.5) & ~skip).any()):
            why = "one side of the sphere shortcut or of the threshold is missing"
        for r_ in np.unique(pairs[:, 0]):
            cand = [p for p in np.nonzero(pairs[:, 0] == r_)[0] if hi[p] < 0.5]
            for x in cand:
                for y in cand:
                    if x < y and not (hi[x] < lo[y] or hi[y] < lo[x]):
                        why = "two candidate errors of one estimate with overlapping intervals"
        if why:
            print("stage B seed %d: %s -> redrawn" % (seed, why))
            seed += 1
            continue
        b["cus_th"], b["cus_params"] = np.array([0.5]), np.array([n_top, visib_gt_min], dtype=np.float64)
        rec = E.record(BS.b_case(b, "cus", np.concatenate([est_rows, rows[:, 4:5]], 1), pairs, err, raw=True), "cus", [([0], [0.5])], n_top, visib_gt_min)
        out = dict(b)
        out.update({"cus_est": est_rows, "cus_key": key, "cus_err": err, "cus_lo": lo, "cus_hi": hi, "cus_skip": skip, "seed": np.int64(seed),
                    "height": np.int64(size[1])})
        out.update({"cus_" + k: v for k, v in rec.items()})
        print("stage B seed %d: NE %d  P %d  skipped %d  below 0.5: %d  exact-interval pairs %d  worst undecided %.4f  matched %d  recall %.4f"
              % (seed, len(est_rows), len(err), int(skip.sum()), int((err < 0.5).sum()), int((lo == hi).sum()), worst,
                 int((rec["m_est"] >= 0).sum()), rec["s_recall"][0]))
        return out


def main():
    vsd = np.load(os.path.join(HERE, "vsd.npz"))
    meshes = S.meshes(vsd["hull_faces"].astype(np.int32))
    diam = {k: S.diameter(v) for k, (v, f) in meshes.items()}
    keys = ("R_est", "t_est", "R_gt", "t_gt", "K", "mesh", "W", "H", "kgroup", "cus", "cou_bb_proj", "raises", "behind", "cou_mask", "cou_bb",
            "counts", "boxes", "sphere", "seed", "undecided")
    rec = {k: [] for k in keys}
    images, worst = [], 0.0
    for ci, case in enumerate(CASES):
        name, mesh, size, frac, place, kgroup = case
        v, f = meshes[mesh]
        H, W = size[1], size[0]
        seed = 1000 * ci
        while True:
            pose = draw(case, seed, meshes, diam)
            if place == "touch":                                 # slide the estimate left until its last column is the truth's first
                o_gt = S.oracle_render(pose["R_gt"], pose["t_gt"], pose["K"], v, f, size)
                bg = box_of(o_gt["d"] > 0)
                for step in range(400):
                    pose["t_est"] = pose["t_gt"] - np.array([(0.8 * bg[2] + 0.05 * step) * pose["zc"] / pose["K"][0, 0], 0.0, 0.0])
                    be = box_of(S.oracle_render(pose["R_est"], pose["t_est"], pose["K"], v, f, size)["d"] > 0)
                    if be is not None and be[0] + be[2] <= bg[0]:
                        break
            if place == "behind":
                o_gt = S.oracle_render(pose["R_gt"], pose["t_gt"], pose["K"], v, f, size)
                try:
                    S.oracle_render(pose["R_est"], pose["t_est"], pose["K"], v, f, size)
                    raise AssertionError("the 'behind' case has no vertex at Z <= 0")
                except ValueError:
                    pass
                share = S.undecided_share(o_gt)
                assert share <= 0.05
                break
            o_gt = S.oracle_render(pose["R_gt"], pose["t_gt"], pose["K"], v, f, size)
            o_est = S.oracle_render(pose["R_est"], pose["t_est"], pose["K"], v, f, size)
            share = max(S.undecided_share(o_gt), S.undecided_share(o_est))
            if share <= 0.05 and accept(case, o_est, o_gt):
                break
            seed += 1
            assert seed < 1000 * ci + 600, "no seed gives case %r its property" % name
        worst = max(worst, share)
        sphere = bool(misc.overlapping_sphere_projections(0.5 * diam[mesh], pose["t_est"], pose["t_gt"]))
        if place == "behind":
            cus = bbp = cm = cbb = float("nan")
            raises, counts, boxes = False, [0, 0, 0, 0], [[-1] * 4, [-1] * 4]
            zero = np.zeros((H, W), bool)
            layers = [zero, o_gt["d"] > 0, zero, zero, np.isfinite(o_gt["d_lo"]), np.isfinite(o_gt["d_hi"])]
        else:
            cus, bbp, raises, cm, cbb, d_est, d_gt = evaluate(case, pose, meshes)
            assert np.array_equal(d_est, o_est["d"]) and np.array_equal(d_gt, o_gt["d"])
            me, mg = d_est > 0, d_gt > 0
            counts = [int((me & mg).sum()), int((me | mg).sum()), int(me.sum()), int(mg.sum())]
            boxes = [box_of(m) or [-1] * 4 for m in (me, mg)]
            layers = [me, mg, np.isfinite(o_est["d_lo"]), np.isfinite(o_est["d_hi"]), np.isfinite(o_gt["d_lo"]), np.isfinite(o_gt["d_hi"])]
            for m, lo, hi in ((me, layers[2], layers[3]), (mg, layers[4], layers[5])):
                assert not (hi & ~m).any() and not (m & ~lo).any()           # surely set <= set <= possibly set
        for k in ("R_est", "t_est", "R_gt", "t_gt", "K"):
            rec[k].append(pose[k])
        for k, val in (("mesh", S.MESH_NAMES.index(mesh)), ("W", W), ("H", H), ("kgroup", kgroup), ("cus", cus), ("cou_bb_proj", bbp),
                       ("raises", raises), ("behind", place == "behind"), ("cou_mask", cm), ("cou_bb", cbb), ("counts", counts), ("boxes", boxes),
                       ("sphere", sphere), ("seed", seed), ("undecided", share)):
            rec[k].append(val)
        images.append(np.packbits(np.stack(layers).reshape(6, -1), axis=1))
        print("case %2d %-14s %-9s %3dx%-3d counts %-24s boxes %-44s cus %.6f cou_bb_proj %.6f raises %d sphere %d undecided %.4f seed %d"
              % (ci, name, mesh, W, H, counts, boxes, cus, bbp, raises, sphere, share, seed))
    print("worst undecided share of a side's covered pixels: %.4f (limit 0.05)" % worst)
    # properties the issue lists, by name
    at = {c[0]: i for i, c in enumerate(CASES)}
    c = lambda n, k: rec[k][at[n]]                               # noqa: E731
    assert c("identical_box", "cus") == 0.0 and c("identical_ico", "cus") == 0.0 and c("column_both", "cus") == 0.0
    assert c("disjoint", "cus") == 1.0 and c("disjoint", "counts")[1] > 0 and c("disjoint", "counts")[0] == 0
    assert c("inside", "counts")[0] == c("inside", "counts")[2] < c("inside", "counts")[3]
    assert c("outside_est", "cus") == 1.0 and c("outside_est", "raises") and c("outside_est", "counts")[3] > 0
    assert c("outside_both", "counts")[1] == 0 and c("outside_both", "cus") == 1.0 and c("outside_both", "raises")
    assert c("pixel", "counts")[2] == 1 and c("pixel", "boxes")[0][2:] == [0, 0] and c("pixel", "cou_bb_proj") == 1.0
    assert c("column", "boxes")[0][2] == 0 and c("column", "cou_bb_proj") == 1.0 and c("column_both", "cou_bb_proj") == 1.0
    assert c("touch", "boxes")[0][0] + c("touch", "boxes")[0][2] == c("touch", "boxes")[1][0] and c("touch", "cou_bb_proj") == 1.0
    assert not c("diagonal", "sphere") and c("diagonal", "cus") == 1.0 and c("diagonal", "cou_bb_proj") < 1.0
    assert not c("far", "sphere") and sum(1 for s in rec["sphere"] if s) >= 15
    bx = c("crosstile", "boxes")
    assert all(b[0] < 32 <= b[0] + b[2] and b[1] < 32 <= b[1] + b[3] for b in bx)
    out = {k: np.asarray(v) for k, v in rec.items()}
    out["names"] = np.asarray([c_[0] for c_ in CASES])
    out["mesh_names"] = np.asarray(S.MESH_NAMES)
    out["mesh_diameter"] = np.asarray([diam[k] for k in S.MESH_NAMES])
    out["mesh_crc"] = np.asarray([zlib.crc32(meshes[k][0].tobytes() + meshes[k][1].tobytes()) for k in S.MESH_NAMES], dtype=np.int64)
    out["bb_est"] = np.asarray([b[0] for b in BOXES], dtype=np.float64)
    out["bb_gt"] = np.asarray([b[1] for b in BOXES], dtype=np.float64)
    out["bb_cou"] = np.asarray([float(pose_error.cou_bb(list(a), list(b))) for a, b in BOXES], dtype=np.float64)
    for ci, im in enumerate(images):
        out["bits_%d" % ci] = im
    out.update({"b_" + k: v for k, v in stage_b(meshes).items()})
    path = os.path.join(HERE, "mask_error.npz")
    save_npz(path, out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
