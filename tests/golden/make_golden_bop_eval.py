#!/usr/bin/env python3
"""Row N11 (BOP's matching and recall scores) pinned by the REFERENCE's own script.

Runs ONLY where the reference tree is (CHECKERPOSE_REFERENCE, default /root/reference; nothing of it travels, only the recorded
numbers in bop_eval.npz are committed):

  python tests/golden/make_golden_bop_eval.py

Stage A: bop_toolkit/scripts/eval_calc_scores.py is RUN, whole, under runpy -- once per threshold column of every case of CASES, as
eval_bop19_pose.py runs it.  It cannot reach a dataset here, so what it imports is given stand-ins before it starts:
  dataset_params.get_split_params / get_model_params -> the case's scene and object lists and path templates only the stubs read;
  inout.load_json      -> the targets, scene_gt_info, models_info and the scene's error list of the current column (a fresh copy);
  inout.load_scene_gt  -> the case's ground truths;  inout.save_json -> captures the saved scores and matches;  misc.log -> nothing.
Everything between the error tables and the saved scores is the script's own code and what it calls: the organisation of the
targets, the validity rule, pose_matching.match_poses_scene / match_poses, score.calc_localization_scores.  Nothing of it is restated
here: this file only draws the tables (draw_world) and stores what came back.

Drawn tables (the cases name what they cover): error values from a small set, so that exact ties, values equal to a threshold, inf
and NaN are frequent; 're' (one element) and 'rete' (two elements, where the componentwise rule depends on the scan order) error
types; 1, 10, 65 and 100 columns; groups with n_g = 1, 2, 63, 64, 65, 130 ground truths and n_e = 0, 1, fewer and more estimates,
equal scores, estimate lists not in score order; estimates of an object absent from the image; ground truths whose object is not a
target; inst_count below the instance count with tied visib_fract; visib_gt_min = -1 and 0.1; n_top = 1, 2, 0, -1; an object and a
scene without targets; an image no target names.

Stage B: bop_toolkit/scripts/eval_calc_errors.py is RUN, whole, under runpy, once for each of "mssd", "mspd", "proj", "add", "adi"
and "ad", on a drawn world (draw_b): the closed-form box (one discrete symmetry), icosphere and torus (a continuous symmetry) of
tests/vsd_stages.py as objects 1..3, objects 2 and 3 in symmetric_obj_ids; 3 scenes of 2, 3 and 4 images with a camera matrix per
image; one to three instances per object and image, in interleaved gt_id order; zero to five estimates per (image, object), near an
instance, between two, or beyond the diameter, listed out of score order with tied scores; an object of an image that is no target, a
target whose object is absent, a target with fewer estimates than inst_count.  Its stand-ins: dataset_params as above (plus
symmetric_obj_ids and the path templates), inout.load_ply -> the mesh, load_json -> models_info / targets, load_bop_results -> the
estimates, load_scene_camera / load_scene_gt, save_json -> captures the errors, misc.ensure_dir / log -> nothing.  The saved errors
then go through eval_calc_scores.py, run whole once per threshold, exactly as in stage A.  For "mssd" and "mspd" the parameters are
eval_bop19_pose.py's (n_top = -1, its ten thresholds, visib_gt_min = -1).

Stage B is what the device's fp32 errors are compared with, so the world is redrawn with the next seed unless (guards()):
every recorded normalised error lies at least 4 x the device bound of its row (tests/test_bop_error.py's for MSSD / MSPD / proj,
tests/test_pose_error.py's for ADD / ADI, normalised alike) from every threshold of its kind; two finite errors of one estimate lie
at least 4 x the sum of their bounds apart (the greedy scan compares them); every |t_e - t_g| lies at least 1e-9 x diameter from
the diameter; and both sides of the sphere shortcut occur."""
import copy
import json
import os
import runpy
import sys
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "bop_toolkit"))
sys.path.insert(0, ROOT)
for name in ("imageio", "png"):
    if name not in sys.modules:
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)

from bop_toolkit_lib import dataset_params, inout, misc  # noqa: E402

TH10 = np.arange(0.05, 0.51, 0.05)
BIG = [(1, 0), (1, 1), (2, 1), (2, 3), (63, 5), (63, 70), (64, 64), (64, 3), (65, 66), (65, 2), (130, 140), (130, 4), (3, 3), (5, 8)]
SMALL = [(1, 1), (2, 3), (3, 2), (8, 8), (4, 0), (1, 2), (2, 2), (6, 3)]
# name -> (group shapes, error type, error columns, thresholds per error column (C = product), n_top, visib_gt_min)
CASES = [
    ("big_c1", BIG, "re", 1, [[0.1]], 1, -1),
    ("big_c10", BIG, "re", 1, [[t] for t in TH10], 2, 0.1),
    ("big_rete", BIG, "rete", 2, [[2.0 * k, 1.5 * k] for k in range(1, 11)], 0, -1),
    ("small_c65", SMALL, "re", 5, [[t] for t in np.arange(0.04, 0.53, 0.04)], -1, -1),
    ("small_c100", SMALL, "re", 10, [[t] for t in TH10], -1, 0.1),
    ("scan_order", "scan", "rete", 2, [[5.0, 5.0]], 0, -1),
]
RE_VALUES = [0.01, 0.04, float(TH10[0]), float(TH10[1]), 0.07, float(TH10[3]), 0.2, 0.3, 0.3, float("inf"), float("nan"), 0.6, 0.45]
RETE_VALUES = [1.0, 2.0, 3.0, 3.0, 4.0, 6.0, 4.5, 9.0, float("inf"), float("nan"), 14.0, 20.0]


def draw_world(shapes, etype, c_err, rng):
    """-> dict of the flat arrays of one case (tests/bop_eval_stages.py reads the same layout)"""
    targets, gt, visib, est, score, pair, err = [], [], [], [], [], [], []
    values = RE_VALUES if etype == "re" else RETE_VALUES
    if shapes == "scan":
        # one estimate, thresholds (5, 5): A = (3, 3), B = (1, 4): the scan keeps A, an arg-min on the first element takes B;
        # image 2: B' = (4, 1), A' = (3, 3), C' = (2, 2): the scan ends at B', in the order A', B', C' it would end at C'
        targets = [(1, 1, 1, 2), (1, 2, 1, 3)]
        gt = [(1, 1, 1, 0), (1, 1, 1, 1), (1, 2, 1, 0), (1, 2, 1, 1), (1, 2, 1, 2)]
        visib = [1.0] * 5
        est, score = [(1, 1, 1, 0), (1, 2, 1, 0)], [0.5, 0.5]
        pair = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)]
        err = [(3.0, 3.0), (1.0, 4.0), (4.0, 1.0), (3.0, 3.0), (2.0, 2.0)]
        return pack(targets, gt, visib, est, score, pair, err, [1, 2], [1, 2])
    per_image = 2
    slots = {}
    for k, (n_g, n_e) in enumerate(shapes):
        scene, im = 1 + (k // per_image) % 2, k // (2 * per_image)
        slots.setdefault((scene, im), []).append((1 + k % 3, n_g, n_e))          # objects 1..3
    for (scene, im), groups in slots.items():
        im_gt = []                                            # (obj, visib) in gt_id order: the groups interleaved
        for obj, n_g, n_e in groups:
            im_gt += [(obj, float(rng.choice([0.05, 0.3, 0.3, 0.8, 1.0]))) for _ in range(n_g)]
        im_gt += [(4, 0.9), (4, 0.2)]                         # object 4 is in the image; a target only in scene 1, image 0
        order = rng.permutation(len(im_gt))
        im_gt = [im_gt[k] for k in order]
        for gt_id, (obj, v) in enumerate(im_gt):
            gt.append((scene, im, obj, gt_id))
            visib.append(v)
        for obj, n_g, n_e in groups:
            inst = n_g if rng.random() < 0.5 else max(1, n_g - int(rng.integers(1, 4)))
            targets.append((scene, im, obj, inst))
        if (scene, im) == (1, 0):
            targets.append((scene, im, 4, 1))
        targets.append((scene, im, 5, 1))                     # a target whose object is absent from the image
        for obj, n_e in [(g[0], g[2]) for g in groups] + [(4, 2), (5, 2)]:
            ids = [j for j, (o, _) in enumerate(im_gt) if o == obj]
            equal = (len(ids), n_e) == (3, 3)
            listing = rng.permutation(n_e)                    # the list is not in est_id order
            for est_id in listing:
                est.append((scene, im, obj, int(est_id)))
                score.append(0.7 if equal else float(rng.choice([0.1, 0.5, 0.5, 0.9, round(float(rng.random()), 3)])))
                for g in ids:
                    pair.append((len(est) - 1, g))
                    hit = rng.random() < min(1.0, 3.0 / max(1, len(ids)))      # large groups: mostly far off, a few candidates
                    err.append([float(rng.choice(values)) if hit else float(rng.choice(values[-4:])) for _ in range(c_err)])
    # an image with ground truths and estimates that no target names; scene 3 and object 6 have no targets at all
    gt += [(2, 9, 1, 0), (2, 9, 2, 1)]
    visib += [1.0, 1.0]
    est.append((2, 9, 1, 0))
    score.append(0.9)
    pair.append((len(est) - 1, 0))
    err.append([values[0]] * c_err)
    return pack(targets, gt, visib, est, score, pair, err, [1, 2, 3], [1, 2, 3, 4, 5, 6])


def pack(targets, gt, visib, est, score, pair, err, scene_ids, obj_ids):
    return {"targets": np.array(targets, dtype=np.int64), "gt": np.array(gt, dtype=np.int64), "visib": np.array(visib, dtype=np.float64),
            "est": np.array(est, dtype=np.int64), "score": np.array(score, dtype=np.float64), "pair": np.array(pair, dtype=np.int64),
            "err": np.array(err, dtype=np.float64).reshape(len(pair), -1), "scene_ids": np.array(scene_ids), "obj_ids": np.array(obj_ids)}


def run_script(fx, etype, cols, ths, n_top, visib_gt_min):
    """eval_calc_scores.py on one column -> (scores as saved, matches as saved)"""
    from tests import bop_eval_stages as S                    # the arrays -> bop_toolkit's dicts (no logic of the script)
    targets, scene_gt, info = S.dicts_of(fx)
    scene_errs = S.scene_errs_of(fx, cols)
    saved = {}

    def load_json(path, keys_to_int=False):
        if path == "models_info":
            return {int(o): {"diameter": float(d)} for o, d in zip(fx["obj_ids"], fx.get("diam", np.ones(len(fx["obj_ids"]))))}
        if path.endswith("targets.json"):
            return copy.deepcopy(targets)
        if path.startswith("info|"):
            return copy.deepcopy(info[int(path.split("|")[1])])
        if "errors_" in path:
            return copy.deepcopy(scene_errs.get(int(os.path.basename(path)[len("errors_"):-len(".json")]), []))
        raise AssertionError(path)

    def save_json(path, content):
        saved[os.path.basename(path).split("_")[0]] = content

    patches = [(dataset_params, "get_split_params", lambda *a, **k: {"base_path": "base", "scene_gt_tpath": "gt|{scene_id}",
                                                                      "scene_gt_info_tpath": "info|{scene_id}", "im_size": (int(fx.get("width", 640)), 480),
                                                                      "scene_ids": [int(s) for s in fx["scene_ids"]]}),
               (dataset_params, "get_model_params", lambda *a, **k: {"obj_ids": [int(o) for o in fx["obj_ids"]],
                                                                      "models_info_path": "models_info"}),
               (inout, "load_json", load_json), (inout, "load_scene_gt", lambda path: copy.deepcopy(scene_gt[int(path.split("|")[1])])),
               (inout, "save_json", save_json), (misc, "log", lambda s: None)]
    old = [(m, n, getattr(m, n)) for m, n, _ in patches]
    argv = sys.argv
    try:
        for m, n, fn in patches:
            setattr(m, n, fn)
        sys.argv = ["eval_calc_scores.py", "--error_dir_paths=m_ds-test/error=%s_ntop=%d" % (etype, n_top),
                    "--correct_th_%s=%s" % (etype, ",".join(repr(float(t)) for t in ths)), "--visib_gt_min=%r" % (visib_gt_min,),
                    "--targets_filename=targets.json", "--eval_path=eval"]
        runpy.run_path(os.path.join(REF, "bop_toolkit", "scripts", "eval_calc_scores.py"), run_name="__main__")
    finally:
        sys.argv = argv
        for m, n, fn in old:
            setattr(m, n, fn)
    return saved["scores"], saved["matches"]


def record(fx, etype, columns, n_top, visib_gt_min):
    """eval_calc_scores.py once per column -> the arrays of what it saved"""
    C, E = len(columns), len(columns[0][1])
    rec = None
    for c, (cols, th) in enumerate(columns):
        scores, matches = run_script(fx, etype, cols, th, n_top, visib_gt_min)
        NG = len(matches)
        if rec is None:
            rec = {"m_key": np.array([[m["scene_id"], m["im_id"], m["obj_id"], m["gt_id"]] for m in matches], dtype=np.int64),
                   "m_valid": np.array([bool(m["valid"]) for m in matches]), "m_est": np.full((NG, C), -1, dtype=np.int64),
                   "m_score": np.full((NG, C), -1.0), "m_err": np.full((NG, C, E), -1.0), "m_norm": np.full((NG, C, E), -1.0),
                   "s_recall": np.zeros(C), "s_obj": np.zeros((len(fx["obj_ids"]), C)), "s_scene": np.zeros((len(fx["scene_ids"]), C)),
                   "s_mobj": np.zeros(C), "s_mscene": np.zeros(C), "s_counts": np.zeros((C, 3), dtype=np.int64)}
        for r, m in enumerate(matches):
            assert [m["scene_id"], m["im_id"], m["obj_id"], m["gt_id"]] == rec["m_key"][r].tolist() and bool(m["valid"]) == rec["m_valid"][r]
            rec["m_est"][r, c], rec["m_score"][r, c] = m["est_id"], m["score"]
            if m["est_id"] != -1:
                rec["m_err"][r, c], rec["m_norm"][r, c] = m["error"], m["error_norm"]
        rec["s_recall"][c], rec["s_mobj"][c], rec["s_mscene"][c] = scores["recall"], scores["mean_obj_recall"], scores["mean_scene_recall"]
        rec["s_obj"][:, c] = [scores["obj_recalls"][int(o)] for o in fx["obj_ids"]]
        rec["s_scene"][:, c] = [scores["scene_recalls"][int(s)] for s in fx["scene_ids"]]
        rec["s_counts"][c] = (scores["gt_count"], scores["targets_count"], scores["tp_count"])
    return rec


# ---- stage B ----------------------------------------------------------------------------------------------------------------------------
B_OBJECTS = {1: "box", 2: "ico80", 3: "torus"}
B_SYMMETRIC = [2, 3]
B_WIDTH = 320
# kind -> (n_top, visib_gt_min, thresholds)
B_PARAMS = {"mssd": (-1, -1, np.arange(0.05, 0.51, 0.05)), "mspd": (-1, -1, np.arange(5, 51, 5)), "proj": (1, -1, [2.0, 5.0, 10.0, 20.0, 40.0]),
            "add": (0, 0.1, [0.02, 0.05, 0.1, 0.2, 0.5]), "adi": (2, -1, [0.02, 0.05, 0.1, 0.2, 0.5]), "ad": (-1, -1, [0.02, 0.05, 0.1, 0.2, 0.5])}


def rotation(rng, angle=None):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    angle = rng.uniform(0, np.pi) if angle is None else angle
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def draw_b(rng):
    from tests import vsd_stages as V
    meshes = V.meshes()
    diam = {o: float(V.diameter(meshes[n][0])) for o, n in B_OBJECTS.items()}
    info = {1: {"diameter": diam[1], "symmetries_discrete": [[-1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0]]},
            2: {"diameter": diam[2]}, 3: {"diameter": diam[3], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}
    targets, gt, visib, gR, gt_t, cam, Ks, est, score, eR, et = [], [], [], [], [], [], [], [], [], [], []
    for scene, n_im in ((1, 2), (2, 3), (4, 4)):
        for im in range(n_im):
            im_id = 10 * im + scene
            K = np.array([[286.2 * rng.uniform(0.97, 1.03), 0.0, 162.6 + rng.uniform(-3, 3)], [0.0, 286.8 * rng.uniform(0.97, 1.03), 121.0 + rng.uniform(-3, 3)],
                          [0.0, 0.0, 1.0]])
            cam.append((scene, im_id))
            Ks.append(K)
            inst = []                                          # (obj, R, t)
            for obj in (1, 2, 3):
                if (scene, im, obj) == (2, 1, 3):              # object 3 is absent from this image (and stays a target)
                    continue
                n = int(rng.integers(1, 4))
                c = np.array([rng.uniform(-120, 120), rng.uniform(-90, 90), rng.uniform(600, 900)])
                for _ in range(n):                             # the instances of an object within about a diameter of each other
                    inst.append((obj, rotation(rng), c + rng.normal(size=3) * 0.45 * diam[obj]))
            inst = [inst[k] for k in rng.permutation(len(inst))]
            for gt_id, (obj, R, t) in enumerate(inst):
                gt.append((scene, im_id, obj, gt_id))
                visib.append(float(rng.choice([0.05, 0.4, 0.4, 0.9, 1.0])))
                gR.append(R)
                gt_t.append(t)
            block = []
            for obj in (1, 2, 3):
                mine = [(R, t) for o, R, t in inst if o == obj]
                if (scene, im, obj) != (1, 1, 2):              # object 2 of this image is no target
                    targets.append((scene, im_id, obj, max(1, len(mine) - int(rng.random() < 0.3))))
                n_e = int(rng.integers(0, 6)) if mine else 2
                for _ in range(n_e):
                    R, t = mine[int(rng.integers(len(mine)))] if mine else (np.eye(3), np.array([0.0, 0.0, 700.0]))
                    how = rng.choice(["close", "close", "near", "between", "far"])
                    if how == "between" and len(mine) > 1:
                        t = 0.5 * (t + mine[int(rng.integers(len(mine)))][1])
                    shift = rng.normal(size=3)
                    shift *= {"close": 0.03, "near": 0.25, "between": 0.1, "far": 1.6}[how] * diam[obj] * rng.uniform(0.5, 1.5) / np.linalg.norm(shift)
                    block.append((obj, float(rng.choice([0.2, 0.6, 0.6, round(float(rng.random()), 3)])),
                                  rotation(rng, {"close": 0.03, "near": 0.3, "between": 0.1, "far": 1.0}[how] * rng.uniform(0.5, 1.5)) @ R, t + shift))
            for k in rng.permutation(len(block)):              # the results file is in no order
                obj, sc, R, t = block[k]
                est.append((scene, im_id, obj))
                score.append(sc)
                eR.append(R)
                et.append(t)
    return {"targets": np.array(targets, dtype=np.int64), "gt": np.array(gt, dtype=np.int64), "visib": np.array(visib), "gt_R": np.array(gR),
            "gt_t": np.array(gt_t), "cam": np.array(cam, dtype=np.int64), "K": np.array(Ks), "est": np.array(est, dtype=np.int64),
            "score": np.array(score), "est_R": np.array(eR), "est_t": np.array(et), "scene_ids": np.array([1, 2, 3, 4]), "obj_ids": np.array([1, 2, 3, 4]),
            "mesh": np.array([B_OBJECTS.get(o, "triangle") for o in (1, 2, 3, 4)]),
            "mesh_crc": np.array([zlib.crc32(meshes[B_OBJECTS.get(o, "triangle")][0].tobytes()) for o in (1, 2, 3, 4)], dtype=np.int64),
            "info": np.array([json.dumps(info.get(o, {"diameter": float(V.diameter(meshes["triangle"][0]))})) for o in (1, 2, 3, 4)]),
            "diam": np.array([info[o]["diameter"] if o in info else float(V.diameter(meshes["triangle"][0])) for o in (1, 2, 3, 4)]),
            "sym_obj_ids": np.array(B_SYMMETRIC), "width": np.int64(B_WIDTH)}


def run_errors(b, kind, n_top):
    """eval_calc_errors.py on one error type -> {scene_id: the list it saved}"""
    from tests import bop_eval_stages as S
    targets, scene_gt, _ = S.dicts_of(b, poses=True)
    verts, info = S.b_models(b)
    ests = S.b_ests(b)
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

    patches = [(dataset_params, "get_split_params", lambda *a, **k: {"base_path": "base", "scene_gt_tpath": "gt|{scene_id}", "im_size": (B_WIDTH, 240),
                                                                      "scene_camera_tpath": "cam|{scene_id}", "depth_tpath": "depth",
                                                                      "scene_ids": [int(s) for s in b["scene_ids"]]}),
               (dataset_params, "get_model_params", lambda *a, **k: {"obj_ids": [int(o) for o in b["obj_ids"]], "models_info_path": "models_info",
                                                                      "symmetric_obj_ids": [int(o) for o in b["sym_obj_ids"]], "model_tpath": "{obj_id}"}),
               (inout, "load_json", load_json), (inout, "load_ply", lambda path: {"pts": verts[int(path)].astype(np.float64)}),
               (inout, "load_bop_results", lambda path, version="bop19": copy.deepcopy(ests)),
               (inout, "load_scene_gt", lambda path: copy.deepcopy(scene_gt[int(path.split("|")[1])])),
               (inout, "load_scene_camera", lambda path: copy.deepcopy(cams[int(path.split("|")[1])])),
               (inout, "save_json", save_json), (misc, "log", lambda s: None), (misc, "ensure_dir", lambda path: None)]
    old = [(m, n, getattr(m, n)) for m, n, _ in patches]
    argv = sys.argv
    try:
        for m, n, fn in patches:
            setattr(m, n, fn)
        sys.argv = ["eval_calc_errors.py", "--n_top=%d" % n_top, "--error_type=%s" % kind, "--result_filenames=m_ds-test.csv", "--results_path=res",
                    "--eval_path=eval", "--targets_filename=targets.json"]
        runpy.run_path(os.path.join(REF, "bop_toolkit", "scripts", "eval_calc_errors.py"), run_name="__main__")
    finally:
        sys.argv = argv
        for m, n, fn in old:
            setattr(m, n, fn)
    return saved


def guards(b, kind, rows, pairs, err):
    """-> None when the recorded errors of a kind can be compared with the device's, else what failed"""
    from tests import bop_eval_stages as S
    host, bound = S.host_errors(b, kind, rows, pairs, want_bounds=True)
    if not np.array_equal(np.isinf(host), np.isinf(err)):
        return "the sphere shortcut differs from the restatement's"
    div, factor = S.b_scale(b, kind, rows, pairs)
    norm, nb = (factor * err, factor * bound) if kind == "mspd" else (err / div, bound / div)
    fin = np.isfinite(norm)
    gap = np.abs(norm[fin, None] - np.asarray(B_PARAMS[kind][2], dtype=np.float64)[None, :]).min(1)
    if (gap < 4.0 * nb[fin]).any():
        return "an error within 4 bounds of a threshold"
    for r in np.unique(pairs[:, 0]):
        e, q = norm[(pairs[:, 0] == r) & fin], nb[(pairs[:, 0] == r) & fin]
        for x in range(len(e)):
            for y in range(x):
                if abs(e[x] - e[y]) < 4.0 * (q[x] + q[y]):
                    return "two errors of one estimate within 4 bounds of each other"
    if kind in ("ad", "add", "adi", "mssd"):
        dist = np.array([np.linalg.norm(a[1] - a[3]) for a in S._b_pair_args(b, rows, pairs)])
        if (np.abs(dist - div) < 1e-9 * div).any():
            return "|t_e - t_g| within 1e-9 diameters of the diameter"
        if not (np.isinf(err).any() and fin.any()):
            return "one side of the sphere shortcut is missing"
    return None


def stage_b():
    from tests import bop_eval_stages as S
    seed = 2100
    while True:
        b = draw_b(np.random.default_rng(seed))
        out, why = dict(b), None
        for kind, (n_top, visib_gt_min, ths) in B_PARAMS.items():
            saved = run_errors(b, kind, n_top)
            key, err = [], []
            for scene, lst in saved.items():
                for e in lst:
                    assert len(e["errors"]) > 0 or True
                    for g, v in e["errors"].items():
                        key.append((scene, e["im_id"], e["obj_id"], e["est_id"], g))
                        err.append(v[0])
            key, err = np.array(key, dtype=np.int64).reshape(-1, 5), np.array(err, dtype=np.float64)
            b[kind + "_th"], b[kind + "_params"] = np.asarray(ths, dtype=np.float64), np.array([n_top, visib_gt_min], dtype=np.float64)
            # the saved lists as flat tables: the estimates (those without a ground truth of their object included) and the pairs
            est_rows = np.array([(scene, e["im_id"], e["obj_id"], e["est_id"]) for scene, lst in saved.items() for e in lst], dtype=np.int64).reshape(-1, 4)
            counts = np.array([len(e["errors"]) for lst in saved.values() for e in lst], dtype=np.int64)
            pairs = np.stack([np.repeat(np.arange(len(counts)), counts), key[:, 4]], 1)
            src = S.expand(b, n_top)[0][:, 4]                   # only to find each saved estimate's pose again; checked on the next line
            assert np.array_equal(S.expand(b, n_top)[0][:, :4], est_rows), kind
            rows = np.concatenate([est_rows, src[:, None]], 1)
            why = guards(b, kind, rows, pairs, err)
            if why:
                print("seed %d, %s: %s -> redrawn" % (seed, kind, why))
                break
            fx = S.b_case(b, kind, rows, pairs, err, raw=True)
            rec = record(fx, kind, [([0], [float(t)]) for t in ths], n_top, visib_gt_min)
            out.update({kind + "_th": b[kind + "_th"], kind + "_params": b[kind + "_params"], kind + "_est": est_rows, kind + "_key": key, kind + "_err": err})
            out.update({kind + "_" + k: v for k, v in rec.items()})
            print("B %-5s n_top %2d  NE %3d  P %4d  inf %3d  matched %4d  recall %.3f .. %.3f" % (
                kind, n_top, len(est_rows), len(err), int(np.isinf(err).sum()), int((rec["m_est"] >= 0).sum()), rec["s_recall"].min(), rec["s_recall"].max()))
        if not why:
            out["seed"] = np.int64(seed)
            return out
        seed += 1


def main():
    out = {"names": np.array([c[0] for c in CASES])}
    out.update({"b_" + k: v for k, v in stage_b().items()})
    for k, (name, shapes, etype, c_err, ths, n_top, visib_gt_min) in enumerate(CASES):
        fx = draw_world(shapes, etype, c_err, np.random.default_rng(1100 + k))
        E = len(ths[0])
        if etype == "rete":
            columns = [([0, 1], th) for th in ths]
        else:
            columns = [([e], th) for e in range(c_err) for th in ths]
        C = len(columns)
        fx["col_err"] = np.array([c[0] for c in columns], dtype=np.int64)
        fx["col_th"] = np.array([c[1] for c in columns], dtype=np.float64)
        fx["params"] = np.array([n_top, visib_gt_min], dtype=np.float64)
        rec = record(fx, etype, columns, n_top, visib_gt_min)
        print("%-11s C %3d  NG %4d  NE %4d  P %6d  matched %6d  recall %.3f .. %.3f" % (
            name, C, rec["m_est"].shape[0], fx["est"].shape[0], fx["pair"].shape[0], int((rec["m_est"] >= 0).sum()),
            rec["s_recall"].min(), rec["s_recall"].max()))
        for key, v in list(fx.items()) + list(rec.items()):
            out["a%d_%s" % (k, key)] = v
    path = os.path.join(HERE, "bop_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 500000


if __name__ == "__main__":
    main()
