#!/usr/bin/env python
"""Row N23 (rotation / translation errors against the closest symmetric ground truth, the LM report) pinned by the REFERENCE's own
statements.

Runs ONLY where the reference tree is (CHECKERPOSE_REFERENCE, default /root/reference; nothing of it travels, only the recorded
arrays and the recorded text).  Compiled with `ast` while generating, never copied: `get_closest_rot` (test_lm.py:33-55),
`load_lm_obj_sym_info` (lm_dataset_pytorch.py:552-563; `mmcv.load` is a JSON reader over a synthetic 15-entry models_info written
to a temporary file), the per-crop statements test_lm.py:299-327 and the summary :372-419.  `pose_error.re` / `.te`,
`misc.get_symmetry_transformations` and eval_calc_errors.py / eval_calc_scores.py are imported / run as they are.

  cases    pose pairs over four objects -- asymmetric (no sym_info), one discrete half turn, one continuous axis with an offset, a
           continuous axis plus a discrete flip: S = 0 (1 through SymmetrySet), 2, 314, 628.  Half of the drawn pairs are
           dR . R_gt . S_j with |dR| of a few hundredths of a radian, half uniformly random rotations; then the equal pair, an exact
           symmetric copy, half turns, translations with te within 1 mm of 20 and of 50.  Recorded: the reference's re, the index
           of the matrix get_closest_rot returned and the matrix, error_cos of that candidate before the clamp, te, the gap to the
           reference's best candidate with a DIFFERENT matrix.
  report   156 crops of the 13 LINEMOD objects through the statements :299-327, the ADD / ADI functions replaced by a table lookup
           (rows N5 pin those), then :372-419 -> the nine flags per crop, the per-object and overall rates, test_res_str.
  match    the multi-estimate world of tests/golden/bop_eval.npz (stage B) through eval_calc_errors.py --error_type=rete and
           eval_calc_scores.py: the (re, te) table and the matches pose_matching.match_poses made of it.

Asserted while generating (a case is redrawn otherwise): every error at least 1e-6 relative from each of its thresholds; at most
5 % of the symmetric cases have the reference's two best distinct candidates within 2 tol of each other; at least one case has a
cofactor cosine outside [-1, 1] (what the clamp is for).

    python tests/golden/make_golden_rete.py        -> tests/golden/rete.npz"""
import ast
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "bop_toolkit"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from bop_toolkit_lib import misc, pose_error  # noqa: E402

from tests import rete_stages as RS  # noqa: E402

MARGIN = 1e-6
CASE_OBJS = (1, 10, 11, 3)                  # the four kinds of symmetry set, as mesh 0 .. 3 of the cases
MATCH_TH = [[5.0, 5.0], [15.0, 20.0], [40.0, 60.0]]


def _tree(rel):
    return ast.parse(open(os.path.join(REF, "checkerpose", rel)).read())


def _functions(rel, names, ns):
    fns = [n for n in _tree(rel).body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(f.name for f in fns) == sorted(names), (rel, names)
    exec(compile(ast.Module(body=fns, type_ignores=[]), rel, "exec"), ns)


def _names(stmt):
    return [n.id for t in getattr(stmt, "targets", []) for n in ast.walk(t) if isinstance(n, ast.Name)]


def reference_pieces():
    ns = {"np": np, "torch": torch, "pose_error": pose_error, "misc": misc,
          "mmcv": types.SimpleNamespace(load=lambda path: json.load(open(path)))}
    _functions("test_lm.py", ["get_closest_rot"], ns)
    _functions("lm_dataset_pytorch.py", ["load_lm_obj_sym_info"], ns)
    main = [n for n in _tree("test_lm.py").body if isinstance(n, ast.FunctionDef) and n.name == "main"][0]
    for s in main.body:                                              # symmetry_ids and lm13_obj_ids, as the script sets them
        if isinstance(s, ast.Assign) and _names(s) in (["symmetry_ids"], ["lm13_obj_ids"]):
            exec(compile(ast.Module(body=[s], type_ignores=[]), "test_lm.py", "exec"), ns)
    per_crop = None
    for node in ast.walk(main):
        body = getattr(node, "body", None)
        if not isinstance(body, list):
            continue
        i0 = [i for i, s in enumerate(body) if isinstance(s, ast.If) and ast.unparse(s.test) == "obj_id in symmetry_ids"
              and "Calculate_Pose_Error_Main" in [n for b in s.body for n in _names(b)]]
        i1 = [i for i, s in enumerate(body) if isinstance(s, ast.Expr) and ast.unparse(s).startswith("te5_passed_dict[obj_id].append")]
        if i0 and i1:
            assert per_crop is None and i0[0] < i1[0]
            per_crop = compile(ast.Module(body=body[i0[0]:i1[0] + 1], type_ignores=[]), "test_lm.py", "exec")
    assert per_crop is not None
    j0 = next(i for i, s in enumerate(main.body) if "adx2_passed_arr" in _names(s))
    j1 = next(i for i, s in enumerate(main.body) if "test_res_str" in _names(s))
    summary = compile(ast.Module(body=main.body[j0:j1 + 1], type_ignores=[]), "test_lm.py", "exec")
    return ns, per_crop, summary


def synthetic_models_info():
    """15 entries as models_info.json has them; the symmetric ones are test_lm.py's symmetry_ids"""
    rng = np.random.default_rng(23)
    info = {str(o): {"diameter": float(np.round(rng.uniform(90.0, 300.0), 3)), "min_x": -50.0, "size_x": 100.0} for o in range(1, 16)}
    info["10"]["symmetries_discrete"] = [[-1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]]     # half turn about z (eggbox / glue style)
    info["11"]["symmetries_continuous"] = [{"axis": [0, 0, 1], "offset": [3.5, -2.0, 0.0]}]
    info["3"]["symmetries_continuous"] = [{"axis": [0, 1, 0], "offset": [0, 0, 0]}]
    info["3"]["symmetries_discrete"] = [[1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 1.5, 0.0, 0.0, 0.0, 1.0]]      # flip about x, shifted
    info["7"]["symmetries_discrete"] = [[-1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0]]
    return info


def rotation(rng, angle=None):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    angle = rng.uniform(0, np.pi) if angle is None else angle
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def uniform_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def reference_closest(ns, R_est, R_gt, sym_info):
    """get_closest_rot and pose_error.re, then -- with the same two functions -- which candidate that was and how far the best
    candidate with a different matrix lies -> (re, index, closest matrix, error_cos of the winner before the clamp, gap)"""
    closest = ns["get_closest_rot"](R_est, R_gt, sym_info)
    re = pose_error.re(R_est, closest)
    mats = [R_gt] + ([] if sym_info is None else [R_gt.dot(s) for s in sym_info])
    if closest is R_gt:
        index = -1
    else:
        index = next(i for i, m in enumerate(mats[1:]) if np.array_equal(m, closest))
    cos = float(0.5 * (np.trace(R_est.dot(np.linalg.inv(closest))) - 1.0))
    others = [pose_error.re(R_est, m) for m in mats if not np.array_equal(m, closest)]
    gap = (min(others) - re) if others else np.inf
    return re, index, closest, cos, gap


def clear(value, thresholds):
    return all(abs(value - th) > MARGIN * th for th in thresholds)


def draw_cases(ns, sym_info, rng):
    rows = []

    def add(kind, m, R_gt, R_est, t_gt, t_est):
        si = sym_info[CASE_OBJS[m]]
        re, index, closest, cos, gap = reference_closest(ns, R_est, R_gt, si)
        te = float(pose_error.te(t_est.reshape(3, 1), t_gt.reshape(3, 1)))
        if not (clear(re, (2.0, 5.0)) and clear(te, (20.0, 50.0))):
            return False
        rows.append(dict(kind=kind, mesh=m, R_gt=R_gt, R_est=R_est, t_gt=t_gt, t_est=t_est, re=re, index=index, closest=closest, cos=cos, gap=gap, te=te))
        return True

    def t_pair(mag=None):
        t_gt = np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(500, 1100)])
        d = rng.normal(size=3)
        d *= (rng.uniform(1.0, 80.0) if mag is None else mag) / np.linalg.norm(d)
        return t_gt, t_gt + d

    for m, obj in enumerate(CASE_OBJS):
        si = sym_info[obj]
        member = lambda: np.eye(3) if si is None else si[int(rng.integers(len(si)))].astype(np.float64)      # noqa: E731
        n = 0
        while n < 24:                                                # the regime of a trained net: near a symmetric copy
            R_gt = uniform_rotation(rng)
            n += add(0, m, R_gt, rotation(rng, rng.uniform(0.01, 0.06)) @ R_gt.dot(member()), *t_pair())
        n = 0
        while n < 24:
            n += add(1, m, uniform_rotation(rng), uniform_rotation(rng), *t_pair())
        R_gt = uniform_rotation(rng)
        assert add(2, m, R_gt, R_gt.copy(), *t_pair())                # the equal pair
        R_gt = uniform_rotation(rng)
        assert add(3, m, R_gt, R_gt.dot(member()), *t_pair())         # an exact symmetric copy
        for _ in range(6 if si is None else 2):                       # half turns
            R_gt = uniform_rotation(rng)
            assert add(4, m, R_gt, R_gt.dot(rotation(rng, np.pi)), *t_pair())
        for mag in (20.0, 50.0):                                      # te within 1 mm of a threshold, on either side
            for side in (-1.0, 1.0):
                while not add(5, m, uniform_rotation(rng), uniform_rotation(rng), *t_pair(mag + side * rng.uniform(0.01, 1.0))):
                    pass
    return rows


def draw_report(ns, per_crop, summary, info, sym_info, rng):
    lm13 = ns["lm13_obj_ids"]
    diam = {o: info[str(o)]["diameter"] for o in range(1, 16)}
    crops = []
    for obj in lm13:
        for _ in range(12):
            crops.append(obj)
    crops = [crops[k] for k in rng.permutation(len(crops))]
    n = len(crops)
    add_tab, adi_tab = np.zeros(n), np.zeros(n)
    names = ("adx2", "adx5", "adx10", "rete2", "rete5", "re2", "re5", "te2", "te5")
    env = dict(ns, obj_diameter_dict=diam, obj_sym_info_dict=sym_info, vertices_dict={o: None for o in lm13})
    env.update({k + "_passed_dict": {o: [] for o in lm13} for k in names})
    cur = {}
    env["Calculate_ADD_Error_BOP"] = lambda rG, tG, pr, pt, v: add_tab[cur["i"]]
    env["Calculate_ADI_Error_BOP"] = lambda rG, tG, pr, pt, v: adi_tab[cur["i"]]
    rec = dict(R_gt=np.zeros((n, 3, 3)), R_est=np.zeros((n, 3, 3)), t_gt=np.zeros((n, 3)), t_est=np.zeros((n, 3)), re=np.zeros(n), te=np.zeros(n),
               adx=np.zeros(n), flags=np.zeros((n, 9), dtype=np.int32))
    for i, obj in enumerate(crops):
        cur["i"] = i
        si = sym_info[obj]
        while True:
            R_gt = uniform_rotation(rng)
            S = np.eye(3) if si is None else si[int(rng.integers(len(si)))].astype(np.float64)
            R_est = uniform_rotation(rng) if rng.random() < 0.25 else rotation(rng, rng.uniform(0.01, 0.12)) @ R_gt.dot(S)
            t_gt = np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(500, 1100)])
            d = rng.normal(size=3)
            d *= float(rng.choice([5.0, 19.5, 20.4, 35.0, 49.6, 50.5, 80.0])) * rng.uniform(0.995, 1.005) / np.linalg.norm(d)
            t_est = t_gt + d
            add_tab[i] = diam[obj] * float(rng.choice([0.01, 0.0195, 0.0205, 0.04, 0.0495, 0.0505, 0.09, 0.101, 0.3])) * rng.uniform(0.999, 1.001)
            adi_tab[i] = 0.6 * add_tab[i]
            if i == 7:
                add_tab[i] = adi_tab[i] = np.nan                      # NaN counts as 10000 (:306-307)
            if i == 19:
                t_est = t_est * np.nan                                # ... and so does a NaN translation error (:316-317)
            before = {k: len(env[k + "_passed_dict"][obj]) for k in names}
            env.update(obj_id=obj, r_GT=R_gt, t_GT=t_gt.reshape(3, 1), pred_rot=R_est, pred_trans=t_est.reshape(3, 1))
            exec(per_crop, env)
            adx = adi_tab[i] if obj in ns["symmetry_ids"] else add_tab[i]
            ok = clear(env["err_rot"], (2.0, 5.0)) and clear(env["err_trans"], (20.0, 50.0))
            ok = ok and (np.isnan(adx) or clear(adx, [f * diam[obj] for f in (0.02, 0.05, 0.1)]))
            assert all(len(env[k + "_passed_dict"][obj]) == before[k] + 1 for k in names)
            if ok:
                break
            for k in names:                                           # redraw: take the crop's flags back
                env[k + "_passed_dict"][obj].pop()
        rec["R_gt"][i], rec["R_est"][i], rec["t_gt"][i], rec["t_est"][i] = R_gt, R_est, t_gt, t_est
        rec["re"][i], rec["te"][i], rec["adx"][i] = env["err_rot"], env["err_trans"], env["adx_error"]
        rec["flags"][i] = [int(env[k + "_passed_dict"][obj][-1]) for k in names]
    bits = 6
    env.update(adx_type="all", roi_bit_acc_arr=rng.uniform(0.9, 1.0, n), reproj_x_acc_arr=rng.uniform(0.95, 1.0, n),
               reproj_y_acc_arr=rng.uniform(0.95, 1.0, n), bit_err_arr=rng.uniform(0.0, 0.2, (n, 2 * bits + 1)),
               visib_pixel_acc_arr=rng.uniform(0.9, 1.0, n), visib_iou_arr=rng.uniform(0.7, 1.0, n),
               full_pixel_acc_arr=rng.uniform(0.9, 1.0, n), full_iou_arr=rng.uniform(0.7, 1.0, n))
    figs = {k[:-4]: env[k].copy() for k in ("roi_bit_acc_arr", "reproj_x_acc_arr", "reproj_y_acc_arr", "visib_pixel_acc_arr", "visib_iou_arr",
                                            "full_pixel_acc_arr", "full_iou_arr")}
    figs["bit_err_arr"] = env["bit_err_arr"].copy()
    exec(summary, env)
    out = {"rep_" + k: v for k, v in rec.items()}
    out.update({"rep_fig_" + k: v for k, v in figs.items()})
    out.update(rep_obj=np.array(crops, dtype=np.int64), rep_add=add_tab, rep_adi=adi_tab, rep_diam=np.array([diam[o] for o in crops]),
               rep_lm13=np.array(lm13, dtype=np.int64), rep_symmetry_ids=np.array(ns["symmetry_ids"], dtype=np.int64),
               rep_rates=np.stack([env[k + "_passed_arr"] for k in names], 1), rep_overall=np.array([env[k + "_passed"] for k in names]),
               rep_text=np.array(env["test_res_str"]))
    return out


def stage_match():
    """stage B's world of bop_eval.npz through eval_calc_errors.py (rete) and eval_calc_scores.py"""
    import make_golden_bop_eval as G
    from tests import bop_eval_stages as S
    b = dict(S.fixture()["B"])
    n_top = -1
    saved = G.run_errors(b, "rete", n_top)
    key, err = [], []
    for scene, lst in saved.items():
        for e in lst:
            for g, v in e["errors"].items():
                key.append((scene, e["im_id"], e["obj_id"], e["est_id"], g))
                err.append(v)
    key, err = np.array(key, dtype=np.int64).reshape(-1, 5), np.array(err, dtype=np.float64).reshape(-1, 2)
    est_rows = np.array([(scene, e["im_id"], e["obj_id"], e["est_id"]) for scene, lst in saved.items() for e in lst], dtype=np.int64).reshape(-1, 4)
    counts = np.array([len(e["errors"]) for lst in saved.values() for e in lst], dtype=np.int64)
    pairs = np.stack([np.repeat(np.arange(len(counts)), counts), key[:, 4]], 1)
    rows, prs = S.expand(b, n_top)
    assert np.array_equal(rows[:, :4], est_rows) and np.array_equal(prs, pairs)
    th = np.asarray(MATCH_TH, dtype=np.float64)
    for e in (0, 1):                                                  # clear of every threshold, and no two errors of one estimate alike
        assert (np.abs(err[:, e, None] - th[None, :, e]) > 1e-6 * th[None, :, e]).all()
    for r in np.unique(pairs[:, 0]):
        e = err[pairs[:, 0] == r]
        for x in range(len(e)):
            for y in range(x):
                assert np.abs(e[x] - e[y]).min() > 1e-6
    fx = {"targets": b["targets"], "gt": b["gt"], "visib": b["visib"], "est": est_rows, "score": b["score"][rows[:, 4]], "pair": pairs, "err": err,
          "scene_ids": b["scene_ids"], "obj_ids": b["obj_ids"], "diam": b["diam"], "width": b["width"]}
    rec = G.record(fx, "rete", [([0, 1], t) for t in MATCH_TH], n_top, -1)
    print("match: P %d, matched %d of %d x %d, recall %s" % (len(err), int((rec["m_est"] >= 0).sum()), rec["m_est"].shape[0], len(MATCH_TH), rec["s_recall"]))
    out = {"match_key": key, "match_err": err, "match_th": th, "match_params": np.array([n_top, -1.0])}
    out.update({"match_" + k: v for k, v in rec.items()})
    return out


def probe(rows, sym_info):
    """the cofactor form against the reference's trace(R_est . inv(R_gt . S)) over the cases x sampled members, in eps"""
    worst = 0.0
    for r in rows:
        si = sym_info[CASE_OBJS[r["mesh"]]]
        mats = [r["R_gt"]] + ([] if si is None else [r["R_gt"].dot(s) for s in si[::7]])
        for m in mats:
            ref = float(0.5 * (np.trace(r["R_est"].dot(np.linalg.inv(m))) - 1.0))
            worst = max(worst, abs(RS.cos_cof(r["R_est"], m) - ref) / RS.EPS)
    return worst


def main():
    ns, per_crop, summary = reference_pieces()
    info = synthetic_models_info()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "models_info.json")
        json.dump(info, open(path, "w"))
        sym_info = ns["load_lm_obj_sym_info"](path)
    assert [None if sym_info[o] is None else len(sym_info[o]) for o in CASE_OBJS] == [None, 2, 314, 628]
    assert all(sym_info[o] is None or sym_info[o].dtype == np.float32 for o in sym_info)
    seed = 2300
    while True:
        rng = np.random.default_rng(seed)
        rows = draw_cases(ns, sym_info, rng)
        symm = [r for r in rows if r["mesh"] > 0]
        near = [r for r in symm if r["gap"] <= 2.0 * float(RS.tol_re(r["cos"]))]
        outside = [r for r in rows if abs(RS.closest(r["R_est"], r["R_gt"], None if sym_info[CASE_OBJS[r["mesh"]]] is None else
                                                     sym_info[CASE_OBJS[r["mesh"]]].astype(np.float64))[1]) > 1.0]
        if len(near) <= 0.05 * len(symm) and outside:
            break
        print("seed %d: %d near ties of %d, %d cosines outside [-1, 1] -> redrawn" % (seed, len(near), len(symm), len(outside)))
        seed += 1
    print("cases: %d (seed %d), %d symmetric, %d within 2 tol of a distinct candidate, smallest other gap %.3e degrees, %d cosines outside [-1, 1]" % (
        len(rows), seed, len(symm), len(near), min(r["gap"] for r in symm if r["gap"] > 2.0 * float(RS.tol_re(r["cos"]))), len(outside)))
    print("plain candidate kept (index -1) in %d of %d cases on the discrete set" % (
        sum(r["index"] == -1 for r in rows if r["mesh"] == 1), sum(r["mesh"] == 1 for r in rows)))
    print("probe: cofactor cosine against trace(R_est . inv(R_gt . S)): at most %.1f eps" % probe(rows, sym_info))
    out = {"models_info": np.array(json.dumps(info)), "case_objs": np.array(CASE_OBJS, dtype=np.int64), "seed": np.int64(seed)}
    for o in CASE_OBJS[1:]:
        out["sym_info_%d" % o] = sym_info[o]
    for k in ("R_gt", "R_est", "t_gt", "t_est", "re", "cos", "gap", "te", "closest"):
        out["case_" + k] = np.array([r[k] for r in rows], dtype=np.float64)
    for k in ("kind", "mesh", "index"):
        out["case_" + k] = np.array([r[k] for r in rows], dtype=np.int64)
    out.update(draw_report(ns, per_crop, summary, info, sym_info, np.random.default_rng(seed + 1)))
    print(str(out["rep_text"]))
    out.update(stage_match())
    path = os.path.join(HERE, "rete.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 500000


if __name__ == "__main__":
    main()
