"""Row N11 (BOP's matching and recall scores): a float64 numpy restatement of every stage between an error table and the scores --
eval_calc_scores.py:186-238 (organising the targets, dropping unnamed images, validity), pose_matching.py:9-160 (greedy matching)
and score.py:62-137 (targets, true positives, recalls) -- on the flat arrays of tests/golden/bop_eval.npz.  Not a test file:
tests/test_bop_eval.py checks it against what the reference's own script recorded, tests/test_gpu_bop_eval.py uses it to build
inputs.  Every function takes `mut`, the name of ONE deliberate mistake (MUTATIONS), so that the CPU test can show that the
fixture tells the right rule from the wrong one."""
import numpy as np

MUTATIONS = ("argmin", "le", "last_tie", "unstable_sort", "ignore_valid", "targets_no_min", "mean_with_targets_only",
             "ntop_after_pairing")
B_KINDS = ("mssd", "mspd", "proj", "add", "adi", "ad")
_CACHE = {}


def fixture():
    """tests/golden/bop_eval.npz, read once: {case name: its arrays} for stage A, and under "B" the arrays of stage B"""
    if "g" not in _CACHE:
        from tests.common import golden
        g = golden("bop_eval")
        names = [str(n) for n in g["names"]]
        f = {n: {k[len("a%d_" % i):]: g[k] for k in g.files if k.startswith("a%d_" % i)} for i, n in enumerate(names)}
        f["B"] = {k[2:]: g[k] for k in g.files if k.startswith("b_")}
        _CACHE["g"] = f
    return _CACHE["g"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def evalset_of(fx, poses=False):
    from checkerpose_amd import bop_eval as BE
    targets, scene_gt, info = dicts_of(fx, poses)
    return BE.EvalSet.from_dicts(targets, scene_gt, info, fx["scene_ids"].tolist(), fx["obj_ids"].tolist())


def rows_of(targets, gt):
    """the ground-truth rows the script keeps, in the order of its `matches`: scenes and images in the order the targets first name
    them, gt_id ascending -> indices into gt"""
    order, seen = [], set()
    for s, i, _, _ in targets:
        if (s, i) not in seen:
            seen.add((s, i))
            order.append((s, i))
    scenes = []
    for s, _ in order:
        if s not in scenes:
            scenes.append(s)
    keep = []
    for s in scenes:
        for ss, i in order:
            if ss != s:
                continue
            idx = np.nonzero((gt[:, 0] == s) & (gt[:, 1] == i))[0]
            keep.extend(idx[np.argsort(gt[idx, 3], kind="stable")].tolist())
    return np.asarray(keep, dtype=np.int64)


def valid_mask(targets, gt, visib, rows, visib_gt_min):
    """eval_calc_scores.py:213-238 on the kept rows -> bool (len(rows),)"""
    inst = {}
    for s, i, o, n in targets:
        inst[(int(s), int(i), int(o))] = int(n)
    valid = np.zeros(len(rows), dtype=bool)
    if visib_gt_min >= 0:
        for k, r in enumerate(rows):
            valid[k] = tuple(int(x) for x in gt[r, :3]) in inst and visib[r] >= visib_gt_min
        return valid
    images = {}
    for k, r in enumerate(rows):
        images.setdefault((int(gt[r, 0]), int(gt[r, 1])), []).append(k)
    for ks in images.values():
        left = {}
        for k in sorted(ks, key=lambda k: visib[rows[k]], reverse=True):
            key = tuple(int(x) for x in gt[rows[k], :3])
            if key in inst and left.setdefault(key, inst[key]) > 0:
                valid[k] = True
                left[key] -= 1
    return valid


def _order(scores, mut):
    n = len(scores)
    if mut == "unstable_sort":                               # equal scores in reverse list order
        return sorted(range(n), key=lambda k: (-scores[k], -k))
    return sorted(range(n), key=lambda k: scores[k], reverse=True)


def match_group(errs, scores, valid, th, max_ests, mut=None):
    """pose_matching.match_poses.  errs (n_e, n_g, E), scores (n_e,), valid (n_g,) bool, th (E,)
    -> slot (n_g,) int (-1 = unmatched), error (n_g, E), error_norm (n_g, E) (-1.0 where unmatched)"""
    n_e, n_g, E = errs.shape
    slot = np.full(n_g, -1, dtype=np.int64)
    err, norm = np.full((n_g, E), -1.0), np.full((n_g, E), -1.0)
    order = _order(list(scores), mut)
    if max_ests > 0:
        order = order[:max_ests]
    th = np.asarray(th, dtype=np.float64)
    for e in order:
        best, best_err = -1, th.copy()
        free = [j for j in range(n_g) if (valid[j] or mut == "ignore_valid") and slot[j] < 0]
        if mut == "argmin":                                  # the smallest first element among those below the thresholds
            ok = [j for j in free if np.all(errs[e, j] < th)]
            if ok:
                best = min(ok, key=lambda j: errs[e, j, 0])
                best_err = errs[e, best]
        else:
            for j in free:
                c = errs[e, j]
                loose = mut == "le" or (mut == "last_tie" and best >= 0)      # last_tie: `<=` against an earlier candidate only
                if np.all(c <= best_err) if loose else np.all(c < best_err):
                    best, best_err = j, c
        if best >= 0:
            slot[best] = e
            err[best] = best_err
            norm[best] = best_err / th
    return slot, err, norm


def match_all(fx, rows, valid, mut=None):
    """every group and column of a fixture case -> est_id (NG, C), score (NG, C), error (NG, C, E), error_norm (NG, C, E)"""
    gt, est, pair, err = fx["gt"], fx["est"], fx["pair"], fx["err"]
    col_err, col_th, n_top = fx["col_err"], fx["col_th"], int(fx["params"][0])
    C, E = col_th.shape
    NG = len(rows)
    out_est = np.full((NG, C), -1, dtype=np.int64)
    out_score = np.full((NG, C), -1.0)
    out_err, out_norm = np.full((NG, C, E), -1.0), np.full((NG, C, E), -1.0)
    groups = {}
    for k, r in enumerate(rows):
        groups.setdefault(tuple(int(x) for x in gt[r, :3]), []).append(k)
    ests = {}
    for n in range(est.shape[0]):
        ests.setdefault(tuple(int(x) for x in est[n, :3]), []).append(n)
    first = np.searchsorted(pair[:, 0], np.arange(est.shape[0] + 1))      # the pairs of an estimate are consecutive
    for key, ks in groups.items():
        mine = ests.get(key, [])
        if not mine:
            continue
        n_g = len(ks)
        block = np.full((len(mine), n_g, err.shape[1]), np.nan)
        for a, n in enumerate(mine):
            seg = slice(first[n], first[n + 1])                 # a ground truth the estimate has no error for never matches it
            at = np.searchsorted(gt[rows[ks], 3], pair[seg, 1])
            assert np.array_equal(gt[rows[ks], 3][at], pair[seg, 1]), key
            block[a, at] = err[seg]
        scores = fx["score"][mine]
        for c in range(C):
            slot, e, nrm = match_group(block[:, :, col_err[c]], scores, valid[ks], col_th[c], n_top, mut)
            for j, k in enumerate(ks):
                if slot[j] >= 0:
                    out_est[k, c] = est[mine[slot[j]], 3]
                    out_score[k, c] = scores[slot[j]]
                    out_err[k, c], out_norm[k, c] = e[j], nrm[j]
    return out_est, out_score, out_err, out_norm


def scores(fx, rows, valid, est_id, mut=None):
    """score.calc_localization_scores per column -> dict of arrays (recall (C,), obj (n_obj, C), scene (n_scene, C), mobj, mscene
    (C,), counts (C, 3) = gt_count, targets, tp)"""
    gt, n_top = fx["gt"], int(fx["params"][0])
    obj_ids, scene_ids = [int(o) for o in fx["obj_ids"]], [int(s) for s in fx["scene_ids"]]
    C = est_id.shape[1]
    insts = {}
    for k, r in enumerate(rows):
        if valid[k]:
            key = (int(gt[r, 2]), int(gt[r, 0]), int(gt[r, 1]))
            insts[key] = insts.get(key, 0) + 1
    obj_t, scene_t = {o: 0 for o in obj_ids}, {s: 0 for s in scene_ids}
    for (o, s, _), n in insts.items():
        t = min(n_top, n) if (n_top > 0 and mut != "targets_no_min") else n
        obj_t[o] += t
        scene_t[s] += t
    tars = sum(obj_t.values())
    rec = lambda tp, t: 0.0 if t == 0 else tp / float(t)     # noqa: E731
    out = {"recall": np.zeros(C), "obj": np.zeros((len(obj_ids), C)), "scene": np.zeros((len(scene_ids), C)), "mobj": np.zeros(C),
           "mscene": np.zeros(C), "counts": np.zeros((C, 3), dtype=np.int64)}
    for c in range(C):
        obj_tp, scene_tp = {o: 0 for o in obj_ids}, {s: 0 for s in scene_ids}
        for k, r in enumerate(rows):
            if valid[k] and est_id[k, c] != -1:
                obj_tp[int(gt[r, 2])] += 1
                scene_tp[int(gt[r, 0])] += 1
        tps = sum(obj_tp.values())
        out["recall"][c] = rec(tps, tars)
        out["obj"][:, c] = [rec(obj_tp[o], obj_t[o]) for o in obj_ids]
        out["scene"][:, c] = [rec(scene_tp[s], scene_t[s]) for s in scene_ids]
        if mut == "mean_with_targets_only":
            out["mobj"][c] = float(np.mean([rec(obj_tp[o], obj_t[o]) for o in obj_ids if obj_t[o] > 0] or [0.0]))
        else:
            out["mobj"][c] = float(np.mean(list(out["obj"][:, c])))
        out["mscene"][c] = float(np.mean(list(out["scene"][:, c])))
        out["counts"][c] = (len(rows), tars, tps)
    return out


def scene_errs_of(fx, cols=None):
    """{scene_id: the script's scene_errs list} of a fixture case, each estimate's errors restricted to the error columns `cols`"""
    est, pair, err = fx["est"], fx["pair"], fx["err"]
    first = np.searchsorted(pair[:, 0], np.arange(est.shape[0] + 1))
    out = {}
    for n in range(est.shape[0]):
        seg = slice(first[n], first[n + 1])
        vals = err[seg] if cols is None else err[seg][:, cols]
        out.setdefault(int(est[n, 0]), []).append({"im_id": int(est[n, 1]), "obj_id": int(est[n, 2]), "est_id": int(est[n, 3]),
                                                   "score": float(fx["score"][n]),
                                                   "errors": {int(g): [float(x) for x in v] for g, v in zip(pair[seg, 1], vals)}})
    return out


def dicts_of(fx, poses=False):
    """(targets, scene_gt, scene_gt_info) in bop_toolkit's structures; poses: with stage B's cam_R_m2c / cam_t_m2c"""
    targets = [{"scene_id": int(s), "im_id": int(i), "obj_id": int(o), "inst_count": int(n)} for s, i, o, n in fx["targets"]]
    scene_gt, info = {}, {}
    for r, ((s, i, o, g), v) in enumerate(zip(fx["gt"], fx["visib"])):
        lst = scene_gt.setdefault(int(s), {}).setdefault(int(i), [])
        assert len(lst) == int(g)
        lst.append({"obj_id": int(o)})
        if poses:
            lst[-1].update({"cam_R_m2c": fx["gt_R"][r].copy(), "cam_t_m2c": fx["gt_t"][r].reshape(3, 1).copy()})
        info.setdefault(int(s), {}).setdefault(int(i), []).append({"visib_fract": float(v)})
    return targets, scene_gt, info


# ---- stage B: eval_calc_errors.py:193-290 (the targets' top-n estimates x the ground truths of their object) and the errors ---------------
def b_ests(b):
    """stage B's estimates as inout.load_bop_results' list"""
    return [{"scene_id": int(k[0]), "im_id": int(k[1]), "obj_id": int(k[2]), "score": float(s), "R": R.copy(), "t": t.reshape(3, 1).copy(), "time": -1.0}
            for k, s, R, t in zip(b["est"], b["score"], b["est_R"], b["est_t"])]


def b_models(b):
    """(meshes {obj_id: float32 vertices}, models_info {obj_id: dict}) of stage B: the closed-form meshes of tests/vsd_stages.py,
    checked against the recorded CRC"""
    import json
    import zlib
    from tests import vsd_stages as V
    m = V.meshes()
    verts = {int(o): m[str(n)][0] for o, n in zip(b["obj_ids"], b["mesh"])}
    for o, crc in zip(b["obj_ids"], b["mesh_crc"]):
        assert zlib.crc32(verts[int(o)].tobytes()) == int(crc), "mesh of object %d is not the recorded one" % int(o)
    return verts, {int(o): json.loads(str(j)) for o, j in zip(b["obj_ids"], b["info"])}


def expand(b, n_top, mut=None):
    """eval_calc_errors.py:245-290 -> (rows (n, 5): scene, im, obj, est_id, index into b["est"];  pairs (P, 2): row, gt_id), in the
    order the script saves them.  mut "ntop_after_pairing": the first n_top (estimate, ground truth) PAIRS instead of estimates"""
    org, by = {}, {}
    for s, i, o, n in b["targets"].tolist():
        org.setdefault(s, {}).setdefault(i, {})[o] = n
    for n, key in enumerate(map(tuple, b["est"].tolist())):
        by.setdefault(key, []).append(n)
    rows, pairs = [], []
    for s, ims in org.items():
        for i, objs in ims.items():
            for o, inst in objs.items():
                top = None if n_top == 0 else (inst if n_top == -1 else n_top)
                mine = by.get((s, i, o), [])
                order = sorted(range(len(mine)), key=lambda k: b["score"][mine[k]], reverse=True)
                gts = [r[3] for r in b["gt"].tolist() if tuple(r[:3]) == (s, i, o)]
                keep = None
                if mut == "ntop_after_pairing":
                    keep = [(k, g) for k in order for g in gts][slice(0, top)]
                    order = list(dict.fromkeys(k for k, _ in keep))
                else:
                    order = order[slice(0, top)]
                for k in order:
                    rows.append((s, i, o, k, mine[k]))
                    pairs += [(len(rows) - 1, g) for g in gts if keep is None or (k, g) in keep]
    return np.array(rows, dtype=np.int64).reshape(-1, 5), np.array(pairs, dtype=np.int64).reshape(-1, 2)


def _b_pair_args(b, rows, pairs):
    """per pair: (R_e, t_e, R_g, t_g, K, obj)"""
    gt_row = {tuple(k): r for r, k in enumerate(b["gt"].tolist())}
    cam = {tuple(k): n for n, k in enumerate(b["cam"].tolist())}
    for r, g in pairs.tolist():
        s, i, o, _, n = rows[r].tolist()
        q = gt_row[(s, i, o, g)]
        yield b["est_R"][n], b["est_t"][n], b["gt_R"][q], b["gt_t"][q], b["K"][cam[(s, i)]], o


def host_errors(b, kind, rows, pairs, want_bounds=False):
    """the errors of the pairs in float64 (pose_error's functions as tests/test_pose_error.py and tests/test_bop_error.py restate
    them), with eval_calc_errors.py:304-339's sphere shortcut -> (P,) [, the rows' N5 / N7 bounds of the device's error (P,)]"""
    from checkerpose_amd import metric
    from tests import test_bop_error as TB, test_pose_error as TP
    verts, info = b_models(b)
    sym_objs = set(b["sym_obj_ids"].tolist())
    tables = {o: np.stack([np.concatenate([t["R"].reshape(9), t["t"].reshape(3)]) for t in metric.symmetry_transformations(info[o], 0.01)])
              for o in verts}
    one = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])[None]
    err, bound = [], []
    for Re, te, Rg, tg, K, o in _b_pair_args(b, rows, pairs):
        pts = verts[o]
        if kind in ("ad", "add", "adi", "mssd") and not np.linalg.norm(te - tg) < info[o]["diameter"]:
            err.append(float("inf"))
            bound.append(0.0)
            continue
        if kind in ("mssd", "mspd", "proj"):
            T = one if kind == "proj" else tables[o]
            e = TB.restate(Re, te, Rg, tg, K, pts, T, np.float64)[("mssd", "mspd", "proj").index(kind)]
            if want_bounds:
                bound.append(TB.tolerances(TB.scales(Re, te, Rg, tg, K, pts, T), (e, e, e))[("mssd", "mspd", "proj").index(kind)])
        else:
            adi = kind == "adi" or (kind == "ad" and o in sym_objs)
            e = (TP.host_adi if adi else TP.host_add)(Re, te, Rg, tg, pts)
            if want_bounds:
                bound.append(TP.tolerance(Re, te, Rg, tg, pts, e))
        err.append(e)
    return (np.array(err), np.array(bound)) if want_bounds else np.array(err)


def b_scale(b, kind, rows, pairs):
    """what eval_calc_scores.py:246-258 does to an error before the thresholds: (divisor, factor) per pair -- e / diameter for
    "ad" / "add" / "adi" / "mssd", (640 / width) * e for "mspd"."""
    _, info = b_models(b)
    div = np.array([info[int(rows[r, 2])]["diameter"] if kind in ("ad", "add", "adi", "mssd") else 1.0 for r in pairs[:, 0]], dtype=np.float64)
    return div.reshape(-1), (640.0 / float(b["width"]) if kind == "mspd" else 1.0)


def b_case(b, kind, rows, pairs, err, raw=False):
    """stage B's tables of one kind in the layout of a stage A case (match_all, scores, scene_errs_of, dicts_of read it); err: the
    (P,) errors as eval_calc_errors.py saves them -- normalised here as eval_calc_scores.py does"""
    div, factor = b_scale(b, kind, rows, pairs)
    e = np.asarray(err, dtype=np.float64)
    if not raw:
        e = e / div if kind != "mspd" else factor * e
    th = np.asarray(b[kind + "_th"], dtype=np.float64).reshape(-1, 1)
    return {"targets": b["targets"], "gt": b["gt"], "visib": b["visib"], "est": rows[:, :4], "score": b["score"][rows[:, 4]], "pair": pairs,
            "err": e.reshape(-1, 1), "col_err": np.zeros((th.shape[0], 1), dtype=np.int64), "col_th": th, "params": b[kind + "_params"],
            "scene_ids": b["scene_ids"], "obj_ids": b["obj_ids"], "diam": b["diam"], "width": b["width"]}
