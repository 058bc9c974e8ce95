"""micro-benchmark of bop_eval.match + bop_eval.localization_scores (cp_bop_match, cp_bop_scores: BOP's greedy matching and recall
scores for every threshold column in one call), tools/bop_error_bench.py's method.

  python tools/bop_eval_bench.py --device [--out profiles/bop_eval_bench.json] [--calls 100] [--warmup 10] [--quick]
  python tools/bop_eval_bench.py --host-reference /path/to/reference [--out ...] [--quick]

Shapes: 1 000 / 20 000 targets (one (scene, image, object) each, five objects per image, ten scenes), 1 / 8 instances per target with
as many estimates (n_top = -1: n x n pairs per target), 1 / 100 threshold columns (100 = VSD's ten taus x ten thresholds: ten error
columns).  Seeded uniform errors in [0, 1), thresholds 0.05 .. 0.5, every ground truth valid.
--device: events around `--calls` calls after `--warmup` warm-ups of the whole Python calls, as a user pays them (match() uploads
its host tables on every call, outputs and scratch are allocated, localization_scores brings the counts back): `match_ms`,
`scores_ms` and `both_ms`.
--host-reference: bop_toolkit's own pose_matching.match_poses_scene + score.calc_localization_scores, imported from the given
tree, on the same tables, once per column as eval_calc_scores.py runs them, on this host's CPU with 16 threads set (single-threaded
Python loops; the thread setting changes nothing for them): `reference_host_ms`, the time of ALL the shape's columns; for 100 columns
three are timed and the figure is 100 x their mean (`reference_columns_timed` says so).  It is a host figure of another
implementation, not a device baseline; `ratio_host_over_device` is given for what it is when both parts have been run.
The two parts may run on different machines: each updates its own part of the JSON at --out and keeps the other."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(T, n, C) for T in (1000, 20000) for n in (1, 8) for C in (1, 100)]
TH10 = np.arange(0.05, 0.51, 0.05)


def world(T, n, rng):
    """-> (targets, scene_gt, ests without poses) in bop_toolkit's structures: T targets of n instances and n estimates each"""
    targets, scene_gt, ests = [], {}, []
    for k in range(T):
        scene, im, obj = 1 + (k // 5) % 10, k // 50, 1 + k % 5
        targets.append({"scene_id": scene, "im_id": im, "obj_id": obj, "inst_count": n})
        scene_gt.setdefault(scene, {}).setdefault(im, []).extend({"obj_id": obj} for _ in range(n))
        ests += [{"scene_id": scene, "im_id": im, "obj_id": obj, "score": float(s)} for s in rng.random(n)]
    return targets, scene_gt, ests


def columns(C):
    if C == 1:
        return 1, TH10[1:2], np.zeros(1, dtype=np.int64)
    return 10, np.tile(TH10, 10), np.repeat(np.arange(10), 10)


def table(P, c_err, seed):
    return np.random.default_rng(seed).random((P, c_err))


def run_device(a):
    import torch
    from checkerpose_amd import bop_eval as BE
    from tools.bop_error_bench import timed
    rows = []
    shapes, calls, warmup = (SHAPES, a.calls, a.warmup) if not a.quick else ([(1000, 8, 100)], 3, 1)
    for T, n, C in shapes:
        targets, scene_gt, ests = world(T, n, np.random.default_rng(T + n))
        es = BE.EvalSet.from_dicts(targets, scene_gt, None, list(range(1, 11)), list(range(1, 6)))
        pairs = BE.expand_pairs(es, ests, -1)
        c_err, th, cols = columns(C)
        errs = torch.from_numpy(table(pairs.pair_est.shape[0], c_err, 7)).to("cuda:0")
        valid = BE.gt_valid(es, -1)
        m = BE.match(pairs, errs, th, err_cols=cols, n_top=-1, valid=valid)
        sc = BE.localization_scores(es, m, valid, -1)
        t_m = timed(lambda: BE.match(pairs, errs, th, err_cols=cols, n_top=-1, valid=valid), calls, warmup)
        t_s = timed(lambda: BE.localization_scores(es, m, valid, -1), calls, warmup)
        t_b = timed(lambda: BE.localization_scores(es, BE.match(pairs, errs, th, err_cols=cols, n_top=-1, valid=valid), valid, -1), calls, warmup)
        rows.append({"targets": T, "instances": n, "columns": C, "pairs": int(pairs.pair_est.shape[0]), "match_ms": t_m, "scores_ms": t_s,
                     "both_ms": t_b, "recall_column0": float(sc["recall"][0]), "tp_column0": int(sc["tp_count"][0])})
        print("T=%5d n=%d C=%3d: match %.3f ms, scores %.3f ms, both %.3f ms; recall[0] %.4f" % (T, n, C, t_m, t_s, t_b, sc["recall"][0]), flush=True)
    return {"device": torch.cuda.get_device_name(0), "calls": calls, "warmup": warmup, "rows": rows}


def run_host(a):
    sys.path.insert(0, os.path.join(a.host_reference, "bop_toolkit"))
    from bop_toolkit_lib import pose_matching, score
    try:
        import torch
        torch.set_num_threads(16)
    except ImportError:
        pass
    rows = []
    for T, n, C in (SHAPES if not a.quick else [(1000, 1, 1), (1000, 8, 100)]):
        targets, scene_gt, ests = world(T, n, np.random.default_rng(T + n))
        c_err, th, cols = columns(C)
        tab = table(T * n * n, c_err, 7)                       # expand_pairs' order: targets in order, estimates by score, gt_id ascending
        valid = {s: {i: [True] * len(g) for i, g in ims.items()} for s, ims in scene_gt.items()}
        first = {}                                             # the gt_ids of a target: its n instances follow each other in the image's list
        for k, tg in enumerate(targets):
            first[k] = (k % 5) * n
        timed_cols = list(range(C))[:3]
        order = sorted(range(T), key=lambda k: (targets[k]["scene_id"], targets[k]["im_id"], targets[k]["obj_id"]))      # the EvalSet's
        elapsed, recall0 = 0.0, None
        for c in timed_cols:
            matches, scene_errs, p = [], {}, 0
            for k in order:
                tg = targets[k]
                for e in sorted(range(n), key=lambda e: ests[k * n + e]["score"], reverse=True):
                    scene_errs.setdefault(tg["scene_id"], []).append({
                        "im_id": tg["im_id"], "obj_id": tg["obj_id"], "est_id": e, "score": ests[k * n + e]["score"],
                        "errors": {first[k] + g: [float(tab[p + g, cols[c]])] for g in range(n)}})
                    p += n
            t1 = time.perf_counter()                           # the building of the dicts above is not timed
            for s in scene_gt:
                matches += pose_matching.match_poses_scene(s, scene_gt[s], valid[s], scene_errs[s], [float(th[c])], -1)
            sc = score.calc_localization_scores(list(range(1, 11)), list(range(1, 6)), matches, -1, do_print=False)
            elapsed += time.perf_counter() - t1
            recall0 = sc["recall"] if recall0 is None else recall0
        per_col = elapsed * 1e3 / len(timed_cols)
        rows.append({"targets": T, "instances": n, "columns": C, "reference_host_ms": per_col * C, "reference_columns_timed": len(timed_cols),
                     "recall_column0": float(recall0)})
        print("T=%5d n=%d C=%3d: reference on the host %.1f ms (%d columns timed)" % (T, n, C, per_col * C, len(timed_cols)), flush=True)
    return {"what": "bop_toolkit's pose_matching.match_poses_scene + score.calc_localization_scores, once per column, on the host CPU "
                    "(16 threads set; single-threaded Python loops); the building of their input dicts is not timed", "cpus": os.cpu_count(), "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bop_eval_bench.json"))
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--host-reference", default=None)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    res = {"bench": "bop_eval", "device": None, "device_figures": "UNMEASURED", "rows": [], "host": None}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res.update(json.load(f))
    if a.device:
        d = run_device(a)
        res.update({"device": d["device"], "calls": d["calls"], "warmup": d["warmup"], "rows": d["rows"],
                    "device_figures": "device events around the whole Python calls (tools/bop_eval_bench.py)"})
    if a.host_reference:
        res["host"] = run_host(a)
    if res["rows"] and res["host"]:
        host = {(r["targets"], r["instances"], r["columns"]): r["reference_host_ms"] for r in res["host"]["rows"]}
        for r in res["rows"]:
            k = (r["targets"], r["instances"], r["columns"])
            if k in host:
                r["ratio_host_over_device"] = host[k] / r["both_ms"]
    if not a.quick:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
