#!/usr/bin/env python3
"""Row N5 (pose errors) pinned by the REFERENCE's own code: ADD / ADI, diameters and the PoseCNN AUC.

Runs ONLY where the reference tree is (CHECKERPOSE_REFERENCE, default /root/reference; nothing of it travels, only the recorded
numbers in pose_error.npz are committed):

  python tests/golden/make_golden_pose_error.py

Uses `bop_toolkit_lib.pose_error.add` / `.adi` (pose_error.py:147-184), `bop_toolkit_lib.misc.calc_pts_diameter` (misc.py:279-293)
and `compute_auc_posecnn` of checkerpose/test.py (:37-57; test.py itself needs third-party modules this image lacks, so that ONE
function is compiled from its source while generating).  Everything is recorded in float64.

Vertices are NOT stored: every mesh is a row range [start, start + count) of checkerpose_amd/data/fps_lm_15x4096.npy flattened to
(61440, 3) -- the reference's own LM surface samples (fp32, cast to float64 for the reference calls).
  meshes   one object (4096); its first 1, 3, 63, 65, 1000, 4095 points; objects 0-2 cut to 9001; objects 0-4 (20480); all 15
           (61440); the 13 evaluated LM objects cut to 4096 - 37 k points (the mixed batch).
  poses    ground truth: random rotation, depth 400 - 1500 mm.  Estimate: the ground truth turned by m degrees about a random axis
           and moved by m mm in a random direction, m in {0, 0.2, 1, 5, 30, 180}; a half turn about the object's longest principal
           axis (ADI far below ADD); the solver's identity fallback R = I, t = 0 (depth >= 1050 mm: errors above a metre).
  groups   cases with one `group` id form one batch (the last group mixes the 13 meshes); the AUC is recorded per group and over all.
No recorded error lies within 1e-2 mm of 0.02 / 0.05 / 0.1 x diameter (asserted; the pose is redrawn otherwise), so a pass / fail bit
never hinges on rounding."""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "bop_toolkit"))
sys.path.insert(0, ROOT)

from bop_toolkit_lib import misc, pose_error  # noqa: E402
from checkerpose_amd.synthetic import LM_OBJ_IDS  # noqa: E402


def reference_auc():
    src = open(os.path.join(REF, "checkerpose", "test.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "compute_auc_posecnn"][0]
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "test.py", "exec"), ns)
    return ns["compute_auc_posecnn"]


def rodrigues(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def main():
    rng = np.random.default_rng(20240605)
    table = np.load(os.path.join(ROOT, "checkerpose_amd", "data", "fps_lm_15x4096.npy")).reshape(-1, 3).astype(np.float64)
    auc = reference_auc()
    meshes = [(0, 4096)] + [(0, n) for n in (1, 3, 63, 65, 1000, 4095)] + [(0, 9001), (0, 20480), (0, 61440)]
    mixed0 = len(meshes)
    meshes += [((o - 1) * 4096, 4096 - 37 * k) for k, o in enumerate(LM_OBJ_IDS)]
    diam = []
    for s, n in meshes:
        diam.append(misc.calc_pts_diameter(table[s:s + n]))
        print("mesh [%d, +%d): diameter %.6f" % (s, n, diam[-1]), flush=True)
    # (group, mesh, kind): kind = a perturbation magnitude, "half" or "ident"
    plan = [(0, 0, m) for m in (0, 0.2, 1, 5, 30, 180)] + [(0, 0, "half"), (0, 0, "ident")]
    for g, mi in enumerate(range(1, 7), start=1):
        plan += [(g, mi, m) for m in ((1, 5) if meshes[mi][1] == 1 else (0, 5))]
    plan += [(7, 7, m) for m in (0.2, 5, 30)] + [(8, 8, m) for m in (1, 30)] + [(9, 9, 5)]
    kinds = [0.2, 1, 5, 30, 180, 0, 1, 5, "half", 30, 0.2, "ident", 5]
    plan += [(10, mixed0 + k, kinds[k]) for k in range(13)]
    rec = {k: [] for k in ("group", "mesh", "R_gt", "t_gt", "R_est", "t_est", "add", "adi", "tag")}
    for g, mi, kind in plan:
        s, n = meshes[mi]
        pts = table[s:s + n]
        for attempt in range(100):
            R_gt = rodrigues(rng.normal(size=3), rng.uniform(0, 180))
            t_gt = np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(400, 1500)])
            if kind == "ident":
                t_gt[2] = rng.uniform(1050, 1500)                              # far enough for an error above a metre
                R_est, t_est = np.eye(3), np.zeros(3)
            elif kind == "half":
                c = pts - pts.mean(0)
                axis = np.linalg.eigh(c.T @ c)[1][:, -1]                    # longest principal axis, in the model frame
                R_est, t_est = R_gt @ rodrigues(axis, 180.0), t_gt + R_gt @ (pts.mean(0) - rodrigues(axis, 180.0) @ pts.mean(0))
            elif kind == 0:
                R_est, t_est = R_gt.copy(), t_gt.copy()
            else:
                d = rng.normal(size=3)
                R_est, t_est = rodrigues(rng.normal(size=3), kind) @ R_gt, t_gt + kind * d / np.linalg.norm(d)
            e_add = float(pose_error.add(R_est, t_est.reshape(3, 1), R_gt, t_gt.reshape(3, 1), pts))
            e_adi = float(pose_error.adi(R_est, t_est.reshape(3, 1), R_gt, t_gt.reshape(3, 1), pts))
            if all(abs(e - f * diam[mi]) >= 1e-2 for e in (e_add, e_adi) for f in (0.02, 0.05, 0.1)):
                break
        else:
            raise AssertionError("no pose clear of the thresholds for %r" % ((g, mi, kind),))
        assert all(abs(e - f * diam[mi]) >= 1e-2 for e in (e_add, e_adi) for f in (0.02, 0.05, 0.1))
        if kind == 0:
            assert e_add == 0.0 and e_adi == 0.0
        for k, v in zip(rec, (g, mi, R_gt, t_gt, R_est, t_est, e_add, e_adi, str(kind))):
            rec[k].append(v)
        print("group %2d mesh %2d (V=%5d) %-5s add %.6f adi %.6f" % (g, mi, n, kind, e_add, e_adi), flush=True)
    out = {k: np.array(v) for k, v in rec.items()}
    groups = sorted(set(rec["group"]))
    sel = [out["group"] == g for g in groups] + [np.ones(len(plan), bool)]          # last entry: all cases
    out["auc_add"] = np.array([auc(out["add"][m] / 1000.0) for m in sel], dtype=np.float64)
    out["auc_adi"] = np.array([auc(out["adi"][m] / 1000.0) for m in sel], dtype=np.float64)
    out["mesh_start"] = np.array([m[0] for m in meshes], dtype=np.int64)
    out["mesh_count"] = np.array([m[1] for m in meshes], dtype=np.int64)
    out["mesh_diameter"] = np.array(diam, dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "pose_error.npz"), **out)
    print("wrote pose_error.npz: %d cases, %d meshes" % (len(plan), len(meshes)))


if __name__ == "__main__":
    main()
