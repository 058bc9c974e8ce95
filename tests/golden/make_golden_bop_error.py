#!/usr/bin/env python3
"""Row N7 (BOP's MSSD / MSPD / projection error) pinned by the REFERENCE's own code.

Runs ONLY where the reference tree is (CHECKERPOSE_REFERENCE, default /root/reference; nothing of it travels, only the recorded
numbers in bop_error.npz are committed):

  python tests/golden/make_golden_bop_error.py

Uses `bop_toolkit_lib.pose_error.mssd` / `.mspd` / `.proj` (pose_error.py:96-144, 217-232), `misc.get_symmetry_transformations`
(misc.py:43-90), `misc.calc_pts_diameter` and `pose_matching.match_poses` (one estimate against one ground truth, per threshold of
eval_bop19_pose.py:46,51, after the normalisation of eval_calc_scores.py:246-258 at an image width of 640).  Everything is
recorded in float64.

Vertices are NOT stored: every mesh is a row range [start, start + count) of checkerpose_amd/data/fps_lm_15x4096.npy flattened to
(61440, 3) (fp32, cast to float64 for the reference calls).
  meshes   the first 1, 3, 63, 65, 1000, 4095, 4096, 9001, 20480 points; the 13 evaluated LM objects cut to 4096 - 37 k points.
  sets     get_symmetry_transformations of the small model-info dicts of SETS (recorded as JSON with their step): none (S = 1), one
           discrete half turn about an axis off the origin (2), three discrete (4), a continuous axis at steps giving 63, 64 and 65,
           step 0.01 with an offset plus one discrete symmetry (628), step 0.005 plus one discrete symmetry (1256).  The full
           transform lists of the S = 4, 65 and 628 sets are recorded (`set_T_<id>`).
  poses    ground truth: random rotation, depth 400 - 1500 mm.  Estimate: the ground truth turned by m degrees about a random axis
           and moved by m mm, m in {0, 0.2, 1, 5, 30}; the solver's identity fallback R = I, t = 0; "k<i>": the ground truth composed
           with symmetry i of the set, then perturbed by 0.2 -- i = first, last, 63, 64 and the two around the set's middle, so the
           winning symmetry (recorded: `win`) falls on either side of every tile boundary.
  K        LM's intrinsics; group 12 draws one K per pose.
  groups   cases with one `group` id form one batch; the last group mixes the 13 meshes (and symmetry sets of 1 to 628 members).
Every recorded MSSD / diameter and MSPD lies at least 1e-3 x threshold away from every threshold (asserted; the pose is redrawn
otherwise), so a correct / wrong bit never hinges on rounding."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "bop_toolkit"))
sys.path.insert(0, ROOT)

from bop_toolkit_lib import misc, pose_error, pose_matching  # noqa: E402
from checkerpose_amd.synthetic import LM_OBJ_IDS  # noqa: E402

LM_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
TH_MSSD = np.arange(0.05, 0.51, 0.05)
TH_MSPD = np.arange(5, 51, 5)


def half_turn(axis, through=(0.0, 0.0, 0.0)):
    """4x4 (row-major list) of the half turn about `axis` through the point `through`"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    R = 2.0 * np.outer(a, a) - np.eye(3)
    c = np.asarray(through, dtype=np.float64)
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = c - R @ c
    return [float(v) for v in m.reshape(-1)]


# (model-info dict, max_sym_disc_step)
SETS = [
    ({}, 0.01),
    ({"symmetries_discrete": [half_turn((0, 0, 1), (1.0, -1.5, 0.0))]}, 0.01),
    ({"symmetries_discrete": [half_turn((1, 0, 0)), half_turn((0, 1, 0)), half_turn((0, 0, 1))]}, 0.01),
    ({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, float(np.pi / 63.5)),
    ({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, float(np.pi / 64.5)),
    ({"symmetries_continuous": [{"axis": [0, 2, 1], "offset": [0, 0, 0]}]}, float(np.pi / 65.5)),
    ({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [3.5, -2.0, 1.25]}], "symmetries_discrete": [half_turn((1, 0, 0))]}, 0.01),
    ({"symmetries_continuous": [{"axis": [1, 0, 0], "offset": [0, 0, 0]}], "symmetries_discrete": [half_turn((0, 0, 1))]}, 0.005),
]
SET_SIZES = [1, 2, 4, 63, 64, 65, 628, 1256]
RECORD_T = (2, 5, 6)


def rodrigues(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def k_indices(S):
    return sorted({k for k in (0, S - 1, 63, 64, S // 2 - 1, S // 2) if 0 <= k < S})


def correct_bits(err, ths):
    bits = []
    for th in ths:
        m = pose_matching.match_poses([{"est_id": 0, "score": 1.0, "errors": {0: [err]}}], [th])
        bits.append(len(m) == 1 and m[0]["gt_id"] == 0)
    return np.array(bits, dtype=bool)


def clear(err, ths):
    return all(abs(err - th) >= 1e-3 * th for th in ths)


def main():
    rng = np.random.default_rng(20240607)
    table = np.load(os.path.join(ROOT, "checkerpose_amd", "data", "fps_lm_15x4096.npy")).reshape(-1, 3).astype(np.float64)
    meshes = [(0, n) for n in (1, 3, 63, 65, 1000, 4095, 4096, 9001, 20480)]
    mixed0 = len(meshes)
    meshes += [((o - 1) * 4096, 4096 - 37 * k) for k, o in enumerate(LM_OBJ_IDS)]
    diam = []
    for s, n in meshes:
        diam.append(misc.calc_pts_diameter(table[s:s + n]) if n > 1 else 1.0)      # (one point: any positive number)
        print("mesh [%d, +%d): diameter %.6f" % (s, n, diam[-1]), flush=True)
    sets = [misc.get_symmetry_transformations(info, step) for info, step in SETS]
    assert [len(s) for s in sets] == SET_SIZES, [len(s) for s in sets]
    ks = lambda si: ["k%d" % k for k in k_indices(SET_SIZES[si])]   # noqa: E731
    # (group, mesh, set, kind, per-pose K)
    plan = [(0, 6, 0, m, False) for m in (0, 0.2, 1, 5, 30, "ident")]
    plan += [(1, 0, 1, m, False) for m in [1, 5] + ks(1)]
    plan += [(2, 1, 1, m, False) for m in [0, 5] + ks(1)]
    plan += [(3, 2, 1, m, False) for m in [0, 5] + ks(1)]
    plan += [(4, 3, 1, m, False) for m in [0, 30] + ks(1)]
    plan += [(5, 5, 2, m, False) for m in [0, 5] + ks(2)]
    plan += [(6, 4, 3, m, False) for m in [1] + ks(3)]
    plan += [(7, 6, 4, m, False) for m in [0.2] + ks(4)]
    plan += [(8, 7, 5, m, False) for m in [30] + ks(5)]
    plan += [(9, 6, 6, m, False) for m in [5, "ident"] + ks(6)]
    plan += [(10, 8, 6, m, False) for m in [1, "k64"]]
    plan += [(11, 4, 7, m, False) for m in [0.2] + ks(7)]
    plan += [(12, 6, 2, m, True) for m in (0, 0.2, 1, 5, 30, "k3")]
    mixed_sets = [0, 1, 2, 0, 3, 0, 1, 6, 5, 0, 2, 0, 4]
    mixed_kinds = [0.2, 1, 5, 30, "k31", 0, 1, "k313", 30, 0.2, "ident", 5, "k63"]
    plan += [(13, mixed0 + k, mixed_sets[k], mixed_kinds[k], False) for k in range(13)]
    names = ("group", "mesh", "set", "tag", "k", "R_gt", "t_gt", "R_est", "t_est", "K", "mssd", "mspd", "proj", "win", "bits_mssd", "bits_mspd")
    rec = {k: [] for k in names}
    for g, mi, si, kind, own_k in plan:
        s, n = meshes[mi]
        pts = table[s:s + n]
        syms = sets[si]
        for attempt in range(200):
            R_gt = rodrigues(rng.normal(size=3), rng.uniform(0, 180))
            t_gt = np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(400, 1500)])
            K = LM_K.copy()
            if own_k:
                K[0, 0] *= rng.uniform(0.8, 1.3)
                K[1, 1] *= rng.uniform(0.8, 1.3)
                K[0, 2] += rng.uniform(-30, 30)
                K[1, 2] += rng.uniform(-30, 30)
            kidx = -1
            if kind == "ident":
                R_est, t_est = np.eye(3), np.zeros(3)
            elif kind == 0:
                R_est, t_est = R_gt.copy(), t_gt.copy()
            else:
                R0, t0, m = R_gt, t_gt, kind
                if isinstance(kind, str):
                    kidx, m = int(kind[1:]), 0.2
                    R0 = R_gt @ syms[kidx]["R"]
                    t0 = R_gt @ syms[kidx]["t"].reshape(3) + t_gt
                d = rng.normal(size=3)
                R_est, t_est = rodrigues(rng.normal(size=3), m) @ R0, t0 + m * d / np.linalg.norm(d)
            args = (R_est, t_est.reshape(3, 1), R_gt, t_gt.reshape(3, 1))
            e_mssd = float(pose_error.mssd(*args, pts, syms))
            e_mspd = float(pose_error.mspd(*args, K, pts, syms))
            e_proj = float(pose_error.proj(*args, K, pts))
            if clear(e_mssd / diam[mi], TH_MSSD) and clear(e_mspd, TH_MSPD):
                break
        else:
            raise AssertionError("no pose clear of the thresholds for %r" % ((g, mi, si, kind),))
        assert clear(e_mssd / diam[mi], TH_MSSD) and clear(e_mspd, TH_MSPD)
        win = -1
        if kidx >= 0:
            win = int(np.argmin([pose_error.mssd(*args, pts, [sy]) for sy in syms]))
        if kind == 0 and si in (0, 1, 2):
            assert e_mssd == 0.0 and e_mspd == 0.0 and e_proj == 0.0
        vals = (g, mi, si, str(kind), kidx, R_gt, t_gt, R_est, t_est, K, e_mssd, e_mspd, e_proj, win,
                correct_bits(e_mssd / diam[mi], TH_MSSD), correct_bits((640.0 / 640.0) * e_mspd, TH_MSPD))
        for k, v in zip(names, vals):
            rec[k].append(v)
        print("group %2d mesh %2d (V=%5d) set %d (S=%4d) %-5s mssd %.6f mspd %.6f proj %.6f win %d" % (g, mi, n, si, len(syms), kind, e_mssd, e_mspd, e_proj, win), flush=True)
    out = {k: np.array(v) for k, v in rec.items()}
    out["mesh_start"] = np.array([m[0] for m in meshes], dtype=np.int64)
    out["mesh_count"] = np.array([m[1] for m in meshes], dtype=np.int64)
    out["mesh_diameter"] = np.array(diam, dtype=np.float64)
    out["set_info"] = np.array([json.dumps(info) for info, _ in SETS])
    out["set_step"] = np.array([step for _, step in SETS], dtype=np.float64)
    out["set_size"] = np.array(SET_SIZES, dtype=np.int64)
    for si in RECORD_T:
        out["set_T_%d" % si] = np.array([np.concatenate([t["R"].reshape(9), t["t"].reshape(3)]) for t in sets[si]], dtype=np.float64)
    out["th_mssd"], out["th_mspd"] = TH_MSSD, TH_MSPD
    np.savez_compressed(os.path.join(HERE, "bop_error.npz"), **out)
    print("wrote bop_error.npz: %d cases, %d meshes, %d sets" % (len(plan), len(meshes), len(SETS)))


if __name__ == "__main__":
    main()
