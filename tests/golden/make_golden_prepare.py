"""Fixture of the object-preparation kernels (cp_fps, cp_pts_diameter): tests/golden/prepare.npz.

Runs ONLY where the reference tree is (CHECKERPOSE_REFERENCE, default /root/reference; nothing of it travels, only the recorded
results).  The reference's own functions make every recorded value:
  checkerpose/preprocess_data/get_fps_points.py: farthest_point_sample_init_center -- imported with stub `plyfile` / `mmcv` modules
      (the script's PLY reading and dumping sit behind __main__ and are not run);
  bop_toolkit_lib.misc.calc_pts_diameter.
Per case of tests/prepare_cases.py: `ids__<name>` (the reference's fps_ids), `diam__<name>`, `crc__<name>` (CRC-32 of the cloud's
float64 bytes: the clouds are regenerated from seeds, not stored) and an assertion that fps_xyz is the cloud at those ids.
`ulp_clouds` (N_ULP, 6, 3): six points (+-a, +-b, 0) / (+-b, +-a, 0) with every coordinate moved by 0 - 3 ulp, found by a seeded
search for draws on which comparing the SUMS OF SQUARES picks other ids than the reference's comparison of the roots (two different
sums can round to one root, and then the lower index wins); the maker asserts the disagreement for every cloud it keeps and prints
the share of such draws.

  python tests/golden/make_golden_prepare.py"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("CHECKERPOSE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "bop_toolkit"))
sys.path.insert(0, os.path.join(REF, "checkerpose", "preprocess_data"))
sys.path.insert(0, ROOT)
for stub in ("plyfile", "mmcv"):
    if stub not in sys.modules:
        mod = types.ModuleType(stub)
        mod.PlyData = None
        sys.modules[stub] = mod

import get_fps_points as G  # noqa: E402
from bop_toolkit_lib import misc  # noqa: E402
from tests import prepare_cases as C  # noqa: E402


def ulp_search(want, draws=20000):
    rng = np.random.default_rng(2024)
    found, differ = [], 0
    for _ in range(draws):
        a, b = rng.uniform(1.0, 100.0, 2)
        base = np.array([[a, b, 0], [-a, -b, 0], [b, a, 0], [-b, -a, 0], [a, -b, 0], [-b, a, 0]], dtype=np.float64)
        pts = base.copy()
        k = rng.integers(0, 4, size=(6, 2))
        for _step in range(3):
            pts[:, :2] = np.where(k > _step, np.nextafter(pts[:, :2], np.inf), pts[:, :2])
        ref_ids, _ = G.farthest_point_sample_init_center(pts, 6)
        sq_ids, _ = C.fps_rule(pts, 6, squares=True)
        if list(ref_ids) != list(sq_ids):
            differ += 1
            if len(found) < want:
                found.append(pts)
    print("ulp search: the squares-only rule picks other ids in %d of %d draws" % (differ, draws))
    assert len(found) == want
    return np.stack(found)


def main():
    out = {"ulp_clouds": ulp_search(C.N_ULP)}
    for name in C.names():
        pts = np.array(C.cloud(name, out))
        npoint = C.npoint_of(name)
        ids, xyz = G.farthest_point_sample_init_center(pts, npoint)
        ids = np.asarray(ids, dtype=np.int64)
        assert xyz.dtype == np.float64 and np.array_equal(xyz, pts[ids])
        if name.startswith("ulp"):
            assert list(ids) != list(C.fps_rule(pts, npoint, squares=True)[0]), name
        out["ids__" + name] = ids.astype(np.int32)
        out["diam__" + name] = np.float64(misc.calc_pts_diameter(pts))
        out["crc__" + name] = np.uint32(C.crc(pts))
        print("%-18s V=%6d npoint=%5d distinct ids=%5d diameter=%.17g" % (name, pts.shape[0], npoint, np.unique(ids).size, out["diam__" + name]),
              flush=True)
    np.savez_compressed(C.GOLDEN, **out)
    print("wrote", C.GOLDEN, os.path.getsize(C.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
