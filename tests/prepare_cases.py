"""The clouds of tests/golden/prepare.npz and numpy restatements of the device rules (checkerpose_amd/csrc/prepare.hip), shared by the
fixture's maker (tests/golden/make_golden_prepare.py) and by tests/test_prepare.py / tests/test_gpu_prepare.py.

Clouds are regenerated from seeds (only ids, diameters and the tiny hand-made clouds are stored); the fixture records a CRC of each
cloud's bytes, so a generator that drifts is reported as such and not as a wrong id."""
import os
import zlib

import numpy as np

from tests.vsd_stages import _icosphere

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prepare.npz")


def _rand(seed, V, scale=100.0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (V, 3)) * np.array([scale, 0.6 * scale, 0.3 * scale])


def _cube():
    return np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)]) * 40.0


def _grid():
    g = np.stack(np.meshgrid(np.arange(17.0), np.arange(17.0), np.arange(3.0), indexing="ij"), -1).reshape(-1, 3)
    return g[np.random.default_rng(7).permutation(g.shape[0])]


def _dup():
    base = _rand(11, 300)
    return np.concatenate([base, base, base], 0)[np.random.default_rng(12).permutation(900)]


def _ico_noise():
    v, _ = _icosphere(5, 50.0)                         # 20 480 triangles, 10 242 vertices
    return v + np.random.default_rng(13).normal(size=v.shape) * 0.05


# name -> (cloud maker, npoint).  V: 1, 2, around the wave (63 / 64 / 65) and the workgroup (1023 / 1024 / 1025), one cloud of many
# slices; npoint: 1, 2, 512, 4096, a permutation (npoint = V), npoint > V; exact ties (cube, integer grid, duplicated vertices);
# fp32-valued and genuine fp64 coordinates away from the origin.  The ulp cases are stored in the fixture itself (`ulp_clouds`).
GENERATED = {
    "v1_n1": (lambda: np.array([[3.5, -2.0, 7.25]]), 1),
    "v1_n3": (lambda: np.array([[3.5, -2.0, 7.25]]), 3),
    "v2_n2": (lambda: _rand(1, 2), 2),
    "v63_n64": (lambda: _rand(2, 63), 64),
    "v64_n64": (lambda: _rand(3, 64), 64),
    "v65_n2": (lambda: _rand(4, 65), 2),
    "v1023_n512": (lambda: _rand(5, 1023), 512),
    "v1024_n512": (lambda: _rand(6, 1024), 512),
    "v1025_n1": (lambda: _rand(8, 1025), 1),
    "v70001_n512": (lambda: _rand(9, 70001), 512),
    "v4096_n4096": (lambda: _rand(10, 4096), 4096),
    "cube_n8": (_cube, 8),
    "grid17x17x3_n512": (_grid, 512),
    "dup900_n512": (_dup, 512),
    "f32_n512": (lambda: _rand(14, 2000).astype(np.float32).astype(np.float64), 512),
    "f64_off1e3_n512": (lambda: _rand(15, 2000, 30.0) + 1e3, 512),
    "ico20480_n4096": (_ico_noise, 4096),
}
N_ULP = 6                                              # six-point clouds on which the squares and the roots disagree (`ulp_clouds`)

_CLOUDS = {}


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.float64).tobytes())


def cloud(name, golden=None):
    """the float64 (V,3) cloud of a case (cached; read-only)"""
    if name not in _CLOUDS:
        if name.startswith("ulp"):
            a = np.array(golden["ulp_clouds"][int(name[3:])], dtype=np.float64)
        else:
            a = np.ascontiguousarray(GENERATED[name][0](), dtype=np.float64)
        a.setflags(write=False)
        _CLOUDS[name] = a
    return _CLOUDS[name]


def names():
    return list(GENERATED) + ["ulp%d" % k for k in range(N_ULP)]


def npoint_of(name):
    return 6 if name.startswith("ulp") else GENERATED[name][1]


def fps_rule(xyz, npoint, slices=1, squares=False, last=False):
    """The device rule of cp_fps restated: the box centre as the start, roots of unfused sums of squares, `if d < dist`, and the argmax as
    the kernel takes it -- per slice the first index of the slice's largest value, then across the slices' partials the larger value
    and on equal values the smaller index.  Two MUTATIONS for the tests: squares = compare the sums of squares instead of their roots;
    last = the LAST index of the largest value.  -> (ids (npoint,) int64, xyz (npoint,3))"""
    p = np.asarray(xyz, dtype=np.float64)
    V = p.shape[0]
    hi, lo = p.max(axis=0), p.min(axis=0)
    far = (hi + lo) / 2
    dx, dy, dz = hi - lo
    dist = np.full(V, (1.0 * np.sqrt((dx * dx + dy * dy) + dz * dz)) * 10)
    if squares:
        dist = dist * dist
    length = (V + slices - 1) // slices
    ids = np.zeros(npoint, dtype=np.int64)
    with np.errstate(over="ignore"):
        for s in range(npoint):
            ex, ey, ez = p[:, 0] - far[0], p[:, 1] - far[1], p[:, 2] - far[2]
            d = (ex * ex + ey * ey) + ez * ez
            if not squares:
                d = np.sqrt(d)
            dist = np.where(d < dist, d, dist)
            bv, bi = -1.0, -1
            for i0 in range(0, V, length):
                part = dist[i0:i0 + length]
                k = (part.shape[0] - 1 - int(np.argmax(part[::-1]))) if last else int(np.argmax(part))
                if part[k] > bv or (last and part[k] == bv):
                    bv, bi = part[k], i0 + k
            ids[s] = bi
            far = p[bi]
    return ids, p[ids]


def diameter_rule(xyz, tile=1024):
    """cp_pts_diameter restated: the max over the upper triangle of tile pairs of ((dx*dx + dy*dy) + dz*dz), one root at the end"""
    p = np.asarray(xyz, dtype=np.float64)
    best = 0.0
    for i0 in range(0, p.shape[0], tile):
        for j0 in range(i0, p.shape[0], tile):
            d = p[i0:i0 + tile, None, :] - p[None, j0:j0 + tile, :]
            best = max(best, float(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).max()))
    return float(np.sqrt(best))
