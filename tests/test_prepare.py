"""Row N9 (object preparation: farthest-point keypoints, exact diameter), host side.  tests/golden/prepare.npz holds what the REFERENCE's
own get_fps_points.farthest_point_sample_init_center and bop_toolkit_lib.misc.calc_pts_diameter returned
(tests/golden/make_golden_prepare.py); the numpy restatements of the device rules (tests/prepare_cases.py) reproduce every recorded id
and diameter EXACTLY, and two mutations of the rule are caught:
  squares-only (compare sums of squares, not their roots): caught by every one of the `ulp*` cases (that is how they were chosen);
  last-index tie-break: caught by the cases with exact ties -- cube_n8, grid17x17x3_n512, dup900_n512 and the npoint > V case
  v63_n64 (index 0 repeats once every distance is 0; the mutation repeats V - 1).
cp_fps' and cp_pts_diameter's argument checks return before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, metric, prepare, synthetic
from tests import prepare_cases as P


@pytest.fixture(scope="module")
def g():
    return np.load(P.GOLDEN)


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


def test_fixture_holds_every_case_and_the_generator_has_not_drifted(g):
    assert len(P.names()) == 23 and P.N_ULP >= 4
    for name in P.names():
        pts = P.cloud(name, g)
        assert int(g["crc__" + name]) == P.crc(pts), name
        ids = g["ids__" + name]
        assert ids.dtype == np.int32 and ids.shape == (P.npoint_of(name),) and ids.min() >= 0 and ids.max() < pts.shape[0]
    assert sorted(g["ids__v4096_n4096"].tolist()) == list(range(4096))                   # npoint = V: a permutation
    assert sorted(g["ids__v64_n64"].tolist()) == list(range(64))
    assert g["ids__v63_n64"][-1] == 0 and g["ids__v1_n3"].tolist() == [0, 0, 0]          # npoint > V: index 0 repeats
    assert g["ulp_clouds"].shape == (P.N_ULP, 6, 3)


@pytest.mark.parametrize("name", P.names())
def test_rule_restatement_reproduces_every_recorded_id(g, name):
    pts, n = P.cloud(name, g), P.npoint_of(name)
    ids, xyz = P.fps_rule(pts, n)
    assert np.array_equal(ids, g["ids__" + name]), name
    assert np.array_equal(xyz, pts[g["ids__" + name]])
    if pts.shape[0] <= 4096:                                                             # the slices' partials change nothing
        for slices in (2, 3, 7, 256):
            assert np.array_equal(P.fps_rule(pts, n, slices=slices)[0], ids), (name, slices)


@pytest.mark.parametrize("name", P.names())
def test_diameter_restatements_reproduce_the_reference_exactly(g, name):
    pts = P.cloud(name, g)
    ref = float(g["diam__" + name])
    if pts.shape[0] <= 12000:
        assert P.diameter_rule(pts) == ref, name
    assert metric.calc_pts_diameter(pts) == ref, name                                    # the package's host function (pruned all-pairs)


def test_squares_only_mutation_is_caught_by_every_ulp_case(g):
    for k in range(P.N_ULP):
        pts = P.cloud("ulp%d" % k, g)
        assert not np.array_equal(P.fps_rule(pts, 6, squares=True)[0], g["ids__ulp%d" % k]), k


def test_last_index_mutation_is_caught_by_the_tie_cases(g):
    for name in ("cube_n8", "grid17x17x3_n512", "dup900_n512", "v63_n64"):
        pts = P.cloud(name, g)
        assert not np.array_equal(P.fps_rule(pts, P.npoint_of(name), last=True)[0], g["ids__" + name]), name


def test_model_info_and_normalisation_against_direct_numpy(g):
    pts = P.cloud("f64_off1e3_n512", g)
    info = prepare.model_info(pts, 12.5)
    assert list(info) == ["min_x", "min_y", "min_z", "size_x", "size_y", "size_z", "diameter"]
    lo, hi = pts.min(0), pts.max(0)
    assert [info["min_x"], info["min_y"], info["min_z"]] == lo.tolist()
    assert [info["size_x"], info["size_y"], info["size_z"]] == (hi - lo).tolist() and info["diameter"] == 12.5
    assert all(type(v) is float for v in info.values())
    xyz = pts[g["ids__f64_off1e3_n512"]]
    normed, centroid, rng = prepare.normalize_p3d(xyz[:128])
    c = xyz[:128].mean(axis=0)
    m = np.sqrt(((xyz[:128] - c) ** 2).sum(axis=1)).max()
    assert np.array_equal(centroid, c) and rng == m
    assert normed.dtype == torch.float32 and tuple(normed.shape) == (1, 3, 128)
    assert torch.equal(normed, torch.as_tensor((xyz[:128] - c) / m, dtype=torch.float32).t()[None])
    assert torch.equal(normed, synthetic.p3d_from(xyz, 128))                             # what the tests' networks are built from
    assert np.array_equal(xyz[:128], pts[g["ids__f64_off1e3_n512"][:128]])               # (normalize_p3d leaves its input alone)


def test_python_layer_refuses_bad_clouds_without_a_device():
    with pytest.raises(ValueError):
        prepare.pack_clouds([np.zeros((0, 3))])
    with pytest.raises(ValueError):
        prepare.pack_clouds([np.zeros((4, 2))])
    with pytest.raises(ValueError):
        prepare.pack_clouds([])
    for bad in (np.nan, np.inf, -np.inf):
        a = np.zeros((5, 3))
        a[3, 1] = bad
        with pytest.raises(ValueError):
            prepare.pack_clouds([np.ones((2, 3)), a])
    table, off = prepare.pack_clouds([np.ones((2, 3), dtype=np.float32), torch.zeros(5, 3)])
    assert table.dtype == np.float64 and table.shape == (7, 3) and off.dtype == np.int32 and off.tolist() == [0, 2, 7]
    with pytest.raises(RuntimeError):
        prepare.fps_batch([np.ones((2, 3))], 2, device="cpu")                            # no CPU fallback
    with pytest.raises(ValueError):
        prepare.prepare_objects([np.ones((2, 3))], npoint_log2=3, num_p3d=9, device="cpu")


def _off(*v):
    return (C.c_int32 * len(v))(*v)


def test_cp_fps_rejects_bad_arguments_before_any_launch(lib):
    p = C.c_void_p(4096)                                    # fake, aligned; never dereferenced: every call returns before a launch
    ok = _off(0, 5, 9)
    call = lib.cp_fps
    for k in (1, 2, 3, 7, 8, 9):                            # null pts / offsets / host offsets / ids / xyz / scratch
        args = [None, p, p, ok, 2, 4, 0, p, p, p]
        args[k] = None
        assert call(*args) == -1, k
    assert call(None, p, p, ok, 0, 4, 0, p, p, p) == -1                        # no cloud
    assert call(None, p, p, ok, 2, 0, 0, p, p, p) == -1                        # npoint < 1
    assert call(None, p, p, ok, 2, -3, 0, p, p, p) == -1
    assert call(None, p, p, ok, 2, 4, -1, p, p, p) == -1                       # slices outside 0 .. 256
    assert call(None, p, p, ok, 2, 4, 257, p, p, p) == -1
    assert call(None, p, p, _off(0, 5, 5), 2, 4, 0, p, p, p) == -1             # an empty cloud
    assert call(None, p, p, _off(0, 5, 3), 2, 4, 0, p, p, p) == -1             # offsets that fall
    assert call(None, p, p, _off(1, 5, 9), 2, 4, 0, p, p, p) == -1             # a table that does not start at row 0
    assert call(None, C.c_void_p(4096 + 4), p, ok, 2, 4, 0, p, p, p) == -3     # misaligned fp64 table
    assert call(None, p, C.c_void_p(4096 + 2), ok, 2, 4, 0, p, p, p) == -3     # misaligned offsets
    assert call(None, p, p, ok, 2, 4, 0, p, C.c_void_p(4096 + 4), p) == -3     # misaligned xyz
    assert call(None, p, p, ok, 2, 4, 0, p, p, C.c_void_p(4096 + 4)) == -3     # misaligned scratch
    big = _off(*range(0, 65537))
    assert call(None, p, p, big, 65536, 4, 0, p, p, p) == -4                   # more clouds than a grid has rows
    q = lib.cp_fps_scratch_bytes
    assert q(0, 9, 5, 0) == 0 and q(2, 0, 5, 0) == 0 and q(2, 9, 0, 0) == 0 and q(2, 9, 10, 0) == 0 and q(2, 9, 5, 257) == 0
    for M, sumV, Vmax in ((1, 1, 1), (1, 5000, 5000), (21, 21 * 250000, 250000), (3, 70000, 65000)):
        for slices in (0, 1, 7, 256):
            n = q(M, sumV, Vmax, slices)
            G = slices if slices else (n - 8 * (sumV + 4 * M)) // (24 * M)
            assert n == 8 * (sumV + 4 * M) + 24 * M * G and 1 <= G <= 256, (M, sumV, Vmax, slices, n)   # dist, head, 2 x (value, index) per slice
    assert lib.cp_version() >= 210


def test_cp_pts_diameter_rejects_bad_arguments_before_any_launch(lib):
    p = C.c_void_p(4096)
    ok = _off(0, 5, 9)
    call = lib.cp_pts_diameter
    for k in (1, 2, 3, 5, 6):                               # null pts / offsets / host offsets / diameters / scratch
        args = [None, p, p, ok, 2, p, p]
        args[k] = None
        assert call(*args) == -1, k
    assert call(None, p, p, ok, 0, p, p) == -1
    assert call(None, p, p, _off(0, 0, 9), 2, p, p) == -1                      # an empty cloud
    assert call(None, p, p, _off(0, 5, 4), 2, p, p) == -1                      # offsets that fall
    assert call(None, p, p, _off(2, 5, 9), 2, p, p) == -1
    assert call(None, C.c_void_p(4096 + 4), p, ok, 2, p, p) == -3
    assert call(None, p, p, ok, 2, C.c_void_p(4096 + 4), p) == -3
    assert call(None, p, p, ok, 2, p, C.c_void_p(4096 + 4)) == -3
    assert call(None, p, C.c_void_p(4096 + 2), ok, 2, p, p) == -3
    assert call(None, p, p, _off(0, 5792 * 1024 + 1), 1, p, p) == -4           # 2^24 tile pairs or more
    q = lib.cp_pts_diameter_scratch_bytes
    assert q(0, 5) == 0 and q(1, 0) == 0 and q(1, 5792 * 1024 + 1) == 0
    assert q(1, 1) == 8 and q(1, 1024) == 8 and q(1, 1025) == 24 and q(3, 100000) == 3 * 8 * (98 * 99 // 2)
