"""Row N9 on the device: cp_fps / cp_pts_diameter and checkerpose_amd.prepare against what the reference's own functions returned
(tests/golden/prepare.npz, tests/golden/make_golden_prepare.py).  Nothing here has a tolerance: ids are EQUAL, coordinates and
diameters are the recorded bits, and the outputs do not depend on the call, the batch or the number of slices."""
import pickle

import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, metric, prepare, synthetic
from tests import prepare_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g():
    return np.load(P.GOLDEN)


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def test_fps_ids_equal_and_xyz_bitwise_on_every_case(g):
    for name in P.names():
        pts, n = P.cloud(name, g), P.npoint_of(name)
        ids, xyz = prepare.fps_batch([pts], n, DEV)
        assert ids.dtype == torch.int32 and xyz.dtype == torch.float64 and ids.is_cuda and tuple(ids.shape) == (1, n) and tuple(xyz.shape) == (1, n, 3)
        ref = g["ids__" + name]
        got = ids[0].cpu().numpy()
        wrong = np.nonzero(got != ref)[0]
        print("%-18s V=%6d npoint=%5d ids differing: %d" % (name, pts.shape[0], n, wrong.size))
        assert wrong.size == 0, (name, wrong[:5], got[wrong[:5]], ref[wrong[:5]])
        assert np.array_equal(_bits(xyz[0]), pts[ref].view(np.int64)), name
    ids, xyz = prepare.farthest_point_sample_init_center(P.cloud("cube_n8", g), 8, DEV)   # the reference's name and return
    assert type(ids) is list and type(ids[0]) is int and ids == g["ids__cube_n8"].tolist()
    assert type(xyz) is np.ndarray and xyz.dtype == np.float64 and np.array_equal(xyz, P.cloud("cube_n8", g)[ids])


def test_diameters_are_the_reference_bits_and_the_host_function_s(g):
    clouds = [P.cloud(n, g) for n in P.names()]
    out = prepare.pts_diameters(clouds, DEV)                                              # one call, 23 clouds of 1 .. 70 001 points
    assert out.dtype == torch.float64 and out.is_cuda and tuple(out.shape) == (len(clouds),)
    got = out.cpu().numpy()
    for k, name in enumerate(P.names()):
        ref = float(g["diam__" + name])
        print("%-18s got %.17g ref %.17g" % (name, got[k], ref))
        assert got[k] == ref, (name, got[k], ref)
        assert got[k] == metric.calc_pts_diameter(clouds[k]), name
    assert np.array_equal(_bits(prepare.pts_diameters(clouds, DEV)), _bits(out))          # two calls
    for name in ("v1_n1", "v1025_n1", "ico20480_n4096", "ulp0"):                          # a cloud alone
        assert prepare.calc_pts_diameter(P.cloud(name, g), DEV) == float(g["diam__" + name]), name
    f32 = [P.cloud(n, g).astype(np.float32) for n in ("v1023_n512", "f32_n512", "cube_n8")]
    ms = metric.MeshSet.from_arrays(f32, device=DEV)                                      # MeshSet's diameters on the device == its host ones
    assert np.array_equal(ms.diameters, metric.MeshSet.from_arrays(f32).diameters)


def test_fps_is_bitwise_the_same_across_calls_batches_slices_and_npoint(g):
    names = ["v1023_n512", "grid17x17x3_n512", "v70001_n512", "dup900_n512", "v1_n1", "ulp3"]
    clouds = [P.cloud(n, g) for n in names]
    ids, xyz = prepare.fps_batch(clouds, 512, DEV)                                        # a batch of differing sizes
    ids2, xyz2 = prepare.fps_batch(clouds, 512, DEV)
    assert torch.equal(ids, ids2) and np.array_equal(_bits(xyz), _bits(xyz2))             # two calls
    for k, name in enumerate(names):
        one_i, one_x = prepare.fps_batch([clouds[k]], 512, DEV)                           # alone
        assert torch.equal(one_i[0], ids[k]) and np.array_equal(_bits(one_x[0]), _bits(xyz[k])), name
        if P.npoint_of(name) == 512:
            assert np.array_equal(ids[k].cpu().numpy(), g["ids__" + name]), name
    for slices in (1, 3, 64, 256):                                                        # the automatic choice here is 137
        s_i, s_x = prepare.fps_batch(clouds, 512, DEV, _slices=slices)
        assert torch.equal(s_i, ids) and np.array_equal(_bits(s_x), _bits(xyz)), slices
    ico = P.cloud("ico20480_n4096", g)
    short, _ = prepare.fps_batch([ico], 512, DEV)                                         # a prefix: npoint = 512 is the head of npoint = 4096
    assert np.array_equal(short[0].cpu().numpy(), g["ids__ico20480_n4096"][:512])


def test_prepare_object_end_to_end(g, tmp_path):
    pts = P.cloud("ico20480_n4096", g)
    from tests.vsd_stages import _icosphere
    _, faces = _icosphere(5, 50.0)
    obj = prepare.prepare_object(pts, npoint_log2=12, num_p3d=512, faces=faces, device=DEV)
    ref_ids = g["ids__ico20480_n4096"]
    assert obj.fps["npoint"] == 4096 and obj.fps["id"] == ref_ids.tolist() and np.array_equal(obj.fps["xyz"], pts[ref_ids])
    assert obj.diameter == float(g["diam__ico20480_n4096"]) == obj.model_info["diameter"]
    assert obj.model_info == prepare.model_info(pts, obj.diameter)
    obj.save_fps(str(tmp_path / "obj_000001.pkl"))
    with open(str(tmp_path / "obj_000001.pkl"), "rb") as f:
        back = pickle.load(f)
    assert sorted(back) == ["id", "npoint", "xyz"] and back["npoint"] == 4096 and back["id"] == obj.fps["id"] and np.array_equal(back["xyz"], obj.fps["xyz"])
    assert tuple(obj.p3d_xyz.shape) == (512, 3) and np.array_equal(obj.p3d_xyz, pts[ref_ids[:512]])
    assert obj.p3d_normed.dtype == torch.float32 and torch.equal(obj.p3d_normed, synthetic.p3d_from(obj.fps["xyz"], 512))
    assert np.array_equal(obj.centroid, obj.p3d_xyz.mean(axis=0)) and obj.range > 0
    ms = obj.meshset
    assert len(ms) == 1 and ms.diameters[0] == obj.diameter and ms.faces is not None and int(ms.sizes[0]) == pts.shape[0]
    two = prepare.prepare_objects([pts, P.cloud("v4096_n4096", g)], npoint_log2=9, device=DEV)   # one cp_fps + one cp_pts_diameter call
    assert two[0].fps["id"] == ref_ids[:512].tolist() and two[0].diameter == obj.diameter
    assert two[1].diameter == float(g["diam__v4096_n4096"]) and two[1].fps["npoint"] == 512 and tuple(two[1].p3d_normed.shape) == (1, 3, 512)


def test_launch_counts(g):
    lib = _abi.load()
    pts = P.cloud("v1025_n1", g)
    lib.cp_kernel_log_begin()
    prepare.fps_batch([pts, pts], 7, DEV)
    assert lib.cp_kernel_log().decode() == "fps_bbox_kernel + fps_step_kernel x8"         # one launch per sample + the collecting one
    lib.cp_kernel_log_begin()
    prepare.pts_diameters([pts, pts], DEV)
    assert lib.cp_kernel_log().decode() == "pts_diameter_kernel + pts_diameter_finish_kernel"
    lib.cp_kernel_log_begin()
    prepare.prepare_objects([pts, pts], npoint_log2=2, device=DEV)
    assert lib.cp_kernel_log().decode() == "fps_bbox_kernel + fps_step_kernel x5 + pts_diameter_kernel + pts_diameter_finish_kernel"
    assert lib.cp_last_kernel().decode() == "pts_diameter_finish_kernel" and lib.cp_version() >= 210
