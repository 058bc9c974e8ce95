"""checkerpose_amd/scene.py without a device: the shape helpers are plain tensor plumbing (they never ask for a GPU), so each branch
is exercised on CPU tensors and numpy arrays; _abi.marshal, the pure half of _abi.call, without loading the library."""
import ctypes as C

import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, metric, scene

CPU = torch.device("cpu")
TET = np.array([[0.0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 0, 10]])
TET_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def test_the_containers_keep_their_public_home_in_metric():
    assert metric.MeshSet is scene.MeshSet and metric.SymmetrySet is scene.SymmetrySet
    assert metric.symmetry_transformations is scene.symmetry_transformations and metric.calc_pts_diameter is scene.calc_pts_diameter


def test_device_checks_carry_the_callers_name():
    with pytest.raises(RuntimeError, match=r"checkerpose_amd\.vis: CUDA/HIP tensors required \(no CPU fallback\)"):
        scene.require_cuda("vis", torch.zeros(2))
    with pytest.raises(RuntimeError, match=r"checkerpose_amd\.metric: CUDA/HIP tensors required"):
        scene.require_cuda("metric", np.zeros(2))
    with pytest.raises(RuntimeError, match=r"checkerpose_amd\.coco_eval: CUDA/HIP tensors required"):
        scene.require_cuda("coco_eval", device=CPU)
    with pytest.raises(RuntimeError, match=r"checkerpose_amd\.prepare: a CUDA/HIP device is required \(no CPU fallback\)"):
        scene.cuda_device("prepare", "cpu")
    with pytest.raises(RuntimeError, match=r"checkerpose_amd\.metric: CUDA/HIP tensors required"):
        scene.MeshSet.from_arrays([TET]).on("cpu")
    with pytest.raises(RuntimeError, match=r"checkerpose_amd\.metric: CUDA/HIP tensors required"):
        scene.SymmetrySet.identity(1).on("cpu")


def test_camera():
    K1 = np.array([[500.0, 0, 24], [0, 510, 20], [0, 0, 1]])
    K, stride = scene.camera(K1, 3, CPU)
    assert stride == 0 and K.dtype == torch.float64 and K.tolist() == K1.reshape(9).tolist()
    K, stride = scene.camera(torch.from_numpy(np.stack([K1, 2 * K1, 3 * K1])).float(), 3, CPU)
    assert stride == 9 and K.dtype == torch.float64 and tuple(K.shape) == (3, 9) and K[2].tolist() == (3 * K1).reshape(9).tolist()
    with pytest.raises(ValueError, match=r"cam_K must be \(3,3\) or \(B,3,3\), got \(2, 3, 3\)"):
        scene.camera(np.stack([K1, K1]), 3, CPU)
    with pytest.raises(ValueError, match=r"cam_K must be \(3,3\) or \(I,3,3\)"):
        scene.camera(np.stack([K1, K1]), 3, CPU, "I")


def test_mesh_ids():
    v = np.array([4, 8], dtype=np.int64)            # MeshSet.sizes of a tetrahedron and a cube
    s = np.array([2, 1], dtype=np.int64)            # SymmetrySet.sizes
    assert scene.mesh_ids_on(None, 3, CPU, v[:1]) == (None, [4])
    with pytest.raises(ValueError, match="several meshes need mesh_ids"):
        scene.mesh_ids_on(None, 3, CPU, v)
    ids, (vmax, smax) = scene.mesh_ids_on([0, 0, 0], 3, CPU, v, s)              # host ids: the largest over the meshes USED
    assert ids.dtype == torch.int32 and ids.tolist() == [0, 0, 0] and (vmax, smax) == (4, 2)
    ids, (vmax, smax) = scene.mesh_ids_on(np.array([1, 1, 1]), 3, CPU, v, s)
    assert ids.tolist() == [1, 1, 1] and (vmax, smax) == (8, 1)
    ids, (vmax,) = scene.mesh_ids_on(torch.tensor([0, 0, 0]), 3, CPU, v)          # resident ids stay unread: over ALL meshes
    assert ids.dtype == torch.int32 and ids.tolist() == [0, 0, 0] and vmax == 8
    for bad in ([0, 2, 0], [0, -1, 0]):
        with pytest.raises(ValueError, match=r"mesh_ids must be \(B,\) with values in 0\.\.1"):
            scene.mesh_ids_on(bad, 3, CPU, v)
    with pytest.raises(ValueError, match=r"mesh_ids must be \(B,\) with values in 0\.\.1"):
        scene.mesh_ids_on([0, 1], 3, CPU, v)
    with pytest.raises(ValueError, match=r"mesh_ids must be \(B,\)"):
        scene.mesh_ids_on(torch.tensor([0, 1]), 3, CPU, v)


def test_image_ids_and_the_grouping_share_one_default_rule():
    assert scene.image_ids_on(None, 3, 1, CPU) is None                            # one image: every pose reads it
    img = scene.image_ids_on(None, 3, 3, CPU)
    assert img.dtype == torch.int32 and img.tolist() == [0, 1, 2]                 # I == B: image b for pose b
    with pytest.raises(ValueError, match="2 depth images for 3 poses need image_ids"):
        scene.image_ids_on(None, 3, 2, CPU)
    with pytest.raises(ValueError, match="2 frames for 3 poses need image_ids"):
        scene.group_by_image(None, 3, 2)
    assert scene.image_ids_on([1, 0, 1], 3, 2, CPU).tolist() == [1, 0, 1]
    assert scene.image_ids_on(torch.tensor([1, 0, 5]), 3, 2, CPU).tolist() == [1, 0, 5]       # resident ids stay unread
    for bad in ([0, 2, 0], [0, -1, 0], [0, 1]):
        with pytest.raises(ValueError, match=r"image_ids must be \(B,\) with values in 0\.\.1"):
            scene.image_ids_on(bad, 3, 2, CPU)
        with pytest.raises(ValueError, match=r"image_ids must be \(P,\) with values in 0\.\.1"):
            scene.group_by_image(bad, 3, 2)
    ids, off, order = scene.group_by_image([2, 0, 2, 1, 0], 5, 3)
    assert ids.tolist() == [2, 0, 2, 1, 0] and off.tolist() == [0, 2, 3, 5] and order.tolist() == [1, 4, 3, 0, 2]     # stable
    assert all(a.dtype == np.int32 for a in (ids, off, order))
    ids, off, order = scene.group_by_image(torch.tensor([2, 0, 2, 1, 0]), 5, 3)
    assert off.tolist() == [0, 2, 3, 5] and order.tolist() == [1, 4, 3, 0, 2]
    assert scene.group_by_image(None, 3, 1)[0].tolist() == [0, 0, 0] and scene.group_by_image(None, 3, 3)[2].tolist() == [0, 1, 2]
    d, img, n_img = scene.depth_images(np.ones((5, 6)), None, 3, CPU)
    assert d.dtype == torch.float32 and tuple(d.shape) == (1, 5, 6) and img is None and n_img == 1
    with pytest.raises(ValueError, match=r"depth_test must be \(H,W\) or \(I,H,W\)"):
        scene.depth_images(np.ones((2, 2, 5, 6)), None, 3, CPU)


def test_pose_packing():
    R = torch.arange(27, dtype=torch.float32).reshape(3, 3, 3)
    t31, t3 = torch.arange(9, dtype=torch.float64).reshape(3, 3, 1), np.arange(9.0).reshape(3, 3)
    p = scene.pack_poses(R, t31)
    assert p.dtype == torch.float64 and tuple(p.shape) == (3, 12) and p.is_contiguous()
    assert p[1].tolist() == list(range(9, 18)) + [3.0, 4.0, 5.0]
    assert torch.equal(p, scene.pack_poses(R.numpy(), t3, 3, CPU))                # (B,3) and host arrays with a device to go to
    one = scene.pack_poses(R[0], t31[0])                                          # a lone (3,3) is one pose
    assert tuple(one.shape) == (1, 12) and torch.equal(one[0], p[0])
    with pytest.raises(ValueError, match=r"poses must be R \(B,3,3\) and t \(B,3,1\) / \(B,3\)"):
        scene.pack_poses(R, t31, 2)
    with pytest.raises(ValueError, match="poses must be R"):
        scene.pack_poses(R, t31[:2])
    with pytest.raises(ValueError, match="poses must be R"):
        scene.pack_poses(torch.zeros(3, 4, 3), t31)


def test_frame_size():
    assert scene.frame_size((48, 40)) == (48, 40) and scene.frame_size([48.0, 40]) == (48, 40)
    for bad in ((0, 40), (48, 0), (-48, 40), (48, -1)):
        with pytest.raises(ValueError, match=r"size must be \(width, height\), both positive"):
            scene.frame_size(bad)
    with pytest.raises(TypeError):
        scene.frame_size(None)                     # the callers that accept None refuse it with a text of their own first


def test_kinds():
    assert scene.kinds_mask("adi", metric.KINDS, "empty") == metric.KINDS["adi"]
    assert scene.kinds_mask(("add", "adi"), metric.KINDS, "empty") == metric.KINDS["add"] | metric.KINDS["adi"]
    assert scene.kinds_mask(["cou_bb_proj"], metric.MASK_KINDS, "empty") == 2 and scene.kinds_mask("cus", metric.MASK_KINDS, "empty") == 1
    with pytest.raises(ValueError, match=r"kinds must be among \['mspd', 'mssd', 'proj'\], got 'add'"):           # a dict: sorted
        scene.kinds_mask(("mssd", "add"), metric.BOP_KINDS, "empty")
    with pytest.raises(ValueError, match=r"kinds must be among \['cus', 'cou_bb_proj'\], got 'vsd'"):              # a tuple: in order
        scene.kinds_mask("vsd", metric.MASK_KINDS, "empty")
    with pytest.raises(ValueError, match="ask for this or that"):
        scene.kinds_mask((), metric.KINDS, "ask for this or that")
    assert scene.kinds_mask((), metric.OVERLAP_KINDS, None) == 0                  # where the caller allows an empty request


def test_lighting():
    code, amb, light = scene.lighting("phong", 0.25, (1, 2, 3))
    assert (code, amb, list(light)) == (1, 0.25, [1.0, -2.0, -3.0])               # OpenGL's camera frame -> the poses'
    assert scene.lighting("flat", 1, np.zeros(3))[0] == 0
    for args in (("gouraud", 0.5, (0, 0, 0)), ("flat", float("nan"), (0, 0, 0)), ("flat", 0.5, (0, 0)), ("flat", 0.5, (0, np.inf, 0))):
        with pytest.raises(ValueError):
            scene.lighting(*args)
    ms = scene.MeshSet.from_arrays([TET], faces=[TET_F])
    scene.check_shaded_meshes(ms, "flat", "render_rgb")
    with pytest.raises(ValueError, match="phong shading needs vertex normals"):
        scene.check_shaded_meshes(ms, "phong", "render_rgb")
    with pytest.raises(ValueError, match="vis_poses renders triangles"):
        scene.check_shaded_meshes([TET], "flat", "vis_poses")


def test_meshset_from_arrays():
    col = np.array([[255, 0, 0], [0, 128, 0], [0, 0, 64], [10, 20, 30]], dtype=np.uint8)
    nrm = TET / 10.0 + 0.1
    one = scene.MeshSet.from_arrays(TET, faces=TET_F, colors=col, normals=nrm, diameters=5.0)
    lst = scene.MeshSet.from_arrays([TET], faces=[TET_F], colors=[col], normals=[nrm], diameters=[5.0])
    for k in ("verts", "offsets", "faces", "face_offsets", "colors", "normals"):
        assert torch.equal(getattr(one, k), getattr(lst, k)), k
    assert one.verts.dtype == torch.float32 and one.faces.dtype == torch.int32 and one.offsets.tolist() == [0, 4] and len(one) == 1
    assert one.face_offsets.tolist() == [0, 4] and one.sizes.tolist() == [4] and one.diameters.tolist() == [5.0]
    assert torch.equal(one.colors, torch.from_numpy(col.astype(np.float32) / np.float32(255.0)))     # above 1: divided by 255 in fp32
    assert torch.equal(one.colors, scene.MeshSet.from_arrays([TET], colors=[col.astype(np.float32) / np.float32(255.0)]).colors)
    two = scene.MeshSet.from_arrays([TET, TET + 1.0], colors=[None, col])
    assert two.colors[:4].eq(0.5).all() and torch.equal(two.colors[4:], one.colors) and two.sizes.tolist() == [4, 4]
    assert abs(scene.MeshSet.from_arrays([TET]).diameters[0] - np.sqrt(200.0)) < 1e-12
    bad = TET_F.copy()
    bad[3, 2] = 4                                                                  # == V
    with pytest.raises(ValueError, match=r"a face names a vertex outside 0\.\.3"):
        scene.MeshSet.from_arrays([TET], faces=[bad])
    with pytest.raises(ValueError, match="faces must be"):
        scene.MeshSet.from_arrays([TET], faces=[TET_F.astype(np.float64)])
    with pytest.raises(ValueError, match="need one face array per mesh"):
        scene.MeshSet.from_arrays([TET, TET], faces=[TET_F])
    with pytest.raises(ValueError, match="need one normal array per mesh"):
        scene.MeshSet.from_arrays([TET, TET], normals=[nrm, None])
    with pytest.raises(ValueError, match="normals must be"):
        scene.MeshSet.from_arrays([TET], normals=[nrm[:3]])
    with pytest.raises(ValueError, match="colors must be"):
        scene.MeshSet.from_arrays([TET], colors=[col[:3]])
    with pytest.raises(ValueError, match="every mesh must be a non-empty"):
        scene.MeshSet.from_arrays([TET[:, :2]])
    with pytest.raises(ValueError, match="MeshSet needs at least one mesh"):
        scene.MeshSet.from_arrays([])
    assert scene.as_meshset(one) is one and scene.as_meshset(TET) is scene.as_meshset(TET) and len(scene.as_meshset([TET, TET])) == 2
    assert len(scene.as_symmetries(None, 2)) == 2 and scene.as_symmetries(None, 2) is scene.as_symmetries(None, 2)
    with pytest.raises(ValueError, match="1 symmetry sets for 2 meshes"):
        scene.as_symmetries(scene.SymmetrySet.identity(1), 2)


def test_abi_call_marshals_without_the_library():
    t = torch.arange(4, dtype=torch.int32)
    arr, ptr = (C.c_double * 3)(1.0, 2.0, 3.0), C.c_void_p(64)
    out = _abi.marshal((None, t, 7, 2.5, arr, ptr, t[1:]))
    assert out[0] is None and out[1] == t.data_ptr() and out[2] == 7 and out[3] == 2.5 and out[4] is arr and out[5] is ptr
    assert out[6] == t.data_ptr() + 4 and isinstance(out[2], int) and isinstance(out[3], float) and _abi.marshal(()) == []
