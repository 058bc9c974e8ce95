"""checkerpose_amd/scene.py on the device: every branch of the shared argument handling through every caller, at the smallest
shapes where it can still go wrong.  Two ways of saying the same scene must give the same bits (torch.equal on every output):

  camera       one (3,3) K / the same K repeated per pose (per image for vis_poses)
  mesh ids     [0,0,0] on the host (scratch sized by the 4 vertices used) / the same ids as an int32 device tensor (sized by all 8);
               [1,0,1] as a numpy array / as a list
  image ids    None with I == B / arange(B) on the host / on the device
  poses        device tensors / host arrays, where both are accepted (render_rgb, vis_poses)
  wrappers     each one-pose wrapper under the reference's name / row 0 of the batched call

Scene: a tetrahedron (4 vertices, 4 faces) and a cube (8 vertices, 12 faces) with colours and normals, two symmetry transforms for
the first and the identity for the second, B = 3 poses at Z near 400 under one K, a 48 x 40 frame (two by two tiles, the right and
the bottom ones partial), I = 3 depth images and frames.  Every object lies inside the frame, so every row is rendered -- asserted,
because a batch the kernels reject would pass every equality emptily."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W, H, B = 48, 40, 3
CALLS = ("pose_errors", "bop_errors", "vsd_errors", "render_depth", "mask_errors", "gt_info", "render_rgb", "vis_poses")
WITH_K = CALLS[1:]
WITH_IMAGES = ("vsd_errors", "gt_info", "vis_poses")
HOST_POSES = ("render_rgb", "vis_poses")
_C = {}


def _rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    x = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * x + (1.0 - np.cos(angle)) * x.dot(x)


def fixture():
    if "s" in _C:
        return _C["s"]
    from checkerpose_amd import scene
    tet = np.array([[-15.0, -10, -10], [15, -10, -10], [0, 16, -10], [0, 0, 14]])
    tet_f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    cube = np.array([[x, y, z] for x in (-12.0, 12) for y in (-12.0, 12) for z in (-12.0, 12)])
    cube_f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                       [1, 5, 7], [1, 7, 3]])
    rng = np.random.default_rng(48040)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)      # noqa: E731
    s = type("Scene", (), {})()
    s.tet, s.cube = tet, cube
    s.ms = scene.MeshSet.from_arrays([tet, cube], faces=[tet_f, cube_f], normals=[unit(tet), unit(cube)],
                                     colors=[rng.integers(30, 256, size=(4, 3), dtype=np.uint8), rng.uniform(0.2, 1.0, size=(8, 3))])
    s.ss = scene.SymmetrySet.from_transforms([[{"R": np.eye(3), "t": np.zeros(3)}, {"R": _rot((0, 0, 1), np.pi), "t": np.array([1.0, 0, 0])}],
                                              [{"R": np.eye(3), "t": np.zeros(3)}]])
    s.K = np.array([[200.0, 0.0, 24.3], [0.0, 202.0, 19.8], [0.0, 0.0, 1.0]])
    s.Rg = np.stack([_rot((1, 2, 3), 0.4), _rot((-1, 0.5, 2), 1.1), _rot((0.3, -1, 0.2), 2.0)])
    s.tg = np.array([[-18.0, 8.0, 400.0], [4.0, -6.0, 390.0], [20.0, 9.0, 410.0]]).reshape(B, 3, 1)
    s.Re = np.stack([_rot((0.2, 1, -0.4), 0.05 * (b + 1)).dot(s.Rg[b]) for b in range(B)])
    s.te = s.tg + np.array([[1.5, -1.0, 3.0], [-2.0, 0.5, -4.0], [0.5, 2.0, 2.0]]).reshape(B, 3, 1)
    s.depth = (400.0 + np.arange(B)[:, None, None] + rng.uniform(0.0, 2.0, size=(B, H, W))).astype(np.float32)
    s.frames = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    _C["s"] = s
    return s


def run(name, K=None, mesh_ids=(1, 0, 1), image_ids=None, host_poses=False):
    """one of the eight calls on the fixture scene with every optional output -> dict of device tensors"""
    from checkerpose_amd import gt_info as GI, metric, render, vis
    s, dev = fixture(), torch.device("cuda:0")
    K = s.K if K is None else K
    mids = list(mesh_ids) if isinstance(mesh_ids, tuple) else mesh_ids
    R, t = (s.Re, s.te) if host_poses else (torch.from_numpy(s.Re).to(dev), torch.from_numpy(s.te).to(dev))
    if name == "pose_errors":
        return metric.pose_errors(R, t, s.Rg, s.tg, s.ms, mesh_ids=mids)
    if name == "bop_errors":
        return metric.bop_errors(R, t, s.Rg, s.tg, K, s.ms, symmetries=s.ss, mesh_ids=mids)
    if name == "vsd_errors":
        return metric.vsd_errors(R, t, s.Rg, s.tg, K, s.ms, s.depth, image_ids=image_ids, mesh_ids=mids, sphere_check=False,
                                 return_counts=True, return_depth=True)
    if name == "render_depth":
        return {"depth": metric.render_depth(R, t, K, s.ms, (W, H), mesh_ids=mids)}
    if name == "mask_errors":
        return metric.mask_errors(R, t, s.Rg, s.tg, K, s.ms, (W, H), mesh_ids=mids, return_counts=True, return_boxes=True, return_masks=True)
    if name == "gt_info":
        return GI.gt_info(R, t, K, s.ms, s.depth, image_ids=image_ids, mesh_ids=mids, return_masks=True, return_depth=True)
    if name == "render_rgb":
        return render.render_rgb(R, t, K, s.ms, (W, H), mesh_ids=mids, return_depth=True, return_mask=True, return_boxes=True)
    assert name == "vis_poses"
    return vis.vis_poses(R, t, K, s.ms, torch.from_numpy(s.frames).to(dev), image_ids=image_ids, mesh_ids=mids, depth=s.depth, depth_diff=True)


def base(name, mesh_ids=(1, 0, 1)):
    """the call said the plain way, computed once and left unchanged"""
    key = (name, mesh_ids)
    if key not in _C:
        _C[key] = run(name, mesh_ids=mesh_ids)
    return _C[key]


def same(got, want, what):
    assert list(got.keys()) == list(want.keys()), what
    for k, v in want.items():
        assert torch.is_tensor(v) and v.is_cuda and got[k].dtype == v.dtype, (what, k)
        assert torch.equal(got[k], v), (what, k)


@pytest.mark.parametrize("mesh_ids", [(1, 0, 1), (0, 0, 0)])
def test_every_row_of_the_scene_is_rendered_and_scored(mesh_ids):
    for name in ("pose_errors", "bop_errors"):
        assert all(bool(torch.isfinite(v).all()) and bool((v > 0).all()) for v in base(name, mesh_ids).values()), name
    v = base("vsd_errors", mesh_ids)
    assert bool(torch.isfinite(v["vsd"]).all()) and bool((v["counts"][:, 0] > 0).all())
    assert bool((v["depth"] > 0).flatten(2).any(2).all())                              # both renders of every pose hold pixels
    assert bool((base("render_depth", mesh_ids)["depth"] > 0).flatten(1).any(1).all())
    m = base("mask_errors", mesh_ids)
    assert bool(m["ok"].all()) and bool(torch.isfinite(m["cus"]).all()) and bool(torch.isfinite(m["cou_bb_proj"]).all())
    assert bool((m["counts"][:, 2:] > 0).all()) and bool((m["boxes"] >= 0).all())
    g = base("gt_info", mesh_ids)
    assert bool(g["ok"].all()) and bool((g["px_count_visib"] > 0).all()) and bool((g["px_count_all"] == g["px_count_valid"]).all())
    r = base("render_rgb", mesh_ids)
    assert bool((r["ok"] == 1).all()) and bool((r["boxes"] >= 0).all())
    p = base("vis_poses", mesh_ids)
    assert bool((p["ok"] == 1).all()) and bool((p["boxes"] >= 0).all()) and bool((p["diff_ok"] == 1).all())
    assert bool(torch.isfinite(p["diff_stats"]).all())
    # inside the frame: no silhouette touches the border, so nothing was clipped away
    box = m["boxes"].reshape(-1, 4)
    assert bool((box[:, 0] > 0).all()) and bool((box[:, 1] > 0).all())
    assert bool((box[:, 0] + box[:, 2] < W - 1).all()) and bool((box[:, 1] + box[:, 3] < H - 1).all())


@pytest.mark.parametrize("name", WITH_K)
def test_one_camera_equals_the_same_camera_repeated(name):
    s = fixture()
    same(run(name, K=np.repeat(s.K[None], B, 0)), base(name), name)                    # (B,3,3); (I,3,3) for vis_poses: I == B
    same(run(name, K=torch.from_numpy(s.K).to("cuda:0")), base(name), name)           # a device K


@pytest.mark.parametrize("name", CALLS)
def test_host_mesh_ids_equal_device_mesh_ids(name):
    dev_ids = torch.zeros(B, dtype=torch.int32, device="cuda:0")                       # scratch sized by all 8 vertices, not the 4 used
    same(run(name, mesh_ids=dev_ids), base(name, (0, 0, 0)), name)
    same(run(name, mesh_ids=torch.tensor([1, 0, 1], device="cuda:0")), base(name), name)        # int64 on the device


@pytest.mark.parametrize("name", CALLS)
def test_mesh_ids_as_array_equal_a_list(name):
    same(run(name, mesh_ids=np.array([1, 0, 1])), base(name), name)
    same(run(name, mesh_ids=torch.tensor([1, 0, 1], dtype=torch.int16)), base(name), name)      # a CPU tensor is a host array


@pytest.mark.parametrize("name", WITH_IMAGES)
def test_default_image_ids_equal_arange(name):
    same(run(name, image_ids=list(range(B))), base(name), name)
    same(run(name, image_ids=np.arange(B)), base(name), name)
    same(run(name, image_ids=torch.arange(B, dtype=torch.int32, device="cuda:0")), base(name), name)


@pytest.mark.parametrize("name", HOST_POSES)
def test_host_poses_equal_device_poses(name):
    same(run(name, host_poses=True), base(name), name)


def test_one_pose_wrappers_equal_row_0_of_the_batch():
    from checkerpose_amd import metric
    s = fixture()
    est, gt = (s.Re[0], s.te[0]), (s.Rg[0], s.tg[0])
    for ids, verts, m in (((0, 0, 0), s.tet, 0), ((1, 0, 1), s.cube, 1)):               # row 0 is the tetrahedron, then the cube
        syms = s.ss.transforms(m)
        pe, be, ve, me = (base(n, ids) for n in ("pose_errors", "bop_errors", "vsd_errors", "mask_errors"))
        assert metric.Calculate_ADD_Error_BOP(gt[0], gt[1], est[0], est[1], verts) == float(pe["add"][0])
        assert metric.Calculate_ADI_Error_BOP(gt[0], gt[1], est[0], est[1], verts) == float(pe["adi"][0])
        assert metric.mssd(est[0], est[1], gt[0], gt[1], verts, syms) == float(be["mssd"][0])
        assert metric.mspd(est[0], est[1], gt[0], gt[1], s.K, verts, syms) == float(be["mspd"][0])
        assert metric.proj(est[0], est[1], gt[0], gt[1], s.K, verts) == float(be["proj"][0])
        got = metric.vsd(est[0], est[1], gt[0], gt[1], s.depth[0], s.K, 15.0, None, True, s.ms.diameters[m], s.ms, m)
        assert got == [float(e) for e in ve["vsd"][0].cpu()]
        assert metric.cus(est[0], est[1], gt[0], gt[1], s.K, s.ms, m, size=(W, H)) == float(me["cus"][0])
        assert metric.cou_bb_proj(est[0], est[1], gt[0], gt[1], s.K, s.ms, m, size=(W, H)) == float(me["cou_bb_proj"][0])
