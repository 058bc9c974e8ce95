"""Row N18 on the device: cp_vis_poses against the host composition (tests/vis_stages.compose) of the device's OWN per-pose
render_rgb(..., return_depth=True) frames, and cp_depth_diff_vis against the pictures the reference saved (tests/golden/vis_poses.npz).

  exact        vis, ren_rgb, the bits of ren_depth, boxes and ok are EQUAL to the composition, on 70 x 50 (3 x 2 ragged tiles), 32 x 32
               and 33 x 65 frames, 4 images (one without poses), 9 poses with interleaved image ids -- a duplicated pose (a depth tie), a
               pose off the frame, a pose with a vertex behind the camera, a black surface -- both shadings, both modes, surface
               colours and mesh colours
  depth diff   the recorded cases: picture, min, max and diff_ok EQUAL; the mean within 1e-9 * max|dd| of numpy's float64 mean
               (derived: at most 2^22 float64 additions of values <= max|dd|, u = 1.1e-16, so the error is <= 2^22 u max|dd| < 5e-10
               max|dd|); fewer than three distinct differences: diff_ok = 0 and zeros
  invariances  bit-identical across two calls, an image alone / in its batch, poses grouped / interleaved, shared / repeated K, with /
               without depth_diff; draw_boxes=False is the blend without the layer
  launches     the same launch list whatever the poses
  scripts      vis_est_poses and vis_gt_poses equal direct vis_poses calls"""
import json
import os

import numpy as np
import pytest
import torch

from tests import render_rgb_stages as RS
from tests import vis_stages as VS
from tests.common import GOLDEN

pytestmark = pytest.mark.gpu

NAMES = ("box", "ico80", "quad", "tri3", "halfbox")
IMAGE_IDS = [0, 2, 0, 3, 2, 0, 3, 2, 0]                   # interleaved; image 1 has no pose
N_IMG = 4
MESH = ["box", "ico80", "ico80", "quad", "ico80", "tri3", "halfbox", "box", "halfbox"]
SURF = [(0.89, 0.28, 0.13), (0.45, 0.38, 0.92), (0.35, 0.73, 0.63), (0.62, 0.28, 0.91), (0.65, 0.71, 0.22), (0.8, 0.29, 0.89), (0.27, 0.55, 0.22),
        (0.0, 0.0, 0.0), (0.84, 0.63, 0.22)]              # pose 7: a black surface
_C = {}


def mesh_set():
    from checkerpose_amd import metric
    if "ms" not in _C:
        m = RS.meshes()
        _C["ms"] = metric.MeshSet.from_arrays([m[k][0] for k in NAMES], faces=[m[k][1] for k in NAMES], colors=[m[k][2] for k in NAMES],
                                               normals=[m[k][3] for k in NAMES], diameters=[100.0] * len(NAMES))
    return _C["ms"]


def _rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene(size):
    """(R (9,3,3), t (9,3,1), K (3,3), frames uint8 (4,H,W,3) numpy) of a frame size, seeded"""
    if size not in _C:
        W, H = size
        rng = np.random.default_rng(1000 * W + H)
        f = 2.2 * max(W, H)
        K = np.array([[f, 0.0, W / 2.0 + 0.3], [0.0, f * 1.01, H / 2.0 - 0.2], [0.0, 0.0, 1.0]])
        R = np.stack([_rot(rng) for _ in IMAGE_IDS])
        t = np.array([[-35.0, 5.0, 420.0], [4.0, -3.0, 380.0], [25.0, 10.0, 400.0], [-10.0, 8.0, 350.0], [4.0, -3.0, 380.0], [5000.0, 0.0, 400.0],
                      [0.0, 0.0, 10.0], [20.0, 6.0, 300.0], [70.0, -20.0, 450.0]]).reshape(-1, 3, 1)
        R[4] = R[1]                                                    # pose 4 duplicates pose 1: an exact depth tie
        frames = rng.integers(0, 256, size=(N_IMG, H, W, 3), dtype=np.uint8)
        frames[:, : H // 5] = 255
        _C[size] = (R, t, K, frames)
    return _C[size]


def per_pose_frames(size, shading, colour_mode):
    """the device's own render_rgb of every pose alone, once per configuration -> (m_rgb (9,H,W,3), m_depth (9,H,W), ok (9,))"""
    key = ("frames", size, shading, colour_mode)
    if key not in _C:
        from checkerpose_amd import render
        R, t, K, _ = scene(size)
        dev = torch.device("cuda:0")
        rgbs, depths, oks = [], [], []
        for b in range(len(IMAGE_IDS)):
            r = render.render_rgb(torch.from_numpy(R[b:b + 1]).to(dev), torch.from_numpy(t[b:b + 1]).to(dev), K, mesh_set(), size,
                                  mesh_ids=[NAMES.index(MESH[b])], shading=shading, bg_color=(0, 0, 0),
                                  surf_color=SURF[b] if colour_mode == "surf" else None, return_depth=True)
            rgbs.append(r["rgb"][0].cpu().numpy())
            depths.append(r["depth"][0].cpu().numpy())
            oks.append(int(r["ok"][0]))
        _C[key] = (np.stack(rgbs), np.stack(depths), np.array(oks))
    return _C[key]


def device_call(size, shading="phong", colour_mode="surf", poses=None, image_ids=None, n_img=N_IMG, frames=None, K=None, **kw):
    from checkerpose_amd import vis
    R, t, K0, fr = scene(size)
    poses = list(range(len(IMAGE_IDS))) if poses is None else poses
    dev = torch.device("cuda:0")
    return vis.vis_poses(torch.from_numpy(R[poses]).to(dev), torch.from_numpy(t[poses]).to(dev), K0 if K is None else K, mesh_set(),
                         torch.from_numpy(fr if frames is None else frames).to(dev),
                         image_ids=[IMAGE_IDS[b] for b in poses] if image_ids is None else image_ids,
                         mesh_ids=[NAMES.index(MESH[b]) for b in poses], surf_colors=[SURF[b] for b in poses] if colour_mode == "surf" else None,
                         shading=shading, **kw)


def host(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


CONFIGS = [((70, 50), "phong", "surf"), ((70, 50), "flat", "mesh"), ((32, 32), "phong", "surf"), ((32, 32), "flat", "mesh"), ((33, 65), "phong", "mesh"),
           ((33, 65), "flat", "surf"), ((70, 50), "flat", "surf"), ((70, 50), "phong", "mesh")]


@pytest.mark.parametrize("size,shading,colour_mode", CONFIGS)
def test_equals_the_host_composition_of_the_devices_own_renders(size, shading, colour_mode):
    m_rgb, m_depth, ok = per_pose_frames(size, shading, colour_mode)
    frames = scene(size)[3]
    assert ok.tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 1]                  # pose 6 has a vertex behind the camera
    assert not m_depth[5].any() and m_depth[0].any()                   # pose 5 is off the frame
    for resolve in (True, False):
        d = host(device_call(size, shading, colour_mode, resolve_visib=resolve))
        assert d["ok"].tolist() == ok.tolist()
        for img in range(N_IMG):
            mine = [b for b, i in enumerate(IMAGE_IDS) if i == img]
            e = VS.compose(frames[img], m_rgb[mine], m_depth[mine], resolve=resolve)
            what = (size, shading, colour_mode, resolve, img)
            assert np.array_equal(d["ren_rgb"][img], e["ren_rgb"]), what
            assert np.array_equal(d["ren_depth"][img].view(np.int32), e["ren_depth"].view(np.int32)), what
            assert np.array_equal(d["vis"][img], e["vis"]), what
            assert d["boxes"][mine].tolist() == e["boxes"].tolist(), what
    if colour_mode == "surf":                                          # the black surface occludes and has no box
        assert d["boxes"][7].tolist() == [-1, -1, -1, -1] and m_depth[7].any()
    assert d["boxes"][5].tolist() == [-1, -1, -1, -1] and d["boxes"][6].tolist() == [-1, -1, -1, -1]
    assert not d["ren_depth"][1].any() and np.array_equal(d["vis"][1], frames[1] // 2)      # the image without poses
    tie = (m_depth[1] > 0) & (m_depth[1] == m_depth[4])
    assert tie.any() and np.array_equal(m_depth[1], m_depth[4])


def _golden():
    if "golden" not in _C:
        z = np.load(os.path.join(GOLDEN, "vis_poses.npz"))
        _C["golden"] = (z, json.loads(bytes(z["meta"]).decode()))
    return _C["golden"]


def test_depth_difference_equals_the_recorded_pictures():
    from checkerpose_amd import vis
    z, meta = _golden()
    dev = torch.device("cuda:0")
    n = 0
    for shape in ((40, 48), (31, 33)):
        cis = [ci for ci, m in enumerate(meta) if m["dd"] and z["c%02d_frame" % ci].shape[:2] == shape]
        rens = np.stack([VS.compose(z["c%02d_frame" % ci], z["c%02d_m_rgb" % ci], z["c%02d_m_depth" % ci])["ren_depth"] for ci in cis])
        deps = np.stack([z["c%02d_depth" % ci] for ci in cis])
        # one extra render with two distinct differences only, and one without a valid pixel
        two = np.zeros(shape, dtype=np.float32)
        two[2:9, 3:12] = 500.0
        rens = np.concatenate([rens, two[None], np.zeros((1,) + shape, dtype=np.float32)])
        deps = np.concatenate([deps, np.full((1,) + shape, 490.0, dtype=np.float32), deps[:1]])
        batch = host(vis.depth_diff_vis(torch.from_numpy(rens).to(dev), torch.from_numpy(deps).to(dev)))
        for j, ci in enumerate(cis):
            name = meta[ci]["name"]
            assert int(batch["diff_ok"][j]) == 1, name
            assert np.array_equal(batch["depth_diff"][j], z["c%02d_dd_vis" % ci]), name
            assert np.array_equal(batch["diff_stats"][j, :2], z["c%02d_dd_minmax" % ci]), name
            dd, valid = VS.dd_of(rens[j], deps[j])
            mean, bound = float(dd[valid].astype(np.float64).mean()), 1e-9 * float(np.abs(dd).max())
            print("%s: mean %.17g device %.17g bound %.3g" % (name, mean, batch["diff_stats"][j, 2], bound))
            assert abs(batch["diff_stats"][j, 2] - mean) <= bound, name
            alone = host(vis.depth_diff_vis(torch.from_numpy(rens[j:j + 1]).to(dev), torch.from_numpy(deps[j]).to(dev)))      # alone = in the batch
            assert all(np.array_equal(alone[k][0].view(np.uint8), batch[k][j].view(np.uint8)) for k in ("depth_diff", "diff_stats", "diff_ok")), name
            n += 1
        k2 = len(cis)
        assert int(batch["diff_ok"][k2]) == 0 and not batch["depth_diff"][k2].any() and batch["diff_stats"][k2].tolist() == [10.0, 10.0, 10.0]
        assert int(batch["diff_ok"][k2 + 1]) == 0 and not batch["depth_diff"][k2 + 1].any() and np.isnan(batch["diff_stats"][k2 + 1]).all()
        again = host(vis.depth_diff_vis(torch.from_numpy(rens).to(dev), torch.from_numpy(deps).to(dev)))
        assert all(np.array_equal(again[k].view(np.uint8), batch[k].view(np.uint8)) for k in batch)
        # the image map: every render against depth image 0, by ids and as the one image
        ids = host(vis.depth_diff_vis(torch.from_numpy(rens).to(dev), torch.from_numpy(deps).to(dev), image_ids=[0] * len(rens)))
        one = host(vis.depth_diff_vis(torch.from_numpy(rens).to(dev), torch.from_numpy(deps[0]).to(dev)))
        assert all(np.array_equal(ids[k].view(np.uint8), one[k].view(np.uint8)) for k in ids)
        assert np.array_equal(ids["depth_diff"][0], batch["depth_diff"][0])
    assert n >= 4


def same(a, b, keys=("vis", "ren_rgb", "ren_depth", "boxes", "ok")):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in keys)


def test_outputs_do_not_depend_on_the_call_the_batch_or_the_order():
    size = (70, 50)
    R, t, K, frames = scene(size)
    base = host(device_call(size))
    assert same(base, host(device_call(size)))                                           # two calls
    for img in range(N_IMG):                                                             # an image alone against its batch
        mine = [b for b, i in enumerate(IMAGE_IDS) if i == img]
        if not mine:
            continue
        alone = host(device_call(size, poses=mine, image_ids=[0] * len(mine), frames=frames[img:img + 1]))
        for k in ("vis", "ren_rgb", "ren_depth"):
            assert np.array_equal(alone[k][0].view(np.uint8), base[k][img].view(np.uint8)), (img, k)
        assert np.array_equal(alone["boxes"], base["boxes"][mine]) and np.array_equal(alone["ok"], base["ok"][mine])
    grouped = sorted(range(len(IMAGE_IDS)), key=lambda b: IMAGE_IDS[b])                  # grouped against interleaved (stable: same order per image)
    g = host(device_call(size, poses=grouped))
    assert same(g, base, ("vis", "ren_rgb", "ren_depth")) and np.array_equal(g["boxes"], base["boxes"][grouped]) and np.array_equal(g["ok"], base["ok"][grouped])
    assert same(host(device_call(size, K=np.stack([K] * N_IMG))), base)                  # shared against repeated K
    depth = np.where(base["ren_depth"] > 0, base["ren_depth"] - np.float32(3.0), np.float32(600.0)).astype(np.float32)
    depth[:, ::7] = 0.0
    depth[:, 1::5] += np.float32(25.0)
    with_dd = host(device_call(size, depth=torch.from_numpy(depth), depth_diff=True))    # with and without depth_diff
    assert same(with_dd, base)
    from checkerpose_amd import vis
    direct = host(vis.depth_diff_vis(torch.from_numpy(base["ren_depth"]).cuda(), torch.from_numpy(depth).cuda()))
    assert all(np.array_equal(with_dd[k].view(np.uint8), direct[k].view(np.uint8)) for k in direct)
    for img in range(N_IMG):
        pic, stats, ok = VS.depth_diff(base["ren_depth"][img], depth[img])
        assert int(with_dd["diff_ok"][img]) == ok and np.array_equal(with_dd["depth_diff"][img], pic), img
        assert np.array_equal(with_dd["diff_stats"][img, :2], stats[:2], equal_nan=True)
    plain = host(device_call(size, draw_boxes=False))                                    # the blend without the layer
    assert same(plain, base, ("ren_rgb", "ren_depth", "boxes", "ok"))
    assert np.array_equal(plain["vis"], ((frames.astype(np.int64) + base["ren_rgb"]) // 2).astype(np.uint8))
    assert (base["vis"] != plain["vis"]).any()
    white = host(device_call(size, box_color=(1.0, 0.5, 0.0)))
    on = (white["vis"] != plain["vis"]).any(-1)
    assert on.any() and (white["vis"][on][:, 0] == 255).all()


def test_an_image_may_hold_more_than_32_poses():
    """cp_render_scene clamps an image's rows of the image-to-poses CSR to 32 (one bit per pose); cp_vis_poses, which reads the rows
    through the same accessor, must not.  33 tetrahedra (tests/test_gpu_scene.py's) in ONE 48 x 40 image at 33 distinct depths,
    overlapping near the centre, the nearest one LAST in the order: ren_depth is, bit for bit, the per-pixel smallest positive value
    of render_depth's 33 images (the rule at the top of vis_poses.hip: m_depth is cp_render_depth's, the update a strict minimum)."""
    from checkerpose_amd import metric, vis
    from tests import test_gpu_scene as SC
    s, n, dev = SC.fixture(), 33, torch.device("cuda:0")
    R = np.stack([SC._rot((1, 2, 3), 0.19 * j) for j in range(n)])
    t = np.array([[3.0 * np.cos(1.3 * j), 3.0 * np.sin(1.3 * j), 476.0 - 3.0 * j] for j in range(n)]).reshape(n, 3, 1)      # pose 32: Z = 380
    Rd, td = torch.from_numpy(R).to(dev), torch.from_numpy(t).to(dev)
    each = metric.render_depth(Rd, td, s.K, s.ms, (SC.W, SC.H), mesh_ids=[0] * n).cpu().numpy()
    assert each.shape == (n, SC.H, SC.W) and all(e.any() for e in each)
    want = np.where(each > 0, each, np.float32(np.inf)).min(axis=0)
    want[np.isinf(want)] = 0.0
    r = host(vis.vis_poses(Rd, td, s.K, s.ms, torch.zeros(1, SC.H, SC.W, 3, dtype=torch.uint8, device=dev), image_ids=[0] * n, mesh_ids=[0] * n))
    assert r["ok"].tolist() == [1] * n
    assert np.array_equal(r["ren_depth"][0].view(np.int32), want.view(np.int32))
    assert ((each[n - 1] > 0) & (r["ren_depth"][0] == each[n - 1])).any()            # the last pose, past row 32, owns pixels


def test_the_launch_list_does_not_depend_on_the_poses():
    from checkerpose_amd import _abi
    lib = _abi.load()
    logs = []
    for poses in (None, [5, 6], [0], [1, 4, 7]):
        lib.cp_kernel_log_begin()
        device_call((70, 50), poses=poses, resolve_visib=poses is None)
        logs.append(lib.cp_kernel_log().decode())
    assert len(set(logs)) == 1, logs
    for k in ("vis_pose_kernel", "vis_vertex_kernel", "vis_scene_tile_kernel", "vis_finish_kernel"):
        assert logs[0].count(k) == 1, logs[0]
    from checkerpose_amd import vis
    lib.cp_kernel_log_begin()
    vis.depth_diff_vis(torch.zeros(2, 31, 33, device="cuda:0"), torch.ones(31, 33, device="cuda:0"))
    log = lib.cp_kernel_log().decode()
    for k in ("dd_init_kernel", "dd_reduce_kernel", "dd_second_kernel", "dd_stats_kernel", "dd_colour_kernel"):
        assert log.count(k) == 1, log


def test_the_scripts_equal_direct_calls():
    from checkerpose_amd import vis
    size = (70, 50)
    R, t, K, frames = scene(size)
    ms = mesh_set()
    obj_index = {3 + 2 * m: m for m in range(len(NAMES))}                               # object ids 3, 5, 7, 9, 11
    obj_of = lambda b: 3 + 2 * NAMES.index(MESH[b])                                     # noqa: E731
    palette = json.load(open(os.path.join(GOLDEN, "vis_colors.json")))
    im_of = {0: 11, 2: 4, 3: 8}                                                          # image ids of the scene
    cam = {im: {"cam_K": K, "depth_scale": 1.0} for im in (11, 4, 8)}
    fr = {11: frames[0], 4: frames[2], 8: frames[3]}
    use = [b for b in range(len(IMAGE_IDS)) if b != 6]
    # ground truths: per image in ascending im_id, gt order
    scene_gt = {}
    for b in use:
        scene_gt.setdefault(im_of[IMAGE_IDS[b]], []).append({"obj_id": obj_of(b), "cam_R_m2c": R[b], "cam_t_m2c": t[b]})
    out = vis.vis_gt_poses(scene_gt, cam, fr, ms, obj_index, palette=palette)
    assert list(out.keys()) == [4, 8, 11]
    dev = torch.device("cuda:0")
    for im, img in ((4, 2), (8, 3), (11, 0)):
        mine = [b for b in use if IMAGE_IDS[b] == img]
        d = vis.vis_poses(torch.from_numpy(R[mine]).to(dev), torch.from_numpy(t[mine]).to(dev), K, ms, torch.from_numpy(frames[img:img + 1]).to(dev),
                          mesh_ids=[NAMES.index(MESH[b]) for b in mine], surf_colors=[palette[(obj_of(b) - 1) % len(palette)] for b in mine],
                          image_ids=[0] * len(mine), shading="flat")
        for k in ("vis", "ren_rgb", "ren_depth"):
            assert torch.equal(out[im][k], d[k][0]), (im, k)
        assert torch.equal(out[im]["boxes"], d["boxes"]) and torch.equal(out[im]["ok"], d["ok"])
    # estimates: image 4 (poses 1, 4, 7) -- two of the same object with scores, n_top = 1 keeps the better one
    ests = [{"im_id": 4, "obj_id": obj_of(1), "score": 0.3, "R": R[1], "t": t[1]}, {"im_id": 4, "obj_id": obj_of(7), "score": 0.9, "R": R[7], "t": t[7]},
            {"im_id": 4, "obj_id": obj_of(4), "score": 0.8, "R": _rot(np.random.default_rng(3)), "t": t[4]}]
    out = vis.vis_est_poses(ests, cam, fr, ms, obj_index, palette=None, n_top=1)
    assert list(out.keys()) == [(4, obj_of(1)), (4, obj_of(7))]
    d = vis.vis_poses(torch.from_numpy(np.stack([ests[2]["R"], R[7]])).to(dev), torch.from_numpy(np.stack([t[4], t[7]])).to(dev), K, ms,
                      torch.from_numpy(np.stack([frames[2], frames[2]])).to(dev), mesh_ids=[NAMES.index(MESH[4]), NAMES.index(MESH[7])])
    for g, key in enumerate(out.keys()):
        for k in ("vis", "ren_rgb", "ren_depth"):
            assert torch.equal(out[key][k], d[k][g]), (key, k)
        assert torch.equal(out[key]["boxes"], d["boxes"][g:g + 1])
    joined = vis.vis_est_poses(ests, cam, fr, ms, obj_index, palette=palette, vis_per_obj_id=False, n_top=0, resolve_visib=False)
    assert list(joined.keys()) == [4] and joined[4]["boxes"].shape == (3, 4)
