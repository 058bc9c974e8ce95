"""Row N10 on the device: cp_gt_info / cp_gt_info_from_depth against tests/golden/gt_info.npz and the stages of
tests/gt_info_stages.py (fixture and oracle: tests/test_gt_info.py; bounds: tests/vsd_stages.py's, unchanged).

  counting     cp_gt_info_from_depth on the recorded depth_gt_large gives the scripts' counts, both boxes, visib_fract (the same bits)
               and both masks EXACTLY;
  rasteriser   the in-frame depth gt_info returns equals metric.render_depth at (W,H) bit for bit, and passes the oracle's interval
               check on every case;
  end to end   the in-frame outputs (px_count_valid, px_count_visib, bbox_visib, both masks) EQUAL the numpy counting applied to the
               depth gt_info returns; every count lies in the interval the undecided pixels allow, every box between the box of the
               surely-set and of the possibly-set pixels, the masks equal the oracle's on every decided pixel;
  bitwise      two calls, a pose alone against in its batch of mixed meshes, with / without the images, shared K against repeated
               K, poses that are not rendered (ok = 0) next to ones that are;
  integration  targets.make_training_batch labels from gt_info's masks and bbox_visib equal the ones from the numpy counting's."""
import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, gt_info as GI, metric, targets
from tests import gt_info_stages as G
from tests import vsd_stages as S
from tests.test_gt_info import depth_of, fixture, intervals, n_cases, oracle, recorded, size_of
from tests.test_vsd_error import mesh_set

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_SHARED = {}
LAUNCHES = "gt_info_pose_kernel + gt_info_vertex_kernel + gt_info_tile_kernel + gt_info_finish_kernel"


def _dev(a, shape):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))).to(DEV)


def _scenes():
    """scene -> the fixture cases of it (one frame size and delta each); the pose behind the camera rides in its scene's batch"""
    g, _ = fixture()
    out = {}
    for c in range(n_cases()):
        out.setdefault(int(g["scene"][c]), []).append(c)
    return out


def _inputs(idx):
    g, _ = fixture()
    n = len(idx)
    images = sorted({int(g["image"][c]) for c in idx})
    depth = torch.from_numpy(np.stack([g["depth_%d" % i] for i in images])).to(DEV)
    return (_dev(g["R"][idx], (n, 3, 3)), _dev(g["t"][idx], (n, 3, 1)), _dev(g["K"][idx], (n, 3, 3)), depth,
            [images.index(int(g["image"][c])) for c in idx], [int(m) for m in g["mesh"][idx]])


def _run(scene):
    """scene `scene` through gt_info (masks and depth back), once, shared"""
    if scene not in _SHARED:
        g, _ = fixture()
        idx = _scenes()[scene]
        R, t, K, depth, img, ids = _inputs(idx)
        lib = _abi.load()
        lib.cp_kernel_log_begin()
        out = GI.gt_info(R, t, K, mesh_set(), depth, image_ids=img, mesh_ids=ids, delta=float(g["delta"][idx[0]]), return_masks=True, return_depth=True)
        assert lib.cp_kernel_log().decode() == LAUNCHES
        W, H = size_of(idx[0])
        assert out["px_count_all"].dtype == torch.int32 and out["visib_fract"].dtype == torch.float64 and out["ok"].dtype == torch.bool
        assert tuple(out["bbox_obj"].shape) == (len(idx), 4) and out["bbox_visib"].dtype == torch.int32
        assert tuple(out["mask"].shape) == (len(idx), H, W) and out["mask"].dtype == torch.uint8 and out["depth"].dtype == torch.float32
        _SHARED[scene] = (idx, {k: v.cpu().numpy() for k, v in out.items()})
    return _SHARED[scene]


def _row(out, j):
    """pose j of a result (numpy) as gt_info_stages.count's dict"""
    r = {k: out[k][j] for k in G.INFO_KEYS}
    if "mask" in out:
        assert set(np.unique(out["mask"][j])) <= {0, 255} and set(np.unique(out["mask_visib"][j])) <= {0, 255}
        r["mask"], r["mask_visib"] = out["mask"][j] > 0, out["mask_visib"][j] > 0
    return r


def _same(a, b, keys=G.INFO_KEYS + ("ok",)):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in keys)


def test_counting_on_the_recorded_canvas_equals_the_scripts():
    g, _ = fixture()
    for scene, idx in _scenes().items():
        idx = [c for c in idx if g["ok"][c]]
        _, _, K, depth, img, _ = _inputs(idx)
        large = torch.from_numpy(np.stack([g["large_%d" % c] for c in idx])).to(DEV)
        out = GI.gt_info_from_depth(large, depth, K, image_ids=img, delta=float(g["delta"][idx[0]]), return_masks=True)
        out = {k: v.cpu().numpy() for k, v in out.items()}
        assert out["ok"].all()
        for j, c in enumerate(idx):
            got, rec = _row(out, j), recorded(c)
            print("case %2d %s" % (c, [np.asarray(got[k]).tolist() for k in G.INFO_KEYS]))
            assert G.same_info(got, rec), (c, got, rec)
            assert np.array_equal(got["mask"], rec["mask"]) and np.array_equal(got["mask_visib"], rec["mask_visib"]), c
        plain = GI.gt_info_from_depth(large, depth, K, image_ids=img, delta=float(g["delta"][idx[0]]))
        assert "mask" not in plain and _same({k: v.cpu().numpy() for k, v in plain.items()}, out)
    c = 0                                                                               # one (H,W) image, one K
    one = GI.gt_info_from_depth(torch.from_numpy(g["large_%d" % c])[None].to(DEV), depth_of(c), g["K"][c], delta=float(g["delta"][c]))
    assert G.same_info({k: v.cpu().numpy()[0] for k, v in one.items()}, recorded(c))


def test_in_frame_depth_equals_render_depth_and_passes_the_interval_check():
    g, _ = fixture()
    worst = 0.0
    for scene in _scenes():
        idx, out = _run(scene)
        R, t, K, _, _, ids = _inputs(idx)
        size = size_of(idx[0])
        d = metric.render_depth(R, t, K, mesh_set(), size, mesh_ids=ids).cpu().numpy()
        assert np.array_equal(d.view(np.uint32), out["depth"].view(np.uint32)), scene       # bit for bit: the canvas grid is anchored at (0, 0)
        for j, c in enumerate(idx):
            if not g["ok"][c]:
                assert (out["depth"][j] == 0).all()
                continue
            o = {k: (G.frame_of(v, size) if isinstance(v, np.ndarray) else v) for k, v in oracle(c).items()}
            ok, ratio, nbad = S.check_render(out["depth"][j], o)
            worst = max(worst, ratio)
            print("case %2d worst |diff| / tol_d on decided pixels %.4f, pixels outside their interval %d" % (c, ratio, nbad))
            assert ok, (c, ratio, nbad)
    print("gt_info in-frame depth: worst |diff| / tol_d %.4f" % worst)


def test_gt_info_end_to_end():
    g, _ = fixture()
    equal = 0
    for scene in _scenes():
        idx, out = _run(scene)
        for j, c in enumerate(idx):
            got = _row(out, j)
            if not g["ok"][c]:                                                          # a vertex at Z <= 0: not rendered
                assert not out["ok"][j] and G.same_info(got, recorded(c)) and not got["mask"].any() and not got["mask_visib"].any()
                continue
            assert out["ok"][j]
            W, H = size_of(c)
            canvas = np.zeros((3 * H, 3 * W), dtype=np.float32)
            canvas[H:2 * H, W:2 * W] = out["depth"][j]
            mine = G.count(canvas, depth_of(c), g["K"][c], float(g["delta"][c]))         # the numpy counting on the depth it returned
            for k in ("px_count_valid", "px_count_visib", "bbox_visib"):
                assert np.array_equal(np.asarray(got[k]), np.asarray(mine[k])), (c, k, got[k], mine[k])
            assert np.array_equal(got["mask"], mine["mask"]) and np.array_equal(got["mask_visib"], mine["mask_visib"]), c
            assert got["px_count_all"] >= mine["px_count_all"]                          # the canvas holds the frame
            assert float(got["visib_fract"]) == (got["px_count_visib"] / float(got["px_count_all"]) if got["px_count_all"] > 0 else 0.0)
            iv = intervals(c)
            bad = G.check_against_intervals(got, iv, (W, H))
            same = G.same_info(got, recorded(c))
            equal += same
            print("case %2d device %s recorded %s equal %s slack all %d visib %d"
                  % (c, [np.asarray(got[k]).tolist() for k in G.INFO_KEYS], [np.asarray(recorded(c)[k]).tolist() for k in G.INFO_KEYS], same,
                     iv["all"][1] - iv["all"][0], iv["visib"][1] - iv["visib"][0]))
            assert not bad, (c, bad)
    print("gt_info: %d of %d rendered cases equal the recorded results outright" % (equal, n_cases() - 1))


def test_bitwise_two_calls_alone_without_images_and_shared_k():
    g, _ = fixture()
    ms = mesh_set()
    idx, out = _run(1)
    R, t, K, depth, img, ids = _inputs(idx)
    kw = dict(delta=float(g["delta"][idx[0]]))
    again = GI.gt_info(R, t, K, ms, depth, image_ids=img, mesh_ids=ids, **kw)            # a second call, no images
    assert sorted(again) == sorted(G.INFO_KEYS + ("ok",)) and _same({k: v.cpu().numpy() for k, v in again.items()}, out)
    only_depth = GI.gt_info(R, t, K, ms, depth, image_ids=img, mesh_ids=ids, return_depth=True, **kw)
    assert _same({k: v.cpu().numpy() for k, v in only_depth.items()}, out, G.INFO_KEYS + ("ok", "depth"))
    for j in (1, 6, 7, 14, len(idx) - 1):                                               # a pose alone (an edge, the margin, the canvas edge, a shared image)
        one = GI.gt_info(R[j:j + 1], t[j:j + 1], K[j], ms, depth[img[j]], mesh_ids=[ids[j]], return_masks=True, return_depth=True, **kw)
        one = {k: v.cpu().numpy() for k, v in one.items()}
        assert all(np.array_equal(one[k][0], out[k][j]) for k in one), (j, {k: one[k][0] for k in G.INFO_KEYS})
    same_k = [j for j, c in enumerate(idx) if g["kgroup"][c] == 0]                       # one K for all: shared against repeated
    sel = torch.tensor(same_k, device=DEV)
    shared = GI.gt_info(R[sel], t[sel], K[same_k[0]], ms, depth, image_ids=[img[j] for j in same_k], mesh_ids=[ids[j] for j in same_k],
                        return_masks=True, **kw)
    assert all(np.array_equal(v.cpu().numpy(), out[k][same_k]) for k, v in shared.items())


def test_poses_that_are_not_rendered_leave_their_neighbours_alone():
    g, _ = fixture()
    ms = mesh_set()
    idx, ref = _run(1)
    R, t, K, depth, img, ids = _inputs(idx)
    j = 0                                                                               # the box in the middle of the frame, five times
    R5, t5, K5 = R[j:j + 1].repeat(5, 1, 1), t[j:j + 1].repeat(5, 1, 1).clone(), K[j:j + 1].repeat(5, 1, 1).clone()
    t5[0, 2, 0] = 10.0                                                                  # straddles the camera plane
    t5[1, 0, 0] = float("nan")
    K5[2, 0, 0] = float("inf")
    mesh = torch.tensor([ids[j], ids[j], ids[j], 99, ids[j]], dtype=torch.int32, device=DEV)         # device-side ids are checked on the device
    image = torch.tensor([img[j], img[j], img[j], img[j], img[j]], dtype=torch.int32, device=DEV)
    out = GI.gt_info(R5, t5, K5, ms, depth, image_ids=image, mesh_ids=mesh, return_masks=True, return_depth=True)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert out["ok"].tolist() == [False, False, False, False, True]
    for b in range(4):
        assert out["px_count_all"][b] == 0 and out["px_count_valid"][b] == 0 and out["px_count_visib"][b] == 0 and out["visib_fract"][b] == 0.0
        assert out["bbox_obj"][b].tolist() == [-1] * 4 and out["bbox_visib"][b].tolist() == [-1] * 4
        assert not out["mask"][b].any() and not out["mask_visib"][b].any() and not out["depth"][b].any()
    assert all(np.array_equal(out[k][4], ref[k][j]) for k in out)
    image[4] = 1000                                                                     # an image id out of range
    bad = GI.gt_info(R5, t5, K5, ms, depth, image_ids=image, mesh_ids=mesh)
    assert not bad["ok"].any() and not bad["px_count_all"].any()
    with pytest.raises(ValueError, match="no faces"):
        GI.gt_info(R5, t5, K5, metric.MeshSet.from_arrays([np.ones((4, 3), np.float32)], diameters=[1.0]), depth[0])


def test_full_frame_pair_and_scene_gt_info():
    g, meshes = fixture()
    ms = mesh_set()
    rng = np.random.default_rng(5)
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    Rm = np.stack([g["R"][21], g["R"][10]])                                             # the 20 480-triangle sphere, cut by the left edge; the torus
    tm = np.array([[-240.0, -30.0, 420.0], [60.0, 40.0, 380.0]])
    names = [str(n) for n in g["mesh_names"]]
    ids = [names.index("ico20480"), names.index("torus")]
    depth = (350.0 + 80.0 * rng.random((480, 640))).astype(np.float32)
    depth[rng.random(depth.shape) < 0.1] = 0.0
    out = GI.gt_info(_dev(Rm, (2, 3, 3)), _dev(tm, (2, 3, 1)), K, ms, depth, mesh_ids=ids, return_masks=True, return_depth=True)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for b in range(2):
        canvas = np.zeros((3 * 480, 3 * 640), dtype=np.float32)
        canvas[480:960, 640:1280] = out["depth"][b]
        mine = G.count(canvas, depth, K, 15.0)
        got = _row(out, b)
        print("640 x 480 pose %d %s" % (b, [np.asarray(got[k]).tolist() for k in G.INFO_KEYS]))
        assert all(np.array_equal(np.asarray(got[k]), np.asarray(mine[k])) for k in ("px_count_valid", "px_count_visib", "bbox_visib", "mask", "mask_visib"))
        assert got["px_count_visib"] > 1000 and got["px_count_all"] >= mine["px_count_all"]
    assert out["bbox_obj"][0, 0] < 0 and out["px_count_all"][0] > int((out["depth"][0] > 0).sum())      # the truncated part is counted
    assert out["px_count_all"][1] == int((out["depth"][1] > 0).sum())
    scene_gt = {4: [{"obj_id": 6, "cam_R_m2c": Rm[0], "cam_t_m2c": tm[0].reshape(3, 1)}, {"obj_id": 7, "cam_R_m2c": Rm[1], "cam_t_m2c": tm[1].reshape(3, 1)}]}
    info = GI.scene_gt_info(scene_gt, {4: {"cam_K": K, "depth_scale": 0.5}}, {4: depth * np.float32(2.0)}, ms, {6: ids[0], 7: ids[1]}, device=DEV)
    assert list(info) == [4] and len(info[4]) == 2
    for b in range(2):
        assert G.same_info(info[4][b], _row(out, b)) and type(info[4][b]["px_count_all"]) is int and type(info[4][b]["visib_fract"]) is float


def test_make_training_batch_takes_the_masks_and_boxes():
    g, _ = fixture()
    idx, out = _run(3)                                                                  # 160 x 120, two objects in one image
    W, H = size_of(idx[0])
    rng = np.random.default_rng(2)
    frames = torch.from_numpy(rng.integers(0, 256, (len(idx), H, W, 3), dtype=np.uint8)).to(DEV)
    pts = np.stack([fixture()[1]["ico80"][0][:32].astype(np.float64)] * 1)[0]
    R, t, K, _, _, _ = _inputs(idx)
    boxes_dev = [out["bbox_visib"][j].tolist() for j in range(len(idx))]
    assert all(b[2] > 0 and b[3] > 0 for b in boxes_dev)
    rows = list(range(len(idx)))
    from_device = targets.make_training_batch(frames, torch.from_numpy(out["mask_visib"]).to(DEV), torch.from_numpy(out["mask"]).to(DEV), R, t, K,
                                              boxes_dev, pts, is_train=False, img_index=rows)
    host = []
    for j, c in enumerate(idx):
        canvas = np.zeros((3 * H, 3 * W), dtype=np.float32)
        canvas[H:2 * H, W:2 * W] = out["depth"][j]
        host.append(G.count(canvas, depth_of(c), g["K"][c], float(g["delta"][c])))
    mv = torch.from_numpy(np.stack([255 * h["mask_visib"].astype(np.uint8) for h in host])).to(DEV)
    mf = torch.from_numpy(np.stack([255 * h["mask"].astype(np.uint8) for h in host])).to(DEV)
    from_numpy = targets.make_training_batch(frames, mv, mf, R, t, K, [h["bbox_visib"] for h in host], pts, is_train=False, img_index=rows)
    assert len(from_device) == len(from_numpy) == 11
    for a, b in zip(from_device, from_numpy):
        assert torch.equal(a, b)
    assert from_device[2].any() and from_device[1].any() and from_device[7].any()       # the crops' masks and the labels are not empty
