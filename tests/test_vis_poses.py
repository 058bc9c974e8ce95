"""Row N18 (poses drawn over the photograph) on the CPU: the restatement of tests/vis_stages.py EQUALS every picture the reference's
own vis_object_poses saved (tests/golden/vis_poses.npz, made by tests/golden/make_golden_vis_poses.py); the host half of
checkerpose_amd/vis.py (select_estimates, the grouping and the vis_name keys of the two scripts, the refusals); the entry points'
argument checks with fake pointers, both scratch queries, the library version."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from checkerpose_amd import scene, vis
from tests import vis_stages as VS
from tests.common import GOLDEN

_G = {}


def golden():
    """(npz, meta) loaded once"""
    if not _G:
        z = np.load(os.path.join(GOLDEN, "vis_poses.npz"))
        _G["z"], _G["meta"] = z, json.loads(bytes(z["meta"]).decode())
    return _G["z"], _G["meta"]


def case(z, ci, key):
    return z["c%02d_%s" % (ci, key)]


def test_fixture_covers_what_the_issue_lists():
    z, meta = golden()
    assert len(meta) >= 12
    names = " ".join(m["name"] for m in meta)
    for word in ("overlap", "tie", "black", "nopixel", "border", "saturate", "none", "48x40", "33x31", "resolve", "sum"):
        assert word in names, word
    assert sum(m["dd"] for m in meta) >= 4
    assert os.path.getsize(os.path.join(GOLDEN, "vis_poses.npz")) < (1 << 20)
    for ci, m in enumerate(meta):
        if m["dd"]:
            ren = VS.compose(case(z, ci, "frame"), case(z, ci, "m_rgb"), case(z, ci, "m_depth"))["ren_depth"]
            dd, valid = VS.dd_of(ren, case(z, ci, "depth"))
            assert VS.distinct_dd(ren, case(z, ci, "depth")) >= 3
            assert (case(z, ci, "depth") == 0).any()                                   # sensor depth with zeros
            assert (dd[valid] < 15).any() and (dd[valid] > 15).any() and (dd[valid] == 15).any()


def test_restatement_equals_every_recorded_picture():
    z, meta = golden()
    for ci, m in enumerate(meta):
        r = VS.compose(case(z, ci, "frame"), case(z, ci, "m_rgb"), case(z, ci, "m_depth"), resolve=m["resolve"])
        assert np.array_equal(r["vis"], case(z, ci, "vis")), m["name"]
        assert r["boxes"].shape == (m["n"], 4)
        if m["dd"]:
            pic, stats, ok = VS.depth_diff(r["ren_depth"], case(z, ci, "depth"))
            assert ok == 1 and np.array_equal(pic, case(z, ci, "dd_vis")), m["name"]
            assert np.array_equal(stats[:2], case(z, ci, "dd_minmax")), m["name"]


def test_restatement_edge_rules():
    z, meta = golden()
    by = {m["name"]: i for i, m in enumerate(meta)}
    ci = by["tie_resolve_48x40"]                            # of two equal depths the earlier pose keeps the pixel
    r = VS.compose(case(z, ci, "frame"), case(z, ci, "m_rgb"), case(z, ci, "m_depth"))
    both = (case(z, ci, "m_depth")[0] > 0) & (case(z, ci, "m_depth")[1] > 0)
    assert both.any() and np.array_equal(r["ren_rgb"][both], case(z, ci, "m_rgb")[0][both])
    ci = by["black_resolve_48x40"]                          # a black surface occludes but has no box
    r = VS.compose(case(z, ci, "frame"), case(z, ci, "m_rgb"), case(z, ci, "m_depth"))
    assert r["boxes"][1].tolist() == [-1, -1, -1, -1] and (r["ren_rgb"][case(z, ci, "m_depth")[1] > 0] == 0).all()
    ci = by["saturate_sum_48x40"]
    r = VS.compose(case(z, ci, "frame"), case(z, ci, "m_rgb"), case(z, ci, "m_depth"), resolve=False)
    assert (case(z, ci, "m_rgb").astype(np.int64).sum(0) > 255).any() and r["ren_rgb"].max() == 255
    ci = by["border_resolve_33x31"]                         # a box covering the frame, one on the border, one of a single pixel
    r = VS.compose(case(z, ci, "frame"), case(z, ci, "m_rgb"), case(z, ci, "m_depth"))
    assert r["boxes"][1].tolist() == [0, 0, 32, 30] and r["boxes"][2].tolist() == [32, 30, 0, 0]
    ci = by["none_resolve_48x40"]
    r = VS.compose(case(z, ci, "frame"), case(z, ci, "m_rgb"), case(z, ci, "m_depth"))
    assert np.array_equal(r["vis"], case(z, ci, "frame") // 2) and not r["ren_depth"].any()
    # fewer than three distinct differences: no picture
    ren = np.zeros((4, 5), dtype=np.float32)
    ren[1:3, 1:4] = 500.0
    pic, stats, ok = VS.depth_diff(ren, np.full((4, 5), 490.0, dtype=np.float32))
    assert ok == 0 and not pic.any() and stats.tolist() == [10.0, 10.0, 10.0]
    pic, stats, ok = VS.depth_diff(ren, np.zeros((4, 5), dtype=np.float32))
    assert ok == 0 and np.isnan(stats).all()


def _est(im_id, obj_id, score, tag):
    return {"im_id": im_id, "obj_id": obj_id, "score": score, "R": np.eye(3), "t": np.array([0.0, 0.0, 500.0 + tag]), "tag": tag}


def test_select_estimates_sorts_stably_and_cuts():
    ests = [_est(3, 5, 0.5, 0), _est(3, 5, 0.9, 1), _est(3, 5, 0.5, 2), _est(3, 2, 0.1, 3), _est(1, 5, 0.7, 4), _est(3, 5, 0.9, 5), _est(3, 2, 0.4, 6)]
    tags = lambda sel: {im: {o: [e["tag"] for e in v] for o, v in d.items()} for im, d in sel.items()}      # noqa: E731
    assert tags(vis.select_estimates(ests, n_top=0)) == {3: {5: [1, 5, 0, 2], 2: [6, 3]}, 1: {5: [4]}}           # ties keep input order
    assert tags(vis.select_estimates(ests, n_top=1)) == {3: {5: [1], 2: [6]}, 1: {5: [4]}}
    assert tags(vis.select_estimates(ests, n_top=3)) == {3: {5: [1, 5, 0], 2: [6, 3]}, 1: {5: [4]}}
    scene_gt = {3: [{"obj_id": 5}, {"obj_id": 5}, {"obj_id": 7}], 1: [{"obj_id": 5}]}
    assert tags(vis.select_estimates(ests, n_top=-1, scene_gt=scene_gt)) == {3: {5: [1, 5], 2: []}, 1: {5: [4]}}
    assert list(vis.select_estimates(ests, n_top=0).keys()) == [3, 1] and list(vis.select_estimates(ests, n_top=0)[3].keys()) == [5, 2]
    with pytest.raises(ValueError):
        vis.select_estimates(ests, n_top=-1)
    with pytest.raises(ValueError):
        vis.select_estimates(ests, n_top=-2)
    assert vis.select_estimates([], n_top=1) == {}


def test_scripts_group_poses_and_name_pictures(monkeypatch):
    """vis_est_poses / vis_gt_poses make ONE vis_poses call; its arguments and the keys of the result (no device: vis_poses is replaced)"""
    calls = []

    def fake(R, t, cam_K, meshes, frames, image_ids=None, mesh_ids=None, surf_colors=None, **kw):
        calls.append(dict(R=R, t=t, K=cam_K, frames=frames, image_ids=list(image_ids), mesh_ids=list(mesh_ids), surf=surf_colors, kw=kw))
        n_img, P = frames.shape[0], len(image_ids)
        return {"vis": torch.arange(n_img)[:, None, None, None].expand(n_img, 4, 6, 3), "ren_rgb": torch.zeros(n_img, 4, 6, 3),
                "ren_depth": torch.zeros(n_img, 4, 6), "boxes": torch.arange(P)[:, None].expand(P, 4), "ok": torch.ones(P)}

    monkeypatch.setattr(vis, "vis_poses", fake)
    ests = [_est(3, 5, 0.5, 0), _est(3, 5, 0.9, 1), _est(3, 2, 0.1, 3), _est(1, 5, 0.7, 4)]
    cam = {1: {"cam_K": np.eye(3) * 2, "depth_scale": 0.5}, 3: {"cam_K": np.eye(3) * 3, "depth_scale": 1.0}}
    frames = {1: np.full((4, 6, 3), 10, dtype=np.uint8), 3: np.full((4, 6, 3), 30, dtype=np.uint8)}
    palette = [[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]]
    obj_index = {2: 0, 5: 1}
    out = vis.vis_est_poses(ests, cam, frames, "meshes", obj_index, palette=palette, n_top=0, device="cpu")
    assert list(out.keys()) == [(3, 5), (3, 2), (1, 5)] and len(calls) == 1
    c = calls[0]
    assert c["image_ids"] == [0, 0, 1, 2] and c["mesh_ids"] == [1, 1, 0, 1]
    assert c["t"].reshape(-1, 3)[:, 2].tolist() == [501.0, 500.0, 503.0, 504.0]                  # score order inside (3, 5)
    assert c["frames"][:, 0, 0, 0].tolist() == [30, 30, 10] and c["K"][:, 0, 0].tolist() == [3.0, 3.0, 2.0]
    assert np.array_equal(c["surf"], np.array([palette[1], palette[1], palette[1], palette[1]]))  # (5 - 1) % 3 == 1 == (2 - 1) % 3
    assert out[(3, 5)]["boxes"][:, 0].tolist() == [0, 1] and out[(1, 5)]["boxes"][:, 0].tolist() == [3] and int(out[(3, 2)]["vis"][0, 0, 0]) == 1
    calls.clear()
    out = vis.vis_est_poses(ests, cam, frames, "meshes", obj_index, vis_per_obj_id=False, n_top=1, device="cpu", resolve_visib=False,
                            depth={1: np.ones((4, 6)), 3: np.ones((4, 6))}, depth_diff=True)
    assert list(out.keys()) == [3, 1] and calls[0]["image_ids"] == [0, 0, 1] and calls[0]["surf"] is None
    assert calls[0]["kw"]["resolve_visib"] is False and calls[0]["kw"]["depth_diff"] is True
    assert calls[0]["kw"]["depth"][:, 0, 0].tolist() == [1.0, 0.5]                                # depth * depth_scale
    calls.clear()
    gts = {7: [{"obj_id": 5, "cam_R_m2c": np.eye(3), "cam_t_m2c": [0, 0, 600.0]}, {"obj_id": 2, "cam_R_m2c": np.eye(3), "cam_t_m2c": [0, 0, 700.0]}],
           4: [{"obj_id": 2, "cam_R_m2c": np.eye(3), "cam_t_m2c": [0, 0, 800.0]}]}
    cam = {4: {"cam_K": np.eye(3)}, 7: {"cam_K": np.eye(3)}}
    frames = {4: np.zeros((4, 6, 3), dtype=np.uint8), 7: np.zeros((4, 6, 3), dtype=np.uint8)}
    out = vis.vis_gt_poses(gts, cam, frames, "meshes", obj_index, palette=palette, device="cpu")
    assert list(out.keys()) == [4, 7] and calls[0]["image_ids"] == [0, 1, 1] and calls[0]["mesh_ids"] == [0, 1, 0]
    assert calls[0]["kw"]["shading"] == "flat"
    calls.clear()
    out = vis.vis_gt_poses(gts, cam, frames, "meshes", obj_index, gt_ids=[1], device="cpu")
    assert calls[0]["image_ids"] == [1] and calls[0]["mesh_ids"] == [0] and out[4]["boxes"].shape[0] == 0
    with pytest.raises(ValueError):
        vis.vis_gt_poses(gts, cam, frames, "meshes", {5: 1}, device="cpu")                       # an object without a mesh
    with pytest.raises(ValueError):
        vis.vis_gt_poses(gts, cam, {4: frames[4], 7: np.zeros((5, 6, 3), dtype=np.uint8)}, "meshes", obj_index, device="cpu")
    with pytest.raises(ValueError):
        vis.vis_est_poses(ests, cam, frames, "meshes", obj_index, image_ids=[0], device="cpu")
    assert vis.vis_est_poses([], cam, frames, "meshes", obj_index, device="cpu") == {}


def test_package_names_and_csr():
    import checkerpose_amd
    for n in ("vis_poses", "depth_diff_vis", "select_estimates", "vis_est_poses", "vis_gt_poses"):
        assert getattr(checkerpose_amd, n) is getattr(vis, n)
    ids, off, order = scene.group_by_image([2, 0, 2, 3, 0, 2], 6, 5)
    assert ids.tolist() == [2, 0, 2, 3, 0, 2] and off.tolist() == [0, 2, 2, 5, 6, 6] and order.tolist() == [1, 4, 0, 2, 5, 3]      # stable
    assert scene.group_by_image(None, 3, 1)[1].tolist() == [0, 3] and scene.group_by_image(None, 3, 3)[2].tolist() == [0, 1, 2]


def _mesh_set():
    from checkerpose_amd import metric
    from tests import render_rgb_stages as RS
    m = RS.meshes()
    return metric.MeshSet.from_arrays([m["box"][0]], faces=[m["box"][1]], colors=[m["box"][2]], normals=[m["box"][3]], diameters=[100.0])


def test_refusals_are_value_errors_and_there_is_no_cpu_fallback():
    ms = _mesh_set()
    R, t, K = np.eye(3)[None].repeat(2, 0), np.array([[0.0, 0.0, 500.0]] * 2), np.array([[500.0, 0, 20], [0, 500.0, 16], [0, 0, 1]])
    fr = torch.zeros((2, 32, 40, 3), dtype=torch.uint8)
    for kw in (dict(shading="gouraud"), dict(frames=fr.float()), dict(frames=fr[0]), dict(frames=fr[..., :2]), dict(image_ids=[0, 2]),
               dict(image_ids=[0, -1]), dict(image_ids=[0]), dict(surf_colors=[[0.5, float("nan"), 0.5]] * 2), dict(surf_colors=[[0.1, 0.2, 0.3]] * 3),
               dict(depth_diff=True), dict(depth_diff=True, depth=torch.zeros(2, 32, 41)), dict(depth_diff=True, depth=torch.zeros(3, 32, 40)),
               dict(box_color=(0.3, float("inf"), 0.3)), dict(ambient_weight=float("nan")), dict(light_cam_pos=(0, 0)), dict(meshes="box")):
        a = dict(R=R, t=t, cam_K=K, meshes=ms, frames=fr)
        a.update(kw)
        with pytest.raises(ValueError):
            vis.vis_poses(**a)
    with pytest.raises(ValueError):
        vis.vis_poses(R[:0], t[:0], K, ms, fr)                                                    # no poses
    with pytest.raises(ValueError):
        vis.vis_poses(R, t, K, ms, torch.zeros((3, 32, 40, 3), dtype=torch.uint8))                # 3 frames, 2 poses, no image_ids
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vis.vis_poses(R, t, K, ms, fr)
    for ren, dep in ((torch.zeros(2, 8, 9), torch.zeros(2, 8, 10)), (torch.zeros(2, 8, 9), torch.zeros(8)), (torch.zeros(9), torch.zeros(9)),
                     (torch.zeros(2, 8, 9), "depth")):
        with pytest.raises(ValueError):
            vis.depth_diff_vis(ren, dep)
    with pytest.raises(ValueError):
        vis.depth_diff_vis(torch.zeros(2, 8, 9), torch.zeros(8, 9), delta=float("nan"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vis.depth_diff_vis(torch.zeros(2, 8, 9), torch.zeros(8, 9))


def test_entry_points_refuse_bad_arguments_before_any_launch(lib):
    """fake, never-dereferenced device pointers; the CSR copies are real host memory (they are read)"""
    assert lib.cp_version() >= 219
    A, P, n_img = 0x10000, 5, 3
    off, order = (C.c_int32 * 4)(0, 2, 2, 5), (C.c_int32 * 5)(0, 3, 1, 2, 4)
    vec = (C.c_double * 3)(0.3, 0.3, 0.3)
    names = ("poses", "K", "ks", "verts", "v_off", "faces", "f_off", "M", "mesh_ids", "colors", "normals", "surf", "iop", "img_off", "order", "off_h", "order_h",
             "frames", "shading", "amb", "light", "box", "resolve", "draw", "H", "W", "P", "I", "Vmax", "vis", "ren_rgb", "ren_depth", "boxes", "ok", "scratch")
    good = dict(zip(names, (A, A, 0, A, A, A, A, 2, A, A, A, A, A, A, A, off, order, A, 1, 0.5, vec, vec, 1, 1, 40, 48, P, n_img, 12, A, A, A, A, A, A)))

    def call(**kw):
        a = dict(good)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = lib.cp_vis_poses(None, *[a[n] for n in names])
        assert lib.cp_kernel_log() == b"", kw
        return rc

    for n in ("poses", "K", "verts", "v_off", "faces", "f_off", "iop", "img_off", "order", "off_h", "order_h", "frames", "light", "box", "vis",
              "ren_rgb", "ren_depth", "boxes", "ok", "scratch", "normals", "mesh_ids"):
        assert call(**{n: None}) == -1, n
    for kw in (dict(P=0), dict(I=0), dict(M=0), dict(Vmax=0), dict(H=0), dict(W=-1), dict(ks=4), dict(shading=2), dict(resolve=2), dict(draw=-1),
               dict(amb=float("nan")), dict(amb=float("inf")), dict(light=(C.c_double * 3)(0, float("nan"), 0)), dict(box=(C.c_double * 3)(0, 0, float("inf")))):
        assert call(**kw) == -1, kw
    for kw in (dict(scratch=A + 8), dict(poses=A + 4), dict(surf=A + 4), dict(verts=A + 2), dict(ren_depth=A + 2), dict(boxes=A + 1), dict(iop=A + 2)):
        assert call(**kw) == -3, kw
    for bad in ((1, 2, 2, 5), (0, 2, 2, 4), (0, 3, 2, 5), (0, 2, 2, 6)):
        assert call(off_h=(C.c_int32 * 4)(*bad)) == -1, bad
    for bad in ((0, 3, 1, 2, 5), (0, -1, 1, 2, 4)):
        assert call(order_h=(C.c_int32 * 5)(*bad)) == -1, bad
    assert call(W=1 << 24) == -4
    assert call(H=4096, W=4096, I=64, off_h=(C.c_int32 * 65)(*([0] + [P] * 64))) == -4           # 3 I H W >= 2^31
    assert lib.cp_vis_poses_scratch_bytes(5, 12, 3) == 5 * 48 * 4 + 4 * 5 * 12 * 16
    assert lib.cp_vis_poses_scratch_bytes(0, 12, 3) == 0 and lib.cp_vis_poses_scratch_bytes(5, -1, 3) == 0 and lib.cp_vis_poses_scratch_bytes(5, 12, 0) == 0

    def dd(**kw):
        a = dict(ren=A, depth=A, ids=A, nd=2, delta=15.0, s=0.8, H=40, W=48, I=3, out=A, stats=A, ok=A, scratch=A)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = lib.cp_depth_diff_vis(None, *[a[n] for n in ("ren", "depth", "ids", "nd", "delta", "s", "H", "W", "I", "out", "stats", "ok", "scratch")])
        assert lib.cp_kernel_log() == b"", kw
        return rc

    for n in ("ren", "depth", "out", "stats", "ok", "scratch", "ids"):
        assert dd(**{n: None}) == -1, n                                                           # (no ids: 2 depth images for 3 renders)
    for kw in (dict(nd=0), dict(H=0), dict(W=0), dict(I=0), dict(delta=float("nan")), dict(s=0.0), dict(s=float("nan")), dict(s=-0.8)):
        assert dd(**kw) == -1, kw
    for kw in (dict(ren=A + 2), dict(depth=A + 1), dict(ids=A + 2), dict(stats=A + 4), dict(scratch=A + 8)):
        assert dd(**kw) == -3, kw
    assert dd(H=32768, W=32768, I=1) == -4 and dd(H=1024, W=1024, I=1 << 14) == -4
    assert lib.cp_depth_diff_vis_scratch_bytes(3, 40, 48) == 96 + 96 + 48 and lib.cp_depth_diff_vis_scratch_bytes(1, 31, 33) == 32 + 32 + 16
    assert lib.cp_depth_diff_vis_scratch_bytes(0, 40, 48) == 0 and lib.cp_depth_diff_vis_scratch_bytes(3, 40, 0) == 0
