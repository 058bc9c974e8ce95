"""Row N10 (BOP ground-truth info and masks), host side.  tests/golden/gt_info.npz holds what the REFERENCE's own scripts
calc_gt_info.py and calc_gt_masks.py saved when they were run whole (runpy) with a stub renderer handing them the float64 oracle's
depth on the 3W x 3H canvas (tests/golden/make_golden_gt_info.py).  The stages of tests/gt_info_stages.py are checked here against
those records -- they are the yardsticks of tests/test_gpu_gt_info.py, which cannot read the reference:

  count(...)           reproduces every recorded count, both boxes, visib_fract (the same bits) and both masks EXACTLY;
  its mutations        'bop18', px_count_all on the frame, px_count_valid over the canvas mask, bbox_obj gated on px_count_all, box
                       width + 1, clipped bbox_obj, the fp64 difference against delta: each is reported against the fixture;
  oracle_canvas(...)   its nominal depth equals the recorded depth_gt_large bit for bit; at most 5 % of a case's covered canvas
                       pixels are undecided (the largest share is 0.0191); the recorded results pass the interval check."""
import ctypes as C
import inspect
import json
import zlib

import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, gt_info as GI
from tests import gt_info_stages as G
from tests import vsd_stages as S
from tests.common import golden
from tests.test_vsd_error import fixture as vsd_fixture

_CACHE = {}


def fixture():
    """(golden arrays, {mesh name: (verts, faces)}) -- built once, never modified"""
    if "g" not in _CACHE:
        g = golden("gt_info")
        meshes = vsd_fixture()[1]
        for i, name in enumerate(g["mesh_names"]):
            v, f = meshes[str(name)]
            assert str(name) == "hull" or zlib.crc32(v.tobytes() + f.tobytes()) == int(g["mesh_crc"][i]), name
        _CACHE["g"] = (g, meshes)
    return _CACHE["g"]


def n_cases():
    return len(fixture()[0]["ok"])


def size_of(c):
    g, _ = fixture()
    return int(g["W"][c]), int(g["H"][c])


def depth_of(c):
    g, _ = fixture()
    return g["depth_%d" % int(g["image"][c])]


def recorded(c):
    g, _ = fixture()
    out = {k: g[k][c] for k in G.INFO_KEYS}
    if g["ok"][c]:
        out["mask"], out["mask_visib"] = G.unpack(g["mask_%d" % c], size_of(c)), G.unpack(g["visib_%d" % c], size_of(c))
    return out


def oracle(c):
    """oracle_canvas of fixture case c: computed once, shared by every test that needs it"""
    if ("o", c) not in _CACHE:
        g, meshes = fixture()
        v, f = meshes[str(g["mesh_names"][g["mesh"][c]])]
        _CACHE[("o", c)] = G.oracle_canvas(g["R"][c], g["t"][c], g["K"][c], v, f, size_of(c))
    return _CACHE[("o", c)]


def intervals(c):
    if ("iv", c) not in _CACHE:
        g, _ = fixture()
        _CACHE[("iv", c)] = G.intervals(oracle(c), depth_of(c), g["K"][c], float(g["delta"][c]), size_of(c))
    return _CACHE[("iv", c)]


def test_fixture_covers_what_the_issue_lists():
    g, meshes = fixture()
    n = n_cases()
    ok = g["ok"]
    assert n >= 24 and (~ok).sum() == 1 and not ok[-1]
    names = {str(g["mesh_names"][m]) for m in g["mesh"]}
    assert {"triangle", "box", "halfbox", "ico80", "ico1280", "ico20480", "torus", "zeroarea"} <= names
    sizes = {size_of(c) for c in range(n)}
    assert {(33, 31), (160, 120), (64, 64)} <= sizes and all(33 <= w <= 160 and 31 <= h <= 120 for w, h in sizes)
    assert all(w % 32 or h % 32 for w, h in sizes if (w, h) != (64, 64)) and set(g["delta"].tolist()) == {5.0, 15.0}
    assert len(set(g["kgroup"].tolist())) >= 3
    a, v, vis = g["px_count_all"], g["px_count_valid"], g["px_count_visib"]
    bo, bv = g["bbox_obj"], g["bbox_visib"]
    assert ((a > 0) & (vis == a) & (bo[:, 0] >= 0) & (bo == bv).all(1)).any()                     # wholly in the frame
    assert (bo[ok & (vis > 0), 0] < 0).any() and (bo[ok & (vis > 0), 1] < 0).any()                  # straddling the left / top edge
    W, H = g["W"], g["H"]
    sel = ok & (vis > 0)
    assert (bo[sel, 0] + bo[sel, 2] >= W[sel]).any() and (bo[sel, 1] + bo[sel, 3] >= H[sel]).any()  # the right / bottom edge
    assert ((bo[:, 0] < 0) & (bo[:, 1] < 0) & (vis > 0)).any()                                      # a corner
    margin = [c for c in range(n) if ok[c] and a[c] > 0 and vis[c] == 0 and not (G.frame_of(g["large_%d" % c], size_of(c)) > 0).any()]
    assert margin and all(bo[c].tolist() == [-1] * 4 and bv[c].tolist() == [-1] * 4 and g["visib_fract"][c] == 0.0 for c in margin)
    assert any((g["large_%d" % c][:, 0] > 0).any() or (g["large_%d" % c][:, -1] > 0).any() for c in margin)     # cut by the canvas edge
    assert (ok & (a == 0)).any()                                                                    # wholly off the canvas
    assert any(ok[c] and vis[c] == 0 and v[c] == a[c] and a[c] > 0 for c in range(n))              # behind an occluder entirely
    assert any(ok[c] and 0 < vis[c] < a[c] and v[c] == a[c] for c in range(n))                     # ... partly
    assert any(ok[c] and vis[c] > v[c] > 0 for c in range(n))                                       # holes: visible, not valid
    assert any(ok[c] and (depth_of(c) == 0).all() and v[c] == 0 and vis[c] == a[c] > 0 for c in range(n))      # all-zero depth
    im = g["image"][ok]
    assert (np.bincount(im) == 3).any()                                                             # three objects, one depth image
    one = [c for c in range(n) if a[c] == 1]
    assert one and bo[one[0], 2:].tolist() == [0, 0] and bv[one[0], 2:].tolist() == [0, 0] and vis[one[0]] == 1
    assert float(g["worst_undecided"]) <= 0.05


def test_counting_restatement_reproduces_the_scripts_exactly():
    g, _ = fixture()
    for c in range(n_cases() - 1):
        mine, rec = G.count(g["large_%d" % c], depth_of(c), g["K"][c], float(g["delta"][c])), recorded(c)
        assert G.same_info(mine, rec), (c, {k: mine[k] for k in G.INFO_KEYS}, {k: rec[k] for k in G.INFO_KEYS})
        assert np.array_equal(mine["mask"], rec["mask"]) and np.array_equal(mine["mask_visib"], rec["mask_visib"]), c
        assert type(mine["px_count_all"]) is int and type(mine["visib_fract"]) is float


def test_each_mutation_of_the_counting_is_reported_against_the_fixture():
    g, _ = fixture()
    hit = {m: 0 for m in G.MUTATIONS}
    for c in range(n_cases() - 1):
        rec = recorded(c)
        for m in G.MUTATIONS:
            mine = G.count(g["large_%d" % c], depth_of(c), g["K"][c], float(g["delta"][c]), mutation=m)
            hit[m] += not (G.same_info(mine, rec) and np.array_equal(mine["mask_visib"], rec["mask_visib"]))
    print("mutations caught (cases):", hit)
    assert all(hit[m] >= 1 for m in G.MUTATIONS), hit
    assert hit["all_on_frame"] >= 5 and hit["clip_obj"] >= 5 and hit["plus_one"] >= 15 and hit["bop18"] >= 3 and hit["gate_on_all"] >= 2


def test_oracle_equals_the_recorded_canvas_and_the_records_pass_the_interval_check():
    g, _ = fixture()
    worst = 0.0
    for c in range(n_cases() - 1):
        o = oracle(c)
        assert o["d"].dtype == np.float32 and np.array_equal(o["d"], g["large_%d" % c]), c
        share = S.undecided_share(o)
        worst = max(worst, share)
        assert share <= 0.05 and share == float(g["undecided"][c]), (c, share)
        bad = G.check_against_intervals(recorded(c), intervals(c), size_of(c))
        assert not bad, (c, bad)
        wrong = dict(recorded(c))                                                       # the check reports a moved box and a flipped mask
        if wrong["px_count_visib"] > 20:
            wrong["bbox_visib"] = [wrong["bbox_visib"][0] + 3] + list(wrong["bbox_visib"][1:])
            assert G.check_against_intervals(wrong, intervals(c), size_of(c))
            wrong = dict(recorded(c))
            wrong["mask"] = ~wrong["mask"]
            assert G.check_against_intervals(wrong, intervals(c), size_of(c))
    print("largest undecided share of the covered canvas pixels: %.4f" % worst)
    assert worst == float(g["worst_undecided"])
    with pytest.raises(ValueError):                                                     # the pose behind the camera is outside the render rule
        oracle(n_cases() - 1)


def test_argument_checks_without_a_device():
    from tests.test_vsd_error import mesh_set
    ms = mesh_set()
    R, t = torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3, 1, dtype=torch.float64)
    d = np.zeros((8, 8), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GI.gt_info(R, t, np.eye(3), ms, d, mesh_ids=[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GI.gt_info_from_depth(torch.zeros(1, 24, 24), d, np.eye(3))
    sig = inspect.signature(GI.gt_info)
    assert list(sig.parameters) == ["R", "t", "cam_K", "meshes", "depth", "image_ids", "mesh_ids", "delta", "return_masks", "return_depth"]
    assert sig.parameters["delta"].default == 15.0 and sig.parameters["return_masks"].default is False
    assert list(inspect.signature(GI.gt_info_from_depth).parameters) == ["depth_gt_large", "depth", "cam_K", "image_ids", "delta", "return_masks"]
    assert list(inspect.signature(GI.scene_gt_info).parameters)[:6] == ["scene_gt", "scene_camera", "depths", "meshes", "obj_index", "delta"]
    for fn in (GI.gt_info, GI.scene_gt_info):
        assert "make_training_batch" in fn.__doc__


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    p = C.c_void_p(4096)                                    # fake, aligned; never dereferenced: every call returns before a launch

    def gi(poses=p, K=p, ks=9, verts=p, voff=p, faces=p, foff=p, M=2, ids=p, depth=p, img=p, n_img=2, H=48, W=64, delta=15.0, B=2, Vmax=8,
           cnt=p, fr=p, box=p, ok=p, mask=None, visib=None, dgt=None, scr=p):
        return lib.cp_gt_info(None, poses, K, ks, verts, voff, faces, foff, M, ids, depth, img, n_img, H, W, delta, B, Vmax, cnt, fr, box, ok,
                              mask, visib, dgt, scr)

    for name in ("poses", "K", "verts", "voff", "faces", "foff", "depth", "cnt", "fr", "box", "ok", "scr"):
        assert gi(**{name: None}) == -1, name
    assert gi(B=0) == -1 and gi(M=0) == -1 and gi(Vmax=0) == -1 and gi(H=0) == -1 and gi(W=-1) == -1 and gi(n_img=0) == -1
    assert gi(ks=3) == -1 and gi(delta=float("nan")) == -1
    assert gi(ids=None) == -1 and gi(img=None) == -1                                    # several meshes / images need ids
    assert gi(mask=p) == -1 and gi(visib=p) == -1                                       # both masks or neither
    assert gi(poses=C.c_void_p(4100)) == -3 and gi(scr=C.c_void_p(4104)) == -3 and gi(faces=C.c_void_p(4098)) == -3
    assert gi(dgt=C.c_void_p(4098)) == -3 and gi(box=C.c_void_p(4097)) == -3 and gi(fr=C.c_void_p(4100)) == -3
    assert gi(mask=C.c_void_p(4097), visib=C.c_void_p(4099), B=1 << 20, H=480, W=640) == -4         # uint8 images: any address; 2^20 x 2700 tiles

    def fd(large=p, K=p, ks=0, depth=p, img=p, n_img=2, H=48, W=64, delta=15.0, B=2, cnt=p, fr=p, box=p, ok=p, mask=None, visib=None, scr=p):
        return lib.cp_gt_info_from_depth(None, large, K, ks, depth, img, n_img, H, W, delta, B, cnt, fr, box, ok, mask, visib, scr)

    for name in ("large", "K", "depth", "cnt", "fr", "box", "ok", "scr"):
        assert fd(**{name: None}) == -1, name
    assert fd(B=0) == -1 and fd(ks=5) == -1 and fd(img=None) == -1 and fd(H=0) == -1 and fd(mask=p) == -1 and fd(delta=float("nan")) == -1
    assert fd(large=C.c_void_p(4098)) == -3 and fd(scr=C.c_void_p(4100)) == -3 and fd(B=1 << 20, H=480, W=640) == -4
    assert lib.cp_gt_info_scratch_bytes(0, 8) == 0 and lib.cp_gt_info_scratch_bytes(1, -1) == 0
    for B, V in ((1, 0), (1, 3), (2, 10242), (256, 10242)):
        n = lib.cp_gt_info_scratch_bytes(B, V)
        assert n % 16 == 0 and n >= 128 * B + 16 * B * V
    assert lib.cp_version() >= 211
    for name in ("cp_gt_info", "cp_gt_info_from_depth", "cp_gt_info_scratch_bytes"):
        assert name in _abi.SIGNATURES


def test_scene_gt_info_structure_through_a_stubbed_device_call(tmp_path):
    g, _ = fixture()
    idx = [c for c in range(n_cases() - 1) if g["scene"][c] == 1 and g["kgroup"][c] == 0]
    images = sorted({int(g["image"][c]) for c in idx})
    scene_gt = {7 * im: [{"obj_id": int(g["mesh"][c]) + 1, "cam_R_m2c": g["R"][c], "cam_t_m2c": g["t"][c].reshape(3, 1)} for c in idx if g["image"][c] == im]
                for im in images}
    scene_camera = {7 * im: {"cam_K": g["K"][idx[0]], "depth_scale": 0.5} for im in images}
    depths = {7 * im: g["depth_%d" % im] * np.float32(2.0) for im in images}
    order = [c for im in images for c in idx if g["image"][c] == im]
    seen = {}

    def call(R, t, K, meshes, depth, image_ids=None, mesh_ids=None, delta=15.0, return_masks=False):
        seen.update(R=R, t=t, K=K, depth=depth, image_ids=image_ids, mesh_ids=mesh_ids, delta=delta, meshes=meshes)
        cols = {k: torch.from_numpy(np.stack([np.asarray(g[k][c]) for c in order])) for k in GI.KEYS}
        cols["px_count_all"] = cols["px_count_all"].to(torch.int32)
        if return_masks:
            cols["mask"] = torch.from_numpy(np.stack([255 * recorded(c)["mask"].astype(np.uint8) for c in order]))
            cols["mask_visib"] = torch.from_numpy(np.stack([255 * recorded(c)["mask_visib"].astype(np.uint8) for c in order]))
        return cols

    obj_index = {m + 1: m for m in range(len(S.MESH_NAMES))}
    info = GI.scene_gt_info(scene_gt, scene_camera, depths, "meshes", obj_index, delta=15.0, device="cpu", _call=call)
    assert seen["meshes"] == "meshes" and tuple(seen["R"].shape) == (len(order), 3, 3) and tuple(seen["t"].shape) == (len(order), 3, 1)
    assert seen["mesh_ids"] == [int(g["mesh"][c]) for c in order] and seen["image_ids"] == [images.index(int(g["image"][c])) for c in order]
    assert seen["depth"].dtype == np.float32 and np.array_equal(seen["depth"], np.stack([g["depth_%d" % im] for im in images]))   # depth_scale applied
    assert tuple(seen["K"].shape) == (len(order), 3, 3) and seen["delta"] == 15.0
    assert sorted(info) == [7 * im for im in images]
    j = 0
    for im in images:
        assert len(info[7 * im]) == len(scene_gt[7 * im])
        for e in info[7 * im]:
            c = order[j]
            j += 1
            assert sorted(e) == sorted(G.INFO_KEYS)
            assert all(type(e[k]) is int for k in G.INFO_KEYS[:3]) and type(e["visib_fract"]) is float
            assert all(type(x) is int for x in e["bbox_obj"] + e["bbox_visib"]) and len(e["bbox_obj"]) == 4
            assert G.same_info(e, recorded(c)), c
    both, masks = GI.scene_gt_info(scene_gt, scene_camera, depths, "meshes", obj_index, device="cpu", _call=call, return_masks=True)
    assert both == info and sorted(masks) == sorted((7 * int(g["image"][c]), gt) for im in images for gt, c in enumerate(c for c in idx if g["image"][c] == im))
    m, mv = masks[(7 * images[1], 0)]
    assert m.dtype == np.uint8 and set(np.unique(m)) <= {0, 255} and m.shape == (45, 67)
    path = tmp_path / "scene_gt_info.json"
    GI.save_scene_gt_info(str(path), info)
    back = json.loads(path.read_text())
    assert sorted(back, key=int) == [str(7 * im) for im in images] and back[str(7 * images[0])] == info[7 * images[0]]
    assert path.read_text().count("\n") == len(images) + 1                               # one line per image
    with pytest.raises(ValueError, match="obj_index"):
        GI.scene_gt_info(scene_gt, scene_camera, depths, "meshes", {}, device="cpu", _call=call)
    assert GI.scene_gt_info({3: []}, {3: {"cam_K": np.eye(3)}}, {}, "meshes", {}, _call=call) == {3: []}
