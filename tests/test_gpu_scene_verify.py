"""GPU: row N31 on the device.  verify_scene_mask over the committed cases of tests/scene_verify_stages.py -- two small frames ((96, 80):
3 x 3 tiles; (70, 50): a partial last word), occluding, interpenetrating and identical poses, a fully hidden pose under an empty and a
non-empty visible mask, exactly 32 and 33 poses in one image, interleaved images, per-pose intrinsics, several meshes, shared and permuted
mask ids, poses partly and wholly off the frame, every way of being uncounted in front of a counted pose, delta = 0 and a huge delta --
against the numpy rule applied to the device's own metric.render_depth of the same poses: counts, boxes, ok, slot and planes EQUAL, the
five quotients the same bits; against render_scene's planes; against verify_poses_mask with every pose alone; the identities (alone /
batches / permuted images, planes); select_poses; the refusals; the caller."""
import numpy as np
import pytest
import torch

from tests import icp_stages as I
from tests import scene_verify_stages as SV

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_MS, _RUNS = {}, {}
KEYS = ("counts", "box", "box_pvis", "ok", "slot") + SV.QUOTIENTS


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _meshset(case):
    from checkerpose_amd.metric import MeshSet
    if case.meshes not in _MS:
        v, f = I.mesh_arrays(case.meshes)
        _MS[case.meshes] = MeshSet.from_arrays(v, diameters=I.diameters(case.meshes), faces=f)
    return _MS[case.meshes]


def _ids(ids, bound):
    """host ids are checked by the wrapper; ids out of range travel as a resident tensor and reach the kernel"""
    ids = np.asarray(ids, np.int32)
    return _up(ids) if ((ids < 0) | (ids >= bound)).any() else ids


def _renders(case):
    """the device's own depth renders of the case's poses -> (P,H,W) float32 numpy (zeros for a pose that is not rendered)"""
    from checkerpose_amd import metric
    D = metric.render_depth(_up(case.R), _up(case.t), _up(case.K), _meshset(case), case.size, mesh_ids=_ids(case.mesh_ids, len(case.meshes)))
    return D.cpu().numpy()


def _packed(case):
    from checkerpose_amd import coco_eval
    key = ("packed", case.name)
    if key not in _RUNS:
        _RUNS[key] = (coco_eval.pack_masks(_up(case.full.astype(np.uint8))), coco_eval.pack_masks(_up(case.visible.astype(np.uint8))))
    return _RUNS[key]


def _args(case, idx=None, image_ids=None, n_images=None, **over):
    idx = np.arange(case.P) if idx is None else np.asarray(idx)
    full, vis = _packed(case)
    mids = case.mask_ids[idx] if case.mask_ids is not None else (None if len(idx) == case.P and (idx == np.arange(case.P)).all() else idx.astype(np.int32))
    n_img = case.n_images if n_images is None else n_images
    img = case.image_ids[idx] if image_ids is None else np.asarray(image_ids, np.int32)
    a = dict(R=_up(case.R[idx]), t=_up(case.t[idx]), cam_K=_up(case.K[idx] if case.K.ndim == 3 else case.K), meshes=_meshset(case), full=full,
             visible=vis, image_ids=_up(img) if np.bincount(np.clip(img, 0, None)).max() > SV.MAX_POSES else _ids(img, n_img), delta=case.delta, mask_ids=None if mids is None else _ids(mids, case.N),
             mesh_ids=_ids(case.mesh_ids[idx], len(case.meshes)), status=None if case.status is None else _up(case.status[idx]), n_images=n_img,
             return_planes=True)
    a.update(over)
    return a


def _device(case, idx=None, **over):
    """verify_scene_mask on the device -> dict of numpy arrays in scene_verify_stages.reference's layout"""
    from checkerpose_amd import postprocess as Q
    a = _args(case, idx, **over)
    res = Q.verify_scene_mask(**a)
    score, info = res[0], res[1]
    P = len(score)
    assert score.dtype == torch.float64 and tuple(score.shape) == (P,) and info["ok"].dtype == torch.bool and info["slot"].dtype == torch.int32
    assert all(info[k].dtype == torch.int32 and tuple(info[k].shape) == (P,) for k in SV.COUNTS)
    assert all(info[k].dtype == torch.float64 and tuple(info[k].shape) == (P,) for k in SV.QUOTIENTS[:4])
    assert all(info[k].dtype == torch.int32 and tuple(info[k].shape) == (P, 4) for k in ("box", "box_pvis"))
    out = dict(counts=np.stack([info[k].cpu().numpy() for k in SV.COUNTS], 1), box=info["box"].cpu().numpy(), box_pvis=info["box_pvis"].cpu().numpy(),
               ok=info["ok"].cpu().numpy(), slot=info["slot"].cpu().numpy(), score=score.cpu().numpy(), full_bits=None, visib_bits=None, choice=None)
    out.update({k: info[k].cpu().numpy() for k in SV.QUOTIENTS[:4]})
    if a["return_planes"]:
        W, H = case.size
        assert all(res[2][k].dtype == torch.int32 and tuple(res[2][k].shape) == (a["n_images"], H, W) for k in ("full_bits", "visib_bits"))
        out["full_bits"], out["visib_bits"] = res[2]["full_bits"].cpu().numpy(), res[2]["visib_bits"].cpu().numpy()
    if case.cand is not None and idx is None:
        out["choice"] = Q.select_poses(score.view(*case.cand), info["ok"].view(*case.cand)).cpu().numpy()
    return out


def _run(name):
    """a committed case on the device: (case, the device's renders, its outputs); computed once, left unchanged"""
    if name not in _RUNS:
        case = SV.make(name)
        _RUNS[name] = (case, _renders(case), _device(case))
    return _RUNS[name]


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _rows(out, rows):
    return {k: out[k][rows] for k in KEYS}


# ------------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name", list(SV.CASES))
def test_device_equals_the_rule(name):
    """counts, boxes, ok, slot, the planes and the choice EQUAL the numpy rule's on the device's own renders; the quotients bit for bit"""
    case, D, out = _run(name)
    want = SV.check_case(case, D, out, log=print)
    assert out["counts"].dtype == np.int32 and out["full_bits"].dtype == np.int32
    if name in ("occl_a", "occl_b_d0", "occl_b_d15", "mixed_b", "select_a", "crowd32_b"):
        assert len(SV.partly_hidden(case, D)) >= 1                                  # no pass from scenes without occlusion
    if name == "occl_a":
        assert 0 < out["counts"][1, 1] < out["counts"][1, 0] and out["counts"][2, 7] > 0 and out["iou"][2] > 0.95 and out["iou_vis"][2] < 0.8
    if name == "hidden_tie_a":
        assert out["counts"][2, 1] == out["counts"][3, 1] == 0 < out["counts"][2, 0] and np.isnan(out["score"][2]) and not out["ok"][2]
        assert out["score"][3] == 0.0 and out["ok"][3] and (out["counts"][:2, 1] == out["counts"][:2, 0]).all() and (out["counts"][:2, 0] > 0).all()
    if name == "occl_b_big":
        assert np.array_equal(out["counts"][:, 1], out["counts"][:, 0])
    if name == "crowd33_b":
        assert out["slot"][36] == 32 and not out["ok"][36] and out["counts"][36, :5].tolist() == [0] * 5 and D[36].any()
        assert _same(_rows(out, np.arange(36)), _rows(_run("crowd32_b")[2], np.arange(36)))
    if name == "uncounted_a":
        for b in range(1, 14, 2):
            assert _same(_rows(out, [b]), _rows(out, [14]), keys=tuple(k for k in KEYS if k != "slot")), b
        assert out["slot"].tolist() == [0, 1] * 6 + [-1, 0, 0] and not out["ok"][0:14:2].any()
    if want["choice"] is not None:
        assert out["choice"].tolist() == want["choice"].tolist() == SV.reference(case, SV.cpu_renders(case))["choice"].tolist() == [1, 1]


@pytest.mark.parametrize("name", ["occl_a", "occl_b_d15", "hidden_tie_a", "crowd32_b"])
def test_planes_equal_render_scene(name):
    """full_bits / visib_bits EQUAL render_scene's planes (row N19) for cases whose poses both calls accept: one K, every pose counted"""
    from checkerpose_amd import render
    case, D, out = _run(name)
    assert case.K.ndim == 2 and all(case.counted(b) for b in range(case.P))
    sc = render.render_scene(_up(case.R), _up(case.t), _up(case.K), _meshset(case), case.size, case.image_ids, mesh_ids=case.mesh_ids,
                             n_images=case.n_images, shading="flat", delta=case.delta)
    assert sc["ok"].all() and np.array_equal(sc["slot"].cpu().numpy(), out["slot"])
    assert np.array_equal(sc["full_bits"].cpu().numpy(), out["full_bits"]) and np.array_equal(sc["visib_bits"].cpu().numpy(), out["visib_bits"])
    assert np.array_equal(sc["px_count_visib"].cpu().numpy(), out["counts"][:, 1])


@pytest.mark.parametrize("name", ["occl_a", "mixed_b", "uncounted_a", "crowd33_b"])
def test_every_pose_alone_equals_verify_poses_mask(name):
    """with every pose in its own image: n_model, n_inter, n_vis_in, box, iou, cover EQUAL verify_poses_mask's; n_pvis == n_model"""
    from checkerpose_amd import postprocess as Q
    case, D, _ = _run(name)
    rows = np.array([b for b in range(case.P) if int(case.image_ids[b]) < case.n_images])      # (an image id out of range is this row's own refusal)
    solo = _device(case, idx=rows, image_ids=np.arange(len(rows)), n_images=len(rows), return_planes=False)
    a = _args(case, rows)
    score, info = Q.verify_poses_mask(a["R"], a["t"], a["cam_K"], a["meshes"], a["full"], visible=a["visible"], mask_ids=a["mask_ids"],
                                      mesh_ids=a["mesh_ids"], status=a["status"])
    for k, col in (("n_model", 0), ("n_inter", 2), ("n_vis_in", 3), ("n_mask", 5), ("n_vis", 6)):
        assert np.array_equal(info[k].cpu().numpy(), solo["counts"][:, col]), k
    assert np.array_equal(info["box"].cpu().numpy(), solo["box"])
    for k in ("iou", "cover"):
        assert np.array_equal(info[k].cpu().numpy().view(np.uint64), solo[k].view(np.uint64)), k
    assert np.array_equal(solo["counts"][:, 1], solo["counts"][:, 0]) and np.array_equal(solo["counts"][:, 4], solo["counts"][:, 3])
    assert not solo["counts"][:, 7].any() and np.array_equal(solo["box"], solo["box_pvis"])


@pytest.mark.parametrize("name", ["occl_a", "mixed_b", "uncounted_a", "crowd32_b"])
def test_bitwise_identities(name):
    """an image alone = in batches of two images = all images = the images permuted; with planes = without planes; call to call"""
    case, D, out = _run(name)
    assert _same(out, _device(case)) and np.array_equal(out["visib_bits"], _device(case)["visib_bits"])
    plain = _device(case, return_planes=False)
    assert plain["full_bits"] is None and _same(out, plain)
    ids = case.image_ids
    for i0 in range(0, case.n_images, 2):                                          # images i0, i0 + 1 as a call of their own
        rows = np.nonzero((ids >= i0) & (ids < i0 + 2))[0]
        if len(rows):
            part = _device(case, idx=rows, image_ids=ids[rows] - i0, n_images=2)
            n = min(2, case.n_images - i0)
            assert _same(_rows(out, rows), part), i0
            assert np.array_equal(part["full_bits"][:n], out["full_bits"][i0:i0 + n]) and np.array_equal(part["visib_bits"][:n], out["visib_bits"][i0:i0 + n])
            assert not part["full_bits"][n:].any() and not part["visib_bits"][n:].any()
    for i in range(case.n_images):                                                 # every image alone
        rows = np.nonzero(ids == i)[0]
        if len(rows):
            one = _device(case, idx=rows, image_ids=np.zeros(len(rows), np.int32), n_images=1)
            assert _same(_rows(out, rows), one), i
            assert np.array_equal(one["visib_bits"][0], out["visib_bits"][i]) and np.array_equal(one["full_bits"][0], out["full_bits"][i])
    rows = np.nonzero(ids < case.n_images)[0]                                      # the images renumbered in reverse, the poses in their order
    rev = _device(case, idx=rows, image_ids=case.n_images - 1 - ids[rows])
    assert _same(_rows(out, rows), rev) and np.array_equal(rev["visib_bits"][::-1], out["visib_bits"])


def test_select_poses_on_the_scores():
    from checkerpose_amd import postprocess as Q
    case, D, out = _run("select_a")
    want = SV.reference(case, D)
    assert out["choice"].tolist() == want["choice"].tolist() == SV.select(out["score"].reshape(case.cand), out["ok"].reshape(case.cand)).tolist() == [1, 1]
    s = out["score"].reshape(case.cand)
    assert (s[1] == s[2]).all() and (s[1] > s[0]).all()                             # an exact tie made on the device: the same scene twice
    a = _args(case)
    score, info = Q.verify_scene_mask(**dict(a, return_planes=False))
    C_, B = case.cand
    choice, Rs, ts = Q.select_poses(score.view(C_, B), info["ok"].view(C_, B), a["R"].view(C_, B, 3, 3), a["t"].view(C_, B, 3, 1))
    assert choice.cpu().tolist() == [1, 1] and torch.equal(Rs[0], a["R"][2]) and torch.equal(Rs[1], a["R"][3])


def test_refusals_on_the_device():
    from checkerpose_amd import coco_eval
    from checkerpose_amd import postprocess as Q
    case, D, _ = _run("occl_a")
    a = _args(case)
    for name, bad in (("status", torch.ones(2, dtype=torch.int32, device=DEV)), ("mask_ids", [0, 1, 2, 0, 1, 0]), ("mask_ids", [0, 1]), ("mask_ids", None),
                      ("mesh_ids", [0, 1, 2, 0, 1, 0]), ("mask_ids", torch.zeros(5, dtype=torch.int32, device=DEV)), ("image_ids", [0, 0, 1, 1, 2, 3]),
                      ("image_ids", [0, 1]), ("image_ids", [0, 0, 1, 1, 2, -1]), ("image_ids", torch.zeros(5, dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError, match="masks for" if bad is None else name):
            Q.verify_scene_mask(**dict(a, **{name: bad}))
    with pytest.raises(ValueError, match="n_images"):                              # resident ids are not read
        Q.verify_scene_mask(**dict(a, image_ids=_up(case.image_ids), n_images=None))
    crowd = SV.make("crowd33_b")
    with pytest.raises(ValueError, match="at most 32"):                            # host ids: 33 poses in image 0
        Q.verify_scene_mask(**dict(_args(crowd), image_ids=crowd.image_ids.tolist()))
    with pytest.raises(ValueError, match="visible"):
        Q.verify_scene_mask(**dict(a, visible=coco_eval.pack_masks(torch.zeros(2, 50, 70, dtype=torch.uint8, device=DEV))))
    with pytest.raises(ValueError, match="delta"):
        Q.verify_scene_mask(**dict(a, delta=-0.5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.verify_scene_mask(**dict(a, R=a["R"].cpu()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.verify_scene_mask(**dict(a, status=torch.ones(6, dtype=torch.int32)))
    cpu = coco_eval.PackedMasks(a["full"].bits.cpu(), a["full"].area.cpu(), a["full"].box.cpu(), 80, 96)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.verify_scene_mask(**dict(a, full=cpu))


# ------------------------------------------------------------------------------------------------------------------ the caller
def test_estimate_poses_scene_verified_is_the_composition_of_its_parts():
    from checkerpose_amd import postprocess as Q
    from checkerpose_amd.metric import MeshSet
    from checkerpose_amd.synthetic import build_net
    from tests import pnp_stages as S
    rng = np.random.default_rng(9)
    frames = torch.from_numpy(rng.integers(0, 256, (4, 80, 96, 3), dtype=np.uint8)).cuda()               # (W, H) = (96, 80)
    boxes = [[20, 16, 48, 40], [50, 24, 30, 44], None, [-6, 44, 40, 40]]
    net = build_net(npoint=512, seed=1).cuda().eval()
    net.set_compute_dtype("bf16")
    p3d = torch.from_numpy(S.lmo_model(512).astype(np.float32)).cuda()
    K = I.K_A.astype(np.float32)
    v, f = I.mesh_arrays(("box", "torus"))
    ms = MeshSet.from_arrays(v, faces=f)
    mesh_ids = [0, 1, 0, 1]
    B = 4
    spec = dict(meshes=ms, mesh_ids=mesh_ids, delta=15.0)
    for idx, n_frames in (([0, 1, 0, 1], 2), ([0, 1, 2, 3], 4)):
        kw = dict(img_index=idx, seed=3, resize_method="crop_resize")
        fr = frames[:n_frames]
        plain = Q.estimate_poses(net, fr, boxes, p3d, K, **kw)
        assert all(torch.equal(x, y) for x, y in zip(plain[:4], Q.estimate_poses_scene_verified(net, fr, boxes, p3d, K, spec, **kw)[:4]))      # refine=None: one candidate
        stages, inl, status, final = Q._estimate_stages(net, fr, boxes, p3d, K, refine="lm", **kw)
        masks = Q.estimate_poses_masks(net, fr, boxes, p3d, K, channel=1, **kw)[5]                         # the pastes of a separate forward
        vis = Q.estimate_poses_masks(net, fr, boxes, p3d, K, channel=0, **kw)[5]
        R, t, inl2, status2, final2, rep = Q.estimate_poses_scene_verified(net, fr, boxes, p3d, K, spec, return_verify=True, refine="lm", **kw)
        assert torch.equal(inl2, inl) and torch.equal(status2, status) and np.array_equal(final2, final) and rep["stages"] == ("solver", "lm")
        assert torch.equal(rep["full"].bits, masks.bits) and torch.equal(rep["visible"].bits, vis.bits) and torch.equal(rep["visible"].area, vis.area)
        image_ids = [c * n_frames + i for c in range(2) for i in idx]
        assert list(rep["image_ids"]) == image_ids
        Rc, tc = torch.stack([s[1] for s in stages]), torch.stack([s[2] for s in stages])
        score, info = Q.verify_scene_mask(Rc.reshape(2 * B, 3, 3), tc.reshape(2 * B, 3, 1), K, ms, masks, vis, image_ids, 15.0, mask_ids=list(range(B)) * 2,
                                          mesh_ids=mesh_ids * 2, status=status.repeat(2), n_images=2 * n_frames)
        choice, R2, t2 = Q.select_poses(score.view(2, B), info["ok"].view(2, B), Rc, tc)
        assert np.array_equal(rep["score"].cpu().numpy(), score.view(2, B).cpu().numpy(), equal_nan=True) and torch.equal(rep["choice"], choice)
        assert all(torch.equal(rep["info"][k], info[k]) for k in SV.COUNTS + ("ok", "box", "box_pvis", "slot"))
        assert torch.equal(R, R2) and torch.equal(t, t2) and tuple(R.shape) == (B, 3, 3) and tuple(t.shape) == (B, 3, 1)
        pick = choice.cpu().tolist()
        assert all(torch.equal(R[b], stages[pick[b]][1][b]) and torch.equal(t[b], stages[pick[b]][2][b]) for b in range(B))      # the chosen candidate's bits
        assert all(pick[b] == 0 for b in range(B) if int(status[b]) == 0)                                  # the fallback never loses its place
        assert rep["info"]["slot"].cpu().tolist() == ([0, 0, 1, 1] * 2 if n_frames == 2 else [0] * 8)
        if n_frames == 4:                                                          # one crop per frame: estimate_poses_mask_verified's bits
            rep28 = Q.estimate_poses_mask_verified(net, fr, boxes, p3d, K, dict(meshes=ms, mesh_ids=mesh_ids), return_verify=True, refine="lm", **kw)[5]
            for k in ("n_model", "n_inter", "n_vis_in", "n_mask", "n_vis", "box"):
                assert torch.equal(rep["info"][k], rep28["info"][k]), k
            for k in ("iou", "cover"):
                assert torch.equal(rep["info"][k].view(torch.int64), rep28["info"][k].view(torch.int64)), k
            assert torch.equal(rep["info"]["n_pvis"], rep["info"]["n_model"])
    with pytest.raises(NotImplementedError, match="warp_affine"):
        Q.estimate_poses_scene_verified(net, frames, boxes, p3d, K, spec, img_index=[0, 1, 0, 1], resize_method="crop_resize_by_warp_affine")
