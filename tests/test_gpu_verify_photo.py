"""GPU: row N35 on the device.  verify_poses_photo over the cases of tests/photo_stages.py -- frames of 33 x 31 (partial tiles on both
sides), 64 x 64 and 96 x 40 with three frames; 1, 3 and 257 poses; textured nearest and linear, vertex colours, a surface colour, mixed
MeshSets; flat and phong; with and without visible masks; bgr on and off -- against the numpy rule applied to the device's own
render.render_rgb colour and depth of the same poses and the frames: counts, sums and ok EQUAL, ncc, gain and offset within 4 ulp (three
to four correctly rounded operations: the same bits are expected, the bound allows one ulp each).  The identities and the can on the
device, a pose alone and in a batch, the edge cases, the caller against its composition."""
import numpy as np
import pytest
import torch

from tests import icp_stages as I
from tests import photo_stages as PS
from tests import render_tex_stages as RT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ULP_BOUND = 4
_MS, _RUNS = {}, {}
INT_KEYS = ("n_model", "n") + PS.SUMS
F64_KEYS = ("ncc", "gain", "offset")


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _meshset(names, tex_filter="nearest"):
    from checkerpose_amd.metric import MeshSet
    key = (tuple(names), tex_filter)
    if key not in _MS:
        verts, kw = PS.meshset_args(names, tex_filter)
        _MS[key] = MeshSet.from_arrays(verts, **kw)
    return _MS[key]


def _ids(ids, limit):
    """host ids are checked by the wrapper; ids that name no row travel as a resident tensor and reach the kernel"""
    if ids is None:
        return None
    ids = np.asarray(ids)
    return _up(ids.astype(np.int32)) if ((ids < 0) | (ids >= limit)).any() else ids


def _pick(x, idx):
    return None if x is None else np.asarray(x)[idx]


def _call_args(case, idx):
    """what render_rgb and verify_poses_photo share, for the rows idx of the case"""
    ms = _meshset(case.meshes, case.tex_filter)
    return dict(R=_up(case.R[idx]), t=_up(case.t[idx]), cam_K=_up(case.K[idx] if case.K.ndim == 3 else case.K), meshes=ms,
                mesh_ids=_ids(_pick(case.mesh_ids, idx), len(case.meshes)), **case.render_kwargs())


def _renders(case, idx):
    """the device's own colour and depth renders of the case's poses -> (C (P,H,W,3) uint8, D (P,H,W) float32, ok (P,)) numpy"""
    from checkerpose_amd import render
    res = render.render_rgb(size=case.size, return_depth=True, **_call_args(case, idx))
    return res["rgb"].cpu().numpy(), res["depth"].cpu().numpy(), res["ok"].cpu().numpy().astype(bool)


def _device(case, idx=None, **over):
    """verify_poses_photo on the device -> dict of numpy arrays"""
    from checkerpose_amd import coco_eval
    from checkerpose_amd import postprocess as Q
    idx = np.arange(case.P) if idx is None else np.asarray(idx)
    whole = len(idx) == case.P and (idx == np.arange(case.P)).all()
    a = _call_args(case, idx)
    image_ids = None if case.n_img == 1 else np.array([case.image_of(b) for b in idx], dtype=np.int32)
    if case.image_ids is None and whole:
        image_ids = None                                                          # the default rule: the one frame, or frame p for pose p
    visible = mask_ids = None
    if case.masks is not None:
        visible = coco_eval.pack_masks(_up(case.masks.astype(np.uint8)))
        mask_ids = None if (case.mask_ids is None and whole) else np.array([case.mask_of(b) for b in idx], dtype=np.int32)
    a.update(frames=_up(case.frames), min_pixels=case.min_pixels, image_ids=_ids(image_ids, case.n_img), visible=visible,
             mask_ids=_ids(mask_ids, 0 if case.masks is None else len(case.masks)), status=None if case.status is None else _up(case.status[idx]),
             bgr=case.bgr)
    a.update(over)
    score, info = Q.verify_poses_photo(**a)
    P = len(idx)
    assert score.dtype == torch.float64 and tuple(score.shape) == (P,) and info["ok"].dtype == torch.bool
    assert all(info[k].dtype == torch.int32 and tuple(info[k].shape) == (P,) for k in ("n_model", "n"))
    assert all(info[k].dtype == torch.int64 and tuple(info[k].shape) == (P,) for k in PS.SUMS)
    assert all(info[k].dtype == torch.float64 and tuple(info[k].shape) == (P,) for k in F64_KEYS)
    assert sorted(info) == sorted(INT_KEYS + F64_KEYS + ("ok",))
    out = {k: info[k].cpu().numpy() for k in info}
    out["score"] = score.cpu().numpy()
    return out


def _want(case, idx, C, D, rendered):
    """the numpy rule on the device's renders -> the same layout"""
    rows = []
    for j, b in enumerate(idx):
        m = case.mask_of(b)
        img = case.image_of(b)
        counted = bool(rendered[j]) and (case.status is None or case.status[b] != 0) and 0 <= img < case.n_img \
            and (m is None or 0 <= m < len(case.masks)) and (case.mesh_ids is None or 0 <= case.mesh_ids[b] < len(case.meshes))
        frame = case.frames[img] if 0 <= img < case.n_img else case.frames[0]
        mask = case.masks[m] if (m is not None and 0 <= m < len(case.masks)) else None
        rows.append(PS.reference(C[j], D[j], frame, case.min_pixels, mask, case.bgr, counted))
    return {k: np.array([r[k] for r in rows]) for k in INT_KEYS + F64_KEYS + ("score", "ok")}


def _run(name):
    """a case on the device: (case, its renders, its outputs, the rule's); computed once, left unchanged"""
    if name not in _RUNS:
        case = PS.make(name)
        idx = np.arange(case.P)
        C, D, rendered = _renders(case, idx)
        _RUNS[name] = (case, (C, D, rendered), _device(case), _want(case, idx, C, D, rendered))
    return _RUNS[name]


def _check(out, want, log=None, what=""):
    for k in INT_KEYS:
        assert np.array_equal(out[k].astype(np.int64), want[k].astype(np.int64)), (what, k)
    assert np.array_equal(out["ok"], want["ok"]), what
    worst = 0
    for k in F64_KEYS + ("score",):
        assert np.array_equal(np.isnan(out[k]), np.isnan(want[k])), (what, k)
        d = int(max(PS.ulp_distance(out[k], want[k])))
        if log:
            log("%s %s: worst distance %d ulp" % (what, k, d))
        worst = max(worst, d)
    assert worst <= ULP_BOUND, (what, worst)
    assert np.array_equal(out["score"], out["ncc"], equal_nan=True)
    return worst


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) and a[k].dtype == b[k].dtype for k in INT_KEYS + F64_KEYS + ("score", "ok"))


def _rows(out, rows):
    return {k: v[np.asarray(rows)] for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name", list(PS.CASES))
def test_device_equals_the_rule(name):
    case, (C, D, rendered), out, want = _run(name)
    worst = _check(out, want, log=print, what=name)
    print("%s: P %d, counted %d, ok %d, n %d..%d, worst %d ulp" % (name, case.P, rendered.sum(), out["ok"].sum(), out["n"].min(), out["n"].max(), worst))
    assert rendered.all() and out["ok"].sum() >= max(1, case.P // 2) and (out["n"][out["ok"]] >= case.min_pixels).all()      # no pass from trivial sums
    assert (np.abs(out["ncc"][out["ok"]]) <= 1.0).all()
    if case.masks is not None:
        assert (out["n"] < out["n_model"]).any()                                  # the masks bite
    else:
        assert np.array_equal(out["n"], out["n_model"])


@pytest.mark.parametrize("name", ["tex_nearest_33x31_3", "tex_linear_64_3", "vcol_96x40_3", "mixed_64_3"])
def test_a_pose_alone_and_in_a_batch(name):
    """a pose alone, in its batch, in reverse order, from call to call: the same bits"""
    case, _, out, _ = _run(name)
    assert _same(out, _device(case))
    for b in range(case.P):
        assert _same(_rows(out, [b]), _device(case, idx=[b])), b
    rev = np.arange(case.P)[::-1].copy()
    assert _same(_rows(out, rev), _device(case, idx=rev))


def test_rows_of_the_second_pose_block_alone():
    case, _, out, _ = _run("mixed_96x40_257")
    for rows in ([0], [255, 256], [256]):
        assert _same(_rows(out, rows), _device(case, idx=rows)), rows


def test_bgr_and_masks_change_what_they_should():
    """bgr touches the frame's luma only; without the masks n is n_model"""
    case, (C, D, rendered), out, _ = _run("tex_linear_64_3")
    flipped = _device(case, frames=_up(case.frames[..., ::-1]), bgr=not case.bgr)
    assert _same(out, flipped)                                                    # the same photograph stored the other way
    other = _device(case, bgr=not case.bgr)
    assert np.array_equal(other["Sa"], out["Sa"]) and np.array_equal(other["Saa"], out["Saa"]) and not np.array_equal(other["Sb"], out["Sb"])
    bare = _device(case, visible=None, mask_ids=None)
    assert np.array_equal(bare["n"], out["n_model"]) and np.array_equal(bare["n_model"], out["n_model"]) and (bare["n"] > out["n"]).any()


# ----------------------------------------------------------------------------------------------------- the identities, the can
def _frame_over(img, D, seed):
    H, W = D.shape
    bg = np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8)
    return np.where((D > 0)[..., None], img, bg)


def test_identities_on_the_device():
    from checkerpose_amd import postprocess as Q
    from checkerpose_amd import render
    ms = _meshset(["cbox"])
    size, K = (64, 64), RT._cam((64, 64), 140.0)
    R, t = _up(RT._pose(0.5, -0.7, 0.3, (0, 0, 0))[0][None]), _up(np.array([[2.0, -1.0, 320.0]]))
    for kw in (dict(shading="flat", ambient_weight=0.5), dict(shading="phong", ambient_weight=0.3, surf_color=(0.45, 0.4, 0.3))):
        res = render.render_rgb(R, t, K, ms, size, return_depth=True, **kw)
        C, D = res["rgb"][0].cpu().numpy(), res["depth"][0].cpu().numpy()
        score, info = Q.verify_poses_photo(R, t, K, ms, _up(_frame_over(C, D, 1)[None]), 8, **kw)
        assert bool(info["ok"][0]) and float(score[0]) == 1.0 and float(info["gain"][0]) == 1.0 and float(info["offset"][0]) == 0.0
        assert int(info["n"][0]) == int((D > 0).sum()) > 200
    Y = PS.luma(C)                                                                # the dark surface colour: Y <= 126
    assert Y[D > 0].max() <= 126 and len(np.unique(Y[D > 0])) > 3
    grey = np.repeat(np.clip(2 * Y + 3, 0, 255).astype(np.uint8)[..., None], 3, -1)
    score, info = Q.verify_poses_photo(R, t, K, ms, _up(_frame_over(grey, D, 2)[None]), 8, **kw)
    assert float(score[0]) == 1.0 and float(info["gain"][0]) == 2.0 and float(info["offset"][0]) == 3.0 and bool(info["ok"][0])
    neg = np.repeat((255 - Y).astype(np.uint8)[..., None], 3, -1)
    score, info = Q.verify_poses_photo(R, t, K, ms, _up(_frame_over(neg, D, 3)[None]), 8, **kw)
    assert float(score[0]) == -1.0 and float(info["gain"][0]) == -1.0 and float(info["offset"][0]) == 255.0


@pytest.mark.parametrize("filt,shading", [("nearest", "flat"), ("linear", "phong")])
def test_the_can_on_the_device(filt, shading):
    """the frame is the can rendered at the true pose; the candidate turned half way about the axis has the same silhouette and loses"""
    from checkerpose_amd import postprocess as Q
    from checkerpose_amd import render
    ms = _meshset(["can"], filt)
    size, K = (64, 64), RT._cam((64, 64), 100.0)
    Rt, Rh, t = PS.can_poses()
    R, tt = _up(np.stack([Rt, Rh])), _up(np.stack([t, t]))
    res = render.render_rgb(R, tt, K, ms, size, shading=shading, return_depth=True)
    C, D = res["rgb"].cpu().numpy(), res["depth"].cpu().numpy()
    iou = PS.silhouette_iou(D[0], D[1])
    frame = _up(_frame_over(C[0], D[0], 4)[None])
    score, info = Q.verify_poses_photo(R, tt, K, ms, frame, 8, shading=shading)
    s = score.cpu().numpy()
    print("can %s %s on the device: ncc true %.17g turned %.17g, silhouette IoU %.6f" % (filt, shading, s[0], s[1], iou))
    assert iou >= 0.98 and s[0] == 1.0 and s[1] < 0.0 and info["ok"].all()
    want = [PS.reference(C[k], D[k], frame[0].cpu().numpy(), 8) for k in (0, 1)]
    assert max(PS.ulp_distance(s, [w["ncc"] for w in want])) <= ULP_BOUND
    choice, Rs, ts = Q.select_poses(score.view(2, 1), info["ok"].view(2, 1), R.view(2, 1, 3, 3), tt.view(2, 1, 3, 1))
    assert choice.cpu().tolist() == [0] and torch.equal(Rs[0], R[0])
    back = torch.tensor([1, 0], device=DEV)
    score2, info2 = Q.verify_poses_photo(R[back], tt[back], K, ms, frame, 8, shading=shading)
    assert Q.select_poses(score2.view(2, 1), info2["ok"].view(2, 1)).cpu().tolist() == [1] and torch.equal(score2, score[back])


# -------------------------------------------------------------------------------------------------------------------- the edges
def _edge_case():
    c = PS.PhotoCase("edges_64_10", ["tbox", "cico"], (64, 64), 150.0, 10, 21, n_img=2, masks=3, shared_masks=True, min_pixels=10)
    c.image_ids = np.array([0, 0, 0, 0, 0, 2, 0, 0, 1, 0], dtype=np.int32)          # 5: no such frame; 8: the flat frame
    c.mask_ids = np.array([0, 1, 2, 0, 1, 2, 3, 1, 0, 2], dtype=np.int32)           # 6: no such mask
    c.mesh_ids = np.array([0, 1, 0, 1, 2, 1, 0, 1, 0, 1], dtype=np.int32)           # 4: no such mesh
    c.status = np.array([1, 0, 1, 1, 1, 1, 1, 1, 1, 7], dtype=np.int32)             # 1: the solver's fallback
    c.t[2, 2] = -320.0                                                            # 2: behind the camera
    c.R[3, 1, 1] = np.nan                                                         # 3: a NaN pose
    c.frames[1] = 77                                                              # frame 1: flat
    c.masks[1] = False                                                            # mask 1: 3 x 3 pixels about pose 7's centre
    K = c.K_of(7)
    u, v = int(K[0, 0] * c.t[7, 0] / c.t[7, 2] + K[0, 2]), int(K[1, 1] * c.t[7, 1] / c.t[7, 2] + K[1, 2])
    c.masks[1, v - 1:v + 2, u - 1:u + 2] = True
    return c


def test_edge_cases():
    case = _edge_case()
    idx = np.arange(case.P)
    C, D, rendered = _renders(case, idx)
    out, want = _device(case), _want(case, idx, C, D, rendered)
    _check(out, want, what="edges")
    nan_bits = np.array([np.nan]).view(np.uint64)[0]
    assert rendered.tolist() == [True, True, False, False, False, True, True, True, True, True]
    assert out["ok"].tolist() == [True] + [False] * 8 + [True]
    for b in range(1, 9):
        assert all(out[k][b:b + 1].view(np.uint64)[0] == nan_bits for k in F64_KEYS + ("score",)), b
    for b in range(1, 7):                                                         # not counted: zero sums, although 1, 5 and 6 render
        assert all(out[k][b] == 0 for k in INT_KEYS), b
    assert D[1].any() and D[5].any() and D[6].any()
    assert out["n"][7] == 9 and out["n_model"][7] > 100 and out["Sa"][7] > 0     # n < min_pixels: counted, reported, not scored
    assert out["n"][8] >= 10 and out["Sbb"][8] == 77 * 77 * out["n"][8] and out["Saa"][8] > 0      # a flat frame patch: vb == 0
    case.min_pixels = 9                                                           # exactly n: pose 7 is scored now
    lower = _device(case)
    _check(lower, _want(case, idx, C, D, rendered), what="edges, min_pixels 9")
    assert lower["ok"].tolist() == [True] + [False] * 6 + [True, False, True] and _same(_rows(out, [0, 9]), _rows(lower, [0, 9]))
    assert all(np.array_equal(lower[k], out[k]) for k in INT_KEYS)
    # a flat render: a surface colour at ambient_weight = 1 -> va == 0
    flat = _device(case, idx=[0, 9], surf_color=(0.3, 0.6, 0.2), ambient_weight=1.0)
    assert not flat["ok"].any() and np.isnan(flat["score"]).all() and (flat["n"] >= 10).all()
    assert (flat["n"] * flat["Saa"] == flat["Sa"] * flat["Sa"]).all() and (flat["Sa"] > 0).all()


def test_refusals_on_the_device():
    from checkerpose_amd import coco_eval
    from checkerpose_amd import postprocess as Q
    case = PS.make("tex_nearest_33x31_3")
    a = _call_args(case, np.arange(3))
    a.update(frames=_up(case.frames), min_pixels=8, visible=coco_eval.pack_masks(_up(case.masks.astype(np.uint8))))
    Q.verify_poses_photo(**a)
    for name, bad in (("status", torch.ones(2, dtype=torch.int32, device=DEV)), ("mask_ids", [0, 1, 3]), ("mask_ids", [0, 1]), ("mesh_ids", [0, 1, 3]),
                      ("image_ids", [0, 0, 1]), ("mask_ids", torch.zeros(5, dtype=torch.int32, device=DEV)), ("min_pixels", 1)):
        with pytest.raises(ValueError, match=name):
            Q.verify_poses_photo(**dict(a, **{name: bad}))
    with pytest.raises(ValueError, match="need mask_ids"):
        Q.verify_poses_photo(**dict(a, visible=coco_eval.pack_masks(_up(case.masks[:2].astype(np.uint8)))))
    with pytest.raises(ValueError, match="need image_ids"):
        Q.verify_poses_photo(**dict(a, frames=_up(np.repeat(case.frames, 2, 0))))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.verify_poses_photo(**dict(a, R=a["R"].cpu()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.verify_poses_photo(**dict(a, frames=a["frames"].cpu()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.verify_poses_photo(**dict(a, status=torch.ones(3, dtype=torch.int32)))


# ------------------------------------------------------------------------------------------------------------------ the caller
def test_estimate_poses_photo_verified_is_the_composition_of_its_parts():
    from checkerpose_amd import postprocess as Q
    from checkerpose_amd.metric import MeshSet
    from checkerpose_amd.synthetic import build_net
    from tests import pnp_stages as S
    rng = np.random.default_rng(9)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 80, 96, 3), dtype=np.uint8)).cuda()               # (W, H) = (96, 80)
    boxes = [[20, 16, 48, 40], [50, 24, 30, 44], None, [-6, 44, 40, 40]]
    idx = [0, 1, 0, 1]
    net = build_net(npoint=512, seed=1).cuda().eval()
    net.set_compute_dtype("bf16")
    p3d = torch.from_numpy(S.lmo_model(512).astype(np.float32)).cuda()
    K = I.K_A.astype(np.float32)
    v, f = I.mesh_arrays(("box", "torus"))
    ms = MeshSet.from_arrays(v, faces=f)
    mesh_ids = [0, 1, 0, 1]
    spec = dict(meshes=ms, min_pixels=8, mesh_ids=mesh_ids, shading="flat", ambient_weight=0.4)
    kw = dict(img_index=idx, seed=3, resize_method="crop_resize")
    B = 4
    plain = Q.estimate_poses(net, frames, boxes, p3d, K, **kw)
    assert all(torch.equal(x, y) for x, y in zip(plain[:4], Q.estimate_poses_photo_verified(net, frames, boxes, p3d, K, spec, **kw)[:4]))      # refine=None: one candidate
    with pytest.raises(ValueError, match="frames"):
        Q.estimate_poses_photo_verified(net, frames.float(), boxes, p3d, K, spec, **kw)
    for use_visible in (True, False):
        keep = {}
        stages, inl, status, final = Q._estimate_stages(net, frames, boxes, p3d, K, refine="lm", keep=keep, **kw)
        vis = Q.paste_masks(keep["seg"], keep["padded"], (80, 96), "crop_resize", 0) if use_visible else None
        R, t, inl2, status2, final2, rep = Q.estimate_poses_photo_verified(net, frames, boxes, p3d, K, dict(spec, use_visible=use_visible), return_verify=True,
                                                                           refine="lm", **kw)
        assert torch.equal(inl2, inl) and torch.equal(status2, status) and np.array_equal(final2, final) and rep["stages"] == ("solver", "lm")
        assert (rep["visible"] is None) if vis is None else (torch.equal(rep["visible"].bits, vis.bits) and torch.equal(rep["visible"].area, vis.area))
        Rc, tc = torch.stack([s[1] for s in stages]), torch.stack([s[2] for s in stages])
        score, info = Q.verify_poses_photo(Rc.reshape(2 * B, 3, 3), tc.reshape(2 * B, 3, 1), K, ms, frames, 8, image_ids=idx * 2, visible=vis,
                                           mask_ids=(list(range(B)) * 2) if use_visible else None, mesh_ids=mesh_ids * 2, status=status.repeat(2),
                                           shading="flat", ambient_weight=0.4)
        choice, R2, t2 = Q.select_poses(score.view(2, B), info["ok"].view(2, B), Rc, tc)
        assert np.array_equal(rep["score"].cpu().numpy(), score.view(2, B).cpu().numpy(), equal_nan=True) and torch.equal(rep["choice"], choice)
        assert all(torch.equal(rep["info"][k], info[k]) for k in INT_KEYS + ("ok",))
        assert all(np.array_equal(rep["info"][k].cpu().numpy(), info[k].cpu().numpy(), equal_nan=True) for k in F64_KEYS)
        assert torch.equal(R, R2) and torch.equal(t, t2) and tuple(R.shape) == (B, 3, 3) and tuple(t.shape) == (B, 3, 1)
        pick = choice.cpu().tolist()
        assert all(torch.equal(R[b], stages[pick[b]][1][b]) and torch.equal(t[b], stages[pick[b]][2][b]) for b in range(B))      # the chosen candidate's bits
        assert all(pick[b] == 0 for b in range(B) if int(status[b]) == 0)                                  # the fallback never loses its place
        assert list(rep["image_ids"]) == idx * 2
    with pytest.raises(NotImplementedError, match="warp_affine"):
        Q.estimate_poses_photo_verified(net, frames, boxes, p3d, K, spec, img_index=idx, resize_method="crop_resize_by_warp_affine")
