"""CPU: row N35's rule (tests/photo_stages.py) checked on itself -- the identities its form was chosen for, every tampering caught, the can
whose silhouette does not see half a turn -- with renders from the fp32 restatements of the device's arithmetic (render_tex_f32 /
render_f32), and the argument checks and the routing of the two Python functions, which run without a GPU."""
import inspect

import numpy as np
import pytest
import torch

from tests import photo_stages as PS
from tests import render_tex_stages as RT

SIZE = (64, 64)
K = RT._cam(SIZE, 100.0)
T = np.array([1.0, 2.0, 320.0])
_R = {}


def _render(name, seed, filt="nearest", shading="flat", ambient=0.5, surf_color=None):
    """a pose of a mesh, rendered once -> (C, D)"""
    key = (name, seed, filt, shading, ambient, surf_color)
    if key not in _R:
        R = RT._pose(*np.random.default_rng(seed).uniform(-1, 1, 3), (0, 0, 0))[0]
        _R[key] = PS.cpu_render(name, R, T, K, SIZE, filt, shading, ambient, surf_color)
    return _R[key]


def _noise(seed, shape=(64, 64, 3)):
    return np.random.default_rng(100 + seed).integers(0, 256, shape).astype(np.uint8)


def _over(C, D, bg):
    return np.where((D > 0)[..., None], C, bg)


RENDERS = (("tbox", 1, "nearest", "flat"), ("tbox", 2, "nearest", "flat"), ("cico", 0, "nearest", "phong"), ("tico", 1, "linear", "flat"),
           ("cbox", 2, "nearest", "flat"), ("tquad", 3, "nearest", "phong"))


# ---------------------------------------------------------------------------------------------------------------------- the rule itself
def test_luma_is_exact_on_greys_and_weighs_the_channels():
    g = np.arange(256, dtype=np.uint8)
    assert np.array_equal(PS.luma(np.stack([g, g, g], -1)), g)                     # weights sum to 256, + 128 rounds g + 0.5 down to g
    assert sum(PS.LUMA) == 256
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 200, 90]], dtype=np.uint8)
    assert PS.luma(px).tolist() == [(77 * 255 + 128) >> 8, (150 * 255 + 128) >> 8, (29 * 255 + 128) >> 8, (770 + 30000 + 2610 + 128) >> 8]
    assert np.array_equal(PS.luma(px[:, ::-1], swap=True), PS.luma(px))            # the same pixel stored B G R


def test_pack_and_read_are_inverse():
    m = np.random.default_rng(3).random((3, 5, 70)) < 0.5
    bits = PS.pack(m)
    assert bits.shape == (3, 5, 3) and bits.dtype == np.int32 and np.array_equal(PS.read(bits, 70), m)
    one = np.zeros((1, 1, 70), dtype=bool)
    one[0, 0, 37] = True
    assert PS.pack(one).view(np.uint32)[0, 0].tolist() == [0, 1 << 5, 0]           # pixel 37 = bit 5 of word 1


def test_the_sums_are_the_plain_loops():
    C, D = _render("tbox", 1)
    frame, mask = _noise(1), np.random.default_rng(5).random((64, 64)) < 0.7
    got = PS.sums_of(C, D, frame, mask)
    want = dict(n_model=0, n=0, Sa=0, Sb=0, Saa=0, Sbb=0, Sab=0)
    for y in range(64):
        for x in range(64):
            if D[y, x] > 0:
                want["n_model"] += 1
                if mask[y, x]:
                    a = (77 * int(C[y, x, 0]) + 150 * int(C[y, x, 1]) + 29 * int(C[y, x, 2]) + 128) >> 8
                    b = (77 * int(frame[y, x, 0]) + 150 * int(frame[y, x, 1]) + 29 * int(frame[y, x, 2]) + 128) >> 8
                    want["n"] += 1
                    want["Sa"] += a; want["Sb"] += b; want["Saa"] += a * a; want["Sbb"] += b * b; want["Sab"] += a * b      # noqa: E702
    assert got == want and 0 < want["n"] < want["n_model"] < 64 * 64


def test_the_bounds_of_the_frame_size():
    """H W <= 2^22: a tile's sums fit int32, a pose's products int64"""
    assert 1024 * 255 ** 2 < 2 ** 31
    n = PS.MAX_PIXELS
    assert n * (n * 255 ** 2) < 2 ** 63 and (n * 255) ** 2 < 2 ** 63


@pytest.mark.parametrize("spec", RENDERS)
def test_identities(spec):
    C, D = _render(*spec)
    n = int((D > 0).sum())
    same = PS.reference(C, D, _over(C, D, _noise(7)), 8)
    assert same["ok"] and same["ncc"] == 1.0 and same["score"] == 1.0 and same["gain"] == 1.0 and same["offset"] == 0.0 and same["n"] == n > 100
    # a grey frame 2 Y + 3 of a render with Y <= 126
    dark = (C.astype(np.int64) * 126 // 255).astype(np.uint8)
    Y = PS.luma(dark)
    assert Y.max() <= 126
    grey = np.repeat((2 * Y + 3).astype(np.uint8)[..., None], 3, -1)
    lin = PS.reference(dark, D, _over(grey, D, _noise(8)), 8)
    assert lin["ok"] and lin["ncc"] == 1.0 and lin["gain"] == 2.0 and lin["offset"] == 3.0
    neg = PS.reference(dark, D, _over(255 - np.repeat(Y.astype(np.uint8)[..., None], 3, -1), D, _noise(9)), 8)
    assert neg["ok"] and neg["ncc"] == -1.0 and neg["gain"] == -1.0 and neg["offset"] == 255.0


def test_nan_cases():
    C, D = _render("tbox", 1)
    frame = _noise(1)
    nan_out = lambda r: not r["ok"] and all(np.isnan(r[k]) for k in ("ncc", "score", "gain", "offset"))      # noqa: E731
    r = PS.reference(C, D, frame, 8)
    assert r["ok"] and -1.0 < r["ncc"] < 1.0
    flat_render = PS.reference(np.full_like(C, 90), D, frame, 8)
    flat_frame = PS.reference(C, D, np.full_like(frame, 17), 8)
    assert nan_out(flat_render) and flat_render["n"] == r["n"] and nan_out(flat_frame) and flat_frame["Sb"] == 17 * r["n"]
    assert PS.reference(C, D, frame, r["n"])["ok"] and nan_out(PS.reference(C, D, frame, r["n"] + 1))
    off = PS.reference(C, D, frame, 8, counted=False)
    assert nan_out(off) and all(off[k] == 0 for k in ("n_model", "n") + PS.SUMS)
    assert nan_out(PS.reference(C, np.zeros_like(D), frame, 2))                   # nothing rendered


def _tamper_cases():
    """name -> (arguments of PS.reference, the outputs a tampering may change)"""
    C, D = _render("tbox", 1)
    Cc, Dc = _render("cico", 0, "nearest", "phong")
    mask = np.random.default_rng(5).random((64, 64)) < 0.7
    Rt, _, t = PS.can_poses()
    Ck, Dk = PS.cpu_render("can", Rt, t, K, SIZE, "nearest", "flat", 0.5)
    n = PS.sums_of(C, D, _noise(1))["n"]
    return {"noise": dict(C=C, D=D, frame=_noise(1), min_pixels=8),
            "masked": dict(C=Cc, D=Dc, frame=_noise(2), min_pixels=8, mask=mask),
            "bgr": dict(C=Cc, D=Dc, frame=_noise(3), min_pixels=8, bgr=True),
            "exactly_min": dict(C=C, D=D, frame=_noise(1), min_pixels=n),
            "can_identity": dict(C=Ck, D=Dk, frame=_over(Ck, Dk, _noise(1)), min_pixels=8)}


CAUGHT_BY = {"luma_weights": "noise", "no_round": "noise", "ge_zero": "noise", "ignore_mask": "masked", "cov_without_n": "noise",
             "split_sqrt": "can_identity", "min_pixels_off_by_one": "exactly_min", "bgr_on_render": "bgr"}


@pytest.mark.parametrize("tamper", PS.TAMPERINGS)
def test_every_tampering_is_caught(tamper):
    cases = _tamper_cases()
    a = cases[CAUGHT_BY[tamper]]
    right, wrong = PS.reference(**a), PS.reference(**a, tamper=(tamper,))
    bits = lambda r: [r[k] for k in ("n_model", "n") + PS.SUMS] + [np.float64(r[k]).view(np.uint64) for k in ("ncc", "gain", "offset")] + [r["ok"]]      # noqa: E731
    assert right["ok"] and bits(right) != bits(wrong), tamper
    if tamper == "split_sqrt":                                                     # the identity the form was chosen for is what it breaks
        assert right["ncc"] == 1.0 and wrong["ncc"] != 1.0 and abs(wrong["ncc"] - 1.0) < 1e-15
    if tamper == "min_pixels_off_by_one":
        assert not wrong["ok"] and np.isnan(wrong["ncc"])


@pytest.mark.parametrize("filt,shading", [("nearest", "flat"), ("linear", "phong")])
def test_the_can(filt, shading):
    """against the frame rendered at the true pose the true pose scores 1.0 and the pose turned half way about the axis far lower, while
    the two silhouettes are the same: what rows N26 / N28 / N31 cannot tell apart"""
    Rt, Rh, t = PS.can_poses()
    C0, D0 = PS.cpu_render("can", Rt, t, K, SIZE, filt, shading, 0.5)
    C1, D1 = PS.cpu_render("can", Rh, t, K, SIZE, filt, shading, 0.5)
    frame = _over(C0, D0, _noise(4))
    true, turned = PS.reference(C0, D0, frame, 8), PS.reference(C1, D1, frame, 8)
    iou = PS.silhouette_iou(D0, D1)
    print("can %s %s: ncc true %.17g turned %.17g, silhouette IoU %.6f (n %d / %d)" % (filt, shading, true["ncc"], turned["ncc"], iou, true["n"], turned["n"]))
    assert true["ok"] and turned["ok"] and true["ncc"] == 1.0 and turned["ncc"] < 0.0        # the label's halves swap: anti-correlated
    assert iou >= 0.98 and true["n"] > 400
    # under another brightness of the scene (gain 0.5, offset 40 on the frame) the gap stays
    dim = _over((C0.astype(np.int64) // 2 + 40).astype(np.uint8), D0, _noise(4))
    assert PS.reference(C0, D0, dim, 8)["ncc"] > 0.99 and PS.reference(C1, D1, dim, 8)["ncc"] < 0.0


def test_cases_are_well_formed():
    shapes = set()
    for name in PS.CASES:
        c = PS.make(name)
        W, H = c.size
        assert c.frames.shape == (c.n_img, H, W, 3) and c.frames.dtype == np.uint8 and c.R.shape == (c.P, 3, 3) and c.t.shape == (c.P, 3)
        assert np.allclose(np.linalg.det(c.R), 1.0) and (c.masks is None or c.masks.shape[1:] == (H, W))
        assert all(0 <= c.image_of(b) < c.n_img for b in range(c.P))
        shapes.add((c.size, c.P))
    assert {s for s, _ in shapes} == {(33, 31), (64, 64), (96, 40)} and {p for _, p in shapes} == {1, 3, 257}


# ---------------------------------------------------------------------------------------------------------------- the Python functions
def _host_args():
    from checkerpose_amd.metric import MeshSet
    verts, kw = PS.meshset_args(["tbox"])
    return dict(R=torch.eye(3, dtype=torch.float64)[None], t=torch.tensor([[0.0, 0.0, 300.0]], dtype=torch.float64), cam_K=K,
                meshes=MeshSet.from_arrays(verts, **kw), frames=torch.zeros(1, 31, 33, 3, dtype=torch.uint8), min_pixels=8)


def test_verify_poses_photo_argument_checks():
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd.coco_eval import PackedMasks
    assert str(inspect.signature(PP.verify_poses_photo)) == (
        "(R, t, cam_K, meshes, frames, min_pixels, image_ids=None, visible=None, mask_ids=None, mesh_ids=None, status=None, shading='phong', "
        "ambient_weight=0.5, light_cam_pos=(0, 0, 0), surf_color=None, bgr=False)")
    assert inspect.signature(PP.verify_poses_photo).parameters["min_pixels"].default is inspect.Parameter.empty      # NO default
    a = _host_args()
    for bad in (1, 0, -3, 2.5, None, True, "8", 1 << 31):
        with pytest.raises(ValueError, match="min_pixels"):
            PP.verify_poses_photo(**dict(a, min_pixels=bad))
    for bad in (a["frames"].float(), a["frames"].numpy(), torch.zeros(1, 31, 33, 4, dtype=torch.uint8), torch.zeros(31, 33, dtype=torch.uint8), None):
        with pytest.raises(ValueError, match="frames"):
            PP.verify_poses_photo(**dict(a, frames=bad))
    with pytest.raises(ValueError, match="2\\^22"):
        PP.verify_poses_photo(**dict(a, frames=torch.zeros(1, 2049, 2048, 3, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="shading"):
        PP.verify_poses_photo(**dict(a, shading="gouraud"))
    with pytest.raises(ValueError, match="ambient_weight"):
        PP.verify_poses_photo(**dict(a, ambient_weight=float("nan")))
    with pytest.raises(ValueError, match="mask_ids"):
        PP.verify_poses_photo(**dict(a, mask_ids=[0]))
    z = lambda n, h, w: PackedMasks(torch.zeros(n, h, (w + 31) // 32, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), None, h, w)      # noqa: E731
    for other in (z(1, 31, 32), z(1, 30, 33), z(0, 31, 33)):
        with pytest.raises(ValueError, match="visible"):
            PP.verify_poses_photo(**dict(a, visible=other))
    with pytest.raises(ValueError, match="visible"):
        PP.verify_poses_photo(**dict(a, visible=torch.zeros(1, 31, 33)))
    with pytest.raises(ValueError, match="faces"):
        PP.verify_poses_photo(**dict(a, meshes=np.zeros((4, 3))))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # well-formed arguments on the host: still no fallback
        PP.verify_poses_photo(**a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.verify_poses_photo(**dict(a, visible=z(1, 31, 33), shading="flat"))


def test_public_functions_of_postprocess():
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import verify_photo as M
    own = {n for n, f in vars(PP).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == PP.__name__}
    assert "verify_poses_photo" not in own and "estimate_poses_photo_verified" not in own and {"select_poses", "estimate_poses"} <= own
    assert {n for n, f in vars(M).items() if inspect.isfunction(f) and not n.startswith("_")} == {"verify_poses_photo", "estimate_poses_photo_verified"}
    assert PP.verify_poses_photo is M.verify_poses_photo and PP.estimate_poses_photo_verified is M.estimate_poses_photo_verified


def test_verify_values():
    from checkerpose_amd import postprocess as PP
    assert str(inspect.signature(PP.estimate_poses_photo_verified)) == "(net, frames, Bboxes, p3d_xyz, cam_K, verify, return_verify=False, **estimate_kwargs)"
    frames, p3d, K3 = torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(8, 3), torch.eye(3)
    for bad in (None, "yes", dict(), dict(meshes=None), dict(min_pixels=8), dict(mesh_ids=[0], min_pixels=8)):
        with pytest.raises(ValueError, match="verify"):
            PP.estimate_poses_photo_verified(None, frames, [], p3d, K3, bad)
    for key in ("image_ids", "status", "mask_ids"):
        with pytest.raises(ValueError, match="must not name"):
            PP.estimate_poses_photo_verified(None, frames, [], p3d, K3, {"meshes": None, "min_pixels": 8, key: [0]})
    for extra in ("grid", "depth", "tau", "delta", "ssaa", "bg_color"):
        with pytest.raises(ValueError, match="unknown"):
            PP.estimate_poses_photo_verified(None, frames, [], p3d, K3, {"meshes": None, "min_pixels": 8, extra: 1.0})
    for bad in (1, 0, 2.0, None):
        with pytest.raises(ValueError, match="min_pixels"):
            PP.estimate_poses_photo_verified(None, frames, [], p3d, K3, dict(meshes=None, min_pixels=bad))
    ok = dict(meshes=None, min_pixels=8)
    for bad in (frames.float(), frames.float() / 255.0, frames.numpy()):
        with pytest.raises(ValueError, match="frames"):
            PP.estimate_poses_photo_verified(None, bad, [], p3d, K3, ok)
    with pytest.raises(NotImplementedError, match="warp_affine"):
        PP.estimate_poses_photo_verified(None, frames, [], p3d, K3, ok, resize_method="crop_resize_by_warp_affine")
    with pytest.raises(ValueError, match="img_index"):
        PP.estimate_poses_photo_verified(None, frames[None], [[0, 0, 2, 2]], p3d, K3, ok, img_index=[1])
    with pytest.raises(ValueError, match="refine"):                              # estimate_poses' own refusals hold
        PP.estimate_poses_photo_verified(None, frames, [], p3d, K3, ok, refine="gn")
    with pytest.raises(TypeError):
        PP.estimate_poses_photo_verified(None, frames, [], p3d, K3, ok, no_such_keyword=1)


def test_estimate_poses_photo_verified_routes(monkeypatch):
    """ONE forward, the one paste of channel 0 (none without use_visible), the candidates' order, the ONE verify_poses_photo and ONE
    select_poses call with their arguments and the gather, with stubs in place of every device call"""
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import preprocess as PRE
    from tests import icp_stages as I
    B = 2
    calls = []
    base_R = torch.arange(B * 9, dtype=torch.float64).reshape(B, 3, 3)
    base_t = torch.arange(B * 3, dtype=torch.float64).reshape(B, 3, 1)
    status = torch.tensor([1, 0], dtype=torch.int32)
    monkeypatch.setattr(PRE, "get_roi_batch", lambda *a, **k: "crops")
    monkeypatch.setattr(PP, "correspondences", lambda out, **k: ("p2d", "valid", None))
    monkeypatch.setattr(PP, "solve_pnp_ransac", lambda *a, **k: (base_R, base_t, "inl", status))
    monkeypatch.setattr(PP, "refine_poses_lm", lambda p3d, p2d, mask, K, R, t, status=None: (calls.append(("lm",)), (R + 100.0, t + 100.0, None, None))[1])

    def net(crops, _):
        calls.append(("forward",))
        return ("roi", "xb", "yb", "SEG", "xid", "yid")

    def paste(seg, boxes, frame_size, method, channel):
        calls.append(("paste", seg, boxes, frame_size, method, channel))
        return "masks%d" % channel

    def verify(R, t, K, meshes, frames, min_pixels, **kw):
        calls.append(("verify", R, t, K, meshes, frames, min_pixels, kw))
        P = R.shape[0]
        return torch.arange(P, dtype=torch.float64), dict(ok=torch.ones(P, dtype=torch.bool), marker="info")

    def select(score, ok, R, t):
        calls.append(("select", score, ok, R, t))
        choice = torch.tensor([score.shape[0] - 1, 0], dtype=torch.int32)
        return choice, R[choice.long(), torch.arange(B)], t[choice.long(), torch.arange(B)]

    monkeypatch.setattr(PP, "paste_masks", paste)
    monkeypatch.setattr(PP, "verify_poses_photo", verify)
    monkeypatch.setattr(PP, "select_poses", select)
    frames = torch.zeros(2, 40, 48, 3, dtype=torch.uint8)
    Ks = np.stack([I.K_A, I.K_B])
    boxes = [[5, 5, 10, 10], [6, 6, 10, 10]]
    args = (net, frames, boxes, "p3d", Ks)
    spec = dict(meshes="VM", min_pixels=9, mesh_ids=[1, 0], shading="flat", bgr=True)
    padded = [PRE.padding_Bbox(b, 1.5) for b in boxes]
    for refine, names, shift, use_visible in ((None, ("solver",), (0.0,), True), ("lm", ("solver", "lm"), (0.0, 100.0), True), ("lm", ("solver", "lm"), (0.0, 100.0), False)):
        del calls[:]
        v_spec = dict(spec) if use_visible else dict(spec, use_visible=False)
        R, t, inl, st, final, rep = PP.estimate_poses_photo_verified(*args, v_spec, return_verify=True, img_index=[1, 0], refine=refine, resize_method="crop_resize")
        C_ = len(names)
        assert [c[0] for c in calls] == ["forward"] + ["lm"] * (C_ - 1) + ["paste"] * (1 if use_visible else 0) + ["verify", "select"]      # ONE forward
        pastes = [c for c in calls if c[0] == "paste"]
        assert [c[5] for c in pastes] == ([0] if use_visible else []) and all(c[1] == "SEG" and c[3] == (40, 48) and c[4] == "crop_resize" for c in pastes)
        assert all(np.array_equal(np.asarray(c[2]), np.asarray(padded)) for c in pastes)
        v, s = calls[-2], calls[-1]
        want_R = torch.cat([base_R + x for x in shift])
        want_t = torch.cat([base_t + x for x in shift])
        assert torch.equal(v[1], want_R) and torch.equal(v[2], want_t) and v[2].shape == (C_ * B, 3, 1)      # candidate-major, the stages' order
        assert np.array_equal(v[3], np.concatenate([Ks] * C_)) and v[4] == "VM" and v[5] is frames and v[6] == 9       # the call's own uint8 frames
        kw = v[7]
        assert sorted(kw) == ["bgr", "image_ids", "mask_ids", "mesh_ids", "shading", "status", "visible"] and kw["visible"] == ("masks0" if use_visible else None)
        assert kw["shading"] == "flat" and kw["bgr"] is True and list(kw["image_ids"]) == [1, 0] * C_      # img_index as image ids
        assert (list(kw["mask_ids"]) == [0, 1] * C_ if use_visible else kw["mask_ids"] is None)
        assert list(kw["mesh_ids"]) == [1, 0] * C_ and torch.equal(kw["status"], status.repeat(C_))
        assert s[1].shape == (C_, B) and s[2].shape == (C_, B) and torch.equal(s[3], want_R.view(C_, B, 3, 3)) and torch.equal(s[4], want_t.view(C_, B, 3, 1))
        assert torch.equal(R[0], base_R[0] + shift[-1]) and torch.equal(R[1], base_R[1]) and torch.equal(t[0], base_t[0] + shift[-1]) and torch.equal(t[1], base_t[1])
        assert inl == "inl" and st is status                                       # still the solver's
        assert rep["stages"] == names and rep["choice"].tolist() == [C_ - 1, 0] and rep["score"].shape == (C_, B) and rep["info"]["marker"] == "info"
        assert rep["visible"] == ("masks0" if use_visible else None) and list(rep["image_ids"]) == [1, 0] * C_
        assert len(PP.estimate_poses_photo_verified(*args, v_spec, img_index=[1, 0], refine=refine, resize_method="crop_resize")) == 5
