"""GPU: row N28 on the device.  verify_poses_mask over the committed cases of tests/verify_mask_stages.py -- two small frames ((96, 80):
3 x 3 tiles; (70, 50): a partial last word), several meshes, shared and permuted mask ids, per-pose intrinsics, with and without visible
masks, empty / full-frame / one-pixel / checkerboard / own-silhouette masks, poses partly and wholly off the frame, behind the camera,
with status 0, a mask id and a mesh id out of range, NaN -- against the numpy rule applied to the device's own metric.render_depth of
the same poses: counts, box, labels, ok and choice EQUAL, iou, cover and score the same bits; against the existing composition on the
device (render_depth > 0 -> pack_masks -> overlap counts); the identities (alone / batch, labels); select_poses; the caller."""
import numpy as np
import pytest
import torch

from tests import icp_stages as I
from tests import verify_mask_stages as VM

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_MS, _RUNS = {}, {}


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _meshset(case):
    from checkerpose_amd.metric import MeshSet
    if case.meshes not in _MS:
        v, f = I.mesh_arrays(case.meshes)
        _MS[case.meshes] = MeshSet.from_arrays(v, diameters=I.diameters(case.meshes), faces=f)
    return _MS[case.meshes]


def _mesh_ids(case, idx):
    """host ids are checked by the wrapper; ids that name no mesh travel as a resident tensor and reach the kernel"""
    ids = case.mesh_ids[idx]
    return _up(ids) if (ids >= len(case.meshes)).any() else ids


def _renders(case):
    """the device's own depth renders of the case's poses -> (P,H,W) float32 numpy (zeros for a pose whose mesh id names no mesh)"""
    from checkerpose_amd import metric
    D = metric.render_depth(_up(case.R), _up(case.t), _up(case.K), _meshset(case), case.size, mesh_ids=_mesh_ids(case, np.arange(case.P)))
    return D.cpu().numpy()


def _packed(case, D):
    """the case's masks packed on the device by row N15's pack_masks -> (full, visible or None)"""
    from checkerpose_amd import coco_eval
    F, Vm = case.masks(D)
    return coco_eval.pack_masks(_up(F.astype(np.uint8))), None if Vm is None else coco_eval.pack_masks(_up(Vm.astype(np.uint8)))


def _args(case, D, idx=None, **over):
    idx = np.arange(case.P) if idx is None else np.asarray(idx)
    full, vis = _packed(case, D)
    mids = case.mask_ids[idx] if case.mask_ids is not None else (None if len(idx) == case.P and (idx == np.arange(case.P)).all() else idx.astype(np.int32))
    if mids is not None and (mids >= case.N).any():
        mids = _up(mids)
    a = dict(R=_up(case.R[idx]), t=_up(case.t[idx]), cam_K=_up(case.K[idx] if case.K.ndim == 3 else case.K), meshes=_meshset(case), full=full,
             visible=vis, mask_ids=mids, mesh_ids=_mesh_ids(case, idx), status=None if case.status is None else _up(case.status[idx]),
             return_labels=True)
    a.update(over)
    return a


def _device(case, D, idx=None, **over):
    """verify_poses_mask on the device -> dict of numpy arrays in verify_mask_stages.reference's layout"""
    from checkerpose_amd import postprocess as Q
    a = _args(case, D, idx, **over)
    res = Q.verify_poses_mask(**a)
    score, info = res[0], res[1]
    P = len(score)
    assert score.dtype == torch.float64 and tuple(score.shape) == (P,) and info["ok"].dtype == torch.bool
    assert all(info[k].dtype == torch.int32 and tuple(info[k].shape) == (P,) for k in VM.COUNTS) and info["iou"].dtype == info["cover"].dtype == torch.float64
    assert info["box"].dtype == torch.int32 and tuple(info["box"].shape) == (P, 4)
    out = dict(counts=np.stack([info[k].cpu().numpy() for k in VM.COUNTS], 1), box=info["box"].cpu().numpy(), score=score.cpu().numpy(),
               iou=info["iou"].cpu().numpy(), cover=info["cover"].cpu().numpy(), ok=info["ok"].cpu().numpy(), labels=None, choice=None)
    if a["return_labels"]:
        assert res[2].dtype == torch.uint8 and tuple(res[2].shape) == (P,) + D.shape[1:]
        out["labels"] = res[2].cpu().numpy()
    if case.cand is not None and idx is None:
        out["choice"] = Q.select_poses(score.view(*case.cand), info["ok"].view(*case.cand)).cpu().numpy()
    return out


def _run(name):
    """a committed case on the device: (case, the device's renders, its outputs); computed once, left unchanged"""
    if name not in _RUNS:
        case = VM.make(name)
        D = _renders(case)
        _RUNS[name] = (case, D, _device(case, D))
    return _RUNS[name]


def _same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True) for k in ("counts", "box", "score", "iou", "cover", "ok", "labels"))


def _rows(out, rows):
    return {k: (None if v is None or k == "choice" else v[rows]) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name", list(VM.CASES))
def test_device_equals_the_rule(name):
    """counts, box, labels, ok and the choice EQUAL the numpy rule's on the device's own renders; iou, cover, score bit for bit"""
    case, D, out = _run(name)
    want = VM.check_case(case, D, out, log=print)
    assert out["counts"].dtype == np.int32 and out["labels"].dtype == np.uint8
    assert len(VM.nontrivial(case, D)) >= 1                                       # no pass from trivial counts
    if name == "mixed_b_5":
        assert out["score"][0] == 1.0 and out["ok"][0] and out["score"][2] == 0.0 and out["ok"][2] and out["counts"][3, 1] == 1
    if want["choice"] is not None:
        assert out["choice"].tolist() == want["choice"].tolist() == VM.reference(case, VM.cpu_renders(case))["choice"].tolist() == [1, 0]


@pytest.mark.parametrize("name", ["mixed_a_6", "mixed_b_5", "edges_b_9"])
def test_counts_equal_the_composition(name):
    """the existing way to the same numbers on the device: render_depth > 0 -> pack_masks -> overlap counts (mask_ious; the words' and)"""
    from checkerpose_amd import coco_eval
    case, D, out = _run(name)
    full, vis = _packed(case, D)
    sil = coco_eval.pack_masks(_up((D > 0).astype(np.uint8)))
    rows = [b for b in range(case.P) if case.counted(b)]
    mids = np.array([case.mask_of(b) for b in rows])
    assert np.array_equal(sil.area.cpu().numpy()[rows], out["counts"][rows, 0]) and np.array_equal(sil.box.cpu().numpy()[rows], out["box"][rows])
    pop = lambda w: np.unpackbits(np.ascontiguousarray(w).view(np.uint8).reshape(len(w), -1), axis=1).sum(1)      # noqa: E731
    sw = sil.bits.cpu().numpy()[rows]
    assert np.array_equal(pop(sw & full.bits.cpu().numpy()[mids]), out["counts"][rows, 1])
    if vis is not None:
        assert np.array_equal(pop(sw & vis.bits.cpu().numpy()[mids]), out["counts"][rows, 2])
        assert np.array_equal(vis.area.cpu().numpy()[mids], out["counts"][rows, 4])
    assert np.array_equal(full.area.cpu().numpy()[mids], out["counts"][rows, 3])
    live = [i for i, b in enumerate(rows) if out["ok"][b]]
    iou = coco_eval.mask_ious(sil, full, np.stack([np.array(rows)[live], mids[live]], 1)).cpu().numpy()
    assert np.array_equal(iou.view(np.uint64), out["iou"][np.array(rows)[live]].view(np.uint64))


def test_not_counted_rows_are_exact():
    for name in ("edges_a_9", "edges_b_9"):
        case, D, out = _run(name)
        nan_bits = np.array([np.nan]).view(np.uint64)[0]
        for b in range(2, 7):
            assert out["score"][b:b + 1].view(np.uint64)[0] == nan_bits == out["iou"][b:b + 1].view(np.uint64)[0] == out["cover"][b:b + 1].view(np.uint64)[0]
            assert not out["ok"][b] and not out["counts"][b, :3].any() and (out["box"][b] == -1).all() and not (out["labels"][b] & 1).any()
        assert not out["labels"][4].any() and out["counts"][4].tolist() == [0] * 5                         # an invalid mask id: zeros
        F, Vm = case.masks(D)
        assert np.array_equal(out["labels"][3], F[1] * np.uint8(2) + Vm[1] * np.uint8(4)) and out["counts"][3, 3] == F[1].sum()      # status 0: still its mask bits
        assert D[3].any() and D[4].any() and not D[2].any() and not D[5].any() and not D[6].any()          # 3, 4: rendered, yet not counted
        assert out["ok"][1] and out["score"][1] == 0.0 and out["counts"][1].tolist()[:3] == [0, 0, 0] and out["ok"][0] and out["ok"][7]


@pytest.mark.parametrize("name", ["mixed_a_6", "mixed_b_5", "edges_a_9"])
def test_bitwise_identities(name):
    """a pose alone, in batches of 3 and in its whole batch, with and without the labels, from call to call: the same bits"""
    case, D, out = _run(name)
    assert _same(out, _device(case, D))
    plain = _device(case, D, return_labels=False)
    assert plain["labels"] is None and _same(dict(out, labels=None), plain)
    for b in range(case.P):
        assert _same(_rows(out, [b]), _device(case, D, idx=[b])), b
    for b0 in range(0, case.P, 3):
        rows = list(range(b0, min(b0 + 3, case.P)))
        assert _same(_rows(out, rows), _device(case, D, idx=rows)), rows
    rev = np.arange(case.P)[::-1].copy()
    assert _same(_rows(out, rev), _device(case, D, idx=rev))
    if case.holes is not None:                                                    # without the visible masks: the other outputs keep their bits
        bare = _device(case, D, visible=None)
        assert np.array_equal(bare["counts"][:, [0, 1, 3]], out["counts"][:, [0, 1, 3]]) and not bare["counts"][:, [2, 4]].any() and np.isnan(bare["cover"]).all()
        assert np.array_equal(bare["score"], out["score"], equal_nan=True) and np.array_equal(bare["labels"], out["labels"] & 3)


def test_select_poses_on_the_scores():
    from checkerpose_amd import postprocess as Q
    for name in ("select_a", "select_b"):
        case, D, out = _run(name)
        want = VM.reference(case, D)
        assert out["choice"].tolist() == want["choice"].tolist() == VM.select(out["score"].reshape(case.cand), out["ok"].reshape(case.cand)).tolist()
    case, D, out = _run("select_a")
    s = out["score"].reshape(case.cand)
    assert s[1, 0] == s[2, 0] > s[0, 0] and out["choice"].tolist() == [1, 0]       # an exact tie made on the device: the same pose twice
    a = _args(case, D)
    score, info = Q.verify_poses_mask(**dict(a, return_labels=False))
    C_, B = case.cand
    choice, Rs, ts = Q.select_poses(score.view(C_, B), info["ok"].view(C_, B), a["R"].view(C_, B, 3, 3), a["t"].view(C_, B, 3, 1))
    assert choice.cpu().tolist() == [1, 0] and torch.equal(Rs[0], a["R"][2]) and torch.equal(Rs[1], a["R"][1])


def test_refusals_on_the_device():
    from checkerpose_amd import coco_eval
    from checkerpose_amd import postprocess as Q
    case, D, _ = _run("mixed_a_6")
    a = _args(case, D)
    for name, bad in (("status", torch.ones(2, dtype=torch.int32, device=DEV)), ("mask_ids", [0, 1, 2, 3, 4, 0]), ("mask_ids", [0, 1]), ("mask_ids", None),
                      ("mesh_ids", [0, 1, 2, 0, 1, 3]), ("mask_ids", torch.zeros(5, dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError, match="masks for" if bad is None else name):
            Q.verify_poses_mask(**dict(a, **{name: bad}))
    with pytest.raises(ValueError, match="visible"):
        Q.verify_poses_mask(**dict(a, visible=coco_eval.pack_masks(torch.zeros(4, 50, 70, dtype=torch.uint8, device=DEV))))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.verify_poses_mask(**dict(a, R=a["R"].cpu()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.verify_poses_mask(**dict(a, status=torch.ones(6, dtype=torch.int32)))
    cpu = coco_eval.PackedMasks(a["full"].bits.cpu(), a["full"].area.cpu(), a["full"].box.cpu(), 80, 96)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.verify_poses_mask(**dict(a, full=cpu, visible=None))


# ------------------------------------------------------------------------------------------------------------------ the caller
def test_estimate_poses_mask_verified_is_the_composition_of_its_parts():
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
    spec = dict(meshes=ms, mesh_ids=mesh_ids)
    kw = dict(img_index=idx, seed=3, resize_method="crop_resize")
    B = 4
    plain = Q.estimate_poses(net, frames, boxes, p3d, K, **kw)
    assert all(torch.equal(x, y) for x, y in zip(plain[:4], Q.estimate_poses_mask_verified(net, frames, boxes, p3d, K, spec, **kw)[:4]))      # refine=None: one candidate
    for use_visible in (True, False):
        keep = {}
        stages, inl, status, final = Q._estimate_stages(net, frames, boxes, p3d, K, refine="lm", keep=keep, **kw)
        masks = Q.estimate_poses_masks(net, frames, boxes, p3d, K, channel=1, **kw)[5]                     # the pastes of a separate forward
        vis = Q.estimate_poses_masks(net, frames, boxes, p3d, K, channel=0, **kw)[5] if use_visible else None
        R, t, inl2, status2, final2, rep = Q.estimate_poses_mask_verified(net, frames, boxes, p3d, K, dict(spec, use_visible=use_visible), return_verify=True,
                                                                          refine="lm", **kw)
        assert torch.equal(inl2, inl) and torch.equal(status2, status) and np.array_equal(final2, final) and rep["stages"] == ("solver", "lm")
        assert torch.equal(rep["full"].bits, masks.bits) and torch.equal(rep["full"].area, masks.area)
        assert (rep["visible"] is None) if vis is None else torch.equal(rep["visible"].bits, vis.bits)
        Rc, tc = torch.stack([s[1] for s in stages]), torch.stack([s[2] for s in stages])
        score, info = Q.verify_poses_mask(Rc.reshape(2 * B, 3, 3), tc.reshape(2 * B, 3, 1), K, ms, masks, visible=vis, mask_ids=list(range(B)) * 2,
                                          mesh_ids=mesh_ids * 2, status=status.repeat(2))
        choice, R2, t2 = Q.select_poses(score.view(2, B), info["ok"].view(2, B), Rc, tc)
        assert np.array_equal(rep["score"].cpu().numpy(), score.view(2, B).cpu().numpy(), equal_nan=True) and torch.equal(rep["choice"], choice)
        assert all(torch.equal(rep["info"][k], info[k]) for k in VM.COUNTS + ("ok", "box"))
        assert torch.equal(R, R2) and torch.equal(t, t2) and tuple(R.shape) == (B, 3, 3) and tuple(t.shape) == (B, 3, 1)
        pick = choice.cpu().tolist()
        assert all(torch.equal(R[b], stages[pick[b]][1][b]) and torch.equal(t[b], stages[pick[b]][2][b]) for b in range(B))      # the chosen candidate's bits
        assert all(pick[b] == 0 for b in range(B) if int(status[b]) == 0)                                  # the fallback never loses its place
    with pytest.raises(NotImplementedError, match="warp_affine"):
        Q.estimate_poses_mask_verified(net, frames, boxes, p3d, K, spec, img_index=idx, resize_method="crop_resize_by_warp_affine")
