"""GPU: row N30 on the device.  mask_extents, contour_samples and refine_poses_mask over the committed cases of
tests/mask_refine_stages.py -- two small frames ((96, 80): 3 x 3 tiles; (70, 50): a partial last word), grids 1, 5 and 64, several
meshes, shared and permuted mask ids, per-pose intrinsics, own / shifted silhouettes, empty / full-frame / one-pixel / checkerboard
masks, poses partly and wholly off the frame, behind the camera, with status 0, a mask id and a mesh id out of range, NaN.  The extents
and the samples' pixels EQUAL the numpy rule's on the device's own metric.render_depth, the depths bitwise; the refinement is replayed
from the device's records one iteration at a time (the tolerance route: tests/mask_refine_stages.py says why); the identities (alone /
batches of 3 / all, with / without records); the caller against the composition of its parts."""
import numpy as np
import pytest
import torch

from tests import icp_stages as I
from tests import mask_refine_stages as MR

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


def _ids(ids, idx, n):
    """host ids are checked by the wrapper; ids that name nothing travel as a resident tensor and reach the kernel"""
    if ids is None:
        return None
    ids = np.asarray(ids)[idx].astype(np.int32)
    return _up(ids) if (ids >= n).any() else ids


def _packed(case):
    from checkerpose_amd import coco_eval
    return coco_eval.pack_masks(_up(case.masks.astype(np.uint8)))


def _args(case, idx=None, **over):
    idx = np.arange(case.P) if idx is None else np.asarray(idx)
    whole = len(idx) == case.P and (idx == np.arange(case.P)).all()
    mids = _ids(case.mask_ids, idx, len(case.masks)) if case.mask_ids is not None else (None if whole and len(case.masks) == case.P else idx.astype(np.int32))
    a = dict(R=_up(case.R0[idx]), t=_up(case.t0[idx]), cam_K=_up(case.K[idx] if case.K.ndim == 3 else case.K), meshes=_meshset(case), full=_packed(case),
             max_dist=case.max_dist, dof=case.dof, mask_ids=mids, mesh_ids=_ids(case.mesh_ids, idx, len(case.meshes)),
             status=None if case.status_in is None else _up(case.status_in[idx]), grid=case.grid, max_iters=case.max_iters, step_tol=case.step_tol,
             min_pairs=case.min_pairs, return_records=True)
    a.update(over)
    return a


def _device(case, idx=None, **over):
    """refine_poses_mask on the device -> dict of numpy arrays (records None without them) and the per-pose samples"""
    from checkerpose_amd import postprocess as Q
    a = _args(case, idx, **over)
    res = Q.refine_poses_mask(**a)
    R, t, status, info = res[:4]
    P = len(status)
    assert R.dtype == t.dtype == torch.float64 and tuple(R.shape) == (P, 3, 3) and tuple(t.shape) == (P, 3, 1) and status.dtype == torch.int32
    raw = torch.cat([info["cost0"][:, None], info["cost"][:, None], info["n_samples"][:, None].double(), info["n0"][:, None].double(),
                     info["n"][:, None].double(), info["iters"][:, None].double(), info["H"].reshape(P, 36)], 1).cpu().numpy()
    smp = {k: v.cpu().numpy() for k, v in info["samples"].items()}
    return dict(R=R.cpu().numpy(), t=t.cpu().numpy().reshape(P, 3), status=status.cpu().numpy(), info=raw,
                records=res[4].cpu().numpy() if a["return_records"] else None,
                samples=[{k: v[b] for k, v in smp.items()} for b in range(P)], extents={k: v.cpu().numpy() for k, v in info["extents"].items()})


def _renders(case):
    """the device's own depth renders of the case's poses -> (P,H,W) float32 numpy"""
    from checkerpose_amd import metric
    D = metric.render_depth(_up(case.R0), _up(case.t0), _up(case.K), _meshset(case), case.size, mesh_ids=_ids(case.mesh_ids, np.arange(case.P), len(case.meshes)))
    return D.cpu().numpy()


def _run(name):
    """a committed case on the device: (case, the device's renders, its outputs); computed once, left unchanged"""
    if name not in _RUNS:
        case = MR.make(name)
        _RUNS[name] = (case, _renders(case), _device(case))
    return _RUNS[name]


def _same(a, b, keys=("R", "t", "status", "info", "records")):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _rows(out, rows):
    return {k: (None if out[k] is None else out[k][rows]) for k in ("R", "t", "status", "info", "records")}


# ------------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name", list(MR.CASES))
def test_mask_extents_equal_the_rule(name):
    from checkerpose_amd import coco_eval
    from checkerpose_amd import postprocess as Q
    case = MR.make(name)
    want = [MR.extents(m) for m in case.masks]
    ext = Q.mask_extents(_packed(case))
    assert ext["row"].dtype == ext["col"].dtype == torch.int32
    assert np.array_equal(ext["row"].cpu().numpy(), np.stack([w[0] for w in want])) and np.array_equal(ext["col"].cpu().numpy(), np.stack([w[1] for w in want]))
    W, H = case.size
    dirty = coco_eval.PackedMasks(_up(MR.pack_bits(case.masks, dirty=True)), _up(case.masks.reshape(len(case.masks), -1).sum(1).astype(np.int32)), None, H, W)
    ext2 = Q.mask_extents(dirty)                                                  # bits at columns >= W are ignored
    assert torch.equal(ext2["row"], ext["row"]) and torch.equal(ext2["col"], ext["col"])


def test_mask_extents_on_paste_masks_output():
    from checkerpose_amd import coco_eval
    from checkerpose_amd import postprocess as Q
    rng = np.random.default_rng(3)
    seg = _up(rng.normal(size=(4, 2, 16, 16)).astype(np.float32))
    boxes = [[5, 4, 30, 28], [40, 10, 40, 30], [-8, 20, 30, 40], [0, 0, 70, 50]]
    for c in (0, 1):
        p = Q.paste_masks(seg, boxes, (50, 70), "crop_resize", channel=c)
        dense = coco_eval.unpack_masks(p).cpu().numpy().astype(bool)
        assert dense.any()
        ext = Q.mask_extents(p)
        want = [MR.extents(m) for m in dense]
        assert np.array_equal(ext["row"].cpu().numpy(), np.stack([w[0] for w in want])) and np.array_equal(ext["col"].cpu().numpy(), np.stack([w[1] for w in want]))


@pytest.mark.parametrize("name", list(MR.CASES))
def test_device_replays_the_rule(name):
    """stage A EQUAL on the device's own renders (depth bitwise metric.render_depth's), then the records one iteration at a time"""
    from checkerpose_amd import postprocess as Q
    case, D, out = _run(name)
    st = MR.check_case(case, out["samples"], out["records"], out["R"], out["t"], out["status"], out["info"], renders=list(D), log=print)
    cpu = MR.restatement_outputs(case, MR.case_samples(case)[0])
    print(name, "device status", out["status"].tolist(), "restatement free-running", cpu[3].tolist())
    assert st["iters"] > 0 or st["passed"] == case.P
    a = _args(case)
    alone = Q.contour_samples(a["R"], a["t"], a["cam_K"], a["meshes"], case.size, mesh_ids=a["mesh_ids"], grid=case.grid)      # stage A on its own: the same bits
    for k in ("rect", "shape", "pixel", "depth", "X", "ok"):
        assert np.array_equal(alone[k].cpu().numpy(), np.stack([s[k] for s in out["samples"]]), equal_nan=True), k
    want = [MR.extents(m) for m in case.masks]
    assert np.array_equal(out["extents"]["row"], np.stack([w[0] for w in want])) and np.array_equal(out["extents"]["col"], np.stack([w[1] for w in want]))


def test_what_the_device_did():
    case, D, out = _run("self_g5")
    assert (out["status"] != 0).all() and (out["info"][:, 3] == out["info"][:, 2]).all()                   # pairs = samples
    assert np.abs(out["R"] - case.R0).max() < 1e-9 and (np.abs(out["t"] - case.t0).max(1) < 1e-9 * case.t0[:, 2]).all()
    for name in ("near_t_g5", "shift_t_g64", "shift_t_g5"):
        case, D, out = _run(name)
        assert (out["status"] != 0).all() and np.array_equal(out["R"].view(np.uint64), case.R0.view(np.uint64))      # dof "t": R bitwise
    case, D, out = _run("edges_96")
    assert out["status"][0] != 0 and out["status"][1] != 0 and (out["status"][2:] == 0).all()
    assert np.array_equal(out["R"][2:].view(np.uint64), case.R0[2:].view(np.uint64)) and np.array_equal(out["t"][2:].view(np.uint64), case.t0[2:].view(np.uint64))
    assert not (np.stack([s["pixel"] for s in out["samples"]])[1][:, 0] == case.size[0] - 1).any() and (D[1] > 0)[:, case.size[0] - 1].any()
    case, D, out = _run("masks_70")
    assert out["status"][0] != 0 and (out["status"][1:4] == 0).all() and out["info"][2, 3] == 0
    case, D, out = _run("near_g1")
    assert (out["status"] == 0).all() and (out["info"][:, 2] == 4).all()


@pytest.mark.parametrize("name", ["near_rt_g64", "near_t_g5", "edges_96", "masks_70"])
def test_bitwise_identities(name):
    """a pose alone, in batches of 3 and in its whole batch, with and without the records, from call to call: the same bits"""
    case, D, out = _run(name)
    assert _same(out, _device(case))
    plain = _device(case, return_records=False)
    assert plain["records"] is None and _same(dict(out, records=None), plain)
    for b in range(case.P):
        assert _same(_rows(out, [b]), _device(case, idx=[b])), b
    for b0 in range(0, case.P, 3):
        rows = list(range(b0, min(b0 + 3, case.P)))
        assert _same(_rows(out, rows), _device(case, idx=rows)), rows
    rev = np.arange(case.P)[::-1].copy()
    assert _same(_rows(out, rev), _device(case, idx=rev))


def test_refusals_on_the_device():
    from checkerpose_amd import postprocess as Q
    case, D, _ = _run("near_t_g5")
    a = _args(case)
    for name, bad in (("status", torch.ones(2, dtype=torch.int32, device=DEV)), ("mask_ids", [0, 1, 2, 0]), ("mask_ids", [0, 1]), ("mask_ids", None),
                      ("mesh_ids", [0, 1, 2, 0]), ("max_dist", torch.ones(3, dtype=torch.float64, device=DEV))):
        with pytest.raises(ValueError, match="masks for" if bad is None else name):
            Q.refine_poses_mask(**dict(a, **{name: bad}))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.refine_poses_mask(**dict(a, R=a["R"].cpu()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.refine_poses_mask(**dict(a, max_dist=torch.ones(4, dtype=torch.float64)))
    per_pose = Q.refine_poses_mask(**dict(a, max_dist=torch.full((4,), case.max_dist, dtype=torch.float64, device=DEV)))
    assert torch.equal(per_pose[0], _up(_run("near_t_g5")[2]["R"])) and torch.equal(per_pose[1].reshape(4, 3), _up(_run("near_t_g5")[2]["t"]))


# ------------------------------------------------------------------------------------------------------------------ the caller
def test_estimate_poses_mask_refined_is_the_composition_of_its_parts():
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
    rspec = dict(max_dist=30.0, dof="t", grid=5)
    kw = dict(img_index=idx, seed=3, resize_method="crop_resize", refine="lm")
    B = 4
    stages, inl, status, final = Q._estimate_stages(net, frames, boxes, p3d, K, **kw)
    masks = Q.estimate_poses_masks(net, frames, boxes, p3d, K, channel=1, **kw)[5]                         # the pastes of a separate forward
    vis = Q.estimate_poses_masks(net, frames, boxes, p3d, K, channel=0, **kw)[5]
    R, t, inl2, status2, final2, rep = Q.estimate_poses_mask_refined(net, frames, boxes, p3d, K, rspec, spec, return_verify=True, **kw)
    assert torch.equal(inl2, inl) and torch.equal(status2, status) and np.array_equal(final2, final) and rep["stages"] == ("solver", "lm", "sil")
    assert torch.equal(rep["full"].bits, masks.bits) and torch.equal(rep["visible"].bits, vis.bits)
    Rs, ts, rstatus, rinfo = Q.refine_poses_mask(stages[-1][1], stages[-1][2], K, ms, masks, 30.0, "t", mesh_ids=mesh_ids, status=status, grid=5)
    assert torch.equal(rep["refine"][0], rstatus) and torch.equal(rep["refine"][1]["n0"], rinfo["n0"])
    print("refine status", rstatus.tolist(), "pairs", rinfo["n0"].tolist(), "solver status", status.tolist())
    cand = list(stages) + [("sil", Rs, ts)]
    Rc, tc = torch.stack([s[1].reshape(B, 3, 3) for s in cand]), torch.stack([s[2].reshape(B, 3, 1) for s in cand])
    st3 = torch.cat([status.repeat(2), torch.where(rstatus != 0, status, torch.zeros_like(status))])
    score, info = Q.verify_poses_mask(Rc.reshape(3 * B, 3, 3), tc.reshape(3 * B, 3, 1), K, ms, masks, visible=vis, mask_ids=list(range(B)) * 3,
                                      mesh_ids=mesh_ids * 3, status=st3)
    choice, R2, t2 = Q.select_poses(score.view(3, B), info["ok"].view(3, B), Rc, tc)
    assert np.array_equal(rep["score"].cpu().numpy(), score.view(3, B).cpu().numpy(), equal_nan=True) and torch.equal(rep["choice"], choice)
    assert torch.equal(R, R2) and torch.equal(t, t2) and tuple(R.shape) == (B, 3, 3) and tuple(t.shape) == (B, 3, 1)
    pick = choice.cpu().tolist()
    assert all(torch.equal(R[b], cand[pick[b]][1].reshape(B, 3, 3)[b]) for b in range(B)) and all(pick[b] == 0 for b in range(B) if int(status[b]) == 0)
    # the "sil" candidate removed by its status (a gate no sample passes: every refinement passes through): estimate_poses_mask_verified
    none = Q.estimate_poses_mask_refined(net, frames, boxes, p3d, K, dict(rspec, max_dist=1e-9), spec, return_verify=True, **kw)
    plain = Q.estimate_poses_mask_verified(net, frames, boxes, p3d, K, spec, return_verify=True, **kw)
    assert (none[5]["refine"][0] == 0).all() and all(torch.equal(x, y) for x, y in zip(none[:4], plain[:4])) and np.array_equal(none[4], plain[4])
    assert torch.equal(none[5]["choice"], plain[5]["choice"]) and np.array_equal(none[5]["score"][:2].cpu().numpy(), plain[5]["score"].cpu().numpy(), equal_nan=True)
    assert np.isnan(none[5]["score"][2].cpu().numpy()).all()


def test_estimate_poses_mask_refined_with_live_candidates(monkeypatch):
    """the small random net above gives masks without a single pair, so its "sil" candidates all pass through.  Here the forward and the
    paste are replaced by a committed case's poses and masks and everything behind them runs on the device: the refinement is live, the
    call is still bitwise the composition of its parts, and "sil" wins where the restatement's silhouette IoU rises (every pose of
    near_t_g5: tests/test_mask_refine.py::test_cost_and_iou)"""
    from checkerpose_amd import coco_eval
    from checkerpose_amd import postprocess as Q
    case = MR.make("near_t_g5")
    B = case.P
    W, H = case.size
    R0, t0 = _up(case.R0), _up(case.t0).reshape(B, 3, 1)
    status = torch.ones(B, dtype=torch.int32, device=DEV)
    masks = coco_eval.pack_masks(_up(case.masks[case.mask_ids].astype(np.uint8)))      # crop b's own mask

    def stages_stub(net, frames, Bboxes, p3d_xyz, cam_K, keep=None, **kw):
        keep["seg"], keep["padded"] = "SEG", "PADDED"
        return [("solver", R0, t0)], "inl", status, "final"

    monkeypatch.setattr(Q, "_estimate_stages", stages_stub)
    monkeypatch.setattr(Q, "paste_masks", lambda seg, boxes, size, method, channel: masks)
    frames = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV)
    ms, K = _meshset(case), _up(case.K)
    spec = dict(meshes=ms, mesh_ids=case.mesh_ids, use_visible=False)
    rspec = dict(max_dist=case.max_dist, dof=case.dof, grid=case.grid)
    R, t, inl, st, final, rep = Q.estimate_poses_mask_refined(None, frames, None, None, K, rspec, spec, return_verify=True)
    Rs, ts, rstatus, rinfo = Q.refine_poses_mask(R0, t0, K, ms, masks, case.max_dist, case.dof, mesh_ids=case.mesh_ids, status=status, grid=case.grid)
    want = _run("near_t_g5")[2]
    assert (rstatus != 0).all() and torch.equal(rep["refine"][0], rstatus) and rep["stages"] == ("solver", "sil")
    assert torch.equal(Rs, _up(want["R"])) and torch.equal(ts.reshape(B, 3), _up(want["t"]))      # the committed case's own refinement
    Rc, tc = torch.stack([R0, Rs]), torch.stack([t0, ts])
    score, info = Q.verify_poses_mask(Rc.reshape(2 * B, 3, 3), tc.reshape(2 * B, 3, 1), K, ms, masks, mask_ids=list(range(B)) * 2,
                                      mesh_ids=list(case.mesh_ids) * 2, status=status.repeat(2))
    choice, R2, t2 = Q.select_poses(score.view(2, B), info["ok"].view(2, B), Rc, tc)
    print("scores", score.view(2, B).cpu().numpy().round(4).tolist(), "choice", choice.cpu().tolist())
    assert torch.equal(rep["score"], score.view(2, B)) and torch.equal(rep["choice"], choice) and torch.equal(R, R2) and torch.equal(t, t2)
    assert choice.cpu().tolist() == [1] * B and torch.equal(R, Rs) and torch.equal(t, ts) and (score.view(2, B)[1] > score.view(2, B)[0]).all()
    assert inl == "inl" and st is status and final == "final"
