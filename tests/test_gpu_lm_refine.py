"""GPU: row N22 on the device.  refine_poses_lm replayed one iteration at a time from its own records (tests/lm_stages.py) over the
thread-stride and minimum-count edges, batch sizes, shared and per-crop models / intrinsics and iteration bounds, started from
solve_pnp_ransac's own output (noisy crops with outliers) and from perturbed truths (noise-free crops); the bitwise pass-throughs;
the exact properties and bitwise identities of the call; its callers; pose_covariance; the refusals."""
import numpy as np
import pytest
import torch

from tests import lm_stages as L
from tests import pnp_stages as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_CACHE = {}


def _case(name):
    """a committed case; the noisy ones start from the DEVICE solver's poses over its inliers"""
    if name in _CACHE:
        return _CACHE[name]
    from checkerpose_amd.postprocess import solve_pnp_ransac
    case = L.CASES[name]()
    if case.mask is None:
        R, t, inl, status = solve_pnp_ransac(torch.from_numpy(case.p3d).float().to(DEV), torch.from_numpy(case.p2d).float().to(DEV),
                                             torch.from_numpy(case.valid).to(DEV), torch.from_numpy(case.K).float().to(DEV), seed=case.seed)
        case.with_start(R.cpu().numpy(), t.cpu().numpy(), inl.cpu().numpy(), status.cpu().numpy())
        assert case.status_in.all() and (case.mask.sum(1) > 0.5 * case.N).all()             # the inputs are what the test is named after
    _CACHE[name] = case
    return case


def _args(case, first=None, uint8=False):
    n = case.B if first is None else first
    mask = torch.from_numpy(case.mask[:n]).to(DEV)
    return dict(p3d_xyz=torch.from_numpy(case.p3d[:n] if case.p3d.ndim == 3 else case.p3d).float().to(DEV),
                p2d=torch.from_numpy(case.p2d[:n]).float().to(DEV), mask=mask if uint8 else mask.bool(),
                cam_K=torch.from_numpy(case.K[:n] if case.K.ndim == 3 else case.K).float().to(DEV),
                R=torch.from_numpy(case.R0[:n]).to(DEV), t=torch.from_numpy(case.t0[:n]).to(DEV),
                status=None if case.status_in is None else torch.from_numpy(case.status_in[:n]).to(DEV),
                max_iters=case.max_iters, step_tol=case.step_tol, return_records=True)


def _device_run(case, **kw):
    from checkerpose_amd.postprocess import refine_poses_lm
    R, t, status, info, rec = refine_poses_lm(**_args(case, **kw))
    torch.cuda.synchronize()
    flat = torch.cat([info["cost0"][:, None], info["cost"][:, None], info["n"][:, None].double(), info["iters"][:, None].double(),
                      info["H"].reshape(-1, 36)], 1)
    assert tuple(R.shape) == (len(status), 3, 3) and tuple(t.shape) == (len(status), 3, 1) and status.dtype == torch.int32
    assert info["status"] is status and R.dtype == t.dtype == torch.float64
    return [rec.cpu().numpy(), R.cpu().numpy(), t.cpu().numpy()[:, :, 0], status.cpu().numpy(), flat.cpu().numpy()]


def _bitwise(a, b, n=None):
    return all(np.array_equal(x[:n], y[:n], equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(L.CASES))
def test_device_stages(name):
    case = _case(name)
    rec, R, t, status, info = _device_run(case)
    assert rec.shape == (case.B, case.max_iters, L.REC)
    total = L.check_case(case, rec, R, t, status, info, log=print)
    refined = status != 0
    # the exact properties
    assert (info[refined, 1] <= info[refined, 0]).all()
    assert (np.abs(np.einsum("bji,bjk->bik", R[refined], R[refined]) - np.eye(3)) <= 1e-12).all()
    if name.startswith("exact") and case.max_iters == 20:
        assert (status == 1).all() and total["accepted"] >= 3 * case.B
    if name.startswith("noisy") and case.max_iters >= 20:
        assert (status == 1).all()
    if name in ("exact_it1", "exact_it2", "noisy_it1", "noisy_it2", "origin_it5"):
        assert (status == 2).all() and (info[:, 3] == case.max_iters).all()
    if name == "origin":
        assert (status == 3).all() and (info[:, 3] == 12).all()
    if name == "passthrough":
        assert status.tolist()[1:6] == [0] * 5 and status[0] != 0 and status[6] != 0
    if name == "behind_camera":
        assert status.tolist() == [0, 0]


def test_pass_throughs_are_bitwise():
    for name in ("passthrough", "behind_camera"):
        case = _case(name)
        rec, R, t, status, info = _device_run(case)
        for b in np.nonzero(status == 0)[0]:
            assert np.array_equal(R[b].view(np.uint64), case.R0[b].view(np.uint64)), (name, b)             # NaN payloads included
            assert np.array_equal(t[b].view(np.uint64), case.t0[b].view(np.uint64)), (name, b)
            assert np.isnan(rec[b]).all()
    # the identity fallback of a solver stays the identity: three valid points -> solve_pnp_ransac's status 0
    from checkerpose_amd.postprocess import refine_poses_lm, solve_pnp_ransac
    case = _case("exact_3x256")
    a = _args(case)
    valid = torch.zeros(case.B, case.N, 3, dtype=torch.uint8, device=DEV)
    valid[1:, :, 0] = 1
    valid[0, :3, 0] = 1
    R, t, inl, st = solve_pnp_ransac(a["p3d_xyz"], a["p2d"], valid, a["cam_K"], seed=1)
    assert st.tolist() == [0, 1, 1]
    R2, t2, st2, info = refine_poses_lm(a["p3d_xyz"], a["p2d"], valid[:, :, 0].contiguous(), a["cam_K"], R, t, status=st)
    assert st2[0] == 0 and torch.equal(R2[0], torch.eye(3, dtype=torch.float64, device=DEV)) and not t2[0].any() and (st2[1:] != 0).all()


def test_bitwise_identities():
    from checkerpose_amd import _abi
    case = _case("exact_33x512")
    a = _device_run(case)
    assert _bitwise(a, _device_run(case))                                        # two calls
    assert _bitwise(a, _device_run(case, first=1), 1)                            # crop 0 alone == crop 0 inside its batch
    assert _bitwise(a, _device_run(case, uint8=True))                            # a uint8 mask == a bool mask
    lm = _case("exact_3x4096_lm")                                                # per-crop models and intrinsics
    assert _bitwise(_device_run(lm), _device_run(lm, first=2), 2)
    # the `out` buffers are not read: the same call through the C ABI into buffers filled with 0, NaN and 1e300
    lib = _abi.load()
    g = _args(case)
    B, N = case.B, case.N
    pin = torch.cat([g["R"].reshape(B, 9), g["t"].reshape(B, 3)], 1).contiguous()
    mk = g["mask"].contiguous().view(torch.uint8)
    outs = []
    for fill in (0.0, float("nan"), 1e300):
        pose = torch.full((B, 12), fill, dtype=torch.float64, device=DEV)
        info = torch.full((B, L.INFO), fill, dtype=torch.float64, device=DEV)
        st = torch.full((B,), 77, dtype=torch.int32, device=DEV)
        rec = torch.full((B, case.max_iters, L.REC), float("nan"), dtype=torch.float64, device=DEV)
        _abi.check(lib.cp_pnp_refine_lm(torch.cuda.current_stream(DEV).cuda_stream, g["p3d_xyz"].data_ptr(), 0, g["p2d"].data_ptr(), mk.data_ptr(), 1,
                                        g["cam_K"].data_ptr(), 0, B, N, pin.data_ptr(), None, case.max_iters, case.step_tol, pose.data_ptr(),
                                        st.data_ptr(), info.data_ptr(), rec.data_ptr()), "cp_pnp_refine_lm")
        torch.cuda.synchronize()
        outs.append([rec.cpu().numpy(), pose[:, :9].reshape(B, 3, 3).cpu().numpy(), pose[:, 9:].cpu().numpy(), st.cpu().numpy(), info.cpu().numpy()])
    assert _bitwise(a, outs[0]) and _bitwise(a, outs[1]) and _bitwise(a, outs[2])
    # in place: pose_out == pose_in
    pose = pin.clone()
    info = torch.empty(B, L.INFO, dtype=torch.float64, device=DEV)
    st = torch.empty(B, dtype=torch.int32, device=DEV)
    _abi.check(lib.cp_pnp_refine_lm(torch.cuda.current_stream(DEV).cuda_stream, g["p3d_xyz"].data_ptr(), 0, g["p2d"].data_ptr(), mk.data_ptr(), 1,
                                    g["cam_K"].data_ptr(), 0, B, N, pose.data_ptr(), None, case.max_iters, case.step_tol, pose.data_ptr(),
                                    st.data_ptr(), info.data_ptr(), None), "cp_pnp_refine_lm")
    torch.cuda.synchronize()
    assert np.array_equal(pose[:, :9].reshape(B, 3, 3).cpu().numpy(), a[1]) and np.array_equal(info.cpu().numpy(), a[4])


def test_refined_poses_are_no_worse_on_noisy_crops():
    """not an acceptance number of the row, a sanity check of its sign: over the inliers, the refined pose's cost is below the start's"""
    case = _case("noisy_3x512")
    rec, R, t, status, info = _device_run(case)
    assert (info[:, 1] < info[:, 0]).all()


def test_pose_covariance_against_the_host():
    from checkerpose_amd.postprocess import pose_covariance, refine_poses_lm
    case = _case("passthrough")
    R, t, status, info = refine_poses_lm(**dict(_args(case), return_records=False))
    cov = pose_covariance(info)
    assert cov.is_cuda and tuple(cov.shape) == (case.B, 6, 6) and cov.dtype == torch.float64
    H, cost, n = info["H"].cpu(), info["cost"].cpu(), info["n"].cpu()
    for b in range(case.B):
        if int(status[b]) == 0:
            assert torch.isnan(cov[b]).all()
            continue
        # two LU inversions of H (rotation entries ~1e5, translation entries ~1: a condition number up to ~1e8) agree to about
        # cond x eps = 1e-8 of sqrt(C_ii C_jj); 1e-6 leaves two orders
        inv = torch.linalg.inv(H[b])
        scale = torch.sqrt(torch.outer(torch.diag(inv), torch.diag(inv)))
        want = cost[b] / (2 * n[b] - 6) * inv
        assert ((cov[b].cpu() - want).abs() <= 1e-6 * cost[b] / (2 * n[b] - 6) * scale).all()
        assert ((pose_covariance(info, sigma=0.5)[b].cpu() - 0.25 * inv).abs() <= 1e-6 * 0.25 * scale).all()
    assert int((status != 0).sum()) == 2


def test_refusals_on_the_device():
    from checkerpose_amd.postprocess import refine_poses_lm
    a = dict(_args(_case("exact_3x7")), return_records=False)
    for name, bad in (("max_iters", 0), ("max_iters", 65), ("step_tol", 0.0), ("step_tol", float("nan")), ("mask", a["mask"][:, :6]),
                      ("R", a["R"][:2]), ("status", torch.ones(2, dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError, match=name):
            refine_poses_lm(**dict(a, **{name: bad}))
    with pytest.raises(ValueError, match="p3d_xyz"):
        refine_poses_lm(**dict(a, p3d_xyz=torch.zeros(8, 3, device=DEV)))
    with pytest.raises(ValueError, match="p3d_xyz"):
        refine_poses_lm(**dict(a, cam_K=torch.eye(3, device=DEV).expand(2, 3, 3)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine_poses_lm(**dict(a, mask=a["mask"].cpu()))


# ------------------------------------------------------------------------------------------------------------ the callers
@pytest.mark.parametrize("solver", ["epnp", "gc"])
def test_estimate_poses_refine_is_the_composition_of_its_steps(solver):
    from checkerpose_amd import postprocess as Q, preprocess as PP
    from checkerpose_amd.synthetic import build_net
    rng = np.random.default_rng(9)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 480, 640, 3), dtype=np.uint8)).cuda()
    boxes = [[100, 80, 120, 90], [300, 200, 60, 140], None, [-10, 400, 90, 90]]
    idx = [0, 1, 0, 1]
    net = build_net(npoint=512, seed=1).cuda().eval()
    net.set_compute_dtype("bf16")
    p3d = torch.from_numpy(S.lmo_model(512).astype(np.float32)).cuda()
    K = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]], dtype=np.float32)
    kw = dict(img_index=idx, seed=3)
    if solver == "gc":
        kw.update(solver="gc", graph=Q.radius_graph(p3d, 20.0), spatial_coherence_weight=0.05, prog_max_iters=128)
    plain = Q.estimate_poses(net, frames, boxes, p3d, K, **kw)
    none = Q.estimate_poses(net, frames, boxes, p3d, K, refine=None, **kw)
    assert all(torch.equal(x, y) for x, y in zip(plain[:4], none[:4])) and np.array_equal(plain[4], none[4])
    R, t, inl, status, final = Q.estimate_poses(net, frames, boxes, p3d, K, refine="lm", **kw)
    assert torch.equal(inl, plain[2]) and torch.equal(status, plain[3]) and np.array_equal(final, plain[4])
    padded = [None if b is None else PP.padding_Bbox(b, 1.5) for b in boxes]
    crops = PP.get_roi_batch(frames, padded, 256, PP.INTER_LINEAR, "crop_square_resize", img_index=idx)
    with torch.no_grad():
        out = net(crops, None)
    p2d, valid, _ = Q.correspondences(out, Bboxes=final)
    R2, t2, st2, info = Q.refine_poses_lm(p3d, p2d, plain[2], K, plain[0], plain[1], status=plain[3])
    assert torch.equal(R, R2) and torch.equal(t, t2) and tuple(R.shape) == (4, 3, 3) and tuple(t.shape) == (4, 3, 1)
    assert (st2[plain[3] == 0] == 0).all()
    E = Q.evaluate_poses(net, frames, boxes, p3d, K, R2, t2, p3d.cpu().numpy(), kinds=("add",), refine="lm", **kw)
    assert torch.equal(E[1], R2) and float(E[0]["add"].abs().max()) == 0.0


def test_from_id_to_pose_refine_is_the_batched_call():
    from checkerpose_amd.postprocess import from_id_to_pose, radius_graph, refine_poses_lm, solve_pnp_gc, solve_pnp_ransac
    case = L.CASES["noisy_3x512"]()
    p3, p2, K = case.p3d, case.p2d[0], case.K
    roi_xy = p2.astype(np.float32)[None]
    xid, yid = np.arange(case.N), np.zeros(case.N, np.int64)
    bit = np.ones((case.N, 1), np.float32)
    d3, d2, dK = torch.from_numpy(p3).float().to(DEV), torch.from_numpy(p2).float().to(DEV)[None], torch.from_numpy(K).float().to(DEV)
    valid = torch.zeros(1, case.N, 3, dtype=torch.uint8, device=DEV)
    valid[0, :, 0] = 1
    # the cv2 twin
    common = (p3.astype(np.float32), roi_xy, K.astype(np.float32), bit, xid, yid)
    plain = from_id_to_pose(*common, return_inliers=True, seed=5)
    none = from_id_to_pose(*common, return_inliers=True, seed=5, refine=None)
    assert all(np.array_equal(x, y) for x, y in zip(plain, none))
    Rf, tf, inl = from_id_to_pose(*common, return_inliers=True, seed=5, refine="lm")
    R, t, im, st = solve_pnp_ransac(d3, d2, valid, dK, seed=5)
    R2, t2, st2, _ = refine_poses_lm(d3, d2, im, dK, R, t, status=st)
    assert int(st[0]) == 1 and int(st2[0]) != 0 and np.array_equal(inl, plain[2])
    assert np.array_equal(Rf, R2[0].cpu().numpy()) and np.array_equal(tf, t2[0].cpu().numpy()) and tf.shape == (3, 1)
    assert not np.array_equal(Rf, plain[0])
    # the graph-cut backend, on the noise-free crop its own caller test uses (tests/test_gpu_pnp_gc.py)
    from tests import gc_stages as G
    gc = G.CASES["outliers_0.3"]()
    p3, p2, va, K = gc.case.crop(0)
    common = (p3.astype(np.float32), p2.astype(np.float32)[None], K.astype(np.float32), va.astype(np.float32)[:, None], np.arange(gc.N), np.zeros(gc.N, np.int64))
    gkw = dict(use_progressivex=True, progx_backend="device", neighborhood_ball_radius=20, spatial_coherence_weight=gc.lam, prog_max_iters=400,
               reprojErr_thresh=2, seed=gc.case.seed)
    plain = from_id_to_pose(*common, **gkw)
    none = from_id_to_pose(*common, refine=None, **gkw)
    assert np.array_equal(plain[0], none[0]) and np.array_equal(plain[1], none[1])
    Rf, tf = from_id_to_pose(*common, refine="lm", **gkw)
    d3, d2, dK = torch.from_numpy(p3).float().to(DEV), torch.from_numpy(p2).float().to(DEV)[None], torch.from_numpy(K).float().to(DEV)
    valid = torch.zeros(1, gc.N, 3, dtype=torch.uint8, device=DEV)
    valid[0, :, 0] = torch.from_numpy(va).to(DEV)
    R, t, im, st = solve_pnp_gc(d3, d2, valid, dK, radius_graph(d3, 20.0), spatial_coherence_weight=gc.lam, iterations=400, seed=gc.case.seed)
    R2, t2, st2, _ = refine_poses_lm(d3, d2, im, dK, R, t, status=st)
    assert int(st[0]) == 1 and int(st2[0]) != 0
    assert np.array_equal(Rf, R2[0].cpu().numpy()) and np.array_equal(tf, t2[0].cpu().numpy())
    Rt, tt, _ = gc.case.truth[0]
    assert np.abs(Rf - Rt).max() <= S.e_margins()[0] and np.linalg.norm(tf[:, 0] - tt) <= S.e_margins()[1] * np.linalg.norm(tt)
    common = common[:3]
    bit, xid, yid, roi_xy = np.ones((gc.N, 1), np.float32), np.arange(gc.N), np.zeros(gc.N, np.int64), p2.astype(np.float32)[None]
    # fewer than 4 valid points: still the identity
    few = np.zeros_like(bit)
    few[:3] = 1.0
    Ri, ti = from_id_to_pose(common[0], roi_xy, common[2], few, xid, yid, refine="lm")
    assert np.array_equal(Ri, np.eye(3)) and not ti.any()
