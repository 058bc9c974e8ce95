"""GPU: row N25 on the device.  lift_correspondences bit for bit against the numpy restatement; solve_pose_depth replayed from its own
records (tests/depth_pose_stages.py) over the committed cases -- 3, 5, 64, 512 and 4096 keypoints, batches that share images, shared and
per-crop intrinsics, iteration counts at the round boundaries, a depth image with an occluder slab, holes, NaN and zeros --; the
fallbacks, bitwise; seed determinism; estimate_poses(solver="depth") against the composition of its parts; the converging crops' ADD."""
import numpy as np
import pytest
import torch

from tests import depth_pose_stages as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_RUNS = {}


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _args(case, **over):
    a = dict(p3d_xyz=_up(case.p3d), p2d=_up(case.p2d), valid=_up(case.valid), cam_K=_up(case.K), depth=_up(case.depth),
             dist_threshold=_up(np.asarray(case.thr, np.float64)) if np.ndim(case.thr) else case.thr, image_ids=case.image_ids, column=case.column,
             iterations=case.iterations, seed=case.seed, return_hypotheses=True)
    a.update(over)
    return a


def _flat(R, t, inl, status, rec):
    assert R.dtype == t.dtype == torch.float64 and inl.dtype == torch.bool and status.dtype == torch.int32
    B = len(status)
    assert tuple(R.shape) == (B, 3, 3) and tuple(t.shape) == (B, 3, 1)
    out = dict(R=R, t=t[:, :, 0], inliers=inl, status=status, **rec)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _device_run(case, **over):
    from checkerpose_amd.postprocess import solve_pose_depth
    return _flat(*solve_pose_depth(**_args(case, **over)))


def _run(name):
    """a committed case on the device, computed once and left unchanged"""
    if name not in _RUNS:
        _RUNS[name] = (D.make(name), _device_run(D.make(name)))
    return _RUNS[name]


# ------------------------------------------------------------------------------------------------------------------- stage A
@pytest.mark.parametrize("name", list(D.CASES))
def test_lift_is_the_restatement_bit_for_bit(name):
    from checkerpose_amd.postprocess import lift_correspondences
    case = D.make(name)
    a = _args(case)
    Q, lifted, n = lift_correspondences(a["p2d"], a["valid"], a["cam_K"], a["depth"], image_ids=a["image_ids"], column=case.column)
    assert Q.dtype == torch.float32 and lifted.dtype == torch.bool and n.dtype == torch.int32
    assert tuple(Q.shape) == (case.B, case.N, 3) and tuple(lifted.shape) == (case.B, case.N) and tuple(n.shape) == (case.B,)
    Q, lifted, n = Q.cpu().numpy(), lifted.cpu().numpy(), n.cpu().numpy()
    for b in range(case.B):
        Qn, ln = case.lifted(b)
        assert np.array_equal(lifted[b], ln), (name, b)
        assert np.array_equal(Q[b].view(np.uint32), Qn.view(np.uint32)), (name, b)
        assert n[b] == ln.sum()
    # the solver's own stage A is the same launch
    _, out = _run(name)
    assert np.array_equal(out["Q"].view(np.uint32), Q.view(np.uint32)) and np.array_equal(out["lifted"] != 0, lifted) and np.array_equal(out["n_lifted"], n)


# ------------------------------------------------------------------------------------------------------------- stages B and C
@pytest.mark.parametrize("name", list(D.CASES))
def test_replay_of_the_records(name):
    case, out = _run(name)
    res = D.check_case(case, out)
    print("%s: order (dR, dt) = %.3e %.3e, seen %.3e %.3e, %d hypotheses replayed" % ((name,) + res["order"] + res["seen"] + (res["hyps"],)))
    assert res["near"] == [], res["near"]
    ref = D.restatement_outputs(case)
    assert np.array_equal(out["status"], ref["status"])             # no decision near its boundary: the free-running rule decides alike
    assert np.array_equal(out["inliers"], ref["inliers"])


def test_fallbacks_are_the_identity_bitwise():
    from checkerpose_amd.postprocess import solve_pose_depth
    eye = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    seen = 0
    for name in ("two_lifted", "collinear", "three_lifted"):
        case, out = _run(name)
        for b in np.nonzero(out["status"] == 0)[0]:
            pose = np.concatenate([out["R"][b].reshape(9), out["t"][b]])
            assert np.array_equal(pose.view(np.uint64), eye.view(np.uint64)) and not out["inliers"][b].any(), (name, b)
            assert np.isnan(out["steps"][b]).all()
            seen += 1
    assert seen >= 4
    assert _run("collinear")[1]["status"].tolist() == [0] and (_run("collinear")[1]["hypotheses"][0, :, 0] == -1).all()
    assert _run("two_lifted")[1]["n_lifted"].tolist() == [2, 0] and np.isnan(_run("two_lifted")[1]["hypotheses"]).all()
    # a threshold entry that is not positive and finite: that crop alone falls back
    case, ref = _run("n64_b3")
    thr = _up(np.array([8.0, float("nan"), -1.0]))
    R, t, inl, status = solve_pose_depth(**_args(case, dist_threshold=thr, return_hypotheses=False))
    assert status.tolist() == [1, 0, 0] and not inl[1:].any()
    assert np.array_equal(R[0].cpu().numpy().view(np.uint64), ref["R"][0].view(np.uint64))
    assert np.array_equal(torch.cat([R[1:].reshape(2, 9), t[1:].reshape(2, 3)], 1).cpu().numpy().view(np.uint64), np.stack([eye, eye]).view(np.uint64))


def test_same_seed_same_bits():
    case, out = _run("n512_b5_slab")
    again = _device_run(case)
    for k in out:
        assert np.array_equal(out[k], again[k], equal_nan=True), k
    other = _device_run(case, seed=case.seed + 1)
    assert not np.array_equal(out["hypotheses"][:, :64], other["hypotheses"][:, :64], equal_nan=True)
    # the default path (no fill of the scratch, no records returned) gives the same bits
    from checkerpose_amd.postprocess import solve_pose_depth
    R, t, inl, status = solve_pose_depth(**_args(case, return_hypotheses=False))
    assert np.array_equal(R.cpu().numpy(), out["R"]) and np.array_equal(t.cpu().numpy()[:, :, 0], out["t"]) and np.array_equal(inl.cpu().numpy(), out["inliers"])


def test_converging_crops_reach_the_truth():
    """the feature's point, end to end: ADD of the device's pose to the truth (metric.pose_errors) is at most 2 x the ADD of the
    free-running numpy rule on the same crop (the margin is for summation order at ties)"""
    from checkerpose_amd import metric
    pairs = D.converging()
    assert len(pairs) >= 20
    for name in sorted({n for n, _ in pairs}):
        case, out = _run(name)
        ref = D.restatement_outputs(case)
        for b in case.converging:
            X = case.crop(b)[0]
            Rt, tt = case.truth[b]
            dev = float(metric.pose_errors(_up(out["R"][b:b + 1]), _up(out["t"][b:b + 1, :, None]), Rt[None], tt[None, :, None], X.astype(np.float32),
                                           kinds=("add",))["add"][0])
            own = D.add_error(X, ref["R"][b], ref["t"][b], Rt, tt)
            print("%s crop %d: ADD device %.4f, numpy rule %.4f" % (name, b, dev, own))
            assert out["status"][b] == 1 and dev <= 2.0 * own, (name, b, dev, own)
            assert own < 0.05 * np.linalg.norm(X, axis=1).max()         # and the rule itself is near the truth: 5 % of the model's radius


# ------------------------------------------------------------------------------------------------------------------ the callers
def test_refusals_on_the_device():
    from checkerpose_amd.postprocess import lift_correspondences, solve_pose_depth
    case = D.make("n64_b3")
    a = _args(case)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        solve_pose_depth(**dict(a, p2d=a["p2d"].cpu()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        solve_pose_depth(**dict(a, depth=a["depth"].cpu()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        solve_pose_depth(**dict(a, dist_threshold=torch.ones(3, dtype=torch.float64)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lift_correspondences(a["p2d"], a["valid"].cpu(), a["cam_K"], a["depth"], image_ids=a["image_ids"])
    with pytest.raises(ValueError, match="image_ids"):
        solve_pose_depth(**dict(a, image_ids=[0, 1, 2]))
    with pytest.raises(ValueError, match="need image_ids"):
        solve_pose_depth(**dict(a, image_ids=None))                 # 2 images for 3 crops
    with pytest.raises(ValueError, match="dist_threshold"):
        solve_pose_depth(**dict(a, dist_threshold=_up(np.ones(2))))
    # an empty batch: nothing is launched, the shapes are kept
    R, t, inl, status, rec = solve_pose_depth(a["p3d_xyz"], a["p2d"][:0], a["valid"][:0], a["cam_K"], a["depth"][:1], 8.0, return_hypotheses=True)
    assert tuple(R.shape) == (0, 3, 3) and tuple(t.shape) == (0, 3, 1) and tuple(inl.shape) == (0, 64) and tuple(status.shape) == (0,)
    assert tuple(rec["hypotheses"].shape) == (0, 150, 14) and tuple(rec["steps"].shape) == (0, 4, 14) and tuple(rec["Q"].shape) == (0, 64, 3)
    Q, lifted, n = lift_correspondences(a["p2d"][:0], a["valid"][:0], a["cam_K"], a["depth"][:1])
    assert tuple(Q.shape) == (0, 64, 3) and tuple(lifted.shape) == (0, 64) and tuple(n.shape) == (0,)


def test_estimate_poses_depth_is_the_composition_of_its_parts():
    from checkerpose_amd import postprocess as Q
    from checkerpose_amd import preprocess as PP
    from checkerpose_amd.synthetic import build_net
    from tests import pnp_stages as S
    rng = np.random.default_rng(9)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 480, 640, 3), dtype=np.uint8)).cuda()
    depth = torch.from_numpy(rng.uniform(300.0, 1500.0, (2, 480, 640)).astype(np.float32)).cuda()
    boxes = [[100, 80, 120, 90], [300, 200, 60, 140], None, [-10, 400, 90, 90]]
    idx = [0, 1, 0, 1]
    net = build_net(npoint=512, seed=1).cuda().eval()
    net.set_compute_dtype("bf16")
    p3d = torch.from_numpy(S.lmo_model(512).astype(np.float32)).cuda()
    K = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]], dtype=np.float32)
    kw = dict(img_index=idx, seed=3)
    plain = Q.estimate_poses(net, frames, boxes, p3d, K, **kw)
    R, t, inl, status, final = Q.estimate_poses(net, frames, boxes, p3d, K, solver="depth", depth=depth, dist_threshold=400.0, iterations=65, **kw)
    assert np.array_equal(final, plain[4]) and tuple(R.shape) == (4, 3, 3) and tuple(t.shape) == (4, 3, 1)
    padded = [None if b is None else PP.padding_Bbox(b, 1.5) for b in boxes]
    crops = PP.get_roi_batch(frames, padded, 256, PP.INTER_LINEAR, "crop_square_resize", img_index=idx)
    with torch.no_grad():
        out = net(crops, None)
    p2d, valid, _ = Q.correspondences(out, Bboxes=final)
    parts = Q.solve_pose_depth(p3d, p2d, valid, K, depth, 400.0, image_ids=idx, iterations=65, seed=3)
    assert torch.equal(R, parts[0]) and torch.equal(t, parts[1]) and torch.equal(inl, parts[2]) and torch.equal(status, parts[3])
    assert int(status.sum()) >= 1                                   # (random depth under a wide threshold: some crop is solved)
    lm = Q.estimate_poses(net, frames, boxes, p3d, K, solver="depth", depth=depth, dist_threshold=400.0, iterations=65, refine="lm", **kw)
    R2, t2 = Q.refine_poses_lm(p3d, p2d, parts[2], K, parts[0], parts[1], status=parts[3])[:2]
    assert torch.equal(lm[0], R2) and torch.equal(lm[1], t2) and torch.equal(lm[2], inl) and torch.equal(lm[3], status)
    E = Q.evaluate_poses(net, frames, boxes, p3d, K, R, t, p3d.cpu().numpy(), kinds=("add",), solver="depth", depth=depth, dist_threshold=400.0,
                         iterations=65, **kw)
    assert torch.equal(E[1], R) and float(E[0]["add"].abs().max()) == 0.0
