"""Row N33 on the device: rank_correspondences against np.lexsort bit for bit; every committed case of tests/cpnp_stages.py replayed
through its checker from the device's own records; the fallbacks, batching and record switch bitwise; the tie to row N4; the caller as
the composition of its parts."""
import numpy as np
import pytest
import torch

from tests import cpnp_stages as Cp
from tests import pnp_stages as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ------------------------------------------------------------------------------------------------------------- the ranking
def _lexsort_rank(s2, valid):
    """np.lexsort on (index, key) over the ranked points -> order (N,) int32 with -1 beyond nv, nv, n_dropped"""
    with np.errstate(invalid="ignore"):
        good = np.isfinite(s2).all(1) & (s2 > 0).all(1)
    idx = np.nonzero(valid.astype(bool) & good)[0]
    order = np.full(len(valid), -1, np.int32)
    with np.errstate(all="ignore"):
        order[:len(idx)] = idx[np.lexsort((idx, s2[idx, 0] + s2[idx, 1]))]
    return order, len(idx), int((valid.astype(bool) & ~good).sum())


RANK_KINDS = ("random", "all_equal", "blocks", "descending", "ascending", "bad", "none_valid", "all_valid")


def _rank_inputs(kind, B, N, seed):
    rng = np.random.default_rng(seed)
    s2 = rng.uniform(0.05, 50.0, size=(B, N, 2))
    valid = (rng.random((B, N, 3)) < 0.7).astype(np.uint8)
    if kind == "all_equal":
        s2[:] = 3.0
    elif kind == "blocks":
        s2[:] = np.repeat(rng.integers(1, 4, size=(B, N, 1)) * 0.25, 2, 2)
    elif kind in ("descending", "ascending"):
        ramp = np.arange(N, dtype=np.float64) + 1.0
        s2[:] = (ramp[::-1] if kind == "descending" else ramp)[None, :, None]
    elif kind == "bad":
        kinds = (np.nan, np.inf, 0.0, -1.0, -np.inf, -0.0, 5e-324, 1.7976931348623157e308)      # the last two are RANKED: finite and > 0
        for b in range(B):
            for j, i in enumerate(rng.choice(N, max(1, N // 3), replace=False)):
                s2[b, i, j % 2] = kinds[j % len(kinds)]
    elif kind == "none_valid":
        valid[:] = 0
    elif kind == "all_valid":
        valid[:] = 1
    return s2, valid


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 5, 63, 64, 65, 255, 256, 257, 1000, 4096])
def test_rank_is_lexsort_bit_for_bit(N, B):
    from checkerpose_amd.postprocess import rank_correspondences
    for k, kind in enumerate(RANK_KINDS):
        s2, valid = _rank_inputs(kind, B, N, 1000 * N + 10 * B + k)
        ds2, dvalid = _t(s2), _t(valid)
        for column in range(3):
            order, nr, nd = rank_correspondences(ds2, dvalid, column=column)
            assert order.dtype == nr.dtype == nd.dtype == torch.int32 and tuple(order.shape) == (B, N) and tuple(nr.shape) == tuple(nd.shape) == (B,)
            order, nr, nd = order.cpu().numpy(), nr.cpu().numpy(), nd.cpu().numpy()
            for b in range(B):
                want = _lexsort_rank(s2[b], valid[b, :, column])
                assert (nr[b], nd[b]) == want[1:], (kind, column, b)
                assert np.array_equal(order[b], want[0]), (kind, column, b)
                assert np.array_equal(order[b], Cp.rank(s2[b], valid[b, :, column])[0])
            if kind == "none_valid":
                assert not nr.any() and (order == -1).all()
            if kind == "all_valid":
                assert (nr == N).all() and not nd.any()
            if kind == "bad":
                assert nd.sum() > 0 or N < 63                 # (at N = 1 and 5 the few bad points may all be invalid)


# ------------------------------------------------------------------------------------------------------------- the solver
def _solve(case, rows=None, hypotheses=True, **kw):
    from checkerpose_amd.postprocess import solve_pnp_conf
    rows = slice(None) if rows is None else rows
    a = dict(p3d_xyz=_t(case.p3d[rows] if case.p3d.ndim == 3 else case.p3d, torch.float32), p2d=_t(case.p2d[rows], torch.float32),
             valid=_t(case.valid[rows]), sigma2=_t(case.sigma2[rows]), cam_K=_t(case.K[rows] if case.K.ndim == 3 else case.K, torch.float32),
             chi2_threshold=case.chi2, column=case.column, iterations=case.iterations, seed=case.seed, guided=case.guided,
             return_hypotheses=hypotheses)
    a.update(kw)
    out = solve_pnp_conf(**a)
    torch.cuda.synchronize()
    R, t, inl, status, info = out[:5]
    B = len(status)
    assert tuple(R.shape) == (B, 3, 3) and tuple(t.shape) == (B, 3, 1) and R.dtype == t.dtype == torch.float64
    assert inl.dtype == torch.bool and status.dtype == torch.int32 and set(info) == {"order", "n_ranked", "n_dropped"}
    o = dict(R=R.cpu().numpy(), t=t.cpu().numpy()[:, :, 0], inliers=inl.cpu().numpy(), status=status.cpu().numpy(),
             order=info["order"].cpu().numpy(), n_ranked=info["n_ranked"].cpu().numpy(), n_dropped=info["n_dropped"].cpu().numpy())
    if hypotheses:
        assert tuple(out[5].shape) == (B, case.iterations, 14)
        o["records"] = out[5].cpu().numpy()
    return o


def _bitwise(a, b, rows=None, keys=None):
    return all(np.array_equal(a[k][rows] if rows is not None else a[k], b[k], equal_nan=True) for k in (keys or b) if k in a)


_RUNS = {}


def _run(name):
    if name not in _RUNS:
        case = Cp.cached(name)[0]
        _RUNS[name] = (case, _solve(case))
    return _RUNS[name]


@pytest.mark.parametrize("name", list(Cp.CASES))
def test_device_replays_through_the_checker(name):
    case, o = _run(name)
    total = Cp.check_case(case, o, log=print)
    print("%s: worst refit difference %.3e (taus %.1e / %.1e)" % (name, total.get("refit_1e15", 0) * 1e-15, *S.taus()))
    want = Cp.cached(name)[1]
    assert np.array_equal(o["status"], want["status"]) or name.startswith("edge_")          # (degenerate data: the checker's stages decide)
    dropped = case.valid[:, :, case.column].astype(bool) & ~(np.isfinite(case.sigma2).all(2) & (case.sigma2 > 0).all(2))
    assert not (o["inliers"] & dropped).any()                                                 # dropped points never appear in inliers
    assert not (o["inliers"] & ~case.valid[:, :, case.column].astype(bool)).any()


def test_dropped_points_are_never_inliers_even_when_they_fit():
    """noise-free, no outliers: every valid point fits the pose, and the ones with a bad variance still stay out"""
    case, o = _run("bad_variances")
    ranked = np.zeros((case.B, case.N), bool)
    for b in range(case.B):
        ranked[b, o["order"][b, :o["n_ranked"][b]]] = True
    assert (o["n_dropped"] > 0).all() and (o["status"] == 1).all()
    out = np.stack([tr[2] for tr in case.truth])
    assert np.array_equal(o["inliers"], ranked & ~out)


def test_identity_and_p3p_crops_are_row_n4_bitwise():
    from checkerpose_amd.postprocess import solve_pnp_ransac
    for name in ("nv_0", "nv_3", "nv_4"):
        case, o = _run(name)
        R, t, inl, status = solve_pnp_ransac(_t(case.p3d, torch.float32), _t(case.p2d, torch.float32), _t(case.valid), _t(case.K, torch.float32),
                                             column=case.column, iterations=case.iterations, seed=case.seed)
        assert np.array_equal(o["R"], R.cpu().numpy()) and np.array_equal(o["t"], t.cpu().numpy()[:, :, 0]), name
        assert np.array_equal(o["inliers"], inl.cpu().numpy()) and np.array_equal(o["status"], status.cpu().numpy()), name
        assert np.isnan(o["records"]).all(), name                                              # no hypotheses below 5 ranked points
        assert (o["status"] == (1 if name == "nv_4" else 0)).all(), name
    # a P3P crop made by DROPPING: 6 valid points, two with a bad variance -> the four that remain, in ascending keypoint order
    case = Cp.cached("nv_6")[0]
    s2 = case.sigma2.copy()
    vid = np.nonzero(case.valid[0, :, 0])[0]
    s2[0, vid[1], 0], s2[0, vid[4], 1] = np.nan, 0.0
    o = _solve(case, sigma2=_t(s2))
    valid4 = case.valid.copy()
    valid4[0, vid[[1, 4]], 0] = 0
    R, t, inl, status = solve_pnp_ransac(_t(case.p3d, torch.float32), _t(case.p2d, torch.float32), _t(valid4), _t(case.K, torch.float32))
    assert o["n_ranked"].tolist() == [4] and o["n_dropped"].tolist() == [2] and o["status"].tolist() == [1] == status.cpu().tolist()
    assert np.array_equal(o["R"], R.cpu().numpy()) and np.array_equal(o["t"], t.cpu().numpy()[:, :, 0]) and np.array_equal(o["inliers"], inl.cpu().numpy())


@pytest.mark.parametrize("name", ["shape_3x257", "per_crop_K_p3d", "bad_variances", "unguided_3x65"])
def test_a_crop_alone_is_the_crop_in_its_batch(name):
    """the hash sampler takes the crop's index: crop 0 alone is crop 0 of the batch, bitwise, records included"""
    case, o = _run(name)
    alone = _solve(case, rows=slice(0, 1))
    assert _bitwise(o, alone, rows=slice(0, 1))


@pytest.mark.parametrize("name", ["shape_3x257", "iterations_150", "nv_4", "edge_coplanar"])
def test_results_do_not_depend_on_return_hypotheses(name):
    case, o = _run(name)
    plain = _solve(case, hypotheses=False)
    assert "records" not in plain and _bitwise(o, plain)


def test_one_large_batch():
    """B = 32, N = 512: every crop through the checker; more workgroups than one wave of the rank kernel's grid"""
    case = Cp._make("batch_32x512", 400, 32, 512, (0.3, 0.5, 0.7), iterations=150)
    o = _solve(case)
    total = Cp.check_case(case, o, log=print)
    assert total["status1"] >= 30 and total["all_inlier"] > 0


# ------------------------------------------------------------------------------------------------------------- tie to row N4
@pytest.mark.parametrize("name", ["shape_6x512", "shape_4x65", "thr_2", "outliers_0.6", "column_1"])
def test_unguided_equal_variances_are_row_n4(name):
    """guided=False, every variance 4.0, chi2 = thr^2 / 4: the counts are solve_pnp_ransac's outside the band, the masks equal, the pose
    within taus()"""
    from checkerpose_amd.postprocess import solve_pnp_conf, solve_pnp_ransac
    case = S.CASES[name]()
    a = (_t(case.p3d, torch.float32), _t(case.p2d, torch.float32), _t(case.valid))
    K = _t(case.K, torch.float32)
    kw = dict(column=case.column, iterations=case.iterations, seed=case.seed, return_hypotheses=True)
    R4, t4, inl4, st4, rec4 = solve_pnp_ransac(*a, K, reproj_threshold=case.thr, **kw)
    s2 = torch.full((case.B, case.N, 2), 4.0, dtype=torch.float64, device=DEV)
    thr = float(np.float32(case.thr))
    R, t, inl, st, info, rec = solve_pnp_conf(*a, s2, K, thr * thr / 4.0, guided=False, **kw)
    torch.cuda.synchronize()
    rec, rec4 = rec.cpu().numpy(), rec4.cpu().numpy()
    assert np.array_equal(np.isnan(rec[:, :, 0]), np.isnan(rec4[:, :, 0]))                     # the same records exist
    nv = case.valid[:, :, case.column].astype(bool).sum(1)
    assert np.array_equal(info["n_ranked"].cpu().numpy(), nv) and not info["n_dropped"].any()
    thr2 = thr * thr
    differ = 0
    for b in range(case.B):
        p3, p2, va, Kb = case.crop(b)
        vid = np.nonzero(va)[0]
        assert np.array_equal(info["order"][b, :nv[b]].cpu().numpy(), vid)                     # every key ties: the ascending valid list
        for h in np.nonzero(~np.isnan(rec[b, :, 0]))[0]:
            if rec[b, h, 0] == rec4[b, h, 0]:
                continue
            differ += 1                                       # allowed only where a point sits in the band under one of the two recorded poses
            assert rec[b, h, 0] >= 0 and rec4[b, h, 0] >= 0, (b, h)
            both = np.stack([rec[b, h, 2:14], rec4[b, h, 2:14]])
            d2 = S._sq_errors(p3[vid], p2[vid], Kb, both[:, :9].reshape(2, 3, 3), both[:, 9:])
            lo, hi = (d2 <= thr2 * (1 - S.BAND)).sum(1), (d2 <= thr2 * (1 + S.BAND)).sum(1)
            assert lo[0] <= rec[b, h, 0] <= hi[0] and lo[1] <= rec4[b, h, 0] <= hi[1], (b, h)
            assert max(lo[0], lo[1]) <= min(hi[0], hi[1]) and (hi > lo).any(), "counts %r / %r differ outside the band" % (rec[b, h, 0], rec4[b, h, 0])
    assert torch.equal(inl, inl4) and torch.equal(st, st4)
    ok = (st4 != 0).cpu().numpy()
    dR = float((R - R4).abs().max())
    dt = float((torch.linalg.norm((t - t4).reshape(-1, 3), dim=1).cpu()[ok] / torch.linalg.norm(t4.reshape(-1, 3), dim=1).cpu()[ok]).max()) if ok.any() else 0.0
    bits = torch.equal(R, R4) and torch.equal(t, t4) and np.array_equal(rec[:, :, [0] + list(range(2, 14))], rec4[:, :, [0] + list(range(2, 14))], equal_nan=True)
    print("%s: against solve_pnp_ransac |dR| %.3e |dt|/|t| %.3e, counts that differ %d, bits equal (pose and records): %s" % (name, dR, dt, differ, bits))
    assert dR <= S.taus()[0] and dt <= S.taus()[1]


# ------------------------------------------------------------------------------------------------------------- the caller
def test_estimate_poses_conf_is_the_composition_of_its_parts():
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
    plain = Q.estimate_poses(net, frames, boxes, p3d, K, **kw)                                 # existing behaviour: the final boxes
    padded = [None if b is None else PP.padding_Bbox(b, 1.5) for b in boxes]
    crops = PP.get_roi_batch(frames, padded, 256, PP.INTER_LINEAR, "crop_square_resize", img_index=idx)
    with torch.no_grad():
        out = net(crops, None)
    p2d, valid, _ = Q.correspondences(out, Bboxes=plain[4])
    for conf, check_seg in ((dict(chi2_threshold=9.21), False), (dict(chi2_threshold=5.99, floor=0.5, guided=False), True)):
        sigma2 = Q.code_confidence(out, plain[4], **({"floor": conf["floor"]} if "floor" in conf else {}))
        R0, t0, inl0, st0, info0 = Q.solve_pnp_conf(p3d, p2d, valid, sigma2, K, conf["chi2_threshold"], column=1 if check_seg else 0, seed=3,
                                                    guided=conf.get("guided", True))
        R, t, inl, status, final, info = Q.estimate_poses_conf(net, frames, boxes, p3d, K, conf, return_info=True, check_seg=check_seg, **kw)
        assert torch.equal(R, R0) and torch.equal(t, t0) and torch.equal(inl, inl0) and torch.equal(status, st0) and np.array_equal(final, plain[4])
        assert torch.equal(info["sigma2"], sigma2) and all(torch.equal(info[k], info0[k]) for k in info0) and "R0" not in info
        assert int(info["n_ranked"][2]) == 0 and int(status[2]) == 0                           # crop 2 has no box: variance 0, nothing ranked
        five = Q.estimate_poses_conf(net, frames, boxes, p3d, K, conf, check_seg=check_seg, **kw)
        assert len(five) == 5 and torch.equal(five[0], R0) and torch.equal(five[1], t0)
        for fit, mask in (("inliers", inl0), ("valid", valid[:, :, 1 if check_seg else 0].contiguous())):
            Rw, tw, stw, infow = Q.refine_poses_lm_weighted(p3d, p2d, mask, sigma2.rsqrt().float(), K, R0, t0, 2.5, status=st0, max_iters=12)
            got = Q.estimate_poses_conf(net, frames, boxes, p3d, K, conf, weighted=dict(huber_delta=2.5, fit=fit, max_iters=12), return_info=True,
                                        check_seg=check_seg, **kw)
            assert torch.equal(got[0], Rw) and torch.equal(got[1], tw) and torch.equal(got[2], inl0) and torch.equal(got[3], st0)
            assert torch.equal(got[5]["refine_status"], stw) and torch.equal(got[5]["R0"], R0) and torch.equal(got[5]["t0"], t0)
            assert torch.equal(got[5]["n_clipped"], infow["n_clipped"]) and torch.equal(got[5]["order"], info0["order"])
            print("conf=%r fit=%s: solver status %s, ranked %s, dropped %s, refine status %s" % (conf, fit, st0.tolist(), info0["n_ranked"].tolist(),
                                                                                               info0["n_dropped"].tolist(), stw.tolist()))
    again = Q.estimate_poses(net, frames, boxes, p3d, K, **kw)                                 # the shared forward helper changed nothing
    assert all(torch.equal(a, b) for a, b in zip(plain[:4], again[:4])) and np.array_equal(plain[4], again[4])


def test_refusals_on_the_device():
    from checkerpose_amd import postprocess as Q
    B, N = 2, 8
    a = dict(p3d_xyz=torch.zeros(N, 3, device=DEV), p2d=torch.zeros(B, N, 2, device=DEV), valid=torch.ones(B, N, 3, dtype=torch.uint8, device=DEV),
             sigma2=torch.ones(B, N, 2, dtype=torch.float64, device=DEV), cam_K=torch.eye(3, device=DEV), chi2_threshold=5.99)
    for name, bad in (("p3d_xyz", torch.zeros(N + 1, 3, device=DEV)), ("cam_K", torch.eye(4, device=DEV))):
        with pytest.raises(ValueError, match="p3d_xyz must be"):
            Q.solve_pnp_conf(**dict(a, **{name: bad}))
    for name, bad in (("chi2_threshold", 0.0), ("chi2_threshold", float("inf")), ("iterations", 257), ("column", 3)):
        with pytest.raises(ValueError, match=name):
            Q.solve_pnp_conf(**dict(a, **{name: bad}))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.solve_pnp_conf(**dict(a, sigma2=a["sigma2"].cpu()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.rank_correspondences(a["sigma2"], a["valid"].cpu())
    frames = torch.zeros(4, 4, 3, dtype=torch.uint8, device=DEV)
    for name, value in (("solver", "gc"), ("refine", "lm"), ("graph", None), ("depth", None), ("dist_threshold", 1.0), ("reproj_threshold", 2.0)):
        with pytest.raises(ValueError, match=name):
            Q.estimate_poses_conf(None, frames, [], a["p3d_xyz"], a["cam_K"], dict(chi2_threshold=5.99), **{name: value})
    with pytest.raises(ValueError, match="conf must be"):
        Q.estimate_poses_conf(None, frames, [], a["p3d_xyz"], a["cam_K"], dict(floor=0.5))
    R, t, inl, status, info = Q.solve_pnp_conf(**a)                                            # degenerate but well-formed: the identity fallback
    assert status.tolist() == [0, 0] and not inl.any() and info["n_ranked"].tolist() == [N, N]
