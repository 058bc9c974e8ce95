"""GPU: row N32 on the device.  code_confidence against its restatement at the lane-count edges, every special logit and box;
refine_poses_lm_weighted replayed one iteration at a time from its own records (tests/wlm_stages.py) over every committed case; the
bitwise pass-throughs and identities of the call; its exact scaling property; row N22 as its special case; the refusals;
estimate_poses_weighted as the composition of its parts."""
import numpy as np
import pytest
import torch

from tests import pnp_stages as S
from tests import wlm_stages as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INF = float("inf")
_CACHE = {}


def _case(name):
    if name not in _CACHE:
        _CACHE[name] = W.make(name)
    return _CACHE[name]


def _args(case, rows=None, scale=None, delta=None, records=True):
    rows = slice(None) if rows is None else rows
    return dict(p3d_xyz=torch.from_numpy(case.p3d[rows] if case.p3d.ndim == 3 else case.p3d).float().to(DEV),
                p2d=torch.from_numpy(case.p2d[rows]).float().to(DEV), mask=torch.from_numpy(case.mask[rows]).to(DEV).bool(),
                scale=torch.from_numpy(case.scale[rows] if scale is None else scale[rows]).to(DEV),
                cam_K=torch.from_numpy(case.K[rows] if case.K.ndim == 3 else case.K).float().to(DEV),
                R=torch.from_numpy(case.R0[rows]).to(DEV), t=torch.from_numpy(case.t0[rows]).to(DEV), huber_delta=case.delta if delta is None else delta,
                status=None if case.status_in is None else torch.from_numpy(case.status_in[rows]).to(DEV),
                max_iters=case.max_iters, step_tol=case.step_tol, return_records=records)


def _flat(info):
    return torch.cat([info["cost0"][:, None], info["cost"][:, None], info["n"][:, None].double(), info["iters"][:, None].double(),
                      info["H"].reshape(-1, 36), info["n_clipped0"][:, None].double(), info["n_clipped"][:, None].double()], 1)


def _device_run(case, **kw):
    """-> [records, R, t, status, info (B,42) with the two counts as the wrapper returns them (0 on pass-through rows)]"""
    from checkerpose_amd.postprocess import refine_poses_lm_weighted
    out = refine_poses_lm_weighted(**_args(case, **kw))
    torch.cuda.synchronize()
    R, t, status, info = out[:4]
    assert tuple(R.shape) == (len(status), 3, 3) and tuple(t.shape) == (len(status), 3, 1) and status.dtype == torch.int32
    assert info["status"] is status and R.dtype == t.dtype == torch.float64 and info["n_clipped"].dtype == torch.int64
    rec = out[4].cpu().numpy() if len(out) == 5 else None
    return [rec, R.cpu().numpy(), t.cpu().numpy()[:, :, 0], status.cpu().numpy(), _flat(info).cpu().numpy()]


def _raw_info(flat, status):
    """the wrapper's info back in the entry point's layout: NaN counts on pass-through rows"""
    flat = flat.copy()
    flat[status == 0, 40:] = np.nan
    return flat


def _bitwise(a, b, rows=None):
    return all(np.array_equal(x[rows] if rows is not None else x, y, equal_nan=True) for x, y in zip(a, b) if x is not None and y is not None)


# ------------------------------------------------------------------------------------------------------------- code_confidence
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_code_confidence_against_the_restatement(B, N):
    from checkerpose_amd import _abi
    from checkerpose_amd.postprocess import code_confidence
    worst = 0.0
    for r in (1, 6):
        rows = 1 + 2 * r + 2                                                     # more rows than the codes need
        seed = N + 2 * r + B
        for shift in range(0, 6, B):                                             # every box at every (B, N, r): tests/test_wlm.py checks the operands
            bits, bbox = W.conf_inputs(B, N, r, rows, seed, shift)
            for floor in (1.0 / 12.0, 0.5):
                want = W.code_confidence(bits, bbox, 64, 48, r, floor)
                got = torch.full((B, N, 2), -7.0, dtype=torch.float64, device=DEV)
                _abi.call("cp_code_confidence", DEV, torch.from_numpy(bits).to(DEV), rows, r, torch.from_numpy(bbox).to(DEV), B, N, 64, 48, floor, got)
                got = got.cpu().numpy()
                assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0.0, want == 0.0)
                ok = np.isfinite(want) & (want != 0.0)
                assert np.isfinite(got[ok]).all() and (got[ok] > 0).all()
                dev = np.abs(got[ok] - want[ok]) / want[ok]
                worst = max(worst, float(dev.max()) if dev.size else 0.0)
                assert (dev <= W.CONF_RTOL).all(), (r, shift, floor, float(dev.max()))
        if r == 6:                                                               # the wrapper: the forward's 13-row block and its default floor
            block = torch.from_numpy(bits[:, :13].copy()).to(DEV)
            outputs = (block[:, :1], block[:, 1:7], block[:, 7:], torch.zeros(B, 2, 64, 48, device=DEV), None, None)
            s2 = code_confidence(outputs, bbox)
            want = W.code_confidence(bits[:, :13], bbox, 64, 48, 6)
            ok = np.isfinite(want) & (want != 0.0)
            got = s2.cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want)) and (np.abs(got[ok] - want[ok]) <= W.CONF_RTOL * want[ok]).all()
            cat = code_confidence(tuple(x.clone() if torch.is_tensor(x) else x for x in outputs), torch.from_numpy(bbox).to(DEV))      # no shared base
            assert torch.equal(torch.nan_to_num(cat, nan=-1.0), torch.nan_to_num(s2, nan=-1.0))
    print("code_confidence B %d N %d: largest relative deviation %.3e (bound %.3e = 64 ulp)" % (B, N, worst, W.CONF_RTOL))


# ------------------------------------------------------------------------------------------------------------- refine_poses_lm_weighted
@pytest.mark.parametrize("name", list(W.CASES))
def test_device_stages(name):
    case = _case(name)
    rec, R, t, status, info = _device_run(case)
    assert rec.shape == (case.B, case.max_iters, W.REC)
    total = W.check_case(case, rec, R, t, status, _raw_info(info, status), log=print)
    print("%-18s device against numpy, worst trial: |dR| %.3e (tau %.3e)  |dt|/|t| %.3e (tau %.3e)"
          % (name, total["dR_1e18"] * 1e-18, W.taus()[0], total["dt_1e18"] * 1e-18, W.taus()[1]))
    refined = status != 0
    assert (info[refined, 1] <= info[refined, 0]).all()
    assert (np.abs(np.einsum("bji,bjk->bik", R[refined], R[refined]) - np.eye(3)) <= 1e-12).all()
    if name == "passthrough":
        assert [int(s != 0) for s in status] == W.PASS_EXPECT
    elif name.startswith(("unit", "hetero")):
        assert (status == 1).all() and (info[:, 40:] == 0).all()


def test_pass_throughs_are_bitwise():
    case = _case("passthrough")
    rec, R, t, status, info = _device_run(case)
    for b in np.nonzero(status == 0)[0]:
        assert np.array_equal(R[b].view(np.uint64), case.R0[b].view(np.uint64)), b                  # NaN payloads included
        assert np.array_equal(t[b].view(np.uint64), case.t0[b].view(np.uint64)), b
        assert np.isnan(rec[b]).all() and np.isnan(info[b, :2]).all() and np.isnan(info[b, 4:40]).all() and (info[b, 40:] == 0).all()
    assert int((status == 0).sum()) == W.PASS_EXPECT.count(0)


@pytest.mark.parametrize("name", ["unit_3x256", "hetero_3x7", "hetero_3x512"])
def test_doubled_scales_quadruple_the_costs_and_nothing_else(name):
    case = _case(name)
    a = _device_run(case)
    b = _device_run(case, scale=case.scale * np.float32(2.0))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert np.array_equal(a[0][:, :, [0, 3, 4]], b[0][:, :, [0, 3, 4]], equal_nan=True) and np.array_equal(a[0][:, :, 5:], b[0][:, :, 5:], equal_nan=True)
    assert np.array_equal(4.0 * a[0][:, :, 1:3], b[0][:, :, 1:3], equal_nan=True)
    assert np.array_equal(4.0 * a[4][:, :2], b[4][:, :2]) and np.array_equal(4.0 * a[4][:, 4:40], b[4][:, 4:40]) and np.array_equal(a[4][:, 2:4], b[4][:, 2:4])


@pytest.mark.parametrize("name", [k for k in W.CASES if k.startswith("unit")])
def test_unit_scales_and_no_kernel_against_row_n22(name):
    from checkerpose_amd.postprocess import refine_poses_lm
    case = _case(name)
    rec, R, t, status, info = _device_run(case)
    g = _args(case)
    R2, t2, st2, info2, rec2 = refine_poses_lm(g["p3d_xyz"], g["p2d"], g["mask"], g["cam_K"], g["R"], g["t"], status=g["status"], max_iters=case.max_iters,
                                               step_tol=case.step_tol, return_records=True)
    R2, t2, rec2 = R2.cpu().numpy(), t2.cpu().numpy()[:, :, 0], rec2.cpu().numpy()
    assert np.array_equal(status, st2.cpu().numpy()) and np.array_equal(rec[:, :, 3], rec2[:, :, 3], equal_nan=True)
    dR, dt = float(np.abs(R - R2).max()), float((np.linalg.norm(t - t2, axis=1) / np.linalg.norm(t2, axis=1)).max())
    same = np.array_equal(rec, rec2, equal_nan=True) and np.array_equal(R, R2) and np.array_equal(t, t2) and np.array_equal(info[:, :40], _flat_n22(info2))
    print("%-12s against refine_poses_lm: |dR| %.3e  |dt|/|t| %.3e  bits equal: %s" % (name, dR, dt, same))
    assert dR <= W.taus()[0] and dt <= W.taus()[1]


def _flat_n22(info):
    return torch.cat([info["cost0"][:, None], info["cost"][:, None], info["n"][:, None].double(), info["iters"][:, None].double(),
                      info["H"].reshape(-1, 36)], 1).cpu().numpy()


def test_alone_in_threes_and_all_together():
    case = _case("passthrough")                                                  # 13 crops, refined and passed through, one shared model
    whole = _device_run(case)
    for lo in range(0, case.B, 3):
        rows = slice(lo, min(lo + 3, case.B))
        assert _bitwise(whole, _device_run(case, rows=rows), rows), lo
    for b in (0, 6, 7, 11):
        assert _bitwise(whole, _device_run(case, rows=slice(b, b + 1)), slice(b, b + 1)), b
    per = _case("outlier_3x256")                                                 # per-crop models and intrinsics
    assert per.p3d.ndim == 3 and per.K.ndim == 3
    whole = _device_run(per)
    assert _bitwise(whole, _device_run(per, rows=slice(1, 2)), slice(1, 2)) and _bitwise(whole, _device_run(per, rows=slice(0, 2)), slice(0, 2))
    assert _bitwise(whole, _device_run(per))                                     # two calls


@pytest.mark.parametrize("name", ["outlier_3x512", "passthrough"])
def test_with_and_without_records(name):
    case = _case(name)
    a, b = _device_run(case), _device_run(case, records=False)
    assert b[0] is None and _bitwise(a[1:], b[1:])


def test_refusals_on_the_device():
    from checkerpose_amd.postprocess import code_confidence, refine_poses_lm_weighted
    a = dict(_args(_case("hetero_3x7")), return_records=False)
    for name, bad in (("max_iters", 0), ("max_iters", 65), ("step_tol", 0.0), ("step_tol", float("nan")), ("huber_delta", 0.0), ("huber_delta", -2.0),
                      ("huber_delta", float("nan")), ("mask", a["mask"][:, :6]), ("R", a["R"][:2]), ("status", torch.ones(2, dtype=torch.int32, device=DEV)),
                      ("scale", a["scale"][:, :, :1]), ("scale", a["scale"].double()), ("scale", a["scale"][:2])):
        with pytest.raises(ValueError, match=name):
            refine_poses_lm_weighted(**dict(a, **{name: bad}))
    with pytest.raises(ValueError, match="p3d_xyz"):
        refine_poses_lm_weighted(**dict(a, p3d_xyz=torch.zeros(8, 3, device=DEV)))
    for name in ("mask", "scale", "R"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            refine_poses_lm_weighted(**dict(a, **{name: a[name].cpu()}))
    block = torch.zeros(2, 13, 8, device=DEV)
    outputs = (block[:, :1], block[:, 1:7], block[:, 7:], torch.zeros(2, 2, 64, 64, device=DEV), None, None)
    for floor in (0.0, -1.0, float("nan"), INF):
        with pytest.raises(ValueError, match="floor"):
            code_confidence(outputs, np.zeros((2, 4), np.int32), floor=floor)
    with pytest.raises(ValueError, match="Bboxes"):
        code_confidence(outputs, np.zeros((3, 4), np.int32))
    with pytest.raises(ValueError, match="13-row"):
        code_confidence((block[:, :1].clone(), block[:, 1:4].clone(), block[:, 7:].clone(), outputs[3], None, None), np.zeros((2, 4), np.int32))


# ------------------------------------------------------------------------------------------------------------ the caller
def test_estimate_poses_weighted_is_the_composition_of_its_parts(monkeypatch):
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
    plain = Q.estimate_poses(net, frames, boxes, p3d, K, **kw)
    padded = [None if b is None else PP.padding_Bbox(b, 1.5) for b in boxes]
    crops = PP.get_roi_batch(frames, padded, 256, PP.INTER_LINEAR, "crop_square_resize", img_index=idx)
    with torch.no_grad():
        out = net(crops, None)
    p2d, valid, _ = Q.correspondences(out, Bboxes=plain[4])
    sigma2 = Q.code_confidence(out, plain[4])
    scale = sigma2.rsqrt().float()
    assert tuple(sigma2.shape) == (4, 512, 2) and (sigma2[2] == 0).all() and bool((sigma2[[0, 1, 3]] > 0).all())      # crop 2 has no box
    for fit, mask in (("inliers", plain[2]), ("valid", valid[:, :, 0].contiguous())):
        R, t, inl, status, final, info = Q.estimate_poses_weighted(net, frames, boxes, p3d, K, dict(huber_delta=2.5, fit=fit), return_info=True, **kw)
        assert torch.equal(inl, plain[2]) and torch.equal(status, plain[3]) and np.array_equal(final, plain[4])
        assert torch.equal(info["R0"], plain[0]) and torch.equal(info["t0"], plain[1]) and torch.equal(info["sigma2"], sigma2)
        R2, t2, st2, info2 = Q.refine_poses_lm_weighted(p3d, p2d, mask, scale, K, plain[0], plain[1], 2.5, status=plain[3])
        assert torch.equal(R, R2) and torch.equal(t, t2) and torch.equal(info["status"], st2) and tuple(R.shape) == (4, 3, 3) and tuple(t.shape) == (4, 3, 1)
        assert torch.equal(info["n_clipped"], info2["n_clipped"]) and torch.equal(info["cost"].nan_to_num(-1.0), info2["cost"].nan_to_num(-1.0))
        passed = st2 == 0
        assert bool(passed[2]) and bool((st2[plain[3] == 0] == 0).all())
        assert torch.equal(R[passed], plain[0][passed]) and torch.equal(t[passed], plain[1][passed])            # the solver's pose, bitwise
        five = Q.estimate_poses_weighted(net, frames, boxes, p3d, K, dict(huber_delta=2.5, fit=fit), **kw)
        assert len(five) == 5 and torch.equal(five[0], R) and torch.equal(five[1], t)
        print("fit=%s: solver status %s, refine status %s, clipped %s" % (fit, plain[3].tolist(), st2.tolist(), info2["n_clipped"].tolist()))
    # fit="inliers", scales forced to 1, delta = +inf: row N22's refinement
    lm = Q.estimate_poses(net, frames, boxes, p3d, K, refine="lm", **kw)
    monkeypatch.setattr(Q, "code_confidence", lambda outputs, final, **k: torch.ones(4, 512, 2, dtype=torch.float64, device=DEV))
    R, t, inl, status, final = Q.estimate_poses_weighted(net, frames, boxes, p3d, K, dict(huber_delta=INF, fit="inliers"), **kw)
    ok = (status != 0).cpu().numpy()
    dR = float((R - lm[0]).abs().max())
    dt = float((torch.linalg.norm((t - lm[1]).reshape(4, 3), dim=1)[ok] / torch.linalg.norm(lm[1].reshape(4, 3), dim=1)[ok]).max()) if ok.any() else 0.0
    print("unit scales, delta = +inf against estimate_poses(refine='lm'): |dR| %.3e  |dt|/|t| %.3e  bits equal: %s" % (dR, dt, torch.equal(R, lm[0]) and torch.equal(t, lm[1])))
    assert dR <= W.taus()[0] and dt <= W.taus()[1] and torch.equal(R[~torch.from_numpy(ok).to(DEV)], lm[0][~torch.from_numpy(ok).to(DEV)])
