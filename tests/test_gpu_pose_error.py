"""Row N5 on the device: cp_pose_errors / metric.pose_errors against the reference's recorded ADD / ADI (tests/golden/pose_error.npz)
and against the host restatement of tests/test_pose_error.py.

Tolerance (derived, not tuned): |got - ref| <= 16 * 2^-24 * (r_max + |tr| + ref) with r_max the mesh's largest vertex norm and tr the
relative translation R_est^T (t_gt - t_est) -- a few fp32 roundings of coordinates of that size, which is all the kernel's model-frame
arithmetic can lose (about 1.3e-4 mm + 1e-6 x error for the LM objects, four orders below the smallest pass threshold)."""
import time

import numpy as np
import pytest
import torch

from checkerpose_amd import metric
from tests.common import golden
from tests.test_pose_error import host_add, host_adi, lm_table, mesh_of, tolerance

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, shape):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))).to(DEV)


def _batch(g, idx):
    n = len(idx)
    return _dev(g["R_est"][idx], (n, 3, 3)), _dev(g["t_est"][idx], (n, 3, 1)), _dev(g["R_gt"][idx], (n, 3, 3)), _dev(g["t_gt"][idx], (n, 3, 1))


def _check(g, c, pts, add, adi, what):
    for name, got, ref in (("add", add, g["add"][c]), ("adi", adi, g["adi"][c])):
        tol = tolerance(g["R_est"][c], g["t_est"][c], g["R_gt"][c], g["t_gt"][c], pts, ref)
        print("%s case %2d V=%5d %-5s %s got %.9g ref %.9g |diff| %.3e tol %.3e" % (what, c, len(pts), g["tag"][c], name, got, ref, abs(got - ref), tol))
        assert abs(got - ref) <= tol, (what, c, name, got, ref, tol)
        if str(g["tag"][c]) == "0":
            assert got == 0.0, (what, c, name, got)
    assert adi <= add, (what, c, add, adi)                       # same q_i, same distance expression, j = i among the candidates


def test_goldens_in_batches_and_one_by_one():
    g, table = golden("pose_error"), lm_table()
    single_mesh_groups = [k for k in sorted(set(g["group"].tolist())) if len(set(g["mesh"][g["group"] == k].tolist())) == 1]
    assert len(single_mesh_groups) >= 10
    for k in single_mesh_groups:
        idx = np.nonzero(g["group"] == k)[0]
        pts = mesh_of(g, table, g["mesh"][idx[0]])
        ms = metric.MeshSet.from_arrays([pts], diameters=[g["mesh_diameter"][g["mesh"][idx[0]]]])
        out = metric.pose_errors(*_batch(g, idx), ms)
        again = metric.pose_errors(*_batch(g, idx), ms)
        assert out["add"].dtype == torch.float64 and out["add"].is_cuda and tuple(out["adi"].shape) == (len(idx),)
        assert torch.equal(out["add"], again["add"]) and torch.equal(out["adi"], again["adi"])          # two calls: bit-identical
        add, adi = out["add"].cpu().numpy(), out["adi"].cpu().numpy()
        for j, c in enumerate(idx):
            _check(g, c, pts, add[j], adi[j], "batch")
            one = metric.pose_errors(*_batch(g, idx[j:j + 1]), ms)                                        # the reduction order does not depend on B
            assert float(one["add"][0]) == add[j] and float(one["adi"][0]) == adi[j], (c, "batch != single")
            only = metric.pose_errors(*_batch(g, idx[j:j + 1]), ms, kinds=("adi",))
            assert list(only) == ["adi"] and float(only["adi"][0]) == adi[j]
            a1 = metric.Calculate_ADD_Error_BOP(g["R_gt"][c], g["t_gt"][c], g["R_est"][c], g["t_est"][c], pts)         # the reference-named twins
            i1 = metric.Calculate_ADI_Error_BOP(g["R_gt"][c], g["t_gt"][c].reshape(3, 1), g["R_est"][c], g["t_est"][c].reshape(3, 1), pts)
            assert isinstance(a1, float) and isinstance(i1, float) and a1 == add[j] and i1 == adi[j]
            _check(g, c, pts, a1, i1, "twin")
        if len(pts) == 1:
            assert np.array_equal(add, adi)                                                                # one vertex: its own nearest neighbour


def test_mixed_meshes_equal_per_object_calls():
    g, table = golden("pose_error"), lm_table()
    k = max(g["group"].tolist())
    idx = np.nonzero(g["group"] == k)[0]
    mesh_list = sorted(set(g["mesh"][idx].tolist()))
    assert len(mesh_list) == 13
    arrays = [mesh_of(g, table, mi) for mi in mesh_list]
    ms = metric.MeshSet.from_arrays(arrays, diameters=g["mesh_diameter"][mesh_list])
    ids = np.array([mesh_list.index(mi) for mi in g["mesh"][idx]])
    out = metric.pose_errors(*_batch(g, idx), ms, mesh_ids=ids)
    out_dev_ids = metric.pose_errors(*_batch(g, idx), ms, mesh_ids=torch.from_numpy(ids).to(DEV))
    out_list = metric.pose_errors(*_batch(g, idx), arrays, mesh_ids=ids)
    for o in (out_dev_ids, out_list):
        assert torch.equal(o["add"], out["add"]) and torch.equal(o["adi"], out["adi"])
    add, adi = out["add"].cpu().numpy(), out["adi"].cpu().numpy()
    for j, c in enumerate(idx):
        _check(g, c, arrays[ids[j]], add[j], adi[j], "mixed")
        one = metric.pose_errors(*_batch(g, idx[j:j + 1]), arrays[ids[j]])
        assert float(one["add"][0]) == add[j] and float(one["adi"][0]) == adi[j], (c, "mixed != per object")
        a1 = metric.Calculate_ADD_Error_BOP(g["R_gt"][c], g["t_gt"][c], g["R_est"][c], g["t_est"][c], arrays[ids[j]])   # and the twins, one pose at a time
        i1 = metric.Calculate_ADI_Error_BOP(g["R_gt"][c], g["t_gt"][c], g["R_est"][c], g["t_est"][c], arrays[ids[j]])
        assert isinstance(a1, float) and isinstance(i1, float) and a1 == add[j] and i1 == adi[j], (c, "mixed != twins")
        _check(g, c, arrays[ids[j]], a1, i1, "twin")
    s = metric.summarize(out, ms.diameters, mesh_ids=ids)
    want = metric.summarize({"add": g["add"][idx], "adi": g["adi"][idx]}, ms.diameters, mesh_ids=ids)
    for key in ("passed_2", "passed_5", "passed_10", "supp_passed_2", "supp_passed_5", "supp_passed_10"):
        assert s[key] == want[key], key                                                                    # no golden error sits near a threshold
    assert abs(s["auc_posecnn"] - want["auc_posecnn"]) <= 1e-6
    bad = metric.pose_errors(*_batch(g, idx[:2]), ms, mesh_ids=torch.tensor([0, 13], device=DEV))         # an id outside the table: NaN, no fault
    assert torch.isfinite(bad["add"][0]) and torch.isnan(bad["add"][1]) and torch.isnan(bad["adi"][1])
    Re, te, Rg, tg = _batch(g, idx[:2])
    Re[1, 0, 0] = float("nan")                                                                              # a NaN pose: NaN in both errors, its neighbour untouched
    nanp = metric.pose_errors(Re, te, Rg, tg, ms, mesh_ids=ids[:2])
    assert torch.isnan(nanp["add"][1]) and torch.isnan(nanp["adi"][1])
    assert float(nanp["add"][0]) == add[0] and float(nanp["adi"][0]) == adi[0]


def test_poses_straight_from_the_solver():
    from checkerpose_amd.postprocess import solve_pnp_ransac
    from tests.test_pnp import K_LMO, make_case
    rng = np.random.default_rng(21)
    B, N = 6, 512
    cases = [make_case(rng) for _ in range(B)]
    xyz = cases[0][0]
    valid = np.zeros((B, N, 3), np.uint8)
    for b, c in enumerate(cases):
        valid[b, :, 0] = c[2]
    valid[5, :, 0] = 0                                                                                     # crop 5: the identity fallback
    R, t, inl, status = solve_pnp_ransac(torch.from_numpy(xyz).float().to(DEV), torch.from_numpy(np.stack([c[1] for c in cases])).float().to(DEV),
                                         torch.from_numpy(valid).to(DEV), torch.from_numpy(K_LMO).float().to(DEV), seed=4)
    assert R.is_cuda and R.dtype == torch.float64 and tuple(t.shape) == (B, 3, 1)
    R_gt, t_gt = np.stack([c[4] for c in cases]), np.stack([c[5] for c in cases])
    pts = xyz.astype(np.float32)
    out = metric.pose_errors(R, t, R_gt, t_gt, pts)                                                        # device poses in, host ground truth uploaded
    add, adi = out["add"].cpu().numpy(), out["adi"].cpu().numpy()
    Rh, th, st = R.cpu().numpy(), t.cpu().numpy(), status.cpu().numpy()
    assert st.tolist() == [1, 1, 1, 1, 1, 0]
    r_max = float(np.linalg.norm(pts.astype(np.float64), axis=1).max())
    for b in range(B):
        ra, ri = host_add(Rh[b], th[b], R_gt[b], t_gt[b], pts), host_adi(Rh[b], th[b], R_gt[b], t_gt[b], pts)
        ta, ti = tolerance(Rh[b], th[b], R_gt[b], t_gt[b], pts, ra), tolerance(Rh[b], th[b], R_gt[b], t_gt[b], pts, ri)
        print("solver crop %d status %d add %.6f (host %.6f) adi %.6f (host %.6f) tol %.2e" % (b, st[b], add[b], ra, adi[b], ri, ta))
        assert abs(add[b] - ra) <= ta and abs(adi[b] - ri) <= ti and adi[b] <= add[b]
        if st[b] == 1:                 # test_pnp.py pins max |dR| < 5e-3 and |dt| < 5e-3 |t| for the device solver: ADD <= |dt| + 3 max|dR| r_max
            assert add[b] < 5e-3 * np.linalg.norm(t_gt[b]) + 3 * 5e-3 * r_max, (b, add[b])
    assert np.array_equal(Rh[5], np.eye(3)) and not th[5].any() and add[5] > 400.0


def test_evaluate_poses_end_to_end():
    from checkerpose_amd import postprocess as Q
    from tests.common import build_net
    rng = np.random.default_rng(9)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 480, 640, 3), dtype=np.uint8)).to(DEV)
    boxes = [[100, 80, 120, 90], [300, 200, 60, 140], None, [-10, 400, 90, 90]]
    net = build_net(npoint=512, seed=1).to(DEV).eval()
    net.set_compute_dtype("bf16")
    pts = lm_table()[:4096]
    p3d = torch.from_numpy(pts[:512]).to(DEV)
    K = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]], dtype=np.float32)
    R_gt = np.stack([np.eye(3)] * 4)
    t_gt = np.array([[10.0, -20.0, 800.0 + 100 * b] for b in range(4)])
    err, R, t, inl, status, final = Q.evaluate_poses(net, frames, boxes, p3d, K, R_gt, t_gt, pts, img_index=[0, 1, 0, 1])
    assert sorted(err) == ["add", "adi"]
    add, adi = err["add"].cpu().numpy(), err["adi"].cpu().numpy()
    assert err["add"].is_cuda and err["add"].dtype == torch.float64 and add.shape == (4,) and adi.shape == (4,)
    assert np.isfinite(add).all() and np.isfinite(adi).all() and (adi <= add).all()
    assert tuple(R.shape) == (4, 3, 3) and tuple(t.shape) == (4, 3, 1) and status.dtype == torch.int32 and final.shape == (4, 4)
    Rh, th, st = R.cpu().numpy(), t.cpu().numpy(), status.cpu().numpy()
    print("evaluate_poses status", st.tolist())

    def against_host(add, adi, st, Rh, th):
        for b in range(4):
            Rb, tb = (np.eye(3), np.zeros(3)) if st[b] == 0 else (Rh[b], th[b])                            # status 0: scored as R = I, t = 0
            ra, ri = host_add(Rb, tb, R_gt[b], t_gt[b], pts), host_adi(Rb, tb, R_gt[b], t_gt[b], pts)
            assert abs(add[b] - ra) <= tolerance(Rb, tb, R_gt[b], t_gt[b], pts, ra), (b, add[b], ra)
            assert abs(adi[b] - ri) <= tolerance(Rb, tb, R_gt[b], t_gt[b], pts, ri), (b, adi[b], ri)
    against_host(add, adi, st, Rh, th)
    # the identity fallback (test_network_with_test_data.py:111-114), made certain: a border filter as wide as half the 64 x 64 map
    # leaves no valid correspondence in any crop (the random-init network alone solves all four crops above)
    err0, R0, t0, _, status0, _ = Q.evaluate_poses(net, frames, boxes, p3d, K, R_gt, t_gt, pts, img_index=[0, 1, 0, 1], discard_bd_pixel=32)
    st0 = status0.cpu().numpy()
    assert (st0 == 0).all() and torch.equal(R0.cpu(), torch.eye(3, dtype=torch.float64).expand(4, 3, 3)) and not t0.any()
    add0, adi0 = err0["add"].cpu().numpy(), err0["adi"].cpu().numpy()
    against_host(add0, adi0, st0, R0.cpu().numpy(), t0.cpu().numpy())
    assert (add0 > 700.0).all()                                                                            # scored against depths of 800 mm and more


def test_adi_batch_is_not_slower_than_the_host_path():
    """the one timing inequality: ADI of 256 poses over 4 096 vertices on the device <= the host path (numpy + cKDTree, one pose at a
    time) over the same batch"""
    pts = lm_table()[:4096]
    rng = np.random.default_rng(5)
    B = 256
    R_gt = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(B)])
    R_gt *= np.sign(np.linalg.det(R_gt))[:, None, None]
    t_gt = np.stack([rng.uniform(-100, 100, B), rng.uniform(-100, 100, B), rng.uniform(400, 1500, B)], 1)
    R_est, t_est = np.roll(R_gt, 1, 0) * 1.0, t_gt + rng.normal(scale=5.0, size=(B, 3))
    ms = metric.MeshSet.from_arrays([pts], diameters=[1.0])
    args = (_dev(R_est, (B, 3, 3)), _dev(t_est, (B, 3, 1)), _dev(R_gt, (B, 3, 3)), _dev(t_gt, (B, 3, 1)), ms)
    for _ in range(2):
        out = metric.pose_errors(*args, kinds=("adi",))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        out = metric.pose_errors(*args, kinds=("adi",))
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / 5
    t0 = time.perf_counter()
    host = [host_adi(R_est[b], t_est[b], R_gt[b], t_gt[b], pts) for b in range(B)]
    host_ms = (time.perf_counter() - t0) * 1e3
    got = out["adi"].cpu().numpy()
    print("ADI B=256 V=4096: device %.3f ms, host %.1f ms, ratio %.0f" % (dev_ms, host_ms, host_ms / dev_ms))
    for b in range(0, B, 17):
        assert abs(got[b] - host[b]) <= tolerance(R_est[b], t_est[b], R_gt[b], t_gt[b], pts, host[b])
    assert dev_ms <= host_ms, (dev_ms, host_ms)
