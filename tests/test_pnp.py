"""Row N4 (pose from correspondences).  cv2 is not part of the reference's tree, so parity with it is UNPINNED (oracle/pnp_oracle.py
says why); what IS checked: the oracle recovers known poses (exact data to 1e-9, 30 % outliers + pixel noise to the noise level, and
finds exactly the true inlier set), reproduces the reference's identity fallbacks (test_network_with_test_data.py:111-114), and the
device kernel (cp_pnp_ransac) follows the oracle on the same inputs and samples (shared counter-based hash): identical on noise-free
data and on the fallbacks, inlier sets within 2 % and poses within 2e-3 under noise (the eigen-solvers pick different bases of
EPnP's degenerate null space; both stay within 5e-3 of the true pose)."""
import os

import numpy as np
import pytest
import torch

from oracle import pnp_oracle as P
from checkerpose_amd.synthetic import DATA

K_LMO = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1.0]])      # LM-O camera


def _model(n=512):
    return np.load(os.path.join(DATA, "fps_lmo_obj01.npy"))[:n].astype(np.float32).astype(np.float64)      # mm, as the kernel reads them


def _pose(rng):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = rng.uniform(0.1, np.pi - 0.1)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    return R, np.array([rng.uniform(-120, 120), rng.uniform(-90, 90), rng.uniform(500, 1300)])


def make_case(rng, n=512, outlier_frac=0.3, noise=0.5, valid_frac=0.8):
    xyz = _model(n)
    R, t = _pose(rng)
    uv = P.project(xyz, K_LMO, R, t)
    out = rng.random(n) < outlier_frac
    uvn = uv + rng.normal(scale=noise, size=uv.shape)
    uvn[out] += rng.uniform(20, 80, size=(int(out.sum()), 2)) * rng.choice([-1, 1], size=(int(out.sum()), 2))
    valid = rng.random(n) < valid_frac
    return xyz, uvn.astype(np.float32).astype(np.float64), valid, out, R, t


def test_hash_and_sampling_are_deterministic():
    assert P._hash32(1, 2, 3, 4) == P._hash32(1, 2, 3, 4) != P._hash32(1, 2, 3, 5)
    assert [P._hash32(7, b, 11, 0) for b in range(3)] == [714418499, 1957091910, 2981744819]      # known answers shared with pnp.hip
    s = P.sample_indices(3, 1, 17, 40, 5)
    assert len(set(s)) == 5 and all(0 <= v < 40 for v in s) and s == P.sample_indices(3, 1, 17, 40, 5)


def test_epnp_recovers_exact_poses():
    rng = np.random.default_rng(0)
    xyz = _model(64)
    for n in (4, 5, 6, 64):
        for _ in range(4):
            R, t = _pose(rng)
            uv = P.project(xyz[:n], K_LMO, R, t)
            Re, te, err = P.epnp(xyz[:n], uv, K_LMO)
            if n >= 5:
                assert err < 1e-8 and np.abs(Re - R).max() < 1e-8 and np.abs(te - t).max() < 1e-6, (n, err)
            else:        # 4 points leave a 4-dimensional null space: EPnP's linearisation + 5 Gauss-Newton steps need not reach the
                assert np.isfinite(err) and np.isfinite(Re).all()      # pose (4 valid points go to P3P instead: solve_four_points)
            assert abs(np.linalg.det(Re) - 1) < 1e-12


def test_ransac_finds_the_true_inlier_set_and_the_pose():
    rng = np.random.default_rng(1)
    for crop in range(3):
        xyz, uv, valid, out, R, t = make_case(rng)
        Re, te, mask, status = P.solve_pnp_ransac(xyz, uv, valid, K_LMO, 2.0, 150, seed=5, crop=crop)
        assert status == 1
        assert not (mask & ~valid).any() and not (mask & out).any()                 # no invalid and no outlier among the inliers
        assert mask.sum() >= 0.97 * (valid & ~out).sum()                            # 0.5 px noise: a few true inliers fall beyond 2 px
        assert np.abs(Re - R).max() < 5e-3 and np.linalg.norm(te - t) < 5e-3 * np.linalg.norm(t)


def test_reference_fallbacks():
    xyz = _model(16)
    rng = np.random.default_rng(2)
    R, t = _pose(rng)
    uv = P.project(xyz, K_LMO, R, t)
    for nvalid in (0, 3):                                   # num_valid < 4 -> R = I, t = 0, inliers None (:111-114)
        valid = np.zeros(16, bool)
        valid[:nvalid] = True
        Re, te, mask, status = P.solve_pnp_ransac(xyz, uv, valid, K_LMO)
        assert status == 0 and np.array_equal(Re, np.eye(3)) and not te.any() and not mask.any()
    valid = np.zeros(16, bool)
    valid[[1, 4, 9, 12]] = True                             # exactly 4: no RANSAC, P3P + the 4th point (as cv2 does); all 4 are inliers
    Re, te, mask, status = P.solve_pnp_ransac(xyz, uv, valid, K_LMO)
    assert status == 1 and np.array_equal(mask, valid)
    assert np.abs(Re - R).max() < 1e-8 and np.abs(te - t).max() < 1e-6


def test_four_points_p3p_known_answers():
    """exactly 4 correspondences (test_network_with_test_data.py:100: `num_valid >= 4` reaches cv2.solvePnPRansac, which then runs its
    P3P kernel): the true pose is recovered from exact data for random poses and random 4-subsets of the model; every P3P solution
    reproduces the three points it was solved from"""
    rng = np.random.default_rng(11)
    xyz = _model(512)
    for trial in range(60):
        R, t = _pose(rng)
        sel = rng.choice(512, 4, replace=False)
        uv = P.project(xyz[sel], K_LMO, R, t)
        f, dists = P.p3p_distances(xyz[sel[:3]], uv[:3], K_LMO)
        assert 1 <= len(dists) <= 4
        for sd in dists:
            Rk, tk = P._absolute_orientation(sd[:, None] * f, xyz[sel[:3]])
            assert np.abs(P.project(xyz[sel[:3]], K_LMO, Rk, tk) - uv[:3]).max() < 1e-6          # a valid pose of the 3 points
        rt = P.solve_four_points(xyz[sel], uv, K_LMO)
        assert rt is not None
        assert np.abs(rt[0] - R).max() < 1e-7 and np.abs(rt[1] - t).max() < 1e-5, trial


@pytest.mark.gpu
def test_device_four_points_p3p():
    """cp_pnp_ransac with exactly 4 valid correspondences per crop: P3P on the device == the oracle == the true pose; the 4 valid
    keypoints are the inliers; 4 collinear points (no solution) -> the identity fallback."""
    from checkerpose_amd.postprocess import solve_pnp_ransac
    rng = np.random.default_rng(12)
    B, N = 8, 512
    xyz = _model(N)
    p2d = np.zeros((B, N, 2))
    valid = np.zeros((B, N, 3), np.uint8)
    poses = []
    for b in range(B):
        R, t = _pose(rng)
        poses.append((R, t))
        p2d[b] = P.project(xyz, K_LMO, R, t)
        valid[b, rng.choice(N, 4, replace=False), 0] = 1
    dev = torch.device("cuda:0")
    Kf = K_LMO.astype(np.float32).astype(np.float64)
    p2f = p2d.astype(np.float32)
    Rd, td, inl, status = solve_pnp_ransac(torch.from_numpy(xyz).float().to(dev), torch.from_numpy(p2f).to(dev), torch.from_numpy(valid).to(dev),
                                           torch.from_numpy(K_LMO).float().to(dev), column=0, reproj_threshold=2.0, iterations=150, seed=1)
    torch.cuda.synchronize()
    Rd, td, inl, status = Rd.cpu().numpy(), td.cpu().numpy()[:, :, 0], inl.cpu().numpy(), status.cpu().numpy()
    for b in range(B):
        Ro, to, mo, so = P.solve_pnp_ransac(xyz, p2f[b].astype(np.float64), valid[b, :, 0].astype(bool), Kf, 2.0, 150, seed=1, crop=b)
        assert status[b] == so == 1, b
        assert np.array_equal(inl[b].astype(bool), mo) and int(mo.sum()) == 4
        assert np.abs(Rd[b] - Ro).max() < 1e-6 and np.abs(td[b] - to).max() < 1e-5 * max(1.0, np.linalg.norm(to)), b
        assert np.abs(Rd[b] - poses[b][0]).max() < 2e-3 and np.linalg.norm(td[b] - poses[b][1]) < 5e-3 * np.linalg.norm(poses[b][1])   # fp32 pixels


@pytest.mark.gpu
def test_device_pnp_equals_oracle():
    from checkerpose_amd.postprocess import solve_pnp_ransac
    rng = np.random.default_rng(3)
    B, N = 6, 512
    cases = [make_case(rng) for _ in range(B)]
    cases[4] = make_case(rng, outlier_frac=0.0, noise=0.0, valid_frac=1.0)              # exact data
    p2d = np.stack([c[1] for c in cases])
    valid = np.zeros((B, N, 3), np.uint8)
    for b, c in enumerate(cases):
        valid[b, :, 0] = 1                                                              # column 0 (all): every keypoint
        valid[b, :, 1] = c[2]                                                           # column 1: the case's validity mask
    valid[5, :, 1] = 0
    valid[5, [3, 70, 200], 1] = 1                                                       # crop 5: 3 valid -> identity fallback
    dev = torch.device("cuda:0")
    xyz = cases[0][0]
    R, t, inl, status, rec = solve_pnp_ransac(torch.from_numpy(xyz).float().to(dev), torch.from_numpy(p2d).float().to(dev),
                                              torch.from_numpy(valid).to(dev), torch.from_numpy(K_LMO).float().to(dev), column=1,
                                         reproj_threshold=2.0, iterations=150, seed=9, return_hypotheses=True)
    torch.cuda.synchronize()
    R, t, inl, status, rec = R.cpu().numpy(), t.cpu().numpy()[:, :, 0], inl.cpu().numpy(), status.cpu().numpy(), rec.cpu().numpy()
    Kf = K_LMO.astype(np.float32).astype(np.float64)
    # Everything but a noisy 5-point hypothesis' pose is exact given the device's own records: which records exist, every count,
    # the winner, the mask and the refit over the device's inlier list (tests/pnp_stages.py), on all six crops.
    from tests import pnp_stages as S
    und = pairs = 0
    for b in range(B):
        st = S.check_crop(xyz, p2d[b], valid[b, :, 1], Kf, 2.0, 150, 9, b, rec[b], R[b], t[b], inl[b], int(status[b]))
        und, pairs = und + st["undecided"], pairs + st["pairs"]
    assert und <= S.UNDECIDED_CAP * pairs, (und, pairs)
    for b, c in enumerate(cases):
        Ro, to, mo, so = P.solve_pnp_ransac(xyz, p2d[b], valid[b, :, 1].astype(bool), Kf, 2.0, 150, seed=9, crop=b)
        assert status[b] == so, b
        # A 5-point sample leaves M^T M with a two-dimensional exact null space: its basis is arbitrary (Jacobi here, LAPACK in the
        # oracle), EPnP's beta approximations are not invariant under that choice and Gauss-Newton stops after 5 steps, so a
        # hypothesis' pose -- hence its inlier count, hence the winner among near-ties -- may differ in the last correspondences.
        # Noise-free data (crop 4) and the fallback (crop 5) are exact; elsewhere the sets agree up to 2 % and the poses to 2e-3:
        # the statement about hypothesis-level ambiguity (what is exact is checked stage by stage above).
        if b >= 4:
            assert np.array_equal(inl[b], mo), (b, int(inl[b].sum()), int(mo.sum()))
            assert np.abs(R[b] - Ro).max() < 1e-6 and np.abs(t[b] - to).max() < 1e-5 * max(1.0, np.linalg.norm(to)), b
        else:
            assert int((inl[b] != mo).sum()) <= 0.02 * mo.sum(), (b, int(inl[b].sum()), int(mo.sum()))
            assert np.abs(R[b] - Ro).max() < 2e-3 and np.linalg.norm(t[b] - to) < 2e-3 * np.linalg.norm(to), b
        if b < 5:
            assert np.abs(R[b] - c[4]).max() < 5e-3 and np.linalg.norm(t[b] - c[5]) < 5e-3 * np.linalg.norm(c[5])
    assert status[5] == 0 and np.array_equal(R[5], np.eye(3)) and not t[5].any() and not inl[5].any()
    assert np.abs(R[4] - cases[4][4]).max() < 1e-5                                      # exact data (fp32 inputs): the true pose


@pytest.mark.gpu
def test_device_pnp_consumes_the_forward(lib):
    """forward -> cp_correspondences -> cp_pnp_ransac without leaving the device (random-init weights: the pose is meaningless, the
    plumbing is what is checked: shapes, dtypes, status in {0, 1}, inliers a subset of the valid column, proper rotations)"""
    from checkerpose_amd.postprocess import correspondences, solve_pnp_ransac
    from checkerpose_amd.synthetic import build_net, det_image, det_tensor
    dev = torch.device("cuda:0")
    net = build_net(seed=1).to(dev)
    with torch.no_grad():
        out = net(det_image(3, seed=5).to(dev), None)
    grid = (det_tensor("roi_xy", (3, 2, 64, 64), 300.0) + 320.0).to(dev)
    p2d, valid, count = correspondences(out, grid)
    R, t, inl, status = solve_pnp_ransac(torch.from_numpy(_model(512)).float().to(dev), p2d, valid, torch.from_numpy(K_LMO).float().to(dev))
    torch.cuda.synchronize()
    assert tuple(R.shape) == (3, 3, 3) and tuple(t.shape) == (3, 3, 1) and R.dtype == torch.float64
    assert set(status.cpu().tolist()) <= {0, 1}
    assert not (inl & ~valid[:, :, 0].bool()).any()
    for b in range(3):
        assert abs(float(torch.linalg.det(R[b])) - 1.0) < 1e-9 or int(status[b]) == 0


@pytest.mark.gpu
def test_from_id_to_pose_drop_in_signature():
    """checkerpose_amd.postprocess.from_id_to_pose: the reference's signature (numpy arrays of one image), validity mask as
    test_network_with_test_data.py:50-66 (checked against the reference-made n2 fixture's index lists), pose from the device solver."""
    from checkerpose_amd.postprocess import from_id_to_pose
    from tests.common import golden
    rng = np.random.default_rng(7)
    xyz = _model(512)
    R, t = _pose(rng)
    uv = P.project(xyz, K_LMO, R, t)
    # a 64x64 RoI grid whose cell centres are the image coordinates; each keypoint "predicts" the cell nearest to its projection
    xs = np.linspace(uv[:, 0].min() - 1, uv[:, 0].max() + 1, 64)
    ys = np.linspace(uv[:, 1].min() - 1, uv[:, 1].max() + 1, 64)
    roi_xy = np.stack(np.meshgrid(xs, ys), -1)                                          # (H, W, 2) = (x, y)
    xid = np.abs(uv[:, 0:1] - xs[None]).argmin(1)
    yid = np.abs(uv[:, 1:2] - ys[None]).argmin(1)
    roi_bit = (rng.random((512, 1)) < 0.85).astype(np.float32)
    seg = (rng.random((64, 64)) < 0.9).astype(np.float32)
    cell = max(xs[1] - xs[0], ys[1] - ys[0])
    Re, te, inl = from_id_to_pose(xyz, roi_xy, K_LMO, roi_bit, xid, yid, check_seg=True, seg_mask=seg, discard_bd_pixel=2,
                                  return_inliers=True, reprojErr_thresh=cell, cv_max_iters=150)
    want = (roi_bit[:, 0] > 0.5) & (seg[yid, xid] > 0.5) & (xid >= 2) & (xid < 62) & (yid >= 2) & (yid < 62)
    assert inl is not None and set(inl.tolist()) <= set(np.nonzero(want)[0].tolist()) and len(inl) > 0.8 * want.sum()
    assert Re.shape == (3, 3) and te.shape == (3, 1)
    assert np.abs(Re - R).max() < 0.05 and np.linalg.norm(te[:, 0] - t) < 0.05 * np.linalg.norm(t)      # quantised to the 64x64 grid
    assert len(from_id_to_pose(xyz, roi_xy, K_LMO, roi_bit, xid, yid)) == 2
    Rf, tf, inf_ = from_id_to_pose(xyz, roi_xy, K_LMO, np.zeros((512, 1), np.float32), xid, yid, return_inliers=True)
    assert np.array_equal(Rf, np.eye(3)) and not tf.any() and inf_ is None             # :111-114
    with pytest.raises(ValueError):
        from_id_to_pose(xyz, roi_xy, K_LMO, roi_bit, xid, yid, use_progressivex=True)


def test_from_id_to_pose_hands_the_solver_the_reference_lists(monkeypatch):
    """CPU: the drop-in from_id_to_pose builds exactly the (valid_p3d, valid_disc_p2d) lists the REFERENCE's own function handed to
    its (recording) solver -- n2_from_id_to_pose.npz, made by tests/golden/make_golden_r2.py from the reference's code -- for
    check_seg in {False, full, visib} x discard_bd_pixel in {0, 2}; the device solver is replaced by a recorder here."""
    import torch
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd.detweights import det_tensor
    from tests.common import golden
    g, e = golden("n2_from_id_to_pose"), golden("e2e_injected")
    rec = {}

    def recorder(p3d, p2d, valid, K, column=0, reproj_threshold=2.0, iterations=150, seed=0, return_hypotheses=False):
        rec["valid"], rec["p2d"] = valid[0, :, column].numpy().astype(bool), p2d[0].numpy()
        n = p2d.shape[1]
        return (torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3, 1, dtype=torch.float64), valid[:, :, column].bool(),
                torch.ones(1, dtype=torch.int32))
    monkeypatch.setattr(PP, "solve_pnp_ransac", recorder)
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))   # noqa: E731
    roi = np.where(sig(e["roi"]) > 0.5, 1.0, 0.0).transpose(0, 2, 1)                       # test.py:294-303
    seg = np.where(sig(e["seg"] - g["seg_shift"]) > 0.5, 1.0, 0.0)                         # test.py:313-314
    seg_visib, seg_full = seg[:, 0], seg[:, 1]
    xid, yid = e["xid"].astype(np.int64), e["yid"].astype(np.int64)
    grid = (det_tensor(str(g["grid_name"]), (2, 2, 64, 64), float(g["grid_scale"])) + float(g["grid_shift"])).numpy().transpose(0, 2, 3, 1)
    xyz = _model(512)
    for b in range(2):
        for cs, sm in (("all", None), ("full", seg_full), ("visib", seg_visib)):
            for bd in (0, 2):
                key = "b%d_%s_bd%d" % (b, cs, bd)
                R, t, inl = PP.from_id_to_pose(xyz, grid[b], np.eye(3), roi[b], xid[b], yid[b], check_seg=sm is not None,
                                               seg_mask=None if sm is None else sm[b], discard_bd_pixel=bd, return_inliers=True,
                                               device="cpu")
                assert np.nonzero(rec["valid"])[0].tolist() == g[key + "_idx"].tolist(), key
                assert np.array_equal(rec["p2d"][rec["valid"]], g[key + "_p2d"]), key
                assert inl.tolist() == g[key + "_idx"].tolist()                           # the recorder calls every valid point an inlier
