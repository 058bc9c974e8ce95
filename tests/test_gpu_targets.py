"""Row N6 on the device: checkerpose_amd.targets (cp_encode_targets, cp_code_report) against what the reference's own statements
recorded (tests/golden/targets.npz) and against the host restatements of tests/test_targets.py.

Labels, ids and every integer count must be EQUAL (the fixture keeps every decision >= 1e-6 away from a rounding boundary).
Floating-point bounds are derived, not tuned:
  proj_xy   |du| <= 64 * 2^-53 * (A_u + |u| A_z) / |z| with A_i = sum_j |P_ij| |p_j|: the forward error of a 4-term fp64 dot product
            (and of the 3-term ones that form P) and one division, with head room; the worst observed ratio is printed.
  figures   within one fp32 rounding (2^-24 relative) of the recorded ones -- the reference forms some in float32, which ones depends
            on numpy's promotion rules -- and EQUAL to the float64 figures recomputed from the counts.
  te        8 * 2^-53 * (|t_est| + |t_gt|);  re: error_cos within 64 * 2^-53 of the float64 value, so the angle within that divided by
            sqrt(1 - c^2).  The pose fixture also holds half turns (c = -1), where that quotient is unbounded: there the bound is
            acos(1 - d) with d the error_cos bound, since |acos a - acos b| <= acos(1 - |a - b|) on [-1, 1] (acos is steepest at the
            ends of the interval).  Equal poses give exactly 0.0."""
import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, targets
from checkerpose_amd import preprocess as PP
from tests.common import build_net, golden
from tests.test_targets import COUNT_KEYS, FIGURE_KEYS, enc_case, host_encode, lm_keypoints, rep_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -53


def _up(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _group(g, k):
    idx = np.nonzero(g["enc_group"] == k)[0]
    return idx, [enc_case(g, i) for i in idx]


def _finals(cs):
    return [None if c["no_det"] else c["final"] for c in cs]


def _check_labels(lab, cs, what):
    for b, c in enumerate(cs):
        assert np.array_equal(lab["roi_mask_bits"][b, 0].cpu().numpy(), c["roi"]), (what, b, "roi")
        assert np.array_equal(lab["pixel_x_codes"][b].cpu().numpy().T, c["x_code"]), (what, b, "x_code")
        assert np.array_equal(lab["pixel_y_codes"][b].cpu().numpy().T, c["y_code"]), (what, b, "y_code")
        assert np.array_equal(lab["x_id"][b].cpu().numpy(), c["x_id"]) and np.array_equal(lab["y_id"][b].cpu().numpy(), c["y_id"]), (what, b, "ids")


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)


def test_encode_targets_equals_the_reference():
    g = golden("targets")
    lib = _abi.load()
    worst = 0.0
    for k in (0, 1):                                                                      # N = 512 shared: S = 64 and S = 128
        idx, cs = _group(g, k)
        S, B = cs[0]["S"], len(cs)
        R, t = _up(g["enc_R"][idx]), _up(g["enc_t"][idx])
        lib.cp_kernel_log_begin()
        lab = targets.encode_targets(cs[0]["pts"], g["enc_K"], R, t, _finals(cs), S, return_proj=True)
        assert lib.cp_kernel_log().decode() == "encode_targets_kernel"                    # one launch per call
        assert lab["roi_mask_bits"].dtype == torch.float32 and tuple(lab["pixel_x_codes"].shape) == (B, cs[0]["bits"], 512)
        assert lab["x_id"].dtype == torch.int32 and lab["proj_xy"].dtype == torch.float64
        _check_labels(lab, cs, "group %d" % k)
        again = targets.encode_targets(cs[0]["pts"], g["enc_K"], R, t, _finals(cs), S, return_proj=True)
        assert _same(lab, again)                                                          # two calls: bit-identical
        per_crop = targets.encode_targets(_up(np.stack([c["pts"] for c in cs])), _up(np.stack([g["enc_K"]] * B)), R, t, _finals(cs), S, return_proj=True)
        table = targets.encode_targets(_up(cs[0]["pts"][None]), g["enc_K"], R, t.reshape(B, 3, 1), _finals(cs), S, obj_ids=[1] * B, return_proj=True)
        assert _same(lab, per_crop) and _same(lab, table)                                 # the three keypoint forms: identical bits
        for b, c in enumerate(cs):
            one = targets.encode_targets(c["pts"], g["enc_K"], R[b:b + 1], t[b:b + 1], _finals(cs)[b:b + 1], S, return_proj=True)
            assert all(torch.equal(one[key][0], lab[key][b]) for key in lab), (k, b, "batch != single")
            if c["no_det"]:
                assert not lab["x_id"][b].any() and not lab["proj_xy"][b].any()
                continue
            worst = max(worst, _proj_ratio(lab, b, c))
    idx, cs = _group(g, 2)                                                                # the LM twin: object table + obj_ids, N = 4096
    tab = np.stack([lm_keypoints(o, 4096) for o in (1, 2, 3)])
    obj = [c["obj"] for c in cs]
    R, t = _up(g["enc_R"][idx]), _up(g["enc_t"][idx])
    lab = targets.encode_targets(tab, g["enc_K"], R, t, _finals(cs), 64, obj_ids=torch.tensor(obj), return_proj=True)
    _check_labels(lab, cs, "lm")
    per_crop = targets.encode_targets(np.stack([c["pts"] for c in cs]), g["enc_K"], R, t, _finals(cs), 64, return_proj=True)
    assert _same(lab, per_crop)
    for b, c in enumerate(cs):
        worst = max(worst, _proj_ratio(lab, b, c))
    print("worst |d proj| / bound = %.3e" % worst)
    assert worst <= 1.0
    with pytest.raises(ValueError, match="no area"):
        targets.encode_targets(cs[0]["pts"], g["enc_K"], R[:1], t[:1], [[3, 3, 0, 10]], 64)
    with pytest.raises(ValueError, match="power of two"):
        targets.encode_targets(cs[0]["pts"], g["enc_K"], R[:1], t[:1], [[3, 3, 10, 10]], 48)
    with pytest.raises(ValueError, match="obj_ids"):
        targets.encode_targets(tab, g["enc_K"], R[:1], t[:1], [[3, 3, 10, 10]], 64, obj_ids=[4])


def _proj_ratio(lab, b, c):
    """max over the recorded keypoints of |d proj| / (64 eps (A_u + |u| A_z) / |z|); depth is held to the same dot-product bound"""
    st = c["proj_step"]
    P = c["K"] @ np.hstack((c["R"], c["t"].reshape(3, 1)))
    ph = np.abs(np.hstack((c["pts"], np.ones((c["N"], 1)))))[::st]
    A = ph @ np.abs(P).T                                                                    # (n, 3)
    got, z = lab["proj_xy"][b].cpu().numpy()[::st], lab["depth"][b].cpu().numpy()[::st]
    ref, zr = c["proj_xy"], c["depth"]
    r = 0.0
    for k in (0, 1):
        bound = 64 * EPS * (A[:, k] + np.abs(ref[:, k]) * A[:, 2]) / np.abs(zr)
        r = max(r, float((np.abs(got[:, k] - ref[:, k]) / bound).max()))
    return max(r, float((np.abs(z - zr) / (64 * EPS * A[:, 2])).max()))


def test_encode_targets_saturates():
    """quotients far beyond the int range and a non-finite pose: defined results (out of the RoI, ids at the clip / 0), no trap"""
    pts = np.array([[0.0, 0.0, 0.0], [1e3, 0.0, 0.0], [-1e3, 0.0, 0.0], [0.0, 0.0, 0.0]])
    K = np.array([[1e300, 0.0, 0.0], [0.0, 1e300, 0.0], [0.0, 0.0, 1.0]])
    R, t = _up(np.eye(3)[None]), _up(np.array([[0.0, 0.0, 1.0]]))
    lab = targets.encode_targets(pts, K, R, t, [[-5, -5, 10, 10]], 8)
    assert lab["roi_mask_bits"][0, 0].tolist() == [1.0, 0.0, 0.0, 1.0] and lab["x_id"][0].tolist() == [4, 7, 0, 4]
    bad = targets.encode_targets(pts, np.eye(3), R, _up(np.array([[float("nan"), 0.0, 1.0]])), [[-5, -5, 10, 10]], 8)
    assert not bad["roi_mask_bits"].any() and not bad["x_id"].any()


def test_code_report_equals_the_reference():
    g = golden("targets")
    lib = _abi.load()
    for name in ("rep0", "rep1", "rep2"):
        pred, lab, (group, S, nb, seg_size) = rep_case(g, name)
        B, N = pred["logit_roi"].shape[0], pred["logit_roi"].shape[2]
        block = torch.zeros(B, 13, N, device=DEV)                                          # the network's layout: slices of one logit block
        block[:, 0:1], block[:, 1:1 + nb], block[:, 7:7 + nb] = _up(pred["logit_roi"]), _up(pred["logit_x"]), _up(pred["logit_y"])
        outs = (block[:, 0:1], block[:, 1:1 + nb], block[:, 7:7 + nb], _up(pred["seg"]))
        labels = {k: _up(v) for k, v in lab.items()}
        mv, mf = _up(pred["mask_visib"]), _up(pred["mask_full"])
        lib.cp_kernel_log_begin()
        rep = targets.code_report(outs, labels, mv, mf)
        assert lib.cp_kernel_log().decode() == "code_report_kernel"
        again = targets.code_report(outs, labels, mv, mf)
        assert _same(rep, again)
        as_float = targets.code_report(tuple(o.contiguous() for o in outs), labels, mv.float() / 255.0, mf.float() / 255.0)   # the loader's 0 / 1 masks
        assert _same(rep, as_float)
        for k in COUNT_KEYS:
            assert rep[k].dtype == torch.int32 and np.array_equal(rep[k].cpu().numpy(), g["%s_%s" % (name, k)]), (name, k)
        host = targets.figures_from_counts({k: rep[k].cpu().numpy() for k in COUNT_KEYS}, N, seg_size * seg_size, nb)
        for k in FIGURE_KEYS:
            got, ref = rep[k].cpu().numpy(), g["%s_%s" % (name, k)]
            assert rep[k].dtype == torch.float64 and np.array_equal(got, host[k]), (name, k)                # fp64 from the counts: exact
            print("%s %-16s worst rel. difference to the recorded figure %.3e" % (name, k, float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)).max())))
            assert np.all(np.abs(got - ref) <= 2.0 ** -24 * np.abs(ref)), (name, k)
        for b in range(B):                                                                  # a batch of B equals B batches of one
            one = targets.code_report(tuple(o[b:b + 1] for o in outs), {k: v[b:b + 1] for k, v in labels.items()}, mv[b:b + 1], mf[b:b + 1])
            assert all(torch.equal(one[k][0], rep[k][b]) for k in rep), (name, b)
    with pytest.raises(ValueError, match="bits"):
        targets.code_report(outs, {k: v[:, :1] for k, v in labels.items()}, mv, mf)


def test_pose_re_te_against_the_reference():
    pe, g = golden("pose_error"), golden("targets")
    n = len(pe["add"])
    re, te, cos_dev = targets.pose_re_te(_up(pe["R_est"]), _up(pe["t_est"]), pe["R_gt"], pe["t_gt"], return_cos=True)
    cos_dev = cos_dev.cpu().numpy()
    assert re.dtype == torch.float64 and te.dtype == torch.float64 and tuple(re.shape) == (n,)
    re, te = re.cpu().numpy(), te.cpu().numpy()
    seen_half = seen_same = 0
    for c in range(n):
        tol_t = 8 * EPS * (np.linalg.norm(pe["t_est"][c]) + np.linalg.norm(pe["t_gt"][c]))
        assert abs(te[c] - g["pose_te"][c]) <= tol_t, (c, te[c], g["pose_te"][c])
        cos = 0.5 * (np.trace(pe["R_est"][c] @ np.linalg.inv(pe["R_gt"][c])) - 1.0)
        d = 64 * EPS
        assert abs(cos_dev[c] - cos) <= d, (c, cos_dev[c], cos)                             # error_cos itself, before the clamp
        if np.array_equal(pe["R_est"][c], pe["R_gt"][c]):
            seen_same += 1
            assert re[c] == 0.0 and g["pose_re"][c] <= np.rad2deg(np.arccos(1 - d)), (c, re[c], g["pose_re"][c])
            continue
        if abs(cos) > 1 - 1e-9:                      # half turns: the derivative bound is void, the Hoelder bound holds (module docstring)
            seen_half += 1
            tol = np.rad2deg(np.arccos(1 - d))
        else:
            tol = np.rad2deg(d / np.sqrt(1 - cos * cos))
        print("case %2d %-5s re %.9f ref %.9f |diff| %.3e tol %.3e" % (c, pe["tag"][c], re[c], g["pose_re"][c], abs(re[c] - g["pose_re"][c]), tol))
        assert abs(re[c] - g["pose_re"][c]) <= tol, (c, re[c], g["pose_re"][c], tol)
    assert seen_same >= 5 and seen_half >= 2


def _scene(B, seed=0, W=640, H=480):
    """B synthetic samples: a uint8 noise frame each, a rendered disc as the full mask, the disc minus a half plane as the visible one,
    a GT pose whose keypoints project into the disc's neighbourhood, and the visible mask's bounding box"""
    rng = np.random.default_rng(seed)
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    frames = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    full, vis, Rs, ts, boxes = [], [], [], [], []
    for b in range(B):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q *= np.sign(np.linalg.det(q))
        t = np.array([rng.uniform(-60, 60), rng.uniform(-40, 40), rng.uniform(500, 700)])
        u, v = K[0, 0] * t[0] / t[2] + K[0, 2], K[1, 1] * t[1] / t[2] + K[1, 2]
        r = K[0, 0] * 60.0 / t[2]
        f = (xx - u) ** 2 + (yy - v) ** 2 <= r * r
        m = f & (xx < u + 0.5 * r)
        ys, xs = np.nonzero(m)
        boxes.append([int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)])
        full.append(f.astype(np.uint8) * 255); vis.append(m.astype(np.uint8) * 255); Rs.append(q); ts.append(t)
    return frames, np.stack(vis), np.stack(full), np.stack(Rs), np.stack(ts), K, boxes


def test_make_training_batch_feeds_a_training_step():
    from checkerpose_amd.losses.code_loss import MaskedCodeLoss, UnmaskedCodeLoss
    from checkerpose_amd.losses.mask_loss import MaskLoss_interpolate
    B, S = 2, 64
    frames, vis, full, Rs, ts, K, boxes = _scene(B, seed=3)
    pts = lm_keypoints(1, 512)
    fr, mv, mf, R, t = _up(frames), _up(vis), _up(full), _up(Rs), _up(ts)
    np.random.seed(11)
    batch = targets.make_training_batch(fr, mv, mf, R, t, K, boxes, pts, is_train=True)
    assert len(batch) == 11
    roi_x, m_full, m_vis, R_o, t_o, Bbox, K_o, roi_gt, x_gt, y_gt, roi_xy = batch
    np.random.seed(11)
    grown = [targets.aug_Bbox(np.array(b), 1.5) for b in boxes]                             # the same draws, in the same order
    final = np.array([PP.get_final_Bbox(b, "crop_square_resize", 640, 480) for b in grown])
    assert roi_x.dtype == torch.uint8 and torch.equal(roi_x, PP.get_roi_batch(fr, grown, 256, PP.INTER_LINEAR))
    assert torch.equal(m_vis, PP.get_roi_batch(mv[..., None], grown, S, PP.INTER_NEAREST)[..., 0].float() / 255.0)
    assert torch.equal(m_full, PP.get_roi_batch(mf[..., None], grown, S, PP.INTER_NEAREST)[..., 0].float() / 255.0)
    assert set(m_vis.unique().tolist()) <= {0.0, 1.0} and 0 < float(m_vis.mean()) < float(m_full.mean())
    assert np.array_equal(Bbox.cpu().numpy(), final) 
    assert all(torch.is_tensor(x) and x.is_cuda for x in batch)                             # the whole tuple lives on the device
    assert torch.equal(R_o, R) and torch.equal(t_o, t) and K_o.dtype == torch.float64 and np.array_equal(K_o.cpu().numpy(), K)
    lab = targets.encode_targets(pts, K, R, t, final, S)
    assert torch.equal(roi_gt, lab["roi_mask_bits"]) and torch.equal(x_gt, lab["pixel_x_codes"]) and torch.equal(y_gt, lab["pixel_y_codes"])
    host = [host_encode(pts, K, Rs[b], ts[b], final[b], S) for b in range(B)]            # the golden-equal restatement, from host arrays
    h_roi = _up(np.stack([h["roi"][None] for h in host]), torch.float32)
    h_x = _up(np.stack([h["x_code"].T for h in host]), torch.float32)
    h_y = _up(np.stack([h["y_code"].T for h in host]), torch.float32)
    assert torch.equal(roi_gt, h_roi) and torch.equal(x_gt, h_x) and torch.equal(y_gt, h_y)
    assert 0.2 < float(roi_gt.mean()) <= 1.0
    for b in range(B):                                                                      # the loader's coordinate grid: its 4 corners, float64 -> float32
        sx, sy = final[b, 2] / S, final[b, 3] / S
        ref = np.array([[final[b, 0], final[b, 1]], [sx * (S - 1) + final[b, 0], final[b, 1]], [final[b, 0], sy * (S - 1) + final[b, 1]],
                        [sx * (S - 1) + final[b, 0], sy * (S - 1) + final[b, 1]]]).astype(np.float32)
        got = roi_xy[b].permute(1, 2, 0)[[0, 0, -1, -1], [0, -1, 0, -1]].cpu().numpy()
        assert tuple(roi_xy.shape) == (B, 2, S, S) and np.array_equal(got, ref), (b, got, ref)
    g = golden("targets")
    for i in np.nonzero(~g["enc_no_det"])[0]:                                               # ... and against the reference's recorded corners
        c = enc_case(g, i)
        grid = targets.roi_xy_grid([c["final"]], c["S"], DEV)[0].permute(1, 2, 0)[[0, 0, -1, -1], [0, -1, 0, -1]].cpu().numpy()
        assert np.array_equal(grid, c["corners"]), i
    # one training step on this batch against the same step fed labels made on the host
    net = build_net(seed=3).cuda().train()
    roi_loss, bit_loss, seg_loss = UnmaskedCodeLoss("BCE"), MaskedCodeLoss("BCE"), MaskLoss_interpolate()

    def step(roi_t, x_t, y_t, v_t, f_t):
        net.zero_grad()
        with torch.enable_grad():
            roi, xb, yb, seg, _, _ = net(roi_x, None, 3)
            nb = xb.shape[1]
            parts = [roi_loss(roi, roi_t), bit_loss(xb, x_t[:, :nb], roi_t), bit_loss(yb, y_t[:, :nb], roi_t), seg_loss(seg[:, 0:1], v_t),
                     seg_loss(seg[:, 1:2], f_t)]
            sum(parts).backward()
        torch.cuda.synchronize()
        return [float(p.detach()) for p in parts]

    got = step(roi_gt, x_gt, y_gt, m_vis, m_full)
    ref = step(h_roi, h_x, h_y, _up(np.stack([v for v in m_vis.cpu().numpy()])), _up(np.stack([v for v in m_full.cpu().numpy()])))
    print("losses on the device-made batch", got, "on host-made labels", ref)
    assert all(np.isfinite(v) and v > 0 for v in got)
    for a, b in zip(got, ref):
        assert abs(a - b) <= 1e-3 * abs(b), (got, ref)                                      # tests/test_gpu_train_step.py: first-step losses


def test_make_training_batch_test_mode_and_lm_form():
    B = 3
    frames, vis, full, Rs, ts, K, boxes = _scene(B, seed=5)
    tab = np.stack([lm_keypoints(o, 512) for o in (1, 2, 3)])
    boxes[1] = None                                                                         # no detection: the loader's dummy sample
    out = targets.make_training_batch(_up(frames), _up(vis), _up(full), _up(Rs), _up(ts), K, boxes, tab, is_train=False, obj_ids=[3, 1, 2])
    assert len(out) == 12 and out[7].is_cuda and out[7].tolist() == [3, 1, 2]
    roi_x, m_full, m_vis, _, _, Bbox, _, _, roi_gt, x_gt, y_gt, roi_xy = out
    assert not roi_x[1].any() and not m_vis[1].any() and not Bbox[1].any() and not roi_gt[1].any() and not x_gt[1].any() and not roi_xy[1].any()
    padded = [None if b is None else PP.padding_Bbox(b, 1.5) for b in boxes]
    final = [None if b is None else PP.get_final_Bbox(b, "crop_square_resize", 640, 480) for b in padded]
    for b, o in ((0, 3), (2, 2)):
        h = host_encode(tab[o - 1], K, Rs[b], ts[b], final[b], 64)
        assert np.array_equal(roi_gt[b, 0].cpu().numpy(), h["roi"]) and np.array_equal(y_gt[b].cpu().numpy().T, h["y_code"])
        assert np.array_equal(Bbox[b].cpu().numpy(), final[b])
    with pytest.raises(ValueError, match="ground-truth box"):
        targets.make_training_batch(_up(frames), _up(vis), _up(full), _up(Rs), _up(ts), K, boxes, tab[0])


def test_evaluate_batch_end_to_end():
    from checkerpose_amd import metric
    B = 3
    frames, vis, full, Rs, ts, K, boxes = _scene(B, seed=9)
    boxes[2] = None
    pts = lm_keypoints(1, 512)
    net = build_net(seed=1).cuda().eval()
    ms = metric.MeshSet.from_arrays([pts.astype(np.float32)], diameters=[100.0])
    res = targets.evaluate_batch(net, _up(frames), _up(vis), _up(full), boxes, pts.astype(np.float32), K, Rs, ts, ms)
    rep = targets.code_report(res["outputs"], res["labels"], *res["mask_crops"])
    assert all(torch.equal(rep[k], res["report"][k]) for k in rep) and set(rep) == set(res["report"])
    padded = [None if b is None else PP.padding_Bbox(b, 1.5) for b in boxes]
    final = [None if b is None else PP.get_final_Bbox(b, "crop_square_resize", 640, 480) for b in padded]
    lab = targets.encode_targets(pts, K, _up(Rs), ts, final, 64)
    assert all(torch.equal(lab[k], res["labels"][k]) for k in lab)
    assert torch.equal(res["mask_crops"][0], PP.get_roi_batch(_up(vis)[..., None], padded, 64, PP.INTER_NEAREST)[..., 0])
    for name in targets.COLUMNS:
        col = res[name]
        assert tuple(col["R"].shape) == (B, 3, 3) and tuple(col["re"].shape) == (B,) and set(col["errors"]) == {"add", "adi"}
        re, te = targets.pose_re_te(Rs, ts, col["R"], col["t"])                               # test.py's argument order
        assert torch.equal(re, col["re"]) and torch.equal(te, col["te"])
        assert bool(torch.isfinite(col["re"]).all()) and bool(torch.isfinite(col["te"]).all())
    assert int(res["report"]["n_in_roi"][2]) == 0 and float(res["report"]["reproj_x_acc"][2]) == 1.0      # the missing detection
    table, text = targets.summarize_report([res, res], 100.0)
    keys = [ln.split(" ", 1)[0] for ln in text.splitlines()]
    assert keys[:7] == ["acc", "adx2", "adx5", "adx10", "adx_err", "re", "te"] and keys[7] == "full_adx2" and "visib_te" in keys
    assert keys[keys.index("visib_te") + 1:keys.index("visib_te") + 9] == ["roi_bit_acc", "reproj_x_acc", "reproj_y_acc", "bit_err_arr",
                                                                           "visib_pixel_acc", "visib_iou", "full_pixel_acc", "full_iou"]
    assert keys[-6:] == ["AUC_posecnn_ADD", "full_AUC_posecnn_ADD", "visib_AUC_posecnn_ADD", "AUC_posecnn_ADI", "full_AUC_posecnn_ADI",
                         "visib_AUC_posecnn_ADI"]
    assert abs(table["roi_bit_acc"] - float(res["report"]["roi_bit_acc"].mean())) <= 1e-12 and table["bit_err_arr"].shape == (13,)
