"""Row N34 on the device: every committed case of tests/calib_stages.py through its checker -- integers with ==, floating sums within
the derived bound, the fit by its certificate -- plus what only the device can show: two calls bitwise equal, halves that add to the
whole, a crop alone against the same crop in a batch, the two accumulate kernels agreeing bitwise, CalibratedNet inside the wrappers."""
import math

import numpy as np
import pytest
import torch

from tests import calib_stages as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT_KEYS = ("count", "positives", "n", "n_nan", "n_right")
ALL_KEYS = INT_KEYS + ("sum_p", "nll", "brier", "g", "h")


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(d):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


def _labels(case, rows=slice(None)):
    return dict(roi_mask_bits=_t(case["roi"][rows]), pixel_x_codes=_t(case["gx"][rows]), pixel_y_codes=_t(case["gy"][rows]))


def _bits(case, rows=slice(None)):
    K = 1 + 2 * case["r"]
    return _t(case["block"][rows])[:, :K, :]              # a view of the wider block where the case has one: a batch stride


def _same(a, b, keys):
    return all(torch.equal(a[k].view(torch.int64) if a[k].dtype == torch.float64 else a[k], b[k].view(torch.int64) if b[k].dtype == torch.float64 else b[k])
               for k in keys)


# ------------------------------------------------------------------------------------------------------------- reliability
REL = S.reliability_cases()


@pytest.mark.parametrize("case", REL, ids=[c["name"] for c in REL])
def test_reliability_against_the_oracle(case):
    from checkerpose_amd.postprocess import add_reliability, reliability
    bits, labels = _bits(case), _labels(case)
    if case["block"].shape[1] > bits.shape[1] and bits.shape[0] > 1:
        assert not bits.is_contiguous()
    acc = reliability(bits, labels, scale=case["scale"], bins=case["M"])
    assert np.array_equal(acc["edges"].cpu().numpy(), case["edges"]) and np.array_equal(acc["scale"].cpu().numpy(), case["scale"])
    ratios = {}
    S.check_reliability(case, _np(acc), ratios)
    print("%s: largest |device - fsum| / ((n + 8) 2^-53 fsum|terms|): %s" % (case["name"], {k: round(v, 3) for k, v in ratios.items()}))
    again = reliability(bits.contiguous(), labels, scale=torch.from_numpy(case["scale"]), bins=case["M"])
    assert _same(acc, again, ALL_KEYS)                                            # bitwise, with and without the batch stride
    B = bits.shape[0]
    if B > 1:
        h = B // 2
        a = reliability(_bits(case, slice(0, h)), _labels(case, slice(0, h)), scale=case["scale"], bins=case["M"])
        b = reliability(_bits(case, slice(h, B)), _labels(case, slice(h, B)), scale=case["scale"], bins=case["M"])
        assert _same(add_reliability(a, b), acc, INT_KEYS)                        # counts add exactly


def test_reliability_figures_from_device_accumulators():
    from checkerpose_amd.postprocess import reliability, reliability_figures
    case = S.bits_case(17, 512, 6, 15, 150, scale="ones")
    fig = reliability_figures(reliability(_bits(case), _labels(case)))           # the defaults: no scale, 15 bins
    o = S.reliability(case)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(o["count"] > 0, np.abs(o["positives"] / o["count"] - o["sum_p"] / o["count"]), 0.0)
    assert np.allclose(fig["ece"], (o["count"] * gap).sum(1) / o["n"], rtol=1e-12) and np.allclose(fig["mce"], gap.max(1), rtol=1e-12)
    assert np.array_equal(fig["accuracy"], o["n_right"] / o["n"]) and np.allclose(fig["nll"], o["nll"] / o["n"], rtol=1e-12)
    print("ECE per row %s" % np.round(fig["ece"], 4).tolist())


# ------------------------------------------------------------------------------------------------------------- the fit
FIT = S.fit_cases()


def _fit(case, **kw):
    from checkerpose_amd.postprocess import fit_code_scale
    a = dict(groups=case["groups"], s_min=case["s_min"], s_max=case["s_max"], step_tol=case["step_tol"], max_iters=case["max_iters"])
    a.update(kw)
    scale, info = fit_code_scale(_bits(case), _labels(case), **a)
    return scale, info


@pytest.mark.parametrize("case", FIT, ids=[c["name"] for c in FIT])
def test_fit_is_certified_by_the_oracle(case):
    from checkerpose_amd.postprocess import reliability
    scale, info = _fit(case)
    K = 1 + 2 * case["r"]
    assert scale.dtype == torch.float64 and tuple(scale.shape) == (K,) and info["status"].dtype == torch.int32
    out = dict(_np(info), scale=scale.cpu().numpy())
    ratios, report = {}, []
    S.check_fit(case, out, ratios, report)
    print("%s: status %s, evaluations %s, s %s" % (case["name"], out["status"].tolist(), out["iters"].tolist(), np.round(out["s"], 6).tolist()))
    assert (out["nll_after"] <= out["nll_before"]).all()
    scale2, info2 = _fit(case)
    assert torch.equal(scale, scale2) and _same(info, info2, ("status", "iters", "nll_before", "nll_after", "n", "s", "lo", "hi"))
    if "recovery" in case["name"]:
        grp = S.group_rows(case["groups"], case["r"]).tolist()
        for gi, s, n, h in report:
            if out["status"][gi] == S.OK:
                s0, se = case["s0"][grp.index(gi)], 1.0 / math.sqrt(h)
                print("   group %d: s* = %.6f, s0 = %.6f: %.2f standard errors of 1 / sqrt(h) = %.4f (n = %d)" % (gi, s, s0, (s - s0) / se, se, n))
                assert abs(s - s0) <= 5.0 * se
    if case["groups"] == "row" and np.isfinite(out["nll_after"]).all():
        # the fit's accumulate kernel and the reliability kernel add the same terms in the same order: bitwise the same NLL at the returned s
        rel = reliability(_bits(case), _labels(case), scale=scale, bins=2)
        assert torch.equal(rel["nll"], info["nll_after"]) and torch.equal(rel["n"], info["n"])
        ones = reliability(_bits(case), _labels(case), bins=2)
        assert torch.equal(ones["nll"], info["nll_before"])


def test_fit_statuses_and_frozen_groups():
    sep = _fit(S.fit_case(3, 64, 6, 305, kind="separable"))[1]
    assert (sep["status"] == S.CAPPED_HIGH).all() and (sep["s"] == 64.0).all()
    anti = _fit(S.fit_case(3, 63, 6, 306, kind="antiseparable"))[1]
    assert (anti["status"] == S.CAPPED_LOW).all() and (anti["s"] == 2.0 ** -6).all()
    scale, empty = _fit(S.fit_case(3, 65, 6, 308, kind="no_roi"))
    assert (empty["status"][1:] == S.EMPTY).all() and (scale[1:] == 1.0).all() and (empty["n"][1:] == 0).all() and (empty["iters"][1:] == 1).all()
    # a group that has stopped is frozen: more launches after it leave its numbers untouched
    case = S.fit_case(3, 257, 6, 300)
    s60, i60 = _fit(case, max_iters=60)
    s200, i200 = _fit(case, max_iters=200)
    assert torch.equal(s60, s200) and _same(i60, i200, ("status", "iters", "nll_before", "nll_after", "s", "lo", "hi"))
    assert int(i60["iters"].max()) < 20


# ------------------------------------------------------------------------------------------------------------- sigma2 consistency
PIT = S.pit_cases()


def _pit(case, rows=slice(None), **kw):
    from checkerpose_amd.postprocess import sigma2_consistency
    targets = dict(proj_xy=_t(case["proj"][rows]), roi_mask_bits=_t(case["roi"][rows]))
    bins = case["edges"] if len(case["edges"]) else 1
    return sigma2_consistency(_t(case["p2d"][rows]), _t(case["valid"][rows]), _t(case["sigma2"][rows]), targets, column=case["column"], bins=bins, **kw)


@pytest.mark.parametrize("case", PIT, ids=[c["name"] for c in PIT])
def test_sigma2_consistency_against_the_oracle(case):
    out = _pit(case)
    ratios = {}
    S.check_pit(case, _np(out), ratios)
    print("%s: largest |device - fsum| / ((n + 8) 2^-53 fsum|terms|): %s" % (case["name"], {k: round(v, 3) for k, v in ratios.items()}))
    again = _pit(case)
    keys = ("counts", "n", "n_dropped", "sum_d2", "sum_u", "sum_v", "gate_counts")
    assert _same(out, again, keys)
    o = S.pit(case)
    gates = np.array([[int((d2 < g).sum()) for g in (5.99, 9.21)] for d2 in o["d2"]], dtype=np.int64)
    assert np.array_equal(out["gate_counts"].cpu().numpy(), gates)
    n = int(o["n"].sum())
    assert out["n_total"] == n and out["n_dropped_total"] == int(o["n_dropped"].sum()) and np.array_equal(out["counts_total"], o["counts"].sum(0))
    if n:
        assert np.array_equal(out["coverage"], gates.sum(0) / n) and abs(out["inflation"] - S.fs(o["sum_d2"]) / (2 * n)) <= 1e-12 * abs(out["inflation"])
    else:
        assert np.isnan(out["coverage"]).all() and np.isnan(out["inflation"])
    B = case["p2d"].shape[0]
    if B >= 3:                                                                   # a crop alone == the same crop inside a batch of 3
        three = _pit(case, slice(0, 3))
        for b in range(3):
            alone = _pit(case, slice(b, b + 1))
            assert all(torch.equal(alone[k][0], three[k][b]) for k in keys), b


def test_sigma2_consistency_reads_a_true_variance_as_one():
    """the instrument on data that ARE chi-square with 2 degrees of freedom: coverage and inflation within 5 binomial / normal sigmas"""
    from checkerpose_amd.postprocess import sigma2_consistency
    rng = np.random.default_rng(77)
    B, N = 17, 512
    proj = rng.uniform(50.0, 400.0, size=(B, N, 2))
    s2 = rng.uniform(0.5, 20.0, size=(B, N, 2))
    for spread, infl in ((1.0, 1.0), (2.0, 4.0)):
        p2d = proj + np.sqrt(s2) * rng.normal(size=(B, N, 2)) * spread
        out = sigma2_consistency(_t(p2d, torch.float32), torch.ones(B, N, 3, dtype=torch.uint8, device=DEV), _t(s2),
                                 dict(proj_xy=_t(proj), roi_mask_bits=torch.ones(B, 1, N, device=DEV)))
        n = B * N
        print("spread %.0f: coverage %s, inflation %.4f, bins %s" % (spread, out["coverage"].tolist(), out["inflation"], out["counts_total"].tolist()))
        assert out["n_total"] == n and abs(out["inflation"] - infl) <= 5.0 * infl / math.sqrt(n)      # d2 / 2 has variance 1 per point
        if spread == 1.0:
            for cov, q in zip(out["coverage"], (1.0 - math.exp(-5.99 / 2), 1.0 - math.exp(-9.21 / 2))):
                assert abs(cov - q) <= 5.0 * math.sqrt(q * (1.0 - q) / n)
            assert (np.abs(out["counts_total"] - n / 10) <= 5.0 * math.sqrt(n * 0.09)).all()           # ten equal-probability bins
        else:
            assert out["coverage"][0] < 0.6


# ------------------------------------------------------------------------------------------------------------- empty batches, refusals
def test_empty_batches_and_host_tensors():
    from checkerpose_amd import postprocess as Q
    bits = torch.zeros(0, 13, 8, device=DEV)
    labels = dict(roi_mask_bits=torch.zeros(0, 1, 8, device=DEV), pixel_x_codes=torch.zeros(0, 6, 8, device=DEV), pixel_y_codes=torch.zeros(0, 6, 8, device=DEV))
    acc = Q.reliability(bits, labels)
    assert tuple(acc["count"].shape) == (13, 15) and not acc["count"].any() and not acc["n"].any() and not acc["nll"].any()
    scale, info = Q.fit_code_scale(bits, labels, groups="significance")
    assert (scale == 1.0).all() and (info["status"] == S.EMPTY).all() and tuple(info["status"].shape) == (7,)
    out = Q.sigma2_consistency(torch.zeros(0, 8, 2, device=DEV), torch.zeros(0, 8, 3, dtype=torch.uint8, device=DEV),
                               torch.zeros(0, 8, 2, dtype=torch.float64, device=DEV),
                               dict(proj_xy=torch.zeros(0, 8, 2, dtype=torch.float64, device=DEV), roi_mask_bits=torch.zeros(0, 1, 8, device=DEV)))
    assert tuple(out["counts"].shape) == (0, 10) and out["n_total"] == 0 and np.isnan(out["inflation"])
    case = S.bits_case(2, 8, 6, 15, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.reliability(_bits(case).cpu(), _labels(case))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.fit_code_scale(_bits(case), dict(_labels(case), pixel_x_codes=torch.from_numpy(case["gx"])))
    from checkerpose_amd import _abi
    assert _abi.load().cp_version() >= 244


# ------------------------------------------------------------------------------------------------------------- CalibratedNet
def test_calibrated_net_inside_the_wrappers():
    from checkerpose_amd import postprocess as Q
    from checkerpose_amd.synthetic import build_net
    rng = np.random.default_rng(9)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 480, 640, 3), dtype=np.uint8)).cuda()
    boxes = [[100, 80, 120, 90], [300, 200, 60, 140], None, [-10, 400, 90, 90]]
    idx = [0, 1, 0, 1]
    net = build_net(npoint=512, seed=1).cuda().eval()
    net.set_compute_dtype("bf16")
    from tests import pnp_stages as P
    p3d = torch.from_numpy(P.lmo_model(512).astype(np.float32)).cuda()
    K = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]], dtype=np.float32)
    conf = dict(chi2_threshold=9.21)
    bare = Q.estimate_poses_conf(net, frames, boxes, p3d, K, conf, return_info=True, img_index=idx, seed=3)
    ones = Q.estimate_poses_conf(Q.CalibratedNet(net, np.ones(13)), frames, boxes, p3d, K, conf, return_info=True, img_index=idx, seed=3)
    assert all(torch.equal(a, b) for a, b in zip(bare[:4], ones[:4])) and np.array_equal(bare[4], ones[4])
    assert all(torch.equal(bare[5][k], ones[5][k]) for k in bare[5])                                    # sigma2, the ranking: bitwise
    scale = rng.uniform(0.4, 2.5, size=13)
    keep0, keep1 = {}, {}
    Q._forward_correspondences(net, frames, boxes, img_index=idx, keep=keep0)
    final = Q._forward_correspondences(Q.CalibratedNet(net, torch.from_numpy(scale)), frames, boxes, img_index=idx, keep=keep1)[2]
    assert torch.equal(keep0["p2d"], keep1["p2d"]) and torch.equal(keep0["valid"], keep1["valid"])
    out0, out1 = keep0["outputs"], keep1["outputs"]
    assert torch.equal(out0[3], out1[3]) and torch.equal(out0[4], out1[4]) and torch.equal(out0[5], out1[5])
    block = out0[0]._base if out0[0]._base is not None else torch.cat(out0[:3], 1)
    scaled = block * torch.from_numpy(scale).to(torch.float32).to(DEV).reshape(1, 13, 1)
    assert out1[0]._base is not None and tuple(out1[0]._base.shape) == (4, 13, 512) and torch.equal(out1[0]._base, scaled)
    manual = (scaled[:, :1], scaled[:, 1:7], scaled[:, 7:]) + tuple(out0[3:])
    assert torch.equal(Q.code_confidence(out1, final), Q.code_confidence(manual, final))
    assert not torch.equal(Q.code_confidence(out1, final), Q.code_confidence(out0, final))
    # the calibrated net through the other wrappers that take `net`
    w = Q.estimate_poses_weighted(Q.CalibratedNet(net, scale), frames, boxes, p3d, K, dict(huber_delta=2.5, fit="valid"), img_index=idx, seed=3)
    assert tuple(w[0].shape) == (4, 3, 3) and torch.isfinite(w[0]).all()
