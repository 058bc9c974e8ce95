"""Row N34 on the CPU: the numpy restatement of the calibration instruments (tests/calib_stages.py) checks itself on every committed
case, its checker catches every named tampering at its named stage, the fit's certificate and the 5-sigma recovery hold on the oracle,
no committed whitened residual sits undecidably close to an edge, the figures are what their formulas say, and the entry points and
wrappers refuse what they must.  No device needed."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

from tests import calib_stages as S

INF = float("inf")


# ------------------------------------------------------------------------------------------------------------- the oracle on itself
def test_oracle_passes_its_own_checker_on_every_case():
    for case in S.reliability_cases():
        o = S.reliability(case)
        S.check_reliability(case, o)
        K = 1 + 2 * case["r"]
        assert (o["count"].sum(1) == o["n"]).all() and (o["positives"] <= o["count"]).all() and o["count"].shape == (K, case["M"])
        assert o["n"][0] + o["n_nan"][0] == case["roi"].size                     # row 0 counts every keypoint
        n_roi = int((case["roi"] > 0.5).sum())
        assert ((o["n"][1:] + o["n_nan"][1:]) == n_roi).all(), case["name"]      # the x / y rows: inside the GT RoI only
    for case in S.pit_cases():
        o = S.pit(case)
        S.check_pit(case, o)
        assert ((o["n"] + o["n_dropped"]) == case["valid"].shape[1]).all() and (o["counts"].sum(1) == o["n"]).all()


def test_cases_cover_what_the_rule_can_get_wrong():
    rel = S.reliability_cases()
    assert {c["bits"].shape[2] for c in rel} >= set(S.N_LIST) and {c["bits"].shape[0] for c in rel} >= set(S.B_LIST)
    assert {c["r"] for c in rel} == {1, 6} and {c["M"] for c in rel} == {1, 2, 15, 64}
    assert any(c["block"].shape[1] > c["bits"].shape[1] for c in rel)                                  # a batch stride
    special = [c for c in rel if c["name"].startswith("special")]
    seen = np.concatenate([c["bits"].reshape(-1) for c in special])
    assert np.isnan(seen).any() and np.isposinf(seen).any() and np.isneginf(seen).any() and (seen == np.float32(1e30)).any()
    assert (seen == np.float32(-1e30)).any() and ((seen == 0) & np.signbit(seen)).any() and ((seen == 0) & ~np.signbit(seen)).any()
    on_edge = 0
    for c in special:
        for k in range(1 + 2 * c["r"]):
            z, _ = S.row_samples(c, k)
            with np.errstate(all="ignore"):
                on_edge += int(np.isin(z[~np.isnan(z)].astype(np.float64) * c["scale"][k], c["edges"]).sum())
    assert on_edge > 100                                                                               # products exactly on an edge
    o = S.reliability(next(c for c in rel if c["name"].startswith("empty_crop")))
    assert o["n"][1] > 0
    assert S.reliability(next(c for c in rel if c["name"].startswith("no_roi")))["n"][1:].sum() == 0
    pit = S.pit_cases()
    assert {c["column"] for c in pit} == {0, 1, 2} and {c["p2d"].shape[1] for c in pit} >= set(S.N_LIST)
    bad = np.concatenate([c["sigma2"].reshape(-1) for c in pit if "bad" in c["name"]])
    assert np.isnan(bad).any() and np.isinf(bad).any() and (bad < 0).any() and ((bad == 0) & np.signbit(bad)).any() and ((bad == 0) & ~np.signbit(bad)).any()
    for c in pit:
        if "bad" in c["name"]:                       # one axis only: the other variance of a bad point is good
            s2 = c["sigma2"]
            with np.errstate(invalid="ignore"):
                good = np.isfinite(s2) & (s2 > 0)
            assert not (~good).all(2).any() and (~good).any()


def test_no_committed_residual_is_undecided_and_the_on_edge_points_are_exact():
    hits = 0
    for case in S.pit_cases():
        o = S.pit(case)
        assert S.pit_undecided(case, o) == 0, case["name"]
        if "on_edge" in case["name"]:
            hits += sum(int((d2 == 1.0).sum()) for d2 in o["d2"])
            # an on-edge point goes to the UPPER bin: edges 0.25, 1.0, ..: d2 == 1.0 is bin 2
            assert all((np.searchsorted(case["edges"], d2[d2 == 1.0], side="right") == 2).all() for d2 in o["d2"])
    assert hits > 100


@pytest.mark.parametrize("name", list(S.TAMPERINGS))
def test_tamperings_are_caught_by_their_named_stage(name):
    kind, make, tamper, stage = S.TAMPERINGS[name]
    case = make()
    S.CHECKERS[kind](case, S.ORACLES[kind](case))
    with pytest.raises(S.StageError) as e:
        S.CHECKERS[kind](case, tamper(case))
    assert e.value.stage == stage, str(e.value)


# ------------------------------------------------------------------------------------------------------------- the fit
def test_fit_oracle_is_certified_and_recovers_the_truth():
    seen = set()
    for case in S.fit_cases():
        o, report = S.fit(case), []
        S.check_fit(case, o, report=report)
        seen |= set(o["status"].tolist())
        assert (o["nll_after"] <= o["nll_before"]).all(), case["name"]
        if "recovery" in case["name"]:
            grp = S.group_rows(case["groups"], case["r"]).tolist()
            for gi, s, n, h in report:
                if o["status"][gi] != S.OK:
                    continue
                s0, se = case["s0"][grp.index(gi)], 1.0 / math.sqrt(h)
                print("%s group %d: s* = %.6f, s0 = %.6f, %.2f standard errors (n = %d)" % (case["name"], gi, s, s0, (s - s0) / se, n))
                assert abs(s - s0) <= 5.0 * se
    assert seen == {S.OK, S.CAPPED_HIGH, S.CAPPED_LOW, S.EMPTY, S.NOT_CONVERGED}
    sep = S.fit(S.fit_case(3, 64, 6, 305, kind="separable"))
    assert (sep["status"] == S.CAPPED_HIGH).all() and (sep["s"] == 64.0).all()
    anti = S.fit(S.fit_case(3, 63, 6, 306, kind="antiseparable"))
    assert (anti["status"] == S.CAPPED_LOW).all() and (anti["s"] == 2.0 ** -6).all()
    assert (S.fit(S.fit_case(3, 65, 6, 308, kind="no_roi"))["status"][1:] == S.EMPTY).all()


def test_newton_alone_leaves_the_bracket_on_the_committed_case():
    case = S.fit_case(3, 257, 6, 311, kind="newton_leaves", groups="significance")
    n, nll, g, h = S.group_eval(case, [0], 1.0)[:4]
    assert not case["s_min"] < 1.0 - g / h < case["s_max"]
    assert (S.fit(case)["status"] == S.OK).all()


def test_group_forms():
    assert S.group_rows("row", 6).tolist() == list(range(13))
    assert S.group_rows("significance", 6).tolist() == [0, 1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6]
    assert S.group_rows("all", 1).tolist() == [0, 0, 0]
    from checkerpose_amd import calibrate as M
    for r in (1, 6):
        for form in ("row", "significance", "all"):
            g, G = M._groups(form, r)
            assert g.tolist() == S.group_rows(form, r).tolist() and G == g.max() + 1 and g.dtype == np.int32
    assert M._groups([0, 2, 2], 1) [0].tolist() == [0, 2, 2]
    for bad in ("bit", [0, 1], [0, 1, 3], [0, -1, 1], [0.5, 1, 1]):
        with pytest.raises(ValueError, match="groups"):
            M._groups(bad, 1)


# ------------------------------------------------------------------------------------------------------------- edges and figures
def test_edge_tables():
    from checkerpose_amd import calibrate as M
    for n in (1, 2, 15, 64):
        assert np.array_equal(M.logit_edges(n), S.logit_edges(n)) and np.array_equal(M.chi2_edges(n), S.chi2_edges(n))
        assert len(M.logit_edges(n)) == n - 1
    assert M.logit_edges(2).tolist() == [0.0] and M.logit_edges(4)[1] == 0.0
    assert np.allclose(M.logit_edges([0.1, 0.5, 0.9]), [math.log(1 / 9), 0.0, math.log(9)])
    assert abs(M.chi2_edges(20)[18] - 5.99) < 0.01 and abs(-2.0 * math.log(0.01) - 9.21) < 0.01          # the 95 % / 99 % quantiles
    for bad in (0, 65, -1):
        with pytest.raises(ValueError, match="bins"):
            M.logit_edges(bad)
        with pytest.raises(ValueError, match="bins"):
            M.chi2_edges(bad)
    for bad in ([0.5, 0.5], [0.6, 0.4], [0.0, 0.5], [0.5, 1.0], [float("nan")], np.linspace(0.01, 0.99, 64)):
        with pytest.raises(ValueError, match="bins"):
            M.logit_edges(bad)
    for bad in ([1.0, 1.0], [2.0, 1.0], [float("nan")], np.arange(64.0)):
        with pytest.raises(ValueError, match="bins"):
            M.chi2_edges(bad)


def _as_torch(o, case):
    acc = {k: torch.from_numpy(np.asarray(o[k])) for k in ("count", "positives", "n", "n_nan", "n_right", "sum_p", "nll", "brier", "g", "h")}
    acc["edges"], acc["scale"] = torch.from_numpy(case["edges"]), torch.from_numpy(case["scale"])
    return acc


def test_reliability_figures_and_add_reliability():
    from checkerpose_amd import calibrate as M
    case = S.bits_case(3, 257, 6, 15, 100, scale="ones")
    o = S.reliability(case)
    fig = M.reliability_figures(_as_torch(o, case))
    for k in range(13):
        z, y = S.row_samples(case, k)
        c = S.terms(z, y, 1.0)
        b = S.bin_of(c["t"], case["edges"])
        gaps = [abs(y[b == m].mean() - c["p"][b == m].mean()) for m in range(15) if (b == m).any()]
        ece = sum((b == m).sum() / len(z) * abs(y[b == m].mean() - c["p"][b == m].mean()) for m in range(15) if (b == m).any())
        assert abs(fig["ece"][k] - ece) < 1e-12 and abs(fig["mce"][k] - max(gaps)) < 1e-12
        assert abs(fig["nll"][k] - c["nll"].mean()) < 1e-12 and abs(fig["brier"][k] - c["brier"].mean()) < 1e-12
        assert fig["accuracy"][k] == ((z > 0) == y).mean()
    # halves add to the whole: integers exactly
    half = [dict(case, bits=case["bits"][sl], roi=case["roi"][sl], gx=case["gx"][sl], gy=case["gy"][sl]) for sl in (slice(0, 1), slice(1, 3))]
    a, b = (_as_torch(S.reliability(h), case) for h in half)
    both = M.add_reliability(a, b)
    for key in ("count", "positives", "n", "n_nan", "n_right"):
        assert torch.equal(both[key], torch.from_numpy(o[key])), key
    assert np.allclose(both["nll"].numpy(), o["nll"], rtol=1e-12)
    with pytest.raises(ValueError, match="different edges"):
        M.add_reliability(a, dict(b, edges=b["edges"] + 1.0))
    empty = M.reliability_figures(_as_torch(S.reliability(S.bits_case(1, 5, 1, 2, 1, kind="no_roi")), S.bits_case(1, 5, 1, 2, 1, kind="no_roi")))
    assert np.isnan(empty["ece"][1:]).all() and not np.isnan(empty["ece"][0])


# ------------------------------------------------------------------------------------------------------------- refusals
def test_abi_argument_checks_return_before_any_launch(lib):
    assert lib.cp_version() >= 244
    one, N = C.c_void_p(4096), 64
    scale = (C.c_double * 13)(*([1.0] * 13))
    edges = (C.c_double * 14)(*S.logit_edges(15))
    grp = (C.c_int32 * 13)(*range(13))

    def rel(**kw):
        a = dict(bits=one, bs=13 * N, rows=13, r=6, roi=one, gx=one, gy=one, gb=6, scale=scale, edges=edges, M=15, B=2, N=N, ints=one, sums=one, scratch=one)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = lib.cp_code_reliability(None, a["bits"], a["bs"], a["rows"], a["r"], a["roi"], a["gx"], a["gy"], a["gb"], a["scale"], a["edges"], a["M"],
                                     a["B"], a["N"], a["ints"], a["sums"], a["scratch"])
        assert lib.cp_kernel_log() == b"", kw
        return rc
    for name in ("bits", "roi", "gx", "gy", "scale", "edges", "ints", "sums", "scratch"):
        assert rel(**{name: None}) == -1 and rel(B=0, **{name: None}) == -1, name
    assert rel(B=-1) == -1 and rel(N=0) == -1 and rel(r=0) == -1 and rel(r=31) == -1 and rel(rows=12) == -1 and rel(gb=5) == -1
    assert rel(bs=13 * N - 1) == -1 and rel(M=0) == -1 and rel(M=65) == -1
    for bad in (0.0, -1.0, float("nan"), INF):
        sc = (C.c_double * 13)(*([1.0] * 12 + [bad]))
        assert rel(scale=sc) == -1, bad
    for i, bad in ((3, float("nan")), (3, edges[2]), (3, edges[4]), (0, edges[1])):      # NaN, equal to the one before, beyond the next, descending
        e = (C.c_double * 14)(*edges)
        e[i] = bad
        assert rel(edges=e) == -1, (i, bad)
    assert rel(M=1, edges=None, B=0) == 0                                          # one bin needs no table
    for name in ("bits", "roi", "gx", "gy"):
        assert rel(**{name: C.c_void_p(4098)}) == -3, name
    for name in ("ints", "sums", "scratch"):
        assert rel(**{name: C.c_void_p(4100)}) == -3, name
    assert rel(B=0) == 0
    assert lib.cp_code_reliability_scratch_bytes(6, 15) == 1024 * 13 * (3 * 15 + 7) * 8
    assert lib.cp_code_reliability_scratch_bytes(0, 15) == 0 == lib.cp_code_reliability_scratch_bytes(6, 65) == lib.cp_code_reliability_scratch_bytes(31, 1)

    def fit(**kw):
        a = dict(bits=one, bs=13 * N, rows=13, r=6, roi=one, gx=one, gy=one, gb=6, grp=grp, G=13, B=2, N=N, s_min=2.0 ** -6, s_max=64.0, tol=1e-8, it=60,
                 scale=one, info=one, scratch=one)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = lib.cp_fit_code_scale(None, a["bits"], a["bs"], a["rows"], a["r"], a["roi"], a["gx"], a["gy"], a["gb"], a["grp"], a["G"], a["B"], a["N"],
                                   a["s_min"], a["s_max"], a["tol"], a["it"], a["scale"], a["info"], a["scratch"])
        assert lib.cp_kernel_log() == b"", kw
        return rc
    for name in ("bits", "roi", "gx", "gy", "grp", "scale", "info", "scratch"):
        assert fit(**{name: None}) == -1, name
    assert fit(B=-1) == -1 and fit(N=0) == -1 and fit(r=0) == -1 and fit(rows=12) == -1 and fit(gb=5) == -1 and fit(bs=1) == -1
    assert fit(G=0) == -1 and fit(G=14) == -1 and fit(G=12) == -1                   # (row 12's group index 12 is out of a 12-group range)
    assert fit(grp=(C.c_int32 * 13)(*([0] * 12 + [-1]))) == -1
    for kw in (dict(s_min=0.0), dict(s_min=-1.0), dict(s_min=2.0), dict(s_max=0.5), dict(s_max=INF), dict(s_min=1.0, s_max=1.0), dict(s_min=float("nan")),
               dict(tol=0.0), dict(tol=INF), dict(tol=float("nan")), dict(it=0), dict(it=257)):
        assert fit(**kw) == -1, kw
    for name in ("scale", "info", "scratch"):
        assert fit(**{name: C.c_void_p(4100)}) == -3, name
    assert fit(bits=C.c_void_p(4098)) == -3
    assert fit(B=0) == 0 and lib.cp_fit_code_scale_info_doubles() == 12 and lib.cp_fit_code_scale_scratch_bytes(6) == 1024 * 13 * 4 * 8
    assert lib.cp_fit_code_scale_scratch_bytes(0) == 0

    e5 = (C.c_double * 5)(0.25, 1.0, 4.0, 5.99, 9.21)

    def pit(**kw):
        a = dict(p2d=one, proj=one, s2=one, valid=one, vs=3, roi=one, edges=e5, E=5, B=2, N=N, counts=one, nn=one, sums=one)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = lib.cp_sigma2_consistency(None, a["p2d"], a["proj"], a["s2"], a["valid"], a["vs"], a["roi"], a["edges"], a["E"], a["B"], a["N"], a["counts"],
                                       a["nn"], a["sums"])
        assert lib.cp_kernel_log() == b"", kw
        return rc
    for name in ("p2d", "proj", "s2", "valid", "roi", "edges", "counts", "nn", "sums"):
        assert pit(**{name: None}) == -1, name
    assert pit(B=-1) == -1 and pit(N=0) == -1 and pit(vs=0) == -1 and pit(E=-1) == -1 and pit(E=64) == -1
    assert pit(edges=(C.c_double * 5)(0.25, 1.0, 1.0, 5.99, 9.21)) == -1 and pit(edges=(C.c_double * 5)(0.25, 1.0, float("nan"), 5.99, 9.21)) == -1
    assert pit(edges=(C.c_double * 5)(9.21, 5.99, 4.0, 1.0, 0.25)) == -1
    for name in ("proj", "s2", "sums"):
        assert pit(**{name: C.c_void_p(4100)}) == -3, name
    for name in ("p2d", "roi", "counts", "nn"):
        assert pit(**{name: C.c_void_p(4098)}) == -3, name
    assert pit(B=0) == 0 and pit(B=0, E=0, edges=None) == 0


def _host_inputs(B=2, N=8, r=6):
    bits = torch.zeros(B, 1 + 2 * r, N)
    labels = dict(roi_mask_bits=torch.ones(B, 1, N), pixel_x_codes=torch.zeros(B, r, N), pixel_y_codes=torch.zeros(B, r, N))
    return bits, labels


def test_wrapper_refusals():
    from checkerpose_amd import postprocess as PP
    bits, labels = _host_inputs()
    for fn in (PP.reliability, PP.fit_code_scale):
        for bad in (bits[:, :12], bits[:, :1], bits.double(), bits[0], torch.zeros(2, 63, 8)):
            with pytest.raises(ValueError, match="logit block"):
                fn(bad, labels)
        for key, bad in (("roi_mask_bits", labels["roi_mask_bits"][:, :, :7]), ("pixel_x_codes", labels["pixel_x_codes"][:, :5]),
                         ("pixel_y_codes", labels["pixel_y_codes"][:1])):
            with pytest.raises(ValueError, match="labels"):
                fn(bits, dict(labels, **{key: bad}))
        with pytest.raises(ValueError, match="labels"):
            fn(bits, {})
        with pytest.raises(RuntimeError, match="no CPU fallback"):               # well-formed arguments on the host: still no fallback
            fn(bits, labels)
    for bad in (np.zeros(13), -np.ones(13), np.ones(12), np.full(13, np.nan), np.full(13, INF)):
        with pytest.raises(ValueError, match="scale"):
            PP.reliability(bits, labels, scale=bad)
    for bad in (0, 65, [0.5, 0.4]):
        with pytest.raises(ValueError, match="bins"):
            PP.reliability(bits, labels, bins=bad)
    for kw, word in ((dict(groups="bit"), "groups"), (dict(groups=[0] * 12), "groups"), (dict(s_min=0.0), "bracket"), (dict(s_min=2.0), "bracket"),
                     (dict(s_max=0.5), "bracket"), (dict(s_max=INF), "bracket"), (dict(s_min=1.0, s_max=1.0), "bracket"), (dict(step_tol=0.0), "step_tol"),
                     (dict(step_tol=float("nan")), "step_tol"), (dict(max_iters=0), "max_iters"), (dict(max_iters=257), "max_iters")):
        with pytest.raises(ValueError, match=word):
            PP.fit_code_scale(bits, labels, **kw)
    B, N = 2, 8
    a = dict(p2d=torch.zeros(B, N, 2), valid=torch.ones(B, N, 3, dtype=torch.uint8), sigma2=torch.ones(B, N, 2, dtype=torch.float64),
             targets=dict(proj_xy=torch.zeros(B, N, 2, dtype=torch.float64), roi_mask_bits=torch.ones(B, 1, N)))
    for name, bad in (("p2d", a["p2d"][:, :, :1]), ("valid", a["valid"][:, :7]), ("valid", a["valid"].bool()), ("sigma2", a["sigma2"].float()),
                      ("sigma2", a["sigma2"][:1]), ("targets", {}), ("targets", dict(a["targets"], proj_xy=a["targets"]["proj_xy"].float())),
                      ("targets", dict(a["targets"], roi_mask_bits=torch.ones(B, N)))):
        with pytest.raises(ValueError, match=name):
            PP.sigma2_consistency(**dict(a, **{name: bad}))
    for column in (-1, 3):
        with pytest.raises(ValueError, match="column"):
            PP.sigma2_consistency(**dict(a, column=column))
    with pytest.raises(ValueError, match="bins"):
        PP.sigma2_consistency(**dict(a, bins=[2.0, 1.0]))
    with pytest.raises(ValueError, match="gates"):
        PP.sigma2_consistency(**dict(a, gates=(9.21, 5.99)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.sigma2_consistency(**a)
    for bad in (np.ones(12), np.zeros(13), -np.ones(13), np.full(13, np.nan), np.ones(1), np.full(13, 1e-60)):
        with pytest.raises(ValueError, match="scale"):
            PP.CalibratedNet(torch.nn.Identity(), bad)


class _StubNet(torch.nn.Module):
    """a net whose three logit outputs are slices of one block (as the module's are) or three separate tensors"""

    def __init__(self, block, sliced):
        super().__init__()
        self.block, self.sliced, self.calls = block, sliced, []

    def forward(self, x, y=None, obj_ids=None):
        self.calls.append((x, y, obj_ids))
        b = self.block
        roi, xb, yb = (b[:, :1], b[:, 1:7], b[:, 7:]) if self.sliced else (b[:, :1].clone(), b[:, 1:7].clone(), b[:, 7:].clone())
        return roi, xb, yb, torch.zeros(b.shape[0], 2, 4, 4), torch.arange(3), torch.arange(4)


@pytest.mark.parametrize("sliced", [True, False])
def test_calibrated_net_on_the_host(sliced):
    """the wrapper itself is plain torch: its contract can be checked without a device"""
    from checkerpose_amd.postprocess import CalibratedNet
    rng = np.random.default_rng(5)
    block = torch.from_numpy(rng.normal(size=(3, 13, 8)).astype(np.float32))
    scale = rng.uniform(0.3, 3.0, size=13)
    net = _StubNet(block, sliced)
    cal = CalibratedNet(net, scale)
    roi, xb, yb, seg, xid, yid = cal("crops", None, obj_ids="ids")
    assert net.calls == [("crops", None, "ids")]
    assert roi._base is xb._base is yb._base and tuple(roi._base.shape) == (3, 13, 8) and roi._base.is_contiguous()
    assert tuple(roi.shape) == (3, 1, 8) and tuple(xb.shape) == tuple(yb.shape) == (3, 6, 8)
    want = block.numpy() * scale.astype(np.float32)[None, :, None]
    assert np.array_equal(roi._base.numpy(), want)
    assert np.array_equal(np.signbit(want), np.signbit(block.numpy()))                       # no sign moves
    assert torch.equal(xid, torch.arange(3)) and torch.equal(yid, torch.arange(4)) and seg.shape == (3, 2, 4, 4)
    ones = CalibratedNet(net, np.ones(13))("crops")
    assert torch.equal(ones[0]._base, block) and ones[0]._base is not block                   # bitwise the bare net's, in a block of its own
    with pytest.raises(ValueError, match="logit rows"):
        CalibratedNet(net, np.ones(11))("crops")
    assert "scale" not in cal.state_dict()


def test_collect_logits_on_the_host():
    from checkerpose_amd.calibrate import collect_logits
    rng = np.random.default_rng(6)
    blocks = [torch.from_numpy(rng.normal(size=(b, 13, 8)).astype(np.float32)) for b in (2, 3)]
    batches = []
    for blk in blocks:
        B = blk.shape[0]
        lab = (torch.ones(B, 1, 8), torch.zeros(B, 6, 8), torch.ones(B, 6, 8))
        batches.append((blk, None, None, None, None, None, None) + lab + (None,))            # make_training_batch's 11 entries

    class Net(torch.nn.Module):
        def forward(self, x, y=None):
            return x[:, :1], x[:, 1:7], x[:, 7:], None, None, None
    bits, labels = collect_logits(Net(), batches)
    assert torch.equal(bits, torch.cat(blocks, 0)) and tuple(labels["pixel_y_codes"].shape) == (5, 6, 8) and labels["pixel_y_codes"].all()
    with pytest.raises(ValueError, match="no batches"):
        collect_logits(Net(), [])


def test_public_functions():
    """the new functions live in checkerpose_amd/calibrate.py and are re-exported: postprocess.py itself defines what it defined"""
    from checkerpose_amd import calibrate as M
    from checkerpose_amd import postprocess as PP
    names = {"reliability", "reliability_figures", "add_reliability", "fit_code_scale", "sigma2_consistency", "collect_logits", "CalibratedNet"}
    assert all(getattr(PP, n) is getattr(M, n) for n in names)
    own = {n for n, f in vars(PP).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == PP.__name__}
    assert not (names & own) and {"solve_pnp_ransac", "estimate_poses", "correspondences"} <= own
    sig = inspect.signature(M.fit_code_scale)
    assert list(sig.parameters) == ["outputs_or_bits", "labels", "groups", "s_min", "s_max", "step_tol", "max_iters"]
    assert (sig.parameters["groups"].default, sig.parameters["s_min"].default, sig.parameters["s_max"].default) == ("row", 2.0 ** -6, 2.0 ** 6)
    assert (sig.parameters["step_tol"].default, sig.parameters["max_iters"].default) == (1e-8, 60)
    sig = inspect.signature(M.sigma2_consistency)
    assert (sig.parameters["column"].default, sig.parameters["bins"].default, sig.parameters["gates"].default) == (0, 10, (5.99, 9.21))
    assert inspect.signature(M.reliability).parameters["bins"].default == 15
    assert (M.STATUS_OK, M.STATUS_CAPPED_HIGH, M.STATUS_CAPPED_LOW, M.STATUS_EMPTY, M.STATUS_NOT_CONVERGED) == (S.OK, S.CAPPED_HIGH, S.CAPPED_LOW, S.EMPTY,
                                                                                                          S.NOT_CONVERGED)
