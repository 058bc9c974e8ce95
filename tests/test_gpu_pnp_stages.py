"""GPU: cp_pnp_ransac stage by stage (tests/pnp_stages.py replays the hypothesis records the device leaves in its scratch) over the
shapes, parameters and edges the three comparisons of tests/test_pnp.py never reach: N up to 4096 with per-crop models, N not a
multiple of 64, 5 / 6 valid points, batches of 256, every round count of `iterations`, thresholds, outlier ratios at which rounds
1..3 run, validity columns 1 / 2, per-crop intrinsics, degenerate models; and the bitwise properties of the call."""
import time

import numpy as np
import pytest
import torch

from oracle import pnp_oracle as P
from tests import pnp_stages as S

pytestmark = pytest.mark.gpu


def _device_run(case, first=None, **kw):
    from checkerpose_amd.postprocess import solve_pnp_ransac
    dev = torch.device("cuda:0")
    n = case.B if first is None else first
    p3 = case.p3d[:n] if case.p3d.ndim == 3 else case.p3d
    K = case.K[:n] if case.K.ndim == 3 else case.K
    args = dict(column=case.column, reproj_threshold=case.thr, iterations=case.iterations, seed=case.seed, return_hypotheses=True)
    args.update(kw)
    out = solve_pnp_ransac(torch.from_numpy(p3).float().to(dev), torch.from_numpy(case.p2d[:n]).float().to(dev),
                           torch.from_numpy(case.valid[:n]).to(dev), torch.from_numpy(K).float().to(dev), **args)
    torch.cuda.synchronize()
    out = [o.cpu().numpy() for o in out]
    out[1] = out[1][:, :, 0]
    return out                                               # R, t, inliers, status[, records]


def _bitwise(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(S.CASES))
def test_device_stages(name):
    case = S.CASES[name]()
    t0 = time.time()
    R, t, inl, status, rec = _device_run(case)
    t1 = time.time()
    assert rec.shape == (case.B, case.iterations, 14)
    total = S.check_case(case, rec, R, t, inl, status, log=print)
    for b in case.full_oracle:                               # noise-free crops with >= 5 valid points: the full oracle, exactly
        p3, p2, va, K = case.crop(b)
        Ro, to, mo, so = P.solve_pnp_ransac(p3, p2, va, K, case.thr, case.iterations, case.seed, b)
        assert status[b] == so == 1, (name, b)
        assert np.array_equal(inl[b], mo), (name, b, int(inl[b].sum()), int(mo.sum()))
        # the pose: with equal masks the oracle's refit ran over the same list, which stage D has just compared within TAU in the
        # orientation of the control-point axes that fits; against the oracle's own orientation today's bounds for exact data hold
        dR, dt = np.abs(R[b] - Ro).max(), np.linalg.norm(t[b] - to) / np.linalg.norm(to)
        print("crop %d vs the full oracle: |dR| = %.3e, |dt|/|t| = %.3e" % (b, dR, dt))
        assert dR <= S.TAU_CAP[0] and dt <= S.TAU_CAP[1], (name, b, dR, dt)
    if case.oracle_status:                                   # degenerate inputs: the same verdict as the oracle
        for b in range(case.B):
            p3, p2, va, K = case.crop(b)
            assert status[b] == P.solve_pnp_ransac(p3, p2, va, K, case.thr, case.iterations, case.seed, b)[3], (name, b)
    print("%s: device %.3f s, checks %.3f s" % (name, t1 - t0, time.time() - t1))


def test_two_calls_agree_bitwise():
    for name in ("shape_6x512", "outliers_0.6", "shape_4x33"):
        case = S.CASES[name]()
        assert _bitwise(_device_run(case), _device_run(case)), name
        plain = _device_run(case, return_hypotheses=False)   # ... and the records are a by-product: the default path gives the same
        assert len(plain) == 4 and _bitwise(plain, _device_run(case)[:4]), name


def test_leading_crops_of_a_larger_batch():
    """the hash is keyed on the position in the batch: the first 8 crops of a 40-crop batch equal the same 8 run alone"""
    case = S._standard("batch_40", 80, 40, 512, (0.3, 0.6))
    assert _bitwise([o[:8] for o in _device_run(case)], _device_run(case, first=8))


def test_rows_outside_the_valid_column_are_never_read_into_a_result():
    case = S.CASES["column_1"]()
    base = _device_run(case)
    poisoned = S.CASES["column_1"]()
    off = poisoned.valid[:, :, 1] == 0
    assert off.sum() > 100
    junk = np.array([np.nan, np.inf, -np.inf, 1e30])
    poisoned.p2d[off] = junk[np.arange(int(off.sum()) * 2) % 4].reshape(-1, 2)
    p3 = np.repeat(poisoned.p3d[None], case.B, 0).copy()
    p3[off] = junk[(np.arange(int(off.sum()) * 3) + 1) % 4].reshape(-1, 3)
    poisoned.p3d = p3
    repeated = S.CASES["column_1"]()
    repeated.p3d = np.repeat(repeated.p3d[None], case.B, 0).copy()
    assert _bitwise(base, _device_run(repeated))             # (the same model per crop instead of shared: no change by itself)
    with np.errstate(all="ignore"):
        assert _bitwise(base, _device_run(poisoned))


def test_shared_model_and_K_equal_their_repetition():
    case = S.CASES["shape_6x512"]()
    base = _device_run(case)
    rep = S.CASES["shape_6x512"]()
    rep.p3d = np.repeat(rep.p3d[None], case.B, 0).copy()
    assert _bitwise(base, _device_run(rep))
    rep.K = np.repeat(rep.K[None], case.B, 0).copy()
    assert _bitwise(base, _device_run(rep))


def test_wrapper_refuses_bad_arguments_on_device_tensors():
    from checkerpose_amd.postprocess import solve_pnp_ransac
    dev = torch.device("cuda:0")
    p3, p2 = torch.zeros(8, 3, device=dev), torch.zeros(2, 8, 2, device=dev)
    va, K = torch.ones(2, 8, 3, dtype=torch.uint8, device=dev), torch.eye(3, device=dev)
    for bad in (dict(iterations=0), dict(iterations=257), dict(column=3), dict(column=-1)):
        with pytest.raises(ValueError):
            solve_pnp_ransac(p3, p2, va, K, **bad)
    for bad_valid in (va[:, :, :2], va[:, :7], va.float(), va[:1]):
        with pytest.raises(ValueError):
            solve_pnp_ransac(p3, p2, bad_valid, K)
    for bad_p3, bad_K in ((torch.zeros(7, 3, device=dev), K), (p3, torch.eye(4, device=dev))):
        with pytest.raises(ValueError):
            solve_pnp_ransac(bad_p3, p2, va, bad_K)
