"""GPU: row N26 on the device.  verify_poses over the committed cases of tests/verify_stages.py -- one, three, five and eight poses that
share images and meshes, shared and per-pose intrinsics, tau as a number and a tensor, three occlusion weights, an occluder slab, a far
plane, holes, NaN, inf and negative depths, poses partly and wholly off the frame, behind the camera, with status 0, an image id out of
range, exact ties at tau -- against the numpy rule applied to the device's own metric.render_depth of the same poses: counts, labels
and choice EQUAL, fit, den and score the same bits; the identities (alone / batch, labels, repeat); select_poses; the callers."""
import numpy as np
import pytest
import torch

from tests import icp_stages as I
from tests import verify_stages as VS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_MS, _RUNS = {}, {}


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _meshset(case):
    from checkerpose_amd.metric import MeshSet
    if case.meshes not in _MS:
        v, f = I.mesh_arrays(case.meshes)
        _MS[case.meshes] = MeshSet.from_arrays(v, diameters=I.diameters(case.meshes), faces=f)
    return _MS[case.meshes]


def _renders(case, idx=None):
    """the device's own depth renders of the case's poses -> (P,H,W) float32 numpy"""
    from checkerpose_amd import metric
    idx = np.arange(case.P) if idx is None else np.asarray(idx)
    D = metric.render_depth(_up(case.R[idx]), _up(case.t[idx]), _up(case.K[idx] if case.K.ndim == 3 else case.K), _meshset(case), case.size,
                            mesh_ids=None if case.mesh_ids is None else case.mesh_ids[idx])
    return D.cpu().numpy()


def _args(case, D, idx=None, **over):
    idx = np.arange(case.P) if idx is None else np.asarray(idx)
    ids = None if case.image_ids is None else case.image_ids[idx]
    if ids is not None and (ids >= case.n_img).any():
        ids = _up(ids)                                                           # (host ids are checked by the wrapper; resident ones reach the kernel)
    a = dict(R=_up(case.R[idx]), t=_up(case.t[idx]), cam_K=_up(case.K[idx] if case.K.ndim == 3 else case.K), meshes=_meshset(case),
             depth=_up(case.sensor(D)), tau=_up(np.asarray(case.tau, np.float64)[idx]) if np.ndim(case.tau) else case.tau, image_ids=ids,
             mesh_ids=None if case.mesh_ids is None else case.mesh_ids[idx], status=None if case.status is None else _up(case.status[idx]),
             occlusion_weight=case.occlusion_weight, return_labels=True)
    a.update(over)
    return a


def _device(case, D, idx=None, **over):
    """verify_poses on the device -> dict of numpy arrays in verify_stages.reference's layout (choice: select_poses over the scores)"""
    from checkerpose_amd import postprocess as Q
    a = _args(case, D, idx, **over)
    res = Q.verify_poses(**a)
    score, info = res[0], res[1]
    P = len(score)
    assert score.dtype == torch.float64 and tuple(score.shape) == (P,) and info["ok"].dtype == torch.bool
    assert all(info[k].dtype == torch.int32 and tuple(info[k].shape) == (P,) for k in VS.COUNTS) and info["fit"].dtype == info["den"].dtype == torch.float64
    out = dict(counts=np.stack([info[k].cpu().numpy() for k in VS.COUNTS], 1), score=score.cpu().numpy(), fit=info["fit"].cpu().numpy(),
               den=info["den"].cpu().numpy(), ok=info["ok"].cpu().numpy(), labels=None, choice=None)
    if a["return_labels"]:
        assert res[2].dtype == torch.uint8 and tuple(res[2].shape) == (P,) + D.shape[1:]
        out["labels"] = res[2].cpu().numpy()
    if case.cand is not None and idx is None:
        out["choice"] = Q.select_poses(score.view(*case.cand), info["ok"].view(*case.cand)).cpu().numpy()
    return out


def _run(name):
    """a committed case on the device: (case, the device's renders, its outputs); computed once, left unchanged"""
    if name not in _RUNS:
        case = VS.make(name)
        D = _renders(case)
        _RUNS[name] = (case, D, _device(case, D))
    return _RUNS[name]


def _same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True) for k in ("counts", "score", "fit", "den", "ok", "labels"))


# ------------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name", list(VS.CASES) + list(VS.SELECTION))
def test_device_equals_the_rule(name):
    """the six counts, the label map and the choice EQUAL the numpy rule's on the device's own renders; fit, den, score bit for bit"""
    case, D, out = _run(name)
    want = VS.check_case(case, D, out, log=print)
    assert out["counts"].dtype == np.int32 and out["labels"].dtype == np.uint8
    assert (want["counts"][:, 0] > 0).any()
    if name == "tie_1":                                                          # the ties are ties on the device's render too
        S, on = case.sensor(D)[0], D[0] > 0
        assert (np.abs(S - D[0])[on] == np.float32(4.0)).mean() > 0.9 and out["counts"][0, 2] == out["counts"][0, 0] > 500


def test_not_counted_rows_are_exact():
    case, D, out = _run("edges_8")
    nan_bits = np.array([np.nan]).view(np.uint64)[0]
    for b in range(1, 7):
        assert out["score"][b:b + 1].view(np.uint64)[0] == nan_bits and not out["ok"][b] and not out["counts"][b].any() and not out["labels"][b].any()
        assert out["fit"][b] == 0.0 and out["den"][b] == 0.0
    assert not D[1].any() and not D[2].any() and not D[5].any() and D[3].any() and D[4].any() and D[6].any()      # 3, 4, 6: rendered, yet not counted
    assert out["ok"][0] and out["ok"][7] and out["counts"][0, 0] > 0
    # den == 0 with counts: everything the model covers is missing
    R, t = _up(case.R[7:8]), _up(case.t[7:8])
    from checkerpose_amd import postprocess as Q
    score, info = Q.verify_poses(R, t, _up(case.K), _meshset(case), torch.zeros(80, 96, device=DEV), 8.0)
    assert np.isnan(score.cpu().numpy()).all() and not bool(info["ok"][0]) and int(info["n_model"][0]) == int(info["n_missing"][0]) == int((D[7] > 0).sum()) > 0


@pytest.mark.parametrize("name", ["mixed_3", "mixed_5", "edges_8"])
def test_bitwise_identities(name):
    """a pose alone and in its batch, with and without the labels, from call to call: the same bits"""
    case, D, out = _run(name)
    assert _same(out, _device(case, D))
    plain = _device(case, D, return_labels=False)
    assert plain["labels"] is None and _same(dict(out, labels=None), plain)
    for b in range(case.P):
        one = _device(case, D, idx=[b])
        assert _same({k: (None if v is None else v[b:b + 1]) for k, v in out.items()}, one), b
    rev = np.arange(case.P)[::-1]
    assert _same({k: (None if v is None else v[rev]) for k, v in out.items()}, _device(case, D, idx=rev))


# ------------------------------------------------------------------------------------------------------------------- the choice
def test_select_poses():
    from checkerpose_amd import postprocess as Q
    nan = float("nan")
    score = np.array([[0.5, 0.2, nan, 0.9, nan, 0.3, -np.inf],
                      [0.7, 0.2, 0.1, 0.9, nan, 0.3, np.inf],
                      [0.7, 0.1, 0.4, 0.1, nan, 0.8, 0.0]])
    ok = np.ones(score.shape, bool)
    ok[2, 5] = False
    got = Q.select_poses(_up(score), _up(ok))
    assert got.dtype == torch.int32 and got.cpu().tolist() == VS.select(score, ok).tolist() == [1, 0, 2, 0, 0, 0, 1]
    assert Q.select_poses(_up(score)).cpu().tolist() == VS.select(score, np.ones(score.shape, bool)).tolist() == [1, 0, 2, 0, 0, 2, 1]
    assert Q.select_poses(_up(score), _up(ok.astype(np.uint8))).cpu().tolist() == [1, 0, 2, 0, 0, 0, 1]
    assert Q.select_poses(_up(score[:1])).cpu().tolist() == [0] * 7
    rng = np.random.default_rng(5)
    big = np.round(rng.random((64, 1000)), 1)                                    # 64 candidates, many exact ties, more than one block
    big[rng.random(big.shape) < 0.2] = nan
    okb = rng.random(big.shape) < 0.7
    R, t = rng.normal(size=(64, 1000, 3, 3)), rng.normal(size=(64, 1000, 3, 1))
    choice, Rs, ts = Q.select_poses(_up(big), _up(okb), _up(R), _up(t))
    want = VS.select(big, okb)
    assert np.array_equal(choice.cpu().numpy(), want)
    assert np.array_equal(Rs.cpu().numpy(), R[want, np.arange(1000)]) and np.array_equal(ts.cpu().numpy(), t[want, np.arange(1000)])
    assert tuple(Q.select_poses(torch.zeros(3, 0, dtype=torch.float64, device=DEV)).shape) == (0,)
    # an exact tie made on the device: the same pose twice
    case, D, out = _run("tie_select")
    s = out["score"].reshape(case.cand)
    assert s[1, 0] == s[2, 0] > s[0, 0] and out["choice"].tolist() == [1, 0]


@pytest.mark.parametrize("name", list(VS.SELECTION))
def test_selection_cases(name):
    """start pose against tests/icp_stages.py's CPU refinement of it: the device chooses what the numpy rule chooses on a CPU"""
    case, D, out = _run(name)
    want = VS.SELECTION[name][3]
    cpu = VS.reference(case, VS.cpu_renders(case))
    assert out["choice"].tolist() == cpu["choice"].tolist() == [want] * case.cand[1]
    print(name, "device", np.round(out["score"], 4).tolist(), "cpu", np.round(cpu["score"], 4).tolist())      # (the renders differ in a few silhouette pixels)


def test_refusals_on_the_device():
    from checkerpose_amd import postprocess as Q
    case, D, _ = _run("mixed_3")
    a = _args(case, D)
    for name, bad in (("tau", torch.ones(2, dtype=torch.float64, device=DEV)), ("status", torch.ones(2, dtype=torch.int32, device=DEV)), ("tau", 0.0),
                      ("occlusion_weight", 2.0), ("image_ids", [0, 1, 5]), ("mesh_ids", [0, 1, 2])):
        with pytest.raises(ValueError, match=name):
            Q.verify_poses(**dict(a, **{name: bad}))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.verify_poses(**dict(a, depth=a["depth"].cpu()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.verify_poses(**dict(a, tau=a["tau"].cpu()))
    with pytest.raises(ValueError, match="2\\^24"):
        Q.verify_poses(a["R"][:1], a["t"][:1], I.K_A, a["meshes"], torch.zeros(4097, 4096, device=DEV), 8.0, mesh_ids=[0])


# ------------------------------------------------------------------------------------------------------------------ the callers
def test_estimate_poses_verified_is_the_composition_of_its_parts():
    from checkerpose_amd import postprocess as Q
    from checkerpose_amd.metric import MeshSet
    from checkerpose_amd.synthetic import build_net
    from tests import pnp_stages as S
    rng = np.random.default_rng(9)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 480, 640, 3), dtype=np.uint8)).cuda()
    boxes = [[100, 80, 120, 90], [300, 200, 60, 140], None, [-10, 400, 90, 90]]
    idx = [0, 1, 0, 1]
    net = build_net(npoint=512, seed=1).cuda().eval()
    net.set_compute_dtype("bf16")
    p3d = torch.from_numpy(S.lmo_model(512).astype(np.float32)).cuda()
    K = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]], dtype=np.float32)
    v, f = I.mesh_arrays(("box",))
    ms = MeshSet.from_arrays(v, faces=f)
    depth = torch.from_numpy(rng.uniform(300.0, 1500.0, (2, 480, 640)).astype(np.float32)).cuda()
    icp = dict(meshes=ms, depth=depth, max_dist=40.0, grid=16, max_iters=5)
    spec = dict(meshes=ms, depth=depth, tau=400.0, occlusion_weight=0.5)
    kw = dict(img_index=idx, seed=3)
    plain = Q.estimate_poses(net, frames, boxes, p3d, K, **kw)
    lm = Q.estimate_poses(net, frames, boxes, p3d, K, refine="lm", **kw)
    both = Q.estimate_poses(net, frames, boxes, p3d, K, refine="lm+icp", icp=icp, **kw)
    B = 4
    for refine, cands, names in ((None, [plain], ("solver",)), ("lm", [plain, lm], ("solver", "lm")), ("lm+icp", [plain, lm, both], ("solver", "lm", "icp"))):
        R, t, inl, status, final, rep = Q.estimate_poses_verified(net, frames, boxes, p3d, K, spec, return_verify=True, refine=refine,
                                                                  icp=icp if refine == "lm+icp" else None, **kw)
        C_ = len(cands)
        assert torch.equal(inl, plain[2]) and torch.equal(status, plain[3]) and np.array_equal(final, plain[4]) and rep["stages"] == names
        Rc, tc = torch.stack([c[0] for c in cands]), torch.stack([c[1] for c in cands])
        score, info = Q.verify_poses(Rc.reshape(C_ * B, 3, 3), tc.reshape(C_ * B, 3, 1), K, ms, depth, 400.0, image_ids=idx * C_,
                                     status=plain[3].repeat(C_), occlusion_weight=0.5)
        choice, R2, t2 = Q.select_poses(score.view(C_, B), info["ok"].view(C_, B), Rc, tc)
        assert np.array_equal(rep["score"].cpu().numpy(), score.view(C_, B).cpu().numpy(), equal_nan=True) and torch.equal(rep["choice"], choice)
        assert all(torch.equal(rep["info"][k], info[k]) for k in VS.COUNTS + ("ok",))
        assert torch.equal(R, R2) and torch.equal(t, t2) and tuple(R.shape) == (B, 3, 3) and tuple(t.shape) == (B, 3, 1)
        pick = choice.cpu().tolist()
        assert all(torch.equal(R[b], cands[pick[b]][0][b]) and torch.equal(t[b], cands[pick[b]][1][b]) for b in range(B))       # the chosen candidate's bits
        assert all(pick[b] == 0 for b in range(B) if int(plain[3][b]) == 0)                                                  # the fallback never loses its place
        five = Q.estimate_poses_verified(net, frames, boxes, p3d, K, spec, refine=refine, icp=icp if refine == "lm+icp" else None, **kw)
        assert len(five) == 5 and torch.equal(five[0], R) and torch.equal(five[1], t)
    none = Q.evaluate_poses(net, frames, boxes, p3d, K, R2, t2, p3d.cpu().numpy(), kinds=("add",), refine="lm+icp", icp=icp, **kw)
    assert all(torch.equal(x, y) for x, y in zip(both[:4], none[1:5]))                                                       # without verify: unchanged
    E = Q.evaluate_poses(net, frames, boxes, p3d, K, R2, t2, p3d.cpu().numpy(), kinds=("add",), refine="lm+icp", icp=icp, verify=spec, **kw)
    assert torch.equal(E[1], R2) and float(E[0]["add"].abs().max()) == 0.0
