"""Row N8 on the device: cp_vsd_errors / cp_vsd_from_depth / cp_render_depth against tests/golden/vsd.npz and the stages of
tests/vsd_stages.py (bounds: its module docstring; fixture and oracle: tests/test_vsd_error.py).

  counting     cp_vsd_from_depth on the recorded renders gives the reference's counts EXACTLY, the errors as their float64 quotients;
  rasteriser   render_depth passes the oracle's interval check on every case (decided pixels within tol_d, the others inside
               [d_lo - tol_d, d_hi + tol_d]);
  end to end   vsd_errors' counts EQUAL the numpy counting applied to the depth images it returns, and lie within the interval the
               undecided pixels of both renders allow;
  bitwise      two calls, a case alone against in its batch, with / without the depth output, the bop_toolkit-named twin, NaN / inf
               in images no pose refers to, a 640 x 480 batch.
The sphere shortcut is taken ON the device (no host synchronisation), so the launch list of a call is fixed: what is asserted is
that a pose it skips is not rendered (its returned depth images are zero), scores 1.0 with zero counts, and that the call's
launches are the four of every call.
Measured on one MI355X: worst depth |diff| / tol_d over the 48 renders 0.032, no pixel outside its interval; the device's counts equal
the reference's recorded ones in all 24 cases."""
import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, metric
from tests import vsd_stages as S
from tests.test_vsd_error import fixture, mesh_set, n_cases, oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_SHARED = {}


def _dev(a, shape):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))).to(DEV)


def _groups():
    """fixture cases that can share one call: same image size, delta and normalisation"""
    g, _ = fixture()
    out = {}
    for c in range(n_cases()):
        out.setdefault((int(g["W"][c]), int(g["H"][c]), float(g["delta"][c]), bool(g["norm"][c])), []).append(c)
    return out


def _poses(idx):
    g, _ = fixture()
    n = len(idx)
    return (_dev(g["R_est"][idx], (n, 3, 3)), _dev(g["t_est"][idx], (n, 3, 1)), _dev(g["R_gt"][idx], (n, 3, 3)), _dev(g["t_gt"][idx], (n, 3, 1)),
            _dev(g["K"][idx], (n, 3, 3)))


def _images(idx, name):
    g, _ = fixture()
    return torch.from_numpy(np.stack([g["%s_%d" % (name, c)] for c in idx])).to(DEV)


def _run(key, **kw):
    """group `key` through vsd_errors (sphere_check off, counts and depth back), once, shared"""
    if key not in _SHARED:
        g, _ = fixture()
        idx = _groups()[key]
        out = metric.vsd_errors(*_poses(idx), mesh_set(), _images(idx, "test"), delta=key[2], normalized_by_diameter=key[3],
                                mesh_ids=g["mesh"][idx], sphere_check=False, return_counts=True, return_depth=True)
        assert out["vsd"].dtype == torch.float64 and tuple(out["vsd"].shape) == (len(idx), 10) and out["counts"].dtype == torch.int32
        assert tuple(out["depth"].shape) == (len(idx), 2, key[1], key[0]) and out["depth"].dtype == torch.float32
        _SHARED[key] = (idx, {k: v.cpu().numpy() for k, v in out.items()})
    return _SHARED[key]


def test_counting_on_the_recorded_renders_equals_the_reference():
    g, _ = fixture()
    for key, idx in _groups().items():
        diam = g["mesh_diameter"][g["mesh"][idx]]
        out = metric.vsd_from_depth(_images(idx, "est"), _images(idx, "gt"), _images(idx, "test"), _dev(g["K"][idx], (len(idx), 3, 3)), diam,
                                    delta=key[2], normalized_by_diameter=key[3])
        counts, err = out["counts"].cpu().numpy(), out["vsd"].cpu().numpy()
        for j, c in enumerate(idx):
            print("case %2d counts %s" % (c, counts[j].tolist()))
            assert np.array_equal(counts[j], g["counts"][c]), (c, counts[j], g["counts"][c])
            assert np.array_equal(err[j], g["errors"][c]) and np.array_equal(err[j], S.errors_of(counts[j])), c
    one = metric.vsd_from_depth(_images([4], "est"), _images([4], "gt"), g["test_4"], g["K"][4], float(g["mesh_diameter"][g["mesh"][4]]))
    assert np.array_equal(one["counts"].cpu().numpy()[0], g["counts"][4])              # one (H,W) image, one K, a float diameter


def test_render_depth_passes_the_interval_check_on_every_case():
    g, _ = fixture()
    worst = 0.0
    for key, idx in _groups().items():
        R_est, t_est, R_gt, t_gt, K = _poses(idx)
        ids = np.concatenate([g["mesh"][idx], g["mesh"][idx]])
        d = metric.render_depth(torch.cat([R_est, R_gt]), torch.cat([t_est, t_gt]), torch.cat([K, K]), mesh_set(), (key[0], key[1]), mesh_ids=ids)
        assert tuple(d.shape) == (2 * len(idx), key[1], key[0]) and d.dtype == torch.float32
        d = d.cpu().numpy()
        for j, c in enumerate(idx):
            for s, side in enumerate(("est", "gt")):
                ok, ratio, nbad = S.check_render(d[s * len(idx) + j], oracle(c, side))
                worst = max(worst, ratio)
                print("case %2d %-3s worst |diff| / tol_d on decided pixels %.4f, pixels outside their interval %d" % (c, side, ratio, nbad))
                assert ok, (c, side, ratio, nbad)
    print("render_depth: worst |diff| / tol_d %.4f" % worst)


def test_vsd_errors_end_to_end():
    g, _ = fixture()
    for key in _groups():
        idx, out = _run(key)
        for j, c in enumerate(idx):
            diam = float(g["mesh_diameter"][g["mesh"][c]])
            for s, side in enumerate(("est", "gt")):
                assert S.check_render(out["depth"][j, s], oracle(c, side))[0], (c, side)
            counts, err = S.score(g["test_%d" % c], out["depth"][j, 0], out["depth"][j, 1], g["K"][c], key[2], g["taus"], key[3], diam)
            low, high = S.count_interval(g["test_%d" % c], oracle(c, "est"), oracle(c, "gt"), g["K"][c], key[2], g["taus"], key[3], diam)
            print("case %2d device %s recorded %s slack %d" % (c, out["counts"][j].tolist(), g["counts"][c].tolist(), int(high[0] - low[0])))
            assert np.array_equal(out["counts"][j], counts), (c, out["counts"][j], counts)
            assert np.array_equal(out["vsd"][j], err) and np.array_equal(out["vsd"][j], S.errors_of(out["counts"][j])), c
            assert (out["counts"][j] >= low).all() and (out["counts"][j] <= high).all(), (c, out["counts"][j], low, high)
            assert (g["counts"][c] >= low).all() and (g["counts"][c] <= high).all(), c    # the reference's own counts lie in it too
            if g["counts"][c, 0] == 0:
                assert (out["vsd"][j] == 1.0).all() and out["counts"][j, 0] == 0


def test_bitwise_two_calls_alone_without_depth_twin_and_unreferenced_images():
    g, _ = fixture()
    ms = mesh_set()
    key = (67, 45, 15.0, True)
    idx, out = _run(key)
    args = _poses(idx)
    test = _images(idx, "test")
    kw = dict(delta=15.0, normalized_by_diameter=True, mesh_ids=g["mesh"][idx], sphere_check=False, return_counts=True)
    again = metric.vsd_errors(*args, ms, test, **kw)                                    # a second call, no depth output
    assert sorted(again) == ["counts", "vsd"]
    assert np.array_equal(again["counts"].cpu().numpy(), out["counts"]) and np.array_equal(again["vsd"].cpu().numpy(), out["vsd"])
    # images no pose refers to may hold anything; ids through image_ids in another order
    junk = torch.full((1,) + tuple(test.shape[1:]), float("nan"), device=DEV)
    junk[0, ::2] = float("inf")
    stack = torch.cat([junk, test.flip(0), junk])
    ids = torch.arange(len(idx), 0, -1, dtype=torch.int32, device=DEV)
    moved = metric.vsd_errors(*args, ms, stack, image_ids=ids, **kw)
    assert np.array_equal(moved["counts"].cpu().numpy(), out["counts"]) and np.array_equal(moved["vsd"].cpu().numpy(), out["vsd"])
    for j in (1, 3, len(idx) - 1):                                                      # a case alone, and bop_toolkit's twin
        c = idx[j]
        one = metric.vsd_errors(*(a[j:j + 1] for a in args), ms, test[j], delta=15.0, mesh_ids=[int(g["mesh"][c])], sphere_check=False,
                                return_counts=True, return_depth=True)
        assert np.array_equal(one["counts"].cpu().numpy()[0], out["counts"][j]) and np.array_equal(one["vsd"].cpu().numpy()[0], out["vsd"][j])
        assert np.array_equal(one["depth"].cpu().numpy()[0], out["depth"][j])
        twin = metric.vsd(g["R_est"][c], g["t_est"][c], g["R_gt"][c], g["t_gt"][c].reshape(3, 1), g["test_%d" % c], g["K"][c], 15, list(g["taus"]),
                          True, float(g["mesh_diameter"][g["mesh"][c]]), ms, int(g["mesh"][c]), "step", device=DEV)
        assert isinstance(twin, list) and twin == out["vsd"][j].tolist()
    with pytest.raises(ValueError, match="no faces"):
        metric.vsd_errors(*(a[:1] for a in args), metric.MeshSet.from_arrays([np.ones((4, 3), np.float32)], diameters=[1.0]), test[0])


def test_full_frame_batch_against_the_numpy_counting():
    g, meshes = fixture()
    ms = mesh_set()
    rng = np.random.default_rng(11)
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    c = 11                                                                              # the 20 480-triangle sphere; and the torus
    R = np.stack([g["R_gt"][c], g["R_gt"][13]])
    t_gt = np.array([[20.0, -30.0, 420.0], [-60.0, 40.0, 380.0]])
    t_est = t_gt + np.array([[2.0, 1.0, 4.0], [-6.0, 3.0, 9.0]])
    ids = [int(g["mesh"][c]), int(g["mesh"][13])]
    test = (400.0 + 60.0 * rng.random((2, 480, 640))).astype(np.float32)
    test[rng.random(test.shape) < 0.1] = 0.0
    f = lambda a, s: _dev(a, s)                                                         # noqa: E731
    lib = _abi.load()
    lib.cp_kernel_log_begin()
    out = metric.vsd_errors(f(R, (2, 3, 3)), f(t_est, (2, 3, 1)), f(R, (2, 3, 3)), f(t_gt, (2, 3, 1)), K, ms, test, mesh_ids=ids,
                            return_counts=True, return_depth=True)
    assert lib.cp_kernel_log().decode() == "vsd_pose_kernel + vsd_vertex_kernel + vsd_tile_kernel + vsd_sum_kernel"
    depth, counts, err = (out[k].cpu().numpy() for k in ("depth", "counts", "vsd"))
    for b in range(2):
        want, e = S.score(test[b], depth[b, 0], depth[b, 1], K, 15.0, g["taus"], True, float(g["mesh_diameter"][ids[b]]))
        print("640 x 480 pose %d counts %s" % (b, counts[b].tolist()))
        assert np.array_equal(counts[b], want) and np.array_equal(err[b], e) and counts[b, 1] > 1000
    plain = metric.vsd_errors(f(R, (2, 3, 3)), f(t_est, (2, 3, 1)), f(R, (2, 3, 3)), f(t_gt, (2, 3, 1)), K, ms, test, mesh_ids=ids)
    assert sorted(plain) == ["vsd"] and np.array_equal(plain["vsd"].cpu().numpy(), err)


def test_sphere_shortcut_and_poses_that_are_not_rendered():
    g, _ = fixture()
    ms = mesh_set()
    idx = [c for c in _groups()[(67, 45, 15.0, True)] if not g["sphere"][c]] + [2, 3]
    assert len(idx) >= 4 and g["sphere"][2] and g["sphere"][3]
    lib = _abi.load()
    lib.cp_kernel_log_begin()
    out = metric.vsd_errors(*_poses(idx), ms, _images(idx, "test"), mesh_ids=g["mesh"][idx], return_counts=True, return_depth=True)
    assert lib.cp_kernel_log().decode() == "vsd_pose_kernel + vsd_vertex_kernel + vsd_tile_kernel + vsd_sum_kernel"
    err, counts, depth = (out[k].cpu().numpy() for k in ("vsd", "counts", "depth"))
    _, ref = _run((67, 45, 15.0, True))
    pos = {c: j for j, c in enumerate(_groups()[(67, 45, 15.0, True)])}
    for j, c in enumerate(idx):
        if g["sphere"][c]:                                                              # overlapping: exactly what the call without the check gives
            assert np.array_equal(counts[j], ref["counts"][pos[c]]) and np.array_equal(err[j], ref["vsd"][pos[c]])
        else:                                                                           # [1.0] * len(taus), and nothing was rendered
            assert (err[j] == 1.0).all() and (counts[j] == 0).all() and (depth[j] == 0).all(), c
            assert (ref["depth"][pos[c]] > 0).any()
    # a vertex at Z <= 0 in either pose: NaN, a miss; a non-finite pose likewise; the pose next to them is untouched
    R_est, t_est, R_gt, t_gt, K = _poses([2, 2, 2, 2])
    t_est = t_est.clone()
    t_gt = t_gt.clone()
    t_est[0, 2, 0] = 10.0                                                               # the box straddles the camera plane
    t_gt[1, 2, 0] = -400.0
    t_est[2, 0, 0] = float("nan")
    out = metric.vsd_errors(R_est, t_est, R_gt, t_gt, K, ms, g["test_2"], mesh_ids=[1, 1, 1, 1], sphere_check=False, return_counts=True,
                            return_depth=True)
    err, counts, depth = (out[k].cpu().numpy() for k in ("vsd", "counts", "depth"))
    assert np.isnan(err[:3]).all() and (counts[:3] == 0).all() and (depth[:3] == 0).all()
    assert np.array_equal(err[3], ref["vsd"][pos[2]]) and np.array_equal(counts[3], ref["counts"][pos[2]])
    assert not metric.bop_recall(err, "vsd")["correct"][:3].any()
    d = metric.render_depth(R_est[:1], t_est[:1], K[:1], ms, (67, 45), mesh_ids=[1])
    assert (d == 0).all()


def test_evaluate_poses_with_vsd_and_unchanged_defaults():
    from checkerpose_amd import postprocess as Q
    from tests.common import build_net
    g, meshes = fixture()
    rng = np.random.default_rng(9)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 480, 640, 3), dtype=np.uint8)).to(DEV)
    boxes = [[100, 80, 120, 90], [300, 200, 60, 140], None, [-10, 400, 90, 90]]
    net = build_net(npoint=512, seed=1).to(DEV).eval()
    net.set_compute_dtype("bf16")
    v, f = meshes["hull"]
    ms = metric.MeshSet.from_arrays([v], diameters=[float(g["mesh_diameter"][7])], faces=[f])
    p3d = torch.from_numpy(v[:512]).to(DEV)
    K = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]], dtype=np.float32)
    R_gt = np.stack([np.eye(3)] * 4)
    t_gt = np.array([[10.0, -20.0, 800.0 + 100 * b] for b in range(4)])
    depth = (700.0 + 300.0 * rng.random((2, 480, 640))).astype(np.float32)
    err, R, t, inl, status, final = Q.evaluate_poses(net, frames, boxes, p3d, K, R_gt, t_gt, ms, kinds=("mssd", "mspd", "vsd"),
                                                     depth_test=depth, image_ids=[0, 1, 0, 1], img_index=[0, 1, 0, 1])
    assert sorted(err) == ["mspd", "mssd", "vsd"] and tuple(err["vsd"].shape) == (4, 10)
    direct = metric.vsd_errors(R, t, R_gt, t_gt, K, ms, depth, image_ids=[0, 1, 0, 1])
    bop = metric.bop_errors(R, t, R_gt, t_gt, K, ms, kinds=("mssd", "mspd"))
    assert torch.equal(torch.nan_to_num(err["vsd"], nan=-1.0), torch.nan_to_num(direct["vsd"], nan=-1.0))
    assert torch.equal(err["mssd"], bop["mssd"]) and torch.equal(err["mspd"], bop["mspd"])
    s = metric.summarize_bop(err, diameters=ms.diameters[0], im_width=640)
    assert "AR" in s and 0.0 <= s["AR"] <= 1.0
    print("evaluate_poses vsd", err["vsd"].cpu().numpy()[:, ::3].tolist(), "status", status.tolist(), "AR", s["AR"])
    lib = _abi.load()
    lib.cp_kernel_log_begin()
    plain = metric.score_poses(R, t, R_gt, t_gt, K, ms)                                 # without "vsd": the launch list it had before
    assert lib.cp_kernel_log().decode() == "adi_min_kernel + pose_error_finish_kernel" and sorted(plain) == ["add", "adi"]
    lib.cp_kernel_log_begin()
    metric.score_poses(R, t, R_gt, t_gt, K, ms, kinds=("add", "vsd"), depth_test=depth, image_ids=[0, 1, 0, 1])
    assert lib.cp_kernel_log().decode() == "pose_error_finish_kernel + vsd_pose_kernel + vsd_vertex_kernel + vsd_tile_kernel + vsd_sum_kernel"
