"""GPU: row N24 on the device.  surface_samples against metric.render_depth and the float64 geometry; refine_poses_icp replayed one
iteration at a time from its own records (tests/icp_stages.py) over the committed cases -- grids of 64, 289, 1024 and 4096 slots,
batches that share images and meshes, shared and per-pose intrinsics, iteration bounds, a depth image with an occluder, a far plane,
holes and NaN --; the exact properties; the converging cases' ADD; the bitwise pass-throughs and identities; the callers."""
import numpy as np
import pytest
import torch

from tests import icp_stages as I

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_MS, _RUNS = {}, {}
KEYS = ("rect", "shape", "pixel", "depth", "face", "X", "N", "ok")


def _meshset(case):
    from checkerpose_amd.metric import MeshSet
    if case.meshes not in _MS:
        v, f = I.mesh_arrays(case.meshes)
        _MS[case.meshes] = MeshSet.from_arrays(v, diameters=I.diameters(case.meshes), faces=f)
    return _MS[case.meshes]


def _args(case, idx=None, **over):
    idx = np.arange(case.P) if idx is None else np.asarray(idx)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)             # noqa: E731
    a = dict(R=up(case.R0[idx]), t=up(case.t0[idx]), cam_K=up(case.K[idx] if case.K.ndim == 3 else case.K), meshes=_meshset(case),
             depth=up(case.depth), max_dist=up(np.asarray(case.max_dist)[idx]) if np.ndim(case.max_dist) else case.max_dist,
             image_ids=None if case.image_ids is None else case.image_ids[idx], mesh_ids=None if case.mesh_ids is None else case.mesh_ids[idx],
             status=None if case.status_in is None else up(case.status_in[idx]), grid=case.grid, max_iters=case.max_iters, step_tol=case.step_tol,
             min_pairs=case.min_pairs, inertia=case.inertia, return_records=True)
    a.update(over)
    return a


def _samples(case, idx=None):
    from checkerpose_amd.postprocess import surface_samples
    a = _args(case, idx)
    return surface_samples(a["R"], a["t"], a["cam_K"], a["meshes"], case.size, mesh_ids=a["mesh_ids"], grid=case.grid)


def _flat(R, t, status, info, rec):
    flat = torch.cat([info["cost0"][:, None], info["cost"][:, None], info["n_samples"][:, None].double(), info["n0"][:, None].double(),
                      info["n"][:, None].double(), info["iters"][:, None].double(), info["H"].reshape(-1, 36)], 1)
    assert tuple(R.shape) == (len(status), 3, 3) and tuple(t.shape) == (len(status), 3, 1) and status.dtype == torch.int32
    assert info["status"] is status and R.dtype == t.dtype == torch.float64
    return [rec.cpu().numpy(), R.cpu().numpy(), t.cpu().numpy()[:, :, 0], status.cpu().numpy(), flat.cpu().numpy()]


def _device_run(case, idx=None, **over):
    from checkerpose_amd.postprocess import refine_poses_icp
    out = _flat(*refine_poses_icp(**_args(case, idx, **over)))
    torch.cuda.synchronize()
    return out


def _run(name):
    """a committed case on the device: (case, samples as numpy, per-pose sample dicts, outputs); computed once, left unchanged"""
    if name not in _RUNS:
        case = I.make(name)
        smp = {k: v.cpu().numpy() for k, v in _samples(case).items()}
        _RUNS[name] = (case, smp, [{k: smp[k][b] for k in KEYS} for b in range(case.P)], _device_run(case))
    return _RUNS[name]


def _bitwise(a, b, n=None):
    return all(np.array_equal(x[:n], y[:n], equal_nan=True) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------- stage A
@pytest.mark.parametrize("name", ["torus_3_g17", "ico80_1_g64", "mixed_5_g17", "mixed_5_g64", "torus_off_frame", "narrow_triangle", "halfbox_3_g32",
                                  "torus_1_g8", "passthrough"])
def test_surface_samples(name):
    from checkerpose_amd import metric
    case, smp, per, _ = _run(name)
    a = _args(case)
    W, H = case.size
    S = case.grid ** 2
    assert smp["pixel"].shape == (case.P, S, 2) and smp["X"].shape == (case.P, S, 3) and smp["face"].shape == (case.P, S) and smp["rect"].shape == (case.P, 4)
    ren = metric.render_depth(a["R"], a["t"], a["cam_K"], a["meshes"], case.size, mesh_ids=a["mesh_ids"]).cpu().numpy()
    for b in range(case.P):
        s, K, R, t = per[b], case.K_of(b), case.R0[b], case.t0[b]
        v, f = case.geometry(b)
        finite = np.isfinite(R).all() and np.isfinite(t).all()
        assert s["ok"] == int(finite)
        if not finite:
            assert (s["face"] == -1).all() and (s["rect"] == -1).all() and (s["shape"] == 0).all() and (s["pixel"] == -1).all() and not ren[b].any()
            continue
        x0, y0, x1, y1 = s["rect"]
        nx, ny = s["shape"]
        assert nx == min(case.grid, x1 - x0 + 1) and ny == min(case.grid, y1 - y0 + 1)
        # the lattice rule, the render's bits at the lattice pixels, the slots beyond nx * ny
        want = I.lattice_pixels(I.lattice((x0, y0, x1, y1), case.size, case.grid), case.grid)
        assert np.array_equal(s["pixel"], want)
        used = nx * ny
        px, py = s["pixel"][:used, 0], s["pixel"][:used, 1]
        assert np.array_equal(s["depth"][:used].view(np.uint32), ren[b][py, px].view(np.uint32))
        assert np.array_equal(s["face"][:used] >= 0, s["depth"][:used] > 0) and (s["face"][used:] == -1).all() and not s["depth"][used:].any()
        # the rectangle: contains every covered pixel, lies within the float64 bounding box of the projected vertices grown by one pixel
        ys, xs = np.nonzero(ren[b] > 0)
        assert xs.min() >= x0 and xs.max() <= x1 and ys.min() >= y0 and ys.max() <= y1
        u, w_, Z, _ = I.V.screen(R, t, K, v)
        assert x0 >= max(0, np.floor(u.min() - 0.5) - 1) and x1 <= min(W - 1, np.ceil(u.max() - 0.5) + 1)
        assert y0 >= max(0, np.floor(w_.min() - 0.5) - 1) and y1 <= min(H - 1, np.ceil(w_.max() - 0.5) + 1)
        k = s["face"] >= 0
        assert k.sum() >= 4
        # X reprojects to the pixel centre and to the depth
        C = s["X"][k] @ R.T + t
        uu, vv = K[0, 0] * C[:, 0] / C[:, 2] + K[0, 2], K[1, 1] * C[:, 1] / C[:, 2] + K[1, 2]
        assert np.abs(uu - (s["pixel"][k, 0] + 0.5)).max() <= 1e-9 and np.abs(vv - (s["pixel"][k, 1] + 0.5)).max() <= 1e-9
        assert (np.abs(C[:, 2] - s["depth"][k].astype(np.float64)) <= 1e-9 * C[:, 2]).all()
        # N: unit, orthogonal to two edges of its face, towards the camera
        N = s["N"][k]
        tri = v.astype(np.float64)[f[s["face"][k]]]
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        assert np.abs(np.linalg.norm(N, axis=1) - 1.0).max() <= 1e-12
        assert np.abs((N * e1).sum(1) / np.linalg.norm(e1, axis=1)).max() <= 1e-9 and np.abs((N * e2).sum(1) / np.linalg.norm(e2, axis=1)).max() <= 1e-9
        assert (((N @ R.T) * C).sum(1) < 0).all()
        # and both against the restatement from the device's own (pixel, depth, face)
        I.check_samples(s, K, R, t, v, f, b)


def test_a_vertex_behind_the_camera_is_not_sampled():
    from checkerpose_amd.postprocess import refine_poses_icp, surface_samples
    case = I.make("torus_3_g17")
    a = _args(case)
    t = a["t"].clone()
    t[1, 2] = 30.0                                                              # the torus reaches 55 from its centre: vertices at Z <= 0
    s = surface_samples(a["R"], t, a["cam_K"], a["meshes"], case.size, grid=case.grid)
    assert s["ok"].tolist() == [1, 0, 1] and (s["face"][1] == -1).all() and (s["rect"][1] == -1).all() and (s["face"][0] >= 0).any()
    R2, t2, st, info = refine_poses_icp(**dict(a, t=t, return_records=False))
    assert st[1] == 0 and torch.equal(t2[1, :, 0], t[1]) and torch.equal(R2[1], a["R"][1]) and info["n_samples"].tolist()[1] == 0 and st[0] != 0


# ------------------------------------------------------------------------------------------------------------ stages B and C
@pytest.mark.parametrize("name", list(I.CASES))
def test_device_stages(name):
    from checkerpose_amd import metric
    case, smp, per, out = _run(name)
    rec, R, t, status, info = out
    assert rec.shape == (case.P, case.max_iters, I.REC)
    I.check_case(case, per, rec, R, t, status, info, log=print)
    refined = status != 0
    # the exact properties
    assert (info[refined, 1] <= info[refined, 0]).all()
    assert (np.abs(np.einsum("bji,bjk->bik", R[refined], R[refined]) - np.eye(3)) <= 1e-12).all()
    if case.max_iters < 20:
        assert (status[refined] == 2).all() and (info[refined, 5] == case.max_iters).all()
    if name == "passthrough":
        assert status.tolist()[1:] == [0] * 4 and status[0] != 0
    if name in I.CONVERGING:
        # the feature's point, end to end: the device's final ADD is below a quarter of its starting ADD (it follows from the replay)
        a = _args(case)
        idx = np.nonzero(refined)[0]
        Rt = np.stack([case.truth_of(b)[1] for b in idx])
        tt = np.stack([case.truth_of(b)[2] for b in idx])
        ids = None if case.mesh_ids is None else case.mesh_ids[idx]
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)        # noqa: E731
        e0 = metric.pose_errors(a["R"][idx], a["t"][idx], Rt, tt, a["meshes"], mesh_ids=ids, kinds=("add",))["add"].cpu().numpy()
        e1 = metric.pose_errors(up(R[idx]), up(t[idx]), Rt, tt, a["meshes"], mesh_ids=ids, kinds=("add",))["add"].cpu().numpy()
        assert len(idx) and (e1 < 0.25 * e0).all() and np.isin(status[idx], (1, 2)).all(), (e0, e1, status)


def test_pass_throughs_are_bitwise():
    case, smp, per, out = _run("passthrough")
    rec, R, t, status, info = out
    for b in np.nonzero(status == 0)[0]:
        assert np.array_equal(R[b].view(np.uint64), case.R0[b].view(np.uint64)), b                     # NaN payloads included
        assert np.array_equal(t[b].view(np.uint64), case.t0[b].view(np.uint64)), b
        assert np.isnan(rec[b]).all() and np.isnan(info[b, :2]).all() and np.isnan(info[b, 6:]).all() and info[b, 5] == 0
    assert info[1, 2] > 0 and info[1, 3] == 0 and info[2, 2] == 0 and info[4, 2] > 0 and info[4, 3] < case.min_pairs
    case = I.make("torus_3_g17")
    a = _args(case)

    def passes(o, n_samples_positive=True):
        rec, R, t, status, info = o
        assert status.tolist() == [0] * case.P
        assert np.array_equal(R.view(np.uint64), case.R0.view(np.uint64)) and np.array_equal(t.view(np.uint64), case.t0.view(np.uint64))
        assert np.isnan(rec).all() and np.isnan(info[:, :2]).all() and np.isnan(info[:, 6:]).all() and (info[:, 3:6] == 0).all()
        assert ((info[:, 2] > 0) == n_samples_positive).all()

    passes(_device_run(case, depth=torch.zeros_like(a["depth"])))                                    # depth all 0
    passes(_device_run(case, max_dist=1e-7))                                                         # no pair survives
    off = a["t"].clone()
    off[:, 0] += 2000.0                                                                              # the mesh off the frame
    o = _device_run(case, t=off)
    assert o[3].tolist() == [0] * 3 and np.array_equal(o[2], off.cpu().numpy()) and (o[4][:, 2] == 0).all() and np.isnan(o[0]).all()
    s = _samples(case)
    from checkerpose_amd.postprocess import surface_samples
    s_off = surface_samples(a["R"], off, a["cam_K"], a["meshes"], case.size, grid=case.grid)
    assert s_off["ok"].tolist() == [1, 1, 1] and (s_off["rect"] == -1).all() and (s_off["face"] == -1).all() and (s["face"] >= 0).any()


def test_bitwise_identities():
    from checkerpose_amd import _abi
    from checkerpose_amd.postprocess import refine_poses_icp
    case, smp, per, a = _run("mixed_5_g17")
    assert _bitwise(a, _device_run(case))                                        # two calls
    assert _bitwise(a, _device_run(case, idx=[0]), 1)                            # pose 0 alone == pose 0 inside its batch
    s = _samples(case)
    assert _bitwise(a, _device_run(case, samples=s))                             # samples= == the internal render
    assert _bitwise(a, _device_run(case, samples=s, grid=3))                     # (grid is then the samples')
    perm = np.array([3, 0, 4, 2, 1])
    p = _device_run(case, idx=perm)
    assert _bitwise([x[perm] for x in a], p)                                     # a permuted batch == the permuted result
    one = I.make("torus_1_g8")
    b = _device_run(one)
    assert _bitwise(b, _device_run(one, depth=torch.from_numpy(one.depth[0]).to(DEV)))               # depth (H,W) == (1,H,W)
    # the `out` buffers are not read: the same call through the C ABI into buffers filled with 0, NaN and 1e300
    g = _args(case)
    P, S = case.P, case.grid ** 2
    ms = g["meshes"]
    pin = torch.cat([g["R"].reshape(P, 9), g["t"].reshape(P, 3)], 1).contiguous()
    diam = ms.faces_on(DEV)[2]
    img = torch.from_numpy(case.image_ids).to(DEV)
    mid = torch.from_numpy(case.mesh_ids).to(DEV)
    for fill in (0.0, float("nan"), 1e300):
        pose = torch.full((P, 12), fill, dtype=torch.float64, device=DEV)
        info = torch.full((P, I.INFO), fill, dtype=torch.float64, device=DEV)
        st = torch.full((P,), 77, dtype=torch.int32, device=DEV)
        rec = torch.full((P, case.max_iters, I.REC), float("nan"), dtype=torch.float64, device=DEV)
        _abi.call("cp_icp_refine", DEV, pin, g["cam_K"].reshape(9).contiguous(), 0, s["X"], s["N"], s["face"], S, g["depth"], img, case.depth.shape[0],
                  case.size[1], case.size[0], g["max_dist"], diam, len(ms), mid, None, case.max_iters, case.step_tol, case.min_pairs, case.inertia, P,
                  pose, st, info, rec)
        torch.cuda.synchronize()
        o = [rec.cpu().numpy(), pose[:, :9].reshape(P, 3, 3).cpu().numpy(), pose[:, 9:].cpu().numpy(), st.cpu().numpy(), info.cpu().numpy()]
        assert _bitwise(a, o), fill
    # surface_samples too: two calls, pose 0 alone, a permuted batch
    s2, s0, sp = _samples(case), _samples(case, [0]), _samples(case, perm)
    for k in KEYS:
        x = s[k].cpu().numpy()
        assert np.array_equal(x, s2[k].cpu().numpy(), equal_nan=True) and np.array_equal(x[:1], s0[k].cpu().numpy(), equal_nan=True), k
        assert np.array_equal(x[perm], sp[k].cpu().numpy(), equal_nan=True), k
    R2, t2, st2, info2 = refine_poses_icp(**dict(g, return_records=False))      # without records: the same poses
    assert np.array_equal(R2.cpu().numpy(), a[1]) and np.array_equal(st2.cpu().numpy(), a[3])


def test_refusals_on_the_device():
    from checkerpose_amd.postprocess import refine_poses_icp
    case = I.make("torus_3_g17")
    a = dict(_args(case), return_records=False)
    for name, bad in (("max_iters", 0), ("step_tol", float("nan")), ("min_pairs", 3), ("inertia", -1.0), ("grid", 65), ("max_dist", 0.0),
                      ("max_dist", torch.ones(2, dtype=torch.float64, device=DEV)), ("status", torch.ones(2, dtype=torch.int32, device=DEV)),
                      ("samples", dict(X=1)), ("samples", {k: v[:2] for k, v in _samples(case).items()})):
        with pytest.raises(ValueError, match=name):
            refine_poses_icp(**dict(a, **{name: bad}))
    with pytest.raises(ValueError, match="image_ids"):
        refine_poses_icp(**dict(a, image_ids=[0, 1, 2]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine_poses_icp(**dict(a, R=a["R"].cpu()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine_poses_icp(**dict(a, depth=a["depth"].cpu()))


# ------------------------------------------------------------------------------------------------------------------ the callers
def test_estimate_poses_refine_is_the_composition_of_its_steps():
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
    spec = dict(meshes=MeshSet.from_arrays(v, faces=f), depth=torch.from_numpy(rng.uniform(300.0, 1500.0, (2, 480, 640)).astype(np.float32)).cuda(),
                max_dist=40.0, grid=16, max_iters=5)
    kw = dict(img_index=idx, seed=3)
    plain = Q.estimate_poses(net, frames, boxes, p3d, K, **kw)
    none = Q.estimate_poses(net, frames, boxes, p3d, K, refine=None, icp=spec, **kw)
    assert all(torch.equal(x, y) for x, y in zip(plain[:4], none[:4])) and np.array_equal(plain[4], none[4])      # the default is unchanged
    lm = Q.estimate_poses(net, frames, boxes, p3d, K, refine="lm", **kw)
    rest = {k: x for k, x in spec.items() if k not in ("meshes", "depth", "max_dist")}
    for refine, start in (("icp", plain), ("lm+icp", lm)):
        R, t, inl, status, final = Q.estimate_poses(net, frames, boxes, p3d, K, refine=refine, icp=spec, **kw)
        assert torch.equal(inl, plain[2]) and torch.equal(status, plain[3]) and np.array_equal(final, plain[4])
        R2, t2, st2, info = Q.refine_poses_icp(start[0], start[1], K, spec["meshes"], spec["depth"], spec["max_dist"], image_ids=idx, status=plain[3], **rest)
        assert torch.equal(R, R2) and torch.equal(t, t2) and tuple(R.shape) == (4, 3, 3) and tuple(t.shape) == (4, 3, 1)
        assert (st2[plain[3] == 0] == 0).all()
    E = Q.evaluate_poses(net, frames, boxes, p3d, K, R2, t2, p3d.cpu().numpy(), kinds=("add",), refine="lm+icp", icp=spec, **kw)
    assert torch.equal(E[1], R2) and float(E[0]["add"].abs().max()) == 0.0
