"""GPU: row N17 on the device.  cp_radius_graph_* EQUAL to the numpy restatement; cp_graphcut_label EQUAL (labels and flow value) to
scipy's exact max-flow on hand-built inputs; solve_pnp_gc replayed stage by stage from its own records (tests/gc_stages.py) over
shapes, outlier fractions, thresholds, iteration counts, per-crop intrinsics, validity columns and degenerate clouds; the bitwise
properties of the call; and its two callers."""
import numpy as np
import pytest
import torch

from tests import gc_stages as G
from tests import pnp_stages as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------ cp_radius_graph_*
def _clouds(n, m, radius, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < m:                                       # refuse any pair within 1e-9 relative of radius^2
        x = S.lmo_model(512)[:n] if (n == 512 and not out) else rng.uniform(-40, 40, size=(n, 3))
        x = x.astype(np.float32)
        if n < 2 or G.min_margin(x, radius) > 1e-9:
            out.append(x)
    return np.stack(out)


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 512])
def test_radius_graph_equals_the_restatement(n, m):
    from checkerpose_amd.postprocess import radius_graph
    x = _clouds(n, m, 20.0, 100 * n + m)
    g = radius_graph(torch.from_numpy(x[0] if m == 1 else x).to(DEV), 20.0)
    assert (g.M, g.N) == (m, n) and g.offsets.dtype == torch.int32 and g.indices.dtype == torch.int32 and g.base.dtype == torch.int64
    base = 0
    for k in range(m):
        off, idx = G.radius_graph_np(x[k], 20.0)
        o, i = g.neighbours(k)
        assert np.array_equal(o, off) and np.array_equal(i, idx), (n, m, k)
        assert int(g.base[k]) == base and g.totals[k] == len(idx)
        base += len(idx)
    assert g.n_indices == base and g.max_edges == max(g.totals)


def test_radius_graph_without_edges_and_complete():
    from checkerpose_amd.postprocess import radius_graph
    x = _clouds(65, 2, 20.0, 7)
    g = radius_graph(x, 0.0, device=DEV)
    assert g.totals == [0, 0] and not g.offsets.any()
    g = radius_graph(x, 1000.0, device=DEV)
    assert g.totals == [65 * 64] * 2
    for k in range(2):
        o, i = g.neighbours(k)
        assert np.array_equal(o, 64 * np.arange(66)) and np.array_equal(i.reshape(65, 64), np.array([[j for j in range(65) if j != r] for r in range(65)]))


# ------------------------------------------------------------------------------------------------------------ cp_graphcut_label
@pytest.fixture(scope="module")
def label_cases():
    return G.label_cases()


@pytest.mark.parametrize("name", ["random_1", "random_6", "random_63", "random_64", "random_65", "no_edges", "chain_lam1", "chain_lam0.1",
                                  "star_flipped", "star_kept", "two_components", "all_inlier", "all_outlier", "cin_equals_Q", "lam_0", "lam_1",
                                  "n4096_deg8", "ape_512"])
def test_graphcut_label_equals_scipy(label_cases, name):
    from checkerpose_amd.postprocess import graphcut_label
    cin, off, idx, w = label_cases[name]
    lab, flow, status, sweeps = graphcut_label(torch.from_numpy(cin.astype(np.int32)).to(DEV), torch.from_numpy(off).to(DEV),
                                               torch.from_numpy(idx).to(DEV), w)
    lab, flow, status, sweeps = lab.cpu().numpy(), flow.cpu().numpy(), status.cpu().numpy(), sweeps.cpu().numpy()
    print("%s: sweeps %s" % (name, sweeps.tolist()))
    assert not status.any()
    for b in range(len(cin)):
        want, fv = G.label(cin[b], off, idx, w)
        assert np.array_equal(lab[b], want), (name, b, np.nonzero(lab[b] != want)[0][:8])
        assert int(flow[b]) == fv, (name, b)
    assert 16 * int(sweeps.max()) <= G.MAX_SWEEPS


# ------------------------------------------------------------------------------------------------------------ solve_pnp_gc
def _graph(gc, repeat=None):
    from checkerpose_amd.postprocess import radius_graph
    models = gc.models if repeat is None else np.repeat(gc.models, repeat, 0)
    return radius_graph(torch.from_numpy(models).float().to(DEV), G.RADIUS)


def _device_run(gc, first=None, graph=None, graph_ids="case", **kw):
    from checkerpose_amd.postprocess import solve_pnp_gc
    case = gc.case
    n = case.B if first is None else first
    p3 = case.p3d[:n] if case.p3d.ndim == 3 else case.p3d
    K = case.K[:n] if case.K.ndim == 3 else case.K
    gid = gc.graph_ids if isinstance(graph_ids, str) else graph_ids
    args = dict(graph_ids=None if gid is None else torch.from_numpy(np.asarray(gid[:n], np.int32)).to(DEV), column=case.column,
                reproj_threshold=case.thr, spatial_coherence_weight=gc.lam, iterations=case.iterations, min_inliers=gc.min_inliers,
                seed=case.seed, return_stages=True)
    args.update(kw)
    out = solve_pnp_gc(torch.from_numpy(p3).float().to(DEV), torch.from_numpy(case.p2d[:n]).float().to(DEV),
                       torch.from_numpy(case.valid[:n]).to(DEV), torch.from_numpy(K).float().to(DEV), _graph(gc) if graph is None else graph, **args)
    torch.cuda.synchronize()
    R, t, inl, status, st = out
    return [R.cpu().numpy(), t.cpu().numpy()[:, :, 0], inl.cpu().numpy(), status.cpu().numpy(), {k: v.cpu().numpy() for k, v in st.items()}]


def _bitwise(a, b, n=None):
    """everything the call returns, bit for bit -- but for the sweep counts (steps[..., 29]): within a sweep the threads see each other's
    pushes as they land, so how many sweeps a max flow takes depends on their timing; the flow's cut does not"""
    def flat(o):
        steps = o[4]["steps"].copy()
        steps[..., 29] = 0.0
        return list(o[:4]) + [steps] + [o[4][k] for k in sorted(o[4]) if k != "steps"]
    return all(np.array_equal(x[:n], y[:n], equal_nan=True) for x, y in zip(flat(a), flat(b)))


@pytest.mark.parametrize("name", list(G.CASES))
def test_device_stages(name):
    gc = G.CASES[name]()
    R, t, inl, status, st = _device_run(gc)
    assert st["hypotheses"].shape == (gc.B, gc.case.iterations, 14) and st["steps"].shape == (gc.B, G.LO_MAX + 1, G.STEP)
    total = G.check_case(gc, st, R, t, inl, status, log=print)
    if name == "nv_5":
        assert total["status1"] == 0 and total["written"] == 0
    if name.startswith(("shape_", "outliers_", "column_", "per_crop_K")):      # noise-free, 400 iterations: every crop is solved, and known
        assert total["status1"] == gc.B and total["all_inlier"] > 0


@pytest.mark.parametrize("name", list(G.EDGE_CASES))
def test_degenerate_clouds_end_with_status_0_or_1(name):
    gc = G.EDGE_CASES[name]()
    R, t, inl, status, st = _device_run(gc)
    assert set(status.tolist()) <= {0, 1}, status
    for b in range(gc.B):
        if status[b] == 0:
            assert np.array_equal(R[b], np.eye(3)) and not t[b].any() and not inl[b].any()
        else:
            assert np.isfinite(R[b]).all() and np.isfinite(t[b]).all() and inl[b].sum() >= gc.min_inliers and not (inl[b] & ~gc.case.valid[b, :, 0].astype(bool)).any()


def test_bitwise_properties():
    gc = G.CASES["thr_8"]()
    a = _device_run(gc)
    assert _bitwise(a, _device_run(gc))                                         # two calls
    assert _bitwise(a, _device_run(gc, first=1), 1)                             # crop 0 alone == crop 0 inside its batch
    rep = _graph(gc, repeat=3)                                                  # one shared graph == that graph repeated under graph_ids
    assert rep.M == 3 and rep.totals == [rep.totals[0]] * 3
    assert _bitwise(a, _device_run(gc, graph=rep, graph_ids=np.array([2, 0, 1], np.int32)))
    lm = G.CASES["shape_2x4096_lm"]()                                           # per-crop graphs picked by graph_ids, in either order
    b = _device_run(lm)
    g2 = _graph(lm)
    from checkerpose_amd.postprocess import RadiusGraph
    swapped = RadiusGraph(g2.offsets.flip(0).contiguous(), torch.cat([g2.indices[g2.totals[0]:], g2.indices[:g2.totals[0]]]),
                          torch.tensor([0, g2.totals[1]], dtype=torch.int64, device=DEV), g2.totals[::-1], g2.radius)
    assert _bitwise(b, _device_run(lm, graph=swapped, graph_ids=np.array([1, 0], np.int32)))


def test_refusals_on_the_device():
    from checkerpose_amd.postprocess import solve_pnp_gc
    gc = G.CASES["shape_4x33"]()
    with pytest.raises(RuntimeError, match="crop 1"):                           # a graph id outside the graph: refused by the kernel, by name
        _device_run(gc, graph=_graph(gc, repeat=2), graph_ids=np.array([0, 5, 1, 0], np.int32))
    with pytest.raises(ValueError):
        solve_pnp_gc(torch.zeros(33, 3, device=DEV), torch.zeros(2, 33, 2, device=DEV), torch.ones(2, 33, 3, dtype=torch.uint8, device=DEV),
                     torch.eye(3, device=DEV), _graph(gc), iterations=513)


# ------------------------------------------------------------------------------------------------------------ the callers
def test_estimate_poses_gc_is_the_composition_of_its_steps():
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
    graph = Q.radius_graph(p3d, 20.0)
    R, t, inl, status, final = Q.estimate_poses(net, frames, boxes, p3d, K, img_index=idx, solver="gc", graph=graph,
                                                spatial_coherence_weight=0.05, prog_max_iters=128, seed=3)
    padded = [None if b is None else PP.padding_Bbox(b, 1.5) for b in boxes]
    crops = PP.get_roi_batch(frames, padded, 256, PP.INTER_LINEAR, "crop_square_resize", img_index=idx)
    want_final = np.array([[0, 0, 0, 0] if b is None else PP.get_final_Bbox(b, "crop_square_resize", 640, 480) for b in padded])
    assert np.array_equal(final, want_final)
    with torch.no_grad():
        out = net(crops, None)
    p2d, valid, _ = Q.correspondences(out, Bboxes=want_final)
    R2, t2, inl2, st2 = Q.solve_pnp_gc(p3d, p2d, valid, K, graph, spatial_coherence_weight=0.05, iterations=128, seed=3)
    assert torch.equal(R, R2) and torch.equal(t, t2) and torch.equal(inl, inl2) and torch.equal(status, st2)
    assert tuple(R.shape) == (4, 3, 3) and tuple(t.shape) == (4, 3, 1) and status.dtype == torch.int32
    E, Re, te, inle, ste, fe = Q.evaluate_poses(net, frames, boxes, p3d, K, R2, t2, p3d.cpu().numpy(), kinds=("add",), img_index=idx, solver="gc",
                                                graph=graph, spatial_coherence_weight=0.05, prog_max_iters=128, seed=3)
    assert torch.equal(Re, R2) and torch.equal(ste, st2) and float(E["add"].abs().max()) == 0.0


def test_from_id_to_pose_device_backend_is_the_batched_solver():
    from checkerpose_amd.postprocess import from_id_to_pose, radius_graph, solve_pnp_gc
    gc = G.CASES["outliers_0.3"]()
    p3, p2, va, K = gc.case.crop(0)
    # the reference's inputs of one image: a (1, N) "RoI" whose cell x holds keypoint x's image point
    roi_xy = p2.astype(np.float32)[None]
    xid, yid = np.arange(gc.N), np.zeros(gc.N, np.int64)
    bit = va.astype(np.float32)[:, None]
    Rf, tf, inl = from_id_to_pose(p3.astype(np.float32), roi_xy, K.astype(np.float32), bit, xid, yid, use_progressivex=True, progx_backend="device",
                                  neighborhood_ball_radius=20, spatial_coherence_weight=gc.lam, prog_max_iters=400, reprojErr_thresh=2,
                                  return_inliers=True, seed=gc.case.seed)
    valid = np.zeros((1, gc.N, 3), np.uint8)
    valid[0, :, 0] = va
    R, t, _, status = solve_pnp_gc(torch.from_numpy(p3).float().to(DEV), torch.from_numpy(p2).float().to(DEV)[None], torch.from_numpy(valid).to(DEV),
                                   torch.from_numpy(K).float().to(DEV), radius_graph(torch.from_numpy(p3).float().to(DEV), 20.0),
                                   spatial_coherence_weight=gc.lam, iterations=400, seed=gc.case.seed)
    assert int(status[0]) == 1 and inl is None                                 # inliers None, as in the reference (:99)
    assert np.array_equal(Rf, R[0].cpu().numpy()) and np.array_equal(tf, t[0].cpu().numpy()) and tf.shape == (3, 1)
    Rt, tt, _ = gc.case.truth[0]
    assert np.abs(Rf - Rt).max() <= S.e_margins()[0] and np.linalg.norm(tf[:, 0] - tt) <= S.e_margins()[1] * np.linalg.norm(tt)
    few = bit.copy()
    few[np.nonzero(va)[0][5:]] = 0.0                                           # 5 valid points: the identity
    Ri, ti = from_id_to_pose(p3.astype(np.float32), roi_xy, K.astype(np.float32), few, xid, yid, use_progressivex=True, progx_backend="device")
    assert np.array_equal(Ri, np.eye(3)) and not ti.any()
