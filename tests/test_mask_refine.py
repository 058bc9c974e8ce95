"""Row N30 on a CPU: the numpy restatement of csrc/mask_refine.hip (tests/mask_refine_stages.py) against brute force and its own
properties, the checker against its named tamperings, the library's and the wrappers' refusals, and the routing of
estimate_poses_mask_refined with stubs.  Nothing here launches a kernel."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import icp_stages as I
from tests import mask_refine_stages as MR
from tests.pnp_stages import StageError

_RUNS = {}


def _run(name):
    """the restatement's free run of a committed case, computed once and left unchanged"""
    if name not in _RUNS:
        case = MR.make(name)
        smp, D = MR.case_samples(case)
        _RUNS[name] = (case, smp, D, MR.restatement_outputs(case, smp))
    return _RUNS[name]


# ------------------------------------------------------------------------------------------------------------- the restatement
def test_extents_against_brute_force():
    rng = np.random.default_rng(5)
    masks = [rng.random((50, 70)) < p for p in (0.0, 0.02, 0.5, 1.0)] + list(MR.make("masks_70").masks)
    for m in masks:
        row, col = MR.extents(m)
        H, W = m.shape
        for y in range(H):
            xs = [x for x in range(W) if m[y, x]]
            assert tuple(row[y]) == ((xs[0], xs[-1]) if xs else (-1, -1))
        for x in range(W):
            ys = [y for y in range(H) if m[y, x]]
            assert tuple(col[x]) == ((ys[0], ys[-1]) if ys else (-1, -1))
    bits = MR.pack_bits(np.stack(masks), dirty=True).view(np.uint32)
    assert bits.shape == (len(masks), 50, 3) and (bits[:, :, 2] >> 6 == (1 << 26) - 1).all()      # the partial last word, its spare bits set
    assert np.array_equal((bits[:, :, 2] >> 5) & 1, np.stack(masks)[:, :, 69])


def test_own_silhouette_is_a_fixed_point():
    """a pose against its own silhouette: every sample pairs with |r| < 1e-9 and the pose stays within 1e-9"""
    case, smp, D, (rec, R, t, status, info) = _run("self_g5")
    for b in range(case.P):
        row, col = case.extents_of(b)
        a = MR.associate(smp[b]["X"], smp[b]["pixel"], case.grid, case.K_of(b), case.R0[b], case.t0[b], row, col, case.size, case.max_dist)
        n_samples = int((smp[b]["pixel"][:, 0] >= 0).sum())
        assert a["n"] == n_samples == info[b, 2] == info[b, 3] >= 6 and np.abs(a["r"][a["pair"]]).max() < 1e-9
        assert status[b] != 0 and np.abs(R[b] - case.R0[b]).max() < 1e-9 and np.abs(t[b] - case.t0[b]).max() < 1e-9 * case.t0[b][2]


@pytest.mark.parametrize("name", [n for n in MR.CASES])
def test_cost_and_iou(name):
    """on every "shift" and "near" pose: c falls over every accepted step (c' < c over the step's own pairs -- the re-association that
    follows changes the pairs, so the NEXT c is another sum and may lie above c': seen on near_rt_g64), the cost at the returned pose
    lies below the input pose's, and the silhouette IoU with the mask ends not below where it began"""
    case, smp, D, (rec, R, t, status, info) = _run(name)
    for b in range(case.P):
        if case.kind[b] not in ("shift", "near") or status[b] == 0:
            continue
        acc = rec[b][rec[b][:, 4] == 1.0]
        assert len(acc) and (acc[:, 3] < acc[:, 2]).all()
        c_states = np.concatenate([[info[b, 0]], [r[2] for r in rec[b][1:] if not np.isnan(r[0])], [info[b, 1]]])
        print(name, b, "c over the states:", c_states[0], "->", c_states[-1], "non-increasing:", bool((np.diff(c_states) <= 0).all()))
        assert c_states[-1] < c_states[0]
        i0, i1 = MR.silhouette_iou(case, b, case.R0[b], case.t0[b]), MR.silhouette_iou(case, b, R[b], t[b])
        print(name, b, "IoU", i0, "->", i1)
        assert i1 >= i0


def test_dof_t_returns_R_bitwise_and_the_shift_bound():
    for name in ("near_t_g5", "shift_t_g64", "shift_t_g5"):
        case, smp, D, (rec, R, t, status, info) = _run(name)
        assert case.dof == "t" and (status != 0).all() and np.array_equal(R.view(np.uint64), case.R0.view(np.uint64))
        done = ~np.isnan(rec[:, :, 0])
        assert np.array_equal(np.broadcast_to(case.R0.reshape(case.P, 1, 9), rec[:, :, 6:15].shape)[done].view(np.uint64), rec[:, :, 6:15][done].view(np.uint64))
        for b in range(case.P):
            if case.kind[b] == "shift":
                e = MR.shift_error(case, b, t[b])
                print(name, b, "shift error / Z", e)
                assert e <= MR.SHIFT_BOUND


def test_measured_tau_and_the_route():
    tau, shift = MR.measure_all()
    assert tau[0] <= MR.MEASURED_TAU[0] <= 2 * max(tau[0], 1e-16) and tau[1] <= MR.MEASURED_TAU[1] <= 2 * max(tau[1], 1e-16)
    assert shift <= MR.SHIFT_BOUND <= 1.25 * shift
    for name in MR.CASES:                                                         # the kernel's summation order passes the replay too
        case, smp, D, _ = _run(name)
        MR.check_case(case, smp, *MR.restatement_outputs(case, smp, sums=MR.kernel_sum), renders=D)


@pytest.mark.parametrize("name", [n for n in MR.CASES])
def test_checker_accepts_the_restatement(name):
    case, smp, D, out = _run(name)
    st = MR.check_case(case, smp, *out, renders=D)
    assert st["iters"] > 0 or st["passed"] == case.P


@pytest.mark.parametrize("tamper", MR.TAMPERINGS)
def test_tampering_is_caught(tamper):
    """ONE rule changed: the named case's outputs change, and check_case refuses the changed outputs"""
    case, smp, D, good = _run(MR.TAMPER_CASE[tamper])
    bad_smp, _ = MR.case_samples(case, (tamper,))
    bad = MR.restatement_outputs(case, bad_smp, tamper=(tamper,))
    assert any(not np.array_equal(g, x, equal_nan=True) for g, x in zip(good, bad)) or any(not np.array_equal(g["pixel"], x["pixel"]) for g, x in zip(smp, bad_smp))
    with pytest.raises(StageError):
        MR.check_case(case, bad_smp, *bad, renders=D)


def test_tamperings_listed():
    assert set(MR.TAMPERINGS) == {"no_border", "no_half", "right_first", "swap_axes", "no_gate", "no_reassoc", "ignore_mask_ids", "t_moves_R"} == set(MR.TAMPER_CASE)
    assert len(MR.TAMPERINGS) >= 8 and all(n in MR.CASES for n in MR.TAMPER_CASE.values())


def test_what_the_cases_cover():
    cases = {n: MR.make(n) for n in MR.CASES}
    assert {c.size for c in cases.values()} == {(96, 80), (70, 50)} and {c.grid for c in cases.values()} == {1, 5, 64}
    assert {c.dof for c in cases.values()} == {"t", "rt"}
    assert any(c.K.ndim == 3 for c in cases.values()) and any(c.mesh_ids is not None and len(set(c.mesh_ids)) == 3 for c in cases.values())
    c = cases["near_t_g5"]
    assert len(c.masks) < c.P and list(c.mask_ids) != sorted(c.mask_ids)          # shared and permuted
    case, smp, D, (rec, R, t, status, info) = _run("near_rt_g64")
    assert all(s["shape"][0] == s["rect"][2] - s["rect"][0] + 1 < 64 for s in smp)          # grid 64: nx = w
    case, smp, D, (rec, R, t, status, info) = _run("near_g1")
    assert (status == 0).all() and (info[:, 2] == 4).all()                        # four slots: below min_pairs
    case, smp, D, (rec, R, t, status, info) = _run("edges_96")
    W = case.size[0]
    assert status[0] != 0 and (D[1] > 0)[:, W - 1].any() and status[1] != 0       # cut at the right edge, still refined
    tam = MR.case_samples(case, ("no_border",))[0][1]
    assert (tam["pixel"][:, 0] == W - 1).any() and not (smp[1]["pixel"][:, 0] == W - 1).any()      # its border samples are dropped
    assert smp[2]["ok"] == 1 and not D[2].any() and info[2, 2] == 0               # wholly outside
    assert smp[3]["ok"] == 0 and np.isnan(case.R0[4]).any() and case.status_in[5] == 0
    assert case.mask_of(6) is None and case.mesh_of(7) is None and (status[2:] == 0).all()
    assert np.array_equal(R[2:].view(np.uint64), case.R0[2:].view(np.uint64)) and np.array_equal(t[2:].view(np.uint64), case.t0[2:].view(np.uint64))
    case, smp, D, (rec, R, t, status, info) = _run("masks_70")
    m = case.masks
    assert not m[1].any() and m[2].all() and m[3].sum() == 1 and m[4, 0, 0] and not m[4, 0, 1]
    assert status[0] != 0 and status[1] == 0 and status[2] == 0 and status[3] == 0 and info[2, 3] == 0      # the full frame: every extent on the border
    for name in ("shift_t_g64", "shift_t_g5"):
        c = cases[name]
        assert all(k == "shift" and s[0] == int(s[0]) for k, s in zip(c.kind, c.shift))


# ------------------------------------------------------------------------------------------------------------- the library
def test_abi_refusals():
    """the library on a CPU box: the new symbols resolve, the scratch sizing, refusals with fake pointers (nothing launches)"""
    from checkerpose_amd import _abi
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import refine_mask as M
    lib = _abi.load()
    assert lib.cp_version() >= 240
    assert lib.cp_mask_refine_record_doubles() == MR.REC == M.MASK_REFINE_RECORD and lib.cp_mask_refine_info_doubles() == MR.INFO == M.MASK_REFINE_INFO
    assert lib.cp_contour_samples_scratch_bytes(3, 64, 5) == 288 + 3 * 20 * 8 + 3 * 64 * 16 and lib.cp_contour_samples_scratch_bytes(0, 64, 5) == 0
    assert lib.cp_contour_samples_scratch_bytes(3, -1, 5) == 0 and lib.cp_contour_samples_scratch_bytes(3, 64, 0) == 0 and lib.cp_contour_samples_scratch_bytes(3, 64, 65) == 0
    for n in ("mask_extents", "contour_samples", "refine_poses_mask", "estimate_poses_mask_refined"):
        assert getattr(PP, n) is getattr(M, n)
    buf = C.create_string_buffer(4096 + 16)
    p = (C.addressof(buf) + 15) & ~15

    def call(fn, ok, *pairs):
        a = list(ok)
        for i, v in pairs:
            a[i] = v
        lib.cp_kernel_log_begin()
        rc = fn(*a)
        assert lib.cp_kernel_log() == b""
        return rc

    #        0     1  2  3   4   5  6
    ok_e = [None, p, 2, 50, 70, p, p]
    e = lambda *pairs: call(lib.cp_mask_extents, ok_e, *pairs)      # noqa: E731
    INVALID, ALIGN, RANGE = e((1, None)), e((1, p + 2)), e((3, 1 << 16), (4, 1 << 16))
    assert len({0, INVALID, ALIGN, RANGE}) == 4
    assert [e((5, None)), e((6, None)), e((2, 0)), e((3, 0)), e((4, -1))] == [INVALID] * 5 and [e((5, p + 2)), e((6, p + 2))] == [ALIGN] * 2
    #        0     1  2  3  4  5  6  7  8  9     10  11  12 13 14 15 16 17 18 19 20 21
    ok_s = [None, p, p, 0, p, p, p, p, 1, None, 80, 96, 3, 8, 5, p, p, p, p, p, p, p]
    s = lambda *pairs: call(lib.cp_contour_samples, ok_s, *pairs)      # noqa: E731
    assert [s((i, None)) for i in (1, 2, 4, 5, 6, 7, 15, 16, 17, 18, 19, 20, 21)] == [INVALID] * 13
    assert [s((14, 0)), s((14, 65)), s((8, 0)), s((8, 2)), s((3, 4)), s((10, 0)), s((12, 0))] == [INVALID] * 7
    assert [s((21, p + 8)), s((1, p + 4)), s((2, p + 4)), s((15, p + 2)), s((17, p + 2)), s((18, p + 2)), s((19, p + 4)), s((20, p + 2))] == [ALIGN] * 8
    assert s((10, 1 << 16), (11, 1 << 16)) == RANGE
    #        0     1  2  3  4  5  6  7  8  9  10    11 12  13  14 15    16 17  18    19 20 21 22 23 24
    ok_r = [None, p, p, 0, p, p, p, 5, p, p, None, 3, 80, 96, p, None, 1, 20, 1e-6, 6, 3, p + 512, p, p, None]
    r = lambda *pairs: call(lib.cp_mask_refine, ok_r, *pairs)      # noqa: E731
    assert [r((i, None)) for i in (1, 2, 4, 5, 6, 8, 9, 14, 21, 22, 23)] == [INVALID] * 11
    assert [r((7, 0)), r((7, 65)), r((16, 2)), r((16, -1)), r((17, 0)), r((17, 65)), r((18, 0.0)), r((18, float("inf"))), r((18, float("nan"))), r((19, 5)),
            r((11, 0)), r((11, 4)), r((20, 0)), r((3, 4)), r((12, 0))] == [INVALID] * 15
    assert r((11, 4), (10, p), (12, 1 << 16), (13, 1 << 16)) == RANGE             # with ids NM != P is no refusal (the size rule speaks next)
    assert [r((1, p + 4)), r((4, p + 4)), r((5, p + 2)), r((6, p + 2)), r((8, p + 2)), r((9, p + 2)), r((10, p + 2)), r((14, p + 4)), r((15, p + 2)),
            r((21, p + 516)), r((22, p + 2)), r((23, p + 4)), r((24, p + 4))] == [ALIGN] * 13
    assert r((21, p + 8)) == INVALID                                              # a partial overlap of the poses
    assert r((12, 1 << 16), (13, 1 << 16)) == RANGE and r((20, 1 << 24), (11, 1 << 24), (21, p)) == RANGE


# ------------------------------------------------------------------------------------------------------------- the Python layer
def _host_args():
    from checkerpose_amd.coco_eval import PackedMasks
    from checkerpose_amd.metric import MeshSet
    v, f = I.mesh_arrays(("box",))
    ms = MeshSet.from_arrays(v, faces=f)
    full = PackedMasks(torch.zeros(1, 80, 3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.full((1, 4), -1, dtype=torch.int32), 80, 96)
    return dict(R=torch.eye(3, dtype=torch.float64)[None], t=torch.tensor([[0.0, 0.0, 300.0]], dtype=torch.float64), cam_K=torch.from_numpy(I.K_A),
                meshes=ms, full=full, max_dist=8.0, dof="t")


def test_defaults_and_refusals():
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd.coco_eval import PackedMasks
    assert str(inspect.signature(PP.refine_poses_mask)) == ("(R, t, cam_K, meshes, full, max_dist, dof, mask_ids=None, mesh_ids=None, status=None, grid=32, "
                                                            "max_iters=20, step_tol=1e-06, min_pairs=6, return_records=False)")
    assert str(inspect.signature(PP.contour_samples)) == "(R, t, cam_K, meshes, size, mesh_ids=None, grid=32)" and str(inspect.signature(PP.mask_extents)) == "(masks)"
    assert str(inspect.signature(PP.estimate_poses_mask_refined)) == "(net, frames, Bboxes, p3d_xyz, cam_K, refine_mask, verify, return_verify=False, **estimate_kwargs)"
    a = _host_args()
    with pytest.raises(TypeError):                                                # max_dist and dof have no default
        PP.refine_poses_mask(a["R"], a["t"], a["cam_K"], a["meshes"], a["full"])
    for bad in (None, "r", "tr", 1):
        with pytest.raises(ValueError, match="dof"):
            PP.refine_poses_mask(**dict(a, dof=bad))
    for key, bad, match in (("max_iters", 0, "max_iters"), ("max_iters", 65, "max_iters"), ("step_tol", 0.0, "step_tol"), ("step_tol", float("inf"), "step_tol"),
                            ("min_pairs", 5, "min_pairs"), ("grid", 0, "grid"), ("grid", 65, "grid"), ("max_dist", 0.0, "max_dist"), ("max_dist", float("nan"), "max_dist"),
                            ("full", None, "full"), ("full", torch.zeros(1, 80, 3, dtype=torch.int32), "full")):
        with pytest.raises(ValueError, match=match):
            PP.refine_poses_mask(**dict(a, **{key: bad}))
    z = lambda n, h, w: PackedMasks(torch.zeros(n, h, (w + 31) // 32, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), None, h, w)      # noqa: E731
    with pytest.raises(ValueError, match="no masks"):
        PP.refine_poses_mask(**dict(a, full=z(0, 80, 96)))
    with pytest.raises(ValueError, match="no masks"):
        PP.mask_extents(z(0, 80, 96))
    with pytest.raises(ValueError, match="masks"):
        PP.mask_extents(torch.zeros(1, 80, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="grid"):
        PP.contour_samples(a["R"], a["t"], a["cam_K"], a["meshes"], (96, 80), grid=65)
    for call in (lambda: PP.refine_poses_mask(**a), lambda: PP.mask_extents(a["full"]),
                 lambda: PP.contour_samples(a["R"], a["t"], a["cam_K"], a["meshes"], (96, 80))):      # well-formed arguments on the host: still no fallback
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_refine_mask_values():
    from checkerpose_amd import postprocess as PP
    frames, p3d, K = torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(8, 3), torch.eye(3)
    ok_v = dict(meshes=None)
    for bad in (None, "yes", dict(), dict(max_dist=8.0), dict(dof="t")):
        with pytest.raises(ValueError, match="refine_mask"):
            PP.estimate_poses_mask_refined(None, frames, [], p3d, K, bad, ok_v)
    for extra in ("meshes", "mask_ids", "status", "mesh_ids", "return_records"):
        with pytest.raises(ValueError, match="unknown"):
            PP.estimate_poses_mask_refined(None, frames, [], p3d, K, {"max_dist": 8.0, "dof": "t", extra: 1}, ok_v)
    ok_r = dict(max_dist=8.0, dof="t")
    with pytest.raises(ValueError, match="verify"):
        PP.estimate_poses_mask_refined(None, frames, [], p3d, K, ok_r, dict())
    with pytest.raises(NotImplementedError, match="warp_affine"):
        PP.estimate_poses_mask_refined(None, frames, [], p3d, K, ok_r, ok_v, resize_method="crop_resize_by_warp_affine")
    with pytest.raises(ValueError, match="refine"):
        PP.estimate_poses_mask_refined(None, frames, [], p3d, K, ok_r, ok_v, refine="gn")


def test_estimate_poses_mask_refined_routes(monkeypatch):
    """ONE forward, the pastes, the last stage's pose through refine_poses_mask, the candidates' order with "sil" last, the ONE
    verify_poses_mask and ONE select_poses call, with stubs in place of every device call"""
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import preprocess as PRE
    B = 2
    calls = []
    base_R = torch.arange(B * 9, dtype=torch.float64).reshape(B, 3, 3)
    base_t = torch.arange(B * 3, dtype=torch.float64).reshape(B, 3, 1)
    status = torch.tensor([1, 1], dtype=torch.int32)
    rstatus = torch.tensor([2, 0], dtype=torch.int32)
    monkeypatch.setattr(PRE, "get_roi_batch", lambda *a, **k: "crops")
    monkeypatch.setattr(PP, "correspondences", lambda out, **k: ("p2d", "valid", None))
    monkeypatch.setattr(PP, "solve_pnp_ransac", lambda *a, **k: (base_R, base_t, "inl", status))
    monkeypatch.setattr(PP, "refine_poses_lm", lambda p3d, p2d, mask, K, R, t, status=None: (calls.append(("lm",)), (R + 100.0, t + 100.0, None, None))[1])

    def net(crops, _):
        calls.append(("forward",))
        return ("roi", "xb", "yb", "SEG", "xid", "yid")

    def paste(seg, boxes, frame_size, method, channel):
        calls.append(("paste", seg, boxes, frame_size, method, channel))
        return "masks%d" % channel

    def refine(R, t, K, meshes, full, max_dist, dof, **kw):
        calls.append(("sil", R, t, K, meshes, full, max_dist, dof, kw))
        return R + 1000.0, t + 1000.0, rstatus, "rinfo"

    def verify(R, t, K, meshes, full, **kw):
        calls.append(("verify", R, t, K, meshes, full, kw))
        P = R.shape[0]
        return torch.arange(P, dtype=torch.float64), dict(ok=torch.ones(P, dtype=torch.bool), marker="info")

    def select(score, ok, R, t):
        calls.append(("select", score, ok, R, t))
        choice = torch.tensor([score.shape[0] - 1, 0], dtype=torch.int32)
        return choice, R[choice.long(), torch.arange(B)], t[choice.long(), torch.arange(B)]

    monkeypatch.setattr(PP, "paste_masks", paste)
    monkeypatch.setattr(PP, "refine_poses_mask", refine)
    monkeypatch.setattr(PP, "verify_poses_mask", verify)
    monkeypatch.setattr(PP, "select_poses", select)
    frames = torch.zeros(2, 40, 48, 3, dtype=torch.uint8)
    K = np.stack([I.K_A, I.K_B])
    boxes = [[5, 5, 10, 10], [6, 6, 10, 10]]
    args = (net, frames, boxes, "p3d", K)
    spec = dict(meshes="VM", mesh_ids=[1, 0])
    rspec = dict(max_dist=7.0, dof="t", grid=5)
    for refine_kw, names, shift in ((None, ("solver", "sil"), (0.0, 1000.0)), ("lm", ("solver", "lm", "sil"), (0.0, 100.0, 1100.0))):
        del calls[:]
        R, t, inl, st, final, rep = PP.estimate_poses_mask_refined(*args, rspec, spec, return_verify=True, img_index=[1, 0], refine=refine_kw, resize_method="crop_resize")
        C_ = len(names)
        assert [c[0] for c in calls] == ["forward"] + ["lm"] * (C_ - 2) + ["paste", "paste", "sil", "verify", "select"]      # ONE forward, ONE of each
        sil = [c for c in calls if c[0] == "sil"][0]
        assert torch.equal(sil[1], base_R + shift[-2]) and torch.equal(sil[2], base_t + shift[-2]) and sil[3] is K and sil[4] == "VM" and sil[5] == "masks1"
        assert sil[6] == 7.0 and sil[7] == "t" and sorted(sil[8]) == ["grid", "mesh_ids", "status"] and sil[8]["grid"] == 5 and torch.equal(sil[8]["status"], status)
        v, s = calls[-2], calls[-1]
        want_R = torch.cat([base_R + x for x in shift])
        want_t = torch.cat([base_t + x for x in shift])
        assert torch.equal(v[1], want_R) and torch.equal(v[2], want_t) and np.array_equal(v[3], np.concatenate([K] * C_)) and v[5] == "masks1"
        kw = v[6]
        assert list(kw["mask_ids"]) == [0, 1] * C_ and list(kw["mesh_ids"]) == [1, 0] * C_ and kw["visible"] == "masks0"
        assert kw["status"].tolist() == [1, 1] * (C_ - 1) + [1, 0]                  # a pass-through "sil" is no candidate
        assert torch.equal(s[3], want_R.view(C_, B, 3, 3)) and torch.equal(R[0], base_R[0] + shift[-1]) and torch.equal(R[1], base_R[1])
        assert inl == "inl" and st is status and rep["stages"] == names and rep["refine"][0] is rstatus and rep["refine"][1] == "rinfo"
        assert len(PP.estimate_poses_mask_refined(*args, rspec, spec, img_index=[1, 0], refine=refine_kw, resize_method="crop_resize")) == 5
    assert sorted(spec) == ["mesh_ids", "meshes"] and sorted(rspec) == ["dof", "grid", "max_dist"]      # the callers' dicts are left alone
