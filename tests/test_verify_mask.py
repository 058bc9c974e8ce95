"""CPU: row N28's rule in numpy (tests/verify_mask_stages.py) -- its identities on CPU renders, its tamperings, what the committed cases
cover --, the library's host half with fake pointers, and the Python layer's refusals, defaults and estimate_poses_mask_verified's routing
with stubs (no device)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import icp_stages as I
from tests import verify_mask_stages as VM
from tests.pnp_stages import StageError


def _run(name):
    """a committed case on the CPU: (case, render_f32 renders, the rule's outputs); the first two cached by verify_mask_stages"""
    case = VM.make(name)
    D = VM.cpu_renders(case)
    return case, D, VM.reference(case, D)


# ------------------------------------------------------------------------------------------------------------------- the rule
def test_pack_and_read_by_hand():
    m = np.zeros((1, 2, 70), bool)
    m[0, 0, [0, 31, 32, 69]] = True
    m[0, 1, 5] = True
    bits = VM.pack(m)
    assert bits.dtype == np.int32 and bits.shape == (1, 2, 3)
    assert bits.view(np.uint32).tolist() == [[[1 | (1 << 31), 1, 1 << 5], [1 << 5, 0, 0]]]
    assert np.array_equal(VM.read(bits, 2, 70), m)
    assert not np.array_equal(VM.read(bits, 2, 70, ("bit_reverse",)), m) and not np.array_equal(VM.read(bits, 2, 70, ("floor_stride",)), m)
    assert VM.read(bits, 2, 70, ("bit_reverse",))[0, 0, [0, 31]].tolist() == [True, True] and VM.read(bits, 2, 70, ("bit_reverse",))[0, 1, 26]
    w96 = np.random.default_rng(0).random((2, 3, 96)) < 0.5
    assert np.array_equal(VM.read(VM.pack(w96), 3, 96), w96) and np.array_equal(VM.read(VM.pack(w96), 3, 96, ("floor_stride",)), w96)      # 96 = 3 * 32


def test_translation_by_hand():
    """a 2 x 2 silhouette on a 6 x 4 frame against its own mask, the mask moved one pixel, two pixels, and the complement"""
    D = np.zeros((4, 6), np.float32)
    D[1:3, 1:3] = 300.0
    own = D > 0
    assert VM.counts_of(D, own) == (4, 4, 0) and VM.box_of(D) == [1, 1, 2, 2]
    assert VM.finish(4, 4, 0, 4, 0)[:2] == (1.0, 1.0) and VM.finish(4, 4, 0, 4, 0)[3] and np.isnan(VM.finish(4, 4, 0, 4, 0)[2])
    one = np.roll(own, 1, 1)                                                     # columns 2..3: two pixels shared, union 4 + 4 - 2 = 6
    assert VM.counts_of(D, one) == (4, 2, 0) and VM.finish(4, 2, 0, 4, 0)[0] == 2.0 / 6.0
    assert VM.finish(4, 2, 0, 4, 0, tamper=("union_no_inter",))[0] == 2.0 / 8.0
    two = np.roll(own, 2, 1)                                                     # disjoint
    assert VM.counts_of(D, two) == (4, 0, 0) and VM.finish(4, 0, 0, 4, 0)[0] == 0.0 and VM.finish(4, 0, 0, 4, 0)[3]
    diag = np.roll(one, 1, 0)                                                    # one pixel shared
    assert VM.counts_of(D, diag, own) == (4, 1, 4) and VM.finish(4, 1, 4, 4, 4)[::2] == (1.0 / 7.0, 1.0)
    assert VM.counts_of(D, ~one)[1] == 4 - 2
    assert VM.counts_of(D, own, tamper=("ge_zero",)) == (24, 4, 0) and VM.box_of(D, ("ge_zero",)) == [0, 0, 5, 3]
    # the finish's special values
    s, iou, cover, ok = VM.finish(0, 0, 0, 0, 0)
    assert np.isnan(s) and np.isnan(iou) and np.isnan(cover) and not ok          # union == 0
    s, iou, cover, ok = VM.finish(9, 0, 0, 0, 5)
    assert (s, cover, ok) == (0.0, 0.0, True)                                    # an empty full mask under a non-empty render: exactly 0
    s, iou, cover, ok = VM.finish(0, 0, 0, 7, 5, counted=False)
    assert np.isnan(s) and np.isnan(cover) and not ok
    assert VM.finish(1 << 24, 1 << 23, 0, 1 << 24, 0)[0] == (1 << 23) / float(3 << 23)      # the largest sums the frame bound allows: exact
    lab = VM.labels_of(D, one, own, True)
    assert lab[1].tolist() == [0, 1 | 4, 1 | 2 | 4, 2, 0, 0] and VM.labels_of(D, one, None, False)[1].tolist() == [0, 0, 2, 2, 0, 0]


@pytest.mark.parametrize("name", list(VM.CASES))
def test_identities_on_cpu_renders(name):
    """per counted pose: the counts are what a dense comparison gives; the pose's own silhouette gives iou == 1, a mask disjoint from
    it iou == 0, a mask and its complement split n_model; and the condition: poses with 0 < n_inter < min(n_model, n_mask) exist"""
    case, D, out = _run(name)
    VM.check_case(case, D, out)
    F, Vm = case.masks(D)
    assert len(VM.nontrivial(case, D)) >= 1
    for b in range(case.P):
        n = out["counts"][b]
        if not case.counted(b):
            assert not n[:3].any() and (out["box"][b] == -1).all() and np.isnan(out["score"][b]) and np.isnan(out["cover"][b]) and not out["ok"][b]
            continue
        sil = D[b] > 0
        m = case.mask_of(b)
        assert n[0] == sil.sum() and n[1] == (sil & F[m]).sum() and n[3] == F[m].sum() and n[1] <= min(n[0], n[3])
        assert n[2] == (0 if Vm is None else (sil & Vm[m]).sum()) and n[4] == (0 if Vm is None else Vm[m].sum())
        assert VM.counts_of(D[b], F[m])[1] + VM.counts_of(D[b], ~F[m])[1] == n[0]                    # complement symmetry
        if n[0]:
            own = VM.finish(n[0], VM.counts_of(D[b], sil)[1], 0, int(sil.sum()), 0)
            assert own[0] == 1.0 and own[3]
            assert VM.finish(n[0], VM.counts_of(D[b], ~sil)[1], 0, int((~sil).sum()), 0)[0] == 0.0
            ys, xs = np.nonzero(sil)
            assert out["box"][b].tolist() == [xs.min(), ys.min(), xs.max(), ys.max()]
        if out["ok"][b]:
            assert 0.0 <= out["score"][b] <= 1.0 and out["score"][b] == out["iou"][b] == n[1] / float(int(n[0]) + int(n[3]) - int(n[1]))
        lab = out["labels"][b]
        assert np.array_equal(lab & 1, sil.astype(np.uint8)) and np.array_equal((lab >> 1) & 1, F[m].astype(np.uint8))


@pytest.mark.parametrize("tamper", VM.TAMPERINGS)
def test_tamperings_are_caught(tamper):
    """ONE rule changed: the named case's outputs change, and check_case refuses the changed outputs"""
    case, D, good = _run(VM.CAUGHT_BY[tamper])
    bad = VM.reference(case, D, (tamper,))
    assert not np.array_equal(good["counts"], bad["counts"]) or not np.array_equal(good["score"], bad["score"], equal_nan=True)
    with pytest.raises(StageError):
        VM.check_case(case, D, bad)


def test_tamperings_listed():
    assert set(VM.TAMPERINGS) == {"bit_reverse", "floor_stride", "union_no_inter", "vis_area", "ignore_mask_ids", "ge_zero"} == set(VM.CAUGHT_BY)
    assert all(n in VM.CASES for n in VM.CAUGHT_BY.values())


def test_what_the_cases_cover():
    cases = {n: VM.make(n) for n in VM.CASES}
    assert {c.size for c in cases.values()} == {(96, 80), (70, 50)}
    assert any(c.K.ndim == 3 for c in cases.values()) and any(c.K.ndim == 2 for c in cases.values())
    assert any(c.holes is None for c in cases.values()) and any(c.holes is not None for c in cases.values())
    assert any(c.mask_ids is None for c in cases.values())
    a = cases["mixed_a_6"]
    assert len(set(a.mesh_ids)) == 3 and len(set(a.mask_ids)) < a.P and list(a.mask_ids) != sorted(a.mask_ids) and a.N == 4      # shared and permuted
    case, D, out = _run("mixed_a_6")
    F, _ = case.masks(D)
    assert F[2].all() and np.array_equal(F[1], VM.checkerboard(case.size)) and out["counts"][3, 1] == out["counts"][3, 0]        # the full frame
    case, D, out = _run("mixed_b_5")
    F, Vm = case.masks(D)
    assert Vm is None and np.array_equal(F[0], D[0] > 0) and out["score"][0] == 1.0 and out["ok"][0]                         # the own silhouette
    assert not F[2].any() and out["counts"][2, 0] > 0 and out["score"][2] == 0.0 and out["ok"][2]                            # the empty mask
    assert F[3].sum() == 1 and F[3][:, 69].any() and out["counts"][3].tolist()[:2] == [out["counts"][3, 0], 1]               # one pixel, last column
    assert np.nonzero((D[3] > 0).any(0))[0].max() == 69 and np.isnan(out["cover"]).all()                                    # partly off the frame
    for name in ("edges_a_9", "edges_b_9"):
        case, D, e = _run(name)
        W = case.size[0]
        assert np.nonzero((D[0] > 0).any(0))[0].max() == W - 1 and e["ok"][0]                                                # cut at the right edge
        assert case.rendered(1) and not D[1].any() and e["ok"][1] and e["score"][1] == 0.0 and (e["box"][1] == -1).all()      # wholly off: iou 0
        assert not case.rendered(2) and case.rendered(3) and case.status[3] == 0 and case.mask_ids[4] >= case.N and not case.rendered(5)
        assert case.mesh_ids[6] >= len(case.meshes) and np.isnan(e["score"][2:7]).all() and not e["ok"][2:7].any() and not e["counts"][2:7, :3].any()
        assert e["counts"][4].tolist() == [0] * 5 and not e["labels"][4].any() and (e["labels"][3] & 2).any() and not (e["labels"][3] & 1).any()
        assert e["ok"][7] and e["ok"][8] and 0 < e["cover"][7] < 1
    s = _run("select_a")[2]
    assert s["choice"].tolist() == [1, 0] and s["score"][2] == s["score"][4] > s["score"][0]                                 # the exact tie
    assert _run("select_b")[2]["choice"].tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------------------- the library
def test_abi_refusals():
    """the library on a CPU box: the new symbols resolve, the scratch sizing, refusals with fake pointers (nothing launches)"""
    from checkerpose_amd import _abi
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import verify_mask as M
    lib = _abi.load()
    assert lib.cp_version() >= 238
    assert lib.cp_verify_poses_mask_scratch_bytes(3, 64) == 384 + 3 * 64 * 16 and lib.cp_verify_poses_mask_scratch_bytes(0, 64) == 0
    assert lib.cp_verify_poses_mask_scratch_bytes(3, -1) == 0 and lib.cp_verify_poses_mask_scratch_bytes(1, 0) == 128
    assert M.VERIFY_MASK_COUNTS == VM.COUNTS and M.VERIFY_MASK_MAX_PIXELS == 1 << 24
    assert M.VERIFY_MASK_LABELS == {"model": VM.MODEL, "full": VM.FULL, "visible": VM.VISIBLE}
    assert PP.verify_poses_mask is M.verify_poses_mask and PP.estimate_poses_mask_verified is M.estimate_poses_mask_verified
    buf = C.create_string_buffer(4096 + 16)
    p = (C.addressof(buf) + 15) & ~15
    #       0     1  2  3  4  5  6  7  8  9     10 11 12    13    14    15 16  17  18    19 20 21 22 23 24 25 26 27    28
    ok_a = [None, p, p, 0, p, p, p, p, 1, None, p, p, None, None, None, 3, 80, 96, None, 3, 8, p, p, p, p, p, p, None, p]

    def a_with(*pairs):
        a = list(ok_a)
        for i, v in pairs:
            a[i] = v
        lib.cp_kernel_log_begin()
        rc = lib.cp_verify_poses_mask(*a)
        assert lib.cp_kernel_log() == b""
        return rc

    INVALID, ALIGN, RANGE = a_with((1, None)), a_with((1, p + 4)), a_with((16, 4097), (17, 4096))
    assert len({0, INVALID, ALIGN, RANGE}) == 4
    assert [a_with((i, None)) for i in (2, 4, 5, 6, 7, 10, 11, 21, 22, 23, 24, 25, 26, 28)] == [INVALID] * 14                  # null
    assert [a_with((8, 0)), a_with((8, 2)), a_with((20, 0)), a_with((3, 4)), a_with((16, 0)), a_with((17, 0)), a_with((19, 0)), a_with((19, -2))] == [INVALID] * 8
    assert [a_with((15, 0)), a_with((15, -1)), a_with((15, 2)), a_with((15, 4))] == [INVALID] * 4                             # M; no ids although M != P
    assert a_with((15, 4), (14, p), (16, 4097), (17, 4096)) == RANGE                                                          # with ids M != P is no refusal (the size rule speaks next)
    assert [a_with((12, p)), a_with((13, p))] == [INVALID] * 2                                                                # visible without its area, and the reverse
    assert [a_with((28, p + 8)), a_with((2, p + 4)), a_with((23, p + 4)), a_with((24, p + 4)), a_with((25, p + 4)), a_with((4, p + 2)), a_with((9, p + 2)),
            a_with((10, p + 2)), a_with((11, p + 2)), a_with((12, p + 2), (13, p)), a_with((12, p), (13, p + 2)), a_with((14, p + 2)), a_with((18, p + 2)),
            a_with((21, p + 2)), a_with((22, p + 2))] == [ALIGN] * 15
    assert a_with((16, 0), (28, p + 8)) == INVALID and a_with((16, 4097), (17, 4096), (28, p + 8)) == ALIGN                     # the classes' order
    assert [a_with((16, 1), (17, (1 << 24) + 1)), a_with((16, 4096), (17, 4096), (19, 1 << 12), (15, 1 << 12)),
            a_with((19, 1 << 20), (15, 1 << 20), (20, 1 << 12))] == [RANGE] * 3


# ------------------------------------------------------------------------------------------------------------- the Python layer
def _host_args():
    from checkerpose_amd.coco_eval import PackedMasks
    from checkerpose_amd.metric import MeshSet
    v, f = I.mesh_arrays(("box",))
    ms = MeshSet.from_arrays(v, faces=f)
    full = PackedMasks(torch.zeros(1, 80, 3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.full((1, 4), -1, dtype=torch.int32), 80, 96)
    return dict(R=torch.eye(3, dtype=torch.float64)[None], t=torch.tensor([[0.0, 0.0, 300.0]], dtype=torch.float64), cam_K=torch.from_numpy(I.K_A),
                meshes=ms, full=full)


def test_defaults_and_refusals():
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd.coco_eval import PackedMasks
    sig = inspect.signature(PP.verify_poses_mask)
    assert str(sig) == "(R, t, cam_K, meshes, full, visible=None, mask_ids=None, mesh_ids=None, status=None, return_labels=False)"
    assert str(inspect.signature(PP.estimate_poses_mask_verified)) == "(net, frames, Bboxes, p3d_xyz, cam_K, verify, return_verify=False, **estimate_kwargs)"
    a = _host_args()
    for bad in (None, torch.zeros(1, 80, 3, dtype=torch.int32), "masks"):
        with pytest.raises(ValueError, match="full"):
            PP.verify_poses_mask(**dict(a, full=bad))
    with pytest.raises(ValueError, match="visible"):
        PP.verify_poses_mask(**dict(a, visible=torch.zeros(1, 80, 96)))
    z = lambda n, h, w: PackedMasks(torch.zeros(n, h, (w + 31) // 32, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), None, h, w)      # noqa: E731
    for other in (z(2, 80, 96), z(1, 80, 95), z(1, 79, 96)):                     # another length, width, height
        with pytest.raises(ValueError, match="visible"):
            PP.verify_poses_mask(**dict(a, visible=other))
    with pytest.raises(ValueError, match="bits"):                                # the words' dtype and shape
        PP.verify_poses_mask(**dict(a, full=PackedMasks(torch.zeros(1, 80, 3, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), None, 80, 96)))
    with pytest.raises(ValueError, match="bits"):
        PP.verify_poses_mask(**dict(a, full=PackedMasks(torch.zeros(1, 80, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), None, 80, 96)))
    with pytest.raises(ValueError, match="no masks"):
        PP.verify_poses_mask(**dict(a, full=z(0, 80, 96)))
    with pytest.raises(ValueError, match="2\\^24"):
        PP.verify_poses_mask(**dict(a, full=PackedMasks(torch.zeros(1, 4097, 128, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), None, 4097, 4096)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # well-formed arguments on the host: still no fallback
        PP.verify_poses_mask(**a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.verify_poses_mask(**dict(a, visible=a["full"], return_labels=True))


def test_public_functions_of_postprocess():
    """the new functions live in checkerpose_amd/verify_mask.py and are re-exported: postprocess.py itself defines what it defined"""
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import verify_mask as M
    own = {n for n, f in vars(PP).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == PP.__name__}
    assert "verify_poses_mask" not in own and "estimate_poses_mask_verified" not in own and {"verify_poses", "select_poses", "estimate_poses_verified"} <= own
    assert {n for n, f in vars(M).items() if inspect.isfunction(f) and not n.startswith("_")} == {"verify_poses_mask", "estimate_poses_mask_verified"}


def test_verify_values():
    from checkerpose_amd import postprocess as PP
    frames, p3d, K = torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(8, 3), torch.eye(3)
    for bad in (None, "yes", dict(), dict(mesh_ids=[0]), dict(use_visible=False)):
        with pytest.raises(ValueError, match="verify"):
            PP.estimate_poses_mask_verified(None, frames, [], p3d, K, bad)
    for key in ("image_ids", "status", "mask_ids"):
        with pytest.raises(ValueError, match="must not name"):
            PP.estimate_poses_mask_verified(None, frames, [], p3d, K, {"meshes": None, key: [0]})
    for extra in ("grid", "depth", "tau", "occlusion_weight"):                   # row N26's keys belong to estimate_poses_verified
        with pytest.raises(ValueError, match="unknown"):
            PP.estimate_poses_mask_verified(None, frames, [], p3d, K, {"meshes": None, extra: 1.0})
    ok = dict(meshes=None)
    with pytest.raises(NotImplementedError, match="warp_affine"):
        PP.estimate_poses_mask_verified(None, frames, [], p3d, K, ok, resize_method="crop_resize_by_warp_affine")
    with pytest.raises(ValueError, match="refine"):                              # estimate_poses' own refusals hold
        PP.estimate_poses_mask_verified(None, frames, [], p3d, K, ok, refine="gn")
    with pytest.raises(TypeError):
        PP.estimate_poses_mask_verified(None, frames, [], p3d, K, ok, no_such_keyword=1)


def test_estimate_poses_mask_verified_routes(monkeypatch):
    """ONE forward, the two pastes, the candidates' order, the ONE verify_poses_mask and ONE select_poses call with their arguments and
    the gather, with stubs in place of every device call"""
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import preprocess as PRE
    B = 2
    calls = []
    base_R = torch.arange(B * 9, dtype=torch.float64).reshape(B, 3, 3)
    base_t = torch.arange(B * 3, dtype=torch.float64).reshape(B, 3, 1)
    status = torch.tensor([1, 0], dtype=torch.int32)
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

    def verify(R, t, K, meshes, full, **kw):
        calls.append(("verify", R, t, K, meshes, full, kw))
        P = R.shape[0]
        return torch.arange(P, dtype=torch.float64), dict(ok=torch.ones(P, dtype=torch.bool), marker="info")

    def select(score, ok, R, t):
        calls.append(("select", score, ok, R, t))
        choice = torch.tensor([score.shape[0] - 1, 0], dtype=torch.int32)
        return choice, R[choice.long(), torch.arange(B)], t[choice.long(), torch.arange(B)]

    monkeypatch.setattr(PP, "paste_masks", paste)
    monkeypatch.setattr(PP, "verify_poses_mask", verify)
    monkeypatch.setattr(PP, "select_poses", select)
    frames = torch.zeros(2, 40, 48, 3, dtype=torch.uint8)
    K = np.stack([I.K_A, I.K_B])
    boxes = [[5, 5, 10, 10], [6, 6, 10, 10]]
    args = (net, frames, boxes, "p3d", K)
    spec = dict(meshes="VM", mesh_ids=[1, 0])
    padded = [PRE.padding_Bbox(b, 1.5) for b in boxes]
    for refine, names, shift, use_visible in ((None, ("solver",), (0.0,), True), ("lm", ("solver", "lm"), (0.0, 100.0), True), ("lm", ("solver", "lm"), (0.0, 100.0), False)):
        del calls[:]
        v_spec = dict(spec) if use_visible else dict(spec, use_visible=False)
        R, t, inl, st, final, rep = PP.estimate_poses_mask_verified(*args, v_spec, return_verify=True, img_index=[1, 0], refine=refine, resize_method="crop_resize")
        C_ = len(names)
        assert [c[0] for c in calls] == ["forward"] + ["lm"] * (C_ - 1) + ["paste"] * (2 if use_visible else 1) + ["verify", "select"]      # ONE forward
        pastes = [c for c in calls if c[0] == "paste"]
        assert [c[5] for c in pastes] == ([1, 0] if use_visible else [1]) and all(c[1] == "SEG" and c[3] == (40, 48) and c[4] == "crop_resize" for c in pastes)
        assert all(np.array_equal(np.asarray(c[2]), np.asarray(padded)) for c in pastes)
        v, s = calls[-2], calls[-1]
        want_R = torch.cat([base_R + x for x in shift])
        want_t = torch.cat([base_t + x for x in shift])
        assert torch.equal(v[1], want_R) and torch.equal(v[2], want_t) and v[2].shape == (C_ * B, 3, 1)      # candidate-major, the stages' order
        assert np.array_equal(v[3], np.concatenate([K] * C_)) and v[4] == "VM" and v[5] == "masks1"
        kw = v[6]
        assert sorted(kw) == ["mask_ids", "mesh_ids", "status", "visible"] and kw["visible"] == ("masks0" if use_visible else None)
        assert list(kw["mask_ids"]) == [0, 1] * C_ and list(kw["mesh_ids"]) == [1, 0] * C_ and torch.equal(kw["status"], status.repeat(C_))
        assert s[1].shape == (C_, B) and s[2].shape == (C_, B) and torch.equal(s[3], want_R.view(C_, B, 3, 3)) and torch.equal(s[4], want_t.view(C_, B, 3, 1))
        assert torch.equal(R[0], base_R[0] + shift[-1]) and torch.equal(R[1], base_R[1]) and torch.equal(t[0], base_t[0] + shift[-1]) and torch.equal(t[1], base_t[1])
        assert inl == "inl" and st is status                                       # still the solver's
        assert rep["stages"] == names and rep["choice"].tolist() == [C_ - 1, 0] and rep["score"].shape == (C_, B) and rep["info"]["marker"] == "info"
        assert rep["full"] == "masks1" and rep["visible"] == ("masks0" if use_visible else None)
        assert len(PP.estimate_poses_mask_verified(*args, v_spec, img_index=[1, 0], refine=refine, resize_method="crop_resize")) == 5
    assert sorted(spec) == ["mesh_ids", "meshes"]                                  # the caller's dict is left alone
