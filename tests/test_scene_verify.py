"""CPU: row N31's rule in numpy (tests/scene_verify_stages.py) -- its identities on CPU renders, a hand count, its tamperings, what the
committed cases cover --, the library's host half with fake pointers, and the Python layer's refusals, defaults and
estimate_poses_scene_verified's routing with stubs (no device)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import icp_stages as I
from tests import scene_verify_stages as SV
from tests import verify_mask_stages as VM
from tests.pnp_stages import StageError


def _run(name):
    """a committed case on the CPU: (case, render_f32 renders, the rule's outputs); the first two cached by scene_verify_stages"""
    case = SV.make(name)
    D = SV.cpu_renders(case)
    return case, D, SV.reference(case, D)


def _col(out, key):
    return out["counts"][:, SV.COUNTS.index(key)].astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------- the rule
def test_hand_count_on_a_6_by_4_frame():
    """two 2 x 2 squares sharing one column on a 6 x 4 frame, K = identity-like (fx = fy = 1, cx = cy = 0): A at depth 10 over columns
    1..2, B at depth 12 over columns 2..3, rows 1..2.  Slot order A, B."""
    K = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    A, B = np.zeros((4, 6), np.float32), np.zeros((4, 6), np.float32)
    A[1:3, 1:3], B[1:3, 2:4] = 10.0, 12.0
    assert SV.slots_of([0, 1, 0, 5, 1, 0], 2).tolist() == [0, 0, 1, -1, 1, 2]
    ren, owner = SV.composite([(0, A), (1, B)])
    assert ren[1].tolist() == [0, 10, 10, 12, 0, 0] and owner[1].tolist() == [-1, 0, 0, 1, -1, -1] and not ren[0].any() and not ren[3].any()
    # at pixel (2, 1): dist = depth * sqrt(1 + 4 + 1): 12 sqrt(6) - 10 sqrt(6) = 4.899 in float32
    visA, visB0, visB5 = (SV.predicted_visible(A, ren, K, 0.0), SV.predicted_visible(B, ren, K, 0.0), SV.predicted_visible(B, ren, K, 5.0))
    assert visA.sum() == 4 and np.array_equal(visA, A > 0)
    assert visB0.sum() == 2 and visB0[1].tolist() == [False, False, False, True, False, False]          # column 2 is hidden
    assert visB5.sum() == 3 and visB5[1, 2] and not visB5[2, 2]                                        # 4.899 <= 5; at (2, 2) it is 36 - 30 = 6
    assert SV.predicted_visible(B, ren, K, 4.8).sum() == 2 and SV.predicted_visible(B, ren, K, 6.0).sum() == 4
    assert SV.predicted_visible(B, ren, K, 6.0, ("lt_visible",)).sum() == 3                              # exactly delta: <= keeps it, < does not
    assert SV.predicted_visible(B, ren, K, 2.0, ("depth_not_dist",)).sum() == 4                         # on depths the difference is 2
    assert SV.box_of(visB0) == [3, 1, 3, 2] and SV.box_of(np.zeros((4, 6), bool)) == [-1] * 4
    # the tie: the same square twice -- both fully visible, the earlier slot owns
    ren2, own2 = SV.composite([(0, A), (1, A)])
    assert np.array_equal(ren2, A) and own2[1, 1] == 0 and SV.composite([(0, A), (1, A)], ("tie_later",))[1][1, 1] == 1
    assert SV.predicted_visible(A, ren2, K, 0.0).sum() == 4 and SV.predicted_visible(A, ren2, K, 0.0, ("lt_visible",)).sum() == 0
    # B against a visible mask that holds column 3 alone and a full mask that holds its square: everything by hand
    f = SV.finish(n_model=4, n_pvis=2, n_inter=4, n_vis_in=2, n_pvis_in=2, n_mask=4, n_vis=2)
    assert (f["iou"], f["cover"], f["iou_vis"], f["visib_fract"], f["score"], f["ok"]) == (1.0, 1.0, 1.0, 0.5, 1.0, True)
    f = SV.finish(4, 2, 4, 3, 1, 4, 3)                                            # the network sees three pixels, one of the predicted two
    assert f["iou_vis"] == 1.0 / 4.0 and f["cover"] == 1.0 and f["visib_fract"] == 0.5
    f = SV.finish(4, 0, 4, 0, 0, 4, 0)                                            # fully hidden under an empty visible mask
    assert np.isnan(f["iou_vis"]) and np.isnan(f["score"]) and not f["ok"] and f["iou"] == 1.0 and np.isnan(f["cover"]) and f["visib_fract"] == 0.0
    f = SV.finish(4, 0, 4, 2, 0, 4, 2)                                            # fully hidden under a non-empty one
    assert f["iou_vis"] == 0.0 and f["ok"]
    f = SV.finish(0, 0, 0, 0, 0, 7, 5, counted=False)
    assert all(np.isnan(f[k]) for k in SV.QUOTIENTS) and not f["ok"]
    f = SV.finish(0, 0, 0, 0, 0, 7, 5)                                            # wholly off the frame: exact zeros, no fraction
    assert f["iou"] == 0.0 and f["iou_vis"] == 0.0 and f["ok"] and np.isnan(f["visib_fract"])


@pytest.mark.parametrize("name", list(SV.CASES))
def test_identities_on_cpu_renders(name):
    case, D, out = _run(name)
    SV.check_case(case, D, out)
    slots = case.slots()
    n = {k: _col(out, k) for k in SV.COUNTS}
    assert np.array_equal(out["slot"], slots)
    for b in range(case.P):
        if not case.counted(b):
            assert not out["counts"][b, :5].any() and out["counts"][b, 7] == 0 and (out["box"][b] == -1).all() and (out["box_pvis"][b] == -1).all()
            assert not out["ok"][b] and all(np.isnan(out[k][b]) for k in SV.QUOTIENTS)
            continue
        m, img = case.mask_of(b), int(case.image_ids[b])
        sil = D[b] > 0
        # row N28's numbers, untouched by the scene
        alone = VM.finish(*VM.counts_of(D[b], case.full[m], case.visible[m]), int(case.full[m].sum()), int(case.visible[m].sum()))
        assert n["n_model"][b] == sil.sum() and n["n_inter"][b] == (sil & case.full[m]).sum() and n["n_vis_in"][b] == (sil & case.visible[m]).sum()
        assert np.array_equal(np.array([out["iou"][b], out["cover"][b]]).view(np.uint64), np.array([alone[1], alone[2]]).view(np.uint64))
        assert 0 <= n["n_pvis_in"][b] <= min(n["n_pvis"][b], n["n_vis_in"][b]) and n["n_pvis"][b] <= n["n_model"][b]
        assert n["n_hidden_seen"][b] == n["n_vis_in"][b] - n["n_pvis_in"][b] >= 0
        pv = ((out["visib_bits"][img].view(np.uint32) >> np.uint32(slots[b])) & 1).astype(bool)
        fb = ((out["full_bits"][img].view(np.uint32) >> np.uint32(slots[b])) & 1).astype(bool)
        assert np.array_equal(fb, sil) and pv.sum() == n["n_pvis"][b] and not (pv & ~sil).any() and out["box_pvis"][b].tolist() == SV.box_of(pv)
        if out["ok"][b]:
            assert 0.0 <= out["score"][b] <= 1.0 and out["score"][b] == out["iou_vis"][b]
    # the front-most pose of every pixel is visible there; the owner is the earliest slot at the composite's depth
    own = out["owner"]
    for img in range(case.n_images):
        bits = out["visib_bits"][img].view(np.uint32)
        has = own[img] >= 0
        assert np.array_equal(has, out["full_bits"][img] != 0)
        assert (((bits[has] >> own[img][has].astype(np.uint32)) & 1) == 1).all()


@pytest.mark.parametrize("name", list(SV.CASES))
def test_every_pose_alone_in_its_image(name):
    """with every pose in an image of its own nothing occludes: n_pvis == n_model, iou_vis == the IoU of the silhouette with V"""
    case = SV.make(name)
    D = SV.cpu_renders(case)
    solo = SV.SceneCase(case.name + "_solo", case.size, case.meshes, case.mesh_ids, case.K, case.R, case.t, np.arange(case.P), case.P, case.full,
                        case.visible, case.delta, mask_ids=case.mask_ids, status=case.status)
    out = SV.reference(solo, D)
    assert np.array_equal(_col(out, "n_pvis"), _col(out, "n_model")) and np.array_equal(_col(out, "n_pvis_in"), _col(out, "n_vis_in"))
    assert not _col(out, "n_hidden_seen").any() and np.array_equal(out["box"], out["box_pvis"]) and (out["slot"] == 0).all()
    for b in range(case.P):
        if solo.counted(b):
            m = case.mask_of(b)
            want = VM.finish(*VM.counts_of(D[b], case.visible[m]), int(case.visible[m].sum()), 0)      # the IoU of the silhouette with V
            assert np.array_equal(np.array([out["iou_vis"][b]]).view(np.uint64), np.array([want[1]]).view(np.uint64))


def test_truth_poses_under_their_own_scene_give_one():
    for name in ("occl_a", "occl_b_d0", "occl_b_d15", "occl_b_big", "select_a"):
        case, D, out = _run(name)
        rows = [0, 1] if case.cand is None else [2, 3, 4, 5]
        for k in ("iou", "cover", "iou_vis", "score"):
            assert (out[k][rows] == 1.0).all(), (name, k)
        assert not _col(out, "n_hidden_seen")[rows].any()
    case, D, out = _run("crowd32_b")
    assert (out["iou_vis"] == 1.0).all() and (out["iou"] == 1.0).all() and out["ok"].all()


@pytest.mark.parametrize("tamper", SV.TAMPERINGS)
def test_tamperings_are_caught(tamper):
    """ONE rule changed: the named case's outputs change, and check_case refuses the changed outputs"""
    case, D, good = _run(SV.CAUGHT_BY[tamper])
    bad = SV.reference(case, D, (tamper,))
    assert any(not np.array_equal(good[k], bad[k], equal_nan=True) for k in good if good[k] is not None)
    with pytest.raises(StageError):
        SV.check_case(case, D, bad)


def test_tamperings_listed():
    assert set(SV.TAMPERINGS) == {"tie_later", "lt_visible", "depth_not_dist", "uncounted_occludes", "swap_fv", "pvis_in_over_model",
                                  "ignore_mask_ids", "ignore_image_ids"} == set(SV.CAUGHT_BY)
    assert all(n in SV.CASES for n in SV.CAUGHT_BY.values())


def test_what_the_cases_cover():
    cases = {n: SV.make(n) for n in SV.CASES}
    assert {c.size for c in cases.values()} == {(96, 80), (70, 50)}
    # a. partly hidden; the occluder has n_hidden_seen > 0 when the order is flipped
    case, D, o = _run("occl_a")
    n = {k: _col(o, k) for k in SV.COUNTS}
    assert 0 < n["n_pvis"][1] < n["n_model"][1] and n["n_hidden_seen"][1] == 0                        # the torus behind the box, as the network sees it
    assert n["n_hidden_seen"][2] > 0 and n["n_pvis"][2] < n["n_model"][2] and o["iou"][2] == 1.0 and o["cover"][2] == 1.0      # the box: row N28 sees nothing
    assert o["iou_vis"][2] < 0.75 and o["iou_vis"][3] < 0.6 and 0.6 < o["iou"][3] < 0.8               # the torus 15 % nearer: in front of the box
    assert case.image_ids.tolist() == [0, 0, 1, 1, 2, 2] and case.mesh_ids.tolist()[4:] == [1, 0]     # image 2: the torus first
    assert n["n_hidden_seen"][5] > 0 and 0 < o["iou_vis"][4] < o["iou"][4] and 0.85 < o["iou_vis"][5] < 1 == o["iou"][5]      # 6 % nearer: interpenetrating
    # b. fully hidden under an empty and a non-empty visible mask;  c. the tie
    case, D, o = _run("hidden_tie_a")
    n = {k: _col(o, k) for k in SV.COUNTS}
    assert n["n_pvis"][2] == n["n_pvis"][3] == 0 < n["n_model"][2] == n["n_model"][3]
    assert not case.visible[1].any() and np.isnan(o["iou_vis"][2]) and not o["ok"][2] and o["iou"][2] == 1.0 and o["visib_fract"][2] == 0.0
    assert case.visible[2].any() and o["iou_vis"][3] == 0.0 and o["ok"][3] and n["n_hidden_seen"][3] == n["n_model"][3]
    assert np.array_equal(case.R[0], case.R[1]) and np.array_equal(case.t[0], case.t[1]) and case.delta == 0.0
    assert n["n_pvis"][0] == n["n_model"][0] == n["n_pvis"][1] == n["n_model"][1] > 0 and o["iou_vis"][0] == o["iou_vis"][1] == 1.0
    assert set(np.unique(o["owner"][0])) == {-1, 0} and o["slot"].tolist() == [0, 1, 2, 3]
    # d. exactly 32 in one image;  e. interleaved;  a 33rd is not counted and occludes nothing
    case, D, o = _run("crowd32_b")
    ids = case.image_ids
    assert (ids == 0).sum() == 32 and (ids == 1).sum() == 4 and o["slot"][ids == 0].tolist() == list(range(32)) and o["slot"][ids == 1].tolist() == [0, 1, 2, 3]
    assert sorted(np.nonzero(ids == 1)[0].tolist()) == [3, 11, 20, 30] and o["ok"].all() and case.mask_ids is None and case.N == case.P
    part = SV.partly_hidden(case, D)
    assert (ids[part] == 0).sum() >= 4 and (ids[part] == 1).sum() >= 2 and (o["visib_bits"][0].view(np.uint32) >> 31).any()
    c33, D33, o33 = _run("crowd33_b")
    assert c33.P == 37 and o33["slot"][36] == 32 and not c33.counted(36) and c33.rendered(36) and (D33[36] > 0).sum() > 500
    assert np.array_equal(o33["counts"][:36], o["counts"]) and np.array_equal(o33["iou_vis"][:36], o["iou_vis"]) and np.isnan(o33["score"][36])
    # f. per-pose K, several meshes, shared and permuted mask ids;  g. partly / wholly outside;  i. the mask kinds
    case, D, o = _run("mixed_b")
    n = {k: _col(o, k) for k in SV.COUNTS}
    assert case.K.ndim == 3 and len(set(case.mesh_ids.tolist())) == 3 and len(set(case.mask_ids.tolist())) < case.P
    assert case.mask_ids.tolist() != sorted(case.mask_ids.tolist()) and case.N == 5 != case.P
    assert np.nonzero((D[2] > 0).any(0))[0].max() == 69 and 0 < n["n_model"][2] and o["box"][2][2] == 69      # cut at the right edge
    assert case.rendered(3) and n["n_model"][3] == 0 and o["ok"][3] and o["iou_vis"][3] == 0.0 and (o["box"][3] == -1).all()
    assert not case.full[0].any() and case.full[1].all() and case.full[2].sum() == 1 and case.full[2][:, 69].any()
    assert np.array_equal(case.full[3], VM.checkerboard(case.size, 2)) and n["n_inter"][2] == n["n_model"][2] and o["iou"][4] == o["iou_vis"][4] == 0.0 and o["ok"][4]
    assert 0 < n["n_pvis"][0] < n["n_model"][0]
    # h. every way of being uncounted, in front of a counted pose that comes out as if alone
    case, D, o = _run("uncounted_a")
    assert len(SV.WAYS) == 7 and case.P == 15
    assert [case.counted(b) for b in range(0, 14, 2)] == [False] * 7 and all(case.counted(b) for b in range(1, 15, 2)) and case.counted(14)
    assert not case.rendered(0) and not case.rendered(2) and not case.rendered(4) and not case.rendered(6)
    assert all(case.rendered(b) and (D[b] > 0).sum() > 1000 for b in (8, 10, 12))                      # rendered, in front, yet not counted
    assert case.mask_ids[8] >= case.N and case.status[10] == 0 and case.image_ids[12] >= case.n_images and o["slot"][12] == -1
    assert all(((D[8] > 0) & (D[b] > 0) & (D[8] < np.where(D[b] > 0, D[b], 1e9))).sum() > 300 for b in (9,))      # it would hide the torus
    for b in range(1, 14, 2):
        assert np.array_equal(o["counts"][b], o["counts"][14]) and np.array_equal(o["box_pvis"][b], o["box_pvis"][14])
        assert all(np.array_equal(o[k][b:b + 1].view(np.uint64), o[k][14:15].view(np.uint64)) for k in SV.QUOTIENTS)
        assert o["slot"][b] == (0 if b == 13 else 1)
    assert 0 < o["iou_vis"][14] < 1 and o["visib_fract"][14] == 1.0
    # j. delta = 0 and a delta beyond the scene's depth range
    d0, big = _run("occl_b_d0"), _run("occl_b_big")
    assert d0[0].delta == 0.0 and big[0].delta > 1e5 and np.array_equal(_col(big[2], "n_pvis"), _col(big[2], "n_model"))
    assert (_col(d0[2], "n_pvis") < _col(d0[2], "n_model")).sum() >= 4 and (_col(d0[2], "n_pvis") <= _col(_run("occl_b_d15")[2], "n_pvis")).all()
    # k. candidate-major with an exact score tie
    case, D, o = _run("select_a")
    s = o["score"].reshape(case.cand)
    assert case.cand == (3, 2) and o["choice"].tolist() == [1, 1] and (s[1] == s[2]).all() and (s[1] > s[0]).all()
    assert case.image_ids.tolist() == [c * 1 + 0 for c in range(3) for _ in range(2)]


# ------------------------------------------------------------------------------------------------------------- the library
def test_abi_refusals():
    """the library on a CPU box: the new symbols resolve, the scratch sizing, refusals with fake pointers (nothing launches)"""
    from checkerpose_amd import _abi
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import verify_scene as M
    lib = _abi.load()
    assert lib.cp_version() >= 241
    assert lib.cp_verify_scene_mask_scratch_bytes(3, 64, 2) == 3 * 192 + 3 * 64 * 16 + 2 * 128 and lib.cp_verify_scene_mask_scratch_bytes(0, 64, 1) == 0
    assert lib.cp_verify_scene_mask_scratch_bytes(3, -1, 1) == 0 and lib.cp_verify_scene_mask_scratch_bytes(3, 64, 0) == 0
    assert lib.cp_verify_scene_mask_scratch_bytes(1, 0, 1) == 192 + 128
    assert M.VERIFY_SCENE_COUNTS == SV.COUNTS and M.VERIFY_SCENE_MAX_PIXELS == 1 << 24 and M.VERIFY_SCENE_MAX_POSES == SV.MAX_POSES == 32
    assert PP.verify_scene_mask is M.verify_scene_mask and PP.estimate_poses_scene_verified is M.estimate_poses_scene_verified
    buf = C.create_string_buffer(4096 + 16)
    p = (C.addressof(buf) + 15) & ~15
    d = C.c_double
    #       0     1  2  3  4  5  6  7  8  9     10 11 12 13 14    15 16  17  18 19 20    21      22 23 24 25 26 27 28 29 30 31 32 33    34    35
    ok_a = [None, p, p, 0, p, p, p, p, 1, None, p, p, p, p, None, 3, 80, 96, p, 2, None, d(1.0), 3, 8, p, p, p, p, p, p, p, p, p, None, None, p]

    def a_with(*pairs):
        a = list(ok_a)
        for i, v in pairs:
            a[i] = v
        lib.cp_kernel_log_begin()
        rc = lib.cp_verify_scene_mask(*a)
        assert lib.cp_kernel_log() == b""                                          # nothing was launched
        return rc

    INVALID, ALIGN, RANGE = a_with((1, None)), a_with((1, p + 4)), a_with((16, 4097), (17, 4096))
    assert len({0, INVALID, ALIGN, RANGE}) == 4
    nulls = (2, 4, 5, 6, 7, 10, 11, 12, 13, 18, 24, 25, 26, 27, 28, 29, 30, 31, 32, 35)
    assert [a_with((i, None)) for i in nulls] == [INVALID] * len(nulls)
    assert [a_with((8, 0)), a_with((8, 2)), a_with((23, 0)), a_with((3, 4)), a_with((16, 0)), a_with((17, 0)), a_with((22, 0)), a_with((22, -2))] == [INVALID] * 8
    assert [a_with((15, 0)), a_with((15, -1)), a_with((15, 2)), a_with((15, 4)), a_with((19, 0)), a_with((19, -3))] == [INVALID] * 6      # NM, I
    assert [a_with((33, p)), a_with((34, p))] == [INVALID] * 2                                                                # one plane without the other
    assert [a_with((21, d(-1.0))), a_with((21, d(float("nan")))), a_with((21, d(float("inf")))), a_with((21, d(1e39)))] == [INVALID] * 4
    assert a_with((21, d(0.0)), (16, 4097), (17, 4096)) == RANGE                                                              # delta = 0 is no refusal
    assert a_with((15, 4), (14, p), (16, 4097), (17, 4096)) == RANGE                                                          # with ids NM != P is no refusal
    al = [(35, p + 8), (2, p + 4), (27, p + 4), (28, p + 4), (29, p + 4), (30, p + 4), (31, p + 4), (4, p + 2), (9, p + 2), (10, p + 2), (11, p + 2),
          (12, p + 2), (13, p + 2), (14, p + 2), (18, p + 2), (20, p + 2), (24, p + 2), (25, p + 2), (26, p + 2)]
    assert [a_with(x) for x in al] == [ALIGN] * len(al)
    assert a_with((33, p + 2), (34, p)) == ALIGN and a_with((33, p), (34, p + 2)) == ALIGN
    assert a_with((16, 0), (35, p + 8)) == INVALID and a_with((16, 4097), (17, 4096), (35, p + 8)) == ALIGN                     # the classes' order
    assert [a_with((16, 1), (17, (1 << 24) + 1)), a_with((16, 4096), (17, 4096), (22, 1 << 12), (15, 1 << 12)), a_with((16, 4096), (17, 4096), (19, 1 << 12)),
            a_with((22, 1 << 20), (15, 1 << 20), (23, 1 << 12))] == [RANGE] * 4


# ------------------------------------------------------------------------------------------------------------- the Python layer
def _host_args():
    from checkerpose_amd.coco_eval import PackedMasks
    from checkerpose_amd.metric import MeshSet
    v, f = I.mesh_arrays(("box",))
    ms = MeshSet.from_arrays(v, faces=f)
    z = lambda: PackedMasks(torch.zeros(1, 80, 3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.full((1, 4), -1, dtype=torch.int32), 80, 96)      # noqa: E731
    return dict(R=torch.eye(3, dtype=torch.float64)[None], t=torch.tensor([[0.0, 0.0, 300.0]], dtype=torch.float64), cam_K=torch.from_numpy(I.K_A),
                meshes=ms, full=z(), visible=z(), image_ids=[0], delta=15.0)


def test_defaults_and_refusals():
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd.coco_eval import PackedMasks
    sig = inspect.signature(PP.verify_scene_mask)
    assert str(sig) == ("(R, t, cam_K, meshes, full, visible, image_ids, delta, mask_ids=None, mesh_ids=None, status=None, n_images=None, "
                        "return_planes=False)")
    assert sig.parameters["delta"].default is inspect.Parameter.empty and sig.parameters["image_ids"].default is inspect.Parameter.empty
    assert str(inspect.signature(PP.estimate_poses_scene_verified)) == "(net, frames, Bboxes, p3d_xyz, cam_K, verify, return_verify=False, **estimate_kwargs)"
    a = _host_args()
    for bad in (None, torch.zeros(1, 80, 3, dtype=torch.int32), "masks"):
        with pytest.raises(ValueError, match="full"):
            PP.verify_scene_mask(**dict(a, full=bad))
        with pytest.raises(ValueError, match="visible"):
            PP.verify_scene_mask(**dict(a, visible=bad))
    z = lambda n, h, w: PackedMasks(torch.zeros(n, h, (w + 31) // 32, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), None, h, w)      # noqa: E731
    for other in (z(2, 80, 96), z(1, 80, 95), z(1, 79, 96)):
        with pytest.raises(ValueError, match="visible"):
            PP.verify_scene_mask(**dict(a, visible=other))
    with pytest.raises(ValueError, match="no masks"):
        PP.verify_scene_mask(**dict(a, full=z(0, 80, 96), visible=z(0, 80, 96)))
    with pytest.raises(ValueError, match="2\\^24"):
        PP.verify_scene_mask(**dict(a, full=z(1, 4097, 4096), visible=z(1, 4097, 4096)))
    for bad in (-1.0, float("nan"), float("inf"), None, "15", True):
        with pytest.raises(ValueError, match="delta"):
            PP.verify_scene_mask(**dict(a, delta=bad))
    with pytest.raises(ValueError, match="image_ids"):
        PP.verify_scene_mask(**dict(a, image_ids=None))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # well-formed arguments on the host: still no fallback
        PP.verify_scene_mask(**a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.verify_scene_mask(**dict(a, delta=0, return_planes=True))


def test_public_functions():
    """the new functions live in checkerpose_amd/verify_scene.py and are re-exported: postprocess.py itself defines what it defined"""
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import verify_scene as M
    own = {n for n, f in vars(PP).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == PP.__name__}
    assert "verify_scene_mask" not in own and "estimate_poses_scene_verified" not in own and {"verify_poses", "select_poses"} <= own
    assert {n for n, f in vars(M).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == M.__name__} == \
        {"verify_scene_mask", "estimate_poses_scene_verified"}


def test_verify_values():
    from checkerpose_amd import postprocess as PP
    frames, p3d, K = torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(8, 3), torch.eye(3)
    for bad in (None, "yes", dict(), dict(meshes=None), dict(delta=1.0), dict(mesh_ids=[0], delta=1.0)):
        with pytest.raises(ValueError, match="verify"):
            PP.estimate_poses_scene_verified(None, frames, [], p3d, K, bad)
    for key in ("image_ids", "status", "mask_ids"):
        with pytest.raises(ValueError, match="must not name"):
            PP.estimate_poses_scene_verified(None, frames, [], p3d, K, {"meshes": None, "delta": 1.0, key: [0]})
    for extra in ("use_visible", "depth", "tau", "weight"):
        with pytest.raises(ValueError, match="unknown"):
            PP.estimate_poses_scene_verified(None, frames, [], p3d, K, {"meshes": None, "delta": 1.0, extra: 1.0})
    ok = dict(meshes=None, delta=1.0)
    with pytest.raises(NotImplementedError, match="warp_affine"):
        PP.estimate_poses_scene_verified(None, frames, [], p3d, K, ok, resize_method="crop_resize_by_warp_affine")
    with pytest.raises(ValueError, match="refine"):                              # estimate_poses' own refusals hold
        PP.estimate_poses_scene_verified(None, frames, [], p3d, K, ok, refine="gn")
    with pytest.raises(TypeError):
        PP.estimate_poses_scene_verified(None, frames, [], p3d, K, ok, no_such_keyword=1)
    two = torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="at most 32"):                          # 33 crops of one frame
        PP.estimate_poses_scene_verified(None, two, [[0, 0, 2, 2]] * 33, p3d, K, ok, img_index=[1] * 33)
    with pytest.raises(ValueError, match="img_index"):
        PP.estimate_poses_scene_verified(None, two, [[0, 0, 2, 2]] * 2, p3d, K, ok, img_index=[0, 2])


def test_estimate_poses_scene_verified_routes(monkeypatch):
    """ONE forward, the two pastes, the candidates' order, the image-id arithmetic, the ONE verify_scene_mask and ONE select_poses call
    with their arguments and the gather, with stubs in place of every device call"""
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import preprocess as PRE
    B = 3
    calls = []
    base_R = torch.arange(B * 9, dtype=torch.float64).reshape(B, 3, 3)
    base_t = torch.arange(B * 3, dtype=torch.float64).reshape(B, 3, 1)
    status = torch.tensor([1, 0, 1], dtype=torch.int32)
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

    def verify(R, t, K, meshes, full, visible, image_ids, delta, **kw):
        calls.append(("verify", R, t, K, meshes, full, visible, image_ids, delta, kw))
        P = R.shape[0]
        return torch.arange(P, dtype=torch.float64), dict(ok=torch.ones(P, dtype=torch.bool), marker="info")

    def select(score, ok, R, t):
        calls.append(("select", score, ok, R, t))
        choice = torch.tensor([score.shape[0] - 1, 0, 0], dtype=torch.int32)
        return choice, R[choice.long(), torch.arange(B)], t[choice.long(), torch.arange(B)]

    monkeypatch.setattr(PP, "paste_masks", paste)
    monkeypatch.setattr(PP, "verify_scene_mask", verify)
    monkeypatch.setattr(PP, "select_poses", select)
    frames = torch.zeros(2, 40, 48, 3, dtype=torch.uint8)
    K = np.stack([I.K_A, I.K_B, I.K_A])
    boxes = [[5, 5, 10, 10], [6, 6, 10, 10], [7, 7, 10, 10]]
    args = (net, frames, boxes, "p3d", K)
    spec = dict(meshes="VM", mesh_ids=[1, 0, 1], delta=7.5)
    padded = [PRE.padding_Bbox(b, 1.5) for b in boxes]
    for refine, names, shift in ((None, ("solver",), (0.0,)), ("lm", ("solver", "lm"), (0.0, 100.0))):
        del calls[:]
        R, t, inl, st, final, rep = PP.estimate_poses_scene_verified(*args, dict(spec), return_verify=True, img_index=[1, 0, 1], refine=refine, resize_method="crop_resize")
        C_ = len(names)
        assert [c[0] for c in calls] == ["forward"] + ["lm"] * (C_ - 1) + ["paste", "paste", "verify", "select"]      # ONE forward, both pastes
        pastes = [c for c in calls if c[0] == "paste"]
        assert [c[5] for c in pastes] == [1, 0] and all(c[1] == "SEG" and c[3] == (40, 48) and c[4] == "crop_resize" for c in pastes)
        assert all(np.array_equal(np.asarray(c[2]), np.asarray(padded)) for c in pastes)
        v, s = calls[-2], calls[-1]
        want_R = torch.cat([base_R + x for x in shift])
        want_t = torch.cat([base_t + x for x in shift])
        assert torch.equal(v[1], want_R) and torch.equal(v[2], want_t) and v[2].shape == (C_ * B, 3, 1)      # candidate-major, the stages' order
        assert np.array_equal(v[3], np.concatenate([K] * C_)) and v[4] == "VM" and v[5] == "masks1" and v[6] == "masks0" and v[8] == 7.5
        assert list(v[7]) == [c * 2 + i for c in range(C_) for i in (1, 0, 1)]     # image_ids = c * n_frames + img_index
        kw = v[9]
        assert sorted(kw) == ["mask_ids", "mesh_ids", "n_images", "status"] and kw["n_images"] == C_ * 2
        assert list(kw["mask_ids"]) == [0, 1, 2] * C_ and list(kw["mesh_ids"]) == [1, 0, 1] * C_ and torch.equal(kw["status"], status.repeat(C_))
        assert s[1].shape == (C_, B) and s[2].shape == (C_, B) and torch.equal(s[3], want_R.view(C_, B, 3, 3)) and torch.equal(s[4], want_t.view(C_, B, 3, 1))
        assert torch.equal(R[0], base_R[0] + shift[-1]) and torch.equal(R[1], base_R[1]) and torch.equal(t[2], base_t[2])
        assert inl == "inl" and st is status                                       # still the solver's
        assert rep["stages"] == names and rep["choice"].tolist() == [C_ - 1, 0, 0] and rep["score"].shape == (C_, B) and rep["info"]["marker"] == "info"
        assert rep["full"] == "masks1" and rep["visible"] == "masks0" and list(rep["image_ids"]) == list(v[7])
        assert len(PP.estimate_poses_scene_verified(*args, dict(spec), img_index=[1, 0, 1], refine=refine, resize_method="crop_resize")) == 5
    del calls[:]                                                                   # one frame, no img_index: every crop in image 0, scene c = image c
    PP.estimate_poses_scene_verified(net, frames[0], boxes, "p3d", I.K_A, dict(spec), refine="lm")
    v = [c for c in calls if c[0] == "verify"][0]
    assert list(v[7]) == [0, 0, 0, 1, 1, 1] and v[9]["n_images"] == 2 and np.array_equal(v[3], I.K_A)
    assert sorted(spec) == ["delta", "mesh_ids", "meshes"]                         # the caller's dict is left alone
