"""CPU: row N27's rule (tests/paste_stages.py) cross-checked against torch's "nearest-exact" where the two agree, with the stated
counter-example where torch's float is wrong; properties that do not come from the restatement; every tampering of the restatement
caught by a named case; the refusals of the Python wrappers and of the C entry points (no launch, no device)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import paste_stages as PS

AGREE = (1, 2, 3, 5, 7, 31, 33, 63, 64, 65, 96, 100, 127, 128, 129, 200, 256, 300, 333, 480, 640)      # the issue's set


def _plane(Sh, Sw, seed):
    return np.random.default_rng(seed).normal(size=(Sh, Sw)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ 1. against torch
@pytest.mark.parametrize("S", [16, 64])
def test_restatement_equals_torch_nearest_exact_on_the_agreeing_sizes(S):
    plane = _plane(S, S, S)
    on = torch.from_numpy(PS.threshold(plane).astype(np.float32))[None, None]
    for k, rw in enumerate(AGREE):
        rh = AGREE[(k + 7) % len(AGREE)]
        x1, y1 = 3, 2
        H, W = rh + 5, rw + 7                              # the window lies wholly inside the frame
        got = PS.paste(plane, (x1, y1, x1 + rw, y1 + rh, rw, rh), H, W)
        want = np.zeros((H, W), np.uint8)
        want[y1:y1 + rh, x1:x1 + rw] = F.interpolate(on, size=(rh, rw), mode="nearest-exact")[0, 0].numpy().astype(np.uint8)
        assert np.array_equal(got, want), (S, rw, rh)


def test_torch_nearest_exact_is_wrong_at_rw_41_and_the_integer_rule_is_not():
    """(2 * 20 + 1) * 64 / (2 * 41) = 32 exactly: the float rule reads cell 31"""
    ours = PS.cells(0, 41, 0, 64, 41)
    src = torch.arange(64, dtype=torch.float32)[None, None, None, :]
    theirs = F.interpolate(src, size=(1, 41), mode="nearest-exact")[0, 0, 0].numpy().astype(np.int64)
    assert np.nonzero(ours != theirs)[0].tolist() == [20] and ours[20] == 32 and theirs[20] == 31
    assert (2 * 20 + 1) * 64 == 32 * (2 * 41)


# ------------------------------------------------------------------------------------------------------------ 2. properties
@pytest.mark.parametrize("Sh,Sw", [(16, 16), (8, 16), (64, 64)])
def test_unit_scale_is_a_translation_and_k_scale_is_k_by_k_blocks(Sh, Sw):
    plane = _plane(Sh, Sw, 3)
    on = PS.threshold(plane).astype(np.uint8)
    H, W, x1, y1 = 3 * Sh + 9, 3 * Sw + 11, 5, 4
    m = PS.paste(plane, (x1, y1, x1 + Sw, y1 + Sh, Sw, Sh), H, W)
    want = np.zeros((H, W), np.uint8)
    want[y1:y1 + Sh, x1:x1 + Sw] = on
    assert np.array_equal(m, want)
    for k in (2, 3):
        m = PS.paste(plane, (x1, y1, x1 + k * Sw, y1 + k * Sh, k * Sw, k * Sh), H, W)
        want = np.zeros((H, W), np.uint8)
        want[y1:y1 + k * Sh, x1:x1 + k * Sw] = np.kron(on, np.ones((k, k), np.uint8))
        assert np.array_equal(m, want), k


def test_empty_results_and_the_window_bound():
    ones = np.ones((16, 16), np.float32)
    H, W = 31, 33
    for win in ((40, 5, 60, 25, 20, 20), (-30, 5, -10, 25, 20, 20), (5, 31, 25, 51, 20, 20), (5, -25, 25, -5, 20, 20),      # off the frame
                (0, 0, 0, 0, 0, 0), (3, 3, 20, 20, 0, 17), (3, 3, 20, 20, 17, -1)):                                         # no roi
        m = PS.paste(ones, win, H, W)
        assert PS.area_box(m) == (0, [-1, -1, -1, -1]) and PS.rle(m) == [H * W], win
    m = PS.paste(-ones, (2, 2, 22, 22, 20, 20), H, W)                                                                       # an all-clear plane
    assert PS.area_box(m) == (0, [-1, -1, -1, -1])
    rng = np.random.default_rng(5)
    for _ in range(200):
        x1, y1 = (int(v) for v in rng.integers(-40, 40, 2))
        w, h, rw, rh = (int(v) for v in rng.integers(1, 80, 4))
        win = (x1, y1, x1 + w, y1 + h, rw, rh)
        m = PS.paste(ones, win, H, W)
        inside = np.zeros((H, W), bool)
        inside[max(y1, 0):max(min(y1 + h, H), 0), max(x1, 0):max(min(x1 + w, W), 0)] = True
        assert not m[~inside].any(), win
        # an all-set plane fills exactly where the crop read a real pixel
        lx, hx = max(x1, 0), min(x1 + w, W, x1 + rw)
        ly, hy = max(y1, 0), min(y1 + h, H, y1 + rh)
        assert int(m.sum()) == max(hx - lx, 0) * max(hy - ly, 0), win


def test_threshold_is_the_pinned_one():
    z0 = PS.Z0
    z = np.array([z0, np.nextafter(z0, np.float32(1)), np.nextafter(z0, np.float32(-1)), 0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0], np.float32)
    assert PS.threshold(z).tolist() == [False, True, False, False, False, False, True, False, True, False]
    # what the reference computes: sigmoid in fp32, then > 0.5
    assert (torch.sigmoid(torch.from_numpy(z)) > 0.5).tolist() == PS.threshold(z).tolist()


# ------------------------------------------------------------------------------------------------------------ 3. tamperings
def _threshold_plane():
    p = np.full((16, 16), -1.0, np.float32)
    p[4:9, 3:11] = PS.Z0
    p[9:12, 3:11] = 1.0
    return p


TAMPER_CASES = {
    # name -> (tampering, plane, window, H, W)
    "downsample_5": ("left_edge", _plane(16, 16, 11), (4, 6, 9, 11, 5, 5), 31, 33),
    "window_longer_than_roi": ("x2_only", np.ones((16, 16), np.float32), (2, 3, 20, 20, 10, 10), 31, 33),
    "threshold_plane": ("ge", _threshold_plane(), (1, 1, 29, 29, 28, 28), 31, 33),
    "non_square_plane": ("swapped", _plane(8, 16, 13), (3, 2, 43, 42, 40, 40), 50, 70),
}


@pytest.mark.parametrize("name", sorted(TAMPER_CASES))
def test_every_tampering_of_the_rule_is_caught_by_its_case(name):
    rule, plane, win, H, W = TAMPER_CASES[name]
    good, bad = PS.paste(plane, win, H, W), PS.paste(plane, win, H, W, rule=rule)
    assert good.any() and not np.array_equal(good, bad)
    for other in (r for r, *_ in TAMPER_CASES.values() if r != rule):          # (a case need not catch the others; it must be defined for them)
        PS.paste(plane, win, H, W, rule=other)


def test_row_major_ravel_is_caught():
    m = PS.paste(_plane(16, 16, 17), (3, 2, 27, 22, 24, 20), 31, 33)
    assert PS.rle(m) != PS.rle(m, order="C") and sum(PS.rle(m)) == 31 * 33
    first = np.zeros((3, 4), np.uint8)
    first[0, 0] = first[1, 0] = 1
    assert PS.rle(first) == [0, 2, 10] and PS.rle(first, order="C") == [0, 1, 3, 1, 7]


def test_pack_is_cp_coco_packs_layout():
    m = np.zeros((2, 70), np.uint8)
    m[0, 0] = m[0, 31] = m[0, 32] = m[1, 69] = 1
    assert PS.pack(m).view(np.uint32).tolist() == [[0x80000001, 1, 0], [0, 0, 1 << 5]]


# ------------------------------------------------------------------------------------------------------------ 4. refusals
def test_python_wrappers_refuse_without_a_device():
    from checkerpose_amd import coco_eval as CE
    from checkerpose_amd import postprocess as PP
    seg = torch.zeros(2, 2, 16, 16)
    boxes = [[1, 2, 10, 10], None]
    for fn in (PP.paste_masks, PP.paste_masks_rle):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(seg, boxes, (31, 33))
        with pytest.raises(NotImplementedError, match="warp_affine"):
            fn(seg, boxes, (31, 33), resize_method="crop_resize_by_warp_affine")
        with pytest.raises(NotImplementedError, match="unknown decoder type"):
            fn(seg, boxes, (31, 33), resize_method="stretch")
        for bad in (seg[0], seg.double(), torch.zeros(2, 2, 129, 16), torch.zeros(2, 2, 16, 0), np.zeros((2, 2, 16, 16), np.float32)):
            with pytest.raises(ValueError, match="seg"):
                fn(bad, boxes, (31, 33))
        for channel in (2, -1, 1.0, True, None):
            with pytest.raises(ValueError, match="channel"):
                fn(seg, boxes, (31, 33), channel=channel)
        with pytest.raises(ValueError, match="channel"):
            fn(seg[:, :1], boxes, (31, 33), channel=1)
        for size in ((0, 33), (31, 4097), (31,), 31, (31.5, 33), (31, 33, 3), None):
            with pytest.raises(ValueError, match="frame_size"):
                fn(seg, boxes, size)
        with pytest.raises(ValueError, match="boxes"):
            fn(seg, boxes[:1], (31, 33))
        with pytest.raises(ValueError, match="box"):
            fn(seg, [[1, 2, 3], None], (31, 33))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CE.segmentation_results(seg, boxes, (31, 33), 1, 2, 3, 0.5)
    with pytest.raises(NotImplementedError, match="warp_affine"):
        PP.estimate_poses_masks(None, torch.zeros(1, 40, 40, 3, dtype=torch.uint8), [], None, None, resize_method="crop_resize_by_warp_affine")
    packed = CE.PackedMasks(torch.zeros(1, 4, 1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32), 4, 4)
    with pytest.raises(RuntimeError):
        CE.unpack_masks(packed)


def test_estimate_poses_masks_runs_one_forward_and_pastes_its_seg(monkeypatch):
    """stubs in place of every device call: the forward runs once, its seg and the PADDED boxes reach paste_masks"""
    from checkerpose_amd import paste
    from checkerpose_amd import postprocess as PP
    from checkerpose_amd import preprocess as PRE
    forwards, pasted = [], []
    monkeypatch.setattr(PRE, "get_roi_batch", lambda *a, **k: "crops")
    monkeypatch.setattr(PP, "correspondences", lambda out, **k: ("p2d", "valid", None))
    monkeypatch.setattr(PP, "solve_pnp_ransac", lambda *a, **k: ("R0", "t0", "inl", "status"))
    monkeypatch.setattr(paste, "paste_masks", lambda *a: pasted.append(a) or "masks")

    def net(crops, _):
        forwards.append(crops)
        return ("roi", "xb", "yb", "seg", "xid", "yid")

    frames = torch.zeros(2, 40, 48, 3, dtype=torch.uint8)
    out = PP.estimate_poses_masks(net, frames, [[5, 5, 10, 10], None], "p3d", "K", channel=1, img_index=[1, 0], resize_method="crop_resize")
    assert out[:4] == ("R0", "t0", "inl", "status") and out[5] == "masks" and len(out) == 6 and forwards == ["crops"]
    (seg, padded, size, method, channel), = pasted
    assert seg == "seg" and size == (40, 48) and method == "crop_resize" and channel == 1
    assert padded[1] is None and np.array_equal(padded[0], PRE.padding_Bbox([5, 5, 10, 10], 1.5))
    assert PP.estimate_poses(net, frames, [[5, 5, 10, 10], None], "p3d", "K", img_index=[1, 0])[:4] == out[:4] and len(pasted) == 1


def test_c_entry_points_refuse_before_any_launch(lib):
    assert lib.cp_version() >= 237
    buf = C.create_string_buffer(4096 + 16)
    p = (C.addressof(buf) + 15) & ~15
    ok = [None, p, 2 * 64 * 64, 64, 64, p, 3, 480, 640, p, p, p]

    def call(name, *pairs):
        a = list(ok)
        if name == "cp_paste_rle_write":
            a[11] = 16
        for i, v in pairs:
            a[i] = v
        lib.cp_kernel_log_begin()
        rc = getattr(lib, name)(*a)
        assert lib.cp_kernel_log() == b""
        return rc

    for name in ("cp_paste_masks", "cp_paste_rle_count", "cp_paste_rle_write"):
        INVALID, ALIGN, RANGE = call(name, (1, None)), call(name, (1, p + 2)), call(name, (6, 1 << 24))
        assert (INVALID, ALIGN, RANGE) == (-1, -3, -4)
        ptrs = (1, 5, 9, 10) + ((11,) if name != "cp_paste_rle_write" else ())
        assert [call(name, (i, None)) for i in ptrs] == [INVALID] * len(ptrs)
        assert [call(name, (i, v)) for i, v in ((6, 0), (6, -1), (2, -1), (3, 0), (3, 129), (4, 0), (4, 129), (7, 0), (7, 4097), (8, 0), (8, 4097))] \
            == [INVALID] * 11
        assert [call(name, (i, p + 2)) for i in ptrs] == [ALIGN] * len(ptrs)
        assert call(name, (7, 0), (1, p + 2)) == INVALID and call(name, (6, 1 << 24), (1, p + 2)) == ALIGN
    assert call("cp_paste_rle_write", (9, p + 4)) == -3 and call("cp_paste_rle_write", (11, 0)) == -1
    lib.cp_kernel_log_begin()
    assert [lib.cp_coco_unpack(None, None, 2, 31, 33, p), lib.cp_coco_unpack(None, p, 2, 31, 33, None), lib.cp_coco_unpack(None, p, 0, 31, 33, p),
            lib.cp_coco_unpack(None, p, 2, 0, 33, p), lib.cp_coco_unpack(None, p, 2, 31, 0, p)] == [-1] * 5
    assert lib.cp_coco_unpack(None, p + 2, 2, 31, 33, p) == -3
    assert [lib.cp_coco_unpack(None, p, 2, 1 << 16, 1 << 15, p), lib.cp_coco_unpack(None, p, 1 << 24, 31, 33, p),
            lib.cp_coco_unpack(None, p, 1 << 23, 4096, 4096, p)] == [-4] * 3
    assert lib.cp_kernel_log() == b""
