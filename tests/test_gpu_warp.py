"""Row N21 on the device: cp_warp_affine_u8 / cp_warp_mask_bits against the numpy restatement (tests/warp_stages.py), byte for byte, and
"crop_resize_by_warp_affine" through every call that takes a resize_method.  Small shapes: 2 frames of 48 x 64, C in {1, 3, 4}, outputs
8 x 8 and 16 x 12, at most 12 crops.  Every comparison is equality.

  bytes        warp_affine == warp_stages.warp for both interpolations: random matrices with rotation and anisotropic scale, inverse_map,
               every C, an img_index with repeats, a None entry and a crop wholly off the frame (both all zero)
  properties   the slices, half-pixel means, quarter turns, the bilinear bound and the hand-worked double roundings of tests/test_warp.py
  methods      where max(bw, bh) == crop_size with even sides and integer centres, the new method equals crop_square_resize
  mask bits    get_roi_mask_bits == get_roi_batch(INTER_NEAREST) of the expanded 0 / 255 mask, several bits of one plane
  batches      make_training_batch / scene_training_batch (is_train=False, and with an augment plan): crops == get_roi_batch of the same
               boxes, labels == encode_targets on get_final_Bbox's boxes; the rects handed to the augmentation hold every pixel read
  poses        estimate_poses runs with the new method and returns the shapes the square method returns
  refusals     C = 5, null pointers, B with a mismatched img_index, the 2^20 range"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import warp_stages as WS

pytestmark = pytest.mark.gpu

NEW = "crop_resize_by_warp_affine"
H, W = 48, 64
DEV = "cuda:0"


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _frames(C_):
    return np.random.default_rng(50 + C_).integers(1, 256, size=(2, H, W, C_), dtype=np.uint8)


def _rot(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


def _matrices(rng, n, out_w, out_h):
    """forward matrices dst = M . src: rotation x anisotropic scale (shear through the order) about a source point near the frame"""
    mats = []
    for _ in range(n):
        L = _rot(rng.uniform(-180, 180)) @ np.diag(rng.uniform(0.15, 1.6, size=2)) @ _rot(rng.uniform(-30, 30))
        c = np.array([rng.uniform(-6, W + 6), rng.uniform(-6, H + 6)])
        mats.append(np.hstack([L, (np.array([out_w / 2.0, out_h / 2.0]) - L @ c)[:, None]]))
    return mats


@pytest.mark.parametrize("C_", [1, 3, 4])
@pytest.mark.parametrize("out_size", [(8, 8), (16, 12)])
def test_bytes_equal_the_restatement(C_, out_size):
    from checkerpose_amd import preprocess as PP
    frames = _frames(C_)
    fr = _up(frames)
    rng = np.random.default_rng(1000 * C_ + out_size[0])
    mats = _matrices(rng, 10, *out_size)
    mats[3] = None                                                                            # no box
    mats[7] = np.array([[1.0, 0.0, 300.0], [0.0, 1.0, -200.0]])                               # wholly off the frame
    mats.append(np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 2.0]]))                                 # singular: D = 0 -> every pixel reads (0, 0)
    idx = [0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0]
    for interp in (PP.INTER_NEAREST, PP.INTER_LINEAR):
        got = PP.warp_affine(fr, mats, out_size if out_size[0] != out_size[1] else out_size[0], interp, img_index=idx)
        want = WS.warp_batch(frames, mats, out_size, interp, img_index=idx)
        assert got.shape == (11, out_size[1], out_size[0], C_) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), want), (C_, out_size, interp)
        assert not want[3].any() and not want[7].any() and want[[0, 1, 2, 4, 5, 6, 8, 9]].any()
        inv = [None if m is None else WS.invert(m).reshape(2, 3) for m in mats[:10]]          # the same maps handed over as inverse maps
        got_inv = PP.warp_affine(fr, inv, out_size, interp, inverse_map=True, img_index=idx[:10])
        assert np.array_equal(got_inv.cpu().numpy(), want[:10]), (C_, out_size, interp, "inverse_map")
    # one image for all crops, image b for crop b, out= given, a (H, W, C) image, a tensor of matrices
    one = PP.warp_affine(fr[1], mats[:3], out_size)
    assert np.array_equal(one.cpu().numpy(), WS.warp_batch(frames[1:], mats[:3], out_size))
    given = torch.zeros(2, out_size[1], out_size[0], C_, dtype=torch.uint8, device=DEV)
    assert PP.warp_affine(fr, torch.from_numpy(np.stack(mats[:2])), out_size, out=given) is given
    assert np.array_equal(given.cpu().numpy(), WS.warp_batch(frames, mats[:2], out_size))
    assert PP.warp_affine(fr, [], out_size, img_index=[]).shape == (0, out_size[1], out_size[0], C_)


def test_crop_resize_by_warp_affine_equals_the_restatement():
    from checkerpose_amd import preprocess as PP
    frames = _frames(3)
    centers = [(30.25, 20.5), (5.0, 40.0), None, (70.0, 10.0), (32.0, 24.0)]
    scales, rots, idx = [20.0, 9.5, 10.0, 30.0, 200.0], [0.0, 33.0, 0.0, -120.0, 90.0], [0, 1, 0, 1, 1]
    for out_size in (8, (16, 12)):
        size = (out_size, out_size) if isinstance(out_size, int) else out_size
        mats = [None if c is None else PP.get_affine_transform(np.array(c), (s, s), r, size) for c, s, r in zip(centers, scales, rots)]
        got = PP.crop_resize_by_warp_affine(_up(frames), centers, scales, out_size, rot=rots, interpolation=PP.INTER_LINEAR, img_index=idx)
        assert np.array_equal(got.cpu().numpy(), WS.warp_batch(frames, mats, size, WS.INTER_LINEAR, img_index=idx))
    mats0 = [None if c is None else PP.get_affine_transform(np.array(c), (s, s), 0, (8, 8)) for c, s in zip(centers, scales)]
    got = PP.crop_resize_by_warp_affine(_up(frames), centers, scales, 8, interpolation=PP.INTER_NEAREST, img_index=idx)          # rot: a scalar
    assert np.array_equal(got.cpu().numpy(), WS.warp_batch(frames, mats0, 8, WS.INTER_NEAREST, img_index=idx))


@pytest.mark.parametrize("prop", WS.PROPERTIES, ids=lambda f: f.__name__)
def test_device_has_the_property(prop):
    from checkerpose_amd import preprocess as PP

    def on_device(img, M, out_size, interp, inverse_map):
        return PP.warp_affine(_up(img), [M], out_size, interp, inverse_map=inverse_map)[0].cpu().numpy()
    assert prop(on_device, PP.get_affine_transform) == []


def test_equals_crop_square_resize_where_both_are_the_plain_slice():
    """max(bw, bh) == crop_size, even sides, integer centres: both methods give the zero-padded slice (scale 1, no resampling)"""
    from checkerpose_amd import preprocess as PP
    frames = _frames(3)
    fr = _up(frames)
    for crop, boxes in ((8, [[10, 12, 8, 8], [-3, 20, 8, 4], [60, 44, 6, 8], [20, -5, 8, 2], [-40, -40, 8, 8], [57, 3, 8, 6], None]),
                        (16, [[30, 20, 16, 16], [-7, 40, 16, 10], [55, -3, 4, 16], [24, 16, 16, 2]])):
        idx = [b % 2 for b in range(len(boxes))]
        for interp in (PP.INTER_NEAREST, PP.INTER_LINEAR):
            new = PP.get_roi_batch(fr, boxes, crop, interp, NEW, img_index=idx)
            old = PP.get_roi_batch(fr, boxes, crop, interp, "crop_square_resize", img_index=idx)
            assert torch.equal(new, old), (crop, interp)
            for b, box in enumerate(boxes):
                if box is not None:
                    x1, y1 = PP.get_final_Bbox(box, NEW, W, H)[:2]
                    assert np.array_equal(new[b].cpu().numpy(), WS.padded_slice(frames[idx[b]], int(y1), int(x1), crop, crop)), (crop, b)
        assert new[:-1].any()


def test_get_roi_batch_is_the_warp_of_the_reference_map():
    """boxes of any shape: get_roi_batch(NEW) == the restatement under get_scale_and_Bbox_center + get_affine_transform; zero crops for
    None and for boxes without area"""
    from checkerpose_amd import preprocess as PP
    frames = _frames(4)
    boxes = [[10, 12, 21, 30], [-9, 3, 20, 14], [4, -11, 13, 22], [W - 8, 5, 19, 12], [6, H - 7, 15, 18], [-5, -6, W + 11, H + 13], [W // 2, H // 2, 1, 1],
             None, [5, 5, 0, 7], [5, 5, 7, -2], [200, 100, 9, 9], [-10, 5, 100, 20]]
    idx = [b % 2 for b in range(len(boxes))]
    for crop in (8, 16):
        mats = []
        for box in boxes:
            if box is None or box[2] <= 0 or box[3] <= 0:
                mats.append(None)
                continue
            scale, c = PP.get_scale_and_Bbox_center(box, frames[0])
            mats.append(PP.get_affine_transform(c, (scale, scale), 0, (crop, crop)))
        for interp in (PP.INTER_NEAREST, PP.INTER_LINEAR):
            got = PP.get_roi_batch(_up(frames), boxes, crop, interp, NEW, img_index=idx).cpu().numpy()
            assert np.array_equal(got, WS.warp_batch(frames, mats, crop, interp, img_index=idx)), (crop, interp)
            assert not got[[7, 8, 9, 10]].any() and got[:7].any() and got[11].any()
    assert mats[11][0, 0] == 16 / 64.0                      # the 100-wide box: the scale is clamped to max(H, W) = 64 ...
    assert list(PP.get_final_Bbox(boxes[11], NEW, W, H)) == [-10, -35, 100, 100]      # ... and the final box is not (the reference's mismatch)


def test_mask_bits_equal_the_crop_of_the_expanded_mask():
    from checkerpose_amd import preprocess as PP
    rng = np.random.default_rng(77)
    plane = rng.integers(0, 2 ** 32, size=(2, H, W), dtype=np.uint64).astype(np.uint32)
    plane[:, 10:30, 20:50] |= np.uint32(1 << 31) | np.uint32(1)
    bits_t = _up(plane.view(np.int32))
    boxes = [[-9, 3, 20, 14], [4, -11, 13, 22], [W - 8, 5, 19, 12], [6, H - 7, 15, 18], [3, 4, 11, 9], [-5, -6, W + 11, H + 13], [W // 2, H // 2, 1, 1],
             None, [5, 5, 0, 7], [24, 12, 16, 14]]
    bit = [0, 31, 7, 16, 31, 0, 5, 3, 3, 31]
    idx = [b % 2 for b in range(len(boxes))]
    expanded = np.stack([np.where((plane[idx[b]] >> np.uint32(bit[b])) & np.uint32(1), 255, 0).astype(np.uint8) for b in range(len(boxes))])[..., None]
    for crop in (8, 16):
        got = PP.get_roi_mask_bits(bits_t, bit, boxes, crop, NEW, img_index=idx)
        want = PP.get_roi_batch(_up(expanded), boxes, crop, PP.INTER_NEAREST, NEW)
        assert got.shape == want.shape == (len(boxes), crop, crop, 1) and torch.equal(got, want), crop
        assert not got[7].any() and not got[8].any() and got[9].all() and got[:7].any()
        assert set(np.unique(got.cpu().numpy())) <= {0, 255}
    assert not PP.get_roi_mask_bits(bits_t, [32, -1], [boxes[9]] * 2, 8, NEW, img_index=[0, 0]).any()          # a bit outside 0..31
    assert torch.equal(PP.get_roi_mask_bits(bits_t[1], [31], [boxes[9]], 8, NEW), got.new_full((1, 8, 8, 1), 255))


def _batch_inputs(B=6):
    rng = np.random.default_rng(31)
    frames = rng.integers(1, 256, size=(2, H, W, 3), dtype=np.uint8)
    vis = np.zeros((2, H, W), np.uint8)
    vis[0, 8:30, 10:40], vis[1, 20:44, 30:60] = 255, 255
    full = np.maximum(vis, np.roll(vis, 4, axis=2))
    boxes = [[10, 8, 30, 22], [30, 20, 30, 24], [-6, 2, 25, 31], None, [40, 30, 31, 25], [12, 10, 9, 9]][:B]
    idx = [0, 1, 0, 1, 1, 0][:B]
    Rs = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(B)])
    ts = np.stack([[rng.uniform(-20, 20), rng.uniform(-20, 20), 600.0] for _ in range(B)])
    K = np.array([[150.0, 0.0, 32.0], [0.0, 150.0, 24.0], [0.0, 0.0, 1.0]])
    pts = rng.normal(size=(32, 3)) * 20.0
    return frames, vis, full, boxes, idx, Rs, ts, K, pts


def _check_labels(batch, pts, K, Rs, ts, final, S):
    from checkerpose_amd import targets
    lab = targets.encode_targets(pts, K, Rs, ts, final, S)
    assert torch.equal(batch[-4], lab["roi_mask_bits"]) and torch.equal(batch[-3], lab["pixel_x_codes"]) and torch.equal(batch[-2], lab["pixel_y_codes"])
    assert torch.equal(batch[-1], targets.roi_xy_grid(final, S, batch[-1].device))
    want = np.array([[0, 0, 0, 0] if b is None else [int(v) for v in b] for b in final])
    assert np.array_equal(batch[5].cpu().numpy(), want)


def test_make_training_batch_with_the_new_method():
    from checkerpose_amd import augment as A
    from checkerpose_amd import preprocess as PP
    from checkerpose_amd import targets
    frames, vis, full, boxes, idx, Rs, ts, K, pts = _batch_inputs()
    fr, mv, mf, R, t = _up(frames), _up(vis), _up(full), _up(Rs), _up(ts)
    kw = dict(is_train=False, crop_size_img=16, crop_size_gt=8, resize_method=NEW, img_index=idx)
    batch = targets.make_training_batch(fr, mv, mf, R, t, K, boxes, pts, **kw)
    padded = [None if b is None else PP.padding_Bbox(b, 1.5) for b in boxes]
    final = [None if b is None else PP.get_final_Bbox(b, NEW, W, H) for b in padded]
    assert len(batch) == 11
    assert torch.equal(batch[0], PP.get_roi_batch(fr, padded, 16, PP.INTER_LINEAR, NEW, img_index=idx)) and batch[0].any() and not batch[0][3].any()
    assert torch.equal(batch[1], PP.get_roi_batch(mf.unsqueeze(-1), padded, 8, PP.INTER_NEAREST, NEW, img_index=idx)[..., 0].float() / 255.0)
    assert torch.equal(batch[2], PP.get_roi_batch(mv.unsqueeze(-1), padded, 8, PP.INTER_NEAREST, NEW, img_index=idx)[..., 0].float() / 255.0)
    assert batch[1].sum() > batch[2].sum() > 0
    _check_labels(batch, pts, K, R, t, final, 8)
    plan = A.sample_plan(len(boxes), np.random.default_rng(5), color_aug_prob=1.0, frame_hw=(H, W))
    assert not plan.is_identity().all()
    aug = targets.make_training_batch(fr, mv, mf, R, t, K, boxes, pts, augment=plan, **kw)
    whole = A.augment_frames(fr, plan, img_index=idx)                                        # every pixel of every sample's frame
    assert torch.equal(aug[0], PP.get_roi_batch(whole, padded, 16, PP.INTER_LINEAR, NEW, img_index=np.arange(len(boxes))))
    assert not torch.equal(aug[0], batch[0])
    for a, b in zip(aug[1:], batch[1:]):
        assert torch.equal(a, b)


def test_the_rectangle_holds_every_pixel_the_crop_reads():
    """a position-coded frame; everything outside roi_window's rectangle is recoloured: the crop must not move (and must move when the
    rectangle's own border pixels are recoloured as well: the rectangle is not just generous)"""
    from checkerpose_amd import preprocess as PP
    y, x = np.mgrid[0:H, 0:W]
    frame = np.stack([x + 1, y + 1, (x + y) % 255 + 1], -1).astype(np.uint8)
    boxes = [[10, 12, 21, 30], [-9, 3, 20, 14], [4, -11, 13, 22], [W - 8, 5, 19, 12], [6, H - 7, 15, 18], [20, 10, 9, 9], [3, 4, 11, 9], [31, 17, 2, 2]]
    for crop in (8, 16):
        for b, box in enumerate(boxes):
            for interp in (PP.INTER_NEAREST, PP.INTER_LINEAR):
                x1, y1, x2, y2 = PP.roi_window(box, NEW, W, H, crop)[:4]
                assert 0 <= x1 < x2 <= W and 0 <= y1 < y2 <= H
                changed = 255 - frame
                changed[y1:y2, x1:x2] = frame[y1:y2, x1:x2]
                both = PP.get_roi_batch(_up(np.stack([frame, changed])), [box, box], crop, interp, NEW)
                assert torch.equal(both[0], both[1]) and both[0].any(), (crop, b, interp)
    # the rectangle of a crop size is tight on the side the taps reach: recolouring its own first column / row moves the INTER_LINEAR crop
    x1, y1, x2, y2 = PP.roi_window(boxes[0], NEW, W, H, 16)[:4]
    changed = frame.copy()
    changed[y1:y2, x1] = 255 - frame[y1:y2, x1]
    both = PP.get_roi_batch(_up(np.stack([frame, changed])), [boxes[0]] * 2, 16, PP.INTER_LINEAR, NEW)
    assert not torch.equal(both[0], both[1])


def test_scene_training_batch_with_the_new_method():
    from checkerpose_amd import augment as A
    from checkerpose_amd import preprocess as PP
    from checkerpose_amd import render
    from tests import test_gpu_scene_labels as SL
    size = (70, 50)
    s = SL.scene_of(size)
    poses = [j for j in range(len(s["img"])) if s["img"][j] != 3]
    _, _, dev, a = SL._args(size, "phong", "surf", "shared", poses)
    p3 = np.random.default_rng(7).uniform(-45.0, 45.0, size=(24, 3))
    kw = dict(n_images=SL.N_IMG, surf_colors=a["surf"], shading="phong", crop_size_img=16, crop_size_gt=8, is_train=False, resize_method=NEW)
    batch, kept = render.scene_training_batch(SL.mesh_set(), a["mesh"], a["R"], a["t"], a["K"], size, a["img"], p3, **kw)
    sc = SL.scene_call(size, poses=poses, with_bg=False)
    assert len(kept) >= 4 and len(batch) == 11
    img = np.asarray(a["img"])[kept]
    padded = [PP.padding_Bbox(b, 1.5) for b in sc["bbox_visib"].cpu().numpy()[kept]]
    final = [PP.get_final_Bbox(b, NEW, size[0], size[1]) for b in padded]
    slot = sc["slot"].cpu().numpy()[kept]
    kd = torch.from_numpy(kept).to(dev)
    assert torch.equal(batch[0], PP.get_roi_batch(sc["rgb"], padded, 16, PP.INTER_LINEAR, NEW, img_index=img)) and batch[0].any()
    assert torch.equal(batch[1], PP.get_roi_mask_bits(sc["full_bits"], slot, padded, 8, NEW, img_index=img)[..., 0].float() / 255.0)
    assert torch.equal(batch[2], PP.get_roi_mask_bits(sc["visib_bits"], slot, padded, 8, NEW, img_index=img)[..., 0].float() / 255.0)
    assert batch[1].sum() > batch[2].sum() > 0
    _check_labels(batch, p3, a["K"], a["R"][kd], a["t"][kd], final, 8)
    plan = A.sample_plan(len(poses), np.random.default_rng(11), color_aug_prob=1.0, frame_hw=(size[1], size[0]))
    aug, kept2 = render.scene_training_batch(SL.mesh_set(), a["mesh"], a["R"], a["t"], a["K"], size, a["img"], p3, augment=plan, **kw)
    assert kept2.tolist() == kept.tolist()
    whole = A.augment_frames(sc["rgb"], plan.select(kept), img_index=img)
    assert torch.equal(aug[0], PP.get_roi_batch(whole, padded, 16, PP.INTER_LINEAR, NEW, img_index=np.arange(len(kept))))
    assert not torch.equal(aug[0], batch[0])
    for x, y in zip(aug[1:], batch[1:]):
        assert torch.equal(x, y)


def test_estimate_poses_runs_with_the_new_method():
    from checkerpose_amd import postprocess as Q
    from checkerpose_amd import preprocess as PP
    from checkerpose_amd.synthetic import build_net
    rng = np.random.default_rng(9)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 120, 160, 3), dtype=np.uint8)).cuda()
    boxes = [[40, 30, 50, 40], [100, 60, 30, 70], None, [-10, 90, 40, 40]]
    idx = [0, 1, 0, 1]
    net = build_net(npoint=512, seed=1).cuda().eval()
    net.set_compute_dtype("bf16")
    p3d = torch.from_numpy(rng.normal(size=(512, 3)).astype(np.float32) * 50).cuda()
    K = np.array([[572.4, 0, 80.0], [0, 573.6, 60.0], [0, 0, 1]], dtype=np.float32)
    new = Q.estimate_poses(net, frames, boxes, p3d, K, img_index=idx, resize_method=NEW)
    old = Q.estimate_poses(net, frames, boxes, p3d, K, img_index=idx, resize_method="crop_square_resize")
    for a, b in zip(new[:4], old[:4]):
        assert a.shape == b.shape and a.dtype == b.dtype
    padded = [None if b is None else PP.padding_Bbox(b, 1.5) for b in boxes]
    want = np.array([[0, 0, 0, 0] if b is None else PP.get_final_Bbox(b, NEW, 160, 120) for b in padded])
    assert np.array_equal(new[4], want) and np.array_equal(new[4], old[4])                   # the square case (:195)
    assert torch.isfinite(new[0]).all() and torch.isfinite(new[1]).all()


def test_refusals_return_before_a_launch(lib):
    from checkerpose_amd import preprocess as PP
    fr = _up(_frames(3))
    inv = torch.zeros(2, 6, dtype=torch.float64, device=DEV)
    out = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    lib.cp_kernel_log_begin()
    assert lib.cp_warp_affine_u8(None, p(fr), 2, H, W, 5, p(inv), None, p(out), 2, 8, 8, 1) == -1             # C = 5
    assert lib.cp_warp_affine_u8(None, None, 2, H, W, 3, p(inv), None, p(out), 2, 8, 8, 1) == -1              # null pointers
    assert lib.cp_warp_affine_u8(None, p(fr), 2, H, W, 3, None, None, p(out), 2, 8, 8, 1) == -1
    assert lib.cp_warp_affine_u8(None, p(fr), 2, H, W, 3, p(inv), None, None, 2, 8, 8, 1) == -1
    assert lib.cp_warp_affine_u8(None, p(fr), 2, H, W, 3, p(inv), None, p(out), 3, 8, 8, 1) == -1             # 3 crops of 2 images, no img_index
    assert lib.cp_warp_mask_bits(None, p(fr), 2, H, W, p(inv), None, None, p(out), 2, 8, 8) == -1
    assert lib.cp_kernel_log() == b""
    with pytest.raises(RuntimeError, match="img_index"):
        PP.warp_affine(fr, [None] * 3, 8)
    with pytest.raises(RuntimeError, match="img_index"):
        PP.warp_affine(fr, [None] * 2, 8, img_index=[0, 2])
    with pytest.raises(ValueError, match="2\\^20"):
        PP.warp_affine(fr, [np.array([[1.0, 0.0, 2.0e6], [0.0, 1.0, 0.0]]), None], 8)
    with pytest.raises(ValueError, match="2\\^20"):
        PP.warp_affine(fr, [np.array([[1.0, 0.0, np.inf], [0.0, 1.0, 0.0]]), None], 8, inverse_map=True)
    with pytest.raises(NotImplementedError):
        PP.warp_affine(fr, [None, None], 8, interpolation=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        PP.get_roi_batch(fr.cpu(), [[1, 1, 4, 4]], 8, resize_method=NEW)
    with pytest.raises(RuntimeError):
        PP.warp_affine(torch.zeros(2, H, W, 5, dtype=torch.uint8, device=DEV), [None, None], 8)
    with pytest.raises(NotImplementedError, match="unknown decoder type"):
        PP.get_roi_batch(fr, [[1, 1, 4, 4]], 8, resize_method="crop_by_magic")
    assert lib.cp_kernel_log() == b""
