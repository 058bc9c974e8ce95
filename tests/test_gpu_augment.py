"""GPU: checkerpose_amd.augment.augment_frames (cp_augment_frames, csrc/augment.hip) against the numpy
restatement tests/augment_stages.py, bit for bit: every stage alone and the full chain, the invariances the kernel promises, tile
edges (64 x 32 tiles), the wiring into targets.make_training_batch, and the refusals."""
import numpy as np
import pytest
import torch

from tests import augment_stages as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE_W, TILE_H = 64, 32
SIZES = [(5, 5), (33, 31), (70, 50), (160, 120)]                                          # (W, H)
EDGE_SIZES = [(TILE_W - 1, TILE_H - 1), (TILE_W, TILE_H), (TILE_W + 1, TILE_H + 1)]


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _scene(W, H, n_img=3, n_bg=2, seed=0):
    """noise frames with a bright square across the first tile corner (where the frame has one), disc masks, a background pool"""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(n_img, H, W, 3), dtype=np.uint8)
    cy, cx = min(TILE_H, H - 1), min(TILE_W, W - 1)
    frames[:, max(cy - 3, 0):cy + 3, max(cx - 3, 0):cx + 3] = 255
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.stack([(((xx - W * (0.3 + 0.2 * i)) ** 2 + (yy - H * 0.5) ** 2) <= (0.3 * min(H, W)) ** 2).astype(np.uint8) * 255
                      for i in range(n_img)])
    bgs = rng.integers(0, 256, size=(n_bg, H, W, 3), dtype=np.uint8)
    return frames, masks, bgs


def _single_stage_plans(A, H, W, rng):
    """name -> one-sample plan with exactly that stage on"""
    def base():
        p = A.AugmentPlan.identity(1, (H, W))
        p.key[:] = rng.integers(0, 1 << 32, dtype=np.uint64)
        return p
    plans = {"off": base()}
    p = base(); p.bg_index[:] = 1; plans["bg"] = p
    p = base(); p.sp_on[:] = 1; p.sp_thresh[:] = A.threshold_u32(0.05); plans["salt_pepper"] = p
    p = base(); p.motion_on[:] = 1; p.motion_w[0] = A.motion_weights(37.0, 0.6); plans["motion"] = p
    p = base(); p.drop_on[:] = 1; p.drop_thresh[:] = A.threshold_u32(0.3); plans["dropout"] = p
    p = base(); p.gauss_on[:] = 1; p.gauss_w[0] = A.gaussian_weights(0.9); plans["gaussian"] = p
    p = base(); p.lut[0] = A.compose_lut(add=[15, -20, 3], invert=[True, False, True], mul_pc=[1.3, 0.8, 1.1], mul=1.2, contrast=[1.7, 0.6, 1.0])
    plans["lut"] = p
    return plans


def _full_plan(A, B, H, W, seed, n_bg=2):
    """sampled plans with both optional ops, bg on and off; sample 0 forced to everything-off, sample 1 to everything-on"""
    rng = np.random.default_rng(seed)
    plan = A.sample_plan(B, rng, use_peper_salt=True, use_motion_blur=True, change_bg=0.5, n_bg=n_bg, frame_hw=(H, W))
    off = A.AugmentPlan.identity(1, (H, W))
    for k in ("bg_index", "sp_on", "motion_on", "drop_on", "gauss_on", "lut", "motion_w", "gauss_w"):
        getattr(plan, k)[0] = getattr(off, k)[0]
    plan.bg_index[1] = 0
    plan.sp_on[1], plan.sp_thresh[1] = 1, A.threshold_u32(0.05)
    plan.motion_on[1], plan.motion_w[1] = 1, A.motion_weights(200.0, -0.4)
    plan.drop_on[1], plan.drop_thresh[1] = 1, A.threshold_u32(0.1)
    plan.gauss_on[1], plan.gauss_w[1] = 1, A.gaussian_weights(0.7)
    plan.lut[1] = A.compose_lut(add=[-9, -9, -9], mul_pc=[0.9, 1.35, 1.0], contrast=[1.9, 1.9, 1.9])
    return plan


@pytest.mark.parametrize("W,H", SIZES + EDGE_SIZES)
def test_each_stage_alone_matches_the_restatement(W, H):
    from checkerpose_amd import augment as A
    frames, masks, bgs = _scene(W, H, seed=W * 1000 + H)
    fr, mk, bg = _up(frames), _up(masks), _up(bgs)
    for name, plan in _single_stage_plans(A, H, W, np.random.default_rng(W + H)).items():
        got = A.augment_frames(fr, plan, masks=mk, backgrounds=bg, img_index=[2]).cpu().numpy()
        ref = S.augment_stages(frames, plan, masks, bgs, img_index=[2])
        assert np.array_equal(got, ref), (name, W, H, int((got != ref).sum()))
        if name == "off":
            assert np.array_equal(got[0], frames[2])
        else:
            assert not np.array_equal(got[0], frames[2]), name                     # the stage did something on this scene


@pytest.mark.parametrize("W,H", SIZES + EDGE_SIZES)
def test_full_chain_matches_the_restatement(W, H):
    from checkerpose_amd import augment as A
    frames, masks, bgs = _scene(W, H, seed=7)
    B = 8
    plan = _full_plan(A, B, H, W, seed=W + 31 * H)
    idx = [0, 1, 2, 1, 1, 0, 2, 2]                                                  # several samples share a frame
    got = A.augment_frames(_up(frames), plan, masks=_up(masks), backgrounds=_up(bgs), img_index=idx).cpu().numpy()
    ref = S.augment_stages(frames, plan, masks, bgs, img_index=idx)
    for b in range(B):
        assert np.array_equal(got[b], ref[b]), (b, W, H, int((got[b] != ref[b]).sum()))
    assert np.array_equal(got[0], frames[0])                                        # everything off: the frame itself


def test_bitwise_invariances():
    from checkerpose_amd import augment as A
    W, H, B = 160, 120, 8
    frames, masks, bgs = _scene(W, H, seed=11)
    fr, mk, bg = _up(frames), _up(masks), _up(bgs)
    plan = _full_plan(A, B, H, W, seed=5)
    idx = np.array([0, 1, 2, 1, 1, 0, 2, 2])
    whole = A.augment_frames(fr, plan, masks=mk, backgrounds=bg, img_index=idx)
    for b in (1, 4, 7):                                                             # alone
        one = A.augment_frames(fr, plan.select([b]), masks=mk, backgrounds=bg, img_index=idx[[b]])
        assert torch.equal(one[0], whole[b]), b
    perm = np.array([5, 1, 7, 0, 3, 2, 6, 4])                                       # another batch position
    moved = A.augment_frames(fr, plan.select(perm), masks=mk, backgrounds=bg, img_index=idx[perm])
    assert torch.equal(moved, whole[torch.from_numpy(perm).to(DEV)])
    rects = np.array([[10 + 9 * b, 5 + 3 * b, 90 + 8 * b, 60 + 7 * b] for b in range(B)])     # with rects: equal inside the rect
    rects[3] = [0, 0, W, H]
    rects[5] = [70, 40, 70, 40]                                                     # empty: nothing has to be computed
    out = torch.full((B, H, W, 3), 77, dtype=torch.uint8, device=DEV)
    part = A.augment_frames(fr, plan, masks=mk, backgrounds=bg, img_index=idx, rects=rects, out=out)
    assert part.data_ptr() == out.data_ptr()
    for b, (x1, y1, x2, y2) in enumerate(rects):
        assert torch.equal(part[b, y1:y2, x1:x2], whole[b, y1:y2, x1:x2]), b
    assert bool((part[5] == 77).all())                                              # no tile met the empty rect
    assert bool((part[0, 96:, :] == 77).all())                                      # tiles below the first rect were skipped
    given = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=DEV)                  # out= given
    assert A.augment_frames(fr, plan, masks=mk, backgrounds=bg, img_index=idx, out=given) is given and torch.equal(given, whole)


def test_make_training_batch_with_a_plan():
    from checkerpose_amd import augment as A
    from checkerpose_amd import preprocess as PP
    from checkerpose_amd import targets
    W, H, B = 160, 120, 4
    frames, masks, bgs = _scene(W, H, n_img=B, seed=13)
    full = np.maximum(masks, np.roll(masks, 5, axis=2))
    rng = np.random.default_rng(2)
    Rs = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(B)])
    ts = np.stack([[0.0, 0.0, 600.0]] * B)
    K = np.array([[150.0, 0.0, 80.0], [0.0, 150.0, 60.0], [0.0, 0.0, 1.0]])
    pts = rng.normal(size=(64, 3)) * 20.0
    boxes = []
    for m in masks:
        ys, xs = np.nonzero(m)
        boxes.append([int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)])
    plan = _full_plan(A, B, H, W, seed=3)
    fr, mv, mf, bg = _up(frames), _up(masks), _up(full), _up(bgs)
    args = (fr, mv, mf, _up(Rs), _up(ts), K, boxes, pts)
    np.random.seed(4)
    plain = targets.make_training_batch(*args, crop_size_img=64, crop_size_gt=16)
    np.random.seed(4)
    none = targets.make_training_batch(*args, crop_size_img=64, crop_size_gt=16, augment=None, backgrounds=None)
    np.random.seed(4)
    aug = targets.make_training_batch(*args, crop_size_img=64, crop_size_gt=16, augment=plan, backgrounds=bg)
    np.random.seed(4)
    grown = [targets.aug_Bbox(np.array(b), 1.5) for b in boxes]
    assert len(plain) == len(none) == len(aug) == 11
    for a, b in zip(plain, none):                                                   # augment=None: today's output
        assert torch.equal(a, b)
    assert torch.equal(plain[0], PP.get_roi_batch(fr, grown, 64, PP.INTER_LINEAR))
    ref_frames = _up(S.augment_stages(frames, plan, masks, bgs))
    assert torch.equal(aug[0], PP.get_roi_batch(ref_frames, grown, 64, PP.INTER_LINEAR))
    assert not torch.equal(aug[0], plain[0])
    for a, b in zip(plain[1:], aug[1:]):                                            # every other entry is unaffected
        assert torch.equal(a, b)


def test_refusals():
    from checkerpose_amd import augment as A
    frames, masks, bgs = _scene(33, 31, seed=1)
    fr, mk, bg = _up(frames), _up(masks), _up(bgs)
    plan = A.AugmentPlan.identity(3, (31, 33))
    with pytest.raises(ValueError, match="5 x 5"):
        A.augment_frames(fr[:, :4].contiguous(), A.AugmentPlan.identity(3, (4, 33)))
    with pytest.raises(ValueError, match="5 x 5"):
        A.augment_frames(fr[:, :, :4].contiguous(), A.AugmentPlan.identity(3, (31, 4)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.augment_frames(torch.from_numpy(frames), plan)
    plan.bg_index[1] = 0
    with pytest.raises(ValueError, match="masks and backgrounds"):
        A.augment_frames(fr, plan, backgrounds=bg)
    with pytest.raises(ValueError, match="masks and backgrounds"):
        A.augment_frames(fr, plan, masks=mk)
    plan.bg_index[1] = 2
    with pytest.raises(ValueError, match="outside the pool"):
        A.augment_frames(fr, plan, masks=mk, backgrounds=bg)
    with pytest.raises(ValueError, match="img_index"):
        A.augment_frames(fr, A.AugmentPlan.identity(2, (31, 33)))
    with pytest.raises(ValueError, match="img_index"):
        A.augment_frames(fr, A.AugmentPlan.identity(2, (31, 33)), img_index=[0, 3])
