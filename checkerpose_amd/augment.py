"""Training-frame augmentation on the device: the colour chain and the background swap of the reference's
loaders, planned on the host, applied to whole batches of resident frames in ONE HIP launch.

The reference augments one frame at a time on the host before it crops: `replace_bg` (lm_dataset_pytorch.py:376-384,523-541; always
for `img_type == "syn"`, with `change_bg_prob` for real images) and `apply_augmentation` (bop_dataset_pytorch.py:400-405,
lm_dataset_pytorch.py:482-487; with probability 0.8 the imgaug chain of GDR_Net_Augmentation.build_augmentations :161-178).  Here

  sample_plan      draws everything random or floating-point once, on the host, into an `AugmentPlan` of small integer arrays;
  augment_frames   applies a plan: frames + masks + a background pool, all on the device -> augmented uint8 frames (cp_augment_frames,
                   csrc/augment.hip: integer work only, bit-exact against the numpy restatement tests/augment_stages.py).

`targets.make_training_batch(..., augment=plan, backgrounds=pool)` runs it on the windows it crops.

UNPINNED: parity with imgaug.  imgaug and cv2 are not available to this project, so the rules below are this project's statement of
those augmenters; each names the imgaug behaviour it models, the places to check with imgaug at hand.  The chain is random, and `rng`
is NOT the loader's `np.random` / `random` / imgaug streams: no run reproduces imgaug's draws.
Out of scope: reading or resizing background files (`get_bg_image`: the pool arrives at frame size), `truncate_fg` (no loader calls
it), `image_augmentations_lm` / `_bop` (unused by the loaders), `sigma >= 1.5` (the chain draws sigma in [0, 1)).
No CPU fallback: CPU tensors raise."""
import numpy as np
import torch

from . import _abi

_NO_CPU = "checkerpose_amd.augment: CUDA/HIP tensors required (no CPU fallback)"

F_SP, F_MOTION, F_DROP, F_GAUSS, F_LUT, F_RECT = 1, 2, 4, 8, 16, 32          # csrc/augment.hip
OP_SP, OP_SP_VALUE, OP_DROP = 1, 2, 3                                       # the hash's op ids
_HEAD_BYTES, _REC_WORDS, _REC_BYTES = 256, 44, 944
_IDENTITY_LUT = np.broadcast_to(np.arange(256, dtype=np.uint8), (3, 256))

# chain probabilities and ranges (GDR_Net_Augmentation.py:161-178)
P_SP, P_MOTION, P_DROP, P_GAUSS, P_ADD, P_INVERT, P_MUL_PC, P_MUL, P_CONTRAST = 0.3, 0.2, 0.4, 0.5, 0.5, 0.4, 0.5, 0.5, 0.5
SP_P, DROP_P, DROP_SIZE_PERCENT = 0.05, 0.1, 0.05
ADD_RANGE, ADD_PER_CHANNEL = (-20, 20), 0.3
INVERT_P = 0.2
MUL_RANGE, MUL_PER_CHANNEL = (0.7, 1.4), 0.8
CONTRAST_RANGE, CONTRAST_PER_CHANNEL = (0.5, 2.0), 0.3


def sp_value_table():
    """imgaug SaltAndPepper's replacement `Beta(0.5, 0.5) * 255`: the arcsine law through its quantile function sin(pi u / 2)^2 at the
    256 midpoints u = (i + 0.5) / 256, cast by truncation -> uint8 (256,), indexed by eight hash bits"""
    u = (np.arange(256, dtype=np.float64) + 0.5) / 256.0
    return (np.sin(np.pi * u / 2.0) ** 2 * 255.0).astype(np.uint8)


def threshold_u32(p):
    """a probability as the hash threshold `p * 2**32` (a pixel / cell is hit where hash < threshold), saturated at 2**32 - 1"""
    return np.uint32(min(max(int(float(p) * 4294967296.0), 0), 4294967295))


def gaussian_weights(sigma):
    """imgaug GaussianBlur's cv2 backend: ksize = 3.3 sigma (sigma < 3), int(max(ksize, 5)), made odd -- always 5 for sigma < 1.5;
    weights exp(-(i - 2)^2 / (2 sigma^2)) normalised in float64 -> int32 (5,) summing to 4096, the centre tap taking the remainder"""
    sigma = float(sigma)
    if not 0.0 <= sigma < 1.5:
        raise ValueError("gaussian_weights: sigma must be in [0, 1.5) (a 5-tap kernel), got %r" % sigma)
    if sigma < 1e-3:
        return np.array([0, 0, 4096, 0, 0], dtype=np.int32)
    i = np.arange(5, dtype=np.float64)
    w = np.exp(-(i - 2.0) ** 2 / (2.0 * sigma * sigma))
    q = np.rint(w / w.sum() * 4096.0).astype(np.int64)
    q[2] = 4096 - (q[0] + q[1] + q[3] + q[4])
    return q.astype(np.int32)


def motion_weights(angle, direction):
    """imgaug MotionBlur(k=5): the centre column of a 5 x 5 matrix weighted linspace(d, 1 - d, 5) with d = (direction + 1) / 2, rotated
    by `angle` degrees about the centre with bilinear sampling (zero outside), divided by its sum -> int32 (25,) row-major summing to
    65536, the largest tap taking the remainder"""
    d01 = (min(max(float(direction), -1.0), 1.0) + 1.0) / 2.0
    m = np.zeros((5, 5), dtype=np.float64)
    m[:, 2] = np.linspace(d01, 1.0 - d01, 5)
    a = np.deg2rad(float(angle))
    ca, sa = np.cos(a), np.sin(a)
    yy, xx = np.mgrid[0:5, 0:5].astype(np.float64) - 2.0
    sx, sy = ca * xx + sa * yy + 2.0, -sa * xx + ca * yy + 2.0            # inverse map: where each output tap samples the column
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    pad = np.zeros((9, 9), dtype=np.float64)
    pad[2:7, 2:7] = m
    ix, iy = np.clip(x0.astype(np.int64) + 2, 0, 7), np.clip(y0.astype(np.int64) + 2, 0, 7)
    inside = (x0 >= -2) & (x0 <= 5) & (y0 >= -2) & (y0 <= 5)
    r = ((1 - fy) * ((1 - fx) * pad[iy, ix] + fx * pad[iy, ix + 1]) + fy * ((1 - fx) * pad[iy + 1, ix] + fx * pad[iy + 1, ix + 1])) * inside
    w = (r / r.sum()).reshape(-1)
    q = np.rint(w * 65536.0).astype(np.int64)
    k = int(np.argmax(w))
    q[k] = 0
    q[k] = 65536 - q.sum()
    return q.astype(np.int32)


def dropout_grid(H, W):
    """imgaug CoarseDropout(size_percent=0.05): the mask is drawn on a grid of max(3, int(size * 0.05)) cells per side and enlarged to
    the frame by nearest neighbour -> (gh, gw)"""
    return max(3, int(H * DROP_SIZE_PERCENT)), max(3, int(W * DROP_SIZE_PERCENT))


def lut_add(lut, a):
    """imgaug Add on uint8: clip(v + a, 0, 255), a an integer per channel (3,)"""
    return np.clip(lut.astype(np.int64) + np.asarray(a, dtype=np.int64).reshape(3, 1), 0, 255).astype(np.uint8)


def lut_invert(lut, channels):
    """imgaug Invert on uint8: 255 - v on the channels drawn (3,) bool"""
    return np.where(np.asarray(channels, dtype=bool).reshape(3, 1), 255 - lut, lut).astype(np.uint8)


def lut_multiply(lut, m):
    """imgaug Multiply on uint8: clip(v * m, 0, 255) in float64, cast by truncation; m per channel (3,)"""
    return np.clip(lut.astype(np.float64) * np.asarray(m, dtype=np.float64).reshape(3, 1), 0.0, 255.0).astype(np.uint8)


def lut_contrast(lut, alpha):
    """imgaug ContrastNormalization (LinearContrast) on uint8: clip(128 + alpha (v - 128), 0, 255) in float64, cast by truncation"""
    return np.clip(128.0 + np.asarray(alpha, dtype=np.float64).reshape(3, 1) * (lut.astype(np.float64) - 128.0), 0.0, 255.0).astype(np.uint8)


def compose_lut(add=None, invert=None, mul_pc=None, mul=None, contrast=None):
    """the chain's pointwise tail as ONE table per channel: Add, Invert, Multiply (per channel), Multiply, Contrast in that order, each
    uint8 -> uint8 with its own clip before the next (imgaug's uint8 paths); None skips an op -> uint8 (3,256)"""
    lut = np.ascontiguousarray(_IDENTITY_LUT)
    if add is not None:
        lut = lut_add(lut, add)
    if invert is not None:
        lut = lut_invert(lut, invert)
    if mul_pc is not None:
        lut = lut_multiply(lut, mul_pc)
    if mul is not None:
        lut = lut_multiply(lut, np.repeat(np.float64(mul), 3))
    if contrast is not None:
        lut = lut_contrast(lut, contrast)
    return lut


def _per_channel(rng, q, draw):
    """imgaug's `per_channel=q`: with probability q one value per channel, otherwise one value for all three -> (3,)"""
    v = draw(3)
    return v if rng.random() < q else np.repeat(v[:1], 3)


_FIELDS = ("key", "bg_index", "sp_on", "sp_thresh", "motion_on", "motion_w", "drop_on", "drop_thresh", "drop_grid", "gauss_on", "gauss_w",
           "lut", "color_on", "add_on", "add", "invert_on", "invert", "mul_pc_on", "mul_pc", "mul_on", "mul", "contrast_on", "contrast",
           "sigma", "angle", "direction")


class AugmentPlan:
    """What `augment_frames` applies, numpy arrays with one row per sample:
      key uint32 (the hash key: drawn with the sample, never its position in a launch); bg_index int32 (-1: no swap);
      sp_on, motion_on, drop_on, gauss_on uint8; sp_thresh, drop_thresh uint32 (p * 2**32); motion_w int32 (B,25) summing to 65536;
      drop_grid int32 (B,2) = gh, gw; gauss_w int32 (B,5) summing to 4096; lut uint8 (B,3,256).
    For inspection only (the device reads none of them): color_on (the 0.8 draw), {add,invert,mul_pc,mul,contrast}_on and their
    values add int32 (B,3), invert uint8 (B,3), mul_pc / contrast float64 (B,3), mul float64 (B,), sigma, angle, direction float64."""

    def __init__(self, **arrays):
        for k in _FIELDS:
            setattr(self, k, arrays[k])
        self.B = int(self.key.shape[0])

    @staticmethod
    def identity(B, frame_hw=(480, 640)):
        """every op off, identity tables, no background swap"""
        gh, gw = dropout_grid(*frame_hw)
        z8 = lambda *s: np.zeros((B,) + s, dtype=np.uint8)      # noqa: E731
        motion = np.zeros((B, 25), dtype=np.int32)
        motion[:, 12] = 65536
        gauss = np.zeros((B, 5), dtype=np.int32)
        gauss[:, 2] = 4096
        return AugmentPlan(key=np.zeros(B, dtype=np.uint32), bg_index=np.full(B, -1, dtype=np.int32), sp_on=z8(),
                           sp_thresh=np.zeros(B, dtype=np.uint32), motion_on=z8(), motion_w=motion, drop_on=z8(),
                           drop_thresh=np.zeros(B, dtype=np.uint32), drop_grid=np.tile(np.array([[gh, gw]], dtype=np.int32), (B, 1)),
                           gauss_on=z8(), gauss_w=gauss, lut=np.ascontiguousarray(np.broadcast_to(_IDENTITY_LUT, (B, 3, 256))),
                           color_on=z8(), add_on=z8(), add=np.zeros((B, 3), dtype=np.int32), invert_on=z8(), invert=z8(3), mul_pc_on=z8(),
                           mul_pc=np.ones((B, 3)), mul_on=z8(), mul=np.ones(B), contrast_on=z8(), contrast=np.ones((B, 3)),
                           sigma=np.zeros(B), angle=np.zeros(B), direction=np.zeros(B))

    def select(self, index):
        """the plan of the samples `index` (an int sequence / array), in that order: rows keep their keys"""
        idx = np.asarray(index, dtype=np.int64).reshape(-1)
        return AugmentPlan(**{k: np.ascontiguousarray(getattr(self, k)[idx]) for k in _FIELDS})

    def is_identity(self):
        """(B,) bool: no op, identity tables, no swap"""
        off = (self.sp_on == 0) & (self.motion_on == 0) & (self.drop_on == 0) & (self.gauss_on == 0) & (self.bg_index < 0)
        return off & (self.lut == _IDENTITY_LUT[None]).all((1, 2))


def sample_plan(B, rng, use_peper_salt=False, use_motion_blur=False, color_aug_prob=0.8, change_bg=None, n_bg=0, frame_hw=(480, 640)):
    """The random side of `replace_bg` + `apply_augmentation` for B samples -> AugmentPlan.
      rng: a numpy.random.Generator -- NOT the loader's np.random / random / imgaug streams; use_peper_salt / use_motion_blur:
      build_augmentations' switches; color_aug_prob: the loaders' 0.8; change_bg: None (the BOP loader: never), a probability (the LM
      loader's change_bg_prob for real images) or a per-sample bool array (how a caller forces the swap for img_type == "syn"); n_bg:
      the size of the background pool the swap draws from (uniformly); frame_hw: (H, W) of the frames (the dropout grid).
    A sample that fails the colour draw has every colour op off and identity tables.  Each op is then switched on with the chain's
    `Sometimes` probability and its parameters drawn from the chain's ranges (module constants above)."""
    B = int(B)
    H, W = (int(v) for v in frame_hw)
    plan = AugmentPlan.identity(B, (H, W))
    plan.key[:] = rng.integers(0, 1 << 32, size=B, dtype=np.uint64).astype(np.uint32)
    if change_bg is not None:
        swap = (rng.random(B) < float(change_bg)) if np.ndim(change_bg) == 0 else np.asarray(change_bg, dtype=bool).reshape(-1)
        if swap.shape[0] != B:
            raise ValueError("change_bg: one flag per sample")
        if swap.any() and n_bg <= 0:
            raise ValueError("sample_plan: a background swap needs n_bg > 0")
        pick = rng.integers(0, max(int(n_bg), 1), size=B)
        plan.bg_index[:] = np.where(swap, pick, -1)
    uni = lambda lo, hi: (lambda n: rng.uniform(lo, hi, size=n))      # noqa: E731
    for b in range(B):
        if not rng.random() < color_aug_prob:
            continue
        plan.color_on[b] = 1
        ops = {}
        if use_peper_salt and rng.random() < P_SP:
            plan.sp_on[b], plan.sp_thresh[b] = 1, threshold_u32(SP_P)
        if use_motion_blur and rng.random() < P_MOTION:
            plan.angle[b], plan.direction[b] = rng.uniform(0.0, 360.0), rng.uniform(-1.0, 1.0)
            plan.motion_on[b], plan.motion_w[b] = 1, motion_weights(plan.angle[b], plan.direction[b])
        if rng.random() < P_DROP:
            plan.drop_on[b], plan.drop_thresh[b] = 1, threshold_u32(DROP_P)
        if rng.random() < P_GAUSS:
            plan.sigma[b] = rng.random()                    # `sigma = np.random.rand()`, drawn anew at every build_augmentations call
            if plan.sigma[b] >= 1e-3:
                plan.gauss_on[b], plan.gauss_w[b] = 1, gaussian_weights(plan.sigma[b])
        if rng.random() < P_ADD:
            plan.add_on[b] = 1
            plan.add[b] = ops["add"] = _per_channel(rng, ADD_PER_CHANNEL, lambda n: rng.integers(ADD_RANGE[0], ADD_RANGE[1] + 1, size=n))
        if rng.random() < P_INVERT:
            plan.invert_on[b] = 1
            plan.invert[b] = ops["invert"] = rng.random(3) < INVERT_P       # per_channel=True: every channel has its own draw
        if rng.random() < P_MUL_PC:
            plan.mul_pc_on[b] = 1
            plan.mul_pc[b] = ops["mul_pc"] = _per_channel(rng, MUL_PER_CHANNEL, uni(*MUL_RANGE))
        if rng.random() < P_MUL:
            plan.mul_on[b] = 1
            plan.mul[b] = ops["mul"] = rng.uniform(*MUL_RANGE)
        if rng.random() < P_CONTRAST:
            plan.contrast_on[b] = 1
            plan.contrast[b] = ops["contrast"] = _per_channel(rng, CONTRAST_PER_CHANNEL, uni(*CONTRAST_RANGE))
        plan.lut[b] = compose_lut(**ops)
    return plan


def pack_plan(plan, img_index, rects=None):
    """the device blob of cp_augment_frames (layout: include/checkerpose_hip.h) -> uint8 array of cp_augment_plan_bytes(B) bytes"""
    B = plan.B
    rec = np.zeros((B, _REC_BYTES // 4), dtype=np.int32)
    ident = (plan.lut == _IDENTITY_LUT[None]).all((1, 2))
    flags = (F_SP * (plan.sp_on != 0) + F_MOTION * (plan.motion_on != 0) + F_DROP * (plan.drop_on != 0) + F_GAUSS * (plan.gauss_on != 0)
             + F_LUT * ~ident).astype(np.int32)
    rec[:, 0] = plan.key.astype(np.uint32).view(np.int32)
    rec[:, 2] = plan.bg_index
    rec[:, 3] = img_index
    rec[:, 4] = plan.sp_thresh.astype(np.uint32).view(np.int32)
    rec[:, 5] = plan.drop_thresh.astype(np.uint32).view(np.int32)
    rec[:, 6:8] = plan.drop_grid
    if rects is not None:
        flags |= F_RECT
        rec[:, 8:12] = rects
    rec[:, 1] = flags
    rec[:, 12:17] = plan.gauss_w
    rec[:, 17:42] = plan.motion_w
    rec[:, _REC_WORDS:] = np.ascontiguousarray(plan.lut).reshape(B, 768).view(np.int32)
    return np.concatenate([sp_value_table(), rec.view(np.uint8).reshape(-1)])


def augment_frames(frames, plan, masks=None, backgrounds=None, img_index=None, rects=None, out=None):
    """Apply an AugmentPlan to frames resident on the device, one launch (cp_augment_frames).
      frames uint8 (n_img,H,W,3) / (H,W,3), addressed through img_index (B,) as in preprocess.get_roi_batch (default: frame b, or the
      only frame); masks uint8 (n_img,H,W) / (H,W): the visible masks, needed where any bg_index >= 0 (non-zero keeps the frame's
      pixel: replace_bg's `im[~mask.astype(bool)] = bg[...]`); backgrounds uint8 (n_bg,H,W,3), already at frame size; rects: optional
      int (B,4) x1, y1, x2, y2 (half open) -- 64 x 32 tiles that do not meet a sample's rect are not computed and the output there is
      unspecified (for the crop that follows); out: optional uint8 (B,H,W,3) result tensor.
    Per sample: background swap -> salt and pepper -> motion blur -> coarse dropout -> Gaussian blur -> the composed table, each step
    giving uint8 before the next (steps and rounding: csrc/augment.hip).  H, W >= 5.  -> uint8 (B,H,W,3) on the frames' device."""
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8):
        raise RuntimeError(_NO_CPU + ": frames must be a uint8 CUDA tensor")
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError("augment_frames: frames (n_img, H, W, 3), contiguous")
    n_img, H, W = (int(v) for v in frames.shape[:3])
    if H < 5 or W < 5:
        raise ValueError("augment_frames: frames of at least 5 x 5 pixels (four mirrored halo pixels), got %d x %d" % (H, W))
    dev, B = frames.device, plan.B
    if img_index is None:
        if n_img not in (1, B):
            raise ValueError("augment_frames: img_index is needed when %d samples come from %d frames" % (B, n_img))
        idx = np.zeros(B, dtype=np.int32) if n_img == 1 else np.arange(B, dtype=np.int32)
    else:
        idx = np.asarray(img_index.detach().cpu() if torch.is_tensor(img_index) else img_index, dtype=np.int32).reshape(-1)
        if idx.shape[0] != B or (B and (idx.min() < 0 or idx.max() >= n_img)):
            raise ValueError("augment_frames: img_index must hold one valid frame number per sample")
    n_bg = 0
    if (plan.bg_index >= 0).any():
        if masks is None or backgrounds is None:
            raise ValueError("augment_frames: the plan swaps backgrounds (bg_index >= 0): masks and backgrounds are needed")
    if masks is not None:
        if not (torch.is_tensor(masks) and masks.is_cuda and masks.dtype == torch.uint8):
            raise RuntimeError(_NO_CPU + ": masks must be a uint8 CUDA tensor")
        masks = (masks.unsqueeze(0) if masks.dim() == 2 else masks).contiguous()
        if tuple(masks.shape) != (n_img, H, W):
            raise ValueError("augment_frames: masks must be (n_img, H, W) like the frames")
    if backgrounds is not None:
        if not (torch.is_tensor(backgrounds) and backgrounds.is_cuda and backgrounds.dtype == torch.uint8):
            raise RuntimeError(_NO_CPU + ": backgrounds must be a uint8 CUDA tensor")
        backgrounds = (backgrounds.unsqueeze(0) if backgrounds.dim() == 3 else backgrounds).contiguous()
        if backgrounds.dim() != 4 or tuple(backgrounds.shape[1:]) != (H, W, 3) or backgrounds.shape[0] < 1:
            raise ValueError("augment_frames: backgrounds must be (n_bg, H, W, 3), at the frames' size")
        n_bg = int(backgrounds.shape[0])
    if B and int(plan.bg_index.max()) >= max(n_bg, 1) and (plan.bg_index >= 0).any():
        raise ValueError("augment_frames: bg_index %d is outside the pool of %d backgrounds" % (int(plan.bg_index.max()), n_bg))
    if (plan.gauss_w.sum(1) != 4096).any() or (plan.motion_w.sum(1) != 65536).any() or (plan.gauss_w < 0).any() or (plan.motion_w < 0).any():
        raise ValueError("augment_frames: gauss_w rows must be non-negative and sum to 4096, motion_w rows to 65536")
    if (plan.drop_grid < 1).any():
        raise ValueError("augment_frames: drop_grid must be positive")
    if rects is not None:
        rects = np.asarray(rects.detach().cpu() if torch.is_tensor(rects) else rects, dtype=np.int64).reshape(-1, 4)
        if rects.shape[0] != B:
            raise ValueError("augment_frames: rects (B, 4) x1, y1, x2, y2")
        rects = np.clip(rects, -1, max(H, W) + 1).astype(np.int32)
    if out is None:
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    elif not (torch.is_tensor(out) and tuple(out.shape) == (B, H, W, 3) and out.dtype == torch.uint8 and out.is_contiguous() and out.device == dev):
        raise ValueError("augment_frames: out must be a contiguous uint8 (B, H, W, 3) tensor on the frames' device")
    if B == 0:
        return out
    lib = _abi.load()
    blob = pack_plan(plan, idx, rects)
    assert blob.nbytes == lib.cp_augment_plan_bytes(B)
    blob_t = torch.from_numpy(blob).to(dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _abi.check(lib.cp_augment_frames(st, frames.data_ptr(), n_img, H, W, masks.data_ptr() if masks is not None else None,
                                         backgrounds.data_ptr() if backgrounds is not None else None, n_bg, blob_t.data_ptr(), B,
                                         out.data_ptr()), "cp_augment_frames")
    return out                                # (blob_t may be freed: torch's allocator reuses a block in stream order)
