"""Predicted masks pasted into the frame on the device (csrc/paste_masks.hip).

The network's fourth output, `seg` (B,2,S,S) fp32 logits -- channel 0 the visible mask, channel 1 the full one, at crop resolution --
brought back into its photograph as the operands of row N15 (coco_eval): PackedMasks bit rows (paste_masks) or the column-major RLE
(paste_masks_rle), straight from the logits and the crop windows; no dense mask exists anywhere.  estimate_poses_masks is
postprocess.estimate_poses that also returns the masks of its ONE forward.  The three are reached as postprocess.paste_masks,
postprocess.paste_masks_rle and postprocess.estimate_poses_masks; coco_eval.segmentation_results builds the BOP'22 result dicts.
The rule is the project's own (the reference never pastes a mask), stated at the top of the kernel file and restated in numpy by
tests/paste_stages.py.  No CPU fallback: CPU tensors raise."""
import numpy as np
import torch

from . import _abi

PASTE_METHODS = ("crop_square_resize", "crop_resize")
PASTE_MAX_CELLS, PASTE_MAX_FRAME = 128, 4096        # csrc/paste_masks.hip: PM_SMAX, PM_FMAX


def _check_paste_method(resize_method):
    if resize_method == "crop_resize_by_warp_affine":
        raise NotImplementedError("crop_resize_by_warp_affine has no window: masks are pasted for 'crop_square_resize' and 'crop_resize'")
    if resize_method not in PASTE_METHODS:
        raise NotImplementedError("unknown decoder type: %s" % (resize_method,))


def _paste_inputs(seg, Bboxes, frame_size, resize_method, channel):
    """paste_masks' arguments checked -> (plane (B,Sh,Sw) view or copy with a contiguous plane, its stride in floats, windows (B,6)
    int32 on the device or None for B == 0, B, Sh, Sw, H, W)"""
    from . import preprocess as PP
    _check_paste_method(resize_method)
    if not torch.is_tensor(seg) or seg.dim() != 4 or seg.dtype != torch.float32:
        raise ValueError("seg must be the (B,C,Sh,Sw) float32 logits of the segmentation head")
    B, C_, Sh, Sw = (int(v) for v in seg.shape)
    if not (1 <= Sh <= PASTE_MAX_CELLS and 1 <= Sw <= PASTE_MAX_CELLS):
        raise ValueError("seg planes of 1..%d cells per side, got %dx%d" % (PASTE_MAX_CELLS, Sh, Sw))
    if isinstance(channel, bool) or not isinstance(channel, (int, np.integer)) or channel not in (0, 1) or channel >= C_:
        raise ValueError("channel is 0 (visible) or 1 (full) and below seg's %d channel(s), got %r" % (C_, channel))
    try:
        H, W = (int(v) for v in frame_size)
        exact = (H, W) == tuple(frame_size)
    except (TypeError, ValueError):
        raise ValueError("frame_size must be (H, W), got %r" % (frame_size,)) from None
    if not exact or not (1 <= H <= PASTE_MAX_FRAME and 1 <= W <= PASTE_MAX_FRAME):
        raise ValueError("frame_size (H, W) of whole numbers in 1..%d, got %r" % (PASTE_MAX_FRAME, frame_size))
    if len(Bboxes) != B:
        raise ValueError("%d boxes for %d seg planes" % (len(Bboxes), B))
    for box in Bboxes:
        if box is not None and len(box) != 4:
            raise ValueError("a box is (x, y, w, h) or None, got %r" % (box,))
    if not seg.is_cuda:
        raise RuntimeError("checkerpose_amd.paste: CUDA/HIP tensors required (no CPU fallback)")
    plane = seg[:, int(channel)]                          # taken through its strides where the channel plane is contiguous
    if not ((plane.stride(2) == 1 or Sw == 1) and (plane.stride(1) == Sw or Sh == 1) and (plane.stride(0) >= 0 or B <= 1)):
        plane = plane.contiguous()
    bstride = int(plane.stride(0)) if B > 1 else Sh * Sw
    win = torch.from_numpy(PP._windows(Bboxes, resize_method, W, H)).to(seg.device) if B else None
    return plane, bstride, win, B, Sh, Sw, H, W


def paste_masks(seg, Bboxes, frame_size, resize_method="crop_square_resize", channel=0):
    """Row N27 (cp_paste_masks): the network's predicted masks pasted back into their photograph, as coco_eval.PackedMasks -- the
    operand of mask_ious, CocoSet, evaluate, rle_encode -- without a dense mask anywhere.
      seg: the CUDA tensor (B,C,Sh,Sw) of fp32 logits as the module returns it (taken through its strides where the channel's plane is
      contiguous, copied otherwise); Bboxes: the (B,4) ALREADY padded boxes (x, y, w, h) get_roi_batch cut the crops from, None = an
      empty mask; frame_size: (H, W); resize_method: "crop_square_resize" or "crop_resize" ("crop_resize_by_warp_affine":
      NotImplementedError); channel: 0 the visible mask, 1 the full one.
    The rule (the project's own, stated at the top of csrc/paste_masks.hip): the integer, pixel-centre inverse of the crop window.  The
    visible mask's `box` is the tight modal box of the detection."""
    from . import coco_eval
    plane, bstride, win, B, Sh, Sw, H, W = _paste_inputs(seg, Bboxes, frame_size, resize_method, channel)
    dev = seg.device
    bits = torch.empty((B, H, (W + 31) // 32), dtype=torch.int32, device=dev)
    area = torch.empty((B,), dtype=torch.int32, device=dev)
    box = torch.empty((B, 4), dtype=torch.int32, device=dev)
    if B:
        _abi.call("cp_paste_masks", dev, plane, bstride, Sh, Sw, win, B, H, W, bits, area, box)
    return coco_eval.PackedMasks(bits, area, box, H, W)


def paste_masks_rle(seg, Bboxes, frame_size, resize_method="crop_square_resize", channel=0):
    """paste_masks' masks as pycoco_utils.binary_mask_to_rle's run lengths, straight from the logits and the windows
    (cp_paste_rle_count / cp_paste_rle_write: no frame-sized bits are stored; equal to coco_eval.rle_encode(paste_masks(...))).
    -> (counts int32 (total,), offsets int64 (B + 1,), area int32 (B,), box int32 (B,4) xmin ymin xmax ymax, -1s when empty) on the
    device: rle_encode's layout plus annotate_masks' area and box."""
    plane, bstride, win, B, Sh, Sw, H, W = _paste_inputs(seg, Bboxes, frame_size, resize_method, channel)
    dev = seg.device
    n_runs = torch.empty((B,), dtype=torch.int32, device=dev)
    area = torch.empty((B,), dtype=torch.int32, device=dev)
    box = torch.empty((B, 4), dtype=torch.int32, device=dev)
    offsets = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
    if B == 0:
        return torch.empty((0,), dtype=torch.int32, device=dev), offsets, area, box
    _abi.call("cp_paste_rle_count", dev, plane, bstride, Sh, Sw, win, B, H, W, n_runs, area, box)
    offsets[1:] = torch.cumsum(n_runs, 0)
    total = int(offsets[-1])
    counts = torch.empty((total,), dtype=torch.int32, device=dev)
    _abi.call("cp_paste_rle_write", dev, plane, bstride, Sh, Sw, win, B, H, W, offsets, counts, total)
    return counts, offsets, area, box


def estimate_poses_masks(net, frames, Bboxes, p3d_xyz, cam_K, channel=0, **estimate_kwargs):
    """estimate_poses (estimate_kwargs are its keywords) that also returns the predicted masks of the same crops pasted into the
    frames (row N27): ONE forward, its `seg` output goes through paste_masks with the crops' own padded boxes and resize_method.
    -> (R, t, inliers, status, final boxes) as estimate_poses, bit for bit, plus the coco_eval.PackedMasks of channel `channel`."""
    from . import postprocess
    _check_paste_method(estimate_kwargs.get("resize_method", "crop_square_resize"))
    keep = {}
    stages, inl, status, final = postprocess._estimate_stages(net, frames, Bboxes, p3d_xyz, cam_K, keep=keep, **estimate_kwargs)
    H, W = (int(v) for v in frames.shape[-3:-1])
    masks = paste_masks(keep["seg"], keep["padded"], (H, W), estimate_kwargs.get("resize_method", "crop_square_resize"), channel)
    return stages[-1][1], stages[-1][2], inl, status, final, masks
