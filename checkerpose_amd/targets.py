"""Ground-truth side on the device: the labels of the reference's data loader and the code / mask figures of its
test loop, without a host round trip per sample.

The reference makes the training labels one sample at a time inside `bop_dataset_pytorch.py` (`project_pts` :21-36, the statements
:356-380 of `__getitem__`, `aug_Bbox` :165-185 and the two INTER_NEAREST mask crops :302-320; `lm_dataset_pytorch.py:393,438-462` with
a per-sample object) and turns them into `roi_bit_acc`, `reproj_x_acc`, `bit_err_arr`, the mask accuracies / IoUs and `re` / `te`
per crop in Python (`test.py:388-389,432-457`).  Here:

  encode_targets       keypoints + K, R, t + the crops' final boxes -> roi_mask_bits / pixel_x_codes / pixel_y_codes (cp_encode_targets)
  make_training_batch  frames + masks + GT poses + boxes -> the loader's tuple for a batch (get_roi_batch x 3 + encode_targets)
  batch_from_frames    its body, with the two mask crops as an argument (render.scene_training_batch cuts them from bit planes)
  code_report          network outputs + labels + GT mask crops -> test.py's per-crop code / mask figures and their integer counts
  pose_re_te           bop_toolkit_lib.pose_error.re / te, batched
  evaluate_batch       frames + boxes + GT -> everything test.py scores per crop; summarize_report -> its score lines
  pose_re_te_sym       re against the closest symmetric ground truth (test_lm.py's get_closest_rot) + te, one launch (cp_pose_rete; row N23)
  summarize_report_lm  test_lm.py's score file over the 13 LINEMOD objects: rete_pass_counts (cp_rete_pass_counts) + lm_report_text

No CPU fallback: CPU tensors raise, as in `preprocess` / `postprocess`."""
import numpy as np
import torch

from . import _abi
from . import preprocess as PP

_NO_CPU = "checkerpose_amd.targets: CUDA/HIP tensors required (no CPU fallback)"


def aug_Bbox(GT_Bbox, padding_ratio):
    """the training loader's box jitter (bop_dataset_pytorch.py:165-185): the box scaled by 1 +- 0.25 and `padding_ratio`, its centre
    moved by up to a quarter of its size.  Draws from `np.random` exactly as the reference does -- one `random_sample()` for the scale,
    then one `random_sample(2)` for the shift -- so the same `np.random.seed` gives the reference's box.  -> int array (x, y, w, h)"""
    x, y, w, h = (GT_Bbox[k] for k in range(4))
    cx, cy = 0.5 * (x + (x + w)), 0.5 * (y + (y + h))
    bw, bh = (x + w) - x, (y + h) - y
    scale = 1 + 0.25 * (2 * np.random.random_sample() - 1)
    shift = 0.25 * (2 * np.random.random_sample(2) - 1)
    ax, ay = cx + bw * shift[0], cy + bh * shift[1]
    aw, ah = int(bw * scale * padding_ratio), int(bh * scale * padding_ratio)
    return np.array([int(ax - aw / 2), int(ay - ah / 2), aw, ah])


def _device_of(*xs):
    dev = None
    for x in xs:
        if torch.is_tensor(x):
            if not x.is_cuda:
                raise RuntimeError(_NO_CPU)
            dev = dev or x.device
    if dev is None:
        raise RuntimeError(_NO_CPU + ": give at least one of the arguments as a tensor on the device")
    return dev


def _f64(x, dev):
    if torch.is_tensor(x):
        if not x.is_cuda:
            raise RuntimeError(_NO_CPU)
        return x.detach().to(device=dev, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(dev)


def _host_boxes(final_Bboxes):
    """-> ((B,4) int32 array with the dummy box (0,0,0,0) for a missing detection, (B,) uint8 flags)"""
    if torch.is_tensor(final_Bboxes):
        final_Bboxes = final_Bboxes.detach().cpu().numpy()
    B = len(final_Bboxes)
    boxes, flags = np.zeros((B, 4), dtype=np.int32), np.zeros(B, dtype=np.uint8)
    for b, box in enumerate(final_Bboxes):
        if box is None:
            flags[b] = 1
        else:
            boxes[b] = [int(v) for v in box]
    return boxes, flags


def encode_targets(p3d_xyz, cam_K, R, t, final_Bboxes, crop_size_gt=64, obj_ids=None, return_proj=False):
    """The loader's labels for a batch of crops, one launch (cp_encode_targets; bop_dataset_pytorch.py:293,356-380).
      p3d_xyz: keypoints in original units, (N,3) shared, (B,N,3) per crop, or -- with `obj_ids` (B,) 1-based, the LM loader's
      `unnorm_xyz[obj_id-1]` -- the object table (n_obj,N,3); cam_K (3,3) / (B,3,3); R (B,3,3); t (B,3) / (B,3,1): tensors on the
      device or host arrays (uploaded as float64; at least one argument must be a device tensor);
      final_Bboxes: (B,4) x, y, w, h of `preprocess.get_final_Bbox`, host array / list (None = no detection: all-zero labels, the
      loader's dummy :328-338) or an integer tensor; crop_size_gt: a power of two in 8 .. 256.
    A box with w <= 0 or h <= 0 that is not a missing detection raises before anything is launched.  The arithmetic is the
    reference's in float64; the float -> int conversion saturates where numpy's is undefined (quotients beyond the int range), a NaN
    quotient counts as outside the RoI.
    -> dict of device tensors: roi_mask_bits (B,1,N) f32, pixel_x_codes / pixel_y_codes (B,bits,N) f32 in {0,1} MSB first, x_id / y_id
    (B,N) int32 (after the clip to [0, S-1]); with return_proj also proj_xy (B,N,2) and depth (B,N) float64."""
    dev = _device_of(p3d_xyz, cam_K, R, t)
    boxes, flags = _host_boxes(final_Bboxes)
    B = boxes.shape[0]
    p3 = _f64(p3d_xyz, dev)
    K, Rm, tv = _f64(cam_K, dev), _f64(R, dev).reshape(-1, 3, 3), _f64(t, dev).reshape(-1, 3)
    S = int(crop_size_gt)
    if S < 8 or S > 256 or S & (S - 1):
        raise ValueError("crop_size_gt must be a power of two in 8 .. 256, got %r" % (crop_size_gt,))
    if Rm.shape[0] != B or tv.shape[0] != B or K.shape[-2:] != (3, 3) or K.dim() not in (2, 3) or (K.dim() == 3 and K.shape[0] != B):
        raise ValueError("R (B,3,3), t (B,3) and cam_K (3,3) / (B,3,3) must match the %d boxes" % B)
    ids_t, n_obj = None, 0
    if obj_ids is not None:
        ids = (obj_ids.detach().cpu().numpy() if torch.is_tensor(obj_ids) else np.asarray(obj_ids)).astype(np.int64).reshape(-1)
        if p3.dim() != 3 or ids.shape[0] != B or (B and (ids.min() < 1 or ids.max() > p3.shape[0])):
            raise ValueError("obj_ids: one 1-based row of the (n_obj,N,3) keypoint table per crop")
        ids_t, n_obj = torch.from_numpy(ids.astype(np.int32)).to(dev), int(p3.shape[0])
        bstride = 0
    elif p3.dim() == 3:
        if p3.shape[0] != B:
            raise ValueError("p3d_xyz (B,N,3) must have one keypoint set per box (or give obj_ids for an object table)")
        bstride = 3 * int(p3.shape[1])
    elif p3.dim() == 2:
        bstride = 0
    else:
        raise ValueError("p3d_xyz must be (N,3), (B,N,3) or (n_obj,N,3)")
    if p3.shape[-1] != 3:
        raise ValueError("p3d_xyz must end in 3 coordinates")
    N, bits = int(p3.shape[-2]), S.bit_length() - 1
    bad = [b for b in range(B) if not flags[b] and (boxes[b, 2] <= 0 or boxes[b, 3] <= 0)]
    if bad:
        raise ValueError("final_Bboxes: boxes %r have no area (w <= 0 or h <= 0) and are not marked as missing detections (None)" % bad)
    out = {"roi_mask_bits": torch.empty(B, 1, N, dtype=torch.float32, device=dev),
           "pixel_x_codes": torch.empty(B, bits, N, dtype=torch.float32, device=dev),
           "pixel_y_codes": torch.empty(B, bits, N, dtype=torch.float32, device=dev),
           "x_id": torch.empty(B, N, dtype=torch.int32, device=dev), "y_id": torch.empty(B, N, dtype=torch.int32, device=dev)}
    if return_proj:
        out["proj_xy"] = torch.empty(B, N, 2, dtype=torch.float64, device=dev)
        out["depth"] = torch.empty(B, N, dtype=torch.float64, device=dev)
    if B == 0:
        return out
    boxes_t = torch.from_numpy(boxes).to(dev)
    lib = _abi.load()
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _abi.check(lib.cp_encode_targets(st, p3.data_ptr(), bstride, ids_t.data_ptr() if ids_t is not None else None, n_obj,
                                         K.data_ptr(), 9 if K.dim() == 3 else 0, Rm.data_ptr(), tv.data_ptr(), boxes_t.data_ptr(),
                                         boxes.ctypes.data, flags.ctypes.data, B, N, S, out["roi_mask_bits"].data_ptr(),
                                         out["pixel_x_codes"].data_ptr(), out["pixel_y_codes"].data_ptr(), out["x_id"].data_ptr(),
                                         out["y_id"].data_ptr(), out["proj_xy"].data_ptr() if return_proj else None,
                                         out["depth"].data_ptr() if return_proj else None), "cp_encode_targets")
    return out


def roi_xy_grid(final_Bboxes, crop_size_gt, device):
    """`mapping_pixel_position_to_original_position_2d` (bop_dataset_pytorch.py:223-235) of the loader's pixel grid for a batch:
    (B,2,S,S) f32, [x | y] original-image coordinates of every crop pixel (float64 product and sum, then the cast); zeros for a
    missing detection"""
    boxes, flags = _host_boxes(final_Bboxes)
    bx = torch.from_numpy(boxes.astype(np.float64)).to(device)
    keep = torch.from_numpy(1.0 - flags.astype(np.float64)).to(device)
    S = int(crop_size_gt)
    px = torch.arange(S, dtype=torch.float64, device=device)
    gx = ((bx[:, 2:3] / S) * px[None] + bx[:, 0:1]) * keep[:, None]                # (B,S)
    gy = ((bx[:, 3:4] / S) * px[None] + bx[:, 1:2]) * keep[:, None]
    return torch.stack([gx[:, None, :].expand(-1, S, -1), gy[:, :, None].expand(-1, -1, S)], 1).float().contiguous()


def _mask_images(m):
    if not (torch.is_tensor(m) and m.is_cuda and m.dtype == torch.uint8):
        raise RuntimeError("checkerpose_amd.targets: masks must be uint8 CUDA tensors (n_img, H, W) or (H, W), 0 / 255 (no CPU path)")
    if m.dim() == 2:
        m = m[None]
    return m.contiguous().unsqueeze(-1)


def make_training_batch(frames, masks_visib, masks_full, R, t, cam_K, Bboxes, p3d_xyz, is_train=True, padding_ratio=1.5,
                        crop_size_img=256, crop_size_gt=64, resize_method="crop_square_resize", img_index=None, obj_ids=None,
                        augment=None, backgrounds=None):
    """What the reference's loader returns for the samples of a batch (`__getitem__`, bop_dataset_pytorch.py:274-383), made on the
    device from full frames: `aug_Bbox` (is_train; it draws from np.random) or `padding_Bbox` per box on the host -> three
    `preprocess.get_roi_batch` launches (image INTER_LINEAR at crop_size_img, the two masks INTER_NEAREST at crop_size_gt, then / 255
    as `transform_pre` :393-396) -> `get_final_Bbox` -> `encode_targets`.
      frames uint8 (n_img,H,W,3) / (H,W,3); masks_visib, masks_full uint8 (n_img,H,W) / (H,W) with 0 / 255; R (B,3,3), t (B,3) /
      (B,3,1), cam_K (3,3) / (B,3,3); Bboxes (B,4) x, y, w, h (`bbox_visib`, or the detections when is_train is False: None = no
      detection -> the loader's dummy sample); p3d_xyz / obj_ids as in encode_targets; img_index: the frame of each box.
    -> (roi_x uint8 (B,crop,crop,3), roi_entire_mask (B,S,S) f32, roi_mask (B,S,S) f32, R, t, Bbox (B,4) int32 tensor (the FINAL box),
        cam_K (R, t, cam_K as float64 device tensors in the shapes given; host arrays are uploaded), roi_mask_bits (B,1,N), pixel_x_codes (B,bits,N), pixel_y_codes (B,bits,N), roi_xy_oris (B,2,S,S) f32) -- the loader's 11
    entries in its order, every one a tensor on the frames' device; with obj_ids, `obj_ids` (int64 (B,)) follows cam_K as in the LM
    loader (12 entries).
    The image stays uint8: the models normalise on the device (ToTensor + Normalize, cp_u8hwc_to_nhwc_norm).
    augment: an `augment.AugmentPlan` of B samples (`augment.sample_plan`), or None.  With a plan the frames go through
    `augment.augment_frames` first -- the LM loader's background replacement (`replace_bg`, against masks_visib, from the pool
    `backgrounds` uint8 (n_bg,H,W,3)) and the colour chain (`apply_augmentation`) -- computed only on the tiles that meet each
    sample's crop window, and roi_x is cut from the augmented frames; the mask crops and every other entry are unaffected.  With None
    (the default) nothing is augmented and the launches are the ones listed above.  Parity of the chain with imgaug is UNPINNED
    (augment.py)."""
    if not (torch.is_tensor(frames) and frames.is_cuda):
        raise RuntimeError(_NO_CPU)
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    H, W = int(frames.shape[1]), int(frames.shape[2])
    mv, mf = _mask_images(masks_visib), _mask_images(masks_full)
    if tuple(mv.shape[1:3]) != (H, W) or tuple(mf.shape[1:3]) != (H, W):
        raise ValueError("masks must have the frames' height and width")
    crop_masks = lambda grown: (PP.get_roi_batch(mv, grown, crop_size_gt, PP.INTER_NEAREST, resize_method, img_index=img_index),      # noqa: E731
                                PP.get_roi_batch(mf, grown, crop_size_gt, PP.INTER_NEAREST, resize_method, img_index=img_index))
    return batch_from_frames(frames, crop_masks, R, t, cam_K, Bboxes, p3d_xyz, is_train, padding_ratio, crop_size_img, crop_size_gt,
                             resize_method, img_index, obj_ids, augment, backgrounds, mv[..., 0])


def batch_from_frames(frames, crop_masks, R, t, cam_K, Bboxes, p3d_xyz, is_train, padding_ratio, crop_size_img, crop_size_gt,
                      resize_method, img_index, obj_ids, augment, backgrounds, swap_masks):
    """The body of make_training_batch, shared with render.scene_training_batch: everything but where the two mask crops come from.
    frames: uint8 (n_img,H,W,3) on the device; crop_masks(grown boxes) -> (roi_mask, roi_entire), uint8 (B,S,S,1) INTER_NEAREST crops
    of the visible and the full masks, called after the image crop; swap_masks: uint8 (n_img,H,W) for a plan's background swap, or
    None when the plan asks for none.  The other arguments and the result are make_training_batch's."""
    H, W = int(frames.shape[1]), int(frames.shape[2])
    if is_train:
        if any(b is None for b in Bboxes):
            raise ValueError("a training sample needs its ground-truth box")
        grown = [aug_Bbox(np.asarray(b), padding_ratio) for b in Bboxes]
    else:
        grown = [None if b is None else PP.padding_Bbox(b, padding_ratio) for b in Bboxes]
    if augment is None:
        roi_x = PP.get_roi_batch(frames, grown, crop_size_img, PP.INTER_LINEAR, resize_method, img_index=img_index)
    else:
        from . import augment as AUG
        wins = np.zeros((len(grown), 4), dtype=np.int64)
        for b, box in enumerate(grown):
            if box is not None:                  # the window the crop reads (cp_crop_resize_u8 / cp_warp_affine_u8): [x1, x2) x [y1, y2) inside the frame
                wins[b] = PP.roi_window([int(v) for v in box], resize_method, W, H, crop_size_img)[:4]
        aug = AUG.augment_frames(frames, augment, masks=swap_masks, backgrounds=backgrounds, img_index=img_index, rects=wins)
        roi_x = PP.get_roi_batch(aug, grown, crop_size_img, PP.INTER_LINEAR, resize_method, img_index=np.arange(len(grown)))
    roi_mask, roi_entire = crop_masks(grown)
    final = [None if b is None else PP.get_final_Bbox(b, resize_method, W, H) for b in grown]
    lab = encode_targets(p3d_xyz, cam_K, R, t, final, crop_size_gt, obj_ids=obj_ids)
    dev = frames.device
    boxes, _ = _host_boxes(final)
    out = (roi_x, roi_entire[..., 0].float() / 255.0, roi_mask[..., 0].float() / 255.0, _f64(R, dev), _f64(t, dev),
           torch.from_numpy(boxes).to(dev), _f64(cam_K, dev))
    if obj_ids is not None:
        out = out + (torch.as_tensor(obj_ids).to(device=dev, dtype=torch.int64).reshape(-1),)
    return out + (lab["roi_mask_bits"], lab["pixel_x_codes"], lab["pixel_y_codes"], roi_xy_grid(final, crop_size_gt, dev))


def _rows(x, rows, N):
    """a (B,rows,N) f32 tensor whose rows are N apart and dense: as it is (any batch stride), or a contiguous copy"""
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(2) != 1 or (rows > 1 and x.stride(1) != N) or x.stride(0) < rows * N:
        x = x.contiguous()
    return x


def code_report(outputs, labels, masks_visib, masks_full):
    """The per-crop code and mask figures test.py prints beside ADD (:432-457), one launch for the batch (cp_code_report).
      outputs: the network's tuple (roi (B,1,N), x bits (B,nb,N), y bits (B,nb,N), seg (B,2,H,W) LOGITS, ...; nb may be below the
      labels' bits: a truncated `stage`); labels: encode_targets' dict (or any dict with roi_mask_bits / pixel_x_codes / pixel_y_codes);
      masks_visib / masks_full: the GT mask crops (B,S,S), uint8 (non-zero = set) or float (0 / 1, what make_training_batch returns),
      read at F.interpolate(mode="nearest") positions for the seg size (test.py:320-323).  Decisions are logit > 0.
    -> dict of device tensors: roi_bit_acc, reproj_x_acc, reproj_y_acc, visib_pixel_acc, visib_iou, full_pixel_acc, full_iou (B,) f64,
       bit_err_arr (B, 2 nb + 1) f64, and the integer counts they are quotients of (int32): n_in_roi, roi_bit_mismatch, x_id_abs_diff,
       y_id_abs_diff, {visib,full}_{mismatch,intersection,union} (B,), x_bit_mismatch / y_bit_mismatch (B,nb)."""
    roi, xb, yb, seg = outputs[0], outputs[1], outputs[2], outputs[3]
    g_roi, g_x, g_y = labels["roi_mask_bits"], labels["pixel_x_codes"], labels["pixel_y_codes"]
    for x in (roi, xb, yb, seg, g_roi, g_x, g_y, masks_visib, masks_full):
        if not (torch.is_tensor(x) and x.is_cuda):
            raise RuntimeError(_NO_CPU)
    dev = roi.device
    B, _, N = roi.shape
    nb, bits = int(xb.shape[1]), int(g_x.shape[1])
    if tuple(xb.shape) != (B, nb, N) or tuple(yb.shape) != (B, nb, N) or seg.dim() != 4 or seg.shape[0] != B or seg.shape[1] != 2:
        raise ValueError("outputs must be (roi (B,1,N), x bits (B,nb,N), y bits (B,nb,N), seg (B,2,H,W), ...)")
    if tuple(g_roi.shape) != (B, 1, N) or tuple(g_x.shape) != (B, bits, N) or tuple(g_y.shape) != (B, bits, N) or not 1 <= nb <= bits:
        raise ValueError("labels must be roi_mask_bits (B,1,N) and pixel_x_codes / pixel_y_codes (B,bits,N) with bits >= the %d predicted" % nb)
    S = int(masks_visib.shape[-1])
    if tuple(masks_visib.shape) != (B, S, S) or tuple(masks_full.shape) != (B, S, S) or masks_visib.dtype != masks_full.dtype:
        raise ValueError("masks_visib / masks_full must both be (B,S,S) crops of one dtype")
    if masks_visib.dtype == torch.uint8:
        mv, mf, mask_f32 = masks_visib.contiguous(), masks_full.contiguous(), 0
    else:
        mv, mf, mask_f32 = masks_visib.float().contiguous(), masks_full.float().contiguous(), 1
    H, W = int(seg.shape[2]), int(seg.shape[3])
    roi, xb, yb = _rows(roi, 1, N), _rows(xb, nb, N), _rows(yb, nb, N)
    seg = seg.detach().float().contiguous()
    g_roi, g_x, g_y = g_roi.float().contiguous(), g_x.float().contiguous(), g_y.float().contiguous()
    counts = torch.empty(B, 10 + 2 * nb, dtype=torch.int32, device=dev)
    fig = torch.empty(B, 8 + 2 * nb, dtype=torch.float64, device=dev)
    if B:
        lib = _abi.load()
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _abi.check(lib.cp_code_report(st, roi.data_ptr(), roi.stride(0), xb.data_ptr(), xb.stride(0), yb.data_ptr(), yb.stride(0), nb,
                                          seg.data_ptr(), H, W, g_roi.data_ptr(), g_x.data_ptr(), g_y.data_ptr(), bits, mv.data_ptr(),
                                          mf.data_ptr(), mask_f32, S, B, N, counts.data_ptr(), fig.data_ptr()), "cp_code_report")
    out = {k: fig[:, i] for i, k in enumerate(FIGURES)}
    out["bit_err_arr"] = fig[:, 7:]
    out.update({k: counts[:, i] for i, k in enumerate(COUNTS)})
    out["x_bit_mismatch"], out["y_bit_mismatch"] = counts[:, 10:10 + nb], counts[:, 10 + nb:]
    return out


FIGURES = ("roi_bit_acc", "reproj_x_acc", "reproj_y_acc", "visib_pixel_acc", "visib_iou", "full_pixel_acc", "full_iou")
COUNTS = ("n_in_roi", "roi_bit_mismatch", "x_id_abs_diff", "y_id_abs_diff", "visib_mismatch", "visib_intersection", "visib_union",
          "full_mismatch", "full_intersection", "full_union")


def figures_from_counts(counts, N, n_pixels, nb):
    """the float64 figures of code_report from its integer counts (host arrays), formed as test.py:433-457 forms them:
    counts: dict name -> (B,) / (B,nb) integer arrays -> dict name -> float64 arrays.  What the kernel computes, restated."""
    c = {k: np.asarray(v, dtype=np.float64) for k, v in counts.items()}
    npoint = np.maximum(c["n_in_roi"], 1.0)
    err_roi = c["roi_bit_mismatch"] / float(N)
    out = {"roi_bit_acc": 1.0 - err_roi,
           "reproj_x_acc": 1.0 - (c["x_id_abs_diff"] / npoint) / float(2 ** nb),
           "reproj_y_acc": 1.0 - (c["y_id_abs_diff"] / npoint) / float(2 ** nb),
           "bit_err_arr": np.concatenate([err_roi[:, None], c["x_bit_mismatch"] / npoint[:, None], c["y_bit_mismatch"] / npoint[:, None]], 1)}
    for m in ("visib", "full"):
        out[m + "_pixel_acc"] = 1.0 - c[m + "_mismatch"] / float(n_pixels)
        u = c[m + "_union"]
        out[m + "_iou"] = np.where(u < 1, 1.0, c[m + "_intersection"] / np.where(u < 1, 1.0, u))
    return out


def pose_re_te(R_est, t_est, R_gt, t_gt, return_cos=False):
    """`bop_toolkit_lib.pose_error.re` / `.te` (pose_error.py:187-214) for a batch, float64 on the device:
      re = acos(clamp((trace(R_est . inv(R_gt)) - 1) / 2, -1, 1)) in degrees -- with the inverse, not the transpose, as the reference
      has it (formed from the cofactors: 3 x 3; the trace is taken as 3 + trace((R_est - R_gt) . inv(R_gt)), so equal poses give
      exactly 0); te = |t_gt - t_est|.
    R_* (B,3,3), t_* (B,3) / (B,3,1): device tensors or host arrays (at least one a device tensor).  -> (re (B,), te (B,)); with
    return_cos also the reference's `error_cos` before the clamp."""
    dev = _device_of(R_est, t_est, R_gt, t_gt)
    Re, Rg = _f64(R_est, dev).reshape(-1, 3, 3), _f64(R_gt, dev).reshape(-1, 3, 3)
    te_, tg = _f64(t_est, dev).reshape(-1, 3), _f64(t_gt, dev).reshape(-1, 3)
    r0, r1, r2 = Rg[:, 0], Rg[:, 1], Rg[:, 2]
    cof = torch.stack([torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)], 1)     # rows = columns of adj
    det = (r0 * cof[:, 0]).sum(1)
    # trace(Re . inv(Rg)) = 3 + trace((Re - Rg) . adj / det), adj_ki = cof_ik: equal poses give cos = 1, i.e. 0 degrees, exactly
    cos = 1.0 + 0.5 * (((Re - Rg) * cof).sum((1, 2)) / det)
    re = torch.rad2deg(torch.acos(cos.clamp(-1.0, 1.0)))
    d = tg - te_
    te = torch.sqrt((d * d).sum(1))
    return (re, te, cos) if return_cos else (re, te)


def pose_re_te_sym(R_est, t_est, R_gt, t_gt, symmetries=None, mesh_ids=None, return_cos=False, return_index=False, return_closest=False):
    """`pose_error.re` / `.te` for a batch with the rotation error taken against the closest symmetric ground truth, as test_lm.py
    takes it (`get_closest_rot`, :33-55, then `pose_error.re(pred_rot, r_GT_sym)`, :309-310), one launch (cp_pose_rete; the rule is at
    the top of csrc/rete.hip).  The candidates are R_gt itself (index -1), then R_gt . S_k in the set's order; the first one with the
    smallest re wins; te = |t_gt - t_est| does not look at the symmetries.
      R_* (P,3,3), t_* (P,3) / (P,3,1): device tensors or host arrays (at least one a device tensor);
      symmetries: a scene.SymmetrySet, or per-mesh lists of {"R", "t"} as scene.as_symmetries takes them (only "R" is used); None =
      no symmetries, the plain re / te;  mesh_ids (P,): each pair's set among the M of `symmetries` (None with one set); ids on the
      host are checked here, ids on the device stay unread (an id outside 0 .. M-1 gives NaN and index -1).
    -> (re (P,) degrees, te (P,)), then in this order where asked: cos (the winner's `error_cos` before the clamp), index (int32: the
    winner's place in its set, -1 = R_gt itself), R_gt_sym (P,3,3) = what get_closest_rot returns."""
    from . import scene as SC
    dev = _device_of(R_est, t_est, R_gt, t_gt)
    Re, Rg = _f64(R_est, dev).reshape(-1, 3, 3), _f64(R_gt, dev).reshape(-1, 3, 3)
    te_, tg = _f64(t_est, dev).reshape(-1, 3), _f64(t_gt, dev).reshape(-1, 3)
    P = int(Re.shape[0])
    if Rg.shape[0] != P or te_.shape[0] != P or tg.shape[0] != P:
        raise ValueError("R_est, t_est, R_gt, t_gt must describe the same number of poses")
    A, Bp = torch.cat([Re.reshape(P, 9), te_], 1).contiguous(), torch.cat([Rg.reshape(P, 9), tg], 1).contiguous()
    tab = off = ids = None
    off_host = ids_host = None
    M = 0
    if symmetries is None:
        if mesh_ids is not None:
            raise ValueError("mesh_ids without symmetries")
    else:
        ss = symmetries if isinstance(symmetries, SC.SymmetrySet) else SC.SymmetrySet.from_transforms(symmetries)
        M = len(ss)
        tab, off = ss.on(dev)
        off_host = np.ascontiguousarray(ss.offsets.numpy(), dtype=np.int32)
        if mesh_ids is None:
            if M != 1:
                raise ValueError("mesh_ids: several symmetry sets need one id per pose")
        elif torch.is_tensor(mesh_ids) and mesh_ids.is_cuda:
            ids = mesh_ids.detach().to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        else:
            h = (mesh_ids.numpy() if torch.is_tensor(mesh_ids) else np.asarray(mesh_ids)).astype(np.int64).reshape(-1)
            if h.shape[0] == P and P and (h.min() < 0 or h.max() >= M):
                raise ValueError("mesh_ids must lie in 0 .. %d" % (M - 1))
            ids_host = np.ascontiguousarray(h, dtype=np.int32)
            ids = torch.from_numpy(ids_host).to(dev)
        if ids is not None and ids.shape[0] != P:
            raise ValueError("mesh_ids: one id per pose (%d), got %d" % (P, ids.shape[0]))
    re, te = torch.empty(P, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
    cos, idx = torch.empty(P, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
    if P:
        _abi.call("cp_pose_rete", dev, A, Bp, P, tab, off, None if off_host is None else off_host.ctypes.data, M, ids,
                  None if ids_host is None else ids_host.ctypes.data, re, te, cos, idx)
    out = (re, te) + ((cos,) if return_cos else ()) + ((idx,) if return_index else ())
    if return_closest:
        if tab is None:
            closest = Rg.clone()
        else:
            base = off.long()[ids.long()] if ids is not None else torch.zeros(P, dtype=torch.int64, device=dev)
            S = tab[:, :9].reshape(-1, 3, 3)[(base + idx.long().clamp(min=0)).clamp(max=tab.shape[0] - 1)]
            closest = torch.where((idx >= 0)[:, None, None], torch.matmul(Rg, S), Rg)
        out = out + (closest,)
    return out


LM13_OBJ_IDS = (1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15)      # LINEMOD's 13 objects (3 and 7 are not evaluated)
LM_SYMMETRIC_OBJ_IDS = (10, 11, 7, 3)
RETE_COUNTS = ("n", "adx2", "adx5", "adx10", "rete2", "rete5", "re2", "re5", "te2", "te5")


def rete_pass_counts(re, te, adx, diameters, slots, n_obj):
    """The integer pass counts of test_lm.py:306-327 per object slot, one launch (cp_rete_pass_counts): re, te, adx, diameters (P,)
    float64 and slots (P,) in 0 .. n_obj-1 (device tensors or host arrays, at least one on the device; host slots are checked).
    -> (n_obj, 10) int32 device tensor, columns RETE_COUNTS; NaN counts as 10000, every `<` is strict."""
    dev = _device_of(re, te, adx, diameters, slots)
    r, t, a, d = (_f64(x, dev).reshape(-1) for x in (re, te, adx, diameters))
    P, n_obj = int(r.shape[0]), int(n_obj)
    if not 1 <= n_obj <= 256:
        raise ValueError("n_obj must be in 1 .. 256, got %r" % (n_obj,))
    slot_host = None
    if torch.is_tensor(slots) and slots.is_cuda:
        sl = slots.detach().to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    else:
        h = (slots.numpy() if torch.is_tensor(slots) else np.asarray(slots)).astype(np.int64).reshape(-1)
        if h.size and (h.min() < 0 or h.max() >= n_obj):
            raise ValueError("slots must lie in 0 .. %d" % (n_obj - 1))
        slot_host = np.ascontiguousarray(h, dtype=np.int32)
        sl = torch.from_numpy(slot_host).to(dev)
    if not (t.shape[0] == a.shape[0] == d.shape[0] == sl.shape[0] == P):
        raise ValueError("re, te, adx, diameters and slots must have one entry per pose")
    counts = torch.zeros(n_obj, len(RETE_COUNTS), dtype=torch.int32, device=dev)
    if P == 0:
        return counts
    _abi.call("cp_rete_pass_counts", dev, r, t, a, d, sl, None if slot_host is None else slot_host.ctypes.data, P, n_obj, counts)
    return counts


COLUMNS =("all", "full", "visib")          # correspondences()' validity columns: RoI bit | also in the full mask | in the visible mask


def evaluate_batch(net, frames, masks_visib, masks_full, Bboxes, p3d_xyz, cam_K, R_gt, t_gt, vertices, mesh_ids=None,
                   kinds=("add", "adi"), img_index=None, obj_ids=None, padding_ratio=1.5, crop_size=256, crop_size_gt=64,
                   resize_method="crop_square_resize", discard_bd_pixel=0, reproj_threshold=2.0, iterations=150, seed=0,
                   symmetries=None, depth_test=None, image_ids=None, size=None, re_symmetries=None):
    """test.py's loop body for a batch (:279-457), everything it scores per crop, without leaving the device: what
    `postprocess.evaluate_poses` does -- crops, ONE forward, correspondences, EPnP + RANSAC, ADD / ADD-S -- for the three correspondence
    sets the reference scores (all RoI keypoints | inside the predicted full mask | inside the visible mask, :335-368), plus `re` / `te`
    of each pose (called as test.py calls them, ground truth first: for rotation matrices the same angle up to rounding) and the code / mask report against labels made from the GT pose on the crops' final boxes.
      frames / masks_visib / masks_full / Bboxes (detections; None = no detection) / p3d_xyz / obj_ids / cam_K as in
      make_training_batch(is_train=False); R_gt, t_gt, vertices, mesh_ids, kinds, symmetries, depth_test, image_ids as in
      postprocess.evaluate_poses (kind "vsd" needs depth_test; "cus" / "cou_bb_proj" need size = (W, H)).
      re_symmetries: None, or what pose_re_te_sym takes as `symmetries` (with mesh_ids choosing each crop's set): then each column's
      "re" is the error against the closest symmetric ground truth in test_lm.py's order (:309-310, the estimate first) and
      "re_index" (int32, -1 = the plain ground truth) is added.  None runs what ran before the keyword existed.
    -> dict: "all" / "full" / "visib" -> {"errors": {kind: (B,) f64}, "R", "t", "status", "re", "te"}; "report": code_report's dict;
       "labels": encode_targets' dict; "final_Bboxes": (B,4) int array; "outputs": the network's tuple; "mask_crops": the GT
       (visible, full) uint8 crops (B,S,S)."""
    from . import metric
    from . import postprocess as post
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    H, W = int(frames.shape[1]), int(frames.shape[2])
    padded = [None if b is None else PP.padding_Bbox(b, padding_ratio) for b in Bboxes]
    crops = PP.get_roi_batch(frames, padded, crop_size, PP.INTER_LINEAR, resize_method, img_index=img_index)
    m_vis = PP.get_roi_batch(_mask_images(masks_visib), padded, crop_size_gt, PP.INTER_NEAREST, resize_method, img_index=img_index)[..., 0]
    m_full = PP.get_roi_batch(_mask_images(masks_full), padded, crop_size_gt, PP.INTER_NEAREST, resize_method, img_index=img_index)[..., 0]
    final = [None if b is None else PP.get_final_Bbox(b, resize_method, W, H) for b in padded]
    boxes, _ = _host_boxes(final)
    with torch.no_grad():
        out = net(crops, None) if obj_ids is None else net(crops, None, obj_ids)
    p2d, valid, _ = post.correspondences(out, discard_bd_pixel=discard_bd_pixel, Bboxes=boxes)
    if obj_ids is not None and torch.as_tensor(p3d_xyz).dim() == 3:
        ids = torch.as_tensor(obj_ids).long().reshape(-1).to(torch.as_tensor(p3d_xyz).device)
        p3_pose = torch.as_tensor(p3d_xyz)[ids - 1]                   # the object table -> one keypoint set per crop for the solver
    else:
        p3_pose = p3d_xyz
    res = {}
    for col, name in enumerate(COLUMNS):
        R, t, _, status = post.solve_pnp_ransac(p3_pose, p2d, valid, cam_K, column=col, reproj_threshold=reproj_threshold,
                                                iterations=iterations, seed=seed)
        if re_symmetries is None:
            re, te = pose_re_te(R_gt, t_gt, R, t)      # test.py:388-389 passes the ground truth first: trace(R_gt . inv(R_pred))
        else:
            re, te, re_index = pose_re_te_sym(R, t, R_gt, t_gt, symmetries=re_symmetries, mesh_ids=mesh_ids, return_index=True)
        res[name] = {"errors": metric.score_poses(R, t, R_gt, t_gt, cam_K, vertices, mesh_ids=mesh_ids, kinds=kinds, symmetries=symmetries,
                                                depth_test=depth_test, image_ids=image_ids, size=size),
                     "R": R, "t": t,
                     "status": status, "re": re, "te": te}
        if re_symmetries is not None:
            res[name]["re_index"] = re_index
    Rg = R_gt if torch.is_tensor(R_gt) else torch.from_numpy(np.ascontiguousarray(np.asarray(R_gt, dtype=np.float64))).to(frames.device)
    labels = encode_targets(p3d_xyz, cam_K, Rg, t_gt, final, crop_size_gt, obj_ids=obj_ids)
    res["report"] = code_report(out, labels, m_vis, m_full)
    res["labels"], res["final_Bboxes"], res["outputs"], res["mask_crops"] = labels, boxes, out, (m_vis, m_full)
    return res


def summarize_report(batches, diameters, symmetric=False):
    """The key / value lines of test.py's score file (:474-525) from accumulated `evaluate_batch` results.
      batches: a list of evaluate_batch dicts (or one); diameters: the object's diameter, or one per crop over all batches;
      symmetric: ADI is the main metric (and ADD the supplementary one) of a symmetric object, the other way round otherwise
      (test.py:127-136).  A NaN error counts as 10000 (:379-380); pass rates use the strict `<`.
    -> (dict key -> value, the text of the lines)"""
    from .metric import compute_auc_posecnn
    if isinstance(batches, dict):
        batches = [batches]
    host = lambda x: x.detach().cpu().numpy().astype(np.float64)      # noqa: E731
    main, supp = ("adi", "add") if symmetric else ("add", "adi")
    n = sum(int(b["report"]["roi_bit_acc"].shape[0]) for b in batches)
    diam = np.broadcast_to(np.asarray(diameters, dtype=np.float64).reshape(-1), (n,))
    rows, tail = [], []
    for name in COLUMNS:
        pfx = "" if name == "all" else name + "_"
        err = np.concatenate([host(b[name]["errors"][main]) for b in batches])
        err = np.where(np.isnan(err), 10000.0, err)
        passed = [float(np.mean(err < f * diam)) for f in (0.02, 0.05, 0.1)]
        if name == "all":
            rows.append(("acc", passed[2]))
        rows += [(pfx + "adx2", passed[0]), (pfx + "adx5", passed[1]), (pfx + "adx10", passed[2]), (pfx + "adx_err", float(np.mean(err))),
                 (pfx + "re", float(np.mean(np.concatenate([host(b[name]["re"]) for b in batches])))),
                 (pfx + "te", float(np.mean(np.concatenate([host(b[name]["te"]) for b in batches]))))]
        tail.append((pfx + "AUC_posecnn_" + main.upper(), float(compute_auc_posecnn(err / 1000.0))))
    for name in COLUMNS:
        if all(supp in b[name]["errors"] for b in batches):
            pfx = "" if name == "all" else name + "_"
            err = np.concatenate([host(b[name]["errors"][supp]) for b in batches])
            tail.append((pfx + "AUC_posecnn_" + supp.upper(), float(compute_auc_posecnn(np.where(np.isnan(err), 10000.0, err) / 1000.0))))
    rep = lambda k: np.concatenate([host(b["report"][k]) for b in batches], 0)      # noqa: E731
    rows += [(k, float(np.mean(rep(k)))) for k in ("roi_bit_acc", "reproj_x_acc", "reproj_y_acc")]
    rows.append(("bit_err_arr", np.mean(rep("bit_err_arr"), axis=0)))
    rows += [(k, float(np.mean(rep(k)))) for k in ("visib_pixel_acc", "visib_iou", "full_pixel_acc", "full_iou")]
    rows += tail
    text = "".join("%s %s\n" % (k, np.array2string(v, max_line_width=10 ** 6) if isinstance(v, np.ndarray) else "%.4f" % v) for k, v in rows)
    return dict(rows), text


def lm_report_text(counts, figures, adx_type="all"):
    """The LM report from its integer counts, on the host: test_lm.py:372-419 restated.
      counts: (n_obj, 10) integers, columns RETE_COUNTS, one row per evaluated object (the 13 of LINEMOD);  figures: dict with the
      means over all crops of roi_bit_acc, reproj_x_acc, reproj_y_acc, visib_pixel_acc, visib_iou, full_pixel_acc, full_iou (floats)
      and bit_err_arr (1-d array).
    Per object the pass rate is count / n (what np.mean of the 0 / 1 flags gives; an object without a sample gives NaN, as np.mean of
    an empty list does); each reported rate is np.mean over the objects.
    -> (dict key -> value, the text of the score file's lines in its order and format)"""
    c = np.asarray(counts, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rates = c[:, 1:] / c[:, :1]
    mean = {k: float(np.mean(rates[:, i])) for i, k in enumerate(RETE_COUNTS[1:])}
    rows = [("adx_type", adx_type), ("acc", mean["adx10"])] + [(k, mean[k]) for k in RETE_COUNTS[1:]]
    rows += [(k, float(figures[k])) for k in ("roi_bit_acc", "reproj_x_acc", "reproj_y_acc")]
    rows.append(("bit_err_arr", np.asarray(figures["bit_err_arr"])))
    rows += [(k, float(figures[k])) for k in ("visib_pixel_acc", "visib_iou", "full_pixel_acc", "full_iou")]
    text = "".join("%s %s\n" % (k, v if isinstance(v, (str, np.ndarray)) else "%.4f" % v) for k, v in rows)
    out = dict(rows)
    out["per_object"] = {k: rates[:, i] for i, k in enumerate(RETE_COUNTS[1:])}
    out["counts"] = np.asarray(counts)
    return out, text


def summarize_report_lm(batches, obj_ids, diameters, symmetric_obj_ids=LM_SYMMETRIC_OBJ_IDS, lm_obj_ids=LM13_OBJ_IDS, adx_type="all"):
    """test_lm.py's score file (:299-327 per crop, :372-419 the summary) from accumulated `evaluate_batch` results over several objects.
      batches: a list of evaluate_batch dicts (or one), scored with kinds "add" and / or "adi" as their objects need and -- for the
      reference's numbers -- with re_symmetries;  obj_ids: each crop's object id over all batches, in order;  diameters: {obj_id:
      diameter} or one diameter per crop;  symmetric_obj_ids: the objects whose main error is ADI (ADD for the others) -- test_lm.py's
      `symmetry_ids`;  lm_obj_ids: the objects the means run over, in the report's order;  adx_type: the correspondence column
      scored, "all" / "full" / "visib" (targets.COLUMNS).
    The nine pass flags are counted per object on the device (cp_rete_pass_counts: NaN counts as 10000, strict `<`); 13 x 10
    integers come to the host, where lm_report_text forms the rates and their means; the code / mask figures are the means over all
    crops, as summarize_report forms them.
    -> (dict key -> value, the text of the lines test_lm.py:411-419 writes)"""
    if isinstance(batches, dict):
        batches = [batches]
    if adx_type not in COLUMNS:
        raise ValueError("adx_type must be among %s, got %r" % (COLUMNS, adx_type))
    ids = (obj_ids.detach().cpu().numpy() if torch.is_tensor(obj_ids) else np.asarray(obj_ids)).astype(np.int64).reshape(-1)
    n = sum(int(b[adx_type]["re"].shape[0]) for b in batches)
    if ids.shape[0] != n:
        raise ValueError("obj_ids: one object id per crop (%d), got %d" % (n, ids.shape[0]))
    order = [int(o) for o in lm_obj_ids]
    if len(set(order)) != len(order) or not order:
        raise ValueError("lm_obj_ids must name each evaluated object once")
    slot_of = {o: k for k, o in enumerate(order)}
    stray = sorted(set(ids.tolist()) - set(order))
    if stray:
        raise ValueError("obj_ids %r are not among lm_obj_ids" % (stray,))
    slots = np.array([slot_of[int(o)] for o in ids], dtype=np.int32)
    if isinstance(diameters, dict):
        diam = np.array([float(diameters[int(o)]) for o in ids], dtype=np.float64)
    else:
        diam = np.asarray(diameters, dtype=np.float64).reshape(-1)
        if diam.shape[0] != n:
            raise ValueError("diameters: a dict obj_id -> diameter or one per crop (%d), got %d" % (n, diam.shape[0]))
    sym = np.isin(ids, np.asarray(list(symmetric_obj_ids), dtype=np.int64))
    dev = batches[0][adx_type]["re"].device
    cat = lambda f: torch.cat([f(b).detach().to(device=dev, dtype=torch.float64).reshape(-1) for b in batches])      # noqa: E731
    for need, kind in ((sym.any(), "adi"), ((~sym).any(), "add")):
        if need and not all(kind in b[adx_type]["errors"] for b in batches):
            raise ValueError("batches: the %s objects need kind %r in evaluate_batch's kinds" % ("symmetric" if kind == "adi" else "asymmetric", kind))
    if sym.all():
        adx = cat(lambda b: b[adx_type]["errors"]["adi"])
    elif not sym.any():
        adx = cat(lambda b: b[adx_type]["errors"]["add"])
    else:
        adx = torch.where(torch.from_numpy(sym).to(dev), cat(lambda b: b[adx_type]["errors"]["adi"]), cat(lambda b: b[adx_type]["errors"]["add"]))
    counts = rete_pass_counts(cat(lambda b: b[adx_type]["re"]), cat(lambda b: b[adx_type]["te"]), adx, torch.from_numpy(diam).to(dev), slots,
                              len(order)).cpu().numpy()
    rep = lambda k: torch.cat([b["report"][k].detach().to(torch.float64) for b in batches], 0).cpu().numpy()      # noqa: E731
    figures = {k: float(np.mean(rep(k))) for k in FIGURES}
    figures["bit_err_arr"] = np.mean(rep("bit_err_arr"), axis=0)
    return lm_report_text(counts, figures, adx_type)
