"""Input side on the device: the RoI crops of the reference's data loader as ONE HIP launch per batch.

The reference's `bop_dataset_pytorch.py` crops every detection on the host: `padding_Bbox` (:147-163) -> `get_roi(x, Bbox,
crop_size, interpolation, resize_method)` (:132-145: `crop_square_resize` :55-91 in every config, or `crop_resize` :94-108, then
`cv2.resize`) -> `get_final_Bbox` (:188-222) -> `transform_pre` (:385-398).  Here the full uint8 images go to the GPU once and
`get_roi_batch` cuts all crops of a batch there (`cp_crop_resize_u8`, csrc/preprocess.hip); the uint8 crops feed the model's uint8
forward (`net(crops_u8, ...)`: ToTensor + Normalize on the device, `cp_u8hwc_to_nhwc_norm`).  The window arithmetic (a handful of
integer operations per box, on the host) is the reference's; the resize is cv2's 8-bit arithmetic (see the kernel's header).

Row N21: the loader's third resize_method, "crop_resize_by_warp_affine" (:39-52, :111-129, :136-139): `get_scale_and_Bbox_center` ->
`get_affine_transform` (GDR_Net_Augmentation.py:199-240; three float32 point pairs, then the 2 x 3 matrix that maps one triple onto the
other, solved here in closed form in float64 where the reference calls cv2.getAffineTransform) -> `cv2.warpAffine`, which is
`warp_affine` here: the matrix is inverted on the host (six doubles per crop) and `cp_warp_affine_u8` (csrc/warp_affine.hip, where the
fixed-point rule is stated) warps the whole batch in one launch.  Parity with cv2's own bytes is UNPINNED, as for cv2.resize.
No CPU fallback: CPU tensors raise."""
import numpy as np
import torch

from . import _abi

INTER_NEAREST, INTER_LINEAR = 0, 1          # cv2.INTER_NEAREST / cv2.INTER_LINEAR


def padding_Bbox(Bbox, padding_ratio):
    """the detection box (x, y, w, h) grown about its centre (bop_dataset_pytorch.py:147-163) -> int array (x, y, w, h)"""
    x, y, w, h = (float(v) for v in Bbox)
    pw, ph = int(w * padding_ratio), int(h * padding_ratio)
    return np.array([int(x + 0.5 * w - pw / 2), int(y + 0.5 * h - ph / 2), pw, ph])


def roi_window(Bbox, resize_method, img_w, img_h, crop_size=None):
    """(x1, y1, x2, y2, roi_w, roi_h) of cp_crop_resize_u8 for one box: the square about the box centre, cut with int() as the
    reference does (crop_square_resize :55-77), or the box clamped to the image (crop_resize :94-106).
    "crop_resize_by_warp_affine" has no such window.  With crop_size the result is the frame rectangle [x1, x2) x [y1, y2) its crop can
    read, clamped to the frame (roi_w = x2 - x1, roi_h = y2 - y1; all zero for a box that gives a zero crop) -- the bounding box of the
    four output corners' source points at that crop_size, floor / ceil + 1.  The warp rounds coordinates to 1/32 pixel (to whole pixels
    under INTER_NEAREST), so a tap beyond that rectangle has weight 0.  The rectangle depends on the crop size, so WITHOUT crop_size the
    method stays what it was for this function before row N21: NotImplementedError."""
    if resize_method == "crop_resize_by_warp_affine":
        if crop_size is None:
            raise NotImplementedError("crop_resize_by_warp_affine has no window: roi_window(..., crop_size) gives the frame rectangle its crop reads")
        return _warp_rect(Bbox, img_w, img_h, crop_size)
    x1, y1, bw, bh = (v for v in Bbox)
    x2, y2 = x1 + bw, y1 + bh
    if resize_method == "crop_square_resize":
        if bh > bw:
            c = 0.5 * (x1 + x2)
            x1, x2 = c - bh / 2, c + bh / 2
        else:
            c = 0.5 * (y1 + y2)
            y1, y2 = c - bw / 2, c + bw / 2
        side = int(max(bh, bw))
        return int(x1), int(y1), int(x2), int(y2), side, side
    if resize_method == "crop_resize":
        x1, y1, x2, y2 = _clamped_box(x1, y1, x2, y2, img_w, img_h)
        # the reference cuts `img[y1:y2, x1:x2]` (:106): a NEGATIVE end (box wholly left of / above the frame) is Python's
        # "counted from the far edge", so such a box yields the frame minus a margin, not an empty crop (n3_windows.npz pins it)
        x2 = x2 if x2 >= 0 else max(img_w + x2, 0)
        y2 = y2 if y2 >= 0 else max(img_h + y2, 0)
        return x1, y1, x2, y2, max(x2 - x1, 0), max(y2 - y1, 0)
    raise NotImplementedError("unknown decoder type: %s" % resize_method)      # the reference's message (:145)


def _clamped_box(x1, y1, x2, y2, img_w, img_h):
    """crop_resize :94-104 / get_final_Bbox :212-220"""
    return int(max(x1, 0)), int(max(y1, 0)), int(min(x2, img_w)), int(min(y2, img_h))


def get_final_Bbox(Bbox, resize_method, max_x, max_y):
    """the box the crop actually covers (bop_dataset_pytorch.py:188-222), what the post-processing maps pixel codes back with
    (crop_resize: the clamped corners as they are, also where x2 < x1 -- the reference's own result for a box off the frame).
    crop_resize_by_warp_affine is the square case (:195), and with it the reference's mismatch: this box is cut with int() and WITHOUT
    the scale clamp min(.., max(H, W)), while the crop's pixels come from the float centre and the clamped scale (get_scale_and_Bbox_center)
    -- for an odd side the two differ by half a pixel, for a box larger than the frame by the clamp.  Kept as the reference has it."""
    if resize_method == "crop_resize_by_warp_affine":
        resize_method = "crop_square_resize"
    if resize_method == "crop_resize":
        x1, y1, x2, y2 = _clamped_box(Bbox[0], Bbox[1], Bbox[0] + Bbox[2], Bbox[1] + Bbox[3], max_x, max_y)
    else:
        x1, y1, x2, y2, _, _ = roi_window(Bbox, resize_method, max_x, max_y)
    return np.array([x1, y1, x2 - x1, y2 - y1])


def _windows(Bboxes, resize_method, W, H):
    """roi_window of every box -> (B,6) int32; a None entry keeps the all-zero window (an empty roi: a zero crop)"""
    win = np.zeros((len(Bboxes), 6), dtype=np.int32)
    for b, box in enumerate(Bboxes):
        if box is not None:
            win[b] = roi_window([int(v) for v in box], resize_method, W, H)
    return win


def _img_index_on(img_index, B, n_img, dev):
    """the image of each box as an int32 tensor on dev, or None where the kernels' default holds (image b, or the only image)"""
    if img_index is None:
        if n_img not in (1, B):
            raise RuntimeError("checkerpose_amd.preprocess: img_index is needed when %d boxes come from %d images" % (B, n_img))
        return None
    idx_np = np.asarray(img_index, dtype=np.int32).reshape(-1)
    if idx_np.shape[0] != B or (B and (idx_np.min() < 0 or idx_np.max() >= n_img)):
        raise RuntimeError("checkerpose_amd.preprocess: img_index must hold one valid image number per box")
    return torch.from_numpy(idx_np).to(dev)


def _images_on_device(images):
    """uint8 CUDA images as (n_img, H, W, C <= 4), contiguous; anything else raises"""
    if not (torch.is_tensor(images) and images.is_cuda and images.dtype == torch.uint8):
        raise RuntimeError("checkerpose_amd.preprocess: images must be a uint8 CUDA tensor (no CPU path)")
    if images.dim() == 3:
        images = images.unsqueeze(0)
    if images.dim() != 4 or images.shape[3] > 4 or not images.is_contiguous():
        raise RuntimeError("checkerpose_amd.preprocess: images (n_img, H, W, C <= 4), contiguous")
    return images


# ---- row N21: crop_resize_by_warp_affine ------------------------------------------------------------------------------------------
def get_dir(src_point, rot_rad):
    """src_point turned by rot_rad (GDR_Net_Augmentation.py:191-197)"""
    sn, cs = np.sin(rot_rad), np.cos(rot_rad)
    return [src_point[0] * cs - src_point[1] * sn, src_point[0] * sn + src_point[1] * cs]


def get_3rd_point(a, b):
    """b plus (a - b) turned by 90 degrees (GDR_Net_Augmentation.py:186-188)"""
    direct = a - b
    return b + np.array([-direct[1], direct[0]], dtype=np.float32)


def affine_points(center, scale, rot, output_size, shift=(0, 0)):
    """The two float32 point triples (src, dst), each (3, 2), that get_affine_transform hands to cv2.getAffineTransform
    (GDR_Net_Augmentation.py:207-233), operation for operation and dtype for dtype: a centre given as a tuple / list becomes float32, a
    scalar scale a float32 pair, a pair stays what it is (a tuple of Python floats multiplies in float64), and every sum is rounded to
    float32 only when it is stored into the triples."""
    if isinstance(center, (tuple, list)):
        center = np.array(center, dtype=np.float32)
    if isinstance(scale, (int, float)):
        scale = np.array([scale, scale], dtype=np.float32)
    if isinstance(output_size, (int, float)):
        output_size = (output_size, output_size)
    src_w, dst_w, dst_h = scale[0], output_size[0], output_size[1]
    rot_rad = np.pi * rot / 180
    src_dir = get_dir([0, src_w * -0.5], rot_rad)
    dst_dir = np.array([0, dst_w * -0.5], np.float32)
    shifted = np.multiply(scale, shift)
    src = np.zeros((3, 2), dtype=np.float32)
    dst = np.zeros((3, 2), dtype=np.float32)
    src[0, :] = center + shifted
    src[1, :] = center + src_dir + shifted
    dst[0, :] = [dst_w * 0.5, dst_h * 0.5]
    dst[1, :] = np.array([dst_w * 0.5, dst_h * 0.5], np.float32) + dst_dir
    src[2:, :] = get_3rd_point(src[0, :], src[1, :])
    dst[2:, :] = get_3rd_point(dst[0, :], dst[1, :])
    return src, dst


def affine_from_points(src, dst):
    """The (2, 3) float64 matrix that maps the three points src (3, 2) onto dst (3, 2) -- what cv2.getAffineTransform solves for, here in
    closed form (Cramer's rule on the two edge vectors); collinear src points give a matrix of NaN (warp_affine's "no box")."""
    p, q = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    (d1x, d1y), (d2x, d2y) = p[1] - p[0], p[2] - p[0]
    (e1x, e1y), (e2x, e2y) = q[1] - q[0], q[2] - q[0]
    det = d1x * d2y - d1y * d2x
    if det == 0 or not np.isfinite(det):
        return np.full((2, 3), np.nan)
    m00, m01 = (e1x * d2y - e2x * d1y) / det, (e2x * d1x - e1x * d2x) / det
    m10, m11 = (e1y * d2y - e2y * d1y) / det, (e2y * d1x - e1y * d2x) / det
    return np.array([[m00, m01, q[0, 0] - m00 * p[0, 0] - m01 * p[0, 1]], [m10, m11, q[0, 1] - m10 * p[0, 0] - m11 * p[0, 1]]])


def get_affine_transform(center, scale, rot, output_size, shift=(0, 0), inv=False):
    """`get_affine_transform` (GDR_Net_Augmentation.py:199-240): centre (cx, cy), scale a scalar or (w, h) (only w is used, as there),
    rot in degrees, output_size an int or (w, h) -> the (2, 3) float64 matrix dst = M . src (inv: src = M . dst)."""
    src, dst = affine_points(center, scale, rot, output_size, shift)
    return affine_from_points(dst, src) if inv else affine_from_points(src, dst)


def get_scale_and_Bbox_center(Bbox, image):
    """`get_scale_and_Bbox_center` (bop_dataset_pytorch.py:111-129): the float centre of the box (x, y, w, h) and
    scale = min(max(bh, bw), max(H, W)) as a float.  image: anything with a .shape that starts (H, W), or the pair (H, W).
    -> (scale, centre (2,) float64)"""
    x1, y1, bw, bh = Bbox[0], Bbox[1], Bbox[2], Bbox[3]
    x2, y2 = x1 + bw, y1 + bh
    H, W = (image.shape if hasattr(image, "shape") else image)[:2]
    return min(max(bh, bw), max(int(H), int(W))) * 1.0, np.array([0.5 * (x1 + x2), 0.5 * (y1 + y2)])


def _roi_affine(Bbox, img_w, img_h, crop_size):
    """get_roi's matrix for one box (bop_dataset_pytorch.py:136-139 -> :39-52), or None where the crop is zero: no box, or a box with
    w <= 0 or h <= 0 (the reference would hand cv2 a singular system)"""
    if Bbox is None or Bbox[2] <= 0 or Bbox[3] <= 0:
        return None
    scale, center = get_scale_and_Bbox_center(Bbox, (img_h, img_w))
    return get_affine_transform(center, (scale, scale), 0, (crop_size, crop_size))


WARP_RANGE = float(1 << 20)        # the int32 fixed point (10 fraction bits) of the warp holds source coordinates up to 2^21


def _inverse_maps(M, inverse_map, out_w, out_h):
    """The (B, 6) float64 inverse maps a00 a01 b0 a10 a11 b1 of cp_warp_affine_u8 from B forward matrices (2, 3) (None entries, and
    matrices that hold a NaN, become rows of NaN: zero crops), inverted as cv2.invertAffineTransform does (csrc/warp_affine.hip);
    ValueError where a map sends an output corner further than 2^20 pixels from the origin."""
    B = len(M)
    mats = np.full((B, 2, 3), np.nan)
    for b in range(B):
        if M[b] is not None:
            mats[b] = np.asarray(M[b].detach().cpu() if torch.is_tensor(M[b]) else M[b], dtype=np.float64).reshape(2, 3)
    mats[np.isnan(mats).any(axis=(1, 2))] = np.nan
    if inverse_map:
        inv = mats.reshape(B, 6).copy()
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            D = mats[:, 0, 0] * mats[:, 1, 1] - mats[:, 0, 1] * mats[:, 1, 0]
            D = np.where(D != 0, 1.0 / D, 0.0)
            a00, a01, a10, a11 = mats[:, 1, 1] * D, mats[:, 0, 1] * -D, mats[:, 1, 0] * -D, mats[:, 0, 0] * D
            b0 = -a00 * mats[:, 0, 2] - a01 * mats[:, 1, 2]
            b1 = -a10 * mats[:, 0, 2] - a11 * mats[:, 1, 2]
        inv = np.stack([a00, a01, b0, a10, a11, b1], 1)
        inv[np.isnan(mats[:, 0, 0])] = np.nan
    with np.errstate(invalid="ignore"):
        far = np.abs(_corner_sources(inv, out_w, out_h)).max(axis=(1, 2))
    if (far[~np.isnan(inv[:, 0])] > WARP_RANGE).any() or np.isnan(far[~np.isnan(inv[:, 0])]).any():
        raise ValueError("warp_affine: a matrix sends an output corner further than 2^20 pixels from the origin (the int32 fixed point "
                         "of the warp would wrap, as it does in OpenCV)")
    return np.ascontiguousarray(inv)


def _corner_sources(inv, out_w, out_h):
    """the source points (B, 4, 2) of the output corners (0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1) under the inverse maps (B, 6)"""
    cx = np.array([0.0, out_w - 1.0, 0.0, out_w - 1.0])
    cy = np.array([0.0, 0.0, out_h - 1.0, out_h - 1.0])
    sx = inv[:, 0:1] * cx + inv[:, 1:2] * cy + inv[:, 2:3]
    sy = inv[:, 3:4] * cx + inv[:, 4:5] * cy + inv[:, 5:6]
    return np.stack([sx, sy], 2)


def _warp_rect(Bbox, img_w, img_h, crop_size):
    """roi_window's rectangle of "crop_resize_by_warp_affine" """
    if Bbox is None or Bbox[2] <= 0 or Bbox[3] <= 0:
        return 0, 0, 0, 0, 0, 0
    inv = _inverse_maps([_roi_affine(Bbox, img_w, img_h, crop_size)], False, crop_size, crop_size)
    pts = _corner_sources(inv, crop_size, crop_size)[0]
    lo, hi = pts.min(0), pts.max(0)
    x1, y1 = min(max(int(np.floor(lo[0])), 0), img_w), min(max(int(np.floor(lo[1])), 0), img_h)
    x2, y2 = min(max(int(np.ceil(hi[0])) + 1, 0), img_w), min(max(int(np.ceil(hi[1])) + 1, 0), img_h)
    return x1, y1, x2, y2, max(x2 - x1, 0), max(y2 - y1, 0)


def warp_affine(images, M, out_size, interpolation=INTER_LINEAR, inverse_map=False, img_index=None, out=None):
    """`cv2.warpAffine(img, M, (w, h), flags=interpolation)` with BORDER_CONSTANT 0 for a batch, on the GPU (cp_warp_affine_u8; the
    fixed-point rule is in csrc/warp_affine.hip).
    images: uint8 CUDA tensor (n_img, H, W, C) or (H, W, C), C <= 4; M: (B, 2, 3) forward matrices dst = M . src (array, tensor, or a
    list whose None entries -- like matrices that hold a NaN -- give zero crops); inverse_map: M already maps dst to src
    (cv2.WARP_INVERSE_MAP); out_size: an int or (w, h); img_index: the image of each matrix (default: image b, or the only image).
    -> uint8 CUDA tensor (B, h, w, C).  A matrix that sends an output corner further than 2^20 pixels from the origin is refused with
    ValueError."""
    images = _images_on_device(images)
    if interpolation not in (INTER_NEAREST, INTER_LINEAR):
        raise NotImplementedError("interpolation %r: cv2.INTER_NEAREST (0) and cv2.INTER_LINEAR (1) are built" % (interpolation,))
    out_w, out_h = (int(out_size), int(out_size)) if np.ndim(out_size) == 0 else (int(out_size[0]), int(out_size[1]))
    if out_w <= 0 or out_h <= 0:
        raise ValueError("warp_affine: out_size must be positive")
    n_img, H, W, C_ = (int(v) for v in images.shape)
    B = len(M)
    inv, idx_t = _inverse_maps(M, inverse_map, out_w, out_h), _img_index_on(img_index, B, n_img, images.device)
    if out is None:
        out = torch.empty(B, out_h, out_w, C_, dtype=torch.uint8, device=images.device)
    elif tuple(out.shape) != (B, out_h, out_w, C_) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != images.device:
        raise RuntimeError("checkerpose_amd.preprocess: out must be a contiguous uint8 (B, h, w, C) tensor on the images' device")
    if B:
        inv_t = torch.from_numpy(inv).to(images.device)
        _abi.call("cp_warp_affine_u8", images.device, images, n_img, H, W, C_, inv_t, idx_t, out, B, out_h, out_w, int(interpolation))
    return out


def crop_resize_by_warp_affine(images, centers, scales, output_size, rot=0, interpolation=INTER_LINEAR, img_index=None):
    """`crop_resize_by_warp_affine` (bop_dataset_pytorch.py:39-52) for a batch: crop b is the scale x scale square about centers[b],
    turned by rot degrees, warped to output_size (an int or (w, h)).
    centers (B, 2) (a None entry: a zero crop); scales (B,) or (B, 2) (w, h; only w is used, as in the reference); rot a scalar or (B,).
    -> uint8 CUDA tensor (B, h, w, C).  (The reference returns (h, w) for a one-channel image; here the channel axis stays.)"""
    B = len(centers)
    size = (output_size, output_size) if np.ndim(output_size) == 0 else (output_size[0], output_size[1])
    rots = np.broadcast_to(np.asarray(rot, dtype=np.float64), (B,))
    mats = []
    for b in range(B):
        if centers[b] is None:
            mats.append(None)
            continue
        sc = (float(scales[b]), float(scales[b])) if np.ndim(scales[b]) == 0 else (float(scales[b][0]), float(scales[b][1]))
        mats.append(get_affine_transform(np.asarray(centers[b], dtype=np.float64), sc, float(rots[b]), size))
    return warp_affine(images, mats, size, interpolation, img_index=img_index)


def get_roi_batch(images, Bboxes, crop_size, interpolation=INTER_LINEAR, resize_method="crop_square_resize", img_index=None, out=None):
    """`get_roi` (bop_dataset_pytorch.py:132-145) for a batch, on the GPU.
    images: uint8 CUDA tensor (n_img, H, W, C) or (H, W, C) (C <= 4, the loader's cv2.imread layout); Bboxes: (B, 4) boxes
    (x, y, w, h), ALREADY padded / augmented as the loader does before get_roi; None entries give a zero crop (the loader's dummy
    input for a missing detection, :325-337); img_index: for each box the image it is cut from (default: image b, or the only
    image).  resize_method: "crop_square_resize", "crop_resize" (cp_crop_resize_u8) or "crop_resize_by_warp_affine" (the affine map of
    _roi_affine through warp_affine; a box with w <= 0 or h <= 0 gives a zero crop there -- the reference would hand cv2 a singular
    system).  -> uint8 CUDA tensor (B, crop_size, crop_size, C)."""
    images = _images_on_device(images)
    if interpolation not in (INTER_NEAREST, INTER_LINEAR):
        raise NotImplementedError("interpolation %r: cv2.INTER_NEAREST (0) and cv2.INTER_LINEAR (1) are built" % (interpolation,))
    n_img, H, W, C_ = (int(v) for v in images.shape)
    B = len(Bboxes)
    if resize_method == "crop_resize_by_warp_affine":
        return warp_affine(images, [_roi_affine(box, W, H, crop_size) for box in Bboxes], crop_size, interpolation, img_index=img_index, out=out)
    win, idx_t = _windows(Bboxes, resize_method, W, H), _img_index_on(img_index, B, n_img, images.device)
    if out is None:
        out = torch.empty(B, crop_size, crop_size, C_, dtype=torch.uint8, device=images.device)
    elif tuple(out.shape) != (B, crop_size, crop_size, C_) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != images.device:
        raise RuntimeError("checkerpose_amd.preprocess: out must be a contiguous uint8 (B, crop, crop, C) tensor on the images' device")
    if B == 0:
        return out
    win_t = torch.from_numpy(win).to(images.device)
    lib = _abi.load()
    st = torch.cuda.current_stream(images.device).cuda_stream
    _abi.check(lib.cp_crop_resize_u8(st, images.data_ptr(), n_img, H, W, C_, win_t.data_ptr(), idx_t.data_ptr() if idx_t is not None else None,
                                     out.data_ptr(), B, int(crop_size), int(interpolation)), "cp_crop_resize_u8")
    return out                                # (win_t / idx_t may be freed: torch's allocator reuses a block in stream order)


def get_roi_mask_bits(bits, bit, Bboxes, crop_size, resize_method="crop_square_resize", img_index=None):
    """`get_roi_batch(..., INTER_NEAREST)` of the 0 / 255 mask images that ONE BIT of a bit plane stands for, without expanding them
    (cp_crop_mask_bits, or cp_warp_mask_bits for "crop_resize_by_warp_affine": the same window, zero-padding and index arithmetic, so
    the same bytes).
    bits: int32 CUDA tensor (n_img, H, W) or (H, W) -- render.render_scene's "full_bits" / "visib_bits"; bit: (B,) for each box the
    bit of its mask (render_scene's "slot"; a value outside 0..31 gives a zero crop); Bboxes, resize_method, img_index: get_roi_batch's.
    -> uint8 CUDA tensor (B, crop_size, crop_size, 1), the shape get_roi_batch gives for a mask."""
    if not (torch.is_tensor(bits) and bits.is_cuda and bits.dtype == torch.int32):
        raise RuntimeError("checkerpose_amd.preprocess: bits must be an int32 CUDA tensor (no CPU path)")
    if bits.dim() == 2:
        bits = bits.unsqueeze(0)
    if bits.dim() != 3 or not bits.is_contiguous():
        raise RuntimeError("checkerpose_amd.preprocess: bits (n_img, H, W), contiguous")
    n_img, H, W = (int(v) for v in bits.shape)
    B = len(Bboxes)
    bit_np = np.asarray(bit.detach().cpu() if torch.is_tensor(bit) else bit).reshape(-1).astype(np.int32)
    if bit_np.shape[0] != B:
        raise ValueError("bit must hold one bit number per box")
    out = torch.empty(B, int(crop_size), int(crop_size), 1, dtype=torch.uint8, device=bits.device)
    if resize_method == "crop_resize_by_warp_affine":          # cp_warp_mask_bits: warp_affine(INTER_NEAREST)'s coordinates, so the same bytes
        inv = _inverse_maps([_roi_affine(box, W, H, crop_size) for box in Bboxes], False, int(crop_size), int(crop_size))
        idx_t = _img_index_on(img_index, B, n_img, bits.device)
        if B:
            inv_t, bit_t = torch.from_numpy(inv).to(bits.device), torch.from_numpy(bit_np).to(bits.device)
            _abi.call("cp_warp_mask_bits", bits.device, bits, n_img, H, W, inv_t, idx_t, bit_t, out, B, int(crop_size), int(crop_size))
        return out
    win, idx_t = _windows(Bboxes, resize_method, W, H), _img_index_on(img_index, B, n_img, bits.device)
    if B == 0:
        return out
    win_t, bit_t = torch.from_numpy(win).to(bits.device), torch.from_numpy(bit_np).to(bits.device)
    _abi.call("cp_crop_mask_bits", bits.device, bits, n_img, H, W, win_t, idx_t, bit_t, out, B, int(crop_size))
    return out
