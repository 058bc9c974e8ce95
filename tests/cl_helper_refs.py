"""The channels-last helper kernels (csrc/elementwise.hip, csrc/pack_layout.hip, the resampling / pooling backward of
csrc/train_dense.hip) restated from their definitions in float64 torch / numpy: no GPU, no kernel arithmetic.  tests/test_cl_helpers.py
checks each restatement against torch where torch has the operation; tests/test_gpu_cl_helpers.py holds the device to them.

All tensors are NCHW on the CPU unless a name says otherwise."""
import numpy as np
import torch

from tests.common import det_tensor


# ---- bilinear x2, align_corners=True:  src = o (n - 1) / (2n - 1);  i0 = floor(src);  i1 = i0 + (i0 < n - 1);  l1 = src - i0
def up_taps(n, f32_coord=False):
    """(i0, i1, l1) of the 2n outputs of an axis of n inputs; exact integer arithmetic for floor(), n == 1 has scale 0.
    f32_coord: the source coordinate as ATen forms it for a float32 tensor (UpSample.h: area_pixel_compute_scale<float>, then
    src = scale * dst in float32): the float32 quotient times the float32 output index, rounded to float32.  Its error grows with n
    (2e-6 of a pixel at n = 64, 1e-3 at n = 16400), so at large n every float32 implementation of that definition, torch's
    included, leaves the exact map by that much times the difference of the two taps; the interpolation itself stays float64."""
    o = np.arange(2 * n, dtype=np.int64)
    if f32_coord:
        scale = np.float32(n - 1) / np.float32(2 * n - 1) if n > 1 else np.float32(0)
        src = (scale * o.astype(np.float32)).astype(np.float32)
        i0 = src.astype(np.int64)
        l1 = (src - i0.astype(np.float32)).astype(np.float64)         # exact: both are float32 and within one of each other
    else:
        den = max(2 * n - 1, 1)
        num = o * (n - 1)                               # src = num / den
        i0 = num // den
        l1 = (num - i0 * den).astype(np.float64) / den
    i1 = i0 + (i0 < n - 1)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l1)


def up_matrix(n):
    """the (2n, n) float64 weight matrix of one axis: row o holds 1 - l1 at i0 and l1 at i1 (added, so i0 == i1 gives 1)"""
    i0, i1, l1 = up_taps(n)
    M = torch.zeros(2 * n, n, dtype=torch.float64)
    r = torch.arange(2 * n)
    M.index_put_((r, i0), 1.0 - l1, accumulate=True)
    M.index_put_((r, i1), l1, accumulate=True)
    return M


def up2x_ref(x, f32_coord=False):
    """(B, C, H, W) -> (B, C, 2H, 2W) float64, rows then columns, by gathering the two taps (a 16400-row case needs no dense matrix)"""
    x = x.double()
    y0, y1, ly = up_taps(x.shape[2], f32_coord)
    x0, x1, lx = up_taps(x.shape[3], f32_coord)
    t = x[:, :, y0, :] * (1.0 - ly)[:, None] + x[:, :, y1, :] * ly[:, None]
    return t[..., x0] * (1.0 - lx) + t[..., x1] * lx


def up2x_matrix_ref(x):
    """the same map written with the two explicit weight matrices:  out = My x Mx^T"""
    return torch.einsum("oh,bchw,pw->bcop", up_matrix(x.shape[2]), x.double(), up_matrix(x.shape[3]))


def up2x_bwd_ref(dy, H, W):
    """adjoint of up2x_ref:  din = My^T dy Mx,  (B, C, 2H, 2W) -> (B, C, H, W) float64"""
    assert dy.shape[2] == 2 * H and dy.shape[3] == 2 * W
    return torch.einsum("oh,bcop,pw->bchw", up_matrix(H), dy.double(), up_matrix(W))


# ---- HRNet fuse:  out = relu?( sum_t src_t[b, :, y >> sh_t, x >> sh_t] )   (nearest upsample by 2^sh: source index = floor(dst / 2^sh))
def _nearest(src, sh, H, W):
    assert src.shape[2] << sh == H and src.shape[3] << sh == W
    return src[:, :, torch.arange(H) >> sh][..., torch.arange(W) >> sh]


def fuse_sum_ref(srcs, shifts, relu):
    """float64 sum of the nearest-upsampled sources"""
    H, W = srcs[0].shape[2] << shifts[0], srcs[0].shape[3] << shifts[0]
    acc = torch.zeros(srcs[0].shape[0], srcs[0].shape[1], H, W, dtype=torch.float64)
    for s, sh in zip(srcs, shifts):
        acc = acc + _nearest(s.double(), sh, H, W)
    return acc.clamp_min(0.0) if relu else acc


def fuse_sum_ref_f32(srcs, shifts, relu):
    """the documented arithmetic: term 0 is copied, terms 1 .. nsrc-1 are added in that order in fp32 (IEEE adds: one defined result)"""
    H, W = srcs[0].shape[2] << shifts[0], srcs[0].shape[3] << shifts[0]
    acc = None
    for s, sh in zip(srcs, shifts):
        t = _nearest(s.float(), sh, H, W)
        acc = t.clone() if acc is None else acc + t
    return torch.where(acc > 0, acc, torch.zeros_like(acc)) if relu else acc


def fuse_sum_bwd_ref(dout, out, shift, relu):
    """gradient of ONE source:  dsrc[y, x] = sum over the 2^sh x 2^sh block of dout * [out > 0]  (no mask without the ReLU)"""
    dz = dout.double()
    if relu:
        dz = dz * (out > 0)
    B, Cc, H, W = dz.shape
    n = 1 << shift
    return dz.reshape(B, Cc, H // n, n, W // n, n).sum((3, 5))


# ---- F.max_pool2d(x, 3, 2, 1): -inf padding; the window is scanned in row-major order with a strict >, so the FIRST maximum wins
def _pool_scan(x):
    B, Cc, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    m = torch.full((B, Cc, Ho, Wo), float("-inf"), dtype=x.dtype)
    arg = torch.full((B, Cc, Ho, Wo), -1, dtype=torch.int64)
    for oy in range(Ho):
        for ox in range(Wo):
            for r in range(3):
                for s in range(3):
                    y, xx = 2 * oy - 1 + r, 2 * ox - 1 + s
                    if not (0 <= y < H and 0 <= xx < W):
                        continue
                    v = x[:, :, y, xx]
                    upd = v > m[:, :, oy, ox]
                    m[:, :, oy, ox] = torch.where(upd, v, m[:, :, oy, ox])
                    arg[:, :, oy, ox] = torch.where(upd, torch.full_like(arg[:, :, oy, ox], y * W + xx), arg[:, :, oy, ox])
    return m, arg


POOL_SHAPES = [(2, 16, 2, 2), (1, 8, 2, 6), (1, 8, 4, 2), (2, 24, 6, 10)]


def pool_inputs(shape):
    """distinct values; a post-ReLU map (about half the entries exactly 0: most windows hold ties); one big tie"""
    x = det_tensor("r_mp%s" % (shape,), shape)
    return {"distinct": x, "relu": x.clamp_min(0), "const": torch.full(shape, 0.5)}


def maxpool_ref(x):
    return _pool_scan(x)[0]


def maxpool_bwd_ref(x, dout):
    """every window hands its gradient to its arg-max pixel (the first maximum); float64"""
    B, Cc, H, W = x.shape
    _, arg = _pool_scan(x)
    din = torch.zeros(B, Cc, H * W, dtype=torch.float64)
    din.scatter_add_(2, arg.reshape(B, Cc, -1), dout.double().reshape(B, Cc, -1))
    return din.reshape(B, Cc, H, W)


# ---- layout at the boundary
def nchw_to_nhwc_ref(x, cphys, torch_dtype):
    """(B, C, H, W) fp32 -> (B, H, W, cphys) `torch_dtype`: channel c of pixel (h, w) lands at [b, h, w, c]; channels >= C are zero"""
    B, Cc, H, W = x.shape
    out = torch.zeros(B, H, W, cphys, dtype=torch_dtype)
    for c in range(Cc):
        out[:, :, :, c] = x[:, c].to(torch_dtype)
    return out


def nhwc_to_nchw_ref(t, Cc, coff):
    """channels [coff, coff + C) of a (B, H, W, cstride) tensor -> (B, C, H, W) fp32 (widening is exact)"""
    B, H, W, _ = t.shape
    out = torch.empty(B, Cc, H, W, dtype=torch.float32)
    for c in range(Cc):
        out[:, c] = t[:, :, :, coff + c].float()
    return out


IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def u8_norm_ref(u8, cphys, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """(B, H, W, 3) uint8 -> (B, H, W, cphys) fp32: ToTensor's x / 255, then Normalize's (x - mean) / std, every step an IEEE float32
    operation on float32 mean / std (numpy float32 arrays: no reciprocal, no wider intermediate); channels >= 3 are zero"""
    x = np.asarray(u8).astype(np.float32)
    v = x / np.float32(255.0)
    v = (v - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    assert v.dtype == np.float32
    out = np.zeros(x.shape[:3] + (cphys,), np.float32)
    out[..., :3] = v
    return torch.from_numpy(out)
