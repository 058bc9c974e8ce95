"""tests/cl_helper_refs.py against torch (CPU only): the proof that the references, not the kernels, define "right" for
tests/test_gpu_cl_helpers.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cl_helper_refs as R
from tests.common import det_tensor

UP_SHAPES = [(1, 2, 1, 1), (2, 3, 1, 5), (2, 3, 4, 1), (1, 4, 3, 2), (2, 3, 5, 7), (1, 2, 16, 2)]


@pytest.mark.parametrize("shape", UP_SHAPES)
def test_up2x_ref_is_interpolate_align_corners(shape):
    x = det_tensor("r_up%s" % (shape,), shape).double()
    want = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    assert float((R.up2x_ref(x) - want).abs().max()) <= 1e-14
    assert float((R.up2x_matrix_ref(x) - want).abs().max()) <= 1e-14


@pytest.mark.parametrize("shape", [(1, 2, 1, 5), (2, 3, 5, 7), (1, 2, 2, 3000), (1, 2, 16400, 2)])
def test_up2x_ref_on_the_float32_coordinate_is_float32_interpolate(shape):
    """what a float32 tensor gets from ATen: the coordinate scale * dst is formed in float32.  The reference with that coordinate
    follows torch's float32 result to float32 rounding at every size; the exact map does so only while the axis is short."""
    x = det_tensor("r_upf%s" % (shape,), shape)
    want = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True).double()
    rel = lambda ref: float(((want - ref).abs() / (1 + ref.abs())).max())      # noqa: E731
    assert rel(R.up2x_ref(x, f32_coord=True)) <= 5e-7
    exact = rel(R.up2x_ref(x))
    assert exact <= 5e-7 if max(shape[2:]) <= 8 else exact >= 1e-4             # n = 3000: 3e-4; n = 16400: 1.8e-3


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_up_matrix_rows_are_convex_weights(n):
    M = R.up_matrix(n)
    assert M.shape == (2 * n, n) and float(M.min()) >= 0.0
    assert float((M.sum(1) - 1).abs().max()) <= 1e-15
    assert M[0, 0] == 1.0 and abs(float(M[-1, -1]) - 1.0) <= 1e-15          # align_corners: the ends map onto the ends
    if n == 1:
        assert torch.equal(M, torch.ones(2, 1, dtype=torch.float64))       # scale 0: both outputs are the one input


@pytest.mark.parametrize("shape", UP_SHAPES)
@torch.enable_grad()
def test_up2x_bwd_ref_is_autograd_and_the_adjoint(shape):
    B, Cc, H, W = shape
    x = det_tensor("r_upx%s" % (shape,), shape).double().requires_grad_(True)
    dy = det_tensor("r_upd%s" % (shape,), (B, Cc, 2 * H, 2 * W)).double()
    y = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    (want,) = torch.autograd.grad(y, x, dy)
    got = R.up2x_bwd_ref(dy, H, W)
    assert float((got - want).abs().max()) <= 1e-14
    lhs, rhs = float((R.up2x_ref(x.detach()) * dy).sum()), float((x.detach() * got).sum())
    assert abs(lhs - rhs) <= 1e-12 * (1 + abs(lhs))
    if H == 1:                                                              # the H = 1 gradient is the sum of both output rows
        col = torch.einsum("bcop,pw->bcow", dy, R.up_matrix(W))
        assert float((got[:, :, 0] - (col[:, :, 0] + col[:, :, 1])).abs().max()) <= 1e-14
    if W == 1:
        row = torch.einsum("oh,bcop->bchp", R.up_matrix(H), dy)
        assert float((got[..., 0] - (row[..., 0] + row[..., 1])).abs().max()) <= 1e-14


FUSE_CASES = [((2, 8, 32, 32), (0,), 0), ((1, 8, 32, 32), (0, 5), 1), ((2, 6, 8, 12), (1, 0, 2), 0), ((1, 4, 32, 32), (0, 1, 3, 5), 1),
              ((1, 4, 16, 48), (4, 2, 0, 3), 0)]


def _fuse_srcs(tag, shape, shifts):
    B, Cc, H, W = shape
    return [det_tensor("%s%d_%d" % (tag, k, sh), (B, Cc, H >> sh, W >> sh)) for k, sh in enumerate(shifts)]


@pytest.mark.parametrize("shape,shifts,relu", FUSE_CASES)
def test_fuse_sum_refs_are_nearest_upsample_sums(shape, shifts, relu):
    srcs = _fuse_srcs("r_fs", shape, shifts)
    want = torch.zeros(shape, dtype=torch.float64)
    for s, sh in zip(srcs, shifts):
        want = want + (F.interpolate(s.double(), scale_factor=1 << sh, mode="nearest") if sh else s.double())
    want = F.relu(want) if relu else want
    got = R.fuse_sum_ref(srcs, shifts, relu)
    assert torch.equal(got, want)
    g32 = R.fuse_sum_ref_f32(srcs, shifts, relu)
    assert g32.dtype == torch.float32
    assert float((g32.double() - got).abs().max()) <= len(shifts) * 2.0 ** -24 * float(sum(s.abs().max() for s in srcs))


def test_fuse_sum_ref_f32_one_term_is_a_bit_copy_and_the_order_is_left_to_right():
    s = det_tensor("r_fs_copy", (1, 4, 4, 4))
    s[0, 0, 0, :2] = torch.tensor([-0.0, 0.0])
    out = R.fuse_sum_ref_f32([s], (0,), 0)
    assert torch.equal(out.view(torch.int32), s.view(torch.int32))          # -0.0 survives: term 0 is copied, not added to +0.0
    a, b, c = (torch.full((1, 1, 1, 1), v) for v in (1.0, 2.0 ** -24, 2.0 ** -24))
    assert float(R.fuse_sum_ref_f32([a, b, c], (0, 0, 0), 0)) == 1.0        # (1 + e) + e: each e is lost;  1 + (e + e) would be 1 + 2^-23
    assert float(R.fuse_sum_ref_f32([b, c, a], (0, 0, 0), 0)) == 1.0 + 2.0 ** -23


@pytest.mark.parametrize("shift", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("relu", [0, 1])
@torch.enable_grad()
def test_fuse_sum_bwd_ref_is_avg_pool_and_autograd(shift, relu):
    Hs, Ws = (1, 1) if shift == 5 else (2, 3)
    H, W = Hs << shift, Ws << shift
    dout = det_tensor("r_fb_d%d" % shift, (2, 4, H, W)).double()
    src = det_tensor("r_fb_s%d" % shift, (2, 4, Hs, Ws)).double().requires_grad_(True)
    other = det_tensor("r_fb_o%d" % shift, (2, 4, H, W)).double()
    z = other + (F.interpolate(src, scale_factor=1 << shift, mode="nearest") if shift else src)
    out = F.relu(z) if relu else z
    (want,) = torch.autograd.grad(out, src, dout)
    got = R.fuse_sum_bwd_ref(dout, out.detach() if relu else None, shift, relu)
    assert float((got - want).abs().max()) <= 1e-12
    dz = dout * (out.detach() > 0) if relu else dout
    pooled = F.avg_pool2d(dz, 1 << shift) * float(4 ** shift)
    assert float((got - pooled).abs().max()) <= 1e-12


@pytest.mark.parametrize("shape", R.POOL_SHAPES)
@pytest.mark.parametrize("kind", ["distinct", "relu", "const"])
@torch.enable_grad()
def test_maxpool_refs_are_max_pool2d_and_its_cpu_gradient(shape, kind):
    x = R.pool_inputs(shape)[kind].double()
    B, Cc, H, W = shape
    assert torch.equal(R.maxpool_ref(x), F.max_pool2d(x, 3, 2, 1))
    dout = det_tensor("r_mpd%s" % (shape,), (B, Cc, H // 2, W // 2)).double()
    xg = x.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(F.max_pool2d(xg, 3, 2, 1), xg, dout)     # ATen's CPU kernel: first maximum in row-major order
    got = R.maxpool_bwd_ref(x, dout)
    assert torch.equal(got, want)
    assert float((got.sum((2, 3)) - dout.sum((2, 3))).abs().max()) <= 1e-12  # each window gives its gradient to exactly one pixel
    if kind == "const":                                                      # one big tie: the first tap inside the image takes it
        hit = torch.zeros(H, W, dtype=torch.bool)
        for oy in range(H // 2):
            for ox in range(W // 2):
                hit[max(2 * oy - 1, 0), max(2 * ox - 1, 0)] = True
        assert torch.equal((got != 0).any(0).any(0), hit)


def test_layout_refs():
    x = det_tensor("r_lay", (2, 5, 3, 7))
    cl = R.nchw_to_nhwc_ref(x, 8, torch.float32)
    assert cl.shape == (2, 3, 7, 8) and float(cl[..., 5:].abs().max()) == 0.0
    assert torch.equal(cl[..., :5], x.permute(0, 2, 3, 1))
    assert cl[1, 2, 4, 3] == x[1, 3, 2, 4]
    assert torch.equal(R.nhwc_to_nchw_ref(cl, 5, 0), x)
    assert torch.equal(R.nhwc_to_nchw_ref(cl, 3, 2), x[:, 2:5])
    assert torch.equal(R.nchw_to_nhwc_ref(x, 8, torch.bfloat16)[..., :5], x.to(torch.bfloat16).permute(0, 2, 3, 1))


def test_u8_norm_ref_is_totensor_then_normalize():
    u8 = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1).repeat(2, 1, 1, 3)
    got = R.u8_norm_ref(u8, 5)
    chw = u8.permute(0, 3, 1, 2).to(torch.float32).div(255)                                    # transforms.ToTensor
    mean, std = torch.tensor(R.IMAGENET_MEAN), torch.tensor(R.IMAGENET_STD)
    want = chw.sub(mean[:, None, None]).div(std[:, None, None])                                # transforms.Normalize
    assert torch.equal(got[..., :3].view(torch.int32), want.permute(0, 2, 3, 1).contiguous().view(torch.int32))
    assert float(got[..., 3:].abs().max()) == 0.0
    wide = (np.arange(256, dtype=np.float64)[:, None] / 255 - np.array(R.IMAGENET_MEAN)) / np.array(R.IMAGENET_STD)
    assert float(np.abs(got[0, ..., :3].reshape(256, 3).numpy() - wide).max()) <= 4e-7 * 3     # a few float32 ulps at |v| <= 2.7
