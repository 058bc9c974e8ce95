"""The channels-last helper kernels (csrc/elementwise.hip, csrc/pack_layout.hip, the resampling / pooling backward of
csrc/train_dense.hip) against the float64 references of tests/cl_helper_refs.py, at the smallest shapes that reach each path:
H = 1 / W = 1, both channel-group index forms, both forms of the source coordinate (float32 up to 128 inputs on an axis, exact
beyond), channel slices on either side, every nsrc and shift, ties in the pool, the 32x33 transpose tile's ragged edges, the grid-z
rows of the upsample.

What is compared how:
  bit-exact    cp_fuse_sum_act (fp32: the ordered fp32 sum; bf16: that sum rounded once), cp_maxpool3x3s2, cp_nchw_to_nhwc,
               cp_nhwc_to_nchw_f32, cp_u8hwc_to_nhwc_norm, cp_fuse_sum_act_bwd_group against the single launches
  fp32 bound   forward upsample TOL[CP_F32]; backward (upsample, fuse, pool) TOLT[CP_F32]; both relative to 1 + |ref|
  bf16 bound   one fp32 computation and one rounding to nearest:  |dev - ref| <= 2^-8 |ref| + TOL[CP_F32] (1 + |ref|)
               (half a bf16 ulp of the result, plus the fp32 computation)
Every comparison prints its largest error as a fraction of its bound before it asserts."""
import ctypes as C

import pytest
import torch

from checkerpose_amd import _abi
from checkerpose_amd._abi import CP_BF16, CP_F32, CpFuseBwdItem
from tests import cl_helper_refs as R
from tests.common import det_tensor
from tests.test_gpu_parity import DT, TOL, close, dev, from_cl, rnd, rup, st, to_cl
from tests.test_gpu_train_dense import TOLT

pytestmark = pytest.mark.gpu
DTYPES = [CP_F32, CP_BF16]
BITS = {CP_F32: torch.int32, CP_BF16: torch.int16}
NAN = float("nan")


def slab(x, dtype, cstride, coff, fill):
    """NCHW fp32 CPU -> (B, H, W, cstride) `dtype` on the GPU: x in channels [coff, coff + C), `fill` everywhere else"""
    B, Cc, H, W = x.shape
    t = torch.full((B, H, W, cstride), fill, dtype=DT[dtype])
    t[..., coff:coff + Cc] = x.permute(0, 2, 3, 1).to(DT[dtype])
    return t.to(dev()).contiguous()


def slice_only(t, Cc, coff, fill):
    """the kernel wrote channels [coff, coff + C) and nothing else: the sentinel around the slice is intact, the slice is finite"""
    t = t.float().cpu()
    assert bool((t[..., :coff] == fill).all()) and bool((t[..., coff + Cc:] == fill).all()), "wrote outside the channel slice"
    assert bool(torch.isfinite(t[..., coff:coff + Cc]).all()), "left a prefilled NaN (or read one) inside the channel slice"


def bound(dtype, ref, tol32):
    ref = ref.double().abs()
    return tol32 * (1 + ref) if dtype == CP_F32 else 2.0 ** -8 * ref + TOL[CP_F32] * (1 + ref)


def within(label, dtype, got, ref, tol32, check=True):
    """fp32: the project's `close` at tol32; bf16: the derived bound of the module docstring.  -> worst error / bound
    (check=False: print the figure and leave the assertion to the caller)"""
    got, ref = got.double(), ref.double()
    ratio = float(((got - ref).abs() / bound(dtype, ref, tol32)).max())
    print("CLH %-44s %s  max|dev| %.4e  max|ref| %.4e  worst error / bound = %.4f"
          % (label, "fp32" if dtype == CP_F32 else "bf16", float(got.abs().max()), float(ref.abs().max()), ratio))
    assert bool(torch.isfinite(got).all())
    if check:
        if dtype == CP_F32:
            close(got, ref, tol32)
        assert ratio <= 1.0, "%s: error is %.3f of its bound" % (label, ratio)
    return ratio


def same_bits(a, b, dtype):
    assert a.dtype == b.dtype == DT[dtype] and a.shape == b.shape
    return torch.equal(a.cpu().contiguous().view(BITS[dtype]), b.cpu().contiguous().view(BITS[dtype]))


# ------------------------------------------------------------------------------------------------ bilinear x2, forward
# C = 32: shift path; C = 24: division path; 128 | 129 inputs on an axis: the last float32 coordinate | the first exact one
UP_SHAPES = [(1, 8, 1, 1), (2, 8, 1, 5), (2, 8, 4, 1), (1, 32, 3, 2), (2, 24, 3, 5), (1, 8, 128, 3), (1, 8, 129, 3), (1, 8, 3, 129)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", UP_SHAPES)
def test_upsample2x_edge_shapes_slice_to_slice(lib, dtype, shape):
    B, Cc, H, W = shape
    x = rnd(det_tensor("clh_up%s" % (shape,), shape), dtype)
    cs, co = Cc + 16, 8
    xin = slab(x, dtype, cs, co, NAN)                                   # a read outside the slice shows up as NaN
    out = torch.full((B, 2 * H, 2 * W, cs), 7.0, dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_upsample2x_bilinear_ac(st(), dtype, xin.data_ptr(), out.data_ptr(), B, H, W, Cc, cs, co, cs, co))
    torch.cuda.synchronize()
    slice_only(out, Cc, co, 7.0)
    within("upsample2x %s" % (shape,), dtype, from_cl(out[..., co:], Cc), R.up2x_ref(x), TOL[CP_F32])


GRID_Z_ROWS = (0, 65534, 65535, 65536, 65537, 65599)


def _up_grid_z(lib, dtype):
    """B * 2H = 65600 output rows: gridDim.y = 65535, gridDim.z = 2, row = blockIdx.z * gridDim.y + blockIdx.y"""
    B, Cc, H, W = 2, 8, 16400, 2
    x = rnd(det_tensor("clh_upz", (B, Cc, H, W)), dtype)
    xin = to_cl(x, dtype)
    out = torch.full((B, 2 * H, 2 * W, Cc), NAN, dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_upsample2x_bilinear_ac(st(), dtype, xin.data_ptr(), out.data_ptr(), B, H, W, Cc, Cc, 0, Cc, 0))
    torch.cuda.synchronize()
    return x, from_cl(out, Cc), (lambda t: t.permute(0, 2, 1, 3).reshape(B * 2 * H, Cc, 2 * W))


@pytest.mark.parametrize("dtype", DTYPES)
def test_upsample2x_rows_beyond_grid_y(lib, dtype):
    """every one of the 65600 rows, the rows either side of the gridDim.y seam by name, against the exact align_corners map.
    H = 16400 is far beyond the length up to which the kernel keeps ATen's float32 coordinate scale * dst (cp_up_coord: 128 inputs);
    that product would be off by 1e-3 of a pixel here, and torch's own float32 F.interpolate leaves the exact map by 90 times this
    bound on this input (tests/test_cl_helpers.py::test_up2x_ref_on_the_float32_coordinate_is_float32_interpolate)."""
    x, got, rows = _up_grid_z(lib, dtype)
    ref = R.up2x_ref(x)
    worst = [within("upsample2x grid-z row %d" % r, dtype, rows(got)[r], rows(ref)[r], TOL[CP_F32], check=False) for r in GRID_Z_ROWS]
    worst.append(within("upsample2x grid-z all rows", dtype, got, ref, TOL[CP_F32], check=False))
    assert max(worst) <= 1.0, "worst error is %.1f times the bound" % max(worst)
    if dtype == CP_F32:
        close(got, ref, TOL[CP_F32])


# ------------------------------------------------------------------------------------------------ bilinear x2, backward
def _up_bwd(lib, dtype, dy, base, accumulate, o_cs, o_co, i_cs, i_co):
    B, Cc, H, W = base.shape
    dyc = slab(dy, dtype, o_cs, o_co, NAN)
    dxc = slab(base if accumulate else torch.full_like(base, NAN), dtype, i_cs, i_co, 7.0)
    _abi.check(lib.cp_upsample2x_bilinear_ac_bwd(st(), dtype, dyc.data_ptr(), dxc.data_ptr(), B, H, W, Cc, o_cs, o_co, i_cs, i_co,
                                                 accumulate))
    torch.cuda.synchronize()
    return dxc


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", UP_SHAPES)
def test_upsample2x_bwd_edge_shapes_slice_to_slice(lib, dtype, shape):
    """H = 1 (W = 1): the scale is 0, both output rows (columns) map to source 0 and the gradient is their sum"""
    B, Cc, H, W = shape
    dy = rnd(det_tensor("clh_upd%s" % (shape,), (B, Cc, 2 * H, 2 * W)), dtype)
    base = rnd(det_tensor("clh_upb%s" % (shape,), shape), dtype)
    ref = R.up2x_bwd_ref(dy, H, W)
    for acc in (0, 1):
        dxc = _up_bwd(lib, dtype, dy, base, acc, Cc + 16, 8, Cc + 24, 16)
        slice_only(dxc, Cc, 16, 7.0)
        within("upsample2x_bwd %s acc %d" % (shape, acc), dtype, from_cl(dxc[..., 16:], Cc), ref + (base if acc else 0), TOLT[CP_F32])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 8, 1, 5), (2, 8, 4, 1), (2, 24, 3, 5), (1, 8, 129, 3)])
def test_upsample2x_forward_and_backward_are_adjoint(lib, dtype, shape):
    """<up(x), dy> == <x, up_bwd(dy)> in float64 from the two device results.  Each device element is within its per-element bound e
    of the exact map, so the two inner products differ by at most sum e(u) |dy| + sum e(g) |x| (the bounds taken at the device values)."""
    B, Cc, H, W = shape
    x = rnd(det_tensor("clh_adx%s" % (shape,), shape), dtype)
    dy = rnd(det_tensor("clh_ady%s" % (shape,), (B, Cc, 2 * H, 2 * W)), dtype)
    xin = to_cl(x, dtype)
    up = torch.full((B, 2 * H, 2 * W, Cc), NAN, dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_upsample2x_bilinear_ac(st(), dtype, xin.data_ptr(), up.data_ptr(), B, H, W, Cc, Cc, 0, Cc, 0))
    g = from_cl(_up_bwd(lib, dtype, dy, x, 0, Cc, 0, Cc, 0), Cc).double()
    u = from_cl(up, Cc).double()
    lhs, rhs = float((u * dy.double()).sum()), float((x.double() * g).sum())
    lim = float((bound(dtype, u, TOLT[CP_F32]) * dy.double().abs()).sum() + (bound(dtype, g, TOLT[CP_F32]) * x.double().abs()).sum())
    print("CLH adjoint %s %s  <up x, dy> %.9e  <x, up_bwd dy> %.9e  |difference| / bound = %.4f"
          % (shape, "fp32" if dtype == CP_F32 else "bf16", lhs, rhs, abs(lhs - rhs) / lim))
    assert abs(lhs - rhs) <= lim


# ------------------------------------------------------------------------------------------------ HRNet fuse sum, forward
FUSE_CASES = [  # (B, C, H, W, shifts, relu)
    (2, 8, 32, 32, (0,), 0),                 # the row carrier of netbuilder.py: a byte copy
    (2, 8, 4, 6, (0,), 1),
    (1, 8, 8, 8, (3, 0), 0),
    (1, 16, 32, 32, (0, 5), 1),              # the shift-5 source is 1x1
    (2, 24, 8, 12, (1, 0, 2), 0),
    (1, 8, 32, 32, (0, 1, 3, 5), 1),
    (1, 8, 16, 48, (4, 2, 0, 3), 0),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", FUSE_CASES)
def test_fuse_sum_is_the_ordered_fp32_sum(lib, dtype, case):
    B, Cc, H, W, shifts, relu = case
    srcs = [rnd(det_tensor("clh_fs%s_%d" % (case, k), (B, Cc, H >> sh, W >> sh)), dtype) for k, sh in enumerate(shifts)]
    srcs[0][0, 0, 0, 0], srcs[0][0, 1, 0, 0] = -0.0, 0.0
    dv = [to_cl(s, dtype) for s in srcs]
    arr = (C.c_void_p * 4)(*([t.data_ptr() for t in dv] + [None] * (4 - len(dv))))
    sh = (C.c_int32 * 4)(*(list(shifts) + [0] * (4 - len(shifts))))
    cs, co = Cc + 16, 8
    out = torch.full((B, H, W, cs), 7.0, dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_fuse_sum_act(st(), dtype, len(shifts), arr, sh, out.data_ptr(), B, H, W, Cc, relu, cs, co))
    torch.cuda.synchronize()
    slice_only(out, Cc, co, 7.0)
    ref = R.fuse_sum_ref_f32(srcs, shifts, relu).permute(0, 2, 3, 1).to(DT[dtype])
    got = out[..., co:co + Cc].cpu()
    assert torch.equal(got, ref)                                           # every value; +-0 compare equal here ...
    if not relu:
        assert same_bits(got, ref, dtype)                                  # ... and without the ReLU every bit, the sign of zero too
    if len(shifts) == 1 and not relu:
        assert same_bits(got, dv[0].cpu(), dtype)                          # one term, no activation: a byte copy of the source


# ------------------------------------------------------------------------------------------------ HRNet fuse sum, backward
def _fuse_bwd_case(tag, dtype, B, Cc, Hs, Ws, shift, relu):
    H, W = Hs << shift, Ws << shift
    dout = rnd(det_tensor("clh_fb_d%s" % (tag,), (B, Cc, H, W)), dtype)
    out = rnd(det_tensor("clh_fb_o%s" % (tag,), (B, Cc, H, W)), dtype).clamp_min(0)    # about half exact zeros ...
    out.view(-1)[::7] = -0.0                                                           # ... and -0.0: the mask is out > 0
    out.view(-1)[3::7] = 0.0
    base = rnd(det_tensor("clh_fb_b%s" % (tag,), (B, Cc, Hs, Ws)), dtype)
    return dout, (out if relu else None), base


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shift", [0, 1, 2, 3, 4, 5])
def test_fuse_sum_bwd_every_shift_with_and_without_relu(lib, dtype, shift):
    B, Cc = 2, 16
    Hs, Ws = {4: (2, 3), 5: (1, 1)}.get(shift, (3, 5))
    for relu in (0, 1):
        dout, out, base = _fuse_bwd_case((shift, relu), dtype, B, Cc, Hs, Ws, shift, relu)
        ref = R.fuse_sum_bwd_ref(dout, out, shift, relu)
        dc, oc = to_cl(dout, dtype), (to_cl(out, dtype) if relu else None)
        for acc in (0, 1):
            ds = to_cl(base if acc else torch.full_like(base, NAN), dtype)
            _abi.check(lib.cp_fuse_sum_act_bwd(st(), dtype, dc.data_ptr(), oc.data_ptr() if relu else None, ds.data_ptr(), B, Hs, Ws, Cc,
                                               shift, relu, acc))
            torch.cuda.synchronize()
            within("fuse_sum_bwd shift %d relu %d acc %d" % (shift, relu, acc), dtype, from_cl(ds, Cc), ref + (base if acc else 0),
                   TOLT[CP_F32])


@pytest.mark.parametrize("dtype", DTYPES)
def test_fuse_sum_bwd_group_equals_the_single_launches(lib, dtype):
    """the form the trainer launches: cp_fuse_sum_act_bwd_item per term, one cp_fuse_sum_act_bwd_group for the module"""
    B = 2
    members = [(12, 20, 16, 0, 1, 0), (3, 5, 8, 2, 0, 1), (1, 1, 24, 5, 1, 1), (2, 3, 8, 3, 0, 0)]   # (Hs, Ws, C, shift, relu, accumulate)
    E = lib.cp_chan_align(dtype)
    assert any((B * Hs * Ws * (Cc // E)) % 256 for Hs, Ws, Cc, _, _, _ in members) and B * 12 * 20 * (16 // E) > 256
    single, grouped, keep, items, nbs = [], [], [], [], []
    for k, (Hs, Ws, Cc, shift, relu, acc) in enumerate(members):
        dout, out, base = _fuse_bwd_case(("g", k), dtype, B, Cc, Hs, Ws, shift, relu)
        dc, oc = to_cl(dout, dtype), (to_cl(out, dtype) if relu else None)
        a, b = (to_cl(base if acc else torch.full_like(base, NAN), dtype) for _ in range(2))
        op = oc.data_ptr() if relu else None
        _abi.check(lib.cp_fuse_sum_act_bwd(st(), dtype, dc.data_ptr(), op, a.data_ptr(), B, Hs, Ws, Cc, shift, relu, acc))
        it, nb = CpFuseBwdItem(), C.c_uint32()
        _abi.check(lib.cp_fuse_sum_act_bwd_item(dtype, dc.data_ptr(), op, b.data_ptr(), B, Hs, Ws, Cc, shift, relu, acc, C.byref(it), C.byref(nb)))
        assert nb.value == (B * Hs * Ws * (Cc // E) + 255) // 256
        within("fuse_sum_bwd group member %d" % k, dtype, from_cl(a, Cc), R.fuse_sum_bwd_ref(dout, out, shift, relu) + (base if acc else 0),
               TOLT[CP_F32])
        single.append(a), grouped.append(b), keep.extend([dc, oc]), items.append(it), nbs.append(nb.value)
    raw, prefix, total = _abi.device_table(items, nbs, dev())
    _abi.check(lib.cp_fuse_sum_act_bwd_group(st(), dtype, raw.data_ptr(), prefix.data_ptr(), len(items), total))
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(single, grouped)):
        assert same_bits(a, b, dtype), "member %d" % k


# ------------------------------------------------------------------------------------------------ max pool 3x3 / s2 / p1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.POOL_SHAPES)
def test_maxpool_forward_exact_and_backward_first_maximum(lib, dtype, shape):
    B, Cc, H, W = shape
    dout = rnd(det_tensor("clh_mpd%s" % (shape,), (B, Cc, H // 2, W // 2)), dtype)
    base = rnd(det_tensor("clh_mpb%s" % (shape,), shape), dtype)
    dc = to_cl(dout, dtype)
    for kind, x in R.pool_inputs(shape).items():
        x = rnd(x, dtype)
        xin = to_cl(x, dtype)
        o = torch.full((B, H // 2, W // 2, Cc), NAN, dtype=DT[dtype], device=dev())
        _abi.check(lib.cp_maxpool3x3s2(st(), dtype, xin.data_ptr(), o.data_ptr(), B, H, W, Cc))
        torch.cuda.synchronize()
        assert torch.equal(from_cl(o, Cc), R.maxpool_ref(x)), kind                          # a max has no rounding
        ref = R.maxpool_bwd_ref(x, dout)
        for acc in (0, 1):
            di = to_cl(base if acc else torch.full_like(base, NAN), dtype)
            _abi.check(lib.cp_maxpool3x3s2_bwd(st(), dtype, xin.data_ptr(), dc.data_ptr(), di.data_ptr(), B, H, W, Cc, acc))
            torch.cuda.synchronize()
            got = from_cl(di, Cc)
            within("maxpool_bwd %s %s acc %d" % (shape, kind, acc), dtype, got, ref + (base if acc else 0), TOLT[CP_F32])
            if not acc:      # conservation: every window gives its gradient to exactly one pixel (error: the per-element bounds, summed)
                gap = (got.double().sum((2, 3)) - dout.double().sum((2, 3))).abs()
                lim = bound(dtype, ref, TOLT[CP_F32]).sum((2, 3))
                print("CLH maxpool_bwd %s %s conservation  worst gap / bound = %.4f" % (shape, kind, float((gap / lim).max())))
                assert bool((gap <= lim).all()), kind
                assert torch.equal(got != 0, ref != 0), kind                                # the same pixels win, whatever the rounding


# ------------------------------------------------------------------------------------------------ layout at the boundary
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,cphys", [((2, 3, 5, 7), 8), ((1, 37, 3, 11), 40)])
def test_nchw_to_nhwc_exact_with_zero_padding(lib, dtype, shape, cphys):
    B, Cc, H, W = shape
    x = det_tensor("clh_n2h%s" % (shape,), shape)
    xd = x.to(dev())
    out = torch.full((B, H, W, cphys), NAN, dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_nchw_to_nhwc(st(), dtype, xd.data_ptr(), out.data_ptr(), B, Cc, H, W, cphys))
    torch.cuda.synchronize()
    assert same_bits(out, R.nchw_to_nhwc_ref(x, cphys, DT[dtype]), dtype)                  # fp32: a byte copy; bf16: rounded once
    assert bool((out[..., Cc:].cpu().view(BITS[dtype]) == 0).all())                        # the padding is +0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cc", [1, 31, 33, 70])
def test_nhwc_slice_to_nchw_exact_on_ragged_tiles(lib, dtype, Cc):
    B = 3
    cs, co = rup(Cc, 8) + 16, 8
    for H, W in ((1, 1), (1, 31), (3, 11), (7, 11)):                                       # H W = 1, 31, 33, 77 against the 32-pixel tile
        x = rnd(det_tensor("clh_h2n%d_%d" % (Cc, H * W), (B, Cc, H, W)), dtype)
        xin = slab(x, dtype, cs, co, NAN)
        out = torch.full((B, Cc, H, W), NAN, dtype=torch.float32, device=dev())
        _abi.check(lib.cp_nhwc_to_nchw_f32(st(), dtype, xin.data_ptr(), out.data_ptr(), B, Cc, H, W, cs, co))
        torch.cuda.synchronize()
        got = out.cpu()
        assert bool(torch.isfinite(got).all()), "H W = %d: output not fully written, or read outside the slice" % (H * W)
        assert torch.equal(got.view(torch.int32), R.nhwc_to_nchw_ref(xin.cpu(), Cc, co).view(torch.int32))
        assert torch.equal(got, x)


@pytest.mark.parametrize("dtype,cphys", [(CP_F32, 4), (CP_F32, 5), (CP_BF16, 8)])
def test_u8_normalise_every_byte_value_exact(lib, dtype, cphys):
    v = torch.arange(256, dtype=torch.int64)
    img = torch.stack([(v * m + 11 * c) % 256 for c, m in enumerate((1, 3, 7))], -1).reshape(16, 16, 3)    # odd multipliers: permutations
    u8 = torch.stack([img, 255 - img]).to(torch.uint8)                                                  # B = 2
    assert all(len(set(u8[b, ..., c].reshape(-1).tolist())) == 256 for b in range(2) for c in range(3))
    out = torch.full((2, 16, 16, cphys), NAN, dtype=DT[dtype], device=dev())
    mean, std = (C.c_float * 3)(*R.IMAGENET_MEAN), (C.c_float * 3)(*R.IMAGENET_STD)
    ud = u8.to(dev())
    _abi.check(lib.cp_u8hwc_to_nhwc_norm(st(), dtype, ud.data_ptr(), out.data_ptr(), 2, 16, 16, cphys, mean, std))
    torch.cuda.synchronize()
    assert same_bits(out, R.u8_norm_ref(u8, cphys).to(DT[dtype]), dtype)
    assert bool((out[..., 3:].cpu().view(BITS[dtype]) == 0).all())
