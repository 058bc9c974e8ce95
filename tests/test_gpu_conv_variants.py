"""GPU (-m gpu): the conv kernels' large-batch instantiations and the training program's call forms, one test per variant.

tests/test_gpu_parity.py and tests/test_gpu_train_dense.py reach the instantiations the dispatchers pick at small sizes, in the
forward form (fresh dense output, residual absent or a separate tensor).  Here every case names the kernel symbol it was written
for (cp_last_kernel(), a literal in the table: a moved dispatcher threshold fails the test instead of silently re-pointing it) and
runs the forms the trainer and the decoder use: residual aliasing the output (the data-gradient accumulate `residual = out = gx`),
operands that are channel slices of wider buffers, strided scatter through explicit output strides.

Reference: torch conv2d on the CPU in float64 over operands rounded to the storage type; affine, residual and activation in
float64; data gradients = torch.autograd.grad of that forward plus the buffer's previous contents.
Bounds (got vs. float64 reference):
  fp32 : |d| <= 2e-5 * (1 + |ref|)                       (TOL[CP_F32], the per-op contract)
  bf16 : |d| <= 3e-2 * (1 + |ref|)                       (TOL[CP_BF16], the hard bound) AND
         |d| <= 2^-8 * |ref| + 2e-5 * (1 + |ref|)        (derived: operands are bf16-exact and accumulation is fp32, so beyond the
                                                          fp32 term the only error is ONE round-to-nearest of the output row)
         bf16 keeps 8 significant bits, so one round-to-nearest is at most half an ulp = 2^-8 relative (reached just above a power
         of two, 2^-9 just below the next): a correct kernel sits right under this bound (observed 0.96 .. 0.99 of it), while
         truncation (up to 2^-7) or a second rounding on the way (up to 2^-8 + 2^-9) breaks it.
Layout checks: input channels outside the operand slice are NaN (a read outside poisons the result); everything of an output
buffer outside the addressed region must keep its bits (NaN sentinel, compared as integers); physical pad channels are exactly zero.
Every test prints one `CONVVAR` line (symbol, worst error relative to each bound) before it asserts.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from checkerpose_amd import _abi
from checkerpose_amd._abi import ACT_LEAKY, ACT_NONE, ACT_RELU, CP_BF16, CP_F32, CpConvDesc
from tests.common import det_tensor
from tests.test_gpu_parity import DT, TOL, dev, from_cl, pack, rnd, rup, st, to_cl

pytestmark = pytest.mark.gpu
F32, BF16 = CP_F32, CP_BF16
RAW = {CP_F32: torch.int32, CP_BF16: torch.int16}
DTN = {CP_F32: "fp32", CP_BF16: "bf16"}
SLOPE = float(torch.tensor(0.01, dtype=torch.float32))        # the slope as the device sees it
NAN = float("nan")


def esz(dtype):
    return 8 if dtype == CP_BF16 else 4


def slab(x, dtype, coff=0, extra=0, fill=NAN):
    """NCHW fp32 (CPU) -> channels-last (B, H, W, coff + Cphys + extra) on the GPU: channels [coff, coff + Cphys) hold x, zero
    padded to the physical count; every other channel holds `fill`."""
    B, Cc, H, W = x.shape
    cp = rup(Cc, esz(dtype))
    t = torch.full((B, H, W, coff + cp + extra), fill, dtype=DT[dtype])
    t[..., coff:coff + cp] = 0
    t[..., coff:coff + Cc] = x.permute(0, 2, 3, 1).to(DT[dtype])
    return t.to(dev()).contiguous()


def fresh(B, H, W, ctot, dtype):
    return torch.full((B, H, W, ctot), NAN, dtype=DT[dtype], device=dev())


def ostr_of(buf, coff=0):
    _, H, W, ct = buf.shape
    return (coff, H * W * ct, W * ct, ct, 1)


def vec(n, t=None):
    v = torch.zeros(rup(n, 16))
    if t is not None:
        v[:n] = t
    return v.to(dev())


def affine(name, Cout, random):
    """(scale, shift) fp32 on the CPU: random per channel, or the trainer's (1, 0)"""
    if random:
        return 1.0 + 0.3 * det_tensor(name + "s", (Cout,)), 0.2 * det_tensor(name + "t", (Cout,))
    return torch.ones(Cout), torch.zeros(Cout)


def conv64(x, w, stride, pad):
    with torch.no_grad():
        return F.conv2d(x.double(), w.double(), None, stride, pad)


def epilogue64(y, scale, shift, res, act):
    y = y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    if act == ACT_RELU:
        y = y.clamp_min(0.0)
    elif act == ACT_LEAKY:
        y = torch.where(y > 0, y, y * SLOPE)
    return y


def dgrad64(xshape, w, dy, stride, pad):
    """d/dx of conv2d(x, w, stride, pad) against dy, in float64"""
    x = torch.zeros(xshape, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        y = F.conv2d(x, w.double(), None, stride, pad)
        assert tuple(y.shape) == tuple(dy.shape)
        (dx,) = torch.autograd.grad(y, x, dy.double())
    return dx


def launch(lib, fn, dtype, xin, cin, in_coff, pw, sc, sh, geom, out_hw, cout, out, ostr, res=None, act=ACT_NONE, ksplit=0):
    """one launch of cp_conv2d_igemm / cp_conv3x3_halo / cp_gemm_rows; returns the symbol the library recorded"""
    R, S, stride, pad = geom
    B, H, W, cs = xin.shape
    d = CpConvDesc()
    d.dtype, d.out_f32, d.B, d.H, d.W = dtype, 0, B, H, W
    d.Cin, d.in_cstride, d.in_coff = cin, cs, in_coff
    d.R, d.S, d.stride, d.pad, d.Ho, d.Wo, d.Cout = R, S, stride, pad, out_hw[0], out_hw[1], cout
    d.act, d.slope = act, (SLOPE if act == ACT_LEAKY else 0.0)
    d.o_base, d.o_sb, d.o_sy, d.o_sx, d.o_sc = ostr
    d.ksplit = ksplit
    _abi.check(fn(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                  res.data_ptr() if res is not None else None, out.data_ptr()), "launch")
    torch.cuda.synchronize()
    return lib.cp_last_kernel().decode()


def pack_halo(lib, dtype, w, cin_phys):
    Cout, Cin = w.shape[0], w.shape[1]
    buf = torch.empty(lib.cp_packed_halo_weight_bytes(dtype, Cout, cin_phys), dtype=torch.uint8, device=dev())
    wd = w.contiguous().to(dev())
    _abi.check(lib.cp_pack_conv3x3_halo_weight(st(), dtype, wd.data_ptr(), Cout, Cin, cin_phys, buf.data_ptr()), "pack halo")
    torch.cuda.synchronize()
    return buf


def pack_gemm(lib, dtype, w, cin_phys):
    Cout, Cin = w.shape[0], w.shape[1]
    buf = torch.empty(lib.cp_packed_gemm_weight_bytes(dtype, Cout, cin_phys), dtype=torch.uint8, device=dev())
    wd = w.contiguous().to(dev())
    _abi.check(lib.cp_pack_gemm_weight(st(), dtype, wd.data_ptr(), Cout, Cin, cin_phys, buf.data_ptr()), "pack gemm")
    torch.cuda.synchronize()
    return buf


def weight_dgrad(lib, w):
    """cp_weight_dgrad: (Cout, Cin, R, S) -> (Cin, Cout, R, S), taps flipped (fp32, CPU), as TrainProgram.weight_dgrad does"""
    Cout, Cin, R, S = w.shape
    wd = w.contiguous().to(dev())
    wt = torch.empty(Cin, Cout, R, S, device=dev())
    _abi.check(lib.cp_weight_dgrad(st(), wd.data_ptr(), Cout, Cin, R, S, wt.data_ptr()), "cp_weight_dgrad")
    torch.cuda.synchronize()
    return wt.cpu()


def verify(part, sym, dtype, buf, before, coff, Cout, ref):
    """buf (B, H, W, ctot) after the launch(es), `before` its contents before; the slice [coff, coff + Cphys) is the output.
    Outside the slice: bit-identical; pad channels: exactly zero; logical channels: within the bounds of the module docstring."""
    cp = rup(Cout, esz(dtype))
    ctot = buf.shape[-1]
    if ctot > cp:
        outside = torch.ones(ctot, dtype=torch.bool, device=buf.device)
        outside[coff:coff + cp] = False
        assert torch.equal(buf.view(RAW[dtype])[..., outside], before.view(RAW[dtype])[..., outside]), \
            "%s: channels outside the output slice changed" % sym
    if cp > Cout:
        assert float(buf[..., coff + Cout:coff + cp].float().abs().max()) == 0.0, "%s: padded channels must be exactly zero" % sym
    got = from_cl(buf[..., coff:coff + cp], Cout).double()
    assert tuple(got.shape) == tuple(ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: unwritten or poisoned output elements" % sym
    d, a = (got - ref).abs(), ref.abs()
    err = float((d / (1 + a)).max())
    hard = float((d / (TOL[dtype] * (1 + a))).max())
    derived = float((d / (2.0 ** -8 * a + 2e-5 * (1 + a))).max()) if dtype == CP_BF16 else 0.0
    print("CONVVAR part=%s dtype=%s sym=%s err=%.3e of_hard=%.3f of_derived=%.3f" % (part, DTN[dtype], sym, err, hard, derived))
    assert hard <= 1.0, "%s: max |d| / (1 + |ref|) = %.3e > %.1e" % (sym, err, TOL[dtype])
    assert derived <= 1.0, "%s: %.3f x the derived bf16 bound 2^-8 |ref| + 2e-5 (1 + |ref|)" % (sym, derived)


# ------------------------------------------------------------------------------------------------ A1: conv_igemm_kernel<*, 4, *>
# 3x3 / pad 1 onto a 137 x 137 map: M = 18769 = 73.3 blocks of 256 pixels (partial last block, 6 idle workgroups from the grid's
# round-up to 8), Cin = 8 (fp32) / 16 (bf16) -> KC = 5: > 4 (MT = 4 from 512 blocks) and below the split-K floor of 6.
# (dtype, Cout, stride, random affine, act, residual: None | "sep" | "alias", output a channel slice, expected symbol)
# Over the 7 cases of a dtype: affine 4x, ReLU 3x, leaky 2x, none 2x, separate residual 3x, residual aliasing the output 4x.
A1_CASES = [
    (F32, 108, 1, True, ACT_RELU, "alias", False, "conv_igemm_kernel<F32Tag, 4, 1>"),      # 7 tiles, the 7th holds 12 channels
    (F32, 224, 1, False, ACT_LEAKY, "sep", False, "conv_igemm_kernel<F32Tag, 4, 2>"),
    (F32, 336, 1, True, ACT_NONE, "alias", False, "conv_igemm_kernel<F32Tag, 4, 3>"),
    (F32, 512, 1, False, ACT_RELU, "sep", False, "conv_igemm_kernel<F32Tag, 4, 4>"),
    (F32, 556, 1, True, ACT_LEAKY, "alias", False, "conv_igemm_kernel<F32Tag, 4, 5>"),     # 35 tiles, the last holds 12 channels
    (F32, 224, 2, True, ACT_NONE, "sep", False, "conv_igemm_kernel<F32Tag, 4, 2>"),        # 274 x 274 / stride 2 -> 137 x 137
    (F32, 108, 1, False, ACT_RELU, "alias", True, "conv_igemm_kernel<F32Tag, 4, 1>"),      # o_base = 12, o_sx = Cout + 20
    (BF16, 108, 1, True, ACT_RELU, "alias", False, "conv_igemm_kernel<BF16Tag, 4, 1>"),    # ... and 4 physical pad channels
    (BF16, 224, 1, False, ACT_LEAKY, "sep", False, "conv_igemm_kernel<BF16Tag, 4, 2>"),
    (BF16, 336, 1, True, ACT_NONE, "alias", False, "conv_igemm_kernel<BF16Tag, 4, 3>"),
    (BF16, 512, 1, False, ACT_RELU, "sep", False, "conv_igemm_kernel<BF16Tag, 4, 4>"),
    (BF16, 556, 1, True, ACT_LEAKY, "alias", False, "conv_igemm_kernel<BF16Tag, 4, 5>"),
    (BF16, 224, 2, True, ACT_NONE, "sep", False, "conv_igemm_kernel<BF16Tag, 4, 2>"),
    (BF16, 108, 1, False, ACT_RELU, "alias", True, "conv_igemm_kernel<BF16Tag, 4, 1>"),
]


def _id(case):
    return "-".join(str(v) for v in case[:-1]) if isinstance(case, tuple) else str(case)


@pytest.mark.parametrize("case", A1_CASES, ids=_id)
def test_igemm_mt4_tiles(lib, case):
    """the 256-pixel tiled kernel (what runs at training and benchmark batch) with its MFMA-layout epilogue: all ten
    instantiations, both ksplit settings (KC = 5 is below the split-K floor: the same kernel)"""
    dtype, Cout, stride, rand_aff, act, resmode, sliced, expect = case
    Cin, Ho = (8 if dtype == CP_F32 else 16), 137
    Hin = Ho if stride == 1 else 2 * Ho
    key = "a1%s" % (case[:7],)
    x = rnd(det_tensor(key + "x", (1, Cin, Hin, Hin)), dtype)
    w = rnd(det_tensor(key + "w", (Cout, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5 * 1.7), dtype)
    scale, shift = affine(key, Cout, rand_aff)
    res = rnd(det_tensor(key + "r", (1, Cout, Ho, Ho)), dtype)
    ref = epilogue64(conv64(x, w, stride, 1), scale, shift, res, act)
    assert tuple(ref.shape) == (1, Cout, Ho, Ho)
    xin = to_cl(x, dtype)
    pw = pack(lib, dtype, w, xin.shape[-1], 3, 3)
    sc, sh = vec(Cout, scale), vec(Cout, shift)
    cp = rup(Cout, esz(dtype))
    coff, extra = (12, 8) if sliced else (0, 0)
    for ksplit in (0, -1):
        if resmode == "alias":
            out = slab(res, dtype, coff, extra)
            rbuf = out
        else:
            out = fresh(1, Ho, Ho, coff + cp + extra, dtype)
            rbuf = slab(res, dtype, coff, extra)
        before = out.clone()
        sym = launch(lib, lib.cp_conv2d_igemm, dtype, xin, xin.shape[-1], 0, pw, sc, sh, (3, 3, stride, 1), (Ho, Ho), cp, out,
                     ostr_of(out, coff), rbuf, act, ksplit)
        assert sym == expect
        verify("A1", sym, dtype, out, before, coff, Cout, ref)


# ------------------------------------------------------------------------------------------------ A2: the two missing split-K forms
A2_CASES = [  # (B, Cin, H, W, Cout, expected symbol): bf16, ksplit = 0, ragged maps (the last 32-pixel block is partial)
    (1, 24, 63, 65, 40, "conv_igemm_splitk_kernel<BF16Tag, 2, 4>"),    # KC = 7, 3 tiles over workgroups of 2: the second one's 2nd tile absent
    (2, 96, 63, 65, 16, "conv_igemm_splitk_kernel<BF16Tag, 3, 8>"),    # KC = 27; 3 tiles per workgroup > n_tiles = 1: clamped weight tile,
]                                                                      # skipped epilogue items


@pytest.mark.parametrize("alias", [False, True], ids=["fresh", "alias"])
@pytest.mark.parametrize("case", A2_CASES, ids=_id)
def test_igemm_splitk_missing_forms(lib, case, alias):
    B, Cin, H, W, Cout, expect = case
    dtype = CP_BF16
    key = "a2%s" % (case[:5],)
    x = rnd(det_tensor(key + "x", (B, Cin, H, W)), dtype)
    w = rnd(det_tensor(key + "w", (Cout, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5 * 1.7), dtype)
    scale, shift = affine(key, Cout, not alias)
    res = rnd(det_tensor(key + "r", (B, Cout, H, W)), dtype) if alias else None
    act = ACT_NONE if alias else ACT_RELU
    ref = epilogue64(conv64(x, w, 1, 1), scale, shift, res, act)
    xin = to_cl(x, dtype)
    pw = pack(lib, dtype, w, xin.shape[-1], 3, 3)
    cp = rup(Cout, 8)
    out = slab(res, dtype) if alias else fresh(B, H, W, cp, dtype)
    before = out.clone()
    sym = launch(lib, lib.cp_conv2d_igemm, dtype, xin, xin.shape[-1], 0, pw, vec(Cout, scale), vec(Cout, shift), (3, 3, 1, 1), (H, W),
                 cp, out, ostr_of(out), out if alias else None, act, 0)
    assert sym == expect
    verify("A2", sym, dtype, out, before, 0, Cout, ref)


# ------------------------------------------------------------------------------------------------ A3: MT = 2, LDS epilogue off by alignment
def test_igemm_mt2_vector_epilogue_by_alignment(lib):
    """bf16, NT = 2: the LDS-transposed epilogue needs 16-byte row pieces (o_base % 8 == 0); o_base = 4 is legal (host check: % 4) and
    must take the MFMA-layout vector epilogue, 8-byte stores into a wider sentinel-filled buffer.  KC = 5: no split-K."""
    dtype, B, Cin, H, W, Cout, coff, extra = CP_BF16, 1, 16, 13, 21, 32, 4, 12
    x = rnd(det_tensor("a3x", (B, Cin, H, W)), dtype)
    w = rnd(det_tensor("a3w", (Cout, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5 * 1.7), dtype)
    scale, shift = affine("a3", Cout, True)
    res = rnd(det_tensor("a3r", (B, Cout, H, W)), dtype)
    ref = epilogue64(conv64(x, w, 1, 1), scale, shift, res, ACT_RELU)
    xin = to_cl(x, dtype)
    pw = pack(lib, dtype, w, xin.shape[-1], 3, 3)
    out = fresh(B, H, W, coff + Cout + extra, dtype)
    before = out.clone()
    sym = launch(lib, lib.cp_conv2d_igemm, dtype, xin, xin.shape[-1], 0, pw, vec(Cout, scale), vec(Cout, shift), (3, 3, 1, 1), (H, W),
                 Cout, out, ostr_of(out, coff), slab(res, dtype, coff, extra), ACT_RELU, 0)
    assert sym == "conv_igemm_kernel<BF16Tag, 2, 2>"
    verify("A3", sym, dtype, out, before, coff, Cout, ref)


# ------------------------------------------------------------------------------------------------ B: data-gradient launches
# TrainProgram._dgrad / conv_backward_group: g (the output gradient) convolved with cp_weight_dgrad(w), scale 1, shift 0, no
# activation, residual = out = gx (accumulate in place).  g is a channel slice of a wider NaN-filled buffer; gx holds g0 before.
# (name, kernel, B, Cin, Cout, H, W, k, pad, {dtype: [(ksplit, expected symbol)]}) of the FORWARD layer Cin -> Cout on an H x W map
B_S1_CASES = [
    ("3x3 18->36", "halo", 2, 18, 36, 13, 21, 3, 1,                                        # dgrad Cout' = 18: the small-Cout kernel
     {F32: [(0, "conv3x3_halo_s_kernel<F32Tag, 2>")], BF16: [(0, "conv3x3_halo_s_kernel<BF16Tag, 2>")]}),
    ("3x3 128->64", "halo", 2, 128, 64, 13, 21, 3, 1,                                      # Cout' = 128: the regular kernel
     {F32: [(0, "conv3x3_halo_kernel<F32Tag, true>")], BF16: [(0, "conv3x3_halo_kernel<BF16Tag, true>")]}),
    ("3x3 256->32", "halo", 3, 256, 32, 8, 16, 3, 1,                                       # Cout' = 256: the wide kernel
     {F32: [(0, "conv3x3_halo4_kernel<F32Tag, true, false, false>")], BF16: [(0, "conv3x3_halo4_kernel<BF16Tag, true, false, false>")]}),
    ("1x1 256->64", "gemm", 2, 256, 64, 13, 21, 1, 0,                                      # bottleneck conv1: Cout' = 256, K = 64
     {F32: [(0, "gemm_rows_kernel<F32Tag, true>")], BF16: [(0, "gemm_rows_kernel<BF16Tag, true>")]}),
    ("1x1 64->48", "igemm", 2, 64, 48, 5, 7, 1, 0,                                         # M = 70, K = 48: the plan does not split it
     {F32: [(0, "conv_igemm_kernel<F32Tag, 2, 4>"), (-1, "conv_igemm_kernel<F32Tag, 2, 4>")],
      BF16: [(0, "conv_igemm_kernel<BF16Tag, 2, 4>"), (-1, "conv_igemm_kernel<BF16Tag, 2, 4>")]}),
    ("2x2p1 256->64", "igemm", 2, 256, 64, 8, 12, 2, 1,                                    # patch generator: (H + 1, W + 1) -> (H, W), dgrad pad 0
     {F32: [(0, "conv_igemm_kernel<F32Tag, 2, 4>"), (-1, "conv_igemm_kernel<F32Tag, 2, 4>")],
      BF16: [(0, "conv_igemm_splitk_kernel<BF16Tag, 1, 4>"), (-1, "conv_igemm_kernel<BF16Tag, 2, 4>")]}),
]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", B_S1_CASES, ids=lambda c: c[0].replace(" ", "_"))
def test_dgrad_inplace_stride1(lib, dtype, case):
    name, kind, B, Cin, Cout, H, W, k, pad, expect = case
    E = esz(dtype)
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    w = rnd(det_tensor("b1w" + name, (Cout, Cin, k, k), (2.0 / (Cout * k * k)) ** 0.5 * 1.7), dtype)
    dy = rnd(det_tensor("b1d" + name, (B, Cout, Ho, Wo)), dtype)
    g0 = rnd(det_tensor("b1g" + name, (B, Cin, H, W)), dtype)
    ref = g0.double() + dgrad64((B, Cin, H, W), w, dy, 1, pad)
    g = slab(dy, dtype, coff=E, extra=2 * E)                       # in_coff = E > 0, in_cstride = Cphys + 3 E
    gcp = rup(Cout, E)
    wt = weight_dgrad(lib, w)                                      # (Cin, Cout, k, k): the data-gradient conv's (Cout', Cin', k, k)
    if kind == "halo":
        pw, fn = pack_halo(lib, dtype, wt, gcp), lib.cp_conv3x3_halo
    elif kind == "gemm":
        pw, fn = pack_gemm(lib, dtype, wt, gcp), lib.cp_gemm_rows
    else:
        pw, fn = pack(lib, dtype, wt, gcp, k, k), lib.cp_conv2d_igemm
    one, zero = vec(Cin, torch.ones(Cin)), vec(Cin)
    for ksplit, sym_expect in expect[dtype]:
        gx = slab(g0, dtype)
        before = gx.clone()
        sym = launch(lib, fn, dtype, g, gcp, E, pw, one, zero, (k, k, 1, k - 1 - pad), (H, W), gx.shape[-1], gx, ostr_of(gx), gx,
                     ACT_NONE, ksplit)
        assert sym == sym_expect
        verify("B", sym, dtype, gx, before, 0, Cin, ref)


@pytest.mark.parametrize("ksplit", [0, -1])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_dgrad_inplace_3x3_stride2_phases(lib, dtype, ksplit):
    """3x3 / s2 / p1 36 -> 72 on a 12 x 20 map (H != W): four transposed-phase launches over the 6 x 10 gradient that interleave
    into gx through the output strides, each with residual = gx.  gx is a channel slice of a wider sentinel buffer.  Every pixel
    is covered exactly once: g0 + dx everywhere.  (bf16, ksplit = 0: the 2 x 2-tap phase has KC = 9 and runs split-K.)"""
    B, Cin, Cout, H, W = 2, 36, 72, 12, 20
    E = esz(dtype)
    w = rnd(det_tensor("b2w", (Cout, Cin, 3, 3), (2.0 / (Cout * 9)) ** 0.5 * 1.7), dtype)
    dy = rnd(det_tensor("b2d", (B, Cout, H // 2, W // 2)), dtype)
    g0 = rnd(det_tensor("b2g", (B, Cin, H, W)), dtype)
    ref = g0.double() + dgrad64((B, Cin, H, W), w, dy, 2, 1)
    g = slab(dy, dtype, coff=E, extra=2 * E)
    gcp, cp, coff = rup(Cout, E), rup(Cin, E), 8
    gx = slab(g0, dtype, coff=coff, extra=8)
    before = gx.clone()
    cs = gx.shape[-1]
    one, zero = vec(Cin, torch.ones(Cin)), vec(Cin)
    tag = "F32Tag" if dtype == CP_F32 else "BF16Tag"
    tiled = "conv_igemm_kernel<%s, 2, 3>" % tag
    expect = [tiled, tiled, tiled, "conv_igemm_splitk_kernel<BF16Tag, 1, 4>" if (dtype == CP_BF16 and ksplit == 0) else tiled]
    syms = []
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        pw = pack(lib, dtype, w, gcp, 1 + a, 1 + b, rows=Cin, transposed=1, phase=ph)
        syms.append(launch(lib, lib.cp_conv2d_igemm, dtype, g, gcp, E, pw, one, zero, (1 + a, 1 + b, 1, 0), (H // 2, W // 2), cp, gx,
                           (coff + (a * W + b) * cs, H * W * cs, 2 * W * cs, 2 * cs, 1), gx, ACT_NONE, ksplit))
    assert syms == expect
    verify("B", " + ".join(sorted(set(syms))), dtype, gx, before, coff, Cin, ref)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_dgrad_inplace_1x1_stride2_scatter(lib, dtype):
    """1x1 / s2 64 -> 128 (ResNet shortcut) on a 9 x 13 map (odd H and W) -> 5 x 7: the data gradient goes through the output
    strides into every other pixel of gx, a channel slice of a wider sentinel buffer; the odd pixels keep the bits of g0."""
    B, Cin, Cout, H, W = 2, 64, 128, 9, 13
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    E = esz(dtype)
    w = rnd(det_tensor("b3w", (Cout, Cin, 1, 1), (2.0 / Cout) ** 0.5 * 1.7), dtype)
    dy = rnd(det_tensor("b3d", (B, Cout, Ho, Wo)), dtype)
    g0 = rnd(det_tensor("b3g", (B, Cin, H, W)), dtype)
    ref = g0.double() + dgrad64((B, Cin, H, W), w, dy, 2, 0)
    g = slab(dy, dtype, coff=E, extra=2 * E)
    gcp = rup(Cout, E)
    pw = pack(lib, dtype, weight_dgrad(lib, w), gcp, 1, 1)
    coff = 8
    one, zero = vec(Cin, torch.ones(Cin)), vec(Cin)
    expect = "conv_igemm_kernel<%s, 2, 4>" % ("F32Tag" if dtype == CP_F32 else "BF16Tag")
    for ksplit in (0, -1):
        gx = slab(g0, dtype, coff=coff, extra=8)
        before = gx.clone()
        cs = gx.shape[-1]
        sym = launch(lib, lib.cp_conv2d_igemm, dtype, g, gcp, E, pw, one, zero, (1, 1, 1, 0), (Ho, Wo), rup(Cin, E), gx,
                     (coff, H * W * cs, 2 * W * cs, 2 * cs, 1), gx, ACT_NONE, ksplit)
        assert sym == expect
        r, r0 = gx.view(RAW[dtype]), before.view(RAW[dtype])
        assert torch.equal(r[:, 1::2], r0[:, 1::2]) and torch.equal(r[:, :, 1::2], r0[:, :, 1::2]), "odd pixels must not be touched"
        verify("B", sym, dtype, gx, before, coff, Cin, ref)


# ------------------------------------------------------------------------------------------------ C: halo forward forms
# (name, B, Cin, H, W, Cout, act, slices, {dtype: expected symbol}); slices: input = channels [E, E + Cphys) of a NaN-padded buffer,
# output (and the residual, which shares its layout) = channels [8, 8 + Cphys) of a sentinel-filled buffer (the decoder's concat layout)
C_CASES = [
    ("s1 40->12", 2, 40, 13, 21, 12, ACT_RELU, False,                       # Cout <= 16: 12 physical channels in fp32, 16 in bf16
     {F32: "conv3x3_halo_s_kernel<F32Tag, 1>", BF16: "conv3x3_halo_s_kernel<BF16Tag, 1>"}),
    ("small 40->36", 2, 40, 13, 21, 36, ACT_RELU, True,
     {F32: "conv3x3_halo_s_kernel<F32Tag, 3>", BF16: "conv3x3_halo_s_kernel<BF16Tag, 3>"}),
    ("regular 40->100", 2, 40, 13, 21, 100, ACT_LEAKY, True,                # 100 / 104 physical channels: partial last 32-channel group
     {F32: "conv3x3_halo_kernel<F32Tag, true>", BF16: "conv3x3_halo_kernel<BF16Tag, true>"}),
    ("wide 24->256", 2, 24, 8, 16, 256, ACT_RELU, True,
     {F32: "conv3x3_halo4_kernel<F32Tag, true, false, false>", BF16: "conv3x3_halo4_kernel<BF16Tag, true, false, false>"}),
]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", C_CASES, ids=lambda c: c[0].replace(" ", "_"))
def test_halo_forward_forms(lib, dtype, case):
    name, B, Cin, H, W, Cout, act, sliced, expect = case
    E = esz(dtype)
    x = rnd(det_tensor("c_x" + name, (B, Cin, H, W)), dtype)
    w = rnd(det_tensor("c_w" + name, (Cout, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5 * 1.7), dtype)
    scale, shift = affine("c_" + name, Cout, True)
    res = rnd(det_tensor("c_r" + name, (B, Cout, H, W)), dtype)
    ref = epilogue64(conv64(x, w, 1, 1), scale, shift, res, act)
    icoff, iextra, coff, extra = (E, 2 * E, 8, 16) if sliced else (0, 0, 0, 0)
    xin = slab(x, dtype, icoff, iextra)
    cip, cp = rup(Cin, E), rup(Cout, E)
    pw = pack_halo(lib, dtype, w, cip)
    out = fresh(B, H, W, coff + cp + extra, dtype)
    before = out.clone()
    sym = launch(lib, lib.cp_conv3x3_halo, dtype, xin, cip, icoff, pw, vec(Cout, scale), vec(Cout, shift), (3, 3, 1, 1), (H, W), cp, out,
                 ostr_of(out, coff), slab(res, dtype, coff, extra), act, 0)
    assert sym == expect[dtype]
    verify("C", sym, dtype, out, before, coff, Cout, ref)
