"""GPU (-m gpu): parity of the HIP path, called through the C ABI, against the CPU oracle and the committed
golden vectors.  Tolerances (written here, per SURVEY.md §8c / BASELINE.json north_star):
  fp32 path : |logit - oracle| <= 1e-4 absolute on logits of O(1..5); per-op 2e-5 * (1 + |ref|); ids bit-exact
  bf16 path : not a 1e-4 path (bf16 has 8 mantissa bits): per-op 3e-2 * (1 + |ref|), end-to-end bit agreement >= 97 %
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from checkerpose_amd import _abi
from checkerpose_amd._abi import ACT_LEAKY, ACT_NONE, ACT_RELU, CP_BF16, CP_F32, CpConvDesc
from oracle import checkerpose_oracle as O
from tests import free_running as FR
from tests.common import (ape_p3d, build_net, det_image, det_tensor, golden, inject_feats, lm_p3d, oracle_kwargs)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DT = {CP_F32: torch.float32, CP_BF16: torch.bfloat16}
TOL = {CP_F32: 2e-5, CP_BF16: 3e-2}


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def rup(x, m):
    return (x + m - 1) // m * m


def to_cl(x, dtype, cphys=None):
    """NCHW fp32 CPU -> channels-last (B,H,W,Cphys) `dtype` on the GPU, zero padded."""
    B, Cc, H, W = x.shape
    E = 8 if dtype == CP_BF16 else 4
    cp = cphys or rup(Cc, E)
    out = torch.zeros(B, H, W, cp, dtype=DT[dtype])
    out[..., :Cc] = x.permute(0, 2, 3, 1).to(DT[dtype])
    return out.to(dev()).contiguous()


def from_cl(t, Cc):
    return t[..., :Cc].float().cpu().permute(0, 3, 1, 2).contiguous()


def rnd(x, dtype):
    """round the reference INPUT the way the device sees it (bf16 inputs are rounded once)"""
    return x.to(DT[dtype]).float()


def close(a, b, tol):
    a, b = a.double(), b.double()
    err = ((a - b).abs() / (1 + b.abs())).max().item()
    assert err <= tol, "max rel err %.3e > %.1e" % (err, tol)


def st():
    return torch.cuda.current_stream().cuda_stream


def pack(lib, dtype, w, cin_phys, R, S, rows=None, transposed=0, phase=0):
    Cout, Cin = (w.shape[1], w.shape[0]) if transposed else (w.shape[0], w.shape[1])
    rows = rows or Cout
    buf = torch.empty(lib.cp_packed_weight_bytes(dtype, rows, cin_phys, R, S), dtype=torch.uint8, device=dev())
    wd = w.contiguous().to(dev())
    _abi.check(lib.cp_pack_conv_weight(st(), dtype, wd.data_ptr(), Cout, Cin, R, S, cin_phys, transposed, phase, None, rows,
                                       buf.data_ptr()))
    torch.cuda.synchronize()
    return buf


def run_conv(lib, dtype, x, w, scale, shift, stride, pad, act=ACT_NONE, slope=0.0, residual=None, ksplit=0):
    """x NCHW fp32 (CPU), w (Cout,Cin,R,S).  Returns NCHW fp32 (CPU) from the channels-last HIP conv."""
    B, Cin, H, W = x.shape
    Cout, _, R, S = w.shape
    E = 8 if dtype == CP_BF16 else 4
    xin = to_cl(x, dtype)
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    cop = rup(Cout, E)
    out = torch.full((B, Ho, Wo, cop), float("nan"), dtype=DT[dtype], device=dev())
    pw = pack(lib, dtype, w, xin.shape[-1], R, S)
    n16 = rup(Cout, 16)
    sc = torch.zeros(n16); sc[:Cout] = scale
    sh = torch.zeros(n16); sh[:Cout] = shift
    sc, sh = sc.to(dev()), sh.to(dev())
    res = to_cl(residual, dtype) if residual is not None else None
    d = CpConvDesc()
    d.dtype, d.out_f32, d.B, d.H, d.W = dtype, 0, B, H, W
    d.Cin, d.in_cstride, d.in_coff = xin.shape[-1], xin.shape[-1], 0
    d.R, d.S, d.stride, d.pad, d.Ho, d.Wo, d.Cout, d.act, d.slope = R, S, stride, pad, Ho, Wo, cop, act, slope
    d.o_base, d.o_sb, d.o_sy, d.o_sx, d.o_sc = 0, Ho * Wo * cop, Wo * cop, cop, 1
    d.ksplit = ksplit
    _abi.check(lib.cp_conv2d_igemm(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                   res.data_ptr() if res is not None else None, out.data_ptr()), "conv")
    torch.cuda.synchronize()
    if cop > Cout:
        assert float(out[..., Cout:].float().abs().max()) == 0.0, "padded channels must be exactly zero"
    return from_cl(out, Cout)


CONV_CASES = [  # (B, Cin, H, W, Cout, k, stride, pad, act, residual)
    (2, 3, 32, 32, 64, 3, 2, 1, ACT_RELU, False),      # stem: 3 input channels padded to 4 / 8
    (1, 64, 16, 16, 64, 3, 2, 1, ACT_RELU, False),
    (2, 18, 16, 16, 18, 3, 1, 1, ACT_RELU, True),      # HRNet basic block, ragged channels + residual
    (1, 36, 9, 11, 72, 3, 2, 1, ACT_NONE, False),      # odd spatial sizes
    (1, 144, 8, 8, 18, 1, 1, 0, ACT_NONE, False),      # fuse 1x1
    (1, 256, 8, 8, 256, 3, 1, 1, ACT_RELU, False),     # decoder 3x3
    (2, 256, 16, 16, 64, 2, 1, 1, ACT_NONE, False),    # patch_generator k=2 pad=1 -> (H+1, W+1)
    (3, 64, 1, 100, 128, 1, 1, 0, ACT_LEAKY, False),   # linear over keypoints, M not a tile multiple
    (1, 16, 40, 40, 10, 7, 2, 3, ACT_RELU, False),     # 7x7 stride 2 (resnet stem shape class)
    (1, 144, 8, 8, 144, 3, 1, 1, ACT_RELU, True),      # B = 1 HRNet 8x8 branch: 41 K chunks over 8 waves (split-K), residual
    (3, 72, 16, 16, 72, 3, 1, 1, ACT_RELU, False),     # 21 chunks over 4 waves, ragged channel tiles (72 = 4.5 tiles)
    (1, 72, 16, 16, 144, 3, 2, 1, ACT_NONE, False),    # stride-2 fuse conv, 64 output pixels
    (2, 320, 1, 77, 256, 1, 1, 0, ACT_LEAKY, False),   # refinement MLP rows at small batch: K = 320, M = 154 (ragged pixel tile)
    (32, 144, 8, 8, 144, 3, 1, 1, ACT_RELU, True),     # B = 32: 3 channel tiles per workgroup (64 x 3 workgroups), 8 waves
    (16, 72, 16, 16, 72, 3, 1, 1, ACT_RELU, False),    # 2 channel tiles per workgroup (5 tiles: one workgroup's second tile absent), 4 waves
]


@pytest.mark.parametrize("ksplit", [0, -1])
@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_igemm_vs_torch_cpu(lib, dtype, case, ksplit):
    """ksplit = 0: the library picks the split-K variant where its plan says so (bf16, long K, small grid: most of these
    shapes); -1: always the tiled kernel (for fp32 and short-K shapes both settings run the same kernel)."""
    B, Cin, H, W, Cout, k, stride, pad, act, has_res = case
    x = det_tensor("cx%s" % (case,), (B, Cin, H, W))
    w = det_tensor("cw%s" % (case,), (Cout, Cin, k, k), (2.0 / (Cin * k * k)) ** 0.5 * 1.7)
    scale = 1.0 + 0.3 * det_tensor("cs%s" % (case,), (Cout,))
    shift = 0.2 * det_tensor("ct%s" % (case,), (Cout,))
    ref = F.conv2d(rnd(x, dtype), rnd(w, dtype), None, stride, pad) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    res = None
    if has_res:
        res = det_tensor("cr%s" % (case,), tuple(ref.shape))
        ref = ref + rnd(res, dtype)
    ref = F.relu(ref) if act == ACT_RELU else (F.leaky_relu(ref, 0.01) if act == ACT_LEAKY else ref)
    got = run_conv(lib, dtype, x, w, scale, shift, stride, pad, act, 0.01, res, ksplit)
    close(got, ref, TOL[dtype])


HALO_CASES = [  # (B, Cin, H, W, Cout, act, residual)
    (2, 64, 16, 32, 64, ACT_RELU, False),      # exact tiles, Cin = 2..4 chunks, Cout = 2 groups
    (1, 256, 16, 16, 256, ACT_RELU, False),    # decoder shape class: 2 channel blocks of 128
    (2, 18, 24, 40, 18, ACT_RELU, True),       # HRNet branch 0: ragged Cin/Cout (18 -> 20/24), partial chunk, residual
    (1, 36, 13, 21, 72, ACT_NONE, False),      # H, W not tile multiples (masked stores, zero halo)
    (3, 144, 8, 16, 40, ACT_LEAKY, True),      # single tile row, Cout = 40 (second half of a lane's 8 channels absent)
    (1, 512, 8, 16, 32, ACT_RELU, False),      # deep K (16/32 chunks), odd/even chunk counts
    (2, 64, 24, 40, 256, ACT_RELU, True),      # wide (Cout % 256 == 0) kernel: ragged tile rows / cols, residual, 2..4 chunks
    (1, 40, 17, 16, 512, ACT_LEAKY, False),    # ... two 256-channel blocks, partial chunk
    (3, 256, 32, 32, 256, ACT_RELU, False),    # ... decoder shape class
]


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", HALO_CASES)
def test_conv3x3_halo_vs_torch_cpu(lib, dtype, case):
    """LDS-halo 3x3/s1/p1 kernel (cp_conv3x3_halo) == torch CPU conv + affine + residual + act."""
    B, Cin, H, W, Cout, act, has_res = case
    x = det_tensor("hx%s" % (case,), (B, Cin, H, W))
    w = det_tensor("hw%s" % (case,), (Cout, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5 * 1.7)
    scale = 1.0 + 0.3 * det_tensor("hs%s" % (case,), (Cout,))
    shift = 0.2 * det_tensor("ht%s" % (case,), (Cout,))
    ref = F.conv2d(rnd(x, dtype), rnd(w, dtype), None, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    res = None
    if has_res:
        res = det_tensor("hr%s" % (case,), tuple(ref.shape))
        ref = ref + rnd(res, dtype)
    ref = F.relu(ref) if act == ACT_RELU else (F.leaky_relu(ref, 0.01) if act == ACT_LEAKY else ref)
    E = 8 if dtype == CP_BF16 else 4
    xin = to_cl(x, dtype)
    cop = rup(Cout, E)
    out = torch.full((B, H, W, cop), float("nan"), dtype=DT[dtype], device=dev())
    pw = torch.empty(lib.cp_packed_halo_weight_bytes(dtype, Cout, xin.shape[-1]), dtype=torch.uint8, device=dev())
    wd = w.contiguous().to(dev())
    _abi.check(lib.cp_pack_conv3x3_halo_weight(st(), dtype, wd.data_ptr(), Cout, Cin, xin.shape[-1], pw.data_ptr()))
    n16 = rup(Cout, 16)
    sc = torch.zeros(n16); sc[:Cout] = scale
    sh = torch.zeros(n16); sh[:Cout] = shift
    sc, sh = sc.to(dev()), sh.to(dev())
    rs = to_cl(res, dtype) if res is not None else None
    d = CpConvDesc()
    d.dtype, d.out_f32, d.B, d.H, d.W = dtype, 0, B, H, W
    d.Cin, d.in_cstride, d.in_coff = xin.shape[-1], xin.shape[-1], 0
    d.R, d.S, d.stride, d.pad, d.Ho, d.Wo, d.Cout, d.act, d.slope = 3, 3, 1, 1, H, W, cop, act, 0.01
    d.o_base, d.o_sb, d.o_sy, d.o_sx, d.o_sc = 0, H * W * cop, W * cop, cop, 1
    _abi.check(lib.cp_conv3x3_halo(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                   rs.data_ptr() if rs is not None else None, out.data_ptr()), "halo conv")
    torch.cuda.synchronize()
    if cop > Cout:
        assert float(out[..., Cout:].float().abs().max()) == 0.0, "padded channels must be exactly zero"
    close(from_cl(out, Cout), ref, TOL[dtype])
    d.stride = 2                                        # unsupported shape -> loud error, no silent fallback
    assert lib.cp_conv3x3_halo(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(), None, out.data_ptr()) == -1


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", [(2, 256, 16, 16, 64, ACT_NONE), (1, 64, 13, 21, 64, ACT_RELU), (3, 40, 32, 32, 24, ACT_LEAKY), (1, 256, 64, 64, 64, ACT_NONE)])
def test_conv2x2_halo_vs_torch_cpu(lib, dtype, case):
    """cp_conv2x2_halo (k = 2 / stride 1 / pad 1 on the LDS-staged halo tile: Index2Feat_module.patch_generator, pipeline.py:144-145,156)
    == F.conv2d(x, w, padding=1) * scale + shift (+ act): the (H + 1) x (W + 1) output incl. its last row / column (which see only
    zero padding below / right), ragged tiles, a channel count that is not a multiple of the chunk, pad channels zero."""
    B, Cin, H, W, Cout, act = case
    E = 8 if dtype == CP_BF16 else 4
    x = det_tensor("c2x%s" % (case[:5],), (B, Cin, H, W))
    w = det_tensor("c2w%s" % (case[:5],), (Cout, Cin, 2, 2), (2.0 / (Cin * 4)) ** 0.5 * 1.7)
    scale = 1.0 + 0.3 * det_tensor("c2s%s" % (case[:5],), (Cout,))
    shift = 0.2 * det_tensor("c2t%s" % (case[:5],), (Cout,))
    ref = F.conv2d(rnd(x, dtype), rnd(w, dtype), None, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    ref = F.relu(ref) if act == ACT_RELU else (F.leaky_relu(ref, 0.2) if act == ACT_LEAKY else ref)
    xin = to_cl(x, dtype)
    cip, cop = xin.shape[-1], rup(Cout, E)
    assert lib.cp_conv2x2_halo_supported(dtype, H, W, cop) == 1 and lib.cp_conv2x2_halo_supported(dtype, H, W, 96) == 0
    pw = torch.empty(lib.cp_packed_conv2x2_halo_weight_bytes(dtype, Cout, cip), dtype=torch.uint8, device=dev())
    wd = w.contiguous().to(dev())
    _abi.check(lib.cp_pack_conv2x2_halo_weight(st(), dtype, wd.data_ptr(), Cout, Cin, cip, pw.data_ptr()), "pack 2x2")
    n16 = rup(Cout, 16)
    sc = torch.zeros(n16); sc[:Cout] = scale
    sh = torch.zeros(n16); sh[:Cout] = shift
    sc, sh = sc.to(dev()), sh.to(dev())
    Ho, Wo = H + 1, W + 1
    d = CpConvDesc()
    d.dtype, d.out_f32, d.B, d.H, d.W = dtype, 0, B, H, W
    d.Cin, d.in_cstride, d.in_coff = cip, cip, 0
    d.R, d.S, d.stride, d.pad, d.Ho, d.Wo, d.Cout, d.act, d.slope = 2, 2, 1, 1, Ho, Wo, cop, act, 0.2
    d.o_base, d.o_sb, d.o_sy, d.o_sx, d.o_sc = 0, Ho * Wo * cop, Wo * cop, cop, 1
    out = torch.full((B, Ho, Wo, cop), float("nan"), dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_conv2x2_halo(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(), None, out.data_ptr()), "conv 2x2")
    torch.cuda.synchronize()
    assert not torch.isnan(out.float()).any(), "every output element must be written"
    if cop > Cout:
        assert float(out[..., Cout:].float().abs().max()) == 0.0, "padded channels must be exactly zero"
    close(from_cl(out, Cout), ref, TOL[dtype])
    d.Ho = H                                              # wrong output extent -> loud error
    assert lib.cp_conv2x2_halo(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(), None, out.data_ptr()) == -1


SEG_CASES = [  # (B, Cin, H, W, S)
    (2, 256, 16, 32, 2),     # exact tiles
    (1, 64, 13, 21, 2),      # ragged tile rows / cols (masked stores, lanes past the image still shuffle)
    (3, 40, 8, 16, 1),       # one head output, partial K chunk
]


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", SEG_CASES)
def test_conv3x3_halo_seg_vs_torch_cpu(lib, dtype, case):
    """cp_conv3x3_halo_seg: relu(bn(conv3x3(x))) as cp_conv3x3_halo writes it, AND the 1x1 head (seg_block, pipeline.py:349,383)
    on the STORED activations in the same launch: both against torch CPU; the feature map bit-identical to the plain kernel."""
    B, Cin, H, W, S = case
    Cout = 256
    x = det_tensor("sgx%s" % (case,), (B, Cin, H, W))
    w = det_tensor("sgw%s" % (case,), (Cout, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5 * 1.7)
    scale = 1.0 + 0.3 * det_tensor("sgs%s" % (case,), (Cout,))
    shift = 0.2 * det_tensor("sgt%s" % (case,), (Cout,))
    wseg = det_tensor("sgh%s" % (case,), (S, Cout), 0.1)
    bseg = det_tensor("sgb%s" % (case,), (S,), 0.5)
    feat = F.relu(F.conv2d(rnd(x, dtype), rnd(w, dtype), None, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    xin = to_cl(x, dtype)
    out = torch.full((B, H, W, Cout), float("nan"), dtype=DT[dtype], device=dev())
    out2 = torch.full((B, H, W, Cout), float("nan"), dtype=DT[dtype], device=dev())
    seg = torch.full((B, S, H, W), float("nan"), dtype=torch.float32, device=dev())
    pw = torch.empty(lib.cp_packed_halo_weight_bytes(dtype, Cout, xin.shape[-1]), dtype=torch.uint8, device=dev())
    wd = w.contiguous().to(dev())
    _abi.check(lib.cp_pack_conv3x3_halo_weight(st(), dtype, wd.data_ptr(), Cout, Cin, xin.shape[-1], pw.data_ptr()))
    sc, sh = scale.to(dev()), shift.to(dev())
    sw, sb = rnd(wseg, dtype).contiguous().to(dev()), bseg.to(dev())
    d = CpConvDesc()
    d.dtype, d.out_f32, d.B, d.H, d.W = dtype, 0, B, H, W
    d.Cin, d.in_cstride, d.in_coff = xin.shape[-1], xin.shape[-1], 0
    d.R, d.S, d.stride, d.pad, d.Ho, d.Wo, d.Cout, d.act, d.slope = 3, 3, 1, 1, H, W, Cout, ACT_RELU, 0.0
    d.o_base, d.o_sb, d.o_sy, d.o_sx, d.o_sc = 0, H * W * Cout, W * Cout, Cout, 1
    assert lib.cp_conv3x3_halo_seg_supported(dtype, Cout, S) == 1 and lib.cp_conv3x3_halo_seg_supported(dtype, 512, S) == 0
    _abi.check(lib.cp_conv3x3_halo_seg(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr(),
                                       sw.data_ptr(), sb.data_ptr(), S, seg.data_ptr()), "halo_seg")
    _abi.check(lib.cp_conv3x3_halo(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(), None, out2.data_ptr()), "halo")
    torch.cuda.synchronize()
    assert torch.equal(out, out2)                                           # same main loop, same stores
    close(from_cl(out, Cout), feat, TOL[dtype])
    stored = out.float().cpu().permute(0, 3, 1, 2)                          # the head reads what was stored
    ref = F.conv2d(stored, rnd(wseg, dtype).view(S, Cout, 1, 1), bseg)
    assert float((seg.cpu() - ref).abs().max()) <= 2e-4 * max(1.0, float(ref.abs().max()))


S2_CASES = [  # (B, Cin, ctot, coff, H, W, Cout, act)
    (2, 256, 256, 0, 64, 64, 36, ACT_RELU),      # HRNet transition1[1]
    (3, 64, 96, 32, 16, 32, 48, ACT_LEAKY),      # channel slice of a wider buffer, W = 32 (2 tiles per wave), 3 full M tiles
    (1, 32, 32, 0, 8, 64, 8, ACT_NONE),          # one band, one chunk, one partial M tile
]


@pytest.mark.parametrize("case", S2_CASES)
def test_conv3x3_s2_small_vs_torch_cpu(lib, case):
    """cp_conv3x3_s2_small (3x3 / stride 2 with the input chunk staged in LDS) == torch conv2d(stride 2, pad 1) + affine + act."""
    B, Cin, ctot, coff, H, W, Cout, act = case
    dtype = CP_BF16
    xall = det_tensor("s2x%s" % (case,), (B, ctot, H, W))
    w = det_tensor("s2w%s" % (case,), (Cout, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5 * 1.7)
    scale = 1.0 + 0.3 * det_tensor("s2s%s" % (case,), (Cout,))
    shift = 0.2 * det_tensor("s2t%s" % (case,), (Cout,))
    ref = F.conv2d(rnd(xall[:, coff:coff + Cin], dtype), rnd(w, dtype), None, 2, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    ref = F.relu(ref) if act == ACT_RELU else (F.leaky_relu(ref, 0.01) if act == ACT_LEAKY else ref)
    xin = to_cl(xall, dtype)
    ocp = rup(Cout, 8)
    assert lib.cp_conv3x3_s2_small_supported(H, W, Cin, ocp) == 1
    pw = torch.empty(lib.cp_conv3x3_s2_small_weight_bytes(Cin, ocp), dtype=torch.uint8, device=dev())
    wd = w.contiguous().to(dev())
    _abi.check(lib.cp_pack_conv3x3_s2_small_weight(st(), wd.data_ptr(), Cout, Cin, Cin, ocp, pw.data_ptr()))
    n16 = rup(Cout, 16)
    sc = torch.zeros(n16); sc[:Cout] = scale
    sh = torch.zeros(n16); sh[:Cout] = shift
    sc, sh = sc.to(dev()), sh.to(dev())
    Ho, Wo = H // 2, W // 2
    out = torch.full((B, Ho, Wo, ocp), float("nan"), dtype=DT[dtype], device=dev())
    d = CpConvDesc()
    d.dtype, d.out_f32, d.B, d.H, d.W = dtype, 0, B, H, W
    d.Cin, d.in_cstride, d.in_coff = Cin, ctot, coff
    d.R, d.S, d.stride, d.pad, d.Ho, d.Wo, d.Cout, d.act, d.slope = 3, 3, 2, 1, Ho, Wo, ocp, act, 0.01
    d.o_base, d.o_sb, d.o_sy, d.o_sx, d.o_sc = 0, Ho * Wo * ocp, Wo * ocp, ocp, 1
    _abi.check(lib.cp_conv3x3_s2_small(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr()), "s2 conv")
    torch.cuda.synchronize()
    assert not torch.isnan(out.float()).any()
    if ocp > Cout:
        assert float(out[..., Cout:].float().abs().max()) == 0.0, "padded channels must be exactly zero"
    close(from_cl(out, Cout), ref, TOL[dtype])
    d.stride = 1                                        # not this kernel's shape -> loud error
    assert lib.cp_conv3x3_s2_small(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr()) == -1
    assert lib.cp_conv3x3_s2_small_supported(H, 48, Cin, ocp) == 0 and lib.cp_conv3x3_s2_small_supported(H, W, Cin, 56) == 0


UP_CASES = [  # (B, Cin, cin_total, coff, Hs, Ws, Cout, act): low-resolution source (Hs, Ws), conv at (2 Hs, 2 Ws)
    (2, 64, 64, 0, 16, 16, 256, ACT_RELU),       # exact tiles
    (1, 96, 160, 64, 12, 20, 256, ACT_RELU),     # channel slice of a wider buffer, tile rows / cols ragged (24 x 40)
    (2, 40, 40, 0, 4, 8, 512, ACT_LEAKY),        # one tile per crop, two 256-channel blocks, partial chunk
    (1, 256, 256, 0, 32, 32, 256, ACT_RELU),     # decoder shape class (many tiles per crop, interior tiles)
    (1, 32, 32, 0, 5, 9, 256, ACT_NONE),         # odd source size
    (1, 32, 32, 0, 130, 3, 256, ACT_NONE),       # more than 128 source rows: the exact source coordinate of cp_up_coord
]


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", UP_CASES)
def test_conv3x3_halo_up2x_bit_identical_to_unfused(lib, dtype, case):
    """cp_conv3x3_halo_up2x (bilinear x2 interpolated inside the conv's halo loader, pipeline.py:199-200) gives the SAME BITS as
    cp_upsample2x_bilinear_ac followed by cp_conv3x3_halo, and both match torch (interpolate align_corners + conv)."""
    B, Cin, ctot, coff, Hs, Ws, Cout, act = case
    H, W = 2 * Hs, 2 * Ws
    xall = det_tensor("ux%s" % (case,), (B, ctot, Hs, Ws))
    w = det_tensor("uw%s" % (case,), (Cout, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5 * 1.7)
    scale = 1.0 + 0.3 * det_tensor("us%s" % (case,), (Cout,))
    shift = 0.2 * det_tensor("ut%s" % (case,), (Cout,))
    xs = rnd(xall[:, coff:coff + Cin], dtype)
    up = F.interpolate(xs, scale_factor=2, mode="bilinear", align_corners=True)
    ref = F.conv2d(rnd(up, dtype), rnd(w, dtype), None, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    ref = F.relu(ref) if act == ACT_RELU else (F.leaky_relu(ref, 0.01) if act == ACT_LEAKY else ref)
    xin = to_cl(xall, dtype)                                   # (B, Hs, Ws, ctot)
    assert xin.shape[-1] == ctot
    pw = torch.empty(lib.cp_packed_halo_weight_bytes(dtype, Cout, Cin), dtype=torch.uint8, device=dev())
    wd = w.contiguous().to(dev())
    _abi.check(lib.cp_pack_conv3x3_halo_weight(st(), dtype, wd.data_ptr(), Cout, Cin, Cin, pw.data_ptr()))
    sc, sh = scale.to(dev()).contiguous(), shift.to(dev()).contiguous()
    d = CpConvDesc()
    d.dtype, d.out_f32, d.B, d.H, d.W = dtype, 0, B, H, W
    d.R, d.S, d.stride, d.pad, d.Ho, d.Wo, d.Cout, d.act, d.slope = 3, 3, 1, 1, H, W, Cout, act, 0.01
    d.o_base, d.o_sb, d.o_sy, d.o_sx, d.o_sc = 0, H * W * Cout, W * Cout, Cout, 1
    # unfused pair
    upb = torch.full((B, H, W, Cin), float("nan"), dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_upsample2x_bilinear_ac(st(), dtype, xin.data_ptr(), upb.data_ptr(), B, Hs, Ws, Cin, ctot, coff, Cin, 0))
    d.Cin, d.in_cstride, d.in_coff = Cin, Cin, 0
    out_a = torch.full((B, H, W, Cout), float("nan"), dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_conv3x3_halo(st(), C.byref(d), upb.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(), None, out_a.data_ptr()))
    # fused
    d.Cin, d.in_cstride, d.in_coff = Cin, ctot, coff
    out_b = torch.full((B, H, W, Cout), float("nan"), dtype=DT[dtype], device=dev())
    assert lib.cp_conv3x3_halo_up2x_supported(dtype, Cout) == 1
    _abi.check(lib.cp_conv3x3_halo_up2x(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(), out_b.data_ptr()),
               "fused upsample conv")
    torch.cuda.synchronize()
    assert torch.equal(out_a.view(torch.int16 if dtype == CP_BF16 else torch.int32), out_b.view(torch.int16 if dtype == CP_BF16 else torch.int32)), \
        "fused and unfused paths must agree bit for bit"
    close(from_cl(out_b, Cout), ref, TOL[dtype])
    d.H = H + 1                                                # odd upsampled size -> loud error
    assert lib.cp_conv3x3_halo_up2x(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(), out_b.data_ptr()) == -1
    assert lib.cp_conv3x3_halo_up2x_supported(dtype, 128) == 0


@pytest.mark.parametrize("dtype,Cc", [(CP_BF16, 18), (CP_BF16, 32), (CP_BF16, 8), (CP_F32, 16), (CP_F32, 10)])
@pytest.mark.parametrize("shape", [(2, 16, 32), (1, 13, 21), (3, 8, 16)])
def test_basicblock_fused_vs_torch_cpu(lib, dtype, Cc, shape):
    """Fused BasicBlock (cp_basicblock_fused) == relu(bn2(conv2(relu(bn1(conv1(x))))) + x), incl. image borders
    (the intermediate's out-of-image ring must be zero padding, not conv1 of padded x) and ragged tiles."""
    B, H, W = shape
    x = det_tensor("bx%s%d" % (shape, Cc), (B, Cc, H, W))
    w1 = det_tensor("bw1%d" % Cc, (Cc, Cc, 3, 3), (2.0 / (Cc * 9)) ** 0.5 * 1.7)
    w2 = det_tensor("bw2%d" % Cc, (Cc, Cc, 3, 3), (2.0 / (Cc * 9)) ** 0.5 * 1.7)
    s1, t1 = 1.0 + 0.3 * det_tensor("bs1%d" % Cc, (Cc,)), 0.3 * det_tensor("bt1%d" % Cc, (Cc,))
    s2, t2 = 1.0 + 0.3 * det_tensor("bs2%d" % Cc, (Cc,)), 0.3 * det_tensor("bt2%d" % Cc, (Cc,))
    xr = rnd(x, dtype)
    y1 = F.relu(F.conv2d(xr, rnd(w1, dtype), None, 1, 1) * s1.view(1, -1, 1, 1) + t1.view(1, -1, 1, 1))
    if dtype == CP_BF16:
        y1 = rnd(y1, dtype)                    # the intermediate is stored as bf16 in LDS
    ref = F.relu(F.conv2d(y1, rnd(w2, dtype), None, 1, 1) * s2.view(1, -1, 1, 1) + t2.view(1, -1, 1, 1) + xr)
    E = 8 if dtype == CP_BF16 else 4
    xin = to_cl(x, dtype)
    cp = xin.shape[-1]
    out = torch.full((B, H, W, cp), float("nan"), dtype=DT[dtype], device=dev())
    nb = lib.cp_packed_halo_weight_bytes(dtype, Cc, cp)
    pw1 = torch.empty(nb, dtype=torch.uint8, device=dev()); pw2 = torch.empty(nb, dtype=torch.uint8, device=dev())
    w1d, w2d = w1.contiguous().to(dev()), w2.contiguous().to(dev())
    _abi.check(lib.cp_pack_conv3x3_rows_weight(st(), dtype, w1d.data_ptr(), Cc, Cc, cp, pw1.data_ptr()))
    _abi.check(lib.cp_pack_conv3x3_halo_weight(st(), dtype, w2d.data_ptr(), Cc, Cc, cp, pw2.data_ptr()))

    def pad(v):
        o = torch.zeros(rup(Cc, 16)); o[:Cc] = v
        return o.to(dev())
    a = [pad(v) for v in (s1, t1, s2, t2)]
    d = CpConvDesc()
    d.dtype, d.out_f32, d.B, d.H, d.W = dtype, 0, B, H, W
    d.Cin, d.in_cstride, d.in_coff = cp, cp, 0
    d.R, d.S, d.stride, d.pad, d.Ho, d.Wo, d.Cout, d.act, d.slope = 3, 3, 1, 1, H, W, cp, ACT_RELU, 0.0
    d.o_base, d.o_sb, d.o_sy, d.o_sx, d.o_sc = 0, H * W * cp, W * cp, cp, 1
    _abi.check(lib.cp_basicblock_fused(st(), C.byref(d), xin.data_ptr(), pw1.data_ptr(), a[0].data_ptr(), a[1].data_ptr(),
                                       pw2.data_ptr(), a[2].data_ptr(), a[3].data_ptr(), out.data_ptr()), "fused basic block")
    torch.cuda.synchronize()
    if cp > Cc:
        assert float(out[..., Cc:].float().abs().max()) == 0.0
    close(from_cl(out, Cc), ref, 2e-5 if dtype == CP_F32 else 3e-2)
    assert lib.cp_basicblock_fused(st(), C.byref(d), xin.data_ptr(), pw1.data_ptr(), a[0].data_ptr(), a[1].data_ptr(),
                                   pw2.data_ptr(), a[2].data_ptr(), a[3].data_ptr(), xin.data_ptr()) == -1   # in-place refused


@pytest.mark.parametrize("shape", [(3, 64, 64), (2, 96, 128), (1, 256, 256)])
def test_hr_stem_fused_vs_torch_cpu(lib, shape):
    """cp_hr_stem (layout change + conv1/s2 + BN + ReLU + conv2/s2 + BN + ReLU in one launch, bf16) == torch CPU with the
    image and the 64-channel intermediate rounded to bf16; image borders (zero padding of BOTH convs), several tiles."""
    B, Hin, Win = shape
    img = det_tensor("stimg%s" % (shape,), (B, 3, Hin, Win), 1.7)
    w1 = det_tensor("stw1", (64, 3, 3, 3), (2.0 / 27) ** 0.5 * 1.7)
    w2 = det_tensor("stw2", (64, 64, 3, 3), (2.0 / 576) ** 0.5 * 1.7)
    s1, t1 = 1.0 + 0.3 * det_tensor("sts1", (64,)), 0.2 * det_tensor("stt1", (64,))
    s2, t2 = 1.0 + 0.3 * det_tensor("sts2", (64,)), 0.2 * det_tensor("stt2", (64,))
    v4 = lambda v: v.view(1, -1, 1, 1)   # noqa: E731
    y1 = rnd(F.relu(F.conv2d(rnd(img, CP_BF16), rnd(w1, CP_BF16), None, 2, 1) * v4(s1) + v4(t1)), CP_BF16)
    ref = F.relu(F.conv2d(y1, rnd(w2, CP_BF16), None, 2, 1) * v4(s2) + v4(t2))
    d = dev()
    p1 = torch.empty(lib.cp_hr_stem_weight_bytes(0), dtype=torch.uint8, device=d)
    p2 = torch.empty(lib.cp_hr_stem_weight_bytes(1), dtype=torch.uint8, device=d)
    w1d, w2d = w1.contiguous().to(d), w2.contiguous().to(d)
    _abi.check(lib.cp_pack_hr_stem_weights(st(), w1d.data_ptr(), w2d.data_ptr(), p1.data_ptr(), p2.data_ptr()))
    a = [v.contiguous().to(d) for v in (s1, t1, s2, t2)]
    imgd = img.contiguous().to(d)
    out = torch.full((B, Hin // 4, Win // 4, 64), float("nan"), dtype=torch.bfloat16, device=d)
    _abi.check(lib.cp_hr_stem(st(), imgd.data_ptr(), B, Hin, Win, p1.data_ptr(), a[0].data_ptr(), a[1].data_ptr(), p2.data_ptr(),
                              a[2].data_ptr(), a[3].data_ptr(), out.data_ptr()), "hr stem")
    torch.cuda.synchronize()
    close(from_cl(out, 64), ref, 3e-2)
    assert lib.cp_hr_stem(st(), imgd.data_ptr(), B, Hin + 8, Win, p1.data_ptr(), a[0].data_ptr(), a[1].data_ptr(), p2.data_ptr(),
                          a[2].data_ptr(), a[3].data_ptr(), out.data_ptr()) == -1                 # not a whole number of tiles


FUSE_OUT_CASES = [  # (B, C, H, W, [(Cout, k, relu), ...]): the convs of an HRNet-W18 stage-4 fuse layer, by source branch
    (3, 18, 64, 64, [(36, 3, False), (18, 3, True), (18, 3, True)]),       # 4 bands per crop
    (2, 36, 32, 32, [(18, 1, False), (72, 3, False), (36, 3, True)]),      # 2 bands
    (2, 72, 16, 16, [(18, 1, False), (36, 1, False), (144, 3, False)]),    # output rows of 8 pixels: a 16-pixel tile spans 2 rows
    (3, 144, 8, 8, [(18, 1, False), (36, 1, False), (72, 1, False)]),      # 1x1 only, 18 channel groups
    (1, 18, 64, 64, [(36, 3, False)]),                                     # stage 2: one conv per source
    (2, 40, 12, 20, [(24, 3, True), (50, 1, True), (7, 3, False), (16, 1, False)]),   # odd sizes: ragged tiles, 4 convs, Cout 7 / 50
]


@pytest.mark.parametrize("case", FUSE_OUT_CASES)
def test_hr_fuse_out_vs_torch_cpu(lib, case):
    """cp_hr_fuse_out (every first-level fuse conv of one source branch in one launch) == the per-conv torch reference."""
    from checkerpose_amd._abi import CpFuseConv
    B, Cc, H, W, convs = case
    dtype = CP_BF16
    x = det_tensor("fo_x%s" % (case[:4],), (B, Cc, H, W))
    xin = to_cl(x, dtype)
    cp = xin.shape[-1]
    assert lib.cp_hr_fuse_out_supported(H, W, cp) == 1
    arr = (CpFuseConv * len(convs))()
    keep, outs, refs = [], [], []
    for i, (Cout, k, relu) in enumerate(convs):
        w = det_tensor("fo_w%d%s" % (i, case[:4]), (Cout, Cc, k, k), (2.0 / (Cc * k * k)) ** 0.5 * 1.7)
        scale = 1.0 + 0.3 * det_tensor("fo_s%d%s" % (i, case[:4]), (Cout,))
        shift = 0.2 * det_tensor("fo_t%d%s" % (i, case[:4]), (Cout,))
        r = F.conv2d(rnd(x, dtype), rnd(w, dtype), None, 2 if k == 3 else 1, 1 if k == 3 else 0)
        r = r * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        refs.append(F.relu(r) if relu else r)
        kind = 1 if k == 3 else 0
        ocp = rup(Cout, 8)
        pw = torch.empty(lib.cp_hr_fuse_out_weight_bytes(cp, ocp, kind), dtype=torch.uint8, device=dev())
        wd = w.contiguous().to(dev())
        _abi.check(lib.cp_pack_hr_fuse_out_weight(st(), wd.data_ptr(), Cout, Cc, cp, ocp, kind, pw.data_ptr()))
        n = lib.cp_hr_fuse_out_affine_floats(ocp)
        aff = torch.zeros(2, n)
        aff[0, :Cout] = scale
        aff[1, :Cout] = shift
        aff = aff.to(dev())
        out = torch.full((B, H >> kind, W >> kind, ocp), float("nan"), dtype=DT[dtype], device=dev())
        arr[i].packed_w, arr[i].affine, arr[i].out = pw.data_ptr(), aff.data_ptr(), out.data_ptr()
        arr[i].kind, arr[i].Cout, arr[i].out_cphys, arr[i].relu = kind, Cout, ocp, 1 if relu else 0
        keep += [pw, aff, wd]
        outs.append(out)
    _abi.check(lib.cp_hr_fuse_out(st(), xin.data_ptr(), B, H, W, cp, len(convs), arr), "cp_hr_fuse_out")
    torch.cuda.synchronize()
    for (Cout, k, relu), out, ref in zip(convs, outs, refs):
        assert not torch.isnan(out.float()).any(), "every output element must be written"
        if out.shape[-1] > Cout:
            assert float(out[..., Cout:].float().abs().max()) == 0.0, "padded channels must be exactly zero"
        close(from_cl(out, Cout), ref, TOL[dtype])
    assert lib.cp_hr_fuse_out(st(), xin.data_ptr(), B, H + 1, W, cp, len(convs), arr) == -1       # odd size: loud error
    assert lib.cp_hr_fuse_out(st(), xin.data_ptr(), B, H, W, cp, 5, arr) == -1                    # more than 4 convs


@pytest.mark.parametrize("nsrc", [1, 3])
@pytest.mark.parametrize("cfg", [(36, 32, 32, 3), (72, 16, 16, 5), (144, 8, 8, 3), (36, 32, 32, 1), (18, 64, 64, 3),
                                 (72, 16, 16, 193), (144, 8, 8, 99), (144, 8, 8, 195)])      # crops per workgroup by batch: 2 | 2 | 4, ragged last group
def test_hr_branch_chain_vs_torch_cpu(lib, cfg, nsrc):
    """cp_hr_branch_chain (one launch, map resident in LDS, K packed across taps) == the previous module's fuse sum
    (nearest-upsampled terms, ReLU) followed by the 4 BasicBlocks of an HRNet branch, every stored tensor rounded to bf16
    (timm HighResolutionModule.branches[j], restated oracle _hr_module).  Odd batches (two crops per workgroup on the
    72/144-channel branches), pad channels exactly zero, in-place refused.  The low-resolution chains pack 1 crop per workgroup below 96
    crops (144 channels: 2 from 96, 4 from 192; 72 channels: 2 from 192 -- hr_chain.hip CHAIN_CPW_FULL_B): the last three cases run the
    packed forms with a ragged last group."""
    Cc, H, W, B = cfg
    assert lib.cp_hr_chain_supported(Cc, H, W) == 1 and lib.cp_hr_chain_supported(18, 32, 32) == 0
    dtype = CP_BF16
    v4 = lambda v: v.view(1, -1, 1, 1)   # noqa: E731
    terms = [det_tensor("ct0%d" % Cc, (B, Cc, H, W))]
    shifts = [0]
    if nsrc == 3:
        terms += [det_tensor("ct1%d" % Cc, (B, Cc, H // 2, W // 2)), det_tensor("ct2%d" % Cc, (B, Cc, H, W), 0.5)]
        shifts += [1, 0]
    x = None
    for t, sh in zip(terms, shifts):
        u = rnd(t, dtype)
        if sh:
            u = F.interpolate(u, scale_factor=2 ** sh, mode="nearest")
        x = u if x is None else x + u
    x = rnd(F.relu(x) if nsrc > 1 else x, dtype)
    ws = [det_tensor("cw%d_%d" % (i, Cc), (Cc, Cc, 3, 3), (2.0 / (Cc * 9)) ** 0.5 * 1.5) for i in range(8)]
    affs = [(1.0 + 0.3 * det_tensor("cs%d_%d" % (i, Cc), (Cc,)), 0.2 * det_tensor("cb%d_%d" % (i, Cc), (Cc,))) for i in range(8)]
    for i in range(1, 8, 2):
        affs[i] = (affs[i][0] * 0.4, affs[i][1])               # damp the residual branch like a trained net's last BN
    for k in range(4):
        t = rnd(F.relu(F.conv2d(x, rnd(ws[2 * k], dtype), None, 1, 1) * v4(affs[2 * k][0]) + v4(affs[2 * k][1])), dtype)
        x = rnd(F.relu(F.conv2d(t, rnd(ws[2 * k + 1], dtype), None, 1, 1) * v4(affs[2 * k + 1][0]) + v4(affs[2 * k + 1][1]) + x), dtype)
    ref = x
    blob = torch.empty(lib.cp_hr_chain_weight_bytes(Cc, H, W), dtype=torch.uint8, device=dev())
    for i, w in enumerate(ws):
        wd = w.contiguous().to(dev())
        sd_ = affs[i][0].contiguous().to(dev())               # the folded-BN scale goes into the packed weights
        _abi.check(lib.cp_pack_hr_chain_weight(st(), wd.data_ptr(), sd_.data_ptr(), Cc, H, W, i, blob.data_ptr()))
        torch.cuda.synchronize()
    n = lib.cp_hr_chain_affine_floats(Cc, H, W)
    aff = torch.zeros(8, 2, n)
    for i, (s_, t_) in enumerate(affs):
        aff[i, 0, :Cc], aff[i, 1, :Cc] = s_, t_
    aff = aff.to(dev())
    srcs = [to_cl(t, dtype) for t in terms]
    cp = srcs[0].shape[-1]
    out = torch.full((B, H, W, cp), float("nan"), dtype=DT[dtype], device=dev())
    arr_p = (C.c_void_p * 4)(*([s_.data_ptr() for s_ in srcs] + [None] * (4 - nsrc)))
    arr_s = (C.c_int32 * 4)(*(shifts + [0] * (4 - nsrc)))
    _abi.check(lib.cp_hr_branch_chain(st(), B, Cc, H, W, nsrc, arr_p, arr_s, 1 if nsrc > 1 else 0, blob.data_ptr(), aff.data_ptr(),
                                      out.data_ptr()), "hr chain")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    if cp > Cc:
        assert float(out[..., Cc:].float().abs().max()) == 0.0
    close(from_cl(out, Cc), ref, 4e-2)
    arr_p[0] = out.data_ptr()
    assert lib.cp_hr_branch_chain(st(), B, Cc, H, W, nsrc, arr_p, arr_s, 0, blob.data_ptr(), aff.data_ptr(), out.data_ptr()) == -1


@pytest.mark.parametrize("tconvs", [[(36, False)], [(36, False), (18, True)], [(36, False), (18, True), (18, True)]])
def test_hr_branch_chain_tail_vs_fuse_out_and_torch(lib, tconvs):
    """cp_hr_branch_chain_tail: the 64 x 64 x 18 chain launch also produces the stride-2 fuse-layer convs that read its output
    (timm HighResolutionModule.fuse_layers[i][0][0], i = 1..3).  The chain output is bit-identical to cp_hr_branch_chain's; every
    tail output matches torch's conv3x3 / stride 2 over that (bf16) output + folded BN (+ ReLU), pad channels exactly zero -- the same
    reference cp_hr_fuse_out is held to; bad tails are refused."""
    from checkerpose_amd._abi import CpChainTail
    Cc, H, W, B, dtype = 18, 64, 64, 3, CP_BF16
    assert lib.cp_hr_chain_tail_supported(18, 64, 64) == 1 and lib.cp_hr_chain_tail_supported(36, 32, 32) == 0
    terms = [det_tensor("tt0", (B, Cc, H, W)), det_tensor("tt1", (B, Cc, H // 2, W // 2))]
    shifts = [0, 1]
    ws = [det_tensor("tw%d" % i, (Cc, Cc, 3, 3), (2.0 / (Cc * 9)) ** 0.5 * 1.5) for i in range(8)]
    affs = [(1.0 + 0.3 * det_tensor("ts%d" % i, (Cc,)), 0.2 * det_tensor("tb%d" % i, (Cc,))) for i in range(8)]
    for i in range(1, 8, 2):
        affs[i] = (affs[i][0] * 0.4, affs[i][1])
    blob = torch.empty(lib.cp_hr_chain_weight_bytes(Cc, H, W), dtype=torch.uint8, device=dev())
    for i, w in enumerate(ws):
        wd, sd_ = w.contiguous().to(dev()), affs[i][0].contiguous().to(dev())
        _abi.check(lib.cp_pack_hr_chain_weight(st(), wd.data_ptr(), sd_.data_ptr(), Cc, H, W, i, blob.data_ptr()))
        torch.cuda.synchronize()
    n = lib.cp_hr_chain_affine_floats(Cc, H, W)
    aff = torch.zeros(8, 2, n)
    for i, (s_, t_) in enumerate(affs):
        aff[i, 0, :Cc], aff[i, 1, :Cc] = s_, t_
    aff = aff.to(dev())
    srcs = [to_cl(t, dtype) for t in terms]
    cp = srcs[0].shape[-1]
    arr_p = (C.c_void_p * 4)(*([s_.data_ptr() for s_ in srcs] + [None] * 2))
    arr_s = (C.c_int32 * 4)(*(shifts + [0, 0]))
    plain = torch.full((B, H, W, cp), float("nan"), dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_hr_branch_chain(st(), B, Cc, H, W, 2, arr_p, arr_s, 1, blob.data_ptr(), aff.data_ptr(), plain.data_ptr()), "hr chain")
    # ---- tail
    tb = torch.zeros(lib.cp_hr_chain_tail_weight_bytes(), dtype=torch.uint8, device=dev())
    tsh = torch.zeros(lib.cp_hr_chain_tail_channels(), dtype=torch.float32, device=dev())
    tl = CpChainTail()
    keep, touts, tw, piece = [], [], [], 0
    for i, (Cout, relu) in enumerate(tconvs):
        w = det_tensor("ttw%d" % i, (Cout, Cc, 3, 3), (2.0 / (Cc * 9)) ** 0.5 * 1.7)
        scale, shift = 1.0 + 0.3 * det_tensor("tts%d" % i, (Cout,)), 0.2 * det_tensor("ttt%d" % i, (Cout,))
        ocp = rup(Cout, 8)
        wd, sd_ = w.contiguous().to(dev()), scale.contiguous().to(dev())
        _abi.check(lib.cp_pack_hr_chain_tail_weight(st(), wd.data_ptr(), sd_.data_ptr(), Cout, piece, ocp, tb.data_ptr()), "tail pack")
        tsh[piece * 8: piece * 8 + Cout] = shift.to(dev())
        o = torch.full((B, H // 2, W // 2, ocp), float("nan"), dtype=DT[dtype], device=dev())
        tl.out[i], tl.Cout[i], tl.out_cphys[i], tl.relu[i] = o.data_ptr(), Cout, ocp, 1 if relu else 0
        touts.append(o)
        tw.append((w, scale, shift, relu))
        keep += [wd, sd_]
        piece += ocp // 8
    tl.packed_w, tl.shift, tl.nconv = tb.data_ptr(), tsh.data_ptr(), len(tconvs)
    out = torch.full((B, H, W, cp), float("nan"), dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_hr_branch_chain_tail(st(), B, Cc, H, W, 2, arr_p, arr_s, 1, blob.data_ptr(), aff.data_ptr(), out.data_ptr(), C.byref(tl)),
               "hr chain tail")
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), plain.view(torch.int16)), "the chain's own output must not change"
    x = from_cl(out, Cc)                                       # exactly the (bf16) map the tail read from LDS
    for (w, scale, shift, relu), o in zip(tw, touts):
        Cout = w.shape[0]
        r = F.conv2d(x, rnd(w * scale.view(-1, 1, 1, 1), dtype), None, 2, 1) + shift.view(1, -1, 1, 1)     # the scale lives in the bf16 weights
        r = F.relu(r) if relu else r
        assert bool(torch.isfinite(o.float()).all()), "every output element must be written"
        if o.shape[-1] > Cout:
            assert float(o[..., Cout:].float().abs().max()) == 0.0, "padded channels must be exactly zero"
        close(from_cl(o, Cout), r, TOL[dtype])
    tl.nconv = 4
    assert lib.cp_hr_branch_chain_tail(st(), B, Cc, H, W, 2, arr_p, arr_s, 1, blob.data_ptr(), aff.data_ptr(), out.data_ptr(), C.byref(tl)) == -1
    tl.nconv = len(tconvs)
    if len(tconvs) > 1:                                        # padded channel counts beyond the 96 the tail holds (refused before any launch)
        tl.out_cphys[0] = 96
        assert lib.cp_hr_branch_chain_tail(st(), B, Cc, H, W, 2, arr_p, arr_s, 1, blob.data_ptr(), aff.data_ptr(), out.data_ptr(), C.byref(tl)) == -1
    assert lib.cp_pack_hr_chain_tail_weight(st(), keep[0].data_ptr(), keep[1].data_ptr(), 36, 9, 40, tb.data_ptr()) == -1     # past 96 channels


@pytest.mark.parametrize("Cc,H,W,B,tconvs", [
    (36, 32, 32, 3, [(0, 18, False), (1, 72, False), (1, 36, True)]),      # stage 4, branch 1: 1x1 -> 0, s2 -> 2, s2 (+ReLU) towards 3
    (36, 32, 32, 2, [(0, 18, False)]),                                     # stage 2
    (72, 16, 16, 5, [(0, 18, False), (0, 36, False), (1, 144, False)]),    # stage 4, branch 2 (one crop per workgroup at this batch)
    (144, 8, 8, 6, [(0, 18, False), (0, 36, False), (0, 72, False)]),      # stage 4, branch 3 (one crop per workgroup at this batch)
    (72, 16, 16, 193, [(0, 18, False), (0, 36, False), (1, 144, False)]),  # ... two crops per workgroup (from 192 crops), ragged batch
    (144, 8, 8, 98, [(0, 18, False), (0, 36, False), (0, 72, False)]),     # ... two crops per workgroup (96 .. 191 crops)
    (144, 8, 8, 194, [(0, 18, False), (0, 36, False), (0, 72, False)]),    # ... four crops per workgroup, ragged batch
])
def test_hr_branch_chain_tails_vs_torch(lib, Cc, H, W, B, tconvs):
    """cp_hr_branch_chain_tails (round 5): the 36 / 72 / 144-channel chain launches also produce the first-level fuse-layer convs that read
    their branch (timm HighResolutionModule.fuse_layers[i][j]: the 1x1 conv + BN towards higher-resolution branches, the first 3x3 /
    stride-2 conv + BN (+ ReLU) towards lower-resolution ones) off the map in LDS.  The chain output is bit-identical to
    cp_hr_branch_chain's; every tail output matches torch's conv over that (bf16) output with the BN scale folded into bf16 weights --
    the reference cp_hr_fuse_out is held to; padded channels exactly zero; unsupported (kind, Cout) pairs are refused."""
    from checkerpose_amd._abi import CpChainTailConv
    dtype = CP_BF16
    terms = [det_tensor("ct0_%d" % Cc, (B, Cc, H, W)), det_tensor("ct1_%d" % Cc, (B, Cc, H // 2, W // 2))]
    shifts = [0, 1]
    ws = [det_tensor("ctw%d_%d" % (i, Cc), (Cc, Cc, 3, 3), (2.0 / (Cc * 9)) ** 0.5 * 1.5) for i in range(8)]
    affs = [(1.0 + 0.3 * det_tensor("cts%d" % i, (Cc,)), 0.2 * det_tensor("ctb%d" % i, (Cc,))) for i in range(8)]
    for i in range(1, 8, 2):
        affs[i] = (affs[i][0] * 0.4, affs[i][1])
    blob = torch.empty(lib.cp_hr_chain_weight_bytes(Cc, H, W), dtype=torch.uint8, device=dev())
    for i, w in enumerate(ws):
        wd, sd_ = w.contiguous().to(dev()), affs[i][0].contiguous().to(dev())
        _abi.check(lib.cp_pack_hr_chain_weight(st(), wd.data_ptr(), sd_.data_ptr(), Cc, H, W, i, blob.data_ptr()))
        torch.cuda.synchronize()
    n = lib.cp_hr_chain_affine_floats(Cc, H, W)
    aff = torch.zeros(8, 2, n)
    for i, (s_, t_) in enumerate(affs):
        aff[i, 0, :Cc], aff[i, 1, :Cc] = s_, t_
    aff = aff.to(dev())
    srcs = [to_cl(t, dtype) for t in terms]
    cp = srcs[0].shape[-1]
    arr_p = (C.c_void_p * 4)(*([s_.data_ptr() for s_ in srcs] + [None] * 2))
    arr_s = (C.c_int32 * 4)(*(shifts + [0, 0]))
    plain = torch.full((B, H, W, cp), float("nan"), dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_hr_branch_chain(st(), B, Cc, H, W, 2, arr_p, arr_s, 1, blob.data_ptr(), aff.data_ptr(), plain.data_ptr()), "hr chain")
    arr = (CpChainTailConv * len(tconvs))()
    keep, touts, tw = [], [], []
    for i, (kind, Cout, relu) in enumerate(tconvs):
        k = 3 if kind else 1
        assert lib.cp_hr_chain_tailconv_supported(Cc, H, W, kind, Cout) == 1
        w = det_tensor("ctt%d_%d" % (i, Cc), (Cout, Cc, k, k), (2.0 / (Cc * k * k)) ** 0.5 * 1.7)
        scale, shift = 1.0 + 0.3 * det_tensor("ctts%d" % i, (Cout,)), 0.2 * det_tensor("cttt%d" % i, (Cout,))
        ocp = rup(Cout, 8)
        wd, sd_ = w.contiguous().to(dev()), scale.contiguous().to(dev())
        buf = torch.empty(lib.cp_hr_chain_tailconv_weight_bytes(Cc, H, W, kind, Cout), dtype=torch.uint8, device=dev())
        _abi.check(lib.cp_pack_hr_chain_tailconv_weight(st(), wd.data_ptr(), sd_.data_ptr(), Cc, H, W, kind, Cout, buf.data_ptr()), "tail pack")
        sh = torch.zeros(rup(Cout, 16), dtype=torch.float32, device=dev())
        sh[:Cout] = shift.to(dev())
        o = torch.full((B, H >> kind, W >> kind, ocp), float("nan"), dtype=DT[dtype], device=dev())
        arr[i].packed_w, arr[i].shift, arr[i].out = buf.data_ptr(), sh.data_ptr(), o.data_ptr()
        arr[i].kind, arr[i].Cout, arr[i].out_cphys, arr[i].relu = kind, Cout, ocp, 1 if relu else 0
        touts.append(o)
        tw.append((kind, w, scale, shift, relu))
        keep += [wd, sd_, buf, sh]
    out = torch.full((B, H, W, cp), float("nan"), dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_hr_branch_chain_tails(st(), B, Cc, H, W, 2, arr_p, arr_s, 1, blob.data_ptr(), aff.data_ptr(), out.data_ptr(), len(tconvs), arr),
               "hr chain tails")
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), plain.view(torch.int16)), "the chain's own output must not change"
    x = from_cl(out, Cc)                                       # exactly the (bf16) map the tails read from LDS
    for (kind, w, scale, shift, relu), o in zip(tw, touts):
        Cout = w.shape[0]
        wq = rnd(w * scale.view(-1, 1, 1, 1), dtype)           # the scale lives in the bf16 weights
        r = (F.conv2d(x, wq, None, 2, 1) if kind else F.conv2d(x, wq)) + shift.view(1, -1, 1, 1)
        r = F.relu(r) if relu else r
        assert bool(torch.isfinite(o.float()).all()), "every output element must be written"
        if o.shape[-1] > Cout:
            assert float(o[..., Cout:].float().abs().max()) == 0.0, "padded channels must be exactly zero"
        close(from_cl(o, Cout), r, TOL[dtype])
    assert lib.cp_hr_chain_tailconv_supported(Cc, H, W, 1, 18) == 0 and lib.cp_hr_chain_tailconv_supported(18, 64, 64, 0, 18) == 0
    assert lib.cp_hr_branch_chain_tails(st(), B, Cc, H, W, 2, arr_p, arr_s, 1, blob.data_ptr(), aff.data_ptr(), out.data_ptr(), 4, arr) == -1
    arr[0].out = out.data_ptr()                                # a tail output aliasing the chain output: refused
    assert lib.cp_hr_branch_chain_tails(st(), B, Cc, H, W, 2, arr_p, arr_s, 1, blob.data_ptr(), aff.data_ptr(), out.data_ptr(), 1, arr) == -1


@pytest.mark.parametrize("ds", [False, True])
@pytest.mark.parametrize("shape", [(2, 16, 32), (1, 13, 21), (9, 8, 16), (3, 64, 64)])
def test_bottleneck_fused_vs_torch_cpu(lib, shape, ds):
    """Fused Bottleneck (cp_bottleneck_fused, bf16) == relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) +
    shortcut(x)) with both intermediates rounded to bf16 (they live in LDS as bf16): identity shortcut (256 in) and the
    projection shortcut of layer1.0 (64 in); image borders (t1's out-of-image ring must be zero padding), ragged tiles,
    more crops than XCDs, a channel-sliced input and a strided output."""
    dtype = CP_BF16
    B, H, W = shape
    Cin = 64 if ds else 256
    x = det_tensor("btx%s%d" % (shape, Cin), (B, Cin, H, W))
    w1 = det_tensor("btw1%d" % Cin, (64, Cin, 1, 1), (2.0 / Cin) ** 0.5 * 1.7)
    w2 = det_tensor("btw2", (64, 64, 3, 3), (2.0 / (64 * 9)) ** 0.5 * 1.7)
    w3 = det_tensor("btw3", (256, 64, 1, 1), (2.0 / 64) ** 0.5 * 0.7)
    wd = det_tensor("btwd", (256, 64, 1, 1), (2.0 / 64) ** 0.5)
    aff = [(1.0 + 0.3 * det_tensor("bts%d" % i, (n,)), 0.3 * det_tensor("btt%d" % i, (n,))) for i, n in enumerate((64, 64, 256, 256))]
    v4 = lambda v: v.view(1, -1, 1, 1)
    xr = rnd(x, dtype)
    y1 = rnd(F.relu(F.conv2d(xr, rnd(w1, dtype)) * v4(aff[0][0]) + v4(aff[0][1])), dtype)
    y2 = rnd(F.relu(F.conv2d(y1, rnd(w2, dtype), None, 1, 1) * v4(aff[1][0]) + v4(aff[1][1])), dtype)
    short = F.conv2d(xr, rnd(wd, dtype)) * v4(aff[3][0]) + v4(aff[3][1]) if ds else xr
    ref = F.relu(F.conv2d(y2, rnd(w3, dtype)) * v4(aff[2][0]) + v4(aff[2][1]) + short)
    cs, coff = Cin + 16, 8                                         # input = channel slice [8, 8+Cin) of a wider tensor
    xin = torch.zeros(B, H, W, cs, dtype=DT[dtype], device=dev())
    xin[..., coff:coff + Cin] = x.permute(0, 2, 3, 1).to(dev()).to(DT[dtype])
    ocs = 256 + 8
    out = torch.full((B, H, W, ocs), float("nan"), dtype=DT[dtype], device=dev())
    pws = []
    for w, (co, ci, r) in zip((w1, w2, w3, wd), ((64, Cin, 1), (64, 64, 3), (256, 64, 1), (256, 64, 1))):
        pw = torch.empty(lib.cp_packed_weight_bytes(dtype, co, ci, r, r), dtype=torch.uint8, device=dev())
        wdev = w.contiguous().to(dev())
        _abi.check(lib.cp_pack_conv_weight(st(), dtype, wdev.data_ptr(), co, ci, r, r, ci, 0, 0, None, co, pw.data_ptr()))
        pws.append(pw)
    a = [v.contiguous().to(dev()) for pair in aff for v in pair]
    d = CpConvDesc()
    d.dtype, d.out_f32, d.B, d.H, d.W = dtype, 0, B, H, W
    d.Cin, d.in_cstride, d.in_coff = Cin, cs, coff
    d.R, d.S, d.stride, d.pad, d.Ho, d.Wo, d.Cout, d.act, d.slope = 3, 3, 1, 1, H, W, 256, ACT_RELU, 0.0
    d.o_base, d.o_sb, d.o_sy, d.o_sx, d.o_sc = 0, H * W * ocs, W * ocs, ocs, 1
    args = (pws[0].data_ptr(), a[0].data_ptr(), a[1].data_ptr(), pws[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(),
            pws[2].data_ptr(), a[4].data_ptr(), a[5].data_ptr())
    args += (pws[3].data_ptr(), a[6].data_ptr(), a[7].data_ptr()) if ds else (None, None, None)
    _abi.check(lib.cp_bottleneck_fused(st(), C.byref(d), xin.data_ptr(), *args, out.data_ptr()), "fused bottleneck")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[..., 256:].float()).all())          # channels past 256 of the output rows untouched
    close(from_cl(out[..., :256].contiguous(), 256), ref, 4e-2)
    assert lib.cp_bottleneck_fused(st(), C.byref(d), xin.data_ptr(), *args, xin.data_ptr()) == -1      # in-place refused
    assert lib.cp_bottleneck_fused(st(), C.byref(d), xin.data_ptr(), *(args[:9] + (args[9], None, None)), out.data_ptr()) == -1 or not ds
    d.Cin = 256 if ds else 64
    assert lib.cp_bottleneck_fused(st(), C.byref(d), xin.data_ptr(), *args, out.data_ptr()) == -1      # Cin must match the shortcut kind
    d.Cin, d.dtype = Cin, CP_F32
    assert lib.cp_bottleneck_fused(st(), C.byref(d), xin.data_ptr(), *args, out.data_ptr()) == -1      # bf16 only


GEMM_CASES = [  # (B, H, W, Cin, Cout, act, residual)
    (2, 1, 200, 256, 512, ACT_NONE, False),     # EdgeConv node GEMM shape class, M = 400 not a multiple of 128
    (1, 16, 16, 64, 256, ACT_RELU, True),       # bottleneck conv3 + residual, K = 1 (f32: 1) super-chunk
    (3, 1, 100, 320, 256, ACT_LEAKY, False),    # pre_graph MLP: K = 320 (ragged super-chunk)
    (1, 8, 8, 1024, 136, ACT_RELU, True),       # deep K, Cout = 136 (partial last channel group), residual
    (1, 5, 7, 144, 100, ACT_NONE, False),       # odd everything
    # M >= 16384 without residual, K <= 256: the bf16 weight-stationary persistent kernel (gemm_rows_ws_kernel)
    (33, 1, 512, 256, 512, ACT_NONE, False),    # EdgeConv node GEMM at full N: two column groups, M = 16896 (264 row tiles)
    (4, 1, 4133, 160, 136, ACT_LEAKY, False),   # ragged M (16532 = 258.3 tiles), K = 160 (5 chunks), partial last group
    (2, 96, 96, 72, 256, ACT_RELU, False),      # image-shaped rows (H, W strides), K = 72 (ragged chunk)
    # ... 256 < K <= 512: its 8-wave variant (a wave owns 32 channels)
    (33, 1, 512, 512, 256, ACT_LEAKY, False),   # refinement pre_graph MLP: M = 16896
    (4, 1, 4133, 320, 296, ACT_LEAKY, False),   # stage-0 pre_graph MLP K = 320 (10 chunks), ragged M, two column groups, partial last group
]


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", GEMM_CASES)
def test_gemm_rows_vs_torch_cpu(lib, dtype, case):
    """LDS-staged 1x1 conv / Linear kernel (cp_gemm_rows) == torch CPU conv1x1 + affine + residual + act."""
    B, H, W, Cin, Cout, act, has_res = case
    x = det_tensor("gx%s" % (case,), (B, Cin, H, W))
    w = det_tensor("gw%s" % (case,), (Cout, Cin, 1, 1), (2.0 / Cin) ** 0.5 * 1.7)
    scale = 1.0 + 0.3 * det_tensor("gs%s" % (case,), (Cout,))
    shift = 0.2 * det_tensor("gt%s" % (case,), (Cout,))
    ref = F.conv2d(rnd(x, dtype), rnd(w, dtype)) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    res = None
    if has_res:
        res = det_tensor("gr%s" % (case,), tuple(ref.shape))
        ref = ref + rnd(res, dtype)
    ref = F.relu(ref) if act == ACT_RELU else (F.leaky_relu(ref, 0.01) if act == ACT_LEAKY else ref)
    E = 8 if dtype == CP_BF16 else 4
    xin = to_cl(x, dtype)
    cop = rup(Cout, E)
    out = torch.full((B, H, W, cop), float("nan"), dtype=DT[dtype], device=dev())
    pw = torch.empty(lib.cp_packed_gemm_weight_bytes(dtype, Cout, xin.shape[-1]), dtype=torch.uint8, device=dev())
    wd = w.contiguous().to(dev())
    _abi.check(lib.cp_pack_gemm_weight(st(), dtype, wd.data_ptr(), Cout, Cin, xin.shape[-1], pw.data_ptr()))
    n16 = rup(Cout, 16)
    sc = torch.zeros(n16); sc[:Cout] = scale
    sh = torch.zeros(n16); sh[:Cout] = shift
    sc, sh = sc.to(dev()), sh.to(dev())
    rs = to_cl(res, dtype) if res is not None else None
    d = CpConvDesc()
    d.dtype, d.out_f32, d.B, d.H, d.W = dtype, 0, B, H, W
    d.Cin, d.in_cstride, d.in_coff = xin.shape[-1], xin.shape[-1], 0
    d.R, d.S, d.stride, d.pad, d.Ho, d.Wo, d.Cout, d.act, d.slope = 1, 1, 1, 0, H, W, cop, act, 0.01
    d.o_base, d.o_sb, d.o_sy, d.o_sx, d.o_sc = 0, H * W * cop, W * cop, cop, 1
    _abi.check(lib.cp_gemm_rows(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                rs.data_ptr() if rs is not None else None, out.data_ptr()), "gemm rows")
    torch.cuda.synchronize()
    if cop > Cout:
        assert float(out[..., Cout:].float().abs().max()) == 0.0
    close(from_cl(out, Cout), ref, TOL[dtype])
    d.R = 3
    assert lib.cp_gemm_rows(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(), None, out.data_ptr()) == -1


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_convtranspose_phases_vs_torch_cpu(lib, dtype):
    """ConvTranspose2d(k3,s2,p1,op1) (pipeline.py:187-197) as 4 sub-pixel phase convs."""
    B, Cin, H, W, Cout = 2, 32, 5, 6, 24
    x = det_tensor("tx", (B, Cin, H, W))
    w = det_tensor("tw", (Cin, Cout, 3, 3), 0.2)
    ref = F.conv_transpose2d(rnd(x, dtype), rnd(w, dtype), None, stride=2, padding=1, output_padding=1)
    xin = to_cl(x, dtype)
    cop = rup(Cout, 8 if dtype == CP_BF16 else 4)
    out = torch.full((B, 2 * H, 2 * W, cop), float("nan"), dtype=DT[dtype], device=dev())
    one = torch.ones(rup(Cout, 16), device=dev()); zero = torch.zeros(rup(Cout, 16), device=dev())
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        pw = pack(lib, dtype, w, xin.shape[-1], 1 + a, 1 + b, transposed=1, phase=ph)
        d = CpConvDesc()
        d.dtype, d.out_f32, d.B, d.H, d.W = dtype, 0, B, H, W
        d.Cin, d.in_cstride, d.in_coff = xin.shape[-1], xin.shape[-1], 0
        d.R, d.S, d.stride, d.pad, d.Ho, d.Wo, d.Cout, d.act, d.slope = 1 + a, 1 + b, 1, 0, H, W, cop, ACT_NONE, 0.0
        d.o_base, d.o_sb, d.o_sy, d.o_sx, d.o_sc = (a * 2 * W + b) * cop, 4 * H * W * cop, 2 * 2 * W * cop, 2 * cop, 1
        _abi.check(lib.cp_conv2d_igemm(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), one.data_ptr(), zero.data_ptr(), None,
                                       out.data_ptr()), "convT phase")
    torch.cuda.synchronize()
    close(from_cl(out, Cout), ref, TOL[dtype])


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_upsample_fuse_maxpool(lib, dtype):
    tol = TOL[dtype]
    # bilinear x2 align_corners into a channel slice of a wider buffer (how the decoder builds its concat)
    x = det_tensor("ux", (2, 24, 5, 7))
    xin = to_cl(x, dtype)
    out = torch.zeros(2, 10, 14, 40, dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_upsample2x_bilinear_ac(st(), dtype, xin.data_ptr(), out.data_ptr(), 2, 5, 7, 24, 24, 0, 40, 16))
    torch.cuda.synchronize()
    ref = F.interpolate(rnd(x, dtype), scale_factor=2, mode="bilinear", align_corners=True)
    close(out[..., 16:40].float().cpu().permute(0, 3, 1, 2), ref, max(tol, 1e-5) if dtype == CP_F32 else 1e-2)
    assert float(out[..., :16].float().abs().max()) == 0.0
    # HRNet fuse: identity + two nearest-upsampled terms, ReLU
    a, b, c = det_tensor("fa", (2, 20, 8, 8)), det_tensor("fb", (2, 20, 4, 4)), det_tensor("fc", (2, 20, 2, 2))
    srcs = [to_cl(t, dtype, 24 if dtype == CP_BF16 else 20) for t in (a, b, c)]
    cp = srcs[0].shape[-1]
    o = torch.empty(2, 8, 8, cp, dtype=DT[dtype], device=dev())
    arr = (C.c_void_p * 4)(*[s.data_ptr() for s in srcs], None)
    sh = (C.c_int32 * 4)(0, 1, 2, 0)
    _abi.check(lib.cp_fuse_sum_act(st(), dtype, 3, arr, sh, o.data_ptr(), 2, 8, 8, cp, 1, cp, 0))
    torch.cuda.synchronize()
    ref = F.relu(rnd(a, dtype) + F.interpolate(rnd(b, dtype), scale_factor=2, mode="nearest")
                 + F.interpolate(rnd(c, dtype), scale_factor=4, mode="nearest"))
    close(from_cl(o, 20), ref, tol)
    wide = torch.full((2, 8, 8, cp + 16), 7.0, dtype=DT[dtype], device=dev())     # into the channel slice [8, 8 + cp) of a wider tensor
    _abi.check(lib.cp_fuse_sum_act(st(), dtype, 3, arr, sh, wide.data_ptr(), 2, 8, 8, cp, 1, cp + 16, 8))
    torch.cuda.synchronize()
    assert torch.equal(wide[..., 8:8 + cp], o) and float((wide[..., :8] - 7).abs().max()) == 0 and float((wide[..., 8 + cp:] - 7).abs().max()) == 0
    # max pool 3x3 s2 p1
    x = det_tensor("mp", (2, 16, 12, 10))
    xin = to_cl(x, dtype)
    o = torch.empty(2, 6, 5, 16, dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_maxpool3x3s2(st(), dtype, xin.data_ptr(), o.data_ptr(), 2, 12, 10, 16))
    torch.cuda.synchronize()
    close(from_cl(o, 16), F.max_pool2d(rnd(x, dtype), 3, 2, 1), 1e-7)


def _edge_ref(sd, pfx, x, idx, slope=0.2):
    return O.static_graph_module(sd, pfx, x, idx, slope)


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("Cc,pfx", [(64, "init_net.pre_query_block.0"), (256, "refine_net.1.pre_query_block.2")])
def test_edgeconv_factored_vs_reference_form(lib, dtype, Cc, pfx):
    """Factored EdgeConv (per-node GEMM -> [P'|Q'], gather-max) == the reference's per-edge conv+BN+LeakyReLU+max
    on the real LM-O `ape` kNN graph, with mixed-sign BatchNorm gammas."""
    from checkerpose_amd.engine import Program, WeightStore
    from checkerpose_amd.netbuilder import NetEmitter
    net = build_net(seed=0)
    sd_cpu = net.state_dict()
    assert (sd_cpu[pfx + ".conv.1.weight"] < 0).any() and (sd_cpu[pfx + ".conv.1.weight"] > 0).any()
    idx = net.init_net.knn_idx
    B, N = 3, 512
    x = det_tensor("ex%d" % Cc, (B, Cc, N))
    ref = _edge_ref(sd_cpu, pfx, rnd(x, dtype), idx)
    sd = {k: v.to(dev()) for k, v in sd_cpu.items() if k.startswith(pfx)}
    ws = WeightStore(lib, sd, dtype, dev())
    prog = Program(lib, ws, dtype, B, dev())
    em = NetEmitter(prog, sd)
    xin = prog.act(1, N, Cc)
    idx_d = idx.to(torch.int32).contiguous().to(dev())
    out = em.edgeconv(pfx, xin, dict(idx=idx_d, gids=None, K=20, G=1), 0.2)
    prog._add(lambda *a: 0, lambda P: (), "keepalive", [xin.tbuf, out.tbuf], [])   # nothing is recycled before read-back
    prog.finalize()
    es = 2 if dtype == CP_BF16 else 4

    def tview(a):
        n = a.B * a.H * a.W * a.cstride
        return prog.workspace[a.tbuf.offset: a.tbuf.offset + n * es].view(DT[dtype]).view(a.B, a.W, a.cstride)

    tview(xin).copy_(x.permute(0, 2, 1).to(DT[dtype]))
    prog.run(st())
    torch.cuda.synchronize()
    got = tview(out).float().cpu().permute(0, 2, 1)
    close(got, ref, 1e-5 if dtype == CP_F32 else 4e-2)


@pytest.mark.parametrize("Cc,pfx", [(64, "init_net.pre_query_block.0"), (256, "refine_net.1.pre_query_block.2")])
def test_edgeconv_fused_vs_reference_form(lib, monkeypatch, Cc, pfx):
    """cp_edgeconv_fused (node GEMM + LDS gather-max in one launch, N = 512, bf16) == the reference's per-edge
    conv + BN + LeakyReLU + max (StaticGraph_module) on the real `ape` graph with mixed-sign BN gammas, a channel-sliced
    output and per-sample LM graphs (graph ids), B not a multiple of anything."""
    from checkerpose_amd import engine
    from checkerpose_amd.engine import Program, WeightStore
    from checkerpose_amd.netbuilder import NetEmitter
    monkeypatch.setattr(engine, "EDGE_FUSED_MIN_BATCH", 1)
    monkeypatch.setattr(engine, "MLP_FUSED_MIN_ROWS", 1)
    dtype = CP_BF16
    net = build_net(seed=0)
    sd_cpu = net.state_dict()
    idx15 = O.knn(lm_p3d(512), 20)                                      # (15, N, K): per-sample graphs
    obj = torch.tensor([3, 15, 1, 9, 9])
    B, N = 5, 512
    x = det_tensor("efx%d" % Cc, (B, Cc, N))
    ref = torch.cat([_edge_ref(sd_cpu, pfx, rnd(x[i:i + 1], dtype), idx15[obj[i] - 1:obj[i]]) for i in range(B)], 0)
    sd = {k: v.to(dev()) for k, v in sd_cpu.items() if k.startswith(pfx)}
    ws = WeightStore(lib, sd, dtype, dev())
    prog = Program(lib, ws, dtype, B, dev())
    em = NetEmitter(prog, sd)
    xin = prog.act(1, N, Cc)
    wide = prog.act(1, N, Cc + 64)
    idx_d = idx15.to(torch.int32).contiguous().to(dev())
    gids = (obj - 1).to(torch.int32).to(dev())
    out = em.edgeconv(pfx, xin, dict(idx=idx_d, gids=gids, K=20, G=15), 0.2, out=wide.slice(64, Cc))
    assert prog.ops[-1][2].startswith("edge_fused")
    prog._add(lambda *a: 0, lambda P: (), "keepalive", [xin.tbuf, wide.tbuf], [])
    prog.finalize()

    def tview(a):
        n = a.B * a.H * a.W * a.cstride
        return prog.workspace[a.tbuf.offset: a.tbuf.offset + n * 2].view(torch.bfloat16).view(a.B, a.W, a.cstride)

    tview(xin).copy_(x.permute(0, 2, 1).to(torch.bfloat16))
    tview(wide).fill_(7.0)
    prog.run(st())
    torch.cuda.synchronize()
    got = tview(wide).float().cpu()
    assert float((got[..., :64] - 7.0).abs().max()) == 0.0               # channels outside the slice untouched
    close(got[..., 64:].permute(0, 2, 1), ref, 4e-2)
    assert out.coff == 64


def test_edgeconv_fused_keys_saturate_at_the_f16_range(lib):
    """The gather keys P' = s (W1 x) of cp_edgeconv_fused / cp_edgeconv_tiled are tabled as IEEE halves (v_pk_maximum3_f16):
    |P'| beyond 65 504 is CLAMPED there, where a bf16 / fp32 table would carry the value ("Numerical range").  Pinned
    here so that the behaviour is a documented contract, not a surprise: four channels are driven to |P'| ~ 2e5 through their folded
    BatchNorm scale; the kernel must equal leaky(max_k clamp_f16(P'_j) + Q'_i) and must NOT equal the unclamped form there; the other
    60 channels are untouched by the clamp."""
    B, N, K, Cc = 2, 512, 20, 64
    idx = O.knn(ape_p3d(512), K)                                        # (1, N, K)
    x = rnd(det_tensor("clampx", (B, N, Cc)), CP_BF16)
    w1 = rnd(det_tensor("clampw1", (Cc, Cc), (3.0 / Cc) ** 0.5), CP_BF16)
    dq = rnd(det_tensor("clampdq", (Cc, Cc), (3.0 / Cc) ** 0.5), CP_BF16)        # W2 - W1
    dq[:4] = 0.0                                                        # big channels: Q' = t (keeps the sum inside fp32 / bf16 sanity)
    s_ = 1.0 + 0.3 * det_tensor("clamps", (Cc,))
    s_[:4] = torch.tensor([4e5, -4e5, 2.5e5, -3e5])                     # folded scale: |P'| up to ~2e5, both signs
    t_ = det_tensor("clampt", (Cc,), 0.5)
    P = (x @ w1.t()) * s_                                               # (B, N, C) fp32
    assert float(P[..., :4].abs().max()) > 1.2e5 and float(P[..., 4:].abs().max()) < 100.0
    Q = (x @ dq.t()) * s_ + t_
    gi = idx[0]                                                         # (N, K)

    def form(tab):
        nb = tab[:, gi]                                                 # (B, N, K, C)
        return F.leaky_relu(nb.max(dim=2)[0] + Q, 0.2)
    ref = form(P.clamp(-65504.0, 65504.0).to(torch.float16).float())
    unclamped = form(P)
    wpq = torch.cat([w1, dq], 0).contiguous().to(dev())
    scale, shift = torch.cat([s_, s_]).to(dev()), torch.cat([torch.zeros_like(t_), t_]).to(dev())
    pk = torch.empty(lib.cp_edgeconv_fused_weight_bytes(Cc, Cc), dtype=torch.uint8, device=dev())
    _abi.check(lib.cp_pack_edgeconv_fused_weight(st(), wpq.data_ptr(), Cc, Cc, pk.data_ptr()))
    xd = x.to(torch.bfloat16).to(dev())
    idx_d = idx.to(torch.int32).contiguous().to(dev())
    out = torch.empty(B, N, Cc, dtype=torch.bfloat16, device=dev())
    _abi.check(lib.cp_edgeconv_fused(st(), xd.data_ptr(), Cc, 0, pk.data_ptr(), scale.data_ptr(), shift.data_ptr(), idx_d.data_ptr(), None,
                                     out.data_ptr(), Cc, 0, B, N, K, Cc, Cc, 1, 0.2))
    torch.cuda.synchronize()
    got = out.float().cpu()
    rel = (got - ref).abs() / (ref.abs() + 1.0)
    assert float(rel.max()) <= 2e-2, float(rel.max())                   # bf16 output rounding + f16 key rounding
    big = got[..., :4]
    assert float(big.max()) <= 65504.0 * 1.01 + 1.0                     # positive side saturates at the f16 maximum (+ t)
    assert float((got - unclamped).abs()[..., :4].max()) > 3e4          # ... where the unclamped form is far away
    assert float(((got - unclamped).abs() / (unclamped.abs() + 1.0))[..., 4:].max()) <= 2e-2   # untouched channels: no clamp in play


@pytest.mark.parametrize("N,Cc,pfx", [(4096, 64, "init_net.pre_query_block.0"), (4096, 256, "refine_net.1.pre_query_block.2"),
                                      (1024, 256, "refine_net.0.pre_query_block.1")])
def test_edgeconv_tiled_vs_reference_form(lib, N, Cc, pfx):
    """cp_edgeconv_tiled (N > 512: key-table launch + per-patch LDS-staged gather launch, bf16) == the reference's per-edge
    conv + BN + LeakyReLU + max (StaticGraph_module, pipeline_lm.py:45-59) on the real LM graphs (per-sample graph ids, three
    objects), rows renumbered into patches by graph_sched.tile_schedule and un-permuted for the comparison; channel-sliced
    output, B = 5 (the grid is padded to a multiple of 8 crops)."""
    from checkerpose_amd.graph_sched import tile_schedule
    net = build_net(seed=0)
    sd = net.state_dict()
    objs = [0, 4, 13]                                                  # LM objects 1, 5, 14 (5: the largest halo)
    P = lm_p3d(N)[objs]
    idx3 = O.knn(P, 20)                                                # (3, N, K) original numbering
    sc = tile_schedule(idx3.numpy(), P.numpy())
    assert sc is not None and sc["HPAD"] % 64 == 0 and lib.cp_edgeconv_tiled_supported(N, 20, Cc, Cc, sc["HPAD"])
    gsel = torch.tensor([2, 0, 1, 1, 2])
    B = 5
    x = det_tensor("etx%d_%d" % (Cc, N), (B, Cc, N))
    xb = rnd(x, CP_BF16)
    ref = torch.cat([_edge_ref(sd, pfx, xb[i:i + 1], idx3[gsel[i]:gsel[i] + 1]) for i in range(B)], 0)        # (B, C', N)
    w = sd[pfx + ".conv.0.weight"]
    w1, w2 = w[:, :Cc, 0, 0], w[:, Cc:, 0, 0]
    bn = pfx + ".conv.1"
    s_ = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + 1e-5)
    t_ = sd[bn + ".bias"] - sd[bn + ".running_mean"] * s_
    wpq = torch.cat([w1, w2 - w1], 0).contiguous().to(dev())
    scale, shift = torch.cat([s_, s_]).to(dev()), torch.cat([torch.zeros_like(t_), t_]).to(dev())
    pf = torch.empty(lib.cp_edgeconv_fused_weight_bytes(Cc, Cc), dtype=torch.uint8, device=dev())
    pq = torch.empty(lib.cp_edgeconv_tiled_weight_bytes(Cc, Cc), dtype=torch.uint8, device=dev())
    _abi.check(lib.cp_pack_edgeconv_fused_weight(st(), wpq.data_ptr(), Cc, Cc, pf.data_ptr()))
    _abi.check(lib.cp_pack_edgeconv_tiled_weight(st(), wpq.data_ptr(), Cc, Cc, pq.data_ptr()))
    perm = torch.from_numpy(sc["perm"]).to(dev())
    halo, nbr = torch.from_numpy(sc["halo"]).contiguous().to(dev()), torch.from_numpy(sc["nbr"]).contiguous().to(dev())
    gids = gsel.to(torch.int32).to(dev())
    x_orig = xb.permute(0, 2, 1).contiguous().to(torch.bfloat16).to(dev())            # (B, N, C) original order
    x_int = torch.empty_like(x_orig)
    _abi.check(lib.cp_permute_rows(st(), x_orig.data_ptr(), x_int.data_ptr(), perm.data_ptr(), gids.data_ptr(), B, N, Cc * 2))
    assert torch.equal(x_int.cpu(), torch.stack([x_orig[i].cpu()[sc["perm"][gsel[i]].astype(np.int64)] for i in range(B)]))
    ktab = torch.empty(lib.cp_edgeconv_tiled_table_bytes(B, N, Cc), dtype=torch.uint8, device=dev())
    wide = torch.full((B, N, Cc + 64), 7.0, dtype=torch.bfloat16, device=dev())
    _abi.check(lib.cp_edgeconv_tiled(st(), x_int.data_ptr(), Cc, 0, pf.data_ptr(), pq.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                     halo.data_ptr(), nbr.data_ptr(), gids.data_ptr(), ktab.data_ptr(), wide.data_ptr(), Cc + 64, 64,
                                     B, N, 20, Cc, Cc, 3, int(sc["HPAD"]), 0.2))
    torch.cuda.synchronize()
    got_int = wide.float().cpu()
    assert float((got_int[..., :64] - 7.0).abs().max()) == 0.0           # channels outside the slice untouched
    out_f = torch.empty(B, Cc, N, dtype=torch.float32, device=dev())      # un-permute through cp_permute_cols on (B, C, N) fp32
    src = wide[..., 64:].float().permute(0, 2, 1).contiguous()
    _abi.check(lib.cp_permute_cols(st(), src.data_ptr(), out_f.data_ptr(), perm.data_ptr(), gids.data_ptr(), B, Cc, N, 4, 1))
    torch.cuda.synchronize()
    close(out_f.cpu(), ref, 4e-2)


@pytest.mark.parametrize("B,N", [(3, 512), (2, 100), (1, 4096)])
def test_mlp_query_fused_vs_torch(lib, B, N):
    """cp_mlp_query_fused (MLP_QueryNet, pipeline.py:168-180, as one launch) == the three nn.Linear layers in torch with the bf16
    roundings the kernel makes (input rows, layer-1 activations) and fp32 from there on; a channel-sliced input, rows that do not
    fill the last 64-row tile, logits written into their two rows of a (B, 13, N) block and nothing else touched."""
    net = build_net(seed=0)
    sd = net.state_dict()
    pfx = "refine_net.1.query_block.mlps."
    w = [sd[pfx + "%d.weight" % j].float() for j in (0, 2, 4)]
    b = [sd[pfx + "%d.bias" % j].float() for j in (0, 2, 4)]
    x = rnd(det_tensor("mlpq%d_%d" % (B, N), (B, N, 256)), CP_BF16)
    h1 = rnd(F.leaky_relu(x @ rnd(w[0], CP_BF16).t() + b[0], 0.01), CP_BF16)
    h2 = F.leaky_relu(h1 @ rnd(w[1], CP_BF16).t() + b[1], 0.01)
    ref = h2 @ w[2].t() + b[2]                                          # (B, N, 2)
    wide = torch.zeros(B, N, 320, dtype=torch.bfloat16, device=dev())
    wide[..., 64:] = x.to(torch.bfloat16).to(dev())
    pk = []
    for wi, (co, ci) in zip(w[:2], ((256, 256), (64, 256))):
        buf = torch.empty(lib.cp_packed_gemm_weight_bytes(CP_BF16, co, ci), dtype=torch.uint8, device=dev())
        wd = wi.contiguous().to(dev())
        _abi.check(lib.cp_pack_gemm_weight(st(), CP_BF16, wd.data_ptr(), co, ci, ci, buf.data_ptr()))
        pk.append(buf)
    ones = [torch.ones(256, device=dev()), torch.ones(64, device=dev())]
    bd = [t.contiguous().to(dev()) for t in b]
    w3 = w[2].contiguous().to(dev())
    bits = torch.full((B, 13, N), 7.0, device=dev())
    _abi.check(lib.cp_mlp_query_fused(st(), wide.data_ptr(), 320, 64, B, N, pk[0].data_ptr(), ones[0].data_ptr(), bd[0].data_ptr(), 0.01,
                                      pk[1].data_ptr(), ones[1].data_ptr(), bd[1].data_ptr(), 0.01, w3.data_ptr(), bd[2].data_ptr(),
                                      bits.data_ptr(), 5 * N, 13 * N, 1, 6 * N))
    torch.cuda.synchronize()
    got = bits.cpu()
    keep = [r for r in range(13) if r not in (5, 11)]
    assert float((got[:, keep] - 7.0).abs().max()) == 0.0               # only rows 5 and 11 of the logit block are written
    close(torch.stack([got[:, 5], got[:, 11]], -1), ref, 2e-3)          # fp32 accumulation order only (inputs rounded identically)


@pytest.mark.parametrize("B,N,stage", [(3, 512, 1), (2, 100, 0), (1, 4096, 2), (5, 33, 0)])
def test_mlp_pair_fused_vs_torch(lib, B, N, stage):
    """cp_mlp_pair_fused (Refine_moduleGNN.pre_graph_module, pipeline.py:237-240 / :283-286, as one launch) == the two nn.Linear +
    LeakyReLU in torch with the kernel's bf16 roundings (input rows, hidden rows, output); Cin = 320 (stage 0: 256 + 64) and 512,
    a channel-sliced output, row counts that do not fill the last 32-row tile, fewer tiles than workgroups."""
    net = build_net(seed=0)
    sd = net.state_dict()
    pfx = "refine_net.%d.pre_graph_module." % stage
    w = [sd[pfx + "%d.weight" % j].float() for j in (0, 2)]
    b = [sd[pfx + "%d.bias" % j].float() for j in (0, 2)]
    Cin = w[0].shape[1]
    assert Cin == (320 if stage == 0 else 512)
    x = rnd(det_tensor("mlpp%d_%d" % (B, N), (B, N, Cin)), CP_BF16)
    h1 = rnd(F.leaky_relu(x @ rnd(w[0], CP_BF16).t() + b[0], 0.01), CP_BF16)
    ref = F.leaky_relu(h1 @ rnd(w[1], CP_BF16).t() + b[1], 0.01)          # (B, N, 256)
    xin = x.to(torch.bfloat16).to(dev())
    pk = []
    for wi, ci in zip(w, (Cin, 256)):
        buf = torch.empty(lib.cp_packed_gemm_weight_bytes(CP_BF16, 256, ci), dtype=torch.uint8, device=dev())
        wd = wi.contiguous().to(dev())
        _abi.check(lib.cp_pack_gemm_weight(st(), CP_BF16, wd.data_ptr(), 256, ci, ci, buf.data_ptr()))
        pk.append(buf)
    bd = [t.contiguous().to(dev()) for t in b]
    wide = torch.full((B, N, 320), 7.0, dtype=torch.bfloat16, device=dev())
    _abi.check(lib.cp_mlp_pair_fused(st(), xin.data_ptr(), Cin, 0, Cin, B, N, pk[0].data_ptr(), bd[0].data_ptr(), 0.01,
                                     pk[1].data_ptr(), bd[1].data_ptr(), 0.01, wide.data_ptr(), 320, 64))
    torch.cuda.synchronize()
    got = wide.float().cpu()
    assert float((got[..., :64] - 7.0).abs().max()) == 0.0               # channels outside the slice untouched
    close(got[..., 64:], ref, 2e-2)                                      # bf16 output rounding + one-ulp hidden flips


@pytest.mark.parametrize("Cin", [64, 128, 256, 384])
def test_mlp_pair_fused_every_instance(lib, Cin):
    """cp_mlp_pair_fused through the C ABI at the input widths the model never uses: Cin = 64 / 128 (used to size the LDS for 16
    pieces under a kernel<4> launch: out-of-bounds LDS, silently wrong -- now kernel<2> with zero-weight padding chunks), 256
    (kernel<2>, full) and 384 (kernel<3>); same torch reference as above.  Unsupported widths are refused."""
    B, N = 2, 200
    w = [det_tensor("mpi_w1_%d" % Cin, (256, Cin), (6.0 / Cin) ** 0.5), det_tensor("mpi_w2", (256, 256), (6.0 / 256) ** 0.5)]
    b = [det_tensor("mpi_b1", (256,), 0.1), det_tensor("mpi_b2", (256,), 0.1)]
    x = rnd(det_tensor("mpi_x%d" % Cin, (B, N, Cin)), CP_BF16)
    h1 = rnd(F.leaky_relu(x @ rnd(w[0], CP_BF16).t() + b[0], 0.01), CP_BF16)
    ref = F.leaky_relu(h1 @ rnd(w[1], CP_BF16).t() + b[1], 0.01)
    assert lib.cp_mlp_pair_fused_supported(Cin, 256, 256) == 1
    assert lib.cp_mlp_pair_fused_supported(48, 256, 256) == 0 and lib.cp_mlp_pair_fused_supported(Cin, 128, 256) == 0
    xin = x.to(torch.bfloat16).to(dev())
    pk = []
    for wi, ci in zip(w, (Cin, 256)):
        buf = torch.empty(lib.cp_packed_gemm_weight_bytes(CP_BF16, 256, ci), dtype=torch.uint8, device=dev())
        wd = wi.contiguous().to(dev())
        _abi.check(lib.cp_pack_gemm_weight(st(), CP_BF16, wd.data_ptr(), 256, ci, ci, buf.data_ptr()))
        pk.append(buf)
    bd = [t.contiguous().to(dev()) for t in b]
    out = torch.full((B, N, 256), 7.0, dtype=torch.bfloat16, device=dev())
    _abi.check(lib.cp_mlp_pair_fused(st(), xin.data_ptr(), Cin, 0, Cin, B, N, pk[0].data_ptr(), bd[0].data_ptr(), 0.01,
                                     pk[1].data_ptr(), bd[1].data_ptr(), 0.01, out.data_ptr(), 256, 0))
    torch.cuda.synchronize()
    close(out.float().cpu(), ref, 2e-2)
    assert lib.cp_mlp_pair_fused(st(), xin.data_ptr(), 48, 0, 48, B, N, pk[0].data_ptr(), bd[0].data_ptr(), 0.01,
                                 pk[1].data_ptr(), bd[1].data_ptr(), 0.01, out.data_ptr(), 256, 0) == -1


@pytest.mark.parametrize("B,N,H,Cg", [(3, 512, 16, 64), (2, 1024, 32, 256), (1, 4096, 64, 256), (5, 64, 16, 128)])
def test_mlp_pair_fused_gather_equals_gather_then_pair(lib, B, N, H, Cg):
    """cp_mlp_pair_fused_gather (Index2Feat_module's 4-tap gather x RoI bit, pipeline.py:156-163,280, done by the fused pair's DMA
    loader: the (B, N, 256) local-feature tensor never exists) == cp_index2feat_gather into the concat buffer followed by
    cp_mlp_pair_fused, BIT FOR BIT (same rows reach the same MFMAs), and both == torch within the bf16 bounds.  Border ids (0 and
    H/2 - 1: taps on the map's last row / column), masked rows, a channel-sliced patch map, row counts that leave the last tile
    ragged."""
    k, E = 2, 64
    Hp = H + 1
    Cin = 256 + Cg
    pm = torch.full((B, Hp, Hp, 96), 3.0, dtype=torch.bfloat16, device=dev())         # patch map: channels [16, 80) of a wider tensor
    pm[..., 16:80] = det_tensor("pgm%d" % H, (B, Hp, Hp, E)).to(torch.bfloat16).to(dev())
    xid = torch.from_numpy(((np.arange(B * N).reshape(B, N) * 7 + 3) % (H // 2)).astype(np.int32))
    yid = torch.from_numpy(((np.arange(B * N).reshape(B, N) * 5 + 1) % (H // 2)).astype(np.int32))
    xid[:, :4] = torch.tensor([0, H // 2 - 1, 0, H // 2 - 1], dtype=torch.int32)
    yid[:, :4] = torch.tensor([0, 0, H // 2 - 1, H // 2 - 1], dtype=torch.int32)
    mask = (det_tensor("pgmask", (B, N)) > -0.4).float()
    assert 0.1 < float(mask.mean()) < 0.9
    cat = torch.zeros(B, N, Cin, dtype=torch.bfloat16, device=dev())                  # [local 256 | graph Cg]
    cat[..., 256:] = det_tensor("pgg%d" % Cg, (B, N, Cg)).to(torch.bfloat16).to(dev())
    w = [det_tensor("pg_w1_%d" % Cin, (256, Cin), (6.0 / Cin) ** 0.5), det_tensor("pg_w2", (256, 256), (6.0 / 256) ** 0.5)]
    b = [det_tensor("pg_b1", (256,), 0.1), det_tensor("pg_b2", (256,), 0.1)]
    pk = []
    for wi, ci in zip(w, (Cin, 256)):
        buf = torch.empty(lib.cp_packed_gemm_weight_bytes(CP_BF16, 256, ci), dtype=torch.uint8, device=dev())
        wd = wi.contiguous().to(dev())
        _abi.check(lib.cp_pack_gemm_weight(st(), CP_BF16, wd.data_ptr(), 256, ci, ci, buf.data_ptr()))
        pk.append(buf)
    bd = [t.contiguous().to(dev()) for t in b]
    xd, yd, md = xid.to(dev()), yid.to(dev()), mask.to(dev())
    # (a) the two-launch form: gather into the concat buffer, then the pair
    pmc = pm[..., 16:80].contiguous()
    _abi.check(lib.cp_index2feat_gather(st(), CP_BF16, pmc.data_ptr(), xd.data_ptr(), yd.data_ptr(), md.data_ptr(), cat.data_ptr(), B, N, Hp, Hp,
                                        E, k, Cin, 0))
    two = torch.full((B, N, 256), 7.0, dtype=torch.bfloat16, device=dev())
    _abi.check(lib.cp_mlp_pair_fused(st(), cat.data_ptr(), Cin, 0, Cin, B, N, pk[0].data_ptr(), bd[0].data_ptr(), 0.01,
                                     pk[1].data_ptr(), bd[1].data_ptr(), 0.01, two.data_ptr(), 256, 0))
    # (b) one launch: the local part of `cat` is poisoned to prove it is never read
    cat2 = cat.clone()
    cat2[..., :256] = float("nan")
    g = _abi.CpI2fGather()
    zeros = torch.zeros(256, dtype=torch.uint8, device=dev())
    g.patches, g.x_id, g.y_id, g.mask, g.zeros = pm.data_ptr(), xd.data_ptr(), yd.data_ptr(), md.data_ptr(), zeros.data_ptr()
    g.p_cstride, g.p_coff, g.Hp, g.Wp, g.k = 96, 16, Hp, Hp, k
    assert lib.cp_mlp_pair_fused_gather_supported(Cg, E, k) == 1
    one = torch.full((B, N, 320), 7.0, dtype=torch.bfloat16, device=dev())
    _abi.check(lib.cp_mlp_pair_fused_gather(st(), C.byref(g), cat2.data_ptr(), Cin, 256, Cg, B, N, pk[0].data_ptr(), bd[0].data_ptr(), 0.01,
                                            pk[1].data_ptr(), bd[1].data_ptr(), 0.01, one.data_ptr(), 320, 64))
    torch.cuda.synchronize()
    assert float((one[..., :64].float() - 7.0).abs().max()) == 0.0
    assert torch.equal(one[..., 64:], two)
    # torch reference of the whole span
    pmf = pm[..., 16:80].float().cpu()
    bi = torch.arange(B)[:, None].expand(B, N)
    taps = [pmf[bi, 2 * yid.long() + dy, 2 * xid.long() + dx] for dy, dx in ((0, 0), (k, 0), (0, k), (k, k))]     # sf1..sf4 (B, N, 64)
    x = torch.cat([torch.cat(taps, -1) * mask[..., None], cat[..., 256:].float().cpu()], -1)
    h1 = rnd(F.leaky_relu(x @ rnd(w[0], CP_BF16).t() + b[0], 0.01), CP_BF16)
    ref = F.leaky_relu(h1 @ rnd(w[1], CP_BF16).t() + b[1], 0.01)
    close(one[..., 64:].float().cpu(), ref, 2e-2)
    assert lib.cp_mlp_pair_fused_gather(st(), C.byref(g), cat2.data_ptr(), Cin, 256, Cg, B, 100, pk[0].data_ptr(), bd[0].data_ptr(), 0.01,
                                        pk[1].data_ptr(), bd[1].data_ptr(), 0.01, one.data_ptr(), 320, 64) == -1      # N not a power of two


def test_edgeconv_per_sample_graphs_lm(lib):
    """LM twin: each sample gathers along its own object's graph (pipeline_lm.py:55-57), 1-based obj_ids."""
    B, N, K, Cc = 4, 512, 20, 64
    idx = O.knn(lm_p3d(512), K)                                    # (15, N, K)
    obj = torch.tensor([3, 15, 1, 9])
    pq = det_tensor("lmpq", (B, N, 2 * Cc))
    P, Q = pq[..., :Cc], pq[..., Cc:]
    gi = idx[obj - 1]                                              # (B,N,K)
    nb = torch.gather(P.unsqueeze(2).expand(B, N, K, Cc), 1, gi.unsqueeze(-1).expand(B, N, K, Cc))
    ref = F.leaky_relu(nb.max(dim=2)[0] + Q, 0.2)
    out = torch.empty(B, N, Cc, device=dev())
    pq_d, idx_d = pq.to(dev()), idx.to(torch.int32).contiguous().to(dev())
    gids = (obj - 1).to(torch.int32).to(dev())
    _abi.check(lib.cp_edgeconv_gather_max(st(), CP_F32, pq_d.data_ptr(), idx_d.data_ptr(), gids.data_ptr(), out.data_ptr(),
                                          B, N, K, Cc, 15, Cc, 0, 0.2))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)                              # pure gather/max/add: bit exact


@pytest.mark.parametrize("H", [16, 32, 64])
def test_index2feat_gather_vs_golden(lib, H):
    """4-tap local feature gather incl. border ids, against the REFERENCE module's golden output."""
    g = golden("blk_index2feat_h%d" % H)
    i = {16: 0, 32: 1, 64: 2}[H]
    net = build_net(seed=0)
    sd = net.state_dict()
    B, N = 2, 512
    f = det_tensor("i2f%d" % H, (B, 256, H, H))
    w = sd["refine_net.%d.local_feat_ext_block.patch_generator.weight" % i]
    bias = sd["refine_net.%d.local_feat_ext_block.patch_generator.bias" % i]
    patches = run_conv(lib, CP_F32, f, w, torch.ones(64), bias, 1, 1)          # (B,64,H+1,W+1)
    p_cl = patches.permute(0, 2, 3, 1).contiguous().to(dev())
    xid = torch.from_numpy(g["xid"].astype(np.int32)).to(dev()); yid = torch.from_numpy(g["yid"].astype(np.int32)).to(dev())
    mask = torch.ones(B, N, device=dev())
    out = torch.zeros(B, N, 320, device=dev())
    _abi.check(lib.cp_index2feat_gather(st(), CP_F32, p_cl.data_ptr(), xid.data_ptr(), yid.data_ptr(), mask.data_ptr(),
                                        out.data_ptr(), B, N, H + 1, H + 1, 64, 2, 320, 0))
    torch.cuda.synchronize()
    got = out[..., :256].cpu().permute(0, 2, 1)
    close(got[:, :, ::4], torch.from_numpy(g["out"]), 2e-5)
    assert float(out[..., 256:].abs().max()) == 0.0
    mask0 = torch.zeros(B, N, device=dev())                       # RoI mask multiply (pipeline.py:280)
    _abi.check(lib.cp_index2feat_gather(st(), CP_F32, p_cl.data_ptr(), xid.data_ptr(), yid.data_ptr(), mask0.data_ptr(),
                                        out.data_ptr(), B, N, H + 1, H + 1, 64, 2, 320, 0))
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


def test_index2feat_conv_gathered_vs_golden(lib):
    """cp_index2feat_conv (patch conv evaluated only at the gathered taps + RoI mask, bf16) against the REFERENCE
    Index2Feat_module's golden output at the 64 x 64 stage incl. border ids (taps that read the conv's zero padding), a
    channel-sliced output and a masked-out keypoint."""
    H = 64
    g = golden("blk_index2feat_h%d" % H)
    net = build_net(seed=0)
    sd = net.state_dict()
    B, N = 2, 512
    f = det_tensor("i2f%d" % H, (B, 256, H, H))
    w = sd["refine_net.2.local_feat_ext_block.patch_generator.weight"]
    bias = sd["refine_net.2.local_feat_ext_block.patch_generator.bias"]
    assert lib.cp_index2feat_conv_supported(256, 64, 2) == 1
    d = dev()
    pw = torch.empty(lib.cp_index2feat_conv_weight_bytes(), dtype=torch.uint8, device=d)
    wd = w.contiguous().to(d)
    _abi.check(lib.cp_pack_index2feat_conv_weight(st(), wd.data_ptr(), pw.data_ptr()))
    fin = to_cl(f, CP_BF16)
    xid = torch.from_numpy(g["xid"].astype(np.int32)).to(d); yid = torch.from_numpy(g["yid"].astype(np.int32)).to(d)
    mask = torch.ones(B, N, device=d); mask[1, 8] = 0.0
    out = torch.full((B, N, 320), 5.0, dtype=torch.bfloat16, device=d)
    bd = bias.contiguous().to(d)
    _abi.check(lib.cp_index2feat_conv(st(), fin.data_ptr(), 256, 0, pw.data_ptr(), bd.data_ptr(), xid.data_ptr(), yid.data_ptr(),
                                      mask.data_ptr(), out.data_ptr(), B, N, H, H, 2, 320, 64), "index2feat conv")
    torch.cuda.synchronize()
    got = out[..., 64:].float().cpu().permute(0, 2, 1)                     # (B, 256, N)
    ref = torch.from_numpy(g["out"]).clone()                               # keypoints ::4 of the reference output
    assert float(got[1, :, 8].abs().max()) == 0.0                          # RoI mask
    ref[1, :, 2] = 0.0
    close(got[:, :, ::4], ref, 3e-2)
    assert float((out[..., :64].float() - 5.0).abs().max()) == 0.0         # channels outside the slice untouched


def test_bits_decode_exact(lib):
    B, N = 3, 700
    bits = det_tensor("bits", (B, 13, N))
    bits[0, 0, 0] = 0.0; bits[0, 1, 1] = 0.0; bits[0, 4, 2] = -0.0          # z == 0 -> bit 0 (pipeline.py:89-90)
    bd = bits.to(dev())
    mask = torch.empty(B, N, device=dev()); xid = torch.empty(B, N, dtype=torch.int32, device=dev()); yid = torch.empty_like(xid)
    x64 = torch.empty(B, N, dtype=torch.int64, device=dev()); y64 = torch.empty_like(x64)
    _abi.check(lib.cp_bits_decode(st(), bd.data_ptr(), -1, mask.data_ptr(), xid.data_ptr(), yid.data_ptr(), x64.data_ptr(), y64.data_ptr(), B, N))
    rx, ry = O.id_from_code_prob(bits[:, 1:4]), O.id_from_code_prob(bits[:, 7:10])
    assert torch.equal(mask.cpu(), O.mask_from_prob(bits[:, 0:1])[:, 0]) and torch.equal(x64.cpu(), rx) and torch.equal(y64.cpu(), ry)
    for s in range(3):
        _abi.check(lib.cp_bits_decode(st(), bd.data_ptr(), s, mask.data_ptr(), xid.data_ptr(), yid.data_ptr(), x64.data_ptr(), y64.data_ptr(), B, N))
        rx = rx * 2 + O.id_from_bit_prob(bits[:, 4 + s:5 + s]); ry = ry * 2 + O.id_from_bit_prob(bits[:, 10 + s:11 + s])
        assert torch.equal(x64.cpu(), rx) and torch.equal(y64.cpu(), ry) and torch.equal(xid.cpu().long(), rx)
    assert torch.equal(x64.cpu(), O.id_from_code_prob(bits[:, 1:7]))         # == MSB-first decode of all 6 bits


def test_bits_decode_sigmoid_threshold_sweep(lib):
    """Index work is bit exact: the reference thresholds sigmoid(z) > 0.5 in fp32, which is false for 0 < z <= 1.5 * 2^-24.
    Logits around that edge (and subnormals, +-0) decoded on the device == the REFERENCE's from_mask_prob_to_mask /
    from_code_prob_to_id / from_bit_prob_to_id outputs (tests/golden/sigmoid_threshold.npz)."""
    g = golden("sigmoid_threshold")
    z = torch.from_numpy(g["z_bits"]).view(torch.float32)
    n = z.numel()
    bits = torch.zeros(1, 13, n)
    bits[0, 0] = z
    bits[0, 1], bits[0, 2], bits[0, 3] = z, z.flip(0), z.roll(7)              # the fixture's 3-bit code rows
    bits[0, 7], bits[0, 8], bits[0, 9] = z.roll(7), z, z.flip(0)
    for s in range(3):
        bits[0, 4 + s] = z.roll(s)
        bits[0, 10 + s] = z.flip(0).roll(s)
    bd = bits.to(dev())
    mask = torch.empty(1, n, device=dev()); xid = torch.empty(1, n, dtype=torch.int32, device=dev()); yid = torch.empty_like(xid)
    x64 = torch.empty(1, n, dtype=torch.int64, device=dev()); y64 = torch.empty_like(x64)
    _abi.check(lib.cp_bits_decode(st(), bd.data_ptr(), -1, mask.data_ptr(), xid.data_ptr(), yid.data_ptr(), x64.data_ptr(), y64.data_ptr(), 1, n))
    assert np.array_equal(mask.cpu().numpy().astype(np.uint8), g["mask"].reshape(1, n))
    assert np.array_equal(x64.cpu().numpy(), g["ids3"].astype(np.int64))
    bit = torch.from_numpy(g["bit"].astype(np.int64)).view(-1)               # reference from_bit_prob_to_id(z)
    m = torch.from_numpy(g["mask"].astype(np.int64)).view(-1)
    assert np.array_equal(y64.cpu().numpy()[0], (4 * m.roll(7) + 2 * m + m.flip(0)).numpy())
    rx, ry = x64.cpu()[0].clone(), y64.cpu()[0].clone()
    for s in range(3):
        _abi.check(lib.cp_bits_decode(st(), bd.data_ptr(), s, mask.data_ptr(), xid.data_ptr(), yid.data_ptr(), x64.data_ptr(), y64.data_ptr(), 1, n))
        rx = 2 * rx + bit.roll(s); ry = 2 * ry + bit.flip(0).roll(s)
        assert torch.equal(x64.cpu()[0], rx) and torch.equal(y64.cpu()[0], ry)


# ------------------------------------------------------------------------------------------- end to end
def _cmp_e2e(out, ref, tol=1e-4, margin=None):
    names = ("roi", "xb", "yb", "seg")
    worst = 0.0
    for a, b, n in zip(out[:4], ref[:4], names):
        b = b if torch.is_tensor(b) else torch.from_numpy(np.asarray(b))
        assert tuple(a.shape) == tuple(b.shape), n
        worst = max(worst, float((a.float().cpu() - b).abs().max()))
    assert worst <= tol, "max |logit - ref| = %.3e" % worst
    for a, b in zip(out[4:], ref[4:]):
        b = b if torch.is_tensor(b) else torch.from_numpy(np.asarray(b).astype(np.int64))
        assert a.dtype == torch.int64 and torch.equal(a.cpu(), b)
    return worst


def _oracle_replayer(net, img, knn_idx, npoint, kw, inter=None):
    """oracle_forward(forced) of tests/free_running.py for a case: call it BEFORE net.to(dev()) (the state dict is cloned on the
    CPU).  `inter` (the intermediates of the case's free oracle run) lends its backbone features, which no decision reaches."""
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    feats = None if inter is None else inter["img_feats"]
    return lambda forced: O.posenet_forward(sd, img, knn_idx, npoint, forced=forced, img_feats=feats, **kw)


def _free_running_both_selections(net, run, oracle_forward, ref, label):
    """The free-running forward `run()` on the fp32 path under both kernel selections, each against the oracle replaying THAT run's
    own decisions (tests/free_running.py): every logit of every keypoint within 1e-4, final ids == the run's own logits decoded.
    No margin condition: where the run took the free reference's decisions this is _cmp_e2e(run(), ref)."""
    stats = {}
    for sel in ("auto", "per_crop"):
        net.set_kernel_selection(sel)
        stats[sel] = FR.assert_free_running_parity(run(), oracle_forward, ref_free=ref, tol=1e-4, label="%s [%s]" % (label, sel))
        assert stats[sel]["keypoints_compared"] == ref[0].shape[0] * ref[0].shape[2]
    net.set_kernel_selection("auto")
    return stats


def _bf16_replay_floors(out, oracle_forward, ref, label):
    """bf16 free-running run against the fp32 oracle replaying the bf16 run's OWN decisions: what is left is arithmetic error under
    given decisions, i.e. what the contract's TEACHER-FORCED floors bound (mean |dlogit| <= 2 % of the logit
    RMS, max <= 0.5, seg agreement >= 99 %) -- the same numbers, unchanged; and the ids the run returns are its own logits decoded."""
    from checkerpose_amd.agreement import logit_agreement
    FR.assert_ids_match_own_logits(out)
    _, ref_f, st = FR.replay(out, oracle_forward, ref_free=ref)
    rp = logit_agreement(out, ref_f)
    print("bf16 replay %s: mean |dlogit| / rms %.5f, max |dlogit| %.4f, seg agreement %.5f, decisions differing from the free oracle run %s"
          % (label, rp["mean_abs_dlogit_over_rms"], rp["max_abs_dlogit"], rp["seg_agreement"], st["decisions_differing_from_free_ref"]))
    assert rp["mean_abs_dlogit_over_rms"] <= 0.02 and rp["max_abs_dlogit"] <= 0.5 and rp["seg_agreement"] >= 0.99, (label, rp)
    return rp


def test_e2e_fp32_vs_golden_hrnet_and_oracle(lib):
    """Full PoseNet_GNNskip (HRNet-W18 + decoder + 3 refine stages), fp32 path, B=1, LM-O ape N=512: against the
    golden 6-tuple (reference head on the oracle backbone) AND a live oracle run; also InitNet_GNN alone (config #1)."""
    g = golden("e2e_hrnet")
    net = build_net(seed=int(g["seed"]), overrides=g)
    img = det_image(1)
    ref, _ = O.posenet_forward(net.state_dict(), img, net.init_net.knn_idx, 512, **oracle_kwargs())
    net = net.to(dev())
    out = net(img.to(dev()), ape_p3d(512).to(dev()).expand(1, -1, -1))
    w_o = _cmp_e2e(out, ref)
    # HIP vs the REFERENCE-made golden directly (north_star's tolerance is HIP <-> reference, not via the oracle)
    w_g = _cmp_e2e(out, (g["roi"], g["xb"], g["yb"], g["seg"], g["xid"], g["yid"]), tol=1e-4)
    print("e2e_hrnet: max |HIP - oracle| = %.3e, max |HIP - reference golden| = %.3e" % (w_o, w_g))
    o2 = net(img.to(dev()), None)                       # second call = hipGraph replay; must be identical
    for a, b in zip(out, o2):
        assert torch.equal(a, b)
    init_out = net.init_net(img.to(dev()))
    assert tuple(init_out.shape) == (1, 7, 512)
    assert float((init_out.cpu() - torch.from_numpy(g["init_out"])).abs().max()) <= 1e-4
    o3, feats, gf = net.init_net(img.to(dev()), return_graph_feats=True)
    assert [tuple(f.shape[1:]) for f in feats] == [(128, 64, 64), (256, 32, 32), (512, 16, 16), (1024, 8, 8)]
    assert tuple(gf.shape) == (1, 64, 512) and torch.equal(o3, init_out)
    # the returned features themselves (all four incre modules are live when they are asked for; without return_img_feats the
    # launch program drops the highest-resolution one, which nothing reads)
    sdi = {k[len("init_net."):]: v for k, v in net.state_dict().items() if k.startswith("init_net.")}
    _, rfeats, rg = O.init_net_forward({k: v.cpu() for k, v in sdi.items()}, "", img, net.init_net.knn_idx.cpu(), 512)
    for f, r in zip(feats, rfeats):
        close(f.cpu(), r, 1e-4)
    close(gf.cpu(), rg, 1e-4)


@pytest.mark.parametrize("name,npoint,lm,fseed,B", [("e2e_injected", 512, False, 0, 2), ("e2e_lm_injected", 512, True, 1, 3),
                                                   ("e2e_lm4096_injected", 4096, True, 2, 2)])
def test_e2e_head_vs_reference_golden_direct(lib, name, npoint, lm, fseed, B):
    """The whole head (conv1x1 .. EdgeConv .. decoder .. 3 refinement stages .. seg) on the HIP fp32 path against the 6-tuples the
    REFERENCE's own PoseNet_GNNskip produced (tests/golden/make_golden*.py: backbone features injected through a timm stub,
    here through forward_injected_feats) -- no oracle in between: logits within 1e-4, ids bit-exact.  Covers config #2's head,
    the LM twin with per-sample graphs and config #5 (LM x 4096 keypoints)."""
    g = golden(name)
    net = build_net(npoint=npoint, seed=int(g["seed"]), lm=lm, overrides=g).to(dev())
    feats = [f.to(dev()) for f in inject_feats(B, seed=fseed)]
    obj = torch.from_numpy(g["obj_ids"]).to(dev()) if lm else None
    img = torch.zeros(B, 3, 256, 256, device=dev())
    out = net.forward_injected_feats(img, feats, obj_ids=obj)
    w = _cmp_e2e(out, (g["roi"], g["xb"], g["yb"], g["seg"], g["xid"], g["yid"]), tol=1e-4)
    print("%s: max |HIP - reference golden| = %.3e (decision margin of the fixture %.2e)" % (name, w, float(g["margin"])))
    again = net.forward_injected_feats(img, feats, obj_ids=obj)          # hipGraph replay
    for a, b in zip(out, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["res4", "conv2", "lm_res4"])
def test_initnet_variants_vs_reference_golden(lib, name):
    """InitNet_GNN(res_log2=4) -> (B,9,N) and InitNet_GNN(num_conv1x1=2) (init.py:78,83-95), and the LM twin with res_log2 = 4
    (init_lm.py:72-128): HIP fp32 on the full backbone vs the oracle, and the head alone vs the REFERENCE's output through injected
    features (initnet_variants.npz)."""
    from tests.test_oracle import build_init_variant
    g = golden("initnet_variants")
    net = build_init_variant(name)
    img = det_image(2, seed=17)
    lm = name.startswith("lm_")
    obj = torch.from_numpy(g["lm_res4_obj_ids"]) if lm else None
    ref, _, _ = O.init_net_forward(net.state_dict(), "", img, net.knn_idx[obj - 1] if lm else net.knn_idx, 512)
    net = net.to(dev())
    out = net(img.to(dev()), obj.to(dev())) if lm else net(img.to(dev()))
    assert tuple(out.shape) == tuple(ref.shape) == (2, net.num_out_bits, 512)
    assert float((out.cpu() - ref).abs().max()) <= 1e-4
    res = net._run(img.to(dev()), obj.to(dev()) if lm else None, inject_feats=[f.to(dev()) for f in inject_feats(2, seed=4)])
    bits = res["bits"]
    o2 = torch.cat([bits[:, 0:4], bits[:, 7:10]], 1) if net.res_log2 == 3 else bits[:, :net.num_out_bits]
    assert float((o2.cpu() - torch.from_numpy(g[name + "_out"])).abs().max()) <= 1e-4


def test_e2e_fp32_batch_ragged_and_stage_truncation(lib):
    net = build_net(seed=1)
    img = det_image(3, seed=5)
    sd = net.state_dict()
    ref, inter = O.posenet_forward(sd, img, net.init_net.knn_idx, 512, **oracle_kwargs())
    ref1, _ = O.posenet_forward(sd, img, net.init_net.knn_idx, 512, stage=1, **oracle_kwargs())
    replay = _oracle_replayer(net, img, net.init_net.knn_idx, 512, oracle_kwargs(), inter)
    replay1 = _oracle_replayer(net, img, net.init_net.knn_idx, 512, dict(oracle_kwargs(), stage=1), inter)
    net = net.to(dev())
    eager = net(img.to(dev()), None)                     # 1st call: sequential eager replay (program order)
    _cmp_e2e(eager, ref)
    for _ in range(4):                                   # 2nd..: hipGraph with parallel lanes (HRNet branches,
        again = net(img.to(dev()), None)                 # decoder || refinement) must reproduce it bit for bit
        for a, b in zip(eager, again):
            assert torch.equal(a, b)
    out1 = net(img.to(dev()), None, stage=1)
    assert tuple(out1[1].shape) == (3, 4, 512) and tuple(out1[3].shape) == (3, 2, 16, 16)
    _cmp_e2e(out1, ref1)
    _free_running_both_selections(net, lambda: net(img.to(dev()), None), replay, ref, "ragged B=3")
    _free_running_both_selections(net, lambda: net(img.to(dev()), None, stage=1), replay1, ref1, "ragged B=3 stage=1")


def test_e2e_lm_per_object_graphs_vs_golden(lib):
    g = golden("e2e_lm_injected")   # head only (features injected) -> compare the full net against the live oracle instead,
    net = build_net(seed=int(g["seed"]), lm=True, overrides=g)               # and the golden pins the oracle (tests/test_oracle.py)
    obj = torch.tensor([1, 9, 15, 9])
    img = det_image(4, seed=2)
    ref, _ = O.posenet_forward(net.state_dict(), img, net.init_net.knn_idx[obj - 1], 512, **oracle_kwargs())
    net = net.to(dev())
    out = net(img.to(dev()), None, obj.to(dev()))
    _cmp_e2e(out, ref)


def test_e2e_n4096_dense_keypoints(lib):
    """config #5 shape class: N=4096 keypoints (stress of the gather), B=1, fp32."""
    net = build_net(npoint=4096, seed=3)
    img = det_image(1, seed=7)
    ref, inter = O.posenet_forward(net.state_dict(), img, net.init_net.knn_idx, 4096, **oracle_kwargs())
    replay = _oracle_replayer(net, img, net.init_net.knn_idx, 4096, oracle_kwargs(), inter)
    net = net.to(dev())
    _cmp_e2e(net(img.to(dev()), None), ref)
    _free_running_both_selections(net, lambda: net(img.to(dev()), None), replay, ref, "N=4096 dense")


_ORACLE_CACHE = {}


def _lm4096_case():
    """config #5's full-network case (LM twin, 4096 keypoints, seed 2, objects LM_OBJ_IDS[3] / [11]) and its CPU-oracle forward,
    computed once per session (the oracle takes ~10 s)"""
    if "lm4096" not in _ORACLE_CACHE:
        from tests.common import LM_OBJ_IDS
        obj = torch.tensor([LM_OBJ_IDS[3], LM_OBJ_IDS[11]])
        net = build_net(npoint=4096, seed=2, lm=True)                 # seed with a mixed RoI bit (47 %), margin 5.6e-5
        img = det_image(2, seed=32)
        ref, inter = O.posenet_forward(net.state_dict(), img, net.init_net.knn_idx[obj - 1], 4096, **oracle_kwargs())
        replay = _oracle_replayer(net, img, net.init_net.knn_idx[obj - 1], 4096, oracle_kwargs(), inter)
        _ORACLE_CACHE["lm4096"] = (obj, replay, img, ref)
    obj, replay, img, ref = _ORACLE_CACHE["lm4096"]
    net = build_net(npoint=4096, seed=2, lm=True)
    return obj, net, img, ref


def _lm4096_replayer():
    """oracle_forward(forced) of _lm4096_case() (tests/free_running.py)"""
    _lm4096_case()
    return _ORACLE_CACHE["lm4096"][1]


def _lm4096_golden_case():
    """config #5's REFERENCE-made case: the head (everything the reference's own code pins) on injected backbone features with the
    repaired weights of `e2e_lm4096_injected` (every one of its 13 x B x 4096 logits >= 1e-3 from zero, tests/golden/make_golden.py:
    center_and_repair) -- the 6-tuple the reference's PoseNet_GNNskip_LM produced is the comparison target, no oracle in between.
    -> (obj_ids, net, feats, ref 6-tuple of CPU tensors)"""
    g = golden("e2e_lm4096_injected")
    net = build_net(npoint=4096, seed=int(g["seed"]), lm=True, overrides=g)
    feats = inject_feats(2, seed=2)
    obj = torch.from_numpy(g["obj_ids"])
    ref = tuple(torch.from_numpy(g[k]) for k in ("roi", "xb", "yb", "seg", "xid", "yid"))
    assert float(g["margin"]) >= 5e-4
    return obj, net, feats, ref


def _teacher_bits(ref):
    B, N = ref[0].shape[0], ref[0].shape[2]
    t = torch.zeros(B, 13, N)
    t[:, 0:1], t[:, 1:7], t[:, 7:13] = ref[0], ref[1], ref[2]
    return t


def test_e2e_lm13_n4096_config5(lib):
    """BASELINE config #5 as a COMBINATION: the LM shared estimator (per-sample graphs `knn_idx[obj_ids-1]`,
    pipeline_lm.py:392-425) at npt=4096 dense keypoints, obj_ids from the 13 evaluated LM objects
    (test_network_with_test_data.py:533), fp32 path vs the oracle (pinned for this config by knn_lm4096 +
    e2e_lm4096_injected).  Teacher-forced per stage, and free-running by decision replay: this seed's smallest decision margin
    (5.6e-5) is BELOW the 1e-4 tolerance, so a legitimate fp32 difference may flip that decision and everything downstream of it --
    the oracle replays the decisions the device took, and all 2 x 4096 keypoints are compared (both kernel selections).
    (The reference-pinned free-running check of config #5 at a 1e-3 margin is test_e2e_head_vs_reference_golden_direct.)"""
    obj, net, img, ref = _lm4096_case()
    replay = _lm4096_replayer()
    z = torch.cat([ref[0], ref[1][:, :-1], ref[2][:, :-1]], 1)
    margin = float(z.abs().min())
    net = net.to(dev())
    out_t = net.forward_teacher_forced(img.to(dev()), _teacher_bits(ref).to(dev()), obj_ids=obj.to(dev()))
    _cmp_e2e(out_t, ref)
    out = net(img.to(dev()), None, obj.to(dev()))
    print("config #5 full net: decision margin of the free oracle run %.2e" % margin)
    _free_running_both_selections(net, lambda: net(img.to(dev()), None, obj.to(dev())), replay, ref, "config #5 LM N=4096")
    assert tuple(out[1].shape) == (2, 6, 4096) and out[4].dtype == torch.int64


@pytest.mark.parametrize("chain", [False, True])
def test_e2e_bf16_accuracy_contract(lib, monkeypatch, chain):
    """bf16 path (BASELINE config #2, the path bench.py times): not a 1e-4 path -- its written contract
    (checkerpose_amd/agreement.py), checked against the CPU oracle at B=4 on random-init weights:
      teacher-forced (discrete feedback taken from the oracle, so one flipped bit cannot compound):
        every one of the 13 logit rows agrees on >= 98 % of the thresholded bits, both seg masks on >= 99 %,
        mean |dlogit| <= 2 % of the logit RMS, max |dlogit| <= 0.5;
      free-running (what a user sees; flips of an early bit change later stages' gather positions):
        roi + the 3+3 InitNet bits >= 98 %, every later row >= 95 %, final (x_id, y_id) pairs equal for >= 90 % of the
        keypoints, mean id error <= 0.5 px;
      free-running against the fp32 oracle REPLAYING the bf16 run's own decisions (arithmetic error under given decisions, over
        every keypoint): the teacher-forced floors on mean / max |dlogit| and seg, and final ids == the run's own logits decoded.
    (measured, round 2, vs the fp32 HIP path on 8 crops: teacher-forced min row 0.9895, mean |dlogit| 0.74 % of RMS,
    max 0.35; free-running min row 0.984, id pairs equal 96.2 %, 0.16 px)"""
    from checkerpose_amd import engine
    from checkerpose_amd.agreement import logit_agreement, margin_contract_violations
    # both kernel selections of the HRNet branches: per-conv launches (small batches) / one LDS-resident chain launch each
    monkeypatch.setattr(engine, "STEM_MIN_BATCH", 1 if chain else 1 << 30)
    monkeypatch.setattr(engine, "CHAIN_MIN_BATCH", 1 if chain else 1 << 30)
    monkeypatch.setattr(engine, "EDGE_FUSED_MIN_BATCH", 1 if chain else 1 << 30)
    monkeypatch.setattr(engine, "MLP_FUSED_MIN_ROWS", 1 if chain else 1 << 30)
    net = build_net(seed=1)
    img = det_image(4, seed=3)
    ref, inter = O.posenet_forward(net.state_dict(), img, net.init_net.knn_idx, 512, **oracle_kwargs())
    replay = _oracle_replayer(net, img, net.init_net.knn_idx, 512, oracle_kwargs(), inter)
    net = net.to(dev()).set_compute_dtype("bf16")
    tf = logit_agreement(net.forward_teacher_forced(img.to(dev()), _teacher_bits(ref).to(dev())), ref)
    out_fr = net(img.to(dev()), None)
    fr = logit_agreement(out_fr, ref, tau=tf["tau"], explain=True, knn_idx=net.init_net.knn_idx)
    _bf16_replay_floors(out_fr, replay, ref, "config #2 B=4 chain=%s" % chain)
    print("bf16 teacher-forced:", tf)
    print("bf16 free-running  :", fr)
    # margin-aware clauses: flips only at near-ties of the reference; free-running id mismatches trace back to such a flip
    assert margin_contract_violations(tf, fr) == [], (margin_contract_violations(tf, fr), tf, fr)
    assert tf["bit_agreement_min_row"] >= 0.98 and tf["seg_agreement"] >= 0.99, tf
    assert tf["mean_abs_dlogit_over_rms"] <= 0.02 and tf["max_abs_dlogit"] <= 0.5, tf
    rows = fr["bit_agreement_per_row"]
    for r in ("roi", "x5", "x4", "x3", "y5", "y4", "y3"):
        assert rows[r] >= 0.98, (r, rows[r])
    assert fr["bit_agreement_min_row"] >= 0.95 and fr["seg_agreement"] >= 0.99, fr
    assert fr["xy_id_equal"] >= 0.90 and fr["id_abs_err_mean_px"] <= 0.5, fr


@pytest.mark.parametrize("tiled", [False, True])
def test_e2e_bf16_accuracy_contract_n4096_lm(lib, monkeypatch, tiled):
    """The same written contract on BASELINE config #5 in the dtype `bench.py --workload lm13_n4096` times: LM shared estimator,
    per-sample graphs, npt=4096, bf16, against the CPU oracle (pinned for this config by knn_lm4096 + e2e_lm4096_injected; the
    reference-made fixture itself is the subject of test_bf16_on_the_centred_reference_fixture_n4096 below);
    both EdgeConv paths: node GEMM + L2 gather (small batches) and the patch-tiled LDS-staged launches (cp_edgeconv_tiled: the
    program then runs in the internal patch order, so this also covers the row renumbering and the un-permuted outputs)."""
    from checkerpose_amd import engine
    from checkerpose_amd.agreement import logit_agreement, margin_contract_violations
    from tests.common import LM_OBJ_IDS
    monkeypatch.setattr(engine, "EDGE_FUSED_MIN_BATCH", 1 if tiled else 1 << 30)
    monkeypatch.setattr(engine, "MLP_FUSED_MIN_ROWS", 1 if tiled else 1 << 30)
    obj, net, img, ref = _lm4096_case()     # (a statistical contract about near-ties: a small decision margin of the case is what it measures)
    net = net.to(dev()).set_compute_dtype("bf16")
    tf = logit_agreement(net.forward_teacher_forced(img.to(dev()), _teacher_bits(ref).to(dev()), obj_ids=obj.to(dev())), ref)
    out_fr = net(img.to(dev()), None, obj.to(dev()))
    fr = logit_agreement(out_fr, ref, tau=tf["tau"], explain=True, knn_idx=net.init_net.knn_idx, graph_ids=obj - 1)
    _bf16_replay_floors(out_fr, _lm4096_replayer(), ref, "config #5 LM N=4096 tiled=%s" % tiled)      # (see the B = 4 contract test)
    print("bf16 N=4096 LM teacher-forced:", tf)
    print("bf16 N=4096 LM free-running  :", fr)
    assert margin_contract_violations(tf, fr) == [], (margin_contract_violations(tf, fr), tf, fr)
    names = [c[2].split(":")[0] for pr in net._programs.values() for c in pr["prog"].calls]
    assert ("edge_tiled" in names) == tiled and ("edge_gather" in names) != tiled
    assert tf["bit_agreement_min_row"] >= 0.98 and tf["seg_agreement"] >= 0.99, tf
    assert tf["mean_abs_dlogit_over_rms"] <= 0.02 and tf["max_abs_dlogit"] <= 0.5, tf
    rows = fr["bit_agreement_per_row"]
    for r in ("roi", "x5", "x4", "x3", "y5", "y4", "y3"):
        assert rows[r] >= 0.98, (r, rows[r])
    assert fr["bit_agreement_min_row"] >= 0.95 and fr["seg_agreement"] >= 0.99, fr
    assert fr["xy_id_equal"] >= 0.90 and fr["id_abs_err_mean_px"] <= 0.5, fr


KNOWN_CENTRED_FIXTURE_VIOLATIONS = ("a flip at margin", "flips above tau", "start at the keypoint's own near-tie")


@pytest.mark.parametrize("tiled", [False, True])
def test_bf16_on_the_centred_reference_fixture_n4096(lib, monkeypatch, tiled):
    """config #5's REFERENCE-made 6-tuple (`e2e_lm4096_injected`: injected backbone features, weights repaired so that every logit is
    >= 1e-3 from zero -- the decision margin is above the fp32 tolerance) as the bf16 path's comparison target.  `center_and_repair`
    also CENTRES every logit row on zero (half / half over batch and keypoints): 18 % of the 106 496 decisions sit within 0.2 of the
    threshold at a logit RMS of 1.03 -- the right stress for the 1e-4 comparison (test_e2e_head_vs_reference_golden_direct), the
    densest possible population of near-ties for a statistical contract.  Asserted: everything the contract states as a floor or as a
    hard bound -- teacher-forced rows >= 98 %, seg >= 99 %, mean |dlogit| <= 2 % of the logit RMS (and <= 2.5 bf16 epsilons of it), max <=
    0.5, clause (a) (no flip at a margin >= max(0.2, 4 % of the RMS)); free-running rows >= 95 %, final id pairs >= 90 %, id error <= 0.5
    px, >= 95 % of the mismatches explained.  KNOWN violations on this fixture, listed not hidden: the tail clauses (b) / (c) (largest flip
    margin 8 x the mean error against 6 x) and the own-near-tie share of clause (d) (39-41 % against 60 %: with this many near-ties most
    mismatches are carried in from a neighbour's flip).  With the keypoint side in bf16 (round 5) the same fixture broke the FLOORS
    (mean error above the cap, id pairs 79-80 %)."""
    from checkerpose_amd import engine
    from checkerpose_amd.agreement import logit_agreement, margin_contract_violations
    monkeypatch.setattr(engine, "EDGE_FUSED_MIN_BATCH", 1 if tiled else 1 << 30)
    monkeypatch.setattr(engine, "MLP_FUSED_MIN_ROWS", 1 if tiled else 1 << 30)
    obj, net, feats, ref = _lm4096_golden_case()
    net = net.to(dev()).set_compute_dtype("bf16")
    img = torch.zeros(2, 3, 256, 256, device=dev())
    fd = [f.to(dev()) for f in feats]
    tf = logit_agreement(net.forward_injected_feats(img, fd, obj_ids=obj.to(dev()), teacher_bits=_teacher_bits(ref).to(dev())), ref)
    fr = logit_agreement(net.forward_injected_feats(img, fd, obj_ids=obj.to(dev())), ref, tau=tf["tau"], explain=True,
                         knn_idx=net.init_net.knn_idx, graph_ids=obj - 1)
    viol = margin_contract_violations(tf, fr)
    print("centred fixture, tiled %s: tf mean %.5f (%.4f of rms) max flip margin %.4f; fr id pairs %.4f; violations: %s"
          % (tiled, tf["mean_abs_dlogit"], tf["mean_abs_dlogit_over_rms"], tf["max_flip_margin"], fr["xy_id_equal"], viol))
    unknown = [v for v in viol if not any(k in v for k in KNOWN_CENTRED_FIXTURE_VIOLATIONS)]
    assert unknown == [], unknown                                           # hard clause (a), the mean-error cap, the explained share: hold
    assert tf["max_flip_margin"] < max(0.2, 0.04 * tf["logit_rms"]), tf
    assert tf["bit_agreement_min_row"] >= 0.98 and tf["seg_agreement"] >= 0.99, tf
    assert tf["mean_abs_dlogit_over_rms"] <= 0.02 and tf["max_abs_dlogit"] <= 0.5, tf
    assert fr["bit_agreement_min_row"] >= 0.95 and fr["seg_agreement"] >= 0.99, fr
    assert fr["xy_id_equal"] >= 0.90 and fr["id_abs_err_mean_px"] <= 0.5 and fr["id_mismatches_explained_frac"] >= 0.95, fr


def test_e2e_teacher_forced_per_stage(lib):
    """Per-stage parity with the discrete feedback forced to the oracle's decisions: every stage's logits must match
    even if an earlier near-zero logit would have flipped a bit."""
    net = build_net(seed=2)
    img = det_image(2, seed=11)
    ref, inter = O.posenet_forward(net.state_dict(), img, net.init_net.knn_idx, 512, **oracle_kwargs())
    tbits = torch.zeros(2, 13, 512)
    tbits[:, 0:1], tbits[:, 1:7], tbits[:, 7:13] = ref[0], ref[1], ref[2]
    # adversarial teacher: flip the sign of the 64 smallest-margin decision logits -> a different gather pattern
    flipped = tbits.clone()
    flat = flipped[:, [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11]].reshape(-1)
    idx = flat.abs().argsort()[:64]
    sel = flipped[:, [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11]].reshape(-1)
    sel[idx] = -sel[idx]
    flipped[:, [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11]] = sel.reshape(2, 11, 512)
    forced = {"roi": O.mask_from_prob(flipped[:, 0:1]),
              "x": [O.id_from_code_prob(flipped[:, 1:4 + i]) for i in range(3)],
              "y": [O.id_from_code_prob(flipped[:, 7:10 + i]) for i in range(3)]}
    ref_f, _ = O.posenet_forward(net.state_dict(), img, net.init_net.knn_idx, 512, forced=forced, **oracle_kwargs())
    net = net.to(dev())
    out = net.forward_teacher_forced(img.to(dev()), tbits.to(dev()))
    _cmp_e2e(out, ref)
    out_f = net.forward_teacher_forced(img.to(dev()), flipped.to(dev()))
    worst = max(float((a.cpu() - b).abs().max()) for a, b in zip(out_f[:4], ref_f[:4]))
    assert worst <= 1e-4, worst
    assert float((ref_f[1] - ref[1]).abs().max()) > 1e-3       # the flipped teacher really changed later stages


def test_e2e_resnet34_backbone(lib):
    """resnet34 backbone (config/lm/res34GNN2_res6_gnn3Skip_mlpQuery_lm.txt): 7x7 stem, max-pool, strided BasicBlocks."""
    net = build_net(seed=8, backbone="resnet34")   # seed with a mixed RoI bit (49 %) and margin 9e-4
    img = det_image(2, seed=9)
    kw = dict(oracle_kwargs(), backbone="resnet34")
    ref, inter = O.posenet_forward(net.state_dict(), img, net.init_net.knn_idx, 512, **kw)
    replay = _oracle_replayer(net, img, net.init_net.knn_idx, 512, kw, inter)
    net = net.to(dev())
    _cmp_e2e(net(img.to(dev()), None), ref)
    _free_running_both_selections(net, lambda: net(img.to(dev()), None), replay, ref, "resnet34")


@pytest.mark.parametrize("backbone", ["hrnet_w18_small", "hrnet_w30"])
def test_e2e_other_hrnet_backbones(lib, backbone):
    """The reference's other HRNet names (backbone.py:43, init.py:15-24; no shipped config uses them): hrnet_w18_small (one 32-plane
    Bottleneck in layer1, ONE module per stage, two BasicBlocks per branch, widths 16 / 32 / 64 / 128) and hrnet_w30 (hrnet_w18's
    layout at widths 30 / 60 / 120 / 240) -- timm's published layouts (checkerpose_amd/model/backbone.py: HRNET_CFGS; their parameter
    counts reproduce timm's model-zoo figures: tests/test_oracle.py), same "incre" heads, same four pyramid features.  fp32 <= 1e-4 vs
    the oracle (teacher-forced, and free-running by decision replay over every keypoint: hrnet_w18_small's smallest decision margin,
    8.8e-5, is below the tolerance), both through the per-crop and the per-conv launches; bf16 (keypoint side half): the
    teacher-forced floors of the contract."""
    from checkerpose_amd.agreement import logit_agreement
    net = build_net(seed=6, backbone=backbone)
    img = det_image(2, seed=11)
    kw = dict(oracle_kwargs(), backbone=backbone)
    ref, inter = O.posenet_forward(net.state_dict(), img, net.init_net.knn_idx, 512, **kw)
    replay = _oracle_replayer(net, img, net.init_net.knn_idx, 512, kw, inter)
    net = net.to(dev())
    tb = _teacher_bits(ref).to(dev())
    _cmp_e2e(net.forward_teacher_forced(img.to(dev()), tb), ref)
    _free_running_both_selections(net, lambda: net(img.to(dev()), None), replay, ref, backbone)
    net.set_kernel_selection("per_crop")                # the launches of the 256-crop step (fused stem, Bottleneck / chains where they fit)
    _cmp_e2e(net.forward_teacher_forced(img.to(dev()), tb), ref)
    net.set_kernel_selection("auto")
    net.set_compute_dtype("bf16")
    tf = logit_agreement(net.forward_teacher_forced(img.to(dev()), tb), ref)
    assert tf["bit_agreement_all_rows"] >= 0.99 and tf["bit_agreement_min_row"] >= 0.96 and tf["seg_agreement"] >= 0.99, (backbone, tf)
    assert tf["mean_abs_dlogit_over_rms"] <= 0.02 and tf["max_abs_dlogit"] <= 0.5, (backbone, tf)


@pytest.mark.parametrize("case", ["woEdgeConv", "woEdgeConv_lm", "stage1_without", "init_only"])
def test_e2e_without_graph_modules(lib, case):
    """`num_graph_module = 0` (shipped: config/lm/hr18GNN2_res6_gnn3Skip_mlpQuery_lm_woEdgeConv.txt -- init_network_num_graph_module = 0
    AND network_num_graph_module = 0 -- and config/lm/init_gnn0_hrnetw18_npt512_lm.txt): with an empty `pre_query_block` the
    reinterpreted conv1x1 rows are InitNet's graph feature (init.py:112-118) and a refinement stage's pre-graph MLP rows are the feature
    it hands to the next stage (pipeline.py:288-297).  The plain and the LM twin, a per-stage tuple with one empty stage
    (pipeline.py:335), and InitNet alone: fp32 <= 1e-4 vs the oracle on both kernel selections -- teacher-forced and free-running by
    decision replay over every keypoint (the 0 / 0 cases' smallest decision margin is 3.65e-5: a free comparison is ill-posed) --
    and bf16: the teacher-forced floors, and the same floors for the free-running run against the replay of its own decisions on
    both selections (per_crop takes the fused pair MLP, whose output reaches the next stage's rows through the carry copy)."""
    from checkerpose_amd.agreement import logit_agreement
    lm = case == "woEdgeConv_lm"
    ig, gr = {"woEdgeConv": (0, 0), "woEdgeConv_lm": (0, 0), "stage1_without": (2, (3, 0, 3)), "init_only": (0, 3)}[case]
    net = build_net(seed=4, lm=lm, init_graph=ig, graph=gr)
    img = det_image(2, seed=13)
    obj = torch.tensor([2, 9]) if lm else None
    knn_idx = net.init_net.knn_idx[obj - 1] if lm else net.init_net.knn_idx
    if case == "init_only":                             # InitNet_GNN alone (config init_gnn0_*: the pretraining network)
        sd_i = {k[len("init_net."):]: v for k, v in net.state_dict().items() if k.startswith("init_net.")}
        ref_i, _, _ = O.init_net_forward(sd_i, "", img, knn_idx, 512, "hrnet_w18", 0, 0.2)
        init = net.init_net.to(dev())
        out_i = init(img.to(dev()))
        assert float((out_i.cpu() - ref_i).abs().max()) <= 1e-4
        init.set_kernel_selection("per_crop")
        assert float((init(img.to(dev())).cpu() - ref_i).abs().max()) <= 1e-4
        return
    kw = dict(oracle_kwargs(), init_n_graph=ig, n_graph=gr)
    ref, inter = O.posenet_forward(net.state_dict(), img, knn_idx, 512, **kw)
    replay = _oracle_replayer(net, img, knn_idx, 512, kw, inter)
    net = net.to(dev())
    tb = _teacher_bits(ref).to(dev())
    okw = dict(obj_ids=obj.to(dev())) if lm else {}
    for sel in ("auto", "per_crop"):
        net.set_kernel_selection(sel)
        _cmp_e2e(net.forward_teacher_forced(img.to(dev()), tb, **okw), ref)
    free = (lambda: net(img.to(dev()), None, obj.to(dev()))) if lm else (lambda: net(img.to(dev()), None))
    _free_running_both_selections(net, free, replay, ref, case)
    net.set_compute_dtype("bf16")
    tf = logit_agreement(net.forward_teacher_forced(img.to(dev()), tb, **okw), ref)
    assert tf["bit_agreement_all_rows"] >= 0.99 and tf["bit_agreement_min_row"] >= 0.96 and tf["seg_agreement"] >= 0.99, (case, tf)
    assert tf["mean_abs_dlogit_over_rms"] <= 0.02 and tf["max_abs_dlogit"] <= 0.5, (case, tf)
    for sel in ("auto", "per_crop"):
        net.set_kernel_selection(sel)
        _bf16_replay_floors(free(), replay, ref, "%s bf16 [%s]" % (case, sel))


def test_batch_buckets_and_inplace_weight_edit(lib):
    """(a) Ragged batches run in the next cached program size (1, 2, 3, 4, 6, 8, 12, 16, ...) instead of building a program per
    size: B=5 and B=6 share ONE program, the 5 crops' outputs equal the first rows of the 6-crop forward bit for bit and the
    oracle within 1e-4.  (b) Eval programs fold BatchNorm / pack weights at build time: an in-place edit of a parameter (EMA swap,
    optimizer step in eval mode, a child's load_state_dict) must be seen by the next forward."""
    from checkerpose_amd.model._runtime import batch_bucket
    assert [batch_bucket(b) for b in (1, 3, 5, 6, 7, 9, 17, 33, 200, 256)] == [1, 3, 6, 6, 8, 12, 24, 48, 256, 256]
    net = build_net(seed=1)
    img = det_image(6, seed=5)
    ref, _ = O.posenet_forward(net.state_dict(), img[:5], net.init_net.knn_idx, 512, **oracle_kwargs())
    net = net.to(dev())
    o6 = net(img.to(dev()), None)
    o5 = net(img[:5].to(dev()), None)
    assert len(net._programs) == 1 and net.program_for(5) is net.program_for(6)
    for a, b in zip(o5, o6):
        assert a.shape[0] == 5 and torch.equal(a, b[:5])
    _cmp_e2e(o5, ref)
    assert tuple(net.input_buffer(5).shape) == (5, 3, 256, 256)
    # (b)
    w = net.refine_net[2].query_block.mlps[4].weight
    with torch.no_grad():
        w.mul_(-1.0)                                        # flips the last x / y bit logits' weight: no module hook fires, but the
    #                                                         tensor's version counter moves (as under an optimizer step / EMA copy_)
    o5b = net(img[:5].to(dev()), None)
    assert not torch.equal(o5b[1][:, -1], o5[1][:, -1])
    sd = {k: v.cpu() for k, v in net.state_dict().items()}
    ref_b, _ = O.posenet_forward(sd, img[:5], net.init_net.knn_idx.cpu(), 512, **oracle_kwargs())
    _cmp_e2e(o5b, ref_b)
    with torch.no_grad():
        net.init_net.mlp.bias.add_(0.25)                    # a child's parameter, edited through the child
    o5c = net(img[:5].to(dev()), None)
    assert float((o5c[0] - o5b[0]).abs().max()) > 0.2


@pytest.mark.parametrize("mode", ["per_crop", "tiled"])
def test_kernel_selection_pins_bits_across_batch_sizes(lib, mode):
    """`auto` picks per-conv / split-K launches below 40-96 crops and per-crop LDS-resident launches above (other accumulation
    order -> other bf16 bits for the same crop); `set_kernel_selection("per_crop" | "tiled")` pins ONE selection, after which a
    crop's outputs are bit-identical at batch 3 and inside a batch of 96 (across the `auto` crossovers)."""
    net = build_net(seed=1).to(dev()).set_compute_dtype("bf16").set_kernel_selection(mode)
    img3 = det_image(3, seed=3).to(dev())
    small = net(img3, None)
    big = net(img3.repeat(32, 1, 1, 1), None)
    for a, b in zip(small, big):
        assert b.shape[0] == 96 and torch.equal(b, a.repeat(32, *([1] * (a.dim() - 1))))
    names = {c[2].split(":")[0] for c in net.program_for(3).calls}
    assert ("hr_chain" in names) == (mode == "per_crop") and ("edge_fused" in names) == (mode == "per_crop")
    auto = build_net(seed=1).to(dev()).set_compute_dtype("bf16")
    assert "hr_chain" not in {c[2].split(":")[0] for c in auto.program_for(3).calls} if auto(img3, None) is not None else True


def test_batch_slices_concurrent_graphs_bitwise(lib, monkeypatch):
    """B=16 is run as two concurrent 8-crop slice graphs (CHECKERPOSE_AMD_SPLITS=2): identical, bit for bit, to the
    unsplit sequential replay; bf16 so the test is cheap on the CPU side (no oracle needed: pure scheduling check)."""
    from checkerpose_amd import engine
    monkeypatch.setattr(engine, "STEM_MIN_BATCH", 1)
    monkeypatch.setattr(engine, "CHAIN_MIN_BATCH", 1)      # slices and the unsplit batch must pick the same kernels
    monkeypatch.setattr(engine, "USE_SPLITK", False)       # (the split-K conv variant is chosen by output pixels = batch size)
    monkeypatch.setattr(engine, "EDGE_FUSED_MIN_BATCH", 1)
    monkeypatch.setattr(engine, "MLP_FUSED_MIN_ROWS", 1)
    img = det_image(16, seed=3).to(dev())
    net = build_net(seed=1).to(dev()).set_compute_dtype("bf16")
    net.batch_splits = 2
    o1 = net(img, None)            # eager (sequential)
    o2 = net(img, None)            # two graphs launched concurrently
    o3 = net(img, None)
    ref = build_net(seed=1).to(dev()).set_compute_dtype("bf16")
    ref.batch_splits, ref.use_graph = 1, False
    o4 = ref(img, None)
    for a, b, c, d in zip(o1, o2, o3, o4):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    assert len(net.program_for(16).progs) == 2 and len(ref.program_for(16).progs) == 1


def test_edge_neighbour_schedule_bitwise(lib, monkeypatch):
    """The bank-conflict-aware neighbour order handed to cp_edgeconv_fused (graph_sched.py) changes nothing: forward with the
    scheduled lists == forward with the kNN order, bit for bit (the max over a keypoint's neighbours ignores their order)."""
    from checkerpose_amd import engine
    monkeypatch.setattr(engine, "EDGE_FUSED_MIN_BATCH", 1)
    monkeypatch.setattr(engine, "MLP_FUSED_MIN_ROWS", 1)
    img = det_image(4, seed=3).to(dev())
    a = build_net(seed=1).to(dev()).set_compute_dtype("bf16")
    o1 = [t.clone() for t in a(img, None)]
    assert any(k[0] == "edge_sched" for k in a._stores[list(a._stores)[0]].cache if isinstance(k, tuple))
    monkeypatch.setattr(engine, "EDGE_SCHED", False)
    b = build_net(seed=1).to(dev()).set_compute_dtype("bf16")
    for x, y in zip(o1, b(img, None)):
        assert torch.equal(x, y)


def test_postprocess_correspondences_on_device(lib):
    """Next-row N2: device-side correspondence list == the reference's host-side extraction (oracle restatement of
    test.py:294-329 + from_id_to_pose :50-59), bit exact, on real forward outputs."""
    from checkerpose_amd.postprocess import correspondences
    net = build_net(seed=1)
    img = det_image(3, seed=5)
    ref, _ = O.posenet_forward(net.state_dict(), img, net.init_net.knn_idx, 512, **oracle_kwargs())
    grid = det_tensor("roi_xy", (3, 2, 64, 64), 300.0) + 320.0
    rp2d, rvalid, rcount = O.correspondences(ref[0], ref[3], ref[4], ref[5], grid)
    net = net.to(dev())
    out = net(img.to(dev()), None)
    p2d, valid, count = correspondences(out, grid.to(dev()))
    torch.cuda.synchronize()
    assert torch.equal(p2d.cpu(), rp2d) and torch.equal(valid.cpu(), rvalid) and torch.equal(count.cpu(), rcount)
    assert 0 < int(rcount[:, 0].min()) and int(rcount[:, 2].sum()) <= int(rcount[:, 0].sum())
    for bd in (2, 5):                                  # from_id_to_pose's discard_bd_pixel (:60-63)
        rp2d, rvalid, rcount = O.correspondences(ref[0], ref[3], ref[4], ref[5], grid, discard_bd_pixel=bd)
        p2d, valid, count = correspondences(out, grid.to(dev()), discard_bd_pixel=bd)
        assert torch.equal(p2d.cpu(), rp2d) and torch.equal(valid.cpu(), rvalid) and torch.equal(count.cpu(), rcount)


def test_postprocess_correspondences_from_final_bboxes(lib):
    """cp_correspondences_bbox builds the loader's coordinate grid on the fly: same result as handing over the (B,2,H,W) roi_xy_ori
    tensor the loader makes from the crop's final box (mapping_pixel_position_to_original_position_2d, bop_dataset_pytorch.py:223-235,
    in float64, cast to float32 at :380), bit for bit -- boxes with negative corners, odd sizes and a degenerate one"""
    from checkerpose_amd.postprocess import correspondences
    net = build_net(seed=1).to(dev())
    out = net(det_image(5, seed=5).to(dev()), None)
    boxes = np.array([[-2, 4, 45, 45], [100, 37, 211, 211], [0, 0, 64, 64], [310, 200, 77, 77], [5, 5, 0, 0]])
    S = 64
    pix = np.linspace(0, S - 1, S)                                             # the loader's roi_xy (:266-269)
    gx, gy = np.meshgrid(pix, pix)
    grid = np.stack([np.stack([b[2] / S * gx + b[0], b[3] / S * gy + b[1]]) for b in boxes])          # float64
    grid_t = torch.from_numpy(grid).type(torch.float)
    for bd in (0, 3):
        want = correspondences(out, grid_t.to(dev()), discard_bd_pixel=bd)
        got = correspondences(out, None, discard_bd_pixel=bd, Bboxes=boxes)
        got_t = correspondences(out, discard_bd_pixel=bd, Bboxes=torch.from_numpy(boxes).to(dev()))
        for a, b, c in zip(want, got, got_t):
            assert torch.equal(a, b) and torch.equal(a, c)
    with pytest.raises(ValueError):
        correspondences(out, grid_t.to(dev()), Bboxes=boxes)
    with pytest.raises(ValueError):
        correspondences(out)


def test_postprocess_correspondences_vs_reference_from_id_to_pose(lib):
    """cp_correspondences on the golden's inputs == the lists the REFERENCE's from_id_to_pose handed to its (stubbed,
    recording) solver: check_seg in {False, full, visib} x discard_bd_pixel in {0, 2} (n2_from_id_to_pose.npz)."""
    from checkerpose_amd.postprocess import correspondences
    g, e = golden("n2_from_id_to_pose"), golden("e2e_injected")
    d = dev()
    outs = (torch.from_numpy(e["roi"]).to(d), torch.from_numpy(e["xb"]).to(d), torch.from_numpy(e["yb"]).to(d),
            torch.from_numpy(e["seg"] - g["seg_shift"]).to(d), torch.from_numpy(e["xid"].astype(np.int64)).to(d),
            torch.from_numpy(e["yid"].astype(np.int64)).to(d))
    grid = det_tensor(str(g["grid_name"]), (2, 2, 64, 64), float(g["grid_scale"])) + float(g["grid_shift"])
    for bd in (0, 2):
        p2d, valid, count = correspondences(outs, grid.to(d), discard_bd_pixel=bd)
        p2d, valid, count = p2d.cpu(), valid.cpu(), count.cpu()
        for b in range(2):
            for col, cs in enumerate(("all", "full", "visib")):
                key = "b%d_%s_bd%d" % (b, cs, bd)
                sel = valid[b, :, col].bool()
                assert torch.nonzero(sel)[:, 0].tolist() == g[key + "_idx"].tolist(), key
                assert np.array_equal(p2d[b][sel].numpy(), g[key + "_p2d"]), key
                assert int(count[b, col]) == len(g[key + "_idx"])


def test_uint8_input_path_on_device(lib):
    """Next-row N3: raw uint8 HWC crops normalised on the device == ToTensor+Normalize on the host (oracle
    restatement of bop_dataset_pytorch.py:385-391): bit-identical network outputs in fp32, and within 1e-4 of the oracle."""
    net = build_net(seed=1)
    u8 = (det_tensor("u8img", (2, 256, 256, 3)).abs() * 255.999).to(torch.uint8)
    x = O.preprocess_uint8(u8)
    ref, _ = O.posenet_forward(net.state_dict(), x, net.init_net.knn_idx, 512, **oracle_kwargs())
    net = net.to(dev())
    o_float = net(x.to(dev()), None)
    o_u8 = net(u8.to(dev()), None)
    for a, b in zip(o_float, o_u8):
        assert torch.equal(a, b)
    _cmp_e2e(o_u8, ref)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_full_batch_size_property_batch_independence(lib, dt, monkeypatch):
    """Size-independent property at the BENCH batch size (bench.py default: 256 crops): a crop's outputs must not depend on
    its batch mates or on the batch size (different grids, tiles, persistent-block schedules, workspace placement, graph
    lanes).  256 crops = 4 distinct crops x 64 copies: every copy must equal, bit for bit, the B=4 forward -- which
    test_e2e_* pins to the oracle (fp32) and test_e2e_bf16_accuracy_contract bounds (bf16)."""
    from checkerpose_amd import engine
    monkeypatch.setattr(engine, "EDGE_FUSED_MIN_BATCH", 1)
    monkeypatch.setattr(engine, "MLP_FUSED_MIN_ROWS", 1)
    monkeypatch.setattr(engine, "STEM_MIN_BATCH", 1)
    monkeypatch.setattr(engine, "USE_SPLITK", False)     # ... and no batch-size-dependent split-K conv variant
    monkeypatch.setattr(engine, "CHAIN_MIN_BATCH", 1)    # same kernel selection at B=4 and B=256 (below 16 crops the engine
    #                                                      would pick per-conv launches: other K order, other bf16 roundings)
    net = build_net(seed=1).to(dev()).set_compute_dtype(dt)
    img4 = det_image(4, seed=3 if dt == "bf16" else 21).to(dev())     # bf16: the crops of the accuracy-contract test
    ref4 = net(img4, None)
    big = img4.repeat(64, 1, 1, 1)                        # crop i of the big batch == crop i % 4
    net(big, None)                                        # eager
    out = net(big, None)                                  # hipGraph with lanes
    for a, r in zip(out, ref4):
        assert a.shape[0] == 256
        assert torch.equal(a, r.repeat(64, *([1] * (r.dim() - 1))))


YCBV_FP32 = (1, 6, 11, 16, 21)


@pytest.mark.parametrize("obj", YCBV_FP32)
def test_e2e_ycbv_object_graph(lib, obj):
    """BASELINE config #4: a YCB-V object = its own FPS keypoints -> its own kNN graph (pinned by the reference-made knn_ycbv512
    fixture in test_oracle.py) and its own weights (the reference trains one network per object, train.py:384,396; bench.py's
    ycbv_rr21 uses seed = object id too).  Five per-object networks: fp32 <= 1e-4 vs the oracle (teacher-forced; free-running by
    decision replay: every logit, ids == the run's own logits decoded, both kernel selections), and the bf16
    teacher-forced contract of DESIGN.md §5.  All 21 graphs run in test_e2e_ycbv_all_21_graphs_one_batch."""
    from checkerpose_amd.agreement import logit_agreement
    from tests.common import ycbv_p3d
    p3d = ycbv_p3d(obj, 512)
    net = build_net(p3d=p3d, seed=obj)
    img = det_image(1, seed=40 + obj)
    ref, inter = O.posenet_forward(net.state_dict(), img, net.init_net.knn_idx, 512, **oracle_kwargs())
    replay = _oracle_replayer(net, img, net.init_net.knn_idx, 512, oracle_kwargs(), inter)
    assert not torch.equal(net.init_net.knn_idx, O.knn(ape_p3d(512), 20))       # really a different graph
    net = net.to(dev())
    out_t = net.forward_teacher_forced(img.to(dev()), _teacher_bits(ref).to(dev()))
    _cmp_e2e(out_t, ref)
    _free_running_both_selections(net, lambda: net(img.to(dev()), None), replay, ref, "ycbv obj %d" % obj)
    net.set_compute_dtype("bf16")
    tf = logit_agreement(net.forward_teacher_forced(img.to(dev()), _teacher_bits(ref).to(dev())), ref)
    # one crop = 512 decisions per logit row (the contract's 98 % per row is stated over the >= 2048 of a 4-crop batch: with
    # random-init weights a row whose logits sit near 0 loses ~10 of 512 to bf16 rounding): all 13 rows together >= 99 %, no row < 96 %
    assert tf["bit_agreement_all_rows"] >= 0.99 and tf["bit_agreement_min_row"] >= 0.96 and tf["seg_agreement"] >= 0.99, (obj, tf)
    assert tf["mean_abs_dlogit_over_rms"] <= 0.02 and tf["max_abs_dlogit"] <= 0.5, (obj, tf)


def test_e2e_ycbv_all_21_graphs_one_batch(lib):
    """All 21 YCB-V kNN graphs in ONE forward: the per-sample-graph twin (pipeline_lm.py:55-57 semantics) built over the 21 objects'
    keypoints, a batch of 21 crops with obj_ids 1..21 -- every graph gathers for its own crop; fp32 teacher-forced <= 1e-4 vs the
    oracle (which gathers through `knn_idx[obj_ids - 1]`), and the bf16 contract over the 21 x 512 decisions per row."""
    from checkerpose_amd.agreement import logit_agreement
    from tests.common import ycbv_p3d
    p3d = torch.cat([ycbv_p3d(o, 512) for o in range(1, 22)], 0)               # (21, 3, 512)
    net = build_net(p3d=p3d, seed=4, lm=True)
    assert tuple(net.init_net.knn_idx.shape) == (21, 512, 20)
    g = golden("knn_ycbv512")
    for k, o in enumerate(g["objs"]):                                           # the tables the forward gathers through = the reference's
        assert (np.sort(net.init_net.knn_idx[o - 1].numpy(), 1) == np.sort(g["idx"][k].astype(np.int64), 1)).all()
    obj = torch.arange(1, 22)
    img = det_image(21, seed=77)
    ref, _ = O.posenet_forward(net.state_dict(), img, net.init_net.knn_idx[obj - 1], 512, **oracle_kwargs())
    net = net.to(dev())
    out_t = net.forward_teacher_forced(img.to(dev()), _teacher_bits(ref).to(dev()), obj_ids=obj.to(dev()))
    _cmp_e2e(out_t, ref)
    net.set_compute_dtype("bf16")
    tf = logit_agreement(net.forward_teacher_forced(img.to(dev()), _teacher_bits(ref).to(dev()), obj_ids=obj.to(dev())), ref)
    assert tf["bit_agreement_min_row"] >= 0.98 and tf["seg_agreement"] >= 0.99, tf
    assert tf["mean_abs_dlogit_over_rms"] <= 0.02 and tf["max_abs_dlogit"] <= 0.5, tf
