"""GPU (-m gpu): training-side dense kernels through the C ABI against torch-CPU autograd of the
same op (fp32 reference of the op; inputs rounded to the storage type first for bf16).
Tolerances: fp32 2e-4 * (1 + |ref|) (sums over up to ~1e5 pixels in a different order, atomics across slices);
bf16 3e-2 * (1 + |ref|) relative to the fp32 result on bf16-rounded inputs.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from checkerpose_amd import _abi
from checkerpose_amd._abi import ACT_LEAKY, ACT_NONE, ACT_RELU, CP_BF16, CP_F32, CpConvDesc, CpWgradDesc
from tests.common import det_tensor
from tests.test_gpu_parity import DT, close, dev, from_cl, pack, rnd, rup, st, to_cl

pytestmark = pytest.mark.gpu
TOLT = {CP_F32: 2e-4, CP_BF16: 3e-2}


WG_WS = {}


def wgrad(lib, dtype, dy_cl, x_cl, Cout, Cin, R, S, stride, pad, dy_coff=0, x_coff=0):
    """runs both reductions of the pixel-slice partials (fp32 atomics; scratch buffer + reduce launch) and checks they agree"""
    a = _wgrad(lib, dtype, dy_cl, x_cl, Cout, Cin, R, S, stride, pad, dy_coff, x_coff, False)
    b = _wgrad(lib, dtype, dy_cl, x_cl, Cout, Cin, R, S, stride, pad, dy_coff, x_coff, True)
    sc = float(a.abs().max()) + 1e-30
    assert float((a - b).abs().max()) / sc < 1e-5
    return b


def _wgrad(lib, dtype, dy_cl, x_cl, Cout, Cin, R, S, stride, pad, dy_coff, x_coff, use_ws):
    B, Ho, Wo, dcs = dy_cl.shape
    _, H, W, xcs = x_cl.shape
    dw = torch.zeros(Cout, Cin, R, S, dtype=torch.float32, device=dev())
    d = CpWgradDesc()
    d.dtype, d.B, d.H, d.W, d.Ho, d.Wo = dtype, B, H, W, Ho, Wo
    d.Cout, d.dy_cstride, d.dy_coff, d.Cin, d.x_cstride, d.x_coff = Cout, dcs, dy_coff, Cin, xcs, x_coff
    d.R, d.S, d.stride, d.pad = R, S, stride, pad
    d.dw_base, d.dw_sco, d.dw_sci, d.dw_sr, d.dw_ss = 0, Cin * R * S, R * S, S, 1
    if use_ws:
        if "ws" not in WG_WS:
            WG_WS["ws"] = torch.empty(64 << 20, dtype=torch.uint8, device=dev())
        _abi.check(lib.cp_conv2d_wgrad_ws(st(), C.byref(d), dy_cl.data_ptr(), x_cl.data_ptr(), dw.data_ptr(), WG_WS["ws"].data_ptr(),
                                          WG_WS["ws"].numel()), "wgrad_ws")
    else:
        _abi.check(lib.cp_conv2d_wgrad(st(), C.byref(d), dy_cl.data_ptr(), x_cl.data_ptr(), dw.data_ptr()), "wgrad")
    torch.cuda.synchronize()
    return dw.cpu()


WGRAD_CASES = [  # (B, Cin, H, W, Cout, k, stride, pad)
    (2, 18, 16, 24, 36, 3, 1, 1),      # ragged channels both sides
    (3, 64, 16, 16, 64, 3, 1, 1),
    (1, 256, 8, 8, 256, 3, 1, 1),      # 4x4 channel blocks
    (2, 3, 32, 32, 64, 3, 2, 1),       # stem, 3 input channels
    (2, 36, 14, 18, 72, 3, 2, 1),      # stride 2, odd-ish sizes (generic per-tap kernel)
    (2, 18, 64, 64, 18, 3, 2, 1),      # stride 2 on power-of-two maps, <= 32 x 32 channels: all-taps kernel (fuse layers 64 -> 32)
    (3, 24, 32, 32, 32, 3, 2, 1),      # ... 16 x 16 output
    (2, 18, 16, 16, 18, 3, 2, 1),      # ... 8 x 8 output (one 8 x 8 tile per image)
    (3, 18, 32, 32, 72, 3, 2, 1),      # stride 2, wide output: the per-tap kernel
    (2, 3, 64, 64, 64, 3, 2, 1),       # the stem: 3 input channels
    (2, 144, 8, 8, 18, 1, 1, 0),       # fuse 1x1
    (2, 256, 16, 16, 64, 2, 1, 1),     # patch_generator k=2 pad=1
    (3, 64, 1, 100, 128, 1, 1, 0),     # linear over keypoints, pixel tail
    (1, 16, 40, 40, 10, 7, 2, 3),      # 7x7 stride 2
    (16, 32, 32, 32, 32, 3, 1, 1),     # many pixel slices (atomics across slices)
    (2, 72, 64, 64, 144, 3, 1, 1),     # all-taps 3x3 kernel: 1 x 64 tiles, ragged channel blocks (72 / 144)
    (2, 18, 64, 128, 18, 3, 1, 1),     # all-taps kernel, W > 64, one active wave quadrant
    (3, 256, 16, 16, 128, 3, 1, 1),    # all-taps kernel, 4 x 16 tiles
    (4, 32, 32, 32, 24, 3, 1, 1),      # tap-split small-channel kernel (<= 32 x 32), 2 x 32 tiles
    (5, 18, 8, 8, 18, 3, 1, 1),        # tap-split kernel, 8 x 8 tiles, odd tile count
]


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", WGRAD_CASES)
def test_wgrad_vs_torch_autograd(lib, dtype, case):
    B, Cin, H, W, Cout, k, stride, pad = case
    x = rnd(det_tensor("wx%s" % (case,), (B, Cin, H, W)), dtype)
    w = det_tensor("ww%s" % (case,), (Cout, Cin, k, k), 0.1).requires_grad_(True)
    with torch.enable_grad():
        y = F.conv2d(x, w, None, stride, pad)
    dy = rnd(det_tensor("wd%s" % (case,), tuple(y.shape)), dtype)
    (ref,) = torch.autograd.grad(y, w, dy)
    got = wgrad(lib, dtype, to_cl(dy, dtype), to_cl(x, dtype), Cout, Cin, k, k, stride, pad)
    scale = ref.abs().max().item()
    close(got / scale, ref / scale, TOLT[dtype])


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_wgrad_channel_slices(lib, dtype):
    """operands that are channel slices of wider buffers (concat layouts)"""
    B, H, W = 2, 8, 8
    xa = rnd(det_tensor("sl_x", (B, 48, H, W)), dtype)
    dya = rnd(det_tensor("sl_d", (B, 40, H, W)), dtype)
    x, dy = xa[:, 16:48], dya[:, 8:32]
    w = torch.zeros(24, 32, 3, 3, requires_grad=True)
    with torch.enable_grad():
        y = F.conv2d(x, w, None, 1, 1)
    (ref,) = torch.autograd.grad(y, w, dy)
    got = wgrad(lib, dtype, to_cl(dya, dtype), to_cl(xa, dtype), 24, 32, 3, 3, 1, 1, dy_coff=8, x_coff=16)
    scale = ref.abs().max().item()
    close(got / scale, ref / scale, TOLT[dtype])


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_wgrad_convtranspose(lib, dtype):
    """ConvTranspose2d(k3,s2,p1,op1) weight gradient = conv wgrad with the layer input as `dy` and dout as `x`"""
    B, Ci, Co, H = 2, 64, 32, 8
    x = rnd(det_tensor("ct_x", (B, Ci, H, H)), dtype)
    w = det_tensor("ct_w", (Ci, Co, 3, 3), 0.1).requires_grad_(True)
    with torch.enable_grad():
        y = F.conv_transpose2d(x, w, None, 2, 1, 1)
    dy = rnd(det_tensor("ct_d", tuple(y.shape)), dtype)
    (ref,) = torch.autograd.grad(y, w, dy)
    got = wgrad(lib, dtype, to_cl(x, dtype), to_cl(dy, dtype), Ci, Co, 3, 3, 2, 1)
    scale = ref.abs().max().item()
    close(got / scale, ref / scale, TOLT[dtype])


def conv_cl(lib, dtype, xin, pw, Cout, R, S, stride, pad, Ho, Wo, ostr=None, out=None):
    B, H, W, cs = xin.shape
    E = 8 if dtype == CP_BF16 else 4
    cop = rup(Cout, E)
    if out is None:
        out = torch.zeros(B, Ho, Wo, cop, dtype=DT[dtype], device=dev())
    n16 = rup(Cout, 16)
    sc = torch.zeros(n16, device=dev()); sc[:Cout] = 1.0
    sh = torch.zeros(n16, device=dev())
    d = CpConvDesc()
    d.dtype, d.out_f32, d.B, d.H, d.W = dtype, 0, B, H, W
    d.Cin, d.in_cstride, d.in_coff = cs, cs, 0
    d.R, d.S, d.stride, d.pad, d.Ho, d.Wo, d.Cout, d.act, d.slope = R, S, stride, pad, Ho, Wo, cop, ACT_NONE, 0.0
    if ostr is None:
        d.o_base, d.o_sb, d.o_sy, d.o_sx, d.o_sc = 0, Ho * Wo * cop, Wo * cop, cop, 1
    else:
        d.o_base, d.o_sb, d.o_sy, d.o_sx, d.o_sc = ostr
    _abi.check(lib.cp_conv2d_igemm(st(), C.byref(d), xin.data_ptr(), pw.data_ptr(), sc.data_ptr(), sh.data_ptr(), None,
                                   out.data_ptr()), "conv")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", [(2, 18, 12, 16, 36, 3, 1), (2, 64, 8, 8, 32, 1, 0), (1, 32, 9, 9, 16, 2, 1)])
def test_dgrad_stride1(lib, dtype, case):
    """dx of a stride-1 conv = conv(dy, cp_weight_dgrad(w), pad R-1-pad)"""
    B, Cin, H, W, Cout, k, pad = case
    x = torch.zeros(B, Cin, H, W, requires_grad=True)
    w = rnd(det_tensor("dg_w%s" % (case,), (Cout, Cin, k, k), 0.2), dtype)
    with torch.enable_grad():
        y = F.conv2d(x, w, None, 1, pad)
    dy = rnd(det_tensor("dg_d%s" % (case,), tuple(y.shape)), dtype)
    (ref,) = torch.autograd.grad(y, x, dy)
    wd = w.to(dev()).contiguous()
    wt = torch.empty(Cin, Cout, k, k, device=dev())
    _abi.check(lib.cp_weight_dgrad(st(), wd.data_ptr(), Cout, Cin, k, k, wt.data_ptr()))
    torch.cuda.synchronize()
    dyc = to_cl(dy, dtype)
    pw = pack(lib, dtype, wt.cpu(), dyc.shape[-1], k, k)
    got = conv_cl(lib, dtype, dyc, pw, Cin, k, k, 1, k - 1 - pad, H, W)
    close(from_cl(got, Cin), ref, TOLT[dtype])


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_dgrad_stride2_and_convtranspose(lib, dtype):
    """dx of a 3x3/s2/p1 conv = the ConvTranspose phase launches on w itself; dx of ConvTranspose2d = 3x3/s2 conv with w"""
    B, Cin, H, Cout = 2, 36, 16, 72
    x = torch.zeros(B, Cin, H, H, requires_grad=True)
    w = rnd(det_tensor("d2_w", (Cout, Cin, 3, 3), 0.2), dtype)
    with torch.enable_grad():
        y = F.conv2d(x, w, None, 2, 1)
    dy = rnd(det_tensor("d2_d", tuple(y.shape)), dtype)
    (ref,) = torch.autograd.grad(y, x, dy)
    E = 8 if dtype == CP_BF16 else 4
    dyc = to_cl(dy, dtype)
    cop = rup(Cin, E)
    out = torch.zeros(B, H, H, cop, dtype=DT[dtype], device=dev())
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        pw = pack(lib, dtype, w, dyc.shape[-1], 1 + a, 1 + b, rows=Cin, transposed=1, phase=ph)
        conv_cl(lib, dtype, dyc, pw, Cin, 1 + a, 1 + b, 1, 0, H // 2, H // 2,
                ostr=((a * H + b) * cop, H * H * cop, 2 * H * cop, 2 * cop, 1), out=out)
    close(from_cl(out, Cin), ref, TOLT[dtype])
    # ConvTranspose2d data-gradient
    xt = torch.zeros(B, 64, 8, 8, requires_grad=True)
    wt = rnd(det_tensor("d2_wt", (64, 32, 3, 3), 0.2), dtype)
    with torch.enable_grad():
        yt = F.conv_transpose2d(xt, wt, None, 2, 1, 1)
    dyt = rnd(det_tensor("d2_dt", tuple(yt.shape)), dtype)
    (reft,) = torch.autograd.grad(yt, xt, dyt)
    dytc = to_cl(dyt, dtype)
    pw = pack(lib, dtype, wt, dytc.shape[-1], 3, 3)          # read as conv weight (Cout'=64, Cin'=32, 3, 3)
    got = conv_cl(lib, dtype, dytc, pw, 64, 3, 3, 2, 1, 8, 8)
    close(from_cl(got, 64), reft, TOLT[dtype])


def _vec(n, t=None):
    v = torch.zeros(rup(n, 16), device=dev())
    if t is not None:
        v[:n] = t.to(dev())
    return v


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", [(2, 18, 16, 16, ACT_RELU, True), (3, 64, 8, 8, ACT_LEAKY, False), (4, 256, 4, 4, ACT_NONE, False),
                                  (2, 36, 32, 32, ACT_RELU, False)])
def test_bn_train_fwd_bwd(lib, dtype, case):
    B, Cc, H, W, act, has_res = case
    M = B * H * W
    x = rnd(det_tensor("bn_x%s" % (case,), (B, Cc, H, W)) * 1.5 + 0.3, dtype).requires_grad_(True)
    res = rnd(det_tensor("bn_r%s" % (case,), (B, Cc, H, W)), dtype).requires_grad_(True) if has_res else None
    gamma = (1.0 + 0.5 * det_tensor("bn_g%s" % (case,), (Cc,))).requires_grad_(True)
    beta = (0.2 * det_tensor("bn_b%s" % (case,), (Cc,))).requires_grad_(True)
    rm0, rv0 = 0.1 * det_tensor("bn_m%s" % (case,), (Cc,)), 1.0 + 0.3 * det_tensor("bn_v%s" % (case,), (Cc,)).abs()
    rm, rv = rm0.clone(), rv0.clone()
    with torch.enable_grad():
        z = F.batch_norm(x, rm, rv, gamma, beta, True, 0.1, 1e-5)
        if has_res:
            z = z + res
        y = F.relu(z) if act == ACT_RELU else (F.leaky_relu(z, 0.2) if act == ACT_LEAKY else z)
    dy = rnd(det_tensor("bn_d%s" % (case,), (B, Cc, H, W)), dtype)
    grads = torch.autograd.grad(y, [x, gamma, beta] + ([res] if has_res else []), dy)
    # ---- HIP
    xc = to_cl(x.detach(), dtype)
    cs = xc.shape[-1]
    g_d, b_d, rm_d, rv_d = gamma.detach().to(dev()), beta.detach().to(dev()), rm0.to(dev()), rv0.to(dev())
    scale, shift, mean, rstd = _vec(Cc), _vec(Cc), _vec(Cc), _vec(Cc)
    ws = torch.zeros(lib.cp_bn_bwd_workspace_bytes(Cc), dtype=torch.uint8, device=dev())
    _abi.check(lib.cp_bn_train_stats(st(), dtype, xc.data_ptr(), M, Cc, cs, 0, g_d.data_ptr(), b_d.data_ptr(), rm_d.data_ptr(),
                                     rv_d.data_ptr(), 0.1, 1e-5, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                                     rstd.data_ptr(), ws.data_ptr()), "bn stats")
    rc_ = to_cl(res.detach(), dtype) if has_res else None
    yc = torch.empty_like(xc)
    _abi.check(lib.cp_affine_act(st(), dtype, xc.data_ptr(), cs, 0, scale.data_ptr(), shift.data_ptr(),
                                 rc_.data_ptr() if has_res else None, cs, 0, yc.data_ptr(), cs, 0, M, Cc, act, 0.2), "affine")
    torch.cuda.synchronize()
    close(from_cl(yc, Cc), y.detach(), TOLT[dtype])
    close(rm_d.cpu(), rm, 1e-5)
    close(rv_d.cpu(), rv, 1e-5)
    if cs > Cc:
        assert float(yc[..., Cc:].float().abs().max()) == 0.0
    dyc = to_cl(dy, dtype)
    dxc = torch.empty_like(xc)
    dres = torch.zeros_like(xc) if has_res else None
    dg, db = torch.zeros(Cc, device=dev()), torch.zeros(Cc, device=dev())
    _abi.check(lib.cp_bn_train_bwd(st(), dtype, dyc.data_ptr(), cs, 0, yc.data_ptr(), cs, 0, xc.data_ptr(), cs, 0,
                                   mean.data_ptr(), rstd.data_ptr(), g_d.data_ptr(), M, Cc, act, 0.2, dxc.data_ptr(), cs, 0,
                                   dres.data_ptr() if has_res else None, cs, 0, 0, dg.data_ptr(), db.data_ptr(),
                                   ws.data_ptr()), "bn bwd")
    torch.cuda.synchronize()
    tol = TOLT[dtype]
    sx = grads[0].abs().max().item()
    close(from_cl(dxc, Cc) / sx, grads[0] / sx, tol)
    close(dg.cpu() / grads[1].abs().max().item(), grads[1] / grads[1].abs().max().item(), tol)
    close(db.cpu() / grads[2].abs().max().item(), grads[2] / grads[2].abs().max().item(), tol)
    if has_res:
        close(from_cl(dres, Cc), grads[3], tol)


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_bias_act_bwd(lib, dtype):
    """x == NULL form: y = leaky(conv + b): dx = dy * act'(y), db = column sums"""
    B, Cc, N = 3, 64, 100
    y = rnd(det_tensor("ba_y", (B, Cc, 1, N)), dtype)
    dy = rnd(det_tensor("ba_d", (B, Cc, 1, N)), dtype)
    dz = torch.where(y > 0, dy, dy * 0.01)
    yc, dyc = to_cl(y, dtype), to_cl(dy, dtype)
    dxc = torch.empty_like(dyc)
    db = torch.zeros(Cc, device=dev())
    ws = torch.zeros(lib.cp_bn_bwd_workspace_bytes(Cc), dtype=torch.uint8, device=dev())
    _abi.check(lib.cp_bn_train_bwd(st(), dtype, dyc.data_ptr(), Cc, 0, yc.data_ptr(), Cc, 0, None, 0, 0, None, None, None,
                                   B * N, Cc, ACT_LEAKY, 0.01, dxc.data_ptr(), Cc, 0, None, 0, 0, 0, None, db.data_ptr(),
                                   ws.data_ptr()), "bias bwd")
    torch.cuda.synchronize()
    close(from_cl(dxc, Cc), dz, TOLT[dtype])
    close(db.cpu(), dz.sum((0, 2, 3)), TOLT[dtype])


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("shape", [(2, 16, 8, 8), (1, 32, 16, 16), (2, 8, 5, 7)])
def test_upsample2x_bwd(lib, dtype, shape):
    B, Cc, H, W = shape
    x = torch.zeros(B, Cc, H, W, requires_grad=True)
    with torch.enable_grad():
        y = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    dy = rnd(det_tensor("up_d%s" % (shape,), tuple(y.shape)), dtype)
    (ref,) = torch.autograd.grad(y, x, dy)
    dyc = to_cl(dy, dtype)
    base = rnd(det_tensor("up_b%s" % (shape,), (B, Cc, H, W)), dtype)
    for acc in (0, 1):
        dxc = to_cl(base, dtype)
        _abi.check(lib.cp_upsample2x_bilinear_ac_bwd(st(), dtype, dyc.data_ptr(), dxc.data_ptr(), B, H, W, Cc, Cc, 0, Cc, 0, acc))
        torch.cuda.synchronize()
        close(from_cl(dxc, Cc), ref + (base if acc else 0), TOLT[dtype])


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("shift", [0, 1, 2])
def test_fuse_sum_bwd(lib, dtype, shift):
    B, Cc, Hs, Ws = 2, 24, 4, 6
    H, W = Hs << shift, Ws << shift
    out = rnd(det_tensor("fs_o%d" % shift, (B, Cc, H, W)), dtype).clamp_min(0)
    dout = rnd(det_tensor("fs_d%d" % shift, (B, Cc, H, W)), dtype)
    dz = dout * (out > 0)
    ref = F.avg_pool2d(dz, 1 << shift) * float(1 << (2 * shift)) if shift else dz
    oc, dc = to_cl(out, dtype), to_cl(dout, dtype)
    ds = torch.zeros(B, Hs, Ws, oc.shape[-1], dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_fuse_sum_act_bwd(st(), dtype, dc.data_ptr(), oc.data_ptr(), ds.data_ptr(), B, Hs, Ws, oc.shape[-1], shift, 1, 0))
    _abi.check(lib.cp_fuse_sum_act_bwd(st(), dtype, dc.data_ptr(), oc.data_ptr(), ds.data_ptr(), B, Hs, Ws, oc.shape[-1], shift, 1, 1))
    torch.cuda.synchronize()
    close(from_cl(ds, Cc), 2 * ref, TOLT[dtype])


def _rev_graph(idx):
    from checkerpose_amd.train_ops import reverse_graph
    return reverse_graph(idx)


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", [(3, 16, 64, 48, 6, 0.2), (2, 64, 64, 64, 20, 0.2), (2, 256, 256, 40, 8, 0.1)])
def test_edgeconv_train_fwd_bwd(lib, dtype, case):
    """factored train-mode EdgeConv vs torch autograd of the reference formulation (init.py:36-68): get_graph_feature ->
    Conv2d(2C->C',1x1) -> BatchNorm2d (batch stats over B*N*K) -> LeakyReLU -> max over K"""
    B, Cin, Co, N, K, slope = case
    x = rnd(det_tensor("ec_x%s" % (case,), (B, Cin, N)), dtype)
    pts = det_tensor("ec_p%s" % (case,), (1, 3, N))
    idx = (-((pts[:, :, :, None] - pts[:, :, None, :]) ** 2).sum(1)).topk(k=K, dim=-1)[1][0]      # (N,K)
    w = det_tensor("ec_w%s" % (case,), (Co, 2 * Cin), (1.0 / Cin) ** 0.5)
    gamma = (1.0 + 0.5 * det_tensor("ec_g%s" % (case,), (Co,)))
    gamma[::3] *= -1                                          # mixed-sign gammas (min/max switch)
    beta = 0.2 * det_tensor("ec_b%s" % (case,), (Co,))
    wpq = torch.cat([w[:, :Cin], w[:, Cin:] - w[:, :Cin]], 0)                    # (2C', C)
    pq = rnd(torch.einsum("oc,bcn->bno", wpq, x), dtype).requires_grad_(True)   # (B,N,2C') -- the kernel's input
    gamma.requires_grad_(True); beta.requires_grad_(True)
    rm, rv = torch.zeros(Co), torch.ones(Co)
    with torch.enable_grad():
        P, Q = pq[:, :, :Co], pq[:, :, Co:]
        e = (P[:, idx, :] + Q[:, :, None, :]).permute(0, 3, 1, 2)                # (B,C',N,K) == conv output
        z = F.leaky_relu(F.batch_norm(e, rm, rv, gamma, beta, True, 0.1, 1e-5), slope)
        y = z.max(dim=-1)[0]                                                     # (B,C',N)
    gout = rnd(det_tensor("ec_d%s" % (case,), (B, Co, N)), dtype)
    dpq_ref, dg_ref, db_ref = torch.autograd.grad(y, [pq, gamma, beta], gout)
    # ---- HIP
    d = dev()
    pqd = pq.detach().to(DT[dtype]).to(d).contiguous()
    idx32 = idx.int().to(d).contiguous()[None]
    rev_ptr, rev_edge = _rev_graph(idx32)
    out = torch.zeros(B, N, Co, dtype=DT[dtype], device=d)
    kstar = torch.zeros(B, N, Co, dtype=torch.uint8, device=d)
    vec = [torch.zeros(Co, device=d) for _ in range(4)]
    g_d, b_d = gamma.detach().to(d), beta.detach().to(d)
    rm_d, rv_d = torch.zeros(Co, device=d), torch.ones(Co, device=d)
    ws = torch.empty(lib.cp_edge_train_workspace_bytes(B, Co), dtype=torch.uint8, device=d)
    _abi.check(lib.cp_edgeconv_train_fwd(st(), dtype, pqd.data_ptr(), idx32.data_ptr(), None, g_d.data_ptr(), b_d.data_ptr(),
                                         rm_d.data_ptr(), rv_d.data_ptr(), 0.1, 1e-5, out.data_ptr(), Co, 0, kstar.data_ptr(),
                                         vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(),
                                         ws.data_ptr(), B, N, K, Co, 1, slope), "edge fwd")
    torch.cuda.synchronize()
    close(out.float().cpu(), y.detach().permute(0, 2, 1), TOLT[dtype])
    close(rm_d.cpu(), rm, 1e-4)
    close(rv_d.cpu(), rv, 1e-4)
    gc = gout.permute(0, 2, 1).contiguous().to(DT[dtype]).to(d)
    dpq = torch.zeros(B, N, 2 * Co, dtype=DT[dtype], device=d)
    dg, db = torch.zeros(Co, device=d), torch.zeros(Co, device=d)
    _abi.check(lib.cp_edgeconv_train_bwd(st(), dtype, pqd.data_ptr(), idx32.data_ptr(), rev_ptr.data_ptr(), rev_edge.data_ptr(),
                                         None, out.data_ptr(), Co, 0, kstar.data_ptr(), gc.data_ptr(), Co, 0, g_d.data_ptr(),
                                         vec[2].data_ptr(), vec[3].data_ptr(), dpq.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                         ws.data_ptr(), B, N, K, Co, 1, slope), "edge bwd")
    torch.cuda.synchronize()
    D = dpq.float().cpu()
    dP, dQ = D[:, :, :Co] + D[:, :, Co:], D[:, :, Co:]
    tol = TOLT[dtype]
    s = dpq_ref.abs().max().item()
    close(dQ / s, dpq_ref[:, :, Co:] / s, tol)
    close(dP / s, dpq_ref[:, :, :Co] / s, 2 * tol)
    close(dg.cpu() / dg_ref.abs().max().item(), dg_ref / dg_ref.abs().max().item(), tol)
    close(db.cpu() / db_ref.abs().max().item(), db_ref / db_ref.abs().max().item(), tol)


def test_edge_weight_views(lib):
    Co, Ci = 24, 16
    w = det_tensor("ewv", (Co, 2 * Ci))
    wd = w.to(dev())
    o0 = torch.empty(2 * Co, Ci, device=dev())
    o1 = torch.empty(Ci, 2 * Co, device=dev())
    _abi.check(lib.cp_edge_weight_view(st(), wd.data_ptr(), Co, Ci, 0, o0.data_ptr()))
    _abi.check(lib.cp_edge_weight_view(st(), wd.data_ptr(), Co, Ci, 1, o1.data_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(o0.cpu(), torch.cat([w[:, :Ci], w[:, Ci:] - w[:, :Ci]], 0))
    assert torch.equal(o1.cpu(), torch.cat([w[:, :Ci].t(), w[:, Ci:].t()], 1))


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_strided_to_nhwc_and_memset(lib, dtype):
    B, Cc, N = 2, 3, 10
    bits = det_tensor("s2n", (B, 13, N))
    src = bits.to(dev())
    E = 8 if dtype == CP_BF16 else 4
    out = torch.full((B, N, E), 7.0, dtype=DT[dtype], device=dev())
    _abi.check(lib.cp_strided_to_nhwc(st(), dtype, src.data_ptr(), CP_F32, 4 * N, 13 * N, 1, N, out.data_ptr(), B, N, Cc, E))
    torch.cuda.synchronize()
    ref = torch.zeros(B, N, E)
    ref[..., :Cc] = rnd(bits[:, 4:7].permute(0, 2, 1), dtype)
    assert torch.equal(out.float().cpu(), ref)
    _abi.check(lib.cp_memset_zero(st(), out.data_ptr(), out.numel() * out.element_size()))
    torch.cuda.synchronize()
    assert float(out.float().abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [CP_F32])
def test_edgeconv_train_full_layer_real_graph(lib, dtype):
    """whole train-mode StaticGraph_module at the real size (ape kNN graph, N=512, K=20, C=256): node GEMM ->
    cp_edgeconv_train_fwd ; backward: cp_edgeconv_train_bwd -> two wgrad launches + the [W1 W2]-view data-gradient,
    against torch autograd of the reference formulation w.r.t. x, W, gamma, beta"""
    from tests.common import ape_p3d
    from checkerpose_amd.model.init import knn
    B, Cin, Co, N, K, slope = 2, 256, 256, 512, 20, 0.2
    idx = knn(ape_p3d(N), K)[0]
    x = rnd(det_tensor("fl_x", (B, Cin, N)), dtype).requires_grad_(True)
    w = det_tensor("fl_w", (Co, 2 * Cin), (1.0 / Cin) ** 0.5).requires_grad_(True)
    gamma = (1.0 + 0.5 * det_tensor("fl_g", (Co,)))
    gamma[::3] *= -1
    beta = 0.2 * det_tensor("fl_b", (Co,))
    gamma.requires_grad_(True); beta.requires_grad_(True)
    with torch.enable_grad():
        nb = x[:, :, idx]                                                        # (B,C,N,K)
        ctr = x[:, :, :, None].expand(-1, -1, -1, K)
        e = F.conv2d(torch.cat([nb - ctr, ctr], 1), w[:, :, None, None])
        z = F.leaky_relu(F.batch_norm(e, torch.zeros(Co), torch.ones(Co), gamma, beta, True, 0.1, 1e-5), slope)
        y = z.max(dim=-1)[0]
    gout = rnd(det_tensor("fl_d", (B, Co, N)), dtype)
    dx_ref, dw_ref, dg_ref, db_ref = torch.autograd.grad(y, [x, w, gamma, beta], gout)
    d = dev()
    wd = w.detach().to(d)
    wpq = torch.empty(2 * Co, Cin, 1, 1, device=d)
    wdg = torch.empty(Cin, 2 * Co, 1, 1, device=d)
    _abi.check(lib.cp_edge_weight_view(st(), wd.data_ptr(), Co, Cin, 0, wpq.data_ptr()))
    _abi.check(lib.cp_edge_weight_view(st(), wd.data_ptr(), Co, Cin, 1, wdg.data_ptr()))
    torch.cuda.synchronize()
    xc = to_cl(x.detach()[:, :, None, :], dtype)                                 # (B,1,N,C)
    pq = conv_cl(lib, dtype, xc, pack(lib, dtype, wpq.cpu(), Cin, 1, 1), 2 * Co, 1, 1, 1, 0, 1, N)
    idx32 = idx.int().to(d).contiguous()[None]
    rev_ptr, rev_edge = _rev_graph(idx32)
    out = torch.zeros(B, N, Co, dtype=DT[dtype], device=d)
    kstar = torch.zeros(B, N, Co, dtype=torch.uint8, device=d)
    vec = [torch.zeros(Co, device=d) for _ in range(4)]
    g_d, b_d = gamma.detach().to(d), beta.detach().to(d)
    ws = torch.empty(lib.cp_edge_train_workspace_bytes(B, Co), dtype=torch.uint8, device=d)
    _abi.check(lib.cp_edgeconv_train_fwd(st(), dtype, pq.data_ptr(), idx32.data_ptr(), None, g_d.data_ptr(), b_d.data_ptr(),
                                         None, None, 0.1, 1e-5, out.data_ptr(), Co, 0, kstar.data_ptr(), vec[0].data_ptr(),
                                         vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), ws.data_ptr(), B, N, K, Co, 1, slope))
    torch.cuda.synchronize()
    close(out.float().cpu(), y.detach().permute(0, 2, 1), TOLT[dtype])
    gc = gout.permute(0, 2, 1).contiguous().to(DT[dtype]).to(d)
    D = torch.zeros(B, 1, N, 2 * Co, dtype=DT[dtype], device=d)
    dg, db = torch.zeros(Co, device=d), torch.zeros(Co, device=d)
    _abi.check(lib.cp_edgeconv_train_bwd(st(), dtype, pq.data_ptr(), idx32.data_ptr(), rev_ptr.data_ptr(), rev_edge.data_ptr(), None,
                                         out.data_ptr(), Co, 0, kstar.data_ptr(), gc.data_ptr(), Co, 0, g_d.data_ptr(),
                                         vec[2].data_ptr(), vec[3].data_ptr(), D.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                         ws.data_ptr(), B, N, K, Co, 1, slope))
    torch.cuda.synchronize()
    close(dg.cpu() / dg_ref.abs().max().item(), dg_ref / dg_ref.abs().max().item(), TOLT[dtype])
    dw = torch.zeros(Co, 2 * Cin, device=d)
    for half in (0, 1):
        de = CpWgradDesc()
        de.dtype, de.B, de.H, de.W, de.Ho, de.Wo = dtype, B, 1, N, 1, N
        de.Cout, de.dy_cstride, de.dy_coff, de.Cin, de.x_cstride, de.x_coff = Co, 2 * Co, half * Co, Cin, Cin, 0
        de.R, de.S, de.stride, de.pad = 1, 1, 1, 0
        de.dw_base, de.dw_sco, de.dw_sci, de.dw_sr, de.dw_ss = half * Cin, 2 * Cin, 1, 1, 1
        _abi.check(lib.cp_conv2d_wgrad(st(), C.byref(de), D.data_ptr(), xc.data_ptr(), dw.data_ptr()))
    torch.cuda.synchronize()
    s = dw_ref.abs().max().item()
    close(dw.cpu() / s, dw_ref / s, TOLT[dtype])
    dx = conv_cl(lib, dtype, D, pack(lib, dtype, wdg.cpu(), 2 * Co, 1, 1), Cin, 1, 1, 1, 0, 1, N)
    s = dx_ref.abs().max().item()
    close(from_cl(dx, Cin)[:, :, 0] / s, dx_ref.detach() / s, TOLT[dtype])


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", [(2, 18, 16, 16, ACT_RELU, True), (3, 64, 8, 8, ACT_LEAKY, False), (2, 36, 32, 32, ACT_RELU, False)])
def test_bn_two_launch_forms(lib, dtype, case):
    """cp_bn_stats_accumulate + cp_bn_apply / cp_bn_bwd_accumulate + cp_bn_bwd_apply (fp64 atomics, no finalize launch)
    against torch autograd -- the forms the training program uses"""
    _bn_two_launch(lib, dtype, case)


def _bn_two_launch(lib, dtype, case):
    """the body of test_bn_two_launch_forms: runs the four launches, asserts them against torch autograd and returns what they wrote"""
    B, Cc, H, W, act, has_res = case
    M = B * H * W
    x = rnd(det_tensor("b2_x%s" % (case,), (B, Cc, H, W)) * 1.5 + 0.3, dtype).requires_grad_(True)
    res = rnd(det_tensor("b2_r%s" % (case,), (B, Cc, H, W)), dtype).requires_grad_(True) if has_res else None
    gamma = (1.0 + 0.5 * det_tensor("b2_g%s" % (case,), (Cc,))).requires_grad_(True)
    beta = (0.2 * det_tensor("b2_b%s" % (case,), (Cc,))).requires_grad_(True)
    rm, rv = torch.zeros(Cc), torch.ones(Cc)
    with torch.enable_grad():
        z = F.batch_norm(x, rm, rv, gamma, beta, True, 0.1, 1e-5)
        if has_res:
            z = z + res
        y = F.relu(z) if act == ACT_RELU else F.leaky_relu(z, 0.2)
    dy = rnd(det_tensor("b2_d%s" % (case,), (B, Cc, H, W)), dtype)
    grads = torch.autograd.grad(y, [x, gamma, beta] + ([res] if has_res else []), dy)
    xc = to_cl(x.detach(), dtype)
    cs = xc.shape[-1]
    g_d, b_d = gamma.detach().to(dev()), beta.detach().to(dev())
    rm_d, rv_d = torch.zeros(Cc, device=dev()), torch.ones(Cc, device=dev())
    mean, rstd = _vec(Cc), _vec(Cc)
    acc = torch.zeros(2, lib.cp_bn_acc_doubles(Cc), dtype=torch.float64, device=dev())       # [fwd | bwd] accumulator blocks
    rc_ = to_cl(res.detach(), dtype) if has_res else None
    yc = torch.empty_like(xc)
    _abi.check(lib.cp_bn_stats_accumulate(st(), dtype, xc.data_ptr(), M, Cc, cs, 0, acc[0].data_ptr()), "stats acc")
    _abi.check(lib.cp_bn_apply(st(), dtype, xc.data_ptr(), cs, 0, acc[0].data_ptr(), g_d.data_ptr(), b_d.data_ptr(), rm_d.data_ptr(),
                               rv_d.data_ptr(), 0.1, 1e-5, rc_.data_ptr() if has_res else None, cs, 0, yc.data_ptr(), cs, 0, M, Cc, act,
                               0.2, mean.data_ptr(), rstd.data_ptr()), "bn apply")
    torch.cuda.synchronize()
    close(from_cl(yc, Cc), y.detach(), TOLT[dtype])
    close(rm_d.cpu(), rm, 1e-5)
    close(rv_d.cpu(), rv, 1e-5)
    dyc = to_cl(dy, dtype)
    dres = torch.zeros_like(xc) if has_res else None
    dg, db = torch.zeros(Cc, device=dev()), torch.zeros(Cc, device=dev())
    _abi.check(lib.cp_bn_bwd_accumulate(st(), dtype, dyc.data_ptr(), cs, 0, yc.data_ptr(), cs, 0, xc.data_ptr(), cs, 0, mean.data_ptr(),
                                        rstd.data_ptr(), M, Cc, act, 0.2, acc[1].data_ptr()), "bwd acc")
    _abi.check(lib.cp_bn_bwd_apply(st(), dtype, dyc.data_ptr(), cs, 0, yc.data_ptr(), cs, 0, xc.data_ptr(), cs, 0, mean.data_ptr(),
                                   rstd.data_ptr(), g_d.data_ptr(), acc[1].data_ptr(), M, Cc, act, 0.2, dyc.data_ptr(), cs, 0,
                                   dres.data_ptr() if has_res else None, cs, 0, 1, dg.data_ptr(), db.data_ptr()), "bwd apply")
    torch.cuda.synchronize()
    tol = TOLT[dtype]
    sx = grads[0].abs().max().item()
    close(from_cl(dyc, Cc) / sx, grads[0] / sx, tol)                      # dx written in place over dy
    close(dg.cpu() / grads[1].abs().max().item(), grads[1] / grads[1].abs().max().item(), tol)
    close(db.cpu() / grads[2].abs().max().item(), grads[2] / grads[2].abs().max().item(), tol)
    if has_res:
        close(from_cl(dres, Cc), grads[3], tol)
    return [t.clone() for t in (yc, dyc, mean, rstd, rm_d, rv_d, dg, db, acc)] + ([dres] if has_res else [])


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_wgrad_group_equals_the_single_layer_launches(lib, dtype):
    """cp_wgrad_group (the partial-sum launches of several layers in one launch per kernel kind, every layer cut for its share of the
    workgroups) + ONE cp_wgrad_reduce_batch against cp_conv2d_wgrad_ws layer by layer: all-taps 3x3 layers (36 / 72 / 144 channels),
    the <= 32-channel variant, generic layers (1x1, 3x3 stride 2, a tiny one that adds with atomics), channel offsets."""
    from checkerpose_amd._abi import CpWgradItem, CpWgradReduceItem
    E = 8 if dtype == CP_BF16 else 4
    layers = [  # (B, Cin, H, W, Cout, k, stride, pad, share of the workgroups)
        (4, 36, 32, 32, 36, 3, 1, 1, 40), (4, 72, 16, 16, 72, 3, 1, 1, 24), (2, 144, 8, 8, 144, 3, 1, 1, 9), (4, 18, 64, 64, 18, 3, 1, 1, 64),
        (4, 18, 32, 32, 18, 3, 1, 1, 16), (4, 36, 32, 32, 18, 1, 1, 0, 12), (4, 18, 64, 64, 36, 3, 2, 1, 30), (2, 144, 8, 8, 72, 1, 1, 0, 6),
        (2, 8, 8, 8, 8, 1, 1, 0, 2), (4, 18, 64, 64, 18, 3, 2, 1, 20), (2, 36, 32, 32, 72, 3, 2, 1, 8), (2, 36, 14, 18, 72, 3, 2, 1, 10)]
    arena = torch.empty(256 << 20, dtype=torch.uint8, device=dev())
    off, keep, comp, red, want, dws = 0, [], {}, [], [], []
    for n, (B, Cin, H, W, Cout, k, stride, pad, share) in enumerate(layers):
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        x_cl = to_cl(rnd(det_tensor("wgg_x%d" % n, (B, Cin, H, W)), dtype), dtype)
        dy_cl = to_cl(rnd(det_tensor("wgg_d%d" % n, (B, Cout, Ho, Wo)), dtype), dtype)
        want.append(_wgrad(lib, dtype, dy_cl, x_cl, Cout, Cin, k, k, stride, pad, 0, 0, True))
        dw = torch.zeros(Cout, Cin, k, k, dtype=torch.float32, device=dev())
        d = CpWgradDesc()
        d.dtype, d.B, d.H, d.W, d.Ho, d.Wo = dtype, B, H, W, Ho, Wo
        d.Cout, d.dy_cstride, d.dy_coff, d.Cin, d.x_cstride, d.x_coff = Cout, dy_cl.shape[-1], 0, Cin, x_cl.shape[-1], 0
        d.R, d.S, d.stride, d.pad = k, k, stride, pad
        d.dw_base, d.dw_sco, d.dw_sci, d.dw_sr, d.dw_ss = 0, Cin * k * k, k * k, k, 1
        ci, ri = CpWgradItem(), CpWgradReduceItem()
        _abi.check(lib.cp_conv2d_wgrad_item(C.byref(d), dy_cl.data_ptr(), x_cl.data_ptr(), dw.data_ptr(), arena.data_ptr() + off, arena.numel() - off,
                                            share, C.byref(ci), C.byref(ri)), "wgrad item")
        assert ci.blocks == ci.gx * ci.gy and ci.blocks > 0
        if dtype == CP_BF16 and k == 3 and W % 16 == 0:                      # all-taps kinds: 0 / 1 at stride 1, 4 at stride 2 (narrow layers only)
            want_kind = (1 if max(Cin, Cout) <= 32 else 0) if stride == 1 else (4 if max(Cin, Cout) <= 32 else 2)
            assert ci.kind == want_kind and ci.blocks <= max(share, ci.gy) * (9 if want_kind == 2 else 1)
        if ri.ws:
            off += (ri.S * ri.GY * ri.taps_in_block * 4096 * 4 + 255) // 256 * 256
            red.append(ri)
        comp.setdefault(int(ci.kind), []).append(ci)
        keep += [x_cl, dy_cl, d]
        dws.append(dw)
    assert off <= arena.numel()
    for kind, items in sorted(comp.items()):
        arr = (CpWgradItem * len(items))(*items)
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev())
        pre = [0]
        for it in items:
            pre.append(pre[-1] + it.blocks)
        prefix = torch.tensor(pre, dtype=torch.int32, device=dev())
        _abi.check(lib.cp_wgrad_group(st(), kind, raw.data_ptr(), prefix.data_ptr(), len(items), pre[-1]), "cp_wgrad_group")
        keep += [raw, prefix]
    arr = (CpWgradReduceItem * len(red))(*red)
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev())
    pre = [0]
    for it in red:
        pre.append(pre[-1] + lib.cp_wgrad_reduce_item_blocks(C.byref(it)))
    prefix = torch.tensor(pre, dtype=torch.int32, device=dev())
    _abi.check(lib.cp_wgrad_reduce_batch(st(), raw.data_ptr(), prefix.data_ptr(), len(red), pre[-1]), "reduce batch")
    torch.cuda.synchronize()
    assert len(red) < len(layers)                    # the tiny layer added with atomics
    for n, (dw, w) in enumerate(zip(dws, want)):
        sc = float(w.abs().max()) + 1e-30
        assert float((dw.cpu() - w).abs().max()) / sc < 1e-5, layers[n]
    assert lib.cp_wgrad_group(st(), 9, raw.data_ptr(), prefix.data_ptr(), 1, 1) != 0


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_bn_group_launches_equal_the_single_layer_launches(lib, dtype):
    """cp_bn_group (the four BatchNorm passes of several independent layers, one launch per pass over a device table of cp_bn_item_*
    parameter blocks) against the single-layer launches on the same inputs -- the shapes of an HRNet stage-4 module at the training
    batch (18/36/72/144 channels at 64/32/16/8 squared), with and without a residual, ReLU / LeakyReLU / no activation, a channel
    slice of a wider buffer, and a bias-only layer (raw NULL) in the backward.  Same block plan and arithmetic per item: the apply
    passes are bit-identical given equal sums; the fp64 atomics may land in another order (last-bit differences in the sums)."""
    from checkerpose_amd._abi import CpBnItem, CP_BN_ITEM_STATS, CP_BN_ITEM_APPLY, CP_BN_ITEM_BWD_SUMS, CP_BN_ITEM_BWD_APPLY
    import ctypes as C
    B = 8
    cases = [(18, 64, ACT_RELU, True, 0), (36, 32, ACT_RELU, False, 0), (72, 16, ACT_LEAKY, True, 0), (144, 8, ACT_NONE, False, 0),
             (18, 32, ACT_RELU, True, 24)]                     # last: channels [24, 42) of a 48-channel buffer
    E = 8 if dtype == CP_BF16 else 4
    L = []
    for n, (Cc, H, act, has_res, coff) in enumerate(cases):
        M = B * H * H
        x = rnd(det_tensor("bg_x%d" % n, (B, Cc, H, H)) * 1.5 + 0.3, dtype)
        xc = to_cl(x, dtype)
        if coff:                                             # embed in a wider buffer
            wide = torch.zeros(B, H, H, 48, dtype=xc.dtype, device=dev())
            wide[..., coff:coff + xc.shape[-1]] = xc
            xc, cs = wide, 48
        else:
            cs = xc.shape[-1]
        rc_ = to_cl(rnd(det_tensor("bg_r%d" % n, (B, Cc, H, H)), dtype), dtype) if has_res else None
        dyc0 = to_cl(rnd(det_tensor("bg_d%d" % n, (B, Cc, H, H)), dtype), dtype)
        L.append(dict(C=Cc, M=M, act=act, xc=xc, cs=cs, coff=coff, rc=rc_, dyc0=dyc0, g=(1.0 + 0.5 * det_tensor("bg_g%d" % n, (Cc,))).to(dev()),
                      b=(0.2 * det_tensor("bg_b%d" % n, (Cc,))).to(dev()), nacc=lib.cp_bn_acc_doubles(Cc)))
    Cb, Mb = 24, B * 16 * 16                                  # a bias-only layer's backward (no BatchNorm input): raw NULL, no dgamma
    dyb0 = to_cl(rnd(det_tensor("bg_db", (B, Cb, 16, 16)), dtype), dtype)
    yb = to_cl(rnd(det_tensor("bg_yb", (B, Cb, 16, 16)), dtype), dtype)

    def group(kind, items):
        arr = (CpBnItem * len(items))(*items)
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev())
        pre = [0]
        for it in items:
            assert it.kind == kind and it.dtype == dtype and it.blocks > 0
            pre.append(pre[-1] + it.blocks)
        prefix = torch.tensor(pre, dtype=torch.int32, device=dev())
        _abi.check(lib.cp_bn_group(st(), dtype, kind, raw.data_ptr(), prefix.data_ptr(), len(items), pre[-1], max(it.lds_bytes for it in items)),
                   "cp_bn_group")
        torch.cuda.synchronize()

    def run(grouped):
        S = []
        for l in L:
            Cc = l["C"]
            S.append(dict(rm=torch.zeros(Cc, device=dev()), rv=torch.ones(Cc, device=dev()), mean=_vec(Cc), rstd=_vec(Cc),
                          acc=torch.zeros(2, l["nacc"], dtype=torch.float64, device=dev()), yc=torch.zeros_like(l["dyc0"]), dyc=l["dyc0"].clone(),
                          dres=torch.zeros_like(l["dyc0"]) if l["rc"] is not None else None, dg=torch.zeros(Cc, device=dev()),
                          db=torch.zeros(Cc, device=dev())))
        accb = torch.zeros(lib.cp_bn_acc_doubles(Cb), dtype=torch.float64, device=dev())
        dyb, dbb = dyb0.clone(), torch.zeros(Cb, device=dev())
        ycs = S[0]["yc"].shape[-1]

        def a_stats(l, s):
            return (dtype, l["xc"].data_ptr(), l["M"], l["C"], l["cs"], l["coff"], s["acc"][0].data_ptr())

        def a_apply(l, s):
            rp = l["rc"].data_ptr() if l["rc"] is not None else None
            return (dtype, l["xc"].data_ptr(), l["cs"], l["coff"], s["acc"][0].data_ptr(), l["g"].data_ptr(), l["b"].data_ptr(), s["rm"].data_ptr(),
                    s["rv"].data_ptr(), 0.1, 1e-5, rp, s["yc"].shape[-1], 0, s["yc"].data_ptr(), s["yc"].shape[-1], 0, l["M"], l["C"], l["act"], 0.2,
                    s["mean"].data_ptr(), s["rstd"].data_ptr())

        def a_bsums(l, s):
            w = s["yc"].shape[-1]
            return (dtype, s["dyc"].data_ptr(), w, 0, s["yc"].data_ptr(), w, 0, l["xc"].data_ptr(), l["cs"], l["coff"], s["mean"].data_ptr(),
                    s["rstd"].data_ptr(), l["M"], l["C"], l["act"], 0.2, s["acc"][1].data_ptr())

        def a_bapply(l, s):
            w = s["yc"].shape[-1]
            drp = s["dres"].data_ptr() if s["dres"] is not None else None
            return (dtype, s["dyc"].data_ptr(), w, 0, s["yc"].data_ptr(), w, 0, l["xc"].data_ptr(), l["cs"], l["coff"], s["mean"].data_ptr(),
                    s["rstd"].data_ptr(), l["g"].data_ptr(), s["acc"][1].data_ptr(), l["M"], l["C"], l["act"], 0.2, s["dyc"].data_ptr(), w, 0,
                    drp, w, 0, 1, s["dg"].data_ptr(), s["db"].data_ptr())
        wb = dyb.shape[-1]
        bias_sums = (dtype, dyb.data_ptr(), wb, 0, yb.data_ptr(), wb, 0, None, 0, 0, None, None, Mb, Cb, ACT_LEAKY, 0.1, accb.data_ptr())
        bias_apply = (dtype, dyb.data_ptr(), wb, 0, yb.data_ptr(), wb, 0, None, 0, 0, None, None, None, accb.data_ptr(), Mb, Cb, ACT_LEAKY, 0.1,
                      dyb.data_ptr(), wb, 0, None, 0, 0, 1, None, dbb.data_ptr())
        if grouped:
            def items(fn, argsets):
                out = []
                for a in argsets:
                    it = CpBnItem()
                    _abi.check(fn(*(a + (C.byref(it),))), "item")
                    out.append(it)
                return out
            group(CP_BN_ITEM_STATS, items(lib.cp_bn_item_stats, [a_stats(l, s) for l, s in zip(L, S)]))
            group(CP_BN_ITEM_APPLY, items(lib.cp_bn_item_apply, [a_apply(l, s) for l, s in zip(L, S)]))
            group(CP_BN_ITEM_BWD_SUMS, items(lib.cp_bn_item_bwd_sums, [a_bsums(l, s) for l, s in zip(L, S)] + [bias_sums]))
            group(CP_BN_ITEM_BWD_APPLY, items(lib.cp_bn_item_bwd_apply, [a_bapply(l, s) for l, s in zip(L, S)] + [bias_apply]))
        else:
            for l, s in zip(L, S):
                a = a_stats(l, s)
                _abi.check(lib.cp_bn_stats_accumulate(st(), *a), "stats")
                _abi.check(lib.cp_bn_apply(st(), *a_apply(l, s)), "apply")
                _abi.check(lib.cp_bn_bwd_accumulate(st(), *a_bsums(l, s)), "bwd sums")
                _abi.check(lib.cp_bn_bwd_apply(st(), *a_bapply(l, s)), "bwd apply")
            _abi.check(lib.cp_bn_bwd_accumulate(st(), *bias_sums), "bias sums")
            _abi.check(lib.cp_bn_bwd_apply(st(), *bias_apply), "bias apply")
        torch.cuda.synchronize()
        out = []
        for s in S:
            out += [s[k].float().cpu() for k in ("yc", "dyc", "mean", "rstd", "rm", "rv", "dg", "db")] + ([s["dres"].float().cpu()] if s["dres"] is not None else [])
        return out + [dyb.float().cpu(), dbb.cpu()]

    ref = run(False)
    for _ in range(2):
        got = run(True)
        assert len(got) == len(ref)
        for a, b in zip(got, ref):
            sc = float(b.abs().max()) + 1e-12
            assert float((a - b).abs().max()) <= (2e-2 if dtype == CP_BF16 else 2e-5) * sc
    # the host-side item builders run the single-layer entry points' checks
    it = CpBnItem()
    x = L[0]["xc"]
    accz = torch.zeros(512, dtype=torch.float64, device=dev())
    S_ptr = accz.data_ptr()
    assert lib.cp_bn_item_stats(dtype, x.data_ptr(), 0, 18, x.shape[-1], 0, S_ptr, C.byref(it)) != 0
    assert lib.cp_bn_item_stats(dtype, x.data_ptr(), 64, 18, x.shape[-1], 3, S_ptr, C.byref(it)) != 0          # channel offset off the vector grid
    assert lib.cp_bn_group(st(), dtype, 7, x.data_ptr(), x.data_ptr(), 1, 1, 0) != 0
    assert lib.cp_bn_group(st(), dtype, 0, x.data_ptr(), x.data_ptr(), 17, 1, 0) != 0                           # more than CP_BN_GROUP_MAX items


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_pack_batch_matches_single_launch_packers(lib, dtype):
    """cp_pack_batch (one launch over a device table of items) produces bit-identical images to the single-launch entry points
    for every item kind: generic (plain, row-mapped, ConvTranspose phase), halo small / regular / wide, GEMM, dgrad view,
    EdgeConv views, float copy"""
    from checkerpose_amd._abi import CpPackItem
    d = dev()
    E = 8 if dtype == CP_BF16 else 4
    es = 2 if dtype == CP_BF16 else 4
    items, expect, keep = [], [], []

    def W(name, shape):
        t = det_tensor(name, shape).to(d).contiguous()
        keep.append(t)
        return t

    def out_bytes(n):
        t = torch.full((n,), 0x5A, dtype=torch.uint8, device=d)
        keep.append(t)
        return t

    # generic: plain 3x3, row-mapped 1x1, transposed phase 3
    for (co, ci, r, s, tr, ph, rmap, rows) in [(36, 18, 3, 3, 0, 0, None, 36), (7, 64, 1, 1, 0, 0, [0, 1, 2, 3, -1, -1, -1, 4, 5, 6], 10),
                                               (24, 40, 2, 2, 1, 3, None, 24)]:
        w = W("pb_g%d%d" % (co, tr), (ci, co, 3, 3) if tr else (co, ci, r, s))
        cphys = rup(ci, E)
        nb = lib.cp_packed_weight_bytes(dtype, rows, cphys, r, s)
        a, b = out_bytes(nb), out_bytes(nb)
        rm = torch.tensor(rmap, dtype=torch.int32, device=d) if rmap else None
        keep.append(rm)
        _abi.check(lib.cp_pack_conv_weight(st(), dtype, w.data_ptr(), co, ci, r, s, cphys, tr, ph, rm.data_ptr() if rmap else None, rows, a.data_ptr()))
        it = CpPackItem()
        _abi.check(lib.cp_pack_item_conv(dtype, w.data_ptr(), co, ci, r, s, cphys, tr, ph, rm.data_ptr() if rmap else None, rows, b.data_ptr(), C.byref(it)))
        items.append(it); expect.append((a, b))
    for co, ci in [(18, 18), (72, 36), (128, 64), (256, 32)]:          # halo: small, small, regular, wide
        w = W("pb_h%d" % co, (co, ci, 3, 3))
        cphys = rup(ci, E)
        nb = lib.cp_packed_halo_weight_bytes(dtype, co, cphys)
        a, b = out_bytes(nb), out_bytes(nb)
        _abi.check(lib.cp_pack_conv3x3_halo_weight(st(), dtype, w.data_ptr(), co, ci, cphys, a.data_ptr()))
        it = CpPackItem()
        _abi.check(lib.cp_pack_item_halo(dtype, w.data_ptr(), co, ci, cphys, b.data_ptr(), C.byref(it)))
        items.append(it); expect.append((a, b))
    w = W("pb_gemm", (200, 96))
    nb = lib.cp_packed_gemm_weight_bytes(dtype, 200, 96)
    a, b = out_bytes(nb), out_bytes(nb)
    _abi.check(lib.cp_pack_gemm_weight(st(), dtype, w.data_ptr(), 200, 96, 96, a.data_ptr()))
    it = CpPackItem()
    _abi.check(lib.cp_pack_item_gemm(dtype, w.data_ptr(), 200, 96, 96, b.data_ptr(), C.byref(it)))
    items.append(it); expect.append((a, b))
    w = W("pb_dg", (24, 16, 3, 3))
    a, b = out_bytes(24 * 16 * 9 * 4), out_bytes(24 * 16 * 9 * 4)
    _abi.check(lib.cp_weight_dgrad(st(), w.data_ptr(), 24, 16, 3, 3, a.data_ptr()))
    it = CpPackItem()
    _abi.check(lib.cp_pack_item_dgrad_view(w.data_ptr(), 24, 16, 3, 3, b.data_ptr(), C.byref(it)))
    items.append(it); expect.append((a, b))
    w = W("pb_ev", (24, 32))
    for mode in (0, 1):
        a, b = out_bytes(2 * 24 * 16 * 4), out_bytes(2 * 24 * 16 * 4)
        _abi.check(lib.cp_edge_weight_view(st(), w.data_ptr(), 24, 16, mode, a.data_ptr()))
        it = CpPackItem()
        _abi.check(lib.cp_pack_item_edge_view(w.data_ptr(), 24, 16, mode, b.data_ptr(), C.byref(it)))
        items.append(it); expect.append((a, b))
    src = W("pb_cp", (37,))
    a, b = out_bytes(37 * 4), out_bytes(37 * 4)
    a.copy_(src.view(torch.uint8).flatten())
    it = CpPackItem()
    _abi.check(lib.cp_pack_item_copy_f32(src.data_ptr(), b.data_ptr(), 37, C.byref(it)))
    items.append(it); expect.append((a, b))

    arr = (CpPackItem * len(items))(*items)
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(d)
    pre, acc = [0], 0
    for it in items:
        acc += (int(it.total) + 255) // 256
        pre.append(acc)
    prefix = torch.tensor(pre, dtype=torch.int64).to(torch.int32).to(d)
    _abi.check(lib.cp_pack_batch(st(), dtype, tab.data_ptr(), prefix.data_ptr(), len(items), acc), "pack batch")
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(expect):
        assert torch.equal(a, b), "item %d (kind %d) differs from its single-launch packer" % (k, items[k].kind)
    assert es in (2, 4)


# ---- deterministic mode (cp_set_deterministic): the same comparisons as above on the fixed-order forms
def _deterministic(on):
    import checkerpose_amd
    was = checkerpose_amd.is_deterministic()
    checkerpose_amd.set_deterministic(on)
    return was


WGRAD_DET_CASES = [
    (2, 18, 16, 24, 36, 3, 1, 1),      # 18-channel small layers: below atomics_max, so the default mode never takes them through the workspace
    (2, 18, 16, 16, 18, 3, 2, 1),
    (5, 18, 8, 8, 18, 3, 1, 1),
    (2, 144, 8, 8, 18, 1, 1, 0),       # fuse 1x1
    (1, 16, 40, 40, 10, 7, 2, 3),      # 7x7 stem
    (2, 72, 64, 64, 144, 3, 1, 1),     # all-taps 3x3
    (16, 32, 32, 32, 32, 3, 1, 1),     # many pixel slices
]


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", WGRAD_DET_CASES)
def test_wgrad_deterministic_vs_torch_autograd(lib, dtype, case):
    """cp_conv2d_wgrad_ws in deterministic mode: every layer, however small, goes through partial tiles in the workspace and the
    fixed-order reduce launch (the default mode adds small layers with atomics even when it is given a workspace) -- against the same
    torch-autograd reference and TOLT as test_wgrad_vs_torch_autograd; two calls bit-identical; without a workspace the call is refused.
    measured (MI355X): max |err| / (max |ref| + |ref|) 2.3e-7 .. 9.3e-7 in fp32, 7.2e-8 .. 4.0e-7 in bf16."""
    assert case in WGRAD_CASES
    B, Cin, H, W, Cout, k, stride, pad = case
    x = rnd(det_tensor("wx%s" % (case,), (B, Cin, H, W)), dtype)
    w = det_tensor("ww%s" % (case,), (Cout, Cin, k, k), 0.1).requires_grad_(True)
    with torch.enable_grad():
        y = F.conv2d(x, w, None, stride, pad)
    dy = rnd(det_tensor("wd%s" % (case,), tuple(y.shape)), dtype)
    (ref,) = torch.autograd.grad(y, w, dy)
    dyc, xc = to_cl(dy, dtype), to_cl(x, dtype)
    was = _deterministic(True)
    try:
        got = _wgrad(lib, dtype, dyc, xc, Cout, Cin, k, k, stride, pad, 0, 0, True)
        again = _wgrad(lib, dtype, dyc, xc, Cout, Cin, k, k, stride, pad, 0, 0, True)
        with pytest.raises(RuntimeError, match=r"code -1\)"):                # CP_ERR_INVALID: no atomics in this mode (wgrad.hip)
            _wgrad(lib, dtype, dyc, xc, Cout, Cin, k, k, stride, pad, 0, 0, False)
    finally:
        _deterministic(was)
    scale = ref.abs().max().item()
    err = ((got.double() - ref.double()).abs() / (scale + ref.double().abs())).max().item()
    print("wgrad deterministic %s %s: max rel err %.2e" % ("bf16" if dtype == CP_BF16 else "fp32", case, err))
    close(got / scale, ref / scale, TOLT[dtype])
    assert torch.equal(got, again)


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", [(2, 18, 16, 16, ACT_RELU, True), (3, 64, 8, 8, ACT_LEAKY, False), (2, 36, 32, 32, ACT_RELU, False),
                                  (3, 18, 40, 40, ACT_RELU, True)])
def test_bn_two_launch_forms_deterministic(lib, dtype, case):
    """the two-launch BatchNorm forms in deterministic mode (64 accumulator sets, at most 64 blocks, each block alone in its set, the
    consumers add the sets in index order): the assertions of test_bn_two_launch_forms against torch autograd, with the accumulators
    sized by cp_bn_acc_doubles AFTER the mode is set (the size depends on it), and two runs bit-identical down to the fp64 sums.
    The last shape has 4800 rows: the default plan would cut it into 75 blocks, so the 64-block cap is in force (75 rows per block,
    ragged against the rows-per-pass of a block)."""
    B, Cc, H, W, _, _ = case
    if H == 40:
        assert B * H * W // 64 > 64
    acc_default = lib.cp_bn_acc_doubles(Cc)
    was = _deterministic(True)
    try:
        assert lib.cp_bn_acc_doubles(Cc) == 64 * 2 * rup(Cc, 16) and lib.cp_bn_acc_doubles(Cc) > acc_default
        a = _bn_two_launch(lib, dtype, case)
        b = _bn_two_launch(lib, dtype, case)
    finally:
        _deterministic(was)
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
