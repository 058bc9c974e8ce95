"""GPU: the woProg ablation PoseNet_GNNskip_ABwoProg (reference model/pipeline_lm.py:430-517) -- the 1 + 2r-logit query head with
its code decode (cp_mlp_query_fused_n), the eval program against the reference-made fixture and the oracle, the bf16 program's
structure, the training step and hipGraph replay."""
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from checkerpose_amd import _abi
from checkerpose_amd._abi import CP_BF16, CP_F16
from oracle import checkerpose_oracle as O
from tests.common import det_image, det_tensor, golden, inject_feats
from tests.free_running import assert_ids_match_own_logits
from checkerpose_amd.synthetic import build_woprog
from tests.test_woprog import code_band_ok, woprog_oracle

pytestmark = pytest.mark.gpu

TDT = {CP_BF16: torch.bfloat16, CP_F16: torch.float16}
Z0 = struct.unpack("<f", struct.pack("<I", 0x33C00000))[0]       # include/checkerpose_hip.h CP_SIGMOID_HALF_Z0_BITS


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


def _gemm_pack(lib, dtype, w, co, ci):
    buf = torch.empty(lib.cp_packed_gemm_weight_bytes(dtype, co, ci), dtype=torch.uint8, device=dev())
    wd = w.contiguous().to(dev())
    _abi.check(lib.cp_pack_gemm_weight(st(), dtype, wd.data_ptr(), co, ci, ci, buf.data_ptr()))
    torch.cuda.synchronize()
    return buf


def _cmp(out, ref, tol, band=2e-4, min_frac=0.99):
    """logits / seg within tol x the block's scale; ids equal wherever every bit of the code clears `band` on the reference side,
    and that covers at least min_frac of the keypoints (no vacuous pass); at EVERY keypoint, band or not, the returned ids are the
    oracle's code decode of the run's own logits"""
    assert_ids_match_own_logits(out, init_bits=out[1].shape[1])
    for a, b, k in zip(out[:4], ref[:4], ("roi", "xb", "yb", "seg")):
        b = torch.as_tensor(np.asarray(b)) if not torch.is_tensor(b) else b
        a = a.float().cpu()
        assert a.shape == b.shape, k
        err = float((a - b).abs().max())
        assert err <= tol * max(1.0, float(b.abs().max())), (k, err)
    xb, yb = [torch.as_tensor(np.asarray(t)) for t in ref[1:3]]
    okx, oky = code_band_ok(xb, yb, band)
    assert float(okx.float().mean()) >= min_frac and float(oky.float().mean()) >= min_frac
    rx, ry = [torch.as_tensor(np.asarray(t)).long() for t in ref[4:6]]
    assert torch.equal(out[4].cpu()[okx], rx[okx]) and torch.equal(out[5].cpu()[oky], ry[oky])


@pytest.mark.parametrize("dtype", [CP_BF16, CP_F16])
@pytest.mark.parametrize("B,N", [(3, 333), (2, 512)])
def test_query_head_13_with_decode_vs_torch(lib, dtype, B, N):
    """cp_mlp_query_fused_n(nout = 13): logits == the three Linear layers with 16-bit rows / weights / first hidden rows and fp32 from
    there on, written through strides into a wider block; the ids of its epilogue == cp_bits_decode's on the kernel's own logits,
    including logits placed at and just past the sigmoid threshold"""
    net = build_woprog(seed=0)
    sd = net.state_dict()
    w = [sd["query_block.mlps.%d.weight" % j].float() for j in (0, 2, 4)]
    b = [sd["query_block.mlps.%d.bias" % j].float().clone() for j in (0, 2, 4)]
    w[2] = w[2].clone()
    for row, v in ((2, Z0), (5, np.nextafter(np.float32(Z0), np.float32(1)).item()), (8, 0.0), (11, -Z0)):
        w[2][row] = 0.0                       # row's logit == its bias, exactly
        b[2][row] = v
    rnd = lambda t: t.to(TDT[dtype]).float()   # noqa: E731
    x = rnd(det_tensor("wq%d_%d" % (B, N), (B, N, 256)))
    h1 = rnd(F.leaky_relu(x @ rnd(w[0]).t() + b[0], 0.01))
    h2 = F.leaky_relu(h1 @ rnd(w[1]).t() + b[1], 0.01)
    ref = (h2 @ w[2].t() + b[2]).permute(0, 2, 1)            # (B, 13, N)
    wide = torch.zeros(B, N, 320, dtype=TDT[dtype], device=dev())
    wide[..., 64:] = x.to(TDT[dtype]).to(dev())
    pk = [_gemm_pack(lib, dtype, w[0], 256, 256), _gemm_pack(lib, dtype, w[1], 64, 256)]
    ones = [torch.ones(256, device=dev()), torch.ones(64, device=dev())]
    bd = [t.contiguous().to(dev()) for t in b]
    w3 = w[2].contiguous().to(dev())
    blk = torch.full((B, 15, N), 7.0, device=dev())          # rows 1..13 of a 15-row block
    x64, y64 = torch.zeros(B, N, dtype=torch.int64, device=dev()), torch.zeros(B, N, dtype=torch.int64, device=dev())
    x32, y32 = torch.zeros(B, N, dtype=torch.int32, device=dev()), torch.zeros(B, N, dtype=torch.int32, device=dev())
    _abi.check(lib.cp_mlp_query_fused_n(st(), dtype, wide.data_ptr(), 320, 64, B, N, pk[0].data_ptr(), ones[0].data_ptr(),
                                        bd[0].data_ptr(), 0.01, pk[1].data_ptr(), ones[1].data_ptr(), bd[1].data_ptr(), 0.01,
                                        w3.data_ptr(), bd[2].data_ptr(), 13, blk.data_ptr(), N, 15 * N, 1, N,
                                        x64.data_ptr(), y64.data_ptr(), x32.data_ptr(), y32.data_ptr()))
    torch.cuda.synchronize()
    got = blk.cpu()
    assert float((got[:, [0, 14]] - 7.0).abs().max()) == 0.0
    z = got[:, 1:14]
    err = ((z.double() - ref.double()).abs() / (1 + ref.double().abs())).max().item()
    assert err <= 5e-3, err
    for row, v in ((2, Z0), (5, None), (8, 0.0), (11, -Z0)):
        assert torch.equal(z[:, row], torch.full_like(z[:, row], v if v is not None else b[2][row].item()))
    # cp_bits_decode over the same logits in its own (B, 13, N) block: stages -1, 0, 1, 2 give the 6-bit ids
    bits = z.contiguous().to(dev())
    mask = torch.zeros(B, N, device=dev())
    xi, yi = torch.zeros(B, N, dtype=torch.int32, device=dev()), torch.zeros(B, N, dtype=torch.int32, device=dev())
    xr, yr = torch.zeros(B, N, dtype=torch.int64, device=dev()), torch.zeros(B, N, dtype=torch.int64, device=dev())
    for s in (-1, 0, 1, 2):
        _abi.check(lib.cp_bits_decode(st(), bits.data_ptr(), s, mask.data_ptr(), xi.data_ptr(), yi.data_ptr(), xr.data_ptr(),
                                      yr.data_ptr(), B, N))
    xc, yc = torch.zeros_like(xr), torch.zeros_like(yr)
    _abi.check(lib.cp_code_decode(st(), bits.data_ptr(), 13, 6, xc.data_ptr(), yc.data_ptr(), None, None, B, N))
    torch.cuda.synchronize()
    assert torch.equal(x64, xr) and torch.equal(y64, yr) and torch.equal(xc, xr) and torch.equal(yc, yr)
    assert torch.equal(x32.long(), xr) and torch.equal(y32.long(), yr)
    assert torch.equal((x64 >> 4) & 1, (z[:, 2] > Z0).long().to(dev())) and bool(((x64 >> 4) & 1 == 0).all())   # z == Z0 -> bit 0
    assert bool(((x64 >> 1) & 1 == 1).all())                                                                  # just past Z0 -> 1


@pytest.mark.parametrize("selection", ["auto", "per_crop"])
def test_fp32_vs_reference_fixture(lib, selection):
    g = golden("e2e_lm_woprog_injected")
    net = build_woprog(seed=int(g["seed"]), overrides=g).to(dev())
    net.set_kernel_selection(selection)
    obj = torch.from_numpy(g["obj_ids"]).long().to(dev())
    feats = [f.to(dev()) for f in inject_feats(3, seed=int(g["feat_seed"]))]
    img = torch.zeros(3, 3, 256, 256, device=dev())
    for stage, pfx in ((None, ""), (2, "s2_")):
        out = net.forward_injected_feats(img, feats, stage=stage, obj_ids=obj)
        _cmp(out, [g[pfx + k] for k in ("roi", "xb", "yb", "seg", "xid", "yid")], 1e-4)
        again = net.forward_injected_feats(img, feats, stage=stage, obj_ids=obj)     # hipGraph replay == the eager first run
        for a, b in zip(out, again):
            assert torch.equal(a, b)


def test_fp32_full_net_vs_oracle_ragged_stage2_and_inplace_edit(lib):
    net = build_woprog(seed=2)
    obj = torch.tensor([1, 5, 13, 5, 9])
    img = det_image(5, seed=3)
    net = net.to(dev())
    for stage in (None, 2):
        sd = {k: v.cpu() for k, v in net.state_dict().items()}
        with torch.no_grad():
            ref = woprog_oracle(sd, img, net.init_net.knn_idx.cpu()[obj - 1], stage=stage)
        out = net(img.to(dev()), None, obj.to(dev()), stage=stage)
        _cmp(out, ref, 1e-4, min_frac=0.97)
    with torch.no_grad():                                   # an in-place edit: the cached program must see it
        net.query_block.mlps[4].bias.mul_(-1.0)
    sd = {k: v.cpu() for k, v in net.state_dict().items()}
    with torch.no_grad():
        ref = woprog_oracle(sd, img, net.init_net.knn_idx.cpu()[obj - 1])
    _cmp(net(img.to(dev()), None, obj.to(dev())), ref, 1e-4, min_frac=0.97)


KEYPOINT_OPS = ("init_net.conv1x1", "init_net.pre_query_block", "refine_net.", "query_block.", "edge_gather", "code_decode")


@pytest.mark.parametrize("B", [2, 64])
def test_bf16_floors_and_program_structure(lib, B):
    net = build_woprog(seed=1).to(dev())
    obj = torch.tensor([(3 * i) % 13 + 1 for i in range(B)])
    img = det_image(B, seed=4)
    ref32 = net(img.to(dev()), None, obj.to(dev()))
    net.set_compute_dtype("bf16")
    out = net(img.to(dev()), None, obj.to(dev()))
    z16 = torch.cat([out[0], out[1], out[2]], 1).float()
    z32 = torch.cat([ref32[0], ref32[1], ref32[2]], 1)
    agree = float(((z16 > 0) == (z32 > 0)).float().mean())
    rel = float((z16 - z32).abs().mean() / z32.pow(2).mean().sqrt())
    print("woprog bf16 B=%d: bit agreement %.4f, mean |dlogit| / rms %.4f" % (B, agree, rel))
    assert agree >= 0.99 and rel <= 0.02
    again = net(img.to(dev()), None, obj.to(dev()))              # hipGraph replay (the first run was eager) == the eager run
    for a, b in zip(out, again):
        assert torch.equal(a, b)
    pr = [v for k, v in net._programs.items() if k[0] == B and k[3] == "bf16"][0]
    prog = pr["prog"].progs[0]
    ops = [(i, op) for i, op in enumerate(prog.ops) if not isinstance(op[0], str)]
    names = [op[2] for _, op in ops]
    assert not any(n == "decode" for n in names)                  # no cp_bits_decode: InitNet's head is not emitted
    assert not any("init_net.mlp" in n for n in names)
    head = [n for n in names if n.startswith("mlp_fused:query_block") or n.endswith("query_block.mlps.4")]
    assert len(head) == 1, head
    if B == 64:                                                   # fused per-crop regime: head + decode in one launch
        assert head == ["mlp_fused:query_block.mlps.0"]
    assert ("code_decode" in names) == (head != ["mlp_fused:query_block.mlps.0"])     # a decode launch only behind the generic head
    # every keypoint-side op sits on lane 1 (inside the region), and nothing makes lane 1 wait for another lane
    kp = [(n, op[3]) for n, (_, op) in zip(names, ops) if any(t in n for t in KEYPOINT_OPS)]
    assert len(kp) >= 1 + 2 + 3 * (1 + 3) + 1, kp                 # conv1x1, 2 init EdgeConvs, 3 stages x (pair MLP + 3 EdgeConvs), head
    assert all(lane == 1 for _, lane in kp), [x for x in kp if x[1] != 1]
    assert not any(op[0] in ("__sync__", "__wait__") and op[2] == 1 for op in prog.ops)
    # the logit block is written by the head alone: no launch writes it before (or beside) the head
    bits_ptr = pr["io"]["bits"].data_ptr()
    writers = [prog.ops[i][2] for i, (_, w) in sorted(prog._rw.items())
               if not isinstance(prog.ops[i][0], str) and any(t.fixed is not None and t.fixed.data_ptr() == bits_ptr for t in w)]
    assert writers == head, writers


def test_decoder_launches_equal_posenets(lib):
    """up_net -> seg_block comes out of ONE emitter (netbuilder._emit_decoder) for PoseNet_GNNskip and the woProg ablation: with equal
    num_filters, backbone and stage count the decoder's launches -- the skip upsamples, every up_net conv, seg_block -- are the same
    (lane, recorder name) sequence in both programs, whatever each pipeline runs between them on its keypoint lane"""
    from checkerpose_amd.synthetic import build_net
    B = 2
    obj = torch.tensor([4, 11]).to(dev())
    img = det_image(B, seed=4).to(dev())
    seqs = []
    for net in (build_net(512, lm=True), build_woprog()):
        assert (net.cfg["num_filters"], net.init_net.backbone_name, net.num_refine_steps) == (256, "hrnet_w18", 3)
        net = net.to(dev()).set_compute_dtype("bf16")
        net(img, None, obj)
        prog = net.program_for(B).progs[0]
        launches = [(item[2], prog.calls[item[1]][2]) for item in prog.sched if item[0] == "op"]
        seqs.append([(lane, n) for lane, n in launches if "up_net." in n or n == "upsample2x" or "seg_block" in n])
    names = [n for _, n in seqs[0]]
    assert sum("up_net.0.0" in n for n in names) == 4 and all(sum("up_net.%d." % i in n for n in names) >= 2 for i in (1, 2)), names
    assert {lane for lane, _ in seqs[0]} >= {0, 3, 4, 5}              # the chain and the transposed conv's other three phases
    assert seqs[0] == seqs[1], [(a, b) for a, b in zip(*seqs) if a != b]


# the conv_log families (the keys of bench.py's MFMA_KERNELS)
MFMA_FAMILIES = {"conv_igemm", "conv3x3_halo", "conv3x3_halo4", "conv3x3_halo_s", "conv3x3_s2_small", "gemm_rows", "basicblock_fused",
                 "bottleneck_fused", "hr_chain", "hr_fuse_out", "edge_fused", "edge_tiled", "hr_stem", "patch_gather", "mlp_fused"}


@pytest.mark.parametrize("dtype,selection", [("bf16", "per_crop"), ("fp32", "auto")])
def test_conv_log_in_step_with_launches(lib, dtype, selection):
    """What Program._mfma owns, on every program slice: a launch named family:key has the NEXT conv_log row, of that family and key
    (bench.py walks the two lists in step while it times the launches), no row is left over, and prog.flops is the sum of the
    logged flops"""
    from checkerpose_amd.synthetic import build_net
    B = 2
    net = build_net(512).to(dev()).set_compute_dtype(dtype)
    net.set_kernel_selection(selection)
    with torch.no_grad():
        net(det_image(B, seed=4).to(dev()), None)
    progs = net.program_for(B).progs
    assert progs and all(len(p.conv_log) > 0 for p in progs)
    for prog in progs:
        families = MFMA_FAMILIES | {e[5] for e in prog.conv_log}
        log = iter(prog.conv_log)
        for _, _, name in prog.calls:
            fam, _, key = name.partition(":")
            if fam in families:
                e = next(log, None)
                assert e is not None and (e[5], e[0]) == (fam, key), (name, e)
        assert next(log, None) is None
        assert prog.flops == sum(e[4] for e in prog.conv_log)


# ---- training step against torch-CPU autograd over the oracle in train mode (helpers restated from tests/test_gpu_train_step.py:
# the EdgeConv arg-max slots and the (Leaky)ReLU branches the device took are teacher-forced into the oracle -- both are
# discontinuous, and the ~1e-6 forward differences would otherwise route a few near-tie gradients differently)
def _device_kstar(net):
    pr = list(net._train_programs.values())[-1]
    out = {}
    for pfx, d in pr["prog"].debug.items():
        B, N = d["out"].B, d["out"].W
        out[pfx] = d["st"]["kstar"].view(B, N, -1).permute(0, 2, 1).long().cpu().contiguous()
    return out


def _device_masks(net):
    prog = list(net._train_programs.values())[-1]["prog"]
    out = {}
    for key, a in prog.kinks.items():
        if a.tbuf not in prog.grads:
            continue
        v = prog.read_act(a) > 0
        if a.H == 1 and "pre_query_block." in key:
            out[key] = v[:, 0].permute(0, 2, 1).contiguous()
        elif a.H == 1:
            out[key] = v[:, 0].contiguous()
        else:
            out[key] = v.permute(0, 3, 1, 2).contiguous()
    return out


def _oracle_step(net, img, obj, seeds, kstar, masks, stage=None):
    O.FORCE_KSTAR.clear(); O.FORCE_KSTAR.update(kstar)
    O.FORCE_MASK.clear(); O.FORCE_MASK.update(masks)
    try:
        sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
        params = [k for k, _ in net.named_parameters()]
        for k in params:
            sd[k].requires_grad_(True)
        with torch.enable_grad(), O.bn_train():
            outs = woprog_oracle(sd, img, net.init_net.knn_idx[obj - 1], stage=stage)
            grads = torch.autograd.grad(list(outs[:4]), [sd[k] for k in params], seeds, allow_unused=True)
    finally:
        O.FORCE_KSTAR.clear()
        O.FORCE_MASK.clear()
    return outs, dict(zip(params, grads)), sd


def _compare_grads(net, ref_grads, sd_ref, tol_max=5e-4, tol_global=1e-4):
    worst, num, den = (0.0, None), 0.0, 0.0
    for k, p in net.named_parameters():
        g_ref, g = ref_grads[k], p.grad
        if g_ref is None:
            assert g is None or float(g.abs().max()) == 0.0, k
            continue
        assert g is not None, "no gradient for %s" % k
        d = g.cpu().double() - g_ref.double()
        num, den = num + float((d * d).sum()), den + float((g_ref.double() ** 2).sum())
        em = float(d.abs().max()) / max(float(g_ref.abs().max()), 1e-12)
        if em > worst[0]:
            worst = (em, k)
    glob = (num / den) ** 0.5
    print("woprog gradient parity: global rel-L2 %.3e, worst tensor max-norm err %.3e (%s)" % (glob, worst[0], worst[1]))
    assert worst[0] <= tol_max, worst
    assert glob <= tol_global, glob
    nstats = 0
    for k, b in net.named_buffers():
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert float((b.cpu() - sd_ref[k]).abs().max()) <= 1e-4 * (1 + float(sd_ref[k].abs().max())), k
            nstats += 1
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(sd_ref[k]), k
    assert nstats > 0


def test_training_step_vs_oracle_autograd(lib):
    """one train-mode forward + backward: outputs within 2e-4 of the oracle in train mode, every parameter gradient (the 13-row
    head's output layer over the (B, 13, N) gradient block, stage 0's pair MLP with Cin = 64, InitNet's EdgeConvs / conv1x1 / backbone
    reached through the refinement graph) and every BatchNorm running statistic equal to autograd's; init_net.mlp gets none;
    then the eval program of the updated weights against the oracle's eval forward"""
    B = 2
    obj = torch.tensor([4, 11])
    img = det_image(B, seed=5)
    seeds = [det_tensor("g_roi", (B, 1, 512)), det_tensor("g_x", (B, 6, 512)), det_tensor("g_y", (B, 6, 512)),
             det_tensor("g_seg", (B, 2, 64, 64), 0.05)]
    net_cpu = build_woprog(seed=3).train()
    net = build_woprog(seed=3).to(dev()).train()
    with torch.enable_grad():
        res = net(img.to(dev()), None, obj.to(dev()))
        torch.cuda.synchronize()
        masks = _device_masks(net)
        torch.autograd.backward(list(res[:4]), [s.to(dev()) for s in seeds])
    torch.cuda.synchronize()
    outs, ref_grads, sd_ref = _oracle_step(net_cpu, img, obj, seeds, _device_kstar(net), masks)
    for a, b in zip(res[:4], outs[:4]):        # 2e-4 of the block's scale: the logits reach |z| ~ 3 behind 11 train-mode EdgeConvs
        assert float((a.detach().cpu() - b.detach()).abs().max()) <= 2e-4 * max(1.0, float(b.detach().abs().max()))
    okx, oky = code_band_ok(outs[1].detach(), outs[2].detach())
    assert float(okx.float().mean()) >= 0.99 and float(oky.float().mean()) >= 0.99
    assert torch.equal(res[4].cpu()[okx], outs[4][okx]) and torch.equal(res[5].cpu()[oky], outs[5][oky])
    for n, p in net.named_parameters():
        if n.startswith("init_net.mlp."):
            assert p.grad is None, n
    _compare_grads(net, ref_grads, sd_ref)
    net.eval()                                                   # the eval program folds the updated running statistics
    with torch.no_grad():
        ev = net(img.to(dev()), None, obj.to(dev()))
        ref_ev = woprog_oracle({k: v.detach() for k, v in sd_ref.items()}, img, net_cpu.init_net.knn_idx[obj - 1])
    for a, b in zip(ev[:4], ref_ev[:4]):
        assert float((a.cpu() - b).abs().max()) <= 2e-4 * max(1.0, float(b.abs().max()))


def _train_loss(out, gt_x, gt_y):
    """BCE on the roi bit, the x / y codes and the two seg maps (the terms train_lm.py:286-296 sums, with fixed targets)"""
    roi, xb, yb, seg = out[:4]
    l = F.binary_cross_entropy_with_logits(xb, gt_x) + F.binary_cross_entropy_with_logits(yb, gt_y)
    l = l + F.binary_cross_entropy_with_logits(roi[:, 0], torch.ones_like(roi[:, 0]))
    return l + F.binary_cross_entropy_with_logits(seg, torch.zeros_like(seg)) * 0.1


def test_training_determinism_and_adam(lib):
    with torch.enable_grad():              # (earlier tests of the session may leave grad mode off)
        _determinism_and_adam()


def _determinism_and_adam():
    from checkerpose_amd import set_deterministic
    from checkerpose_amd.optim import Adam
    net = build_woprog(seed=3).to(dev())
    net.train()
    B = 2
    obj = torch.tensor([4, 11]).to(dev())
    img = det_image(B, seed=5).to(dev())
    gen = torch.Generator().manual_seed(0)
    gt_x = (torch.rand(B, 6, 512, generator=gen) > 0.5).float().to(dev())
    gt_y = (torch.rand(B, 6, 512, generator=gen) > 0.5).float().to(dev())
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    # deterministic mode: two steps from the same state are bit-identical
    set_deterministic(True)
    try:
        grads = []
        for _ in range(2):
            net.load_state_dict(sd0)
            net.zero_grad(set_to_none=True)
            o = net(img, None, obj)
            _train_loss(o, gt_x, gt_y).backward()
            grads.append([p.grad.clone() for p in net.parameters() if p.grad is not None] + [o[1].detach().clone()])
        assert len(grads[0]) == len(grads[1]) and all(torch.equal(a, b) for a, b in zip(*grads))
    finally:
        set_deterministic(False)
    net.load_state_dict(sd0)
    net.zero_grad(set_to_none=True)
    opt = Adam(net.parameters(), lr=1e-4)
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        loss = _train_loss(net(img, None, obj), gt_x, gt_y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("woprog Adam losses: %.4f -> %.4f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]
    assert net.init_net.mlp.weight.grad is None
