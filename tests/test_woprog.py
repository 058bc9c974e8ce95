"""CPU: the woProg ablation PoseNet_GNNskip_ABwoProg (reference model/pipeline_lm.py:430-517) -- the drop-in's containers, its
constructor / forward errors, the new C-ABI symbols' argument validation, and this file's oracle (composed from the blocks in
oracle/checkerpose_oracle.py) against the reference-made fixture e2e_lm_woprog_injected.npz."""
import ctypes as C
import json
import os

import pytest
import torch

from checkerpose_amd import _abi
from checkerpose_amd.synthetic import build_woprog, lm_p3d
from oracle import checkerpose_oracle as O
from tests.common import GOLDEN, golden, inject_feats


def woprog_oracle(sd, img, knn_idx, npoint=512, res_log2=6, n_graph=3, slope=0.01, graph_slope=0.2, stage=None, img_feats=None):
    """PoseNet_GNNskip_ABwoProg.forward (pipeline_lm.py:480-517) from the oracle's blocks; knn_idx = the per-sample (B, N, K) table"""
    r = res_log2
    active = stage if stage is not None else r - 3
    _, feats, g = O.init_net_forward(sd, "init_net.", img, knn_idx, npoint, "hrnet_w18", 2, 0.2, img_feats)
    f = feats[-1]
    for i in range(active):
        if i > 0:
            f = torch.cat([f, feats[-i - 1]], dim=1)
        f = O.upsample_module(sd, "up_net.%d" % i, f, is_convtrans=(i == 0))
        g = O.mlp_leaky(sd, "refine_net.%d.pre_graph_module" % i, g.permute(0, 2, 1), (0, 2), slope, True).permute(0, 2, 1)
        for j in range(n_graph):
            g = O.static_graph_module(sd, "refine_net.%d.pre_query_block.%d" % (i, j), g, knn_idx, graph_slope)
    seg = O._conv(sd, "seg_block", f)
    bits = O.mlp_leaky(sd, "query_block.mlps", g.permute(0, 2, 1), (0, 2, 4), slope, False).permute(0, 2, 1)
    xb, yb = bits[:, 1:1 + r], bits[:, 1 + r:1 + 2 * r]
    return (bits[:, 0:1], xb, yb, seg, O.id_from_code_prob(xb), O.id_from_code_prob(yb))


def code_band_ok(xb, yb, band=2e-4):
    """(B, N) masks: every bit of the x (y) code clears |z| > band, so the id is decided the same way on both sides"""
    return (xb.abs() > band).all(1), (yb.abs() > band).all(1)


def test_import_names_of_the_reference_scripts():
    from checkerpose_amd.model.pipeline_lm import PoseNet_GNNskip, PoseNet_GNNskip_ABwoProg, Refine_moduleGNN_ABwoProg  # noqa: F401


def test_state_dict_keys_and_shapes_in_reference_order():
    with open(os.path.join(GOLDEN, "woprog_state_dict_keys.json")) as f:
        ref = [(k, list(s)) for k, s in json.load(f)]
    net = build_woprog()
    # (the fixture's backbone is the parameter-free timm stub: the backbone's own keys are pinned by the existing key tests)
    ours = [(k, list(v.shape)) for k, v in net.state_dict().items() if not k.startswith("init_net.img_backbone.")]
    assert ours == ref
    assert net.init_net.knn_idx is net.refine_net[2].pre_query_block[0].knn_idx     # one shared table


def test_constructor_and_forward_errors():
    from checkerpose_amd.model.init_lm import InitNet_GNN
    from checkerpose_amd.model.pipeline_lm import PoseNet_GNNskip_ABwoProg
    p3d = lm_p3d(512)
    init_net = InitNet_GNN(npoint=512, p3d_normed=p3d, res_log2=4, backbone_name="hrnet_w18", pretrain_backbone=False,
                           max_batch_size=8, num_graph_module=2, graph_k=20, graph_leaky_slope=0.2)
    kw = dict(init_net=init_net, npoint=512, p3d_normed=p3d, local_k=2, num_graph_module=3)
    with pytest.raises(ValueError, match="res_log2"):
        PoseNet_GNNskip_ABwoProg(res_log2=3, **kw)
    with pytest.raises(ValueError, match="query type"):
        PoseNet_GNNskip_ABwoProg(query_type="conv", **kw)
    with pytest.raises(ValueError, match="graph_k"):
        PoseNet_GNNskip_ABwoProg(graph_k=16, **kw)
    net = PoseNet_GNNskip_ABwoProg(res_log2=5, **kw)          # an init net with res_log2 != 3 is fine: its logits are unused
    assert net.query_block.mlps[4].weight.shape == (11, 64)
    with pytest.raises(ValueError, match="stage"):
        net(torch.zeros(1, 3, 256, 256), None, torch.tensor([1]), stage=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(1, 3, 256, 256), None, torch.tensor([1]))


@pytest.mark.parametrize("stage", [None, 2])
def test_composed_oracle_reproduces_reference_fixture(stage):
    g = golden("e2e_lm_woprog_injected")
    net = build_woprog(seed=int(g["seed"]), overrides=g)
    obj = torch.from_numpy(g["obj_ids"]).long()
    with torch.no_grad():
        o = woprog_oracle(net.state_dict(), None, net.init_net.knn_idx[obj - 1], stage=stage,
                          img_feats=inject_feats(3, seed=int(g["feat_seed"])))
    pfx = "" if stage is None else "s2_"
    for a, k in zip(o[:4], ("roi", "xb", "yb", "seg")):
        ref = torch.from_numpy(g[pfx + k])
        assert a.shape == ref.shape, k
        # 1e-5 relative to the block's scale (the fixture's head is scaled to O(1)-O(10) logits: make_golden_woprog.py GAIN)
        assert float((a - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max())), k
    okx, oky = code_band_ok(o[1], o[2])
    assert float(okx.float().mean()) >= 0.99 and float(oky.float().mean()) >= 0.99
    assert torch.equal(o[4][okx], torch.from_numpy(g[pfx + "xid"]).long()[okx])
    assert torch.equal(o[5][oky], torch.from_numpy(g[pfx + "yid"]).long()[oky])


def test_new_abi_symbols_validate_before_launch(lib):
    one = C.c_void_p(16)
    z = (one, one, one, 0.01, one, one, one, 0.01, one, one)
    ok = (_abi.CP_BF16, one, 256, 0, 1, 1) + z
    assert lib.cp_mlp_query_fused_supported(256, 256, 64, 13) == 1 and lib.cp_mlp_query_fused_supported(256, 256, 64, 2) == 1
    assert lib.cp_mlp_query_fused_supported(256, 256, 64, 7) == 0 and lib.cp_mlp_query_fused_supported(256, 256, 64, 17) == 0
    f = lib.cp_mlp_query_fused_n
    assert f(None, *ok, 7, one, 0, 0, 0, 0, None, None, None, None) == -1          # nout outside {2, 9, 11, 13}
    assert f(None, *ok, 13, None, 0, 0, 0, 0, None, None, None, None) == -1        # no output block
    assert f(None, *ok, 13, one, 0, 0, 0, 0, one, None, None, None) == -1          # x ids without y ids
    assert f(None, *ok, 2, one, 0, 0, 0, 0, one, one, None, None) == -1            # ids behind the 2-logit head
    assert f(None, *ok, 13, one, 0, 0, 0, 0, None, None, one, None) == -1          # 32-bit ids without the 64-bit ones
    assert f(None, _abi.CP_F32, *ok[1:], 13, one, 0, 0, 0, 0, None, None, None, None) == -1     # fp32 rows
    assert lib.cp_code_decode(None, one, 13, 7, one, one, None, None, 1, 1) == -1    # 1 + 2r > rows
    assert lib.cp_code_decode(None, one, 13, 6, None, one, None, None, 1, 1) == -1
    assert lib.cp_code_decode(None, one, 13, 6, one, one, None, None, 0, 1) == -1
