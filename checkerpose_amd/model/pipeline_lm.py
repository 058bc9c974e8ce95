"""Drop-in for reference checkerpose/model/pipeline_lm.py (LM shared estimator): PoseNet_GNNskip (:342-425) whose forward
takes per-sample 1-based `obj_ids`; each sample gathers along its own object's kNN graph (`self.knn_idx[obj_ids-1]`,
pipeline_lm.py:55-57), and the woProg ablation PoseNet_GNNskip_ABwoProg (:430-517, config/lm/*_lm_woProg.txt): no progressive
prediction -- the refinement stages only refine the graph feature and one query head at the top decodes all 1 + 2 * res_log2 bits."""
import torch.nn as nn

from ._runtime import HipForwardMixin
from .pipeline import (IMG_FEATS_DIMS, Index2Feat_module, MLP_QueryNet, PoseNet_GNNskip as _PoseNet_GNNskip,  # noqa: F401
                       Refine_moduleGNN, StaticGraph_module, get_gdrn_upsample_module, get_MLP_leakyReLU_layers, knn)


class PoseNet_GNNskip(_PoseNet_GNNskip):
    LM = True

    def forward(self, img, p3d_normed, obj_ids, stage=None):
        active = stage if stage is not None else self.num_refine_steps
        res = self._run(img, obj_ids, stage=stage)
        return self._outputs(res, active)


class Refine_moduleGNN_ABwoProg(nn.Module):
    """pipeline_lm.py:286-339 container: pre_graph_module (Linear gdim -> qd0 + LeakyReLU, Linear qd0 -> qd0 + LeakyReLU) and the
    EdgeConvs; no Index2Feat, no query head."""

    def __init__(self, npoint, p3d_normed, num_filters=256, max_batch_size=64, query_dims=None, local_k=4,
                 leaky_slope=0.01, num_graph_module=2, graph_k=20, graph_leaky_slope=0.2, query_type="mlp",
                 graph_feat_dim=64, knn_idx=None):
        super().__init__()
        self.npoint = npoint
        if query_type == "mlp":
            self.query_dims = (num_filters, 256, 64) if query_dims is None else tuple(query_dims)
        else:
            raise ValueError("query type {} not supported in Refine_module".format(query_type))   # pipeline_lm.py:304
        self.pre_graph_module = get_MLP_leakyReLU_layers((graph_feat_dim, self.query_dims[0], self.query_dims[0]), True, leaky_slope)
        self.pre_query_block = nn.ModuleList()
        if knn_idx is None:
            knn_idx = knn(p3d_normed, graph_k)
        for _ in range(num_graph_module):
            self.pre_query_block.append(StaticGraph_module(self.query_dims[0], self.query_dims[0], knn_idx, graph_leaky_slope))


class PoseNet_GNNskip_ABwoProg(HipForwardMixin, nn.Module):
    """pipeline_lm.py:430-517.  InitNet runs up to its graph feature (its Linear(64 -> 7) head is discarded by the reference and not
    launched here); refine_net[i] refines the graph feature, up_net[i] feeds only seg_block, and query_block maps the final graph
    feature to 1 + 2 * res_log2 logits whose x / y codes give the ids (from_code_prob_to_id, MSB first)."""
    LM = True

    def __init__(self, init_net, npoint, p3d_normed, res_log2=6, num_filters=256, max_batch_size=64, query_dims=None,
                 seg_output_dim=2, local_k=4, leaky_slope=0.01, num_graph_module=2, graph_k=20, graph_leaky_slope=0.2,
                 query_type="mlp"):
        super().__init__()
        if not 4 <= res_log2 <= 6:
            # res_log2 = 3 has no refinement stage: the 64-channel init feature would meet the num_filters-wide query head, which
            # fails in the reference too; above 6 the (B, 13, N) logit block has no room
            raise ValueError("PoseNet_GNNskip_ABwoProg: res_log2 must be in 4..6")
        if query_type != "mlp":
            raise ValueError("query type {} not supported in Refine_module".format(query_type))   # pipeline_lm.py:476
        if graph_k != init_net.graph_k:
            raise ValueError("PoseNet_GNNskip_ABwoProg: graph_k must equal the init net's (one shared kNN table)")
        self.npoint = npoint
        self.init_net = init_net
        self.res_log2 = res_log2
        self.num_bits = 2 * res_log2 + 1
        self.num_refine_steps = res_log2 - 3
        self.cfg = dict(res_log2=res_log2, num_filters=num_filters, query_dims=tuple(query_dims) if query_dims else None,
                        seg_output_dim=seg_output_dim, local_k=local_k, leaky_slope=leaky_slope,
                        num_graph_module=num_graph_module, graph_slope=graph_leaky_slope)
        feats = IMG_FEATS_DIMS[init_net.backbone_name]
        self.up_net = nn.ModuleList()
        for i in range(self.num_refine_steps):
            if i == 0:
                self.up_net.append(get_gdrn_upsample_module(True, feats[-1], num_filters))
            else:
                self.up_net.append(get_gdrn_upsample_module(False, num_filters + feats[-i - 1], num_filters))
        self.refine_net = nn.ModuleList()
        knn_idx = init_net.knn_idx     # identical table (same points, same k): pipeline_lm.py:313 recomputes it per module
        for i in range(self.num_refine_steps):
            ng = num_graph_module if isinstance(num_graph_module, int) else num_graph_module[i]
            gdim = 64 if i == 0 else (num_filters if query_dims is None else query_dims[0])
            self.refine_net.append(Refine_moduleGNN_ABwoProg(npoint, p3d_normed, num_filters, max_batch_size, query_dims, local_k,
                                                             leaky_slope, ng, graph_k, graph_leaky_slope, query_type, gdim,
                                                             knn_idx=knn_idx))
        self.seg_block = nn.Conv2d(num_filters, seg_output_dim, kernel_size=1, padding=0, bias=True)
        self.query_dims = (num_filters, 256, 64) if query_dims is None else tuple(query_dims)
        self.query_block = MLP_QueryNet(self.query_dims, 3, self.num_bits, leaky_slope)
        self._init_runtime()
        import weakref
        object.__setattr__(init_net, "_owner", weakref.ref(self))     # init_net.load_state_dict() must drop OUR folded weights too

    def _net_cfg(self):
        c = dict(self.cfg)
        c.update(kind="woprog", npoint=self.npoint, backbone=self.init_net.backbone_name,
                 init_num_graph_module=len(self.init_net.pre_query_block),
                 init_graph_slope=self.init_net.graph_leaky_slope, num_conv1x1=getattr(self.init_net, "num_conv1x1", 1))
        return c

    def _knn_table(self):
        return self.init_net.knn_idx

    def _keypoints(self):
        return self.init_net._p3d

    def set_compute_dtype(self, name):
        self.init_net.set_compute_dtype(name)
        return super().set_compute_dtype(name)

    def _outputs(self, res):
        # the logit block holds the query head's rows packed: [roi | x code (r rows, MSB first) | y code (r rows)]
        bits, r = res["bits"], self.res_log2
        return (bits[:, 0:1], bits[:, 1:1 + r], bits[:, 1 + r:1 + 2 * r], res["seg"], res["x64"], res["y64"])

    def _check_call(self, stage):
        if self.npoint > 512:
            raise ValueError("PoseNet_GNNskip_ABwoProg: npoint must be <= 512 (the shipped woProg config uses 512); got %d" % self.npoint)
        if stage is not None and not 1 <= stage <= self.num_refine_steps:
            # stage 0 feeds the 64-channel init feature into the num_filters-wide query head: the reference fails there
            raise ValueError("PoseNet_GNNskip_ABwoProg: stage must be None or in 1..%d" % self.num_refine_steps)

    def forward_injected_feats(self, img, feats, stage=None, obj_ids=None):
        """Test hook: the forward with the backbone's four features GIVEN (NCHW fp32 list, as `img_backbone` returns them in the
        reference) -- how the reference-made `*_injected` goldens were produced.  `img` only supplies B and the size."""
        self._check_call(stage)
        return self._outputs(self._run(img, obj_ids, stage=stage, inject_feats=feats))

    def forward(self, img, p3d_normed, obj_ids, stage=None):
        """pipeline_lm.py:480-517.  `p3d_normed` has no numeric effect (MLP_QueryNet ignores it: pipeline.py:174-180)."""
        self._check_call(stage)
        return self._outputs(self._run(img, obj_ids, stage=stage))
