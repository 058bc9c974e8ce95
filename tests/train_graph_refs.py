"""The train-mode graph kernels (csrc/train_edge.hip; the EdgeConv backward and the Index2Feat scatter of csrc/train_ops.hip) restated
from their definitions in float64 torch: no GPU, no kernel arithmetic.  tests/test_train_graph_refs.py checks each restatement against
plain torch autograd; tests/test_gpu_train_graph_forms.py holds the device to them.

Channels-last everywhere, as the kernels see their operands: pq (B, N, 2C) = [P | Q], out / gout (B, N, C), neighbour lists PER SAMPLE
(B, N, K) (graphs[graph_ids] for per-sample graphs)."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F


def synthetic_graphs(G, N, K, seed):
    """(G, N, K) int32 neighbour lists that are NOT kNN graphs.  Per graph: one hub node that every row lists (at a slot that moves
    from row to row), two nodes nobody lists (in-degree 0: a row of zeros in the reverse graph, right next to the hub's long row),
    rows with a self loop (i % 3 == 0) and rows without one (i % 3 == 1), rows that list one neighbour twice (i % 4 == 2: a tie of the
    max over K that the first slot must win), other slots uniform over the listed nodes, another draw per graph.  The hub's in-degree
    (>= N) is kept off the multiples of 6: the reverse gather of train_edge.hip walks 6 edges at a time."""
    assert K >= 3 and N >= 12
    out = np.zeros((G, N, K), dtype=np.int64)
    for g in range(G):
        rng = np.random.RandomState(seed * 1000 + g)
        hub, d0, d1 = (int(v) for v in rng.choice(N, 3, replace=False))
        live = np.array([j for j in range(N) if j not in (d0, d1)])
        idx = live[rng.randint(0, len(live), size=(N, K))]
        for i in range(N):
            p = int(rng.randint(K))
            s1, s2 = (p + 1) % K, (p + 2) % K
            if i % 3 == 1 and i != hub:                         # no self loop
                for k in range(K):
                    while idx[i, k] == i:
                        idx[i, k] = live[rng.randint(len(live))]
            idx[i, p] = hub
            if i % 3 == 0 and i not in (d0, d1):                # a self loop (never on the two unlisted nodes)
                idx[i, s1] = i
            if i % 4 == 2:                                      # the same neighbour twice
                idx[i, s2] = idx[i, s1]
        spare = [i for i in range(N) if i % 12 == 11]           # rows with no promise to keep beyond the hub: free slots for the fix-up
        while np.count_nonzero(idx == hub) % 6 == 0:
            i = spare.pop()
            k = int(np.flatnonzero(idx[i] != hub)[0])
            idx[i, k] = hub
        out[g] = idx
    return torch.from_numpy(out).int()


def in_degree(idx):
    """(..., N, K) neighbour lists -> (..., N) number of (i, k) with idx[i, k] == j"""
    N = idx.shape[-2]
    flat = idx.reshape(-1, N * idx.shape[-1]).long()
    deg = torch.zeros(flat.shape[0], N, dtype=torch.long)
    deg.scatter_add_(1, flat, torch.ones_like(flat))
    return deg.reshape(idx.shape[:-2] + (N,))


def _gather_rows(T, idx):
    """T (B, N, C), idx (B, N, K) -> (B, N, K, C): T[b, idx[b, i, k], :]"""
    b = torch.arange(T.shape[0])[:, None, None]
    return T[b, idx.long()]


def first_argmax_slots(P_fp32, idx, scale_fp32):
    """(B, N, C) int64: argmax_k( P[b, idx[b,i,k], c] * scale[c] ) in float32 -- ONE IEEE multiply per candidate and torch.argmax's
    first maximum: the rule of edge_train_fwd_kernel (strict `>` in list order).  scale == 1 is the plain EdgeConv's rule."""
    assert P_fp32.dtype == torch.float32 and scale_fp32.dtype == torch.float32
    v = _gather_rows(P_fp32, idx) * scale_fp32                               # (B, N, K, C)
    return v.argmax(dim=2)


EdgeTrainRef = namedtuple("EdgeTrainRef", "out dpq dgamma dbeta mean var var_unbiased z")


def edge_train_ref(pq, idx_per_sample, gamma, beta, slope, kstar, gout, eps=1e-5, pos=None, band=0.0):
    """float64 autograd of the reference formulation (model/init.py: get_graph_feature -> 1x1 conv -> BatchNorm2d in batch-statistics
    mode -> LeakyReLU -> max over K) on the factored operands:  e[b,i,k,c] = P[b, idx[b,i,k], c] + Q[b,i,c]  ->  F.batch_norm over the
    B*N*K edges  ->  LeakyReLU  ->  selection over K.  The selection is a gather at `kstar` (B, N, C) (FORCE_KSTAR of
    oracle/checkerpose_oracle.py: the max routes its gradient to ONE neighbour, so gradient comparisons pin that choice);
    kstar = None takes the plain max.  LeakyReLU's derivative jumps at 0, and a float32 forward cannot tell the sign of a pre-activation
    z that is smaller than its own rounding error: where |z| <= band, `pos` (B, N, C) bool -- the sign the device's output shows --
    picks the branch (FORCE_MASK of the oracle, confined to that band); everywhere else, and always with pos = None, the branch is
    z > 0.  Returns out (B, N, C), d pq (B, N, 2C), d gamma, d beta, the batch mean, the biased variance, the unbiased variance
    (what the running update uses) and the selected pre-activation z (B, N, C)."""
    C = gamma.numel()
    with torch.enable_grad():
        pq64 = pq.detach().double().requires_grad_(True)
        g64, b64 = gamma.detach().double().requires_grad_(True), beta.detach().double().requires_grad_(True)
        e = _gather_rows(pq64[:, :, :C], idx_per_sample) + pq64[:, :, None, C:]          # (B, N, K, C)
        z = F.batch_norm(e.permute(0, 3, 1, 2), None, None, g64, b64, True, 0.0, eps)    # (B, C, N, K)
        if kstar is None:
            y, at = F.leaky_relu(z, slope).max(dim=-1)
            zs = z.detach().gather(-1, at.unsqueeze(-1)).squeeze(-1)
        else:
            zsel = z.gather(-1, kstar.long().permute(0, 2, 1).unsqueeze(-1)).squeeze(-1)  # leaky after the selection == before it
            zs = zsel.detach()
            up = zs > 0
            if pos is not None:
                up = torch.where(zs.abs() <= band, pos.permute(0, 2, 1), up)
            y = torch.where(up, zsel, zsel * slope)
        out = y.permute(0, 2, 1)                                                          # (B, N, C)
        dpq, dg, db = torch.autograd.grad(out, [pq64, g64, b64], gout.double())
    ed = e.detach()
    n = ed.shape[0] * ed.shape[1] * ed.shape[2]
    mean = ed.mean(dim=(0, 1, 2))
    var = ((ed - mean) ** 2).mean(dim=(0, 1, 2))
    return EdgeTrainRef(out.detach(), dpq, dg, db, mean, var, var * n / max(n - 1, 1), zs.permute(0, 2, 1))


EdgeGatherBwdRef = namedtuple("EdgeGatherBwdRef", "dQ dP kstar deg sum_abs")


def edge_gather_bwd_ref(pq, idx_per_sample, gout, slope):
    """cp_edgeconv_gather_max_bwd:  out = leaky(max_k P[idx] + Q),  dQ = gout * leaky'(out),  dP[j] = sum of dQ over the edges (i, k)
    with idx[i,k] == j that won the max (first maximum: no arithmetic precedes the comparison).  pq float32 holding the storage-rounded
    values, gout float32.  dQ is float32 and EXACT: the sign of max + Q is the sign of the exact sum, gout * slope is one float32
    multiply.  dP is float64; deg (B, N) is the node's in-degree (all its reverse edges, winners or not) and sum_abs (B, N, C) the sum
    of |dQ| over the winners -- what bounds a float32 sum of those terms in any order."""
    assert pq.dtype == torch.float32 and gout.dtype == torch.float32
    B, N, C2 = pq.shape
    C = C2 // 2
    P, Q = pq[:, :, :C], pq[:, :, C:]
    kstar = first_argmax_slots(P, idx_per_sample, torch.ones(C))
    cand = _gather_rows(P, idx_per_sample)                                    # (B, N, K, C)
    m = cand.gather(2, kstar.unsqueeze(2)).squeeze(2)
    pos = (m.double() + Q.double()) > 0
    dQ = torch.where(pos, gout, gout * torch.tensor(slope, dtype=torch.float32))
    win = idx_per_sample.long().gather(2, kstar)                              # (B, N, C): the node that receives dQ[b, i, c]
    dP = torch.zeros(B, N, C, dtype=torch.float64).scatter_add_(1, win, dQ.double())
    sum_abs = torch.zeros(B, N, C, dtype=torch.float64).scatter_add_(1, win, dQ.double().abs())
    return EdgeGatherBwdRef(dQ, dP, kstar, in_degree(idx_per_sample), sum_abs)


Index2FeatBwdRef = namedtuple("Index2FeatBwdRef", "dpatches n sum_abs")


def index2feat_taps(x_id, y_id, mask, Hp, Wp, k):
    """the four taps of every keypoint as the forward (graph_ops.hip) takes them: tap t reads pixel (2 y_id + (t & 1 ? k : 0),
    2 x_id + (t & 2 ? k : 0)); a tap outside the Hp x Wp map or under mask == 0 reads (and so receives) nothing.
    -> y, x (4, B, N) int64 and ok (4, B, N) bool"""
    t = torch.arange(4)[:, None, None]
    y = 2 * y_id.long()[None] + torch.where((t & 1) != 0, k, 0)
    x = 2 * x_id.long()[None] + torch.where((t & 2) != 0, k, 0)
    ok = (mask[None] != 0) & (y >= 0) & (y < Hp) & (x >= 0) & (x < Wp)
    return y, x, ok


def index2feat_bwd_ref(gout, x_id, y_id, mask, Hp, Wp, k):
    """cp_index2feat_gather_bwd_t in float64: dpatches[b, y, x, e] = sum over keypoints i and taps t that land on (y, x) of
    gout[b, i, t*E + e] * mask[b, i].  gout (B, N, 4E) holds the values the kernel reads (rounded to its storage type first).
    Also per output element the number of contributions n (B, Hp, Wp) and the sum of |contribution| (B, Hp, Wp, E)."""
    B, N, E4 = gout.shape
    E = E4 // 4
    y, x, ok = index2feat_taps(x_id, y_id, mask, Hp, Wp, k)
    contrib = (gout.double() * mask.double()[:, :, None]).reshape(B, N, 4, E).permute(2, 0, 1, 3)      # (4, B, N, E)
    b = torch.arange(B)[None, :, None].expand(4, B, N)
    dp = torch.zeros(B, Hp, Wp, E, dtype=torch.float64)
    sa = torch.zeros(B, Hp, Wp, E, dtype=torch.float64)
    n = torch.zeros(B, Hp, Wp, dtype=torch.long)
    dp.index_put_((b[ok], y[ok], x[ok]), contrib[ok], accumulate=True)
    sa.index_put_((b[ok], y[ok], x[ok]), contrib[ok].abs(), accumulate=True)
    n.index_put_((b[ok], y[ok], x[ok]), torch.ones(int(ok.sum()), dtype=torch.long), accumulate=True)
    return Index2FeatBwdRef(dp, n, sa)


def fp32_sum_bound(n, sum_abs):
    """|float32 sum of n terms, in any order, each term at most one rounding away from its exact value  -  the exact sum|
    <= (n + 1) * 2^-24 * sum |term|   (n - 1 additions and one rounding per term, first order; n stays far below 2^24)"""
    return (n.double() + 1.0) * 2.0 ** -24 * sum_abs
