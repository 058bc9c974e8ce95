"""GPU (-m gpu): the train-mode graph kernels at training's batch sizes and call forms, through the C ABI, against the float64
references of tests/train_graph_refs.py (proved against plain torch autograd on the CPU by tests/test_train_graph_refs.py):

  A  cp_edgeconv_train_fwd / cp_edgeconv_train_bwd (csrc/train_edge.hip): sub-blocks of several chunks (the keypoint loop runs more
     than once), the batch tail of the XCD labelling, per-sample graphs, channel slices, K = 1 / 64, both ends of the channel dispatch
  B  cp_edgeconv_gather_max_bwd (csrc/train_ops.hip): per-sample graphs, a gout slice, both ends of pass B's threads-per-node, ragged N
  C  cp_index2feat_gather_bwd_t, atomic and deterministic form: one / two LDS chunks, ragged pixel-quad count, masked crops, ids off the map

The graphs are tests/train_graph_refs.synthetic_graphs: a hub, in-degree 0 nodes, repeated neighbours, rows without a self loop.
Tolerances: TOLT of tests/test_gpu_train_dense.py exactly as test_edgeconv_train_fwd_bwd applies it (A); exactness and the float32
summation bound (n + 1) 2^-24 sum|term| taken from the reference's own counts (B, C).  Nothing is tuned here."""
import pytest
import torch

import checkerpose_amd
from checkerpose_amd import _abi
from checkerpose_amd._abi import CP_BF16, CP_F32
from checkerpose_amd.train_ops import reverse_graph
from tests import train_graph_refs as R
from tests.common import det_tensor
from tests.test_gpu_parity import DT, close, dev, rnd, st
from tests.test_gpu_train_dense import TOLT

pytestmark = pytest.mark.gpu
CP_ERR_INVALID, CP_ERR_ALIGN = -1, -3
NAME = {CP_F32: "fp32", CP_BF16: "bf16"}
ELEMS = {CP_F32: 4, CP_BF16: 8}
EPS, MOMENTUM = 1e-5, 0.1


def relerr(a, b):
    """the figure close() bounds: max |a - b| / (1 + |b|)"""
    a, b = a.double(), b.double()
    return float(((a - b).abs() / (1 + b.abs())).max())


def edge_plan(B, N, KPB):
    """edge_plan() of csrc/train_edge.hip: (S sub-blocks per crop, npb keypoints per sub-block, chunks of KPB keypoints per crop)"""
    chunks = -(-N // KPB)
    s = max(1, min(512 // B, chunks))
    npb = -(-chunks // s) * KPB
    return -(-N // npb), npb, chunks


def random_graphs(G, N, K, seed):
    """(G, N, K) int32 uniform neighbour lists (repeats allowed) for the K the synthetic graphs are not made for"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(0, N, (G, N, K), generator=gen).int()


class EdgeTrain:
    """one train-mode EdgeConv problem on the device: operands, buffers (optionally channel slices of wider ones) and the two calls"""

    def __init__(self, lib, dtype, tag, B, N, C, K, graphs, gids, slope, slices):
        self.lib, self.dtype, self.B, self.N, self.C, self.K, self.slope = lib, dtype, B, N, C, K, slope
        self.G = graphs.shape[0]
        d = dev()
        self.pq = rnd(det_tensor(tag + "_pq", (B, N, 2 * C)), dtype)                         # rounded to the storage type first
        self.gamma = 1.0 + 0.5 * det_tensor(tag + "_g", (C,))
        self.gamma[::3] *= -1                                                                 # negative entries (min / max switch) ...
        self.gamma[1] = 0.0                                                                   # ... and exact zeros: every candidate ties
        self.gamma[C - 2] = 0.0
        self.beta = 0.2 * det_tensor(tag + "_b", (C,))
        self.gout = rnd(det_tensor(tag + "_d", (B, N, C)), dtype)
        self.rm0 = 0.1 * det_tensor(tag + "_m", (C,))
        self.rv0 = 1.0 + 0.3 * det_tensor(tag + "_v", (C,)).abs()
        self.graphs = graphs
        self.idx_ps = (graphs[torch.tensor(gids)] if gids is not None else graphs[:1].expand(B, -1, -1)).long()
        self.pq_d = self.pq.to(DT[dtype]).to(d).contiguous()
        self.idx_d = graphs.int().contiguous().to(d)
        self.gid_d = torch.tensor(gids, dtype=torch.int32, device=d) if gids is not None else None
        self.rev_ptr, self.rev_edge = reverse_graph(self.idx_d)
        self.out_cs, self.out_coff = (C + 32, 16) if slices else (C, 0)
        self.g_cs, self.g_coff = (C + 32, 24) if slices else (C, 0)
        self.out = torch.full((B, N, self.out_cs), 7.0, dtype=DT[dtype], device=d)
        self.gbuf = torch.full((B, N, self.g_cs), float("nan"), dtype=DT[dtype], device=d)
        self.gbuf[:, :, self.g_coff:self.g_coff + C] = self.gout.to(DT[dtype]).to(d)
        self.kstar = torch.full((B, N, C), 255, dtype=torch.uint8, device=d)
        self.vec = [torch.zeros(C, device=d) for _ in range(4)]                               # scale, shift, mean, rstd
        self.g_d, self.b_d = self.gamma.to(d), self.beta.to(d)
        self.rm_d, self.rv_d = self.rm0.to(d), self.rv0.to(d)
        self.dpq = torch.full((B, N, 2 * C), float("nan"), dtype=DT[dtype], device=d)
        self.dg, self.db = torch.zeros(C, device=d), torch.zeros(C, device=d)
        self.ws = torch.empty(lib.cp_edge_train_workspace_bytes(B, C), dtype=torch.uint8, device=d)

    def fwd(self, **o):
        p = lambda t: t.data_ptr() if t is not None else None                                 # noqa: E731
        rc = self.lib.cp_edgeconv_train_fwd(
            st(), self.dtype, p(self.pq_d), p(self.idx_d), p(self.gid_d), p(self.g_d), p(self.b_d), p(self.rm_d), p(self.rv_d), MOMENTUM,
            EPS, p(self.out), o.get("out_cs", self.out_cs), o.get("out_coff", self.out_coff), p(self.kstar), p(self.vec[0]), p(self.vec[1]),
            p(self.vec[2]), p(self.vec[3]), p(self.ws), self.B, self.N, o.get("K", self.K), o.get("C", self.C), self.G, self.slope)
        torch.cuda.synchronize()
        return rc

    def bwd(self, **o):
        p = lambda t: t.data_ptr() if t is not None else None                                 # noqa: E731
        rc = self.lib.cp_edgeconv_train_bwd(
            st(), self.dtype, p(self.pq_d), p(self.idx_d), p(self.rev_ptr), p(self.rev_edge), p(self.gid_d), p(self.out),
            o.get("out_cs", self.out_cs), o.get("out_coff", self.out_coff), p(self.kstar), p(self.gbuf), o.get("g_cs", self.g_cs),
            o.get("g_coff", self.g_coff), p(self.g_d), p(self.vec[2]), p(self.vec[3]), p(self.dpq), p(self.dg), p(self.db), p(self.ws),
            self.B, self.N, o.get("K", self.K), o.get("C", self.C), self.G, self.slope)
        torch.cuda.synchronize()
        return rc

    def check(self, what):
        """both calls against edge_train_ref at the device's own (verified) arg-max slots; prints and returns the observed maxima"""
        C, dtype, tol = self.C, self.dtype, TOLT[self.dtype]
        _abi.check(self.fwd(), "edge train fwd")
        scale, shift, mean, rstd = (v.cpu() for v in self.vec)
        ks = self.kstar.cpu().long()
        want_ks = R.first_argmax_slots(self.pq[:, :, :C].contiguous(), self.idx_ps, scale)
        assert torch.equal(ks, want_ks), "%d arg-max slots differ from the first maximum of P * scale" % int((ks != want_ks).sum())
        wide = self.out.float().cpu()
        out = wide[:, :, self.out_coff:self.out_coff + C]
        # LeakyReLU's branch: the reference's own z > 0, except where |z| is within the float32 forward tolerance of 0 -- there the
        # float32 forward cannot know the sign and the branch the device's output shows is the one its backward must follow
        band = TOLT[CP_F32]
        ref = R.edge_train_ref(self.pq, self.idx_ps, self.gamma, self.beta, self.slope, ks, self.gout, EPS, pos=out > 0, band=band)
        flips = (ref.z > 0) != (out > 0)
        assert not bool((flips & (ref.z.abs() > band)).any())
        if self.out_cs > C:                                                                   # nothing outside the slice was touched
            assert bool((wide[:, :, :self.out_coff] == 7.0).all()) and bool((wide[:, :, self.out_coff + C:] == 7.0).all())
        rstd_ref = 1.0 / torch.sqrt(ref.var + EPS)
        scale_ref = self.gamma.double() * rstd_ref
        saved = {"scale": (scale, scale_ref), "shift": (shift, self.beta.double() - ref.mean * scale_ref), "mean": (mean, ref.mean),
                 "rstd": (rstd, rstd_ref)}
        rm_ref = (1 - MOMENTUM) * self.rm0.double() + MOMENTUM * ref.mean
        rv_ref = (1 - MOMENTUM) * self.rv0.double() + MOMENTUM * ref.var_unbiased                # unbiased over B*N*K
        _abi.check(self.bwd(), "edge train bwd")
        D = self.dpq.float().cpu()
        dP, dQ = D[:, :, :C] + D[:, :, C:], D[:, :, C:]
        s = float(ref.dpq.abs().max())
        sg, sb = float(ref.dgamma.abs().max()), float(ref.dbeta.abs().max())
        seen = {"out": relerr(out, ref.out), "dQ": relerr(dQ / s, ref.dpq[:, :, C:] / s), "dP": relerr(dP / s, ref.dpq[:, :, :C] / s),
                "dgamma": relerr(self.dg.cpu() / sg, ref.dgamma / sg), "dbeta": relerr(self.db.cpu() / sb, ref.dbeta / sb),
                "saved": max(relerr(a, b) for a, b in saved.values()),
                "running": max(relerr(self.rm_d.cpu(), rm_ref), relerr(self.rv_d.cpu(), rv_ref))}
        print("edge_train %s %s B=%d N=%d C=%d K=%d G=%d: " % (what, NAME[dtype], self.B, self.N, C, self.K, self.G)
              + " ".join("%s %.2e" % kv for kv in seen.items())
              + " kstar max %d, signs taken from the device %d (of %d with |z| <= %.0e)" % (int(ks.max()), int(flips.sum()), int((ref.z.abs() <= band).sum()), band))
        close(out, ref.out, tol)
        for a, b in saved.values():
            close(a, b, TOLT[CP_F32])                                                         # float32 vectors in both storage types
        close(self.rm_d.cpu(), rm_ref, 1e-4)                                                  # as test_edgeconv_train_fwd_bwd
        close(self.rv_d.cpu(), rv_ref, 1e-4)
        close(dQ / s, ref.dpq[:, :, C:] / s, tol)
        close(dP / s, ref.dpq[:, :, :C] / s, 2 * tol)
        close(self.dg.cpu() / sg, ref.dgamma / sg, tol)
        close(self.db.cpu() / sb, ref.dbeta / sb, tol)
        assert bool(torch.isfinite(D).all())                                                  # the NaN around a gout slice never got in
        return ks


# ------------------------------------------------------------------------------------------------ A: train-mode EdgeConv
@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_edge_train_sub_blocks_of_several_chunks(lib, dtype):
    """B = 64, N = 100, C = 256, K = 6: 512 / B = 8 sub-blocks for 13 (bf16, KPB = 8) / 25 (fp32, KPB = 4) chunks, so every block walks
    2 / 4 chunks -- the keypoint loop of all four kernels re-stages its neighbour lists between two barriers -- and the last
    sub-block holds 4 keypoints (half a chunk in bf16: idle lanes `continue` past the work and still meet the barriers).  Eight full
    rounds of the XCD labelling.  The plan is recomputed here so that a later change of edge_plan() cannot turn this into a
    single-chunk case unnoticed.
    measured (MI355X), max |err| / (1 + |ref|), gradients scaled by max |d pq|: fp32 out 1.3e-7, dQ 1.5e-8, dP 2.4e-7, dgamma 7.0e-8,
    dbeta 2.9e-8; bf16 out 2.6e-3, dQ 1.6e-4, dP 1.5e-3, dgamma 6.2e-8, dbeta 2.8e-8; saved vectors 5.1e-8, running statistics 4.2e-8;
    all 1 638 400 arg-max bytes equal; ~270 outputs with |z| <= 2e-4, none whose sign differed from the reference's."""
    B, N, C, K = 64, 100, 256, 6
    KPB = 256 // (C // ELEMS[dtype])
    S, npb, chunks = edge_plan(B, N, KPB)
    assert npb > KPB and N % npb != 0 and S < chunks, (S, npb, chunks)
    assert (S, npb) == (7, 16) and N - (S - 1) * npb == 4
    graphs = R.synthetic_graphs(1, N, K, 31)
    EdgeTrain(lib, dtype, "ef_mc", B, N, C, K, graphs, None, 0.2, False).check("multi-chunk")


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_edge_train_graphs_slices_and_batch_tail(lib, dtype):
    """B = 9 (second round of the labelling: one live label, seven blocks per sub-block exit early), three graphs with repeated ids
    (rev_ptr + g (N + 1), rev_edge + g N K, idx + g N K), C = 32 (bottom of the dispatch: tpk = 4 in bf16, 8 in fp32), synthetic graphs;
    out written into channels [16, 48) of a 64-wide buffer of 7.0 (the rest must stay 7.0), gout read from channels [24, 56) of a
    buffer that is NaN elsewhere.
    measured (MI355X): fp32 out 1.2e-7, dQ 2.5e-8, dP 1.4e-7, dgamma 4.3e-8, dbeta 3.6e-8; bf16 out 2.6e-3, dQ 3.4e-4, dP 1.6e-3,
    dgamma 3.6e-8, dbeta 2.1e-8."""
    B, N, C, K = 9, 48, 32, 6
    gids = [2, 0, 1, 1, 2, 0, 0, 2, 1]
    graphs = R.synthetic_graphs(3, N, K, 32)
    EdgeTrain(lib, dtype, "ef_gs", B, N, C, K, graphs, gids, 0.2, True).check("graphs+slices")


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("K", [1, 64])
def test_edge_train_k_extremes(lib, dtype, K):
    """K = 1 (the four-rows-in-flight loops never run; every slot is 0) and K = 64 (the limit: 16 rounds of four rows, arg-max bytes up
    to 63, in-degrees around 64 in the reverse gather); K = 65 is refused by both calls.
    measured (MI355X): K = 1 fp32 out 1.1e-7, dQ 4.6e-8, dP 6.1e-8; bf16 out 2.6e-3, dQ 1.0e-3, dP 1.8e-3; K = 64 fp32 out 1.1e-7,
    dQ 2.4e-8, dP 1.4e-7; bf16 out 2.5e-3, dQ 2.8e-4, dP 1.2e-3; dgamma / dbeta <= 6.0e-8 throughout; arg-max bytes reach 63."""
    B, N, C = 2, 80, 64
    e = EdgeTrain(lib, dtype, "ef_k%d" % K, B, N, C, K, random_graphs(1, N, K, 33 + K), None, 0.2, False)
    ks = e.check("K=%d" % K)
    assert int(ks.max()) == K - 1
    if K == 64:
        assert e.fwd(K=65) == CP_ERR_INVALID and e.bwd(K=65) == CP_ERR_INVALID


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_edge_train_top_of_the_dispatch(lib, dtype):
    """C = 512: tpk = 64 (bf16, 4 keypoints per block) / 128 (fp32, 2 keypoints per block), N = 20, K = 5 (one round of four rows plus
    a tail row), synthetic graph.
    measured (MI355X): fp32 out 1.2e-7, dQ 4.1e-8, dP 9.0e-8, dgamma 5.3e-8, dbeta 3.4e-8; bf16 out 2.9e-3, dQ 8.5e-4, dP 1.8e-3,
    dgamma 5.0e-8, dbeta 3.6e-8."""
    B, N, C, K = 2, 20, 512, 5
    EdgeTrain(lib, dtype, "ef_top", B, N, C, K, R.synthetic_graphs(1, N, K, 34), None, 0.1, False).check("C=512")


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_edge_train_running_statistics_and_saved_vectors(lib, dtype):
    """running_mean / running_var start from non-trivial values and after one call hold (1 - m) old + m new with the UNBIASED variance
    over B*N*K; scale, shift, mean, rstd equal the reference (EdgeTrain.check asserts both in every case of this file -- this is the
    case with so few edges (B*N*K = 126) that the biased variance would miss the same tolerance, with per-sample graphs at a middle
    channel count, and a second call updates the running statistics a second time).
    measured (MI355X), both storage types: saved vectors 5.0e-8, running statistics 4.3e-8 (tolerances 2e-4 and 1e-4)."""
    B, N, C, K = 3, 14, 64, 3
    e = EdgeTrain(lib, dtype, "ef_rs", B, N, C, K, R.synthetic_graphs(2, N, K, 35), [1, 0, 1], 0.2, False)
    e.check("running stats")
    ref = R.edge_train_ref(e.pq, e.idx_ps, e.gamma, e.beta, e.slope, None, e.gout, EPS)
    _abi.check(e.fwd(), "second forward")
    rm, rv, rv_biased = e.rm0.double(), e.rv0.double(), e.rv0.double()
    for _ in range(2):
        rm, rv = (1 - MOMENTUM) * rm + MOMENTUM * ref.mean, (1 - MOMENTUM) * rv + MOMENTUM * ref.var_unbiased
        rv_biased = (1 - MOMENTUM) * rv_biased + MOMENTUM * ref.var
    close(e.rm_d.cpu(), rm, 1e-4)
    close(e.rv_d.cpu(), rv, 1e-4)
    assert relerr(rv_biased, rv) > 2e-4                                       # the check above tells the two variances apart


@pytest.mark.parametrize("dtype", [CP_F32, CP_BF16])
def test_edge_train_refusals(lib, dtype):
    """bf16 C = 16 has no kernel instance (tpk = 2); a channel slice that overruns its row is refused by the forward AND by the
    backward, for `out` and for `gout`.  The backward had no such check (it would have read past the rows of both buffers): this test
    is what added `out_coff + C > out_cstride || gout_coff + C > gout_cstride` to cp_edgeconv_train_bwd."""
    B, N, C, K = 2, 16, 32, 3
    E = ELEMS[dtype]
    e = EdgeTrain(lib, dtype, "ef_rf", B, N, C, K, R.synthetic_graphs(1, N, K, 36), None, 0.2, True)
    _abi.check(e.fwd(), "valid forward")
    _abi.check(e.bwd(), "valid backward")
    if dtype == CP_BF16:
        assert e.fwd(C=16) == CP_ERR_INVALID and e.bwd(C=16) == CP_ERR_INVALID
    assert e.fwd(out_coff=e.out_cs - C + E) == CP_ERR_ALIGN
    assert e.fwd(out_cs=C, out_coff=E) == CP_ERR_ALIGN
    assert e.bwd(out_coff=e.out_cs - C + E) == CP_ERR_ALIGN
    assert e.bwd(out_cs=C, out_coff=E) == CP_ERR_ALIGN
    assert e.bwd(g_coff=e.g_cs - C + E) == CP_ERR_ALIGN
    assert e.bwd(g_cs=C, g_coff=E) == CP_ERR_ALIGN
    assert e.fwd(out_coff=e.out_cs - C) == 0 and e.bwd(out_coff=e.out_cs - C, g_coff=e.g_cs - C) == 0      # flush with the row's end is fine


# ------------------------------------------------------------------------------------------------ B: plain EdgeConv backward
GATHER_CASES = [  # (dtype, B, N, K, C, G, graph ids, gout as a slice)
    (CP_F32, 9, 48, 6, 64, 3, [2, 0, 1, 1, 2, 0, 0, 2, 1], False),      # per-sample graphs, batch tail
    (CP_BF16, 9, 48, 6, 64, 3, [2, 0, 1, 1, 2, 0, 0, 2, 1], False),
    (CP_F32, 3, 50, 6, 64, 1, None, True),                              # gout slice; N = 50 against 16 nodes per block in pass B
    (CP_BF16, 3, 50, 6, 64, 2, [1, 1, 0], True),
    (CP_BF16, 2, 48, 6, 32, 1, None, False),                            # pass B: 8 threads per node, 32 nodes per block, ragged
    (CP_F32, 2, 21, 5, 512, 1, None, False),                            # pass B: 128 threads per node, 2 nodes per block, odd N
]


@pytest.mark.parametrize("case", GATHER_CASES, ids=lambda c: "%s-B%d-N%d-K%d-C%d-G%d%s" % ((NAME[c[0]],) + tuple(c[1:6]) + ("-slice" if c[7] else "",)))
def test_edgeconv_gather_max_bwd_forms(lib, case):
    """cp_edgeconv_gather_max_bwd against edge_gather_bwd_ref: the arg-max bytes and dQ exact (a select and at most one multiply), dP
    within (deg + 1) 2^-24 sum|winning dQ| (a float32 sum in edge order; exactly 0 where nothing won, in-degree 0 included), two calls
    bit-identical, every element of dpq overwritten (it starts as NaN).
    measured (MI355X): dQ and the arg-max bytes exact in all six cases; dP max err 7.1e-7 .. 2.2e-6, at most 0.33 of the bound;
    in-degrees up to 61 next to 2 degree-0 nodes per graph."""
    dtype, B, N, K, C, G, gids, sl = case
    d = dev()
    tag = "eg_%s" % (case[1:6],)
    graphs = R.synthetic_graphs(G, N, K, 41)
    idx_ps = (graphs[torch.tensor(gids)] if gids is not None else graphs[:1].expand(B, -1, -1)).long()
    pq = rnd(det_tensor(tag + "pq", (B, N, 2 * C)), dtype)
    gout = det_tensor(tag + "d", (B, N, C))
    ref = R.edge_gather_bwd_ref(pq, idx_ps, gout, 0.2)
    g_cs, g_coff = (C + 24, 12) if sl else (C, 0)
    gbuf = torch.full((B, N, g_cs), float("nan"), device=d)
    gbuf[:, :, g_coff:g_coff + C] = gout.to(d)
    pq_d = pq.to(DT[dtype]).to(d).contiguous()
    idx_d = graphs.int().contiguous().to(d)
    gid_d = torch.tensor(gids, dtype=torch.int32, device=d) if gids is not None else None
    rev_ptr, rev_edge = reverse_graph(idx_d)
    runs = []
    for _ in range(2):
        dpq = torch.full((B, N, 2 * C), float("nan"), device=d)
        ws = torch.full((lib.cp_edgeconv_bwd_workspace_bytes(B, N, C),), 255, dtype=torch.uint8, device=d)
        _abi.check(lib.cp_edgeconv_gather_max_bwd(st(), dtype, pq_d.data_ptr(), idx_d.data_ptr(), rev_ptr.data_ptr(), rev_edge.data_ptr(),
                                                  gid_d.data_ptr() if gid_d is not None else None, gbuf.data_ptr(), dpq.data_ptr(),
                                                  ws.data_ptr(), B, N, K, C, G, g_cs, g_coff, 0.2), "gather_max_bwd")
        torch.cuda.synchronize()
        runs.append((dpq.cpu(), ws[:B * N * C].cpu().reshape(B, N, C).long()))
    (D, ks), (D2, _) = runs
    assert torch.equal(D, D2)
    assert torch.equal(ks, ref.kstar)
    assert torch.equal(D[:, :, C:], ref.dQ)
    bound = R.fp32_sum_bound(ref.deg[:, :, None], ref.sum_abs)
    err = (D[:, :, :C].double() - ref.dP).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("gather_max_bwd %s: dQ exact, dP max err %.2e, max err / bound %.3f, max in-degree %d, degree-0 nodes %d"
          % (tag, float(err.max()), worst, int(ref.deg.max()), int((ref.deg == 0).sum())))
    assert bool((err <= bound).all())
    assert bool((D[:, :, :C][ref.deg == 0] == 0).all()) and int((ref.deg == 0).sum()) >= 2 * B


def test_edgeconv_gather_max_bwd_refuses_48_channels(lib):
    """C = 48: pass B gives a node C / 4 = 12 threads, which does not divide the 256 of a block"""
    d = dev()
    B, N, K, C = 1, 16, 3, 48
    pq, gout, dpq = torch.zeros(B, N, 2 * C, device=d), torch.zeros(B, N, C, device=d), torch.zeros(B, N, 2 * C, device=d)
    idx_d = R.synthetic_graphs(1, N, K, 42).to(d)
    rev_ptr, rev_edge = reverse_graph(idx_d)
    ws = torch.zeros(lib.cp_edgeconv_bwd_workspace_bytes(B, N, C), dtype=torch.uint8, device=d)
    for dtype, buf in ((CP_F32, pq), (CP_BF16, pq.bfloat16())):
        assert lib.cp_edgeconv_gather_max_bwd(st(), dtype, buf.data_ptr(), idx_d.data_ptr(), rev_ptr.data_ptr(), rev_edge.data_ptr(), None,
                                              gout.data_ptr(), dpq.data_ptr(), ws.data_ptr(), B, N, K, C, 1, C, 0, 0.2) == CP_ERR_ALIGN


# ------------------------------------------------------------------------------------------------ C: Index2Feat scatter
I2F_B, I2F_HP, I2F_K = 3, 17, 2
I2F_CASES = [(512, 8, False), (513, 8, True), (600, 8, False), (600, 64, True)]      # (N, E_ch, gout as a slice)
_I2F_REFS = {}


def i2f_problem(N, E, gdtype):
    """ids in [0, 8) (every pixel collects many contributions), ~40 % of the mask zero, the rest 1.0 or 0.5, crop 1 fully masked, two
    keypoints with an id beyond the map (all four taps outside), one on its last column (two taps inside, two outside); the reference is
    computed once per problem and shared by the atomic and the deterministic run"""
    key = (N, E, gdtype)
    if key not in _I2F_REFS:
        B, Hp = I2F_B, I2F_HP
        gen = torch.Generator().manual_seed(5000 + N + E)
        x_id = torch.randint(0, 8, (B, N), generator=gen).int()
        y_id = torch.randint(0, 8, (B, N), generator=gen).int()
        r = torch.rand(B, N, generator=gen)
        mask = torch.where(r < 0.4, 0.0, torch.where(r < 0.8, 1.0, 0.5)).float()
        mask[1] = 0.0
        x_id[0, 5], y_id[2, 7], x_id[0, 11] = 9, 12, 8
        mask[0, 5] = mask[2, 7] = mask[0, 11] = 1.0
        mask[0, N - 1], mask[2, N - 1] = 1.0, 0.5                                             # the last slots of the last LDS chunk count
        gout = rnd(det_tensor("i2f_g%s" % (key,), (B, N, 4 * E)), gdtype)
        _I2F_REFS[key] = (x_id, y_id, mask, gout, R.index2feat_bwd_ref(gout, x_id, y_id, mask, Hp, Hp, I2F_K))
    return _I2F_REFS[key]


def run_i2f(lib, N, E, gdtype, sl):
    d = dev()
    B, Hp = I2F_B, I2F_HP
    x_id, y_id, mask, gout, ref = i2f_problem(N, E, gdtype)
    g_cs, g_coff = (4 * E + 16, 8) if sl else (4 * E, 0)
    gbuf = torch.full((B, N, g_cs), float("nan"), dtype=DT[gdtype], device=d)
    gbuf[:, :, g_coff:g_coff + 4 * E] = gout.to(DT[gdtype]).to(d)
    x_d, y_d, m_d = x_id.to(d), y_id.to(d), mask.to(d)
    dp = torch.full((B, Hp, Hp, E), float("nan"), device=d)                                   # poisoned: every element must be written
    _abi.check(lib.cp_index2feat_gather_bwd_t(st(), gdtype, gbuf.data_ptr(), x_d.data_ptr(), y_d.data_ptr(), m_d.data_ptr(), dp.data_ptr(),
                                              B, N, Hp, Hp, E, I2F_K, g_cs, g_coff), "index2feat bwd")
    torch.cuda.synchronize()
    return dp.cpu(), ref


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("gdtype", [CP_F32, CP_BF16])
@pytest.mark.parametrize("case", I2F_CASES, ids=lambda c: "N%d-E%d%s" % (c[0], c[1], "-slice" if c[2] else ""))
def test_index2feat_bwd_forms(lib, case, gdtype, det):
    """cp_index2feat_gather_bwd_t, hardware-atomic scatter and deterministic gather (2048 (keypoint, tap) slots per LDS chunk: N = 512 is
    exactly one chunk, 513 and 600 two with a ragged second one; 17 x 17 x 8 channels = 578 pixel-quads, 2.26 blocks): every element
    within (n + 1) 2^-24 sum|contribution| of the float64 scatter (bf16 gout is an exact input), the fully masked crop exactly zero, a
    NaN-filled dpatches fully overwritten, NaN around a gout slice never read; the deterministic form twice, bit-identical.
    measured (MI355X): fp32 gout max err 1.1e-6 .. 1.8e-6, 0.21 .. 0.32 of the bound in both forms; bf16 gout <= 1.2e-7 (0.011 of the
    bound: sums of a few dozen 8-bit significands are nearly exact in float32); up to 35 contributions per pixel, 705 untouched pixels
    (odd coordinates, the masked crop) exactly zero."""
    N, E, sl = case
    was = checkerpose_amd.is_deterministic()
    try:
        checkerpose_amd.set_deterministic(det)
        got, ref = run_i2f(lib, N, E, gdtype, sl)
        again = run_i2f(lib, N, E, gdtype, sl)[0] if det else None
    finally:
        checkerpose_amd.set_deterministic(was)
    assert 4 * N > 2048 or N == 512
    bound = R.fp32_sum_bound(ref.n[..., None], ref.sum_abs)
    err = (got.double() - ref.dpatches).abs()
    assert bool(torch.isfinite(got).all())
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("index2feat_bwd %s %s N=%d E=%d%s: max err %.2e, max err / bound %.3f, contributions per pixel <= %d, untouched pixels %d"
          % ("det" if det else "atomic", NAME[gdtype], N, E, " slice" if sl else "", float(err.max()), worst, int(ref.n.max()),
             int((ref.n == 0).sum())))
    assert bool((err <= bound).all())
    assert bool((got[1] == 0).all()) and int(ref.n[1].sum()) == 0
    assert int(ref.n.max()) >= 8
    if det:
        assert torch.equal(got, again)
