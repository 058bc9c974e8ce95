"""tests/train_graph_refs.py against plain torch (CPU only): the proof that the references, not the kernels, define "right" for
tests/test_gpu_train_graph_forms.py -- and that reverse_graph() (host side of every reverse-graph gather) survives the synthetic graphs."""
import pytest
import torch
import torch.nn.functional as F

from tests import train_graph_refs as R
from tests.common import det_tensor


@pytest.mark.parametrize("G,N,K,seed", [(3, 48, 6, 1), (1, 20, 5, 2), (2, 50, 6, 3), (1, 21, 5, 4), (2, 12, 3, 5)])
def test_synthetic_graphs_have_the_promised_properties(G, N, K, seed):
    idx = R.synthetic_graphs(G, N, K, seed)
    assert idx.shape == (G, N, K) and idx.dtype == torch.int32
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    assert torch.equal(idx, R.synthetic_graphs(G, N, K, seed))                # a function of its arguments
    deg = R.in_degree(idx)
    rows = torch.arange(N)[:, None]
    for g in range(G):
        l = idx[g].long()
        hubs = [j for j in range(N) if bool((l == j).any(dim=1).all())]
        assert hubs, "no node is listed by every row"
        assert int((deg[g] == 0).sum()) >= 2
        srt = l.sort(dim=1)[0]
        assert bool((srt[:, 1:] == srt[:, :-1]).any()), "no row repeats a neighbour"
        self_loop = (l == rows).any(dim=1)
        assert bool(self_loop.any()) and bool((~self_loop).any())
        assert bool(((deg[g] > 6) & (deg[g] % 6 != 0)).any())
        assert int(deg[g][hubs[0]]) >= N and int(deg[g][hubs[0]]) % 6 != 0
        # a degree-0 node next to the hub's long row is what the CSR walk must survive: rev_ptr repeats a value there
        assert int(deg[g].sum()) == N * K
    for a in range(G):
        for b in range(a + 1, G):
            assert not torch.equal(idx[a], idx[b])
    kn = (-(torch.arange(N)[:, None] - torch.arange(N)[None, :]).abs()).topk(K, dim=-1)[1]      # a kNN graph: slot 0 is the node itself
    assert bool((kn[:, 0] == torch.arange(N)).all()) and not bool((idx[0][:, 0].long() == torch.arange(N)).all())


@pytest.mark.parametrize("G,N,K", [(3, 48, 6), (1, 20, 5), (2, 50, 6)])
def test_reverse_graph_on_the_synthetic_graphs(G, N, K):
    """rev_edge[g, rev_ptr[g, j] : rev_ptr[g, j+1]] are exactly the flat edge ids i*K+k with idx[g, i, k] == j, increasing --
    with in-degree 0 (an empty range), repeated neighbours (two edges of one row) and G > 1"""
    from checkerpose_amd.train_ops import reverse_graph
    idx = R.synthetic_graphs(G, N, K, 7)
    rev_ptr, rev_edge = reverse_graph(idx)
    assert rev_ptr.shape == (G, N + 1) and rev_edge.shape == (G, N * K)
    assert rev_ptr.dtype == torch.int32 and rev_edge.dtype == torch.int32
    deg = R.in_degree(idx)
    for g in range(G):
        flat = idx[g].reshape(-1).tolist()
        assert int(rev_ptr[g, 0]) == 0 and int(rev_ptr[g, N]) == N * K
        for j in range(N):
            want = [e for e, v in enumerate(flat) if v == j]
            got = rev_edge[g, int(rev_ptr[g, j]):int(rev_ptr[g, j + 1])].tolist()
            assert got == want, (g, j)
            assert len(want) == int(deg[g, j])
    p2, e2 = reverse_graph(idx[0])                                            # (N, K) form == graph 0
    assert torch.equal(p2[0], rev_ptr[0]) and torch.equal(e2[0], rev_edge[0])


def test_first_argmax_slots_takes_the_first_maximum():
    """ties (a repeated neighbour; equal products; a zero scale, where +0 and -0 tie) go to the lowest slot, as the kernel's strict `>`"""
    P = torch.tensor([[[1.0, -2.0], [3.0, 0.5], [3.0, -0.5], [-1.0, 4.0]]])                    # (1, 4, 2)
    idx = torch.tensor([[[3, 1, 2, 1], [0, 0, 0, 0], [2, 1, 1, 3], [3, 3, 2, 0]]])            # (1, 4, 4)
    k = R.first_argmax_slots(P, idx, torch.tensor([1.0, 1.0]))
    assert k[0, :, 0].tolist() == [1, 0, 0, 2]
    assert k[0, :, 1].tolist() == [0, 0, 3, 0]
    k0 = R.first_argmax_slots(P, idx, torch.tensor([0.0, -1.0]))
    assert k0[0, :, 0].tolist() == [0, 0, 0, 0]                                               # every product is +-0
    assert k0[0, :, 1].tolist() == [2, 0, 0, 3]                                               # negative scale: the minimum of P wins
    # many candidates, many ties: equal to a scalar loop with strict >
    Pq = (det_tensor("fa_p", (2, 30, 8)) * 4).round() / 4
    ix = R.synthetic_graphs(1, 30, 7, 3)[0].long()[None].expand(2, -1, -1)
    sc = torch.tensor([1.0, -1.0, 0.5, 0.0, 2.0, -0.25, 1.0, 3.0])
    got = R.first_argmax_slots(Pq, ix, sc)
    for b in range(2):
        for i in range(30):
            for c in range(8):
                best, ks = -float("inf"), 0
                for kk in range(7):
                    v = float(Pq[b, ix[b, i, kk], c] * sc[c])
                    if v > best:
                        best, ks = v, kk
                assert int(got[b, i, c]) == ks


def _edge_inputs(B, N, C, K, G, seed):
    graphs = R.synthetic_graphs(G, N, K, seed)
    gids = torch.arange(B) % G
    idx = graphs[gids].long()
    pq = det_tensor("er_pq%d" % seed, (B, N, 2 * C))
    gamma = 1.0 + 0.5 * det_tensor("er_g%d" % seed, (C,))
    gamma[::3] *= -1
    beta = 0.2 * det_tensor("er_b%d" % seed, (C,))
    gout = det_tensor("er_d%d" % seed, (B, N, C))
    return pq, idx, gamma, beta, gout


@pytest.mark.parametrize("case", [(3, 24, 8, 5, 2, 0.2), (2, 13, 4, 3, 1, 0.1)])
def test_edge_train_ref_at_the_first_argmax_is_unforced_autograd(case):
    """no ties (rows that repeat a neighbour are de-duplicated here): the gather at first_argmax_slots IS the max, so edge_train_ref equals
    autograd of the reference formulation written the long way (explicit edge tensor, nn-style BatchNorm2d, max over K)"""
    B, N, C, K, G, slope = case
    pq, idx, gamma, beta, gout = _edge_inputs(B, N, C, K, G, 11)
    for i in range(N):                                                        # distinct neighbours per row: a max without ties
        idx[:, i] = (torch.arange(K) * 5 + i) % N
    with torch.enable_grad():
        p = pq.double().requires_grad_(True)
        g, b = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        bi = torch.arange(B)[:, None, None]
        e = (p[:, :, :C][bi, idx] + p[:, :, None, C:]).permute(0, 3, 1, 2)                    # (B, C, N, K)
        mu = e.mean(dim=(0, 2, 3), keepdim=True)
        var = ((e - mu) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        z = (e - mu) / torch.sqrt(var + 1e-5) * g[None, :, None, None] + b[None, :, None, None]
        y = F.leaky_relu(z, slope).max(dim=-1)[0].permute(0, 2, 1)
        want = torch.autograd.grad(y, [p, g, b], gout.double())
    scale = (gamma.double() / torch.sqrt(var.flatten() + 1e-5)).float()
    kstar = R.first_argmax_slots(pq[:, :, :C].contiguous(), idx, scale)
    ref = R.edge_train_ref(pq, idx, gamma, beta, slope, kstar, gout)
    free = R.edge_train_ref(pq, idx, gamma, beta, slope, None, gout)
    for r in (ref, free):
        assert float((r.out - y.detach()).abs().max()) <= 1e-12
        assert float((r.dpq - want[0]).abs().max()) <= 1e-12
        assert float((r.dgamma - want[1]).abs().max()) <= 1e-11
        assert float((r.dbeta - want[2]).abs().max()) <= 1e-11
    n = B * N * K
    mu, var = mu.detach(), var.detach()
    assert float((ref.mean - mu.flatten()).abs().max()) <= 1e-14
    assert float((ref.var - var.flatten()).abs().max()) <= 1e-14
    assert float((ref.var_unbiased - e.detach().permute(1, 0, 2, 3).reshape(C, -1).var(dim=1, unbiased=True)).abs().max()) <= 1e-13
    assert abs(float(ref.var_unbiased[0] / ref.var[0]) - n / (n - 1)) <= 1e-12


def test_edge_train_ref_with_a_forced_slot_routes_the_gradient_there():
    """a forced slot that is NOT the max: the output is that candidate and dP lands on that neighbour only"""
    B, N, C, K = 1, 12, 2, 3
    pq, idx, gamma, beta, gout = _edge_inputs(B, N, C, K, 1, 12)
    kstar = torch.full((B, N, C), 2)
    ref = R.edge_train_ref(pq, idx, torch.ones(C), torch.zeros(C), 0.2, kstar, gout)
    e = pq[:, :, :C].double()[0][idx[0, :, 2]] + pq[0, :, C:].double()
    z = (e - ref.mean) / torch.sqrt(ref.var + 1e-5)
    assert float((ref.out[0] - F.leaky_relu(z, 0.2)).abs().max()) <= 1e-12


def test_edge_train_ref_takes_a_given_sign_only_inside_the_band():
    """pos overrides LeakyReLU's branch where |z| <= band and nowhere else; with band = 0 (and z != 0) it changes nothing"""
    B, N, C, K = 2, 12, 4, 3
    pq, idx, gamma, beta, gout = _edge_inputs(B, N, C, K, 1, 13)
    kstar = torch.zeros(B, N, C, dtype=torch.long)
    base = R.edge_train_ref(pq, idx, gamma, beta, 0.2, kstar, gout)
    wrong = ~(base.z > 0)
    same = R.edge_train_ref(pq, idx, gamma, beta, 0.2, kstar, gout, pos=wrong, band=0.0)
    assert torch.equal(same.out, base.out) and torch.equal(same.dpq, base.dpq)
    band = float(base.z.abs().median())
    inside = base.z.abs() <= band
    forced = R.edge_train_ref(pq, idx, gamma, beta, 0.2, kstar, gout, pos=wrong, band=band)
    want = torch.where(inside == (base.z > 0), base.z * 0.2, base.z)          # flipped inside, untouched outside
    assert float((forced.out - want).abs().max()) <= 1e-15
    assert bool(inside.any()) and bool((~inside).any())
    assert float((forced.dbeta - base.dbeta).abs().max()) > 1e-3              # and the gradient follows the branch


@pytest.mark.parametrize("case", [(3, 24, 8, 5, 2, 0.2), (2, 13, 4, 3, 1, 0.1)])
def test_edge_gather_bwd_ref_is_autograd_of_the_plain_max(case):
    B, N, C, K, G, slope = case
    pq, idx, _, _, gout = _edge_inputs(B, N, C, K, G, 21)
    for i in range(N):
        idx[:, i] = (torch.arange(K) * 5 + i) % N
    with torch.enable_grad():
        p = pq.double().requires_grad_(True)
        bi = torch.arange(B)[:, None, None]
        y = F.leaky_relu((p[:, :, :C][bi, idx]).max(dim=2)[0] + p[:, :, C:], slope)
        (want,) = torch.autograd.grad(y, p, gout.double())
    ref = R.edge_gather_bwd_ref(pq, idx, gout, slope)
    assert float((ref.dQ.double() - want[:, :, C:]).abs().max()) <= 1e-7      # float32 gout * slope against the float64 product
    assert float((ref.dP - want[:, :, :C]).abs().max()) <= 1e-6
    assert torch.equal(ref.deg, R.in_degree(idx))
    assert bool((ref.sum_abs >= ref.dP.abs() - 1e-12).all())
    assert float((ref.sum_abs.sum(1) - ref.dQ.double().abs().sum(1)).abs().max()) <= 1e-9     # every |dQ| lands on exactly one node


def test_edge_gather_bwd_ref_on_ties_follows_the_first_slot():
    pq = torch.zeros(1, 12, 2)
    pq[0, :, 0] = torch.tensor([5.0, 5.0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    idx = R.synthetic_graphs(1, 12, 3, 9).long()
    idx[0, 4] = torch.tensor([1, 0, 1])                                       # nodes 0 and 1 tie: slot 0 (node 1) wins
    ref = R.edge_gather_bwd_ref(pq, idx, torch.ones(1, 12, 1), 0.2)
    assert int(ref.kstar[0, 4, 0]) == 0
    assert float(ref.dQ[0, 4, 0]) == 1.0                                      # 5 + 0 > 0


@pytest.mark.parametrize("N,E,k,Hp", [(40, 4, 2, 17), (33, 8, 1, 9)])
def test_index2feat_bwd_ref_is_autograd_of_the_indexed_gather(N, E, k, Hp):
    B, Wp = 3, Hp + 2
    gen = torch.Generator().manual_seed(N)
    x_id = torch.randint(0, (Wp - 1) // 2, (B, N), generator=gen)
    y_id = torch.randint(0, (Hp - 1) // 2, (B, N), generator=gen)
    x_id[0, 3], y_id[2, 5], x_id[1, 1] = Wp, Hp // 2 + 3, -1                  # outside the map: contribute nothing
    mask = (torch.rand(B, N, generator=gen) > 0.4).float() * (1.0 - 0.5 * (torch.rand(B, N, generator=gen) > 0.7).float())
    mask[1] = 0
    mask[0, 3] = mask[2, 5] = 1.0
    gout = det_tensor("i2r_g%d" % N, (B, N, 4 * E))
    with torch.enable_grad():
        patches = det_tensor("i2r_p%d" % N, (B, Hp, Wp, E)).double().requires_grad_(True)
        outs = []
        for t in range(4):                                                    # plain indexing, tap by tap
            y = 2 * y_id + (k if t & 1 else 0)
            x = 2 * x_id + (k if t & 2 else 0)
            ok = (y >= 0) & (y < Hp) & (x >= 0) & (x < Wp)
            v = patches[torch.arange(B)[:, None], y.clamp(0, Hp - 1), x.clamp(0, Wp - 1)]     # (B, N, E)
            outs.append(v * (ok.double() * mask.double())[:, :, None])
        out = torch.cat(outs, dim=-1)
        (want,) = torch.autograd.grad(out, patches, gout.double())
    ref = R.index2feat_bwd_ref(gout, x_id, y_id, mask, Hp, Wp, k)
    assert float((ref.dpatches - want).abs().max()) <= 1e-13
    assert float(ref.dpatches[1].abs().max()) == 0.0 and int(ref.n[1].sum()) == 0
    _, _, ok = R.index2feat_taps(x_id, y_id, mask, Hp, Wp, k)
    assert int(ref.n.sum()) == int(ok.sum()) and int(ref.n.max()) > 1
    assert bool((ref.sum_abs >= ref.dpatches.abs() - 1e-13).all())
    assert bool((ref.sum_abs[ref.n == 0] == 0).all())
    bound = R.fp32_sum_bound(ref.n[..., None], ref.sum_abs)
    assert bound.shape == ref.dpatches.shape and bool((bound[ref.n == 0] == 0).all())
