"""CPU: the decision-replay helper (tests/free_running.py) with the ORACLE standing in for the device -- what it must accept (a
run replaying bit-identically under its own decisions; a run that landed on the other side of a near-tie) and what it must reject
(an arithmetic error at a clear decision, ids that contradict the logits, a gather at the wrong pixel)."""
import pytest
import torch

from oracle import checkerpose_oracle as O
from tests import free_running as FR
from tests.common import build_net, det_image, oracle_kwargs

torch.set_grad_enabled(False)

_CASES = {}


def _case(name):
    """-> (oracle_forward(forced), free-running 6-tuple of the oracle).  The backbone runs once per case: its features are injected
    into the replays (they do not depend on the decisions)."""
    if name not in _CASES:
        lm, ig, gr, stage, seed, iseed = {"plain": (False, 2, 3, None, 1, 5), "lm": (True, 2, 3, None, 2, 2),
                                          "woEdgeConv": (False, 0, 0, None, 4, 13), "stage2": (False, 2, 3, 2, 1, 5)}[name]
        net = build_net(seed=seed, lm=lm, init_graph=ig, graph=gr)
        img = det_image(2, seed=iseed)
        knn_idx = net.init_net.knn_idx[torch.tensor([2, 9]) - 1] if lm else net.init_net.knn_idx
        kw = dict(oracle_kwargs(), init_n_graph=ig, n_graph=gr, stage=stage)
        sd = net.state_dict()
        ref, inter = O.posenet_forward(sd, img, knn_idx, 512, **kw)
        feats = inter["img_feats"]

        def oracle_forward(forced, _a=(sd, img, knn_idx, kw, feats)):
            return O.posenet_forward(_a[0], _a[1], _a[2], 512, forced=forced, img_feats=_a[4], **_a[3])
        _CASES[name] = (oracle_forward, ref)
    return _CASES[name]


def _clone(ref):
    return [t.clone() for t in ref]


@pytest.mark.parametrize("name", ["plain", "lm", "woEdgeConv", "stage2"])
def test_own_decisions_replay_bit_identically(name):
    """the oracle forced to its own free-running decisions IS its free run, bit for bit (plain, LM twin with (B, N, K) tables,
    num_graph_module = 0, stage = 2 truncation); the helper then needs no second oracle run when it is given the free reference"""
    fwd, ref = _case(name)
    forced = FR.decisions_from_logits(ref)
    nst = ref[1].shape[1] - 3
    assert len(forced["x"]) == nst + 1 == len(forced["y"]) and forced["roi"].shape == ref[0].shape
    assert torch.equal(forced["x"][-1], ref[4]) and torch.equal(forced["y"][-1], ref[5])
    ref_f, _ = fwd(forced)
    for a, b in zip(ref_f, ref):
        assert torch.equal(a, b)
    calls = []
    st = FR.assert_free_running_parity(ref, lambda f: calls.append(1) or fwd(f), ref_free=ref, label=name)
    assert calls == [] and not st["oracle_replayed"]
    assert st["max_abs_dlogit"] == 0.0 and st["decisions_differing_from_free_ref"] == 0 and st["keypoints_compared"] == 2 * 512
    st = FR.assert_free_running_parity(ref, fwd, label=name + " (no free reference)")
    assert st["oracle_replayed"] and st["max_abs_dlogit"] == 0.0


def _other_side_of_the_nearest_tie(fwd, ref):
    """a stand-in device that takes the OTHER decision at the reference's smallest-margin feedback logit and is otherwise exact: the
    oracle under that decision, the logit itself mirrored to the other side of the threshold (a difference of 2 |z|)"""
    z = torch.cat([ref[0], ref[1][:, :-1], ref[2][:, :-1]], 1)          # the decisions that feed a later stage
    margin, flat = z.abs().flatten().min(0)
    b, r, n = [int(v) for v in torch.unravel_index(flat, z.shape)]
    nfb = ref[1].shape[1] - 1
    slot, row = (0, 0) if r == 0 else ((1, r - 1) if r <= nfb else (2, r - 1 - nfb))

    def mirrored(t):
        t = _clone(t)
        t[slot][b, row, n] = -ref[slot][b, row, n]
        return t
    stand = mirrored(ref)
    for _ in range(ref[1].shape[1]):             # each pass fixes one more stage's decisions
        forced = FR.decisions_from_logits(stand)
        nxt = mirrored(fwd(forced)[0])
        nxt[4], nxt[5] = forced["x"][-1], forced["y"][-1]
        done = FR.same_decisions(FR.decisions_from_logits(nxt), forced)
        stand = nxt
        if done:
            break
    assert done
    stand[4], stand[5] = FR.decisions_from_logits(stand)["x"][-1], FR.decisions_from_logits(stand)["y"][-1]
    return stand, float(margin), (b, slot, row, n)


def test_near_tie_stand_in_passes_replay_and_fails_the_free_comparison():
    """num_graph_module = 0 case of test_gpu_parity (seed 4 / image seed 13): its smallest feedback margin is 3.65e-5, below the 1e-4
    tolerance.  A stand-in on the other side of that near-tie has other final ids than the free reference (so the plain 6-tuple
    comparison rejects it) and is accepted by the replay with max |dlogit| = 2 x the margin"""
    fwd, ref = _case("woEdgeConv")
    stand, margin, where = _other_side_of_the_nearest_tie(fwd, ref)
    assert margin < 5e-5, margin
    assert not (torch.equal(stand[4], ref[4]) and torch.equal(stand[5], ref[5]))          # the plain 6-tuple comparison fails on the ids
    st = FR.assert_free_running_parity(stand, fwd, ref_free=ref, label="near-tie stand-in %s" % (where,))
    assert st["oracle_replayed"] and st["decisions_differing_from_free_ref"] >= 1
    assert abs(st["max_abs_dlogit"] - 2 * margin) <= 1e-6
    assert abs(st["max_free_margin_at_first_difference"] - margin) <= 1e-9


def test_rejects_a_late_logit_moved_at_a_clear_decision():
    """mutant 1 -- LOGITS assertion: the last stage's x logit of one keypoint with |z| > 1e-2 moved by 3e-4 (no decision changes)"""
    fwd, ref = _case("plain")
    m = _clone(ref)
    n = int((ref[1][0, -1].abs() > 1e-2).nonzero()[0])
    m[1][0, -1, n] += 3e-4 * torch.sign(ref[1][0, -1, n])
    assert FR.same_decisions(FR.decisions_from_logits(m), FR.decisions_from_logits(ref))
    with pytest.raises(AssertionError, match=FR.LOGITS):
        FR.assert_free_running_parity(m, fwd, ref_free=ref)
    with pytest.raises(AssertionError, match=FR.LOGITS):
        FR.assert_free_running_parity(m, fwd)


def test_rejects_final_ids_that_disagree_with_the_own_logits():
    """mutant 2 -- OWN_IDS assertion: one keypoint's final x_id (then y_id) off by one bit, logits untouched"""
    fwd, ref = _case("lm")
    for k in (4, 5):
        m = _clone(ref)
        m[k][1, 77] ^= 1
        with pytest.raises(AssertionError, match=FR.OWN_IDS):
            FR.assert_free_running_parity(m, fwd, ref_free=ref)
        with pytest.raises(AssertionError, match=FR.OWN_IDS):
            FR.assert_ids_match_own_logits(m)
    FR.assert_ids_match_own_logits(ref)
    m = _clone(ref)
    m[4] = m[4].int()
    with pytest.raises(AssertionError, match=FR.OWN_IDS):
        FR.assert_ids_match_own_logits(m)


@pytest.mark.parametrize("name", ["plain", "woEdgeConv"])
def test_rejects_a_gather_at_the_wrong_pixel(name):
    """mutant 3 -- LOGITS assertion: a stand-in whose second refinement stage gathered one keypoint one pixel beside the id its own
    first-stage logits encode (built with `forced`), all rows up to that stage untouched, later rows and ids self-consistent"""
    fwd, ref = _case(name)
    forced = FR.decisions_from_logits(ref)
    on = (forced["roi"][0, 0] > 0.5).nonzero().flatten()               # the gathered rows of a keypoint outside the RoI are zeroed
    assert len(on) > 0
    n = int(on[len(on) // 2])
    bad = {"roi": forced["roi"], "x": [t.clone() for t in forced["x"]], "y": forced["y"]}
    bad["x"][1][0, n] += 1 if int(bad["x"][1][0, n]) < 15 else -1      # 4-bit ids after the first stage
    wrong = fwd(bad)[0]
    m = _clone(ref)
    m[1][:, 4:], m[2][:, 4:], m[3] = wrong[1][:, 4:], wrong[2][:, 4:], wrong[3]
    assert torch.equal(m[1][:, :4], ref[1][:, :4]) and torch.equal(m[0], ref[0])
    assert float((m[1][:, 4:] - ref[1][:, 4:]).abs().max()) > 0        # the shifted pixel did reach the logits
    own = FR.decisions_from_logits(m)
    m[4], m[5] = own["x"][-1], own["y"][-1]
    FR.assert_ids_match_own_logits(m)
    with pytest.raises(AssertionError, match=FR.LOGITS):
        FR.assert_free_running_parity(m, fwd, ref_free=ref)
