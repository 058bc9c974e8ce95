"""Free-running parity by DECISION REPLAY (test infrastructure; a plain module, no fixtures, no pytest hooks).

The product's forward is free-running: each stage thresholds its own logits into ids and the next stage gathers image features
at those ids (oracle/checkerpose_oracle.py: posenet_forward).  Comparing such a run with the oracle's own free run is ill-posed
wherever a reference logit sits within the tolerance of the threshold: the two sides may legitimately land on different sides of
the near-tie and everything downstream of it differs by O(1).  It becomes well-posed -- for every keypoint, row and crop, with no
margin condition -- when the oracle is forced to the decisions THE RUN UNDER TEST TOOK:

  1. forced = decisions_from_logits(out)            the run's own logits, decoded with the oracle's decode functions
  2. ref_f  = oracle_forward(forced)                the oracle under those decisions
  3. |out logits - ref_f logits| <= tol             roi, x bits, y bits, seg: everything, unconditionally
  4. out's final ids == the ids of step 1           bit for bit

If 3 holds, a decision on which the run and the oracle's free run differ has |z| <= tol on the oracle's side at the first stage
where the crop's decisions differ (up to there both computed from the same inputs), so nothing else needs a margin.  Where the
run's decisions equal the free reference's, ref_f IS the free reference and the check is the plain 6-tuple comparison.

Scope: PoseNet_GNNskip and its LM twin, `stage=` truncation, any n_graph tuple.  InitNet alone has no feedback and the woProg
ablation decodes one code at the end: for those only assert_ids_match_own_logits applies.
"""
import numpy as np
import torch

from oracle import checkerpose_oracle as O

LOGITS = "free-running logits differ from the oracle replaying the run's own decisions"
OWN_IDS = "final ids disagree with the run's own logits"
BOOKKEEPING = "first differing decision has a free-run margin above the tolerance"
SIGMOID_HALF = 2.0 ** -23      # fp32 sigmoid(z) > 0.5 first holds at z > 1.5 * 2^-24 (tests/golden/sigmoid_threshold.npz): slack of the margin self-check


def _t(x):
    x = x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x))
    x = x.detach().cpu()
    return x.long() if not x.is_floating_point() else x.float()


def _six(out):
    out = out[0] if (isinstance(out, (tuple, list)) and len(out) == 2 and isinstance(out[1], dict)) else out     # (6-tuple, inter)
    return [_t(x) for x in out[:6]]


def _ids_per_stage(zb, init_bits):
    """(B, init_bits + S, N) logits, MSB first -> [ids after InitNet, after stage 0, ...]: pipeline.py:367-381 as the oracle does it"""
    ids = [O.id_from_code_prob(zb[:, :init_bits])]
    for r in range(init_bits, zb.shape[1]):
        ids.append(ids[-1] * 2 + O.id_from_bit_prob(zb[:, r:r + 1]))
    return ids


def decisions_from_logits(out, init_bits=3):
    """the `forced` dict of oracle.posenet_forward for the decisions a 6-tuple's OWN logits encode: {"roi": (B,1,N) 1.0 / 0.0,
    "x": [ids after InitNet, after refinement stage 0, 1, ..], "y": [...]}.  The last entry is the final id (it feeds nothing)."""
    roi, xb, yb = _six(out)[:3]
    return {"roi": O.mask_from_prob(roi), "x": _ids_per_stage(xb, init_bits), "y": _ids_per_stage(yb, init_bits)}


def same_decisions(a, b):
    return (torch.equal(a["roi"], b["roi"]) and len(a["x"]) == len(b["x"])
            and all(torch.equal(p, q) for p, q in zip(a["x"] + a["y"], b["x"] + b["y"])))


def assert_ids_match_own_logits(out, init_bits=3):
    """step 4: the returned (x_id, y_id) are int64 and equal the decode of the returned logits at EVERY keypoint (no band, no margin)"""
    d = decisions_from_logits(out, init_bits)
    for name, got, want in (("x_id", out[4], d["x"][-1]), ("y_id", out[5], d["y"][-1])):
        assert torch.is_tensor(got) and got.dtype == torch.int64, "%s: %s is not int64" % (OWN_IDS, name)
        bad = _t(got) != want
        assert not bool(bad.any()), "%s: %s at %d of %d keypoints, first (crop, keypoint) %s" % (
            OWN_IDS, name, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
    return d


def _first_difference(d_out, d_free, ref_free, init_bits):
    """decisions of the run that differ from the free reference's: their number (B x rows x N single-bit decisions, ids compared
    bit by bit through the per-stage ids), and the largest |z| of the free reference among those of the FIRST stage at which the
    crop differs at all -- up to that stage both sides computed the crop from the same inputs (a later stage's EdgeConv layers mix a
    keypoint with neighbours whose gather positions already differ), so there, and only there, the margin is bounded by the logit
    tolerance.  Stage 0 = InitNet (roi + init_bits x / y bits), stage s > 0 = refinement stage s - 1."""
    roi, xb, yb = ref_free[:3]
    B = roi.shape[0]
    nst = len(d_out["x"])
    diff, marg = [], []                                   # per stage: (B, rows, N) bool / float
    for s in range(nst):
        if s == 0:
            dx = d_out["x"][0] ^ d_free["x"][0]
            dy = d_out["y"][0] ^ d_free["y"][0]
            rows = [d_out["roi"][:, 0] != d_free["roi"][:, 0]]
            rows += [((dx >> (init_bits - 1 - i)) & 1).bool() for i in range(init_bits)]
            rows += [((dy >> (init_bits - 1 - i)) & 1).bool() for i in range(init_bits)]
            z = torch.cat([roi, xb[:, :init_bits], yb[:, :init_bits]], 1)
        else:
            r = init_bits + s - 1
            # the new bit alone: the upper bits are the previous stages' decisions, counted there
            rows = [((d_out["x"][s] ^ d_free["x"][s]) & 1).bool(), ((d_out["y"][s] ^ d_free["y"][s]) & 1).bool()]
            z = torch.cat([xb[:, r:r + 1], yb[:, r:r + 1]], 1)
        diff.append(torch.stack(rows, 1))
        marg.append(z.abs())
    n_diff = int(sum(int(d.sum()) for d in diff))
    worst = 0.0
    for b in range(B):
        for s in range(nst):
            if bool(diff[s][b].any()):
                worst = max(worst, float(marg[s][b][diff[s][b]].max()))
                break
    return n_diff, worst


def replay(out, oracle_forward, ref_free=None, init_bits=3):
    """steps 1-2.  -> (forced, ref_f 6-tuple of CPU tensors, stats).  `ref_free` (the oracle's own free run of the same case) is
    reused as ref_f when the run took exactly its decisions, which saves the second oracle forward."""
    o = _six(out)
    forced = decisions_from_logits(o, init_bits)
    stats = {"decisions_differing_from_free_ref": None, "max_free_margin_at_first_difference": None, "oracle_replayed": True}
    ref_f = None
    if ref_free is not None:
        rf = _six(ref_free)
        d_free = decisions_from_logits(rf, init_bits)
        assert len(d_free["x"]) == len(forced["x"]), "ref_free has %d stages, the run %d" % (len(d_free["x"]) - 1, len(forced["x"]) - 1)
        n, m = _first_difference(forced, d_free, rf, init_bits)
        stats["decisions_differing_from_free_ref"], stats["max_free_margin_at_first_difference"] = n, m
        if same_decisions(forced, d_free):
            ref_f, stats["oracle_replayed"] = rf, False
    if ref_f is None:
        with torch.no_grad():
            ref_f = _six(oracle_forward(forced))
    return forced, ref_f, stats


def assert_free_running_parity(out, oracle_forward, ref_free=None, tol=1e-4, init_bits=3, label=""):
    """Steps 1-4 of the module docstring on the free-running 6-tuple `out`; `oracle_forward(forced)` runs the case's oracle (a
    closure over its state dict / image / kNN table / kwargs, `stage=` included) and returns its 6-tuple (or (6-tuple, inter)).
    Prints and returns {max_abs_dlogit, keypoints_compared (== B x N: nothing is excluded), decisions_differing_from_free_ref,
    max_free_margin_at_first_difference, oracle_replayed}."""
    o = _six(out)
    assert_ids_match_own_logits(out, init_bits)
    forced, ref_f, stats = replay(out, oracle_forward, ref_free, init_bits)
    worst = 0.0
    for a, b, n in zip(o[:4], ref_f[:4], ("roi", "xb", "yb", "seg")):
        assert tuple(a.shape) == tuple(b.shape), "%s: shape of %s %s != %s" % (LOGITS, n, tuple(a.shape), tuple(b.shape))
        worst = max(worst, float((a - b).abs().max()))
    stats = dict(max_abs_dlogit=worst, keypoints_compared=int(o[0].shape[0] * o[0].shape[2]), **stats)
    print("free-running replay %s: %s" % (label, stats))
    assert worst <= tol, "%s: max |logit - ref_f| = %.3e > %.1e (%s)" % (LOGITS, worst, tol, label)
    m = stats["max_free_margin_at_first_difference"]
    # holds by construction once the logits passed (the crop's first differing stage saw the same inputs on both sides): a larger
    # value means this module's stage bookkeeping is wrong, not the run
    assert m is None or m <= tol + SIGMOID_HALF, "%s: %.3e > %.1e (%s)" % (BOOKKEEPING, m, tol, label)
    return stats
