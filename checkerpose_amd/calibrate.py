"""Calibration of the code logits on the device (csrc/calibrate.hip).

Rows N32 / N33 read the code logits as probabilities: code_confidence turns p (1 - p) per bit into a pixel variance, the weighted
refinement whitens with it, solve_pnp_conf gates inliers at a chi-square quantile.  Whether a trained network's logits deserve that is
a question about the weights; this module is the instrument that answers it on a validation set, and the one-parameter-per-row
correction when the answer is no:
  reliability / reliability_figures / add_reliability   per logit row, the reliability diagram's accumulators (is a bit at
                                                         sigmoid = 0.9 right 90 % of the time?), ECE, MCE, NLL, Brier, sign accuracy;
  fit_code_scale                                         one inverse temperature per group of rows, the minimiser of the rows' NLL
                                                         (convex, bracketed Newton, the whole iteration enqueued on the device);
  sigma2_consistency                                     the histogram of the whitened residuals under the TRUE pose against
                                                         chi-square with 2 degrees of freedom: coverage at the gates, inflation;
  CalibratedNet                                          a net whose logit rows are multiplied by the fitted scales, accepted
                                                         wherever the wrappers take `net`;
  collect_logits                                         forward + encode_targets over batches, concatenated on the device.
All are reached through postprocess.  The rule is the project's own (the reference has no calibration), stated at the top of the kernel
file and restated in numpy by tests/calib_stages.py.  Nothing here changes an existing call.  No CPU fallback: CPU tensors raise."""
import math

import numpy as np
import torch

from . import _abi

CALIB_MAX_BINS, CALIB_MAX_ITERS, CALIB_INFO = 64, 256, 12               # csrc/calibrate.hip
STATUS_OK, STATUS_CAPPED_HIGH, STATUS_CAPPED_LOW, STATUS_EMPTY, STATUS_NOT_CONVERGED = 0, 1, 2, 3, 4      # CP_CALIB_*
STATUS_NAMES = ("OK", "CAPPED_HIGH", "CAPPED_LOW", "EMPTY", "NOT_CONVERGED")
_NO_CPU = "checkerpose_amd.calibrate: CUDA/HIP tensors required (no CPU fallback)"


def logit_edges(bins):
    """The bin edges of reliability() in LOGIT space, float64 on the host.  An int M: the M equal-width probability bins, edge k =
    log(k / (M - k)) for k = 1 .. M - 1; an array: ascending probability edges strictly inside (0, 1), edge = log(p / (1 - p))."""
    if isinstance(bins, (int, np.integer)):
        M = int(bins)
        if not 1 <= M <= CALIB_MAX_BINS:
            raise ValueError("bins must be in 1..%d, got %r" % (CALIB_MAX_BINS, bins))
        return np.array([math.log(k / (M - k)) for k in range(1, M)], dtype=np.float64)
    p = np.asarray(bins, dtype=np.float64).reshape(-1)
    if p.size > CALIB_MAX_BINS - 1 or not (np.all(p > 0.0) and np.all(p < 1.0)) or np.any(np.diff(p) <= 0.0):
        raise ValueError("bins: at most %d probability edges strictly inside (0, 1), strictly ascending" % (CALIB_MAX_BINS - 1))
    e = np.array([math.log(v / (1.0 - v)) for v in p], dtype=np.float64)
    if np.any(np.diff(e) <= 0.0):
        raise ValueError("bins: the probability edges do not stay apart in logit space")
    return e


def chi2_edges(bins):
    """The bin edges of sigma2_consistency() in chi-square units, float64 on the host.  An int M: the M equal-probability bins of
    chi-square with 2 degrees of freedom, edge k = -2 log(1 - k / M) for k = 1 .. M - 1 (closed form: its CDF is 1 - exp(-x / 2));
    an array: ascending edges as they are."""
    if isinstance(bins, (int, np.integer)):
        M = int(bins)
        if not 1 <= M <= CALIB_MAX_BINS:
            raise ValueError("bins must be in 1..%d, got %r" % (CALIB_MAX_BINS, bins))
        return np.array([-2.0 * math.log(1.0 - k / M) for k in range(1, M)], dtype=np.float64)
    e = np.asarray(bins, dtype=np.float64).reshape(-1).copy()
    if e.size > CALIB_MAX_BINS - 1 or np.any(np.isnan(e)) or np.any(np.diff(e) <= 0.0):
        raise ValueError("bins: at most %d edges, no NaN, strictly ascending" % (CALIB_MAX_BINS - 1))
    return e


def _bits_block(outputs_or_bits):
    """the (B, K, N) fp32 logit block (rows N apart and dense, any batch stride) of a network tuple or of a tensor given as it is"""
    if torch.is_tensor(outputs_or_bits):
        bits = outputs_or_bits
    else:
        roi, xb, yb = outputs_or_bits[0], outputs_or_bits[1], outputs_or_bits[2]
        if not (torch.is_tensor(roi) and torch.is_tensor(xb) and torch.is_tensor(yb)):
            raise ValueError("outputs must be the network's tuple (roi (B,1,N), x bits (B,r,N), y bits (B,r,N), ...) or the (B,1+2r,N) block")
        B, _, N = roi.shape
        K = 1 + int(xb.shape[1]) + int(yb.shape[1])
        base = roi._base if roi._base is not None and tuple(roi._base.shape) == (B, K, N) else None
        bits = base if base is not None else torch.cat([roi, xb, yb], 1)
        if xb.shape[1] != yb.shape[1]:
            raise ValueError("outputs: the x and y code rows must be as many")
    if bits.dim() != 3 or bits.shape[1] < 3 or bits.shape[1] % 2 != 1 or bits.shape[1] > 61 or bits.shape[2] < 1:
        raise ValueError("the logit block must be (B, 1 + 2r, N) with 1 <= r <= 30 and N >= 1, got %r" % (tuple(bits.shape),))
    bits = bits.detach()
    if bits.dtype != torch.float32:
        raise ValueError("the logit block must be float32, got %s" % bits.dtype)
    K, N = int(bits.shape[1]), int(bits.shape[2])
    if bits.stride(2) != 1 or bits.stride(1) != N or (bits.shape[0] > 1 and bits.stride(0) < K * N):
        bits = bits.contiguous()
    return bits


def _labels(labels, B, r, N, dev):
    try:
        g_roi, g_x, g_y = labels["roi_mask_bits"], labels["pixel_x_codes"], labels["pixel_y_codes"]
    except (KeyError, TypeError, IndexError):
        raise ValueError("labels must be encode_targets' dict: roi_mask_bits, pixel_x_codes, pixel_y_codes")
    if not all(torch.is_tensor(x) for x in (g_roi, g_x, g_y)):
        raise ValueError("labels must hold tensors")
    gb = int(g_x.shape[1]) if g_x.dim() == 3 else -1
    if tuple(g_roi.shape) != (B, 1, N) or tuple(g_x.shape) != (B, gb, N) or tuple(g_y.shape) != (B, gb, N) or gb < r:
        raise ValueError("labels must be roi_mask_bits (B,1,N) and pixel_x_codes / pixel_y_codes (B,bits,N) with bits >= the %d predicted" % r)
    return g_roi.float().contiguous(), g_x.float().contiguous(), g_y.float().contiguous(), gb


def _need_cuda(*tensors):
    """the last of a wrapper's argument checks: well-formed arguments on the host still have no fallback"""
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(_NO_CPU)


def _bstride(bits):
    return bits.stride(0) if bits.shape[0] > 1 else int(bits.shape[1]) * int(bits.shape[2])


def reliability(outputs_or_bits, labels, scale=None, bins=15):
    """The reliability accumulators of every logit row (cp_code_reliability; csrc/calibrate.hip states the rule).
      outputs_or_bits: the network's tuple (its logit block is found as correspondences finds it) or the (B, 1 + 2r, N) fp32 block
      itself (a batch stride is fine); labels: encode_targets' dict; scale: None (ones) or (1 + 2r,) inverse temperatures, finite and
      > 0, e.g. fit_code_scale's; bins: an int M (equal-width probability bins) or ascending probability edges (logit_edges).
    Row 0 counts every keypoint, the x / y rows only where the GT RoI bit is set.  t = float64(z) * scale; bin = the number of edges <= t.
    -> dict of device tensors: count, positives (K,M) int64; sum_p (K,M) f64; n, n_nan, n_right (K,) int64 (n_right: the sign is right, (z > 0) == y); nll, brier, g, h (K,) f64 (sums, not
       means; g and h are the NLL's first and second derivative in the scale); plus edges (M-1,) and scale (K,) f64 as they were used.
       Integer outputs do not depend on the launch shape; two calls agree bitwise."""
    bits = _bits_block(outputs_or_bits)
    B, K, N = (int(v) for v in bits.shape)
    r = (K - 1) // 2
    dev = bits.device
    g_roi, g_x, g_y, gb = _labels(labels, B, r, N, dev)
    edges = logit_edges(bins)
    M = int(edges.size) + 1
    sc = np.ones(K, dtype=np.float64) if scale is None else np.ascontiguousarray(
        scale.detach().cpu().numpy() if torch.is_tensor(scale) else np.asarray(scale), dtype=np.float64).reshape(-1)
    if sc.shape != (K,) or not (np.all(np.isfinite(sc)) and np.all(sc > 0.0)):
        raise ValueError("scale must hold %d finite inverse temperatures > 0" % K)
    _need_cuda(bits, g_roi, g_x, g_y)
    lib = _abi.load()
    ints = torch.zeros(K, 2 * M + 3, dtype=torch.int64, device=dev)
    sums = torch.zeros(K, M + 4, dtype=torch.float64, device=dev)
    scratch = torch.empty(max(8, lib.cp_code_reliability_scratch_bytes(r, M)) if B else 8, dtype=torch.uint8, device=dev)
    if B:
        _abi.call("cp_code_reliability", dev, bits, _bstride(bits), K, r, g_roi, g_x, g_y, gb, sc.ctypes.data, edges.ctypes.data if M > 1 else None,
                  M, B, N, ints, sums, scratch)
    return dict(count=ints[:, :M], positives=ints[:, M:2 * M], n=ints[:, 2 * M], n_nan=ints[:, 2 * M + 1], n_right=ints[:, 2 * M + 2], sum_p=sums[:, :M],
                nll=sums[:, M], brier=sums[:, M + 1], g=sums[:, M + 2], h=sums[:, M + 3],
                edges=torch.from_numpy(edges).to(dev), scale=torch.from_numpy(sc).to(dev))


_ACC_SUMS = ("count", "positives", "n", "n_nan", "n_right", "sum_p", "nll", "brier", "g", "h")


def add_reliability(a, b):
    """Merge two reliability() results of the same edges and scale (two batches of one validation set).  Counts add exactly; the
    floating sums add once more (a + b)."""
    if not (torch.equal(a["edges"], b["edges"]) and torch.equal(a["scale"], b["scale"])):
        raise ValueError("add_reliability: the two accumulators were made with different edges or scales")
    out = {k: a[k] + b[k] for k in _ACC_SUMS}
    out["edges"], out["scale"] = a["edges"], a["scale"]
    return out


def reliability_figures(acc):
    """The figures of a reliability() result, formed on the host in float64 -> dict of numpy arrays per row: ece = sum_b n_b / n
    |pos_b / n_b - sum_p_b / n_b| over the non-empty bins, mce = the largest of those gaps, nll and brier as means, accuracy = the share of
    counted samples whose sign is right (n_right / n: (z > 0) == y, code_report's decision), n, n_nan; per bin confidence = sum_p_b / n_b and frequency =
    pos_b / n_b (NaN where empty).  A row without counted samples gives NaN."""
    c = {k: acc[k].detach().cpu().numpy() for k in _ACC_SUMS}
    cnt, pos, sp = c["count"].astype(np.float64), c["positives"].astype(np.float64), c["sum_p"]
    n = c["n"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        conf, freq = sp / cnt, pos / cnt
        gap = np.where(cnt > 0, np.abs(freq - conf), 0.0)
        ece = (cnt * gap).sum(1) / n
        mce = np.where(n > 0, gap.max(1), np.nan)
        acc_sign = c["n_right"].astype(np.float64) / n
        return dict(ece=ece, mce=mce, nll=c["nll"] / n, brier=c["brier"] / n, accuracy=acc_sign, n=c["n"], n_nan=c["n_nan"],
                    confidence=conf, frequency=freq)


def _groups(groups, r):
    K = 1 + 2 * r
    if isinstance(groups, str):
        if groups == "row":
            g = np.arange(K)
        elif groups == "significance":
            g = np.concatenate([[0], 1 + np.arange(r), 1 + np.arange(r)])
        elif groups == "all":
            g = np.zeros(K)
        else:
            raise ValueError("groups must be 'row', 'significance', 'all' or an array of %d group indices, got %r" % (K, groups))
    else:
        g = np.asarray(groups.detach().cpu().numpy() if torch.is_tensor(groups) else groups).reshape(-1)
        if g.shape != (K,) or np.any(g != np.floor(g)) or g.min() < 0 or g.max() >= K:
            raise ValueError("groups: %d integers in [0, %d), one per logit row" % (K, K))
    g = np.ascontiguousarray(g, dtype=np.int32)
    return g, int(g.max()) + 1


def fit_code_scale(outputs_or_bits, labels, groups="row", s_min=2.0 ** -6, s_max=2.0 ** 6, step_tol=1e-8, max_iters=60):
    """One inverse temperature per group of logit rows, fitted on the device (cp_fit_code_scale; csrc/calibrate.hip states the
    iteration, tests/calib_stages.py restates it).
      outputs_or_bits, labels: as reliability() -- pass the validation set's logits and labels concatenated on the device
      (collect_logits); groups: "row" (1 + 2r groups, the default), "significance" (x bit j and y bit j share one: 1 + r groups), "all"
      (one group) or (1 + 2r,) group indices; [s_min, s_max]: the bracket, s_min <= 1 <= s_max (interface parameters, not tolerances);
      step_tol: stop when |s' - s| <= step_tol * s; max_iters in 1..256 evaluations.
    Each group minimises its rows' summed NLL of sigmoid(s z) against the labels: convex in s, bracketed Newton from s = 1.  The whole
    iteration is enqueued at once: no host round trip.
    -> (scale (1 + 2r,) f64 device tensor: the row's group's s, info): info = dict(status (G,) int32 -- STATUS_OK / STATUS_CAPPED_HIGH
       (separable data: every sign right, s = s_max) / STATUS_CAPPED_LOW / STATUS_EMPTY (no counted sample, s = 1) /
       STATUS_NOT_CONVERGED -- iters (G,) int32, nll_before, nll_after (G,) f64 sums at s = 1 and at the returned s, n (G,) int64,
       s, lo, hi (G,) f64, group_of_row (1 + 2r,) int32)."""
    bits = _bits_block(outputs_or_bits)
    B, K, N = (int(v) for v in bits.shape)
    r = (K - 1) // 2
    dev = bits.device
    g_roi, g_x, g_y, gb = _labels(labels, B, r, N, dev)
    grp, G = _groups(groups, r)
    s_min, s_max, step_tol, max_iters = float(s_min), float(s_max), float(step_tol), int(max_iters)
    if not (0.0 < s_min <= 1.0 <= s_max < float("inf") and s_min < s_max):
        raise ValueError("the bracket must satisfy 0 < s_min <= 1 <= s_max < inf and s_min < s_max, got [%r, %r]" % (s_min, s_max))
    if not 0.0 < step_tol < float("inf"):
        raise ValueError("step_tol must be a finite number > 0, got %r" % (step_tol,))
    if not 1 <= max_iters <= CALIB_MAX_ITERS:
        raise ValueError("max_iters must be in 1..%d, got %r" % (CALIB_MAX_ITERS, max_iters))
    _need_cuda(bits, g_roi, g_x, g_y)
    lib = _abi.load()
    scale = torch.ones(K, dtype=torch.float64, device=dev)
    info = torch.zeros(G, CALIB_INFO, dtype=torch.float64, device=dev)
    if B == 0:
        info[:, 0], info[:, 1], info[:, 2], info[:, 3] = 1.0, s_min, s_max, float(STATUS_EMPTY)
    scratch = torch.empty(max(8, lib.cp_fit_code_scale_scratch_bytes(r)) if B else 8, dtype=torch.uint8, device=dev)
    if B:
        _abi.call("cp_fit_code_scale", dev, bits, _bstride(bits), K, r, g_roi, g_x, g_y, gb, grp.ctypes.data, G, B, N, s_min, s_max, step_tol,
                  max_iters, scale, info, scratch)
    return scale, dict(status=info[:, 3].to(torch.int32), iters=info[:, 4].to(torch.int32), nll_before=info[:, 5], nll_after=info[:, 6],
                       n=info[:, 7].to(torch.int64), s=info[:, 0], lo=info[:, 1], hi=info[:, 2],
                       group_of_row=torch.from_numpy(grp).to(dev))


def sigma2_consistency(p2d, valid, sigma2, targets, column=0, bins=10, gates=(5.99, 9.21)):
    """Is sigma2 a variance?  The histogram of the whitened residuals the solver would see under the TRUE pose (cp_sigma2_consistency).
      p2d (B,N,2) f32 and valid (B,N,3) uint8 from correspondences(); sigma2 (B,N,2) f64 from code_confidence(); targets:
      encode_targets(..., return_proj=True)'s dict (proj_xy, roi_mask_bits) for the same crops; column as solve_pnp_conf takes it;
      bins: an int M (equal-probability bins of chi-square with 2 degrees of freedom: a flat histogram means a true variance) or
      ascending edges (chi2_edges); gates: chi-square thresholds whose coverage is wanted (a second launch over the same inputs).
    A keypoint counts iff valid, its GT RoI bit is set and both variances are finite and > 0 (row N33's rule); d2 = du^2 / sigma2_x +
    dv^2 / sigma2_y with du = p2d_x - proj_x.
    -> dict: per crop counts (B,M) int32, n, n_dropped (B,) int32, sum_d2, sum_u, sum_v (B,) f64 (sum_u / sum_v: the SIGNED whitened
       residuals, a systematic offset between the cell grid and the projection shows there; reported, not corrected), gate_counts
       (B,len(gates)) int64: the counted keypoints with d2 < gate; totals (host floats / ints): n_total, n_dropped_total, counts_total
       (M,) int64, coverage (len(gates),) = the share with d2 < gate, to be read against 0.95 / 0.99 for the defaults, inflation =
       sum d2 / (2 n): the factor sigma2 would have to be multiplied by for the mean to fit, mean_u, mean_v; edges, gates as used."""
    if not (torch.is_tensor(p2d) and torch.is_tensor(valid) and torch.is_tensor(sigma2)):
        raise ValueError("p2d, valid and sigma2 must be tensors")
    if p2d.dim() != 3 or p2d.shape[2] != 2:
        raise ValueError("p2d must be (B,N,2), got %r" % (tuple(p2d.shape),))
    B, N, _ = (int(v) for v in p2d.shape)
    if tuple(valid.shape) != (B, N, 3) or valid.dtype != torch.uint8 or not 0 <= int(column) < 3:
        raise ValueError("valid must be the (B,N,3) uint8 tensor of correspondences(), column in 0..2")
    if tuple(sigma2.shape) != (B, N, 2) or sigma2.dtype != torch.float64:
        raise ValueError("sigma2 must be the (B,N,2) float64 tensor of code_confidence()")
    try:
        proj, g_roi = targets["proj_xy"], targets["roi_mask_bits"]
    except (KeyError, TypeError, IndexError):
        raise ValueError("targets must be encode_targets(..., return_proj=True)'s dict (proj_xy, roi_mask_bits)")
    if not (torch.is_tensor(proj) and tuple(proj.shape) == (B, N, 2) and proj.dtype == torch.float64 and torch.is_tensor(g_roi)
            and tuple(g_roi.shape) == (B, 1, N)):
        raise ValueError("targets: proj_xy must be (B,N,2) float64 and roi_mask_bits (B,1,N)")
    if N < 1:
        raise ValueError("N must be >= 1")
    edges = chi2_edges(bins)
    gate = np.ascontiguousarray(np.asarray(gates, dtype=np.float64).reshape(-1))
    if gate.size > CALIB_MAX_BINS - 1 or np.any(np.isnan(gate)) or np.any(np.diff(gate) <= 0.0):
        raise ValueError("gates: at most %d thresholds, no NaN, strictly ascending" % (CALIB_MAX_BINS - 1))
    _need_cuda(p2d, valid, sigma2, proj, g_roi)
    dev = p2d.device
    p2, va, s2, pr, gr = p2d.detach().float().contiguous(), valid.contiguous(), sigma2.contiguous(), proj.contiguous(), g_roi.float().contiguous()

    def run(e):
        E = int(e.size)
        counts = torch.zeros(B, E + 1, dtype=torch.int32, device=dev)
        nn = torch.zeros(B, 2, dtype=torch.int32, device=dev)
        sums = torch.zeros(B, 3, dtype=torch.float64, device=dev)
        if B:
            _abi.call("cp_sigma2_consistency", dev, p2, pr, s2, va.data_ptr() + int(column), 3, gr, e.ctypes.data if E else None, E, B, N, counts,
                      nn, sums)
        return counts, nn, sums

    counts, nn, sums = run(edges)
    out = dict(counts=counts, n=nn[:, 0], n_dropped=nn[:, 1], sum_d2=sums[:, 0], sum_u=sums[:, 1], sum_v=sums[:, 2],
               edges=edges, gates=gate)
    if gate.size:
        gc = run(gate)[0].to(torch.int64).cumsum(1)[:, :-1]             # counted points below each gate (d2 == gate is above)
    else:
        gc = torch.zeros(B, 0, dtype=torch.int64, device=dev)
    out["gate_counts"] = gc
    n_tot = int(nn[:, 0].to(torch.int64).sum().item()) if B else 0
    sd2 = sums.cpu().numpy().astype(np.float64)
    tot = [math.fsum(sd2[:, j]) for j in range(3)]
    out["n_total"], out["n_dropped_total"] = n_tot, (int(nn[:, 1].to(torch.int64).sum().item()) if B else 0)
    out["counts_total"] = counts.to(torch.int64).sum(0).cpu().numpy()
    gct = gc.sum(0).cpu().numpy().astype(np.float64)
    nan = float("nan")
    out["coverage"] = gct / n_tot if n_tot else np.full(gate.shape, nan)
    out["inflation"] = tot[0] / (2.0 * n_tot) if n_tot else nan
    out["mean_u"], out["mean_v"] = (tot[1] / n_tot, tot[2] / n_tot) if n_tot else (nan, nan)
    return out


class CalibratedNet(torch.nn.Module):
    """`net` with its 1 + 2r logit rows multiplied by float32(scale) (fit_code_scale's result): the wrapped net's forward signature, the
    same 6-tuple.  The three logit tensors are slices of ONE (B, 1 + 2r, N) block, so correspondences' and code_confidence's fast path
    holds; seg and the two id tensors pass through as they are.  Scales are > 0: no sign moves, so no decoded id moves.  Accepted
    wherever the wrappers take `net` (estimate_poses_conf, estimate_poses_weighted, evaluate_batch, ...)."""

    def __init__(self, net, scale):
        super().__init__()
        sc = scale.detach().to(torch.float64).cpu() if torch.is_tensor(scale) else torch.as_tensor(np.asarray(scale, dtype=np.float64))
        sc = sc.reshape(-1)
        if sc.numel() < 3 or sc.numel() % 2 != 1 or not bool((torch.isfinite(sc) & (sc > 0)).all()):
            raise ValueError("scale must hold 1 + 2r finite inverse temperatures > 0")
        sc32 = sc.to(torch.float32)
        if not bool((torch.isfinite(sc32) & (sc32 > 0)).all()):
            raise ValueError("scale must stay finite and > 0 in float32")
        self.net = net
        self.register_buffer("scale", sc32.reshape(1, -1, 1), persistent=False)

    def forward(self, *args, **kwargs):
        out = self.net(*args, **kwargs)
        roi, xb, yb = out[0], out[1], out[2]
        B, _, N = roi.shape
        nx, ny = int(xb.shape[1]), int(yb.shape[1])
        K = 1 + nx + ny
        if K != self.scale.shape[1]:
            raise ValueError("CalibratedNet: %d scales for a net with %d logit rows" % (self.scale.shape[1], K))
        base = roi._base if roi._base is not None and tuple(roi._base.shape) == (B, K, N) else None
        block = base if base is not None else torch.cat([roi, xb, yb], 1)
        scaled = block * self.scale.to(device=block.device, dtype=block.dtype)
        return (scaled[:, :1], scaled[:, 1:1 + nx], scaled[:, 1 + nx:]) + tuple(out[3:])


def collect_logits(net, batches):
    """Run the forward and encode_targets over an iterable of make_training_batch-style batches and concatenate on the device: what
    reliability() and fit_code_scale() take for a validation set.
      batches: tuples as targets.make_training_batch returns them (roi_x first; the labels roi_mask_bits, pixel_x_codes, pixel_y_codes
      are the three entries before the last); the 12-entry LM form (obj_ids after cam_K) passes obj_ids to the net.
    -> (bits (B_total, 1 + 2r, N) f32, labels dict)"""
    blocks, lab = [], ([], [], [])
    with torch.no_grad():
        for batch in batches:
            obj_ids = batch[7] if len(batch) == 12 else None
            out = net(batch[0], None) if obj_ids is None else net(batch[0], None, obj_ids)
            blocks.append(_bits_block(out))
            for dst, src in zip(lab, batch[-4:-1]):
                dst.append(src.float())
    if not blocks:
        raise ValueError("collect_logits: no batches")
    return torch.cat(blocks, 0), dict(roi_mask_bits=torch.cat(lab[0], 0), pixel_x_codes=torch.cat(lab[1], 0), pixel_y_codes=torch.cat(lab[2], 0))
