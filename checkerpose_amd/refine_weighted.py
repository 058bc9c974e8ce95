"""Poses refined with the code logits' own confidences on the device (csrc/code_confidence.hip,
csrc/pnp_refine_w.hip).

The network's main output is a binary code per keypoint; the post-forward path keeps the logits' signs alone.  A keypoint whose most
significant x bit sits at logit 0.01 (32 cells off if the bit is wrong) then votes like one whose twelve bits are all at +-10, and
every correspondence the solver's 2-px threshold cut off is lost to row N22's refinement.  code_confidence reads the logits as
independent Bernoulli bits and gives each keypoint a pixel variance per axis; refine_poses_lm_weighted is row N22's
Levenberg-Marquardt with those as per-point, per-axis scales and a Huber loss, so that it may run over every valid correspondence;
estimate_poses_weighted is postprocess.estimate_poses with that refinement as its last stage, from ONE forward.  All three are reached
through postprocess.  The rules are the project's own (the reference never refines), stated at the top of the kernel files and
restated in numpy by tests/wlm_stages.py.  UNPINNED: whether a trained network's logits are calibrated enough for the variance to be
one in fact -- no trained weights exist here.  No CPU fallback: CPU tensors raise."""
import numpy as np
import torch

from . import _abi

WLM_MAX_ITERS, WLM_NMAX, WLM_RECORD, WLM_INFO = 64, 4096, 17, 42        # csrc/pnp_refine_w.hip
CODE_FLOOR = 1.0 / 12.0                                                 # cells^2: the variance of uniform quantisation to one cell


def code_confidence(outputs, Bboxes, floor=CODE_FLOOR):
    """Per-keypoint, per-axis pixel variance of the decoded code (row N32; csrc/code_confidence.hip states the rule).
      outputs: the 6-tuple of PoseNet_GNNskip.forward, handled as in postprocess.correspondences (the full 13-row logit block);
      Bboxes: the (B,4) final boxes (x, y, w, h) of the crops (host array or int32 CUDA tensor), as correspondences takes them;
      floor > 0, finite, in cells^2: default 1/12, the variance of uniform quantisation to one cell (derived, not tuned).
    Per bit with logit z: q = p (1 - p), p = sigmoid(z); per axis v = sum_j 4^(r-1-j) q_j, the variance in cells^2 of the code under
    independent Bernoulli bits; sigma2 = (box side / grid side)^2 (floor + v).
    -> sigma2 (B,N,2) f64 on the device, pixels^2, x then y.  0 on an axis whose box side is 0; NaN where a logit is NaN."""
    roi, xb, yb, seg, xid, yid = outputs
    if not roi.is_cuda:
        raise RuntimeError("checkerpose_amd.refine_weighted: CUDA/HIP tensors required (no CPU fallback)")
    floor = float(floor)
    if not 0.0 < floor < float("inf"):
        raise ValueError("floor must be a finite number > 0 (in cells^2), got %r" % (floor,))
    B, _, N = roi.shape
    H, W = int(seg.shape[2]), int(seg.shape[3])
    base = roi._base if roi._base is not None and tuple(roi._base.shape) == (B, 13, N) else None
    bits = base if base is not None else torch.cat([roi, xb, yb], 1).contiguous()
    if bits.shape[1] != 13 or bits.dtype != torch.float32:
        raise ValueError("need the full 13-row fp32 logit block (all refinement stages active)")
    bb = Bboxes if torch.is_tensor(Bboxes) else torch.as_tensor(np.asarray(Bboxes), dtype=torch.int32)
    bb = bb.to(device=roi.device, dtype=torch.int32).contiguous()
    if tuple(bb.shape) != (B, 4):
        raise ValueError("Bboxes must be (B,4): x, y, w, h of every crop")
    sigma2 = torch.empty(B, N, 2, dtype=torch.float64, device=roi.device)
    if B == 0:
        return sigma2
    _abi.call("cp_code_confidence", roi.device, bits.contiguous(), 13, 6, bb, B, N, H, W, floor, sigma2)
    return sigma2


def refine_poses_lm_weighted(p3d_xyz, p2d, mask, scale, cam_K, R, t, huber_delta, status=None, max_iters=20, step_tol=1e-10,
                             return_records=False):
    """postprocess.refine_poses_lm (row N22) with per-point, per-axis scales and a Huber loss (row N32; csrc/pnp_refine_w.hip states
    the rule, tests/wlm_stages.py restates it).
      p3d_xyz, p2d, mask, cam_K, R, t, status, max_iters, step_tol, return_records: as refine_poses_lm;
      scale (B,N,2) fp32 CUDA tensor: 1 / sigma per keypoint and axis, e.g. code_confidence(...).rsqrt().float(); residuals and
      Jacobian rows are multiplied by it (ones give refine_poses_lm's problem);
      huber_delta > 0 (+inf allowed: no robust kernel), NO default, in whitened units (sigmas) per scalar component: beyond it a
      component's cost grows linearly.  Nothing in the project or the reference fixes one: with scales that are true 1 / sigma, 1.345
      is the textbook 95 %-efficiency choice and 2 - 3 is common; it is the caller's choice.
    -> (R (B,3,3) f64, t (B,3,1) f64, refine_status (B,) int32, info[, records]) as refine_poses_lm.  refine_status 0 (pass-through,
       the input pose bitwise) also where a selected point's scale is not finite or <= 0.  info: refine_poses_lm's dict, its costs the
       robust whitened ones and H the whitened, Huber-weighted J^T J at the returned pose -- pose_covariance(info, sigma=1.0) is the
       covariance -- plus n_clipped0, n_clipped (B,) int64: the components beyond huber_delta at the input / returned pose (0 on
       pass-through rows)."""
    max_iters = int(max_iters)
    if not 1 <= max_iters <= WLM_MAX_ITERS:
        raise ValueError("max_iters must be in 1..%d for cp_pnp_refine_wlm, got %r" % (WLM_MAX_ITERS, max_iters))
    step_tol = float(step_tol)
    if not 0.0 < step_tol < float("inf"):
        raise ValueError("step_tol must be a finite number > 0, got %r" % (step_tol,))
    huber_delta = float(huber_delta)
    if not huber_delta > 0.0:
        raise ValueError("huber_delta must be a number > 0 (+inf allowed), got %r" % (huber_delta,))
    if p2d.dim() != 3 or p2d.shape[2] != 2:
        raise ValueError("p2d must be (B,N,2), got %r" % (tuple(p2d.shape),))
    B, N, _ = p2d.shape
    if not 1 <= N <= WLM_NMAX:
        raise ValueError("p2d: N must be in 1..%d, got %d" % (WLM_NMAX, N))
    if not torch.is_tensor(mask) or tuple(mask.shape) != (B, N) or mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError("mask must be a (B,N) bool or uint8 tensor")
    if not torch.is_tensor(scale) or tuple(scale.shape) != (B, N, 2) or scale.dtype != torch.float32:
        raise ValueError("scale must be a (B,N,2) float32 tensor (1 / sigma per keypoint and axis)")
    if not torch.is_tensor(R) or not torch.is_tensor(t) or tuple(R.shape) != (B, 3, 3) or tuple(t.shape) not in ((B, 3, 1), (B, 3)):
        raise ValueError("R must be (B,3,3) and t (B,3,1) / (B,3) tensors")
    if status is not None and (not torch.is_tensor(status) or tuple(status.shape) != (B,)):
        raise ValueError("status must be a (B,) tensor or None")
    if not (p2d.is_cuda and mask.is_cuda and scale.is_cuda and R.is_cuda and t.is_cuda and (status is None or status.is_cuda)):
        raise RuntimeError("checkerpose_amd.refine_weighted: CUDA/HIP tensors required (no CPU fallback)")
    dev = p2d.device
    p3 = torch.as_tensor(p3d_xyz, dtype=torch.float32, device=dev).contiguous()
    K = torch.as_tensor(cam_K, dtype=torch.float32, device=dev).contiguous()
    if p3.shape[-2:] != (N, 3) or K.shape[-2:] != (3, 3) or (p3.dim() == 3 and p3.shape[0] != B) or (K.dim() == 3 and K.shape[0] != B):
        raise ValueError("p3d_xyz must be (N,3) / (B,N,3) and cam_K (3,3) / (B,3,3)")
    p2 = p2d.contiguous().float()
    mk = mask.contiguous().view(torch.uint8)
    sc = scale.to(dev).contiguous()
    pose_in = torch.cat([R.reshape(B, 9).to(dev, torch.float64), t.reshape(B, 3).to(dev, torch.float64)], 1).contiguous()
    st_in = None if status is None else status.to(device=dev, dtype=torch.int32).contiguous()
    pose = torch.empty(B, 12, dtype=torch.float64, device=dev)
    rstatus = torch.empty(B, dtype=torch.int32, device=dev)
    info = torch.empty(B, WLM_INFO, dtype=torch.float64, device=dev)
    rec = torch.full((B, max_iters, WLM_RECORD), float("nan"), dtype=torch.float64, device=dev) if return_records else None
    if B:
        _abi.call("cp_pnp_refine_wlm", dev, p3, 3 * N if p3.dim() == 3 else 0, p2, mk, 1, sc, K, 9 if K.dim() == 3 else 0, B, N, pose_in, st_in,
                  huber_delta, max_iters, step_tol, pose, rstatus, info, rec)
    out_info = dict(cost0=info[:, 0], cost=info[:, 1], n=info[:, 2].long(), iters=info[:, 3].long(), H=info[:, 4:40].view(B, 6, 6), status=rstatus,
                    n_clipped0=info[:, 40].nan_to_num(0.0).long(), n_clipped=info[:, 41].nan_to_num(0.0).long())
    out = (pose[:, :9].view(B, 3, 3), pose[:, 9:].view(B, 3, 1), rstatus, out_info)
    if return_records:
        out += (rec,)
    return out


def _check_weighted(weighted):
    """estimate_poses_weighted's `weighted` argument: a dict with huber_delta and fit (optionally floor, max_iters, step_tol)"""
    if not isinstance(weighted, dict) or "huber_delta" not in weighted or "fit" not in weighted:
        raise ValueError('weighted must be dict(huber_delta=..., fit="inliers" | "valid"[, floor=..., max_iters=..., step_tol=...])')
    extra = [k for k in weighted if k not in ("huber_delta", "fit", "floor", "max_iters", "step_tol")]
    if extra:
        raise ValueError("weighted: unknown key(s) %r (the scales are the logits' own, the status the solver's)" % (extra,))
    if weighted["fit"] not in ("inliers", "valid"):
        raise ValueError('weighted: fit must be "inliers" or "valid", got %r' % (weighted["fit"],))


def estimate_poses_weighted(net, frames, Bboxes, p3d_xyz, cam_K, weighted, return_info=False, **estimate_kwargs):
    """postprocess.estimate_poses with the weighted robust refinement as its last stage (row N32; RGB-only): the same call
    (estimate_kwargs are estimate_poses' keywords, `refine` refused: this call IS a refinement) with ONE forward and one
    correspondences; code_confidence reads the same logits and final boxes, scale = sigma2.rsqrt().float(); the solver runs as in
    estimate_poses; refine_poses_lm_weighted then fits from the solver's pose.
      weighted: a dict with `huber_delta` (refine_poses_lm_weighted's, no default) and `fit`: "inliers" = over the solver's inlier
      set, "valid" = over every valid correspondence (the column the solver saw: check_seg), which is what the Huber loss is for;
      optionally `floor` (code_confidence's), `max_iters`, `step_tol`.
    -> (R, t, inliers, status, final boxes) as estimate_poses with the refined R, t; a crop whose refinement passed through (solver
       status 0, fewer than 6 points to fit, an empty box, ...) keeps the solver's pose bitwise.  return_info=True appends
       refine_poses_lm_weighted's info dict, with refine_status under "status", plus sigma2 and the solver's R, t ("R0", "t0")."""
    from . import postprocess
    _check_weighted(weighted)
    if "refine" in estimate_kwargs:
        raise ValueError("estimate_poses_weighted runs its own refinement: refine=%r is refused" % (estimate_kwargs["refine"],))
    keep = {}
    stages, inl, status, final = postprocess._estimate_stages(net, frames, Bboxes, p3d_xyz, cam_K, keep=keep, **estimate_kwargs)
    _, R0, t0 = stages[-1]
    sigma2 = postprocess.code_confidence(keep["outputs"], final, **({"floor": weighted["floor"]} if "floor" in weighted else {}))
    scale = sigma2.rsqrt().float()
    if weighted["fit"] == "inliers":
        mask = inl
    else:
        mask = keep["valid"][:, :, 1 if estimate_kwargs.get("check_seg", False) else 0].contiguous()
    kw = {k: weighted[k] for k in ("max_iters", "step_tol") if k in weighted}
    R, t, rstatus, info = postprocess.refine_poses_lm_weighted(p3d_xyz, keep["p2d"], mask, scale, cam_K, R0, t0, weighted["huber_delta"],
                                                               status=status, **kw)
    if not return_info:
        return R, t, inl, status, final
    return R, t, inl, status, final, dict(info, sigma2=sigma2, R0=R0, t0=t0)
