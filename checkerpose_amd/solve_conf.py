"""Poses solved with the code logits' own confidences on the device (csrc/pnp_conf.hip).

Row N32 reads a pixel variance per keypoint and axis from the code logits (code_confidence) and uses it after the pose has been found.
The stage that decides the pose, solve_pnp_ransac (row N4), ignores it: its 5-point samples are uniform over the valid keypoints and
every keypoint is gated at the same 2 px.  rank_correspondences orders the valid keypoints by variance; solve_pnp_conf is row N4's
solver with the samples drawn PROSAC-style (Chum & Matas 2005) from a pool that grows down that ranking and the inliers gated on the
whitened residual; estimate_poses_conf is postprocess.estimate_poses with that solver, from ONE forward.  All three are reached through
postprocess.  The rule is the project's own (the reference neither ranks nor whitens), stated at the top of the kernel file and
restated in numpy by tests/cpnp_stages.py.  UNPINNED, as in row N32: whether a trained network's logits rank its errors -- no trained
weights exist here; the rule is the published one for the inputs it is given.  No CPU fallback: CPU tensors raise."""
import torch

from . import _abi

CONF_MAX_ITERS, CONF_NMAX, CONF_HYP = 256, 4096, 14                    # csrc/pnp_conf.hip (pnp_core.h's PNP_*)


def _check_sigma2_valid(who, sigma2, valid, column):
    if not torch.is_tensor(sigma2) or sigma2.dim() != 3 or sigma2.shape[2] != 2 or sigma2.dtype != torch.float64:
        raise ValueError("%s: sigma2 must be the (B,N,2) float64 tensor of code_confidence()" % who)
    B, N, _ = sigma2.shape
    if not 1 <= N <= CONF_NMAX:
        raise ValueError("%s: N must be in 1..%d, got %d" % (who, CONF_NMAX, N))
    if not torch.is_tensor(valid) or tuple(valid.shape) != (B, N, 3) or valid.dtype != torch.uint8 or not 0 <= column < 3:
        raise ValueError("%s: valid must be the (B,N,3) uint8 tensor of correspondences(), column in 0..2" % who)
    return B, N


def rank_correspondences(sigma2, valid, column=0):
    """The ranking of row N33 alone (csrc/pnp_conf.hip, pnp_conf_rank_kernel).
      sigma2 (B,N,2) f64 CUDA tensor: code_confidence's result, pixels^2 (x, y); valid (B,N,3) uint8 from correspondences(), `column` as
      solve_pnp_ransac takes it.
    A valid keypoint is ranked iff both of its variances are finite and > 0; the key is sigma2_x + sigma2_y (one fp64 add); the order is
    ascending key, ties by ascending keypoint index.
    -> (order (B,N) int32: the ranked keypoints, best first, -1 beyond n_ranked; n_ranked (B,) int32; n_dropped (B,) int32: the valid
       keypoints that are not ranked)."""
    B, N = _check_sigma2_valid("rank_correspondences", sigma2, valid, column)
    if not (sigma2.is_cuda and valid.is_cuda):
        raise RuntimeError("checkerpose_amd.solve_conf: CUDA/HIP tensors required (no CPU fallback)")
    dev = sigma2.device
    s2 = sigma2.contiguous()
    va = valid.contiguous()
    order = torch.empty(B, N, dtype=torch.int32, device=dev)
    n_ranked = torch.empty(B, dtype=torch.int32, device=dev)
    n_dropped = torch.empty(B, dtype=torch.int32, device=dev)
    if B:
        _abi.call("cp_rank_correspondences", dev, s2, va.data_ptr() + column, 3, B, N, order, n_ranked, n_dropped)
    return order, n_ranked, n_dropped


def solve_pnp_conf(p3d_xyz, p2d, valid, sigma2, cam_K, chi2_threshold, column=0, iterations=150, seed=0, guided=True,
                   return_hypotheses=False):
    """solve_pnp_ransac (row N4) guided by per-keypoint variances (row N33; csrc/pnp_conf.hip states the rule, tests/cpnp_stages.py
    restates it).
      p3d_xyz, p2d, valid, cam_K, column, iterations, seed, return_hypotheses: as solve_pnp_ransac (the same argument checks);
      sigma2 (B,N,2) f64 CUDA tensor: code_confidence's result, passed as it is.  A valid keypoint whose variance is not finite or not
      > 0 on either axis is dropped for this call: never sampled, never an inlier;
      chi2_threshold: finite, > 0, NO default.  Keypoint i is an inlier iff du^2 / sigma2_x + dv^2 / sigma2_y <= chi2_threshold.  With
      variances that are true ones the left side is chi^2 with 2 degrees of freedom: 5.99 is its 95 % quantile, 9.21 its 99 % one.
      Nothing in the project or the reference fixes one; it is the caller's choice;
      guided=True: hypothesis h draws its 5 points from the first n_h of the ranking, n_h = the smallest n in [5, nv] with
      C(n,5) * iterations >= (h + 1) * C(nv,5) (PROSAC's growth function with T_N = iterations, no forced member, no ceiling
      recursion: the hypotheses stay independent); guided=False: from all nv ranked points, as row N4 samples.
    The stopping rule between rounds of 64 is row N4's, which assumes uniform sampling: under guidance it is merely conservative.  The
    refit over the winner's inliers is row N4's, unweighted (refine_poses_lm_weighted is the weighted polish).
    -> (R (B,3,3) f64, t (B,3,1) f64, inliers (B,N) bool, status (B,) int32, info[, hypotheses]); info = dict(order=, n_ranked=,
       n_dropped=) as rank_correspondences returns them; hypotheses (B, iterations, 14) f64 = [inlier count or -1, pool size n_h,
       R row-major, t], NaN where the solver wrote nothing."""
    if not 0 < int(iterations) <= CONF_MAX_ITERS:
        raise ValueError("iterations must be in 1..%d for cp_pnp_conf, got %r" % (CONF_MAX_ITERS, iterations))
    chi2_threshold = float(chi2_threshold)
    if not 0.0 < chi2_threshold < float("inf"):
        raise ValueError("chi2_threshold must be a finite number > 0 (5.99 / 9.21: the 95 %% / 99 %% quantiles of chi^2, 2 dof), got %r"
                         % (chi2_threshold,))
    B, N, _ = p2d.shape
    if tuple(valid.shape) != (B, N, 3) or valid.dtype != torch.uint8 or not 0 <= column < 3:
        raise ValueError("valid must be the (B,N,3) uint8 tensor of correspondences(), column in 0..2")
    if not torch.is_tensor(sigma2) or tuple(sigma2.shape) != (B, N, 2) or sigma2.dtype != torch.float64:
        raise ValueError("sigma2 must be the (B,N,2) float64 tensor of code_confidence()")
    if not (p2d.is_cuda and valid.is_cuda and sigma2.is_cuda):
        raise RuntimeError("checkerpose_amd.solve_conf: CUDA/HIP tensors required (no CPU fallback)")
    lib = _abi.load()
    dev = p2d.device
    p3 = torch.as_tensor(p3d_xyz, dtype=torch.float32, device=dev).contiguous()
    K = torch.as_tensor(cam_K, dtype=torch.float32, device=dev).contiguous()
    if p3.shape[-2:] != (N, 3) or K.shape[-2:] != (3, 3):
        raise ValueError("p3d_xyz must be (N,3) / (B,N,3) and cam_K (3,3) / (B,3,3)")
    p2 = p2d.contiguous().float()
    va = valid.contiguous()
    s2 = sigma2.contiguous()
    pose = torch.empty(B, 12, dtype=torch.float64, device=dev)
    inl = torch.empty(B, N, dtype=torch.uint8, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    order = torch.empty(B, N, dtype=torch.int32, device=dev)
    n_ranked = torch.empty(B, dtype=torch.int32, device=dev)
    n_dropped = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = lib.cp_pnp_conf_scratch_bytes(B, N)
    if return_hypotheses:
        hyp = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=dev)
        scratch = hyp.view(torch.uint8)
    else:
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _abi.call("cp_pnp_conf", dev, p3, 3 * N if p3.dim() == 3 else 0, p2, va.data_ptr() + column, 3, s2, K, 9 if K.dim() == 3 else 0, B, N,
              chi2_threshold, int(iterations), int(seed) & 0xFFFFFFFF, 1 if guided else 0, pose, inl, status, order, n_ranked, n_dropped, scratch)
    out = (pose[:, :9].view(B, 3, 3), pose[:, 9:].view(B, 3, 1), inl.bool(), status, dict(order=order, n_ranked=n_ranked, n_dropped=n_dropped))
    if return_hypotheses:
        out += (hyp[:B * int(iterations) * CONF_HYP].view(B, int(iterations), CONF_HYP),)
    return out


_CONF_KEYS = ("chi2_threshold", "floor", "guided")
_ESTIMATE_KEYS = ("img_index", "obj_ids", "padding_ratio", "crop_size", "resize_method", "check_seg", "discard_bd_pixel", "iterations", "seed")
_REFUSED_KEYS = ("solver", "refine", "graph", "depth", "dist_threshold", "icp", "spatial_coherence_weight", "prog_max_iters", "reproj_threshold")


def _check_conf(conf):
    """estimate_poses_conf's `conf` argument: a dict with chi2_threshold (optionally floor and guided)"""
    if not isinstance(conf, dict) or "chi2_threshold" not in conf:
        raise ValueError("conf must be dict(chi2_threshold=...[, floor=..., guided=...])")
    extra = [k for k in conf if k not in _CONF_KEYS]
    if extra:
        raise ValueError("conf: unknown key(s) %r (the variances are the logits' own)" % (extra,))


def estimate_poses_conf(net, frames, Bboxes, p3d_xyz, cam_K, conf, weighted=None, return_info=False, **estimate_kwargs):
    """postprocess.estimate_poses with the confidence-guided solver (row N33; RGB-only): ONE forward and one correspondences;
    code_confidence reads the same logits and the final boxes; solve_pnp_conf takes the column check_seg selects.
      conf: a dict with `chi2_threshold` (solve_pnp_conf's, no default), optionally `floor` (code_confidence's) and `guided`;
      weighted: None, or estimate_poses_weighted's dict (huber_delta, fit[, max_iters, step_tol]; a `floor` belongs in conf and is
      refused here): refine_poses_lm_weighted then runs from the solver's pose with the same sigma2;
      estimate_kwargs: estimate_poses' img_index, obj_ids, padding_ratio, crop_size, resize_method, check_seg, discard_bd_pixel,
      iterations, seed.  solver, refine, graph, depth and their companions (dist_threshold, icp, spatial_coherence_weight,
      prog_max_iters, reproj_threshold) are refused: this call IS a solver, and its gate is chi2_threshold.
    -> (R, t, inliers, status, final boxes) as estimate_poses.  return_info=True appends a dict: solve_pnp_conf's info (order, n_ranked,
       n_dropped) plus sigma2, and with `weighted` refine_poses_lm_weighted's info (refine_status under "refine_status") and the
       solver's R, t ("R0", "t0")."""
    from . import postprocess
    from .refine_weighted import _check_weighted
    _check_conf(conf)
    refused = [k for k in estimate_kwargs if k in _REFUSED_KEYS]
    if refused:
        raise ValueError("estimate_poses_conf runs its own solver: %r refused" % (refused,))
    unknown = [k for k in estimate_kwargs if k not in _ESTIMATE_KEYS]
    if unknown:
        raise TypeError("estimate_poses_conf: unexpected keyword(s) %r" % (unknown,))
    if weighted is not None:
        _check_weighted(weighted)
        if "floor" in weighted:
            raise ValueError("weighted: floor belongs in conf (one code_confidence serves the solver and the refinement)")
    kw = dict(estimate_kwargs)
    check_seg, iterations, seed = kw.pop("check_seg", False), kw.pop("iterations", 150), kw.pop("seed", 0)
    keep = {}
    p2d, valid, final = postprocess._forward_correspondences(net, frames, Bboxes, keep=keep, **kw)
    sigma2 = postprocess.code_confidence(keep["outputs"], final, **({"floor": conf["floor"]} if "floor" in conf else {}))
    column = 1 if check_seg else 0
    R, t, inl, status, info = postprocess.solve_pnp_conf(p3d_xyz, p2d, valid, sigma2, cam_K, conf["chi2_threshold"], column=column,
                                                         iterations=iterations, seed=seed, guided=conf.get("guided", True))
    info = dict(info, sigma2=sigma2)
    if weighted is not None:
        mask = inl if weighted["fit"] == "inliers" else valid[:, :, column].contiguous()
        wkw = {k: weighted[k] for k in ("max_iters", "step_tol") if k in weighted}
        R0, t0 = R, t
        R, t, rstatus, winfo = postprocess.refine_poses_lm_weighted(p3d_xyz, p2d, mask, sigma2.rsqrt().float(), cam_K, R0, t0,
                                                                    weighted["huber_delta"], status=status, **wkw)
        winfo = dict(winfo)
        winfo["refine_status"] = winfo.pop("status")
        info = dict(info, R0=R0, t0=t0, **winfo)
    if not return_info:
        return R, t, inl, status, final
    return R, t, inl, status, final, info
