"""On-device post-forward decode: the 2D-3D correspondence list the reference builds on the
host in test.py:294-329 / test_network_with_test_data.py:from_id_to_pose :50-66, computed by one HIP kernel so that
only (B,N,2) floats + (B,N,3) validity bytes leave the GPU.  The reference's PnP (Progressive-X / cv2) stays untouched and can
consume these; `solve_pnp_ransac` is the opt-in on-device twin of its cv2 branch (row N4), after which 12 doubles per crop leave."""
import numpy as np
import torch

from . import _abi
from .paste import estimate_poses_masks, paste_masks, paste_masks_rle      # noqa: F401  (row N27: checkerpose_amd/paste.py)
from .verify_mask import estimate_poses_mask_verified, verify_poses_mask   # noqa: F401  (row N28: checkerpose_amd/verify_mask.py)
from .verify_scene import estimate_poses_scene_verified, verify_scene_mask   # noqa: F401  (row N31: checkerpose_amd/verify_scene.py)
from .verify_photo import estimate_poses_photo_verified, verify_poses_photo   # noqa: F401  (row N35: checkerpose_amd/verify_photo.py)
from .refine_mask import contour_samples, estimate_poses_mask_refined, mask_extents, refine_poses_mask   # noqa: F401  (row N30: checkerpose_amd/refine_mask.py)
from .refine_weighted import code_confidence, estimate_poses_weighted, refine_poses_lm_weighted   # noqa: F401  (row N32: checkerpose_amd/refine_weighted.py)
from .solve_conf import estimate_poses_conf, rank_correspondences, solve_pnp_conf   # noqa: F401  (row N33: checkerpose_amd/solve_conf.py)
from .calibrate import CalibratedNet, add_reliability, collect_logits, fit_code_scale, reliability, reliability_figures, sigma2_consistency   # noqa: F401  (row N34: checkerpose_amd/calibrate.py)


def correspondences(outputs, roi_xy_ori=None, discard_bd_pixel=0, Bboxes=None):
    """outputs: the 6-tuple of PoseNet_GNNskip.forward (full 6+6 bits); roi_xy_ori: (B,2,H,W) fp32 CUDA tensor
    (the dataset's original-image coordinate grid of the crop, bop_dataset_pytorch.py) -- or, instead of it, Bboxes: the (B,4)
    final boxes (x, y, w, h) of the crops (`get_final_Bbox`, :188-222; host array or int32 CUDA tensor), from which the kernel
    builds the very same grid entries on the fly (16 bytes per crop travel instead of 32 KB).  Returns
    (p2d (B,N,2) f32, valid (B,N,3) uint8 [all | in full mask | in visible mask], count (B,3) int32).
    discard_bd_pixel: from_id_to_pose's border filter (test_network_with_test_data.py:60-63), 0 = off."""
    roi, xb, yb, seg, xid, yid = outputs
    if not roi.is_cuda or (roi_xy_ori is not None and not roi_xy_ori.is_cuda):
        raise RuntimeError("checkerpose_amd.postprocess: CUDA/HIP tensors required (no CPU fallback)")
    if (roi_xy_ori is None) == (Bboxes is None):
        raise ValueError("give either roi_xy_ori or Bboxes")
    B, _, N = roi.shape
    H, W = seg.shape[2], seg.shape[3]
    if roi_xy_ori is not None and tuple(roi_xy_ori.shape) != (B, 2, H, W):
        raise ValueError("roi_xy_ori must be (B,2,%d,%d)" % (H, W))
    lib = _abi.load()
    # the three logit views are slices of one (B,13,N) block when they come from the module; rebuild it otherwise
    base = roi._base if roi._base is not None and tuple(roi._base.shape) == (B, 13, N) else None
    bits = base if base is not None else torch.cat([roi, xb, yb], 1).contiguous()
    if bits.shape[1] != 13:
        raise ValueError("need the full 13-row logit block (all refinement stages active)")
    seg = seg.contiguous(); xid = xid.contiguous(); yid = yid.contiguous()
    p2d = torch.empty(B, N, 2, dtype=torch.float32, device=roi.device)
    valid = torch.empty(B, N, 3, dtype=torch.uint8, device=roi.device)
    count = torch.empty(B, 3, dtype=torch.int32, device=roi.device)
    st = torch.cuda.current_stream(roi.device).cuda_stream
    if Bboxes is not None:
        bb = Bboxes if torch.is_tensor(Bboxes) else torch.as_tensor(np.asarray(Bboxes), dtype=torch.int32)
        bb = bb.to(device=roi.device, dtype=torch.int32).contiguous()
        if tuple(bb.shape) != (B, 4):
            raise ValueError("Bboxes must be (B,4): x, y, w, h of every crop")
        _abi.check(lib.cp_correspondences_bbox(st, bits.data_ptr(), seg.data_ptr(), xid.data_ptr(), yid.data_ptr(), bb.data_ptr(),
                                               p2d.data_ptr(), valid.data_ptr(), count.data_ptr(), B, N, H, W, int(discard_bd_pixel)),
                   "cp_correspondences_bbox")
        return p2d, valid, count
    rxy = roi_xy_ori.contiguous().float()
    _abi.check(lib.cp_correspondences(st, bits.data_ptr(), seg.data_ptr(), xid.data_ptr(), yid.data_ptr(), rxy.data_ptr(),
                                      p2d.data_ptr(), valid.data_ptr(), count.data_ptr(), B, N, H, W, int(discard_bd_pixel)),
               "cp_correspondences")
    return p2d, valid, count


PNP_MAX_ITERS = 256        # csrc/pnp.hip: 4 rounds of 64 hypotheses


def solve_pnp_ransac(p3d_xyz, p2d, valid, cam_K, column=0, reproj_threshold=2.0, iterations=150, seed=0, return_hypotheses=False):
    """On-device twin of from_id_to_pose's cv2 branch (test_network_with_test_data.py:100-114; defaults reprojErr_thresh=2,
    cv_max_iters=150): EPnP + RANSAC over the correspondences of `correspondences()`.
      p3d_xyz (N,3) or (B,N,3) model keypoints in original units; p2d (B,N,2), valid (B,N,3) from correspondences();
      column 0 = all RoI keypoints | 1 = also inside the full mask | 2 = inside the visible mask (check_seg variants);
      cam_K (3,3) or (B,3,3).
    Returns (R (B,3,3) f64, t (B,3,1) f64, inliers (B,N) bool, status (B,) int32: 0 = the reference's identity fallback).
    return_hypotheses=True adds a fifth value, the solver's hypothesis records as a (B, iterations, 14) f64 tensor
    ([inlier count or -1, unused, R row-major, t]; include/checkerpose_hip.h), NaN where the solver wrote nothing: what
    tests/pnp_stages.py replays.  It costs one fill of the scratch; the default path is unchanged."""
    if not 0 < int(iterations) <= PNP_MAX_ITERS:        # no silent clamp: cv2 would run them all
        raise ValueError("iterations (cv_max_iters) must be in 1..%d for cp_pnp_ransac, got %r" % (PNP_MAX_ITERS, iterations))
    B, N, _ = p2d.shape
    if tuple(valid.shape) != (B, N, 3) or valid.dtype != torch.uint8 or not 0 <= column < 3:
        raise ValueError("valid must be the (B,N,3) uint8 tensor of correspondences(), column in 0..2")
    if not (p2d.is_cuda and valid.is_cuda):
        raise RuntimeError("checkerpose_amd.postprocess: CUDA/HIP tensors required (no CPU fallback)")
    lib = _abi.load()
    dev = p2d.device
    p3 = torch.as_tensor(p3d_xyz, dtype=torch.float32, device=dev).contiguous()
    K = torch.as_tensor(cam_K, dtype=torch.float32, device=dev).contiguous()
    if p3.shape[-2:] != (N, 3) or K.shape[-2:] != (3, 3):
        raise ValueError("p3d_xyz must be (N,3) / (B,N,3) and cam_K (3,3) / (B,3,3)")
    p2 = p2d.contiguous().float()
    va = valid.contiguous()
    pose = torch.empty(B, 12, dtype=torch.float64, device=dev)
    inl = torch.empty(B, N, dtype=torch.uint8, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = lib.cp_pnp_ransac_scratch_bytes(B, N)
    if return_hypotheses:
        hyp = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=dev)
        scratch = hyp.view(torch.uint8)
    else:
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _abi.check(lib.cp_pnp_ransac(st, p3.data_ptr(), 3 * N if p3.dim() == 3 else 0, p2.data_ptr(), va.data_ptr() + column, 3, K.data_ptr(),
                                 9 if K.dim() == 3 else 0, B, N, float(reproj_threshold), int(iterations), int(seed) & 0xFFFFFFFF,
                                 pose.data_ptr(), inl.data_ptr(), status.data_ptr(), scratch.data_ptr()), "cp_pnp_ransac")
    out = (pose[:, :9].view(B, 3, 3), pose[:, 9:].view(B, 3, 1), inl.bool(), status)
    if return_hypotheses:
        out += (hyp[:B * int(iterations) * 14].view(B, int(iterations), 14),)
    return out


GC_MAX_ITERS, GC_NMAX, GC_MAX_EDGES, GC_LO_MAX, GC_Q = 512, 4096, 1 << 21, 8, 1 << 16        # csrc/pnp_gc.hip


class RadiusGraph:
    """The neighbourhood graphs of M objects (radius_graph): CSR on the device.  offsets (M,N+1) int32 = row starts of object m
    relative to base[m]; indices int32 = neighbours, ascending per row; base (M,) int64; totals = directed edges per object (host)."""

    def __init__(self, offsets, indices, base, totals, radius):
        self.offsets, self.indices, self.base, self.totals, self.radius = offsets, indices, base, [int(x) for x in totals], float(radius)
        self.M, self.N = int(offsets.shape[0]), int(offsets.shape[1]) - 1
        self.max_edges, self.n_indices = max(self.totals), sum(self.totals)

    def neighbours(self, m=0):
        """object m's graph on the host: (offsets (N+1,), indices) numpy int32"""
        b = sum(self.totals[:m])
        return self.offsets[m].cpu().numpy(), self.indices[b:b + self.totals[m]].cpu().numpy()


def radius_graph(p3d_xyz, radius=20.0, device="cuda:0"):
    """Row N17, once per object: the graph over which solve_pnp_gc's Potts term acts (the reference's neighborhood_ball_radius = 20).
    p3d_xyz (N,3) or (M,N,3) model keypoints (a tensor on a device stays there); pair {i,j}, i != j, is an edge when the squared
    distance, in fp64 from the fp32 coordinates, is <= radius^2.  MODEL space: static per object and symmetric -- which space
    pyprogressivex's FLANN radius graph lives in cannot be checked here (parity UNPINNED).  N <= 4096, at most 2^21 directed edges
    per object (ValueError).  Two launches (count, fill) with one host read of the edge totals in between."""
    if torch.is_tensor(p3d_xyz) and p3d_xyz.is_cuda:
        device = p3d_xyz.device
    pts = torch.as_tensor(p3d_xyz, dtype=torch.float32)
    if pts.dim() == 2:
        pts = pts[None]
    if pts.dim() != 3 or pts.shape[2] != 3 or not 1 <= pts.shape[1] <= GC_NMAX or pts.shape[0] < 1:
        raise ValueError("p3d_xyz must be (N,3) or (M,N,3) with 1 <= N <= %d, got %r" % (GC_NMAX, tuple(pts.shape)))
    radius = float(radius)
    if not 0.0 <= radius < 1e150:
        raise ValueError("radius must be a finite number >= 0, got %r" % radius)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("checkerpose_amd.postprocess: CUDA/HIP tensors required (no CPU fallback)")
    lib = _abi.load()
    pts = pts.to(dev).contiguous()
    M, N = int(pts.shape[0]), int(pts.shape[1])
    offsets = torch.empty(M, N + 1, dtype=torch.int32, device=dev)
    totals = torch.empty(M, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _abi.check(lib.cp_radius_graph_count(st, pts.data_ptr(), M, N, radius, offsets.data_ptr(), totals.data_ptr()), "cp_radius_graph_count")
        tot = totals.cpu().tolist()
        if max(tot) > GC_MAX_EDGES:
            raise ValueError("radius_graph: object %d has %d directed edges at radius %g, more than %d" % (tot.index(max(tot)), max(tot), radius, GC_MAX_EDGES))
        base = torch.tensor([sum(tot[:m]) for m in range(M)], dtype=torch.int64).to(dev)
        indices = torch.empty(max(sum(tot), 1), dtype=torch.int32, device=dev)
        _abi.check(lib.cp_radius_graph_fill(st, pts.data_ptr(), M, N, radius, offsets.data_ptr(), base.data_ptr(), indices.data_ptr(), sum(tot)),
                   "cp_radius_graph_fill")
    return RadiusGraph(offsets, indices, base, tot, radius)


def graphcut_label(cin, offsets, indices, w):
    """cp_graphcut_label: the labelling step of solve_pnp_gc alone.  cin (B,N) / (N,) int32 CUDA (-1 = not a node), one symmetric CSR
    graph (offsets (N+1,), indices, columns ascending, int32 CUDA), w = capacity per direction of an edge (integer, Q = 65536 is the
    source capacity).  -> (labels (B,N) bool = the minimal source side of a minimum cut, flow value (B,) int64, status (B,) int32,
    sweeps (B,) int32); RuntimeError where the kernel's sweep bound did not suffice."""
    if not (cin.is_cuda and offsets.is_cuda and indices.is_cuda):
        raise RuntimeError("checkerpose_amd.postprocess: CUDA/HIP tensors required (no CPU fallback)")
    if cin.dim() == 1:
        cin = cin[None]
    B, N = cin.shape
    if cin.dtype != torch.int32 or offsets.dtype != torch.int32 or indices.dtype != torch.int32 or tuple(offsets.shape) != (N + 1,):
        raise ValueError("cin (B,N), offsets (N+1,), indices: int32 tensors")
    E = int(indices.numel())
    if not 1 <= N <= GC_NMAX or E > GC_MAX_EDGES or not 0 <= int(w) <= 1 << 28:
        raise ValueError("N in 1..%d, at most %d directed edges, w in 0..2^28" % (GC_NMAX, GC_MAX_EDGES))
    lib = _abi.load()
    dev = cin.device
    cin, offsets = cin.contiguous(), offsets.contiguous()
    indices = indices.contiguous() if E else torch.zeros(1, dtype=torch.int32, device=dev)
    labels = torch.empty(B, N, dtype=torch.uint8, device=dev)
    flow = torch.empty(B, dtype=torch.int64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    sweeps = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(B * max(E, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _abi.check(lib.cp_graphcut_label(st, cin.data_ptr(), offsets.data_ptr(), indices.data_ptr(), B, N, E, int(w), labels.data_ptr(),
                                         flow.data_ptr(), status.data_ptr(), sweeps.data_ptr(), scratch.data_ptr(), scratch.numel() * 4),
                   "cp_graphcut_label")
    bad = torch.nonzero(status < 0).flatten().tolist()
    if bad:
        raise RuntimeError("cp_graphcut_label: problem %d hit the sweep bound (status %d)" % (bad[0], int(status[bad[0]])))
    return labels.bool(), flow, status, sweeps


def solve_pnp_gc(p3d_xyz, p2d, valid, cam_K, graph, graph_ids=None, column=0, reproj_threshold=2.0, spatial_coherence_weight=0.1,
                 iterations=400, min_inliers=6, seed=0, return_stages=False):
    """Graph-cut RANSAC on the device (row N17): what the reference's `--use_progressivex` branch (pyprogressivex.find6DPoses with
    maximum_model_number = 1, test_network_with_test_data.py:68-99) comes down to.  The rule is this project's own -- parity with
    pyprogressivex (its sampler, confidence default, unary kernel, inner RANSAC, neighbourhood space, PEARL's model validation) is
    UNPINNED; tests/gc_stages.py restates it in numpy, include/checkerpose_hip.h states it in full:
      hypotheses from 4 correspondences (P3P + the fourth point), MSAC score, OpenCV's stopping rule between rounds of 64;
      the winner's inlier set = the minimal source side of the minimum cut of [unary: squared residual / threshold^2 against 1;
      Potts: spatial_coherence_weight per edge of `graph` between two valid points], in integers (Q = 65536);
      EPnP over that set, repeated (at most 8 times) while the MSAC score improves.
    Inputs and outputs as solve_pnp_ransac; graph = radius_graph(...) of the model keypoints, graph_ids (B,) = the object of each crop
    (required when the graph holds more than one); iterations in 1..512; fewer than min_inliers valid points or labelled inliers ->
    the identity with status 0 (the reference's `num_valid >= 6` rule).
    -> (R (B,3,3) f64, t (B,3,1) f64, inliers (B,N) bool, status (B,) int32[, stages]); stages (return_stages=True): dict with
       hypotheses (B,iterations,14) f64 [count or -1, score, R, t], steps (B,9,30) f64 [k, P_k (12), score(P_k), |L_k|, refit ok,
       Q_k (12), score(Q_k), sweeps], cin (B,9,N) int32 (-1 invalid; -2 where the step did not run), labels (B,9,N) uint8 (255 where
       the step did not run); NaN where the solver wrote nothing.
    RuntimeError naming the crop where the max-flow's sweep bound was hit (never an approximate labelling)."""
    if not 0 < int(iterations) <= GC_MAX_ITERS:          # no silent clamp
        raise ValueError("iterations (prog_max_iters) must be in 1..%d for cp_pnp_gc, got %r" % (GC_MAX_ITERS, iterations))
    if not isinstance(graph, RadiusGraph):
        raise ValueError("graph must be the RadiusGraph of the model keypoints (postprocess.radius_graph)")
    B, N, _ = p2d.shape
    if tuple(valid.shape) != (B, N, 3) or valid.dtype != torch.uint8 or not 0 <= column < 3:
        raise ValueError("valid must be the (B,N,3) uint8 tensor of correspondences(), column in 0..2")
    if graph.N != N:
        raise ValueError("the graph is over %d keypoints, the crops have %d" % (graph.N, N))
    if graph.M > 1 and graph_ids is None:
        raise ValueError("graph_ids is required: the graph holds %d objects" % graph.M)
    lam = float(spatial_coherence_weight)
    if not 0.0 <= lam <= 4096.0:
        raise ValueError("spatial_coherence_weight must be in 0..4096, got %r" % spatial_coherence_weight)
    if not 4 <= int(min_inliers) or not float(reproj_threshold) > 0:
        raise ValueError("min_inliers must be >= 4 and reproj_threshold > 0")
    if not (p2d.is_cuda and valid.is_cuda):
        raise RuntimeError("checkerpose_amd.postprocess: CUDA/HIP tensors required (no CPU fallback)")
    lib = _abi.load()
    dev = p2d.device
    gid = None
    if graph_ids is not None:
        gid = torch.as_tensor(graph_ids).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(gid.shape) != (B,):
            raise ValueError("graph_ids must be (B,)")
    p3 = torch.as_tensor(p3d_xyz, dtype=torch.float32, device=dev).contiguous()
    K = torch.as_tensor(cam_K, dtype=torch.float32, device=dev).contiguous()
    if p3.shape[-2:] != (N, 3) or K.shape[-2:] != (3, 3):
        raise ValueError("p3d_xyz must be (N,3) / (B,N,3) and cam_K (3,3) / (B,3,3)")
    p2 = p2d.contiguous().float()
    va = valid.contiguous()
    pose = torch.empty(B, 12, dtype=torch.float64, device=dev)
    inl = torch.empty(B, N, dtype=torch.uint8, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = lib.cp_pnp_gc_scratch_bytes(B, N, graph.max_edges)
    if nbytes == 0:
        raise ValueError("cp_pnp_gc: bad shape (B = %d, N = %d, max_edges = %d)" % (B, N, graph.max_edges))
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    S = GC_LO_MAX + 1
    o_steps = B * GC_MAX_ITERS * 14
    o_cin = (o_steps + B * S * 30) * 8
    o_lab = o_cin + B * S * N * 4
    raw = scratch.view(torch.uint8)
    if return_stages:
        scratch[:o_steps + B * S * 30] = float("nan")
        raw[o_cin:o_lab].view(torch.int32).fill_(-2)
        raw[o_lab:o_lab + B * S * N].fill_(255)
    w = int(np.floor(lam * GC_Q + 0.5))
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _abi.check(lib.cp_pnp_gc(st, p3.data_ptr(), 3 * N if p3.dim() == 3 else 0, p2.data_ptr(), va.data_ptr() + column, 3, K.data_ptr(),
                                 9 if K.dim() == 3 else 0, graph.offsets.data_ptr(), graph.indices.data_ptr(), graph.base.data_ptr(),
                                 gid.data_ptr() if gid is not None else None, graph.M, graph.max_edges, graph.n_indices, B, N,
                                 float(reproj_threshold), w, int(iterations), int(min_inliers), int(seed) & 0xFFFFFFFF,
                                 pose.data_ptr(), inl.data_ptr(), status.data_ptr(), scratch.data_ptr()), "cp_pnp_gc")
    bad = torch.nonzero(status < 0).flatten().tolist()
    if bad:
        code = int(status[bad[0]])
        raise RuntimeError("cp_pnp_gc: crop %d %s (status %d); %d of %d crops failed"
                           % (bad[0], "hit the max-flow's sweep bound" if code == -1 else "names a graph outside the RadiusGraph", code, len(bad), B))
    out = (pose[:, :9].view(B, 3, 3), pose[:, 9:].view(B, 3, 1), inl.bool(), status)
    if return_stages:
        out += (dict(hypotheses=scratch[:B * int(iterations) * 14].view(B, int(iterations), 14),
                     steps=scratch[o_steps:o_steps + B * S * 30].view(B, S, 30),
                     cin=raw[o_cin:o_lab].view(torch.int32).view(B, S, N), labels=raw[o_lab:o_lab + B * S * N].view(B, S, N)),)
    return out


LM_MAX_ITERS, LM_NMAX, LM_RECORD, LM_INFO = 64, 4096, 17, 40        # csrc/pnp_refine.hip


def refine_poses_lm(p3d_xyz, p2d, mask, cam_K, R, t, status=None, max_iters=20, step_tol=1e-10, return_records=False):
    """Levenberg-Marquardt polish of solved poses on the device (row N22; opt-in -- the reference does not refine): minimises the
    squared reprojection error over each crop's selected correspondences, starting from (R, t).  What cv2.solvePnPRefineLM does for
    a cv2 user, under this project's own rule (csrc/pnp_refine.hip states it, tests/lm_stages.py restates it; parity with cv2 UNPINNED).
      p3d_xyz (N,3) / (B,N,3), p2d (B,N,2), cam_K (3,3) / (B,3,3): as solve_pnp_ransac; mask (B,N) bool or uint8: the points to fit,
      e.g. the `inliers` of solve_pnp_ransac / solve_pnp_gc; R (B,3,3), t (B,3,1) / (B,3): the poses to start from; status (B,) or
      None: crops whose entry is 0 (the solvers' identity fallback) are left alone; max_iters in 1..64; step_tol > 0.
    -> (R (B,3,3) f64, t (B,3,1) f64, refine_status (B,) int32, info[, records])
       refine_status: 1 = stopped by the step rule, 2 = max_iters ran out, 3 = lambda passed 1e8, 0 = pass-through (the input pose,
       bitwise: status 0 given, fewer than 6 selected points, a non-finite pose or selected pixel, a selected point behind the camera);
       info: dict of device tensors -- cost0, cost (B,) f64: sums of squared pixels at the input / returned pose; n (B,) int64
       selected points; iters (B,) int64; H (B,6,6) f64: the undamped J^T J at the returned pose (rotation then translation);
       status = refine_status.  Pass-through rows hold NaN in cost0, cost and H.
       records (return_records=True): (B, max_iters, 17) f64, [lambda, c, c', accepted, s, R' (9), t' (3)] per executed iteration,
       NaN where none ran."""
    max_iters = int(max_iters)
    if not 1 <= max_iters <= LM_MAX_ITERS:
        raise ValueError("max_iters must be in 1..%d for cp_pnp_refine_lm, got %r" % (LM_MAX_ITERS, max_iters))
    step_tol = float(step_tol)
    if not 0.0 < step_tol < float("inf"):
        raise ValueError("step_tol must be a finite number > 0, got %r" % (step_tol,))
    if p2d.dim() != 3 or p2d.shape[2] != 2:
        raise ValueError("p2d must be (B,N,2), got %r" % (tuple(p2d.shape),))
    B, N, _ = p2d.shape
    if not 1 <= N <= LM_NMAX:
        raise ValueError("p2d: N must be in 1..%d, got %d" % (LM_NMAX, N))
    if not torch.is_tensor(mask) or tuple(mask.shape) != (B, N) or mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError("mask must be a (B,N) bool or uint8 tensor")
    if not torch.is_tensor(R) or not torch.is_tensor(t) or tuple(R.shape) != (B, 3, 3) or tuple(t.shape) not in ((B, 3, 1), (B, 3)):
        raise ValueError("R must be (B,3,3) and t (B,3,1) / (B,3) tensors")
    if status is not None and (not torch.is_tensor(status) or tuple(status.shape) != (B,)):
        raise ValueError("status must be a (B,) tensor or None")
    if not (p2d.is_cuda and mask.is_cuda and R.is_cuda and t.is_cuda and (status is None or status.is_cuda)):
        raise RuntimeError("checkerpose_amd.postprocess: CUDA/HIP tensors required (no CPU fallback)")
    lib = _abi.load()
    dev = p2d.device
    p3 = torch.as_tensor(p3d_xyz, dtype=torch.float32, device=dev).contiguous()
    K = torch.as_tensor(cam_K, dtype=torch.float32, device=dev).contiguous()
    if p3.shape[-2:] != (N, 3) or K.shape[-2:] != (3, 3) or (p3.dim() == 3 and p3.shape[0] != B) or (K.dim() == 3 and K.shape[0] != B):
        raise ValueError("p3d_xyz must be (N,3) / (B,N,3) and cam_K (3,3) / (B,3,3)")
    p2 = p2d.contiguous().float()
    mk = mask.contiguous().view(torch.uint8)
    pose_in = torch.cat([R.reshape(B, 9).to(dev, torch.float64), t.reshape(B, 3).to(dev, torch.float64)], 1).contiguous()
    st_in = None if status is None else status.to(device=dev, dtype=torch.int32).contiguous()
    pose = torch.empty(B, 12, dtype=torch.float64, device=dev)
    rstatus = torch.empty(B, dtype=torch.int32, device=dev)
    info = torch.empty(B, LM_INFO, dtype=torch.float64, device=dev)
    rec = torch.full((B, max_iters, LM_RECORD), float("nan"), dtype=torch.float64, device=dev) if return_records else None
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _abi.check(lib.cp_pnp_refine_lm(st, p3.data_ptr(), 3 * N if p3.dim() == 3 else 0, p2.data_ptr(), mk.data_ptr(), 1, K.data_ptr(),
                                        9 if K.dim() == 3 else 0, B, N, pose_in.data_ptr(), st_in.data_ptr() if st_in is not None else None,
                                        max_iters, step_tol, pose.data_ptr(), rstatus.data_ptr(), info.data_ptr(),
                                        rec.data_ptr() if rec is not None else None), "cp_pnp_refine_lm")
    out_info = dict(cost0=info[:, 0], cost=info[:, 1], n=info[:, 2].long(), iters=info[:, 3].long(), H=info[:, 4:].view(B, 6, 6), status=rstatus)
    out = (pose[:, :9].view(B, 3, 3), pose[:, 9:].view(B, 3, 1), rstatus, out_info)
    if return_records:
        out += (rec,)
    return out


def pose_covariance(info, sigma=None):
    """First-order covariance of the refined poses' increments (w, v) from refine_poses_lm's `info`: sigma^2 inv(H), (B,6,6) f64 on
    the device, rotation (radians) then translation (units of the model).  sigma: the pixel noise's standard deviation (a number or
    a (B,) tensor); None = estimated per crop from the residuals, sigma^2 = cost / (2 n - 6).  Rows that were not refined (status 0)
    or have no redundancy (2 n <= 6) are NaN.  Plain torch on the device."""
    H, n, status = info["H"], info["n"], info["status"]
    B = H.shape[0]
    dof = 2 * n - 6
    ok = (status != 0) & (dof > 0)
    if sigma is None:
        s2 = info["cost"] / dof.clamp(min=1).to(torch.float64)
    else:
        s2 = torch.as_tensor(sigma, dtype=torch.float64, device=H.device).expand(B) ** 2
    eye = torch.eye(6, dtype=torch.float64, device=H.device).expand(B, 6, 6)
    inv = torch.linalg.inv(torch.where(ok[:, None, None], H, eye))
    cov = s2[:, None, None] * inv
    return torch.where(ok[:, None, None], cov, torch.full_like(cov, float("nan")))


ICP_MAX_ITERS, ICP_GRID_MAX, ICP_RECORD, ICP_INFO = 64, 64, 18, 42        # csrc/icp_refine.hip
_SAMPLE_KEYS = ("rect", "shape", "pixel", "depth", "face", "X", "N", "ok")


def _check_grid(grid):
    grid = int(grid)
    if not 1 <= grid <= ICP_GRID_MAX:
        raise ValueError("grid must be in 1..%d, got %r" % (ICP_GRID_MAX, grid))
    return grid


def surface_samples(R, t, cam_K, meshes, size, mesh_ids=None, grid=32):
    """Stage A of refine_poses_icp (row N24) on its own: ONE raster pass of the P poses of `meshes` (a MeshSet with faces) on a frame of
    size = (width, height), then per pose a lattice of at most grid x grid pixels over its projected rectangle inside the frame
    (csrc/icp_refine.hip states the rule).  S = grid * grid slots per pose; slot j * nx + i is lattice pixel (i, j), slots beyond nx * ny
    are empty.  -> dict of device tensors:
      rect (P,4) int32 x0 y0 x1 y1 (-1 four times when empty); shape (P,2) int32 nx ny; pixel (P,S,2) int32; depth (P,S) f32:
      metric.render_depth's value at the pixel; face (P,S) int32: the winning face, -1 = empty slot; X (P,S,3) f64 the model-space
      point, N (P,S,3) f64 the face's unit normal towards the camera (NaN in empty slots); ok (P,) int32: 0 where the pose was not
      rendered (a non-finite entry, a vertex at Z <= 0, a mesh id out of range)."""
    from . import scene
    grid = _check_grid(grid)
    dev, poses, P = scene.mesh_poses(R, t, meshes)
    K, k_stride = scene.camera(cam_K, P, dev, "P")
    ids, (vmax,) = scene.mesh_ids_on(mesh_ids, P, dev, meshes.sizes)
    W, H = scene.frame_size(size)
    verts, v_off = meshes.on(dev)
    faces, f_off, _ = meshes.faces_on(dev)
    S = grid * grid
    out = dict(rect=torch.empty((P, 4), dtype=torch.int32, device=dev), shape=torch.empty((P, 2), dtype=torch.int32, device=dev),
               pixel=torch.empty((P, S, 2), dtype=torch.int32, device=dev), depth=torch.empty((P, S), dtype=torch.float32, device=dev),
               face=torch.empty((P, S), dtype=torch.int32, device=dev), X=torch.empty((P, S, 3), dtype=torch.float64, device=dev),
               N=torch.empty((P, S, 3), dtype=torch.float64, device=dev), ok=torch.empty((P,), dtype=torch.int32, device=dev))
    scratch = torch.empty(_abi.load().cp_surface_samples_scratch_bytes(P, vmax), dtype=torch.uint8, device=dev)
    _abi.call("cp_surface_samples", dev, poses, K, k_stride, verts, v_off, faces, f_off, len(meshes), ids, H, W, P, vmax, grid,
              *[out[k] for k in _SAMPLE_KEYS], scratch)
    return out


def refine_poses_icp(R, t, cam_K, meshes, depth, max_dist, image_ids=None, mesh_ids=None, status=None, grid=32, max_iters=20, step_tol=1e-6,
                     min_pairs=6, inertia=1e-2, samples=None, return_records=False):
    """Projective point-to-plane ICP of poses against the sensor's depth image on the device (row N24; opt-in -- the reference does not
    refine): what a user with an RGB-D frame runs after an RGB-only estimate, whose error is largest along the viewing ray.  The rule
    is this project's own (csrc/icp_refine.hip states it, tests/icp_stages.py restates it; parity with any ICP library UNPINNED):
    surface samples of each mesh rendered ONCE at the input pose (surface_samples), re-associated with the depth pixel they project
    to after every accepted step, point-to-plane residuals with the normals frozen per association, Levenberg-Marquardt with a step
    bound and an absolute damping term.
      R (P,3,3), t (P,3,1) / (P,3): the poses to start from (CUDA/HIP tensors); cam_K (3,3) / (P,3,3); meshes: a MeshSet with faces
      (its diameters give rho = diameter / 2); depth (H,W) / (I,H,W) in the meshes' units with image_ids (P,) when poses share images
      (as `depth_test` elsewhere); mesh_ids (P,) with several meshes; status (P,) or None: poses whose entry is 0 are left alone.
      max_dist: a number or a (P,) tensor in the meshes' units, NO default: pairs farther apart than this are dropped (occluders,
      background) and no step moves the object by more.  Nothing in the project or the reference fixes one; a fraction of the mesh
      diameter (0.1 - 0.3) is a reasonable start, and it is the caller's choice.
      grid in 1..64: the lattice per pose; max_iters in 1..64; step_tol > 0; min_pairs >= 6; inertia >= 0: the weight of the absolute
      damping term inertia * n * diag(rho^2 x 3, 1 x 3) (UNPINNED design default 1e-2; 0 lets a box seen face-on slide along its faces);
      samples: a surface_samples(...) result for THESE poses, so that several depth hypotheses share one render (grid is then its).
    A box seen nearly face-on stays weakly constrained in the face's plane: that is point-to-plane's nature, not tuned away.
    -> (R (P,3,3) f64, t (P,3,1) f64, refine_status (P,) int32, info[, records])
       refine_status: 1 = an accepted step below step_tol, 2 = max_iters ran out, 3 = lambda passed 1e8 or fewer than min_pairs pairs
       were left after a step, 0 = pass-through (the input pose, bitwise: status 0 given, a non-finite pose or cam_K, a pose that is not
       rendered, fewer than min_pairs samples or pairs under the input pose);
       info: dict of device tensors -- cost0, cost (P,) f64: sums of squared point-to-plane distances at the input / returned pose;
       n_samples, n0, n (P,) int64: samples, pairs at the input pose, pairs at the returned pose; iters (P,) int64; H (P,6,6) f64: the
       undamped J^T J at the returned pose over its pairs (rotation then translation); status = refine_status.  Pass-through rows hold
       NaN in cost0, cost and H.
       records (return_records=True): (P, max_iters, 18) f64, [lambda, n, c, c', accepted, s, R' (9), t' (3)] per executed iteration,
       NaN where none ran."""
    from . import scene
    max_iters, min_pairs, step_tol, inertia = int(max_iters), int(min_pairs), float(step_tol), float(inertia)
    if not 1 <= max_iters <= ICP_MAX_ITERS:
        raise ValueError("max_iters must be in 1..%d for cp_icp_refine, got %r" % (ICP_MAX_ITERS, max_iters))
    if not 0.0 < step_tol < float("inf"):
        raise ValueError("step_tol must be a finite number > 0, got %r" % (step_tol,))
    if min_pairs < 6:
        raise ValueError("min_pairs must be >= 6, got %r" % (min_pairs,))
    if not 0.0 <= inertia < float("inf"):
        raise ValueError("inertia must be a finite number >= 0, got %r" % (inertia,))
    grid = _check_grid(grid)
    dev, poses, P = scene.mesh_poses(R, t, meshes)
    if torch.is_tensor(max_dist):
        scene.require_cuda("postprocess", max_dist)
        if max_dist.numel() != P:
            raise ValueError("max_dist must be a number or a (P,) tensor")
        md = max_dist.reshape(P).to(device=dev, dtype=torch.float64).contiguous()
    else:
        if not 0.0 < float(max_dist) < float("inf"):
            raise ValueError("max_dist must be a finite number > 0 (in the meshes' units), got %r" % (max_dist,))
        md = torch.full((P,), float(max_dist), dtype=torch.float64, device=dev)
    if torch.is_tensor(depth):
        scene.require_cuda("postprocess", depth)
    if status is not None and (not torch.is_tensor(status) or tuple(status.shape) != (P,)):
        raise ValueError("status must be a (P,) tensor or None")
    if status is not None:
        scene.require_cuda("postprocess", status)
    K, k_stride = scene.camera(cam_K, P, dev, "P")
    ids, _ = scene.mesh_ids_on(mesh_ids, P, dev, meshes.sizes)
    images, img_ids, n_img = scene.depth_images(depth, image_ids, P, dev)
    H, W = int(images.shape[1]), int(images.shape[2])
    if samples is None:
        samples = surface_samples(R, t, cam_K, meshes, (W, H), mesh_ids=mesh_ids, grid=grid)
    else:
        if not isinstance(samples, dict) or any(k not in samples for k in _SAMPLE_KEYS):
            raise ValueError("samples must be the dict surface_samples returns")
        scene.require_cuda("postprocess", *[samples[k] for k in _SAMPLE_KEYS])
        S = int(samples["face"].shape[1]) if samples["face"].dim() == 2 else 0
        if tuple(samples["face"].shape) != (P, S) or tuple(samples["X"].shape) != (P, S, 3) or tuple(samples["N"].shape) != (P, S, 3) or not 1 <= S <= ICP_GRID_MAX ** 2:
            raise ValueError("samples do not belong to these %d poses" % P)
    sX, sN, sF = samples["X"].contiguous(), samples["N"].contiguous(), samples["face"].contiguous()
    if sX.dtype != torch.float64 or sN.dtype != torch.float64 or sF.dtype != torch.int32:
        raise ValueError("samples must be the dict surface_samples returns")
    S = int(sF.shape[1])
    _, _, diam = meshes.faces_on(dev)
    st_in = None if status is None else status.to(device=dev, dtype=torch.int32).contiguous()
    pose = torch.empty(P, 12, dtype=torch.float64, device=dev)
    rstatus = torch.empty(P, dtype=torch.int32, device=dev)
    info = torch.empty(P, ICP_INFO, dtype=torch.float64, device=dev)
    rec = torch.full((P, max_iters, ICP_RECORD), float("nan"), dtype=torch.float64, device=dev) if return_records else None
    _abi.call("cp_icp_refine", dev, poses, K, k_stride, sX, sN, sF, S, images, img_ids, n_img, H, W, md, diam, len(meshes), ids, st_in,
              max_iters, step_tol, min_pairs, inertia, P, pose, rstatus, info, rec)
    out_info = dict(cost0=info[:, 0], cost=info[:, 1], n_samples=info[:, 2].long(), n0=info[:, 3].long(), n=info[:, 4].long(),
                    iters=info[:, 5].long(), H=info[:, 6:].view(P, 6, 6), status=rstatus)
    out = (pose[:, :9].view(P, 3, 3), pose[:, 9:].view(P, 3, 1), rstatus, out_info)
    if return_records:
        out += (rec,)
    return out


DEPTH_POSE_MAX_ITERS, DEPTH_POSE_NMAX, DEPTH_POSE_RECORD, DEPTH_POSE_STEPS = 256, 4096, 14, 4        # csrc/pose_depth.hip


def _depth_pose_inputs(who, p2d, valid, cam_K, depth, image_ids, column):
    """the arguments lift_correspondences and solve_pose_depth share -> (dev, B, N, p2d, valid, K, K stride, images, image ids, I, H, W)"""
    from . import scene
    if not torch.is_tensor(p2d) or p2d.dim() != 3 or p2d.shape[2] != 2:
        raise ValueError("p2d must be a (B,N,2) tensor")
    B, N, _ = p2d.shape
    if not 1 <= N <= DEPTH_POSE_NMAX:
        raise ValueError("p2d: N must be in 1..%d for %s, got %d" % (DEPTH_POSE_NMAX, who, N))
    if not torch.is_tensor(valid) or tuple(valid.shape) != (B, N, 3) or valid.dtype != torch.uint8 or not 0 <= int(column) < 3:
        raise ValueError("valid must be the (B,N,3) uint8 tensor of correspondences(), column in 0..2")
    scene.require_cuda("postprocess", p2d, valid)
    if torch.is_tensor(depth):
        scene.require_cuda("postprocess", depth)
    dev = p2d.device
    K = torch.as_tensor(cam_K, dtype=torch.float32, device=dev).contiguous()
    if K.shape[-2:] != (3, 3) or K.dim() not in (2, 3) or (K.dim() == 3 and K.shape[0] != B):
        raise ValueError("cam_K must be (3,3) / (B,3,3)")
    images, ids, n_img = scene.depth_images(depth, image_ids, B, dev)
    return (dev, B, N, p2d.contiguous().float(), valid.contiguous(), K, 9 if K.dim() == 3 else 0, images, ids, n_img,
            int(images.shape[1]), int(images.shape[2]))


def lift_correspondences(p2d, valid, cam_K, depth, image_ids=None, column=0):
    """Stage A of solve_pose_depth (row N25) on its own: each valid correspondence lifted to a camera-frame point by the sensor's depth
    under it.  p2d (B,N,2), valid (B,N,3) from correspondences(), column as solve_pnp_ransac; cam_K (3,3) / (B,3,3); depth (H,W) /
    (I,H,W) in the keypoints' units with image_ids (B,) when crops share images (as `depth_test` elsewhere).  A keypoint with
    (u, v) = its p2d reads z = depth[floor v, floor u]; it is dropped outside the frame or where z is not finite or <= 0, else
    Q = ((u - cx) / fx z, (v - cy) / fy z, z): the ray through (u, v) as given, not through the pixel centre.
    -> (Q (B,N,3) f32, 0 where not lifted; lifted (B,N) bool; n_lifted (B,) int32)"""
    dev, B, N, p2, va, K, ks, images, ids, n_img, H, W = _depth_pose_inputs("cp_lift_correspondences", p2d, valid, cam_K, depth, image_ids, column)
    Q = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
    lifted = torch.empty(B, N, dtype=torch.uint8, device=dev)
    n_lifted = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:                                            # nothing to launch (an empty tensor has no address to hand over)
        return Q, lifted.bool(), n_lifted
    _abi.call("cp_lift_correspondences", dev, p2, va.data_ptr() + int(column), 3, K, ks, images, ids, n_img, H, W, B, N, Q, lifted, n_lifted)
    return Q, lifted.bool(), n_lifted


def solve_pose_depth(p3d_xyz, p2d, valid, cam_K, depth, dist_threshold, image_ids=None, column=0, iterations=150, seed=0,
                     return_hypotheses=False):
    """Pose from depth-lifted correspondences on the device (row N25; opt-in -- the reference uses no depth at test time): with the
    sensor's depth under each correspondence the 2-D -- 3-D problem of solve_pnp_ransac becomes a 3-D -- 3-D one, solved by RANSAC over
    three-pair absolute orientation and a least-squares fit over the inliers, re-evaluated at most 3 times while the inlier set grows.
    No mesh, no start pose.  The rule is this project's own (csrc/pose_depth.hip states it, tests/depth_pose_stages.py restates it).
      p3d_xyz, p2d, valid, column, cam_K, iterations (1..256), seed as solve_pnp_ransac; depth, image_ids as lift_correspondences.
      dist_threshold: a number or a (B,) tensor in the keypoints' units, NO default: a lifted point farther than this from the posed
      model point is an outlier (occluders, background, wrong codes).  Nothing in the project or the reference fixes one; the depth
      noise plus the model-space size of a grid cell is a reasonable start, and it is the caller's choice.
    -> (R (B,3,3) f64, t (B,3,1) f64, inliers (B,N) bool, status (B,) int32: 0 = the identity fallback -- fewer than 3 lifted
       keypoints, no hypothesis with 3 inliers, or a threshold entry that is not positive and finite)
    return_hypotheses=True adds a fifth value, the solver's records as a dict of device tensors: hypotheses (B,iterations,14) f64
    [inlier count or -1, unused, R row-major, t], steps (B,4,14) f64 [the step's inlier count, accepted, R, t after the step], NaN where
    the solver wrote nothing; Q, lifted (uint8), n_lifted: stage A's outputs."""
    iterations = int(iterations)
    if not 0 < iterations <= DEPTH_POSE_MAX_ITERS:        # no silent clamp
        raise ValueError("iterations must be in 1..%d for cp_pose_depth_ransac, got %r" % (DEPTH_POSE_MAX_ITERS, iterations))
    dev, B, N, p2, va, K, ks, images, ids, n_img, H, W = _depth_pose_inputs("cp_pose_depth_ransac", p2d, valid, cam_K, depth, image_ids, column)
    thr_b, thr = None, 0.0
    if torch.is_tensor(dist_threshold):
        if not dist_threshold.is_cuda:
            raise RuntimeError("checkerpose_amd.postprocess: CUDA/HIP tensors required (no CPU fallback)")
        if dist_threshold.numel() != B:
            raise ValueError("dist_threshold must be a number or a (B,) tensor")
        thr_b = dist_threshold.reshape(B).to(device=dev, dtype=torch.float64).contiguous()
    else:
        if dist_threshold is None or not 0.0 < float(dist_threshold) < float("inf"):
            raise ValueError("dist_threshold must be a finite number > 0 (in the keypoints' units), got %r" % (dist_threshold,))
        thr = float(dist_threshold)
    p3 = torch.as_tensor(p3d_xyz, dtype=torch.float32, device=dev).contiguous()
    if p3.shape[-2:] != (N, 3) or p3.dim() not in (2, 3) or (p3.dim() == 3 and p3.shape[0] != B):
        raise ValueError("p3d_xyz must be (N,3) / (B,N,3)")
    pose = torch.empty(B, 12, dtype=torch.float64, device=dev)
    inl = torch.empty(B, N, dtype=torch.uint8, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:                                            # nothing to launch
        out = (pose[:, :9].view(0, 3, 3), pose[:, 9:].view(0, 3, 1), inl.bool(), status)
        if return_hypotheses:
            out += (dict(hypotheses=pose.new_empty(0, iterations, DEPTH_POSE_RECORD), steps=pose.new_empty(0, DEPTH_POSE_STEPS, DEPTH_POSE_RECORD),
                         Q=p2.new_empty(0, N, 3), n_lifted=status.new_empty(0), lifted=inl.new_empty(0, N)),)
        return out
    nbytes = _abi.load().cp_pose_depth_ransac_scratch_bytes(B, N, iterations)
    o_steps = B * iterations * DEPTH_POSE_RECORD
    o_q = o_steps + B * DEPTH_POSE_STEPS * DEPTH_POSE_RECORD
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    if return_hypotheses:
        scratch[:o_q] = float("nan")
    _abi.call("cp_pose_depth_ransac", dev, p3, 3 * N if p3.dim() == 3 else 0, p2, va.data_ptr() + int(column), 3, K, ks, images, ids, n_img,
              H, W, B, N, thr, thr_b, iterations, int(seed) & 0xFFFFFFFF, pose, inl, status, scratch)
    out = (pose[:, :9].view(B, 3, 3), pose[:, 9:].view(B, 3, 1), inl.bool(), status)
    if return_hypotheses:
        raw = scratch.view(torch.uint8)
        b_q, b_n = o_q * 8, o_q * 8 + B * N * 12
        out += (dict(hypotheses=scratch[:o_steps].view(B, iterations, DEPTH_POSE_RECORD),
                     steps=scratch[o_steps:o_q].view(B, DEPTH_POSE_STEPS, DEPTH_POSE_RECORD),
                     Q=raw[b_q:b_n].view(torch.float32).view(B, N, 3), n_lifted=raw[b_n:b_n + 4 * B].view(torch.int32),
                     lifted=raw[b_n + 4 * B:b_n + 4 * B + B * N].view(B, N)),)
    return out


VERIFY_MAX_PIXELS, VERIFY_CMAX = 1 << 24, 64        # csrc/pose_verify.hip
VERIFY_COUNTS = ("n_model", "n_missing", "n_match", "n_occluded", "n_through", "sum_q")
VERIFY_LABELS = ("none", "match", "occluded", "through", "missing")        # the label map's values 0..4


def verify_poses(R, t, cam_K, meshes, depth, tau, image_ids=None, mesh_ids=None, status=None, occlusion_weight=1.0, return_labels=False):
    """Hypothesis verification of poses against the sensor's depth image on the device (row N26; opt-in -- the reference does not
    verify): each pose is rendered and compared pixel by pixel with what the sensor saw, inside one tile kernel -- no depth frame is
    stored.  The rule is this project's own (csrc/pose_verify.hip states it, tests/verify_stages.py restates it).  With D the pose's
    render (metric.render_depth's bits) and S the sensor's depth, every pixel with D > 0 is a model pixel and is
      missing (S not finite or <= 0) | match (|S - D| <= tau) | occluded (S - D < -tau: something in front of the model) |
      through (S - D > tau: the sensor saw past the model's surface);
    a match also adds q = min(63, int(64 |S - D| / tau)) to sum_q (fp32).  fit = n_match - sum_q / 64,
    den = n_match + n_through + occlusion_weight n_occluded, score = fit / den in [0, 1]: a per-pose confidence that comes from the pose.
      R (P,3,3), t (P,3,1) / (P,3): CUDA/HIP tensors; cam_K (3,3) / (P,3,3); meshes: a MeshSet with faces; depth (H,W) / (I,H,W) in the
      meshes' units with image_ids (P,) when poses share images (as `depth_test` elsewhere; H W <= 2^24); mesh_ids (P,) with several
      meshes; status (P,) or None: a pose whose entry is 0 (the solvers' identity fallback) is no candidate.
      tau: a number or a (P,) tensor in the meshes' units, NO default: the depth tolerance.  Nothing in the project or the reference
      fixes one; the sensor's noise plus the pose error still to be accepted is a reasonable start (BOP's VSD uses 20 mm), and it is the
      caller's choice.  occlusion_weight in [0, 1] (default 1: every measured model pixel that does not support the pose counts against
      it; lower it where occluders are expected).
    -> (score (P,) f64, info[, labels (P,H,W) uint8: 0 none, 1 match, 2 occluded, 3 through, 4 missing])
       info: dict of device tensors -- n_model, n_missing, n_match, n_occluded, n_through, sum_q (P,) int32; ok (P,) bool; fit, den (P,)
       f64.  score is NaN with ok False when den == 0 or the pose is not counted (all counts 0): a non-finite pose or cam_K, a vertex at
       Z <= 0, an image or mesh id out of range, status 0, a tau entry that as float32 is not positive and finite.  Every output is a
       function of integer sums: bitwise the same for a pose alone or in a batch, with or without labels."""
    from . import scene
    occlusion_weight = float(occlusion_weight)
    if not 0.0 <= occlusion_weight <= 1.0:
        raise ValueError("occlusion_weight must be in [0, 1], got %r" % (occlusion_weight,))
    if not torch.is_tensor(tau) and (tau is None or not 0.0 < float(tau) < float("inf")):
        raise ValueError("tau must be a finite number > 0 (in the meshes' units), got %r" % (tau,))
    dev, poses, P = scene.mesh_poses(R, t, meshes)
    if torch.is_tensor(tau):
        scene.require_cuda("postprocess", tau)
        if tau.numel() != P:
            raise ValueError("tau must be a number or a (P,) tensor")
        tau_d = tau.reshape(P).to(device=dev, dtype=torch.float64).contiguous()
    else:
        tau_d = torch.full((P,), float(tau), dtype=torch.float64, device=dev)
    if torch.is_tensor(depth):
        scene.require_cuda("postprocess", depth)
    if status is not None and (not torch.is_tensor(status) or tuple(status.shape) != (P,)):
        raise ValueError("status must be a (P,) tensor or None")
    if status is not None:
        scene.require_cuda("postprocess", status)
    K, k_stride = scene.camera(cam_K, P, dev, "P")
    ids, (vmax,) = scene.mesh_ids_on(mesh_ids, P, dev, meshes.sizes)
    images, img_ids, n_img = scene.depth_images(depth, image_ids, P, dev)
    H, W = int(images.shape[1]), int(images.shape[2])
    if H * W > VERIFY_MAX_PIXELS:
        raise ValueError("depth: H * W must be <= 2^24 for cp_verify_poses (its sums are int32), got %d x %d" % (H, W))
    verts, v_off = meshes.on(dev)
    faces, f_off, _ = meshes.faces_on(dev)
    st_in = None if status is None else status.to(device=dev, dtype=torch.int32).contiguous()
    counts = torch.empty((P, len(VERIFY_COUNTS)), dtype=torch.int32, device=dev)
    score, fit, den = (torch.empty((P,), dtype=torch.float64, device=dev) for _ in range(3))
    ok = torch.empty((P,), dtype=torch.uint8, device=dev)
    labels = torch.empty((P, H, W), dtype=torch.uint8, device=dev) if return_labels else None
    scratch = torch.empty(_abi.load().cp_verify_poses_scratch_bytes(P, vmax), dtype=torch.uint8, device=dev)
    _abi.call("cp_verify_poses", dev, poses, K, k_stride, verts, v_off, faces, f_off, len(meshes), ids, images, img_ids, n_img, H, W, tau_d,
              st_in, occlusion_weight, P, vmax, counts, score, fit, den, ok, labels, scratch)
    info = {k: counts[:, i] for i, k in enumerate(VERIFY_COUNTS)}
    info.update(ok=ok.bool(), fit=fit, den=den)
    return (score, info, labels) if return_labels else (score, info)


def select_poses(score, ok=None, R=None, t=None):
    """The choice among C candidate poses of each of B crops on the device (row N26): score (C,B) as verify_poses gives it for poses laid
    out candidate-major, ok (C,B) bool / uint8 or None (then every score that is not NaN is eligible).  Per crop the eligible candidate
    with the largest score wins, the smallest candidate index on equal scores, candidate 0 when none is eligible.  C <= 64.
    -> choice (B,) int32, or (choice, R_sel (B,3,3), t_sel (B,3,1)) when R (C,B,3,3) and t (C,B,3,1) are given: plain indexing, the
       chosen candidate's bits."""
    from . import scene
    if not torch.is_tensor(score) or score.dim() != 2 or not 1 <= score.shape[0] <= VERIFY_CMAX:
        raise ValueError("score must be a (C,B) tensor with C in 1..%d" % VERIFY_CMAX)
    C_, B = int(score.shape[0]), int(score.shape[1])
    if ok is not None and (not torch.is_tensor(ok) or tuple(ok.shape) != (C_, B) or ok.dtype not in (torch.bool, torch.uint8)):
        raise ValueError("ok must be a (C,B) bool or uint8 tensor or None")
    if (R is None) != (t is None):
        raise ValueError("give both R (C,B,3,3) and t (C,B,3,1), or neither")
    if R is not None and (not torch.is_tensor(R) or not torch.is_tensor(t) or tuple(R.shape) != (C_, B, 3, 3) or tuple(t.shape) != (C_, B, 3, 1)):
        raise ValueError("R must be (C,B,3,3) and t (C,B,3,1) tensors")
    scene.require_cuda("postprocess", score, *[x for x in (ok, R, t) if x is not None])
    dev = score.device
    sc = score.to(torch.float64).contiguous()
    okb = None if ok is None else ok.to(dev).contiguous().view(torch.uint8)
    choice = torch.empty((B,), dtype=torch.int32, device=dev)
    if B:                                                 # (an empty tensor has no address to hand over)
        _abi.call("cp_select_poses", dev, sc, okb, C_, B, choice)
    if R is None:
        return choice
    idx, cols = choice.long(), torch.arange(B, device=dev)
    return choice, R[idx, cols], t[idx, cols]


REFINES = (None, "lm", "icp", "lm+icp")


def _check_refine(refine, allowed=(None, "lm")):
    if refine not in allowed:
        raise ValueError("refine must be %s, got %r" % (" or ".join("None" if a is None else repr(a) for a in allowed), refine))


def _check_icp(refine, icp):
    """estimate_poses' `icp` argument: required with an "icp" refinement, a dict with meshes, depth and max_dist"""
    if refine in ("icp", "lm+icp"):
        if not isinstance(icp, dict) or any(k not in icp for k in ("meshes", "depth", "max_dist")):
            raise ValueError("refine=%r needs icp=dict(meshes=..., depth=..., max_dist=...[, mesh_ids=..., ...])" % (refine,))
        if "image_ids" in icp or "status" in icp or "samples" in icp:
            raise ValueError("icp must not name image_ids, status or samples: they are the call's img_index and the solver's status")


def _check_verify(verify):
    """estimate_poses_verified's `verify` argument: a dict with meshes, depth and tau (optionally mesh_ids and occlusion_weight)"""
    if not isinstance(verify, dict) or any(k not in verify for k in ("meshes", "depth", "tau")):
        raise ValueError("verify must be dict(meshes=..., depth=..., tau=...[, mesh_ids=..., occlusion_weight=...])")
    if "image_ids" in verify or "status" in verify:
        raise ValueError("verify must not name image_ids or status: they are the call's img_index and the solver's status")
    extra = [k for k in verify if k not in ("meshes", "depth", "tau", "mesh_ids", "occlusion_weight")]
    if extra:
        raise ValueError("verify: unknown key(s) %r" % (extra,))


def estimate_poses(net, frames, Bboxes, p3d_xyz, cam_K, img_index=None, obj_ids=None, padding_ratio=1.5, crop_size=256,
                   resize_method="crop_square_resize", check_seg=False, discard_bd_pixel=0, reproj_threshold=2.0, iterations=150, seed=0, solver="epnp",
                   graph=None, spatial_coherence_weight=0.1, prog_max_iters=400, refine=None, icp=None, depth=None,
                   dist_threshold=None):
    """The inner loop of the reference's test.py (:198-330) for a whole batch without leaving the GPU: detection boxes on full uint8
    frames -> padded RoI crops (`padding_Bbox` + `get_roi`, bop_dataset_pytorch.py:344-354; preprocess.get_roi_batch) -> network forward
    (uint8 input, normalised on the device) -> correspondences from the crops' final boxes (`get_final_Bbox`; N2) -> EPnP + RANSAC (N4).
      frames: uint8 CUDA tensor (n_img, H, W, 3) or (H, W, 3); Bboxes: (B, 4) detection boxes (x, y, w, h), None = no detection;
      p3d_xyz (N,3) / (B,N,3) model keypoints in original units; cam_K (3,3) / (B,3,3); obj_ids for the LM shared estimator.
      solver "epnp" (default): solve_pnp_ransac; "gc": solve_pnp_gc (row N17, the `--use_progressivex` path) over `graph` =
      radius_graph(p3d_xyz) with spatial_coherence_weight and prog_max_iters iterations; obj_ids then also name each crop's graph.
      "depth" (row N25): solve_pose_depth over the correspondences lifted by `depth` ((H,W) / (n_img,H,W), in the units of p3d_xyz) with
      `dist_threshold` (no default) and `iterations`; each crop's image is the call's img_index.  Both keywords are required with
      "depth" and refused with the other solvers; reproj_threshold plays no part.
      refine None (default): the solver's pose as it is; "lm" (row N22): refine_poses_lm over the solver's inliers at its defaults,
      with either solver -- the returned R, t are then the refined ones, inliers and status still the solver's.
      "icp" (row N24): refine_poses_icp against the frames' depth, "lm+icp": N22 first, then N24.  Both need icp = a dict with
      `meshes` (a MeshSet with faces, in the units of p3d_xyz), `depth` ((H,W) / (n_img,H,W)) and `max_dist`, and optionally `mesh_ids`
      and refine_poses_icp's other keywords; each crop's image is the call's img_index.
      The last stage's pose is returned as it is; estimate_poses_verified (row N26) runs the same stages and keeps per crop the stage's
      pose that the frames' depth supports best.
    -> (R (B,3,3) f64, t (B,3,1) f64, inliers (B,N) bool, status (B,) int32 (0: identity fallback), final boxes (B,4) int array)"""
    stages, inl, status, final = _estimate_stages(**locals())        # (the first statement: locals() holds the arguments alone)
    return stages[-1][1], stages[-1][2], inl, status, final


def _forward_correspondences(net, frames, Bboxes, img_index=None, obj_ids=None, padding_ratio=1.5, crop_size=256,
                             resize_method="crop_square_resize", discard_bd_pixel=0, keep=None):
    """_estimate_stages up to and including correspondences -- crops, ONE forward, the final boxes -- without a solver run
    (estimate_poses_conf brings its own).  keep: as _estimate_stages fills it.  -> (p2d, valid, final boxes)"""
    from . import preprocess as PP
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    H, W = int(frames.shape[1]), int(frames.shape[2])
    padded = [None if b is None else PP.padding_Bbox(b, padding_ratio) for b in Bboxes]
    crops = PP.get_roi_batch(frames, padded, crop_size, PP.INTER_LINEAR, resize_method, img_index=img_index)
    final = np.array([[0, 0, 0, 0] if b is None else PP.get_final_Bbox(b, resize_method, W, H) for b in padded], dtype=np.int32)
    with torch.no_grad():
        out = net(crops, None) if obj_ids is None else net(crops, None, obj_ids)
    if keep is not None:
        keep["seg"], keep["padded"] = out[3], padded
    p2d, valid, _ = correspondences(out, discard_bd_pixel=discard_bd_pixel, Bboxes=final)
    if keep is not None:
        keep["outputs"], keep["p2d"], keep["valid"] = out, p2d, valid
    return p2d, valid, final


def _estimate_stages(net, frames, Bboxes, p3d_xyz, cam_K, img_index=None, obj_ids=None, padding_ratio=1.5, crop_size=256,
                     resize_method="crop_square_resize", check_seg=False, discard_bd_pixel=0, reproj_threshold=2.0, iterations=150, seed=0,
                     solver="epnp", graph=None, spatial_coherence_weight=0.1, prog_max_iters=400, refine=None, icp=None, depth=None,
                     dist_threshold=None, keep=None):
    """estimate_poses' arguments -> (stages: [(name, R, t)] after the solver, "lm" and "icp" as far as `refine` runs them, inliers, status,
    final boxes).  keep: a dict that receives the forward's `seg` logits and the `padded` boxes of the crops (estimate_poses_masks), and the
    forward's whole `outputs`, `p2d` and `valid` of correspondences (estimate_poses_weighted)"""
    from . import preprocess as PP
    if solver not in ("epnp", "gc", "depth"):
        raise ValueError("solver must be 'epnp', 'gc' or 'depth', got %r" % (solver,))
    if solver == "depth" and (depth is None or dist_threshold is None):
        raise ValueError("solver='depth' needs depth=... (the frames' depth images) and dist_threshold=... (no default)")
    if solver != "depth" and (depth is not None or dist_threshold is not None):
        raise ValueError("depth and dist_threshold belong to solver='depth', got solver=%r" % (solver,))
    _check_refine(refine, REFINES)
    _check_icp(refine, icp)
    if solver == "gc" and graph is None:
        raise ValueError("solver='gc' needs graph=radius_graph(p3d_xyz)")
    p2d, valid, final = _forward_correspondences(net, frames, Bboxes, img_index, obj_ids, padding_ratio, crop_size, resize_method,
                                                 discard_bd_pixel, keep)
    if solver == "gc":
        R, t, inl, status = solve_pnp_gc(p3d_xyz, p2d, valid, cam_K, graph, graph_ids=obj_ids if graph.M > 1 else None,
                                         column=1 if check_seg else 0, reproj_threshold=reproj_threshold,
                                         spatial_coherence_weight=spatial_coherence_weight, iterations=prog_max_iters, seed=seed)
    elif solver == "depth":
        R, t, inl, status = solve_pose_depth(p3d_xyz, p2d, valid, cam_K, depth, dist_threshold, image_ids=img_index,
                                             column=1 if check_seg else 0, iterations=iterations, seed=seed)
    else:
        R, t, inl, status = solve_pnp_ransac(p3d_xyz, p2d, valid, cam_K, column=1 if check_seg else 0, reproj_threshold=reproj_threshold,
                                             iterations=iterations, seed=seed)
    stages = [("solver", R, t)]
    if refine in ("lm", "lm+icp"):
        R, t = refine_poses_lm(p3d_xyz, p2d, inl, cam_K, R, t, status=status)[:2]
        stages.append(("lm", R, t))
    if refine in ("icp", "lm+icp"):
        kw = {k: v for k, v in icp.items() if k not in ("meshes", "depth", "max_dist")}
        R, t = refine_poses_icp(R, t, cam_K, icp["meshes"], icp["depth"], icp["max_dist"], image_ids=img_index, status=status, **kw)[:2]
        stages.append(("icp", R, t))
    return stages, inl, status, final


def estimate_poses_verified(net, frames, Bboxes, p3d_xyz, cam_K, verify, return_verify=False, **estimate_kwargs):
    """estimate_poses with hypothesis verification (row N26): the same call (estimate_kwargs are estimate_poses' keywords), but instead
    of the last stage's pose unconditionally, the poses after each stage the call runs -- the solver's, then after "lm", then after
    "icp": 1, 2 or 3 candidates per crop -- are scored by ONE verify_poses call against the frames' depth and ONE select_poses keeps per
    crop the one the sensor supports.
      verify: a dict with `meshes` (a MeshSet with faces, in the units of p3d_xyz), `depth` ((H,W) / (n_img,H,W)), `tau` (no default) and
      optionally `mesh_ids` and `occlusion_weight`; each crop's image is the call's img_index and a crop with solver status 0 is no
      candidate, so `image_ids` and `status` are refused.
    -> (R, t, inliers, status, final boxes) as estimate_poses: R, t the chosen candidates' (their bits), inliers and status still the
       solver's; return_verify=True appends a dict: score (C,B), choice (B,) int32, stages (a tuple of "solver" / "lm" / "icp") and info
       (verify_poses' dict over the C * B poses, candidate-major)."""
    _check_verify(verify)
    stages, inl, status, final = _estimate_stages(net, frames, Bboxes, p3d_xyz, cam_K, **estimate_kwargs)
    R, t, report = _verify_stages(stages, cam_K, estimate_kwargs.get("img_index"), status, verify)
    return (R, t, inl, status, final, report) if return_verify else (R, t, inl, status, final)


def _verify_stages(stages, cam_K, img_index, status, verify):
    """estimate_poses_verified's verification: the stages' poses candidate-major through ONE verify_poses and ONE select_poses
    -> (R, t of the chosen candidates, the report of return_verify)"""
    C_, B = len(stages), int(stages[0][1].shape[0])
    Rc = torch.stack([r.reshape(B, 3, 3) for _, r, _ in stages])
    tc = torch.stack([x.reshape(B, 3, 1) for _, _, x in stages])

    def per_candidate(x):                                 # a per-crop (B,) argument -> (C * B,), candidate-major
        if x is None:
            return None
        return x.reshape(-1).repeat(C_) if torch.is_tensor(x) else np.tile(np.asarray(x).reshape(-1), C_)

    K = cam_K if torch.is_tensor(cam_K) else np.asarray(cam_K)
    if K.ndim == 3:
        K = K.repeat(C_, 1, 1) if torch.is_tensor(K) else np.tile(K, (C_, 1, 1))
    depth, tau = verify["depth"], verify["tau"]
    if img_index is None and B > 1 and getattr(depth, "ndim", 0) == 3 and len(depth) == B:
        img_index = np.arange(B)                          # the default rule (image b for crop b), said before the crops are stacked
    score, info = verify_poses(Rc.reshape(C_ * B, 3, 3), tc.reshape(C_ * B, 3, 1), K, verify["meshes"], depth,
                               per_candidate(tau) if torch.is_tensor(tau) else tau, image_ids=per_candidate(img_index),
                               mesh_ids=per_candidate(verify.get("mesh_ids")), status=per_candidate(status),
                               occlusion_weight=verify.get("occlusion_weight", 1.0))
    score = score.view(C_, B)
    choice, R, t = select_poses(score, info["ok"].view(C_, B), Rc, tc)
    return R, t, dict(score=score, choice=choice, stages=tuple(n for n, _, _ in stages), info=info)


def evaluate_poses(net, frames, Bboxes, p3d_xyz, cam_K, R_gt, t_gt, vertices, mesh_ids=None, kinds=("add", "adi"), symmetries=None,
                   depth_test=None, image_ids=None, size=None, **estimate_kwargs):
    """estimate_poses followed by metric.pose_errors against the given ground-truth poses: test.py's loop body from the detection
    boxes to the ADD / ADD-S errors (:198-427) with only the errors leaving the GPU.
      R_gt (B,3,3), t_gt (B,3,1) / (B,3): tensors or host arrays; vertices: a (V,3) array, a list with mesh_ids, or a metric.MeshSet
      (units of p3d_xyz); estimate_kwargs go to estimate_poses.  Crops whose solver fell back to the identity pose (status 0) are
      scored with it, as the reference scores them (from_id_to_pose returns R = I, t = 0 and test.py goes on).
      kinds may also name "mssd", "mspd", "proj" (metric.bop_errors, with cam_K and `symmetries`: a metric.SymmetrySet, a list of
      bop_toolkit `syms` lists, or None = the identity alone); without them nothing more is launched.
      kind "vsd" (metric.vsd_errors at its defaults) needs `depth_test` (H,W) / (I,H,W) in the units of `vertices`, a MeshSet with
      faces, and `image_ids` (B,) when poses share images; its errors are (B, T), one column per tau.
      kinds "cus" / "cou_bb_proj" (metric.mask_errors, no sphere shortcut) need `size` = (W, H) of the frame and a MeshSet with faces.
      A `verify` keyword (row N26) routes the call through estimate_poses_verified: the scored poses are then the chosen ones;
      `return_verify` is refused: this call's return has no place for the report -- call estimate_poses_verified itself for it.
    -> (errors: dict kind -> (B,) f64 CUDA tensor, R, t, inliers, status, final boxes)"""
    from . import metric
    if "return_verify" in estimate_kwargs:
        raise ValueError("evaluate_poses does not return the verification's report (return_verify): call estimate_poses_verified for it")
    verify = estimate_kwargs.pop("verify", None)
    if verify is None:
        R, t, inl, status, final = estimate_poses(net, frames, Bboxes, p3d_xyz, cam_K, **estimate_kwargs)
    else:
        R, t, inl, status, final = estimate_poses_verified(net, frames, Bboxes, p3d_xyz, cam_K, verify, **estimate_kwargs)
    errors = metric.score_poses(R, t, R_gt, t_gt, cam_K, vertices, mesh_ids=mesh_ids, kinds=kinds, symmetries=symmetries,
                                depth_test=depth_test, image_ids=image_ids, size=size)
    return errors, R, t, inl, status, final


def from_id_to_pose(p3d_xyz, roi_xy_ori, cam_K, roi_mask_bit, pixel_x_id, pixel_y_id, check_seg=False, seg_mask=None,
                    use_progressivex=False, neighborhood_ball_radius=20, spatial_coherence_weight=0.1, prog_max_iters=400,
                    discard_bd_pixel=0, return_inliers=False, reprojErr_thresh=2, cv_max_iters=150, device="cuda:0", seed=0,
                    progx_backend=None, refine=None):
    """Same name, arguments (numpy arrays of ONE image) and returns as the reference's `from_id_to_pose`
    (test_network_with_test_data.py:32-115), with its cv2 branch running on the device (`cp_pnp_ransac`):
      the validity mask is built exactly as :50-66 (RoI bit > 0.5, optional seg mask at the predicted pixel, optional border
      discard), then EPnP + RANSAC (reprojErr_thresh, cv_max_iters) -> R (3,3), t (3,1) [, inlier indices into ALL keypoints];
      fewer than 4 valid correspondences -> R = I, t = 0, inliers None (:111-114).
    `use_progressivex=True` is the third-party pyprogressivex solver of the reference and is not rebuilt: ValueError, unless
    progx_backend="device" asks for this project's graph-cut RANSAC (solve_pnp_gc, row N17; parity with pyprogressivex UNPINNED):
    neighborhood_ball_radius -> radius_graph, spatial_coherence_weight, prog_max_iters, reprojErr_thresh -> the solver; fewer than 6
    valid points -> the identity; inliers None, as in the reference (:99).
    refine="lm" (row N22, not in the reference) polishes a solved pose over the solver's inliers with refine_poses_lm at its defaults,
    on the device cv2 twin and on progx_backend="device" alike; None (default) leaves the solver's pose as it is.
    For whole batches straight from the network's outputs use correspondences() + solve_pnp_ransac() instead."""
    import numpy as np
    if progx_backend not in (None, "device"):
        raise ValueError("progx_backend must be None or 'device', got %r" % (progx_backend,))
    _check_refine(refine)
    if use_progressivex and progx_backend is None:
        raise ValueError("use_progressivex=True needs the third-party pyprogressivex solver, which is not built; "
                         "progx_backend='device' runs this project's graph-cut RANSAC (solve_pnp_gc) in its place")
    num_all_pt = p3d_xyz.shape[0]
    roi_h, roi_w, _ = roi_xy_ori.shape
    disc_p2d = roi_xy_ori[pixel_y_id, pixel_x_id]
    valid_mask = (roi_mask_bit[:, 0] > 0.5)
    if check_seg:
        valid_mask = np.logical_and(valid_mask, seg_mask[pixel_y_id, pixel_x_id] > 0.5)
    if discard_bd_pixel > 0:
        bd_mask = np.zeros((roi_h, roi_w))
        bd_mask[discard_bd_pixel:(roi_h - discard_bd_pixel), discard_bd_pixel:(roi_w - discard_bd_pixel)] = 1.0
        valid_mask = np.logical_and(valid_mask, bd_mask[pixel_y_id, pixel_x_id] > 0.5)
    if use_progressivex:
        R_predict, t_predict, inliers = np.eye(3), np.zeros((3, 1)), None
        if int(valid_mask.sum()) >= 6:                # :68
            dev = torch.device(device)
            valid = torch.zeros(1, num_all_pt, 3, dtype=torch.uint8, device=dev)
            valid[0, :, 0] = torch.from_numpy(np.ascontiguousarray(valid_mask)).to(dev)
            p2d = torch.from_numpy(np.ascontiguousarray(disc_p2d, dtype=np.float32)).to(dev)[None]
            p3 = torch.from_numpy(np.ascontiguousarray(p3d_xyz, dtype=np.float32)).to(dev)
            Kd = torch.from_numpy(np.ascontiguousarray(cam_K, dtype=np.float32)).to(dev)
            R, t, inl, status = solve_pnp_gc(p3, p2d, valid, Kd, radius_graph(p3, float(neighborhood_ball_radius)), column=0,
                                             reproj_threshold=float(reprojErr_thresh), spatial_coherence_weight=float(spatial_coherence_weight),
                                             iterations=int(prog_max_iters), seed=seed)
            if refine == "lm":
                R, t = refine_poses_lm(p3, p2d, inl, Kd, R, t, status=status)[:2]
            if int(status[0]) == 1:
                R_predict, t_predict = R[0].cpu().numpy(), t[0].cpu().numpy()
    elif int(valid_mask.sum()) < 4:
        R_predict, t_predict, inliers = np.eye(3), np.zeros((3, 1)), None
    else:
        dev = torch.device(device)
        valid = torch.zeros(1, num_all_pt, 3, dtype=torch.uint8, device=dev)
        valid[0, :, 0] = torch.from_numpy(np.ascontiguousarray(valid_mask)).to(dev)
        p2d = torch.from_numpy(np.ascontiguousarray(disc_p2d, dtype=np.float32)).to(dev)[None]
        p3 = torch.from_numpy(np.ascontiguousarray(p3d_xyz, dtype=np.float32)).to(dev)
        Kd = torch.from_numpy(np.ascontiguousarray(cam_K, dtype=np.float32)).to(dev)
        R, t, inl, status = solve_pnp_ransac(p3, p2d, valid, Kd, column=0,
                                             reproj_threshold=float(reprojErr_thresh), iterations=int(cv_max_iters), seed=seed)
        if refine == "lm":
            R, t = refine_poses_lm(p3, p2d, inl, Kd, R, t, status=status)[:2]
        if int(status[0]) == 1:
            R_predict, t_predict = R[0].cpu().numpy(), t[0].cpu().numpy()
            inliers = np.nonzero(inl[0].cpu().numpy())[0]
        else:                                     # no hypothesis with a full sample of inliers: cv2 reports failure; identity like :111-114
            R_predict, t_predict, inliers = np.eye(3), np.zeros((3, 1)), None
    if return_inliers:
        return R_predict, t_predict, inliers
    return R_predict, t_predict
