"""Self-occlusion measure on the device: the reference's preprocess_data/get_overall_visibility.py -- step 6 of
its data preparation, the measure of the paper's section 3.5 -- without qhull and without the host.

  compute_vis_hpr(points, viewpoint=None, radius_param=2.0)   the reference's name, arguments and return (:20-42): one view
  hpr_visibility(vertices, R, t=(0, 0, 400))                  n_views poses of one cloud in ONE cp_hpr_visibility call -> device counts
                                                              (V,) int32 (and the (n_views, V) uint8 mask on request)
  overall_visibility(vertices, R=None, ...)                   the script's statistic: mean, min, max, the nine `below` ratios
The per-view rule is PINNED: Katz et al.'s spherical flip in numpy's own fp64 expressions, then the vertex set of the convex hull of
the flipped points plus the viewpoint, by a bounded, deterministic insertion that reproduces qhull's vertex
sets on every recorded case (tests/golden/visibility.npz: what the reference's own function returned, each decision at least 1e-6
cloud units from a tie; closer to a tie than that, qhull's own merging decides and nothing is claimed).
The DEFAULT VIEW SET of overall_visibility is UNPINNED: the reference reads its 2 562 rotations from datasets/sampled_poses_2562.pkl,
a file it does not ship; with R=None the views are the rotations of render.sample_views(min_n_views) (hinter_sampling's 2 562 at the
default).  Pass the pickle's rotations as R to reproduce a published figure.
Not rebuilt: the reference's V = 3 case (qhull accepts three points plus the viewpoint; V < 4 raises ValueError here), clouds of
float32 computed in float32 (everything is promoted to float64, as prepare.pack_clouds does) and reading PLY files.
There is no CPU fallback."""
import math

import numpy as np
import torch

from . import _abi, scene
from .prepare import pack_clouds

STATUS = {1: "degenerate cloud: the flipped points are coincident, collinear or coplanar",
          2: "the horizon of an insertion is not a simple cycle",
          3: "face table full",
          4: "more insertions than points",
          5: "a vertex at the viewpoint or a non-finite norm"}
RADIUS_PARAM_MAX = 8.0           # radius = max norm * 10^radius_param: beyond this the flipped cloud's relief drowns in fp64


def _radius_param(radius_param):
    rp = float(radius_param)
    if not (math.isfinite(rp) and 0.0 <= rp <= RADIUS_PARAM_MAX):
        raise ValueError("radius_param must be a finite number in [0, %g], got %r" % (RADIUS_PARAM_MAX, radius_param))
    return rp


def _cloud(vertices):
    table, _ = pack_clouds([vertices])
    if table.shape[0] < 4:
        raise ValueError("need at least 4 vertices, got %d (the reference's V = 3 case is not rebuilt)" % table.shape[0])
    if table.shape[0] > 2 ** 22:
        raise ValueError("at most 2^22 vertices")
    return table


def _poses(R, t):
    R = R.detach().cpu().numpy() if torch.is_tensor(R) else np.asarray(R)
    t = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    R = np.ascontiguousarray(R, dtype=np.float64)
    if R.ndim == 2:
        R = R[None]
    if R.ndim != 3 or R.shape[1:] != (3, 3) or R.shape[0] < 1:
        raise ValueError("R must be (n_views, 3, 3) with n_views >= 1, got %r" % (R.shape,))
    t = np.ascontiguousarray(t, dtype=np.float64)
    if t.shape in ((3, 1), (1, 3)):
        t = t.reshape(3)
    if t.shape != (3,) and t.shape != (R.shape[0], 3):
        raise ValueError("t must be (3,) or (n_views, 3), got %r" % (t.shape,))
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        raise ValueError("R or t holds NaN or infinite entries")
    return R, t


def _camera(v, R, t):
    """pc = R p + t by the kernel's order of operations -> (V,3)"""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([((R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z) + t[k] for k in range(3)], axis=1)


def _vertex_at_viewpoint(v, R, t):
    """the first view in which some vertex maps to (0, 0, 0), or None.  |R p| lies between the smallest and the largest singular
    value of R times |p|, so only views whose |t| falls in that band for some vertex are evaluated (none, for an object that does
    not reach the camera), and those exactly, with the kernel's own expression."""
    norms = np.sort(np.sqrt((v * v).sum(axis=1)))
    sv = np.linalg.svd(R, compute_uv=False)
    tn = np.linalg.norm(np.broadcast_to(t, (R.shape[0], 3)), axis=1)
    lo = tn / (sv[:, 0] * (1.0 + 1e-6) + 1e-300)
    with np.errstate(divide="ignore", invalid="ignore"):
        hi = np.where(sv[:, 2] > 0, tn / (sv[:, 2] * (1.0 - 1e-6)), np.inf)
    first = np.searchsorted(norms, lo * (1.0 - 1e-9), side="left")
    last = np.searchsorted(norms, hi * (1.0 + 1e-9), side="right")
    for k in np.nonzero(last > first)[0]:
        pc = _camera(v, R[k], t if t.ndim == 1 else t[k])
        if ((pc * pc).sum(axis=1) == 0).any():
            return int(k)
    return None


def hpr_visibility(vertices, R, t=(0, 0, 400.0), radius_param=2.0, device="cuda:0", return_mask=False, _workgroups=0):
    """Hidden-point-removal visibility of one cloud under n_views poses, one cp_hpr_visibility call.
    vertices (V,3) array / tensor, promoted to float64 (V >= 4, finite); R (n_views,3,3); t (3,) or (n_views,3): the camera-space
    cloud of view i is R_i p + t_i and the viewpoint is the origin.
    -> counts (V,) int32 on the device: the number of views in which each vertex is visible; with return_mask=True also
    mask (n_views,V) uint8.  ValueError for V < 4, non-finite input, n_views < 1, a radius_param outside [0, 8] and a vertex at the
    viewpoint, all before any launch; RuntimeError naming the first failing view and its status code when a view cannot be
    finished (all points coincident, for example: the reference raises QhullError there).  `_workgroups` (1 .. 65535) forces the
    number of workgroups that share the views (tests, measurement: the output does not depend on it)."""
    rp = _radius_param(radius_param)
    v = _cloud(vertices)
    R, t = _poses(R, t)
    wg = int(_workgroups)
    if not 0 <= wg <= 65535:
        raise ValueError("_workgroups must be in 0 .. 65535")
    hit = _vertex_at_viewpoint(v, R, t)
    if hit is not None:
        raise ValueError("a vertex lies at the viewpoint in view %d (norm 0: the flip is undefined)" % hit)
    dev = scene.cuda_device("prepare", device)
    n, V = R.shape[0], v.shape[0]
    nbytes = _abi.load().cp_hpr_visibility_scratch_bytes(n, V, wg)
    if nbytes == 0:
        raise ValueError("cp_hpr_visibility: bad shape (n_views = %d, V = %d, workgroups = %d)" % (n, V, wg))
    pts, Rd, td = torch.from_numpy(v).to(dev), torch.from_numpy(R).to(dev), torch.from_numpy(t).to(dev)
    counts = torch.empty(V, dtype=torch.int32, device=dev)
    mask = torch.empty((n, V), dtype=torch.uint8, device=dev) if return_mask else None
    status = torch.empty(n, dtype=torch.int32, device=dev)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _abi.call("cp_hpr_visibility", dev, pts, Rd, td, 0 if t.ndim == 1 else 3, n, V, rp, wg, counts, mask, status, scratch)
    codes = status.cpu().numpy()
    bad = np.nonzero(codes)[0]
    if bad.size:
        code = int(codes[bad[0]])
        raise RuntimeError("hpr_visibility: view %d failed with status %d (%s); %d of %d views failed"
                           % (int(bad[0]), code, STATUS.get(code, "unknown"), bad.size, n))
    return (counts, mask) if return_mask else counts


def compute_vis_hpr(points, viewpoint=None, radius_param=2.0, device="cuda:0"):
    """get_overall_visibility.py:20-42 on the device: points (n,3) in camera space, viewpoint None (the origin) or (3,)
    -> (n,) float64 numpy array of 0.0 / 1.0"""
    rp = _radius_param(radius_param)
    pts = _cloud(points)
    if viewpoint is not None:
        vp = np.asarray(viewpoint, dtype=np.float64).reshape(-1)
        if vp.shape != (3,) or not np.isfinite(vp).all():
            raise ValueError("viewpoint must be three finite coordinates")
        pts = pts - vp
    _, mask = hpr_visibility(pts, np.eye(3)[None], (0.0, 0.0, 0.0), rp, device, return_mask=True)
    return mask[0].cpu().numpy().astype(np.float64)


def overall_visibility(vertices, R=None, t=(0, 0, 400.0), min_n_views=2562, radius_param=2.0, device="cuda:0"):
    """The script's statistic (get_overall_visibility.py:99-122) -> {"mean": (V,) float64 = counts / n_views, "min", "max",
    "below": the nine ratios np.mean(mean < i * 0.1) for i = 1 .. 9 (strict <, the script's i * 0.1 thresholds), "n_views"}.
    R=None: the rotations of render.sample_views(min_n_views) -- an UNPINNED stand-in for the reference's unshipped
    sampled_poses_2562.pkl (see the module's docstring); the per-view rule is pinned."""
    if R is None:
        from .render import sample_views
        views, _ = sample_views(int(min_n_views))
        if not views:
            raise ValueError("min_n_views must give at least one view")
        R = np.stack([np.asarray(v["R"], dtype=np.float64).reshape(3, 3) for v in views])
    counts = hpr_visibility(vertices, R, t, radius_param, device)
    n_views = int(np.asarray(R).shape[0]) if np.asarray(R).ndim == 3 else 1
    mean = counts.cpu().numpy().astype(np.float64) / n_views
    below = np.array([np.mean(mean < i * 0.1) for i in range(1, 10)])
    return {"mean": mean, "min": float(mean.min()), "max": float(mean.max()), "below": below, "n_views": n_views}
