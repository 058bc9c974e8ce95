"""On-device pose scoring: the twin of the reference's metric.py and of the scoring block of its test
scripts (test.py:378-427, test_lm.py:300-321, compute_auc_posecnn test.py:37-57).

  pose_errors(...)                       batched ADD / ADD-S (ADI) on device tensors -- takes what solve_pnp_ransac returns
  Calculate_ADD_Error_BOP / _ADI_        the reference's names and numpy-in, float-out signatures (one pose; B = 1 of the above)
  MeshSet                                the packed vertex table of several objects, uploaded once, with their diameters
  compute_auc_posecnn, summarize         pass rates at 2 / 5 / 10 % of the diameter and the PoseCNN AUC (host: one float per image)

ADI is an all-pairs search: V^2 distance evaluations per pose and no spatial index.  Measured on one MI355X (tools/pose_error_bench.py,
profiles/pose_error_bench.json): one pose takes 0.16 / 0.36 / 1.44 ms at 4 096 / 20 480 / 61 440 vertices, 256 poses 0.60 / 11.6 / 101 ms
(about 9e12 pairs/s when the chip is full); beyond about 1e5 vertices subsample the mesh (the reference's own LM tables are 4 096
farthest-point samples per object).  There is no CPU fallback."""
import weakref

import numpy as np
import torch

from . import _abi

KINDS = {"add": _abi.POSE_ERR_ADD, "adi": _abi.POSE_ERR_ADI}


def calc_pts_diameter(pts):
    """largest pairwise distance of a point set (bop_toolkit_lib.misc.calc_pts_diameter restated): exact, in float64.
    Only points that can be an end of the longest pair are compared: with c the centroid and L a distance that IS attained,
    |p_i - p_j| <= |p_i - c| + max_k |p_k - c|, so a point whose bound falls below L is dropped before the all-pairs pass.
    The pass over the K points kept is K^2 (chunked: about 100 MB of temporaries whatever K); a sphere-like cloud keeps most of its
    points, so for real BOP meshes of 1e5+ vertices pass the `diameter` of models_info.json to MeshSet instead of computing it."""
    p = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    if p.shape[0] == 0:
        raise ValueError("calc_pts_diameter: empty point set")
    r = np.linalg.norm(p - p.mean(0), axis=1)
    a = p[int(r.argmax())]
    for _ in range(3):                                  # a few farthest-point hops: a lower bound that is an actual distance
        d = np.linalg.norm(p - a, axis=1)
        a, low = p[int(d.argmax())], float(d.max())
    keep = p[r + r.max() >= low * (1.0 - 1e-9)]
    best = 0.0
    rows = max(1, (1 << 21) // keep.shape[0])              # rows x K x 3 doubles per chunk: 48 MB, + the products
    for i0 in range(0, keep.shape[0], rows):
        d = keep[i0:i0 + rows, None, :] - keep[None, :, :]
        best = max(best, float((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).max()))
    return float(np.sqrt(best))


class MeshSet:
    """The vertices of M objects packed into one (sumV, 3) fp32 table + (M + 1) int32 offsets (cp_pose_errors' layout), and their
    diameters.  Built on the host; the device copies are made once per device on first use."""

    def __init__(self, verts, offsets, diameters):
        self.verts = verts                  # (sumV, 3) float32 CPU tensor
        self.offsets = offsets              # (M + 1,) int32 CPU tensor
        self.diameters = diameters          # (M,) float64 numpy
        self.sizes = np.diff(offsets.numpy()).astype(np.int64)
        self._dev = {}

    @classmethod
    def from_arrays(cls, arrays, diameters=None):
        """arrays: a list of (V_m, 3) arrays / tensors (or ONE such array); diameters: one per mesh, or None = computed as the
        reference does (largest pairwise distance of the vertices)"""
        if torch.is_tensor(arrays) or isinstance(arrays, np.ndarray):
            arrays = [arrays]
        host = []
        for a in arrays:
            a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
            if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] == 0:
                raise ValueError("every mesh must be a non-empty (V, 3) array, got %r" % (a.shape,))
            host.append(np.ascontiguousarray(a, dtype=np.float32))
        if not host:
            raise ValueError("MeshSet needs at least one mesh")
        off = np.zeros(len(host) + 1, dtype=np.int64)
        off[1:] = np.cumsum([a.shape[0] for a in host])
        if off[-1] >= 2 ** 31:
            raise ValueError("vertex table too large for int32 offsets")
        if diameters is None:
            diameters = [calc_pts_diameter(a) for a in host]
        diameters = np.asarray(diameters, dtype=np.float64).reshape(-1)
        if diameters.shape[0] != len(host):
            raise ValueError("need one diameter per mesh")
        return cls(torch.from_numpy(np.concatenate(host, 0)), torch.from_numpy(off.astype(np.int32)), diameters)

    def __len__(self):
        return int(self.offsets.numel()) - 1

    def on(self, device):
        """(verts, offsets) on `device`, uploaded on the first call"""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("checkerpose_amd.metric: CUDA/HIP tensors required (no CPU fallback)")
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._dev:
            self._dev[key] = (self.verts.to(device), self.offsets.to(device))
        return self._dev[key]


def _as_poses(R, t, B=None):
    """(B,3,3) + (B,3,1) / (B,3) float64 -> contiguous (B,12) [R row-major | t]"""
    if R.dim() == 2:
        R = R[None]
    B = R.shape[0] if B is None else B
    if tuple(R.shape) != (B, 3, 3) or t.numel() != 3 * B:
        raise ValueError("poses must be R (B,3,3) and t (B,3,1) / (B,3); got %r and %r" % (tuple(R.shape), tuple(t.shape)))
    return torch.cat([R.reshape(B, 9).to(torch.float64), t.reshape(B, 3).to(torch.float64)], 1).contiguous()


def pose_errors(R_est, t_est, R_gt, t_gt, vertices, mesh_ids=None, kinds=("add", "adi")):
    """ADD and / or ADD-S (ADI) of B poses against their ground truth, on the device (cp_pose_errors).
      R_est, t_est: (B,3,3) / (B,3,1) CUDA tensors, e.g. straight from solve_pnp_ransac; R_gt, t_gt: the same shapes (tensors on the
      same device, or host arrays, which are uploaded: 96 bytes per pose);
      vertices: one (V,3) array / tensor for every pose, a list of them, or a MeshSet; with several meshes `mesh_ids` (B,) names
      each pose's mesh;  kinds: any of "add", "adi".
    R_est is taken as ORTHONORMAL (the solver's poses and its identity fallback are): the kernel works in the model frame with the
    relative pose I + R_est^T (R_gt - R_est), which is the reference's rigid change of frame only then -- with a sheared or scaled
    estimate neither the reference's ADD nor R_est^T R_gt is what comes out.  A pose with a NaN / inf entry scores NaN in both errors.
    -> dict kind -> (B,) float64 CUDA tensor, in the vertices' units.  ADI costs V^2 per pose (module docstring)."""
    if not (torch.is_tensor(R_est) and torch.is_tensor(t_est) and R_est.is_cuda and t_est.is_cuda):
        raise RuntimeError("checkerpose_amd.metric: CUDA/HIP tensors required (no CPU fallback)")
    dev = R_est.device
    mask = 0
    for k in ([kinds] if isinstance(kinds, str) else kinds):
        if k not in KINDS:
            raise ValueError("kinds must be among %s, got %r" % (sorted(KINDS), k))
        mask |= KINDS[k]
    if not mask:
        raise ValueError("kinds is empty: ask for \"add\", \"adi\" or both")
    est = _as_poses(R_est, t_est)
    B = est.shape[0]
    if B == 0:
        raise ValueError("no poses")
    gt = _as_poses(torch.as_tensor(R_gt, dtype=torch.float64).to(dev), torch.as_tensor(t_gt, dtype=torch.float64).to(dev), B)
    ms = vertices if isinstance(vertices, MeshSet) else _cached_meshset(vertices)
    verts, offsets = ms.on(dev)
    M = len(ms)
    if mesh_ids is None:
        if M != 1:
            raise ValueError("several meshes need mesh_ids")
        ids, vmax = None, int(ms.sizes[0])
    elif torch.is_tensor(mesh_ids) and mesh_ids.is_cuda:      # stays on the device: an id outside 0..M-1 scores NaN (cp_pose_errors)
        if mesh_ids.numel() != B:
            raise ValueError("mesh_ids must be (B,)")
        ids, vmax = mesh_ids.reshape(-1).to(device=dev, dtype=torch.int32).contiguous(), int(ms.sizes.max())
    else:
        ids_host = np.asarray(mesh_ids).reshape(-1).astype(np.int64)
        if ids_host.shape[0] != B or ids_host.min() < 0 or ids_host.max() >= M:
            raise ValueError("mesh_ids must be (B,) with values in 0..%d" % (M - 1))
        ids, vmax = torch.from_numpy(ids_host.astype(np.int32)).to(dev), int(ms.sizes[np.unique(ids_host)].max())
    lib = _abi.load()
    out = {k: torch.empty(B, dtype=torch.float64, device=dev) for k, bit in KINDS.items() if mask & bit}
    scratch = None
    if mask & KINDS["adi"]:
        scratch = torch.empty(lib.cp_pose_errors_scratch_bytes(B, vmax), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _abi.check(lib.cp_pose_errors(st, est.data_ptr(), gt.data_ptr(), verts.data_ptr(), offsets.data_ptr(), M,
                                      None if ids is None else ids.data_ptr(), B, vmax, mask,
                                      out["add"].data_ptr() if "add" in out else None, out["adi"].data_ptr() if "adi" in out else None,
                                      None if scratch is None else scratch.data_ptr()), "cp_pose_errors")
    return out


_MESH_CACHE = {}        # id(array) -> (weak reference to the array, MeshSet): the upload of a mesh happens once per array


def _cached_meshset(vertices):
    """MeshSet of a bare (V,3) array / tensor or a list of them; cached per array OBJECT (test.py's loop passes the same `vertices`
    for every image), dropped when the array is collected.  The array is taken as constant: edit it in place and the cache is stale."""
    if isinstance(vertices, (list, tuple)):
        return MeshSet.from_arrays(list(vertices), diameters=np.full(len(vertices), np.nan))
    key = id(vertices)
    hit = _MESH_CACHE.get(key)
    if hit is not None and hit[0]() is vertices:
        return hit[1]
    ms = MeshSet.from_arrays([vertices], diameters=[np.nan])
    _MESH_CACHE[key] = (weakref.ref(vertices, lambda _r, k=key: _MESH_CACHE.pop(k, None)), ms)
    return ms


def _one_pose(kind, R_GT, t_GT, R_predict, t_predict, vertices, device):
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("checkerpose_amd.metric: a CUDA/HIP device is required (no CPU fallback)")
    f = lambda a, s: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(s))).to(dev)   # noqa: E731
    out = pose_errors(f(R_predict, (1, 3, 3)), f(t_predict, (1, 3, 1)), f(R_GT, (1, 3, 3)), f(t_GT, (1, 3, 1)), vertices, kinds=(kind,))
    return float(out[kind][0])


def Calculate_ADD_Error_BOP(R_GT, t_GT, R_predict, t_predict, vertices, device="cuda:0"):
    """the reference's metric.py:8-12 (numpy arrays of one pose -> float), scored on the device"""
    return _one_pose("add", R_GT, t_GT, R_predict, t_predict, vertices, device)


def Calculate_ADI_Error_BOP(R_GT, t_GT, R_predict, t_predict, vertices, device="cuda:0"):
    """the reference's metric.py:14-18 (numpy arrays of one pose -> float), scored on the device"""
    return _one_pose("adi", R_GT, t_GT, R_predict, t_predict, vertices, device)


def compute_auc_posecnn(errors):
    """Area under the accuracy-threshold curve up to 0.1 (errors in metres), as test.py:37-57 computes it after the YCB-Video
    toolbox: errors above 0.1 count as misses; nan when there is no error or none within 0.1."""
    d = np.sort(np.asarray(errors, dtype=np.float64).reshape(-1))
    n = d.shape[0]
    hit = d <= 0.1
    if n == 0 or not hit.any():
        return np.nan
    rec = d[hit]
    prec = (np.arange(1, n + 1, dtype=np.float64) / n)[hit]
    mrec = np.concatenate(([0.0], rec, [0.1]))
    mpre = np.maximum.accumulate(np.concatenate(([0.0], prec, [prec[-1]])))
    step = np.nonzero(mrec[1:] != mrec[:-1])[0] + 1
    return float(((mrec[step] - mrec[step - 1]) * mpre[step]).sum() * 10)


def _to_numpy(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _summary(err, diam):
    """err (n,), diam (n,): pass rates with the strict `<` of test.py:382-386 and the AUC of err / 1000 (test.py:480)"""
    err = np.where(np.isnan(err), 10000.0, err)             # test.py:379-380
    n = err.shape[0]
    out = {"count": int(n)}
    for pct, f in ((2, 0.02), (5, 0.05), (10, 0.1)):
        out["passed_%d" % pct] = float((err < f * diam).sum()) / n if n else float("nan")
    out["auc_posecnn"] = compute_auc_posecnn(err / 1000.0)
    return out


def summarize(errors, diameters, symmetric=None, mesh_ids=None):
    """The numbers test.py / test_lm.py print from the per-image errors (in mm).
      errors: the dict pose_errors() returns (or {"add": ..., "adi": ...} arrays); diameters: a float, one per pose, or -- with
      mesh_ids -- one per mesh (MeshSet.diameters); symmetric: bool or per-mesh bools: ADI is the main metric of a symmetric object
      and ADD the supplementary one, the other way round otherwise (test.py:127-136).
    -> {"passed_2", "passed_5", "passed_10", "auc_posecnn", "count"} of the main metric (+ "supp_*" of the other one when both
    errors are given); with mesh_ids also "per_mesh": {mesh id -> the same dict for that mesh's poses} (test_lm.py:319-321)."""
    err = {k: _to_numpy(v).astype(np.float64).reshape(-1) for k, v in errors.items()}
    if not err or set(err) - set(KINDS):
        raise ValueError("errors must hold \"add\" and / or \"adi\"")
    n = next(iter(err.values())).shape[0]
    ids = None if mesh_ids is None else _to_numpy(mesh_ids).astype(np.int64).reshape(-1)
    diam = np.asarray(diameters, dtype=np.float64).reshape(-1)
    sym = np.zeros(1, bool) if symmetric is None else np.asarray(symmetric, dtype=bool).reshape(-1)
    if ids is not None:
        diam = diam[ids] if diam.shape[0] != 1 else np.broadcast_to(diam, (n,))
        sym = sym[ids] if sym.shape[0] != 1 else np.broadcast_to(sym, (n,))
    else:
        diam, sym = np.broadcast_to(diam, (n,)), np.broadcast_to(sym, (n,))
    for k in ("adi" if sym.any() else None, "add" if (~sym).any() else None):
        if k is not None and k not in err:
            raise ValueError("the main metric of %s objects is %r: it is not among the errors given"
                             % ("symmetric" if k == "adi" else "non-symmetric", k))
    both = len(err) == 2

    def block(sel):
        main = np.where(sym[sel], err["adi"][sel] if "adi" in err else 0.0, err["add"][sel] if "add" in err else 0.0)
        out = _summary(main, diam[sel])
        if both:
            supp = np.where(sym[sel], err["add"][sel], err["adi"][sel])
            out.update({"supp_" + k: v for k, v in _summary(supp, diam[sel]).items() if k != "count"})
        return out

    res = block(np.ones(n, bool))
    if ids is not None:
        res["per_mesh"] = {int(m): block(ids == m) for m in np.unique(ids)}
    return res
