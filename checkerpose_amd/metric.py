"""On-device pose scoring: the twin of the reference's metric.py and of the scoring block of its test
scripts (test.py:378-427, test_lm.py:300-321, compute_auc_posecnn test.py:37-57).

  pose_errors(...)                       batched ADD / ADD-S (ADI) on device tensors -- takes what solve_pnp_ransac returns
  Calculate_ADD_Error_BOP / _ADI_        the reference's names and numpy-in, float-out signatures (one pose; B = 1 of the above)
  MeshSet                                the packed vertex table of several objects, uploaded once, with their diameters
  compute_auc_posecnn, summarize         pass rates at 2 / 5 / 10 % of the diameter and the PoseCNN AUC (host: one float per image)
  bop_errors, mssd / mspd / proj, SymmetrySet, bop_recall, summarize_bop      BOP's MSSD / MSPD / projection error (row N7): below
  vsd_errors, vsd, render_depth, vsd_from_depth                               BOP's VSD with its depth rasteriser (row N8): below
  mask_errors, mask_overlap, box_overlap, cus / cou_bb_proj / cou_mask / cou_bb   BOP's overlap errors (row N12): at the end

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

    def __init__(self, verts, offsets, diameters, faces=None, face_offsets=None, colors=None, normals=None):
        self.verts = verts                  # (sumV, 3) float32 CPU tensor
        self.offsets = offsets              # (M + 1,) int32 CPU tensor
        self.diameters = diameters          # (M,) float64 numpy
        self.sizes = np.diff(offsets.numpy()).astype(np.int64)
        self.faces = faces                  # (sumF, 3) int32 CPU tensor, vertex indices local to each mesh, or None (VSD needs them)
        self.face_offsets = face_offsets    # (M + 1,) int32 CPU tensor, or None
        self.colors = colors                # (sumV, 3) float32 CPU tensor in [0, 1], rows as verts, or None (render.render_rgb)
        self.normals = normals              # (sumV, 3) float32 CPU tensor, or None (phong shading needs them)
        self._dev = {}
        self._dev_faces = {}
        self._dev_shading = {}

    @classmethod
    def from_arrays(cls, arrays, diameters=None, faces=None, device=None, colors=None, normals=None):
        """arrays: a list of (V_m, 3) arrays / tensors (or ONE such array); diameters: one per mesh, or None = computed as the
        reference does (largest pairwise distance of the vertices) -- on the host, or with `device` on that device
        (prepare.pts_diameters: the same bits); faces: None, or one (F_m, 3) integer array of vertex indices
        per mesh (or ONE such array with one mesh) -- the triangles vsd_errors / render_depth rasterise;
        colors: None, or per mesh a (V_m, 3) uint8 / float array of vertex colours or None (that mesh is 0.5 grey) -- as
        renderer_py's add_object takes them: a mesh whose largest value is > 1 is divided by 255 (in float32);
        normals: None, or one (V_m, 3) float array per mesh (every mesh): render.render_rgb's phong shading.
        With both None the object is what it was before these arguments existed."""
        if torch.is_tensor(arrays) or isinstance(arrays, np.ndarray):
            arrays = [arrays]
            if faces is not None and (torch.is_tensor(faces) or isinstance(faces, np.ndarray)):
                faces = [faces]
            if colors is not None and (torch.is_tensor(colors) or isinstance(colors, np.ndarray)):
                colors = [colors]
            if normals is not None and (torch.is_tensor(normals) or isinstance(normals, np.ndarray)):
                normals = [normals]
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
        if diameters is None and device is not None:
            from .prepare import pts_diameters
            diameters = pts_diameters(host, device).cpu().numpy()
        elif diameters is None:
            diameters = [calc_pts_diameter(a) for a in host]
        diameters = np.asarray(diameters, dtype=np.float64).reshape(-1)
        if diameters.shape[0] != len(host):
            raise ValueError("need one diameter per mesh")
        ftab = foff = None
        if faces is not None:
            faces = list(faces)
            if len(faces) != len(host):
                raise ValueError("need one face array per mesh")
            fhost = []
            for f, a in zip(faces, host):
                f = f.detach().cpu().numpy() if torch.is_tensor(f) else np.asarray(f)
                if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
                    raise ValueError("faces must be (F, 3) integer arrays, got %r %s" % (f.shape, f.dtype))
                if f.shape[0] and (f.min() < 0 or f.max() >= a.shape[0]):
                    raise ValueError("a face names a vertex outside 0..%d" % (a.shape[0] - 1))
                fhost.append(np.ascontiguousarray(f, dtype=np.int32))
            fo = np.zeros(len(fhost) + 1, dtype=np.int64)
            fo[1:] = np.cumsum([f.shape[0] for f in fhost])
            if fo[-1] >= 2 ** 31 // 3:
                raise ValueError("face table too large for int32 offsets")
            ftab = torch.from_numpy(np.concatenate(fhost, 0).reshape(-1, 3)) if fo[-1] else torch.zeros((1, 3), dtype=torch.int32)
            foff = torch.from_numpy(fo.astype(np.int32))
        ctab = ntab = None
        if colors is not None:
            colors = list(colors)
            if len(colors) != len(host):
                raise ValueError("need one colour array (or None) per mesh")
            chost = []
            for c, a in zip(colors, host):
                if c is None:
                    chost.append(np.full(a.shape, 0.5, dtype=np.float32))
                    continue
                c = c.detach().cpu().numpy() if torch.is_tensor(c) else np.asarray(c)
                if c.shape != a.shape:
                    raise ValueError("colors must be (V, 3) like the vertices, got %r" % (c.shape,))
                c = np.array(c, dtype=np.float32)
                if not np.isfinite(c).all():
                    raise ValueError("colors must be finite")
                if c.max() > 1.0:
                    c /= np.float32(255.0)
                chost.append(c)
            ctab = torch.from_numpy(np.ascontiguousarray(np.concatenate(chost, 0)))
        if normals is not None:
            normals = list(normals)
            if len(normals) != len(host) or any(n is None for n in normals):
                raise ValueError("need one normal array per mesh")
            nhost = []
            for n, a in zip(normals, host):
                n = n.detach().cpu().numpy() if torch.is_tensor(n) else np.asarray(n)
                if n.shape != a.shape:
                    raise ValueError("normals must be (V, 3) like the vertices, got %r" % (n.shape,))
                nhost.append(np.ascontiguousarray(n, dtype=np.float32))
            ntab = torch.from_numpy(np.ascontiguousarray(np.concatenate(nhost, 0)))
        return cls(torch.from_numpy(np.concatenate(host, 0)), torch.from_numpy(off.astype(np.int32)), diameters, ftab, foff, ctab, ntab)

    def __len__(self):
        return int(self.offsets.numel()) - 1

    def _key(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("checkerpose_amd.metric: CUDA/HIP tensors required (no CPU fallback)")
        return (device.type, device.index if device.index is not None else torch.cuda.current_device())

    def on(self, device):
        """(verts, offsets) on `device`, uploaded on the first call"""
        key = self._key(device)
        if key not in self._dev:
            self._dev[key] = (self.verts.to(device), self.offsets.to(device))
        return self._dev[key]

    def faces_on(self, device):
        """(faces, face offsets, diameters) on `device`, uploaded on the first call; ValueError without a face table"""
        if self.faces is None:
            raise ValueError("this MeshSet has no faces: build it with MeshSet.from_arrays(..., faces=...) to render it")
        key = self._key(device)
        if key not in self._dev_faces:
            self._dev_faces[key] = (self.faces.to(device), self.face_offsets.to(device),
                                    torch.from_numpy(np.ascontiguousarray(self.diameters, dtype=np.float64)).to(device))
        return self._dev_faces[key]


    def shading_on(self, device):
        """(colors or None, normals or None) on `device`, uploaded on the first call"""
        key = self._key(device)
        if key not in self._dev_shading:
            self._dev_shading[key] = (None if self.colors is None else self.colors.to(device),
                                      None if self.normals is None else self.normals.to(device))
        return self._dev_shading[key]


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


# ---- BOP's MSSD / MSPD / projection error (cp_bop_errors) ---------------------------------------------------------
# The twin of the three renderer-free functions of bop_toolkit_lib/pose_error.py (mssd :96-118, mspd :121-144, proj :217-232), of
# misc.get_symmetry_transformations (:43-90) and of the recall eval_bop19_pose.py / eval_calc_scores.py compute from them.
#   bop_errors(...)                        batched, on device tensors -- takes what solve_pnp_ransac returns
#   mssd / mspd / proj                     bop_toolkit's names and numpy-in, float-out signatures (B = 1 of the above)
#   SymmetrySet                            the packed symmetry transformations of several objects, uploaded once
#   bop_recall, summarize_bop              recall per threshold and its mean (AR_MSSD / AR_MSPD); host: one float per pose
BOP_KINDS = {"mssd": _abi.BOP_ERR_MSSD, "mspd": _abi.BOP_ERR_MSPD, "proj": _abi.BOP_ERR_PROJ}
_BOP_MAPS = {None: 0, "small": _abi.BOP_MAP_SMALL, "large": _abi.BOP_MAP_LARGE}


def _rotation_about(angle, axis):
    """rotation by `angle` about `axis` through the origin (bop_toolkit_lib.transform.rotation_matrix restated, 3x3 part): the
    axis is normalised first; R = cos I + (1 - cos) a a^T + sin [a]_x, summed in that order"""
    import math
    sina, cosa = math.sin(angle), math.cos(angle)
    a = np.array(np.asarray(axis, dtype=np.float64).reshape(-1)[:3], dtype=np.float64, copy=True)
    a /= math.sqrt(np.dot(a, a))
    R = np.diag([cosa, cosa, cosa])
    R += np.outer(a, a) * (1.0 - cosa)
    a *= sina
    R += np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return R


def symmetry_transformations(model_info, max_sym_disc_step=0.01):
    """The symmetry set of one models_info.json entry as a list of {"R": (3,3), "t": (3,1)} (misc.get_symmetry_transformations
    restated).  Discrete symmetries: the identity plus every 4x4 of "symmetries_discrete".  Each continuous symmetry is sampled at
    count = ceil(pi / max_sym_disc_step) steps of 2 pi / count, i = 1 .. count - 1 -- so WITH a continuous symmetry the identity is
    not in the set, which then has (count - 1) * (1 + number of discrete symmetries) members per continuous axis: every
    discretised rotation composed with every discrete one."""
    disc = [{"R": np.eye(3), "t": np.zeros((3, 1))}]
    for sym in model_info.get("symmetries_discrete", ()):
        m = np.reshape(np.asarray(sym, dtype=np.float64), (4, 4))
        disc.append({"R": m[:3, :3], "t": m[:3, 3].reshape(3, 1)})
    cont = []
    for sym in model_info.get("symmetries_continuous", ()):
        offset = np.asarray(sym["offset"], dtype=np.float64).reshape(3, 1)
        count = int(np.ceil(np.pi / max_sym_disc_step))
        step = 2.0 * np.pi / count
        for i in range(1, count):
            R = _rotation_about(i * step, sym["axis"])
            cont.append({"R": R, "t": -R.dot(offset) + offset})
    if not cont:
        return disc
    return [{"R": c["R"].dot(d["R"]), "t": c["R"].dot(d["t"]) + c["t"]} for d in disc for c in cont]


class SymmetrySet:
    """The symmetry transformations of M objects packed into one (sumS, 12) fp64 table [R row-major | t] + (M + 1) int32 offsets
    (cp_bop_errors' layout), in MeshSet order.  Built on the host; the device copies are made once per device on first use."""

    def __init__(self, table, offsets):
        self.table = table                  # (sumS, 12) float64 CPU tensor
        self.offsets = offsets              # (M + 1,) int32 CPU tensor
        self.sizes = np.diff(offsets.numpy()).astype(np.int64)
        self._dev = {}

    @classmethod
    def from_transforms(cls, sets):
        """sets: one list of {"R": (3,3), "t": (3,) / (3,1)} per mesh (what bop_toolkit passes as `syms`)"""
        rows, off = [], [0]
        for syms in sets:
            if len(syms) == 0:
                raise ValueError("every mesh needs at least one symmetry transformation (the identity for an asymmetric object)")
            for s in syms:
                rows.append(np.concatenate([np.asarray(s["R"], dtype=np.float64).reshape(9), np.asarray(s["t"], dtype=np.float64).reshape(3)]))
            off.append(len(rows))
        if not rows:
            raise ValueError("SymmetrySet needs at least one mesh")
        return cls(torch.from_numpy(np.ascontiguousarray(np.stack(rows, 0))), torch.tensor(off, dtype=torch.int32))

    @classmethod
    def from_models_info(cls, infos, max_sym_disc_step=0.01):
        """infos: one models_info.json entry (dict) per mesh, in MeshSet order -> misc.get_symmetry_transformations of each"""
        if isinstance(infos, dict):
            raise ValueError("pass a LIST of models_info entries, one per mesh in MeshSet order")
        return cls.from_transforms([symmetry_transformations(i, max_sym_disc_step) for i in infos])

    @classmethod
    def identity(cls, M):
        return cls.from_transforms([[{"R": np.eye(3), "t": np.zeros(3)}]] * int(M))

    def transforms(self, m):
        """mesh m's set back as bop_toolkit's list of {"R", "t"}"""
        t = self.table.numpy()[int(self.offsets[m]):int(self.offsets[m + 1])]
        return [{"R": r[:9].reshape(3, 3).copy(), "t": r[9:].reshape(3, 1).copy()} for r in t]

    def __len__(self):
        return int(self.offsets.numel()) - 1

    def on(self, device):
        """(table, offsets) on `device`, uploaded on the first call"""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("checkerpose_amd.metric: CUDA/HIP tensors required (no CPU fallback)")
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._dev:
            self._dev[key] = (self.table.to(device), self.offsets.to(device))
        return self._dev[key]


_IDENTITY_SETS = {}     # M -> SymmetrySet of M identities (symmetries=None)


def bop_errors(R_est, t_est, R_gt, t_gt, cam_K, vertices, symmetries=None, mesh_ids=None, kinds=("mssd", "mspd", "proj"), _mapping=None):
    """BOP's MSSD, MSPD and / or projection error of B poses against their ground truth, on the device (cp_bop_errors).
      R_est, t_est: (B,3,3) / (B,3,1) CUDA tensors, e.g. straight from solve_pnp_ransac; R_gt, t_gt: the same shapes (tensors on the
      same device, or host arrays, which are uploaded);  cam_K: (3,3) for every pose or (B,3,3), tensor or array;
      vertices: one (V,3) array / tensor for every pose, a list of them, or a MeshSet; with several meshes `mesh_ids` (B,), on the
      host or on the device, names each pose's mesh;  symmetries: a SymmetrySet in the same mesh order, a list of bop_toolkit `syms`
      lists, or None = the identity alone for every mesh;  kinds: any of "mssd", "mspd", "proj".
    MSSD comes in the vertices' units, MSPD and proj in pixels of cam_K.  A pose with a NaN / inf entry (either pose, or K), or a
    device-side mesh id outside 0..M-1, scores NaN in every kind.  `_mapping` ("small" / "large") forces one of the kernel's two
    mappings (measurement and tests: results are bit-identical).
    -> dict kind -> (B,) float64 CUDA tensor."""
    if not (torch.is_tensor(R_est) and torch.is_tensor(t_est) and R_est.is_cuda and t_est.is_cuda):
        raise RuntimeError("checkerpose_amd.metric: CUDA/HIP tensors required (no CPU fallback)")
    dev = R_est.device
    mask = 0
    for k in ([kinds] if isinstance(kinds, str) else kinds):
        if k not in BOP_KINDS:
            raise ValueError("kinds must be among %s, got %r" % (sorted(BOP_KINDS), k))
        mask |= BOP_KINDS[k]
    if not mask:
        raise ValueError("kinds is empty: ask for \"mssd\", \"mspd\" and / or \"proj\"")
    if _mapping not in _BOP_MAPS:
        raise ValueError("_mapping must be None, \"small\" or \"large\"")
    est = _as_poses(R_est, t_est)
    B = est.shape[0]
    if B == 0:
        raise ValueError("no poses")
    gt = _as_poses(torch.as_tensor(R_gt, dtype=torch.float64).to(dev), torch.as_tensor(t_gt, dtype=torch.float64).to(dev), B)
    K = torch.as_tensor(cam_K).to(device=dev, dtype=torch.float64)
    if tuple(K.shape) == (3, 3):
        K, k_stride = K.reshape(9).contiguous(), 0
    elif tuple(K.shape) == (B, 3, 3):
        K, k_stride = K.reshape(B, 9).contiguous(), 9
    else:
        raise ValueError("cam_K must be (3,3) or (B,3,3), got %r" % (tuple(K.shape),))
    ms = vertices if isinstance(vertices, MeshSet) else _cached_meshset(vertices)
    M = len(ms)
    if symmetries is None:
        if M not in _IDENTITY_SETS:
            _IDENTITY_SETS[M] = SymmetrySet.identity(M)
        ss = _IDENTITY_SETS[M]
    else:
        ss = symmetries if isinstance(symmetries, SymmetrySet) else SymmetrySet.from_transforms(symmetries)
    if len(ss) != M:
        raise ValueError("%d symmetry sets for %d meshes" % (len(ss), M))
    verts, v_off = ms.on(dev)
    table, s_off = ss.on(dev)
    if mesh_ids is None:
        if M != 1:
            raise ValueError("several meshes need mesh_ids")
        ids, vmax, smax = None, int(ms.sizes[0]), int(ss.sizes[0])
    elif torch.is_tensor(mesh_ids) and mesh_ids.is_cuda:      # stays on the device: an id outside 0..M-1 scores NaN (cp_bop_errors)
        if mesh_ids.numel() != B:
            raise ValueError("mesh_ids must be (B,)")
        ids = mesh_ids.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        vmax, smax = int(ms.sizes.max()), int(ss.sizes.max())
    else:
        ids_host = np.asarray(mesh_ids).reshape(-1).astype(np.int64)
        if ids_host.shape[0] != B or ids_host.min() < 0 or ids_host.max() >= M:
            raise ValueError("mesh_ids must be (B,) with values in 0..%d" % (M - 1))
        used = np.unique(ids_host)
        ids, vmax, smax = torch.from_numpy(ids_host.astype(np.int32)).to(dev), int(ms.sizes[used].max()), int(ss.sizes[used].max())
    lib = _abi.load()
    out = {k: torch.empty(B, dtype=torch.float64, device=dev) for k, bit in BOP_KINDS.items() if mask & bit}
    scratch = torch.empty(lib.cp_bop_errors_map_scratch_bytes(B, smax, vmax, _BOP_MAPS[_mapping]), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ptr = lambda k: out[k].data_ptr() if k in out else None   # noqa: E731
    with torch.cuda.device(dev):
        _abi.check(lib.cp_bop_errors(st, est.data_ptr(), gt.data_ptr(), K.data_ptr(), k_stride, verts.data_ptr(), v_off.data_ptr(),
                                     table.data_ptr(), s_off.data_ptr(), M, None if ids is None else ids.data_ptr(), B, vmax, smax,
                                     mask | _BOP_MAPS[_mapping], ptr("mssd"), ptr("mspd"), ptr("proj"), scratch.data_ptr()),
                   "cp_bop_errors")
    return out


def _one_bop(kind, R_est, t_est, R_gt, t_gt, K, pts, syms, device):
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("checkerpose_amd.metric: a CUDA/HIP device is required (no CPU fallback)")
    f = lambda a, s: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(s))).to(dev)   # noqa: E731
    out = bop_errors(f(R_est, (1, 3, 3)), f(t_est, (1, 3, 1)), f(R_gt, (1, 3, 3)), f(t_gt, (1, 3, 1)),
                     np.eye(3) if K is None else np.asarray(K, dtype=np.float64).reshape(3, 3), pts,
                     symmetries=None if syms is None else [list(syms)], kinds=(kind,))
    return float(out[kind][0])


def mssd(R_est, t_est, R_gt, t_gt, pts, syms, device="cuda:0"):
    """bop_toolkit_lib.pose_error.mssd (numpy arrays of one pose -> float), scored on the device"""
    return _one_bop("mssd", R_est, t_est, R_gt, t_gt, None, pts, syms, device)


def mspd(R_est, t_est, R_gt, t_gt, K, pts, syms, device="cuda:0"):
    """bop_toolkit_lib.pose_error.mspd (numpy arrays of one pose -> float), scored on the device"""
    return _one_bop("mspd", R_est, t_est, R_gt, t_gt, K, pts, syms, device)


def proj(R_est, t_est, R_gt, t_gt, K, pts, device="cuda:0"):
    """bop_toolkit_lib.pose_error.proj (numpy arrays of one pose -> float), scored on the device"""
    return _one_bop("proj", R_est, t_est, R_gt, t_gt, K, pts, None, device)


def bop_thresholds(kind):
    """eval_bop19_pose.py:46,51: the ten thresholds of correctness of MSSD (fractions of the diameter) and MSPD (pixels at width 640)"""
    if kind == "mssd":
        return np.arange(0.05, 0.51, 0.05)
    if kind == "mspd":
        return np.arange(5, 51, 5)
    if kind == "vsd":                                      # eval_bop19_pose.py:31,34: vsd_taus and its correct_th are the same ten values
        return np.arange(0.05, 0.51, 0.05)
    if kind == "cus":                                      # eval_calc_scores.py:43
        return np.array([0.5])
    raise ValueError("%r has no default thresholds (BOP'19 scores \"mssd\" and \"mspd\"): pass `thresholds`" % (kind,))


def bop_recall(errors, kind, diameters=None, im_width=None, thresholds=None, mesh_ids=None):
    """Recall of one error kind over its thresholds, with ONE estimate per target as test.py produces (then BOP's greedy matching is
    the comparison alone): eval_calc_scores.py:246-263 + pose_matching.py:68.
      errors: (n,) tensor / array of `kind` ("mssd", "mspd", "proj" or "cus");  MSSD is divided by the diameter (`diameters`: a float,
      one per pose, or -- with mesh_ids -- one per mesh), MSPD is multiplied by 640 / im_width, proj and cus are taken as they are;  thresholds:
      default bop_thresholds(kind).  A pose is correct when error < threshold, STRICT; NaN is a miss.
    -> {"thresholds", "correct": (n, T) bool, "recall": (T,), "AR_<KIND>": their mean, "count"} and, with mesh_ids,
       "per_mesh": {mesh id -> {"recall", "AR_<KIND>", "count"}}.
    Several estimates or instances per target, or a targets file: checkerpose_amd.bop_eval does the matching (row N11)."""
    if kind == "vsd":
        return _vsd_recall(errors, thresholds, mesh_ids)
    if kind not in BOP_KINDS and kind != "cus":
        raise ValueError("kind must be among %s, got %r" % (sorted(BOP_KINDS) + ["cus", "vsd"], kind))
    e = _to_numpy(errors).astype(np.float64).reshape(-1)
    n = e.shape[0]
    ids = None if mesh_ids is None else _to_numpy(mesh_ids).astype(np.int64).reshape(-1)
    if kind == "mssd":
        if diameters is None:
            raise ValueError("MSSD is scored relative to the object diameter: pass `diameters`")
        diam = np.asarray(diameters, dtype=np.float64).reshape(-1)
        diam = diam[ids] if (ids is not None and diam.shape[0] != 1) else np.broadcast_to(diam, (n,))
        e = e / diam
    elif kind == "mspd":
        if im_width is None:
            raise ValueError("MSPD is scored at an image width of 640: pass `im_width`")
        e = (640.0 / float(im_width)) * e
    th = bop_thresholds(kind) if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    correct = e[:, None] < th[None, :]
    name = "AR_" + kind.upper()

    def block(sel):
        c = correct[sel]
        rec = c.mean(0) if c.shape[0] else np.full(th.shape[0], np.nan)
        return {"recall": rec, name: float(rec.mean()), "count": int(c.shape[0])}

    res = block(np.ones(n, bool))
    res.update({"thresholds": th, "correct": correct})
    if ids is not None:
        res["per_mesh"] = {int(m): block(ids == m) for m in np.unique(ids)}
    return res


def _vsd_recall(errors, thresholds, mesh_ids):
    """bop_recall(.., "vsd"): errors (n, T), one column per tau (vsd_errors' "vsd"); a pose is correct for the pair (tau, threshold)
    when its error at that tau < threshold, STRICT; NaN is a miss (eval_calc_scores.py:246-263 run once per tau).
    -> {"thresholds", "correct": (n, T, Th) bool, "recall": (T, Th), "AR_VSD": their mean over all pairs, "count"} (+ "per_mesh")"""
    e = _to_numpy(errors).astype(np.float64)
    if e.ndim != 2:
        raise ValueError("VSD errors must be (n, T), one column per tau; got %r" % (e.shape,))
    th = bop_thresholds("vsd") if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    correct = e[:, :, None] < th[None, None, :]
    ids = None if mesh_ids is None else _to_numpy(mesh_ids).astype(np.int64).reshape(-1)

    def block(sel):
        c = correct[sel]
        rec = c.mean(0) if c.shape[0] else np.full(correct.shape[1:], np.nan)
        return {"recall": rec, "AR_VSD": float(rec.mean()), "count": int(c.shape[0])}

    res = block(np.ones(e.shape[0], bool))
    res.update({"thresholds": th, "correct": correct})
    if ids is not None:
        res["per_mesh"] = {int(m): block(ids == m) for m in np.unique(ids)}
    return res


def summarize_bop(errors, diameters=None, im_width=None, mesh_ids=None, thresholds=None):
    """bop_recall of every kind in `errors` (the dict bop_errors returns; other keys, e.g. "add", are ignored; "proj" only when
    `thresholds` names it).  thresholds: optional dict kind -> thresholds.
    -> {kind: bop_recall's dict} plus "AR_MSSD" / "AR_MSPD" at the top.  With "vsd" in `errors` (vsd_errors' (n, T) array) also
    "vsd" / "AR_VSD", and -- when all three are there -- "AR" = mean(AR_VSD, AR_MSSD, AR_MSPD) (eval_bop19_pose.py:243).
    One estimate per target is assumed; checkerpose_amd.bop_eval.evaluate_results matches several to several (row N11)."""
    thresholds = thresholds or {}
    res = {}
    for kind in BOP_KINDS:
        if kind not in errors or (kind == "proj" and "proj" not in thresholds):
            continue
        res[kind] = bop_recall(errors[kind], kind, diameters=diameters, im_width=im_width, thresholds=thresholds.get(kind), mesh_ids=mesh_ids)
        res["AR_" + kind.upper()] = res[kind]["AR_" + kind.upper()]
    if "vsd" in errors:
        res["vsd"] = bop_recall(errors["vsd"], "vsd", thresholds=thresholds.get("vsd"), mesh_ids=mesh_ids)
        res["AR_VSD"] = res["vsd"]["AR_VSD"]
        if "AR_MSSD" in res and "AR_MSPD" in res:
            res["AR"] = float(np.mean([res["AR_VSD"], res["AR_MSSD"], res["AR_MSPD"]]))
    if not res:
        raise ValueError("errors holds none of \"mssd\", \"mspd\", \"vsd\" (or \"proj\" with thresholds)")
    return res


def score_poses(R_est, t_est, R_gt, t_gt, cam_K, vertices, mesh_ids=None, kinds=("add", "adi"), symmetries=None, depth_test=None,
                image_ids=None, size=None, **vsd_kwargs):
    """pose_errors, bop_errors, vsd_errors and / or mask_errors by the kinds asked (postprocess.evaluate_poses, targets.evaluate_batch):
    kinds of "add" / "adi" alone are exactly pose_errors -- nothing else is launched.  "vsd" needs `depth_test` (and a MeshSet with
    faces); vsd_kwargs (delta, taus, normalized_by_diameter, sphere_check) go to vsd_errors; its (B, T) errors come back under "vsd".
    "cus" / "cou_bb_proj" need `size` = (W, H) (and a MeshSet with faces): mask_errors, without the sphere shortcut."""
    names = [kinds] if isinstance(kinds, str) else list(kinds)
    want_vsd = "vsd" in names
    masks = [k for k in names if k in MASK_KINDS]
    names = [k for k in names if k != "vsd" and k not in MASK_KINDS]
    if want_vsd and depth_test is None:
        raise ValueError("kind \"vsd\" needs depth_test")
    if masks and size is None:
        raise ValueError("kinds \"cus\" / \"cou_bb_proj\" need size=(W, H)")
    bop = [k for k in names if k in BOP_KINDS]
    if not bop and not want_vsd and not masks:
        return pose_errors(R_est, t_est, R_gt, t_gt, vertices, mesh_ids=mesh_ids, kinds=kinds)
    rest = [k for k in names if k not in BOP_KINDS]
    out = pose_errors(R_est, t_est, R_gt, t_gt, vertices, mesh_ids=mesh_ids, kinds=rest) if rest else {}
    if bop:
        out.update(bop_errors(R_est, t_est, R_gt, t_gt, cam_K, vertices, symmetries=symmetries, mesh_ids=mesh_ids, kinds=bop))
    if want_vsd:
        out["vsd"] = vsd_errors(R_est, t_est, R_gt, t_gt, cam_K, vertices, depth_test, image_ids=image_ids, mesh_ids=mesh_ids,
                                **vsd_kwargs)["vsd"]
    if masks:
        out.update(mask_errors(R_est, t_est, R_gt, t_gt, cam_K, vertices, size, mesh_ids=mesh_ids, kinds=masks))
    return out


# ---- BOP's VSD (cp_vsd_errors) ------------------------------------------------------------------------------------
# The twin of bop_toolkit_lib/pose_error.py:17-93 (vsd) with the renderer it asks for: a depth rasteriser in HIP fused with the
# reference's pixel counting.  The reference's own renderers (vispy / OpenGL / the C++ bop_renderer) do not run here.
#   vsd_errors(...)                        batched, on device tensors -- takes what solve_pnp_ransac returns, and depth images
#   vsd                                    bop_toolkit's name and signature (one pose; `renderer` is a MeshSet with faces)
#   render_depth                           the rasteriser alone
#   bop_recall(.., "vsd"), summarize_bop   recall per (tau, threshold) pair, AR_VSD and BOP'19's AR
def _vsd_common(R, t, cam_K, meshes, mesh_ids):
    if not (torch.is_tensor(R) and torch.is_tensor(t) and R.is_cuda and t.is_cuda):
        raise RuntimeError("checkerpose_amd.metric: CUDA/HIP tensors required (no CPU fallback)")
    if not isinstance(meshes, MeshSet):
        raise ValueError("VSD renders triangles: pass a MeshSet built with faces")
    if meshes.faces is None:
        raise ValueError("this MeshSet has no faces: build it with MeshSet.from_arrays(..., faces=...) to render it")
    dev = R.device
    poses = _as_poses(R, t)
    B = poses.shape[0]
    if B == 0:
        raise ValueError("no poses")
    K = torch.as_tensor(cam_K).to(device=dev, dtype=torch.float64)
    if tuple(K.shape) == (3, 3):
        K, k_stride = K.reshape(9).contiguous(), 0
    elif tuple(K.shape) == (B, 3, 3):
        K, k_stride = K.reshape(B, 9).contiguous(), 9
    else:
        raise ValueError("cam_K must be (3,3) or (B,3,3), got %r" % (tuple(K.shape),))
    M = len(meshes)
    if mesh_ids is None:
        if M != 1:
            raise ValueError("several meshes need mesh_ids")
        ids, vmax = None, int(meshes.sizes[0])
    elif torch.is_tensor(mesh_ids) and mesh_ids.is_cuda:
        if mesh_ids.numel() != B:
            raise ValueError("mesh_ids must be (B,)")
        ids, vmax = mesh_ids.reshape(-1).to(device=dev, dtype=torch.int32).contiguous(), int(meshes.sizes.max())
    else:
        ids_host = np.asarray(mesh_ids).reshape(-1).astype(np.int64)
        if ids_host.shape[0] != B or ids_host.min() < 0 or ids_host.max() >= M:
            raise ValueError("mesh_ids must be (B,) with values in 0..%d" % (M - 1))
        ids, vmax = torch.from_numpy(ids_host.astype(np.int32)).to(dev), int(meshes.sizes[np.unique(ids_host)].max())
    return dev, poses, B, K, k_stride, M, ids, vmax


def _vsd_images(depth_test, image_ids, B, dev):
    d = torch.as_tensor(depth_test)
    if d.dim() == 2:
        d = d[None]
    if d.dim() != 3:
        raise ValueError("depth_test must be (H,W) or (I,H,W), got %r" % (tuple(d.shape),))
    d = d.to(device=dev, dtype=torch.float32).contiguous()
    n_img = int(d.shape[0])
    if image_ids is None:
        if n_img == 1:
            img = None
        elif n_img == B:
            img = torch.arange(B, dtype=torch.int32, device=dev)
        else:
            raise ValueError("%d depth images for %d poses need image_ids" % (n_img, B))
    elif torch.is_tensor(image_ids) and image_ids.is_cuda:        # stays on the device: an id outside 0..I-1 scores NaN
        if image_ids.numel() != B:
            raise ValueError("image_ids must be (B,)")
        img = image_ids.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    else:
        host = np.asarray(image_ids).reshape(-1).astype(np.int64)
        if host.shape[0] != B or host.min() < 0 or host.max() >= n_img:
            raise ValueError("image_ids must be (B,) with values in 0..%d" % (n_img - 1))
        img = torch.from_numpy(host.astype(np.int32)).to(dev)
    return d, img, n_img


def _vsd_taus(taus):
    import ctypes as C
    tv = bop_thresholds("vsd") if taus is None else np.asarray(taus, dtype=np.float64).reshape(-1)
    if not 1 <= tv.shape[0] <= 16 or not np.isfinite(tv).all():
        raise ValueError("taus: 1 to 16 finite values")
    return tv, (C.c_double * tv.shape[0])(*tv.tolist())


def vsd_errors(R_est, t_est, R_gt, t_gt, cam_K, meshes, depth_test, image_ids=None, delta=15.0, taus=None, normalized_by_diameter=True,
               mesh_ids=None, sphere_check=True, return_counts=False, return_depth=False):
    """BOP's VSD of B poses against their ground truth, rendered and counted on the device (cp_vsd_errors).
      R_est, t_est: (B,3,3) / (B,3,1) CUDA tensors; R_gt, t_gt: the same shapes (tensors or host arrays); cam_K: (3,3) or (B,3,3);
      meshes: a MeshSet built with faces (with several meshes, mesh_ids (B,) names each pose's);  depth_test: (H,W) or (I,H,W) depth
      images in the vertices' units (mm; 0 = no measurement), image_ids (B,) names each pose's image (default: the one image, or
      image b for pose b when I == B);  delta: the visibility tolerance (15 mm for lm / lmo / ycbv);  taus: default
      bop_thresholds("vsd");  sphere_check: the shortcut of bop_toolkit's caller (eval_calc_errors.py:299-318) -- a pose whose
      sphere projection does not overlap the ground truth's is not rendered and scores 1.0 at every tau.
    A pose with a NaN / inf entry, a device-side mesh / image id out of range, or any vertex at Z <= 0 scores NaN (a miss).
    -> {"vsd": (B,T) float64 CUDA tensor} (+ "counts": (B,T+2) int32 = union, inter, cost count per tau; + "depth": (B,2,H,W)
    float32 = the estimate's and the ground truth's render).  The counts are the same bits with or without the depth output."""
    dev, est, B, K, k_stride, M, ids, vmax = _vsd_common(R_est, t_est, cam_K, meshes, mesh_ids)
    gt = _as_poses(torch.as_tensor(R_gt, dtype=torch.float64).to(dev), torch.as_tensor(t_gt, dtype=torch.float64).to(dev), B)
    d, img, n_img = _vsd_images(depth_test, image_ids, B, dev)
    H, W = int(d.shape[1]), int(d.shape[2])
    tv, ctaus = _vsd_taus(taus)
    T = tv.shape[0]
    verts, v_off = meshes.on(dev)
    faces, f_off, diam = meshes.faces_on(dev)
    lib = _abi.load()
    err = torch.empty((B, T), dtype=torch.float64, device=dev)
    counts = torch.empty((B, T + 2), dtype=torch.int32, device=dev)
    depth = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev) if return_depth else None
    scratch = torch.empty(lib.cp_vsd_errors_scratch_bytes(B, vmax, H, W), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _abi.check(lib.cp_vsd_errors(st, est.data_ptr(), gt.data_ptr(), K.data_ptr(), k_stride, verts.data_ptr(), v_off.data_ptr(),
                                     faces.data_ptr(), f_off.data_ptr(), M, None if ids is None else ids.data_ptr(), d.data_ptr(),
                                     None if img is None else img.data_ptr(), n_img, H, W, float(delta), diam.data_ptr(), ctaus, T,
                                     1 if normalized_by_diameter else 0, 1 if sphere_check else 0, B, vmax, err.data_ptr(),
                                     counts.data_ptr(), None if depth is None else depth.data_ptr(), scratch.data_ptr()),
                   "cp_vsd_errors")
    out = {"vsd": err}
    if return_counts:
        out["counts"] = counts
    if return_depth:
        out["depth"] = depth
    return out


def vsd_from_depth(depth_est, depth_gt, depth_test, cam_K, diameters, image_ids=None, delta=15.0, taus=None, normalized_by_diameter=True):
    """vsd_errors' counting on caller-supplied renders (cp_vsd_from_depth): depth_est, depth_gt (B,H,W) float32 CUDA tensors;
    diameters: a float or one per pose.  -> {"vsd": (B,T) f64, "counts": (B,T+2) int32}"""
    if not (torch.is_tensor(depth_est) and torch.is_tensor(depth_gt) and depth_est.is_cuda and depth_gt.is_cuda):
        raise RuntimeError("checkerpose_amd.metric: CUDA/HIP tensors required (no CPU fallback)")
    if depth_est.dim() != 3 or depth_est.shape != depth_gt.shape:
        raise ValueError("depth_est and depth_gt must both be (B,H,W)")
    dev = depth_est.device
    de = depth_est.to(torch.float32).contiguous()
    dg = depth_gt.to(device=dev, dtype=torch.float32).contiguous()
    B, H, W = (int(v) for v in de.shape)
    if B == 0:
        raise ValueError("no poses")
    d, img, n_img = _vsd_images(depth_test, image_ids, B, dev)
    if tuple(d.shape[1:]) != (H, W):
        raise ValueError("depth_test is %r, the renders are %r" % (tuple(d.shape[1:]), (H, W)))
    K = torch.as_tensor(cam_K).to(device=dev, dtype=torch.float64)
    if tuple(K.shape) == (3, 3):
        K, k_stride = K.reshape(9).contiguous(), 0
    elif tuple(K.shape) == (B, 3, 3):
        K, k_stride = K.reshape(B, 9).contiguous(), 9
    else:
        raise ValueError("cam_K must be (3,3) or (B,3,3), got %r" % (tuple(K.shape),))
    diam = np.asarray(diameters, dtype=np.float64).reshape(-1)
    if diam.shape[0] not in (1, B):
        raise ValueError("diameters: a float or one per pose")
    diam = torch.from_numpy(np.array(np.broadcast_to(diam, (B,)), dtype=np.float64)).to(dev)
    tv, ctaus = _vsd_taus(taus)
    T = tv.shape[0]
    lib = _abi.load()
    err = torch.empty((B, T), dtype=torch.float64, device=dev)
    counts = torch.empty((B, T + 2), dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.cp_vsd_errors_scratch_bytes(B, 0, H, W), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _abi.check(lib.cp_vsd_from_depth(st, de.data_ptr(), dg.data_ptr(), K.data_ptr(), k_stride, d.data_ptr(),
                                         None if img is None else img.data_ptr(), n_img, H, W, float(delta), diam.data_ptr(), ctaus, T,
                                         1 if normalized_by_diameter else 0, B, err.data_ptr(), counts.data_ptr(), scratch.data_ptr()),
                   "cp_vsd_from_depth")
    return {"vsd": err, "counts": counts}


def render_depth(R, t, cam_K, meshes, size, mesh_ids=None):
    """Depth images of B poses of `meshes` (a MeshSet with faces), rendered on the device (cp_render_depth): depth[b, y, x] is the
    eye-space Z of the front-most surface on the ray through image point (x + 0.5, y + 0.5), 0 where there is none -- what
    bop_toolkit's renderer.render_object(...)['depth'] holds.  size: (width, height), as bop_toolkit's renderers take it.
    A pose with a non-finite entry or any vertex at Z <= 0 renders nothing (zeros).  -> (B,H,W) float32 CUDA tensor"""
    dev, poses, B, K, k_stride, M, ids, vmax = _vsd_common(R, t, cam_K, meshes, mesh_ids)
    W, H = int(size[0]), int(size[1])
    if W <= 0 or H <= 0:
        raise ValueError("size must be (width, height), both positive")
    verts, v_off = meshes.on(dev)
    faces, f_off, _ = meshes.faces_on(dev)
    lib = _abi.load()
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.cp_vsd_errors_scratch_bytes(B, vmax, H, W), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _abi.check(lib.cp_render_depth(st, poses.data_ptr(), K.data_ptr(), k_stride, verts.data_ptr(), v_off.data_ptr(), faces.data_ptr(),
                                       f_off.data_ptr(), M, None if ids is None else ids.data_ptr(), H, W, B, vmax, depth.data_ptr(),
                                       scratch.data_ptr()), "cp_render_depth")
    return depth


def vsd(R_est, t_est, R_gt, t_gt, depth_test, K, delta, taus, normalized_by_diameter, diameter, renderer, obj_id, cost_type="step",
        device="cuda:0"):
    """bop_toolkit_lib.pose_error.vsd (numpy arrays of one pose -> list of floats, one per tau), rendered and scored on the device.
    `renderer` is a MeshSet with faces and `obj_id` the index of the object's mesh in it; `diameter` is the one the distances are
    normalised by (it replaces the MeshSet's for this call).  Only the 'step' cost exists.  No sphere shortcut: that is the caller's."""
    if cost_type != "step":
        raise ValueError("only the 'step' pixel-wise matching cost is implemented")
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("checkerpose_amd.metric: a CUDA/HIP device is required (no CPU fallback)")
    if not isinstance(renderer, MeshSet) or renderer.faces is None:
        raise ValueError("renderer must be a MeshSet built with faces")
    m = int(obj_id)
    if not 0 <= m < len(renderer):
        raise ValueError("obj_id must be a mesh index in 0..%d" % (len(renderer) - 1))
    v0, v1 = int(renderer.offsets[m]), int(renderer.offsets[m + 1])
    f0, f1 = int(renderer.face_offsets[m]), int(renderer.face_offsets[m + 1])
    one = MeshSet.from_arrays([renderer.verts[v0:v1]], diameters=[float(diameter)], faces=[renderer.faces[f0:f1]])
    f = lambda a, s: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(s))).to(dev)   # noqa: E731
    out = vsd_errors(f(R_est, (1, 3, 3)), f(t_est, (1, 3, 1)), f(R_gt, (1, 3, 3)), f(t_gt, (1, 3, 1)),
                     np.asarray(K, dtype=np.float64).reshape(3, 3), one, np.asarray(depth_test, dtype=np.float32), delta=delta, taus=taus,
                     normalized_by_diameter=normalized_by_diameter, sphere_check=False)
    return [float(v) for v in out["vsd"][0].cpu()]


# ---- BOP's overlap errors (cp_mask_errors / cp_mask_overlap / cp_box_overlap) ------------------------------------
# The twin of the last four functions of bop_toolkit_lib/pose_error.py: cou_mask :235-253, cus :256-286, cou_bb :289-297, cou_bb_proj
# :300-330 (with misc.calc_2d_bbox / misc.iou).  With them every error of that file runs on the device.
#   mask_errors(...)                       batched cus / cou_bb_proj: both silhouettes rasterised per tile, nothing stored unless asked
#   mask_overlap(...)                      the counting half on caller-supplied masks: cou_mask, and cou_bb of the masks' boxes
#   box_overlap(...)                       1 - iou of box pairs
#   cou_mask, cou_bb, cus, cou_bb_proj     bop_toolkit's names and argument order (one pair)
MASK_KINDS = ("cus", "cou_bb_proj")
OVERLAP_KINDS = ("cou_mask", "cou_bb")


def mask_errors(R_est, t_est, R_gt, t_gt, cam_K, meshes, size, mesh_ids=None, kinds=("cus", "cou_bb_proj"), sphere_check=False,
                return_counts=False, return_boxes=False, return_masks=False):
    """BOP's 'cus' (complement over union of the projected silhouettes) and / or 'cou_bb_proj' (of their bounding boxes) of B poses
    against their ground truth, rendered and counted on the device (cp_mask_errors).
      R_est, t_est: (B,3,3) / (B,3,1) CUDA tensors, e.g. straight from solve_pnp_ransac; R_gt, t_gt: the same shapes (tensors or host
      arrays); cam_K: (3,3) or (B,3,3); meshes: a MeshSet built with faces (with several meshes, mesh_ids (B,) names each pair's);
      size: (width, height) of the frame, as bop_toolkit's renderers take it;  kinds: any of "cus", "cou_bb_proj";
      sphere_check: the shortcut of bop_toolkit's caller (eval_calc_errors.py:299-302,357-362), which belongs to 'cus' ALONE -- a pair
      whose sphere projections do not overlap scores cus = 1.0 unrendered; cou_bb_proj is computed whatever the check says.
    A silhouette pixel is set exactly where render_depth(..., size) > 0.  cus = 1 - inter / union, 1.0 when the union is empty.
    cou_bb_proj = 1 - iou of the boxes (xmin, ymin, xmax - xmin, ymax - ymin): no + 1, not clipped; where a side's silhouette is
    EMPTY (e.g. wholly outside the frame) the reference raises (xs.min() of nothing) -- here cou_bb_proj is NaN, a miss under the
    strict `<` of the matching.  A pair with a NaN / inf entry, a device-side mesh id out of range, or any vertex at Z <= 0 on
    either side scores NaN in both kinds.
    -> dict kind -> (B,) float64 CUDA tensor; + "counts": (B,4) int32 = inter, union, n_est, n_gt and "ok": (B,) bool
    (return_counts); + "boxes": (B,2,4) int32 = the estimate's and the ground truth's x, y, w, h, -1 where empty (return_boxes);
    + "masks": (B,2,H,W) bool (return_masks).  A sphere-skipped pair that is not rendered (no "cou_bb_proj" among the kinds) has
    counts 0, boxes -1 and empty masks.  The errors are the same bits with or without the optional outputs.
    return_masks forfeits the early leave: every tile of every pair then walks its pixels to store them (zeros where nothing is
    rendered), which is the stored-image cost the fused call otherwise avoids -- ask for masks only when they are wanted."""
    names = [kinds] if isinstance(kinds, str) else list(kinds)
    for k in names:
        if k not in MASK_KINDS:
            raise ValueError("kinds must be among %s, got %r" % (list(MASK_KINDS), k))
    if not names:
        raise ValueError("kinds is empty: ask for \"cus\", \"cou_bb_proj\" or both")
    dev, est, B, K, k_stride, M, ids, vmax = _vsd_common(R_est, t_est, cam_K, meshes, mesh_ids)
    gt = _as_poses(torch.as_tensor(R_gt, dtype=torch.float64).to(dev), torch.as_tensor(t_gt, dtype=torch.float64).to(dev), B)
    if size is None:
        raise ValueError("size=(width, height) is required: a MeshSet has no frame")
    W, H = int(size[0]), int(size[1])
    if W <= 0 or H <= 0:
        raise ValueError("size must be (width, height), both positive")
    verts, v_off = meshes.on(dev)
    faces, f_off, diam = meshes.faces_on(dev)
    lib = _abi.load()
    out = {k: torch.empty(B, dtype=torch.float64, device=dev) for k in MASK_KINDS if k in names}
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev) if return_counts else None
    ok = torch.empty(B, dtype=torch.uint8, device=dev) if return_counts else None
    boxes = torch.empty((B, 2, 4), dtype=torch.int32, device=dev) if return_boxes else None
    masks = torch.empty((B, 2, H, W), dtype=torch.uint8, device=dev) if return_masks else None
    scratch = torch.empty(lib.cp_mask_errors_scratch_bytes(B, vmax), dtype=torch.uint8, device=dev)
    ptr = lambda x: None if x is None else x.data_ptr()     # noqa: E731
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _abi.check(lib.cp_mask_errors(st, est.data_ptr(), gt.data_ptr(), K.data_ptr(), k_stride, verts.data_ptr(), v_off.data_ptr(),
                                      faces.data_ptr(), f_off.data_ptr(), M, ptr(ids), diam.data_ptr(), H, W, 1 if sphere_check else 0,
                                      B, vmax, ptr(out.get("cus")), ptr(out.get("cou_bb_proj")), ptr(counts), ptr(boxes), ptr(ok),
                                      ptr(masks), scratch.data_ptr()), "cp_mask_errors")
    if return_counts:
        out["counts"], out["ok"] = counts, ok.view(torch.bool)
    if return_boxes:
        out["boxes"] = boxes
    if return_masks:
        out["masks"] = masks.view(torch.bool)
    return out


def _as_masks(m, dev=None):
    m = torch.as_tensor(m)
    if dev is not None:
        m = m.to(dev)
    if m.dim() == 2:
        m = m[None]
    if m.dim() != 3:
        raise ValueError("masks must be (H,W) or (B,H,W), got %r" % (tuple(m.shape),))
    if m.dtype == torch.bool:
        return m.contiguous().view(torch.uint8)
    if m.dtype == torch.uint8:
        return m.contiguous()
    return (m != 0).view(torch.uint8)                         # astype(bool) of any other type


def mask_overlap(mask_est, mask_gt, kinds=("cou_mask", "cou_bb"), return_counts=False, return_boxes=False):
    """pose_error.cou_mask of B mask pairs and / or cou_bb of the masks' bounding boxes, on the device in ONE launch (cp_mask_overlap).
      mask_est, mask_gt: (B,H,W) (or (H,W)) CUDA tensors, bool or uint8 (any other dtype is compared with 0 first): nonzero = set,
      as the reference's astype(bool) -- e.g. the network's predicted segmentation against mask_visib.
    cou_mask = 1 - inter / union, 1.0 when the union is empty;  cou_bb = 1 - iou of the boxes (xmin, ymin, xmax - xmin, ymax - ymin)
    of the two masks, NaN where a mask is empty (misc.calc_2d_bbox raises there).
    -> dict kind -> (B,) float64 CUDA tensor (+ "counts": (B,4) int32 = inter, union, n_est, n_gt; + "boxes": (B,2,4) int32, -1 where empty)"""
    names = [kinds] if isinstance(kinds, str) else list(kinds)
    for k in names:
        if k not in OVERLAP_KINDS:
            raise ValueError("kinds must be among %s, got %r" % (list(OVERLAP_KINDS), k))
    if not names and not return_counts and not return_boxes:
        raise ValueError("kinds is empty: ask for \"cou_mask\", \"cou_bb\" or both")
    if not (torch.is_tensor(mask_est) and mask_est.is_cuda):
        raise RuntimeError("checkerpose_amd.metric: CUDA/HIP tensors required (no CPU fallback)")
    dev = mask_est.device
    me, mg = _as_masks(mask_est), _as_masks(mask_gt, dev)
    if me.shape != mg.shape:
        raise ValueError("mask_est is %r, mask_gt %r" % (tuple(me.shape), tuple(mg.shape)))
    B, H, W = (int(v) for v in me.shape)
    if B == 0 or H == 0 or W == 0:
        raise ValueError("no masks")
    lib = _abi.load()
    out = {k: torch.empty(B, dtype=torch.float64, device=dev) for k in OVERLAP_KINDS if k in names}
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev) if return_counts else None
    boxes = torch.empty((B, 2, 4), dtype=torch.int32, device=dev) if return_boxes else None
    ptr = lambda x: None if x is None else x.data_ptr()     # noqa: E731
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _abi.check(lib.cp_mask_overlap(st, me.data_ptr(), mg.data_ptr(), H, W, B, ptr(out.get("cou_mask")), ptr(out.get("cou_bb")),
                                       ptr(counts), ptr(boxes)), "cp_mask_overlap")
    if return_counts:
        out["counts"] = counts
    if return_boxes:
        out["boxes"] = boxes
    return out


def box_overlap(bb_est, bb_gt):
    """pose_error.cou_bb = 1 - misc.iou of B box pairs (x, y, w, h), on the device (cp_box_overlap): bb_est (B,4) CUDA tensor (any
    real dtype; computed in float64), bb_gt the same shape (tensor or host array).  -> (B,) float64 CUDA tensor"""
    if not (torch.is_tensor(bb_est) and bb_est.is_cuda):
        raise RuntimeError("checkerpose_amd.metric: CUDA/HIP tensors required (no CPU fallback)")
    dev = bb_est.device
    a = bb_est.reshape(-1, 4).to(torch.float64).contiguous()
    c = torch.as_tensor(bb_gt).to(device=dev, dtype=torch.float64).reshape(-1, 4).contiguous()
    if a.shape != c.shape or a.shape[0] == 0:
        raise ValueError("bb_est and bb_gt must both be (B,4), B > 0")
    B = int(a.shape[0])
    out = torch.empty(B, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _abi.check(_abi.load().cp_box_overlap(st, a.data_ptr(), c.data_ptr(), B, out.data_ptr()), "cp_box_overlap")
    return out


def _one_device(device):
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("checkerpose_amd.metric: a CUDA/HIP device is required (no CPU fallback)")
    return dev


def cou_mask(mask_est, mask_gt, device="cuda:0"):
    """bop_toolkit_lib.pose_error.cou_mask (two hxw arrays -> float), counted on the device"""
    dev = _one_device(device)
    f = lambda m: torch.from_numpy(np.ascontiguousarray(np.asarray(m).astype(bool))).to(dev)   # noqa: E731
    return float(mask_overlap(f(mask_est), f(mask_gt), kinds=("cou_mask",))["cou_mask"][0])


def cou_bb(bb_est, bb_gt, device="cuda:0"):
    """bop_toolkit_lib.pose_error.cou_bb (two boxes x, y, w, h -> float), on the device"""
    dev = _one_device(device)
    f = lambda b: torch.from_numpy(np.asarray(b, dtype=np.float64).reshape(1, 4)).to(dev)   # noqa: E731
    return float(box_overlap(f(bb_est), f(bb_gt))[0])


def _one_mask_error(kind, R_est, t_est, R_gt, t_gt, K, renderer, obj_id, size, device):
    dev = _one_device(device)
    if not isinstance(renderer, MeshSet) or renderer.faces is None:
        raise ValueError("renderer must be a MeshSet built with faces")
    if size is None:
        raise ValueError("size=(width, height) is required: a MeshSet has no frame")
    m = int(obj_id)
    if not 0 <= m < len(renderer):
        raise ValueError("obj_id must be a mesh index in 0..%d" % (len(renderer) - 1))
    f = lambda a, s: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(s))).to(dev)   # noqa: E731
    out = mask_errors(f(R_est, (1, 3, 3)), f(t_est, (1, 3, 1)), f(R_gt, (1, 3, 3)), f(t_gt, (1, 3, 1)),
                      np.asarray(K, dtype=np.float64).reshape(3, 3), renderer, size, mesh_ids=None if len(renderer) == 1 else [m],
                      kinds=(kind,))
    return float(out[kind][0])


def cus(R_est, t_est, R_gt, t_gt, K, renderer, obj_id, size=None, device="cuda:0"):
    """bop_toolkit_lib.pose_error.cus (numpy arrays of one pose -> float), rendered and counted on the device.  `renderer` is a
    MeshSet with faces and `obj_id` the index of the object's mesh in it; size=(W, H) is required, because a MeshSet has no frame.
    No sphere shortcut: that is the caller's."""
    return _one_mask_error("cus", R_est, t_est, R_gt, t_gt, K, renderer, obj_id, size, device)


def cou_bb_proj(R_est, t_est, R_gt, t_gt, K, renderer, obj_id, size=None, device="cuda:0"):
    """bop_toolkit_lib.pose_error.cou_bb_proj, with cus' arguments.  NaN where the reference raises (a silhouette with no pixel)."""
    return _one_mask_error("cou_bb_proj", R_est, t_est, R_gt, t_gt, K, renderer, obj_id, size, device)
