"""The scene arguments of the scoring and rendering calls, each handled ONCE: what turns "poses, a camera, a MeshSet, ids, a frame"
into what a device call takes.  metric, gt_info, render, vis, bop_eval, coco_eval, prepare and visibility build on it.

  MeshSet, SymmetrySet            the packed vertex / face / colour / normal tables and symmetry sets of several objects, uploaded once
  symmetry_transformations, calc_pts_diameter      their host makers (bop_toolkit_lib.misc restated)
  require_cuda, cuda_device       the two device checks (there is no CPU fallback), with the calling module's name in the message
  on_device                       the per-device upload cache behind MeshSet.on / faces_on / shading_on and SymmetrySet.on
  pack_poses, poses_to_device, upload_pose         R, t -> (B,12) float64; host poses to the device; one numpy pose to (1,3,3)
  camera, mesh_ids_on, image_ids_host / image_ids_on / depth_images / group_by_image, frame_size, kinds_mask      the shape helpers
  mesh_poses, as_meshset, as_symmetries            the pose + mesh prologue of the rendering calls; bare arrays / lists -> the containers
  lighting, check_shaded_meshes, vec3, surf_colors_host      the shading arguments of render.render_rgb, vis.vis_poses and render.render_scene

The shape helpers are plain tensor plumbing: they never ask whether a tensor is on a GPU (require_cuda is a call of its own), so
they run on CPU tensors."""
import ctypes as C
import math
import weakref

import numpy as np
import torch


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


# ---- device checks and the upload cache ---------------------------------------------------------------------------------------------
def require_cuda(module, *tensors, device=None):
    """RuntimeError unless every one of `tensors` is a CUDA/HIP tensor (and `device`, when given, a CUDA/HIP device)"""
    ok = device is None or device.type == "cuda"
    for x in tensors:
        ok = ok and torch.is_tensor(x) and x.is_cuda
    if not ok:
        raise RuntimeError("checkerpose_amd.%s: CUDA/HIP tensors required (no CPU fallback)" % module)


def cuda_device(module, device):
    """torch.device(device); RuntimeError unless it names a CUDA/HIP device that is there"""
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("checkerpose_amd.%s: a CUDA/HIP device is required (no CPU fallback)" % module)
    return dev


def on_device(cache, device, make):
    """cache[device] -- made by make(device) on the first call for that device; the messages name metric, where the containers
    were first written"""
    device = torch.device(device)
    require_cuda("metric", device=device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in cache:
        cache[key] = make(device)
    return cache[key]


# ---- MeshSet ---------------------------------------------------------------------------------------------------------------------
def _is_array(x):
    return torch.is_tensor(x) or isinstance(x, np.ndarray)


def _per_mesh(items, single, rule, verts=None, count=None, none_ok=False):
    """The per-mesh arrays of MeshSet.from_arrays -> a list of numpy arrays.  items: a list, or ONE array when the vertices came as
    one (`single`); with `verts` (the vertex arrays already made) there must be one entry per mesh (ValueError `count`); every entry
    goes to numpy (None stays None where `none_ok`) and through rule(array, vertices of its mesh), which checks it and gives the
    array to keep."""
    items = [items] if single and _is_array(items) else list(items)
    if verts is not None and len(items) != len(verts):
        raise ValueError(count)
    host = [x.detach().cpu().numpy() if torch.is_tensor(x) else (None if x is None and none_ok else np.asarray(x)) for x in items]
    return [rule(x, None if verts is None else verts[m]) for m, x in enumerate(host)]


def _offsets(arrays, limit, what):
    off = np.zeros(len(arrays) + 1, dtype=np.int64)
    off[1:] = np.cumsum([a.shape[0] for a in arrays])
    if off[-1] >= limit:
        raise ValueError("%s table too large for int32 offsets" % what)
    return off


def _vertex_rule(a, _):
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] == 0:
        raise ValueError("every mesh must be a non-empty (V, 3) array, got %r" % (a.shape,))
    return np.ascontiguousarray(a, dtype=np.float32)


def _face_rule(f, a):
    if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError("faces must be (F, 3) integer arrays, got %r %s" % (f.shape, f.dtype))
    if f.shape[0] and (f.min() < 0 or f.max() >= a.shape[0]):
        raise ValueError("a face names a vertex outside 0..%d" % (a.shape[0] - 1))
    return np.ascontiguousarray(f, dtype=np.int32)


def _color_rule(c, a):
    if c is None:
        return np.full(a.shape, 0.5, dtype=np.float32)
    if c.shape != a.shape:
        raise ValueError("colors must be (V, 3) like the vertices, got %r" % (c.shape,))
    c = np.array(c, dtype=np.float32)
    if not np.isfinite(c).all():
        raise ValueError("colors must be finite")
    if c.max() > 1.0:
        c /= np.float32(255.0)
    return c


def _normal_rule(n, a):
    if n.shape != a.shape:
        raise ValueError("normals must be (V, 3) like the vertices, got %r" % (n.shape,))
    return np.ascontiguousarray(n, dtype=np.float32)


TEX_FILTERS = {"nearest": 0, "linear": 1}
TEX_MAX_SIDE = 16384


def _texture_rule(t, _):
    """one mesh's texture -> uint8 (Ht, Wt, 3) in the file's row order, or None"""
    if t is None:
        return None
    if t.ndim != 3 or t.shape[2] not in (3, 4):
        raise ValueError("a texture must be an (Ht, Wt, 3 | 4) array, got %r" % (t.shape,))
    if min(t.shape[:2]) < 1 or max(t.shape[:2]) > TEX_MAX_SIDE:
        raise ValueError("a texture's sides must lie in 1..%d, got %r" % (TEX_MAX_SIDE, t.shape[:2]))
    t = t[:, :, :3]
    if t.dtype == np.uint8:
        return np.ascontiguousarray(t)
    if not np.issubdtype(t.dtype, np.floating) and not np.issubdtype(t.dtype, np.integer):
        raise ValueError("a texture must hold uint8 or float values, got %s" % t.dtype)
    f = t.astype(np.float64)
    if not np.isfinite(f).all() or f.min() < 0.0:
        raise ValueError("a texture must hold finite values >= 0")
    if f.max() > 1.0:
        if f.max() > 255.0 or (f != np.rint(f)).any():
            raise ValueError("a texture whose largest value is > 1 must hold whole numbers in 0..255")
        return np.ascontiguousarray(f.astype(np.uint8))
    return np.ascontiguousarray(np.rint(255.0 * f).astype(np.uint8))     # UNPINNED: the project's own quantisation (half to even)


def _uv_rule(u, a):
    if u is None:
        return None
    if u.ndim != 2 or u.shape != (a.shape[0], 2):
        raise ValueError("uvs must be (V, 2) like the vertices, got %r" % (u.shape,))
    u = np.ascontiguousarray(u, dtype=np.float32)
    if not np.isfinite(u).all():
        raise ValueError("uvs must be finite")
    return u


def _texture_tables(textures, uvs, tex_filter, single, host):
    """MeshSet.from_arrays' texture arguments -> (uv (sumV,2) float32, texels (sum Wt Ht,) int32 RGBX words, offsets (M+1,) int32,
    dims (M,2) int32 = Wt, Ht) as CPU tensors, or None without textures"""
    if tex_filter not in TEX_FILTERS:
        raise ValueError("tex_filter must be \"nearest\" or \"linear\", got %r" % (tex_filter,))
    M = len(host)
    if textures is None:
        if uvs is not None and any(u is not None for u in ([uvs] if single and _is_array(uvs) else list(uvs))):
            raise ValueError("uvs without a texture")
        return None
    tex = _per_mesh(textures, single and _is_array(textures) and np.ndim(textures) == 3, _texture_rule, host,
                    "need one texture (or None) per mesh", none_ok=True)
    uv = _per_mesh([None] * M if uvs is None else uvs, single, _uv_rule, host, "need one uv array (or None) per mesh", none_ok=True)
    for m in range(M):
        if (tex[m] is None) != (uv[m] is None):
            raise ValueError("mesh %d: %s" % (m, "a texture without uvs" if uv[m] is None else "uvs without a texture"))
    if all(t is None for t in tex):
        return None
    off = np.zeros(M + 1, dtype=np.int64)
    off[1:] = np.cumsum([0 if t is None else t.shape[0] * t.shape[1] for t in tex])
    if off[-1] >= 2 ** 31:
        raise ValueError("the textures hold %d texels: 2^31 or more" % off[-1])
    dims = np.array([(0, 0) if t is None else (t.shape[1], t.shape[0]) for t in tex], dtype=np.int32)
    words = np.zeros(int(off[-1]), dtype=np.uint32)
    for m, t in enumerate(tex):
        if t is not None:
            w = t.astype(np.uint32)
            words[off[m]:off[m + 1]] = (w[:, :, 0] | (w[:, :, 1] << 8) | (w[:, :, 2] << 16)).reshape(-1)
    uvt = np.concatenate([np.zeros((a.shape[0], 2), dtype=np.float32) if uv[m] is None else uv[m] for m, a in enumerate(host)], 0)
    return (torch.from_numpy(np.ascontiguousarray(uvt)), torch.from_numpy(words.view(np.int32)), torch.from_numpy(off.astype(np.int32)),
            torch.from_numpy(dims))


def _table(arrays):
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(arrays, 0)))


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
        self.uvs = self.texels = self.tex_offsets = self.tex_dims = None     # the texture tables (row N20), set by from_arrays
        self.tex_filter = "nearest"         # lives on the MeshSet, as GL keeps it on the texture object
        self._dev_tex = {}

    @classmethod
    def from_arrays(cls, arrays, diameters=None, faces=None, device=None, colors=None, normals=None, uvs=None, textures=None,
                    tex_filter="nearest"):
        """arrays: a list of (V_m, 3) arrays / tensors (or ONE such array); diameters: one per mesh, or None = computed as the
        reference does (largest pairwise distance of the vertices) -- on the host, or with `device` on that device
        (prepare.pts_diameters: the same bits); faces: None, or one (F_m, 3) integer array of vertex indices
        per mesh (or ONE such array with one mesh) -- the triangles vsd_errors / render_depth rasterise;
        colors: None, or per mesh a (V_m, 3) uint8 / float array of vertex colours or None (that mesh is 0.5 grey) -- as
        renderer_py's add_object takes them: a mesh whose largest value is > 1 is divided by 255 (in float32);
        normals: None, or one (V_m, 3) float array per mesh (every mesh): render.render_rgb's phong shading.
        With both None the object is what it was before these arguments existed.
        textures: None, or per mesh None or an (Ht, Wt, 3 | 4) image in the FILE's row order (row 0 on top, as inout.load_im gives it;
        alpha is dropped; sides 1..16384, fewer than 2^31 texels in all): uint8 as it is; floats whose largest value is > 1 must be
        whole numbers in 0..255; floats <= 1 are quantised round-half-even(255 x) (UNPINNED: the project's own choice -- the reference
        keeps image / 255 in float32);  uvs: per mesh None or a finite (V_m, 2) float array (texture_u, texture_v), given exactly for
        the meshes that have a texture;  tex_filter "nearest" or "linear": GL's sampler rule with clamp-to-edge, no mipmaps
        (csrc/render_shade.h).  A textured mesh is coloured by its texture, its vertex colours are ignored (add_object's order).
        With textures None the MeshSet is what it is without these arguments."""
        single = _is_array(arrays)
        host = _per_mesh(arrays, single, _vertex_rule)
        if not host:
            raise ValueError("MeshSet needs at least one mesh")
        off = _offsets(host, 2 ** 31, "vertex")
        if diameters is None and device is not None:
            from .prepare import pts_diameters
            diameters = pts_diameters(host, device).cpu().numpy()
        elif diameters is None:
            diameters = [calc_pts_diameter(a) for a in host]
        diameters = np.asarray(diameters, dtype=np.float64).reshape(-1)
        if diameters.shape[0] != len(host):
            raise ValueError("need one diameter per mesh")
        ftab = foff = ctab = ntab = None
        if faces is not None:
            fhost = _per_mesh(faces, single, _face_rule, host, "need one face array per mesh")
            fo = _offsets(fhost, 2 ** 31 // 3, "face")
            ftab = torch.from_numpy(np.concatenate(fhost, 0).reshape(-1, 3)) if fo[-1] else torch.zeros((1, 3), dtype=torch.int32)
            foff = torch.from_numpy(fo.astype(np.int32))
        if colors is not None:
            ctab = _table(_per_mesh(colors, single, _color_rule, host, "need one colour array (or None) per mesh", none_ok=True))
        if normals is not None:
            normals = [normals] if single and _is_array(normals) else list(normals)
            if len(normals) != len(host) or any(n is None for n in normals):
                raise ValueError("need one normal array per mesh")
            ntab = _table(_per_mesh(normals, False, _normal_rule, host))
        tex = _texture_tables(textures, uvs, tex_filter, single, host)
        ms = cls(torch.from_numpy(np.concatenate(host, 0)), torch.from_numpy(off.astype(np.int32)), diameters, ftab, foff, ctab, ntab)
        if tex is not None:
            ms.uvs, ms.texels, ms.tex_offsets, ms.tex_dims = tex
            ms.tex_filter = tex_filter
        return ms

    def __len__(self):
        return int(self.offsets.numel()) - 1

    def on(self, device):
        """(verts, offsets) on `device`, uploaded on the first call"""
        return on_device(self._dev, device, lambda d: (self.verts.to(d), self.offsets.to(d)))

    def faces_on(self, device):
        """(faces, face offsets, diameters) on `device`, uploaded on the first call; ValueError without a face table"""
        if self.faces is None:
            raise ValueError("this MeshSet has no faces: build it with MeshSet.from_arrays(..., faces=...) to render it")
        return on_device(self._dev_faces, device, lambda d: (
            self.faces.to(d), self.face_offsets.to(d), torch.from_numpy(np.ascontiguousarray(self.diameters, dtype=np.float64)).to(d)))

    def shading_on(self, device):
        """(colors or None, normals or None) on `device`, uploaded on the first call"""
        return on_device(self._dev_shading, device, lambda d: (None if self.colors is None else self.colors.to(d),
                                                               None if self.normals is None else self.normals.to(d)))

    def textures_on(self, device, use=True):
        """the texture arguments of the _tex entry points: (uvs, texels, offsets, dims, filter code) on `device`, uploaded on the first
        call; four Nones and 0 without textures or with `use` false (a surface colour overrides them)"""
        if self.texels is None or not use:
            return None, None, None, None, 0
        return on_device(self._dev_tex, device, lambda d: (self.uvs.to(d), self.texels.to(d), self.tex_offsets.to(d), self.tex_dims.to(d))) + (
            TEX_FILTERS[self.tex_filter],)


_MESH_CACHE = {}        # id(array) -> (weak reference to the array, MeshSet): the upload of a mesh happens once per array


def as_meshset(vertices):
    """a MeshSet as it is; a bare (V,3) array / tensor or a list of them -> a MeshSet without diameters, cached per array OBJECT
    (test.py's loop passes the same `vertices` for every image), dropped when the array is collected.  The array is taken as
    constant: edit it in place and the cache is stale."""
    if isinstance(vertices, MeshSet):
        return vertices
    if isinstance(vertices, (list, tuple)):
        return MeshSet.from_arrays(list(vertices), diameters=np.full(len(vertices), np.nan))
    key = id(vertices)
    hit = _MESH_CACHE.get(key)
    if hit is not None and hit[0]() is vertices:
        return hit[1]
    ms = MeshSet.from_arrays([vertices], diameters=[np.nan])
    _MESH_CACHE[key] = (weakref.ref(vertices, lambda _r, k=key: _MESH_CACHE.pop(k, None)), ms)
    return ms


# ---- SymmetrySet -----------------------------------------------------------------------------------------------------------------
def _rotation_about(angle, axis):
    """rotation by `angle` about `axis` through the origin (bop_toolkit_lib.transform.rotation_matrix restated, 3x3 part): the
    axis is normalised first; R = cos I + (1 - cos) a a^T + sin [a]_x, summed in that order"""
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
    def from_models_info(cls, infos, max_sym_disc_step=0.01, rotations_as=None):
        """infos: one models_info.json entry (dict) per mesh, in MeshSet order -> misc.get_symmetry_transformations of each.
        rotations_as=np.float32 rounds every rotation entry through float32, as the LM loader's `load_lm_obj_sym_info` keeps them
        (lm_dataset_pytorch.py:552-563), so that targets.pose_re_te_sym meets the candidates test_lm.py meets; the translations and
        the default (None: float64 as computed) are unchanged."""
        if isinstance(infos, dict):
            raise ValueError("pass a LIST of models_info entries, one per mesh in MeshSet order")
        if rotations_as is not None and np.dtype(rotations_as) != np.dtype(np.float32):
            raise ValueError("rotations_as must be None or np.float32, got %r" % (rotations_as,))
        ss = cls.from_transforms([symmetry_transformations(i, max_sym_disc_step) for i in infos])
        if rotations_as is not None:
            ss.table[:, :9] = ss.table[:, :9].to(torch.float32).to(torch.float64)
        return ss

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
        return on_device(self._dev, device, lambda d: (self.table.to(d), self.offsets.to(d)))


_IDENTITY_SETS = {}     # M -> SymmetrySet of M identities (symmetries=None)


def as_symmetries(symmetries, M):
    """a SymmetrySet as it is, a list of bop_toolkit `syms` lists packed, None = the identity alone for each of M meshes"""
    if symmetries is None:
        if M not in _IDENTITY_SETS:
            _IDENTITY_SETS[M] = SymmetrySet.identity(M)
        ss = _IDENTITY_SETS[M]
    else:
        ss = symmetries if isinstance(symmetries, SymmetrySet) else SymmetrySet.from_transforms(symmetries)
    if len(ss) != M:
        raise ValueError("%d symmetry sets for %d meshes" % (len(ss), M))
    return ss


# ---- poses -----------------------------------------------------------------------------------------------------------------------
def pack_poses(R, t, B=None, dev=None):
    """(B,3,3) + (B,3,1) / (B,3) -> contiguous (B,12) float64 [R row-major | t]; a lone (3,3) is one pose.  With `dev`, R and t
    may be host arrays too: they go there first (96 bytes per pose)."""
    if dev is not None:
        R, t = torch.as_tensor(R, dtype=torch.float64).to(dev), torch.as_tensor(t, dtype=torch.float64).to(dev)
    if R.dim() == 2:
        R = R[None]
    B = R.shape[0] if B is None else B
    if tuple(R.shape) != (B, 3, 3) or t.numel() != 3 * B:
        raise ValueError("poses must be R (B,3,3) and t (B,3,1) / (B,3); got %r and %r" % (tuple(R.shape), tuple(t.shape)))
    return torch.cat([R.reshape(B, 9).to(torch.float64), t.reshape(B, 3).to(torch.float64)], 1).contiguous()


def poses_to_device(module, R, t):
    """solve_pnp_ransac's device tensors as they are; host arrays / CPU tensors go to the current device (96 bytes per pose)"""
    if torch.is_tensor(R) and R.is_cuda:
        dev = R.device
    elif torch.is_tensor(t) and t.is_cuda:
        dev = t.device
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("checkerpose_amd.%s: a CUDA/HIP device is required (no CPU fallback)" % module)
        dev = torch.device("cuda", torch.cuda.current_device())
    return torch.as_tensor(R).to(device=dev, dtype=torch.float64), torch.as_tensor(t).to(device=dev, dtype=torch.float64)


def upload_pose(R, t, dev):
    """one pose as host arrays (the reference's numpy-in signatures) -> float64 R (1,3,3) and t (1,3,1) on `dev`"""
    f = lambda a, s: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(s))).to(dev)   # noqa: E731
    return f(R, (1, 3, 3)), f(t, (1, 3, 1))


def mesh_poses(R, t, meshes):
    """The prologue of every call that rasterises: R, t must be CUDA/HIP tensors and `meshes` a MeshSet with faces
    -> (device, (B,12) poses, B)"""
    require_cuda("metric", R, t)
    if not isinstance(meshes, MeshSet):
        raise ValueError("VSD renders triangles: pass a MeshSet built with faces")
    if meshes.faces is None:
        raise ValueError("this MeshSet has no faces: build it with MeshSet.from_arrays(..., faces=...) to render it")
    poses = pack_poses(R, t)
    if poses.shape[0] == 0:
        raise ValueError("no poses")
    return R.device, poses, poses.shape[0]


# ---- camera, ids, frame, kinds ---------------------------------------------------------------------------------------------------
def camera(cam_K, n, dev, letter="B"):
    """cam_K (3,3) for all, or (n,3,3) -> (float64 K on dev, its stride in doubles: 0 or 9); `letter` names n in the message"""
    K = torch.as_tensor(cam_K).to(device=dev, dtype=torch.float64)
    if tuple(K.shape) == (3, 3):
        return K.reshape(9).contiguous(), 0
    if tuple(K.shape) == (n, 3, 3):
        return K.reshape(n, 9).contiguous(), 9
    raise ValueError("cam_K must be (3,3) or (%s,3,3), got %r" % (letter, tuple(K.shape)))


def _resident(x, dev):
    return torch.is_tensor(x) and x.device.type == dev.type


def mesh_ids_on(mesh_ids, B, dev, *sizes):
    """Each pose's mesh among M = len(sizes[0]): -> (int32 ids on dev, or None with one mesh; the largest entry of every size
    table in `sizes` -- MeshSet.sizes, SymmetrySet.sizes -- that a pose can reach).  Ids that already live on dev's kind of device
    stay there unread (an id outside 0..M-1 scores NaN in the kernels), so the largest is over ALL meshes; host ids are checked and
    the largest is over the meshes used."""
    M = len(sizes[0])
    if mesh_ids is None:
        if M != 1:
            raise ValueError("several meshes need mesh_ids")
        return None, [int(s[0]) for s in sizes]
    if _resident(mesh_ids, dev):
        if mesh_ids.numel() != B:
            raise ValueError("mesh_ids must be (B,)")
        return mesh_ids.reshape(-1).to(device=dev, dtype=torch.int32).contiguous(), [int(s.max()) for s in sizes]
    host = np.asarray(mesh_ids).reshape(-1).astype(np.int64)
    if host.shape[0] != B or host.min() < 0 or host.max() >= M:
        raise ValueError("mesh_ids must be (B,) with values in 0..%d" % (M - 1))
    used = np.unique(host)
    return torch.from_numpy(host.astype(np.int32)).to(dev), [int(s[used].max()) for s in sizes]


def image_ids_host(image_ids, B, n_img, what="depth images", letter="B"):
    """Each pose's image on the host -> (B,) int64, or None when there is ONE image and no ids (every pose reads it).  The default
    rule: the one image, or image b for pose b when I == B."""
    if image_ids is None:
        if n_img == 1:
            return None
        if n_img == B:
            return np.arange(B, dtype=np.int64)
        raise ValueError("%d %s for %d poses need image_ids" % (n_img, what, B))
    host = np.asarray(image_ids).reshape(-1).astype(np.int64)
    if host.shape[0] != B or (B and (host.min() < 0 or host.max() >= n_img)):
        raise ValueError("image_ids must be (%s,) with values in 0..%d" % (letter, n_img - 1))
    return host


def image_ids_on(image_ids, B, n_img, dev):
    """-> int32 ids on dev, or None for the one image.  Ids that already live on dev's kind of device stay there unread (an id
    outside 0..I-1 scores NaN); host ids are checked."""
    if _resident(image_ids, dev):
        if image_ids.numel() != B:
            raise ValueError("image_ids must be (B,)")
        return image_ids.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    host = image_ids_host(image_ids, B, n_img)
    return None if host is None else torch.from_numpy(host.astype(np.int32)).to(dev)


def depth_images(depth, image_ids, B, dev):
    """depth (H,W) or (I,H,W) and the ids of B poses -> (float32 (I,H,W) on dev, image_ids_on's ids, I)"""
    d = torch.as_tensor(depth)
    if d.dim() == 2:
        d = d[None]
    if d.dim() != 3:
        raise ValueError("depth_test must be (H,W) or (I,H,W), got %r" % (tuple(d.shape),))
    d = d.to(device=dev, dtype=torch.float32).contiguous()
    return d, image_ids_on(image_ids, B, int(d.shape[0]), dev), int(d.shape[0])


def group_by_image(image_ids, P, n_img):
    """-> (image of pose (P,) int32, img_off (I+1,) int32, pose_order (P,) int32): the stable grouping of the poses by image, all
    on the host (device ids are downloaded)"""
    ids = image_ids_host(image_ids.cpu() if torch.is_tensor(image_ids) else image_ids, P, n_img, "frames", "P")
    if ids is None:
        ids = np.zeros(P, dtype=np.int64)
    order = np.argsort(ids, kind="stable").astype(np.int32)
    off = np.zeros(n_img + 1, dtype=np.int32)
    off[1:] = np.cumsum(np.bincount(ids, minlength=n_img))
    return ids.astype(np.int32), off, order


def frame_size(size):
    """size = (width, height), as bop_toolkit's renderers take it -> (W, H), both positive"""
    W, H = int(size[0]), int(size[1])
    if W <= 0 or H <= 0:
        raise ValueError("size must be (width, height), both positive")
    return W, H


def kinds_mask(kinds, table, empty):
    """One kind or several -> their bits or-ed.  table: a dict name -> bit (the message lists the names sorted), or a tuple of names
    (bit 1 << position; listed in order).  empty: the ValueError text of an empty request, or None where that is allowed."""
    bits = table if isinstance(table, dict) else {k: 1 << n for n, k in enumerate(table)}
    mask = 0
    for k in ([kinds] if isinstance(kinds, str) else kinds):
        if k not in bits:
            raise ValueError("kinds must be among %s, got %r" % (sorted(table) if isinstance(table, dict) else list(table), k))
        mask |= bits[k]
    if not mask and empty is not None:
        raise ValueError(empty)
    return mask


# ---- lighting ----------------------------------------------------------------------------------------------------------------------
SHADINGS = {"flat": 0, "phong": 1}


def vec3(x, name):
    """three finite values -> a ctypes double[3]"""
    v = np.asarray(x, dtype=np.float64).reshape(-1)
    if v.shape[0] != 3 or not np.isfinite(v).all():
        raise ValueError("%s must be 3 finite values, got %r" % (name, x))
    return (C.c_double * 3)(*v.tolist())


def lighting(shading, ambient_weight, light_cam_pos):
    """render_rgb's / vis_poses' light (renderer.py:23-29) -> (SHADINGS code, ambient weight, the light as a double[3] in the
    poses' camera frame: light_cam_pos is in OpenGL's -- x right, y UP, z towards the viewer)"""
    if shading not in SHADINGS:
        raise ValueError("shading must be \"flat\" or \"phong\", got %r" % (shading,))
    amb = float(ambient_weight)
    if not math.isfinite(amb):
        raise ValueError("ambient_weight must be finite")
    light = np.asarray(light_cam_pos, dtype=np.float64).reshape(-1)
    if light.shape[0] != 3:
        raise ValueError("light_cam_pos must be 3 values")
    return SHADINGS[shading], amb, vec3(light * np.array([1.0, -1.0, -1.0]), "light_cam_pos")


def check_shaded_meshes(meshes, shading, who):
    if not isinstance(meshes, MeshSet):
        raise ValueError("%s renders triangles: pass a MeshSet built with faces" % who)
    if shading == "phong" and meshes.normals is None:
        raise ValueError("phong shading needs vertex normals: MeshSet.from_arrays(..., normals=...)")


def surf_colors_host(surf_colors, P):
    """one colour per pose, or one for all, RGB in [0, 1] -> float64 (P,3) on the host; None stays None (the mesh's own colours)"""
    if surf_colors is None:
        return None
    surf = np.asarray(surf_colors.cpu() if torch.is_tensor(surf_colors) else surf_colors, dtype=np.float64)
    if surf.size == 3:
        surf = np.tile(surf.reshape(1, 3), (P, 1))
    if surf.shape != (P, 3) or not np.isfinite(surf).all():
        raise ValueError("surf_colors must be (P,3) or one colour, all finite")
    return surf
