"""Object preparation on the device: what every other row starts from -- an object's farthest-point keypoints
and its diameter -- for an object that is not one of the reference's 44 pickles (another BOP dataset, a CAD model of one's own).

  farthest_point_sample_init_center(xyz, npoint)   the reference's name and return (preprocess_data/get_fps_points.py:65-90)
  fps_batch(clouds, npoint)                        M clouds in one cp_fps call -> device ids (M,npoint) int32, xyz (M,npoint,3) fp64
  pts_diameters(clouds) / calc_pts_diameter(pts)   exact largest pairwise distance (bop_toolkit_lib.misc.calc_pts_diameter) on the device
  prepare_object / prepare_objects                 -> ObjectModel: the fps pickle's dict, diameter, models_info entry, p3d_xyz,
                                                      p3d_normed with its centroid / range, and a MeshSet
Ids and diameters are the reference's bit for bit (tests/golden/prepare.npz): the kernels keep numpy's unfused fp64 expressions and
compare roots, not squares.  Timing: tools/prepare_bench.py, profiles/prepare_bench.json.
Not here: reading PLY files (pass the vertex array) and the kNN graph (construction-time, on the CPU for its tie order:
model/init.py).  The convex-hull visibility statistic of get_overall_visibility.py is row N16: checkerpose_amd/visibility.py.
There is no CPU fallback."""
import pickle

import numpy as np
import torch

from . import _abi, scene
from .aux_utils.pointnet2_utils import pc_normalize
from .scene import MeshSet


def pack_clouds(clouds):
    """one (V,3) array / tensor or a list of them -> (fp64 host table (sumV,3), int32 host offsets (M+1)); the reference promotes
    the PLY's floats to float64 the same way (get_fps_points.py:112-115)"""
    if torch.is_tensor(clouds) or isinstance(clouds, np.ndarray):
        clouds = [clouds]
    host = []
    for a in clouds:
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] == 0:
            raise ValueError("every cloud must be a non-empty (V, 3) array, got %r" % (a.shape,))
        a = np.ascontiguousarray(a, dtype=np.float64)
        if not np.isfinite(a).all():
            raise ValueError("a cloud holds NaN or infinite coordinates")
        host.append(a)
    if not host:
        raise ValueError("need at least one cloud")
    if len(host) > 65535:
        raise ValueError("at most 65535 clouds per call")
    off = np.zeros(len(host) + 1, dtype=np.int64)
    off[1:] = np.cumsum([a.shape[0] for a in host])
    if off[-1] >= 2 ** 31:
        raise ValueError("point table too large for int32 offsets")
    return np.concatenate(host, 0), off.astype(np.int32)


def _upload(clouds, device):
    dev = scene.cuda_device("prepare", device)
    table, off = pack_clouds(clouds)
    return dev, torch.from_numpy(table).to(dev), torch.from_numpy(off).to(dev), off


def _fps(dev, pts, off_dev, off, npoint, slices=0):
    npoint = int(npoint)
    if npoint < 1:
        raise ValueError("npoint must be at least 1")
    M, sizes = off.shape[0] - 1, np.diff(off)
    nbytes = _abi.load().cp_fps_scratch_bytes(M, int(off[-1]), int(sizes.max()), int(slices))
    if nbytes == 0:
        raise ValueError("cp_fps: bad shape (M = %d, slices = %r)" % (M, slices))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ids = torch.empty((M, npoint), dtype=torch.int32, device=dev)
    xyz = torch.empty((M, npoint, 3), dtype=torch.float64, device=dev)
    _abi.call("cp_fps", dev, pts, off_dev, off.ctypes.data, M, npoint, int(slices), ids, xyz, scratch)
    return ids, xyz


def _diameters(dev, pts, off_dev, off):
    M, sizes = off.shape[0] - 1, np.diff(off)
    nbytes = _abi.load().cp_pts_diameter_scratch_bytes(M, int(sizes.max()))
    if nbytes == 0:
        raise ValueError("cp_pts_diameter: a cloud of %d points is too large (at most 5792 * 1024)" % int(sizes.max()))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(M, dtype=torch.float64, device=dev)
    _abi.call("cp_pts_diameter", dev, pts, off_dev, off.ctypes.data, M, out, scratch)
    return out


def fps_batch(clouds, npoint, device="cuda:0", _slices=0):
    """Farthest-point samples of M clouds by the reference's rule, one cp_fps call.  clouds: a list of (V_m,3) arrays / tensors (or ONE),
    promoted to float64; non-finite coordinates raise ValueError.  npoint > V_m is legal (the reference then repeats index 0).
    -> (ids (M,npoint) int32, xyz (M,npoint,3) float64) on the device.  `_slices` (1 .. 256) forces the number of slices each cloud is
    cut into (tests, measurement: the output does not depend on it)."""
    dev, pts, off_dev, off = _upload(clouds, device)
    return _fps(dev, pts, off_dev, off, npoint, _slices)


def farthest_point_sample_init_center(xyz, npoint, device="cuda:0"):
    """get_fps_points.py:65-90 on the device: -> (fps_ids: list of int, fps_xyz: (npoint,3) float64 numpy)"""
    ids, pts = fps_batch([xyz], npoint, device)
    return [int(i) for i in ids[0].cpu().numpy()], pts[0].cpu().numpy()


def pts_diameters(clouds, device="cuda:0"):
    """exact largest pairwise distance of each of M clouds (promoted to float64) -> (M,) float64 on the device"""
    dev, pts, off_dev, off = _upload(clouds, device)
    return _diameters(dev, pts, off_dev, off)


def calc_pts_diameter(pts, device="cuda:0"):
    """bop_toolkit_lib.misc.calc_pts_diameter on the device (V^2 / 2 pairs) -> float"""
    return float(pts_diameters([pts], device)[0])


def model_info(vertices, diameter):
    """the object's entry of models_info.json as bop_toolkit's scripts/calc_model_info.py:36-47 forms it (that script is Python 2;
    restated): the bounding box's corner and size, and the diameter"""
    v = np.asarray(vertices)
    ref_pt = [float(c) for c in v.min(axis=0).flatten()]
    size = [float(c) for c in (v.max(axis=0) - ref_pt).flatten()]
    return {"min_x": ref_pt[0], "min_y": ref_pt[1], "min_z": ref_pt[2], "size_x": size[0], "size_y": size[1], "size_z": size[2],
            "diameter": float(diameter)}


def normalize_p3d(p3d_xyz):
    """train.py:118-125: -> (p3d_normed (1,3,n) float32 tensor, centroid (3,), range) through pc_normalize"""
    normed, centroid, m = pc_normalize(np.asarray(p3d_xyz, dtype=np.float64).copy(), return_stat=True)
    return torch.as_tensor(normed, dtype=torch.float32).transpose(1, 0).unsqueeze(0), centroid, float(m)


class ObjectModel:
    """What the train / test scripts load per object, made from its vertices: `fps` (the pickle's dict {"npoint", "id", "xyz"}),
    `diameter`, `model_info`, `p3d_xyz` (num_p3d,3), `p3d_normed` (1,3,num_p3d) fp32 with `centroid` and `range`, `meshset`."""

    def __init__(self, fps, diameter, info, num_p3d, meshset):
        self.fps, self.diameter, self.model_info, self.meshset = fps, float(diameter), info, meshset
        self.p3d_xyz = fps["xyz"][:num_p3d]
        self.p3d_normed, self.centroid, self.range = normalize_p3d(self.p3d_xyz)

    def save_fps(self, path):
        """obj_XXXXXX.pkl as get_fps_points.py:121-122 writes it (mmcv.dump of a .pkl is a plain pickle)"""
        with open(path, "wb") as f:
            pickle.dump(self.fps, f)


def prepare_objects(list_of_vertices, npoint_log2=12, num_p3d=None, faces=None, device="cuda:0"):
    """prepare_object for several objects with ONE cp_fps and ONE cp_pts_diameter call -> a list of ObjectModel.
    faces: None, or one (F_m,3) integer array per object."""
    vertices = list(list_of_vertices)
    if faces is not None:
        faces = list(faces)
        if len(faces) != len(vertices):
            raise ValueError("need one face array per object")
    npoint = int(2 ** int(npoint_log2))
    num_p3d = npoint if num_p3d is None else int(num_p3d)
    if not 1 <= num_p3d <= npoint:
        raise ValueError("num_p3d must be in 1..%d" % npoint)
    dev, pts, off_dev, off = _upload(vertices, device)
    ids, xyz = _fps(dev, pts, off_dev, off, npoint)
    diam = _diameters(dev, pts, off_dev, off)
    ids, xyz, diam = ids.cpu().numpy(), xyz.cpu().numpy(), diam.cpu().numpy()
    table = pts.cpu().numpy()
    out = []
    for m in range(len(vertices)):
        v = table[off[m]:off[m + 1]]
        fps = {"npoint": npoint, "id": [int(i) for i in ids[m]], "xyz": xyz[m].copy()}
        ms = MeshSet.from_arrays([v], diameters=[diam[m]], faces=None if faces is None else [faces[m]])
        out.append(ObjectModel(fps, diam[m], model_info(v, diam[m]), num_p3d, ms))
    return out


def prepare_object(vertices, npoint_log2=12, num_p3d=None, faces=None, device="cuda:0"):
    """One object's keypoints, diameter and tables from its (V,3) vertices (get_fps_points.py's __main__ + calc_model_info.py, without
    the PLY reader) -> ObjectModel.  npoint = 2 ** npoint_log2 samples are drawn; num_p3d (default: all) of them become the keypoints."""
    return prepare_objects([vertices], npoint_log2, num_p3d, None if faces is None else [faces], device)[0]
