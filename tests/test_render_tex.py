"""Row N20 (UV texture sampling) without a device: the MeshSet's texture tables, the statement and its fp32 restatement, the ABI.

  MeshSet       every ValueError of from_arrays' texture arguments; the RGBX words, offsets, dims, UV table; textures=None leaves the
                MeshSet what it was
  inputs        every case leaves at most 5 % of its covered pixels undecided (the cap of tests/test_render_rgb.py), by the oracle alone
  restatement   render_tex_f32 (the device's arithmetic in numpy float32) lies in the oracle's band on every decided pixel, both filters
  mutations     each of the six mutations of the statement is caught by at least one case (printed: by which)
  ABI           the three _tex entry points exist in the header and in SIGNATURES; their argument checks refuse bad sizes, null UVs with
                texels, an unknown filter -- with fake pointers, nothing launches; cp_version() >= 230"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import render_rgb_stages as RS
from tests import render_tex_stages as TS

HERE = os.path.dirname(os.path.abspath(__file__))
_O, _F32 = {}, {}


def oracle(ci, filt, mut=None):
    """the oracle of a case, computed once and shared (left unchanged by its users)"""
    if (ci, filt, mut) not in _O:
        _O[(ci, filt, mut)] = TS.oracle_tex(filt=filt, mut=mut, **TS.case_args(TS.CASES[ci]))
    return _O[(ci, filt, mut)]


def restated(ci, filt):
    if (ci, filt) not in _F32:
        _F32[(ci, filt)] = TS.render_tex_f32(filt=filt, **TS.case_args(TS.CASES[ci]))[0]
    return _F32[(ci, filt)]


# ---- MeshSet ---------------------------------------------------------------------------------------------------------------------------
def _words(t):
    t = t.astype(np.uint32)
    return (t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16)).reshape(-1)


def test_meshset_packs_the_texture_tables():
    from checkerpose_amd import metric
    m, tx = TS.tex_meshes(), TS.textures()
    names = ("quad", "box", "ico80")
    tex = [tx["t5x3"], None, tx["grad64x16"]]
    uvs = [m["quad"][2], None, m["ico80"][2]]
    ms = metric.MeshSet.from_arrays([m[k][0] for k in names], faces=[m[k][1] for k in names], normals=[m[k][3] for k in names],
                                    diameters=[100.0] * 3, uvs=uvs, textures=tex, tex_filter="linear")
    assert ms.tex_filter == "linear"
    assert ms.tex_offsets.dtype.is_floating_point is False and ms.tex_offsets.tolist() == [0, 15, 15, 15 + 1024]
    assert ms.tex_dims.tolist() == [[5, 3], [0, 0], [64, 16]]
    words = ms.texels.numpy().view(np.uint32)
    assert words.shape == (15 + 1024,) and (words >> 24 == 0).all()
    assert np.array_equal(words[:15], _words(tx["t5x3"])) and np.array_equal(words[15:], _words(tx["grad64x16"]))      # file row order
    assert words[0] == 20 | (250 << 8) | (40 << 16)
    V = [m[k][0].shape[0] for k in names]
    uv = ms.uvs.numpy()
    assert uv.dtype == np.float32 and uv.shape == (sum(V), 2)
    assert np.array_equal(uv[:V[0]], m["quad"][2]) and not uv[V[0]:V[0] + V[1]].any() and np.array_equal(uv[V[0] + V[1]:], m["ico80"][2])
    # alpha is dropped; integer-valued floats above 1 are bytes; floats in [0, 1] are quantised round-half-even(255 x)
    rgba = np.concatenate([tx["t2x2"], np.full((2, 2, 1), 7, dtype=np.uint8)], -1)
    one = lambda t: metric.MeshSet.from_arrays(m["quad"][0], faces=m["quad"][1], diameters=[1.0], uvs=m["quad"][2], textures=t)      # noqa: E731
    assert np.array_equal(one(rgba).texels.numpy().view(np.uint32), _words(tx["t2x2"]))
    assert np.array_equal(one(tx["t2x2"].astype(np.float32)).texels.numpy().view(np.uint32), _words(tx["t2x2"]))
    f01 = np.array([[[0.5, 2.5 / 255.0, 1.0], [0.0, 0.3, 3.5 / 255.0]]])
    assert one(f01).texels.numpy().view(np.uint32).tolist() == [128 | (2 << 8) | (255 << 16), 0 | (76 << 8) | (4 << 16)]      # 127.5 -> 128, 2.5 -> 2, 3.5 -> 4
    assert one(f01).tex_dims.tolist() == [[2, 1]] and one(f01).tex_filter == "nearest"
    # several meshes, ONE of them textured, given as lists with None
    two = metric.MeshSet.from_arrays([m["quad"][0], m["box"][0]], faces=[m["quad"][1], m["box"][1]], diameters=[1.0, 1.0], uvs=[None, m["box"][2]],
                                     textures=[None, tx["t1x1"]])
    assert two.tex_offsets.tolist() == [0, 0, 1] and two.tex_dims.tolist() == [[0, 0], [1, 1]]


def test_meshset_without_textures_is_what_it_was():
    from checkerpose_amd import metric
    v, f, c, n = RS.meshes()["ico80"]
    a = metric.MeshSet.from_arrays([v, v], faces=[f, f], colors=[c, None], normals=[n, n], diameters=[1.0, 2.0])
    for b in (metric.MeshSet.from_arrays([v, v], faces=[f, f], colors=[c, None], normals=[n, n], diameters=[1.0, 2.0], uvs=None, textures=None,
                                         tex_filter="linear"),
              metric.MeshSet.from_arrays([v, v], faces=[f, f], colors=[c, None], normals=[n, n], diameters=[1.0, 2.0], textures=[None, None])):
        for k in ("verts", "offsets", "faces", "face_offsets", "colors", "normals"):
            assert getattr(a, k).dtype == getattr(b, k).dtype and np.array_equal(getattr(a, k).numpy(), getattr(b, k).numpy()), k
        assert np.array_equal(a.diameters, b.diameters) and np.array_equal(a.sizes, b.sizes)
        assert b.texels is None and b.uvs is None and b.tex_offsets is None and b.tex_dims is None
        assert b.textures_on("cpu") == (None, None, None, None, 0)     # no device is asked for


def test_meshset_refuses_bad_texture_arguments():
    from checkerpose_amd import metric
    m, tx = TS.tex_meshes(), TS.textures()
    v, f, uv, _ = m["quad"]
    mk = lambda **kw: metric.MeshSet.from_arrays(v, faces=f, diameters=[1.0], **kw)      # noqa: E731
    mk(uvs=uv, textures=tx["t2x2"])
    nan_uv = uv.copy()
    nan_uv[1, 0] = np.nan
    inf_uv = uv.copy()
    inf_uv[2, 1] = np.inf
    for kw in (dict(textures=tx["t2x2"]),                               # a texture without UVs
               dict(uvs=uv),                                            # UVs without a texture
               dict(uvs=nan_uv, textures=tx["t2x2"]), dict(uvs=inf_uv, textures=tx["t2x2"]),
               dict(uvs=uv[:3], textures=tx["t2x2"]), dict(uvs=np.zeros((4, 3), dtype=np.float32), textures=tx["t2x2"]),      # wrong shapes
               dict(uvs=uv, textures=np.zeros((2, 2), dtype=np.uint8)), dict(uvs=uv, textures=np.zeros((2, 2, 2), dtype=np.uint8)),
               dict(uvs=uv, textures=np.zeros((2, 2, 5), dtype=np.uint8)),
               dict(uvs=uv, textures=np.zeros((0, 2, 3), dtype=np.uint8)), dict(uvs=uv, textures=np.zeros((2, 0, 3), dtype=np.uint8)),      # a side of 0
               dict(uvs=uv, textures=np.zeros((1, 16385, 3), dtype=np.uint8)), dict(uvs=uv, textures=np.zeros((16385, 1, 3), dtype=np.uint8)),
               dict(uvs=uv, textures=np.full((2, 2, 3), 1.5)), dict(uvs=uv, textures=np.full((2, 2, 3), 256.0)),      # floats above 1: whole bytes
               dict(uvs=uv, textures=np.full((2, 2, 3), -0.1)), dict(uvs=uv, textures=np.full((2, 2, 3), np.nan)),
               dict(uvs=uv, textures=tx["t2x2"], tex_filter="cubic"), dict(tex_filter="mipmap")):      # an unknown filter, with or without textures
        with pytest.raises(ValueError):
            mk(**kw)
    with pytest.raises(ValueError):                                     # per mesh: mesh 1 has UVs and no texture
        metric.MeshSet.from_arrays([v, v], faces=[f, f], diameters=[1.0, 1.0], uvs=[uv, uv], textures=[tx["t2x2"], None])
    with pytest.raises(ValueError):                                     # one entry per mesh
        metric.MeshSet.from_arrays([v, v], faces=[f, f], diameters=[1.0, 1.0], uvs=[uv, uv], textures=[tx["t2x2"]])


def test_a_total_of_2_31_texels_is_refused(monkeypatch):
    """eight 16384 x 16384 textures hold 2^31 texels: refused from the shapes, before a word is packed (numpy views of one byte stand
    for the images)"""
    from checkerpose_amd import metric, scene
    v, f, uv, _ = TS.tex_meshes()["quad"]
    big = np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.uint8), shape=(16384, 16384, 3), strides=(0, 0, 0))
    monkeypatch.setattr(scene, "_texture_rule", lambda t, _: t)       # (the rule would copy 768 MB per texture; its checks are pinned above)
    with pytest.raises(ValueError, match="2\\^31"):
        metric.MeshSet.from_arrays([v] * 8, faces=[f] * 8, diameters=[1.0] * 8, uvs=[uv] * 8, textures=[big] * 8)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def test_cases_cover_the_meshes_textures_and_frames_and_keep_the_undecided_cap():
    assert {c["mesh"] for c in TS.CASES} == {"quad", "quadover", "box", "slab", "ico80", "faceted"}
    assert {c["tex"] for c in TS.CASES} == {"t1x1", "t2x2", "t5x3", "check8", "grad64x16"}
    assert {c["size"] for c in TS.CASES} == {(67, 45), (33, 65), (32, 32)}
    for t in TS.textures().values():
        assert t.dtype == np.uint8 and t.max() > 1
    assert len({tuple(p) for p in TS.textures()["t5x3"].reshape(-1, 3).tolist()}) == 15
    for ci, c in enumerate(TS.CASES):
        for filt in TS.FILTERS:
            o = oracle(ci, filt)
            share = RS.undecided_share(o)
            print("%-16s %-8s covered %5d  undecided %.4f" % (c["name"], filt, int(o["covered"].sum()), share))
            assert o["covered"].sum() >= 400 and share <= 0.05, (c["name"], filt, share)


def test_faceted_faces_lie_inside_one_texel():
    v, f, uv, _ = TS.tex_meshes()["faceted"]
    assert len(np.unique(f)) == f.size                                 # no shared vertices
    for k, face in enumerate(f):
        i, j = np.floor(uv[face, 0].astype(np.float64) * 5), np.floor(uv[face, 1].astype(np.float64) * 3)
        assert len(set(i)) == 1 and len(set(j)) == 1 and TS.face_texel(k) == (2 - int(j[0]), int(i[0]))


def test_fp32_restatement_lies_in_the_band():
    worst = -np.inf
    for ci, c in enumerate(TS.CASES):
        for filt in TS.FILTERS:
            ok, ratio, equal, nbad = RS.check_band(restated(ci, filt), oracle(ci, filt))
            print("%-16s %-8s ratio %8.4f  equal %.4f  outside %d" % (c["name"], filt, ratio, equal, nbad))
            assert ok, (c["name"], filt, nbad)
            worst = max(worst, ratio)
    print("fp32 restatement: worst (|u8 - v| - 0.5) / tol_c = %.4f" % worst)
    assert worst <= 1.0


def test_nearest_at_full_ambient_is_the_texel_byte():
    for ci, c in enumerate(TS.CASES):
        if c["ambient"] == 1.0:
            o = oracle(ci, "nearest")
            sel = o["decided"] & o["covered"]
            assert sel.sum() > 300 and np.array_equal(restated(ci, "nearest")[sel], o["texel"][sel].astype(np.uint8)), c["name"]


def test_every_mutation_of_the_statement_is_caught():
    caught = {}
    for mut in TS.MUTATIONS:
        for ci, c in enumerate(TS.CASES):
            for filt in (("linear",) if mut == "nohalf" else TS.FILTERS):
                if mut in caught:
                    break
                ok, ratio, equal, nbad = RS.check_band(restated(ci, filt), oracle(ci, filt, mut))
                if not ok:
                    caught[mut] = (c["name"], filt, nbad)
    for mut in TS.MUTATIONS:
        print("mutation %-9s caught by %s" % (mut, caught.get(mut)))
    assert set(caught) == set(TS.MUTATIONS), sorted(set(TS.MUTATIONS) - set(caught))


def test_sampler_by_hand():
    """the 2 x 2 texture: GL row 0 is the file's LAST row; linear at a texel centre is that texel, midway the mean; clamp-to-edge"""
    t = TS.textures()["t2x2"]
    pt = lambda u, v, filt: TS.sample(t, np.array([u]), np.array([v]), filt)[0].tolist()      # noqa: E731
    assert pt(0.1, 0.1, "nearest") == [20, 20, 250] and pt(0.9, 0.1, "nearest") == [240, 240, 30]      # v small: the file's bottom row
    assert pt(0.1, 0.9, "nearest") == [250, 20, 20] and pt(0.9, 0.9, "nearest") == [20, 250, 20]
    assert pt(0.0, 0.0, "nearest") == pt(-3.0, -0.5, "nearest") == [20, 20, 250]                       # exactly 0, below 0
    assert pt(1.0, 1.0, "nearest") == pt(7.0, 1.5, "nearest") == [20, 250, 20]                         # exactly 1, above 1
    assert pt(0.25, 0.25, "linear") == [20, 20, 250] and pt(0.75, 0.75, "linear") == [20, 250, 20]     # texel centres
    assert pt(0.5, 0.25, "linear") == [130, 130, 140] and pt(0.25, 0.5, "linear") == [135, 20, 135]
    assert pt(0.0, 0.0, "linear") == pt(-1.0, -1.0, "linear") == [20, 20, 250]                         # clamp-to-edge
    assert pt(0.5, 0.5, "linear") == [132.5, 132.5, 80.0]


# ---- the ABI (nothing launches) ---------------------------------------------------------------------------------------------------------
def test_entry_points_and_their_argument_checks():
    from checkerpose_amd import _abi
    lib = _abi.load()
    assert lib.cp_version() >= 230
    header = open(os.path.join(HERE, "..", "include", "checkerpose_hip.h")).read()
    for name in ("cp_render_rgb_tex", "cp_vis_poses_tex", "cp_render_scene_tex"):
        assert name in _abi.SIGNATURES and hasattr(lib, name) and ("int %s(" % name) in header
        plain = _abi.SIGNATURES[name[:-4]][1]
        assert _abi.SIGNATURES[name][1] == plain + [C.c_void_p] * 4 + [C.c_int]      # the old arguments plus uv, texels, tex_off, tex_dims, filter
    INVALID, ALIGN, RANGE = -1, -3, -4
    buf = (C.c_double * 64)()
    a = C.addressof(buf)                                              # host memory: never dereferenced by a refused call
    a16 = (a + 15) & ~15
    vec = (C.c_double * 3)(0.5, 0.5, 0.5)
    off = (C.c_int32 * 3)(0, 1, 2)
    order = (C.c_int32 * 2)(0, 1)

    def rgb(W=8, B=1, uv=a, texels=a, toff=a, dims=a, filt=0):
        return lib.cp_render_rgb_tex(None, a, a, 0, a, a, a, a, 1, None, a, a, vec, vec, 0.5, vec, 1, 1, 0, 8, W, B, 4, a, None, None, None, a, a16,
                                     uv, texels, toff, dims, filt)

    def vis(W=8, B=2, uv=a, texels=a, toff=a, dims=a, filt=0):
        return lib.cp_vis_poses_tex(None, a, a, 0, a, a, a, a, 1, None, a, a, None, a, a, a, off, order, a, 1, 0.5, vec, vec, 1, 1, 8, W, B, 2, 4, a, a, a,
                                    a, a, a16, uv, texels, toff, dims, filt)

    def scn(W=8, B=2, uv=a, texels=a, toff=a, dims=a, filt=0):
        return lib.cp_render_scene_tex(None, a, a, 0, a, a, a, a, 1, None, a, a, None, a, a, a, off, order, None, 0, None, vec, 1, 0.5, vec, 15.0, 0, 8, W,
                                       B, 2, 4, a, a, a, a, a, a, a, a, a, a16, uv, texels, toff, dims, filt)

    for call in (rgb, vis, scn):
        for kw in (dict(uv=None), dict(texels=None), dict(toff=None), dict(dims=None), dict(uv=None, texels=None, toff=None),
                   dict(filt=2), dict(filt=-1), dict(uv=None, texels=None, toff=None, dims=None, filt=3), dict(W=0), dict(W=-1), dict(B=0)):
            assert call(**kw) == INVALID, (call.__name__, kw)
        for kw in (dict(uv=a + 2), dict(texels=a + 1), dict(toff=a + 2), dict(dims=a + 3)):
            assert call(**kw) == ALIGN, (call.__name__, kw)
        # good texture arguments pass their checks: the call reaches the size checks, which refuse a frame side of 2^24 before any launch
        assert call(W=1 << 24) == RANGE and call(W=1 << 24, filt=1) == RANGE
        assert call(W=1 << 24, uv=None, texels=None, toff=None, dims=None) == RANGE


def test_wrappers_pass_no_tables_when_a_surface_colour_overrides():
    from checkerpose_amd import metric
    m, tx = TS.tex_meshes(), TS.textures()
    ms = metric.MeshSet.from_arrays(m["quad"][0], faces=m["quad"][1], diameters=[1.0], uvs=m["quad"][2], textures=tx["t2x2"], tex_filter="linear")
    assert ms.textures_on("cpu", use=False) == (None, None, None, None, 0)
