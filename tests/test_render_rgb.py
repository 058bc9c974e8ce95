"""Row N14 (shaded RGB frames) without a device: the statement, its fp32 restatement, the view sampler, the ABI's argument checks.

  fixture       tests/golden/render_rgb.npz is what the maker wrote for these meshes (CRC), its matrices are the reference's own and
                equal the restated ones, every case keeps the 5 % limit on undecided pixels
  restatement   render_f32 (the device's arithmetic in numpy float32) lies in the oracle's band |u8 - v| <= 0.5 + tol_c on every decided
                pixel of every case, and its worst (|u8 - v| - 0.5) / tol_c stays under 1 / 4 (printed: the README quotes it)
  by hand       uniform colour at ambient 1.0 is exact in either shading; the axis quad under flat shading is min(1, a + cos theta)
  mutations     each of the eight mutations of the statement is caught by at least one case (printed: by which)
  sample_views  equals the recorded reference output: count and views_level exactly, R and t within 8 * 2^-53 * (1 + radius)
  render_views  the scene_gt / scene_camera structure, with the render stubbed
  ABI           cp_render_rgb's argument checks (no launch happens)"""
import ctypes as C
import json
import math
import os
import zlib

import numpy as np
import pytest

from tests import render_rgb_stages as RS

HERE = os.path.dirname(os.path.abspath(__file__))
_G = {}


def golden():
    if not _G:
        z = np.load(os.path.join(HERE, "golden", "render_rgb.npz"))
        _G["z"] = z
        _G["cases"] = json.loads(bytes(z["cases"]).decode())
        _G["views"] = json.loads(bytes(z["views"]).decode())
    return _G["z"], _G["cases"], _G["views"]


def case_args(ci, c):
    z = golden()[0]
    v, f, col, n = RS.meshes()[c["mesh"]]
    k = "%02d" % ci
    return dict(R=z["R_" + k], t=z["t_" + k], K=z["K_" + k], verts=v, faces=f, colors=col, normals=n, size=tuple(c["size"]),
                shading=c["shading"], ambient=c["ambient"], light=tuple(c["light"]), bg=tuple(c["bg"]), surf_color=c["surf_color"], ssaa=c["ssaa"])


_ORACLES = {}


def oracle(ci, c, mut=None):
    """the oracle of a case, computed once and shared (left unchanged by its users)"""
    if (ci, mut) not in _ORACLES:
        z = golden()[0]
        k = "%02d" % ci
        _ORACLES[(ci, mut)] = RS.oracle_rgb(u_mv=z["u_mv_" + k], u_nm=z["u_nm_" + k], mut=mut, **case_args(ci, c))
    return _ORACLES[(ci, mut)]


_F32 = {}


def restated(ci, c):
    if ci not in _F32:
        _F32[ci] = RS.render_f32(**case_args(ci, c))
    return _F32[ci]


def test_fixture_is_the_makers_and_its_matrices_are_the_references():
    z, cases, _ = golden()
    crc = 0
    for name in RS.MESH_NAMES:
        v, f, c, n = RS.meshes()[name]
        for a in (v, f, n) + ((c,) if c is not None else ()):
            crc = zlib.crc32(np.ascontiguousarray(a).tobytes(), crc)
    assert int(z["mesh_crc"][0]) == crc
    assert len(cases) >= 24
    for ci, c in enumerate(cases):
        k = "%02d" % ci
        u_mv, u_nm = RS.uniforms(z["R_" + k], z["t_" + k])
        assert np.array_equal(np.asarray(u_mv, dtype=np.float64), z["u_mv_" + k]), c["name"]
        assert np.allclose(u_nm, z["u_nm_" + k], rtol=1e-12, atol=1e-12), c["name"]
        if c["rendered"] and c["name"] != "coincident":
            share = RS.undecided_share(oracle(ci, c))
            assert share <= 0.05, (c["name"], share)
            assert abs(share - c["undecided"]) < 1e-5, (c["name"], share, c["undecided"])


def test_fp32_restatement_lies_in_the_band_with_a_quarter_to_spare():
    _, cases, _ = golden()
    worst, worst_case, equal_min = -np.inf, None, 1.0
    for ci, c in enumerate(cases):
        if not c["rendered"] or c["name"] == "coincident":
            continue
        img = restated(ci, c)[0]
        ok, ratio, equal, nbad = RS.check_band(img, oracle(ci, c))
        print("%-22s ratio %8.4f  equal %.4f  outside %d" % (c["name"], ratio, equal, nbad))
        assert ok, (c["name"], nbad)
        if ratio > worst:
            worst, worst_case = ratio, c["name"]
        equal_min = min(equal_min, equal)
    print("fp32 restatement: worst (|u8 - v| - 0.5) / tol_c = %.4f (%s); smallest share of pixels equal to round(v) = %.4f" % (worst, worst_case, equal_min))
    assert worst < 0.25, (worst, worst_case)


def test_restated_depth_is_the_depth_restatement_of_row_n8():
    """the walk that keeps the face gives vsd_stages.render_f32's depth, bit for bit"""
    from tests import vsd_stages as S
    _, cases, _ = golden()
    for ci, c in enumerate(cases):
        if c["rendered"] and c["ssaa"] == 1:
            a = case_args(ci, c)
            assert np.array_equal(restated(ci, c)[1], S.render_f32(a["R"], a["t"], a["K"], a["verts"], a["faces"], a["size"])), c["name"]


def test_coincident_triangles_the_smaller_index_wins():
    _, cases, _ = golden()
    ci = [i for i, c in enumerate(cases) if c["name"] == "coincident"][0]
    img, depth, face = restated(ci, cases[ci])
    assert (face >= 0).sum() > 50 and set(np.unique(face[face >= 0])) == {0}
    # face 0 is (3, 4, 5): the blue copy; ambient 1.0 -> exactly its colour
    assert (img[face >= 0] == np.array([20, 20, 250], dtype=np.uint8)).all()
    assert (img[face < 0] == 0).all()


def test_uniform_colour_at_ambient_one_is_exact_in_either_shading():
    _, cases, _ = golden()
    seen = 0
    for ci, c in enumerate(cases):
        if c["surf_color"] is not None and c["ambient"] == 1.0:
            img, depth, face = restated(ci, c)
            # 63.75 -> 64, 127.5 -> 128, 191.25 -> 191;  255 * 0.3 and 255 * 0.7 round to 76.5 and 178.5 in fp32 AND fp64: ties -> 76, 178
            want = np.round(255.0 * np.asarray(c["surf_color"])).astype(np.uint8)
            if c["name"] == "box_surf_tie":
                assert want.tolist() == [76, 26, 178]
            assert (face >= 0).sum() > 100 and (img[face >= 0] == want).all() and (img[face < 0] == 0).all(), c["name"]
            o = oracle(ci, c)
            assert (o["u8"][o["covered"] & o["decided"]] == want).all()
            seen += 1
    assert seen == 3


def test_axis_quad_under_flat_shading_is_the_closed_form():
    """a fronto-parallel quad on the optical axis, the light at the origin: light_w = min(1, a + cos(theta)), theta the angle between
    the pixel's ray and the axis -- the interpolated per-vertex v_L is NOT the pixel's own ray direction, so the closed form is
    evaluated on the interpolated vector: L = sum_i w_i l_i over the face's vertices, cos = -L_z / |L| (n = (0, 0, -1))"""
    _, cases, _ = golden()
    ci = [i for i, c in enumerate(cases) if c["name"] == "quad_axis"][0]
    c = cases[ci]
    a = case_args(ci, c)
    o = oracle(ci, c)
    W, H = a["size"]
    K, z0 = a["K"], float(a["t"][2])
    v = a["verts"].astype(np.float64)
    col = np.array([200, 120, 40]) / 255.0
    n_checked = 0
    for y in range(H):
        for x in range(W):
            if not (o["covered"][y, x] and o["decided"][y, x]):
                continue
            X, Y = (x + 0.5 - K[0, 2]) / K[0, 0] * z0, (y + 0.5 - K[1, 2]) / K[1, 1] * z0       # the point on the quad's plane
            tri = (0, 1, 2) if (X - v[0, 0]) * (v[2, 1] - v[0, 1]) - (Y - v[0, 1]) * (v[2, 0] - v[0, 0]) <= 0 else (0, 2, 3)
            P = v[list(tri)] + np.array([0.0, 0.0, z0])
            # the plane is fronto-parallel: perspective-correct weights are the 3-D barycentrics of (X, Y)
            T = np.array([[P[0, 0], P[1, 0], P[2, 0]], [P[0, 1], P[1, 1], P[2, 1]], [1.0, 1.0, 1.0]])
            w = np.linalg.solve(T, np.array([X, Y, 1.0]))
            L = sum(w[i] * (-P[i] / np.linalg.norm(P[i])) for i in range(3))
            lw = min(1.0, c["ambient"] + max(-L[2] / np.linalg.norm(L), 0.0))
            assert np.abs(o["v"][y, x] - 255.0 * lw * col).max() < 1e-9, (x, y)
            n_checked += 1
    assert n_checked > 500
    ok, ratio, equal, nbad = RS.check_band(restated(ci, c)[0], o)
    assert ok


def test_every_mutation_of_the_statement_is_caught():
    _, cases, _ = golden()
    caught = {}
    for mut in RS.MUTATIONS:
        for ci, c in enumerate(cases):
            if not c["rendered"] or c["name"] == "coincident":
                continue
            if mut == "avgfirst" and c["ssaa"] == 1:
                continue
            if mut == "norm3" and c["shading"] != "phong":
                continue
            o = oracle(ci, c, mut)
            ok, ratio, equal, nbad = RS.check_band(restated(ci, c)[0], o)
            if ok and c["surf_color"] is not None and c["ambient"] == 1.0:
                # the band is stated on the real value v; the hand-worked case is exact, so there the mutated statement's own uint8
                # frame is compared: the only place where the rule that breaks rounding ties can show
                sel = o["covered"] & o["decided"]
                nbad = int((o["u8"][sel] != restated(ci, c)[0][sel]).any(-1).sum())
                ok = nbad == 0
            if not ok:
                caught[mut] = (c["name"], nbad)
                break
    for mut in RS.MUTATIONS:
        print("mutation %-9s caught by %s" % (mut, caught.get(mut)))
    assert set(caught) == set(RS.MUTATIONS), sorted(set(RS.MUTATIONS) - set(caught))


def test_ssaa_average_is_the_integer_rule():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(8, 12, 3)).astype(np.uint8)
    a2 = RS.ssaa_average(img, 2)
    s = img.astype(np.int64).reshape(4, 2, 6, 2, 3).sum((1, 3))
    assert np.array_equal(a2, np.floor(s / 4.0 + 0.5).astype(np.uint8))
    a4 = RS.ssaa_average(img, 4)
    s = img.astype(np.int64).reshape(2, 4, 3, 4, 3).sum((1, 3))
    assert np.array_equal(a4, np.round(s / 16.0).astype(np.uint8))
    blk = np.zeros((4, 4, 3), dtype=np.uint8)
    blk[0, 0] = 8                                                     # 8 / 16 = 0.5 -> 0 (even); 24 / 16 = 1.5 -> 2
    assert RS.ssaa_average(blk, 4)[0, 0, 0] == 0
    blk[0, 1] = 16
    assert RS.ssaa_average(blk, 4)[0, 0, 0] == 2


# ---- sample_views / render_views --------------------------------------------------------------------------------------------------------
def test_sample_views_equals_the_recorded_reference_output():
    from checkerpose_amd.render import sample_views
    z, _, views = golden()
    assert len(views) == 20
    cut = 0
    for m in views:
        got, levels = sample_views(m["n"], m["radius"], tuple(m["azimuth"]), tuple(m["elev"]), m["mode"])
        R, t, lv = z[m["key"] + "_R"], z[m["key"] + "_t"], z[m["key"] + "_level"]
        assert len(got) == R.shape[0], m
        assert [int(x) for x in levels] == lv.tolist(), m
        cut += int(len(levels) > len(got))
        tol = 8.0 * 2.0 ** -53 * (1.0 + m["radius"])
        for k, vw in enumerate(got):
            assert vw["R"].shape == (3, 3) and vw["t"].shape == (3, 1)
            assert np.abs(vw["R"] - R[k]).max() <= tol and np.abs(vw["t"] - t[k]).max() <= tol, (m, k)
    assert cut >= 8                                                   # the restricted ranges cut views
    with pytest.raises(ValueError):
        sample_views(12, mode="halton")


def test_render_views_builds_bop_toolkits_structure(monkeypatch):
    import torch
    from checkerpose_amd import metric, render
    calls = []

    def fake_rgb(R, t, K, meshes, size, mesh_ids=None, **kw):
        calls.append((int(R.shape[0]), kw["ssaa"], kw["shading"]))
        return {"rgb": torch.zeros((R.shape[0], size[1], size[0], 3), dtype=torch.uint8)}

    monkeypatch.setattr(render, "render_rgb", fake_rgb)
    monkeypatch.setattr(metric, "render_depth", lambda R, t, K, meshes, size, mesh_ids=None: torch.full((R.shape[0], size[1], size[0]), 10.0))
    v, f, c, n = RS.meshes()["ico80"]
    ms = metric.MeshSet.from_arrays([v, v], faces=[f, f], colors=[c, None], normals=[n, n], diameters=[100.0, 100.0])
    K = np.array([[100.0, 0, 20], [0, 100.0, 15], [0, 0, 1]])
    out = render.render_views(ms, [5, 9], K, (40, 30), radii=[400.0, 600.0], min_n_views=42, azimuth_range=(0, math.pi), elev_range=(0, 0.5 * math.pi),
                              depth_scale=0.1, ssaa=4, shading="flat", batch=16, device="cpu")
    assert sorted(out) == [5, 9]
    views, levels = render.sample_views(42, 400.0, (0, math.pi), (0, 0.5 * math.pi))
    n1 = len(views)
    for obj_id, r in out.items():
        assert tuple(r["rgb"].shape) == (2 * n1, 30, 40, 3) and tuple(r["depth"].shape) == (2 * n1, 30, 40)
        assert float(r["depth"][0, 0, 0]) == pytest.approx(100.0)     # 10 / depth_scale
        assert sorted(r["scene_gt"]) == list(range(2 * n1)) == sorted(r["scene_camera"])
        for im_id in range(2 * n1):
            gt, cam = r["scene_gt"][im_id], r["scene_camera"][im_id]
            assert len(gt) == 1 and gt[0]["obj_id"] == obj_id and gt[0]["cam_R_m2c"].shape == (3, 3) and gt[0]["cam_t_m2c"].shape == (3, 1)
            assert np.array_equal(cam["cam_K"], K) and cam["depth_scale"] == 0.1 and cam["view_level"] == int(levels[im_id % n1])
        assert np.array_equal(r["scene_gt"][3][0]["cam_R_m2c"], views[3]["R"])
        assert np.linalg.norm(r["scene_gt"][n1][0]["cam_t_m2c"]) == pytest.approx(600.0)
    assert all(b <= 16 and s == 4 and sh == "flat" for b, s, sh in calls) and sum(b for b, _, _ in calls) == 4 * n1


def test_meshset_takes_colours_and_normals_and_stays_what_it_was_without_them():
    from checkerpose_amd import metric
    v, f, c, n = RS.meshes()["ico80"]
    plain = metric.MeshSet.from_arrays(v, faces=f, diameters=[100.0])
    assert plain.colors is None and plain.normals is None
    ms = metric.MeshSet.from_arrays([v, v, v], faces=[f, f, f], colors=[c, None, c.astype(np.float32) / 256.0], normals=[n, n, n], diameters=[1.0] * 3)
    V = v.shape[0]
    assert tuple(ms.colors.shape) == (3 * V, 3) and tuple(ms.normals.shape) == (3 * V, 3)
    assert np.array_equal(ms.colors[:V].numpy(), c.astype(np.float32) / np.float32(255.0))           # maximum > 1: divided by 255
    assert (ms.colors[V:2 * V].numpy() == 0.5).all()                                                   # no colours: grey
    assert np.array_equal(ms.colors[2 * V:].numpy(), c.astype(np.float32) / np.float32(256.0))         # already in [0, 1]: as given
    with pytest.raises(ValueError):
        metric.MeshSet.from_arrays(v, faces=f, colors=c[:-1], diameters=[1.0])
    with pytest.raises(ValueError):
        metric.MeshSet.from_arrays([v, v], faces=[f, f], normals=[n, None], diameters=[1.0, 1.0])


def test_package_exports_the_entry_points():
    import checkerpose_amd
    from checkerpose_amd import render
    for name in ("render_rgb", "sample_views", "render_views", "synthetic_batch"):
        assert getattr(checkerpose_amd, name) is getattr(render, name)


# ---- the ABI's argument checks (nothing launches) ---------------------------------------------------------------------------------------
def test_abi_argument_checks():
    from checkerpose_amd import _abi
    lib = _abi.load()
    assert lib.cp_version() >= 215
    for name in ("cp_render_rgb", "cp_render_rgb_scratch_bytes"):
        assert name in _abi.SIGNATURES and hasattr(lib, name)
    header = open(os.path.join(HERE, "..", "include", "checkerpose_hip.h")).read()
    assert "int cp_render_rgb(" in header and "size_t cp_render_rgb_scratch_bytes(int B, int Vmax);" in header
    assert lib.cp_render_rgb_scratch_bytes(0, 5) == 0 and lib.cp_render_rgb_scratch_bytes(2, -1) == 0
    assert lib.cp_render_rgb_scratch_bytes(3, 10) == 3 * 48 * 4 + 4 * 3 * 10 * 16
    assert lib.cp_render_rgb_scratch_bytes(1, 0) == 48 * 4
    INVALID, ALIGN, RANGE = -1, -3, -4                                 # CP_ERR_INVALID, CP_ERR_ALIGN, CP_ERR_RANGE
    buf = (C.c_double * 64)()
    a = C.addressof(buf)                                              # 8-byte aligned host memory: never dereferenced by a refused call
    a16 = (a + 15) & ~15
    vec = (C.c_double * 3)(0.5, 0.5, 0.5)
    nan = (C.c_double * 3)(0.5, float("nan"), 0.5)

    def call(**kw):
        p = dict(poses=a, K=a, ks=0, verts=a, voff=a, faces=a, foff=a, M=1, ids=None, colors=a, normals=a, surf=vec, light=vec, amb=0.5, bg=vec,
                 shading=1, ssaa=1, bgr=0, H=8, W=8, B=1, Vmax=4, rgb=a, depth=None, mask=None, boxes=None, ok=a, scratch=a16)
        p.update(kw)
        return lib.cp_render_rgb(None, p["poses"], p["K"], p["ks"], p["verts"], p["voff"], p["faces"], p["foff"], p["M"], p["ids"], p["colors"],
                                 p["normals"], p["surf"], p["light"], p["amb"], p["bg"], p["shading"], p["ssaa"], p["bgr"], p["H"], p["W"], p["B"],
                                 p["Vmax"], p["rgb"], p["depth"], p["mask"], p["boxes"], p["ok"], p["scratch"])

    for kw in (dict(poses=None), dict(K=None), dict(verts=None), dict(voff=None), dict(faces=None), dict(foff=None), dict(rgb=None), dict(ok=None),
               dict(scratch=None), dict(surf=None), dict(light=None), dict(bg=None), dict(B=0), dict(M=0), dict(Vmax=0), dict(H=0), dict(W=-1),
               dict(ks=3), dict(ssaa=3), dict(ssaa=0), dict(ssaa=8), dict(shading=2), dict(shading=-1), dict(shading=1, normals=None),
               dict(M=2), dict(amb=float("nan")), dict(amb=float("inf")), dict(surf=nan), dict(light=nan), dict(bg=nan),
               dict(ssaa=2, depth=a), dict(ssaa=4, mask=a), dict(ssaa=2, boxes=a)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(scratch=a16 + 8), dict(poses=a + 4), dict(K=a + 4), dict(verts=a + 2), dict(voff=a + 1), dict(faces=a + 2), dict(foff=a + 2),
               dict(M=2, ids=a + 2), dict(colors=a + 1), dict(normals=a + 2), dict(depth=a + 2), dict(boxes=a + 2)):
        assert call(**kw) == ALIGN, kw
    assert call(H=1 << 20, W=1 << 20) == RANGE
    assert call(B=1 << 20, H=640, W=640) == RANGE                      # 2^24 workgroups or more: refused before any launch


def test_python_argument_checks_without_a_device():
    from checkerpose_amd import metric, render
    v, f, c, n = RS.meshes()["ico80"]
    ms = metric.MeshSet.from_arrays(v, faces=f, colors=c, diameters=[100.0])
    R, t, K = np.eye(3)[None], np.array([[0.0, 0.0, 500.0]]), np.eye(3)
    for kw in (dict(shading="gouraud"), dict(ssaa=3), dict(ssaa=2, return_depth=True), dict(ssaa=4, return_mask=True), dict(ssaa=2, return_boxes=True),
               dict(ambient_weight=float("nan")), dict(light_cam_pos=(0, 0)), dict(bg_color=(0, float("inf"), 0)), dict(shading="phong")):
        with pytest.raises(ValueError):
            render.render_rgb(R, t, K, ms, (8, 8), **{**dict(shading="flat"), **kw})
    with pytest.raises(ValueError):
        render.render_rgb(R, t, K, ms, (0, 8), shading="flat")
    with pytest.raises(ValueError):
        render.render_rgb(R, t, K, v, (8, 8), shading="flat")
