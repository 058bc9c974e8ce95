"""Row N14 on the device: cp_render_rgb against tests/golden/render_rgb.npz and the stages of tests/render_rgb_stages.py.

  exact        ssaa = 1: the depth is metric.render_depth's bits, the mask is 255 * (depth > 0), the boxes are numpy's of the mask;
               ssaa = f equals the integer rule applied on the host to the ssaa = 1 render at (f W, f H) under K * f (f = 2, 4);
               coincident triangles give the smaller index's colour; a uniform colour at ambient 1.0 is that colour
  band         every decided pixel of every case satisfies |u8 - v| <= 0.5 + tol_c (the derived bound of the stages; with SSAA its
               integer form), undecided pixels take a value some candidate surface or the background allows; the worst ratio and
               the share of pixels equal to round(v) outright are printed
  invariances  bit-identical across two calls, alone / in a mixed batch, shared / repeated K, with / without each optional output, out=,
               bgr = the channel flip
  launches     the same launch list whatever the poses are
  synthetic_batch   equals the manual render_rgb -> make_training_batch composition; with an identity colour plan and change_bg the
               crop shows the render under the mask and the pool elsewhere

Measured on an MI355X (the figures the README quotes): see README.md, status block "row N14"."""
import numpy as np
import pytest
import torch

from tests import render_rgb_stages as RS
from tests.test_render_rgb import case_args, golden, oracle

pytestmark = pytest.mark.gpu

_MS = {}


def mesh_set():
    from checkerpose_amd import metric
    if "ms" not in _MS:
        names = list(RS.MESH_NAMES)
        m = RS.meshes()
        _MS["ms"] = metric.MeshSet.from_arrays([m[k][0] for k in names], faces=[m[k][1] for k in names], colors=[m[k][2] for k in names],
                                                normals=[m[k][3] for k in names], diameters=[100.0] * len(names))
        _MS["ids"] = {k: i for i, k in enumerate(names)}
    return _MS["ms"], _MS["ids"]


def render_case(ci, c, **kw):
    from checkerpose_amd import render
    ms, ids = mesh_set()
    a = case_args(ci, c)
    args = dict(mesh_ids=[ids[c["mesh"]]], shading=a["shading"], ambient_weight=a["ambient"], light_cam_pos=a["light"], bg_color=a["bg"],
                surf_color=a["surf_color"], ssaa=a["ssaa"])
    args.update(kw)
    dev = torch.device("cuda:0")
    return render.render_rgb(torch.from_numpy(a["R"][None]).to(dev), torch.from_numpy(a["t"][None]).to(dev), a["K"], ms, a["size"], **args)


_DEV = {}


def device_frame(ci, c):
    """the device's frame of a case, rendered once and shared"""
    if ci not in _DEV:
        r = render_case(ci, c)
        _DEV[ci] = (r["rgb"][0].cpu().numpy(), int(r["ok"][0]))
    return _DEV[ci]


def np_box(mask):
    ys, xs = np.nonzero(mask)
    return [-1, -1, -1, -1] if ys.size == 0 else [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]


def test_depth_mask_and_boxes_are_exact_at_ssaa_1():
    from checkerpose_amd import metric
    ms, ids = mesh_set()
    _, cases, _ = golden()
    dev = torch.device("cuda:0")
    n = 0
    for ci, c in enumerate(cases):
        if c["ssaa"] != 1:
            continue
        a = case_args(ci, c)
        r = render_case(ci, c, return_depth=True, return_mask=True, return_boxes=True)
        d = metric.render_depth(torch.from_numpy(a["R"][None]).to(dev), torch.from_numpy(a["t"][None]).to(dev), a["K"], ms, a["size"],
                                mesh_ids=[ids[c["mesh"]]])
        assert torch.equal(r["depth"].view(torch.int32), d.view(torch.int32)), c["name"]
        mask = r["mask"][0].cpu().numpy()
        assert np.array_equal(mask, 255 * (d[0].cpu().numpy() > 0).astype(np.uint8)), c["name"]
        assert r["boxes"][0].cpu().tolist() == np_box(mask), c["name"]
        assert int(r["ok"][0]) == (1 if c["rendered"] else 0), c["name"]
        if not c["rendered"]:
            bgq = np.round(255.0 * np.float32(np.asarray(c["bg"], dtype=np.float32))).astype(np.uint8)
            assert (r["rgb"][0].cpu().numpy() == bgq).all() and not mask.any()
        n += 1
    assert n >= 20


@pytest.mark.parametrize("f", [2, 4])
def test_ssaa_equals_the_integer_rule_on_the_plain_render(f):
    _, cases, _ = golden()
    for name in ("tri3_phong_s2", "ico80_flat_s4", "box_left_a0", "ico1280_phong"):
        ci = [i for i, c in enumerate(cases) if c["name"] == name][0]
        c = cases[ci]
        a = case_args(ci, c)
        W, H = a["size"]
        Kf = a["K"].copy()
        Kf[:2] *= f
        from checkerpose_amd import render
        ms, ids = mesh_set()
        dev = torch.device("cuda:0")
        big = render.render_rgb(torch.from_numpy(a["R"][None]).to(dev), torch.from_numpy(a["t"][None]).to(dev), Kf, ms, (f * W, f * H),
                                mesh_ids=[ids[c["mesh"]]], shading=a["shading"], ambient_weight=a["ambient"], light_cam_pos=a["light"],
                                bg_color=a["bg"], surf_color=a["surf_color"], ssaa=1)["rgb"][0].cpu().numpy()
        small = render_case(ci, c, ssaa=f)["rgb"][0].cpu().numpy()
        assert np.array_equal(small, RS.ssaa_average(big, f)), (name, f)


def test_coincident_triangles_and_the_uniform_colour_are_exact():
    _, cases, _ = golden()
    seen = 0
    for ci, c in enumerate(cases):
        if c["name"] == "coincident":
            r = render_case(ci, c, return_mask=True)
            img, m = r["rgb"][0].cpu().numpy(), r["mask"][0].cpu().numpy() > 0
            assert m.sum() > 50 and (img[m] == np.array([20, 20, 250], dtype=np.uint8)).all() and (img[~m] == 0).all()
            seen += 1
        elif c["surf_color"] is not None and c["ambient"] == 1.0:
            r = render_case(ci, c, return_mask=True)
            img, m = r["rgb"][0].cpu().numpy(), r["mask"][0].cpu().numpy() > 0
            want = np.round(255.0 * np.asarray(c["surf_color"])).astype(np.uint8)
            assert m.sum() > 100 and (img[m] == want).all() and (img[~m] == 0).all(), c["name"]
            seen += 1
    assert seen == 4


def test_every_decided_pixel_lies_in_the_band():
    """Measured: see the README's row N14 block (worst ratio, share of pixels equal to round(v))."""
    _, cases, _ = golden()
    worst, worst_case, equal_min, n_equal, n_dec = -np.inf, None, 1.0, 0.0, 0
    for ci, c in enumerate(cases):
        if not c["rendered"] or c["name"] == "coincident":
            continue
        img, ok_flag = device_frame(ci, c)
        assert ok_flag == 1
        o = oracle(ci, c)
        ok, ratio, equal, nbad = RS.check_band(img, o)
        print("%-22s ratio %8.4f  equal %.4f  outside %d" % (c["name"], ratio, equal, nbad))
        assert ok, (c["name"], nbad)
        if ratio > worst:
            worst, worst_case = ratio, c["name"]
        equal_min = min(equal_min, equal)
        n_equal += equal * int(o["decided"].sum())
        n_dec += int(o["decided"].sum())
    print("device: worst (|u8 - v| - 0.5) / tol_c = %.4f (%s); pixels equal to round(v): %.5f overall, %.4f in the worst case"
          % (worst, worst_case, n_equal / n_dec, equal_min))
    assert worst <= 1.0


def test_bitwise_invariances():
    from checkerpose_amd import render
    ms, ids = mesh_set()
    _, cases, _ = golden()
    dev = torch.device("cuda:0")
    pick = [i for i, c in enumerate(cases) if tuple(c["size"]) == (67, 45) and c["ssaa"] == 1 and c["shading"] == "phong" and c["ambient"] == 0.5
            and c["surf_color"] is None and c["bg"] == [0, 0, 0] and c["light"] == [0, 0, 0]]
    assert len(pick) >= 4
    R = torch.from_numpy(np.stack([golden()[0]["R_%02d" % i] for i in pick])).to(dev)
    t = torch.from_numpy(np.stack([golden()[0]["t_%02d" % i] for i in pick])).to(dev)
    K = torch.from_numpy(np.stack([golden()[0]["K_%02d" % i] for i in pick])).to(dev)
    mids = [ids[cases[i]["mesh"]] for i in pick]
    full = render.render_rgb(R, t, K, ms, (67, 45), mesh_ids=mids, return_depth=True, return_mask=True, return_boxes=True)
    again = render.render_rgb(R, t, K, ms, (67, 45), mesh_ids=mids, return_depth=True, return_mask=True, return_boxes=True)
    for k in full:
        assert torch.equal(full[k], again[k]), k
    for j, i in enumerate(pick):                                       # alone = in the mixed batch = the fixture's frame
        assert np.array_equal(full["rgb"][j].cpu().numpy(), device_frame(i, cases[i])[0]), cases[i]["name"]
    same_k = [j for j, i in enumerate(pick) if np.array_equal(golden()[0]["K_%02d" % i], golden()[0]["K_%02d" % pick[0]])]
    shared = render.render_rgb(R[same_k], t[same_k], K[0], ms, (67, 45), mesh_ids=[mids[j] for j in same_k])
    assert torch.equal(shared["rgb"], full["rgb"][same_k])
    for opt in ("return_depth", "return_mask", "return_boxes"):
        one = render.render_rgb(R, t, K, ms, (67, 45), mesh_ids=mids, **{opt: True})
        key = opt[len("return_"):]
        assert torch.equal(one["rgb"], full["rgb"]) and torch.equal(one[key], full[key]) and torch.equal(one["ok"], full["ok"])
    plain = render.render_rgb(R, t, K, ms, (67, 45), mesh_ids=mids)
    assert torch.equal(plain["rgb"], full["rgb"])
    buf = torch.full((len(pick), 45, 67, 3), 7, dtype=torch.uint8, device=dev)
    into = render.render_rgb(R, t, K, ms, (67, 45), mesh_ids=mids, out=buf)
    assert into["rgb"] is buf and torch.equal(buf, full["rgb"])
    bgr = render.render_rgb(R, t, K, ms, (67, 45), mesh_ids=mids, bgr=True)
    assert torch.equal(bgr["rgb"], full["rgb"].flip(-1))
    host = render.render_rgb(R.cpu().numpy(), t.cpu().numpy(), K.cpu().numpy(), ms, (67, 45), mesh_ids=mids)       # arrays as well as tensors
    assert torch.equal(host["rgb"], full["rgb"])


def test_the_launch_list_does_not_depend_on_the_poses():
    from checkerpose_amd import _abi, render
    lib = _abi.load()
    ms, ids = mesh_set()
    _, cases, _ = golden()
    dev = torch.device("cuda:0")
    logs = []
    for name in ("box_phong", "box_outside", "box_behind", "box_corner_a1"):
        ci = [i for i, c in enumerate(cases) if c["name"] == name][0]
        a = case_args(ci, cases[ci])
        R, t = torch.from_numpy(a["R"][None]).to(dev), torch.from_numpy(a["t"][None]).to(dev)
        lib.cp_kernel_log_begin()
        render.render_rgb(R, t, a["K"], ms, (67, 45), mesh_ids=[ids["box"]], shading="flat", ssaa=2)
        logs.append(lib.cp_kernel_log().decode())
    assert len(set(logs)) == 1 and logs[0].count("rgb_") == 4, logs
    for k in ("rgb_pose_kernel", "rgb_vertex_kernel", "rgb_tile_kernel", "rgb_finish_kernel"):
        assert k in logs[0]


def test_synthetic_batch_is_the_manual_composition():
    from checkerpose_amd import augment, render, targets
    ms, ids = mesh_set()
    _, cases, _ = golden()
    dev = torch.device("cuda:0")
    pick = [i for i, c in enumerate(cases) if c["name"] in ("box_phong", "ico1280_phong", "grey_phong")]
    z = golden()[0]
    R = torch.from_numpy(np.stack([z["R_%02d" % i] for i in pick])).to(dev)
    t = torch.from_numpy(np.stack([z["t_%02d" % i] for i in pick])).to(dev)
    K = z["K_%02d" % pick[0]]
    mids = [ids[cases[i]["mesh"]] for i in pick]
    B = len(pick)
    p3d = torch.from_numpy(np.stack([RS.meshes()["ico80"][0][:32]] * B)).to(dev)
    np.random.seed(5)
    got = render.synthetic_batch(ms, mids, R, t, K, (67, 45), p3d, shading="phong", ambient_weight=0.5)
    r = render.render_rgb(R, t, K, ms, (67, 45), mesh_ids=mids, shading="phong", ambient_weight=0.5, return_mask=True, return_boxes=True)
    np.random.seed(5)
    want = targets.make_training_batch(r["rgb"], r["mask"], r["mask"], R, t, K, r["boxes"].cpu().numpy(), p3d, img_index=np.arange(B))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # an identity colour plan with the background swap: the render under the mask, the pool elsewhere
    pool = torch.randint(0, 256, (2, 45, 67, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
    plan = augment.sample_plan(B, np.random.default_rng(3), color_aug_prob=0.0, change_bg=np.ones(B, dtype=bool), n_bg=2, frame_hw=(45, 67))
    np.random.seed(5)
    aug = render.synthetic_batch(ms, mids, R, t, K, (67, 45), p3d, augment=plan, backgrounds=pool, shading="phong", ambient_weight=0.5)
    for a, b in zip(aug[1:], want[1:]):
        assert torch.equal(a, b)                                       # only roi_x differs
    bg = pool[torch.from_numpy(np.asarray(plan.bg_index, dtype=np.int64)).to(dev)]
    composed = torch.where((r["mask"] > 0)[..., None], r["rgb"], bg)
    np.random.seed(5)
    manual = targets.make_training_batch(composed, r["mask"], r["mask"], R, t, K, r["boxes"].cpu().numpy(), p3d, img_index=np.arange(B))
    assert torch.equal(aug[0], manual[0]) and not torch.equal(aug[0], want[0])
