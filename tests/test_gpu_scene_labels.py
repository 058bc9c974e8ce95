"""Row N19 on the device: cp_render_scene against the composition it replaces -- the device's OWN vis.vis_poses(resolve_visib=True,
draw_boxes=False) on black frames, then gt_info.gt_info(depth=ren_depth, return_masks=True) -- and the training batch cut from its bit
planes against targets.make_training_batch on that composition.  Every comparison is torch.equal / bit equality.

  scene        70 x 50 (3 x 2 ragged tiles), 32 x 32 and 33 x 65 frames; four images, image 1 without poses; 41 poses interleaved across
               the images: a duplicated pose (a depth tie), two spheres overlapping within delta of each other, a sphere wholly hidden
               behind a box, a box partly off the frame, one wholly in the canvas margin, one with a vertex behind the camera, a black
               surface, and image 3 with exactly 32 small triangles (bit 31 is used).  Both shadings, surface and mesh colours, one K
               for all images and a different K per image.
  exact        depth (bits), rgb where depth > 0, the background elsewhere (a row per image through bg_index, or bg_color; bgr reverses
               the channels), the six gt_info.KEYS, ok and both expanded bit planes; the same at delta = 0, where the overlapping pair
               must lose visible pixels
  crops        get_roi_mask_bits equals get_roi_batch(INTER_NEAREST) on the expanded masks: windows over every frame edge, an empty roi
  batch        scene_training_batch equals make_training_batch on the composition restricted to `kept`, entry by entry
  invariances  two calls; an image alone against its batch; grouped against interleaved poses; with and without backgrounds
  launches     the same four kernels whatever the poses"""
import numpy as np
import pytest
import torch

from tests import render_rgb_stages as RS

pytestmark = pytest.mark.gpu

NAMES = ("box", "ico80", "quad", "tri3", "halfbox")
N_IMG = 4
BG_INDEX = [2, 0, 1, 0]                                        # the background row of each image (3 rows)
SIZES = ((70, 50), (32, 32), (33, 65))
CONFIGS = [((70, 50), "phong", "surf", "shared"), ((70, 50), "flat", "mesh", "per_image"), ((32, 32), "phong", "mesh", "per_image"),
           ((32, 32), "flat", "surf", "shared"), ((33, 65), "phong", "surf", "per_image"), ((33, 65), "flat", "mesh", "shared")]
_C = {}


def mesh_set():
    from checkerpose_amd import metric
    if "ms" not in _C:
        m = RS.meshes()
        _C["ms"] = metric.MeshSet.from_arrays([m[k][0] for k in NAMES], faces=[m[k][1] for k in NAMES], colors=[m[k][2] for k in NAMES],
                                               normals=[m[k][3] for k in NAMES], diameters=[100.0] * len(NAMES))
    return _C["ms"]


def _rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene_of(size):
    """the poses of a frame size, seeded -> dict: R (P,3,3), t (P,3,1), img, mesh (P,), surf (P,3), K (3,3), Ks (4,3,3), bgs (3,H,W,3),
    names: {case: pose index}"""
    if size in _C:
        return _C[size]
    W, H = size
    rng = np.random.default_rng(1000 * W + H)
    f = 2.2 * max(W, H)
    K = np.array([[f, 0.0, W / 2.0 + 0.3], [0.0, f * 1.01, H / 2.0 - 0.2], [0.0, 0.0, 1.0]])
    at = lambda u, v, z: (z * np.linalg.solve(K, np.array([u, v, 1.0]))).tolist()      # noqa: E731  the t whose centre projects to (u, v)
    eye = np.eye(3)
    r_dup = _rot(rng)
    per_image = {
        0: [("dup_a", "ico80", r_dup, [4.0, -3.0, 380.0]), ("dup_b", "ico80", r_dup, [4.0, -3.0, 380.0]),
            ("near", "ico80", _rot(rng), [27.0, 10.0, 388.0]), ("black", "box", _rot(rng), [-28.0, 6.0, 300.0]),
            ("behind", "halfbox", _rot(rng), [0.0, 0.0, 10.0])],
        2: [("front", "box", eye, at(W / 2.0, H / 2.0, 250.0)), ("hidden", "ico80", _rot(rng), at(W / 2.0, H / 2.0, 900.0)),
            ("partly", "halfbox", _rot(rng), at(W - 3.0, H / 2.0 + 1.0, 420.0)), ("margin", "ico80", _rot(rng), at(1.6 * W, 0.5 * H, 400.0))],
        3: [("tri%02d" % k, "tri3", _rot(rng), at((k % 8 + 0.5) * W / 8.0, (k // 8 + 0.5) * H / 4.0, 2500.0 + 10.0 * k)) for k in range(31)]
           + [("tri31", "tri3", eye, at(W / 2.0, H / 2.0, 800.0))],
    }
    queues = {i: list(v) for i, v in per_image.items()}
    rows = []
    while any(queues.values()):                                      # interleave: one pose of every image that still has one, in turn
        for i in (3, 0, 2, 3):
            if queues[i]:
                rows.append((i,) + queues[i].pop(0))
    P = len(rows)
    surf = rng.uniform(0.15, 0.95, size=(P, 3))
    names = {r[1]: j for j, r in enumerate(rows)}
    surf[names["black"]] = 0.0
    Ks = np.stack([K] * N_IMG)
    for i, s in enumerate((1.0, 1.05, 0.95, 1.02)):
        Ks[i, 0, 0] *= s
        Ks[i, 1, 1] *= s
        Ks[i, 0, 2] += 0.25 * i
    bgs = rng.integers(1, 256, size=(3, H, W, 3), dtype=np.uint8)
    _C[size] = dict(R=np.stack([r[3] for r in rows]), t=np.array([r[4] for r in rows]).reshape(P, 3, 1), img=np.array([r[0] for r in rows]),
                    mesh=np.array([NAMES.index(r[2]) for r in rows]), surf=surf, K=K, Ks=Ks, bgs=bgs, names=names)
    return _C[size]


def _args(size, shading, colour, kmode, poses):
    s = scene_of(size)
    poses = list(range(len(s["img"]))) if poses is None else list(poses)
    dev = torch.device("cuda:0")
    return s, poses, dev, dict(R=torch.from_numpy(s["R"][poses]).to(dev), t=torch.from_numpy(s["t"][poses]).to(dev),
                               K=s["K"] if kmode == "shared" else s["Ks"], mesh=s["mesh"][poses].tolist(),
                               surf=s["surf"][poses] if colour == "surf" else None, img=s["img"][poses].tolist())


def scene_call(size, shading="phong", colour="surf", kmode="shared", poses=None, with_bg=True, **kw):
    from checkerpose_amd import render
    s, poses, dev, a = _args(size, shading, colour, kmode, poses)
    if with_bg:
        kw.setdefault("backgrounds", torch.from_numpy(s["bgs"]).to(dev))
        kw.setdefault("bg_index", BG_INDEX)
    kw.setdefault("image_ids", a["img"])
    kw.setdefault("n_images", N_IMG)
    kw.setdefault("cam_K", a["K"])
    return render.render_scene(a["R"], a["t"], meshes=mesh_set(), size=size, mesh_ids=a["mesh"], surf_colors=a["surf"], shading=shading, **kw)


def composition(size, shading="phong", colour="surf", kmode="shared", poses=None, delta=15.0):
    """the three-call route: vis_poses on black frames -> gt_info with its ren_depth as the sensor depth -> (vis dict, gt_info dict)"""
    from checkerpose_amd import gt_info, vis
    key = ("comp", size, shading, colour, kmode, None if poses is None else tuple(poses), delta)
    if key not in _C:
        s, poses, dev, a = _args(size, shading, colour, kmode, poses)
        W, H = size
        v = vis.vis_poses(a["R"], a["t"], a["K"], mesh_set(), torch.zeros((N_IMG, H, W, 3), dtype=torch.uint8, device=dev), image_ids=a["img"],
                          mesh_ids=a["mesh"], surf_colors=a["surf"], resolve_visib=True, draw_boxes=False, shading=shading)
        Kp = a["K"] if kmode == "shared" else a["K"][a["img"]]
        g = gt_info.gt_info(a["R"], a["t"], Kp, mesh_set(), v["ren_depth"], image_ids=a["img"], mesh_ids=a["mesh"], delta=delta, return_masks=True)
        _C[key] = (v, g)
    return _C[key]


def scene_cached(size, shading, colour, kmode):
    key = ("scene", size, shading, colour, kmode)
    if key not in _C:
        _C[key] = scene_call(size, shading, colour, kmode)
    return _C[key]


def assert_labels_equal(r, g, img, what):
    """render_scene's dict r against gt_info's dict g of the same poses (image ids img)"""
    from checkerpose_amd import gt_info, render
    for k in gt_info.KEYS + ("ok",):
        assert r[k].dtype == g[k].dtype and torch.equal(r[k], g[k]), (what, k)
    assert torch.equal(render.scene_masks(r["full_bits"], img, r["slot"]), g["mask"]), what
    assert torch.equal(render.scene_masks(r["visib_bits"], img, r["slot"]), g["mask_visib"]), what


@pytest.mark.parametrize("size,shading,colour,kmode", CONFIGS)
def test_equals_the_composition_it_replaces(size, shading, colour, kmode):
    s = scene_of(size)
    r = scene_cached(size, shading, colour, kmode)
    v, g = composition(size, shading, colour, kmode)
    what = (size, shading, colour, kmode)
    assert r["depth"].dtype == torch.float32 and torch.equal(r["depth"].view(torch.int32), v["ren_depth"].view(torch.int32)), what
    cov = (v["ren_depth"] > 0)[..., None]
    bg = torch.from_numpy(s["bgs"][BG_INDEX]).cuda()
    assert torch.equal(r["rgb"], torch.where(cov, v["ren_rgb"], bg)), what
    assert torch.equal(v["ok"].to(torch.bool), r["ok"])
    assert_labels_equal(r, g, s["img"], what)
    for k in ("full_bits", "visib_bits", "slot"):
        assert r[k].dtype == torch.int32
    # ---- the cases, read from the outputs
    n, h = s["names"], {k: x.cpu().numpy() for k, x in r.items()}
    order_in_image = lambda j: int((s["img"][:j] == s["img"][j]).sum())      # noqa: E731
    assert h["slot"].tolist() == [order_in_image(j) for j in range(len(s["img"]))]
    a, b = n["dup_a"], n["dup_b"]                                     # equal depths: the earlier owns the colour, both are visible
    assert a < b and h["px_count_visib"][a] == h["px_count_visib"][b] > 0 and h["bbox_visib"][a].tolist() == h["bbox_visib"][b].tolist()
    assert h["px_count_visib"][n["hidden"]] == 0 and h["px_count_all"][n["hidden"]] > 0 and h["px_count_valid"][n["hidden"]] > 0
    assert h["bbox_obj"][n["hidden"]].tolist() == [-1] * 4 and h["bbox_visib"][n["hidden"]].tolist() == [-1] * 4
    full = g["mask"].cpu().numpy()
    assert 0 < (full[n["partly"]] > 0).sum() < h["px_count_all"][n["partly"]]      # the canvas counts what the frame cuts off
    assert h["px_count_all"][n["margin"]] > 0 and not full[n["margin"]].any() and h["px_count_visib"][n["margin"]] == 0
    assert not h["ok"][n["behind"]] and h["px_count_all"][n["behind"]] == 0 and h["slot"][n["behind"]] == 4
    assert not ((h["full_bits"][0] >> 4) & 1).any()                   # slot 4 of image 0: never set
    assert h["px_count_visib"][n["black"]] > 0
    if colour == "surf":
        in0 = torch.from_numpy(np.nonzero(s["img"] == 0)[0]).cuda()
        only = (g["mask_visib"][n["black"]] > 0) & (g["mask_visib"][in0].sum(0) == 255)      # where only the black surface is visible
        assert only.any() and int(r["rgb"][0][only].max()) == 0
    assert h["slot"][n["tri31"]] == 31 and (h["visib_bits"][3] < 0).any() and h["px_count_visib"][n["tri31"]] > 0      # bit 31
    assert not h["depth"][1].any() and not h["full_bits"][1].any() and np.array_equal(h["rgb"][1], s["bgs"][BG_INDEX[1]])


@pytest.mark.parametrize("size", SIZES)
def test_delta_zero_and_the_plain_background(size):
    from checkerpose_amd import gt_info
    s = scene_of(size)
    r15 = scene_cached(size, "phong", "surf", "shared") if (size, "phong", "surf", "shared") in CONFIGS else scene_call(size)
    r0 = scene_call(size, delta=0.0, with_bg=False, bg_color=(0.2, 0.4, 0.6))
    _, g0 = composition(size, delta=0.0)
    assert_labels_equal(r0, g0, s["img"], (size, "delta 0"))
    near = s["names"]["near"]                                         # the pair within delta of each other: a strict front-most rule loses pixels
    assert int(r0["px_count_visib"][near]) < int(r15["px_count_visib"][near]) and int(r0["px_count_all"][near]) == int(r15["px_count_all"][near])
    for k in ("depth", "px_count_all"):
        assert torch.equal(r0[k], r15[k])
    cov = (r0["depth"] > 0)[..., None]
    flat = torch.tensor([51, 102, 153], dtype=torch.uint8, device="cuda:0")      # round(255 c)
    assert torch.equal(r0["rgb"], torch.where(cov, r15["rgb"], flat.expand_as(r15["rgb"])))
    rev = scene_call(size, delta=0.0, with_bg=False, bg_color=(0.2, 0.4, 0.6), bgr=True)
    assert torch.equal(rev["rgb"], r0["rgb"].flip(-1))
    for k in gt_info.KEYS + ("ok", "full_bits", "visib_bits", "slot", "depth"):
        assert torch.equal(rev[k], r0[k]), k
    revb = scene_call(size, bgr=True)                                 # with backgrounds: the whole picture is reversed
    assert torch.equal(revb["rgb"], r15["rgb"].flip(-1))


@pytest.mark.parametrize("size", SIZES)
def test_bit_plane_crops_equal_the_crops_of_the_expanded_masks(size):
    from checkerpose_amd import preprocess as PP
    s = scene_of(size)
    W, H = size
    r = scene_cached(*[c for c in CONFIGS if c[0] == size][0])
    _, g = composition(*[c for c in CONFIGS if c[0] == size][0])
    n = s["names"]
    # windows hanging over the left, top, right and bottom edges, one inside, one covering everything, one of a single pixel; an empty roi (None),
    # a box without width (an empty roi under crop_resize)
    boxes = [[-9, 3, 20, 14], [4, -11, 13, 22], [W - 8, 5, 19, 12], [6, H - 7, 15, 18], [3, 4, 11, 9], [-5, -6, W + 11, H + 13], [W // 2, H // 2, 1, 1],
             None, [5, 5, 0, 7]]
    picks = [n["dup_b"], n["near"], n["partly"], n["front"], n["black"], n["tri31"], n["hidden"], n["dup_a"], n["near"]]
    img, slot = s["img"][picks], r["slot"].cpu().numpy()[picks]
    for method in ("crop_square_resize", "crop_resize"):
        for crop in (16, 23):
            for bits, masks in ((r["full_bits"], g["mask"]), (r["visib_bits"], g["mask_visib"])):
                got = PP.get_roi_mask_bits(bits, slot, boxes, crop, method, img_index=img)
                want = PP.get_roi_batch(masks[picks].unsqueeze(-1).contiguous(), boxes, crop, PP.INTER_NEAREST, method)
                assert got.shape == want.shape and got.dtype == torch.uint8 and torch.equal(got, want), (size, method, crop)
                assert not got[7].any() and got[:6].any()
    zero = PP.get_roi_mask_bits(r["full_bits"], [32, -1], [boxes[5]] * 2, 16, img_index=[0, 0])      # a bit outside 0..31
    assert not zero.any()
    one = PP.get_roi_mask_bits(r["full_bits"][3], [31], [boxes[5]], 16)                                # a lone (H,W) plane
    assert torch.equal(one, PP.get_roi_mask_bits(r["full_bits"], [31], [boxes[5]], 16, img_index=[3])) and one.any()


def _batches_equal(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, k)


@pytest.mark.parametrize("size,shading,colour,kmode", [CONFIGS[0], CONFIGS[2], CONFIGS[4]])
def test_training_batch_equals_make_training_batch_on_the_composition(size, shading, colour, kmode):
    from checkerpose_amd import augment, render, targets
    s = scene_of(size)
    poses = [j for j in range(len(s["img"])) if s["img"][j] != 3]      # the 32 tiny triangles have boxes without area: no sample
    _, _, dev, a = _args(size, shading, colour, kmode, poses)
    v, g = composition(size, shading, colour, kmode, poses)
    rng = np.random.default_rng(7)
    p3 = rng.uniform(-45.0, 45.0, size=(24, 3))
    table = rng.uniform(-45.0, 45.0, size=(len(NAMES), 24, 3))
    kw = dict(crop_size_img=64, crop_size_gt=16)
    kept_want = np.nonzero(g["ok"].cpu().numpy() & (g["visib_fract"].cpu().numpy() > 0.1))[0]
    n = {k: poses.index(j) for k, j in s["names"].items() if j in poses}
    assert 4 <= len(kept_want) < len(poses) and n["hidden"] not in kept_want and n["margin"] not in kept_want and n["behind"] not in kept_want
    kd = torch.from_numpy(kept_want).to(dev)
    img = np.asarray(a["img"])[kept_want]
    frames = v["ren_rgb"][torch.from_numpy(img).to(dev)].contiguous()
    Kp = a["K"] if kmode == "shared" else a["K"][img]
    boxes = g["bbox_visib"].cpu().numpy()[kept_want]
    plan = augment.sample_plan(len(poses), np.random.default_rng(11), color_aug_prob=1.0, frame_hw=(size[1], size[0]))
    assert not plan.is_identity().all() and (plan.bg_index < 0).all()

    def ours(**more):
        return render.scene_training_batch(mesh_set(), a["mesh"], a["R"], a["t"], a["K"], size, a["img"], more.pop("p3", p3), n_images=N_IMG,
                                           surf_colors=a["surf"], shading=shading, **kw, **more)

    def theirs(p3d=p3, **more):
        return targets.make_training_batch(frames, g["mask_visib"][kd], g["mask"][kd], a["R"][kd], a["t"][kd], Kp, list(boxes), p3d, **kw, **more)

    batch, kept = ours(is_train=False)
    assert kept.dtype == np.int64 and kept.tolist() == kept_want.tolist() and len(batch) == 11
    _batches_equal(batch, theirs(is_train=False), "test")
    assert batch[1].sum() > batch[2].sum() > 0                        # the full masks hold more than the visible ones: occlusion reached the labels
    np.random.seed(5)
    batch, _ = ours(is_train=True)
    np.random.seed(5)
    _batches_equal(batch, theirs(is_train=True), "train")
    np.random.seed(6)
    batch, _ = ours(is_train=True, augment=plan)
    np.random.seed(6)
    want = theirs(is_train=True, augment=plan.select(kept_want))
    _batches_equal(batch, want, "train + colour plan")
    np.random.seed(6)
    assert not torch.equal(batch[0], ours(is_train=True)[0][0])      # the plan did something
    oid = (np.asarray(a["mesh"]) + 1)
    batch, _ = ours(is_train=False, p3=table, obj_ids=oid)
    assert len(batch) == 12
    _batches_equal(batch, theirs(p3d=table, is_train=False, obj_ids=oid[kept_want]), "obj_ids")
    none, kept0 = ours(is_train=False, visib_threshold=2.0)          # nothing passes: an empty batch, no launch fails
    assert kept0.shape == (0,) and none[0].shape[0] == 0


def _same(a, b, keys):
    return all(torch.equal(a[k], b[k]) if a[k].dtype != torch.float32 else torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in keys)


def test_outputs_do_not_depend_on_the_call_the_batch_the_order_or_the_background():
    from checkerpose_amd import gt_info
    size, cfg = (70, 50), ("flat", "mesh", "per_image")
    s = scene_of(size)
    base = scene_cached(size, *cfg)
    pixel, pose = ("rgb", "depth", "full_bits", "visib_bits"), gt_info.KEYS + ("ok", "slot")
    assert _same(scene_call(size, *cfg), base, pixel + pose)                               # two calls
    dev = torch.device("cuda:0")
    for i in range(N_IMG):                                                               # an image alone against its batch
        mine = [j for j in range(len(s["img"])) if s["img"][j] == i]
        if not mine:
            continue
        alone = scene_call(size, *cfg, poses=mine, image_ids=[0] * len(mine), n_images=1, cam_K=s["Ks"][i],
                           backgrounds=torch.from_numpy(s["bgs"][BG_INDEX[i]:BG_INDEX[i] + 1]).to(dev), bg_index=None)
        for k in pixel:
            assert torch.equal(alone[k][0], base[k][i]), (i, k)
        for k in pose:
            assert torch.equal(alone[k], base[k][torch.tensor(mine, device=dev)]), (i, k)
    grouped = sorted(range(len(s["img"])), key=lambda j: s["img"][j])                     # grouped against interleaved (stable)
    g = scene_call(size, *cfg, poses=grouped)
    assert _same(g, base, pixel)
    for k in pose:
        assert torch.equal(g[k], base[k][torch.tensor(grouped, device=dev)]), k
    plain = scene_call(size, *cfg, with_bg=False)                                      # the labels with and without backgrounds
    assert _same(plain, base, ("depth", "full_bits", "visib_bits") + pose) and not torch.equal(plain["rgb"], base["rgb"])
    same_k = scene_call(size, "flat", "mesh", "shared", cam_K=np.stack([s["K"]] * N_IMG))  # one K against the same K per image
    assert _same(same_k, scene_call(size, "flat", "mesh", "shared"), pixel + pose)


def test_the_launch_list_does_not_depend_on_the_poses():
    from checkerpose_amd import _abi
    lib = _abi.load()
    s = scene_of((70, 50))
    logs = []
    for poses in (None, [s["names"]["behind"], s["names"]["margin"]], [s["names"]["dup_a"]], [j for j in range(len(s["img"])) if s["img"][j] == 3]):
        lib.cp_kernel_log_begin()
        scene_call((70, 50), poses=poses, with_bg=poses is None)
        logs.append(lib.cp_kernel_log().decode())
    assert len(set(logs)) == 1, logs
    assert logs[0] == "scene_pose_kernel + scene_vertex_kernel + scene_tile_kernel + scene_finish_kernel", logs[0]
