"""Row N19 (occluded multi-object training scenes with labels) on the CPU: the refusals of checkerpose_amd/render.py's scene calls, the
entry points' argument, CSR and 32-pose checks with fake pointers, the scratch queries and the library version, scene_masks and the
slot rule on hand-made planes (bit 31 included), sample_scene_poses, and the `kept` filter."""
import ctypes as C

import numpy as np
import pytest
import torch

from checkerpose_amd import augment, preprocess, render, scene


def _mesh_set():
    from checkerpose_amd import metric
    from tests import render_rgb_stages as RS
    m = RS.meshes()
    return metric.MeshSet.from_arrays([m["box"][0]], faces=[m["box"][1]], colors=[m["box"][2]], normals=[m["box"][3]], diameters=[100.0])


def _poses(P):
    return np.eye(3)[None].repeat(P, 0), np.array([[0.0, 0.0, 500.0]] * P), np.array([[500.0, 0, 20], [0, 500.0, 16], [0, 0, 1]])


def test_package_names_and_version(lib):
    import checkerpose_amd
    assert lib.cp_version() >= 220
    for n in ("render_scene", "scene_masks", "scene_training_batch", "sample_scene_poses"):
        assert getattr(checkerpose_amd, n) is getattr(render, n)
    assert render.MAX_SCENE_POSES == 32


def test_refusals_are_value_errors_and_there_is_no_cpu_fallback():
    ms = _mesh_set()
    R, t, K = _poses(3)
    bgs = torch.zeros((2, 32, 40, 3), dtype=torch.uint8)
    good = dict(R=R, t=t, cam_K=K, meshes=ms, size=(40, 32), image_ids=[0, 1, 0])
    for kw in (dict(size=(0, 32)), dict(size=(40, -1)), dict(image_ids=[0, 1]), dict(image_ids=[0, -1, 0]), dict(image_ids=None),
               dict(image_ids=[0, 2, 0], n_images=2), dict(n_images=0), dict(shading="gouraud"), dict(meshes="box"), dict(delta=float("nan")),
               dict(bg_color=(0.1, float("inf"), 0.2)), dict(bg_color=(0.1, 0.2)), dict(ambient_weight=float("nan")), dict(light_cam_pos=(0, 0)),
               dict(surf_colors=[[0.5, float("nan"), 0.5]] * 3), dict(surf_colors=[[0.1, 0.2, 0.3]] * 2),
               dict(bg_index=[0, 1]),                                              # an index without backgrounds
               dict(backgrounds=bgs, bg_index=[0]), dict(backgrounds=bgs, bg_index=[0, 2]), dict(backgrounds=bgs, bg_index=[0, -1]),      # mismatched
               dict(backgrounds=bgs, n_images=3),                                  # 2 rows for 3 images: which row?
               dict(backgrounds=bgs[:, :31]), dict(backgrounds=bgs[..., :2]), dict(backgrounds=bgs.float()), dict(backgrounds=np.zeros((2, 32, 40, 3)))):
        a = dict(good)
        a.update(kw)
        with pytest.raises(ValueError):
            render.render_scene(**a)
    with pytest.raises(ValueError):
        render.render_scene(R[:0], t[:0], K, ms, (40, 32), [])                   # no poses
    R33, t33, _ = _poses(34)
    with pytest.raises(ValueError, match="at most 32"):                           # 33 poses in one image
        render.render_scene(R33, t33, K, ms, (40, 32), [0] * 33 + [1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                    # 32 are fine, and then a device is asked for
        render.render_scene(R33, t33, K, ms, (40, 32), [0] * 32 + [1] * 2)
    for a in (dict(good), dict(good, R=torch.from_numpy(R), t=torch.from_numpy(t)), dict(good, backgrounds=bgs)):      # CPU tensors
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            render.render_scene(**a)
    p3 = np.zeros((8, 3))
    swap = augment.sample_plan(3, np.random.default_rng(0), change_bg=np.array([False, True, False]), n_bg=2, frame_hw=(32, 40))
    with pytest.raises(ValueError, match="swaps backgrounds"):                    # a swap-asking plan
        render.scene_training_batch(ms, None, R, t, K, (40, 32), [0, 1, 0], p3, augment=swap)
    colour = augment.sample_plan(2, np.random.default_rng(0), frame_hw=(32, 40))
    with pytest.raises(ValueError, match="one sample per pose"):
        render.scene_training_batch(ms, None, R, t, K, (40, 32), [0, 1, 0], p3, augment=colour)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render.scene_training_batch(ms, None, R, t, K, (40, 32), [0, 1, 0], p3)
    bits = torch.zeros((2, 32, 40), dtype=torch.int32)
    for bad in (bits, bits.to(torch.uint8), "bits"):
        with pytest.raises(RuntimeError, match="no CPU path"):
            preprocess.get_roi_mask_bits(bad, [0], [[1, 2, 8, 8]], 16, img_index=[0])


def test_kept_follows_ok_and_the_strict_threshold():
    ok = np.array([1, 1, 0, 1, 1, 1], dtype=bool)
    fract = np.array([0.1, np.nextafter(0.1, 1.0), 0.9, 0.0, 1.0, 0.05])
    kept = render.scene_kept(ok, fract, 0.1)
    assert kept.dtype == np.int64 and kept.tolist() == [1, 4]                     # 0.1 itself does not pass; a pose that is not rendered never does
    assert render.scene_kept(ok, fract, 0.0).tolist() == [0, 1, 4, 5] and render.scene_kept(ok, fract, 1.0).tolist() == []
    assert render.scene_kept(torch.tensor([1, 0], dtype=torch.uint8).numpy(), [0.5, 0.5], 0.1).tolist() == [0]


def test_scene_masks_and_the_slot_rule_on_hand_made_planes():
    bits = torch.zeros((3, 4, 5), dtype=torch.int32)
    bits[0, 1, 2] = 0b101                                                         # slots 0 and 2 of image 0
    bits[0, 3, 4] = -(1 << 31)                                                    # bit 31 alone (the int32 view of 0x80000000)
    bits[0, 0, 0] = -1                                                            # every bit
    bits[2, 2, 2] = (1 << 30) | 2
    image_ids, slot = [0, 2, 0, 0, 2, 0, 0], [0, 1, 2, 31, 30, 1, -1]
    m = render.scene_masks(bits, image_ids, slot)
    assert m.dtype == torch.uint8 and tuple(m.shape) == (7, 4, 5) and set(m.unique().tolist()) <= {0, 255}
    set_at = lambda j: sorted((int(y), int(x)) for y, x in torch.nonzero(m[j]))      # noqa: E731
    assert set_at(0) == [(0, 0), (1, 2)] and set_at(2) == [(0, 0), (1, 2)] and set_at(3) == [(0, 0), (3, 4)]
    assert set_at(1) == [(2, 2)] and set_at(4) == [(2, 2)] and set_at(5) == [(0, 0)] and set_at(6) == []      # slot -1: no mask
    assert torch.equal(render.scene_masks(bits, torch.tensor(image_ids), torch.tensor(slot, dtype=torch.int32)), m)
    for bad in (dict(bits=bits.float()), dict(bits=bits[0]), dict(image_ids=[0, 1]), dict(image_ids=[0, 3, 0, 0, 2, 0, 0])):
        a = dict(bits=bits, image_ids=image_ids, slot=slot)
        a.update(bad)
        with pytest.raises(ValueError):
            render.scene_masks(**a)
    # the slot rule is scene.group_by_image's: the rank among the poses of the image, in the order given
    ids, off, order = scene.group_by_image([2, 0, 2, 3, 0, 2], 6, 5)
    rank = np.empty(6, dtype=np.int64)
    for i in range(5):
        rank[order[off[i]:off[i + 1]]] = np.arange(off[i + 1] - off[i])
    assert rank.tolist() == [0, 0, 1, 0, 1, 2]


def test_sample_scene_poses_is_seeded_and_well_formed():
    K = np.array([[600.0, 0.0, 320.5], [0.0, 605.0, 239.5], [0.0, 0.0, 1.0]])
    Ks = np.stack([K, K * np.array([[1.1], [0.9], [1.0]])])
    for cam, n_img in ((K, 5), (Ks, 2)):
        a = render.sample_scene_poses(np.random.default_rng(3), n_img, 8, cam, (640, 480), (400.0, 900.0), 4)
        b = render.sample_scene_poses(np.random.default_rng(3), n_img, 8, cam, (640, 480), (400.0, 900.0), 4)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))                    # the same seed gives the same arrays
        R, t, image_ids, mesh_ids = a
        P = 8 * n_img
        assert R.shape == (P, 3, 3) and t.shape == (P, 3, 1) and R.dtype == np.float64 and t.dtype == np.float64
        assert image_ids.dtype == np.int32 and mesh_ids.dtype == np.int32 and image_ids.tolist() == [j % n_img for j in range(P)]
        assert mesh_ids.min() >= 0 and mesh_ids.max() < 4 and len(set(mesh_ids.tolist())) > 1
        assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(R) - 1.0).max() < 1e-12
        Kp = np.broadcast_to(cam, (n_img, 3, 3))[image_ids]
        uvw = (Kp @ t)[:, :, 0]
        u, v = uvw[:, 0] / uvw[:, 2], uvw[:, 1] / uvw[:, 2]
        assert (u >= -1e-9).all() and (u <= 640 + 1e-9).all() and (v >= -1e-9).all() and (v <= 480 + 1e-9).all()      # centres inside the frame
        assert (t[:, 2, 0] >= 400.0).all() and (t[:, 2, 0] <= 900.0).all()
    c = render.sample_scene_poses(np.random.default_rng(4), 5, 8, K, (640, 480), (400.0, 900.0), 4)
    assert not np.array_equal(c[0], a[0][:40])
    for bad in (dict(n_images=0), dict(objects_per_image=33), dict(objects_per_image=0), dict(z_range=(0.0, 5.0)), dict(z_range=(9.0, 5.0)),
                dict(n_meshes=0), dict(cam_K=np.zeros((3, 3, 3))), dict(size=(0, 480))):
        kw = dict(rng=np.random.default_rng(0), n_images=2, objects_per_image=3, cam_K=K, size=(640, 480), z_range=(400.0, 900.0), n_meshes=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            render.sample_scene_poses(**kw)


def test_entry_points_refuse_bad_arguments_before_any_launch(lib):
    """fake, never-dereferenced device pointers; the CSR copies are real host memory (they are read)"""
    A, P, n_img = 0x10000, 5, 3
    off, order = (C.c_int32 * 4)(0, 2, 2, 5), (C.c_int32 * 5)(0, 3, 1, 2, 4)
    vec = (C.c_double * 3)(0.3, 0.3, 0.3)
    names = ("poses", "K", "ks", "verts", "v_off", "faces", "f_off", "M", "mesh_ids", "colors", "normals", "surf", "iop", "img_off", "order", "off_h", "order_h",
             "bgs", "n_bg", "bg_index", "bg_color", "shading", "amb", "light", "delta", "bgr", "H", "W", "P", "I", "Vmax", "rgb", "depth", "full", "visib", "slot",
             "counts", "fract", "boxes", "ok", "scratch")
    good = dict(zip(names, (A, A, 0, A, A, A, A, 2, A, A, A, A, A, A, A, off, order, A, 3, A, vec, 1, 0.5, vec, 15.0, 0, 40, 48, P, n_img, 12, A, A, A, A, A,
                            A, A, A, A, A)))
    assert len(names) == len(good) == 41

    def call(**kw):
        a = dict(good)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = lib.cp_render_scene(None, *[a[n] for n in names])
        assert lib.cp_kernel_log() == b"", kw
        return rc

    for n in ("poses", "K", "verts", "v_off", "faces", "f_off", "iop", "img_off", "order", "off_h", "order_h", "bg_color", "light", "rgb", "depth", "full",
              "visib", "slot", "counts", "fract", "boxes", "ok", "scratch", "normals", "mesh_ids", "bgs"):
        assert call(**{n: None}) == -1, n
    for kw in (dict(P=0), dict(I=0), dict(M=0), dict(Vmax=0), dict(H=0), dict(W=-1), dict(ks=4), dict(shading=2), dict(bgr=2), dict(bgr=-1),
               dict(amb=float("nan")), dict(amb=float("inf")), dict(delta=float("nan")), dict(light=(C.c_double * 3)(0, float("nan"), 0)),
               dict(bg_color=(C.c_double * 3)(0, 0, float("inf"))), dict(n_bg=0), dict(n_bg=-2), dict(n_bg=2, bg_index=None),
               dict(bgs=None, bg_index=None, n_bg=1), dict(bgs=None, n_bg=0)):
        assert call(**kw) == -1, kw
    for kw in (dict(scratch=A + 8), dict(poses=A + 4), dict(surf=A + 4), dict(fract=A + 4), dict(verts=A + 2), dict(depth=A + 2), dict(full=A + 2),
               dict(visib=A + 1), dict(slot=A + 2), dict(counts=A + 2), dict(boxes=A + 1), dict(iop=A + 2), dict(bg_index=A + 2)):
        assert call(**kw) == -3, kw
    for bad in ((1, 2, 2, 5), (0, 2, 2, 4), (0, 3, 2, 5), (0, 2, 2, 6)):
        assert call(off_h=(C.c_int32 * 4)(*bad)) == -1, bad
    for bad in ((0, 3, 1, 2, 5), (0, -1, 1, 2, 4)):
        assert call(order_h=(C.c_int32 * 5)(*bad)) == -1, bad
    order34 = (C.c_int32 * 34)(*range(34))
    assert call(P=34, I=2, n_bg=2, order_h=order34, off_h=(C.c_int32 * 3)(0, 33, 34)) == -4          # 33 poses in one image
    assert call(P=34, I=2, n_bg=2, order_h=order34, off_h=(C.c_int32 * 3)(0, 32, 34), W=1 << 24) == -4      # 32 pass that check; the size stops it
    assert call(W=1 << 24) == -4
    assert call(H=4096, W=4096, I=64, n_bg=1, off_h=(C.c_int32 * 65)(*([0] + [P] * 64))) == -4       # 3 I H W >= 2^31
    assert call(H=16384, W=16384, I=1, n_bg=1, off_h=(C.c_int32 * 2)(0, P)) == -4                    # a canvas of 9 H W >= 2^31 pixels
    assert lib.cp_render_scene_scratch_bytes(5, 12, 3) == 5 * 64 * 4 + 4 * 5 * 12 * 16
    assert lib.cp_render_scene_scratch_bytes(3, 7, 1) == 3 * 64 * 4 + 4 * 3 * 7 * 16
    assert lib.cp_render_scene_scratch_bytes(0, 12, 3) == 0 and lib.cp_render_scene_scratch_bytes(5, -1, 3) == 0
    assert lib.cp_render_scene_scratch_bytes(5, 12, 0) == 0
    assert lib.cp_vis_poses_scratch_bytes(5, 12, 3) == 5 * 48 * 4 + 4 * 5 * 12 * 16                  # the composition's, for comparison: unchanged

    def crop(**kw):
        a = dict(plane=A, n_img=2, H=40, W=48, win=A, idx=A, bit=A, out=A, B=3, crop=64)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = lib.cp_crop_mask_bits(None, *[a[n] for n in ("plane", "n_img", "H", "W", "win", "idx", "bit", "out", "B", "crop")])
        assert lib.cp_kernel_log() == b"", kw
        return rc

    for n in ("plane", "win", "bit", "out", "idx"):
        assert crop(**{n: None}) == -1, n                                                             # (no idx: 2 planes for 3 crops)
    for kw in (dict(n_img=0), dict(H=0), dict(W=-1), dict(B=0), dict(crop=0)):
        assert crop(**kw) == -1, kw
    for kw in (dict(plane=A + 2), dict(win=A + 1), dict(idx=A + 2), dict(bit=A + 2)):
        assert crop(**kw) == -3, kw
    assert crop(n_img=1, H=65536, W=65536) == -4
