"""Row N21 on the host: the affine map of "crop_resize_by_warp_affine" against what the reference's own code handed to cv2
(tests/golden/warp_affine.npz, written by tests/golden/make_golden_warp.py), the numpy restatement of cv2.warpAffine
(tests/warp_stages.py) against properties that do not come from it, and the mistakes those properties must catch.

  golden      the float32 point triples of get_affine_transform EQUAL the recorded ones bit for bit (66 boxes through get_roi, 38 direct
              calls: rotations, shifts, inv, scalar / pair arguments); scale, centre and final box EQUAL the recorded ones; the product's
              matrix maps the recorded src triple onto the dst triple to within 1e-9 px (float64 on coordinates below 4096: about 1e-12)
  properties  plain slices, (a + b + 1) >> 1 at a half-pixel centre, np.rot90 at quarter turns, the bilinear bound 0.5 + 2 (1/64 + 1/512) G,
              and two hand-worked double roundings (see below)
  mutations   a half-pixel shift, a wrong rd, truncation in place of rint, clamp-to-edge in place of the zero border: each breaks at
              least one property.  Truncation cannot break the first four: their coordinates are multiples of 1/2 pixel, which the
              fixed point holds exactly, and in the bound it moves a coordinate by less than 2/1024 -- the slack the bound leaves.  The
              hand-worked double roundings (warp_stages.double_rounding_fail) are there to catch it."""
import os

import numpy as np
import pytest

from tests import warp_stages as WS
from tests.common import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "warp_affine.npz"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _maps(M, src, dst):
    got = np.asarray(src, dtype=np.float64) @ M[:, :2].T + M[:, 2]
    return float(np.abs(got - np.asarray(dst, dtype=np.float64)).max())


def test_boxes_through_get_roi_equal_the_reference(gold):
    from checkerpose_amd import preprocess as PP
    H, W = (int(v) for v in gold["frame_hw"])
    for i, box in enumerate(gold["boxes"]):
        crop = int(gold["crop_size"][i])
        scale, center = PP.get_scale_and_Bbox_center(box, (H, W))
        assert scale == gold["scale"][i] and np.array_equal(center, gold["center"][i]), i
        assert np.array_equal(PP.get_final_Bbox(box, "crop_resize_by_warp_affine", W, H), gold["final"][i]), i
        src, dst = PP.affine_points(center, (scale, scale), 0, (crop, crop))
        assert src.dtype == np.float32 and np.array_equal(_bits(src), _bits(gold["src"][i])), i
        assert dst.dtype == np.float32 and np.array_equal(_bits(dst), _bits(gold["dst"][i])), i
        M = PP._roi_affine(box, W, H, crop)
        assert M.dtype == np.float64 and _maps(M, gold["src"][i], gold["dst"][i]) <= 1e-9, i
        assert tuple(gold["warp_dsize"][i]) == (crop, crop) and gold["warp_flags"][i] == gold["interpolation"][i]      # what get_roi_batch hands on
        assert _maps(gold["warp_M"][i], gold["src"][i], gold["dst"][i]) <= 1e-9                                          # the recorder's own solve


def test_direct_get_affine_transform_calls_equal_the_reference(gold):
    from checkerpose_amd import preprocess as PP
    for i in range(len(gold["d_rot"])):
        c = tuple(float(v) for v in gold["d_center"][i]) if gold["d_center_is_tuple"][i] else np.array(gold["d_center"][i])
        s = float(gold["d_scale"][i][0]) if gold["d_scale_is_scalar"][i] else tuple(float(v) for v in gold["d_scale"][i])
        if gold["d_scale_is_scalar"][i] and s == int(s) and i % 2:
            s = int(s)                                                     # an int scalar, as the maker passed 133
        o = int(gold["d_out"][i][0]) if gold["d_out_is_int"][i] else tuple(int(v) for v in gold["d_out"][i])
        kw = {"shift": gold["d_shift"][i].copy()} if gold["d_shift_given"][i] else {}
        inv = bool(gold["d_inv"][i])
        src, dst = PP.affine_points(c, s, float(gold["d_rot"][i]), o, **kw)
        first, second = (dst, src) if inv else (src, dst)                  # the order the reference hands them to cv2
        assert np.array_equal(_bits(first), _bits(gold["d_src"][i])) and np.array_equal(_bits(second), _bits(gold["d_dst"][i])), i
        M = PP.get_affine_transform(c, s, float(gold["d_rot"][i]), o, inv=inv, **kw)
        assert _maps(M, gold["d_src"][i], gold["d_dst"][i]) <= 1e-9, i


def test_zero_crops_and_the_frame_rectangle():
    from checkerpose_amd import preprocess as PP
    assert PP._roi_affine(None, 64, 48, 8) is None and PP._roi_affine([5, 5, 0, 9], 64, 48, 8) is None and PP._roi_affine([5, 5, 9, -1], 64, 48, 8) is None
    assert PP.roi_window([5, 5, 0, 9], "crop_resize_by_warp_affine", 64, 48, 8) == (0, 0, 0, 0, 0, 0)
    assert np.isnan(PP.affine_from_points(np.zeros((3, 2)), np.ones((3, 2)))).all()
    # box (22, 12, 16, 16) at crop 8: output pixel p reads 22 + 2 p -> corners 22 and 36 -> [22, 37); at crop 16 22 + p -> [22, 38)
    assert PP.roi_window([22, 12, 16, 16], "crop_resize_by_warp_affine", 64, 48, 8) == (22, 12, 37, 27, 15, 15)
    assert PP.roi_window([22, 12, 16, 16], "crop_resize_by_warp_affine", 64, 48, 16) == (22, 12, 38, 28, 16, 16)
    with pytest.raises(NotImplementedError):                 # the rectangle depends on the crop size: without one, as before row N21
        PP.roi_window([22, 12, 16, 16], "crop_resize_by_warp_affine", 64, 48)
    assert PP.roi_window([-30, 40, 20, 20], "crop_resize_by_warp_affine", 64, 48, 8)[:4] == (0, 40, 0, 48)           # off the frame: empty
    # the final box keeps the reference's mismatch: int() and no scale clamp (a 100-wide box in a 64 x 48 frame), unlike the crop's scale
    assert list(PP.get_final_Bbox([-10, 5, 100, 20], "crop_resize_by_warp_affine", 64, 48)) == [-10, -35, 100, 100]
    assert PP.get_scale_and_Bbox_center([-10, 5, 100, 20], (48, 64))[0] == 64.0
    inv = PP._inverse_maps([np.array([[0.5, 0.0, -11.25], [0.0, 0.5, -6.0]]), None], False, 8, 8)
    assert np.array_equal(inv[0], WS.invert([[0.5, 0.0, -11.25], [0.0, 0.5, -6.0]])) and np.isnan(inv[1]).all()
    with pytest.raises(ValueError, match="2\\^20"):
        PP._inverse_maps([np.array([[1.0, 0.0, -1.0e7], [0.0, 1.0, 0.0]])], False, 8, 8)
    with pytest.raises(ValueError, match="2\\^20"):
        PP._inverse_maps([np.array([[1e-7, 0.0, 0.0], [0.0, 1.0, 0.0]])], False, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        import torch
        PP.warp_affine(torch.zeros(4, 4, 3, dtype=torch.uint8), [None], 8)


def _gat():
    from checkerpose_amd.preprocess import get_affine_transform
    return get_affine_transform


@pytest.mark.parametrize("prop", WS.PROPERTIES, ids=lambda f: f.__name__)
def test_restatement_has_the_property(prop):
    assert prop(WS.warp, _gat()) == []


@pytest.mark.parametrize("mutation", WS.MUTATIONS)
def test_every_mutation_breaks_a_property(mutation):
    mutant = lambda img, M, out, interp, inverse_map: WS.warp(img, M, out, interp, inverse_map, mutate=(mutation,))      # noqa: E731
    broken = [p.__name__ for p in WS.PROPERTIES if p(mutant, _gat())]
    print(mutation, "breaks", broken)
    assert broken, mutation


def test_argument_checks_return_before_any_launch(lib):
    """cp_warp_affine_u8 / cp_warp_mask_bits: every refusal comes from the host-side checks (fake pointers, cp_kernel_log stays empty)"""
    A = 0x10000

    def warp(images=A, n_img=2, H=48, W=64, C=3, inv=A, idx=None, out=A, B=2, oh=8, ow=8, interp=1):
        lib.cp_kernel_log_begin()
        rc = lib.cp_warp_affine_u8(None, images, n_img, H, W, C, inv, idx, out, B, oh, ow, interp)
        assert lib.cp_kernel_log() == b""
        return rc

    def bits(plane=A, n_img=2, H=48, W=64, inv=A, idx=None, bit=A, out=A, B=2, oh=8, ow=8):
        lib.cp_kernel_log_begin()
        rc = lib.cp_warp_mask_bits(None, plane, n_img, H, W, inv, idx, bit, out, B, oh, ow)
        assert lib.cp_kernel_log() == b""
        return rc
    assert lib.cp_version() >= 231
    assert warp(C=5) == -1 and warp(C=0) == -1 and warp(images=None) == -1 and warp(inv=None) == -1 and warp(out=None) == -1
    assert warp(B=3) == -1 and bits(B=3) == -1                       # 3 crops of 2 images without an img_index
    assert warp(B=0) == -1 and warp(oh=0) == -1 and warp(ow=-1) == -1 and warp(interp=2) == -1 and warp(H=0) == -1
    assert warp(inv=A + 4) == -3 and warp(idx=A + 2, B=3) == -3 and warp(C=4, images=A + 1) == -3 and warp(C=4, out=A + 2) == -3
    assert warp(H=1 << 16, W=1 << 16) == -4 and warp(B=1 << 20, n_img=1, oh=1 << 12, ow=1 << 12) == -4
    assert bits(plane=None) == -1 and bits(bit=None) == -1 and bits(inv=None) == -1 and bits(out=None) == -1 and bits(oh=0) == -1
    assert bits(plane=A + 2) == -3 and bits(bit=A + 1) == -3 and bits(H=1 << 16, W=1 << 16) == -4
