#!/usr/bin/env python3
"""Row N21 (crop_resize_by_warp_affine) pinned by the REFERENCE's own code: everything of the crop up to the two cv2 calls.

Runs ONLY where the reference checkout is present (REF below; nothing of the reference travels, only warp_affine.npz is committed):

  python tests/golden/make_golden_warp.py

`bop_dataset_pytorch.py` and `GDR_Net_Augmentation.py` are imported with the third-party modules this image lacks stubbed (`cv2`, `mmcv`,
`imageio`, `torchvision`, `imgaug`, `binary_code_helper`; the trick of make_golden_n3.py).  The two cv2 calls are RECORDERS:
  * `cv2.getAffineTransform(src, dst)` stores both float32 point triples and returns a numpy solve of the 6 x 6 system (zeros where it is
    singular);
  * `cv2.warpAffine(img, M, dsize, flags=)` stores the matrix, `dsize` and the flags it was handed.
The reference's own functions then run over
  * boxes -- inside a 640 x 480 frame, straddling it, off it, larger than it, 1 pixel wide -- through
    `get_roi(frame, box, crop, interpolation, "crop_resize_by_warp_affine")` (:132-145), `get_scale_and_Bbox_center` (:111-129) and
    `get_final_Bbox` (:188-222): per box the scale, the centre, the final box, both triples, and what warpAffine was handed;
  * direct `get_affine_transform(center, scale, rot, output_size, shift, inv)` calls (GDR_Net_Augmentation.py:199-240): rotations,
    non-zero shifts, `inv`, a scalar and a pair for scale and output_size, a tuple and an array for the centre: both triples per call.
Only recorded data goes into the fixture."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "checkerpose"))

REC = {}


def _get_affine_recorder(src, dst):
    REC["src"], REC["dst"] = np.array(src, copy=True), np.array(dst, copy=True)
    assert REC["src"].dtype == np.float32 and REC["dst"].dtype == np.float32
    A = np.zeros((6, 6))
    for i in range(3):
        A[2 * i, :3] = [src[i, 0], src[i, 1], 1.0]
        A[2 * i + 1, 3:] = [src[i, 0], src[i, 1], 1.0]
    try:
        return np.linalg.solve(A, np.asarray(dst, dtype=np.float64).reshape(6)).reshape(2, 3)
    except np.linalg.LinAlgError:
        return np.zeros((2, 3))


def _warp_recorder(img, M, dsize, flags=None, **kw):
    REC["M"], REC["dsize"], REC["flags"] = np.array(M, dtype=np.float64, copy=True), tuple(dsize), flags
    return np.zeros((dsize[1], dsize[0]) + img.shape[2:], dtype=img.dtype)


class _Anything(types.ModuleType):
    """a module whose every attribute is a callable that returns None (imgaug's augmenter constructors at import time)"""
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: None


def install_stubs():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST, cv2.INTER_LINEAR = 0, 1
    cv2.getAffineTransform, cv2.warpAffine = _get_affine_recorder, _warp_recorder
    sys.modules["cv2"] = cv2
    for name in ("mmcv", "imageio", "torchvision", "torchvision.transforms", "binary_code_helper", "binary_code_helper.class_id_encoder_decoder"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["binary_code_helper.class_id_encoder_decoder"].class_id_vec_to_class_code_vecs = None
    sys.modules["imgaug"] = types.ModuleType("imgaug")
    sys.modules["imgaug.augmenters"] = sys.modules["imgaug"].augmenters = _Anything("imgaug.augmenters")


def boxes_under_test(W, H):
    rng = np.random.default_rng(20261019)
    bx = [[10, 12, 21, 30], [4, 0, 13, 26], [8, 20, 40, 10], [100, 100, 64, 64], [101, 57, 33, 32]]                  # inside
    for _ in range(24):
        bx.append([int(rng.integers(0, W - 8)), int(rng.integers(0, H - 8)), int(rng.integers(8, 260)), int(rng.integers(8, 260))])
    for _ in range(24):                                                                                          # straddling any edge
        bx.append([int(rng.integers(-300, W + 100)), int(rng.integers(-300, H + 100)), int(rng.integers(4, 400)), int(rng.integers(4, 400))])
    bx += [[W + 50, 10, 40, 40], [10, H + 80, 30, 60], [-400, -400, 20, 30],                                     # off the frame
           [0, 0, W, H], [-10, -10, W + 20, H + 20], [-100, 50, 900, 30], [30, -200, 50, 1000], [0, 0, 641, 481],  # larger than it
           [20, 10, 1, 1], [30, 20, 1, 9], [30, 20, 7, 1], [W - 1, H - 1, 1, 1], [-1, -1, 2, 2]]                   # 1 pixel wide
    return np.array(bx, dtype=np.int64)


def direct_calls():
    """(center, center_is_tuple, scale, scale_is_scalar, rot, output_size, out_is_int, shift or None, inv)"""
    f32 = lambda a, b: np.array([a, b], dtype=np.float32)      # noqa: E731
    calls = []
    for rot in (0, 90, 180, 270, -90, 30, -17.5, 45.0, 123.456):
        calls.append(((30.0, 20.0), False, (16.0, 16.0), False, rot, (8, 8), False, None, False))
        calls.append(((31.5, 20.25), True, 24.0, True, rot, 12, True, None, False))
        calls.append(((300.7, 199.1), False, (77.0, 50.0), False, rot, (16, 12), False, f32(0.1, -0.2), False))
        calls.append(((-12.3, 500.9), True, 133, True, rot, (64, 48), False, f32(-0.25, 0.125), True))
    calls.append(((10.0, 10.0), False, (1.0, 1.0), False, 0, (256, 256), False, None, True))
    calls.append(((320.0, 240.0), False, (640.0, 640.0), False, 0.0, 256, True, f32(0.3, 0.3), False))
    return calls


def main():
    install_stubs()
    import bop_dataset_pytorch as D                                             # the reference's own modules
    import GDR_Net_Augmentation as G
    W, H = 640, 480
    frame = np.zeros((H, W, 3), np.uint8)
    boxes = boxes_under_test(W, H)
    n = len(boxes)
    crops = np.where(np.arange(n) % 3 == 0, 64, 256).astype(np.int64)
    interps = (np.arange(n) % 2).astype(np.int64)
    out = {"frame_hw": np.array([H, W]), "boxes": boxes, "crop_size": crops, "interpolation": interps,
           "scale": np.zeros(n), "center": np.zeros((n, 2)), "final": np.zeros((n, 4), np.int64), "src": np.zeros((n, 3, 2), np.float32),
           "dst": np.zeros((n, 3, 2), np.float32), "warp_M": np.zeros((n, 2, 3)), "warp_dsize": np.zeros((n, 2), np.int64),
           "warp_flags": np.zeros(n, np.int64)}
    for i, b in enumerate(boxes):
        REC.clear()
        D.get_roi(frame, np.array(b), int(crops[i]), int(interps[i]), "crop_resize_by_warp_affine")
        out["scale"][i], out["center"][i] = D.get_scale_and_Bbox_center(np.array(b), frame)
        out["final"][i] = D.get_final_Bbox(np.array(b), "crop_resize_by_warp_affine", W, H)
        out["src"][i], out["dst"][i], out["warp_M"][i] = REC["src"], REC["dst"], REC["M"]
        out["warp_dsize"][i], out["warp_flags"][i] = REC["dsize"], REC["flags"]
    calls = direct_calls()
    m = len(calls)
    d = {"d_center": np.zeros((m, 2)), "d_center_is_tuple": np.zeros(m, np.uint8), "d_scale": np.zeros((m, 2)), "d_scale_is_scalar": np.zeros(m, np.uint8),
         "d_rot": np.zeros(m), "d_out": np.zeros((m, 2), np.int64), "d_out_is_int": np.zeros(m, np.uint8), "d_shift": np.zeros((m, 2), np.float32),
         "d_shift_given": np.zeros(m, np.uint8), "d_inv": np.zeros(m, np.uint8), "d_src": np.zeros((m, 3, 2), np.float32),
         "d_dst": np.zeros((m, 3, 2), np.float32)}
    for i, (c, c_tup, s, s_scalar, rot, o, o_int, shift, inv) in enumerate(calls):
        REC.clear()
        kw = {} if shift is None else {"shift": shift}
        G.get_affine_transform(tuple(c) if c_tup else np.array(c), s if s_scalar else tuple(s), rot, o if o_int else tuple(o), inv=inv, **kw)
        d["d_center"][i], d["d_center_is_tuple"][i] = c, c_tup
        d["d_scale"][i], d["d_scale_is_scalar"][i] = (s, s) if s_scalar else s, s_scalar
        d["d_rot"][i], d["d_out"][i], d["d_out_is_int"][i] = rot, (o, o) if o_int else o, o_int
        d["d_shift"][i], d["d_shift_given"][i], d["d_inv"][i] = (0, 0) if shift is None else shift, shift is not None, inv
        # with inv the reference hands (dst, src) to cv2: stored here in the order of the CALL, first argument first
        d["d_src"][i], d["d_dst"][i] = REC["src"], REC["dst"]
    out.update(d)
    path = os.path.join(HERE, "warp_affine.npz")
    np.savez_compressed(path, **out)
    print("wrote warp_affine.npz: %d boxes, %d direct calls, %.1f KB" % (n, m, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
