"""GPU: row N27 on the device.  paste_masks / paste_masks_rle / unpack_masks against the numpy rule of tests/paste_stages.py and against
row N15's own pack_masks / rle_encode of the restatement's dense masks -- everything EQUAL, no tolerance: frames 31 x 33, 50 x 70 and
120 x 160 (a tail bit, a width that is no multiple of 32, five words), planes 64 x 64, 16 x 16 and a non-square 8 x 16, windows made by
preprocess._windows from real boxes for both methods; the identities (alone / in a batch, strides / copies); the callers."""
import numpy as np
import pytest
import torch

from tests import coco_stages as CS
from tests import paste_stages as PS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FRAMES = ((31, 33), (50, 70), (120, 160))
PLANES = ((64, 64), (16, 16), (8, 16))
METHODS = ("crop_square_resize", "crop_resize")


def boxes_for(H, W):
    """(x, y, w, h), already padded, as get_roi_batch takes them"""
    return [[3, 2, 20, 17],                                                   # inside
            [-7, -5, 21, 15], [-3, 1, 9, 13], [-1, -2, 8, 5],                 # negative and odd coordinates: x2 - x1 != rw under int()
            [-10, H // 3, 25, 12], [W - 8, 4, 20, 10], [5, -9, 12, 20], [6, H - 6, 14, 15],      # over the left, right, top, bottom edge
            [W + 5, 3, 10, 10], [4, H + 2, 9, 9],                             # wholly outside
            [-30, 2, 12, 10], [2, -40, 10, 15],                               # wholly left / above: crop_resize's negative end
            [-20, -15, W + 50, H + 40],                                       # larger than the frame
            None,
            [10, 8, 1, 1], [12, 9, 5, 3], [11, 7, 5, 5],                      # rw of 1 and 5: down-sampling
            [30, 10, 100, 100]]                                               # rw = 100: non-integer up-sampling in the 160-wide frame


def planes_for(Sh, Sw, n, seed):
    """n planes that cycle through: random logits, all set, all clear, a checkerboard (the most runs), a single cell, the threshold's
    bit pattern with its two float neighbours, +-0, NaN and +-inf"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:Sh, 0:Sw]
    z0 = PS.Z0
    special = np.array([z0, np.nextafter(z0, np.float32(1)), np.nextafter(z0, np.float32(-1)), 0.0, -0.0, np.nan, np.inf, -np.inf], np.float32)
    out = []
    for k in range(n):
        kind = k % 6
        if kind == 0:
            p = rng.normal(size=(Sh, Sw))
        elif kind == 1:
            p = np.full((Sh, Sw), 2.5)
        elif kind == 2:
            p = np.full((Sh, Sw), -2.5)
        elif kind == 3:
            p = np.where((yy + xx) % 2 == 0, 1.0, -1.0)
        elif kind == 4:
            p = np.full((Sh, Sw), -1.0)
            p[int(rng.integers(Sh)), int(rng.integers(Sw))] = 1.0
        else:
            p = special[rng.integers(0, len(special), (Sh, Sw))]
        out.append(np.asarray(p, np.float32))
    return np.stack(out)


_CASES = {}


def case(H, W, Sh, Sw, method):
    """-> (seg (B,2,Sh,Sw) numpy, boxes, windows (B,6), the restatement's dense masks (2,B,H,W)); computed once, left unchanged"""
    from checkerpose_amd import preprocess as PRE
    key = (H, W, Sh, Sw, method)
    if key not in _CASES:
        boxes = boxes_for(H, W)
        B = len(boxes)
        seg = np.stack([planes_for(Sh, Sw, B, 7 * H + Sh), np.roll(planes_for(Sh, Sw, B, 11 * W + Sw), 2, 0)], 1)
        win = PRE._windows(boxes, method, W, H)
        dense = np.stack([[PS.paste(seg[b, c], win[b], H, W) for b in range(B)] for c in range(2)])
        for a in (seg, win, dense):
            a.setflags(write=False)
        _CASES[key] = (seg, boxes, win, dense)
    return _CASES[key]


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _runs(counts, offsets):
    c, o = counts.cpu().numpy(), offsets.cpu().numpy()
    return [c[o[n]:o[n + 1]].tolist() for n in range(len(o) - 1)]


def test_the_windows_hold_the_cases_the_rule_has_to_meet():
    from checkerpose_amd import preprocess as PRE
    for H, W in FRAMES:
        sq, cr = (PRE._windows(boxes_for(H, W), m, W, H).astype(np.int64) for m in METHODS)
        assert (sq[:, 2] - sq[:, 0] != sq[:, 4]).any() and (sq[:, 3] - sq[:, 1] != sq[:, 5]).any()             # int() of a negative corner
        assert (sq[:, 0] < 0).any() and (sq[:, 2] > W).any() and (sq[:, 1] < 0).any() and (sq[:, 3] > H).any()
        assert (sq[:, 0] >= W).any() and (sq[:, 1] >= H).any() and (sq[13] == 0).all()                           # outside; None
        assert ((sq[:, 4] > W) & (sq[:, 5] > H)).any() and {1, 5} <= set(sq[:, 4].tolist())
        assert tuple(cr[10]) == (0, 2, W - 18, 12, W - 18, 10) and tuple(cr[11][[1, 3, 5]]) == (0, H - 25, H - 25)   # the negative end
    assert 100 in PRE._windows(boxes_for(120, 160), METHODS[0], 160, 120)[:, 4]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("Sh,Sw", PLANES)
@pytest.mark.parametrize("H,W", FRAMES)
def test_paste_masks_and_rle_equal_the_rule(H, W, Sh, Sw, method):
    from checkerpose_amd import coco_eval as CE
    from checkerpose_amd import postprocess as Q
    seg, boxes, win, dense = case(H, W, Sh, Sw, method)
    seg_t = _up(seg)
    B = len(boxes)
    assert dense[0].any() and dense[1].any()
    for c in range(2):
        p = Q.paste_masks(seg_t, boxes, (H, W), method, channel=c)
        assert isinstance(p, CE.PackedMasks) and (p.H, p.W, len(p)) == (H, W, B)
        assert p.bits.dtype == p.area.dtype == p.box.dtype == torch.int32 and tuple(p.bits.shape) == (B, H, (W + 31) // 32)
        want = [PS.area_box(m) for m in dense[c]]
        assert np.array_equal(p.bits.cpu().numpy(), np.stack([PS.pack(m) for m in dense[c]]))
        assert p.area.cpu().tolist() == [a for a, _ in want] and p.box.cpu().tolist() == [b for _, b in want]
        q = CE.pack_masks(_up(dense[c]))                                         # what row N15 makes of the dense masks
        assert torch.equal(p.bits, q.bits) and torch.equal(p.area, q.area) and torch.equal(p.box, q.box)
        back = CE.unpack_masks(p)
        assert back.dtype == torch.uint8 and np.array_equal(back.cpu().numpy(), dense[c])
        counts, offsets, area, box = Q.paste_masks_rle(seg_t, boxes, (H, W), method, channel=c)
        c2, o2 = CE.rle_encode(p)
        assert counts.dtype == torch.int32 and offsets.dtype == torch.int64
        assert torch.equal(counts, c2) and torch.equal(offsets, o2) and torch.equal(area, p.area) and torch.equal(box, p.box)
        assert _runs(counts, offsets) == [PS.rle(m) for m in dense[c]]


@pytest.mark.parametrize("method", METHODS)
def test_a_mask_alone_equals_the_mask_in_batches_of_3_and_70(method):
    from checkerpose_amd import postprocess as Q
    H, W = 50, 70
    seg, boxes, win, dense = case(H, W, 16, 16, method)
    B = len(boxes)
    full = Q.paste_masks(_up(seg), boxes, (H, W), method)
    full_rle = _runs(*Q.paste_masks_rle(_up(seg), boxes, (H, W), method)[:2])
    for b in (0, 1, 4, 12, 13, 17):
        for n in (1, 3, 70):
            at = (5 * b + 1) % n
            idx = [(b + 3 * k + 1) % B for k in range(n)]
            idx[at] = b
            s, bx = _up(seg[idx]), [boxes[i] for i in idx]
            p = Q.paste_masks(s, bx, (H, W), method)
            assert torch.equal(p.bits[at], full.bits[b]) and int(p.area[at]) == int(full.area[b]) and torch.equal(p.box[at], full.box[b])
            counts, offsets, area, box = Q.paste_masks_rle(s, bx, (H, W), method)
            assert _runs(counts, offsets)[at] == full_rle[b] and int(area[at]) == int(full.area[b]) and torch.equal(box[at], full.box[b])


def test_channels_through_strides_equal_contiguous_copies():
    from checkerpose_amd import coco_eval as CE
    from checkerpose_amd import postprocess as Q
    H, W = 120, 160
    seg, boxes, win, dense = case(H, W, 8, 16, METHODS[0])
    seg_t = _up(seg)
    wide = torch.zeros(len(boxes), 5, 8, 16, device=DEV)
    wide[:, 1:3] = seg_t
    views = {"module": seg_t, "a channel slice": wide[:, 1:3], "transposed planes": seg_t.transpose(2, 3).contiguous().transpose(2, 3)}
    assert not views["transposed planes"][:, 0].is_contiguous() and views["a channel slice"].stride(0) == 5 * 8 * 16
    for c in range(2):
        copy = seg_t[:, c].contiguous()[:, None]                                 # (B,1,Sh,Sw): the plane on its own
        want = Q.paste_masks(copy, boxes, (H, W), channel=0)
        assert np.array_equal(CE.unpack_masks(want).cpu().numpy(), dense[c])
        want_rle = Q.paste_masks_rle(copy, boxes, (H, W), channel=0)
        for name, v in views.items():
            got = Q.paste_masks(v, boxes, (H, W), channel=c)
            assert torch.equal(got.bits, want.bits) and torch.equal(got.area, want.area) and torch.equal(got.box, want.box), name
            assert all(torch.equal(x, y) for x, y in zip(Q.paste_masks_rle(v, boxes, (H, W), channel=c), want_rle)), name
    one = Q.paste_masks(seg_t[4:5].expand(3, -1, -1, -1), [boxes[0], boxes[4], boxes[12]], (H, W))      # batch stride 0: one plane, three windows
    ref = Q.paste_masks(seg_t[[4, 4, 4]], [boxes[0], boxes[4], boxes[12]], (H, W))
    assert torch.equal(one.bits, ref.bits) and torch.equal(one.box, ref.box)
    empty = Q.paste_masks(seg_t[:0], [], (H, W))
    assert len(empty) == 0 and tuple(empty.bits.shape) == (0, H, 5)
    counts, offsets, area, box = Q.paste_masks_rle(seg_t[:0], [], (H, W))
    assert counts.numel() == 0 and offsets.tolist() == [0] and area.numel() == 0


def test_offsets_that_do_not_fit_leave_the_mask_unwritten_as_cp_coco_rle_write_does():
    from checkerpose_amd import _abi
    from checkerpose_amd import coco_eval as CE
    from checkerpose_amd import postprocess as Q
    H, W = 31, 33
    seg, boxes, win, dense = case(H, W, 16, 16, METHODS[0])
    seg_t, win_t, B = _up(seg), _up(win), len(boxes)
    p = Q.paste_masks(seg_t, boxes, (H, W))
    counts, offsets = CE.rle_encode(p)
    total = int(offsets[-1])
    for mutate in (lambda o: o.__setitem__(slice(5, None), o[5:] + total), lambda o: o.__setitem__(3, -1), lambda o: o.__setitem__(7, o[6] - 1),
                   lambda o: o.__setitem__(slice(9, 11), o[9:11] - 2)):
        off = offsets.clone()
        mutate(off)
        a = torch.full((total,), -7, dtype=torch.int32, device=DEV)
        b = a.clone()
        _abi.call("cp_coco_rle_write", DEV, p.bits, B, H, W, off, a, total)
        _abi.call("cp_paste_rle_write", DEV, seg_t, 2 * 16 * 16, 16, 16, win_t, B, H, W, off, b, total)
        assert torch.equal(a, b) and bool((a == -7).any()) and bool((a != -7).any())


def test_segmentation_results_are_bop22_results_of_the_pasted_masks():
    from checkerpose_amd import coco_eval as CE
    H, W = 120, 160
    seg, boxes, win, dense = case(H, W, 64, 64, METHODS[1])
    B = len(boxes)
    score = np.linspace(0.9, 0.1, B)
    res = CE.segmentation_results(_up(seg), boxes, (H, W), 48, 7, np.arange(B) % 3 + 1, score, time=0.25, resize_method=METHODS[1], channel=1)
    assert CE.check_coco_results(res, ann_type="segm") == (True, "OK") and len(res) == B
    assert np.array_equal(CE.rle_decode([r["segmentation"] for r in res]), dense[1])
    for b, r in enumerate(res):
        area, box = PS.area_box(dense[1][b])
        assert sorted(r) == ["bbox", "category_id", "image_id", "scene_id", "score", "segmentation", "time"]
        assert (r["scene_id"], r["image_id"], r["category_id"], r["score"], r["time"]) == (48, 7, b % 3 + 1, float(score[b]), 0.25)
        assert r["bbox"] == ([box[0], box[1], box[2] - box[0] + 1, box[3] - box[1] + 1] if area else [-1, -1, -1, -1])
        assert r["bbox"] == (CS.bbox_from_binary_mask(dense[1][b]) if area else [-1] * 4) and r["segmentation"]["size"] == [H, W]
    assert sum(1 for r in res if r["bbox"] == [-1] * 4) >= 3                     # empty masks are kept
    assert "time" not in CE.segmentation_results(_up(seg), boxes, (H, W), 48, 7, 1, 0.5)[0]


def test_evaluate_takes_the_packed_masks_where_dense_masks_were():
    from checkerpose_amd import coco_eval as CE
    from checkerpose_amd import postprocess as Q
    H, W = 50, 70
    seg, boxes, win, dense = case(H, W, 16, 16, METHODS[0])
    p = Q.paste_masks(_up(seg), boxes, (H, W))
    keep = np.nonzero(p.area.cpu().numpy() > 0)[0]
    assert len(keep) >= 6
    sel = torch.from_numpy(keep).to(DEV)
    sub = CE.PackedMasks(p.bits[sel].contiguous(), p.area[sel].contiguous(), p.box[sel].contiguous(), H, W)
    img, cat = np.arange(len(keep)) // 2, np.arange(len(keep)) % 2 + 1
    cs = CE.CocoSet(np.unique(img), [1, 2], img, cat, sub.area.cpu().numpy(), masks=sub, device=DEV)
    dets = {"image_id": img, "category_id": cat, "score": np.linspace(0.9, 0.2, len(keep)), "masks": sub}
    out = CE.evaluate(cs, dets, "segm")
    assert out["AP"] == 1.0 and out["AP50"] == 1.0 and out["AR100"] == 1.0
    dense_out = CE.evaluate(CE.CocoSet(np.unique(img), [1, 2], img, cat, sub.area.cpu().numpy(), masks=_up(dense[0][keep]), device=DEV),
                            dict(dets, masks=_up(dense[0][keep])), "segm")
    assert np.array_equal(out["precision"], dense_out["precision"]) and np.array_equal(out["recall"], dense_out["recall"])


def test_estimate_poses_masks_is_estimate_poses_plus_paste_masks_of_the_same_forward():
    from checkerpose_amd import postprocess as Q
    from checkerpose_amd import preprocess as PRE
    from checkerpose_amd.synthetic import build_net
    from tests import pnp_stages as S
    rng = np.random.default_rng(9)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 480, 640, 3), dtype=np.uint8)).cuda()
    boxes = [[100, 80, 120, 90], [300, 200, 60, 140], None, [-10, 400, 90, 90]]
    idx = [0, 1, 0, 1]
    net = build_net(npoint=512, seed=1).cuda().eval()
    net.set_compute_dtype("bf16")
    p3d = torch.from_numpy(S.lmo_model(512).astype(np.float32)).cuda()
    K = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]], dtype=np.float32)
    kw = dict(img_index=idx, seed=3)
    plain = Q.estimate_poses(net, frames, boxes, p3d, K, **kw)
    padded = [None if b is None else PRE.padding_Bbox(b, 1.5) for b in boxes]
    with torch.no_grad():
        seg = net(PRE.get_roi_batch(frames, padded, 256, PRE.INTER_LINEAR, "crop_square_resize", img_index=idx), None)[3]      # a separate forward
    assert tuple(seg.shape) == (4, 2, 64, 64) and seg.dtype == torch.float32
    for channel in (0, 1):
        out = Q.estimate_poses_masks(net, frames, boxes, p3d, K, channel=channel, **kw)
        assert len(out) == 6 and all(torch.equal(x, y) for x, y in zip(out[:4], plain[:4])) and np.array_equal(out[4], plain[4])
        want = Q.paste_masks(seg, padded, (480, 640), channel=channel)
        m = out[5]
        assert (m.H, m.W) == (480, 640) and torch.equal(m.bits, want.bits) and torch.equal(m.area, want.area) and torch.equal(m.box, want.box)
        assert int(m.area[2]) == 0 and m.box[2].tolist() == [-1] * 4             # no detection: an empty mask
        win = PRE._windows(padded, "crop_square_resize", 640, 480)
        dense = np.stack([PS.paste(seg[b, channel].cpu().numpy(), win[b], 480, 640) for b in range(4)])
        assert np.array_equal(m.bits.cpu().numpy(), np.stack([PS.pack(d) for d in dense]))
