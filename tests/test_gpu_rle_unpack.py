"""GPU: row N29 on the device.  rle_unpack / rle_stats against the values the reference recorded (tests/golden/coco_eval.npz), against
row N15's own pack_masks of the dense masks and against the numpy rule of tests/rle_stages.py -- everything EQUAL, no tolerance: the
golden frames 31 x 33, 50 x 70 and 120 x 160 (a tail bit, a width that is no multiple of 32, five words in three 64-column strips; the
checkerboards of 1 024 / 3 432 / 19 042 runs take 2 / 7 / 38 passes of the scan); the shape corners (one pixel, one row, one column,
W of exactly one, two and three words, H one more than the 64-row band); non-canonical and invalid lists beside valid neighbours; the
round trips and the callers (rle_encode, paste_masks_rle, pack_rles, eval_bop22_coco)."""
import os

import numpy as np
import pytest
import torch

from checkerpose_amd import _abi
from checkerpose_amd import coco_eval as CE
from tests import coco_stages as CS
from tests import rle_stages as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coco_eval.npz")
FRAMES = ((31, 33), (50, 70), (120, 160))
BAND = 64                                                          # rle_bits_kernel's rows per wave (RU_BAND)
CORNERS = ((1, 1), (1, 65), (70, 1), (5, 32), (5, 64), (5, 96), (BAND + 1, 40))

_GOLD = {}


def recorded(H, W):
    """-> (counts, offsets, the reference's decoded masks (N,H,W) uint8); loaded once, left unchanged"""
    if (H, W) not in _GOLD:
        gold, tag = np.load(GOLDEN), "%dx%d" % (H, W)
        back = np.unpackbits(gold["roundtrip_" + tag], axis=1)[:, :H * W].reshape(-1, H, W)
        out = (gold["rle_counts_" + tag].astype(np.int32), gold["rle_offsets_" + tag].astype(np.int64), np.ascontiguousarray(back))
        for a in out:
            a.setflags(write=False)
        _GOLD[(H, W)] = out
    return _GOLD[(H, W)]


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def flat(lists):
    offsets = np.zeros(len(lists) + 1, np.int64)
    offsets[1:] = np.cumsum([len(c) for c in lists])
    return np.asarray([v for c in lists for v in c], np.int64).astype(np.int32), offsets


def raw_unpack(counts, offsets, H, W, fill, with_bits=True):
    """the entry point itself on outputs that are filled with `fill` first: whatever the call does not write shows"""
    N, total = len(offsets) - 1, len(counts)
    c, o = up(counts), up(offsets)
    mk = lambda *shape: torch.full(shape, fill, dtype=torch.int32, device=DEV)      # noqa: E731
    ends, bits, area, box, status = mk(max(total, 1)), mk(N, H, (W + 31) // 32), mk(N), mk(N, 4), mk(N)
    _abi.call("cp_coco_rle_unpack", DEV, c if total else None, o, N, H, W, total, ends if total else None, bits if with_bits else None,
              area, box, status)
    return [t.cpu().numpy() for t in (bits, area, box, status)]


def same(p, q):
    return torch.equal(p.bits, q.bits) and torch.equal(p.area, q.area) and torch.equal(p.box, q.box) and (p.H, p.W) == (q.H, q.W)


# ---- the golden frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", FRAMES)
def test_golden_frames_in_one_call_and_every_mask_alone(H, W):
    counts, offsets, back = recorded(H, W)
    want = CE.pack_masks(up(back))                                  # row N15's pack of the masks the reference decoded
    got, status = CE.rle_unpack(up(counts), up(offsets), H, W, return_status=True)
    assert isinstance(got, CE.PackedMasks) and (got.H, got.W, len(got)) == (H, W, 14) and got.bits.dtype == torch.int32
    assert tuple(got.bits.shape) == (14, H, (W + 31) // 32) and status.dtype == torch.int32 and not status.any()
    assert same(got, want)
    assert np.array_equal(got.bits.cpu().numpy(), S.pack_bits(back)) and got.area.cpu().tolist() == back.reshape(14, -1).sum(1).tolist()
    assert got.box.cpu().tolist() == [S.dense_box(m) for m in back]
    for fill in (-1, 0x5a5a5a5a):                                   # every word is written, the zero words too
        bits, area, box, st = raw_unpack(counts, offsets, H, W, fill)
        assert np.array_equal(bits, want.bits.cpu().numpy()) and np.array_equal(area, want.area.cpu().numpy()) and not st.any()
    for n in range(14):                                             # alone = in the batch
        c, o = counts[offsets[n]:offsets[n + 1]], np.asarray([0, offsets[n + 1] - offsets[n]], np.int64)
        one = CE.rle_unpack(up(c), up(o), H, W)
        assert torch.equal(one.bits[0], want.bits[n]) and one.area.item() == want.area[n].item() and torch.equal(one.box[0], want.box[n]), n
    assert max(np.diff(offsets)) == {31: 1024, 50: 3432, 120: 19042}[H] > 512      # more than one pass of the scan


# ---- shape corners ----------------------------------------------------------------------------------------------------------------
def corner_masks(H, W):
    """seeded blobs, the full mask, the empty mask and the checkerboard"""
    rng = np.random.default_rng(1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(4):
        cy, cx, ry, rx = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.5, max(H / 2, 1)), rng.uniform(0.5, max(W / 2, 1))
        out.append(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0)
    out.append(rng.random((H, W)) < 0.5)
    out += [np.ones((H, W), bool), np.zeros((H, W), bool), (yy + xx) % 2 == 0, (yy + xx) % 2 == 1]
    return np.stack(out).astype(np.uint8)


@pytest.mark.parametrize("H,W", CORNERS)
def test_shape_corners(H, W):
    dense = corner_masks(H, W)
    lists = [CS.binary_mask_to_rle(m)["counts"] for m in dense] + [[]]          # ... and the empty LIST
    dense = np.concatenate([dense, np.zeros((1, H, W), np.uint8)])
    counts, offsets = flat(lists)
    got = CE.rle_unpack(up(counts), up(offsets), H, W)
    assert same(got, CE.pack_masks(up(dense)))
    assert np.array_equal(got.bits.cpu().numpy(), S.pack_bits(dense)) and got.box.cpu().tolist() == [S.dense_box(m) for m in dense]
    assert got.area.cpu().tolist() == dense.reshape(len(dense), -1).sum(1).tolist()
    bits = raw_unpack(counts, offsets, H, W, -1)[0]
    assert np.array_equal(bits, S.pack_bits(dense))                 # bits past W are written as zeros


def test_no_masks_and_no_counts():
    lib = _abi.load()
    lib.cp_kernel_log_begin()
    p = CE.rle_unpack(torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), 5, 7)
    assert len(p) == 0 and tuple(p.bits.shape) == (0, 5, 1) and lib.cp_kernel_log() == b""      # N == 0: no launch
    p, st = CE.rle_unpack(torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), 5, 7, return_status=True)
    assert len(p) == 3 and not p.bits.any() and not p.area.any() and (p.box == -1).all() and not st.any()       # three empty lists
    bits, area, box, st = raw_unpack(np.zeros(0, np.int32), np.zeros(4, np.int64), 5, 7, -1)
    assert not bits.any() and not area.any() and (box == -1).all() and not st.any()
    with pytest.raises(ValueError, match="int32"):
        CE.rle_unpack(torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV), 5, 7)


# ---- non-canonical and invalid lists beside valid neighbours ----------------------------------------------------------------------
def test_noncanonical_and_invalid_lists_in_one_batch():
    H, W = 5, 7
    big = 2 ** 31 - 1
    lists = [[3, 4, 28],                                            # 0 valid
             [0, 0, 3, 0, 2, 5, 0, 0, 25],                          # 1 zero-length runs, a leading [0, 0]
             [4, 6],                                                # 2 a short sum: the rest is background
             [5, -1, 3],                                            # 3 a negative count                      -> status 1
             [0, 35],                                               # 4 valid (the full mask)
             [10, 26],                                              # 5 a sum of H W + 1                       -> status 2
             [big, big],                                            # 6 64-bit sums: 2^32 - 2, not a wrapped -2 -> status 2
             [7, 9, 4, 3, 12],                                      # 7 valid
             [big, -5, big],                                        # 8 negative AND too long                  -> status 1
             [35]]                                                  # 9 valid (the empty mask)
    counts, offsets = flat(lists)
    masks, area, box, status = S.unpack(counts, offsets, H, W)
    assert status.tolist() == [0, 0, 0, 1, 0, 2, 2, 0, 1, 0]
    for n in (0, 1, 2, 4, 7, 9):                                    # the rule is rle_to_binary_mask on the valid ones
        assert np.array_equal(masks[n], CS.rle_to_binary_mask({"counts": lists[n], "size": [H, W]})), n
    got, st = CE.rle_unpack(up(counts), up(offsets), H, W, check=False, return_status=True)
    assert st.cpu().tolist() == status.tolist()
    assert np.array_equal(got.bits.cpu().numpy(), S.pack_bits(masks)) and got.area.cpu().tolist() == area.tolist()
    assert got.box.cpu().tolist() == box.tolist()
    bad = [3, 5, 6, 8]
    assert not got.bits[bad].any() and not got.area[bad].any() and (got.box[bad] == -1).all()      # zeroed, over a -1 fill too:
    bits, area2, box2, st2 = raw_unpack(counts, offsets, H, W, -1)
    assert np.array_equal(bits, S.pack_bits(masks)) and area2.tolist() == area.tolist() and box2.tolist() == box.tolist()
    assert same(CE.PackedMasks(got.bits[[0, 1, 2, 4, 7, 9]], got.area[[0, 1, 2, 4, 7, 9]], got.box[[0, 1, 2, 4, 7, 9]], H, W),
                CE.pack_masks(up(masks[[0, 1, 2, 4, 7, 9]].astype(np.uint8))))      # the neighbours are what they are alone
    with pytest.raises(ValueError, match="mask 3: RLE counts do not fit 5x7"):
        CE.rle_unpack(up(counts), up(offsets), H, W)
    a, b, s = CE.rle_stats(up(counts), up(offsets), H, W)
    assert torch.equal(a, got.area) and torch.equal(b, got.box) and torch.equal(s, st)


def test_offsets_that_do_not_fit_the_counts_are_refused_by_the_rule():
    """a negative start, an end past the total, a stretch that runs backwards: status 3, no count is read, the neighbours untouched"""
    H, W = 5, 7
    counts = np.asarray([3, 4, 28, 0, 35, 7, 9, 19], np.int32)
    for off, want in (([-1, 3, 5, 13], [3, 0, 3]), ([0, 3, 5, 8, 6, 6], [0, 0, 0, 3, 0]), ([0, 3, 5, 2 ** 40], [0, 0, 3])):
        off = np.asarray(off, np.int64)
        masks, area, box, status = S.unpack(counts, off, H, W)
        assert status.tolist() == want
        bits, area2, box2, st2 = raw_unpack(counts, off, H, W, -1)
        assert st2.tolist() == want and np.array_equal(bits, S.pack_bits(masks)) and area2.tolist() == area.tolist() and box2.tolist() == box.tolist()
        bad = [n for n, s in enumerate(want) if s]
        assert not bits[bad].any() and (box2[bad] == -1).all() and bits[1].any()
        with pytest.raises(ValueError, match="mask %d: RLE counts do not fit" % bad[0]):
            CE.rle_unpack(up(counts), up(off), H, W)


# ---- round trips and callers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", FRAMES)
def test_rle_encode_of_rle_unpack_is_the_list_and_rle_stats_are_its_area_and_box(H, W):
    counts, offsets, _ = recorded(H, W)
    c, o = up(counts), up(offsets)
    p = CE.rle_unpack(c, o, H, W)
    c2, o2 = CE.rle_encode(p)
    assert torch.equal(c2, c) and torch.equal(o2, o)
    area, box, status = CE.rle_stats(c, o, H, W)
    assert torch.equal(area, p.area) and torch.equal(box, p.box) and not status.any()
    bits, area2, box2, _ = raw_unpack(counts, offsets, H, W, -1, with_bits=False)      # bits = NULL: nothing but area, box, status
    assert (bits == -1).all() and np.array_equal(area2, p.area.cpu().numpy()) and np.array_equal(box2, p.box.cpu().numpy())


def test_paste_masks_rle_goes_straight_to_the_scorer():
    from checkerpose_amd import postprocess as Q
    from tests.test_gpu_paste_masks import case
    H, W = 31, 33
    seg, boxes, _, dense = case(H, W, 16, 16, "crop_square_resize")
    seg_t = up(seg)
    counts, offsets, area, box = Q.paste_masks_rle(seg_t, boxes, (H, W))
    p, q = CE.rle_unpack(counts, offsets, H, W), Q.paste_masks(seg_t, boxes, (H, W))
    assert same(p, q) and torch.equal(p.area, area) and torch.equal(p.box, box) and p.area.any()
    pairs = [[d, g] for d in range(len(p)) for g in range(len(p))]
    assert torch.equal(CE.mask_ious(p, q, pairs), CE.mask_ious(up(dense[0]), up(dense[0]), pairs))      # mask_ious takes it as it is


@pytest.mark.parametrize("H,W", FRAMES)
def test_pack_rles_equals_the_host_decode_and_pack(H, W):
    counts, offsets, back = recorded(H, W)
    rles = [{"counts": counts[offsets[n]:offsets[n + 1]].tolist(), "size": [H, W]} for n in range(14)]
    rles += [{"counts": c, "size": [H, W]} for c in ([], [H * W], [0, 0, 5, 0, 3], [H - 1, 2, 0, 0, H], [7, 9])]      # non-canonical
    want = CE.pack_masks(CE.rle_decode(rles), DEV)                  # the parent's path: host decode, upload, cp_coco_pack
    assert np.array_equal(CE.rle_decode(rles)[:14], back)
    for chunk in (512, 5):
        assert same(CE.pack_rles(rles, DEV, chunk=chunk), want)
    strings = [dict(r, counts=CE.rle_to_string(r["counts"])) for r in rles]
    assert same(CE.pack_rles(strings, DEV), want) and same(CE.pack_rles(CE.rle_dicts(up(counts), up(offsets), H, W, compress=True), DEV),
                                                            CE.pack_masks(up(back)))
    with pytest.raises(ValueError, match="mask 15: RLE counts do not fit"):
        CE.pack_rles(rles[:15] + [{"counts": [H * W, 1], "size": [H, W]}], DEV, chunk=4)
    with pytest.raises(ValueError, match="every RLE must have size"):
        CE.pack_rles(rles[:2] + [{"counts": [1], "size": [W, H]}], DEV)


def test_eval_bop22_coco_scores_lists_and_compressed_strings_alike():
    H, W = 31, 33
    _, _, back = recorded(H, W)
    rle = lambda m: CS.binary_mask_to_rle(m)      # noqa: E731
    xywh = lambda m: CS.bbox_from_binary_mask(m)      # noqa: E731
    gts = [(1, 1, 2), (1, 2, 3), (2, 1, 4), (2, 2, 5), (2, 1, 6)]              # (image, category, golden mask)
    dts = [(1, 1, 2, .9), (1, 1, 3, .8), (1, 2, 3, .7), (2, 1, 4, .95), (2, 1, 5, .6), (2, 2, 6, .5), (2, 2, 5, .4), (1, 2, 7, .3)]
    ann = {"categories": [{"id": 1}, {"id": 2}], "images": [{"id": 1}, {"id": 2}],
           "annotations": [{"id": n + 1, "image_id": i, "category_id": c, "iscrowd": 0, "area": int(back[m].sum()), "bbox": xywh(back[m]),
                            "ignore": 0, "segmentation": rle(back[m])} for n, (i, c, m) in enumerate(gts)]}
    results = [{"scene_id": 4, "image_id": i, "category_id": c, "score": s, "bbox": xywh(back[m]), "segmentation": rle(back[m]), "time": 0.25}
               for i, c, m, s in dts]
    targets = [{"scene_id": 4, "im_id": 1}, {"scene_id": 4, "im_id": 2}]
    plain = CE.eval_bop22_coco({4: ann}, results, targets, "segm", device=DEV)
    squeeze = lambda d: dict(d, segmentation=dict(d["segmentation"], counts=CE.rle_to_string(d["segmentation"]["counts"])))      # noqa: E731
    ann_s = dict(ann, annotations=[squeeze(a) for a in ann["annotations"]])
    packed = CE.eval_bop22_coco({4: ann_s}, [squeeze(r) for r in results], targets, "segm", device=DEV)
    assert all(isinstance(r["segmentation"]["counts"], list) for r in results)                  # the inputs are left as they were
    assert plain == packed and 0 < plain["AP"] < 1 and plain["average_time_per_image"] == 0.25
    # ... and they are the scores of the dense masks
    cs = CE.CocoSet([1, 2], [1, 2], [g[0] for g in gts], [g[1] for g in gts], [int(back[g[2]].sum()) for g in gts],
                    masks=up(back[[g[2] for g in gts]]), device=DEV)
    dense = CE.evaluate(cs, {"image_id": [d[0] for d in dts], "category_id": [d[1] for d in dts], "score": [d[3] for d in dts],
                             "masks": up(back[[d[2] for d in dts]])}, "segm")
    assert {k: dense[k] for k in CE.STAT_NAMES} == {k: plain[k] for k in CE.STAT_NAMES}
