"""CPU: row N29 (COCO RLE masks decoded on the device).  The numpy restatement of the rule (tests/rle_stages.py) against the values the
reference recorded (tests/golden/coco_eval.npz: roundtrip_* is pycoco_utils.rle_to_binary_mask's own output), against the host decoder
and the older restatement on non-canonical lists; the status precedence; pycocotools' string codec against hand-derived vectors and
against a second restatement; one named case per clause of the rule that a slip would break; the host half of
checkerpose_amd/coco_eval.py (rle_flatten, the codec, rle_dicts) and the argument checks of cp_coco_rle_unpack."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from checkerpose_amd import coco_eval as CE
from tests import coco_stages as CS
from tests import rle_stages as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coco_eval.npz")
FRAMES = ((31, 33), (50, 70), (120, 160))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def recorded(gold, H, W):
    """-> (counts, offsets, the reference's decoded masks (N,H,W) bool, the masks it encoded, bbox x y w h)"""
    tag = "%dx%d" % (H, W)
    back = np.unpackbits(gold["roundtrip_" + tag], axis=1)[:, :H * W].reshape(-1, H, W).astype(bool)
    masks = np.unpackbits(gold["masks_" + tag], axis=1)[:, :H * W].reshape(-1, H, W).astype(bool)
    return gold["rle_counts_" + tag], gold["rle_offsets_" + tag], back, masks, gold["bbox_" + tag]


def noncanonical_lists(H, W, seed, n=40):
    """seeded lists that no encoder writes: zero-length runs anywhere, sums below H W, leading [0, 0, ...], m of 0, 1 and 2"""
    rng = np.random.default_rng(seed)
    HW = H * W
    out = [[], [HW], [0], [3], [0, HW], [2, 0], [0, 0, 0, 5, 0, 0, 2, 1], [0, 0, HW], [HW - 1, 1], [H - 1, 2, 0, 0, 3]]
    out = [c for c in out if sum(c) <= HW]
    for _ in range(n):
        m = int(rng.integers(1, 12))
        c = rng.integers(0, max(2, 2 * HW // m), m)
        c[rng.random(m) < 0.3] = 0
        if rng.random() < 0.3:
            c = np.concatenate([np.zeros(int(rng.integers(1, 4)), np.int64), c])
        while c.sum() > HW:                                       # keep the list valid: cut the largest run
            c[np.argmax(c)] //= 2
        out.append([int(v) for v in c])
    return out


# ---- the pinned side --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", FRAMES)
def test_the_rule_reproduces_the_recorded_decodes_areas_and_boxes(gold, H, W):
    counts, offsets, back, masks, bbox = recorded(gold, H, W)
    assert len(back) == 14 and np.array_equal(back, masks)
    for n in range(14):
        c = counts[offsets[n]:offsets[n + 1]]
        assert np.array_equal(S.decode(c, H, W), back[n]), n
        assert S.area(c) == int(back[n].sum()), n
        x, y, w, h = (int(v) for v in bbox[n])                      # the recorded box is x y w h; -1s for the empty mask
        want = [-1] * 4 if w < 0 else [x, y, x + w - 1, y + h - 1]
        assert S.box(c, H, W) == want == S.dense_box(back[n]), n
    got = S.unpack(counts, offsets, H, W)
    assert np.array_equal(got[0], back) and not got[3].any()
    assert counts[offsets[1]:offsets[2]].tolist() == [0, H * W]                # the full mask: a leading 0
    assert counts[offsets[4]:offsets[5]].tolist() == [3 * H + H - 2, 4, H * W - 4 * H - 2]      # one run across a column boundary
    assert max(np.diff(offsets)) == {31: 1024, 50: 3432, 120: 19042}[H]      # the checkerboard


@pytest.mark.parametrize("H,W", ((5, 7), (1, 9), (6, 1), (4, 4)))
def test_the_rule_equals_the_host_decoder_and_the_older_restatement_on_noncanonical_lists(H, W):
    lists = noncanonical_lists(H, W, seed=H * 100 + W)
    assert any(len(c) == 0 for c in lists) and any(len(c) == 1 for c in lists) and any(len(c) == 2 for c in lists)
    assert any(0 in c[1:-1] for c in lists) and any(sum(c) < H * W for c in lists) and any(c[:2] == [0, 0] for c in lists)
    rles = [{"counts": c, "size": [H, W]} for c in lists]
    host = CE.rle_decode(rles)
    for n, c in enumerate(lists):
        want = CS.rle_to_binary_mask(rles[n])
        got = S.decode(c, H, W)
        assert np.array_equal(got, want) and np.array_equal(host[n] != 0, want), c
        assert S.area(c) == int(want.sum()) and S.box(c, H, W) == S.dense_box(want), c
    counts, offsets, size = CE.rle_flatten(rles)
    assert size == (H, W) and np.array_equal(S.unpack(counts, offsets, H, W)[0], host != 0)
    assert np.array_equal(S.pack_bits(host)[:, :, 0] & 1, host[:, :, 0])      # bit 0 of word 0 is column 0


def test_status_precedence_offsets_then_negative_then_sum():
    H, W = 3, 4
    counts = np.asarray([5, -1, 20, 2, 2, 13, 0, 6, 6, 2 ** 31 - 1, 2 ** 31 - 1], np.int64)
    #          mask:      0: negative AND too long | 1: ok | 2: sum 13 = H W + 1 | 3: sum 12 | 4: 2^32 - 2 (no wrap) | 5..7: offsets
    offsets = np.asarray([0, 3, 5, 6, 9, 11], np.int64)
    assert [S.status(counts, offsets, n, H, W) for n in range(5)] == [S.NEGATIVE, S.OK, S.TOO_LONG, S.OK, S.TOO_LONG]
    bad = np.asarray([-1, 2, 1, 12, 11], np.int64)                 # a negative start; a stretch that runs backwards; one past the total
    assert S.status(counts, bad, 0, H, W) == S.BAD_OFFSETS          # ... although its counts [-1 .. 2) would also be negative
    assert S.status(counts, bad, 1, H, W) == S.BAD_OFFSETS and S.status(counts, bad, 2, H, W) == S.BAD_OFFSETS
    assert S.status(counts, bad, 3, H, W) == S.BAD_OFFSETS
    masks, area, box, st = S.unpack(counts, offsets, H, W)
    assert st.tolist() == [1, 0, 2, 0, 2] and not masks[[0, 2, 4]].any() and area[[0, 2, 4]].tolist() == [0, 0, 0]
    assert box[0].tolist() == [-1] * 4 and area[1] == 2 and masks[1].sum() == 2 and area[3] == 6
    with pytest.raises(ValueError, match="RLE counts do not fit"):  # the host twin refuses the same lists
        CE.rle_decode([{"counts": [13], "size": [H, W]}])
    with pytest.raises(ValueError, match="RLE counts do not fit"):
        CE.rle_decode([{"counts": [5, -1, 2], "size": [H, W]}])


# ---- the string codec ---------------------------------------------------------------------------------------------------------------
# Derived by hand from the published rleToString (a value v, from the fourth on v - the value two places back, goes out in 5-bit groups,
# least significant first; a group c is followed by another unless the rest is 0 with c's bit 0x10 clear, or -1 with it set; the
# character is c + 48, + 32 when another group follows):
#   [6, 1]        6 = 00110b: bit 0x10 clear and the rest (6 >> 5) is 0 -> one group, chr(48 + 6) = "6"; 1 -> "1"
#   [0, 16]       0 -> "0"; 16 = 10000b: bit 0x10 is SET and the rest is 0, not -1 -> another group follows: chr(48 + 16 + 32) = "`",
#                 then group 0 with rest 0 -> "0": a lone 16 would read back as -16
#   [5, 3, 7, 1]  "5", "3", "7" as they are; the fourth value goes out as 1 - 3 = -2: -2 & 31 = 30 = 11110b, -2 >> 5 = -1, bit 0x10 set
#                 and the rest is -1 -> one group, chr(48 + 30) = "N"
VECTORS = (([6, 1], "61"), ([0, 16], "0`0"), ([5, 3, 7, 1], "537N"), ([0, 307200], "0PP\\9"), ([100000, 5, 207195], "PeQ35kZZ6"),
           ([3, 1, 3, 1, 3, 1, 500, 2], "313000a?1"))


def test_string_codec_vectors_round_trips_and_the_two_restatements():
    for counts, s in VECTORS:
        assert CE.rle_to_string(counts) == s == S.to_string(counts), counts
        assert CE.rle_from_string(s) == counts == S.from_string(s) == CE.rle_from_string(s.encode("ascii")), s
    assert CE.rle_to_string([]) == "" and CE.rle_from_string("") == []
    rng = np.random.default_rng(29)
    for trial in range(200):
        m = int(rng.integers(1, 30))
        hi = (2, 40, 5000, 2 ** 31)[trial % 4]
        counts = [int(v) for v in rng.integers(0, hi, m)]
        if trial % 7 == 0:
            counts[int(rng.integers(0, m))] = 2 ** 31 - 1
        s = CE.rle_to_string(counts)
        assert s == S.to_string(counts) and set(s) <= {chr(c) for c in range(48, 112)}
        assert CE.rle_from_string(s) == counts == S.from_string(s)
    for bad in ("0P", "12~", "1 2"):                               # ends inside a value; characters outside the alphabet
        with pytest.raises(ValueError):
            CE.rle_from_string(bad)


def test_rle_dicts_emit_compressed_strings_that_flatten_back(gold):
    H, W = 50, 70
    counts, offsets = recorded(gold, H, W)[:2]
    plain = CE.rle_dicts(torch.from_numpy(counts), torch.from_numpy(offsets), H, W)
    packed = CE.rle_dicts(torch.from_numpy(counts), torch.from_numpy(offsets), H, W, compress=True)
    assert all(isinstance(d["counts"], str) and d["size"] == [H, W] for d in packed) and packed[1]["counts"] == S.to_string([0, H * W])
    assert [d["counts"] for d in plain] == [counts[offsets[n]:offsets[n + 1]].tolist() for n in range(14)]
    for rles in (plain, packed, [dict(d, counts=d["counts"].encode("ascii")) for d in packed]):
        c, o, size = CE.rle_flatten(rles)
        assert c.dtype == np.int32 and o.dtype == np.int64 and size == (H, W)
        assert np.array_equal(c, counts) and np.array_equal(o, offsets)


# ---- one named case per clause of the rule ---------------------------------------------------------------------------------------
def test_tampering_strict_comparison_moves_every_run_by_one_pixel(gold):
    counts, offsets, back = recorded(gold, 31, 33)[:3]
    c = counts[offsets[4]:offsets[5]]
    assert np.array_equal(S.decode(c, 31, 33), back[4]) and not np.array_equal(S.decode(c, 31, 33, strict=True), back[4])
    assert S.decode([2, 1], 1, 4).tolist() == [[False, False, True, False]]       # pixel 2 = E_0 starts the set run
    assert S.decode([2, 1], 1, 4, strict=True).tolist() == [[False, False, False, True]]


def test_tampering_row_major_index_transposes_the_mask(gold):
    counts, offsets, back = recorded(gold, 50, 70)[:3]
    c = counts[offsets[4]:offsets[5]]
    assert np.array_equal(S.decode(c, 50, 70), back[4]) and not np.array_equal(S.decode(c, 50, 70, row_major=True), back[4])
    assert S.decode([1, 2], 2, 3).tolist() == [[False, True, False], [True, False, False]]       # pixels 1, 2 = (y 1, x 0), (y 0, x 1)


def test_tampering_even_parity_inverts_the_full_mask(gold):
    counts, offsets, back = recorded(gold, 31, 33)[:3]
    c = counts[offsets[1]:offsets[2]]
    assert c.tolist() == [0, 31 * 33] and back[1].all() and S.decode(c, 31, 33).all() and not S.decode(c, 31, 33, parity=0).any()


def test_tampering_box_without_the_column_crossing_rule(gold):
    H, W = 31, 33
    counts, offsets, back, _, bbox = recorded(gold, H, W)
    c = counts[offsets[4]:offsets[5]]                              # rows H - 2, H - 1 of column 3, rows 0, 1 of column 4
    assert S.box(c, H, W) == [3, 0, 4, H - 1] == S.dense_box(back[4]) and bbox[4].tolist() == [3, 0, 2, H]
    assert S.box(c, H, W, crossing=False) == [3, 1, 4, H - 2]


def test_tampering_dropped_sign_extension_breaks_a_negative_difference():
    assert S.from_string("537N") == [5, 3, 7, 1] and S.from_string("537N", sign_extend=False) == [5, 3, 7, 33]
    assert CE.rle_from_string("537N") == [5, 3, 7, 1]


# ---- the host half -----------------------------------------------------------------------------------------------------------------
def test_rle_flatten_refusals_and_what_it_lets_through():
    ok = {"counts": [3, 2, 7], "size": [3, 4]}
    with pytest.raises(ValueError, match="every RLE must have size"):
        CE.rle_flatten([ok, {"counts": [12], "size": [4, 3]}])
    for big in (2 ** 31, -2 ** 31 - 1, 2 ** 70):
        with pytest.raises(ValueError, match="do not fit int32"):
            CE.rle_flatten([ok, {"counts": [1, big], "size": [3, 4]}])
    with pytest.raises(ValueError, match="do not fit int32"):      # a string whose value leaves int32
        CE.rle_flatten([{"counts": S.to_string([2 ** 31]), "size": [3, 4]}])
    with pytest.raises(ValueError):
        CE.rle_flatten([{"counts": "3~", "size": [3, 4]}])
    c, o, size = CE.rle_flatten([ok, {"counts": [], "size": [3, 4]}, {"counts": [5, -1, 2 ** 31 - 1], "size": (3, 4)}])
    assert c.tolist() == [3, 2, 7, 5, -1, 2 ** 31 - 1] and o.tolist() == [0, 3, 3, 6] and size == (3, 4)      # negative counts: the decoder's to name
    c, o, size = CE.rle_flatten([])
    assert c.shape == (0,) and c.dtype == np.int32 and o.tolist() == [0] and o.dtype == np.int64
    with pytest.raises(ValueError, match="compressed"):            # the host twin is as it was
        CE.rle_decode([{"counts": "61", "size": [1, 7]}])


def test_device_entry_points_have_no_cpu_fallback():
    counts, offsets = torch.tensor([3, 2], dtype=torch.int32), torch.tensor([0, 2], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CE.rle_unpack(counts, offsets, 3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CE.rle_stats(counts, offsets, 3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CE.pack_rles([{"counts": [3, 2], "size": [3, 4]}], "cpu")


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    p = C.c_void_p(4096)                                    # fake, aligned; never dereferenced: every call returns before a launch
    lib.cp_kernel_log_begin()

    def un(counts=p, off=p, N=3, H=31, W=33, total=10, ends=p, bits=p, area=p, box=p, status=p):
        return lib.cp_coco_rle_unpack(None, counts, off, N, H, W, total, ends, bits, area, box, status)
    for name in ("counts", "off", "ends", "area", "box", "status"):
        assert un(**{name: None}) == -1, name
    assert un(N=0) == -1 and un(H=0) == -1 and un(W=0) == -1 and un(W=-3) == -1 and un(total=-1) == -1
    for name in ("counts", "ends", "bits", "area", "box", "status"):
        assert un(**{name: C.c_void_p(4098)}) == -3, name
    assert un(off=C.c_void_p(4100)) == -3
    assert un(H=1 << 16, W=1 << 15) == -4 and un(H=1, W=2 ** 31 - 4096) == -4 and un(N=1 << 24) == -4 and un(total=1 << 31) == -4
    assert un(N=(1 << 24) - 1, H=4096, W=4096) == -4               # 2^34 workgroups in the bits launch
    assert un(H=0, area=C.c_void_p(4098)) == -1 and un(N=1 << 24, area=C.c_void_p(4098)) == -3      # INVALID, then ALIGN, then RANGE
    assert lib.cp_kernel_log() == b""
    assert lib.cp_coco_rle_unpack_scratch_bytes(0) == 0 and lib.cp_coco_rle_unpack_scratch_bytes(-4) == 0
    assert lib.cp_coco_rle_unpack_scratch_bytes(19042) == 4 * 19042 and lib.cp_coco_rle_unpack_scratch_bytes(2 ** 31 - 1) == 4 * (2 ** 31 - 1)
    assert lib.cp_version() >= 239
