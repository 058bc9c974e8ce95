"""Row N29 (csrc/rle_unpack.hip; checkerpose_amd.coco_eval.rle_unpack) restated in numpy: the decoding rule, area and box from the
runs, the status, and pycocotools' string codec written a second way.  The keyword switches are the TAMPERINGS of
tests/test_rle_unpack.py: each turns one clause of the rule into the slip it guards against; the defaults are the rule.

Mask n has m run lengths c_0 .. c_{m-1}; E_j = c_0 + ... + c_j (64-bit); pixel i = x H + y (column-major) has k(i) = #{ j : E_j <= i }
and is set iff k < m and k is odd."""
import numpy as np

OK, NEGATIVE, TOO_LONG, BAD_OFFSETS = 0, 1, 2, 3


def decode(counts, H, W, strict=False, row_major=False, parity=1):
    """the rule -> (H, W) bool.  strict: E_j < i instead of <=; row_major: i = y W + x; parity 0: even instead of odd"""
    E = np.cumsum(np.asarray(counts, np.int64).reshape(-1))
    m = len(E)
    i = np.arange(H * W, dtype=np.int64)
    k = np.searchsorted(E, i, side="left" if strict else "right")      # right: #{E_j <= i}; left: #{E_j < i}
    flat = (k < m) & (k % 2 == parity)
    return flat.reshape(H, W) if row_major else flat.reshape(W, H).T


def area(counts):
    return int(np.asarray(counts, np.int64).reshape(-1)[1::2].sum())


def box(counts, H, W, crossing=True):
    """xmin ymin xmax ymax from the runs, -1s for an empty mask.  crossing False: a run that goes over a column boundary adds only its
    first and last row instead of rows 0 and H - 1"""
    c = np.asarray(counts, np.int64).reshape(-1)
    E = np.cumsum(c)
    x0 = y0 = None
    x1 = y1 = -1
    for k in range(1, len(c), 2):
        if c[k] <= 0:
            continue
        s, e = int(E[k] - c[k]), int(E[k])
        xa, xb = s // H, (e - 1) // H
        ra, rb = s - xa * H, e - 1 - xb * H
        if xa != xb:
            ra, rb = (0, H - 1) if crossing else (min(ra, rb), max(ra, rb))
        x0 = xa if x0 is None else min(x0, xa)
        y0 = ra if y0 is None else min(y0, ra)
        x1, y1 = max(x1, xb), max(y1, rb)
    return [-1, -1, -1, -1] if x0 is None else [x0, y0, x1, y1]


def status(counts, offsets, n, H, W):
    """the status of mask n of a batch (counts, offsets): the offsets first, then a negative count, then the sum"""
    total = len(counts)
    a, b = int(offsets[n]), int(offsets[n + 1])
    if a < 0 or b < a or b > total:
        return BAD_OFFSETS
    c = np.asarray(counts[a:b], np.int64)
    if (c < 0).any():
        return NEGATIVE
    return TOO_LONG if int(c.sum()) > H * W else OK


def dense_box(mask):
    """cp_coco_pack's box of a dense mask"""
    ys, xs = np.nonzero(mask)
    return [-1, -1, -1, -1] if len(xs) == 0 else [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def unpack(counts, offsets, H, W):
    """the whole call -> (masks (N,H,W) bool, area (N,), box (N,4), status (N,)); a mask with a nonzero status is empty"""
    N = len(offsets) - 1
    masks, areas, boxes, st = np.zeros((N, H, W), bool), np.zeros(N, np.int64), np.full((N, 4), -1, np.int64), np.zeros(N, np.int64)
    for n in range(N):
        st[n] = status(counts, offsets, n, H, W)
        if st[n] == OK:
            c = counts[int(offsets[n]):int(offsets[n + 1])]
            masks[n], areas[n], boxes[n] = decode(c, H, W), area(c), box(c, H, W)
    return masks, areas, boxes, st


def pack_bits(masks):
    """cp_coco_pack's words of (N,H,W) masks -> (N,H,WW) int32: bit x & 31 of word x >> 5, zero past W"""
    m = np.asarray(masks) != 0
    N, H, W = m.shape
    WW = (W + 31) // 32
    padded = np.zeros((N, H, WW * 32), bool)
    padded[:, :, :W] = m
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    words = (padded.reshape(N, H, WW, 32).astype(np.uint64) * weights).sum(-1)
    return words.astype(np.uint32).view(np.int32)


# ---- pycocotools' rleToString / rleFrString, written the arithmetic way: a value (from the fourth on: its difference against the value
# two places back) is sent as the smallest number g of 5-bit groups whose two's-complement range [-2^(5g-1), 2^(5g-1)) holds it, least
# significant group first, each group + 48 as a character and + 32 more when another group follows
def to_string(counts):
    counts = [int(v) for v in counts]
    out = ""
    for i, v in enumerate(counts):
        d = v - counts[i - 2] if i > 2 else v
        g = 1
        while not -(1 << (5 * g - 1)) <= d < (1 << (5 * g - 1)):
            g += 1
        u = d % (1 << (5 * g))                                     # the two's complement in 5 g bits
        for j in range(g):
            out += chr(48 + ((u >> (5 * j)) & 31) + (32 if j < g - 1 else 0))
    return out


def from_string(s, sign_extend=True):
    """sign_extend False: the tampering -- the top bit of the last group is taken as a magnitude bit"""
    if isinstance(s, bytes):
        s = s.decode("ascii")
    vals, groups = [], []
    for ch in s:
        c = ord(ch) - 48
        groups.append(c & 31)
        if c & 32:
            continue
        g = len(groups)
        u = sum(v << (5 * j) for j, v in enumerate(groups))
        if sign_extend and u >= 1 << (5 * g - 1):
            u -= 1 << (5 * g)
        groups = []
        vals.append(u + vals[-2] if len(vals) > 2 else u)
    return vals
