"""numpy restatement of checkerpose_amd/csrc/augment.hip: what cp_augment_frames must give bit for bit, one stage
at a time, written for clarity (whole-frame numpy, no tiles).  Shared by tests/test_augment.py (known answers, statistics, the
mutations below) and tests/test_gpu_augment.py (the device against it).

The keyword switches of `augment_stages` / the stage functions are MUTATIONS of the statement -- ways an implementation could plausibly
go wrong -- that the CPU tests must tell from the statement itself; the default of each is the statement."""
import numpy as np

OP_SP, OP_SP_VALUE, OP_DROP = 1, 2, 3
M32 = np.uint64(0xFFFFFFFF)


def fmix32(h):
    """murmur3's finaliser on uint64 arrays holding 32-bit values"""
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def hash_u32(key, op, a, b):
    """hash(key, op, a, b) of the kernel's header; a, b broadcastable non-negative integer arrays -> uint64 array of 32-bit values"""
    s = fmix32(np.uint64(int(key) & 0xFFFFFFFF) ^ np.uint64((op * 0x9E3779B9) & 0xFFFFFFFF))
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    t = fmix32(s ^ ((a * np.uint64(0x85EBCA6B) + np.uint64(0x165667B1)) & M32))
    return fmix32(t ^ ((b * np.uint64(0xC2B2AE35) + np.uint64(0x27D4EB2F)) & M32))


def border_index(n, r, border="reflect101"):
    """source indices of positions -r .. n - 1 + r: BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba), or the mutation BORDER_REFLECT
    (fedcba|abcdefgh|hgfedcb)"""
    p = np.arange(-r, n + r)
    if border == "reflect101":
        p = np.abs(p)
        return np.where(p >= n, 2 * n - 2 - p, p)
    p = np.where(p < 0, -p - 1, p)
    return np.where(p >= n, 2 * n - 1 - p, p)


def stage_background(frame, mask, bg, bg_where_mask=False):
    """replace_bg: the background wherever the visible mask is zero"""
    keep = (mask != 0) if not bg_where_mask else (mask == 0)
    return np.where(keep[..., None], frame, bg).astype(np.uint8)


def stage_salt_pepper(img, key, thresh, table):
    H, W = img.shape[:2]
    y, x = np.mgrid[0:H, 0:W]
    hit = hash_u32(key, OP_SP, y, x) < np.uint64(thresh)
    val = table[(hash_u32(key, OP_SP_VALUE, y, x) >> np.uint64(24)).astype(np.int64)]
    return np.where(hit[..., None], val[..., None], img).astype(np.uint8)


def stage_motion(img, w25, border="reflect101"):
    H, W = img.shape[:2]
    iy, ix = border_index(H, 2, border), border_index(W, 2, border)
    ext = img[iy][:, ix].astype(np.int64)
    acc = np.zeros(img.shape, dtype=np.int64)
    for dy in range(5):
        for dx in range(5):
            acc += int(w25[dy * 5 + dx]) * ext[dy:dy + H, dx:dx + W]
    return ((acc + 32768) >> 16).astype(np.uint8)


def dropout_cells(n, g, use_round=False):
    """the grid cell of each of n pixels on a grid of g cells: min(floor(i * g / n), g - 1), in double"""
    q = np.arange(n, dtype=np.float64) * g / n
    return np.minimum((np.rint(q) if use_round else np.floor(q)).astype(np.int64), g - 1)


def stage_dropout(img, key, thresh, gh, gw, use_round=False, per_channel=False):
    H, W = img.shape[:2]
    cy, cx = dropout_cells(H, gh, use_round)[:, None], dropout_cells(W, gw, use_round)[None, :]
    if per_channel:
        drop = np.stack([hash_u32(key, OP_DROP + 16 * c, cy, cx) < np.uint64(thresh) for c in range(3)], -1)
    else:
        drop = np.broadcast_to((hash_u32(key, OP_DROP, cy, cx) < np.uint64(thresh))[..., None], img.shape)
    return np.where(drop, 0, img).astype(np.uint8)


def gauss_hsum(img, w5, border="reflect101"):
    """the horizontal pass: exact integer sums (H, W, C) int64"""
    W = img.shape[1]
    ext = img[:, border_index(W, 2, border)].astype(np.int64)
    return sum(int(w5[k]) * ext[:, k:k + W] for k in range(5))


def stage_gaussian(img, w5, border="reflect101"):
    H = img.shape[0]
    hs = gauss_hsum(img, w5, border)
    ext = hs[border_index(H, 2, border)]
    acc = sum(int(w5[k]) * ext[k:k + H] for k in range(5))
    return ((acc + (1 << 23)) >> 24).astype(np.uint8)


def stage_lut(img, lut):
    return np.stack([lut[c][img[..., c]] for c in range(3)], -1).astype(np.uint8)


def augment_sample(frame, plan, b, table, mask=None, backgrounds=None, border="reflect101", lut_first=False, cell_round=False,
                   bg_where_mask=False, drop_per_channel=False):
    """one sample through the chain: frame uint8 (H,W,3), row b of the plan's arrays"""
    img = frame
    if plan.bg_index[b] >= 0:
        img = stage_background(img, mask, backgrounds[plan.bg_index[b]], bg_where_mask)
    if lut_first:
        img = stage_lut(img, plan.lut[b])
    key = int(plan.key[b])
    if plan.sp_on[b]:
        img = stage_salt_pepper(img, key, int(plan.sp_thresh[b]), table)
    if plan.motion_on[b]:
        img = stage_motion(img, plan.motion_w[b], border)
    if plan.drop_on[b]:
        img = stage_dropout(img, key, int(plan.drop_thresh[b]), int(plan.drop_grid[b, 0]), int(plan.drop_grid[b, 1]), cell_round,
                            drop_per_channel)
    if plan.gauss_on[b]:
        img = stage_gaussian(img, plan.gauss_w[b], border)
    return img if lut_first else stage_lut(img, plan.lut[b])


def augment_stages(frames, plan, masks=None, backgrounds=None, img_index=None, **mutations):
    """augment_frames on host arrays: frames uint8 (n_img,H,W,3), masks (n_img,H,W), backgrounds (n_bg,H,W,3) -> uint8 (B,H,W,3)"""
    from checkerpose_amd.augment import sp_value_table
    table = sp_value_table()
    B = plan.B
    idx = np.arange(B) % len(frames) if img_index is None else np.asarray(img_index)
    return np.stack([augment_sample(frames[idx[b]], plan, b, table, None if masks is None else masks[idx[b]], backgrounds, **mutations)
                     for b in range(B)])
