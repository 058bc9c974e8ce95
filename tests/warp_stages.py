"""Row N21 restated in numpy: cv2.warpAffine's 8-bit arithmetic (OpenCV's published imgwarp.cpp: invertAffineTransform, the
AB_BITS = 10 / INTER_BITS = 5 fixed point of WarpAffineInvoker, remap's 15-bit bilinear weights, BORDER_CONSTANT 0) as the rule at the top
of checkerpose_amd/csrc/warp_affine.hip states it.  int64 for the fixed point, float64 with every product and sum rounded on its own.
The oracle of tests/test_gpu_warp.py; tests/test_warp.py checks it against properties that do not come from this restatement, and its
four switches (`mutate=`) are the mistakes those properties must catch.

cv2 itself is not available where this runs: parity with cv2's own bytes is UNPINNED."""
import numpy as np

INTER_NEAREST, INTER_LINEAR = 0, 1
AB_BITS, INTER_BITS = 10, 5
AB_SCALE = 1 << AB_BITS
MUTATIONS = ("half_pixel", "wrong_rd", "truncate", "clamp_edge")


def invert(M):
    """invertAffineTransform of a (2, 3) forward matrix -> the six doubles a00 a01 b0 a10 a11 b1"""
    M = np.asarray(M, dtype=np.float64).reshape(2, 3)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    a00, a01, a10, a11 = M[1, 1] * D, M[0, 1] * -D, M[1, 0] * -D, M[0, 0] * D
    p, q = a00 * M[0, 2], a01 * M[1, 2]
    r, s = a10 * M[0, 2], a11 * M[1, 2]
    return np.array([a00, a01, -p - q, a10, a11, -r - s])


def _sat(v, truncate):
    """saturate_cast<int>: round half to even (the `truncate` mutation: toward zero), clamped to int32"""
    v = np.trunc(v) if truncate else np.rint(v)
    return np.clip(v, -2147483648.0, 2147483647.0).astype(np.int64)


def fixed_coords(inv, out_w, out_h, interpolation, mutate=()):
    """(X, Y), int64 (out_h, out_w): X0[y] + adelta[x] and Y0[y] + bdelta[x]"""
    a00, a01, b0, a10, a11, b1 = (float(v) for v in inv)
    if "half_pixel" in mutate:              # sample at A . (x + 1/2, y + 1/2) + b - 1/2, as a resize would
        b0 = b0 + 0.5 * a00 + 0.5 * a01 - 0.5
        b1 = b1 + 0.5 * a10 + 0.5 * a11 - 0.5
    rd = AB_SCALE // 2 if interpolation == INTER_NEAREST else AB_SCALE // (1 << INTER_BITS) // 2
    if "wrong_rd" in mutate:
        rd = 0
    t = "truncate" in mutate
    x, y = np.arange(out_w, dtype=np.float64), np.arange(out_h, dtype=np.float64)
    adelta, bdelta = _sat(a00 * x * AB_SCALE, t), _sat(a10 * x * AB_SCALE, t)
    px, py = a01 * y, a11 * y                # the product, then the sum: two roundings
    X0, Y0 = _sat((px + b0) * AB_SCALE, t) + rd, _sat((py + b1) * AB_SCALE, t) + rd
    return X0[:, None] + adelta[None, :], Y0[:, None] + bdelta[None, :]


def _taps(img, sy, sx, clamp_edge):
    """img (H, W, C) at integer positions (sy, sx) of any shape -> int64 (..., C); zero outside the frame (`clamp_edge`: the edge pixel)"""
    H, W = img.shape[:2]
    inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    v = img[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)].astype(np.int64)
    return v if clamp_edge else v * inside[..., None]


def warp(img, M, out_size, interpolation=INTER_LINEAR, inverse_map=False, mutate=()):
    """cv2.warpAffine(img, M, out_size, flags=interpolation [| WARP_INVERSE_MAP]) with BORDER_CONSTANT 0.
    img uint8 (H, W, C) or (H, W); M (2, 3), or None / holding a NaN for "no box" (a zero crop); out_size an int or (w, h)
    -> uint8 (h, w, C) (the channel axis of a (H, W) image is dropped again)"""
    out_w, out_h = (int(out_size), int(out_size)) if np.ndim(out_size) == 0 else (int(out_size[0]), int(out_size[1]))
    flat = img.ndim == 2
    img3 = img[..., None] if flat else img
    if M is None or np.isnan(np.asarray(M, dtype=np.float64)).any():
        out = np.zeros((out_h, out_w, img3.shape[2]), np.uint8)
        return out[..., 0] if flat else out
    inv = np.asarray(M, dtype=np.float64).reshape(6) if inverse_map else invert(M)
    X, Y = fixed_coords(inv, out_w, out_h, interpolation, mutate)
    ce = "clamp_edge" in mutate
    if interpolation == INTER_NEAREST:
        out = _taps(img3, Y >> AB_BITS, X >> AB_BITS, ce)
    else:
        X, Y = X >> (AB_BITS - INTER_BITS), Y >> (AB_BITS - INTER_BITS)
        sx, sy, fx, fy = X >> INTER_BITS, Y >> INTER_BITS, (X & 31)[..., None], (Y & 31)[..., None]
        acc = ((32 - fy) * (32 - fx) * 32 * _taps(img3, sy, sx, ce) + (32 - fy) * fx * 32 * _taps(img3, sy, sx + 1, ce)
               + fy * (32 - fx) * 32 * _taps(img3, sy + 1, sx, ce) + fy * fx * 32 * _taps(img3, sy + 1, sx + 1, ce))
        out = (acc + 16384) >> 15
    out = out.astype(np.uint8)
    return out[..., 0] if flat else out


def warp_batch(images, mats, out_size, interpolation=INTER_LINEAR, inverse_map=False, img_index=None):
    """warp of every matrix of `mats` on image img_index[b] (default: image b, or the only image) of images (n_img, H, W, C)"""
    B = len(mats)
    idx = img_index if img_index is not None else ([0] * B if images.shape[0] == 1 else list(range(B)))
    return np.stack([warp(images[int(idx[b])], mats[b], out_size, interpolation, inverse_map) for b in range(B)])


def bilinear_exact(img, inv, out_w, out_h):
    """float64 bilinear sampling of the zero-padded image at A . (x, y) + b, and the bound's G: the largest difference between
    horizontally or vertically adjacent pixels in the 4 x 4 neighbourhood (rows / columns floor - 1 .. floor + 2) of the source point
    -> (values (h, w, C), G (h, w))"""
    H, W = img.shape[:2]
    a00, a01, b0, a10, a11, b1 = (float(v) for v in inv)
    pad = np.zeros((H + 8, W + 8, img.shape[2]), np.float64)          # 4 zero pixels all round: every read below stays inside
    pad[4:-4, 4:-4] = img
    y, x = np.mgrid[0:out_h, 0:out_w].astype(np.float64)
    u, v = a00 * x + a01 * y + b0, a10 * x + a11 * y + b1
    far = (u < -2) | (u > W + 1) | (v < -2) | (v > H + 1)              # the whole neighbourhood is zero padding there
    uc, vc = np.clip(u, -2, W + 1), np.clip(v, -2, H + 1)
    iu, iv = np.floor(uc).astype(np.int64), np.floor(vc).astype(np.int64)
    fu, fv = (uc - iu)[..., None], (vc - iv)[..., None]
    at = lambda dy, dx: pad[iv + 4 + dy, iu + 4 + dx]      # noqa: E731
    val = (1 - fv) * ((1 - fu) * at(0, 0) + fu * at(0, 1)) + fv * ((1 - fu) * at(1, 0) + fu * at(1, 1))
    G = np.zeros(u.shape)
    for dy in range(-1, 3):
        for dx in range(-1, 3):
            if dx < 2:
                G = np.maximum(G, np.abs(at(dy, dx + 1) - at(dy, dx)).max(-1))
            if dy < 2:
                G = np.maximum(G, np.abs(at(dy + 1, dx) - at(dy, dx)).max(-1))
    val[far], G[far] = 0.0, 0.0
    return val, G


# ---- properties that do not come from the restatement above: plain slices, np.rot90, hand-worked values, exact bilinear sampling.
# Each takes warp_fn(img (H, W, C), M (2, 3), out_size, interpolation, inverse_map) -> uint8 (h, w, C) -- warp() above, a mutation of it, or
# the device's warp_affine -- and gat = the product's get_affine_transform; each returns the list of the cases that failed.
def property_image(H=48, W=64, smooth=False):
    y, x = np.mgrid[0:H, 0:W]
    if smooth:          # slopes of up to 8 per pixel along both axes, with wrap-around edges: G is 8 over most of the frame
        return np.stack([(8 * x + 8 * y) % 256, (5 * x + 3 * y + 40) % 256, 128 + 100 * np.sin(x / 5.0) * np.cos(y / 7.0)], -1).astype(np.uint8)
    return np.random.default_rng(2100).integers(1, 256, size=(H, W, 3), dtype=np.uint8)


def padded_slice(img, y0, x0, h, w):
    """img[y0:y0 + h, x0:x0 + w] with zeros where it leaves the frame"""
    out = np.zeros((h, w) + img.shape[2:], img.dtype)
    ys, xs = np.arange(y0, y0 + h), np.arange(x0, x0 + w)
    ok_y, ok_x = (ys >= 0) & (ys < img.shape[0]), (xs >= 0) & (xs < img.shape[1])
    out[np.ix_(ok_y, ok_x)] = img[np.ix_(ys[ok_y], xs[ok_x])]
    return out


ORIGINS = ((10, 12, 8), (-3, 5, 8), (60, 44, 8), (20, -5, 16), (-40, -40, 8), (57, 3, 12))      # (x0, y0, n): inside, over each edge, off the frame


def slices_fail(warp_fn, gat):
    """scale 1 with an integer-aligned centre: the plain slice, zero-padded where it leaves the frame, for both interpolations"""
    img, bad = property_image(), []
    for x0, y0, n in ORIGINS:
        M = gat(np.array([x0 + n / 2.0, y0 + n / 2.0]), (float(n), float(n)), 0, (n, n))
        for interp in (INTER_NEAREST, INTER_LINEAR):
            if not np.array_equal(warp_fn(img, M, n, interp, False), padded_slice(img, y0, x0, n, n)):
                bad.append(("slice", x0, y0, n, interp))
    return bad


def half_pixel_fail(warp_fn, gat):
    """a centre on a half pixel in x: (a + b + 1) >> 1 of the two neighbours (INTER_LINEAR); INTER_NEAREST rounds the half up: b"""
    img, bad = property_image(), []
    for x0, y0, n in ORIGINS[:4]:
        M = gat(np.array([x0 + n / 2.0 + 0.5, y0 + n / 2.0]), (float(n), float(n)), 0, (n, n))
        a, b = padded_slice(img, y0, x0, n, n).astype(np.int64), padded_slice(img, y0, x0 + 1, n, n).astype(np.int64)
        if not np.array_equal(warp_fn(img, M, n, INTER_LINEAR, False), ((a + b + 1) >> 1).astype(np.uint8)):
            bad.append(("half_linear", x0, y0, n))
        if not np.array_equal(warp_fn(img, M, n, INTER_NEAREST, False), b.astype(np.uint8)):
            bad.append(("half_nearest", x0, y0, n))
    return bad


def rotations_fail(warp_fn, gat):
    """rot = 90, 180, 270, -90 at integer alignment: np.rot90 of the slice, exactly.  The output centre is (n / 2, n / 2), so the slice
    [x0, x0 + n) x [y0, y0 + n) lines up for the centres below (output pixel p reads c + L (p - n / 2), L the quarter turn)"""
    img, bad = property_image(), []
    for x0, y0, n in ORIGINS[:3]:
        h = n // 2
        for rot, k, c in ((90, 1, (x0 + h - 1, y0 + h)), (180, 2, (x0 + h - 1, y0 + h - 1)), (270, 3, (x0 + h, y0 + h - 1)), (-90, 3, (x0 + h, y0 + h - 1))):
            M = gat(np.array(c, dtype=np.float64), (float(n), float(n)), rot, (n, n))
            for interp in (INTER_NEAREST, INTER_LINEAR):
                if not np.array_equal(warp_fn(img, M, n, interp, False), np.rot90(padded_slice(img, y0, x0, n, n), k)):
                    bad.append(("rot", rot, x0, y0, n, interp))
    return bad


def bilinear_cases():
    """40 seeded cases: scales 4 to 40, any rotation, centres up to 10 pixels off the frame, outputs 8 x 8 and 16 x 12"""
    rng = np.random.default_rng(2121)
    return [((rng.uniform(-10, 74), rng.uniform(-10, 58)), rng.uniform(4, 40), rng.uniform(-180, 180), (8, 8) if i % 2 else (16, 12)) for i in range(40)]


def bilinear_bound_fail(warp_fn, gat):
    """INTER_LINEAR stays within 0.5 + 2 (1/64 + 1/512) G of exact float64 bilinear sampling of the zero-padded image: coordinates are
    rounded to 1/32 pixel (at most 1/64 + 1/1024 off per axis; 1/512 leaves slack), the interpolant's slope per axis is at most G, the
    final rounding adds 0.5"""
    img, bad = property_image(smooth=True), []
    for c, s, rot, out in bilinear_cases():
        M = gat(np.array(c), (s, s), rot, out)
        inv = np.linalg.inv(np.vstack([M, [0.0, 0.0, 1.0]]))[:2].reshape(6)          # not invert() above: numpy's own
        exact, G = bilinear_exact(img, inv, out[0], out[1])
        got = warp_fn(img, M, out, INTER_LINEAR, False).astype(np.float64)
        over = np.abs(got - exact).max(-1) - (0.5 + 2.0 * (1.0 / 64 + 1.0 / 512) * G)
        if (over > 1e-9).any():
            bad.append(("bilinear", c, s, rot, out, float(over.max())))
    return bad


def double_rounding_fail(warp_fn, gat):
    """hand-worked: the coordinate is rounded to 1/1024 pixel FIRST (half to even), then to the pixel / to 1/32 pixel (half up).
    INTER_NEAREST at x + 7 + 1/2 - 2^-12: 1024 times the offset is 7679.75 -> 7680, + 512 -> pixel x + 8 (one rounding would give x + 7).
    INTER_LINEAR at x + 7 + 1/64 - 2^-12: 7183.75 -> 7184, + 16 = 7200 = 32 * 225 -> fx = 1: (31 a + b + 16) >> 5 of pixels x + 7, x + 8."""
    img, bad = property_image(), []
    a, b = padded_slice(img, 4, 7, 8, 8).astype(np.int64), padded_slice(img, 4, 8, 8, 8).astype(np.int64)
    if not np.array_equal(warp_fn(img, np.array([[1.0, 0.0, 7.5 - 2.0 ** -12], [0.0, 1.0, 4.0]]), 8, INTER_NEAREST, True), b.astype(np.uint8)):
        bad.append(("double_nearest",))
    if not np.array_equal(warp_fn(img, np.array([[1.0, 0.0, 7.0 + 1.0 / 64 - 2.0 ** -12], [0.0, 1.0, 4.0]]), 8, INTER_LINEAR, True),
                          ((31 * a + b + 16) >> 5).astype(np.uint8)):
        bad.append(("double_linear",))
    return bad


PROPERTIES = (slices_fail, half_pixel_fail, rotations_fail, bilinear_bound_fail, double_rounding_fail)
