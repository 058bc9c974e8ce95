"""CPU: the host side of checkerpose_amd.augment and the numpy restatement tests/augment_stages.py that the
device is held to: hand-worked answers, an independent cross-check of the Gaussian, the statistics of sample_plan and of the hash, and
the mutations of the statement that the cases must catch."""
import numpy as np
import pytest

from checkerpose_amd import augment as A
from tests import augment_stages as S

ROW = np.array([10, 20, 30, 40, 50], dtype=np.uint8).reshape(1, 5, 1)
W5 = np.array([256, 1024, 1536, 1024, 256])
ROW_HSUM = [71680, 87040, 122880, 158720, 174080]              # by hand: x = 0 reads 30 20 10 20 30, x = 4 reads 30 40 50 40 30, ...

SIGMAS = (1e-3, 0.05, 0.3, 0.5, 0.77, 1.0, 1.2, 1.4999)
MOTIONS = [(a, d) for a in (0.0, 17.0, 45.0, 90.0, 133.3, 270.0, 359.9) for d in (-0.99, -0.3, 0.0, 0.5, 0.99)]


def test_five_tap_row_with_reflect_101():
    assert S.gauss_hsum(ROW, W5)[0, :, 0].tolist() == ROW_HSUM
    assert S.border_index(5, 2).tolist() == [2, 1, 0, 1, 2, 3, 4, 3, 2]
    assert S.border_index(5, 4).tolist() == [4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0]


def test_constant_image_is_unchanged_by_every_quantised_kernel():
    for v in (0, 1, 127, 200, 255):
        img = np.full((7, 9, 3), v, dtype=np.uint8)
        for s in SIGMAS:
            w = A.gaussian_weights(s)
            assert w.sum() == 4096 and (w >= 0).all() and w[0] == w[4] and w[1] == w[3]
            assert np.array_equal(S.stage_gaussian(img, w), img), (v, s)
        for a, d in MOTIONS:
            w = A.motion_weights(a, d)
            assert w.sum() == 65536 and (w >= 0).all()
            assert np.array_equal(S.stage_motion(img, w), img), (v, a, d)


def test_gaussian_kernel_rule():
    assert A.gaussian_weights(0.0).tolist() == [0, 0, 4096, 0, 0] and A.gaussian_weights(9e-4).tolist() == [0, 0, 4096, 0, 0]
    with pytest.raises(ValueError):
        A.gaussian_weights(1.5)
    with pytest.raises(ValueError):
        A.gaussian_weights(-0.1)
    w = A.gaussian_weights(1.0)                    # exp(-2), exp(-1/2), 1 normalised: 0.05449, 0.24420, 0.40262
    assert w.tolist() == [223, 1000, 1650, 1000, 223]


def test_motion_kernel_rule():
    up = A.motion_weights(0.0, 0.0).reshape(5, 5)                 # direction 0: an even centre column
    assert (up[:, 2] > 13000).all() and up.sum() == 65536 and not up[:, [0, 1, 3, 4]].any()
    side = A.motion_weights(90.0, 0.0).reshape(5, 5)              # a quarter turn: the centre row
    assert (side[2] > 13000).all() and not side[[0, 1, 3, 4]].any()
    ramp = A.motion_weights(0.0, 0.8).reshape(5, 5)[:, 2]          # direction weights one end: linspace(0.9, 0.1)
    assert (np.diff(ramp) < 0).all() and abs(ramp[0] / 65536.0 - 0.9 / 2.5) < 1e-4


def test_lut_composition_by_hand():
    v = np.arange(256)
    add = A.compose_lut(add=[20, -20, 0])
    assert add[0, 250] == 255 and add[0, 10] == 30 and add[1, 10] == 0 and add[1, 250] == 230 and (add[2] == v).all()      # both clip ends
    im = A.compose_lut(invert=[True, False, False], mul_pc=[1.5, 1.5, 0.5])
    assert im[0, 100] == 232                        # Invert THEN Multiply: (255 - 100) * 1.5 = 232.5 -> 232, not 255 - 150 = 105
    assert im[1, 100] == 150 and im[1, 200] == 255 and im[2, 201] == 100               # truncation, clip
    c = A.compose_lut(contrast=[2.0, 0.5, 1.0])
    assert c[0, 200] == 255 and c[0, 60] == 0 and c[0, 130] == 132 and c[1, 255] == 191 and c[1, 0] == 64 and (c[2] == v).all()
    chain = A.compose_lut(add=[10, 10, 10], invert=[True, True, True], mul_pc=[0.5, 0.5, 0.5], mul=2.0, contrast=[0.5, 0.5, 0.5])
    # 250 -> 255 (clip) -> 0 -> 0 -> 0 -> 64;   40 -> 50 -> 205 -> 102 -> 204 -> 166
    assert chain[0, 250] == 64 and chain[1, 40] == 166
    assert (A.compose_lut() == v).all()


def test_dropout_cells_by_hand():
    assert A.dropout_grid(33, 31) == (3, 3) and A.dropout_grid(480, 640) == (24, 32) and A.dropout_grid(5, 5) == (3, 3)
    cy, cx = S.dropout_cells(33, 3), S.dropout_cells(31, 3)
    assert [cy[i] for i in (0, 10, 11, 21, 22, 32)] == [0, 0, 1, 1, 2, 2]
    assert [cx[i] for i in (0, 10, 11, 20, 21, 30)] == [0, 0, 1, 1, 2, 2]                      # 20 * 3 / 31 = 1.94, 21 * 3 / 31 = 2.03
    cy, cx = S.dropout_cells(480, 24), S.dropout_cells(640, 32)
    assert [cy[i] for i in (0, 19, 20, 239, 240, 479)] == [0, 0, 1, 11, 12, 23]
    assert [cx[i] for i in (19, 20, 639)] == [0, 1, 31]
    for n, g in ((33, 3), (31, 3), (480, 24), (640, 32), (5, 3), (120, 6), (160, 8)):          # the kernel's exact integer form
        assert np.array_equal(S.dropout_cells(n, g), np.minimum(np.arange(n) * g // n, g - 1))


def test_gaussian_against_scipy():
    """independent implementation: scipy.ndimage.gaussian_filter1d twice in float64, mirror = REFLECT_101, radius 2, renormalised by
    scipy itself.  One grey level: each separable pass of the statement rounds once and the weights are 12-bit."""
    from scipy.ndimage import gaussian_filter1d
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(23, 17, 3), dtype=np.uint8)
    img[5:9, 3:8] = 255
    img[12:14] = 0
    for s in (0.05, 0.3, 0.5, 0.77, 1.0, 1.2, 1.4999):
        ref = img.astype(np.float64)
        for axis in (1, 0):
            ref = gaussian_filter1d(ref, s, axis=axis, mode="mirror", truncate=2.0 / s)
        got = S.stage_gaussian(img, A.gaussian_weights(s)).astype(np.float64)
        assert np.abs(got - ref).max() <= 1.0, (s, np.abs(got - ref).max())


@pytest.fixture(scope="module")
def big_plan():
    return A.sample_plan(20000, np.random.default_rng(2024), use_peper_salt=True, use_motion_blur=True, change_bg=0.25, n_bg=7,
                         frame_hw=(480, 640))


def test_plan_statistics(big_plan):
    p, n = big_plan, 20000
    rates = {"sp_on": A.P_SP, "motion_on": A.P_MOTION, "drop_on": A.P_DROP, "gauss_on": A.P_GAUSS, "add_on": A.P_ADD, "invert_on": A.P_INVERT,
             "mul_pc_on": A.P_MUL_PC, "mul_on": A.P_MUL, "contrast_on": A.P_CONTRAST}
    for name, q in rates.items():
        q *= 0.8
        rate, sd = float(getattr(p, name).mean()), np.sqrt(q * (1 - q) / n)
        assert abs(rate - q) <= 5 * sd, (name, rate, q, sd)
    assert abs(p.color_on.mean() - 0.8) <= 5 * np.sqrt(0.16 / n) and abs((p.bg_index >= 0).mean() - 0.25) <= 5 * np.sqrt(0.1875 / n)
    assert p.bg_index.min() == -1 and p.bg_index.max() == 6 and p.key.dtype == np.uint32 and len(np.unique(p.key)) > n - 10
    assert (p.gauss_w.sum(1) == 4096).all() and (p.motion_w.sum(1) == 65536).all() and (p.gauss_w >= 0).all() and (p.motion_w >= 0).all()
    assert (p.add >= -20).all() and (p.add <= 20).all() and p.add.min() == -20 and p.add.max() == 20
    for f in (p.mul_pc, p.mul):
        assert (f[f != 1.0] >= 0.7).all() and (f <= 1.4).all()
    assert (p.contrast[p.contrast_on == 1] >= 0.5).all() and (p.contrast <= 2.0).all()
    assert (p.sigma >= 0).all() and (p.sigma < 1.0).all() and (p.angle >= 0).all() and (p.angle < 360).all() and (np.abs(p.direction) < 1).all()
    assert (p.sp_thresh[p.sp_on == 1] == int(0.05 * 2 ** 32)).all() and (p.drop_thresh[p.drop_on == 1] == int(0.1 * 2 ** 32)).all()
    assert (p.drop_grid == [24, 32]).all()
    # per_channel=q: the share of three-different draws among the switched-on samples
    for vals, on, q in ((p.add, p.add_on, 0.3 * (1 - 1 / 41 ** 2)), (p.mul_pc, p.mul_pc_on, 0.8), (p.contrast, p.contrast_on, 0.3)):
        if q is not None:
            share = float((np.ptp(vals[on == 1], axis=1) > 0).mean())
            assert abs(share - q) <= 5 * np.sqrt(q * (1 - q) / int((on == 1).sum())), (share, q)
    failed = p.color_on == 0                       # a sample that failed the 0.8 draw: every colour op off, identity tables
    ident = A.AugmentPlan.identity(n, (480, 640))
    for k in ("sp_on", "motion_on", "drop_on", "gauss_on", "lut", "motion_w", "gauss_w"):
        assert np.array_equal(getattr(p, k)[failed], getattr(ident, k)[failed]), k
    assert p.is_identity()[failed & (p.bg_index < 0)].all() and A.AugmentPlan.identity(5).is_identity().all()
    sub = p.select([7, 3, 7])
    assert sub.B == 3 and sub.key[0] == p.key[7] == sub.key[2] and np.array_equal(sub.lut[1], p.lut[3])
    off = A.sample_plan(200, np.random.default_rng(1), frame_hw=(50, 70))              # the switches' defaults: no optional op
    assert not off.sp_on.any() and not off.motion_on.any() and (off.bg_index == -1).all() and (off.drop_grid == [3, 3]).all()
    forced = A.sample_plan(4, np.random.default_rng(1), change_bg=np.array([True, False, True, True]), n_bg=3, frame_hw=(50, 70))
    assert ((forced.bg_index >= 0) == [True, False, True, True]).all()
    with pytest.raises(ValueError):
        A.sample_plan(4, np.random.default_rng(1), change_bg=1.0, n_bg=0)


def test_pack_plan_layout():
    p = A.sample_plan(5, np.random.default_rng(3), True, True, change_bg=1.0, n_bg=2, frame_hw=(120, 160))
    blob = A.pack_plan(p, np.arange(5, dtype=np.int32), np.arange(20).reshape(5, 4))
    assert blob.dtype == np.uint8 and blob.nbytes == 256 + 5 * 944 and np.array_equal(blob[:256], A.sp_value_table())
    rec = blob[256:].reshape(5, 944)
    words = rec[:, :176].copy().view(np.int32)
    assert np.array_equal(words[:, 0].view(np.uint32), p.key) and np.array_equal(words[:, 2], p.bg_index) and words[:, 3].tolist() == [0, 1, 2, 3, 4]
    assert np.array_equal(words[:, 8:12], np.arange(20).reshape(5, 4)) and np.array_equal(words[:, 12:17], p.gauss_w)
    assert np.array_equal(words[:, 17:42], p.motion_w) and np.array_equal(rec[:, 176:].reshape(5, 3, 256), p.lut)
    assert ((words[:, 1] & 32) == 32).all() and np.array_equal((words[:, 1] & 8) != 0, p.gauss_on != 0)
    assert not (A.pack_plan(A.AugmentPlan.identity(2), [0, 0])[256:].reshape(2, 944)[:, 4:8].view(np.int32)).any()      # flags 0, no rect


def test_abi(lib):
    assert lib.cp_version() >= 214 and lib.cp_augment_plan_bytes(5) == 256 + 5 * 944 and lib.cp_augment_plan_bytes(0) == 0
    P = 0x10000
    assert lib.cp_augment_frames(None, P, 1, 4, 9, None, None, 0, P, 1, P) == -1                 # H < 5
    assert lib.cp_augment_frames(None, P, 1, 9, 9, None, None, 2, P, 1, P) == -1                 # a pool size without a pool
    assert lib.cp_augment_frames(None, P, 1, 9, 9, None, None, 0, P + 4, 1, P) == -3             # the plan blob must be 16-byte aligned
    assert lib.cp_augment_frames(None, None, 1, 9, 9, None, None, 0, P, 1, P) == -1
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.augment_frames(torch.zeros(1, 9, 9, 3, dtype=torch.uint8), A.AugmentPlan.identity(1))


def test_hash_statistics():
    H, W, key = 120, 160, 0xC0FFEE11
    y, x = np.mgrid[0:H, 0:W]
    hit = S.hash_u32(key, S.OP_SP, y, x) < np.uint64(A.threshold_u32(0.05))
    n = H * W
    assert abs(int(hit.sum()) - 0.05 * n) <= 5 * np.sqrt(n * 0.05 * 0.95), int(hit.sum())
    img = np.full((H, W, 3), 128, dtype=np.uint8)
    out = S.stage_salt_pepper(img, key, int(A.threshold_u32(0.05)), A.sp_value_table())
    changed = (out != 128).any(-1)
    assert (out[..., 0] == out[..., 1]).all() and (out[..., 1] == out[..., 2]).all()      # a pixel is replaced in all channels
    assert changed.sum() <= hit.sum() and changed.sum() >= hit.sum() - 10                  # (a replacement may itself be 128)
    vals = out[..., 0][hit]
    ends, middle = int(((vals < 32) | (vals >= 224)).sum()), int(((vals >= 96) & (vals < 160)).sum())
    assert ends > middle, (ends, middle)                                                  # U-shaped: the arcsine law
    tab = A.sp_value_table()
    assert tab[0] == 0 and tab[255] == 254 and (np.diff(tab.astype(int)) >= 0).all() and int(tab[127]) in (126, 127, 128)
    other = S.hash_u32(key + 1, S.OP_SP, y, x) < np.uint64(A.threshold_u32(0.05))          # another key, another pattern
    assert (hit & other).sum() < 0.2 * hit.sum()
    assert int(S.fmix32(np.uint64(1))) == 0x514E28B7                                      # murmur3's finaliser, a published value


# ---- mutations of the statement: each must be told from the statement by a hand-worked case ------------------------------------
def _order_case():
    """5 x 5, 200 everywhere, 0 in the middle; Gaussian taps 0 1024 2048 1024 0; table = Multiply 1.5.  By hand: the middle's
    horizontal sums are 819200 | 409600 | 819200 over the three rows -> (2516582400 + 2^23) >> 24 = 150 -> 150 * 1.5 = 225.
    The table first would give 255 / 0 -> 191."""
    plan = A.AugmentPlan.identity(1, (5, 5))
    plan.gauss_on[:] = 1
    plan.gauss_w[0] = [0, 1024, 2048, 1024, 0]
    plan.lut[0] = A.compose_lut(mul=1.5)
    frame = np.full((1, 5, 5, 3), 200, dtype=np.uint8)
    frame[0, 2, 2] = 0
    return frame, plan


def test_mutation_reflect_is_caught():
    assert S.gauss_hsum(ROW, W5, border="reflect")[0, :, 0].tolist() != ROW_HSUM
    assert S.gauss_hsum(ROW, W5, border="reflect")[0, 0, 0] == 58880               # by hand: x = 0 would read 20 10 10 20 30


def test_mutation_lut_before_blur_is_caught():
    frame, plan = _order_case()
    out = S.augment_stages(frame, plan)
    assert out[0, 2, 2].tolist() == [225, 225, 225] and out[0, 0, 0].tolist() == [255, 255, 255] and out[0, 2, 1].tolist() == [255] * 3
    assert S.augment_stages(frame, plan, lut_first=True)[0, 2, 2].tolist() == [191, 191, 191]


def test_mutation_round_cell_is_caught():
    assert S.dropout_cells(33, 3, use_round=True)[10] == 1 and S.dropout_cells(33, 3)[10] == 0
    assert S.dropout_cells(480, 24, use_round=True)[19] == 1 and S.dropout_cells(480, 24)[19] == 0


def test_mutation_background_where_mask_set_is_caught():
    frame = np.full((1, 5, 5, 3), 1, dtype=np.uint8)
    bgs = np.full((1, 5, 5, 3), 2, dtype=np.uint8)
    mask = np.zeros((1, 5, 5), dtype=np.uint8)
    mask[0, 1, 3] = 255
    plan = A.AugmentPlan.identity(1, (5, 5))
    plan.bg_index[:] = 0
    expect = np.full((5, 5, 3), 2, dtype=np.uint8)
    expect[1, 3] = 1                                                               # the object keeps the frame's pixel
    assert np.array_equal(S.augment_stages(frame, plan, mask, bgs)[0], expect)
    assert not np.array_equal(S.augment_stages(frame, plan, mask, bgs, bg_where_mask=True)[0], expect)


def test_mutation_dropout_per_channel_is_caught():
    img = np.full((33, 31, 3), 200, dtype=np.uint8)
    out = S.stage_dropout(img, 12345, int(A.threshold_u32(0.5)), 3, 3)
    assert ((out == 0).all(-1) | (out == 200).all(-1)).all() and (out == 0).any() and (out == 200).any()      # a cell goes in all channels
    cells = out[::11, ::11, 0][:3, :3]                                             # one value per cell: (11 rows) x (10.33 columns)
    assert np.array_equal(out[..., 0], cells[S.dropout_cells(33, 3)][:, S.dropout_cells(31, 3)])
    bad = S.stage_dropout(img, 12345, int(A.threshold_u32(0.5)), 3, 3, per_channel=True)
    assert not ((bad == 0).all(-1) | (bad == 200).all(-1)).all()
