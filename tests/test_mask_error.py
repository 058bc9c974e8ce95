"""Row N12 (BOP's cus / cou_bb_proj / cou_mask / cou_bb), host side.  tests/golden/mask_error.npz holds what the REFERENCE's own
bop_toolkit_lib.pose_error.cus / cou_bb_proj returned when its renderer was a stub handing it the float64 oracle's depth, what
cou_mask / cou_bb returned on those renders' masks and boxes and on hand-made box pairs (tests/golden/make_golden_mask_error.py).
The numpy restatement of tests/mask_error_stages.py -- the yardstick of tests/test_gpu_mask_error.py, which cannot read the
reference -- reproduces every recorded value EXACTLY, and each mutation of a rule is caught by a named case."""
import ctypes as C
import inspect
import zlib

import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, bop_eval, metric
from tests import mask_error_stages as M
from tests import vsd_stages as S


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


def test_fixture_covers_what_the_issue_lists():
    g, meshes = M.fixture()
    n = len(g["names"])
    assert n >= 24 and [str(x) for x in g["mesh_names"]] == list(S.MESH_NAMES)
    for i, name in enumerate(S.MESH_NAMES):
        v, f = meshes[name]
        assert zlib.crc32(v.tobytes() + f.tobytes()) == int(g["mesh_crc"][i]), name
    sizes = {(int(w), int(h)) for w, h in zip(g["W"], g["H"])}
    assert (33, 31) in sizes and (160, 120) in sizes and any(w % 4 for w, _ in sizes) and any(w % 32 for w, _ in sizes)
    assert len(set(g["mesh"].tolist())) >= 8 and set(g["kgroup"].tolist()) == {0, 1, 2, 3}
    assert float(g["undecided"].max()) <= 0.05
    assert not g["sphere"].all() and g["sphere"].sum() >= 15
    assert g["raises"].sum() == 2 and g["behind"].sum() == 1
    for name in ("identical_box", "disjoint", "inside", "crosstile", "outside_est", "outside_both", "pixel", "column", "column_both", "touch",
                 "zeroarea", "halfbox_small", "behind", "k1", "diagonal"):
        M.case(name)


def test_numpy_restatement_reproduces_every_recorded_value_exactly():
    g, _ = M.fixture()
    for c in range(len(g["names"])):
        if g["behind"][c]:
            assert np.isnan(g["cus"][c]) and np.isnan(g["cou_bb_proj"][c])
            continue
        me, mg = M.layers(c)[:2]
        counts = M.counts_of(me, mg)
        assert counts == g["counts"][c].tolist(), c
        be, bg = M.box_of(me), M.box_of(mg)
        assert [be or [-1] * 4, bg or [-1] * 4] == g["boxes"][c].tolist(), c
        assert M.same(M.cou(counts), g["cus"][c]) and M.same(M.cou(counts), g["cou_mask"][c]), c
        assert M.same(M.cou_box(be, bg), g["cou_bb_proj"][c]) and M.same(M.cou_box(be, bg), g["cou_bb"][c]), c
        assert bool(g["raises"][c]) == (be is None or bg is None)
        d = float(g["mesh_diameter"][g["mesh"][c]])
        assert S.sphere_overlap(0.5 * d, g["t_est"][c], g["t_gt"][c]) == bool(g["sphere"][c]), c
        # surely set <= set <= possibly set, on both sides
        L = M.layers(c)
        assert not (L[3] & ~L[0]).any() and not (L[0] & ~L[2]).any() and not (L[5] & ~L[1]).any() and not (L[1] & ~L[4]).any()
    for a, b, e in zip(g["bb_est"], g["bb_gt"], g["bb_cou"]):
        assert M.same(M.cou_box(a.tolist(), b.tolist()), e), (a, b)


def test_named_cases_hold_their_property():
    g, _ = M.fixture()
    v = lambda name, key: g[key][M.case(name)]                # noqa: E731
    assert v("identical_box", "cus") == 0.0 and v("identical_ico", "cus") == 0.0
    assert v("disjoint", "cus") == 1.0 and v("disjoint", "counts")[1] > 0
    assert v("inside", "counts")[0] == v("inside", "counts")[2] < v("inside", "counts")[3]
    assert v("outside_est", "cus") == 1.0 and np.isnan(v("outside_est", "cou_bb_proj")) and v("outside_est", "raises")
    assert v("outside_both", "counts")[1] == 0 and v("outside_both", "cus") == 1.0
    assert v("pixel", "counts")[2] == 1 and v("pixel", "boxes")[0][2:].tolist() == [0, 0] and v("pixel", "cou_bb_proj") == 1.0
    assert v("column", "boxes")[0][2] == 0 and v("column", "boxes")[0][3] > 0 and v("column", "cou_bb_proj") == 1.0
    bx = v("touch", "boxes")
    assert bx[0][0] + bx[0][2] == bx[1][0] and v("touch", "cou_bb_proj") == 1.0
    assert all(b[0] < 32 <= b[0] + b[2] and b[1] < 32 <= b[1] + b[3] for b in v("crosstile", "boxes"))
    assert not v("diagonal", "sphere") and v("diagonal", "cou_bb_proj") < 1.0 and not v("far", "sphere")


def test_each_mutation_is_caught_by_a_named_case():
    g, _ = M.fixture()

    def boxes(name, **mut):
        me, mg = M.layers(M.case(name))[:2]
        return M.box_of(me, **mut), M.box_of(mg, **mut)

    # + 1 in the box width: the one-column silhouette inside the truth's would overlap it
    c = M.case("column")
    assert g["cou_bb_proj"][c] == 1.0 and M.cou_box(*boxes("column", plus_one=True)) < 1.0
    assert not M.same(M.cou_box(*boxes("offset_box", plus_one=True)), g["cou_bb_proj"][M.case("offset_box")])
    # clipped boxes: cou_bb takes boxes that reach outside the frame as they are
    hit = [i for i, (a, b) in enumerate(zip(g["bb_est"], g["bb_gt"]))
           if not M.same(M.cou_box(M.clip_box(a.tolist(), (67, 45)), M.clip_box(b.tolist(), (67, 45))), g["bb_cou"][i])]
    assert 4 in hit and 5 in hit and 11 in hit
    # >= instead of > in iou: two one-column boxes over each other divide 0 by 0
    c = M.case("column_both")
    assert g["cou_bb_proj"][c] == 1.0 and np.isnan(M.cou_box(*boxes("column_both"), or_equal=True))
    assert g["bb_cou"][7] == 1.0 and np.isnan(M.cou_box(g["bb_est"][7].tolist(), g["bb_gt"][7].tolist(), or_equal=True))
    # union 0 giving 0
    c = M.case("outside_both")
    assert g["cus"][c] == 1.0 and M.cou(g["counts"][c].tolist(), empty=0.0) == 0.0
    # the intersection over one side only
    c = M.case("offset_box")
    me, mg = M.layers(c)[:2]
    assert not M.same(M.cou(M.counts_of(me, mg, one_side=True)), g["cus"][c])
    # the sphere check applied to cou_bb_proj: the diagonal pair fails the check, and its boxes overlap
    c = M.case("diagonal")
    assert not g["sphere"][c] and g["cus"][c] == 1.0 and g["cou_bb_proj"][c] != 1.0


def test_intervals_contain_the_recorded_values():
    g, _ = M.fixture()
    for c in range(len(g["names"])):
        if g["behind"][c]:
            continue
        low, high = M.count_interval(c)
        assert all(lo <= v <= hi for lo, v, hi in zip(low, g["counts"][c].tolist(), high)), c
        lo, hi = M.cus_interval(c)
        assert lo <= g["cus"][c] <= hi, c
        for side in (0, 1):
            assert M.box_within(g["boxes"][c][side].tolist(), *M.box_interval(c, side)), (c, side)
        if not g["raises"][c]:
            lo, hi = M.cou_bb_proj_interval(c)
            assert lo <= g["cou_bb_proj"][c] <= hi, c


def test_stage_b_world_holds_what_the_comparison_needs():
    from tests import bop_eval_stages as BS
    b = M.world_b()
    err, lo, hi, skip = b["cus_err"], b["cus_lo"], b["cus_hi"], b["cus_skip"]
    rows, pairs = BS.expand(b, int(b["cus_params"][0]))
    assert np.array_equal(rows[:, :4], b["cus_est"]) and np.array_equal(pairs[:, 1], b["cus_key"][:, 4]) and len(err) == len(pairs) >= 40
    assert skip.any() and (~skip).any() and (err[skip] == 1.0).all() and (err < 0.5).any() and ((err >= 0.5) & ~skip).any()
    assert ((lo <= err) & (err <= hi)).all() and not ((lo <= 0.5) & (0.5 <= hi)).any()       # no interval holds the threshold
    _, info = BS.b_models(b)
    for p, (Re, te, Rg, tg, K, o) in enumerate(BS._b_pair_args(b, rows, pairs)):
        assert S.sphere_overlap(0.5 * info[o]["diameter"], te, tg) == (not skip[p]), p
    for r in np.unique(pairs[:, 0]):                          # candidates of one estimate: disjoint intervals, so the greedy scan is decided
        cand = [p for p in np.nonzero(pairs[:, 0] == r)[0] if hi[p] < 0.5]
        assert all(hi[x] < lo[y] or hi[y] < lo[x] for x in cand for y in cand if x < y)
    # eval_calc_scores.py's recall is the restatement's on the recorded errors
    fx = BS.b_case(b, "cus", np.concatenate([b["cus_est"], rows[:, 4:5]], 1), pairs, err, raw=True)
    assert b["cus_th"].tolist() == [0.5] and np.array_equal(b["cus_th"], metric.bop_thresholds("cus"))
    assert b["cus_m_est"].shape[1] == 1 and (b["cus_m_est"] >= 0).sum() == b["cus_s_counts"][0, 2] > 0
    assert fx["err"].shape == (len(err), 1)


def test_thresholds_and_recall_of_cus():
    assert np.array_equal(metric.bop_thresholds("cus"), np.array([0.5]))
    for kind in ("cou_mask", "cou_bb", "cou_bb_proj", "proj"):
        with pytest.raises(ValueError):
            metric.bop_thresholds(kind)
    r = metric.bop_recall(np.array([0.0, 0.49, 0.5, 1.0, np.nan]), "cus")
    assert r["correct"][:, 0].tolist() == [True, True, False, False, False] and r["recall"].tolist() == [0.4] and r["AR_CUS"] == 0.4
    with pytest.raises(ValueError):
        metric.bop_recall(np.zeros(3), "cou_bb_proj")
    with pytest.raises(ValueError):
        metric.summarize_bop({"cus": np.zeros(3)})           # unchanged: it scores mssd / mspd / vsd (and proj with thresholds)


def test_python_entry_points():
    assert "cus" in bop_eval.ERROR_KINDS
    p = inspect.signature(bop_eval.calc_errors).parameters
    assert p["size"].default is None and p["sphere_check"].default is True
    assert inspect.signature(bop_eval.evaluate_results).parameters["kinds"].default == ("vsd", "mssd", "mspd")
    sig = inspect.signature(metric.mask_errors)
    assert list(sig.parameters) == ["R_est", "t_est", "R_gt", "t_gt", "cam_K", "meshes", "size", "mesh_ids", "kinds", "sphere_check",
                                    "return_counts", "return_boxes", "return_masks"]
    assert sig.parameters["kinds"].default == ("cus", "cou_bb_proj") and sig.parameters["sphere_check"].default is False
    assert list(inspect.signature(metric.cus).parameters)[:8] == ["R_est", "t_est", "R_gt", "t_gt", "K", "renderer", "obj_id", "size"]
    assert list(inspect.signature(metric.cou_bb_proj).parameters)[:8] == list(inspect.signature(metric.cus).parameters)[:8]
    assert list(inspect.signature(metric.cou_mask).parameters)[:2] == ["mask_est", "mask_gt"]
    assert list(inspect.signature(metric.cou_bb).parameters)[:2] == ["bb_est", "bb_gt"]
    from checkerpose_amd import postprocess, targets
    for fn in (postprocess.evaluate_poses, targets.evaluate_batch, metric.score_poses):
        q = inspect.signature(fn).parameters
        assert q["size"].default is None and q["kinds"].default == ("add", "adi")
    R, t = torch.zeros(1, 3, 3), torch.zeros(1, 3, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.mask_errors(R, t, R, t, np.eye(3), None, (64, 48))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.mask_overlap(torch.zeros(1, 4, 4, dtype=torch.bool), torch.zeros(1, 4, 4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.box_overlap(torch.zeros(1, 4), torch.zeros(1, 4))
    with pytest.raises(ValueError, match="kinds"):
        metric.mask_errors(R, t, R, t, np.eye(3), None, (64, 48), kinds=("vsd",))
    with pytest.raises(ValueError, match="size"):
        metric.score_poses(R, t, R, t, np.eye(3), None, kinds=("cus",))


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    p = C.c_void_p(4096)                                    # fake, aligned; never dereferenced: every call returns before a launch

    def me(est=p, gt=p, K=p, ks=9, verts=p, voff=p, faces=p, foff=p, M=2, ids=p, diam=p, H=48, W=64, sphere=1, B=2, Vmax=8, cus=p, bbp=p,
           cnt=None, boxes=None, ok=None, masks=None, scr=p):
        return lib.cp_mask_errors(None, est, gt, K, ks, verts, voff, faces, foff, M, ids, diam, H, W, sphere, B, Vmax, cus, bbp, cnt, boxes,
                                  ok, masks, scr)

    for name in ("est", "gt", "K", "verts", "voff", "faces", "foff", "scr", "diam"):
        assert me(**{name: None}) == -1, name
    assert me(cus=None, bbp=None) == -1                     # at least one error must be asked
    assert me(B=0) == -1 and me(M=0) == -1 and me(Vmax=0) == -1 and me(H=0) == -1 and me(W=-1) == -1 and me(ks=3) == -1
    assert me(ids=None) == -1                               # several meshes need ids
    assert me(est=C.c_void_p(4100)) == -3 and me(scr=C.c_void_p(4104)) == -3 and me(faces=C.c_void_p(4098)) == -3
    assert me(cus=C.c_void_p(4100)) == -3 and me(cnt=C.c_void_p(4098)) == -3 and me(boxes=C.c_void_p(4097)) == -3
    assert me(B=1 << 20, H=480, W=640) == -4                # 2^20 x 300 tiles

    def mo(est=p, gt=p, H=48, W=64, B=2, cm=p, cb=p, cnt=None, boxes=None):
        return lib.cp_mask_overlap(None, est, gt, H, W, B, cm, cb, cnt, boxes)

    assert mo(est=None) == -1 and mo(gt=None) == -1 and mo(cm=None, cb=None) == -1 and mo(B=0) == -1 and mo(H=0) == -1 and mo(W=0) == -1
    assert mo(cm=C.c_void_p(4100)) == -3 and mo(cnt=C.c_void_p(4098)) == -3 and mo(H=1 << 16, W=1 << 15) == -4 and mo(B=1 << 24) == -4

    def bo(a=p, b=p, B=2, out=p):
        return lib.cp_box_overlap(None, a, b, B, out)

    assert bo(a=None) == -1 and bo(b=None) == -1 and bo(out=None) == -1 and bo(B=0) == -1 and bo(a=C.c_void_p(4100)) == -3
    assert lib.cp_mask_errors_scratch_bytes(0, 8) == 0 and lib.cp_mask_errors_scratch_bytes(1, -1) == 0
    for B, V in ((1, 0), (1, 3), (2, 10242), (256, 10242)):
        n = lib.cp_mask_errors_scratch_bytes(B, V)
        assert n % 16 == 0 and n >= 208 * B + 32 * B * V     # 52 header words and 2 x Vmax screen records per pair
    assert lib.cp_version() >= 213
    for name in ("cp_mask_errors", "cp_mask_errors_scratch_bytes", "cp_mask_overlap", "cp_box_overlap"):
        assert name in _abi.SIGNATURES
