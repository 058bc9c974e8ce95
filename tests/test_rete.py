"""Row N23 without a device: the numpy restatement of csrc/rete.hip's rule (tests/rete_stages.py) against what the reference's own
functions recorded (tests/golden/rete.npz, made by tests/golden/make_golden_rete.py), and the host sides of the new entry points.

  restatement  re within tol_re, cos within 64 eps, te within 8 eps (|t_a| + |t_b|) of the recording; the index equal wherever the
               reference's two best distinct candidates lie more than 2 tol apart (at most 5 % may not); the closest matrix; flags,
               counts, rates exact
  mutations    `<=` for `<`, the comparison on cos without the clamp, S . R_gt for R_gt . S, the symmetry's translation added to
               te: each is told from the rule by the fixture
  host         bop_thresholds, the C entry points' refusals (before any launch), the wrappers' ValueErrors, the signatures'
               defaults, lm_report_text equal to the recorded test_res_str byte for byte"""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from checkerpose_amd import _abi, bop_eval, metric, scene, targets
from tests import rete_stages as RS


@pytest.fixture(scope="module")
def fx():
    return RS.fixture()


@pytest.fixture(scope="module")
def tables(fx):
    """the four case sets as (S,12) float64 tables, through the public route: from_models_info(rotations_as=np.float32)"""
    info = RS.models_info(fx)
    ss = scene.SymmetrySet.from_models_info([info[int(o)] for o in fx["case_objs"]], rotations_as=np.float32)
    t, off = ss.table.numpy(), ss.offsets.numpy()
    return [t[off[m]:off[m + 1]] for m in range(len(ss))]


@pytest.fixture(scope="module")
def restated(fx, tables):
    return RS.rete_batch(fx["case_R_est"], fx["case_t_est"], fx["case_R_gt"], fx["case_t_gt"], tables, fx["case_mesh"])


def test_float32_rotations_are_the_loaders(fx, tables):
    assert [len(t) for t in tables] == [1, 2, 314, 628]
    for m, o in enumerate(fx["case_objs"].tolist()[1:], 1):
        rec = fx["sym_info_%d" % o]
        assert rec.dtype == np.float32 and np.array_equal(tables[m][:, :9].reshape(-1, 3, 3), rec.astype(np.float64))
    info = RS.models_info(fx)
    plain = scene.SymmetrySet.from_models_info([info[11]])
    f32 = scene.SymmetrySet.from_models_info([info[11]], rotations_as=np.float32)
    assert not np.array_equal(plain.table[:, :9].numpy(), f32.table[:, :9].numpy())          # the default is not rounded
    assert np.array_equal(plain.table[:, 9:].numpy(), f32.table[:, 9:].numpy())              # the translations are left alone
    assert np.array_equal(plain.table.numpy(), scene.SymmetrySet.from_models_info([info[11]], rotations_as=None).table.numpy())
    with pytest.raises(ValueError, match="rotations_as"):
        scene.SymmetrySet.from_models_info([info[11]], rotations_as=np.float16)


def index_must_match(fx):
    return fx["case_gap"] > 2.0 * RS.tol_re(fx["case_cos"])


def test_restatement_against_the_recording(fx, tables, restated):
    re, te, cs, idx = restated
    assert (np.abs(cs - fx["case_cos"]) <= RS.tol_cos()).all()
    assert (np.abs(re - fx["case_re"]) <= RS.tol_re(fx["case_cos"])).all()
    assert (np.abs(te - fx["case_te"]) <= RS.tol_te(fx["case_t_est"], fx["case_t_gt"])).all()
    must = index_must_match(fx)
    sym = fx["case_mesh"] > 0
    assert (~must[sym]).mean() <= 0.05
    assert np.array_equal(idx[must], fx["case_index"][must])
    for p in np.nonzero(must)[0]:
        T = tables[int(fx["case_mesh"][p])]
        mat = fx["case_R_gt"][p] if idx[p] < 0 else fx["case_R_gt"][p].dot(T[idx[p], :9].reshape(3, 3))
        assert np.array_equal(mat, fx["case_closest"][p])
    equal = fx["case_kind"] == 2
    assert equal.sum() == 4 and (re[equal] == 0.0).all() and (idx[equal] == -1).all() and (cs[equal] == 1.0).all()
    assert ((np.abs(cs) > 1.0).any())                                # the clamp is exercised
    # the plain candidate and the identity member are bitwise equal: "first wins" decides, and the reference decides the same way
    disc = fx["case_mesh"] == 1
    assert (fx["case_index"][disc] == -1).sum() > 10 and (fx["case_index"][disc] == 0).sum() == 0 and np.array_equal(idx[disc], fx["case_index"][disc])


@pytest.mark.parametrize("mut", RS.MUTATIONS)
def test_mutations_are_caught(fx, tables, mut):
    re, te, cs, idx = RS.rete_batch(fx["case_R_est"], fx["case_t_est"], fx["case_R_gt"], fx["case_t_gt"], tables, fx["case_mesh"], mut=mut)
    must = index_must_match(fx)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(re - fx["case_re"]) <= RS.tol_re(fx["case_cos"])).all() and np.array_equal(idx[must], fx["case_index"][must]) and \
            (np.abs(te - fx["case_te"]) <= RS.tol_te(fx["case_t_est"], fx["case_t_gt"])).all()
    assert not ok, mut


def test_flags_counts_rates_and_text(fx):
    lm13 = fx["rep_lm13"].tolist()
    assert tuple(lm13) == targets.LM13_OBJ_IDS and tuple(fx["rep_symmetry_ids"].tolist()) == targets.LM_SYMMETRIC_OBJ_IDS
    sym = np.isin(fx["rep_obj"], fx["rep_symmetry_ids"])
    adx = np.where(sym, fx["rep_adi"], fx["rep_add"])
    assert np.isnan(adx).sum() == 1 and (fx["rep_te"] == 10000).sum() == 1
    flags = RS.pass_flags(fx["rep_re"], fx["rep_te"], adx, fx["rep_diam"])
    assert np.array_equal(flags[:, 1:], fx["rep_flags"]) and tuple(RS.COUNT_COLUMNS) == targets.RETE_COUNTS
    slot = np.array([lm13.index(o) for o in fx["rep_obj"].tolist()])
    counts = RS.pass_counts(fx["rep_re"], fx["rep_te"], adx, fx["rep_diam"], slot, 13)
    per_obj, overall = RS.rates(counts)
    assert np.array_equal(per_obj, fx["rep_rates"]) and np.array_equal(overall, fx["rep_overall"])
    figures = {k: float(np.mean(fx["rep_fig_" + k])) for k in targets.FIGURES}
    figures["bit_err_arr"] = np.mean(fx["rep_fig_bit_err_arr"], axis=0)
    res, text = targets.lm_report_text(counts, figures, "all")
    assert text == str(fx["rep_text"])
    assert res["acc"] == res["adx10"] == overall[2] and res["rete2"] == overall[3] and res["te5"] == overall[8]
    assert np.array_equal(res["per_object"]["re5"], per_obj[:, 6])
    # the restated re of the report's crops, symmetric objects against their closest ground truth
    info = RS.models_info(fx)
    ss = scene.SymmetrySet.from_models_info([info[o] for o in lm13], rotations_as=np.float32)
    t, off = ss.table.numpy(), ss.offsets.numpy()
    re, te, cs, _ = RS.rete_batch(fx["rep_R_est"], fx["rep_t_est"], fx["rep_R_gt"], fx["rep_t_gt"], [t[off[m]:off[m + 1]] for m in range(13)], slot)
    assert (np.abs(re - fx["rep_re"]) <= RS.tol_re(cs)).all()
    fin = np.isfinite(te)
    assert (~fin).sum() == 1 and (fx["rep_te"][~fin] == 10000).all() and (np.abs(te - fx["rep_te"])[fin] <= RS.tol_te(fx["rep_t_est"], fx["rep_t_gt"])[fin]).all()
    assert np.array_equal(RS.pass_flags(re, te, adx, fx["rep_diam"])[:, 1:], fx["rep_flags"])


def test_thresholds_of_the_three_kinds():
    assert metric.bop_thresholds("re").tolist() == [5.0] and metric.bop_thresholds("te").tolist() == [5.0]
    assert metric.bop_thresholds("rete").tolist() == [[5.0, 5.0]]
    for kind in ("proj", "cou_mask", "cou_bb", "cou_bb_proj", "add"):
        with pytest.raises(ValueError):
            metric.bop_thresholds(kind)
    assert all(k in bop_eval.ERROR_KINDS for k in ("re", "te", "rete"))
    assert "no kernel computes" not in inspect.getdoc(bop_eval.calc_errors)


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


def test_abi_argument_checks_return_before_any_launch(lib):
    assert lib.cp_version() >= 233 and lib.cp_rete_pass_columns() == 10 == len(targets.RETE_COUNTS)
    one = C.c_void_p(4096)
    off_ok = (C.c_int32 * 4)(0, 1, 3, 3)                              # an empty set is allowed
    ids_ok = (C.c_int32 * 5)(0, 1, 2, 1, 0)

    def rete(**kw):
        a = dict(A=one, B=one, P=5, syms=one, off=one, off_h=off_ok, M=3, ids=one, ids_h=ids_ok, re=one, te=one, cos=one, idx=one)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = lib.cp_pose_rete(None, a["A"], a["B"], a["P"], a["syms"], a["off"], a["off_h"], a["M"], a["ids"], a["ids_h"], a["re"], a["te"], a["cos"],
                              a["idx"])
        assert lib.cp_kernel_log() == b"", kw
        return rc
    for name in ("A", "B", "re", "te", "off", "off_h"):
        assert rete(**{name: None}) == -1, name
        assert rete(P=0, **{name: None}) == -1, name
    assert rete(P=-1) == -1 and rete(M=0) == -1 and rete(M=-2) == -1
    assert rete(ids=None, ids_h=None) == -1                           # several sets need ids
    assert rete(off_h=(C.c_int32 * 4)(1, 2, 3, 4)) == -1              # does not start at 0
    assert rete(off_h=(C.c_int32 * 4)(0, 2, 1, 3)) == -1              # does not ascend
    assert rete(ids_h=(C.c_int32 * 5)(0, 1, 3, 1, 0)) == -1 and rete(ids_h=(C.c_int32 * 5)(0, -1, 2, 1, 0)) == -1
    for name in ("off", "off_h", "ids", "ids_h"):                     # the table's companions without the table
        a = dict(syms=None, off=None, off_h=None, ids=None, ids_h=None)
        a[name] = one if name in ("off", "ids") else (off_ok if name == "off_h" else ids_ok)
        assert rete(**a) == -1, name
    for name in ("A", "B", "syms", "re", "te", "cos"):
        assert rete(P=0, **{name: C.c_void_p(4100)}) == -3, name
    for name in ("off", "ids", "idx"):
        assert rete(P=0, **{name: C.c_void_p(4098)}) == -3, name
    assert rete(P=0) == 0 and rete(P=0, cos=None, idx=None) == 0 and rete(P=0, ids_h=None) == 0
    assert rete(P=0, syms=None, off=None, off_h=None, ids=None, ids_h=None, M=0) == 0
    assert rete(P=0, M=1, ids=None, ids_h=None, off_h=(C.c_int32 * 2)(0, 628)) == 0
    slot_ok = (C.c_int32 * 5)(0, 12, 3, 3, 1)

    def counts(**kw):
        a = dict(re=one, te=one, adx=one, diam=one, slot=one, slot_h=slot_ok, P=5, n=13, out=one)
        a.update(kw)
        lib.cp_kernel_log_begin()
        rc = lib.cp_rete_pass_counts(None, a["re"], a["te"], a["adx"], a["diam"], a["slot"], a["slot_h"], a["P"], a["n"], a["out"])
        assert lib.cp_kernel_log() == b"", kw
        return rc
    for name in ("re", "te", "adx", "diam", "slot", "out"):
        assert counts(**{name: None}) == -1, name
    assert counts(P=-1) == -1 and counts(n=0) == -1 and counts(n=257) == -1 and counts(n=12) == -1      # slot 12 needs 13 objects
    assert counts(slot_h=(C.c_int32 * 5)(0, -1, 3, 3, 1)) == -1
    for name in ("re", "te", "adx", "diam"):
        assert counts(**{name: C.c_void_p(4100)}) == -3, name
    assert counts(slot=C.c_void_p(4098)) == -3 and counts(out=C.c_void_p(4098)) == -3
    for code in (-1, -3):
        assert lib.cp_strerror(code) not in (b"", b"unknown checkerpose_hip error code")


def test_wrapper_refusals_and_defaults():
    P = 3
    R, t = np.tile(np.eye(3), (P, 1, 1)), np.zeros((P, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        targets.pose_re_te_sym(torch.from_numpy(R), t, R, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        targets.pose_re_te_sym(R, t, R, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        targets.rete_pass_counts(torch.zeros(P, dtype=torch.float64), t[:, 0], t[:, 0], t[:, 0], [0, 0, 0], 1)
    p = inspect.signature(targets.pose_re_te_sym).parameters
    assert list(p) == ["R_est", "t_est", "R_gt", "t_gt", "symmetries", "mesh_ids", "return_cos", "return_index", "return_closest"]
    assert p["symmetries"].default is None and p["mesh_ids"].default is None
    assert p["return_cos"].default is False and p["return_index"].default is False and p["return_closest"].default is False
    assert list(inspect.signature(targets.pose_re_te).parameters) == ["R_est", "t_est", "R_gt", "t_gt", "return_cos"]
    p = inspect.signature(targets.evaluate_batch).parameters
    assert list(p)[-1] == "re_symmetries" and p["re_symmetries"].default is None
    p = inspect.signature(targets.summarize_report_lm).parameters
    assert list(p) == ["batches", "obj_ids", "diameters", "symmetric_obj_ids", "lm_obj_ids", "adx_type"]
    assert p["symmetric_obj_ids"].default == (10, 11, 7, 3) and p["adx_type"].default == "all"
    assert p["lm_obj_ids"].default == (1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15)
    p = inspect.signature(scene.SymmetrySet.from_models_info).parameters
    assert p["rotations_as"].default is None and p["max_sym_disc_step"].default == 0.01
    assert inspect.signature(targets.summarize_report).parameters["symmetric"].default is False
    # summarize_report_lm names the argument it refuses, before it asks for a device
    z = torch.zeros(2, dtype=torch.float64)
    batch = {"all": {"re": z, "te": z, "errors": {"add": z}}, "report": {}}
    with pytest.raises(ValueError, match="adx_type"):
        targets.summarize_report_lm(batch, [1, 2], {1: 100.0, 2: 100.0}, adx_type="visible")
    with pytest.raises(ValueError, match="obj_ids"):
        targets.summarize_report_lm(batch, [1, 2, 4], {1: 100.0, 2: 100.0})
    with pytest.raises(ValueError, match="lm_obj_ids"):
        targets.summarize_report_lm(batch, [1, 3], {1: 100.0, 3: 100.0})
    with pytest.raises(ValueError, match="diameters"):
        targets.summarize_report_lm(batch, [1, 2], [100.0])
    with pytest.raises(ValueError, match="'adi'"):
        targets.summarize_report_lm(batch, [1, 10], {1: 100.0, 10: 100.0})
