"""BOP's evaluation after the errors, on the device (row N11; csrc/bop_match.hip): from a results table to the numbers of the
LM-O / YCB-V tables -- everything bop_toolkit does between scripts/eval_calc_errors.py and scripts/eval_bop19_pose.py's last line.

  EvalSet.from_dicts(...)        targets + scene_gt + scene_gt_info (bop_toolkit's own structures) -> flat tables
  gt_valid(evalset, ...)         eval_calc_scores.py:213-238: which ground truths count
  expand_pairs(evalset, ests, n_top)   eval_calc_errors.py:245-290: the top-n estimates of every target x the ground truths of its object
  calc_errors(pairs, kind, ...)  the errors of those pairs by metric.pose_errors / bop_errors / vsd_errors, with the caller's shortcuts
  match(pairs, errors, ...)      pose_matching.match_poses for every group and every threshold column in ONE launch (cp_bop_match)
  localization_scores(...)       score.calc_localization_scores for every column at once (cp_bop_scores)
  match_poses, match_poses_scene, calc_localization_scores   bop_toolkit's names, signatures and return structures
  evaluate_results(...)          eval_bop19_pose.py: AR_VSD / AR_MSSD / AR_MSPD / AR
  load_bop_results, save_bop_results   the CSV of tools_for_BOP/write_to_cvs.py (host)

A group is one (scene, image, object) with the object's ground truths in the image; a column is one threshold setting (for VSD one
(tau, threshold) pair: 100 columns).  The reference runs its Python loops once per column.  The tables are organised on the host
(dict work on a few thousand rows); errors, matching and counting run on the device.  There is no CPU fallback.

'cus' (row N12) is computed and scored at its own threshold 0.5 (eval_calc_scores.py:43); it is not part of AR.  The 'cou_*' errors
have no place in the reference's scripts: metric.mask_errors / mask_overlap / box_overlap compute them.

Out of scope: the COCO detection scores of eval_bop22_coco.py and calc_gt_coco.py, score.calc_ap, VSD's 'bop18' visibility mode, RGB
rendering, and writing matches_*.json."""
import numpy as np
import torch

from . import _abi, metric, scene

ERROR_KINDS = ("add", "adi", "ad", "mssd", "mspd", "proj", "vsd", "cus", "re", "te", "rete")


def _dev(device):
    return scene.cuda_device("bop_eval", device)


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


class EvalSet:
    """The ground truths and targets of an evaluation as flat tables (numpy on the host; device copies where the kernels read them).
    Rows are in the order of the reference's `matches` list: scenes and images in the order the targets first name them, gt_id
    ascending.  gt_scene / gt_im / gt_obj / gt_id int64 (NG), gt_visib float64 (NG), gt_R (NG,3,3), gt_t (NG,3,1) float64;
    tg_scene / tg_im / tg_obj / tg_inst int64 (T), one row per (scene, image, object) of the targets (a repeated target keeps its
    last entry, as the reference's dict does);  groups: one per (scene, image, object among the image's ground truths), in row
    order of their first ground truth: grp_key (G,3), grp_off (G+1) into grp_rows (NG) = the rows of each group, gt_id ascending;
    grp_target (G) = the group's target row or -1."""

    @classmethod
    def from_dicts(cls, targets, scene_gt, scene_gt_info, scene_ids, obj_ids, device="cuda:0"):
        """targets: the list of test_targets_bop19.json ({"scene_id", "im_id", "obj_id", "inst_count"});  scene_gt: {scene_id:
        inout.load_scene_gt's dict};  scene_gt_info: {scene_id: {im_id: [{"visib_fract", ...}]}} (or None: every fraction 1.0);
        scene_ids, obj_ids: the lists the scores are reported over (dp_split['scene_ids'], dp_model['obj_ids']).
        Images that no target names are dropped (eval_calc_scores.py:206-211)."""
        self = cls()
        self.scene_ids, self.obj_ids = [int(s) for s in scene_ids], [int(o) for o in obj_ids]
        org = {}
        for tg in targets:
            org.setdefault(int(tg["scene_id"]), {}).setdefault(int(tg["im_id"]), {})[int(tg["obj_id"])] = tg
        self.targets_org = org
        rows, tgs, R, t = [], [], [], []
        for scene, ims in org.items():
            for im, objs in ims.items():
                for obj, tg in objs.items():
                    tgs.append((scene, im, obj, int(tg.get("inst_count", 1))))
                info = None if scene_gt_info is None else scene_gt_info[scene][im]
                for gt_id, gt in enumerate(scene_gt[scene][im]):
                    rows.append((scene, im, int(gt["obj_id"]), gt_id, 1.0 if info is None else float(info[gt_id]["visib_fract"])))
                    R.append(np.asarray(gt.get("cam_R_m2c", np.eye(3)), dtype=np.float64).reshape(3, 3))
                    t.append(np.asarray(gt.get("cam_t_m2c", np.zeros(3)), dtype=np.float64).reshape(3, 1))
        if not rows:
            raise ValueError("the targets name no image with a ground truth")
        a = np.array([r[:4] for r in rows], dtype=np.int64)
        self.gt_scene, self.gt_im, self.gt_obj, self.gt_id = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
        self.gt_visib = np.array([r[4] for r in rows], dtype=np.float64)
        self.gt_R, self.gt_t = np.stack(R), np.stack(t)
        tg = np.array(tgs, dtype=np.int64).reshape(-1, 4)
        self.tg_scene, self.tg_im, self.tg_obj, self.tg_inst = tg[:, 0], tg[:, 1], tg[:, 2], tg[:, 3]
        tindex = {(s, i, o): k for k, (s, i, o, _) in enumerate(tgs)}
        groups = {}
        for r, (s, i, o, _, _) in enumerate(rows):
            groups.setdefault((s, i, o), []).append(r)
        self.grp_key = np.array(list(groups.keys()), dtype=np.int64).reshape(-1, 3)
        self.grp_index = {k: g for g, k in enumerate(groups)}
        self.grp_off = np.zeros(len(groups) + 1, dtype=np.int64)
        self.grp_off[1:] = np.cumsum([len(v) for v in groups.values()])
        self.grp_rows = np.concatenate([np.asarray(v, dtype=np.int64) for v in groups.values()])
        self.grp_target = np.array([tindex.get(k, -1) for k in groups], dtype=np.int64)
        oi, si = {o: k for k, o in enumerate(self.obj_ids)}, {s: k for k, s in enumerate(self.scene_ids)}
        self.gt_obj_index = np.array([oi.get(int(o), -1) for o in self.gt_obj], dtype=np.int64)
        self.gt_scene_index = np.array([si.get(int(s), -1) for s in self.gt_scene], dtype=np.int64)
        self.device = torch.device(device)             # checked when the first kernel is asked for
        self._cache = {}
        return self

    @property
    def n_gt(self):
        return int(self.gt_scene.shape[0])

    @property
    def n_groups(self):
        return int(self.grp_key.shape[0])

    def on_device(self):
        """the tables the kernels read, uploaded once: grp_off, grp_rows, gt_obj_index, gt_scene_index (int32), gt_R, gt_t (float64)"""
        if not self._cache:
            dev = _dev(self.device)
            self._cache = {"grp_off": _i32(self.grp_off, dev), "grp_rows": _i32(self.grp_rows, dev),
                           "gt_obj_index": _i32(self.gt_obj_index, dev), "gt_scene_index": _i32(self.gt_scene_index, dev),
                           "gt_R": torch.from_numpy(self.gt_R).to(dev), "gt_t": torch.from_numpy(self.gt_t).to(dev)}
        return self._cache


def gt_valid(evalset, visib_gt_min=-1):
    """eval_calc_scores.py:213-238 -> bool (NG,) numpy.  visib_gt_min >= 0: a ground truth is valid when its object is a target of the
    image and its visib_fract >= visib_gt_min;  -1: per image, the ground truths are taken by decreasing visib_fract (stable) and the
    first inst_count of each target object are valid."""
    es = evalset
    valid = np.zeros(es.n_gt, dtype=bool)
    inst = {(int(s), int(i), int(o)): int(n) for s, i, o, n in zip(es.tg_scene, es.tg_im, es.tg_obj, es.tg_inst)}
    if visib_gt_min >= 0:
        for r in range(es.n_gt):
            valid[r] = (int(es.gt_scene[r]), int(es.gt_im[r]), int(es.gt_obj[r])) in inst and es.gt_visib[r] >= visib_gt_min
        return valid
    start = 0
    while start < es.n_gt:                                   # the rows of an image are consecutive
        end = start
        while end < es.n_gt and es.gt_scene[end] == es.gt_scene[start] and es.gt_im[end] == es.gt_im[start]:
            end += 1
        order = sorted(range(start, end), key=lambda r: es.gt_visib[r], reverse=True)
        to_add = {}
        for r in order:
            k = (int(es.gt_scene[r]), int(es.gt_im[r]), int(es.gt_obj[r]))
            if k not in inst:
                continue
            left = to_add.setdefault(k, inst[k])
            if left > 0:
                valid[r] = True
                to_add[k] = left - 1
        start = end
    return valid


class Pairs:
    """expand_pairs' result.  Estimate rows (NE), in the order of the reference's scene_errs lists: est_scene / est_im / est_obj /
    est_id (the index in the (scene, im, obj) list in input order) / est_src (the index in `ests`) int64, est_score float64,
    est_group (the evalset group, -1 when the image holds no ground truth of the object).  Pairs (P): pair_est (estimate row),
    pair_gt (ground-truth row).  Kernel tables: the estimate rows with a group, sorted by group (kept in list order inside one):
    k_rows (NEk) into the estimate rows, k_est_off (G+1), k_pair_off (G+1), k_pair (Pk) into the pairs, estimate-major."""


def expand_pairs(evalset, ests, n_top, skip_missing=True):
    """eval_calc_errors.py:245-290.  ests: a list of {"scene_id", "im_id", "obj_id", "score", "R", "t"} (inout.load_bop_results'
    structure; R, t are only read by calc_errors).  n_top: 0 = all estimates of a target, -1 = its inst_count, k = k.  Only targets'
    estimates are used; the selection is stable by descending score; one pair per ground truth of the same object in the image.
    skip_missing=False raises the script's ValueError when a target has fewer estimates than asked."""
    es = evalset
    org = {}
    for n, e in enumerate(ests):
        org.setdefault((int(e["scene_id"]), int(e["im_id"]), int(e["obj_id"])), []).append(n)
    rows, pair_est, pair_gt = [], [], []
    for scene, im, obj, inst in zip(es.tg_scene, es.tg_im, es.tg_obj, es.tg_inst):
        key = (int(scene), int(im), int(obj))
        n_top_curr = None if n_top == 0 else (int(inst) if n_top == -1 else int(n_top))
        mine = org.get(key, [])
        if not skip_missing and len(mine) < n_top_curr:
            raise ValueError("Not enough estimates for scene: {}, im: {}, obj: {} (provided: {}, expected: {})".format(
                key[0], key[1], key[2], len(mine), n_top_curr))
        chosen = sorted(enumerate(mine), key=lambda x: ests[x[1]]["score"], reverse=True)[slice(0, n_top_curr)]
        g = es.grp_index.get(key, -1)
        for est_id, n in chosen:
            rows.append((key[0], key[1], key[2], est_id, n, g))
            if g >= 0:
                for r in es.grp_rows[es.grp_off[g]:es.grp_off[g + 1]]:
                    pair_est.append(len(rows) - 1)
                    pair_gt.append(int(r))
    return _pairs_from_rows(es, rows, [float(ests[r[4]]["score"]) for r in rows], pair_est, pair_gt)


def pairs_from_errors(evalset, scene_errs):
    """The error lists eval_calc_errors.py saves -> (Pairs, the (P, E) float64 error table in the pairs' order).
    scene_errs: {scene_id: [{"im_id", "obj_id", "est_id", "score", "errors": {gt_id: [e, ...]}}]}.  The estimates of a group keep
    their list order (it breaks score ties, as in the reference); estimates of an (image, object) without a ground truth among the
    targets' images are kept without pairs; a ground truth an estimate has no error for never matches it (NaN)."""
    es = evalset
    rows, scores, pair_est, pair_gt, table = [], [], [], [], []
    for scene, lst in scene_errs.items():
        for e in lst:
            g = es.grp_index.get((int(scene), int(e["im_id"]), int(e["obj_id"])), -1)
            rows.append((int(scene), int(e["im_id"]), int(e["obj_id"]), int(e["est_id"]), len(rows), g))
            scores.append(float(e["score"]))
            if g >= 0:
                for r in es.grp_rows[es.grp_off[g]:es.grp_off[g + 1]]:
                    pair_est.append(len(rows) - 1)
                    pair_gt.append(int(r))
                    table.append(e["errors"].get(int(es.gt_id[r])))
    E = max([len(v) for v in table if v is not None] + [1])
    arr = np.array([[float("nan")] * E if v is None else [float(x) for x in v] for v in table], dtype=np.float64).reshape(-1, E)
    return _pairs_from_rows(es, rows, scores, pair_est, pair_gt), arr


def _pairs_from_rows(es, rows, scores, pair_est, pair_gt):
    p = Pairs()
    p.evalset = es
    a = np.array(rows, dtype=np.int64).reshape(-1, 6)
    p.est_scene, p.est_im, p.est_obj, p.est_id, p.est_src, p.est_group = (a[:, k] for k in range(6))
    p.est_score = np.asarray(scores, dtype=np.float64).reshape(-1)
    p.pair_est, p.pair_gt = np.asarray(pair_est, dtype=np.int64), np.asarray(pair_gt, dtype=np.int64)
    have = np.nonzero(p.est_group >= 0)[0]
    p.k_rows = have[np.argsort(p.est_group[have], kind="stable")]
    G = es.n_groups
    n_e = np.bincount(p.est_group[p.k_rows], minlength=G).astype(np.int64)
    n_g = np.diff(es.grp_off)
    p.k_est_off = np.zeros(G + 1, dtype=np.int64)
    p.k_est_off[1:] = np.cumsum(n_e)
    p.k_pair_off = np.zeros(G + 1, dtype=np.int64)
    p.k_pair_off[1:] = np.cumsum(n_e * n_g)
    first = np.zeros(len(rows) + 1, dtype=np.int64)          # the pairs of an estimate row are consecutive, gt_id ascending
    first[1:] = np.cumsum(np.bincount(p.pair_est, minlength=len(rows))) if len(rows) else 0
    p.k_pair = (np.concatenate([np.arange(first[r], first[r + 1]) for r in p.k_rows]) if p.k_rows.size else np.zeros(0, np.int64))
    if p.k_est_off[-1] >= 2 ** 31 or es.n_gt >= 2 ** 31:
        raise ValueError("too many estimates / ground truths for int32 tables")
    return p


def _poses_of(ests, idx, dev):
    R = np.stack([np.asarray(ests[n]["R"], dtype=np.float64).reshape(3, 3) for n in idx])
    t = np.stack([np.asarray(ests[n]["t"], dtype=np.float64).reshape(3, 1) for n in idx])
    return torch.from_numpy(R).to(dev), torch.from_numpy(t).to(dev)


def calc_errors(pairs, ests, kind, meshes, obj_index, scene_camera=None, symmetries=None, symmetric_obj_ids=(), depths=None,
                delta=15.0, taus=None, sphere_check=True, size=None):
    """The errors of expand_pairs' pairs, on the device, by the rows that already compute them (metric.pose_errors / bop_errors /
    vsd_errors / mask_errors), with eval_calc_errors.py's shortcuts: inf for "ad" / "add" / "adi" / "mssd" when |t_e - t_g| >=
    diameter (:306-309), the sphere check of VSD and cus (a pair that fails it scores 1.0, :310-318, :357-362).
      kind: "add", "adi", "ad" (ADI for symmetric_obj_ids, else ADD), "mssd", "mspd", "proj", "vsd", "cus";  meshes: a MeshSet (its
      diameters are the models_info diameters; with faces for "vsd" / "cus");  obj_index: {obj_id: index of its mesh};  scene_camera:
      {scene_id: inout.load_scene_camera's dict} or one (3,3) K ("mspd", "proj", "vsd", "cus");  symmetries: as metric.bop_errors';
      depths: {scene_id: {im_id: (H,W) depth in mm}} ("vsd");  delta, taus, sphere_check: metric.vsd_errors';  size: (W, H) of the
      frames ("cus").
    "re", "te", "rete": pose_error.re(R_e, R_g) / .te(t_e, t_g) as eval_calc_errors.py:368-375 calls them (targets.pose_re_te_sym
    without symmetries: cp_pose_rete): no symmetries and no diameter shortcut, the script applies none to these kinds; meshes is not
    read.  A table of the caller's own goes to match() as it is.
    -> float64 CUDA tensor (P, 1), (P, 2) = [re | te] for "rete", or (P, T) for "vsd", in the pairs' order."""
    if kind not in ERROR_KINDS:
        raise ValueError("kind must be among %s, got %r" % (ERROR_KINDS, kind))
    es = pairs.evalset
    dev = _dev(es.device)
    P = int(pairs.pair_est.shape[0])
    if P == 0:
        return torch.zeros((0, 2 if kind == "rete" else (1 if kind != "vsd" else len(metric.vsd_taus(taus)[0]))), dtype=torch.float64, device=dev)
    src = pairs.est_src[pairs.pair_est]
    Re, te = _poses_of(ests, src, dev)
    tabs = es.on_device()
    gi = torch.from_numpy(pairs.pair_gt).to(dev)
    Rg, tg = tabs["gt_R"].index_select(0, gi), tabs["gt_t"].index_select(0, gi)
    if kind in ("re", "te", "rete"):
        from .targets import pose_re_te_sym
        e_re, e_te = pose_re_te_sym(Re, te, Rg, tg)
        return torch.stack([e_re, e_te], 1) if kind == "rete" else (e_re if kind == "re" else e_te)[:, None]
    objs = es.gt_obj[pairs.pair_gt]
    for o in np.unique(objs):
        if int(o) not in obj_index:
            raise ValueError("obj_id %r is not in obj_index" % (int(o),))
    mesh_ids = np.array([obj_index[int(o)] for o in objs], dtype=np.int64)
    K = None
    if kind in ("mspd", "proj", "vsd", "cus"):
        if scene_camera is None:
            raise ValueError("%r needs scene_camera (or one 3x3 K)" % (kind,))
        if isinstance(scene_camera, dict):
            K = np.stack([np.asarray(scene_camera[int(s)][int(i)]["cam_K"], dtype=np.float64).reshape(3, 3)
                          for s, i in zip(es.gt_scene[pairs.pair_gt], es.gt_im[pairs.pair_gt])])
        else:
            K = np.asarray(scene_camera, dtype=np.float64).reshape(3, 3)
    if kind == "cus":
        if size is None:
            raise ValueError("\"cus\" needs size=(W, H)")
        return metric.mask_errors(Re, te, Rg, tg, K, meshes, size, mesh_ids=mesh_ids, kinds=("cus",), sphere_check=sphere_check)["cus"][:, None]
    if kind == "vsd":
        if depths is None:
            raise ValueError("\"vsd\" needs depths")
        keys = sorted(set(zip(es.gt_scene[pairs.pair_gt].tolist(), es.gt_im[pairs.pair_gt].tolist())))
        index = {k: n for n, k in enumerate(keys)}
        stack = np.stack([np.asarray(depths[s][i], dtype=np.float32) for s, i in keys])
        image_ids = [index[k] for k in zip(es.gt_scene[pairs.pair_gt].tolist(), es.gt_im[pairs.pair_gt].tolist())]
        return metric.vsd_errors(Re, te, Rg, tg, K, meshes, stack, image_ids=image_ids, delta=delta, taus=taus, mesh_ids=mesh_ids,
                                 sphere_check=sphere_check)["vsd"]
    if kind in ("mspd", "proj"):
        return metric.bop_errors(Re, te, Rg, tg, K, meshes, symmetries=symmetries, mesh_ids=mesh_ids, kinds=(kind,))[kind][:, None]
    if kind == "mssd":
        e = metric.bop_errors(Re, te, Rg, tg, np.eye(3), meshes, symmetries=symmetries, mesh_ids=mesh_ids, kinds=("mssd",))["mssd"]
    elif kind == "ad":
        sym = np.isin(objs, np.asarray(list(symmetric_obj_ids), dtype=np.int64))
        both = metric.pose_errors(Re, te, Rg, tg, meshes, mesh_ids=mesh_ids, kinds=tuple(k for k, need in (("add", (~sym).any()), ("adi", sym.any())) if need))
        e = both["adi"] if sym.all() else (both["add"] if not sym.any() else torch.where(torch.from_numpy(sym).to(dev), both["adi"], both["add"]))
    else:
        e = metric.pose_errors(Re, te, Rg, tg, meshes, mesh_ids=mesh_ids, kinds=(kind,))[kind]
    diam = torch.from_numpy(np.asarray(meshes.diameters, dtype=np.float64)[mesh_ids]).to(dev)
    d = te.reshape(-1, 3) - tg.reshape(-1, 3)
    dist = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).sqrt()
    return torch.where(dist < diam, e, torch.full_like(e, float("inf")))[:, None]


def _columns(thresholds, err_cols, C_err):
    th = np.asarray(thresholds, dtype=np.float64)
    if th.ndim == 1:
        th = th[:, None]
    if th.ndim != 2 or th.shape[0] == 0 or th.shape[1] not in (1, 2):
        raise ValueError("thresholds must be (C,) or (C, E) with E = 1 or 2, got %r" % (th.shape,))
    C, E = th.shape
    if err_cols is None:
        if C_err != E:
            raise ValueError("%d error columns for %d-element thresholds: pass err_cols" % (C_err, E))
        cols = np.tile(np.arange(E, dtype=np.int64), (C, 1))
    else:
        cols = np.asarray(err_cols, dtype=np.int64)
        cols = cols[:, None] if cols.ndim == 1 else cols
    if cols.shape != (C, E) or cols.min() < 0 or cols.max() >= C_err:
        raise ValueError("err_cols must be (C, E) with values in 0..%d" % (C_err - 1))
    return np.ascontiguousarray(th), np.ascontiguousarray(cols)


def _launch_match(dev, errs, est_score, est_ids, est_off, gt_off, pair_off, gt_rows, valid, NG, thresholds, err_cols, max_ests,
                  _stage=None, _mask=None):
    """cp_bop_match on host tables (numpy) + the device error tensor -> dict of CUDA tensors"""
    if _stage not in (None, "lds", "global") or _mask not in (None, "register", "scratch"):
        raise ValueError("_stage: None / \"lds\" / \"global\"; _mask: None / \"register\" / \"scratch\"")
    errs = errs.to(device=dev, dtype=torch.float64)
    errs = (errs[:, None] if errs.dim() == 1 else errs).contiguous()
    P, C_err = int(errs.shape[0]), max(1, int(errs.shape[1]))
    th, cols = _columns(thresholds, err_cols, C_err)
    C, E = th.shape
    G, NE = int(gt_off.shape[0]) - 1, int(est_score.shape[0])
    if G <= 0 or NG <= 0:
        raise ValueError("no groups")
    if int(pair_off[-1]) != P:
        raise ValueError("%d error rows for %d pairs" % (P, int(pair_off[-1])))
    if np.isnan(np.asarray(est_score, dtype=np.float64)).any():
        raise ValueError("a score is NaN: Python's sort, which the reference relies on, has no order for it")
    n_g = np.diff(gt_off)
    on_scratch = (n_g > 64) | (_mask == "scratch")
    words = np.where(on_scratch, (n_g + 63) // 64, 0)
    mask_off = np.where(on_scratch, np.cumsum(words) - words, -1)
    mask_words = int(words.sum())
    flags = (_abi.BOP_MATCH_NO_LDS if _stage == "global" else 0) | (_abi.BOP_MATCH_SCRATCH_MASK if _mask == "scratch" else 0)
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)     # noqa: E731
    t_score, t_ids, t_eoff, t_goff = f64(est_score), _i32(est_ids, dev), _i32(est_off, dev), _i32(gt_off, dev)
    t_poff = torch.from_numpy(np.ascontiguousarray(pair_off, dtype=np.int64)).to(dev)
    t_rows = None if gt_rows is None else (gt_rows if torch.is_tensor(gt_rows) else _i32(gt_rows, dev))
    t_valid = None if valid is None else (valid.to(device=dev, dtype=torch.uint8).contiguous() if torch.is_tensor(valid)
                                          else torch.from_numpy(np.ascontiguousarray(valid, dtype=np.uint8)).to(dev))
    t_cols, t_th, t_moff = _i32(cols, dev), f64(th), _i32(mask_off, dev)
    out = {"est_id": torch.empty((NG, C), dtype=torch.int32, device=dev), "score": torch.empty((NG, C), dtype=torch.float64, device=dev),
           "error": torch.empty((NG, C, E), dtype=torch.float64, device=dev),
           "error_norm": torch.empty((NG, C, E), dtype=torch.float64, device=dev)}
    scratch = torch.empty(_abi.load().cp_bop_match_scratch_bytes(NE, mask_words, C), dtype=torch.uint8, device=dev)
    nz = lambda x: None if x is None or x.numel() == 0 else x     # noqa: E731  (an empty table goes in as a null pointer)
    _abi.call("cp_bop_match", dev, nz(errs), P, C_err, nz(t_score), nz(t_ids), NE, t_eoff, t_goff, t_poff, G, nz(t_rows), nz(t_valid), NG,
              t_cols, t_th, C, E, int(max_ests), t_moff, mask_words, flags, out["est_id"], out["score"], out["error"], out["error_norm"],
              scratch)
    out["thresholds"] = th
    return out


def match(pairs, errors, thresholds, err_cols=None, n_top=0, valid=None, _stage=None, _mask=None):
    """pose_matching.match_poses for every group of expand_pairs' result and every column, in one launch (cp_bop_match).
      errors: (P,) / (P, C_err) tensor in the pairs' order (calc_errors', or the caller's re / te / rete table);  thresholds: (C,) or
      (C, E) -- E = 2 for rete;  err_cols: (C,) / (C, E) which error column each threshold element reads (default: column k for
      element k, when C_err == E);  n_top: match_poses' max_ests_count (> 0: only the n_top best-scored estimates of a group);
      valid: gt_valid's mask (None = all valid).  _stage / _mask force the kernel's paths (tests: the results are bit-identical).
    -> {"est_id" int32 (NG, C) (-1 = unmatched), "score" (NG, C), "error", "error_norm" (NG, C, E) float64 CUDA tensors (-1.0 where
    unmatched), "thresholds"}; rows in the evalset's order."""
    es = pairs.evalset
    dev = _dev(es.device)
    errors = torch.as_tensor(errors)
    errors = errors[:, None] if errors.dim() == 1 else errors
    if int(errors.shape[0]) != int(pairs.pair_est.shape[0]):
        raise ValueError("errors has %d rows for %d pairs" % (int(errors.shape[0]), int(pairs.pair_est.shape[0])))
    errors = errors.to(dev)
    if not np.array_equal(pairs.k_pair, np.arange(pairs.k_pair.shape[0])) or pairs.k_pair.shape[0] != errors.shape[0]:
        errors = errors.index_select(0, torch.from_numpy(pairs.k_pair).to(dev))
    tabs = es.on_device()
    return _launch_match(dev, errors, pairs.est_score[pairs.k_rows], pairs.est_id[pairs.k_rows], pairs.k_est_off, es.grp_off,
                         pairs.k_pair_off, tabs["grp_rows"], valid, es.n_gt, thresholds, err_cols, n_top, _stage, _mask)


def _recall(tp, targets):
    """score.calc_recall on arrays: tp / float(targets), 0.0 without targets"""
    tp, targets = np.asarray(tp, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    return np.where(targets == 0, 0.0, tp / np.where(targets == 0, 1.0, targets))


def _launch_scores(dev, est_id, valid, gt_obj_index, gt_scene_index, gt_off, gt_rows, n_obj, n_scene, n_top, _bins=None):
    NG, C = int(est_id.shape[0]), int(est_id.shape[1])
    G = int(gt_off.shape[0]) - 1
    NB = 1 + n_obj + n_scene
    counts = torch.empty((NB * (1 + C),), dtype=torch.int32, device=dev)
    t_valid = None if valid is None else (valid.to(device=dev, dtype=torch.uint8).contiguous() if torch.is_tensor(valid)
                                          else torch.from_numpy(np.ascontiguousarray(valid, dtype=np.uint8)).to(dev))
    as32 = lambda x: x if torch.is_tensor(x) else _i32(x, dev)     # noqa: E731
    t_obj, t_scene, t_off = as32(gt_obj_index), as32(gt_scene_index), as32(gt_off)
    t_rows = None if gt_rows is None else as32(gt_rows)
    est_id = est_id.contiguous()
    _abi.call("cp_bop_scores", dev, est_id, t_valid, t_obj, t_scene, NG, t_off, t_rows, G, C, n_obj, n_scene, int(n_top),
              _abi.BOP_SCORES_NO_LDS if _bins == "global" else 0, counts)
    c = counts.cpu().numpy().astype(np.int64)
    return c[:NB], c[NB:].reshape(NB, C)


def _scores_dict(es_scene_ids, es_obj_ids, targets, tp, gt_count):
    """the quotients and means of score.py:112-137 in fp64, per column -> dict of arrays + the reference's dicts per column"""
    n_obj = len(es_obj_ids)
    recall = _recall(tp[0], targets[0])
    obj = _recall(tp[1:1 + n_obj], targets[1:1 + n_obj, None])
    scene = _recall(tp[1 + n_obj:], targets[1 + n_obj:, None])
    C = tp.shape[1]
    res = {"recall": recall, "obj_recalls": obj, "scene_recalls": scene,
           "mean_obj_recall": np.array([float(np.mean(list(obj[:, c]))) for c in range(C)]),
           "mean_scene_recall": np.array([float(np.mean(list(scene[:, c]))) for c in range(C)]),
           "gt_count": int(gt_count), "targets_count": int(targets[0]), "tp_count": tp[0].astype(np.int64),
           "obj_targets": targets[1:1 + n_obj], "scene_targets": targets[1 + n_obj:], "obj_tp": tp[1:1 + n_obj], "scene_tp": tp[1 + n_obj:]}
    return res


def scores_of_column(scores, evalset_or_ids, c=0):
    """column c of localization_scores' result as the dict score.calc_localization_scores returns"""
    scene_ids, obj_ids = (evalset_or_ids.scene_ids, evalset_or_ids.obj_ids) if isinstance(evalset_or_ids, EvalSet) else evalset_or_ids
    return {"recall": float(scores["recall"][c]), "obj_recalls": {o: float(scores["obj_recalls"][k, c]) for k, o in enumerate(obj_ids)},
            "mean_obj_recall": float(scores["mean_obj_recall"][c]),
            "scene_recalls": {s: float(scores["scene_recalls"][k, c]) for k, s in enumerate(scene_ids)},
            "mean_scene_recall": float(scores["mean_scene_recall"][c]), "gt_count": scores["gt_count"],
            "targets_count": scores["targets_count"], "tp_count": int(scores["tp_count"][c])}


def localization_scores(evalset, matched, valid, n_top, _bins=None):
    """score.calc_localization_scores for every column at once (cp_bop_scores: integer counts on the device; the quotients and the
    means over ALL listed objects / scenes in fp64 here).  matched: match()'s dict or its "est_id" tensor; valid: gt_valid's mask.
    -> {"recall" (C,), "obj_recalls" (n_obj, C), "scene_recalls" (n_scene, C), "mean_obj_recall", "mean_scene_recall" (C,),
    "gt_count", "targets_count", "tp_count" (C,), + the integer tables}; scores_of_column gives the reference's dict of a column."""
    es = evalset
    est_id = matched["est_id"] if isinstance(matched, dict) else matched
    ok = np.ones(es.n_gt, dtype=bool) if valid is None else (valid.cpu().numpy() if torch.is_tensor(valid) else np.asarray(valid)).astype(bool)
    out = np.nonzero(ok & ((es.gt_obj_index < 0) | (es.gt_scene_index < 0)))[0]
    if out.size:                                             # the reference's obj_tars[m['obj_id']] / scene_tars[m['scene_id']]
        raise KeyError((int(es.gt_obj[out[0]]), int(es.gt_scene[out[0]])))
    dev = _dev(es.device)
    if not torch.is_tensor(est_id):
        est_id = torch.from_numpy(np.ascontiguousarray(est_id, dtype=np.int32)).to(dev)
    tabs = es.on_device()
    targets, tp = _launch_scores(_dev(es.device), est_id, valid, tabs["gt_obj_index"], tabs["gt_scene_index"], tabs["grp_off"], tabs["grp_rows"],
                                 len(es.obj_ids), len(es.scene_ids), n_top, _bins)
    return _scores_dict(es.scene_ids, es.obj_ids, targets, tp, es.n_gt)


# ---- bop_toolkit's names, signatures and return structures ----------------------------------------------------------------------------
def _group_tables(errs_lists, gt_ids_lists):
    """[(errs of a group, its ground-truth ids)] -> host tables + the (P, E) error array"""
    est_score, est_ids, est_off, pair_off, rows = [], [], [0], [0], []
    for errs, gt_ids in zip(errs_lists, gt_ids_lists):
        for e in errs:
            est_score.append(float(e["score"]))
            est_ids.append(int(e["est_id"]))
            for g in gt_ids:
                v = e["errors"].get(g)
                rows.append([float("nan")] if v is None else [float(x) for x in v])       # an absent pair never matches
        est_off.append(len(est_score))
        pair_off.append(len(rows))
    E = max([len(r) for r in rows] + [1])
    table = np.array([r + [float("nan")] * (E - len(r)) for r in rows], dtype=np.float64).reshape(-1, E)
    return np.array(est_score, dtype=np.float64), np.array(est_ids, dtype=np.int64), np.array(est_off), np.array(pair_off), table


def match_poses(errs, error_ths, max_ests_count=0, gt_valid_mask=None, device="cuda:0"):
    """bop_toolkit_lib.pose_matching.match_poses, one group through cp_bop_match.  The reference scans each estimate's `errors` dict
    in that dict's own order (for two-element errors the result depends on it).  Here the ground truths are scanned in the key order
    of the first estimate's dict, keys only later estimates have after them: the reference's order whenever the estimates' dicts
    agree, as the lists eval_calc_errors.py writes do (increasing gt_id).
    -> the reference's list of {"est_id", "gt_id", "score", "error", "error_norm"}, in matching order."""
    dev = _dev(device)
    ths = [float(x) for x in error_ths]
    gt_ids = list(dict.fromkeys(g for e in errs for g in e["errors"]))
    if not errs or not gt_ids:
        return []
    score, ids, est_off, pair_off, table = _group_tables([errs], [gt_ids])
    valid = None if not gt_valid_mask else np.array([bool(gt_valid_mask[g]) for g in gt_ids])
    out = _launch_match(dev, torch.from_numpy(table), score, np.arange(len(errs)), est_off, np.array([0, len(gt_ids)]), pair_off, None,
                        valid, len(gt_ids), np.array([ths]), None, max_ests_count)
    slot, err, norm = out["est_id"][:, 0].cpu().numpy(), out["error"][:, 0].cpu().numpy(), out["error_norm"][:, 0].cpu().numpy()
    got = [(int(s), j) for j, s in enumerate(slot) if s >= 0]
    rank = {n: k for k, n in enumerate(sorted(range(len(errs)), key=lambda n: errs[n]["score"], reverse=True))}
    return [{"est_id": errs[s]["est_id"], "gt_id": gt_ids[j], "score": errs[s]["score"], "error": [float(x) for x in err[j]],
             "error_norm": [float(x) for x in norm[j]]} for s, j in sorted(got, key=lambda x: rank[x[0]])]


def match_poses_scene(scene_id, scene_gt, scene_gt_valid, scene_errs, correct_th, n_top, device="cuda:0"):
    """bop_toolkit_lib.pose_matching.match_poses_scene, the whole scene in one launch -> the reference's list of dicts (one per ground
    truth: scene_id, im_id, obj_id, gt_id, est_id, score, error, error_norm, valid; -1 where unmatched)."""
    dev = _dev(device)
    ths = [float(x) for x in correct_th]
    org = {}
    for e in scene_errs:
        org.setdefault(e["im_id"], {}).setdefault(e["obj_id"], []).append(e)
    matches, groups, base = [], [], 0
    for im_id, im_gts in scene_gt.items():
        by_obj = {}
        for gt_id, gt in enumerate(im_gts):
            matches.append({"scene_id": scene_id, "im_id": im_id, "obj_id": gt["obj_id"], "gt_id": gt_id, "est_id": -1, "score": -1,
                            "error": -1, "error_norm": -1, "valid": scene_gt_valid[im_id][gt_id]})
            by_obj.setdefault(gt["obj_id"], []).append(gt_id)
        for obj_id, ids in by_obj.items():
            groups.append((org.get(im_id, {}).get(obj_id, []), ids, base))
        base += len(im_gts)
    if not matches:
        return matches
    score, est_slot, est_off, pair_off, table = _group_tables([g[0] for g in groups], [g[1] for g in groups])
    flat = [e for g in groups for e in g[0]]
    gt_off = np.zeros(len(groups) + 1, dtype=np.int64)
    gt_off[1:] = np.cumsum([len(g[1]) for g in groups])
    rows = np.array([g[2] + j for g in groups for j in g[1]], dtype=np.int64)
    valid = np.array([bool(m["valid"]) for m in matches])
    out = _launch_match(dev, torch.from_numpy(table), score, np.arange(len(flat)), est_off, gt_off, pair_off, rows, valid, len(matches),
                        np.array([ths]), None, n_top)
    slot, err, norm = out["est_id"][:, 0].cpu().numpy(), out["error"][:, 0].cpu().numpy(), out["error_norm"][:, 0].cpu().numpy()
    for r, m in enumerate(matches):
        if slot[r] >= 0:
            e = flat[int(slot[r])]
            m.update({"est_id": e["est_id"], "score": e["score"], "error": [float(x) for x in err[r]],
                      "error_norm": [float(x) for x in norm[r]]})
    return matches


def calc_localization_scores(scene_ids, obj_ids, matches, n_top, do_print=False, device="cuda:0"):
    """bop_toolkit_lib.score.calc_localization_scores on a list of match dicts (pose_matching's), counted by cp_bop_scores.
    -> the reference's dict: recall, obj_recalls, mean_obj_recall, scene_recalls, mean_scene_recall, gt_count, targets_count, tp_count."""
    dev = _dev(device)
    scene_ids, obj_ids = list(scene_ids), list(obj_ids)
    if not matches:
        zero = _scores_dict(scene_ids, obj_ids, np.zeros(1 + len(obj_ids) + len(scene_ids), np.int64),
                            np.zeros((1 + len(obj_ids) + len(scene_ids), 1), np.int64), 0)
        return scores_of_column(zero, (scene_ids, obj_ids))
    oi, si = {o: k for k, o in enumerate(obj_ids)}, {s: k for k, s in enumerate(scene_ids)}
    groups = {}
    for r, m in enumerate(matches):
        if m["valid"] and (m["obj_id"] not in oi or m["scene_id"] not in si):
            raise KeyError((m["obj_id"], m["scene_id"]))
        groups.setdefault((m["obj_id"], m["scene_id"], m["im_id"]), []).append(r)
    gt_off = np.zeros(len(groups) + 1, dtype=np.int64)
    gt_off[1:] = np.cumsum([len(v) for v in groups.values()])
    rows = np.concatenate([np.asarray(v, dtype=np.int64) for v in groups.values()])
    est = torch.from_numpy(np.array([-1 if m["est_id"] == -1 else 0 for m in matches], dtype=np.int32)[:, None]).to(dev)
    targets, tp = _launch_scores(dev, est, np.array([bool(m["valid"]) for m in matches]),
                                 np.array([oi.get(m["obj_id"], -1) for m in matches]), np.array([si.get(m["scene_id"], -1) for m in matches]),
                                 gt_off, rows, len(obj_ids), len(scene_ids), n_top)
    res = scores_of_column(_scores_dict(scene_ids, obj_ids, targets, tp, len(matches)), (scene_ids, obj_ids))
    if do_print:
        print("GT count: %d, target count: %d, TP count: %d, recall: %.4f, mean object recall: %.4f, mean scene recall: %.4f" % (
            res["gt_count"], res["targets_count"], res["tp_count"], res["recall"], res["mean_obj_recall"], res["mean_scene_recall"]))
    return res


def evaluate_results(evalset, ests, meshes, obj_index, scene_camera, im_width, symmetries=None, depths=None, delta=15.0,
                     visib_gt_min=-1, kinds=("vsd", "mssd", "mspd"), size=None):
    """scripts/eval_bop19_pose.py from the results table to the final scores: n_top = -1, metric.bop_thresholds' thresholds, MSSD
    divided by the diameter and MSPD multiplied by 640 / im_width before thresholding (eval_calc_scores.py:246-258), VSD over its ten
    taus x ten thresholds.  Arguments: calc_errors'; "vsd" is scored when `depths` is given.  "cus" among the kinds (needs `size`)
    is scored at its threshold 0.5 (eval_calc_scores.py:43) and reported as "AR_CUS"; it is not part of "AR".
    "re", "te", "rete" among the kinds are scored at eval_calc_scores.py:44-46's thresholds (5 degrees, 5, and the pair [5, 5]) and
    reported as "AR_RE" / "AR_TE" / "AR_RETE"; they are not part of "AR" either.
    -> {"AR_VSD", "AR_MSSD", "AR_MSPD": the mean of the overall recall over the kind's columns, "AR": their mean (when all three are
    there), "recall": {kind: (C,) recalls, VSD tau-major}, "scores": {kind: localization_scores' dict}, "valid"}."""
    es = evalset
    valid = gt_valid(es, visib_gt_min)
    pairs = expand_pairs(es, ests, -1)
    res = {"recall": {}, "scores": {}, "valid": valid}
    for kind in kinds:
        if kind == "vsd" and depths is None:
            continue
        errs = calc_errors(pairs, ests, kind, meshes, obj_index, scene_camera=scene_camera, symmetries=symmetries, depths=depths, delta=delta,
                           size=size)
        th = metric.bop_thresholds(kind)
        cols = None
        if kind == "mssd" and errs.shape[0]:
            mesh_ids = np.array([obj_index[int(o)] for o in es.gt_obj[pairs.pair_gt]], dtype=np.int64)
            errs = errs / torch.from_numpy(np.asarray(meshes.diameters, dtype=np.float64)[mesh_ids]).to(errs.device)[:, None]
        elif kind == "mspd":
            errs = (640.0 / float(im_width)) * errs
        elif kind == "vsd":
            T = int(errs.shape[1])
            cols = np.repeat(np.arange(T), th.shape[0])
            th = np.tile(th, T)
        m = match(pairs, errs, th, err_cols=cols, n_top=-1, valid=valid)
        sc = localization_scores(es, m, valid, -1)
        res["scores"][kind], res["recall"][kind] = sc, sc["recall"]
        res["AR_" + kind.upper()] = float(np.mean(list(sc["recall"])))
    if all(k in res for k in ("AR_VSD", "AR_MSSD", "AR_MSPD")):
        res["AR"] = float(np.mean([res["AR_VSD"], res["AR_MSSD"], res["AR_MSPD"]]))
    return res


# ---- the results CSV (inout.load_bop_results / save_bop_results, 'bop19'; tools_for_BOP/write_to_cvs.py writes it) ----------------------
HEADER = "scene_id,im_id,obj_id,score,R,t,time"


def load_bop_results(path):
    """-> list of {"scene_id", "im_id", "obj_id", "score", "R" (3,3), "t" (3,1), "time"}"""
    results = []
    with open(path, "r") as f:
        for n, line in enumerate(f):
            if n == 0 and HEADER in line:
                continue
            elems = line.split(",")
            if len(elems) != 7:
                raise ValueError("A line does not have 7 comma-sep. elements: {}".format(line))
            results.append({"scene_id": int(elems[0]), "im_id": int(elems[1]), "obj_id": int(elems[2]), "score": float(elems[3]),
                            "R": np.array(list(map(float, elems[4].split())), np.float64).reshape((3, 3)),
                            "t": np.array(list(map(float, elems[5].split())), np.float64).reshape((3, 1)), "time": float(elems[6])})
    return results


def save_bop_results(path, results):
    lines = [HEADER]
    for res in results:
        lines.append("{},{},{},{},{},{},{}".format(
            res["scene_id"], res["im_id"], res["obj_id"], res["score"], " ".join(map(str, np.asarray(res["R"]).flatten().tolist())),
            " ".join(map(str, np.asarray(res["t"]).flatten().tolist())), res["time"] if "time" in res else -1))
    with open(path, "w") as f:
        f.write("\n".join(lines))
