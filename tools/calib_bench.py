"""micro-benchmark of row N34: postprocess.reliability (cp_code_reliability), postprocess.fit_code_scale
(cp_fit_code_scale) and postprocess.sigma2_consistency (cp_sigma2_consistency), each beside the composition a user could already write
in torch float64 elementwise operations and reductions -- for the fit, the same bracketed iteration driven from the host, one
evaluation and one read-back per step.

  python tools/calib_bench.py [--out profiles/calib_bench.json] [--rounds 5] [--warmup 2] [--calls 3] [--B 10000]
  python tools/calib_bench.py --resources          (only where hipcc is: adds the compiler's figures of the kernels to the file)

B = 10 000 crops, N = 512 keypoints, r = 6: a validation set's 13-row logit block (266 MB) and its labels, made on the device: logits
z = t / s0 with t ~ 2.5 N(0, 1) and one s0 per row in [2^-1.5, 2^1.5], labels drawn from sigmoid(t) (row 0's are the GT RoI bits: about half of the keypoints lie
inside).  Time: device events around `--calls` repeated WHOLE Python calls (buffers allocated) after `--warmup` warm-up calls; `--rounds`
rounds, the variants in alternating order from round to round; per variant the median over the rounds of the time per call and the
spread = max - min.  The file also carries, over the committed cases of tests/calib_stages.py, the largest ratio of |device - fsum| to the
derived bound (n + 8) 2^-53 fsum|terms| per kind of sum: the measurement behind tests/calib_stages.py's TRANSCENDENTAL_FACTOR.  No time
is fixed in advance; the file holds what was measured, a loss included."""
import argparse
import json
import math
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {"calibrate.hip": ("calib_reliability_kernel", "calib_reliability_finish_kernel", "calib_fit_accum_kernel", "calib_fit_step_kernel",
                             "calib_fit_init_kernel", "calib_pit_kernel")}


def kernel_resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    res = {}
    for src, kernels in KERNELS.items():
        try:
            out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c", os.path.join(ROOT, "checkerpose_amd", "csrc", src),
                                  "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900).stderr
        except (OSError, subprocess.SubprocessError):
            return "UNMEASURED"
        for block in out.split("Function Name: ")[1:]:
            for kernel in kernels:
                if kernel + "E" not in block.split()[0]:
                    continue
                fig = {}
                for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                                 ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                                 ("static_lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)"),
                                 ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
                    m = re.search(pat, block)
                    fig[key] = int(m.group(1)) if m else "UNMEASURED"
                res[kernel] = fig
    return res or "UNMEASURED"


def torch_terms(torch, z32, y, s):
    """the rule's per-sample terms as torch float64 elementwise operations; s broadcasts over (B, K, N)"""
    z = z32.double()
    t = z * s
    e = torch.exp(-t.abs())
    p = torch.where(t >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    d = p - y
    nll = torch.log1p(e) + torch.where(y > 0.5, (-t).clamp_min(0.0), t.clamp_min(0.0))
    return t, p, nll, d


def torch_reliability(torch, bits, y, mask, scale, edges):
    """the user's composition: bucketize + bincount per (row, bin), masked reductions per row"""
    B, K, N = bits.shape
    M = edges.numel() + 1
    t, p, nll, d = torch_terms(torch, bits, y, scale.view(1, K, 1))
    z = bits.double()
    idx = torch.bucketize(t, edges, right=True) + M * torch.arange(K, device=bits.device).view(1, K, 1)
    sel = idx[mask]
    count = torch.bincount(sel, minlength=K * M).view(K, M)
    positives = torch.bincount(idx[mask & (y > 0.5)], minlength=K * M).view(K, M)
    sum_p = torch.bincount(sel, weights=p[mask], minlength=K * M).view(K, M)
    m = mask.double()
    return dict(count=count, positives=positives, sum_p=sum_p, n=mask.sum((0, 2)), nll=(nll * m).sum((0, 2)), brier=(d * d * m).sum((0, 2)),
                g=(d * z * m).sum((0, 2)), h=(p * (1.0 - p) * z * z * m).sum((0, 2)))


def torch_fit(torch, bits, y, mask, s_min, s_max, tol, max_iters):
    """the committed iteration per row, driven from the host: one torch evaluation of every row and one read-back per step"""
    B, K, N = bits.shape
    s, lo, hi = np.ones(K), np.full(K, s_min), np.full(K, s_max)
    done, evals = np.zeros(K, bool), 0
    z, m = bits.double(), mask.double()
    while not done.all() and evals < max_iters:
        st = torch.from_numpy(s).to(bits.device).view(1, K, 1)
        t, p, nll, d = torch_terms(torch, bits, y, st)
        g = (d * z * m).sum((0, 2)).cpu().numpy()
        h = (p * (1.0 - p) * z * z * m).sum((0, 2)).cpu().numpy()
        evals += 1
        for k in range(K):
            if done[k]:
                continue
            if g[k] < 0:
                lo[k] = s[k]
            else:
                hi[k] = s[k]
            c = s[k] - g[k] / h[k] if h[k] > 0 and np.isfinite(h[k]) else np.nan
            if not lo[k] < c < hi[k]:
                c = math.sqrt(lo[k] * hi[k])
            if abs(c - s[k]) <= tol * s[k]:
                done[k] = True
            s[k] = c
    return s, evals


def torch_pit(torch, p2d, proj, s2, valid, roi, edges, column):
    good = (valid[:, :, column] != 0) & (roi[:, 0, :] > 0.5) & torch.isfinite(s2).all(2) & (s2 > 0).all(2)
    dd = p2d.double() - proj
    d2 = dd[..., 0] * dd[..., 0] / s2[..., 0] + dd[..., 1] * dd[..., 1] / s2[..., 1]
    E = edges.numel()
    B = p2d.shape[0]
    idx = torch.bucketize(d2, edges, right=True) + (E + 1) * torch.arange(B, device=p2d.device).view(B, 1)
    counts = torch.bincount(idx[good], minlength=B * (E + 1)).view(B, E + 1)
    w = dd / s2.sqrt()
    g = good.double()
    return counts, good.sum(1), (torch.nan_to_num(d2) * g).sum(1), (torch.nan_to_num(w[..., 0]) * g).sum(1), (torch.nan_to_num(w[..., 1]) * g).sum(1)


def committed_ratios(torch):
    """largest |device - fsum| / ((n + 8) 2^-53 fsum|terms|) per stage over the committed cases"""
    from checkerpose_amd.postprocess import fit_code_scale, reliability, sigma2_consistency
    from tests import calib_stages as S
    dev = "cuda"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    lab = lambda c: dict(roi_mask_bits=t(c["roi"]), pixel_x_codes=t(c["gx"]), pixel_y_codes=t(c["gy"]))      # noqa: E731
    npd = lambda d: {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}      # noqa: E731
    rel, fit, pit = {}, {}, {}
    keep = S.TRANSCENDENTAL_FACTOR
    S.TRANSCENDENTAL_FACTOR = 1e30               # measure, do not judge
    try:
        for c in S.reliability_cases():
            S.check_reliability(c, npd(reliability(t(c["bits"]), lab(c), scale=c["scale"], bins=c["M"])), rel)
        for c in S.fit_cases():
            scale, info = fit_code_scale(t(c["bits"]), lab(c), groups=c["groups"], s_min=c["s_min"], s_max=c["s_max"], step_tol=c["step_tol"],
                                         max_iters=c["max_iters"])
            try:
                S.check_fit(c, dict(npd(info), scale=scale.cpu().numpy()), fit)
            except S.StageError as e:
                fit["error"] = str(e)
    finally:
        S.TRANSCENDENTAL_FACTOR = keep
    for c in S.pit_cases():
        bins = c["edges"] if len(c["edges"]) else 1
        try:
            S.check_pit(c, npd(sigma2_consistency(t(c["p2d"]), t(c["valid"]), t(c["sigma2"]), dict(proj_xy=t(c["proj"]), roi_mask_bits=t(c["roi"])),
                                                  column=c["column"], bins=bins)), pit)
        except S.StageError as e:
            pit["error"] = str(e)
    return {"reliability": rel, "fit_nll": fit, "sigma2_consistency": pit, "factor_in_tests": keep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calib_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--B", type=int, default=10000)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "calib", "timing": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from checkerpose_amd import _abi
    from checkerpose_amd.calibrate import chi2_edges, logit_edges
    from checkerpose_amd.postprocess import fit_code_scale, reliability, sigma2_consistency
    lib = _abi.load()
    dev = torch.device("cuda:0")
    B, N, r, K, M = a.B, 512, 6, 13, 15
    gen = torch.Generator(device=dev)
    gen.manual_seed(3434)
    s0 = torch.exp2(torch.rand(K, generator=gen, device=dev, dtype=torch.float64) * 3.0 - 1.5)
    t_true = torch.randn(B, K, N, generator=gen, device=dev) * 2.5
    bits = (t_true.double() / s0.view(1, K, 1)).float()
    y = (torch.rand(B, K, N, generator=gen, device=dev) < torch.sigmoid(t_true)).float()
    del t_true
    labels = dict(roi_mask_bits=y[:, :1].contiguous(), pixel_x_codes=y[:, 1:7].contiguous(), pixel_y_codes=y[:, 7:].contiguous())
    mask = (y[:, :1] > 0.5).expand(B, K, N).clone()
    mask[:, 0, :] = True
    yd = y.double()
    ones = torch.ones(K, dtype=torch.float64, device=dev)
    e_logit = torch.from_numpy(logit_edges(M)).to(dev)
    proj = torch.rand(B, N, 2, generator=gen, device=dev, dtype=torch.float64) * 350.0 + 50.0
    s2 = torch.rand(B, N, 2, generator=gen, device=dev, dtype=torch.float64) * 20.0 + 0.5
    p2d = (proj + s2.sqrt() * torch.randn(B, N, 2, generator=gen, device=dev, dtype=torch.float64)).float()
    valid = (torch.rand(B, N, 3, generator=gen, device=dev) < 0.8).to(torch.uint8)
    targets = dict(proj_xy=proj, roi_mask_bits=labels["roi_mask_bits"])
    e_chi = torch.from_numpy(chi2_edges(10)).to(dev)
    fit_kw = dict(s_min=2.0 ** -6, s_max=2.0 ** 6, step_tol=1e-8, max_iters=60)
    variants = {
        "reliability": lambda: reliability(bits, labels, bins=M),
        "torch_reliability": lambda: torch_reliability(torch, bits, yd, mask, ones, e_logit),
        "fit_code_scale": lambda: fit_code_scale(bits, labels, **fit_kw),
        "torch_fit_host_driven": lambda: torch_fit(torch, bits, yd, mask, fit_kw["s_min"], fit_kw["s_max"], fit_kw["step_tol"], fit_kw["max_iters"]),
        "sigma2_consistency": lambda: sigma2_consistency(p2d, valid, s2, targets, gates=()),
        "torch_sigma2_consistency": lambda: torch_pit(torch, p2d, proj, s2, valid, labels["roi_mask_bits"], e_chi, 0),
    }
    # the pairs compute the same thing
    acc, ref = reliability(bits, labels, bins=M), torch_reliability(torch, bits, yd, mask, ones, e_logit)
    assert torch.equal(acc["count"], ref["count"]) and torch.equal(acc["positives"], ref["positives"]) and torch.equal(acc["n"], ref["n"])
    assert torch.allclose(acc["nll"], ref["nll"], rtol=1e-9) and torch.allclose(acc["sum_p"], ref["sum_p"], rtol=1e-9)
    scale, info = fit_code_scale(bits, labels, **fit_kw)
    s_host, evals_host = torch_fit(torch, bits, yd, mask, fit_kw["s_min"], fit_kw["s_max"], fit_kw["step_tol"], fit_kw["max_iters"])
    assert np.allclose(scale.cpu().numpy(), s_host, rtol=1e-6), (scale.cpu().numpy(), s_host)
    pit, pref = sigma2_consistency(p2d, valid, s2, targets, gates=()), torch_pit(torch, p2d, proj, s2, valid, labels["roi_mask_bits"], e_chi, 0)
    assert torch.equal(pit["counts"].long(), pref[0]) and torch.equal(pit["n"].long(), pref[1])
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for rd in range(a.rounds):
        names = list(variants) if rd % 2 == 0 else list(variants)[::-1]
        for name in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                variants[name]()
            e1.record()
            e1.synchronize()
            rounds[name].append(e0.elapsed_time(e1) / a.calls)
    timing = {k: {"ms_per_call_median": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "rounds_ms": v} for k, v in rounds.items()}
    for k, v in timing.items():
        print("%-28s %.4f ms per call (spread %.4f)" % (k, v["ms_per_call_median"], v["spread_ms"]), flush=True)
    se = 1.0 / np.sqrt(reliability(bits, labels, scale=scale, bins=2)["h"].cpu().numpy())
    res = {"bench": "calib", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()), "B": B, "N": N, "r": r, "bins": M,
           "bytes_read_per_pass": int(bits.numel() * 4 + y.numel() * 4),
           "method": "device events around %d repeated whole calls after %d warm-up calls; %d rounds, the variants in alternating order; median over "
                     "the rounds, spread = max - min" % (a.calls, a.warmup, a.rounds),
           "timing": timing,
           "fit": {"evaluations_per_group_device": info["iters"].tolist(), "status_device": info["status"].tolist(), "launch_pairs_enqueued": fit_kw["max_iters"] + 1,
                   "evaluations_host_driven": int(evals_host), "s_device": scale.cpu().numpy().tolist(), "s0": s0.cpu().numpy().tolist(),
                   "distance_in_standard_errors": ((scale.cpu().numpy() - s0.cpu().numpy()) / se).tolist(),
                   "nll_before": info["nll_before"].tolist(), "nll_after": info["nll_after"].tolist()},
           "sigma2_consistency": {"inflation": pit["inflation"], "counts_total": pit["counts_total"].tolist(), "n_total": pit["n_total"]},
           "sum_bound_ratios_on_committed_cases": committed_ratios(torch),
           "kernel_resources": "UNMEASURED"}
    if os.path.exists(a.out):
        old = json.load(open(a.out))
        if old.get("kernel_resources", "UNMEASURED") != "UNMEASURED":
            res["kernel_resources"] = old["kernel_resources"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
