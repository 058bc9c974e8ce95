"""micro-benchmark of row N33: postprocess.solve_pnp_conf (cp_pnp_conf), guided and unguided, beside row N4's
solve_pnp_ransac on the same points, and postprocess.rank_correspondences (cp_rank_correspondences) beside torch.sort on the same keys.

  python tools/conf_bench.py [--out profiles/conf_bench.json] [--rounds 5] [--warmup 2] [--calls 10]
  python tools/conf_bench.py --resources          (only where hipcc is: adds the compiler's figures of the kernels to the file)

B = 256 crops, N = 512 keypoints, iterations = 150, on the informative scene of tests/cpnp_stages.py: noise-free crops, every keypoint
valid, half of them outliers (20..80 px off per axis) of which 80 % carry a large variance (9..36 px^2 per axis against 0.25..4);
chi2 = 9.21; row N4 runs at its 2 px.  Time: device events around `--calls` repeated WHOLE Python calls (buffers allocated) after
`--warmup` warm-up calls; `--rounds` rounds, the variants in alternating order from round to round; per variant the median over the
rounds of the time per call and the spread = max - min.  The rounds of 64 hypotheses each solver ran per crop are read from its own
records.  torch.sort sorts the (B, N) keys alone: it neither drops nor compacts, and its ties are not ordered by index.  No time is fixed
in advance; the file holds what was measured."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {"pnp_conf.hip": ("pnp_conf_rank_kernel", "pnp_conf_hypotheses_kernel", "pnp_conf_select_refit_kernel"),
           "pnp.hip": ("pnp_hypotheses_kernel", "pnp_select_refit_kernel")}


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
                if kernel not in block.split()[0]:
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conf_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "conf", "timing": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from checkerpose_amd import _abi
    from checkerpose_amd.postprocess import rank_correspondences, solve_pnp_conf, solve_pnp_ransac
    from tests import cpnp_stages as Cp
    lib = _abi.load()
    dev = torch.device("cuda:0")
    B, N, iterations, chi2 = 256, 512, 150, 9.21
    case = Cp._make("bench", 4343, B, N, 0.5, informative=0.8, valid_frac=1.0, iterations=iterations)
    p3, K = torch.from_numpy(case.p3d).float().to(dev), torch.from_numpy(case.K).float().to(dev)
    p2, valid, s2 = torch.from_numpy(case.p2d).float().to(dev), torch.from_numpy(case.valid).to(dev), torch.from_numpy(case.sigma2).to(dev)
    keys = (s2[:, :, 0] + s2[:, :, 1]).contiguous()
    kw = dict(iterations=iterations, seed=case.seed)
    variants = {
        "solve_pnp_conf_guided": lambda **k: solve_pnp_conf(p3, p2, valid, s2, K, chi2, guided=True, **kw, **k),
        "solve_pnp_conf_unguided": lambda **k: solve_pnp_conf(p3, p2, valid, s2, K, chi2, guided=False, **kw, **k),
        "solve_pnp_ransac": lambda **k: solve_pnp_ransac(p3, p2, valid, K, reproj_threshold=2.0, **kw, **k),
        "rank_correspondences": lambda **k: rank_correspondences(s2, valid),
        "torch_sort_keys": lambda **k: torch.sort(keys, dim=1, stable=True),
    }
    order = rank_correspondences(s2, valid)[0]
    assert torch.equal(order.long(), torch.sort(keys, dim=1, stable=True)[1])          # every keypoint valid and ranked: the same permutation
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for r in range(a.rounds):
        names = list(variants) if r % 2 == 0 else list(variants)[::-1]
        for name in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                variants[name]()
            e1.record()
            e1.synchronize()
            rounds[name].append(e0.elapsed_time(e1) / a.calls)
    timing = {k: {"ms_per_call_median": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "rounds_ms": v} for k, v in rounds.items()}
    ran = {}
    truth_R = np.stack([tr[0] for tr in case.truth])
    for name in list(variants)[:3]:
        out = variants[name](return_hypotheses=True)
        rec = out[-1].cpu().numpy()
        written = (~np.isnan(rec[:, :, 0])).sum(1)
        nr = (written + 63) // 64
        counts = np.where(np.isnan(rec[:, :, 0]), -1, rec[:, :, 0])
        dR = np.abs(out[0].cpu().numpy() - truth_R).max((1, 2))
        ran[name] = {"rounds_per_crop_mean": float(nr.mean()), "rounds_histogram": {str(k): int((nr == k).sum()) for k in sorted(set(nr.tolist()))},
                     "status_1": int((out[3] == 1).sum()), "best_count_mean": float(counts.max(1).mean()),
                     "crops_with_dR_below_1e-4": int((dR < 1e-4).sum())}
    for k, v in timing.items():
        print("%-28s %.4f ms per call (spread %.4f)  %s" % (k, v["ms_per_call_median"], v["spread_ms"], json.dumps(ran.get(k, {}))), flush=True)
    res = {"bench": "conf", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()), "B": B, "N": N, "iterations": iterations,
           "chi2_threshold": chi2,
           "method": "device events around %d repeated whole calls after %d warm-up calls; %d rounds, the variants in alternating order; median over "
                     "the rounds, spread = max - min" % (a.calls, a.warmup, a.rounds),
           "timing": timing, "solvers": ran, "kernel_resources": "UNMEASURED"}
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
