"""micro-benchmark of row N32: postprocess.refine_poses_lm_weighted (cp_pnp_refine_wlm) beside row N22's refine_poses_lm on
the same poses and points, and postprocess.code_confidence (cp_code_confidence) beside the same arithmetic as a chain of torch ops.

  python tools/wlm_bench.py [--out profiles/wlm_bench.json] [--rounds 5] [--warmup 2] [--calls 10]
  python tools/wlm_bench.py --resources          (only where hipcc is: adds the compiler's figures of the kernels to the file)

B = 256 crops, N = 512 keypoints (tests/wlm_stages.py's outlier crops: sigma per point and axis in [0.3, 3] px, 10 % gross outliers, started
2 degrees and 2 % of |t| off), max_iters = 20 with step_tol = 1e-300, so that no crop stops by the step rule and the variants run the same
number of iterations (the histogram is kept).  Time: device events around `--calls` repeated WHOLE Python calls (buffers allocated, the
pose packed) after `--warmup` warm-up calls; `--rounds` rounds, the variants in alternating order from round to round; per variant the
median over the rounds of the time per call and the spread = max - min.  No time is fixed in advance; the file holds what was measured."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {"pnp_refine_w.hip": "pnp_refine_wlm_kernel", "pnp_refine.hip": "pnp_refine_lm_kernel", "code_confidence.hip": "code_confidence_kernel"}


def kernel_resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    res = {}
    for src, kernel in KERNELS.items():
        try:
            out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c", os.path.join(ROOT, "checkerpose_amd", "csrc", src),
                                  "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900).stderr
        except (OSError, subprocess.SubprocessError):
            return "UNMEASURED"
        for block in out.split("Function Name: ")[1:]:
            if kernel not in block.split()[0]:
                continue
            fig = {}
            for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                             ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"), ("static_lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)"),
                             ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
                m = re.search(pat, block)
                fig[key] = int(m.group(1)) if m else "UNMEASURED"
            res[kernel] = fig
    return res or "UNMEASURED"


def torch_confidence(bits, bbox, Hc, Wc, floor=1.0 / 12.0):
    """cp_code_confidence's arithmetic for r = 6 as torch ops on the device"""
    import torch
    z = bits.double()
    e = torch.exp(-z.abs())
    q = e / ((1.0 + e) * (1.0 + e))
    w = torch.tensor([4.0 ** (5 - j) for j in range(6)], dtype=torch.float64, device=bits.device)[None, :, None]
    vx, vy = (w * q[:, 1:7]).sum(1), (w * q[:, 7:13]).sum(1)
    sx, sy = (bbox[:, 2].double() / Wc)[:, None], (bbox[:, 3].double() / Hc)[:, None]
    return torch.stack([sx * sx * (floor + vx), sy * sy * (floor + vy)], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wlm_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "wlm", "timing": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from checkerpose_amd import _abi
    from checkerpose_amd.postprocess import code_confidence, refine_poses_lm, refine_poses_lm_weighted
    from tests import wlm_stages as W
    lib = _abi.load()
    dev = torch.device("cuda:0")
    B, N = 256, 512
    case = W._make("bench", 4242, B, N, "outlier")
    p3, K = torch.from_numpy(case.p3d).float().to(dev), torch.from_numpy(case.K).float().to(dev)
    p2, mask, scale = torch.from_numpy(case.p2d).float().to(dev), torch.from_numpy(case.mask).to(dev).bool(), torch.from_numpy(case.scale).to(dev)
    R0, t0 = torch.from_numpy(case.R0).to(dev), torch.from_numpy(case.t0).to(dev)
    rng = np.random.default_rng(7)
    block = torch.from_numpy((4.0 * rng.normal(size=(B, 13, N))).astype(np.float32)).to(dev)
    outputs = (block[:, :1], block[:, 1:7], block[:, 7:], torch.zeros(B, 2, 64, 64, device=dev), None, None)
    bbox = torch.from_numpy(rng.integers(32, 320, size=(B, 4)).astype(np.int32)).to(dev)
    kw = dict(max_iters=20, step_tol=1e-300)
    variants = {
        "refine_poses_lm_weighted_delta_2.5": lambda: refine_poses_lm_weighted(p3, p2, mask, scale, K, R0, t0, 2.5, **kw),
        "refine_poses_lm_weighted_delta_inf": lambda: refine_poses_lm_weighted(p3, p2, mask, scale, K, R0, t0, float("inf"), **kw),
        "refine_poses_lm": lambda: refine_poses_lm(p3, p2, mask, K, R0, t0, **kw),
        "code_confidence": lambda: code_confidence(outputs, bbox),
        "code_confidence_torch_ops": lambda: torch_confidence(block, bbox, 64, 64),
    }
    dev_max = float((torch_confidence(block, bbox, 64, 64) / code_confidence(outputs, bbox) - 1.0).abs().max())
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for r in range(a.rounds):
        order = list(variants) if r % 2 == 0 else list(variants)[::-1]
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                variants[name]()
            e1.record()
            e1.synchronize()
            rounds[name].append(e0.elapsed_time(e1) / a.calls)
    timing = {k: {"ms_per_call_median": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "rounds_ms": v} for k, v in rounds.items()}
    iters = {}
    for name in list(variants)[:3]:
        out = variants[name]()
        it = out[3]["iters"].cpu().numpy()
        iters[name] = {"status_counts": {str(k): int((out[2] == k).sum()) for k in range(4)},
                       "iterations_histogram": {str(k): int((it == k).sum()) for k in sorted(set(it.tolist()))}}
    for k, v in timing.items():
        print("%-38s %.4f ms per call (spread %.4f)" % (k, v["ms_per_call_median"], v["spread_ms"]), flush=True)
    res = {"bench": "wlm", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()), "B": B, "N": N,
           "method": "device events around %d repeated whole calls after %d warm-up calls; %d rounds, the variants in alternating order; median over "
                     "the rounds, spread = max - min; max_iters = 20, step_tol = 1e-300" % (a.calls, a.warmup, a.rounds),
           "timing": timing, "iterations": iters, "code_confidence_torch_ops_max_relative_deviation": dev_max, "kernel_resources": "UNMEASURED"}
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
