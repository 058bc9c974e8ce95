"""micro-benchmark of augment.augment_frames (cp_augment_frames: background swap + colour chain for a batch of resident frames in one
launch).  tools/mask_error_bench.py's method.

  python tools/augment_bench.py [--out profiles/augment_bench.json] [--calls 100] [--warmup 10] [--repeats 3] [--quick]

Device: events around `--calls` calls after `--warmup` warm-ups, repeated `--repeats` times (median, min and max are recorded: the
run-to-run spread), 640 x 480 frames, one frame per sample, B in {32, 256}, a pool of 8 backgrounds.  The time is that of the whole
Python call (the plan packed and uploaded, the output allocated), as a user pays it.  Configurations:
  full_chain   every stage of every sample on (swap, salt and pepper, motion blur, dropout, Gaussian, table): the worst case, which no
               sampled batch reaches (the chain switches each stage on with probability 0.16 - 0.4);
  sampled      a plan from sample_plan with both optional ops and change_bg 0.5: what a training batch costs;
  all_off      the identity plan: staging and copy only;
  rects_200    full_chain on a 200 x 200 window per sample (what make_training_batch asks for).
Achieved bytes/s counts the compulsory traffic only -- 3 bytes read and 3 written per computed pixel (the tiles that meet the rect),
not the mask, the background or the halo re-reads -- against the 6.3 TB/s an MI355X streams from HBM (8 TB/s peak).
The parent commit has no device composition of this chain, so no ratio is given.  The kernel's share of the call comes from a kernel
trace of the `--quick` run (rocprofv3 --kernel-trace --stats), not from this script."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from checkerpose_amd import _abi  # noqa: E402
from checkerpose_amd import augment as A  # noqa: E402
from tools.bop_error_bench import timed  # noqa: E402

H, W, N_BG = 480, 640, 8
TILE_W, TILE_H = 64, 32
HBM_ACHIEVABLE = 6.3e12


def full_plan(B, rng):
    p = A.AugmentPlan.identity(B, (H, W))
    p.key[:] = rng.integers(0, 1 << 32, size=B, dtype=np.uint64).astype(np.uint32)
    p.bg_index[:] = rng.integers(0, N_BG, size=B)
    p.sp_on[:], p.sp_thresh[:] = 1, A.threshold_u32(A.SP_P)
    p.motion_on[:], p.drop_on[:], p.gauss_on[:] = 1, 1, 1
    p.drop_thresh[:] = A.threshold_u32(A.DROP_P)
    for b in range(B):
        p.motion_w[b] = A.motion_weights(rng.uniform(0, 360), rng.uniform(-1, 1))
        p.gauss_w[b] = A.gaussian_weights(rng.uniform(0.2, 1.0))
        p.lut[b] = A.compose_lut(add=[7, -5, 11], mul_pc=[1.2, 0.9, 1.1], contrast=[1.5, 1.5, 1.5])
    return p


def computed_pixels(rects, B):
    if rects is None:
        return B * H * W
    n = 0
    for x1, y1, x2, y2 in rects:
        tx = range(0, W, TILE_W)
        ty = range(0, H, TILE_H)
        n += sum(min(TILE_W, W - x) * min(TILE_H, H - y) for y in ty for x in tx
                 if x < x2 and x + min(TILE_W, W - x) > x1 and y < y2 and y + min(TILE_H, H - y) > y1)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    calls, warmup, repeats, sizes = a.calls, a.warmup, a.repeats, (32, 256)
    if a.quick:
        calls, warmup, repeats, sizes = 3, 1, 1, (32,)
    rows = []
    for B in sizes:
        rng = np.random.default_rng(B)
        frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
        masks = (torch.rand(B, H, W, device=dev) < 0.3).to(torch.uint8) * 255
        bgs = torch.randint(0, 256, (N_BG, H, W, 3), dtype=torch.uint8, device=dev)
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
        x1, y1 = rng.integers(0, W - 200, size=B), rng.integers(0, H - 200, size=B)
        rects = np.stack([x1, y1, x1 + 200, y1 + 200], 1)
        full = full_plan(B, rng)
        configs = {"full_chain": (full, None),
                   "sampled": (A.sample_plan(B, rng, True, True, change_bg=0.5, n_bg=N_BG, frame_hw=(H, W)), None),
                   "all_off": (A.AugmentPlan.identity(B, (H, W)), None),
                   "rects_200": (full, rects)}
        for name, (plan, rc) in configs.items():
            fn = lambda: A.augment_frames(frames, plan, masks=masks, backgrounds=bgs, rects=rc, out=out)      # noqa: E731
            ts = sorted(timed(fn, calls, warmup) for _ in range(repeats))
            px = computed_pixels(rc, B)
            med = ts[len(ts) // 2]
            row = {"B": B, "config": name, "ms": {"median": med, "min": ts[0], "max": ts[-1]}, "computed_pixels": int(px),
                   "compulsory_bytes": int(6 * px), "achieved_TBps": 6 * px / (med * 1e-3) / 1e12,
                   "share_of_hbm_achievable": 6 * px / (med * 1e-3) / HBM_ACHIEVABLE,
                   "stages_on": {k: float(getattr(plan, k).astype(bool).mean()) for k in ("sp_on", "motion_on", "drop_on", "gauss_on")}}
            rows.append(row)
            print("B=%3d %-10s %.3f ms [%.3f, %.3f]  %.2f TB/s of compulsory traffic (%.0f %% of 6.3 TB/s)"
                  % (B, name, med, ts[0], ts[-1], row["achieved_TBps"], 100 * row["share_of_hbm_achievable"]), flush=True)
    res = {"bench": "augment_frames", "device": torch.cuda.get_device_name(0), "calls": calls, "warmup": warmup, "repeats": repeats,
           "frame": [W, H], "lib_version": int(_abi.load().cp_version()), "hbm_achievable_Bps": HBM_ACHIEVABLE,
           "comparison": "none: the parent commit has no device composition of this chain (the host alternative, imgaug on full frames, "
                         "is not available to measure)", "rows": rows}
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
