"""micro-benchmark of row N27 (cp_paste_masks, cp_paste_rle_count / cp_paste_rle_write).  Not read by bench.py.

  python tools/paste_masks_bench.py [--out profiles/paste_masks_bench.json] [--rounds 9] [--calls 200] [--warmup 3] [--masks 256]
  python tools/paste_masks_bench.py --resources      (only where hipcc is: adds the compiler's figures of the new kernels to the file)

Shape: B = 256 masks, frames of 480 x 640, seg planes of 64 x 64 (a disc of random centre and radius per plane, so the RLE has runs),
square windows of 100 to 200 pixels at random places, some over the frame's edges.
Timed, each with device events around `--calls` back-to-back calls after `--warmup` warm-up calls, in `--rounds` rounds whose order
alternates (forwards, backwards) so that no variant always runs after the same neighbour; every round's figure is kept:
  paste_masks          postprocess.paste_masks, the whole Python call
  rle_encode           coco_eval.rle_encode on its output: the parent's code, the BASELINE of the direct RLE (count, cumulative sum, one
                       host read of the total, write)
  paste_masks+rle_encode   the two together: the route from the logits to the RLE without the direct pair
  paste_masks_rle      postprocess.paste_masks_rle, the whole Python call: the windows made on the host and uploaded (as in paste_masks),
                       then the same host steps as rle_encode around cp_paste_rle_count / _write
  coco_rle_launches / paste_rle_launches
                       the two launches alone (count + write) with the offsets already made: the kernels without the host's share
The SPREAD of a variant is (max - min) of its rounds; the direct RLE pair is kept only if its median is below the baseline's by more than
the larger of the two spreads -- for the launches (the kernels against the parent's kernels on the same masks) and for the whole route
from the logits (paste_masks_rle against paste_masks + rle_encode); the file holds both verdicts and every figure.  The outputs of the
two routes are compared at the timed size first."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("paste_masks_kernel", "paste_rle_kernelILb0", "paste_rle_kernelILb1", "coco_unpack_kernel")


def kernel_resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    res = {}
    for name in ("paste_masks.hip", "coco_eval.hip"):
        src = os.path.join(ROOT, "checkerpose_amd", "csrc", name)
        try:
            out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c", src, "-o", os.devnull,
                                  "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900).stderr
        except (OSError, subprocess.SubprocessError):
            return "UNMEASURED"
        for block in out.split("Function Name: ")[1:]:
            kernel = next((k for k in KERNELS if k in block.split()[0]), None)
            if kernel is None:
                continue
            fig = {}
            for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("static_lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
                m = re.search(pat, block)
                fig[key] = int(m.group(1)) if m else "UNMEASURED"
            res[kernel.replace("ILb0", "<count>").replace("ILb1", "<write>")] = fig
    return res or "UNMEASURED"


def make_inputs(B, H, W, S, seed=0):
    """-> (seg (B,2,S,S) float32, boxes (B,4) int: squares of 100..200 pixels)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S]
    cx, cy, r = rng.uniform(0.3 * S, 0.7 * S, B), rng.uniform(0.3 * S, 0.7 * S, B), rng.uniform(0.15 * S, 0.4 * S, B)
    disc = r[:, None, None] - np.hypot(xx[None] - cx[:, None, None], yy[None] - cy[:, None, None])
    seg = np.stack([disc, disc + 2.0], 1).astype(np.float32)
    side = rng.integers(100, 201, B)
    boxes = np.stack([rng.integers(-40, W - 60, B), rng.integers(-40, H - 60, B), side, side], 1)
    return seg, boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paste_masks_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--masks", type=int, default=256)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "paste_masks", "timing": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from checkerpose_amd import _abi, coco_eval, postprocess, preprocess
    if not torch.cuda.is_available():
        raise SystemExit("paste_masks_bench: no GPU -- a timing is taken on the device or not at all")
    dev = torch.device("cuda:0")
    B, H, W, S = a.masks, 480, 640, 64
    seg_np, boxes = make_inputs(B, H, W, S)
    seg = torch.from_numpy(seg_np).to(dev)
    size = (H, W)
    packed = postprocess.paste_masks(seg, boxes, size)
    counts, offsets = coco_eval.rle_encode(packed)
    d_counts, d_offsets, d_area, d_box = postprocess.paste_masks_rle(seg, boxes, size)
    equal = bool(torch.equal(counts, d_counts) and torch.equal(offsets, d_offsets) and torch.equal(d_area, packed.area) and torch.equal(d_box, packed.box))
    total = int(offsets[-1])
    win = torch.from_numpy(preprocess._windows(boxes, "crop_square_resize", W, H)).to(dev)
    n_runs = torch.empty(B, dtype=torch.int32, device=dev)
    area, box = torch.empty_like(packed.area), torch.empty_like(packed.box)
    out = torch.empty(total, dtype=torch.int32, device=dev)

    def coco_launches():
        _abi.call("cp_coco_rle_count", dev, packed.bits, B, H, W, n_runs)
        _abi.call("cp_coco_rle_write", dev, packed.bits, B, H, W, offsets, out, total)

    def paste_launches():
        _abi.call("cp_paste_rle_count", dev, seg, 2 * S * S, S, S, win, B, H, W, n_runs, area, box)
        _abi.call("cp_paste_rle_write", dev, seg, 2 * S * S, S, S, win, B, H, W, offsets, out, total)

    variants = [("paste_masks", lambda: postprocess.paste_masks(seg, boxes, size)),
                ("rle_encode", lambda: coco_eval.rle_encode(packed)),
                ("paste_masks+rle_encode", lambda: coco_eval.rle_encode(postprocess.paste_masks(seg, boxes, size))),
                ("paste_masks_rle", lambda: postprocess.paste_masks_rle(seg, boxes, size)),
                ("coco_rle_launches", coco_launches),
                ("paste_rle_launches", paste_launches)]
    for _, fn in variants:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    rounds = {name: [] for name, _ in variants}
    for r in range(a.rounds):
        for name, fn in (variants if r % 2 == 0 else variants[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            rounds[name].append(e0.elapsed_time(e1) / a.calls)
    timing = {}
    for name, ms in rounds.items():
        timing[name] = {"ms_per_call_rounds": [round(v, 5) for v in ms], "median_ms": round(float(np.median(ms)), 5),
                        "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5), "spread_ms": round(max(ms) - min(ms), 5)}

    def verdict(new, base):
        n, b = timing[new], timing[base]
        margin = max(n["spread_ms"], b["spread_ms"])
        return {"new": new, "baseline": base, "gain_ms": round(b["median_ms"] - n["median_ms"], 5), "larger_spread_ms": margin,
                "faster_by_more_than_the_spread": bool(b["median_ms"] - n["median_ms"] > margin)}
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.update({"bench": "paste_masks", "device": torch.cuda.get_device_name(0), "lib_version": int(_abi.load().cp_version()),
                "shape": {"B": B, "H": H, "W": W, "S": S, "window_side": [100, 200], "runs_total": total, "mask_area_mean": float(packed.area.float().mean())},
                "method": {"rounds": a.rounds, "calls_per_round": a.calls, "warmup_calls": a.warmup, "order": "alternating", "clock": "device events"},
                "outputs_equal": equal, "timing": timing,
                "keep_direct_rle": {"launches": verdict("paste_rle_launches", "coco_rle_launches"), "route_from_logits": verdict("paste_masks_rle", "paste_masks+rle_encode")}})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v["median_ms"] for k, v in timing.items()}), json.dumps(res["keep_direct_rle"]), "outputs_equal", equal)


if __name__ == "__main__":
    main()
