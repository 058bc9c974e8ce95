"""micro-benchmark of row N29 (cp_coco_rle_unpack).  Not read by bench.py.

  python tools/rle_unpack_bench.py [--out profiles/rle_unpack_bench.json] [--rounds 5] [--warmup 2] [--masks 256,2048]
  python tools/rle_unpack_bench.py --resources      (only where hipcc is: adds the compiler's figures of the new kernels to the file)

Shape: N = 256 and 2 048 masks of 480 x 640 from seeded blobs (an ellipse of random centre and radii per mask, some over the frame's
edges), as the RLE dicts an annotation or result file holds.
Timed, after `--warmup` warm-up calls of every variant, in `--rounds` rounds whose order alternates (forwards, backwards) so that no
variant always runs after the same neighbour; every round's figure is kept:
  pack_rles            coco_eval.pack_rles, from the dicts to PackedMasks: flatten on the host, one small upload per 512 masks,
                       cp_coco_rle_unpack.  Wall clock around a device synchronise.
  pack_rles_parent     the parent commit's pack_rles, kept here as a local function: rle_decode on the host (np.repeat per mask into dense
                       bytes), the upload of 512 dense masks at a time, cp_coco_pack.  Wall clock around a device synchronise: it is
                       host-bound.
  pack_rles_strings    pack_rles on the same masks with pycocotools' compressed strings as counts (the parent refuses them).
  rle_unpack           coco_eval.rle_unpack(check=False) alone from resident run lists, device events around `--calls` calls.
The SPREAD of a variant is (max - min) of its rounds.  The claim under test: pack_rles is not slower than pack_rles_parent at either size
-- the new median is at most the parent's median plus the larger of the two spreads; the file holds the verdict and every figure, and the
bytes each path uploads.  The outputs of the two paths are compared at the timed size first."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("rle_scan_kernel", "rle_bits_kernel")


def kernel_resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "checkerpose_amd", "csrc", "rle_unpack.hip")
    try:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c", src, "-o", os.devnull,
                              "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900).stderr
    except (OSError, subprocess.SubprocessError):
        return "UNMEASURED"
    res = {}
    for block in out.split("Function Name: ")[1:]:
        kernel = next((k for k in KERNELS if k in block.split()[0]), None)
        if kernel is None:
            continue
        fig = {}
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("static_lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, block)
            fig[key] = int(m.group(1)) if m else "UNMEASURED"
        res[kernel] = fig
    return res or "UNMEASURED"


def column_major_rle(mask):
    flat = np.asarray(mask, bool).ravel(order="F")
    change = np.nonzero(flat[1:] != flat[:-1])[0] + 1
    counts = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return ([0] + counts) if flat[0] else counts


def make_rles(N, H, W, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(N):
        cy, cx, ry, rx = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(20, 120), rng.uniform(20, 120)
        out.append({"counts": column_major_rle(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0), "size": [H, W]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_unpack_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--masks", default="256,2048")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {"bench": "rle_unpack", "sizes": "UNMEASURED"}
        res["kernel_resources"] = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_resources"]))
        return
    import torch
    from checkerpose_amd import _abi
    from checkerpose_amd import coco_eval as CE
    if not torch.cuda.is_available():
        raise SystemExit("rle_unpack_bench: no GPU -- a timing is taken on the device or not at all")
    dev = torch.device("cuda:0")
    H, W = 480, 640

    def pack_rles_parent(rles, device, chunk=512):
        return CE.concat_packed([CE.pack_masks(CE.rle_decode(rles[i:i + chunk]), device) for i in range(0, len(rles), chunk)])

    sizes = {}
    ns = [int(v) for v in a.masks.split(",")]
    all_rles = make_rles(max(ns), H, W)                           # the smaller sizes are its first masks
    for N in ns:
        rles = all_rles[:N]
        strings = [dict(r, counts=CE.rle_to_string(r["counts"])) for r in rles]
        new, old = CE.pack_rles(rles, dev), pack_rles_parent(rles, dev)
        same = lambda p, q: bool(torch.equal(p.bits, q.bits) and torch.equal(p.area, q.area) and torch.equal(p.box, q.box))      # noqa: E731
        equal = same(new, old) and same(CE.pack_rles(strings, dev), old)
        counts_h, offsets_h, _ = CE.rle_flatten(rles)
        counts, offsets = torch.from_numpy(counts_h).to(dev), torch.from_numpy(offsets_h).to(dev)

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def events(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.calls

        variants = [("pack_rles", lambda: wall(lambda: CE.pack_rles(rles, dev))),
                    ("pack_rles_parent", lambda: wall(lambda: pack_rles_parent(rles, dev))),
                    ("pack_rles_strings", lambda: wall(lambda: CE.pack_rles(strings, dev))),
                    ("rle_unpack", lambda: events(lambda: CE.rle_unpack(counts, offsets, H, W, check=False)))]
        for _, fn in variants:
            for _ in range(a.warmup):
                fn()
        rounds = {name: [] for name, _ in variants}
        for r in range(a.rounds):
            for name, fn in (variants if r % 2 == 0 else variants[::-1]):
                rounds[name].append(fn())
        timing = {}
        for name, ms in rounds.items():
            timing[name] = {"ms_per_call_rounds": [round(v, 4) for v in ms], "median_ms": round(float(np.median(ms)), 4),
                            "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "spread_ms": round(max(ms) - min(ms), 4),
                            "clock": "device events" if name == "rle_unpack" else "wall clock around a device synchronise"}
        n, b = timing["pack_rles"], timing["pack_rles_parent"]
        margin = max(n["spread_ms"], b["spread_ms"])
        sizes[str(N)] = {"masks": N, "runs_total": int(len(counts_h)), "runs_per_mask_mean": round(len(counts_h) / N, 1),
                         "mask_area_mean": float(new.area.float().mean()), "outputs_equal": equal,
                         "upload_bytes": {"pack_rles": int(counts_h.nbytes + offsets_h.nbytes + 8 * ((N - 1) // 512)), "pack_rles_parent": N * H * W},
                         "timing": timing,
                         "not_slower_than_parent": {"gain_ms": round(b["median_ms"] - n["median_ms"], 4), "larger_spread_ms": margin,
                                                    "speedup_of_medians": round(b["median_ms"] / n["median_ms"], 2),
                                                    "holds": bool(n["median_ms"] <= b["median_ms"] + margin)}}
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.update({"bench": "rle_unpack", "device": torch.cuda.get_device_name(0), "lib_version": int(_abi.load().cp_version()), "frame": [H, W],
                "method": {"rounds": a.rounds, "warmup_calls": a.warmup, "order": "alternating", "calls_per_round_device_events": a.calls},
                "sizes": sizes})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for N, s in sizes.items():
        print(N, json.dumps({k: v["median_ms"] for k, v in s["timing"].items()}), json.dumps(s["not_slower_than_parent"]), "outputs_equal",
              s["outputs_equal"], json.dumps(s["upload_bytes"]))


if __name__ == "__main__":
    main()
