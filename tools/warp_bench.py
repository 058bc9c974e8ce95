"""micro-benchmark of cp_warp_affine_u8 beside cp_crop_resize_u8, the crop kernel that writes the same bytes.

  python tools/warp_bench.py [--out profiles/warp_bench.json] [--windows 9] [--launches 50] [--warmup 20] [--crops 256] [--crop 256]

Both kernels cut the SAME boxes: `--crops` detections (sides 40 .. 300, some over the frame's edges) padded by 1.5 as the loader does, from
16 frames of 640 x 480 x 3 through an img_index, INTER_LINEAR, to crop x crop x 3 -- "crop_square_resize" windows for the old kernel, the
inverse maps of "crop_resize_by_warp_affine" for the new one.  The C entry points are called directly on operands that are already on the
device (the Python wrappers' host arithmetic and uploads are the same handful of numbers per box on both sides and are not what is
compared).  Time: device events around `--launches` back-to-back launches, after `--warmup` launches of each kernel; the sides alternate
window by window in one process; per side the median, minimum and maximum of the windows' per-launch times are kept, with every window.
Bytes: the crops written (crops x crop x crop x 3) plus, as the least a kernel can read, each frame once; the rate is those bytes over the
median time -- a lower bound of the traffic, not a share of peak.  No speed is required of this row."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_bench.json"))
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--crops", type=int, default=256)
    ap.add_argument("--crop", type=int, default=256)
    a = ap.parse_args()
    import torch
    from checkerpose_amd import _abi
    from checkerpose_amd import preprocess as PP
    if not torch.cuda.is_available():
        raise SystemExit("warp_bench: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    W, H, n_img, B, S = 640, 480, 16, a.crops, a.crop
    rng = np.random.default_rng(21)
    frames = torch.from_numpy(rng.integers(0, 256, size=(n_img, H, W, 3), dtype=np.uint8)).to(dev)
    boxes = []
    for _ in range(B):
        w, h = int(rng.integers(40, 300)), int(rng.integers(40, 300))
        boxes.append(PP.padding_Bbox([int(rng.integers(-40, W - 40)), int(rng.integers(-40, H - 40)), w, h], 1.5))
    idx = torch.from_numpy(rng.integers(0, n_img, size=B).astype(np.int32)).to(dev)
    win = torch.from_numpy(PP._windows(boxes, "crop_square_resize", W, H)).to(dev)
    inv = torch.from_numpy(PP._inverse_maps([PP._roi_affine(b, W, H, S) for b in boxes], False, S, S)).to(dev)
    out_old = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    out_new = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    lib = _abi.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    sides = {
        "cp_crop_resize_u8": lambda: _abi.check(lib.cp_crop_resize_u8(st, frames.data_ptr(), n_img, H, W, 3, win.data_ptr(), idx.data_ptr(),
                                                                      out_old.data_ptr(), B, S, 1), "cp_crop_resize_u8"),
        "cp_warp_affine_u8": lambda: _abi.check(lib.cp_warp_affine_u8(st, frames.data_ptr(), n_img, H, W, 3, inv.data_ptr(), idx.data_ptr(),
                                                                      out_new.data_ptr(), B, S, S, 1), "cp_warp_affine_u8"),
    }
    for fn in sides.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in sides}
    for _ in range(a.windows):
        for name, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            windows[name].append(1000.0 * e0.elapsed_time(e1) / a.launches)
    least_bytes = B * S * S * 3 + n_img * H * W * 3
    res = {"bench": "warp_affine", "device": torch.cuda.get_device_name(0), "lib_version": int(lib.cp_version()), "frame": [W, H], "frames": n_img,
           "crops": B, "crop": S, "interpolation": "INTER_LINEAR", "launches_per_window": a.launches, "warmup_launches": a.warmup,
           "least_bytes_per_launch": least_bytes, "sides": {}}
    for name, us in windows.items():
        med = float(np.median(us))
        res["sides"][name] = {"us_per_launch_median": med, "us_per_launch_min": float(min(us)), "us_per_launch_max": float(max(us)),
                              "windows_us": [float(v) for v in us], "least_bytes_over_median_GBps": least_bytes / med / 1e3}
    # the two resamplers agree where nothing is resampled; elsewhere they differ by design -- recorded, not required
    diff = (out_old.to(torch.int16) - out_new.to(torch.int16)).abs()
    res["outputs"] = {"max_abs_difference": int(diff.max()), "share_of_equal_bytes": float((diff == 0).float().mean())}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["sides"], indent=1))


if __name__ == "__main__":
    main()
