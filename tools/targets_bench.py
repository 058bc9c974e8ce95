"""micro-benchmark of checkerpose_amd.targets against the host path a user has today: the numpy restatement of the reference's loader /
test-loop statements (tests/test_targets.py: host_encode, host_report), run one sample at a time as the loader and test.py do, with
the threads the box sets.

  python tools/targets_bench.py [--out profiles/targets_bench.json] [--replays 100]

Device: events around `--replays` calls after 10 warm-ups -- the whole Python call (uploads of the poses and boxes included), and for
the two kernels also the bare C-ABI launch on tensors already resident.  Rows: encode_targets at (B, N) = (32, 512), (256, 512),
(32, 4096); code_report at B = 256 (N = 512, 6 bits, seg 64 x 64); make_training_batch at B = 32 (640 x 480 frames); and the training
step of bench_train.py's configuration (bf16, B = 32) on one fixed pre-made batch and with make_training_batch in front of every step
(same process, same build, events around 40 steps, two alternated pairs): the added milliseconds.
`cp_kernel_log` is recorded per call (one kernel each).  No speed-up is promised: the parent commit has no device path, the host path
is the comparison."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from checkerpose_amd import _abi, targets  # noqa: E402
from checkerpose_amd import preprocess as PP  # noqa: E402
# the host path that is timed IS the tests' yardstick (the numpy restatement pinned to the reference's recorded labels and counts)
from tests.test_targets import host_encode, host_report, lm_keypoints  # noqa: E402

K_LM = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
DEV = "cuda:0"


def device_ms(fn, replays, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / replays


def host_ms(fn, B, repeats=3):
    fn(0)
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        for b in range(B):
            fn(b)
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def scene(rng, B, pts):
    """poses in front of the camera and final boxes of 0.5 - 1.5 x the projected extent"""
    Rs, ts, boxes = [], [], []
    for _ in range(B):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q *= np.sign(np.linalg.det(q))
        t = np.array([rng.uniform(-120, 120), rng.uniform(-80, 80), rng.uniform(600, 1200)])
        uv = host_encode(pts, K_LM, q, t, [0, 0, 64, 64], 64)["proj_xy"]
        lo, ext = uv.min(0), uv.max(0) - uv.min(0)
        side = int(max(ext) * rng.uniform(0.5, 1.5)) + 8
        c = lo + 0.5 * ext + ext * rng.uniform(-0.3, 0.3, size=2)
        Rs.append(q); ts.append(t); boxes.append([int(c[0] - side / 2), int(c[1] - side / 2), side, side])
    return np.stack(Rs), np.stack(ts), np.array(boxes, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "targets_bench.json"))
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--no-train-step", action="store_true")
    a = ap.parse_args()
    lib = _abi.load()
    rng = np.random.default_rng(0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)      # noqa: E731
    rows = []
    for B, N in ((32, 512), (256, 512), (32, 4096)):
        pts = lm_keypoints(1, N)
        Rs, ts, boxes = scene(rng, B, pts)
        p_d, K_d, R_d, t_d = up(pts), up(K_LM), up(Rs), up(ts)
        lib.cp_kernel_log_begin()
        lab = targets.encode_targets(p_d, K_d, R_d, t_d, boxes, 64)
        log = lib.cp_kernel_log().decode()
        call_ms = device_ms(lambda: targets.encode_targets(p_d, K_d, R_d, t_d, boxes, 64), a.replays)
        boxes_d, flags = up(boxes), np.zeros(B, np.uint8)
        st = torch.cuda.current_stream().cuda_stream
        kernel_ms = device_ms(lambda: lib.cp_encode_targets(st, p_d.data_ptr(), 0, None, 0, K_d.data_ptr(), 0, R_d.data_ptr(), t_d.data_ptr(),
                                                            boxes_d.data_ptr(), boxes.ctypes.data, flags.ctypes.data, B, N, 64,
                                                            lab["roi_mask_bits"].data_ptr(), lab["pixel_x_codes"].data_ptr(),
                                                            lab["pixel_y_codes"].data_ptr(), lab["x_id"].data_ptr(), lab["y_id"].data_ptr(),
                                                            None, None), a.replays)
        h = host_ms(lambda b: host_encode(pts, K_LM, Rs[b], ts[b], boxes[b], 64), B)
        rows.append({"what": "encode_targets", "B": B, "N": N, "S": 64, "device_call_ms": call_ms, "device_kernel_ms": kernel_ms, "host_ms": h,
                     "host_over_device_call": h / call_ms, "kernels": log, "in_roi": float(lab["roi_mask_bits"].mean())})
        print(rows[-1], flush=True)
    # code_report, B = 256
    B, N, nb = 256, 512, 6
    pts = lm_keypoints(1, N)
    Rs, ts, boxes = scene(rng, B, pts)
    lab = targets.encode_targets(up(pts), K_LM, up(Rs), up(ts), boxes, 64)
    outs = (torch.randn(B, 1, N, device=DEV), torch.randn(B, nb, N, device=DEV), torch.randn(B, nb, N, device=DEV), torch.randn(B, 2, 64, 64, device=DEV))
    mv = (torch.rand(B, 64, 64, device=DEV) > 0.5).to(torch.uint8) * 255
    mf = (torch.rand(B, 64, 64, device=DEV) > 0.3).to(torch.uint8) * 255
    lib.cp_kernel_log_begin()
    targets.code_report(outs, lab, mv, mf)
    log = lib.cp_kernel_log().decode()
    call_ms = device_ms(lambda: targets.code_report(outs, lab, mv, mf), a.replays)
    t0 = time.perf_counter()
    host_in = [x.cpu().numpy() for x in outs] + [lab[k].cpu().numpy() for k in ("roi_mask_bits", "pixel_x_codes", "pixel_y_codes")] + [mv.cpu().numpy(), mf.cpu().numpy()]
    pull_ms = (time.perf_counter() - t0) * 1e3
    h = host_ms(lambda b: host_report(*[x[b] for x in host_in]), B)
    rows.append({"what": "code_report", "B": B, "N": N, "nb": nb, "seg": 64, "device_call_ms": call_ms, "host_ms": h, "host_pull_ms": pull_ms,
                 "host_over_device_call": (h + pull_ms) / call_ms, "kernels": log})
    print(rows[-1], flush=True)
    # make_training_batch, B = 32
    B = 32
    pts = lm_keypoints(1, 512)
    Rs, ts, boxes = scene(rng, B, pts)
    frames = torch.randint(0, 256, (B, 480, 640, 3), dtype=torch.uint8, device=DEV)
    masks = (torch.rand(B, 480, 640, device=DEV) > 0.5).to(torch.uint8) * 255
    p_d, R_d, t_d = up(pts), up(Rs), up(ts)
    gt_boxes = [[int(b[0]), int(b[1]), int(b[2]), int(b[3])] for b in boxes]
    mtb = lambda: targets.make_training_batch(frames, masks, masks, R_d, t_d, K_LM, gt_boxes, p_d)      # noqa: E731
    lib.cp_kernel_log_begin()
    mtb()
    log = lib.cp_kernel_log().decode()
    mtb_ms = device_ms(mtb, a.replays)
    # the host's share of the loader for the labels alone (cv2 is not in this image: the three crops are not timed on the host)
    h = host_ms(lambda b: (targets.aug_Bbox(np.array(gt_boxes[b]), 1.5), host_encode(pts, K_LM, Rs[b], ts[b], boxes[b], 64)), B)
    rows.append({"what": "make_training_batch", "B": B, "N": 512, "frame": [480, 640], "device_call_ms": mtb_ms, "host_labels_only_ms": h,
                 "kernels": log})
    print(rows[-1], flush=True)
    res = {"bench": "targets", "device": torch.cuda.get_device_name(0), "replays": a.replays, "warmup": 10, "lib_version": int(lib.cp_version()),
           "torch": torch.__version__, "hip": torch.version.hip, "host_threads": os.environ.get("OMP_NUM_THREADS"),
           "host_path": "numpy restatement of bop_dataset_pytorch.py:21-36,356-373 / test.py:432-457, one sample at a time, float64", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:                  # the rows are kept even if the training-step part below does not finish
        json.dump(res, f, indent=1)
    if not a.no_train_step:
        from bench import Ranks
        import bench_train
        rk = Ranks()
        base = bench_train.run_step_bench(rk, 32, 512, "bf16", 40, 10, False)
        # the same step with a batch made by make_training_batch in front of every step (labels pre-made above = the parent's step)
        from checkerpose_amd.losses.code_loss import MaskedCodeLoss, UnmaskedCodeLoss
        from checkerpose_amd.losses.mask_loss import MaskLoss_interpolate
        from checkerpose_amd.optim import Adam
        from checkerpose_amd.synthetic import build_net
        net = build_net(npoint=512, seed=1).to(DEV).train()
        net.set_compute_dtype("bf16")
        opt = Adam(net.parameters(), lr=2e-4)
        roi_loss, bit_loss, seg_loss = UnmaskedCodeLoss("BCE"), MaskedCodeLoss("BCE"), MaskLoss_interpolate()
        fixed = mtb()

        def step(batch):
            opt.zero_grad(set_to_none=True)
            roi, xb, yb, seg, _, _ = net(batch[0], None, 3)
            nb_ = xb.shape[1]
            loss = roi_loss(roi, batch[7]) + bit_loss(xb, batch[8][:, :nb_], batch[7]) + bit_loss(yb, batch[9][:, :nb_], batch[7]) \
                + seg_loss(seg[:, 0:1], batch[2]) + seg_loss(seg[:, 1:2], batch[1])
            loss.backward()
            opt.step()

        alone = [device_ms(lambda: step(fixed), 40), 0.0]                                          # events around 40 steps after 10 warm-ups
        fed = [device_ms(lambda: step(mtb()), 40), 0.0]
        alone[1], fed[1] = device_ms(lambda: step(fixed), 40), device_ms(lambda: step(mtb()), 40)  # alternated: a second pair
        res["train_step"] = {"config": "bench_train.py's step (bf16, B = 32, N = 512) on uint8 crops, both variants in THIS process and build: "
                                       "'premade' steps on one fixed batch made before the loop (what a step fed pre-made labels costs, the "
                                       "stand-in for the parent commit, which has no other way to get labels), 'fed' makes a new batch with "
                                       "make_training_batch in front of every step; not a cross-commit A/B",
                             "bench_train_ms_per_step": base["ms_per_step"],
                             "step_premade_labels_ms": alone, "step_fed_by_make_training_batch_ms": fed,
                             "added_ms": [f - s for f, s in zip(fed, alone)]}
        rk.close()
        print(res["train_step"], flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
