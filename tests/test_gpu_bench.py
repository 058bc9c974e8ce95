"""GPU (-m gpu): bench.py's plain run.  Its line carries the headline keys and nothing that takes runs of its own (those are
`--full`'s), and `--dump-outputs` writes what the timed step returns: the same arrays, bit for bit, as the same workload run in this
process on the same seeded crops."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    import bench
    B, steps, warmup = 8, 3, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", str(B), "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "bench")],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["unit"] == "crops/s" and d["higher_is_better"] is True and d["dtype"] == "bf16" and d["steps"] == steps
    assert d["ms_per_step"] > 0 and abs(d["value"] - B * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"] + 0.1
    assert not {"roofline", "kernel_ms_per_step", "cpu_baseline", "by_batch", "configs"} & set(d), sorted(d)
    with torch.no_grad():
        wl = bench.make_workload("lmo_ape", 512, B, "bf16", torch.device("cuda", 0))
        for _ in range(warmup + steps):
            outs = wl["step"]()
        torch.cuda.synchronize()
        bench.dump_outputs(outs, str(tmp_path / "here"))
    for n in bench.OUTPUT_NAMES:
        a, b = np.load(tmp_path / "bench" / (n + ".npy")), np.load(tmp_path / "here" / (n + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.shape[0] == B
        assert np.array_equal(a, b), n
