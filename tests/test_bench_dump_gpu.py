"""bench.py --dump-outputs on the device: `--steps` sets the timed steps of the result line, `ms_per_step` is their time,
and the dumped outputs of the last timed step are the path's own (label map, trimap, mask of sampled images against the CPU
oracle on the same seeded inputs and weights).  Run as a child process, like the driver runs bench.py."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_bench_dumps_the_last_timed_step(tmp_path, gpu_ctx, oracle):
    import bench
    from gcn_grabcut.model import ResGCNNet
    from gcn_grabcut.synthetic import synthetic_batch

    batch, steps = 12, 3
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(batch),
           "--cpu-sample", "0", "--cpu-all", "0", "--h2d-steps", "0", "--overlap-pass", "0", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(batch * 1e3 / line["ms_per_step"], rel=1e-2)

    files = sorted(p.name for p in tmp_path.glob("*.npy"))
    assert files == line["dumped_outputs"]["files"]
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_MAX_BYTES

    torch.manual_seed(0)                                          # bench.py's weights and inputs
    sd = {k: v.numpy() for k, v in ResGCNNet(hidden_channels=bench.HIDDEN, n_layers=bench.LAYERS).state_dict().items()
          if v.dtype.is_floating_point}
    imgs = synthetic_batch(batch, bench.H, bench.W, config_id=3, first_index=0)
    pick = got["sample_index"].astype(np.int64)
    for k in (0, len(pick) - 1):
        i = int(pick[k])
        want = oracle.segment(imgs[i], sd, bench.HIDDEN, bench.LAYERS, n_segments=bench.N_SEGMENTS, seed=i)
        assert np.array_equal(got["segments"][k], want["segments"])
        assert np.array_equal(got["trimap"][k], want["trimap"])
        assert np.array_equal(got["binary_mask"][k], want["binary_mask"])
