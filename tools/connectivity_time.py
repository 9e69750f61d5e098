"""Wall time of ggc_slic_enforce_connectivity (stream synchronised) on the raw k-means label maps of the bench's images
(400x300, 600 segments) at several batch sizes, and the device memory the first call of the process takes.

    python3 tools/connectivity_time.py [TAG]         BS=256,64,8,1 chooses the batch sizes
    GGC_HIP_LIBRARY=<parent's libggc_hip.so> ...     another build of the library
    GGC_SLIC_CN_TILES=0|1 ...                        rounds on a pending plane throughout | tile-local first round
"""
import os
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [root, os.path.join(root, "src"), os.path.join(root, "tests")]
import numpy as np
import torch

import gpu_helpers as gh
from gcn_grabcut import _native
from gcn_grabcut.synthetic import synthetic_batch

tag = sys.argv[1] if len(sys.argv) > 1 else "run"
sizes = [int(x) for x in os.environ.get("BS", "256,64,8,1").split(",")]
H, W, NSEG = 300, 400, 600
ctx = _native.get_context(0)
# the raw maps come from a context of their own, so that the timed context's first call is the connectivity pass
src = _native.Context(0)
bgr = synthetic_batch(max(sizes), H, W, config_id=4)
lab = gh.preprocess(src, bgr)[1]
gh.slic(src, lab, NSEG)
raw_h = np.empty((max(sizes), H, W), np.int32)
src.call("ggc_debug_read_scratch", b"slic_raw_labels", raw_h.ctypes.data, raw_h.nbytes)
raw = torch.as_tensor(raw_h).cuda()
seg_size = H * W / NSEG                                              # ggc_slic's own min_size and max_size
mn, mx = int(0.5 * seg_size), int(3.0 * seg_size)
src.close()
del lab
torch.cuda.synchronize()
torch.cuda.empty_cache()


def run(b, out, n):
    ctx.call("ggc_slic_enforce_connectivity", _native.current_stream(0), b, H, W, raw.data_ptr(), mn, mx, out.data_ptr(),
             n.data_ptr())
    torch.cuda.synchronize()


for b in sizes:
    out = torch.empty(b, H, W, dtype=torch.int32, device="cuda")
    n = torch.empty(b, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    run(b, out, n)
    free1, _ = torch.cuda.mem_get_info()
    ts = []
    for it in range(40):
        torch.cuda.synchronize()
        t = time.perf_counter()
        run(b, out, n)
        ts.append((time.perf_counter() - t) * 1e3)
    ts = np.sort(np.array(ts[5:]))
    print(f"{tag} B={b:3d} connectivity ms: median {np.median(ts):.3f} min {ts[0]:.3f} p90 {ts[int(len(ts) * 0.9)]:.3f}  "
          f"device memory taken by the first call {(free0 - free1) / 2**20:.1f} MiB  nodes {int(n.sum())}")
