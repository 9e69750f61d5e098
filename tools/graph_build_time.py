"""Wall time of the graph build (ggc_graph_count + ggc_graph_fill, stream synchronised) on the bench's image shape
(400x300, 600 segments) at several batch sizes, and the device memory the first call of the process takes.

    python3 tools/graph_build_time.py [TAG]          BS=256,16,1 chooses the batch sizes
    GGC_HIP_LIBRARY=<parent's libggc_hip.so> ...     another build of the library
    GGC_GRAPH_ONCHIP=0|1|2 ...                       dense matrix | on-chip tables from 24 images on | on-chip at any size
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
sizes = [int(x) for x in os.environ.get("BS", "256,128,64,32,16,8,1").split(",")]
ctx = _native.get_context(0)
bgr = synthetic_batch(max(sizes), 300, 400, config_id=4)
_, lab, hsv, gray, grad = gh.preprocess(ctx, bgr)
seg, nn = gh.slic(ctx, lab, 600)
torch.cuda.synchronize()
print(tag, "Nmax", int(nn.max()), "Nmin", int(nn.min()))
for b in sizes:
    args = [t[:b].contiguous() for t in (seg, nn, lab, hsv, grad)]
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    g = gh.graph(ctx, *args, 4, 4)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    ts = []
    for it in range(40):
        torch.cuda.synchronize()
        t = time.perf_counter()
        g = gh.graph(ctx, *args, 4, 4)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    ts = np.sort(np.array(ts[5:]))
    print(f"{tag} B={b:3d} graph build ms: median {np.median(ts):.3f} min {ts[0]:.3f} p90 {ts[int(len(ts) * 0.9)]:.3f}  "
          f"device memory taken by the first call {(free0 - free1) / 2**20:.1f} MiB  edges {int(g['edge_ptr'][-1])}")
