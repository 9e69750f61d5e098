"""experiment helper: forward time of a trimap network on a batch of DUTS-shape graphs (random weights)

    python3 tools/gcnnet_rate.py [--model gcn|resgcn|gat] [--hidden 128] [--layers 6] [--batch 256] [--heads 8]
"""
import argparse
import os
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "src"))
import numpy as np, torch
from bench import synthetic_region_graph
from gcn_grabcut.data import Batch, Data
from gcn_grabcut.model import GATTrimapNet, GCNTrimapNet, ResGCNNet

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="gcn", choices=["gcn", "resgcn", "gat"])
ap.add_argument("--hidden", type=int, default=128)
ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--heads", type=int, default=8)
ap.add_argument("--batch", type=int, default=int(os.environ.get("B", "256")))
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()
B, D, L = args.batch, args.hidden, args.layers
rng = np.random.default_rng(1)
graphs = [synthetic_region_graph(int(rng.integers(585, 618)), rng) for _ in range(B)]
batch = Batch.from_data_list([Data(x=torch.from_numpy(x), edge_index=torch.from_numpy(ei), edge_attr=torch.from_numpy(ea))
                              for x, ei, ea in graphs]).to("cuda")
torch.manual_seed(0)
if args.model == "gcn":
    m = GCNTrimapNet(hidden_channels=D, n_layers=L)
elif args.model == "resgcn":
    m = ResGCNNet(hidden_channels=D, n_layers=L)
else:
    m = GATTrimapNet(hidden_channels=D, n_layers=L, n_heads=args.heads)
m = m.to("cuda").eval()
for _ in range(2): m.predict_probs_device(batch)
torch.cuda.synchronize(); t = time.perf_counter()
for _ in range(args.iters): m.predict_probs_device(batch)
torch.cuda.synchronize(); dt = (time.perf_counter() - t) / args.iters
n, e = batch.x.size(0), batch.edge_index.size(1)
msg = f"{type(m).__name__}(D={D}, n={L}) batch {B}: {n} nodes, {e} edges: {dt*1e3:.2f} ms per forward = {B/dt:.0f} graphs/s"
if args.model == "gcn":
    flop = L * (2 * n * D * D + 2 * e * D * D) + 2 * n * D * D * 7
    msg += f", {flop/dt/1e12:.1f} TFLOP/s on the products (edge MLP dominates: {L*2*e*D*D/1e9:.0f} GFLOP)"
print(msg)
