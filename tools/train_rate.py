"""
Training throughput of ResGCNNet on one MI355X: graphs/s per optimizer step and library launches per step.

    python3 tools/train_rate.py [--steps 20] [--warmup 3] [--batches 8 64] [--nodes 600] [--hidden 128]

Batches of superpixel-like graphs of about `--nodes` nodes (tests/helpers.py's generator), D=`--hidden`, 6 layers, TrimapLoss,
AdamW, dropout 0.15.  A step is zero_grad + training forward + backward + clip + optimizer step, timed with CUDA events
over `--steps` steps after `--warmup`.  Launches per step are the ggc_train_* scopes counted by ggc_profile_query in one
extra profiled step.  Prints one JSON line per batch size.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "src", ROOT / "tests"):
    sys.path.insert(0, str(p))

SCOPES = ("train_prepare", "train_gcn_forward", "train_gcn_backward", "train_sage_mean", "train_edge_mean",
          "train_graph_pool")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--nodes", type=int, default=600)
    ap.add_argument("--hidden", type=int, default=128)
    args = ap.parse_args()
    import torch
    from helpers import superpixel_like_graph
    from gcn_grabcut import _native
    from gcn_grabcut.data import Batch, Data
    from gcn_grabcut.losses import TrimapLoss
    from gcn_grabcut.model import ResGCNNet

    torch.manual_seed(0)
    model = ResGCNNet(hidden_channels=args.hidden, n_layers=6).cuda().train()
    opt = torch.optim.AdamW(model.param_groups(1e-3), lr=1e-3)
    crit = TrimapLoss(weight=torch.tensor([1.5, 0.8, 1.5], device="cuda"))
    ctx = _native.get_context(0)
    for bs in args.batches:
        graphs = []
        for i in range(bs):
            x, ei, ea = superpixel_like_graph(n=args.nodes - 10 + (i * 7) % 21, seed=i)
            n = x.shape[0]
            g = torch.Generator().manual_seed(i)
            graphs.append(Data(x=torch.as_tensor(x), edge_index=torch.as_tensor(ei), edge_attr=torch.as_tensor(ea),
                               y=torch.randint(0, 3, (n,), generator=g), node_area=torch.rand(n, generator=g) + 0.01,
                               fg_ratio=torch.rand(n, generator=g)))
        b = Batch.from_data_list(graphs).to("cuda")

        def step():
            opt.zero_grad(set_to_none=True)
            loss = crit(model(b), b.y, area=b.node_area, fg_ratio=b.fg_ratio, batch=b.batch)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            opt.step()

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.steps):
            step()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.steps
        ctx.profile_enable(1)
        step()
        per_scope = {s: ctx.profile_query(s) for s in SCOPES}
        ctx.profile_enable(0)
        print(json.dumps({"hidden": args.hidden, "batch_graphs": bs, "nodes": int(b.x.size(0)), "edges": int(b.edge_index.size(1)),
                          "ms_per_step": round(ms, 3), "graphs_per_s": round(bs * 1000.0 / ms, 1),
                          "ggc_entries_per_step": sum(n for n, _ in per_scope.values()),
                          "ggc_ms_per_step": round(sum(t for _, t in per_scope.values()), 3),
                          "per_scope": {k: [n, round(t, 3)] for k, (n, t) in per_scope.items()}}), flush=True)


if __name__ == "__main__":
    main()
