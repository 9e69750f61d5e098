#!/usr/bin/env python3
"""
bench.py — throughput of the GCN-GrabCut hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W        (N > 1: launched by torch.distributed.run)

A "step" is one pass of the hot path over one per-GPU batch of synthetic
DUTS-shaped images that are already resident in HBM:

    --workload full  (default)  configs[2]: SLIC -> graph -> ResGCNNet -> guided-filter
                                trimap -> GrabCut -> clean-up, batch 256 of 400x300 per GPU
    --workload gcn              configs[1]: ResGCNNet forward only on 64 pre-built graphs

Rank 0 prints ONE JSON line: BASELINE.json's metric (images/s; inputs resident in HBM when the clock starts), the
roofline of the kernel the north star grades (the GCNConv scatter-gather, timed with HIP events on its launch stream
inside the timed region), the whole path against the HBM roofline (`pipeline_roofline`: SURVEY section 8(d)'s
algorithmic bytes per image over the step time) with a per-stage table, the rate with the host->device copy of the
batch inside the clock (`h2d_inclusive`, informational), parity against the CPU oracle on a sample, and the oracle
timed on the host cores: one thread per stage group, and all cores with one worker process per image.
Weights are a seeded random init (the reference ships no checkpoint).  Images shard across ranks with no data-path
collective; RCCL only gathers one 64-byte record per rank after the timed region (gcn_grabcut/distributed.py).
`python bench.py --gpus N` without a launcher starts its own N ranks (torch.distributed.run) before touching a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
for _p in (ROOT, ROOT / "src"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)
HIDDEN, LAYERS = 128, 6    # ResGCNNet default (reference model.py:453-454)
H, W, N_SEGMENTS = 300, 400, 600


def synthetic_region_graph(n: int, rng: np.random.Generator, k_nl: int = 4):
    """Region graph of DUTS shape without running SLIC (for --workload gcn): jittered grid of
    n regions, 4-neighbour adjacency + most diagonals, k non-local colour neighbours per node,
    mirrored as in reference graph_builder.py:303-306.  n = 600 -> E ~ 6.4k directed edges."""
    gw = int(round(np.sqrt(n * 4 / 3)))
    gh = int(np.ceil(n / gw))
    ids = np.arange(gh * gw).reshape(gh, gw)
    lo, hi = [], []
    for a, b, p in ((ids[:, :-1], ids[:, 1:], 1.0), (ids[:-1, :], ids[1:, :], 1.0),
                    (ids[:-1, :-1], ids[1:, 1:], 0.9)):
        ok = (a < n) & (b < n) & (rng.random(a.shape) < p)
        lo.append(np.minimum(a[ok], b[ok])); hi.append(np.maximum(a[ok], b[ok]))
    lo, hi = np.concatenate(lo), np.concatenate(hi)
    adj = np.unique(lo.astype(np.int64) * n + hi)
    col = rng.random((n, 3), dtype=np.float32)
    d = np.linalg.norm(col[:, None] - col[None], axis=2)
    np.fill_diagonal(d, np.inf)
    d[adj // n, adj % n] = np.inf
    d[adj % n, adj // n] = np.inf
    nb = np.argpartition(d, k_nl - 1, axis=1)[:, :k_nl]
    rows = np.repeat(np.arange(n), k_nl)
    nl = np.unique(np.minimum(rows, nb.ravel()).astype(np.int64) * n + np.maximum(rows, nb.ravel()))
    codes = np.concatenate([adj, nl])
    pr = np.stack([codes // n, codes % n], 1)
    src = np.concatenate([pr[:, 0], pr[:, 1]])
    dst = np.concatenate([pr[:, 1], pr[:, 0]])
    attr = rng.random((len(pr), 5), dtype=np.float32)
    attr[: len(adj), 4] = 0.0
    attr[len(adj):, 4] = 1.0
    attr[len(adj):, 2] = 0.0
    x = rng.random((n, 19), dtype=np.float32)
    return x, np.stack([src, dst]), np.concatenate([attr, attr], 0)


def agg_bytes(n_nodes: int, n_edges: int, d: int, n_graphs: int) -> int:
    """Algorithmic HBM bytes of one fused GCNConv aggregation launch:
    read XW, gate, h and write h' (4 N D f32) + CSR col incl. self loops + row_ptr + dis + bias."""
    return (4 * n_nodes * d * 4 + (n_edges + n_nodes) * 4 + (n_nodes + n_graphs) * 4
            + n_nodes * 4 + d * 4)


def path_bytes_per_image(p: int, n: float, e: float, d: int = HIDDEN) -> dict:
    """compulsory HBM bytes per image and stage, inputs / outputs in HBM and perfect reuse on chip
    (P pixels, N regions, E directed edges, D hidden).  ~44 MB at 400x300 / 600 regions."""
    agg = 2 * n * d * 4 + (e + n) * 4 + (n + 1) * 4 + n * 4 + d * 4            # one unfused aggregation pass
    return {
        "colour_prep": 35 * p,                                                 # G0: read 3P, write lab/hsv/gray/grad 32P
        "slic": 16 * p,                                                        # G1: read 12P, write the label map 4P
        "graph": 36 * p + (n * 19 + e * 5) * 4 + e * 16,                       # G2-G8: read seg + lab/hsv/grad, write x / edges
        "gcn": 7 * agg + 11 * 2 * n * d * 4 + e * (5 * 4 + 2 * 64 * 4),        # M1-M7: 7 gathers, ~11 dense N x D passes, edge MLP
        "trimap": 9 * p,                                                       # P0-P2: read gray + seg, write the trimap
        "grabcut": 5 * (16 + 3 + 1) * p + 32 * p,                              # C0-C5: t-links, image, mask per iteration; n-links once
        "cleanup_compose": 9 * p,                                              # K0, O0
    }


def launch_own_ranks(n: int) -> None:
    """`--gpus N` given without a launcher: start N ranks with torch.distributed.run as a CHILD process, before this
    process has touched a GPU (device_count() does not initialise one on this image), and leave with its exit code."""
    import subprocess
    import torch
    have = torch.cuda.device_count()
    if have < n:
        raise SystemExit(f"bench.py --gpus {n}: only {have} GPU(s) visible on this node")
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.call(cmd, env=env))


PMC_SUMMARY = "profiles/r03_pmc_bench_hbm.json"
KERNEL_STATS = "profiles/r03_bench_default_kernel_stats.csv"      # rocprofv3 --kernel-trace --stats of this command (tools/r03_profiles.sh)


def pmc_traffic(workload: str, batch: int):
    """HBM bytes per launch of the graded kernel from the PMC counters.  Counters cannot be read from inside a
    timed run (rocprofv3 --pmc serialises every dispatch), so this is the committed summary of the separate
    FETCH_SIZE / WRITE_SIZE passes over this same command (PMC_SUMMARY, written by tools/pmc_bench.sh; the round-1 file
    as a fallback); null for any other workload or batch size.  -> (bytes, source file)"""
    if workload != "full" or batch != 256:
        return None, None
    for rel in (PMC_SUMMARY, "profiles/r02_pmc_bench_hbm.json", "profiles/r01_pmc_bench_hbm.json"):
        try:
            with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), rel)) as fh:
                summary = json.load(fh)
                return int(summary.get("kernels", summary)["k_aggregate_graph<128, 0, 32, true>"]["hbm_bytes_per_launch"]), rel
        except (OSError, KeyError, ValueError):
            continue
    return None, None


def rocprof_launch_us(workload: str, batch: int):
    """Average duration of the graded kernel in the committed rocprofv3 --kernel-trace --stats summary of this command
    (the judge's clock for `roofline`; the in-run HIP-event figure stands beside it).  -> (microseconds, calls, file) or Nones"""
    if workload != "full" or batch != 256:
        return None, None, None
    import csv
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), KERNEL_STATS), newline="") as fh:
            for row in csv.DictReader(fh):
                if "k_aggregate_graph<128, 0, 32, true>" in row["Name"]:
                    return float(row["AverageNs"]) / 1e3, int(row["Calls"]), KERNEL_STATS
    except (OSError, KeyError, ValueError):
        pass
    return None, None, None


DUMP_SAMPLE, DUMP_SEED, DUMP_MAX_BYTES = 8, 1234, 64 * 1000 * 1000


def dump_outputs(out_dir: str, workload: str, out, batch_size: int) -> dict:
    """--dump-outputs: what a caller of the timed path received from its last step, as DIR/<name>.npy in float32 (float64
    for counts and offsets).  full: probs and the graph offsets of the whole batch; label map, trimap, GrabCut mask, cleaned
    mask, overlay, RGBA and the region graphs of a fixed, seeded sample of DUMP_SAMPLE images (its indices in
    sample_index.npy).  gcn: the probabilities of every node.  The inputs are seeded, so two builds compare file for file."""
    import torch
    arrays = {}
    if workload == "full":
        pick = np.sort(np.random.default_rng(DUMP_SEED).choice(batch_size, min(DUMP_SAMPLE, batch_size), replace=False))
        idx = torch.from_numpy(pick).to(out["segments"].device)
        for name in ("segments", "trimap", "gc_mask", "binary_mask", "overlay", "rgba"):
            arrays[name] = out[name].index_select(0, idx).cpu().numpy().astype(np.float32)
        arrays["probs"] = out["probs"].cpu().numpy().astype(np.float32)
        g = out["graphs"]
        node_ptr, edge_ptr = g.node_ptr_host.astype(np.int64), g.edge_ptr_host.astype(np.int64)
        arrays["graph_node_ptr"], arrays["graph_edge_ptr"] = node_ptr.astype(np.float64), edge_ptr.astype(np.float64)
        nodes = np.concatenate([np.arange(node_ptr[i], node_ptr[i + 1]) for i in pick])
        edges = np.concatenate([np.arange(edge_ptr[i], edge_ptr[i + 1]) for i in pick])
        src, dst = g.edge_src.cpu().numpy().astype(np.int64)[edges], g.edge_dst.cpu().numpy().astype(np.int64)[edges]
        first = np.repeat(node_ptr[pick], edge_ptr[pick + 1] - edge_ptr[pick])      # edge ids local to their image
        arrays["graph_edge_index"] = np.stack([src - first, dst - first]).astype(np.float32)
        for name in ("x", "centroids", "area_ratio"):
            arrays[f"graph_{name}"] = getattr(g, name).cpu().numpy()[nodes].astype(np.float32)
        arrays["graph_edge_attr"] = g.edge_attr.reshape(g.edge_src.numel(), -1).cpu().numpy()[edges].astype(np.float32)
        arrays["sample_index"] = pick.astype(np.float32)
    else:
        arrays["probs"] = out.cpu().numpy().astype(np.float32)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_MAX_BYTES}-byte budget")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
    return {"dir": out_dir, "files": sorted(f"{k}.npy" for k in arrays), "bytes": int(total)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=["full", "gcn"], default="full")
    ap.add_argument("--lanes", type=int, default=0, help="concurrent sub-batches of the GrabCut stage (full workload; "
                    "default 4 with one pipeline, 1 per pipeline otherwise)")
    ap.add_argument("--overlap-pass", type=int, default=-1, help="after the contract's run (N=1, full workload, one pipeline): a second "
                    "timed pass of the same steps over this many overlapping pipelines, reported as 'overlapped' (informational, "
                    "never `value`).  0 = skip; -1 (default) = 3, except under rocprofv3, where the pass is skipped: it re-runs "
                    "every kernel under contention, which would blur the profiler's per-kernel summary of the command")
    ap.add_argument("--pipelines", type=int, default=1, help="full workload: pipelines (private contexts, own HIP streams and "
                    "host threads) that take the timed steps in turn, so consecutive batches overlap")
    ap.add_argument("--batch", type=int, default=0, help="images per GPU per step (default 256 full / 64 gcn)")
    ap.add_argument("--cpu-sample", type=int, default=16, help="images run through the CPU oracle on ONE thread (per-stage times, "
                    "parity sample; ~6 s of one core; 0 = no CPU leg at all)")
    ap.add_argument("--cpu-all", type=int, default=256, help="images of the all-cores CPU leg, one worker process per image (0 = skip)")
    ap.add_argument("--cpu-workers", type=int, default=0, help="worker processes of the all-cores leg (default: the cores this "
                    "process may use, at most 16 = one GPU's share of the host)")
    ap.add_argument("--h2d-steps", type=int, default=3, help="extra timed steps that include the host->device copy of the batch (0 = skip)")
    ap.add_argument("--force-collective", action="store_true", help="initialise the RCCL process group, the barriers, the MAX "
                    "all-reduce of the step time and the gather of the per-rank records even when WORLD_SIZE is 1 (warms the "
                    "N > 1 path on a one-GPU box; under torch.distributed.run --nproc-per-node 1 or on its own)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed to "
                    "DIR/<name>.npy (float32 / float64; per-pixel outputs of a fixed, seeded sample of images, at most 64 MB)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.overlap_pass < 0:
        profiled = any(k in os.environ for k in ("ROCP_TOOL_LIBRARIES", "ROCPROF_OUTPUT_PATH", "ROCPROFILER_LIBRARY_CTOR"))
        args.overlap_pass = 0 if profiled else 3
    batch_size = args.batch or (256 if args.workload == "full" else 64)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        launch_own_ranks(args.gpus)

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    collective = world > 1 or args.force_collective          # everything below that talks to other ranks hangs off this
    if collective:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:                  # --force-collective without a launcher: a job of one rank
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)   # RCCL over xGMI; gathers timings only

    from gcn_grabcut import _native
    from gcn_grabcut.data import Batch, Data
    from gcn_grabcut.graph_builder import SuperpixelGraphConfig
    from gcn_grabcut.model import ResGCNNet
    from gcn_grabcut.pipeline import GCNGrabCutPipeline
    from gcn_grabcut.synthetic import synthetic_batch

    # ---- model: seeded random init (reference model.py:501-506); no checkpoint ships
    torch.manual_seed(0)
    model = ResGCNNet(hidden_channels=HIDDEN, n_layers=LAYERS).to(dev).eval()
    ctx = _native.get_context(local_rank)

    host_imgs = host_graphs = None
    if args.workload == "full":
        # this rank's shard of the job's world * B images of config 3 (seeds 30000 + index): the contiguous block the
        # product's sharding rule gives it (gcn_grabcut/distributed.py, the rule tests/test_distributed_cpu.py checks)
        from gcn_grabcut.distributed import shard_range
        shard = shard_range(batch_size * world, rank, world)
        assert len(shard) == batch_size
        host_imgs = synthetic_batch(batch_size, H, W, config_id=3, first_index=shard.start)
        n_pipes = max(1, args.pipelines)
        lanes = args.lanes if args.lanes > 0 else (4 if n_pipes == 1 else 1)
        pipe = GCNGrabCutPipeline(model, sp_config=SuperpixelGraphConfig(n_segments=N_SEGMENTS), device=f"cuda:{local_rank}",
                                  grabcut_lanes=lanes)
        pipes = [pipe] + [pipe.replica(grabcut_lanes=lanes) for _ in range(n_pipes - 1)]
        streams = [torch.cuda.Stream(dev) for _ in range(n_pipes)] if n_pipes > 1 else None
        bgr = torch.from_numpy(host_imgs).to(dev)
        last = {}

        def step():
            last["out"] = pipe.segment_batch_device(bgr, compose=True)

        def run_steps(n):
            """n passes over the batch; with several pipelines, pipeline i takes steps i, i + P, ... on its own stream"""
            if n_pipes == 1:
                for _ in range(n):
                    step()
                return
            import threading

            errors = []

            def worker(i):
                try:
                    torch.cuda.set_device(dev)
                    with torch.cuda.stream(streams[i]):
                        for s in range(i, n, n_pipes):
                            out = pipes[i].segment_batch_device(bgr, compose=True)
                            if s == n - 1:
                                last["out"] = out
                    streams[i].synchronize()
                except Exception as exc:                   # re-raised below: a timing over work that never ran is worthless
                    errors.append(exc)

            threads = [threading.Thread(target=worker, args=(i,), name=f"ggc-pipe{i}") for i in range(n_pipes)]
            for th in threads:
                th.start()
            for th in threads:
                th.join()
            if errors:
                raise errors[0]
    else:
        rng = np.random.default_rng(20_000 + rank)
        host_graphs = [synthetic_region_graph(int(rng.integers(585, 618)), rng) for _ in range(batch_size)]
        batch = Batch.from_data_list([Data(x=torch.from_numpy(x), edge_index=torch.from_numpy(ei),
                                           edge_attr=torch.from_numpy(ea)) for x, ei, ea in host_graphs]).to(dev)
        batch.node_ptr32 = batch.ptr.to(torch.int32)
        last = {}

        n_pipes, lanes = 1, 0

        def step():
            last["out"] = model.predict_probs_device(batch)

        def run_steps(n):
            for _ in range(n):
                step()

    def sync_all():
        torch.cuda.synchronize(dev)
        if collective:
            dist.barrier()
        torch.cuda.synchronize(dev)

    warmup = max(args.warmup, n_pipes) if n_pipes > 1 else args.warmup     # every pipeline allocates its arena once
    run_steps(warmup)
    # the GrabCut stage runs on concurrent lanes with private contexts (created during warm-up): profile them all
    ctxs = [c for p_ in pipes for c in p_._eng.all_contexts()] if args.workload == "full" else [ctx]
    # The timed region brackets ONLY the graded kernel with HIP events (an event pair idles its stream for ~10 us, and a step
    # has several hundred instrumented scopes); the per-stage table comes from ONE extra, untimed step with every scope on.
    for c in ctxs:
        c.profile_enable(2)
    sync_all()
    t0 = time.perf_counter()
    run_steps(args.steps)
    sync_all()
    elapsed = time.perf_counter() - t0
    dumped = None
    if args.dump_outputs and rank == 0:       # before any later step reuses the buffers the outputs live in
        dumped = dump_outputs(args.dump_outputs, args.workload, last["out"], batch_size)
    stage_keys = ("gcn_gemm", "slic_assign", "slic_update", "slic_connectivity", "graph_stats", "graph_knn", "graph_prior",
                  "refine_trimap", "grabcut_init_gmm", "grabcut_gmm", "maxflow_relabel", "maxflow_push")
    q = [c.profile_query("gcn_aggregate") for c in ctxs]
    prof = {"gcn_aggregate": (sum(v[0] for v in q), sum(v[1] for v in q))}
    for c in ctxs:
        c.profile_enable(True)
    run_steps(1)
    sync_all()
    for k in stage_keys:
        q = [c.profile_query(k) for c in ctxs]       # (launch scopes, ms); lanes overlap, so stage times can exceed the step
        prof[k] = (sum(v[0] for v in q), sum(v[1] for v in q))
    for c in ctxs:
        c.profile_enable(False)

    elapsed_rank = elapsed
    if collective:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # ---- informational: the same steps with the host->device copy of the batch inside the clock (SURVEY 8(d) "end-to-end")
    h2d = None
    if args.workload == "full" and args.h2d_steps > 0 and n_pipes == 1:
        pinned = torch.from_numpy(host_imgs).pin_memory()
        sync_all()
        t1 = time.perf_counter()
        for _ in range(args.h2d_steps):
            last["out"] = pipe.segment_batch_device(pinned.to(dev, non_blocking=True), compose=True)
        sync_all()
        e1 = time.perf_counter() - t1
        if collective:
            t = torch.tensor([e1], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            e1 = float(t.item())
        h2d = {"value": round(batch_size * world * args.h2d_steps / e1, 2), "unit": "images/s", "steps": args.h2d_steps,
               "ms_per_step": round(e1 / args.h2d_steps * 1e3, 3), "bytes_per_step_per_gpu": int(host_imgs.nbytes),
               "note": "pinned host batch copied to the device inside the timed region, then the same step"}

    # ---- informational second pass: consecutive batches overlapped (batch k+1's SLIC / graph / GCN under batch k's GrabCut).
    # Not the contract's number: per-kernel event timing is meaningless under overlap, so `value` and `roofline` stay serial.
    overlapped = None
    if world == 1 and args.workload == "full" and n_pipes == 1 and args.overlap_pass > 1:
        try:
            serial_out = last["out"]
            serial_mask = serial_out["binary_mask"].clone()
            n_pipes, keep_lanes = args.overlap_pass, pipe.grabcut_lanes
            pipe.grabcut_lanes = 1
            pipes = [pipe] + [pipe.replica(grabcut_lanes=1) for _ in range(n_pipes - 1)]
            streams = [torch.cuda.Stream(dev) for _ in range(n_pipes)]
            k2 = -(-args.steps // n_pipes) * n_pipes
            run_steps(n_pipes)                       # each replica allocates its arena
            sync_all()
            t1 = time.perf_counter()
            run_steps(k2)
            sync_all()
            e2 = time.perf_counter() - t1
            overlapped = {"pipelines": n_pipes, "grabcut_lanes": 1, "steps": k2, "value": round(batch_size * k2 / e2, 2),
                          "unit": "images/s", "ms_per_step": round(e2 / k2 * 1e3, 3),
                          "masks_identical_to_serial_run": bool(torch.equal(last["out"]["binary_mask"], serial_mask))}
            pipe.grabcut_lanes, n_pipes = keep_lanes, 1
            last["out"] = serial_out
        except Exception as exc:                     # never lose the contract's line over the extra pass
            overlapped = {"error": f"{type(exc).__name__}: {exc}"}
            n_pipes = 1

    images = batch_size * world * args.steps
    value = images / elapsed

    # ---- CPU oracle legs (checker and reported baseline; never part of the timed region)
    from gcn_grabcut.distributed import RankRecord, gather_records, summarise
    rec = RankRecord(n_images=batch_size * args.steps, seconds=elapsed_rank)
    cpu = parity = None
    if args.cpu_sample > 0:
        from oracle import oracle as orc               # checker / CPU baseline only
        sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
        # every rank checks a few images of ITS shard (the gathered record carries the tallies); rank 0 of a single-GPU
        # run checks the full sample and times it
        n_s = min(args.cpu_sample if world == 1 else 2, batch_size)
        if args.workload == "full":
            out = last["out"]
            g = out["graphs"]
            seg_g, tri_g = out["segments"][:n_s].cpu().numpy(), out["trimap"][:n_s].cpu().numpy()
            bin_g, probs_g = out["binary_mask"][:n_s].cpu().numpy(), out["probs"].cpu().numpy()
            stage_s = {"graph_build": 0.0, "gcn_inference": 0.0, "grabcut": 0.0, "postprocess": 0.0}
            t1 = time.perf_counter()
            ref = []
            for i in range(n_s):
                tm = {}
                ref.append(orc.segment(host_imgs[i], sd, HIDDEN, LAYERS, n_segments=N_SEGMENTS, seed=i, timing=tm))
                for k in stage_s:
                    stage_s[k] += tm[k]
            dt = time.perf_counter() - t1
            ious, dl, ei_ok = [], 0.0, []
            esrc, edst = g.edge_src.cpu().numpy().astype(np.int64), g.edge_dst.cpu().numpy().astype(np.int64)
            for i, r in enumerate(ref):
                n0, n1 = int(g.node_ptr_host[i]), int(g.node_ptr_host[i + 1])
                e0, e1 = int(g.edge_ptr_host[i]), int(g.edge_ptr_host[i + 1])
                ei_ok.append(np.array_equal(np.stack([esrc[e0:e1], edst[e0:e1]]) - n0, r["graph"]["edge_index"]))
                if n1 - n0 == r["probs"].shape[0]:
                    dl = max(dl, float(np.abs(probs_g[n0:n1] - r["probs"]).max()))
                ious.append(orc.iou(bin_g[i], r["binary_mask"]) if r["binary_mask"].any() or bin_g[i].any() else 1.0)
            lab_ok = [np.array_equal(seg_g[i], ref[i]["segments"]) for i in range(n_s)]
            tri_ok = [np.array_equal(tri_g[i], ref[i]["trimap"]) for i in range(n_s)]
            msk_ok = [np.array_equal(bin_g[i], ref[i]["binary_mask"]) for i in range(n_s)]
            rec.sum_iou, rec.n_iou, rec.n_checked = float(np.sum(ious)), n_s, n_s
            rec.n_label_exact, rec.n_trimap_exact, rec.n_mask_exact = float(np.sum(lab_ok)), float(np.sum(tri_ok)), float(np.sum(msk_ok))
            parity = {
                "sample": n_s,
                "label_map_exact_pct": round(100.0 * float(np.mean(lab_ok)), 2),
                "edge_index_exact_pct": round(100.0 * float(np.mean(ei_ok)), 2),
                "trimap_pixel_match_pct": round(100.0 * float(np.mean([(tri_g[i] == ref[i]["trimap"]).mean() for i in range(n_s)])), 4),
                "trimap_exact_images_pct": round(100.0 * float(np.mean(tri_ok)), 2),
                "mask_exact_pct": round(100.0 * float(np.mean(msk_ok)), 2),
                "max_abs_dprob": dl, "mean_mask_iou": round(float(np.mean(ious)), 6), "min_mask_iou": round(float(np.min(ious)), 6),
            }
            what = f"{n_s} of the {batch_size} images, full pipeline"
            per_stage = {k: round(v / n_s * 1e3, 2) for k, v in stage_s.items()}
        else:
            probs_g = last["out"].cpu().numpy()
            off = np.cumsum([0] + [x.shape[0] for x, _, _ in host_graphs])
            orc.resgcn_forward(sd, HIDDEN, LAYERS, *host_graphs[0])          # warm
            t1 = time.perf_counter()
            ref = [orc.resgcn_forward(sd, HIDDEN, LAYERS, x, ei, ea) for x, ei, ea in host_graphs[:n_s]]
            dt = time.perf_counter() - t1
            parity = {"sample": n_s, "max_abs_dprob": max(float(np.abs(probs_g[off[i]:off[i + 1]] - ref[i][1]).max())
                                                          for i in range(n_s))}
            what = f"{n_s} of the {batch_size} graphs, GCN forward only"
            per_stage = None
        if rank == 0 and world == 1:                    # the CPU baseline is a rank-0, N=1 leg
            host_cores = len(os.sched_getaffinity(0))
            single = {"value": round(n_s / dt, 3), "unit": "images/s", "cores": 1, "sample": what,
                      "ms_per_image_by_stage": per_stage}
            cpu = {"value": single["value"], "unit": "images/s", "cores": 1, "kind": "port",
                   "sample": f"{what}; C oracle (CPU restatement of the OpenCV + scikit-image + PyG path), 1 thread; host has {host_cores} cores",
                   "single_thread": single, "all_cores": None}
            if args.workload == "full" and args.cpu_all > 0:
                from oracle import cpu_pool
                workers = args.cpu_workers if args.cpu_workers > 0 else min(host_cores, 16)
                n_all = args.cpu_all
                dt_all, res = cpu_pool.run(range(n_all), 0, workers, sd, HIDDEN, LAYERS, N_SEGMENTS, H, W, 3)
                cpu["all_cores"] = {"value": round(n_all / dt_all, 3), "unit": "images/s", "cores": workers,
                                    "sample": f"{n_all} images of the same generator, one worker process per image "
                                              f"(reference dataset.py:496-520 pattern), {workers} processes",
                                    "mean_worker_s_per_image": round(float(np.mean([r["seconds"] for r in res])), 4)}
                # the reported baseline is the better of the two legs; `cores` = the threads it really used
                cpu.update(value=cpu["all_cores"]["value"], cores=workers,
                           sample=f"{n_all} images, full pipeline, C oracle on {workers} worker processes (host has {host_cores} cores); "
                                  f"single thread: {single['value']} images/s")
    records = gather_records(rec, dev if collective else None)      # the path's only collective: 64 bytes per rank

    if rank == 0:
        if args.workload == "full":
            g = last["out"]["graphs"]
            n_nodes, n_edges = int(g.node_ptr_host[-1]), int(g.edge_ptr_host[-1])
        else:
            n_nodes, n_edges = batch.x.size(0), batch.edge_index.size(1)
        launches, agg_ms = prof["gcn_aggregate"]
        agg_avg_s = agg_ms / 1e3 / max(launches, 1)
        b_launch = agg_bytes(n_nodes, n_edges, HIDDEN, batch_size)
        achieved = b_launch / agg_avg_s / 1e9 if launches else 0.0
        traffic, traffic_src = pmc_traffic(args.workload, batch_size)
        roofline = {
            "kernel": "k_aggregate_graph<128,0,32,gated> (GCNConv scatter-gather, graph slice resident in LDS, fused gate/GELU/residual epilogue)",
            "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
            "traffic_source": (f"{traffic_src}: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this command, not this run"
                               if traffic_src else None),
            "bytes_per_launch": b_launch, "avg_launch_us": round(agg_avg_s * 1e6, 2), "launches": launches,
            "clock": "HIP events on the launch stream inside the timed region, minus the calibrated empty-pair offset",
            "event_pair_overhead_us": round(ctx.profile_query("#event_pair_overhead")[1] * 1e3, 2),
            # informational: bytes of all gathered neighbour rows per second; they are served from LDS
            "effective_gather_gbs": round((n_edges + n_nodes) * HIDDEN * 4 / agg_avg_s / 1e9, 1) if launches else 0.0,
        }
        rp_us, rp_calls, rp_src = rocprof_launch_us(args.workload, batch_size)
        if rp_us:       # the same kernel under rocprofv3 (committed summary of this command, not this run)
            roofline.update(rocprof_avg_launch_us=round(rp_us, 2), rocprof_calls=rp_calls,
                            rocprof_frac=round(b_launch / (rp_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4), rocprof_source=rp_src)
        stage_ms = {k: round(v[1] / (args.steps if k == "gcn_aggregate" else 1), 3) for k, v in prof.items() if v[0]}
        pipeline_roofline = stage_table = trimap_hist = None
        if args.workload == "full":
            # ---- the whole path against the HBM roofline (north star: "as fraction of the HBM roofline")
            per_img = path_bytes_per_image(H * W, n_nodes / batch_size, n_edges / batch_size)
            total_b = sum(per_img.values())
            step_s = elapsed / args.steps
            pipeline_roofline = {
                "bound": "hbm", "algorithmic_mb_per_image": round(total_b / 1e6, 2),
                "by_stage_mb_per_image": {k: round(v / 1e6, 3) for k, v in per_img.items()},
                "achieved": round(total_b * batch_size / step_s / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(total_b * batch_size / step_s / 1e9 / HBM_PEAK_GBS, 5),
                "note": "SURVEY 8(d) compulsory bytes per image x images per step / step time; max-flow sweeps are data dependent and not in the model",
            }
            # ---- per stage: launch-stream event time per step, the byte model where SURVEY 8(d) gives one, achieved GB/s
            p_ = H * W * batch_size
            model_b = {"gcn_aggregate": b_launch * launches / args.steps if launches else None,
                       "slic_assign": 10 * 16 * p_, "slic_update": 10 * 16 * p_, "slic_connectivity": 8 * p_,
                       "graph_stats": 36 * p_, "refine_trimap": 9 * p_, "grabcut_gmm": 5 * 20 * p_,
                       "grabcut_init_gmm": 11 * 4 * p_, "maxflow_relabel": None, "maxflow_push": None,
                       "graph_knn": None, "graph_prior": None, "gcn_gemm": None}
            stage_table = {}
            for k, ms in stage_ms.items():
                bts = model_b.get(k)
                stage_table[k] = {"ms_per_step": ms, "model_mb_per_step": round(bts / 1e6, 1) if bts else None,
                                  "achieved_gbs": round(bts / (ms / 1e3) / 1e9, 1) if bts and ms > 0 else None}
            gflop = 2.0 * n_nodes * HIDDEN * HIDDEN * LAYERS / 1e9
            if "gcn_gemm" in stage_table and stage_ms["gcn_gemm"] > 0:
                stage_table["gcn_gemm"]["achieved_tflops_f32"] = round(gflop / stage_ms["gcn_gemm"], 1)
            tri = last["out"]["trimap"]
            hist = torch.bincount(tri.reshape(-1).to(torch.int64), minlength=4).cpu().numpy()
            trimap_hist = {name: round(float(hist[i]) / float(hist.sum()), 4)
                           for i, name in enumerate(("definite_bg", "definite_fg", "probable_bg", "probable_fg"))}
        job = summarise(records)
        if world > 1 and job["checked_images"]:
            parity = {"sample": job["checked_images"], "label_map_exact_pct": job["label_map_exact_pct"],
                      "trimap_exact_images_pct": job["trimap_exact_pct"], "mask_exact_pct": job["mask_exact_pct"],
                      "mean_mask_iou": job["mean_mask_iou"], "note": "tallies gathered from every rank's record"}

        cfg_name = ("configs[2]: full pipeline (SLIC->graph->ResGCNNet->guided-filter trimap->GrabCut 5 it->clean-up), "
                    f"batch {batch_size} of {W}x{H}, n_segments={N_SEGMENTS}") if args.workload == "full" else \
                   (f"configs[1]: batch {batch_size} DUTS-shape region graphs (~600 superpixels), "
                    "ResGCNNet(D=128,n=6) forward only")
        out_json = {
            "metric": "images/sec end-to-end mask (DUTS-shape batch)", "value": round(value, 2),
            "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": cfg_name, "images_per_gpu": batch_size, "nodes": n_nodes,
                       "directed_edges": n_edges, "weights": "seeded random init (torch.manual_seed(0))",
                       "pipelines": n_pipes, "grabcut_lanes": lanes,
                       "inputs": "uint8 batch resident in HBM when the clock starts (h2d_inclusive has the copy inside)"},
            "roofline": roofline, "pipeline_roofline": pipeline_roofline, "cpu_baseline": cpu, "parity_vs_cpu_oracle": parity,
            "stage_ms_per_step": stage_ms, "stages": stage_table, "trimap_label_fractions": trimap_hist,
            "h2d_inclusive": h2d, "ranks": job["per_rank"] if collective else None, "overlapped": overlapped,
            "dumped_outputs": dumped,
        }
        print(json.dumps(out_json), flush=True)
    if collective:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
