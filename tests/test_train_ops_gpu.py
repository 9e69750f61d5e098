"""GPU: the ggc_train_* graph operators (forward and backward, through their autograd Functions) against a float64
CPU torch restatement built from tests/torch_ref.py, on graphs with isolated nodes, a hub of 510 in-edges, duplicate
edges, explicit i->i edges, directed edges, a one-node graph and an edgeless graph, at every training width.
Tolerance: max |err| <= 1e-5 (1 + |ref|) elementwise.  Two runs must give identical bits."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import torch_ref
from helpers import float64_default

pytestmark = pytest.mark.gpu


def _batch_graph(seed=0):
    """Four graphs, concatenated: random directed (duplicates, self loops, isolated nodes), hub, one node, edgeless."""
    rng = np.random.default_rng(seed)
    parts, sizes, off = [], [], 0
    n = 60                                                  # random directed; nodes 50..59 isolated
    src, dst = rng.integers(0, 50, 300), rng.integers(0, 50, 300)
    src = np.concatenate([src, src[:20], np.arange(0, 50, 7)])      # 20 duplicate edges, explicit i->i edges
    dst = np.concatenate([dst, dst[:20], np.arange(0, 50, 7)])
    parts.append(np.stack([src, dst]) + off); sizes.append(n); off += n
    n = 520                                                 # hub: node 0 has 510 in-edges (some repeated)
    hs = rng.integers(1, n, 510)
    rs, rd = rng.integers(0, n, 400), rng.integers(0, n, 400)
    parts.append(np.stack([np.concatenate([hs, rs]), np.concatenate([np.zeros(510, np.int64), rd])]) + off)
    sizes.append(n); off += n
    sizes.append(1); off += 1                               # one-node graph
    sizes.append(4); off += 4                               # edgeless graph
    ei = np.concatenate(parts, 1)
    node_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return torch.from_numpy(ei.astype(np.int64)), off, torch.from_numpy(node_ptr)


def _close(got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double()
    assert got.shape == ref.shape
    err = (got - ref).abs()
    bad = err > 1e-5 * (1 + ref.abs())
    assert not bad.any(), f"max err {err.max().item():.3e} at {bad.nonzero()[:3].tolist()}"


def _prep(ei, n, node_ptr):
    from gcn_grabcut import _native
    from gcn_grabcut.train_ops import GraphPrep
    return GraphPrep(_native.get_context(0), ei.cuda(), n, node_ptr.cuda())


def _inputs(n, e, d, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(xw=r(n, d), bias=r(d), gate=torch.sigmoid(r(n, d)), h=r(n, d), g=r(n, d), enc=r(e, max(d // 2, 8)),
                g_ctx=r(n, max(d // 2, 8)), score=r(n, 1) * 2)


def _run_gpu(ei, n, node_ptr, t):
    """all operators forward + backward on the GPU; returns a dict of float32 host results"""
    from gcn_grabcut import train_ops
    prep = _prep(ei, n, node_ptr)
    c = {k: v.float().cuda().requires_grad_(k not in ("g", "g_ctx")) for k, v in t.items()}
    out = {}
    y = train_ops.gcn_conv_gated(c["xw"], c["bias"], c["gate"], c["h"], prep)
    y.backward(c["g"])
    out.update(gcn_y=y, gcn_g_xw=c["xw"].grad, gcn_g_bias=c["bias"].grad, gcn_g_gate=c["gate"].grad, gcn_g_h=c["h"].grad)
    x = c["h"].detach().clone().requires_grad_(True)
    y2 = train_ops.gcn_conv_gated(c["xw"].detach(), c["bias"].detach(), c["gate"].detach(), None, prep)
    out["gcn_y_nores"] = y2
    m = train_ops.sage_mean(x, prep)
    m.backward(c["g"])
    out.update(sage_m=m, sage_g_x=x.grad)
    enc = c["enc"]
    ctx = train_ops.edge_mean(enc, prep)
    ctx.backward(c["g_ctx"])
    out.update(edge_ctx=ctx, edge_g_enc=enc.grad)
    hh = c["h"].detach().clone().requires_grad_(True)
    hb = train_ops.graph_pool(hh, c["score"], prep)
    hb.backward(c["g"])
    out.update(pool_hb=hb, pool_g_h=hh.grad, pool_g_score=c["score"].grad)
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}


def _run_ref(ei, n, node_ptr, t):
    d = t["xw"].size(1)
    c = {k: v.clone().requires_grad_(k not in ("g", "g_ctx")) for k, v in t.items()}
    out = {}
    o = torch_ref.gcn_conv(c["xw"], ei, torch.eye(d, dtype=torch.float64), c["bias"])
    y = c["h"] + F.gelu(o * c["gate"])
    y.backward(c["g"])
    out.update(gcn_y=y, gcn_g_xw=c["xw"].grad, gcn_g_bias=c["bias"].grad, gcn_g_gate=c["gate"].grad, gcn_g_h=c["h"].grad)
    out["gcn_y_nores"] = y - c["h"]
    x = t["h"].clone().requires_grad_(True)
    m = torch_ref.scatter_mean(x[ei[0]], ei[1], n)
    m.backward(t["g"])
    out.update(sage_m=m, sage_g_x=x.grad)
    ctx = torch_ref.scatter_mean(c["enc"], ei[1], n)
    ctx.backward(t["g_ctx"])
    out.update(edge_ctx=ctx, edge_g_enc=c["enc"].grad)
    batch = torch.repeat_interleave(torch.arange(node_ptr.numel() - 1), (node_ptr[1:] - node_ptr[:-1]).long())
    hh = t["h"].clone().requires_grad_(True)
    with float64_default():
        a = torch_ref.graph_softmax(c["score"], batch)
    g = torch.zeros(node_ptr.numel() - 1, d, dtype=torch.float64).index_add(0, batch, a * hh)[batch]
    g.backward(t["g"])
    out.update(pool_hb=g, pool_g_h=hh.grad, pool_g_score=c["score"].grad)
    return out


@pytest.mark.parametrize("d", [32, 64, 96, 128])
def test_operators_match_float64_reference(gpu_ctx, d):
    ei, n, node_ptr = _batch_graph(seed=d)
    t = _inputs(n, ei.size(1), d, seed=d)
    got, want = _run_gpu(ei, n, node_ptr, t), _run_ref(ei, n, node_ptr, t)
    for k in want:
        try:
            _close(got[k], want[k])
        except AssertionError as e:
            raise AssertionError(f"{k} (D={d}): {e}") from None


def test_single_graph_without_node_ptr_and_edgeless_batch(gpu_ctx):
    """no node_ptr: the whole batch is one graph; E = 0 works for every operator"""
    from gcn_grabcut import _native, train_ops
    for ei, n in ((torch.tensor([[0, 1, 2, 2], [1, 2, 0, 2]]), 3), (torch.zeros(2, 0, dtype=torch.long), 5)):
        prep = train_ops.GraphPrep(_native.get_context(0), ei.cuda(), n)
        t = _inputs(n, ei.size(1), 32, seed=n)
        got = _run_gpu(ei, n, torch.tensor([0, n], dtype=torch.int32), t)
        want = _run_ref(ei, n, torch.tensor([0, n], dtype=torch.int32), t)
        for k in want:
            _close(got[k], want[k])
        assert prep.n_graphs == 1


def test_two_runs_are_bit_identical(gpu_ctx):
    ei, n, node_ptr = _batch_graph(seed=7)
    t = _inputs(n, ei.size(1), 128, seed=7)
    a, b = _run_gpu(ei, n, node_ptr, t), _run_gpu(ei, n, node_ptr, t)
    for k in a:
        assert np.array_equal(a[k].numpy(), b[k].numpy()), k


def test_unsupported_width_and_bad_edges_raise(gpu_ctx):
    from gcn_grabcut import train_ops
    ei, n, node_ptr = _batch_graph(seed=1)
    prep = _prep(ei, n, node_ptr)
    x = torch.randn(n, 48, device="cuda")
    with pytest.raises(ValueError):
        train_ops.sage_mean(x, prep)
    with pytest.raises(ValueError):
        _prep(torch.tensor([[0, 5], [1, 0]]), 3, torch.tensor([0, 3], dtype=torch.int32))
