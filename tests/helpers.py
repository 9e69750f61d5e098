"""Seeded synthetic inputs shared by the tests (test infrastructure)."""
import contextlib

import numpy as np
import torch


@contextlib.contextmanager
def float64_default():
    """torch_ref's helpers allocate some buffers with the default dtype; a float64 restatement runs under this"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def chain_graph(n=80, seed=None, in_dim=19, edge_dim=5):
    """Chain graph with random features — mirrors reference tests/test.py:257-272."""
    gen = torch.Generator()
    gen.manual_seed(0 if seed is None else seed)
    x = torch.randn(n, in_dim, generator=gen)
    src = torch.arange(n - 1)
    dst = torch.arange(1, n)
    edge_index = torch.stack([torch.cat([src, dst]), torch.cat([dst, src])])
    edge_attr = torch.rand(edge_index.size(1), edge_dim, generator=gen)
    return x, edge_index, edge_attr


def superpixel_like_graph(n=600, k_nl=4, seed=0):
    """Jittered-grid region graph shaped like a DUTS superpixel graph:
    4-neighbour adjacency plus k nearest non-adjacent 'colour' neighbours,
    mirrored exactly like reference graph_builder.py:303-306. N~600 -> E~6.4k."""
    rng = np.random.default_rng(seed)
    gw = int(round(np.sqrt(n * 4 / 3)))
    gh = int(np.ceil(n / gw))
    ids = np.arange(gh * gw).reshape(gh, gw)
    keep = ids < n
    pairs = set()
    for a, b in ((ids[:, :-1], ids[:, 1:]), (ids[:-1, :], ids[1:, :]), (ids[:-1, :-1], ids[1:, 1:])):
        ok = (a < n) & (b < n)
        if a is ids[:-1, :-1]:
            ok &= rng.random(a.shape) < 0.35
        for u, v in zip(a[ok].ravel(), b[ok].ravel()):
            pairs.add((int(min(u, v)), int(max(u, v))))
    adj = sorted(pairs)
    col = rng.random((n, 3)).astype(np.float32)
    d = np.linalg.norm(col[:, None] - col[None], axis=2)
    np.fill_diagonal(d, np.inf)
    for u, v in adj:
        d[u, v] = d[v, u] = np.inf
    nb = np.argsort(d, axis=1, kind="stable")[:, :k_nl]
    nl = sorted({(int(min(i, j)), int(max(i, j))) for i in range(n) for j in nb[i]})
    pr = np.array(adj + nl, dtype=np.int64)
    src = np.concatenate([pr[:, 0], pr[:, 1]])
    dst = np.concatenate([pr[:, 1], pr[:, 0]])
    attr = rng.random((len(pr), 5)).astype(np.float32)
    attr[: len(adj), 4] = 0.0
    attr[len(adj):, 4] = 1.0
    attr[len(adj):, 2] = 0.0
    x = rng.random((n, 19)).astype(np.float32)
    return x, np.stack([src, dst]), np.concatenate([attr, attr], 0)


def seeded_state_dict(hidden=128, n_layers=6, seed=0, perturb=True):
    """Deterministic ResGCNNet weights: the reference init (model.py:501-506)
    under torch.manual_seed(seed), with biases / norms / BN stats / jk logits
    perturbed so that every term of the forward pass is exercised."""
    from gcn_grabcut.model import ResGCNNet
    torch.manual_seed(seed)
    m = ResGCNNet(hidden_channels=hidden, n_layers=n_layers)
    sd = m.state_dict()
    if perturb:
        g = torch.Generator()
        g.manual_seed(seed + 1)
        for k, v in sd.items():
            if not v.dtype.is_floating_point:
                continue
            if k.endswith("running_var"):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
            elif k.endswith("running_mean"):
                v.copy_(0.5 + 0.2 * torch.randn(v.shape, generator=g))
            elif v.dim() == 1:
                v.add_(0.1 * torch.randn(v.shape, generator=g))
        m.load_state_dict(sd)
    return m, {k: v.clone() for k, v in m.state_dict().items()}


# ------------------------------------------------------------------------ graph zoo
# Structures the product's graph builder makes and superpixel_like_graph does not: hubs (flat regions make the kNN step
# pick the same few nodes), nodes without incoming edges, asymmetric and repeated edges, batches of tiny and edgeless
# graphs.  Hub and hole indices sit on the kernels' work boundaries: 32 destinations per wave of the fused edge gate,
# 256 per block.

def _hub_edges(rng, n, hub, k, outgoing=False):
    """k edges j -> hub from distinct random j != hub (hub -> j as well when `outgoing`)"""
    others = np.delete(np.arange(n), hub)
    src = rng.choice(others, size=k, replace=False)
    ei = [np.stack([src, np.full(k, hub)])]
    if outgoing:
        dst = rng.choice(others, size=k, replace=False)
        ei.append(np.stack([np.full(k, hub), dst]))
    ei = np.concatenate(ei, 1).astype(np.int64)
    return ei, rng.random((ei.shape[1], 5)).astype(np.float32)


def _cat_graphs(graphs):
    """[(x, ei, ea)] with local indices -> one batch (x, ei, ea, sizes); edges stay grouped by graph"""
    sizes = tuple(int(g[0].shape[0]) for g in graphs)
    off = np.cumsum((0,) + sizes)
    x = np.concatenate([g[0] for g in graphs]).astype(np.float32)
    ei = np.concatenate([np.asarray(g[1], np.int64).reshape(2, -1) + off[i] for i, g in enumerate(graphs)], 1)
    ea = np.concatenate([np.asarray(g[2], np.float32).reshape(-1, 5) for g in graphs])
    return x, ei, ea, sizes


def _with_hubs(n, hubs, k, seed, outgoing=()):
    x, ei, ea = superpixel_like_graph(n=n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for h in hubs:
        e, a = _hub_edges(rng, n, h, k, outgoing=h in outgoing)
        ei, ea = np.concatenate([ei, e], 1), np.concatenate([ea, a])
    return x, ei, ea


def _star(n, seed, background=3):
    """node 0 receives an edge from every other node, over a sparse random directed background"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, n * background)
    dst = rng.integers(0, n, n * background)
    keep = (src != dst) & (dst != 0)
    ei = np.concatenate([np.stack([src[keep], dst[keep]]), np.stack([np.arange(1, n), np.zeros(n - 1, np.int64)])], 1)
    return rng.random((n, 19)).astype(np.float32), ei.astype(np.int64), rng.random((ei.shape[1], 5)).astype(np.float32)


def _edgeless(n, rng):
    return rng.random((n, 19)).astype(np.float32), np.zeros((2, 0), np.int64), np.zeros((0, 5), np.float32)


def hub_graph():
    """superpixel_like_graph(600) with nodes 0, 31, 32 and 255 receiving 520 extra edges each; node 0 also sends 520"""
    return _with_hubs(600, (0, 31, 32, 255), 520, seed=41, outgoing=(0,))


def graph_zoo():
    """name -> (x (N, 19) f32, edge_index (2, E) i64, edge_attr (E, 5) f32, sizes): one batch of graphs per case, nodes and
    edges concatenated graph by graph.  No i -> i edges."""
    zoo = {}
    zoo["hub"] = _cat_graphs([hub_graph()])
    zoo["star"] = _cat_graphs([_star(2000, seed=42)])

    x, ei, ea = superpixel_like_graph(n=700, seed=43)
    holes = np.array([0, 31, 32, 33, 255, 256, *range(400, 440), 699])
    keep = ~np.isin(ei[1], holes)
    zoo["holes"] = _cat_graphs([(x, ei[:, keep], ea[keep])])

    x, ei, ea = superpixel_like_graph(n=500, seed=44)
    rng = np.random.default_rng(44)
    keep = rng.random(ei.shape[1]) >= 0.3                     # each direction dropped on its own: asymmetric
    ei, ea = ei[:, keep], ea[keep]
    dup = np.sort(rng.choice(ei.shape[1], ei.shape[1] // 10, replace=False))
    zoo["directed_dup"] = _cat_graphs([(x, np.concatenate([ei, ei[:, dup]], 1), np.concatenate([ea, ea[dup]]))])

    rng = np.random.default_rng(45)
    small = []
    for _ in range(1500):
        n = int(rng.integers(1, 4))
        if n == 1 or rng.random() < 0.05:
            small.append(_edgeless(n, rng))
            continue
        pairs = np.array([(i, j) for i in range(n) for j in range(n) if i != j])
        pick = rng.random(len(pairs)) < 0.7
        pick[rng.integers(len(pairs))] = True
        e = pairs[pick].T
        small.append((rng.random((n, 19)).astype(np.float32), e, rng.random((e.shape[1], 5)).astype(np.float32)))
    zoo["many_small"] = _cat_graphs(small)

    rng = np.random.default_rng(46)
    zoo["mixed_batch"] = _cat_graphs([_with_hubs(2000, (5,), 600, seed=46), _edgeless(1, rng), _edgeless(4, rng),
                                      superpixel_like_graph(n=37, seed=47), superpixel_like_graph(n=600, seed=48)])
    zoo["edgeless"] = _cat_graphs([_edgeless(n, rng) for n in (50, 1, 300, 2)])
    for name, (x, ei, ea, sizes) in zoo.items():
        assert x.shape == (sum(sizes), 19) and ea.shape == (ei.shape[1], 5) and not (ei[0] == ei[1]).any(), name
    return zoo


def zoo_graphs(x, edge_index, edge_attr, sizes):
    """one zoo case -> its graphs [(x, edge_index, edge_attr)] with local node indices"""
    off = np.cumsum((0,) + tuple(sizes))
    g = np.searchsorted(off, edge_index[1], side="right") - 1
    assert (np.diff(g) >= 0).all() and (np.searchsorted(off, edge_index[0], side="right") - 1 == g).all()
    out = []
    for i in range(len(sizes)):
        m = g == i
        out.append((x[off[i]:off[i + 1]], edge_index[:, m] - off[i], edge_attr[m]))
    return out


def zoo_batch_vector(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
