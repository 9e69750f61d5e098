"""bench.py --dump-outputs on stand-in outputs of the timed path (no GPU): the files a caller's arrays become, their dtypes,
the seeded image sample, per-image (local) edge ids of the sampled graphs, and the size budget at the default batch."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench


def _fake_full_output(b, h, w, rng):
    n_nodes = rng.integers(3, 9, b)
    n_edges = rng.integers(2, 12, b)
    node_ptr = np.concatenate([[0], np.cumsum(n_nodes)]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum(n_edges)]).astype(np.int64)
    src = np.concatenate([node_ptr[i] + rng.integers(0, n_nodes[i], n_edges[i]) for i in range(b)])
    dst = np.concatenate([node_ptr[i] + rng.integers(0, n_nodes[i], n_edges[i]) for i in range(b)])
    n, e = int(node_ptr[-1]), int(edge_ptr[-1])
    graphs = SimpleNamespace(node_ptr_host=node_ptr, edge_ptr_host=edge_ptr,
                             x=torch.rand(n, 19), centroids=torch.rand(n, 2), area_ratio=torch.rand(n),
                             edge_src=torch.from_numpy(src.astype(np.int32)), edge_dst=torch.from_numpy(dst.astype(np.int32)),
                             edge_attr=torch.rand(e, 5))
    u8 = lambda *s: torch.from_numpy(rng.integers(0, 256, s, dtype=np.uint8))     # noqa: E731
    return {"segments": torch.from_numpy(rng.integers(0, 600, (b, h, w), dtype=np.int32)), "trimap": u8(b, h, w),
            "gc_mask": u8(b, h, w), "binary_mask": u8(b, h, w), "overlay": u8(b, h, w, 3), "rgba": u8(b, h, w, 4),
            "probs": torch.rand(n), "graphs": graphs}


def test_full_workload_dump(tmp_path):
    b, h, w = 20, 6, 7
    out = _fake_full_output(b, h, w, np.random.default_rng(0))
    info = bench.dump_outputs(str(tmp_path / "d"), "full", out, b)
    got = {p.stem: np.load(p) for p in (tmp_path / "d").glob("*.npy")}
    assert sorted(f"{k}.npy" for k in got) == info["files"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert info["bytes"] == sum(a.nbytes for a in got.values())

    pick = got["sample_index"].astype(np.int64)
    assert len(pick) == bench.DUMP_SAMPLE and np.all(np.diff(pick) > 0) and pick.max() < b
    again = bench.dump_outputs(str(tmp_path / "e"), "full", out, b)          # the sample is fixed: same files, same bytes
    for name in again["files"]:
        assert np.array_equal(np.load(tmp_path / "e" / name), np.load(tmp_path / "d" / name))

    for name in ("segments", "trimap", "gc_mask", "binary_mask", "overlay", "rgba"):
        assert np.array_equal(got[name], out[name].numpy()[pick].astype(np.float32))
    assert np.array_equal(got["probs"], out["probs"].numpy())

    g = out["graphs"]
    assert np.array_equal(got["graph_node_ptr"], g.node_ptr_host) and np.array_equal(got["graph_edge_ptr"], g.edge_ptr_host)
    e_off = n_off = 0
    for i in pick:
        n0, n1 = g.node_ptr_host[i], g.node_ptr_host[i + 1]
        e0, e1 = g.edge_ptr_host[i], g.edge_ptr_host[i + 1]
        ne, nn = e1 - e0, n1 - n0
        want = np.stack([g.edge_src.numpy()[e0:e1], g.edge_dst.numpy()[e0:e1]]).astype(np.int64) - n0
        assert np.array_equal(got["graph_edge_index"][:, e_off:e_off + ne], want)
        assert np.array_equal(got["graph_edge_attr"][e_off:e_off + ne], g.edge_attr.numpy()[e0:e1])
        assert np.array_equal(got["graph_x"][n_off:n_off + nn], g.x.numpy()[n0:n1])
        e_off, n_off = e_off + ne, n_off + nn
    assert e_off == got["graph_edge_index"].shape[1] and n_off == got["graph_x"].shape[0]


def test_gcn_workload_dump(tmp_path):
    probs = torch.rand(50)
    info = bench.dump_outputs(str(tmp_path), "gcn", probs, 4)
    assert info["files"] == ["probs.npy"]
    a = np.load(tmp_path / "probs.npy")
    assert a.dtype == np.float32 and np.array_equal(a, probs.numpy())


def test_default_batch_dump_fits_the_budget(tmp_path):
    """batch 256 of 400x300 with ~600 regions and ~6.4k directed edges per image (the default workload) stays under 64 MB"""
    rng = np.random.default_rng(1)
    b, n_img, e_img = 256, 600, 6400
    out = _fake_full_output(2, 1, 1, rng)                                   # only the shapes below matter
    n, e = b * n_img, b * e_img
    node_ptr = np.arange(b + 1, dtype=np.int64) * n_img
    edge_ptr = np.arange(b + 1, dtype=np.int64) * e_img
    src = np.repeat(node_ptr[:-1], e_img).astype(np.int32)
    out["graphs"] = SimpleNamespace(node_ptr_host=node_ptr, edge_ptr_host=edge_ptr, x=torch.zeros(n, 19),
                                    centroids=torch.zeros(n, 2), area_ratio=torch.zeros(n), edge_src=torch.from_numpy(src),
                                    edge_dst=torch.from_numpy(src), edge_attr=torch.zeros(e, 5))
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8)                       # noqa: E731
    out.update(segments=torch.zeros(b, bench.H, bench.W, dtype=torch.int32), trimap=z(b, bench.H, bench.W),
               gc_mask=z(b, bench.H, bench.W), binary_mask=z(b, bench.H, bench.W), overlay=z(b, bench.H, bench.W, 3),
               rgba=z(b, bench.H, bench.W, 4), probs=torch.zeros(n))
    info = bench.dump_outputs(str(tmp_path), "full", out, b)
    assert 0 < info["bytes"] <= bench.DUMP_MAX_BYTES


def test_steps_below_one_are_refused(monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
