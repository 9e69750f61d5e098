"""GPU: ResGCNNet at the widths above 128 (160, 200 zero-padded to 224, and 256) and GATTrimapNet at 256 with 1, 2, 4 and 8
heads (a head of 32 ... 256 channels), where the kernels take their wide forms: k_gemm stages W in k-chunks, ResGCNNet's edge
gate holds two context channels per lane and computes one column half per block, GAT's fused edge gate reads W2 from L2,
the gathers run D/32 column slices.  The CPU oracle stops at 128, so the contract here is the float64 restatement on the
graph zoo, with the zoo's bounds: |logit - ref| <= 1e-5 (1 + |ref|), probabilities within 1e-5.  On top: a batch equals
its graphs run one at a time bit for bit, two runs are bit-identical, and the pipeline runs a 256-wide network."""
import numpy as np
import pytest
import torch

from helpers import zoo_graphs
from test_gnn_zoo_oracle import assert_close_f64, ref_f64, zoo_model

pytestmark = pytest.mark.gpu
NETS = [("resgcn", w, None) for w in (160, 200, 256)] + [("gat", 256, h) for h in (1, 2, 4, 8)]
NET_IDS = [f"{k}{w}" + (f"h{h}" if h else "") for k, w, h in NETS]
CASES = ["hub", "star", "holes", "directed_dup", "many_small", "mixed_batch", "edgeless"]
GGC_E_UNSUPPORTED = -5


def _datas(x, ei, ea, sizes):
    from gcn_grabcut.data import Data
    return [Data(x=torch.as_tensor(gx), edge_index=torch.as_tensor(gei), edge_attr=torch.as_tensor(gea)).to("cuda")
            for gx, gei, gea in zoo_graphs(x, ei, ea, sizes)]


@pytest.fixture(scope="module")
def zoo():
    from helpers import graph_zoo
    return graph_zoo()


@pytest.fixture(scope="module", params=NETS, ids=NET_IDS)
def net(request):
    kind, width, heads = request.param
    m, sd = zoo_model(kind, width, heads)
    return m.to("cuda").eval(), sd, kind, heads


@pytest.mark.parametrize("case", CASES)
def test_wide_net_matches_float64_on_zoo(gpu_ctx, zoo, net, case):
    from gcn_grabcut.data import Batch
    m, sd, kind, heads = net
    x, ei, ea, sizes = zoo[case]
    b = Batch.from_data_list(_datas(x, ei, ea, sizes))
    got = m(b).cpu().numpy()
    assert_close_f64(got, m.predict_probs(b), *ref_f64(kind, sd, heads, x, ei, ea, sizes))


def test_wide_net_batch_equals_single_graphs(gpu_ctx, zoo, net):
    from gcn_grabcut.data import Batch
    m = net[0]
    datas = _datas(*zoo["mixed_batch"])
    both = m(Batch.from_data_list(datas)).cpu().numpy()
    one = np.concatenate([m(d).cpu().numpy() for d in datas])
    assert np.array_equal(one, both)


def test_wide_net_runs_are_bit_identical(gpu_ctx, zoo, net):
    from gcn_grabcut.data import Batch
    m = net[0]
    b = Batch.from_data_list(_datas(*zoo["hub"]))
    first = m(b).cpu().numpy()
    assert np.array_equal(first, m(b).cpu().numpy())


def test_pipeline_runs_a_256_wide_resgcn(gpu_ctx):
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    from gcn_grabcut.data import Data
    from gcn_grabcut.synthetic import synthetic_batch
    m, _ = zoo_model("resgcn", 256)
    m = m.to("cuda").eval()
    pipe = GCNGrabCutPipeline(m, sp_config=SuperpixelGraphConfig(n_segments=300), device="cuda")
    imgs = synthetic_batch(2, 120, 160, config_id=9)
    out = pipe.segment_batch_device(pipe._eng.to_device(np.ascontiguousarray(imgs)))
    g = out["graphs"]
    for i in range(len(imgs)):
        n0, n1 = int(g.node_ptr_host[i]), int(g.node_ptr_host[i + 1])
        e0, e1 = int(g.edge_ptr_host[i]), int(g.edge_ptr_host[i + 1])
        ei = torch.stack([g.edge_src[e0:e1], g.edge_dst[e0:e1]]).long() - n0
        d = Data(x=g.x[n0:n1], edge_index=ei, edge_attr=g.edge_attr[e0:e1].reshape(-1, 5))
        assert np.array_equal(out["probs"][n0:n1].cpu().numpy(), m.predict_probs(d)), i


@pytest.mark.parametrize("d", [160, 256])
def test_gcn_aggregate_entry_at_wide_widths(gpu_ctx, d):
    """ggc_gcn_aggregate (the direct gather, LPR = 64 above 128) against a float64 restatement, plain and gated"""
    import torch.nn.functional as F
    from gcn_grabcut import _native
    from helpers import superpixel_like_graph
    n = 1203
    _, ei, _ = superpixel_like_graph(n=n, seed=7)
    rng = np.random.default_rng(d)
    xw = rng.standard_normal((n, d)).astype(np.float32)
    bias = rng.standard_normal(d).astype(np.float32)
    gate = rng.random((n, d)).astype(np.float32)
    h = rng.standard_normal((n, d)).astype(np.float32)
    e = ei.shape[1]
    t = lambda a, dt=None: torch.as_tensor(a, dtype=dt).to("cuda").contiguous()      # noqa: E731
    src, dst = t(ei[0], torch.int32), t(ei[1], torch.int32)
    row_ptr = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    col = torch.empty(e, dtype=torch.int32, device="cuda")
    dis = torch.empty(n, dtype=torch.float32, device="cuda")
    st = _native.current_stream(0)
    gpu_ctx.call("ggc_build_csr", st, n, e, src.data_ptr(), dst.data_ptr(), row_ptr.data_ptr(), col.data_ptr(), dis.data_ptr())
    xw_d, bias_d, gate_d, h_d = t(xw), t(bias), t(gate), t(h)
    out, out_g = torch.empty(n, d, device="cuda"), torch.empty(n, d, device="cuda")
    gpu_ctx.call("ggc_gcn_aggregate", st, n, d, xw_d.data_ptr(), row_ptr.data_ptr(), col.data_ptr(), dis.data_ptr(),
                 bias_d.data_ptr(), None, None, out.data_ptr())
    gpu_ctx.call("ggc_gcn_aggregate", st, n, d, xw_d.data_ptr(), row_ptr.data_ptr(), col.data_ptr(), dis.data_ptr(),
                 bias_d.data_ptr(), gate_d.data_ptr(), h_d.data_ptr(), out_g.data_ptr())
    s64, d64 = torch.as_tensor(ei[0]), torch.as_tensor(ei[1])
    x64 = torch.as_tensor(xw).double()
    dis64 = (1.0 + torch.bincount(d64, minlength=n).double()).rsqrt()
    want = torch.zeros(n, d, dtype=torch.float64).index_add(0, d64, (dis64[s64] * dis64[d64])[:, None] * x64[s64])
    want = want + dis64[:, None] ** 2 * x64 + torch.as_tensor(bias).double()
    want_g = torch.as_tensor(h).double() + F.gelu(want * torch.as_tensor(gate).double())
    for got, w in ((out, want), (out_g, want_g)):
        err = (got.cpu().double() - w).abs()
        assert (err <= 1e-5 * (1.0 + w.abs())).all(), err.max().item()


@pytest.mark.parametrize("name,args", [("ggc_resgcn_configure", (257, 2)), ("ggc_gat_configure", (192, 8, 2)),
                                       ("ggc_gat_configure", (256, 16, 2))],
                         ids=["resgcn257", "gat192", "gat256h16"])
def test_configure_refuses_beyond_the_limits(name, args):
    from gcn_grabcut import _native
    ctx = _native.Context(0)
    try:
        with pytest.raises(_native.GGCError) as e:
            ctx.call(name, *args)
        assert e.value.code == GGC_E_UNSUPPORTED
    finally:
        ctx.close()
