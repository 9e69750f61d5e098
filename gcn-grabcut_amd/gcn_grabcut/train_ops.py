"""
Differentiable graph operators of the ResGCNNet training forward, on the `ggc_train_*` kernels of libggc_hip.so.

`GraphPrep` builds the two CSRs (destination and source, both stable in edge order), `dis` and `inv_cnt` once per
batch; every operator below reads it.  Each operator is a `torch.autograd.Function` whose forward and backward call
one library entry on the current stream.  None of them uses a float atomic, so gradients are reproducible bit for bit
(torch's own `index_add_` / `scatter_add_` on the GPU are not).  There is no CPU path.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _native

TRAIN_WIDTHS = (32, 64, 96, 128, 160, 192, 224, 256)


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None or t.numel() == 0 else t.data_ptr()


class GraphPrep:
    """Graph structure shared by every layer of one training forward."""

    def __init__(self, ctx: "_native.Context", edge_index: torch.Tensor, n_nodes: int,
                 node_ptr: Optional[torch.Tensor] = None):
        dev = edge_index.device
        if dev.type != "cuda":
            raise RuntimeError(f"the training graph operators run on the MI355X only; edge_index is on {dev}")
        n, e = int(n_nodes), int(edge_index.size(1))
        if n < 1:
            raise ValueError("a training batch needs at least one node")
        if e and (int(edge_index.min()) < 0 or int(edge_index.max()) >= n):
            raise ValueError(f"edge_index refers to nodes outside [0, {n})")
        self.ctx, self.n, self.e, self.device = ctx, n, e, dev
        self.stream = _native.current_stream(dev.index if dev.index is not None else torch.cuda.current_device())
        self.src = edge_index[0].to(torch.int32).contiguous()
        self.dst = edge_index[1].to(torch.int32).contiguous()
        i32 = dict(dtype=torch.int32, device=dev)
        self.row_ptr, self.srow_ptr = torch.empty(n + 1, **i32), torch.empty(n + 1, **i32)
        m = max(e, 1)                          # never a NULL pointer for the entries, even without edges
        self.col, self.eid = torch.empty(m, **i32), torch.empty(m, **i32)
        self.scol, self.seid = torch.empty(m, **i32), torch.empty(m, **i32)
        self.dis = torch.empty(n, dtype=torch.float32, device=dev)
        self.inv_cnt = torch.empty(n, dtype=torch.float32, device=dev)
        ctx.call("ggc_train_prepare", self.stream, n, e, _p(self.src), _p(self.dst), self.row_ptr.data_ptr(),
                 self.col.data_ptr(), self.eid.data_ptr(), self.srow_ptr.data_ptr(), self.scol.data_ptr(),
                 self.seid.data_ptr(),
                 self.dis.data_ptr(), self.inv_cnt.data_ptr())
        if node_ptr is None:
            node_ptr = torch.tensor([0, n], dtype=torch.int32, device=dev)
        self.node_ptr = node_ptr.to(device=dev, dtype=torch.int32).contiguous()
        self.n_graphs = self.node_ptr.numel() - 1

    def call(self, name: str, *args) -> None:
        self.ctx.call(name, self.stream, *args)


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).contiguous()


def _check_width(d: int) -> None:
    if d not in TRAIN_WIDTHS:
        raise ValueError(f"training runs at widths {TRAIN_WIDTHS}; got {d}")


class GCNConvGated(torch.autograd.Function):
    """y = [h +] gelu((A_hat xw + bias) * gate)  — GCNConv with the ResGCNNet residual epilogue (model.py:523-528).
    With h=None the residual is left to the caller (so that dropout can sit between the two)."""

    @staticmethod
    def forward(fctx, xw, bias, gate, h, prep: GraphPrep):
        n, d = xw.shape
        _check_width(d)
        xw, bias, gate = _f32(xw), _f32(bias), _f32(gate)
        h = None if h is None else _f32(h)
        out = torch.empty_like(xw)
        y = torch.empty_like(xw)
        prep.call("ggc_train_gcn_forward", n, d, xw.data_ptr(), prep.row_ptr.data_ptr(), prep.col.data_ptr(),
                  prep.dis.data_ptr(), bias.data_ptr(), gate.data_ptr(), _p(h), out.data_ptr(), y.data_ptr())
        fctx.save_for_backward(out, gate)
        fctx.prep, fctx.has_h = prep, h is not None
        return y

    @staticmethod
    def backward(fctx, g_y):
        out, gate = fctx.saved_tensors
        prep: GraphPrep = fctx.prep
        n, d = out.shape
        g_y = _f32(g_y)
        g_out, g_gate, g_xw = torch.empty_like(out), torch.empty_like(out), torch.empty_like(out)
        prep.call("ggc_train_gcn_backward", n, d, g_y.data_ptr(), out.data_ptr(), gate.data_ptr(),
                  prep.srow_ptr.data_ptr(), prep.scol.data_ptr(), prep.dis.data_ptr(),
                  g_out.data_ptr(), g_gate.data_ptr(), g_xw.data_ptr())
        return g_xw, g_out.sum(0), g_gate, (g_y if fctx.has_h else None), None


class SageMean(torch.autograd.Function):
    """m_i = mean of x over the in-neighbours of i (0 for none) — the aggregation of SAGEConv (model.py:531)."""

    @staticmethod
    def forward(fctx, x, prep: GraphPrep):
        n, d = x.shape
        _check_width(d)
        x = _f32(x)
        m = torch.empty_like(x)
        prep.call("ggc_train_sage_mean", n, d, x.data_ptr(), prep.row_ptr.data_ptr(), prep.col.data_ptr(),
                  prep.inv_cnt.data_ptr(), m.data_ptr())
        fctx.prep = prep
        return m

    @staticmethod
    def backward(fctx, g_m):
        prep: GraphPrep = fctx.prep
        g_m = _f32(g_m)
        n, d = g_m.shape
        g_x = torch.empty_like(g_m)
        prep.call("ggc_train_sage_mean_backward", n, d, g_m.data_ptr(), prep.srow_ptr.data_ptr(), prep.scol.data_ptr(),
                  prep.inv_cnt.data_ptr(), g_x.data_ptr())
        return g_x, None


class EdgeMean(torch.autograd.Function):
    """ctx_i = mean of the edge rows enc_e over the edges into i (0 for none) — EdgeContext (model.py:128-139)."""

    @staticmethod
    def forward(fctx, enc, prep: GraphPrep):
        c = enc.size(1)
        enc = _f32(enc)
        out = torch.empty(prep.n, c, dtype=torch.float32, device=enc.device)
        prep.call("ggc_train_edge_mean", prep.n, c, _p(enc), prep.row_ptr.data_ptr(), prep.eid.data_ptr(),
                  prep.inv_cnt.data_ptr(), out.data_ptr())
        fctx.prep, fctx.c = prep, c
        return out

    @staticmethod
    def backward(fctx, g_ctx):
        prep: GraphPrep = fctx.prep
        g_ctx = _f32(g_ctx)
        g_enc = torch.empty(prep.e, fctx.c, dtype=torch.float32, device=g_ctx.device)
        prep.call("ggc_train_edge_mean_backward", prep.e, fctx.c, _p(prep.dst), prep.inv_cnt.data_ptr(),
                  g_ctx.data_ptr(), _p(g_enc))
        return g_enc, None


class GraphPool(torch.autograd.Function):
    """hb_i = sum_{j in graph(i)} softmax_graph(score)_j h_j  — the readout of GlobalContextModule (model.py:176-188),
    broadcast back to every node of the graph."""

    @staticmethod
    def forward(fctx, h, score, prep: GraphPrep):
        n, d = h.shape
        _check_width(d)
        score_shape = score.shape
        h, score = _f32(h), _f32(score.reshape(-1))
        attn = torch.empty(n, dtype=torch.float32, device=h.device)
        hb = torch.empty_like(h)
        prep.call("ggc_train_graph_pool", prep.n_graphs, n, d, prep.node_ptr.data_ptr(), h.data_ptr(),
                  score.data_ptr(), attn.data_ptr(), hb.data_ptr())
        fctx.save_for_backward(h, attn)
        fctx.prep, fctx.score_shape = prep, score_shape
        return hb

    @staticmethod
    def backward(fctx, g_hb):
        h, attn = fctx.saved_tensors
        prep: GraphPrep = fctx.prep
        n, d = h.shape
        g_hb = _f32(g_hb)
        g_h, g_score = torch.empty_like(h), torch.empty_like(attn)
        prep.call("ggc_train_graph_pool_backward", prep.n_graphs, n, d, prep.node_ptr.data_ptr(), h.data_ptr(),
                  attn.data_ptr(), g_hb.data_ptr(), g_h.data_ptr(), g_score.data_ptr())
        return g_h, g_score.view(fctx.score_shape), None


def gcn_conv_gated(xw, bias, gate, h, prep):
    return GCNConvGated.apply(xw, bias, gate, h, prep)


def sage_mean(x, prep):
    return SageMean.apply(x, prep)


def edge_mean(enc, prep):
    return EdgeMean.apply(enc, prep)


def graph_pool(h, score, prep):
    return GraphPool.apply(h, score, prep)
