"""GPU: ResGCNNet's differentiable training forward (train mode) — autograd, agreement with the eval-mode
ggc_resgcn_forward, TrimapLoss gradients of every parameter against a float64 CPU differentiable restatement,
BatchNorm running statistics, bit-identical repeated backward passes, weight re-upload after an optimizer step."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import torch_ref
from helpers import float64_default, hub_graph, seeded_state_dict, superpixel_like_graph

pytestmark = pytest.mark.gpu


def _batch(sizes=(120, 1, 7, 200), seed=0, edgeless=(2,), hub=False):
    """Batch of superpixel-like graphs with training targets; graph indices in `edgeless` get no edges.  With `hub`, the
    first graph is helpers.hub_graph() instead: 600 nodes, four of them with an in-degree above 500."""
    from gcn_grabcut.data import Batch, Data
    graphs = []
    g = torch.Generator().manual_seed(seed)
    for i, n in enumerate(sizes):
        if hub and i == 0:
            x, ei, ea = (torch.as_tensor(a) for a in hub_graph())
            n = x.size(0)
        elif n >= 4 and i not in edgeless:
            x, ei, ea = superpixel_like_graph(n=n, seed=seed + i)
            x, ei, ea = torch.as_tensor(x), torch.as_tensor(ei), torch.as_tensor(ea)
        else:
            x = torch.rand(n, 19, generator=g)
            ei, ea = torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, 5)
        graphs.append(Data(x=x, edge_index=ei, edge_attr=ea, y=torch.randint(0, 3, (n,), generator=g),
                           node_area=torch.rand(n, generator=g) * 0.01 + 1e-4, fg_ratio=torch.rand(n, generator=g)))
    return Batch.from_data_list(graphs)


def _model(hidden=64, layers=3, seed=0, dropout=0.0):
    from gcn_grabcut.model import ResGCNNet
    _, sd = seeded_state_dict(hidden, layers, seed=seed)
    m = ResGCNNet(hidden_channels=hidden, n_layers=layers, dropout=dropout)
    m.load_state_dict(sd)
    return m


def _ref_forward(m, b):
    """float64 CPU restatement of reference model.py:508-536 in train mode (dropout 0), differentiable; `m` is a CPU
    float64 copy of the model, whose nn modules (InputNorm's BatchNorm1d in batch-stat mode included) are used as is."""
    x, ei, ea, batch = b.x.double(), b.edge_index, b.edge_attr.double(), b.batch
    d = m.hidden_channels
    xn = m.in_norm.norm(x)
    h = m.input_proj(xn) * (1.0 + m.prior_booster(x[:, -3:]))
    gate = m.edge_ctx.to_gate(torch_ref.scatter_mean(m.edge_ctx.encode(ea), ei[1], x.size(0)))
    states = [h]
    for gcn, norm in zip(m.gcn_layers, m.norms):
        h = h + F.gelu(torch_ref.gcn_conv(norm(h), ei, gcn.lin.weight, gcn.bias) * gate)
        states.append(h)
    s = torch_ref.sage_conv(h, ei, m.sage.lin_l.weight, m.sage.lin_l.bias, m.sage.lin_r.weight)
    states.append(F.gelu(m.sage_norm(s)))
    w = torch.softmax(m.jk_logits, 0)
    h_jk = torch.stack(states, 0).mul(w[:, None, None]).sum(0)
    with float64_default():
        a = torch_ref.graph_softmax(m.ctx.attn(h_jk), batch)
    ng = int(batch.max()) + 1
    g = torch.zeros(ng, d, dtype=torch.float64).index_add(0, batch, a * h_jk)[batch]
    g = torch.sigmoid(m.ctx.expand(F.relu(m.ctx.compress(g))))
    return m.head(m.fuse(h_jk * g))


def _loss(logits, b):
    from gcn_grabcut import TrimapLoss
    crit = TrimapLoss(weight=torch.tensor([1.5, 0.8, 1.5], dtype=logits.dtype, device=logits.device))
    return crit(logits, b.y, area=b.node_area, fg_ratio=b.fg_ratio, batch=b.batch)


def test_train_forward_has_grad_fn(gpu_ctx):
    m = _model().cuda().train()
    out = m(_batch().to("cuda"))
    assert out.grad_fn is not None and out.shape == (328, 3) and torch.isfinite(out).all()


def test_train_path_agrees_with_eval_path(gpu_ctx):
    m = _model(128, 6, seed=4).cuda()
    b = _batch(sizes=(300, 5, 1, 250), seed=4, edgeless=()).to("cuda")
    m.eval()
    want = m(b)
    m.train()
    m.in_norm.eval()
    got = m(b)
    assert got.grad_fn is not None
    assert (got.detach() - want).abs().max().item() <= 1e-4


@pytest.mark.parametrize("hidden,layers", [(64, 3), (96, 2), (128, 3)])
def test_parameter_gradients_match_float64_reference(gpu_ctx, hidden, layers):
    m = _model(hidden, layers, seed=hidden).cuda().train()
    ref = copy.deepcopy(m).cpu().double().train()
    b = _batch(seed=hidden, hub=hidden == 128)          # at 128 beside a one-node and an edgeless graph: the hub graph
    logits = m(b.to("cuda"))
    _loss(logits, b.to("cuda")).backward()
    ref_logits = _ref_forward(ref, b)
    _loss(ref_logits, b).backward()
    assert (logits.detach().double().cpu() - ref_logits.detach()).abs().max().item() < 1e-4
    n_checked = 0
    for (k, p), (k2, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert k == k2
        assert p.grad is not None, k
        g, r = p.grad.double().cpu(), q.grad
        rel = (g - r).norm().item() / max(r.norm().item(), 1e-12)
        # ctx.attn.bias has an exactly zero gradient (a per-graph softmax ignores a common shift): f32 leaves ~1e-9 there
        analytic_zero = r.norm().item() < 1e-12 and g.abs().max().item() < 1e-7
        assert rel <= 1e-4 or analytic_zero, (k, rel)
        n_checked += 1
    assert n_checked == len(list(m.parameters()))
    for key in ("running_mean", "running_var", "num_batches_tracked"):
        a = getattr(m.in_norm.norm, key).double().cpu()
        r = getattr(ref.in_norm.norm, key).double()
        assert torch.allclose(a, r, rtol=1e-5, atol=1e-6), key


def test_two_backward_passes_are_bit_identical(gpu_ctx):
    m = _model(128, 4, seed=9).cuda().train()
    b = _batch(sizes=(400, 300, 1, 9), seed=9).to("cuda")
    grads = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        m.in_norm.norm.reset_running_stats()
        _loss(m(b), b).backward()
        grads.append([p.grad.cpu().numpy().copy() for p in m.parameters()])
    for (k, _), a, c in zip(m.named_parameters(), *grads):
        assert np.array_equal(a, c), k


def test_optimizer_step_reaches_the_eval_forward(gpu_ctx):
    from gcn_grabcut.model import ResGCNNet
    m = _model(64, 2, seed=5).cuda()
    b = _batch(seed=5).to("cuda")
    before = m.eval()(b).clone()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    m.train()
    _loss(m(b), b).backward()
    opt.step()
    after = m.eval()(b)
    assert not torch.equal(before, after)
    fresh = ResGCNNet(hidden_channels=64, n_layers=2).cuda()
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(fresh.eval()(b), after)


def test_unsupported_training_width_and_other_models_refuse(gpu_ctx):
    from gcn_grabcut.model import GCNTrimapNet, ResGCNNet
    b = _batch(seed=2).to("cuda")
    m = ResGCNNet(hidden_channels=48, n_layers=2).cuda().train()
    with pytest.raises(ValueError):
        m(b)
    assert m.eval()(b).shape == (328, 3)              # inference keeps taking the width
    with pytest.raises(RuntimeError):
        GCNTrimapNet(hidden_channels=32, n_layers=2).cuda().train()(b)
