"""CPU: the networks' width limits.  ResGCNNet takes any width from 8 to 256 (the kernels run a width that is not a multiple of
32 zero-padded to the next one, up to 256), and GATTrimapNet takes 256 with 1, 2, 4 or 8 heads; the state_dicts follow the
reference's shape formulas.  Above the limits every constructor refuses with ValueError."""
import pytest

from gcn_grabcut.model import GATTrimapNet, GCNTrimapNet, ResGCNNet


@pytest.mark.parametrize("hidden", [129, 160, 200, 256])
def test_resgcn_wide_state_dict_shapes(hidden):
    d, n = hidden, 3
    sd = ResGCNNet(hidden_channels=d, n_layers=n).state_dict()
    q = max(d // 4, 8)                  # prior booster hidden width (reference model.py:472)
    c = max(d // 2, 8)                  # edge context width (reference model.py:123)
    want = {
        "input_proj.0.weight": (d, 19),
        "prior_booster.0.weight": (q, 3), "prior_booster.2.weight": (d, q),
        "edge_ctx.encode.0.weight": (c, 5), "edge_ctx.encode.2.weight": (c, c),
        "edge_ctx.to_gate.0.weight": (c,), "edge_ctx.to_gate.1.weight": (d, c),
        "sage.lin_l.weight": (d, d), "sage.lin_r.weight": (d, d),
        "ctx.compress.weight": (d // 2, d), "ctx.expand.weight": (d, d // 2),
        "fuse.1.weight": (d, d), "head.weight": (3, d), "jk_logits": (n + 2,),
    }
    for i in range(n):
        want[f"gcn_layers.{i}.lin.weight"] = (d, d)
        want[f"norms.{i}.weight"] = (d,)
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, (k, tuple(sd[k].shape), shape)


@pytest.mark.parametrize("heads", [1, 2, 4, 8])
def test_gat_256_state_dict_shapes(heads):
    d, n = 256, 2
    sd = GATTrimapNet(hidden_channels=d, n_layers=n, n_heads=heads).state_dict()
    for i in range(n):
        assert tuple(sd[f"convs.{i}.att"].shape) == (1, heads, d // heads)
        assert tuple(sd[f"convs.{i}.lin_l.weight"].shape) == (d, d)
        assert tuple(sd[f"convs.{i}.lin_edge.weight"].shape) == (d, 5)
        assert tuple(sd[f"edge_gates.{i}.proj.2.weight"].shape) == (d, d)
    assert tuple(sd["skip_proj.weight"].shape) == (d, d)
    assert tuple(sd["head.3.weight"].shape) == (3, d)


def test_resgcn_wide_widths_train_at_multiples_of_32():
    from gcn_grabcut import train_ops
    assert {160, 192, 224, 256} <= set(train_ops.TRAIN_WIDTHS)
    assert 48 not in train_ops.TRAIN_WIDTHS and 200 not in train_ops.TRAIN_WIDTHS


@pytest.mark.parametrize("make", [lambda: ResGCNNet(hidden_channels=257), lambda: ResGCNNet(hidden_channels=7),
                                  lambda: GATTrimapNet(hidden_channels=192), lambda: GATTrimapNet(hidden_channels=256, n_heads=16),
                                  lambda: GCNTrimapNet(hidden_channels=160), lambda: GCNTrimapNet(hidden_channels=130)],
                         ids=["resgcn257", "resgcn7", "gat192", "gat256h16", "gcnnet160", "gcnnet130"])
def test_widths_beyond_the_limits_refuse(make):
    with pytest.raises(ValueError):
        make()


def test_resgcn_refusal_names_the_limit():
    with pytest.raises(ValueError, match="256"):
        ResGCNNet(hidden_channels=257)
