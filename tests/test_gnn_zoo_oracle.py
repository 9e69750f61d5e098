"""CPU: the oracle's three inference networks against a float64 torch restatement on the graph zoo (hubs, nodes without
incoming edges, repeated and one-way edges, batches of tiny and edgeless graphs).  The GPU tests hold the kernels
bit-equal to this oracle, so it is pinned on these structures here, at the widths the GPU tests run."""
import numpy as np
import pytest
import torch

import torch_ref
from helpers import float64_default, graph_zoo, seeded_state_dict, zoo_batch_vector
from test_gat_oracle import seeded_gat
from test_gcnnet_oracle import seeded_gcnnet

LAYERS = 3
# (network, width, heads): ResGCNNet and GCNTrimapNet at the MFMA widths and one zero-padded width, GAT at head widths
# 4, 32, 128 (one head across both registers of a lane) and 16
NETS = [("resgcn", d, None) for d in (32, 96, 128, 48)] + [("gcnnet", d, None) for d in (32, 96, 128, 48)] \
    + [("gat", d, h) for d, h in ((32, 8), (64, 2), (128, 1), (128, 8))]
NET_IDS = [f"{k}{d}" + (f"h{h}" if h else "") for k, d, h in NETS]
# the last head layer and its scale: ResGCNNet's seeded logits already reach 3 to 6; GCNTrimapNet's and GAT's stay
# below 0.6 and the scale brings them to O(1) (GCNTrimapNet's edge gates are 0 on an edgeless graph: only its input
# projection reaches the head there, hence the larger scale)
HEAD = {"resgcn": ("head.weight", 1.0), "gcnnet": ("head.6.weight", 20.0), "gat": ("head.3.weight", 10.0)}
LOGIT_MIN = 0.5     # max |logit| of the float64 reference on every case: below it the relative bound is all slack


def zoo_model(kind, width, heads=None):
    """(module, float32 state dict): the seeded weights of the per-network tests, the last head layer scaled so that
    logits reach O(1) and probabilities move away from 1/3"""
    seed = width + (heads or 0) + 17
    if kind == "resgcn":
        m, sd = seeded_state_dict(width, LAYERS, seed=seed)
    elif kind == "gcnnet":
        m, sd = seeded_gcnnet(width, LAYERS, seed=seed)
    else:
        m, sd = seeded_gat(width, LAYERS, seed=seed, heads=heads)
    key, scale = HEAD[kind]
    sd[key] = sd[key] * scale
    m.load_state_dict(sd)
    return m, sd


def np_state(sd):
    return {k: v.numpy() for k, v in sd.items() if v.dtype.is_floating_point}


def ref_f64(kind, sd, heads, x, ei, ea, sizes):
    """float64 logits and probabilities of the torch restatement; `batch` given where the network has a per-graph readout"""
    sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
    x64, ea64, ei = torch.as_tensor(x).double(), torch.as_tensor(ea).double(), torch.as_tensor(ei)
    batch = torch.as_tensor(zoo_batch_vector(sizes))
    with float64_default():
        if kind == "resgcn":
            logits = torch_ref.resgcn_forward(sd64, LAYERS, x64, ei, ea64, batch)
            probs = torch.softmax(logits, -1)
        elif kind == "gcnnet":
            logits, probs = torch_ref.gcnnet_forward(sd64, LAYERS, x64, ei, ea64)
        else:
            logits, probs = torch_ref.gat_forward(sd64, LAYERS, x64, ei, ea64, batch, heads=heads)
    return logits.numpy(), probs.numpy()


def oracle_forward(oracle, kind, sd, width, heads, x, ei, ea, sizes):
    st, batch = np_state(sd), zoo_batch_vector(sizes)
    if kind == "resgcn":
        return oracle.resgcn_forward(st, width, LAYERS, x, ei, ea, batch)
    if kind == "gcnnet":
        return oracle.gcnnet_forward(st, width, LAYERS, x, ei, ea)
    return oracle.gat_forward(st, width, LAYERS, x, ei, ea, batch, heads=heads)


def assert_close_f64(logits, probs, want_l, want_p):
    """|logits - ref| <= 1e-5 (1 + |ref|) elementwise and probabilities within 1e-5 of the float64 reference"""
    assert logits.shape == want_l.shape and np.isfinite(logits).all()
    assert np.abs(want_l).max() >= LOGIT_MIN
    err = np.abs(logits.astype(np.float64) - want_l)
    worst = np.unravel_index(np.argmax(err / (1.0 + np.abs(want_l))), err.shape)
    assert (err <= 1e-5 * (1.0 + np.abs(want_l))).all(), (worst, err[worst], want_l[worst])
    assert np.abs(probs.astype(np.float64) - want_p).max() <= 1e-5


@pytest.fixture(scope="module")
def zoo():
    return graph_zoo()


@pytest.mark.parametrize("kind,width,heads", NETS, ids=NET_IDS)
@pytest.mark.parametrize("case", ["hub", "star", "holes", "directed_dup", "many_small", "mixed_batch", "edgeless"])
def test_oracle_matches_float64_on_zoo(oracle, zoo, case, kind, width, heads):
    x, ei, ea, sizes = zoo[case]
    _, sd = zoo_model(kind, width, heads)
    logits, probs = oracle_forward(oracle, kind, sd, width, heads, x, ei, ea, sizes)
    assert_close_f64(logits, probs, *ref_f64(kind, sd, heads, x, ei, ea, sizes))
