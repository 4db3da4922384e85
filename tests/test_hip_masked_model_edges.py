"""GNNTransformer with masked layers on a batch WITHOUT adj_list: the mask comes from the batch's own edges as keep-bits
(ops.adjacency_bits, built once per forward).

* G8_masked_train with adj_list removed and adj_self_loops = False is the fixture's own mask: logits and every parameter gradient equal
  the dense adj_list path's bit for bit, and sit within the G8 goldens' tolerance (tests/test_hip_parity.py: conftest.assert_close at
  1e-4) of the reference's recorded outputs and gradients.
* The default adj_self_loops = True is the reference's make_adj_list (np.eye + edges): against oracle.reference_math's float64 model
  forward with adj_list = adj | eye, same tolerance.
* A GraphStore batch (store.batches) through a model with two masked layers, forward and backward, equal to the same batch with an
  adj_list made by tests/adjacency_refs.py.
* A graph longer than max_input_len raises ValueError (the reference fails there with a shape error).
"""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from adjacency_refs import adjacency_keep_ref
from conftest import Golden, assert_close
from helpers import edge_cls, grads_of, load_sd, node_encoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "G8_masked_train"
TOL = 1e-4   # tests/test_hip_parity.py:_run_and_compare, the bar of every G8 golden


def _model(g, **over):
    from graphtrans_amd.models.gnn_transformer import GNNTransformer

    a = g.args()
    a.token_layout = "padded"
    for k, v in over.items():
        setattr(a, k, v)
    m = GNNTransformer(g.meta["num_tasks"], node_encoder(g.meta["feat"], a.gnn_emb_dim), edge_cls(g.meta["edge"]), a)
    m = load_sd(m, g.sd).to(DEV)
    m.train(g.meta["training"])
    return m, a


def _run(g, m, b):
    """logits (list) and parameter gradients of sum_i (out_i * w_i), the fixture's loss"""
    m.zero_grad(set_to_none=True)
    outs = m(b)
    outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
    loss = 0
    for i, o in enumerate(outs):
        loss = loss + (o * g.inputs[f"w{i}"].to(DEV)).sum()
    loss.backward()
    return [o.detach().clone() for o in outs], {k: v.detach().clone() for k, v in grads_of(m).items()}


def _without_adj(b):
    b2 = copy.copy(b)
    del b2.adj_list
    assert not hasattr(b2, "adj_list")
    return b2


def test_fixture_mask_from_edges_equals_adj_list_path_and_the_golden():
    g = Golden(NAME)
    assert g.args().num_encoder_layers_masked > 0
    m, _ = _model(g, adj_self_loops=False)
    b = g.batch().to(DEV)
    dense_out, dense_grads = _run(g, m, b)
    bits_out, bits_grads = _run(g, m, _without_adj(b))
    for i, (x, y) in enumerate(zip(bits_out, dense_out)):
        assert torch.equal(x, y), f"logits {i}: bits path differs from the adj_list path"
    for k in dense_grads:
        assert torch.equal(bits_grads[k], dense_grads[k]), f"grad {k}: bits path differs from the adj_list path"
    for i, o in enumerate(bits_out):
        assert_close(o.cpu(), g.out_list[i], atol=TOL, rtol=TOL, what=f"{NAME} out{i}")
    assert g.gsd
    for k, v in g.gsd.items():
        assert_close(bits_grads[k].cpu(), v, atol=TOL, rtol=TOL, what=f"{NAME} grad {k}")


def test_default_self_loops_against_float64_oracle():
    from oracle import reference_math as rm

    g = Golden(NAME)
    m, a = _model(g)
    assert m.adj_self_loops is True
    b = g.batch()
    got, grads = _run(g, m, _without_adj(b.to(DEV)))
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())
    ref_b = copy.copy(b)
    ref_b.adj_list = [np.asarray(x, bool) | np.eye(x.shape[0], dtype=bool) for x in b.adj_list]
    for k in ("x", "edge_attr"):
        v = getattr(ref_b, k, None)
        if v is not None and v.is_floating_point():
            setattr(ref_b, k, v.double())
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in g.sd.items()}
    oargs = SimpleNamespace(**{k: v for k, v in vars(a).items() if k not in ("compute_dtype", "token_layout", "adj_self_loops")})
    torch.set_default_dtype(torch.float64)   # the oracle's helpers allocate in the default dtype
    try:
        with torch.no_grad():
            ref = rm.gnn_transformer(sd, oargs, ref_b, None, g.meta["training"])
    finally:
        torch.set_default_dtype(torch.float32)
    ref = list(ref) if isinstance(ref, (list, tuple)) else [ref]
    assert len(ref) == len(got)
    for i, (o, r) in enumerate(zip(got, ref)):
        assert r.dtype == torch.float64
        assert_close(o.cpu(), r, atol=TOL, rtol=TOL, what=f"self-loops out{i}")
    # and it is a different mask from the fixture's: the run above is not the adj_list answer by accident
    assert any(not np.asarray(x, bool).diagonal().all() for x in b.adj_list)


def test_graph_store_batch_two_masked_layers():
    from graphtrans_amd import synth
    from graphtrans_amd.data import GraphStore
    from graphtrans_amd.models.gnn_transformer import GNNTransformer

    g = Golden(NAME)
    a = g.args()
    a.token_layout, a.num_encoder_layers_masked, a.max_input_len = "padded", 2, 1000
    store = GraphStore(synth.nci1_raw(12, 3))
    torch.manual_seed(0)
    m = GNNTransformer(2, nn.Linear(37, a.gnn_emb_dim), edge_cls("none"), a).to(DEV)
    m.train()
    batches = list(store.batches(6))
    assert len(batches) == 2
    for b in batches:
        assert not hasattr(b, "adj_list")
        outs = []
        for with_list in (False, True):
            bb = copy.copy(b)
            if with_list:
                sizes = torch.bincount(b.batch, minlength=b.num_graphs).cpu().numpy()
                keep, _ = adjacency_keep_ref(b.edge_index.cpu().numpy(), sizes, int(sizes.max()), None, True)
                bb.adj_list = [keep[i, :n, :n].astype(np.float32) for i, n in enumerate(sizes)]
            m.zero_grad(set_to_none=True)
            out = m(bb)
            out.float().square().sum().backward()
            outs.append((out.detach().clone(), {k: v.clone() for k, v in grads_of(m).items()}))
        (o_bits, g_bits), (o_list, g_list) = outs
        assert bool(torch.isfinite(o_bits).all()) and all(bool(torch.isfinite(v).all()) for v in g_bits.values())
        assert torch.equal(o_bits, o_list)
        for k in g_list:
            assert torch.equal(g_bits[k], g_list[k]), k


def test_graph_longer_than_max_input_len_raises():
    g = Golden(NAME)
    sizes = [int(n) for n in g.meta["sizes"]]
    m, _ = _model(g, max_input_len=max(sizes) - 1)
    with pytest.raises(ValueError, match="max_input_len"):
        m(_without_adj(g.batch().to(DEV)))
