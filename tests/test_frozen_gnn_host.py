"""Frozen gnn_node on the fused step, host side (no GPU): the pattern decision engine.frozen_pattern on CPU-built models, the
`gnn_frozen` field of the driver's batch struct, and the --fused_freeze flag of both models' parsers."""
import argparse
import ctypes as C

import pytest
import torch


def _gnn_transformer(**kw):
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    from oracle.reference_math import default_args
    a = default_args(gnn_emb_dim=16, d_model=16, nhead=2, dim_feedforward=32, num_encoder_layers=1, gnn_num_layer=2,
                     gnn_virtual_node=True, graph_pooling="cls", max_seq_len=2, **kw)
    return GNNTransformer(3, torch.nn.Linear(6, 16), lambda d: torch.nn.Linear(2, d), a)


def _pna_transformer(**kw):
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.pna_transformer import PNATransformer
    from oracle.reference_math import default_args
    a = default_args(gnn_virtual_node=False, gnn_num_layer=2, gnn_emb_dim=16, gnn_JK="last", gnn_residual=True, gnn_dropout=0.0,
                     d_model=16, nhead=2, dim_feedforward=32, transformer_dropout=0.0, num_encoder_layers=1,
                     transformer_norm_input=True, graph_pooling="cls", max_seq_len=2, aggregators=["mean", "max"],
                     scalers=["identity", "amplification"], deg=torch.tensor([0, 4, 2, 1]), **kw)
    return PNATransformer(5, ASTNodeEncoder(16, 9, 11, 20), None, a)


BUILDERS = {"gnn": _gnn_transformer, "pna": _pna_transformer}


def _first_conv(model):
    gnn = model.gnn_node
    return (gnn.layers if hasattr(gnn, "layers") else gnn.convs)[0]


def _head(model):
    return model.graph_pred_linear_list[0]


@pytest.mark.parametrize("kind", ["gnn", "pna"])
def test_frozen_pattern(kind):
    from graphtrans_amd import engine
    build = BUILDERS[kind]
    model = build(freeze_gnn=1)
    assert engine.frozen_pattern(model) == "none"
    model.epoch_callback(0)            # before the freeze epoch: nothing happens
    assert engine.frozen_pattern(model) == "none"
    model.epoch_callback(1)
    assert engine.frozen_pattern(model) == "gnn"
    assert all(not p.requires_grad for p in model.gnn_node.parameters())
    assert all(p.requires_grad for n, p in model.named_parameters() if not n.startswith("gnn_node."))
    model.epoch_callback(2)            # later epochs: still exactly gnn_node
    assert engine.frozen_pattern(model) == "gnn"
    model.gnn_node.requires_grad_(False)
    assert engine.frozen_pattern(model) == "gnn"
    _head(model).bias.requires_grad_(False)    # gnn_node plus a head
    assert engine.frozen_pattern(model) == "other"
    model.requires_grad_(True)         # un-frozen by hand
    assert engine.frozen_pattern(model) == "none"
    # one conv only
    model = build()
    _first_conv(model).requires_grad_(False)
    assert engine.frozen_pattern(model) == "other"
    # gnn_node but for one parameter
    model = build()
    model.gnn_node.requires_grad_(False)
    next(model.gnn_node.parameters()).requires_grad_(True)
    assert engine.frozen_pattern(model) == "other"
    # gnn2transformer only
    model = build()
    model.gnn2transformer.weight.requires_grad_(False)
    assert engine.frozen_pattern(model) == "other"
    # everything
    model = build()
    model.requires_grad_(False)
    assert engine.frozen_pattern(model) == "other"


@pytest.mark.parametrize("kind", ["gnn", "pna"])
def test_fused_freeze_is_read_from_the_args_and_defaults_to_off(kind):
    build = BUILDERS[kind]
    assert build().fused_freeze is False
    assert build(fused_freeze=True).fused_freeze is True
    from graphtrans_amd import engine
    m = build(fused_freeze=True)
    assert engine._frozen_ok(m)
    m.gnn_node.requires_grad_(False)
    assert engine._frozen_ok(m)
    m.fused_freeze = False             # the default: a frozen gnn_node leaves the fused path
    assert not engine._frozen_ok(m)
    m.fused_freeze = True
    m.gnn2transformer.bias.requires_grad_(False)
    assert not engine._frozen_ok(m)    # any other pattern stays on the module path, flag or not


def test_parsers_accept_fused_freeze():
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    from graphtrans_amd.models.pna_transformer import PNATransformer
    for cls in (GNNTransformer, PNATransformer):
        parser = argparse.ArgumentParser(conflict_handler="resolve")
        cls.add_args(parser)
        assert parser.parse_args([]).fused_freeze is False
        a = parser.parse_args(["--freeze_gnn", "3", "--fused_freeze"])
        assert a.fused_freeze is True and a.freeze_gnn == 3


def test_batch_struct_carries_gnn_frozen_in_the_old_pad_slot():
    """gt_model_batch::gnn_frozen took the place of the pad word behind sync_bn: no size changes, mirrors and library agree."""
    from graphtrans_amd import _lib, engine
    names = [f[0] for f in engine.BatchDesc._fields_]
    assert "gnn_frozen" in names and "pad2_" not in names
    assert names.index("gnn_frozen") == names.index("sync_bn") + 1
    assert engine.BatchDesc.gnn_frozen.size == 4 and engine.BatchDesc.gnn_frozen.offset == engine.BatchDesc.sync_bn.offset + 4
    assert engine.BatchDesc.gnn_p.offset == engine.BatchDesc.gnn_frozen.offset + 4
    engine._ABI_OK.clear()
    engine._check_abi()
    out = (C.c_int64 * 4)()
    assert _lib.lib().gt_model_abi_sizes(out) == 0
    assert out[0] == C.sizeof(engine.ModelDesc) and out[1] == C.sizeof(engine.BatchDesc)
    bt = engine.BatchDesc()
    assert bt.gnn_frozen == 0
    bt.gnn_frozen = 1
    assert bt.sync_bn == 0 and bt.gnn_p == 0.0
