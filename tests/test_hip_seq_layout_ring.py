"""The one pinned staging ring per device (graphtrans_amd/graph.py:StageRing), shared by the module path's SeqLayout and the fused
step's gt_model_prepare: a slot is refilled only after the H2D copy that last read it has run, whoever took it."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_model_driver_host import check_seq_layout, numpy_layout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _layouts(count):
    """`count` packed layouts built back to back, all kept alive: [(SeqLayout, its numpy oracle)]"""
    from graphtrans_amd.graph import SeqLayout
    out = []
    for i in range(count):
        sizes = np.roll([5, 1, 9, 3, 70, 2, 8], i) + i % 4
        gs = SimpleNamespace(sizes=sizes.astype(np.int64), B=7, device=DEV)
        out.append((SeqLayout(gs, "packed", 64, bool(i % 2)), numpy_layout(sizes, "packed", 64, i % 2)))   # (64 truncates the long graph)
    return out


def test_a_slot_is_not_refilled_before_its_copy_ran():
    from graphtrans_amd.graph import StageRing
    built = _layouts(2 * StageRing.SLOTS + 6)
    torch.cuda.synchronize()
    for lay, want in built:
        check_seq_layout(lay, want)


def test_module_path_layouts_and_fused_steps_share_the_ring():
    from graphtrans_amd import losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    from test_hip_engine import _args
    sizes = torch.bincount(synth.code2_like(B=12, seed=5, num_nodeattributes=300).batch).numpy()
    torch.manual_seed(0)
    model = GNNTransformer(50, ASTNodeEncoder(64, 98, 300, 20), lambda d: torch.nn.Linear(2, d), _args(transformer_dropout=0.0)).to(DEV).train()
    model.fused = True
    y = torch.randint(0, 50, (12, 5), device=DEV)

    def step():
        bb = synth.code2_like(B=12, seed=5, num_nodeattributes=300).to(DEV)
        bb._sizes = sizes
        for p in model.parameters():
            p.grad = None
        loss = losses.code2_loss(model(bb), y)
        loss.backward()
        return loss.detach().clone(), [p.grad.detach().clone() for p in model.parameters()]

    first = step()
    later, built = [], []
    for _ in range(4):
        built += _layouts(40)
        later.append(step())
    torch.cuda.synchronize()
    for loss, grads in later:
        assert torch.equal(loss, first[0])
        for (n, _), a, c in zip(model.named_parameters(), grads, first[1]):
            assert torch.equal(a, c), n
    for lay, want in built:
        check_seq_layout(lay, want)
