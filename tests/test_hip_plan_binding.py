"""engine._Plan on the device against model_layout.ModelLayout on a CPU copy of the same model: the binding adds pointers, streams,
events and buffers to the layout and changes nothing the layout decided.  Then one training step each for the two models that
re-home the most storage (GIN with edge tables, PNANet's position heads) against the module path, at the
tolerances of tests/test_hip_engine.py."""
import copy
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import plan_layout_dump as grid   # noqa: E402

SMALL = ["gt:gin,tables,virtual", "gt:linear37,zero-edge", "gnn:gin,plain,max,one-head", "pnanet:mlp", "pnanet:positions,D=64", "tr:linear37"]


@pytest.mark.parametrize("name", SMALL)
def test_plan_carries_the_layouts_bytes(name):
    from graphtrans_amd import engine
    from graphtrans_amd.model_layout import ModelLayout
    torch.manual_seed(0)
    model = grid.laid_out_grid()[name](DEV)
    twin = copy.deepcopy(model).cpu()
    plan = engine._plan(model)
    lay = ModelLayout(twin)
    cm = engine.ModelDesc()
    lay.fill(cm)
    cm.vn_defer_dw, cm.dw_overlap_min_elems = int(engine.VN_DEFER_DW), engine.DW_OVERLAP_MIN_ELEMS   # the binding's two switches
    assert grid.struct_fields(plan.cm) == grid.struct_fields(cm)
    for arr, other, n in ((plan.conv_desc, lay.conv_desc, plan.L), (plan.vn_desc, lay.vn_desc, plan.L - 1 if plan.has_vn else 0),
                          (plan.enc_desc, lay.enc_desc, int(plan.cm.n_enc))):
        assert [grid.struct_fields(arr[i]) for i in range(n)] == [grid.struct_fields(other[i]) for i in range(n)]
    names, twin_names = ({id(p): k for k, p in m.named_parameters()} for m in (model, twin))
    assert [(names[id(p)], o) for p, o in plan.params] == [(twin_names[id(p)], o) for p, o in lay.params]
    assert plan.total == lay.total == plan.flat.numel()
    for desc, field, t in plan.ptrs:   # the device plan's pointers name the device parameters
        assert getattr(plan.cm if desc is None else desc, field) == t.data_ptr() and t.is_cuda, field


def _step(model, b, loss_of, fused, seed=7):
    model.fused = fused
    for p in model.parameters():
        p.grad = None
    torch.manual_seed(seed)
    loss = loss_of(model(b))
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, \
        {n: t.detach().clone() for n, t in model.named_buffers()}


@pytest.mark.parametrize("name", ["gt:gin,tables,virtual", "pnanet:positions,D=64"])
def test_training_step_matches_module_path(name):
    from graphtrans_amd import engine, losses, synth
    torch.manual_seed(0)
    model = grid.laid_out_grid()[name](DEV)
    with torch.no_grad():   # non-trivial BatchNorm affine / biases
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    model.train()
    if name.startswith("gt:"):
        b = synth.molpcba_like(B=24, seed=4).to(DEV)
        loss_of = lambda out: out.float().square().mean()
    else:
        b = synth.code2_like(B=12, seed=5, num_nodetypes=11, num_nodeattributes=13).to(DEV)
        y = torch.randint(0, 7, (12, 5), generator=torch.Generator().manual_seed(1)).to(DEV)
        loss_of = lambda out: losses.code2_loss(out, y)
    assert engine.eligible(model, b, None)
    ref = copy.deepcopy(model)
    l0, g0, b0 = _step(ref, b, loss_of, False)
    l1, g1, b1 = _step(model, b, loss_of, True)
    tol = dict(rtol=1e-4, atol=1e-6)   # (tests/test_hip_engine.py, fp32)
    assert torch.allclose(l0, l1, **tol), (l0, l1)
    assert set(g0) == set(g1)
    for n in g0:
        scale = max(1.0, float(g0[n].abs().max()))
        assert torch.allclose(g0[n] / scale, g1[n] / scale, **tol), (n, (g0[n] - g1[n]).abs().max())
    for n in b0:   # BatchNorm running statistics advance identically
        assert torch.allclose(b0[n].float(), b1[n].float(), rtol=1e-4, atol=1e-6), n
