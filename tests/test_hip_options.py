"""The library's named runtime options (include/graphtrans_hip.h "Named runtime options", csrc/common.hip): every alternative
implementation that stays in the product library is reachable from a test and is held to the oracle here -- round 5 shipped 31
environment switches latched in function-local statics that no test could flip; they are gone, these two remain.

  attn_f32_exact       fp32 token rows on the exact v_mfma_f32_16x16x4_f32 chains instead of bf16x6 products
  bnstats_rows_kernel  BatchNorm-backward statistics in the register-row bf16x6 dX kernel's epilogue (k_lin3r)"""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import assert_close  # noqa: E402

DEV = "cuda"


def test_option_api_without_a_gpu():
    """set returns the previous value, get reads it, unknown names are an error with a message (no GPU needed)"""
    from graphtrans_amd import _lib
    L = _lib.lib()
    for name in ("attn_f32_exact", "bnstats_rows_kernel", "lin_ring"):
        start = _lib.option_get(name)
        assert start in (0, 1)
        assert _lib.option_set(name, 1) == start
        assert _lib.option_get(name) == 1
        assert _lib.option_set(name, 0) == 1
        assert _lib.option_get(name) == 0
        _lib.option_set(name, start)
    assert L.gt_option_set(b"no_such_option", 1) < 0
    assert b"no_such_option" in L.gt_last_error()
    with pytest.raises(Exception):
        _lib.option_get("no_such_option")


@pytest.mark.gpu
@pytest.mark.parametrize("hd", [32, 64])
def test_attn_f32_exact_option_against_float64(hd):
    """fp32 rows: bf16x6 products (default) and the exact fma chains (option) both meet the fp32 bar against the float64 reference of
    tests/test_hip_attention.py -- and they are different kernels (not the same bits)."""
    from graphtrans_amd import _lib, ops
    from test_hip_attention import make_layout, reference

    torch.manual_seed(0)
    nhead = 4 if hd == 32 else 2
    d = nhead * hd
    lay = make_layout("packed", [1, 7, 33, 64, 65, 130, 31, 32, 513])
    qkv = torch.randn(lay.rows, 3 * d)
    w = torch.randn(lay.rows, d)
    ref_in = qkv.clone().requires_grad_(True)
    ref = reference(ref_in, lay, nhead, hd ** -0.5)
    (ref * w.double()).sum().backward()
    got = {}
    prev = _lib.option_get("attn_f32_exact")
    try:
        for exact in (0, 1):
            _lib.option_set("attn_f32_exact", exact)
            x = qkv.to(DEV).requires_grad_(True)
            out = ops.attention(x, lay, nhead)
            (out * w.to(DEV)).sum().backward()
            assert_close(out.cpu(), ref.detach(), atol=1e-4, rtol=1e-4, what=f"ctx exact={exact}")
            assert_close(x.grad.cpu(), ref_in.grad, atol=1e-4, rtol=1e-4, what=f"d_qkv exact={exact}")
            got[exact] = (out.detach().clone(), x.grad.detach().clone())
    finally:
        _lib.option_set("attn_f32_exact", prev)
    assert not torch.equal(got[0][0], got[1][0]), "the option did not change the forward kernel"
    assert not torch.equal(got[0][1], got[1][1]), "the option did not change the backward kernels"


@pytest.fixture(scope="module")
def bnstats(request):
    """GCN, D = 160, code2_like(B=128) with (request.param) or without a virtual node: the model, the batch, the module path's loss
    and gradients -- made once per module and parameter, shared by the tests below, never changed, dropped behind them -- and the
    fused steps that keep the option at one value (`steady`, filled by _bnstats_fused)."""
    from graphtrans_amd import engine, synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    from test_hip_engine import _args, _run

    args = _args(gnn_virtual_node=request.param, gnn_emb_dim=160, gnn_JK="last")
    torch.manual_seed(0)
    model = GNNTransformer(50, ASTNodeEncoder(160, 98, 300, 20), lambda d: torch.nn.Linear(2, d), args).to(DEV).train()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    b = synth.code2_like(B=128, seed=3, num_nodeattributes=300).to(DEV)
    assert b.num_nodes >= 12288
    y = torch.randint(0, 50, (128, 3), device=DEV)
    assert engine.eligible(model, b, None)
    l0, g0, _ = _run(copy.deepcopy(model), b, y, False, 7)
    case = dict(model=model, b=b, y=y, l0=l0, g0=g0, steady={})
    yield case
    case.clear()


def _bnstats_fused(case, on, flip=False):
    """loss and gradients of one fused step with the option at `on`; flip: set to 1 - on between the forward and backward()"""
    from graphtrans_amd import _lib, losses
    if not flip and on in case["steady"]:
        return case["steady"][on]
    prev = _lib.option_get("bnstats_rows_kernel")
    try:
        _lib.option_set("bnstats_rows_kernel", on)
        m = copy.deepcopy(case["model"])   # (the harness of test_hip_engine._run, opened between its forward and its backward)
        m.fused = True
        torch.manual_seed(7)
        loss = losses.code2_loss(m(case["b"]), case["y"])
        if flip:
            _lib.option_set("bnstats_rows_kernel", 1 - on)
        loss.backward()
        res = loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    finally:
        _lib.option_set("bnstats_rows_kernel", prev)
    if not flip:
        case["steady"][on] = res
    return res


def _bnstats_bar(case, l1, g1, tag):
    l0, g0 = case["l0"], case["g0"]
    assert torch.allclose(l0, l1, rtol=1e-5, atol=1e-6)
    top = max(float(v.norm()) / v.numel() ** 0.5 for v in g0.values())
    for n in g0:   # (ReLU gates at fp32 rounding of zero flip between two summation orders: a relative-L2 bar per tensor)
        den = float(g0[n].norm())
        if den / g0[n].numel() ** 0.5 >= 1e-3 * top:   # (a bias in front of a train-mode BatchNorm has NO gradient: rounding noise only)
            assert float((g0[n] - g1[n]).norm()) / den < 5e-3, (tag, n, float((g0[n] - g1[n]).norm()) / den)


@pytest.mark.gpu
@pytest.mark.parametrize("bnstats", [False, True], indirect=True)
def test_bnstats_rows_kernel_option_against_the_module_path(bnstats):
    """GCN at >= 12288 nodes, D = 160 (ten 16-column tiles: the register-row kernel's shape): with the option the previous layer's
    BatchNorm-backward column sums ride in k_lin3r's dX epilogue (one partial row per 128 rows).  Same gradients as the module path
    (separate statistics pass, the oracle-checked composition of ops) to fp32 summation order, with and without a virtual node; and
    not the bits of the default fused path (another summation order: the branch really ran)."""
    res = {}
    for on in (0, 1):
        l1, res[on] = _bnstats_fused(bnstats, on)
        _bnstats_bar(bnstats, l1, res[on], on)
    bn = [n for n in res[0] if "batch_norms.0" in n or "batch_norms.1" in n]
    assert bn and any(not torch.equal(res[0][n], res[1][n]) for n in bn), "the option did not change how the BatchNorm sums are formed"


@pytest.mark.gpu
@pytest.mark.parametrize("bnstats", [False, True], indirect=True)
@pytest.mark.parametrize("a", [0, 1])
def test_bnstats_rows_kernel_option_flipped_between_forward_and_backward(bnstats, a):
    """The option is read when gt_model_prepare sizes the partial-sum slots; the row count it sized travels with the backward's calls
    (gt_gcn_layer::prev_bn_nparts), so the dX GEMM runs on the kernel that fills exactly those rows whatever the option says by then.
    Forward with the option at `a`, 1 - a before backward(): the module path's gradients to the bar of the test above, and the bits
    of the fused step that keeps the option at `a` throughout.  (With a virtual node and a = 0 no statistics ride in any epilogue --
    the exact kernel takes them only without one --: that case is the control, a flip with nothing to disagree about.)"""
    l1, g1 = _bnstats_fused(bnstats, a, flip=True)
    _bnstats_bar(bnstats, l1, g1, ("flipped", a))
    _, steady = _bnstats_fused(bnstats, a)
    for n in steady:
        assert torch.equal(steady[n], g1[n]), (a, n)


@pytest.mark.gpu
def test_bn_partial_row_count_names_the_dx_kernel_or_is_an_error():
    """gt_gcn_layer::prev_bn_nparts on one layer call (>= 1024 rows, fp32, no weight image bound): ceil(N / 64) runs the exact kernel
    and fills the partial rows; ceil(N / 128) asks for the register-row kernel, which does not take a call without a bound image
    (GT_ERR_UNSUPPORTED); a count that is neither is GT_ERR_INVALID_ARG."""
    from graphtrans_amd import layers, synth
    from graphtrans_amd.modules.conv import GCNConv, edge_spec
    from graphtrans_amd.modules.gnn_module import batch_structure
    from graphtrans_amd.modules.norm import BatchNorm1d

    torch.manual_seed(0)
    D = 64
    b = synth.code2_like(B=24, seed=3, num_nodeattributes=300).to(DEV)
    N = int(b.num_nodes)
    assert N >= 1024 and -(-N // 128) != -(-N // 64)
    conv, bn = GCNConv(D, lambda d: torch.nn.Linear(2, d)).to(DEV), BatchNorm1d(D).to(DEV)
    h = torch.randn(N, D, device=DEV, requires_grad=True)
    _, y = layers.gcn_layer(h, None, batch_structure(b), conv, bn, edge_spec(conv.edge_encoder, b.edge_attr, D), True, False, True)
    fn = y.grad_fn
    desc, saved = fn.desc, fn.saved_tensors[1]
    part = torch.zeros(-(-N // 64) * 2 * D, device=DEV)
    # (this layer's own saved block stands in for the previous layer's: same N and D, which is all the epilogue asks of it)
    desc.prev_saved, desc.prev_bn_w, desc.prev_bn_b, desc.prev_relu = saved.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), 1
    desc.prev_bn_part = part.data_ptr()
    for count, msg in ((-(-N // 64) + 1, "fit neither dX kernel"), (-(-N // 128), "register-row kernel")):
        desc.prev_bn_nparts = count
        with pytest.raises(Exception, match=msg):
            y.sum().backward(retain_graph=True)
    assert not part.any()
    desc.prev_bn_nparts = -(-N // 64)
    y.sum().backward()
    assert torch.isfinite(part).all() and part.view(-1, 2, D)[-1].any()
