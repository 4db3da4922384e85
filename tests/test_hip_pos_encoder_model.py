"""GNNTransformer with pos_encoder=True on the packed token layout (token_layout="packed", opt-in): the packed module path and the
fused step against the reference fixture, against each other, against the padded layout, and with a device-built layout."""
import copy
from types import SimpleNamespace

import pytest
import torch

from conftest import Golden, assert_close
from helpers import edge_cls, grads_of, load_sd, node_encoder, zero_edge_encoder_cls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _args(**kw):
    a = dict(gnn_virtual_node=True, gnn_num_layer=3, gnn_emb_dim=64, gnn_JK="cat", gnn_dropout=0.0, gnn_residual=False,
             gnn_type="gcn", pretrained_gnn=None, freeze_gnn=None, d_model=32, nhead=4, dim_feedforward=64,
             transformer_dropout=0.2, transformer_activation="relu", num_encoder_layers=2, max_input_len=1000,
             transformer_norm_input=True, graph_pooling="cls", num_encoder_layers_masked=0, transformer_prenorm=False,
             pos_encoder=False, max_seq_len=3, compute_dtype=torch.float32, token_layout="auto")
    a.update(kw)
    return SimpleNamespace(**a)


def _run_and_compare(g, module, fwd, float_inputs, atol=1e-4):   # (tests/test_hip_parity.py: the bar of every golden test)
    outs = fwd()
    outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
    assert len(outs) == len(g.out_list)
    loss = 0
    for i, o in enumerate(outs):
        assert_close(o.detach().cpu(), g.out_list[i], atol=atol, rtol=atol, what=f"{g.name} out{i}")
        loss = loss + (o * g.inputs[f"w{i}"].to(DEV)).sum()
    if not g.gsd and not g.gin:
        return
    loss.backward()
    got = grads_of(module)
    for k, v in g.gsd.items():
        assert_close(got[k].cpu(), v, atol=atol, rtol=atol, what=f"{g.name} grad {k}")
    for k, v in g.gin.items():
        assert_close(float_inputs[k].grad.cpu(), v, atol=atol, rtol=atol, what=f"{g.name} grad input {k}")


def _run(model, batch, y, fused, seed):
    from graphtrans_amd import losses
    model.fused = fused
    for p in model.parameters():
        p.grad = None
    torch.manual_seed(seed)
    out = model(batch)
    loss = losses.code2_loss(out, y) if model.max_seq_len is not None else out.float().square().mean()
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, \
        {n: b.detach().clone() for n, b in model.named_buffers()}


@pytest.mark.parametrize("fused", [False, True], ids=["modules", "fused"])
def test_golden_last_pos_on_the_packed_layout(fused):
    """G8_last_pos (pos_encoder, `last` pooling, sizes (9, 1, 17, 6)) with token_layout="packed": outputs and every gradient against
    the reference's, at the 1e-4 bar of the other golden tests; the engine takes the model on `packed` and declines it on `auto`."""
    from graphtrans_amd import engine
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    g = Golden("G8_last_pos_train")
    b = g.batch().to(DEV)

    def build(layout):
        a = g.args()
        a.token_layout = layout
        m = GNNTransformer(g.meta["num_tasks"], node_encoder(g.meta["feat"], a.gnn_emb_dim), edge_cls(g.meta["edge"]), a)
        m = load_sd(m, g.sd).to(DEV)
        return m.train(g.meta["training"])

    m = build("packed")
    assert m.pos_encoder is not None and m._use_packed()
    assert engine.eligible(m, b, None) and not engine.eligible(build("auto"), b, None)
    m.fused = fused
    assert engine.eligible(m, b, None) == fused
    _run_and_compare(g, m, lambda: m(b), {})


CASES = [dict(), dict(d_model=128, nhead=4, dim_feedforward=64), dict(graph_pooling="last", transformer_norm_input=False),
         dict(compute_dtype=torch.bfloat16), dict(max_input_len=8)]


def _fused_vs_modules(args, make_model, make_batch, y, bf16, mm_bf16=None):
    """(a fresh batch for the fused run: one the module path has been through carries its token layout, and the driver then gathers)"""
    from graphtrans_amd import engine, ops
    ops.set_matmul_dtype(torch.bfloat16 if (bf16 if mm_bf16 is None else mm_bf16) else torch.float32)
    try:
        b = make_batch()
        torch.manual_seed(0)
        model = make_model(args).to(DEV)
        with torch.no_grad():  # non-trivial virtual-node embedding and BN statistics
            for p in model.parameters():
                if p.dim() == 1:
                    p.add_(torch.randn_like(p) * 0.1)
            if args.gnn_virtual_node:
                model.gnn_node.virtualnode_embedding.weight.normal_(0, 0.3)
        model.train()
        assert engine.eligible(model, b, None)
        ref_model = copy.deepcopy(model)
        l0, g0, b0 = _run(ref_model, b, y, False, 7)
        b = make_batch()
        assert "_gt_structure" not in b.__dict__
        l1, g1, b1 = _run(model, b, y, True, 7)
        tol = dict(rtol=2e-2, atol=2e-3) if bf16 else dict(rtol=1e-4, atol=1e-6)
        assert torch.allclose(l0, l1, **tol), (l0, l1)
        for n in g0:
            scale = max(1.0, float(g0[n].abs().max()))
            assert torch.allclose(g0[n] / scale, g1[n] / scale, **tol), (n, (g0[n] - g1[n]).abs().max())
        for n in b0:  # BatchNorm running statistics advance identically
            assert torch.allclose(b0[n].float(), b1[n].float(), rtol=1e-4, atol=1e-6), n
        return model
    finally:
        ops.set_matmul_dtype(torch.float32)


MIXED = dict(compute_dtype=torch.bfloat16, mixed=True)   # bf16 token rows behind fp32 GEMMs: the row map + addend epilogue rounding to bf16


@pytest.mark.parametrize("kw", CASES + [MIXED], ids=[",".join(f"{k}={v}" for k, v in c.items()) or "default" for c in CASES + [MIXED]])
def test_fused_matches_packed_module_path_with_pos_encoder(kw):
    """The harness and tolerances of test_hip_engine.py::test_fused_model_matches_module_path with pos_encoder + packed.  The batch has
    >= 1024 nodes: with fp32 GEMMs gnn2transformer stores the token rows + pe through its row map (the driver's fuse_rows branch --
    asked of the library the way the driver asks)."""
    from graphtrans_amd import _lib, engine, synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    kw = dict(kw)
    mixed = kw.pop("mixed", False)
    args = _args(pos_encoder=True, token_layout="packed", **kw)
    bf16 = args.compute_dtype == torch.bfloat16
    make_batch = lambda: synth.code2_like(B=12, seed=5, num_nodeattributes=300).to(DEV)
    b = make_batch()
    y = torch.randint(0, 50, (12, 5), device=DEV)
    N = int(b.batch.numel())
    assert N >= 1024
    if args.max_input_len == 8:
        assert int(torch.bincount(b.batch).max()) > 8
    model = _fused_vs_modules(args, lambda a: GNNTransformer(50, ASTNodeEncoder(64, 98, 300, 20), lambda d: torch.nn.Linear(2, d), a), make_batch, y,
                              bf16, mm_bf16=False if mixed else None)
    plan = engine._plan(model)
    assert plan.cm.pe == model.pos_encoder.pe.data_ptr() and plan.cm.pe_rows == 5000
    if not bf16 or mixed:
        # fp32 GEMMs: the driver's fuse_rows predicate (csrc/model.hip: no caller's layout -- asserted above -- and gt_linear_rows_ok
        # under the plan's bound images) holds, i.e. gnn2transformer stored the token rows + pe through its row map
        imgs = plan.imgs3 if bf16 else (plan.imgs3e or plan.imgs3)
        w = model.gnn2transformer.weight
        with imgs.bound():
            assert _lib.lib().gt_linear_rows_ok(0, 0, 1 if bf16 else 0, w.data_ptr(), N, w.shape[0], w.shape[1]) == 1


def test_fused_matches_packed_module_path_below_1024_node_rows():
    """nci1_like(B=8): ~240 node rows, a Linear node encoder, no edge features -- the driver's gather branch (gt_seq_gather_add)."""
    from graphtrans_amd import synth
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    args = _args(pos_encoder=True, token_layout="packed", max_seq_len=None)
    make_batch = lambda: synth.nci1_like(B=8, seed=1).to(DEV)
    assert int(make_batch().batch.numel()) < 1024
    _fused_vs_modules(args, lambda a: GNNTransformer(2, torch.nn.Linear(37, 64), zero_edge_encoder_cls, a), make_batch, None, False)


@pytest.mark.parametrize("max_input_len", [1000, 20])
def test_packed_equals_padded_with_pos_encoder(max_input_len):
    """One model, token_layout "packed" and "padded" (the reference layout: pad_batch, x + pe[:S], encoder over (S, B, d)): logits and
    gradients at the tolerance of tests/test_hip_attention.py::test_packed_equals_padded_encoder (assert_close's default 1e-4 bar)."""
    from graphtrans_amd import synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    b = synth.code2_like(B=6, seed=3, num_nodeattributes=300).to(DEV)
    assert max_input_len == 1000 or int(torch.bincount(b.batch).max()) > max_input_len
    y = torch.randint(0, 50, (6, 5), device=DEV)
    args = _args(pos_encoder=True, token_layout="packed", transformer_dropout=0.0, max_input_len=max_input_len)
    torch.manual_seed(0)
    packed = GNNTransformer(50, ASTNodeEncoder(64, 98, 300, 20), lambda d: torch.nn.Linear(2, d), args).to(DEV).train()
    padded = copy.deepcopy(packed)
    padded.layout = "padded"
    res = {}
    for name, m, fused in (("padded", padded, False), ("packed", packed, False), ("fused", packed, True)):
        m.fused = fused
        for p in m.parameters():
            p.grad = None
        out = m(b)
        from graphtrans_amd import losses
        losses.code2_loss(out, y).backward()
        res[name] = ([o.detach().float().cpu().clone() for o in out], {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()})
    for name in ("packed", "fused"):
        for i, (o, r) in enumerate(zip(res[name][0], res["padded"][0])):
            assert_close(o, r, what=f"{name} logits {i}")
        for n, gr in res["padded"][1].items():
            assert_close(res[name][1][n], gr, what=f"{name} grad {n}")


@pytest.mark.parametrize("max_input_len", [1000, 150])
def test_device_built_layout_with_pos_encoder_equals_the_host_sizes_run(max_input_len):
    """A batch without host-side sizes: S reaches gt_seq_positions from gt_seq_layout_packed's meta on the device.  Same logits, bit
    for bit, as the run whose layout (and S) came from host sizes -- fused and module path.
    (150 truncates the graphs of 165, 208 and 280 nodes and leaves 1226 token rows.  Bit equality needs both runs on the same GEMM
    kernels: the device-built layout sizes its launches by the upper bound N + B = 1429 rows, and below 1024 exact rows -- e.g. 492
    at max_input_len = 40 -- the host-sizes run's encoder GEMMs take the short-M kernels, which sum in another order, with or
    without a positional encoding.)"""
    from graphtrans_amd import synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    b = synth.code2_like(B=12, seed=5, num_nodeattributes=300).to(DEV)
    sizes = torch.bincount(b.batch).cpu().numpy()
    assert max_input_len == 1000 or sizes.max() > max_input_len
    args = _args(max_input_len=max_input_len, transformer_dropout=0.0, pos_encoder=True, token_layout="packed")
    torch.manual_seed(0)
    model = GNNTransformer(50, ASTNodeEncoder(64, 98, 300, 20), lambda d: torch.nn.Linear(2, d), args).to(DEV).train()
    for fused in (True, False):
        outs = []
        for with_sizes in (True, False):
            bb = synth.code2_like(B=12, seed=5, num_nodeattributes=300).to(DEV)
            if with_sizes:
                bb._sizes = sizes
            model.fused = fused
            with torch.no_grad():
                outs.append([o.clone() for o in model(bb)])
        for u, v in zip(*outs):
            assert torch.equal(u, v), fused
    # the module path's device-built layout handed to the fused step (S through gt_model_batch::lay_meta)
    bb = synth.code2_like(B=12, seed=5, num_nodeattributes=300).to(DEV)
    with torch.no_grad():
        model.fused = False
        model(bb)
        model.fused = True
        assert not bb._gt_structure.layout("packed", max_input_len, True).exact
        again = model(bb)
    for u, v in zip(again, outs[0]):
        assert torch.allclose(u, v, rtol=1e-4, atol=1e-5)


def test_packed_with_pos_encoder_contract_edges_on_the_device():
    from graphtrans_amd import synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    b = synth.code2_like(B=4, seed=2).to(DEV)

    def model(**kw):
        return GNNTransformer(50, ASTNodeEncoder(64, 98, 10030, 20), lambda d: torch.nn.Linear(2, d),
                              _args(pos_encoder=True, token_layout="packed", **kw)).to(DEV).train()

    m = model()
    m.pos_encoder.dropout.p = 0.1
    with pytest.raises(ValueError, match="dropout"):
        m(b)
    with pytest.raises(ValueError, match="max_input_len"):
        model(max_input_len=5001)(b)
    with pytest.raises(ValueError, match="mean pooling"):
        model(graph_pooling="mean")(b)
    m = model()
    m.pos_encoder.pe = m.pos_encoder.pe.cpu()   # a buffer that is not on the model's device
    with pytest.raises(ValueError, match="device"):
        m(b)
    # ... and after the engine has taken the model (its static answer is cached): looked at on every call
    from graphtrans_amd import engine
    m = model()
    assert engine.eligible(m, b, None) and len(m(b)) == 3
    m.pos_encoder.dropout.p = 0.1
    with pytest.raises(ValueError, match="dropout"):
        m(b)
    m.pos_encoder.dropout.p = 0.0
    m.pos_encoder.pe = m.pos_encoder.pe.cpu()
    with pytest.raises(ValueError, match="device"):
        m(b)
    m.pos_encoder.pe = m.pos_encoder.pe.to(DEV)   # moved back (another pointer): the plan follows it
    assert engine.eligible(m, b, None) and len(m(b)) == 3
    assert engine._plan(m).cm.pe == m.pos_encoder.pe.data_ptr()
