"""freeze_gnn on the fused step (`fused_freeze`, engine.frozen_pattern): with exactly gnn_node frozen the model keeps its one-node
forward and runs a backward that stops behind gnn2transformer's weight gradient (gt_model_batch::gnn_frozen, csrc/model.hip) --
against the module-by-module path under autograd, and against the full fused step whose first stage it is."""
import copy

import pytest
import torch

from test_hip_engine import _args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32_TOL = dict(rtol=1e-4, atol=1e-6)
BF16_TOL = dict(rtol=2e-2, atol=2e-3)


def _model(**kw):
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    args = _args(**kw)
    torch.manual_seed(0)
    model = GNNTransformer(50, ASTNodeEncoder(64, 98, 300, 20), lambda d: torch.nn.Linear(2, d), args).to(DEV)
    with torch.no_grad():  # non-trivial virtual-node embedding and BN statistics
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
        if args.gnn_virtual_node:
            model.gnn_node.virtualnode_embedding.weight.normal_(0, 0.3)
    return model.train()


def _batch():
    from graphtrans_amd import synth
    b = synth.code2_like(B=12, seed=5, num_nodeattributes=300).to(DEV)
    y = torch.randint(0, 50, (12, 5), generator=torch.Generator().manual_seed(1)).to(DEV)
    return b, y


def _loss(model, out, y):
    from graphtrans_amd import losses
    return losses.code2_loss(out, y) if model.max_seq_len is not None else out.float().square().mean()


def _step(model, b, y, seed, keep_grads=False):
    if not keep_grads:
        for p in model.parameters():
            p.grad = None
    torch.manual_seed(seed)
    loss = _loss(model, model(b), y)
    loss.backward()
    return loss.detach().clone()


def _run(model, b, y, fused, seed):
    """loss, gradients of the TRAINABLE parameters, buffers (the harness of test_fused_model_matches_module_path)"""
    model.fused = fused
    loss = _step(model, b, y, seed)
    return loss, {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad}, \
        {n: t.detach().clone() for n, t in model.named_buffers()}


def _assert_pattern(model):
    for n, p in model.named_parameters():
        if n.startswith("gnn_node."):
            assert p.grad is None, n
        else:
            assert p.grad is not None, n


def _close(a, b, tol, what):
    scale = max(1.0, float(a.abs().max()))
    assert torch.allclose(a / scale, b / scale, **tol), (what, float((a - b).abs().max()))


def test_fused_freeze_keeps_the_frozen_model_on_the_fused_path():
    from graphtrans_amd import engine
    b, y = _batch()
    model = _model(freeze_gnn=1, fused_freeze=True)
    model.epoch_callback(0)
    assert engine.eligible(model, b, None)
    _step(model, b, y, 3)
    assert all(p.grad is not None for p in model.parameters())
    for p in model.parameters():
        p.grad = None
    model.epoch_callback(1)
    assert engine.frozen_pattern(model) == "gnn"
    assert engine.eligible(model, b, None)
    _step(model, b, y, 3)
    assert engine.state(model)["plan"].frozen          # the step ran fused, on the plan of a frozen gnn_node
    _assert_pattern(model)
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    model.epoch_callback(2)                            # later epochs change nothing
    assert engine.eligible(model, b, None)
    # the default: a frozen gnn_node leaves the fused path
    off = _model(freeze_gnn=1, fused_freeze=False)
    assert engine.eligible(off, b, None)
    off.epoch_callback(1)
    assert not engine.eligible(off, b, None)
    # every other pattern stays on the module path, flag or not
    for freeze in (lambda m: m.gnn_node.convs[0].requires_grad_(False),
                   lambda m: m.gnn2transformer.weight.requires_grad_(False),
                   lambda m: (m.gnn_node.requires_grad_(False), m.graph_pred_linear_list[0].requires_grad_(False))):
        other = _model(fused_freeze=True)
        assert engine.eligible(other, b, None)
        freeze(other)
        assert engine.frozen_pattern(other) == "other" and not engine.eligible(other, b, None)


PARITY = [dict(), dict(gnn_virtual_node=False, gnn_JK="last"), dict(graph_pooling="last", transformer_norm_input=False), dict(max_seq_len=None),
          dict(gnn_type="gin"), dict(gnn_dropout=0.25), dict(compute_dtype=torch.bfloat16), dict(transformer_activation="gelu")]


@pytest.mark.parametrize("kw", PARITY, ids=[",".join(f"{k}={v}" for k, v in c.items()) or "default" for c in PARITY])
def test_frozen_fused_step_matches_module_path(kw):
    from graphtrans_amd import engine, ops
    bf16 = kw.get("compute_dtype") == torch.bfloat16
    ops.set_matmul_dtype(torch.bfloat16 if bf16 else torch.float32)
    try:
        model = _model(fused_freeze=True, **kw)
        model.gnn_node.requires_grad_(False)
        b, y = _batch()
        assert engine.eligible(model, b, None)
        ref = copy.deepcopy(model)
        init = {n: t.detach().clone() for n, t in model.named_buffers()}
        l0, g0, b0 = _run(ref, b, y, False, 7)
        assert not engine.eligible(ref, b, None)
        l1, g1, b1 = _run(model, b, y, True, 7)
        assert engine.state(model)["plan"].frozen
        _assert_pattern(model), _assert_pattern(ref)
        tol = BF16_TOL if bf16 else F32_TOL
        assert torch.allclose(l0, l1, **tol), (l0, l1)
        assert sorted(g0) == sorted(g1) and all(not n.startswith("gnn_node.") for n in g1)
        for n in g0:
            _close(g0[n], g1[n], tol, n)
        for n in b0:  # BatchNorm running statistics advance identically: the forward is the training forward
            assert torch.allclose(b0[n].float(), b1[n].float(), rtol=1e-4, atol=1e-6), n
        moved = [n for n in b1 if n.startswith("gnn_node.") and n.endswith("running_mean") and not torch.equal(b1[n], init[n])]
        assert moved, "the frozen GNN's BatchNorms still run on batch statistics and advance their running ones"
        # a second backward with the gradients in place accumulates
        model.fused = True
        _step(model, b, y, 7, keep_grads=True)
        _assert_pattern(model)
        atol = 2e-3 if bf16 else 1e-6
        for n, p in model.named_parameters():
            if p.requires_grad:
                scale = max(1.0, float(g1[n].abs().max()))
                assert torch.allclose(p.grad / scale, 2 * g1[n] / scale, rtol=1e-3, atol=atol), (n, float((p.grad - 2 * g1[n]).abs().max()))
    finally:
        ops.set_matmul_dtype(torch.float32)


def test_frozen_backward_is_the_first_stage_of_the_full_one():
    """Same model, batch and seed, fully trainable and frozen, both fused: the forward is the same forward (bit-identical loss) and
    everything above gnn2transformer runs the same launches on the same inputs (bit-identical gradients).  gnn2transformer's own
    gradient comes from the dW-only form of its call (no dX beside it, not forked to the overlap stream): fp32 tolerance."""
    from graphtrans_amd import engine
    b, y = _batch()
    full = _model(fused_freeze=True)
    frozen = copy.deepcopy(full)
    frozen.gnn_node.requires_grad_(False)
    assert engine.eligible(full, b, None) and engine.eligible(frozen, b, None)
    l0, g0, b0 = _run(full, b, y, True, 11)
    l1, g1, b1 = _run(frozen, b, y, True, 11)
    assert not engine.state(full)["plan"].frozen and engine.state(frozen)["plan"].frozen
    assert torch.equal(l0, l1), (l0, l1)
    for n in b0:
        assert torch.equal(b0[n], b1[n]), n
    same = [n for n in g1 if n.startswith("transformer_encoder.") or n.startswith("graph_pred_linear")]
    assert len(same) == len(g1) - 2 and sorted(set(g1) - set(same)) == ["gnn2transformer.bias", "gnn2transformer.weight"]
    assert any("cls_embedding" in n for n in same) and any("norm_input" in n for n in same)
    for n in same:
        assert torch.equal(g0[n], g1[n]), (n, float((g0[n] - g1[n]).abs().max()))
    for n in ("gnn2transformer.weight", "gnn2transformer.bias"):
        _close(g0[n], g1[n], F32_TOL, n)


def test_late_and_reversed_freeze():
    from graphtrans_amd import engine
    b, y = _batch()
    model = _model(fused_freeze=True)
    fresh = copy.deepcopy(model)
    _step(model, b, y, 5)
    assert all(p.grad is not None for p in model.parameters())
    model.gnn_node.requires_grad_(False)               # by hand, after a warm-up step: no callback, no invalidate
    assert engine.eligible(model, b, None)
    _step(model, b, y, 5)
    assert engine.state(model)["plan"].frozen
    _assert_pattern(model)
    model.gnn_node.requires_grad_(True)
    assert engine.eligible(model, b, None)
    _step(model, b, y, 5)
    assert not engine.state(model)["plan"].frozen
    _, want, _ = _run(fresh, b, y, True, 5)
    for n, p in model.named_parameters():
        assert p.grad is not None, n
        _close(want[n], p.grad, F32_TOL, n)


def _pna(**kw):
    from graphtrans_amd import synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.pna_transformer import PNATransformer
    from oracle import reference_math as rm
    torch.manual_seed(11)
    args = rm.default_args(gnn_virtual_node=False, gnn_num_layer=3, gnn_emb_dim=64, gnn_JK="last", gnn_residual=True,
                           gnn_dropout=0.0, d_model=64, nhead=4, dim_feedforward=128, transformer_dropout=0.0,
                           num_encoder_layers=2, transformer_norm_input=True, graph_pooling="cls", max_seq_len=3,
                           aggregators=["mean", "max", "min", "std"], scalers=["identity", "amplification", "attenuation"],
                           deg=torch.tensor([0, 40, 25, 9, 3]), **kw)
    b = synth.code2_like(B=24, seed=2, mean_nodes=20.0, max_nodes=60).to(DEV)
    return PNATransformer(50, ASTNodeEncoder(64, 98, 10030, 20), None, args).to(DEV).train(), b


def test_pna_transformer_frozen_on_the_fused_path():
    from conftest import assert_close
    from graphtrans_amd import engine, losses
    model, b = _pna(freeze_gnn=0, fused_freeze=True)
    assert engine.eligible(model, b, None)
    model.epoch_callback(0)
    assert engine.frozen_pattern(model) == "gnn" and engine.eligible(model, b, None)
    ref = copy.deepcopy(model)
    ref.fused = False
    assert not engine.eligible(ref, b, None)
    outs = []
    for m in (model, ref):
        out = m(b)
        losses.code2_loss(out, b.y_arr).backward()
        outs.append([o.detach() for o in out])
    assert engine.state(model)["plan"].frozen
    for o, r in zip(*outs):
        assert_close(o.cpu(), r.cpu(), what="out")
    for (k, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if k.startswith("gnn_node."):
            assert p.grad is None and q.grad is None, k
        else:
            assert p.grad is not None and q.grad is not None, k
            assert_close(p.grad.cpu(), q.grad.cpu(), what=f"grad {k}")
    off, _ = _pna(freeze_gnn=0)
    off.epoch_callback(0)
    assert not engine.eligible(off, b, None)


@pytest.mark.parametrize("kind", ["gcn", "pna"])
def test_frozen_backward_runs_no_aggregate_backward(kind):
    from graphtrans_amd import _lib, engine, losses
    if kind == "pna":
        model, b = _pna(fused_freeze=True)
        step = lambda: losses.code2_loss(model(b), b.y_arr).backward()
    else:
        model = _model(fused_freeze=True)
        b, y = _batch()
        step = lambda: _step(model, b, y, 2)
    step()   # warm-up: plans, streams, workspaces
    bwd = lambda recs: [n for n, _, _ in recs if n.startswith("gt_aggregate_bwd") or n.startswith("gt_pna_aggregate_bwd")]
    try:
        model.gnn_node.requires_grad_(False)
        assert engine.eligible(model, b, None)
        _lib.profile_enable(1)
        step()
        recs = _lib.profile_records()
        assert engine.state(model)["plan"].frozen
        assert recs, "the forward's aggregate calls are recorded"
        assert not bwd(recs), bwd(recs)
        model.gnn_node.requires_grad_(True)
        _lib.profile_enable(1)
        step()
        assert len(bwd(_lib.profile_records())) >= 1
    finally:
        _lib.profile_enable(0)


def test_frozen_backward_issues_one_gradient_allreduce():
    """One-rank nccl group (the recipe of test_fused_backward_issues_the_gradient_allreduce): the frozen backward is one stage, one
    range of the flat buffer, one collective.  A GradSync built BEFORE the freeze keeps working: it still lists gnn_node's
    parameters, whose gradients stay None, and is handed the same single range."""
    import os
    import socket
    import torch.distributed as dist
    from graphtrans_amd import engine
    from graphtrans_amd.dist import GradSync
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        b, y = _batch()
        for built in ("after", "before"):
            model = _model(fused_freeze=True)
            if built == "before":
                sync = GradSync(model.parameters(), world_size=1, always_reduce=True).attach(model)
            model.gnn_node.requires_grad_(False)
            ref = copy.deepcopy(model)
            _, g0, _ = _run(ref, b, y, True, 3)
            if built == "after":
                sync = GradSync(model.parameters(), world_size=1, always_reduce=True).attach(model)
                assert len(sync.params) == len(g0)
            assert engine.eligible(model, b, None)
            sync.zero()
            torch.manual_seed(3)
            _loss(model, model(b), y).backward()
            assert sync._flat_used and len(sync._pending) == 1, (built, len(sync._pending))
            sync.finish()
            torch.cuda.synchronize()
            _assert_pattern(model)
            for n, p in model.named_parameters():
                if p.requires_grad:
                    assert torch.equal(p.grad, g0[n]), (built, n)
    finally:
        dist.destroy_process_group()


def test_fused_adamw_over_frozen_fused_steps():
    from graphtrans_amd import engine
    from graphtrans_amd.optim import FusedAdamW
    b, y = _batch()
    model = _model(fused_freeze=True)
    model.gnn_node.requires_grad_(False)
    opt = FusedAdamW(model.parameters(), lr=1e-3, max_grad_norm=1.0)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    for it in range(2):
        assert engine.eligible(model, b, None)
        _step(model, b, y, 20 + it)
        assert engine.state(model)["plan"].frozen
        opt.step()
    torch.cuda.synchronize()
    sq = sum(float(p.grad.double().square().sum()) for p in model.parameters() if p.requires_grad)
    _assert_pattern(model)
    assert abs(float(opt.last_grad_norm) - sq ** 0.5) <= 1e-5 * sq ** 0.5, (float(opt.last_grad_norm), sq ** 0.5)
    for n, p in model.named_parameters():
        if n.startswith("gnn_node."):
            assert torch.equal(p.detach(), before[n]), n
        else:
            assert not torch.equal(p.detach(), before[n]), n


ROWS = [dict(max_input_len=60), dict(gnn_JK="last", max_input_len=100)]


@pytest.mark.parametrize("kw", ROWS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c in ROWS])
def test_frozen_weight_gradient_reads_the_token_rows_through_the_row_map(kw):
    """The shapes of test_gnn2transformer_writes_the_token_rows_itself (>= 1024 node rows, d_model 128): gnn2transformer's epilogue
    wrote the token rows through a row map, so its dW-only backward call reads the token-row gradient through that map (JK = cat: with
    the row operand in two halves), truncated graphs included.  Against the full fused step -- the same launches above gnn2transformer,
    bit for bit; its own gradient within the suite's 1e-4 fp32 bar, relative L2 (another split of the same sum over the rows) -- and
    against the module path, which unpads with gt_seq_scatter, under that test's bound (gate flips between two fp32 evaluations of a
    3 k-row batch: relative L2 below 3e-2 per tensor, small tensors measured against the typical norm)."""
    from graphtrans_amd import engine, synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    args = _args(gnn_emb_dim=128, d_model=128, dim_feedforward=256, transformer_dropout=0.0, fused_freeze=True, **kw)
    torch.manual_seed(0)
    full = GNNTransformer(50, ASTNodeEncoder(128, 98, 300, 20), lambda d: torch.nn.Linear(2, d), args).to(DEV).train()
    b = synth.code2_like(B=24, seed=21, num_nodeattributes=300).to(DEV)
    assert b.x.shape[0] >= 1024
    y = torch.randint(0, 50, (24, 3), generator=torch.Generator().manual_seed(2)).to(DEV)
    model = copy.deepcopy(full)
    model.gnn_node.requires_grad_(False)
    ref = copy.deepcopy(model)
    assert engine.eligible(full, b, None) and engine.eligible(model, b, None)
    l2, g2, _ = _run(full, b, y, True, 5)
    l1, g1, _ = _run(model, b, y, True, 5)
    l0, g0, _ = _run(ref, b, y, False, 5)
    assert engine.state(model)["plan"].frozen
    _assert_pattern(model), _assert_pattern(ref)
    assert torch.equal(l1, l2)
    for n in g1:
        if n.startswith("gnn2transformer."):
            err = float((g1[n].double() - g2[n].double()).norm() / g2[n].double().norm())
            print(n, "rel L2 against the full fused step", err)
            assert err < 1e-4, (n, err)
        else:
            assert torch.equal(g1[n], g2[n]), n
    assert torch.allclose(l0, l1, rtol=1e-3, atol=1e-5), (l0, l1)
    floor = 1e-2 * float(torch.stack([g0[n].double().norm() for n in g0]).median())
    worst = max(((float((g0[n].double() - g1[n].double()).norm() / g0[n].double().norm().clamp_min(floor)), n) for n in g0))
    print("worst rel L2 against the module path", worst)
    assert worst[0] < 3e-2, worst


def test_frozen_backward_accepts_the_other_stage_bits(monkeypatch):
    """gt_model_backward with gnn_frozen: stage 1 is the whole backward; a staged caller's bits 1 and 2 are accepted afterwards and do
    nothing (same gradients as the one call with 7), and asking for them before stage 1 is the usual stage-order error."""
    from graphtrans_amd import _lib, engine
    b, y = _batch()
    model = _model(fused_freeze=True)
    model.gnn_node.requires_grad_(False)
    _, want, _ = _run(copy.deepcopy(model), b, y, True, 13)
    lib = _lib.lib()
    real = lib.gt_model_backward
    seen = []

    def staged(m, ctx, dlogits, grads, barena, stages, stream):
        early = real(m, ctx, dlogits, grads, barena, 6, stream)   # refused by the argument check: nothing is enqueued
        rcs = [real(m, ctx, dlogits, grads, barena, s, stream) for s in (1, 2, 4)]
        seen.append((stages, early, rcs))
        return max(rcs)

    monkeypatch.setattr(lib, "gt_model_backward", staged)
    _, got, _ = _run(model, b, y, True, 13)
    assert engine.state(model)["plan"].frozen
    assert len(seen) == 1 and seen[0][0] == 7 and seen[0][1] != 0 and seen[0][2] == [0, 0, 0], seen
    _assert_pattern(model)
    torch.cuda.synchronize()
    for n in want:
        assert torch.equal(got[n], want[n]), n
