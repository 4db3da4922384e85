"""The GNN baseline model (graphtrans_amd/models/gnn.py) on the GPU, after the pattern and with the tolerances of tests/test_hip_engine.py:
the fused step (the whole-model driver's read-out mode, csrc/model.hip) against the module path (gnn_node -> ops.graph_pool -> heads) on
the same parameters, batch and dropout seed; both against the float64 statement of tests/test_gnn_baseline_host.py (which that file
pins to the reference's own models/gnn.py); and against tests/golden/gnn_baseline_ref.json, recorded from the reference.
"""
import copy
from types import SimpleNamespace

import pytest
import torch

import test_hip_configs as thc
from test_gnn_baseline_host import fixture_batch, load_fixture, statement_run
from test_hip_configs import BOUNDS, check_grads, precision_report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32_TOL = dict(rtol=1e-4, atol=1e-6)      # tests/test_hip_engine.py: on max-scaled gradients, exact-fp32 GEMMs
BF16_TOL = dict(rtol=2e-2, atol=2e-3)     # ... with ops.set_matmul_dtype(torch.bfloat16)


def _gargs(**kw):
    a = dict(gnn_virtual_node=True, gnn_num_layer=3, gnn_emb_dim=64, gnn_JK="last", gnn_dropout=0.0, gnn_residual=False, gnn_type="gcn",
             graph_pooling="mean", max_seq_len=3, model_type="gnn")
    a.update(kw)
    return SimpleNamespace(**a)


def _build(feat, args, dev=DEV):
    """-> (model, batch, loss(out)): Code2-style (ASTNodeEncoder, Linear edge encoder, stacked heads), Molpcba-style (AtomEncoder /
    BondEncoder, one 16-way head), TU-style (nn.Linear node encoder, the zero edge encoder)"""
    from graphtrans_amd import losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder, AtomEncoder, BondEncoder
    from graphtrans_amd.models.gnn import GNN
    D = args.gnn_emb_dim
    torch.manual_seed(0)
    if feat == "ast":
        model = GNN(50, ASTNodeEncoder(D, 98, 300, 20), lambda d: torch.nn.Linear(2, d), args)
        # sum pooling: graphs of 11 .. 24 rows.  Summed over the ~105 rows of the default batch the pooled rows are O(100), the
        # cross-entropy saturates (loss 112) and BOTH paths sit 1e-5 (max-scaled) from the float64 statement -- 5 to 11 x the 1e-6
        # bar between them is then rounding, not a difference of the paths (measured: module 1.0e-5 / fused 7.2e-6 from float64 on
        # convs.2.linear.bias).  The bar is for O(1) activations: the batch is sized for it, the bar stays.
        small = dict(mean_nodes=14.0, max_nodes=24) if args.graph_pooling == "sum" else {}
        b = synth.code2_like(B=12, seed=5, num_nodeattributes=300, **small).to(dev)
        y = torch.randint(0, 50, (12, 5), generator=torch.Generator().manual_seed(1)).to(dev)
        loss = (lambda out: losses.code2_loss(out, y)) if args.max_seq_len is not None else (lambda out: out.float().square().mean())
    elif feat == "mol":
        args.max_seq_len = None
        model = GNN(16, AtomEncoder(D), lambda d: BondEncoder(d), args)
        b = synth.molpcba_like(B=24, seed=4).to(dev)
        g = torch.Generator().manual_seed(4)
        y = (torch.rand(24, 16, generator=g) > 0.5).float()
        y[torch.rand(24, 16, generator=g) < 0.2] = float("nan")
        y = y.to(dev)
        loss = lambda out: losses.mol_loss(out, y)
    else:
        args.max_seq_len = None
        model = GNN(2, torch.nn.Linear(37, D), lambda d: (lambda _e: 0), args)   # dataset/tud.py:65-71
        b = synth.nci1_like(B=16, seed=3).to(dev)
        loss = lambda out: losses.tud_loss(out, b.y)
    model = model.to(dev)
    with torch.no_grad():   # non-trivial BatchNorm affine / biases and virtual-node embedding
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
        if args.gnn_virtual_node:
            model.gnn_node.virtualnode_embedding.weight.normal_(0, 0.3)
    return model.train(), b, loss


def _run(model, b, loss_of, fused, seed, keep_grads=False):
    model.fused = fused
    if not keep_grads:
        for p in model.parameters():
            p.grad = None
    torch.manual_seed(seed)
    out = model(b)
    loss = loss_of(out)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, \
        {n: t.detach().clone() for n, t in model.named_buffers()}


def _close(a, b, tol, what):
    scale = max(1.0, float(a.abs().max()))
    assert torch.allclose(a / scale, b / scale, **tol), (what, float((a - b).abs().max()))


CASES = [dict(), dict(gnn_virtual_node=False), dict(gnn_type="gin"), dict(gnn_type="gin", gnn_virtual_node=False),
         dict(graph_pooling="sum"), dict(graph_pooling="max"), dict(graph_pooling="max", gnn_type="gin", gnn_virtual_node=False),
         dict(graph_pooling="sum", gnn_type="gin"),
         dict(gnn_residual=True), dict(gnn_dropout=0.25), dict(gnn_dropout=0.25, graph_pooling="max", gnn_residual=True),
         dict(max_seq_len=None), dict(max_seq_len=None, graph_pooling="max", gnn_virtual_node=False),
         dict(feat="mol", gnn_type="gin"), dict(feat="mol", graph_pooling="max"), dict(feat="tud", gnn_virtual_node=False, graph_pooling="sum"),
         dict(feat="tud", gnn_type="gin", graph_pooling="max"),
         dict(bf16=True), dict(bf16=True, feat="mol", gnn_type="gin", graph_pooling="max")]


@pytest.mark.parametrize("kw", CASES, ids=[",".join(f"{k}={v}" for k, v in c.items()) or "default" for c in CASES])
def test_fused_gnn_matches_module_path(kw):
    from graphtrans_amd import engine, ops
    kw = dict(kw)
    feat, bf16 = kw.pop("feat", "ast"), kw.pop("bf16", False)
    ops.set_matmul_dtype(torch.bfloat16 if bf16 else torch.float32)
    try:
        model, b, loss_of = _build(feat, _gargs(**kw))
        assert engine.eligible(model, b, None)
        l0, g0, b0 = _run(copy.deepcopy(model), b, loss_of, False, 7)
        l1, g1, b1 = _run(model, b, loss_of, True, 7)
        assert engine.state(model)["plan"].readout in (1, 2, 3)   # the driver's read-out mode ran
        tol = BF16_TOL if bf16 else F32_TOL
        assert torch.allclose(l0, l1, **tol), (l0, l1)
        assert set(g0) == set(g1)
        for n in g0:
            _close(g0[n], g1[n], tol, n)
        for n in b0:   # BatchNorm running statistics advance identically
            assert torch.allclose(b0[n].float(), b1[n].float(), rtol=1e-4, atol=1e-6), n
        # a second backward onto the gradients in place accumulates: 2 x (same seed, same dropout masks)
        _run(model, b, loss_of, True, 7, keep_grads=True)
        atol = 2e-3 if bf16 else 1e-6
        for n, p in model.named_parameters():
            scale = max(1.0, float(g1[n].abs().max()))
            assert torch.allclose(p.grad / scale, 2 * g1[n] / scale, rtol=1e-3, atol=atol), (n, float((p.grad - 2 * g1[n]).abs().max()))
    finally:
        ops.set_matmul_dtype(torch.float32)


@pytest.mark.parametrize("pooling", ["sum", "mean", "max"])
def test_fused_gnn_eval_matches_module_path(pooling):
    from graphtrans_amd import engine
    model, b, _ = _build("ast", _gargs(graph_pooling=pooling))
    model.eval()
    with torch.no_grad():
        assert engine.eligible(model, b, None)
        model.fused = True
        a = [t.clone() for t in model(b)]
        model.fused = False
        c = model(b)
    assert len(a) == len(c) == 3
    for u, v in zip(a, c):
        assert torch.allclose(u, v, rtol=1e-4, atol=1e-5)


def test_module_path_routing():
    """JK = sum, a perturbation and one frozen parameter leave the fused path; the module path runs them.  d loss / d perturb against the
    float64 statement."""
    from graphtrans_amd import engine
    model, b, loss_of = _build("ast", _gargs(gnn_JK="sum"))
    assert not engine.eligible(model, b, None)
    assert len(model(b)) == 3
    model, b, loss_of = _build("ast", _gargs())
    next(model.gnn_node.convs[1].parameters()).requires_grad_(False)
    assert not engine.eligible(model, b, None)
    loss_of(model(b)).backward()
    assert model.graph_pred_linear_list[0].weight.grad is not None
    # perturb
    args = _gargs(graph_pooling="max", max_seq_len=None)
    model, b, _ = _build("ast", args)
    N = b.batch.numel()
    perturb = (torch.randn(N, 64, generator=torch.Generator().manual_seed(2)) * 0.1).to(DEV).requires_grad_(True)
    assert engine.eligible(model, b, None) and not engine.eligible(model, b, perturb)
    sq = lambda out: out.square().mean()
    out = model(b, perturb)
    sq(out).backward()
    ref_out, _, ref_g, ref_dp = statement_run(model.state_dict(), args, b.to("cpu"), sq, torch.float64, perturb=perturb)
    assert float((out.detach().cpu().double() - ref_out.detach()).abs().max()) <= 1e-4
    scale = max(float(ref_dp.abs().max()), 1e-30)
    assert float((perturb.grad.cpu().double() - ref_dp).abs().max()) / scale <= 1e-4
    _close(ref_g["graph_pred_linear.weight"].float(), model.graph_pred_linear.weight.grad.cpu(), F32_TOL, "head")


# ---- against the float64 statement ------------------------------------------------------------------------------------------------
def _oracle_run(model, args, b, loss_of, dtype=torch.float32):
    """test_hip_configs.oracle_run for this model: the statement of tests/test_gnn_baseline_host.py instead of rm.gnn_transformer"""
    return statement_run(model.state_dict(), args, b, loss_of, dtype)


@pytest.mark.parametrize("case", ["gcn-virtual-mean", "gin-max"])
def test_fused_gnn_fp32_vs_float64_statement(case, monkeypatch):
    """Exact-fp32 mode, <= 16 graphs: logits within 1e-4 elementwise, every gradient through test_hip_configs.check_grads with that
    file's fp32_noise model run on THIS model's oracle, BOUNDS["fp32"] on the precision report."""
    from graphtrans_amd import engine, losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder, AtomEncoder, BondEncoder
    from graphtrans_amd.models.gnn import GNN
    from oracle import reference_math as rm
    monkeypatch.setattr(thc, "oracle_run", _oracle_run)   # fp32_noise calls it: same perturbations, same quantile, this model's math
    torch.manual_seed(5)
    if case == "gcn-virtual-mean":
        args = _gargs(max_seq_len=5)
        model = GNN(50, ASTNodeEncoder(64, 98, 300, 20), lambda d: torch.nn.Linear(2, d), args)
        b = synth.code2_like(B=16, seed=5, num_nodeattributes=300, num_vocab=50)
        oloss, hloss = (lambda out: rm.code2_loss(out, b.y_arr)), (lambda out, bd: losses.code2_loss(out, bd.y_arr))
    else:
        args = _gargs(gnn_type="gin", gnn_virtual_node=False, graph_pooling="max", max_seq_len=None)
        model = GNN(16, AtomEncoder(64), lambda d: BondEncoder(d), args)
        b = synth.molpcba_like(B=16, seed=5, num_tasks=16)
        oloss, hloss = (lambda out: rm.mol_loss(out, b.y)), (lambda out, bd: losses.mol_loss(out, bd.y))
    ref_out, ref_loss, ref_g = _oracle_run(model, args, b, oloss, torch.float64)
    noise = thc.fp32_noise(model, args, b, oloss, ref_g)
    _, o32_loss, o32_g = _oracle_run(model, args, b, oloss, torch.float32)
    o32 = precision_report(o32_g, o32_loss, ref_g, ref_loss)
    assert engine.eligible(model.to(DEV).train(), b.to(DEV), None)
    outs, loss, grads = thc.hip_run(model, b, hloss, torch.float32)
    refs = [o.detach() for o in (ref_out if isinstance(ref_out, (list, tuple)) else [ref_out])]
    top = max(float(r.abs().max()) for r in refs)
    lerr = max(float((o.double() - r).abs().max()) for o, r in zip(outs, refs))
    rep = precision_report(grads, loss, ref_g, ref_loss)
    print(f"\n[gnn {case}] logits: max |err| {lerr:.2e} (largest logit {top:.2f}); loss rel {rep['loss_rel_err']:.2e}; grad rel-L2 worst "
          f"{rep['grad_rel_l2_worst']:.2e} ({rep['grad_rel_l2_worst_param']}) median {rep['grad_rel_l2_median']:.2e}; fp32 oracle itself: "
          f"worst {o32['grad_rel_l2_worst']:.2e} median {o32['grad_rel_l2_median']:.2e}")
    assert 0.1 <= top <= 100.0, top     # inputs of O(1): the absolute bar below means what it says
    assert lerr <= 1e-4, lerr
    bound = BOUNDS["fp32"]
    assert rep["loss_rel_err"] <= bound["loss"] and rep["grad_rel_l2_worst"] <= bound["worst"], rep
    assert rep["grad_rel_l2_median"] <= max(bound["median"], 3.0 * o32["grad_rel_l2_median"]), (rep, o32)   # (as that file applies it)
    check_grads(grads, ref_g, noise, what=f"gnn {case} fp32")


def test_gnn_equals_the_recorded_reference():
    """tests/golden/gnn_baseline_ref.json (the reference's own fp32 run of models/gnn.py) loaded into GNN: logits within 1e-4, gradients
    within check_grads' bars (noise 0: its base of 1e-3 of the tensor's largest entry) against the RECORDED fp32 gradients.  Both data
    paths: the module path and, where the engine takes it, the fused step."""
    from graphtrans_amd import engine
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn import GNN
    for c in load_fixture():
        D = c["args"].gnn_emb_dim
        if c["feat"] == "code2":
            ne, ee = ASTNodeEncoder(D, 11, 13, 20), (lambda d: torch.nn.Linear(2, d))
        else:
            ne, ee = torch.nn.Linear(6, D), (lambda d: (lambda _e: 0))
        model = GNN(5, ne, ee, c["args"])
        model.load_state_dict(c["sd"], strict=True)
        model = model.to(DEV).train()
        b = fixture_batch(c["inputs"]).to(DEV)
        for fused in (False, True):
            model.fused = fused
            assert engine.eligible(model, b, None) == fused, (c["name"], fused)
            loss, grads, _ = _run(model, b, lambda out: out.square().mean(), fused, 0)
            model.fused = fused
            with torch.no_grad():
                out = model(b)   # (training mode, p = 0: the same forward; the buffers are not part of the comparison)
            assert float((out.cpu() - c["logits"]).abs().max()) <= 1e-4, (c["name"], fused)
            check_grads({k: v.cpu() for k, v in grads.items()}, {k: v.double() for k, v in c["grads"].items()},
                        {k: 0.0 for k in c["grads"]}, what=f"recorded reference {c['name']} fused={fused}")


def test_fused_gnn_backward_issues_the_gradient_allreduce():
    """dist.GradSync.attach on a one-rank nccl group: the staged backward hands the three ranges {heads | message passing | input
    encoder} to RCCL; the gradients are unchanged."""
    import os
    import socket
    import torch.distributed as dist
    from graphtrans_amd.dist import GradSync
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        model, b, loss_of = _build("ast", _gargs(graph_pooling="max"))
        _, g0, _ = _run(copy.deepcopy(model), b, loss_of, True, 3)
        sync = GradSync(model.parameters(), world_size=1, always_reduce=True).attach(model)
        sync.zero()
        torch.manual_seed(3)
        loss_of(model(b)).backward()
        assert sync._flat_used and len(sync._pending) == 3
        sync.finish()
        torch.cuda.synchronize()
        for n, p in model.named_parameters():
            assert torch.equal(p.grad, g0[n]), n
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("fused", [True, False], ids=["fused-FusedAdamW", "modules-torchAdamW"])
def test_five_training_steps(fused):
    """Five optimizer steps, a different batch every step: the fused GNN under FusedAdamW, and the module path under torch.optim.AdamW.
    The two trajectories are NOT compared with each other, nor at their end: tests/test_hip_training_steps.py says why (Adam's first
    update is lr * sign(g): rounding noise in a gradient whose exact value is 0 becomes a parameter difference of 2 * lr) and has no
    fused-vs-module tolerance to import -- it holds each run, step by step, to the float64 oracle at the run's OWN state.  So does this
    test, with that file's bars: the loss within 1e-4 (relative), every gradient through check_grads (noise 0: its base of 1e-3, the
    98 % quantile and the capped tail that let ONE flipped ReLU gate pass -- measured here: with the batch of seed 22 the fused run's
    layer-1 tensors sit 2e-4 .. 8e-4 of their largest entry from float64 at an identical loss, one step later the module path's do,
    every other step both are at 1e-6), and FusedAdamW against a float64 torch.optim.AdamW twin fed the run's own gradients
    (`_twin_check` of that file: 1e-5 relative, 1e-7 / 1e-8 / 1e-10 absolute; the clipping norm to 1e-5)."""
    import torch.nn.functional as F
    from test_hip_training_steps import CLIP, LR, WD, _twin_check

    from graphtrans_amd import engine, losses, synth
    from graphtrans_amd.optim import FusedAdamW
    args = _gargs()
    model, _, _ = _build("ast", args)
    model.fused = fused
    names = [k for k, _ in model.named_parameters()]
    params = [p for _, p in model.named_parameters()]
    if fused:
        opt = FusedAdamW(model.parameters(), lr=LR, weight_decay=WD, max_grad_norm=CLIP)
        tparams = [p.detach().cpu().double().clone().requires_grad_(True) for p in params]
        twin = torch.optim.AdamW(tparams, lr=LR, weight_decay=WD)
    else:
        opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD)
    dev, worst = {}, 0.0
    for step in range(5):
        bc = synth.code2_like(B=12, seed=20 + step, num_nodeattributes=300)
        yc = torch.randint(0, 50, (12, 5), generator=torch.Generator().manual_seed(step))
        _, l64, g64 = statement_run(model.state_dict(), args, bc, lambda out: sum(F.cross_entropy(p, yc[:, i]) for i, p in enumerate(out)) / len(out),
                                    torch.float64)
        b, y = copy.copy(bc).to(DEV), yc.to(DEV)
        assert engine.eligible(model, b, None) == fused, f"step {step}"
        loss, grads, _ = _run(model, b, lambda out: losses.code2_loss(out, y), fused, step)
        lerr = abs(float(loss) - float(l64)) / abs(float(l64))
        worst = max(worst, lerr)
        assert lerr <= 1e-4, (step, float(loss), float(l64))
        check_grads({k: v.cpu() for k, v in grads.items()}, g64, {k: 0.0 for k in g64}, what=f"gnn step {step} {'fused' if fused else 'modules'}")
        if fused:
            for q, p in zip(tparams, params):
                q.grad = p.grad.detach().cpu().double()
            tnorm = torch.nn.utils.clip_grad_norm_(tparams, CLIP)
            opt.step()
            twin.step()
            assert abs(float(opt.last_grad_norm) - float(tnorm)) / float(tnorm) <= 1e-5, step
            _twin_check(opt, twin, tparams, names, dev)
        else:
            torch.nn.utils.clip_grad_norm_(model.parameters(), CLIP)
            opt.step()
    torch.cuda.synchronize()
    print(f"\n[gnn, five steps, {'fused + FusedAdamW' if fused else 'modules + torch AdamW'}] worst loss rel err {worst:.1e}; deviation from the "
          "float64 twin: " + (", ".join(f"{k} {v:.1e}" for k, v in dev.items()) or "-"))
