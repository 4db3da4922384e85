"""The PNA baseline model (graphtrans_amd/models/pna.py) on the GPU, after the pattern and with the tolerances of
tests/test_hip_gnn_baseline.py: the fused step (the whole-model driver's read-out mode with the PNA stack and the head kinds of
csrc/mlp_heads.hip) against the module path (pna_module -> ops.graph_pool -> ops.head_mlp | ops.linear + ops.head_group) on the same
parameters, batch and dropout seed; both against the float64 statement of tests/test_pna_baseline_host.py (which that file pins to the
reference's own models/pna.py); and against tests/golden/pna_baseline_ref.json, recorded from the reference.
"""
import copy
from types import SimpleNamespace

import pytest
import torch

import test_hip_configs as thc
from test_gnn_baseline_host import fixture_batch
from test_hip_configs import BOUNDS, check_grads, precision_report
from test_hip_gnn_baseline import BF16_TOL, F32_TOL, _close, _run
from test_pna_baseline_host import AGGS, SCALERS, fixture_loss, load_fixture, statement_run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEG = [0, 5, 9, 7, 3, 1, 0, 2]   # in-degree histogram (tests/test_hip_pna.py)


def _pargs(**kw):
    a = dict(gnn_num_layer=3, gnn_emb_dim=64, gnn_dropout=0.0, gnn_residual=True, graph_pooling="mean", max_seq_len=3, model_type="pna",
             aggregators=list(AGGS), scalers=list(SCALERS), deg=torch.tensor(DEG))
    a.update(kw)
    return SimpleNamespace(**a)


def _build(feat, args, dev=DEV, num_tasks=50):
    """-> (model, batch, loss(out)): Code2-style (ASTNodeEncoder, position heads), Molpcba-style (AtomEncoder, narrow MLP, 16 tasks),
    TU-style (nn.Linear node encoder, narrow MLP)"""
    from graphtrans_amd import losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder, AtomEncoder
    from graphtrans_amd.models.pna import PNANet
    D = args.gnn_emb_dim
    torch.manual_seed(0)
    if feat == "ast":
        model = PNANet(num_tasks, ASTNodeEncoder(D, 98, 300, 20), None, args)
        small = dict(mean_nodes=14.0, max_nodes=24) if args.graph_pooling == "sum" else {}   # (pooled rows of O(1): test_hip_gnn_baseline._build)
        b = synth.code2_like(B=12, seed=5, num_nodeattributes=300, **small).to(dev)
        y = torch.randint(0, num_tasks, (12, 5), generator=torch.Generator().manual_seed(1)).to(dev)
        loss = (lambda out: losses.code2_loss(out, y)) if args.max_seq_len is not None else (lambda out: out.float().square().mean())
    elif feat == "mol":
        args.max_seq_len = None
        model = PNANet(16, AtomEncoder(D), None, args)
        b = synth.molpcba_like(B=24, seed=4).to(dev)
        g = torch.Generator().manual_seed(4)
        y = (torch.rand(24, 16, generator=g) > 0.5).float()
        y[torch.rand(24, 16, generator=g) < 0.2] = float("nan")
        y = y.to(dev)
        loss = lambda out: losses.mol_loss(out, y)
    else:
        args.max_seq_len = None
        model = PNANet(2, torch.nn.Linear(37, D), None, args)   # dataset/tud.py:65
        b = synth.nci1_like(B=16, seed=3).to(dev)
        loss = lambda out: losses.tud_loss(out, b.y)
    model = model.to(dev)
    with torch.no_grad():   # non-trivial BatchNorm affine / biases
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    return model.train(), b, loss


CASES = [dict(), dict(gnn_dropout=0.25), dict(graph_pooling="sum"), dict(graph_pooling="max"), dict(feat="mol"), dict(feat="tud"),
         dict(aggregators=["mean", "max", "min", "std", "sum", "var"]), dict(bf16=True)]


@pytest.mark.parametrize("kw", CASES, ids=[",".join(f"{k}={v}" for k, v in c.items()) or "default" for c in CASES])
def test_fused_pna_matches_module_path(kw):
    from graphtrans_amd import engine, ops
    kw = dict(kw)
    feat, bf16 = kw.pop("feat", "ast"), kw.pop("bf16", False)
    ops.set_matmul_dtype(torch.bfloat16 if bf16 else torch.float32)
    try:
        model, b, loss_of = _build(feat, _pargs(**kw))
        assert engine.eligible(model, b, None)
        l0, g0, b0 = _run(copy.deepcopy(model), b, loss_of, False, 7)
        l1, g1, b1 = _run(model, b, loss_of, True, 7)
        plan = engine.state(model)["plan"]
        assert plan.readout in (1, 2, 3) and plan.head_kind == (2 if feat == "ast" else 1)   # the driver's read-out mode and head kind ran
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


def test_fused_pna_is_reproducible():
    model, b, loss_of = _build("ast", _pargs(gnn_dropout=0.25))
    _, g0, _ = _run(model, b, loss_of, True, 11)
    _, g1, _ = _run(model, b, loss_of, True, 11)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


@pytest.mark.parametrize("msl", [3, None], ids=["heads", "mlp"])
def test_fused_pna_eval_matches_module_path(msl):
    from graphtrans_amd import engine
    model, b, _ = _build("ast", _pargs(max_seq_len=msl, graph_pooling="max"))
    model.eval()
    with torch.no_grad():
        assert engine.eligible(model, b, None)
        model.fused = True
        a = model(b)
        a = [t.clone() for t in a] if msl else [a.clone()]
        model.fused = False
        c = model(b)
        c = list(c) if msl else [c]
    assert len(a) == len(c) == (msl or 1)
    for u, v in zip(a, c):
        assert torch.allclose(u, v, rtol=1e-4, atol=1e-5)


def test_module_path_routing():
    """One frozen parameter, a model without the residual connection and a perturbation without `fused_flag` leave the fused path; the
    module path runs them.  With `fused_flag` the perturbation stays fused and d loss / d perturb agrees with the module path's."""
    from graphtrans_amd import engine
    model, b, loss_of = _build("ast", _pargs())
    next(model.pna_module.layers[1].parameters()).requires_grad_(False)
    assert not engine.eligible(model, b, None)
    loss_of(model(b)).backward()
    assert model.graph_pred_linear_list[0][2].weight.grad is not None and model.graph_pred_linear_list[2][0].bias.grad is not None
    model, b, loss_of = _build("ast", _pargs(gnn_residual=False))
    assert not engine.eligible(model, b, None)
    assert len(model(b)) == 3
    # D = 40: towers of 10 columns (not a multiple of 4) and position heads of a width the grouped kernel does not take
    model, b, loss_of = _build("ast", _pargs(gnn_emb_dim=40))
    assert not engine.eligible(model, b, None)
    out = model(b)
    assert len(out) == 3 and tuple(out[0].shape) == (12, 50)
    # perturb
    for msl in (3, None):
        model, b, _ = _build("ast", _pargs(max_seq_len=msl))
        N = b.batch.numel()
        p0 = (torch.randn(N, 64, generator=torch.Generator().manual_seed(2)) * 0.1).to(DEV)
        sq = lambda out: sum(o.square().mean() for o in (out if msl else [out]))
        pm = p0.clone().requires_grad_(True)
        assert engine.eligible(model, b, None) and not engine.eligible(model, b, pm)
        sq(model(b, pm)).backward()
        gm = {n: p.grad.clone() for n, p in model.named_parameters()}
        model.fused_flag = True
        engine.invalidate(model)
        for p in model.parameters():
            p.grad = None
        pf = p0.clone().requires_grad_(True)
        assert engine.eligible(model, b, pf)
        sq(model(b, pf)).backward()
        _close(pm.grad, pf.grad, F32_TOL, "d perturb")
        for n, p in model.named_parameters():
            _close(gm[n], p.grad, F32_TOL, n)


# ---- against the float64 statement ------------------------------------------------------------------------------------------------
def _oracle_run(model, args, b, loss_of, dtype=torch.float32):
    """test_hip_configs.oracle_run for this model; the gradients under the names named_parameters() uses (the shared node encoder once)"""
    out, loss, grads = statement_run(model.state_dict(), args, b, loss_of, dtype)
    names = {k for k, _ in model.named_parameters()}
    return out, loss, {k: v for k, v in grads.items() if k in names}


def _vs_float64(case, model, args, b, oloss, hloss, fused, monkeypatch):
    from graphtrans_amd import engine
    monkeypatch.setattr(thc, "oracle_run", _oracle_run)   # fp32_noise calls it: same perturbations, same quantile, this model's math
    ref_out, ref_loss, ref_g = _oracle_run(model, args, b, oloss, torch.float64)
    noise = thc.fp32_noise(model, args, b, oloss, ref_g)
    _, o32_loss, o32_g = _oracle_run(model, args, b, oloss, torch.float32)
    o32 = precision_report(o32_g, o32_loss, ref_g, ref_loss)
    model.fused = fused
    assert engine.eligible(model.to(DEV).train(), b.to(DEV), None) == fused
    outs, loss, grads = thc.hip_run(model, b, hloss, torch.float32)
    refs = [o.detach() for o in (ref_out if isinstance(ref_out, (list, tuple)) else [ref_out])]
    top = max(float(r.abs().max()) for r in refs)
    lerr = max(float((o.double() - r).abs().max()) for o, r in zip(outs, refs))
    rep = precision_report(grads, loss, ref_g, ref_loss)
    print(f"\n[pna {case} fused={fused}] logits: max |err| {lerr:.2e} (largest logit {top:.2f}); loss rel {rep['loss_rel_err']:.2e}; grad rel-L2 "
          f"worst {rep['grad_rel_l2_worst']:.2e} ({rep['grad_rel_l2_worst_param']}) median {rep['grad_rel_l2_median']:.2e}; fp32 oracle itself: "
          f"worst {o32['grad_rel_l2_worst']:.2e} median {o32['grad_rel_l2_median']:.2e}")
    assert 0.1 <= top <= 100.0, top     # inputs of O(1): the absolute bar below means what it says
    assert lerr <= 1e-4, lerr
    bound = BOUNDS["fp32"]
    assert rep["loss_rel_err"] <= bound["loss"] and rep["grad_rel_l2_worst"] <= bound["worst"], rep
    assert rep["grad_rel_l2_median"] <= max(bound["median"], 3.0 * o32["grad_rel_l2_median"]), (rep, o32)   # (as that file applies it)
    check_grads(grads, ref_g, noise, what=f"pna {case} fused={fused} fp32")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "modules"])
@pytest.mark.parametrize("case", ["heads-mean", "mlp-max"])
def test_pna_fp32_vs_float64_statement(case, fused, monkeypatch):
    """Exact-fp32 mode, 16 graphs: logits within 1e-4 elementwise, every gradient through test_hip_configs.check_grads with that file's
    fp32_noise model run on THIS model's oracle, BOUNDS["fp32"] on the precision report.  Both data paths."""
    from graphtrans_amd import losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder, AtomEncoder
    from graphtrans_amd.models.pna import PNANet
    from oracle import reference_math as rm
    torch.manual_seed(5)
    if case == "heads-mean":
        args = _pargs(max_seq_len=5)
        model = PNANet(50, ASTNodeEncoder(64, 98, 300, 20), None, args)
        b = synth.code2_like(B=16, seed=5, num_nodeattributes=300, num_vocab=50)
        oloss, hloss = (lambda out: rm.code2_loss(out, b.y_arr)), (lambda out, bd: losses.code2_loss(out, bd.y_arr))
    else:
        args = _pargs(graph_pooling="max", max_seq_len=None)
        model = PNANet(16, AtomEncoder(64), None, args)
        b = synth.molpcba_like(B=16, seed=5, num_tasks=16)
        oloss, hloss = (lambda out: rm.mol_loss(out, b.y)), (lambda out, bd: losses.mol_loss(out, bd.y))
    _vs_float64(case, model, args, b, oloss, hloss, fused, monkeypatch)


def test_pna_real_shape_vs_float64_statement(monkeypatch):
    """The shape of configs/code2/pna/base.yml on 16 graphs: D = 272, 4 layers, five heads x 5002, mean pooling, on the fused step"""
    from graphtrans_amd import losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.pna import PNANet
    from oracle import reference_math as rm
    torch.manual_seed(6)
    args = _pargs(gnn_emb_dim=272, gnn_num_layer=4, max_seq_len=5)
    model = PNANet(5002, ASTNodeEncoder(272, 98, 300, 20), None, args)
    b = synth.code2_like(B=16, seed=6, num_nodeattributes=300, mean_nodes=40.0, max_nodes=80)
    oloss, hloss = (lambda out: rm.code2_loss(out, b.y_arr)), (lambda out, bd: losses.code2_loss(out, bd.y_arr))
    _vs_float64("real-shape", model, args, b, oloss, hloss, True, monkeypatch)


def test_pna_equals_the_recorded_reference():
    """tests/golden/pna_baseline_ref.json (the reference's own fp32 run of models/pna.py) loaded into PNANet: logits within 1e-4 (3 x the
    reference's own recorded fp32 noise where larger), gradients within check_grads' bars against the RECORDED fp32 gradients.  Both
    data paths: the module path and the fused step."""
    from graphtrans_amd import engine
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.pna import PNANet
    for c in load_fixture():
        D = c["args"].gnn_emb_dim
        model = PNANet(c["num_tasks"], ASTNodeEncoder(D, 11, 13, 20), None, c["args"])
        model.load_state_dict(c["sd"], strict=True)
        model = model.to(DEV).train()
        b = fixture_batch(c["inputs"]).to(DEV)
        names = {k for k, _ in model.named_parameters()}
        for fused in (False, True):
            model.fused = fused
            assert engine.eligible(model, b, None) == fused, (c["name"], fused)
            loss, grads, _ = _run(model, b, fixture_loss, fused, 0)
            model.fused = fused
            with torch.no_grad():
                out = model(b)   # (training mode, p = 0: the same forward; the buffers are not part of the comparison)
            outs = list(out) if isinstance(out, (list, tuple)) else [out]
            tol = max(1e-4, 3 * c["out_noise"])
            for o, r in zip(outs, c["logits"]):
                assert float((o.cpu() - r).abs().max()) <= tol, (c["name"], fused)
            check_grads({k: v.cpu() for k, v in grads.items()}, {k: v.double() for k, v in c["grads"].items() if k in names},
                        {k: c["grad_noise"] for k in c["grads"]}, what=f"recorded reference {c['name']} fused={fused}")


def test_fused_pna_backward_issues_the_gradient_allreduce():
    """dist.GradSync.attach on a one-rank nccl group: the staged backward hands the three ranges {heads (hidden layers included) | message
    passing | input encoder} to RCCL; the gradients are unchanged."""
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
        model, b, loss_of = _build("ast", _pargs(graph_pooling="max"))
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
