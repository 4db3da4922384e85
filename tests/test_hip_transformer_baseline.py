"""The plain Transformer baseline (graphtrans_amd/models/transformer.py) on the GPU, with the tolerances of
tests/test_hip_gnn_baseline.py: `fused_embed` on (token rows straight from the embedding tables, ops.embed_tokens) against off (the
composition node_encoder -> + perturb -> ops.seq_gather) on the same weights; both against the float64 statement of
tests/test_transformer_baseline_host.py (which that file pins to the reference's own models/transformer.py); and against
tests/golden/transformer_baseline_ref.json, recorded from the reference.
"""
import copy
from types import SimpleNamespace

import pytest
import torch

import test_hip_configs as thc
from test_hip_configs import BOUNDS, check_grads, precision_report
from test_hip_gnn_baseline import BF16_TOL, F32_TOL, _close
from test_transformer_baseline_host import fixture_batch, fixture_loss, load_fixture, statement_run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _targs(**kw):
    a = dict(d_model=64, nhead=4, dim_feedforward=128, transformer_dropout=0.0, transformer_activation="relu", num_encoder_layers=2,
             max_input_len=20, transformer_norm_input=False, graph_pooling="cls", max_seq_len=3, model_type="transformer",
             gnn_type="gcn", gnn_virtual_node=False)
    a.update(kw)
    return SimpleNamespace(**a)


def _build(feat, args, dev=DEV, attrs=300):
    """-> (model, batch, loss(out)): Code2-style (ASTNodeEncoder, stacked heads), Molpcba-style (AtomEncoder, one 16-way head), TU-style
    (nn.Linear(37, d) node encoder).  At max_input_len 20 each batch holds truncated graphs and, for mol / tud, untruncated ones."""
    from graphtrans_amd import losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder, AtomEncoder
    from graphtrans_amd.models.transformer import Transformer
    D = args.d_model
    torch.manual_seed(0)
    if feat == "ast":
        model = Transformer(50, ASTNodeEncoder(D, 98, attrs, 20), None, args)
        b = synth.code2_like(B=12, seed=5, num_nodeattributes=300).to(dev)
        y = torch.randint(0, 50, (12, 5), generator=torch.Generator().manual_seed(1)).to(dev)
        loss = (lambda out: losses.code2_loss(out, y)) if args.max_seq_len is not None else (lambda out: out.float().square().mean())
    elif feat == "mol":
        args.max_seq_len = None
        model = Transformer(16, AtomEncoder(D), None, args)
        b = synth.molpcba_like(B=24, seed=4).to(dev)
        g = torch.Generator().manual_seed(4)
        y = (torch.rand(24, 16, generator=g) > 0.5).float()
        y[torch.rand(24, 16, generator=g) < 0.2] = float("nan")
        y = y.to(dev)
        loss = lambda out: losses.mol_loss(out, y)
    else:
        args.max_seq_len = None
        model = Transformer(2, torch.nn.Linear(37, D), None, args)   # dataset/tud.py:65
        b = synth.nci1_like(B=16, seed=3).to(dev)
        loss = lambda out: losses.tud_loss(out, b.y)
    model = model.to(dev)
    with torch.no_grad():   # non-trivial LayerNorm affine / biases
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    return model.train(), b, loss


def _perturb(b, D, seed=2):
    return (torch.randn(b.batch.numel(), D, generator=torch.Generator().manual_seed(seed)) * 0.1).to(DEV)


def _run(model, b, loss_of, fused_embed, perturb=None):
    model.fused_embed = fused_embed
    for p in model.parameters():
        p.grad = None
    pt = None if perturb is None else perturb.clone().requires_grad_(True)
    out = model(b, pt)
    loss = loss_of(out)
    loss.backward()
    outs = [o.detach().float().clone() for o in (out if isinstance(out, (list, tuple)) else [out])]
    return outs, loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, None if pt is None else pt.grad.clone()


@pytest.fixture
def embed_calls(monkeypatch):
    """counts the calls of ops.embed_tokens"""
    from graphtrans_amd import ops
    calls, real = [], ops.embed_tokens

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "embed_tokens", counted)
    return calls


CASES = [dict(feat="ast"), dict(feat="ast", perturb=True), dict(feat="ast", max_input_len=1000, max_seq_len=None),
         dict(feat="mol"), dict(feat="mol", perturb=True), dict(feat="tud", perturb=True),
         dict(feat="ast", perturb=True, bf16=True), dict(feat="mol", bf16=True)]


@pytest.mark.parametrize("kw", CASES, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c in CASES])
def test_fused_embed_matches_the_composition(kw, embed_calls):
    """cls pooling, every encoder kind, training mode at dropout 0 and eval mode: logits, loss, every parameter gradient and
    perturb.grad.  The nn.Linear encoder has no tables: `fused_embed` on runs the composition there."""
    kw = dict(kw)
    feat, with_perturb, bf16 = kw.pop("feat"), kw.pop("perturb", False), kw.pop("bf16", False)
    if bf16:
        kw["compute_dtype"] = torch.bfloat16   # the bf16 token stream
    tol = BF16_TOL if bf16 else F32_TOL
    model, b, loss_of = _build(feat, _targs(**kw))
    perturb = _perturb(b, 64) if with_perturb else None
    o0, l0, g0, p0 = _run(copy.deepcopy(model), b, loss_of, False, perturb)
    assert not embed_calls
    o1, l1, g1, p1 = _run(model, b, loss_of, True, perturb)
    assert len(embed_calls) == (0 if feat == "tud" else 1)
    assert torch.allclose(l0, l1, **tol), (l0, l1)
    assert len(o0) == len(o1)
    for i, (u, v) in enumerate(zip(o0, o1)):
        _close(u, v, tol, f"logits {i}")
    assert set(g0) == set(g1)
    for n in g0:
        _close(g0[n], g1[n], tol, n)
    if with_perturb:
        _close(p0, p1, tol, "perturb.grad")
        assert p1.dtype == torch.float32 and p1.shape == perturb.shape
    model.eval()
    with torch.no_grad():
        model.fused_embed = True
        a = model(b, perturb)
        model.fused_embed = False
        c = model(b, perturb)
    for u, v in zip(a if isinstance(a, (list, tuple)) else [a], c if isinstance(c, (list, tuple)) else [c]):
        _close(u.float(), v.float(), tol, "eval logits")


@pytest.mark.parametrize("pooling", ["sum", "mean", "max"])
@pytest.mark.parametrize("feat", ["ast", "mol", "tud"])
def test_node_poolings_with_a_truncated_graph_vs_float64_statement(pooling, feat):
    """unpad_batch over the un-transformed rows, then the pooling over ALL nodes: logits within 1e-4, d loss / d perturb within 1e-4 of
    its largest entry (the bars of test_hip_gnn_baseline.test_module_path_routing), the heads' gradient at F32_TOL"""
    args = _targs(graph_pooling=pooling, max_seq_len=None)
    model, b, _ = _build(feat, args)
    assert int(torch.bincount(b.batch).max()) > args.max_input_len
    perturb = _perturb(b, 64).requires_grad_(True)
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
    """test_hip_configs.oracle_run for this model: the statement of tests/test_transformer_baseline_host.py"""
    return statement_run(model.state_dict(), args, b, loss_of, dtype)


@pytest.mark.parametrize("case", ["code2-cls-fused", "code2-cls-composition", "mol-mean"])
def test_transformer_fp32_vs_float64_statement(case, monkeypatch, embed_calls):
    """Exact-fp32 mode, 16 graphs: logits within 1e-4 elementwise, every gradient through test_hip_configs.check_grads with that file's
    fp32_noise model run on THIS model's oracle, BOUNDS["fp32"] on the precision report (test_hip_gnn_baseline's statement test)."""
    from graphtrans_amd import losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder, AtomEncoder
    from graphtrans_amd.models.transformer import Transformer
    from oracle import reference_math as rm
    monkeypatch.setattr(thc, "oracle_run", _oracle_run)   # fp32_noise calls it: same perturbations, same quantile, this model's math
    torch.manual_seed(5)
    if case.startswith("code2"):
        args = _targs(max_seq_len=5, max_input_len=40)
        model = Transformer(50, ASTNodeEncoder(64, 98, 300, 20), None, args)
        b = synth.code2_like(B=16, seed=5, num_nodeattributes=300, num_vocab=50)
        oloss, hloss = (lambda out: rm.code2_loss(out, b.y_arr)), (lambda out, bd: losses.code2_loss(out, bd.y_arr))
    else:
        args = _targs(graph_pooling="mean", max_seq_len=None)
        model = Transformer(16, AtomEncoder(64), None, args)
        b = synth.molpcba_like(B=16, seed=5, num_tasks=16)
        oloss, hloss = (lambda out: rm.mol_loss(out, b.y)), (lambda out, bd: losses.mol_loss(out, bd.y))
    model.fused_embed = case.endswith("fused")
    ref_out, ref_loss, ref_g = _oracle_run(model, args, b, oloss, torch.float64)
    noise = thc.fp32_noise(model, args, b, oloss, ref_g)
    _, o32_loss, o32_g = _oracle_run(model, args, b, oloss, torch.float32)
    o32 = precision_report(o32_g, o32_loss, ref_g, ref_loss)
    outs, loss, grads = thc.hip_run(model, b, hloss, torch.float32)
    assert len(embed_calls) == (1 if case.endswith("fused") else 0)
    refs = [o.detach() for o in (ref_out if isinstance(ref_out, (list, tuple)) else [ref_out])]
    top = max(float(r.abs().max()) for r in refs)
    lerr = max(float((o.double() - r).abs().max()) for o, r in zip(outs, refs))
    rep = precision_report(grads, loss, ref_g, ref_loss)
    print(f"\n[transformer {case}] logits: max |err| {lerr:.2e} (largest logit {top:.2f}); loss rel {rep['loss_rel_err']:.2e}; grad rel-L2 worst "
          f"{rep['grad_rel_l2_worst']:.2e} ({rep['grad_rel_l2_worst_param']}) median {rep['grad_rel_l2_median']:.2e}; fp32 oracle itself: "
          f"worst {o32['grad_rel_l2_worst']:.2e} median {o32['grad_rel_l2_median']:.2e}")
    assert 0.1 <= top <= 100.0, top     # inputs of O(1): the absolute bar below means what it says
    assert lerr <= 1e-4, lerr
    bound = BOUNDS["fp32"]
    assert rep["loss_rel_err"] <= bound["loss"] and rep["grad_rel_l2_worst"] <= bound["worst"], rep
    assert rep["grad_rel_l2_median"] <= max(bound["median"], 3.0 * o32["grad_rel_l2_median"]), (rep, o32)
    check_grads(grads, ref_g, noise, what=f"transformer {case} fp32")


def test_transformer_equals_the_recorded_reference(embed_calls):
    """tests/golden/transformer_baseline_ref.json (the reference's own fp32 run of models/transformer.py, with a perturbation) loaded
    into Transformer: logits within 1e-4, gradients within check_grads' bars (noise 0: its base of 1e-3 of the tensor's largest entry)
    against the RECORDED fp32 gradients, d perturb at F32_TOL.  `fused_embed` off and on."""
    from test_transformer_baseline_host import _build as host_build
    for c in load_fixture():
        model = host_build(c["args"], c["feat"])
        model.load_state_dict(c["sd"], strict=True)
        model = model.to(DEV).train()
        b = fixture_batch(c["inputs"]).to(DEV)
        perturb = c["inputs"]["perturb"].to(DEV)
        for fused_embed in (False, True):
            n0 = len(embed_calls)
            outs, _, grads, dp = _run(model, b, fixture_loss, fused_embed, perturb)
            assert len(embed_calls) - n0 == (1 if fused_embed and c["name"] == "code2-cls-heads3" else 0), (c["name"], fused_embed)
            assert len(outs) == len(c["logits"])
            for o, r in zip(outs, c["logits"]):
                assert float((o.cpu() - r).abs().max()) <= 1e-4, (c["name"], fused_embed)
            check_grads({k: v.cpu() for k, v in grads.items()}, {k: v.double() for k, v in c["grads"].items()},
                        {k: 0.0 for k in c["grads"]}, what=f"recorded reference {c['name']} fused_embed={fused_embed}")
            _close(c["perturb_grad"], dp.cpu(), F32_TOL, f"{c['name']} perturb grad")


def test_a_table_beyond_the_sorted_backward_runs_the_composition(embed_calls):
    """an attribute table of 20000 rows (> 16384, the sort's limit): the predicate says no, `fused_embed` on runs the composition, and
    the result is the statement's"""
    from graphtrans_amd import ops
    args = _targs(max_seq_len=None)
    model, b, _ = _build("ast", args, attrs=20000)
    assert model.node_encoder.attribute_encoder.weight.shape[0] > ops.EMBED_SORT_MAX_ROWS
    sq = lambda out: out.square().mean()
    outs, _, grads, _ = _run(model, b, sq, True)
    assert not embed_calls
    ref_out, _, ref_g = statement_run(model.state_dict(), args, b.to("cpu"), sq, torch.float64)
    assert float((outs[0].cpu().double() - ref_out.detach()).abs().max()) <= 1e-4
    _close(ref_g["graph_pred_linear.weight"].float(), grads["graph_pred_linear.weight"].cpu(), F32_TOL, "head")
    _close(ref_g["node_encoder.attribute_encoder.weight"].float(), grads["node_encoder.attribute_encoder.weight"].cpu(), F32_TOL, "table")


def test_flag_step_agrees_with_the_manual_loop_on_the_composition(embed_calls):
    """flag.flag_step (m = 3) on the model with `fused_embed` on, against the same three passes written out on a copy that runs the
    composition: the perturbation after its two ascents, its last gradient and the accumulated parameter gradients"""
    from graphtrans_amd import flag, losses
    m, step = 3, 8e-3
    model, b, _ = _build("ast", _targs())
    y = torch.randint(0, 50, (12, 5), generator=torch.Generator().manual_seed(1)).to(DEV)
    calc = lambda out, batch: losses.code2_loss(out, y)
    twin = copy.deepcopy(model)
    model.fused_embed, twin.fused_embed = True, False
    start = (torch.rand(b.batch.numel(), 64, generator=torch.Generator().manual_seed(3)) * 2 - 1).mul_(step).to(DEV)
    pa, pb = start.clone(), start.clone().requires_grad_(True)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    loss_a = flag.flag_step(model, b, opt, calc, m=m, step_size=step, perturb=pa)
    assert len(embed_calls) == m
    twin.train()
    for i in range(m):
        loss_b = calc(twin(b, pb), b) / m
        loss_b.backward()
        if i < m - 1:
            with torch.no_grad():
                pb.add_(step * pb.grad.sign())
                pb.grad.zero_()
    assert len(embed_calls) == m
    assert torch.allclose(loss_a, loss_b.detach(), **F32_TOL), (loss_a, loss_b)
    _close(pb.grad, pa.grad, F32_TOL, "perturb.grad")
    moved = (pa.detach() - pb.detach()).abs() > 1e-9   # a sign flipped by rounding in a gradient of ~0 moves an element by 2 * step
    assert float(moved.float().mean()) <= 1e-3, float(moved.float().mean())
    assert float((pa.detach() - start).abs().max()) > 0
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        _close(q.grad, p.grad, F32_TOL, n)
