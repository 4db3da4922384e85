"""ops.set_matmul_precision("high") through the models: the `mixed` mode (fp32 GNN-side GEMMs, bf16 token rows) with the GNN side at three
bf16 products per fp32 product, held to the project's own `mixed` criteria against the float64 oracle; fused and module paths agree; the
benchmark-size step (k_lin3r and k_lin3r_dw inside the driver) is reproducible, close to the "highest" step and leaves the default path's
bits alone; a backward uses the precision of its forward."""
import contextlib
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@contextlib.contextmanager
def precision(p):
    from graphtrans_amd import ops
    prev = ops.set_matmul_precision(p)
    try:
        yield
    finally:
        ops.set_matmul_precision(prev)


@pytest.mark.parametrize("workload,graphs", [("code2", 24), ("molpcba", 64)])
def test_mixed_mode_with_high_precision_vs_oracle(workload, graphs):
    """test_fused_precision_modes_vs_oracle[mixed] with the fp32 GEMMs under "high": the same bounds (loss 5e-4, logits 1.5e-2 of the largest
    logit, every gradient tensor within 4 x its oracle bf16-noise)"""
    from graphtrans_amd import engine
    from test_hip_configs import BOUNDS, _args, build, check_lowp_grads, hip_run, oracle_run, precision_report
    kw = dict(compute_dtype=torch.bfloat16)
    if workload == "molpcba":
        kw.update(gnn_type="gin", max_seq_len=None)
    args = _args(**kw)
    model, b, oloss, hloss = build(workload, args, graphs, 5)
    ref_out64, ref_loss64, ref_g64 = oracle_run(model, args, b, oloss, torch.float64)
    with precision("high"):
        assert engine.eligible(model.to(DEV).train(), b.to(DEV), None), "the benchmarked configuration must run on the fused path"
        outs, loss, grads = hip_run(model, b, hloss, torch.float32)
    rep = precision_report(grads, loss, ref_g64, ref_loss64)
    print(f"\n[{workload} mixed+high] loss {float(loss):.6f} vs fp64 oracle {float(ref_loss64):.6f} (rel {rep['loss_rel_err']:.2e}); "
          f"grad rel-L2 err worst {rep['grad_rel_l2_worst']:.2e} median {rep['grad_rel_l2_median']:.2e} over {rep['tensors']} tensors; "
          "worst: " + ", ".join(f"{k} {e:.1e}" for k, e in rep["worst4"]))
    bound = BOUNDS["mixed"]
    assert rep["loss_rel_err"] <= bound["loss"], rep
    refs = [o.detach() for o in (ref_out64 if isinstance(ref_out64, (list, tuple)) else [ref_out64])]
    top = max(float(r.abs().max()) for r in refs)
    lerr = max(float((o.double() - r).abs().max()) for o, r in zip(outs, refs)) / max(top, 1.0)
    print(f"[{workload} mixed+high] logits: max elementwise error {lerr:.2e} of the largest logit ({top:.2f}); bound {bound['logits']:g}")
    assert lerr <= bound["logits"], (lerr, bound["logits"])
    check_lowp_grads(model, args, b, oloss, grads, ref_g64, "mixed", what=f"{workload} mixed+high")


def test_fused_and_module_paths_agree_under_high():
    """test_fused_model_matches_module_path's default case and fp32 tolerances, both paths under "high" """
    from graphtrans_amd import engine, synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    from test_hip_engine import _args, _run
    args = _args()
    torch.manual_seed(0)
    model = GNNTransformer(50, ASTNodeEncoder(64, 98, 300, 20), lambda d: torch.nn.Linear(2, d), args).to(DEV)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
        model.gnn_node.virtualnode_embedding.weight.normal_(0, 0.3)
    model.train()
    b = synth.code2_like(B=12, seed=5, num_nodeattributes=300).to(DEV)
    y = torch.randint(0, 50, (12, 5), device=DEV)
    with precision("high"):
        assert engine.eligible(model, b, None)
        ref_model = copy.deepcopy(model)
        l0, g0, b0 = _run(ref_model, b, y, False, 7)
        l1, g1, b1 = _run(model, b, y, True, 7)
    tol = dict(rtol=1e-4, atol=1e-6)
    assert torch.allclose(l0, l1, **tol), (l0, l1)
    for n in g0:
        scale = max(1.0, float(g0[n].abs().max()))
        assert torch.allclose(g0[n] / scale, g1[n] / scale, **tol), (n, (g0[n] - g1[n]).abs().max())
    for n in b0:
        assert torch.allclose(b0[n].float(), b1[n].float(), **tol), n


@pytest.fixture(scope="module")
def bench_model():
    """the Code2 b256 `mixed` model and batch of test_fused_backward_is_bitwise_reproducible_at_benchmark_size (built once)"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    torch.manual_seed(0)
    args, model, gen, loss_fn, _ = bench.build("code2", torch.bfloat16, torch.device(DEV), 256)
    for m in model.modules():
        if hasattr(m, "dropout_p"):
            m.dropout_p = 0.0
    model.gnn_node.drop_ratio = 0.0
    model.train()
    b = bench.attach_sizes(gen(0)).to(DEV)
    return model, b, loss_fn


def _step(model, b, loss_fn, before_backward=None):
    for p in model.parameters():
        p.grad = None
    b.__dict__.pop("_gt_structure", None)
    loss = loss_fn(model(b), b)
    if before_backward is not None:
        before_backward()
    loss.backward()
    return loss.detach().clone(), [p.grad.detach().clone() for p in model.parameters()]


def test_benchmark_size_step_under_high(bench_model):
    from graphtrans_amd import engine, ops
    model, b, loss_fn = bench_model
    assert ops.get_matmul_dtype() == torch.float32 and ops.get_matmul_precision() == "highest"
    assert engine.eligible(model, b, None)
    l6, g6 = _step(model, b, loss_fn)
    with precision("high"):
        assert engine.eligible(model, b, None)
        l3, g3 = _step(model, b, loss_fn)
        l3b, g3b = _step(model, b, loss_fn)
    assert torch.equal(l3, l3b) and all(torch.equal(u, v) for u, v in zip(g3, g3b))
    d = abs(float(l3) - float(l6)) / abs(float(l6))
    print(f"\n[code2 b256 mixed] loss highest {float(l6):.6f} high {float(l3):.6f} (rel {d:.2e})")
    assert d <= 5e-4, d
    assert any(not torch.equal(u, v) for u, v in zip(g3, g6)), "the three-product kernels did not run"
    l6b, g6b = _step(model, b, loss_fn)   # back under "highest": the first result, bit for bit
    assert torch.equal(l6, l6b) and all(torch.equal(u, v) for u, v in zip(g6, g6b))


def test_backward_uses_the_precision_of_its_forward(bench_model):
    from graphtrans_amd import ops
    model, b, loss_fn = bench_model
    with precision("high"):
        _, g_stay = _step(model, b, loss_fn)
        _, g_switch = _step(model, b, loss_fn, before_backward=lambda: ops.set_matmul_precision("highest"))
        assert ops.get_matmul_precision() == "highest"
    bad = [n for (n, _), u, v in zip(model.named_parameters(), g_stay, g_switch) if not torch.equal(u, v)]
    assert not bad, (len(bad), bad[:4])
