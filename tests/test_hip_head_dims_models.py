"""Head dims beyond 8 / 16 / 32 / 64 at the model level: the encoder stack at d_model 512 with four heads (head dim 128) and
the whole GNNTransformer on the fused path at head dims 128 (d_model 128, one head) and 48 (d_model 192, four heads), against
the CPU oracle in float64 with the criteria tests/test_hip_configs.py uses for the shipped configurations."""
import copy

import pytest
import torch

from conftest import assert_close, quantile_err, rel_l2
from test_hip_configs import (BOUNDS, ER_ARGS, _args, _encoder_oracle, check_grads, fp32_noise, hip_run, oracle_run,
                              precision_report)
from test_hip_engine import _args as _engine_args
from test_hip_engine import _run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_encoder_hd128_n513_vs_oracle(dtype):
    """TransformerNodeEncoder at d = 512, nhead 4 (head dim 128), ffn 1024, 2 layers over ragged sequences of up to 512 + CLS
    positions, with the criterion of test_hip_configs.test_c5_encoder_hd64_n513_vs_oracle: fp32 outputs elementwise 1e-4,
    gradients 98 %-quantile within max(1e-3, 10 x the fp32 oracle's own noise) and 5e-2 in relative L2; bf16 outputs 3e-2,
    gradients 8e-2 in relative L2."""
    from graphtrans_amd.modules.transformer_encoder import TransformerNodeEncoder

    torch.manual_seed(2)
    args = _args(**{**ER_ARGS, "d_model": 512, "nhead": 4, "dim_feedforward": 1024, "num_encoder_layers": 2}, compute_dtype=dtype)
    enc = TransformerNodeEncoder(args)
    sizes = [512, 300, 65, 1]
    S, B, d = 512, len(sizes), 512
    x = torch.zeros(S, B, d)
    mask = torch.zeros(B, S, dtype=torch.bool)
    for i, n in enumerate(sizes):
        x[S - n:, i] = torch.randn(n, d)
        mask[i, :S - n] = True
    valid = torch.cat([~mask, torch.ones(B, 1, dtype=torch.bool)], 1).t().unsqueeze(-1)   # (S+1, B, 1): real positions
    w = torch.randn(S + 1, B, d) * valid     # the padded query rows carry no loss (their values are layout-dependent)
    state = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    ref, dx_ref, g_ref = _encoder_oracle(state, args, x, mask, w, torch.float64)
    enc = enc.to(DEV).train()
    xd = x.to(DEV).requires_grad_(True)
    out, _ = enc(xd, mask.to(DEV))
    (out.float() * w.to(DEV)).sum().backward()
    got = out.detach().float().cpu() * valid
    dx = xd.grad.cpu() * valid[:S]
    grads = {k: p.grad.float().cpu() for k, p in enc.named_parameters() if p.grad is not None}
    print(f"\n[hd128 encoder {dtype}] outputs: max abs err {float((got.double() - ref * valid).abs().max()):.2e} (max |ref| {float(ref.abs().max()):.2f})")
    if dtype == torch.float32:
        assert_close(got, ref * valid, atol=1e-4, rtol=1e-4, what="encoder out")
        noise = {}
        for seed in (None, 1, 2):
            _, dx32, g32 = _encoder_oracle(state, args, x, mask, w, torch.float32, perturb_seed=seed, eps=6e-8)
            noise["d x"] = max(noise.get("d x", 0.0), quantile_err(dx32 * valid[:S], dx_ref * valid[:S]))
            for k, r in g_ref.items():
                noise[k] = max(noise.get(k, 0.0), quantile_err(g32[k], r))
        errs = {"d x": quantile_err(dx, dx_ref * valid[:S])}
        errs.update({k: quantile_err(grads[k], r) for k, r in g_ref.items()})
        ratio = {k: errs[k] / max(1e-3, 10 * noise[k]) for k in errs}
        worst = max(ratio, key=ratio.get)
        print(f"[hd128 encoder fp32] worst gradient: {worst} 98%-quantile err {errs[worst]:.1e} (fp32 oracle noise {noise[worst]:.1e})")
        assert ratio[worst] <= 1.0, (worst, errs[worst], noise[worst])
        assert max(rel_l2(grads[k], r) for k, r in g_ref.items()) <= 5e-2
    else:
        assert_close(got, ref * valid, atol=3e-2, rtol=3e-2, what="encoder out")
        errs = {"d x": rel_l2(dx, dx_ref * valid[:S])}
        errs.update({k: rel_l2(grads[k], r) for k, r in g_ref.items()})
        worst = max(errs, key=errs.get)
        print(f"[hd128 encoder bf16] worst relative L2 gradient error {errs[worst]:.2e} ({worst})")
        assert errs[worst] <= 8e-2, (worst, errs[worst])


def _small_model(d_model, nhead, dropout=0.0):
    """the model and batch of test_hip_engine.test_fused_model_matches_module_path (CPU), with the batch's own labels"""
    from graphtrans_amd import synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer

    args = _engine_args(d_model=d_model, nhead=nhead, transformer_dropout=dropout)
    torch.manual_seed(0)
    model = GNNTransformer(50, ASTNodeEncoder(64, 98, 300, 20), lambda d: torch.nn.Linear(2, d), args)
    with torch.no_grad():  # non-trivial virtual-node embedding and BN statistics
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
        model.gnn_node.virtualnode_embedding.weight.normal_(0, 0.3)
    model.train()
    b = synth.code2_like(B=12, seed=5, num_nodeattributes=300, num_vocab=50, max_seq_len=args.max_seq_len)
    return args, model, b


@pytest.mark.parametrize("d_model,nhead", [(128, 1), (192, 4)], ids=["hd128", "hd48"])
def test_fused_model_new_head_dims_vs_oracle(d_model, nhead):
    """GNNTransformer on the fused path (eligibility asserted), fp32, 12 Code2-like graphs, train mode: loss, logits and every
    parameter gradient against the float64 oracle -- BOUNDS["fp32"] and check_grads with the fp32 oracle's own noise, as the fp32 leg
    of test_hip_configs.test_fused_precision_modes_vs_oracle."""
    from graphtrans_amd import engine, losses
    from oracle import reference_math as rm

    args, model, b = _small_model(d_model, nhead)
    oloss = lambda out: rm.code2_loss(out, b.y_arr)   # noqa: E731
    hloss = lambda out, bd: losses.code2_loss(out, bd.y_arr)   # noqa: E731
    ref_out64, ref_loss64, ref_g64 = oracle_run(model, args, b, oloss, torch.float64)
    noise = fp32_noise(model, args, b, oloss, ref_g64)
    _, o32_loss, o32_g = oracle_run(model, args, b, oloss, torch.float32)
    o32 = precision_report(o32_g, o32_loss, ref_g64, ref_loss64)
    assert engine.eligible(model.to(DEV).train(), b.to(DEV), None), "must run on the fused path"
    outs, loss, grads = hip_run(model, b, hloss, torch.float32)
    rep = precision_report(grads, loss, ref_g64, ref_loss64)
    bound = BOUNDS["fp32"]
    refs = [o.detach() for o in (ref_out64 if isinstance(ref_out64, (list, tuple)) else [ref_out64])]
    top = max(float(r.abs().max()) for r in refs)
    lerr = max(float((o.double() - r).abs().max()) for o, r in zip(outs, refs)) / max(top, 1.0)
    print(f"\n[d_model {d_model} nhead {nhead}] loss rel err {rep['loss_rel_err']:.2e}; logits max err {lerr:.2e} of {top:.2f}; "
          f"grad rel-L2 worst {rep['grad_rel_l2_worst']:.2e} ({rep['grad_rel_l2_worst_param']}) median {rep['grad_rel_l2_median']:.2e}; "
          f"fp32 oracle itself: worst {o32['grad_rel_l2_worst']:.2e} median {o32['grad_rel_l2_median']:.2e}")
    assert rep["loss_rel_err"] <= bound["loss"], rep
    assert lerr <= bound["logits"], (lerr, bound["logits"])
    assert rep["grad_rel_l2_worst"] <= bound["worst"], rep
    assert rep["grad_rel_l2_median"] <= max(bound["median"], 3.0 * o32["grad_rel_l2_median"]), (rep, o32)
    check_grads(grads, ref_g64, noise, what=f"d_model {d_model} nhead {nhead} fp32")


def test_fused_model_matches_module_path_head_dim_48():
    """test_hip_engine.test_fused_model_matches_module_path at d_model 192, nhead 4: the driver's workspaces at a head dim that is
    not a whole number of 32-deep steps (transformer dropout 0.2 on, same seeds on both paths)."""
    from graphtrans_amd import engine

    args, model, b = _small_model(192, 4, dropout=0.2)
    model = model.to(DEV).train()
    b = b.to(DEV)
    y = b.y_arr
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
        assert torch.allclose(b0[n].float(), b1[n].float(), rtol=1e-4, atol=1e-6), n
