"""The training loop of bench.py -- GradSync.zero() -> model(b) -> loss -> backward() -> sync.finish() -> FusedAdamW.step(), a different
batch every step -- with EVERY step held to the float64 oracle (oracle/reference_math.py) at the HIP run's own parameters.

Nothing is compared at the end of two independent trajectories (Adam's first update is lr * sign(g): rounding noise in a near-zero
gradient becomes a parameter difference of 2 * lr).  Each step is checked where the HIP run stands (teacher forcing):

  1. loss and logits of the step against the float64 oracle on a snapshot of the state taken before the step;
  2. every parameter gradient (check_grads / check_lowp_grads of tests/test_hip_configs.py; the accumulated step against the gradient
     of loss_a + loss_b, with the fp32 oracle's own noise on that sum);
  3. the BatchNorm buffers the step wrote: 0.9 x snapshot + 0.1 x the oracle's batch mean / unbiased variance, num_batches_tracked;
  4. the optimizer against a float64 CPU torch.optim.AdamW twin that is fed the HIP run's own gradients (parameters, both moments,
     the clipping norm, step counts -- the numbers of tests/test_hip_optim.py);
  5. the path that ran: engine.eligible at every step, `.grad` IS the persistent view of the flat buffer, FusedAdamW's reuse path
     (plan["same"]) from the second direct step on, off for the accumulated step and on again one step later, the weight images;
  6. an eval forward between two steps: logits against the oracle on the running statistics, buffers bit-identical afterwards.

The run crosses the 1024-node-row line at which the fused driver switches to the image-backed GEMMs (big, small, big, big + big
accumulated, small), so layouts, staging ring, arena sizes and kernels change between steps while the state is carried along.

test_stale_parameters_are_caught (CPU, oracle only) shows that check 2 has teeth: the exact float64 gradient with ONE parameter group
left one optimizer step behind fails check_grads for every group and step.

Measured on one MI355X run (worst over the steps of a case; the bound in brackets):
  fp32 fused, FusedAdamW     loss 6.1e-08 [1e-4], logits 1.0e-06 [1e-4], BatchNorm buffers 6.9e-07 [1e-4], eval logits 3.6e-07 [1e-4];
                             gradients: closest tensor gnn_node.convs.2.linear.bias, err 6.7e-05 (tol 1.0e-03);
                             twin: norm 5.3e-08 rel [1e-5], parameters 5.2e-07 abs [1e-7 + 1e-5 |p|], exp_avg 2.6e-09 [1e-8], exp_avg_sq 5.7e-11 [1e-10]
  fp32 modules, FusedAdamW   loss 5.9e-08, logits 1.5e-06, BatchNorm buffers 7.7e-07, eval logits 2.9e-07; gradients: closest tensor
                             gnn_node.batch_norms.1.weight at the accumulated step, err 7.5e-04 (tol 1.0e-03);
                             twin: norm 5.3e-08, parameters 4.9e-07, exp_avg 2.3e-09, exp_avg_sq 5.6e-11
  fp32 modules, torch AdamW  loss 5.7e-08, logits 1.2e-06, BatchNorm buffers 8.6e-07, eval logits 3.7e-07; gradients: closest tensor
                             gnn_node.convs.2.linear.bias, err 3.9e-05 (tol 1.0e-03)
  mixed fused, FusedAdamW    loss 9.7e-05 rel [5e-4], logits 5.5e-03 of the largest [1.5e-2], BatchNorm buffers 4.6e-07, eval logits 4.4e-03;
                             gradients: closest tensor graph_pred_linear_list.0.bias at 3.1 x the oracle's bf16-noise [4 x];
                             twin: norm 2.8e-08, parameters 7.0e-07, exp_avg 2.4e-09, exp_avg_sq 6.9e-11
Each GPU case takes 3 to 5 s, the CPU test 15 to 20 s.

exp_avg_sq sits at half its absolute bound for a known reason: k_adamw forms 1 - beta2 as 1.0f - 0.999f, 1.3e-5 away from 0.001, so at
torch's default betas the second moment is 1.3e-5 (relative) from torch.optim.AdamW's.  The parameters do not see it (5e-7); correcting
it changes the trajectory of every run and is left for a change of its own.  With second moments above 3e-5 this comparison would fail.

Gate flips.  A gradient failure on ONE small step with loss, logits and buffers of that step at 1e-7 is a ReLU gate flip until shown
otherwise, not stale state.  With seed 35 for the last small batch the fused case fails there, on every run: gnn_node.batch_norms.1.weight
2.4e-03, convs.1.root_emb.weight 2.0e-03, batch_norms.1.bias 1.9e-03, convs.0.edge_encoder.weight 1.8e-03 against tol 1.0e-03, thirty GNN
tensors below the last conv above 3e-04, everything else at 1e-6.  The loop's gradient is bit-identical to that of a fresh model loaded
with the same state, the module path gives the same figures, and the fp32 oracle at that state is at 1e-6.  In the float64 oracle at
that state ONE pre-activation of the last GCNConv's per-edge ReLU (relu(x_j + edge_emb), 1026 x 128 units) is 2.5e-07, at a mean
magnitude of 0.74: within fp32 rounding of zero.  The float64 gradient with that one gate taken on the other side agrees with the HIP
gradient to 1.7e-06 on every tensor.  The HIP gradient is the exact gradient on the other side of a kink, and in a batch of 6 graphs
(361 rows) one edge's row weighs ten times what it does at the ~3 k rows check_grads' base of 1e-3 is sized for.  The bound stays as it
is; the last small batch uses seed 36.  A later change to any kernel's rounding can meet such a unit again (a few per cent per small
step): look for a pre-activation within 1e-6 of zero before looking for stale state.  A stale image or pointer moves the worst tensor
by 2e-2 and more (test_stale_parameters_are_caught).
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, quantile_err
from test_hip_configs import BOUNDS, MODES, _args, check_grads, check_lowp_grads, fp32_noise, oracle_run

DEV = "cuda:0"
LR, WD, CLIP, SCHED = 1e-3, 0.01, 1.0, dict(step_size=2, gamma=0.5)
# (graphs, mean nodes, seed) of every forward; an inner list of two is ONE optimizer step accumulated over two micro-batches
BIG, SMALL = (24, 105.0), (6, 40.0)
STEPS = [[BIG + (31,)], [SMALL + (32,)], [BIG + (33,), BIG + (34,)], [SMALL + (36,)]]   # (36, not 35: see the header on gate flips)
GROUPS = dict(encoder="transformer_encoder.", convs="gnn_node.convs.", gnn2transformer="gnn2transformer.",
              vn_mlps="gnn_node.mlp_virtualnode_list.", heads="graph_pred_linear_list.")


def _train_args(**kw):
    """the dimensions at which test_gnn2transformer_writes_the_token_rows_itself finds the image-backed kernels taken"""
    return _args(gnn_num_layer=3, gnn_emb_dim=128, d_model=128, dim_feedforward=256, num_encoder_layers=2, nhead=4, max_seq_len=3, **kw)


def _model(args):
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer

    torch.manual_seed(0)
    return GNNTransformer(50, ASTNodeEncoder(128, 98, 300, 20), lambda d: torch.nn.Linear(2, d), args).train()


def _batch(graphs, mean_nodes, seed):
    """(batch, targets), both on the CPU"""
    from graphtrans_amd import synth

    b = synth.code2_like(B=graphs, seed=seed, mean_nodes=mean_nodes, num_nodeattributes=300)
    n = int(b.x.shape[0])
    assert (n >= 1024) if graphs == BIG[0] else (n < 1024), n   # the two sides of the line at which the image-backed GEMMs come in
    return b, torch.randint(0, 50, (graphs, 3), generator=torch.Generator().manual_seed(seed))


def _oloss(y):
    """dataset/code.py:39-45 in the oracle's own dtype (reference_math.code2_loss casts the logits to fp32)"""
    return lambda out: sum(F.cross_entropy(p, y[:, i]) for i, p in enumerate(out)) / len(out)


def oracle_sum(model, args, items, dtype):
    """oracle_run over the micro-batches of one step: (logits per micro-batch, loss per micro-batch, gradient of the SUM of the losses)"""
    outs, losses, total = [], [], {}
    for b, y in items:
        out, loss, g = oracle_run(model, args, b, _oloss(y), dtype)
        outs.append(torch.stack([o.detach() for o in out], 1))   # (B, heads, classes), as StackedHeads holds them
        losses.append(loss)
        for k, v in g.items():
            total[k] = v if k not in total else total[k] + v
    return outs, losses, total


def fp32_noise_sum(model, args, items, ref64, eps=6e-8, seeds=(1, 2)):
    """test_hip_configs.fp32_noise for a gradient accumulated over several micro-batches: conftest.quantile_err of the SUMMED fp32-oracle
    gradient against the summed float64 one, maximum over the unperturbed run and runs with every parameter moved by ~1 fp32 ulp (the
    same perturbed parameters for all micro-batches of a run: one step, one set of weights)."""
    if len(items) == 1:
        return fp32_noise(model, args, items[0][0], _oloss(items[0][1]), ref64, eps=eps, seeds=seeds)
    noise = {k: 0.0 for k in ref64}
    for s in (None,) + tuple(seeds):
        m2 = model
        if s is not None:
            m2 = copy.deepcopy(model)
            g = torch.Generator().manual_seed(s)
            with torch.no_grad():
                for p in m2.parameters():
                    p.mul_(1 + eps * torch.randn(p.shape, generator=g))
        g32 = oracle_sum(m2, args, items, torch.float32)[2]
        for k in noise:
            noise[k] = max(noise[k], quantile_err(g32[k], ref64[k]))
    return noise


@pytest.fixture
def bn_stats(monkeypatch):
    """reference_math.batch_norm wrapped: while `tap["rec"]` is a dict, every train-mode call records, per prefix as gnn_node sees it,
    the batch mean and the UNBIASED variance -- what nn.BatchNorm1d folds into its running statistics."""
    from oracle import reference_math as rm

    tap, real = {"rec": None}, rm.batch_norm

    def batch_norm(x, sd, prefix, training, eps=1e-5):
        if training and tap["rec"] is not None:
            tap["rec"][prefix] = (x.detach().mean(0), x.detach().var(0, unbiased=True))
        return real(x, sd, prefix, training, eps)

    monkeypatch.setattr(rm, "batch_norm", batch_norm)
    return tap


# --------------------------------------------------------------------------------------------------------------------
# the bounds have teeth (CPU)
# --------------------------------------------------------------------------------------------------------------------
def test_stale_parameters_are_caught():
    """Parameters advanced by fp32 torch AdamW (same hyper-parameters, clipping and schedule) over the five batches, gradients from the
    fp32 oracle.  At every step after the first the EXACT float64 gradient, evaluated with one parameter group left at its values of
    one step earlier -- what a stale weight image or a stale cached pointer would compute -- is handed to check_grads in place of a
    HIP gradient and must fail; the fp32 oracle's own gradient along the same trajectory must pass.  Groups: encoder, gnn_node.convs,
    gnn2transformer, virtual-node MLPs, heads (the least visible: heads one step stale move the worst tensor by > 2e-2)."""
    args = _train_args()
    model = _model(args)
    names = [k for k, _ in model.named_parameters()]
    opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD)
    sched = torch.optim.lr_scheduler.StepLR(opt, **SCHED)
    prev = None
    for s, step in enumerate(STEPS):
        items = [_batch(*spec) for spec in step]
        _, _, g32 = oracle_sum(model, args, items, torch.float32)
        if prev is not None:
            _, _, ref64 = oracle_sum(model, args, items, torch.float64)
            noise = fp32_noise_sum(model, args, items, ref64)
            check_grads(g32, ref64, noise, what=f"step {s}: the fp32 oracle itself")
            for group, prefix in GROUPS.items():
                stale = copy.deepcopy(model)
                keys = [k for k in names if k.startswith(prefix)]
                assert keys, group
                stale.load_state_dict({k: prev[k] for k in keys}, strict=False)
                _, _, g_stale = oracle_sum(stale, args, items, torch.float64)
                with pytest.raises(AssertionError):
                    check_grads(g_stale, ref64, noise, what=f"step {s}: {group} one step stale")
        prev = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for k, p in model.named_parameters():
            p.grad = g32[k].clone()
        torch.nn.utils.clip_grad_norm_(model.parameters(), CLIP)
        opt.step()
        sched.step()


# --------------------------------------------------------------------------------------------------------------------
# the loop on the GPU
# --------------------------------------------------------------------------------------------------------------------
def _cpu_state(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def _twin_check(opt, twin, tparams, names, dev):
    """FusedAdamW after its step against the float64 twin after the same step on the same gradients -> largest deviations"""
    state = opt.state_dict()["state"]
    for i, (n, p, q) in enumerate(zip(names, opt.param_groups[0]["params"], tparams)):
        st, tw = opt.state[p], twin.state[q]
        assert float(state[i]["step"]) == float(tw["step"]), (n, "step")
        for k, a, r, atol in (("param", p, q, 1e-7), ("exp_avg", st["exp_avg"], tw["exp_avg"], 1e-8),
                              ("exp_avg_sq", st["exp_avg_sq"], tw["exp_avg_sq"], 1e-10)):
            a, r = a.detach().cpu().double(), r.detach()
            assert torch.allclose(a, r, rtol=1e-5, atol=atol), (n, k, float((a - r).abs().max()))
            dev[k] = max(dev.get(k, 0.0), float((a - r).abs().max()))


def _run_loop(mode, fused, fused_opt, steps):
    """The HIP run.  -> one record per optimizer step (everything on the CPU) and the record of the eval forward; checks 4 and 5 are
    made on the way (they need no oracle)."""
    from graphtrans_amd import engine, losses, ops
    from graphtrans_amd.dist import GradSync
    from graphtrans_amd.optim import FusedAdamW

    matmul, tokens = MODES[mode]
    args = _train_args(compute_dtype=tokens)
    cpu_model = _model(args)
    model = copy.deepcopy(cpu_model).to(DEV).train()
    model.fused = fused
    names = [k for k, _ in model.named_parameters()]
    params = [p for _, p in model.named_parameters()]
    sync = GradSync(model.parameters(), world_size=1).attach(model)
    if fused_opt:
        opt = FusedAdamW(model.parameters(), lr=LR, weight_decay=WD, max_grad_norm=CLIP)
        tparams = [p.detach().cpu().double().clone().requires_grad_(True) for p in params]
        twin = torch.optim.AdamW(tparams, lr=LR, weight_decay=WD)
        tsched = torch.optim.lr_scheduler.StepLR(twin, **SCHED)
    else:
        opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD)
    sched = torch.optim.lr_scheduler.StepLR(opt, **SCHED)
    records, eval_rec, forwards, direct_steps = [], None, 0, 0
    ops.set_matmul_dtype(matmul)
    try:
        for s, step in enumerate(steps):
            items = [_batch(*spec) for spec in step]
            rec = dict(items=items, before=_cpu_state(model), logits=[], loss=[], after_forward=[], dev={})
            sync.zero()
            for b, y in items:
                bd, yd = b.to(DEV), y.to(DEV)
                bd.__dict__.pop("_gt_structure", None)   # graph_prep is part of the step (bench.py)
                if fused:
                    assert engine.eligible(model, bd, None), f"step {s} left the fused path"
                out = model(bd)
                loss = losses.code2_loss(out, yd)
                loss.backward()
                forwards += 1
                rec["logits"].append(torch.stack(list(out), 1).detach().float().cpu())
                rec["loss"].append(float(loss.detach()))
                rec["after_forward"].append({k: v.detach().cpu().clone() for k, v in model.named_buffers()})
            sync.finish()
            rec["forwards"] = forwards
            rec["grads"] = {k: p.grad.detach().cpu().clone() for k, p in zip(names, params)}   # (the views are overwritten next step)
            direct = len(items) == 1
            if fused:   # check 5: the gradients ARE the persistent views (direct), or fresh sums (accumulated)
                plan = engine.state(model)["plan"]
                assert len(plan.tlist) == len(params) and len(plan.tviews) == len(params)
                is_view = [p.grad is v for p, v in zip(plan.tlist, plan.tviews)]
                assert all(is_view) if direct else not any(is_view), (s, direct, sum(is_view))
                if mode == "fp32":
                    assert plan.imgs3e is not None
                else:
                    assert plan.imgs3 is not None and plan.imgs1 is not None
            if fused_opt:
                for q, p in zip(tparams, params):
                    q.grad = p.grad.detach().cpu().double()
                tnorm = torch.nn.utils.clip_grad_norm_(tparams, CLIP)
                opt.step()
                twin.step()
                tsched.step()
                nerr = abs(float(opt.last_grad_norm) - float(tnorm)) / float(tnorm)
                assert nerr <= 1e-5, (s, float(opt.last_grad_norm), float(tnorm))
                rec["dev"]["norm"] = nerr
                _twin_check(opt, twin, tparams, names, rec["dev"])
                if fused:   # the reuse path: the same gradient tensors as at the last direct step
                    direct_steps += direct
                    same = opt._plans[0]["same"]
                    assert same == (direct and direct_steps >= 2), (s, same, direct, direct_steps)
            else:
                torch.nn.utils.clip_grad_norm_(model.parameters(), CLIP)
                opt.step()
            sched.step()
            torch.cuda.synchronize()
            records.append(rec)
            if s == 1:   # check 6: an eval forward between two steps reads the running statistics and writes nothing
                b, y = _batch(*steps[1][0])
                bd = b.to(DEV)
                before = {k: v.detach().clone() for k, v in model.named_buffers()}
                model.eval()
                with torch.no_grad():
                    out = model(bd)
                    logits = torch.stack(list(out), 1).float().cpu()
                model.train()
                for k, v in model.named_buffers():
                    assert torch.equal(v, before[k]), ("eval forward wrote", k)
                eval_rec = dict(batch=b, state=_cpu_state(model), logits=logits)
    finally:
        ops.set_matmul_dtype(torch.float32)
    return args, cpu_model, records, eval_rec


def _logit_check(mode, got, ref, what):
    """check 1 / 6 on the logits -> the figure that was bounded"""
    err = (got.double() - ref).abs()
    if mode == "fp32":
        e = float((err / ref.abs().clamp_min(1.0)).max())
        assert e <= 1e-4, (what, e)
        return e
    e = float(err.max()) / max(float(ref.abs().max()), 1.0)
    assert e <= BOUNDS[mode]["logits"], (what, e)
    return e


def _check_records(mode, args, cpu_model, records, eval_rec, tap, what):
    """checks 1-3 and 6, the CPU half: one float64 oracle run per micro-batch at the snapshot taken before the step"""
    from oracle import noise as on
    from oracle import reference_math as rm

    worst = {}
    for s, rec in enumerate(records):
        cpu_model.load_state_dict(rec["before"])
        items = rec["items"]
        stats = []
        for it in items:   # (one by one: the recorder keeps the statistics of each micro-batch apart)
            tap["rec"] = {}
            try:
                stats.append((oracle_sum(cpu_model, args, [it], torch.float64), tap["rec"]))
            finally:
                tap["rec"] = None
        ref_g, lerr, oerr = {}, 0.0, 0.0
        for i, ((outs, losses, g), _) in enumerate(stats):
            ref_loss = float(losses[0])
            if mode == "fp32":
                e = abs(rec["loss"][i] - ref_loss) / max(1.0, abs(ref_loss))
                assert e <= 1e-4, (s, i, rec["loss"][i], ref_loss)
            else:
                e = abs(rec["loss"][i] - ref_loss) / abs(ref_loss)
                assert e <= BOUNDS[mode]["loss"], (s, i, rec["loss"][i], ref_loss)
            lerr = max(lerr, e)
            oerr = max(oerr, _logit_check(mode, rec["logits"][i], outs[0], f"step {s}.{i} logits"))
            for k, v in g.items():
                ref_g[k] = v if k not in ref_g else ref_g[k] + v
        # check 3: the buffers after every forward of the step, from the snapshot and the oracle's batch statistics
        buf, berr, seen = dict(rec["before"]), 0.0, 0
        for i, (_, bn) in enumerate(stats):
            got = rec["after_forward"][i]
            for prefix, (mean, var) in bn.items():
                k = "gnn_node." + prefix
                for name, stat in ((k + ".running_mean", mean), (k + ".running_var", var)):
                    buf[name] = 0.9 * buf[name].double() + 0.1 * stat
                    assert_close(got[name], buf[name], what=f"step {s}.{i} {name}")
                    berr = max(berr, float((got[name].double() - buf[name]).abs().max()) / max(1.0, float(buf[name].abs().max())))
                    seen += 1
                assert int(got[k + ".num_batches_tracked"]) == rec["forwards"] - len(items) + i + 1, (s, i, k)
        assert seen == 2 * sum(k.endswith("running_mean") for k in rec["before"]) * len(items)   # every BatchNorm of the model was reached
        print(f"\n[{what} step {s}] loss err {lerr:.1e}, logits err {oerr:.1e}, BatchNorm buffers err {berr:.1e}, optimizer vs float64 twin: "
              + (", ".join(f"{k} {v:.1e}" for k, v in rec["dev"].items()) or "-"))
        for k, v in dict(loss=lerr, logits=oerr, bn=berr, **rec["dev"]).items():
            worst[k] = max(worst.get(k, 0.0), v)
        # check 2
        if mode == "fp32":
            noise = fp32_noise_sum(cpu_model, args, items, ref_g)
            check_grads(rec["grads"], ref_g, noise, what=f"{what} step {s}")
        else:
            assert len(items) == 1
            check_lowp_grads(cpu_model, args, items[0][0], _oloss(items[0][1]), rec["grads"], ref_g, mode, what=f"{what} step {s}")
    # check 6
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in eval_rec["state"].items()}
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            ref = torch.stack(rm.gnn_transformer(sd, on.oracle_args(args), eval_rec["batch"], None, False), 1)
    finally:
        torch.set_default_dtype(torch.float32)
    worst["eval logits"] = _logit_check(mode, eval_rec["logits"], ref, "eval logits")
    print(f"[{what}] worst over the run: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


CASES = [("fp32", True, True, 4), ("fp32", False, True, 4), ("fp32", False, False, 4), ("mixed", True, True, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,fused,fused_opt,nsteps", CASES,
                         ids=["fp32-fused-FusedAdamW", "fp32-modules-FusedAdamW", "fp32-modules-torchAdamW", "mixed-fused-FusedAdamW"])
def test_every_training_step_vs_float64_oracle(mode, fused, fused_opt, nsteps, bn_stats):
    """fp32: big, small, big + big accumulated, small (five forwards, four optimizer steps); mixed: big, small, big (check_lowp_grads
    costs four more oracle runs per step).  modules + torch.optim.AdamW is the module path under torch's own in-place updates."""
    steps = STEPS if nsteps == 4 else [STEPS[0], STEPS[1], [STEPS[2][0]]]
    args, cpu_model, records, eval_rec = _run_loop(mode, fused, fused_opt, steps)
    what = f"{mode} {'fused' if fused else 'modules'} {'FusedAdamW' if fused_opt else 'torch AdamW'}"
    _check_records(mode, args, cpu_model, records, eval_rec, bn_stats, what)
