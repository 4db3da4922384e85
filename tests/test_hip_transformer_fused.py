"""The Transformer baseline's fused step (`model.fused_step`: engine.py on the driver's encoder-only mode, csrc/model.hip) on the GPU:
the step is ONE gt_model_forward call; it computes what the module path computes on the same weights (F32_TOL / BF16_TOL of
tests/test_hip_gnn_baseline.py), what the float64 statement of tests/test_transformer_baseline_host.py says (the bars of
tests/test_hip_configs.py) and what tests/golden/transformer_baseline_ref.json recorded from the reference; it is deterministic; what it
does not cover keeps today's path bit for bit; eval, dropout, FLAG and two AdamW steps; and the driver's refusals through the C ABI.
Shapes, builders and tolerances are those of tests/test_hip_transformer_baseline.py.
"""
import copy
import ctypes as C

import pytest
import torch

import test_hip_configs as thc
from test_hip_configs import BOUNDS, check_grads, precision_report
from test_hip_gnn_baseline import BF16_TOL, F32_TOL, _close
from test_hip_transformer_baseline import CASES, _build, _oracle_run, _perturb, _targs, embed_calls  # noqa: F401  (embed_calls: a fixture)
from test_transformer_baseline_host import fixture_batch, fixture_loss, load_fixture
from test_transformer_fused_host import INVALID, _batch as _c_batch, _enc_only_model, _prepare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FUSED_CASES = [c for c in CASES if not (c["feat"] == "tud" and c.get("perturb"))] + [dict(feat="tud"), dict(feat="tud", bf16=True)]
IDS = [",".join(f"{k}={v}" for k, v in c.items()) for c in FUSED_CASES]


@pytest.fixture
def calls(monkeypatch, embed_calls):
    """counts gt_model_forward, ops.embed_tokens (the existing `embed_calls` fixture) and ops.seq_gather"""
    from graphtrans_amd import _lib, ops
    lib = _lib.lib()
    n = dict(forward=0, embed=embed_calls, gather=[])
    real_fwd, real_gather = lib.gt_model_forward, ops.seq_gather

    class Lib:   # the engine looks the entry point up on the library object at every call
        def __getattr__(self, k):
            return getattr(lib, k)

        def gt_model_forward(self, *a):
            n["forward"] += 1
            return real_fwd(*a)

    def gather(*a, **kw):
        n["gather"].append(1)
        return real_gather(*a, **kw)
    proxy = Lib()
    monkeypatch.setattr(_lib, "lib", lambda: proxy)
    monkeypatch.setattr(ops, "seq_gather", gather)
    return n


def _run(model, b, loss_of, fused_step, perturb=None, fused_flag=None):
    model.fused_step = fused_step
    model.fused_flag = fused_step if fused_flag is None else fused_flag
    for p in model.parameters():
        p.grad = None
    pt = None if perturb is None else perturb.clone().requires_grad_(True)
    out = model(b, pt)
    loss = loss_of(out)
    loss.backward()
    outs = [o.detach().float().clone() for o in (out if isinstance(out, (list, tuple)) else [out])]
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    return outs, loss.detach().clone(), grads, None if pt is None else pt.grad.clone()


def _case(kw):
    kw = dict(kw)
    feat, with_perturb, bf16 = kw.pop("feat"), kw.pop("perturb", False), kw.pop("bf16", False)
    if bf16:
        kw["compute_dtype"] = torch.bfloat16
    model, b, loss_of = _build(feat, _targs(**kw))
    return feat, model, b, loss_of, (_perturb(b, 64) if with_perturb else None), (BF16_TOL if bf16 else F32_TOL)


def _subset(b, keep):
    """the batch `b` without the nodes where `keep` is False (every graph keeps a node); the edges are not this model's input"""
    from graphtrans_amd.data import Batch
    d = {k: v for k, v in b.__dict__.items() if not k.startswith("_gt") and k != "_sizes"}
    d["x"], d["batch"] = b.x[keep].contiguous(), b.batch[keep].contiguous()
    if getattr(b, "node_depth", None) is not None:
        d["node_depth"] = b.node_depth[keep].contiguous()
    d["edge_index"], d["edge_attr"] = torch.zeros((2, 0), dtype=torch.int64, device=b.x.device), None
    return Batch(**d)


def _first_graph_one_node(b):
    keep = torch.ones_like(b.batch, dtype=torch.bool)
    keep[1:int((b.batch == 0).sum())] = False
    return _subset(b, keep)


def _single_graph(b, g):
    """graph `g` of the batch on its own (the callers' loss reads no labels)"""
    out = _subset(b, b.batch == g)
    out.batch = torch.zeros_like(out.batch)
    out._num_graphs = 1
    return out


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b)) and len(a) == len(b)


# ---- 1. the step is the driver's ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feat", ["ast", "mol", "tud"])
def test_the_fused_step_is_one_driver_call(feat, calls):
    from graphtrans_amd import engine
    model, b, loss_of = _build(feat, _targs())
    model.fused_step = True
    assert engine.eligible(model, b, None)
    _run(model, b, loss_of, True)
    assert calls["forward"] == 1 and not calls["embed"] and not calls["gather"]
    _run(model, b, loss_of, False)
    assert calls["forward"] == 1
    assert (len(calls["embed"]), len(calls["gather"])) == ((0, 1) if feat == "tud" else (1, 0))   # what they are today
    assert not engine.eligible(model, b, None)


# ---- 2. / 7. fused against the module path on the same weights, training and eval ---------------------------------------------------
@pytest.mark.parametrize("kw", FUSED_CASES, ids=IDS)
def test_fused_step_matches_the_module_path(kw, calls):
    feat, model, b, loss_of, perturb, tol = _case(kw)
    o0, l0, g0, p0 = _run(copy.deepcopy(model), b, loss_of, False, perturb)
    assert calls["forward"] == 0
    o1, l1, g1, p1 = _run(model, b, loss_of, True, perturb)
    assert calls["forward"] == 1
    assert torch.allclose(l0, l1, **tol), (l0, l1)
    assert len(o0) == len(o1)
    for i, (u, v) in enumerate(zip(o0, o1)):
        _close(u, v, tol, f"logits {i}")
    assert set(g0) == set(g1)
    for n in g0:
        _close(g0[n], g1[n], tol, n)
    if perturb is not None:
        _close(p0, p1, tol, "perturb.grad")
        assert p1.dtype == torch.float32 and p1.shape == perturb.shape
        sizes = torch.bincount(b.batch)
        dropped = torch.cat([torch.arange(int(n), device=DEV) < int(n) - 20 for n in sizes])   # the leading nodes of a truncated graph
        assert bool(dropped.any()) and float(p1[dropped].abs().max()) == 0.0 and float(p1[~dropped].abs().max()) > 0
    # eval under no_grad: the training-mode logits (p = 0), on both paths
    model.eval()
    with torch.no_grad():
        a = model(b, perturb)
        model.fused_step = False
        c = model(b, perturb)
    assert calls["forward"] == 2
    for u, v, w in zip(a if isinstance(a, (list, tuple)) else [a], c if isinstance(c, (list, tuple)) else [c], o1):
        _close(u.float(), w, tol, "eval logits vs training logits")
        _close(u.float(), v.float(), tol, "eval logits vs the module path")


@pytest.mark.parametrize("shape", ["single-graph", "first-graph-one-node", "host-sizes"])
@pytest.mark.parametrize("feat", ["ast", "mol", "tud"])
def test_fused_step_on_edge_batches(feat, shape, calls):
    """a batch of one (truncated) graph, a batch whose first graph has one node, and per-graph sizes known on the host (the layout
    staged through the ring instead of built on the device)"""
    model, b, _ = _build(feat, _targs(max_seq_len=None))
    if shape == "single-graph":
        b = _single_graph(b, int(torch.bincount(b.batch).argmax()))
        assert b.batch.numel() > 20
    elif shape == "first-graph-one-node":
        b = _first_graph_one_node(b)
        assert int((b.batch == 0).sum()) == 1
    else:
        b._sizes = torch.bincount(b.batch).cpu().numpy()
    sq = lambda out: out.float().square().mean()
    perturb = _perturb(b, 64) if feat != "tud" else None
    twin = copy.deepcopy(model)
    b0 = copy.copy(b)
    o0, l0, g0, p0 = _run(twin, b0, sq, False, perturb)
    o1, l1, g1, p1 = _run(model, b, sq, True, perturb)
    assert calls["forward"] == 1
    _close(o0[0], o1[0], F32_TOL, "logits")
    for n in g0:
        _close(g0[n], g1[n], F32_TOL, n)
    if perturb is not None:
        _close(p0, p1, F32_TOL, "perturb.grad")


# ---- 3. against the float64 statement -------------------------------------------------------------------------------------------------
def test_fused_step_fp32_vs_float64_statement(monkeypatch, calls):
    """test_hip_transformer_baseline.test_transformer_fp32_vs_float64_statement's cls case with `fused_step` on: logits within 1e-4,
    BOUNDS["fp32"] on the precision report, every gradient through check_grads with the fp32_noise model of this model's oracle"""
    from graphtrans_amd import losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.transformer import Transformer
    from oracle import reference_math as rm
    monkeypatch.setattr(thc, "oracle_run", _oracle_run)
    torch.manual_seed(5)
    args = _targs(max_seq_len=5, max_input_len=40)
    model = Transformer(50, ASTNodeEncoder(64, 98, 300, 20), None, args)
    b = synth.code2_like(B=16, seed=5, num_nodeattributes=300, num_vocab=50)
    oloss, hloss = (lambda out: rm.code2_loss(out, b.y_arr)), (lambda out, bd: losses.code2_loss(out, bd.y_arr))
    model.fused_step = True
    ref_out, ref_loss, ref_g = _oracle_run(model, args, b, oloss, torch.float64)
    noise = thc.fp32_noise(model, args, b, oloss, ref_g)
    _, o32_loss, o32_g = _oracle_run(model, args, b, oloss, torch.float32)
    o32 = precision_report(o32_g, o32_loss, ref_g, ref_loss)
    outs, loss, grads = thc.hip_run(model, b, hloss, torch.float32)
    assert calls["forward"] == 1 and not calls["embed"]
    refs = [o.detach() for o in ref_out]
    top = max(float(r.abs().max()) for r in refs)
    lerr = max(float((o.double() - r).abs().max()) for o, r in zip(outs, refs))
    rep = precision_report(grads, loss, ref_g, ref_loss)
    print(f"\n[transformer fused step] logits: max |err| {lerr:.2e} (largest logit {top:.2f}); loss rel {rep['loss_rel_err']:.2e}; grad rel-L2 "
          f"worst {rep['grad_rel_l2_worst']:.2e} ({rep['grad_rel_l2_worst_param']}) median {rep['grad_rel_l2_median']:.2e}; fp32 oracle "
          f"itself: worst {o32['grad_rel_l2_worst']:.2e} median {o32['grad_rel_l2_median']:.2e}")
    assert 0.1 <= top <= 100.0, top
    assert lerr <= 1e-4, lerr
    bound = BOUNDS["fp32"]
    assert rep["loss_rel_err"] <= bound["loss"] and rep["grad_rel_l2_worst"] <= bound["worst"], rep
    assert rep["grad_rel_l2_median"] <= max(bound["median"], 3.0 * o32["grad_rel_l2_median"]), (rep, o32)
    check_grads(grads, ref_g, noise, what="transformer fused step fp32")


# ---- 4. against the recorded reference -------------------------------------------------------------------------------------------------
def test_fused_step_equals_the_recorded_reference(calls):
    """every cls case of tests/golden/transformer_baseline_ref.json (recorded with a perturbation: `fused_flag` on), by the rule of
    test_transformer_equals_the_recorded_reference: logits within 1e-4, gradients within check_grads' bars at noise 0, d perturb at
    F32_TOL.  The fixture's batch carries its per-graph sizes: the layout goes through the staging ring."""
    from test_transformer_baseline_host import _build as host_build
    ran = 0
    for c in load_fixture():
        if c["args"].graph_pooling != "cls":
            continue
        model = host_build(c["args"], c["feat"])
        model.load_state_dict(c["sd"], strict=True)
        model = model.to(DEV).train()
        b = fixture_batch(c["inputs"]).to(DEV)
        perturb = c["inputs"]["perturb"].to(DEV)
        n0 = calls["forward"]
        outs, _, grads, dp = _run(model, b, fixture_loss, True, perturb)
        assert calls["forward"] == n0 + 1, c["name"]
        assert len(outs) == len(c["logits"])
        for o, r in zip(outs, c["logits"]):
            assert float((o.cpu() - r).abs().max()) <= 1e-4, c["name"]
        check_grads({k: v.cpu() for k, v in grads.items()}, {k: v.double() for k, v in c["grads"].items()},
                    {k: 0.0 for k in c["grads"]}, what=f"recorded reference {c['name']} fused_step")
        _close(c["perturb_grad"], dp.cpu(), F32_TOL, f"{c['name']} perturb grad")
        ran += 1
    assert ran >= 1


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(feat="ast"), dict(feat="ast", perturb=True), dict(feat="mol", perturb=True), dict(feat="tud"),
                                dict(feat="mol", bf16=True)], ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_fused_step_is_deterministic(kw):
    _, model, b, loss_of, perturb, _ = _case(kw)
    o0, l0, g0, p0 = _run(model, b, loss_of, True, perturb)
    o1, l1, g1, p1 = _run(model, b, loss_of, True, perturb)
    assert _same(o0, o1) and torch.equal(l0, l1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    if perturb is not None:
        assert torch.equal(p0, p1)


# ---- 6. fallbacks keep today's path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["mean-pooling", "big-table", "frozen-parameter", "tensor-hook", "tud-perturb", "perturb-without-fused_flag"])
def test_what_the_fused_step_does_not_cover_keeps_the_module_path(what, calls):
    from graphtrans_amd import engine
    feat, kw, attrs = "ast", {}, 300
    if what == "mean-pooling":
        kw = dict(graph_pooling="mean", max_seq_len=None)
    elif what == "big-table":
        attrs = 20000
    elif what == "tud-perturb":
        feat = "tud"
    model, b, loss_of = _build(feat, _targs(**kw), attrs=attrs)
    if kw.get("graph_pooling") == "mean":
        loss_of = lambda out: out.float().square().mean()
    perturb = _perturb(b, 64) if "perturb" in what else None
    flag = what != "perturb-without-fused_flag"
    if what == "frozen-parameter":
        model.transformer.cls_embedding.requires_grad_(False)
    if what == "tensor-hook":
        model.graph_pred_linear_list[0].bias.register_hook(lambda g: g)
    twin = copy.deepcopy(model)
    if what == "tensor-hook":
        twin.graph_pred_linear_list[0].bias.register_hook(lambda g: g)

    def run(m, fused):
        m.fused_step, m.fused_flag = fused, fused and flag
        pt = None if perturb is None else perturb.clone().requires_grad_(True)
        out = m(b, pt)
        loss_of(out).backward()
        outs = [o.detach().clone() for o in (out if isinstance(out, (list, tuple)) else [out])]
        return outs, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}, None if pt is None else pt.grad.clone()

    model.fused_step, model.fused_flag = True, flag
    assert not engine.eligible(model, b, None if perturb is None else perturb.clone().requires_grad_(True))
    o1, g1, p1 = run(model, True)
    o0, g0, p0 = run(twin, False)
    assert calls["forward"] == 0
    assert _same(o0, o1) and set(g0) == set(g1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    if perturb is not None:
        assert torch.equal(p0, p1)


# ---- 7. evaluate() ---------------------------------------------------------------------------------------------------------------------
def test_evaluate_gives_the_same_accuracy_on_both_paths(calls):
    from graphtrans_amd.evaluate import TudAccuracy, evaluate
    model, b, _ = _build("tud", _targs())
    batches = [b, _first_graph_one_node(b)]
    for x in batches:
        x.y = b.y
    n = sum(int(x.batch.max()) + 1 for x in batches)
    model.fused_step = True
    acc1 = evaluate(model, batches, TudAccuracy(n, DEV))
    assert calls["forward"] == 2 and model.training
    model.fused_step = False
    acc0 = evaluate(model, batches, TudAccuracy(n, DEV))
    assert calls["forward"] == 2
    assert acc0 == acc1 and 0.0 <= acc1["acc"] <= 1.0


# ---- 8. dropout is wired ---------------------------------------------------------------------------------------------------------------
def test_dropout_reaches_the_encoder_layers(calls):
    model, b, _ = _build("mol", _targs(transformer_dropout=0.1))
    ref, _, _ = _build("mol", _targs(transformer_dropout=0.0))
    ref.load_state_dict(model.state_dict())
    model.fused_step = ref.fused_step = True

    def fwd(m, seed=7):
        torch.manual_seed(seed)
        with torch.no_grad():
            return m(b).float().clone()
    a, c = fwd(model.train()), fwd(model.train())
    p0 = fwd(ref.train())
    assert torch.equal(a, c)
    assert not torch.equal(a, fwd(model, seed=8))
    assert float((a - p0).abs().max()) > 1e-3
    assert torch.equal(fwd(model.eval()), fwd(ref.eval()))
    assert calls["forward"] == 6


# ---- 9. FLAG ---------------------------------------------------------------------------------------------------------------------------
def test_flag_step_stays_on_the_fused_step(calls):
    """flag.flag_step (m = 3) with `fused_step` + `fused_flag` against the same three passes on a twin with both off: the last loss,
    perturb.grad, the accumulated gradients and the parameters after the step at F32_TOL, as the module path's flag_step test"""
    from graphtrans_amd import flag, losses
    m, step = 3, 8e-3
    model, b, _ = _build("ast", _targs())
    y = torch.randint(0, 50, (12, 5), generator=torch.Generator().manual_seed(1)).to(DEV)
    calc = lambda out, batch: losses.code2_loss(out, y)
    twin = copy.deepcopy(model)
    model.fused_step = model.fused_flag = True
    start = (torch.rand(b.batch.numel(), 64, generator=torch.Generator().manual_seed(3)) * 2 - 1).mul_(step).to(DEV)
    pa, pb = start.clone(), start.clone()
    loss_a = flag.flag_step(model, b, torch.optim.SGD(model.parameters(), lr=0.05), calc, m=m, step_size=step, perturb=pa)
    assert calls["forward"] == m and not calls["embed"] and not calls["gather"]
    loss_b = flag.flag_step(twin, b, torch.optim.SGD(twin.parameters(), lr=0.05), calc, m=m, step_size=step, perturb=pb)
    assert calls["forward"] == m and len(calls["embed"]) == m
    assert torch.allclose(loss_a, loss_b, **F32_TOL), (loss_a, loss_b)
    _close(pb.grad, pa.grad, F32_TOL, "perturb.grad")
    moved = (pa.detach() - pb.detach()).abs() > 1e-9   # a sign flipped by rounding in a gradient of ~0 moves an element by 2 * step
    assert float(moved.float().mean()) <= 1e-3, float(moved.float().mean())
    assert float((pa.detach() - start).abs().max()) > 0
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        _close(q.grad, p.grad, F32_TOL, n + ".grad")
        _close(q.detach(), p.detach(), F32_TOL, n)


# ---- 10. two AdamW steps ---------------------------------------------------------------------------------------------------------------
def test_two_adamw_steps_match_the_module_path(calls):
    """a gradient written at a wrong offset of the flat buffer moves the wrong parameter: after each of two FusedAdamW steps every
    parameter agrees with the twin's on the module path.
    eps = 1e-4: AdamW's first steps are lr * g / (|g| + eps).  The key bias of every attention layer has a gradient of exactly zero in
    exact arithmetic (softmax ignores a shift of all scores of a row), so what both paths compute there is rounding noise (<= 1e-7);
    with the default eps = 1e-8 the optimizer would normalise that noise into steps of +-lr whose sign is arbitrary.  1e-4 lies
    between the noise and the gradients that mean something (>= 1e-3 of the largest here): a gradient at a wrong offset still moves
    the wrong parameter by about lr = 1e-3, a hundred times F32_TOL on parameters of O(0.1)."""
    from graphtrans_amd.optim import FusedAdamW
    model, b, loss_of = _build("ast", _targs())
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    twin = copy.deepcopy(model)
    model.fused_step = True
    kw = dict(lr=1e-3, weight_decay=0.01, eps=1e-4)
    oa, ob = FusedAdamW(model.parameters(), **kw), FusedAdamW(twin.parameters(), **kw)
    for step in range(2):
        for mod, opt in ((model, oa), (twin, ob)):
            opt.zero_grad(set_to_none=True)
            loss_of(mod(b)).backward()
            opt.step()
        assert calls["forward"] == step + 1
        for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
            _close(q.detach(), p.detach(), F32_TOL, f"step {step} {n}")
            assert not torch.equal(p.detach(), before[n].detach()), n   # every parameter moved


# ---- 11. the driver's refusals, through the C ABI --------------------------------------------------------------------------------------
def test_the_driver_refuses_before_any_launch():
    """gt_model_prepare is where the mode is checked: GT_ERR_INVALID_ARG with a message, and no forward can follow a failed prepare"""
    cases = []
    cm, k0 = _enc_only_model()
    cm.enc_only = 0
    cases.append(("L == 0 without the mode flag", cm, _c_batch()[0]))
    cm, k1 = _enc_only_model()
    cm.readout = 2
    cases.append(("the mode with readout", cm, _c_batch()[0]))
    cm, k2 = _enc_only_model()
    bt = _c_batch()[0]
    bt.gnn_frozen = 1
    cases.append(("the mode with gnn_frozen", cm, bt))
    cm, k3 = _enc_only_model(embed_kind=1)
    bt = _c_batch(linear=True)[0]
    bt.perturb = 0x70000
    cases.append(("the mode with perturb and the Linear encoder", cm, bt))
    from graphtrans_amd import _lib
    for what, cm, bt in cases:
        rc, _, err = _prepare(cm, bt)
        assert rc == INVALID and err, (what, rc, err)
        # the context of a refused prepare takes no forward: the entry point returns the same error class, nothing is enqueued
        ctx = C.create_string_buffer(int(_lib.lib().gt_model_ctx_bytes()))
        assert _lib.lib().gt_model_forward(C.byref(cm), ctx, 0x1000, 0x2000, None) == INVALID, what
    torch.cuda.synchronize()
