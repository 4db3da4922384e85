"""FLAG on the fused step (`fused_flag`, engine._perturb_ok): forward(batched_data, perturb) as one autograd node that adds the
perturbation inside the input encoder and hands d h_list[0] out as its gradient; gt_flag_ascent and gt_embed_sum_fwd_add through the
C ABI; graphtrans_amd.flag.flag_step, every one of its backwards held to the float64 oracle at the run's own perturbation."""
import copy
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import test_hip_configs as thc
from test_gnn_baseline_host import gnn_statement
from test_hip_configs import check_grads
from test_hip_engine import _args
from test_hip_gnn_baseline import _gargs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32_TOL = dict(rtol=1e-4, atol=1e-6)
BF16_TOL = dict(rtol=2e-2, atol=2e-3)
UNSUPPORTED = -2
GUARD = 64
SENT = -12345.0
D = 64


# =====================================================================================================================================
# kernels, through the C ABI
# =====================================================================================================================================
def _guarded(n, fill=SENT):
    buf = torch.full((n + GUARD,), fill, dtype=torch.float32, device=DEV)
    return buf, buf[:n]


def _bits(t):
    return t.contiguous().view(torch.int32)


FLAG_GRID_ELEMS = 2048 * 256 * 4   # what one full grid of k_flag_ascent covers (csrc/flag.hip): above it the stride loop takes a second trip


@pytest.mark.parametrize("n", [4, 8, 1020, 1024, 1028, FLAG_GRID_ELEMS + 4])
def test_flag_ascent_is_torchs_formula_bit_for_bit(n):
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    g = torch.Generator().manual_seed(n)
    grad = torch.randn(n, generator=g)
    i = torch.arange(n)
    grad[i % 8 == 0] = grad[i % 8 == 0].abs() + 0.1            # +
    grad[i % 8 == 1] = -grad[i % 8 == 1].abs() - 0.1           # -
    grad[i % 8 == 2] = 0.0                                     # +0
    grad[i % 8 == 3] = -0.0                                    # -0
    grad[i % 8 == 4] = 1e-40                                   # a denormal
    grad[i % 8 == 5] = float("inf")
    grad[i % 8 == 6] = float("-inf")
    if n >= 8:
        grad[7] = float("nan")                                 # one NaN
    perturb = torch.randn(n, generator=g) * 1e-2
    step = 8e-3
    pbuf, p = _guarded(n)
    gbuf, gr = _guarded(n)
    p.copy_(perturb)
    gr.copy_(grad)
    want = p.clone() + step * torch.sign(gr.clone())
    _lib.check(_lib.lib().gt_flag_ascent(p.data_ptr(), gr.data_ptr(), n, step, _stream()), "gt_flag_ascent")
    torch.cuda.synchronize()
    assert torch.equal(_bits(p), _bits(want))
    assert not bool(torch.isnan(p).any())                      # torch.sign(NaN) is 0: the element stays where it was
    assert bool((_bits(gr) == 0).all())                        # every element +0
    assert bool((pbuf[n:] == SENT).all()) and bool((gbuf[n:] == SENT).all())


def test_flag_ascent_refuses_a_count_that_is_no_multiple_of_4():
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    pbuf, p = _guarded(8, 1.0)
    gbuf, gr = _guarded(8, 1.0)
    assert _lib.lib().gt_flag_ascent(p.data_ptr(), gr.data_ptr(), 6, 0.5, _stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((pbuf == 1.0).all()) and bool((gbuf == 1.0).all())


def _embed_call(name, tabs, idx, N, Dm, add, add_before):
    """tabs: list of fp32 [rows][Dm]; idx: list of (int64 tensor, stride); -> out [N][Dm] behind a guard"""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    T = len(tabs)
    I64, P = C.c_int64 * T, C.c_void_p * T
    ip = P(*[t.data_ptr() for t, _ in idx])
    st = I64(*[s for _, s in idx])
    cl = I64(*[-1] * T)
    tp = P(*[t.data_ptr() for t in tabs])
    buf, out = _guarded(N * Dm, float("nan"))
    if name == "gt_embed_sum_fwd":
        rc = _lib.lib().gt_embed_sum_fwd(T, ip, st, cl, tp, N, Dm, out.data_ptr(), _stream())
    else:
        rc = _lib.lib().gt_embed_sum_fwd_add(T, ip, st, cl, tp, add.data_ptr() if add is not None else None, add_before, N, Dm,
                                             out.data_ptr(), _stream())
    _lib.check(rc, name)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[N * Dm:]).all()), "a store behind the end of the output"
    return out.view(N, Dm)


@pytest.mark.parametrize("vn", [False, True], ids=["plain", "virtual"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("Dm", [4, 260])
@pytest.mark.parametrize("N", [1, 5, 257])
def test_embed_sum_fwd_add_is_the_fp32_chain(N, Dm, T, vn):
    g = torch.Generator().manual_seed(1000 * N + 10 * Dm + T)
    rows = [7, 11, 5][:T]
    tabs = [torch.randn(r, Dm, generator=g).to(DEV) for r in rows]
    x = torch.stack([torch.randint(0, r, (N,), generator=g) for r in rows], 1).to(DEV)   # [N][T] int64
    idx = [(x[:, t], T) for t in range(T)]
    perturb = (torch.randn(N, Dm, generator=g) * 0.1).to(DEV)
    want = tabs[0][x[:, 0]]
    for t in range(1, T):
        want = want + tabs[t][x[:, t]]
    want = want + perturb
    plain_tabs, plain_idx = list(tabs), list(idx)
    if vn:   # one more table with a stride-0 index: the virtual-node row, behind the perturbation
        vrow = torch.randn(1, Dm, generator=g).to(DEV)
        zero = torch.zeros(1, dtype=torch.int64, device=DEV)
        tabs, idx = tabs + [vrow], idx + [(zero, 0)]
        want = want + vrow
    got = _embed_call("gt_embed_sum_fwd_add", tabs, idx, N, Dm, perturb, T)
    assert torch.equal(_bits(got), _bits(want))
    # add == NULL is gt_embed_sum_fwd
    a = _embed_call("gt_embed_sum_fwd_add", tabs, idx, N, Dm, None, 0)
    b = _embed_call("gt_embed_sum_fwd", tabs, idx, N, Dm, None, 0)
    assert torch.equal(_bits(a), _bits(b))
    # in front of every table, and behind all of them
    first = _embed_call("gt_embed_sum_fwd_add", plain_tabs, plain_idx, N, Dm, perturb, 0)
    w0 = perturb + plain_tabs[0][x[:, 0]]
    for t in range(1, T):
        w0 = w0 + plain_tabs[t][x[:, t]]
    assert torch.equal(_bits(first), _bits(w0))


# =====================================================================================================================================
# models
# =====================================================================================================================================
class Case:
    """a model on the CPU with its batch, losses and oracle; .dev() -> (model, batch) on the GPU"""

    def __init__(self, name):
        from graphtrans_amd import losses, synth
        from graphtrans_amd.encoders import ASTNodeEncoder, AtomEncoder, BondEncoder
        from graphtrans_amd.models.gnn import GNN
        from graphtrans_amd.models.gnn_transformer import GNNTransformer
        from graphtrans_amd.models.pna_transformer import PNATransformer
        from oracle import reference_math as rm
        kw = dict(CASES[name])
        feat, kind, small = kw.pop("feat", "ast"), kw.pop("kind", "gt"), kw.pop("small", False)
        self.pseed = kw.pop("pseed", 4)
        self.name, self.kind, self.bf16 = name, kind, kw.get("compute_dtype") == torch.bfloat16
        torch.manual_seed(0)
        if kind == "pna":   # test_hip_frozen_gnn._pna, built on the CPU (the oracle and its noise model read the parameters there)
            torch.manual_seed(11)
            self.args = _pna_args(fused_flag=True, **kw)
            b = synth.code2_like(B=24, seed=2, mean_nodes=20.0, max_nodes=60)
            model = PNATransformer(50, ASTNodeEncoder(D, 98, 10030, 20), None, self.args)
        else:
            args = _gargs(fused_flag=True, **kw) if kind == "gnn" else _args(transformer_dropout=0.0, fused_flag=True, **kw)
            cls = GNN if kind == "gnn" else GNNTransformer
            if feat == "ast":
                model = cls(50, ASTNodeEncoder(D, 98, 300, 20), lambda d: torch.nn.Linear(2, d), args)
                b = synth.code2_like(B=12, seed=5, num_nodeattributes=300, **(dict(mean_nodes=14.0, max_nodes=24) if small else {}))
            elif feat == "mol":
                args.max_seq_len = None
                model = cls(16, AtomEncoder(D), lambda d: BondEncoder(d), args)
                b = synth.molpcba_like(B=24, seed=4)
            else:
                args.max_seq_len = None
                model = cls(2, torch.nn.Linear(37, D), lambda d: (lambda _e: 0), args)
                b = synth.nci1_like(B=16, seed=3)
            self.args = args
        self.feat = feat
        with torch.no_grad():   # non-trivial BatchNorm affine / biases and virtual-node embedding
            g = torch.Generator().manual_seed(3)
            for p in model.parameters():
                if p.dim() == 1:
                    p.add_(torch.randn(p.shape, generator=g) * 0.1)
            if getattr(self.args, "gnn_virtual_node", False):
                model.gnn_node.virtualnode_embedding.weight.copy_(torch.randn(1, D, generator=g) * 0.3)
        self.model, self.b = model.train(), b
        gy = torch.Generator().manual_seed(1)
        B = int(b.batch[-1]) + 1
        msl = getattr(self.args, "max_seq_len", None)
        # the oracle's losses stay in the dtype of its logits (rm.code2_loss / rm.mol_loss narrow them to fp32)
        if feat == "mol":
            y = (torch.rand(B, 16, generator=gy) > 0.5).float()
            y[torch.rand(B, 16, generator=gy) < 0.2] = float("nan")
            self.oloss, self.hloss = (lambda out: _bce(out, y)), (lambda out: losses.mol_loss(out, self._y(y)))
        elif feat == "tud":
            self.oloss, self.hloss = (lambda out: rm.tud_loss(out, b.y)), (lambda out: losses.tud_loss(out, self._y(b.y)))
        elif msl is None:
            self.oloss, self.hloss = (lambda out: out.square().mean()), (lambda out: out.float().square().mean())
        else:
            y = torch.randint(0, 50, (B, msl), generator=gy)
            self.oloss, self.hloss = (lambda out: _ce(out, y)), (lambda out: losses.code2_loss(out, self._y(y)))
        self.N = int(b.batch.numel())
        self._ydev = {}

    def _y(self, y):
        t = self._ydev.get(id(y))
        if t is None:
            t = self._ydev[id(y)] = y.to(DEV)
        return t

    def dev(self):
        return copy.deepcopy(self.model).to(DEV).train(), copy.copy(self.b).to(DEV)

    def perturb(self, seed=None, scale=0.1):
        seed = self.pseed if seed is None else seed
        # (seed 4: with seeds 2 and 3 the virtual-node models of the 1417-row batch sit on a ReLU kink -- the fp32 ORACLE alone is then
        # 1e-4 .. 1e-3 of a tensor's largest entry from float64 on the layer-0 / layer-1 edge-encoder gradients, with seed 4 it is at
        # 4e-6 .. 6e-6 on every case; measured on the CPU.  The seed moved, the bars did not: tests/test_hip_training_steps.py)
        return (torch.randn(self.N, D, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV).requires_grad_(True)

    def oracle(self, model, perturb, dtype=torch.float64, scale=1.0):
        """-> (outputs, loss, {parameter: gradient, "perturb": d loss / d perturb}) of the oracle at `model`'s parameters and `perturb`"""
        from oracle import reference_math as rm
        sd = {k: (v.detach().cpu().to(dtype).requires_grad_(True) if v.is_floating_point() else v.detach().cpu().clone())
              for k, v in model.state_dict().items()}
        oargs = SimpleNamespace(**{k: v for k, v in vars(self.args).items() if k not in ("compute_dtype", "token_layout", "fused_flag")})
        bb = copy.copy(self.b)
        for k in ("x", "edge_attr"):
            v = getattr(bb, k, None)
            if v is not None and v.is_floating_point():
                setattr(bb, k, v.to(dtype))
        pt = perturb.detach().cpu().to(dtype).requires_grad_(True)
        fwd = {"gt": rm.gnn_transformer, "pna": rm.pna_transformer, "gnn": gnn_statement}[self.kind]
        torch.set_default_dtype(dtype)
        try:
            out = fwd(sd, oargs, bb, pt, True)
            loss = self.oloss(out) * scale
            loss.backward()
        finally:
            torch.set_default_dtype(torch.float32)
        grads = {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.requires_grad and v.grad is not None}
        grads["perturb"] = pt.grad
        return out, loss.detach(), grads


def _ce(out, y):
    import torch.nn.functional as F
    return sum(F.cross_entropy(p, y[:, i]) for i, p in enumerate(out)) / len(out)


def _bce(out, y):
    import torch.nn.functional as F
    lab = y == y
    return F.binary_cross_entropy_with_logits(out[lab], y.to(out.dtype)[lab])


def _pna_args(**kw):
    from oracle import reference_math as rm
    return rm.default_args(gnn_virtual_node=False, gnn_num_layer=3, gnn_emb_dim=64, gnn_JK="last", gnn_residual=True,
                           gnn_dropout=0.0, d_model=64, nhead=4, dim_feedforward=128, transformer_dropout=0.0,
                           num_encoder_layers=2, transformer_norm_input=True, graph_pooling="cls", max_seq_len=3,
                           aggregators=["mean", "max", "min", "std"], scalers=["identity", "amplification", "attenuation"],
                           deg=torch.tensor([0, 40, 25, 9, 3]), **kw)


# code2_like(B=12, seed=5) has 1417 node rows: above the 1024 rows from which the weight images are bound, so the image-backed dX GEMMs
# (with a virtual node) and the GCN form with the BatchNorm statistics in the dX epilogue (without one) write layer 0 there; "small" is
# the same generator at 186 rows, where the small kernels do
CASES = {
    "gcn-virtual-cat": dict(),
    "gcn-virtual-cat-small": dict(small=True),
    "gcn-plain": dict(gnn_virtual_node=False),
    "gcn-plain-small": dict(gnn_virtual_node=False, gnn_JK="last", small=True),
    "gin-virtual": dict(feat="mol", gnn_type="gin"),
    "jk-last": dict(gnn_JK="last"),
    "residual": dict(gnn_residual=True),
    "gnn-dropout": dict(gnn_dropout=0.25),
    "pos-encoder": dict(pos_encoder=True, token_layout="packed"),
    "single-head": dict(max_seq_len=None),
    "gnn-sum": dict(kind="gnn", graph_pooling="sum", small=True),
    # (perturbation seed 5: with seed 4 ONE ReLU gate of GIN layer 0's MLP flips on the fused path -- fused 3.8e-3 of the largest entry of
    # d convs.0.mlp.0.weight from float64, the module path 1.5e-6 --, with seed 7 the same gate flips on the MODULE path -- 2.4e-3 against
    # the fused path's 2.3e-6 --, with seed 5 both are at 2e-6: measured on the GPU, both paths against the float64 oracle)
    "gnn-max": dict(kind="gnn", graph_pooling="max", gnn_type="gin", pseed=5),
    "pna": dict(kind="pna"),
    "linear-encoder": dict(feat="tud"),
    "linear-encoder-plain": dict(feat="tud", gnn_virtual_node=False, gnn_JK="last"),
    "bf16": dict(compute_dtype=torch.bfloat16),
}
NO_ORACLE = ("gnn-dropout", "bf16")   # (the oracle has no dropout mask to share; bf16 is held to the module path only)
_cache = {}


def case(name):
    c = _cache.get(name)
    if c is None:
        c = _cache[name] = Case(name)
    return c


def _close(a, b, tol, what):
    scale = max(1.0, float(a.abs().max()))
    assert torch.allclose(a / scale, b / scale, **tol), (what, float((a - b).abs().max()))


def _run(model, b, c, perturb, fused, seed):
    model.fused = fused
    for p in model.parameters():
        p.grad = None
    perturb.grad = None
    torch.manual_seed(seed)
    out = model(b, perturb)
    loss = c.hloss(out)
    loss.backward()
    torch.cuda.synchronize()
    outs = [o.detach().float().clone() for o in (out if isinstance(out, (list, tuple)) else [out])]
    return outs, loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, \
        {n: t.detach().clone() for n, t in model.named_buffers()}


# ---- 1. routing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gcn-virtual-cat", "gnn-max", "pna", "linear-encoder"])
def test_fused_flag_routes_a_perturbation_to_the_fused_step(name):
    from graphtrans_amd import engine
    from graphtrans_amd.dist import GradSync
    c = case(name)
    model, b = c.dev()
    perturb = c.perturb()
    assert model.fused_flag and engine.eligible(model, b, None)
    assert engine.eligible(model, b, perturb)
    assert engine.eligible(model, b, perturb.detach())              # without requires_grad: the forward only adds
    model.fused_flag = False                                        # the default: a perturbation leaves the fused path
    assert not engine.eligible(model, b, perturb) and engine.eligible(model, b, None)
    model.fused_flag = True
    # what the kernels cannot read
    assert not engine.eligible(model, b, perturb.detach().double())
    assert not engine.eligible(model, b, perturb.detach().cpu())
    assert not engine.eligible(model, b, perturb.detach().t().contiguous().t())
    assert not engine.eligible(model, b, torch.zeros(c.N, D + 4, device=DEV))
    # a frozen gnn_node, with or without fused_freeze
    model.gnn_node.requires_grad_(False)
    assert not engine.eligible(model, b, perturb)
    model.fused_freeze = True
    assert not engine.eligible(model, b, perturb)
    if c.kind != "gnn":
        assert engine.eligible(model, b, None)
    model.gnn_node.requires_grad_(True)
    model.fused_freeze = False
    assert engine.eligible(model, b, perturb)
    # an active GradSync: FLAG under data parallelism stays on the module path
    sync = GradSync(model.parameters(), world_size=1, always_reduce=True).attach(model)
    assert sync.active and not engine.eligible(model, b, perturb) and engine.eligible(model, b, None)
    sync.always_reduce = False
    assert engine.eligible(model, b, perturb)


# ---- 2. fused == module path at the same perturbation and seed ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_fused_flag_matches_module_path(name, monkeypatch):
    from graphtrans_amd import engine, ops
    c = case(name)
    ops.set_matmul_dtype(torch.bfloat16 if c.bf16 else torch.float32)
    try:
        model, b = c.dev()
        ref = copy.deepcopy(model)
        perturb, perturb_ref = c.perturb(), c.perturb()
        assert engine.eligible(model, b, perturb)
        handed = []

        def nan_buffer(N, Dm, dev):   # d perturb starts as NaN: an element layer 0's input-gradient kernel does not write is seen
            t = torch.full((N, Dm), float("nan"), dtype=torch.float32, device=dev)
            handed.append(t)
            return t

        monkeypatch.setattr(engine, "_d_perturb_buffer", nan_buffer)
        o0, l0, g0, b0 = _run(ref, b, c, perturb_ref, False, 7)
        assert not handed
        o1, l1, g1, b1 = _run(model, b, c, perturb, True, 7)
        assert len(handed) == 1 and handed[0].shape == (c.N, D)
        tol = BF16_TOL if c.bf16 else F32_TOL
        assert torch.allclose(l0, l1, **tol), (l0, l1)
        assert set(g0) == set(g1)
        for n in g0:
            _close(g0[n], g1[n], tol, n)
        assert not bool(torch.isnan(perturb.grad).any())
        _close(perturb_ref.grad, perturb.grad, tol, "perturb.grad")
        for n in b0:   # BatchNorm running statistics advance identically
            assert torch.allclose(b0[n].float(), b1[n].float(), rtol=1e-4, atol=1e-6), n
        # a perturbation without requires_grad only adds: same outputs, no d perturb buffer
        handed.clear()
        o2, l2, g2, _ = _run(model, b, c, perturb.detach(), True, 7)
        assert not handed
        assert torch.equal(l1, l2)
        for n in g1:
            assert torch.equal(g1[n], g2[n]), n
        # eval under no_grad (one model, so one set of running statistics, on both paths)
        model.eval()
        with torch.no_grad():
            model.fused = True
            assert engine.eligible(model, b, perturb)
            a = model(b, perturb)
            a = [t.clone() for t in a] if not torch.is_tensor(a) else a.clone()
            model.fused = False
            assert not engine.eligible(model, b, perturb)
            r = model(b, perturb)
        assert not handed
        for u, v in zip(a if not torch.is_tensor(a) else [a], r if not torch.is_tensor(r) else [r]):
            _close(v.float(), u.float(), dict(rtol=2e-2, atol=2e-3) if c.bf16 else dict(rtol=1e-4, atol=1e-5), "eval logits")
    finally:
        ops.set_matmul_dtype(torch.float32)


# ---- 3. against float64 -----------------------------------------------------------------------------------------------------
ORACLE_CASES = [n for n in CASES if n not in NO_ORACLE]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_fused_flag_fp32_vs_float64(name, monkeypatch):
    """exact-fp32 GEMMs: logits and loss within 1e-4; every parameter gradient and d perturb (one more entry of the dictionary) through
    test_hip_configs.check_grads with its shipped base and factor, the noise from that file's fp32_noise on the oracle with the same
    perturbation"""
    from graphtrans_amd import engine
    c = case(name)
    model, b = c.dev()
    perturb = c.perturb()
    ref_out, ref_loss, ref_g = c.oracle(c.model, perturb, torch.float64)
    monkeypatch.setattr(thc, "oracle_run", lambda m, args, bb, loss_of, dtype=torch.float32: c.oracle(m, perturb, dtype))
    noise = thc.fp32_noise(c.model, c.args, c.b, c.oloss, ref_g)
    assert engine.eligible(model, b, perturb)
    outs, loss, grads, _ = _run(model, b, c, perturb, True, 0)
    grads = {k: v.cpu() for k, v in grads.items()}
    grads["perturb"] = perturb.grad.detach().cpu()
    refs = [o.detach() for o in (ref_out if isinstance(ref_out, (list, tuple)) else [ref_out])]
    lerr = max(float((o.cpu().double() - r).abs().max()) for o, r in zip(outs, refs))
    loss_err = abs(float(loss) - float(ref_loss)) / max(1.0, abs(float(ref_loss)))
    print(f"\n[flag {name}] logits max |err| {lerr:.2e}, loss err {loss_err:.2e}")
    assert lerr <= 1e-4, lerr
    assert loss_err <= 1e-4, (float(loss), float(ref_loss))
    check_grads(grads, ref_g, noise, what=f"flag {name} fp32")


# ---- 4. the FLAG loop, teacher-forced --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "modules"])
@pytest.mark.parametrize("name", ["gcn-virtual-cat", "gin-virtual"])
def test_flag_step_teacher_forced(name, fused, monkeypatch):
    """flag_step, m = 3: after each backward the loss, the parameter gradients accumulated so far and perturb.grad against the float64
    oracle at the run's CURRENT perturbation; after each ascent perturb bit for bit against torch's formula on the run's gradient.
    check_grads with noise 0 (its base of 1e-3), as tests/test_hip_gnn_baseline.py::test_five_training_steps holds its steps; with
    the starting perturbation of seed 4 the fp32 oracle's own three backwards are within 6e-6 of float64 on both models (seed 6 meets
    a ReLU kink on the second one: 1.4e-3 and 8.6e-3)."""
    from graphtrans_amd import engine, flag
    from graphtrans_amd.optim import FusedAdamW
    c = case(name)
    model, b = c.dev()
    model.fused_flag = fused
    m, step = 3, 8e-3
    perturb = (torch.rand(c.N, D, generator=torch.Generator().manual_seed(4)) * 2 * step - step).to(DEV)
    assert engine.eligible(model, b, perturb) == fused
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    acc64, losses_seen, ptrs, accum_calls = {}, [], [], []
    done = [0]

    def check_backward():
        torch.cuda.synchronize()
        k = done[0]
        _, l64, g64 = c.oracle(model, perturb, torch.float64, scale=1.0 / m)
        dp64 = g64.pop("perturb")
        for n in g64:
            acc64[n] = g64[n] if n not in acc64 else acc64[n] + g64[n]
        lerr = abs(float(losses_seen[k]) - float(l64)) / max(1.0 / m, abs(float(l64)))
        assert lerr <= 1e-4, (k, float(losses_seen[k]), float(l64))
        got = {n: p.grad.detach().cpu() for n, p in model.named_parameters()}
        got["perturb"] = perturb.grad.detach().cpu()
        want = dict(acc64)
        want["perturb"] = dp64
        check_grads(got, want, {n: 0.0 for n in want}, what=f"flag step {name} {'fused' if fused else 'modules'} backward {k}")
        ptrs.append([p.grad.data_ptr() for p in model.parameters()])
        if fused:
            plan = engine.state(model)["plan"]
            assert engine._grads_are_views(plan.tlist, plan.tviews), k   # `.grad` is still the plan's view
        done[0] += 1

    real_ascent = flag.ascent

    def ascent(p, s):
        check_backward()
        g, p0 = p.grad.detach().clone(), p.detach().clone()
        real_ascent(p, s)
        torch.cuda.synchronize()
        assert torch.equal(_bits(p.detach()), _bits(p0 + s * torch.sign(g)))
        assert bool((_bits(p.grad) == 0).all())

    def calc_loss(out, batch):
        loss = c.hloss(out)
        losses_seen.append(loss.detach() / m)
        return loss

    class Checked:   # the caller's optimizer: the last backward is looked at right in front of its step
        def zero_grad(self, set_to_none=True):
            opt.zero_grad(set_to_none=set_to_none)

        def step(self):
            check_backward()
            opt.step()

    monkeypatch.setattr(flag, "ascent", ascent)
    if fused:
        plan = engine._plan(model)
        real_accum = plan.flat_accum
        monkeypatch.setattr(plan, "flat_accum", lambda: (accum_calls.append(1), real_accum())[1])
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    last = flag.flag_step(model, b, Checked(), calc_loss, m=m, step_size=step, perturb=perturb)
    torch.cuda.synchronize()
    assert done[0] == m and len(losses_seen) == m
    assert torch.equal(last, losses_seen[-1])
    assert ptrs[0] == ptrs[1] == ptrs[2]                     # accumulated in place, on either path
    if fused:
        assert len(accum_calls) == m - 1                     # the second and third backward took the flat-accumulation path
        plan = engine.state(model)["plan"]
        assert sorted(ptrs[0]) == sorted(v.data_ptr() for v in plan.tviews)
    assert any(not torch.equal(before[n], p.detach()) for n, p in model.named_parameters())   # the optimizer stepped


# ---- 5. staged backward, reproducibility ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gcn-virtual-cat", "gcn-plain", "gin-virtual", "linear-encoder", "gnn-max"])
def test_staged_backward_gives_the_same_bits(name, monkeypatch):
    from graphtrans_amd import _lib, engine
    c = case(name)
    model, b = c.dev()
    perturb = c.perturb()

    def run():
        _run(model, b, c, perturb, True, 5)
        return perturb.grad.detach().clone(), engine.state(model)["plan"].flat.clone()

    dp0, flat0 = run()
    dp1, flat1 = run()
    assert torch.equal(_bits(dp0), _bits(dp1)) and torch.equal(_bits(flat0), _bits(flat1))   # two fused runs
    lib = _lib.lib()
    real = lib.gt_model_backward
    seen = []

    def staged(m, ctx, dlogits, grads, barena, stages, stream):
        rcs = [real(m, ctx, dlogits, grads, barena, s, stream) for s in (1, 2, 4)]
        seen.append((stages, rcs))
        return min(rcs)

    monkeypatch.setattr(lib, "gt_model_backward", staged)
    dp2, flat2 = run()
    assert seen == [(7, [0, 0, 0])], seen
    assert torch.equal(_bits(dp0), _bits(dp2)) and torch.equal(_bits(flat0), _bits(flat2))
