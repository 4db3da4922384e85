"""The composite layer entry points of csrc/layers.hip against the float64 references of tests/layer_refs.py, with the dropout masks
replayed from their specification: gt_encoder_layer[_pooled]_* through layers._EncoderLayer, gt_gcn_layer_* and gt_vn_update_* through
layers._GcnLayer / layers._VnUpdate (both halves on a stand-in context, as tests/test_hip_layer_composites.py does), gt_gin_layer_*
through ctypes on a layers.GinLayerDesc with every buffer at exactly the size its `*_bytes` / `*_grad_elems` entry point returns and a
sentinel band behind it.

Every case: the outputs (and the saved / workspace blocks) start as NaN, a second run gives the same bits, the values are compared
with layer_refs.compare_fp32 (fp32 rows: conftest.assert_close at its defaults) or layer_refs.compare_bf16 (bf16 rows: 3 x / 4 x the
distance of the bf16-storage reference Rbf from the float64 one), and the GEMM launch labels are pinned.  tests/test_layer_refs_host.py
shows on the CPU that these comparisons reject every flaw of layer_refs.FLAWS on the same inputs."""
import contextlib
import ctypes as C

import pytest
import torch

import layer_refs as R
from test_hip_layer_composites import _Ctx, recorded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
BAND = 4096

# case: (forward labels, backward labels) -- eval cases run the forward only
LABELS = {
    'enc-i-full-train': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_lin1[fwd]', 'k_lin1[fwd+ln]'],
        ['k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx+lnb]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_linear_dw', 'k_lin1[dx]', 'gate-out dX']),
    'enc-i-full-eval': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_lin1[fwd]', 'k_lin1[fwd+ln]'],
        []),
    'enc-i-pooled-train': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_lin1[fwd]', 'k_lin1[fwd+ln]'],
        ['k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_linear_dw', 'k_lin1[dx]', 'gate-out dX']),
    'enc-i-pooled-eval': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_lin1[fwd]', 'k_lin1[fwd+ln]'],
        []),
    'enc-ii-full-train': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_linear_fwd', 'k_lin1[fwd+ln]'],
        ['k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_linear_dw', 'k_lin1[dx]', 'gate-out dX']),
    'enc-ii-full-eval': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_linear_fwd', 'k_lin1[fwd+ln]'],
        []),
    'enc-ii-pooled-train': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_linear_fwd', 'k_lin1[fwd+ln]'],
        ['k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_linear_dw', 'k_lin1[dx]', 'gate-out dX']),
    'enc-ii-pooled-eval': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_linear_fwd', 'k_lin1[fwd+ln]'],
        []),
    'enc-iii-full-train': (['k_small_fwd', 'k_small_fwd', 'k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw', 'k_small_dw', 'k_small_dx']),
    'enc-iii-full-eval': (['k_small_fwd', 'k_small_fwd', 'k_small_fwd', 'k_small_fwd'],
        []),
    'enc-iii-pooled-train': (['k_small_fwd', 'k_small_fwd', 'k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw', 'k_small_dw', 'k_small_dx']),
    'enc-iii-pooled-eval': (['k_small_fwd', 'k_small_fwd', 'k_small_fwd', 'k_small_fwd'],
        []),
    'enc-ii-full-train-p0.3': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_linear_fwd', 'k_lin1[fwd+ln]'],
        ['k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_linear_dw', 'k_lin1[dx]', 'gate-out dX']),
    'enc-iii-full-train-p0.3': (['k_small_fwd', 'k_small_fwd', 'k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw', 'k_small_dw', 'k_small_dx']),
    'enc-iii-pooled-train-p0.3': (['k_small_fwd', 'k_small_fwd', 'k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw', 'k_small_dw', 'k_small_dx']),
    'enc-i-large': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_lin1[fwd]', 'k_lin2[fwd]'],
        ['k_lin1[dx]', 'k_dw16', 'k_lin2[dx]', 'k_dw16', 'k_lin1[dx]', 'k_dw16', 'k_dw16', 'k_lin1[dx]', 'gate-out dX']),
    'gcn-1-linear-vn-relu-res-p0-train': (['k_small_fwd'],
        ['k_small_dx', 'k_small_dw']),
    'gcn-1-tables-p0.25-train': (['k_small_fwd'],
        ['k_small_dx', 'k_small_dw']),
    'gcn-1-none-vn-relu-res-eval': (['k_small_fwd'],
        []),
    'gcn-1-linear-vn-relu-res-p0.25-train': (['k_small_fwd'],
        ['k_small_dx', 'k_small_dw']),
    'gcn-2-tables-vn-relu-res-p0.25-train': (['k_lin32[fwd]'],
        ['k_lin32[dx]', 'k_lin32_dw']),
    'gcn-2-none-res-p0-train': (['k_lin32[fwd]'],
        ['k_lin32[dx]', 'k_lin32_dw']),
    'gcn-2-linear-vn-p0.25-train': (['k_lin32[fwd]'],
        ['k_lin32[dx]', 'k_lin32_dw']),
    'gcn-2-linear-relu-res-eval': (['k_lin32[fwd]'],
        []),
    'vn-1-res-p0.0': (['k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw']),
    'vn-1-res-p0.25': (['k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw']),
    'vn-1-nores-p0.0': (['k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw']),
    'vn-1-nores-p0.25': (['k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw']),
    'vn-2-res-p0.0': (['k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw']),
    'vn-2-res-p0.25': (['k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw']),
    'vn-2-nores-p0.0': (['k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw']),
    'vn-2-nores-p0.25': (['k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw']),
    'gin-1-p0-train': (['k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw']),
    'gin-1-p0.25-train': (['k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw']),
    'gin-1-eval': (['k_small_fwd', 'k_small_fwd'],
        []),
    'gin-2-p0-train': (['k_lin32[fwd]', 'k_lin32[fwd]'],
        ['k_lin32[dx]', 'k_lin32_dw', 'k_lin32[dx]', 'k_lin32_dw']),
    'gin-2-p0.25-train': (['k_lin32[fwd]', 'k_lin32[fwd]'],
        ['k_lin32[dx]', 'k_lin32_dw', 'k_lin32[dx]', 'k_lin32_dw']),
    'gin-2-eval': (['k_lin32[fwd]', 'k_lin32[fwd]'],
        []),
}
# every fused arm occurs in some case
REQUIRED = ("k_lin1[fwd+ln]", "k_lin1[dx+lnb]", "k_lin2[fwd]", "k_lin2[dx]", "k_dw16", "gate-out dX")


@contextlib.contextmanager
def nan_allocations():
    """torch.empty / torch.empty_like hand out NaN (byte buffers: 0xFF, a NaN in fp32 and in bf16) while the layer ops allocate their
    outputs, saved blocks and workspaces: an element the kernels do not write shows in the comparison"""
    empty, empty_like = torch.empty, torch.empty_like

    def fill(t):
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(255)
        return t

    torch.empty = lambda *a, **k: fill(empty(*a, **k))
    torch.empty_like = lambda *a, **k: fill(empty_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like


def report(case, ratios, fwd, bwd):
    for n, r in ratios.items():
        print(f"RATIO | {case} | {n} | " + (f"{r[0]:.3f} | {r[1]:.3f}" if isinstance(r, tuple) else f"{r:.4f}"))
    print(f"LABELS    {case!r}: ({fwd},\n        {bwd}),")


def same_bits(a, b):
    assert set(a) == set(b)
    for n in a:
        assert bool(torch.isfinite(a[n].float()).all()), f"{n}: not finite (an element no kernel wrote?)"
        assert torch.equal(a[n], b[n]), f"{n}: a second run gives other bits"


# ---- encoder ------------------------------------------------------------------------------------------------------------------------
def run_encoder(case):
    from graphtrans_amd import _lib, layers, ops
    from graphtrans_amd.w3 import W1Images
    from test_hip_attention import make_layout
    c = R.ENC_CASES[case]
    inp = R.encoder_inputs(case)
    dt = c["dtype"]
    mod = torch.nn.TransformerEncoderLayer(R.D_MODEL, R.NHEAD, c["ffn"], 0.0, c["act"])
    mod.load_state_dict(inp["params"])
    mod = mod.to(DEV)
    lay = make_layout("packed", list(c["lens"]))
    lay.kind = "packed"
    lay.last_rows = inp["pool_rows"].to(DEV)
    assert lay.rows == inp["x"].shape[0] and int(lay.last_rows.max()) < lay.rows
    x, dy = inp["x"].to(DEV).to(dt), inp["dy"].to(DEV).to(dt)
    params = layers.encoder_layer_params(mod)
    assert [n for n, _ in zip(layers.ENC_PARAM_ORDER, params)] == list(R.ENC_PARAM_ORDER)
    imgs = None
    if c["images"]:
        imgs = W1Images([mod.self_attn.in_proj_weight, mod.self_attn.out_proj.weight, mod.linear1.weight, mod.linear2.weight])
        imgs.build()
    ctx = _Ctx()
    ops.set_matmul_dtype(BF if dt == BF else torch.float32)
    bwd, out = [], {}
    try:
        with imgs.bound() if imgs is not None else contextlib.nullcontext(), nan_allocations():
            fwd, y = recorded(lambda: layers._EncoderLayer.forward(ctx, x, lay, c["pooled"], R.NHEAD, c["p"], R.ENC_SEED, c["training"], R.LN_EPS,
                                                                   c["act"], *params))
            out["y"] = y
            if c["training"]:
                bwd, g = recorded(lambda: layers._EncoderLayer.backward(ctx, dy))
                out["dx"] = g[0]
                out.update({"d " + n: t for n, t in zip(layers.ENC_PARAM_ORDER, g[-12:])})
            # the gate on the dX output has no label of its own: the question enc_rows_bwd asks, with its arguments
            code, M = _lib.GT_BF16 if dt == BF else _lib.GT_F32, (len(c["lens"]) if c["pooled"] else lay.rows)
            gate_out = bool(_lib.lib().gt_linear_bwd_gate_out_ok(code, code, code, mod.linear2.weight.data_ptr(), M, R.D_MODEL, c["ffn"]))
    finally:
        ops.set_matmul_dtype(torch.float32)
    torch.cuda.synchronize()
    return fwd, bwd + (["gate-out dX"] if gate_out and c["training"] else []), {n: t.detach().clone() for n, t in out.items()}


@pytest.mark.parametrize("case", list(R.ENC_CASES))
def test_encoder_layer(case):
    c = R.ENC_CASES[case]
    fwd, bwd, out = run_encoder(case)
    same_bits(out, run_encoder(case)[2])
    r64 = R.encoder_reference(case)
    if not c["training"]:
        r64 = {"y": r64["y"]}
    got = {n: t.float().cpu() for n, t in out.items()}
    if c["dtype"] == BF:
        rbf = R.encoder_reference(case, bf16=True)
        noise = R.bf16_noise({n: rbf[n] for n in r64}, r64)
        report(case, R.bf16_ratios(got, r64, noise), fwd, bwd)
        R.compare_bf16(got, r64, {n: rbf[n] for n in r64}, what=case)
    else:
        report(case, {n: R.fp32_margin(got[n], r64[n]) for n in R.tensors(r64)}, fwd, bwd)
        R.compare_fp32(got, r64, what=case)
    assert (fwd, bwd) == LABELS.get(case), "the GEMM launch labels changed"


def test_every_fused_arm_is_covered():
    """over the pinned labels of the encoder cases: the fused LayerNorm forward, the LayerNorm-backward epilogue, the ring kernels, k_dw16
    and the gate on the dX output ("gate-out dX": no kernel label, appended by run_encoder when gt_linear_bwd_gate_out_ok says yes)"""
    seen = {l for k, (f, b) in LABELS.items() if k.startswith("enc-") for l in f + b}
    for need in REQUIRED:
        assert need in seen, (need, sorted(seen))


# ---- GCN layer and virtual-node update -------------------------------------------------------------------------------------------------
def _graph(gb):
    from graphtrans_amd.graph import GraphStructure
    return GraphStructure.build(gb["edge_index"].to(DEV), gb["batch"].to(DEV), num_graphs=gb["B"])


def _bn(params, name, n):
    from graphtrans_amd.modules.norm import BatchNorm1d
    bn = BatchNorm1d(n, eps=R.BN_EPS, momentum=R.BN_MOMENTUM)
    bn.load_state_dict({k[len(name) + 1:]: v for k, v in params.items() if k.startswith(name + ".")}, strict=False)
    assert int(bn.num_batches_tracked) == 0
    return bn.to(DEV)


def _running(out, bn, name):
    out[name + " running_mean"], out[name + " running_var"] = bn.running_mean, bn.running_var
    out[name + " num_batches_tracked"] = bn.num_batches_tracked.double()


def _f32_compute():
    from graphtrans_amd import _lib, ops
    ops.set_matmul_dtype(torch.float32)
    assert ops.f32_compute_code() == _lib.GT_F32


def _edge_spec(c, inp, P):
    """(ops.EdgeSpec, edge parameters on the device, their names in the reference)"""
    from graphtrans_amd import ops
    if c["edge"] == "linear":
        w, b = P["conv.edge_encoder.weight"], P["conv.edge_encoder.bias"]
        return ops.EdgeSpec("linear", attr=inp["attr"].to(DEV), weight=w, bias=b), [w, b], ["weight", "bias"]
    if c["edge"] == "tables":
        tabs = [P[f"conv.edge_encoder.bond_embedding_list.{i}.weight"] for i in range(len(R.TABLE_ROWS))]
        off = [0] + [sum(R.TABLE_ROWS[:i + 1]) for i in range(len(R.TABLE_ROWS) - 1)]
        assert inp["attr"].dtype == torch.int64 and all(int(inp["attr"][:, i].max()) < r for i, r in enumerate(R.TABLE_ROWS))
        return ops.EdgeSpec("tables", attr=inp["attr"].to(DEV), tab_off=off), tabs, [f"bond_embedding_list.{i}.weight" for i in range(len(tabs))]
    return ops.EdgeSpec("none"), [], []


def run_gcn(case):
    from graphtrans_amd import layers
    c = R.GCN_CASES[case]
    inp = R.gcn_inputs(case)
    gb = inp["graph"]
    _f32_compute()
    gs = _graph(gb)
    P = {k: v.to(DEV).contiguous() for k, v in inp["params"].items()}
    bn = _bn(inp["params"], "bn", gb["D"])
    spec, edge_params, edge_names = _edge_spec(c, inp, P)
    h = inp["h_in"].to(DEV)
    vn = inp["vn"].to(DEV) if c["has_vn"] else None
    gx, gy = (inp["gx"].to(DEV) if c["has_vn"] else None), inp["gy"].to(DEV)
    params = (P["conv.linear.weight"], P["conv.linear.bias"], P["conv.root_emb.weight"], bn.weight.detach(), bn.bias.detach(), *edge_params)
    ctx = _Ctx()
    bwd, out = [], {}
    with nan_allocations():
        fwd, (x, y) = recorded(lambda: layers._GcnLayer.forward(ctx, h, vn, gs, spec, c["relu"], c["residual"], c["training"], bn, c["p"],
                                                                R.CONV_SEED, *params))
        out["y"] = y
        if c["has_vn"]:
            out["x"] = x
        if c["training"]:
            bwd, g = recorded(lambda: layers._GcnLayer.backward(ctx, gx, gy))
            out["d_h"] = g[0]
            if c["has_vn"]:
                out["d_vn"] = g[1]
            out.update({"d " + n: t for n, t in zip(("lin_w", "lin_b", "root", "bn_w", "bn_b", *edge_names), g[10:])})
            assert len(g) == 15 + len(edge_names)
    torch.cuda.synchronize()
    _running(out, bn, "bn")
    return fwd, bwd, {n: t.detach().clone() for n, t in out.items()}


def run_vn(case):
    from graphtrans_amd import layers
    c = R.VN_CASES[case]
    inp = R.vn_inputs(case)
    gb = inp["graph"]
    D = gb["D"]
    _f32_compute()
    gs = _graph(gb)
    P = {k: v.to(DEV).contiguous() for k, v in inp["params"].items()}
    bn1, bn2 = _bn(inp["params"], "mlp.1", 2 * D), _bn(inp["params"], "mlp.4", D)
    x, vn, g_out = inp["x"].to(DEV), inp["vn"].to(DEV), inp["g_out"].to(DEV)
    params = (P["mlp.0.weight"], P["mlp.0.bias"], bn1.weight.detach(), bn1.bias.detach(), P["mlp.3.weight"], P["mlp.3.bias"],
              bn2.weight.detach(), bn2.bias.detach())
    ctx = _Ctx()
    with nan_allocations():
        fwd, out_vn = recorded(lambda: layers._VnUpdate.forward(ctx, x, vn, gs, c["residual"], c["training"], bn1, bn2, c["p"], R.CONV_SEED, *params))
        bwd, g = recorded(lambda: layers._VnUpdate.backward(ctx, g_out))
    torch.cuda.synchronize()
    out = {"vn": out_vn, "d_x": g[0], "d_vn": g[1]}
    out.update({"d " + n: t for n, t in zip(("w1", "b1", "bn1_w", "bn1_b", "w2", "b2", "bn2_w", "bn2_b"), g[-8:])})
    _running(out, bn1, "bn1")
    _running(out, bn2, "bn2")
    return fwd, bwd, {n: t.detach().clone() for n, t in out.items()}


# ---- GIN layer, through ctypes -----------------------------------------------------------------------------------------------------------
class Banded:
    """n bytes of 0xFF (NaN in fp32) followed by a BAND of 0x5A that must survive"""
    def __init__(self, nbytes):
        self.n = int(nbytes)
        assert self.n % 4 == 0
        self.buf = torch.full((self.n + BAND,), 255, dtype=torch.uint8, device=DEV)
        self.buf[self.n:] = 0x5A

    def f32(self, *shape):
        return self.buf[:self.n].view(torch.float32).view(*shape)

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr())

    def check(self, what):
        assert bool((self.buf[self.n:] == 0x5A).all()), f"{what}: a store behind the end of the buffer"


def run_gin(case):
    from graphtrans_amd import _lib, layers
    from graphtrans_amd.graph import _ptr, _stream
    c = R.GIN_CASES[case]
    inp = R.gin_inputs(case)
    gb = inp["graph"]
    N, B, D, E = gb["N"], gb["B"], gb["D"], gb["E"]
    _f32_compute()
    L = _lib.lib()
    gs = _graph(gb)
    assert gs.E == E and gs.B == B
    P = {k: v.to(DEV).contiguous() for k, v in inp["params"].items()}
    rs = {k: P[k].clone() for k in P if "running" in k}
    nbt1, nbt = torch.zeros((), dtype=torch.int64, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    desc = layers.GinLayerDesc()
    desc.N, desc.E, desc.B, desc.D = N, E, B, D
    desc.has_vn, desc.relu, desc.residual, desc.training, desc.compute = 1, int(c["relu"]), int(c["residual"]), int(c["training"]), _lib.GT_F32
    desc.bn_momentum, desc.bn_eps = R.BN_MOMENTUM, R.BN_EPS
    desc.seed, desc.dropout_p = R.CONV_SEED, (c["p"] if c["training"] else 0.0)
    layers._fill_graph(desc, gs)
    keep = []
    if c["edge"] == "linear":
        attr = inp["attr"].to(DEV).contiguous()
        desc.edge_mode, desc.edge_cols = _lib.GT_EDGE_LINEAR, 2
        desc.edge_attr, desc.edge_w, desc.edge_b = _ptr(attr), _ptr(P["conv.edge_encoder.weight"]), _ptr(P["conv.edge_encoder.bias"])
        edge_elems = [("weight", (D, 2)), ("bias", (D,))]
    else:
        attr = inp["attr"].to(DEV).contiguous()
        tables = torch.cat([P[f"conv.edge_encoder.bond_embedding_list.{i}.weight"] for i in range(len(R.TABLE_ROWS))]).contiguous()
        assert attr.dtype == torch.int64 and all(int(inp["attr"][:, i].max()) < r for i, r in enumerate(R.TABLE_ROWS))
        desc.edge_mode, desc.edge_cols, desc.table_rows = _lib.GT_EDGE_TABLES, len(R.TABLE_ROWS), tables.shape[0]
        acc = 0
        for i, r in enumerate(R.TABLE_ROWS):
            desc.tab_off[i] = acc
            acc += r
        desc.edge_attr, desc.edge_w = _ptr(attr), _ptr(tables)
        keep.append(tables)
        edge_elems = [(f"bond_embedding_list.{i}.weight", (r, D)) for i, r in enumerate(R.TABLE_ROWS)]
    keep.append(attr)
    for f, k in (("eps", "conv.eps"), ("w1", "conv.mlp.0.weight"), ("b1", "conv.mlp.0.bias"), ("bn1_w", "conv.mlp.1.weight"),
                 ("bn1_b", "conv.mlp.1.bias"), ("w2", "conv.mlp.3.weight"), ("b2", "conv.mlp.3.bias"), ("bn_w", "bn.weight"), ("bn_b", "bn.bias"),
                 ("bn1_rm", "conv.mlp.1.running_mean"), ("bn1_rv", "conv.mlp.1.running_var"), ("bn_rm", "bn.running_mean"), ("bn_rv", "bn.running_var")):
        t = rs[k] if "running" in k else P[k]
        assert t.dtype == torch.float32 and t.is_contiguous()
        setattr(desc, f, _ptr(t))
    desc.bn1_nbt, desc.bn_nbt = _ptr(nbt1), _ptr(nbt)
    d = C.byref(desc)
    saved_b, ws_b, n_grads = L.gt_gin_layer_saved_bytes(d), L.gt_gin_layer_workspace_bytes(d), L.gt_gin_layer_grad_elems(d)
    assert n_grads == 20 + sum(int(torch.tensor(s).prod()) for _, s in edge_elems) + 4 * D * D + 9 * D
    saved, ws, grads = Banded(saved_b), Banded(ws_b), Banded(4 * n_grads)
    x_out, y, d_h, d_vn = Banded(4 * N * D), Banded(4 * N * D), Banded(4 * N * D), Banded(4 * B * D)
    h, vn, gx, gy = (inp[k].to(DEV).contiguous() for k in ("h_in", "vn", "gx", "gy"))
    fwd, _ = recorded(lambda: _lib.check(L.gt_gin_layer_fwd(d, _ptr(h), _ptr(vn), x_out.ptr(), y.ptr(), saved.ptr(), ws.ptr(), ws_b, _stream()),
                                         "gt_gin_layer_fwd"))
    out = {"y": y.f32(N, D), "x": x_out.f32(N, D)}
    bwd = []
    if c["training"]:
        bwd, _ = recorded(lambda: _lib.check(L.gt_gin_layer_bwd(d, x_out.ptr(), _ptr(gy), _ptr(gx), saved.ptr(), d_h.ptr(), d_vn.ptr(), grads.ptr(),
                                                                ws.ptr(), ws_b, _stream()), "gt_gin_layer_bwd"))
        out.update({"d_h": d_h.f32(N, D), "d_vn": d_vn.f32(B, D)})
        flat, off = grads.f32(n_grads), 20
        out["d eps"] = flat[:1]
        blocks = edge_elems + [("w1", (2 * D, D)), ("b1", (2 * D,)), ("bn1_w", (2 * D,)), ("bn1_b", (2 * D,)), ("w2", (D, 2 * D)), ("b2", (D,)),
                               ("bn_w", (D,)), ("bn_b", (D,))]
        for n, shape in blocks:
            k = int(torch.tensor(shape).prod())
            out["d " + n] = flat[off:off + k].view(*shape)
            off += k
        assert off == n_grads
    torch.cuda.synchronize()
    for b, what in ((saved, "saved"), (ws, "workspace"), (grads, "grads"), (x_out, "x_out"), (y, "y"), (d_h, "d_h_in"), (d_vn, "d_vn")):
        b.check(f"{case}: {what}")
    for nm, key, n in (("bn1", "conv.mlp.1", nbt1), ("bn", "bn", nbt)):
        out[nm + " running_mean"], out[nm + " running_var"] = rs[key + ".running_mean"], rs[key + ".running_var"]
        out[nm + " num_batches_tracked"] = n.double()
    return fwd, bwd, {n: t.detach().clone() for n, t in out.items()}


GRAPH_CASES = [(run_gcn, R.gcn_reference, c) for c in R.GCN_CASES] + [(run_vn, R.vn_reference, c) for c in R.VN_CASES] + \
              [(run_gin, R.gin_reference, c) for c in R.GIN_CASES]


@pytest.mark.parametrize("run,reference,case", GRAPH_CASES, ids=[c for _, _, c in GRAPH_CASES])
def test_graph_layer(run, reference, case):
    fwd, bwd, out = run(case)
    same_bits(out, run(case)[2])
    r64 = reference(case)
    got = {n: t.double().cpu() for n, t in out.items()}
    report(case, {n: R.fp32_margin(got[n].reshape(r64[n].shape), r64[n]) for n in R.tensors(r64)}, fwd, bwd)
    R.compare_fp32(got, r64, what=case)
    assert (fwd, bwd) == LABELS.get(case), "the GEMM launch labels changed"
