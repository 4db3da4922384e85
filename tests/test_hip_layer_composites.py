"""The composite layer entry points of csrc/layers.hip (gt_encoder_layer[_pooled]_*, gt_gcn_layer_*, gt_vn_update_*; of gt_gin_layer_*
the buffer sizes only) as a record of what they do, through graphtrans_amd/layers.py and ctypes.  Their VALUES, gt_gin_layer_fwd / _bwd
included, are checked against float64 references in tests/test_hip_layer_references.py.  Here:

  - which GEMM kernels each forward and backward launches, in order (the launch profiler's labels, mask 32, as in
    tests/test_hip_linear_dispatch.py): a changed row is a changed behaviour;
  - the pooled encoder layer against the full one on the pooled rows;
  - the byte and element counts of `*_saved_bytes`, `*_workspace_bytes`, `*_grad_elems` (host arithmetic, no device): the callers' arenas
    are planned from them, so a changed integer is a changed behaviour.

The autograd Functions' two halves are called directly on a stand-in context, so that both run on the calling thread, where the weight
images are bound."""
import ctypes as C

import pytest
import torch

from conftest import assert_close

DEV = "cuda:0"
BF = torch.bfloat16

GT_F32, GT_BF16 = 0, 1
GT_EDGE_NONE, GT_EDGE_LINEAR, GT_EDGE_TABLES = 0, 1, 2


# ---- buffer sizes -----------------------------------------------------------------------------------------------------------------------
# Host arithmetic only: these entry points answer without a device.  Six shapes per descriptor: a 79-row / 3-sequence encoder layer and a 40-node / 3-graph batch, the Code2
# dims (D 300, d 128, ffn 512, 32 k rows, 256 graphs) and odd ones.
def _enc_desc(rows, d, ffn, nhead, dtype, compute, act, num_seqs):
    from graphtrans_amd import layers
    desc = layers.EncoderLayerDesc()
    desc.rows, desc.d_model, desc.ffn, desc.nhead, desc.dtype, desc.compute, desc.act, desc.num_seqs = rows, d, ffn, nhead, dtype, compute, act, num_seqs
    return desc


def _conv_desc(cls, N, E, B, D, edge_mode, edge_cols, table_rows, has_vn, compute):
    desc = cls()
    desc.N, desc.E, desc.B, desc.D, desc.edge_mode, desc.edge_cols, desc.table_rows, desc.has_vn, desc.compute = \
        N, E, B, D, edge_mode, edge_cols, table_rows, has_vn, compute
    return desc


def _vn_desc(N, B, D, compute):
    from graphtrans_amd import layers
    desc = layers.VnUpdateDesc()
    desc.N, desc.B, desc.D, desc.compute = N, B, D, compute
    return desc


# (rows, d_model, ffn, nhead, dtype, compute, act, num_seqs): (saved, workspace, pooled saved, pooled workspace, grad elems)
ENC_SIZES = {
    (79, 128, 512, 4, GT_BF16, GT_BF16, 0, 3): (226560, 1012992, 90880, 1076736, 198272),
    (79, 128, 256, 4, GT_BF16, GT_BF16, 1, 3): (226560, 906496, 90880, 943104, 132480),
    (79, 128, 512, 4, GT_F32, GT_F32, 0, 3): (449024, 1235456, 178688, 1164544, 198272),
    (32768, 128, 512, 4, GT_BF16, GT_BF16, 0, 256): (93847552, 127140608, 35196928, 60820480, 198272),
    (32768, 128, 512, 4, GT_F32, GT_F32, 1, 256): (253231104, 236585984, 69865472, 108107008, 198272),
    (1001, 64, 136, 2, GT_F32, GT_BF16, 0, 7): (2371072, 2809344, 1054464, 1544448, 34504),
}
CONV_SHAPES = [   # (N, E, B, D, edge_mode, edge_cols, table_rows, has_vn, compute)
    (40, 86, 3, 32, GT_EDGE_LINEAR, 2, 0, 1, GT_F32),
    (40, 86, 3, 32, GT_EDGE_LINEAR, 2, 0, 0, GT_F32),
    (32768, 65000, 256, 300, GT_EDGE_LINEAR, 2, 0, 1, GT_F32),
    (32768, 65000, 256, 300, GT_EDGE_TABLES, 3, 13, 1, GT_BF16),
    (1001, 3003, 7, 64, GT_EDGE_NONE, 0, 0, 0, GT_F32),
    (12289, 40000, 33, 144, GT_EDGE_TABLES, 2, 9, 0, GT_F32),
]
# CONV_SHAPES row: (saved, workspace, grad elems)
GCN_SIZES = [
    (10496, 1083136, 1248),
    (10496, 1082624, 1248),
    (78645760, 146101248, 92100),
    (78645760, 135280640, 95100),
    (513024, 1222144, 4352),
    (14158592, 34511616, 22608),
]
GIN_SIZES = [
    (31488, 1138944, 4500),
    (31488, 1138944, 4500),
    (235937024, 399103744, 363620),
    (235937024, 361557760, 366620),
    (1539072, 2961664, 16980),
    (42475008, 95051776, 85556),
]
# (N, B, D, compute): (saved, workspace, grad elems)
VN_SIZES = {
    (40, 3, 32, GT_F32): (3328, 47616, 4384),
    (32768, 256, 300, GT_F32): (1850624, 4873984, 362700),
    (32768, 256, 300, GT_BF16): (1850624, 4151552, 362700),
    (1001, 7, 64, GT_F32): (12288, 122880, 16960),
    (12289, 33, 144, GT_F32): (118272, 663040, 84240),
    (5, 1, 4, GT_F32): (1536, 7680, 100),
}


def measured_sizes():
    """the tables above as the loaded library answers them"""
    from graphtrans_amd import _lib, layers
    L = _lib.lib()
    enc = {}
    for k in ENC_SIZES:
        d = C.byref(_enc_desc(*k))
        enc[k] = (L.gt_encoder_layer_saved_bytes(d), L.gt_encoder_layer_workspace_bytes(d), L.gt_encoder_layer_pooled_saved_bytes(d),
                  L.gt_encoder_layer_pooled_workspace_bytes(d), L.gt_encoder_layer_grad_elems(d))
    conv = {}
    for kind, cls in (("gcn", layers.GcnLayerDesc), ("gin", layers.GinLayerDesc)):
        conv[kind] = []
        for k in CONV_SHAPES:
            d = C.byref(_conv_desc(cls, *k))
            conv[kind].append(tuple(getattr(L, f"gt_{kind}_layer_{q}")(d) for q in ("saved_bytes", "workspace_bytes", "grad_elems")))
    vn = {}
    for k in VN_SIZES:
        d = C.byref(_vn_desc(*k))
        vn[k] = (L.gt_vn_update_saved_bytes(d), L.gt_vn_update_workspace_bytes(d), L.gt_vn_update_grad_elems(d))
    return enc, conv["gcn"], conv["gin"], vn


def test_buffer_sizes():
    enc, gcn, gin, vn = measured_sizes()
    assert len(ENC_SIZES) == 6 and len(GCN_SIZES) == 6 and len(GIN_SIZES) == 6 and len(VN_SIZES) == 6
    assert enc == ENC_SIZES
    assert gcn == GCN_SIZES
    assert gin == GIN_SIZES
    assert vn == VN_SIZES


# ---- launch labels, pooled == full ---------------------------------------------------------------------------------------------------
# 3 sequences of 5, 70 and 1 tokens plus CLS: 79 rows, one sequence crosses a 64-query tile, one is a single token
LENS, D_MODEL, NHEAD = [6, 71, 2], 128, 4
# id: (row storage, W1Images bound, ffn, activation, training, dropout p) -- every branch of the row half once:
ENC_CONFIGS = {
    "i": (BF, True, 512, "relu", True, 0.3),       # fused out_proj+norm1 and linear2+norm2, gate-out, LayerNorm-backward epilogue
    "ii": (BF, True, 256, "gelu", False, 0.0),     # fused LayerNorm forward and gate-out, no LayerNorm-backward epilogue (contraction 256)
    "iii": (torch.float32, False, 512, "relu", False, 0.0),   # fp32 rows, nothing bound: every fallback arm
}
CASES = [f"enc-{c}-{k}" for c in ENC_CONFIGS for k in ("full", "pooled")] + ["gcn-vn", "gcn", "vn"]
# case: (forward labels, backward labels), recorded on the revision before the composites shared their helpers
LABELS = {
    'enc-i-full': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_lin1[fwd]', 'k_lin1[fwd+ln]'],
        ['k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx+lnb]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_linear_dw', 'k_lin1[dx]']),
    'enc-i-pooled': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_lin1[fwd]', 'k_lin1[fwd+ln]'],
        ['k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_linear_dw', 'k_lin1[dx]']),
    'enc-ii-full': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_linear_fwd', 'k_lin1[fwd+ln]'],
        ['k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_linear_dw', 'k_lin1[dx]']),
    'enc-ii-pooled': (['k_lin1[fwd]', 'k_lin1[fwd+ln]', 'k_linear_fwd', 'k_lin1[fwd+ln]'],
        ['k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_lin1[dx]', 'k_linear_dw', 'k_linear_dw', 'k_lin1[dx]']),
    'enc-iii-full': (['k_small_fwd', 'k_small_fwd', 'k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw', 'k_small_dw', 'k_small_dx']),
    'enc-iii-pooled': (['k_small_fwd', 'k_small_fwd', 'k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw', 'k_small_dw', 'k_small_dx']),
    'gcn-vn': (['k_small_fwd'],
        ['k_small_dx', 'k_small_dw']),
    'gcn': (['k_small_fwd'],
        ['k_small_dx', 'k_small_dw']),
    'vn': (['k_small_fwd', 'k_small_fwd'],
        ['k_small_dx', 'k_small_dw', 'k_small_dx', 'k_small_dw']),
}


class _Ctx:
    """what a Function's forward / backward use of autograd's context"""
    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def set_materialize_grads(self, value):
        pass


def recorded(fn):
    """(labels of the GEMM kernels fn() launched, fn's result)"""
    from graphtrans_amd import _lib
    _lib.profile_enable(32)
    try:
        out = fn()
        names = [r[0] for r in _lib.profile_records()]
    finally:
        _lib.profile_enable(0)
    return names, out


def _layout():
    from test_hip_attention import make_layout
    lay = make_layout("packed", LENS)
    lay.kind = "packed"
    lay.last_rows = torch.tensor([r0 + n - 1 for r0, n, _, _ in lay.desc_cpu], dtype=torch.int64, device=DEV)
    return lay


def run_encoder(config, pooled, dropout=True, dy_rows=None):
    """one forward and one backward of the (pooled) encoder layer -> (forward labels, backward labels, {name: tensor});
    dy_rows: the (3, d) gradient of the pooled rows, which the full layer gets as a dy that is zero elsewhere"""
    import contextlib

    from graphtrans_amd import layers, ops
    from graphtrans_amd.w3 import W1Images
    dt, images, ffn, act, training, p = ENC_CONFIGS[config]
    if not dropout:
        training, p = False, 0.0
    torch.manual_seed(11)
    mod = torch.nn.TransformerEncoderLayer(D_MODEL, NHEAD, ffn, 0.0, act)
    with torch.no_grad():
        for ln in (mod.norm1, mod.norm2):
            ln.weight.add_(0.1 * torch.randn(D_MODEL))
            ln.bias.add_(0.1 * torch.randn(D_MODEL))
    mod = mod.to(DEV)
    lay = _layout()
    x = torch.randn(lay.rows, D_MODEL).to(DEV).to(dt)
    dy = torch.randn(lay.rows, D_MODEL).to(DEV).to(dt)
    if dy_rows is not None:
        dy = torch.zeros_like(dy)
        dy[lay.last_rows] = dy_rows
    if pooled:
        dy = dy[lay.last_rows].contiguous()
    params = layers.encoder_layer_params(mod)
    imgs = None
    if images:
        imgs = W1Images([mod.self_attn.in_proj_weight, mod.self_attn.out_proj.weight, mod.linear1.weight, mod.linear2.weight])
        imgs.build()
    ctx = _Ctx()
    ops.set_matmul_dtype(BF if dt == BF else torch.float32)
    try:
        with imgs.bound() if imgs is not None else contextlib.nullcontext():
            fwd, y = recorded(lambda: layers._EncoderLayer.forward(ctx, x, lay, pooled, NHEAD, p, 1234567, training, mod.norm1.eps, act, *params))
            bwd, g = recorded(lambda: layers._EncoderLayer.backward(ctx, dy))
    finally:
        ops.set_matmul_dtype(torch.float32)
    torch.cuda.synchronize()
    out = {"y": y, "dx": g[0]}
    out.update({"d " + n: t for n, t in zip(layers.ENC_PARAM_ORDER, g[-12:])})
    return fwd, bwd, out


def _graph_batch():
    """40 nodes in 3 graphs, 86 edges with 2 attribute columns"""
    from graphtrans_amd.graph import GraphStructure
    torch.manual_seed(12)
    sizes = [9, 25, 6]
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    first = torch.tensor([0, 9, 34])
    g = torch.randint(0, 3, (86,))
    src = first[g] + (torch.rand(86) * torch.tensor(sizes)[g]).long()
    dst = first[g] + (torch.rand(86) * torch.tensor(sizes)[g]).long()
    ei = torch.stack([src, dst]).to(DEV)
    gs = GraphStructure.build(ei, batch.to(DEV), num_graphs=3)
    return gs, torch.randn(86, 2).to(DEV)


def run_gcn(has_vn, D=32):
    from graphtrans_amd import layers, ops
    from graphtrans_amd.modules.conv import GCNConv
    from graphtrans_amd.modules.norm import BatchNorm1d
    gs, attr = _graph_batch()
    torch.manual_seed(13)
    conv, bn = GCNConv(D, lambda d: torch.nn.Linear(2, d)).to(DEV), BatchNorm1d(D).to(DEV)
    spec = ops.EdgeSpec("linear", attr=attr, weight=conv.edge_encoder.weight, bias=conv.edge_encoder.bias)
    h = torch.randn(40, D).to(DEV)
    vn = torch.randn(3, D).to(DEV) if has_vn else None
    gx, gy = (torch.randn(40, D).to(DEV) if has_vn else None), torch.randn(40, D).to(DEV)
    ctx = _Ctx()
    params = (conv.linear.weight, conv.linear.bias, conv.root_emb.weight, bn.weight, bn.bias, spec.weight, spec.bias)
    fwd, (x, y) = recorded(lambda: layers._GcnLayer.forward(ctx, h, vn, gs, spec, True, True, True, bn, 0.0, 0, *params))
    bwd, g = recorded(lambda: layers._GcnLayer.backward(ctx, gx, gy))
    torch.cuda.synchronize()
    out = {"y": y, "d_h": g[0], "bn running_mean": bn.running_mean, "bn running_var": bn.running_var}
    if has_vn:
        out.update({"x": x, "d_vn": g[1]})
    out.update({"d " + n: t for n, t in zip(("lin_w", "lin_b", "root", "bn_w", "bn_b", "edge_w", "edge_b"), g[-7:])})
    return fwd, bwd, out


def run_vn(D=32):
    from graphtrans_amd import layers
    from graphtrans_amd.modules.norm import BatchNorm1d
    gs, _ = _graph_batch()
    torch.manual_seed(14)
    seq = torch.nn.Sequential(torch.nn.Linear(D, 2 * D), BatchNorm1d(2 * D), torch.nn.ReLU(), torch.nn.Linear(2 * D, D), BatchNorm1d(D),
                              torch.nn.ReLU()).to(DEV)
    x, vn, g_out = torch.randn(40, D).to(DEV), torch.randn(3, D).to(DEV), torch.randn(3, D).to(DEV)
    ctx = _Ctx()
    params = (seq[0].weight, seq[0].bias, seq[1].weight, seq[1].bias, seq[3].weight, seq[3].bias, seq[4].weight, seq[4].bias)
    fwd, out_vn = recorded(lambda: layers._VnUpdate.forward(ctx, x, vn, gs, True, True, seq[1], seq[4], 0.0, 0, *params))
    bwd, g = recorded(lambda: layers._VnUpdate.backward(ctx, g_out))
    torch.cuda.synchronize()
    out = {"vn": out_vn, "d_x": g[0], "d_vn": g[1]}
    out.update({"d " + n: t for n, t in zip(("w1", "b1", "bn1_w", "bn1_b", "w2", "b2", "bn2_w", "bn2_b"), g[-8:])})
    return fwd, bwd, out


def run_case(case):
    if case.startswith("enc-"):
        _, config, kind = case.split("-")
        return run_encoder(config, kind == "pooled")
    return run_vn() if case == "vn" else run_gcn(case == "gcn-vn")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_launch_labels(case):
    fwd, bwd, out = run_case(case)
    print(f"\n{case!r}: ({fwd},\n    {bwd}),")
    assert all(bool(torch.isfinite(t.float()).all()) for t in out.values())
    assert (fwd, bwd) == LABELS[case]


def pooled_vs_full(config):
    """-> [(name, pooled tensor, full tensor)] at dropout 0, the full layer fed a dy that is zero outside the pooled rows"""
    torch.manual_seed(15)
    dy_rows = torch.randn(len(LENS), D_MODEL).to(DEV).to(ENC_CONFIGS[config][0])
    _, _, full = run_encoder(config, False, dropout=False, dy_rows=dy_rows)
    _, _, pool = run_encoder(config, True, dropout=False, dy_rows=dy_rows)
    last = _layout().last_rows
    return [(n, pool[n].float().cpu(), (full[n][last] if n == "y" else full[n]).float().cpu()) for n in full]


# per row storage type: the bounds of tests/test_hip_attention_head_dims.py:test_pooled_entry_points_agree_with_the_full_kernels
# (measured on the revision before the composites shared their helpers: y equal bit for bit in all three configurations; dx 7.8e-3 at
# |dx| <= 4.3 with bf16 rows, equal with fp32 rows; the fp32 gradient tensors within 4.8e-7 at magnitudes of 1 to 8)
POOLED_TOL = {torch.float32: 1e-4, BF: 2e-2}


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(ENC_CONFIGS))
def test_pooled_layer_agrees_with_the_full_layer(config):
    tol = POOLED_TOL[ENC_CONFIGS[config][0]]
    pairs = pooled_vs_full(config)
    assert len(pairs) == 14 and float(pairs[1][2].abs().max()) > 0
    for name, got, want in pairs:
        print(f"\n[{config}] {name}: max |pooled - full| {float((got - want).abs().max()):.3e}, max |full| {float(want.abs().max()):.3e}; tol {tol:g}")
    for name, got, want in pairs:
        assert_close(got, want, atol=tol, rtol=tol, what=f"{config}: {name}")
