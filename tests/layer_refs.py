"""float64 references, shared inputs and comparison functions for the composite layer entry points of csrc/layers.hip
(gt_encoder_layer[_pooled]_*, gt_gcn_layer_*, gt_gin_layer_*, gt_vn_update_*), used by tests/test_layer_refs_host.py (CPU) and
tests/test_hip_layer_references.py (GPU).  Nothing here needs a GPU to import.

The references are written from the contracts in include/graphtrans_hip.h and the reference model's lines that csrc/layers.hip cites
(torch nn.TransformerEncoderLayer post-norm; modules/gnn_module.py:199-229; modules/conv.py:18-71), on oracle.reference_math and
attention_refs.reference -- not from the kernels.  Gradients come from autograd in float64.

* `keep_mask_rc`: THE SPECIFICATION of the row/column dropout that csrc/norm.hip (bn_hash, ln_hash) and csrc/linear.hip (lin_hash)
  share: keep = hash(seed, row, col) >= thr.  The ROW that enters the hash is the row of the matrix the kernel runs on: the token row
  in the full encoder layer, the SEQUENCE INDEX in the pooled layer (enc_rows_* runs on M = num_seqs gathered rows,
  include/graphtrans_hip.h: "drawn per pooled-row index"), the node row in the GCN / GIN layers and the graph row in the
  virtual-node update.
* `encoder_reference`, `gcn_reference`, `gin_reference`, `vn_reference`: {name: float64 tensor} of every output, plus "pre": the ReLU
  pre-activations (for the tie condition of the fp32 cases).  `flaw` (a key of FLAWS) builds a deliberately WRONG variant, used only by
  the host tests to show that the comparison tells it from the right one.  `bf16=True` (encoder) builds Rbf: the same pipeline with
  bf16 weight images and every tensor that enc_saved / enc_work keep in the row type rounded to bf16 (RNE) where it is stored.
* the cases and their inputs (ENC_CASES, GCN_CASES, GIN_CASES, VN_CASES, `*_inputs`): the GPU tests and the host tests walk the same sets.
* `compare_fp32`, `bf16_noise`, `compare_bf16`: the comparisons.
"""
import math

import numpy as np
import torch

import attention_refs
from conftest import rel_l2
from oracle import reference_math as rm

F64 = torch.float64
BF = torch.bfloat16
ENC_PARAM_ORDER = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                   "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
                   "norm2.bias")
# csrc/layers.hip: the dropout seeds of the encoder layer's row-wise half, xor-ed onto the layer's seed (the attention takes the seed itself)
ENC_SEED_NORM1, ENC_SEED_FFN, ENC_SEED_NORM2 = 0x5851F42D4C957F2D, 0x2545F4914F6CDD1D, 0x14057B7EF767814F
TIE = 3e-5    # fp32 cases: no ReLU pre-activation with |z| < TIE * max|z| (about ten fp32 roundings of a 64-term dot product)
N2_MAX = 0.05  # bf16 cases: relL2(Rbf, R64) of every tensor stays below this
L2_FACTOR, MAX_FACTOR = 3.0, 4.0   # bf16 rows: relL2(K, R64) <= 3 n2 and max|K - R64| <= 4 nmax (see compare_bf16)


# ----------------------------------------------------------------------------------------------------------------------------
# dropout
# ----------------------------------------------------------------------------------------------------------------------------
def _p32(p):
    return float(np.float32(p))   # the entry points receive p as a C float


def keep_mask_rc(rows, D, p, seed):
    """bool [rows][D], True = kept.  rows: a count (rows 0 .. rows-1) or an int64 vector of row numbers.

        x = (row * 0x9E3779B1 + seed_lo) ^ (col * 0x85EBCA77 + seed_hi);  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b;
        x ^= x >> 16   (all mod 2^32);   keep = x >= thr,  thr = clamp(int(p * 2^32), 1, 2^32 - 1) of the fp32 p"""
    M = 0xFFFFFFFF
    r = (torch.arange(rows, dtype=torch.int64) if isinstance(rows, int) else torch.as_tensor(rows, dtype=torch.int64)).reshape(-1, 1)
    c = torch.arange(D, dtype=torch.int64).reshape(1, -1)
    s0, s1 = seed & M, (seed >> 32) & M
    x = (((r * 0x9E3779B1) & M) + s0 & M) ^ (((c * 0x85EBCA77) & M) + s1 & M)
    x = x ^ (x >> 16); x = (x * 0x7feb352d) & M
    x = x ^ (x >> 15); x = (x * 0x846ca68b) & M
    x = x ^ (x >> 16)
    thr = min(max(int(_p32(p) * 4294967296.0), 1), 4294967295)
    return x >= thr


class _Drop(torch.autograd.Function):
    """y = x * keep * scale; the backward replays (bkeep, bscale), which a flaw may make differ from the forward's"""
    @staticmethod
    def forward(ctx, x, keep, scale, bkeep, bscale):
        ctx.m = bkeep * bscale
        return x * keep * scale

    @staticmethod
    def backward(ctx, g):
        return g * ctx.m, None, None, None, None


def _drop(x, keep, p, bwd_no_scale=False, bwd_no_mask=False):
    if keep is None:
        return x
    k = keep.to(F64)
    s = 1.0 / (1.0 - _p32(p))
    return _Drop.apply(x, k, s, torch.ones_like(k) if bwd_no_mask else k, 1.0 if bwd_no_scale else s)


def _rb(t):
    return t.float().to(BF).to(F64)


class _Q(torch.autograd.Function):
    """a tensor stored in bf16: rounded in the forward (fwd) and its gradient rounded in the backward (bwd)"""
    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return _rb(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (_rb(g) if ctx.bwd else g), None, None


class _ActDrop(torch.autograd.Function):
    """f = drop(act(z)); backward d_z = d_f * m, m = act'(z) * bkeep * bscale -- the multiplier the gelu layer saves (g1, rounded to the
    row type when `rnd`); for relu the gate of the stored f1 and the dropout scale"""
    @staticmethod
    def forward(ctx, z, act, keep, scale, bkeep, bscale, rnd):
        if act == "relu":
            f, da = torch.relu(z), (z > 0).to(F64)
        else:
            cdf = 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))
            f, da = z * cdf, cdf + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
        m = da * bkeep * bscale
        ctx.m = _rb(m) if (rnd and act == "gelu") else m
        return f * keep * scale

    @staticmethod
    def backward(ctx, g):
        return g * ctx.m, None, None, None, None, None, None


class _Attn(torch.autograd.Function):
    """attention_refs.reference as one differentiable node"""
    @staticmethod
    def forward(ctx, qkv, lay, nhead, scale, keep, inv):
        ctx.a = (lay, nhead, scale, keep, inv)
        ctx.save_for_backward(qkv)
        with torch.enable_grad():
            return attention_refs.reference(qkv, torch.zeros(qkv.shape[0], qkv.shape[1] // 3, dtype=F64), *ctx.a)[0]

    @staticmethod
    def backward(ctx, d_ctx):
        with torch.enable_grad():
            return attention_refs.reference(ctx.saved_tensors[0], d_ctx, *ctx.a)[1], None, None, None, None, None


# ----------------------------------------------------------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(str(k) for k in key))) % (2 ** 31))
    return g


def _randn(g, *shape, s=1.0):
    return torch.randn(*shape, generator=g) * s


def _away(g, n, lo, hi):
    """+-U(lo, hi): a bias that keeps a ReLU's pre-activation away from 0 for most units, open and closed gates in equal numbers"""
    sign = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    return sign * (lo + (hi - lo) * torch.rand(n, generator=g))


# ----------------------------------------------------------------------------------------------------------------------------
# encoder layer
# ----------------------------------------------------------------------------------------------------------------------------
D_MODEL, NHEAD, LN_EPS, ENC_SEED = 128, 4, 1e-5, 1234567
LENS = (6, 71, 2)                                   # tests/test_hip_layer_composites.py: 79 rows, one sequence crosses a 64-query tile
LENS_LARGE = (513, 600, 1, 64, 65, 400, 420)        # 2063 rows: the ring kernels and k_dw16 inside a composite
# id: (row storage, W1Images bound, ffn, activation, dropout p) -- tests/test_hip_layer_composites.py:ENC_CONFIGS
ENC_CONFIGS = {"i": (BF, True, 512, "relu", 0.3), "ii": (BF, True, 256, "gelu", 0.0), "iii": (torch.float32, False, 512, "relu", 0.0)}


def _enc_case(config, pooled, training, p=None, lens=LENS, ffn=None, data_seed=0):
    dt, images, f, act, p0 = ENC_CONFIGS[config]
    return dict(dtype=dt, images=images, ffn=ffn or f, act=act, p=p0 if p is None else p, pooled=pooled, training=training,
                lens=tuple(lens), data_seed=data_seed)


ENC_CASES = {f"enc-{c}-{'pooled' if pooled else 'full'}-{'train' if tr else 'eval'}": _enc_case(c, pooled, tr)
             for c in ENC_CONFIGS for pooled in (False, True) for tr in (True, False)}
ENC_CASES["enc-ii-full-train-p0.3"] = _enc_case("ii", False, True, p=0.3)
ENC_CASES["enc-iii-full-train-p0.3"] = _enc_case("iii", False, True, p=0.3)     # the four seeds and masks at the fp32 bar
ENC_CASES["enc-iii-pooled-train-p0.3"] = _enc_case("iii", True, True, p=0.3)
ENC_CASES["enc-i-large"] = _enc_case("i", False, True, p=0.1, lens=LENS_LARGE, ffn=1024)
def encoder_inputs(case):
    """{params: {name: fp32}, x, dy (already rounded to the row type, fp32 on the CPU), pool_rows} of one ENC_CASES entry"""
    c = ENC_CASES[case] if isinstance(case, str) else case
    g = _gen("enc", c["ffn"], c["act"], c["lens"], c["data_seed"])
    d, F = D_MODEL, c["ffn"]
    P = {"self_attn.in_proj_weight": _randn(g, 3 * d, d, s=d ** -0.5), "self_attn.in_proj_bias": _randn(g, 3 * d, s=0.1),
         "self_attn.out_proj.weight": _randn(g, d, d, s=d ** -0.5), "self_attn.out_proj.bias": _randn(g, d, s=0.1),
         "linear1.weight": _randn(g, F, d, s=0.5 * d ** -0.5), "linear1.bias": _away(g, F, 1.5, 3.0),
         "linear2.weight": _randn(g, d, F, s=F ** -0.5), "linear2.bias": _randn(g, d, s=0.1),
         "norm1.weight": 1 + _randn(g, d, s=0.1), "norm1.bias": _randn(g, d, s=0.1),
         "norm2.weight": 1 + _randn(g, d, s=0.1), "norm2.bias": _randn(g, d, s=0.1)}
    rows, B = sum(c["lens"]), len(c["lens"])
    x = _randn(g, rows, d).to(c["dtype"]).float()
    dy = _randn(g, B if c["pooled"] else rows, d).to(c["dtype"]).float()
    pool = torch.tensor(np.cumsum(c["lens"]) - 1, dtype=torch.int64)
    return dict(params=P, x=x, dy=dy, pool_rows=pool)


def encoder_reference(case, inp=None, flaw=None, bf16=False):
    """Post-norm encoder layer (csrc/layers.hip enc_rows_fwd and gt_encoder_layer_fwd; torch nn.TransformerEncoderLayer):

        qkv = x Win^T + bin;  ctx = attention(qkv), scale 1 / sqrt(d / nhead), keep mask of `seed`;  a = ctx Wo^T + bo
        x1 = LN1(x + drop(a; seed ^ ENC_SEED_NORM1));  f1 = drop(act(x1 W1^T + b1); seed ^ ENC_SEED_FFN);  f2 = f1 W2^T + b2
        y = LN2(x1 + drop(f2; seed ^ ENC_SEED_NORM2));  p = 0 when not training

    The hash row of the three row-wise dropouts is the token row in the full layer and the sequence index in the pooled layer, whose
    row-wise half runs on the num_seqs gathered rows; the pooled layer returns y on those rows and takes a dy on those rows.
    -> {"y", "dx", "d <param>" for ENC_PARAM_ORDER, "pre": {"ffn": z1} for relu}"""
    c = ENC_CASES[case] if isinstance(case, str) else case
    inp = inp or encoder_inputs(c)
    d, act = D_MODEL, c["act"]
    p = c["p"] if c["training"] else 0.0
    lay = attention_refs.Layout("packed", c["lens"])
    q = (lambda t, fwd=True, bwd=True: _Q.apply(t, fwd, bwd)) if bf16 else (lambda t, fwd=True, bwd=True: t)
    P = {n: inp["params"][n].to(F64).clone().requires_grad_(True) for n in ENC_PARAM_ORDER}
    W = {n: (q(P[n], True, False) if n.endswith("weight") and "norm" not in n else P[n]) for n in P}   # bf16 weight images
    x = inp["x"].to(F64).clone().requires_grad_(True)
    xin = q(x, False, True)                                           # dx is stored in the row type
    qkv = q(xin @ W["self_attn.in_proj_weight"].t() + W["self_attn.in_proj_bias"])
    aseed = ENC_SEED ^ ENC_SEED_NORM1 if flaw == "attn_seed_xor" else ENC_SEED
    keep = attention_refs.keep_masks(lay, NHEAD, p, aseed) if p > 0 else None
    ctx = q(_Attn.apply(qkv, lay, NHEAD, 1.0 / math.sqrt(d / NHEAD), keep, 1.0 / (1.0 - _p32(p))))
    if c["pooled"]:
        pool = inp["pool_rows"] - 1 if flaw == "pooled_row_early" else inp["pool_rows"]
        resid, ctx_rows, rowid = xin[pool], ctx[pool], torch.arange(len(c["lens"]))
    else:
        resid, ctx_rows, rowid = xin, ctx, torch.arange(x.shape[0])
    F = c["ffn"]
    k1 = keep_mask_rc(rowid, d, p, ENC_SEED ^ ENC_SEED_NORM1) if p > 0 else None
    kf = keep_mask_rc(rowid, F, p, ENC_SEED ^ ENC_SEED_FFN).to(F64) if p > 0 else torch.ones(len(rowid), F, dtype=F64)
    k2 = keep_mask_rc(rowid, d, p, ENC_SEED ^ ENC_SEED_NORM2) if p > 0 else None
    a = q(ctx_rows @ W["self_attn.out_proj.weight"].t() + W["self_attn.out_proj.bias"])
    x1 = q(rm.layer_norm(resid + _drop(a, k1, p, bwd_no_scale=flaw == "norm1_bwd_scale"), P, "norm1", LN_EPS))
    z1 = x1 @ W["linear1.weight"].t() + W["linear1.bias"]
    s = 1.0 / (1.0 - _p32(p))
    f1 = q(_ActDrop.apply(z1, act, kf, s, torch.ones_like(kf) if flaw == "ffn_mask_not_replayed" else kf,
                          1.0 if flaw == "gelu_mul_no_scale" else s, bf16))
    f2 = q(f1 @ W["linear2.weight"].t() + W["linear2.bias"])
    res2 = resid if flaw == "norm2_resid_x" else q(x1, False, True)     # (norm2's backward stores its d_x1 before linear1's adds to it)
    y = q(rm.layer_norm(res2 + _drop(f2, k2, p), P, "norm2", LN_EPS), True, False)
    (y * inp["dy"].to(F64)).sum().backward()
    out = {"y": y.detach(), "dx": x.grad}
    out.update({"d " + n: (P[n].grad if P[n].grad is not None else torch.zeros_like(P[n])) for n in ENC_PARAM_ORDER})
    out["pre"] = {"ffn": z1.detach()} if act == "relu" else {}
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# graph batches
# ----------------------------------------------------------------------------------------------------------------------------
def graph_batch(which):
    """dict(sizes, batch int64 [N], edge_index int64 [2][E], N, B, E, D).
    1: the 40-node / 3-graph / 86-edge batch of tests/test_hip_layer_composites.py, D = 32.
    2: N = 1100, B = 9, E = 3000, D = 36: duplicate edges, self loops, a single-node graph (with a self loop), a graph without edges;
       more rows than BatchNorm's small-rows tier."""
    if which == 1:
        g = torch.Generator().manual_seed(12)
        sizes = [9, 25, 6]
        first = torch.tensor([0, 9, 34])
        gi = torch.randint(0, 3, (86,), generator=g)
        src = first[gi] + (torch.rand(86, generator=g) * torch.tensor(sizes)[gi]).long()
        dst = first[gi] + (torch.rand(86, generator=g) * torch.tensor(sizes)[gi]).long()
        D = 32
    else:
        g = _gen("graph batch 2")
        sizes = [200, 1, 150, 120, 99, 180, 130, 100, 120]     # graph 1: one node; graph 4: no edge
        first = torch.tensor(np.cumsum([0] + sizes[:-1]))
        st = torch.tensor(sizes)
        with_edges = torch.tensor([0, 2, 3, 5, 6, 7, 8])
        gi = with_edges[torch.randint(0, 7, (2900,), generator=g)]
        src = first[gi] + (torch.rand(2900, generator=g) * st[gi]).long()
        dst = first[gi] + (torch.rand(2900, generator=g) * st[gi]).long()
        dup = torch.randint(0, 2900, (60,), generator=g)
        gl = torch.cat([torch.tensor([1]), with_edges[torch.randint(0, 7, (39,), generator=g)]])
        loop = first[gl] + (torch.rand(40, generator=g) * st[gl]).long()
        src, dst = torch.cat([src, src[dup], loop]), torch.cat([dst, dst[dup], loop])
        D = 36
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    ei = torch.stack([src, dst]).long()
    N = int(sum(sizes))
    assert 0 <= int(ei.min()) and int(ei.max()) < N and bool((batch[ei[0]] == batch[ei[1]]).all())
    return dict(sizes=sizes, batch=batch, edge_index=ei, N=N, B=len(sizes), E=int(ei.shape[1]), D=D)


TABLE_ROWS = (5, 3)     # two attribute columns, BondEncoder-style tables
BN_EPS, BN_MOMENTUM, CONV_SEED, GIN_EPS = 1e-5, 0.1, 0x9E3779B97F4A7C15, 0.3


def _conv_case(batch, edge, has_vn, relu, residual, p, training, data_seed=0):
    """data_seed: picked per case so that no ReLU pre-activation of the float64 reference is a tie (tests/test_layer_refs_host.py asserts
    it; seed 0 serves all cases but one)"""
    return dict(batch=batch, edge=edge, has_vn=has_vn, relu=relu, residual=residual, p=p, training=training, data_seed=data_seed)


# every value of edge mode, has_vn, relu, residual, p and training / eval at both sizes
GCN_CASES = {
    "gcn-1-linear-vn-relu-res-p0-train": _conv_case(1, "linear", True, True, True, 0.0, True),
    "gcn-1-tables-p0.25-train": _conv_case(1, "tables", False, False, False, 0.25, True),
    "gcn-1-none-vn-relu-res-eval": _conv_case(1, "none", True, True, True, 0.25, False),
    "gcn-1-linear-vn-relu-res-p0.25-train": _conv_case(1, "linear", True, True, True, 0.25, True),
    "gcn-2-tables-vn-relu-res-p0.25-train": _conv_case(2, "tables", True, True, True, 0.25, True),
    "gcn-2-none-res-p0-train": _conv_case(2, "none", False, False, True, 0.0, True),
    "gcn-2-linear-vn-p0.25-train": _conv_case(2, "linear", True, False, False, 0.25, True),
    "gcn-2-linear-relu-res-eval": _conv_case(2, "linear", False, True, True, 0.0, False, data_seed=21),
}
GIN_CASES = {f"gin-{b}-{m}": _conv_case(b, e, True, True, True, p, tr)
             for b, e in ((1, "linear"), (2, "tables")) for m, p, tr in (("p0-train", 0.0, True), ("p0.25-train", 0.25, True), ("eval", 0.0, False))}
VN_CASES = {f"vn-{b}-{'res' if r else 'nores'}-p{p}": dict(batch=b, residual=r, p=p, training=True, data_seed=0)
            for b in (1, 2) for r in (True, False) for p in (0.0, 0.25)}


def _edge_inputs(g, c, gb, P, prefix):
    E, D = gb["E"], gb["D"]
    if c["edge"] == "linear":
        P[prefix + ".edge_encoder.weight"], P[prefix + ".edge_encoder.bias"] = _randn(g, D, 2, s=0.25), _randn(g, D, s=0.2)
        return _randn(g, E, 2)
    if c["edge"] == "tables":
        for i, r in enumerate(TABLE_ROWS):
            P[f"{prefix}.edge_encoder.bond_embedding_list.{i}.weight"] = _randn(g, r, D, s=0.25)
        return torch.stack([torch.randint(0, r, (E,), generator=g) for r in TABLE_ROWS], dim=1)
    return None


def _bn_inputs(g, P, name, n, away=True):
    P[name + ".weight"], P[name + ".bias"] = 0.5 + 0.5 * torch.rand(n, generator=g), (_away(g, n, 2.0, 3.5) if away else _randn(g, n, s=0.2))
    P[name + ".running_mean"], P[name + ".running_var"] = _randn(g, n, s=0.3), 0.5 + torch.rand(n, generator=g)


def gcn_inputs(case):
    """{params (state_dict keys of a GNN layer: conv.*, bn.*), h_in, vn, attr, gx, gy, graph}"""
    c = GCN_CASES[case] if isinstance(case, str) else case
    gb = graph_batch(c["batch"])
    g = _gen("gcn", c["batch"], c["edge"], c["data_seed"])
    N, B, D = gb["N"], gb["B"], gb["D"]
    P = {"conv.linear.weight": _randn(g, D, D, s=0.5 * D ** -0.5), "conv.linear.bias": _away(g, D, 2.0, 3.5),
         "conv.root_emb.weight": _randn(g, 1, D, s=0.3)}
    attr = _edge_inputs(g, c, gb, P, "conv")
    _bn_inputs(g, P, "bn", D, away=c["relu"])
    return dict(params=P, h_in=_randn(g, N, D), vn=_randn(g, B, D, s=0.3), attr=attr, gx=_randn(g, N, D), gy=_randn(g, N, D), graph=gb)


def gin_inputs(case):
    c = GIN_CASES[case] if isinstance(case, str) else case
    gb = graph_batch(c["batch"])
    g = _gen("gin", c["batch"], c["edge"], c["data_seed"])
    N, B, D = gb["N"], gb["B"], gb["D"]
    P = {"conv.eps": torch.tensor([GIN_EPS]), "conv.mlp.0.weight": _randn(g, 2 * D, D, s=0.3 * D ** -0.5), "conv.mlp.0.bias": _randn(g, 2 * D, s=0.1),
         "conv.mlp.3.weight": _randn(g, D, 2 * D, s=(2 * D) ** -0.5), "conv.mlp.3.bias": _randn(g, D, s=0.1)}
    _bn_inputs(g, P, "conv.mlp.1", 2 * D)
    attr = _edge_inputs(g, c, gb, P, "conv")
    _bn_inputs(g, P, "bn", D, away=c["relu"])
    h = _away(g, N * D, 1.5, 3.0).view(N, D) + _randn(g, N, D, s=0.2)     # relu(x_j + e) stays away from its kink
    return dict(params=P, h_in=h, vn=_randn(g, B, D, s=0.2), attr=attr, gx=_randn(g, N, D), gy=_randn(g, N, D), graph=gb)


def vn_inputs(case):
    c = VN_CASES[case] if isinstance(case, str) else case
    gb = graph_batch(c["batch"])
    g = _gen("vn", c["batch"], c["data_seed"])
    N, B, D = gb["N"], gb["B"], gb["D"]
    P = {"mlp.0.weight": _randn(g, 2 * D, D, s=0.3 * D ** -0.5), "mlp.0.bias": _randn(g, 2 * D, s=0.1),
         "mlp.3.weight": _randn(g, D, 2 * D, s=(2 * D) ** -0.5), "mlp.3.bias": _randn(g, D, s=0.1)}
    _bn_inputs(g, P, "mlp.1", 2 * D)
    _bn_inputs(g, P, "mlp.4", D)
    return dict(params=P, x=_randn(g, N, D, s=0.3), vn=_randn(g, B, D), g_out=_randn(g, B, D), graph=gb)


def _sd64(params):
    return {k: (v.to(F64).clone().requires_grad_(True) if "running" not in k else v.to(F64).clone()) for k, v in params.items()}


def _running(z, sd, name, training, flaw=None):
    """(running_mean, running_var, num_batches_tracked) of nn.BatchNorm1d after one forward on z: momentum update with the UNBIASED
    variance in training mode, untouched in eval mode; num_batches_tracked starts at 0"""
    rmean, rvar = sd[name + ".running_mean"].clone(), sd[name + ".running_var"].clone()
    if not training:
        return rmean, rvar, torch.tensor(0.0, dtype=F64)
    z = z.detach()
    var = z.var(0, unbiased=flaw != "bn_running_var_biased")
    return (1 - BN_MOMENTUM) * rmean + BN_MOMENTUM * z.mean(0), (1 - BN_MOMENTUM) * rvar + BN_MOMENTUM * var, torch.tensor(1.0, dtype=F64)


def _tail(z, x, h, c, sd, pre, flaw):
    """y = drop(relu?(BN(z)); seed) (+ x if residual): the tail the GCN and the GIN layer share (gnn_module.py:204-212)"""
    t = rm.batch_norm(z, sd, "bn", c["training"], BN_EPS)
    if c["relu"]:
        pre["bn"] = t.detach()
        t = torch.relu(t)
    p = c["p"] if c["training"] else 0.0
    t = _drop(t, keep_mask_rc(z.shape[0], z.shape[1], p, CONV_SEED) if p > 0 else None, p)
    if c["residual"]:
        t = t + (h if flaw == "residual_from_h_in" else x)
    return t


def _conv_outputs(out, sd, names, h, vn, c, x, y):
    """the outputs of a training-mode conv layer: y, d_h, (x, d_vn), "d <short name>" per parameter and "d <key below edge_encoder>" """
    out.update({"y": y.detach(), "d_h": h.grad})
    if c["has_vn"]:
        out.update({"x": x.detach(), "d_vn": vn.grad})
    edge = "conv.edge_encoder."
    for short, key in list(names) + [(k[len(edge):], k) for k in sorted(sd) if k.startswith(edge)]:
        out["d " + short] = sd[key].grad if sd[key].grad is not None else torch.zeros_like(sd[key])
    return out


def gcn_forward(sd, h, vn, gb, attr, c, pre=None, flaw=None):
    """differentiable (x, y, conv output): x = h_in + vn[batch] if has_vn (gnn_module.py:199);
    y = drop(relu?(BN(gcn_conv(x))); seed) (+ x if residual) (gnn_module.py:204-212, conv.py:50-71)"""
    pre = {} if pre is None else pre
    x = h + vn[gb["batch"]] if c["has_vn"] else h
    z = rm.gcn_conv(sd, "conv", x, gb["edge_index"], attr)
    with torch.no_grad():   # the inner ReLUs' pre-activations (conv.py:63,65)
        hl = rm.linear(x, sd, "conv.linear")
        e = rm.edge_encode(sd, "conv.edge_encoder", attr)
        pre["msg"] = hl[gb["edge_index"][0]] + (0 if e is None else e)
        pre["self"] = hl + sd["conv.root_emb.weight"]
    return x, _tail(z, x, h, c, sd, pre, flaw), z


def gcn_reference(case, inp=None, flaw=None):
    """-> x, y, d_h (d_h_in), d_vn, the seven parameter gradients, the updated running statistics; the loss is <y, gy> + <x, gx>
    (gx: the layer's dx_extra, the gradient reaching x from its other consumers; only with a virtual node)"""
    c = GCN_CASES[case] if isinstance(case, str) else case
    inp = inp or gcn_inputs(c)
    sd, gb = _sd64(inp["params"]), inp["graph"]
    h, vn = inp["h_in"].to(F64).requires_grad_(True), inp["vn"].to(F64).requires_grad_(True)
    pre = {}
    x, y, z = gcn_forward(sd, h, vn, gb, inp["attr"], c, pre, flaw)
    loss = (y * inp["gy"].to(F64)).sum()
    if c["has_vn"]:
        loss = loss + (x * inp["gx"].to(F64)).sum()
    if c["training"]:
        loss.backward()
    out = {"pre": pre}
    if c["training"]:
        _conv_outputs(out, sd, (("lin_w", "conv.linear.weight"), ("lin_b", "conv.linear.bias"), ("root", "conv.root_emb.weight"),
                                ("bn_w", "bn.weight"), ("bn_b", "bn.bias")), h, vn, c, x, y)
    else:
        out.update({"y": y.detach()}, **({"x": x.detach()} if c["has_vn"] else {}))
    out["bn running_mean"], out["bn running_var"], out["bn num_batches_tracked"] = _running(z, sd, "bn", c["training"], flaw)
    return out


def gin_forward(sd, h, vn, gb, attr, c, pre=None, flaw=None):
    """differentiable (x, y, z1, z2): y = drop(relu?(BN(mlp((1 + eps) x + sum_j relu(x_j + e_ij)))); seed) (+ x) (conv.py:18-36)"""
    pre = {} if pre is None else pre
    x = h + vn[gb["batch"]] if c["has_vn"] else h
    sdc = dict(sd)
    if flaw == "gin_no_one_plus_eps":
        sdc["conv.eps"] = sd["conv.eps"] * 0.0
    z2 = rm.gin_conv(sdc, "conv", x, gb["edge_index"], attr, c["training"])
    with torch.no_grad():
        e = rm.edge_encode(sd, "conv.edge_encoder", attr)
        pre["msg"] = x[gb["edge_index"][0]] + (0 if e is None else e)
        z1 = rm.linear((1 + sdc["conv.eps"]) * x + rm.gin_aggregate(x, e, gb["edge_index"]), sd, "conv.mlp.0")
        pre["bn1"] = rm.batch_norm(z1, sd, "conv.mlp.1", c["training"], BN_EPS)
    return x, _tail(z2, x, h, c, sd, pre, flaw), z1, z2


def gin_reference(case, inp=None, flaw=None):
    c = GIN_CASES[case] if isinstance(case, str) else case
    inp = inp or gin_inputs(c)
    sd, gb = _sd64(inp["params"]), inp["graph"]
    h, vn = inp["h_in"].to(F64).requires_grad_(True), inp["vn"].to(F64).requires_grad_(True)
    pre = {}
    x, y, z1, z2 = gin_forward(sd, h, vn, gb, inp["attr"], c, pre, flaw)
    out = {"pre": pre}
    if c["training"]:
        ((y * inp["gy"].to(F64)).sum() + (x * inp["gx"].to(F64)).sum()).backward()
        _conv_outputs(out, sd, (("eps", "conv.eps"), ("w1", "conv.mlp.0.weight"), ("b1", "conv.mlp.0.bias"), ("bn1_w", "conv.mlp.1.weight"),
                                ("bn1_b", "conv.mlp.1.bias"), ("w2", "conv.mlp.3.weight"), ("b2", "conv.mlp.3.bias"), ("bn_w", "bn.weight"),
                                ("bn_b", "bn.bias")), h, vn, c, x, y)
    else:
        out.update({"y": y.detach(), "x": x.detach()})
    for nm, z, key in (("bn1", z1, "conv.mlp.1"), ("bn", z2, "bn")):
        out[nm + " running_mean"], out[nm + " running_var"], out[nm + " num_batches_tracked"] = _running(z, sd, key, c["training"], flaw)
    return out


def vn_forward(sd, x, vn, gb, c, pre=None, flaw=None, prefix="mlp"):
    """differentiable (vn_out, z1, z2): drop(relu(BN2(Lin2(relu(BN1(Lin1(segment_sum(x) + vn)))))); seed) (+ vn) (gnn_module.py:217-229)"""
    pre = {} if pre is None else pre
    batch = gb["batch"]
    if flaw == "vn_pool_wrong_graph":     # the last node of each graph lands in the next graph's sum
        last = torch.tensor(np.cumsum(gb["sizes"]) - 1)
        batch = batch.clone()
        batch[last] = (batch[last] + 1) % gb["B"]
    t = rm.segment_sum(x, batch, gb["B"]) + vn
    z1 = rm.linear(t, sd, prefix + ".0")
    t = rm.batch_norm(z1, sd, prefix + ".1", c["training"], BN_EPS)
    pre["bn1"] = t.detach()
    z2 = rm.linear(torch.relu(t), sd, prefix + ".3")
    t = rm.batch_norm(z2, sd, prefix + ".4", c["training"], BN_EPS)
    pre["bn2"] = t.detach()
    p = c["p"] if c["training"] else 0.0
    t = _drop(torch.relu(t), keep_mask_rc(gb["B"], t.shape[1], p, CONV_SEED) if p > 0 else None, p)
    return (t + vn if c["residual"] else t), z1, z2


def vn_reference(case, inp=None, flaw=None):
    c = VN_CASES[case] if isinstance(case, str) else case
    inp = inp or vn_inputs(c)
    sd, gb = _sd64(inp["params"]), inp["graph"]
    x, vn = inp["x"].to(F64).requires_grad_(True), inp["vn"].to(F64).requires_grad_(True)
    pre = {}
    out_vn, z1, z2 = vn_forward(sd, x, vn, gb, c, pre, flaw)
    (out_vn * inp["g_out"].to(F64)).sum().backward()
    out = {"pre": pre, "vn": out_vn.detach(), "d_x": x.grad, "d_vn": vn.grad}
    for short, key in (("w1", "mlp.0.weight"), ("b1", "mlp.0.bias"), ("bn1_w", "mlp.1.weight"), ("bn1_b", "mlp.1.bias"), ("w2", "mlp.3.weight"),
                       ("b2", "mlp.3.bias"), ("bn2_w", "mlp.4.weight"), ("bn2_b", "mlp.4.bias")):
        out["d " + short] = sd[key].grad
    for nm, z, key in (("bn1", z1, "mlp.1"), ("bn2", z2, "mlp.4")):
        out[nm + " running_mean"], out[nm + " running_var"], out[nm + " num_batches_tracked"] = _running(z, sd, key, c["training"], flaw)
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# flaws: name -> (reference function, the cases whose comparison must reject it)
# ----------------------------------------------------------------------------------------------------------------------------
FLAWS = {
    "norm1_bwd_scale": (encoder_reference, ("enc-i-full-train", "enc-iii-full-train-p0.3", "enc-i-large")),   # norm1's 1 / (1 - p) missing in the backward
    "ffn_mask_not_replayed": (encoder_reference, ("enc-i-full-train", "enc-ii-full-train-p0.3", "enc-iii-pooled-train-p0.3")),
    "attn_seed_xor": (encoder_reference, ("enc-i-full-train", "enc-i-pooled-train", "enc-iii-full-train-p0.3")),  # attention seed ^ ENC_SEED_NORM1
    "norm2_resid_x": (encoder_reference, ("enc-i-full-eval", "enc-ii-pooled-train", "enc-iii-full-train", "enc-i-large")),
    "pooled_row_early": (encoder_reference, ("enc-i-pooled-train", "enc-ii-pooled-eval", "enc-iii-pooled-train")),
    "gelu_mul_no_scale": (encoder_reference, ("enc-ii-full-train-p0.3",)),           # the saved gelu multiplier without 1 / (1 - p)
    "bn_running_var_biased": (gcn_reference, ("gcn-1-linear-vn-relu-res-p0-train", "gcn-1-tables-p0.25-train")),
    "residual_from_h_in": (gcn_reference, ("gcn-1-linear-vn-relu-res-p0.25-train", "gcn-2-tables-vn-relu-res-p0.25-train", "gcn-1-none-vn-relu-res-eval")),
    "gin_no_one_plus_eps": (gin_reference, tuple(GIN_CASES)),
    "vn_pool_wrong_graph": (vn_reference, tuple(VN_CASES)),
}


# ----------------------------------------------------------------------------------------------------------------------------
# comparisons
# ----------------------------------------------------------------------------------------------------------------------------
def tensors(out):
    return {k: v for k, v in out.items() if k != "pre"}


def tie_margin(z):
    """min|z| / max|z| of a ReLU's pre-activations: the fp32 cases need it above TIE"""
    z = z.abs()
    return float(z.min()) / float(z.max())


def fp32_margin(got, ref):
    """max over the elements of |got - ref| / (1e-4 max(1, max|ref|) + 1e-4 |ref|): conftest.assert_close at its defaults passes iff <= 1"""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    if ref.numel() == 0:
        return 0.0
    tol = 1e-4 * max(1.0, float(ref.abs().max())) + 1e-4 * ref.abs()
    return float(((got - ref).abs() / tol).max())


def compare_fp32(got, ref, what=""):
    """fp32 rows: every tensor within conftest.assert_close at its defaults (1e-4 scale-relative, the project's bar) -> {name: margin}"""
    from conftest import assert_close
    ref = tensors(ref)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    margins = {n: fp32_margin(got[n].reshape(ref[n].shape), ref[n]) for n in ref}
    for n in ref:
        assert_close(got[n].reshape(ref[n].shape), ref[n], what=f"{what}: {n}")
    return margins


def bf16_noise(rbf, r64):
    """{name: (n2, nmax)}: relL2(Rbf, R64) and max|Rbf - R64| per tensor -- the REFERENCE's own distance under bf16 storage"""
    return {n: (rel_l2(rbf[n], r64[n]), float((rbf[n] - r64[n]).abs().max())) for n in tensors(r64)}


def bf16_ratios(got, r64, noise):
    """{name: (relL2(K, R64) / n2, max|K - R64| / nmax)}.  A tensor with nmax == 0 is one that no bf16 rounding reaches (d norm2.bias,
    the fp32 column sum of the bf16 dy the test hands in): the kernel computes it in fp32 from exact inputs, so it is held to the
    fp32 rows' bar and both entries are fp32_margin scaled so that the bar sits at the factors"""
    out = {}
    for n, (n2, nmax) in noise.items():
        k = torch.as_tensor(got[n]).double().reshape(r64[n].shape)
        if nmax == 0.0:
            m = fp32_margin(k, r64[n])
            out[n] = (m * L2_FACTOR, m * MAX_FACTOR)
        else:
            out[n] = (rel_l2(k, r64[n]) / n2, float((k - r64[n]).abs().max()) / nmax)
    return out


def compare_bf16(got, r64, rbf, what=""):
    """bf16 rows: relL2(K, R64) <= 3 n2 and max|K - R64| <= 4 nmax per tensor.  The kernel rounds at the same points as Rbf but
    accumulates in another order and flips other ReLU gates: its distance to R64 is a second draw of the same noise; the triangle
    inequality gives 2, the rest is head room.  A tensor that no bf16 rounding reaches (nmax == 0) is held to the fp32 rows' bar
    instead, see bf16_ratios.  -> {name: (l2 ratio, max ratio)}"""
    noise = bf16_noise(rbf, r64)
    assert set(got) == set(noise), (sorted(got), sorted(noise))
    ratios = bf16_ratios(got, r64, noise)
    bad = {n: r for n, r in ratios.items() if not (r[0] <= L2_FACTOR and r[1] <= MAX_FACTOR)}
    assert not bad, f"{what}: (relL2 / n2, max / nmax) beyond ({L2_FACTOR:g}, {MAX_FACTOR:g}): {bad}"
    return ratios
