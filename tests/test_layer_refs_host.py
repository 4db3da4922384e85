"""CPU tests of tests/layer_refs.py: the float64 references of the composite layers are anchored on torch / oracle.reference_math at
p = 0, the dropout masks have the rates and the four distinct seeds they should, the inputs of the fp32 cases have no ReLU tie, the
bf16 bounds stay far below a flaw's effect, and every flaw of layer_refs.FLAWS is rejected by the comparison its case uses."""
import math
from types import SimpleNamespace

import pytest
import torch

import layer_refs as R
from conftest import assert_close

_CACHE = {}


def ref(kind, case, **kw):
    """one evaluation of a reference per (case, flaw, bf16), shared by the tests of this file"""
    key = (kind, case, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = {"enc": R.encoder_reference, "gcn": R.gcn_reference, "gin": R.gin_reference, "vn": R.vn_reference}[kind](case, **kw)
    return _CACHE[key]


def kind_of(case):
    return case.split("-")[0]


# ---- anchors at p = 0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["enc-iii-full-eval", "enc-ii-full-eval", "enc-iii-pooled-eval"])
def test_encoder_reference_is_torch_encoder_layer(case):
    c = R.ENC_CASES[case]
    inp = R.encoder_inputs(case)
    mod = torch.nn.TransformerEncoderLayer(R.D_MODEL, R.NHEAD, c["ffn"], 0.0, c["act"]).double()
    mod.load_state_dict({k: v.double() for k, v in inp["params"].items()})
    x = inp["x"].double().requires_grad_(True)
    dy_full = torch.zeros_like(x)
    if c["pooled"]:
        dy_full[inp["pool_rows"]] = inp["dy"].double()
    else:
        dy_full = inp["dy"].double()
    ys, r0 = [], 0
    for n in c["lens"]:
        ys.append(mod(x[r0:r0 + n].unsqueeze(1)).squeeze(1))
        r0 += n
    y = torch.cat(ys)
    (y * dy_full).sum().backward()
    want = {"y": y.detach()[inp["pool_rows"]] if c["pooled"] else y.detach(), "dx": x.grad}
    want.update({"d " + n: dict(mod.named_parameters())[n].grad for n in R.ENC_PARAM_ORDER})
    got = R.tensors(ref("enc", case))
    assert set(got) == set(want) and len(got) == 14
    for n in want:
        err = float((got[n] - want[n]).abs().max())
        assert err <= 1e-10 * max(1.0, float(want[n].abs().max())), (n, err)


def _gnn_chain(kind):
    """two layers with a virtual node and residuals, stated twice: reference_math.gnn_node and the chained layer_refs forwards"""
    gb = R.graph_batch(1)
    B, D = gb["B"], gb["D"]
    c0 = dict(batch=1, edge="linear", has_vn=True, relu=True, residual=True, p=0.0, training=True)
    c1 = dict(c0, relu=False)
    make = R.gcn_inputs if kind == "gcn" else R.gin_inputs
    i0, i1 = make(dict(c0, data_seed=0)), make(dict(c1, data_seed=5))
    iv = R.vn_inputs(dict(batch=1, residual=True, p=0.0, training=True, data_seed=0))
    sd = {"virtualnode_embedding.weight": torch.randn(1, D, generator=torch.Generator().manual_seed(3))}
    for l, i in enumerate((i0, i1)):
        for k, v in i["params"].items():
            sd[(f"convs.{l}." + k[5:]) if k.startswith("conv.") else f"batch_norms.{l}." + k[3:]] = v
    sd.update({"mlp_virtualnode_list.0." + k[4:]: v for k, v in iv["params"].items()})
    sd = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    x0 = i0["h_in"].double().requires_grad_(True)
    data = SimpleNamespace(x=x0, edge_index=gb["edge_index"], edge_attr=i0["attr"], batch=gb["batch"])
    args = R.rm.default_args(gnn_virtual_node=True, gnn_num_layer=2, gnn_emb_dim=D, gnn_residual=True, gnn_type=kind)
    want = R.rm.gnn_node(sd, "", args, data, training=True)
    # the same through the layer references
    vn = sd["virtualnode_embedding.weight"][torch.zeros(B, dtype=torch.long)]
    fwd = R.gcn_forward if kind == "gcn" else R.gin_forward
    def layer_sd(l):
        conv, bn = f"convs.{l}.", f"batch_norms.{l}."
        return {**{"conv." + k[len(conv):]: v for k, v in sd.items() if k.startswith(conv)},
                **{"bn." + k[len(bn):]: v for k, v in sd.items() if k.startswith(bn)}}

    s0, s1 = layer_sd(0), layer_sd(1)
    sv = {("mlp." + k[23:]): v for k, v in sd.items() if k.startswith("mlp_virtualnode_list.0.")}
    xa, ya = fwd(s0, x0, vn, gb, i0["attr"], c0)[:2]
    vn1 = R.vn_forward(sv, xa, vn, gb, dict(residual=True, p=0.0, training=True))[0]
    got = fwd(s1, ya, vn1, gb, i0["attr"], c1)[1]
    return want, got, x0, sd


@pytest.mark.parametrize("kind", ["gcn", "gin"])
def test_graph_references_are_gnn_node(kind):
    want, got, x0, sd = _gnn_chain(kind)
    assert float((want - got).detach().abs().max()) <= 1e-10 * float(want.detach().abs().max())
    g = torch.randn(want.shape, generator=torch.Generator().manual_seed(4)).double()
    leaves = [x0] + [v for v in sd.values() if v.requires_grad]
    gw = torch.autograd.grad((want * g).sum(), leaves, allow_unused=True)
    gg = torch.autograd.grad((got * g).sum(), leaves, allow_unused=True)
    used = 0
    for a, b in zip(gw, gg):
        assert (a is None) == (b is None)
        if a is not None:
            used += 1
            assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(a.abs().max()))
    assert used >= 20


def test_running_statistics_are_batchnorm1d():
    case = "gcn-1-tables-p0.25-train"
    inp = R.gcn_inputs(case)
    out = ref("gcn", case)
    sd = R._sd64(inp["params"])
    z = R.gcn_forward(sd, inp["h_in"].double(), inp["vn"].double(), inp["graph"], inp["attr"], R.GCN_CASES[case])[2].detach()
    bn = torch.nn.BatchNorm1d(z.shape[1], eps=R.BN_EPS, momentum=R.BN_MOMENTUM).double()
    bn.load_state_dict({k[3:]: v.double() for k, v in inp["params"].items() if k.startswith("bn.")}, strict=False)
    bn.train()(z)
    assert_close(out["bn running_mean"], bn.running_mean, atol=1e-12, rtol=1e-12)
    assert_close(out["bn running_var"], bn.running_var, atol=1e-12, rtol=1e-12)
    assert int(out["bn num_batches_tracked"]) == int(bn.num_batches_tracked) == 1


# ---- masks ---------------------------------------------------------------------------------------------------------------------
def test_keep_mask_is_the_norm_tests_mask():
    from test_hip_norm import _bn_keep_mask
    assert _bn_keep_mask is R.keep_mask_rc
    m = R.keep_mask_rc(5, 8, 0.25, 99)
    # the hash by hand for (row 3, col 5)
    M = 0xFFFFFFFF
    x = ((3 * 0x9E3779B1 + 99) & M) ^ ((5 * 0x85EBCA77 + 0) & M)
    x ^= x >> 16; x = (x * 0x7feb352d) & M; x ^= x >> 15; x = (x * 0x846ca68b) & M; x ^= x >> 16
    assert bool(m[3, 5]) == (x >= (1 << 30))
    assert torch.equal(R.keep_mask_rc(torch.tensor([3]), 8, 0.25, 99)[0], m[3])


def _rate_ok(mask, p):
    n, rate = mask.numel(), float(mask.double().mean())
    assert abs(rate - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n), (rate, p, n)


def test_mask_rates_and_the_four_encoder_seeds():
    p, rows, d, F = 0.3, sum(R.LENS_LARGE), R.D_MODEL, 1024
    seeds = [R.ENC_SEED ^ s for s in (R.ENC_SEED_NORM1, R.ENC_SEED_FFN, R.ENC_SEED_NORM2)]
    m1, mf, m2 = R.keep_mask_rc(rows, d, p, seeds[0]), R.keep_mask_rc(rows, F, p, seeds[1]), R.keep_mask_rc(rows, d, p, seeds[2])
    lay = R.attention_refs.Layout("packed", R.LENS_LARGE)
    att = R.attention_refs.masks_on_valid_keys(R.attention_refs.keep_masks(lay, R.NHEAD, p, R.ENC_SEED), lay)
    for m in (m1, mf, m2, att):
        _rate_ok(m, float(torch.tensor(p, dtype=torch.float32)))
    # pairwise different: the three row masks on their common columns, and each against the attention mask of one sequence and head
    a0 = R.attention_refs.keep_mask(R.ENC_SEED, 1, 0, R.NHEAD, 128, p)
    four = [m1[:128, :128], mf[:128, :128], m2[:128, :128], a0]
    for i in range(4):
        for j in range(i + 1, 4):
            agree = float((four[i] == four[j]).double().mean())
            assert abs(agree - (0.49 + 0.09)) < 0.05, (i, j, agree)    # independent masks agree on p^2 + (1 - p)^2 = 0.58
    for case in ("gcn-2-linear-vn-p0.25-train", "vn-2-res-p0.25", "gin-2-p0.25-train"):
        gb = R.graph_batch(2)
        _rate_ok(R.keep_mask_rc(gb["B"] if case.startswith("vn") else gb["N"], gb["D"], 0.25, R.CONV_SEED), 0.25)


# ---- conditions on the inputs ----------------------------------------------------------------------------------------------------
FP32_CASES = [c for c in R.ENC_CASES if c.startswith("enc-iii")] + list(R.GCN_CASES) + list(R.GIN_CASES) + list(R.VN_CASES)
BF16_CASES = [c for c in R.ENC_CASES if not c.startswith("enc-iii")]


@pytest.mark.parametrize("case", FP32_CASES)
def test_fp32_cases_have_no_relu_tie(case):
    pre = ref(kind_of(case), case)["pre"]
    assert pre, "a case without a ReLU?"
    for name, z in pre.items():
        m = R.tie_margin(z)
        print(f"\n{case} {name}: min|z| / max|z| = {m:.3e} over {z.numel()} pre-activations")
        assert m >= R.TIE, (case, name, m)


@pytest.mark.parametrize("case", BF16_CASES)
def test_bf16_noise_is_small(case):
    noise = R.bf16_noise(ref("enc", case, bf16=True), ref("enc", case))
    assert len(noise) == 14
    for n, (n2, nmax) in noise.items():
        print(f"\n{case} {n}: n2 {n2:.3e} nmax {nmax:.3e}")
        assert (0 < n2 < R.N2_MAX) or (nmax == 0 and n == "d norm2.bias"), (case, n, n2)


# ---- flaws -------------------------------------------------------------------------------------------------------------------------
def test_the_listed_flaws_exist():
    assert set(R.FLAWS) >= {"norm1_bwd_scale", "ffn_mask_not_replayed", "attn_seed_xor", "norm2_resid_x", "pooled_row_early",
                            "gelu_mul_no_scale", "bn_running_var_biased", "residual_from_h_in", "gin_no_one_plus_eps", "vn_pool_wrong_graph"}


@pytest.mark.parametrize("flaw,case", [(f, c) for f, (_, cases) in R.FLAWS.items() for c in cases])
def test_flaw_is_rejected(flaw, case):
    """a kernel that computed the flawed function -- with the bf16 storage noise of Rbf on top where the case has bf16 rows -- exceeds
    the bound of its case's comparison by a factor of 3 at least"""
    kind = kind_of(case)
    r64 = ref(kind, case)
    bad = R.tensors(ref(kind, case, flaw=flaw))
    if case in BF16_CASES:
        rbf = ref(kind, case, bf16=True)
        fake = {n: bad[n] + (rbf[n] - r64[n]) for n in bad}
        ratios = R.bf16_ratios(fake, r64, R.bf16_noise(rbf, r64))
        worst = max(max(r[0] / R.L2_FACTOR, r[1] / R.MAX_FACTOR) for r in ratios.values())
        with pytest.raises(AssertionError):
            R.compare_bf16(fake, r64, rbf)
    else:
        worst = max(R.fp32_margin(bad[n], r64[n]) for n in bad)
        with pytest.raises(AssertionError):
            R.compare_fp32(bad, r64)
    print(f"\n{flaw} on {case}: the violated bound is exceeded {worst:.1f} times")
    assert worst >= 3.0, (flaw, case, worst)
    # and the unflawed reference passes its own comparison
    if case in BF16_CASES:
        R.compare_bf16({n: v for n, v in R.tensors(rbf).items()}, r64, rbf)
    else:
        R.compare_fp32(R.tensors(r64), r64)
