"""GPU parity of PNA's `sum` and `var` aggregators (modules/pna/aggregators.py:11-34) through every layer that carries them: the K = 6
aggregate kernels [mean | max | min | std | sum | var] (gt_pna_aggregate_*_k), PNAConv, the fused gt_pna_layer_* step of PNATransformer.

References: the float64 oracle (oracle/reference_math.py, pinned to the reference by tests/test_oracle_golden.py) under conftest.assert_close
at its defaults (1e-4 scale-relative), and the reference's own recorded `sum` / `var` outputs in tests/golden/G9_pna_aggr_scalers.npz.
`var` is compared against float64 for the reason tests/test_hip_pna.py gives for `std`: the kernel's shift-free Welford M2 / deg carries
no E[m^2] - E[m]^2 cancellation (and so is never negative), an fp32 evaluation of the reference formula does."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import Golden, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL6 = ["mean", "max", "min", "std", "sum", "var"]
DEG = torch.tensor([0, 5, 9, 7, 3, 1, 0, 2])
N_NODES = 120


def _hand_graph():
    """120 nodes, edges (src -> dst) written out by rule rather than drawn: a star of in-degree 45 on node 0, node 119 without in-edges,
    node 118 without out-edges, node 117 with exactly one in-edge, every third chord doubled (ties for max / min between identical
    sources), a ring and two chord families over nodes 1..116 for the ordinary degrees."""
    src, dst = [], []
    for j in range(1, 46):            # star: 1..45 -> 0
        src.append(j), dst.append(0)
    body = list(range(1, 117))        # ring + chords among 1..116
    for i, v in enumerate(body):
        src.append(v), dst.append(body[(i + 1) % len(body)])
        if i % 2 == 0:
            src.append(v), dst.append(body[(i * 7 + 3) % len(body)])
        if i % 5 == 0:
            src.append(body[(i * 11 + 50) % len(body)]), dst.append(v)
    n_single = len(src)
    for k in range(0, n_single, 3):   # duplicated edges (the star's too: in-degree 60 on node 0)
        src.append(src[k]), dst.append(dst[k])
    src += [0, 0, 119, 119]           # the hub and the source-only node feed the body
    dst += [5, 77, 9, 60]
    src += [3, 40, 41]                # 118: in-edges only
    dst += [118, 118, 118]
    src.append(8), dst.append(117)    # 117: in-degree 1 (and one out-edge)
    src.append(117), dst.append(30)
    ei = torch.tensor([src, dst], dtype=torch.int64)
    indeg = torch.bincount(ei[1], minlength=N_NODES)
    outdeg = torch.bincount(ei[0], minlength=N_NODES)
    assert indeg[119] == 0 and indeg[117] == 1 and indeg[0] >= 40 and outdeg[118] == 0 and indeg[118] > 0 and outdeg[119] > 0
    pairs = ei.t().tolist()
    assert len({tuple(p) for p in pairs}) < len(pairs)   # duplicates present
    return ei


def _structure(ei, n):
    from graphtrans_amd.graph import GraphStructure

    return GraphStructure.build(ei.to(DEV), torch.zeros(n, dtype=torch.int64, device=DEV), num_graphs=1)


_KERNEL_CASES = {}


def _kernel_case(D, towers):
    """Inputs, the float64 oracle's K = 6 output and gradients, the structure: made once per shape, shared by the tests below."""
    key = (D, towers)
    if key not in _KERNEL_CASES:
        from oracle import reference_math as rm

        g = torch.Generator().manual_seed(1000 + D)
        F = D // towers
        ei = _hand_graph()
        U, V = torch.randn(N_NODES, D, generator=g), torch.randn(N_NODES, D, generator=g)
        w = torch.randn(N_NODES, towers, 6 * F, generator=g)
        Ur, Vr = U.double().requires_grad_(True), V.double().requires_grad_(True)
        row, col = ei[0], ei[1]
        m = (Ur[col] + Vr[row]).view(-1, towers, F)
        ref = rm.pna_aggregators(m, col, N_NODES, ALL6)
        (ref * w.double()).sum().backward()
        _KERNEL_CASES[key] = dict(U=U, V=V, w=w, ref=ref.detach(), dU=Ur.grad, dV=Vr.grad, gs=_structure(ei, N_NODES), ei=ei)
    return _KERNEL_CASES[key]


# every LPN / NCH branch of pna_launch: D <= 64 (LPN 16), <= 128 (LPN 32), <= 256 (LPN 64), <= 512 (NCH 2), <= 768 (NCH 3), <= 1024 (NCH 4)
SHAPES = [(16, 1), (64, 4), (128, 4), (256, 4), (272, 4), (520, 2), (1024, 4)]


@pytest.mark.parametrize("D,towers", SHAPES)
def test_k6_aggregate_vs_oracle(D, towers):
    from graphtrans_amd import ops

    c = _kernel_case(D, towers)
    Ud, Vd = c["U"].to(DEV).requires_grad_(True), c["V"].to(DEV).requires_grad_(True)
    out = ops.pna_aggregate(Ud, Vd, c["gs"], towers, slots=6)
    assert out.shape == (N_NODES, towers, 6 * (D // towers))
    (out * c["w"].to(DEV)).sum().backward()
    F = D // towers
    got = out.detach().cpu()
    for i, name in enumerate(ALL6):
        assert_close(got[:, :, i * F:(i + 1) * F], c["ref"][:, :, i * F:(i + 1) * F], what=f"agg {name}")
    assert_close(Ud.grad.cpu(), c["dU"], what="dU")
    assert_close(Vd.grad.cpu(), c["dV"], what="dV")
    # the exact zeros the layout promises: sum and var of the empty neighbourhood, var of the in-degree-1 node; var is never negative
    assert (got[119, :, 4 * F:] == 0).all() and (got[117, :, 5 * F:] == 0).all() and (got[:, :, 5 * F:] >= 0).all()


def _raw_fwd(c, D, towers, slots):
    from graphtrans_amd import _lib
    from graphtrans_amd.ops import _ptr, _stream

    gs = c["gs"]
    U, V = c["U"].to(DEV), c["V"].to(DEV)
    out = torch.full((N_NODES, towers, slots * (D // towers)), float("nan"), device=DEV)
    mean_v = torch.full((N_NODES, D), float("nan"), device=DEV)
    arg = torch.full((N_NODES, 2, D), -7, dtype=torch.int32, device=DEV)
    if slots == 4:
        _lib.launch("gt_pna_aggregate_fwd", _ptr(U), _ptr(V), N_NODES, D, towers, _ptr(gs.in_ptr), _ptr(gs.in_src), _ptr(gs.in_eid),
                    _ptr(out), _ptr(mean_v), _ptr(arg), _stream())
    else:
        _lib.launch("gt_pna_aggregate_fwd_k", _ptr(U), _ptr(V), N_NODES, D, towers, slots, _ptr(gs.in_ptr), _ptr(gs.in_src),
                    _ptr(gs.in_eid), _ptr(out), _ptr(mean_v), _ptr(arg), _stream())
    torch.cuda.synchronize()
    return out, mean_v, arg


@pytest.mark.parametrize("D,towers", SHAPES)
def test_k6_classic_slots_have_the_k4_bits(D, towers):
    """Slots 0..3 of the K = 6 output, mean_v and arg are bit-identical to what the K = 4 entry point writes; ops.pna_aggregate's
    default still is that entry point."""
    from graphtrans_amd import ops

    c = _kernel_case(D, towers)
    F = D // towers
    o4, m4, a4 = _raw_fwd(c, D, towers, 4)
    o6, m6, a6 = _raw_fwd(c, D, towers, 6)
    assert not torch.isnan(o4).any() and not torch.isnan(o6).any() and not torch.isnan(m6).any()
    assert torch.equal(o6[:, :, :4 * F], o4)
    assert torch.equal(m6, m4) and torch.equal(a6, a4)
    assert torch.equal(ops.pna_aggregate(c["U"].to(DEV), c["V"].to(DEV), c["gs"], towers), o4)
    with pytest.raises(RuntimeError, match="slots must be 4"):   # (the library's own check: no launch)
        _raw_fwd(c, D, towers, 5)


def test_k6_sum_var_match_the_references_recorded_values():
    """G9: the reference's own aggregate_sum / aggregate_var outputs on src (40 x 4 x 6) scattered by `index` into n segments (two of
    them empty).  Every message gets a source node of its own (n + k, V = src[k] as 24 columns), U = 0, one tower."""
    from graphtrans_amd import ops

    g = Golden("G9_pna_aggr_scalers")
    src, index, n = g.inputs["src"], g.inputs["index"], g.meta["n"]
    E = src.shape[0]
    Fw = src[0].numel()
    assert (E, Fw) == (40, 24)
    N = n + E
    V = torch.zeros(N, Fw)
    V[n:] = src.reshape(E, Fw)
    ei = torch.stack([torch.arange(n, N), index.to(torch.int64)])
    out = ops.pna_aggregate(torch.zeros(N, Fw, device=DEV), V.to(DEV), _structure(ei, N), 1, slots=6).cpu()
    assert_close(out[:n, 0, 4 * Fw:5 * Fw], g.outs["sum"].reshape(n, Fw), what="sum")
    assert_close(out[:n, 0, 5 * Fw:6 * Fw], g.outs["var"].reshape(n, Fw), what="var")
    empty = torch.bincount(index.to(torch.int64), minlength=n) == 0
    assert int(empty.sum()) == 2 and (out[:n][empty][:, 0, 4 * Fw:] == 0).all()


def _tiny_batch(seed):
    from graphtrans_amd import synth

    return synth.tiny_mixed(seed=seed, sizes=tuple(int(s) for s in np.random.default_rng(seed).integers(1, 30, 6)), feat="code2")


def _randomize(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.2))
            if n.endswith("module.weight") or "norm" in n and n.endswith("weight"):
                p.add_(1.0)


CONV_CASES = [(32, ["sum", "var"], ["identity"]),
              (32, ALL6, ["identity", "amplification", "attenuation"]),
              (32, ["sum", "mean", "var"], ["amplification", "linear", "inverse_linear"]),
              (32, ["var"], ["attenuation", "identity"]),        # first scaler not the identity: x rides in a block of its own
              (24, ["sum", "var", "max"], ["identity", "amplification"])]   # F = 6: the zero-padded tower rows


@pytest.mark.parametrize("D,aggs,scalers", CONV_CASES)
def test_pna_conv_sum_var_vs_oracle(D, aggs, scalers):
    from graphtrans_amd.modules.pna.pna_module import PNAConv
    from oracle import reference_math as rm

    b = _tiny_batch(3)
    ei = torch.cat([b.edge_index, b.edge_index[:, ::3]], dim=1).contiguous()   # duplicated edges
    N = b.num_nodes
    conv = PNAConv(D, D, aggregators=aggs, scalers=scalers, deg=DEG, towers=4, divide_input=True)
    _randomize(conv, 7)
    g = torch.Generator().manual_seed(8)
    x, w = torch.randn(N, D, generator=g), torch.randn(N, D, generator=g)
    sd = {"c." + k: v.double().requires_grad_(True) for k, v in conv.state_dict().items()}
    xr = x.double().requires_grad_(True)
    torch.set_default_dtype(torch.float64)
    try:
        ref = rm.pna_conv(sd, "c", xr, ei, aggs, scalers, rm.pna_avg_deg(DEG), towers=4)
        (ref * w.double()).sum().backward()
    finally:
        torch.set_default_dtype(torch.float32)
    conv = conv.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    out = conv(xd, ei.to(DEV))
    (out * w.to(DEV)).sum().backward()
    assert_close(out.detach().cpu(), ref.detach(), what="out")
    assert_close(xd.grad.cpu(), xr.grad, what="dx")
    for k, p in conv.named_parameters():
        assert_close(p.grad.cpu(), sd["c." + k].grad, what=f"grad {k}")


def _oracle_run(model, args, b, dtype, ws=None):
    from oracle import reference_math as rm

    sd = {k: (v.to(dtype).requires_grad_(True) if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items()}
    torch.set_default_dtype(dtype)   # the oracle's helpers allocate in the default dtype
    try:
        ref = rm.pna_transformer(sd, args, b, None, True)
        if ws is None:
            g = torch.Generator().manual_seed(2)
            ws = [torch.randn(r.shape, generator=g, dtype=torch.float64) for r in ref]
        sum((r * w.to(dtype)).sum() for r, w in zip(ref, ws)).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return [r.detach() for r in ref], {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.grad is not None}, ws


def _noise(a32, b64):
    return float((a32.double() - b64).abs().max()) / max(1.0, float(b64.abs().max()))


@pytest.mark.parametrize("D,aggs,scalers", CONV_CASES[:3])
def test_pna_transformer_sum_var_fused_step(D, aggs, scalers):
    """PNATransformer (2 PNA layers of width 32, d_model 32, cls pooling, three heads) with the new aggregators: (a) stays on the fused
    step, (b) which matches the float64 oracle in outputs and every parameter gradient, (c) and the module-by-module path.
    (b) uses tests/test_hip_pna.py's rule for the reference's fp32 std / var conditioning: max(1e-4, 3 x the noise of the oracle's own
    fp32 evaluation against its float64 one), per tensor; the figures are printed before they are asserted."""
    from graphtrans_amd import engine
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.pna_transformer import PNATransformer
    from oracle.reference_math import default_args

    torch.manual_seed(1)
    args = default_args(gnn_emb_dim=D, gnn_num_layer=2, gnn_residual=True, gnn_dropout=0.0, d_model=32, nhead=2, dim_feedforward=48,
                        transformer_dropout=0.0, num_encoder_layers=2, transformer_norm_input=True, aggregators=aggs, scalers=scalers,
                        deg=DEG, graph_pooling="cls", max_seq_len=3)
    b = _tiny_batch(5)
    model = PNATransformer(7, ASTNodeEncoder(D, 11, 13, 20), None, args)
    _randomize(model, 11)
    model.train()
    ref, gref, ws = _oracle_run(model, args, b, torch.float64)
    ref32, gref32, _ = _oracle_run(model, args, b, torch.float32, ws)
    model = model.to(DEV)
    bd = b.to(DEV)
    module_path = copy.deepcopy(model)
    module_path.fused = False
    assert engine.eligible(model, bd, None) and not engine.eligible(module_path, bd, None)                     # (a)
    outs = []
    for m in (model, module_path):
        out = m(bd)
        sum((o * w.float().to(DEV)).sum() for o, w in zip(out, ws)).backward()
        outs.append(out)
    failures = []

    def close64(got, want, noise, what):
        tol = max(1e-4, 3 * noise)
        err = float((got.double().cpu() - want).abs().max()) / max(1.0, float(want.abs().max()))
        print(f"{what}: err {err:.3e} (scale-relative), oracle fp32 noise {noise:.3e}, tol {tol:.3e}")
        try:
            assert_close(got.double().cpu(), want, atol=tol, rtol=tol, what=what)
        except AssertionError as e:
            failures.append(str(e))

    for i, (o, r, r32) in enumerate(zip(outs[0], ref, ref32)):                                                 # (b)
        close64(o.detach(), r, _noise(r32, r), f"out{i}")
    for k, p in model.named_parameters():
        if k in gref:
            close64(p.grad, gref[k], _noise(gref32[k], gref[k]), f"grad {k}")
    assert not failures, "\n".join(failures)
    for i, (o, r) in enumerate(zip(*outs)):                                                                    # (c)
        assert_close(o.detach().cpu(), r.detach().cpu(), what=f"fused vs module out{i}")
    for (k, p), (_, q) in zip(model.named_parameters(), module_path.named_parameters()):
        assert p.grad is not None and q.grad is not None, k
        assert_close(p.grad.cpu(), q.grad.cpu(), what=f"fused vs module grad {k}")


def test_pna_layer_rejects_other_slot_counts():
    """gt_pna_layer::agg_slots: 5 is GT_ERR_INVALID_ARG in both directions; 0 (a zeroed struct) sizes and checks like 4, 6 sizes the
    operand at 7 F.  Every call here returns before any launch."""
    from graphtrans_amd import _lib, layers

    L = _lib.lib()
    N, D, T, S = 1000, 64, 4, 3

    def desc(slots):
        d = layers.PnaLayerDesc()
        d.N, d.D, d.T, d.S, d.agg_slots = N, D, T, S, slots
        return d

    buf = torch.zeros(64, device=DEV)
    p = C.c_void_p(buf.data_ptr())
    for slots, named in ((5, True), (-1, True), (0, False), (4, False), (6, False)):
        d = desc(slots)   # every pointer of the descriptor is null: the classic and extended layouts stop at that check instead
        assert L.gt_pna_layer_fwd(C.byref(d), p, p, p, p, 0, None) == -1   # GT_ERR_INVALID_ARG
        assert (b"agg_slots" in L.gt_last_error()) == named
        assert L.gt_pna_layer_bwd(C.byref(d), p, p, p, p, p, p, 0, None) == -1
        assert (b"agg_slots" in L.gt_last_error()) == named
    saved = {s: L.gt_pna_layer_saved_bytes(C.byref(desc(s))) for s in (0, 4, 6)}
    work = {s: L.gt_pna_layer_workspace_bytes(C.byref(desc(s))) for s in (0, 4, 6)}
    assert saved[0] == saved[4] and work[0] == work[4]
    assert saved[6] - saved[4] >= 2 * N * D * 4 and work[6] - work[4] >= 2 * N * D * 4
