"""The GNN baseline model (graphtrans_amd/models/gnn.py, model_type "gnn") without a GPU: registry and alias, the constructor's
contract, the state_dict keys, the read-out mode of the whole-model driver on the host (gt_model_prepare / gt_model_grad_ranges), and --
where the reference tree is on the box -- the pin of the chain

    reference models/gnn.py (fp32, float64)  <->  `gnn_statement` below (float64, built from oracle/reference_math.py pieces)

in a child process that binds the reference the way oracle/make_golden.py does.  The same child records
tests/golden/gnn_baseline_ref.json (two tiny configurations run by the reference itself: inputs, weights, logits, parameter
gradients), which tests/test_hip_gnn_baseline.py loads on the GPU box.

`gnn_statement`, `statement_run` and `load_fixture` are imported by the GPU tests: the statement is written once, here.
"""
import ctypes as C
import copy
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import assert_close

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
FIXTURE = os.path.join(REPO, "tests", "golden", "gnn_baseline_ref.json")
needs_ref = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "models", "gnn.py")), reason="the reference tree is not on this box")


def _args(**kw):
    a = dict(gnn_virtual_node=False, gnn_num_layer=3, gnn_emb_dim=16, gnn_JK="last", gnn_dropout=0.0, gnn_residual=False,
             gnn_type="gcn", graph_pooling="mean", max_seq_len=None, model_type="gnn")
    a.update(kw)
    return SimpleNamespace(**a)


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 statement of models/gnn.py:98-115
# ---------------------------------------------------------------------------------------------------------------------------------
def gnn_statement(sd, args, data, perturb=None, training=True):
    """GNN.forward: gnn_node -> global_add / mean / max_pool -> head(s), from oracle/reference_math.py pieces, in the dtype of `sd`."""
    from oracle import reference_math as rm

    h = rm.gnn_node(sd, "gnn_node", args, data, perturb, training)
    B = int(data.batch[-1]) + 1
    if args.graph_pooling == "sum":
        hg = rm.segment_sum(h, data.batch, B)
    elif args.graph_pooling == "mean":
        hg = rm.scatter_mean(h, data.batch, B)
    elif args.graph_pooling == "max":
        hg = rm.scatter_minmax(h, data.batch, B, "max")
    else:
        raise ValueError(args.graph_pooling)
    if args.max_seq_len is None:
        return rm.linear(hg, sd, "graph_pred_linear")
    return [rm.linear(hg, sd, f"graph_pred_linear_list.{i}") for i in range(args.max_seq_len)]


def statement_run(state_dict, args, b, loss_of, dtype=torch.float64, perturb=None):
    """-> (outputs, loss, {parameter key: gradient}[, d perturb]) of `gnn_statement` at `state_dict` in `dtype` (test_hip_configs.oracle_run
    for this model)."""
    sd = {k: (v.detach().cpu().to(dtype).requires_grad_(True) if v.is_floating_point() else v.detach().cpu().clone()) for k, v in state_dict.items()}
    oargs = SimpleNamespace(**{k: v for k, v in vars(args).items() if k not in ("compute_dtype", "token_layout")})
    bb = copy.copy(b)
    for k in ("x", "edge_attr"):
        v = getattr(bb, k, None)
        if v is not None and v.is_floating_point():
            setattr(bb, k, v.to(dtype))
    pt = None if perturb is None else perturb.detach().cpu().to(dtype).requires_grad_(True)
    torch.set_default_dtype(dtype)   # the oracle's helpers allocate zeros / ones in the default dtype
    try:
        out = gnn_statement(sd, oargs, bb, pt, True)
        loss = loss_of(out)
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    grads = {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.requires_grad and v.grad is not None}
    return (out, loss.detach(), grads) if pt is None else (out, loss.detach(), grads, pt.grad)


# ---------------------------------------------------------------------------------------------------------------------------------
# registry, constructor, state_dict
# ---------------------------------------------------------------------------------------------------------------------------------
def _encoders(feat, D):
    from graphtrans_amd.encoders import ASTNodeEncoder
    if feat == "code2":
        return ASTNodeEncoder(D, 11, 13, 20), (lambda d: torch.nn.Linear(2, d))
    return torch.nn.Linear(6, D), (lambda d: (lambda _e: 0))   # dataset/tud.py:65-71


def _build(args, feat="code2"):
    from graphtrans_amd.models.gnn import GNN
    ne, ee = _encoders(feat, args.gnn_emb_dim)
    return GNN(5, ne, ee, args)


def test_registry_and_alias():
    import argparse

    from graphtrans_amd.models import MODELS, get_model_and_parser
    from graphtrans_amd.models.gnn import GNN
    assert MODELS["gnn"] is GNN
    from models.gnn import GNN as aliased
    assert aliased is GNN
    parser = argparse.ArgumentParser()
    assert get_model_and_parser(SimpleNamespace(model_type="gnn"), parser) is GNN
    assert GNN.get_emb_dim(_args(gnn_emb_dim=48)) == 48
    assert GNN.name(_args(gnn_type="gin", gnn_virtual_node=True)) == "gnn+gin-virtual" and GNN.name(_args()) == "gnn+gcn"
    assert set(MODELS) == {"gnn", "gnn-transformer", "pna-transformer"}


def test_constructor_contract():
    with pytest.raises(ValueError):
        _build(_args(gnn_num_layer=1))
    with pytest.raises(ValueError):
        _build(_args(graph_pooling="median"))
    for pooling in ("attention", "set2set"):
        with pytest.raises(NotImplementedError, match=pooling):
            _build(_args(graph_pooling=pooling))
    with pytest.raises(ValueError, match="cat"):
        _build(_args(gnn_JK="cat"))
    for pooling in ("sum", "mean", "max"):
        assert _build(_args(graph_pooling=pooling)).graph_pooling == pooling


def expected_keys(args, feat="code2", num_tasks=5):
    """{state_dict key: shape} of models/gnn.py:31-96 over modules/gnn_module.py, written out by hand"""
    D, L = args.gnn_emb_dim, args.gnn_num_layer
    k = {}

    def lin(p, o, i):
        k[p + ".weight"], k[p + ".bias"] = (o, i), (o,)

    def bn(p, n):
        k[p + ".weight"] = k[p + ".bias"] = k[p + ".running_mean"] = k[p + ".running_var"] = (n,)
        k[p + ".num_batches_tracked"] = ()
    g = "gnn_node."
    if feat == "code2":
        k[g + "node_encoder.type_encoder.weight"], k[g + "node_encoder.attribute_encoder.weight"] = (11, D), (13, D)
        k[g + "node_encoder.depth_encoder.weight"] = (21, D)
    else:
        lin(g + "node_encoder", D, 6)
    for l in range(L):
        c = f"{g}convs.{l}"
        if args.gnn_type == "gcn":
            lin(c + ".linear", D, D)
            k[c + ".root_emb.weight"] = (1, D)
        else:
            k[c + ".eps"] = (1,)
            lin(c + ".mlp.0", 2 * D, D)
            bn(c + ".mlp.1", 2 * D)
            lin(c + ".mlp.3", D, 2 * D)
        if feat == "code2":
            lin(c + ".edge_encoder", D, 2)
        bn(f"{g}batch_norms.{l}", D)
    if args.gnn_virtual_node:
        k[g + "virtualnode_embedding.weight"] = (1, D)
        for l in range(L - 1):
            m = f"{g}mlp_virtualnode_list.{l}"
            lin(m + ".0", 2 * D, D)
            bn(m + ".1", 2 * D)
            lin(m + ".3", D, 2 * D)
            bn(m + ".4", D)
    if args.max_seq_len is None:
        lin("graph_pred_linear", num_tasks, D)
    else:
        for i in range(args.max_seq_len):
            lin(f"graph_pred_linear_list.{i}", num_tasks, D)
    return k


@pytest.mark.parametrize("msl", [None, 3])
@pytest.mark.parametrize("vn", [False, True], ids=["plain", "virtual"])
@pytest.mark.parametrize("gnn_type", ["gcn", "gin"])
def test_state_dict_keys_on_meta(gnn_type, vn, msl):
    args = _args(gnn_type=gnn_type, gnn_virtual_node=vn, max_seq_len=msl)
    with torch.device("meta"):
        model = _build(args)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert got == expected_keys(args)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference itself, in a child process (the parent's `models` / `modules` are this repository's alias packages)
# ---------------------------------------------------------------------------------------------------------------------------------
SIZES = (9, 1, 12, 6)
REF_CASES = [(pool, gnn_type, vn, msl) for pool in ("sum", "mean", "max") for gnn_type in ("gcn", "gin") for vn in (False, True)
             for msl in (None, 3)]
FIXTURE_CASES = [dict(name="gcn-virtual-mean", feat="code2", gnn_type="gcn", gnn_virtual_node=True, graph_pooling="mean"),
                 dict(name="gin-max", feat="tud", gnn_type="gin", gnn_virtual_node=False, graph_pooling="max")]


def _tensor_json(t):
    t = t.detach().cpu()
    return dict(dtype=str(t.dtype).replace("torch.", ""), shape=list(t.shape), data=t.reshape(-1).tolist())


def _tensor_from(d):
    return torch.tensor(d["data"], dtype=getattr(torch, d["dtype"])).reshape(d["shape"])


def load_fixture(path=FIXTURE):
    """-> [dict(name, feat, args (SimpleNamespace), inputs, sd, logits, grads)] with tensors"""
    with open(path) as f:
        raw = json.load(f)
    out = []
    for c in raw["configs"]:
        out.append(dict(name=c["name"], feat=c["feat"], args=SimpleNamespace(**c["args"]),
                        inputs={k: _tensor_from(v) for k, v in c["inputs"].items()}, sd={k: _tensor_from(v) for k, v in c["sd"].items()},
                        logits=_tensor_from(c["logits"]), grads={k: _tensor_from(v) for k, v in c["grads"].items()}))
    return out


def fixture_batch(inputs):
    from graphtrans_amd.data import Batch
    d = {k: inputs[k] for k in ("x", "edge_index", "edge_attr", "batch", "node_depth") if k in inputs}
    d.setdefault("edge_attr", None)
    return Batch(**d)


def _child(out_path):
    """Runs with the REFERENCE's `models` / `modules` bound (oracle/make_golden.py's binding, loaded as a module): every comparison of
    the pin, the measured gaps and the fixture's content into `out_path` (JSON)."""
    import importlib.util
    import inspect

    torch.set_num_threads(1)
    spec = importlib.util.spec_from_file_location("mg", os.path.join(REPO, "oracle", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    from models.gnn import GNN as RefGNN
    assert os.path.realpath(inspect.getsourcefile(RefGNN)).startswith(REF + os.sep)
    from graphtrans_amd import synth
    from graphtrans_amd.models.gnn import GNN

    def ref_encoders(feat, D):
        return mg.make_node_encoder(feat, D), mg.edge_cls("linear" if feat == "code2" else "none")

    def run_ref(model, b, loss_of, dtype):
        m = copy.deepcopy(model).to(dtype).train()
        bb = copy.copy(b)
        for k in ("x", "edge_attr"):
            v = getattr(bb, k, None)
            if v is not None and v.is_floating_point():
                setattr(bb, k, v.to(dtype))
        if hasattr(bb, "node_depth"):
            bb.node_depth = bb.node_depth.clone()   # the reference's ASTNodeEncoder clamps its input in place
        out = m(bb)
        loss_of(out).backward()
        outs = list(out) if isinstance(out, (list, tuple)) else [out]
        return [o.detach() for o in outs], {k: p.grad.detach() for k, p in m.named_parameters() if p.grad is not None}

    def weighted(ws):
        return lambda out: sum((o * w.to(o.dtype)).sum() for o, w in zip(out if isinstance(out, (list, tuple)) else [out], ws))

    report = dict(cases=[], configs=[])
    for i, (pool, gnn_type, vn, msl) in enumerate(REF_CASES):
        feat = "code2" if i % 3 else "tud"
        D = 16
        args = _args(graph_pooling=pool, gnn_type=gnn_type, gnn_virtual_node=vn, max_seq_len=msl, gnn_emb_dim=D)
        torch.manual_seed(0)
        b = synth.tiny_mixed(seed=40 + i, sizes=SIZES, feat=feat)
        ne, ee = ref_encoders(feat, D)
        ref = RefGNN(5, ne, ee, args)
        mg.randomize(ref, 60 + i)
        # same keys and shapes as this repository's model
        with torch.device("meta"):
            mine = _build(args, feat)
        ref_keys = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
        assert ref_keys == {k: tuple(v.shape) for k, v in mine.state_dict().items()} == expected_keys(args, feat), (pool, gnn_type, vn, msl)
        g = torch.Generator().manual_seed(1234)
        ws = [torch.randn(len(SIZES), 5, generator=g) for _ in range(msl or 1)]
        loss_of = weighted(ws)
        o32, g32 = run_ref(ref, b, loss_of, torch.float32)
        o64, g64 = run_ref(ref, b, loss_of, torch.float64)
        so, _, sg = statement_run(ref.state_dict(), args, b, loss_of, torch.float64)
        so = list(so) if isinstance(so, (list, tuple)) else [so]
        case = dict(case=f"{pool},{gnn_type},vn={vn},max_seq_len={msl},{feat}", out_gap=0.0, grad_gap=0.0, out_noise=0.0, grad_noise=0.0, wiring=0.0)

        def cmp(kind, key, a32, a64, st):
            # the bound of tests/test_oracle_golden.py: 1e-4, or 3 x the reference's OWN fp32-vs-float64 noise on that tensor where larger
            noise = float((a32.double() - a64).abs().max()) / max(1.0, float(a64.abs().max()))
            tol = max(1e-4, 3 * noise)
            gap = float((a32.double() - st).abs().max()) / max(1.0, float(st.abs().max()))
            case[kind + "_gap"], case[kind + "_noise"] = max(case[kind + "_gap"], gap), max(case[kind + "_noise"], noise)
            case["wiring"] = max(case["wiring"], float((a64 - st).abs().max()) / max(1.0, float(st.abs().max())))
            assert_close(a64, st, atol=1e-9, rtol=1e-9, what=f"{case['case']} float64 {kind} {key}")   # the same math: the wiring
            assert_close(a32, st, atol=tol, rtol=tol, what=f"{case['case']} fp32 {kind} {key}")
        for j, (a, c, s) in enumerate(zip(o32, o64, so)):
            cmp("out", str(j), a, c, s.detach())
        assert set(g32) == set(g64)
        for k in g64:
            cmp("grad", k, g32[k], g64[k], sg[k] if k in sg else torch.zeros_like(g64[k]))
        report["cases"].append(case)
    # ---- the fixture: two configurations run by the reference, D = 8, L = 2, B = 4
    for c in FIXTURE_CASES:
        args = _args(gnn_type=c["gnn_type"], gnn_virtual_node=c["gnn_virtual_node"], graph_pooling=c["graph_pooling"], gnn_emb_dim=8,
                     gnn_num_layer=2)
        torch.manual_seed(0)
        b = synth.tiny_mixed(seed=77, sizes=SIZES, feat=c["feat"])
        ne, ee = ref_encoders(c["feat"], 8)
        ref = RefGNN(5, ne, ee, args)
        mg.randomize(ref, 91)
        with torch.no_grad():   # logits of O(1): the randomised weights are large
            for p in ref.parameters():
                if p.dim() > 1 and p.shape[0] > 1:
                    p.mul_(0.5)
        inputs = {k: v.clone() for k, v in mg.batch_inputs(b).items()}
        o32, g32 = run_ref(ref, b, lambda out: out.square().mean(), torch.float32)
        report["configs"].append(dict(name=c["name"], feat=c["feat"], args=vars(args), inputs={k: _tensor_json(v) for k, v in inputs.items()},
                                      sd={k: _tensor_json(v) for k, v in ref.state_dict().items()}, logits=_tensor_json(o32[0]),
                                      grads={k: _tensor_json(v) for k, v in g32.items()}))
    with open(out_path, "w") as f:
        json.dump(report, f)


@pytest.fixture(scope="module")
def ref_report(tmp_path_factory):
    out = tmp_path_factory.mktemp("gnn_ref") / "report.json"
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--ref-child", str(out)], cwd=REPO, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    with open(out) as f:
        return json.load(f)


@needs_ref
def test_reference_gnn_equals_the_float64_statement(ref_report):
    """Every (pooling, conv, virtual node, max_seq_len) case: same keys and shapes as this repository's GNN, the float64 reference equal
    to the statement at 1e-9 (same math), the fp32 reference within max(1e-4, 3 x its own fp32-vs-float64 noise) of it (asserted in
    the child, tensor by tensor; the figures are printed here)."""
    cases = ref_report["cases"]
    assert len(cases) == len(REF_CASES) == 24
    for c in cases:
        print(f"[{c['case']}] fp32 reference vs float64 statement: logits {c['out_gap']:.2e} (reference's own noise {c['out_noise']:.2e}), "
              f"gradients {c['grad_gap']:.2e} ({c['grad_noise']:.2e}); float64 reference vs statement {c['wiring']:.1e}")
        assert c["wiring"] <= 1e-9 and c["out_gap"] <= max(1e-4, 3 * c["out_noise"]) and c["grad_gap"] <= max(1e-4, 3 * c["grad_noise"])


@needs_ref
def test_fixture_is_what_the_reference_gives(ref_report):
    """tests/golden/gnn_baseline_ref.json regenerated by the child: integer inputs and shapes equal, float values within 1e-5 of the
    tensor's scale -- a tolerance, not bit equality: the reference runs fp32 torch CPU kernels (index_add_, GEMM, BatchNorm reductions)
    whose summation order follows the thread count and the BLAS build of the box."""
    kept = load_fixture()
    with open(FIXTURE) as f:
        raw = json.load(f)
    assert os.path.getsize(FIXTURE) < 200 * 1024
    made = ref_report["configs"]
    assert [c["name"] for c in made] == [c["name"] for c in raw["configs"]] == [c["name"] for c in FIXTURE_CASES]
    for new, old_raw, old in zip(made, raw["configs"], kept):
        assert new["args"] == old_raw["args"] and new["feat"] == old_raw["feat"]
        for part in ("inputs", "sd", "grads"):
            assert sorted(new[part]) == sorted(old_raw[part]), part
            for k, v in new[part].items():
                t = _tensor_from(v)
                if t.is_floating_point():
                    assert_close(t, old[part][k], atol=1e-5, rtol=1e-5, what=f"{new['name']} {part} {k}")
                else:
                    assert torch.equal(t, old[part][k]), (new["name"], part, k)
        assert_close(_tensor_from(new["logits"]), old["logits"], atol=1e-5, rtol=1e-5, what=new["name"] + " logits")


def test_fixture_agrees_with_the_statement():
    """(no reference needed) the recorded fp32 logits and gradients against the float64 statement at the recorded weights: 1e-4"""
    for c in load_fixture():
        b = fixture_batch(c["inputs"])
        out, _, grads = statement_run(c["sd"], c["args"], b, lambda o: o.square().mean(), torch.float64)
        assert_close(c["logits"], out.detach(), what=c["name"] + " logits")
        assert set(grads) >= set(c["grads"])
        for k, v in c["grads"].items():
            assert_close(v, grads[k], what=f"{c['name']} grad {k}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the driver's read-out mode, host only (gt_model_prepare asks sizes and dispatch questions: no device call)
# ---------------------------------------------------------------------------------------------------------------------------------
INVALID = -1   # GT_ERR_INVALID_ARG


def _driver_model(readout=2, L=3, D=32, Nh=15, has_vn=True):
    """A gt_model as the plan fills it for a GCN read-out model, written out by hand: model_layout.ModelLayout (step 1 of a plan: offsets
    and every other non-pointer field) and engine.bind_storage (step 2: pointers) build the real one, and
    tests/test_model_layout_host.py holds it against this one; device pointers are made-up addresses (never followed on the host)"""
    from graphtrans_amd import engine, layers
    fake = 0x10000
    keep = []
    cm = engine.ModelDesc()
    cm.conv, cm.L, cm.n_enc, cm.has_vn, cm.jk_cat, cm.residual = 0, L, 0, int(has_vn), 0, 0
    cm.embed_kind, cm.n_tables, cm.vn0_in_embed, cm.embed_sorted = 2, 3, int(has_vn), 1
    cm.D, cm.d, cm.Nh, cm.ldy = D, D, Nh, (Nh + 3) // 4 * 4
    conv = (layers.GcnLayerDesc * L)()
    vn = (layers.VnUpdateDesc * max(L - 1, 1))()
    for l in range(L):
        conv[l].D = D
        conv[l].edge_mode, conv[l].edge_cols = 1, 2   # GT_EDGE_LINEAR
    for l in range(L - 1):
        vn[l].D = D
    keep += [conv, vn]
    cm.conv_layers = C.cast(conv, C.c_void_p)
    cm.vn = C.cast(vn, C.c_void_p) if has_vn else None
    off = 0
    for t, rows in enumerate((11, 13, 21)):
        cm.tables[t], cm.table_rows[t], cm.table_clamp[t] = fake * (t + 1), rows, (20 if t == 2 else -1)
        cm.off_tables[t] = off
        off += rows * D
    cm.off_ne_w = cm.off_ne_b = -1
    cm.off_vn_emb = off if has_vn else -1
    off += D if has_vn else 0
    per_conv = D * D + D + D + 2 * D + D + 2 * D
    for l in range(L):
        cm.off_conv[l] = off
        off += per_conv
    if has_vn:
        for l in range(L - 1):
            cm.off_vn[l] = off
            off += 2 * D * D + 2 * D + 4 * D + 2 * D * D + D + 2 * D
    for k in ("off_g2t_w", "off_g2t_b", "off_cls", "off_nin_w", "off_nin_b", "off_nout_w", "off_nout_b"):
        setattr(cm, k, -1)
    cm.off_head_w = off
    off += (Nh * D + 3) // 4 * 4
    cm.off_head_b = off
    off += (Nh + 3) // 4 * 4
    cm.grad_total = off
    cm.vn_emb = fake * 9 if has_vn else None
    cm.head_w, cm.head_b, cm.zero_i64 = fake * 10, fake * 11, fake * 12
    cm.readout = readout
    return cm, keep


def _driver_batch(sizes=(5, 70, 9, 3, 200)):
    from graphtrans_amd import engine
    sizes = np.ascontiguousarray(sizes, np.int64)
    bt = engine.BatchDesc()
    bt.N, bt.E, bt.B = int(sizes.sum()), 2 * int(sizes.sum()), sizes.size
    bt.edge_index, bt.batch, bt.sizes_host = 0x20000, 0x30000, sizes.ctypes.data
    bt.x, bt.x_stride0, bt.x_stride1, bt.node_depth, bt.depth_stride, bt.edge_attr = 0x40000, 2, 1, 0x50000, 1, 0x60000
    bt.zeros_B, bt.ident_B, bt.ptr01 = 0x70000, 0x80000, 0x90000
    bt.training, bt.compute, bt.tdt, bt.will_bwd = 1, 0, 0, 1
    return bt, sizes


def _prepare(cm, bt):
    from graphtrans_amd import _lib, engine
    L = _lib.lib()
    ctx = C.create_string_buffer(int(L.gt_model_ctx_bytes()))
    sz = engine.SizesDesc()
    rc = L.gt_model_prepare(C.byref(cm), C.byref(bt), ctx, C.byref(sz))
    return rc, sz, L.gt_last_error()


def test_abi_sizes_match_the_mirrors():
    from graphtrans_amd import _lib, engine
    from graphtrans_amd.graph import StageRingDesc
    out = (C.c_int64 * 4)()
    _lib.check(_lib.lib().gt_model_abi_sizes(out), "gt_model_abi_sizes")
    assert tuple(out) == (C.sizeof(engine.ModelDesc), C.sizeof(engine.BatchDesc), C.sizeof(engine.ImageSet), C.sizeof(StageRingDesc))
    names = [f[0] for f in engine.ModelDesc._fields_]
    assert names[-4:] == ["readout", "pad_readout_", "pe", "pe_rows"]   # in front of the tail tests/test_pos_encoder_host.py pins
    assert engine.ModelDesc().readout == 0                              # a zeroed struct is the token path


@pytest.mark.parametrize("readout", [1, 2, 3], ids=["sum", "mean", "max"])
@pytest.mark.parametrize("has_vn", [True, False], ids=["virtual", "plain"])
def test_readout_prepare_builds_no_token_layout(readout, has_vn):
    cm, keep = _driver_model(readout=readout, has_vn=has_vn)
    bt, sizes = _driver_batch()
    rc, sz, err = _prepare(cm, bt)   # (bt.ring is NULL: a staging-ring slot would have been an error)
    assert rc == 0, err
    assert sz.rows == 0 and sz.num_work == 0 and sz.max_npos == 0 and sz.exact == 1
    N, B, D = int(sizes.sum()), sizes.size, 32
    assert sz.arena_bytes >= 4 * (3 + 1) * N * D + 4 * B * D and sz.barena_bytes >= 4 * 4 * N * D
    # max carries the winning rows [B][D] int32 on top of what sum needs
    if readout == 3:
        cm1, keep1 = _driver_model(readout=1, has_vn=has_vn)
        assert sz.arena_bytes > _prepare(cm1, bt)[1].arena_bytes


@pytest.mark.parametrize("has_vn", [True, False], ids=["virtual", "plain"])
def test_readout_grad_ranges_tile_the_buffer_heads_first(has_vn):
    from graphtrans_amd import _lib
    cm, keep = _driver_model(has_vn=has_vn)
    lo, hi = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    _lib.check(_lib.lib().gt_model_grad_ranges(C.byref(cm), lo, hi), "gt_model_grad_ranges")
    r = list(zip(lo, hi))
    assert r[0] == (cm.off_head_w, cm.grad_total)                     # stage 1: the heads
    assert r[1][1] == cm.off_head_w and r[2] == (0, r[1][0])          # message passing up to the heads, the input encoder below it
    assert r[1][0] == (cm.off_vn_emb if has_vn else cm.off_conv[0])
    assert all(a < b for a, b in r)
    assert sorted(r) == [r[2], r[1], r[0]] and r[2][0] == 0 and r[0][1] == cm.grad_total   # they tile [0, grad_total)


def test_readout_rejects_what_the_mode_does_not_build():
    from graphtrans_amd import layers
    bt, sizes = _driver_batch()

    def bad(change):
        cm, keep = _driver_model()
        b2, _ = _driver_batch()
        b2.sizes_host = sizes.ctypes.data
        change(cm, b2, keep)
        return _prepare(cm, b2)[0]

    def with_encoder(cm, b, keep):
        enc = (layers.EncoderLayerDesc * 1)()
        keep.append(enc)
        cm.n_enc, cm.enc, cm.d = 1, C.cast(enc, C.c_void_p), 32

    def with_pe(cm, b, keep):
        cm.pe, cm.pe_rows = 0xA0000, 5000

    assert bad(lambda cm, b, keep: None) == 0
    assert bad(with_encoder) == INVALID
    assert bad(lambda cm, b, keep: setattr(cm, "jk_cat", 1)) == INVALID
    assert bad(with_pe) == INVALID
    assert bad(lambda cm, b, keep: setattr(b, "gnn_frozen", 1)) == INVALID
    assert bad(lambda cm, b, keep: setattr(cm, "conv", 2)) == INVALID       # no PNA stack in this mode
    assert bad(lambda cm, b, keep: setattr(cm, "readout", 7)) == INVALID    # not a GT_POOL_* kind
    # the token path still needs its encoder: readout == 0 with n_enc == 0 is rejected as before
    assert bad(lambda cm, b, keep: setattr(cm, "readout", 0)) == INVALID


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--ref-child":
        _child(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "--write-fixture":   # (re)record tests/golden/gnn_baseline_ref.json from the reference
        _child(FIXTURE + ".tmp")
        with open(FIXTURE + ".tmp") as f:
            configs = json.load(f)["configs"]
        os.remove(FIXTURE + ".tmp")
        with open(FIXTURE, "w") as f:
            json.dump(dict(configs=configs), f)
        print(FIXTURE, os.path.getsize(FIXTURE), "bytes")
    else:
        sys.exit("usage: test_gnn_baseline_host.py --ref-child OUT.json | --write-fixture")
