"""The PNA baseline model (graphtrans_amd/models/pna.py, model_type "pna") without a GPU: registry and alias, the constructor's contract,
the state_dict keys, the read-out mode of the whole-model driver with the PNA stack and the two head kinds on the host (gt_model_prepare /
gt_model_grad_ranges), and -- where the reference tree is on the box -- the pin of the chain

    reference models/pna.py (fp32, float64)  <->  `pna_net_statement` below (float64, built from oracle/reference_math.py pieces)

in a child process that binds the reference the way oracle/make_golden.py::_load_ref_pna does.  The same child records
tests/golden/pna_baseline_ref.json (two tiny configurations run by the reference itself: inputs, weights, logits, parameter gradients),
which tests/test_hip_pna_baseline.py loads on the GPU box.

`pna_net_statement`, `statement_run` and `load_fixture` are imported by the GPU tests: the statement is written once, here.
"""
import argparse
import base64
import copy
import ctypes as C
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import assert_close
from test_gnn_baseline_host import INVALID, _driver_batch, _prepare, fixture_batch
from test_gnn_baseline_host import _driver_model as _gnn_driver_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
FIXTURE = os.path.join(REPO, "tests", "golden", "pna_baseline_ref.json")
needs_ref = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "models", "pna.py")), reason="the reference tree is not on this box")
DEG_HIST = [0, 41, 30, 12, 6, 3, 1, 1]   # in-degree histogram (oracle/make_golden.py: PNA_DEG_HIST)
AGGS, SCALERS = ["mean", "max", "min", "std"], ["identity", "amplification", "attenuation"]


def _args(**kw):
    a = dict(gnn_num_layer=2, gnn_emb_dim=16, gnn_dropout=0.0, gnn_residual=True, graph_pooling="mean", max_seq_len=None, model_type="pna",
             aggregators=list(AGGS), scalers=list(SCALERS), deg=torch.tensor(DEG_HIST))
    a.update(kw)
    return SimpleNamespace(**a)


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 statement of models/pna.py:94-104
# ---------------------------------------------------------------------------------------------------------------------------------
def pna_net_statement(sd, args, data, perturb=None, training=True):
    """PNANet.forward: pna_module -> global_add / mean / max_pool -> mlp | per-position two-layer heads, from oracle/reference_math.py
    pieces, in the dtype of `sd`."""
    from oracle import reference_math as rm

    h = rm.pna_node_embedding(sd, "pna_module", args, data, perturb, training)
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
        return rm.linear(torch.relu(rm.linear(torch.relu(rm.linear(hg, sd, "mlp.0")), sd, "mlp.2")), sd, "mlp.4")
    return [rm.linear(torch.relu(rm.linear(hg, sd, f"graph_pred_linear_list.{i}.0")), sd, f"graph_pred_linear_list.{i}.2")
            for i in range(args.max_seq_len)]


def statement_run(state_dict, args, b, loss_of, dtype=torch.float64, perturb=None):
    """-> (outputs, loss, {parameter key: gradient}[, d perturb]) of `pna_net_statement` at `state_dict` in `dtype`
    (test_hip_configs.oracle_run for this model).  The node encoder is one module under two keys: the statement reads
    `pna_module.node_encoder.*`, whose gradient is reported under both."""
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
        out = pna_net_statement(sd, oargs, bb, pt, True)
        loss = loss_of(out)
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    grads = {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.requires_grad and v.grad is not None}
    for k in [k for k in grads if k.startswith("pna_module.node_encoder.")]:
        grads[k[len("pna_module."):]] = grads[k]
    return (out, loss.detach(), grads) if pt is None else (out, loss.detach(), grads, pt.grad)


# ---------------------------------------------------------------------------------------------------------------------------------
# registry, constructor, state_dict
# ---------------------------------------------------------------------------------------------------------------------------------
def _encoder(feat, D):
    from graphtrans_amd.encoders import ASTNodeEncoder
    return ASTNodeEncoder(D, 11, 13, 20) if feat == "code2" else torch.nn.Linear(6, D)   # dataset/tud.py:65


def _build(args, feat="code2", num_tasks=5):
    from graphtrans_amd.models.pna import PNANet
    return PNANet(num_tasks, _encoder(feat, args.gnn_emb_dim), None, args)


def test_registry_and_alias():
    from graphtrans_amd.models import ABLATION_MODELS, MODELS, get_model_and_parser
    from graphtrans_amd.models.pna import PNANet
    parser = argparse.ArgumentParser()
    parser.add_argument("--gnn_residual", default=False)
    parser.add_argument("--gnn_dropout", type=float, default=0.0)
    parser.add_argument("--gnn_emb_dim", type=int, default=300)
    parser.add_argument("--gnn_num_layer", type=int, default=5)
    assert get_model_and_parser(SimpleNamespace(model_type="pna"), parser) is PNANet
    ns = parser.parse_args(["--aggregators", "mean", "sum"])           # the parser now knows the PNA flags
    assert ns.aggregators == ["mean", "sum"] and ns.scalers == SCALERS and ns.gnn_emb_dim == 70 and ns.gnn_residual is True
    assert set(MODELS) == {"gnn", "gnn-transformer", "pna-transformer"} and ABLATION_MODELS == {"pna": PNANet}
    for name, cls in MODELS.items():                                    # the first table is looked up as before
        assert get_model_and_parser(SimpleNamespace(model_type=name), argparse.ArgumentParser(conflict_handler="resolve")) is cls
    with pytest.raises(KeyError):
        get_model_and_parser(SimpleNamespace(model_type="transformer"), parser)
    from models.pna import PNANet as aliased
    assert aliased is PNANet
    assert PNANet.need_deg() is True and PNANet.get_emb_dim(_args(gnn_emb_dim=48)) == 48 and PNANet.name(_args()) == "pna"


def test_constructor_contract():
    with pytest.raises(ValueError):
        _build(_args(graph_pooling="median"))
    for pooling in ("attention", "set2set"):
        with pytest.raises(NotImplementedError, match=pooling):
            _build(_args(graph_pooling=pooling))
    for pooling in ("sum", "mean", "max"):
        m = _build(_args(graph_pooling=pooling))
        assert m.graph_pooling == pooling and m.gnn_node is m.pna_module and m.pna_module.node_encoder is m.node_encoder
    with pytest.raises(AttributeError):
        m.gnn_node = None                                               # read-only
    assert _build(_args()).fused_flag is False and _build(_args(fused_flag=True)).fused_flag is True


def expected_keys(args, feat="code2", num_tasks=5):
    """{state_dict key: shape} of models/pna.py:38-71 over modules/pna/pna_module.py:33-55 and modules/pna_layer.py:99-122, by hand"""
    D, L, T = args.gnn_emb_dim, args.gnn_num_layer, 4
    F = D // T
    k = {}

    def lin(p, o, i):
        k[p + ".weight"], k[p + ".bias"] = (o, i), (o,)
    for g in ("", "pna_module."):
        if feat == "code2":
            k[g + "node_encoder.type_encoder.weight"], k[g + "node_encoder.attribute_encoder.weight"] = (11, D), (13, D)
            k[g + "node_encoder.depth_encoder.weight"] = (21, D)
        else:
            lin(g + "node_encoder", D, 6)
    for l in range(L):
        c = f"pna_module.layers.{l}"
        for t in range(T):
            lin(f"{c}.pre_nns.{t}.0", F, 2 * F)
            lin(f"{c}.post_nns.{t}.0", F, (len(args.aggregators) * len(args.scalers) + 1) * F)
        lin(c + ".lin", D, D)
        b = f"pna_module.batch_norms.{l}.module"
        k[b + ".weight"] = k[b + ".bias"] = k[b + ".running_mean"] = k[b + ".running_var"] = (D,)
        k[b + ".num_batches_tracked"] = ()
    if args.max_seq_len is None:
        lin("mlp.0", 35, D)
        lin("mlp.2", 17, 35)
        lin("mlp.4", num_tasks, 17)
    else:
        for i in range(args.max_seq_len):
            lin(f"graph_pred_linear_list.{i}.0", D, D)
            lin(f"graph_pred_linear_list.{i}.2", num_tasks, D)
    return k


@pytest.mark.parametrize("msl", [None, 3])
@pytest.mark.parametrize("feat", ["code2", "tud"])
def test_state_dict_keys_on_meta(feat, msl):
    args = _args(max_seq_len=msl)
    with torch.device("meta"):
        model = _build(args, feat)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == expected_keys(args, feat)
    assert list(model.state_dict())[0].startswith("node_encoder.")     # registered first, as in the reference


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference itself, in a child process (the parent's `models` / `modules` are this repository's alias packages)
# ---------------------------------------------------------------------------------------------------------------------------------
SIZES = (9, 1, 12, 6)
FIXTURE_CASES = [dict(name="heads-mean", feat="code2", num_tasks=7, gnn_emb_dim=16, gnn_num_layer=2, max_seq_len=3, graph_pooling="mean"),
                 dict(name="mlp-max", feat="code2", num_tasks=3, gnn_emb_dim=16, gnn_num_layer=1, max_seq_len=None, graph_pooling="max")]


def _tensor_json(t):
    """fp32 values as base64 of their little-endian bytes (5.3 characters per value, exact), integers as a list"""
    t = t.detach().cpu().contiguous()
    d = dict(dtype=str(t.dtype).replace("torch.", ""), shape=list(t.shape))
    if t.dtype == torch.float32:
        d["b64"] = base64.b64encode(t.numpy().astype("<f4").tobytes()).decode()
    else:
        d["data"] = t.reshape(-1).tolist()
    return d


def _tensor_from(d):
    if "b64" in d:
        return torch.from_numpy(np.frombuffer(base64.b64decode(d["b64"]), dtype="<f4").copy()).reshape(d["shape"])
    return torch.tensor(d["data"], dtype=getattr(torch, d["dtype"])).reshape(d["shape"])


def _case_args(c):
    return _args(**{k: c[k] for k in ("gnn_emb_dim", "gnn_num_layer", "max_seq_len", "graph_pooling")})


def _args_json(args):
    return {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in vars(args).items()}


def load_fixture(path=FIXTURE):
    """-> [dict(name, feat, num_tasks, args (SimpleNamespace), inputs, sd, logits [per head], grads)] with tensors"""
    with open(path) as f:
        raw = json.load(f)
    out = []
    for c in raw["configs"]:
        a = dict(c["args"])
        a["deg"] = torch.tensor(a["deg"])
        sd = {k: _tensor_from(v) for k, v in c["sd"].items()}
        sd.update({"pna_module." + k: v for k, v in sd.items() if k.startswith("node_encoder.")})   # one module under two keys, stored once
        out.append(dict(name=c["name"], feat=c["feat"], num_tasks=c["num_tasks"], args=SimpleNamespace(**a),
                        out_noise=float(c["out_noise"]), grad_noise=float(c["grad_noise"]),
                        inputs={k: _tensor_from(v) for k, v in c["inputs"].items()}, sd=sd,
                        logits=[_tensor_from(v) for v in c["logits"]], grads={k: _tensor_from(v) for k, v in c["grads"].items()}))
    return out


def fixture_loss(out):
    outs = list(out) if isinstance(out, (list, tuple)) else [out]
    return sum(o.square().mean() for o in outs)


def _child(out_path):
    """Runs with the REFERENCE's `models` / `modules` bound (oracle/make_golden.py's binding, loaded as a module): every comparison of
    the pin, the measured gaps and the fixture's content into `out_path` (JSON)."""
    import importlib
    import importlib.util
    import inspect

    torch.set_num_threads(1)
    spec = importlib.util.spec_from_file_location("mg", os.path.join(REPO, "oracle", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg._load_ref_pna()   # binds the in-tree PNAConv where modules/pna/pna_module.py and models/pna.py import PyG's
    RefPNANet = importlib.import_module("models.pna").PNANet
    assert os.path.realpath(inspect.getsourcefile(RefPNANet)).startswith(REF + os.sep)
    from graphtrans_amd import synth

    def run_ref(model, b, loss_of, dtype):
        m = copy.deepcopy(model).to(dtype).train()
        bb = mg._B(x=b.x, edge_index=b.edge_index, edge_attr=getattr(b, "edge_attr", None), batch=b.batch,
                   node_depth=b.node_depth.clone())   # the reference's ASTNodeEncoder clamps its input in place
        out = m(bb)
        loss_of(out).backward()
        outs = list(out) if isinstance(out, (list, tuple)) else [out]
        return [o.detach() for o in outs], {k: p.grad.detach() for k, p in m.named_parameters() if p.grad is not None}

    report = dict(cases=[], configs=[])
    for i, c in enumerate(FIXTURE_CASES):
        args = _case_args(c)
        torch.manual_seed(0)
        b = synth.tiny_mixed(seed=77 + i, sizes=SIZES, feat=c["feat"])
        ref = RefPNANet(c["num_tasks"], mg.make_node_encoder(c["feat"], args.gnn_emb_dim), None, args)
        mg.randomize(ref, 91 + i)
        with torch.no_grad():   # logits of O(1): the randomised weights are large
            for p in ref.parameters():
                if p.dim() > 1 and p.shape[0] > 1:
                    p.mul_(0.5)
        with torch.device("meta"):
            mine = _build(args, c["feat"], c["num_tasks"])
        ref_keys = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
        assert ref_keys == {k: tuple(v.shape) for k, v in mine.state_dict().items()} == expected_keys(args, c["feat"], c["num_tasks"]), c["name"]
        assert list(ref.state_dict()) == list(mine.state_dict()), c["name"]   # the order too
        inputs = {k: v.clone() for k, v in mg.batch_inputs(b).items()}
        o32, g32 = run_ref(ref, b, fixture_loss, torch.float32)
        o64, g64 = run_ref(ref, b, fixture_loss, torch.float64)
        so, _, sg = statement_run(ref.state_dict(), args, b, fixture_loss, torch.float64)
        so = list(so) if isinstance(so, (list, tuple)) else [so]
        case = dict(case=c["name"], out_gap=0.0, grad_gap=0.0, out_noise=0.0, grad_noise=0.0, wiring=0.0)

        def cmp(kind, key, a32, a64, st):
            # the bound of tests/test_oracle_golden.py: 1e-4, or 3 x the reference's OWN fp32-vs-float64 noise on that tensor where larger
            noise = float((a32.double() - a64).abs().max()) / max(1.0, float(a64.abs().max()))
            tol = max(1e-4, 3 * noise)
            gap = float((a32.double() - st).abs().max()) / max(1.0, float(st.abs().max()))
            case[kind + "_gap"], case[kind + "_noise"] = max(case[kind + "_gap"], gap), max(case[kind + "_noise"], noise)
            case["wiring"] = max(case["wiring"], float((a64 - st).abs().max()) / max(1.0, float(st.abs().max())))
            assert_close(a64, st, atol=1e-9, rtol=1e-9, what=f"{case['case']} float64 {kind} {key}")   # the same math: the wiring
            assert_close(a32, st, atol=tol, rtol=tol, what=f"{case['case']} fp32 {kind} {key}")
        assert len(o32) == len(so) == (c["max_seq_len"] or 1)
        for j, (a, c64, s) in enumerate(zip(o32, o64, so)):
            cmp("out", str(j), a, c64, s.detach())
        assert set(g32) == set(g64)
        for k in g64:
            cmp("grad", k, g32[k], g64[k], sg[k] if k in sg else torch.zeros_like(g64[k]))
        report["cases"].append(case)
        # (out_noise / grad_noise: the reference's own fp32-vs-float64 distance on its worst tensor, max-scaled -- the fp32 `std`
        # aggregator cancels on in-degree <= 1 segments, oracle/make_golden.py:g12_pna -- the yardstick of every comparison with fp32 records)
        report["configs"].append(dict(name=c["name"], feat=c["feat"], num_tasks=c["num_tasks"], args=_args_json(args),
                                      out_noise=case["out_noise"], grad_noise=case["grad_noise"],
                                      inputs={k: _tensor_json(v) for k, v in inputs.items()},
                                      sd={k: _tensor_json(v) for k, v in ref.state_dict().items() if not k.startswith("pna_module.node_encoder.")},
                                      logits=[_tensor_json(o) for o in o32],
                                      grads={k: _tensor_json(v) for k, v in g32.items()}))
    with open(out_path, "w") as f:
        json.dump(report, f)


@pytest.fixture(scope="module")
def ref_report(tmp_path_factory):
    out = tmp_path_factory.mktemp("pna_ref") / "report.json"
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--ref-child", str(out)], cwd=REPO, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    with open(out) as f:
        return json.load(f)


@needs_ref
def test_reference_pna_net_equals_the_float64_statement(ref_report):
    """Both head forms: same keys, shapes and key order as this repository's PNANet, the float64 reference equal to the statement at 1e-9
    (same math), the fp32 reference within max(1e-4, 3 x its own fp32-vs-float64 noise) of it (asserted in the child, tensor by tensor;
    the figures are printed here)."""
    cases = ref_report["cases"]
    assert [c["case"] for c in cases] == [c["name"] for c in FIXTURE_CASES]
    for c in cases:
        print(f"[{c['case']}] fp32 reference vs float64 statement: logits {c['out_gap']:.2e} (reference's own noise {c['out_noise']:.2e}), "
              f"gradients {c['grad_gap']:.2e} ({c['grad_noise']:.2e}); float64 reference vs statement {c['wiring']:.1e}")
        assert c["wiring"] <= 1e-9 and c["out_gap"] <= max(1e-4, 3 * c["out_noise"]) and c["grad_gap"] <= max(1e-4, 3 * c["grad_noise"])


@needs_ref
def test_fixture_is_what_the_reference_gives(ref_report):
    """tests/golden/pna_baseline_ref.json regenerated by the child: integer inputs and shapes equal, float values within 1e-5 of the
    tensor's scale (a tolerance, not bit equality: the reference's fp32 CPU kernels sum in an order that follows the box)."""
    kept = load_fixture()
    with open(FIXTURE) as f:
        raw = json.load(f)
    assert os.path.getsize(FIXTURE) < 128 * 1024
    made = ref_report["configs"]
    assert [c["name"] for c in made] == [c["name"] for c in raw["configs"]] == [c["name"] for c in FIXTURE_CASES]
    for new, old_raw, old in zip(made, raw["configs"], kept):
        assert new["args"] == old_raw["args"] and new["feat"] == old_raw["feat"] and new["num_tasks"] == old_raw["num_tasks"]
        for part in ("inputs", "sd", "grads"):
            assert sorted(new[part]) == sorted(old_raw[part]), part
            for k, v in new[part].items():
                t = _tensor_from(v)
                if t.is_floating_point():
                    assert_close(t, old[part][k], atol=1e-5, rtol=1e-5, what=f"{new['name']} {part} {k}")
                else:
                    assert torch.equal(t, old[part][k]), (new["name"], part, k)
        assert len(new["logits"]) == len(old["logits"])
        for j, v in enumerate(new["logits"]):
            assert_close(_tensor_from(v), old["logits"][j], atol=1e-5, rtol=1e-5, what=f"{new['name']} logits {j}")


def test_fixture_agrees_with_the_statement():
    """(no reference needed) the recorded fp32 logits and gradients against the float64 statement at the recorded weights: 1e-4, or 3 x
    the reference's own recorded fp32-vs-float64 noise where larger (the bound the child holds the same pair to)"""
    cases = load_fixture()
    assert [c["name"] for c in cases] == [c["name"] for c in FIXTURE_CASES]
    for c in cases:
        b = fixture_batch(c["inputs"])
        out, _, grads = statement_run(c["sd"], c["args"], b, fixture_loss, torch.float64)
        outs = list(out) if isinstance(out, (list, tuple)) else [out]
        assert len(outs) == len(c["logits"])
        for j, (o, r) in enumerate(zip(outs, c["logits"])):
            tol = max(1e-4, 3 * c["out_noise"])
            assert_close(r, o.detach(), atol=tol, rtol=tol, what=f"{c['name']} logits {j}")
        assert set(grads) >= set(c["grads"])
        tol = max(1e-4, 3 * c["grad_noise"])
        assert tol <= 1e-3, tol   # (a record this noisy would pin nothing)
        for k, v in c["grads"].items():
            assert_close(v, grads[k], atol=tol, rtol=tol, what=f"{c['name']} grad {k}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the driver's read-out mode with the PNA stack and the head kinds, host only (gt_model_prepare asks sizes: no device call)
# ---------------------------------------------------------------------------------------------------------------------------------
def _driver_model(head_kind=2, readout=2, L=3, D=32, T_out=7, pos=3, h1=35, h2=17):
    """A gt_model as the plan fills it for a PNANet, by hand: test_gnn_baseline_host._driver_model's struct (made-up device addresses,
    never followed on the host) with a schematic PNA stack in place of the GCN layers and the head block re-laid behind the tower
    parameters.  The real one comes from model_layout.ModelLayout (step 1: offsets, shape) and engine.bind_storage (step 2: pointers);
    tests/test_model_layout_host.py compares shape and head block with this one."""
    from graphtrans_amd import layers
    fake = 0x10000
    Nh = T_out * pos if head_kind == 2 else T_out
    cm, keep = _gnn_driver_model(readout=readout, L=L, D=D, Nh=Nh, has_vn=False)
    cm.conv, cm.residual = 2, 1
    conv = (layers.PnaLayerDesc * L)()
    for l in range(L):
        conv[l].D, conv[l].T, conv[l].S, conv[l].agg_slots = D, 4, 4, 4
    cm.conv_layers = C.cast(conv, C.c_void_p)
    cm.pna_src, cm.pna_img, cm.pna_map, cm.pna_inv = fake * 20, fake * 21, fake * 22, fake * 23
    cm.pna_n_src = cm.pna_n_img = 4096
    cm.off_pna_src, off = cm.off_head_w, cm.off_head_w + 4096
    for k in ("off_hid_w", "off_hid_b", "off_hid2_w", "off_hid2_b"):
        setattr(cm, k, -1)
    c4 = lambda n: (n + 3) // 4 * 4
    cm.head_kind = head_kind
    first, hk = off, D
    if head_kind == 1:
        cm.head_h1, cm.head_h2 = h1, h2
        cm.hid_w, cm.hid_b, cm.hid2_w, cm.hid2_b = fake * 30, fake * 31, fake * 32, fake * 33
        cm.off_hid_w, off = off, off + c4(h1 * D)
        cm.off_hid2_w, off = off, off + c4(h2 * h1)
        cm.off_hid_b, off = off, off + c4(h1)
        cm.off_hid2_b, off = off, off + c4(h2)
        hk = h2
    elif head_kind == 2:
        cm.head_pos = pos
        cm.hid_w, cm.hid_b = fake * 30, fake * 31
        cm.off_hid_w, off = off, off + pos * D * D
        cm.off_hid_b, off = off, off + pos * D
    cm.off_head_w, off = off, off + c4(Nh * hk)
    cm.off_head_b, off = off, off + c4(Nh)
    cm.grad_total = off
    return cm, keep + [conv], first


def test_abi_sizes_match_the_mirrors():
    from graphtrans_amd import _lib, engine
    from graphtrans_amd.graph import StageRingDesc
    out = (C.c_int64 * 4)()
    _lib.check(_lib.lib().gt_model_abi_sizes(out), "gt_model_abi_sizes")
    assert tuple(out) == (C.sizeof(engine.ModelDesc), C.sizeof(engine.BatchDesc), C.sizeof(engine.ImageSet), C.sizeof(StageRingDesc))
    names = [f[0] for f in engine.ModelDesc._fields_]
    assert names[-4:] == ["readout", "pad_readout_", "pe", "pe_rows"]          # the head fields sit in front of the pinned tail
    assert names[-16:-4] == ["head_kind", "head_h1", "head_h2", "head_pos", "hid_w", "hid_b", "hid2_w", "hid2_b", "off_hid_w", "off_hid_b",
                             "off_hid2_w", "off_hid2_b"]
    assert engine.ModelDesc().head_kind == 0                                    # a zeroed struct has the linear heads of before


@pytest.mark.parametrize("readout", [1, 2, 3], ids=["sum", "mean", "max"])
def test_pna_readout_prepare_with_each_head_kind(readout):
    N, B, D = 287, 5, 32
    sizes_of = {}
    for kind in (0, 1, 2):
        cm, keep, _ = _driver_model(head_kind=kind, readout=readout, T_out=21 if kind != 2 else 7)   # (the same Nh = 21 for all three)
        bt, sizes = _driver_batch()
        assert (int(sizes.sum()), sizes.size) == (N, B)
        rc, sz, err = _prepare(cm, bt)   # (bt.ring is NULL: a staging-ring slot would have been an error)
        assert rc == 0, err
        assert sz.rows == 0 and sz.num_work == 0 and sz.max_npos == 0 and sz.exact == 1
        assert sz.arena_bytes >= 4 * (3 + 1) * N * D + 4 * B * D and sz.barena_bytes >= 4 * 3 * N * D
        sizes_of[kind] = (sz.arena_bytes, sz.barena_bytes)
    # the saved hidden activations: [B][35] + [B][17] for the MLP, [B][3 * D] for the position heads (256-byte slots)
    assert sizes_of[1][0] > sizes_of[0][0] and sizes_of[2][0] > sizes_of[0][0]
    assert sizes_of[2][1] > sizes_of[0][1]   # + d hidden [B][3 * D] and the dH partials


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_pna_readout_grad_ranges_start_at_the_first_head_float(kind):
    from graphtrans_amd import _lib
    cm, keep, first = _driver_model(head_kind=kind)
    lo, hi = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    _lib.check(_lib.lib().gt_model_grad_ranges(C.byref(cm), lo, hi), "gt_model_grad_ranges")
    r = list(zip(lo, hi))
    assert r[0] == (first, cm.grad_total)                                       # stage 1: the whole head block, hidden layers included
    assert first == (cm.off_head_w if kind == 0 else cm.off_hid_w)
    assert r[1] == (cm.off_conv[0], first) and r[2] == (0, cm.off_conv[0])      # message passing (towers included), the input encoder
    assert all(a < b for a, b in r) and r[2][0] == 0 and r[0][1] == cm.grad_total


def test_pna_readout_rejects_what_it_does_not_build():
    def bad(change, **kw):
        cm, keep, _ = _driver_model(**kw)
        bt, sizes = _driver_batch()
        change(cm, bt)
        rc, _, err = _prepare(cm, bt)
        assert rc == 0 or err
        return rc

    assert bad(lambda cm, b: None) == 0
    assert bad(lambda cm, b: setattr(cm, "residual", 0)) == INVALID            # the PNA conditions hold in this mode too
    assert bad(lambda cm, b: setattr(cm, "pna_src", None)) == INVALID
    assert bad(lambda cm, b: setattr(cm, "has_vn", 1)) == INVALID
    assert bad(lambda cm, b: setattr(cm, "readout", 0)) == INVALID             # the head kinds need the read-out mode
    assert bad(lambda cm, b: setattr(cm, "head_kind", 3)) == INVALID
    assert bad(lambda cm, b: setattr(cm, "hid_w", None)) == INVALID
    assert bad(lambda cm, b: setattr(cm, "head_pos", 17)) == INVALID
    assert bad(lambda cm, b: setattr(cm, "head_pos", 2)) == INVALID            # Nh = 21 does not split into 2 heads
    assert bad(lambda cm, b: None, D=24) == INVALID                            # position heads: D % 16
    assert bad(lambda cm, b: None, D=24, head_kind=1) == 0                     # ... the MLP takes any D % 4
    assert bad(lambda cm, b: setattr(cm, "head_h1", 65), head_kind=1) == INVALID
    assert bad(lambda cm, b: setattr(cm, "hid2_w", None), head_kind=1) == INVALID


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--ref-child":
        _child(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "--write-fixture":   # (re)record tests/golden/pna_baseline_ref.json from the reference
        _child(FIXTURE + ".tmp")
        with open(FIXTURE + ".tmp") as f:
            configs = json.load(f)["configs"]
        os.remove(FIXTURE + ".tmp")
        with open(FIXTURE, "w") as f:
            json.dump(dict(configs=configs), f)
        print(FIXTURE, os.path.getsize(FIXTURE), "bytes")
    else:
        sys.exit("usage: test_pna_baseline_host.py --ref-child OUT | --write-fixture")
