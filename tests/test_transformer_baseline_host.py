"""The plain Transformer baseline (graphtrans_amd/models/transformer.py, model_type "transformer") without a GPU: import and alias, the
third registry table and get_model_class, the constructor's contract, name() / get_emb_dim(), the state_dict keys, the new C entry
points in the header and in _lib.SIGNATURES, and -- where the reference tree is on the box -- the pin of the chain

    reference models/transformer.py (fp32, float64)  <->  `transformer_statement` below (float64, oracle/reference_math.py pieces)

in a child process that binds the reference the way oracle/make_golden.py does.  The same child records
tests/golden/transformer_baseline_ref.json (three tiny configurations run by the reference itself: inputs, weights, logits, parameter
gradients and the gradient of `perturb`), which tests/test_hip_transformer_baseline.py loads on the GPU box.

`transformer_statement`, `statement_run`, `load_fixture` and `fixture_batch` are imported by the GPU tests: the statement is written
once, here.
"""
import base64
import copy
import json
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import assert_close

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
FIXTURE = os.path.join(REPO, "tests", "golden", "transformer_baseline_ref.json")
needs_ref = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "models", "transformer.py")), reason="the reference tree is not on this box")
SIZES = (5, 1, 9, 3)   # at max_input_len 7 the 9-node graph drops its two leading nodes


def _args(**kw):
    a = dict(d_model=16, nhead=2, dim_feedforward=32, transformer_dropout=0.0, transformer_activation="relu", num_encoder_layers=2,
             max_input_len=7, transformer_norm_input=False, graph_pooling="cls", max_seq_len=None, model_type="transformer",
             gnn_type="gcn", gnn_virtual_node=False)
    a.update(kw)
    return SimpleNamespace(**a)


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 statement of models/transformer.py:86-115
# ---------------------------------------------------------------------------------------------------------------------------------
def transformer_statement(sd, args, data, perturb=None, training=True):
    """Transformer.forward: node encoder -> + perturb -> pad_batch -> TransformerNodeEncoder -> out[-1] (cls) | unpad_batch over the
    UN-transformed rows -> global_add / mean / max_pool -> head(s), from oracle/reference_math.py pieces, in the dtype of `sd`."""
    from oracle import reference_math as rm

    node_depth = data.node_depth if hasattr(data, "node_depth") else None
    encoded = rm.node_encode(sd, "node_encoder", data.x, node_depth)
    tmp = encoded + perturb if perturb is not None else encoded
    padded, mask, _, S = rm.pad_batch(tmp, data.batch, args.max_input_len)
    out, _ = rm.transformer_node_encoder(sd, "transformer", args, padded, mask, training)
    if args.graph_pooling == "cls":
        hg = out[-1]
    else:
        h = rm.unpad_batch(out, tmp, data.batch, S)
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
    """-> (outputs, loss, {parameter key: gradient}[, d perturb]) of `transformer_statement` at `state_dict` in `dtype`"""
    sd = {k: (v.detach().cpu().to(dtype).requires_grad_(True) if v.is_floating_point() else v.detach().cpu().clone()) for k, v in state_dict.items()}
    oargs = SimpleNamespace(**{k: v for k, v in vars(args).items() if k not in ("compute_dtype", "token_layout", "fused_embed")})
    bb = copy.copy(b)
    if bb.x.is_floating_point():
        bb.x = bb.x.to(dtype)
    pt = None if perturb is None else perturb.detach().cpu().to(dtype).requires_grad_(True)
    torch.set_default_dtype(dtype)   # the oracle's helpers allocate zeros / ones in the default dtype
    try:
        out = transformer_statement(sd, oargs, bb, pt, True)
        loss = loss_of(out)
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    grads = {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.requires_grad and v.grad is not None}
    return (out, loss.detach(), grads) if pt is None else (out, loss.detach(), grads, pt.grad)


def weighted(ws):
    """loss(out) = sum_i (out_i * w_i).sum() for one output or a list of them"""
    return lambda out: sum((o * w.to(device=o.device, dtype=o.dtype)).sum() for o, w in zip(out if isinstance(out, (list, tuple)) else [out], ws))


def fixture_loss(out):
    outs = out if isinstance(out, (list, tuple)) else [out]
    return sum(o.square().mean() for o in outs) / len(outs)


# ---------------------------------------------------------------------------------------------------------------------------------
# import, registry, constructor, names, state_dict, C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def _node_encoder(feat, D):
    from graphtrans_amd.encoders import ASTNodeEncoder, AtomEncoder
    if feat == "code2":
        return ASTNodeEncoder(D, 11, 13, 20)
    if feat == "mol":
        return AtomEncoder(D)
    return torch.nn.Linear(6, D)   # dataset/tud.py:65


def _build(args, feat="code2", num_tasks=5):
    from graphtrans_amd.models.transformer import Transformer
    return Transformer(num_tasks, _node_encoder(feat, args.d_model), None, args)


def test_import_and_alias():
    import graphtrans_amd.models.transformer as mod
    from models.transformer import Transformer as aliased
    assert aliased is mod.Transformer
    import models
    assert models.transformer is mod and models.get_model_class is not None and models.BASELINE_MODELS["transformer"] is mod.Transformer


def test_registry_tables():
    import argparse

    from graphtrans_amd.models import ABLATION_MODELS, BASELINE_MODELS, MODELS, get_model_and_parser, get_model_class
    from graphtrans_amd.models.gnn import GNN
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    from graphtrans_amd.models.pna import PNANet
    from graphtrans_amd.models.pna_transformer import PNATransformer
    from graphtrans_amd.models.transformer import Transformer
    assert BASELINE_MODELS == {"transformer": Transformer}
    want = {"gnn": GNN, "gnn-transformer": GNNTransformer, "pna-transformer": PNATransformer, "pna": PNANet, "transformer": Transformer}
    for name, cls in want.items():
        assert get_model_class(name) is cls, name
    for bad in ("transformer-gnn", "", "Transformer"):
        with pytest.raises(KeyError):
            get_model_class(bad)
    # the two pinned tables and the reference's entry point are as they were
    assert MODELS == {"gnn": GNN, "gnn-transformer": GNNTransformer, "pna-transformer": PNATransformer}
    assert ABLATION_MODELS == {"pna": PNANet}
    with pytest.raises(KeyError):
        get_model_and_parser(SimpleNamespace(model_type="transformer"), argparse.ArgumentParser())
    # add_args is the encoder's group, as in the reference
    parser = argparse.ArgumentParser()
    get_model_class("transformer").add_args(parser)
    ns = parser.parse_args([])
    assert ns.d_model == 128 and ns.num_encoder_layers == 4 and ns.max_input_len == 1000 and not ns.transformer_norm_input


def test_constructor_contract():
    for pooling in ("cls", "sum", "mean", "max"):
        m = _build(_args(graph_pooling=pooling))
        assert m.graph_pooling == pooling and (m.transformer.cls_embedding is not None) == (pooling == "cls")
    for pooling in ("attention", "set2set"):
        with pytest.raises(NotImplementedError, match=pooling):
            _build(_args(graph_pooling=pooling))
    for pooling in ("last", "median", ""):
        with pytest.raises(ValueError, match="Invalid graph pooling type."):
            _build(_args(graph_pooling=pooling))
    m = _build(_args(max_seq_len=3))
    assert len(m.graph_pred_linear_list) == 3 and not hasattr(m, "graph_pred_linear")
    assert hasattr(_build(_args()), "graph_pred_linear")
    # forward's argument checks come before anything touches the device
    from graphtrans_amd.data import Batch
    m = _build(_args())
    empty = Batch(x=torch.zeros((0, 2), dtype=torch.int64), edge_index=torch.zeros((2, 0), dtype=torch.int64), edge_attr=None,
                  batch=torch.zeros(0, dtype=torch.int64), node_depth=torch.zeros((0, 1), dtype=torch.int64))
    with pytest.raises(ValueError, match="empty batch"):
        m(empty)
    from graphtrans_amd import synth
    b = synth.tiny_mixed(seed=1, sizes=SIZES, feat="code2")
    with pytest.raises(ValueError, match="one row per node"):
        m(b, torch.zeros(sum(SIZES) - 1, 16))
    assert m.fused_embed in (True, False) and _build(_args(fused_embed=True)).fused_embed and not _build(_args(fused_embed=False)).fused_embed


def test_name_and_emb_dim_are_the_reference_strings():
    from graphtrans_amd.models.transformer import Transformer
    assert Transformer.get_emb_dim(_args(d_model=48)) == 48
    assert Transformer.name(_args()) == "transformer-pooling=cls+gcn-d=16-tdp=0.0"
    assert Transformer.name(_args(graph_pooling="mean", gnn_type="gin", gnn_virtual_node=True, d_model=256, transformer_dropout=0.3)) == \
        "transformer-pooling=mean+gin-virtual-d=256-tdp=0.3"
    assert Transformer.need_deg() is False


def test_new_symbols_in_the_header_and_the_binding():
    from graphtrans_amd import _lib
    L = _lib.lib()
    with open(os.path.join(REPO, "include", "graphtrans_hip.h")) as f:
        header = f.read()
    for name, nargs in (("gt_embed_tokens_fwd", 12), ("gt_embed_tokens_bwd_workspace_bytes", 3), ("gt_embed_tokens_bwd", 13)):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        assert m.group(1).count(",") + 1 == nargs == len(_lib.SIGNATURES[name][1]), name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    # rejected on the host, before anything is launched (no device here): bad dim, 17 tables
    assert L.gt_embed_tokens_fwd(1, None, None, None, None, None, None, 4, 6, _lib.GT_F32, None, None) == -2   # GT_ERR_UNSUPPORTED
    assert b"gt_embed_tokens_fwd" in L.gt_last_error()
    assert L.gt_embed_tokens_bwd(17, None, _lib.GT_F32, None, None, 4, 8, None, None, None, None, 0, None) == -2
    assert b"gt_embed_tokens_bwd" in L.gt_last_error()
    assert L.gt_embed_tokens_bwd_workspace_bytes(3, 100, 16) == L.gt_embed_sum_bwd_sorted_workspace_bytes(3, 100, 16)


def test_encoders_hand_out_their_columns():
    from graphtrans_amd.encoders import ASTNodeEncoder, AtomEncoder
    ast, atom = ASTNodeEncoder(8, 11, 13, 20), AtomEncoder(8)
    x, depth = torch.zeros((4, 2), dtype=torch.int64), torch.zeros((4, 1), dtype=torch.int64)
    cols, tabs, clamps = ast.embed_columns(x, depth.view(-1))
    assert [c.shape for c in cols] == [(4,)] * 3 and cols[0].stride(0) == 2 and clamps == [None, None, 20]
    assert [t is w for t, w in zip(tabs, (ast.type_encoder.weight, ast.attribute_encoder.weight, ast.depth_encoder.weight))] == [True] * 3
    cols, tabs, clamps = atom.embed_columns(torch.zeros((4, 9), dtype=torch.int64))
    assert len(cols) == len(tabs) == 9 and clamps is None and tabs[3] is atom.atom_embedding_list[3].weight


# ---------------------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------------------
FIXTURE_CASES = [dict(name="code2-cls-heads3", feat="code2", graph_pooling="cls", max_seq_len=3),
                 dict(name="atom-mean", feat="mol", graph_pooling="mean", max_seq_len=None),
                 dict(name="linear-max", feat="tud", graph_pooling="max", max_seq_len=None)]


def _tensor_json(t):
    """integers as lists; floats as the base64 of their little-endian bytes (bit exact, a quarter of the decimal text)"""
    t = t.detach().cpu().contiguous()
    d = dict(dtype=str(t.dtype).replace("torch.", ""), shape=list(t.shape))
    if t.is_floating_point():
        d["b64"] = base64.b64encode(t.numpy().astype("<f4" if t.dtype == torch.float32 else "<f8").tobytes()).decode("ascii")
    else:
        d["data"] = t.reshape(-1).tolist()
    return d


def _tensor_from(d):
    dt = getattr(torch, d["dtype"])
    if "b64" in d:
        a = np.frombuffer(base64.b64decode(d["b64"]), dtype="<f4" if dt == torch.float32 else "<f8").copy()
        return torch.from_numpy(a).to(dt).reshape(d["shape"])
    return torch.tensor(d["data"], dtype=dt).reshape(d["shape"])


def load_fixture(path=FIXTURE):
    """-> [dict(name, feat, args (SimpleNamespace), inputs (with `perturb`), sd, logits (list), grads, perturb_grad)] with tensors"""
    with open(path) as f:
        raw = json.load(f)
    out = []
    for c in raw["configs"]:
        out.append(dict(name=c["name"], feat=c["feat"], args=SimpleNamespace(**c["args"]), keys=list(c["sd"]),
                        inputs={k: _tensor_from(v) for k, v in c["inputs"].items()}, sd={k: _tensor_from(v) for k, v in c["sd"].items()},
                        logits=[_tensor_from(v) for v in c["logits"]], grads={k: _tensor_from(v) for k, v in c["grads"].items()},
                        perturb_grad=_tensor_from(c["perturb_grad"])))
    return out


def fixture_batch(inputs):
    from graphtrans_amd.data import Batch
    d = {k: inputs[k] for k in ("x", "edge_index", "edge_attr", "batch", "node_depth") if k in inputs}
    d.setdefault("edge_attr", None)
    return Batch(_sizes=np.asarray(SIZES, dtype=np.int64), **d)


def test_state_dict_keys_on_meta_equal_the_recorded_list():
    """keys, their order and shapes as the reference's own state_dict has them (recorded in the fixture)"""
    for c in load_fixture():
        with torch.device("meta"):
            model = _build(c["args"], c["feat"])
        got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        assert got == [(k, tuple(c["sd"][k].shape)) for k in c["keys"]], c["name"]
        top = {k.split(".")[0] for k, _ in got}
        assert top == {"node_encoder", "transformer", "graph_pred_linear" if c["args"].max_seq_len is None else "graph_pred_linear_list"}


def test_fixture_agrees_with_the_statement():
    """(no reference needed) the recorded fp32 logits and gradients against the float64 statement at the recorded weights: 1e-4"""
    assert os.path.getsize(FIXTURE) < 256 * 1024
    cases = load_fixture()
    assert [c["name"] for c in cases] == [c["name"] for c in FIXTURE_CASES]
    for c in cases:
        a = c["args"]
        assert (a.d_model, a.nhead, a.dim_feedforward, a.num_encoder_layers, a.transformer_dropout, a.max_input_len) == (16, 2, 32, 2, 0.0, 7)
        b = fixture_batch(c["inputs"])
        assert torch.bincount(b.batch).tolist() == list(SIZES)
        out, _, grads, dp = statement_run(c["sd"], a, b, fixture_loss, torch.float64, perturb=c["inputs"]["perturb"])
        outs = out if isinstance(out, (list, tuple)) else [out]
        assert len(outs) == len(c["logits"]) == (a.max_seq_len or 1)
        for i, (o, r) in enumerate(zip(outs, c["logits"])):
            assert_close(r, o.detach(), what=f"{c['name']} logits {i}")
        assert set(grads) >= set(c["grads"])
        for k, v in c["grads"].items():
            assert_close(v, grads[k], what=f"{c['name']} grad {k}")
        assert_close(c["perturb_grad"], dp, what=c["name"] + " perturb grad")
        if a.graph_pooling == "cls":   # the dropped nodes never reach the output ...
            assert (c["perturb_grad"][6:8] == 0).all()
        else:                          # ... but keep their input rows in front of the pooling (unpad_batch's base)
            assert (c["perturb_grad"][6:8] != 0).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference itself, in a child process (the parent's `models` / `modules` are this repository's alias packages)
# ---------------------------------------------------------------------------------------------------------------------------------
REF_CASES = [(pool, feat, msl) for pool in ("cls", "sum", "mean", "max") for feat, msl in (("code2", 3), ("mol", None), ("tud", None))]


def _child(out_path):
    """Runs with the REFERENCE's `models` / `modules` bound (oracle/make_golden.py's binding, loaded as a module): every comparison of
    the pin, the measured gaps and the fixture's content into `out_path` (JSON)."""
    import importlib.util
    import inspect

    torch.set_num_threads(1)
    spec = importlib.util.spec_from_file_location("mg", os.path.join(REPO, "oracle", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    from models.transformer import Transformer as RefTransformer
    assert os.path.realpath(inspect.getsourcefile(RefTransformer)).startswith(REF + os.sep)
    from graphtrans_amd import synth

    def run_ref(model, b, loss_of, dtype, perturb):
        m = copy.deepcopy(model).to(dtype).train()
        bb = copy.copy(b)
        if bb.x.is_floating_point():
            bb.x = bb.x.to(dtype)
        if hasattr(bb, "node_depth"):
            bb.node_depth = bb.node_depth.clone()   # the reference's ASTNodeEncoder clamps its input in place
        pt = perturb.detach().to(dtype).requires_grad_(True)
        out = m(bb, pt)
        loss_of(out).backward()
        outs = list(out) if isinstance(out, (list, tuple)) else [out]
        return [o.detach() for o in outs], {k: p.grad.detach() for k, p in m.named_parameters() if p.grad is not None}, pt.grad.detach()

    report = dict(cases=[], configs=[])
    for i, (pool, feat, msl) in enumerate(REF_CASES):
        args = _args(graph_pooling=pool, max_seq_len=msl)
        torch.manual_seed(0)
        b = synth.tiny_mixed(seed=40 + i, sizes=SIZES, feat=feat)
        ref = RefTransformer(5, mg.make_node_encoder(feat, 16), None, args)
        mg.randomize(ref, 60 + i)
        with torch.device("meta"):
            mine = _build(args, feat)
        assert [(k, tuple(v.shape)) for k, v in ref.state_dict().items()] == [(k, tuple(v.shape)) for k, v in mine.state_dict().items()], (pool, feat)
        g = torch.Generator().manual_seed(1234)
        ws = [torch.randn(len(SIZES), 5, generator=g) for _ in range(msl or 1)]
        perturb = torch.randn(sum(SIZES), 16, generator=g) * 0.1
        loss_of = weighted(ws)
        o32, g32, p32 = run_ref(ref, b, loss_of, torch.float32, perturb)
        o64, g64, p64 = run_ref(ref, b, loss_of, torch.float64, perturb)
        so, _, sg, sp = statement_run(ref.state_dict(), args, b, loss_of, torch.float64, perturb=perturb)
        so = list(so) if isinstance(so, (list, tuple)) else [so]
        case = dict(case=f"{pool},{feat},max_seq_len={msl}", out_gap=0.0, grad_gap=0.0, out_noise=0.0, grad_noise=0.0, wiring=0.0)

        def cmp(kind, key, a32, a64, st):
            # the bar of tests/test_gnn_baseline_host.py: 1e-9 in float64 (the same math: the wiring); the fp32 reference within 1e-4, or
            # 3 x the reference's OWN fp32-vs-float64 noise on that tensor where larger
            noise = float((a32.double() - a64).abs().max()) / max(1.0, float(a64.abs().max()))
            tol = max(1e-4, 3 * noise)
            gap = float((a32.double() - st).abs().max()) / max(1.0, float(st.abs().max()))
            case[kind + "_gap"], case[kind + "_noise"] = max(case[kind + "_gap"], gap), max(case[kind + "_noise"], noise)
            case["wiring"] = max(case["wiring"], float((a64 - st).abs().max()) / max(1.0, float(st.abs().max())))
            assert_close(a64, st, atol=1e-9, rtol=1e-9, what=f"{case['case']} float64 {kind} {key}")
            assert_close(a32, st, atol=tol, rtol=tol, what=f"{case['case']} fp32 {kind} {key}")
        for j, (a, c, s) in enumerate(zip(o32, o64, so)):
            cmp("out", str(j), a, c, s.detach())
        assert set(g32) == set(g64)
        for k in g64:
            cmp("grad", k, g32[k], g64[k], sg[k] if k in sg else torch.zeros_like(g64[k]))
        cmp("grad", "perturb", p32, p64, sp)
        report["cases"].append(case)
    # ---- the fixture: three configurations run by the reference in fp32
    for c in FIXTURE_CASES:
        args = _args(graph_pooling=c["graph_pooling"], max_seq_len=c["max_seq_len"])
        torch.manual_seed(0)
        b = synth.tiny_mixed(seed=77, sizes=SIZES, feat=c["feat"])
        ref = RefTransformer(5, mg.make_node_encoder(c["feat"], 16), None, args)
        mg.randomize(ref, 91)
        with torch.no_grad():   # logits of O(1): the randomised weights are large
            for p in ref.parameters():
                if p.dim() > 1 and p.shape[0] > 1:
                    p.mul_(0.5)
        inputs = {k: v.clone() for k, v in mg.batch_inputs(b).items()}
        inputs["perturb"] = torch.randn(sum(SIZES), 16, generator=torch.Generator().manual_seed(5)) * 0.1
        o32, g32, p32 = run_ref(ref, b, fixture_loss, torch.float32, inputs["perturb"])
        report["configs"].append(dict(name=c["name"], feat=c["feat"], args=vars(args), inputs={k: _tensor_json(v) for k, v in inputs.items()},
                                      sd={k: _tensor_json(v) for k, v in ref.state_dict().items()}, logits=[_tensor_json(o) for o in o32],
                                      grads={k: _tensor_json(v) for k, v in g32.items()}, perturb_grad=_tensor_json(p32)))
    with open(out_path, "w") as f:
        json.dump(report, f)


@pytest.fixture(scope="module")
def ref_report(tmp_path_factory):
    out = tmp_path_factory.mktemp("transformer_ref") / "report.json"
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--ref-child", str(out)], cwd=REPO, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    with open(out) as f:
        return json.load(f)


@needs_ref
def test_reference_transformer_equals_the_float64_statement(ref_report):
    """Every (pooling, encoder kind) case, one graph truncated and a perturbation present: same keys, order and shapes as this
    repository's Transformer, the float64 reference equal to the statement at 1e-9 (same math), the fp32 reference within
    max(1e-4, 3 x its own fp32-vs-float64 noise) of it (asserted in the child, tensor by tensor; the figures are printed here)."""
    cases = ref_report["cases"]
    assert len(cases) == len(REF_CASES) == 12
    for c in cases:
        print(f"[{c['case']}] fp32 reference vs float64 statement: logits {c['out_gap']:.2e} (reference's own noise {c['out_noise']:.2e}), "
              f"gradients {c['grad_gap']:.2e} ({c['grad_noise']:.2e}); float64 reference vs statement {c['wiring']:.1e}")
        assert c["wiring"] <= 1e-9 and c["out_gap"] <= max(1e-4, 3 * c["out_noise"]) and c["grad_gap"] <= max(1e-4, 3 * c["grad_noise"])


@needs_ref
def test_fixture_is_what_the_reference_gives(ref_report):
    """tests/golden/transformer_baseline_ref.json regenerated by the child: integer inputs, shapes and key order equal, float values
    within 1e-5 of the tensor's scale -- a tolerance, not bit equality: the reference runs fp32 torch CPU kernels whose summation order
    follows the thread count and the BLAS build of the box."""
    kept = load_fixture()
    with open(FIXTURE) as f:
        raw = json.load(f)
    made = ref_report["configs"]
    assert [c["name"] for c in made] == [c["name"] for c in raw["configs"]] == [c["name"] for c in FIXTURE_CASES]
    for new, old_raw, old in zip(made, raw["configs"], kept):
        assert new["args"] == old_raw["args"] and new["feat"] == old_raw["feat"]
        assert list(new["sd"]) == list(old_raw["sd"])
        for part in ("inputs", "sd", "grads"):
            assert sorted(new[part]) == sorted(old_raw[part]), part
            for k, v in new[part].items():
                t = _tensor_from(v)
                if t.is_floating_point():
                    assert_close(t, old[part][k], atol=1e-5, rtol=1e-5, what=f"{new['name']} {part} {k}")
                else:
                    assert torch.equal(t, old[part][k]), (new["name"], part, k)
        assert len(new["logits"]) == len(old["logits"])
        for i, v in enumerate(new["logits"]):
            assert_close(_tensor_from(v), old["logits"][i], atol=1e-5, rtol=1e-5, what=f"{new['name']} logits {i}")
        assert_close(_tensor_from(new["perturb_grad"]), old["perturb_grad"], atol=1e-5, rtol=1e-5, what=new["name"] + " perturb grad")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--ref-child":
        _child(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "--write-fixture":   # (re)record tests/golden/transformer_baseline_ref.json from the reference
        _child(FIXTURE + ".tmp")
        with open(FIXTURE + ".tmp") as f:
            configs = json.load(f)["configs"]
        os.remove(FIXTURE + ".tmp")
        with open(FIXTURE, "w") as f:
            json.dump(dict(configs=configs), f)
        print(FIXTURE, os.path.getsize(FIXTURE), "bytes")
    else:
        sys.exit("usage: test_transformer_baseline_host.py --ref-child OUT.json | --write-fixture")
