"""What the engine's plan derives from a model's module tree alone, on a fixed grid of models, into one JSON file:
python tools/plan_layout_dump.py OUT.json

For every model of `laid_out_grid()` (every one of them eligible): the named_parameters name and the flat-buffer offset of every
entry of `plan.params`, `plan.total`, `plan.ranges`, the names in `plan.gnn_plist` and `plan.tlist`, every non-pointer field of
`plan.cm` and of the descriptor arrays, and `engine._eligible_static(model)`.  For every model of `eligibility_grid()`:
`_eligible_static` alone.  Names, integers and a few float hyper-parameters only -- tests/golden/plan_layouts.json is this tool's
output, and tests/test_model_layout_host.py holds graphtrans_amd.model_layout against it on the CPU.

The tool reads nothing but the plan's public attributes, so it runs unchanged against any revision of the package.  The grids build
their models on whatever device they are given: the dump needs the GPU (the plan binds device resources), the host test does not."""
import ctypes as C
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

_PTR = (C.c_void_p, C.c_char_p)


def struct_fields(s):
    """{field: value} of every non-pointer field of a ctypes struct (arrays as lists; pointer arrays and nested structs left out)"""
    out = {}
    for name, ctype in s._fields_:
        if ctype in _PTR or issubclass(ctype, C.Structure):
            continue
        v = getattr(s, name)
        if issubclass(ctype, C.Array):
            if ctype._type_ in _PTR:
                continue
            v = [list(r) if isinstance(r, C.Array) else r for r in v]
        out[name] = v
    return out


def _gt_args(**kw):   # (the defaults of tests/test_hip_engine.py::_args)
    a = dict(gnn_virtual_node=True, gnn_num_layer=3, gnn_emb_dim=64, gnn_JK="cat", gnn_dropout=0.0, gnn_residual=False,
             gnn_type="gcn", pretrained_gnn=None, freeze_gnn=None, d_model=32, nhead=4, dim_feedforward=64,
             transformer_dropout=0.2, transformer_activation="relu", num_encoder_layers=2, max_input_len=1000,
             transformer_norm_input=True, graph_pooling="cls", num_encoder_layers_masked=0, transformer_prenorm=False,
             pos_encoder=False, max_seq_len=3, compute_dtype=torch.float32, token_layout="auto")
    a.update(kw)
    return SimpleNamespace(**a)


def _lin_edge(d):
    return torch.nn.Linear(2, d)


def _zero_edge(d):
    return lambda _e: 0


def gt(node="ast", edge=_lin_edge, tasks=50, after=None, **kw):
    """GNNTransformer builder; after: applied to the built model (freezes parameters, swaps a submodule)"""
    def build(dev):
        from graphtrans_amd.encoders import ASTNodeEncoder, AtomEncoder
        from graphtrans_amd.models.gnn_transformer import GNNTransformer
        args = _gt_args(**kw)
        D = args.gnn_emb_dim
        ne = {"ast": lambda: ASTNodeEncoder(D, 98, 300, 20), "atom": lambda: AtomEncoder(D)}.get(node, node)()
        model = GNNTransformer(tasks, ne, edge, args).to(dev)
        if after is not None:
            after(model)
        return model
    return build


def _bond_edge(d):
    from graphtrans_amd.encoders import BondEncoder
    return BondEncoder(d)


def _pna_args(**kw):   # (tools/driver_dump.py's `pna`)
    a = dict(gnn_virtual_node=False, gnn_num_layer=3, gnn_emb_dim=64, gnn_JK="last", gnn_residual=True, gnn_dropout=0.25, gnn_type="gcn",
             pretrained_gnn=None, freeze_gnn=None, d_model=64, nhead=4, dim_feedforward=128, transformer_dropout=0.1,
             transformer_activation="relu", num_encoder_layers=2, max_input_len=1000, transformer_norm_input=True, graph_pooling="cls",
             num_encoder_layers_masked=0, transformer_prenorm=False, pos_encoder=False, max_seq_len=3,
             aggregators=["mean", "max", "min", "std"], scalers=["identity", "amplification", "attenuation"],
             deg=torch.tensor([0, 40, 25, 9, 3]))
    a.update(kw)
    return SimpleNamespace(**a)


def pnat(after=None, **kw):
    def build(dev):
        from graphtrans_amd.encoders import ASTNodeEncoder
        from graphtrans_amd.models.pna_transformer import PNATransformer
        args = _pna_args(**kw)
        model = PNATransformer(50, ASTNodeEncoder(args.gnn_emb_dim, 98, 10030, 20), None, args).to(dev)
        if after is not None:
            after(model)
        return model
    return build


def pnanet(node="ast", **kw):
    def build(dev):
        from graphtrans_amd.encoders import ASTNodeEncoder
        from graphtrans_amd.models.pna import PNANet
        a = dict(gnn_num_layer=2, gnn_emb_dim=32, gnn_dropout=0.0, gnn_residual=True, graph_pooling="mean", max_seq_len=None, model_type="pna",
                 aggregators=["mean", "max", "min", "std"], scalers=["identity", "amplification", "attenuation"],
                 deg=torch.tensor([0, 40, 25, 9, 3]))
        a.update(kw)
        D = a["gnn_emb_dim"]
        ne = ASTNodeEncoder(D, 11, 13, 20) if node == "ast" else node()
        return PNANet(7, ne, None, SimpleNamespace(**a)).to(dev)
    return build


def gnn(node="ast", edge=_lin_edge, **kw):
    def build(dev):
        from graphtrans_amd.encoders import ASTNodeEncoder
        from graphtrans_amd.models.gnn import GNN
        a = dict(gnn_virtual_node=True, gnn_num_layer=3, gnn_emb_dim=64, gnn_JK="last", gnn_dropout=0.1, gnn_residual=False, gnn_type="gcn",
                 graph_pooling="mean", max_seq_len=3, model_type="gnn")
        a.update(kw)
        ne = ASTNodeEncoder(a["gnn_emb_dim"], 98, 300, 20) if node == "ast" else node()
        return GNN(50, ne, edge, SimpleNamespace(**a)).to(dev)
    return build


def tr(node="ast", **kw):
    def build(dev):
        from graphtrans_amd.encoders import ASTNodeEncoder
        from graphtrans_amd.models.transformer import Transformer
        a = dict(d_model=64, nhead=4, dim_feedforward=128, transformer_dropout=0.1, transformer_activation="relu", num_encoder_layers=2,
                 max_input_len=100, transformer_norm_input=False, graph_pooling="cls", max_seq_len=3, model_type="transformer",
                 gnn_type="gcn", gnn_virtual_node=False, fused_step=True)
        a.update(kw)
        ne = ASTNodeEncoder(a["d_model"], 98, 300, 20) if node == "ast" else node()
        return Transformer(50, ne, None, SimpleNamespace(**a)).to(dev)
    return build


def _freeze_gnn(model):
    model.gnn_node.requires_grad_(False)


def _freeze_conv0(model):
    model.gnn_node.convs[0].requires_grad_(False)


def laid_out_grid():
    """name -> build(device) -> model; every model eligible, the whole plan recorded"""
    return {
        "gt:default": gt(),
        "gt:last,plain,one-head,pool-last": gt(gnn_JK="last", gnn_virtual_node=False, max_seq_len=None, graph_pooling="last",
                                              transformer_norm_input=False),
        "gt:gin,tables,virtual": gt(node="atom", edge=_bond_edge, tasks=16, gnn_type="gin", max_seq_len=None),
        "gt:linear37,zero-edge": gt(node=lambda: torch.nn.Linear(37, 64), edge=_zero_edge, tasks=2, max_seq_len=None,
                                    gnn_virtual_node=False, gnn_JK="last"),
        "gt:pos_encoder,packed": gt(pos_encoder=True, token_layout="packed"),
        "gt:frozen": gt(fused_freeze=True, after=_freeze_gnn),
        "pnat:driver_dump": pnat(),
        "pnat:sum,var": pnat(gnn_num_layer=2, aggregators=["mean", "sum", "var"], scalers=["identity", "amplification"]),
        "gnn:gcn,virtual,mean,3-heads": gnn(),
        "gnn:gin,plain,max,one-head": gnn(gnn_type="gin", gnn_virtual_node=False, graph_pooling="max", max_seq_len=None),
        "pnanet:mlp": pnanet(),
        "pnanet:positions,D=64": pnanet(max_seq_len=3, gnn_emb_dim=64),
        "tr:ast": tr(),
        "tr:linear37": tr(node=lambda: torch.nn.Linear(37, 64)),
    }


def eligibility_grid():
    """name -> (build(device) -> model, the static check the variant is aimed at); only `_eligible_static` is recorded"""
    class OtherEdge(torch.nn.Module):   # an edge encoder that is a module but no Linear
        def __init__(self, d):
            super().__init__()
            self.weight, self.bias = torch.nn.Parameter(torch.zeros(d, 2)), torch.nn.Parameter(torch.zeros(d))

    def nobias_edge(d):
        return torch.nn.Linear(2, d, bias=False)

    return {
        # ---- token path, GCN / GIN
        "gt:pool-mean": (gt(graph_pooling="mean"), "_use_packed(): mean pooling runs on the padded layout"),
        "gt:padded": (gt(token_layout="padded"), "_use_packed(): the padded layout was asked for"),
        "gt:pos_encoder,auto": (gt(pos_encoder=True), "_use_packed(): a positional encoding keeps the padded layout unless packed is asked for"),
        "gt:masked-layer": (gt(num_encoder_layers_masked=1), "_use_packed(): a masked encoder layer"),
        "gt:D=66": (gt(gnn_emb_dim=66), "D % 4"),
        "gt:JK=sum": (gt(gnn_JK="sum"), "JK not in (last, cat)"),
        "gt:edge-5-cols": (gt(edge=lambda d: torch.nn.Linear(5, d)), "an edge Linear with more than 4 input columns"),
        "gt:edge-no-bias": (gt(edge=nobias_edge), "an edge Linear without a bias"),
        "gt:edge-other-module": (gt(edge=OtherEdge), "an edge encoder module that is no Linear"),
        "gt:edge-nonzero-callable": (gt(edge=lambda d: (lambda _e: 1)), "a callable edge encoder that does not return 0"),
        "gt:17-gnn-layers": (gt(gnn_num_layer=17), "more GNN layers than GT_MODEL_MAX_LAYERS"),
        "gt:17-encoder-layers": (gt(num_encoder_layers=17), "more encoder layers than GT_MODEL_MAX_LAYERS"),
        "gt:d_model=36": (gt(d_model=36), "_encoder_ok: d_model % 8"),
        "gt:ffn=60": (gt(dim_feedforward=60), "_encoder_ok: the FFN width % 8"),
        "gt:g2t-K%4": (gt(gnn_emb_dim=64, gnn_JK="last", after=lambda m: setattr(m, "gnn2transformer", torch.nn.Linear(62, 32).to(
            m.gnn2transformer.weight.device))), "gnn2transformer's input width % 4"),
        "gt:node-linear-no-bias": (gt(node=lambda: torch.nn.Linear(37, 64, bias=False), edge=_zero_edge, max_seq_len=None),
                                   "_eligible_static_rest: a Linear input encoder without a bias"),
        "gt:node-other": (gt(node=lambda: torch.nn.Embedding(98, 64)), "_eligible_static_rest: an input encoder that is neither kind of tables nor a Linear"),
        "gt:gnn-frozen,no-fused_freeze": (gt(after=_freeze_gnn), "_frozen_ok: gnn_node frozen without fused_freeze"),
        "gt:one-conv-frozen,fused_freeze": (gt(fused_freeze=True, after=_freeze_conv0), "_frozen_ok: the pattern is not exactly gnn_node"),
        "gt:head-frozen": (gt(after=lambda m: m.graph_pred_linear_list[0].requires_grad_(False)), "_frozen_ok: a frozen head"),
        "gt:gelu": (gt(transformer_activation="gelu"), "(eligible) the GELU encoder"),
        "gt:residual,last": (gt(gnn_residual=True, gnn_JK="last"), "(eligible) residual GNN, JK last"),
        "gt:gin,linear-edge": (gt(gnn_type="gin"), "(eligible) GIN with Linear edges"),
        "gt:tables-too-many-rows": (gt(node="atom", edge=_bond_edge, tasks=16, gnn_type="gin", max_seq_len=None, gnn_emb_dim=1024, d_model=32),
                                    "tables_fit_lds: a layer's edge tables beyond the LDS budget at D = 1024"),
        # ---- PNATransformer
        "pnat:F%4": (pnat(gnn_emb_dim=40, d_model=32, nhead=4, dim_feedforward=64), "_pna_convs_ok: F = D / towers = 10, F % 4"),
        "pnat:no-residual": (pnat(gnn_residual=False), "_pna_convs_ok: PNANodeEmbedding without the residual connection"),
        "pnat:pool-mean": (pnat(graph_pooling="mean"), "_eligible_static_pna: mean pooling"),
        "pnat:frozen,fused_freeze": (pnat(fused_freeze=True, after=_freeze_gnn), "(eligible) exactly gnn_node frozen with fused_freeze"),
        "pnat:ffn=60": (pnat(dim_feedforward=60), "_encoder_ok under the PNA stack"),
        # ---- read-out mode
        "gnn:sum,gin,virtual": (gnn(gnn_type="gin", graph_pooling="sum"), "(eligible) GIN with a virtual node, sum pooling"),
        "gnn:JK=cat": (_gnn_jk_cat(), "read-out with JK cat (set after the constructor, which refuses it)"),
        "gnn:D=66": (gnn(gnn_emb_dim=66), "D % 4 in the read-out mode"),
        "gnn:17-layers": (gnn(gnn_num_layer=17), "more GNN layers than GT_MODEL_MAX_LAYERS in the read-out mode"),
        "gnn:gnn-frozen": (_frozen(gnn(), _freeze_gnn), "_frozen_ok: no frozen pattern in the read-out mode"),
        "pnanet:positions,D=40": (pnanet(max_seq_len=3, gnn_emb_dim=40), "head kind 2 with D % 16"),
        "pnanet:mlp,D=40": (pnanet(gnn_emb_dim=40), "_pna_convs_ok: F = 10 under head kind 1"),
        "pnanet:sum,var": (pnanet(aggregators=["mean", "sum", "var"], scalers=["identity"], graph_pooling="max"), "(eligible) six aggregate slots"),
        "pnanet:17-positions": (pnanet(max_seq_len=17, gnn_emb_dim=64), "head kind 2 with more than 16 positions"),
        # ---- encoder-only mode
        "tr:pool-mean": (tr(graph_pooling="mean"), "_eligible_static_enc_only: pooling other than cls"),
        "tr:linear-width": (_tr_wrong_width(), "_eligible_static_enc_only: a Linear encoder whose width is not d_model"),
        "tr:17-layers": (tr(num_encoder_layers=17), "_eligible_static_enc_only: more encoder layers than GT_MODEL_MAX_LAYERS"),
        "tr:big-table": (tr(node=lambda: _ast(64, 98, 20000)), "_eligible_static_enc_only: a table beyond EMBED_SORT_MAX_ROWS"),
        "tr:head-frozen": (_frozen(tr(), lambda m: m.graph_pred_linear_list[0].requires_grad_(False)), "_eligible_static_enc_only: any frozen parameter"),
        "tr:d_model=36": (tr(d_model=36, nhead=2), "_encoder_ok in the encoder-only mode"),
        "tr:no-fused_step": (tr(fused_step=False), "(eligible statically: fused_step is a per-call check)"),
    }


def _ast(D, types, attrs):
    from graphtrans_amd.encoders import ASTNodeEncoder
    return ASTNodeEncoder(D, types, attrs, 20)


def _frozen(build, freeze):
    def b(dev):
        model = build(dev)
        freeze(model)
        return model
    return b


def _gnn_jk_cat():
    def b(dev):
        model = gnn()(dev)
        model.gnn_node.JK = "cat"
        return model
    return b


def _tr_wrong_width():
    def b(dev):
        model = tr(node=lambda: torch.nn.Linear(37, 64))(dev)
        model.node_encoder = torch.nn.Linear(37, 48).to(dev)
        return model
    return b


def record(model, plan):
    names = {id(p): n for n, p in model.named_parameters()}
    r = dict(params=[[names[id(p)], int(o)] for p, o in plan.params], total=int(plan.total), ranges=[[int(a), int(b)] for a, b in plan.ranges],
             gnn_plist=[names[id(p)] for p in plan.gnn_plist], tlist=[names[id(p)] for p in plan.tlist], cm=struct_fields(plan.cm))
    conv = plan.conv_desc
    r["conv_desc"] = [struct_fields(conv[l]) for l in range(plan.L)] if conv is not None else []
    r["vn_desc"] = [struct_fields(plan.vn_desc[l]) for l in range(plan.L - 1)] if plan.has_vn else []
    r["enc_desc"] = [struct_fields(plan.enc_desc[i]) for i in range(int(plan.cm.n_enc))]
    return r


def main(out_path):
    from graphtrans_amd import engine
    dev = "cuda:0"
    res = dict(laid_out={}, eligibility={})
    for name, build in laid_out_grid().items():
        torch.manual_seed(0)
        model = build(dev)
        ok = bool(engine._eligible_static(model))
        assert ok, name + ": a laid-out model must be eligible"
        r = record(model, engine._plan(model))
        r["eligible_static"] = ok
        res["laid_out"][name] = r
        print(name, "total", r["total"], "ranges", r["ranges"], flush=True)
    for name, (build, aim) in eligibility_grid().items():
        torch.manual_seed(0)
        ok = bool(engine._eligible_static(build(dev)))
        res["eligibility"][name] = dict(eligible_static=ok, aim=aim)
        print(name, ok, "|", aim, flush=True)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
    n = sum(1 for v in res["eligibility"].values() if v["eligible_static"])
    print("wrote", out_path, os.path.getsize(out_path), "bytes;", len(res["laid_out"]), "laid out;", n, "of", len(res["eligibility"]), "variants eligible")


if __name__ == "__main__":
    main(sys.argv[1])
