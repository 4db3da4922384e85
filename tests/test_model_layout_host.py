"""graphtrans_amd/model_layout.py without a GPU: the gradient layout of every model family, built from the real model classes on the
CPU, against

  * tests/golden/plan_layouts.json -- what engine._Plan gave for the same models on the device at the commit before the layout was
    split from the binding (tools/plan_layout_dump.py; the grids are that tool's);
  * itself (every parameter once, disjoint intervals, stacked groups consecutive);
  * the storage step (engine.bind_storage) on the CPU model: pointers, contiguous groups, an unchanged state_dict;
  * the three hand-built struct mirrors of the host tests (an independent statement of the same layout);
  * the C side on the host: gt_model_grad_ranges and gt_model_prepare over the real struct.
"""
import ctypes as C
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import plan_layout_dump as grid   # noqa: E402

with open(os.path.join(REPO, "tests", "golden", "plan_layouts.json")) as f:
    GOLD = json.load(f)
LAID_OUT = grid.laid_out_grid()
VARIANTS = grid.eligibility_grid()
# set by the binding from the import-time switches (GT_VN_DEFER_DW, DW_OVERLAP_MIN_ELEMS), not by the layout
BINDING_FIELDS = ("vn_defer_dw", "dw_overlap_min_elems")


def _build(name):
    torch.manual_seed(0)
    return LAID_OUT[name]("cpu")


def _layout(model):
    from graphtrans_amd import engine
    from graphtrans_amd.model_layout import ModelLayout
    lay = ModelLayout(model)
    cm = engine.ModelDesc()
    lay.fill(cm)
    return lay, cm


def test_the_grids_are_the_recorded_ones():
    assert sorted(LAID_OUT) == sorted(GOLD["laid_out"]) and sorted(VARIANTS) == sorted(GOLD["eligibility"])
    answers = [v["eligible_static"] for v in GOLD["eligibility"].values()]
    assert len(answers) >= 20 and True in answers and False in answers and all(v["eligible_static"] for v in GOLD["laid_out"].values())
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "plan_layouts.json")) < 200 * 1024


@pytest.mark.parametrize("name", sorted(LAID_OUT))
def test_layout_reproduces_the_recording(name):
    gold = GOLD["laid_out"][name]
    model = _build(name)
    before = {k: (v.data_ptr(), v.clone()) for k, v in model.state_dict().items()}
    lay, cm = _layout(model)
    names = {id(p): n for n, p in model.named_parameters()}
    assert [[names[id(p)], o] for p, o in lay.params] == gold["params"]
    assert lay.total == gold["total"]
    got = grid.struct_fields(cm)
    assert {k: v for k, v in got.items() if k not in BINDING_FIELDS} == {k: v for k, v in gold["cm"].items() if k not in BINDING_FIELDS}
    assert [grid.struct_fields(lay.conv_desc[l]) for l in range(lay.L)] == gold["conv_desc"] if lay.conv_desc is not None else gold["conv_desc"] == []
    assert [grid.struct_fields(lay.vn_desc[l]) for l in range(lay.L - 1 if lay.has_vn else 0)] == gold["vn_desc"]
    assert [grid.struct_fields(lay.enc_desc[i]) for i in range(len(lay.enc_layers))] == gold["enc_desc"]
    # the layout leaves the model alone: same storage, same values
    for k, v in model.state_dict().items():
        assert v.data_ptr() == before[k][0] and torch.equal(v, before[k][1]), k
    # ---- flat-buffer integrity
    assert sorted(names[id(p)] for p, _ in lay.params) == sorted(names.values())          # every parameter exactly once
    spans = sorted((o, o + p.numel()) for p, o in lay.params)
    assert spans[0][0] >= 0 and spans[-1][1] <= lay.total
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))                             # disjoint
    off = {id(p): o for p, o in lay.params}
    order = [id(p) for p, _ in lay.params]
    groups = list(lay.storage_groups)
    if lay.kind != "pna" and lay.conv_desc is not None and lay.conv_desc[0].edge_mode == 2:
        # the edge tables of ALL layers are one storage, but each layer's tables lie in that layer's gradient block: a run per layer
        tabs, n = groups.pop(0), int(lay.conv_desc[0].edge_cols)
        groups += [tabs[i:i + n] for i in range(0, len(tabs), n)]
    for group in groups:                                                                   # a stacked group: consecutive, in order
        for a, b in zip(group, group[1:]):
            assert off[id(b)] == off[id(a)] + a.numel() and order.index(id(b)) == order.index(id(a)) + 1


@pytest.mark.parametrize("name", sorted(LAID_OUT) + sorted(VARIANTS))
def test_structural_predicate_equals_the_recorded_answer(name):
    from graphtrans_amd.model_layout import structural_ok
    torch.manual_seed(0)
    if name in LAID_OUT:
        model, want = LAID_OUT[name]("cpu"), GOLD["laid_out"][name]["eligible_static"]
    else:
        model, want = VARIANTS[name][0]("cpu"), GOLD["eligibility"][name]["eligible_static"]
    try:
        got = bool(structural_ok(model))
    except Exception:   # (engine._eligible_static holds the one `try`: a model the helpers cannot read is not eligible)
        got = False
    assert got == want, VARIANTS.get(name, (None, "a laid-out model"))[1]


@pytest.mark.parametrize("name", sorted(LAID_OUT))
def test_storage_step_on_the_cpu_model(name):
    from graphtrans_amd import engine
    from graphtrans_amd.model_layout import ModelLayout
    model = _build(name)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    lay = ModelLayout(model)
    cm = engine.ModelDesc()
    engine.bind_storage(lay, cm)
    for desc, field, t in lay.ptrs:
        assert getattr(cm if desc is None else desc, field) == t.data_ptr(), field
    for t, w in enumerate(lay.embed):
        assert cm.tables[t] == w.data_ptr()
    for group in lay.storage_groups:   # one contiguous storage: member i starts where member i - 1 ends
        at = group[0].data_ptr()
        for p in group:
            assert p.data_ptr() == at and p.is_contiguous()
            at += 4 * p.numel()
    if len(lay.heads) > 1:   # e.g. head i's weight starts i * rows * d floats behind head_w
        rows = lay.heads[0].weight.shape[0]
        for i, h in enumerate(lay.heads):
            assert h.weight.data_ptr() == cm.head_w + 4 * i * rows * h.weight.shape[1] and h.bias.data_ptr() == cm.head_b + 4 * i * rows
    after = model.state_dict()
    assert list(after) == list(before)
    for k, v in after.items():
        assert torch.equal(v, before[k]), k


# ---- the hand-built mirrors of the host tests ---------------------------------------------------------------------------------------
def _diff(cm, mirror):
    a, b = grid.struct_fields(cm), grid.struct_fields(mirror)
    return {k for k in a if a[k] != b[k]}


def test_gnn_mirror_equals_the_layout():
    from test_gnn_baseline_host import _driver_model
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn import GNN
    for has_vn in (True, False):
        a = SimpleNamespace(gnn_virtual_node=has_vn, gnn_num_layer=3, gnn_emb_dim=32, gnn_JK="last", gnn_dropout=0.0, gnn_residual=False,
                            gnn_type="gcn", graph_pooling="mean", max_seq_len=3, model_type="gnn")
        lay, cm = _layout(GNN(5, ASTNodeEncoder(32, 11, 13, 20), lambda d: torch.nn.Linear(2, d), a))
        mirror, keep = _driver_model(readout=2, L=3, D=32, Nh=15, has_vn=has_vn)
        # off_hid*: the mirror leaves the four offsets of a head block it does not have at 0, the layout writes -1 (absent)
        assert _diff(cm, mirror) == {"off_hid_w", "off_hid_b", "off_hid2_w", "off_hid2_b"}
        for l in range(3):
            assert (lay.conv_desc[l].D, lay.conv_desc[l].edge_mode, lay.conv_desc[l].edge_cols) == (32, 1, 2)


def test_pna_mirror_equals_the_layout_in_shape_and_head_block():
    from test_pna_baseline_host import _args, _build, _driver_model
    for kind, msl in ((1, None), (2, 3)):
        lay, cm = _layout(_build(_args(gnn_num_layer=3, gnn_emb_dim=32, max_seq_len=msl, scalers=["identity", "amplification", "attenuation", "linear"]),
                                  num_tasks=7))   # (four scalers: the mirror's S = 4 output blocks)
        mirror, keep, first = _driver_model(head_kind=kind, readout=2, L=3, D=32, T_out=7, pos=3)
        # the mirror's stack is schematic -- GCN-sized layer blocks, 4096 made-up tower floats, no image offsets, kinds or degree
        # averages --, so every offset behind the input encoder differs by a constant; the head block is compared relative to its start
        schematic = {"off_conv", "off_pna_src", "pna_n_src", "pna_n_img", "pna_img_off", "pna_kinds", "pna_avg_log", "pna_avg_lin",
                     "off_hid_w", "off_hid_b", "off_hid2_w", "off_hid2_b", "off_head_w", "off_head_b", "grad_total"}
        assert _diff(cm, mirror) <= schematic
        start = int(cm.off_hid_w)
        for k in ("off_hid_w", "off_hid_b", "off_head_w", "off_head_b", "grad_total") + (("off_hid2_w", "off_hid2_b") if kind == 1 else ()):
            assert getattr(cm, k) - start == getattr(mirror, k) - first, k
        if kind == 2:
            assert cm.off_hid2_w == mirror.off_hid2_w == -1 and cm.off_hid2_b == mirror.off_hid2_b == -1
        assert cm.off_pna_src + cm.pna_n_src == start   # the head block lies right behind the tower parameters
        assert all((lay.conv_desc[l].D, lay.conv_desc[l].T, lay.conv_desc[l].S, lay.conv_desc[l].agg_slots) == (32, 4, 4, 4) for l in range(3))


class _Tables(torch.nn.Module):   # an AtomEncoder-style input encoder with the mirror's table sizes
    def __init__(self, d, rows):
        super().__init__()
        self.atom_embedding_list = torch.nn.ModuleList([torch.nn.Embedding(r, d) for r in rows])


def test_enc_only_mirror_equals_the_layout():
    from test_transformer_fused_host import _enc_only_model
    from graphtrans_amd.models.transformer import Transformer
    a = SimpleNamespace(d_model=64, nhead=4, dim_feedforward=128, transformer_dropout=0.0, transformer_activation="relu", num_encoder_layers=2,
                        max_input_len=20, transformer_norm_input=False, graph_pooling="cls", max_seq_len=None, model_type="transformer",
                        gnn_type="gcn", gnn_virtual_node=False, fused_step=True)
    for kind, ne in ((0, _Tables(64, (11, 13))), (1, torch.nn.Linear(37, 64))):
        lay, cm = _layout(Transformer(6, ne, None, a))
        mirror, keep = _enc_only_model(embed_kind=kind, d=64, Nh=6, n_enc=2)
        # nout_eps: the mirror leaves the final norm's eps at 0 (no kernel runs on the host), the layout carries the module's 1e-5
        assert _diff(cm, mirror) == {"nout_eps"}
        for i in range(2):
            assert (lay.enc_desc[i].d_model, lay.enc_desc[i].ffn, lay.enc_desc[i].nhead) == (64, 128, 4)


# ---- the C side on the host, over the real struct -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LAID_OUT))
def test_c_side_takes_the_bound_struct(name):
    from test_transformer_fused_host import _prepare
    from test_gnn_baseline_host import _driver_batch
    from graphtrans_amd import _lib, engine
    from graphtrans_amd.model_layout import ModelLayout, model_parts
    model = _build(name)
    lay = ModelLayout(model)
    cm = engine.ModelDesc()
    engine.bind_storage(lay, cm)
    cm.zero_i64 = 0x10000   # (made-up device addresses, never followed on the host, for what the device step of the plan allocates)
    if lay.kind == "pna":
        cm.pna_img, cm.pna_map, cm.pna_inv = 0x20000, 0x30000, 0x40000
    lo, hi = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    _lib.check(_lib.lib().gt_model_grad_ranges(C.byref(cm), lo, hi), "gt_model_grad_ranges")
    r = list(zip(lo, hi))
    # three ranges that tile [0, total); range 0 starts where the header says it does for the family
    assert r[2][0] == 0 and r[2][1] == r[1][0] and r[1][1] == r[0][0] and r[0][1] == lay.total
    start = cm.off_cls if lay.enc_only else ((cm.off_hid_w if lay.head_kind else cm.off_head_w) if lay.readout else cm.off_g2t_w)
    assert r[0][0] == start
    # what lies below range 0 is exactly gnn_node (the input encoder in the encoder-only mode): engine's `tail_outside_gnn`
    gnn, _, ne = model_parts(model)
    assert {id(p) for p, o in lay.params if o < start} == {id(p) for p in (gnn if gnn is not None else ne).parameters()}
    bt, sizes = _driver_batch()
    if lay.enc_only:
        bt.E, bt.edge_index, bt.edge_attr = 0, None, None
    if lay.embed_kind == "linear":
        bt.x_stride0, bt.node_depth = lay.ne_K, None
    rc, sz, err = _prepare(cm, bt, ring=not lay.readout)
    assert rc == 0, err


# ---- the PNA gather map against the module's own map --------------------------------------------------------------------------------
@pytest.mark.parametrize("aggs,scalers", [(["mean", "max", "min", "std"], ["identity", "amplification", "attenuation"]),
                                          (["mean", "sum", "var"], ["identity"])], ids=["classic,3-scalers", "sum-var,identity"])
def test_pna_gather_map_equals_the_modules_post_maps(aggs, scalers):
    """model_layout.pna_maps and PNAConv._post_maps state the same re-stacking of the post nets: per layer and tower, the map's
    post-net block with its source base subtracted IS the module's map, the module's "appended zero" index standing where the engine's
    map says -1; the same for the bias; and the inverse map is a bijection from the source onto the used image entries."""
    import numpy as np
    from graphtrans_amd.model_layout import pna_maps
    from graphtrans_amd.modules.pna.pna_module import PNAConv
    T, F, L = 4, 16, 2
    conv = PNAConv(T * F, T * F, aggregators=aggs, scalers=scalers, deg=torch.tensor([0, 40, 25, 9, 3]), towers=T, divide_input=True)
    S, K = len(conv._blocks), conv.agg_slots
    assert K == (6 if "sum" in aggs else 4)
    mp, inv, img_off = pna_maps(L, T, F, aggs, conv._blocks, scalers, K)
    wmap, bmap = (m.numpy() for m in conv._post_maps("cpu"))
    cols = (len(aggs) * len(scalers) + 1) * F
    KF, per_layer = (1 + K) * F, T * F * 2 * F + T * F + T * F * cols + T * F
    assert wmap.shape == (S * F * KF,) and bmap.shape == (S * F,)
    for l in range(L):
        s_post_w = l * per_layer + T * F * 2 * F + T * F
        s_post_b = s_post_w + T * F * cols
        for t in range(T):
            blk = mp[img_off[l][2] + t * S * F * KF:img_off[l][2] + (t + 1) * S * F * KF]
            assert np.array_equal(np.where(blk >= 0, blk - (s_post_w + t * F * cols), F * cols), wmap), (l, t)
            bias = mp[img_off[l][3] + t * S * F:img_off[l][3] + (t + 1) * S * F]
            assert np.array_equal(np.where(bias >= 0, bias - (s_post_b + t * F), F), bmap), (l, t)
    used = np.nonzero(mp >= 0)[0]
    assert inv.shape == (L * per_layer,) and np.array_equal(np.sort(inv), used) and np.array_equal(mp[inv], np.arange(L * per_layer))
