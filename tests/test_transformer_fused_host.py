"""The Transformer baseline's fused step on the host (no GPU): the model's opt-in attributes, the struct mirrors against the library's
sizes, the encoder-only mode's gradient ranges and its checks in gt_model_prepare (host code: sizes and refusals, no device call).  (No
export was added: tests/test_cabi_exports.py keeps comparing the header's symbols with the binding's.)
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

INVALID = -1   # GT_ERR_INVALID_ARG


def _targs(**kw):
    a = dict(d_model=64, nhead=4, dim_feedforward=128, transformer_dropout=0.0, transformer_activation="relu", num_encoder_layers=2,
             max_input_len=20, transformer_norm_input=False, graph_pooling="cls", max_seq_len=None, model_type="transformer",
             gnn_type="gcn", gnn_virtual_node=False)
    a.update(kw)
    return SimpleNamespace(**a)


def test_fused_step_and_fused_flag_come_from_args_and_default_to_off():
    from graphtrans_amd.models.transformer import Transformer
    m = Transformer(2, torch.nn.Linear(37, 64), None, _targs())
    assert m.fused_step is False and m.fused_flag is False
    m = Transformer(2, torch.nn.Linear(37, 64), None, _targs(fused_step=1, fused_flag="yes"))
    assert m.fused_step is True and m.fused_flag is True
    m = Transformer(2, torch.nn.Linear(37, 64), None, _targs(fused_step=True))
    assert m.fused_step is True and m.fused_flag is False


def test_model_parts_answers_for_every_family():
    """engine.model_parts is the one place that knows where a model keeps its stack, its token encoder and its input encoder"""
    from graphtrans_amd import engine
    from graphtrans_amd.models.transformer import Transformer
    ne = torch.nn.Linear(37, 64)
    m = Transformer(2, ne, None, _targs())
    gnn, enc, inp = engine.model_parts(m)
    assert gnn is None and enc is m.transformer and inp is ne
    assert engine.emb_dim(m) == 64 and engine.frozen_pattern(m) == "none"
    ne.bias.requires_grad_(False)
    assert engine.frozen_pattern(m) == "other"   # no message passing: never "gnn"


def test_a_cpu_model_is_not_eligible_and_off_never_asks():
    from graphtrans_amd import engine
    from graphtrans_amd.models.transformer import Transformer
    m = Transformer(2, torch.nn.Linear(37, 64), None, _targs())
    b = SimpleNamespace(x=torch.zeros(3, 37), batch=torch.zeros(3, dtype=torch.int64))
    assert not engine.eligible(m, b, None)          # fused_step off
    m.fused_step = True
    assert not engine.eligible(m, b, None)          # parameters on the CPU
    assert not engine._eligible_static_enc_only(Transformer(2, torch.nn.Linear(37, 64), None, _targs(graph_pooling="mean")))


def test_abi_sizes_still_match_the_mirrors():
    from graphtrans_amd import _lib, engine
    from graphtrans_amd.graph import StageRingDesc
    out = (C.c_int64 * 4)()
    _lib.check(_lib.lib().gt_model_abi_sizes(out), "gt_model_abi_sizes")
    assert tuple(out) == (C.sizeof(engine.ModelDesc), C.sizeof(engine.BatchDesc), C.sizeof(engine.ImageSet), C.sizeof(StageRingDesc))
    cm = engine.ModelDesc()
    assert cm.enc_only == 0 and cm.readout == 0     # a zeroed struct is the token path
    cm.enc_only = 1                                 # the mode flag IS the word beside `readout`
    assert cm.pad_readout_ == 1 and engine.ModelDesc.pad_readout_.offset == engine.ModelDesc.readout.offset + 4


def _enc_only_model(embed_kind=0, d=64, Nh=6, n_enc=2, tables=(11, 13)):
    """A gt_model as the plan fills it for the Transformer baseline, by hand; device pointers are made-up addresses (never followed on
    the host).  Gradient layout: input encoder, cls, encoder layers, final norm, heads.  The real one comes from
    model_layout.ModelLayout (step 1: offsets, shape) and engine.bind_storage (step 2: pointers); tests/test_model_layout_host.py holds
    it against this one field by field."""
    from graphtrans_amd import engine, layers
    fake = 0x10000
    cm = engine.ModelDesc()
    cm.enc_only = 1
    cm.L, cm.n_enc, cm.with_cls, cm.embed_kind = 0, n_enc, 1, embed_kind
    cm.D, cm.d, cm.Nh, cm.ldy, cm.max_input_len = d, d, Nh, (Nh + 3) // 4 * 4, 20
    enc = (layers.EncoderLayerDesc * n_enc)()
    for i in range(n_enc):
        enc[i].d_model, enc[i].ffn, enc[i].nhead = d, 2 * d, 4
    cm.enc = C.cast(enc, C.c_void_p)
    off = 0
    cm.off_ne_w = cm.off_ne_b = -1
    if embed_kind == 1:
        cm.ne_K, cm.ne_w, cm.ne_b = 37, fake * 20, fake * 21
        cm.off_ne_w, cm.off_ne_b = 0, (d * 37 + 3) // 4 * 4
        off = cm.off_ne_b + d
    else:
        cm.n_tables, cm.embed_sorted = len(tables), 1
        for t, rows in enumerate(tables):
            cm.tables[t], cm.table_rows[t], cm.table_clamp[t] = fake * (t + 1), rows, -1
            cm.off_tables[t] = off
            off += rows * d
    for k in ("off_vn_emb", "off_g2t_w", "off_g2t_b", "off_nin_w", "off_nin_b", "off_hid_w", "off_hid_b", "off_hid2_w", "off_hid2_b"):
        setattr(cm, k, -1)
    cm.off_cls, cm.cls = off, fake * 30
    off += d
    per_enc = 3 * d * d + 3 * d + d * d + d + 2 * (2 * d * d) + 2 * d + d + 4 * d
    for i in range(n_enc):
        cm.off_enc[i] = off
        off += per_enc
    cm.off_nout_w, cm.off_nout_b, cm.nout_w, cm.nout_b = off, off + d, fake * 31, fake * 32
    off += 2 * d
    cm.off_head_w, cm.head_w = off, fake * 33
    off += (Nh * d + 3) // 4 * 4
    cm.off_head_b, cm.head_b = off, fake * 34
    off += (Nh + 3) // 4 * 4
    cm.grad_total = off
    return cm, [enc]


def _batch(sizes=(5, 70, 9, 1, 30), linear=False):
    from graphtrans_amd import engine
    sizes = np.ascontiguousarray(sizes, np.int64)
    bt = engine.BatchDesc()
    bt.N, bt.E, bt.B = int(sizes.sum()), 0, sizes.size
    bt.batch, bt.sizes_host = 0x30000, sizes.ctypes.data
    bt.x, bt.x_stride0, bt.x_stride1 = 0x40000, (37 if linear else 2), 1
    bt.training, bt.compute, bt.tdt, bt.will_bwd = 1, 0, 0, 1
    return bt, sizes


def _prepare(cm, bt, ring=True):
    from graphtrans_amd import _lib, engine
    from graphtrans_amd.graph import StageRingDesc
    L = _lib.lib()
    ctx = C.create_string_buffer(int(L.gt_model_ctx_bytes()))
    sz = engine.SizesDesc()
    keep = None
    if ring:   # a host-built layout is staged into a slot of the caller's ring: plain host memory stands in for the pinned slots
        keep = C.create_string_buffer(1 << 16)
        rd = StageRingDesc()
        rd.base, rd.slot_bytes, rd.slots, rd.next = C.addressof(keep), 1 << 16, 1, 0
        bt.ring = C.addressof(rd)
        keep = (keep, rd)
    rc = L.gt_model_prepare(C.byref(cm), C.byref(bt), ctx, C.byref(sz))
    err = L.gt_last_error()
    return rc, sz, (err.decode() if isinstance(err, bytes) else str(err))


def test_grad_ranges_tile_the_buffer_with_an_empty_middle():
    from graphtrans_amd import _lib
    for kind in (0, 1):
        cm, keep = _enc_only_model(embed_kind=kind)
        lo, hi = (C.c_int64 * 3)(), (C.c_int64 * 3)()
        assert _lib.lib().gt_model_grad_ranges(C.byref(cm), lo, hi) == 0, _lib.lib().gt_last_error()
        tail, total = int(cm.off_cls), int(cm.grad_total)
        assert 0 < tail < total
        assert list(zip(lo, hi)) == [(tail, total), (tail, tail), (0, tail)]
        assert all(l <= h for l, h in zip(lo, hi)) and sorted(zip(lo, hi))[0][0] == 0 and max(hi) == total


@pytest.mark.parametrize("kind", [0, 1], ids=["tables", "linear"])
def test_prepare_sizes_the_token_layout_and_no_node_matrices(kind):
    """the mode takes the token path's layout (packed, with CLS) and asks for no [N][D] fp32 node-row matrices"""
    cm, keep = _enc_only_model(embed_kind=kind)
    bt, sizes = _batch(linear=kind == 1)
    rc, sz, err = _prepare(cm, bt)
    assert rc == 0, err
    kept = np.minimum(sizes, 20)
    assert sz.rows == int(kept.sum()) + sizes.size and sz.max_npos == 21 and sz.exact == 1
    d, rows = 64, sz.rows
    assert sz.arena_bytes >= 4 * rows * d and sz.barena_bytes >= 2 * 4 * rows * d


def test_prepare_refuses_what_the_mode_does_not_cover():
    cases = {}
    cm, k0 = _enc_only_model()
    cm.enc_only = 0
    cases["L == 0 without the mode flag"] = (cm, _batch()[0])
    cm, k1 = _enc_only_model()
    cm.readout = 2
    cases["readout"] = (cm, _batch()[0])
    cm, k2 = _enc_only_model()
    bt = _batch()[0]
    bt.gnn_frozen = 1
    cases["gnn_frozen"] = (cm, bt)
    cm, k3 = _enc_only_model(embed_kind=1)
    bt = _batch(linear=True)[0]
    bt.perturb = 0x70000
    cases["perturb with the Linear encoder"] = (cm, bt)
    cm, k4 = _enc_only_model()
    cm.with_cls = 0
    cases["no CLS"] = (cm, _batch()[0])
    cm, k5 = _enc_only_model()
    cm.n_enc = 0
    cases["no encoder layer"] = (cm, _batch()[0])
    cm, k6 = _enc_only_model()
    cm.embed_sorted = 0
    cases["a table beyond the sorted backward"] = (cm, _batch()[0])
    for what, (cm, bt) in cases.items():
        rc, _, err = _prepare(cm, bt)
        assert rc == INVALID and err, (what, rc, err)
