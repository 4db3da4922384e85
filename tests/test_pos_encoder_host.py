"""PositionalEncoding on the packed token layout, host side (no GPU): the padded position of every node
(graph.SeqLayout.positions -- what csrc/segment.hip:k_seq_positions computes on the device) against the oracle's
pad_batch + positional_encoding, and the driver's struct mirrors after gt_model gained `pe` / `pe_rows`."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

SIZES = (9, 1, 17, 6)


def _layout(max_input_len, with_cls=True, kind="packed"):
    from graphtrans_amd.graph import SeqLayout
    gs = SimpleNamespace(sizes=np.asarray(SIZES, dtype=np.int64), B=len(SIZES), device="cpu")
    return SeqLayout(gs, kind, max_input_len, with_cls)


@pytest.mark.parametrize("kind", ["packed", "padded"])
def test_positions_index_the_rows_pad_batch_and_positional_encoding_produce(kind):
    from graphtrans_amd.models.gnn_transformer import PositionalEncoding
    from oracle import reference_math as rm
    d = 16
    torch.manual_seed(0)
    batch = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
    h = torch.randn(sum(SIZES), d)
    padded, mask, _, S = rm.pad_batch(h, batch, 1000)
    rows = rm.positional_encoding(padded)   # (S, B, d)
    pos = _layout(1000, kind=kind).positions()
    assert pos.dtype == np.int32 and pos.shape == (sum(SIZES),) and S == 17
    assert (pos >= 0).all()                 # nothing truncated
    pe = PositionalEncoding(d, dropout=0).pe[:, 0]
    p = torch.from_numpy(pos.astype(np.int64))
    assert torch.equal(rows[p, batch], h + pe[p])
    # every valid (position, graph) cell is hit exactly once
    hit = torch.zeros(S, len(SIZES), dtype=torch.int64)
    hit.index_put_((p, batch), torch.ones_like(p), accumulate=True)
    assert torch.equal(hit == 1, ~mask.t())


@pytest.mark.parametrize("with_cls", [True, False])
def test_positions_under_truncation_follow_the_left_padding_formula(with_cls):
    """max_input_len = 8: S = 8, the graphs of 9 and 17 nodes keep their LAST 8; node row graph_ptr[b+1] - kept_b + j sits at
    padded position S - kept_b + j, the dropped leading nodes get -1.  (Not through oracle.positional_encoding: it sizes its
    table from the truncated S and could not expose an offset error.)"""
    max_len = 8
    n = np.asarray(SIZES)
    S = min(int(n.max()), max_len)
    gptr = np.concatenate([[0], np.cumsum(n)])
    want = np.full(int(n.sum()), -1, np.int64)
    for b in range(len(n)):
        kept = min(int(n[b]), S)
        for j in range(kept):
            want[gptr[b + 1] - kept + j] = S - kept + j
    pos = _layout(max_len, with_cls).positions()
    assert np.array_equal(pos.astype(np.int64), want)
    assert (pos[:1] == -1).all() and (pos[10:19] == -1).all() and int((pos == -1).sum()) == 1 + 9   # sizes 9 and 17 truncate
    assert pos.max() == S - 1 and pos[8] == 7 and pos[9] == 7                                     # last node of a graph: S - 1


def test_model_struct_mirrors_match_the_library():
    """gt_model ends with {pe, pe_rows}, gt_model_batch with {lay_S, lay_meta}: the ctypes mirrors and the library agree
    (engine._check_abi, as test_cabi_exports does), and the new entry points are exported."""
    import ctypes as C
    from graphtrans_amd import _lib, engine
    engine._ABI_OK.clear()
    engine._check_abi()
    names = [f[0] for f in engine.ModelDesc._fields_]
    assert names[-2:] == ["pe", "pe_rows"]
    out = (C.c_int64 * 4)()
    assert _lib.lib().gt_model_abi_sizes(out) == 0
    assert out[0] == C.sizeof(engine.ModelDesc) and out[1] == C.sizeof(engine.BatchDesc)
    for fn in ("gt_seq_positions", "gt_seq_gather_add", "gt_linear_set_rows_add"):
        assert fn in _lib.SIGNATURES and hasattr(_lib.lib(), fn)


def test_packed_with_pos_encoder_contract_edges():
    """token_layout="packed" + pos_encoder is accepted; "auto" keeps the padded layout; what the kernels cannot read raises."""
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    from oracle.reference_math import default_args

    def model(**kw):
        a = default_args(gnn_emb_dim=16, d_model=16, nhead=2, dim_feedforward=32, num_encoder_layers=1, gnn_num_layer=2,
                         graph_pooling="last", max_seq_len=None, pos_encoder=True, **kw)
        return GNNTransformer(3, torch.nn.Linear(6, 16), lambda d: torch.nn.Linear(2, d), a)

    assert model(token_layout="packed")._use_packed() is True
    assert model(token_layout="auto")._use_packed() is False
    assert model(token_layout="padded")._use_packed() is False
    m = model(token_layout="packed")
    m.pos_encoder.dropout.p = 0.1
    with pytest.raises(ValueError, match="dropout"):
        m._use_packed()
    with pytest.raises(ValueError, match="max_input_len"):
        model(token_layout="packed", max_input_len=5001)._use_packed()
    m = model(token_layout="packed")
    m.pos_encoder.pe = m.pos_encoder.pe.double()
    with pytest.raises(ValueError, match="fp32"):
        m._use_packed()
    a = default_args(gnn_emb_dim=16, d_model=16, nhead=2, dim_feedforward=32, num_encoder_layers=1, gnn_num_layer=2,
                     graph_pooling="mean", max_seq_len=None, pos_encoder=True, token_layout="packed")
    with pytest.raises(ValueError, match="mean pooling"):
        GNNTransformer(3, torch.nn.Linear(6, 16), lambda d: torch.nn.Linear(2, d), a)._use_packed()
