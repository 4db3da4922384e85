"""`GraphStore` for float-feature datasets (TU: x (N,37) f32, no edge features; ER: x (N,256) f32 + edge_attr (E,2) f32), its epoch
iterator and the PNA in-degree histogram, on the GPU (csrc/collate.hip: the float instance of k_collate_fill, gt_store_in_degree,
gt_degree_histogram).

Everything is compared BITWISE: float rows are copied, the rest is integer work.  References: oracle/collate.py for the batch, the
numpy statement of tests/test_graph_store_host.py for the histogram.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from graphtrans_amd import synth
from oracle import collate as oc
from test_graph_store_host import max_in_degree, np_degree_histogram, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def float_graphs(G, x_cols, seed, ea_cols=0):
    """G graphs of odd and even sizes with float32 features of arbitrary bit patterns (NaN, -0.0 and denormals among them).
    Graph 3 is a single node without edges, graph 7 has nodes but no edge at all."""
    rng = np.random.default_rng(seed)
    graphs = []
    for i in range(G):
        n = 1 if i == 3 else int(rng.integers(1, 41))
        m = 0 if i in (3, 7) or n < 2 else int(rng.integers(0, 3 * n))
        x = rng.standard_normal((n, x_cols), dtype=np.float32)
        k = min(4, x.size)
        x.reshape(-1)[:k] = np.array([np.nan, -0.0, 1e-42, np.inf], np.float32)[:k]
        g = dict(x=x, edge_index=rng.integers(0, n, (2, m)).astype(np.int64), y=rng.integers(0, 2, 1).astype(np.int64))
        if ea_cols:
            g["edge_attr"] = rng.standard_normal((m, ea_cols), dtype=np.float32)
        graphs.append(g)
    return graphs


def check_batch(b, want, keys, what):
    for k in keys:
        assert same(getattr(b, k).cpu().numpy(), want[k]), (what, k)


# ----------------------------------------------------------------------------------------- float collate
@pytest.mark.parametrize("x_cols", [1, 3, 4, 8, 37, 38])
def test_float_x_collate_matches_oracle(x_cols):
    """x_cols 4 and 8: 16-byte vectors for every graph; 38: vectors only for graphs at an even node offset on both sides; 1, 3, 37:
    whatever alignment the offsets leave, dwords otherwise."""
    from graphtrans_amd.data import GraphStore
    raw = float_graphs(64, x_cols, seed=x_cols)
    store = GraphStore(raw)
    assert store.x.dtype == torch.float32 and store.edge_attr is None
    rng = np.random.default_rng(0)
    for B in (1, 2, 17, 64):
        ids = rng.permutation(64)[:B]
        if B == 17:
            ids[5] = ids[2]          # a repeated id
            ids[9], ids[11] = 3, 7   # the one-node graph and the edgeless graph
        want = oc.collate([raw[i] for i in ids])
        b = store.collate(ids)
        assert b.x.dtype == torch.float32 and b.x.shape == (want["x"].shape[0], x_cols) and b.edge_attr is None
        check_batch(b, want, ("x", "edge_index", "batch", "y"), (x_cols, B))
        assert b.num_graphs == B and np.array_equal(b._sizes, np.diff(want["ptr"]))
    for ids in ([3], [7, 3, 3]):
        check_batch(store.collate(ids), oc.collate([raw[i] for i in ids]), ("x", "edge_index", "batch", "y"), ids)
    b = store.collate([])
    assert b.x.shape == (0, x_cols) and b.x.dtype == torch.float32 and b.edge_index.shape == (2, 0) and b.num_graphs == 0
    with pytest.raises(IndexError):
        store.collate([64])
    with pytest.raises(IndexError):
        store.collate([0, -1])
    assert store.nbytes() >= store.x.numel() * 4


def test_float_edge_attr_collate_matches_oracle():
    """the ER shape: float x and float edge_attr (E, 2) stored, no augmentation"""
    from graphtrans_amd.data import GraphStore
    raw = synth.er_raw(12, 1, n=64, feat_dim=8)
    store = GraphStore(raw)
    assert not store.augment and store.edge_attr.dtype == torch.float32 and store.x.dtype == torch.float32
    assert store.nbytes() >= store.x.numel() * 4 + store.edge_attr.numel() * 4
    for ids in ([0], [11, 2, 2, 5], np.random.default_rng(1).permutation(12), np.arange(12)):
        want = oc.collate([raw[i] for i in ids])
        b = store.collate(ids)
        assert b.edge_attr.dtype == torch.float32 and b.edge_attr.shape == want["edge_attr"].shape
        check_batch(b, want, ("x", "edge_index", "edge_attr", "batch", "y"), list(ids))
    ref = synth.er_stress(12, 1, n=64, feat_dim=8)
    for k in ("x", "edge_index", "edge_attr", "batch", "y"):
        assert same(b.__dict__[k].cpu().numpy(), getattr(ref, k).numpy()), k
    b = store.collate([])
    assert b.x.shape == (0, 8) and b.edge_attr.shape == (0, 2) and b.edge_attr.dtype == torch.float32
    # odd edge counts, 3 float columns, next to an int64 x: every mix of the two kinds goes through the float instance
    raw = float_graphs(20, 4, seed=9, ea_cols=3)
    for g in raw:
        g["x"] = np.arange(g["x"].shape[0] * 2).reshape(-1, 2)
    store = GraphStore(raw)
    assert store.x.dtype == torch.int64 and store.edge_attr.dtype == torch.float32
    ids = [19, 3, 7, 0, 0, 12]
    b = store.collate(ids)
    assert b.x.dtype == torch.int64
    check_batch(b, oc.collate([raw[i] for i in ids]), ("x", "edge_index", "edge_attr", "batch", "y"), "int x, float edge_attr")


def test_nci1_store_collates_to_the_benchmark_batch():
    from graphtrans_amd.data import GraphStore
    b = GraphStore(synth.nci1_raw(32, 0)).collate(np.arange(32))
    ref = synth.nci1_like(32, 0)
    assert b.edge_attr is None and ref.edge_attr is None
    for k in ("x", "edge_index", "batch", "y"):
        assert same(getattr(b, k).cpu().numpy(), getattr(ref, k).numpy()), k


def test_constructor_contract():
    from graphtrans_amd.data import GraphStore
    g = lambda x, **kw: dict(x=x, edge_index=np.zeros((2, 0), np.int64), **kw)   # noqa: E731
    with pytest.raises(TypeError):
        GraphStore([g(np.zeros((3, 4), np.float64))])
    with pytest.raises(TypeError):
        GraphStore([g(np.zeros((3, 4), np.float16))])
    with pytest.raises(TypeError):
        GraphStore([g(np.zeros((3, 4), np.float32), edge_attr=np.zeros((0, 2), np.float64))])
    with pytest.raises(ValueError):
        GraphStore([g(np.zeros((3, 4), np.float32)), g(np.zeros((2, 4), np.int64))])
    with pytest.raises(ValueError):
        GraphStore([g(np.zeros((3, 4), np.float32)), g(np.zeros((2, 5), np.float32))])
    with pytest.raises(ValueError):
        GraphStore([g(np.zeros((3, 2), np.int64), edge_attr=np.zeros((0, 2), np.int64)),
                    g(np.zeros((3, 2), np.int64), edge_attr=np.zeros((0, 2), np.float32))])
    # integer kinds other than int64 are widened as before
    s = GraphStore([dict(x=np.arange(6, dtype=np.int32).reshape(3, 2), edge_index=np.array([[0], [2]])), g(np.ones((1, 2), np.uint8))])
    b = s.collate([1, 0])
    assert s.x.dtype == torch.int64 and b.x.cpu().tolist() == [[1, 1], [0, 1], [2, 3], [4, 5]] and b.edge_index.cpu().tolist() == [[1], [3]]


def test_gt_collate_rejects_mismatched_descriptors_and_keeps_the_bounds_guard():
    from graphtrans_amd import _lib
    from graphtrans_amd.data import GraphStore, _CollateOut, _StoreDesc
    raw = float_graphs(6, 4, seed=2, ea_cols=2)
    store = GraphStore(raw)
    L = _lib.lib()
    assert L.gt_version() >= 101
    ids = np.array([0, 1, 2, 4, 5], np.int64)
    want = oc.collate([raw[i] for i in ids])
    N, E = want["x"].shape[0], want["edge_index"].shape[1]
    d_ids = torch.from_numpy(ids).to(DEV)
    x = torch.full((N, 4), -7.0, device=DEV)
    xi = torch.zeros(N, 4, dtype=torch.int64, device=DEV)
    batch = torch.full((N,), -1, dtype=torch.int64, device=DEV)
    ei = torch.full((2, E), -1, dtype=torch.int64, device=DEV)
    ea = torch.full((E, 2), -7.0, device=DEV)
    eai = torch.zeros(E, 2, dtype=torch.int64, device=DEV)
    ws_bytes = L.gt_collate_workspace_bytes(ids.size)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(desc, out, n=N, e=E):
        return L.gt_collate(ctypes.byref(desc), d_ids.data_ptr(), ids.size, n, e, ctypes.byref(out), ws.data_ptr(), ws_bytes, stream)

    def desc(**kw):
        d = _StoreDesc.from_buffer_copy(store._desc)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def out(**kw):
        o = dict(x=None, node_depth=None, batch=batch.data_ptr(), ptr=None, edge_index=ei.data_ptr(), edge_attr_f32=ea.data_ptr(),
                 edge_attr_i64=None, y=None, x_f32=x.data_ptr())
        o.update(kw)
        return _CollateOut(**o)

    INVALID = -1
    assert call(desc(x=xi.data_ptr()), out()) == INVALID                                   # both x and x_f32
    assert call(desc(x_f32=None), out()) == INVALID                                        # neither
    assert call(desc(), out(x=xi.data_ptr(), x_f32=None)) == INVALID                       # int64 output for a float store
    assert call(desc(), out(x=xi.data_ptr())) == INVALID                                   # both outputs
    assert call(desc(), out(edge_attr_f32=None, edge_attr_i64=eai.data_ptr())) == INVALID  # int64 edge_attr output, float stored
    assert call(desc(edge_attr=eai.data_ptr()), out()) == INVALID                          # both edge_attr kinds stored
    assert call(desc(edge_attr_f32=None), out()) == INVALID                                # float edge_attr output, none stored
    rank = torch.zeros(int(store.nodes.sum()) + 1, dtype=torch.int64, device=DEV)
    assert call(desc(attr_rank=rank.data_ptr()), out()) == INVALID                         # float edge_attr on an augmenting store
    assert b"edge_attr_f32" in L.gt_last_error()
    torch.cuda.synchronize()
    assert float(x.max()) == -7.0 and int(batch.max()) == -1   # nothing ran
    # a stated N one short of the truth: the last graph does not fit and is skipped; nothing of it is written
    assert call(desc(), out(), n=N - 1) == 0
    torch.cuda.synchronize()
    n_last = raw[5]["x"].shape[0]
    assert same(x.cpu().numpy()[:N - n_last], want["x"][:N - n_last]) and bool((x[N - n_last:] == -7.0).all())
    assert np.array_equal(batch.cpu().numpy()[:N - n_last], want["batch"][:N - n_last]) and bool((batch[N - n_last:] == -1).all())
    assert call(desc(), out()) == 0
    torch.cuda.synchronize()
    assert same(x.cpu().numpy(), want["x"]) and same(ea.cpu().numpy(), want["edge_attr"])


# ----------------------------------------------------------------------------------------- the batch is model input
def test_collated_nci1_batch_trains_the_fused_model_bit_for_bit():
    from graphtrans_amd import engine, losses
    from graphtrans_amd.data import GraphStore
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    args = SimpleNamespace(gnn_virtual_node=False, gnn_num_layer=3, gnn_emb_dim=64, gnn_JK="last", gnn_dropout=0.0, gnn_residual=False,
                           gnn_type="gcn", pretrained_gnn=None, freeze_gnn=None, d_model=32, nhead=4, dim_feedforward=64,
                           transformer_dropout=0.0, transformer_activation="relu", num_encoder_layers=1, max_input_len=1000,
                           transformer_norm_input=True, graph_pooling="cls", num_encoder_layers_masked=0, transformer_prenorm=False,
                           pos_encoder=False, max_seq_len=None, compute_dtype=torch.float32, token_layout="auto")
    torch.manual_seed(0)
    zero = lambda d: (lambda _e: 0)   # dataset/tud.py:67-71
    model = GNNTransformer(2, torch.nn.Linear(37, 64), zero, args).to(DEV).train()
    ref = synth.nci1_like(16, 3).to(DEV)
    got = GraphStore(synth.nci1_raw(16, 3)).collate(np.arange(16))
    assert engine.eligible(model, got, None) and engine.eligible(model, ref, None)

    def run(b):
        for p in model.parameters():
            p.grad = None
        torch.manual_seed(9)
        out = model(b)
        losses.tud_loss(out, b.y).backward()
        torch.cuda.synchronize()
        return out.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}

    o0, g0 = run(ref)
    o1, g1 = run(got)
    assert torch.equal(o0, o1)
    assert set(g0) == set(g1) and len(g0) > 0
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# ----------------------------------------------------------------------------------------- degree_histogram
def _code2_with_edge_case_chains():
    raw = synth.code2_raw(64, 5, mean_nodes=40.0)
    raw[1]["node_is_attributed"][:] = 0            # no next-token chain at all
    raw[2]["node_is_attributed"][:] = 1            # every node on the chain
    raw[3]["node_is_attributed"][:] = 0
    raw[3]["node_is_attributed"][0] = 1            # a single attributed node: still no edge
    raw.append(dict(x=np.array([[1, 2]]), edge_index=np.zeros((2, 0), np.int64), node_depth=np.zeros((1, 1), np.int64),
                    node_is_attributed=np.ones((1, 1), np.int64), y_arr=np.arange(5).reshape(1, 5)))
    return raw


@pytest.mark.parametrize("name", ["code2", "molpcba", "nci1"])
def test_degree_histogram_matches_numpy_statement(name):
    from graphtrans_amd.data import GraphStore
    raw = {"code2": _code2_with_edge_case_chains, "molpcba": lambda: synth.molpcba_raw(64, 3), "nci1": lambda: synth.nci1_raw(64, 0)}[name]()
    store = GraphStore(raw)
    assert store.augment == (name == "code2")
    G = len(raw)
    rng = np.random.default_rng(2)
    subset = rng.permutation(G)[:23]
    repeated = np.concatenate([subset[:5], subset[:5], [1, 2, 3, G - 1, 2]])
    for ids in (None, subset, repeated, [G - 1], []):
        top = max_in_degree(raw, ids)
        for bins in (800, 10 if top < 10 else top + 1, top + 1):
            got = store.degree_histogram(ids, bins=bins)
            assert got.dtype == torch.int64 and got.device.type == "cpu" and got.shape == (bins,)
            assert np.array_equal(got.numpy(), np_degree_histogram(raw, ids, bins=bins)), (name, bins)
        if top > 0:
            with pytest.raises(ValueError, match=str(top)):
                store.degree_histogram(ids, bins=top)
    total = store.degree_histogram(bins=800)
    assert int(total.sum()) == int(store.nodes.sum())
    assert int((total * torch.arange(800)).sum()) == int(store.out_edges.sum())   # every emitted edge has one destination
    with pytest.raises(IndexError):
        store.degree_histogram([G])
    with pytest.raises(ValueError):
        store.degree_histogram(bins=0)
    with pytest.raises(ValueError):
        store.degree_histogram(bins=8192)   # above what the per-block counters in LDS hold
    assert np.array_equal(store.degree_histogram(bins=8191)[:800].numpy(), total.numpy())


def test_gt_degree_histogram_rejects_bins_out_of_range():
    from graphtrans_amd import _lib
    from graphtrans_amd.data import GraphStore
    store = GraphStore(synth.nci1_raw(4, 0))
    L = _lib.lib()
    deg = torch.zeros(int(store.nodes.sum()), dtype=torch.int32, device=DEV)
    hist = torch.zeros(8, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert L.gt_degree_histogram(ctypes.byref(store._desc), deg.data_ptr(), None, 4, 8192, hist.data_ptr(), stream) == -2   # GT_ERR_UNSUPPORTED
    assert L.gt_degree_histogram(ctypes.byref(store._desc), deg.data_ptr(), None, 4, 0, hist.data_ptr(), stream) == -1
    assert L.gt_degree_histogram(ctypes.byref(store._desc), deg.data_ptr(), None, 5, 7, hist.data_ptr(), stream) == -1      # more graphs than stored, no ids


# ----------------------------------------------------------------------------------------- batches
def test_batches_walk_an_epoch():
    from graphtrans_amd.data import GraphStore, epoch_batches
    raw = synth.nci1_raw(50, 4)
    for i, g in enumerate(raw):
        g["y"] = np.array([i], np.int64)   # distinct labels: the labels name the graphs
    store = GraphStore(raw)
    got = list(store.batches(16, shuffle=True, seed=1))
    assert [b.num_graphs for b in got] == [16, 16, 16, 2]
    y = torch.cat([b.y for b in got]).cpu().numpy()
    assert sorted(y.tolist()) == list(range(50)) and y.tolist() != list(range(50))
    assert np.array_equal(y, np.concatenate(epoch_batches(50, 16, True, rng=1)))
    want = oc.collate([raw[i] for i in y[16:32]])
    check_batch(got[1], want, ("x", "edge_index", "batch", "y"), "second batch")
    assert [b.num_graphs for b in store.batches(16, shuffle=True, drop_last=True, seed=1)] == [16, 16, 16]
    split = np.array([40, 3, 17, 8, 25])
    y = torch.cat([b.y for b in store.batches(2, ids=split)]).cpu().numpy()
    assert y.tolist() == split.tolist()
