"""Host side of the graph store for float-feature datasets (TU / ER shapes), epoch batches and the PNA in-degree histogram.

No GPU here: the raw generators against the ready batches, the ready batches against digests taken before the generators were
factored (bench.py trains on them), `data.epoch_batches` (pure index logic), and the numpy statement of the histogram that
tests/test_hip_graph_store.py holds `GraphStore.degree_histogram` to.
"""
import hashlib

import numpy as np
import pytest

from graphtrans_amd import synth
from graphtrans_amd.data import epoch_batches
from oracle import collate as oc


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def np_degree_histogram(graphs, ids=None, bins=800, augment=None):
    """dataset/code.py:122-130 / dataset/mol.py:71-79: `deg += bincount(degree(edge_index[1], num_nodes), minlength=bins)` per
    graph, over the edges the loader hands out (the augmented ones where the dataset carries `augment_edge`).  A degree >= bins
    fails, as the reference's `+=` does."""
    augment = ("node_is_attributed" in graphs[0]) if augment is None else augment
    hist = np.zeros(bins, np.int64)
    for i in (range(len(graphs)) if ids is None else ids):
        g = graphs[i]
        ei = oc.augment_edge(g["edge_index"], g["node_is_attributed"])[0] if augment else np.asarray(g["edge_index"])
        d = np.bincount(ei[1], minlength=g["x"].shape[0])
        hist += np.bincount(d, minlength=bins)   # shape error if a degree >= bins
    return hist


def max_in_degree(graphs, ids=None):
    augment = "node_is_attributed" in graphs[0]
    top = 0
    for i in (range(len(graphs)) if ids is None else ids):
        g = graphs[i]
        ei = oc.augment_edge(g["edge_index"], g["node_is_attributed"])[0] if augment else np.asarray(g["edge_index"])
        top = max(top, int(np.bincount(ei[1], minlength=1).max()))
    return top


# ------------------------------------------------------------------------------ raw generators
def test_nci1_raw_collates_to_nci1_like():
    for B, s in ((32, 0), (5, 3)):
        got = oc.collate(synth.nci1_raw(B, s))
        b = synth.nci1_like(B, s)
        assert "edge_attr" not in got and b.edge_attr is None
        for k in ("x", "edge_index", "batch", "y"):
            assert same(got[k], getattr(b, k).numpy()), (B, s, k)
        assert got["x"].dtype == np.float32 and got["x"].shape[1] == 37
    assert synth.nci1_raw(3, 0, num_features=5)[0]["x"].shape[1] == 5


def test_er_raw_collates_to_er_stress():
    kw = dict(n=64, feat_dim=8)
    got = oc.collate(synth.er_raw(3, 1, **kw))
    b = synth.er_stress(3, 1, **kw)
    for k in ("x", "edge_index", "edge_attr", "batch", "y"):
        assert same(got[k], getattr(b, k).numpy()), k
    assert got["x"].dtype == np.float32 and got["edge_attr"].dtype == np.float32 and got["edge_attr"].shape[1] == 2


def _digest(b):
    h = hashlib.sha256()
    for k in sorted(b.keys()):
        v = getattr(b, k)
        if v is None:
            h.update(f"{k}:None;".encode())
            continue
        a = v.numpy()
        h.update(f"{k}:{a.dtype}:{a.shape};".encode())
        h.update(a.tobytes())
    return h.hexdigest()


# sha256 over every attribute (name, dtype, shape, bytes) of the batch, taken at the commit before nci1_like / er_stress were
# factored into raw generators
DIGESTS = {
    "nci1": "f8d9cf8fd10a0fce2645ea0696d109ff0cde8d0ebf3edb75ae6c1e8e3ef4d574",
    "er": "d5f7b9022c1c69d096adaa707968b9785ad37b4e3262b68c7ed0fa8d245975c5",
    "code2": "02cdd5f79610684113909e284aba8cf801ecdb603b18fcfef1c882c5c222f28d",
    "molpcba": "e4f968dbc1e335327ca69481dd0476f655795f0db97d8484e960b66a5ca2927a",
}


@pytest.mark.parametrize("name", sorted(DIGESTS))
def test_ready_batches_are_unchanged(name):
    b = {"nci1": lambda: synth.nci1_like(32, 0), "er": lambda: synth.er_stress(2, 0, n=64, feat_dim=8),
         "code2": lambda: synth.code2_like(8, 0), "molpcba": lambda: synth.molpcba_like(8, 0)}[name]()
    assert _digest(b) == DIGESTS[name]


# ------------------------------------------------------------------------------ epoch_batches
def test_epoch_batches_in_order():
    bs = epoch_batches(10, 4)
    assert [b.tolist() for b in bs] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert all(b.dtype == np.int64 for b in bs)
    assert [b.tolist() for b in epoch_batches(10, 4, drop_last=True)] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert [b.tolist() for b in epoch_batches(8, 4, drop_last=True)] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert [b.tolist() for b in epoch_batches(3, 4)] == [[0, 1, 2]] and epoch_batches(3, 4, drop_last=True) == []


@pytest.mark.parametrize("n,bs", [(50, 16), (64, 16), (1, 3), (7, 1)])
def test_epoch_batches_shuffled_cover_every_id_once(n, bs):
    for drop_last in (False, True):
        got = epoch_batches(n, bs, shuffle=True, drop_last=drop_last, rng=1)
        sizes = [b.size for b in got]
        full, rest = divmod(n, bs)
        assert sizes == [bs] * full + ([rest] if rest and not drop_last else [])
        flat = np.concatenate(got) if got else np.zeros(0, np.int64)
        assert np.unique(flat).size == flat.size and set(flat.tolist()) <= set(range(n))
        if not drop_last:
            assert sorted(flat.tolist()) == list(range(n))


def test_epoch_batches_seed_and_generator():
    a = epoch_batches(50, 16, shuffle=True, rng=7)
    b = epoch_batches(50, 16, shuffle=True, rng=7)
    c = epoch_batches(50, 16, shuffle=True, rng=8)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not all(np.array_equal(x, y) for x, y in zip(a, c))
    assert np.concatenate(a).tolist() != list(range(50))
    # a Generator is advanced: two epochs from one generator differ, and match two epochs of an equal generator
    g1, g2 = np.random.default_rng(3), np.random.default_rng(3)
    e1, e2 = epoch_batches(20, 8, True, rng=g1), epoch_batches(20, 8, True, rng=g1)
    f1, f2 = epoch_batches(20, 8, True, rng=g2), epoch_batches(20, 8, True, rng=g2)
    assert np.concatenate(e1).tolist() != np.concatenate(e2).tolist()
    assert np.concatenate(e1).tolist() == np.concatenate(f1).tolist() and np.concatenate(e2).tolist() == np.concatenate(f2).tolist()


def test_epoch_batches_over_a_split_and_empty():
    split = np.array([40, 3, 17, 8, 25, 11, 30])
    got = epoch_batches(split, 3)
    assert [b.tolist() for b in got] == [[40, 3, 17], [8, 25, 11], [30]]
    got = epoch_batches(split, 3, shuffle=True, rng=0)
    assert sorted(np.concatenate(got).tolist()) == sorted(split.tolist()) and [b.size for b in got] == [3, 3, 1]
    assert split.tolist() == [40, 3, 17, 8, 25, 11, 30]   # the caller's array is not permuted in place
    assert epoch_batches([], 4) == [] and epoch_batches(np.zeros(0, np.int64), 4, shuffle=True, drop_last=True) == []
    assert epoch_batches(0, 4) == []
    with pytest.raises(ValueError):
        epoch_batches(5, 0)


# ------------------------------------------------------------------------------ the histogram's numpy statement
def test_numpy_degree_histogram_on_hand_made_graphs():
    """the graph of test_oracle_augment_edge_properties: AST 0->1, 0->4, 1->2, 1->3, chain 1 -> 2 -> 4.
    Augmented edges: [[0,0,1,1, 1,4,2,3, 1,2, 2,4], [1,4,2,3, 0,0,1,1, 2,4, 1,2]]; in-degrees of nodes 0..4 = 2, 4, 3, 1, 2."""
    g = dict(x=np.zeros((5, 2), np.int64), edge_index=np.array([[0, 0, 1, 1], [1, 4, 2, 3]]),
             node_is_attributed=np.array([0, 1, 1, 0, 1]).reshape(-1, 1))
    assert np_degree_histogram([g], bins=6).tolist() == [0, 1, 2, 1, 1, 0]
    # the stored edges alone (a dataset without the transform): in-degrees 0, 1, 1, 1, 1
    assert np_degree_histogram([g], bins=6, augment=False).tolist() == [1, 4, 0, 0, 0, 0]
    # a one-node graph without edges adds one node of degree 0; a graph listed twice counts twice
    lone = dict(x=np.zeros((1, 2), np.int64), edge_index=np.zeros((2, 0), np.int64), node_is_attributed=np.ones((1, 1), np.int64))
    assert np_degree_histogram([g, lone], bins=5).tolist() == [1, 1, 2, 1, 1]
    assert np_degree_histogram([g, lone], ids=[1, 0, 0], bins=5).tolist() == [1, 2, 4, 2, 2]
    assert max_in_degree([g, lone]) == 4 and max_in_degree([g, lone], ids=[1]) == 0
    with pytest.raises(ValueError):
        np_degree_histogram([g], bins=4)   # degree 4 needs 5 bins
