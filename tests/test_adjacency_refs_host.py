"""The numpy reference of the adjacency keep-bits (tests/adjacency_refs.py) against the G8_masked_train fixture, whose adj{g} arrays
were made by the reference's recipe without the identity (oracle/make_golden.py), and against its own two forms."""
import numpy as np
import pytest

from adjacency_refs import adjacency_keep_ref, pack_keep, random_edges, unpack_words
from conftest import Golden


def _fixture():
    g = Golden("G8_masked_train")
    sizes = [int(n) for n in g.meta["sizes"]]
    adj = [g.inputs[f"adj{i}"].numpy().astype(bool) for i in range(len(sizes))]
    return g.inputs["edge_index"].numpy(), sizes, adj


def test_fixture_adjacency_without_self_loops():
    ei, sizes, adj = _fixture()
    T = max(sizes)
    keep, words = adjacency_keep_ref(ei, sizes, T, None, self_loops=False)
    assert keep.shape == (len(sizes), T, T) and words.shape == (len(sizes), T, (T + 31) // 32) and words.dtype == np.uint32
    for b, n in enumerate(sizes):
        assert adj[b].shape == (n, n)
        assert np.array_equal(keep[b, :n, :n], adj[b]), f"graph {b}"
        assert not keep[b, n:, :].any() and not keep[b, :, n:].any(), f"graph {b}: something outside the top-left block"


def test_self_loops_are_the_identity_on_the_block():
    ei, sizes, adj = _fixture()
    T = max(sizes) + 3   # (a T wider than every graph: the pad rows and columns stay empty)
    keep, _ = adjacency_keep_ref(ei, sizes, T, None, self_loops=True)
    for b, n in enumerate(sizes):
        assert np.array_equal(keep[b, :n, :n], adj[b] | np.eye(n, dtype=bool)), f"graph {b}"
        assert not keep[b, n:, :].any() and not keep[b, :, n:].any(), f"graph {b}"


@pytest.mark.parametrize("T", [17, 32, 33, 65, 130])
def test_packed_and_dense_forms_agree_and_tail_bits_are_zero(T):
    sizes = [min(T, n) for n in (9, 1, T, 6, T - 1)]
    ei = random_edges(sizes, seed=T, duplicates=True, loops=True)
    kv = np.ones((len(sizes), T), np.float32)
    kv[0, :2] = 0.0
    kv[2, T // 2:] = 0.0
    for key_valid in (None, kv):
        keep, words = adjacency_keep_ref(ei, sizes, T, key_valid, self_loops=True)
        W = (T + 31) // 32
        assert words.shape == (len(sizes), T, W)
        bits = unpack_words(words, T)
        assert np.array_equal(bits[:, :, :T], keep)
        assert not bits[:, :, T:].any(), "bits at k >= T"
        for b, q, k in ((0, 0, 0), (2, T - 1, T - 1), (2, 3, T - 1), (4, 1, 2)):   # the addressing rule, bit by bit
            assert bool((int(words[b, q, k >> 5]) >> (k & 31)) & 1) == bool(keep[b, q, k])
            byte = words[b, q].view(np.uint8)[k >> 3]   # little-endian words: byte k >> 3, bit k & 7 is the same bit
            assert bool((int(byte) >> (k & 7)) & 1) == bool(keep[b, q, k])
        assert np.array_equal(pack_keep(keep), words)
        if key_valid is not None:
            assert not keep[0, :, :2].any() and not keep[2, :, T // 2:].any()
