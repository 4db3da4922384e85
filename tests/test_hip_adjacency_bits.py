"""gt_adj_mask_bits / ops.adjacency_bits against the numpy reference of tests/adjacency_refs.py, word for word.

Cases: one word and a partial word (T 17); three words with a partial last one, a single-node graph and graphs that end on, one
before and one behind a word boundary (T 65); five words and three 64-row tiles (T 130); a graph without edges and a batch without
any edge; duplicate edges and explicit self-loop edges under both self_loops values; with and without key_valid (a prefix and a
suffix of zeros, the pattern of test_dense_masks_fp32_head_dim_128).  The words behind the end of the output stay untouched."""
import numpy as np
import pytest
import torch

from adjacency_refs import adjacency_keep_ref, random_edges

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


def _structure(ei, sizes):
    from graphtrans_amd.graph import GraphStructure

    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    gs = GraphStructure.build(torch.from_numpy(ei).to(DEV), batch.to(DEV), num_graphs=len(sizes), sizes=sizes)
    gs.validate()
    return gs


def _key_valid(B, T):
    kv = torch.ones(B, T)
    kv[0, T - T // 4:] = 0.0   # a suffix
    kv[B - 1, :3] = 0.0        # a prefix
    return kv


def _check(ei, sizes, T, key_valid, self_loops):
    from graphtrans_amd import _lib, ops
    from graphtrans_amd.graph import _ptr, _stream

    gs = _structure(ei, sizes)
    want_keep, want_words = adjacency_keep_ref(ei, sizes, T, None if key_valid is None else key_valid.numpy(), self_loops)
    kv = None if key_valid is None else key_valid.to(DEV)
    got = ops.adjacency_bits(gs, T, key_valid=kv, self_loops=self_loops)
    B, W = len(sizes), (T + 31) // 32
    assert (got.B, got.T, got.W) == (B, T, W) and got.bits.dtype == torch.int32 and tuple(got.bits.shape) == (B, T, W)
    want = torch.from_numpy(want_words.view(np.int32))
    assert torch.equal(got.bits.cpu(), want), f"{int((got.bits.cpu() != want).sum())} of {want.numel()} words differ"
    assert torch.equal(got.dense().cpu(), torch.from_numpy(want_keep).float())
    # the raw entry into a guarded buffer: every word written, none behind the end
    buf = torch.full((B * T * W + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    _lib.launch("gt_adj_mask_bits", _ptr(gs.graph_ptr), _ptr(gs.out_ptr), _ptr(gs.out_dst), gs.N, gs.E, B, T, _ptr(kv),
                1 if self_loops else 0, _ptr(buf), _stream())
    torch.cuda.synchronize()
    assert torch.equal(buf[:B * T * W].cpu().view(B, T, W), want)
    assert bool((buf[B * T * W:] == 0x5A5A5A5A).all()), "a store behind the end of bits"


@pytest.mark.parametrize("with_kv", [False, True])
@pytest.mark.parametrize("sizes,T", [((9, 4, 17, 6), 17), ((1, 33, 64, 65, 31), 65), ((130, 5, 64, 129), 130)])
def test_bits_equal_the_reference(sizes, T, with_kv):
    ei = random_edges(sizes, seed=T)
    _check(ei, list(sizes), T, _key_valid(len(sizes), T) if with_kv else None, True)


@pytest.mark.parametrize("self_loops", [False, True])
def test_duplicate_and_self_loop_edges(self_loops):
    sizes = [9, 4, 17, 6]
    ei = random_edges(sizes, seed=3, duplicates=True, loops=True)
    assert (ei[0] == ei[1]).any() and np.unique(ei, axis=1).shape[1] < ei.shape[1]
    _check(ei, sizes, 17, None, self_loops)
    _check(ei, sizes, 17, _key_valid(4, 17), self_loops)


@pytest.mark.parametrize("self_loops", [False, True])
def test_graph_without_edges_and_batch_without_edges(self_loops):
    sizes = [9, 4, 17, 6]
    _check(random_edges(sizes, seed=4, empty_graphs=(1, 2)), sizes, 17, None, self_loops)
    _check(np.zeros((2, 0), np.int64), sizes, 17, _key_valid(4, 17), self_loops)


def test_wider_T_than_every_graph_leaves_the_pad_empty():
    sizes = [9, 4, 17, 6]
    _check(random_edges(sizes, seed=5), sizes, 40, None, True)
