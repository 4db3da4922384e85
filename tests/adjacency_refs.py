"""numpy reference of gt_adj_mask_bits / ops.adjacency_bits, written from the entry's stated semantics (include/graphtrans_hip.h):

with n_b = sizes[b] and ptr the prefix sum of sizes, keep[b][q][k] is True exactly when
  * q < n_b and k < n_b, and
  * the batch has an edge (ptr[b] + q) -> (ptr[b] + k) (row = edge_index[0], column = edge_index[1]; duplicates change nothing), or
    self_loops and q == k (the reference's np.eye, data/adj_list.py), and
  * key_valid is None or key_valid[b][k] != 0.
Packed form: uint32 words [B][T][ceil(T / 32)], key k = bit k & 31 of word k >> 5; bits at k >= T are 0.  A graph with n_b > T keeps
its first T nodes only (the model rejects such batches before it builds a mask).
"""
import numpy as np


def adjacency_keep_ref(edge_index, sizes, T, key_valid=None, self_loops=True):
    """-> (keep bool [B][T][T], words uint32 [B][T][W])"""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    sizes = np.asarray(sizes, np.int64)
    B, T = sizes.size, int(T)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    keep = np.zeros((B, T, T), dtype=bool)
    for b in range(B):
        n = int(min(sizes[b], T))
        sel = (ei[0] >= ptr[b]) & (ei[0] < ptr[b + 1])
        q, k = ei[0][sel] - ptr[b], ei[1][sel] - ptr[b]
        ok = (q < n) & (k >= 0) & (k < n)
        keep[b, q[ok], k[ok]] = True
        if self_loops:
            keep[b, np.arange(n), np.arange(n)] = True
    if key_valid is not None:
        keep &= (np.asarray(key_valid).reshape(B, 1, T) != 0)
    return keep, pack_keep(keep)


def pack_keep(keep):
    """bool [B][T][T] -> uint32 [B][T][W]: one python-level OR per bit position, no numpy packbits (its bit order is not the entry's)"""
    B, T, _ = keep.shape
    W = (T + 31) // 32
    wide = np.zeros((B, T, W * 32), dtype=np.uint32)
    wide[:, :, :T] = keep
    words = np.zeros((B, T, W), dtype=np.uint32)
    for j in range(32):
        words |= wide[:, :, j::32] << np.uint32(j)
    return words


def unpack_words(words, T):
    """uint32 [B][T][W] -> bool [B][T][W * 32] (every bit, the tail included)"""
    words = np.asarray(words, np.uint32)
    B, Tq, W = words.shape
    out = np.zeros((B, Tq, W * 32), dtype=bool)
    for j in range(32):
        out[:, :, j::32] = (words >> np.uint32(j)) & np.uint32(1)
    return out


def random_edges(sizes, seed, degree=3, empty_graphs=(), duplicates=False, loops=False):
    """edge_index int64 [2][E] of a block-diagonal batch: about `degree` out-edges per node inside each graph, in shuffled order;
    the graphs of `empty_graphs` get none.  duplicates: every tenth edge twice; loops: explicit (v, v) edges on every third node."""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    src, dst = [], []
    for b, n in enumerate(sizes):
        if b in empty_graphs or n == 0:
            continue
        m = int(n) * degree if n > 1 else 0
        s, d = rng.integers(0, n, m), rng.integers(0, n, m)
        if not loops:
            d = np.where(d == s, (d + 1) % n, d)
        else:
            v = np.arange(0, n, 3)
            s, d = np.concatenate([s, v]), np.concatenate([d, v])
        src.append(s + ptr[b])
        dst.append(d + ptr[b])
    if not src:
        return np.zeros((2, 0), np.int64)
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    if duplicates:
        ei = np.concatenate([ei, ei[:, ::10]], axis=1)
    return ei[:, rng.permutation(ei.shape[1])]
