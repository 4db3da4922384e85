"""Host half of the token layout and of the whole-model driver (csrc/seq_layout_host.h, csrc/model.hip), runnable without a GPU: the
layout built in C (gt_seq_layout_host, and graphtrans_amd/graph.py:SeqLayout on top of it) equals the numpy statement of it below (the
reference's pad_batch bookkeeping modules/utils.py:9-16 + the CLS position of modules/transformer_encoder.py:50-55), the staging ring
hands its slots out round robin, and the ctypes mirrors of the driver's structs have the library's sizes."""
import ctypes as C

import numpy as np
import pytest

KINDS = {"packed": 0, "padded": 1}


class _FakeGS:
    def __init__(self, sizes, device="cpu"):
        self.sizes = np.asarray(sizes, np.int64)
        self.B = len(sizes)
        self.device = device


def numpy_layout(sizes, kind, max_input_len, with_cls):
    """The oracle: ((rows, max_npos, num_work, S, row_stride), desc [B][4] int32, last_rows [B] int64, work [num_work][2] int32)."""
    n = np.asarray(sizes, np.int64)
    B = n.size
    cls = 1 if with_cls else 0
    S = int(min(int(n.max()) if B else 0, max_input_len))  # modules/utils.py:16
    kept = np.minimum(n, S)
    kv_len = kept + cls
    desc = np.zeros((B, 4), dtype=np.int32)
    if kind == "padded":
        npos = S + cls
        desc[:, 0] = np.arange(B)
        desc[:, 1] = npos
        desc[:, 2] = npos - kv_len
        desc[:, 3] = kv_len
        row_stride, rows, max_npos = B, npos * B, npos
    else:
        tok_ptr = np.concatenate([[0], np.cumsum(kv_len)])
        desc[:, 0] = tok_ptr[:-1]
        desc[:, 1] = kv_len
        desc[:, 2] = 0
        desc[:, 3] = kv_len
        row_stride, rows, max_npos = 1, int(tok_ptr[-1]), int(kv_len.max()) if B else 0
    # attention tile list: (sequence, 64-position tile) for every tile that exists; sequences dealt to the eight XCD slices by length
    # rank, each slice holds its own in descending length, padded with {-1, 0} entries to equal size
    tiles = (desc[:, 1].astype(np.int64) + 63) // 64
    if B:
        order = np.argsort(-desc[:, 1].astype(np.int64), kind="stable")
        xcd = np.arange(B) % 8                              # eighth of the sequence of length rank r
        perm = order[np.argsort(xcd, kind="stable")]        # = concat(order[x::8] for x in 0..7)
        xs = np.sort(xcd)                                   # eighth of perm[i]
        t = tiles[perm]
        cnt = np.bincount(xs, weights=t, minlength=8).astype(np.int64)   # tiles per eighth
        wpx = int(cnt.max())
        tot = int(t.sum())
        ws = np.repeat(perm, t)
        first = np.cumsum(t) - t                            # first work item of every sequence
        wt = np.arange(tot, dtype=np.int64) - np.repeat(first, t)
        seg0 = np.cumsum(cnt) - cnt                         # first work item of every eighth
        wx = np.repeat(xs, t)
        dest = wx * wpx + (np.arange(tot, dtype=np.int64) - seg0[wx])
        work = np.empty((8 * wpx, 2), np.int32)
        work[:, 0] = -1
        work[:, 1] = 0
        work[dest, 0] = ws
        work[dest, 1] = wt
    else:
        work = np.zeros((0, 2), np.int32)
    # token row of the last position (CLS / last node) of every sequence: the pooled row
    last_row = desc[:, 0].astype(np.int64) + (desc[:, 1].astype(np.int64) - 1) * row_stride
    return (rows, max_npos, int(work.shape[0]), S, row_stride), desc, last_row, work


def _host_layout(sizes, kind, max_len, cls):
    """the same four values from the raw entry"""
    from graphtrans_amd import _lib
    L = _lib.lib()
    sizes = np.ascontiguousarray(sizes, np.int64)
    B = sizes.size
    meta = (C.c_int64 * 8)()
    _lib.check(L.gt_seq_layout_host(KINDS[kind], sizes.ctypes.data, B, max_len, cls, None, 0, meta), "size")
    buf = np.zeros(meta[5], np.uint8)
    _lib.check(L.gt_seq_layout_host(KINDS[kind], sizes.ctypes.data, B, max_len, cls, buf.ctypes.data, buf.size, meta), "fill")
    return ((meta[0], meta[1], meta[2], meta[6], meta[7]), buf[:B * 16].view(np.int32).reshape(B, 4),
            buf[meta[3]:meta[3] + B * 8].view(np.int64), buf[meta[4]:meta[4] + meta[2] * 8].view(np.int32).reshape(-1, 2))


def check_seq_layout(lay, want):
    """a SeqLayout (on any device) against numpy_layout's answer"""
    meta, desc, last, work = want
    assert (lay.rows, lay.max_npos, lay.num_work, lay.S, lay.row_stride) == meta
    assert all(type(v) is int for v in (lay.rows, lay.max_npos, lay.num_work, lay.row_stride))
    assert lay.desc_cpu.dtype == np.int32 and np.array_equal(lay.desc_cpu, desc)
    assert np.array_equal(lay.desc.cpu().numpy(), desc) and np.array_equal(lay.last_rows.cpu().numpy(), last)
    if lay.work is None:    # (GPU layouts without a work item)
        assert meta[2] == 0 and lay.desc.is_cuda
    else:
        assert np.array_equal(lay.work.cpu().numpy(), work)


def _check_both(sizes, max_len):
    from graphtrans_amd.graph import SeqLayout
    for kind in KINDS:
        for cls in (0, 1):
            want = numpy_layout(sizes, kind, max_len, cls)
            meta, desc, last, work = _host_layout(sizes, kind, max_len, cls)
            assert meta == want[0]
            assert np.array_equal(desc, want[1]) and np.array_equal(last, want[2]) and np.array_equal(work, want[3])
            check_seq_layout(SeqLayout(_FakeGS(sizes), kind, max_len, bool(cls)), want)


@pytest.mark.parametrize("seed", range(6))
def test_host_layout_equals_numpy_layout(seed):
    rng = np.random.default_rng(seed)
    for _ in range(12):
        B = int(rng.integers(1, 300))
        sizes = rng.integers(1, 700, size=B).astype(np.int64)
        if seed % 3 == 0:
            sizes[:] = sizes[0]          # ties: the stable order by index decides
        max_len = int(rng.choice([1000, 200, 64, 1]))
        _check_both(sizes, max_len)


@pytest.mark.parametrize("sizes", [(), (1,), (130,)], ids=["B0", "B1", "B1-three-tiles"])
def test_host_layout_of_no_and_one_sequence(sizes):
    for max_len in (1000, 64, 1):
        _check_both(np.asarray(sizes, np.int64), max_len)


def test_packed_host_entry_is_the_packed_kind():
    from graphtrans_amd import _lib
    sizes = np.array([5, 70, 9, 3, 200], np.int64)
    m6 = (C.c_int64 * 6)()
    _lib.check(_lib.lib().gt_seq_layout_packed_host(sizes.ctypes.data, 5, 100, 1, None, 0, m6), "size")
    buf = np.zeros(m6[5], np.uint8)
    _lib.check(_lib.lib().gt_seq_layout_packed_host(sizes.ctypes.data, 5, 100, 1, buf.ctypes.data, buf.size, m6), "fill")
    meta, desc, last, work = numpy_layout(sizes, "packed", 100, 1)
    assert tuple(m6[:3]) == meta[:3]
    assert np.array_equal(buf[:80].view(np.int32).reshape(5, 4), desc) and np.array_equal(buf[m6[3]:m6[3] + 40].view(np.int64), last)
    assert np.array_equal(buf[m6[4]:m6[4] + m6[2] * 8].view(np.int32).reshape(-1, 2), work)


def test_host_layout_small_buffer_is_an_error():
    from graphtrans_amd import _lib
    sizes = np.array([5, 3, 9], np.int64)
    meta = (C.c_int64 * 6)()
    buf = np.zeros(8, np.uint8)
    rc = _lib.lib().gt_seq_layout_packed_host(sizes.ctypes.data, 3, 100, 1, buf.ctypes.data, buf.size, meta)
    assert rc != 0 and b"too small" in _lib.lib().gt_last_error()


def test_stage_ring_take_is_round_robin_and_refuses_what_does_not_fit():
    """gt_stage_ring_take on a ring without events over plain memory (no GPU call is made for a null event)"""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import StageRingDesc
    L = _lib.lib()
    slots, slot_bytes = 5, 48
    buf = np.zeros(slots * slot_bytes, np.uint8)
    ring = StageRingDesc()
    ring.base, ring.slot_bytes, ring.slots, ring.next = buf.ctypes.data, slot_bytes, slots, 0
    slot, event = C.c_void_p(), C.c_void_p(1)
    for i in range(2 * slots + 3):
        assert L.gt_stage_ring_take(C.byref(ring), (0, 1, slot_bytes)[i % 3], C.byref(slot), C.byref(event)) == 0
        assert slot.value == buf.ctypes.data + (i % slots) * slot_bytes and event.value is None
        assert ring.next == (i + 1) % slots
    before = ring.next
    slot.value = 7
    rc = L.gt_stage_ring_take(C.byref(ring), slot_bytes + 1, C.byref(slot), C.byref(event))
    assert rc != 0 and b"exceed the staging slot" in L.gt_last_error()
    assert ring.next == before and slot.value == 7


def test_struct_mirrors_have_the_library_sizes():
    from graphtrans_amd import engine
    engine._ABI_OK.clear()
    engine._check_abi()   # raises on a mismatch
    assert engine._ABI_OK
