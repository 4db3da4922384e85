"""Per-batch index structures for the HIP kernels (built once per collated batch on device).

Replaces the reference's per-layer `degree(row)` (modules/conv.py:57), its unsorted scatter
(conv.py:28,63) and the `batch.eq(i)` loops of pad_batch (modules/utils.py:9-13) with one call to
`gt_graph_prep`, plus the sequence layouts (`SeqLayout`) that describe how node rows map to
transformer token rows (padded = the reference's (S,B,d) layout; packed = no padding rows at all).
"""
import ctypes as C
import threading

import numpy as np
import torch

from . import _lib


def _stream():
    """raw hipStream_t of torch's current stream.  With an EXPLICIT device index: torch.cuda.current_stream() without one
    resolves "the current device" through torch._utils._get_available_device_type() -> torch.cuda.is_available() ->
    hipGetDeviceCount, 110 us of host time per call on the MI355X boxes (rocprofv3 --hip-trace: 5 calls = 0.55 ms per step)."""
    return torch.cuda.current_stream(torch.cuda.current_device()).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


class GraphStructure:
    """graph_ptr, node_graph, CSR by destination (in_*), CSC by source (out_*), deg, dis."""

    __slots__ = ("N", "E", "B", "device", "graph_ptr", "node_graph", "in_ptr", "in_src", "in_eid", "out_ptr",
                 "out_dst", "out_eid", "deg", "dis", "status", "_sizes", "_layouts", "_pna_scales", "_ws", "ready_event")

    @staticmethod
    def build(edge_index, batch, num_graphs=None, sizes=None, stream=None):
        """edge_index (2,E) int64, batch (N,) int64 sorted; both on the GPU.  `num_graphs` / `sizes`
        (host values, e.g. PyG Batch.num_graphs / the collater's per-graph node counts) avoid the
        device sync the reference performs at modules/gnn_module.py:195."""
        if not edge_index.is_cuda:
            raise RuntimeError("graphtrans_amd kernels run on the GPU only (no CPU fallback)")
        gs = GraphStructure()
        dev = edge_index.device
        N, E = int(batch.numel()), int(edge_index.shape[1])
        if num_graphs is None:
            num_graphs = len(sizes) if sizes is not None else (int(batch[-1].item()) + 1 if N > 0 else 0)
        B = int(num_graphs)
        edge_index = edge_index.contiguous()
        batch = batch.contiguous()
        if edge_index.dtype != torch.int64 or batch.dtype != torch.int64:
            raise TypeError("edge_index and batch must be int64 (PyG collation dtype)")
        i32 = dict(dtype=torch.int32, device=dev)
        gs.N, gs.E, gs.B, gs.device = N, E, B, dev
        gs.graph_ptr = torch.empty(B + 1, **i32)
        gs.node_graph = torch.empty(max(N, 1), **i32)
        gs.in_ptr = torch.empty(N + 1, **i32)
        gs.out_ptr = torch.empty(N + 1, **i32)
        idx = torch.empty(4, max(E, 1), **i32)
        gs.in_src, gs.in_eid, gs.out_dst, gs.out_eid = idx[0], idx[1], idx[2], idx[3]
        dd = torch.empty(2, max(N, 1), dtype=torch.float32, device=dev)
        gs.deg, gs.dis = dd[0], dd[1]
        gs.status = torch.empty(1, **i32)
        L = _lib.lib()
        ws_bytes = L.gt_graph_prep_workspace_bytes(N, E, B)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.launch("gt_graph_prep", _ptr(edge_index), _ptr(batch), N, E, B, _ptr(gs.graph_ptr), _ptr(gs.node_graph),
                    _ptr(gs.in_ptr), _ptr(gs.in_src), _ptr(gs.in_eid), _ptr(gs.out_ptr), _ptr(gs.out_dst),
                    _ptr(gs.out_eid), _ptr(gs.deg), _ptr(gs.dis), _ptr(gs.status), _ptr(ws), ws_bytes, _stream() if stream is None else stream)
        gs._ws = ws   # (with a caller's stream the workspace must outlive this call's allocator scope)
        gs.ready_event = None   # set by a caller that built on a side stream: consumers wait for it once (engine.prep_*)
        gs._sizes = None if sizes is None else np.asarray(sizes, dtype=np.int64)
        gs._layouts = {}
        gs._pna_scales = None
        return gs

    def validate(self):
        """Raise if gt_graph_prep saw an out-of-range edge/batch index (device sync)."""
        s = int(self.status.item())
        if s:
            raise ValueError("edge_index / batch out of range or batch not sorted (gt_graph_prep status %d)" % s)

    @property
    def sizes(self):
        """Host per-graph node counts (one small D2H copy if the collater did not supply them)."""
        if self._sizes is None:
            p = self.graph_ptr.cpu().numpy().astype(np.int64)
            self._sizes = np.diff(p)
        return self._sizes

    def layout(self, kind, max_input_len, with_cls):
        key = (kind, int(max_input_len), bool(with_cls))
        if key not in self._layouts:
            if kind == "packed" and self._sizes is None and torch.device(self.device).type == "cuda":
                # sizes unknown on the host (a bare device batch): build the layout on the device, no D2H sync
                self._layouts[key] = SeqLayout.packed_on_device(self, int(max_input_len), bool(with_cls))
            else:
                self._layouts[key] = SeqLayout(self, kind, int(max_input_len), bool(with_cls))
        return self._layouts[key]


class StageRingDesc(C.Structure):   # gt_stage_ring (include/graphtrans_hip.h; size checked by engine._check_abi)
    _fields_ = [("base", C.c_void_p), ("slot_bytes", C.c_int64), ("slots", C.c_int32), ("next", C.c_int32), ("events", C.c_void_p * 64)]


class StageRing:
    """ONE pinned host allocation per device cut into slots (pinning costs ~1 ms per allocation), handed out round robin by
    gt_stage_ring_take; a slot is reused only after the H2D copy that last read it has completed (its library event, recorded behind
    that copy, is waited for if the host is more than a ring ahead of the device).  Both paths stage their token layout here: SeqLayout
    below and gt_model_prepare (engine.py), each under `lock` (autograd's backward threads and data-loader threads build layouts too)."""
    SLOTS, SLOT_BYTES = 64, 1 << 17

    def __init__(self, device):
        lib = _lib.lib()
        self.buf = torch.empty(self.SLOTS * self.SLOT_BYTES, dtype=torch.uint8).pin_memory()
        self.desc = d = StageRingDesc()
        d.base, d.slot_bytes, d.slots, d.next = self.buf.data_ptr(), self.SLOT_BYTES, self.SLOTS, 0
        with torch.cuda.device(device):   # the events belong to the ring's device
            for i in range(self.SLOTS):
                d.events[i] = lib.gt_event_create()
        self.lock = threading.Lock()

    def take(self, nbytes):
        """(the first `nbytes` of the next slot, the library event to record behind the copy that reads them)"""
        slot, event = C.c_void_p(), C.c_void_p()
        with self.lock:
            _lib.check(_lib.lib().gt_stage_ring_take(C.byref(self.desc), nbytes, C.byref(slot), C.byref(event)), "gt_stage_ring_take")
        off = slot.value - self.desc.base
        return self.buf[off:off + nbytes], event


_RINGS = {}
_RINGS_LOCK = threading.Lock()   # held for the table only: a wait on one device's ring does not block another device


def stage_ring(device):
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    with _RINGS_LOCK:
        ring = _RINGS.get(key)
        if ring is None:
            ring = _RINGS[key] = StageRing(key)
    return ring


_KINDS = {"packed": 0, "padded": 1}   # enum gt_seq_kind


class SeqLayout:
    """seq_desc[B][4] = {row0, npos, kv_off, kv_len} (see include/graphtrans_hip.h).

    exact: rows / num_work / max_npos are the true counts (host-built).  A device-built layout (packed_on_device) only
    knows upper bounds on the host: its token buffers must be ZERO-initialised, the rows past the true count then stay
    finite through every row-wise kernel and contribute exactly 0 to every weight gradient.

    padded: the reference layout of pad_batch + CLS (modules/utils.py:5-29,
            modules/transformer_encoder.py:50-55): rows = S' x B, position-major, left padded.
    packed: only real tokens, graph after graph: rows = sum_b (kept_b + cls).
    """

    exact = True

    @classmethod
    def packed_on_device(cls, gs, max_input_len, with_cls):
        """gt_seq_layout_packed: desc / last_rows / work list from graph_ptr on the device (the reference's pad_batch loop,
        modules/utils.py:9-16, costs O(B) device syncs; the host-built layout one D2H copy when sizes are unknown)."""
        self = cls.__new__(cls)
        B, N, c = gs.B, gs.N, 1 if with_cls else 0
        dev = gs.device
        self.kind, self.with_cls, self.B, self.exact = "packed", with_cls, B, False
        self.row_stride = 1
        self.rows = N + B * c                      # upper bound: truncation (n > max_input_len) only removes rows
        self.max_npos = min(int(max_input_len), N) + c
        self.num_work = B + self.rows // 64        # upper bound on sum_b ceil(kv_len_b / 64)
        self.desc = torch.empty((B, 4), dtype=torch.int32, device=dev)
        self.last_rows = torch.empty(B, dtype=torch.int64, device=dev)
        self.work = torch.empty((max(self.num_work, 1), 2), dtype=torch.int32, device=dev)
        self.meta = torch.empty(4, dtype=torch.int32, device=dev)
        _lib.launch("gt_seq_layout_packed", _ptr(gs.graph_ptr), B, int(max_input_len), c, _ptr(self.desc), _ptr(self.last_rows),
                    _ptr(self.work), self.num_work, _ptr(self.meta), _stream())
        return self

    def __init__(self, gs, kind, max_input_len, with_cls):
        if kind not in _KINDS:
            raise ValueError(kind)
        n, B = gs.sizes, gs.B
        # desc / last_rows / attention work list: ONE blob from the library's host builder (csrc/seq_layout_host.h), sized first and
        # then written straight into the buffer the H2D copy reads
        L = _lib.lib()
        sizes = np.ascontiguousarray(n, dtype=np.int64)
        args = (_KINDS[kind], sizes.ctypes.data, B, int(max_input_len), 1 if with_cls else 0)
        meta = (C.c_int64 * 8)()
        _lib.check(L.gt_seq_layout_host(*args, None, 0, meta), "gt_seq_layout_host")
        self.rows, self.max_npos, self.num_work, o_l, o_w, nbytes, S, self.row_stride = meta
        self.kind, self.with_cls, self.S, self.B = kind, with_cls, S, B   # S = min(largest graph, max_input_len): modules/utils.py:16
        self.kept = np.minimum(n, S)
        self._n = n
        on_gpu = torch.device(gs.device).type == "cuda"
        event = None
        if not on_gpu:
            hb = torch.empty(nbytes, dtype=torch.uint8)
        elif nbytes <= StageRing.SLOT_BYTES:
            # ONE pinned staging slot from the device's ring (pin_memory() per array cost ~30 us each) and ONE non_blocking H2D copy: a
            # pageable copy would block the host until everything already queued on the stream has drained (a 10 ms/step stall once)
            hb, event = stage_ring(gs.device).take(nbytes)
        else:   # (larger than a ring slot: its own pinned buffer)
            hb = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        _lib.check(L.gt_seq_layout_host(*args, hb.data_ptr(), nbytes, meta), "gt_seq_layout_host")
        nd, nl, nw = B * 16, B * 8, self.num_work * 8
        self.desc_cpu = hb[:nd].numpy().view(np.int32).reshape(B, 4).copy()   # (owned: the slot is reused later)
        if on_gpu:
            with torch.cuda.device(gs.device):
                db = torch.empty(nbytes, dtype=torch.uint8, device=gs.device)
                db.copy_(hb, non_blocking=True)
                if event is not None:   # on the stream of the copy, whatever the caller's current device is
                    _lib.check(L.gt_event_record(event, torch.cuda.current_stream(gs.device).cuda_stream), "gt_event_record")
        else:
            db = hb
        self._dev = db
        self.desc = db[:nd].view(torch.int32).view(B, 4)
        self.last_rows = db[o_l:o_l + nl].view(torch.int64)
        self.work = db[o_w:o_w + nw].view(torch.int32).view(-1, 2) if self.num_work or not on_gpu else None

    def positions(self):
        """int32 [N] (host, exact layouts): the padded position of every node -- pad_batch left-pads to S (modules/utils.py:16-25),
        so the j-th kept node of graph b, node row graph_ptr[b+1] - kept_b + j, sits at S - kept_b + j; -1 for the nodes a truncated
        graph drops.  What PositionalEncoding indexes its table by, whatever the token layout (csrc/segment.hip:k_seq_positions)."""
        n, kept, S = np.asarray(self._n, dtype=np.int64), np.asarray(self.kept, dtype=np.int64), self.S
        j = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)   # index of the node inside its graph
        drop = np.repeat(n - kept, n)
        return np.where(j >= drop, S - np.repeat(kept, n) + (j - drop), -1).astype(np.int32)
