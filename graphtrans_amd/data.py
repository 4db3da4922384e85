"""Minimal stand-in for the PyG `Batch` object the reference's modules consume.

The reference reads only attributes (`x, edge_index, edge_attr, batch, node_depth, y, y_arr,
adj_list`; modules/gnn_module.py:61-62,173-174, models/gnn_transformer.py:95,103), so a plain
attribute bag with `.to(device)` is a drop-in for the hot path.
"""
import ctypes

import torch


def _stream():   # (graph.py imports this module's Batch lazily; keep data.py free of package imports at module level)
    from .graph import _stream as f
    return f()


class Batch:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def to(self, device, non_blocking=False):
        out = Batch()
        for k, v in self.__dict__.items():
            out.__dict__[k] = v.to(device, non_blocking=non_blocking) if isinstance(v, torch.Tensor) else v
        return out

    @property
    def num_graphs(self):
        if "_num_graphs" in self.__dict__:
            return self._num_graphs
        return int(self.batch[-1]) + 1

    @property
    def num_nodes(self):
        return self.batch.numel()

    def keys(self):
        return [k for k in self.__dict__ if not k.startswith("_")]


class _StoreDesc(ctypes.Structure):  # gt_graph_store (include/graphtrans_hip.h)
    _fields_ = [(k, ctypes.c_void_p) for k in ("node_ptr", "edge_ptr", "x", "node_depth", "edge_src", "edge_dst",
                                                "edge_attr", "attr_rank", "y")] + \
               [("y_row_bytes", ctypes.c_int64), ("num_graphs", ctypes.c_int64), ("x_cols", ctypes.c_int32),
                ("ea_cols", ctypes.c_int32), ("x_f32", ctypes.c_void_p), ("edge_attr_f32", ctypes.c_void_p)]


class _CollateOut(ctypes.Structure):  # gt_collate_out
    _fields_ = [(k, ctypes.c_void_p) for k in ("x", "node_depth", "batch", "ptr", "edge_index", "edge_attr_f32",
                                                "edge_attr_i64", "y", "x_f32")]


HIST_MAX_BINS = 8191   # gt_degree_histogram: (bins + 1) 64-bit counters per block in LDS


def epoch_batches(ids, batch_size, shuffle=False, drop_last=False, rng=None):
    """One epoch of mini-batches over the graph ids `ids` (an int n = range(n), or a split's index array), as
    `DataLoader(dataset[ids], batch_size, shuffle, drop_last)` walks them (main.py:149-152): every id exactly once, in
    permuted order when `shuffle`, the short last batch kept unless `drop_last`.  `rng`: a numpy Generator or a seed
    (None = fresh entropy).  Returns a list of int64 numpy arrays; pure index logic, no GPU.
    The trainer's skip of one-node / one-graph batches (trainers/base_trainer.py:25) is the trainer's business."""
    import numpy as np
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    ids = np.arange(ids, dtype=np.int64) if np.isscalar(ids) else np.array(ids, dtype=np.int64).reshape(-1)
    if shuffle:
        gen = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        ids = ids[gen.permutation(ids.size)]
    end = ids.size - ids.size % batch_size if drop_last else ids.size
    return [ids[i:i + batch_size] for i in range(0, end, batch_size)]


class GraphStore:
    """A whole dataset resident in HBM, mini-batches assembled on the device (`gt_collate`).

    Stands where the reference has `dataset[idx]` + per-sample `augment_edge` (dataset/utils.py:89-141,
    dataset/code.py:97-101) + PyG's DataLoader collation (main.py:149-152): `collate(ids)` returns the
    same `Batch` attributes (x, edge_index, edge_attr, batch, node_depth, y | y_arr) for the graphs `ids`
    in that order.  If the graphs carry `node_is_attributed` the Code2 augmentation is applied
    (edges [ast, ast^-1, next-token, next-token^-1], float (E,2) edge_attr); otherwise edges and
    edge_attr are copied as stored.  Per-graph sizes stay on the host, so sizing a batch costs no sync.

    `x` and `edge_attr` keep their kind: integer arrays are stored as int64 (Code2, Molpcba), float32 arrays as
    float32 (TU datasets: x (N,37) through an nn.Linear node encoder, dataset/tud.py; ER-shaped stores: x (N,256) and
    edge_attr (E,2)) and come back bit for bit.  Any other floating dtype is a TypeError (a silent cast would not be
    bit-exact); graphs that disagree in dtype or column count are a ValueError.

    `batches(...)` walks an epoch as the DataLoader would; `degree_histogram(...)` is the PNA in-degree histogram
    `args.deg` (dataset/code.py:119-132, dataset/mol.py:70-81).
    """

    @staticmethod
    def _features(graphs, key):
        """concatenated rows of `key` as int64 or float32 (see the class docstring)"""
        import numpy as np
        arrs = [np.asarray(g[key]) for g in graphs]
        for a in arrs:
            if a.dtype.kind == "f" and a.dtype != np.float32 or a.dtype.kind not in "iubf":
                raise TypeError(f"GraphStore: {key} must be integer or float32, got {a.dtype} (cast it explicitly)")
        if len({a.dtype.kind == "f" for a in arrs}) > 1:
            raise ValueError(f"GraphStore: graphs disagree in the dtype of {key} (integer and float32)")
        if any(a.ndim != 2 for a in arrs) or len({a.shape[1] for a in arrs}) > 1:
            raise ValueError(f"GraphStore: {key} must be (rows, cols) with the same cols in every graph")
        return np.concatenate(arrs, 0).astype(np.float32 if arrs[0].dtype.kind == "f" else np.int64)

    def __init__(self, graphs, device="cuda", label_key=None):
        import numpy as np
        from . import _lib
        if not torch.cuda.is_available():
            raise RuntimeError("graphtrans_amd.GraphStore lives in GPU memory (no CPU fallback)")
        self._np, self._lib = np, _lib
        dev = torch.device(device)
        g0 = graphs[0]
        self.label_key = label_key or ("y_arr" if "y_arr" in g0 else ("y" if "y" in g0 else None))
        self.nodes = np.array([g["x"].shape[0] for g in graphs], np.int64)
        self.edges = np.array([g["edge_index"].shape[1] for g in graphs], np.int64)
        self.augment = "node_is_attributed" in g0
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        cat = lambda k, ax=0: np.concatenate([np.asarray(g[k]) for g in graphs], ax)  # noqa: E731
        self.node_ptr = up(np.concatenate([[0], np.cumsum(self.nodes)]).astype(np.int64))
        self.edge_ptr = up(np.concatenate([[0], np.cumsum(self.edges)]).astype(np.int64))
        self.x = up(self._features(graphs, "x"))   # int64 or float32
        ei = cat("edge_index", 1).astype(np.int64)
        self.edge_src, self.edge_dst = up(ei[0]), up(ei[1])
        self.node_depth = up(cat("node_depth").reshape(-1).astype(np.int64)) if "node_depth" in g0 else None
        # int64 or float32; an augmenting store writes its own edge_attr and ignores a stored one
        self.edge_attr = up(self._features(graphs, "edge_attr")) if (g0.get("edge_attr") is not None and not self.augment) else None
        self.y = up(cat(self.label_key)) if self.label_key else None
        self.attr_rank = None
        self.out_edges = self.edges
        if self.augment:
            flag = cat("node_is_attributed").reshape(-1).astype(np.int64)
            cnt = np.add.reduceat((flag == 1).astype(np.int64), np.cumsum(self.nodes) - self.nodes) if len(graphs) else flag[:0]
            self.out_edges = 2 * self.edges + 2 * np.maximum(cnt - 1, 0)
            dflag = up(flag)
            self.attr_rank = torch.empty(flag.size + 1, dtype=torch.int64, device=dev)
            _lib.launch("gt_attr_rank", dflag.data_ptr(), flag.size, self.attr_rank.data_ptr(),
                        _stream())
        p = lambda t, dt=None: None if (t is None or (dt is not None and t.dtype != dt)) else t.data_ptr()  # noqa: E731
        self._desc = _StoreDesc(p(self.node_ptr), p(self.edge_ptr), p(self.x, torch.int64), p(self.node_depth), p(self.edge_src),
                                p(self.edge_dst), p(self.edge_attr, torch.int64), p(self.attr_rank), p(self.y),
                                0 if self.y is None else self.y[0].numel() * self.y.element_size(), len(graphs),
                                self.x.shape[1], 0 if self.edge_attr is None else self.edge_attr.shape[1],
                                p(self.x, torch.float32), p(self.edge_attr, torch.float32))
        self.device = dev
        self._deg = None   # in-degree of every store node (gt_store_in_degree), built on the first degree_histogram

    def __len__(self):
        return int(self.nodes.size)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.node_ptr, self.edge_ptr, self.x, self.edge_src, self.edge_dst,
                                                            self.node_depth, self.edge_attr, self.y, self.attr_rank, self._deg)
                   if t is not None)

    def collate(self, ids):
        """ids: host sequence / numpy / CPU tensor of graph indices (a sampler's output)."""
        np = self._np
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= len(self)):
            raise IndexError("graph id out of range")
        B = int(ids.size)
        sizes = self.nodes[ids]
        N, E = int(sizes.sum()), int(self.out_edges[ids].sum())
        dev = self.device
        i64 = dict(dtype=torch.int64, device=dev)
        d_ids = torch.from_numpy(ids).to(dev, non_blocking=True)
        x = torch.empty(N, self.x.shape[1], dtype=self.x.dtype, device=dev)
        batch = torch.empty(N, **i64)
        edge_index = torch.empty(2, E, **i64)
        depth = torch.empty(N, 1, **i64) if self.node_depth is not None else None
        ea_f = ea_i = None
        if self.augment:
            ea_f = torch.empty(E, 2, dtype=torch.float32, device=dev)
        elif self.edge_attr is not None and self.edge_attr.dtype == torch.float32:
            ea_f = torch.empty(E, self.edge_attr.shape[1], dtype=torch.float32, device=dev)
        elif self.edge_attr is not None:
            ea_i = torch.empty(E, self.edge_attr.shape[1], **i64)
        y = torch.empty((B,) + tuple(self.y.shape[1:]), dtype=self.y.dtype, device=dev) if self.y is not None else None
        L = self._lib.lib()
        ws_bytes = L.gt_collate_workspace_bytes(B)
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        xf = x.dtype == torch.float32
        out = _CollateOut(None if xf else p(x), p(depth), p(batch), None, p(edge_index), p(ea_f), p(ea_i), p(y), p(x) if xf else None)
        self._lib.launch("gt_collate", ctypes.byref(self._desc), p(d_ids), B, N, E, ctypes.byref(out), p(ws), ws_bytes,
                         _stream())
        b = Batch(x=x, edge_index=edge_index, batch=batch, edge_attr=ea_f if ea_f is not None else ea_i)
        if depth is not None:
            b.node_depth = depth
        if y is not None:
            setattr(b, self.label_key, y)
        b._num_graphs, b._sizes = B, sizes
        b._graph_ids = d_ids   # evaluate.Code2F1 looks the reference word sets up by these
        return b

    def batches(self, batch_size, ids=None, shuffle=False, drop_last=False, seed=None):
        """One epoch of collated batches over `ids` (default: the whole store; a split's indices otherwise), in the order of
        `epoch_batches`.  Collation is enqueued on the current stream without synchronising."""
        for chunk in epoch_batches(len(self) if ids is None else ids, batch_size, shuffle, drop_last, seed):
            yield self.collate(chunk)

    def degree_histogram(self, ids=None, bins=800):
        """`args.deg` of the PNA models: CPU int64 (bins,), hist[d] = number of nodes with in-degree d among the graphs `ids`
        (None = every graph; an id listed twice counts twice), the in-degree taken over the edges as `collate` emits them
        (the augmented edges on a Code2-shaped store).  Restates dataset/code.py:122-130 (bins 800) and dataset/mol.py:71-79
        (bins 10).  A degree >= bins is a ValueError (the reference fails at `deg += bincount(...)`).  One-off: synchronises."""
        np = self._np
        bins = int(bins)
        if not 1 <= bins <= HIST_MAX_BINS:
            raise ValueError(f"bins must be in 1..{HIST_MAX_BINS}, got {bins}")
        d_ids = None
        B = len(self)
        if ids is not None:
            ids = np.asarray(ids, dtype=np.int64).reshape(-1)
            if ids.size and (ids.min() < 0 or ids.max() >= len(self)):
                raise IndexError("graph id out of range")
            B = int(ids.size)
            d_ids = torch.from_numpy(ids).to(self.device)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        if self._deg is None:
            deg = torch.empty(max(int(self.nodes.sum()), 1), dtype=torch.int32, device=self.device)
            self._lib.launch("gt_store_in_degree", ctypes.byref(self._desc), p(deg), _stream())
            self._deg = deg
        hist = torch.empty(bins + 1, dtype=torch.int64, device=self.device)
        self._lib.launch("gt_degree_histogram", ctypes.byref(self._desc), p(self._deg), p(d_ids), B, bins, p(hist), _stream())
        hist = hist.cpu()
        if int(hist[bins]):
            sel = np.arange(len(self)) if ids is None else np.unique(ids)
            ptr = np.concatenate([[0], np.cumsum(self.nodes)])
            deg = self._deg.cpu().numpy()
            top = max(int(deg[ptr[g]:ptr[g + 1]].max()) for g in sel if self.nodes[g])
            raise ValueError(f"degree_histogram: the largest in-degree is {top}, which needs bins >= {top + 1} (got {bins})")
        return hist[:bins].clone()
