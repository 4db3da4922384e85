"""Exact inputs, a float64 reference and guarded launchers for the GCN / GIN aggregate kernels (csrc/aggregate.hip, csrc/aggregate_wide.h).

Used by tests/test_aggregate_refs_host.py (CPU) and tests/test_hip_aggregate_kernels.py (GPU).  Importable without a GPU.

* EXACT ARITHMETIC.  `h`, `g`, the edge attributes, the Linear weight and bias, the table rows, the dense edge rows and `root` are small
  integers (|h| <= 4, the rest <= 2), GIN's eps is 2, and GCN cases carry THEIR OWN `deg` in {1, 4, 16} with `dis = deg^-0.5` in
  {1, 1/2, 1/4} (the kernels take both as plain inputs).  Every product of the op is then a multiple of 2^-4, and as long as the sum of
  the absolute values of an output's terms stays below 2^24 * 2^-4 every partial sum in ANY order is an fp32 number: the fp32 kernels
  must return the float64 reference bit for bit whatever their summation order or fma contraction.  `assert_representable` checks that
  condition on the reference alone.  bf16 cases store the same integers; the reference rounds its exact `out`, `grad_h` and `d_dense`
  to bf16 once (round to nearest even), parameter gradients stay fp32.
* `ladder_graph`: in- and out-degrees 0..9, 17, 33, one 65 and a hub of min(300, 4 N) on the LAST node, runs of empty rows beside long
  ones, self loops, duplicate edges, an edge order that differs from the CSR order.  CSR / CSC come from oracle.graph_struct (numpy).
* `ref_aggregate(case, flaw)`: the op stated over a list of (owner row, edge, attribute row) triples.  `flaw`, one of FLAWS, restates a
  plausible kernel mistake IN THE REFERENCE ONLY; the host test uses them to show that the cases can tell right from wrong.
* `launch_fwd` / `launch_bwd`: gt_aggregate_fwd / gt_aggregate_bwd through _lib.launch with every output AND the workspace pre-filled
  with NaN, every output between PAD sentinel elements on either side (asserted untouched), no NaN left in an output.
"""
import ctypes as C

import numpy as np
import torch

from oracle.graph_struct import graph_struct

DEV = "cuda:0"
PAD = 64
SENTINEL = 7.0
EPS = 2.0
FLAWS = ("tail_dup_u2", "tail_dup_u4", "tail_drop", "first_trip_stale", "norm_dst", "gate_ge", "gate_on_dst", "attr_by_position",
         "self_loop_skipped", "last_node_skipped", "attr_col_past_K")
CONVS = ("gcn", "gin")
# the ladder: every residue of the kernels' 2- and 4-edge trips, long rows next to runs of empty ones
PATTERN = (0, 0, 33, 0, 1, 2, 0, 17, 3, 0, 0, 4, 9, 5, 0, 6, 7, 8,
           0, 1, 0, 0, 2, 1, 0, 3, 0, 1, 0, 0, 5, 0, 1, 2, 0, 0)   # (a sparse second half: the large cases stay cheap on the host)
CHUNK_ELEMS = 1 << 22   # float64 elements of one temporary of the reference


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(str(k) for k in key))) % (2 ** 31))
    return g


def _ints(shape, g, hi):
    return torch.randint(-hi, hi + 1, shape, generator=g).double()


# ----------------------------------------------------------------------------------------------------------------------------
# graphs
# ----------------------------------------------------------------------------------------------------------------------------
def ladder_degrees(N):
    deg = np.array([PATTERN[i % len(PATTERN)] for i in range(N)], np.int64)
    if 2 <= N < len(PATTERN):
        deg[0] = 1   # a graph too small for the pattern's odd rows still has a one-edge row (never a source: ladder_graph)
    if N >= 4:
        deg[N // 3] = 65
    deg[N - 1] = min(300, 4 * N)
    return deg


def ladder_graph(N, seed):
    """edge_index (2, E) int64.  Node i receives ladder_degrees(N)[i] edges; their sources are drawn from the long rows (degree >= 17) only,
    so that after the reversed edge set is appended every other node has exactly its ladder degree (plus its self loops) in BOTH
    directions and the empty rows stay empty.  Every 7th edge is a self loop, duplicates are allowed, the edge list is shuffled."""
    rng = np.random.default_rng(seed)
    deg = ladder_degrees(N)
    pool = np.flatnonzero(deg >= 17)
    if pool.size == 0:
        pool = np.array([N - 1])
    dst = np.repeat(np.arange(N, dtype=np.int64), deg)
    src = pool[rng.integers(0, pool.size, dst.size)]
    loops = np.arange(dst.size) % 7 == 6
    src[loops] = dst[loops]
    ei = np.stack([np.concatenate([src, dst]), np.concatenate([dst, src])])
    return ei[:, rng.permutation(ei.shape[1])].copy()


def self_loops(N, count):
    """`count` self loops on node N - 1 and nothing else (the N = 1 variant with edges)"""
    return np.full((2, count), N - 1, np.int64)


def no_edges():
    return np.zeros((2, 0), np.int64)


# ----------------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------------
class Case:
    """One call: conv in CONVS, mode in {none, linear, tables, dense}, K attribute columns, table row counts `rows` (one per column), a
    graph, and CPU float64 / int64 inputs.  Everything is drawn from a generator seeded by the case's name."""

    def __init__(self, conv, mode, N, D, ei, dtype=torch.float32, K=0, rows=(), integer=True, deg=None, name=None):
        assert conv in CONVS and mode in ("none", "linear", "tables", "dense") and D % 4 == 0
        assert (mode == "linear" and 1 <= K <= 4) or (mode == "tables" and len(rows) == K and 1 <= K <= 4) or (mode in ("none", "dense") and K == 0)
        self.conv, self.mode, self.N, self.D, self.K, self.dtype, self.integer = conv, mode, int(N), int(D), int(K), dtype, integer
        self.ei = np.ascontiguousarray(ei, np.int64)
        self.E = E = int(self.ei.shape[1])
        self.name = name or f"{conv}-{mode}{K or ''}{'x'.join(str(r) for r in rows)}-N{N}-D{D}-E{E}-{str(dtype)[6:]}"
        gs = graph_struct(self.ei, np.zeros(N, np.int64), num_nodes=N, num_graphs=1)
        self.gs = gs
        self.src, self.dst = torch.from_numpy(self.ei[0]), torch.from_numpy(self.ei[1])
        g = _gen(self.name)
        # d_eps sums |g h| over N D terms and the Linear gradients |t a| over E: smaller values where that would pass 2^24 (2^20 for
        # the latter, in units of 2^-4), checked by assert_representable
        big, long = N * D > (1 << 22), E > (1 << 19)
        if integer:
            self.h, self.g = _ints((N, D), g, 2 if big else 4), _ints((N, D), g, 1 if big or long else 2)
            if long:
                self.g *= torch.randint(0, 2, (N, D), generator=g).double()
            self.h[N - 1, 0], self.g[N - 1, 0] = 3.0, 1.0   # the last node's rows are never all zero (last_node_skipped)
            self.root = _ints((D,), g, 2)
            self.root[0] = 1.0
            self.eps = EPS
            self.deg = torch.tensor([1.0, 4.0, 16.0], dtype=torch.float64)[torch.randint(0, 3, (N,), generator=g)]
        else:
            # Real-valued cases (compared with a tolerance): normal values, but everything a relu gate reads sits on a grid -- h and the
            # dense rows on 1/64, attributes / weights / bias / tables / root on 1/8 -- so that h + e is exact in fp32 and in float64 and
            # no gate depends on rounding (one flipped gate moves a gradient element by O(1), in any fp32 evaluation).  g, the
            # graph's deg^-1/2 norms and eps are not dyadic: the sums are rounded, in an order the kernel chooses.
            grid = lambda shape, q: (torch.randn(shape, generator=g, dtype=torch.float64) * q).round() / q
            self.h, self.g = grid((N, D), 64), torch.randn(N, D, generator=g, dtype=torch.float64)
            self.root, self.eps = grid((D,), 8), 0.37
            self.deg = torch.as_tensor(deg, dtype=torch.float64)
        self.dis = self.deg.pow(-0.5)
        draw = (lambda shape: _ints(shape, g, 2)) if integer else (lambda shape: grid(shape, 64 if mode == "dense" else 8))
        self.attr = self.w = self.b = self.tables = self.dense = None
        self.tab_off, self.table_rows = (), 0
        if mode == "linear":
            self.attr, self.w, self.b = draw((E, K)), draw((D, K)), draw((D,))
        elif mode == "tables":
            self.table_rows = int(sum(rows))
            self.tab_off = tuple(int(v) for v in np.concatenate([[0], np.cumsum(rows)[:-1]]))
            self.attr = torch.stack([torch.randint(0, r, (E,), generator=g) for r in rows], dim=1) if E else torch.zeros(0, K, dtype=torch.int64)
            self.tables = draw((self.table_rows, D))
        elif mode == "dense":
            self.dense = draw((E, D))
        self._dev = None

    # the storage type's view of the inputs (integers are exact in both; real-valued bf16 cases are rounded ONCE, here, and the
    # reference then works on what the kernel reads)
    def quantised(self):
        if self.dtype == torch.float64 or (self.dtype == torch.float32 and self.integer):
            return self   # (float64: no kernel reads it; the host test's comparison with the oracle)
        q = object.__new__(Case)
        q.__dict__.update(self.__dict__)
        rt = lambda t, dt: None if t is None else t.to(dt).double()
        q.h, q.g, q.dense = rt(self.h, self.dtype), rt(self.g, self.dtype), rt(self.dense, self.dtype)
        q.root, q.w, q.b, q.tables = (rt(t, torch.float32) for t in (self.root, self.w, self.b, self.tables))
        q.deg, q.dis = rt(self.deg, torch.float32), rt(self.dis, torch.float32)
        q.eps = float(torch.tensor(self.eps, dtype=torch.float32))
        if self.mode == "linear":
            q.attr = rt(self.attr, torch.float32)
        return q

    def dev(self):
        """device copies in the C entry points' types, uploaded once"""
        if self._dev is None:
            i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32) if len(a) else np.zeros(1, np.int32)).to(DEV)
            f32 = lambda t: None if t is None else t.float().contiguous().to(DEV)
            st = lambda t: None if t is None else t.to(self.dtype).contiguous().to(DEV)
            gs = self.gs
            d = dict(h=st(self.h), g=st(self.g), in_ptr=i32(gs["in_ptr"]), in_src=i32(gs["in_src"]), in_eid=i32(gs["in_eid"]),
                     out_ptr=i32(gs["out_ptr"]), out_dst=i32(gs["out_dst"]), out_eid=i32(gs["out_eid"]), deg=f32(self.deg), dis=f32(self.dis),
                     self_param=f32(self.root if self.conv == "gcn" else torch.tensor([self.eps], dtype=torch.float64)),
                     w=f32(self.w if self.mode == "linear" else self.tables), b=f32(self.b), dense=st(self.dense))
            d["attr"] = None if self.attr is None else (self.attr.float() if self.mode == "linear" else self.attr.long()).contiguous().to(DEV)
            if d["attr"] is not None and d["attr"].numel() == 0:
                d["attr"] = torch.zeros(1, max(self.K, 1), dtype=d["attr"].dtype, device=DEV)
            if d["dense"] is not None and d["dense"].numel() == 0:
                d["dense"] = torch.zeros(1, self.D, dtype=self.dtype, device=DEV)
            self._dev = d
        return self._dev


# ----------------------------------------------------------------------------------------------------------------------------
# reference
# ----------------------------------------------------------------------------------------------------------------------------
def _slots(ptr, eid, N, flaw, loop_mask):
    """The (owner row, edge, attribute row) triples one direction sums over: position q of the CSR / CSC row i gives (i, eid[q], eid[q]).
    The structural flaws change the list, nothing else."""
    ptr, eid = np.asarray(ptr, np.int64), np.asarray(eid, np.int64)
    deg = np.diff(ptr)
    owner = np.repeat(np.arange(N, dtype=np.int64), deg)
    pos = np.arange(eid.size, dtype=np.int64)
    k, ka = eid.copy(), eid.copy()
    last = ptr[1:] - 1   # position of a row's last edge (rows with deg > 0)
    if flaw in ("tail_dup_u2", "tail_dup_u4"):
        U = int(flaw[-1])
        rows = np.flatnonzero((deg > 0) & (deg % U != 0))
        owner, k, ka = np.concatenate([owner, rows]), np.concatenate([k, eid[last[rows]]]), np.concatenate([ka, eid[last[rows]]])
    elif flaw == "tail_drop":
        rows = np.flatnonzero(deg % 2 == 1)
        keep = np.ones(eid.size, bool)
        keep[last[rows]] = False
        owner, k, ka = owner[keep], k[keep], ka[keep]
    elif flaw == "first_trip_stale":
        full = np.flatnonzero(deg > 0)
        prev, cur = full[:-1], full[1:]
        for u in range(2):
            has = deg[cur] > u
            q = np.minimum(ptr[prev] + u, ptr[prev + 1] - 1)[has]
            k[ptr[cur][has] + u] = ka[ptr[cur][has] + u] = eid[q]
    elif flaw == "attr_by_position":
        ka = pos
    elif flaw == "self_loop_skipped":
        keep = ~loop_mask[k]
        owner, k, ka = owner[keep], k[keep], ka[keep]
    elif flaw == "last_node_skipped":
        keep = owner != N - 1
        owner, k, ka = owner[keep], k[keep], ka[keep]
    return torch.from_numpy(owner), torch.from_numpy(k), torch.from_numpy(ka)


def _embed(c, ka, flaw):
    """e of the attribute rows ka: [len(ka)][D] float64, or None"""
    if c.mode == "none":
        return None
    if c.mode == "linear":
        e = torch.addmm(c.b, c.attr[ka], c.w.t())
        if flaw == "attr_col_past_K" and c.K < 4:
            e = e + c.attr[ka, 0:1]   # a phantom weight column of ones that reads attribute column 0
        return e
    if c.mode == "tables":
        return sum(c.tables[c.tab_off[j] + c.attr[ka, j]] for j in range(c.K))
    return c.dense[ka]


def _weight(c, owner, other, flaw):
    if c.conv != "gcn":
        return None
    return (c.dis[owner] * (c.dis[owner] if flaw == "norm_dst" else c.dis[other])).unsqueeze(1)


def _chunks(n, D):
    step = max(1, CHUNK_ELEMS // max(D, 1))
    return [(a, min(n, a + step)) for a in range(0, n, step)]


def ref_forward(case, flaw=None, with_abs=False):
    """out [N][D] float64 (and the sum of the absolute values of each element's terms)"""
    c = case.quantised()
    N, D = c.N, c.D
    owner, k, ka = _slots(c.gs["in_ptr"], c.gs["in_eid"], N, flaw, (c.src == c.dst).numpy())
    if c.conv == "gcn":
        out = torch.relu(c.h + c.root) / c.deg.unsqueeze(1)
    else:
        out = (1.0 + c.eps) * c.h
    ab = out.abs() if with_abs else None
    for a, b in _chunks(owner.numel(), D):
        o, kk = owner[a:b], k[a:b]
        other = c.src[kk]
        m = c.h[other]
        e = _embed(c, ka[a:b], flaw)
        if e is not None:
            m = m + e
        m = torch.relu_(m)
        wgt = _weight(c, o, other, flaw)
        if wgt is not None:
            m *= wgt
        out.index_add_(0, o, m)
        if with_abs:
            ab.index_add_(0, o, m)   # the terms are >= 0
    if flaw == "last_node_skipped":
        out[N - 1] = 0.0
    return (out, ab) if with_abs else out


def ref_backward(case, flaw=None, with_abs=False):
    """dict of float64 gradients: grad_h [N][D], d_self (GCN: [D]; GIN: the scalar d_eps as [1]), d_edge_w / d_edge_b (Linear: [D][K], [D];
    tables: [rows][D]), d_dense [E][D]; with_abs adds `<name>_abs` for each."""
    c = case.quantised()
    N, D = c.N, c.D
    owner, k, ka = _slots(c.gs["out_ptr"], c.gs["out_eid"], N, flaw, (c.src == c.dst).numpy())
    skip = flaw == "last_node_skipped"
    live = torch.ones(N, 1, dtype=torch.float64)
    if skip:
        live[N - 1] = 0.0
    r = {}
    if c.conv == "gcn":
        s = (c.h + c.root > 0).double() * c.g / c.deg.unsqueeze(1) * live
        r["grad_h"], r["d_self"] = s.clone(), s.sum(0)
        ab = {"grad_h": s.abs(), "d_self": s.abs().sum(0)}
    else:
        r["grad_h"], r["d_self"] = (1.0 + c.eps) * c.g * live, (c.g * c.h * live).sum().reshape(1)
        ab = {"grad_h": r["grad_h"].abs(), "d_self": (c.g * c.h * live).abs().sum().reshape(1)}
    if c.mode == "linear":
        r["d_edge_w"], r["d_edge_b"] = torch.zeros(D, c.K, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)
    elif c.mode == "tables":
        r["d_edge_w"] = torch.zeros(c.table_rows, D, dtype=torch.float64)
    elif c.mode == "dense":
        r["d_dense"] = torch.zeros(c.E, D, dtype=torch.float64)
    for name in list(r):
        if name not in ab:
            ab[name] = torch.zeros_like(r[name])
    ge = flaw == "gate_ge"
    for a, b in _chunks(owner.numel(), D):
        o, kk, kka = owner[a:b], k[a:b], ka[a:b]
        other = c.dst[kk]
        pre = c.h[other if flaw == "gate_on_dst" else o]
        e = _embed(c, kka, flaw)
        if e is not None:
            pre = pre + e
        t = c.g[other] * ((pre >= 0) if ge else (pre > 0)).double()
        wgt = _weight(c, o, other, flaw)
        if wgt is not None:
            t *= wgt
        r["grad_h"].index_add_(0, o, t)
        at = t.abs() if with_abs else None
        if with_abs:
            ab["grad_h"].index_add_(0, o, at)
        if c.mode == "linear":
            att = c.attr[kka]
            r["d_edge_w"] += t.t() @ att
            r["d_edge_b"] += t.sum(0)
            if with_abs:
                ab["d_edge_w"] += at.t() @ att.abs()
                ab["d_edge_b"] += at.sum(0)
        elif c.mode == "tables":
            for j in range(c.K):
                idx = c.tab_off[j] + c.attr[kka, j]
                r["d_edge_w"].index_add_(0, idx, t)
                if with_abs:
                    ab["d_edge_w"].index_add_(0, idx, at)
        elif c.mode == "dense":
            r["d_dense"][kka] = t   # one term each; the flawed lists may write a row twice or not at all
            if with_abs:
                ab["d_dense"][kka] = at
    if skip:
        r["grad_h"][N - 1] = 0.0
    if with_abs:
        r.update({n + "_abs": v for n, v in ab.items()})
    return r


def ref_aggregate(case, flaw=None, with_abs=False):
    """forward and backward of one case: dict with `out` and ref_backward's entries"""
    assert flaw is None or flaw in FLAWS, flaw
    r = ref_backward(case, flaw, with_abs)
    if with_abs:
        r["out"], r["out_abs"] = ref_forward(case, flaw, True)
    else:
        r["out"] = ref_forward(case, flaw)
    return r


OUTPUTS = ("out", "grad_h", "d_self", "d_edge_w", "d_edge_b", "d_dense")
STORED = ("out", "grad_h", "d_dense")   # in the storage type; the rest are fp32 parameter gradients


def assert_representable(case, ref):
    """The condition under which an fp32 evaluation in any order equals `ref` (made with with_abs=True): every term is a multiple of 2^-4
    (of 1 for GIN's d_eps, a sum of integer products) and the absolute sum of an output's terms, in units of that granularity, is
    below 2^24; and the float64 values survive a round trip through fp32."""
    assert case.integer
    for name in OUTPUTS:
        if name not in ref:
            continue
        v, a = ref[name], ref[name + "_abs"]
        gran = 1.0 if (name == "d_self" and case.conv == "gin") else 16.0
        top = float(a.max()) if a.numel() else 0.0
        assert top * gran < 2 ** 24, f"{case.name}: {name} abs-sum {top} x {gran}"
        assert torch.equal(v * gran, (v * gran).round()), f"{case.name}: {name} is not a multiple of 1/{gran}"
        assert torch.equal(v.float().double(), v), f"{case.name}: {name} does not survive fp32"


def expected(case, ref):
    """what the kernel must return, bit for bit: the exact values in fp32, `out` / `grad_h` / `d_dense` rounded once to the storage type"""
    return {n: (ref[n].float().to(case.dtype) if n in STORED else ref[n].float()) for n in OUTPUTS if n in ref}


def same(a, b):
    """every output equal by value"""
    return all(torch.equal(a[n], b[n]) for n in OUTPUTS if n in a)


def flaw_applies(case, flaw):
    """Whether this case can show the flaw at all, from its inputs alone."""
    c, gs = case, case.gs
    din, dout = gs["deg_in"], gs["deg_out"]
    E = c.E
    if flaw in ("tail_dup_u2", "tail_dup_u4"):
        U = int(flaw[-1])
        return bool(((din % U != 0) | (dout % U != 0)).any())
    if flaw == "tail_drop":
        return bool(((din % 2 == 1) | (dout % 2 == 1)).any())
    if flaw == "first_trip_stale":   # some stale edge must differ from the row's own in its far end or, with attributes, in its id
        loops = (c.src == c.dst).numpy()
        for ptr, eid, far in ((gs["in_ptr"], gs["in_eid"], c.src), (gs["out_ptr"], gs["out_eid"], c.dst)):
            _, k0, _ = _slots(ptr, eid, c.N, None, loops)
            _, k1, _ = _slots(ptr, eid, c.N, flaw, loops)
            if bool((far[k0] != far[k1]).any()) or (c.mode != "none" and bool((k0 != k1).any())):
                return True
        return False
    if flaw == "norm_dst":
        return c.conv == "gcn" and bool((c.dis[c.src] != c.dis[c.dst]).any())
    if flaw in ("gate_ge", "gate_on_dst"):   # some gate of an edge with a non-zero upstream gradient must change
        q = c.quantised()
        for a, b in _chunks(E, c.D):
            ka = torch.arange(a, b)
            e = _embed(q, ka, None)
            pre = q.h[q.src[a:b]] + (0.0 if e is None else e)
            other = (pre == 0) if flaw == "gate_ge" else ((q.h[q.dst[a:b]] + (0.0 if e is None else e) > 0) != (pre > 0))
            if bool((other & (q.g[q.dst[a:b]] != 0)).any()):
                return True
        return False
    if flaw == "attr_by_position":   # some edge id differs from its CSR / CSC position
        pos = np.arange(E)
        return c.mode != "none" and bool((gs["in_eid"] != pos).any() or (gs["out_eid"] != pos).any())
    if flaw == "self_loop_skipped":
        return bool((c.src == c.dst).any())
    if flaw == "last_node_skipped":
        return True
    if flaw == "attr_col_past_K":
        return c.mode == "linear" and c.K < 4 and E > 0
    raise KeyError(flaw)


# ----------------------------------------------------------------------------------------------------------------------------
# launchers
# ----------------------------------------------------------------------------------------------------------------------------
class _Guarded:
    """n elements pre-filled with NaN between PAD sentinel elements on either side"""

    def __init__(self, shape, dtype):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
        self.buf[PAD:PAD + self.n] = float("nan")
        assert (self.buf.data_ptr() + PAD * self.buf.element_size()) % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + PAD * self.buf.element_size()

    def body(self):
        return self.buf[PAD:PAD + self.n].reshape(self.shape)

    def take(self, what, written=True):
        assert bool((self.buf[:PAD] == SENTINEL).all()), f"{what}: the kernel wrote before the start of its output"
        assert bool((self.buf[PAD + self.n:] == SENTINEL).all()), f"{what}: the kernel wrote past the end of its output"
        out = self.body()
        if written:
            assert not bool(torch.isnan(out).any()), f"{what}: {int(torch.isnan(out).sum())} elements were never written"
        else:
            assert bool(torch.isnan(out).all()), f"{what}: written by a call that was refused"
        return out


def _codes(case):
    from graphtrans_amd import _lib
    conv = _lib.GT_CONV_GCN if case.conv == "gcn" else _lib.GT_CONV_GIN
    mode = {"none": _lib.GT_EDGE_NONE, "linear": _lib.GT_EDGE_LINEAR, "tables": _lib.GT_EDGE_TABLES, "dense": _lib.GT_EDGE_DENSE}[case.mode]
    return conv, mode, (_lib.GT_F32 if case.dtype == torch.float32 else _lib.GT_BF16)


def _check_inputs(case, d):
    """host-side bounds of everything the kernels index with: a slip in a test is a Python assertion, not a GPU fault"""
    N, E, D = case.N, case.E, case.D
    gs = case.gs
    for ptr, nbr, eid in (("in_ptr", "in_src", "in_eid"), ("out_ptr", "out_dst", "out_eid")):
        p = np.asarray(gs[ptr])
        assert p.shape == (N + 1,) and p[0] == 0 and p[-1] == E and (np.diff(p) >= 0).all()
        assert d[ptr].numel() == N + 1 and d[nbr].numel() >= max(E, 1) and d[eid].numel() >= max(E, 1)
        if E:
            assert 0 <= gs[nbr].min() and gs[nbr].max() < N and 0 <= gs[eid].min() and gs[eid].max() < E
    assert d["h"].shape == (N, D) and d["g"].shape == (N, D) and d["deg"].numel() == N and d["dis"].numel() == N
    assert d["self_param"].numel() == (D if case.conv == "gcn" else 1)
    if case.mode == "linear":
        assert d["attr"].dtype == torch.float32 and d["attr"].numel() >= E * case.K and d["w"].shape == (D, case.K) and d["b"].shape == (D,)
    elif case.mode == "tables":
        assert d["attr"].dtype == torch.int64 and d["w"].shape == (case.table_rows, D)
        for j in range(case.K):
            hi = (case.tab_off[j + 1] if j + 1 < case.K else case.table_rows) - case.tab_off[j]
            assert E == 0 or (0 <= int(case.attr[:, j].min()) and int(case.attr[:, j].max()) < hi)
    elif case.mode == "dense":
        assert d["dense"].numel() >= E * D
    for t in d.values():
        assert t is None or (t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0)


def _toff(case):
    return (C.c_int32 * max(len(case.tab_off), 1))(*case.tab_off) if case.mode == "tables" else None


def _p(t):
    return None if t is None else t.data_ptr()


def launch_fwd(case):
    """gt_aggregate_fwd on the case's inputs: out [N][D] in the storage type"""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    d = case.dev()
    _check_inputs(case, d)
    conv, mode, dt = _codes(case)
    out = _Guarded((case.N, case.D), case.dtype)
    _lib.launch("gt_aggregate_fwd", conv, mode, dt, _p(d["h"]), case.N, case.E, case.D, _p(d["in_ptr"]), _p(d["in_src"]), _p(d["in_eid"]),
                _p(d["deg"]), _p(d["dis"]), _p(d["self_param"]), _p(d["attr"]), case.K, _p(d["w"]), _p(d["b"]), _toff(case),
                case.table_rows, _p(d["dense"]), out.ptr, _stream())
    torch.cuda.synchronize()
    return out.take("out").cpu()


def launch_bwd(case, expect_status=0):
    """gt_aggregate_bwd on the case's inputs: dict of CPU tensors named as ref_backward's (d_self: [D] for GCN, [1] for GIN).
    With a non-zero expect_status: asserts that status, that no output and no workspace element was written, and returns the message."""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    d = case.dev()
    _check_inputs(case, d)
    conv, mode, dt = _codes(case)
    N, E, D, K = case.N, case.E, case.D, case.K
    f32 = torch.float32
    bufs = {"grad_h": _Guarded((N, D), case.dtype), "d_self": _Guarded((D if case.conv == "gcn" else 1 + (D + 63) // 64,), f32)}
    if case.mode == "linear":
        bufs["d_edge_w"], bufs["d_edge_b"] = _Guarded((D, K), f32), _Guarded((D,), f32)
    elif case.mode == "tables":
        bufs["d_edge_w"] = _Guarded((case.table_rows, D), f32)
    elif case.mode == "dense":
        bufs["d_dense"] = _Guarded((E, D), case.dtype)
    L = _lib.lib()
    ws_bytes = int(L.gt_aggregate_bwd_workspace_bytes(conv, mode, D, K, case.table_rows))
    ws = torch.full(((ws_bytes + 3) // 4,), float("nan"), dtype=f32, device=DEV)
    ptr = lambda n: bufs[n].ptr if n in bufs else None
    args = (conv, mode, dt, _p(d["h"]), _p(d["g"]), N, E, D, _p(d["out_ptr"]), _p(d["out_dst"]), _p(d["out_eid"]), _p(d["deg"]), _p(d["dis"]),
            _p(d["self_param"]), _p(d["attr"]), K, _p(d["w"]), _p(d["b"]), _toff(case), case.table_rows, _p(d["dense"]), ptr("grad_h"),
            ptr("d_self"), ptr("d_edge_w"), ptr("d_edge_b"), ptr("d_dense"), ws.data_ptr(), ws.numel() * 4, _stream())
    if expect_status:
        rc = L.gt_aggregate_bwd(*args)
        torch.cuda.synchronize()
        assert rc == expect_status, f"status {rc}, expected {expect_status}"
        for n, b in bufs.items():
            b.take(n, written=False)
        assert bool(torch.isnan(ws).all()), "the workspace was written by a call that was refused"
        return L.gt_last_error().decode(errors="replace")
    _lib.launch("gt_aggregate_bwd", *args)
    torch.cuda.synchronize()
    res = {n: b.take(n).cpu() for n, b in bufs.items()}
    if case.conv == "gin":
        res["d_self"] = res["d_self"][:1]   # d_eps; the rest are k_agg_reduce's column-tile sums
    return res


# ----------------------------------------------------------------------------------------------------------------------------
# the case table of tests/test_hip_aggregate_kernels.py (walked by tests/test_aggregate_refs_host.py too)
# ----------------------------------------------------------------------------------------------------------------------------
F32, BF16 = torch.float32, torch.bfloat16
# D -> instantiation, from launch_cfg / wide_w of csrc/aggregate.hip.  fp32 rows of 193..448 columns with D % ceil(D / 64) == 0 take
# k_aggw_* with W = ceil(D / 64) floats per lane; everything else k_agg_* with (lanes per node, float4 chunks per lane):
#   D <= 64 (16, 1) | <= 128 (32, 1) | <= 256 (64, 1) | <= 512 (64, 2) | <= 768 (64, 3) | <= 1024 (64, 4)
#   fp32:   8, 36, 64 -> (16,1)   68, 128 -> (32,1)   132, 192 -> (64,1)   264, 512 -> (64,2) [264: 264 % 5 != 0, not wide]
#           516, 768 -> (64,3)    772, 1024 -> (64,4)
#           196 -> W 4 (49 live lanes)   256 -> W 4   260 -> W 5 (52 lanes)   300 -> W 5 (60)   320 -> W 5
#           324 -> W 6 (54 lanes)   384 -> W 6   392 -> W 7 (56 lanes)   448 -> W 7
#   bf16 (never wide):  8, 36, 64 -> (16,1)   68, 128 -> (32,1)   132, 256 -> (64,1)   300 -> (64,2)   516 -> (64,3)   1024 -> (64,4)
# Each instantiation exists per edge variant: none, Linear K <= 2 (EDGE_LINEAR2), Linear K = 3, 4 (GT_EDGE_LINEAR), tables, dense; the
# wide kernels also per conv.
SWEEP_D = {F32: (8, 36, 64, 68, 128, 132, 192, 264, 512, 516, 768, 772, 1024, 196, 256, 260, 300, 320, 324, 384, 392, 448),
           BF16: (8, 36, 64, 68, 128, 132, 256, 300, 516, 1024)}
SWEEP_N = 67
BWD_LDS_ROWS_X_DIM = 8192   # gt_aggregate_bwd: table rows x D x 20 bytes <= 160 KiB


def sweep_rows(D):
    """table row counts of the sweep's K = 1 and K = 4 cases: a single-row table among them, total rows x D <= the backward's LDS limit"""
    budget = min(BWD_LDS_ROWS_X_DIM // D, 12)   # 8 at D = 1024
    assert budget >= 8
    return (min(budget, 5),), (1, 2, 3, budget - 6)


def sweep_modes(D):
    r1, r4 = sweep_rows(D)
    return [("none", 0, ()), ("linear", 1, ()), ("linear", 2, ()), ("linear", 3, ()), ("linear", 4, ()), ("tables", 1, r1), ("tables", 4, r4),
            ("dense", 0, ())]


_GRAPHS = {}


def graph(N, kind="ladder"):
    key = (N, kind)
    if key not in _GRAPHS:
        _GRAPHS[key] = {"ladder": lambda: ladder_graph(N, 1000 + N), "none": no_edges, "loops3": lambda: self_loops(N, 3)}[kind]()
    return _GRAPHS[key]


class Spec:
    """a case of the table, built on demand; fwd / bwd: which directions the GPU test launches"""

    def __init__(self, group, conv, mode, N, D, dtype, K=0, rows=(), kind="ladder", fwd=True, bwd=True):
        self.group, self.args, self.kind, self.fwd, self.bwd = group, (conv, mode, N, D, dtype, K, tuple(rows)), kind, fwd, bwd
        self.id = f"{group}-{conv}-{mode}{K or ''}{'r%d' % sum(rows) if rows else ''}-N{N}-D{D}-{kind}-{str(dtype)[6:]}"

    def make(self):
        conv, mode, N, D, dtype, K, rows = self.args
        return Case(conv, mode, N, D, graph(N, self.kind), dtype=dtype, K=K, rows=rows, name=self.id)


def sweep_specs(dtype, D):
    return [Spec("sweep", conv, mode, SWEEP_N, D, dtype, K, rows) for conv in CONVS for mode, K, rows in sweep_modes(D)]


# forward walk lengths: chunk = N / (4096 x nodes per wave) = 3, 3, 2, 8, 8, the last wave-tile cut short mid-walk
WALKS = ((8, 3 * 16384 + 5), (132, 3 * 4096 + 1), (196, 2 * 4096 + 3), (16, 8 * 16384 + 7), (300, 8 * 4096 + 2))


def fwd_chunk(D, N):
    """a.chunk of gt_aggregate_fwd"""
    return max(1, min(8, N // (4096 * (4 if D <= 64 else (2 if D <= 128 else 1)))))


def walk_specs(D, N, dtype):
    return [Spec("walk", conv, mode, N, D, dtype, K) for conv in CONVS for mode, K in (("linear", 2), ("none", 0))]


WALK_PARAMS = [(D, N, F32) for D, N in WALKS] + [(D, N, BF16) for D, N in WALKS[:2]]
SMALL_D = (8, 132, 300)


def small_specs(D):
    out = []
    for conv in CONVS:
        for mode, K in (("none", 0), ("linear", 2)):
            out += [Spec("small", conv, mode, N, D, F32, K, kind="none" if N == 1 else "ladder") for N in (1, 2, 3, 5, 9)]
            out += [Spec("small", conv, mode, 1, D, F32, K, kind="loops3"), Spec("small", conv, mode, 37, D, F32, K, kind="none")]
    return out


REDUCE_PARAMS = [(N, D) for D in (132, 300) for N in (5, 100, 1000, 4001)]


def reduce_specs(N, D):
    return [Spec("reduce", conv, mode, N, D, F32, K, rows) for conv in CONVS for mode, K, rows in (("linear", 4, ()), ("tables", 3, (4, 1, 6)))]


def table_limit_specs():
    """forward: 200 rows x 64 x 4 bytes > 48 KiB, not staged in LDS (its backward is over the limit: not launched);
    backward: 64 rows x 128 x 20 bytes == 160 KiB exactly; 65 rows: refused"""
    return ([Spec("tables", conv, "tables", SWEEP_N, 64, F32, 2, (100, 100), bwd=False) for conv in CONVS]
            + [Spec("tables", conv, "tables", SWEEP_N, 128, F32, 4, (16, 16, 16, 16)) for conv in CONVS])


def table_refused_spec():
    return Spec("tables", "gcn", "tables", SWEEP_N, 128, F32, 4, (16, 16, 16, 17), fwd=False, bwd=False)


def all_spec_groups():
    """[(id, [Spec])] of the whole table, grouped as the GPU tests are parametrised"""
    groups = [(f"sweep-{str(dt)[6:]}-D{D}", sweep_specs(dt, D)) for dt in (F32, BF16) for D in SWEEP_D[dt]]
    groups += [(f"walk-{str(dt)[6:]}-D{D}-N{N}", walk_specs(D, N, dt)) for D, N, dt in WALK_PARAMS]
    groups += [(f"small-D{D}", small_specs(D)) for D in SMALL_D]
    groups += [(f"reduce-N{N}-D{D}", reduce_specs(N, D)) for N, D in REDUCE_PARAMS]
    groups += [("tables", table_limit_specs() + [table_refused_spec()])]
    return groups
