"""Plain references, shared inputs and guarded launchers for the small kernels of csrc/util.hip and csrc/segment.hip.

Three parts, used by tests/test_kernel_refs_host.py (CPU), tests/test_hip_row_kernels.py and tests/test_hip_segment_kernels.py (GPU):

* `ref_*`: each operation stated in a few lines of numpy / CPU torch from the contract comments of the two files (not from the kernels'
  loops).  The token references take an optional `flaw`, one of FLAWS: a deliberately wrong variant, used ONLY by the host tests to show
  that the inputs below can tell the right statement from a wrong one.
* the input sets of the token, segment, column-sum and row-move tests: BATCHES, MAX_LENS, `seq_case` / `seq_data`, `segment_data`,
  `colsum_data`, `rows_data`, `rows_add_data`, `scatter_grad`.  The GPU tests of those kernels take their inputs from here, so the host
  tests can walk the same sets and show that they tell right from wrong.  (The remaining GPU tests -- copy2d, repitch, gather_f32, add3,
  dropout, the grid-cap cases, the identity map and gt_seq_layout_packed -- build theirs locally, beside the assertion; the references
  have no wrong variant for those.)
* `launch_*`: one launcher per entry point.  Before `_lib.launch` it asserts on the host that every tensor is on the device,
  contiguous, of the C signature's type and large enough for these arguments, that every index array stays inside what it
  indexes, and (`_call`) that the arguments are the C prototype's, by name and in its order, each of the kind the ctypes signature
  takes: a slip in a test is a Python assertion, not a GPU fault.  Outputs live in buffers allocated PAD elements larger than
  needed, pre-filled with SENTINEL; the launcher asserts that the tail survived and returns the needed part.

Layouts of both kinds come from test_model_driver_host.numpy_layout, the suite's one layout oracle.
"""
import numpy as np
import torch

from test_model_driver_host import numpy_layout

DEV = "cuda:0"
GT_F32, GT_BF16 = 0, 1
DTYPES = {GT_F32: torch.float32, GT_BF16: torch.bfloat16}
SENTINEL = 7.0
PAD = 64

# ----------------------------------------------------------------------------------------------------------------------------
# input sets
# ----------------------------------------------------------------------------------------------------------------------------
BATCHES = {
    "tiny": (9, 1, 17, 6),
    "edges": (1, 3, 4, 5, 31, 32, 33, 36, 64, 65, 130),   # the 4-wave stride, the 32-row unroll of k_segment_sum, 64-position tiles
    "with_empty": (0, 0, 5, 0, 70, 0),                   # segment ops only: a token layout needs >= 1 node per graph
}
SEQ_BATCHES = ("tiny", "edges")
MAX_LENS = (1000, 8, 1)     # no, some and almost all nodes dropped
KINDS = ("packed", "padded")
SEQ_DIMS = (8, 300, 4096)
FLAWS = ("keep_first", "node0_off_by_one", "stride_swapped", "cls_at_kept_minus_1")


def _gen(*key):
    """a CPU generator seeded by the case's name"""
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(str(k) for k in key))) % (2 ** 31))
    return g


def ints(shape, g, lo=-8, hi=8):
    """integer-valued fp32 in [lo, hi]: exact in bf16, and every partial sum of a few thousand of them is exact in fp32"""
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def graph_arrays(sizes):
    """(graph_ptr int32 [B+1], node_graph int32 [N]) of a batch of graph sizes"""
    n = np.asarray(sizes, np.int64)
    gptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    return gptr, np.repeat(np.arange(n.size, dtype=np.int32), n)


def seq_case(batch, kind, max_len, with_cls):
    """the layout of one token case, from numpy_layout: a dict of plain numpy arrays and ints"""
    sizes = BATCHES[batch]
    (rows, max_npos, _, S, row_stride), desc, last_rows, _ = numpy_layout(sizes, kind, max_len, with_cls)
    gptr, ng = graph_arrays(sizes)
    return dict(name=f"{batch}-{kind}-max{max_len}-cls{with_cls}", sizes=np.asarray(sizes, np.int64), B=len(sizes), N=int(gptr[-1]), S=S,
                rows=int(rows), max_npos=int(max_npos), row_stride=int(row_stride), with_cls=int(with_cls), kind=kind, gptr=gptr, ng=ng,
                desc=desc, last_rows=last_rows)


def seq_cases(kind):
    return [seq_case(b, kind, m, c) for b in SEQ_BATCHES for m in MAX_LENS for c in (1, 0)]


def seq_data(case, D):
    """fp32 CPU inputs of one token case at width D: random node rows / tokens / base (copies must keep every bit), an fp32 CLS row
    that is NOT representable in bf16 (so `cls32` shows its one rounding), and integer-valued twins for the adjoint identity"""
    g = _gen(case["name"], D)
    N, rows, B = case["N"], case["rows"], case["B"]
    return dict(h=torch.randn(N, D, generator=g), tok=torch.randn(rows, D, generator=g), base=torch.randn(N, D, generator=g),
                cls=torch.randn(D, generator=g), h_int=ints((N, D), g), tok_int=ints((rows, D), g), cls_int=ints((D,), g))


SEGMENT_DIMS = (4, 300, 1024)     # one partial column tile of k_segment_sum, two tiles with the second partial, four full tiles
BCAST_DIMS = (4, 300)


def segment_data(batch, D, integer=True):
    """x [N][D] and add / seg [B][D] of a segment case, fp32 on the CPU"""
    g = _gen("segment", batch, D, integer)
    sizes = BATCHES[batch]
    N, B = int(sum(sizes)), len(sizes)
    if integer:
        return ints((N, D), g), ints((B, D), g)
    return torch.randn(N, D, generator=g), torch.randn(B, D, generator=g)


COLSUM_DIMS = (4, 60, 128, 200, 256, 300)    # CW = 16, 16, 32, 32, 64, 64 float4 columns, a partial last tile in each tier
COLSUM_TALL = 1100                           # rows of the matrix that row_idx points into


def colsum_groups(D):
    C = D // 4
    return 256 // (64 if C >= 64 else (32 if C >= 32 else 16))


def colsum_rows(D):
    gr = colsum_groups(D)
    return (0, 1, gr - 1, 8 * gr, 8 * gr + 1, 1000)


def colsum_data(D, rows, integer=True):
    """x [COLSUM_TALL][D] fp32 and row_idx int64 [rows]: a permutation prefix with repeats into the taller matrix"""
    g = _gen("colsum", D, rows, integer)
    x = ints((COLSUM_TALL, D), g) if integer else torch.randn(COLSUM_TALL, D, generator=g)
    idx = torch.randperm(COLSUM_TALL, generator=g)[:rows]
    if rows >= 3:
        idx[rows // 2] = idx[0]      # repeats
        idx[-1] = idx[1]
    return x, idx.to(torch.int64)


ROWS_TOTAL = 50
ROWS_N = (0, 1, 37)
ROWS_DIMS = (4, 300)


def rows_data(n, dim):
    """x [n][dim], idx = the first n of a permutation of ROWS_TOTAL rows, and a full [ROWS_TOTAL][dim] matrix; integer-valued fp32"""
    g = _gen("rows", n, dim)
    return ints((n, dim), g, -64, 64), torch.randperm(ROWS_TOTAL, generator=g)[:n].to(torch.int64), ints((ROWS_TOTAL, dim), g, -64, 64)


def rows_add_data(n, dim, dtype):
    """rows_data with a fraction added to x and full BEFORE the cast to dtype: values of the storage type whose fp32 sum is not
    representable in it, so that the one rounding of gt_rows_add happens (the integers of rows_data add exactly).  The first row also
    holds, whatever the draw, 1 + ulp / 2 (a tie that goes to the even 1) and 1 + 3 ulp / 4 (which a truncation gets wrong)."""
    x, idx, full = rows_data(n, dim)
    g = _gen("rows_add", n, dim)
    x, full = (x + torch.rand(x.shape, generator=g)).to(dtype), (full + torch.rand(full.shape, generator=g)).to(dtype)
    if n:
        ulp = 2.0 ** (-7 if dtype == torch.bfloat16 else -23)
        full[idx[0], 0], full[idx[0], 1] = 1.0, 1.0
        x[0, 0], x[0, 1] = ulp / 2, 3 * ulp / 4
    return x, idx, full


NAN_NEG_SIGNALLING = 0xff800001 - (1 << 32)     # sign set, quiet bit clear, payload in the bits bf16 drops: bf16 0xffc0 by the rule
NAN_HIGH_PAYLOAD = 0x7fa00000                   # quiet bit clear, a payload bit bf16 keeps: bf16 0x7fe0


def scatter_grad(n, dim):
    """fp32 rows [n][dim] for gt_rows_scatter that need rounding, with (n > 0) two NaNs that are not the canonical one and +-inf"""
    x, _, _ = rows_data(n, dim)
    grad = x + torch.rand(x.shape, generator=_gen("scatter", n, dim)) * 1e-2
    if n:
        bits = grad.view(torch.int32)
        bits[0, 0], bits[0, 2] = NAN_NEG_SIGNALLING, NAN_HIGH_PAYLOAD
        grad[0, 1], grad[n - 1, dim - 1] = float("inf"), -float("inf")
    return grad


# ----------------------------------------------------------------------------------------------------------------------------
# references: node rows <-> token rows
# ----------------------------------------------------------------------------------------------------------------------------
def _seq_rows(b, gptr, desc, row_stride, with_cls, rows, flaw):
    """(node0, kept, token rows of the kept nodes, CLS token row) of sequence b.  A graph keeps its LAST kv_len - with_cls nodes;
    kept node j sits at position kv_off + j, the CLS at kv_off + kept; position p is token row row0 + p * row_stride."""
    row0, _, kv_off, kv_len = (int(v) for v in desc[b])
    kept = kv_len - with_cls
    node0 = int(gptr[b + 1]) - kept
    if flaw == "keep_first":
        node0 = int(gptr[b])
    elif flaw == "node0_off_by_one":
        node0 = max(node0 - 1, 0)
    pos = kv_off + np.arange(kept + 1)
    if flaw == "cls_at_kept_minus_1":
        pos[kept] = kv_off + kept - 1
    tok = (row0 * row_stride + pos) % max(rows, 1) if flaw == "stride_swapped" else row0 + pos * row_stride
    return node0, kept, tok[:kept], int(tok[kept])


def ref_seq_gather(h, cls, gptr, desc, row_stride, rows, with_cls, flaw=None):
    """(tokens [rows][D], pad mask int16 [B][max npos]): every position < npos that holds neither a kept node nor the CLS is a zero
    row; mask 1 = padding, 0 = node or CLS, -1 = a position >= npos of its sequence, which the layout does not have."""
    B = desc.shape[0]
    tokens = torch.zeros((rows, h.shape[1]), dtype=h.dtype)
    mask = np.full((B, int(desc[:, 1].max()) if B else 0), -1, np.int16)
    for b in range(B):
        node0, kept, tok, cls_row = _seq_rows(b, gptr, desc, row_stride, with_cls, rows, flaw)
        tokens[torch.from_numpy(tok.astype(np.int64))] = h[node0:node0 + kept]
        if with_cls:
            tokens[cls_row] = cls.to(h.dtype)
        _, npos, kv_off, kv_len = (int(v) for v in desc[b])
        p = np.arange(npos)
        mask[b, :npos] = (p < kv_off) | (p >= kv_off + kv_len)
    return tokens, mask


def ref_seq_scatter(tokens, base, gptr, desc, row_stride, with_cls, N, flaw=None):
    """(node rows [N][D], cls rows [B][D] or None): the gather read backwards.  The leading nodes that a truncated graph drops
    take their `base` row, or 0 without a base."""
    B = desc.shape[0]
    h = torch.zeros((N, tokens.shape[1]), dtype=tokens.dtype) if base is None else base.clone()
    cls = torch.zeros((B, tokens.shape[1]), dtype=tokens.dtype) if with_cls else None
    for b in range(B):
        node0, kept, tok, cls_row = _seq_rows(b, gptr, desc, row_stride, with_cls, tokens.shape[0], flaw)
        h[node0:node0 + kept] = tokens[torch.from_numpy(tok.astype(np.int64))]
        if with_cls:
            cls[b] = tokens[cls_row]
    return h, cls


def ref_token_rows(gptr, desc, row_stride, with_cls, N, flaw=None):
    """(rows int32 [N]: the token row of every node, -1 for dropped nodes; the CLS token row of every sequence, int64 [B])"""
    B = desc.shape[0]
    rows = np.full(N, -1, np.int32)
    cls_rows = np.zeros(B, np.int64)
    for b in range(B):
        node0, kept, tok, cls_rows[b] = _seq_rows(b, gptr, desc, row_stride, with_cls, 1 << 30, flaw)
        rows[node0:node0 + kept] = tok
    return rows, cls_rows


# ----------------------------------------------------------------------------------------------------------------------------
# references: segment ops and column sums (float64: exact for the integer inputs, the yardstick for the random ones)
# ----------------------------------------------------------------------------------------------------------------------------
def ref_segment_sum(x, add, gptr):
    """out[b] = add[b] + sum of the rows of graph b, float64 [B][D]"""
    B = len(gptr) - 1
    out = torch.zeros((B, x.shape[1]), dtype=torch.float64) if add is None else add.double().clone()
    for b in range(B):
        out[b] += x[int(gptr[b]):int(gptr[b + 1])].double().sum(0)
    return out


def ref_segment_abs_sum(x, add, gptr):
    """sum of |terms| of every output element (the scale of the rounding bound), float64 [B][D]"""
    return ref_segment_sum(x.abs(), None if add is None else add.abs(), gptr)


def ref_bcast_add(x, seg, node_graph):
    """out[n] = x[n] + seg[node_graph[n]] (x absent: the broadcast alone), float64"""
    out = seg.double()[torch.from_numpy(np.asarray(node_graph, np.int64))]
    return out if x is None else out + x.double()


def ref_colsum(x, row_idx=None, drop_last=False):
    """out[c] = sum over r of x[row_idx[r]][c] (row_idx absent: all rows), float64 [D].  drop_last: the wrong variant that loses a row."""
    sel = x.double() if row_idx is None else x.double()[row_idx]
    return (sel[:-1] if drop_last else sel).sum(0)


# ----------------------------------------------------------------------------------------------------------------------------
# references: util.hip
# ----------------------------------------------------------------------------------------------------------------------------
def ref_rows_take(x, idx):
    """out[i] = x[idx[i]]"""
    return x[idx]


def ref_rows_put(x, idx, total_rows, out_before=None):
    """out = 0 [total_rows][dim]; out[idx[i]] = x[i].  out_before: the wrong variant without the zero fill."""
    out = torch.zeros((total_rows, x.shape[1]), dtype=x.dtype) if out_before is None else out_before.clone()
    out[idx] = x
    return out


def ref_rows_add(x, idx, out_before, flaw=None):
    """out[idx[i]] += x[i] in fp32, rounded once (to nearest-even) to the storage type (idx does not repeat).  Wrong variants for the
    host tests: "truncate" chops the fp32 sum to bf16 instead of rounding it; "half_up" rounds ties away from zero instead of to even
    (the sum of two bf16 values of like size has 9 significant bits more often than not: a tie)."""
    out = out_before.clone()
    s = out_before[idx].float() + x.float()
    if flaw == "truncate":
        s = (s.view(torch.int32) & ~0xFFFF).view(torch.float32)
    elif flaw == "half_up":
        s = ((s.view(torch.int32) + 0x8000) & ~0xFFFF).view(torch.float32)
    out[idx] = s.to(out.dtype)
    return out


def ref_rows_gather(x, idx, n):
    """fp32 out[i] = x[idx[i]] widened exactly; idx None: rows 0 .. n-1"""
    return (x[:n] if idx is None else x[idx]).float()


def to_storage(g, dtype):
    """fp32 -> the storage type: round to nearest-even; a NaN keeps its sign and the high payload bits and is quieted (gt_common.h:
    bits >> 16 | 0x40).  torch's own CPU conversion agrees on everything but which NaN comes out, so only that is restated."""
    out = g.to(dtype)
    nan = g.isnan()
    if dtype == torch.bfloat16 and bool(nan.any()):
        out.view(torch.int16)[nan] = ((g.contiguous().view(torch.int32)[nan] >> 16) | 0x40).to(torch.int16)
    return out


def ref_rows_scatter(g, idx, total_rows, dtype):
    """out = 0 [total_rows][dim] of dtype; out[idx[i]] = g[i] rounded to nearest-even (NaN preserved); idx None: rows 0 .. n-1"""
    out = torch.zeros((total_rows, g.shape[1]), dtype=dtype)
    out[torch.arange(g.shape[0]) if idx is None else idx] = to_storage(g, dtype)
    return out


def ref_copy2d(dst, dst_col0, src, src_col0, width):
    """dst[r][dst_col0 .. +width) = src[r][src_col0 .. +width) for every row of src; the rest of dst is what it was"""
    out = dst.clone()
    out[:src.shape[0], dst_col0:dst_col0 + width] = src[:, src_col0:src_col0 + width]
    return out


def ref_repitch(src, dst_cols):
    """dst[r][c] = src[r][c] for c < src_cols, else 0"""
    out = torch.zeros((src.shape[0], dst_cols), dtype=src.dtype)
    k = min(dst_cols, src.shape[1])
    out[:, :k] = src[:, :k]
    return out


def ref_gather_f32(src, map_):
    """dst[i] = src[map[i]], 0 where map[i] < 0"""
    m = map_.long()
    return torch.where(m < 0, torch.zeros(()), src[m.clamp(min=0)])


def ref_add3(a, b, c=None):
    return a + b if c is None else a + b + c


def ref_dropout_mask(n, p, seed):
    """the kept set of gt_dropout: drop_hash(seed, element index) >= p * 2^32 (csrc/util.hip), restated with int64 tensors masked to
    32 bits.  p is the fp32 value the entry point receives."""
    M = 0xFFFFFFFF
    s0, s1 = seed & M, (seed >> 32) & M
    x = ((torch.arange(n, dtype=torch.int64) * 0x9E3779B1) & M) ^ s0
    x = x ^ (x >> 16); x = (x * 0x7feb352d) & M
    x = x ^ (x >> 15); x = (x * 0x846ca68b) & M
    x = x ^ (x >> 16)
    x = x ^ s1
    t = float(np.float32(p)) * 4294967296.0
    thr = int(min(max(t, 1.0), 4294967295.0)) if p > 0 else 0
    return x >= thr


def ref_dropout(x, p, seed):
    """y = kept ? x * (1 / (1 - p)) : 0, the product in fp32 and rounded once to the storage type"""
    inv_keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    y = (x.float() * torch.tensor(inv_keep, dtype=torch.float32)).to(x.dtype)
    return torch.where(ref_dropout_mask(x.numel(), p, seed).reshape(x.shape), y, torch.zeros((), dtype=x.dtype))


# ----------------------------------------------------------------------------------------------------------------------------
# comparisons
# ----------------------------------------------------------------------------------------------------------------------------
def same(got, want):
    """bit for bit: torch.equal on the bit patterns (so NaN equals the same NaN, and -0 is not +0)"""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.is_floating_point():
        view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
        return torch.equal(got.view(view), want.view(view))
    return torch.equal(got, want)


def differences(got, want, limit=6):
    """the first elements whose bits differ, as text for an assertion message"""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"{got.dtype} {tuple(got.shape)} vs {want.dtype} {tuple(want.shape)}"
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    gb, wb = got.view(view).reshape(-1), want.view(view).reshape(-1)
    bad = (gb != wb).nonzero().reshape(-1)
    mask = (1 << 8 * got.element_size()) - 1
    return f"{bad.numel()} of {gb.numel()} differ: " + ", ".join(
        f"[{int(i)}] got {float(got.reshape(-1)[i])} ({int(gb[i]) & mask:#x}) want {float(want.reshape(-1)[i])} ({int(wb[i]) & mask:#x})"
        for i in bad[:limit])


# ----------------------------------------------------------------------------------------------------------------------------
# guarded launchers
# ----------------------------------------------------------------------------------------------------------------------------
class _Ptr(int):
    """an address (device buffer or stream): told apart from a size or a code when _call checks the kind of every argument"""


def _p(t, offset_bytes=0):
    return None if t is None else _Ptr(t.data_ptr() + offset_bytes)


def _stream():
    from graphtrans_amd.graph import _stream as s
    return _Ptr(s())


_PROTOTYPES = {}


def prototype(name):
    """the parameter names of entry point `name`, in order, from its declaration in include/graphtrans_hip.h"""
    if not _PROTOTYPES:
        import os
        import re
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "graphtrans_hip.h")) as fh:
            text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
        for m in re.finditer(r"\b(gt_\w+)\s*\(([^()]*)\)\s*;", text):
            _PROTOTYPES[m.group(1)] = [re.findall(r"\w+", a)[-1] for a in m.group(2).split(",") if a.strip() not in ("", "void")]
    return _PROTOTYPES[name]


def _call(name, **args):
    """Launch `name` with its arguments given BY THE NAMES of the C prototype.  They must be the prototype's parameters in the
    prototype's order, as many as _lib.py's ctypes signature, and each of the kind the signature takes: an address (or None) for a
    pointer, a plain int for an integer, a float for a float -- so a swapped pair, a missing argument or a size passed where a pointer
    belongs is an assertion here."""
    import ctypes as C
    from graphtrans_amd import _lib
    kinds = _lib.SIGNATURES[name][1]
    assert list(args) == prototype(name), f"{name}: arguments {list(args)}, the prototype is {prototype(name)}"
    assert len(args) == len(kinds), f"{name}: {len(args)} arguments, the ctypes signature has {len(kinds)}"
    for (what, v), kind in zip(args.items(), kinds):
        if kind is C.c_void_p:
            assert v is None or type(v) is _Ptr, f"{name}: {what} must be an address or None, not {v!r}"
        elif kind is C.c_float:
            assert type(v) is float, f"{name}: {what} must be a float, not {v!r}"
        else:
            assert kind in (C.c_int, C.c_int64, C.c_uint64, C.c_size_t) and type(v) is int, f"{name}: {what} must be a plain int, not {v!r}"
    _lib.launch(name, *(int(v) if type(v) is _Ptr else v for v in args.values()))


def _ok(t, dtype, min_elems, what):
    """a device tensor the kernel may touch `min_elems` elements of"""
    assert isinstance(t, torch.Tensor) and t.is_cuda, f"{what}: not on the device"
    assert t.is_contiguous(), f"{what}: not contiguous"
    assert t.dtype == dtype, f"{what}: {t.dtype}, the entry point takes {dtype}"
    assert t.numel() >= min_elems, f"{what}: {t.numel()} elements, the kernel touches {min_elems}"
    assert t.data_ptr() % 16 == 0, f"{what}: not 16-byte aligned"


def _opt(t, dtype, min_elems, what):
    if t is not None:
        _ok(t, dtype, min_elems, what)


def _index_ok(idx, n, limit, what, lowest=0):
    """an index tensor of >= n entries, the first n inside [lowest, limit)"""
    v = idx.detach().cpu().reshape(-1)[:n]
    assert v.numel() == n, f"{what}: {v.numel()} entries, {n} needed"
    if n:
        assert int(v.min()) >= lowest and int(v.max()) < limit, f"{what}: values {int(v.min())} .. {int(v.max())} outside [{lowest}, {limit})"


def out_buffer(n, dtype, init=None):
    """a flat device buffer of n + PAD elements filled with SENTINEL (its first n from `init` when given)"""
    buf = torch.full((n + PAD,), SENTINEL, dtype=dtype, device=DEV)
    if init is not None:
        assert init.numel() == n and init.dtype == dtype
        buf[:n] = init.reshape(-1).to(DEV)
    return buf


def _take(buf, shape):
    """the needed part of an out_buffer, after checking that the tail kept its sentinel"""
    n = int(np.prod(shape))
    assert bool((buf[n:] == SENTINEL).all()), "the kernel wrote past the end of its output"
    return buf[:n].reshape(shape)


def _code(dtype):
    return {torch.float32: GT_F32, torch.bfloat16: GT_BF16}[dtype]


def launch_copy2d(dst_init, dst_col0, src, src_col0, width):
    """dst [R][dst_cols] (initial contents given) <- columns of src [rows][src_cols]; columns in elements, converted to bytes here"""
    elt = src.element_size()
    rows, src_cols = src.shape
    dst_cols = dst_init.shape[1]
    assert dst_init.dtype == src.dtype and dst_init.shape[0] >= rows
    assert 0 <= dst_col0 and dst_col0 + width <= dst_cols and 0 <= src_col0 and src_col0 + width <= src_cols
    _ok(src, src.dtype, rows * src_cols, "src")
    assert all(v * elt % 16 == 0 for v in (dst_col0, src_col0, width, dst_cols, src_cols)), "offsets, width and pitches: multiples of 16 bytes"
    buf = out_buffer(dst_init.numel(), src.dtype, dst_init)
    _call("gt_copy2d", dst=_p(buf, dst_col0 * elt), dst_pitch_bytes=dst_cols * elt, src=_p(src, src_col0 * elt), src_pitch_bytes=src_cols * elt,
          width_bytes=width * elt, rows=rows, stream=_stream())
    return _take(buf, dst_init.shape)


def _rows_into(name, x, idx, out_init):
    """gt_rows_put / gt_rows_add: rows x [n][dim] into out [total_rows][dim] (initial contents given) at idx"""
    n, dim = x.shape
    dtype = x.dtype
    total_rows = out_init.shape[0]
    _ok(x, dtype, n * dim, "x")
    _ok(idx, torch.int64, n, "idx")
    assert idx.numel() == n and out_init.dtype == dtype and out_init.shape[1] == dim
    _index_ok(idx, n, total_rows, "idx")
    assert len(set(idx.cpu().tolist())) == n, "idx repeats"
    buf = out_buffer(out_init.numel(), dtype, out_init)
    if name == "gt_rows_put":
        _call(name, dtype=_code(dtype), x=_p(x), idx=_p(idx), n=n, total_rows=total_rows, dim=dim, out=_p(buf), stream=_stream())
    else:
        _call(name, dtype=_code(dtype), x=_p(x), idx=_p(idx), n=n, dim=dim, out=_p(buf), stream=_stream())
    return _take(buf, out_init.shape)


def launch_rows_take(x, idx, out_init):
    """out[i] = x[idx[i]] for i < len(idx); x [source rows][dim]"""
    n, dim = idx.numel(), x.shape[1]
    dtype = x.dtype
    _ok(x, dtype, x.shape[0] * dim, "x")
    _ok(idx, torch.int64, n, "idx")
    _index_ok(idx, n, x.shape[0], "idx")
    assert out_init.dtype == dtype and out_init.shape[1] == dim and out_init.shape[0] >= n
    buf = out_buffer(out_init.numel(), dtype, out_init)
    _call("gt_rows_take", dtype=_code(dtype), x=_p(x), idx=_p(idx), n=n, dim=dim, out=_p(buf), stream=_stream())
    return _take(buf, out_init.shape)


def launch_rows_put(x, idx, out_init):
    return _rows_into("gt_rows_put", x, idx, out_init)


def launch_rows_add(x, idx, out_init):
    return _rows_into("gt_rows_add", x, idx, out_init)


def launch_rows_gather(x, idx, n):
    """fp32 [n][dim] <- rows of x (idx None: the first n)"""
    dim = x.shape[1]
    _ok(x, x.dtype, x.shape[0] * dim, "x")
    if idx is None:
        assert n <= x.shape[0]
    else:
        _ok(idx, torch.int64, n, "idx")
        _index_ok(idx, n, x.shape[0], "idx")
    buf = out_buffer(n * dim, torch.float32)
    _call("gt_rows_gather", dtype=_code(x.dtype), x=_p(x), idx=_p(idx), n=n, dim=dim, out=_p(buf), stream=_stream())
    return _take(buf, (n, dim))


def launch_rows_scatter(g, idx, total_rows, dtype):
    """[total_rows][dim] of dtype <- fp32 rows g (idx None: rows 0 .. n-1)"""
    n, dim = g.shape
    _ok(g, torch.float32, n * dim, "grad")
    if idx is None:
        assert n <= total_rows
    else:
        _ok(idx, torch.int64, n, "idx")
        _index_ok(idx, n, total_rows, "idx")
        assert len(set(idx.cpu().tolist())) == n, "idx repeats"
    buf = out_buffer(total_rows * dim, dtype)
    _call("gt_rows_scatter", dtype=_code(dtype), grad=_p(g), idx=_p(idx), n=n, total_rows=total_rows, dim=dim, out=_p(buf), stream=_stream())
    return _take(buf, (total_rows, dim))


def launch_add3(a, b, c):
    n = a.numel()
    for t, what in ((a, "a"), (b, "b")):
        _ok(t, torch.float32, n, what)
    _opt(c, torch.float32, n, "c")
    buf = out_buffer(n, torch.float32)
    _call("gt_add3", a=_p(a), b=_p(b), c=_p(c), n=n, out=_p(buf), stream=_stream())
    return _take(buf, a.shape)


def launch_gather_f32(src, map_):
    n = map_.numel()
    _ok(src, torch.float32, 1, "src")
    _ok(map_, torch.int32, n, "map")
    _index_ok(map_, n, src.numel(), "map", lowest=-(1 << 31))
    buf = out_buffer(n, torch.float32)
    _call("gt_gather_f32", dst=_p(buf), src=_p(src), map=_p(map_), n=n, stream=_stream())
    return _take(buf, (n,))


def launch_repitch(src, dst_cols):
    """[rows][dst_cols] <- src [rows][src_cols], elements of 2 or 4 bytes"""
    rows, src_cols = src.shape
    if src_cols:
        _ok(src, src.dtype, rows * src_cols, "src")
    assert src.element_size() in (2, 4)
    buf = out_buffer(rows * dst_cols, src.dtype)
    _call("gt_repitch", dst=_p(buf), dst_cols=dst_cols, src=_p(src) if src_cols else None, src_cols=src_cols, rows=rows,
          elt_bytes=src.element_size(), stream=_stream())
    return _take(buf, (rows, dst_cols))


def launch_dropout(x, p, seed):
    n = x.numel()
    _ok(x, x.dtype, n, "x")
    assert n % 4 == 0 and n < 1 << 32 and 0.0 <= p < 1.0 and 0 <= seed < 1 << 64
    buf = out_buffer(n, x.dtype)
    _call("gt_dropout", dtype=_code(x.dtype), x=_p(x), y=_p(buf), n=n, p=float(p), seed=int(seed), stream=_stream())
    return _take(buf, x.shape)


def launch_segment_bcast_add(x, seg, node_graph):
    """[N][D] = x[n] + seg[node_graph[n]]; x may be None"""
    B, D = seg.shape
    N = node_graph.numel()
    _ok(seg, seg.dtype, B * D, "seg")
    _opt(x, seg.dtype, N * D, "x")
    _ok(node_graph, torch.int32, N, "node_graph")
    _index_ok(node_graph, N, B, "node_graph")
    buf = out_buffer(N * D, seg.dtype)
    _call("gt_segment_bcast_add", dtype=_code(seg.dtype), x=_p(x), seg=_p(seg), node_graph=_p(node_graph), num_nodes=N, num_graphs=B, dim=D,
          out=_p(buf), stream=_stream())
    return _take(buf, (N, D))


def _gptr_ok(gptr, B, N):
    v = gptr.detach().cpu().reshape(-1)
    assert v.numel() >= B + 1, "graph_ptr: shorter than B + 1"
    v = v[:B + 1].long()
    assert int(v[0]) == 0 and int(v[-1]) == N and bool((v[1:] >= v[:-1]).all()), "graph_ptr: not a partition of the N rows"


def launch_segment_sum(x, add, gptr):
    """[B][D] = add[b] + sum of graph b's rows, on the one-block-per-graph kernel whatever N"""
    N, D = x.shape
    B = gptr.numel() - 1
    _ok(x, x.dtype, max(N * D, 1), "x")
    _opt(add, x.dtype, B * D, "add")
    _ok(gptr, torch.int32, B + 1, "graph_ptr")
    _gptr_ok(gptr, B, N)
    buf = out_buffer(B * D, x.dtype)
    _call("gt_segment_sum", dtype=_code(x.dtype), x=_p(x), add=_p(add), graph_ptr=_p(gptr), num_nodes=N, num_graphs=B, dim=D, out=_p(buf),
          stream=_stream())
    return _take(buf, (B, D))


def launch_colsum(x, row_idx, rows):
    """fp32 [D] = column sums of x's first `rows` rows (gt_colsum_f32), or of the rows row_idx[0 .. rows) (gt_colsum_rows_f32)"""
    D = x.shape[1]
    _ok(x, x.dtype, x.shape[0] * D, "x")
    buf = out_buffer(D, torch.float32)
    if row_idx is None:
        assert rows <= x.shape[0]
        _call("gt_colsum_f32", dtype=_code(x.dtype), x=_p(x), rows=rows, dim=D, out=_p(buf), stream=_stream())
    else:
        _ok(row_idx, torch.int64, max(rows, 1), "row_idx")
        _index_ok(row_idx, rows, x.shape[0], "row_idx")
        _call("gt_colsum_rows_f32", dtype=_code(x.dtype), x=_p(x), row_idx=_p(row_idx), rows=rows, D=D, out=_p(buf), stream=_stream())
    return _take(buf, (D,))


class DeviceLayout:
    """the layout arrays of a seq_case on the device, and the host-side bounds every token launcher checks"""

    def __init__(self, case):
        self.case = case
        self.gptr = torch.tensor(case["gptr"], device=DEV)
        self.ng = torch.tensor(case["ng"], device=DEV)
        self.desc = torch.tensor(case["desc"], device=DEV)

    def check(self, token_rows):
        c = self.case
        B, N = c["B"], c["N"]
        _ok(self.gptr, torch.int32, B + 1, "graph_ptr")
        _ok(self.ng, torch.int32, N, "node_graph")
        _ok(self.desc, torch.int32, 4 * B, "seq_desc")
        _gptr_ok(self.gptr, B, N)
        _index_ok(self.ng, N, B, "node_graph")
        d = self.desc.cpu().numpy().astype(np.int64)
        n = np.diff(self.gptr.cpu().numpy().astype(np.int64))
        kept = d[:, 3] - c["with_cls"]
        assert (d >= 0).all() and (d[:, 1] >= 1).all() and (d[:, 1] <= c["max_npos"]).all(), "seq_desc: npos outside [1, max_npos]"
        assert (d[:, 2] + d[:, 3] <= d[:, 1]).all() and (kept >= 0).all() and (kept <= n).all(), "seq_desc: kv range outside the sequence / graph"
        assert (d[:, 0] + (d[:, 1] - 1) * c["row_stride"] < token_rows).all(), "seq_desc: a position beyond the token matrix"


def launch_seq_gather(lay, h, cls, cls32=None, want_mask=True):
    """(tokens [rows][D], pad mask uint8 [B][max_npos] or None).  cls32 given: gt_seq_gather_cls32 (an fp32 CLS row, no mask)."""
    c = lay.case
    D = h.shape[1]
    lay.check(c["rows"])
    _ok(h, h.dtype, c["N"] * D, "h")
    assert h.shape[0] == c["N"]
    tok = out_buffer(c["rows"] * D, h.dtype)
    args = dict(graph_ptr=_p(lay.gptr), seq_desc=_p(lay.desc), num_seqs=c["B"], row_stride=c["row_stride"], max_npos=c["max_npos"],
                with_cls=c["with_cls"], dim=D, tokens=_p(tok))
    if cls32 is not None:
        _ok(cls32, torch.float32, D, "cls32")
        _call("gt_seq_gather_cls32", dtype=_code(h.dtype), h=_p(h), cls32=_p(cls32), **args, stream=_stream())
        return _take(tok, (c["rows"], D)), None
    if c["with_cls"]:
        _ok(cls, h.dtype, D, "cls")
    mask = out_buffer(c["B"] * c["max_npos"], torch.uint8) if want_mask else None
    _call("gt_seq_gather", dtype=_code(h.dtype), h=_p(h), cls=_p(cls) if c["with_cls"] else None, **args, pad_mask=_p(mask), stream=_stream())
    return _take(tok, (c["rows"], D)), (_take(mask, (c["B"], c["max_npos"])) if want_mask else None)


def launch_seq_scatter(lay, tokens, base, want_cls=True):
    """(h_out [N][D], cls_out [B][D] or None) from token rows"""
    c = lay.case
    D = tokens.shape[1]
    lay.check(tokens.shape[0])
    _ok(tokens, tokens.dtype, c["rows"] * D, "tokens")
    _opt(base, tokens.dtype, c["N"] * D, "base")
    h = out_buffer(c["N"] * D, tokens.dtype)
    cls = out_buffer(c["B"] * D, tokens.dtype) if want_cls else None
    _call("gt_seq_scatter", dtype=_code(tokens.dtype), tokens=_p(tokens), base=_p(base), graph_ptr=_p(lay.gptr), node_graph=_p(lay.ng),
          seq_desc=_p(lay.desc), num_seqs=c["B"], row_stride=c["row_stride"], with_cls=c["with_cls"], num_nodes=c["N"], dim=D, h_out=_p(h),
          cls_out=_p(cls), stream=_stream())
    return _take(h, (c["N"], D)), (_take(cls, (c["B"], D)) if want_cls else None)


def launch_seq_token_rows(lay, cls32, D, dtype):
    """(tokens [rows][D] of dtype, SENTINEL except the CLS rows; rows int32 [N])"""
    c = lay.case
    lay.check(c["rows"])
    if c["with_cls"]:
        _ok(cls32, torch.float32, D, "cls32")
    tok = out_buffer(c["rows"] * D, dtype)
    rows = out_buffer(c["N"], torch.int32)
    _call("gt_seq_token_rows", dtype=_code(dtype), cls32=_p(cls32) if c["with_cls"] else None, graph_ptr=_p(lay.gptr), node_graph=_p(lay.ng),
          seq_desc=_p(lay.desc), num_seqs=c["B"], row_stride=c["row_stride"], with_cls=c["with_cls"], N=c["N"], D=D, tokens=_p(tok), rows=_p(rows),
          stream=_stream())
    return _take(tok, (c["rows"], D)), _take(rows, (c["N"],))


def launch_seq_layout_packed(gptr, B, max_len, with_cls, work_cap, work_room):
    """(desc int32 [B][4], last_rows int64 [B], work int32 [work_room][2] -- SENTINEL past work_cap --, meta int32 [4])"""
    assert 0 <= work_cap <= work_room and 0 < B <= 65535 and max_len > 0
    _ok(gptr, torch.int32, B + 1, "graph_ptr")
    _gptr_ok(gptr, B, int(gptr[B]))
    desc = out_buffer(4 * B, torch.int32)
    last = out_buffer(B, torch.int64)
    work = out_buffer(2 * work_room, torch.int32)
    meta = out_buffer(4, torch.int32)
    _call("gt_seq_layout_packed", graph_ptr=_p(gptr), B=B, max_input_len=max_len, with_cls=with_cls, seq_desc=_p(desc), last_rows=_p(last),
          work_items=_p(work), work_capacity=work_cap, meta=_p(meta), stream=_stream())
    return _take(desc, (B, 4)), _take(last, (B,)), _take(work, (work_room, 2)), _take(meta, (4,))
