"""gt_embed_tokens_fwd / gt_embed_tokens_bwd (csrc/embed.hip) and ops.embed_tokens against the composition of the tested ops they
replace, bit for bit:

    forward   ops.embed_sum -> + perturb (fp32) -> ops.seq_gather(h, cls, gs, packed layout) -> .to(dtype)
    backward  gt_seq_scatter of the token gradient -> .float() -> gt_embed_sum_bwd_sorted with the same plan

Outputs are prefilled with NaN: a row the kernels do not write shows.  d cls: the float64 column sum of the CLS rows of the gradient,
within (B - 1) * 2^-24 * sum_b |g_b| per column (a fixed-order fp32 sum of B terms).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOM_DIMS = [119, 4, 12, 12, 10, 6, 6, 2, 2]


def _gs(sizes):
    from graphtrans_amd.graph import GraphStructure
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    return GraphStructure.build(torch.zeros((2, 0), dtype=torch.int64, device=DEV), batch, sizes=list(sizes))


def _encoder(form, N, D, gen):
    """-> (columns, tables, clamps) on the GPU.  one: T = 1; code2: columns 0 / 1 as strided views of one (N, 2) matrix + a depth
    column with clamp 20 and values above it; atom: the nine AtomEncoder tables"""
    if form == "one":
        rows, clamps = [5], None
        cols = [torch.randint(0, 5, (N,), generator=gen).to(DEV)]
    elif form == "code2":
        rows, clamps = [11, 13, 21], [None, None, 20]
        x = torch.stack([torch.randint(0, 11, (N,), generator=gen), torch.randint(0, 13, (N,), generator=gen)], 1).to(DEV)
        depth = torch.randint(0, 27, (N,), generator=gen)
        depth[0] = 26   # above the clamp whatever the draw
        cols = [x[:, 0], x[:, 1], depth.to(DEV)]
    else:
        rows, clamps = ATOM_DIMS, None
        x = torch.stack([torch.randint(0, r, (N,), generator=gen) for r in rows], 1).to(DEV)
        cols = [x[:, i] for i in range(len(rows))]
    tables = [torch.randn(r, D, generator=gen).to(DEV) for r in rows]
    return cols, tables, clamps


def _desc(cols, tables, clamps):
    T = len(tables)
    I64, P = C.c_int64 * T, C.c_void_p * T
    idx = P(*[c.data_ptr() for c in cols])
    strides = I64(*[c.stride(0) if c.shape[0] > 1 else 1 for c in cols])
    clamp = I64(*[-1 if clamps is None or clamps[t] is None else int(clamps[t]) for t in range(T)])
    tabs = P(*[t.data_ptr() for t in tables])
    rows = I64(*[t.shape[0] for t in tables])
    return T, idx, strides, clamp, tabs, rows


def _code(dtype):
    from graphtrans_amd import _lib
    return _lib.GT_F32 if dtype == torch.float32 else _lib.GT_BF16


def _token_rows(gs, lay, D, dtype, cls32, fill=float("nan")):
    """gt_seq_token_rows into a `fill`-prefilled token matrix -> (tokens, row map)"""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _ptr, _stream
    tokens = torch.full((lay.rows, D), fill, dtype=dtype, device=DEV)
    rowmap = torch.full((gs.N,), -7, dtype=torch.int32, device=DEV)
    _lib.launch("gt_seq_token_rows", _code(dtype), _ptr(cls32), _ptr(gs.graph_ptr), _ptr(gs.node_graph), _ptr(lay.desc), lay.B, lay.row_stride,
                1 if lay.with_cls else 0, gs.N, D, _ptr(tokens), _ptr(rowmap), _stream())
    return tokens, rowmap


def _fwd_kernel(cols, tables, clamps, perturb, gs, lay, dtype, cls32):
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _ptr, _stream
    D = tables[0].shape[1]
    T, idx, strides, clamp, tabs, _ = _desc(cols, tables, clamps)
    tokens, rowmap = _token_rows(gs, lay, D, dtype, cls32)
    _lib.launch("gt_embed_tokens_fwd", T, idx, strides, clamp, tabs, _ptr(perturb), _ptr(rowmap), gs.N, D, _code(dtype), _ptr(tokens), _stream())
    return tokens, rowmap


def _plan(cols, tables, clamps, N):
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _ptr, _stream
    L = _lib.lib()
    T, idx, strides, clamp, _, rows = _desc(cols, tables, clamps)
    plan = torch.empty(L.gt_embed_sort_plan_bytes(T, rows, N), dtype=torch.uint8, device=DEV)
    wsb = L.gt_embed_sort_workspace_bytes(T, rows, N)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    _lib.launch("gt_embed_sort", T, idx, strides, clamp, rows, N, _ptr(plan), plan.numel(), _ptr(ws), wsb, _stream())
    return plan


def _nan_grads(tables):
    return [torch.full_like(t, float("nan")) for t in tables]


def _bwd_kernel(cols, tables, clamps, plan, g, rowmap, N, want_dadd):
    """gt_embed_tokens_bwd into NaN-prefilled outputs -> (d_tables, d_add)"""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _ptr, _stream
    D = tables[0].shape[1]
    T, _, _, _, _, rows = _desc(cols, tables, clamps)
    grads = _nan_grads(tables)
    dt = (C.c_void_p * T)(*[x.data_ptr() for x in grads])
    dadd = torch.full((N, D), float("nan"), dtype=torch.float32, device=DEV) if want_dadd else None
    wsb = _lib.lib().gt_embed_tokens_bwd_workspace_bytes(T, N, D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    _lib.launch("gt_embed_tokens_bwd", T, rows, _code(g.dtype), _ptr(g), _ptr(rowmap), N, D, _ptr(plan), dt, _ptr(dadd), _ptr(ws), wsb, _stream())
    return grads, dadd


def _bwd_reference(cols, tables, clamps, plan, g, gs, lay):
    """gt_seq_scatter of the token gradient -> .float() -> gt_embed_sum_bwd_sorted with the same plan -> (d_tables, d node rows)"""
    from graphtrans_amd import _lib, ops
    from graphtrans_amd.graph import _ptr, _stream
    D = tables[0].shape[1]
    T, _, _, _, _, rows = _desc(cols, tables, clamps)
    dh, _ = ops._scatter_raw(g, None, gs, lay, False)
    dh = dh.float()
    grads = _nan_grads(tables)
    dt = (C.c_void_p * T)(*[x.data_ptr() for x in grads])
    wsb = _lib.lib().gt_embed_sum_bwd_sorted_workspace_bytes(T, gs.N, D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    _lib.launch("gt_embed_sum_bwd_sorted", T, rows, _ptr(dh), gs.N, D, _ptr(plan), dt, _ptr(ws), wsb, _stream())
    return grads, dh


def _dropped(sizes, max_len):
    """bool [N]: the leading nodes a truncated graph drops (modules/utils.py:17-21 keeps the last max_len)"""
    out = []
    for n in sizes:
        out += [True] * max(n - max_len, 0) + [False] * min(n, max_len)
    return torch.tensor(out)


def _check_all(cols, tables, clamps, sizes, max_len, with_cls, gen, dtypes=(torch.float32, torch.bfloat16)):
    """Forward and backward, kernels and op, for both token types (where D allows) with and without a perturbation"""
    from graphtrans_amd import ops
    gs = _gs(sizes)
    N, D, B = gs.N, tables[0].shape[1], len(sizes)
    lay = gs.layout("packed", max_len, with_cls)
    dropped = _dropped(sizes, max_len)
    assert lay.rows == int((~dropped).sum()) + (B if with_cls else 0)
    cls = torch.randn(1, 1, D, generator=gen).to(DEV) if with_cls else None
    plan = _plan(cols, tables, clamps, N)
    for dtype in dtypes:
        if dtype == torch.bfloat16 and D % 8:
            continue
        for has_perturb in (False, True):
            what = (sizes, max_len, with_cls, D, dtype, has_perturb)
            perturb = (torch.randn(N, D, generator=gen) * 0.5).to(DEV) if has_perturb else None
            # ---- forward
            h = ops.embed_sum(cols, tables, clamps)
            if perturb is not None:
                h = h + perturb
            ref, _ = ops.seq_gather(h, cls, gs, lay)
            ref = ref.to(dtype)
            cls32 = None if cls is None else cls.reshape(-1).contiguous()
            got, rowmap = _fwd_kernel(cols, tables, clamps, perturb, gs, lay, dtype, cls32)
            assert torch.equal(got, ref), ("forward kernel", what)
            assert torch.equal(rowmap.cpu() < 0, dropped), ("row map", what)
            assert ops.embed_tokens_supported(cols, tables, gs, lay, dtype)
            tabs_a = [t.clone().requires_grad_(True) for t in tables]
            cls_a = None if cls is None else cls.clone().requires_grad_(True)
            pert_a = None if perturb is None else perturb.clone().requires_grad_(True)
            tok = ops.embed_tokens(cols, tabs_a, clamps, gs, lay, cls=cls_a, perturb=pert_a, out_dtype=dtype)
            assert tok.dtype == dtype and torch.equal(tok.detach(), ref), ("forward op", what)
            # ---- backward
            g = torch.randn(lay.rows, D, generator=gen).to(DEV).to(dtype)
            want_t, want_dh = _bwd_reference(cols, tables, clamps, plan, g, gs, lay)
            got_t, got_dadd = _bwd_kernel(cols, tables, clamps, plan, g, rowmap, N, has_perturb)
            again_t, again_dadd = _bwd_kernel(cols, tables, clamps, plan, g, rowmap, N, has_perturb)
            tok.backward(g)
            for t in range(len(tables)):
                assert torch.equal(got_t[t], want_t[t]), ("d_table kernel", t, what)
                assert torch.equal(again_t[t], got_t[t]), ("determinism", t, what)
                assert torch.equal(tabs_a[t].grad, want_t[t]), ("d_table op", t, what)
                key = cols[t].cpu().clamp(max=clamps[t]) if clamps and clamps[t] is not None else cols[t].cpu()
                hit = torch.bincount(key[~dropped], minlength=tables[t].shape[0]) > 0
                assert (got_t[t][~hit.to(DEV)] == 0).all(), ("rows no kept node hits", t, what)
            if has_perturb:
                assert torch.equal(got_dadd, want_dh) and torch.equal(again_dadd, got_dadd), ("d_perturb kernel", what)
                assert torch.equal(pert_a.grad, want_dh), ("d_perturb op", what)
                assert (got_dadd[dropped.to(DEV)] == 0).all(), ("d_perturb of dropped nodes", what)
            if with_cls:
                gc = g[lay.last_rows].double()
                want = gc.sum(0)
                bound = (B - 1) * 2.0 ** -24 * gc.abs().sum(0)
                err = (cls_a.grad.reshape(-1).double() - want).abs()
                assert bool((err <= bound).all()), ("d_cls", what, float(err.max()), float(bound.min()))


SIZES = [(1,), (5, 1, 9, 3), (64,), (65, 70, 200)]
FORMS = ["one", "code2", "atom"]
WIDTHS = [8, 40, 256, 4]
CASES = []
for _i, (_s, _m, _c) in enumerate((s, m, c) for s in SIZES for m in (1000, 7) for c in (True, False)):
    CASES.append((_s, _m, _c, FORMS[_i % 3], WIDTHS[(_i + _i // 4) % 4]))
# every form at the shipped width, every width with the Code2 form, on the batch with a truncated and an untouched graph
CASES += [((5, 1, 9, 3), 7, True, f, 256) for f in FORMS] + [((5, 1, 9, 3), 7, True, "code2", d) for d in (4, 8, 40)]


@pytest.mark.parametrize("sizes,max_len,with_cls,form,D", CASES,
                         ids=["%s-len%d-%s-%s-D%d" % ("_".join(map(str, c[0])), c[1], "cls" if c[2] else "nocls", c[3], c[4]) for c in CASES])
def test_embed_tokens_equal_the_composition(sizes, max_len, with_cls, form, D):
    gen = torch.Generator().manual_seed(11)
    cols, tables, clamps = _encoder(form, sum(sizes), D, gen)
    _check_all(cols, tables, clamps, sizes, max_len, with_cls, gen)


def test_cases_cover_what_they_must():
    assert {c[3] for c in CASES} == set(FORMS) and {c[4] for c in CASES} == set(WIDTHS)
    assert {c[0] for c in CASES} == set(SIZES) and {c[1] for c in CASES} == {1000, 7} and {c[2] for c in CASES} == {True, False}
    for s in SIZES:   # each batch with and without truncation and CLS
        assert {(c[1], c[2]) for c in CASES if c[0] == s} == {(1000, True), (1000, False), (7, True), (7, False)}
    assert all(n > 7 for n in (65, 70, 200))   # (65, 70, 200) at max_input_len 7: every graph is truncated


@pytest.mark.parametrize("max_len", [1000, 7])
def test_table_collisions(max_len):
    """A 2-row table over 335 nodes (each table row crosses several 64-position chunks: the fix-up kernel adds the partials), a table
    with unused rows, and -- on (5, 1, 9, 3) at max_input_len 7 -- a table row hit only by the two nodes the 9-node graph drops"""
    gen = torch.Generator().manual_seed(12)
    sizes = (65, 70, 200)
    N, D = sum(sizes), 40
    two = torch.randint(0, 2, (N,), generator=gen)
    sparse = torch.tensor([3, 17])[torch.randint(0, 2, (N,), generator=gen)]
    cols = [two.to(DEV), sparse.to(DEV)]
    tables = [torch.randn(2, D, generator=gen).to(DEV), torch.randn(50, D, generator=gen).to(DEV)]
    _check_all(cols, tables, None, sizes, max_len, True, gen)
    sizes = (5, 1, 9, 3)
    N = sum(sizes)
    idx = torch.randint(0, 3, (N,), generator=gen)
    idx[6:8] = 3   # the two leading nodes of the 9-node graph: dropped at max_input_len 7
    assert _dropped(sizes, 7).nonzero().reshape(-1).tolist() == [6, 7]
    tables = [torch.randn(4, 8, generator=gen).to(DEV)]
    _check_all([idx.to(DEV)], tables, None, sizes, max_len, True, gen)
    if max_len == 7:   # (explicitly: row 3 of that table gets exactly 0, not what its dropped nodes would have summed to)
        from graphtrans_amd import ops
        gs = _gs(sizes)
        lay = gs.layout("packed", 7, True)
        tab = tables[0].clone().requires_grad_(True)
        cls = torch.zeros(1, 1, 8, device=DEV)
        ops.embed_tokens([idx.to(DEV)], [tab], None, gs, lay, cls=cls).backward(torch.ones(lay.rows, 8, device=DEV))
        assert (tab.grad[3] == 0).all() and (tab.grad[:3] != 0).any()


def test_argument_errors():
    """bad D, 17 tables, NULL rows: an error status and a message that names the function (checked before any launch)"""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    L = _lib.lib()
    gen = torch.Generator().manual_seed(13)
    N = 6
    one = torch.randint(0, 5, (N,), generator=gen).to(DEV)
    tab = torch.randn(5, 16, generator=gen).to(DEV)
    rowmap = torch.arange(N, dtype=torch.int32, device=DEV)
    tokens = torch.zeros(N, 16, device=DEV)
    before = tokens.clone()
    plan = _plan([one], [tab], None, N)
    ws = torch.empty(L.gt_embed_tokens_bwd_workspace_bytes(17, N, 16), dtype=torch.uint8, device=DEV)
    dtab = torch.zeros_like(tab)

    def fwd(T, D, code, rows_ptr):
        _, idx, strides, clamp, tabs, _ = _desc([one] * T, [tab] * T, None)
        return L.gt_embed_tokens_fwd(T, idx, strides, clamp, tabs, None, rows_ptr, N, D, code, tokens.data_ptr(), _stream())

    def bwd(T, D, code, rows_ptr):
        rows = (C.c_int64 * T)(*[5] * T)
        dt = (C.c_void_p * T)(*[dtab.data_ptr()] * T)
        return L.gt_embed_tokens_bwd(T, rows, code, tokens.data_ptr(), rows_ptr, N, D, plan.data_ptr(), dt, None, ws.data_ptr(), ws.numel(), _stream())

    for fn, name in ((fwd, b"gt_embed_tokens_fwd"), (bwd, b"gt_embed_tokens_bwd")):
        for args in ((1, 6, _lib.GT_F32, rowmap.data_ptr()),      # D not a multiple of 4
                     (1, 12, _lib.GT_BF16, rowmap.data_ptr()),    # bf16 tokens: D not a multiple of 8
                     (1, 0, _lib.GT_F32, rowmap.data_ptr()),
                     (17, 16, _lib.GT_F32, rowmap.data_ptr()),    # more than 16 tables
                     (0, 16, _lib.GT_F32, rowmap.data_ptr()),
                     (1, 16, 5, rowmap.data_ptr()),               # not a token dtype
                     (1, 16, _lib.GT_F32, None)):                 # NULL rows
            assert fn(*args) != 0, (name, args)
            assert name in L.gt_last_error(), (name, args, L.gt_last_error())
    torch.cuda.synchronize()
    assert torch.equal(tokens, before) and (dtab == 0).all()
    assert fwd(1, 16, _lib.GT_F32, rowmap.data_ptr()) == 0   # (the same calls with good arguments run)


def test_op_rejects_what_the_predicate_rejects():
    from graphtrans_amd import ops
    gen = torch.Generator().manual_seed(14)
    sizes = (5, 1, 9, 3)
    gs = _gs(sizes)
    N = gs.N
    cols, tables, clamps = _encoder("code2", N, 8, gen)
    packed, padded = gs.layout("packed", 7, True), gs.layout("padded", 7, True)
    assert ops.embed_tokens_supported(cols, tables, gs, packed) and not ops.embed_tokens_supported(cols, tables, gs, padded)
    assert not ops.embed_tokens_supported(cols, [t[:, :6].contiguous() for t in tables], gs, packed)   # D % 4
    assert not ops.embed_tokens_supported(cols, [t[:, :4].contiguous() for t in tables], gs, packed, torch.bfloat16)   # D % 8 for bf16
    big = [tables[0], torch.zeros(ops.EMBED_SORT_MAX_ROWS + 1, 8, device=DEV), tables[2]]
    assert not ops.embed_tokens_supported(cols, big, gs, packed)
    assert not ops.embed_tokens_supported([c.int() for c in cols], tables, gs, packed)
    assert not ops.embed_tokens_supported([c.cpu() for c in cols], tables, gs, packed)
    cls = torch.zeros(1, 1, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.embed_tokens(cols, tables, clamps, gs, padded, cls=cls)
    with pytest.raises(ValueError):
        ops.embed_tokens(cols, tables, clamps, gs, packed, cls=None)   # the layout has CLS rows
    with pytest.raises(ValueError):
        ops.embed_tokens(cols, tables, clamps, gs, packed, cls=cls, perturb=torch.zeros(N - 1, 8, device=DEV))
