"""PositionalEncoding on the packed token layout, kernel level, through the C ABI: the padded position of every node
(gt_seq_positions), the gather with a row-gathered addend (gt_seq_gather_add) and the same addend in the epilogue of the
row-mapped gnn2transformer GEMM (gt_linear_set_rows_add).  The add is one fp32 add and one rounding on both sides of every
comparison, so everything but the fused LayerNorm is held bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GT_F32, GT_BF16 = 0, 1


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def _p(t):
    return None if t is None else t.data_ptr()


def _layout(sizes, max_len, with_cls):
    """packed layout arrays of a batch + the positions the contract defines, in plain numpy"""
    sizes = np.asarray(sizes, dtype=np.int64)
    B = len(sizes)
    S = min(int(sizes.max()), max_len)
    gptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    kept = np.minimum(sizes, S)
    kv = kept + with_cls
    tok_ptr = np.concatenate([[0], np.cumsum(kv)])
    desc = np.zeros((B, 4), np.int32)
    desc[:, 0], desc[:, 1], desc[:, 3] = tok_ptr[:-1], kv, kv
    pos = np.full(int(sizes.sum()), -1, np.int32)
    for b in range(B):
        pos[gptr[b + 1] - kept[b]:gptr[b + 1]] = S - kept[b] + np.arange(kept[b])
    ng = np.repeat(np.arange(B, dtype=np.int32), sizes)
    return dict(B=B, S=S, N=int(sizes.sum()), rows=int(tok_ptr[-1]), max_npos=int(kv.max()), pos=pos, gptr=torch.tensor(gptr, device=DEV),
                desc=torch.tensor(desc, device=DEV), ng=torch.tensor(ng, device=DEV))


def _big_sizes(max_len):
    rng = np.random.default_rng(max_len)   # the batch of test_row_map_equals_pad_and_unpad_passes
    sizes = rng.integers(1, 120, 40)
    sizes[3] = 1
    return sizes


def _positions(L, with_cls, S_dev=None):
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    pos = torch.full((L["N"],), -7, dtype=torch.int32, device=DEV)
    _lib.launch("gt_seq_positions", _p(L["gptr"]), _p(L["ng"]), _p(L["desc"]), with_cls, L["N"], 0 if S_dev is not None else L["S"], S_dev, _p(pos),
                _stream())
    return pos


POS_CASES = [((9, 1, 17, 6), 8), ((9, 1, 17, 6), 1000), ("big", 50), ("big", 7)]


@pytest.mark.parametrize("with_cls", [1, 0])
@pytest.mark.parametrize("sizes,max_len", POS_CASES, ids=[f"{'4graphs' if s != 'big' else '40graphs'}-max{m}" for s, m in POS_CASES])
def test_positions_equal_the_left_padding_formula(sizes, max_len, with_cls):
    """gt_seq_positions, with S as a host value and with S read on the device from gt_seq_layout_packed's meta: bit-exact against numpy
    (node row graph_ptr[b+1] - kept_b + j -> S - kept_b + j; -1 for dropped nodes), and the device-built desc is the one used here."""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    sizes = _big_sizes(max_len) if isinstance(sizes, str) else sizes
    L = _layout(sizes, max_len, with_cls)
    assert np.array_equal(_positions(L, with_cls).cpu().numpy(), L["pos"])
    B = L["B"]
    desc = torch.empty((B, 4), dtype=torch.int32, device=DEV)
    last = torch.empty(B, dtype=torch.int64, device=DEV)
    cap = B + (L["N"] + B) // 64
    work = torch.empty((cap, 2), dtype=torch.int32, device=DEV)
    meta = torch.empty(4, dtype=torch.int32, device=DEV)
    _lib.launch("gt_seq_layout_packed", _p(L["gptr"]), B, max_len, with_cls, _p(desc), _p(last), _p(work), cap, _p(meta), _stream())
    assert torch.equal(desc, L["desc"]) and int(meta[3]) == L["S"]
    L2 = dict(L, desc=desc)
    assert np.array_equal(_positions(L2, with_cls, S_dev=meta.data_ptr() + 12).cpu().numpy(), L["pos"])


@pytest.mark.parametrize("tok_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("sizes,max_len,with_cls", [((9, 1, 17, 6), 8, 1), ((9, 1, 17, 6), 1000, 0), ("big", 50, 1)])
def test_gather_with_addend_equals_add_then_gather(tok_dtype, sizes, max_len, with_cls):
    """gt_seq_gather_add on fp32 node rows = torch's fp32 h + pe[pos], converted ONCE to the token type, placed by gt_seq_gather_cls32:
    bit for bit in fp32 and in bf16 (both sides round one fp32 sum to nearest-even); CLS rows untouched.  A table wider than the rows
    (its own pitch) and token-typed node rows too."""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    sizes = _big_sizes(max_len) if isinstance(sizes, str) else sizes
    L = _layout(sizes, max_len, with_cls)
    D, ld = 48, 64
    torch.manual_seed(3)
    h32 = torch.randn(L["N"], D, device=DEV)
    cls = torch.randn(D, device=DEV)
    table = torch.randn(L["S"] + 3, ld, device=DEV)
    pos = _positions(L, with_cls)
    tcode = GT_BF16 if tok_dtype == torch.bfloat16 else GT_F32
    st = _stream()
    idx = pos.long().clamp(min=0)
    summed = (h32 + table[idx, :D]).to(tok_dtype)   # (dropped nodes: never gathered)
    ref = torch.full((L["rows"], D), 7.0, dtype=tok_dtype, device=DEV)
    _lib.launch("gt_seq_gather_cls32", tcode, _p(summed), _p(cls), _p(L["gptr"]), _p(L["desc"]), L["B"], 1, L["max_npos"], with_cls, D, _p(ref), st)
    got = torch.full((L["rows"], D), 7.0, dtype=tok_dtype, device=DEV)
    _lib.launch("gt_seq_gather_add", tcode, GT_F32, _p(h32), None, _p(cls), _p(table), ld, _p(pos), _p(L["gptr"]), _p(L["desc"]), L["B"], 1,
                L["max_npos"], with_cls, D, _p(got), None, st)
    assert torch.equal(got, ref)
    if with_cls:   # the CLS rows carry no position
        last = (L["desc"][:, 0] + L["desc"][:, 1] - 1).long()
        assert torch.equal(got[last], cls.to(tok_dtype).expand(L["B"], D))
    # node rows already in the token type (ops.seq_gather on bf16 rows): the sum of the widened row, one rounding
    ht = h32.to(tok_dtype)
    summed_t = (ht.float() + table[idx, :D]).to(tok_dtype)
    ref_t = torch.full((L["rows"], D), 7.0, dtype=tok_dtype, device=DEV)
    _lib.launch("gt_seq_gather_cls32", tcode, _p(summed_t), _p(cls), _p(L["gptr"]), _p(L["desc"]), L["B"], 1, L["max_npos"], with_cls, D, _p(ref_t), st)
    got_t = torch.full((L["rows"], D), 7.0, dtype=tok_dtype, device=DEV)
    _lib.launch("gt_seq_gather_add", tcode, tcode, _p(ht), _p(cls.to(tok_dtype)), None, _p(table), ld, _p(pos), _p(L["gptr"]), _p(L["desc"]), L["B"], 1,
                L["max_npos"], with_cls, D, _p(got_t), None, st)
    assert torch.equal(got_t, ref_t)


@pytest.mark.parametrize("tok_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("max_len,with_cls", [(50, 1), (50, 0), (7, 1), (7, 0)])
def test_row_map_with_addend_equals_gemm_add_gather(tok_dtype, max_len, with_cls):
    """gt_linear_set_rows + gt_linear_set_rows_add (gnn2transformer storing token rows + pe[position] in its epilogue) against the same
    GEMM into fp32 node rows, a torch fp32 add of pe[pos], the conversion to the token type and gt_seq_gather_cls32: bit for bit."""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    from graphtrans_amd.w3 import W3Images
    lib = _lib.lib()
    B, K, N = 40, 256, 128
    L = _layout(_big_sizes(max_len), max_len, with_cls)
    Nn, rows = L["N"], L["rows"]
    assert Nn >= 1024 and int((L["pos"] < 0).sum()) > 0   # truncation drops nodes at both limits
    torch.manual_seed(1)
    x = torch.randn(Nn, K, device=DEV)
    W = torch.randn(N, K, device=DEV) / K ** 0.5
    bias, cls = torch.randn(N, device=DEV), torch.randn(N, device=DEV)
    pe = torch.randn(max_len, N, device=DEV)
    tcode = GT_BF16 if tok_dtype == torch.bfloat16 else GT_F32
    pos = _positions(L, with_cls)
    imgs = W3Images([W])
    imgs.build()
    st = _stream()
    with imgs.bound():
        assert lib.gt_linear_rows_ok(GT_F32, GT_F32, tcode, _p(W), Nn, N, K) == 1
        hn = torch.empty(Nn, N, device=DEV)
        _lib.launch("gt_linear_fwd_ld2", GT_F32, GT_F32, GT_F32, _p(x), _p(W), _p(bias), _p(hn), Nn, N, K, K, N, 0, 0.0, 0, st)
        summed = (hn + pe[pos.long().clamp(min=0)]).to(tok_dtype)
        tok_ref = torch.full((rows, N), 7.0, dtype=tok_dtype, device=DEV)
        _lib.launch("gt_seq_gather_cls32", tcode, _p(summed), _p(cls), _p(L["gptr"]), _p(L["desc"]), B, 1, L["max_npos"], with_cls, N, _p(tok_ref), st)
        tok = torch.full((rows, N), 7.0, dtype=tok_dtype, device=DEV)
        rmap = torch.empty(Nn, dtype=torch.int32, device=DEV)
        _lib.launch("gt_seq_token_rows", tcode, _p(cls) if with_cls else None, _p(L["gptr"]), _p(L["ng"]), _p(L["desc"]), B, 1, with_cls, Nn, N, _p(tok),
                    _p(rmap), st)
        _lib.launch("gt_linear_set_rows_add", _p(pe), _p(pos), N)   # (before the row map: the two compose in either order)
        _lib.launch("gt_linear_set_rows", _p(rmap))
        _lib.launch("gt_linear_fwd_ld2", GT_F32, tcode, GT_F32, _p(x), _p(W), _p(bias), _p(tok), Nn, N, K, K, N, 0, 0.0, 0, st)
        assert torch.equal(tok, tok_ref)
        # consumed: the next row-mapped call adds nothing
        tok2 = torch.full((rows, N), 7.0, dtype=tok_dtype, device=DEV)
        _lib.launch("gt_seq_token_rows", tcode, _p(cls) if with_cls else None, _p(L["gptr"]), _p(L["ng"]), _p(L["desc"]), B, 1, with_cls, Nn, N, _p(tok2),
                    _p(rmap), st)
        _lib.launch("gt_linear_set_rows", _p(rmap))
        _lib.launch("gt_linear_fwd_ld2", GT_F32, tcode, GT_F32, _p(x), _p(W), _p(bias), _p(tok2), Nn, N, K, K, N, 0, 0.0, 0, st)
        plain = torch.full((rows, N), 7.0, dtype=tok_dtype, device=DEV)
        _lib.launch("gt_seq_gather_cls32", tcode, _p(hn.to(tok_dtype)), _p(cls), _p(L["gptr"]), _p(L["desc"]), B, 1, L["max_npos"], with_cls, N, _p(plain), st)
        assert torch.equal(tok2, plain)
        # the addend without a row map is refused, and so is every backward call
        _lib.launch("gt_linear_set_rows_add", _p(pe), _p(pos), N)
        with pytest.raises(RuntimeError):
            _lib.launch("gt_linear_fwd_ld2", GT_F32, GT_F32, GT_F32, _p(x), _p(W), _p(bias), _p(hn.clone()), Nn, N, K, K, N, 0, 0.0, 0, st)
        hn2 = torch.empty_like(hn)
        _lib.launch("gt_linear_fwd_ld2", GT_F32, GT_F32, GT_F32, _p(x), _p(W), _p(bias), _p(hn2), Nn, N, K, K, N, 0, 0.0, 0, st)
        assert torch.equal(hn2, hn)
    # a GEMM without a bound image refuses the addend (and the row map), and the next plain call is unaffected
    _lib.launch("gt_linear_set_rows_add", _p(pe), _p(pos), N)
    _lib.launch("gt_linear_set_rows", _p(rmap))
    with pytest.raises(RuntimeError):
        _lib.launch("gt_linear_fwd_ld2", GT_F32, tcode, GT_F32, _p(x), _p(W), _p(bias), _p(tok), Nn, N, K, K, N, 0, 0.0, 0, st)
    hn3 = torch.empty_like(hn)
    _lib.launch("gt_linear_fwd_ld2", GT_F32, GT_F32, GT_F32, _p(x), _p(W), _p(bias), _p(hn3), Nn, N, K, K, N, 0, 0.0, 0, st)
    assert rel(hn3, hn) < 1e-5   # (the exact-fp32 kernel without the image: the same values to accumulation order, nothing added)


@pytest.mark.parametrize("tok_dtype,tol", [(torch.bfloat16, 1e-2), (torch.float32, 1e-5)])
@pytest.mark.parametrize("max_len,with_cls", [(50, 1), (7, 0)])
def test_row_map_with_layernorm_and_addend_equals_add_gather_layernorm(tok_dtype, tol, max_len, with_cls):
    """gt_linear_set_rows_layernorm + gt_linear_set_rows_add: the un-normalised token rows bit for bit, the normalised rows and the
    saved statistics against gt_layernorm_fwd on those token rows, with the assertions and bounds of
    tests/test_hip_linear3x.py::test_row_map_with_layernorm_equals_gather_then_layernorm."""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    from graphtrans_amd.w3 import W3Images
    lib = _lib.lib()
    B, K, N = 40, 256, 128
    L = _layout(_big_sizes(max_len), max_len, with_cls)
    Nn, rows = L["N"], L["rows"]
    assert Nn >= 1024 and lib.gt_linear_rows_layernorm_ok(N) == 1
    torch.manual_seed(2)
    x = torch.randn(Nn, K, device=DEV) * (0.5 + torch.rand(Nn, 1, device=DEV))
    W = torch.randn(N, K, device=DEV) / K ** 0.5
    bias, cls = torch.randn(N, device=DEV), torch.randn(N, device=DEV)
    lw, lb = torch.rand(N, device=DEV) + 0.5, torch.randn(N, device=DEV) * 0.2
    pe = torch.randn(max_len, N, device=DEV)
    tcode = GT_BF16 if tok_dtype == torch.bfloat16 else GT_F32
    pos = _positions(L, with_cls)
    imgs = W3Images([W])
    imgs.build()
    st = _stream()
    with imgs.bound():
        hn = torch.empty(Nn, N, device=DEV)
        _lib.launch("gt_linear_fwd_ld2", GT_F32, GT_F32, GT_F32, _p(x), _p(W), _p(bias), _p(hn), Nn, N, K, K, N, 0, 0.0, 0, st)
        summed = (hn + pe[pos.long().clamp(min=0)]).to(tok_dtype)
        tok_ref = torch.zeros(rows, N, dtype=tok_dtype, device=DEV)
        _lib.launch("gt_seq_gather_cls32", tcode, _p(summed), _p(cls), _p(L["gptr"]), _p(L["desc"]), B, 1, L["max_npos"], with_cls, N, _p(tok_ref), st)
        xin_ref = torch.empty_like(tok_ref)
        mean_ref, rstd_ref = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
        _lib.launch("gt_layernorm_fwd", tcode, _p(tok_ref), None, _p(lw), _p(lb), 1e-5, 0.0, 0, rows, N, _p(xin_ref), _p(mean_ref), _p(rstd_ref), st)
        tok, xin = torch.zeros(rows, N, dtype=tok_dtype, device=DEV), torch.zeros(rows, N, dtype=tok_dtype, device=DEV)
        mean, rstd = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
        rmap = torch.empty(Nn, dtype=torch.int32, device=DEV)
        _lib.launch("gt_seq_token_rows_layernorm", tcode, _p(cls) if with_cls else None, _p(L["gptr"]), _p(L["ng"]), _p(L["desc"]), B, 1, with_cls, Nn, N,
                    _p(tok), _p(rmap), _p(lw), _p(lb), 1e-5, _p(xin), _p(mean), _p(rstd), st)
        _lib.launch("gt_linear_set_rows_layernorm", _p(rmap), _p(lw), _p(lb), 1e-5, _p(xin), _p(mean), _p(rstd))
        _lib.launch("gt_linear_set_rows_add", _p(pe), _p(pos), N)
        _lib.launch("gt_linear_fwd_ld2", GT_F32, tcode, GT_F32, _p(x), _p(W), _p(bias), _p(tok), Nn, N, K, K, N, 0, 0.0, 0, st)
    assert torch.equal(tok, tok_ref)
    assert rel(mean, mean_ref) < 1e-5 and rel(rstd, rstd_ref) < 1e-5
    assert float((xin.float() - xin_ref.float()).abs().max()) <= tol * max(1.0, float(xin_ref.float().abs().max()))
    assert rel(xin.float(), xin_ref.float()) < tol * 0.1
