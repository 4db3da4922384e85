"""gt_graph_pool_fwd / gt_graph_pool_bwd (csrc/segment.hip) through the C ABI against the float64 statement below.

Forward bounds per element, n_b rows in the graph, against the float64 result on the STORED inputs (bf16 inputs are widened exactly):
  sum    |out - ref| <= n_b * 2^-24 * sum_i |x_i|        no term passes through more than n_b fp32 additions, whatever the association
                                                           (one block per graph: ceil(n_b / 4) + 2; row chunks: 64 + n_b / 64)
  mean   the sum bound / n_b + 2 * 2^-24 * |ref|           one correctly rounded division on top (its 2^-24 |ref| twice over)
  bf16   + 2^-8 * |ref|                                    the one rounding of the output (round to nearest even: half an ulp of 2^-7)
  max    bit for bit, arg = the first maximum in row order; an empty graph gives 0 and arg -1
Backward: sum and max bit for bit (copies and zeros), mean within 2 ulp of d_out / n_b (one rounded reciprocal, one rounded product);
dx starts as NaN, so an element the one pass does not write is seen.  Two runs are bit-identical, forward and backward.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
KINDS = {"sum": 1, "mean": 2, "max": 3}
UNSUPPORTED = -2
GUARD = 64          # sentinel elements behind every output: a store past the end is seen
SENT = -12345.0

# graph sizes from {0, 1, 3, 4, 5, 33, 130}: empty graphs (first, middle, last), fewer rows than the four waves, across the 32-row
# unrolled step; B = 1 and B = 7
BATCHES = {"B7": [3, 0, 130, 1, 33, 4, 5], "B7-empty-ends": [0, 33, 33, 0, 1, 130, 0], "B1-130": [130], "B1-5": [5], "B1-empty": [0]}
# the row-chunk path (N >= 4096 with a workspace): one graph of 3008 rows across 48 chunks, graph borders on and off the 64-row chunk
# borders (64, 3072, 3200, 3264 are; 3201 is not), an empty graph on a border
CHUNKED = [64, 3008, 0, 128, 1, 63, 900]
DIMS = [4, 8, 260, 300]     # 260 crosses the 256-column tile of the one-block-per-graph kernels
DT = [torch.float32, torch.bfloat16]
VALUES = ["normal", "ties", "negative"]


def _values(kind, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "normal":
        return torch.randn(N, D, generator=g)
    if kind == "ties":   # integers in [-2, 2]: equal maxima in every graph of more than a few rows
        return torch.randint(-2, 3, (N, D), generator=g).float()
    return -(torch.randn(N, D, generator=g).abs() + 0.5)   # every column negative: a max that starts from 0 fails


def _gptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def reference(x, gptr, kind):
    """float64: (out [B][D], arg [B][D] (max only), sum_i |x_i| [B][D], n [B])"""
    x = x.double().numpy()
    B, D = len(gptr) - 1, x.shape[1]
    out, arg, mag = np.zeros((B, D)), np.full((B, D), -1, np.int32), np.zeros((B, D))
    n = np.diff(gptr).astype(np.int64)
    for b in range(B):
        s = x[gptr[b]:gptr[b + 1]]
        if not len(s):
            continue
        mag[b] = np.abs(s).sum(0)
        if kind == "sum":
            out[b] = s.sum(0)
        elif kind == "mean":
            out[b] = s.sum(0) / len(s)
        else:
            a = s.argmax(0)        # the first maximum
            arg[b] = gptr[b] + a
            out[b] = s[a, np.arange(D)]
    return torch.from_numpy(out), torch.from_numpy(arg), torch.from_numpy(mag), torch.from_numpy(n)


def _code(t):
    return 0 if t.dtype == torch.float32 else 1


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def _check_guard(buf, n, fill):
    assert bool((buf[n:] == fill).all()), "a store behind the end of an output"


def pool_fwd(x, gptr_dev, B, kind, workspace=True):
    """-> (out [B][D] of x's dtype, arg [B][D] int32 or None), on the device"""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    L = _lib.lib()
    N, D = x.shape
    obuf, out = _guarded((B, D), x.dtype, SENT)
    abuf, arg = _guarded((B, D), torch.int32, -7) if kind == "max" else (None, None)
    ws, wsb = None, 0
    if workspace:
        wsb = int(L.gt_graph_pool_workspace_bytes(KINDS[kind], N, D))
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    _lib.check(L.gt_graph_pool_fwd(KINDS[kind], _code(x), x.data_ptr() if N else None, gptr_dev.data_ptr(), N, B, D, out.data_ptr(),
                                   arg.data_ptr() if arg is not None else None, ws.data_ptr() if ws is not None else None, wsb, _stream()),
               "gt_graph_pool_fwd")
    torch.cuda.synchronize()
    _check_guard(obuf, B * D, SENT)
    if abuf is not None:
        _check_guard(abuf, B * D, -7)
    return out, arg


def pool_bwd(d_out, arg, gptr_dev, ng_dev, N, kind):
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    B, D = d_out.shape
    buf, dx = _guarded((N, D), d_out.dtype, float("nan"))
    buf[N * D:] = SENT
    _lib.check(_lib.lib().gt_graph_pool_bwd(KINDS[kind], _code(d_out), d_out.data_ptr(), arg.data_ptr() if arg is not None else None,
                                            gptr_dev.data_ptr(), ng_dev.data_ptr(), N, B, D, dx.data_ptr(), _stream()), "gt_graph_pool_bwd")
    torch.cuda.synchronize()
    _check_guard(buf, N * D, SENT)
    return dx


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _ulp(ref, dtype):
    """spacing of `dtype` at |ref| (ref already holds values of that dtype)"""
    if dtype == torch.float32:
        a = ref.float().abs()
        return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()
    a = ref.double().abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def _check_case(sizes, D, dtype, values, seed, workspace=True):
    gptr = _gptr(sizes)
    N, B = int(gptr[-1]), len(sizes)
    xs = _values(values, N, D, seed).to(dtype)                 # the stored inputs
    x = xs.to(DEV)
    gptr_dev = torch.from_numpy(gptr).to(DEV)
    ng_dev = torch.repeat_interleave(torch.arange(B, dtype=torch.int32), torch.from_numpy(np.diff(gptr)).long()).to(DEV)
    worst = {}
    for kind in KINDS:
        ref, rarg, mag, n = reference(xs, gptr, kind)
        out, arg = pool_fwd(x, gptr_dev, B, kind, workspace)
        out2, arg2 = pool_fwd(x, gptr_dev, B, kind, workspace)
        assert torch.equal(_bits(out), _bits(out2)), (kind, "two forward runs differ")
        got = out.cpu().double()
        nn = n.double().reshape(-1, 1)
        if kind == "max":
            assert torch.equal(got, ref), (kind, sizes, D, float((got - ref).abs().max()))
            assert torch.equal(arg.cpu(), rarg) and torch.equal(arg, arg2), (kind, sizes, D)
        else:
            bound = nn * U * mag
            if kind == "mean":
                bound = bound / nn.clamp(min=1) + 2 * U * ref.abs()
            if dtype == torch.bfloat16:
                bound = bound + 2.0 ** -8 * ref.abs()
            err = (got - ref).abs()
            assert bool((err <= bound).all()), (kind, sizes, D, dtype, values, float((err - bound).max()))
            worst[kind] = float((err / bound.clamp(min=1e-300)).max())
        assert bool((got[n == 0] == 0).all())                  # an empty graph pools to 0 (arg -1: in rarg)
        # ---- backward
        if N == 0:
            continue
        g = torch.Generator().manual_seed(seed + 1)
        d_cpu = torch.randn(B, D, generator=g).to(dtype)
        d_out = d_cpu.to(DEV)
        dx = pool_bwd(d_out, arg, gptr_dev, ng_dev, N, kind)
        dx2 = pool_bwd(d_out, arg, gptr_dev, ng_dev, N, kind)
        assert torch.equal(_bits(dx), _bits(dx2)), (kind, "two backward runs differ")
        dxc = dx.cpu()
        assert not bool(torch.isnan(dxc).any()), (kind, "an element of dx was not written")
        rows = ng_dev.cpu().long()
        if kind == "sum":
            assert torch.equal(_bits(dxc), _bits(d_cpu[rows])), kind
        elif kind == "max":
            want = torch.where(rarg[rows].long() == torch.arange(N).reshape(-1, 1), d_cpu[rows].float(), torch.zeros(N, D)).to(dtype)
            assert torch.equal(dxc, want), kind
        else:
            want = (d_cpu[rows].double() / nn[rows].clamp(min=1)).to(dtype)   # d_out / n rounded once to the storage type
            err = (dxc.double() - want.double()).abs()
            assert bool((err <= 2 * _ulp(want, dtype)).all()), (kind, float((err / _ulp(want, dtype)).max()))
    return worst


@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", DIMS)
def test_graph_pool_one_block_per_graph(D, dtype):
    worst = {}
    for bi, (name, sizes) in enumerate(BATCHES.items()):
        for vi, values in enumerate(VALUES):
            for ws in ((True, False) if name == "B7" else (True,)):   # (a missing workspace below 4096 rows changes nothing)
                w = _check_case(sizes, D, dtype, values, 100 * bi + 10 * vi + D, ws)
                for k, v in w.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print(f"\ngt_graph_pool D={D} {dtype}: largest err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("values", VALUES)
def test_graph_pool_row_chunks_and_fixup(values, dtype):
    """N = 4164 >= 4096 with a workspace: the load-balanced row chunks and the per-graph fix-up, all three kinds; without a workspace the
    same batch runs one block per graph and must give the same maxima and rows bit for bit"""
    assert sum(CHUNKED) >= 4100 and max(CHUNKED) >= 3000
    w = _check_case(CHUNKED, 8, dtype, values, 7)
    print(f"\ngt_graph_pool row chunks {values} {dtype}: largest err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))
    _check_case(CHUNKED, 8, dtype, values, 7, workspace=False)
    _check_case(CHUNKED, 400, dtype, values, 8)   # more columns than the chunk kernels' 320 threads: their column loop runs twice


def test_graph_pool_dim_not_a_multiple_of_4_is_unsupported():
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    L = _lib.lib()
    x = torch.zeros(8, 6, device=DEV)
    gptr = torch.tensor([0, 8], dtype=torch.int32, device=DEV)
    ng = torch.zeros(8, dtype=torch.int32, device=DEV)
    out = torch.zeros(1, 6, device=DEV)
    arg = torch.zeros(1, 6, dtype=torch.int32, device=DEV)
    for kind in KINDS.values():
        assert L.gt_graph_pool_fwd(kind, 0, x.data_ptr(), gptr.data_ptr(), 8, 1, 6, out.data_ptr(), arg.data_ptr(), None, 0, _stream()) == UNSUPPORTED
        assert L.gt_graph_pool_bwd(kind, 0, out.data_ptr(), arg.data_ptr(), gptr.data_ptr(), ng.data_ptr(), 8, 1, 6, x.data_ptr(), _stream()) == UNSUPPORTED
    assert L.gt_graph_pool_fwd(9, 0, x.data_ptr(), gptr.data_ptr(), 8, 1, 8, out.data_ptr(), arg.data_ptr(), None, 0, _stream()) == -1


@pytest.mark.parametrize("kind", list(KINDS))
def test_graph_pool_autograd(kind):
    """ops.graph_pool: forward and the gradient with respect to the node rows, against the float64 statement"""
    from graphtrans_amd import ops
    from graphtrans_amd.graph import GraphStructure
    sizes = BATCHES["B7"]
    gptr = _gptr(sizes)
    N, B, D = int(gptr[-1]), len(sizes), 12
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    gs = GraphStructure.build(torch.zeros((2, 0), dtype=torch.int64, device=DEV), batch.to(DEV), num_graphs=B, sizes=np.asarray(sizes))
    xs = _values("ties" if kind == "max" else "normal", N, D, 3)
    w = torch.randn(B, D, generator=torch.Generator().manual_seed(4))
    x = xs.to(DEV).requires_grad_(True)
    out = ops.graph_pool(x, gs, kind)
    (out * w.to(DEV)).sum().backward()
    ref, rarg, mag, n = reference(xs, gptr, kind)
    assert float((out.detach().cpu().double() - ref).abs().max()) <= 1e-5
    wr = w.double()[batch]
    if kind == "mean":
        wr = wr / n.double()[batch].reshape(-1, 1)
    elif kind == "max":
        wr = torch.where(rarg[batch].long() == torch.arange(N).reshape(-1, 1), wr, torch.zeros_like(wr))
    assert float((x.grad.cpu().double() - wr).abs().max()) <= 1e-6
    with pytest.raises(ValueError):
        ops.graph_pool(x, gs, "median")
