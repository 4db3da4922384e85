"""compute = GT_COMPUTE_F32_HIGH ("high", csrc/linear3x.h): every fp32 operand counts as the sum of its first two bf16 planes and a GEMM on
a bound weight image keeps the three products (w1, a0), (w0, a1), (w0, a0).  Through the C ABI (gt_linear_fwd_ld2 / gt_linear_bwd_ld2 with
compute = 2, gt_linear_products) at the smallest shapes at which each kernel can go wrong:

* k_lin3r (M >= 12 288): ragged M, K % 32 of 4 / 0 / 12 / 16, one and two column blocks, both tile widths;
* k_lin3 below that (and the narrow dX of the first two k_lin3r shapes);
* k_lin3r_dw: both operands split on the fly.

Checked against (a) the float64 evaluation of exactly the kept products ("emu": pins the product set -- a missing first-order product
moves the result by 1.7e-3 in relative L2, the three extra products of bf16x6 by 4.4e-6, torch's fp32 GEMM sits at 1.5-3.1e-7), (b) float64
itself (2^-16; the emulated value has 4.4e-6), (c) the six-product result (the mode really engaged: >= 5 x its error), run to run, and the
default path's bits before and after.

The weight gradient at 33 x 300 x 300 is a short-M call: under compute = 0 it runs k_small_dw (gt_linear_products: 0), under "high" the
dispatcher sends the dW of such a call on a bound weight to k_lin3r_dw from 32 rows on (csrc/linear.hip: bwd_high_small_dw), two stages of
which the second holds one row; below 32 rows (the M = 8 call of the last test) nothing changes."""
import functools

import pytest
import torch

from test_hip_linear3x import rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, HIGHEST, HIGH = 0, 0, 2   # gt_dtype GT_F32; gt_compute GT_COMPUTE_F32 / GT_COMPUTE_F32_HIGH
FWD, DX, DW = 0, 1, 2          # gt_linear_products' `which`

R_SHAPES = [(12289, 132, 68), (12416, 320, 96), (13000, 600, 300), (16001, 272, 272)]   # k_lin3r
X_SHAPES = [(2048, 64, 36), (1024, 20, 132), (4100, 256, 256), (6700, 600, 300)]        # k_lin3
DW_SHAPES = [(12289, 132, 68), (1500, 20, 132), (33, 300, 300), (6700, 600, 300)]
_ids = lambda shapes: [f"{m}x{n}x{k}" for m, n, k in shapes]


def _p(t):
    return None if t is None else t.data_ptr()


def planes(t):
    """the two bf16 planes of an fp32 tensor (round to nearest even, as gt_pack_bf16), as float64"""
    t0 = t.to(torch.bfloat16).float()
    t1 = (t - t0).to(torch.bfloat16).float()   # (t - t0 is exact in fp32)
    return t0.double(), t1.double()


def kept(a, b):
    """float64 value of the three kept products of a @ b: a0 b0 + a0 b1 + a1 b0"""
    a0, a1 = planes(a)
    b0, b1 = planes(b)
    return a0 @ b0 + a0 @ b1 + a1 @ b0


@functools.lru_cache(maxsize=None)
def case(M, N, K):
    """inputs, bound-able images and the shared float64 references of one shape (computed once, never modified)"""
    from graphtrans_amd.w3 import W3Images
    torch.manual_seed(M + N + K)
    x = torch.randn(M, K, device=DEV) * (1.0 + 3.0 * torch.rand(M, 1, device=DEV))
    W = torch.randn(N, K, device=DEV) / K ** 0.5
    b = torch.randn(N, device=DEV)
    dy = torch.randn(M, N, device=DEV)
    imgs = W3Images([W])
    imgs.build()
    return dict(x=x, W=W, b=b, dy=dy, imgs=imgs)


def fwd(c, compute, act=0, bound=True, y=None, ldy=None):
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    x, W, b = c["x"], c["W"], c["b"]
    M, K = x.shape
    N = W.shape[0]
    y = torch.empty(M, N, device=DEV) if y is None else y
    call = lambda: _lib.launch("gt_linear_fwd_ld2", F32, F32, compute, _p(x), _p(W), _p(b), _p(y), M, N, K, K, ldy or N, act, 0.0, 0, _stream())
    if bound:
        with c["imgs"].bound():
            call()
    else:
        call()
    return y


def bwd(c, compute, want_dx, want_dw, add1=None, add2=None, bound=True):
    """dX (+ addends) and / or dW, db of one gt_linear_bwd_ld2 call"""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    x, W, dy = c["x"], c["W"], c["dy"]
    M, K = x.shape
    N = W.shape[0]
    dx = torch.empty(M, K, device=DEV) if want_dx else None
    dw = torch.empty(N, K, device=DEV) if want_dw else None
    db = torch.empty(N, device=DEV) if want_dw else None
    ws_bytes = _lib.lib().gt_linear_bwd_workspace_bytes(compute, M, N, K)
    assert ws_bytes == _lib.lib().gt_linear_bwd_workspace_bytes(HIGHEST, M, N, K)   # "high" sizes as fp32
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
    call = lambda: _lib.launch("gt_linear_bwd_ld2", F32, F32, compute, _p(x) if want_dw else None, _p(W), _p(dy), None, _p(add1), _p(add2), _p(dx),
                               _p(dw), _p(db), M, N, K, K, N, 0.0, _p(ws), ws_bytes, _stream())
    if bound:
        with c["imgs"].bound():
            call()
    else:
        call()
    return dx, dw, db


def products(c, which, compute, bound=True):
    from graphtrans_amd import _lib
    M, K = c["x"].shape
    N = c["W"].shape[0]
    ask = lambda: _lib.lib().gt_linear_products(which, F32, F32, compute, _p(c["W"]), M, N, K)
    if bound:
        with c["imgs"].bound():
            return ask()
    return ask()


def check(tag, run, emu, y64, t32):
    """run(compute) -> result.  The issue's five requirements on one GEMM form."""
    before = run(HIGHEST)
    hi, hi2 = run(HIGH), run(HIGH)
    after = run(HIGHEST)
    e_emu, e_t, e_hi, e_6 = rel(hi, emu), rel(t32, y64), rel(hi, y64), rel(before, y64)
    print(f"\n{tag}: high vs kept products {e_emu:.2e} (torch fp32 vs float64 {e_t:.2e});  vs float64: high {e_hi:.2e}, highest {e_6:.2e} "
          f"({e_hi / max(e_6, 1e-30):.1f} x)")
    assert e_emu <= max(3 * e_t, 1e-6), (e_emu, e_t)        # the product set, up to accumulation order
    assert e_hi <= 2.0 ** -16, e_hi
    assert e_hi >= 5 * e_6, (e_hi, e_6)                       # the mode engaged
    assert torch.equal(hi, hi2)                               # run to run
    assert torch.equal(before, after)                         # the default is untouched


@pytest.mark.parametrize("M,N,K", R_SHAPES + X_SHAPES, ids=_ids(R_SHAPES + X_SHAPES))
def test_forward(M, N, K):
    c = case(M, N, K)
    x, W, b = c["x"], c["W"], c["b"]
    assert products(c, FWD, HIGH) == 3 and products(c, FWD, HIGHEST) == 6
    emu = kept(x, W.t()) + b.double()
    y64 = torch.nn.functional.linear(x.double(), W.double(), b.double())
    check(f"fwd {M}x{N}x{K}", lambda cp: fwd(c, cp), emu, y64, torch.nn.functional.linear(x, W, b))
    # ReLU in the epilogue: the same values, gated
    e = rel(fwd(c, HIGH, act=1), torch.relu(emu))
    assert e <= max(3 * rel(torch.relu(torch.nn.functional.linear(x, W, b)), torch.relu(y64)), 1e-6), e


@pytest.mark.parametrize("M,N,K", R_SHAPES + X_SHAPES, ids=_ids(R_SHAPES + X_SHAPES))
def test_input_gradient(M, N, K):
    c = case(M, N, K)
    W, dy = c["W"], c["dy"]
    assert products(c, DX, HIGH) == 3 and products(c, DX, HIGHEST) == 6
    emu, d64, t32 = kept(dy, W), dy.double() @ W.double(), dy @ W
    check(f"dX  {M}x{N}x{K}", lambda cp: bwd(c, cp, True, False)[0], emu, d64, t32)
    torch.manual_seed(1)
    a1, a2 = torch.randn(M, K, device=DEV), torch.randn(M, K, device=DEV)
    add = a1.double() + a2.double()
    check(f"dX+ {M}x{N}x{K}", lambda cp: bwd(c, cp, True, False, a1, a2)[0], emu + add, d64 + add, t32 + a1 + a2)


@pytest.mark.parametrize("M,N,K", DW_SHAPES, ids=_ids(DW_SHAPES))
def test_weight_gradient(M, N, K):
    """(33 x 300 x 300: a short-M call -- k_small_dw under "highest", for which the predicate answers 0, k_lin3r_dw under "high")"""
    c = case(M, N, K)
    x, dy = c["x"], c["dy"]
    got = (products(c, DW, HIGH), products(c, DW, HIGHEST))
    want = (3, 6 if M > 512 else 0)   # (a short-M call is no split kernel under "highest": k_small_dw)
    print(f"\ndW {M}x{N}x{K}: gt_linear_products -> high {got[0]}, highest {got[1]}")
    emu, w64, t32 = kept(dy.t(), x), dy.double().t() @ x.double(), dy.t() @ x
    if got != want:   # (the figures of a case that is about to fail)
        hi, six = bwd(c, HIGH, False, True)[1], bwd(c, HIGHEST, False, True)[1]
        print(f"dW {M}x{N}x{K}: vs float64: high {rel(hi, w64):.2e}, highest {rel(six, w64):.2e}; high vs kept products {rel(hi, emu):.2e}")
    assert got == want, got
    check(f"dW  {M}x{N}x{K}", lambda cp: bwd(c, cp, False, True)[1], emu, w64, t32)
    # the bias gradient is a plain column sum of dY in either mode
    db = bwd(c, HIGH, False, True)[2]
    assert rel(db, dy.double().sum(0)) <= max(3 * rel(dy.sum(0), dy.double().sum(0)), 1e-6)
    # dX and dW of ONE call are those of the separate calls
    dx, dw, _ = bwd(c, HIGH, True, True)
    assert torch.equal(dx, bwd(c, HIGH, True, False)[0]) and torch.equal(dw, bwd(c, HIGH, False, True)[1])


def test_rows_past_m_and_columns_past_n_are_not_written():
    """k_lin3r under "high": the output buffer around the result keeps its canary (rows past M, columns past N, a wider pitch)"""
    M, N, K = 12289, 132, 68
    c = case(M, N, K)
    emu = kept(c["x"], c["W"].t()) + c["b"].double()
    buf = torch.full((M + 200, N), 7.0, device=DEV)
    fwd(c, HIGH, y=buf)
    torch.cuda.synchronize()
    assert bool((buf[M:] == 7.0).all())
    assert torch.equal(buf[:M], fwd(c, HIGH))
    wide = torch.full((M + 130, N + 20), 7.0, device=DEV)
    fwd(c, HIGH, y=wide, ldy=N + 20)
    torch.cuda.synchronize()
    assert bool((wide[:, N:] == 7.0).all()) and bool((wide[M:] == 7.0).all())
    assert torch.equal(wide[:M, :N], buf[:M])
    assert rel(buf[:M], emu) <= 1e-6


def test_high_without_a_three_product_kernel_is_fp32_bit_for_bit():
    """no image bound, and a short-M call: compute = 2 equals compute = 0, and the predicate says so"""
    c = case(4100, 256, 256)
    assert products(c, FWD, HIGH, bound=False) == 0 and products(c, DX, HIGH, bound=False) == 0 and products(c, DW, HIGH, bound=False) == 0
    assert torch.equal(fwd(c, HIGH, bound=False), fwd(c, HIGHEST, bound=False))
    for a, b in zip(bwd(c, HIGH, True, True, bound=False), bwd(c, HIGHEST, True, True, bound=False)):
        assert torch.equal(a, b)
    small = dict(c, x=c["x"][:8].contiguous(), dy=c["dy"][:8].contiguous())
    for which in (FWD, DX, DW):
        assert products(small, which, HIGH) == 0
    assert torch.equal(fwd(small, HIGH), fwd(small, HIGHEST))
    for a, b in zip(bwd(small, HIGH, True, True), bwd(small, HIGHEST, True, True)):
        assert torch.equal(a, b)
    # an unknown compute value is still an error
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    y = torch.empty(8, 256, device=DEV)
    rc = _lib.lib().gt_linear_fwd_ld2(F32, F32, 3, _p(small["x"]), _p(c["W"]), None, _p(y), 8, 256, 256, 256, 256, 0, 0.0, 0, _stream())
    assert rc == -1   # GT_ERR_INVALID_ARG
