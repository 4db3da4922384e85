"""The PNA baseline's head kernels (csrc/mlp_heads.hip) against float64 references computed here, on the CPU.

Grouped output layer (gt_head_group_*): fp32 compute against float64 within F32_TOL on max-scaled tensors; bf16 compute against float64
evaluated on operands first rounded to bf16 (round-to-nearest-even, as gt_pack_bf16) -- the products of two bf16 values are exact in
fp32, what is left is fp32 accumulation, so the same F32_TOL applies.  dbias has no product: it is the fp32 column sum of dY as stored,
in both modes.  The pad columns [G*T, ldy) of Y keep a sentinel; the backward takes a ReLU output as H, so kernel and reference gate
on the same values; two runs give the same bits.

Narrow MLP (gt_head_mlp_*): plain fp32 against float64 within F32_TOL; the backward reference gates with the kernel's own saved
activations (a value that rounds to the other side of 0 in fp32 would otherwise flip a gate).
"""
import ctypes as C

import pytest
import torch

from test_hip_gnn_baseline import F32_TOL, _close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GT_F32, GT_BF16 = 0, 1
INVALID, UNSUPPORTED = -1, -2
SENTINEL = -12345.0


def _c4(n):
    return (n + 3) // 4 * 4


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    from graphtrans_amd.graph import _stream
    return _stream()


def _rnd(t, bf16):
    return t.bfloat16().double() if bf16 else t.double()


def _group_fwd(compute, H, W, b, G, K, T, ldy):
    from graphtrans_amd import _lib
    M = H.shape[0]
    Y = torch.full((M, ldy), SENTINEL, dtype=torch.float32, device=DEV)
    _lib.launch("gt_head_group_fwd", compute, _p(H), H.stride(0), _p(W), _p(b), _p(Y), ldy, M, G, K, T, _st())
    return Y


def _group_bwd(compute, H, W, dY, G, K, T):
    from graphtrans_amd import _lib
    M = H.shape[0]
    dH = torch.full_like(H, SENTINEL)
    dW = torch.full_like(W, SENTINEL)
    db = torch.full((G * T,), SENTINEL, dtype=torch.float32, device=DEV)
    wsb = _lib.lib().gt_head_group_workspace_bytes(M, G, K, T)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
    _lib.launch("gt_head_group_bwd", compute, _p(H), H.stride(0), _p(W), _p(dY), dY.stride(0), 1, _p(dH), dH.stride(0), _p(dW), _p(db),
                M, G, K, T, _p(ws), wsb, _st())
    return dH, dW, db


GROUP_SHAPES = [(1, 1, 16, 1), (12, 3, 48, 37), (70, 5, 272, 50), (300, 2, 64, 129), (16, 5, 272, 5002)]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,G,K,T", GROUP_SHAPES, ids=["x".join(map(str, s)) for s in GROUP_SHAPES])
def test_head_group_vs_float64(M, G, K, T, bf16):
    g = torch.Generator().manual_seed(M * 7 + T)
    H = torch.relu(torch.randn(M, G * K, generator=g))            # a ReLU output: exact zeros where the gate closes
    W = torch.randn(G * T, K, generator=g) / K ** 0.5
    b = torch.randn(G * T, generator=g)
    dY = torch.randn(M, G * T, generator=g)
    compute = GT_BF16 if bf16 else GT_F32
    Hr, Wr, dYr = (_rnd(t, bf16).view(*s) for t, s in ((H, (M, G, K)), (W, (G, T, K)), (dY, (M, G, T))))
    ref_Y = (torch.einsum("mgk,gtk->mgt", Hr, Wr) + b.double().view(G, T)).reshape(M, G * T)
    ref_dH = (torch.einsum("mgt,gtk->mgk", dYr, Wr) * (H.view(M, G, K) > 0)).reshape(M, G * K)
    ref_dW = torch.einsum("mgt,mgk->gtk", dYr, Hr).reshape(G * T, K)
    ref_db = dY.double().sum(0)                                     # no product: the column sum of dY as stored
    Hd, Wd, bd = torch.zeros(M, G * K + 8).to(DEV)[:, :G * K].copy_(H), W.to(DEV), b.to(DEV)   # H as a column slice of wider rows (ldh > G*K)
    N = G * T
    for ldy in (_c4(N), _c4(N) + 8):
        Y = _group_fwd(compute, Hd, Wd, bd, G, K, T, ldy)
        assert bool((Y[:, N:] == SENTINEL).all()), "pad columns written"
        _close(ref_Y.float(), Y[:, :N].cpu(), F32_TOL, f"Y ldy={ldy}")
        assert torch.equal(Y, _group_fwd(compute, Hd, Wd, bd, G, K, T, ldy))
    dYd = torch.full((M, _c4(N) + 4), float("nan"), dtype=torch.float32, device=DEV)   # NaN pad columns: never read
    dYd[:, :N] = dY.to(DEV)
    dH, dW, db = _group_bwd(compute, Hd, Wd, dYd, G, K, T)
    _close(ref_dH.float(), dH.cpu(), F32_TOL, "dH")
    _close(ref_dW.float(), dW.cpu(), F32_TOL, "dW")
    _close(ref_db.float(), db.cpu(), F32_TOL, "dbias")
    assert bool(((dH == 0) | (Hd > 0)).all())                        # the gate is exact
    again = _group_bwd(compute, Hd, Wd, dYd, G, K, T)
    for a, c, what in zip((dH, dW, db), again, ("dH", "dW", "dbias")):
        assert torch.equal(a, c), what


MLP_SHAPES = [(1, 16, 1, 35, 17), (5, 16, 2, 35, 17), (70, 272, 128, 35, 17), (257, 64, 3, 35, 17), (5, 16, 2, 64, 64)]


@pytest.mark.parametrize("M,D,T,H1,H2", MLP_SHAPES, ids=["x".join(map(str, s)) for s in MLP_SHAPES])
def test_head_mlp_vs_float64(M, D, T, H1, H2):
    from graphtrans_amd import _lib
    g = torch.Generator().manual_seed(M + D + T)
    x = torch.randn(M, D, generator=g)
    W1, b1 = torch.randn(H1, D, generator=g) / D ** 0.5, torch.randn(H1, generator=g) * 0.3
    W2, b2 = torch.randn(H2, H1, generator=g) / H1 ** 0.5, torch.randn(H2, generator=g) * 0.3
    W3, b3 = torch.randn(T, H2, generator=g) / H2 ** 0.5, torch.randn(T, generator=g) * 0.3
    dy = torch.randn(M, T, generator=g)
    dev = [t.to(DEV) for t in (x, W1, b1, W2, b2, W3, b3)]
    xd, W1d, b1d, W2d, b2d, W3d, b3d = dev

    def fwd():
        a1 = torch.full((M, H1), SENTINEL, device=DEV)
        a2 = torch.full((M, H2), SENTINEL, device=DEV)
        y = torch.full((M, T), SENTINEL, device=DEV)
        _lib.launch("gt_head_mlp_fwd", GT_F32, _p(xd), D, _p(W1d), _p(b1d), _p(W2d), _p(b2d), _p(W3d), _p(b3d), _p(a1), _p(a2), _p(y), T, M, D,
                    H1, H2, T, _st())
        return a1, a2, y
    a1, a2, y = fwd()
    r1 = torch.relu(x.double() @ W1.double().t() + b1.double())
    r2 = torch.relu(r1 @ W2.double().t() + b2.double())
    ry = r2 @ W3.double().t() + b3.double()
    _close(r1.float(), a1.cpu(), F32_TOL, "a1")
    _close(r2.float(), a2.cpu(), F32_TOL, "a2")
    _close(ry.float(), y.cpu(), F32_TOL, "y")
    for a, c in zip((a1, a2, y), fwd()):
        assert torch.equal(a, c)
    dyd = dy.to(DEV)

    def bwd():
        outs = [torch.full(s, SENTINEL, device=DEV) for s in ((M, D), (H1, D), (H1,), (H2, H1), (H2,), (T, H2), (T,))]
        wsb = _lib.lib().gt_head_mlp_workspace_bytes(M, H1, H2)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
        _lib.launch("gt_head_mlp_bwd", GT_F32, _p(xd), D, _p(W1d), _p(W2d), _p(W3d), _p(a1), _p(a2), _p(dyd), T, _p(outs[0]), D,
                    *[_p(t) for t in outs[1:]], M, D, H1, H2, T, _p(ws), wsb, _st())
        return outs
    got = bwd()
    m1, m2 = (a1.cpu() > 0).double(), (a2.cpu() > 0).double()       # the kernel's own gates
    d2 = (dy.double() @ W3.double()) * m2
    d1 = (d2 @ W2.double()) * m1
    refs = [d1 @ W1.double(), d1.t() @ x.double(), d1.sum(0), d2.t() @ r1, d2.sum(0), dy.double().t() @ r2, dy.double().sum(0)]
    for r, o, what in zip(refs, got, ("dx", "dW1", "db1", "dW2", "db2", "dW3", "db3")):
        _close(r.float(), o.cpu(), F32_TOL, what)
    for a, c in zip(got, bwd()):
        assert torch.equal(a, c)


def test_bad_arguments_are_rejected_with_a_message():
    from graphtrans_amd import _lib
    L = _lib.lib()
    M, G, T = 4, 2, 5
    buf = torch.full((4096,), SENTINEL, device=DEV)
    y = torch.full((M, 64), SENTINEL, device=DEV)

    def group(K, ldy):
        return L.gt_head_group_fwd(GT_F32, _p(buf), G * K, _p(buf), _p(buf), _p(y), ldy, M, G, K, T, _st())

    def mlp(H1):
        return L.gt_head_mlp_fwd(GT_F32, _p(buf), 16, _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), _p(y), 8, M, 16, H1,
                                 17, T, _st())
    for call, want in ((lambda: group(24, 12), UNSUPPORTED), (lambda: group(528, 12), UNSUPPORTED), (lambda: group(16, 8), INVALID),
                       (lambda: mlp(65), UNSUPPORTED)):
        rc = call()
        assert rc == want and L.gt_last_error().decode(), rc
    dh = torch.full((M, G * 24), SENTINEL, device=DEV)
    rc = L.gt_head_group_bwd(GT_F32, _p(buf), G * 24, _p(buf), _p(buf), 12, 1, _p(dh), G * 24, None, None, M, G, 24, T, _p(buf), 4096 * 4, _st())
    assert rc == UNSUPPORTED and L.gt_last_error().decode()
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((dh == SENTINEL).all()) and bool((buf == SENTINEL).all())   # nothing was launched
