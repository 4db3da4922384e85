"""Which kernels one gt_linear_fwd* / gt_linear_bwd* call launches (csrc/linear.hip's two host dispatchers), as the launch profiler
names them (mask 32 = GT_PROF_GEMM_KERNEL: one record per GEMM kernel, forking onto the weight-gradient stream stays on), for one call
per kernel label and one per per-call request, each at the smallest shape its eligibility predicate admits -- and the results of that
call against a float64 evaluation of the same operands (1e-4 for fp32 storage and compute, 3e-2 where bf16 is involved: the bounds of
tests/test_hip_linear.py), so that a call which reaches the right kernel with a wrong argument fill fails too.  The tables are the
dispatchers' specification: a change of a row's labels is a change of behaviour."""
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GT_F32, GT_BF16 = 0, 1
BF = torch.bfloat16


def _p(t):
    return None if t is None else t.data_ptr()


def _code(t):
    return GT_BF16 if t.dtype == BF else GT_F32


def _st():
    from graphtrans_amd.graph import _stream
    return _stream()


def recorded(fn):
    """(labels of the GEMM kernels fn() launched, fn's result)"""
    from graphtrans_amd import _lib
    _lib.profile_enable(32)
    try:
        out = fn()
        names = [r[0] for r in _lib.profile_records()]
    finally:
        _lib.profile_enable(0)
    return names, out


def bound(imgs):
    import contextlib
    return imgs.bound() if imgs is not None else contextlib.nullcontext()


def w3(*weights):
    from graphtrans_amd.w3 import W3Images
    imgs = W3Images(list(weights))
    imgs.build()
    return imgs


def w1(*weights):
    from graphtrans_amd.w3 import W1Images
    imgs = W1Images(list(weights))
    imgs.build()
    return imgs


def close(got, want, tol, what):
    assert_close(got.double().cpu(), want.cpu(), atol=tol, rtol=tol, what=what)


def operands(M, N, K, xdt=torch.float32, ydt=torch.float32, seed=0):
    torch.manual_seed(1000 * seed + M + 3 * N + 7 * K)
    x = torch.randn(M, K, device=DEV).to(xdt)
    W = torch.randn(N, K, device=DEV) / K ** 0.5
    b = torch.randn(N, device=DEV)
    dy = torch.randn(M, N, device=DEV).to(ydt)
    return x, W, b, dy


def w64(W, comp):
    return (W.to(BF) if comp == GT_BF16 else W).double()


def workspace(comp, M, N, K, groups=1):
    from graphtrans_amd import _lib
    n = int(_lib.lib().gt_linear_bwd_grouped_workspace_bytes(comp, M, N, K, groups))
    return torch.empty(max(n, 16), dtype=torch.uint8, device=DEV), n


def run_fwd(x, W, b, comp, ydt, imgs=None, act=0):
    from graphtrans_amd import _lib
    M, K = x.shape
    N = W.shape[0]
    y = torch.empty(M, N, dtype=ydt, device=DEV)
    with bound(imgs):
        names, _ = recorded(lambda: _lib.launch("gt_linear_fwd_ld2", _code(x), _code(y), comp, _p(x), _p(W), _p(b), _p(y), M, N, K, K, N, act, 0.0, 0,
                                                _st()))
    return names, y


def run_bwd(x, W, dy, comp, imgs=None, ymask=None, p=0.0, a1=None, a2=None, want_dx=True, want_dw=True, before=None):
    """gt_linear_bwd_ld2; `before` (a callable) places the per-call requests in front of it"""
    from graphtrans_amd import _lib
    M, N = dy.shape
    K = W.shape[1]
    dx = torch.empty(M, K, dtype=x.dtype, device=DEV) if want_dx else None
    dw, db = (torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)) if want_dw else (None, None)
    ws, wsb = workspace(comp, M, N, K)

    def call():
        if before is not None:
            before()
        _lib.launch("gt_linear_bwd_ld2", _code(x), _code(dy), comp, _p(x), _p(W), _p(dy), _p(ymask), _p(a1), _p(a2), _p(dx), _p(dw), _p(db),
                    M, N, K, K, N, p, _p(ws), wsb, _st())
    with bound(imgs):
        names, _ = recorded(call)
    return names, dx, dw, db


def ref_bwd(x, Wd, dy, ymask=None, p=0.0, a1=None, a2=None, mul=None):
    dz = dy.double()
    if ymask is not None:
        dz = dz * (ymask > 0) / (1.0 - p)
    if mul is not None:
        dz = dz * mul.double()
    dx = dz @ Wd
    for a in (a1, a2):
        if a is not None:
            dx = dx + a.double()
    return dx, dz.t() @ x.double(), dz.sum(0)


# ---- one row per kernel label ----------------------------------------------------------------------------------------------------------
# id: (M, N, K, x storage, y storage, compute, images, forward labels, backward labels)
#   images: None, "w3" (bf16x3 images of W and W^T bound), "w1" (fragment-order bf16 images bound)
F32, B16 = torch.float32, BF
KERNELS = {
    "heads":        (17, 4096, 128, F32, F32, GT_F32, None, ["k_heads_fwd"], ["k_heads_dx+reduce", "k_small_dw"]),   # dW: the wide short-M site
    "small":        (20, 12, 8, F32, F32, GT_F32, None, ["k_small_fwd"], ["k_small_dx", "k_small_dw"]),
    "tiled":        (600, 64, 64, F32, F32, GT_F32, None, ["k_linear_fwd"], ["k_linear_dx", "k_linear_dw"]),
    "tiled-bf16":   (600, 64, 64, B16, B16, GT_BF16, None, ["k_linear_fwd"], ["k_linear_dx", "k_linear_dw"]),
    "exact-fp32":   (1025, 64, 64, F32, F32, GT_F32, None, ["k_lin32[fwd]"], ["k_lin32[dx]", "k_lin32_dw"]),
    "bf16x6":       (1025, 64, 64, F32, F32, GT_F32, "w3", ["k_lin3[fwd]"], ["k_lin3[dx]", "k_lin3r_dw"]),
    "bf16x6-bf16y": (1025, 64, 64, F32, B16, GT_F32, "w3", ["k_lin3[fwd]"], ["k_lin3[dx]", "k_lin3_dw"]),
    "bf16x6-rows":  (12289, 144, 144, F32, F32, GT_F32, "w3", ["k_lin3r[fwd]"], ["k_lin3r[dx]", "k_lin3r_dw"]),
    "stationary":   (1029, 128, 128, B16, B16, GT_BF16, "w1", ["k_lin1[fwd]"], ["k_lin1[dx]", "k_dw16"]),
    "ring-fwd":     (2049, 128, 1024, B16, B16, GT_BF16, "w1", ["k_lin2[fwd]"], ["k_lin1[dx]", "k_dw16"]),
    "ring-dx":      (2049, 1024, 128, B16, B16, GT_BF16, "w1", ["k_lin1[fwd]"], ["k_lin2[dx]", "k_dw16"]),
}


@pytest.mark.parametrize("row", list(KERNELS), ids=list(KERNELS))
def test_one_call_per_kernel_label(row):
    M, N, K, xdt, ydt, comp, images, want_fwd, want_bwd = KERNELS[row]
    x, W, b, dy = operands(M, N, K, xdt, ydt)
    imgs = {None: lambda: None, "w3": lambda: w3(W), "w1": lambda: w1(W)}[images]()
    tol = 1e-4 if (xdt, ydt, comp) == (F32, F32, GT_F32) else 3e-2
    Wd = w64(W, comp)
    names, y = run_fwd(x, W, b, comp, ydt, imgs)
    print(f"\n{row}: fwd {names}")
    assert names == want_fwd
    close(y, x.double() @ Wd.t() + b.double(), tol, "y")
    a1 = torch.randn(M, K, device=DEV).to(xdt)
    names, dx, dw, db = run_bwd(x, W, dy, comp, imgs, a1=a1)
    print(f"{row}: bwd {names}")
    assert names == want_bwd
    rdx, rdw, rdb = ref_bwd(x, Wd, dy, a1=a1)
    close(dx, rdx, tol, "dx")
    close(dw, rdw, tol, "dW")
    close(db, rdb, tol, "db")


def test_grouped_calls_on_bound_images():
    """k_lin3[fwd], k_lin3[dx] and k_lin3r_dw with blockIdx.y = group (gt_linear_fwd_grouped / gt_linear_bwd_grouped, every group's images
    bound); unbound, the same calls run the tiled kernels' grouped launches"""
    from graphtrans_amd import _lib
    M, T, K, N = 1027, 2, 36, 20
    torch.manual_seed(M)
    x = torch.randn(M, T * K, device=DEV)
    W = (torch.randn(T, N, K, device=DEV) / K ** 0.5).contiguous()
    b = torch.randn(T, N, device=DEV)
    dy = torch.randn(M, T * N, device=DEV)
    a1 = torch.randn(M, T * K, device=DEV)
    ws, wsb = workspace(GT_F32, M, N, K, T)
    imgs = w3(*[W[t] for t in range(T)])
    xd, Wd = x.double().view(M, T, K), W.double()
    for bind, want_fwd, want_bwd in ((imgs, ["k_lin3[fwd]"], ["k_lin3[dx]", "k_lin3r_dw"]), (None, ["k_linear_fwd"], ["k_linear_dx", "k_linear_dw"])):
        y, dx = torch.empty(M, T * N, device=DEV), torch.empty(M, T * K, device=DEV)
        dw, db = torch.empty(T, N, K, device=DEV), torch.empty(T, N, device=DEV)
        with bound(bind):
            nf, _ = recorded(lambda: _lib.launch("gt_linear_fwd_grouped", GT_F32, GT_F32, GT_F32, _p(x), _p(W), _p(b), _p(y), M, N, K, T * K, T * N, T, K, N,
                                                 0, 0.0, 0, _st()))
            nb, _ = recorded(lambda: _lib.launch("gt_linear_bwd_grouped", GT_F32, GT_F32, GT_F32, _p(x), _p(W), _p(dy), None, _p(a1), None, _p(dx), _p(dw),
                                                 _p(db), M, N, K, T * K, T * N, T, K, N, 0.0, _p(ws), wsb, _st()))
        print(f"\ngrouped, bound={bind is not None}: {nf} {nb}")
        assert nf == want_fwd and nb == want_bwd
        close(y, (torch.einsum("mtk,tnk->mtn", xd, Wd) + b.double()).reshape(M, T * N), 1e-4, "y")
        dyd = dy.double().view(M, T, N)
        close(dx, torch.einsum("mtn,tnk->mtk", dyd, Wd).reshape(M, T * K) + a1.double(), 1e-4, "dx")
        close(dw, torch.einsum("mtn,mtk->tnk", dyd, xd), 1e-4, "dW")
        close(db, dyd.sum(0), 1e-4, "db")


def test_layernorm_epilogues_of_the_stationary_kernel():
    """k_lin1[fwd+ln] (gt_linear_layernorm_fwd) and k_lin1[dx+lnb] (gt_linear_bwd_dx_layernorm), dropout off"""
    from graphtrans_amd import _lib
    lib = _lib.lib()
    M, N, K = 1029, 128, 128
    x, W, b, dy = operands(M, N, K, BF, BF)
    Wd = w64(W, GT_BF16)
    resid = (2.0 * torch.randn(M, N, device=DEV)).to(BF)
    g, be = 1.0 + 0.1 * torch.randn(N, device=DEV), 0.1 * torch.randn(N, device=DEV)
    imgs = w1(W)
    a, y = torch.empty(M, N, dtype=BF, device=DEV), torch.empty(M, N, dtype=BF, device=DEV)
    mu, rs = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    with imgs.bound():
        names, _ = recorded(lambda: _lib.launch("gt_linear_layernorm_fwd", GT_BF16, GT_BF16, _p(x), _p(W), _p(b), _p(a), M, N, K, _p(resid), _p(g), _p(be),
                                                1e-5, 0.0, 0, _p(y), _p(mu), _p(rs), _st()))
    assert names == ["k_lin1[fwd+ln]"]
    close(a, x.double() @ Wd.t() + b.double(), 3e-2, "a")
    z = resid.double() + a.double()
    close(y, torch.nn.functional.layer_norm(z, (N,), g.double(), be.double(), 1e-5), 3e-2, "y")
    close(mu, z.mean(1), 3e-2, "mean")
    close(rs, 1.0 / torch.sqrt(z.var(1, unbiased=False) + 1e-5), 3e-2, "rstd")
    # backward: weight [N][K], K = the LayerNorm dim; g = dY W + add1 is the gradient of LayerNorm(sub + res) * gam
    sub, res = torch.randn(M, K, device=DEV).to(BF), (2.0 * torch.randn(M, K, device=DEV)).to(BF)
    gam = 1.0 + 0.1 * torch.randn(K, device=DEV)
    a1 = torch.randn(M, K, device=DEV).to(BF)
    zz = (sub.double() + res.double()).requires_grad_(True)
    gd = gam.double().requires_grad_(True)
    mu64, rs64 = zz.detach().mean(1), 1.0 / torch.sqrt(zz.detach().var(1, unbiased=False) + 1e-5)
    mu, rs = mu64.float(), rs64.float()
    gy = dy.double() @ Wd + a1.double()
    torch.nn.functional.layer_norm(zz, (K,), gd, None, 1e-5).backward(gy)
    ds, dr = torch.empty(M, K, dtype=BF, device=DEV), torch.empty(M, K, dtype=BF, device=DEV)
    dg, dbe = torch.empty(K, device=DEV), torch.empty(K, device=DEV)
    wsb = int(lib.gt_linear_bwd_dx_layernorm_workspace_bytes(M, N, K))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    with imgs.bound():
        names, _ = recorded(lambda: _lib.launch("gt_linear_bwd_dx_layernorm", GT_BF16, GT_BF16, _p(W), _p(dy), _p(a1), None, M, N, K, _p(sub), _p(res),
                                                _p(gam), _p(mu), _p(rs), 0.0, 0, _p(ds), _p(dr), _p(dg), _p(dbe), _p(ws), wsb, _st()))
    assert names == ["k_lin1[dx+lnb]"]
    close(ds, zz.grad, 3e-2, "d_sub")
    close(dr, zz.grad, 3e-2, "d_resid")
    close(dg, gd.grad, 3e-2, "ln dW")
    close(dbe, gy.sum(0), 3e-2, "ln db")


# ---- one row per per-call request ----------------------------------------------------------------------------------------------------
def bn_operands(M, K):
    bn_x = torch.randn(M, K, device=DEV)
    mean, rstd = bn_x.mean(0).contiguous(), (1.0 / torch.sqrt(bn_x.var(0, unbiased=False) + 1e-5)).contiguous()
    return bn_x, mean, rstd, 1.0 + 0.1 * torch.randn(K, device=DEV), 0.1 * torch.randn(K, device=DEV)


def bn_ref(dx64, bn_x, mean, rstd, w, b, relu):
    xhat = (bn_x.double() - mean.double()) * rstd.double()
    d = dx64 * ((xhat * w.double() + b.double()) > 0) if relu else dx64
    return torch.stack([d.sum(0), (d * xhat).sum(0)])


@pytest.mark.parametrize("M,N,K,images,option,rows_per_part,want", [
    (1025, 64, 64, False, 0, 64, ["k_lin32[dx]"]),        # the exact kernel's epilogue
    (12289, 144, 144, True, 0, 64, ["k_lin32[dx]"]),      # a bound image does not move the request off the exact kernel ...
    (12289, 144, 144, True, 1, 128, ["k_lin3r[dx]"]),     # ... unless option "bnstats_rows_kernel" is set
], ids=["exact", "bound", "bound+option"])
def test_bnstats_request(M, N, K, images, option, rows_per_part, want):
    from graphtrans_amd import _lib
    x, W, b, dy = operands(M, N, K)
    imgs = w3(W) if images else None
    bn_x, mean, rstd, bw, bb = bn_operands(M, K)
    nparts = (M + rows_per_part - 1) // rows_per_part
    part = torch.zeros(nparts, 2, K, device=DEV)
    prev = _lib.option_set("bnstats_rows_kernel", option)
    try:
        with bound(imgs):
            assert int(_lib.lib().gt_linear_bwd_bnstats_rows_for(GT_F32, GT_F32, GT_F32, _p(W), M, N, K)) == nparts
        names, dx, _, _ = run_bwd(x, W, dy, GT_F32, imgs, want_dw=False,
                                  before=lambda: _lib.launch("gt_linear_bwd_bnstats", _p(bn_x), K, _p(mean), _p(rstd), _p(bw), _p(bb), 1, _p(part)))
    finally:
        _lib.option_set("bnstats_rows_kernel", prev)
    assert names == want
    rdx = dy.double() @ W.double()
    close(dx, rdx, 1e-4, "dx")
    close(part.double().sum(0), bn_ref(rdx, bn_x, mean, rstd, bw, bb, True), 1e-4, "BatchNorm partials")


def test_bcast_request():
    from graphtrans_amd import _lib
    M, N, K, B = 12289, 144, 144, 37
    x, W, b, dy = operands(M, N, K)
    imgs = w3(W)
    rows = torch.randn(B, K, device=DEV)
    idx = torch.sort(torch.randint(0, B, (M,), dtype=torch.int32)).values.to(DEV)
    names, dx, _, _ = run_bwd(x, W, dy, GT_F32, imgs, want_dw=False, before=lambda: _lib.launch("gt_linear_bwd_bcast", _p(rows), _p(idx)))
    assert names == ["k_lin3r[dx]"]
    close(dx, dy.double() @ W.double() + rows[idx.long()].double(), 1e-4, "dx")


def row_map(M, R):
    """GEMM row m <-> row rmap[m] of an R-row matrix, -1 for every seventh row"""
    torch.manual_seed(M + R)
    rmap = torch.randperm(R, device=DEV)[:M].to(torch.int32)
    rmap[::7] = -1
    return rmap.contiguous()


@pytest.mark.parametrize("layernorm", [False, True], ids=["rows", "rows+layernorm"])
def test_row_map_requests(layernorm):
    """gt_linear_set_rows in front of a forward and of a backward call, gt_linear_set_rows_layernorm in front of a forward call"""
    from graphtrans_amd import _lib
    M, N, K, R = 1025, 128, 64, 1100
    x, W, b, _ = operands(M, N, K)
    imgs = w3(W)
    rmap = row_map(M, R)
    kept = (rmap >= 0).nonzero().squeeze(1)
    to = rmap[kept].long()
    y = torch.zeros(R, N, device=DEV)
    lw, lb = 1.0 + 0.1 * torch.randn(N, device=DEV), 0.1 * torch.randn(N, device=DEV)
    xin, mean, rstd = torch.zeros(R, N, device=DEV), torch.zeros(R, device=DEV), torch.zeros(R, device=DEV)

    def fwd():
        if layernorm:
            _lib.launch("gt_linear_set_rows_layernorm", _p(rmap), _p(lw), _p(lb), 1e-5, _p(xin), _p(mean), _p(rstd))
        else:
            _lib.launch("gt_linear_set_rows", _p(rmap))
        _lib.launch("gt_linear_fwd_ld2", GT_F32, GT_F32, GT_F32, _p(x), _p(W), _p(b), _p(y), M, N, K, K, N, 0, 0.0, 0, _st())
    with imgs.bound():
        names, _ = recorded(fwd)
    assert names == ["k_lin3[fwd]"]
    want = torch.zeros(R, N, dtype=torch.float64, device=DEV)
    want[to] = (x.double() @ W.double().t() + b.double())[kept]
    close(y, want, 1e-4, "y")
    if layernorm:
        close(xin[to], torch.nn.functional.layer_norm(want[to], (N,), lw.double(), lb.double(), 1e-5), 1e-4, "ln_out")
        close(mean[to], want[to].mean(1), 1e-4, "ln_mean")
        close(rstd[to], 1.0 / torch.sqrt(want[to].var(1, unbiased=False) + 1e-5), 1e-4, "ln_rstd")
        return
    dtok = torch.randn(R, N, device=DEV)
    dx, dw, db = torch.empty(M, K, device=DEV), torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    ws, wsb = workspace(GT_F32, M, N, K)

    def bwd():
        _lib.launch("gt_linear_set_rows", _p(rmap))
        _lib.launch("gt_linear_bwd_ld2", GT_F32, GT_F32, GT_F32, _p(x), _p(W), _p(dtok), None, None, None, _p(dx), _p(dw), _p(db), M, N, K, K, N, 0.0,
                    _p(ws), wsb, _st())
    with imgs.bound():
        names, _ = recorded(bwd)
    assert names == ["k_lin3[dx]", "k_lin3r_dw"]
    dy = torch.zeros(M, N, dtype=torch.float64, device=DEV)
    dy[kept] = dtok.double()[to]
    rdx, rdw, rdb = ref_bwd(x, W.double(), dy)
    close(dx, rdx, 1e-4, "dx")
    close(dw, rdw, 1e-4, "dW")
    close(db, rdb, 1e-4, "db")


def test_cat2_calls():
    from graphtrans_amd import _lib
    M, N, K1, K2 = 1025, 64, 32, 36
    torch.manual_seed(5)
    x1, x2 = torch.randn(M, K1, device=DEV), torch.randn(M, K2, device=DEV)
    W, b = torch.randn(N, K1 + K2, device=DEV) / (K1 + K2) ** 0.5, torch.randn(N, device=DEV)
    dy = torch.randn(M, N, device=DEV)
    imgs = w3(W)
    y, dx1, dx2 = torch.empty(M, N, device=DEV), torch.empty_like(x1), torch.empty_like(x2)
    dw, db = torch.empty_like(W), torch.empty_like(b)
    ws, wsb = workspace(GT_F32, M, N, K1 + K2)
    with imgs.bound():
        nf, _ = recorded(lambda: _lib.launch("gt_linear_fwd_cat2", GT_F32, GT_F32, _p(x1), K1, K1, _p(x2), K2, K2, _p(W), _p(b), _p(y), M, N, N, _st()))
        nb, _ = recorded(lambda: _lib.launch("gt_linear_bwd_cat2", GT_F32, GT_F32, _p(x1), K1, K1, _p(x2), K2, K2, _p(W), _p(dy), _p(dx1), K1, _p(dx2), K2,
                                             _p(dw), _p(db), M, N, N, _p(ws), wsb, _st()))
    assert nf == ["k_lin3[fwd]"] and nb == ["k_lin3[dx]", "k_lin3r_dw"]
    cat = torch.cat([x1, x2], 1)
    close(y, cat.double() @ W.double().t() + b.double(), 1e-4, "y")
    rdx, rdw, rdb = ref_bwd(cat, W.double(), dy)
    close(torch.cat([dx1, dx2], 1), rdx, 1e-4, "dx")
    close(dw, rdw, 1e-4, "dW")
    close(db, rdb, 1e-4, "db")


def test_gate_out_call():
    """gt_linear_bwd_gate_out: the gate on the dX OUTPUT, the weight gradient from the ungated dY"""
    from graphtrans_amd import _lib
    M, N, K, p = 1029, 128, 128, 0.3
    _, W, _, dy = operands(M, N, K, BF, BF)
    f1 = (torch.relu(torch.randn(M, K, device=DEV)) * (torch.rand(M, K, device=DEV) > p)).to(BF)
    a1 = torch.randn(M, K, device=DEV).to(BF)
    imgs = w1(W)
    dx, dw, db = torch.empty(M, K, dtype=BF, device=DEV), torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    ws, wsb = workspace(GT_BF16, M, N, K)
    with imgs.bound():
        names, _ = recorded(lambda: _lib.launch("gt_linear_bwd_gate_out", GT_BF16, GT_BF16, GT_BF16, _p(f1), _p(W), _p(dy), _p(f1), _p(a1), None, _p(dx),
                                                _p(dw), _p(db), M, N, K, K, N, p, _p(ws), wsb, _st()))
    assert names == ["k_lin1[dx]", "k_dw16"]
    g = dy.double() @ w64(W, GT_BF16)
    close(dx, g * (f1 > 0) / (1.0 - p) + a1.double(), 3e-2, "dx")    # (the addends join behind the gate)
    close(dw, dy.double().t() @ f1.double(), 3e-2, "dW")
    close(db, dy.double().sum(0), 3e-2, "db")


def test_mul_call():
    """gt_linear_bwd_mul: dZ = dY * gmul for dX, dW and db"""
    from graphtrans_amd import _lib
    M, N, K = 600, 64, 64
    x, W, _, dy = operands(M, N, K)
    gm = torch.rand(M, N, device=DEV)
    dx, dw, db = torch.empty(M, K, device=DEV), torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    ws, wsb = workspace(GT_F32, M, N, K)
    names, _ = recorded(lambda: _lib.launch("gt_linear_bwd_mul", GT_F32, GT_F32, GT_F32, _p(x), _p(W), _p(dy), _p(gm), None, None, _p(dx), _p(dw), _p(db),
                                            M, N, K, K, N, _p(ws), wsb, _st()))
    assert names == ["k_linear_dx", "k_linear_dw"]
    rdx, rdw, rdb = ref_bwd(x, W.double(), dy, mul=gm)
    close(dx, rdx, 1e-4, "dx")
    close(dw, rdw, 1e-4, "dW")
    close(db, rdb, 1e-4, "db")


@pytest.mark.parametrize("given", [False, True], ids=["no-weight_t", "weight_t"])
def test_wt_call(given):
    """gt_linear_bwd_wt: the exact kernel's dX reads the caller's W^T when there is one (here the transpose of ANOTHER matrix, so that
    the result tells which one was read), the weight gradient does not"""
    from graphtrans_amd import _lib
    M, N, K = 1025, 64, 64
    x, W, _, dy = operands(M, N, K)
    other = torch.randn(N, K, device=DEV) / K ** 0.5
    wt = other.t().contiguous()
    dx, dw, db = torch.empty(M, K, device=DEV), torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    ws, wsb = workspace(GT_F32, M, N, K)
    names, _ = recorded(lambda: _lib.launch("gt_linear_bwd_wt", GT_F32, GT_F32, GT_F32, _p(x), _p(W), _p(wt) if given else None, _p(dy), None, None, None,
                                            _p(dx), _p(dw), _p(db), M, N, K, 0.0, _p(ws), wsb, _st()))
    assert names == ["k_lin32[dx]", "k_lin32_dw"]
    _, rdw, rdb = ref_bwd(x, W.double(), dy)
    close(dx, dy.double() @ (other if given else W).double(), 1e-4, "dx")
    close(dw, rdw, 1e-4, "dW")
    close(db, rdb, 1e-4, "db")


@pytest.mark.parametrize("M,want", [(1025, ["k_lin32_dw"]), (20, ["k_small_dw"])], ids=["exact-fp32", "small"])
def test_dw_forked_call_inside_an_overlap_section(M, want):
    """gt_linear_bwd_dw_forked between gt_overlap_dw_begin and _end: the weight gradient alone, on the section's side stream"""
    from graphtrans_amd import _lib
    lib = _lib.lib()
    N, K = 64, 64
    x, W, _, dy = operands(M, N, K)
    yf = torch.relu(torch.randn(M, N, device=DEV))
    dw, db = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    ws, wsb = workspace(GT_F32, M, N, K)
    side = lib.gt_stream_create(0)
    assert side
    torch.cuda.synchronize()
    _lib.launch("gt_overlap_dw_begin", _st(), side)
    try:
        names, _ = recorded(lambda: _lib.launch("gt_linear_bwd_dw_forked", GT_F32, GT_F32, GT_F32, _p(x), _p(W), _p(dy), _p(yf), _p(dw), _p(db), M, N, K, K, N,
                                                0.2, _p(ws), wsb, _st()))
    finally:
        _lib.launch("gt_overlap_dw_end")
        torch.cuda.synchronize()
        lib.gt_stream_destroy(side)
    assert names == want
    _, rdw, rdb = ref_bwd(x, W.double(), dy, ymask=yf, p=0.2)
    close(dw, rdw, 1e-4, "dW")
    close(db, rdb, 1e-4, "db")


# ---- how long a request lives ---------------------------------------------------------------------------------------------------------
def test_a_request_does_not_outlive_a_call_that_fails_validation():
    """gt_linear_bwd_bnstats / gt_linear_bwd_bcast followed by a backward call that is refused (ldy < N): the next, valid call runs
    without the request (tests/test_hip_linear3x.py has the same for the row map)"""
    from graphtrans_amd import _lib
    M, N, K = 12289, 144, 144
    x, W, b, dy = operands(M, N, K)
    imgs = w3(W)
    bn_x, mean, rstd, bw, bb = bn_operands(M, K)
    part = torch.full(((M + 63) // 64, 2, K), 7.0, device=DEV)
    rows, idx = torch.randn(5, K, device=DEV), torch.zeros(M, dtype=torch.int32, device=DEV)
    dx = torch.empty(M, K, device=DEV)
    ws, wsb = workspace(GT_F32, M, N, K)
    call = lambda ldy: _lib.launch("gt_linear_bwd_ld2", GT_F32, GT_F32, GT_F32, None, _p(W), _p(dy), None, None, None, _p(dx), None, None, M, N, K, K, ldy, 0.0,
                                   _p(ws), wsb, _st())
    with imgs.bound():
        _lib.launch("gt_linear_bwd_bnstats", _p(bn_x), K, _p(mean), _p(rstd), _p(bw), _p(bb), 0, _p(part))
        _lib.launch("gt_linear_bwd_bcast", _p(rows), _p(idx))
        with pytest.raises(RuntimeError):
            call(N - 4)
        names, _ = recorded(lambda: call(N))
    assert names == ["k_lin3r[dx]"]           # (with the statistics request it would have been the exact kernel)
    close(dx, dy.double() @ W.double(), 1e-4, "dx")
    assert bool((part == 7.0).all())


def test_a_forward_call_leaves_a_backward_request_in_place():
    """a forward call between gt_linear_bwd_bnstats and the backward call it is meant for: the backward still takes the request"""
    from graphtrans_amd import _lib
    M, N, K = 1025, 64, 64
    x, W, b, dy = operands(M, N, K)
    bn_x, mean, rstd, bw, bb = bn_operands(M, K)
    part = torch.zeros((M + 63) // 64, 2, K, device=DEV)
    y = torch.empty(M, N, device=DEV)

    def before():
        _lib.launch("gt_linear_bwd_bnstats", _p(bn_x), K, _p(mean), _p(rstd), _p(bw), _p(bb), 0, _p(part))
        _lib.launch("gt_linear_fwd_ld2", GT_F32, GT_F32, GT_F32, _p(x), _p(W), _p(b), _p(y), M, N, K, K, N, 0, 0.0, 0, _st())
    names, dx, _, _ = run_bwd(x, W, dy, GT_F32, None, want_dw=False, before=before)
    assert names == ["k_lin32[fwd]", "k_lin32[dx]"]
    rdx = dy.double() @ W.double()
    close(dx, rdx, 1e-4, "dx")
    close(part.double().sum(0), bn_ref(rdx, bn_x, mean, rstd, bw, bb, False), 1e-4, "BatchNorm partials")
