"""The attention kernels reading the masked_fill predicate from keep-bits (gt_attn_fwd_bits / gt_attn_bwd_bits, ops.attention(keep_bits=)).

A. Bits against dense, same kernels: the bits of a batch (key_valid folded in) against the dense form of the same batch's bits without
   key_valid plus the key_valid mask.  Only the source of the predicate differs, the arithmetic is the same instantiation's: ctx, lse
   and d_qkv are compared with torch.equal.  T 17 (one partial word), 65 (a third word of one bit), 70 and 130 (three query tiles, five
   key steps); head dims 8, 64, 128; fp32 and bf16 rows; p = 0 and p = 0.3.  Graphs smaller than T give fully masked query rows.
B. Bits against the float64 masked_fill reference of tests/attention_refs.py at the tolerance test_hip_attention_kernels.py applies
   to its dense-mask case (attention_refs.TOL through conftest.assert_close).
C. ops.attention: keep_bits together with a dense mask raises ValueError; a layout with more positions than the bit rows hold is the
   library's GT_ERR_UNSUPPORTED (status -2); forward and backward through autograd equal the dense call's.
"""
import numpy as np
import pytest
import torch

import attention_refs as R
from adjacency_refs import random_edges
from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = R.DEV
NHEAD = 2
P = 0.3
_CACHE = {}


def _masks(T):
    """(AdjacencyBits with key_valid folded in, dense (B, T, T) of the same edges without key_valid, key_valid (B, T)), on the device"""
    if T not in _CACHE:
        from graphtrans_amd import ops
        from graphtrans_amd.graph import GraphStructure

        sizes = [T, max(1, T - 5), max(1, T // 2), 1]   # every graph but the first leaves fully masked query rows behind it
        ei = random_edges(sizes, seed=100 + T, degree=4)
        batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
        gs = GraphStructure.build(torch.from_numpy(ei).to(DEV), batch.to(DEV), num_graphs=len(sizes), sizes=sizes)
        kv = torch.ones(len(sizes), T)
        kv[0, T - T // 4:] = 0.0
        kv[2, :3] = 0.0
        kv = kv.to(DEV)
        bits = ops.adjacency_bits(gs, T, key_valid=kv, self_loops=True)
        dense = ops.adjacency_bits(gs, T, key_valid=None, self_loops=True).dense().contiguous()
        assert bool((dense * kv.reshape(len(sizes), 1, T)).sum(-1).eq(0).any()), "no fully masked row in the case"
        _CACHE[T] = (bits, dense, kv, len(sizes))
    return _CACHE[T]


def _launch(lay, dl, qkv, d_ctx, nhead, scale, p, bits=None, dense=None, kv=None, mask_value=-1e6):
    """forward and backward through the raw entries: (ctx, lse, d_qkv), NaN-prefilled"""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _ptr, _stream
    from graphtrans_amd.ops import _dtype_code

    rows, d = qkv.shape[0], qkv.shape[1] // 3
    ctx = torch.full((rows, d), R.NAN, dtype=qkv.dtype, device=DEV)
    lse = torch.full((2, nhead, rows), R.NAN, dtype=torch.float32, device=DEV)
    d_qkv = torch.full((rows, 3 * d), R.NAN, dtype=qkv.dtype, device=DEV)
    delta = torch.empty((nhead, rows), dtype=torch.float32, device=DEV)
    fwd_head = (_dtype_code(qkv), _ptr(qkv), _ptr(ctx), _ptr(lse), rows, d, nhead, _ptr(dl.desc), lay.B, lay.row_stride, lay.max_npos, None, 0)
    bwd_head = (_dtype_code(qkv), _ptr(qkv), _ptr(ctx), _ptr(d_ctx), _ptr(lse), _ptr(delta), _ptr(d_qkv), rows, d, nhead, _ptr(dl.desc), lay.B,
                lay.row_stride, lay.max_npos, None, 0)
    tail = (float(mask_value), float(scale), float(p), R.SEED, _stream())
    if bits is not None:
        _lib.launch("gt_attn_fwd_bits", *fwd_head, _ptr(bits.bits), bits.T, *tail)
        _lib.launch("gt_attn_bwd_bits", *bwd_head, _ptr(bits.bits), bits.T, *tail)
    else:
        _lib.launch("gt_attn_fwd", *fwd_head, _ptr(dense), _ptr(kv), *tail)
        _lib.launch("gt_attn_bwd", *bwd_head, _ptr(dense), _ptr(kv), *tail)
    torch.cuda.synchronize()
    return ctx, lse, d_qkv


def _same(a, b):
    return torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32), b.view(torch.int16 if b.element_size() == 2 else torch.int32))


# ---- A: bits against dense, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hd", [8, 64, 128])
@pytest.mark.parametrize("T", [17, 65, 70, 130])
def test_bits_equal_dense_masks(T, hd, dtype):
    bits, dense, kv, B = _masks(T)
    lay = R.Layout("packed", [T] * B)
    dl = R.DeviceLayout(lay)
    qkv, d_ctx = R.random_inputs(lay, NHEAD, hd, dtype, 21)
    x, g = qkv.to(DEV).to(dtype), d_ctx.to(DEV).to(dtype)
    for p in (0.0, P):
        got = _launch(lay, dl, x, g, NHEAD, hd ** -0.5, p, bits=bits)
        want = _launch(lay, dl, x, g, NHEAD, hd ** -0.5, p, dense=dense, kv=kv)
        for name, a, b in zip(("ctx", "lse", "d_qkv"), got, want):
            assert not bool(b.isnan().any()), f"{name}: the dense call left rows unwritten"
            assert _same(a, b), f"T {T} hd {hd} p {p}: {name} differs in {int((a != b).sum())} of {a.numel()} elements"


# ---- B: bits against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, P])
@pytest.mark.parametrize("inst", ["fp32-hd32", "fp32-hd48", "bf16-hd64"])
def test_bits_against_float64_reference(inst, p):
    dtype, hd = R.INSTANTIATIONS[inst]
    T = 70
    bits, dense, kv, B = _masks(T)
    lay = R.Layout("packed", [T] * B)
    qkv, d_ctx = R.random_inputs(lay, R.NHEAD, hd, dtype, 12)
    keep = R.keep_masks(lay, R.NHEAD, p, R.SEED) if p > 0 else None
    key = ("ref", inst, p)
    if key not in _CACHE:
        _CACHE[key] = R.reference(qkv, d_ctx, lay, R.NHEAD, hd ** -0.5, keep, 1.0 / (1.0 - p), dense_mask=dense.cpu(), key_valid=kv.cpu(),
                                  mask_value=-1e6)
    ref_ctx, ref_dqkv, ref_lse = _CACHE[key]
    ctx, lse, d_qkv = _launch(lay, R.DeviceLayout(lay), qkv.to(DEV).to(dtype), d_ctx.to(DEV).to(dtype), R.NHEAD, hd ** -0.5, p, bits=bits)
    tol = R.TOL[dtype]
    e = [float((a.double() - b).abs().max()) for a, b in ((ctx.float().cpu(), ref_ctx), (d_qkv.float().cpu(), ref_dqkv), (R.lse_natural(lse), ref_lse))]
    print(f"\n[bits {inst} p {p}] max abs err ctx {e[0]:.2e}, d_qkv {e[1]:.2e} (max |d_qkv| {float(ref_dqkv.abs().max()):.2f}), lse {e[2]:.2e}; tol {tol:g}")
    assert_close(ctx.float().cpu(), ref_ctx, atol=tol, rtol=tol, what="ctx")
    assert_close(d_qkv.float().cpu(), ref_dqkv, atol=tol, rtol=tol, what="d_qkv")
    # as the dense-mask case does: the fully masked rows' lse (-1e6 + log T) apart from the others', each at its own scale
    filled = ((dense * kv.reshape(B, 1, T)).sum(-1) == 0).reshape(-1).cpu()
    assert 0 < int(filled.sum()) < filled.numel()
    assert_close(R.lse_natural(lse)[:, ~filled], ref_lse[:, ~filled], atol=tol, rtol=tol, what="lse")
    assert_close(R.lse_natural(lse)[:, filled], ref_lse[:, filled], atol=tol, rtol=tol, what="lse of the fully masked rows")


# ---- C: the op ---------------------------------------------------------------------------------------------------------------------------
class _Lay:
    def __init__(self, B, T):
        ar = torch.arange(B, dtype=torch.int32, device=DEV)
        self.desc = torch.stack([ar * T, torch.full_like(ar, T), torch.zeros_like(ar), torch.full_like(ar, T)], dim=1).contiguous()
        self.B, self.row_stride, self.rows, self.max_npos = B, 1, B * T, T


def test_op_forward_backward_and_argument_errors():
    from graphtrans_amd import ops

    T, hd = 65, 16
    bits, dense, kv, B = _masks(T)
    g = torch.Generator().manual_seed(5)
    base = torch.randn(B * T, 3 * NHEAD * hd, generator=g).to(DEV)
    w = torch.randn(B * T, NHEAD * hd, generator=g).to(DEV)
    outs = []
    for kw in (dict(keep_bits=bits), dict(dense_mask=dense, key_valid=kv)):
        x = base.clone().requires_grad_(True)
        y = ops.attention(x, _Lay(B, T), NHEAD, dropout_p=P, seed=7, **kw)
        (y * w).sum().backward()
        outs.append((y.detach(), x.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    with pytest.raises(ValueError):
        ops.attention(base, _Lay(B, T), NHEAD, dense_mask=dense, keep_bits=bits)
    with pytest.raises(ValueError):
        ops.attention(base, _Lay(B, T), NHEAD, key_valid=kv, keep_bits=bits)
    longer = torch.randn(B * (T + 1), 3 * NHEAD * hd, generator=g).to(DEV)
    with pytest.raises(RuntimeError, match=r"status -2"):   # GT_ERR_UNSUPPORTED
        ops.attention(longer, _Lay(B, T + 1), NHEAD, keep_bits=bits)
