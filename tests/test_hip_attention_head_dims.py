"""The fused attention kernels at every kind of head dim the library accepts (multiples of 8 up to 128): below 32 (24), between
32 and 64 (48), above 64 with a partial last 32-deep step (96 is whole, 128 is whole; 48 and 24 are padded) -- against the float64
CPU reference of tests/test_hip_attention.py, in both storage types and token layouts, with dropout, through the pooled entry
points, with dense masked_fill masks, plus the gt_attn_head_dim_ok query.

Tolerances are the op's own (tests/test_hip_attention.py): 1e-4 for fp32 rows, 2e-2 for bf16 rows, atol = rtol."""
import pytest
import torch

from conftest import assert_close
from test_hip_attention import make_layout, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hd", [24, 48, 64, 96, 128])
@pytest.mark.parametrize("kind", ["packed", "padded"])
def test_attention_fwd_bwd_head_dims(dtype, hd, kind):
    """tests/test_hip_attention.py:test_attention_fwd_bwd at the new head dims (64 is the control), nhead 2."""
    from graphtrans_amd import ops

    torch.manual_seed(0)
    nhead, tol = 2, TOL[dtype]
    d = nhead * hd
    lens = [1, 7, 33, 64, 65, 130, 31, 32]
    lay = make_layout(kind, lens)
    qkv = torch.randn(lay.rows, 3 * d)
    w = torch.randn(lay.rows, d)
    qkv_q = qkv.to(dtype).float()  # the reference sees the same (rounded) inputs
    ref_in = qkv_q.clone().requires_grad_(True)
    ref = reference(ref_in, lay, nhead, hd ** -0.5)
    (ref * w.double()).sum().backward()
    x = qkv.to(DEV).to(dtype).requires_grad_(True)
    out = ops.attention(x, lay, nhead)
    (out.float() * w.to(DEV)).sum().backward()
    e_out = float((out.detach().float().cpu().double() - ref.detach()).abs().max())
    e_dqkv = float((x.grad.float().cpu().double() - ref_in.grad).abs().max())
    print(f"\n[hd {hd} {dtype} {kind}] max abs err ctx {e_out:.2e}, d_qkv {e_dqkv:.2e} (max |d_qkv| {float(ref_in.grad.abs().max()):.2f}); tol {tol:g}")
    assert_close(out.float().cpu(), ref.detach(), atol=tol, rtol=tol, what="ctx")
    assert_close(x.grad.float().cpu(), ref_in.grad, atol=tol, rtol=tol, what="d_qkv")


def test_attention_long_sequences_fp32_head_dim_128():
    """S = 1001 and 517 at head dim 128: 32 key tiles, online-softmax rescaling.  Inputs x 2.0 (the head-dim-32 test uses x 3.0):
    at head dim 128 the scores are sums of 128 products, and at x 3.0 plain fp32 torch on the CPU alone already uses 66-81 % of the
    1e-4 tolerance on d_qkv; at x 2.0 it uses 12-15 % while the scores still spread (standard deviation 4)."""
    from graphtrans_amd import ops

    torch.manual_seed(1)
    nhead, hd = 2, 128
    d = nhead * hd
    lay = make_layout("packed", [1001, 517])
    qkv = torch.randn(lay.rows, 3 * d) * 2.0
    ref_in = qkv.clone().requires_grad_(True)
    w = torch.randn(lay.rows, d)
    ref = reference(ref_in, lay, nhead, hd ** -0.5)
    (ref * w.double()).sum().backward()
    x = qkv.to(DEV).requires_grad_(True)
    out = ops.attention(x, lay, nhead)
    (out * w.to(DEV)).sum().backward()
    print(f"\n[long hd 128] max abs err ctx {float((out.cpu().double() - ref.detach()).abs().max()):.2e}, "
          f"d_qkv {float((x.grad.cpu().double() - ref_in.grad).abs().max()):.2e} (max |d_qkv| {float(ref_in.grad.abs().max()):.2f})")
    assert_close(out.cpu(), ref.detach(), what="ctx")
    assert_close(x.grad.cpu(), ref_in.grad, what="d_qkv")


def _keep_masks(hd, nhead, lens, p, seed, dtype):
    """the dropout keep mask per (sequence, head), recovered with one-hot V rows (q = k = 0 -> uniform weights 1 / n)"""
    from graphtrans_amd import ops

    d = nhead * hd
    lay = make_layout("packed", lens)
    probe = torch.zeros(lay.rows, 3 * d)
    for row0, npos, _, _ in lay.desc_cpu:
        for j in range(npos):
            for h in range(nhead):
                probe[row0 + j, 2 * d + h * hd + j] = 1.0
    got = ops.attention(probe.to(DEV).to(dtype), lay, nhead, dropout_p=p, seed=seed).float().cpu()
    keep = {}
    for b, (row0, npos, _, _) in enumerate(lay.desc_cpu):
        for h in range(nhead):
            blk = got[row0:row0 + npos, h * hd:h * hd + npos]
            keep[(b, h)] = blk > 0
            vals = blk[keep[(b, h)]]
            # 1 / (n (1 - p)) computed in fp32 and stored as bf16: one rounding, 2^-9 relative
            assert torch.allclose(vals, torch.full_like(vals, 1.0 / npos / (1 - p)), rtol=2.0 ** -8)
            assert float(got[row0:row0 + npos, h * hd + npos:(h + 1) * hd].abs().max() if npos < hd else 0.0) == 0.0
    return lay, keep


@pytest.mark.parametrize("hd", [128, 48])
def test_attention_dropout_replay_bf16_head_dims(hd):
    """tests/test_hip_attention.py:test_attention_dropout_replay_and_rate in bf16 at head dims 128 and 48, and bitwise
    run-to-run reproducibility of d_qkv with dropout on."""
    from graphtrans_amd import ops

    torch.manual_seed(2)
    nhead, p, seed, dt = 2, 0.3, 1234567, torch.bfloat16
    d = nhead * hd
    lens = [48, 17, 5]
    lay, keep = _keep_masks(hd, nhead, lens, p, seed, dt)
    kept = sum(int(m.sum()) for m in keep.values())
    total = sum(m.numel() for m in keep.values())
    assert abs(kept / total - (1 - p)) < 0.05
    qkv = torch.randn(lay.rows, 3 * d).to(dt).float()
    w = torch.randn(lay.rows, d)
    ref_in = qkv.clone().requires_grad_(True)
    ref = reference(ref_in, lay, nhead, hd ** -0.5, keep, 1.0 / (1 - p))
    (ref * w.double()).sum().backward()
    grads = []
    for _ in range(2):
        x = qkv.to(DEV).to(dt).requires_grad_(True)
        out = ops.attention(x, lay, nhead, dropout_p=p, seed=seed)
        (out.float() * w.to(DEV)).sum().backward()
        grads.append(x.grad.clone())
    assert torch.equal(grads[0], grads[1])
    assert_close(out.float().cpu(), ref.detach(), atol=2e-2, rtol=2e-2, what="ctx (dropout)")
    assert_close(grads[0].float().cpu(), ref_in.grad, atol=2e-2, rtol=2e-2, what="d_qkv (dropout)")
    again = ops.attention(x.detach(), lay, nhead, dropout_p=p, seed=seed)
    other = ops.attention(x.detach(), lay, nhead, dropout_p=p, seed=seed + 1)
    assert torch.equal(again, out.detach()) and not torch.equal(other, out.detach())


def test_dropout_decisions_do_not_depend_on_the_head_dim():
    """keep(seed, sequence, head, query, key) is a function of the position: the same mask at head dim 128, 64 and 48"""
    nhead, p, seed, lens = 2, 0.3, 1234567, [48, 17, 5]
    _, k128 = _keep_masks(128, nhead, lens, p, seed, torch.bfloat16)
    _, k64 = _keep_masks(64, nhead, lens, p, seed, torch.bfloat16)
    _, k48 = _keep_masks(48, nhead, lens, p, seed, torch.bfloat16)
    for key in k64:
        assert torch.equal(k128[key], k64[key]) and torch.equal(k48[key], k64[key]), key


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hd", [128, 48])
def test_pooled_entry_points_agree_with_the_full_kernels(dtype, hd):
    """gt_attn_fwd_last / gt_attn_bwd_last: ctx on the last row of every sequence, and d_qkv for a d_ctx that is zero outside the
    last rows, against gt_attn_fwd / gt_attn_bwd on the same inputs."""
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _ptr, _stream
    from graphtrans_amd.ops import _dtype_code

    torch.manual_seed(5)
    nhead, tol = 2, TOL[dtype]
    d = nhead * hd
    lens = [1, 7, 33, 64, 65, 130, 31, 32, 200]
    lay = make_layout("packed", lens)
    rows = lay.rows
    last = torch.tensor([r0 + n - 1 for r0, n, _, _ in lay.desc_cpu], device=DEV)
    qkv = torch.randn(rows, 3 * d).to(DEV).to(dtype)
    d_ctx = torch.zeros(rows, d, device=DEV, dtype=dtype)
    d_ctx[last] = torch.randn(len(lens), d, device=DEV).to(dtype)
    scale, code = hd ** -0.5, _dtype_code(qkv)
    ctx_full = torch.zeros(rows, d, device=DEV, dtype=dtype)
    lse_full = torch.zeros(2, nhead, rows, device=DEV)
    _lib.launch("gt_attn_fwd", code, _ptr(qkv), _ptr(ctx_full), _ptr(lse_full), rows, d, nhead, _ptr(lay.desc), lay.B, lay.row_stride,
                lay.max_npos, None, 0, None, None, 0.0, scale, 0.0, 0, _stream())
    ctx_last = torch.zeros(rows, d, device=DEV, dtype=dtype)
    lse_last = torch.zeros(2, nhead, rows, device=DEV)
    _lib.launch("gt_attn_fwd_last", code, _ptr(qkv), _ptr(ctx_last), _ptr(lse_last), rows, d, nhead, _ptr(lay.desc), lay.B, lay.row_stride,
                lay.max_npos, scale, 0.0, 0, _stream())
    assert_close(ctx_last[last].float().cpu(), ctx_full[last].float().cpu(), atol=tol, rtol=tol, what="pooled ctx")
    dq_full = torch.zeros(rows, 3 * d, device=DEV, dtype=dtype)
    delta = torch.zeros(nhead, rows, device=DEV)
    _lib.launch("gt_attn_bwd", code, _ptr(qkv), _ptr(ctx_full), _ptr(d_ctx), _ptr(lse_full), _ptr(delta), _ptr(dq_full), rows, d, nhead,
                _ptr(lay.desc), lay.B, lay.row_stride, lay.max_npos, None, 0, None, None, 0.0, scale, 0.0, 0, _stream())
    dq_last = torch.zeros(rows, 3 * d, device=DEV, dtype=dtype)   # (the pooled backward asks for a zero-filled d_qkv)
    delta2 = torch.zeros(nhead, rows, device=DEV)
    _lib.launch("gt_attn_bwd_last", code, _ptr(qkv), _ptr(ctx_last), _ptr(d_ctx), _ptr(lse_last), _ptr(delta2), _ptr(dq_last), rows, d, nhead,
                _ptr(lay.desc), lay.B, lay.row_stride, lay.max_npos, None, 0, scale, 0.0, 0, _stream())
    torch.cuda.synchronize()
    assert float(dq_full.float().abs().max()) > 0
    assert_close(dq_last.float().cpu(), dq_full.float().cpu(), atol=tol, rtol=tol, what="pooled d_qkv")


def _masked_fill_reference(qkv, B, T, nhead, scale, dense_mask, key_valid, mask_value=-1e6):
    """CausalSelfAttention's core (modules/masked_transformer_encoder.py): masked_fill(mask == 0, mask_value), softmax, . V"""
    qkv = qkv.double()
    d = qkv.shape[1] // 3
    hd = d // nhead
    x = qkv.view(B, T, 3, nhead, hd)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))          # (B, nh, T, hd)
    att = (q @ k.transpose(-2, -1)) * scale
    if dense_mask is not None:
        att = att.masked_fill(dense_mask.view(B, 1, T, T) == 0, mask_value)
    if key_valid is not None:
        att = att.masked_fill(key_valid.view(B, 1, 1, T) == 0, mask_value)
    y = torch.softmax(att, dim=-1) @ v
    return y.transpose(1, 2).reshape(B * T, d)


def test_dense_masks_fp32_head_dim_128():
    """ops.attention(..., dense_mask=, key_valid=) at head dim 128, fp32, against the masked_fill(-1e6) reference"""
    from graphtrans_amd import ops

    torch.manual_seed(6)
    B, T, nhead, hd = 3, 70, 2, 128
    d = nhead * hd
    lay = make_layout("packed", [T] * B)
    qkv = torch.randn(B * T, 3 * d)
    w = torch.randn(B * T, d)
    dense = (torch.rand(B, T, T) < 0.6).float()
    dense[1, 5] = 0.0                        # a fully masked row: uniform weights
    valid = torch.ones(B, T)
    valid[0, 50:] = 0.0
    valid[2, :3] = 0.0
    ref_in = qkv.clone().requires_grad_(True)
    ref = _masked_fill_reference(ref_in, B, T, nhead, hd ** -0.5, dense, valid)
    (ref * w.double()).sum().backward()
    x = qkv.to(DEV).requires_grad_(True)
    out = ops.attention(x, lay, nhead, dense_mask=dense.to(DEV), key_valid=valid.to(DEV), mask_value=-1e6)
    (out * w.to(DEV)).sum().backward()
    assert_close(out.cpu(), ref.detach(), what="ctx (dense masks)")
    assert_close(x.grad.cpu(), ref_in.grad, what="d_qkv (dense masks)")


def test_head_dim_query_and_the_error_for_a_rejected_head_dim():
    from graphtrans_amd import _lib, ops
    from graphtrans_amd._lib import GT_BF16, GT_F32

    L = _lib.lib()
    for code in (GT_F32, GT_BF16):
        for hd in range(8, 129, 8):
            for nhead in (1, 4):
                assert L.gt_attn_head_dim_ok(code, hd * nhead, nhead) == 1, (code, hd, nhead)
        for hd in (4, 12, 136, 256):
            assert L.gt_attn_head_dim_ok(code, hd * 2, 2) == 0, (code, hd)
        assert L.gt_attn_head_dim_ok(code, 100, 3) == 0
        assert L.gt_attn_head_dim_ok(code, 0, 4) == 0 and L.gt_attn_head_dim_ok(code, 64, 0) == 0
    assert L.gt_attn_head_dim_ok(7, 64, 2) == 0   # not a storage type
    lay = make_layout("packed", [5, 9])
    with pytest.raises(RuntimeError, match=r"head_dim 136 unsupported \(multiples of 8 from 8 to 128\)"):
        ops.attention(torch.randn(lay.rows, 3 * 272, device=DEV), lay, 2)
