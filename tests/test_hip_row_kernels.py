"""Every kernel of csrc/util.hip against the plain references of tests/kernel_refs.py, bit for bit (`kernel_refs.same`: torch.equal on
the bit patterns).  The kernels are index arithmetic plus one rounding at most, so nothing here has a tolerance.  Inputs, guarded
launchers and sentinel-padded outputs are kernel_refs'; tests/test_kernel_refs_host.py shows without a GPU that these inputs tell the
references from wrong variants of them.

Coverage of the exported entry points of util.hip:
  gt_rows_take, gt_rows_put, gt_rows_add     test_rows_take_put_add, test_grid_cap_rows_take_put_add, test_arguments_rejected_before_any_launch
  gt_rows_gather, gt_rows_scatter            test_rows_gather_and_scatter, test_grid_cap_rows_gather_scatter
  gt_copy2d                                  test_copy2d_column_slabs, test_grid_cap_copy2d
  gt_repitch                                 test_repitch, test_grid_cap_repitch
  gt_gather_f32                              test_gather_f32, test_grid_cap_gather_f32
  gt_add3                                    test_add3, test_grid_cap_add3
  gt_dropout                                 test_dropout_kept_set_and_values, test_grid_cap_dropout (statistics and the autograd wrapper:
                                             tests/test_hip_xent.py)
The grid-cap cases cross grid_for's 8192 blocks of 256 threads (4096 for gt_dropout) by the smallest margin that leaves a partial
last pass, so the grid-stride branch of every loop in the file runs once.
"""
import pytest
import torch

import kernel_refs as kr
from kernel_refs import DEV, GT_BF16, GT_F32, SENTINEL, same

pytestmark = pytest.mark.gpu
DT = [torch.float32, torch.bfloat16]
CAP_ITEMS = 8192 * 256     # items one pass of a capped grid covers (grid_for)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dim", kr.ROWS_DIMS)
@pytest.mark.parametrize("n", kr.ROWS_N)
def test_rows_take_put_add(n, dim, dtype):
    x, idx, full = kr.rows_data(n, dim)
    x, full = x.to(dtype), full.to(dtype)
    dx, didx, dfull = x.to(DEV), idx.to(DEV), full.to(DEV)
    sent = torch.full((max(n, 1) + 2, dim), SENTINEL, dtype=dtype)
    # take: out[i] = full[idx[i]]; rows past n (all of them for n == 0) keep the sentinel
    got = kr.launch_rows_take(dfull, didx, sent)
    assert same(got[:n], kr.ref_rows_take(full, idx)) and same(got[n:], sent[n:])
    # put: all ROWS_TOTAL rows zero-filled, then the n rows
    got = kr.launch_rows_put(dx, didx, torch.full_like(full, SENTINEL))
    assert same(got, kr.ref_rows_put(x, idx, kr.ROWS_TOTAL))
    # add: one fp32 add, one rounding to nearest-even, on values whose sum is not representable in the storage type (the host tests
    # show that an add that truncates, or rounds ties away from zero, gives other bits on these inputs); n == 0 leaves out untouched
    x, idx, full = kr.rows_add_data(n, dim, dtype)
    got = kr.launch_rows_add(x.to(DEV), didx, full)
    want = kr.ref_rows_add(x, idx, full)
    assert same(got, want), kr.differences(got, want)
    assert n or same(got, full)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("with_idx", [True, False])
@pytest.mark.parametrize("dim", kr.ROWS_DIMS)
@pytest.mark.parametrize("n", kr.ROWS_N)
def test_rows_gather_and_scatter(n, dim, with_idx, dtype):
    x, idx, full = kr.rows_data(n, dim)
    g = torch.Generator().manual_seed(n * 1000 + dim)
    full = (full + torch.rand(full.shape, generator=g)).to(dtype)      # (not bf16-representable before the cast: real bf16 bit patterns after)
    idx_d = idx.to(DEV) if with_idx else None
    got = kr.launch_rows_gather(full.to(DEV), idx_d, n)
    assert got.dtype == torch.float32 and same(got, kr.ref_rows_gather(full, idx if with_idx else None, n))
    # scatter: fp32 rows that need rounding; a negative signalling NaN, a NaN with a payload bit that bf16 keeps, and +-inf among them
    grad = kr.scatter_grad(n, dim)
    got = kr.launch_rows_scatter(grad.to(DEV), idx_d, kr.ROWS_TOTAL, dtype).cpu()
    want = kr.ref_rows_scatter(grad, idx if with_idx else None, kr.ROWS_TOTAL, dtype)
    assert same(got, want), kr.differences(got, want)      # (the NaNs bit for bit too: quieted, sign and high payload kept)
    if n:
        r, r1 = (int(idx[0]), int(idx[n - 1])) if with_idx else (0, n - 1)
        assert got[r].isnan().tolist()[:3] == [True, False, True] and float(got[r, 1]) == float("inf") and float(got[r1, dim - 1]) == -float("inf")
        if dtype == torch.bfloat16:
            assert [v & 0xFFFF for v in got[r].view(torch.int16).tolist()[:3]] == [0xffc0, 0x7f80, 0x7fe0]
        else:   # fp32 rows are moved, not converted: the very same NaNs
            assert same(got[r], grad[0])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("width_bytes", [16, 1200])
@pytest.mark.parametrize("rows", [1, 33])
def test_copy2d_column_slabs(rows, width_bytes, dtype):
    """both directions of the JK = "cat" column slab: narrow rows into the second half of rows twice as wide, and that half back"""
    w = width_bytes // (4 if dtype == torch.float32 else 2)
    g = torch.Generator().manual_seed(rows + width_bytes)
    narrow = torch.randn(rows, w, generator=g).to(dtype)
    wide = torch.randn(rows + 1, 2 * w, generator=g).to(dtype)        # (one row more than is copied: it must survive)
    got = kr.launch_copy2d(wide, w, narrow.to(DEV), 0, w)
    assert same(got, kr.ref_copy2d(wide, w, narrow, 0, w)) and same(got[:, :w], wide[:, :w]) and same(got[rows], wide[rows])
    back = torch.full((rows + 1, w), SENTINEL, dtype=dtype)
    got = kr.launch_copy2d(back, 0, wide[:rows].contiguous().to(DEV), w, w)
    assert same(got, kr.ref_copy2d(back, 0, wide[:rows], w, w)) and same(got[:rows], wide[:rows, w:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["4-byte", "2-byte"])
@pytest.mark.parametrize("src_cols,dst_cols", [(5, 8), (8, 5), (0, 4)])
@pytest.mark.parametrize("rows", [1, 19])
def test_repitch(rows, src_cols, dst_cols, dtype):
    g = torch.Generator().manual_seed(rows * 10 + src_cols)
    src = torch.randint(1, 30000, (rows, src_cols), generator=g).to(dtype)       # (no zero: a zero fill is told from a copied element)
    assert same(kr.launch_repitch(src.to(DEV), dst_cols), kr.ref_repitch(src, dst_cols))


def test_gather_f32():
    g = torch.Generator().manual_seed(5)
    src = torch.randn(97, generator=g)
    m = torch.randint(-20, 97, (1000,), generator=g).to(torch.int32)      # negatives, repeats, 1000 = 3 * 256 + 232
    m[0], m[-1] = -1, 96
    assert bool((m < 0).any()) and len(set(m.tolist())) < 1000
    assert same(kr.launch_gather_f32(src.to(DEV), m.to(DEV)), kr.ref_gather_f32(src, m))


@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("n", [4, 1028])
def test_add3(n, with_c):
    g = torch.Generator().manual_seed(n)
    a, b, c = (kr.ints((n,), g, -1000, 1000) for _ in range(3))    # small integers: the sum is exact in any order
    c = c if with_c else None
    assert same(kr.launch_add3(a.to(DEV), b.to(DEV), None if c is None else c.to(DEV)), kr.ref_add3(a, b, c))


DROPOUT_SEEDS = (20240611, 0x9E3779B97F4A7C15)     # the second above 2^32, high bits of the high word set


def _check_dropout(x, p, seed):
    got = kr.launch_dropout(x.to(DEV), p, seed).cpu()
    keep = kr.ref_dropout_mask(x.numel(), p, seed).reshape(x.shape)
    assert torch.equal(got != 0, keep)                # (no input is 0: the kept set is the non-zero set)
    assert same(got, kr.ref_dropout(x, p, seed))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("seed", DROPOUT_SEEDS)
@pytest.mark.parametrize("p", [0.25, 0.9])
def test_dropout_kept_set_and_values(p, seed, dtype):
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(40, 300, generator=g) + 0.5).to(dtype) * (1 - 2 * torch.randint(0, 2, (40, 300), generator=g)).to(dtype)
    assert bool((x != 0).all())
    _check_dropout(x, p, seed)
    if seed > 1 << 32:   # the high word reaches the kernel: the low word alone gives another mask
        assert not torch.equal(kr.ref_dropout_mask(x.numel(), p, seed), kr.ref_dropout_mask(x.numel(), p, seed & 0xFFFFFFFF))


# ---- one case per loop across the grid cap -----------------------------------------------------------------------------------
CAP_ROWS, CAP_DIM = 4100, 2048      # 4100 * 2048 / 4 = 2 099 200 float4 items > 8192 * 256 = 2 097 152


def test_grid_cap_rows_take_put_add():
    assert CAP_ROWS * CAP_DIM // 4 > CAP_ITEMS
    g = torch.Generator().manual_seed(1)
    x = kr.ints((CAP_ROWS, CAP_DIM), g, -64, 64)
    idx = torch.randperm(CAP_ROWS, generator=g)
    dx, didx = x.to(DEV), idx.to(DEV)
    assert same(kr.launch_rows_take(dx, didx, torch.full_like(x, SENTINEL)), kr.ref_rows_take(x, idx))
    assert same(kr.launch_rows_put(dx, didx, torch.full_like(x, SENTINEL)), kr.ref_rows_put(x, idx, CAP_ROWS))
    before = torch.roll(x, 1, 0)
    assert same(kr.launch_rows_add(dx, didx, before), kr.ref_rows_add(x, idx, before))


def test_grid_cap_rows_gather_scatter():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(CAP_ROWS, CAP_DIM, generator=g)
    idx = torch.randperm(CAP_ROWS, generator=g)
    xb = x.to(torch.bfloat16)
    assert same(kr.launch_rows_gather(xb.to(DEV), idx.to(DEV), CAP_ROWS), kr.ref_rows_gather(xb, idx, CAP_ROWS))
    assert same(kr.launch_rows_scatter(x.to(DEV), idx.to(DEV), CAP_ROWS, torch.bfloat16), kr.ref_rows_scatter(x, idx, CAP_ROWS, torch.bfloat16))


def test_grid_cap_copy2d():
    rows, w = 4100, 513 * 4     # 513 16-byte chunks per row: 4100 * 513 = 2 103 300 items
    assert rows * (w // 4) > CAP_ITEMS
    g = torch.Generator().manual_seed(3)
    src = torch.randn(rows, w + 4, generator=g)
    dst = torch.full((rows, w + 8), SENTINEL)
    assert same(kr.launch_copy2d(dst, 8, src.to(DEV), 4, w), kr.ref_copy2d(dst, 8, src, 4, w))


def test_grid_cap_repitch():
    rows, src_cols, dst_cols = 4099, 509, 513     # 4099 * 513 = 2 102 787 items
    assert rows * dst_cols > CAP_ITEMS
    src = torch.randint(1, 30000, (rows, src_cols), generator=torch.Generator().manual_seed(4)).to(torch.int16)
    assert same(kr.launch_repitch(src.to(DEV), dst_cols), kr.ref_repitch(src, dst_cols))


def test_grid_cap_gather_f32():
    n = CAP_ITEMS + 300
    g = torch.Generator().manual_seed(5)
    src = torch.randn(5000, generator=g)
    m = torch.randint(-500, 5000, (n,), generator=g).to(torch.int32)
    assert same(kr.launch_gather_f32(src.to(DEV), m.to(DEV)), kr.ref_gather_f32(src, m))


def test_grid_cap_add3():
    n = 4 * (CAP_ITEMS + 300)
    g = torch.Generator().manual_seed(6)
    a, b, c = (kr.ints((n,), g, -1000, 1000) for _ in range(3))
    assert same(kr.launch_add3(a.to(DEV), b.to(DEV), c.to(DEV)), kr.ref_add3(a, b, c))


def test_grid_cap_dropout():
    n = 4 * (4096 * 256 + 300)      # gt_dropout caps its grid at 4096 blocks
    x = torch.rand(n, generator=torch.Generator().manual_seed(7)) + 0.5
    _check_dropout(x, 0.25, DROPOUT_SEEDS[1])


# ---- argument checks that return before any launch -------------------------------------------------------------------------
def test_arguments_rejected_before_any_launch():
    """only arguments the entry points reject up front: every pointer below is a valid device buffer of 64 elements"""
    from graphtrans_amd import _lib
    st = int(kr._stream())
    x = torch.zeros(64, dtype=torch.float32, device=DEV)
    out = torch.zeros(64, dtype=torch.float32, device=DEV)
    idx = torch.zeros(8, dtype=torch.int64, device=DEV)
    px, po, pi = x.data_ptr(), out.data_ptr(), idx.data_ptr()
    bad = [
        ("dim must be a positive multiple of 4", "gt_rows_take", (GT_F32, px, pi, 2, 6, po, st)),
        ("dim must be a positive multiple of 4", "gt_rows_put", (GT_F32, px, pi, 2, 4, 6, po, st)),
        ("dim must be a positive multiple of 4", "gt_rows_add", (GT_BF16, px, pi, 2, 2, po, st)),
        ("dim must be a positive multiple of 4", "gt_rows_gather", (GT_F32, px, pi, 2, 7, po, st)),
        ("dim must be a positive multiple of 4", "gt_rows_scatter", (GT_F32, px, pi, 2, 4, 0, po, st)),
        ("bad dtype", "gt_rows_take", (2, px, pi, 2, 4, po, st)),
        ("bad dtype", "gt_rows_put", (-1, px, pi, 2, 4, 4, po, st)),
        ("bad dtype", "gt_rows_add", (7, px, pi, 2, 4, po, st)),
        ("bad dtype", "gt_rows_gather", (2, px, pi, 2, 4, po, st)),
        ("bad dtype", "gt_rows_scatter", (2, px, pi, 2, 4, 4, po, st)),
        ("bad dtype", "gt_dropout", (2, px, po, 16, 0.5, 1, st)),
        ("multiples of 16 bytes", "gt_copy2d", (po, 24, px, 16, 16, 2, st)),
        ("multiples of 16 bytes", "gt_copy2d", (po, 16, px, 40, 16, 2, st)),
        ("multiples of 16 bytes", "gt_copy2d", (po, 32, px, 32, 8, 2, st)),
        ("n must be a multiple of 4 below 2^32", "gt_dropout", (GT_F32, px, po, 18, 0.5, 1, st)),
        ("p must be in [0,1)", "gt_dropout", (GT_F32, px, po, 16, 1.0, 1, st)),
        ("elt_bytes must be 2 or 4", "gt_repitch", (po, 4, px, 4, 2, 8, st)),
        ("element count must be a multiple of 4", "gt_add3", (px, px, None, 6, po, st)),
    ]
    for msg, name, args in bad:
        with pytest.raises(RuntimeError) as e:
            _lib.launch(name, *args)
        assert name in str(e.value) and msg in str(e.value), (name, str(e.value))
    torch.cuda.synchronize()
    assert not x.any() and not out.any()      # and nothing ran
