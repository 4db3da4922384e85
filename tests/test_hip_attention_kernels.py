"""The three attention kernels (csrc/attention.hip: k_attn_fwd, k_attn_bwd_dq, k_attn_bwd_dkv) in the configuration training runs them
in -- dropout on, a work list, pooled last layer, dense masks with dropout -- against tests/attention_refs.py: the float64 reference
and keep_mask, the specification of the dropout decision.  Every launch goes through the raw launchers there (outputs prefilled with
NaN, guard bands), never through ops.attention, whose torch.empty outputs can inherit a right answer from the previous call.

Common shapes: lengths 1, 31, 32, 33, 63, 64, 65, 97, 129, 200 (key step 32, query block 64, up to 4 query blocks x 7 key steps),
nhead 3, padded layouts at S = 201 (every sequence left padded, odd kv_off), the four instantiations of attention_refs.INSTANTIATIONS.

  A  decisions: with q = 0 the keep decision of every (sequence, head, query, key) is read off ctx, dV and dQ and must EQUAL keep_mask;
     exact in both storage types (value checks in bf16 cannot see one wrong decision at length 200, tests/test_attention_refs_host.py)
  B  values with dropout p = 0.3 on random data, NaN in the K / V thirds of the padding rows: ctx, d_qkv, lse
  C  work lists (1 item; 13 shuffled; 16 slots with three {-1, 0}; the numpy_layout oracle's; a real SeqLayout's): against the
     reference, and bit for bit against the 3-D grid; a zero-length sequence under the 3-D grid
  D  the pooled entry points against the reference, and what they must leave unwritten
  E  dense masks with and without dropout; the DENSE kernel's own decisions first

Tolerances are the op's own (tests/test_hip_attention.py): 1e-4 for fp32 rows, 2e-2 for bf16 rows, atol = rtol in conftest.assert_close
(relative to max(1, max |reference|)), for ctx, d_qkv and lse alike.

Measured on an MI355X: max abs error against the float64 reference as ctx / d_qkv / lse, with max |d_qkv| of the reference, which
is the scale assert_close takes the tolerance relative to, in brackets.  (The padded layouts' d_qkv is ten times larger than the packed
ones': the up to 200 padding query positions of a sequence hold random Q and d_ctx and all feed dK / dV of its few keys.)
  B, p 0.3, 3-D grid; check C's work-list launches of the same inputs give the same bits, hence the same figures
    fp32-hd32   packed 3.8e-07 / 7.8e-07 [4.3] / 4.2e-07     padded 3.8e-07 / 8.5e-06 [44.7] / 4.2e-07      tol 1e-4
    fp32-hd48   packed 9.3e-07 / 1.1e-06 [4.4] / 4.8e-07     padded 7.9e-07 / 1.5e-05 [42.3] / 4.7e-07      tol 1e-4
    bf16-hd64   packed 6.7e-03 / 9.8e-03 [3.8] / 4.3e-07     padded 1.3e-02 / 1.2e-01 [46.4] / 4.6e-07      tol 2e-2
    bf16-hd128  packed 6.7e-03 / 1.3e-02 [4.8] / 4.1e-07     padded 1.3e-02 / 1.2e-01 [51.6] / 4.4e-07      tol 2e-2
  D, pooled, the worst of packed / padded, p 0 / 0.3 (work_items NULL and the list: the same bits)
    fp32-hd32   2.0e-07 / 4.6e-07 [2.9 - 4.3] / 2.8e-07      fp32-hd48   3.4e-07 / 1.1e-06 [2.6 - 4.4] / 4.5e-07    tol 1e-4
    bf16-hd64   1.3e-02 / 1.9e-02 [2.7 - 4.3] / 3.8e-07      bf16-hd128  1.3e-02 / 1.3e-02 [3.4 - 5.1] / 3.1e-07    tol 2e-2
  E, dense masks, p 0 then p 0.3
    fp32-hd32   5.8e-07 / 8.1e-07 [2.2] / 3.4e-07   then   6.6e-07 / 8.4e-07 [3.0] / 3.4e-07                       tol 1e-4
    fp32-hd48   5.8e-07 / 8.2e-07 [2.6] / 4.1e-07   then   7.4e-07 / 1.6e-06 [2.7] / 4.1e-07                       tol 1e-4
    bf16-hd64   4.6e-03 / 8.3e-03 [2.3] / 2.7e-07   then   7.5e-03 / 8.9e-03 [3.0] / 2.7e-07                       tol 2e-2
The thirds of d_qkv are printed separately but judged together.  In the padded layouts dK carries the noise of dV's scale, not of its
own: B bf16-hd64 padded has dQ 1.4e-02 [3.4], dK 9.2e-02 [4.3], dV 1.2e-01 [46.4] (fp32-hd32: 7.1e-07, 4.7e-06, 8.5e-06).  A sequence of
one key has dK = 0 exactly (ds = P (dP keep / (1 - p) - delta) cancels term by term), and what is left is the rounding of delta =
rowsum(dO * O) with O stored in the storage type, summed over 201 query positions: a property of saving ctx in bf16, not of a kernel.
The bf16 kernels' lse is as close to the float64 reference as the fp32 kernels' (both see the same rounded inputs and accumulate the
scores in fp32); the reference gives no reason to move the bf16 lse tolerance off the op's 2e-2, so it stays.
"""
import pytest
import torch

import attention_refs as R
from conftest import assert_close
from kernel_refs import differences, same

pytestmark = pytest.mark.gpu
DEV = R.DEV
P = 0.3
NHEAD = R.NHEAD
INSTS = list(R.INSTANTIATIONS)
KINDS = ["packed", "padded"]
_CACHE = {}


def common_layout(kind, work=None):
    return R.Layout(kind, R.LENS, S=R.S_PADDED if kind == "padded" else None, work=work)


def run(lay, qkv, d_ctx, dtype, hd, p, use_work=False, pooled=False, dense_mask=None, key_valid=None, mask_value=0.0, dl=None, nhead=NHEAD):
    """forward then backward through the raw launchers; device tensors ctx, lse, d_qkv, delta (NaN where nothing was written)"""
    dl = dl or R.DeviceLayout(lay)
    x, g = qkv.to(DEV).to(dtype), d_ctx.to(DEV).to(dtype)
    dm = None if dense_mask is None else dense_mask.to(DEV).contiguous()
    kv = None if key_valid is None else key_valid.to(DEV).contiguous()
    scale = hd ** -0.5
    ctx, lse = R.launch_fwd(dl, x, nhead, scale, p, R.SEED, use_work=use_work and not pooled, pooled=pooled, dense_mask=dm, key_valid=kv,
                            mask_value=mask_value)
    d_qkv, delta = R.launch_bwd(dl, x, ctx, g, lse, nhead, scale, p, R.SEED, use_work=use_work, pooled=pooled, dense_mask=dm, key_valid=kv,
                                mask_value=mask_value)
    return dict(ctx=ctx, lse=lse, d_qkv=d_qkv, delta=delta)


def check_values(out, ref, rows, dtype, label, lse_rows=None):
    """ctx, d_qkv and lse of the token rows `rows` against the float64 reference at the op's tolerance; prints the measured errors"""
    tol = R.TOL[dtype]
    ref_ctx, ref_dqkv, ref_lse = ref
    lse_rows = rows if lse_rows is None else lse_rows
    ctx, d_qkv, lse = out["ctx"].float().cpu()[rows], out["d_qkv"].float().cpu()[rows], R.lse_natural(out["lse"])[:, lse_rows]
    e = [float((a.double() - b).abs().max()) for a, b in ((ctx, ref_ctx[rows]), (d_qkv, ref_dqkv[rows]), (lse, ref_lse[:, lse_rows]))]
    print(f"\n[{label}] max abs err ctx {e[0]:.2e}, d_qkv {e[1]:.2e} (max |d_qkv| {float(ref_dqkv[rows].abs().max()):.2f}), lse {e[2]:.2e} "
          f"(max |lse| {float(ref_lse[:, lse_rows].abs().max()):.2f}); tol {tol:g}")
    assert_close(ctx, ref_ctx[rows], atol=tol, rtol=tol, what=f"{label}: ctx")
    assert_close(d_qkv, ref_dqkv[rows], atol=tol, rtol=tol, what=f"{label}: d_qkv")
    d = ref_ctx.shape[1]
    for i, part in enumerate(("dQ", "dK", "dV")):   # (reported only: the op's tolerance is relative to the scale of d_qkv as a whole)
        got, want = d_qkv[:, i * d:(i + 1) * d], ref_dqkv[rows][:, i * d:(i + 1) * d]
        print(f"    {part} max abs err {float((got.double() - want).abs().max()):.2e} (max |{part}| {float(want.abs().max()):.2f})")
    assert_close(lse, ref_lse[:, lse_rows], atol=tol, rtol=tol, what=f"{label}: lse")


def assert_same(a, b, what):
    assert same(a, b), f"{what}: {differences(a, b)}"


def value_case(name, inst, make_layout, p=P, nan_padding=False, last_only=False):
    """inputs and float64 reference of one (layout, instantiation), computed once and shared (never modified)"""
    key = (name, inst, p, nan_padding, last_only)
    if key not in _CACHE:
        dtype, hd = R.INSTANTIATIONS[inst]
        lay = make_layout()
        qkv, d_ctx = R.random_inputs(lay, NHEAD, hd, dtype, 11, nan_padding=nan_padding, last_only=last_only)
        keep = R.keep_masks(lay, NHEAD, p, R.SEED) if p > 0 else None
        ref = R.reference(qkv, d_ctx, lay, NHEAD, hd ** -0.5, keep, 1.0 / (1.0 - p))
        _CACHE[key] = (lay, qkv, d_ctx, ref)
    return _CACHE[key]


# ---- A: the decisions of each kernel ---------------------------------------------------------------------------------------------
def recover_decisions(lay, nhead, dtype, hd, p, dense_mask=None, backward=True):
    """the probe launches of attention_refs.probe_inputs: (forward, dV, dQ) read-outs, {(sequence, head): float64 [query][key]};
    backward = False: the forward read-out alone"""
    dl = R.DeviceLayout(lay)
    fwd, dv, dq = (R.new_probe_values(lay, nhead) for _ in range(3))
    chunks = R.probe_chunks(lay, hd)
    assert len(chunks) == -(-lay.max_npos // hd)
    for c0 in chunks:
        qkv, d_ctx = R.probe_inputs(lay, nhead, hd, c0, "v")
        if not backward:
            dm = None if dense_mask is None else dense_mask.to(DEV).contiguous()
            ctx, _ = R.launch_fwd(dl, qkv.to(DEV).to(dtype), nhead, hd ** -0.5, p, R.SEED, dense_mask=dm)
            R.read_fwd(fwd, ctx.float().cpu(), lay, nhead, hd, c0)
            continue
        out = run(lay, qkv, d_ctx, dtype, hd, p, dense_mask=dense_mask, dl=dl, nhead=nhead)
        R.read_fwd(fwd, out["ctx"].float().cpu(), lay, nhead, hd, c0)
        R.read_dv(dv, out["d_qkv"].float().cpu(), lay, nhead, hd, c0)
        qkv, d_ctx = R.probe_inputs(lay, nhead, hd, c0, "k")
        out = run(lay, qkv, d_ctx, dtype, hd, p, dense_mask=dense_mask, dl=dl, nhead=nhead)
        R.read_dq(dq, out["d_qkv"].float().cpu(), lay, nhead, hd, c0)
    return fwd, dv, dq


def check_forward_decisions(fwd, want, lay, dtype, p):
    """check A.1: ctx of the "v" probe is keep / (n (1 - p)): the decisions equal keep_mask, dropped weights are exactly 0, kept ones
    the level to one rounding of the storage type; then the keep rate within 5 binomial standard deviations"""
    rtol = 2.0 ** -7 if dtype == torch.bfloat16 else 1e-5
    got_all = []
    for (b, h), m in sorted(want.items()):
        off, n = int(lay.desc[b, 2]), int(lay.desc[b, 3])
        f, m = fwd[(b, h)][:, off:off + n], m[:, off:off + n]
        assert not f.isnan().any(), f"forward: unwritten ctx in sequence {b} head {h}"
        bad = (f > 0) != m
        assert not bad.any(), f"forward: {int(bad.sum())} decisions of sequence {b} head {h} differ, first (query, key - kv_off) {bad.nonzero()[0].tolist()}"
        level = 1.0 / (n * (1.0 - p))
        assert bool((f[~m] == 0).all()) and float((f[m] - level).abs().max() if m.any() else 0.0) <= rtol * level
        got_all.append((f > 0).reshape(-1))
    got_all = torch.cat(got_all)
    rate, bound = R.rate_bound(R.drop_thr(p), got_all.numel())       # 5 sqrt(rate (1 - rate) / decisions)
    assert abs(float(got_all.double().mean()) - rate) <= bound, (float(got_all.double().mean()), rate, bound)


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("inst", INSTS)
def test_keep_decisions_of_all_three_kernels_equal_keep_mask(inst, kind, p):
    dtype, hd = R.INSTANTIATIONS[inst]
    lay = common_layout(kind)
    want = R.keep_masks(lay, NHEAD, p, R.SEED)
    fwd, dv, dq = recover_decisions(lay, NHEAD, dtype, hd, p)
    check_forward_decisions(fwd, want, lay, dtype, p)
    scale = hd ** -0.5
    for (b, h), m in sorted(want.items()):
        off, n = int(lay.desc[b, 2]), int(lay.desc[b, 3])
        m = m[:, off:off + n]
        v, q = dv[(b, h)][:, off:off + n], dq[(b, h)][:, off:off + n]
        assert not v.isnan().any() and not q.isnan().any(), f"unwritten d_qkv in sequence {b} head {h}"
        bad = (v > 0) != m
        assert not bad.any(), f"dK/dV: {int(bad.sum())} decisions of sequence {b} head {h} differ, first (query, key - kv_off) {bad.nonzero()[0].tolist()}"
        assert bool((v[~m] == 0).all())
        skip = R.undecided_queries(want[(b, h)], off, n)        # all kept or all dropped: the row is 0 up to the rounding of delta
        level = scale / (n * (1.0 - p))
        assert float(q[skip].abs().max() if skip.any() else 0.0) <= level * 2.0 ** -7
        bad = ((q > 0) != m) | ((q < 0) == m)
        bad[skip] = False
        assert not bad.any(), f"dQ: {int(bad.sum())} decisions of sequence {b} head {h} differ, first (query, key - kv_off) {bad.nonzero()[0].tolist()}"


# ---- B: values with dropout at multi-tile lengths --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("inst", INSTS)
def test_values_with_dropout_at_multi_tile_lengths(inst, kind):
    dtype, hd = R.INSTANTIATIONS[inst]
    lay, qkv, d_ctx, ref = value_case(f"common-{kind}", inst, lambda: common_layout(kind), nan_padding=kind == "padded")
    assert kind == "packed" or bool(qkv.isnan().any())
    out = run(lay, qkv, d_ctx, dtype, hd, P)
    check_values(out, ref, lay.valid_rows(), dtype, f"B {inst} {kind} p {P}")


# ---- C: work lists ---------------------------------------------------------------------------------------------------------------
LENS_13 = {"packed": ((33, 64, 65, 97, 129, 200), None),                                 # 1 + 1 + 2 + 2 + 3 + 4 tiles
           "padded": ((1, 2, 5, 9, 17, 31, 32, 33, 35, 38, 39, 40, 40), 41)}             # 13 sequences of one tile


def _work_layout(name, kind):
    if name == "one":
        return R.Layout(kind, [17], S=18 if kind == "padded" else None, work=[[0, 0]])
    if name in ("13", "16"):
        lens, S = LENS_13[kind]
        lay = R.Layout(kind, lens, S=S)
        assert len(lay.tiles()) == 13
        work = R.shuffled_work(lay, 1, pad_at=(6, 7, 8) if name == "16" else ())
        assert work.shape[0] == int(name)
        return lay.with_work(work)
    assert name == "oracle"
    return common_layout(kind, R.oracle_work(R.LENS, kind))


def check_work_list(name, inst, make_layout, dl_of=None):
    dtype, hd = R.INSTANTIATIONS[inst]
    lay, qkv, d_ctx, ref = value_case(name, inst, make_layout)
    dl = dl_of(lay) if dl_of else None
    listed = run(lay, qkv, d_ctx, dtype, hd, P, use_work=True, dl=dl)
    check_values(listed, ref, lay.position_rows(), dtype, f"C {name} {inst}")
    grid = run(lay, qkv, d_ctx, dtype, hd, P, use_work=False, dl=dl)
    for what in ("ctx", "lse", "delta", "d_qkv"):
        assert_same(listed[what], grid[what], f"{what}: work list vs 3-D grid")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("inst", INSTS)
@pytest.mark.parametrize("name", ["one", "13", "16", "oracle"])
def test_work_list_launch_against_reference_and_3d_grid(name, inst, kind):
    """num_work 1 (work_per_xcd 1, seven XCD slices empty); 13 items (work_per_xcd 2: the w >= num_work guard on slots 13 .. 15);
    16 slots with {-1, 0} at 6, 7, 8; the oracle's list of the common lengths (padded per XCD slice)"""
    check_work_list(f"{name}-{kind}", inst, lambda: _work_layout(name, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("inst", ["fp32-hd32", "bf16-hd64"])
def test_work_list_of_a_real_seq_layout(inst, kind):
    """the desc and work tensors inside GraphStructure.build(...).layout(kind, max_len, True), one graph longer than max_len"""
    from graphtrans_amd.graph import GraphStructure

    sizes, max_len = [5, 1, 40, 157, 23, 64, 100, 63], 130
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    gs = GraphStructure.build(torch.zeros((2, 0), dtype=torch.int64, device=DEV), batch, sizes=sizes)
    sl = gs.layout(kind, max_len, True)
    torch.cuda.synchronize()
    assert sl.work is not None and int(sl.desc_cpu[:, 3].max()) == max_len + 1

    def make():
        return R.Layout.from_desc(sl.desc_cpu, sl.row_stride, sl.rows, work=sl.work.cpu().numpy())

    check_work_list(f"seqlayout-{kind}", inst, make, dl_of=lambda lay: R.DeviceLayout(lay, desc=sl.desc.reshape(-1), work=sl.work.reshape(-1)))


@pytest.mark.parametrize("inst", INSTS)
def test_zero_length_sequence_under_the_3d_grid(inst):
    """npos = 0 in the middle of a batch: all three kernels return before they touch memory for it -- the four token rows its row0 points
    at stay NaN in every output, and its neighbours are right"""
    dtype, hd = R.INSTANTIATIONS[inst]
    desc = [[0, 33, 0, 33], [33, 0, 0, 0], [37, 65, 0, 65]]
    lay, qkv, d_ctx, ref = value_case("zero-length", inst, lambda: R.Layout.from_desc(desc, 1, 102))
    out = run(lay, qkv, d_ctx, dtype, hd, P)
    check_values(out, ref, lay.position_rows(), dtype, f"C zero-length {inst}")
    gap = torch.arange(33, 37)
    assert bool(out["ctx"].cpu()[gap].isnan().all()) and bool(out["d_qkv"].cpu()[gap].isnan().all())
    assert bool(out["lse"].cpu()[:, :, gap].isnan().all()) and bool(out["delta"].cpu()[:, gap].isnan().all())


# ---- D: pooled entry points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, P])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("inst", INSTS)
def test_pooled_entry_points_against_reference(inst, kind, p):
    """gt_attn_fwd_last / gt_attn_bwd_last (work_items NULL and the full list): the last rows' ctx and lse, d_qkv on every row; rows
    outside each sequence's last 64-row tile are NOT written by the forward (still NaN), nor is their dQ (still the caller's zeros)"""
    dtype, hd = R.INSTANTIATIONS[inst]
    d = NHEAD * hd
    lay, qkv, d_ctx, ref = value_case(f"pooled-{kind}", inst, lambda: common_layout(kind, R.oracle_work(R.LENS, kind)), p=p, last_only=True)
    last, tile_rows = lay.last_rows(), lay.last_tile_rows()
    outside = torch.ones(lay.rows, dtype=torch.bool)
    outside[tile_rows] = False
    assert int(outside.sum()) > 0 and sorted((d_ctx.abs().sum(1) > 0).nonzero().reshape(-1).tolist()) == sorted(last.tolist())
    outs = {w: run(lay, qkv, d_ctx, dtype, hd, p, use_work=w, pooled=True) for w in (False, True)}
    for w, out in outs.items():
        label = f"D {inst} {kind} p {p} work {w}"
        tol = R.TOL[dtype]
        ref_ctx, ref_dqkv, ref_lse = ref
        ctx, lse, d_qkv = out["ctx"].float().cpu(), R.lse_natural(out["lse"]), out["d_qkv"].float().cpu()
        e = [float((ctx[last].double() - ref_ctx[last]).abs().max()), float((d_qkv.double() - ref_dqkv).abs().max()),
             float((lse[:, last] - ref_lse[:, last]).abs().max())]
        print(f"\n[{label}] max abs err ctx {e[0]:.2e}, d_qkv {e[1]:.2e} (max |d_qkv| {float(ref_dqkv.abs().max()):.2f}), lse {e[2]:.2e}; tol {tol:g}")
        assert_close(ctx[last], ref_ctx[last], atol=tol, rtol=tol, what=f"{label}: ctx of the last rows")
        assert_close(lse[:, last], ref_lse[:, last], atol=tol, rtol=tol, what=f"{label}: lse of the last rows")
        assert_close(ctx[tile_rows], ref_ctx[tile_rows], atol=tol, rtol=tol, what=f"{label}: ctx of the last tiles")
        assert bool(ctx[outside].isnan().all()) and bool(out["lse"].cpu()[:, :, outside].isnan().all()), f"{label}: the forward wrote outside the last tiles"
        assert bool((out["d_qkv"].cpu()[outside][:, :d] == 0).all()), f"{label}: dQ outside the last tiles is not the caller's zero"
        assert_close(d_qkv[:, d:], ref_dqkv[:, d:], atol=tol, rtol=tol, what=f"{label}: dK, dV of every row")
        assert_close(d_qkv[:, :d], ref_dqkv[:, :d], atol=tol, rtol=tol, what=f"{label}: dQ")
    for what in ("ctx", "lse", "delta", "d_qkv"):
        assert_same(outs[True][what], outs[False][what], f"pooled {what}: work list vs 3-D grid")


# ---- E: dense masks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, P])
@pytest.mark.parametrize("inst", ["fp32-hd32", "fp32-hd48", "bf16-hd64"])
def test_dense_masks_with_and_without_dropout(inst, p):
    """B = 3, T = 70, the masks of test_dense_masks_fp32_head_dim_128 (a fully masked row, a key_valid prefix and suffix) on the DENSE
    instantiations; with dropout their own decisions (all-ones dense mask, check A.1) come first"""
    dtype, hd = R.INSTANTIATIONS[inst]
    B, T = 3, 70
    lay = R.Layout("packed", [T] * B)
    dense, valid = R.dense_masks(B, T)
    keep = None
    if p > 0:
        keep = R.keep_masks(lay, NHEAD, p, R.SEED)
        fwd, _, _ = recover_decisions(lay, NHEAD, dtype, hd, p, dense_mask=torch.ones(B, T, T), backward=False)
        check_forward_decisions(fwd, keep, lay, dtype, p)
    qkv, d_ctx = R.random_inputs(lay, NHEAD, hd, dtype, 12)
    ref = R.reference(qkv, d_ctx, lay, NHEAD, hd ** -0.5, keep, 1.0 / (1.0 - p), dense_mask=dense, key_valid=valid, mask_value=-1e6)
    out = run(lay, qkv, d_ctx, dtype, hd, p, dense_mask=dense, key_valid=valid, mask_value=-1e6)
    filled = ((dense * valid.reshape(B, 1, T)).sum(-1) == 0).reshape(-1)            # fully masked rows: lse = -1e6 + log T
    assert int(filled.sum()) == 1
    rows = torch.arange(lay.rows)
    check_values(out, ref, rows, dtype, f"E {inst} p {p}", lse_rows=rows[~filled])
    tol = R.TOL[dtype]
    assert_close(R.lse_natural(out["lse"])[:, filled], ref[2][:, filled], atol=tol, rtol=tol, what="lse of the fully masked row")
