"""Every kernel of csrc/segment.hip that had no reference of its own, against the plain references of tests/kernel_refs.py.

Everything is bit for bit (`kernel_refs.same`: torch.equal on the bit patterns) except the two random-valued sums, whose bounds are
derived from the kernels' addition chains in the docstrings of test_segment_sum_random_within_the_chain_bound and
test_colsum_random_within_the_chain_bound.  Largest observed error / bound on the MI355X (printed by those tests):
  gt_segment_sum                       0.522 (edges, D = 1024; max |err| 6.0e-06)
  gt_colsum_f32 / gt_colsum_rows_f32   0.249 (fp32 rows, D = 300), 0.036 (bf16 rows, D = 256)
Inputs, guarded launchers and sentinel-padded outputs are kernel_refs'; tests/test_kernel_refs_host.py shows without a GPU that these
inputs tell the references from wrong variants of them (first instead of last nodes, node0 off by one, row_stride and 1 swapped, CLS
one position early, a dropped row).

Coverage of the exported entry points of segment.hip:
  gt_segment_bcast_add                 test_bcast_add, test_bcast_add_identity_map
  gt_segment_sum                       test_segment_sum_integer_exact, test_segment_sum_random_within_the_chain_bound
  gt_segment_sum_ws, gt_segment_sum_workspace_bytes
                                       tests/test_hip_parity.py::test_segment_sum_two_phase (the two-phase kernels above 4096 rows)
  gt_colsum_f32, gt_colsum_rows_f32    test_colsum_integer_exact, test_colsum_random_within_the_chain_bound, test_seq_scatter
  gt_seq_gather, gt_seq_gather_cls32   test_seq_gather
  gt_seq_scatter                       test_seq_scatter
  gt_seq_token_rows                    test_seq_token_rows
  gt_seq_layout_packed                 test_seq_layout_packed
  gt_seq_positions, gt_seq_gather_add  tests/test_hip_pos_encoder_kernels.py
  gt_seq_token_rows_layernorm          tests/test_hip_linear3x.py, tests/test_hip_pos_encoder_kernels.py
"""
import numpy as np
import pytest
import torch

import kernel_refs as kr
from kernel_refs import DEV, SENTINEL, same

pytestmark = pytest.mark.gpu
DT = [torch.float32, torch.bfloat16]
U = 2.0 ** -24      # unit roundoff of fp32


def _graphs(batch):
    gptr, ng = kr.graph_arrays(kr.BATCHES[batch])
    return gptr, ng, torch.tensor(gptr, device=DEV), torch.tensor(ng, device=DEV)


# ---- gt_segment_bcast_add ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("D", kr.BCAST_DIMS)
@pytest.mark.parametrize("batch", list(kr.BATCHES))
def test_bcast_add(batch, D, dtype):
    _, ng, _, d_ng = _graphs(batch)
    x, seg = kr.segment_data(batch, D)           # integers in [-8, 8]: x + seg is exact in bf16
    dx, dseg = x.to(dtype).to(DEV), seg.to(dtype).to(DEV)
    assert same(kr.launch_segment_bcast_add(dx, dseg, d_ng), kr.ref_bcast_add(x, seg, ng).to(dtype))
    assert same(kr.launch_segment_bcast_add(None, dseg, d_ng), kr.ref_bcast_add(None, seg, ng).to(dtype))      # x == NULL


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("D", kr.BCAST_DIMS)
def test_bcast_add_identity_map(D, dtype):
    """N == B with node_graph = 0 .. B-1, as model.hip adds two [B][D] matrices"""
    B = 11
    g = torch.Generator().manual_seed(D)
    x, seg = kr.ints((B, D), g), kr.ints((B, D), g)
    ng = torch.arange(B, dtype=torch.int32)
    got = kr.launch_segment_bcast_add(x.to(dtype).to(DEV), seg.to(dtype).to(DEV), ng.to(DEV))
    assert same(got, (x + seg).to(dtype))


# ---- gt_segment_sum: the one-block-per-graph kernel, called directly so that it runs below gt_segment_sum_ws's 4096-row switch ------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("D", kr.SEGMENT_DIMS)
@pytest.mark.parametrize("batch", list(kr.BATCHES))
def test_segment_sum_integer_exact(batch, D, dtype):
    """integers in [-8, 8]: every partial sum is exact in fp32 in any order, so the result is the int64 sum converted once"""
    gptr, _, d_gptr, _ = _graphs(batch)
    x, add = kr.segment_data(batch, D)
    dx, dadd = x.to(dtype).to(DEV), add.to(dtype).to(DEV)
    assert same(kr.launch_segment_sum(dx, dadd, d_gptr), kr.ref_segment_sum(x, add, gptr).to(dtype))
    assert same(kr.launch_segment_sum(dx, None, d_gptr), kr.ref_segment_sum(x, None, gptr).to(dtype))


@pytest.mark.parametrize("D", kr.SEGMENT_DIMS)
@pytest.mark.parametrize("batch", list(kr.BATCHES))
def test_segment_sum_random_within_the_chain_bound(batch, D):
    """k_segment_sum: wave w of the block adds the rows beg + w, beg + w + 4, ... of its graph of n rows one after another into an
    accumulator that starts at 0: ceil(n / 4) additions at most, the first of them (0 + x) exact.  The four accumulators are then added as
    a tree, (s0 + s1) + (s2 + s3): 2 more additions on every path, and `add` is 1 more.  So no term passes through more than
    L = ceil(n / 4) + 2 + [add] additions, of which at most L - 1 round, and with u = 2^-24
        |got - exact| <= ((1 + u)^(L - 1) - 1) * sum|terms| <= L * u * sum|terms|          (L < 2^12)
    per element.  L is read off the kernel, per graph; nothing is tuned."""
    gptr, _, d_gptr, _ = _graphs(batch)
    x, add = kr.segment_data(batch, D, integer=False)
    n = torch.from_numpy(np.diff(gptr).astype(np.int64))
    for a in (add, None):
        got = kr.launch_segment_sum(x.to(DEV), None if a is None else a.to(DEV), d_gptr).cpu().double()
        L = ((n + 3) // 4 + 2 + (a is not None)).double().reshape(-1, 1)
        bound = L * U * kr.ref_segment_abs_sum(x, a, gptr)
        err = (got - kr.ref_segment_sum(x, a, gptr)).abs()
        ratio = float((err / bound.clamp(min=1e-300)).max())
        print(f"gt_segment_sum {batch} D={D} add={a is not None}: max |err| {float(err.max()):.3e}, max err/bound {ratio:.3f}")
        assert bool((err <= bound).all())


# ---- gt_colsum_f32 / gt_colsum_rows_f32 -----------------------------------------------------------------------------------------
def _colsum_both(x, idx, rows, dtype):
    """(over the first `rows` rows of x[idx], over row_idx = idx into x): the same sum from both entry points"""
    xd = x.to(dtype)
    didx = torch.cat([idx, idx.new_zeros(1)]).to(DEV)       # (never a null pointer, also for rows == 0)
    plain = kr.launch_colsum(xd[idx].contiguous().to(DEV) if rows else xd[:1].to(DEV), None, rows)
    return plain, kr.launch_colsum(xd.to(DEV), didx, rows)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("D", kr.COLSUM_DIMS)
def test_colsum_integer_exact(D, dtype):
    for rows in kr.colsum_rows(D):
        x, idx = kr.colsum_data(D, rows)
        want = kr.ref_colsum(x, idx).float()
        for got in _colsum_both(x, idx, rows, dtype):
            assert same(got, want), (D, rows)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("D", kr.COLSUM_DIMS)
def test_colsum_random_within_the_chain_bound(D, dtype):
    """k_colsum_f32: with CW = 16 / 32 / 64 float4 columns per block there are groups = 256 / CW row groups; a thread adds the rows
    g, g + groups, ... one after another into an accumulator that starts at 0: ceil(rows / groups) additions at most, the first exact.
    Thread group 0 then adds the other groups - 1 partial sums to its own, one after another: groups - 1 more.  So no term passes through
    more than L = ceil(rows / groups) + groups - 1 additions, at most L - 1 of them rounding:
        |got - exact| <= L * 2^-24 * sum|terms|          per element, as for gt_segment_sum.
    bf16 rows are widened exactly before they are added, so the same bound holds against the sum of the bf16 values."""
    gr = kr.colsum_groups(D)
    worst = 0.0
    for rows in kr.colsum_rows(D):
        x, idx = kr.colsum_data(D, rows, integer=False)
        xq = x.to(dtype).float()
        want, scale = kr.ref_colsum(xq, idx), kr.ref_colsum(xq.abs(), idx)
        bound = (-(-rows // gr) + gr - 1) * U * scale
        for got in _colsum_both(x, idx, rows, dtype):
            err = (got.cpu().double() - want).abs()
            worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
            assert bool((err <= bound).all()), (D, rows)
    print(f"gt_colsum D={D} {dtype}: max err/bound {worst:.3f}")


# ---- node rows <-> token rows -----------------------------------------------------------------------------------------------------
SEQ = [pytest.param(k, D, t, id=f"{k}-D{D}-{'f32' if t == torch.float32 else 'bf16'}") for k in kr.KINDS for D in kr.SEQ_DIMS for t in DT]


@pytest.mark.parametrize("kind,D,dtype", SEQ)
def test_seq_gather(kind, D, dtype):
    """tokens equal ref_seq_gather (zero pad rows of the padded kind included); gt_seq_gather_cls32 rounds its fp32 CLS row once to the
    token type.  pad_mask: the padded kind writes all of it.  In the packed kind the kernel leaves the entries at p >= npos_b alone -- they
    keep the sentinel here; ops._gather_raw allocates that buffer with torch.empty, and only the padded path of modules/utils.py asks for
    a mask, where npos_b == max_npos for every sequence."""
    for case in kr.seq_cases(kind):
        lay = kr.DeviceLayout(case)
        d = kr.seq_data(case, D)
        h, cls = d["h"].to(dtype), d["cls"].to(dtype)
        want, want_mask = kr.ref_seq_gather(h, cls, case["gptr"], case["desc"], case["row_stride"], case["rows"], case["with_cls"])
        got, mask = kr.launch_seq_gather(lay, h.to(DEV), cls.to(DEV))
        assert same(got, want), case["name"]
        assert kind == "packed" or (want_mask >= 0).all()
        want_mask = np.where(want_mask < 0, int(SENTINEL), want_mask).astype(np.uint8)
        assert np.array_equal(mask.cpu().numpy(), want_mask), case["name"]
        got32, _ = kr.launch_seq_gather(lay, h.to(DEV), None, cls32=d["cls"].to(DEV))
        assert same(got32, want), case["name"]
        if case["with_cls"] and dtype == torch.bfloat16:
            assert not torch.equal(cls.float(), d["cls"])      # (the rounding was there to be done)


@pytest.mark.parametrize("kind,D,dtype", SEQ)
def test_seq_scatter(kind, D, dtype):
    """h_out and cls_out equal ref_seq_scatter with a base and with base == NULL (without a CLS, cls_out is not written); on
    integer-valued data <gather(h), t> == <h, scatter(t)> + <cls, sum_b cls_out[b]> exactly, and gt_colsum_rows_f32 over the layout's
    last_rows is cls_out.sum(0)."""
    for case in kr.seq_cases(kind):
        lay = kr.DeviceLayout(case)
        d = kr.seq_data(case, D)
        wc = case["with_cls"]
        tok, base = d["tok"].to(dtype), d["base"].to(dtype)
        for b in (base, None):
            want_h, want_cls = kr.ref_seq_scatter(tok, b, case["gptr"], case["desc"], case["row_stride"], wc, case["N"])
            got_h, got_cls = kr.launch_seq_scatter(lay, tok.to(DEV), None if b is None else b.to(DEV))
            assert same(got_h, want_h), case["name"]
            assert same(got_cls, want_cls if wc else torch.full((case["B"], D), SENTINEL, dtype=dtype)), case["name"]
        # the adjoint identity, every term an integer: exact in float64
        hi, ti, ci = d["h_int"].to(dtype), d["tok_int"].to(dtype), d["cls_int"].to(dtype)
        gathered, _ = kr.launch_seq_gather(lay, hi.to(DEV), ci.to(DEV), want_mask=False)
        sh, sc = kr.launch_seq_scatter(lay, ti.to(DEV), None)
        lhs = (gathered.cpu().double() * ti.double()).sum()
        rhs = (hi.double() * sh.cpu().double()).sum() + ((ci.double() * sc.cpu().double().sum(0)).sum() if wc else 0.0)
        assert float(lhs) == float(rhs), case["name"]
        if wc:
            last = torch.tensor(case["last_rows"], device=DEV)
            assert same(kr.launch_colsum(ti.to(DEV), last, case["B"]), sc.cpu().double().sum(0).float()), case["name"]


@pytest.mark.parametrize("kind,D,dtype", SEQ)
def test_seq_token_rows(kind, D, dtype):
    """rows equal ref_token_rows; the CLS rows of `tokens` hold cls32 rounded once and nothing else of it is touched; h written through
    `rows` by hand then reproduces the gather's tokens (the padded kind's pad rows, which this kernel does not own, keep the sentinel)."""
    for case in kr.seq_cases(kind):
        lay = kr.DeviceLayout(case)
        d = kr.seq_data(case, D)
        wc = case["with_cls"]
        h, cls = d["h"].to(dtype), d["cls"].to(dtype)
        want_rows, cls_rows = kr.ref_token_rows(case["gptr"], case["desc"], case["row_stride"], wc, case["N"])
        tokens, rows = kr.launch_seq_token_rows(lay, d["cls"].to(DEV), D, dtype)
        assert np.array_equal(rows.cpu().numpy(), want_rows), case["name"]
        want_tok = torch.full((case["rows"], D), SENTINEL, dtype=dtype)
        if wc:
            want_tok[torch.from_numpy(cls_rows)] = cls
        assert same(tokens, want_tok), case["name"]
        by_hand = tokens.clone()
        keep = rows >= 0
        by_hand[rows[keep].long()] = h.to(DEV)[keep]
        gathered, _ = kr.ref_seq_gather(h, cls, case["gptr"], case["desc"], case["row_stride"], case["rows"], wc)
        owned = torch.zeros(case["rows"], dtype=torch.bool)
        owned[torch.from_numpy(want_rows[want_rows >= 0].astype(np.int64))] = True
        if wc:
            owned[torch.from_numpy(cls_rows)] = True
        assert kind == "padded" or bool(owned.all())
        gathered[~owned] = SENTINEL
        assert same(by_hand, gathered), case["name"]


# ---- gt_seq_layout_packed -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_cls", [1, 0])
@pytest.mark.parametrize("max_len", [1000, 3])
@pytest.mark.parametrize("B", [1, 1023, 1024, 1025, 2500])
def test_seq_layout_packed(B, max_len, with_cls):
    """one block walks the graphs in chunks of 1024 and carries the row and work-item prefix sums across chunks: desc, last_rows and
    meta = {rows, num_work, max kv_len, S} equal numpy_layout(.., "packed", ..); the work list is the (sequence, 64-position tile) pairs
    in sequence order (numpy_layout's own list is the host builder's, dealt to XCD slices: not this kernel's), {-1, -1} from num_work to
    work_cap, and nothing is written past a work_cap smaller than num_work."""
    from test_model_driver_host import numpy_layout
    sizes = np.random.default_rng(B).integers(1, 6, B)
    sizes[B // 2] = 200          # several attention tiles (at max_len 1000) in the middle of a chunk
    (rows, max_npos, _, S, _), desc, last_rows, _ = numpy_layout(sizes, "packed", max_len, with_cls)
    tiles = (desc[:, 1].astype(np.int64) + 63) // 64
    work = np.stack([np.repeat(np.arange(B), tiles), np.concatenate([np.arange(t) for t in tiles])], 1).astype(np.int32)
    num_work = int(tiles.sum())
    gptr = torch.tensor(kr.graph_arrays(sizes)[0], device=DEV)
    room = num_work + 5
    for cap in (room, num_work - 1, 0):
        got_desc, got_last, got_work, meta = kr.launch_seq_layout_packed(gptr, B, max_len, with_cls, cap, room)
        assert np.array_equal(got_desc.cpu().numpy(), desc) and np.array_equal(got_last.cpu().numpy(), last_rows)
        assert meta.cpu().tolist() == [rows, num_work, max_npos, S]
        want = np.full((room, 2), int(SENTINEL), np.int32)
        want[:cap] = -1
        k = min(cap, num_work)
        want[:k] = work[:k]
        assert np.array_equal(got_work.cpu().numpy(), want), cap
