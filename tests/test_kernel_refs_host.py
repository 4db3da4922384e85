"""The references of tests/kernel_refs.py have teeth before a GPU sees them (runs without one).

* On the padded layout `ref_seq_gather` / `ref_seq_scatter` are oracle.reference_math.pad_batch / unpad_batch (mask and a truncating
  max_input_len included), `ref_segment_sum` is reference_math.segment_sum, and the packed layout holds the same kept rows as the
  padded one, row for row.
* The input sets that the token, column-sum and row-move GPU tests take from kernel_refs (seq_cases x SEQ_DIMS, colsum_data, rows_data,
  rows_add_data, scatter_grad) tell the right statement from the deliberately wrong ones: keeps the FIRST nodes, node0 off by one,
  row_stride and 1 swapped, CLS at position kept - 1, one row dropped from a column sum, put without the zero fill, an add that truncates
  or rounds ties upward, a conversion that loses a NaN's sign or payload.  A wrong variant that an input CANNOT tell apart by construction (nothing truncated,
  row_stride == 1, no CLS, no rows) must then equal the right one: `differs == applies`, both ways, and every variant applies somewhere
  in the sets.  Only references are made wrong here, never a kernel.
"""
import numpy as np
import pytest
import torch

import kernel_refs as kr
from oracle import reference_math as rm


def _gather(case, d, flaw=None, key="h"):
    return kr.ref_seq_gather(d[key], d["cls"], case["gptr"], case["desc"], case["row_stride"], case["rows"], case["with_cls"], flaw)


def _scatter(case, d, base, flaw=None):
    return kr.ref_seq_scatter(d["tok"], base, case["gptr"], case["desc"], case["row_stride"], case["with_cls"], case["N"], flaw)


@pytest.mark.parametrize("case", kr.seq_cases("padded"), ids=lambda c: c["name"])
def test_padded_gather_and_scatter_are_pad_batch_and_unpad_batch(case):
    max_len = int(case["name"].split("max")[1].split("-")[0])
    d = kr.seq_data(case, 8)
    batch = torch.from_numpy(case["ng"]).long()
    padded, mask, _, S = rm.pad_batch(d["h"], batch, max_len)
    B, cls = case["B"], case["with_cls"]
    assert S == case["S"] and case["rows"] == (S + cls) * B
    tokens, ref_mask = _gather(case, d)
    tokens = tokens.reshape(S + cls, B, 8)
    assert torch.equal(tokens[:S], padded)
    assert np.array_equal(ref_mask[:, :S], mask.numpy().astype(np.int16))
    if cls:   # modules/transformer_encoder.py:50-55: the CLS row after the last position, never masked
        assert torch.equal(tokens[S], d["cls"].expand(B, 8)) and not ref_mask[:, S].any()
    h_out, cls_out = _scatter(case, d, d["base"])
    tok = d["tok"].reshape(S + cls, B, 8)
    assert torch.equal(h_out, rm.unpad_batch(tok[:S], d["base"], batch, S))
    if cls:
        assert torch.equal(cls_out, tok[S])
    h0, _ = _scatter(case, d, None)   # no base: dropped nodes are 0
    assert torch.equal(h0, rm.unpad_batch(tok[:S], torch.zeros_like(d["base"]), batch, S))


@pytest.mark.parametrize("batch", list(kr.BATCHES))
@pytest.mark.parametrize("D", kr.SEGMENT_DIMS)
def test_segment_sum_is_global_add_pool(batch, D):
    gptr, ng = kr.graph_arrays(kr.BATCHES[batch])
    for integer in (True, False):
        x, add = kr.segment_data(batch, D, integer)
        want = rm.segment_sum(x.double(), torch.from_numpy(ng).long(), len(gptr) - 1)
        assert torch.allclose(kr.ref_segment_sum(x, None, gptr), want, rtol=1e-14, atol=1e-12)
        assert torch.allclose(kr.ref_segment_sum(x, add, gptr), want + add.double(), rtol=1e-14, atol=1e-12)
        assert torch.equal(kr.ref_bcast_add(x, add, ng), x.double() + add.double()[torch.from_numpy(ng).long()])
        assert torch.equal(kr.ref_bcast_add(None, add, ng), add.double()[torch.from_numpy(ng).long()])


@pytest.mark.parametrize("case", kr.seq_cases("packed"), ids=lambda c: c["name"])
def test_packed_layout_holds_the_padded_layouts_kept_rows(case):
    batch, _, max_len, cls = case["name"].split("-")
    pad = kr.seq_case(batch, "padded", int(max_len[3:]), case["with_cls"])
    d = kr.seq_data(case, 8)
    packed, _ = _gather(case, d)
    padded, _ = _gather(pad, d)
    total = 0
    for b in range(case["B"]):
        row0, npos, kv_off, kv_len = (int(v) for v in case["desc"][b])
        assert kv_off == 0 and npos == kv_len and int(pad["desc"][b, 3]) == kv_len
        prow = int(pad["desc"][b, 0]) + (int(pad["desc"][b, 2]) + np.arange(kv_len)) * pad["row_stride"]
        assert torch.equal(packed[row0:row0 + kv_len], padded[torch.from_numpy(prow)])
        total += kv_len
    assert total == case["rows"]   # and nothing else: the packed layout has no pad row


def _applies(case, flaw):
    """whether this input can tell the wrong variant from the right one at all"""
    return {"keep_first": bool((case["sizes"] > case["S"]).any()), "node0_off_by_one": True,
            "stride_swapped": case["row_stride"] != 1, "cls_at_kept_minus_1": bool(case["with_cls"])}[flaw]


@pytest.mark.parametrize("D", kr.SEQ_DIMS)
@pytest.mark.parametrize("kind", kr.KINDS)
def test_token_inputs_tell_the_wrong_variants_apart(kind, D):
    seen = {f: 0 for f in kr.FLAWS}
    for case in kr.seq_cases(kind):
        d = kr.seq_data(case, D)
        tokens, mask = _gather(case, d)
        scat = {name: _scatter(case, d, base) for name, base in (("base", d["base"]), ("nobase", None))}
        rows, cls_rows = kr.ref_token_rows(case["gptr"], case["desc"], case["row_stride"], case["with_cls"], case["N"])
        # the three references agree with each other: h written through `rows` + the CLS rows gives the gather's tokens
        by_rows = torch.zeros_like(tokens)
        keep = torch.from_numpy(rows >= 0)
        by_rows[torch.from_numpy(rows[rows >= 0].astype(np.int64))] = d["h"][keep]
        if case["with_cls"]:
            by_rows[torch.from_numpy(cls_rows)] = d["cls"]
            assert np.array_equal(cls_rows, case["last_rows"])
        assert torch.equal(by_rows, tokens), case["name"]
        # ... and gather / scatter are adjoint on the integer inputs (exact in float64)
        ti, _ = _gather(case, d, key="h_int") if not case["with_cls"] else kr.ref_seq_gather(
            d["h_int"], d["cls_int"], case["gptr"], case["desc"], case["row_stride"], case["rows"], 1)
        hs, cs = kr.ref_seq_scatter(d["tok_int"], None, case["gptr"], case["desc"], case["row_stride"], case["with_cls"], case["N"])
        rhs = (d["h_int"].double() * hs.double()).sum() + ((d["cls_int"].double() * cs.double().sum(0)).sum() if case["with_cls"] else 0.0)
        assert float((ti.double() * d["tok_int"].double()).sum()) == float(rhs), case["name"]
        for flaw in kr.FLAWS:
            ap = _applies(case, flaw)
            seen[flaw] += ap
            wt, _ = _gather(case, d, flaw)
            assert (not torch.equal(wt, tokens)) == ap, (case["name"], flaw, "gather")
            for name, base in (("base", d["base"]), ("nobase", None)):
                wh, wc = _scatter(case, d, base, flaw)
                same = torch.equal(wh, scat[name][0]) and (wc is None or torch.equal(wc, scat[name][1]))
                assert (not same) == ap, (case["name"], flaw, "scatter", name)
            wr, wcr = kr.ref_token_rows(case["gptr"], case["desc"], case["row_stride"], case["with_cls"], case["N"], flaw)
            same = np.array_equal(wr, rows) and (not case["with_cls"] or np.array_equal(wcr, cls_rows))
            assert (not same) == ap, (case["name"], flaw, "token rows")
    assert all(seen[f] > 0 for f in kr.FLAWS if f != "stride_swapped"), seen
    assert (seen["stride_swapped"] > 0) == (kind == "padded")


@pytest.mark.parametrize("D", kr.COLSUM_DIMS)
def test_colsum_inputs_notice_a_dropped_row(D):
    for rows in kr.colsum_rows(D):
        for integer in (True, False):
            x, idx = kr.colsum_data(D, rows, integer)
            assert idx.numel() == rows and (rows < 3 or len(set(idx.tolist())) < rows)          # with repeats
            for ri, xs in ((idx, x), (None, x[:rows])):
                right, wrong = kr.ref_colsum(xs, ri), kr.ref_colsum(xs, ri, drop_last=True)
                assert (not torch.equal(right, wrong)) == (rows > 0), (D, rows, integer)
            assert torch.allclose(kr.ref_colsum(x, idx), x.double()[idx].sum(0), rtol=0, atol=0)


@pytest.mark.parametrize("dim", kr.ROWS_DIMS)
@pytest.mark.parametrize("n", kr.ROWS_N)
def test_rows_inputs_notice_a_missing_zero_fill(n, dim):
    x, idx, full = kr.rows_data(n, dim)
    assert len(set(idx.tolist())) == n
    right = kr.ref_rows_put(x, idx, kr.ROWS_TOTAL)
    wrong = kr.ref_rows_put(x, idx, kr.ROWS_TOTAL, out_before=torch.full_like(full, kr.SENTINEL))
    assert not torch.equal(right, wrong)
    assert torch.equal(right[idx], x) and float(right.abs().sum()) == float(x.abs().sum())
    # take and add read / change exactly the indexed rows
    assert torch.equal(kr.ref_rows_take(full, idx), full[idx])
    added = kr.ref_rows_add(x, idx, full)
    untouched = torch.ones(kr.ROWS_TOTAL, dtype=torch.bool)
    untouched[idx] = False
    assert torch.equal(added[untouched], full[untouched]) and torch.equal(added[idx], full[idx] + x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dim", kr.ROWS_DIMS)
@pytest.mark.parametrize("n", [n for n in kr.ROWS_N if n])
def test_rows_add_inputs_notice_a_wrong_rounding(n, dim, dtype):
    """the one rounding of gt_rows_add is there to be done on these inputs: in bf16 the exact fp32 sum is not representable, and an add
    that truncates on the store, or that rounds ties away from zero, gives other bits; in fp32 the sum itself needs its rounding"""
    x, idx, full = kr.rows_add_data(n, dim, dtype)
    right = kr.ref_rows_add(x, idx, full)
    exact = full[idx].double() + x.double()
    assert not torch.equal(right[idx].double(), exact)                     # a rounding happened ...
    assert torch.equal(right[idx], exact.float().to(dtype)) or dtype == torch.float32
    if dtype == torch.bfloat16:
        assert torch.equal(right[idx], (full[idx].float() + x.float()).to(dtype)) and bool((right[idx].double() != exact).any())
        for flaw in ("truncate", "half_up"):                               # ... and a wrong one shows
            assert not torch.equal(kr.ref_rows_add(x, idx, full, flaw), right), flaw
    ulp = 2.0 ** (-7 if dtype == torch.bfloat16 else -23)
    assert right[idx[0], :2].tolist() == [1.0, 1.0 + ulp] and float(x[0, 0]) == ulp / 2 and float(x[0, 1]) == 3 * ulp / 4
    untouched = torch.ones(kr.ROWS_TOTAL, dtype=torch.bool)
    untouched[idx] = False
    assert torch.equal(right[untouched], full[untouched])


@pytest.mark.parametrize("dim", kr.ROWS_DIMS)
def test_scatter_inputs_notice_a_lost_nan_sign_or_payload(dim):
    """the NaNs of scatter_grad are not the canonical one: torch's own conversion (which NaN it makes is its own affair), a conversion
    that drops the sign, and one that does not quiet all differ from the rule on them"""
    grad = kr.scatter_grad(1, dim)
    assert grad.isnan().tolist()[0][:3] == [True, False, True]
    got = [v & 0xFFFF for v in kr.to_storage(grad, torch.bfloat16).view(torch.int16).tolist()[0][:3]]
    assert got == [0xffc0, 0x7f80, 0x7fe0]
    truncated = [(v >> 16) & 0xFFFF for v in grad.view(torch.int32).tolist()[0][:3]]      # no quieting: 0xff80 is -inf, not a NaN
    assert truncated == [0xff80, 0x7f80, 0x7fa0] and got[0] != 0x7fc0 and got[2] != 0x7fc0


def test_call_checks_names_order_and_kinds(monkeypatch):
    from graphtrans_amd import _lib
    sent = []
    monkeypatch.setattr(_lib, "launch", lambda name, *a: sent.append((name, a)))
    P = kr._Ptr
    good = dict(dtype=0, x=P(4096), idx=P(8192), n=2, dim=4, out=P(12288), stream=P(0))
    kr._call("gt_rows_take", **good)
    assert sent == [("gt_rows_take", (0, 4096, 8192, 2, 4, 12288, 0))] and all(type(v) is int for v in sent[0][1])
    assert kr.prototype("gt_rows_put") == ["dtype", "x", "idx", "n", "total_rows", "dim", "out", "stream"]
    swapped = dict(dtype=0, x=P(4096), idx=P(8192), dim=4, n=2, out=P(12288), stream=P(0))
    for bad in (swapped, dict(good, n=P(2)), dict(good, x=4096), dict(good, dim=4.0), {k: v for k, v in good.items() if k != "idx"},
                dict(good, extra=1)):
        with pytest.raises(AssertionError):
            kr._call("gt_rows_take", **bad)
    with pytest.raises(AssertionError):
        kr._call("gt_dropout", dtype=0, x=P(4096), y=P(8192), n=16, p=1, seed=3, stream=P(0))      # p must be a float
    for name in ("gt_copy2d", "gt_rows_add", "gt_rows_gather", "gt_rows_scatter", "gt_add3", "gt_gather_f32", "gt_repitch", "gt_dropout",
                 "gt_segment_bcast_add", "gt_segment_sum", "gt_colsum_f32", "gt_colsum_rows_f32", "gt_seq_gather", "gt_seq_gather_cls32",
                 "gt_seq_scatter", "gt_seq_token_rows", "gt_seq_layout_packed"):
        assert len(kr.prototype(name)) == len(_lib.SIGNATURES[name][1]), name      # the header and the ctypes table agree
    assert len(sent) == 1


def test_dropout_mask_depends_on_both_seed_words_and_keeps_one_minus_p():
    n = 1 << 16
    for p in (0.25, 0.9):
        a = kr.ref_dropout_mask(n, p, 12345)
        b = kr.ref_dropout_mask(n, p, 12345 + (0x9E3779B9 << 32))     # only the high word differs (it is XORed onto the hash: high bits set)
        c = kr.ref_dropout_mask(n, p, 12346)
        assert not torch.equal(a, b) and not torch.equal(a, c)
        for m in (a, b, c):   # a binomial's 6 sigma
            assert abs(float(m.double().mean()) - (1 - p)) < 6 * np.sqrt(p * (1 - p) / n)
    assert bool(kr.ref_dropout_mask(64, 0.0, 3).all())
    x = torch.arange(1, 65, dtype=torch.float32)
    y = kr.ref_dropout(x, 0.25, 3)
    m = kr.ref_dropout_mask(64, 0.25, 3)
    assert torch.equal(y[m], x[m] * torch.tensor(np.float32(1) / np.float32(0.75))) and not y[~m].any()


def test_small_references():
    src = torch.arange(15, dtype=torch.float32).reshape(3, 5)
    assert torch.equal(kr.ref_repitch(src, 8)[:, :5], src) and not kr.ref_repitch(src, 8)[:, 5:].any()
    assert torch.equal(kr.ref_repitch(src, 2), src[:, :2])
    assert kr.ref_repitch(torch.zeros(3, 0), 4).shape == (3, 4)
    m = torch.tensor([2, -1, 2, 0, -5], dtype=torch.int32)
    assert kr.ref_gather_f32(torch.tensor([10.0, 11.0, 12.0]), m).tolist() == [12.0, 0.0, 12.0, 10.0, 0.0]
    dst = torch.zeros(4, 8)
    out = kr.ref_copy2d(dst, 4, src[:, :4].contiguous(), 0, 4)
    assert torch.equal(out[:3, 4:], src[:, :4]) and not out[:, :4].any() and not out[3].any()
    g = torch.tensor([[1.0, float("nan"), float("inf"), -float("inf")]])
    s = kr.ref_rows_scatter(g, None, 2, torch.bfloat16)
    assert kr.same(s[0, [0, 2, 3]], g[0, [0, 2, 3]].to(torch.bfloat16)) and not s[1].any()
    assert s[0].view(torch.int16).tolist()[1] == 0x7fc0 and bool(s[0, 1].isnan())      # the quiet NaN of gt_common.h, whatever torch makes of it
    neg = kr.to_storage(-g[:, 1:2], torch.bfloat16)
    assert neg.view(torch.int16).tolist() == [[0xffc0 - 0x10000]]
    assert not kr.same(torch.tensor([0.0]), torch.tensor([-0.0])) and kr.same(torch.tensor([float("nan")]), torch.tensor([float("nan")]))


def test_every_exported_entry_of_the_two_files_is_named_in_a_coverage_note():
    """the coverage notes in the docstrings of the two GPU files against the `extern "C"` entries of util.hip and segment.hip, and
    those against _lib.py's signature table"""
    import os
    import re
    from graphtrans_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    notes = ""
    for f in ("test_hip_row_kernels.py", "test_hip_segment_kernels.py"):
        with open(os.path.join(root, "tests", f)) as fh:
            notes += fh.read().split('"""')[1]
    for f in ("util.hip", "segment.hip"):
        with open(os.path.join(root, "graphtrans_amd", "csrc", f)) as fh:
            names = re.findall(r'extern "C" \w+ (gt_\w+)\(', fh.read())
        assert len(names) >= 10
        for name in names:
            assert name in _lib.SIGNATURES, name
            assert re.search(rf"\b{name}\b", notes), f"{name} ({f}) has no coverage note"
