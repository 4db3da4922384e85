"""The evaluation kernels (csrc/metrics.hip) through the C ABI against the statements of tests/eval_refs.py.

Bit for bit wherever no bound is given: gt_eval_argmax (integers), gt_eval_seq_f1 (the same correctly rounded float64 divisions and
products as the statement), gt_eval_count_correct (integers).  Bounds:
  gt_eval_rows_mean_f64   |out - fsum(rows) / n| <= n * 2^-53: the rows lie in [0, 1], no term passes through more than
                          ceil(n / 256) + 8 float64 additions and one division
  gt_eval_ap_sorted       |ap - statement| <= (n + 8) * 2^-52: up to n terms in [0, 1] of three roundings each, summed in another
                          order than the statement's
Sentinel elements stand behind every output (a store past the end is seen), the logits' padding holds 3e38 (a read outside a head
wins the argmax and is seen), and every kernel runs twice for bit-identical results.
"""
import numpy as np
import pytest
import torch

import eval_refs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNSUPPORTED = -2
GUARD = 64
NAN = float("nan")


def _L():
    from graphtrans_amd import _lib
    return _lib, _lib.lib()


def _stream():
    from graphtrans_amd.graph import _stream as f
    return f()


def _guarded(n, dtype, fill):
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _check_guard(buf, n, fill):
    assert bool((buf[n:] == fill).all()), "a store behind the end of an output"


# ---- argmax -------------------------------------------------------------------------------------------------------------------
KINDS = ["ties", "first", "last", "nan", "neginf"]


def _rows(kind, rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (rows, C), generator=g).float()     # integer-valued: rows full of ties
    if kind == "first":
        x[:, 0] = 7.0
    elif kind == "last":
        x[:, C - 1] = 7.0
    elif kind == "nan":
        for r in range(rows):                                    # one NaN, or two (the first wins), beside a +inf
            c = int(torch.randint(0, C, (1,), generator=g))
            x[r, c] = NAN
            if r % 2:
                x[r, int(torch.randint(0, C, (1,), generator=g))] = NAN
            if C > 2:
                x[r, (c + 1) % C] = float("inf")
    elif kind == "neginf":
        x[:] = float("-inf")
        if rows > 1:
            x[1, C - 1] = -3e38                                   # one finite column among -inf
    return x


def _argmax(x, B, H, C, hs, ld, offset):
    """x [B*H][C] (host) laid out as the kernel reads it, `offset` floats behind a 16-byte boundary; -> pred [B][H] int64 (host)"""
    _lib, L = _L()
    flat = torch.full((offset + B * ld + 8,), 3e38)
    body = flat[offset:offset + B * ld].view(B, ld)
    for h in range(H):
        body[:, h * hs:h * hs + C] = x.view(B, H, C)[:, h]
    dev = flat.to(DEV)
    assert dev.data_ptr() % 16 == 0
    outs = []
    for _ in range(2):
        pbuf, pred = _guarded(B * H, torch.int32, -7)
        _lib.check(L.gt_eval_argmax(dev.data_ptr() + 4 * offset, B, H, C, ld, hs, pred.data_ptr(), _stream()), "gt_eval_argmax")
        torch.cuda.synchronize()
        _check_guard(pbuf, B * H, -7)
        outs.append(pred.cpu())
    assert torch.equal(outs[0], outs[1])
    return outs[0].view(B, H).long()


@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 257, 5002])
def test_argmax(C, H, B):
    # (head_stride, ld, base offset in floats): tight; padded ld; head_stride > C, heads off the 16-byte grid; the base pointer 4
    # bytes behind a 16-byte boundary; every head on the 16-byte grid (head_stride and ld multiples of 4), whatever C is
    hs4 = (C + 3) // 4 * 4
    layouts = [(C, H * C, 0), (C, H * C + 5, 0), (C + 3, H * (C + 3) + 2, 0), (C, H * C, 1), (hs4, H * hs4 + 4, 0)]
    for kind in KINDS:
        x = _rows(kind, B * H, C, seed=1000 * C + 10 * H + B)
        want = torch.from_numpy(eval_refs.argmax_rows(x.numpy())).view(B, H)
        for hs, ld, offset in layouts:
            got = _argmax(x, B, H, C, hs, ld, offset)
            assert torch.equal(got, want), (kind, hs, ld, offset, got.tolist(), want.tolist())


def test_argmax_unsupported_touches_nothing():
    _lib, L = _L()
    x = torch.zeros(17 * 8 + 8, device=DEV)
    pbuf, pred = _guarded(17, torch.int32, -7)
    assert L.gt_eval_argmax(x.data_ptr(), 1, 17, 8, 17 * 8, 8, pred.data_ptr(), _stream()) == UNSUPPORTED   # H > 16
    assert L.gt_eval_argmax(x.data_ptr(), 1, 1, 0, 8, 8, pred.data_ptr(), _stream()) == UNSUPPORTED          # C < 1
    torch.cuda.synchronize()
    assert bool((pbuf == -7).all())


# ---- seq_f1, rows_mean ------------------------------------------------------------------------------------------------------
SEQ_C, SEQ_H = 80, 5      # ids 0..77 are words, 78 = __UNK__, 79 = __EOS__
EOS, UNK = SEQ_C - 1, SEQ_C - 2


def _seq_case(R, G=12, seed=0):
    """-> pred [9][H], graph ids [9], ref_ids [G][R], n_ref [G] (numpy): the edge cases in rows 0..5, random rows after"""
    rng = np.random.default_rng(seed)
    ref_ids = np.full((G, R), -1, np.int32)
    n_ref = np.zeros(G, np.int32)
    for g in range(G):
        k = int(rng.integers(0, R + 1))
        ref_ids[g, :k] = rng.permutation(SEQ_C - 2)[:k]
        n_ref[g] = k + int(rng.integers(0, 3))                   # plus out-of-vocabulary words
    ref_ids[3, :] = -1; n_ref[3] = 0                             # an empty label
    ref_ids[4, :] = -1; n_ref[4] = 3                             # a label of out-of-vocabulary words only
    ref_ids[5, :] = rng.permutation(SEQ_C - 2)[:R]; n_ref[5] = R  # a full row
    gids = np.array([7, 5, 5, 3, 4, 5, 0, 11, 2], np.int64)
    pred = rng.integers(0, SEQ_C - 2, (9, SEQ_H)).astype(np.int32)
    pred[0] = [EOS, 1, 2, 3, 4]                                  # __EOS__ at position 0
    pred[1] = [ref_ids[5, 0], 9, ref_ids[5, R - 1], 11, 12]      # no __EOS__ at all, hits on the first and the last reference id
    pred[2] = [ref_ids[5, 0], ref_ids[5, 0], 8, 8, ref_ids[5, 0]]   # duplicate predictions
    pred[3] = [4, 5, EOS, 6, 7]                                  # n_ref = 0
    pred[4] = [UNK, 6, UNK, EOS, EOS]                            # a predicted __UNK__
    pred[5] = [ref_ids[5, R - 1], UNK, EOS, ref_ids[5, 0], 1]
    return pred, gids, ref_ids, n_ref


def _seq_f1(pred, gids, ref_ids, n_ref, row_off, rows_cap, rows=None):
    _lib, L = _L()
    B, H = pred.shape
    G, R = ref_ids.shape
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    dp, dg, dr, dn = d(pred), d(gids), d(ref_ids), d(n_ref)
    rbuf = None
    if rows is None:
        rbuf, rows = _guarded(3 * rows_cap, torch.float64, -5.0)
    _lib.check(L.gt_eval_seq_f1(dp.data_ptr(), B, H, SEQ_C, dr.data_ptr(), dn.data_ptr(), R, G, None if dg is None else dg.data_ptr(),
                                rows.data_ptr(), row_off, rows_cap, _stream()), "gt_eval_seq_f1")
    torch.cuda.synchronize()
    if rbuf is not None:
        _check_guard(rbuf, 3 * rows_cap, -5.0)
    return rows


@pytest.mark.parametrize("R", [1, 64])
@pytest.mark.parametrize("B", [1, 9])
def test_seq_f1(B, R):
    pred, gids, ref_ids, n_ref = _seq_case(R)
    want = np.array([eval_refs.seq_f1(pred[b], SEQ_C, ref_ids[gids[b]], n_ref[gids[b]]) for b in range(9)])
    assert want[0].tolist() == [0.0, 0.0, 0.0] and (want[1] > 0).all() and want[3].tolist() == [0.0, 0.0, 0.0]
    row_off, cap = 3, 14
    for lo in range(0, 9, B):            # B = 1: nine launches of one graph
        for _ in range(2):
            rows = _seq_f1(pred[lo:lo + B], gids[lo:lo + B], ref_ids, n_ref, row_off, cap).cpu().view(cap, 3).numpy()
            assert np.array_equal(rows[row_off:row_off + B], want[lo:lo + B]), (lo, rows[row_off:row_off + B], want[lo:lo + B])
            assert (rows[:row_off] == -5.0).all() and (rows[row_off + B:] == -5.0).all()       # only its own rows are written
    # graph_ids NULL: graph b of the batch is row b of the table
    n = min(B, 9)
    want0 = np.array([eval_refs.seq_f1(pred[b], SEQ_C, ref_ids[b], n_ref[b]) for b in range(n)])
    rows = _seq_f1(pred[:n], None, ref_ids, n_ref, 0, n).cpu().view(n, 3).numpy()
    assert np.array_equal(rows, want0)


def test_seq_f1_unsupported_touches_nothing():
    _lib, L = _L()
    pred = torch.zeros(17, dtype=torch.int32, device=DEV)
    ref = torch.zeros(65, dtype=torch.int32, device=DEV)
    nref = torch.ones(1, dtype=torch.int32, device=DEV)
    rbuf, rows = _guarded(3, torch.float64, -5.0)
    assert L.gt_eval_seq_f1(pred.data_ptr(), 1, 5, SEQ_C, ref.data_ptr(), nref.data_ptr(), 65, 1, None, rows.data_ptr(), 0, 1, _stream()) == UNSUPPORTED
    assert L.gt_eval_seq_f1(pred.data_ptr(), 1, 17, SEQ_C, ref.data_ptr(), nref.data_ptr(), 64, 1, None, rows.data_ptr(), 0, 1, _stream()) == UNSUPPORTED
    assert L.gt_eval_seq_f1(pred.data_ptr(), 1, 5, SEQ_C, ref.data_ptr(), nref.data_ptr(), 64, 1, None, rows.data_ptr(), 1, 1, _stream()) == -1   # past the rows
    torch.cuda.synchronize()
    assert bool((rbuf == -5.0).all())


@pytest.mark.parametrize("n", [1, 255, 4099])
def test_rows_mean(n):
    """rows written by gt_eval_seq_f1 in one launch, and in launches of 1000 and of 7 (or 613) graphs: the same rows, the same mean, bit
    for bit; within n * 2^-53 of the exactly rounded sum / n"""
    _lib, L = _L()
    _, _, ref_ids, n_ref = _seq_case(64, G=40, seed=3)
    rng = np.random.default_rng(n)
    gids = rng.integers(0, 40, n).astype(np.int64)
    pred = np.where(rng.random((n, SEQ_H)) < 0.15, EOS, ref_ids[gids][np.arange(n)[:, None], rng.integers(0, 6, (n, SEQ_H))]).astype(np.int32)
    pred[pred < 0] = 9
    want_rows = np.array([eval_refs.seq_f1(pred[b], SEQ_C, ref_ids[gids[b]], n_ref[gids[b]]) for b in range(n)])
    want = eval_refs.rows_mean(want_rows)
    means = []
    for step in (n, 1000, 7 if n < 1000 else 613):
        rbuf, rows = _guarded(3 * n, torch.float64, -5.0)
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            _seq_f1(pred[lo:hi], gids[lo:hi], ref_ids, n_ref, lo, n, rows=rows)
        _check_guard(rbuf, 3 * n, -5.0)
        assert np.array_equal(rows.cpu().view(n, 3).numpy(), want_rows)
        for _ in range(2):
            obuf, out = _guarded(3, torch.float64, -5.0)
            _lib.check(L.gt_eval_rows_mean_f64(rows.data_ptr(), n, out.data_ptr(), _stream()), "gt_eval_rows_mean_f64")
            torch.cuda.synchronize()
            _check_guard(obuf, 3, -5.0)
            means.append(out.cpu().tolist())
    assert all(m == means[0] for m in means), means
    err = max(abs(a - b) for a, b in zip(means[0], want))
    print(f"rows_mean n {n}: max |out - fsum / n| = {err:.3e}, bound {n * 2.0 ** -53:.3e}")
    assert err <= n * 2.0 ** -53


def test_count_correct_accumulates_over_launches():
    _lib, L = _L()
    g = torch.Generator().manual_seed(0)
    cbuf, count = _guarded(1, torch.int64, 0)
    cbuf[1:] = -9
    total = 0
    for B in (5, 1, 700):       # three launches, one of a single graph
        y = torch.randint(0, 3, (B,), generator=g)
        pred = torch.where(torch.rand(B, generator=g) < 0.5, y, (y + 1) % 3)
        total += int((pred == y).sum())
        dp, dy = pred.to(torch.int32).to(DEV), y.to(DEV)
        _lib.check(L.gt_eval_count_correct(dp.data_ptr(), dy.data_ptr(), B, count.data_ptr(), _stream()), "gt_eval_count_correct")
    torch.cuda.synchronize()
    assert int(count[0]) == total and bool((cbuf[1:] == -9).all())


# ---- ap_sorted --------------------------------------------------------------------------------------------------------------
CHUNK = 256     # k_ap_sorted walks a task in chunks of 256 entries


def _ap_case(T, n, seed):
    """scores [T][n] sorted descending from 4 distinct values, labels in the same order: NaN = unlabelled at the front (task 0), in
    the middle (task 1), at the end (task 2) and at random everywhere; a tie run across the chunk border in every task"""
    rng = np.random.default_rng(seed)
    values = np.array([-1.5, -0.25, 0.5, 2.0], np.float32)
    scores = -np.sort(-values[rng.integers(0, 4, (T, n))], axis=1)
    if n > CHUNK:
        scores[:, CHUNK - 6:CHUNK + 5] = scores[:, CHUNK - 6:CHUNK - 5]        # entries 250..260 tie: sorted order is kept
    labels = rng.integers(0, 2, (T, n)).astype(np.float32)
    labels[rng.random((T, n)) < 0.3] = np.nan
    k = max(1, n // 5)
    for t in range(T):
        if n > 4:
            where = t % 4
            if where == 0:
                labels[t, :k] = np.nan
            elif where == 1:
                labels[t, n // 2:n // 2 + k] = np.nan
            elif where == 2:
                labels[t, n - k:] = np.nan
    if T >= 8:       # not valid: every label positive, every label negative, every entry unlabelled
        labels[5] = np.where(np.isnan(labels[5]), np.nan, 1.0)
        labels[6] = np.where(np.isnan(labels[6]), np.nan, 0.0)
        labels[7] = np.nan
    return np.ascontiguousarray(scores), labels


def _ap(scores, labels):
    _lib, L = _L()
    T, n = scores.shape
    ds, dl = torch.from_numpy(scores).to(DEV), torch.from_numpy(labels).to(DEV)
    outs = []
    for _ in range(2):
        abuf, ap = _guarded(T, torch.float64, -5.0)
        vbuf, valid = _guarded(T, torch.uint8, 77)
        _lib.check(L.gt_eval_ap_sorted(ds.data_ptr(), dl.data_ptr(), T, n, n, ap.data_ptr(), valid.data_ptr(), _stream()), "gt_eval_ap_sorted")
        torch.cuda.synchronize()
        _check_guard(abuf, T, -5.0)
        _check_guard(vbuf, T, 77)
        outs.append((ap.cpu().numpy(), valid.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    return outs[0]


def _ap_check(scores, labels):
    T, n = scores.shape
    ap, valid = _ap(scores, labels)
    worst = 0.0
    for t in range(T):
        want, ok = eval_refs.average_precision(scores[t], labels[t])
        assert int(valid[t]) == int(ok), (t, valid[t], ok)
        if ok:
            worst = max(worst, abs(ap[t] - want))
        else:
            assert ap[t] == 0.0
    print(f"ap_sorted T {T} n {n}: {int(valid.sum())} valid tasks, max |ap - statement| = {worst:.3e}, bound {(n + 8) * 2.0 ** -52:.3e}")
    assert worst <= (n + 8) * 2.0 ** -52
    return valid


@pytest.mark.parametrize("T", [1, 3, 128])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4099])
def test_ap_sorted(n, T):
    scores, labels = _ap_case(T, n, seed=100 * n + T)
    if n == 2:
        labels[0] = [1.0, 0.0]                     # the smallest valid task
    valid = _ap_check(scores, labels)
    if n >= 255:
        assert valid[0] == 1
        if T >= 8:
            assert valid[5] == 0 and valid[6] == 0 and valid[7] == 0


def test_ap_sorted_invalid_tasks_and_ties_across_the_chunk_border():
    n = 2 * CHUNK + 9
    scores, labels = _ap_case(4, n, seed=5)
    scores[0, CHUNK - 100:2 * CHUNK + 3] = scores[0, CHUNK - 100]          # one run over two chunk borders
    scores[0, 2 * CHUNK + 3:] = np.minimum(scores[0, 2 * CHUNK + 3:], scores[0, CHUNK - 100])
    labels[0, CHUNK - 3:CHUNK + 3] = [1.0, 0.0, 1.0, 1.0, np.nan, 0.0]
    labels[1] = np.where(np.isnan(labels[1]), np.nan, 1.0)                 # every label positive
    labels[2] = np.where(np.isnan(labels[2]), np.nan, 0.0)                 # every label negative
    labels[3] = np.nan                                                     # every entry unlabelled
    valid = _ap_check(scores, labels)
    assert valid.tolist() == [1, 0, 0, 0]


def test_ap_sorted_flags_a_nan_score():
    scores = np.array([[NAN, 2.0, 1.0, 0.5], [NAN, 2.0, 1.0, 0.5]], np.float32)    # torch.sort puts NaN first
    labels = np.array([[1.0, 0.0, 1.0, 0.0], [NAN, 0.0, 1.0, 0.0]], np.float32)
    ap, valid = _ap(scores, labels)
    assert valid.tolist() == [2, 1] and ap[0] == 0.0                               # an unlabelled entry's score is never read as a score
    assert abs(ap[1] - eval_refs.average_precision(scores[1], labels[1])[0]) <= 12 * 2.0 ** -52
