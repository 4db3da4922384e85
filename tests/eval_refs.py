"""Plain numpy / Python statements of the three evaluation metrics, written from their definitions; nothing here imports the
library under test.  tests/test_eval_refs_host.py pins them to torch.argmax, to literal `set` code over word lists and to
scikit-learn; the GPU tests compare the kernels with them."""
import math

import numpy as np


def argmax_rows(x):
    """torch.argmax over the last axis of a 2-D array: the first maximum in column order; a NaN counts as the maximum and the
    first NaN wins; a row of -inf gives 0."""
    x = np.asarray(x)
    nan = np.isnan(x)
    first = np.argmax(np.where(nan, -np.inf, x), axis=1)      # np.argmax returns the first of equal maxima
    return np.where(nan.any(1), np.argmax(nan, axis=1), first).astype(np.int64)


def decode(pred_row, C):
    """decode_arr_to_seq: the ids before the first C - 1 (__EOS__)"""
    out = []
    for w in pred_row:
        if int(w) == C - 1:
            break
        out.append(int(w))
    return out


def seq_f1(pred_row, C, ref_ids_row, n_ref):
    """(precision, recall, F1) of one graph in float64: the decoded prediction as a set against the reference set given as its
    in-vocabulary ids (padded with -1) and its size n_ref; a predicted C - 2 (__UNK__) matches no reference word."""
    pred = set(decode(pred_row, C))
    ref = set(int(r) for r in ref_ids_row if int(r) >= 0)
    tp = len([w for w in pred if w != C - 2 and w in ref])
    fp = len(pred) - tp
    fn = int(n_ref) - tp
    precision = tp / (tp + fp) if tp + fp > 0 else 0.0
    recall = tp / (tp + fn) if tp + fn > 0 else 0.0
    f1 = 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    return precision, recall, f1


def rows_mean(rows):
    """column means of [n][3] float64 rows, exactly rounded sums"""
    rows = np.asarray(rows, np.float64)
    return [math.fsum(rows[:, k].tolist()) / rows.shape[0] for k in range(rows.shape[1])]


def average_precision(scores, labels):
    """(AP, valid) of one task: scikit-learn's average_precision_score over the labelled entries (label not NaN; 1 = positive).
    Thresholds at the distinct scores, tied scores one threshold; precision = tp / (tp + fp), recall = tp / P at each;
    AP = sum_i (recall_i - recall_{i-1}) * precision_i in float64.  valid (the OGB rule): a positive and a negative among the
    labelled entries.  AP is 0.0 when the task is not valid.  The entries may come in any order."""
    scores, labels = np.asarray(scores, np.float64), np.asarray(labels, np.float64)
    keep = ~np.isnan(labels)
    s, y = scores[keep], labels[keep] == 1
    if np.isnan(s).any():
        raise ValueError("NaN score")
    P, N = int(y.sum()), int((~y).sum())
    if P == 0 or N == 0:
        return 0.0, False
    order = np.argsort(-s, kind="stable")
    s, y = s[order], y[order]
    ends = np.concatenate([np.nonzero(s[1:] != s[:-1])[0], [s.size - 1]])
    tp, fp = np.cumsum(y)[ends], np.cumsum(~y)[ends]
    ap, prev = 0.0, 0.0
    for t, f in zip(tp.tolist(), fp.tolist()):
        recall = t / P
        ap += (recall - prev) * (t / (t + f))
        prev = recall
    return ap, True
