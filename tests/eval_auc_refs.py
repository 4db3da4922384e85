"""Plain Python statements of ROC-AUC over a sorted table and of the column sums, written from their definitions; nothing here
imports the library under test.  tests/test_eval_auc_host.py pins `roc_auc` to scikit-learn; the GPU tests compare the kernels
with it bit for bit (`num / den` on Python ints is the correctly rounded quotient)."""
import math

import numpy as np


def roc_auc(scores, labels):
    """(num, den, valid) of one task.  Scores are taken as fp32 and sorted descending with a stable sort (NaN first, as
    torch.sort puts it); labels follow (NaN = unlabelled, 1 = positive, anything else negative).  With tp_e, fp_e the labelled
    positives / negatives among entries 0..e at the end e of a run of equal scores (runs over all entries, labelled or not) and
    tp_e', fp_e' those at the run end before it (0 before the first):
        num = sum_e (fp_e - fp_e') * (tp_e + tp_e'),   den = 2 P N,   AUC = num / den
    valid: 1 when the labelled entries hold a positive and a negative (the OGB rule), 2 when a labelled entry's score is NaN,
    else 0; num = 0 unless valid == 1.  The entries may come in any order."""
    s = np.asarray(scores, np.float32)
    y = np.asarray(labels, np.float64)
    nan = np.isnan(s)
    order = np.argsort(-np.where(nan, np.float32(0), s), kind="stable")
    order = np.concatenate([order[nan[order]], order[~nan[order]]])             # NaN first, each part in its stable order
    s, y = s[order].tolist(), y[order].tolist()
    lab = [v == v for v in y]
    P = sum(1 for v, ok in zip(y, lab) if ok and v == 1.0)
    N = sum(1 for v, ok in zip(y, lab) if ok and v != 1.0)
    den = 2 * P * N
    if any(ok and v != v for v, ok in zip(s, lab)):
        return 0, den, 2
    if P == 0 or N == 0:
        return 0, den, 0
    n = len(s)
    num = tp = fp = tp_prev = fp_prev = 0
    for i in range(n):
        if lab[i]:
            tp += y[i] == 1.0
            fp += y[i] != 1.0
        if i == n - 1 or s[i + 1] != s[i]:          # a run end; a NaN score is a run of its own
            num += (fp - fp_prev) * (tp + tp_prev)
            tp_prev, fp_prev = tp, fp
    return int(num), den, 1


def rows_sum(rows):
    """column sums of [n][3] float64 rows, exactly rounded"""
    rows = np.asarray(rows, np.float64)
    return [math.fsum(rows[:, k].tolist()) for k in range(rows.shape[1])]
