"""CPU-side checks of the ROC-AUC evaluation layer: the built library exports the two new entry points with the declared arity,
the statement of tests/eval_auc_refs.py is scikit-learn's roc_auc_score, and `mol_evaluator` is keyed by the reference's
`dataset.eval_metric`."""
import ctypes
import os
import re

import numpy as np
import pytest

import eval_auc_refs
from conftest import REPO

EPS = 2.0 ** -52


def test_library_exports_the_auc_and_rows_sum_entry_points():
    from graphtrans_amd import _lib, ops
    src = open(os.path.join(REPO, "include", "graphtrans_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for name, sibling in (("gt_eval_auc_sorted", "gt_eval_ap_sorted"), ("gt_eval_rows_sum_f64", "gt_eval_rows_mean_f64")):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported"
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert proto, f"{name} is not declared in include/graphtrans_hip.h"
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len(proto.group(1).split(",")) and (res, args) == _lib.SIGNATURES[sibling]   # the sibling's convention
        assert getattr(L, name).argtypes == args
    assert callable(ops.eval_auc_sorted) and callable(ops.eval_rows_sum)


@pytest.mark.parametrize("positives", [0.05, 0.5])
@pytest.mark.parametrize("n", [2, 3, 5, 17, 255, 256, 257, 1000, 4099])
def test_auc_statement_is_sklearn(n, positives):
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(n)
    worst = 0.0
    for quantised in (True, False):
        scores = rng.standard_normal(n).astype(np.float32)
        if quantised:
            scores = (np.round(scores * 4) / 4).astype(np.float32)   # multiples of 0.25: heavy ties
        y = (rng.random(n) < positives).astype(np.float32)
        y[0], y[1] = 1.0, 0.0
        labels = y.copy()
        labels[2:][rng.random(n - 2) < 0.2] = np.nan
        keep = ~np.isnan(labels)
        want = metrics.roc_auc_score(labels[keep], scores[keep])
        num, den, valid = eval_auc_refs.roc_auc(scores, labels)
        assert valid == 1 and den == 2 * int((labels[keep] == 1).sum()) * int((labels[keep] != 1).sum())
        worst = max(worst, abs(num / den - want))
    print(f"n {n} positives {positives}: max |statement - sklearn| = {worst:.3e}, bound {(n + 8) * EPS:.3e}")
    assert worst <= (n + 8) * EPS


def test_auc_statement_by_hand():
    nan = float("nan")
    assert eval_auc_refs.roc_auc([3.0, 2.0, 1.0], [1.0, 1.0, 0.0]) == (4, 4, 1)            # separated: 1.0
    assert eval_auc_refs.roc_auc([3.0, 2.0, 1.0], [0.0, 1.0, 1.0]) == (0, 4, 1)            # inverted: 0.0
    assert eval_auc_refs.roc_auc([1.0, 1.0, 1.0, 1.0], [0.0, 1.0, nan, 1.0]) == (2, 4, 1)  # one run: 0.5
    assert eval_auc_refs.roc_auc([1.0, 3.0, 2.0], [0.0, 1.0, nan]) == (2, 2, 1)            # any order in, unlabelled skipped
    assert eval_auc_refs.roc_auc([2.0, 1.0], [1.0, nan]) == (0, 0, 0)
    assert eval_auc_refs.roc_auc([2.0, 1.0], [0.0, 0.0]) == (0, 0, 0)
    assert eval_auc_refs.roc_auc([nan, 2.0, 1.0], [nan, 1.0, 0.0]) == (2, 2, 1)            # a NaN score without a label is ignored
    assert eval_auc_refs.roc_auc([2.0, nan, 1.0], [1.0, 0.0, 0.0])[2] == 2
    assert eval_auc_refs.rows_sum([[0.1, 1.0, 0.0], [0.2, 1.0, 0.5], [0.3, 1.0, 0.25]]) == [0.6, 3.0, 0.75]       # 0.1 + 0.2 + 0.3 in floats is 0.6000000000000001


def test_mol_evaluator_is_keyed_by_the_eval_metric():
    from graphtrans_amd import evaluate
    for bad in ("F1", "acc", "auc", None):
        with pytest.raises(ValueError, match="eval_metric"):        # before anything asks for a GPU
            evaluate.mol_evaluator(bad, 4, 1)
    assert issubclass(evaluate.MolAP, evaluate._MolRanked) and issubclass(evaluate.MolRocAuc, evaluate._MolRanked)
    assert (evaluate.MolAP.KEY, evaluate.MolRocAuc.KEY) == ("ap", "rocauc")
