"""The metric statements of tests/eval_refs.py against their sources (torch.argmax, literal `set` code over word lists as the OGB
F1 evaluator runs it, scikit-learn's average_precision_score), and the host half of graphtrans_amd.evaluate: encode_code2_refs.
No GPU."""
import numpy as np
import pytest
import torch

import eval_refs
from graphtrans_amd.evaluate import encode_code2_refs

EPS = 2.0 ** -52


def _vocab(n_words):
    """vocab2idx as get_vocab_mapping builds it: the words, then __UNK__, then __EOS__ (dataset/utils.py:57-58)"""
    v = {"w%d" % i: i for i in range(n_words)}
    v["__UNK__"] = n_words
    v["__EOS__"] = n_words + 1
    return v


def _f1_with_sets(pred_words, label_words):
    """the OGB evaluator's per-graph code, literally"""
    label, prediction = set(label_words), set(pred_words)
    true_positive = len(label.intersection(prediction))
    false_positive = len(prediction - label)
    false_negative = len(label - prediction)
    precision = true_positive / (true_positive + false_positive) if true_positive + false_positive > 0 else 0
    recall = true_positive / (true_positive + false_negative) if true_positive + false_negative > 0 else 0
    f1 = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0
    return precision, recall, f1


def test_argmax_statement_is_torch_argmax():
    g = torch.Generator().manual_seed(0)
    x = torch.randint(-2, 3, (40, 9), generator=g).float()          # ties in every row
    x[3, 4] = float("nan")
    x[4, 2] = x[4, 7] = float("nan")                                 # the first NaN wins
    x[5, :] = float("-inf")                                          # a row of -inf gives 0
    x[6, :] = float("-inf"); x[6, 8] = -1e30
    x[7, 0], x[7, 1] = -0.0, 0.0; x[7, 2:] = -1.0                    # the two zeros are equal: the first wins
    x[8, 0] = float("inf"); x[8, 5] = float("nan")                   # NaN above +inf
    x[9, :] = 1.0
    assert np.array_equal(eval_refs.argmax_rows(x.numpy()), torch.argmax(x, dim=1).numpy())
    one = torch.tensor([[2.5], [float("nan")], [float("-inf")]])
    assert np.array_equal(eval_refs.argmax_rows(one.numpy()), torch.argmax(one, dim=1).numpy())


def test_f1_statement_is_the_set_code_on_word_lists():
    rng = np.random.default_rng(1)
    vocab = _vocab(10)
    idx2vocab = {i: w for w, i in vocab.items()}
    C, H = len(vocab), 5
    labels = []
    for g in range(200):
        k = int(rng.integers(0, 8))
        labels.append([("w%d" % rng.integers(0, 10)) if rng.random() < 0.7 else ("oov%d" % rng.integers(0, 4)) for _ in range(k)])
    labels[0] = []                                   # an empty label
    labels[1] = ["oov1", "oov2", "oov1"]             # only out-of-vocabulary words
    ref_ids, n_ref = encode_code2_refs(labels, vocab)
    pred = rng.integers(0, C, (200, H))
    pred[2] = C - 1                                  # __EOS__ at position 0
    pred[3] = [1, 1, 2, 2, 1]                        # duplicates, no __EOS__
    pred[4] = [C - 2, 3, C - 2, C - 1, 5]            # a predicted __UNK__
    for g in range(200):
        words = [idx2vocab[i] for i in eval_refs.decode(pred[g], C)]
        assert eval_refs.seq_f1(pred[g], C, ref_ids[g], n_ref[g]) == _f1_with_sets(words, labels[g]), g


def test_encode_code2_refs():
    vocab = _vocab(70)
    ref_ids, n_ref = encode_code2_refs([["w3", "w1", "w3", "w1"], ["w2", "zzz", "w2", "yyy"], [], ["zzz"],
                                        ["__UNK__", "w5", "__EOS__"]], vocab)
    assert ref_ids.dtype == np.int32 and n_ref.dtype == np.int32 and ref_ids.shape == (5, 2)
    assert sorted(ref_ids[0].tolist()) == [1, 3] and n_ref[0] == 2                 # duplicates collapse
    assert sorted(ref_ids[1].tolist()) == [-1, 2] and n_ref[1] == 3                # out-of-vocabulary words count, without an id
    assert ref_ids[2].tolist() == [-1, -1] and n_ref[2] == 0                       # an empty label
    assert ref_ids[3].tolist() == [-1, -1] and n_ref[3] == 1
    assert sorted(ref_ids[4].tolist()) == [-1, 5] and n_ref[4] == 3                # the marker words are out-of-vocabulary
    ref_ids, n_ref = encode_code2_refs([[], []], vocab)
    assert ref_ids.shape == (2, 1) and (ref_ids == -1).all()                        # R is at least 1
    ref_ids, n_ref = encode_code2_refs([["w%d" % i for i in range(64)]], vocab)
    assert ref_ids.shape == (1, 64) and sorted(ref_ids[0].tolist()) == list(range(64)) and n_ref[0] == 64
    with pytest.raises(ValueError, match="64"):
        encode_code2_refs([["w%d" % i for i in range(65)]], vocab)


@pytest.mark.parametrize("n", [2, 3, 17, 256, 257, 4099])
def test_ap_statement_is_sklearn(n):
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(n)
    values = np.array([-1.5, -0.25, 0.5, 2.0], np.float32)
    for trial in range(6):
        scores = values[rng.integers(0, 4, n)]                       # tie-heavy: 4 distinct scores
        if trial == 5:
            scores = rng.standard_normal(n).astype(np.float32)      # and once without ties
        y = rng.integers(0, 2, n).astype(np.float32)
        y[0], y[1] = 1.0, 0.0
        labels = y.copy()
        labels[2:][rng.random(n - 2) < 0.3] = np.nan
        keep = ~np.isnan(labels)
        want = metrics.average_precision_score(labels[keep], scores[keep])
        got, valid = eval_refs.average_precision(scores, labels)
        assert valid
        print(f"n {n} trial {trial}: |statement - sklearn| = {abs(got - want):.3e}, bound {(n + 8) * EPS:.3e}")
        assert abs(got - want) <= (n + 8) * EPS
    assert eval_refs.average_precision(values[[0, 1, 2]], [1.0, 1.0, np.nan]) == (0.0, False)
    assert eval_refs.average_precision(values[[0, 1, 2]], [0.0, np.nan, 0.0]) == (0.0, False)
    assert eval_refs.average_precision(values[[0, 1]], [np.nan, np.nan]) == (0.0, False)
