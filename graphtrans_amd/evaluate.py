"""Evaluation without a host round trip per batch: the reference's `eval` loops (dataset/code.py:49-78, dataset/mol.py:36-58,
dataset/tud.py:33-43) and the OGB evaluators behind them (F1 for ogbg-code2, AP for ogbg-molpcba), on csrc/metrics.hip.

    ev = Code2F1(*encode_code2_refs(split_labels, vocab2idx), num_vocab=len(vocab2idx), max_seq_len=5, num_graphs=len(split))
    result = evaluate(model, store.batches(256, ids=split), ev)      # {"precision": .., "recall": .., "F1": ..}

`update` only enqueues kernels on the current stream (no `.item()`, no `.cpu()`, no boolean indexing, no allocation: every
buffer is made in the constructor for `num_graphs` graphs); `result()` holds the one synchronisation of a pass.

`result()` speaks of the batches this process was given, whether or not torch.distributed is initialised.  `result(group)` (and
`evaluate(..., group=group)`) is collective over a process group: every rank calls it and every rank receives the dict that one
evaluator fed all the ranks' shards in rank order would return.  F1 exchanges float64 column sums and counts, accuracy two
integers; AP and ROC-AUC are rank statistics, so the ranks' score and label columns are gathered into the one table and every
rank sorts it (bit-identical to the single process).  Tensors travel as `ops._dist_reduce` sends them: on the device over
nccl, through the host elsewhere.  The gathered table's width is a host number, so `MolAP` / `MolRocAuc` exchange their counts
before the columns: that is a second read on nccl; through the host every exchange is one.
"""
import numpy as np
import torch

from . import ops

MAX_REF_WORDS = 64   # gt_eval_seq_f1: R <= 64
MAX_HEADS = 16       # gt_eval_argmax / gt_eval_seq_f1: H <= 16


def encode_code2_refs(seqs, vocab2idx):
    """The reference word sets of a split as arrays, once, on the host: (ref_ids int32 [G][R], n_ref int32 [G]).

    seqs[g] is graph g's raw label, a list of words (`batch.y[i]` in dataset/code.py:71).  ref_ids[g] holds the ids of its distinct
    in-vocabulary words, padded with -1; n_ref[g] counts ALL its distinct words, so an out-of-vocabulary word is a word the model
    cannot hit (a false negative), as in the OGB evaluator's string sets.  The marker words `__UNK__` and `__EOS__` inside a label
    count as out-of-vocabulary: a predicted `__UNK__` never matches and `__EOS__` ends the prediction.  R is the largest row
    (at least 1); more than 64 distinct in-vocabulary words in one label is a ValueError."""
    unk, eos = vocab2idx.get("__UNK__"), vocab2idx.get("__EOS__")
    rows, n_ref = [], np.zeros(len(seqs), np.int32)
    for g, seq in enumerate(seqs):
        words = set(seq)
        n_ref[g] = len(words)
        ids = sorted(vocab2idx[w] for w in words if w in vocab2idx and vocab2idx[w] != unk and vocab2idx[w] != eos)
        rows.append(ids)
    R = max([len(r) for r in rows] + [1])
    if R > MAX_REF_WORDS:
        raise ValueError(f"encode_code2_refs: a label holds {R} distinct in-vocabulary words, at most {MAX_REF_WORDS} are supported")
    ref_ids = np.full((len(seqs), R), -1, np.int32)
    for g, ids in enumerate(rows):
        ref_ids[g, :len(ids)] = ids
    return ref_ids, n_ref


def _logits(pred):
    """What a model returns -> (fp32 tensor whose first element is logits[0][0], B, H, C, ld, head_stride).
    A StackedHeads (or any list whose heads are equally spaced views of one buffer), a (B, H, C) or a (B, C) tensor is used
    where it lies; heads that are separate tensors are stacked first (one copy; the fused models never return those)."""
    stacked = getattr(pred, "stacked", None)
    if stacked is None and isinstance(pred, (list, tuple)):
        heads = list(pred)
        if not heads or any(h.dim() != 2 or h.shape != heads[0].shape for h in heads):
            raise TypeError("evaluate: a list of (B, C) heads expected")
        h0 = heads[0]
        if not h0.is_cuda:
            raise RuntimeError("graphtrans_amd.evaluate runs on the GPU only (no CPU fallback)")
        step = (heads[1].data_ptr() - h0.data_ptr()) // 4 if len(heads) > 1 else h0.shape[1]
        spaced = h0.dtype == torch.float32 and h0.stride(1) == 1 and step >= h0.shape[1] and all(
            h.dtype == h0.dtype and h.stride() == h0.stride() and h.data_ptr() - h0.data_ptr() == 4 * step * i
            for i, h in enumerate(heads))
        B, C = h0.shape
        ld = h0.stride(0) if B > 1 else len(heads) * step
        if spaced and ld >= (len(heads) - 1) * step + C:
            return h0, B, len(heads), C, ld, step
        stacked = torch.stack([h.to(torch.float32) for h in heads], 1)
    t = stacked if stacked is not None else pred
    if not isinstance(t, torch.Tensor) or t.dim() not in (2, 3):
        raise TypeError("evaluate: logits as a (B, C) or (B, H, C) tensor, a StackedHeads or a list of (B, C) heads expected")
    if not t.is_cuda:
        raise RuntimeError("graphtrans_amd.evaluate runs on the GPU only (no CPU fallback)")
    if t.dtype != torch.float32 or t.stride(-1) != 1:
        t = t.to(torch.float32).contiguous()
    if t.dim() == 2:
        B, C = t.shape
        return t, B, 1, C, (t.stride(0) if B > 1 else C), C
    B, H, C = t.shape
    hs = t.stride(1) if H > 1 else C
    return t, B, H, C, (t.stride(0) if B > 1 else H * hs), hs


class _Evaluator:
    def __init__(self, num_graphs, device):
        if not torch.cuda.is_available():
            raise RuntimeError("graphtrans_amd.evaluate runs on the GPU only (no CPU fallback)")
        self.num_graphs = int(num_graphs)
        if self.num_graphs < 1:
            raise ValueError("num_graphs must be >= 1")
        self.device = torch.device(device)
        self.seen = 0   # graphs written so far (host count: batch sizes are known on the host)

    def skip(self, num_graphs):
        """`evaluate` passed over a batch of `num_graphs` graphs"""

    def _room(self, B):
        if self.seen + B > self.num_graphs:
            raise ValueError(f"more than num_graphs = {self.num_graphs} graphs in one evaluation pass")


def _gather_counts(n, group, device):
    """every rank's host count as a list in rank order (`ops._dist_reduce`: a device tensor on nccl, a host tensor elsewhere)"""
    import torch.distributed as dist
    where = device if dist.get_backend(group) == "nccl" else "cpu"
    return ops._dist_reduce(torch.tensor([n], dtype=torch.int64, device=where), group, gather=True).view(-1).tolist()


class Code2F1(_Evaluator):
    """ogbg-code2's metric (the OGB "F1" evaluator over decoded word sets): mean precision, recall and F1 over the graphs seen.
    ref_ids / n_ref: `encode_code2_refs` of the split; `graph_ids` of `update` index them (None: the batches walk the split in
    order).  num_vocab = len(vocab2idx): `__UNK__` is id num_vocab - 2, `__EOS__` id num_vocab - 1 (dataset/utils.py:57-58)."""

    def __init__(self, ref_ids, n_ref, num_vocab, max_seq_len, num_graphs, device="cuda"):
        super().__init__(num_graphs, device)
        ref_ids = np.ascontiguousarray(np.asarray(ref_ids, np.int32))
        n_ref = np.ascontiguousarray(np.asarray(n_ref, np.int32)).reshape(-1)
        if ref_ids.ndim != 2 or ref_ids.shape[0] != n_ref.size or ref_ids.shape[0] < 1:
            raise ValueError("Code2F1: ref_ids [G][R] and n_ref [G] expected")
        if ref_ids.shape[1] > MAX_REF_WORDS or not 1 <= int(max_seq_len) <= MAX_HEADS:
            raise ValueError(f"Code2F1: at most {MAX_REF_WORDS} reference words and {MAX_HEADS} positions are supported")
        self.C, self.H = int(num_vocab), int(max_seq_len)
        self.ref_ids = torch.from_numpy(ref_ids).to(self.device)
        self.n_ref = torch.from_numpy(n_ref).to(self.device)
        self.pred = torch.empty(self.num_graphs, self.H, dtype=torch.int32, device=self.device)
        self.rows = torch.empty(self.num_graphs, 3, dtype=torch.float64, device=self.device)
        self.out = torch.empty(3, dtype=torch.float64, device=self.device)
        self.cursor = 0   # position in the reference table of the next batch that comes without graph ids

    def reset(self):
        self.seen = self.cursor = 0

    def skip(self, num_graphs):
        self.cursor += num_graphs   # without graph ids the batches walk the reference table in order: stay in step

    def update(self, pred, batch=None, graph_ids=None):
        t, B, H, C, ld, hs = _logits(pred)
        if H != self.H or C != self.C:
            raise ValueError(f"Code2F1: {self.H} heads of {self.C} logits expected, got {H} of {C}")
        self._room(B)
        if graph_ids is None and self.cursor + B > self.ref_ids.shape[0]:
            raise ValueError("Code2F1: without graph_ids the batches walk the reference table in order, and it has ended")
        p = self.pred[self.seen:self.seen + B]
        ops.eval_argmax(t, B, H, C, ld, hs, p)
        if graph_ids is None:   # graphs cursor .. cursor + B of the table
            ops.eval_seq_f1(p, B, H, C, self.ref_ids[self.cursor:], self.n_ref[self.cursor:], self.rows, self.seen)
        else:
            ops.eval_seq_f1(p, B, H, C, self.ref_ids, self.n_ref, self.rows, self.seen, graph_ids)
        self.seen += B
        self.cursor += B

    def result(self, group=None):
        if group is not None:
            return self._result_ranks(group)
        if self.seen == 0:
            raise RuntimeError("Code2F1.result(): no graph was evaluated")
        p, r, f = ops.eval_rows_mean(self.rows, self.seen, self.out).tolist()   # the one synchronisation
        return {"precision": p, "recall": r, "F1": f}

    def _result_ranks(self, group):
        """the mean over every rank's graphs: the local column sums and the count travel, the ranks' sums are added in rank order
        in float64 and divided once (a mean of the ranks' means would weigh a short shard like a long one)"""
        packed = torch.zeros(4, dtype=torch.float64, device=self.device)   # a rank that saw nothing sends zeros
        if self.seen:
            ops.eval_rows_sum(self.rows, self.seen, packed)
            packed[3:].fill_(float(self.seen))
        every = ops._dist_reduce(packed, group, gather=True).tolist()       # the one synchronisation
        sums, n = [0.0, 0.0, 0.0], 0
        for s0, s1, s2, count in every:
            sums = [sums[0] + s0, sums[1] + s1, sums[2] + s2]
            n += int(count)
        if n == 0:
            raise RuntimeError("Code2F1.result(): no graph was evaluated on any rank")
        return {"precision": sums[0] / n, "recall": sums[1] / n, "F1": sums[2] / n}


class _MolRanked(_Evaluator):
    """The rank statistics of the molecule datasets: the (task, graph) score and label tables, their sort and the gather of the
    labels behind it; a subclass names the kernel over the sorted table and the key of its result."""
    KEY = KERNEL = WHAT = None

    def __init__(self, num_graphs, num_tasks, device="cuda"):
        super().__init__(num_graphs, device)
        self.T = int(num_tasks)
        kw = dict(device=self.device)
        self.scores = torch.empty(self.T, self.num_graphs, dtype=torch.float32, **kw)   # task major: a task's scores are one row
        self.labels = torch.empty(self.T, self.num_graphs, dtype=torch.float32, **kw)
        self.value = torch.empty(self.T, dtype=torch.float64, **kw)
        self.valid = torch.empty(self.T, dtype=torch.uint8, **kw)

    def reset(self):
        self.seen = 0

    def update(self, pred, batch, graph_ids=None):
        name = type(self).__name__
        y = batch.y if hasattr(batch, "y") else batch
        if not (isinstance(pred, torch.Tensor) and pred.is_cuda and y.is_cuda):
            raise RuntimeError("graphtrans_amd.evaluate runs on the GPU only (no CPU fallback)")
        B = pred.shape[0]
        if pred.dim() != 2 or pred.shape[1] != self.T or y.numel() != B * self.T:
            raise ValueError(f"{name}: (B, {self.T}) logits and labels expected")
        self._room(B)
        cols = slice(self.seen, self.seen + B)
        self.scores[:, cols].copy_(pred.t())                 # strided device copies (with the cast, if any) into the column range
        self.labels[:, cols].copy_(y.view(B, self.T).t())
        self.seen += B

    def _table(self, group):
        """(scores, labels, n): this process's [T][seen] tables, or with a group the ranks' tables side by side in rank order --
        the table one evaluator fed every rank's shard in that order holds, so the sort and the kernel give the same bits"""
        n = self.seen
        if group is None:
            return self.scores[:, :n], self.labels[:, :n], n
        counts = _gather_counts(n, group, self.device)
        width = max(counts)
        if width == 0:
            return None, None, 0
        wire = torch.zeros(2, self.T, width, dtype=torch.float32, device=self.device)   # padded to the largest count on the wire
        wire[0, :, :n].copy_(self.scores[:, :n])
        wire[1, :, :n].copy_(self.labels[:, :n])
        every = ops._dist_reduce(wire, group, gather=True)                               # (world, 2, T, width)
        both = torch.cat([every[r, :, :, :c] for r, c in enumerate(counts)], 2)
        return both[0], both[1], sum(counts)

    def result(self, group=None):
        name = type(self).__name__
        scores, labels, n = self._table(group)
        if n == 0:
            raise RuntimeError(f"{name}.result(): no graph was evaluated")
        s, order = torch.sort(scores, dim=1, descending=True, stable=True)
        lab = torch.gather(labels, 1, order)
        type(self).KERNEL(s, lab, n, self.value, self.valid)
        value, valid = torch.cat([self.value, self.valid.to(torch.float64)]).cpu().view(2, self.T).numpy()   # the one synchronisation
        if (valid == 2).any():
            raise RuntimeError(f"{name}: NaN scores on labelled entries of {int((valid == 2).sum())} task(s); scores must be finite")
        if not (valid == 1).any():
            raise RuntimeError(f"No positively labeled data available. Cannot compute {self.WHAT}.")
        return {self.KEY: float(value[valid == 1].sum() / (valid == 1).sum())}


class MolAP(_MolRanked):
    """ogbg-molpcba's metric (the OGB "ap" evaluator): scikit-learn's average_precision_score per task over its labelled graphs,
    averaged over the tasks whose labels hold a positive and a negative.  Scores must be finite."""
    KEY, KERNEL, WHAT = "ap", staticmethod(ops.eval_ap_sorted), "Average Precision"


class MolRocAuc(_MolRanked):
    """ogbg-molhiv's metric (the OGB "rocauc" evaluator): scikit-learn's roc_auc_score per task over its labelled graphs, averaged
    over the tasks whose labels hold a positive and a negative.  Scores must be finite."""
    KEY, KERNEL, WHAT = "rocauc", staticmethod(ops.eval_auc_sorted), "ROC-AUC"


def mol_evaluator(eval_metric, num_graphs, num_tasks, device="cuda"):
    """The evaluator of a molecule dataset by the reference's `dataset.eval_metric`: "ap" (ogbg-molpcba) or "rocauc" (ogbg-molhiv)"""
    kinds = {"ap": MolAP, "rocauc": MolRocAuc}
    if eval_metric not in kinds:
        raise ValueError(f"mol_evaluator: eval_metric {eval_metric!r} is not one of {sorted(kinds)}")
    return kinds[eval_metric](num_graphs, num_tasks, device)


class TudAccuracy(_Evaluator):
    """TU datasets: correct / num_graphs (dataset/tud.py:36-43 divides by len(loader.dataset))."""

    def __init__(self, num_graphs, device="cuda"):
        super().__init__(num_graphs, device)
        self.pred = torch.empty(self.num_graphs, dtype=torch.int32, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)

    def reset(self):
        self.seen = 0
        self.count.zero_()

    def update(self, pred, batch, graph_ids=None):
        y = batch.y if hasattr(batch, "y") else batch
        t, B, H, C, ld, hs = _logits(pred)
        if H != 1 or y.numel() != B:
            raise ValueError("TudAccuracy: (B, C) logits and B labels expected")
        self._room(B)
        p = self.pred[self.seen:self.seen + B]
        ops.eval_argmax(t, B, 1, C, ld, hs, p)
        ops.eval_count_correct(p, y.reshape(-1), B, self.count)
        self.seen += B

    def result(self, group=None):
        if group is None:
            return {"acc": int(self.count.item()) / self.num_graphs}   # the one synchronisation
        both = torch.empty(2, dtype=torch.int64, device=self.device)
        both[:1].copy_(self.count)
        both[1:].fill_(self.num_graphs)
        correct, graphs = ops._dist_reduce(both, group, gather=False).tolist()   # the one synchronisation
        return {"acc": correct / graphs}


def evaluate(model, batches, evaluator, skip_single_node=None, group=None):
    """One evaluation pass, the loop of dataset/*.py: model.eval(), torch.no_grad(), every batch through `evaluator.update`,
    training mode restored on exit.  A batch whose x has one row is skipped as the Code2 and Molpcba loops do
    (dataset/code.py:57, dataset/mol.py:44); the TU loop does not skip (`skip_single_node` overrides the choice by evaluator).
    Batches made by `GraphStore.collate` carry their graph ids, which `Code2F1` uses to find the reference sets.
    With a process group (`batches` being this rank's shard, e.g. `store.batches(256, ids=split[rank::world])`) the call is
    collective and returns on every rank what `evaluator.result(group)` says: the result over all the ranks' shards."""
    if skip_single_node is None:
        skip_single_node = not isinstance(evaluator, TudAccuracy)
    was_training = model.training
    model.eval()
    evaluator.reset()
    try:
        with torch.no_grad():
            for batch in batches:
                if skip_single_node and batch.x.shape[0] == 1:
                    evaluator.skip(1)   # one node is one graph
                    continue
                evaluator.update(model(batch), batch, getattr(batch, "_graph_ids", None))
    finally:
        model.train(was_training)
    return evaluator.result() if group is None else evaluator.result(group)
