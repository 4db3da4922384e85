"""One evaluation pass (the reference's `eval`, dataset/code.py:49-78 and dataset/mol.py:36-58) over a synthetic split, two ways:
  device    graphtrans_amd.evaluate: `update` enqueues gt_eval_argmax + gt_eval_seq_f1 (Code2) or two strided copies (Molpcba) behind
            every forward, `result()` synchronises once (gt_eval_rows_mean_f64; torch.sort + gt_eval_ap_sorted)
  host      the reference's loop, written out below: torch.argmax per head + torch.cat + a `.cpu()` per graph + Python sets per graph
            (Code2); `.cpu()` of every batch of logits and one scikit-learn average_precision_score per task (Molpcba; the numpy
            statement of tests/eval_refs.py stands in where scikit-learn does not import, and the line says so); the same loop with
            roc_auc_score (Molhiv; tests/eval_auc_refs.py stands in)
Rows: code2 (bench.py's Code2 model, 5 heads of 5002 logits), molpcba (128 tasks) and molhiv (the Molpcba model with one task, about
3.5 % positives and a few unlabelled graphs, scored by `MolRocAuc`: torch.sort + gt_eval_auc_sorted), `--batches` batches of `--batch`
graphs each, generated once and kept on the device; the label sets are random words of the vocabulary plus out-of-vocabulary words.
Per row, one JSON line (wall times of a whole pass in ms, each the median of `--reps` passes, device drained at the end of each):
  forward_ms        model.eval() forwards alone
  device_pass_ms    evaluate(model, batches, evaluator): forwards + metric
  host_pass_ms      forwards + the host loop
  device_metric_ms  the evaluator alone on logits kept from the forwards (update per batch + result), and
  host_metric_ms    the host loop alone on the same logits
  metric_kernel_ms  HIP-event time of the gt_eval_* launches of one pass (sum), and `metric_share` = that over forward_ms
  equal             the two ways agree: F1 rows bit for bit, AP and ROC-AUC within (n + 8) * 2^-52

    python tools/eval_bench.py [--batches 16] [--batch 256] [--reps 5] [--rows code2,molpcba,molhiv] [--mode mixed]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps):
    out, ts = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return out, round(statistics.median(ts), 3)


def forwards(model, batches):
    model.eval()
    outs = []
    with torch.no_grad():
        for b in batches:
            outs.append(model(b))
    return outs


def code2_labels(G, num_vocab, seed):
    rng = np.random.default_rng(seed)
    vocab = {"w%d" % i: i for i in range(num_vocab - 2)}
    vocab["__UNK__"], vocab["__EOS__"] = num_vocab - 2, num_vocab - 1
    seqs = [[("w%d" % rng.integers(0, num_vocab - 2)) if rng.random() < 0.9 else "oov%d" % rng.integers(0, 50)
             for _ in range(int(rng.integers(1, 8)))] for _ in range(G)]
    return vocab, seqs


def host_code2(outs, seqs, idx2vocab):
    """dataset/code.py:63-78 and the OGB F1 evaluator, on the model outputs `outs`"""
    seq_pred, rows = [], []
    for pred_list in outs:
        mat = torch.cat([torch.argmax(p, dim=1).view(-1, 1) for p in pred_list], dim=1)
        for arr in mat:                                  # decode_arr_to_seq, dataset/utils.py:173-185
            eos = (arr == len(idx2vocab) - 1).nonzero()
            clipped = arr[: torch.min(eos)] if len(eos) > 0 else arr
            seq_pred.append([idx2vocab[int(x)] for x in clipped.cpu()])
    for ref, pred in zip(seqs, seq_pred):
        label, prediction = set(ref), set(pred)
        tp, fp, fn = len(label & prediction), len(prediction - label), len(label - prediction)
        p = tp / (tp + fp) if tp + fp > 0 else 0
        r = tp / (tp + fn) if tp + fn > 0 else 0
        rows.append((p, r, 2 * p * r / (p + r) if p + r > 0 else 0))
    rows = np.array(rows, np.float64)
    return {"precision": float(np.average(rows[:, 0])), "recall": float(np.average(rows[:, 1])), "F1": float(np.average(rows[:, 2]))}, rows


def host_mol(outs, batches, ap_score, key="ap"):
    """dataset/mol.py:50-58 and the OGB ap evaluator (or, with roc_auc_score for `ap_score`, its rocauc evaluator: the same loop)"""
    y_true = torch.cat([b.y.view(o.shape).detach().cpu() for b, o in zip(batches, outs)], 0).numpy()
    y_pred = torch.cat([o.detach().cpu() for o in outs], 0).numpy()
    aps = []
    for i in range(y_true.shape[1]):
        if np.sum(y_true[:, i] == 1) > 0 and np.sum(y_true[:, i] == 0) > 0:
            lab = y_true[:, i] == y_true[:, i]
            aps.append(ap_score(y_true[lab, i], y_pred[lab, i]))
    return {key: sum(aps) / len(aps)}


def molhiv_row(tok, batch_graphs):
    """bench.py's Molpcba model with one task; labels of about 3.5 % positives (ogbg-molhiv's share) and 1 % unlabelled"""
    import bench
    from graphtrans_amd import synth
    from graphtrans_amd.encoders import AtomEncoder, BondEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    args = bench.model_args("molpcba", tok)
    model = GNNTransformer(1, AtomEncoder(args.gnn_emb_dim), lambda d: BondEncoder(d), args).to("cuda:0")

    def gen(seed):
        b = synth.molpcba_like(B=batch_graphs, seed=seed, num_tasks=1)
        g = torch.Generator().manual_seed(1000 + seed)
        y = (torch.rand(batch_graphs, 1, generator=g) < 0.035).float()
        y[torch.rand(batch_graphs, 1, generator=g) < 0.01] = float("nan")
        b.y = y
        return b
    return model, gen


def metric_kernel_ms(_lib, fn):
    _lib.TIMER = timer = _lib.KernelTimer(["gt_eval_argmax", "gt_eval_seq_f1", "gt_eval_rows_mean_f64", "gt_eval_ap_sorted",
                                            "gt_eval_auc_sorted"])
    try:
        fn()
    finally:
        _lib.TIMER = None
    return {k: round(v["total_ms"], 4) for k, v in timer.summary().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", default="code2,molpcba,molhiv")
    ap.add_argument("--mode", default="mixed", choices=["mixed", "bf16", "fp32"])
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "eval_bench needs a GPU"
    import bench
    import eval_auc_refs
    import eval_refs
    from graphtrans_amd import _lib, ops
    from graphtrans_amd.evaluate import Code2F1, MolAP, MolRocAuc, encode_code2_refs, evaluate
    matmul, tok = bench.MODES[opt.mode]
    ops.set_matmul_dtype(matmul)
    try:
        from sklearn.metrics import average_precision_score as ap_score
        ap_name = "scikit-learn"
    except ImportError:
        ap_score = lambda y, s: eval_refs.average_precision(s, y)[0]   # noqa: E731
        ap_name = "numpy statement (scikit-learn does not import)"
    try:
        from sklearn.metrics import roc_auc_score as auc_score
    except ImportError:
        def auc_score(y, s):
            num, den, _ = eval_auc_refs.roc_auc(s, y)
            return num / den
    G = opt.batches * opt.batch
    for row in opt.rows.split(","):
        torch.manual_seed(0)
        if row == "molhiv":
            model, gen = molhiv_row(tok, opt.batch)
        else:
            _, model, gen, _, _ = bench.build(row, tok, "cuda:0", opt.batch)
        batches = [gen(seed).to("cuda:0") for seed in range(opt.batches)]
        if row == "code2":
            vocab, seqs = code2_labels(G, 5002, 0)
            idx2vocab = {i: w for w, i in vocab.items()}
            ev = Code2F1(*encode_code2_refs(seqs, vocab), num_vocab=5002, max_seq_len=5, num_graphs=G)
            host = lambda outs: host_code2(outs, seqs, idx2vocab)[0]   # noqa: E731
        elif row == "molhiv":
            ev = MolRocAuc(num_graphs=G, num_tasks=1)
            host = lambda outs: host_mol(outs, batches, auc_score, "rocauc")   # noqa: E731
        else:
            ev = MolAP(num_graphs=G, num_tasks=128)
            host = lambda outs: host_mol(outs, batches, ap_score)     # noqa: E731

        def device_metric(outs):
            ev.reset()
            for o, b in zip(outs, batches):
                ev.update(o, b)
            return ev.result()

        forwards(model, batches)   # warm every shape
        outs, t_fwd = timed(lambda: forwards(model, batches), opt.reps)
        res_dev, t_dev = timed(lambda: evaluate(model, batches, ev), opt.reps)
        res_host, t_host = timed(lambda: host(forwards(model, batches)), opt.reps)
        _, t_dev_metric = timed(lambda: device_metric(outs), opt.reps)
        _, t_host_metric = timed(lambda: host(outs), max(1, opt.reps // 2))
        kern = metric_kernel_ms(_lib, lambda: device_metric(outs))
        if row == "code2":
            equal = bool(np.array_equal(ev.rows[:ev.seen].cpu().numpy(), host_code2(outs, seqs, idx2vocab)[1]))
        else:
            key = "rocauc" if row == "molhiv" else "ap"
            equal = bool(abs(res_dev[key] - res_host[key]) <= (G + 8) * 2.0 ** -52)
        print(json.dumps(dict(row=row, mode=opt.mode, batches=opt.batches, batch=opt.batch, graphs=G, reps=opt.reps,
                              forward_ms=t_fwd, device_pass_ms=t_dev, host_pass_ms=t_host, device_metric_ms=t_dev_metric,
                              host_metric_ms=t_host_metric, metric_kernel_ms=kern,
                              metric_share=round(sum(kern.values()) / t_fwd, 5), host_ap=ap_name if row != "code2" else None,
                              device=res_dev, host=res_host, equal=equal)), flush=True)
        del model, batches, outs, ev
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
