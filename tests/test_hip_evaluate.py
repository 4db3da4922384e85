"""graphtrans_amd.evaluate end to end on the smallest models the suite builds: `evaluate(model, batches, evaluator)` against the
statements of tests/eval_refs.py applied to the same model's logits copied to the host.

Each pass walks three batches, one of them of a single graph.  Per graph everything is exact: the argmax, the (precision, recall,
F1) rows bit for bit, the number of correct predictions.  The Code2 means are the kernel's fixed-order float64 sums, compared with
the exactly rounded sum / n within n * 2^-53 (the bound of gt_eval_rows_mean_f64, tests/test_hip_eval_kernels.py); AP within
(n + 8) * 2^-52 per task, hence for the mean over tasks.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import eval_refs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NUM_VOCAB, SEQ = 30, 3          # ids 0..27 are words, 28 = __UNK__, 29 = __EOS__


def _gnn_args(**kw):
    a = dict(gnn_virtual_node=True, gnn_num_layer=2, gnn_emb_dim=64, gnn_JK="last", gnn_dropout=0.0, gnn_residual=False, gnn_type="gcn",
             graph_pooling="mean", max_seq_len=SEQ, model_type="gnn")
    a.update(kw)
    return SimpleNamespace(**a)


def _vocab():
    v = {"w%d" % i: i for i in range(NUM_VOCAB - 2)}
    v["__UNK__"], v["__EOS__"] = NUM_VOCAB - 2, NUM_VOCAB - 1
    return v


def _labels(G, seed):
    """raw labels: word lists with duplicates and out-of-vocabulary words, one of them empty"""
    rng = np.random.default_rng(seed)
    out = [[("w%d" % rng.integers(0, NUM_VOCAB - 2)) if rng.random() < 0.8 else "oov%d" % rng.integers(0, 3)
            for _ in range(int(rng.integers(1, 6)))] for _ in range(G)]
    out[1] = []
    return out


def _bias_heads(model, seed):
    """spread the head biases so that every vocabulary id, __EOS__ and __UNK__ included, is some graph's argmax now and then"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g).to(p.device) * 0.3)


def _host_logits(model, batches):
    """the same model's logits of every batch, on the host: a list of (B, H, C) or (B, C) float32 arrays"""
    out = []
    was = model.training
    model.eval()
    with torch.no_grad():
        for b in batches:
            o = model(b)
            o = getattr(o, "stacked", o)
            out.append((torch.stack(list(o), 1) if isinstance(o, (list, tuple)) else o).float().cpu().numpy())
    model.train(was)
    return out


def _code2_statement(logits, graph_ids, ref_ids, n_ref):
    rows = []
    for lg, gids in zip(logits, graph_ids):
        B, H, C = lg.shape
        pred = eval_refs.argmax_rows(lg.reshape(B * H, C)).reshape(B, H)
        rows += [eval_refs.seq_f1(pred[b], C, ref_ids[g], n_ref[g]) for b, g in enumerate(gids)]
    return np.array(rows)


def _check_code2(result, ev, want_rows):
    n = len(want_rows)
    assert ev.seen == n
    assert np.array_equal(ev.rows[:n].cpu().numpy(), want_rows)          # per graph: bit for bit
    want = eval_refs.rows_mean(want_rows)
    for k, name in enumerate(("precision", "recall", "F1")):
        print(f"{name}: evaluate {result[name]!r} statement {want[k]!r}")
        assert abs(result[name] - want[k]) <= n * 2.0 ** -53
    assert set(result) == {"precision", "recall", "F1"}


def test_code2_gnn_batches_in_table_order():
    """2-layer GCN `gnn`, three collated batches (5, 1 and 4 graphs) without graph ids: the batches walk the reference table"""
    from graphtrans_amd import synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.evaluate import Code2F1, encode_code2_refs, evaluate
    from graphtrans_amd.models.gnn import GNN
    torch.manual_seed(0)
    model = GNN(NUM_VOCAB, ASTNodeEncoder(64, 98, 300, 20), lambda d: torch.nn.Linear(2, d), _gnn_args()).to(DEV)
    _bias_heads(model, 1)
    batches = [synth.code2_like(B=B, seed=s, num_nodeattributes=300, mean_nodes=20.0, max_nodes=40).to(DEV) for B, s in ((5, 1), (1, 2), (4, 3))]
    ref_ids, n_ref = encode_code2_refs(_labels(10, 0), _vocab())
    ev = Code2F1(ref_ids, n_ref, NUM_VOCAB, SEQ, num_graphs=10)
    model.train()
    result = evaluate(model, batches, ev)
    assert model.training                                                  # training mode is restored
    want_rows = _code2_statement(_host_logits(model, batches), [range(0, 5), range(5, 6), range(6, 10)], ref_ids, n_ref)
    _check_code2(result, ev, want_rows)
    model.eval()
    assert evaluate(model, batches, ev) == result and not model.training   # a second pass: the same bits; eval mode stays


def test_code2_gnn_transformer_from_a_graph_store():
    """1-encoder-layer `gnn-transformer`, batches of 4, 4 and 1 graphs collated from a GraphStore in shuffled order: the batches
    carry their graph ids, which select the reference sets on the device"""
    from graphtrans_amd import synth
    from graphtrans_amd.data import GraphStore
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.evaluate import Code2F1, encode_code2_refs, evaluate
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    from oracle import reference_math as rm
    torch.manual_seed(0)
    args = rm.default_args(gnn_virtual_node=True, gnn_num_layer=2, gnn_emb_dim=64, gnn_JK="cat", gnn_type="gcn", d_model=64, nhead=2,
                           dim_feedforward=128, transformer_dropout=0.0, num_encoder_layers=1, transformer_norm_input=True,
                           graph_pooling="cls", max_seq_len=SEQ)
    model = GNNTransformer(NUM_VOCAB, ASTNodeEncoder(64, 20, 50, 20), lambda d: torch.nn.Linear(2, d), args).to(DEV)
    _bias_heads(model, 2)
    store = GraphStore(synth.code2_raw(B=12, seed=4, mean_nodes=20.0, max_nodes=40, num_nodetypes=20, num_nodeattributes=50,
                                       num_vocab=NUM_VOCAB, max_seq_len=SEQ), device=DEV)
    ids = np.random.default_rng(0).permutation(12)[:9]                     # a split: 9 of the 12 graphs, shuffled
    ref_ids, n_ref = encode_code2_refs(_labels(12, 5), _vocab())
    ev = Code2F1(ref_ids, n_ref, NUM_VOCAB, SEQ, num_graphs=9)
    model.train()
    result = evaluate(model, store.batches(4, ids=ids), ev)
    assert model.training
    batches = list(store.batches(4, ids=ids))
    assert [b.num_graphs for b in batches] == [4, 4, 1]
    want_rows = _code2_statement(_host_logits(model, batches), [ids[0:4], ids[4:8], ids[8:9]], ref_ids, n_ref)
    _check_code2(result, ev, want_rows)


def _mol_setup():
    from graphtrans_amd import synth
    from graphtrans_amd.encoders import AtomEncoder, BondEncoder
    from graphtrans_amd.models.gnn import GNN
    torch.manual_seed(0)
    T = 16
    model = GNN(T, AtomEncoder(64), lambda d: BondEncoder(d), _gnn_args(max_seq_len=None)).to(DEV)
    batches = []
    g = torch.Generator().manual_seed(7)
    for B, s in ((6, 1), (1, 2), (5, 3)):
        b = synth.molpcba_like(B=B, seed=s, num_tasks=T)
        y = (torch.rand(B, T, generator=g) > 0.5).float()
        y[torch.rand(B, T, generator=g) < 0.2] = float("nan")              # unlabelled entries
        b.y = y
        batches.append(b.to(DEV))
    return model, batches, T


def test_molpcba_ap():
    from graphtrans_amd.evaluate import MolAP, evaluate
    model, batches, T = _mol_setup()
    ev = MolAP(num_graphs=12, num_tasks=T)
    model.train()
    result = evaluate(model, batches, ev)
    assert model.training and set(result) == {"ap"}
    scores = np.concatenate(_host_logits(model, batches), 0)
    labels = np.concatenate([b.y.cpu().numpy() for b in batches], 0)
    aps = [eval_refs.average_precision(scores[:, t], labels[:, t]) for t in range(T)]
    valid = [a for a, ok in aps if ok]
    assert len(valid) >= 4
    want = sum(valid) / len(valid)
    print(f"ap: evaluate {result['ap']!r} statement {want!r} over {len(valid)} valid tasks")
    assert abs(result["ap"] - want) <= (12 + 8) * 2.0 ** -52
    assert evaluate(model, batches, ev) == result


def test_molpcba_ap_without_a_valid_task_raises():
    from graphtrans_amd.evaluate import MolAP, evaluate
    model, batches, T = _mol_setup()
    for b in batches:
        b.y = torch.where(torch.isnan(b.y), b.y, torch.ones_like(b.y))     # every label positive: no task is valid
    with pytest.raises(RuntimeError, match="No positively labeled data|Cannot compute"):
        evaluate(model.train(), batches, MolAP(num_graphs=12, num_tasks=T))
    assert model.training                                                  # restored on the way out of an exception too


def test_tud_accuracy():
    from graphtrans_amd import synth
    from graphtrans_amd.evaluate import TudAccuracy, evaluate
    from graphtrans_amd.models.gnn import GNN
    torch.manual_seed(0)
    model = GNN(2, torch.nn.Linear(37, 64), lambda d: (lambda _e: 0), _gnn_args(max_seq_len=None)).to(DEV)
    batches = [synth.nci1_like(B=B, seed=s).to(DEV) for B, s in ((6, 1), (1, 2), (5, 3))]
    ev = TudAccuracy(num_graphs=12)
    model.train()
    result = evaluate(model, batches, ev)
    assert model.training
    correct = sum(int((eval_refs.argmax_rows(lg) == b.y.cpu().numpy()).sum()) for lg, b in zip(_host_logits(model, batches), batches))
    assert result == {"acc": correct / 12}
    assert evaluate(model, batches, ev) == result                          # reset() clears the device counter


class _Replay(torch.nn.Module):
    """a model that returns prepared logits, batch by batch"""

    def __init__(self, outs):
        super().__init__()
        self.outs, self.calls = outs, 0

    def forward(self, batch):
        self.calls += 1
        return self.outs[batch.k]


def test_single_node_batches_are_skipped_as_the_reference_loops_do():
    from graphtrans_amd.data import Batch
    from graphtrans_amd.evaluate import MolAP, TudAccuracy, evaluate
    g = torch.Generator().manual_seed(0)
    sizes = [(3, 7), (1, 1), (2, 5)]         # (graphs, node rows): the middle batch is one graph of one node
    logits = [torch.randn(B, 2, generator=g).to(DEV) for B, _ in sizes]
    ys = [torch.tensor([0, 1, 1]), torch.tensor([1]), torch.tensor([1, 0])]
    batches = [Batch(x=torch.zeros(n, 1, device=DEV), y=y.to(DEV), k=k) for k, ((_, n), y) in enumerate(zip(sizes, ys))]
    hits = [int((lg.cpu().argmax(1) == y).sum()) for lg, y in zip(logits, ys)]
    model = _Replay(logits)
    assert evaluate(model, batches, TudAccuracy(num_graphs=6)) == {"acc": sum(hits) / 6} and model.calls == 3    # dataset/tud.py: no skip
    assert evaluate(model, batches, TudAccuracy(num_graphs=6), skip_single_node=True) == {"acc": (hits[0] + hits[2]) / 6}
    for b, y in zip(batches, ys):
        b.y = torch.stack([y.float(), 1 - y.float()], 1).to(DEV)
    model.calls = 0
    mol = MolAP(num_graphs=6, num_tasks=2)
    result = evaluate(model, batches, mol)                                  # dataset/mol.py:44: the one-node batch is passed over
    assert mol.seen == 5 and model.calls == 2
    s = torch.cat([logits[0], logits[2]]).cpu().numpy()
    y = torch.cat([batches[0].y, batches[2].y]).cpu().numpy()
    aps = [eval_refs.average_precision(s[:, t], y[:, t]) for t in range(2)]
    assert all(ok for _, ok in aps) and abs(result["ap"] - (aps[0][0] + aps[1][0]) / 2) <= 13 * 2.0 ** -52


def test_update_enqueues_without_synchronising():
    """every evaluator's `update` under torch's sync debug mode: a `.item()`, a `.cpu()` or a boolean index would raise"""
    from graphtrans_amd.evaluate import Code2F1, MolAP, TudAccuracy, encode_code2_refs
    g = torch.Generator().manual_seed(0)
    ref_ids, n_ref = encode_code2_refs(_labels(12, 0), _vocab())
    f1, f1_ids = Code2F1(ref_ids, n_ref, NUM_VOCAB, SEQ, num_graphs=12), Code2F1(ref_ids, n_ref, NUM_VOCAB, SEQ, num_graphs=12)
    ap, acc = MolAP(num_graphs=12, num_tasks=4), TudAccuracy(num_graphs=12)
    sizes = (6, 1, 5)
    stacked = [torch.randn(B, SEQ * NUM_VOCAB + 2, generator=g).to(DEV)[:, :SEQ * NUM_VOCAB].view(B, SEQ, NUM_VOCAB) for B in sizes]
    heads = [[s[:, i] for i in range(SEQ)] for s in stacked]                # a plain list of views: what StackedHeads is
    gids = [torch.randint(0, 12, (B,), generator=g).to(DEV) for B in sizes]
    mol = [(torch.randn(B, 4, generator=g).to(DEV), (torch.rand(B, 4, generator=g) > 0.5).float().to(DEV)) for B in sizes]
    tud = [(torch.randn(B, 2, generator=g).to(DEV), torch.randint(0, 2, (B,), generator=g).to(DEV)) for B in sizes]
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for k in range(3):
            f1.update(stacked[k])
            f1_ids.update(heads[k], None, gids[k])
            ap.update(mol[k][0], mol[k][1])
            acc.update(tud[k][0], tud[k][1])
        with pytest.raises(RuntimeError):      # the mode is live: the read `result()` is there for does raise
            acc.count.item()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert f1.seen == f1_ids.seen == ap.seen == acc.seen == 12
    # and they computed what the statements say
    for ev, ids in ((f1, [range(0, 6), range(6, 7), range(7, 12)]), (f1_ids, [t.cpu().numpy() for t in gids])):
        want = _code2_statement([s.cpu().numpy() for s in stacked], ids, ref_ids, n_ref)
        res = ev.result()
        assert np.array_equal(ev.rows.cpu().numpy(), want)
        assert abs(res["F1"] - eval_refs.rows_mean(want)[2]) <= 12 * 2.0 ** -53
    hits = sum(int((p.cpu().argmax(1) == y.cpu()).sum()) for p, y in tud)
    assert acc.result() == {"acc": hits / 12}
    s, y = np.concatenate([p.cpu().numpy() for p, _ in mol]), np.concatenate([t.cpu().numpy() for _, t in mol])
    aps = [a for a, ok in (eval_refs.average_precision(s[:, t], y[:, t]) for t in range(4)) if ok]
    assert aps and abs(ap.result()["ap"] - sum(aps) / len(aps)) <= 20 * 2.0 ** -52
