"""`result(group)` of the four evaluators with two real ranks: both processes share cuda:0 and exchange over gloo, as
tests/test_hip_dp.py does.  Every rank must receive the dict that one evaluator fed the ranks' shards in rank order returns:
MolAP, MolRocAuc (the gathered table is that evaluator's table) and TudAccuracy (integers) bit for bit, Code2F1 (float64 sums
added per rank, then across ranks) within n * 2^-53 of math.fsum of the union's per-graph rows divided by n.  Round 0 shards
7 + 4 graphs, round 1 leaves rank 1 without a graph.  No model: the workers feed `update` directly."""
import datetime
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NUM_VOCAB, SEQ, TASKS = 50, 5, 3
SHARDS = [(7, 4), (7, 0)]        # graphs on (rank 0, rank 1), round by round
CAP = (7, 4)                     # what each rank's evaluators are built for: its shard of round 0


def _refs():
    from graphtrans_amd.evaluate import encode_code2_refs
    vocab = {"w%d" % i: i for i in range(NUM_VOCAB - 2)}
    vocab["__UNK__"], vocab["__EOS__"] = NUM_VOCAB - 2, NUM_VOCAB - 1
    rng = np.random.default_rng(0)
    seqs = [[("w%d" % rng.integers(0, 6)) if rng.random() < 0.8 else "oov" for _ in range(int(rng.integers(1, 6)))] for _ in range(11)]
    return encode_code2_refs(seqs, vocab)


def _shard(rnd, rank):
    """what rank `rank` sees in round `rnd`, on the device: Code2 logits with graph ids, Molecule scores with labels, TU logits
    with labels; None for an empty shard"""
    B = SHARDS[rnd][rank]
    if B == 0:
        return None
    g = torch.Generator().manual_seed(100 * rnd + rank)
    lo = sum(SHARDS[rnd][:rank])
    code = torch.randn(B, SEQ, NUM_VOCAB, generator=g)
    code[:, :, :6] += 2.0                                                   # words 0..5 win often: precision and recall above 0
    code[:, 2:, NUM_VOCAB - 1] += 3.0                                       # and __EOS__ ends many predictions
    gids = torch.arange(lo, lo + B).flip(0)
    mol = (torch.round(torch.randn(B, TASKS, generator=g) * 2) / 2)         # halves: scores tie within and across ranks
    y = (torch.rand(B, TASKS, generator=g) > 0.5).float()
    y[torch.rand(B, TASKS, generator=g) < 0.2] = float("nan")
    y[0, 0], y[1, 0] = 1.0, 0.0                                             # task 0 is valid on every shard
    tud = torch.randn(B, 2, generator=g)
    ty = torch.randint(0, 2, (B,), generator=g)
    return tuple(t.to(DEV) for t in (code, gids, mol, y, tud, ty))


def _evaluators(num_graphs):
    from graphtrans_amd.evaluate import Code2F1, MolAP, MolRocAuc, TudAccuracy
    ref_ids, n_ref = _refs()
    return dict(f1=Code2F1(ref_ids, n_ref, NUM_VOCAB, SEQ, num_graphs=num_graphs), ap=MolAP(num_graphs, TASKS),
                rocauc=MolRocAuc(num_graphs, TASKS), acc=TudAccuracy(num_graphs))


def _feed(evs, shard):
    if shard is None:
        return
    code, gids, mol, y, tud, ty = shard
    evs["f1"].update(code, None, gids)
    evs["ap"].update(mol, y)
    evs["rocauc"].update(mol, y)
    evs["acc"].update(tud, ty)


def _reset(evs):
    for ev in evs.values():
        ev.reset()


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))   # a lost peer fails, not hangs
    group = dist.group.WORLD
    evs = _evaluators(CAP[rank])
    for rnd in range(len(SHARDS)):
        _reset(evs)
        _feed(evs, _shard(rnd, rank))
        out[("ranks", rnd, rank)] = {k: ev.result(group) for k, ev in evs.items()}
        if SHARDS[rnd][rank]:
            out[("local", rnd, rank)] = {k: ev.result() for k, ev in evs.items()}      # no group: this rank's own number
    dist.destroy_process_group()


def test_two_ranks_receive_the_single_process_result():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    out = dict(out)
    one = _evaluators(sum(CAP))                    # TudAccuracy divides by the graphs its evaluators were built for: 7 + 4
    for rnd, sizes in enumerate(SHARDS):
        n = sum(sizes)
        _reset(one)
        for rank in range(2):
            _feed(one, _shard(rnd, rank))
        want = {k: ev.result() for k, ev in one.items()}
        got = out[("ranks", rnd, 0)]
        print(f"round {rnd}: ranks {got}\n         one process {want}")
        assert got == out[("ranks", rnd, 1)]                                   # every rank holds the same dict
        assert set(got) == set(want)
        for k in ("ap", "rocauc", "acc"):
            assert got[k] == want[k], (rnd, k)                                 # bit for bit
        rows = one["f1"].rows[:n].cpu().numpy()
        assert set(got["f1"]) == {"precision", "recall", "F1"}
        for c, name in enumerate(("precision", "recall", "F1")):
            exact = math.fsum(rows[:, c].tolist()) / n
            assert abs(got["f1"][name] - exact) <= n * 2.0 ** -53, (rnd, name, got["f1"][name], exact)
        assert rows[:, 2].max() > 0.0                                          # the rows are not all zero
        for rank, B in enumerate(sizes):                                       # result() without a group stays local
            if B == 0:
                assert ("local", rnd, rank) not in out
                continue
            alone = _evaluators(CAP[rank])
            _feed(alone, _shard(rnd, rank))
            assert out[("local", rnd, rank)] == {k: ev.result() for k, ev in alone.items()}, (rnd, rank)
        if sizes[1]:
            assert out[("local", rnd, 0)]["acc"] != got["acc"] or out[("local", rnd, 0)]["rocauc"] != got["rocauc"]
