"""The GNN baseline model (model_type "gnn": message passing -> per-graph pooling -> heads) on synthetic batches: the fused step (the
whole-model driver's read-out mode) against the module path of the same parameters, and the pooling kernels alone.

Steps (zero the gradients, graph structure, forward, loss, backward -- bench.py's step with `--no-optimizer` --, batches with their
host-side sizes attached, same process, alternating, all warmed up first):
  code2   GCN-Virtual, 5 layers of width 300, JK = last, mean pooling, 5 stacked 5002-way heads, synth.code2_like, batch 256 and 32
  nci1    GCN, 3 layers of width 128, JK = last, mean pooling, one 2-way head, synth.nci1_like, batch 32
in the `mixed` and `fp32` modes of bench.py.  The model has no token rows, so the two modes differ in nothing the model runs (fp32-stored,
exact-fp32 GEMMs in both): the second is a repeat, and its distance from the first is the run-to-run spread.
Device events around `--steps` steps, `--reps` times: one JSON line per (workload, batch, mode) with the ms/step of every repetition,
graphs/s at the median and the module-path / fused ratio.

Pooling kernels alone at the Code2 b256 shape (N x 300 fp32): microseconds per gt_graph_pool_fwd / gt_graph_pool_bwd call and that time
over the time of ONE read of the N x D fp32 rows at the 8 TB/s HBM figure bench.py uses (`x_one_read`; the rows of a looped call sit in
the Infinity Cache, so values below 1 are possible and say nothing about HBM).

    python tools/gnn_baseline_bench.py [--steps 100] [--reps 5]
"""
import argparse
import copy
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
HBM_GBS = 8000.0
ORDER = ("fused", "module")


def build(workload, B):
    from graphtrans_amd import losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn import GNN
    a = dict(gnn_virtual_node=True, gnn_num_layer=5, gnn_emb_dim=300, gnn_JK="last", gnn_dropout=0.0, gnn_residual=False, gnn_type="gcn",
             graph_pooling="mean", max_seq_len=5, model_type="gnn")
    if workload == "nci1":
        a.update(gnn_virtual_node=False, gnn_num_layer=3, gnn_emb_dim=128, gnn_dropout=0.5, max_seq_len=None)
    args = SimpleNamespace(**a)
    if workload == "code2":
        model = GNN(5002, ASTNodeEncoder(300, 98, 10030, 20), lambda d: torch.nn.Linear(2, d), args)
        return model.to(DEV), (lambda s: synth.code2_like(B=B, seed=s)), (lambda out, b: losses.code2_loss(out, b.y_arr))
    model = GNN(2, torch.nn.Linear(37, 128), lambda d: (lambda _e: 0), args)
    return model.to(DEV), (lambda s: synth.nci1_like(B=B, seed=s)), (lambda out, b: losses.tud_loss(out, b.y))


def attach_sizes(b):
    b._sizes = torch.bincount(b.batch, minlength=b.num_graphs).numpy()
    return b


def steps(model, batches, loss_fn, n):
    for i in range(n):
        b = batches[i % len(batches)]
        b.__dict__.pop("_gt_structure", None)   # the graph structure is part of the step, as in bench.py
        for p in model.parameters():
            p.grad = None
        loss_fn(model(b), b).backward()


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn(n)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def bench_steps(opt):
    from graphtrans_amd import engine, ops
    for workload, B in (("code2", 256), ("code2", 32), ("nci1", 32)):
        for mode in ("mixed", "fp32"):
            ops.set_matmul_dtype(torch.float32)
            torch.manual_seed(0)
            fused, gen, loss_fn = build(workload, B)
            fused.train()
            models = {"fused": fused, "module": copy.deepcopy(fused)}
            models["module"].fused = False
            batches = [attach_sizes(gen(s)).to(DEV) for s in range(8)]
            assert engine.eligible(fused, batches[0], None) and not engine.eligible(models["module"], batches[0], None)
            for k in ORDER:
                steps(models[k], batches, loss_fn, opt.warmup)
            assert engine.state(fused)["plan"].readout
            ms = {k: [] for k in ORDER}
            for _ in range(opt.reps):   # alternating: drift of the clocks hits both alike
                for k in ORDER:
                    ms[k].append(timed(lambda n, k=k: steps(models[k], batches, loss_fn, n), opt.steps))
            med = {k: statistics.median(v) for k, v in ms.items()}
            print(json.dumps(dict(model="gnn", workload=workload, mode=mode, batch=B, nodes=int(batches[0].batch.numel()), steps=opt.steps,
                                  **{k + "_ms": [round(v, 4) for v in ms[k]] for k in ORDER},
                                  **{k + "_graphs_per_s": round(B / med[k] * 1e3, 1) for k in ORDER},
                                  spread={k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
                                  module_over_fused=round(med["module"] / med["fused"], 3))), flush=True)


def bench_kernels(opt):
    from graphtrans_amd import _lib, synth
    from graphtrans_amd.graph import GraphStructure, _stream
    L = _lib.lib()
    b = attach_sizes(synth.code2_like(B=256, seed=0)).to(DEV)
    gs = GraphStructure.build(b.edge_index, b.batch, num_graphs=256, sizes=b._sizes)
    N, B, D = gs.N, gs.B, 300
    x = torch.randn(N, D, device=DEV)
    out, d_out, dx = torch.empty(B, D, device=DEV), torch.randn(B, D, device=DEV), torch.empty(N, D, device=DEV)
    arg = torch.empty(B, D, dtype=torch.int32, device=DEV)
    read_us = N * D * 4 / (HBM_GBS * 1e9) * 1e6
    res = dict(kernels="gt_graph_pool", nodes=N, graphs=B, dim=D, largest_graph=int(b._sizes.max()), one_read_us=round(read_us, 2))
    for name, kind in (("sum", 1), ("mean", 2), ("max", 3)):
        wsb = int(L.gt_graph_pool_workspace_bytes(kind, N, D))
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        a = arg.data_ptr() if kind == 3 else None

        def fwd(n, ws_ptr=ws.data_ptr(), wsb=wsb):
            for _ in range(n):
                _lib.check(L.gt_graph_pool_fwd(kind, 0, x.data_ptr(), gs.graph_ptr.data_ptr(), N, B, D, out.data_ptr(), a, ws_ptr, wsb, _stream()), "fwd")

        def bwd(n):
            for _ in range(n):
                _lib.check(L.gt_graph_pool_bwd(kind, 0, d_out.data_ptr(), a, gs.graph_ptr.data_ptr(), gs.node_graph.data_ptr(), N, B, D,
                                               dx.data_ptr(), _stream()), "bwd")
        for tag, fn in (("fwd", fwd), ("fwd_one_block_per_graph", lambda n: fwd(n, None, 0)), ("bwd", bwd)):
            fn(20)
            us = statistics.median(timed(fn, 200) for _ in range(opt.reps)) * 1e3
            res[f"{name}_{tag}_us"] = round(us, 2)
            res[f"{name}_{tag}_x_one_read"] = round(us / read_us, 2)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["steps", "kernels"])
    opt = ap.parse_args()
    if opt.only != "steps":
        bench_kernels(opt)
    if opt.only != "kernels":
        bench_steps(opt)


if __name__ == "__main__":
    main()
