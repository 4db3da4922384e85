"""The masked encoder's attention mask: the host-made adj_list (dense fp32 (B, T, T) path) against keep-bits built on the device from the
batch's edges (ops.adjacency_bits), on one GNNTransformer with masked layers, forward + backward without the optimizer.

Shapes (bench.py's models of the same names with `--masked_layers` masked layers in front of the encoder, padded token layout):
  code2  synth.code2_like, batch 32      nci1  synth.nci1_like, batch 128
Arms, alternating in one process after a warm-up of both (tools/transformer_baseline_bench.py's scheme):
  dense  every batch carries `adj_list` (numpy, eye + edges, as the reference's data/adj_list.py makes it): today's path
  bits   the same batches without it
Same model object, same batches, dropout on: the two arms compute the same numbers (tests/test_hip_masked_model_edges.py).
Device events around `--steps` steps, `--reps` times per arm: one JSON line per shape with the ms/step of every repetition, the
spread of identical runs ((max - min) / median), bits / dense at the medians, and the mask build alone (`mask_build_ms`: the dense
arm's per-graph host-to-device copies into the zeroed (B, T, T) tensor against gt_adj_mask_bits, both from existing structures,
host clock around a device synchronise, median of `--reps` x 10 builds) with the bytes of either mask.

    python tools/adj_mask_bench.py [--steps 30] [--reps 5] [--shapes code2,nci1] [--masked_layers 2]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
SHAPES = {"code2": 32, "nci1": 128}


def build(shape, masked_layers):
    import bench
    from graphtrans_amd import losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    args = bench.model_args(shape, torch.float32)
    args.num_encoder_layers_masked, args.token_layout = masked_layers, "padded"
    D, B = args.gnn_emb_dim, SHAPES[shape]
    if shape == "code2":
        model = GNNTransformer(5002, ASTNodeEncoder(D, 98, 10030, 20), lambda d: torch.nn.Linear(2, d), args)
        return model.to(DEV), (lambda s: synth.code2_like(B=B, seed=s)), (lambda out, b: losses.code2_loss(out, b.y_arr))
    model = GNNTransformer(2, torch.nn.Linear(37, D), lambda _d: (lambda _x: 0), args)
    return model.to(DEV), (lambda s: synth.nci1_like(B=B, seed=s)), (lambda out, b: losses.tud_loss(out, b.y))


def host_adj_list(b):
    """data/adj_list.py:make_adj_list per graph: np.eye(n) with adj[row, col] = 1 for every edge"""
    sizes = torch.bincount(b.batch, minlength=b.num_graphs).numpy()
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    ei = b.edge_index.numpy()
    graph = np.searchsorted(ptr, ei[0], side="right") - 1
    out = []
    for g, n in enumerate(sizes):
        a = np.eye(n)
        sel = graph == g
        a[ei[0][sel] - ptr[g], ei[1][sel] - ptr[g]] = 1
        out.append(a)
    return sizes, out


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


def mask_build_ms(b_dense, reps):
    """median ms of building one batch's mask from what the step already has: (dense path, bits path)"""
    from graphtrans_amd import ops
    from graphtrans_amd.modules.gnn_module import batch_structure
    gs = batch_structure(b_dense)
    T = int(min(gs.sizes.max(), 1000))
    kv = torch.zeros(gs.B, T, dtype=torch.bool, device=DEV)

    def dense():
        m = torch.zeros((gs.B, T, T), device=DEV)
        for i, a in enumerate(b_dense.adj_list):   # models/gnn_transformer.py, the adj_list branch
            n = a.shape[0]
            m[i, 0:n, 0:n] = torch.from_numpy(np.asarray(a)).to(DEV)
        return m

    out = []
    for fn in (dense, lambda: ops.adjacency_bits(gs, T, key_valid=kv)):
        fn()
        ts = []
        for _ in range(10 * reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        out.append(statistics.median(ts))
    return out[0], out[1], gs.B * T * T * 4, gs.B * T * ((T + 31) // 32) * 4, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="code2,nci1")
    ap.add_argument("--masked_layers", type=int, default=2)
    opt = ap.parse_args()
    from graphtrans_amd import ops
    for shape in opt.shapes.split(","):
        ops.set_matmul_dtype(torch.float32)
        torch.manual_seed(0)
        model, gen, loss_fn = build(shape, opt.masked_layers)
        model.train()
        arms = {"dense": [], "bits": []}
        for s in range(4):
            b = gen(s)
            sizes, adj = host_adj_list(b)
            b._sizes = sizes
            arms["bits"].append(b.to(DEV))
            bd = copy.copy(b)
            bd.adj_list = adj
            arms["dense"].append(bd.to(DEV))
        order = ("dense", "bits")
        for k in order:
            steps(model, arms[k], loss_fn, opt.warmup)
        ms = {k: [] for k in order}
        for _ in range(opt.reps):   # alternating: drift of the clocks hits both alike
            for k in order:
                ms[k].append(timed(lambda n, k=k: steps(model, arms[k], loss_fn, n), opt.steps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        build_dense, build_bits, bytes_dense, bytes_bits, T = mask_build_ms(arms["dense"][0], opt.reps)
        print(json.dumps(dict(
            model="gnn_transformer+masked", shape=shape, batch=SHAPES[shape], nodes=int(arms["bits"][0].batch.numel()), T=T,
            masked_layers=opt.masked_layers, steps=opt.steps, **{k + "_ms": [round(v, 4) for v in ms[k]] for k in order},
            spread={k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()}, bits_over_dense=round(med["bits"] / med["dense"], 4),
            mask_build_ms=dict(dense=round(build_dense, 4), bits=round(build_bits, 4)),
            mask_bytes=dict(dense=bytes_dense, bits=bytes_bits))), flush=True)


if __name__ == "__main__":
    main()
