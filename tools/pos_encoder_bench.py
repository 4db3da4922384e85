"""What the packed token layout + fused step are worth for the `pos_encoder: True` configurations.

Workload: NCI1-shaped batches (synth.nci1_like) through the two model shapes of the reference's
configs/NCI1/gnn-transformer/no-virtual/ablation-pos_encoder (gd=128 l=3: GCN, 3 encoder layers; gin l=4: GIN, 4 encoder layers;
both 5 message-passing layers of width 128 -- the TU datasets' default --, d_model 128, ffn 256, cls pooling, norm_input, dropouts
0.1), forward + backward, at batch 32 and 256.
token_layout="padded" (pad_batch, torch add of pe, module-by-module: the only path such a model had) against token_layout="packed"
(the fused step), same parameters, same process, alternating, both warmed up first; device events around `--steps` steps, repeated
`--reps` times.  Prints one line per (config, batch) with the ms/step of every repetition and the ratio of the medians.

    python tools/pos_encoder_bench.py [--steps 200] [--reps 3] [--mode fp32|mixed]
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
CONFIGS = {"gd=128,l=3": dict(gnn_type="gcn", gnn_emb_dim=128, num_encoder_layers=3),
           "gin,l=4": dict(gnn_type="gin", gnn_emb_dim=128, num_encoder_layers=4)}


def build(cfg, dtype):
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    from oracle.reference_math import default_args
    args = default_args(gnn_virtual_node=False, graph_pooling="cls", transformer_norm_input=True, d_model=128, dim_feedforward=256,
                        transformer_dropout=0.1, gnn_dropout=0.1, pos_encoder=True, max_seq_len=None, compute_dtype=dtype,
                        token_layout="packed", **cfg)
    torch.manual_seed(0)
    packed = GNNTransformer(2, torch.nn.Linear(37, args.gnn_emb_dim), lambda _d: (lambda _x: 0), args).to(DEV).train()
    padded = copy.deepcopy(packed)
    padded.layout = "padded"
    return padded, packed


def steps(model, batches, loss_fn, n):
    for i in range(n):
        b = batches[i % len(batches)]
        for p in model.parameters():
            p.grad = None
        loss_fn(model(b), b.y).backward()


def timed(model, batches, loss_fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    steps(model, batches, loss_fn, n)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mode", default="fp32", choices=["fp32", "mixed"], help="mixed: bf16 token rows behind fp32 GEMMs (bench.py's default)")
    opt = ap.parse_args()
    from graphtrans_amd import engine, losses, synth
    dtype = torch.bfloat16 if opt.mode == "mixed" else torch.float32
    for name, cfg in CONFIGS.items():
        for B in (32, 256):
            padded, packed = build(cfg, dtype)
            batches = [synth.nci1_like(B=B, seed=s).to(DEV) for s in range(8)]
            assert engine.eligible(packed, batches[0], None) and not engine.eligible(padded, batches[0], None)
            loss_fn = losses.tud_loss
            for m in (padded, packed):
                steps(m, batches, loss_fn, opt.warmup)
            ms = {"padded": [], "packed": []}
            for _ in range(opt.reps):   # alternating: drift of the clocks hits both alike
                ms["padded"].append(timed(padded, batches, loss_fn, opt.steps))
                ms["packed"].append(timed(packed, batches, loss_fn, opt.steps))
            med = {k: statistics.median(v) for k, v in ms.items()}
            print(json.dumps(dict(config=name, mode=opt.mode, batch=B, nodes=int(batches[0].batch.numel()), steps=opt.steps,
                                  padded_ms=[round(v, 4) for v in ms["padded"]], packed_fused_ms=[round(v, 4) for v in ms["packed"]],
                                  speedup=round(med["padded"] / med["packed"], 3))), flush=True)


if __name__ == "__main__":
    main()
