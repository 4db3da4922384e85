"""The PNA baseline model (model_type "pna": PNA message passing -> per-graph pooling -> MLP heads) at the shape of
configs/code2/pna/base.yml: the fused step (the whole-model driver's read-out mode with the per-position heads) against the module path
of the same parameters.

Steps (zero the gradients, graph structure, forward, loss, backward -- bench.py's step with `--no-optimizer` --, batches with their
host-side sizes attached, same process, alternating, all warmed up first):
  code2   PNA, 4 layers of width 272, 4 towers, mean pooling, 5 positions x (Linear(272, 272) -> ReLU -> Linear(272, 5002)),
          synth.code2_like, batch 128
with exact-fp32 GEMMs (`fp32`; bench.py's `mixed` is the same here: no token rows) and with ops.set_matmul_dtype(bfloat16) (`bf16`).
Device events around `--steps` steps, `--reps` times: one JSON line per mode with the ms/step of every repetition, graphs/s at the
median and the module-path / fused ratio.

    python tools/pna_baseline_bench.py [--steps 50] [--reps 5]
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

from tools.gnn_baseline_bench import DEV, ORDER, attach_sizes, steps, timed   # noqa: E402


def build(B):
    from graphtrans_amd import losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder
    from graphtrans_amd.models.pna import PNANet
    b0 = synth.code2_like(B=B, seed=0)
    deg = torch.bincount(torch.bincount(b0.edge_index[1], minlength=b0.num_nodes))   # the in-degree histogram (dataset/code.py:122-130)
    args = SimpleNamespace(gnn_num_layer=4, gnn_emb_dim=272, gnn_dropout=0.3, gnn_residual=True, graph_pooling="mean", max_seq_len=5,
                           model_type="pna", aggregators=["mean", "max", "min", "std"], scalers=["identity", "amplification", "attenuation"],
                           deg=deg)
    model = PNANet(5002, ASTNodeEncoder(272, 98, 10030, 20), None, args)
    return model.to(DEV), (lambda s: synth.code2_like(B=B, seed=s)), (lambda out, b: losses.code2_loss(out, b.y_arr))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    opt = ap.parse_args()
    from graphtrans_amd import engine, ops
    B = opt.batch
    for mode in ("fp32", "bf16"):
        ops.set_matmul_dtype(torch.bfloat16 if mode == "bf16" else torch.float32)
        torch.manual_seed(0)
        fused, gen, loss_fn = build(B)
        fused.train()
        models = {"fused": fused, "module": copy.deepcopy(fused)}
        models["module"].fused = False
        batches = [attach_sizes(gen(s)).to(DEV) for s in range(8)]
        assert engine.eligible(fused, batches[0], None) and not engine.eligible(models["module"], batches[0], None)
        for k in ORDER:
            steps(models[k], batches, loss_fn, opt.warmup)
        plan = engine.state(fused)["plan"]
        assert plan.readout and plan.head_kind == 2
        ms = {k: [] for k in ORDER}
        for _ in range(opt.reps):   # alternating: drift of the clocks hits both alike
            for k in ORDER:
                ms[k].append(timed(lambda n, k=k: steps(models[k], batches, loss_fn, n), opt.steps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps(dict(model="pna", workload="code2", mode=mode, batch=B, nodes=int(batches[0].batch.numel()), steps=opt.steps,
                              **{k + "_ms": [round(v, 4) for v in ms[k]] for k in ORDER},
                              **{k + "_graphs_per_s": round(B / med[k] * 1e3, 1) for k in ORDER},
                              spread={k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
                              module_over_fused=round(med["module"] / med["fused"], 3))), flush=True)
    ops.set_matmul_dtype(torch.float32)


if __name__ == "__main__":
    main()
