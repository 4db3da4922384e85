"""The plain Transformer baseline (model_type "transformer": node encoder -> token rows -> TransformerNodeEncoder -> cls read-out ->
heads) on synthetic dataset-shaped batches: forward + backward without the optimizer, and for the two table encoders `fused_embed` on
(token rows straight from the embedding tables, ops.embed_tokens) against off (embed_sum -> + perturb -> seq_gather -> cast).

The three shipped shapes (configs/{code2,molpcba,NCI1}/transformer/pooling=cls.yml: d_model 256, 5 encoder layers, 4 heads, FFN 512,
max_input_len 1000):
  code2    ASTNodeEncoder, 5 stacked 5002-way heads, synth.code2_like, batch 16, dropout 0.3
  molpcba  AtomEncoder, one 128-way head, synth.molpcba_like, batch 256, dropout 0.3
  nci1     nn.Linear(37, 256) (no tables: the composition only), one 2-way head, synth.nci1_like, batch 128, dropout 0.1
Steps (zero the gradients, graph structure, forward, loss, backward), batches with their host-side sizes attached, same process, the
variants alternating, all warmed up first; token stream bf16 (`mixed`) or fp32.  `--perturb` adds a FLAG perturbation to every
forward.  Device events around `--steps` steps, `--reps` times for every variant: one JSON line per (workload, mode) with the ms/step of
every repetition, graphs/s at the median, the spread of identical runs ((max - min) / median) and composition / fused.

`--fused_step` adds a third variant to the alternation, `step`: the same model with `fused_step` on (and `fused_flag` under
`--perturb`; the Linear encoder keeps the module path with a perturbation), i.e. the whole step as one call per direction on the
whole-model driver.  Its baseline is the default module path in the same process (`fused`; `composition` for nci1):
`step_over_off` = ms/step of `step` / ms/step of that baseline at the medians.

    python tools/transformer_baseline_bench.py [--steps 50] [--reps 5] [--workloads code2,molpcba,nci1] [--modes mixed,fp32] [--fused_step]

Kernel times and launch counts come from a separate run under the profiler (kernel trace + statistics) of ONE variant, e.g.
`--workloads code2 --modes mixed --reps 1 --fused_step --variants step`.
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
SHAPES = {"code2": 16, "molpcba": 256, "nci1": 128}


def build(workload, compute_dtype):
    from graphtrans_amd import losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder, AtomEncoder
    from graphtrans_amd.models.transformer import Transformer
    B = SHAPES[workload]
    args = SimpleNamespace(d_model=256, nhead=4, dim_feedforward=512, transformer_dropout=0.1 if workload == "nci1" else 0.3,
                           transformer_activation="relu", num_encoder_layers=5, max_input_len=1000, transformer_norm_input=False,
                           graph_pooling="cls", max_seq_len=5 if workload == "code2" else None, model_type="transformer", gnn_type="gcn",
                           gnn_virtual_node=False, compute_dtype=compute_dtype)
    if workload == "code2":
        model = Transformer(5002, ASTNodeEncoder(256, 98, 10030, 20), None, args)
        return model.to(DEV), (lambda s: synth.code2_like(B=B, seed=s)), (lambda out, b: losses.code2_loss(out, b.y_arr))
    if workload == "molpcba":
        model = Transformer(128, AtomEncoder(256), None, args)
        return model.to(DEV), (lambda s: synth.molpcba_like(B=B, seed=s)), (lambda out, b: losses.mol_loss(out, b.y))
    model = Transformer(2, torch.nn.Linear(37, 256), None, args)
    return model.to(DEV), (lambda s: synth.nci1_like(B=B, seed=s)), (lambda out, b: losses.tud_loss(out, b.y))


def attach_sizes(b):
    b._sizes = torch.bincount(b.batch, minlength=b.num_graphs).numpy()
    return b


def steps(model, batches, perturbs, loss_fn, n):
    for i in range(n):
        b = batches[i % len(batches)]
        b.__dict__.pop("_gt_structure", None)   # the graph structure is part of the step, as in bench.py
        for p in model.parameters():
            p.grad = None
        pt = None
        if perturbs is not None:
            pt = perturbs[i % len(batches)]
            pt.grad = None
        loss_fn(model(b, pt), b).backward()


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn(n)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default="code2,molpcba,nci1")
    ap.add_argument("--modes", default="mixed,fp32")
    ap.add_argument("--perturb", action="store_true", help="a FLAG perturbation in every forward")
    ap.add_argument("--fused_step", action="store_true", help="add the variant with model.fused_step on (the whole-model driver)")
    ap.add_argument("--variants", default="", help="run only these variants (comma list of fused,composition,step): profiler runs")
    opt = ap.parse_args()
    from graphtrans_amd import ops
    for workload in opt.workloads.split(","):
        for mode in opt.modes.split(","):
            ops.set_matmul_dtype(torch.float32)
            torch.manual_seed(0)
            fused, gen, loss_fn = build(workload, torch.bfloat16 if mode == "mixed" else torch.float32)
            fused.train()
            models = {"fused": fused, "composition": copy.deepcopy(fused)}
            models["fused"].fused_embed, models["composition"].fused_embed = True, False
            order = ("fused", "composition") if workload != "nci1" else ("composition",)   # (no tables: one variant, repeated)
            base = order[0]   # `fused_step` off with everything else at its default: today's path
            if opt.fused_step:
                models["step"] = copy.deepcopy(fused)
                models["step"].fused_step = models["step"].fused_flag = True
                order = order + ("step",)
            if opt.variants:
                order = tuple(k for k in order if k in opt.variants.split(","))
            batches = [attach_sizes(gen(s)).to(DEV) for s in range(8)]
            perturbs = None
            if opt.perturb:
                perturbs = [torch.empty(b.batch.numel(), 256, device=DEV).uniform_(-8e-3, 8e-3).requires_grad_(True) for b in batches]
            for k in order:
                steps(models[k], batches, perturbs, loss_fn, opt.warmup)
            ms = {k: [] for k in order}
            for _ in range(opt.reps):   # alternating: drift of the clocks hits both alike
                for k in order:
                    ms[k].append(timed(lambda n, k=k: steps(models[k], batches, perturbs, loss_fn, n), opt.steps))
            med = {k: statistics.median(v) for k, v in ms.items()}
            B = SHAPES[workload]
            res = dict(model="transformer", workload=workload, mode=mode, batch=B, nodes=int(batches[0].batch.numel()), steps=opt.steps,
                       perturb=bool(opt.perturb), **{k + "_ms": [round(v, 4) for v in ms[k]] for k in order},
                       **{k + "_graphs_per_s": round(B / med[k] * 1e3, 1) for k in order},
                       spread={k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()})
            if "fused" in med and "composition" in med:
                res["composition_over_fused"] = round(med["composition"] / med["fused"], 4)
            if "step" in med and base in med:
                res["step_over_off"] = round(med["step"] / med[base], 4)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
