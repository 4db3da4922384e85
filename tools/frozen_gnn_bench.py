"""What the fused step is worth once `--freeze_gnn` has frozen gnn_node (`--fused_freeze`, engine.frozen_pattern).

Workload: bench.py's Code2 GCN-Virtual model (5 GCN layers of width 300 with a virtual node, JK = cat, 4 encoder layers d_model 128,
cls pooling, norm_input, 5 stacked heads) on synth.code2_like batches with their host-side sizes attached, forward + backward, at
batch 256 and 32.  Three steps of the same parameters, same process, alternating, all warmed up first:
  (a) frozen_module   gnn_node frozen, fused_freeze off: the module-by-module path (what a frozen model ran before the flag existed)
  (b) frozen_fused    gnn_node frozen, fused_freeze on: the fused forward + a backward that stops behind gnn2transformer
  (c) full_fused      everything trainable: the full fused step ((b)'s launches are a subset of its launches)
Device events around `--steps` steps, repeated `--reps` times.  Prints one JSON line per batch size with the ms/step of every
repetition, the run-to-run spread of each configuration ((max - min) / median over the repetitions) and the ratios of the medians.

    python tools/frozen_gnn_bench.py [--steps 100] [--reps 5] [--mode mixed|fp32]
"""
import argparse
import copy
import importlib.util
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
ORDER = ("frozen_module", "frozen_fused", "full_fused")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def steps(model, batches, loss_fn, n):
    for i in range(n):
        b = batches[i % len(batches)]
        for p in model.parameters():
            p.grad = None
        loss_fn(model(b), b).backward()


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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 32])
    ap.add_argument("--mode", default="mixed", choices=["fp32", "mixed"], help="mixed: bf16 token rows behind fp32 GEMMs (bench.py's default)")
    opt = ap.parse_args()
    from graphtrans_amd import engine
    bench = _bench_module()
    dtype = torch.bfloat16 if opt.mode == "mixed" else torch.float32
    for B in opt.batches:
        torch.manual_seed(0)
        _, full, gen, loss_fn, _ = bench.build("code2", dtype, torch.device(DEV), B)
        full.train()
        full.fused_freeze = True
        models = {"full_fused": full, "frozen_fused": copy.deepcopy(full), "frozen_module": copy.deepcopy(full)}
        for k in ("frozen_fused", "frozen_module"):
            models[k].gnn_node.requires_grad_(False)
        models["frozen_module"].fused_freeze = False
        batches = [bench.attach_sizes(gen(s)).to(DEV) for s in range(8)]
        assert engine.eligible(full, batches[0], None) and engine.eligible(models["frozen_fused"], batches[0], None)
        assert not engine.eligible(models["frozen_module"], batches[0], None)
        for k in ORDER:
            steps(models[k], batches, loss_fn, opt.warmup)
        assert engine.state(models["frozen_fused"])["plan"].frozen and not engine.state(full)["plan"].frozen
        ms = {k: [] for k in ORDER}
        for _ in range(opt.reps):   # alternating: drift of the clocks hits all three alike
            for k in ORDER:
                ms[k].append(timed(models[k], batches, loss_fn, opt.steps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        print(json.dumps(dict(workload="code2", mode=opt.mode, batch=B, nodes=int(batches[0].batch.numel()), steps=opt.steps,
                              **{k + "_ms": [round(v, 4) for v in ms[k]] for k in ORDER},
                              spread={k: round(v, 4) for k, v in spread.items()},
                              frozen_fused_vs_module=round(med["frozen_module"] / med["frozen_fused"], 3),
                              frozen_fused_vs_full=round(med["frozen_fused"] / med["full_fused"], 3))), flush=True)


if __name__ == "__main__":
    main()
