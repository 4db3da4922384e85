"""What the fused step is worth under FLAG (`--fused_flag`, graphtrans_amd/flag.py).

Workload: one FLAG training step -- graphtrans_amd.flag.flag_step with m = 3 (three forward / backward passes with a perturbation that
requires a gradient, two ascents, one FusedAdamW step) -- on bench.py's models and synth batches with their host-side sizes attached:
Code2 GCN-Virtual at batch 256 and 32, Molpcba GIN-Virtual at batch 256.  Two copies of the same parameters, same process:
  (a) flag_off   fused_flag off: forward(batch, perturb) runs module by module (what a FLAG run did before the flag existed)
  (b) flag_on    fused_flag on: every forward / backward is the fused step, the second and third backward accumulate with one add
Both are warmed up, then timed alternately (device events around `--steps` steps, `--reps` repetitions each), first in the order
(a, b), then the whole run again in the order (b, a): drift of the clocks and whatever else the box is doing hit both alike.
Prints one JSON line per shape: the ms/step of every repetition in both orders, the run-to-run spread of each variant
((max - min) / median), and off / on from the medians over all repetitions.

    python tools/flag_bench.py [--steps 30] [--reps 5] [--mode mixed|fp32] [--shapes code2:256 code2:32 molpcba:256]
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
M, STEP_SIZE = 3, 8e-3


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def steps(model, opt, batches, loss_fn, n):
    from graphtrans_amd.flag import flag_step
    for i in range(n):
        flag_step(model, batches[i % len(batches)], opt, loss_fn, m=M, step_size=STEP_SIZE)


def timed(model, opt, batches, loss_fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    steps(model, opt, batches, loss_fn, n)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["code2:256", "code2:32", "molpcba:256"])
    ap.add_argument("--mode", default="mixed", choices=["fp32", "mixed"], help="mixed: bf16 token rows behind fp32 GEMMs (bench.py's default)")
    opt = ap.parse_args()
    from graphtrans_amd import engine
    from graphtrans_amd.optim import FusedAdamW
    bench = _bench_module()
    dtype = torch.bfloat16 if opt.mode == "mixed" else torch.float32
    for shape in opt.shapes:
        workload, B = shape.split(":")
        B = int(B)
        torch.manual_seed(0)
        _, base, gen, loss_fn, _ = bench.build(workload, dtype, torch.device(DEV), B)
        base.train()
        models = {"flag_off": base, "flag_on": copy.deepcopy(base)}
        models["flag_on"].fused_flag = True
        models["flag_off"].fused_flag = False
        opts = {k: FusedAdamW(m.parameters(), lr=1e-4, weight_decay=1e-2) for k, m in models.items()}
        batches = [bench.attach_sizes(gen(s)).to(DEV) for s in range(8)]
        N = int(batches[0].batch.numel())
        probe = torch.zeros((N, engine.emb_dim(base)), device=DEV).requires_grad_(True)
        assert engine.eligible(models["flag_on"], batches[0], probe) and not engine.eligible(models["flag_off"], batches[0], probe)
        for k in models:
            steps(models[k], opts[k], batches, loss_fn, opt.warmup)
        ms = {}
        for order in (("flag_off", "flag_on"), ("flag_on", "flag_off")):
            for _ in range(opt.reps):
                for k in order:
                    ms.setdefault((order[0], k), []).append(timed(models[k], opts[k], batches, loss_fn, opt.steps))
        allr = {k: [v for (_, kk), vs in ms.items() if kk == k for v in vs] for k in models}
        med = {k: statistics.median(v) for k, v in allr.items()}
        print(json.dumps(dict(workload=workload, mode=opt.mode, batch=B, nodes=N, m=M, steps=opt.steps,
                              **{f"{k}_ms_{first}_first": [round(v, 4) for v in ms[(first, k)]] for (first, k) in ms},
                              median_ms={k: round(v, 4) for k, v in med.items()},
                              spread={k: round((max(v) - min(v)) / med[k], 4) for k, v in allr.items()},
                              ratio_by_order={first: round(statistics.median(ms[(first, "flag_off")]) / statistics.median(ms[(first, "flag_on")]), 4)
                                              for first in ("flag_off", "flag_on")},
                              off_over_on=round(med["flag_off"] / med["flag_on"], 4))), flush=True)


if __name__ == "__main__":
    main()
