"""The position-grouped output layer of the PNA baseline's heads (gt_head_group_*, csrc/mlp_heads.hip) at the shape of
configs/code2/pna/base.yml -- M = 128 graphs, G = 5 positions, K = 272, T = 5002 -- kernel by kernel, against what the library could
do for the same math without it: gt_linear_fwd_grouped / gt_linear_bwd_grouped on a logits buffer whose heads sit at a pitch of
c4(T) = 5004 columns (their y_group_stride must be a multiple of 4), plus the copy between that buffer and the contiguous
[M][G][T] logits losses.code2_loss reads (forward) and writes (the gradient).

Microseconds per call (device events around `--calls` back-to-back calls, median of `--reps`), random operands, fp32 and bf16 compute;
`weights_read_us` is ONE read of the 27.2 MB of weights at the 8 TB/s HBM figure bench.py uses.  One JSON line per compute mode.

    python tools/head_group_bench.py [--calls 50] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gnn_baseline_bench import DEV, HBM_GBS, timed   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", type=int, nargs=4, default=[128, 5, 272, 5002], metavar=("M", "G", "K", "T"))
    opt = ap.parse_args()
    from graphtrans_amd import _lib
    from graphtrans_amd.graph import _stream
    L = _lib.lib()
    M, G, K, T = opt.shape
    N, Tp = G * T, (T + 3) // 4 * 4
    ldy = (N + 3) // 4 * 4
    g = torch.Generator().manual_seed(0)
    H = torch.relu(torch.randn(M, G * K, generator=g)).to(DEV)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    Y, dY = torch.empty(M, ldy, device=DEV), torch.randn(M, ldy, generator=g).to(DEV)
    Yp, dYp = torch.empty(M, G * Tp, device=DEV), torch.zeros(M, G * Tp, device=DEV)
    dH, dW, db = torch.empty_like(H), torch.empty_like(W), torch.empty_like(b)
    p = lambda t: None if t is None else t.data_ptr()
    for name, compute in (("fp32", 0), ("bf16", 1)):
        wsb = int(L.gt_head_group_workspace_bytes(M, G, K, T))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
        wsb2 = int(L.gt_linear_bwd_grouped_workspace_bytes(compute, M, T, K, G))
        ws2 = torch.empty(max(wsb2, 16), dtype=torch.uint8, device=DEV)

        def bwd(dh, dw, dbias):
            return lambda n: [_lib.check(L.gt_head_group_bwd(compute, p(H), G * K, p(W), p(dY), ldy, 1, p(dh), G * K, p(dw), p(dbias), M, G, K, T,
                                                             p(ws), wsb, _stream()), "bwd") for _ in range(n)]
        runs = {
            "fwd": lambda n: [_lib.check(L.gt_head_group_fwd(compute, p(H), G * K, p(W), p(b), p(Y), ldy, M, G, K, T, _stream()), "fwd") for _ in range(n)],
            "dh": bwd(dH, None, None),
            "dw": bwd(None, dW, db),
            "pitched_fwd": lambda n: [_lib.check(L.gt_linear_fwd_grouped(0, 0, compute, p(H), p(W), p(b), p(Yp), M, T, K, G * K, G * Tp, G, K, Tp, 0, 0.0,
                                                                         0, _stream()), "grouped fwd") for _ in range(n)],
            "pitched_fwd_copy": lambda n: [Yp.view(M, G, Tp)[:, :, :T].contiguous() for _ in range(n)],
            "pitched_bwd": lambda n: [_lib.check(L.gt_linear_bwd_grouped(0, 0, compute, p(H), p(W), p(dYp), None, None, None, p(dH), p(dW), p(db), M, T, K,
                                                                         G * K, G * Tp, G, K, Tp, 0.0, p(ws2), wsb2, _stream()), "grouped bwd")
                                      for _ in range(n)],
            "pitched_bwd_copy": lambda n: [dYp.view(M, G, Tp)[:, :, :T].copy_(dY[:, :N].view(M, G, T)) for _ in range(n)],
        }
        res = dict(kernels="gt_head_group", compute=name, M=M, G=G, K=K, T=T, gflop_per_product=round(2 * M * K * N / 1e9, 3),
                   weights_read_us=round(N * K * 4 / (HBM_GBS * 1e9) * 1e6, 2))
        for tag, fn in runs.items():
            try:
                fn(5)
                res[tag + "_us"] = round(statistics.median(timed(fn, opt.calls) for _ in range(opt.reps)) * 1e3, 2)
            except RuntimeError as e:   # (the pitched route where the library does not take the shape)
                res[tag + "_error"] = str(e)[:160]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
