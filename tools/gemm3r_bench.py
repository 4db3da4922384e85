#!/usr/bin/env python
"""The split GEMMs on bound weight images alone on the chip: k_lin3r (rows straight into MFMA fragments, csrc/linear3r.h; M >= 12 288) or
k_lin3 (both operands through the LDS) forward, un-gated dX, dX with an addend, and the weight gradient (k_lin3r_dw + its reduce), under
"highest" (six bf16 products per fp32 product) and "high" (three: compute = GT_COMPUTE_F32_HIGH), alternating in the same process.
usage: python tools/gemm3r_bench.py [--precision highest|high|both] [--shapes MxNxK,...] [--rounds R]
(GPU box; A/B against another build: GT_LIB_PATH)"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from graphtrans_amd import _lib
from graphtrans_amd.graph import _stream
from graphtrans_amd.w3 import W3Images

DEV = "cuda:0"
CODES = {"highest": 0, "high": 2}   # enum gt_compute
DEFAULT_SHAPES = [(31598, 300, 300), (131072, 256, 256), (16000, 272, 272), (31598, 600, 300), (31598, 300, 600), (12800, 300, 300), (6700, 600, 300)]


def timeit(fn, n=100):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cur = torch.cuda.current_stream(0)
    s.record(cur)
    for _ in range(n):
        fn()
    e.record(cur)
    torch.cuda.synchronize()
    return 1e3 * s.elapsed_time(e) / n


def _p(t):
    return None if t is None else t.data_ptr()


class Gemm:
    def __init__(self, M, N, K):
        self.M, self.N, self.K = M, N, K
        self.x = torch.randn(M, K, device=DEV)
        self.W = torch.randn(N, K, device=DEV) / K ** 0.5
        self.b = torch.randn(N, device=DEV)
        self.dy = torch.randn(M, N, device=DEV)
        self.a1 = torch.randn(M, K, device=DEV)
        self.y, self.dx = torch.empty(M, N, device=DEV), torch.empty(M, K, device=DEV)
        self.dw, self.db = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
        self.ws_bytes = _lib.lib().gt_linear_bwd_workspace_bytes(0, M, N, K)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=DEV)
        self.imgs = W3Images([self.W])
        self.imgs.build()

    def fwd(self, c):
        _lib.launch("gt_linear_fwd_ld2", 0, 0, c, _p(self.x), _p(self.W), _p(self.b), _p(self.y), self.M, self.N, self.K, self.K, self.N, 0, 0.0, 0, _stream())

    def bwd(self, c, dx, dw, add=None):
        _lib.launch("gt_linear_bwd_ld2", 0, 0, c, _p(self.x) if dw else None, _p(self.W), _p(self.dy), None, _p(add), None, _p(self.dx) if dx else None,
                    _p(self.dw) if dw else None, _p(self.db) if dw else None, self.M, self.N, self.K, self.K, self.N, 0.0, _p(self.ws), self.ws_bytes, _stream())

    def products(self, which, c):
        return _lib.lib().gt_linear_products(which, 0, 0, c, _p(self.W), self.M, self.N, self.K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=["highest", "high", "both"], default="both")
    ap.add_argument("--shapes", default="")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds per shape; the median is reported with min .. max")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s] or DEFAULT_SHAPES
    precisions = ["highest", "high"] if a.precision == "both" else [a.precision]
    for M, N, K in shapes:
        g = Gemm(M, N, K)
        fl = 2.0 * M * N * K
        forms = [("fwd", lambda c: g.fwd(c), 0), ("dX", lambda c: g.bwd(c, True, False), 1), ("dX+addend", lambda c: g.bwd(c, True, False, g.a1), 1),
                 ("dW+db+reduce", lambda c: g.bwd(c, False, True), 2)]
        times = {(f, p): [] for f, _, _ in forms for p in precisions}
        with g.imgs.bound():
            for _ in range(a.rounds):
                for f, fn, _ in forms:
                    for p in precisions:   # the two precisions back to back: same clocks, same neighbours
                        times[(f, p)].append(timeit(lambda: fn(CODES[p]), n=50 if f.startswith("dW") else 100))
            prods = {(f, p): g.products(which, CODES[p]) for f, _, which in forms for p in precisions}
        for f, _, _ in forms:
            row = []
            for p in precisions:
                t = sorted(times[(f, p)])
                med = t[len(t) // 2]
                row.append(f"{p} ({prods[(f, p)]} products) {med:6.1f} us [{t[0]:.1f} .. {t[-1]:.1f}] {fl / med / 1e6:6.1f} TF")
            ratio = ""
            if len(precisions) == 2:
                h6, h3 = sorted(times[(f, "highest")]), sorted(times[(f, "high")])
                ratio = f"  high / highest = {h3[len(h3) // 2] / h6[len(h6) // 2]:.3f}"
            print(f"{M:7d} x {N:4d} x {K:4d} {f:13s}: " + "   ".join(row) + ratio, flush=True)


if __name__ == "__main__":
    main()
