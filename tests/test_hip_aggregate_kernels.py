"""The GCN / GIN aggregate kernels (k_agg_fwd / k_agg_bwd, k_aggw_fwd / k_aggw_bwd, k_agg_reduce, k_eps_finish) against the float64
reference of tests/aggregate_refs.py, bit for bit, at every launch branch.

Inputs are small integers and dyadic GCN norms (see aggregate_refs): every sum of the op is exact in fp32 in any order, so `out`,
`grad_h`, `d_self` (GCN: D values; GIN: element 0), `d_edge_w`, `d_edge_b` and `d_dense` are compared with torch.equal.  Outputs and
the backward's workspace are pre-filled with NaN and sit between sentinels (aggregate_refs.launch_*): a row, a partial or a gradient
the kernels fail to write is a failure, and so is a write outside.  tests/test_aggregate_refs_host.py shows on the CPU that these very
cases tell the reference from eleven plausible kernel mistakes (a doubled or dropped tail edge, a stale prefetched index, ...).

a. sweep: every (lanes per node, chunks) / W instantiation x conv x edge variant on the ladder graph (N = 67): aggregate_refs.SWEEP_D
   and the map above it.
b. walks: forward walk lengths (a.chunk) 3, 3, 2, 8, 8 with the last wave-tile cut short mid-walk, backward on the same cases.
c. small: N = 1, 2, 3, 5, 9, N = 1 with self loops only, E = 0.
d. reduce: 1, 13, 125 and 501 partial rows (bwd_grid at N = 5, 100, 1000, 4001; 251 if only one block fits a CU): fewer blocks than
   waves, the 8-deep loop (more than 56 rows) and the 32-deep loop (more than 248) of k_agg_reduce.
e. tables: forward tables too large for LDS; the backward's LDS limit exactly, and one row over it (refused, nothing written).
f. real-valued data through ops.aggregate at the op's own tolerances, with a bitwise repeat.
"""
import numpy as np
import pytest
import torch

import aggregate_refs as ar
from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = ar.DEV


def _hint(case, name, got):
    """which deliberately wrong reference, if any, the kernel's output equals"""
    for flaw in ar.FLAWS:
        wrong = ar.expected(case, ar.ref_aggregate(case, flaw))
        if name in wrong and torch.equal(wrong[name], got):
            return f" (equals the reference with flaw {flaw})"
    return ""


def _run(specs):
    failures = []
    for spec in specs:
        case = spec.make()
        want = ar.expected(case, ar.ref_aggregate(case))
        got = {}
        if spec.fwd:
            got["out"] = ar.launch_fwd(case)
        if spec.bwd:
            got.update(ar.launch_bwd(case))
        assert set(got) == ({"out"} if spec.fwd else set()) | ({n for n in want if n != "out"} if spec.bwd else set()), (spec.id, sorted(got))
        for name, t in got.items():
            if not torch.equal(t, want[name]):
                bad = (t != want[name]).reshape(t.shape[0], -1)
                rows = torch.nonzero(bad.any(1)).flatten().tolist()
                failures.append(f"{spec.id}: {name}: {int(bad.sum())} of {bad.numel()} elements differ, rows {rows[:8]}{'...' if len(rows) > 8 else ''}"
                                f"{_hint(case, name, t) if case.N * case.D <= 1 << 18 else ''}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("D", ar.SWEEP_D[ar.F32])
def test_sweep_fp32(D):
    _run(ar.sweep_specs(ar.F32, D))


@pytest.mark.parametrize("D", ar.SWEEP_D[ar.BF16])
def test_sweep_bf16(D):
    _run(ar.sweep_specs(ar.BF16, D))


@pytest.mark.parametrize("conv", ar.CONVS)
@pytest.mark.parametrize("D,N,dtype", ar.WALK_PARAMS, ids=lambda v: str(v).replace("torch.", ""))
def test_walk_lengths(D, N, dtype, conv):
    assert ar.fwd_chunk(D, N) == {8: 3, 132: 3, 196: 2, 16: 8, 300: 8}[D]
    npw = 4 if D <= 64 else (2 if D <= 128 else 1)
    assert N % (ar.fwd_chunk(D, N) * npw) != 0   # the last wave-tile stops mid-walk
    _run([s for s in ar.walk_specs(D, N, dtype) if s.args[0] == conv])
    ar._GRAPHS.pop((N, "ladder"), None)


@pytest.mark.parametrize("D", ar.SMALL_D)
def test_small_and_empty_graphs(D):
    _run(ar.small_specs(D))


@pytest.mark.parametrize("N,D", ar.REDUCE_PARAMS)
def test_reduce_depths(N, D):
    _run(ar.reduce_specs(N, D))


def test_table_limits():
    _run(ar.table_limit_specs())
    case = ar.table_refused_spec().make()
    assert case.table_rows * case.D * 20 == 160 * 1024 + case.D * 20
    msg = ar.launch_bwd(case, expect_status=-2)   # GT_ERR_UNSUPPORTED; launch_bwd asserts that nothing was written
    assert "does not fit the per-wave LDS accumulators" in msg


@pytest.mark.parametrize("D,dtype", [(36, ar.F32), (132, ar.F32), (300, ar.F32), (516, ar.F32), (300, ar.BF16)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_real_valued_through_ops(D, dtype):
    """normal h and g, the graph's own deg / dis from GraphStructure.build, the autograd wrapper: float64 reference at the op's tolerances
    (1e-4 fp32, 3e-2 bf16, scale-relative as everywhere in the suite), and a second run that must repeat every bit"""
    from graphtrans_amd import ops
    from graphtrans_amd.graph import GraphStructure

    N = 1000
    ei = ar.graph(N)
    gs = GraphStructure.build(torch.from_numpy(ei).to(DEV), torch.zeros(N, dtype=torch.int64, device=DEV), num_graphs=1)
    deg = gs.deg.cpu().double()
    assert torch.equal(deg, torch.from_numpy(np.bincount(ei[0], minlength=N) + 1.0))
    tol = 1e-4 if dtype == ar.F32 else 3e-2
    for conv in ar.CONVS:
        for mode, K in (("linear", 3), ("none", 0)):
            case = ar.Case(conv, mode, N, D, ei, dtype=dtype, K=K, integer=False, deg=deg)
            ref = ar.ref_aggregate(case)
            runs = []
            for _ in range(2):
                h = case.h.to(dtype).to(DEV).requires_grad_(True)
                sp = (case.root.float().reshape(1, D) if conv == "gcn" else torch.tensor([case.eps], dtype=torch.float32)).to(DEV).requires_grad_(True)
                if mode == "linear":
                    w, b = case.w.float().to(DEV).requires_grad_(True), case.b.float().to(DEV).requires_grad_(True)
                    edge = ops.EdgeSpec("linear", attr=case.attr.float().to(DEV), weight=w, bias=b)
                else:
                    w = b = None
                    edge = ops.EdgeSpec("none")
                out = ops.aggregate(h, gs, conv, sp, edge)
                out.backward(case.g.to(dtype).to(DEV))
                torch.cuda.synchronize()
                got = {"out": out.detach(), "grad_h": h.grad, "d_self": sp.grad.reshape(-1)}
                if mode == "linear":
                    got.update(d_edge_w=w.grad, d_edge_b=b.grad)
                runs.append({n: t.cpu() for n, t in got.items()})
            for n, t in runs[0].items():
                assert_close(t.double(), ref[n], atol=tol, rtol=tol, what=f"{case.name} {n}")
                assert torch.equal(t, runs[1][n]), f"{case.name} {n}: the second run differs"
