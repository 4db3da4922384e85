"""tests/aggregate_refs.py has teeth before a GPU sees it (runs without one).

* With no flaw and real-valued inputs `ref_aggregate` is oracle.reference_math.gcn_aggregate / gin_aggregate plus the self term, and
  autograd through them, to 1e-12 -- with the graph's real `deg`, so the reference is shown to be the op.
* For every case of the GPU test's table (aggregate_refs.all_spec_groups): the representability condition that makes the comparison an
  equality holds (assert_representable), and every deliberately wrong variant of the reference differs from the right one exactly
  where the case can show it: `differs == applies`, both ways.  Every variant applies in at least one fp32 and one bf16 case; the three
  tail variants apply in every case with edges.  Only the reference is made wrong here, never a kernel.
"""
import numpy as np
import pytest
import torch

import aggregate_refs as ar
from oracle import reference_math as rm


def _real_case(conv, mode, K, rows, dtype=torch.float64):
    N, D = 150, 20
    ei = ar.ladder_graph(N, 5)
    deg = np.bincount(ei[0], minlength=N) + 1.0   # GCN's deg (conv.py:57): out-degree + 1
    return ar.Case(conv, mode, N, D, ei, dtype=dtype, K=K, rows=rows, integer=False, deg=deg)


@pytest.mark.parametrize("mode,K,rows", [("none", 0, ()), ("linear", 1, ()), ("linear", 3, ()), ("tables", 2, (3, 1)), ("dense", 0, ())])
@pytest.mark.parametrize("conv", ar.CONVS)
def test_reference_is_the_oracles_op(conv, mode, K, rows):
    c = _real_case(conv, mode, K, rows)
    ref = ar.ref_aggregate(c)
    leaf = lambda t: None if t is None else t.clone().requires_grad_(True)
    h, root, w, b, tables, dense = (leaf(t) for t in (c.h, c.root, c.w, c.b, c.tables, c.dense))
    eps = torch.tensor([c.eps], dtype=torch.float64, requires_grad=True)
    e = {"none": lambda: None, "linear": lambda: c.attr @ w.t() + b, "dense": lambda: dense,
         "tables": lambda: sum(tables[c.tab_off[j] + c.attr[:, j]] for j in range(K))}[mode]()
    ei = torch.from_numpy(c.ei)
    assert torch.equal(rm.gcn_degree(ei, c.N, torch.float64), c.deg)
    out = rm.gcn_aggregate(h, e, ei, root) if conv == "gcn" else (1 + eps) * h + rm.gin_aggregate(h, e, ei)
    (out * c.g).sum().backward()
    close = lambda a, b, what: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12, msg=lambda m: f"{what}: {m}")
    close(ref["out"], out.detach(), "out")
    close(ref["grad_h"], h.grad, "grad_h")
    close(ref["d_self"], root.grad if conv == "gcn" else eps.grad, "d_self")
    if mode == "linear":
        close(ref["d_edge_w"], w.grad, "d_edge_w")
        close(ref["d_edge_b"], b.grad, "d_edge_b")
    elif mode == "tables":
        close(ref["d_edge_w"], tables.grad, "d_edge_w")
    elif mode == "dense":
        close(ref["d_dense"], dense.grad, "d_dense")


def test_ladder_graph_has_the_rows_it_promises():
    for N in (ar.SWEEP_N, 1000):
        ei = ar.graph(N)
        for end in (0, 1):   # out-degrees (CSC rows) and in-degrees (CSR rows)
            deg = np.bincount(ei[end], minlength=N)
            assert set(range(10)) <= set(deg.tolist()) and deg[N - 1] >= min(300, 4 * N) and (deg >= 65).sum() >= 2
            assert all(((deg % U == r) & (deg > U)).any() for U in (2, 4) for r in range(U))   # every tail residue after a full trip
            empty_beside_long = [i for i in range(1, N - 1) if deg[i] == 0 and deg[i - 1] >= 17 and deg[i + 1] >= 17 or
                                 deg[i] == 0 and deg[i - 1] == 0 and deg[i + 1] >= 33]
            assert empty_beside_long
        assert (ei[0] == ei[1]).any()                                           # self loops
        assert len({(int(a), int(b)) for a, b in ei.T}) < ei.shape[1]            # duplicates
        gs = ar.Case("gin", "none", N, 8, ei).gs
        assert (gs["in_eid"] != np.arange(ei.shape[1])).any()                    # edge id != CSR position


def _differs(case, flaw, want):
    """whether any output of the wrong variant differs from the right one's (the second direction is evaluated only if the first agrees)"""
    assert flaw in ar.FLAWS
    for part in (("bwd", "fwd") if flaw.startswith("gate") else ("fwd", "bwd")):
        got = {"out": ar.ref_forward(case, flaw)} if part == "fwd" else ar.ref_backward(case, flaw)
        if not ar.same(ar.expected(case, got), want):
            return True
    return False


@pytest.mark.parametrize("group", ar.all_spec_groups(), ids=lambda g: g[0])
def test_table_cases_are_exact_and_tell_the_wrong_variants_apart(group):
    for spec in group[1]:
        case = spec.make()
        ref = ar.ref_aggregate(case, with_abs=True)
        ar.assert_representable(case, ref)
        want = ar.expected(case, ref)
        for flaw in ar.FLAWS:
            applies = ar.flaw_applies(case, flaw)
            assert _differs(case, flaw, want) == applies, (spec.id, flaw, applies)
            if case.E and flaw in ("tail_dup_u2", "tail_dup_u4", "tail_drop"):
                assert applies, (spec.id, flaw)
    ar._GRAPHS.clear()


@pytest.mark.parametrize("dtype", [ar.F32, ar.BF16], ids=["float32", "bfloat16"])
def test_every_variant_applies_in_both_types(dtype):
    """already within the sweep at one width (whose cases the walk above shows to follow differs == applies)"""
    cases = [s.make() for s in ar.sweep_specs(dtype, 36)]
    for flaw in ar.FLAWS:
        assert any(ar.flaw_applies(c, flaw) for c in cases), flaw
