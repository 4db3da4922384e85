"""Batch assembly from the HBM-resident graph store (`GraphStore.collate`, csrc/collate.hip) at the batch shapes of the README's
step-time table, and the PNA in-degree histogram (`GraphStore.degree_histogram`) against its numpy statement.

Rows (a store of `--store` graphs, every call collates a fresh random selection of `batch` of them, as a shuffling sampler would):
  nci1     b32, b128   synth.nci1_raw     x (N,37) f32, no edge features
  er       b256        synth.er_raw       x (N,256) f32, edge_attr (E,2) f32, n = 512
  code2    b256        synth.code2_raw    int64 x, augment_edge on the device
  molpcba  b256        synth.molpcba_raw  int64 x and edge_attr
Per row, one JSON line: `device_us` = median over `--calls` calls of the time between two HIP events around one `store.collate(ids)`
(the id upload, the output allocations from the caching allocator and the two launches), its quartiles, `launch_us` = the same
median with the events directly around the `gt_collate` call (the two launches alone), and `host_us` = host wall time per call of
the first loop (device drained once at the end).  The host is the slower side at these sizes, so `device_us` includes the time the
stream waits for the next enqueue.  Then one line for the histogram over a Code2-shaped store of
`--hist-graphs` graphs: the first call (in-degrees + histogram), later calls (the in-degrees are cached on the store), and the numpy
statement (augment_edge + bincount per graph, dataset/code.py:122-130) on the same machine.

`--root DIR` imports graphtrans_amd from another checkout (e.g. the parent commit, built in place) to measure the int64 rows with
that revision's library in the same visit; `--rows` selects rows, `--no-hist` skips the histogram.

    python tools/collate_bench.py [--calls 300] [--warmup 30] [--rows nci1,er,code2,molpcba] [--root DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROWS = [("nci1", 32), ("nci1", 128), ("er", 256), ("code2", 256), ("molpcba", 256)]


def raw_graphs(synth, workload, G):
    if workload == "nci1":
        return synth.nci1_raw(G, 0)
    if workload == "er":
        return synth.er_raw(G, 0)
    if workload == "code2":
        return synth.code2_raw(G, 0)
    return synth.molpcba_raw(G, 0)


def time_collate(_lib, store, B, calls, warmup, seed=0):
    rng = np.random.default_rng(seed)
    ids = [rng.permutation(len(store))[:B] for _ in range(warmup + calls)]
    for i in ids[:warmup]:
        store.collate(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    t0 = time.perf_counter()
    for i, (s, e) in zip(ids[warmup:], ev):
        s.record()
        b = store.collate(i)
        e.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) / calls
    us = sorted(1e3 * s.elapsed_time(e) for s, e in ev)
    q = statistics.quantiles(us, n=4)
    # the C call alone (k_collate_offsets + k_collate_fill): events inside _lib.launch, without the Python around it
    _lib.TIMER = timer = _lib.KernelTimer(["gt_collate"])
    for i in ids[warmup:]:
        store.collate(i)
    _lib.TIMER = None
    torch.cuda.synchronize()
    launch_us = statistics.median(1e3 * s.elapsed_time(e) for _, s, e, _ in timer.records)
    out_bytes = sum(v.numel() * v.element_size() for v in b.__dict__.values() if isinstance(v, torch.Tensor))
    return dict(device_us=round(statistics.median(us), 2), device_us_q1=round(q[0], 2), device_us_q3=round(q[2], 2),
                launch_us=round(launch_us, 2), host_us=round(1e6 * host, 2), nodes=int(b.batch.numel()), edges=int(b.edge_index.shape[1]), batch_bytes=int(out_bytes))


def time_histogram(synth, GraphStore, G, reps):
    from oracle import collate as oc
    raw = synth.code2_raw(G, 1)
    store = GraphStore(raw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = store.degree_histogram(bins=800)
    t_first = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(reps):
        again = store.degree_histogram(bins=800)
    t_cached = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    want = np.zeros(800, np.int64)
    for g in raw:
        ei = oc.augment_edge(g["edge_index"], g["node_is_attributed"])[0]
        want += np.bincount(np.bincount(ei[1], minlength=g["x"].shape[0]), minlength=800)
    t_numpy = time.perf_counter() - t0
    assert np.array_equal(first.numpy(), want) and np.array_equal(again.numpy(), want)
    return dict(row="degree_histogram", workload="code2", graphs=G, nodes=int(store.nodes.sum()), edges=int(store.out_edges.sum()),
                bins=800, first_call_ms=round(1e3 * t_first, 3), cached_call_ms=round(1e3 * t_cached, 3),
                numpy_ms=round(1e3 * t_numpy, 3), max_degree=int(np.nonzero(want)[0].max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--store", type=int, default=2048, help="graphs in each store (er: a quarter of it, 512 KiB of x per graph)")
    ap.add_argument("--rows", default="nci1,er,code2,molpcba")
    ap.add_argument("--hist-graphs", type=int, default=4096)
    ap.add_argument("--no-hist", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="")
    opt = ap.parse_args()
    sys.path.insert(0, os.path.abspath(opt.root))
    from graphtrans_amd import _lib, synth
    from graphtrans_amd.data import GraphStore
    assert torch.cuda.is_available(), "collate_bench needs a GPU"
    version = _lib.lib().gt_version()
    want = opt.rows.split(",")
    for workload, B in ROWS:
        if workload not in want:
            continue
        G = max(opt.store // 4, B) if workload == "er" else opt.store
        store = GraphStore(raw_graphs(synth, workload, G))
        r = time_collate(_lib, store, B, opt.calls, opt.warmup)
        print(json.dumps(dict(row=f"{workload} b{B}", tag=opt.tag, gt_version=version, store_graphs=G,
                              store_mb=round(store.nbytes() / 1e6, 1), calls=opt.calls, **r)), flush=True)
        del store
        torch.cuda.empty_cache()
    if not opt.no_hist:
        print(json.dumps(dict(tag=opt.tag, **time_histogram(synth, GraphStore, opt.hist_graphs, 20))), flush=True)


if __name__ == "__main__":
    main()
