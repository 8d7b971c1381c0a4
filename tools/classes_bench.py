#!/usr/bin/env python3
"""Measurement tool: the reachability classes (pg_reach_classes) against the route to the same answer
that exists without it, on two matrices of 4096 x 4096 end points x 8 services:
  cluster   the config-5 cluster engine's pg_reach_matrix (as tools/groups_bench.py): few classes
  random    uniform random codes of the same shape: every end point its own class

Legs, timed with stream events after warm-up, alternating inside every repetition, best and median:
  classes           pg_reach_classes, the two class arrays only
  classes_quotient  pg_reach_classes with the representatives and the quotient
  torch_dev         the route without the feature, torch on the device over the same buffer: unpack the
                    cells to uint8 by shifts, torch.unique(dim=0, return_inverse=True) on the rows
                    [n_src, n_svc * n_dst] and on the transposed columns [n_dst, n_svc * n_src]
  copy              a plain device copy of the input bytes, as the scale
The call's class arrays are compared with the torch route's, renumbered to first appearance, and its
quotient with the cells torch gathers at the representatives, on the whole matrix before any timing.
Prints one JSON line (and writes it to --out): milliseconds of every leg and each leg's ratio to
torch_dev, per matrix.

  python tools/classes_bench.py [--side 4096] [--services 8] [--reps 9] [--matrix both|cluster|random]
                                [--out profiles/classes_bench.json]
The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/classes_bench.py --reps 3
whose kernel_stats.csv is kept as profiles/classes_bench_kernel_stats.csv (and, with --matrix cluster /
random, as profiles/classes_bench_kernel_stats_cluster.csv / _random.csv).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vpp_amd import device as D, workloads as W  # noqa: E402


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def unpack_cells(mt, n_dst):
    """packed int32 [n_svc, n_src, row_words] -> the ConnActions, uint8 [n_svc, n_src, n_dst]"""
    sh = torch.arange(0, 32, 2, dtype=torch.int32, device=mt.device)
    return ((mt.reshape(mt.shape[0], mt.shape[1], -1, 1) >> sh) & 3).to(torch.uint8).reshape(mt.shape[0], mt.shape[1], -1)[:, :, :n_dst]


def torch_route(mt, n_dst):
    """-> (cells, src inverse, dst inverse): torch.unique's ids, in its own (sorted) numbering"""
    cells = unpack_cells(mt, n_dst)
    n_svc, n_src, _ = cells.shape
    _, si = torch.unique(cells.permute(1, 0, 2).reshape(n_src, -1), dim=0, return_inverse=True)
    _, di = torch.unique(cells.permute(2, 0, 1).reshape(n_dst, -1), dim=0, return_inverse=True)
    return cells, si, di


def first_appearance(inverse):
    """torch.unique's inverse -> (ids numbered by first appearance, the least member of every id)"""
    n, k = inverse.numel(), int(inverse.max()) + 1
    first = torch.full((k,), n, dtype=torch.int64, device=inverse.device)
    first.scatter_reduce_(0, inverse, torch.arange(n, device=inverse.device), "amin")
    order = torch.argsort(first)
    new = torch.empty_like(order)
    new[order] = torch.arange(k, device=inverse.device)
    return new[inverse].to(torch.int32), first[order]


def measure(e, mt, n, reps, warmup):
    n_svc = mt.shape[0]
    sc, dc, sr, dr, q, res = D.reach_classes(e, mt, n_svc, n, n, reps=True, quotient=True)
    cells, si, di = torch_route(mt, n)
    (ws, wsr), (wd, wdr) = first_appearance(si), first_appearance(di)
    assert torch.equal(sc, ws) and torch.equal(dc, wd), "the classes differ from the torch route's"
    assert torch.equal(sr.to(torch.int64), wsr) and torch.equal(dr.to(torch.int64), wdr), "the representatives differ"
    want_q = cells[:, wsr][:, :, wdr]
    assert torch.equal(unpack_cells(q, len(wdr)), want_q), "the quotient differs from the cells at the representatives"
    del cells, si, di, want_q
    dst = torch.empty_like(mt)
    legs = {
        "classes": lambda: D.reach_classes(e, mt, n_svc, n, n),
        "classes_quotient": lambda: D.reach_classes(e, mt, n_svc, n, n, reps=True, quotient=True),
        "torch_dev": lambda: torch_route(mt, n),
        "copy": lambda: dst.copy_(mt),
    }
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    t = {name: [] for name in legs}
    for _ in range(reps):  # alternating
        for name, fn in legs.items():
            t[name].append(event_ms(fn)[0])
    best = {name: min(v) for name, v in t.items()}
    med = {name: statistics.median(v) for name, v in t.items()}
    return {"result": res, "ms_best": best, "ms_median": med,
            "over_torch_dev": {k: best["torch_dev"] / v for k, v in best.items()},
            "over_torch_dev_median": {k: med["torch_dev"] / v for k, v in med.items()},
            "over_copy": {k: best[k] / best["copy"] for k in ("classes", "classes_quotient")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--services", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--matrix", choices=("both", "cluster", "random"), default="both")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "classes_bench needs the GPU"

    e, _r, _local, pool = W.cluster_engine(0)
    g = np.random.default_rng(5)
    ips = pool[g.integers(0, len(pool), a.side)].copy()   # the cluster's pods and Internet hosts, a tenth
    m = g.random(a.side) < 0.1                            # uniform addresses (as tools/groups_bench.py)
    ips[m] = g.integers(0, 1 << 32, int(m.sum()), dtype=np.uint64).astype(np.uint32)
    ports = W.CLUSTER_PORTS
    svc = [(0 if i % 4 != 3 else 1, 40000 + i, ports[i % len(ports)]) for i in range(a.services)]
    cluster = D.reach_matrix(e, ips, ips, svc)
    codes = g.integers(0, 4, (a.services, a.side, a.side), dtype=np.uint8)
    rw = D.reach_row_words(a.side)
    padded = np.zeros((a.services, a.side, 16 * rw), np.uint32)
    padded[:, :, :a.side] = codes
    words = (padded.reshape(a.services, a.side, rw, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=3, dtype=np.uint32)
    random = torch.from_numpy(words.view(np.int32)).cuda()
    torch.cuda.synchronize()
    res = {"tool": "classes_bench", "engine": "config-5 cluster (workloads.cluster_engine)", "reps": a.reps, "side": a.side,
           "n_svc": a.services, "input_bytes": cluster.numel() * 4, "plan": e.debug_reach_classes_plan(a.side),
           "matrices": {name: measure(e, mt, a.side, a.reps, a.warmup) for name, mt in (("cluster", cluster), ("random", random))
                        if a.matrix in ("both", name)}}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
