#!/usr/bin/env python3
"""Measurement tool: the reachability zones (pg_reach_zones) against the route to the same answer that
exists without it, on two closures of 4096 end points:
  cluster   the config-5 cluster engine's pg_reach_matrix (as tools/classes_bench.py) closed by
            pg_reach_closure on the device: few zones
  rings     built on the host: a few hundred rings of mixed sizes (1 .. 32) joined by random forward
            links, the closure in closed form, the end points permuted: many zones

Legs, timed with stream events after warm-up, alternating inside every repetition, best and median:
  zones      pg_reach_zones, out_zone only
  zones_all  pg_reach_zones with every output
  torch_dev  the route without the feature, torch on the device over the same buffer: unpack the cells to
             bool, R & R.T, the first set column of every row (min with the row), torch.unique, the sizes,
             the popcounts, R[rep][:, rep] gathered and packed again
  copy       a plain device copy of the input bytes, as the scale
Every output of the call is compared with the torch route's on the whole matrix before any timing.
Prints one JSON line (and writes it to --out): milliseconds of every leg and each leg's ratio to
torch_dev, per closure.

  python tools/zones_bench.py [--side 4096] [--services 8] [--reps 9] [--matrix both|cluster|rings]
                              [--out profiles/zones_bench.json]
The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/zones_bench.py --reps 3
whose kernel_stats.csv is kept as profiles/zones_bench_kernel_stats.csv.
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

ALLOW = 2


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def unpack_allow(mt, n):
    """packed int32 [rows, row_words] -> bool [rows, n]: the cells that hold ALLOW"""
    sh = torch.arange(0, 32, 2, dtype=torch.int32, device=mt.device)
    return (((mt.reshape(mt.shape[0], -1, 1) >> sh) & 3) == ALLOW).reshape(mt.shape[0], -1)[:, :n]


def pack_allow(r):
    """bool [rows, cols] -> packed int32 [rows, row_words(cols)]: ALLOW where set, padding zero"""
    rows, cols = r.shape
    rw = (cols + 15) // 16
    cells = torch.zeros((rows, 16 * rw), dtype=torch.int32, device=r.device)
    cells[:, :cols] = r.to(torch.int32) * ALLOW
    sh = torch.arange(0, 32, 2, dtype=torch.int32, device=r.device)
    return (cells.reshape(rows, rw, 16) << sh).sum(dim=2, dtype=torch.int32)


def torch_route(mt, n):
    """-> (zone, rep, size, reaches, reached_by, dag words)"""
    r = unpack_allow(mt, n)
    m = r & r.T
    idx = torch.arange(n, device=mt.device)
    first = torch.where(m.any(dim=1), m.to(torch.uint8).argmax(dim=1), n)
    label = torch.minimum(first, idx)
    rep, zone = torch.unique(label, return_inverse=True)   # (sorted: the ids ascend with the representatives)
    size = torch.bincount(zone, minlength=rep.numel())
    rr = r[rep]
    return zone, rep, size, rr.sum(dim=1), r[:, rep].sum(dim=0), pack_allow(rr[:, rep])


def rings_closure(n, g):
    """the packed closure of the `rings` graph over n end points, as uint32 words [n, row_words(n)]"""
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(g.integers(1, 33)), n - sum(sizes)))
    k = len(sizes)
    part = np.repeat(np.arange(k), sizes)
    link = np.triu(g.random((k, k)) < 2.0 / k, 1)
    reach = link.copy()
    while True:   # the closure of the forward links over the k rings
        more = reach | ((reach.astype(np.float32) @ reach.astype(np.float32)) > 0)
        if (more == reach).all():
            break
        reach = more
    reach[np.arange(k), np.arange(k)] = True   # a ring reaches itself (size 1: a self-loop)
    at = part[g.permutation(n)]
    r = reach[at][:, at]
    rw = (n + 15) // 16
    cells = np.zeros((n, 16 * rw), np.uint32)
    cells[:, :n] = np.where(r, ALLOW, g.choice(np.array([0, 1, 3], np.uint32), (n, n)))
    return (cells.reshape(n, rw, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=2, dtype=np.uint32), k


def measure(e, mt, n, reps, warmup):
    zone, rep, size, out, by, dag, res = D.reach_zones(e, mt, n, reps=True, sizes=True, counts=True, dag=True)
    wz, wr, ws, wo, wb, wd = torch_route(mt, n)
    i64 = lambda t: t.to(torch.int64)
    assert torch.equal(i64(zone), wz) and torch.equal(i64(rep), wr), "the zones differ from the torch route's"
    assert torch.equal(i64(size), ws) and torch.equal(i64(out), wo) and torch.equal(i64(by), wb), "the counts differ"
    assert torch.equal(dag, wd), "the zone graph differs"
    assert res["n_zones"] == wr.numel() and res["largest"] == int(ws.max()) and res["n_multi"] == int((ws > 1).sum())
    del wz, wr, ws, wo, wb, wd
    dst = torch.empty_like(mt)
    legs = {
        "zones": lambda: D.reach_zones(e, mt, n),
        "zones_all": lambda: D.reach_zones(e, mt, n, reps=True, sizes=True, counts=True, dag=True),
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
            "over_copy": {k: best[k] / best["copy"] for k in ("zones", "zones_all")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--services", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--matrix", choices=("both", "cluster", "rings"), default="both")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "zones_bench needs the GPU"

    e, _r, _local, pool = W.cluster_engine(0)
    g = np.random.default_rng(5)
    ips = pool[g.integers(0, len(pool), a.side)].copy()   # the cluster's pods and Internet hosts, a tenth
    m = g.random(a.side) < 0.1                            # uniform addresses (as tools/classes_bench.py)
    ips[m] = g.integers(0, 1 << 32, int(m.sum()), dtype=np.uint64).astype(np.uint32)
    ports = W.CLUSTER_PORTS
    svc = [(0 if i % 4 != 3 else 1, 40000 + i, ports[i % len(ports)]) for i in range(a.services)]
    cluster, _, _, closed = D.reach_closure(e, D.reach_matrix(e, ips, ips, svc), a.side)
    words, n_rings = rings_closure(a.side, g)
    rings = torch.from_numpy(words.view(np.int32)).cuda()
    torch.cuda.synchronize()
    res = {"tool": "zones_bench", "engine": "config-5 cluster (workloads.cluster_engine)", "reps": a.reps, "side": a.side,
           "n_svc": a.services, "input_bytes": cluster.numel() * 4, "plan": e.debug_reach_zones_plan(a.side),
           "cluster_closure": closed, "rings": n_rings,
           "matrices": {name: measure(e, mt, a.side, a.reps, a.warmup) for name, mt in (("cluster", cluster), ("rings", rings))
                        if a.matrix in ("both", name)}}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
