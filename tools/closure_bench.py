#!/usr/bin/env python3
"""Measurement tool: the reachability closure (pg_reach_closure) against the route to the same answer
that exists without it, on two inputs of 4096 end points:
  cluster    the config-5 cluster engine's pg_reach_matrix over 4096 end points (the same list on both
             sides) x 8 services
  synthetic  a random graph of 4096 nodes with 2 edges per node on average, one slice (the cluster's
             policy graph may be as shallow as the test fixtures'; this one is some ten levels deep)

Legs, timed with stream events after warm-up, alternating inside every repetition, best and median:
  closure        pg_reach_closure, out_packed only
  closure_hops   pg_reach_closure with out_hops
  closure_count  pg_reach_closure with out_count
  torch_dev      the route without the closure, torch on the device over the same buffer: unpack the
                 ALLOW cells of the slices to fp16, level by level ((F @ A) > 0) & ~R until nothing is
                 new, pack R into the audits' layout
  copy           a plain device copy that moves the bytes one level reads and writes (A, F and R read,
                 R and F' written: five bit matrices), as a scale
The closure's output is compared with the torch route's on the whole matrix first, and so are the two
routes' levels. Prints one JSON line (and writes it to --out): the levels of every input, milliseconds
of every leg and each leg's ratio to torch_dev.

  python tools/closure_bench.py [--side 4096] [--services 8] [--reps 9] [--out profiles/closure_bench.json]
The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/closure_bench.py --reps 3
whose kernel_stats.csv is kept as profiles/closure_bench_kernel_stats.csv.
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


def torch_closure(mt, n):
    """the parent route on the device -> (packed int32 [n, row_words], levels)"""
    sh = torch.arange(0, 32, 2, dtype=torch.int32, device=mt.device)
    cells = ((mt.reshape(mt.shape[0], n, -1, 1) >> sh) & 3).reshape(mt.shape[0], n, -1)[:, :, :n]
    a = (cells == 2).any(dim=0)
    af = a.to(torch.float16)
    reach, front, levels = a.clone(), a, int(a.any())
    while levels:
        front = ((front.to(torch.float16) @ af) > 0) & ~reach   # (a positive sum never rounds to zero)
        if not bool(front.any()):
            break
        levels += 1
        reach |= front
    rw = D.reach_row_words(n)
    codes = torch.zeros((n, 16 * rw), dtype=torch.int32, device=mt.device)
    codes[:, :n] = reach.to(torch.int32) * 2
    return (codes.reshape(n, rw, 16) << sh).sum(dim=2, dtype=torch.int32), levels


def measure(e, mt, n, reps, warmup):
    """mt: int32 [n_svc, n, row_words(n)] -> the result dict of one input"""
    packed, hops, counts, res = D.reach_closure(e, mt, n, hops=True, counts=True)
    want, levels = torch_closure(mt, n)
    assert torch.equal(packed, want), "the closure differs from the torch route's"
    assert res["levels"] == levels, (res, levels)
    reach = D.unpack_closure(packed, n)
    assert (counts.cpu().numpy() == reach.sum(axis=1)).all() and ((hops.cpu().numpy() > 0) == reach).all()
    assert int(hops.max()) == levels and res["n_reachable"] == int(reach.sum())
    del want, hops, counts, reach
    level_bytes = 5 * n * ((n + 31) // 32) * 4
    buf = torch.empty(level_bytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(buf)
    legs = {
        "closure": lambda: D.reach_closure(e, mt, n),
        "closure_hops": lambda: D.reach_closure(e, mt, n, hops=True),
        "closure_count": lambda: D.reach_closure(e, mt, n, counts=True),
        "torch_dev": lambda: torch_closure(mt, n),
        "copy": lambda: dst.copy_(buf),
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
    return {"n": n, "n_svc": int(mt.shape[0]), "input_bytes": mt.numel() * 4, "level_bytes": level_bytes, **res,
            "ms_best": best, "ms_median": med, "over_torch_dev": {k: best["torch_dev"] / v for k, v in best.items()},
            "over_torch_dev_median": {k: med["torch_dev"] / v for k, v in med.items()}}


def random_graph(n, per_node, seed):
    """packed words [1, n, row_words(n)] of a random graph: ALLOW on the edges, DENY_SYN elsewhere"""
    g = np.random.default_rng(seed)
    rw = D.reach_row_words(n)
    codes = np.zeros((n, 16 * rw), np.uint32)
    codes[:, :n] = (g.random((n, n)) < per_node / n) * 2
    words = (codes.reshape(n, rw, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=2, dtype=np.uint32)
    return torch.from_numpy(words.view(np.int32)[None].copy()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--services", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "closure_bench needs the GPU"

    e, _r, _local, pool = W.cluster_engine(0)
    g = np.random.default_rng(5)
    ips = pool[g.integers(0, len(pool), a.side)].copy()   # the cluster's pods and Internet hosts, a tenth
    m = g.random(a.side) < 0.1                            # uniform addresses (as tools/reach_bench.py)
    ips[m] = g.integers(0, 1 << 32, int(m.sum()), dtype=np.uint64).astype(np.uint32)
    ports = W.CLUSTER_PORTS
    svc = [(0 if i % 4 != 3 else 1, 40000 + i, ports[i % len(ports)]) for i in range(a.services)]
    mt = D.reach_matrix(e, ips, ips, svc)
    torch.cuda.synchronize()
    cluster = measure(e, mt, a.side, a.reps, a.warmup)
    synthetic = measure(e, random_graph(a.side, 2.0, 6), a.side, a.reps, a.warmup)

    res = {"tool": "closure_bench", "engine": "config-5 cluster (workloads.cluster_engine)", "reps": a.reps,
           "plan": e.debug_reach_closure_plan(a.side), "cluster": cluster, "synthetic": synthetic}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
