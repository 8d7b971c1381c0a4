#!/usr/bin/env python3
"""Measurement tool: the reachability paths (pg_reach_paths) against the route to the same answer that
exists without it, on two hops matrices of 4096 end points:
  cluster    the closure of the config-5 cluster engine's pg_reach_matrix over 4096 end points x 8 services
  synthetic  the closure of a random graph of 4096 nodes with 2 edges per node on average (tools/
             closure_bench.py's), some tens of levels deep
and three query sets:
  sources    all targets from 64 sources, with the nodes
  random     2^20 random pairs, with the nodes
  all_pairs  every pair: the choke-point call, out_via only

Legs, timed with stream events after warm-up, alternating inside every repetition, best and median:
  paths      pg_reach_paths (the host's sort of the queries and their copy included)
  torch_dev  the route without it, torch on the device over the same buffer: hopsT once per call, then for
             a block of queries and each step ((hops[src] == t - 1) & (hopsT[cur] == 1)).int().argmax(1),
             the block sized so that the boolean block stays near 64 MiB
  copy       a plain device copy of the hops matrix, what k_paths_edges_t reads once, as a scale
The whole output of the call is compared with the torch route's before any timing. Prints one JSON line
(and writes it to --out): milliseconds of every leg and each leg's ratio to torch_dev.

  python tools/paths_bench.py [--side 4096] [--services 8] [--reps 9] [--out profiles/paths_bench.json]
The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/paths_bench.py --reps 3 --no-torch
whose kernel_stats.csv is kept as profiles/paths_bench_kernel_stats.csv.
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from closure_bench import event_ms, random_graph  # noqa: E402

BOOL_BLOCK = 64 << 20


def torch_paths(hops, n, src, dst, max_len, nodes, via):
    """the parent route on the device -> (lengths int16 [Q], nodes int16 [Q, max_len + 1] or None, via int32
    [n] or None). hops: int16 [n, n]; src, dst: int64 device tensors."""
    ht = hops.t().contiguous()
    q_all = src.numel()
    lens = torch.empty(q_all, dtype=torch.int16, device=hops.device)
    rows = torch.full((q_all, max_len + 1), -1, dtype=torch.int16, device=hops.device) if nodes else None
    cnt = torch.zeros(n, dtype=torch.int64, device=hops.device) if via else None
    block = max(1, BOOL_BLOCK // n)
    for b in range(0, q_all, block):
        s, cur = src[b:b + block], dst[b:b + block].clone()
        d = hops[s, cur].to(torch.int64)
        lens[b:b + block] = d.to(torch.int16)
        if nodes:
            fits = (d > 0) & (d <= max_len)
            at = torch.nonzero(fits).squeeze(1)
            rows[b + at, 0] = s[at].to(torch.int16)
            rows[b + at, d[at]] = cur[at].to(torch.int16)
        for t in range(int(d.max()) if d.numel() else 0, 1, -1):
            act = torch.nonzero(d >= t).squeeze(1)
            k = ((hops[s[act]] == t - 1) & (ht[cur[act]] == 1)).int().argmax(1)
            cur[act] = k
            if via:
                cnt += torch.bincount(k, minlength=n)
            if nodes:
                w = act[d[act] <= max_len]
                rows[b + w, t - 1] = cur[w].to(torch.int16)
    return lens, rows, cnt.to(torch.int32) if via else None


def query_sets(n, seed):
    g = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.uint32)
    sources = np.sort(g.choice(n, 64, replace=False)).astype(np.uint32)
    return {"sources": (np.repeat(sources, n), np.tile(i, 64), True, False),
            "random": (g.integers(0, n, 1 << 20).astype(np.uint32), g.integers(0, n, 1 << 20).astype(np.uint32), True, False),
            "all_pairs": (np.repeat(i, n), np.tile(i, n), False, True)}


def measure(e, hops, n, reps, warmup, with_torch):
    """hops: int16 [n, n] on the device -> the result dict of one matrix"""
    levels = int(hops.max())
    out = {"n": n, "levels": levels, "hops_bytes": hops.numel() * 2}
    scratch = torch.empty_like(hops)
    for name, (src, dst, nodes, via) in query_sets(n, 7).items():
        st, dt = torch.from_numpy(src.astype(np.int64)).cuda(), torch.from_numpy(dst.astype(np.int64)).cuda()
        call = lambda: D.reach_paths(e, hops, n, src, dst, max_len=max(1, levels), nodes=nodes, via=via)
        route = lambda: torch_paths(hops, n, st, dt, max(1, levels), nodes, via)
        lens, rows, cnt, res = call()
        if with_torch:
            wl, wr, wc = route()
            assert torch.equal(lens, wl), "the lengths differ from the torch route's"
            assert not nodes or torch.equal(rows, wr), "the nodes differ from the torch route's"
            assert not via or torch.equal(cnt, wc), "the choke-point counts differ from the torch route's"
            del wl, wr, wc
        del lens, rows, cnt
        legs = {"paths": call, "copy": lambda: scratch.copy_(hops)}
        if with_torch:
            legs["torch_dev"] = route
        for _ in range(warmup):
            for fn in legs.values():
                fn()
        t = {leg: [] for leg in legs}
        for _ in range(reps):  # alternating
            for leg, fn in legs.items():
                t[leg].append(event_ms(fn)[0])
        best = {leg: min(v) for leg, v in t.items()}
        med = {leg: statistics.median(v) for leg, v in t.items()}
        out[name] = {"n_queries": int(src.size), "nodes": nodes, "via": via, **res, "ms_best": best, "ms_median": med}
        if with_torch:
            out[name]["over_torch_dev"] = {k: best["torch_dev"] / v for k, v in best.items()}
            out[name]["over_torch_dev_median"] = {k: med["torch_dev"] / v for k, v in med.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--services", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="the call and the copy alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "paths_bench needs the GPU"

    e, _r, _local, pool = W.cluster_engine(0)
    g = np.random.default_rng(5)
    ips = pool[g.integers(0, len(pool), a.side)].copy()   # the end points of tools/closure_bench.py
    m = g.random(a.side) < 0.1
    ips[m] = g.integers(0, 1 << 32, int(m.sum()), dtype=np.uint64).astype(np.uint32)
    ports = W.CLUSTER_PORTS
    svc = [(0 if i % 4 != 3 else 1, 40000 + i, ports[i % len(ports)]) for i in range(a.services)]
    res = {"tool": "paths_bench", "engine": "config-5 cluster (workloads.cluster_engine)", "reps": a.reps,
           "plan": e.debug_reach_paths_plan(a.side)}
    for name, mt in (("cluster", D.reach_matrix(e, ips, ips, svc)), ("synthetic", random_graph(a.side, 2.0, 6))):
        hops = D.reach_closure(e, mt, a.side, hops=True)[1]
        torch.cuda.synchronize()
        del mt
        res[name] = measure(e, hops, a.side, a.reps, a.warmup, not a.no_torch)
        print(name, json.dumps(res[name]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
