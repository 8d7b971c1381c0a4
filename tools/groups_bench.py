#!/usr/bin/env python3
"""Measurement tool: the reachability groups (pg_reach_groups) against the route to the same answer
that exists without it, on the config-5 cluster engine's pg_reach_matrix over 4096 x 4096 end points x
8 services, under four groupings (the same on both sides unless said):
  blocks    64 contiguous blocks of 64
  random    64 groups assigned at random
  one       one group on each side: the worst case for the final atomics
  identity  every src its own group against the 64 dst blocks: the worst case for the flush, with
            one-row chunks

Legs, timed with stream events after warm-up, alternating inside every repetition, best and median:
  groups           pg_reach_groups, out_counts only
  groups_packed    pg_reach_groups with out_packed
  torch_matmul     the route without the feature, torch on the device over the same buffer: unpack the
                   cells by shifts, and per ConnAction multiply the cell mask by the dst one-hot matrix,
                   then the src one-hot matrix by that, in fp32 (sums of ones up to 2^24 = 4096 x 4096
                   are exact)
  torch_index_add  the same with two index_add_ in int32 instead of the two products
  copy             a plain device copy of the input bytes, as the scale
torch_dev is the faster of the two torch legs, and the result says which. The call's counts are compared
with both torch routes' on the whole matrix before any timing. Prints one JSON line (and writes it to
--out): milliseconds of every leg and each leg's ratio to torch_dev, per grouping.

  python tools/groups_bench.py [--side 4096] [--services 8] [--reps 9] [--out profiles/groups_bench.json]
The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/groups_bench.py --reps 3
whose kernel_stats.csv is kept as profiles/groups_bench_kernel_stats.csv.
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
    """packed int32 [n_svc, n_src, row_words] -> the ConnActions, int32 [n_svc, n_src, n_dst]"""
    sh = torch.arange(0, 32, 2, dtype=torch.int32, device=mt.device)
    return ((mt.reshape(mt.shape[0], mt.shape[1], -1, 1) >> sh) & 3).reshape(mt.shape[0], mt.shape[1], -1)[:, :, :n_dst]


def torch_matmul(mt, n_dst, s1h, d1h):
    """s1h fp32 [n_sg, n_src], d1h fp32 [n_dst, n_dg] -> counts int64 [n_svc, n_sg, n_dg, 4]"""
    cells = unpack_cells(mt, n_dst)
    return torch.stack([(s1h @ ((cells == c).to(torch.float32) @ d1h)) for c in range(4)], dim=-1).to(torch.int64)


def torch_index_add(mt, n_dst, sg, dg, n_sg, n_dg):
    """sg, dg int64 device -> counts int64 [n_svc, n_sg, n_dg, 4]"""
    cells = unpack_cells(mt, n_dst)
    out = []
    for c in range(4):
        by_src = torch.zeros((mt.shape[0], n_sg, n_dst), dtype=torch.int32, device=mt.device)
        by_src.index_add_(1, sg, (cells == c).to(torch.int32))
        both = torch.zeros((mt.shape[0], n_sg, n_dg), dtype=torch.int32, device=mt.device)
        out.append(both.index_add_(2, dg, by_src))
    return torch.stack(out, dim=-1).to(torch.int64)


def groupings(n, seed):
    """name -> (src ids, n_sg, dst ids, n_dg)"""
    g = np.random.default_rng(seed)
    blocks = (np.arange(n) * 64 // n).astype(np.uint32)
    rs, rd = (g.integers(0, 64, n).astype(np.uint32) for _ in range(2))
    one = np.zeros(n, np.uint32)
    return {"blocks": (blocks, 64, blocks, 64), "random": (rs, 64, rd, 64), "one": (one, 1, one, 1),
            "identity": (np.arange(n, dtype=np.uint32), n, blocks, 64)}


def measure(e, mt, n, grouping, reps, warmup):
    sg, n_sg, dg, n_dg = grouping
    sgt, dgt = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (sg, dg))
    s1h = torch.zeros((n_sg, n), dtype=torch.float32, device="cuda")
    s1h[sgt, torch.arange(n, device="cuda")] = 1
    d1h = torch.zeros((n, n_dg), dtype=torch.float32, device="cuda")
    d1h[torch.arange(n, device="cuda"), dgt] = 1
    counts, packed = D.reach_groups(e, mt, n, n, sg, dg, n_sg, n_dg, packed=True)
    for want in (torch_matmul(mt, n, s1h, d1h), torch_index_add(mt, n, sgt, dgt, n_sg, n_dg)):
        assert torch.equal(counts, want), "the counts differ from the torch route's"
    assert int(counts.sum()) == mt.shape[0] * n * n
    status = np.bincount(D.unpack_groups(packed, n_dg).ravel(), minlength=4).tolist()
    del want
    dst = torch.empty_like(mt)
    legs = {
        "groups": lambda: D.reach_groups(e, mt, n, n, sg, dg, n_sg, n_dg),
        "groups_packed": lambda: D.reach_groups(e, mt, n, n, sg, dg, n_sg, n_dg, packed=True),
        "torch_matmul": lambda: torch_matmul(mt, n, s1h, d1h),
        "torch_index_add": lambda: torch_index_add(mt, n, sgt, dgt, n_sg, n_dg),
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
    route = min(("torch_matmul", "torch_index_add"), key=lambda k: best[k])
    best["torch_dev"], med["torch_dev"] = best[route], med[route]
    return {"n_src_groups": n_sg, "n_dst_groups": n_dg, "status_pairs": status, "torch_dev_route": route,
            "ms_best": best, "ms_median": med, "over_torch_dev": {k: best["torch_dev"] / v for k, v in best.items()},
            "over_torch_dev_median": {k: med["torch_dev"] / v for k, v in med.items()},
            "over_copy": {k: best[k] / best["copy"] for k in ("groups", "groups_packed")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--services", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "groups_bench needs the GPU"

    e, _r, _local, pool = W.cluster_engine(0)
    g = np.random.default_rng(5)
    ips = pool[g.integers(0, len(pool), a.side)].copy()   # the cluster's pods and Internet hosts, a tenth
    m = g.random(a.side) < 0.1                            # uniform addresses (as tools/reach_bench.py)
    ips[m] = g.integers(0, 1 << 32, int(m.sum()), dtype=np.uint64).astype(np.uint32)
    ports = W.CLUSTER_PORTS
    svc = [(0 if i % 4 != 3 else 1, 40000 + i, ports[i % len(ports)]) for i in range(a.services)]
    mt = D.reach_matrix(e, ips, ips, svc)
    torch.cuda.synchronize()
    res = {"tool": "groups_bench", "engine": "config-5 cluster (workloads.cluster_engine)", "reps": a.reps, "side": a.side,
           "n_svc": a.services, "input_bytes": mt.numel() * 4, "plan": e.debug_reach_groups_plan(a.side),
           "groupings": {name: measure(e, mt, a.side, grp, a.reps, a.warmup) for name, grp in groupings(a.side, 7).items()}}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
