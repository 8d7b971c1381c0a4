#!/usr/bin/env python3
"""Measurement tool: the reachability dominators (pg_reach_dominators) against the route to the same
answer that exists without it, on two matrices of 4096 end points, each from one entry and from 16:
  cluster  the config-5 cluster engine's pg_reach_matrix (as tools/closure_bench.py), all services
  built    the closure bench's random graph (2 edges per node on average, one slice)
The single entry is the end point with the most out-edges; the 16 are drawn at random.

Legs, timed with stream events after warm-up, alternating inside every repetition, best and median:
  result      pg_reach_dominators, the result alone
  all         pg_reach_dominators with out_dom, out_idom and out_cut
  torch_half  the route without the feature, torch on the device over the same buffer: unpack the cells to
              bool, OR the slices, then the same synchronous iteration Avoid' = Avoid | ((ET (x) Avoid) minus
              the diagonal) over n + 1 columns as fp16 matrix products of 0 / 1 operands, until nothing
              changes; Dom, the sizes, idom by the size rule, the cuts, Dom packed again
  torch_fp32  the same with fp32 products
  copy        a plain device copy of the input bytes, as the scale
Every output of the call is compared with both torch routes' before any timing. Prints one JSON line (and
writes it to --out): milliseconds of every leg, each leg's ratio to torch_half, and the milliseconds per
round of the two legs of the call.

  python tools/dominators_bench.py [--side 4096] [--services 8] [--reps 9] [--out profiles/dominators_bench.json]
The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/dominators_bench.py --reps 3
whose kernel_stats.csv is kept as profiles/dominators_bench_kernel_stats.csv.
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
NONE, NO_IDOM = 0xFFFFFFFF, 0xFFFF


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


def random_graph(n, per_node, seed):
    """packed words [1, n, row_words(n)] of a random graph (tools/closure_bench.py's): ALLOW on the edges,
    DENY_SYN elsewhere"""
    g = np.random.default_rng(seed)
    rw = D.reach_row_words(n)
    codes = np.zeros((n, 16 * rw), np.uint32)
    codes[:, :n] = (g.random((n, n)) < per_node / n) * 2
    words = (codes.reshape(n, rw, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=2, dtype=np.uint32)
    return torch.from_numpy(words.view(np.int32)[None].copy()).cuda()


def torch_route(mt, n, entry, dt):
    """-> (dom words int32 [n, row_words], idom int64 [n], cut int64 [n], result dict)"""
    a = unpack_allow(mt.reshape(-1, mt.shape[-1]), n).reshape(-1, n, n).any(dim=0)
    dev = mt.device
    ent = torch.tensor(sorted(set(entry)), dtype=torch.int64, device=dev)
    avoid = torch.zeros((n, n + 1), dtype=torch.bool, device=dev)
    start = torch.zeros(n, dtype=torch.bool, device=dev)
    avoid[ent] = True
    avoid[ent, ent] = False
    start[ent] = True
    et = a.T.to(dt).contiguous()
    v = torch.arange(n, device=dev)
    rounds = 0
    while True:
        p = (et @ avoid.to(dt)) > 0
        p[v, v] = False
        new = avoid | p
        if torch.equal(new, avoid):
            break
        avoid, rounds = new, rounds + 1
    reached = avoid[:, n]
    dom = ~avoid[:, :n] & reached[:, None]
    size = dom.sum(dim=1)
    cut = dom.sum(dim=0) - dom.diagonal().to(torch.int64)
    strict = dom.clone()
    strict[v, v] = False
    hit = strict & (size[None, :] == size[:, None] - 1)
    idom = torch.where(hit.any(dim=1), hit.to(torch.uint8).argmax(dim=1), torch.full_like(size, NO_IDOM))
    choke = (cut > 0) & ~start
    best = int(cut[choke].max()) if bool(choke.any()) else 0
    top = int(torch.nonzero(choke & (cut == best))[0]) if best else NONE
    res = {"n_reached": int(reached.sum()), "n_chokes": int(choke.sum()), "top": top, "top_cut": best,
           "depth": int(size.max()) - 1 if bool(reached.any()) else 0, "rounds": rounds}
    return pack_allow(dom), idom, cut, res


def measure(e, mt, n, entry, reps, warmup):
    n_svc = mt.shape[0]
    call = lambda **kw: D.reach_dominators(e, mt, n, n_svc, entry, **kw)
    dom, idom, cut, res = call(dom=True, idom=True, cut=True)
    assert call()[3] == res, "the result alone differs"
    for dt in (torch.float16, torch.float32):
        wd, wi, wc, wres = torch_route(mt, n, entry, dt)
        assert res == wres, ("the result differs from the torch route's", res, wres)
        assert torch.equal(dom, wd), "out_dom differs"
        assert torch.equal(idom.to(torch.int64) & 0xFFFF, wi) and torch.equal(cut.to(torch.int64), wc), "out_idom or out_cut differs"
        del wd, wi, wc
    dst = torch.empty_like(mt)
    legs = {
        "result": lambda: call(),
        "all": lambda: call(dom=True, idom=True, cut=True),
        "torch_half": lambda: torch_route(mt, n, entry, torch.float16),
        "torch_fp32": lambda: torch_route(mt, n, entry, torch.float32),
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
    return {"n_entry": len(entry), "result": res, "ms_best": best, "ms_median": med,
            "over_torch_half": {k: best["torch_half"] / v for k, v in best.items()},
            "over_torch_half_median": {k: med["torch_half"] / v for k, v in med.items()},
            "ms_per_round": {k: best[k] / max(1, res["rounds"]) for k in ("result", "all", "torch_half", "torch_fp32")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--services", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dominators_bench needs the GPU"

    e, _r, _local, pool = W.cluster_engine(0)
    g = np.random.default_rng(5)
    ips = pool[g.integers(0, len(pool), a.side)].copy()   # the cluster's pods and Internet hosts, a tenth
    m = g.random(a.side) < 0.1                            # uniform addresses (as tools/closure_bench.py)
    ips[m] = g.integers(0, 1 << 32, int(m.sum()), dtype=np.uint64).astype(np.uint32)
    ports = W.CLUSTER_PORTS
    svc = [(0 if i % 4 != 3 else 1, 40000 + i, ports[i % len(ports)]) for i in range(a.services)]
    cluster = D.reach_matrix(e, ips, ips, svc)
    built = random_graph(a.side, 2.0, 6)
    torch.cuda.synchronize()
    busiest = lambda mt: [int(unpack_allow(mt.reshape(-1, mt.shape[-1]), a.side).reshape(-1, a.side, a.side).any(dim=0).sum(dim=1).argmax())]
    many = [int(x) for x in g.integers(0, a.side, 16)]
    runs = {"cluster_1": (cluster, busiest(cluster)), "cluster_16": (cluster, many),
            "built_1": (built, busiest(built)), "built_16": (built, many)}
    res = {"tool": "dominators_bench", "engine": "config-5 cluster (workloads.cluster_engine)", "reps": a.reps, "side": a.side,
           "n_svc": a.services, "plan": e.debug_reach_dominators_plan(a.side),
           "runs": {name: dict(measure(e, mt, a.side, entry, a.reps, a.warmup), input_bytes=mt.numel() * 4)
                    for name, (mt, entry) in runs.items()}}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
