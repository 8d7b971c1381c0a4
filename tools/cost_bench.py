#!/usr/bin/env python3
"""Measurement tool: the reachability cost (pg_reach_cost) against the routes to the same costs that exist
without it, at 8192 end points with 256 and 4096 sources, weights 1..9, on two graphs in one slice:
  random4  4 random edges per end point
  islands  64 islands of 128 end points with about 3 random edges per end point inside and a bridge from
           each to the next: a search runs one round per island at least

Legs, the device ones timed with stream events after warm-up, alternating inside every repetition, best and
median:
  cost     pg_reach_cost with out_cost only, the knobs at their defaults (the cost row in LDS)
  all      pg_reach_cost with out_cost, out_pred, out_len and out_via
  global   `all` with cost_lds_bytes = 0: the row in global memory under global atomics
  torch    (a) the same fixed point as masked (min,+) rounds in torch on the same device: a float matrix with
           0 on the edges and +inf elsewhere, per round min over p of (base[q, p] + mask[p, v]) + weight[v],
           sources in chunks that fit, until no cost falls. Costs only. Timed at the smaller source count
           (it takes n_src * n * n adds per round)
  scipy16  (b) scipy.sparse.csgraph.dijkstra on the CPU over a sixteenth of the sources: what one of 16
           threads would run if the sources were split evenly among them. Costs only
The costs of the call are compared with scipy's (over all sources) and with the torch route's before
anything is timed, `global` byte for byte with `all`. Prints one JSON line (and writes it to --out).

  python tools/cost_bench.py [--sources 256 4096] [--reps 5] [--out profiles/cost_bench.json]
  python tools/cost_bench.py --ab 20 --out profiles/cost_ab.jsonl    # all against global, interleaved, a line each
  python tools/cost_bench.py --chain 10 --out profiles/cost_chain.json   # a chain of 8192: the cost of a round
The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/cost_bench.py --reps 2 --no-torch
whose kernel_stats.csv is kept as profiles/cost_bench_kernel_stats.csv.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vpp_amd import device as D, renderer as R  # noqa: E402

ALLOW = 2
N = 8192


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def pack(a):
    """bool [n, n] -> packed words int32 [1, n, row_words(n)] on the device: ALLOW on the edges, DENY_SYN elsewhere"""
    n = a.shape[0]
    rw = D.reach_row_words(n)
    words = np.zeros((n, rw), np.uint32)
    sh = 2 * np.arange(16, dtype=np.uint32)
    for r0 in range(0, n, 1024):
        cells = np.zeros((min(1024, n - r0), 16 * rw), np.uint32)
        cells[:, :n] = a[r0:r0 + 1024] * ALLOW
        words[r0:r0 + 1024] = (cells.reshape(-1, rw, 16) << sh).sum(axis=2, dtype=np.uint32)
    return torch.from_numpy(words.view(np.int32)[None].copy()).cuda()


def random4(n, seed):
    g = np.random.default_rng(seed)
    a = np.zeros((n, n), bool)
    for r0 in range(0, n, 1024):
        a[r0:r0 + 1024] = g.random((min(1024, n - r0), n)) < 4.0 / n
    return a


def islands(n, seed, size=128):
    g = np.random.default_rng(seed)
    a = np.zeros((n, n), bool)
    for s in range(0, n, size):
        a[s:s + size, s:s + size] = g.random((size, size)) < 3.0 / size
        if s:
            a[s - 1, s] = True
    return a


def scipy_costs(a, w, src):
    """cost u32 [k, n] by scipy's Dijkstra (edge p -> v weighted w[v]) and, for the diagonal, the cheapest cycle"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    rows, cols = np.nonzero(a)
    keep = rows != cols
    m = csr_matrix((w[cols[keep]].astype(np.float64), (rows[keep], cols[keep])), shape=a.shape)
    base = dijkstra(m, directed=True, indices=list(src)).reshape(len(src), -1)
    cost = np.where(np.isfinite(base), base, float(D.NO_COST))
    for q, s in enumerate(src):
        into = np.flatnonzero(a[:, s])
        back = base[q, into] + float(w[s])
        cost[q, s] = back.min() if len(into) and np.isfinite(back.min()) else float(D.NO_COST)
    return cost.astype(np.uint32), m


def torch_costs(mask, w, src, chunk):
    """masked (min,+) rounds until nothing falls -> (cost float [k, n] with inf, rounds)"""
    k, n = len(src), mask.shape[0]
    ids = torch.arange(k, device=mask.device)
    cost = torch.full((k, n), float("inf"), device=mask.device)
    rounds = 0
    while True:
        rounds += 1
        base = cost.clone()
        base[ids, src] = 0.0
        new = torch.empty_like(cost)
        for q0 in range(0, k, chunk):
            new[q0:q0 + chunk] = (base[q0:q0 + chunk, :, None] + mask[None]).amin(dim=1) + w[None]
        new = torch.minimum(new, cost)
        if torch.equal(new, cost):
            return cost, rounds
        cost = new


def measure(e, a, w, src, reps, warmup, with_torch):
    n, k = a.shape[0], len(src)
    mt = pack(a)
    call = lambda **kw: D.reach_cost(e, mt, n, 1, src, w, **kw)
    every = dict(pred=True, len=True, via=True)
    c, p, ln, v, res = call(**every)
    want, csr = scipy_costs(a, w, src)
    assert (c.cpu().numpy().view(np.uint32) == want).all(), "scipy's costs differ from pg_reach_cost's"
    with e.tuning(cost_lds_bytes=0):
        g = call(**every)
    assert all(torch.equal(x, y) for x, y in zip((c, p, ln, v), g[:4])) and g[4] == res, "cost_lds_bytes changes the result"
    assert call()[4] == res
    legs = {"cost": lambda: call(), "all": lambda: call(**every)}

    def run_global():
        with e.tuning(cost_lds_bytes=0):
            return call(**every)
    legs["global"] = run_global
    out = {"result": res, "edges": int(a.sum()), "n_src": k}
    if with_torch:
        mask = torch.where(torch.from_numpy(a).cuda(), 0.0, float("inf")).to(torch.float32)
        wt, st = torch.from_numpy(w.astype(np.float32)).cuda(), torch.from_numpy(np.asarray(src, np.int64)).cuda()
        chunk = max(1, (1 << 31) // (4 * n * n))   # (2 GiB of sums at a time)
        tc, rounds = torch_costs(mask, wt, st, chunk)
        tc = tc.double()   # (float32 cannot hold NO_COST)
        tc = torch.where(torch.isfinite(tc), tc, float(D.NO_COST)).cpu().numpy().astype(np.uint32)
        assert (tc == want).all(), "the torch route's costs differ"
        out["torch_rounds"] = rounds
        legs["torch"] = lambda: torch_costs(mask, wt, st, chunk)
    # (the torch leg takes seconds: it has run once above for the check, is warmed once more here, and is
    # timed in the first two repetitions only: "torch_reps" in the line)
    for r in range(warmup):
        for name, fn in legs.items():
            if name != "torch" or r == 0:
                fn()
    t = {name: [] for name in legs}
    for r in range(reps):  # alternating
        for name, fn in legs.items():
            if name != "torch" or r < 2:
                t[name].append(event_ms(fn)[0])
    if with_torch:
        out["torch_reps"] = len(t["torch"])
    from scipy.sparse.csgraph import dijkstra
    t["scipy16"] = []
    for _ in range(max(2, reps // 2)):
        t0 = time.perf_counter()
        dijkstra(csr, directed=True, indices=list(src[:max(1, k // 16)]))
        t["scipy16"].append((time.perf_counter() - t0) * 1e3)
    best = {name: min(x) for name, x in t.items()}
    med = {name: statistics.median(x) for name, x in t.items()}
    out.update(ms_best=best, ms_median=med, over_all={name: x / best["all"] for name, x in best.items()},
               us_per_source={name: 1e3 * best[name] / k for name in ("cost", "all", "global")})
    return out


def ab(e, graphs, w, src, reps, out):
    """`all` with the row in LDS against the row in global memory: same inputs, interleaved, a JSON line per graph"""
    lines = []
    for name, a in graphs.items():
        mt = pack(a)
        every = dict(pred=True, len=True, via=True)
        legs = {"lds": 160 << 10, "global": 0}
        t = {k: [] for k in legs}
        for r in range(reps + 2):
            for leg, budget in legs.items():
                with e.tuning(cost_lds_bytes=budget):
                    ms = event_ms(lambda: D.reach_cost(e, mt, a.shape[0], 1, src, w, **every))[0]
                if r >= 2:   # (two warm-up rounds)
                    t[leg].append(ms)
        lines.append({"tool": "cost_bench --ab", "graph": name, "n": a.shape[0], "n_src": len(src), "reps": reps,
                      "ms_best": {k: min(x) for k, x in t.items()}, "ms_median": {k: statistics.median(x) for k, x in t.items()},
                      "ms_worst": {k: max(x) for k, x in t.items()}})
    text = "".join(json.dumps(x) + "\n" for x in lines)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    print(text, end="")


def chain(e, reps, out):
    """what a round costs when the frontier is one end point: the chain 0 -> 1 -> .. -> n - 1 from source 0 runs
    n - 1 rounds of two workgroup barriers each in one workgroup; both row variants, interleaved"""
    n = N
    a = np.zeros((n, n), bool)
    a[np.arange(n - 1), np.arange(1, n)] = True
    mt, w = pack(a), np.ones(n, np.uint16)
    t = {"lds": [], "global": []}
    for r in range(reps + 2):
        for leg, budget in (("lds", 160 << 10), ("global", 0)):
            with e.tuning(cost_lds_bytes=budget):
                ms, got = event_ms(lambda: D.reach_cost(e, mt, n, 1, [0], w, cost=False))
            assert got[4] == {"n_reached": n - 1, "n_via": (n - 1) * (n - 2) // 2, "max_cost": n - 1, "longest": n - 1}, got[4]
            if r >= 2:   # (two warm-up rounds)
                t[leg].append(ms)
    line = json.dumps({"tool": "cost_bench --chain", "n": n, "rounds": n - 1, "reps": reps, "ms_best": {k: min(x) for k, x in t.items()},
                       "ms_median": {k: statistics.median(x) for k, x in t.items()},
                       "us_per_round_best": {k: 1e3 * min(x) / (n - 1) for k, x in t.items()}})
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--ab", type=int, default=0, help="repetitions of the A/B alone")
    ap.add_argument("--chain", type=int, default=0, help="repetitions of the one-end-point-frontier run alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cost_bench needs the GPU"

    e = R.Engine(0)   # (the context only names the device: the call reads no table)
    if a.chain:
        return chain(e, a.chain, a.out)
    g = np.random.default_rng(9)
    w = g.integers(1, 10, N).astype(np.uint16)
    graphs = {"random4": random4(N, 6), "islands": islands(N, 7)}
    if a.ab:
        return ab(e, graphs, w, g.integers(0, N, max(a.sources)), a.ab, a.out)
    res = {"tool": "cost_bench", "n": N, "reps": a.reps, "plan": e.debug_reach_cost_plan(N), "runs": {}}
    for k in a.sources:
        src = g.integers(0, N, k)
        for name, graph in graphs.items():
            res["runs"]["%s_%d" % (name, k)] = measure(e, graph, w, src, a.reps, a.warmup, not a.no_torch and k == min(a.sources))
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
