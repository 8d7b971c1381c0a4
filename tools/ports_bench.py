#!/usr/bin/env python3
"""Measurement tool: the port sweep (pg_reach_ports) against the parent route to the same
evaluations -- pg_reach_matrix over the K representative services (TCP, src port, lo[k]), in its
service-major layout -- on the config-5 cluster engine (workloads.cluster_engine), 1024 x 1024 end
points, TCP, K as the world gives it (pg_port_intervals).

Three legs, each against the matrix call with the same outputs: codes only, codes + out_open
(against the codes-only matrix; the matrix has no count), codes + out_words. Timed with stream
events after warm-up, the legs alternating inside every repetition, best and median of the
repetitions. The sweep's codes, words and open counts are compared with the matrix's on every (pair,
interval) first. Prints one JSON line (and writes it to --out): K, pair-intervals, milliseconds and
pair-intervals per second of every leg, the ratios, and for scale the computed (not run) time of
the naive sweep: 65,536 services at the matrix's measured pairs per second.

  python tools/ports_bench.py [--side 1024] [--reps 9] [--out profiles/ports_bench.json]
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

SPORT = 40000


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ports_bench needs the GPU"

    e, _r, _local, pool = W.cluster_engine(0)
    g = np.random.default_rng(5)

    def side():  # the cluster's pods and Internet hosts, a tenth uniform addresses (as tools/reach_bench.py)
        ips = pool[g.integers(0, len(pool), a.side)].copy()
        m = g.random(a.side) < 0.1
        ips[m] = g.integers(0, 1 << 32, int(m.sum()), dtype=np.uint64).astype(np.uint32)
        return ips
    src, dst = side(), side()
    ns, nd = len(src), len(dst)
    lo = D.port_intervals(e, 0)
    k = len(lo)
    assert k <= 4096, "more intervals than pg_reach_matrix takes services"
    svc = [(0, SPORT, int(p)) for p in lo]
    work = ns * nd * k

    def sweep(open_count=False, words=False):
        return D.reach_ports(e, src, dst, 0, SPORT, open_count=open_count, words=words)

    def matrix(words=False):
        return D.reach_matrix(e, src, dst, svc, words=words)

    # the two calls agree on every (pair, interval)
    _, codes, n_open, full = sweep(open_count=True, words=True)
    packed, mfull = matrix(words=True)
    torch.cuda.synchronize()
    assert torch.equal(full, mfull.permute(1, 2, 0)), "sweep and matrix words differ"
    acts = D.unpack_ports(codes, ns, nd, k)
    assert (acts == D.unpack_reach(packed, k, ns, nd).transpose(1, 2, 0)).all()
    ln = np.diff(np.append(lo.astype(np.int64), 65536))
    want_open = ((acts == 2) * ln).sum(axis=2)
    assert (n_open.cpu().numpy().view(np.uint32) == want_open).all()
    del full, mfull, packed, codes

    legs = {"sweep": lambda: sweep(), "sweep_open": lambda: sweep(open_count=True),
            "sweep_words": lambda: sweep(words=True), "matrix": lambda: matrix(),
            "matrix_words": lambda: matrix(words=True)}
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    t = {name: [] for name in legs}
    for _ in range(a.reps):  # alternating
        for name, fn in legs.items():
            t[name].append(event_ms(fn)[0])

    best = {name: min(v) for name, v in t.items()}
    med = {name: statistics.median(v) for name, v in t.items()}
    res = {
        "tool": "ports_bench", "engine": "config-5 cluster (workloads.cluster_engine)", "protocol": "tcp",
        "n_src": ns, "n_dst": nd, "K": k, "pair_intervals": work, "reps": a.reps,
        "open_ports_mean": float(want_open.mean()), "pairs_with_open_ports": int((want_open > 0).sum()),
        "verdict_mix": np.bincount(acts.ravel(), minlength=4).tolist(),
        "ms_best": best, "ms_median": med,
        "pair_intervals_per_s": {name: work / (ms * 1e-3) for name, ms in best.items()},
        "sweep_over_matrix": best["matrix"] / best["sweep"],
        "sweep_open_over_matrix": best["matrix"] / best["sweep_open"],
        "sweep_words_over_matrix_words": best["matrix_words"] / best["sweep_words"],
        "sweep_over_matrix_median": med["matrix"] / med["sweep"],
        # for scale, computed and not run: every port as a service of its own at the matrix's rate
        "naive_65536_services_ms": best["matrix"] * 65536.0 / k,
        "naive_over_sweep": best["matrix"] * 65536.0 / k / best["sweep"],
    }
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
