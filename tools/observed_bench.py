#!/usr/bin/env python3
"""Measurement tool: the observed reachability (pg_reach_observed) against a torch statement of the same
result and against the stream ceiling, on the cluster workload the other audit benches use: the config-5
cluster engine's pods (workloads.cluster_engine) as both end-point lists, 8 services on the cluster ports.

Two flow batches of 2^24 flows each are drawn on the device with pg_gen_tuples:
  skewed    90 % of the addresses from 32 hot pods, the rest uniform u32: most flows repeat few cells
  uniform   every address from the whole pod list: the cells are hit evenly, the worst case for the atomics
Legs, per batch, timed with stream events after warm-up, alternating inside every repetition, best and median:
  observed            pg_reach_observed, out_packed only, the knobs at their defaults
  observed_flow       with out_flow
  observed_tf0/1/2    observed_test_first = 0 (always the atomic), 1 (a plain load first), 2 (a load past the L1 first)
  observed_hbm        observed_lds_bytes = 0: the address tables probed in HBM
  torch               searchsorted over the sorted addresses and service keys, index_put_ into a bool
                      [n_svc, n_src, n_dst] matrix, packed to the audits' words -- on the same device arrays
  stream_probe        pg_stream_probe with fields = 1 over the same flows: what moving the bytes costs
Before any timing the torch matrix is compared with pg_reach_observed's, and every knob setting with the
default's. Prints one JSON line (and writes it to --out): milliseconds of every leg, flows per second,
and the ratios torch / observed and observed / stream_probe.

  python tools/observed_bench.py [--flows 16777216] [--reps 3] [--out profiles/observed_bench.json]
The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/observed_bench.py --reps 1
whose kernel_stats.csv is kept as profiles/observed_bench_kernel_stats.csv.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, default=1 << 24)
    ap.add_argument("--services", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "observed_bench needs the GPU"

    e, _r, _local, pool = W.cluster_engine(0)
    ips = np.unique(np.asarray(pool, np.uint32))
    ports = W.CLUSTER_PORTS
    svc = [(0 if i % 4 != 3 else 1, 40000 + i, ports[i % len(ports)]) for i in range(a.services)]
    assert len({(p, d) for p, _, d in svc}) == len(svc), "the torch baseline takes distinct service keys"
    n_svc, n_ip = len(svc), len(ips)
    gen = dict(port_pool=np.array(ports, np.uint16), port_pool_pct=80, tcp_pct=60, udp_pct=30)
    batches = {"skewed": D.TupleBatch(a.flows), "uniform": D.TupleBatch(a.flows)}
    D.gen_tuples(e, batches["skewed"], seed=21, ip_pool=ips[:: max(1, n_ip // 32)][:32], pool_pct=90, dst_pool_pct=90, **gen)
    D.gen_tuples(e, batches["uniform"], seed=22, ip_pool=ips, pool_pct=100, dst_pool_pct=100, **gen)
    torch.cuda.synchronize()

    # the torch statement: the lists are sorted and distinct, so an index is the searchsorted position
    t_ips = torch.from_numpy(ips.astype(np.int64)).cuda()
    keys = np.array(sorted((p << 16) | d for p, _, d in svc), np.int64)
    order = np.argsort([(p << 16) | d for p, _, d in svc])
    t_keys, t_order = torch.from_numpy(keys).cuda(), torch.from_numpy(order.astype(np.int64)).cuda()
    rw = D.reach_row_words(n_ip)
    shifts = (2 * torch.arange(16, device="cuda", dtype=torch.int32))

    def find(sorted_vals, x):
        at = torch.searchsorted(sorted_vals, x).clamp_(max=len(sorted_vals) - 1)
        return at, sorted_vals[at] == x

    def by_torch(b):
        si, s_ok = find(t_ips, b.src.to(torch.int64) & 0xFFFFFFFF)
        di, d_ok = find(t_ips, b.dst.to(torch.int64) & 0xFFFFFFFF)
        pr = b.proto.to(torch.int64).clamp_(max=3)
        key = (pr << 16) | torch.where(pr < 2, b.dport.to(torch.int64) & 0xFFFF, torch.zeros_like(pr))
        ki, k_ok = find(t_keys, key)
        m = s_ok & d_ok & k_ok
        mat = torch.zeros((n_svc, n_ip, 16 * rw), dtype=torch.bool, device="cuda")
        mat.index_put_((t_order[ki[m]], si[m], di[m]), torch.ones((), dtype=torch.bool, device="cuda"))
        return ((mat.reshape(n_svc, n_ip, rw, 16).to(torch.int32) * 2) << shifts).sum(dim=3, dtype=torch.int32)

    def observed(b, flow=False, **knobs):
        with e.tuning(**knobs):
            return D.reach_observed(e, ips, ips, svc, b, flow=flow)

    probe_out = torch.empty(a.flows, dtype=torch.int32, device="cuda")
    results = {}
    for name, b in batches.items():
        packed, _, _, res = observed(b)
        assert torch.equal(packed, by_torch(b)), "the torch matrix differs from pg_reach_observed's"
        for knobs in ({"observed_test_first": 0}, {"observed_test_first": 1}, {"observed_test_first": 2}, {"observed_lds_bytes": 0}):
            assert torch.equal(observed(b, **knobs)[0], packed), "a knob changes the result"
        legs = {"observed": lambda: observed(b), "observed_flow": lambda: observed(b, flow=True),
                "observed_tf0": lambda: observed(b, observed_test_first=0),
                "observed_tf1": lambda: observed(b, observed_test_first=1),
                "observed_tf2": lambda: observed(b, observed_test_first=2),
                "observed_hbm": lambda: observed(b, observed_lds_bytes=0), "torch": lambda: by_torch(b),
                "stream_probe": lambda: D.stream_probe(e, 1, b, probe_out)}
        for _ in range(a.warmup):
            for fn in legs.values():
                fn()
        t = {k: [] for k in legs}
        for _ in range(a.reps):  # alternating
            for k, fn in legs.items():
                t[k].append(event_ms(fn)[0])
        best = {k: min(v) for k, v in t.items()}
        results[name] = {
            "result": res, "cells": n_svc * n_ip * n_ip, "ms_best": best,
            "ms_median": {k: statistics.median(v) for k, v in t.items()}, "ms_all": t,
            "observed_flows_per_s": a.flows / (best["observed"] * 1e-3),
            # > 1: the call is faster than the torch statement; the call's time over the stream ceiling's
            "torch_over_observed": best["torch"] / best["observed"],
            "observed_over_stream_probe": best["observed"] / best["stream_probe"],
            "tf0_over_tf1": best["observed_tf0"] / best["observed_tf1"],
            "tf0_over_tf2": best["observed_tf0"] / best["observed_tf2"],
            "hbm_over_lds": best["observed_hbm"] / best["observed"],
        }
    out_res = {"tool": "observed_bench", "engine": "config-5 cluster (workloads.cluster_engine)", "n_src": n_ip, "n_dst": n_ip,
               "n_svc": n_svc, "flows": a.flows, "reps": a.reps, "plan": e.debug_reach_observed_plan(n_ip, n_ip, n_svc),
               "default_test_first": e.get_tuning("observed_test_first"), "batches": results}
    line = json.dumps(out_res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
