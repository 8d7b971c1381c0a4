#!/usr/bin/env python3
"""Measurement tool: the rule coverage (pg_reach_rules) against the two routes to the same histograms
that exist without it, on the reach bench's workload: the config-5 cluster engine
(workloads.cluster_engine), 4096 x 4096 end points x 8 services.

Legs, timed with stream events after warm-up, alternating inside every repetition, best and median:
  rules_evals       pg_reach_rules, out_evals only
  rules_cells       pg_reach_rules, out_cells only
  rules_both        pg_reach_rules, both histograms
  rules_evals_noagg, rules_both_noagg
                    the same under rules_wave_agg = 0 (one LDS atomic per lane: the contention experiment)
  classify          pg_classify CONN with `counters` pointing at a scratch array over the product
                    materialised as tuples, service by service; the classify launches alone
  classify_mat      the same with the materialisation
  words_bincount    pg_reach_matrix with out_words, then torch.bincount of 4 * slot + ConnAction
Before any timing every route's histogram is compared with the others: out_evals with the scratch
counters, out_cells with the bincount, and the two rules_wave_agg settings with each other.
Prints one JSON line (and writes it to --out): milliseconds of every leg and the ratio of each baseline
to the rules leg that answers the same question.

  python tools/rules_bench.py [--side 4096] [--services 8] [--reps 7] [--out profiles/rules_bench.json]
The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/rules_bench.py --reps 3
whose kernel_stats.csv is kept as profiles/rules_bench_kernel_stats.csv.
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
from vpp_amd._capi import MODE_CONN  # noqa: E402


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
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--services", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rules_bench needs the GPU"

    e, _r, _local, pool = W.cluster_engine(0)
    g = np.random.default_rng(5)

    def side():   # as tools/reach_bench.py
        ips = pool[g.integers(0, len(pool), a.side)].copy()
        m = g.random(a.side) < 0.1
        ips[m] = g.integers(0, 1 << 32, int(m.sum()), dtype=np.uint64).astype(np.uint32)
        return ips
    src, dst = side(), side()
    ports = W.CLUSTER_PORTS
    svc = [(0 if i % 4 != 3 else 1, 40000 + i, ports[i % len(ports)]) for i in range(a.services)]
    n_svc, ns, nd = len(svc), len(src), len(dst)
    pairs = n_svc * ns * nd
    n_slots = e.num_counter_slots()

    # the classify route: the pairs as tuples on the device, service by service, counted into scratch
    ds = torch.from_numpy(src.view(np.int32)).cuda()
    dd = torch.from_numpy(dst.view(np.int32)).cuda()
    b = D.TupleBatch(ns * nd)
    out = torch.empty(ns * nd, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(n_slots, dtype=torch.int64, device="cuda")

    def materialise(v):
        pr, sp, dp = svc[v]
        b.src.copy_(ds.repeat_interleave(nd))
        b.dst.copy_(dd.repeat(ns))
        b.sport.fill_(sp - 65536 if sp >= 32768 else sp)  # (u16 ports in int16 storage)
        b.dport.fill_(dp - 65536 if dp >= 32768 else dp)
        b.proto.fill_(pr)

    def classify_all():
        """-> (ms of the materialisation, ms of the classify launches)"""
        scratch.zero_()
        mat = cls = 0.0
        for v in range(n_svc):
            mat += event_ms(lambda: materialise(v))[0]
            cls += event_ms(lambda: D.classify(e, MODE_CONN, -1, b, out, counters=scratch))[0]
        return mat, cls

    def words_bincount():
        _, full = D.reach_matrix(e, src, dst, svc, words=True)
        w = full.reshape(-1).to(torch.int64) & 0xFFFFFFFF
        return torch.bincount(((w & 0x3FFFFFFF) << 2) | (w >> 30), minlength=4 * n_slots).reshape(n_slots, 4)

    def rules(evals=True, cells=True):
        return D.reach_rules(e, src, dst, svc, evals=evals, cells=cells)

    # every route's histogram against the others
    ev, ce, res = rules()
    classify_all()
    torch.cuda.synchronize()
    assert torch.equal(ev, scratch), "out_evals differs from pg_classify's counters over the tuples"
    assert torch.equal(ce, words_bincount()), "out_cells differs from the histogram of out_words"
    assert torch.equal(rules(cells=False)[0], ev) and torch.equal(rules(evals=False)[1], ce)
    with e.tuning(rules_wave_agg=0):
        ev0, ce0, _ = rules()
    assert torch.equal(ev0, ev) and torch.equal(ce0, ce), "rules_wave_agg changes the result"
    assert int(ce.sum()) == pairs == res["n_cells"] and int(ev.sum()) == res["n_evals"]

    def noagg(**kw):
        with e.tuning(rules_wave_agg=0):
            return rules(**kw)
    legs = {"rules_evals": lambda: rules(cells=False), "rules_evals_noagg": lambda: noagg(cells=False),
            "rules_cells": lambda: rules(evals=False), "rules_both": rules, "rules_both_noagg": noagg,
            "words_bincount": words_bincount}
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
        classify_all()
    t = {name: [] for name in list(legs) + ["classify", "classify_mat"]}
    for _ in range(a.reps):  # alternating
        for name, fn in legs.items():
            t[name].append(event_ms(fn)[0])
        mat, cls = classify_all()
        t["classify"].append(cls)
        t["classify_mat"].append(mat + cls)
    best = {k: min(v) for k, v in t.items()}
    med = {k: statistics.median(v) for k, v in t.items()}
    out_res = {
        "tool": "rules_bench", "engine": "config-5 cluster (workloads.cluster_engine)", "n_src": ns, "n_dst": nd,
        "n_svc": n_svc, "pairs": pairs, "reps": a.reps, "n_slots": n_slots, "result": res,
        "slots_hit": int((ev > 0).sum()), "evals_per_pair": res["n_evals"] / pairs,
        "plan": e.debug_reach_rules_plan(n_slots, n_slots - res["n_rule_slots"], True, True, 1),
        "ms_best": best, "ms_median": med, "ms_all": t,
        # a baseline's time over the time of the rules leg that answers the same question (> 1: the call is faster)
        "classify_over_rules_evals": best["classify"] / best["rules_evals"],
        "classify_mat_over_rules_evals": best["classify_mat"] / best["rules_evals"],
        "words_bincount_over_rules_cells": best["words_bincount"] / best["rules_cells"],
        "classify_over_rules_both": best["classify"] / best["rules_both"],
        "words_bincount_over_rules_both": best["words_bincount"] / best["rules_both"],
        "noagg_over_agg": best["rules_both_noagg"] / best["rules_both"],
        "evals_noagg_over_agg": best["rules_evals_noagg"] / best["rules_evals"],
        "rules_both_pairs_per_s": pairs / (best["rules_both"] * 1e-3),
    }
    line = json.dumps(out_res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
