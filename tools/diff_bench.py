#!/usr/bin/env python3
"""Measurement tool: the reachability diff (pg_reach_diff) against the routes to the same answer that
exist without it, on two pg_reach_matrix results of 4096 x 4096 end points x 8 services: the config-5
cluster engine (workloads.cluster_engine) and a second one built the same way with one pod's ACL
changed (a DENY of every TCP packet put in front of its rules).

Legs, timed with stream events after warm-up, alternating inside every repetition, best and median:
  diff_count   pg_reach_diff, count only (with the histogram)
  diff_list    pg_reach_diff with the list (a buffer sized by the count)
  diff_rows    pg_reach_diff, count only, with row_changes
  torch_dev    the route without the diff, on the device over the same two buffers: XOR, unpack the
               16 cells of every word by shifts, nonzero
  host_numpy   the same with both buffers copied to the host first, numpy
  copy         a plain device copy of the bytes the diff reads -- two passes over both inputs -- as the
               ceiling
The diff's list is compared with the torch route's on the whole matrix first. A second run repeats the
legs on a synthetic pair in which every cell changes (the per-word row atomics at their worst; the
list is the whole matrix). Prints one JSON line (and writes it to --out): milliseconds of every leg
and each leg's ratio to torch_dev and to copy.

  python tools/diff_bench.py [--side 4096] [--services 8] [--reps 9] [--out profiles/diff_bench.json]
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

KEY = "config/vpp/acls/v2/acl/"


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def edited_engine():
    """the cluster engine again, the first ACL that is bound to an interface and has rules denying all TCP"""
    e, _r, _local, _pool = W.cluster_engine(0)
    for name in e.ACLNames():
        acl = e.GetACLByName(name)
        if acl["rules"] and (acl.get("ingress") or acl.get("egress")):
            deny = {"action": 0, "src": "", "dst": "", "tcp": {"src": [0, 65535], "dst": [0, 65535]}}
            acl = dict(acl, rules=[deny] + acl["rules"])
            e.ApplyTxn(False, [(KEY + name, acl)])
            return e, _r, name
    raise AssertionError("no ACL to change")


def torch_changes(bt, at, n_cols):
    """the parent route on the device -> (row, column) of every changed cell, int64 [m, 2]"""
    x = bt ^ at
    sh = torch.arange(0, 32, 2, dtype=torch.int32, device=x.device)
    cells = ((x.reshape(x.shape[0], -1, 1) >> sh) & 3).reshape(x.shape[0], -1)[:, :n_cols]
    return torch.nonzero(cells)


def numpy_changes(bt, at, n_cols):
    b, a = bt.cpu().numpy().view(np.uint32), at.cpu().numpy().view(np.uint32)
    x = b ^ a
    cells = ((x[:, :, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).reshape(x.shape[0], -1)[:, :n_cols]
    return np.argwhere(cells)


def measure(e, bt, at, n_cols, reps, warmup, host_reps):
    """bt, at: int32 [n_rows, row_words]; -> the result dict of one pair"""
    n_rows = bt.shape[0]
    # check first: the diff's list against the torch route on the whole matrix
    n, changes, trans, rows = D.reach_diff(e, bt, at, n_cols, row_changes=True)
    want = torch_changes(bt, at, n_cols)
    row, col, cb, ca = D.unpack_changes(changes)
    assert n == len(want) == len(row), (n, len(want))
    wn = want.cpu().numpy()
    assert (row == wn[:, 0]).all() and (col == wn[:, 1]).all(), "the diff's list differs from the torch route's"
    assert (cb != ca).all() and int(trans.sum()) == n_rows * n_cols
    assert int(trans.sum() - np.trace(trans)) == n
    assert (rows.cpu().numpy() == np.bincount(wn[:, 0], minlength=n_rows)).all()
    del want, wn, row, col, cb, ca, changes, rows
    dst = [torch.empty_like(bt), torch.empty_like(at)]

    def copy():
        for _ in range(2):
            dst[0].copy_(bt)
            dst[1].copy_(at)

    legs = {
        "diff_count": lambda: D.reach_diff(e, bt, at, n_cols, cap=0),
        "diff_list": lambda: D.reach_diff(e, bt, at, n_cols, cap=n),
        "diff_rows": lambda: D.reach_diff(e, bt, at, n_cols, cap=0, row_changes=True),
        "torch_dev": lambda: torch_changes(bt, at, n_cols),
        "copy": copy,
    }
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    t = {name: [] for name in legs}
    for _ in range(reps):  # alternating
        for name, fn in legs.items():
            t[name].append(event_ms(fn)[0])
    t["host_numpy"] = [event_ms(lambda: numpy_changes(bt, at, n_cols))[0] for _ in range(host_reps)]
    best = {name: min(v) for name, v in t.items()}
    med = {name: statistics.median(v) for name, v in t.items()}
    return {"n_rows": n_rows, "n_cols": n_cols, "cells": n_rows * n_cols, "input_bytes": 2 * bt.numel() * 4,
            "changes": n, "trans": trans.tolist(), "ms_best": best, "ms_median": med,
            "over_torch_dev": {k: best["torch_dev"] / v for k, v in best.items()},
            "over_copy": {k: best["copy"] / v for k, v in best.items()},
            "over_torch_dev_median": {k: med["torch_dev"] / v for k, v in med.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--services", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "diff_bench needs the GPU"

    e0, _r0, _local, pool = W.cluster_engine(0)
    e1, _r1, changed = edited_engine()
    g = np.random.default_rng(5)

    def side():  # the cluster's pods and Internet hosts, a tenth uniform addresses (as tools/reach_bench.py)
        ips = pool[g.integers(0, len(pool), a.side)].copy()
        m = g.random(a.side) < 0.1
        ips[m] = g.integers(0, 1 << 32, int(m.sum()), dtype=np.uint64).astype(np.uint32)
        return ips
    src, dst = side(), side()
    ports = W.CLUSTER_PORTS
    svc = [(0 if i % 4 != 3 else 1, 40000 + i, ports[i % len(ports)]) for i in range(a.services)]
    nd = len(dst)
    bt = D.reach_matrix(e0, src, dst, svc).reshape(-1, D.reach_row_words(nd))
    at = D.reach_matrix(e1, src, dst, svc).reshape(-1, D.reach_row_words(nd))
    torch.cuda.synchronize()
    real = measure(e1, bt, at, nd, a.reps, a.warmup, a.host_reps)
    assert real["changes"] > 0, "the edit changed no pair"

    # every cell changes: after = before with the low bit of every cell flipped
    at.copy_(bt ^ 0x55555555)
    torch.cuda.synchronize()
    worst = measure(e1, bt, at, nd, a.reps, a.warmup, 1)
    assert worst["changes"] == worst["cells"]

    res = {"tool": "diff_bench", "engine": "config-5 cluster (workloads.cluster_engine)", "changed_acl": changed,
           "n_src": len(src), "n_dst": nd, "n_svc": len(svc), "reps": a.reps, "policy_change": real, "all_cells_changed": worst}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
