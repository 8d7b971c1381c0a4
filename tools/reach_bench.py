#!/usr/bin/env python3
"""Measurement tool: the reachability matrix (pg_reach_matrix) against the route it replaces --
the same pairs materialised as tuples on the device, then pg_classify CONN without counters -- on
the config-5 cluster engine (workloads.cluster_engine), 4096 x 4096 end points x 8 services.

Both routes are timed with stream events after warm-up, alternating, best and median of the
repetitions; the parent route's classify time is reported alone and with the materialisation. The two
routes' verdict words are compared on the whole matrix first. Prints one JSON line (and writes it to
--out): pairs, seconds and pairs per second of each route, and matrix rate / classify-only rate.

  python tools/reach_bench.py [--side 4096] [--services 8] [--reps 7] [--out profiles/reach_bench.json]
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "reach_bench needs the GPU"

    e, _r, _local, pool = W.cluster_engine(0)
    g = np.random.default_rng(5)
    # end points: the cluster's pods and Internet hosts, a tenth uniform addresses (duplicates allowed)
    def side():
        ips = pool[g.integers(0, len(pool), a.side)].copy()
        m = g.random(a.side) < 0.1
        ips[m] = g.integers(0, 1 << 32, int(m.sum()), dtype=np.uint64).astype(np.uint32)
        return ips
    src, dst = side(), side()
    ports = W.CLUSTER_PORTS
    svc = [(0 if i % 4 != 3 else 1, 40000 + i, ports[i % len(ports)]) for i in range(a.services)]
    n_svc, ns, nd = len(svc), len(src), len(dst)
    pairs = n_svc * ns * nd

    # the parent route: the pairs as tuples on the device, service by service
    ds = torch.from_numpy(src.view(np.int32)).cuda()
    dd = torch.from_numpy(dst.view(np.int32)).cuda()
    n1 = ns * nd
    b = D.TupleBatch(n1)
    out = torch.empty(n1, dtype=torch.int32, device="cuda")

    def materialise(v):
        pr, sp, dp = svc[v]
        b.src.copy_(ds.repeat_interleave(nd))
        b.dst.copy_(dd.repeat(ns))
        b.sport.fill_(sp - 65536 if sp >= 32768 else sp)  # (u16 ports in int16 storage)
        b.dport.fill_(dp - 65536 if dp >= 32768 else dp)
        b.proto.fill_(pr)

    def classify_all(timed):
        mat = cls = 0.0
        for v in range(n_svc):
            m, _ = event_ms(lambda: materialise(v))
            c, _ = event_ms(lambda: D.classify(e, MODE_CONN, -1, b, out))
            mat, cls = mat + m, cls + c
            if not timed:
                yield v, out
        if timed:
            yield mat, cls

    def matrix(words=False):
        return D.reach_matrix(e, src, dst, svc, words=words)

    # the two routes agree on every pair
    _, full = matrix(words=True)
    torch.cuda.synchronize()
    for v, o in classify_all(False):
        assert torch.equal(o, full[v].reshape(-1)), "service %d: matrix and classify differ" % v
    packed = matrix()
    torch.cuda.synchronize()
    acts = D.unpack_reach(packed, n_svc, ns, nd)
    assert (acts == (full.cpu().numpy().view(np.uint32) >> 30)).all()
    del full

    for _ in range(a.warmup):
        matrix()
        list(classify_all(True))
    t_mat, t_words, t_cls, t_mz = [], [], [], []
    for _ in range(a.reps):  # alternating
        t_mat.append(event_ms(matrix)[0])
        mz, cl = next(classify_all(True))
        t_cls.append(cl)
        t_mz.append(mz + cl)
        t_words.append(event_ms(lambda: matrix(words=True))[0])

    def rate(ms):
        return pairs / (ms * 1e-3)
    res = {
        "tool": "reach_bench", "engine": "config-5 cluster (workloads.cluster_engine)",
        "n_src": ns, "n_dst": nd, "n_svc": n_svc, "pairs": pairs, "reps": a.reps,
        "verdict_mix": np.bincount(acts.ravel(), minlength=4).tolist(),
        "matrix_ms_best": min(t_mat), "matrix_ms_median": statistics.median(t_mat), "matrix_ms_all": t_mat,
        "matrix_words_ms_best": min(t_words),
        "classify_ms_best": min(t_cls), "classify_ms_median": statistics.median(t_cls),
        "classify_plus_materialise_ms_best": min(t_mz),
        "matrix_pairs_per_s": rate(min(t_mat)), "matrix_words_pairs_per_s": rate(min(t_words)),
        "classify_pairs_per_s": rate(min(t_cls)), "classify_plus_materialise_pairs_per_s": rate(min(t_mz)),
        "matrix_over_classify": min(t_cls) / min(t_mat),
        "matrix_over_classify_median": statistics.median(t_cls) / statistics.median(t_mat),
        "matrix_over_classify_plus_materialise": min(t_mz) / min(t_mat),
    }
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
