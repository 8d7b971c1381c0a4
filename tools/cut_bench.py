#!/usr/bin/env python3
"""Measurement tool: the reachability cut (pg_reach_cut) against the routes to the same answer that exist
without it, at 4096 and 16384 end points, each on two graphs in one slice with 8 entries, 8 targets and
max_cut 64:
  random  a random graph of 3 edges per node on average, entries and targets drawn at random, no edge from
          an entry straight to a target
  layers  fully connected layers of widths 8, 100, 20, the rest, 20, 100, 8: the entries the first layer,
          the targets the last, the cut 20 wide

Legs, the device ones timed with stream events after warm-up, alternating inside every repetition, best and
median:
  result      pg_reach_cut, the result alone
  all         pg_reach_cut with out_cut, out_prev and out_next
  torch       the same level-wise search written in torch on the device over the same buffer: unpack the
              cells to an fp16 0 / 1 matrix, then per level one vector-matrix product for the edge arcs and
              O(n) index steps for the other three kinds of arc, parents by argmax over the frontier's rows
              (the least id), the parent chain walked on the host, the residual search from the sink, the two
              plain searches and the flags
  scipy       scipy.sparse.csgraph.maximum_flow on the split graph on the CPU plus residual reachability, from
              a host bool matrix that is already there
  scipy_full  the same with what a user without the call pays first: the device -> host copy of the packed
              matrix and its unpacking
Every exact field of the result and all four flag bits of out_cut are compared with the torch route's and
scipy's before any timing; the witness of the call is validated. Prints one JSON line (and writes it to
--out): milliseconds of every leg, each leg's ratio to `all`, `levels` and the launches of the call.

  python tools/cut_bench.py [--sides 4096 16384] [--reps 5] [--out profiles/cut_bench.json]
The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/cut_bench.py --reps 2 --sides 4096
whose kernel_stats.csv is kept as profiles/cut_bench_kernel_stats.csv.
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
NEAR, FAR, NEAR_REACH, FAR_REACH = 1, 2, 4, 8
EXACT = ("separable", "capped", "n_direct", "cut_size", "n_paths", "near_reach", "far_reach")
MAX_CUT = 64


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


def random_graph(n, per_node, seed):
    g = np.random.default_rng(seed)
    a = np.zeros((n, n), bool)
    for r0 in range(0, n, 1024):
        a[r0:r0 + 1024] = g.random((min(1024, n - r0), n)) < per_node / n
    ids = g.permutation(n)[:16]
    a[np.ix_(ids[:8], ids[8:])] = False   # (no entry next to a target: the input stays separable)
    return a, [int(x) for x in ids[:8]], [int(x) for x in ids[8:]]


def layers_graph(n):
    widths = [8, 100, 20, n - 256, 20, 100, 8]
    at = np.concatenate([[0], np.cumsum(widths)])
    a = np.zeros((n, n), bool)
    for k in range(len(widths) - 1):
        a[at[k]:at[k + 1], at[k + 1]:at[k + 2]] = True
    return a, list(range(8)), list(range(n - 8, n))


def unpack_host(words, n):
    """packed u32 [n_svc, n, row_words] -> bool [n, n]: the cells of any slice that hold ALLOW"""
    a = np.zeros((n, n), bool)
    sh = 2 * np.arange(16, dtype=np.uint32)
    for s in words:
        for r0 in range(0, n, 1024):
            a[r0:r0 + 1024] |= (((s[r0:r0 + 1024, :, None] >> sh) & 3) == ALLOW).reshape(-1, 16 * s.shape[1])[:, :n]
    return a


# ---- (a) the same search in torch ------------------------------------------------------------------
def unpack_allow(mt, n):
    sh = torch.arange(0, 32, 2, dtype=torch.int32, device=mt.device)
    return (((mt.reshape(mt.shape[0], -1, 1) >> sh) & 3) == ALLOW).reshape(mt.shape[0], -1)[:, :n]


def torch_search(M, link, rx, ry, fy, stop, plain, parents):
    """one search of levels: X pulls along M (fy @ M), the back, forward and edge-back arcs as index steps ->
    (rx, ry, the least target reached or -1, px, py, levels)"""
    n = M.shape[0]
    dev = M.device
    ids = torch.arange(n, device=dev)
    fx = torch.zeros(n, dtype=torch.bool, device=dev)
    px = torch.full((n,), -1, dtype=torch.int64, device=dev) if parents else None
    py = torch.full((n,), -1, dtype=torch.int64, device=dev) if parents else None
    levels = 0
    while True:
        levels += 1
        edge = ((fy.to(M.dtype) @ M) > 0)
        if plain:
            nx = edge & ~rx
            ny = nx
        else:
            flow = link >= 0
            back = flow & fy & ~rx
            nx = (edge & ~rx) | back
            src = torch.where(flow, link, ids)
            ny = fx[src] & ~ry
            if parents:
                pulled = torch.nonzero(nx & ~back).flatten()
                if len(pulled):
                    cols = (M[:, pulled] > 0) & fy[:, None]
                    px[pulled] = cols.to(torch.uint8).argmax(dim=0)
                px[back] = ids[back]
                py[ny] = src[ny]
        rx, ry = rx | nx, ry | ny
        if stop is not None:
            hit = torch.nonzero(nx & stop).flatten()
            if len(hit):
                return rx, ry, int(hit[0]), px, py, levels
        if not bool((nx | ny).any()):
            return rx, ry, -1, px, py, levels
        fx, fy = nx, ny


def torch_route(mt, n, entry, target, max_cut, dt=torch.float16):
    """-> (the exact result fields, flags uint8 [n] on the device, levels)"""
    dev = mt.device
    a = unpack_allow(mt.reshape(-1, mt.shape[-1]), n).reshape(-1, n, n).any(dim=0)
    a.fill_diagonal_(False)
    e = torch.zeros(n, dtype=torch.bool, device=dev)
    t = torch.zeros(n, dtype=torch.bool, device=dev)
    e[torch.tensor(sorted(set(entry)), dtype=torch.int64, device=dev)] = True
    t[torch.tensor(sorted(set(target)), dtype=torch.int64, device=dev)] = True
    direct = int((a[e][:, t]).sum()) + int((e & t).sum())
    zero = torch.zeros(n, dtype=torch.uint8, device=dev)
    if direct:
        return dict(zip(EXACT, (0, 0, direct, D.NO_CUT, 0, 0, 0))), zero, 0
    A = a.to(dt)
    AT = A.T.contiguous()
    prev, nxt = [-1] * n, [-1] * n
    e_host, t_host = e.cpu().tolist(), t.cpu().tolist()
    paths = levels = 0
    while True:
        if paths == max_cut + 1:
            return dict(zip(EXACT, (1, 1, 0, D.NO_CUT, paths, 0, 0))), zero, levels
        link = torch.tensor(nxt, dtype=torch.int64, device=dev)
        s_in, s_out, hit, p_in, p_out, lv = torch_search(A, link, e.clone(), e | t, e.clone(), t, False, True)
        levels += lv
        if hit < 0:
            break
        p_in, p_out = p_in.cpu().tolist(), p_out.cpu().tolist()
        v, at_in = hit, True   # the chain from the target's in half back to an entry, the flow flipped
        while True:
            if at_in:
                p = p_in[v]
                if p == v:
                    prev[v] = nxt[v] = -1
                    at_in = False
                    continue
                if not e_host[v] and not t_host[v]:
                    prev[v] = p
                if e_host[p]:
                    break
                nxt[p] = v
                v, at_in = p, False
            else:
                q = p_out[v]
                if q != v:
                    v = q
                at_in = True
        paths += 1
    link = torch.tensor(prev, dtype=torch.int64, device=dev)
    b_out, b_in, _, _, _, lv = torch_search(AT, link, t.clone(), e | t, t.clone(), None, False, False)
    levels += lv
    near = s_in & ~s_out & ~e & ~t
    far = b_out & ~b_in & ~e & ~t
    reach = []
    for c in (near, far):
        r, _, _, _, _, lv = torch_search(A, None, e | c, e | c, e.clone(), None, True, False)
        levels += lv
        reach.append(r & ~c)
    flags = (near * NEAR + far * FAR + reach[0] * NEAR_REACH + reach[1] * FAR_REACH).to(torch.uint8)
    return dict(zip(EXACT, (1, 0, 0, paths, paths, int(reach[0].sum()), int(reach[1].sum())))), flags, levels


# ---- (b) scipy on the CPU --------------------------------------------------------------------------
def scipy_route(a, entry, target, max_cut):
    """-> (the exact result fields, flags uint8 [n])"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import breadth_first_order, maximum_flow
    n = a.shape[0]
    e, t = np.zeros(n, bool), np.zeros(n, bool)
    e[entry] = True
    t[target] = True
    direct = int(a[np.ix_(e, t)].sum()) + int((e & t).sum())
    if direct:
        return dict(zip(EXACT, (0, 0, direct, D.NO_CUT, 0, 0, 0))), np.zeros(n, np.uint8)
    u, v = np.nonzero(a)
    keep = (u != v) & ~t[u] & ~e[v]
    u, v = u[keep], v[keep]
    inner = np.flatnonzero(~e & ~t)
    big = n + 1
    src = np.concatenate([2 * u + 1, 2 * inner, np.full(int(e.sum()), 2 * n), 2 * np.flatnonzero(t)])
    dst = np.concatenate([2 * v, 2 * inner + 1, 2 * np.flatnonzero(e) + 1, np.full(int(t.sum()), 2 * n + 1)])
    cap = np.concatenate([np.full(len(u), big), np.ones(len(inner)), np.full(int(e.sum()) + int(t.sum()), big)]).astype(np.int32)
    m = 2 * n + 2
    capacity = sp.csr_matrix((cap, (src, dst)), shape=(m, m))
    r = maximum_flow(capacity, 2 * n, 2 * n + 1)
    k = int(r.flow_value)
    if k > max_cut:
        return dict(zip(EXACT, (1, 1, 0, D.NO_CUT, max_cut + 1, 0, 0))), np.zeros(n, np.uint8)
    residual = (capacity - r.flow).tocsr()
    residual.data = (residual.data > 0).astype(np.int32)
    residual.eliminate_zeros()
    sides = []
    for start, g in ((2 * n, residual), (2 * n + 1, residual.T.tocsr())):
        seen = np.zeros(m, bool)
        seen[breadth_first_order(g, start, directed=True, return_predecessors=False)] = True
        sides.append(seen)
    ok = ~e & ~t
    near = ok & sides[0][0:2 * n:2] & ~sides[0][1:2 * n:2]
    far = ok & sides[1][1:2 * n:2] & ~sides[1][0:2 * n:2]
    reach = []
    u, v = np.nonzero(a)   # (the plain graph, with node n feeding the entries)
    for c in (near, far):
        left = ~c[u] & ~c[v]
        rows, cols = np.concatenate([u[left], np.full(int(e.sum()), n)]), np.concatenate([v[left], np.flatnonzero(e)])
        g = sp.csr_matrix((np.ones(len(rows), np.int32), (rows, cols)), shape=(n + 1, n + 1))
        seen = np.zeros(n + 1, bool)
        seen[breadth_first_order(g, n, directed=True, return_predecessors=False)] = True
        reach.append(seen[:n])
    flags = (near * NEAR + far * FAR + reach[0] * NEAR_REACH + reach[1] * FAR_REACH).astype(np.uint8)
    return dict(zip(EXACT, (1, 0, 0, k, k, int(reach[0].sum()), int(reach[1].sum())))), flags


def check_witness(a, entry, target, prev, nxt, n_paths):
    held, wanted = set(entry), set(target)
    routes = D.cut_routes(prev, nxt, entry)
    assert len(routes) == n_paths, (len(routes), n_paths)
    inner = [v for r in routes for v in r[1:-1]]
    assert len(set(inner)) == len(inner) and not set(inner) & (held | wanted)
    for r in routes:
        assert r[0] in held and r[-1] in wanted and all(a[u, v] for u, v in zip(r, r[1:])), r
    assert int((prev != D.NO_HOP).sum()) == len(inner)


def measure(e, a, mt, n, entry, target, reps, warmup):
    call = lambda **kw: D.reach_cut(e, mt, n, 1, entry, target, MAX_CUT, **kw)
    cut, prev, nxt, res = call(cut=True, paths=True)
    assert call()[3] == res, "the result alone differs"
    exact = {k: res[k] for k in EXACT}
    wres, wflags, wlevels = torch_route(mt, n, entry, target, MAX_CUT)
    assert exact == wres and torch.equal(cut, wflags), ("the torch route differs", exact, wres)
    assert wlevels == res["levels"], ("the torch route ran other levels", wlevels, res["levels"])
    sres, sflags = scipy_route(a, entry, target, MAX_CUT)
    assert exact == sres and (cut.cpu().numpy() == sflags).all(), ("scipy differs", exact, sres)
    check_witness(a, entry, target, prev.cpu().numpy().view(np.uint16), nxt.cpu().numpy().view(np.uint16), res["n_paths"])
    del wflags

    def scipy_full():
        return scipy_route(unpack_host(mt.cpu().numpy().view(np.uint32), n), entry, target, MAX_CUT)
    legs = {
        "result": lambda: call(),
        "all": lambda: call(cut=True, paths=True),
        "torch": lambda: torch_route(mt, n, entry, target, MAX_CUT),
    }
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    t = {name: [] for name in legs}
    for _ in range(reps):  # alternating
        for name, fn in legs.items():
            t[name].append(event_ms(fn)[0])
    for name, fn in (("scipy", lambda: scipy_route(a, entry, target, MAX_CUT)), ("scipy_full", scipy_full)):
        t[name] = []
        for _ in range(max(2, reps // 2)):
            t0 = time.perf_counter()
            fn()
            t[name].append((time.perf_counter() - t0) * 1e3)
    best = {name: min(v) for name, v in t.items()}
    med = {name: statistics.median(v) for name, v in t.items()}
    # the launches of the call: the edges, the pairs, a level each, an augmentation each, the sets, the finish
    launches = 2 + res["levels"] + res["n_paths"] + (0 if res["capped"] or not res["separable"] else 2)
    return {"result": res, "launches": launches, "edges": int(a.sum()), "ms_best": best, "ms_median": med,
            "over_all": {k: v / best["all"] for k, v in best.items()},
            "over_all_median": {k: v / med["all"] for k, v in med.items()},
            "us_per_level": {k: 1e3 * best[k] / max(1, res["levels"]) for k in ("result", "all", "torch")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cut_bench needs the GPU"

    e = R.Engine(0)   # (the context only names the device: the call reads no table)
    res = {"tool": "cut_bench", "reps": a.reps, "n_entry": 8, "n_target": 8, "max_cut": MAX_CUT, "runs": {}}
    for side in a.sides:
        res.setdefault("plan", {})[str(side)] = e.debug_reach_cut_plan(side)
        for name, (g, entry, target) in (("random", random_graph(side, 3.0, 6)), ("layers", layers_graph(side))):
            mt = pack(g)
            torch.cuda.synchronize()
            res["runs"]["%s_%d" % (name, side)] = dict(measure(e, g, mt, side, entry, target, a.reps, a.warmup), input_bytes=mt.numel() * 4)
            del mt, g
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
