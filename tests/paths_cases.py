"""Query sets, expected paths and checks of the reachability-paths tests (test helper).

Shared by tests/test_paths_host.py (pg_debug_reach_paths_host, no GPU) and tests/test_gpu_paths.py
(pg_reach_paths on the device). Expected values come from numpy alone, never from the product:

Expected(hops) applies the least-predecessor rule of include/policygpu.h. For a graph of up to
TREE_MAX_N nodes it builds, per src i, the predecessor vector
    ((h[i][:, None] == h[i][None, :] - 1) & edges).argmax(0),   pred = i where hops is 1
(n^3 work over all srcs, 17 M at n = 257) and chases it for all queries at once, one numpy step per
path position; for a larger graph it answers the queries' own steps, ((h[src] == t - 1) & (hT[cur] ==
1)).argmax(1) over a block of queries, or, when the queries come from at most FEW_SRCS srcs, those srcs'
predecessor vectors built level by level (the same rule over the edges from level t - 1 to level t).
A step without a predecessor makes the query broken.

thresholds(e) finds the sizes at which the launch changes from pg_debug_reach_paths_plan alone;
check_few_sources runs eight srcs against every dst of a large closure, analytic_queries are queries of
the two cliques and the hub-last star whose paths are written down from the closed forms.

valid(...) checks a run on its own against an edge matrix that does not come from the hops (the codes
of a synthetic graph, the oracle's of an engine): p_0 = src, p_d = dst, d == hops, every step an edge,
the intermediates distinct and neither src nor dst, out_via == np.bincount of the intermediates, and the
result fields.

Every run prefills its outputs (the nodes with NODES_FILL, which is not 0xFFFF) and puts GUARD words
behind each that must stay untouched.
"""
import ctypes as C
import functools

import numpy as np

import closure_cases as cc
from vpp_amd import _capi
from vpp_amd._capi import lib

NONE = 0xFFFF
NODES_FILL = 0xEEEE
LEN_FILL = 0xDDDD
VIA_FILL = 0xFFFFFFFF
GUARD = 3
TREE_MAX_N = 300
FEW_SRCS = 16
OUTPUTS = ((True, True), (True, False), (False, True), (False, False))   # (nodes, via)


class Expected:
    def __init__(self, hops):
        self.h = np.ascontiguousarray(hops, np.uint16)
        self.n = self.h.shape[0]
        self.edges = self.h == 1
        self._pred, self._ht, self._tree = {}, None, None

    def pred(self, i):
        """the predecessor vector of src i, -1 where there is none"""
        if i not in self._pred:
            hi = self.h[i].astype(np.int32)
            if self.n <= TREE_MAX_N:
                mask = (hi[:, None] == hi[None, :] - 1) & self.edges
                p = mask.argmax(0)
                p[~mask.any(0)] = -1
            else:   # the same rule level by level: the edges from level t - 1 to level t alone
                p = np.full(self.n, -1, np.int64)
                for t in range(2, int(hi.max()) + 1):
                    ks, js = np.flatnonzero(hi == t - 1), np.flatnonzero(hi == t)
                    if len(ks) and len(js):
                        mask = self.edges[np.ix_(ks, js)]
                        p[js] = np.where(mask.any(0), ks[mask.argmax(0)], -1)
            p[hi == 1] = i
            self._pred[i] = p
        return self._pred[i]

    def tree(self):
        """pred of every src, [n, n]"""
        if self._tree is None:
            self._tree = np.stack([self.pred(i) for i in range(self.n)]) if self.n else np.zeros((0, 0), np.int64)
        return self._tree

    def step(self, src, cur, t):
        """p_{t-1} of the queries (src, ..) that stand at cur = p_t, -1 where there is none"""
        if self.n <= TREE_MAX_N:
            return self.tree()[src, cur]
        srcs = np.unique(src)
        if len(srcs) <= FEW_SRCS:   # a large graph queried from a few srcs: their predecessor vectors
            out = np.empty(len(src), np.int64)
            for i in srcs:
                out[src == i] = self.pred(int(i))[cur[src == i]]
            return out
        if self._ht is None:
            self._ht = np.ascontiguousarray(self.h.T)
        out = np.empty(len(src), np.int64)
        for b in range(0, len(src), 4096):
            s = slice(b, b + 4096)
            mask = (self.h[src[s]] == t - 1) & (self._ht[cur[s]] == 1)
            k = mask.argmax(1)
            out[s] = np.where(mask.any(1), k, -1)
        return out

    def walk(self, src, dst):
        """-> (d int64 [Q] (0: no path), P int64 [Q, max d + 1] (p_0 .. p_d, then -1), broken bool [Q])"""
        src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
        q = np.arange(len(src))
        d = self.h[src, dst].astype(np.int64) if len(src) else np.zeros(0, np.int64)
        dmax = int(d.max()) if len(src) else 0
        P = np.full((len(src), dmax + 1), -1, np.int64)
        P[q[d > 0], d[d > 0]] = dst[d > 0]
        broken = np.zeros(len(src), bool)
        for t in range(dmax, 1, -1):
            act = np.flatnonzero((d >= t) & ~broken)
            k = self.step(src[act], P[act, t], t)
            broken[act[k < 0]] = True
            P[act, t - 1] = k
        P[q[d > 0], 0] = src[d > 0]
        P[broken] = -1
        d = np.where(broken, 0, d)
        return d, P, broken

    def outputs(self, src, dst, max_len, nodes=True):
        """-> (lengths u16 [Q], nodes u16 [Q, max_len + 1], via u32 [n], result dict) as the call defines them"""
        d, P, broken = self.walk(src, dst)
        Q = len(d)
        rows = np.full((Q, max_len + 1), NONE, np.uint16)
        w = min(max_len + 1, P.shape[1])
        fits = (d > 0) & (d <= max_len)
        rows[fits, :w] = np.where(P[fits, :w] < 0, NONE, P[fits, :w]).astype(np.uint16)
        mid = P[:, 1:].copy()
        if Q:
            mid[np.arange(Q)[d > 0], d[d > 0] - 1] = -1   # (p_d is no intermediate)
        mid = mid[mid >= 0]
        via = np.bincount(mid, minlength=self.n).astype(np.uint32)
        raw = self.h[np.asarray(src, np.int64), np.asarray(dst, np.int64)] if Q else np.zeros(0, np.uint16)
        res = {"n_found": int((d > 0).sum()), "n_unreachable": int((raw == 0).sum()),
               "n_too_long": int(((d > max_len)).sum()) if nodes else 0, "n_broken": int(broken.sum()),
               "n_via": int(np.maximum(d - 1, 0).sum()), "longest": int(d.max()) if Q else 0}
        return d.astype(np.uint16), rows, via, res


def result_dict(res):
    return {k: getattr(res, k) for k in ("n_found", "n_unreachable", "n_too_long", "n_broken", "n_via", "longest")}


def buffers(nq, n, max_len):
    return (np.full(nq + GUARD, LEN_FILL, np.uint16), np.full(nq * (max_len + 1) + GUARD, NODES_FILL, np.uint16),
            np.full(n + GUARD, VIA_FILL, np.uint32))


def finish(nq, n, max_len, lbuf, nbuf, vbuf, res, nodes, via):
    """the guards of a run's buffers, and the run's return value"""
    assert (lbuf[nq:] == LEN_FILL).all() and (nbuf[nq * (max_len + 1):] == NODES_FILL).all() and (vbuf[n:] == VIA_FILL).all(), \
        "a guard was written"
    if not nodes:
        assert (nbuf == NODES_FILL).all()
    if not via:
        assert (vbuf == VIA_FILL).all()
    return (lbuf[:nq], nbuf[:nq * (max_len + 1)].reshape(nq, max_len + 1) if nodes else None, vbuf[:n] if via else None,
            result_dict(res))


def run_host(e, hops, n, src, dst, max_len, nodes=True, via=True):
    """pg_debug_reach_paths_host over prefilled outputs with guards -> (lengths u16 [Q], nodes u16 [Q,
    max_len + 1] or None, via u32 [n] or None, result dict)"""
    h = np.ascontiguousarray(hops, np.uint16)
    s, d = np.ascontiguousarray(src, np.uint32), np.ascontiguousarray(dst, np.uint32)
    nq = s.size
    lbuf, nbuf, vbuf = buffers(nq, n, max_len)
    spec = _capi.pg_reach_paths_spec(h.ctypes.data, n, s.ctypes.data, d.ctypes.data, nq, max_len)
    res = _capi.pg_reach_paths_result(77, 77, 77, 77, 77, 77)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    code = lib.pg_debug_reach_paths_host(e.h, C.byref(spec), p(lbuf), p(nbuf) if nodes else None, p(vbuf) if via else None,
                                         C.byref(res))
    assert code == 0, lib.pg_last_error(e.h)
    return finish(nq, n, max_len, lbuf, nbuf, vbuf, res, nodes, via)


def same(got, x, src, dst, max_len, what, via_defined=True):
    """a run's return value against Expected"""
    lens, rows, via, res = got
    wl, wr, wv, wres = x.outputs(src, dst, max_len, nodes=rows is not None)
    assert res == wres, (what, res, wres)
    assert (lens == wl).all(), (what, "lengths", np.flatnonzero(lens != wl)[:3].tolist())
    assert rows is None or (rows == wr).all(), (what, "nodes", np.argwhere(rows != wr)[:3].tolist())
    assert via is None or not via_defined or (via == wv).all(), (what, "via", np.flatnonzero(via != wv)[:3].tolist())


def valid(got, edges, hops, src, dst, max_len, what):
    """a run without a broken query, on its own against the edge matrix and the hop counts"""
    lens, rows, via, res = got
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    d = lens.astype(np.int64)
    assert (d == hops[src, dst]).all(), (what, "d != hops")
    found, fits = d > 0, (d > 0) & (d <= max_len)
    mids = []
    if rows is not None:
        r = rows.astype(np.int64)
        assert (r[~fits] == NONE).all(), (what, "a row without a path is not all 0xFFFF")
        q = np.flatnonzero(fits)
        assert (r[q, 0] == src[q]).all() and (r[q, d[q]] == dst[q]).all(), (what, "ends")
        pos = np.arange(r.shape[1])[None, :]
        on = pos <= d[q][:, None]
        assert (r[q][~on] == NONE).all() and (r[q][on] < edges.shape[0]).all(), (what, "tail")
        a, b = r[q][:, :-1], r[q][:, 1:]
        step = on[:, 1:]
        assert edges[a[step], b[step]].all(), (what, "a step is no edge")
        inner = (pos >= 1) & (pos < d[q][:, None])
        R = r[q]
        assert not (inner & ((R == src[q][:, None]) | (R == dst[q][:, None]))).any(), (what, "an intermediate is src or dst")
        srt = np.sort(np.where(inner, R, -1 - pos), axis=1)   # (what is no intermediate: a value of its own)
        assert (srt[:, 1:] != srt[:, :-1]).all(), (what, "an intermediate twice")
        mids = [R[inner]]
        if via is not None and fits.sum() == found.sum():
            want = np.bincount(np.concatenate(mids) if mids else np.zeros(0, np.int64), minlength=edges.shape[0])
            assert (via == want).all(), (what, "via != bincount")
    if via is not None:
        assert int(via.astype(np.int64).sum()) == res["n_via"] == int(np.maximum(d - 1, 0).sum()), (what, "n_via")
    assert res["n_found"] == int(found.sum()) and res["n_unreachable"] == int((~found).sum()) and res["n_broken"] == 0, (what, res)
    assert res["n_too_long"] == (int((d > max_len).sum()) if rows is not None else 0), (what, res)
    assert res["longest"] == (int(d.max()) if d.size else 0), (what, res)


# ---- query sets ----------------------------------------------------------------------------------
def all_pairs(n):
    i = np.arange(n, dtype=np.uint32)
    return np.repeat(i, n), np.tile(i, n)


def orders(n, chunk_queries, seed=0):
    """name -> (src, dst): all pairs sorted, shuffled and each twice; from one src chunk_queries - 1,
    chunk_queries and chunk_queries + 1 queries; one query per src"""
    g = np.random.default_rng([seed, n])
    s, d = all_pairs(n)
    perm = g.permutation(n * n)
    out = {"sorted": (s, d), "shuffled": (s[perm], d[perm]), "twice": (np.repeat(s, 2), np.repeat(d, 2))}
    i = n // 2
    for k in (chunk_queries - 1, chunk_queries, chunk_queries + 1):
        out["one src x %d" % k] = (np.full(k, i, np.uint32), (np.arange(k, dtype=np.uint32) * 7 + 3) % n)
    out["one per src"] = (g.permutation(n).astype(np.uint32), g.integers(0, n, n).astype(np.uint32))
    return out


def len_bounds(longest):
    return sorted({1} | {k for k in (longest - 1, longest, longest + 1) if k > 0})


def check(run, s, chunk_queries, variants=True):
    """`run(hops, n, src, dst, max_len, nodes=, via=)` (run_host's contract without the engine) over a
    closure_cases.Synthetic: the hops come from closure_cases.Expected, the edges from the codes"""
    n = s.n
    cx = s.expected()
    hops, edges = cx.hops, cx.edges
    x = Expected(hops)
    longest = max(1, cx.levels)
    sets = orders(n, chunk_queries)
    for name, (src, dst) in sets.items() if variants else [("sorted", sets["sorted"])]:
        got = run(hops, n, src, dst, longest)
        same(got, x, src, dst, longest, (s.family, n, name))
        valid(got, edges, hops, src, dst, longest, (s.family, n, name))
    if variants:
        src, dst = sets["shuffled"]
        for max_len in len_bounds(longest):
            got = run(hops, n, src, dst, max_len)
            same(got, x, src, dst, max_len, (s.family, n, "max_len", max_len))
            valid(got, edges, hops, src, dst, max_len, (s.family, n, "max_len", max_len))
        for nodes, via in OUTPUTS:
            same(run(hops, n, src, dst, max(1, longest - 1), nodes=nodes, via=via), x, src, dst, max(1, longest - 1),
                 (s.family, n, "outputs", nodes, via))
    return x


# ---- the pass boundary, depth, bounded and broken inputs -----------------------------------------
def star_hops(n):
    """hops of the star 0 <-> every other node"""
    h = np.full((n, n), 2, np.uint16)
    h[0, :] = h[:, 0] = 1
    h[0, 0] = 2
    return h


def two_cliques_hops(n):
    """hops of two cliques of half the nodes and one bridge from the first to the second"""
    return cc.Expected(np.where(cc.edges(n, "two-cliques", None), np.uint8(cc.ALLOW), np.uint8(0))[None]).hops


def boundary_graph(family, n):
    """(hops, edges) of the graphs of the pass-boundary tests"""
    if family == "hub-last":
        h = hub_last_hops(n)
        return h, h == 1
    h = star_hops(n) if family == "star" else two_cliques_hops(n)
    edges = cc.edges(n, family, None)
    assert ((h == 1) == edges).all()
    return h, edges


def hub_last_hops(n):
    """hops of the star whose hub is the last node: every two-edge path passes through node n - 1, the last
    bit of the last bit-word"""
    h = np.full((n, n), 2, np.uint16)
    h[n - 1, :] = h[:, n - 1] = 1
    h[n - 1, n - 1] = 2
    return h


def boundary_queries(hops, seed=0):
    """4096 random pairs and the pairs with an end in the last bit-word of a row whose least predecessor lies
    in that word -> (src, dst, the queries with an intermediate in the last word)"""
    n = hops.shape[0]
    g = np.random.default_rng([seed, n])
    src, dst = g.integers(0, n, 4096), g.integers(0, n, 4096)
    last = 32 * ((n - 1) // 32)
    x = Expected(hops)
    tail = np.arange(last, n)
    cs, cd = np.repeat(tail, n), np.tile(np.arange(n), len(tail))
    cs, cd = np.concatenate([cs, cd]), np.concatenate([cd, cs])   # both directions
    keep = hops[cs, cd] >= 2
    cs, cd = cs[keep][:20000], cd[keep][:20000]
    _, P, _ = x.walk(cs, cd)
    d = hops[cs, cd].astype(np.int64)
    hit = P[np.arange(len(cs)), d - 1] >= last
    src, dst = np.concatenate([src, cs[hit]]), np.concatenate([dst, cd[hit]])
    dd, P, _ = x.walk(src, dst)
    inner = (np.arange(P.shape[1])[None, :] >= 1) & (np.arange(P.shape[1])[None, :] < dd[:, None])
    return src.astype(np.uint32), dst.astype(np.uint32), int((inner & (P >= last)).any(axis=1).sum())


# ---- the plan's thresholds -------------------------------------------------------------------------
KIB48 = 48 * 1024   # the LDS a workgroup gets without asking for more


@functools.lru_cache(maxsize=None)
def thresholds(e):
    """from pg_debug_reach_paths_plan alone, {"via_48k", "via_lds", "row_48k"}: lds_bytes grows with n but for
    one drop, behind the last n whose out_via is counted in LDS (via_lds); via_48k is the last n up to there
    whose workgroup stays within 48 KiB, row_48k the last n beyond whose staged row does"""
    lds = np.array([e.debug_reach_paths_plan(n)["lds_bytes"] for n in range(1, (1 << 15) + 1)], np.int64)
    drops = np.flatnonzero(np.diff(lds) < 0) + 1   # (lds[k] belongs to n = k + 1)
    assert len(drops) == 1, drops
    b = int(drops[0])
    return {"via_48k": int(np.flatnonzero(lds[:b] <= KIB48).max()) + 1, "via_lds": b,
            "row_48k": b + int(np.flatnonzero(lds[b:] <= KIB48).max()) + 1}


THRESHOLDS = {"via_48k": 8156, "via_lds": 8192, "row_48k": 24472}   # today's


def few_sources(n, seed=0, k=8, also=()):
    """k srcs (node 0, node n - 1, one more of the last bit-word where it has one, those of `also`, the rest
    random) against every dst -> (src, dst) sorted by src, and a permutation of the queries"""
    g = np.random.default_rng([seed, n, k])
    last = 32 * ((n - 1) // 32)
    srcs = [0, n - 1, last + (n - 1 - last) // 2] + [int(i) for i in also]
    for i in g.permutation(n - 2) + 1:
        if len(set(srcs)) >= k:
            break
        srcs.append(int(i))
    srcs = np.array(sorted(set(srcs)), np.uint32)
    assert len(srcs) == k
    return np.repeat(srcs, n), np.tile(np.arange(n, dtype=np.uint32), k), g.permutation(k * n)


def check_few_sources(run, hops, edges, levels, outputs=False, one_block=None):
    """`run` (run_host's contract without the engine) over few_sources of a large closure (hops, levels) with
    the edge matrix it came from, one src a row of the greatest depth: sorted under max_len = levels, shuffled
    under levels - 1 (some paths are then too long); with `outputs` every output combination; `one_block`: a
    context manager under which the sorted set runs once more"""
    n = hops.shape[0]
    x = Expected(hops)
    src, dst, perm = few_sources(n, also=[int(hops.max(axis=1).argmax())])
    got = run(hops, n, src, dst, levels)
    same(got, x, src, dst, levels, (n, "sorted"))
    valid(got, edges, hops, src, dst, levels, (n, "sorted"))
    res = got[3]
    assert res["longest"] == levels >= 4 and res["n_too_long"] == 0 and res["n_via"] > 2 * res["n_found"], res
    assert (got[2] > 0).sum() > 256, "the paths meet in a few hubs, as a star's do"
    s, d = src[perm], dst[perm]
    got = run(hops, n, s, d, levels - 1)
    same(got, x, s, d, levels - 1, (n, "shuffled"))
    valid(got, edges, hops, s, d, levels - 1, (n, "shuffled"))
    assert got[3]["n_too_long"] > 0 and got[3]["n_via"] == res["n_via"] and (got[2] == x.outputs(src, dst, levels)[2]).all()
    if outputs:
        for nodes, via in OUTPUTS:
            same(run(hops, n, s, d, levels - 1, nodes=nodes, via=via), x, s, d, levels - 1, (n, "outputs", nodes, via))
    if one_block is not None:
        with one_block:
            same(run(hops, n, src, dst, levels), x, src, dst, levels, (n, "one workgroup per CU"))


def analytic_queries(family, n):
    """up to 64 queries of a two-cliques or hub-last graph of n >= 64 nodes with the path the least-predecessor
    rule gives (None: no path), written down from the graphs' closed forms -> [(src, dst, path)]"""
    last = 32 * ((n - 1) // 32)
    if family == "hub-last":
        hub = n - 1
        q = [(i, j, [i, hub, j]) for i, j in ((0, 1), (1, 0), (5, 5), (0, n - 2), (n - 2, 0), (last, last), (n - 2, n - 2),
                                              (n // 2, 7), (last, 3), (3, last))]
        # every node is a predecessor of the hub: the least one is node 0
        return q + [(hub, hub, [hub, 0, hub]), (hub, 4, [hub, 4]), (4, hub, [4, hub]), (0, hub, [0, hub]), (hub, 0, [hub, 0])]
    assert family == "two-cliques" and n - last >= 3 and n >= 64, (family, n)
    h = n // 2
    q = [(i, j, [i, h - 1, h, j]) for i, j in ((0, n - 1), (5, n - 2), (h - 2, last), (1, h + 1), (h - 2, n - 1), (17, last + 1))]
    q += [(h - 1, n - 1, [h - 1, h, n - 1]), (h - 1, h + 1, [h - 1, h, h + 1]), (0, h, [0, h - 1, h]), (h - 2, h, [h - 2, h - 1, h]),
          (h - 1, h, [h - 1, h])]
    # both ends in the last bit-word; a cycle goes through the least node of the clique
    q += [(n - 1, n - 2, [n - 1, n - 2]), (last, n - 1, [last, n - 1]), (n - 1, n - 1, [n - 1, h, n - 1]), (last, last, [last, h, last]),
          (h, h, [h, h + 1, h]), (0, 0, [0, 1, 0]), (3, 3, [3, 0, 3]), (h - 1, h - 1, [h - 1, 0, h - 1]), (2, 9, [2, 9])]
    return q + [(n - 1, 0, None), (h, h - 1, None), (last, 5, None), (n - 1, h - 1, None), (h + 1, 0, None)]


def check_analytic(got, n, queries, max_len):
    """a run over analytic_queries (every path fits max_len) against the paths written down there"""
    lens, rows, via, res = got
    paths = [p for _, _, p in queries]
    assert lens.tolist() == [len(p) - 1 if p else 0 for p in paths]
    assert rows.tolist() == [(p or []) + [NONE] * (max_len + 1 - len(p or [])) for p in paths]
    mids = [k for p in paths if p for k in p[1:-1]]
    assert (via == np.bincount(mids, minlength=n)).all(), np.flatnonzero(via != np.bincount(mids, minlength=n))[:3].tolist()
    found = [p for p in paths if p]
    assert res == {"n_found": len(found), "n_unreachable": len(paths) - len(found), "n_too_long": 0, "n_broken": 0,
                   "n_via": len(mids), "longest": max(len(p) - 1 for p in found)}, res


def ring_hops(n):
    i = np.arange(n)
    return (((i[None, :] - i[:, None] - 1) % n) + 1).astype(np.uint16)


RING_N = 2049
RING_QUERIES = (np.array([5, 5, 0], np.uint32), np.array([4, 5, 2048], np.uint32))
RING_LENGTHS = [2048, 2049, 2048]


def check_ring(run):
    h = ring_hops(RING_N)
    src, dst = RING_QUERIES
    lens, rows, via, res = run(h, RING_N, src, dst, 2049)
    assert lens.tolist() == RING_LENGTHS and res["n_found"] == 3 and res["n_too_long"] == 0 and res["longest"] == 2049, res
    for r, i, d in zip(rows.astype(np.int64), src, RING_LENGTHS):
        assert (r[:d + 1] == (int(i) + np.arange(d + 1)) % RING_N).all() and (r[d + 1:] == NONE).all()
    assert res["n_via"] == 2047 + 2048 + 2047 == int(via.astype(np.int64).sum())
    lens, rows, via2, res = run(h, RING_N, src, dst, 64)
    assert lens.tolist() == RING_LENGTHS and res["n_too_long"] == 3 and res["n_found"] == 3 and (rows == NONE).all()
    assert (via2 == via).all()


def broken_case(n=100, seed=11):
    """a closure's hops with one unreachable cell (i, j) set to 5 -> (hops, (i, j)). No k at level 4 of row
    i has an edge to j, or j were reachable: the first step of (i, j) finds nothing. The cell is chosen
    so that no other query changes: j at level 5 of row i could only be found by a query (i, x) of six
    edges with an edge j -> x."""
    s = cc.synthetic(n, "sparse", seed=seed)
    h = s.expected().hops.copy()
    g = np.random.default_rng(seed)
    for i, j in g.permutation(np.argwhere(h == 0)):
        if not ((h[j] == 1) & (h[i] == 6)).any():
            h[i, j] = 5
            return s, h, (int(i), int(j))
    raise AssertionError("no cell to break")


def check_broken(run):
    s, h, (i, j) = broken_case()
    n = s.n
    src, dst = all_pairs(n)
    x = Expected(h)
    got = run(h, n, src, dst, n)
    lens, rows, via, res = got
    q = i * n + j
    assert res["n_broken"] == 1 and lens[q] == 0 and (rows[q] == NONE).all()
    # Expected says which queries are broken: this one alone, and every other query is right
    same(got, x, src, dst, n, "broken", via_defined=False)
    _, _, broken = x.walk(src, dst)
    assert broken[q] and int(broken.sum()) == res["n_broken"] == 1


EINVAL_CASES = (
    # (what pg_last_error has to name, changes to a valid call)
    ("null spec", {"spec": None}), ("hops", {"hops": None}), ("out_len", {"out_len": None}), ("result", {"result": None}),
    ("src", {"src": None}), ("dst", {"dst": None}), ("2^15", {"n": (1 << 15) + 1}), ("2^24", {"n_queries": (1 << 24) + 1}),
    ("src[2]", {"src_at": (2, 4)}), ("dst[1]", {"dst_at": (1, 0xFFFFFFFF)}), ("max_len", {"max_len": 0}),
    ("max_len", {"max_len": (1 << 15) + 1}), ("2^32", {"n_queries": 1 << 24, "max_len": 255}),
)


def einval(call, ptr_hops, ptr_len, ptr_nodes):
    """`call(spec or None, out_len, out_nodes, out_via, with_result) -> (code, message)` over EINVAL_CASES;
    ptr_*: addresses of valid arrays of the side under test (hops 4 x 4, out_len 4, out_nodes 4 x 5)"""
    for what, ch in EINVAL_CASES:
        nq = ch.get("n_queries", 4)
        src = np.array([0, 1, 2, 3], np.uint32)
        dst = np.array([3, 2, 1, 0], np.uint32)
        # (a count beyond the arrays is refused before an id is read)
        if "src_at" in ch:
            src[ch["src_at"][0]] = ch["src_at"][1]
        if "dst_at" in ch:
            dst[ch["dst_at"][0]] = ch["dst_at"][1]
        spec = _capi.pg_reach_paths_spec(ch.get("hops", ptr_hops), ch.get("n", 4), ch.get("src", src.ctypes.data),
                                         ch.get("dst", dst.ctypes.data), nq, ch.get("max_len", 4))
        code, msg = call(None if "spec" in ch else spec, ch.get("out_len", ptr_len), ptr_nodes, None, "result" not in ch)
        assert code == _capi.PG_EINVAL, (what, code)
        assert what in msg, (what, msg)
