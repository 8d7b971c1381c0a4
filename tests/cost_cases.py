"""Graphs, references and checkers of the reachability-cost tests (test helper).

Shared by tests/test_cost_host.py (pg_debug_reach_cost_host, no GPU) and tests/test_gpu_cost.py
(pg_reach_cost on the device). Packing is closure_cases' (every edge ALLOW in one random slice, the other
cells random codes from {0, 1, 3}, random padding bits).

References, none of them from the product:
  brute(a, w, s)      every simple walk from s, enumerated (n <= 7): cost, and from the definition alone
                      pred, len and via.
  reference(a, w, S)  a heap Dijkstra over adjacency lists for base(s, .) -- edge (p -> v) weighted w[v],
                      base(s, s) = 0 -- then one step over the edge list for all of cost and pred: cost(s, v) = min
                      over p -> v of base(s, p) + w[v], the diagonal included, pred the least p that
                      attains it. tests/test_cost_host.py pins it to brute() and to
                      scipy.sparse.csgraph.dijkstra (costs below 2^31 are exact in float64).
  by_scipy(a, w, S)   the same with scipy's Dijkstra for base: the large graphs.
An Answer holds cost and pred without a bound; at(max_cost) filters them (a cell above the bound is not
reached; the cheapest walk to a cell within the bound stays within it) and follows the predecessors of the
reached cells for len and via, all paths of a source at once.

Families (graph(n, family)): chain (i -> i + 1, one source: n - 1 rounds), ring (a ring with the chord
0 -> n // 2), detour (gadgets of 7 end points in a row: a route of two cheap intermediates beside a route of
one dear intermediate -- the cheapest is not the shortest -- and two tying predecessors, so that "least p"
decides; the last end point of a gadget closes a cycle to its first), islands (five islands with random
edges inside and a bridge to the next, closure_cases' placement from 480 end points on, weights by
island), random4 (4 random edges per end point, weights 1..9), layers (complete edges between consecutive
layers, a weight per layer: layers_want writes the answer down).
"""
import ctypes as C
import heapq

import numpy as np

import closure_cases as cc
import cut_cases as ct
import diff_cases as dc
from vpp_amd import _capi
from vpp_amd._capi import lib

ALLOW = cc.ALLOW
NONE, NO_PRED = 0xFFFFFFFF, 0xFFFF
GUARD = cc.GUARD
SIZES = (1, 2, 31, 32, 33, 64, 65, 127, 128, 129, 300, 2049)
FAMILIES = ("chain", "ring", "detour", "islands", "random4", "layers")
FILLS = (0xEEEEEEEE, 0xDDDD, 0xCCCC, 0xBBBBBBBB)   # cost, pred, len, via
RESULT_FIELDS = ("n_reached", "n_via", "max_cost", "longest")
OUTPUTS = tuple((c, p, l, v) for c in (True, False) for p in (True, False) for l in (True, False) for v in (True, False))


# ---- graphs ----------------------------------------------------------------------------------------
GADGET = 7   # s, h (dear), a, b (cheap, tying), c, t, u
GADGET_EDGES = ((0, 1), (1, 5), (0, 3), (0, 2), (2, 4), (3, 4), (4, 5), (5, 6), (6, 0))
GADGET_WEIGHTS = (3, 5, 1, 1, 1, 2, 1)


def layer_widths(n):
    """up to five layers that add up to n, the first of them narrow"""
    if n < 6:
        return [1] * n
    first = min(3, n // 6)
    rest = n - first
    return [first, rest // 4, rest // 4, rest // 4, rest - 3 * (rest // 4)]


LAYER_WEIGHTS = (7, 2, 65535, 1, 3)


def island_layout(n):
    """(starts, size) of the five islands of n end points"""
    if n >= 2 * cc.ISLANDS * cc.ISLAND:
        return cc.island_starts(n), cc.ISLAND
    size = n // cc.ISLANDS
    return [k * size for k in range(cc.ISLANDS)], size


def family(n, name, seed=0):
    """-> (a bool [n, n], weights u16 [n], sources)"""
    g = np.random.default_rng([seed, n, FAMILIES.index(name), 77])
    a = np.zeros((n, n), bool)
    w = np.ones(n, np.uint16)
    i = np.arange(n)
    if name == "chain":
        a[i[:-1], i[1:]] = True
        w = (1 + i % 3).astype(np.uint16)
        src = [0]
    elif name == "ring":
        a[i, (i + 1) % n] = True
        a[0, n // 2] = True
        w[:] = 3
        src = sorted({0, n // 3, n - 1})
    elif name == "detour":
        for o in range(0, n, GADGET):
            for u, v in GADGET_EDGES:
                if o + u < n and o + v < n:
                    a[o + u, o + v] = True
            if o + GADGET < n:
                a[o + GADGET - 1, o + GADGET] = True   # on to the next gadget
            w[o:o + GADGET] = GADGET_WEIGHTS[:n - o]
        src = sorted({0, (n // 2) // GADGET * GADGET, n - 1})
    elif name == "islands":
        starts, size = island_layout(n)
        w[:] = 7
        for k, s in enumerate(starts):
            a[s:s + size, s:s + size] = g.random((size, size)) < 3.0 / max(size, 1)
            w[s:s + size] = k + 1
            if k and size:
                a[starts[k - 1] + size - 1, s] = True
        src = sorted({0, starts[1], starts[2] + size // 2, n - 1})
    elif name == "random4":
        a = g.random((n, n)) < 4.0 / n
        w = g.integers(1, 10, n).astype(np.uint16)
        src = sorted(set(int(x) for x in g.integers(0, n, 4)))
    else:
        assert name == "layers", name
        widths = layer_widths(n)
        at = np.concatenate([[0], np.cumsum(widths)])
        for k in range(len(widths) - 1):
            a[at[k]:at[k + 1], at[k + 1]:at[k + 2]] = True
            w[at[k]:at[k + 1]] = LAYER_WEIGHTS[k]
        w[at[-2]:] = LAYER_WEIGHTS[len(widths) - 1]
        src = sorted({0, widths[0] - 1})
    return a, w, src


def layers_want(widths, weights, s):
    """the answer for a source s of the first layer of a layers graph, by construction: layer k costs the
    weights of layers 1..k, is k edges away, and its predecessor is the first end point of layer k - 1 (s for
    layer 1); the first end point of every layer between is crossed by every path to a later layer.
    -> (cost u32 [n], pred u16 [n], len u16 [n], via u32 [n])"""
    n = sum(widths)
    at = np.concatenate([[0], np.cumsum(widths)])
    cost, pred = np.full(n, NONE, np.uint32), np.full(n, NO_PRED, np.uint16)
    ln, via = np.zeros(n, np.uint16), np.zeros(n, np.uint32)
    for k in range(1, len(widths)):
        cost[at[k]:at[k + 1]] = sum(int(weights[j]) for j in range(1, k + 1))
        pred[at[k]:at[k + 1]] = s if k == 1 else at[k - 1]
        ln[at[k]:at[k + 1]] = k
        if k + 1 < len(widths):
            via[at[k]] = n - at[k + 1]
    return cost, pred, ln, via


def pack(a, n_svc=3, seed=0):
    """-> (codes u8 [n_svc, n, n], words u32 [n_svc, n, row_words(n)]) as closure_cases.Synthetic makes them"""
    n = a.shape[0]
    g = np.random.default_rng([seed, n, n_svc, 78])
    owner = g.integers(0, n_svc, (n, n), dtype=np.uint8)
    other = np.array([0, 1, 3], np.uint8)[g.integers(0, 3, (n_svc, n, n), dtype=np.uint8)]
    codes = np.where(a[None] & (owner[None] == np.arange(n_svc)[:, None, None]), np.uint8(ALLOW), other)
    words = np.stack([dc.garbage(dc.pack_wide(codes[v]), n, seed + 1 + v) for v in range(n_svc)])
    return codes, words


class Case:
    def __init__(self, n, name, n_svc=3, seed=0):
        self.n, self.family, self.n_svc = n, name, n_svc
        self.a, self.w, self.src = family(n, name, seed)
        self.codes, self.words = pack(self.a, n_svc, seed)

    def edges(self, select=None):
        sel = list(range(self.n_svc)) if select is None else list(select)
        return (self.codes[sel] == ALLOW).any(axis=0) if sel else np.zeros((self.n, self.n), bool)


# ---- references ------------------------------------------------------------------------------------
class Answer:
    """cost u32 [k, n] (NONE where no walk exists) and pred u16 [k, n] of the sources `src`, without a bound"""

    def __init__(self, src, cost, pred):
        self.src, self.cost, self.pred = list(src), np.asarray(cost, np.uint32), np.asarray(pred, np.uint16)

    def at(self, max_cost=0):
        """-> (cost, pred, len u16 [k, n], via u32 [n], result dict) under max_cost"""
        k, n = self.cost.shape
        reached = self.cost != NONE
        if max_cost:
            reached &= self.cost <= max_cost
        cost = np.where(reached, self.cost, np.uint32(NONE))
        pred = np.where(reached, self.pred, np.uint16(NO_PRED))
        ln, via = np.zeros((k, n), np.uint16), np.zeros(n, np.uint32)
        for q, s in enumerate(self.src):
            # every path of the source one step at a time: `cur` is the end point the path has come back to
            on = np.flatnonzero(reached[q])
            cur = pred[q, on].astype(np.int64)
            ln[q, on] = 1
            for _ in range(n + 1):
                go = cur != s
                if not go.any():
                    break
                on, cur = on[go], cur[go]
                assert reached[q, cur].all(), "a path leaves the reached cells"
                np.add.at(via, cur, 1)
                ln[q, on] += 1
                cur = pred[q, cur].astype(np.int64)
            else:
                raise AssertionError("a path does not end")
        res = {"n_reached": int(reached.sum()), "n_via": int(via.sum()), "max_cost": int(cost[reached].max()) if reached.any() else 0,
               "longest": int(ln.max()) if ln.size else 0}
        assert res["n_via"] == int(ln.astype(np.int64).sum()) - res["n_reached"]
        return cost, pred, ln, via, res


def from_base(a, w, src, base):
    """the last step, over the edge list: cost and pred of every cell from base float64 [k, n] (inf where not
    defined)"""
    n = a.shape[0]
    rows, cols = np.nonzero(a)
    cost, pred = np.full((len(src), n), NONE, np.uint32), np.full((len(src), n), NO_PRED, np.uint16)
    for q in range(len(src)):
        cand = base[q][rows] + w[cols].astype(np.float64)
        best = np.full(n, np.inf)
        np.minimum.at(best, cols, cand)
        tie = np.isfinite(cand) & (cand == best[cols])
        least = np.full(n, n, np.int64)
        np.minimum.at(least, cols[tie], rows[tie])
        ok = np.isfinite(best)
        cost[q, ok] = best[ok].astype(np.uint32)
        pred[q, ok] = least[ok]
    return Answer(src, cost, pred)


def base_heap(a, w, s):
    """Dijkstra from s with a heap: base(s, .) as float64, inf where there is no walk; base(s, s) = 0"""
    n = a.shape[0]
    rows, cols = np.nonzero(a)
    start = np.searchsorted(rows, np.arange(n + 1))
    base = np.full(n, np.inf)
    base[s] = 0.0
    heap = [(0.0, s)]
    while heap:
        d, p = heapq.heappop(heap)
        if d > base[p]:
            continue
        for v in cols[start[p]:start[p + 1]]:
            nd = d + float(w[v])
            if nd < base[v]:
                base[v] = nd
                heapq.heappush(heap, (nd, int(v)))
    return base


def reference(a, w, src):
    return from_base(a, w, src, np.stack([base_heap(a, w, s) for s in src]) if len(src) else np.zeros((0, a.shape[0])))


def by_scipy(a, w, src):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    rows, cols = np.nonzero(a)
    keep = rows != cols   # (a self edge never shortens base; the dense step sees it)
    m = csr_matrix((w[cols[keep]].astype(np.float64), (rows[keep], cols[keep])), shape=a.shape)
    return from_base(a, w, src, dijkstra(m, directed=True, indices=list(src)).reshape(len(src), a.shape[0]))


def brute(a, w, s):
    """every simple walk from s (no end point twice, but it may end in s): -> (cost, pred, len, via) of the
    source, each from the definition"""
    n = a.shape[0]
    best = {}

    def walk(u, seen, c):
        for v in np.flatnonzero(a[u]):
            v = int(v)
            if v in seen and v != s:
                continue
            cv = c + int(w[v])
            best[v] = min(best.get(v, cv), cv)
            if v != s:
                walk(v, seen | {v}, cv)
    walk(s, {s}, 0)
    base = lambda p: 0 if p == s else best.get(p)
    cost, pred = np.full(n, NONE, np.uint32), np.full(n, NO_PRED, np.uint16)
    ln, via = np.zeros(n, np.uint16), np.zeros(n, np.uint32)
    for v, c in best.items():
        cost[v] = c
        pred[v] = min(p for p in range(n) if a[p, v] and base(p) is not None and base(p) + int(w[v]) == c)
    for v in best:
        p, steps = int(pred[v]), 1
        while p != s:
            via[p] += 1
            p, steps = int(pred[p]), steps + 1
            assert steps <= n
        ln[v] = steps
    return cost, pred, ln, via


SMALL_WEIGHTS = np.array([1, 2, 3, 65535], np.uint16)


def small_cases():
    """a sample of the graphs of up to 4 end points and random ones of 5 to 7, weights from {1, 2, 3, 65535}:
    (a, w)"""
    g = np.random.default_rng(5)
    for n in (1, 2, 3, 4):
        for bits in range(0, 1 << (n * n), 1 if n < 3 else 5 if n == 3 else 331):
            yield np.array([(bits >> k) & 1 for k in range(n * n)], bool).reshape(n, n), SMALL_WEIGHTS[g.integers(0, 4, n)]
    for n in (5, 6, 7):
        for _ in range(40):
            yield g.random((n, n)) < g.choice([0.2, 0.35, 0.5]), SMALL_WEIGHTS[g.integers(0, 4, n)]


def all_graphs(n):
    """all 2^(n * n) graphs of n <= 4 end points at once, graph b with edge (i, j) at bit i * n + j of b and weights
    from {1, 2, 3, 65535} by b: -> (a bool [G, n, n], w u16 [G, n])"""
    b = np.arange(1 << (n * n), dtype=np.int64)
    a = ((b[:, None] >> np.arange(n * n)) & 1).astype(bool).reshape(-1, n, n)
    w = SMALL_WEIGHTS[((b[:, None] * 2654435761 >> (7 + 2 * np.arange(n))) & 3)]
    return a, w


def brute_all(a, w):
    """brute() for every graph of all_graphs and every source at once: the simple walks are enumerated as
    sequences of end points, each tested against all graphs. -> (cost [G, n, n], pred, len as int64 with NONE /
    NO_PRED / 0, via [G, n] summed over the graph's n sources)"""
    G, n = w.shape
    INF = np.int64(1) << 40
    wl = w.astype(np.int64)
    cost = np.full((G, n, n), INF)

    def extend(s, seq, ok, c):
        for v in range(n):
            if v in seq[1:]:   # (v == s ends the walk in a cycle)
                continue
            step = ok & a[:, seq[-1], v]
            cv = c + wl[:, v]
            cost[:, s, v] = np.where(step, np.minimum(cost[:, s, v], cv), cost[:, s, v])
            if v != s:
                extend(s, seq + [v], step, cv)
    for s in range(n):
        extend(s, [s], np.ones(G, bool), np.zeros(G, np.int64))
    reached = cost < INF
    idx = np.arange(G)
    pred = np.full((G, n, n), NO_PRED, np.int64)
    for s in range(n):
        for v in range(n):
            for p in range(n - 1, -1, -1):
                base = np.zeros(G, np.int64) if p == s else cost[:, s, p]
                hit = reached[:, s, v] & a[:, p, v] & (base < INF) & (base + wl[:, v] == cost[:, s, v])
                pred[:, s, v] = np.where(hit, p, pred[:, s, v])
    assert ((pred != NO_PRED) == reached).all()
    ln, via = np.zeros((G, n, n), np.int64), np.zeros((G, n), np.int64)
    for s in range(n):
        for v in range(n):
            on = reached[:, s, v].copy()
            cur = np.where(on, pred[:, s, v], s)
            ln[:, s, v] = on
            for _ in range(n):
                on &= cur != s
                np.add.at(via, (idx[on], cur[on]), 1)
                ln[:, s, v] += on
                cur = np.where(on, pred[idx, s, np.minimum(cur, n - 1)], s)
            assert not (on & (cur != s)).any()
    return np.where(reached, cost, NONE), pred, ln, via


def union_words(a):
    """the packed words u32 [1, G * n, row_words(G * n)] of the disjoint union of the graphs a bool [G, n, n]:
    ALLOW on the edges, DENY_SYN elsewhere"""
    G, n = a.shape[:2]
    g, i, j = np.nonzero(a)
    rows, cols = g * n + i, g * n + j
    words = np.zeros((G * n, cc.row_words(G * n)), np.uint32)
    np.bitwise_or.at(words, (rows, cols // 16), (np.uint32(ALLOW) << (2 * (cols % 16)).astype(np.uint32)))
    return words[None]


# ---- runs ------------------------------------------------------------------------------------------
def result_dict(res):
    return {k: getattr(res, k) for k in RESULT_FIELDS}


def spec_of(matrix_ptr, n, n_svc, src, w, max_cost=0, select=None):
    """pg_reach_cost_spec -> (spec, the arrays it points into)"""
    s = np.ascontiguousarray(src, np.uint32)
    wt = np.ascontiguousarray(w, np.uint16)
    f = cc.flags(select, n_svc)
    return _capi.pg_reach_cost_spec(matrix_ptr, n, n_svc, f.ctypes.data if f is not None else None, s.ctypes.data if len(s) else None,
                                    len(s), wt.ctypes.data if len(wt) else None, max_cost), (s, wt, f)


def buffers(k, n):
    return (np.full(k * n + GUARD, FILLS[0], np.uint32), np.full(k * n + GUARD, FILLS[1], np.uint16),
            np.full(k * n + GUARD, FILLS[2], np.uint16), np.full(n + GUARD, FILLS[3], np.uint32))


def finish(k, n, bufs, res, given):
    """the guards of a run's buffers -- behind what was given, and all of what was not -- and its return value"""
    out = []
    for i, (buf, fill, on) in enumerate(zip(bufs, FILLS, given)):
        size = n if i == 3 else k * n
        assert (buf[size if on else 0:] == fill).all(), "a guard was written"
        out.append(None if not on else buf[:n] if i == 3 else buf[:size].reshape(k, n))
    return tuple(out) + (result_dict(res),)


def run_host(e, words, n, src, w, max_cost=0, select=None, cost=True, pred=True, len=True, via=True):
    """pg_debug_reach_cost_host over prefilled outputs with guards -> (cost u32 [k, n], pred u16 [k, n], len u16
    [k, n], via u32 [n], result dict), None for what was not asked for"""
    m = np.ascontiguousarray(words, np.uint32)
    n_svc = m.size // (n * cc.row_words(n))
    given = (cost, pred, len, via)
    bufs = buffers(np.size(src), n)
    spec, keep = spec_of(m.ctypes.data, n, n_svc, src, w, max_cost, select)
    res = _capi.pg_reach_cost_result(77, 77, 77, 77)
    p = lambda x, on: x.ctypes.data_as(C.c_void_p) if on else None
    code = lib.pg_debug_reach_cost_host(e.h, C.byref(spec), *[p(b, on) for b, on in zip(bufs, given)], C.byref(res))
    assert code == 0, lib.pg_last_error(e.h)
    del keep
    return finish(np.size(src), n, bufs, res, given)


def same(got, want, what):
    """a run's return value against an Answer.at(..)"""
    for name, x, y in zip(("cost", "pred", "len", "via"), got[:4], want[:4]):
        assert x is None or (x == y).all(), (what, name, np.argwhere(x != y)[:3].tolist())
    assert got[4] == want[4], (what, got[4], want[4])


def invariants(got, a, w, src, what):
    """what holds of any right answer, from the four outputs alone"""
    cost, pred, ln, via, res = got
    n = a.shape[0]
    for q, s in enumerate(src):
        on = np.flatnonzero(cost[q] != NONE)
        assert ((pred[q] != NO_PRED) == (cost[q] != NONE)).all() and ((ln[q] != 0) == (cost[q] != NONE)).all(), what
        p = pred[q, on].astype(np.int64)
        assert (p < n).all() and a[p, on].all(), (what, "a predecessor without an edge")
        first = p == s
        assert (cost[q, p[~first]] != NONE).all(), what
        base = np.where(first, 0, cost[q, p]).astype(np.int64)
        assert (cost[q, on] == base + w[on]).all(), (what, "cost = base(pred) + weight")
        assert (ln[q, on] == np.where(first, 0, ln[q, p]) + 1).all(), (what, "len = len(pred) + 1")
    reached = cost != NONE
    total = int(ln.astype(np.int64).sum()) - int(reached.sum())
    assert int(via.sum()) == total == res["n_via"] and res["n_reached"] == int(reached.sum()), (what, res)
    assert res["max_cost"] == (int(cost[reached].max()) if reached.any() else 0) and res["longest"] == (int(ln.max()) if ln.size else 0), (what, res)


def bounds(x):
    """the max_cost values of a check: 1, the median and the largest cost, and one below it"""
    cost = x.cost[x.cost != NONE]
    if not cost.size:
        return [1]
    return sorted({1, int(np.median(cost)), int(cost.max()), max(1, int(cost.max()) - 1)})


def check(run, words, s, variants=True):
    """`run(words, n, src, w, max_cost, select, cost=, pred=, len=, via=)` (run_host's contract without the
    engine) against reference() on the case s"""
    n = s.n
    x = reference(s.a, s.w, s.src)
    full = run(words, n, s.src, s.w)
    same(full, x.at(), (n, s.family))
    invariants(full, s.a, s.w, s.src, (n, s.family))
    for b in bounds(x) if variants else bounds(x)[-2:-1]:
        got = run(words, n, s.src, s.w, b)
        same(got, x.at(b), (n, s.family, "max_cost", b))
        invariants(got, s.a, s.w, s.src, (n, s.family, "max_cost", b))
    if not variants:
        return full
    for sel in ((0,), (0, s.n_svc - 1), ()):
        same(run(words, n, s.src, s.w, 0, sel), reference(s.edges(sel), s.w, s.src).at(), (n, s.family, "select", sel))
    b = bounds(x)[len(bounds(x)) // 2]
    for given in OUTPUTS[1:]:
        c, p, l, v = given
        same(run(words, n, s.src, s.w, 0, None, cost=c, pred=p, len=l, via=v), x.at(), (n, s.family, "outputs", given))
        same(run(words, n, s.src, s.w, b, None, cost=c, pred=p, len=l, via=v), x.at(b), (n, s.family, "outputs, bounded", given))
    return full


# ---- large layers, sizes from the plan ---------------------------------------------------------------
def large_layers(n):
    """(widths, weights, words [1, n, row_words(n)], the four sources) of a layers graph of n >= 400 end points
    without n x n codes"""
    widths = [4, 40, 5, n - 100, 5, 43, 3]
    return widths, (9, 7, 2, 65535, 1, 3, 4), ct.layers_words(widths), (0, 3, 1, 3)


def check_large_layers(run, n, made=None):
    widths, weights, words, src = made or large_layers(n)
    w = np.repeat(np.array(weights, np.uint16), widths)
    got = run(words, n, src, w)
    rows = [layers_want(widths, weights, s) for s in src]
    for q in range(len(src)):
        for name, x, y in zip(("cost", "pred", "len"), got[:3], rows[q][:3]):
            assert (x[q] == y).all(), (n, q, name)
    assert (got[3] == sum(r[3].astype(np.int64) for r in rows)).all(), n
    reached = len(src) * (n - widths[0])
    assert got[4] == {"n_reached": reached, "n_via": int(got[3].sum()), "max_cost": sum(weights[1:]), "longest": len(widths) - 1}, got[4]
    return got


def first_n(plan, test, lo=0, hi=1 << 15):
    """the least n in (lo, hi] at which test(plan(n)) holds, given that it does not at lo, does at hi and changes
    once between"""
    assert not test(plan(lo)) and test(plan(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if test(plan(mid)) else (mid, hi)
    return hi


# ---- the Engine wrapper on the chain policy ----------------------------------------------------------
WRAPPER_WEIGHTS = {"ns/c5": 9, "ns/c3": 4, "ns/c9": 2, "ns/c10": 65535}
WRAPPER_CASES = ((cc.CHAIN_PODS, ["ns/c0"], 0), (cc.CHAIN_PODS[::-1], ["ns/c2", "ns/c11"], 0), (cc.CHAIN_PODS, ["ns/c0", "ns/c0"], 6),
                 (cc.CHAIN_PODS[3:], ["ns/c4"], 0), (cc.CHAIN_PODS, [], 0))


def check_wrapper(c, host=False):
    """Engine.reachability_cost on a closure_cases.Chain against reference() on the oracle's codes"""
    for pods, src, max_cost in WRAPPER_CASES:
        routes, chokes, res = c.e.reachability_cost(pods, cc.CHAIN_SERVICES, src, WRAPPER_WEIGHTS, max_cost, host=host)
        at = [cc.CHAIN_PODS.index(p) for p in pods]
        a = (c.codes == ALLOW).any(axis=0)[np.ix_(at, at)]
        w = np.array([WRAPPER_WEIGHTS.get(p, 1) for p in pods], np.uint16)
        ids = [pods.index(p) for p in src]
        cost, pred, ln, via, want = reference(a, w, ids).at(max_cost)
        assert res == want and len(routes) == len(src), (res, want)
        for q in range(len(ids)):
            assert set(routes[q]) == {pods[v] for v in np.flatnonzero(cost[q] != NONE)}, (pods, src, q)
            for pod, (cst, path) in routes[q].items():
                walk = [pods.index(p) for p in path]
                assert cst == cost[q, walk[-1]] == int(w[walk[1:]].astype(np.int64).sum()) and len(path) == ln[q, walk[-1]] + 1
                assert walk[0] == ids[q] and pods[walk[-1]] == pod and all(a[u, v] for u, v in zip(walk, walk[1:])), path
        order = sorted((k for k in range(len(pods)) if via[k]), key=lambda k: (-int(via[k]), k))
        assert chokes == [(pods[k], int(via[k])) for k in order], (chokes, via)
    if len(WRAPPER_CASES):
        assert res == dict.fromkeys(RESULT_FIELDS, 0)   # (the last case has no source)


# ---- the arguments ---------------------------------------------------------------------------------
def bad_specs(ptr):
    """(spec, with result, what pg_last_error has to name) of every PG_EINVAL of the contract; the arrays the
    specs point into"""
    S = _capi.pg_reach_cost_spec
    ids = np.array([1, 2, 4, 3], np.uint32)
    w = np.array([1, 2, 3, 0], np.uint16)
    many = np.zeros((1 << 15) + 1, np.uint32)
    wide = np.ones(1 << 15, np.uint16)
    ip, wp, mp, big = ids.ctypes.data, w.ctypes.data, many.ctypes.data, (1 << 15) + 1
    return [(None, True, "spec"), (S(ptr, 3, 1, None, ip, 2, wp, 0), False, "result"), (S(None, 3, 1, None, ip, 2, wp, 0), True, "matrix"),
            (S(ptr, 3, 1, None, None, 2, wp, 0), True, "src"), (S(ptr, 3, 1, None, ip, 2, None, 0), True, "weight"),
            (S(ptr, big, 1, None, ip, 2, wp, 0), True, "n: more"), (S(ptr, 3, 1, None, mp, big, wp, 0), True, "n_src: more"),
            (S(ptr, 1 << 15, 1, None, mp, 1 << 13, wide.ctypes.data, 0), True, "n_src * n"),
            (S(ptr, 3, 0, None, ip, 2, wp, 0), True, "n_svc"), (S(ptr, 3, 4097, None, ip, 2, wp, 0), True, "n_svc"),
            (S(ptr, 3, 1, None, ip, 3, wp, 0), True, "src[2]"), (S(ptr, 4, 1, None, ip, 2, wp, 0), True, "weight[3]")], (ids, w, many, wide)
