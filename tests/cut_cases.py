"""Graphs, entry / target sets and expected answers of the reachability-cut tests (test helper).

Shared by tests/test_cut_host.py (pg_debug_reach_cut_host, no GPU) and tests/test_gpu_cut.py (pg_reach_cut
on the device). Expected values come from numpy / Python / scipy alone and never from the product.

Three references, each -> Answer (n_direct, the cut size, near, far and the two Reach sets as bool [n]):
  brute(a, E, T)    the definition, for n <= 12: the subsets of the end points outside E u T by size; the
                    first size with a separating one gives the minimum cuts; near is the one whose retained
                    region lies inside every other's, far the one whose region that still reaches T does;
                    that exactly one cut qualifies is asserted.
  flow(a, E, T)     a plain-Python augmenting-path maximum flow (depth first, so not the product's order) on
                    the split graph, then the residual rule: near = in half residual-reachable from the source
                    and out half not, far = out half residual-reaches the sink and in half not; the Reach
                    sets by plain searches without the cut.
  flow_scipy(...)   scipy.sparse.csgraph.maximum_flow on the same split graph, residual reachability in
                    numpy; for the large graphs. tests/test_cut_host.py pins it to flow().
Answer.at(max_cut) gives what the call has to report under a bound: capped when the cut is larger.

The witness is not unique, so check_witness validates it: exactly n_paths chains, each from an entry over
existing selected edges to a target, interiors outside E u T and pairwise disjoint, 0xFFFF off the paths.

Inputs: the families of closure_cases (imported, not edited) and four families with written-down answers
(known()):
  layers     consecutive fully connected layers, E the first and T the last: cut_size the least interior
             width, near the first interior layer of that width, far the last.
  hourglass  two cliques sharing k end points, E = {0}, T = {n - 1}: both cuts are the shared end points.
  grid       an r x c grid with edges to the right and downwards, E the left column, T the right one:
             cut_size r, near column 1, far column c - 2.
  zigzag     gadgets of 8 end points e, a, d, t, b1, b2, c1, c2 with e -> a -> d -> t, a -> b1 -> b2 -> t
             and e -> c1 -> c2 -> d: the unique shortest first route e, a, d, t takes the d that the only
             second route needs, so the second augmentation has to cancel flow: cut_size 2 per gadget and
             reroutes > 0.
Every edge is given to one random slice, the other cells hold random codes from {0, 1, 3}, and the padding
bits are random, as closure_cases.Synthetic does.
"""
import ctypes as C
import functools
import itertools

import numpy as np

import closure_cases as cc
import diff_cases as dc
import dominators_cases as dm
from vpp_amd import _capi
from vpp_amd._capi import lib

ALLOW = cc.ALLOW
SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
SMALL_SIZES = (3, 4, 5, 6, 7, 8, 9, 12)   # where the definition runs by brute force
NEW_FAMILIES = ("layers", "hourglass", "grid", "zigzag")
FAMILIES = cc.FAMILIES + NEW_FAMILIES
GUARD = cc.GUARD
NO_HOP, NO_CUT = 0xFFFF, 0xFFFFFFFF
NEAR, FAR, NEAR_REACH, FAR_REACH = 1, 2, 4, 8
EXACT = ("separable", "capped", "n_direct", "cut_size", "n_paths", "near_reach", "far_reach")
RESULT_FIELDS = EXACT + ("levels", "reroutes")
SCIPY_FROM = 130   # expected() takes flow() below and flow_scipy() from here on
LARGE = 1 << 15    # a max_cut that never caps


# ---- the new families ----------------------------------------------------------------------------
def layer_widths(n):
    """E, interior layers, T: below 15 end points one per layer"""
    return [1] * n if n < 15 else [1, 3, 2, n - 13, 2, 4, 1]


def grid_shape(n):
    r = max(1, int(np.sqrt(n)) // 2)
    return r, n // r


GADGET = 8
GADGET_EDGES = ((0, 1), (1, 2), (2, 3), (1, 4), (4, 5), (5, 3), (0, 6), (6, 7), (7, 2))   # e a d t b1 b2 c1 c2


def layers_edges(widths):
    n = sum(widths)
    e = np.zeros((n, n), bool)
    at = np.concatenate([[0], np.cumsum(widths)])
    for k in range(len(widths) - 1):
        e[at[k]:at[k + 1], at[k + 1]:at[k + 2]] = True
    return e


def new_family(n, family):
    """(bool edge matrix [n, n], E, T) of one of NEW_FAMILIES"""
    e = np.zeros((n, n), bool)
    i = np.arange(n)
    if family == "layers":
        w = layer_widths(n)
        return layers_edges(w), tuple(range(w[0])), tuple(range(n - w[-1], n))
    if family == "hourglass":
        k, a = max(0, min(3, n - 2)), n // 2 + 1
        e[:a, :a] = True
        e[max(a - k, 0):, max(a - k, 0):] = True
        e[i, i] = False
        return e, (0,), (n - 1,)
    if family == "grid":
        r, c = grid_shape(n)
        for y in range(r):
            for x in range(c):
                if x + 1 < c:
                    e[y * c + x, y * c + x + 1] = True
                if y + 1 < r:
                    e[y * c + x, (y + 1) * c + x] = True
        return e, tuple(y * c for y in range(r)), tuple(y * c + c - 1 for y in range(r))
    assert family == "zigzag", family
    g = n // GADGET
    for k in range(g):
        for a, b in GADGET_EDGES:
            e[GADGET * k + a, GADGET * k + b] = True
    return e, tuple(GADGET * k for k in range(g)), tuple(GADGET * k + 3 for k in range(g))


def known(n, family):
    """the written-down answer of a new family for its own E and T, all slices: a dict of cut_size, near, far
    (sorted ids), near_reach, far_reach; None where the family is degenerate at n"""
    if family == "layers":
        w = layer_widths(n)
        if len(w) < 3:
            return None
        at = np.concatenate([[0], np.cumsum(w)])
        k = min(w[1:-1])
        first = 1 + w[1:-1].index(k)
        last = len(w) - 2 - w[1:-1][::-1].index(k)
        return {"cut_size": k, "near": list(range(at[first], at[first + 1])), "far": list(range(at[last], at[last + 1])),
                "near_reach": int(at[first]), "far_reach": int(at[last])}
    if family == "hourglass":
        if n < 8:
            return None
        a = n // 2 + 1
        shared = list(range(a - 3, a))
        return {"cut_size": 3, "near": shared, "far": shared, "near_reach": a - 3, "far_reach": a - 3}
    if family == "grid":
        r, c = grid_shape(n)
        if c < 3:
            return None
        return {"cut_size": r, "near": [y * c + 1 for y in range(r)], "far": [y * c + c - 2 for y in range(r)],
                "near_reach": r, "far_reach": r * (c - 2)}
    g = n // GADGET
    return {"cut_size": 2 * g, "near": sorted(GADGET * k + x for k in range(g) for x in (1, 6)),
            "far": sorted(GADGET * k + x for k in range(g) for x in (2, 5)), "near_reach": g, "far_reach": 5 * g} if g else None


# ---- inputs --------------------------------------------------------------------------------------
class Graph:
    """closure_cases.Synthetic's inputs for a given edge matrix: every edge ALLOW in one random slice, the
    other cells random codes from {0, 1, 3}, random padding bits"""

    def __init__(self, e, family, n_svc=3, seed=0):
        n = e.shape[0]
        g = np.random.default_rng([seed, n, 2000 + NEW_FAMILIES.index(family), n_svc])
        self.n, self.n_svc, self.family = n, n_svc, family
        owner = g.integers(0, n_svc, (n, n), dtype=np.uint8)
        other = np.array([0, 1, 3], np.uint8)[g.integers(0, 3, (n_svc, n, n), dtype=np.uint8)]
        self.codes = np.where(e[None] & (owner[None] == np.arange(n_svc)[:, None, None]), np.uint8(ALLOW), other)
        assert ((self.codes == ALLOW).sum(axis=0) == e).all()   # every edge in exactly one slice
        self.words = np.stack([dc.garbage(dc.pack_wide(self.codes[v]), n, seed + 1 + v) for v in range(n_svc)])


@functools.lru_cache(maxsize=None)
def graph(n, family, n_svc=3, seed=0):
    """the inputs of a family at n end points: .n, .n_svc, .codes u8 [n_svc, n, n], .words u32 [n_svc, n, rw]"""
    if family in NEW_FAMILIES:
        return Graph(new_family(n, family)[0], family, n_svc, seed)
    return cc.synthetic(n, family, n_svc, seed)


def edge_matrix(codes, select=None):
    codes = np.asarray(codes)
    sel = list(range(codes.shape[0])) if select is None else list(select)
    return (codes[sel] == ALLOW).any(axis=0) if sel else np.zeros(codes.shape[1:], bool)


def end_sets(n, family, a):
    """(E, T) pairs: a single entry and target; several; overlapping (inseparable); directly joined
    (inseparable, where the graph has an edge between two distinct end points); no entry; no target; with
    duplicates; and for a new family its own sets first"""
    sets = [((0,), (n - 1,)), (tuple(range(min(3, n))), tuple(range(max(n - 3, 0), n))) if n >= 8 else ((0,), (n // 2,)),
            ((0, n // 2), (n // 2, n - 1)), ((), (n - 1,)), ((0,), ()), ((0, 0, n // 3), (n - 1, n - 1, n // 3 * 2))]
    off = a & ~np.eye(n, dtype=bool)
    if off.any():
        i, j = np.argwhere(off)[len(np.argwhere(off)) // 2]
        sets.insert(3, ((int(i), 0), (int(j),)))
    if family in NEW_FAMILIES:
        sets.insert(0, new_family(n, family)[1:])
    return sets


# ---- the references ------------------------------------------------------------------------------
def search(a, start, without=None):
    """the nodes that walks from the bool vector `start` reach in the graph `a` without the nodes `without`"""
    block = np.zeros(len(start), bool) if without is None else without
    seen = start & ~block
    front = seen.copy()
    while front.any():
        front = a[front].any(axis=0) & ~seen & ~block
        seen |= front
    return seen


def as_sets(n, E, T):
    e, t = np.zeros(n, bool), np.zeros(n, bool)
    e[np.array(E, np.int64)] = True
    t[np.array(T, np.int64)] = True
    return e, t


def direct_pairs(a, e, t):
    return int((a | np.eye(len(e), dtype=bool))[np.ix_(e, t)].sum())


class Answer:
    """what the graph alone decides: n_direct, cut_size (None when inseparable), near, far, reach_near,
    reach_far (bool [n])"""

    def __init__(self, n, n_direct, k=None, near=None, far=None, reach_near=None, reach_far=None):
        z = np.zeros(n, bool)
        self.n, self.n_direct, self.cut_size = n, n_direct, k
        self.near, self.far = (z, z) if k is None else (near, far)
        self.reach_near, self.reach_far = (z, z) if k is None else (reach_near, reach_far)

    def flags(self):
        return (NEAR * self.near + FAR * self.far + NEAR_REACH * self.reach_near + FAR_REACH * self.reach_far).astype(np.uint8)

    def at(self, max_cut):
        """(the EXACT fields, out_cut) under max_cut"""
        if self.cut_size is None:
            return dict(zip(EXACT, (0, 0, self.n_direct, NO_CUT, 0, 0, 0))), np.zeros(self.n, np.uint8)
        if self.cut_size > max_cut:
            return dict(zip(EXACT, (1, 1, 0, NO_CUT, max_cut + 1, 0, 0))), np.zeros(self.n, np.uint8)
        return (dict(zip(EXACT, (1, 0, 0, self.cut_size, self.cut_size, int(self.reach_near.sum()), int(self.reach_far.sum())))),
                self.flags())

    def same(self, o):
        return (self.n_direct == o.n_direct and self.cut_size == o.cut_size and (self.flags() == o.flags()).all())


def brute(a, E, T):
    """the definition; n <= 12"""
    n = a.shape[0]
    assert n <= 12
    e, t = as_sets(n, E, T)
    d = direct_pairs(a, e, t)
    if d:
        return Answer(n, d)
    inner = np.flatnonzero(~e & ~t)
    for k in range(len(inner) + 1):
        cuts = []
        for c in itertools.combinations(inner, k):
            block = np.zeros(n, bool)
            block[list(c)] = True
            reach = search(a, e, block)
            if not (reach & t).any():
                cuts.append((block, reach, search(a.T, t, block)))
        if cuts:
            near = [c for c in cuts if all((c[1] <= o[1]).all() for o in cuts)]
            far = [c for c in cuts if all((c[2] <= o[2]).all() for o in cuts)]
            assert len(near) == 1 and len(far) == 1, "the canonical cuts are not unique"
            return Answer(n, 0, k, near[0][0], far[0][0], near[0][1], far[0][1])
    raise AssertionError("the interior itself separates")


def split_arcs(a, e, t):
    """the split graph as (u, v, capacity) with v_in = 2 v, v_out = 2 v + 1, source 2 n, sink 2 n + 1; `big`
    stands for unbounded"""
    n = a.shape[0]
    big = n + 1
    arcs = [(2 * n, 2 * v + 1, big) for v in np.flatnonzero(e)] + [(2 * v, 2 * n + 1, big) for v in np.flatnonzero(t)]
    arcs += [(2 * v, 2 * v + 1, 1) for v in np.flatnonzero(~e & ~t)]
    use = a & ~np.eye(n, dtype=bool) & ~t[:, None] & ~e[None, :]
    arcs += [(2 * int(u) + 1, 2 * int(v), big) for u, v in np.argwhere(use)]
    return arcs


def from_residual(a, e, t, n_direct, k, src_side, sink_side):
    """the residual rule: src_side / sink_side are bool [2 n + 2] over the split graph's nodes"""
    n = a.shape[0]
    inner = ~e & ~t
    near = inner & src_side[0:2 * n:2] & ~src_side[1:2 * n:2]
    far = inner & sink_side[1:2 * n:2] & ~sink_side[0:2 * n:2]
    assert int(near.sum()) == k and int(far.sum()) == k, "a canonical cut is not a minimum cut"
    return Answer(n, n_direct, k, near, far, search(a, e, near), search(a, e, far))


def flow(a, E, T):
    """maximum flow by depth-first augmenting paths in plain Python, then the residual rule"""
    n = a.shape[0]
    e, t = as_sets(n, E, T)
    d = direct_pairs(a, e, t)
    if d:
        return Answer(n, d)
    cap = [dict() for _ in range(2 * n + 2)]
    for u, v, c in split_arcs(a, e, t):
        cap[u][v] = c
        cap[v].setdefault(u, 0)
    s, z = 2 * n, 2 * n + 1
    k = 0
    while True:
        parent = {s: s}
        stack = [s]
        while stack and z not in parent:
            u = stack.pop()
            for v, c in cap[u].items():
                if c > 0 and v not in parent:
                    parent[v] = u
                    stack.append(v)
        if z not in parent:
            break
        v = z
        while v != s:
            cap[parent[v]][v] -= 1
            cap[v][parent[v]] += 1
            v = parent[v]
        k += 1

    def side(start, forward):
        seen = np.zeros(2 * n + 2, bool)
        seen[start] = True
        stack = [start]
        while stack:
            u = stack.pop()
            for v in cap[u]:
                if not seen[v] and (cap[u][v] if forward else cap[v][u]) > 0:
                    seen[v] = True
                    stack.append(v)
        return seen
    return from_residual(a, e, t, 0, k, side(s, True), side(z, False))


def flow_scipy(a, E, T):
    """scipy's maximum flow on the split graph, residual reachability by numpy"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import breadth_first_order, maximum_flow
    n = a.shape[0]
    e, t = as_sets(n, E, T)
    d = direct_pairs(a, e, t)
    if d:
        return Answer(n, d)
    arcs = np.array(split_arcs(a, e, t), np.int64).reshape(-1, 3)
    m = 2 * n + 2
    capacity = sp.csr_matrix((arcs[:, 2].astype(np.int32), (arcs[:, 0], arcs[:, 1])), shape=(m, m))
    r = maximum_flow(capacity, 2 * n, 2 * n + 1)
    # (the flow matrix is antisymmetric: capacity - flow holds the forward and the back arcs)
    residual = (capacity - r.flow).tocsr()
    residual.data = (residual.data > 0).astype(np.int32)
    residual.eliminate_zeros()
    sides = []
    for start, g in ((2 * n, residual), (2 * n + 1, residual.T.tocsr())):
        seen = np.zeros(m, bool)
        seen[breadth_first_order(g, start, directed=True, return_predecessors=False)] = True
        sides.append(seen)
    return from_residual(a, e, t, 0, int(r.flow_value), sides[0], sides[1])


@functools.lru_cache(maxsize=None)
def expected(n, family, E, T, select=None, n_svc=3, seed=0):
    a = edge_matrix(graph(n, family, n_svc, seed).codes, select)
    return (flow if n < SCIPY_FROM else flow_scipy)(a, E, T)


def check_witness(a, E, T, prev, nxt, n_paths, what=None):
    """out_prev / out_next as n_paths disjoint chains from E to T over edges of `a`"""
    n = a.shape[0]
    e, t = as_sets(n, E, T)
    on = (prev != NO_HOP) | (nxt != NO_HOP)
    assert ((prev != NO_HOP) == (nxt != NO_HOP)).all() and not (on & (e | t)).any(), (what, "an end point half on a path, or of E u T")
    starts = np.flatnonzero(on & e[np.where(on, prev, 0)])
    assert len(starts) == n_paths, (what, "paths", len(starts), n_paths)
    seen = np.zeros(n, bool)
    for v in starts:
        v = int(v)
        assert a[prev[v], v], (what, "no edge", int(prev[v]), v)
        while True:
            assert not seen[v] and on[v], (what, "an end point on two paths, or off them", v)
            seen[v] = True
            w = int(nxt[v])
            assert a[v, w], (what, "no edge", v, w)
            if t[w]:
                break
            assert prev[w] == v, (what, "prev and next disagree", v, w)
            v = w
    assert (seen == on).all(), (what, "an end point marked that is on no path from E")


# ---- runs ----------------------------------------------------------------------------------------
def result_dict(res):
    return {k: getattr(res, k) for k in RESULT_FIELDS}


def spec_of(matrix_ptr, n, n_svc, E, T, max_cut, select):
    """pg_reach_cut_spec -> (spec, the arrays it points into: keep them alive for the call)"""
    f = cc.flags(select, n_svc)
    ent, tgt = np.ascontiguousarray(E, np.uint32).reshape(-1), np.ascontiguousarray(T, np.uint32).reshape(-1)
    spec = _capi.pg_reach_cut_spec(matrix_ptr, n, n_svc, f.ctypes.data if f is not None else None, ent.ctypes.data if len(ent) else None,
                                   len(ent), tgt.ctypes.data if len(tgt) else None, len(tgt), max_cut)
    return spec, (f, ent, tgt)


def run_host(e, words, n, E, T, max_cut=LARGE, select=None, cut=True, prev=True, nxt=True):
    """pg_debug_reach_cut_host over prefilled outputs with guards -> (cut u8 [n] or None, prev u16 [n] or None,
    next u16 [n] or None, result dict)"""
    m = np.ascontiguousarray(words, np.uint32)
    n_svc = m.size // (n * cc.row_words(n))
    cbuf = np.full(n + GUARD, 0xEE, np.uint8)
    pbuf = np.full(n + GUARD, 0xEEEE, np.uint16)
    xbuf = np.full(n + GUARD, 0xEEEE, np.uint16)
    spec, keep = spec_of(m.ctypes.data, n, n_svc, E, T, max_cut, select)
    res = _capi.pg_reach_cut_result(*[77] * 9)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    code = lib.pg_debug_reach_cut_host(e.h, C.byref(spec), p(cbuf) if cut else None, p(pbuf) if prev else None,
                                       p(xbuf) if nxt else None, C.byref(res))
    assert code == 0, lib.pg_last_error(e.h)
    del keep
    return finish(n, cbuf, pbuf, xbuf, res, cut, prev, nxt)


def finish(n, cbuf, pbuf, xbuf, res, cut, prev, nxt):
    """the guards of a run's buffers, and the run's return value"""
    assert (cbuf[n:] == 0xEE).all() and (pbuf[n:] == 0xEEEE).all() and (xbuf[n:] == 0xEEEE).all(), "a guard was written"
    assert cut or (cbuf == 0xEE).all()
    assert prev or (pbuf == 0xEEEE).all()
    assert nxt or (xbuf == 0xEEEE).all()
    return cbuf[:n] if cut else None, pbuf[:n] if prev else None, xbuf[:n] if nxt else None, result_dict(res)


def same(got, x, a, E, T, max_cut, what):
    """a run's return value against an Answer under max_cut; the witness validated"""
    c, pv, nx, r = got
    want, flags = x.at(max_cut)
    assert {k: r[k] for k in EXACT} == want, (what, r, want)
    assert c is None or (c == flags).all(), (what, "out_cut", np.flatnonzero(c != flags)[:4].tolist())
    if pv is not None and nx is not None:
        check_witness(a, E, T, pv, nx, want["n_paths"], what)
    for half in (pv, nx):
        if half is not None and want["n_paths"] == 0:
            assert (half == NO_HOP).all(), (what, "a path where there is none")


OUTPUTS = tuple((c, p, x) for c in (True, False) for p in (True, False) for x in (True, False))


def check(run, words, s, n, family, seed=0, small=False):
    """`run(words, n, E, T, max_cut, select, cut=, prev=, nxt=)` (run_host's contract without the engine)
    against expected(): every pair of end_sets under all slices; one slice and no slice, max_cut 0, cut_size - 1,
    cut_size and large, and every combination of the outputs under the first pair. -> the runs' results"""
    a = edge_matrix(s.codes)
    sets = end_sets(n, family, a)
    out = []
    for E, T in sets:
        x = expected(n, family, E, T, None, s.n_svc, seed)
        got = run(words, n, E, T, LARGE, None)
        same(got, x, a, E, T, LARGE, (n, family, E, T))
        out.append(got[3])
    for E, T in sets[:1] if small else sets[:2]:
        for sel in ((1,), ()):
            same(run(words, n, E, T, LARGE, sel), expected(n, family, E, T, sel, s.n_svc, seed), edge_matrix(s.codes, sel), E, T, LARGE,
                 (n, family, E, T, sel))
        x = expected(n, family, E, T, None, s.n_svc, seed)
        k = x.cut_size or 0
        for max_cut in sorted({0, max(k - 1, 0), k, 16}):
            same(run(words, n, E, T, max_cut, None), x, a, E, T, max_cut, (n, family, E, T, "max_cut", max_cut))
    E, T = sets[0]
    x = expected(n, family, E, T, None, s.n_svc, seed)
    for c, p, q in OUTPUTS:
        same(run(words, n, E, T, LARGE, None, cut=c, prev=p, nxt=q), x, a, E, T, LARGE, (n, family, "outputs", c, p, q))
    return out


def check_known(run, words, s, n, family):
    """a new family's own sets against its written-down answer"""
    want = known(n, family)
    if want is None:
        return None
    a, E, T = new_family(n, family)
    c, pv, nx, r = run(words, n, E, T, LARGE, None)
    assert r["separable"] == 1 and r["capped"] == 0 and r["cut_size"] == r["n_paths"] == want["cut_size"], (n, family, r)
    assert np.flatnonzero(c & NEAR).tolist() == want["near"] and np.flatnonzero(c & FAR).tolist() == want["far"], (n, family)
    assert (r["near_reach"], r["far_reach"]) == (want["near_reach"], want["far_reach"]), (n, family, r)
    if family == "zigzag":
        assert r["reroutes"] > 0, (n, r)
    check_witness(a, E, T, pv, nx, r["n_paths"], (n, family))
    return r


# ---- large layers without n x n codes ------------------------------------------------------------
def layers_words(widths, seed=0):
    """the packed words u32 [1, n, row_words(n)] of a layers graph in one slice: ALLOW on the edges, random codes
    from {0, 1, 3} elsewhere, random padding bits; built a layer at a time"""
    n = sum(widths)
    rw = cc.row_words(n)
    g = np.random.default_rng([seed, n, 2100])
    at = np.concatenate([[0], np.cumsum(widths)])
    w = np.empty((n, rw), np.uint32)
    cols = np.arange(rw * 16)
    for k in range(len(widths)):
        lo, hi = (at[k + 1], at[k + 2]) if k + 1 < len(widths) else (0, 0)
        rows = int(at[k + 1] - at[k])
        x = g.integers(0, 1 << 32, (min(rows, 64), rw), dtype=np.uint64).astype(np.uint32)
        x |= (x >> 1) & ~x & np.uint32(0x55555555)   # (a random ALLOW becomes 3)
        x = np.resize(x, (rows, rw))                 # (64 random rows, repeated)
        cells = np.where((cols >= lo) & (cols < hi), ALLOW, 0).reshape(rw, 16)
        allow = (cells << (2 * np.arange(16))).sum(axis=1).astype(np.uint32)
        keep = ~((cells > 0) * 3 << (2 * np.arange(16))).sum(axis=1).astype(np.uint32)
        w[at[k]:at[k + 1]] = (x & keep) | allow
    w[:, -1] &= np.uint32(0xFFFFFFFF >> (2 * (-n & 15)))
    return dc.garbage(w, n, seed + 1)[None]


# ---- what the two test files share beyond the runs -------------------------------------------------
def small_cases():
    """random graphs of 3 to 12 end points with random entry and target sets: (a, E, T)"""
    g = np.random.default_rng(11)
    for n in SMALL_SIZES:
        for _ in range(24 if n <= 9 else 6):
            a = g.random((n, n)) < g.choice([0.2, 0.35, 0.5])
            ids = g.permutation(n)
            ne, nt = int(g.integers(1, 3)), int(g.integers(1, 3))
            yield a, tuple(int(x) for x in ids[:ne]), tuple(int(x) for x in ids[ne:ne + nt])


def plan_of(e, n):
    return e.debug_reach_cut_plan(n)


def plan_sizes(e):
    """n at -1, 0, +1 around the sizes where the plan's lane words change, read from the plan"""
    out = []
    for m in (2048, 4096):
        lo, hi = m - 64, m + 64
        assert plan_of(e, lo)["lane_words"] != plan_of(e, hi)["lane_words"]
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if plan_of(e, mid)["lane_words"] == plan_of(e, lo)["lane_words"] else (lo, mid)
        out += [hi - 1, hi, hi + 1]
    return tuple(out)


def cut_want(c, pods, entry_pods, target_pods, max_cut=16):
    """Engine.reachability_cut's near, far and exact result fields from the oracle's matrix and flow()"""
    at = [cc.CHAIN_PODS.index(p) for p in pods]
    a = dm.oracle_edges(c)[np.ix_(at, at)]
    E, T = [pods.index(p) for p in entry_pods], [pods.index(p) for p in target_pods]
    x = flow(a, tuple(E), tuple(T))
    res, flags = x.at(max_cut)
    res = dict(res, cut_size=None if res["cut_size"] == NO_CUT else res["cut_size"])
    return ([pods[k] for k in range(len(pods)) if flags[k] & NEAR], [pods[k] for k in range(len(pods)) if flags[k] & FAR], res, a, E, T)


def check_wrapper(c, got, pods, entry, target, max_cut=16):
    near, far, routes, res = got
    wn, wf, wres, a, E, T = cut_want(c, pods, entry, target, max_cut)
    assert (near, far) == (wn, wf) and {k: res[k] for k in EXACT} == wres, (got, wn, wf, wres)
    assert len(routes) == wres["n_paths"]
    inner = [p for r in routes for p in r[1:-1]]
    assert len(set(inner)) == len(inner) and not set(inner) & (set(entry) | set(target))
    for r in routes:
        ids = [pods.index(p) for p in r]
        assert ids[0] in E and ids[-1] in T and all(a[u, v] for u, v in zip(ids, ids[1:])), r


WRAPPER_CASES = ((cc.CHAIN_PODS, ["ns/c0"], ["ns/c11"], 16), (cc.CHAIN_PODS[::-1], ["ns/c1", "ns/c0"], ["ns/c10", "ns/c7"], 16),
                 (cc.CHAIN_PODS, ["ns/c0"], ["ns/c11"], 0), (cc.CHAIN_PODS, ["ns/c0"], ["ns/c5"], 16), (cc.CHAIN_PODS, [], ["ns/c5"], 16),
                 (cc.CHAIN_PODS, ["ns/c4", "ns/c2"], ["ns/c4"], 16))


def bad_specs(ptr):
    """(spec, with result, what pg_last_error has to name) of every PG_EINVAL of the contract; the arrays the
    specs point into"""
    S = _capi.pg_reach_cut_spec
    ids = np.array([1, 2, 4, 3], np.uint32)
    many = np.zeros((1 << 15) + 1, np.uint32)
    ip, mp, big = ids.ctypes.data, many.ctypes.data, (1 << 15) + 1
    return [(None, True, "spec"), (S(ptr, 4, 1, None, ip, 2, ip, 2, 1), False, "result"), (S(None, 4, 1, None, ip, 2, ip, 2, 1), True, "matrix"),
            (S(ptr, 4, 1, None, None, 2, ip, 2, 1), True, "entry"), (S(ptr, 4, 1, None, ip, 2, None, 2, 1), True, "target"),
            (S(ptr, big, 1, None, ip, 2, ip, 2, 1), True, "n: more"), (S(ptr, 4, 1, None, mp, big, ip, 2, 1), True, "n_entry"),
            (S(ptr, 4, 1, None, ip, 2, mp, big, 1), True, "n_target"), (S(ptr, 4, 1, None, ip, 2, ip, 2, big), True, "max_cut"),
            (S(ptr, 4, 0, None, ip, 2, ip, 2, 1), True, "n_svc"), (S(ptr, 4, 4097, None, ip, 2, ip, 2, 1), True, "n_svc"),
            (S(ptr, 4, 1, None, ip, 3, ip, 2, 1), True, "entry[2]"), (S(ptr, 4, 1, None, ip, 2, ip, 3, 1), True, "target[2]")], (ids, many)
