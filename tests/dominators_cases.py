"""Graphs, entry sets and expected answers of the reachability-dominators tests (test helper).

Shared by tests/test_dominators_host.py (pg_debug_reach_dominators_host, no GPU) and
tests/test_gpu_dominators.py (pg_reach_dominators on the device). Expected values come from numpy alone
and never from the product.

Expected(edges, entry) follows the definition: reached by a breadth-first search from the entry set E,
then for every reached k one search in the graph without k, so k is in Dom(v) iff v is reached and is not
reached without k. idom (by the size rule, whose uniqueness is asserted), cut and the result fields come
from that Dom. A second, independent route is the synchronous iteration Avoid' = Avoid | ((ET (x) Avoid)
minus the diagonal) as boolean matrix products over n + 1 columns, the last the reached column set in the
entries' rows; it gives `rounds`, and its Dom must equal the first route's (asserted in Expected).
torch_expected() is the second route in torch on any device: the reference of the large random graph,
pinned bit for bit to Expected by the CPU tests.

Inputs: the families of closure_cases (imported, not edited: empty, full, chain, ring, star, two-cliques,
sparse, medium, dense) and four families whose answer for the entry set {0} is written down here (KNOWN):
  diamond  diamonds in a row: s_k = 3k -> a_k = 3k + 1, b_k = 3k + 2 -> s_k+1. No choke point but the
           s nodes; idom(s_k+1) = s_k although no edge joins them.
  bowtie   two cliques (0 .. h and h .. n - 1, h = n // 2) sharing node h, which dominates all of the
           second one.
  ladder   two parallel chains (even and odd nodes) with rungs both ways and a diagonal from each odd node
           to the next even one: nothing dominates past the entry.
  tree     a random arborescence (parent[v] < v) with back edges from nodes to their ancestors: Dom(v) is
           the root path, cut the subtree size - 1, and the back edges change nothing.
Every edge is given to one random slice, the other cells hold random codes from {0, 1, 3}, and the padding
bits are random (graph()), as closure_cases.Synthetic does.

check(run, s) holds a backend (`run`: the host twin here, the device in test_gpu_dominators.py) against
Expected over the entry sets of entry_sets(n), svc_select None, one slice and none, and every combination
of the three optional outputs; the runs put guard words behind every prefilled output and assert that they
stay untouched, and the expected out_dom words have zero padding.
"""
import ctypes as C
import functools

import numpy as np

import closure_cases as cc
import diff_cases as dc
import reach_cases as rc
from vpp_amd import _capi
from vpp_amd._capi import lib

ALLOW = cc.ALLOW
SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
NEW_FAMILIES = ("diamond", "bowtie", "ladder", "tree")
FAMILIES = cc.FAMILIES + NEW_FAMILIES
FILL, GUARD = cc.FILL, cc.GUARD
NONE, NO_IDOM = 0xFFFFFFFF, 0xFFFF
RESULT_FIELDS = ("n_reached", "n_chokes", "top", "top_cut", "depth", "rounds")


# ---- the new families ----------------------------------------------------------------------------
def tree_parents(n, seed=0):
    g = np.random.default_rng([seed, n, 77])
    return np.array([0] + [int(g.integers(0, v)) for v in range(1, n)], np.int64)


def new_edges(n, family, seed=0):
    """the bool edge matrix [n, n] of one of NEW_FAMILIES"""
    e = np.zeros((n, n), bool)
    i = np.arange(n)
    if family == "diamond":
        for k in range(0, n, 3):
            for mid in (k + 1, k + 2):
                if mid < n:
                    e[k, mid] = True
                    if k + 3 < n:
                        e[mid, k + 3] = True
    elif family == "bowtie":
        h = n // 2
        e[:h + 1, :h + 1] = e[h:, h:] = True
        e[i, i] = False
    elif family == "ladder":
        e[i[:-2], i[2:]] = True                       # the two chains
        even = i[(i % 2 == 0) & (i + 1 < n)]
        e[even, even + 1] = e[even + 1, even] = True  # the rungs
        odd = i[(i % 2 == 1) & (i + 1 < n)]
        e[odd, odd + 1] = True                        # the diagonals
    else:
        assert family == "tree", family
        parent = tree_parents(n, seed)
        g = np.random.default_rng([seed, n, 78])
        for v in range(1, n):
            e[parent[v], v] = True
            if g.random() < 0.5:   # a back edge to a random ancestor
                path = [v]
                while path[-1]:
                    path.append(int(parent[path[-1]]))
                e[v, path[int(g.integers(1, len(path)))]] = True
    return e


def known(n, family, seed=0):
    """the written-down answer of a new family for the entry set {0}: (dom bool [n, n], idom int64 [n] with
    -1 for none, cut int64 [n])"""
    dom = np.zeros((n, n), bool)
    idom = np.full(n, -1, np.int64)
    v = np.arange(n)
    dom[v, v] = True
    if family == "diamond":
        for x in range(n):
            dom[x, np.arange(0, x // 3 * 3 + 1, 3)] = True
            if x:
                idom[x] = x // 3 * 3 if x % 3 else x - 3
    elif family == "bowtie":
        h = n // 2
        dom[:, 0] = True
        dom[h + 1:, h] = True
        idom[1:] = 0
        idom[h + 1:] = h
    elif family == "ladder":
        dom[:, 0] = True
        idom[1:] = 0
    else:
        assert family == "tree", family
        parent = tree_parents(n, seed)
        for x in range(1, n):
            dom[x] |= dom[parent[x]]
            idom[x] = parent[x]
    return dom, idom, dom.sum(axis=0) - 1


# ---- inputs --------------------------------------------------------------------------------------
class Graph:
    """closure_cases.Synthetic's inputs for a given edge matrix: every edge ALLOW in one random slice, the
    other cells random codes from {0, 1, 3}, random padding bits"""

    def __init__(self, e, family, n_svc=3, seed=0):
        n = e.shape[0]
        g = np.random.default_rng([seed, n, 1000 + NEW_FAMILIES.index(family), n_svc])
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
        return Graph(new_edges(n, family, seed), family, n_svc, seed)
    return cc.synthetic(n, family, n_svc, seed)


def edge_matrix(codes, select=None):
    codes = np.asarray(codes)
    sel = list(range(codes.shape[0])) if select is None else list(select)
    return (codes[sel] == ALLOW).any(axis=0) if sel else np.zeros(codes.shape[1:], bool)


def entry_sets(n):
    """node 0; a node of the last word; three nodes with a duplicate among them; every node; none"""
    return ((0,), (n - 1,), (n // 2, n // 3, n // 2), tuple(range(n)), ())


# ---- the reference -------------------------------------------------------------------------------
def search(a, start, without=-1):
    """the nodes that walks from the bool vector `start` reach in the graph `a` without node `without`"""
    seen = start.copy()
    if without >= 0:
        seen[without] = False
    front = seen.copy()
    while front.any():
        nxt = a[front].any(axis=0) & ~seen
        if without >= 0:
            nxt[without] = False
        seen |= nxt
        front = nxt
    return seen


def avoid_rounds(a, entry):
    """the synchronous iteration as boolean products -> (Avoid bool [n, n + 1], rounds)"""
    n = a.shape[0]
    avoid = np.zeros((n, n + 1), bool)
    ent = np.array(sorted(set(entry)), np.int64)
    avoid[ent] = True
    avoid[ent, ent] = False
    et = a.T.astype(np.float32)
    v = np.arange(n)
    rounds = 0
    while True:
        p = (et @ avoid.astype(np.float32)) > 0   # (sums <= n < 2^24: exact)
        p[v, v] = False
        new = avoid | p
        if (new == avoid).all():
            return avoid, rounds
        avoid, rounds = new, rounds + 1


class Expected:
    """the dominators of the bool edge matrix `a` from the entry ids `entry`"""

    def __init__(self, a, entry, rounds=True):
        n = a.shape[0]
        self.n, self.entry = n, tuple(entry)
        start = np.zeros(n, bool)
        start[np.array(entry, np.int64)] = True
        self.reached = reached = search(a, start)
        dom = np.zeros((n, n), bool)
        for k in np.flatnonzero(reached):
            dom[:, k] = reached & ~search(a, start, int(k))
        assert (np.diag(dom) == reached).all()
        self.dom = dom
        self.size = size = dom.sum(axis=1)
        self.cut = (dom.sum(axis=0) - np.diag(dom)).astype(np.uint32)
        self.idom = np.full(n, NO_IDOM, np.uint16)
        strict = dom & ~np.eye(n, dtype=bool)
        hit = strict & (size[None, :] == size[:, None] - 1)
        assert (hit.sum(axis=1) == strict.any(axis=1)).all(), "idom is not unique by the size rule"
        rows = np.flatnonzero(hit.any(axis=1))
        self.idom[rows] = hit[rows].argmax(axis=1)
        choke = (self.cut > 0) & ~start
        top = int(np.flatnonzero(choke & (self.cut == self.cut[choke].max()))[0]) if choke.any() else NONE
        self.result = {"n_reached": int(reached.sum()), "n_chokes": int(choke.sum()), "top": top,
                       "top_cut": int(self.cut[top]) if choke.any() else 0, "depth": int(size.max()) - 1 if reached.any() else 0}
        if rounds:
            avoid, self.result["rounds"] = avoid_rounds(a, entry)
            assert (avoid[:, n] == reached).all() and ((~avoid[:, :n] & reached[:, None]) == dom).all(), "the two routes differ"

    def packed(self):
        """out_dom: ALLOW where k dominates v, DENY_SYN elsewhere, padding zero"""
        return cc.pack_reach(self.dom)


@functools.lru_cache(maxsize=None)
def expected(n, family, entry, select=None, n_svc=3, seed=0):
    return Expected(edge_matrix(graph(n, family, n_svc, seed).codes, select), entry)


def torch_expected(a, entry, device):
    """the second route in torch on `device` (a: bool tensor [n, n]) -> (dom bool [n, n], idom int64 [n] with
    NO_IDOM for none, cut int64 [n], result dict), tensors on `device`. The products are fp32 over 0 / 1
    operands (sums <= n < 2^24: exact)"""
    import torch
    n = a.shape[0]
    dt = torch.float32
    avoid = torch.zeros((n, n + 1), dtype=torch.bool, device=device)
    ent = torch.tensor(sorted(set(entry)), dtype=torch.int64, device=device)
    start = torch.zeros(n, dtype=torch.bool, device=device)
    if len(ent):
        avoid[ent] = True
        avoid[ent, ent] = False
        start[ent] = True
    et = a.T.to(dt).contiguous()
    v = torch.arange(n, device=device)
    rounds = 0
    while True:
        p = (et @ avoid.to(dt)) > 0
        p[v, v] = False
        new = avoid | p
        if torch.equal(new, avoid):
            break
        avoid, rounds = new, rounds + 1
    reached = avoid[:, n]
    dom = ~avoid[:, :n] & reached[:, None]
    size = dom.sum(dim=1)
    cut = dom.sum(dim=0) - dom.diagonal().to(torch.int64)
    strict = dom.clone()
    strict[v, v] = False
    hit = strict & (size[None, :] == size[:, None] - 1)
    idom = torch.where(hit.any(dim=1), hit.to(torch.uint8).argmax(dim=1), torch.full_like(size, NO_IDOM))
    choke = (cut > 0) & ~start
    if bool(choke.any()):
        best = int(cut[choke].max())
        top = int(torch.nonzero(choke & (cut == best))[0])
    else:
        best, top = 0, NONE
    res = {"n_reached": int(reached.sum()), "n_chokes": int(choke.sum()), "top": top, "top_cut": best,
           "depth": int(size.max()) - 1 if bool(reached.any()) else 0, "rounds": rounds}
    return dom, idom, cut, res


# ---- the islands past the plan's cuts ------------------------------------------------------------
class IslandCase:
    """closure_cases.Islands at n end points with the entry set {the least node of the first island that
    reaches node n - 1}: the expectation is Expected on the 240 island nodes, embedded"""

    def __init__(self, n):
        self.n, self.s = n, cc.Islands(n, seed=ISLAND_SEEDS[n])
        self.idx = idx = self.s.idx
        a = edge_matrix(self.s.sub)
        last = len(idx) - 1
        assert idx[last] == n - 1
        first = [k for k in range(cc.ISLAND) if search(a, np.arange(len(idx)) == k)[last]]
        assert first, "no node of the first island reaches node n - 1"
        self.sub_entry = first[0]
        self.entry = (int(idx[first[0]]),)
        self.sub = Expected(a, (self.sub_entry,))
        r = self.sub.result
        self.result = dict(r, top=int(idx[r["top"]]) if r["top"] != NONE else NONE)
        self.idom = np.full(n, NO_IDOM, np.uint16)
        has = self.sub.idom != NO_IDOM
        self.idom[idx[has]] = idx[self.sub.idom[has]]
        self.cut = np.zeros(n, np.uint32)
        self.cut[idx] = self.sub.cut

    def non_trivial(self):
        """what keeps the case from passing on a graph that fell apart, on the reference alone"""
        r = self.result
        assert r["n_reached"] >= 150 and r["n_chokes"] >= 20 and r["depth"] >= 6 and r["rounds"] >= 10, r
        return r

    def dom_rows(self):
        """the expected out_dom rows of the island nodes, u32 [240, row_words(n)]; every other row is zero"""
        rows = np.zeros((len(self.idx), self.n), bool)
        rows[:, self.idx] = self.sub.dom
        return dc.pack_wide(np.where(rows, np.uint8(ALLOW), np.uint8(0)))


# the seeds of the islands at the sizes of the plan tests, the least for which some node of the first island
# reaches node n - 1 and the reference meets non_trivial()
ISLAND_SEEDS = {2047: 1, 2048: 1, 2049: 4, 4095: 1, 4096: 1, 4097: 1, 8191: 1, 8192: 2, 8193: 1, 1 << 15: 1}


def plan_sizes(e):
    """n at -1, 0, +1 around the sizes where the plan changes: a lane goes to 2 and to 4 bit-words, and a
    second column tile begins -- read from pg_debug_reach_dominators_plan, near 2048, 4096 and 8192"""
    out = []
    for m in (2048, 4096, 8192):
        lo, hi = m - 64, m + 64
        shape = lambda n: (e.debug_reach_dominators_plan(n)["lane_words"], e.debug_reach_dominators_plan(n)["col_tiles"])
        assert shape(lo) != shape(hi), (m, shape(lo), shape(hi))
        while hi - lo > 1:   # the least n with the wider plan
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if shape(mid) == shape(lo) else (lo, mid)
        out += [hi - 1, hi, hi + 1]
    return tuple(out)


PLAN_SHAPES = ((1, 1), (2, 1), (2, 1), (2, 1), (4, 1), (4, 1), (4, 1), (4, 2), (4, 2))   # (lane_words, col_tiles) at plan_sizes


# ---- runs ----------------------------------------------------------------------------------------
def result_dict(res):
    return {k: getattr(res, k) for k in RESULT_FIELDS}


def spec_of(matrix_ptr, n, n_svc, entry, select):
    """pg_reach_dominators_spec -> (spec, the arrays it points into: keep them alive for the call)"""
    f = cc.flags(select, n_svc)
    ent = np.ascontiguousarray(entry, np.uint32).reshape(-1)
    spec = _capi.pg_reach_dominators_spec(matrix_ptr, n, n_svc, f.ctypes.data if f is not None else None,
                                          ent.ctypes.data if len(ent) else None, len(ent))
    return spec, (f, ent)


def run_host(e, words, n, entry, select=None, dom=True, idom=True, cut=True):
    """pg_debug_reach_dominators_host over prefilled outputs with guards -> (dom words u32 [n, row_words] or
    None, idom u16 [n] or None, cut u32 [n] or None, result dict)"""
    m = np.ascontiguousarray(words, np.uint32)
    rw = cc.row_words(n)
    n_svc = m.size // (n * rw)
    dbuf = np.full(n * rw + GUARD, FILL, np.uint32)
    ibuf = np.full(n + GUARD, 0xEEEE, np.uint16)
    cbuf = np.full(n + GUARD, FILL, np.uint32)
    spec, keep = spec_of(m.ctypes.data, n, n_svc, entry, select)
    res = _capi.pg_reach_dominators_result(77, 77, 77, 77, 77, 77)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    code = lib.pg_debug_reach_dominators_host(e.h, C.byref(spec), p(dbuf) if dom else None, p(ibuf) if idom else None,
                                              p(cbuf) if cut else None, C.byref(res))
    assert code == 0, lib.pg_last_error(e.h)
    del keep
    return finish(n, dbuf, ibuf, cbuf, res, dom, idom, cut)


def finish(n, dbuf, ibuf, cbuf, res, dom, idom, cut):
    """the guards of a run's buffers, and the run's return value"""
    rw = cc.row_words(n)
    assert (dbuf[n * rw:] == FILL).all() and (ibuf[n:] == 0xEEEE).all() and (cbuf[n:] == FILL).all(), "a guard was written"
    assert dom or (dbuf == FILL).all()
    assert idom or (ibuf == 0xEEEE).all()
    assert cut or (cbuf == FILL).all()
    return (dbuf[:n * rw].reshape(n, rw) if dom else None, ibuf[:n] if idom else None, cbuf[:n] if cut else None,
            result_dict(res))


def same(got, x, what):
    """a run's return value against an Expected"""
    d, i, c, r = got
    assert r == x.result, (what, r, x.result)
    assert d is None or (d == x.packed()).all(), (what, "dom", np.argwhere(d != x.packed())[:3].tolist())
    assert i is None or (i == x.idom).all(), (what, "idom", np.flatnonzero(i != x.idom)[:3].tolist())
    assert c is None or (c == x.cut).all(), (what, "cut", np.flatnonzero(c != x.cut)[:3].tolist())


OUTPUTS = tuple((d, i, c) for d in (True, False) for i in (True, False) for c in (True, False))


def check(run, words, s, n, family, seed=0):
    """`run(words, n, entry, select, dom=, idom=, cut=)` (run_host's contract without the engine) against
    Expected: every entry set under all slices; one slice and no slice under two entry sets; every
    combination of the outputs"""
    sets = entry_sets(n)
    for ent in sets:
        same(run(words, n, ent, None), expected(n, family, ent, None, s.n_svc, seed), (n, family, ent))
    for sel in ((1,), ()):
        for ent in (sets[0], sets[2]):
            same(run(words, n, ent, sel), expected(n, family, ent, sel, s.n_svc, seed), (n, family, ent, sel))
    x = expected(n, family, sets[0], None, s.n_svc, seed)
    for d, i, c in OUTPUTS:
        same(run(words, n, sets[0], None, dom=d, idom=i, cut=c), x, (n, family, "outputs", d, i, c))


# ---- real engines and arguments, shared by the two test files ------------------------------------
def chain_expected(c, entry, select=None):
    return Expected(edge_matrix(c.codes, select), entry)


def oracle_edges(c):
    """the chain policy's graph from oracle.world.World.conn alone"""
    ips = np.asarray(cc.CHAIN_IPS, np.uint32)
    return ((rc.oracle_words(c.world, ips, ips, cc.CHAIN_SERVICES) >> 30) == cc.ALLOW).any(axis=0)


def chokepoints_want(c, pods, entry_pods):
    at = [cc.CHAIN_PODS.index(p) for p in pods]
    a = oracle_edges(c)[np.ix_(at, at)]
    x = Expected(a, [pods.index(p) for p in entry_pods])
    order = sorted((k for k in range(len(pods)) if x.cut[k] and pods[k] not in entry_pods), key=lambda k: (-int(x.cut[k]), k))
    res = dict(x.result, top=None if x.result["top"] == NONE else pods[x.result["top"]])
    return [(pods[k], int(x.cut[k])) for k in order], [None if k == NO_IDOM else pods[k] for k in x.idom], res


def bad_specs(ptr):
    """(spec, with result, what pg_last_error has to name) of every PG_EINVAL of the contract; the arrays the
    specs point into"""
    S = _capi.pg_reach_dominators_spec
    ent = np.array([1, 2, 4, 3], np.uint32)
    many = np.zeros((1 << 15) + 1, np.uint32)
    ep = ent.ctypes.data
    return [(None, True, "spec"), (S(ptr, 4, 1, None, ep, 2), False, "result"), (S(None, 4, 1, None, ep, 2), True, "matrix"),
            (S(ptr, 4, 1, None, None, 2), True, "entry"), (S(ptr, (1 << 15) + 1, 1, None, ep, 2), True, "n: more"),
            (S(ptr, 4, 1, None, many.ctypes.data, len(many)), True, "n_entry"), (S(ptr, 4, 0, None, ep, 2), True, "n_svc"),
            (S(ptr, 4, 4097, None, ep, 2), True, "n_svc"), (S(ptr, 4, 1, None, ep, 3), True, "entry[2]")], (ent, many)
