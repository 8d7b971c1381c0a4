"""Closures and expected zones of the reachability-zones tests (test helper).

Shared by tests/test_zones_host.py (pg_debug_reach_zones_host, no GPU) and tests/test_gpu_zones.py
(pg_reach_zones on the device). Expected values come from numpy alone (expected(): the definitions of
include/policygpu.h taken literally -- R = codes == ALLOW, M = R & R.T, the first set column of every row
of M, its minimum with the row's index, the distinct labels ascending, the counts, the representatives'
rows and columns gathered and packed) and, for real engines, from oracle.world.World.conn -- never from
the product. Independently, for the families built as true closures, a plain Tarjan over the *one-hop*
graph (scc()) must give the same partition: assert_inputs() checks that on the CPU.

synthetic(n, family, seed): uint8 codes [n, n], ALLOW where R holds and a random other code elsewhere,
packed with diff_cases.pack_wide:
  empty    no ALLOW cell: n zones, none cyclic
  full     all ALLOW: one zone
  chain    the strict upper triangle (the closure of the path 0 -> 1 -> ..): n acyclic singletons; the zone
           graph is the triangle
  rings    disjoint rings of sizes 1 (a self-loop), 2, 3, .. and acyclic single end points between them,
           forward links between some of them; the closure in closed form (a ring reaches itself and what
           the links' closure over the handful of rings says); the end points permuted, so that members and
           representatives are not contiguous
  corner   rings, permuted so that the 2-ring sits at the end points 0 and n - 1 -- its only partner cells
           are (0, n - 1), the last valid cell of a row's last word, and (n - 1, 0), the first cell of a
           word -- and the 3-ring at 1, the first cell of the last bit-word, and n - 2
  closure  a random sparse graph, n <= 300, with a 2-cycle and an end point without out-edges forced in,
           closed on the host by repeated boolean products
  raw      uniform random codes from all four ConnActions: not transitive; the any-input definition, n_broken
  dup      rings over half as many end points, listed with repeats
assert_inputs() holds the inputs themselves: rings, corner and closure have at least two zones, one of more
than one member and one acyclic singleton wherever n >= 8; raw has n_broken > 0 at n >= 64; every transitive
family has n_broken == 0.

run_host / check hold a backend (the host twin here, the device in test_gpu_zones.py) against expected():
every output is prefilled with 0xFF.., a guard of 3 entries behind each output must stay untouched, as must
the entries past n_zones, the words past the used part of out_dag and every output that was not given; the
variants are out_zone alone, without dag and without counts.
"""
import collections
import ctypes as C

import numpy as np

import closure_cases as cc
import diff_cases as dc
from vpp_amd import _capi
from vpp_amd._capi import lib

ALLOW = 2
FAMILIES = ("empty", "full", "chain", "rings", "corner", "closure", "raw", "dup")
TRANSITIVE = ("empty", "full", "chain", "rings", "corner", "closure", "dup")
CLOSURE_MAX_N = 300
SCC_MAX_EDGES = 200000   # scc() is plain Python: a one-hop graph above this is not walked
FILL = 0xFFFFFFFF
GUARD = 3   # prefilled entries behind every output that must stay untouched
NAMES = ("zone", "rep", "size", "reaches", "reached_by", "dag")

Out = collections.namedtuple("Out", NAMES + ("result",))


def row_words(n):
    return (n + 15) // 16


def pack(codes):
    """uint8 codes [rows, cols] -> packed words, padding zero (diff_cases.pack_wide, a block of rows at a
    time: a matrix of 2^13 rows stays small on the way)"""
    if codes.shape[0] == 0:
        return np.zeros((0, row_words(codes.shape[1])), np.uint32)
    return np.concatenate([dc.pack_wide(codes[r:r + 512]) for r in range(0, codes.shape[0], 512)])


def expected(codes):
    """Out of uint8 codes [n, n], by numpy: the definitions taken literally; the zone graph as packed words"""
    codes = np.asarray(codes, np.uint8)
    n = codes.shape[0]
    R = codes == ALLOW
    M = R & R.T
    idx = np.arange(n)
    first = np.where(M.any(axis=1), M.argmax(axis=1), n)   # the first set column of every row
    label = np.minimum(first, idx)
    rep = np.unique(label)                                  # the distinct labels, ascending
    zone = np.searchsorted(rep, label)
    size = np.bincount(zone, minlength=len(rep))
    Rr = R[rep]
    res = {"n_zones": len(rep), "n_cyclic": int(R[rep, rep].sum()), "n_multi": int((size > 1).sum()),
           "largest": int(size.max()) if n else 0, "n_broken": int((label[label] != label).sum())}
    u = lambda x: np.asarray(x).astype(np.uint32)
    return Out(u(zone), u(rep), u(size), u(Rr.sum(axis=1)), u(R[:, rep].sum(axis=0)),
               pack(np.where(Rr[:, rep], np.uint8(ALLOW), np.uint8(0))), res)


def scc(n, src, dst):
    """Tarjan, iterative, over the edges src[k] -> dst[k] -> the component of every node as the least
    member of it"""
    order = np.argsort(src, kind="stable")
    dst = np.asarray(dst)[order].tolist()
    start = np.searchsorted(np.asarray(src)[order], np.arange(n + 1)).tolist()
    index, low, comp, on = [-1] * n, [0] * n, [-1] * n, [False] * n
    stack, count = [], 0
    for root in range(n):
        if index[root] >= 0:
            continue
        work = [(root, start[root])]
        index[root] = low[root] = count
        count += 1
        stack.append(root)
        on[root] = True
        while work:
            v, k = work.pop()
            if k < start[v + 1]:
                work.append((v, k + 1))
                w = dst[k]
                if index[w] < 0:
                    index[w] = low[w] = count
                    count += 1
                    stack.append(w)
                    on[w] = True
                    work.append((w, start[w]))
                elif on[w]:
                    low[v] = min(low[v], index[w])
                continue
            if work:
                low[work[-1][0]] = min(low[work[-1][0]], low[v])
            if low[v] == index[v]:
                members = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    members.append(w)
                    if w == v:
                        break
                least = min(members)
                for w in members:
                    comp[w] = least
    return np.array(comp, np.int64)


def close(a):
    """the transitive closure (paths of one edge or more) of a bool matrix, by repeated boolean products"""
    reach = a.copy()
    while True:
        more = reach | cc.product(reach, reach)
        if (more == reach).all():
            return reach
        reach = more


def ring_parts(n):
    """the rings and single end points of `rings` over n end points -> [(size, cyclic), ...] in order: rings
    of sizes 1, 2, 3, .., an acyclic single end point after every second ring, the rest single"""
    parts, left, s = [], n, 1
    while left >= s:
        parts.append((s, True))
        left -= s
        if s % 2 == 0 and left:
            parts.append((1, False))
            left -= 1
        s += 1
    return parts + [(1, False)] * left


def rings(n, g, corner=False):
    """(R bool [n, n], one-hop edges (src, dst)) of the rings family, the end points permuted"""
    parts = ring_parts(n)
    K = len(parts)
    size = np.array([s for s, _ in parts], np.int64)
    cyc = np.array([c for _, c in parts], bool)
    first = np.concatenate([[0], np.cumsum(size)[:-1]])
    part = np.repeat(np.arange(K), size)
    # forward links a -> b (a < b): about two per part; their closure over the K parts
    link = np.triu(g.random((K, K)) < 2.0 / max(K, 1), 1)
    reach = close(link) if K > 1 else link
    reach[np.arange(K), np.arange(K)] = cyc
    # the one-hop graph: every ring's cycle, and a link from a random member to a random member
    src = [np.arange(n)[cyc[part]]]
    dst = [(first[part] + (np.arange(n) - first[part] + 1) % size[part])[cyc[part]]]
    la, lb = np.nonzero(link)
    src.append(first[la] + g.integers(0, size[la]))
    dst.append(first[lb] + g.integers(0, size[lb]))
    src, dst = np.concatenate(src), np.concatenate(dst)
    perm = g.permutation(n)   # old index -> new index
    if corner and n >= 8:
        # the 2-ring (old 1, 2) to 0 and n - 1; the 3-ring (old 4, 5, 6) to 1, the last bit-word's first cell, n - 2
        assert parts[:4] == [(1, True), (2, True), (1, False), (3, True)]
        mid = 32 * ((n - 3) // 32)
        mid = mid if mid > 1 else 2
        fixed = {1: 0, 2: n - 1, 4: 1, 5: mid, 6: n - 2}
        assert len(set(fixed.values())) == 5
        rest = [p for p in g.permutation(n).tolist() if p not in set(fixed.values())]
        perm = np.empty(n, np.int64)
        it = iter(rest)
        for old in range(n):
            perm[old] = fixed[old] if old in fixed else next(it)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    R = reach[part[inv]][:, part[inv]]
    return R, (perm[src], perm[dst])


class Synthetic:
    def __init__(self, n, family, seed=0):
        g = np.random.default_rng([seed, n, FAMILIES.index(family)])
        self.n, self.family = n, family
        self.edges = None   # the one-hop graph (src, dst), where the family has one
        i = np.arange(n)
        if family == "raw":
            codes = g.integers(0, 4, (n, n)).astype(np.uint8)
        else:
            if family == "empty":
                R, self.edges = np.zeros((n, n), bool), (i[:0], i[:0])
            elif family == "full":
                R = np.ones((n, n), bool)
                self.edges = tuple(x.ravel() for x in np.indices((n, n))) if n * n <= SCC_MAX_EDGES else None
            elif family == "chain":
                R, self.edges = np.triu(np.ones((n, n), bool), 1), (i[:-1], i[1:])
            elif family in ("rings", "corner"):
                R, self.edges = rings(n, g, corner=family == "corner")
            elif family == "dup":
                m = (n + 1) // 2
                base, _ = rings(m, g)
                pick = g.integers(0, max(m, 1), n)
                R = base[pick][:, pick]
                # (a ring's other members may not be listed: the graph Tarjan walks is the listed closure itself)
                self.edges = np.nonzero(R)
            else:
                assert family == "closure" and n <= CLOSURE_MAX_N, (family, n)
                a = g.random((n, n)) < 1.2 / max(n, 1)
                if n >= 8:
                    a[0, 1] = a[1, 0] = True   # a zone of two
                    a[2, :] = False            # an end point on no cycle
                R, self.edges = close(a), np.nonzero(a)
            other = np.array([0, 1, 3], np.uint8)[g.integers(0, 3, (n, n), dtype=np.uint8)]
            codes = np.where(R, np.uint8(ALLOW), other)
        self.codes = np.ascontiguousarray(codes, np.uint8)
        self.words = pack(self.codes)
        self._want = None

    @property
    def want(self):
        if self._want is None:
            self._want = expected(self.codes)
        return self._want


def synthetic(n, family, seed=0):
    return Synthetic(n, family, seed)


def assert_inputs(s):
    """no test passes on a degenerate input"""
    w, r, n = s.want, s.want.result, s.n
    assert n == 0 or (w.zone[0] == 0 and (np.diff(w.rep.astype(np.int64)) > 0).all() and int(w.size.sum()) == n)
    if s.family in TRANSITIVE:
        assert r["n_broken"] == 0, (s.family, n, r)
        if s.edges is not None and len(s.edges[0]) <= SCC_MAX_EDGES:
            comp = scc(n, *s.edges)
            assert (comp == w.rep[w.zone].astype(np.int64)).all(), (s.family, n, "Tarjan over the one-hop graph disagrees")
    if s.family == "empty":
        assert r["n_zones"] == n and r["n_cyclic"] == 0
    if s.family == "full":
        assert r["n_zones"] == min(n, 1) and r["n_cyclic"] == min(n, 1)
    if s.family == "chain":
        assert r["n_zones"] == n and r["n_cyclic"] == 0 and r["largest"] == min(n, 1)
    if s.family in ("rings", "corner", "closure") and n >= 8:
        acyclic_single = int(((w.size == 1) & (s.codes[w.rep, w.rep] != ALLOW)).sum())
        assert r["n_zones"] >= 2 and r["n_multi"] >= 1 and acyclic_single >= 1, (s.family, n, r)
    if s.family == "corner" and n >= 8:
        assert w.zone[0] == w.zone[n - 1] == 0 and w.size[0] == 2 and w.zone[1] == w.zone[n - 2] == 1 and w.size[1] == 3
    if s.family == "raw" and n >= 64:
        assert r["n_broken"] > 0, (n, r)


# ---- running a backend ---------------------------------------------------------------------------
def sizes(n):
    """entries of (zone, rep, size, reaches, reached_by, dag) without their guards"""
    return n, n, n, n, n, n * row_words(n)


def buffers(n):
    """the six prefilled outputs with their guards"""
    return [np.full(k + GUARD, FILL, np.uint32) for k in sizes(n)]


def given(reps=True, sizes=True, counts=True, dag=True):
    """which of the six outputs a variant hands over"""
    return True, reps or dag, sizes, counts, counts, dag


def finish(bufs, n, flags, res):
    """the guards and the untouched entries of a run's buffers -> Out (None for what was not given)"""
    nz = res.n_zones
    used = (n, nz, nz, nz, nz, nz * row_words(nz))
    out = []
    for buf, k, name, flag in zip(bufs, used, NAMES, flags):
        if not flag:
            assert (buf == FILL).all(), name + " was written though it was not given"
            out.append(None)
            continue
        assert (buf[k:] == FILL).all(), name + ": an entry past the used ones, or the guard, was written"
        out.append(buf[:k].copy())
    if out[5] is not None:
        out[5] = out[5].reshape(nz, row_words(nz))
    return Out(*out, {"n_zones": nz, "n_cyclic": res.n_cyclic, "n_multi": res.n_multi, "largest": res.largest,
                      "n_broken": res.n_broken})


def spec_of(matrix_ptr, n):
    return _capi.pg_reach_zones_spec(matrix_ptr, n)


def run_host(e, words, n, reps=True, sizes=True, counts=True, dag=True):
    """pg_debug_reach_zones_host over prefilled outputs with guards -> Out"""
    m = np.ascontiguousarray(words, np.uint32)
    bufs = buffers(n)
    flags = given(reps, sizes, counts, dag)
    res = _capi.pg_reach_zones_result(FILL, FILL, FILL, FILL, FILL)
    spec = spec_of(m.ctypes.data if m.size else None, n)
    ptrs = [b.ctypes.data_as(C.c_void_p) if f else None for b, f in zip(bufs, flags)]
    code = lib.pg_debug_reach_zones_host(e.h, C.byref(spec), *ptrs, C.byref(res))
    assert code == 0, lib.pg_last_error(e.h)
    return finish(bufs, n, flags, res)


def same(got, want, what):
    """a run's Out against expected()'s, on whatever the run was given"""
    for name in NAMES:
        g, w = getattr(got, name), getattr(want, name)
        if g is None:
            continue
        assert g.shape == w.shape and (g == w).all(), (what, name, np.argwhere(g != w)[:3].tolist() if g.shape == w.shape else (g.shape, w.shape))
    assert got.result == want.result, (what, got.result, want.result)


def identical(a, b, what):
    """two runs byte for byte"""
    for x, y, name in zip(a[:6], b[:6], NAMES):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), (what, name)
    assert a.result == b.result, (what, a.result, b.result)


VARIANTS = ({"reps": False, "sizes": False, "counts": False, "dag": False}, {"dag": False}, {"counts": False})


def check(run, s, words=None, variants=True):
    """`run(words, n, reps=, sizes=, counts=, dag=)` (run_host's contract without the engine) against numpy
    on the Synthetic s; words: another packing of s.codes (garbage in the padding). -> the full run's Out"""
    w = s.words if words is None else words
    what = (s.family, s.n)
    assert_inputs(s)
    full = run(w, s.n)
    same(full, s.want, what)
    if variants:
        for kw in VARIANTS:
            same(run(w, s.n, **kw), s.want, what + (str(kw),))
    return full


# ---- real engines ------------------------------------------------------------------------------
def graph_want(codes):
    """(the zone of every end point as its least member by Tarjan over the one-hop ALLOW graph of the
    oracle's codes [n_svc, n, n], expected() of that graph's closure)"""
    hop = (np.asarray(codes) == ALLOW).any(axis=0)
    comp = scc(hop.shape[0], *np.nonzero(hop))
    want = expected(np.where(close(hop), np.uint8(ALLOW), np.uint8(0)))
    assert (comp == want.rep[want.zone].astype(np.int64)).all() and want.result["n_broken"] == 0
    return comp, want


def wrapper_want(codes, pods):
    """what Engine.reachability_zones returns for `pods`, from the oracle's codes [n_svc, n, n]"""
    from vpp_amd.device import unpack_closure
    _, w = graph_want(codes)
    nz = w.result["n_zones"]
    return ([[p for p, z in zip(pods, w.zone) if z == k] for k in range(nz)], w.reaches, w.reached_by,
            unpack_closure(w.dag, nz))


PODS = dc.PODS + [dc.PODS[1]]   # one pod listed twice


# ---- arguments ---------------------------------------------------------------------------------
def bad_calls(ptr, out):
    """(what, the message's key words, spec or None, the six outputs, result given) of every PG_EINVAL;
    ptr: a matrix, out: an output address"""
    S = _capi.pg_reach_zones_spec
    ok = S(ptr, 4)
    only = (out, None, None, None, None, None)
    return [("null spec", "null spec", None, only, True), ("null result", "result", ok, only, False),
            ("null matrix", "null matrix", S(None, 4), only, True),
            ("null out_zone", "out_zone", ok, (None, out, out, out, out, None), True),
            ("dag without rep", "out_dag needs out_rep", ok, (out, None, None, None, None, out), True),
            ("n", "2^15", S(ptr, (1 << 15) + 1), only, True)]
