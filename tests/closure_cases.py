"""Graphs, engines and expected closures of the reachability-closure tests (test helper).

Shared by tests/test_closure_host.py (pg_debug_reach_closure_host, no GPU) and
tests/test_gpu_closure.py (pg_reach_closure on the device). Expected values come from numpy alone
(Expected: level-wise boolean products on the unpacked ALLOW union of the selected slices) and, for
real engines, from oracle.world.World.conn through reach_cases.oracle_words -- never from the product.

Synthetic inputs (synthetic(n, family, n_svc, seed)): an edge set per family, every edge given to one
random slice (ALLOW there, a random other code in the other slices); non-edge cells hold random codes
from {0, 1, 3}; packed with diff_cases.pack_wide, the padding bits set at random with diff_cases.garbage.
Families: empty, full, chain (i -> i + 1), ring, star (0 <-> every other node), two-cliques (two
cliques of half the nodes and one bridge from the first to the second), sparse (1.5 edges per node),
medium (4 per node), dense (half the cells).

check(run, s) holds a backend (`run`: the host twin here, the device in test_gpu_closure.py) against
Expected: svc_select None, each single slice, two slices and none; max_hops 0, 1, 2, levels - 1,
levels, levels + 1; every combination of the optional outputs; the runs put guard words behind every
prefilled output and assert that they stay untouched, and the expected packed words have zero padding.
Expected's product is an fp32 matrix product, or above 2500 nodes with a small frontier (the star) the OR
of bit-packed rows.

Past 4096 end points (edge_sizes: the plan's tile_cols of 4096 and of 2^15 end points at -1, 0, +1) the
inputs are built without n x n codes. Islands(n): five islands of 48 nodes with about 3 random edges per
node inside and a bridge from each to the next, every other node isolated, placed across the kernel's
cuts (island_starts); its expected closure is Expected on the 240 island nodes scattered into n x n
(Embedded), and check_walk_shape holds the reference alone to what makes the walk non-trivial.
LargeMedium(n): 4 random edges per node; its closure is n^3 work per level and comes from the caller's
reference. large_runs are the runs of such a graph, LARGE_WANT the references' numbers.

The chain policy (chain(extra)): 12 local pods c0..c11 at 10.40.0.1 + k on tap k; out-tap k reflects
TCP 80 from c(k-1), in-tap k reflects TCP 80 to c(k+1), both end in DENY; an extra edge (a, b) is a
REFLECT of UDP 53 ahead of the DENYs of out-tap b and in-tap a. The graph is the path c0 -> .. -> c11
on service 0 and the extra edges on service 1; service 2 (TCP 81) has no edge.
"""
import ctypes as C
import functools

import numpy as np

import diff_cases as dc
import node_matrix as nm
import reach_cases as rc
from oracle.world import World
from vpp_amd import _capi
from vpp_amd._capi import lib

ALLOW = 2
SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 100, 257)
FAMILIES = ("empty", "full", "chain", "ring", "star", "two-cliques", "sparse", "medium", "dense")
SEEDED = FAMILIES + ("islands",)   # (a family's place here goes into its generator's seed)
FILL = 0xFFFFFFFF
GUARD = 3   # prefilled words behind every output that must stay untouched


def row_words(n):
    return (n + 15) // 16


def edges(n, family, g):
    """the bool edge matrix [n, n] of a family"""
    e = np.zeros((n, n), bool)
    i = np.arange(n)
    if family == "full":
        e[:] = True
    elif family in ("chain", "ring"):
        e[i[:-1], i[1:]] = True
        if family == "ring":
            e[n - 1, 0] = True
    elif family == "star":
        e[0, 1:] = e[1:, 0] = True
    elif family == "two-cliques":
        h = n // 2
        e[:h, :h] = e[h:, h:] = True
        e[i, i] = False
        if 0 < h < n:
            e[h - 1, h] = True
    elif family in ("sparse", "medium", "dense"):
        e = g.random((n, n)) < {"sparse": 1.5 / n, "medium": 4.0 / n, "dense": 0.5}[family]
    elif family == "islands":
        starts = island_starts(n)
        for k, s in enumerate(starts):
            e[s:s + ISLAND, s:s + ISLAND] = g.random((ISLAND, ISLAND)) < 3.0 / ISLAND
            if k:
                e[starts[k - 1] + ISLAND - 1, s] = True   # the bridge from the island before
    else:
        assert family == "empty", family
    return e


ISLANDS, ISLAND = 5, 48


def island_starts(n):
    """where the islands of n nodes begin, ascending: at node 0, 24 nodes ahead of columns 2048, 4096 and
    8192 (the cuts of the closure's chunks, lane widths and column tiles) where an island fits there in
    front of the last one, and the last 48 nodes; an island that does not fit goes into the middle of
    the widest gap, 8 columns behind a multiple of 32"""
    assert n >= 2 * ISLANDS * ISLAND, n
    last = n - ISLAND
    starts = [0] + [c - ISLAND // 2 for c in (2048, 4096, 8192) if c + ISLAND // 2 <= last] + [last]
    while len(starts) < ISLANDS:
        gap, at = max((b - (a + ISLAND), a + ISLAND) for a, b in zip(starts, starts[1:]))
        s = (at + (gap - ISLAND) // 2) // 32 * 32 + 8
        assert at <= s and s + ISLAND <= at + gap, (n, starts)
        starts = sorted(starts + [s])
    return starts


def island_nodes(n):
    return np.concatenate([np.arange(s, s + ISLAND) for s in island_starts(n)])


class Synthetic:
    def __init__(self, n, family, n_svc=3, seed=0):
        g = np.random.default_rng([seed, n, SEEDED.index(family), n_svc])
        self.n, self.n_svc, self.family = n, n_svc, family
        e = edges(n, family, g)
        owner = g.integers(0, n_svc, (n, n), dtype=np.uint8)
        other = np.array([0, 1, 3], np.uint8)[g.integers(0, 3, (n_svc, n, n), dtype=np.uint8)]
        self.codes = np.where(e[None] & (owner[None] == np.arange(n_svc)[:, None, None]), np.uint8(ALLOW), other)
        assert ((self.codes == ALLOW).sum(axis=0) == e).all()   # every edge in exactly one slice
        self.words = np.stack([dc.garbage(dc.pack_wide(self.codes[v]), n, seed + 1 + v) for v in range(n_svc)])

    @functools.lru_cache(maxsize=None)
    def expected(self, select=None):
        return Expected(self.codes, select)


def synthetic(n, family, n_svc=3, seed=0):
    return Synthetic(n, family, n_svc, seed)


class Expected:
    """the closure of the ALLOW union of the slices `select` (a tuple of indices; None = all) of uint8
    codes [n_svc, n, n], by level-wise boolean products"""

    def __init__(self, codes, select=None):
        codes = np.asarray(codes)
        n = codes.shape[1]
        sel = list(range(codes.shape[0])) if select is None else list(select)
        a = (codes[sel] == ALLOW).any(axis=0) if sel else np.zeros((n, n), bool)
        self.n, self.edges = n, a
        self.hops = a.astype(np.uint16)
        reach, front, level = a.copy(), a, int(a.any())
        while front.any() and not reach.all():
            front = product(front, a) & ~reach
            if not front.any():
                break
            level += 1
            self.hops[front] = level
            reach |= front
        self.levels = level

    def at(self, max_hops=0):
        """(reach bool, hops u16, counts u32, result dict) under max_hops"""
        hops = self.hops if not max_hops else np.where(self.hops <= max_hops, self.hops, 0).astype(np.uint16)
        reach = hops > 0
        res = {"levels": int(hops.max()) if hops.size else 0, "n_edges": int(self.edges.sum()), "n_reachable": int(reach.sum())}
        return reach, hops, reach.sum(axis=1).astype(np.uint32), res


def product(front, a):
    """the boolean product front (x) a: as an fp32 matrix product (sums below 2^24: exact), or for a large
    graph with a small frontier as the OR of a's bit-packed rows, row by row"""
    n = a.shape[0]
    if n <= 2500 or int(front.sum()) * n > 1 << 30:
        return (front.astype(np.float32) @ a.astype(np.float32)) > 0
    bits = np.packbits(a, axis=1)
    out = np.zeros_like(bits)
    for i in np.flatnonzero(front.any(axis=1)):
        out[i] = np.bitwise_or.reduce(bits[front[i]], axis=0)
    return np.unpackbits(out, axis=1, count=n).astype(bool)


# ---- past 4096 end points ------------------------------------------------------------------------
class Embedded:
    """Expected's interface for a closure `sub` over the nodes `idx` of an n-node graph whose other
    nodes are isolated: sub's matrices scattered into n x n ones"""

    def __init__(self, sub, idx, n):
        self.n, self.levels, self.idx = n, sub.levels, idx
        self.edges = np.zeros((n, n), bool)
        self.hops = np.zeros((n, n), np.uint16)
        self.edges[np.ix_(idx, idx)] = sub.edges
        self.hops[np.ix_(idx, idx)] = sub.hops

    at = Expected.at


class Islands(Synthetic):
    """the family "islands" at n end points: every edge lies among the 240 island nodes, so the closure
    of a selection is Expected on the 240-node subgraph (`sub`, its codes), embedded. Synthetic's inputs
    without n x n codes: every edge in one random slice, the other cells random codes from {0, 1, 3}"""

    def __init__(self, n, n_svc=3, seed=0):
        g = np.random.default_rng([seed, n, SEEDED.index("islands"), n_svc])
        self.n, self.n_svc, self.family, self.codes = n, n_svc, "islands", None
        self.idx = idx = island_nodes(n)
        e = edges(n, "islands", g)
        assert e.sum() == e[np.ix_(idx, idx)].sum()
        e = e[np.ix_(idx, idx)]
        owner = g.integers(0, n_svc, e.shape, dtype=np.uint8)
        # random words, their ALLOW cells (2) turned into 3; the island rows are then packed from codes
        w = g.integers(0, 1 << 32, (n_svc, n, row_words(n)), dtype=np.uint64).astype(np.uint32)
        w |= (w >> 1) & ~w & np.uint32(0x55555555)
        rows = ((w[:, idx, :, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).reshape(n_svc, len(idx), -1)[:, :, :n].astype(np.uint8)
        self.sub = np.where(e[None] & (owner[None] == np.arange(n_svc)[:, None, None]), np.uint8(ALLOW), rows[:, :, idx])
        rows[:, :, idx] = self.sub
        for v in range(n_svc):
            w[v, idx] = dc.pack_wide(rows[v])
        pad = np.uint32(0xFFFFFFFF >> (2 * (-n & 15)))   # the cells of a row's last word
        allow = (w >> 1) & ~w & np.uint32(0x55555555)
        allow[:, :, -1] &= pad
        pop8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1)
        assert int(pop8[allow.view(np.uint8)].sum()) == int((self.sub == ALLOW).sum()) == int(e.sum())   # no ALLOW elsewhere
        self.words = np.stack([dc.garbage(w[v] & np.where(np.arange(row_words(n)) == row_words(n) - 1, pad, np.uint32(0xFFFFFFFF)),
                                          n, seed + 1 + v) for v in range(n_svc)])
        self._expected = {}

    def expected(self, select=None):
        if select not in self._expected:
            self._expected[select] = Embedded(Expected(self.sub, select), self.idx, self.n)
        return self._expected[select]


class LargeMedium:
    """the family "medium" at n end points without n x n codes: every edge in one random slice, the other
    cells random codes from {0, 1, 3}, the padding random. Its closure takes n^3 work per level: the tests
    get it from a reference of their own over edge_matrix(select)"""

    def __init__(self, n, n_svc=3, seed=0, words=True):
        g = np.random.default_rng([seed, n, SEEDED.index("medium"), n_svc])
        self.n, self.n_svc, self.family = n, n_svc, "medium"
        self.i, self.j = np.nonzero(edges(n, "medium", g))
        self.owner = g.integers(0, n_svc, len(self.i))
        if not words:   # (the graph alone)
            return
        w = g.integers(0, 1 << 32, (n_svc, n, row_words(n)), dtype=np.uint64).astype(np.uint32)
        w |= (w >> 1) & ~w & np.uint32(0x55555555)   # (a random ALLOW becomes 3)
        at, shift = (self.owner, self.i, self.j // 16), (2 * (self.j % 16)).astype(np.uint32)
        np.bitwise_and.at(w, at, ~(np.uint32(3) << shift))
        np.bitwise_or.at(w, at, np.uint32(ALLOW) << shift)
        w[:, :, -1] &= np.uint32(0xFFFFFFFF >> (2 * (-n & 15)))
        self.words = np.stack([dc.garbage(w[v], n, seed + 1 + v) for v in range(n_svc)])

    def edge_matrix(self, select=None):
        keep = np.ones(len(self.i), bool) if select is None else np.isin(self.owner, list(select))
        e = np.zeros((self.n, self.n), bool)
        e[self.i[keep], self.j[keep]] = True
        return e


def plan_shape(e, n):
    """(lane_words, col_tiles) of the closure's plan for n end points, from what pg_debug_reach_closure_plan
    gives: a column tile is 64 lanes of lane_words bit-words of 32 columns, the grid row tiles x column tiles"""
    p = e.debug_reach_closure_plan(n)
    assert p["tile_cols"] % 2048 == 0 and p["grid"] % -(-n // p["tile_rows"]) == 0, p
    return p["tile_cols"] // 2048, p["grid"] // -(-n // p["tile_rows"])


def edge_sizes(e):
    """the column tiles of the plans of 4096 and of 2^15 end points, each at -1, 0 and +1: where a lane goes
    from 2 to 4 bit-words, and where a second column of workgroups begins"""
    return tuple(e.debug_reach_closure_plan(m)["tile_cols"] + d for m in (4096, 1 << 15) for d in (-1, 0, 1))


EDGE_PLANS = ((2, 1), (2, 1), (4, 1), (4, 1), (4, 1), (4, 2))   # plan_shape at edge_sizes


def large_runs(levels):
    """(select, max_hops, out_hops, out_count) of the runs of a large closure test: all slices and one slice,
    max_hops 0, 2 and levels - 1, one run without out_hops and one without out_count"""
    return ((None, 0, True, True), ((1,), 0, True, True), (None, 2, True, True), (None, levels - 1, True, True),
            (None, 0, False, True), ((1,), 2, True, False))


LARGE_SEED = 21
# the reference's (edges, reachable, levels) of the large graphs (n, family, seed), all slices, measured on
# the CPU: the islands by Expected on their 240 nodes, medium by Expected's fp32 products
LARGE_WANT = {(4095, "islands", 21): (737, 19463, 14), (4096, "islands", 21): (731, 30521, 24), (4097, "islands", 21): (720, 29971, 29),
              (8191, "islands", 21): (684, 31069, 28), (8192, "islands", 21): (746, 30357, 26), (8193, "islands", 21): (684, 30319, 25),
              (4097, "medium", 21): (16467, 16144251, 14), (8156, "medium", 21): (32737, 63991522, 15),
              (8157, "medium", 21): (32779, 64120079, 14), (8192, "medium", 21): (33057, 64536943, 14),
              (8193, "medium", 21): (32799, 64360456, 15)}


def bit_words(rows):
    """bool [k, n] -> the closure's bit-words u32 [k, ceil(n / 32)]: cell j at bit j % 32 of word j // 32"""
    k, n = rows.shape
    padded = np.zeros((k, -(-n // 32) * 32), bool)
    padded[:, :n] = rows
    return np.packbits(padded, axis=1, bitorder="little").view("<u4")


def walk_shape(x, tile_rows=16):
    """what a closure's level-wise walk looks like, from the expected hops alone: a dict of
    levels; wide / narrow: frontier words (row, 32-column chunk, level) with >= 4 and with 1..3 bits;
    gapped: (16-row tile, level) pairs that need two chunks with an unneeded one between them;
    dead: the least share of row tiles without a frontier over the levels;
    repeats: the share of the non-empty rows of the reach matrix with two equal adjacent non-zero bit-words"""
    rows = np.flatnonzero(x.hops.any(axis=1))
    tiles = -(-x.n // tile_rows)
    out = {"levels": x.levels, "wide": 0, "narrow": 0, "gapped": 0, "dead": 1.0}
    for level in range(1, x.levels + 1):
        f = bit_words(x.hops[rows] == level)
        bits = np.unpackbits(f.view(np.uint8), axis=1).reshape(len(rows), -1, 32).sum(axis=2)
        out["wide"] += int((bits >= 4).sum())
        out["narrow"] += int(((bits >= 1) & (bits <= 3)).sum())
        live = set()
        for t in np.unique(rows // tile_rows):
            need = np.flatnonzero(np.bitwise_or.reduce(f[rows // tile_rows == t], axis=0))
            if len(need):
                live.add(int(t))
                out["gapped"] += int(len(need) >= 2 and (np.diff(need) > 1).any())
        out["dead"] = min(out["dead"], 1.0 - len(live) / tiles)
    r = bit_words(x.hops[rows] > 0)
    same = ((r[:, 1:] == r[:, :-1]) & (r[:, 1:] != 0)).any(axis=1)
    out["repeats"] = float(same.mean()) if len(rows) else 0.0
    return out


def check_walk_shape(x):
    """the preconditions of the large closure tests, on the reference alone: a star fails the last"""
    w = walk_shape(x)
    assert w["levels"] >= 6 and w["wide"] and w["narrow"] and w["gapped"] and w["dead"] > 0.9 and w["repeats"] < 0.1, w
    return w


def pack_reach(reach):
    """bool [n, n] -> the closure's packed words: ALLOW where reachable, DENY_SYN elsewhere, padding zero"""
    return dc.pack_wide(np.where(reach, np.uint8(ALLOW), np.uint8(0)))


def flags(select, n_svc):
    if select is None:
        return None
    f = np.zeros(n_svc, np.uint8)
    f[list(select)] = 1
    return f


def run_host(e, words, n, select=None, max_hops=0, hops=True, counts=True):
    """pg_debug_reach_closure_host over prefilled outputs with guards -> (packed u32 [n, row_words],
    hops u16 [n, n] or None, counts u32 [n] or None, result dict)"""
    m = np.ascontiguousarray(words, np.uint32)
    rw = row_words(n)
    n_svc = m.size // (n * rw)
    pbuf = np.full(n * rw + GUARD, FILL, np.uint32)
    hbuf = np.full(n * n + GUARD, 0xFFFF, np.uint16)
    cbuf = np.full(n + GUARD, FILL, np.uint32)
    f = flags(select, n_svc)
    spec = _capi.pg_reach_closure_spec(m.ctypes.data, n, n_svc, f.ctypes.data if f is not None else None, max_hops)
    res = _capi.pg_reach_closure_result(77, 77, 77)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    code = lib.pg_debug_reach_closure_host(e.h, C.byref(spec), p(pbuf), p(hbuf) if hops else None,
                                           p(cbuf) if counts else None, C.byref(res))
    assert code == 0, lib.pg_last_error(e.h)
    return finish(n, pbuf, hbuf, cbuf, res, hops, counts)


def finish(n, pbuf, hbuf, cbuf, res, hops, counts):
    """the guards of a run's buffers, and the run's return value"""
    rw = row_words(n)
    assert (pbuf[n * rw:] == FILL).all() and (hbuf[n * n:] == 0xFFFF).all() and (cbuf[n:] == FILL).all(), "a guard was written"
    if not hops:
        assert (hbuf == 0xFFFF).all()
    if not counts:
        assert (cbuf == FILL).all()
    return (pbuf[:n * rw].reshape(n, rw), hbuf[:n * n].reshape(n, n) if hops else None, cbuf[:n] if counts else None,
            {"levels": res.levels, "n_edges": res.n_edges, "n_reachable": res.n_reachable})


def same(got, x, max_hops, what):
    """a run's return value against Expected under max_hops"""
    reach, hops, counts, res = x.at(max_hops)
    packed, h, c, r = got
    assert r == res, (what, r, res)
    assert (packed == pack_reach(reach)).all(), (what, rc.mismatch_report(packed[None], pack_reach(reach)[None]))
    assert h is None or (h == hops).all(), (what, "hops", np.argwhere(h != hops)[:3].tolist())
    assert c is None or (c == counts).all(), (what, "counts")


def selections(n_svc):
    return [None] + [(v,) for v in range(n_svc)] + ([(0, n_svc - 1)] if n_svc > 1 else []) + [()]


def hop_bounds(levels):
    return sorted({0, 1, 2} | {k for k in (levels - 1, levels, levels + 1) if k > 0})


def check(run, words, n, expected, n_svc, variants=True):
    """`run(words, n, select, max_hops, hops=, counts=)` (run_host's contract without the engine)
    against `expected(select)` -> Expected"""
    for sel in selections(n_svc) if variants else [None]:
        same(run(words, n, sel, 0), expected(sel), 0, ("select", sel))
    x = expected(None)
    for k in hop_bounds(x.levels):
        same(run(words, n, None, k), x, k, ("max_hops", k))
    if variants:
        for hops, counts in ((False, False), (True, False), (False, True)):
            same(run(words, n, None, 0, hops=hops, counts=counts), x, 0, ("outputs", hops, counts))
            same(run(words, n, (0,), 2, hops=hops, counts=counts), expected((0,)), 2, ("outputs, bounded", hops, counts))


# ---- real engines ------------------------------------------------------------------------------
def oracle_codes(world, ips, services):
    """the oracle's ConnActions [n_svc, n, n] over ips x ips"""
    ips = np.asarray(ips, np.uint32)
    return (rc.oracle_words(world, ips, ips, services) >> 30).astype(np.uint8)


CHAIN_N = 12
CHAIN_SERVICES = [(0, 40000, 80), (1, 40000, 53), (0, 40000, 81)]
CHAIN_PODS = ["ns/c%d" % k for k in range(CHAIN_N)]
CHAIN_IPS = [0x0A280001 + k for k in range(CHAIN_N)]


class Chain:
    """the chain policy with the extra edges `extra`, its engine and its oracle world"""

    def __init__(self, extra=()):
        from vpp_amd import renderer as R
        from vpp_amd import workloads as W
        P, D, RF = 1, 0, 2
        e = R.Engine(0)
        e.SetMainInterfaceName("GbE")
        e.SetVxlanBVIIfName(nm.NODE_IF)
        e.SetHostInterconnectIfName("VPP-Host")
        local = {}
        for k, ip in enumerate(CHAIN_IPS):
            e.SetPodIfName(CHAIN_PODS[k], "tap%d" % k)
            e.RegisterPod(CHAIN_PODS[k], W.ip_str(ip), False)
            local[ip] = "tap%d" % k
        host = lambda k: W.ip_str(CHAIN_IPS[k]) + "/32"
        l4 = lambda p: {"src": [0, 65535], "dst": [p, p]}
        ops = []
        for k in range(CHAIN_N):
            out = [{"action": RF, "src": host(k - 1), "dst": "", "tcp": l4(80)}] if k > 0 else []
            out += [{"action": RF, "src": host(a), "dst": "", "udp": l4(53)} for a, b in extra if b == k]
            inn = [{"action": RF, "src": "", "dst": host(k + 1), "tcp": l4(80)}] if k < CHAIN_N - 1 else []
            inn += [{"action": RF, "src": "", "dst": host(b), "udp": l4(53)} for a, b in extra if a == k]
            deny = [{"action": D, "src": "", "dst": ""}]
            ops.append((dc.KEY + "out-tap%d" % k, {"name": "out-tap%d" % k, "rules": out + deny, "ingress": [],
                                                   "egress": ["tap%d" % k]}))
            ops.append((dc.KEY + "in-tap%d" % k, {"name": "in-tap%d" % k, "rules": inn + deny, "ingress": ["tap%d" % k],
                                                  "egress": []}))
        e.ApplyTxn(True, ops)
        e.num_tables()
        self.e, self.world = e, World(e, local, nm.NODE_IF, no_if_ips=[])
        self.codes = oracle_codes(self.world, CHAIN_IPS, CHAIN_SERVICES)

    @functools.lru_cache(maxsize=None)
    def expected(self, select=None):
        return Expected(self.codes, select)


@functools.lru_cache(maxsize=None)
def chain(extra=()):
    return Chain(extra)


# the oracle's numbers, measured on the CPU: (edges, reachable, levels)
CHAIN_WANT = {((), (0,)): (11, 66, 11), (((11, 0),), (0, 1)): (12, 144, 12), (((11, 0), (3, 9)), (0, 1)): (13, 144, 12),
              ((), (2,)): (0, 0, 0)}
# fixture change (diff_cases.MATRIX_EDIT) over c.dst x c.dst: (edges, reachable) before and after
FIXTURE_WANT = {"svc0": ((829, 1081), (1171, 1927)), "all": ((1669, 2209), (1669, 2209)), "hop2_svc0_before": 252,
                "hop2_all": 540, "closure_opened": 984, "closure_closed": 138, "one_hop_opened": 444, "one_hop_closed": 102}
# node_matrix topologies over rc.sides(t, 64, 53)[0] on both sides, all of rc.services: (edges, reachable)
TOPOLOGY_WANT = {"small": (1166, 2610), "grouped": (76, 331), "uncovered": (1443, 2809), "pair": (1430, 2916)}


@functools.lru_cache(maxsize=None)
def fixture_change():
    """diff_cases.Change(MATRIX_EDIT) with the oracle's codes over c.dst x c.dst, (before, after)"""
    c = dc.Change(dc.MATRIX_EDIT)
    c.closure_codes = tuple(oracle_codes(w, c.dst, dc.SERVICES) for w in (c.w0, c.w1))
    return c


@functools.lru_cache(maxsize=None)
def topology(name):
    """(engine, end points [64], services, the oracle's codes) of a node_matrix topology"""
    t = nm.topo(name)
    ips = rc.sides(t, 64, 53)[0]
    svc = rc.services(t.e)
    return t.e, ips, svc, oracle_codes(t.world, ips, svc)
