"""Flow batches, lists and expected results of the observed-reachability tests (test helper).

Shared by tests/test_observed_host.py (pg_debug_reach_observed_host, no GPU) and tests/test_gpu_observed.py
(pg_reach_observed on the device). Expected values come from numpy alone -- expected(): the semantics of
include/policygpu.h taken literally: a boolean service x flow match matrix from the protocol and port
rules, the listed addresses found by searchsorted over the sorted distinct addresses, the status from
"first that applies", a boolean n_svc x n_src x n_dst array marked through the distinct addresses and
expanded to the lists (so every duplicate counts), packed at the end -- never from the product.

A Case is two lists, the services (protocol, src port, dst port), whether the src port counts, and the
flows (src, dst, src port, dst port, proto). random_case() draws flows of the four statuses on purpose
(a listed or an unlisted src / dst, a service's own protocol and ports or a near miss); assert_inputs()
then holds the case itself, from expected() alone: each status has at least 5 % of the flows, every
service has a matched flow, and between 10 % and 90 % of the cells end up ALLOW. A matrix of fewer than
20 cells cannot meet the cell bounds in general (one cell is 0 % or 100 %): there the bounds are "some
cell ALLOW", and the seeds were chosen on the CPU so that all of this holds.

run_host / the device's runner hold a backend against expected(): every output is written over a
prefilled buffer, a guard of 3 entries behind each must stay untouched, out_flow starts at an odd byte.
The scenario functions below (rows_and_words .. empties) take such a runner and the engine whose knobs,
plan and probe they use; both test files call them, so the CPU suite runs the host twin over the cases
the GPU suite runs the device over.
"""
import collections
import ctypes as C

import numpy as np

import diff_cases as dc
from vpp_amd import _capi
from vpp_amd._capi import lib

ALLOW = 2
MATCHED, NO_SRC, NO_DST, NO_SVC = 0, 1, 2, 3
ACCUMULATE, MATCH_SRC_PORT = 1, 2
TCP, UDP, OTHER, ANY = 0, 1, 2, 3
FILL = 0xFFFFFFFF
GUARD = 3
N_DST = (1, 15, 16, 17, 31, 32, 33)
N_SRC = (1, 2, 65)
N_SVC = (1, 3)

Out = collections.namedtuple("Out", "packed flow svc_flows result")
Case = collections.namedtuple("Case", "src dst services match flows")


def row_words(n):
    return (n + 15) // 16


def u32(x):
    return np.ascontiguousarray(x, np.uint32)


def case(src, dst, services, flows, match=False):
    s, d, sp, dp, pr = flows
    return Case(u32(src), u32(dst), list(services), bool(match),
                (u32(s), u32(d), np.ascontiguousarray(sp, np.uint16), np.ascontiguousarray(dp, np.uint16),
                 np.ascontiguousarray(pr, np.uint8)))


def prefix(c, n):
    """the first n flows of a case"""
    return c._replace(flows=tuple(a[:n] for a in c.flows))


def part(c, lo, hi):
    return c._replace(flows=tuple(a[lo:hi] for a in c.flows))


# ---- the reference ------------------------------------------------------------------------------
def lookup(addresses, ips):
    """(the distinct addresses sorted, the distinct id of every list entry, the distinct id of every ip or -1)"""
    distinct, inv = np.unique(addresses, return_inverse=True)
    if len(distinct) == 0:
        return distinct, inv, np.full(len(ips), -1, np.int64)
    at = np.searchsorted(distinct, ips)
    at = np.where(at < len(distinct), at, 0)
    return distinct, inv, np.where(distinct[at] == ips, at, -1)


def matches(c):
    """bool [n_svc, n]: service v matches flow t"""
    _, _, sport, dport, proto = c.flows
    fp = np.minimum(proto.astype(np.int64), 3)
    M = np.zeros((len(c.services), len(fp)), bool)
    for v, (p, sp, dp) in enumerate(c.services):
        p = min(int(p) & 0xFFFFFFFF, 3)
        m = fp == p
        if p in (TCP, UDP):
            m = m & (dport == dp)
            if c.match:
                m = m & (sport == sp)
        M[v] = m
    return M


def expected(c, into=None):
    """Out of a case by numpy; into: packed words the result is ORed into (ACCUMULATE)"""
    fs, fd = c.flows[0], c.flows[1]
    n, nv, ns, nd = len(fs), len(c.services), len(c.src), len(c.dst)
    sdist, sinv, sid = lookup(c.src, fs)
    ddist, dinv, did = lookup(c.dst, fd)
    M = matches(c)
    status = np.where(sid < 0, NO_SRC, np.where(did < 0, NO_DST, np.where(~M.any(axis=0), NO_SVC, MATCHED))).astype(np.uint8)
    ok = status == MATCHED
    cube = np.zeros((nv, len(sdist), len(ddist)), bool)
    for v in range(nv):
        k = ok & M[v]
        cube[v, sid[k], did[k]] = True
    cells = cube[:, sinv][:, :, dinv] if ns and nd else np.zeros((nv, ns, nd), bool)
    rw = row_words(nd)
    if ns and nd:
        packed = dc.pack_wide(np.where(cells, np.uint8(ALLOW), np.uint8(0)).reshape(nv * ns, nd)).reshape(nv, ns, rw)
    else:
        packed = np.zeros((nv, ns, rw), np.uint32)
    if into is not None:
        packed = packed | np.asarray(into, np.uint32).reshape(packed.shape)
    codes = (packed[..., None] >> (2 * np.arange(16, dtype=np.uint32))) & 3
    res = {"n_matched": int(ok.sum()), "n_no_src": int((status == NO_SRC).sum()), "n_no_dst": int((status == NO_DST).sum()),
           "n_no_svc": int((status == NO_SVC).sum()), "n_cells": int((codes == ALLOW).sum())}
    if not ns or not nd:
        res = dict.fromkeys(res, 0)
    return Out(packed, status, (M & ok).sum(axis=1).astype(np.uint64), res)


def assert_inputs(c, want=None):
    """no test passes on a degenerate batch: from the reference alone"""
    w = expected(c) if want is None else want
    n, r = len(c.flows[0]), w.result
    for name in ("n_matched", "n_no_src", "n_no_dst", "n_no_svc"):
        assert 20 * r[name] >= n, (name, r, n)
    assert (w.svc_flows > 0).all(), w.svc_flows
    cells = len(c.services) * len(c.src) * len(c.dst)
    if cells >= 20:
        assert cells <= 10 * r["n_cells"] and 10 * r["n_cells"] <= 9 * cells, (r["n_cells"], cells)
    else:
        assert r["n_cells"] >= 1


# ---- cases --------------------------------------------------------------------------------------
SERVICES = [(TCP, 40000, 80), (UDP, 40000, 53), (OTHER, 0, 0), (ANY, 1234, 80), (TCP, 40001, 80), (TCP, 40000, 443),
            (255, 7, 7), (UDP, 5, 65535), (TCP, 0, 0), (4, 0, 1), (UDP, 40000, 1), (TCP, 9, 65535)]
NEAR_PORTS = np.array([0, 1, 65535, 52, 54, 79, 81, 442, 444, 65534, 2], np.uint16)


def addresses(g, n, dup=0.2):
    """n listed addresses: distinct random ones, about `dup` of the entries repeats of earlier ones"""
    pool = g.choice(1 << 32, size=max(1, n), replace=False).astype(np.uint32)
    pick = np.arange(n)
    rep = g.random(n) < dup
    pick[rep] = g.integers(0, np.maximum(1, np.arange(n)))[rep]
    return pool[pick]


def outside(g, listed, k):
    """k addresses not in `listed`: random ones and the neighbours of listed ones"""
    near = np.concatenate([listed + np.uint32(1), listed - np.uint32(1)]) if len(listed) else np.zeros(0, np.uint32)
    cand = np.concatenate([g.integers(0, 1 << 32, 2 * k + 8, dtype=np.uint64).astype(np.uint32), near])
    cand = cand[~np.isin(cand, listed)]
    return cand[g.integers(0, len(cand), k)]


def random_flows(g, src, dst, services, n, match, active=0.7, mix=(0.55, 0.15, 0.15, 0.15)):
    """n flows over the lists: by `mix` matched, with an unlisted src, an unlisted dst, off every service;
    the listed ones from the first `active` of each list"""
    kind = g.choice(4, size=n, p=mix)
    act = lambda a: a[:max(1, int(active * len(a)))]
    fs = act(src)[g.integers(0, len(act(src)), n)]
    fd = act(dst)[g.integers(0, len(act(dst)), n)]
    fs = np.where(kind == NO_SRC, outside(g, src, n), fs)
    fd = np.where(kind == NO_DST, outside(g, dst, n), fd)
    v = g.integers(0, len(services), n)
    sp = np.array([s[1] for s in services], np.uint16)[v]
    dp = np.array([s[2] for s in services], np.uint16)[v]
    pr = np.array([min(int(s[0]), 255) for s in services], np.uint8)[v]
    # a service of protocol >= 3 is met by every code >= 3; its ports do not count, nor do OTHER's
    high = pr >= 3
    pr = np.where(high, np.array([3, 4, 255, 77], np.uint8)[g.integers(0, 4, n)], pr)
    free = high | (pr == OTHER)
    dp = np.where(free, g.integers(0, 1 << 16, n).astype(np.uint16), dp)
    sp = np.where(free | (not match), g.integers(0, 1 << 16, n).astype(np.uint16), sp)
    # off every service: a near port (the reference says whether it really misses)
    miss = kind == NO_SVC
    dp = np.where(miss, NEAR_PORTS[g.integers(0, len(NEAR_PORTS), n)], dp)
    pr = np.where(miss, g.integers(0, 2, n).astype(np.uint8), pr)
    return fs, fd, sp, dp, pr


def random_case(n_src, n_dst, n_svc, n, seed=0, match=False, dup=0.2, active=0.7, services=None):
    g = np.random.default_rng([seed, n_src, n_dst, n_svc, n, int(match)])
    services = SERVICES[:n_svc] if services is None else services
    src, dst = addresses(g, n_src, dup), addresses(g, n_dst, dup)
    return case(src, dst, services, random_flows(g, src, dst, services, n, match, active), match)


# ---- running a backend --------------------------------------------------------------------------
def spec_of(c, flags, keep):
    svc = (_capi.pg_service * max(1, len(c.services)))()
    for i, (p, sp, dp) in enumerate(c.services):
        svc[i].protocol, svc[i].src_port, svc[i].dst_port = int(np.int32(np.uint32(p & 0xFFFFFFFF))), int(sp), int(dp)
    keep.extend([svc, c.src, c.dst])
    return _capi.pg_reach_observed_spec(c.src.ctypes.data if len(c.src) else None, len(c.src),
                                        c.dst.ctypes.data if len(c.dst) else None, len(c.dst), svc, len(c.services), flags)


def flags_of(c, into):
    return (MATCH_SRC_PORT if c.match else 0) | (ACCUMULATE if into is not None else 0)


def n_words(c):
    return len(c.services) * len(c.src) * row_words(len(c.dst))


def finish(c, packed, flow, svc, res, given_flow, given_svc):
    """the guards of a run's buffers (numpy copies of them, out_flow from its odd start) -> Out"""
    n, nv, nw = len(c.flows[0]), len(c.services), n_words(c)
    assert (packed[nw:] == FILL).all(), "out_packed: the guard was written"
    assert (flow[n:] == 0xEE).all() and (given_flow or (flow == 0xEE).all()), "out_flow: the guard, or a buffer not given, was written"
    assert (svc[nv:] == np.uint64(0xEEEEEEEEEEEEEEEE)).all() and (given_svc or (svc == np.uint64(0xEEEEEEEEEEEEEEEE)).all()), "out_svc_flows"
    return Out(packed[:nw].reshape(nv, len(c.src), row_words(len(c.dst))).copy(), flow[:n].copy() if given_flow else None,
               svc[:nv].copy() if given_svc else None,
               {k: int(getattr(res, k)) for k in ("n_matched", "n_no_src", "n_no_dst", "n_no_svc", "n_cells")})


def run_host(e, c, into=None, flow=True, svc=True, sport=None):
    """pg_debug_reach_observed_host over prefilled outputs with guards -> Out. sport: False hands a null
    src_port over (only without MATCH_SRC_PORT)"""
    keep = []
    spec = spec_of(c, flags_of(c, into), keep)
    n, nw = len(c.flows[0]), n_words(c)
    packed = np.full(nw + GUARD, FILL, np.uint32)
    if into is not None:
        packed[:nw] = np.asarray(into, np.uint32).ravel()
    fbuf = np.full(n + GUARD + 1, 0xEE, np.uint8)
    sbuf = np.full(len(c.services) + GUARD, 0xEEEEEEEEEEEEEEEE, np.uint64)
    res = _capi.pg_reach_observed_result(7, 7, 7, 7, 7)
    with_sport = c.match if sport is None else sport
    soa = _capi.pg_tuple_soa(*[a.ctypes.data if (i != 2 or with_sport) else None for i, a in enumerate(c.flows)])
    code = lib.pg_debug_reach_observed_host(e.h, C.byref(spec), C.byref(soa) if n else None, n, packed.ctypes.data,
                                            fbuf[1:].ctypes.data if flow else None, sbuf.ctypes.data if svc else None,
                                            C.byref(res))
    assert code == 0, lib.pg_last_error(e.h)
    return finish(c, packed, fbuf[1:], sbuf, res, flow, svc)


def same(got, want, what):
    assert got.packed.shape == want.packed.shape and (got.packed == want.packed).all(), (what, "packed", np.argwhere(got.packed != want.packed)[:3].tolist())
    if got.flow is not None:
        assert (got.flow == want.flow).all(), (what, "flow", np.flatnonzero(got.flow != want.flow)[:3].tolist())
    if got.svc_flows is not None:
        assert (got.svc_flows == want.svc_flows).all(), (what, got.svc_flows, want.svc_flows)
    assert got.result == want.result, (what, got.result, want.result)


def identical(a, b, what):
    """two runs byte for byte"""
    for x, y, name in zip(a[:3], b[:3], Out._fields):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), (what, name)
    assert a.result == b.result, (what, a.result, b.result)


def check(run, c, what, variants=False, **kw):
    """`run(case, into=, flow=, svc=, ...)` (run_host's contract without the engine) against numpy -> Out"""
    want = expected(c, kw.get("into"))
    full = run(c, **kw)
    same(full, want, what)
    if variants:
        same(run(c, flow=False, **kw), want, (what, "no flow"))
        same(run(c, svc=False, **kw), want, (what, "no svc"))
        same(run(c, flow=False, svc=False, **kw), want, (what, "packed alone"))
    return full


# ---- scenarios, for both suites -----------------------------------------------------------------
def flow_counts(e, grid=False):
    """0, 1, around a wave, 4 waves + 3, one vector step of a workgroup +- 1; with `grid` a full grid of
    the plan's tiles plus 1 (the plan under the knobs in force)"""
    p = e.debug_reach_observed_plan(2, 17, 1)
    step = p["block"] * p["vec_flows"]
    counts = [0, 1, 63, 64, 65, 4 * 64 + 3, step - 1, step, step + 1]
    return counts + ([p["grid"] * step + 1] if grid else [])


def rows_and_words(run, e, n_dst):
    """n_dst at the word edges x n_src x n_svc: a random batch that meets assert_inputs, and its prefixes
    at the flow-count edges"""
    counts = flow_counts(e)
    for n_src in N_SRC:
        for n_svc in N_SVC:
            c = random_case(n_src, n_dst, n_svc, 8192, seed=1)
            assert_inputs(c)
            check(run, c, (n_src, n_dst, n_svc), variants=n_dst in (17, 33) and n_src == 65)
            for k in counts:
                check(run, prefix(c, k), (n_src, n_dst, n_svc, k))


def full_grid(run, e):
    """one more flow than a full grid of tiles holds, under blocks_per_cu = 1"""
    with e.tuning(blocks_per_cu=1):
        n = flow_counts(e, grid=True)[-1]
        assert n <= (1 << 20), n
        c = random_case(65, 33, 3, n, seed=2)
        assert_inputs(c)
        check(run, c, ("grid", n))


def address_edges(run, e):
    svc = SERVICES[:3]
    g = np.random.default_rng(3)
    # 0.0.0.0 and 255.255.255.255 listed on both sides; flows one below and one above every listed address
    src = u32([0, 0xFFFFFFFF, 0x0A000001, 0x0A000002, 0x0A000004, 0x7FFFFFFF, 0x80000000])
    dst = u32([0xFFFFFFFF, 0, 0x0A000003, 0xC0A80001, 1])
    ends = np.unique(np.concatenate([src, dst, src + np.uint32(1), src - np.uint32(1), dst + np.uint32(1), dst - np.uint32(1)]))
    fs, fd = [x.ravel() for x in np.meshgrid(ends, ends)]
    n = len(fs)
    v = g.integers(0, 3, n)
    flows = (fs, fd, np.zeros(n, np.uint16), np.array([s[2] for s in svc], np.uint16)[v], np.array([s[0] for s in svc], np.uint8)[v])
    c = case(src, dst, svc, flows)
    w = check(run, c, "edges", variants=True)
    assert w.result["n_no_src"] > 0 and w.result["n_no_dst"] > 0 and w.result["n_matched"] > 0
    # 0.0.0.0 and 255.255.255.255 not listed: flows from and to them are unlisted, whatever marks an empty cell
    c2 = case(src[2:], dst[2:], svc, flows)
    w2 = expected(c2)
    assert (w2.flow[(fs == 0) | (fs == 0xFFFFFFFF)] == NO_SRC).all()
    check(run, c2, "edges not listed")
    # a list that is one address repeated
    c3 = case([0x0A000001] * 7, [0x0A000009] * 19, svc, random_flows(g, u32([0x0A000001]), u32([0x0A000009]), svc, 500, False))
    w3 = check(run, c3, "one address")
    assert w3.result["n_cells"] in (7 * 19, 2 * 7 * 19, 3 * 7 * 19)
    # every address three times on both sides, two services with one key: a matched flow marks 18 cells
    base_s, base_d = addresses(g, 11, 0), addresses(g, 13, 0)
    two = [(TCP, 40000, 80), (UDP, 1, 53), (TCP, 40001, 80)]
    c4 = case(np.repeat(base_s, 3)[g.permutation(33)], np.tile(base_d, 3), two, random_flows(g, base_s, base_d, two, 4000, False))
    one = case(c4.src, c4.dst, two, ([base_s[4]], [base_d[5]], [9], [80], [TCP]))
    assert expected(one).result == {"n_matched": 1, "n_no_src": 0, "n_no_dst": 0, "n_no_svc": 0, "n_cells": 18}
    check(run, one, "18 cells")
    assert_inputs(c4)
    check(run, c4, "triples")


def collisions(run, e):
    """lists chosen with the probe: an address found after at least 4 cells and a probe that wraps past the
    table's end -- asserted through the probe, the expected values from numpy as ever"""
    g = np.random.default_rng(4)
    n_list = 24
    cand = np.unique(g.integers(0, 1 << 32, 40000, dtype=np.uint64).astype(np.uint32))
    _, slot, cap = e.debug_reach_observed_probe(cand[:n_list], cand)
    assert cap >= 2 * n_list
    crowd = cap // 2
    chain = cand[slot == crowd][:6]
    tail = cand[slot == cap - 1][:3]
    assert len(chain) >= 5 and len(tail) == 3, (len(chain), len(tail))
    rest = cand[(slot != crowd) & (slot != cap - 1)][:n_list - len(chain) - len(tail)]
    lst = np.concatenate([chain, tail, rest])
    assert len(lst) == n_list
    steps, slot, cap2 = e.debug_reach_observed_probe(lst, lst)
    assert cap2 == cap and steps.max() >= 4 and (slot.astype(np.int64) + steps - 1 >= cap).any(), (steps, slot, cap)
    # an unlisted address that walks a chain before its empty cell
    miss = cand[~np.isin(cand, lst)]
    msteps, _, _ = e.debug_reach_observed_probe(lst, miss)
    assert msteps.max() >= 4
    long_miss = miss[np.argsort(msteps)[-8:]]
    svc = SERVICES[:3]
    for src, dst in ((lst, g.permutation(lst)[:17]), (g.permutation(lst)[:9], lst)):
        fl = list(random_flows(g, src, dst, svc, 6000, False, active=0.6))   # (a list starts with its chain and its wrap)
        fl[0][:64] = np.resize(long_miss, 64)
        fl[1][64:128] = np.resize(long_miss, 64)
        c = case(src, dst, svc, fl)
        assert_inputs(c)
        check(run, c, "collisions")


def service_edges(run, e):
    g = np.random.default_rng(5)
    src, dst = addresses(g, 9), addresses(g, 21)
    # every protocol code 0..3, 4 and 255 in the services; two services that differ only in src_port
    svc = [(TCP, 40000, 80), (TCP, 40001, 80), (UDP, 40000, 80), (OTHER, 5, 80), (ANY, 0, 0), (4, 1, 1), (255, 2, 2),
           (TCP, 40000, 0), (TCP, 40000, 1), (UDP, 40000, 65535)]
    # flows: every protocol code x the ports 0, 1, 65535 and one next to each service's port x two src ports
    ports = sorted({0, 1, 2, 65535, 65534, 79, 80, 81})
    pr, dp, sp = [x.ravel() for x in np.meshgrid([0, 1, 2, 3, 4, 255], ports, [40000, 40001, 7])]
    n = 12 * len(pr)
    pr, dp, sp = np.resize(pr, n), np.resize(dp, n), np.resize(sp, n)
    flows = (src[g.integers(0, 9, n)], dst[g.integers(0, 21, n)], sp, dp, pr)
    outs = {}
    for match in (False, True):
        c = case(src, dst, svc, flows, match)
        w = expected(c)
        assert (w.svc_flows > 0).all() and w.result["n_no_svc"] > 0, w
        outs[match] = check(run, c, ("services", match), variants=True)
    # the two services share every flow without the flag and none with it
    assert outs[False].svc_flows[0] == outs[False].svc_flows[1] > 0
    assert 0 < outs[True].svc_flows[0] < outs[False].svc_flows[0] and 0 < outs[True].svc_flows[1] < outs[False].svc_flows[1]
    # src_port null without the flag
    check(lambda c, **kw: run(c, sport=False, **kw), case(src, dst, svc, flows, False), "null src_port")


def contention(run, e, knobs=True):
    """2^18 flows all on one cell, and on the 16 cells of one word; observed_test_first changes nothing"""
    g = np.random.default_rng(6)
    src, dst = addresses(g, 5, 0), addresses(g, 40, 0)
    n = 1 << 18
    z = np.zeros(n, np.uint16)
    for what, j in (("one cell", np.full(n, 21)), ("one word", 16 + g.integers(0, 16, n))):
        c = case(src, dst, [(TCP, 1, 80)], (np.full(n, src[3]), dst[j], z, z + np.uint16(80), z.astype(np.uint8)))
        w = expected(c)
        assert w.result == {"n_matched": n, "n_no_src": 0, "n_no_dst": 0, "n_no_svc": 0, "n_cells": 1 if what == "one cell" else 16}
        assert np.count_nonzero(w.packed) == 1
        base = check(run, c, what)
        for tf in (0, 1, 2) if knobs else ():
            with e.tuning(observed_test_first=tf):
                identical(run(c), base, (what, tf))


def table_paths(run, e):
    """the address tables staged in LDS and probed in HBM: the same inputs with observed_lds_bytes unset and
    0, and a side just below and just above the largest that the plan stages"""
    c = random_case(65, 33, 3, 8192, seed=1)
    assert_inputs(c)
    p = e.debug_reach_observed_plan(65, 33, 3)
    assert p["src_in_lds"] == 1 and p["dst_in_lds"] == 1, p
    base = check(run, c, "lds")
    with e.tuning(observed_lds_bytes=0):
        p = e.debug_reach_observed_plan(65, 33, 3)
        assert p["src_in_lds"] == 0 and p["dst_in_lds"] == 0 and p["lds_bytes"] == p["svc_bytes"], p
        identical(check(run, c, "hbm"), base, "hbm")
    # only the dst table fits
    with e.tuning(observed_lds_bytes=12 * p["dst_cap"]):
        p = e.debug_reach_observed_plan(65, 33, 3)
        assert p["src_in_lds"] == 0 and p["dst_in_lds"] == 1, p
        identical(check(run, c, "dst alone"), base, "dst alone")
    staged = lambda k, side: e.debug_reach_observed_plan(*((k, 17) if side == 0 else (17, k)), 3)[("src_in_lds", "dst_in_lds")[side]]
    for side in (0, 1):
        lo, hi = 1, 1 << 20
        assert staged(lo, side) and not staged(hi, side)
        while hi - lo > 1:   # (the cells double with the length: staged() falls once)
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if staged(mid, side) else (lo, mid)
        for k in (lo, hi):
            cs = random_case(*((k, 17) if side == 0 else (17, k)), 3, 1 << 16, seed=7, active=0.5)
            assert_inputs(cs)
            check(run, cs, ("threshold", side, k))


def split_launches(run, e):
    """a 1000-flow batch in launches of 64 and of 128 flows gives what one launch gives"""
    c = random_case(65, 33, 3, 1000, seed=1)
    assert_inputs(c)
    base = check(run, c, "one launch")
    for cap in (64, 128):
        with e.tuning(launch_max_tuples=cap):
            identical(check(run, c, ("pieces", cap)), base, ("pieces", cap))


def accumulate(run, e):
    """two halves with ACCUMULATE on the second give the whole batch's matrix; a call without it clears"""
    c = random_case(65, 33, 3, 8192, seed=1)
    whole = check(run, c, "whole")
    first = check(run, part(c, 0, 4096), "first half")
    second_alone = expected(part(c, 4096, 8192))
    both = check(run, part(c, 4096, 8192), "second half into the first", into=first.packed)
    assert (both.packed == whole.packed).all() and both.result["n_cells"] == whole.result["n_cells"]
    assert both.result["n_cells"] > max(first.result["n_cells"], second_alone.result["n_cells"])
    assert (both.svc_flows == second_alone.svc_flows).all()   # (the counts are the call's own flows)
    # n == 0 with ACCUMULATE keeps the matrix and counts it
    kept = check(run, prefix(c, 0), "nothing into the whole", into=whole.packed)
    assert kept.result == {"n_matched": 0, "n_no_src": 0, "n_no_dst": 0, "n_no_svc": 0, "n_cells": whole.result["n_cells"]}


def bad_calls(c, out, flows_ptrs):
    """(what, the message's key words, spec changes, call changes) of every PG_EINVAL. out: an output
    address; flows_ptrs: the five flow arrays' addresses"""
    big = 1 << 20
    return [("null spec", "null spec", "nospec", {}), ("null result", "result", {}, {"result": False}),
            ("null out_packed", "out_packed", {}, {"packed": None}), ("null flows", "null flows", {}, {"flows": None}),
            ("null src_ip field", "src_ip", {}, {"field": 0}), ("null dst_ip field", "dst_ip", {}, {"field": 1}),
            ("null dst_port field", "dst_port", {}, {"field": 3}), ("null proto field", "proto", {}, {"field": 4}),
            ("null src_port with the flag", "src_port", {"flags": MATCH_SRC_PORT}, {"field": 2}),
            ("no service", "n_svc", {"n_svc": 0}, {}), ("4097 services", "n_svc", {"n_svc": 4097}, {}),
            ("src side", "2^20", {"n_src": big + 1}, {}), ("dst side", "2^20", {"n_dst": big + 1}, {}),
            ("2^32 words", "2^32", {"n_src": big, "n_dst": big, "n_svc": 1}, {}),
            ("2^32 words by services", "2^32", {"n_src": big, "n_dst": 16, "n_svc": 4096}, {}),
            ("flag bits", "flag", {"flags": 4}, {}), ("flag bits", "flag", {"flags": 0x80000001}, {}),
            ("null list", "null src_ip, dst_ip or services", {"src_ip": None}, {}),
            ("null services", "null src_ip, dst_ip or services", {"services": None}, {})]


def einval(call, e, c, out, flows_ptrs):
    """call(spec or None, soa or None, n, packed, result or None) -> code, for every bad call"""
    n = len(c.flows[0])
    for what, words, spec_kw, call_kw in bad_calls(c, out, flows_ptrs):
        keep = []
        spec = spec_of(c, 0, keep)
        if spec_kw == "nospec":
            spec = None
        else:
            for k, v in spec_kw.items():
                if k == "services":
                    spec.services = C.POINTER(_capi.pg_service)()
                else:
                    setattr(spec, k, v)
        ptrs = list(flows_ptrs)
        if "field" in call_kw:
            ptrs[call_kw["field"]] = None
        soa = None if "flows" in call_kw else _capi.pg_tuple_soa(*ptrs)
        res = _capi.pg_reach_observed_result(7, 7, 7, 7, 7)
        code = call(spec, soa, n, call_kw.get("packed", out), res if call_kw.get("result", True) else None)
        assert code == _capi.PG_EINVAL and words in lib.pg_last_error(e.h).decode(), (what, code, lib.pg_last_error(e.h))
        assert res.n_matched == 7 and res.n_cells == 7, what


def empties(run, e):
    """n == 0 clears; an empty side: result zeroed, every flow NO_SRC or NO_DST, the counts cleared"""
    c = random_case(65, 33, 3, 1000, seed=1)
    w = check(run, prefix(c, 0), "no flow", variants=True)
    assert w.result == dict.fromkeys(w.result, 0) and not w.packed.any() and not w.svc_flows.any()
    for src, dst in ((c.src[:0], c.dst), (c.src, c.dst[:0]), (c.src[:0], c.dst[:0])):
        ce = c._replace(src=src, dst=dst)
        w = check(run, ce, "empty side", variants=True)
        assert w.result == dict.fromkeys(w.result, 0) and w.packed.size == 0 and not w.svc_flows.any()
        assert set(np.unique(w.flow)) <= {NO_SRC, NO_DST} and (len(src) == 0) == (w.flow == NO_SRC).all()


def many_services(run, e):
    """4096 services, some sharing a key: the service table alone passes the LDS budget of the address tables
    (asserted from the plan); every service is given three matched flows"""
    g = np.random.default_rng(8)
    nv = 4096
    svc = [((TCP, UDP)[k & 1], 7, k // 3) for k in range(nv - 3)] + [(OTHER, 0, 0), (ANY, 0, 0), (200, 1, 1)]
    p = e.debug_reach_observed_plan(2, 17, nv)
    assert (p["src_in_lds"], p["dst_in_lds"]) == (0, 0) and p["svc_bytes"] == p["lds_bytes"] > (64 << 10), p
    src, dst = addresses(g, 2, 0), addresses(g, 17, 0)
    v = np.resize(np.arange(nv), 3 * nv)
    n = len(v)
    flows = (src[g.integers(0, 2, n)], dst[g.integers(0, 17, n)], np.zeros(n, np.uint16),
             np.array([s[2] for s in svc], np.uint16)[v], np.array([s[0] for s in svc], np.uint8)[v])
    c = case(src, dst, svc, flows)
    w = check(run, c, "4096 services")
    assert w.result["n_matched"] == n and (w.svc_flows >= 3).all() and w.svc_flows.max() >= 6
