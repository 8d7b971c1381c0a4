"""The reachability zones on the host (no GPU): pg_debug_reach_zones_host running the per-word code and
the plan of pg_reach_zones (zones.hpp, the functions the kernels and the launch call) against numpy on
the synthetic closures of tests/zones_cases.py -- every family at the small sizes and around every tile
edge the plan reports -- with garbage in the padding, and against a Python SCC of the oracle's one-hop
graph for real engines: the fixture change of tests/diff_cases.py and the chain policy of
tests/closure_cases.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import closure_cases as cc
import diff_cases as dc
import zones_cases as zc
from vpp_amd import _capi
from vpp_amd import renderer as R
from vpp_amd._capi import lib

SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


def run(*args, **kw):
    return zc.run_host(engine(), *args, **kw)


def test_plan():
    """the tiles cover the matrix, the work items the rows, and no grid is empty"""
    e = engine()
    for n in (1, 16, 17, 127, 128, 129, 1023, 1024, 1025, 4096, 4100, (1 << 13) + 1, 1 << 15):
        p = e.debug_reach_zones_plan(n)
        assert p["tile_rows"] >= 1 and p["tile_cols"] >= 32 and p["tile_cols"] % 32 == 0 and p["label_rows"] >= 1, (n, p)
        assert p["row_tiles"] * p["tile_rows"] >= n > (p["row_tiles"] - 1) * p["tile_rows"], (n, p)
        # (the columns of the working form: rows padded to a multiple of 4 bit-words)
        assert p["col_tiles"] * p["tile_cols"] >= 128 * ((n + 127) // 128) > (p["col_tiles"] - 1) * p["tile_cols"], (n, p)
        assert p["bits_grid"] == p["row_tiles"] * p["col_tiles"] >= 1
        assert p["label_grid"] * p["label_rows"] >= n > (p["label_grid"] - 1) * p["label_rows"] and p["dag_grid"] == n
    plan = _capi.pg_reach_zones_plan()
    assert lib.pg_debug_reach_zones_plan(e.h, (1 << 15) + 1, C.byref(plan)) == _capi.PG_EINVAL
    assert lib.pg_debug_reach_zones_plan(e.h, 4, None) == _capi.PG_EINVAL


@pytest.mark.parametrize("family", zc.FAMILIES)
def test_synthetic(family):
    for n in SIZES:
        if family == "closure" and n > zc.CLOSURE_MAX_N:
            continue
        zc.check(run, zc.synthetic(n, family), variants=n in (17, 65, 129))


@pytest.mark.parametrize("family", ("rings", "corner", "raw", "chain"))
def test_tile_edges(family):
    """one below, on and one above every tile edge the plan reports: the transpose tile's rows and columns,
    and the label work item's rows"""
    p = engine().debug_reach_zones_plan(1 << 15)
    edges = {p["tile_rows"], 2 * p["tile_rows"], p["tile_cols"], p["label_rows"], 2 * p["label_rows"], 64 * 32}
    for n in sorted({max(1, k + d) for k in edges for d in (-1, 0, 1)}):
        zc.check(run, zc.synthetic(n, family, seed=1), variants=False)


@pytest.mark.parametrize("family", ("rings", "corner", "raw", "dup", "full"))
def test_garbage_in_padding(family):
    """random bits in the padding of every row's last word change nothing"""
    for n in (1, 15, 17, 33, 100, 257):
        s = zc.synthetic(n, family, seed=2)
        junk = dc.garbage(s.words, n)
        assert (junk[:, -1] >> (2 * (n & 15))).any(), "no garbage in the padding"
        zc.identical(zc.check(run, s, words=junk, variants=False), run(s.words, n), (family, n))


def test_definitions_by_hand():
    """0 <-> 2 a zone, 1 -> 1 a cyclic singleton, 3 acyclic and reached by all; a code that is not ALLOW is no"""
    A, codes = zc.ALLOW, np.zeros((4, 4), np.uint8)
    codes[0, 2] = codes[2, 0] = codes[0, 0] = codes[2, 2] = codes[1, 1] = A
    codes[0, 3] = codes[2, 3] = codes[1, 3] = A
    codes[3, 0], codes[3, 1], codes[1, 0] = 1, 3, 3
    got = run(zc.pack(codes), 4)
    assert got.zone.tolist() == [0, 1, 0, 2] and got.rep.tolist() == [0, 1, 3] and got.size.tolist() == [2, 1, 1]
    assert got.reaches.tolist() == [3, 2, 0] and got.reached_by.tolist() == [2, 1, 3]
    assert got.dag.tolist() == [[A | A << 4], [A << 2 | A << 4], [0]]
    assert got.result == {"n_zones": 3, "n_cyclic": 2, "n_multi": 1, "largest": 2, "n_broken": 0}
    zc.same(got, zc.expected(codes), "by hand")
    # not transitive: 0 <-> 1 and 1 <-> 2 but not 0 <-> 2 with 1's label 0, 2's label 1: 2 is broken
    codes = np.zeros((3, 3), np.uint8)
    codes[0, 1] = codes[1, 0] = codes[1, 2] = codes[2, 1] = A
    got = run(zc.pack(codes), 3)
    assert got.zone.tolist() == [0, 0, 1] and got.rep.tolist() == [0, 1] and got.result["n_broken"] == 1
    zc.same(got, zc.expected(codes), "broken")


def test_duplicates_share_a_zone_only_on_a_cycle():
    s = zc.synthetic(65, "dup", seed=3)
    w = s.want
    rows, allow = {}, s.codes == zc.ALLOW
    for i in range(s.n):
        rows.setdefault(allow[i].tobytes() + allow[:, i].tobytes(), []).append(i)
    twins = [v for v in rows.values() if len(v) > 1]
    assert any(s.codes[v[0], v[0]] == zc.ALLOW for v in twins) and any(s.codes[v[0], v[0]] != zc.ALLOW for v in twins)
    got = zc.check(run, s)
    for v in twins:
        assert (len(set(got.zone[v].tolist())) == 1) == (s.codes[v[0], v[0]] == zc.ALLOW)


# ---- real engines ------------------------------------------------------------------------------
def test_fixture_change():
    """both engines of the fixture change over c.dst x c.dst: matrix twin -> closure twin -> zones twin
    against a Python SCC of the oracle's one-hop graph"""
    c = cc.fixture_change()
    n = len(c.dst)
    for e, codes in zip((c.e0, c.e1), c.closure_codes):
        comp, want = zc.graph_want(codes)
        assert 1 < want.result["n_zones"] < n and want.result["n_multi"] >= 1
        m = e.debug_reach_matrix_host(c.dst, c.dst, dc.SERVICES, words=False)
        packed, _, counts, _ = e.debug_reach_closure_host(m, n, hops=False)
        got = zc.run_host(e, packed, n)
        zc.same(got, want, "fixture")
        assert (got.rep[got.zone] == comp).all() and (got.reaches == counts[got.rep]).all()


@pytest.mark.parametrize("extra", ((), ((11, 0),), ((3, 1), (9, 7))), ids=("path", "ring", "two-rings"))
def test_chain_policy(extra):
    """the chain policy: a path (12 acyclic zones), a ring (one zone), and two short rings on the path"""
    c = cc.chain(extra)
    comp, want = zc.graph_want(c.codes)
    assert want.result["n_zones"] == {(): 12, ((11, 0),): 1, ((3, 1), (9, 7)): 8}[extra]
    m = c.e.debug_reach_matrix_host(cc.CHAIN_IPS, cc.CHAIN_IPS, cc.CHAIN_SERVICES, words=False)
    packed = c.e.debug_reach_closure_host(m, cc.CHAIN_N, hops=False, counts=False)[0]
    zc.same(zc.run_host(c.e, packed, cc.CHAIN_N), want, extra)
    zones, out, by, graph = c.e.reachability_zones(cc.CHAIN_PODS, cc.CHAIN_SERVICES, host=True)
    wz, wo, wb, wg = zc.wrapper_want(c.codes, cc.CHAIN_PODS)
    assert zones == wz and (out == wo).all() and (by == wb).all() and graph.dtype == bool and (graph == wg).all()


def test_wrapper_host():
    """Engine.reachability_zones(host=True) on the fixture engines, one pod listed twice, against the oracle"""
    c = dc.matrix_change()
    ip = dict(zip(dc.PODS, c.pod_ips))
    ips = np.array([ip[p] for p in zc.PODS], np.uint32)
    seen = []
    for svc in (dc.SERVICES, dc.SERVICES[:1]):
        for e, w in zip((c.e0, c.e1), (c.w0, c.w1)):
            want = zc.wrapper_want(cc.oracle_codes(w, ips, svc), zc.PODS)
            zones, out, by, graph = e.reachability_zones(zc.PODS, svc, host=True)
            assert zones == want[0] and (out == want[1]).all() and (by == want[2]).all() and (graph == want[3]).all()
            assert sum(map(len, zones)) == len(zc.PODS) and zones[0][0] == zc.PODS[0]
            seen.append(zones)
    assert seen[2] != seen[3], "the edit moved no zone under service 0"
    zones, out, by, graph = c.e0.reachability_zones(zc.PODS, [], host=True)
    assert zones == [[p] for p in zc.PODS] and not out.any() and not by.any() and graph.shape == (7, 7) and not graph.any()
    assert c.e0.reachability_zones([], dc.SERVICES, host=True)[0] == []


def test_wrapper_diff_host():
    """Engine.reachability_zones_diff(host=True): the baseline's zones as groups over both closures"""
    from vpp_amd.device import unpack_closure
    c = dc.matrix_change()
    ip = dict(zip(dc.PODS, c.pod_ips))
    ips = np.array([ip[p] for p in zc.PODS], np.uint32)
    svc = dc.SERVICES[:1]   # (under all services the two closures are equal)
    hops = [(cc.oracle_codes(w, ips, svc) == zc.ALLOW).any(axis=0) for w in (c.w0, c.w1)]
    rb, ra = zc.close(hops[0]), zc.close(hops[1])
    zone = zc.expected(np.where(rb, np.uint8(2), np.uint8(0))).zone
    nz = int(zone.max()) + 1
    members = [[p for p, z in zip(zc.PODS, zone) if z == k] for k in range(nz)]
    status = lambda r, a, b: (lambda cells: 2 if cells.all() else 1 if cells.any() else 0)(r[zone == a][:, zone == b])
    want = [(members[a], members[b], status(rb, a, b), status(ra, a, b)) for a in range(nz) for b in range(nz)
            if status(rb, a, b) != status(ra, a, b)]
    assert len(want) >= 2 and any(b == 0 for _, _, b, _ in want) and any(b == 2 for _, _, b, _ in want)
    assert c.e1.reachability_zones_diff(c.e0, zc.PODS, svc, host=True) == want
    assert c.e0.reachability_zones_diff(c.e0, zc.PODS, svc, host=True) == []
    assert c.e1.reachability_zones_diff(c.e0, zc.PODS, dc.SERVICES, host=True) == []


# ---- arguments ---------------------------------------------------------------------------------
def test_einval():
    e = engine()
    w, out = np.zeros(64, np.uint32), np.full(64, zc.FILL, np.uint32)
    res = _capi.pg_reach_zones_result(7, 7, 7, 7, 7)
    for what, words, spec, outs, with_result in zc.bad_calls(w.ctypes.data, out.ctypes.data):
        code = lib.pg_debug_reach_zones_host(e.h, C.byref(spec) if spec is not None else None, *outs,
                                             C.byref(res) if with_result else None)
        assert code == _capi.PG_EINVAL, (what, code)
        assert words in lib.pg_last_error(e.h).decode(), (what, lib.pg_last_error(e.h))
    assert (out == zc.FILL).all() and (res.n_zones, res.n_cyclic, res.n_multi, res.largest, res.n_broken) == (7, 7, 7, 7, 7)
    assert lib.pg_debug_reach_zones_host(None, None, None, None, None, None, None, None, None) == _capi.PG_EINVAL


def test_empty_input():
    """n == 0: PG_OK, the result zeroed, nothing else written; the matrix may be null"""
    bufs = zc.buffers(5)
    res = _capi.pg_reach_zones_result(7, 7, 7, 7, 7)
    code = lib.pg_debug_reach_zones_host(engine().h, C.byref(zc.spec_of(None, 0)), *[b.ctypes.data_as(C.c_void_p) for b in bufs],
                                         C.byref(res))
    assert code == 0 and (res.n_zones, res.n_cyclic, res.n_multi, res.largest, res.n_broken) == (0, 0, 0, 0, 0)
    assert all((b == zc.FILL).all() for b in bufs)
