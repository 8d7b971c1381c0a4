"""The reachability paths on the host: pg_debug_reach_paths_host (the per-word code, the partition and the
plan of paths.hpp, which the kernels and the launch share) against numpy over the graphs of
tests/closure_cases.py, the query orders and chunk boundaries, max_len, the optional outputs, the
2048-column pass boundary, a deep ring, a bounded closure and a broken matrix; the argument checks;
and real engines against the oracle's edges.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import closure_cases as cc
import diff_cases as dc
import paths_cases as pc
from vpp_amd import _capi
from vpp_amd import renderer as R
from vpp_amd._capi import lib


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


def run(*args, **kw):
    return pc.run_host(engine(), *args, **kw)


def chunk(n):
    return engine().debug_reach_paths_plan(n)["chunk_queries"]


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_synthetic(family):
    for n in cc.SIZES:
        pc.check(run, cc.synthetic(n, family), chunk(n), variants=n in (17, 100, 257))


def test_plan():
    e = engine()
    for n in (1, 17, 2048, 4096, 1 << 15):
        p = e.debug_reach_paths_plan(n)
        assert p["chunk_queries"] >= 1 and p["lds_bytes"] % 16 == 0 and 2 * n + 16 <= p["lds_bytes"] <= 160 * 1024, (n, p)


@pytest.mark.parametrize("n", (2047, 2048, 2049))
@pytest.mark.parametrize("family", ("star", "two-cliques", "hub-last"))
def test_pass_boundary(family, n):
    """around 2048 columns, one pass of a wave: random pairs, and the pairs whose least predecessor lies in
    the last bit-word. The star and the two cliques have none (their least predecessors are node 0 and the
    bridge), so the star with its hub at the other end stands beside them: at 2049 nodes its hub is the
    one column of the second pass."""
    h, edges = pc.boundary_graph(family, n)
    src, dst, n_last = pc.boundary_queries(h)
    assert (n_last > 2000) == (family == "hub-last"), n_last
    x = pc.Expected(h)
    got = run(h, n, src, dst, 4)
    pc.same(got, x, src, dst, 4, (family, n))
    pc.valid(got, edges, h, src, dst, 4, (family, n))


# ---- past 4096 end points --------------------------------------------------------------------------
def test_reference_routes(monkeypatch):
    """Expected's routes for a large graph give what the n^2 masks give: the level-wise predecessor vector,
    and a step answered from a few srcs' vectors"""
    for n, family in ((257, "medium"), (200, "sparse"), (64, "two-cliques")):
        h = cc.synthetic(n, family).expected().hops
        want = pc.Expected(h).tree()
        monkeypatch.setattr(pc, "TREE_MAX_N", 0)
        x = pc.Expected(h)
        assert (np.stack([x.pred(i) for i in range(n)]) == want).all(), (n, family)
        src, dst, perm = pc.few_sources(n)
        few = x.outputs(src[perm], dst[perm], n)
        monkeypatch.setattr(pc, "FEW_SRCS", 0)
        many = pc.Expected(h).outputs(src[perm], dst[perm], n)
        monkeypatch.undo()
        tree = pc.Expected(h).outputs(src[perm], dst[perm], n)
        for a, b, c in zip(few, many, tree):
            assert (a == b).all() and (a == c).all() if isinstance(a, np.ndarray) else a == b == c, (n, family)


def test_thresholds():
    """the sizes of the large path tests, found from the plan: the last workgroup within 48 KiB that counts
    out_via in LDS, the last that counts it in LDS at all, the last row that fits 48 KiB alone"""
    e = engine()
    t = pc.thresholds(e)
    assert t == pc.THRESHOLDS
    lds = lambda n: e.debug_reach_paths_plan(n)["lds_bytes"]
    assert lds(t["via_48k"]) <= pc.KIB48 < lds(t["via_48k"] + 1) and lds(t["via_lds"]) > pc.KIB48 > lds(t["via_lds"] + 1)
    assert lds(t["row_48k"]) <= pc.KIB48 < lds(t["row_48k"] + 1) and lds(1 << 15) > 64 * 1024


def test_few_sources():
    for n in (257, 8193, 8156):
        src, dst, perm = pc.few_sources(n)
        srcs = np.unique(src)
        last = 32 * ((n - 1) // 32)
        assert len(srcs) == 8 and srcs[0] == 0 and srcs[-1] == n - 1 and (srcs >= last).sum() >= min(2, n - last)
        assert len(src) == 8 * n and (np.sort(perm) == np.arange(8 * n)).all() and (dst.reshape(8, n) == np.arange(n)).all()


@pytest.mark.parametrize("family", ("two-cliques", "hub-last"))
def test_analytic_queries(family):
    """the paths written down in paths_cases.analytic_queries are Expected's, and the host twin's"""
    for n in (300, 2100):
        h, edges = pc.boundary_graph(family, n)
        queries = pc.analytic_queries(family, n)
        src, dst = np.array([(s, d) for s, d, _ in queries], np.uint32).T
        assert len(queries) <= 64 and max(len(p) for _, _, p in queries if p) == (4 if family == "two-cliques" else 3)
        got = run(h, n, src, dst, 3)
        pc.check_analytic(got, n, queries, 3)
        pc.same(got, pc.Expected(h), src, dst, 3, (family, n))
        pc.valid(got, edges, h, src, dst, 3, (family, n))


def test_medium_at_via_threshold():
    """a random graph of 4 edges per node at the last size whose workgroup counts out_via within 48 KiB of
    LDS: eight srcs against every dst over the CPU reference's closure, paths of up to levels edges"""
    n = pc.THRESHOLDS["via_48k"]
    g = cc.LargeMedium(n, seed=cc.LARGE_SEED, words=False)
    edges = g.edge_matrix()
    cx = cc.Expected(np.where(edges, np.uint8(cc.ALLOW), np.uint8(0))[None])
    r = cx.at(0)[3]
    assert (r["n_edges"], r["n_reachable"], r["levels"]) == cc.LARGE_WANT[n, "medium", cc.LARGE_SEED]
    pc.check_few_sources(run, cx.hops, edges, cx.levels)


def test_ring_depth():
    """the analytic ring at n = 2049: 2048 and 2049 edges, and all three too long for max_len 64"""
    pc.check_ring(run)


def test_bounded_closure():
    """hops taken with max_hops = 2: paths exist exactly where they have at most 2 edges"""
    for n, family in ((100, "medium"), (65, "sparse"), (33, "ring")):
        cx = cc.synthetic(n, family).expected()
        full, h = cx.hops, cx.at(2)[1]
        src, dst = pc.all_pairs(n)
        got = run(h, n, src, dst, n)
        pc.same(got, pc.Expected(h), src, dst, n, (family, n))
        pc.valid(got, cx.edges, h, src, dst, n, (family, n))
        assert ((got[0].reshape(n, n) > 0) == ((full > 0) & (full <= 2))).all()
        # the paths of the bounded matrix are those of the full one
        want = pc.Expected(full).outputs(src, dst, n)[1]
        assert (got[1][got[0] > 0] == want[got[0] > 0]).all()


def test_broken_matrix():
    pc.check_broken(run)


def call(e, spec, out_len, out_nodes, out_via, with_result):
    res = _capi.pg_reach_paths_result(7, 7, 7, 7, 7, 7)
    code = lib.pg_debug_reach_paths_host(e.h, C.byref(spec) if spec is not None else None, out_len, out_nodes, out_via,
                                         C.byref(res) if with_result else None)
    return code, res


def test_einval():
    e = engine()
    h, lens, rows = np.ones((4, 4), np.uint16), np.zeros(4, np.uint16), np.zeros((4, 5), np.uint16)

    def one(spec, out_len, out_nodes, out_via, with_result):
        code, _ = call(e, spec, out_len, out_nodes, out_via, with_result)
        return code, lib.pg_last_error(e.h).decode()

    pc.einval(one, h.ctypes.data, lens.ctypes.data, rows.ctypes.data)
    assert lib.pg_debug_reach_paths_plan(e.h, 4, None, None) == _capi.PG_EINVAL
    # max_len is read with out_nodes only
    s = d = np.zeros(4, np.uint32)
    code, res = call(e, _capi.pg_reach_paths_spec(h.ctypes.data, 4, s.ctypes.data, d.ctypes.data, 4, 0), lens.ctypes.data,
                     None, None, True)
    assert code == 0 and res.n_found == 4 and res.n_too_long == 0


def test_empty_cases():
    """n_queries == 0: PG_OK, the result zeroed, out_via cleared when given, nothing else written; with n ==
    0 as well nothing is written"""
    e = engine()
    h = np.ones((4, 4), np.uint16)
    lens, rows, via = np.full(4, pc.LEN_FILL, np.uint16), np.full(8, pc.NODES_FILL, np.uint16), np.full(4 + pc.GUARD, 9, np.uint32)
    p = lambda x: x.ctypes.data
    code, res = call(e, _capi.pg_reach_paths_spec(p(h), 4, None, None, 0, 4), p(lens), p(rows), p(via), True)
    assert code == 0 and pc.result_dict(res) == dict.fromkeys(pc.result_dict(res), 0)
    assert (lens == pc.LEN_FILL).all() and (rows == pc.NODES_FILL).all() and (via[:4] == 0).all() and (via[4:] == 9).all()
    via[:] = 9
    code, res = call(e, _capi.pg_reach_paths_spec(p(h), 0, None, None, 0, 4), p(lens), p(rows), p(via), True)
    assert code == 0 and pc.result_dict(res) == dict.fromkeys(pc.result_dict(res), 0)
    assert (lens == pc.LEN_FILL).all() and (rows == pc.NODES_FILL).all() and (via == 9).all()
    # a query needs an end point
    s = np.zeros(1, np.uint32)
    code, _ = call(e, _capi.pg_reach_paths_spec(p(h), 0, p(s), p(s), 1, 4), p(lens), None, None, True)
    assert code == _capi.PG_EINVAL


# ---- real engines against World.conn (the oracle) ------------------------------------------------
def engine_hops(c, select=None):
    """the host twins' hops of a chain engine, and the oracle's edges"""
    m = c.e.debug_reach_matrix_host(cc.CHAIN_IPS, cc.CHAIN_IPS, cc.CHAIN_SERVICES, words=False)
    h = cc.run_host(c.e, m, cc.CHAIN_N, select, 0)[1]
    x = c.expected(select)
    assert (h == x.hops).all()
    return h, x.edges


def test_plain_chain():
    """c0 -> c11 is c0, c1, .., c11; over the 66 reachable pairs via[k] == k (11 - k), 220 in all"""
    c = cc.chain()
    h, edges = engine_hops(c)
    n = cc.CHAIN_N
    lens, rows, via, res = run(h, n, [0], [11], n)
    assert lens[0] == 11 and rows[0, :12].tolist() == list(range(12)) and (rows[0, 12:] == pc.NONE).all()
    src, dst = pc.all_pairs(n)
    got = run(h, n, src, dst, n)
    pc.valid(got, edges, h, src, dst, n, "chain")
    assert got[3]["n_found"] == 66 and got[3]["n_unreachable"] == 144 - 66 and got[3]["longest"] == 11
    k = np.arange(n)
    assert (got[2] == k * (11 - k)).all() and got[3]["n_via"] == 220


def test_chain_ring():
    """with the edge c11 -> c0: c5 -> c4 has 11 edges round the ring, c3 -> c3 is the 12-edge cycle"""
    c = cc.chain(((11, 0),))
    h, edges = engine_hops(c)
    n = cc.CHAIN_N
    src, dst = [5, 3], [4, 3]
    got = run(h, n, src, dst, n)
    pc.valid(got, edges, h, src, dst, n, "ring")
    assert got[0].tolist() == [11, 12]
    assert got[1][0, :12].tolist() == [(5 + k) % 12 for k in range(12)]
    assert got[1][1].tolist() == [(3 + k) % 12 for k in range(13)]
    src, dst = pc.all_pairs(n)
    got = run(h, n, src, dst, n)
    pc.valid(got, edges, h, src, dst, n, "ring, all pairs")
    pc.same(got, pc.Expected(h), src, dst, n, "ring, all pairs")


def fixture_hops():
    """the fixture change under service 0: (hops before, hops after) from the host twins, checked against the
    oracle's closures"""
    c = cc.fixture_change()
    out = []
    for e, codes in zip((c.e0, c.e1), c.closure_codes):
        m = e.debug_reach_matrix_host(c.dst, c.dst, dc.SERVICES, words=False)
        h = cc.run_host(e, m, len(c.dst), (0,), 0)[1]
        assert (h == cc.Expected(codes, (0,)).hops).all()
        out.append(h)
    return out


def test_fixture_change():
    """every one of the 984 opened closure cells has, under the after engine, a path with at least one edge
    that is present after and absent before (or the cell was reachable before); the 138 closed cells have
    no path after"""
    c, w = cc.fixture_change(), cc.FIXTURE_WANT
    n = len(c.dst)
    hb, ha = fixture_hops()
    eb, ea = (cc.Expected(codes, (0,)).edges for codes in c.closure_codes)
    opened, closed = np.argwhere((hb == 0) & (ha > 0)), np.argwhere((hb > 0) & (ha == 0))
    assert len(opened) == w["closure_opened"] and len(closed) == w["closure_closed"]
    src, dst = np.concatenate([opened[:, 0], closed[:, 0]]), np.concatenate([opened[:, 1], closed[:, 1]])
    got = pc.run_host(c.e1, ha, n, src, dst, n)
    pc.valid(got, ea, ha, src, dst, n, "fixture")
    lens, rows, via, res = got
    assert (lens[:len(opened)] > 0).all() and (lens[len(opened):] == 0).all()
    assert res["n_found"] == len(opened) and res["n_unreachable"] == len(closed)
    fresh = ea & ~eb
    for d, r in zip(lens[:len(opened)], rows[:len(opened)].astype(np.int64)):
        assert fresh[r[:d], r[1:d + 1]].any(), r[:d + 1]


@pytest.mark.parametrize("name", ("small", "grouped", "uncovered", "pair"))
def test_topology(name):
    """the node_matrix topologies: the validity checks on all 64 x 64 pairs against the oracle's edges"""
    e, ips, svc, codes = cc.topology(name)
    cx = cc.Expected(codes)
    m = e.debug_reach_matrix_host(ips, ips, svc, words=False)
    h = cc.run_host(e, m, 64, None, 0)[1]
    assert (h == cx.hops).all()
    src, dst = pc.all_pairs(64)
    got = pc.run_host(e, h, 64, src, dst, 64)
    pc.valid(got, cx.edges, h, src, dst, 64, name)
    pc.same(got, pc.Expected(h), src, dst, 64, name)


# ---- the wrappers --------------------------------------------------------------------------------
def names(path):
    return [cc.CHAIN_PODS[k] for k in path]


def test_reachability_paths_host():
    c = cc.chain(((11, 0), (3, 9)))
    P = cc.CHAIN_PODS
    pairs = [(P[0], P[11]), (P[5], P[4]), (P[3], P[3]), (P[9], P[2])]
    got = c.e.reachability_paths(P, cc.CHAIN_SERVICES, pairs, host=True)
    x = pc.Expected(c.expected(None).hops)
    d, paths, _ = x.walk([0, 5, 3, 9], [11, 4, 3, 2])
    assert got == [names(p[:k + 1]) for p, k in zip(paths.tolist(), d.tolist())]
    assert got[0] == names([0, 1, 2, 3, 9, 10, 11])   # (through the chord c3 -> c9)
    # the answer comes in the names given, whatever the order of the pods
    assert c.e.reachability_paths(P[::-1], cc.CHAIN_SERVICES, pairs[:1], host=True) == [got[0]]
    plain = cc.chain()
    got = plain.e.reachability_paths(P, cc.CHAIN_SERVICES, [(P[0], P[11]), (P[11], P[0]), (P[2], P[4])], host=True)
    assert got == [names(range(12)), None, names([2, 3, 4])]
    assert plain.e.reachability_paths(P, cc.CHAIN_SERVICES, [(P[0], P[11]), (P[0], P[3])], max_hops=3, host=True) == \
        [None, names([0, 1, 2, 3])]
    assert plain.e.reachability_paths(P, cc.CHAIN_SERVICES, [], host=True) == []


def test_reachability_chokepoints_host():
    plain = cc.chain()
    P = cc.CHAIN_PODS
    got = plain.e.reachability_chokepoints(P, cc.CHAIN_SERVICES, host=True)
    want = sorted(((P[k], k * (11 - k)) for k in range(1, 11)), key=lambda t: -t[1])   # (stable: then by pod order)
    assert got == want and sum(c for _, c in got) == 220
    got = plain.e.reachability_chokepoints(P, cc.CHAIN_SERVICES, sources=[P[0], P[2]], targets=[P[5], P[1]], host=True)
    assert got == [(P[3], 2), (P[4], 2), (P[1], 1), (P[2], 1)]


def test_reachability_closure_diff_paths_host():
    """every opened entry carries its path under the after engine"""
    before, after = cc.chain(), cc.chain(((11, 0),))
    P = cc.CHAIN_PODS
    plain = after.e.reachability_closure_diff(before.e, P, cc.CHAIN_SERVICES, host=True)
    got = after.e.reachability_closure_diff(before.e, P, cc.CHAIN_SERVICES, host=True, paths=True)
    assert len(got) == 144 - 66 and [t[:4] for t in got] == plain
    x = pc.Expected(after.expected(None).hops)
    for a, b, _, _, path in got:
        i, j = P.index(a), P.index(b)
        d, want, _ = x.walk([i], [j])
        assert path == names(want[0, :d[0] + 1].tolist()) and path[0] == a and path[-1] == b and (11, 0) in \
            [(P.index(u), P.index(v)) for u, v in zip(path, path[1:])]
    # a closed entry has no path after
    back = before.e.reachability_closure_diff(after.e, P, cc.CHAIN_SERVICES, dc.CLOSED, host=True, paths=True)
    assert len(back) == 144 - 66 and all(t[4] is None for t in back)
