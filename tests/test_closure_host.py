"""The reachability closure on the host (no GPU): pg_debug_reach_closure_host running the per-word code
of pg_reach_closure (closure.hpp, the functions the kernels call) against numpy on the synthetic graphs
of tests/closure_cases.py, and against numpy on the oracle's words for real engines: the fixture change
of tests/diff_cases.py, the chain policy and four node_matrix topologies.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import closure_cases as cc
import diff_cases as dc
from vpp_amd import _capi
from vpp_amd import device as D
from vpp_amd import renderer as R
from vpp_amd._capi import lib


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


def run(*args, **kw):
    return cc.run_host(engine(), *args, **kw)


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_synthetic(family):
    for n in cc.SIZES:
        s = cc.synthetic(n, family)
        if n & 15:
            assert (s.words[:, :, -1] >> (2 * (n & 15))).any(), "no garbage in the padding"
        cc.check(run, s.words, n, s.expected, s.n_svc)


def test_deep_families():
    """chain at 257 is 256 levels, ring 257; a full graph is one level"""
    assert cc.synthetic(257, "chain").expected().levels == 256
    x = cc.synthetic(257, "ring").expected()
    assert x.levels == 257 and (np.diag(x.hops) == 257).all() and x.at(0)[3]["n_reachable"] == 257 * 257
    assert cc.synthetic(257, "full").expected().levels == 1 and cc.synthetic(257, "empty").expected().levels == 0
    assert cc.synthetic(64, "two-cliques").expected().levels == 3


def test_per_word_code():
    """compaction and expansion are inverse; one slice's words alone give that slice's ALLOW cells"""
    s = cc.synthetic(100, "dense", n_svc=1)
    packed, hops, counts, res = run(s.words, 100, None, 1)
    assert (D.unpack_closure(packed, 100) == (s.codes[0] == cc.ALLOW)).all() and res["levels"] == 1
    assert res["n_edges"] == res["n_reachable"] == int((s.codes[0] == cc.ALLOW).sum())
    assert ((hops == 1) == (s.codes[0] == cc.ALLOW)).all() and (counts == (s.codes[0] == cc.ALLOW).sum(axis=1)).all()


# ---- past 4096 end points ------------------------------------------------------------------------
def test_island_placement():
    """five disjoint islands inside the graph, one across every cut that lies far enough inside it, the last
    ending at node n - 1"""
    for n in cc.edge_sizes(engine()) + (480, 8300, 1 << 15):
        s = cc.island_starts(n)
        assert len(s) == cc.ISLANDS and s[0] == 0 and s[-1] == n - cc.ISLAND and all(b - a >= cc.ISLAND for a, b in zip(s, s[1:]))
        for cut in (2048, 4096, 8192):
            assert (cut + cc.ISLAND // 2 > n - cc.ISLAND) or any(a < cut < a + cc.ISLAND for a in s), (n, cut, s)
    assert cc.island_starts(8193)[-1] + cc.ISLAND - 1 == 8192   # (the last island then reaches over the cut by itself)


def test_edge_sizes():
    """the sizes of the large closure tests and what the plan does there (closure_cases.EDGE_PLANS)"""
    e = engine()
    sizes = cc.edge_sizes(e)
    assert sizes == (4095, 4096, 4097, 8191, 8192, 8193)
    assert tuple(cc.plan_shape(e, n) for n in sizes) == cc.EDGE_PLANS
    assert [cc.plan_shape(e, n)[0] for n in (2048, 2049)] == [1, 2]
    # the pack kernel's second round: more than 256 input words in a row
    assert [cc.row_words(n) > 256 for n in sizes] == [False, False, True, True, True, True]


@pytest.mark.parametrize("k", range(6))
def test_islands(k):
    """the islands at the six sizes around the lane-width and column-tile cuts: the preconditions on the
    reference alone, the committed numbers, and the host twin against the embedded 240-node closure"""
    n = cc.edge_sizes(engine())[k]
    s = cc.Islands(n, seed=cc.LARGE_SEED)
    x = s.expected()
    cc.check_walk_shape(x)
    star = cc.Expected(np.where(cc.edges(300, "star", None), np.uint8(cc.ALLOW), np.uint8(0))[None])
    assert cc.walk_shape(star)["repeats"] > 0.9   # (what the star cannot see)
    r = x.at(0)[3]
    assert (r["n_edges"], r["n_reachable"], r["levels"]) == cc.LARGE_WANT[n, "islands", cc.LARGE_SEED]
    assert (s.words[:, :, -1] >> (2 * (n & 15))).any() or not n & 15, "no garbage in the padding"
    for sel, hop_bound, hops, counts in cc.large_runs(x.levels):
        cc.same(run(s.words, n, sel, hop_bound, hops=hops, counts=counts), s.expected(sel), hop_bound, (n, sel, hop_bound))


# ---- the fixture change ------------------------------------------------------------------------
def test_fixture_oracle_numbers():
    """the oracle alone: the numbers of the fixture graphs (closure_cases.FIXTURE_WANT)"""
    c, w = cc.fixture_change(), cc.FIXTURE_WANT
    assert len(c.dst) == 53
    for k, codes in enumerate(c.closure_codes):
        x0, xa = cc.Expected(codes, (0,)), cc.Expected(codes)
        r0, ra = x0.at(0)[3], xa.at(0)[3]
        assert (r0["n_edges"], r0["n_reachable"]) == w["svc0"][k] and (ra["n_edges"], ra["n_reachable"]) == w["all"][k]
        assert ra["levels"] == 2 and int((xa.hops == 2).sum()) == w["hop2_all"]
    x = cc.Expected(c.closure_codes[0], (0,))
    assert x.levels == 2 and int((x.hops == 2).sum()) == w["hop2_svc0_before"]


def fixture_closures(select):
    """the host closures (before, after) of the fixture change over c.dst x c.dst, checked against numpy"""
    c = cc.fixture_change()
    out = []
    for e, codes in zip((c.e0, c.e1), c.closure_codes):
        m = e.debug_reach_matrix_host(c.dst, c.dst, dc.SERVICES, words=False)
        assert (m == np.stack([dc.pack(v) for v in codes])).all()
        expected = functools.lru_cache(maxsize=None)(lambda sel, codes=codes: cc.Expected(codes, sel))
        cc.check(run, m, len(c.dst), expected, len(dc.SERVICES), variants=select is None)
        out.append(run(m, len(c.dst), select, 0)[0])
    return out


def test_fixture_closure_and_diff():
    """under service 0 the edit opens 984 and closes 138 cells of the closure (444 / 102 one-hop)"""
    c, w = cc.fixture_change(), cc.FIXTURE_WANT
    n = len(c.dst)
    b, a = fixture_closures((0,))
    xb, xa = (cc.Expected(codes, (0,)) for codes in c.closure_codes)
    rb, ra = xb.hops > 0, xa.hops > 0
    assert int((~rb & ra).sum()) == w["closure_opened"] and int((rb & ~ra).sum()) == w["closure_closed"]
    assert int((~xb.edges & xa.edges).sum()) == w["one_hop_opened"] and int((xb.edges & ~xa.edges).sum()) == w["one_hop_closed"]
    e = engine()
    for t, mask in ((dc.OPENED, ~rb & ra), (dc.CLOSED, rb & ~ra)):
        k, changes, _, _ = e.debug_reach_diff_host(b, a, n, t, row_changes=False)
        row, col, _, _ = D.unpack_changes(changes[:k])
        assert k == int(mask.sum()) and (np.stack([row, col], axis=1) == np.argwhere(mask)).all()
    # the one-hop graphs (max_hops = 1) through the same diff
    b1, a1 = (run(m.debug_reach_matrix_host(c.dst, c.dst, dc.SERVICES, words=False), n, (0,), 1)[0] for m in (c.e0, c.e1))
    assert e.debug_reach_diff_host(b1, a1, n, dc.OPENED, cap=0)[0] == w["one_hop_opened"]
    assert e.debug_reach_diff_host(b1, a1, n, dc.CLOSED, cap=0)[0] == w["one_hop_closed"]


def test_fixture_all_services_equal():
    """with all services selected the two closures are equal and the diff says 0"""
    b, a = fixture_closures(None)
    assert (b == a).all()
    assert engine().debug_reach_diff_host(b, a, b.shape[0], dc.ALL, cap=0)[0] == 0


# ---- the chain policy --------------------------------------------------------------------------
def test_chain_oracle_numbers():
    """the oracle alone (closure_cases.CHAIN_WANT)"""
    for (extra, sel), want in cc.CHAIN_WANT.items():
        x = cc.chain(extra).expected(sel)
        r = x.at(0)[3]
        assert (r["n_edges"], r["n_reachable"], r["levels"]) == want, (extra, sel, r)
    assert not np.diag(cc.chain().expected((0,)).hops).any()
    ring, chord = cc.chain(((11, 0),)).expected((0, 1)), cc.chain(((11, 0), (3, 9))).expected((0, 1))
    assert (np.diag(ring.hops) == 12).all() and (ring.hops != chord.hops).any()


@pytest.mark.parametrize("extra", ((), ((11, 0),), ((11, 0), (3, 9))), ids=("path", "ring", "chord"))
def test_chain(extra):
    c = cc.chain(extra)
    m = c.e.debug_reach_matrix_host(cc.CHAIN_IPS, cc.CHAIN_IPS, cc.CHAIN_SERVICES, words=False)
    assert (m == np.stack([dc.pack(v) for v in c.codes])).all()
    cc.check(run, m, cc.CHAIN_N, c.expected, len(cc.CHAIN_SERVICES))


# ---- node_matrix topologies --------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.TOPOLOGY_WANT))
def test_topology(name):
    e, ips, svc, codes = cc.topology(name)
    x = cc.Expected(codes)
    r = x.at(0)[3]
    assert (r["n_edges"], r["n_reachable"]) == cc.TOPOLOGY_WANT[name] and r["levels"] == 2   # the oracle alone
    assert len(set(ips.tolist())) < len(ips), "no duplicate end point"
    m = e.debug_reach_matrix_host(ips, ips, svc, words=False)
    expected = functools.lru_cache(maxsize=None)(lambda sel: cc.Expected(codes, sel))
    cc.check(run, m, len(ips), expected, len(svc), variants=False)


# ---- arguments ---------------------------------------------------------------------------------
def call(e, spec, packed=None, result=True, hops=None, counts=None):
    res = _capi.pg_reach_closure_result(7, 7, 7)
    p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    code = lib.pg_debug_reach_closure_host(e.h, C.byref(spec) if spec is not None else None, p(packed), p(hops), p(counts),
                                           C.byref(res) if result else None)
    return code, res


def test_einval():
    e = engine()
    w, out = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
    S = _capi.pg_reach_closure_spec
    bad = [(None, out, True), (S(None, 4, 1, None, 0), out, True), (S(w.ctypes.data, 4, 1, None, 0), None, True),
           (S(w.ctypes.data, 4, 1, None, 0), out, False),                 # null result
           (S(w.ctypes.data, (1 << 15) + 1, 1, None, 0), out, True),
           (S(w.ctypes.data, 4, 0, None, 0), out, True), (S(w.ctypes.data, 4, 4097, None, 0), out, True)]
    for spec, packed, with_res in bad:
        code, _ = call(e, spec, packed, with_res)
        assert code == _capi.PG_EINVAL, (spec, code)
        assert lib.pg_last_error(e.h), "pg_last_error is empty"
    assert lib.pg_debug_reach_closure_host(None, None, None, None, None, None) == _capi.PG_EINVAL
    assert call(e, S(w.ctypes.data, 4, 1, None, 0), out)[0] == 0


def test_no_end_points():
    """n == 0: PG_OK, the result zeroed, nothing else written"""
    e = engine()
    w = np.zeros(4, np.uint32)
    packed, counts, hops = np.full(4, cc.FILL, np.uint32), np.full(4, cc.FILL, np.uint32), np.full(4, 0xFFFF, np.uint16)
    code, res = call(e, _capi.pg_reach_closure_spec(w.ctypes.data, 0, 1, None, 0), packed, True, hops, counts)
    assert code == 0 and (res.levels, res.n_edges, res.n_reachable) == (0, 0, 0)
    assert (packed == cc.FILL).all() and (counts == cc.FILL).all() and (hops == 0xFFFF).all()


def test_plan():
    e = engine()
    for n in (1, 16, 17, 2048, 2049, 4096, 4097, 1 << 15):
        p = e.debug_reach_closure_plan(n)
        rows, cols = -(-n // p["tile_rows"]), -(-n // p["tile_cols"])
        assert p["tile_rows"] >= 1 and p["tile_cols"] % 32 == 0 and p["grid"] == rows * cols, (n, p)


# ---- the wrappers ------------------------------------------------------------------------------
def test_reachability_closure_host():
    c = cc.chain(((11, 0), (3, 9)))
    x = c.expected(None)
    pods = cc.CHAIN_PODS[::-1]   # the answer comes in the order the pods are given
    reach, hops, levels = c.e.reachability_closure(pods, cc.CHAIN_SERVICES, host=True)
    assert levels == x.levels == 12 and (reach == (x.hops > 0)[::-1, ::-1]).all() and (hops == x.hops[::-1, ::-1]).all()
    reach, hops, levels = c.e.reachability_closure(cc.CHAIN_PODS, cc.CHAIN_SERVICES, max_hops=3, host=True)
    assert levels == 3 and (hops == x.at(3)[1]).all() and (reach == x.at(3)[0]).all()


def test_reachability_closure_diff_host():
    """adding the edge c11 -> c0 opens 144 - 66 cells of the closure, in the pods' names"""
    before, after = cc.chain(), cc.chain(((11, 0),))
    got = after.e.reachability_closure_diff(before.e, cc.CHAIN_PODS, cc.CHAIN_SERVICES, host=True)
    was = before.expected(None).hops > 0
    want = [(cc.CHAIN_PODS[i], cc.CHAIN_PODS[j], 0, 2) for i, j in np.argwhere(~was)]
    assert len(want) == 144 - 66 and got == want
    assert after.e.reachability_closure_diff(before.e, cc.CHAIN_PODS, cc.CHAIN_SERVICES, dc.CLOSED, host=True) == []
    back = before.e.reachability_closure_diff(after.e, cc.CHAIN_PODS, cc.CHAIN_SERVICES, dc.CLOSED, host=True)
    assert back == [(s, d, 2, 0) for s, d, _, _ in want]
