"""The reachability cost on the host: pg_debug_reach_cost_host (cost.hpp's per-word code) against the
references of tests/cost_cases.py -- the enumeration of simple walks on all graphs of up to 4 end points and
random ones up to 7, and the Dijkstra reference, pinned here to that enumeration and to scipy, on every
family at every size; max_cost against the filtered answer; unit weights against the closure's and the
paths' host twins; the plan over the whole range of n and the knob; the arguments; duplicate sources.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import closure_cases as cc
import cost_cases as co
import paths_cases as pc
from vpp_amd import _capi
from vpp_amd import renderer as R
from vpp_amd._capi import lib


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


def run(*args, **kw):
    return co.run_host(engine(), *args, **kw)


# ---- the references among themselves ---------------------------------------------------------------
def test_reference_against_brute_force_and_scipy():
    """the pin of the references, once: cost_cases.reference against the enumeration and against scipy. Runs no
    product code (it passes without pg_reach_cost); the tests below rest on it"""
    for a, w in co.small_cases():
        n = a.shape[0]
        x, y = co.reference(a, w, range(n)), co.by_scipy(a, w, range(n))
        assert (x.cost == y.cost).all() and (x.pred == y.pred).all()
        cost, pred, ln, via, _ = x.at()
        rows = [co.brute(a, w, s) for s in range(n)]
        for s in range(n):
            assert (cost[s] == rows[s][0]).all() and (pred[s] == rows[s][1]).all() and (ln[s] == rows[s][2]).all(), (a.astype(int).tolist(), w, s)
        assert (via == sum(r[3].astype(np.int64) for r in rows)).all()
    for name in co.FAMILIES:
        for n in (33, 300):
            a, w, src = co.family(n, name)
            x, y = co.reference(a, w, src), co.by_scipy(a, w, src)
            assert (x.cost == y.cost).all() and (x.pred == y.pred).all(), (name, n)


def test_vector_brute_force_against_the_plain_one():
    """brute_all is brute, graph by graph, on a sample of the graphs of 3 and 4 end points. Runs no product code
    either: it pins the vector form that test_all_graphs_up_to_4 holds the host twin to"""
    for n in (1, 2, 3, 4):
        a, w = co.all_graphs(n)
        cost, pred, ln, via = co.brute_all(a, w)
        for b in range(0, len(a), 1 if n < 3 else 7 if n == 3 else 1013):
            rows = [co.brute(a[b], w[b], s) for s in range(n)]
            for s in range(n):
                assert (cost[b, s] == rows[s][0]).all() and (pred[b, s] == rows[s][1]).all() and (ln[b, s] == rows[s][2]).all(), (n, b, s)
            assert (via[b] == sum(r[3].astype(np.int64) for r in rows)).all(), (n, b)


# ---- the host twin against the definition ------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 3, 4))
def test_all_graphs_up_to_4(n):
    """every graph of n end points, 512 at a time as one disjoint union, every end point a source"""
    a, w = co.all_graphs(n)
    cost, pred, ln, via = co.brute_all(a, w)
    for lo in range(0, len(a), 512):
        hi = min(lo + 512, len(a))
        G, m = hi - lo, (hi - lo) * n
        got = run(co.union_words(a[lo:hi]), m, np.arange(m), w[lo:hi].ravel())
        # cell (g * n + s, g * n + v) of the union is cell (s, v) of graph g; nothing leaves a graph
        gi = np.arange(G)[:, None, None]
        at = (gi * n + np.arange(n)[None, :, None], gi * n + np.arange(n)[None, None, :])
        off = (np.arange(G) * n)[:, None, None]
        want_pred = np.where(pred[lo:hi] == co.NO_PRED, co.NO_PRED, pred[lo:hi] + off)
        assert (got[0][at] == cost[lo:hi]).all() and (got[1][at] == want_pred).all() and (got[2][at] == ln[lo:hi]).all(), (n, lo)
        assert int((got[0] != co.NONE).sum()) == int((cost[lo:hi] != co.NONE).sum()), "a walk leaves its graph"
        assert (got[3].reshape(G, n) == via[lo:hi]).all(), (n, lo)


def test_random_small_graphs():
    for a, w in co.small_cases():
        n = a.shape[0]
        words = co.pack(a, 2, seed=n)[1]
        got = run(words, n, np.arange(n), w)
        co.same(got, co.reference(a, w, range(n)).at(), (a.astype(int).tolist(), w.tolist()))
        rows = [co.brute(a, w, s) for s in range(n)]
        for s in range(n):
            assert (got[0][s] == rows[s][0]).all() and (got[1][s] == rows[s][1]).all() and (got[2][s] == rows[s][2]).all()


# ---- the families ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", co.FAMILIES)
def test_families(family):
    for n in co.SIZES:
        s = co.Case(n, family)
        co.check(run, s.words, s, variants=n <= 129)


def test_chain_300_and_detour():
    """299 rounds; the cheapest route is not the shortest, and the least of two tying predecessors wins"""
    s = co.Case(300, "chain")
    cost, pred, ln, via, res = run(s.words, 300, [0], s.w)
    assert res == {"n_reached": 299, "n_via": 299 * 298 // 2, "max_cost": int(s.w[1:].sum()), "longest": 299}
    assert (pred[0, 1:] == np.arange(299)).all() and (via[1:] == 298 - np.arange(299)).all() and via[0] == 0
    s = co.Case(7, "detour")
    cost, pred, ln, via, res = run(s.words, 7, [0], s.w)
    # s h a b c t u: t over a -> c at 1 + 1 + 2 although h -> t has fewer edges; c from a, not from b
    assert cost[0].tolist() == [8, 5, 1, 1, 2, 4, 5] and ln[0].tolist() == [5, 1, 1, 1, 2, 3, 4], (cost, ln)
    assert pred[0].tolist() == [6, 0, 0, 0, 2, 4, 5] and via.tolist() == [0, 0, 4, 0, 3, 2, 1], (pred, via)


def test_layers_by_construction():
    for n in (33, 129, 2049):
        s = co.Case(n, "layers")
        widths = co.layer_widths(n)
        got = run(s.words, n, s.src, s.w)
        rows = [co.layers_want(widths, co.LAYER_WEIGHTS, q) for q in s.src]
        for q in range(len(s.src)):
            assert (got[0][q] == rows[q][0]).all() and (got[1][q] == rows[q][1]).all() and (got[2][q] == rows[q][2]).all(), (n, q)
        assert (got[3] == sum(r[3].astype(np.int64) for r in rows)).all()
    co.check_large_layers(run, 2049)


def test_max_cost_is_a_filter():
    """every bound from 1 to past the largest cost on a graph with many distinct costs"""
    s = co.Case(65, "random4")
    x = co.reference(s.a, s.w, s.src)
    top = int(x.cost[x.cost != co.NONE].max())
    for b in range(1, top + 2):
        got = run(s.words, 65, s.src, s.w, b)
        co.same(got, x.at(b), b)
        assert got[4]["max_cost"] <= b
    co.same(run(s.words, 65, s.src, s.w, 0xFFFFFFFF), x.at(), "the largest bound")


def test_duplicate_sources_double_via():
    s = co.Case(129, "islands")
    one = run(s.words, 129, [0], s.w)
    two = run(s.words, 129, [0, 0], s.w)
    assert one[4]["n_via"] > 0 and (two[3] == 2 * one[3]).all()
    assert two[4] == dict(one[4], n_reached=2 * one[4]["n_reached"], n_via=2 * one[4]["n_via"])
    for k in range(3):
        assert (two[k][0] == one[k][0]).all() and (two[k][1] == one[k][0]).all()
    mixed = run(s.words, 129, [64, 0, 64], s.w)
    assert (mixed[3] == one[3] + 2 * run(s.words, 129, [64], s.w)[3]).all() and (mixed[0][1] == one[0][0]).all()


# ---- unit weights: the closure and the paths ---------------------------------------------------------
@pytest.mark.parametrize("family,n", (("medium", 65), ("ring", 33), ("two-cliques", 31), ("sparse", 129), ("star", 17)))
def test_unit_weights_against_closure_and_paths(family, n):
    e = engine()
    s = cc.synthetic(n, family)
    hops = cc.run_host(e, s.words, n)[1]
    cost, pred, ln, via, res = run(s.words, n, np.arange(n), np.ones(n, np.uint16))
    assert (np.where(cost == co.NONE, 0, cost) == hops).all() and (ln == hops).all()
    src, dst = (x.ravel().astype(np.uint32) for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    lens, nodes, pvia, pres = pc.run_host(e, hops, n, src, dst, n)
    assert (lens.reshape(n, n) == ln).all() and (pvia == via).all() and pres["n_via"] == res["n_via"] and pres["longest"] == res["longest"]
    before = np.where(lens > 0, nodes[np.arange(n * n), np.maximum(lens.astype(np.int64), 1) - 1], co.NO_PRED)
    assert (before.reshape(n, n) == pred).all()
    assert res["n_reached"] == pres["n_found"] == int((hops > 0).sum())


# ---- the plan and the knob ---------------------------------------------------------------------------
def test_plan():
    e = engine()
    plan = e.debug_reach_cost_plan
    cap = 160 << 10
    assert e.get_tuning("cost_lds_bytes") == cap
    for n in list(range(0, (1 << 15) + 1, 97)) + [1, 2047, 2048, 2049, 4095, 4096, 4097, 1 << 15]:
        p = plan(n)
        bw = -(-n // 32)
        assert p["lane_words"] == (1 if bw <= 64 else 2 if bw <= 128 else 4) and p["block"] == 1024, (n, p)
        assert p["row_in_lds"] == 1 and p["weights_in_lds"] <= p["row_in_lds"], (n, p)
        staged = 4 * n * p["row_in_lds"] + 2 * n * p["weights_in_lds"]
        vectors = 2 * 4 * bw
        assert staged + vectors <= p["lds_bytes"] <= staged + vectors + 96 and p["lds_bytes"] <= cap and p["lds_bytes"] % 16 == 0, (n, p)
        assert (p["t_rows"], p["t_cols"]) == (128, 1024) and p["t_grid"] == p["t_row_tiles"] * p["t_col_tiles"] == -(-n // 128) * -(-n // 1024), (n, p)
    # the weights leave LDS once, the row stays up to 2^15 end points
    gone = co.first_n(plan, lambda p: not p["weights_in_lds"])
    assert 6 * (gone - 1) < cap <= 6 * gone + 2 * 4 * -(-gone // 32) + 96, gone
    assert plan(gone - 1)["weights_in_lds"] == 1 and plan(gone)["row_in_lds"] == 1 and plan(1 << 15)["lds_bytes"] > 128 << 10
    # the budget: the weights are dropped first, then the row
    n = 300
    with e.tuning(cost_lds_bytes=plan(n)["lds_bytes"]):
        assert (plan(n)["row_in_lds"], plan(n)["weights_in_lds"]) == (1, 1)
    with e.tuning(cost_lds_bytes=4 * n + 2 * n - 1):
        assert (plan(n)["row_in_lds"], plan(n)["weights_in_lds"]) == (1, 0)
    with e.tuning(cost_lds_bytes=4 * n - 1):
        assert (plan(n)["row_in_lds"], plan(n)["weights_in_lds"]) == (0, 0)
    with e.tuning(cost_lds_bytes=0):
        assert (plan(n)["row_in_lds"], plan(n)["weights_in_lds"]) == (0, 0) and plan(n)["lds_bytes"] == plan(0)["lds_bytes"] + 2 * 4 * 12
        assert plan(1 << 15)["row_in_lds"] == 0
    p = _capi.pg_reach_cost_plan()
    assert lib.pg_debug_reach_cost_plan(e.h, (1 << 15) + 1, C.byref(p)) == _capi.PG_EINVAL


def test_knob_range_and_result():
    e = engine()
    for bad in (-1, (160 << 10) + 1):
        with pytest.raises(R.PolicyError):
            e.set_tuning("cost_lds_bytes", bad)
    s = co.Case(129, "random4")
    want = run(s.words, 129, s.src, s.w)
    for v in (0, 1, 4 * 132, 160 << 10):
        with e.tuning(cost_lds_bytes=v):
            got = run(s.words, 129, s.src, s.w)
        assert all((x == y).all() for x, y in zip(got[:4], want[:4])) and got[4] == want[4]
    assert e.get_tuning("cost_lds_bytes") == 160 << 10


# ---- the arguments -----------------------------------------------------------------------------------
def test_einval():
    e = engine()
    m = np.zeros(8, np.uint32)
    bad, keep = co.bad_specs(m.ctypes.data)
    for spec, with_res, names in bad:
        res = _capi.pg_reach_cost_result(7, 7, 7, 7)
        code = lib.pg_debug_reach_cost_host(e.h, C.byref(spec) if spec is not None else None, None, None, None, None,
                                            C.byref(res) if with_res else None)
        assert code == _capi.PG_EINVAL and names in lib.pg_last_error(e.h).decode(), (names, code, lib.pg_last_error(e.h))
        assert co.result_dict(res) == dict.fromkeys(co.RESULT_FIELDS, 7)
    del keep


def test_nothing_to_do():
    """n == 0 or n_src == 0: PG_OK, the result zeroed, out_via cleared when given and n > 0, nothing else written"""
    e = engine()
    s = co.Case(33, "ring")
    got = run(s.words, 33, np.zeros(0, np.uint32), s.w)
    assert got[4] == dict.fromkeys(co.RESULT_FIELDS, 0) and (got[3] == 0).all() and got[0].size == 0
    res = _capi.pg_reach_cost_result(7, 7, 7, 7)
    buf = np.full(8, 0xAB, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    code = lib.pg_debug_reach_cost_host(e.h, C.byref(_capi.pg_reach_cost_spec(None, 0, 1, None, None, 0, None, 5)), p, p, p, p, C.byref(res))
    assert code == 0 and co.result_dict(res) == dict.fromkeys(co.RESULT_FIELDS, 0) and (buf == 0xAB).all()
    # nothing selected: nothing is reached, every entry is still written
    got = run(s.words, 33, s.src, s.w, 0, ())
    assert got[4] == dict.fromkeys(co.RESULT_FIELDS, 0) and (got[0] == co.NONE).all() and (got[1] == co.NO_PRED).all()
    assert (got[2] == 0).all() and (got[3] == 0).all()


def test_wrapper_host():
    """Engine.reachability_cost on the chain policy by its host route, against the reference on the oracle's codes"""
    co.check_wrapper(cc.chain(((0, 5), (2, 9), (11, 0))), host=True)
