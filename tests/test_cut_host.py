"""The reachability cut on the host (no GPU): pg_debug_reach_cut_host running the per-word code and the
plan of pg_reach_cut (cut.hpp, the functions the kernels and the launch call) against the references of
tests/cut_cases.py: the definition by brute force on small random graphs, the plain-Python maximum flow on
the closure's families and on four families with a written-down answer, scipy's maximum flow pinned to the
Python one, the plan at its boundaries, the chain policy through the oracle, and the arguments.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import closure_cases as cc
import cut_cases as ct
from vpp_amd import _capi
from vpp_amd import renderer as R
from vpp_amd._capi import lib


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


def run(*args, **kw):
    return ct.run_host(engine(), *args, **kw)


# ---- the references alone --------------------------------------------------------------------------
def test_residual_rule_is_the_definition():
    """flow() -- the residual rule after a depth-first maximum flow -- against brute(), the definition"""
    apart = separable = 0
    for a, E, T in ct.small_cases():
        b, f = ct.brute(a, E, T), ct.flow(a, E, T)
        assert b.same(f) and (b.reach_near == f.reach_near).all() and (b.reach_far == f.reach_far).all(), (a.astype(int).tolist(), E, T)
        separable += b.cut_size is not None
        apart += b.cut_size is not None and not (b.near == b.far).all()
    assert separable >= 60 and apart >= 5, (separable, apart)


@pytest.mark.parametrize("family", ct.NEW_FAMILIES)
def test_known_answers(family):
    """the written-down answers of the new families against the reference"""
    seen = 0
    for n in ct.SIZES + ct.SMALL_SIZES:
        want = ct.known(n, family)
        if want is None:
            continue
        a, E, T = ct.new_family(n, family)
        x = (ct.flow if n < ct.SCIPY_FROM else ct.flow_scipy)(a, E, T)
        assert x.cut_size == want["cut_size"] and np.flatnonzero(x.near).tolist() == want["near"], (family, n)
        assert np.flatnonzero(x.far).tolist() == want["far"], (family, n)
        assert (int(x.reach_near.sum()), int(x.reach_far.sum())) == (want["near_reach"], want["far_reach"]), (family, n)
        if n <= 12:
            assert ct.brute(a, E, T).same(x)
        seen += 1
    assert seen >= 13


@pytest.mark.parametrize("family", ("medium", "two-cliques", "dense", "layers", "grid", "zigzag"))
def test_scipy_reference(family):
    """scipy's maximum flow with the residual rule in numpy, pinned to the Python flow"""
    for n in (9, 17, 65, 129):
        a = ct.edge_matrix(ct.graph(n, family).codes)
        for E, T in ct.end_sets(n, family, a):
            f, s = ct.flow(a, E, T), ct.flow_scipy(a, E, T)
            assert f.same(s) and (f.reach_near == s.reach_near).all() and (f.reach_far == s.reach_far).all(), (family, n, E, T)


# ---- the host twin ---------------------------------------------------------------------------------
def test_small_graphs():
    """the twin against the definition"""
    for a, E, T in ct.small_cases():
        n = a.shape[0]
        s = ct.Graph(a, "layers", 2, seed=n)
        x = ct.brute(a, E, T)
        for max_cut in sorted({0, max((x.cut_size or 0) - 1, 0), x.cut_size or 0, ct.LARGE}):
            ct.same(run(s.words, n, E, T, max_cut), x, a, E, T, max_cut, (a.astype(int).tolist(), E, T, max_cut))


@pytest.mark.parametrize("family", ct.FAMILIES)
def test_synthetic(family):
    for n in ct.SIZES:
        s = ct.graph(n, family)
        if n & 15:
            assert (s.words[:, :, -1] >> (2 * (n & 15))).any(), "no garbage in the padding"
        ct.check(run, s.words, s, n, family)
        if family in ct.NEW_FAMILIES:
            ct.check_known(run, s.words, s, n, family)


def test_zigzag_reroutes():
    """one gadget: the first route takes d, the second has to push it back"""
    s = ct.graph(8, "zigzag")
    c, pv, nx, r = run(s.words, 8, (0,), (3,))
    assert r["cut_size"] == 2 and r["reroutes"] == 1 and r["n_paths"] == 2, r
    assert (pv[[1, 4, 5]] == [0, 1, 4]).all() and (nx[[1, 4, 5]] == [4, 5, 3]).all()   # e a b1 b2 t
    assert (pv[[6, 7, 2]] == [0, 6, 7]).all() and (nx[[6, 7, 2]] == [7, 2, 3]).all()   # e c1 c2 d t
    _, _, _, one = run(s.words, 8, (0,), (3,), 0)
    assert one["capped"] == 1 and one["n_paths"] == 1 and one["reroutes"] == 0 and one["cut_size"] == ct.NO_CUT


def test_levels_bound():
    """a chain of 300: one path; no search runs more than 2 n + 2 levels"""
    n = 300
    s = ct.graph(n, "chain", 1)
    c, pv, nx, r = run(s.words, n, (0,), (n - 1,))
    assert r["cut_size"] == 1 and r["near_reach"] == 1 and r["far_reach"] == n - 2 and r["levels"] <= 5 * (2 * n + 2), r
    assert np.flatnonzero(c & ct.NEAR).tolist() == [1] and np.flatnonzero(c & ct.FAR).tolist() == [n - 2]
    assert (pv[1:n - 1] == np.arange(n - 2)).all() and (nx[1:n - 1] == np.arange(2, n)).all()


def test_plan():
    e = engine()
    # (64 and 128 bit-words of a row are the last that one step of 1 and of 2 lane words covers)
    assert ct.plan_sizes(e) == (2048, 2049, 2050, 4096, 4097, 4098)
    assert tuple(ct.plan_of(e, n)["lane_words"] for n in ct.plan_sizes(e)) == (1, 2, 2, 2, 4, 4)
    for n in (0, 1, 31, 32, 33, 2048, 2049, 4096, 4097, 8193, 1 << 15):
        p = ct.plan_of(e, n)
        words = -(-n // 32)
        assert p["lane_words"] in (1, 2, 4) and p["level_block"] == 1024 and p["group_nodes"] == 32, (n, p)
        assert p["level_grid"] == words and p["row_steps"] == -(-words // (64 * p["lane_words"])), (n, p)
        assert p["row_steps"] <= 1 or p["lane_words"] == 4
        assert p["t_grid"] == p["t_row_tiles"] * p["t_col_tiles"] and p["t_row_tiles"] == -(-n // p["t_rows"])
        assert p["t_col_tiles"] * p["t_cols"] >= n and p["finish_grid"] == 1 and p["finish_block"] * 32 >= n
    assert ct.plan_of(e, 1 << 15)["row_steps"] == 4
    p = _capi.pg_reach_cut_plan()
    assert lib.pg_debug_reach_cut_plan(e.h, (1 << 15) + 1, C.byref(p)) == _capi.PG_EINVAL
    assert lib.pg_debug_reach_cut_plan(e.h, 4, None) == _capi.PG_EINVAL


@pytest.mark.parametrize("k", range(6))
def test_layers_at_plan_sizes(k):
    """layers at the sizes where the plan changes, against the written-down answer"""
    n = ct.plan_sizes(engine())[k]
    widths = [3, 40, 5, n - 100, 5, 44, 3]
    c, pv, nx, r = run(ct.layers_words(widths), n, (0, 1, 2), (n - 3, n - 2, n - 1))
    assert {f: r[f] for f in ct.EXACT} == dict(zip(ct.EXACT, (1, 0, 0, 5, 5, 43, n - 52))), r
    assert np.flatnonzero(c & ct.NEAR).tolist() == list(range(43, 48)) and np.flatnonzero(c & ct.FAR).tolist() == list(range(n - 52, n - 47))
    assert int(((pv != ct.NO_HOP) & (pv < 3)).sum()) == 5 and int(((nx != ct.NO_HOP) & (nx >= n - 3)).sum()) == 5


# ---- real engines ----------------------------------------------------------------------------------
def test_reachability_cut_host():
    c = cc.chain(((0, 5), (2, 9)))
    for pods, entry, target, max_cut in ct.WRAPPER_CASES:
        ct.check_wrapper(c, c.e.reachability_cut(pods, cc.CHAIN_SERVICES, entry, target, max_cut, host=True), pods, entry, target, max_cut)
    near, far, routes, res = cc.chain().e.reachability_cut(cc.CHAIN_PODS, cc.CHAIN_SERVICES, ["ns/c0"], ["ns/c11"], host=True)
    assert near == ["ns/c1"] and far == ["ns/c10"] and routes == [cc.CHAIN_PODS] and res["cut_size"] == 1
    with pytest.raises(ValueError):
        c.e.reachability_cut(cc.CHAIN_PODS[:4], cc.CHAIN_SERVICES, ["ns/c0"], ["ns/c7"], host=True)
    assert c.e.reachability_cut(cc.CHAIN_PODS, [], ["ns/c0"], ["ns/c3"], host=True)[3]["cut_size"] == 0


# ---- arguments -------------------------------------------------------------------------------------
def call(e, spec, result=True, cut=None, prev=None, nxt=None):
    res = _capi.pg_reach_cut_result(*[7] * 9)
    p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    code = lib.pg_debug_reach_cut_host(e.h, C.byref(spec) if spec is not None else None, p(cut), p(prev), p(nxt),
                                       C.byref(res) if result else None)
    return code, res


def test_einval():
    e = engine()
    w = np.zeros(8, np.uint32)
    bad, keep = ct.bad_specs(w.ctypes.data)
    for spec, with_res, names in bad:
        code, _ = call(e, spec, with_res)
        assert code == _capi.PG_EINVAL, (names, code)
        assert names in lib.pg_last_error(e.h).decode(), (names, lib.pg_last_error(e.h))
    del keep
    assert lib.pg_debug_reach_cut_host(None, None, None, None, None, None) == _capi.PG_EINVAL
    ids = np.array([1, 3, 3, 0], np.uint32)
    code, res = call(e, _capi.pg_reach_cut_spec(w.ctypes.data, 4, 1, None, ids.ctypes.data, 3, ids.ctypes.data + 12, 1, 1 << 15))
    want = dict(zip(ct.EXACT, (1, 0, 0, 0, 0, 2, 2)))
    assert code == 0 and {k: getattr(res, k) for k in ct.EXACT} == want and res.reroutes == 0


def test_no_end_points():
    """n == 0: PG_OK, the result zeroed, nothing else written; the matrix may be null"""
    e = engine()
    c, pv, nx = np.full(4, 0xEE, np.uint8), np.full(4, 0xEEEE, np.uint16), np.full(4, 0xEEEE, np.uint16)
    code, res = call(e, _capi.pg_reach_cut_spec(None, 0, 1, None, None, 0, None, 0, 4), True, c, pv, nx)
    assert code == 0 and ct.result_dict(res) == dict.fromkeys(ct.RESULT_FIELDS, 0)
    assert (c == 0xEE).all() and (pv == 0xEEEE).all() and (nx == 0xEEEE).all()
