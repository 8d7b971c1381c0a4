"""The reachability dominators on the host (no GPU): pg_debug_reach_dominators_host running the per-word
code and the plan of pg_reach_dominators (dominators.hpp, the functions the kernels and the launch call)
against numpy on the graphs of tests/dominators_cases.py: the closure's families and four with a
written-down answer, the islands at the sizes where the plan changes, a chain of 300, the torch reference
of the large GPU test pinned to numpy, the chain policy through the oracle, and the arguments.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import closure_cases as cc
import diff_cases as dc
import dominators_cases as dm
from vpp_amd import _capi
from vpp_amd import device as D
from vpp_amd import renderer as R
from vpp_amd._capi import lib


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


def run(*args, **kw):
    return dm.run_host(engine(), *args, **kw)


# ---- the reference alone -------------------------------------------------------------------------
@pytest.mark.parametrize("family", dm.NEW_FAMILIES)
def test_known_answers(family):
    """the written-down answers of the new families for the entry set {0} against the reference"""
    for n in dm.SIZES:
        x = dm.expected(n, family, (0,))
        dom, idom, cut = dm.known(n, family)
        assert (x.dom == dom).all() and (x.cut == cut).all(), (family, n)
        assert (np.where(x.idom == dm.NO_IDOM, -1, x.idom.astype(np.int64)) == idom).all(), (family, n)
    # what the families are there for
    x = dm.expected(4, "diamond", (0,))
    assert x.result == {"n_reached": 4, "n_chokes": 0, "top": dm.NONE, "top_cut": 0, "depth": 1, "rounds": 2} and x.idom[3] == 0
    x = dm.expected(64, "bowtie", (0,))
    assert x.result["top"] == 32 and x.result["top_cut"] == 31 and x.result["n_chokes"] == 1
    assert dm.expected(65, "ladder", (0,)).result["n_chokes"] == 0
    x = dm.expected(257, "tree", (0,))
    assert x.result["n_chokes"] > 20 and x.result["depth"] >= 6


def test_definition_properties():
    """a single entry dominates every reached end point; an entry is dominated by itself only; the sizes
    along a chain of dominators are distinct"""
    for family in ("medium", "sparse", "two-cliques", "tree"):
        for ent in dm.entry_sets(65)[:3]:
            x = dm.expected(65, family, ent)
            for e in set(ent):
                assert x.dom[e].sum() == 1 and x.dom[e, e] and x.idom[e] == dm.NO_IDOM
            if len(set(ent)) == 1:
                assert (x.dom[:, ent[0]] == x.reached).all()
            assert not x.dom[~x.reached].any()
            for v in np.flatnonzero(x.reached):
                sizes = x.size[x.dom[v]]
                assert len(set(sizes.tolist())) == len(sizes)


@pytest.mark.parametrize("family", ("medium", "two-cliques", "tree", "chain"))
def test_torch_reference(family):
    """the torch route of the large GPU test, on the CPU, bit for bit against the numpy reference"""
    import torch
    for n in (17, 65, 257):
        a = dm.edge_matrix(dm.graph(n, family).codes)
        for ent in dm.entry_sets(n):
            x = dm.expected(n, family, ent)
            dom, idom, cut, res = dm.torch_expected(torch.from_numpy(a), ent, "cpu")
            assert res == x.result, (family, n, ent, res, x.result)
            assert (dom.numpy() == x.dom).all() and (cut.numpy() == x.cut).all() and (idom.numpy() == x.idom).all()


# ---- the host twin -------------------------------------------------------------------------------
@pytest.mark.parametrize("family", dm.FAMILIES)
def test_synthetic(family):
    for n in dm.SIZES:
        s = dm.graph(n, family)
        if n & 15:
            assert (s.words[:, :, -1] >> (2 * (n & 15))).any(), "no garbage in the padding"
        dm.check(run, s.words, s, n, family)


def test_chain_300():
    """many cheap rounds: Dom is lower-triangular, idom(v) = v - 1, cut[k] = 299 - k"""
    n = 300
    s = dm.graph(n, "chain", 1)
    x = dm.expected(n, "chain", (0,), None, 1)
    assert x.result == {"n_reached": n, "n_chokes": n - 2, "top": 1, "top_cut": n - 2, "depth": n - 1, "rounds": n - 1}
    assert (x.dom == np.tri(n, dtype=bool)).all() and (x.idom[1:] == np.arange(n - 1)).all() and (x.cut == n - 1 - np.arange(n)).all()
    dm.same(run(s.words, n, (0,)), x, "chain 300")


def test_plan():
    e = engine()
    assert dm.plan_sizes(e) == (2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)
    assert tuple((e.debug_reach_dominators_plan(n)["lane_words"], e.debug_reach_dominators_plan(n)["col_tiles"])
                 for n in dm.plan_sizes(e)) == dm.PLAN_SHAPES
    for n in (0, 1, 16, 17, 2047, 2048, 4096, 8191, 8192, 1 << 15):
        p = e.debug_reach_dominators_plan(n)
        cols = n + 1   # (the end points and the reached column)
        assert p["lane_words"] in (1, 2, 4) and p["tile_cols"] == 2048 * p["lane_words"] and p["tile_rows"] == 16, (n, p)
        assert p["row_tiles"] == -(-n // 16) and p["col_tiles"] == -(-cols // p["tile_cols"]), (n, p)
        assert p["round_grid"] == p["row_tiles"] * p["col_tiles"] and p["finish_grid"] == n
        assert p["t_grid"] == p["t_row_tiles"] * p["t_col_tiles"] and p["t_row_tiles"] == -(-n // p["t_rows"])
        assert p["t_col_tiles"] * p["t_cols"] >= n and p["cut_grid"] == -(-n // p["cut_rows"]) * -(-n // p["cut_cols"])
    assert e.debug_reach_dominators_plan(1 << 15)["col_tiles"] == 5
    p = _capi.pg_reach_dominators_plan()
    assert lib.pg_debug_reach_dominators_plan(e.h, (1 << 15) + 1, C.byref(p)) == _capi.PG_EINVAL
    assert lib.pg_debug_reach_dominators_plan(e.h, 4, None) == _capi.PG_EINVAL


@pytest.mark.parametrize("k", range(9))
def test_islands(k):
    """the islands at the nine sizes around the lane-width and column-tile cuts: the preconditions on the
    reference alone, and the host twin against the embedded 240-node answer"""
    n = dm.plan_sizes(engine())[k]
    c = dm.IslandCase(n)
    c.non_trivial()
    d, i, cut, res = run(c.s.words, n, c.entry)
    assert res == c.result, (n, res, c.result)
    assert (i == c.idom).all() and (cut == c.cut).all()
    assert (d[c.idx] == c.dom_rows()).all() and not np.delete(d, c.idx, axis=0).any()


# ---- real engines --------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", ((), ((11, 0),), ((11, 0), (3, 9)), ((0, 5), (2, 9))), ids=("path", "ring", "chord", "skips"))
def test_chain_policy(extra):
    c = cc.chain(extra)
    m = c.e.debug_reach_matrix_host(cc.CHAIN_IPS, cc.CHAIN_IPS, cc.CHAIN_SERVICES, words=False)
    assert (m == np.stack([dc.pack(v) for v in c.codes])).all()
    for ent in ((0,), (3,), (11, 4, 11), ()):
        for sel in (None, (0,), (2,)):
            dm.same(dm.run_host(c.e, m, cc.CHAIN_N, ent, sel), dm.chain_expected(c, ent, sel), (extra, ent, sel))


def test_dominators_diff_host():
    """matrix -> dominators -> diff on the host twins from two engines: the skips 0 -> 5 and 2 -> 9 take
    c1 .. c4 out of Dom(c5 ..) and more; OPENED lists exactly the (v, k) that became dominators"""
    before, after = cc.chain(((0, 5), (2, 9))), cc.chain()
    doms = []
    for c in (before, after):
        m = c.e.debug_reach_matrix_host(cc.CHAIN_IPS, cc.CHAIN_IPS, cc.CHAIN_SERVICES, words=False)
        doms.append(dm.run_host(c.e, m, cc.CHAIN_N, (0,))[0])
    xb, xa = dm.chain_expected(before, (0,)), dm.chain_expected(after, (0,))
    opened = ~xb.dom & xa.dom
    assert opened.sum() > 0 and not (xb.dom & ~xa.dom).any()
    k, changes, _, _ = engine().debug_reach_diff_host(doms[0], doms[1], cc.CHAIN_N, dc.OPENED, row_changes=False)
    row, col, cb, ca = D.unpack_changes(changes[:k])
    assert k == int(opened.sum()) and (np.stack([row, col], axis=1) == np.argwhere(opened)).all()
    assert (cb == 0).all() and (ca == 2).all()


def test_reachability_dominators_host():
    c = cc.chain(((0, 5), (2, 9)))
    for pods, entry in ((cc.CHAIN_PODS, ["ns/c0"]), (cc.CHAIN_PODS[::-1], ["ns/c1", "ns/c3"]), (cc.CHAIN_PODS, [])):
        got = c.e.reachability_dominators(pods, cc.CHAIN_SERVICES, entry, host=True)
        assert got == dm.chokepoints_want(c, pods, entry), (pods, entry)
    chokes, idom, res = cc.chain().e.reachability_dominators(cc.CHAIN_PODS, cc.CHAIN_SERVICES, ["ns/c0"], host=True)
    assert chokes == [("ns/c%d" % k, 11 - k) for k in range(1, 11)] and idom == [None] + cc.CHAIN_PODS[:-1]
    assert res == {"n_reached": 12, "n_chokes": 10, "top": "ns/c1", "top_cut": 10, "depth": 11, "rounds": 11}
    with pytest.raises(ValueError):
        c.e.reachability_dominators(cc.CHAIN_PODS[:4], cc.CHAIN_SERVICES, ["ns/c7"], host=True)
    assert c.e.reachability_dominators(cc.CHAIN_PODS, [], ["ns/c0"], host=True)[0] == []


# ---- arguments ---------------------------------------------------------------------------------
def call(e, spec, result=True, dom=None, idom=None, cut=None):
    res = _capi.pg_reach_dominators_result(7, 7, 7, 7, 7, 7)
    p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    code = lib.pg_debug_reach_dominators_host(e.h, C.byref(spec) if spec is not None else None, p(dom), p(idom), p(cut),
                                              C.byref(res) if result else None)
    return code, res


def test_einval():
    e = engine()
    w = np.zeros(8, np.uint32)
    bad, keep = dm.bad_specs(w.ctypes.data)
    for spec, with_res, names in bad:
        code, _ = call(e, spec, with_res)
        assert code == _capi.PG_EINVAL, (names, code)
        assert names in lib.pg_last_error(e.h).decode(), (names, lib.pg_last_error(e.h))
    del keep
    assert lib.pg_debug_reach_dominators_host(None, None, None, None, None, None) == _capi.PG_EINVAL
    ent = np.array([1, 3, 3], np.uint32)
    code, res = call(e, _capi.pg_reach_dominators_spec(w.ctypes.data, 4, 1, None, ent.ctypes.data, 3))
    assert code == 0 and dm.result_dict(res) == {"n_reached": 2, "n_chokes": 0, "top": dm.NONE, "top_cut": 0, "depth": 0, "rounds": 0}


def test_no_end_points():
    """n == 0: PG_OK, the result zeroed, nothing else written; the matrix may be null"""
    e = engine()
    d, c, i = np.full(4, dm.FILL, np.uint32), np.full(4, dm.FILL, np.uint32), np.full(4, 0xEEEE, np.uint16)
    code, res = call(e, _capi.pg_reach_dominators_spec(None, 0, 1, None, None, 0), True, d, i, c)
    assert code == 0 and dm.result_dict(res) == dict.fromkeys(dm.RESULT_FIELDS, 0)
    assert (d == dm.FILL).all() and (c == dm.FILL).all() and (i == 0xEEEE).all()
