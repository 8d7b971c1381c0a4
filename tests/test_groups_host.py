"""The reachability groups on the host (no GPU): pg_debug_reach_groups_host running the per-word code of
pg_reach_groups (groups.hpp, the functions the kernels call) against numpy on the synthetic matrices
and groupings of tests/groups_cases.py, and against numpy on the oracle's codes for real engines: the
fixture change of tests/diff_cases.py and four node_matrix topologies.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import closure_cases as cc
import diff_cases as dc
import groups_cases as gc
from vpp_amd import _capi
from vpp_amd import device as D
from vpp_amd import renderer as R
from vpp_amd._capi import lib


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


def run(*args, **kw):
    return gc.run_host(engine(), *args, **kw)


def shapes():
    cr = engine().debug_reach_groups_plan(1000)["chunk_rows"]
    return (1, 2, 17, cr - 1, cr, cr + 1, 2 * cr + 1), (1, 15, 16, 17, 31, 33, 64, 100, 1000)


def test_plan():
    e = engine()
    for n_dst in (1, 16, 17, 100, 1000, 4096, 4097, 1 << 20):
        p = e.debug_reach_groups_plan(n_dst)
        t = p["tile_words"]
        assert 1 <= p["chunk_rows"] <= 255 and 1 <= t <= 256 and t & (t - 1) == 0, (n_dst, p)
        assert t >= min(256, gc.row_words(n_dst)), (n_dst, p)


@pytest.mark.parametrize("code_mix", gc.MIXES)
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_synthetic(family, code_mix):
    """with the family `one` the n_src list makes a single group's rows straddle a flush"""
    srcs, dsts = shapes()
    for n_svc in (1, 3):
        for n_src in srcs:
            for n_dst in dsts:
                gc.check(run, gc.synthetic(n_svc, n_src, n_dst, family, code_mix), variants=n_dst in (17, 100))


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_garbage_in_padding(family):
    """random bits in the padding of every row's last word change nothing"""
    for n_dst in (1, 15, 17, 33, 100, 1000):
        s = gc.synthetic(2, 37, n_dst, family, seed=2)
        junk = dc.garbage(s.words.reshape(-1, gc.row_words(n_dst)), n_dst).reshape(s.words.shape)
        assert (junk[:, :, -1] >> (2 * (n_dst & 15))).any(), "no garbage in the padding"
        gc.check(run, s, words=junk, variants=False)


def test_status_values():
    """one pair of each status, by hand: NONE, SOME, ALL, EMPTY"""
    codes = np.array([[[0, 2, 2, 1], [3, 2, 2, 1]]], np.uint8)   # 1 x 2 x 4
    sg, dg = np.array([0, 0], np.uint32), np.array([0, 1, 1, 2], np.uint32)
    counts, words = run(gc.pack(codes[0])[None], 1, 2, 4, sg, dg, 1, 4)
    assert counts[0, 0].tolist() == [[1, 0, 0, 1], [0, 0, 4, 0], [0, 2, 0, 0], [0, 0, 0, 0]]
    status = D.unpack_groups(words, 4)
    assert status.shape == (1, 1, 4)
    assert status[0, 0].tolist() == [_capi.GROUPS_NONE, _capi.GROUPS_ALL, _capi.GROUPS_NONE, _capi.GROUPS_EMPTY]
    dg[0] = 1
    _, words = run(gc.pack(codes[0])[None], 1, 2, 4, sg, dg, 1, 4)
    assert D.unpack_groups(words, 4)[0, 0].tolist() == [_capi.GROUPS_EMPTY, _capi.GROUPS_SOME, _capi.GROUPS_NONE,
                                                        _capi.GROUPS_EMPTY]


# ---- real engines ------------------------------------------------------------------------------
def test_fixture_change():
    """both engines of the fixture change, grouped by the fixed rule, against the oracle's codes"""
    c = dc.matrix_change()
    src, dst = gc.doubled(c.src), gc.doubled(c.dst)
    sg, n_sg, dg, n_dg = gc.fixed_groups(len(src), len(dst))
    assert sg[-1] != sg[0] and dg[-1] != dg[0]          # the doubled end points sit in two groups
    statuses = []
    for e, codes in zip((c.e0, c.e1), c.matrix_codes(src, dst)):
        codes = codes.reshape(len(dc.SERVICES), len(src), len(dst))
        m = e.debug_reach_matrix_host(src, dst, dc.SERVICES, words=False)
        want = gc.expected(codes, sg, dg, n_sg, n_dg)
        gc.same(gc.run_host(e, m, len(dc.SERVICES), len(src), len(dst), sg, dg, n_sg, n_dg), want, "fixture")
        assert (want[1][:, :, -1] == _capi.GROUPS_EMPTY).all()
        statuses.append(want[1])
    assert (statuses[0] != statuses[1]).any(), "the edit moved no group pair"


@pytest.mark.parametrize("name", sorted(cc.TOPOLOGY_WANT))
def test_topology(name):
    e, ips, svc, _ = cc.topology(name)
    ends = gc.doubled(ips)
    codes = cc.oracle_codes(nm_world(name), ends, svc)
    sg, n_sg, dg, n_dg = gc.fixed_groups(len(ends), len(ends))
    m = e.debug_reach_matrix_host(ends, ends, svc, words=False)
    gc.same(gc.run_host(e, m, len(svc), len(ends), len(ends), sg, dg, n_sg, n_dg), gc.expected(codes, sg, dg, n_sg, n_dg), name)


def nm_world(name):
    import node_matrix as nm
    return nm.topo(name).world


def test_wrappers_host():
    c = dc.matrix_change()
    (cb, sb), (ca, sa) = gc.wrapper_want(c)
    for e, wc, ws in ((c.e0, cb, sb), (c.e1, ca, sa)):
        counts, status = e.reachability_groups(gc.SRC_GROUPS, gc.DST_GROUPS, dc.SERVICES, host=True)
        assert counts.dtype == np.uint64 and (counts == wc).all() and (status == ws).all()
    want = gc.diff_want(sb, sa)
    assert want, "the edit moved no group pair"
    assert c.e1.reachability_groups_diff(c.e0, gc.SRC_GROUPS, gc.DST_GROUPS, dc.SERVICES, host=True) == want
    assert c.e0.reachability_groups_diff(c.e0, gc.SRC_GROUPS, gc.DST_GROUPS, dc.SERVICES, host=True) == []
    assert c.e0.reachability_groups({}, gc.DST_GROUPS, dc.SERVICES, host=True)[0].shape == (len(dc.SERVICES), 0, 4, 4)


# ---- arguments ---------------------------------------------------------------------------------
def call(e, spec, counts, packed=None):
    p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    return lib.pg_debug_reach_groups_host(e.h, C.byref(spec) if spec is not None else None, p(counts), p(packed))


def test_einval():
    e = engine()
    w, out = np.zeros(64, np.uint32), np.full(64, gc.FILL64, np.uint64)
    *keep, bad = gc.bad_specs(w.ctypes.data)
    for what, spec, with_counts in bad:
        code = call(e, spec, out if with_counts else None)
        assert code == _capi.PG_EINVAL, (what, code)
        msg = lib.pg_last_error(e.h).decode()
        assert msg, what
        if what == "src id":
            assert "src_group[2]" in msg, msg
        if what == "dst id":
            assert "dst_group[3]" in msg, msg
    assert (out == gc.FILL64).all()
    assert lib.pg_debug_reach_groups_host(None, None, None, None) == _capi.PG_EINVAL
    S = _capi.pg_reach_groups_spec
    assert call(e, S(w.ctypes.data, 1, 4, 4, keep[0].ctypes.data, keep[0].ctypes.data, 1, 1), out) == 0
    assert out[:4].tolist() == [16, 0, 0, 0]


@pytest.mark.parametrize("empty", ("n_svc", "n_src", "n_dst"))
def test_empty_sides(empty):
    """an empty side: PG_OK, the counts cleared and every status EMPTY; nothing written with no group"""
    n = {"n_svc": 2, "n_src": 5, "n_dst": 7}
    n[empty] = 0
    sg, dg = np.zeros(n["n_src"], np.uint32), np.zeros(n["n_dst"], np.uint32)
    counts, words = run(np.zeros(0, np.uint32), n["n_svc"], n["n_src"], n["n_dst"], sg, dg, 3, 18)
    assert counts.shape == (n["n_svc"], 3, 18, 4) and not counts.any()
    if n["n_svc"]:
        assert (D.unpack_groups(words, 18) == _capi.GROUPS_EMPTY).all() and (words[:, :, 1] == 0xF).all()
    cbuf, pbuf = gc.buffers(1, 1, 1)
    spec, keep = gc.spec_of(None, n["n_svc"], n["n_src"], n["n_dst"], sg, dg, 0, 3)
    assert call(engine(), spec, cbuf, pbuf) == 0 and (cbuf == gc.FILL64).all() and (pbuf == gc.FILL).all()
