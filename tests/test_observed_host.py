"""The observed reachability on the host (no GPU): pg_debug_reach_observed_host running the tables and the
per-flow code of pg_reach_observed (observed.hpp, the functions the kernel calls) against numpy over the
scenarios of tests/observed_cases.py -- the row and word edges with the flow-count edges, a full grid of
the plan plus one flow, the address and service edges, lists chosen with the probe, contention, the plan
under the knobs, accumulation, every PG_EINVAL and the empty cases -- and the plan and the probe themselves.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import observed_cases as oc
from vpp_amd import _capi
from vpp_amd import renderer as R
from vpp_amd._capi import lib


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


def run(c, **kw):
    return oc.run_host(engine(), c, **kw)


def test_plan():
    """the cells are a power of two of at least twice the list; the knob decides what is staged; the budget
    is spent on the src table first"""
    e = engine()
    for n in (0, 1, 2, 3, 17, 64, 65, 2048, 2049, 1 << 20):
        p = e.debug_reach_observed_plan(n, 17, 3)
        cap = p["src_cap"]
        assert cap >= max(4, 2 * n) and cap & (cap - 1) == 0 and (cap == 4 or cap < 4 * n), (n, p)
        assert p["block"] % 64 == 0 and p["vec_flows"] >= 1 and p["grid"] >= 1
        assert p["lds_bytes"] == p["svc_bytes"] + 12 * (p["src_in_lds"] * p["src_cap"] + p["dst_in_lds"] * p["dst_cap"]), p
        assert p["lds_bytes"] <= 64 << 10
    with e.tuning(observed_lds_bytes=0):
        p = e.debug_reach_observed_plan(4, 4, 1)
        assert (p["src_in_lds"], p["dst_in_lds"]) == (0, 0)
    with e.tuning(observed_lds_bytes=12 * 8):
        assert e.debug_reach_observed_plan(4, 4, 1)["src_in_lds"] == 1 and e.debug_reach_observed_plan(4, 4, 1)["dst_in_lds"] == 0
        p = e.debug_reach_observed_plan(5, 4, 1)
        assert (p["src_in_lds"], p["dst_in_lds"]) == (0, 1)
    # 4096 services take more than the budget on their own: no table is staged beside them
    p = e.debug_reach_observed_plan(4, 4, 4096)
    assert p["svc_bytes"] > 64 << 10 and p["lds_bytes"] == p["svc_bytes"] <= 160 << 10 and (p["src_in_lds"], p["dst_in_lds"]) == (0, 0)
    plan = _capi.pg_reach_observed_plan()
    for bad in ((4, 4, 0), (4, 4, 4097), ((1 << 20) + 1, 4, 1), (4, (1 << 20) + 1, 1)):
        assert lib.pg_debug_reach_observed_plan(e.h, *bad, C.byref(plan)) == _capi.PG_EINVAL
    assert lib.pg_debug_reach_observed_plan(e.h, 4, 4, 1, None) == _capi.PG_EINVAL


def test_knobs():
    e = engine()
    assert e.get_tuning("observed_test_first") in (0, 1, 2) and e.get_tuning("observed_lds_bytes") == 160 << 10
    for key, bad in (("observed_test_first", 3), ("observed_test_first", -1), ("observed_lds_bytes", (160 << 10) + 1)):
        with pytest.raises(R.PolicyError):
            e.set_tuning(key, bad)


def test_probe():
    """a listed address is found where the probe says, an unlisted one ends at an empty cell; 0.0.0.0 and
    255.255.255.255 are addresses like any other"""
    e = engine()
    lst = np.array([0, 0xFFFFFFFF, 5, 5, 9], np.uint32)
    steps, slot, cap = e.debug_reach_observed_probe(lst, np.array([0, 0xFFFFFFFF, 5, 9, 1, 0xFFFFFFFE], np.uint32))
    assert cap == 16 and (steps >= 1).all() and (steps <= 4).all() and (slot < cap).all()
    steps, slot, cap = e.debug_reach_observed_probe(lst[:0], np.array([0, 0xFFFFFFFF], np.uint32))
    assert cap == 4 and (steps == 1).all()


@pytest.mark.parametrize("n_dst", oc.N_DST)
def test_rows_and_words(n_dst):
    oc.rows_and_words(run, engine(), n_dst)


def test_full_grid():
    oc.full_grid(run, engine())


def test_address_edges():
    oc.address_edges(run, engine())


def test_collisions():
    oc.collisions(run, engine())


def test_service_edges():
    oc.service_edges(run, engine())


def test_contention():
    oc.contention(run, engine())


def test_table_paths():
    oc.table_paths(run, engine())


def test_split_launches():
    oc.split_launches(run, engine())


def test_accumulate():
    oc.accumulate(run, engine())


def test_many_services():
    oc.many_services(run, engine())


def test_by_hand():
    """two src (one listed twice), three dst, TCP 80 and UDP 53: five flows, one of each status and a second match"""
    src, dst = [10, 20, 10], [30, 40, 50]
    flows = ([10, 11, 20, 20, 20], [40, 40, 41, 50, 30], [0] * 5, [80, 80, 80, 81, 53], [0, 0, 0, 0, 1])
    c = oc.case(src, dst, [(0, 0, 80), (1, 0, 53)], flows)
    got = run(c)
    assert got.flow.tolist() == [oc.MATCHED, oc.NO_SRC, oc.NO_DST, oc.NO_SVC, oc.MATCHED]
    A = lambda j: 2 << (2 * j)
    assert got.packed.reshape(-1).tolist() == [A(1), 0, A(1), 0, A(0), 0] and got.svc_flows.tolist() == [1, 1]
    assert got.result == {"n_matched": 2, "n_no_src": 1, "n_no_dst": 1, "n_no_svc": 1, "n_cells": 3}
    oc.same(got, oc.expected(c), "by hand")


def test_einval_and_empty():
    e = engine()
    c = oc.random_case(5, 7, 2, 64, seed=1)
    out = np.full(64, 0xFFFFFFFF, np.uint32)

    def call(spec, soa, n, packed, res):
        return lib.pg_debug_reach_observed_host(e.h, C.byref(spec) if spec is not None else None,
                                                C.byref(soa) if soa is not None else None, n, packed, None, None,
                                                C.byref(res) if res is not None else None)

    oc.einval(call, e, c, out.ctypes.data, [a.ctypes.data for a in c.flows])
    assert (out == 0xFFFFFFFF).all()
    oc.empties(run, e)


def test_wrapper():
    """Engine.debug_reach_observed_host against numpy"""
    e = engine()
    c = oc.random_case(65, 33, 3, 4096, seed=1, match=True)
    w = oc.expected(c)
    packed, flow, counts, res = e.debug_reach_observed_host(c.src, c.dst, c.services, c.flows, flags=oc.MATCH_SRC_PORT)
    assert (packed == w.packed).all() and (flow == w.flow).all() and (counts == w.svc_flows).all() and res == w.result
