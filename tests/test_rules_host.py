"""Rule coverage on the host (no GPU): pg_debug_reach_rules_host runs the per-word code, the sink, the
windows and the flushes of pg_reach_rules (rules.hpp: the templates the kernel instantiates, the plan
the launch uses) work item by work item against the oracle (tests/rules_cases.py) -- every slot of
both histograms of every case, nothing filtered.

Form A on uni, uni-nocommon, uni-grouped and uni-wide, form B on nopair, uncovered, pair and big-pair
and with flags bit 0 clear; the services of reach_cases mix protocols <= 2 with ANY and out-of-range
codes, so both forms add into one call on the form A sets.
"""
import ctypes as C

import numpy as np
import pytest

import ports_cases as pc
import reach_cases as rc
import rules_cases as kr
from vpp_amd import _capi
from vpp_amd import device as D
from vpp_amd._capi import lib

TOPOLOGIES = sorted({rc.nm.SETS[s].topology for s in kr.SETS})


@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_oracle_preconditions(topology):
    """on the oracle alone: evals differs from the cells' slot marginal, at least 19 slots hit, and the
    two histograms agree where they must"""
    src, dst, svc, ev, ce = kr.case_hists(topology)   # (asserts the preconditions)
    wev, wce = kr.weighted(ev, ce)
    assert int(wce.sum()) == len(src) * len(dst) * len(svc)
    assert int(wev.sum()) > int(wce.sum())            # some pair takes more than one evaluation
    words = rc.case(topology).words
    assert (wce.sum(axis=0) == np.bincount((words >> 30).ravel(), minlength=4)).all()


@pytest.mark.parametrize("name", kr.SETS)
def test_equals_oracle(name):
    """the 37 x 53 case with all its services: both flags, and each histogram alone"""
    s, c = rc.set_case(name)
    src, dst, svc, ev, ce = kr.case_hists(s.spec.topology)
    wev, wce = kr.weighted(ev, ce)
    assert bool(c.any_services()) and bool(c.no_any_services())
    node = kr.run_host(s.e, src, dst, svc, node=True)
    tab = kr.run_host(s.e, src, dst, svc, node=False)
    kr.same(node, wev, wce, (name, "node"))
    kr.same(tab, wev, wce, (name, "per-table"))
    assert node[2] == tab[2] == kr.want_result(s.e, src, dst, np.ones(len(svc)), wev)
    only_e = kr.run_host(s.e, src, dst, svc, cells=False)
    only_c = kr.run_host(s.e, src, dst, svc, evals=False)
    assert only_e[1] is None and only_c[0] is None
    kr.same(only_e, wev, None, (name, "evals only"))
    kr.same(only_c, None, wce, (name, "cells only"))
    assert only_c[2] == kr.want_result(s.e, src, dst, np.ones(len(svc)), wev, evals=False)


@pytest.mark.parametrize("name", kr.SETS)
def test_shapes(name):
    """every shape of reach_cases.SHAPES: (1, 15), (1, 17) and (64, 33) end in a word whose pairs past
    n_dst are deferred and must count nothing"""
    s, _ = rc.set_case(name)
    for shape in rc.SHAPES:
        src, dst, svc, ev, ce = kr.shape_hists(s.spec.topology, *shape)
        wev, wce = kr.weighted(ev, ce)
        assert int(wce.sum()) == shape[0] * shape[1] * len(svc)
        for node in (True, False):
            got = kr.run_host(s.e, src, dst, svc, node=node)
            kr.same(got, wev, wce, (name, shape, node))
            assert got[2]["n_cells"] == int(wce.sum()) and got[2]["n_evals"] == int(wev.sum())


@pytest.mark.parametrize("name", ("uni", "uni-wide", "pair"))
def test_weights(name):
    """weights 0, 1, 65536 and random ones: the sum over the slices of weight x histogram"""
    s, _ = rc.set_case(name)
    src, dst, svc, ev, ce = kr.case_hists(s.spec.topology)
    w = kr.weights(len(svc))
    assert {0, 1, kr.MAX_WEIGHT} <= set(w.tolist()) and len(set(w.tolist())) > 6
    wev, wce = kr.weighted(ev, ce, w)
    for node in (True, False):
        got = kr.run_host(s.e, src, dst, svc, w, node=node)
        kr.same(got, wev, wce, (name, node))
        assert got[2] == kr.want_result(s.e, src, dst, w, wev)
    zero = kr.run_host(s.e, src, dst, svc, np.zeros(len(svc), np.uint32))
    assert not zero[0].any() and not zero[1].any() and zero[2]["n_cells"] == 0


@pytest.mark.parametrize("cells_knob", (0, 16, None))
@pytest.mark.parametrize("n_slots", (1, 16382, 16383, 100000))
def test_plan(n_slots, cells_knob):
    """no 32-bit cell can wrap between two flushes at the largest weight, the windows fit the LDS a
    workgroup may take, and they are whole, inside the index space and hold the tail first"""
    e = kr.bare_fixture()[0]
    knobs = {} if cells_knob is None else {"rules_hist_cells": cells_knob}
    cap = 16384 if cells_knob is None else cells_knob
    with e.tuning(**knobs):
        for evals, cells in ((True, True), (True, False), (False, True)):
            for n_tail in sorted({min(n_slots, t) for t in (2, 40, 9000)}):
                p = e.debug_reach_rules_plan(n_slots, n_tail, evals, cells, kr.MAX_WEIGHT)
                assert p["flush_words"] * 16 * 4 * kr.MAX_WEIGHT < 1 << 32
                assert p["flush_words"] >= p["block"] == 256          # a workgroup's round fits between two flushes
                assert p["lds_bytes"] == 4 * (p["evals_cells"] + p["cells_cells"]) <= min(4 * cap, 64 << 10)
                assert p["evals_cells"] <= (n_slots if evals else 0) and p["cells_cells"] <= (4 * n_slots if cells else 0)
                assert p["cells_cells"] % 4 == 0 and p["cells_base"] % 4 == 0
                assert p["evals_base"] < n_slots and p["cells_base"] < 4 * n_slots
                if evals and cells and 5 * n_slots <= cap:          # everything fits: nothing takes the global path
                    assert (p["evals_cells"], p["cells_cells"], p["evals_base"], p["cells_base"]) == (n_slots, 4 * n_slots, 0, 0)
                if evals and 0 < p["evals_cells"] < n_slots:        # a partial window starts in the tail
                    assert p["evals_base"] == (n_slots - min(n_tail, p["evals_cells"] // 2)) % n_slots
    # a lighter call flushes less often, never unsafely
    for w in (1, 2, 255, 65535):
        p = e.debug_reach_rules_plan(100, 2, True, True, w)
        assert p["flush_words"] * 64 * w < 1 << 32 <= (p["flush_words"] + 1) * 64 * w


@pytest.mark.parametrize("name", ("uni", "pair"))
def test_flushes_and_windows(name):
    """the twin walks workgroup by workgroup with the kernel's flushes: at weight 65536 a workgroup
    passes its flush bound several times (a wrapped cell would be PG_EFAULT, a lost one a mismatch),
    and under rules_hist_cells = 0 and 16 what the window does not hold goes to the arrays at once"""
    s, _ = rc.set_case(name)
    e = s.e
    src, dst, svc, ev, ce = kr.case_hists(s.spec.topology)
    w = np.full(len(svc), kr.MAX_WEIGHT, np.uint32)
    wev, wce = kr.weighted(ev, ce, w)
    n = e.num_counter_slots()
    p = e.debug_reach_rules_plan(n, 2, True, True, kr.MAX_WEIGHT)
    words = len(svc) * len(src) * ((len(dst) + 15) // 16)
    # each of the twin's two workgroups makes more rounds of 256 words than fit between two flushes
    assert words > (2 * (p["flush_words"] // p["block"]) + 1) * p["block"]
    full = kr.run_host(e, src, dst, svc, w)
    kr.same(full, wev, wce, (name, "default"))
    for knob in (0, 16):
        with e.tuning(rules_hist_cells=knob):
            assert e.debug_reach_rules_plan(n, 2, True, True, kr.MAX_WEIGHT)["lds_bytes"] == 4 * knob
            got = kr.run_host(e, src, dst, svc, w)
        kr.same(got, wev, wce, (name, knob))
        assert got[2] == full[2]


def test_dead_rule():
    """rule 1 copies rule 0: it decides nothing and is reported dead; rule 0 has hits"""
    e, world, src, dst = kr.dead_fixture()
    ev, ce = kr.slice_hists(world, src, dst, kr.DEAD_SERVICES)
    wev, wce = kr.weighted(ev, ce)
    base, n_rules, dflt = e.table_info(e.table_id("dup"))
    assert n_rules == 5 and wev[base] > 0 and wev[base + 1] == 0 and wev[base + 2] > 0   # (the oracle agrees)
    got = kr.run_host(e, src, dst, kr.DEAD_SERVICES)
    kr.same(got, wev, wce, "dead")
    assert got[0][base + 1] == 0 and got[0][base] > 0 and not got[1][base + 1].any()
    assert got[2]["n_dead_rules"] == kr.n_dead(e, wev) == 2 and got[2]["n_rule_slots"] == 5
    pods = ["ns/p%d" % k for k in range(4)]
    rep = e.rule_coverage(pods, pods, kr.DEAD_SERVICES, host=True)
    ev4, ce4 = kr.weighted(*kr.slice_hists(world, src[:4], dst[:4], kr.DEAD_SERVICES))
    assert rep == kr.report_of(e, world, ev4, ce4)
    assert rep["dead_rules"] == [("dup", 1), ("dup", 3)] and rep["acls"]["dup"][0][1] > 0 and rep["acls"]["dup"][-1][0] == -1


@pytest.mark.parametrize("protocol", (pc.TCP, pc.UDP))
def test_coverage_ports(protocol):
    """rule_coverage_ports(host=True) on 3 x 3 pods of the port-sweep fixture == the oracle over all
    65,536 dst ports of the nine pairs, in one call and split into calls of at most 7 services"""
    t = pc.topo("full")
    e, world = t.e, t.world
    pods = ["ns/p0", "ns/p1", "ns/p2"]
    ips = np.array(pc.POD_IPS[:3], np.uint32)
    s, d = np.repeat(np.repeat(ips, 3), 65536), np.repeat(np.tile(ips, 3), 65536)
    dp = np.tile(np.arange(65536, dtype=np.uint16), 9)
    n = len(s)
    act, slot, hist = world.conn(s, d, np.full(n, pc.SPORT, np.uint16), dp, np.full(n, protocol, np.uint8), threads=4, hist=True)
    n_slots = world.slot_unresolved + 1
    ce = np.bincount((slot.astype(np.int64) << 2) | act.astype(np.int64), minlength=4 * n_slots).reshape(n_slots, 4)
    want = kr.report_of(e, world, hist, ce)
    assert sum(sum(r[2]) for rows in want["acls"].values() for r in rows) + sum(want["no_acl"][1]) + sum(want["unresolved"][1]) == n
    k = len(e.port_intervals(protocol))
    assert k > 7
    assert e.rule_coverage_ports(pods, pods, protocol, host=True) == want
    assert e.rule_coverage_ports(pods, pods, protocol, host=True, max_services=7) == want


def test_einval_and_empty():
    """every PG_EINVAL with its word in pg_last_error, on the twin; empty sides clear the given arrays
    and leave the guards"""
    s, c = rc.set_case("uni")
    e = s.e
    n = e.num_counter_slots()
    ev, ce = kr.host_buffers(n)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    res = _capi.pg_reach_rules_result(7, 7, 7, 7, 7, 7)
    calls, keep = kr.einval_calls(e, c.src[:3], c.dst[:3], c.svc[:2], p(ev), p(ce))
    for what, word, spec, oe, oc, with_result in calls:
        code = lib.pg_debug_reach_rules_host(e.h, C.byref(spec) if spec is not None else None, oe, oc,
                                             C.byref(res) if with_result else None, 1)
        assert code == _capi.PG_EINVAL and word in lib.pg_last_error(e.h).decode(), (what, code, lib.pg_last_error(e.h))
    assert res.n_slots == 7 and (ev == kr.FILL).all() and (ce == kr.FILL).all()
    for ns, nd, nv in ((0, 3, 2), (3, 0, 2), (3, 3, 0)):
        ev, ce = kr.host_buffers(n)
        spec, k2 = D.rules_spec(c.src[:ns], c.dst[:nd], c.svc[:nv], None, n)
        res = _capi.pg_reach_rules_result(7, 7, 7, 7, 7, 7)
        assert lib.pg_debug_reach_rules_host(e.h, C.byref(spec), p(ev), p(ce), C.byref(res), 1) == 0
        assert not ev[:n].any() and not ce[:4 * n].any() and (ev[n:] == kr.FILL).all() and (ce[4 * n:] == kr.FILL).all()
        assert D.rules_result(res) == {"n_slots": n, "layout_gen": D.counter_layout_gen(e), "n_cells": 0, "n_evals": 0,
                                       "n_rule_slots": 0, "n_dead_rules": 0}
    del keep
