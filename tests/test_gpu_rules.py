"""Rule coverage on the device: pg_reach_rules against the oracle and, byte for byte, against the host
twin over the products of tests/rules_cases.py -- every node set and shape, pg_classify's counters over
the materialised tuples, the global-atomics path under rules_hist_cells, the flush bound at weight
65536, more words than one stride of the resident grid, a stream of its own over prefilled guarded
buffers, away from the hit counters, every PG_EINVAL, empty input and the wrappers.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import diff_cases as dc
import ports_cases as pc
import reach_cases as rc
import rules_cases as kr
from vpp_amd import _capi
from vpp_amd import device as D
from vpp_amd._capi import MODE_CONN, lib

pytestmark = pytest.mark.gpu


def run_dev(e, src, dst, svc, w=None, evals=True, cells=True, stream=None):
    """pg_reach_rules over prefilled outputs with guards -> (evals u64 [n_slots], cells u64 [n_slots, 4],
    result dict), None for a histogram that was not asked for"""
    st = stream or torch.cuda.current_stream()
    n = e.num_counter_slots()
    with torch.cuda.stream(st):
        ev = torch.full((n + kr.GUARD,), -1, dtype=torch.int64, device="cuda") if evals else None
        ce = torch.full((4 * n + kr.GUARD,), -1, dtype=torch.int64, device="cuda") if cells else None
    spec, keep = D.rules_spec(src, dst, svc, w, n)
    res = _capi.pg_reach_rules_result(7, 7, 7, 7, 7, 7)
    code = lib.pg_reach_rules(e.h, C.byref(spec), ev.data_ptr() if evals else None, ce.data_ptr() if cells else None,
                              C.byref(res), C.c_void_p(st.cuda_stream))
    assert code == 0, lib.pg_last_error(e.h)
    del keep
    # (the call has synchronised its stream: no wait here before the outputs are read)
    ev, ce = (None if t is None else t.cpu().numpy().view(np.uint64) for t in (ev, ce))
    assert ev is None or (ev[n:] == kr.FILL).all(), "guard behind out_evals"
    assert ce is None or (ce[4 * n:] == kr.FILL).all(), "guard behind out_cells"
    return None if ev is None else ev[:n], None if ce is None else ce[:4 * n].reshape(n, 4), D.rules_result(res)


def identical(a, b, what):
    for x, y in zip(a[:2], b[:2]):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), what
    assert a[2] == b[2], (what, a[2], b[2])


def classify_counts(e, src, dst, svc, counters=None):
    """pg_classify(PG_MODE_CONN) over the materialised tuples of the product, counting into a zeroed
    scratch array (or the given device pointer) -> that array as u64, or None"""
    ns, nd = len(src), len(dst)
    s, d = np.tile(np.repeat(src, nd), len(svc)), np.tile(np.tile(dst, ns), len(svc))
    col = lambda k, dt: np.repeat(np.array([x[k] & (0xFF if k == 0 else 0xFFFF) for x in svc], dt), ns * nd)
    t = D.TupleBatch.from_numpy(s, d, col(1, np.uint16), col(2, np.uint16), col(0, np.uint8))
    out = torch.empty(t.n, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(e.num_counter_slots(), dtype=torch.int64, device="cuda") if counters is None else None
    D.classify(e, MODE_CONN, -1, t, out, counters=scratch if counters is None else counters)
    torch.cuda.synchronize()
    return None if scratch is None else scratch.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("name", kr.SETS)
def test_equals_oracle_and_host(name):
    """37 x 53 with all services and every shape: the oracle, and the host twin byte for byte; on one set
    of each form also pg_classify's counters over the materialised tuples"""
    s, _ = rc.set_case(name)
    e = s.e
    src, dst, svc, ev, ce = kr.case_hists(s.spec.topology)
    wev, wce = kr.weighted(ev, ce)
    got = run_dev(e, src, dst, svc)
    kr.same(got, wev, wce, name)
    identical(got, kr.run_host(e, src, dst, svc), name)
    assert got[2] == kr.want_result(e, src, dst, np.ones(len(svc)), wev)
    if name in ("uni", "pair"):
        assert (classify_counts(e, src, dst, svc) == wev).all(), "pg_classify's counters over the tuples"
    for shape in rc.SHAPES:
        src, dst, svc, ev, ce = kr.shape_hists(s.spec.topology, *shape)
        got = run_dev(e, src, dst, svc)
        kr.same(got, *kr.weighted(ev, ce), (name, shape))
        identical(got, kr.run_host(e, src, dst, svc), (name, shape))


@pytest.mark.parametrize("name", ("uni-wide", "big-pair"))
def test_weights(name):
    s, _ = rc.set_case(name)
    src, dst, svc, ev, ce = kr.case_hists(s.spec.topology)
    w = kr.weights(len(svc))
    got = run_dev(s.e, src, dst, svc, w)
    kr.same(got, *kr.weighted(ev, ce, w), name)
    identical(got, kr.run_host(s.e, src, dst, svc, w), name)


@pytest.mark.parametrize("name", ("uni", "pair"))
def test_global_atomics_path(name):
    """rules_hist_cells 0 (global atomics only), 16 (a window of the tail and the first rules) and the
    default, with and without the wave aggregation: identical outputs"""
    s, _ = rc.set_case(name)
    e = s.e
    src, dst, svc, ev, ce = kr.case_hists(s.spec.topology)
    w = kr.weights(len(svc), seed=8)
    wev, wce = kr.weighted(ev, ce, w)
    full = run_dev(e, src, dst, svc, w)
    kr.same(full, wev, wce, (name, "default"))
    for knobs in ({"rules_hist_cells": 0}, {"rules_hist_cells": 16}, {"rules_wave_agg": 0}, {"rules_hist_cells": 16, "rules_wave_agg": 0}):
        with e.tuning(**knobs):
            for evals, cells in ((True, True), (True, False), (False, True)):
                got = run_dev(e, src, dst, svc, w, evals=evals, cells=cells)
                kr.same(got, wev, wce, (name, knobs, evals, cells))


def multiplicity_hists(world, ips, m_src, m_dst, svc):
    """the oracle's histograms of a product whose sides repeat the addresses `ips` m_src / m_dst times:
    the sum over the distinct pairs of their single-tuple histograms times the multiplicities"""
    n_slots = world.slot_unresolved + 1
    ev, ce = np.zeros(n_slots, np.uint64), np.zeros((n_slots, 4), np.uint64)
    for a, ma in zip(ips, m_src):
        for b, mb in zip(ips, m_dst):
            e1, c1 = kr.weighted(*kr.slice_hists(world, np.array([a], np.uint32), np.array([b], np.uint32), svc))
            ev += e1 * np.uint64(ma * mb)
            ce += c1 * np.uint64(ma * mb)
    return ev, ce


def test_flush_bound_on_device():
    """pods without any ACL: every evaluation lands on the "no ACL" slot, one service of weight 65536, one
    workgroup per CU and enough words that every workgroup passes its flush bound: a cell that wrapped
    would lose 2^32"""
    e, world, pods = kr.bare_fixture()
    svc, w = [(pc.TCP, 40000, 80)], np.array([kr.MAX_WEIGHT], np.uint32)
    ips = np.array(pods + [pc.OTHER[0]], np.uint32)
    with e.tuning(blocks_per_cu=1):
        p = e.debug_reach_rules_plan(e.num_counter_slots(), 2, True, True, kr.MAX_WEIGHT, resident=True)
        rounds = p["flush_words"] // p["block"] + 1            # rounds of a workgroup that take it past the bound
        need = (rounds + 1) * p["resident"] * p["block"]       # words: every workgroup makes more than `rounds`
        n = 16
        while n * ((n + 15) // 16) < need:
            n += 16
        n += 3
        assert 1000 < n < 8192, (n, p)
        side = ips[np.arange(n) % len(ips)]
        mult = np.bincount(np.arange(n) % len(ips), minlength=len(ips))
        ev1, ce1 = multiplicity_hists(world, ips, mult, mult, svc)
        assert ev1[world.slot_noacl] > (1 << 32) // kr.MAX_WEIGHT and not ev1[:world.slot_noacl].any()
        got = run_dev(e, side, side, svc, w)
    kr.same(got, ev1 * np.uint64(kr.MAX_WEIGHT), ce1 * np.uint64(kr.MAX_WEIGHT), "flush bound")
    assert got[2]["n_cells"] == n * n * kr.MAX_WEIGHT


@pytest.mark.parametrize("name", ("uni", "pair"))
def test_more_words_than_one_stride(name):
    """blocks_per_cu = 1 and sides tiled 30 x 8: the resident grid strides over the words several times;
    the default launch and the oracle (every pair of the 37 x 53 case 240 times)"""
    s, _ = rc.set_case(name)
    e = s.e
    src, dst, svc, ev, ce = kr.case_hists(s.spec.topology)
    wev, wce = kr.weighted(ev, ce)
    big_src, big_dst = np.tile(src, 30), np.tile(dst, 8)
    with e.tuning(blocks_per_cu=1):
        p = e.debug_reach_rules_plan(e.num_counter_slots(), 2, True, True, 1, resident=True)
        words = len(svc) * len(big_src) * ((len(big_dst) + 15) // 16)
        assert words > 2 * p["resident"] * p["block"] and len(big_dst) % 16
        one = run_dev(e, big_src, big_dst, svc)
    kr.same(one, wev * np.uint64(240), wce * np.uint64(240), (name, "blocks_per_cu = 1"))
    identical(one, run_dev(e, big_src, big_dst, svc), (name, "default launch"))


def test_stream_and_prefill():
    """a non-default stream over prefilled outputs (run_dev holds the guards): evals only, cells only, both"""
    s, _ = rc.set_case("uni-grouped")
    src, dst, svc, ev, ce = kr.case_hists(s.spec.topology)
    wev, wce = kr.weighted(ev, ce)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for evals, cells in ((True, False), (False, True), (True, True)):
        got = run_dev(s.e, src, dst, svc, evals=evals, cells=cells, stream=st)
        assert (got[0] is not None) == evals and (got[1] is not None) == cells
        kr.same(got, wev, wce, (evals, cells))
        assert got[2] == kr.want_result(s.e, src, dst, np.ones(len(svc)), wev, evals=evals)


def test_counters_untouched():
    """the counters and their snapshots are bit-identical before and after a call on that context, and
    out_evals is what a classify of the product's tuples leaves in them"""
    s, _ = rc.set_case("uni")
    e = s.e
    src, dst, svc, ev, ce = kr.case_hists(s.spec.topology)
    D.reset_counters(e)
    classify_counts(e, src, dst, svc, counters=D.counters_device_ptr(e))
    before = D.read_counters(e)
    snap = D.counters_snapshot(e)
    assert before.sum() > 0
    got = run_dev(e, src, dst, svc)
    assert (D.counters_snapshot(e) == snap).all()
    assert (D.read_counters(e) == before).all()
    assert (got[0] == before).all()
    D.reset_counters(e)


def test_einval_and_empty_input():
    s, c = rc.set_case("uni")
    e = s.e
    n = e.num_counter_slots()
    ev = torch.full((n + kr.GUARD,), -1, dtype=torch.int64, device="cuda")
    ce = torch.full((4 * n + kr.GUARD,), -1, dtype=torch.int64, device="cuda")
    res = _capi.pg_reach_rules_result(7, 7, 7, 7, 7, 7)
    calls, keep = kr.einval_calls(e, c.src[:3], c.dst[:3], c.svc[:2], ev.data_ptr(), ce.data_ptr())
    for what, word, spec, oe, oc, with_result in calls:
        code = lib.pg_reach_rules(e.h, C.byref(spec) if spec is not None else None, oe, oc,
                                  C.byref(res) if with_result else None, None)
        assert code == _capi.PG_EINVAL and word in lib.pg_last_error(e.h).decode(), (what, code, lib.pg_last_error(e.h))
    torch.cuda.synchronize()
    assert res.n_slots == 7 and (ev.cpu().numpy() == -1).all() and (ce.cpu().numpy() == -1).all()
    del keep
    # a stale n_slots: an ACL installed between sizing and calling (an engine of this test's own)
    own = pc.fixture("k16")[0]
    stale = own.num_counter_slots()
    own.ApplyTxn(False, [(dc.KEY + "late", {"name": "late", "ingress": ["tap3"], "egress": [], "rules": [
        {"action": 1, "src": "", "dst": ""}]})])
    spec, keep = D.rules_spec(pc.POD_IPS, pc.POD_IPS, c.svc[:2], None, stale)
    code = lib.pg_reach_rules(own.h, C.byref(spec), ev.data_ptr(), None, C.byref(res), None)
    msg = lib.pg_last_error(own.h).decode()
    assert code == _capi.PG_EINVAL and "changed since" in msg and str(stale) in msg and str(own.num_counter_slots()) in msg
    assert own.num_counter_slots() > stale
    del keep
    # empty sides: the given arrays cleared, the guards intact, the result zeroed but for n_slots and the generation
    for ns, nd, nv in ((0, 3, 2), (3, 0, 2), (3, 3, 0)):
        for evals, cells in ((True, True), (True, False), (False, True)):
            got = run_dev(e, c.src[:ns], c.dst[:nd], c.svc[:nv], evals=evals, cells=cells)
            assert all(x is None or not x.any() for x in got[:2])
            assert got[2] == {"n_slots": n, "layout_gen": D.counter_layout_gen(e), "n_cells": 0, "n_evals": 0,
                              "n_rule_slots": 0, "n_dead_rules": 0}


def test_wrappers():
    """Engine.rule_coverage on the device == on the host twin == the oracle, on both engines of the
    fixture change; Engine.rule_coverage_ports on the device == the histogram of pg_reach_ports'
    out_words times the interval lengths"""
    c = dc.matrix_change()
    ips = np.array(c.pod_ips, np.uint32)
    for e, world in ((c.e0, c.w0), (c.e1, c.w1)):
        dev = e.rule_coverage(dc.PODS, dc.PODS, dc.SERVICES)
        assert dev == e.rule_coverage(dc.PODS, dc.PODS, dc.SERVICES, host=True)
        assert dev == kr.report_of(e, world, *kr.weighted(*kr.slice_hists(world, ips, ips, dc.SERVICES)))
        assert dev["dead_rules"] and any(r[1] for rows in dev["acls"].values() for r in rows)
    e = c.e0
    n = e.num_counter_slots()
    for protocol in (pc.TCP, pc.UDP):
        lo, _, words = D.reach_ports(e, ips, ips, protocol, pc.SPORT, words=True)
        torch.cuda.synchronize()
        w = words.cpu().numpy().view(np.uint32).astype(np.int64)
        idx = ((w & 0x3FFFFFFF) << 2) | (w >> 30)
        cells = sum(int(ln) * np.bincount(idx[:, :, k].ravel(), minlength=4 * n) for k, ln in enumerate(pc.lengths(lo)))
        cells = cells.reshape(n, 4)
        assert int(cells.sum()) == len(ips) ** 2 * 65536
        rep = e.rule_coverage_ports(dc.PODS, dc.PODS, protocol)
        host = e.rule_coverage_ports(dc.PODS, dc.PODS, protocol, host=True, max_services=5)
        assert rep == host == e.rule_coverage_ports(dc.PODS, dc.PODS, protocol, max_services=5)
        base_of = {name: e.table_info(e.table_id(name)) for name in rep["acls"]}
        for name, rows in rep["acls"].items():
            base, n_rules, dflt = base_of[name]
            assert [r[2] for r in rows] == [cells[base + k].tolist() for k in range(n_rules)] + [cells[dflt].tolist()], name
        assert rep["no_acl"][1] == cells[n - 2].tolist() and rep["unresolved"][1] == cells[n - 1].tolist()
