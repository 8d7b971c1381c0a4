"""The reachability zones on the device: pg_reach_zones against numpy and, byte for byte, against the host
twin over the closures of tests/zones_cases.py: the small shapes, the shapes around the launch plan's
transpose tile and label work item, runs of several work items per workgroup, more zones than the numbering
counts in LDS, a matrix past 2^13 rows, an input that is not 16-B aligned, a stream of its own over prefilled
buffers, matrix -> closure -> zones -> groups -> diff chained on the device from two engines, the wrappers,
and away from the counters.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import closure_cases as cc
import diff_cases as dc
import groups_cases as gc
import zones_cases as zc
from vpp_amd import _capi
from vpp_amd import device as D
from vpp_amd import renderer as R
from vpp_amd._capi import MODE_CONN, lib

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


def dev(words, offset=0):
    """packed words -> an int32 device tensor of the same shape; offset: words the data starts behind a
    fresh allocation (1: not 16-B aligned)"""
    w = np.ascontiguousarray(words, np.uint32)
    t = torch.empty(w.size + offset, dtype=torch.int32, device="cuda")
    t[offset:] = torch.from_numpy(w.view(np.int32).ravel()).cuda()
    assert t[offset:].data_ptr() % 16 == (4 * offset) % 16
    return t[offset:].reshape(w.shape)


def run_dev(e, mt, n, reps=True, sizes=True, counts=True, dag=True, stream=None):
    """pg_reach_zones over prefilled outputs with guards; zc.run_host's contract on a device tensor"""
    st = stream or torch.cuda.current_stream()
    flags = zc.given(reps, sizes, counts, dag)
    with torch.cuda.stream(st):
        bufs = [torch.full((k + zc.GUARD,), -1, dtype=torch.int32, device="cuda") for k in zc.sizes(n)]
    res = _capi.pg_reach_zones_result(zc.FILL, zc.FILL, zc.FILL, zc.FILL, zc.FILL)
    spec = zc.spec_of(mt.data_ptr() if mt.numel() else None, n)
    code = lib.pg_reach_zones(e.h, C.byref(spec), *[b.data_ptr() if f else None for b, f in zip(bufs, flags)], C.byref(res),
                              C.c_void_p(st.cuda_stream))
    assert code == 0, lib.pg_last_error(e.h)
    # (the call has synchronised its stream: no wait here before the outputs are read)
    return zc.finish([b.cpu().numpy().view(np.uint32) for b in bufs], n, flags, res)


def run(*args, **kw):
    return run_dev(engine(), *args, **kw)


def same_as_host(e, s, mt, **kw):
    """numpy, and the host twin byte for byte"""
    d, h = run_dev(e, mt, s.n, **kw), zc.run_host(e, s.words, s.n, **kw)
    zc.same(d, s.want, (s.family, s.n))
    zc.identical(d, h, (s.family, s.n))
    return d


@pytest.mark.parametrize("family", zc.FAMILIES)
def test_synthetic(family):
    """the small shapes, with blocks_per_cu unset and = 1"""
    e = engine()
    for n in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257):
        s = zc.synthetic(n, family)
        zc.assert_inputs(s)
        mt = dev(s.words)
        same_as_host(e, s, mt)
        with e.tuning(blocks_per_cu=1):
            zc.check(run, s, words=mt, variants=n in (17, 129))


@pytest.mark.parametrize("family", ("rings", "raw"))
def test_tile_edges(family):
    """one below, on and one above a transpose tile's row edge and column edge, a label work item's rows and
    the 64 bit-words of a label pass, taken from the plan"""
    e = engine()
    p = e.debug_reach_zones_plan(1 << 15)
    edges = {p["tile_rows"], 2 * p["tile_rows"], p["tile_cols"], p["label_rows"], 64 * 32}
    for n in sorted({max(1, k + d) for k in edges for d in (-1, 0, 1)}):
        s = zc.synthetic(n, family, seed=1)
        mt = dev(s.words)
        same_as_host(e, s, mt)
        with e.tuning(blocks_per_cu=1):
            zc.check(run, s, words=mt, variants=False)


@pytest.mark.parametrize("family", ("rings", "raw", "empty", "chain"))
def test_past_a_column_tile(family):
    """2^12 + 4 end points: past four whole column tiles and 32 row tiles, the last of each with 4 cells; under
    blocks_per_cu = 1 a label workgroup walks several rows; empty and chain have more zones (one per end
    point) than the numbering counts in LDS"""
    e = engine()
    n = (1 << 12) + 4
    s = zc.synthetic(n, family, seed=4)
    mt = dev(s.words)
    same_as_host(e, s, mt)
    with e.tuning(blocks_per_cu=1):
        zc.check(run, s, words=mt, variants=False)


@pytest.mark.parametrize("n", (4096, 4097))
def test_lds_zone_count_threshold(n):
    """4096 zones are counted in LDS, 4097 in scratch"""
    s = zc.synthetic(n, "empty")
    assert s.want.result["n_zones"] == n
    zc.check(run, s, words=dev(s.words), variants=False)


def test_large():
    """2^13 + 1 end points: 65 x 9 transpose tiles, more than the workgroups of blocks_per_cu = 1 -- every
    workgroup of the bits kernel walks a run of tiles -- and rows of 257 bit-words: five label passes"""
    e = engine()
    s = zc.synthetic((1 << 13) + 1, "rings", seed=5)
    mt = dev(s.words)
    zc.check(run, s, words=mt, variants=False)
    with e.tuning(blocks_per_cu=1):
        zc.check(run, s, words=mt, variants=False)


def test_unaligned_input():
    """the input one word behind a 16-B boundary"""
    for n, family in ((17, "corner"), (100, "rings"), (1025, "raw")):
        s = zc.synthetic(n, family, seed=6)
        zc.check(run, s, words=dev(s.words, offset=1))


def test_stream_and_prefill():
    """a non-default stream over prefilled outputs (run_dev holds the guards), every variant"""
    s = zc.synthetic(1000, "corner", seed=7)
    mt = dev(s.words)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    zc.check(lambda *args, **kw: run(*args, stream=st, **kw), s, words=mt)


def test_garbage_in_padding():
    for family in ("rings", "raw", "full"):
        s = zc.synthetic(100, family, seed=8)
        junk = dc.garbage(s.words, 100)
        assert (junk[:, -1] >> (2 * (100 & 15))).any()
        zc.identical(zc.check(run, s, words=dev(junk), variants=False), zc.run_host(engine(), s.words, 100), "garbage")


def test_device_wrapper():
    """device.reach_zones against numpy"""
    e = engine()
    s = zc.synthetic(257, "rings", seed=9)
    w = s.want
    u = lambda t: t.cpu().numpy().view(np.uint32)
    zone, rep, size, out, by, dag, res = D.reach_zones(e, dev(s.words), 257, reps=True, sizes=True, counts=True, dag=True)
    assert zone.dtype == torch.int32 and (u(zone) == w.zone).all() and (u(rep) == w.rep).all() and (u(size) == w.size).all()
    assert (u(out) == w.reaches).all() and (u(by) == w.reached_by).all() and (u(dag) == w.dag).all() and res == w.result
    zone, rep, size, out, by, dag, res = D.reach_zones(e, dev(s.words), 257)
    assert (u(zone) == w.zone).all() and rep is None and size is None and out is None and by is None and dag is None
    assert res == w.result
    zone, rep, _, _, _, dag, res = D.reach_zones(e, dev(s.words)[:0].contiguous(), 0, dag=True)
    assert zone.numel() == 0 and rep.numel() == 0 and dag.numel() == 0 and res["n_zones"] == 0


# ---- matrix -> closure -> zones (-> groups -> diff) on the device, inputs from two engines -------
def test_fixture_change_chained():
    """D.reach_matrix -> D.reach_closure -> D.reach_zones on both fixture engines against a Python SCC of the
    oracle's one-hop graph, under all services and under service 0 alone; then the zones of the first
    engine's closure are the groups under which both closures are summed, and the diff of the two summaries
    lists the zone pairs the edit connected or cut"""
    c = cc.fixture_change()
    n = len(c.dst)
    ctx = engine()   # (the context only names the device: an engine without tables)
    mts = [D.reach_matrix(e, c.dst, c.dst, dc.SERVICES) for e in (c.e0, c.e1)]
    sel = np.zeros(len(dc.SERVICES), np.uint8)
    sel[0] = 1
    closures, wants = [], []
    for mt, codes in zip(mts, c.closure_codes):
        for select, sub in ((None, codes), (sel, codes[:1])):
            packed, _, counts, _ = D.reach_closure(ctx, mt, n, select, counts=True)
            comp, want = zc.graph_want(sub)
            got = run_dev(ctx, packed, n)
            zc.same(got, want, "fixture")
            assert (got.rep[got.zone] == comp).all()
            assert (got.reaches == counts.cpu().numpy().view(np.uint32)[got.rep]).all()
        closures.append(packed)   # (service 0 alone)
        wants.append(want)
    assert wants[0].result != wants[1].result, "the edit moved no zone"
    zone, nz = wants[0].zone, wants[0].result["n_zones"]
    summaries, statuses = [], []
    for packed, codes in zip(closures, c.closure_codes):
        reach = zc.close((codes[:1] == zc.ALLOW).any(axis=0))
        wc, ws = gc.expected(np.where(reach, np.uint8(2), np.uint8(0))[None], zone, zone, nz, nz)
        counts, status = D.reach_groups(ctx, packed.reshape(1, n, -1), n, n, zone, zone, nz, nz, packed=True)
        assert (counts.cpu().numpy().view(np.uint64) == wc).all()
        summaries.append(status)
        statuses.append(ws)
    # over its own closure every zone pair is uniform: all of its cells reachable, or none
    assert not (statuses[0] == _capi.GROUPS_SOME).any() and (statuses[1] == _capi.GROUPS_SOME).any()
    x = dc.Expected(statuses[0].reshape(nz, nz), statuses[1].reshape(nz, nz), dc.ALL)
    assert x.n > 0, "the edit moved no zone pair"
    k, changes, trans, _ = D.reach_diff(ctx, summaries[0], summaries[1], nz)
    assert k == x.n and (changes.cpu().numpy().view(np.uint32) == x.entries).all() and (trans == x.trans).all()


def test_wrappers():
    """Engine.reachability_zones and reachability_zones_diff on the device give what they give on the host
    twins, and what the oracle says; one pod is listed twice"""
    c = dc.matrix_change()
    ip = dict(zip(dc.PODS, c.pod_ips))
    ips = np.array([ip[p] for p in zc.PODS], np.uint32)
    for svc in (dc.SERVICES, dc.SERVICES[:1]):
        for e, w in zip((c.e0, c.e1), (c.w0, c.w1)):
            want = zc.wrapper_want(cc.oracle_codes(w, ips, svc), zc.PODS)
            got, host = e.reachability_zones(zc.PODS, svc), e.reachability_zones(zc.PODS, svc, host=True)
            for g, h, x in zip(got, host, want):
                assert (g == h if isinstance(g, list) else (g == h).all()) and (g == x if isinstance(g, list) else (g == x).all())
        moved = c.e1.reachability_zones_diff(c.e0, zc.PODS, svc)
        assert moved == c.e1.reachability_zones_diff(c.e0, zc.PODS, svc, host=True) and bool(moved) == (len(svc) == 1)
    for extra in ((), ((11, 0),), ((3, 1), (9, 7))):
        k = cc.chain(extra)
        zones, out, by, graph = k.e.reachability_zones(cc.CHAIN_PODS, cc.CHAIN_SERVICES)
        wz, wo, wb, wg = zc.wrapper_want(k.codes, cc.CHAIN_PODS)
        assert zones == wz and (out == wo).all() and (by == wb).all() and (graph == wg).all()


def test_counters_untouched():
    """the counters and their snapshots are bit-identical before and after a call on that context"""
    import node_matrix as nm
    s = nm.node_set("uni")
    e = s.e
    D.reset_counters(e)
    src, dst, sport, dport, proto = (x[:4099] for x in s.tup)
    t = D.TupleBatch.from_numpy(src, dst, sport, dport, proto)
    out = torch.empty(t.n, dtype=torch.int32, device="cuda")
    D.classify(e, MODE_CONN, -1, t, out, counters=D.counters_device_ptr(e))
    torch.cuda.synchronize()
    before = D.read_counters(e)
    snap = D.counters_snapshot(e)
    assert before.sum() > 0
    g = zc.synthetic(257, "rings", seed=10)
    zc.same(run_dev(e, dev(g.words), 257), g.want, "counters")
    assert (D.counters_snapshot(e) == snap).all()
    assert (D.read_counters(e) == before).all()
    D.reset_counters(e)


def test_einval_and_empty_input():
    e = engine()
    w = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    res = _capi.pg_reach_zones_result(7, 7, 7, 7, 7)
    for what, words, spec, outs, with_result in zc.bad_calls(w.data_ptr(), out.data_ptr()):
        code = lib.pg_reach_zones(e.h, C.byref(spec) if spec is not None else None, *outs,
                                  C.byref(res) if with_result else None, None)
        assert code == _capi.PG_EINVAL and words in lib.pg_last_error(e.h).decode(), (what, code)
    assert (res.n_zones, res.n_cyclic, res.n_multi, res.largest, res.n_broken) == (7, 7, 7, 7, 7)
    assert lib.pg_reach_zones(e.h, C.byref(zc.spec_of(None, 0)), *([out.data_ptr()] * 6), C.byref(res), None) == 0
    assert (res.n_zones, res.n_cyclic, res.n_multi, res.largest, res.n_broken) == (0, 0, 0, 0, 0)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all()
