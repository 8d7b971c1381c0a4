"""The reachability cost on the device: pg_reach_cost against the references of tests/cost_cases.py and, byte
for byte, against the host twin over the same graphs, with blocks_per_cu unset and 1 and with
"cost_lds_bytes" at its default, at a value that drops only the weights from LDS, and at 0 (the row in
global memory); a random graph of 8193 end points and 64 sources against scipy; unit weights chained on the
device with the closure and the paths; layers with written-down answers at the first sizes whose LDS
passes 48 KiB and 64 KiB and at 2^15 end points; an input that is not 16-B aligned, a stream of its own over
prefilled buffers, every subset of the outputs, the wrapper against the oracle, the arguments, and away
from the counters.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import closure_cases as cc
import cost_cases as co
from vpp_amd import _capi
from vpp_amd import device as D
from vpp_amd import renderer as R
from vpp_amd._capi import MODE_CONN, lib

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


@functools.lru_cache(maxsize=None)
def case(n, family):
    return co.Case(n, family)


def dev(words, offset=0):
    """packed words -> an int32 device tensor of the same shape; offset: words the data starts behind a
    fresh allocation (1: not 16-B aligned)"""
    w = np.ascontiguousarray(words, np.uint32)
    t = torch.empty(w.size + offset, dtype=torch.int32, device="cuda")
    t[offset:] = torch.from_numpy(w.view(np.int32).ravel()).cuda()
    assert t[offset:].data_ptr() % 16 == (4 * offset) % 16
    return t[offset:].reshape(w.shape)


def signed(fill, bits):
    return fill - (1 << bits) if fill >> (bits - 1) else fill


def run_dev(e, mt, n, src, w, max_cost=0, select=None, cost=True, pred=True, len=True, via=True, stream=None):
    """pg_reach_cost over prefilled outputs with guards; co.run_host's contract on a device tensor"""
    n_svc = mt.numel() // (n * cc.row_words(n))
    k = int(np.size(src))
    given = (cost, pred, len, via)
    st = stream or torch.cuda.current_stream()
    with torch.cuda.stream(st):
        bufs = [torch.full((size + co.GUARD,), signed(fill, bits), dtype=dt, device="cuda")
                for size, fill, bits, dt in zip((k * n, k * n, k * n, n), co.FILLS, (32, 16, 16, 32),
                                                (torch.int32, torch.int16, torch.int16, torch.int32))]
    st.synchronize()
    spec, keep = co.spec_of(mt.data_ptr(), n, n_svc, src, w, max_cost, select)
    res = _capi.pg_reach_cost_result(77, 77, 77, 77)
    code = lib.pg_reach_cost(e.h, C.byref(spec), *[b.data_ptr() if on else None for b, on in zip(bufs, given)], C.byref(res),
                             C.c_void_p(st.cuda_stream))
    assert code == 0, lib.pg_last_error(e.h)
    del keep
    # (the call has synchronised its stream: no wait here before the outputs are read)
    host = [b.cpu().numpy().view(dt) for b, dt in zip(bufs, (np.uint32, np.uint16, np.uint16, np.uint32))]
    return co.finish(k, n, host, res, given)


def equal_runs(h, d, what):
    """a host twin's and a device's return value, byte for byte"""
    assert h[4] == d[4], (what, h[4], d[4])
    for x, y in zip(h[:4], d[:4]):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), what


def both(e, mt):
    """a `run` for co.check over the device tensor of the words it is given: the device's answer, held byte for
    byte to the host twin's"""
    def go(words, *args, **kw):
        d = run_dev(e, mt, *args, **kw)
        equal_runs(co.run_host(e, words, *args, **kw), d, (args, kw))
        return d
    return go


def only_dev(e, mt):
    return lambda words, *args, **kw: run_dev(e, mt, *args, **kw)


def weights_only_dropped(e, n):
    """a "cost_lds_bytes" under which the plan of n end points keeps the row in LDS and not the weights"""
    with e.tuning(cost_lds_bytes=0):
        fixed = e.debug_reach_cost_plan(n)["lds_bytes"]
    budget = e.debug_reach_cost_plan(n)["lds_bytes"] - fixed - 1   # (one byte short of the row and the weights)
    with e.tuning(cost_lds_bytes=budget):
        p = e.debug_reach_cost_plan(n)
        assert (p["row_in_lds"], p["weights_in_lds"]) == (1, 0), (n, p)
    return budget


@pytest.mark.parametrize("family", co.FAMILIES)
def test_families(family):
    e = engine()
    for n in co.SIZES:
        s = case(n, family)
        mt = dev(s.words)
        assert e.debug_reach_cost_plan(n)["weights_in_lds"] == 1
        full = co.check(both(e, mt), s.words, s, variants=n <= 65)
        for knobs in ({"blocks_per_cu": 1}, {"cost_lds_bytes": weights_only_dropped(e, n)}, {"cost_lds_bytes": 0},
                      {"cost_lds_bytes": 0, "blocks_per_cu": 1}):
            with e.tuning(**knobs):
                equal_runs(full, co.check(only_dev(e, mt), s.words, s, variants=False), (n, family, knobs))


def test_small_graphs():
    """the device against the definition on all graphs of 3 end points as one disjoint union, and on random ones"""
    e = engine()
    a, w = co.all_graphs(3)
    cost, pred, ln, via = co.brute_all(a, w)
    G, n = len(a), 3
    words = co.union_words(a)
    for knobs in ({}, {"cost_lds_bytes": 0}):
        with e.tuning(**knobs):
            got = run_dev(e, dev(words), G * n, np.arange(G * n), w.ravel())
        gi = np.arange(G)[:, None, None]
        at = (gi * n + np.arange(n)[None, :, None], gi * n + np.arange(n)[None, None, :])
        want_pred = np.where(pred == co.NO_PRED, co.NO_PRED, pred + (np.arange(G) * n)[:, None, None])
        assert (got[0][at] == cost).all() and (got[1][at] == want_pred).all() and (got[2][at] == ln).all(), knobs
        assert (got[3].reshape(G, n) == via).all(), knobs
        assert int((got[0] != co.NONE).sum()) == int((cost != co.NONE).sum())
    for a, w in list(co.small_cases())[::3]:
        n = a.shape[0]
        words = co.pack(a, 2, seed=n)[1]
        d = run_dev(e, dev(words), n, np.arange(n), w)
        co.same(d, co.reference(a, w, range(n)).at(), (a.astype(int).tolist(), w.tolist()))
        equal_runs(co.run_host(e, words, n, np.arange(n), w), d, n)


def test_chain_300():
    """299 rounds inside one launch"""
    e = engine()
    s = case(300, "chain")
    mt = dev(s.words)
    for knobs in ({}, {"cost_lds_bytes": 0}):
        with e.tuning(**knobs):
            cost, pred, ln, via, res = run_dev(e, mt, 300, [0], s.w)
        assert res == {"n_reached": 299, "n_via": 299 * 298 // 2, "max_cost": int(s.w[1:].sum()), "longest": 299}, (knobs, res)
        assert (pred[0, 1:] == np.arange(299)).all() and (via[1:] == 298 - np.arange(299)).all() and via[0] == 0


# ---- one random graph against scipy ------------------------------------------------------------------
def test_random_graph():
    """random4 at 8193 end points, 64 sources, weights 1..9. The graph is closure_cases.LargeMedium -- the same
    4 random edges per end point as cost_cases' random4 -- because it packs its words without the n_svc x n x n
    codes that cost_cases.pack would take at this size (200 MB)"""
    e = engine()
    n = 8193
    s = cc.LargeMedium(n, seed=cc.LARGE_SEED)
    a = s.edge_matrix()
    g = np.random.default_rng(6)
    w = g.integers(1, 10, n).astype(np.uint16)
    src = g.integers(0, n, 64)
    src[5] = src[40]   # (a duplicate)
    x = co.by_scipy(a, w, src)
    mt = dev(s.words)
    got = run_dev(e, mt, n, src, w)
    co.same(got, x.at(), "random 8193")
    b = int(np.median(x.cost[x.cost != co.NONE]))
    co.same(run_dev(e, mt, n, src, w, b, pred=False), x.at(b), "random 8193, bounded")
    with e.tuning(cost_lds_bytes=0):
        equal_runs(got, run_dev(e, mt, n, src, w), "random 8193, the row in global memory")


# ---- unit weights: matrix -> closure -> paths and matrix -> cost on the device ---------------------------
@pytest.mark.parametrize("family,n", (("medium", 129), ("ring", 33), ("two-cliques", 65)))
def test_unit_weights_chained(family, n):
    e = engine()
    s = cc.synthetic(n, family)
    mt = dev(s.words)
    _, hops, _, _ = D.reach_closure(e, mt, n, hops=True)
    src, dst = (x.ravel().astype(np.uint32) for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    lens, nodes, pvia, pres = D.reach_paths(e, hops, n, src, dst, max_len=n, nodes=True, via=True)
    cost, pred, ln, via, res = D.reach_cost(e, mt, n, 3, np.arange(n), np.ones(n, np.uint16), pred=True, len=True, via=True)
    hops = hops.cpu().numpy().view(np.uint16).reshape(n, n)
    cost, pred, ln = cost.cpu().numpy().view(np.uint32), pred.cpu().numpy().view(np.uint16), ln.cpu().numpy().view(np.uint16)
    assert (np.where(cost == co.NONE, 0, cost) == hops).all() and (ln == hops).all()
    lens, nodes = lens.cpu().numpy().view(np.uint16).astype(np.int64), nodes.cpu().numpy().view(np.uint16).reshape(n * n, n + 1)
    before = np.where(lens > 0, nodes[np.arange(n * n), np.maximum(lens, 1) - 1], co.NO_PRED)
    assert (before.reshape(n, n) == pred).all()
    assert (pvia.cpu().numpy().view(np.uint32) == via.cpu().numpy().view(np.uint32)).all()
    assert res["n_via"] == pres["n_via"] and res["longest"] == pres["longest"] and res["n_reached"] == pres["n_found"]


# ---- layers with written-down answers, sizes read from the plan ----------------------------------------
def check_layers(e, n):
    widths, weights, words, src = co.large_layers(n)
    mt = dev(words)
    got = co.check_large_layers(lambda _w, *args: run_dev(e, mt, *args), n, (widths, weights, words, src))
    with e.tuning(blocks_per_cu=1):
        equal_runs(got, run_dev(e, mt, n, src, np.repeat(np.array(weights, np.uint16), widths)), n)
    return got


@pytest.mark.parametrize("kib", (48, 64))
def test_layers_where_the_lds_passes(kib):
    """the first n whose workgroup takes more than 48 KiB (the opt-in for large dynamic LDS) and 64 KiB"""
    e = engine()
    n = co.first_n(e.debug_reach_cost_plan, lambda p: p["lds_bytes"] > kib << 10, lo=400)
    assert e.debug_reach_cost_plan(n - 1)["lds_bytes"] <= kib << 10 < e.debug_reach_cost_plan(n)["lds_bytes"]
    check_layers(e, n)


@pytest.mark.parametrize("kib", (48, 64))
def test_layers_where_the_row_alone_passes(kib):
    """the first n whose LDS row alone passes 48 KiB and 64 KiB, with the weights beside it and without"""
    e = engine()
    n = (kib << 10) // 4 + 1
    with e.tuning(cost_lds_bytes=4 * (n - 1)):
        assert e.debug_reach_cost_plan(n - 1)["row_in_lds"] == 1 and e.debug_reach_cost_plan(n)["row_in_lds"] == 0
    got = check_layers(e, n)
    with e.tuning(cost_lds_bytes=weights_only_dropped(e, n)):
        assert e.debug_reach_cost_plan(n)["lds_bytes"] > kib << 10
        equal_runs(got, check_layers(e, n), n)


def test_layers_at_most_end_points():
    """2^15 end points: the row takes 128 KiB of the LDS, the weights are read through L2"""
    e = engine()
    n = 1 << 15
    p = e.debug_reach_cost_plan(n)
    assert (p["lane_words"], p["row_in_lds"], p["weights_in_lds"]) == (4, 1, 0) and p["lds_bytes"] > 128 << 10, p
    check_layers(e, n)


# ---- the launch's surroundings -----------------------------------------------------------------------
def test_unaligned_input():
    """the input one word behind a 16-B boundary"""
    e = engine()
    for n, family in ((33, "random4"), (129, "islands"), (300, "detour")):
        s = case(n, family)
        co.same(run_dev(e, dev(s.words, offset=1), n, s.src, s.w), co.reference(s.a, s.w, s.src).at(), (n, family))


def test_stream_and_prefill():
    """a non-default stream over prefilled outputs (run_dev holds the guards)"""
    e = engine()
    s = case(300, "random4")
    mt = dev(s.words)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    co.check(lambda _w, *args, **kw: run_dev(e, mt, *args, stream=st, **kw), s.words, s, variants=False)


def test_every_subset_of_the_outputs():
    e = engine()
    s = case(129, "random4")
    mt = dev(s.words)
    x = co.reference(s.a, s.w, s.src)
    b = co.bounds(x)[1]
    for knobs in ({}, {"cost_lds_bytes": weights_only_dropped(e, 129)}, {"cost_lds_bytes": 0}):
        with e.tuning(**knobs):
            for c, p, l, v in co.OUTPUTS:
                co.same(run_dev(e, mt, 129, s.src, s.w, 0, None, cost=c, pred=p, len=l, via=v), x.at(), (knobs, c, p, l, v))
                co.same(run_dev(e, mt, 129, s.src, s.w, b, (0, 2), cost=c, pred=p, len=l, via=v),
                        co.reference(s.edges((0, 2)), s.w, s.src).at(b), (knobs, "bounded", c, p, l, v))


def test_device_wrapper():
    """device.reach_cost"""
    e = engine()
    s = case(129, "islands")
    x = co.reference(s.edges((0, 1)), s.w, s.src)
    c, p, ln, v, r = D.reach_cost(e, dev(s.words), 129, 3, s.src, s.w, svc_select=[1, 1, 0], pred=True, len=True, via=True)
    u = lambda t, dt: t.cpu().numpy().view(dt)
    co.same((u(c, np.uint32), u(p, np.uint16), u(ln, np.uint16), u(v, np.uint32), r), x.at(), "device.reach_cost")
    c, p, ln, v, r = D.reach_cost(e, dev(s.words), 129, 3, [0, 0], s.w, max_cost=3, cost=False)
    assert c is None and p is None and ln is None and v is None and r == co.reference(s.a, s.w, [0, 0]).at(3)[4]
    c, p, ln, v, r = D.reach_cost(e, dev(s.words)[:, :0, :0].contiguous(), 0, 3, [], [], via=True)
    assert c.numel() == 0 and v.numel() == 0 and r == dict.fromkeys(co.RESULT_FIELDS, 0)
    assert D.NO_COST == co.NONE == _capi.NO_COST and D.NO_PRED == co.NO_PRED


def test_einval_and_nothing_to_do():
    e = engine()
    w = torch.zeros(8, dtype=torch.int32, device="cuda")
    bad, keep = co.bad_specs(w.data_ptr())
    for spec, with_res, names in bad:
        res = _capi.pg_reach_cost_result(7, 7, 7, 7)
        code = lib.pg_reach_cost(e.h, C.byref(spec) if spec is not None else None, None, None, None, None,
                                 C.byref(res) if with_res else None, None)
        assert code == _capi.PG_EINVAL and names in lib.pg_last_error(e.h).decode(), (names, code, lib.pg_last_error(e.h))
    del keep
    buf = torch.full((40,), -1, dtype=torch.int32, device="cuda")
    res = _capi.pg_reach_cost_result(7, 7, 7, 7)
    code = lib.pg_reach_cost(e.h, C.byref(_capi.pg_reach_cost_spec(None, 0, 1, None, None, 0, None, 3)), buf.data_ptr(),
                             buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), C.byref(res), None)
    torch.cuda.synchronize()
    assert code == 0 and co.result_dict(res) == dict.fromkeys(co.RESULT_FIELDS, 0) and (buf.cpu().numpy() == -1).all()
    # no source: out_via is cleared, nothing else is written
    s = case(33, "ring")
    got = run_dev(e, dev(s.words), 33, np.zeros(0, np.uint32), s.w)
    assert got[4] == dict.fromkeys(co.RESULT_FIELDS, 0) and (got[3] == 0).all()
    # nothing selected: nothing is reached, every entry is still written
    got = run_dev(e, dev(s.words), 33, s.src, s.w, 0, ())
    assert got[4] == dict.fromkeys(co.RESULT_FIELDS, 0) and (got[0] == co.NONE).all() and (got[1] == co.NO_PRED).all()
    assert (got[2] == 0).all() and (got[3] == 0).all()


# ---- matrix -> cost on the device from an engine -------------------------------------------------------
def test_chain_engine_chained():
    """the chain policy with the skips 0 -> 5, 2 -> 9 and 11 -> 0: pg_reach_matrix's output stays on the device and
    feeds pg_reach_cost; the answers against reference() on the oracle's codes, and bit-equal to the host twin's"""
    c = cc.chain(((0, 5), (2, 9), (11, 0)))
    mt = D.reach_matrix(c.e, cc.CHAIN_IPS, cc.CHAIN_IPS, cc.CHAIN_SERVICES)
    words = mt.cpu().numpy().view(np.uint32)
    w = np.array([3, 1, 1, 4, 1, 9, 1, 1, 1, 2, 65535, 1], np.uint16)
    for sel in (None, (0,), (1,)):
        a = (c.codes[list(sel) if sel is not None else slice(None)] == co.ALLOW).any(axis=0)
        for b in (0, 7):
            d = run_dev(c.e, mt, cc.CHAIN_N, np.arange(cc.CHAIN_N), w, b, sel)
            co.same(d, co.reference(a, w, range(cc.CHAIN_N)).at(b), (sel, b))
            equal_runs(co.run_host(c.e, words, cc.CHAIN_N, np.arange(cc.CHAIN_N), w, b, sel), d, (sel, b))


def test_reachability_cost():
    """the wrapper on the chain policy against the oracle's codes, and against its host route"""
    c = cc.chain(((0, 5), (2, 9), (11, 0)))
    co.check_wrapper(c)
    for pods, src, max_cost in co.WRAPPER_CASES:
        assert c.e.reachability_cost(pods, cc.CHAIN_SERVICES, src, co.WRAPPER_WEIGHTS, max_cost) == \
            c.e.reachability_cost(pods, cc.CHAIN_SERVICES, src, co.WRAPPER_WEIGHTS, max_cost, host=True)


def test_counters_untouched():
    """the counters and their snapshots are bit-identical before and after the call on that context"""
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
    g = case(300, "random4")
    co.same(run_dev(e, dev(g.words), 300, g.src, g.w), co.reference(g.a, g.w, g.src).at(), "counters")
    assert (D.counters_snapshot(e) == snap).all()
    assert (D.read_counters(e) == before).all()
    D.reset_counters(e)
