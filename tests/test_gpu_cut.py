"""The reachability cut on the device: pg_reach_cut against the references of tests/cut_cases.py and, byte
for byte including `levels` and `reroutes`, against the host twin over the same graphs with blocks_per_cu
unset and 1; layers at the sizes where the launch plan changes (lanes of 1, 2 and 4 bit-words) and once at
2^15 end points; a random graph of 8193 end points against scipy's maximum flow, which
tests/test_cut_host.py pins to the Python one; an input that is not 16-B aligned, a stream of its own over
prefilled buffers, matrix -> cut chained on the device from an engine, the wrapper against the oracle, the
arguments, and away from the counters.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import closure_cases as cc
import cut_cases as ct
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


def run_dev(e, mt, n, E, T, max_cut=ct.LARGE, select=None, cut=True, prev=True, nxt=True, stream=None):
    """pg_reach_cut over prefilled outputs with guards; ct.run_host's contract on a device tensor"""
    n_svc = mt.numel() // (n * cc.row_words(n))
    st = stream or torch.cuda.current_stream()
    with torch.cuda.stream(st):
        cbuf = torch.full((n + ct.GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        pbuf = torch.full((n + ct.GUARD,), 0xEEEE - 0x10000, dtype=torch.int16, device="cuda")
        xbuf = torch.full((n + ct.GUARD,), 0xEEEE - 0x10000, dtype=torch.int16, device="cuda")
    st.synchronize()
    spec, keep = ct.spec_of(mt.data_ptr(), n, n_svc, E, T, max_cut, select)
    res = _capi.pg_reach_cut_result(*[77] * 9)
    code = lib.pg_reach_cut(e.h, C.byref(spec), cbuf.data_ptr() if cut else None, pbuf.data_ptr() if prev else None,
                            xbuf.data_ptr() if nxt else None, C.byref(res), C.c_void_p(st.cuda_stream))
    assert code == 0, lib.pg_last_error(e.h)
    del keep
    # (the call has synchronised its stream: no wait here before the outputs are read)
    u16 = lambda t: t.cpu().numpy().view(np.uint16)
    return ct.finish(n, cbuf.cpu().numpy(), u16(pbuf), u16(xbuf), res, cut, prev, nxt)


def run(*args, **kw):
    return run_dev(engine(), *args, **kw)


def equal_runs(h, d, what):
    """a host twin's and a device's return value, byte for byte, `levels` and `reroutes` included"""
    assert h[3] == d[3], (what, h[3], d[3])
    for x, y in zip(h[:3], d[:3]):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), what


def both(e, words):
    """a `run` for ct.check over a device tensor: the device's answer, held byte for byte to the host twin's"""
    def go(mt, n, E, T, max_cut=ct.LARGE, select=None, **kw):
        d = run_dev(e, mt, n, E, T, max_cut, select, **kw)
        equal_runs(ct.run_host(e, words, n, E, T, max_cut, select, **kw), d, (n, E, T, max_cut, select, kw))
        return d
    return go


@pytest.mark.parametrize("family", ct.FAMILIES)
def test_synthetic(family):
    e = engine()
    for n in ct.SIZES:
        s = ct.graph(n, family)
        mt = dev(s.words)
        ct.check(both(e, s.words), mt, s, n, family)
        if family in ct.NEW_FAMILIES:
            ct.check_known(run, mt, s, n, family)
        with e.tuning(blocks_per_cu=1):
            ct.check(run, mt, s, n, family, small=True)


def test_small_graphs():
    """the device against the definition, and the host twin"""
    e = engine()
    for a, E, T in ct.small_cases():
        n = a.shape[0]
        s = ct.Graph(a, "layers", 2, seed=n)
        d = run(dev(s.words), n, E, T)
        ct.same(d, ct.brute(a, E, T), a, E, T, ct.LARGE, (a.astype(int).tolist(), E, T))
        equal_runs(ct.run_host(e, s.words, n, E, T), d, (n, E, T))


def test_zigzag_and_chain():
    """flow cancelled on the device; a chain of 300: many cheap levels"""
    s = ct.graph(64, "zigzag")
    r = ct.check_known(run, dev(s.words), s, 64, "zigzag")
    assert r["reroutes"] == 8, r
    n = 300
    s = ct.graph(n, "chain", 1)
    d = run(dev(s.words), n, (0,), (n - 1,))
    assert d[3]["cut_size"] == 1 and d[3]["near_reach"] == 1 and d[3]["far_reach"] == n - 2, d[3]
    equal_runs(ct.run_host(engine(), s.words, n, (0,), (n - 1,)), d, "chain 300")


# ---- every variant of the plan, sizes read from the plan -------------------------------------------
def check_layers(e, n, host_twin):
    widths = [3, 40, 5, n - 100, 5, 44, 3]
    E, T = (0, 1, 2), (n - 3, n - 2, n - 1)
    words = ct.layers_words(widths)
    mt = dev(words)
    c, pv, nx, r = run_dev(e, mt, n, E, T)
    assert {f: r[f] for f in ct.EXACT} == dict(zip(ct.EXACT, (1, 0, 0, 5, 5, 43, n - 52))), r
    assert np.flatnonzero(c & ct.NEAR).tolist() == list(range(43, 48)) and np.flatnonzero(c & ct.FAR).tolist() == list(range(n - 52, n - 47))
    assert np.flatnonzero(c & ct.NEAR_REACH).tolist() == list(range(43)) and np.flatnonzero(c & ct.FAR_REACH).tolist() == list(range(n - 52))
    # the witness without the n x n edge matrix: five chains over consecutive layers
    at = np.concatenate([[0], np.cumsum(widths)])
    layer = np.searchsorted(at, np.arange(n), side="right") - 1
    on = np.flatnonzero(pv != ct.NO_HOP)
    assert len(on) == 25 and (nx[on] != ct.NO_HOP).all() and (layer[pv[on]] == layer[on] - 1).all() and (layer[nx[on]] == layer[on] + 1).all()
    assert len(set(on.tolist())) == 25 and (np.bincount(layer[on], minlength=7) == [0, 5, 5, 5, 5, 5, 0]).all()
    inner = on[layer[on] < 5]
    assert (pv[nx[inner]] == inner).all()
    # capped, the result alone, and a single output
    capped = run_dev(e, mt, n, E, T, 4, None, cut=False, prev=False, nxt=False)[3]
    assert {f: capped[f] for f in ct.EXACT} == dict(zip(ct.EXACT, (1, 1, 0, ct.NO_CUT, 5, 0, 0))), capped
    if host_twin:
        equal_runs(ct.run_host(e, words, n, E, T), (c, pv, nx, r), (n, "layers against the host twin"))


@pytest.mark.parametrize("k", range(6))
def test_layers_at_plan_sizes(k):
    """n at -1, 0, +1 around the two sizes where the plan changes"""
    e = engine()
    n = ct.plan_sizes(e)[k]
    assert e.debug_reach_cut_plan(n)["lane_words"] == (1, 2, 2, 2, 4, 4)[k]
    check_layers(e, n, host_twin=True)


def test_layers_at_most_end_points():
    """2^15 end points: four steps of 256 words along a row"""
    e = engine()
    n = 1 << 15
    assert (e.debug_reach_cut_plan(n)["lane_words"], e.debug_reach_cut_plan(n)["row_steps"]) == (4, 4)
    check_layers(e, n, host_twin=False)


# ---- one random graph against scipy ----------------------------------------------------------------
def test_random_graph():
    """4 edges per node at 8193 end points, 4 entries and 4 targets"""
    e = engine()
    n = 8193
    s = cc.LargeMedium(n, seed=cc.LARGE_SEED)
    a = s.edge_matrix()
    mt = dev(s.words)
    g = np.random.default_rng(5)
    ids = g.permutation(n)[:8]
    E, T = tuple(int(x) for x in ids[:4]), tuple(int(x) for x in ids[4:])
    x = ct.flow_scipy(a, E, T)
    assert x.cut_size is not None and x.cut_size >= 4, x.cut_size
    ct.same(run_dev(e, mt, n, E, T), x, a, E, T, ct.LARGE, "random 8193")
    ct.same(run_dev(e, mt, n, E, T, x.cut_size - 1, nxt=False), x, a, E, T, x.cut_size - 1, "random 8193, capped")


# ---- the launch's surroundings ---------------------------------------------------------------------
def test_unaligned_input():
    """the input one word behind a 16-B boundary"""
    for n, family in ((17, "dense"), (129, "medium"), (257, "grid")):
        s = ct.graph(n, family, 3, 5)
        a = ct.edge_matrix(s.codes)
        for E, T in ct.end_sets(n, family, a)[:3]:
            ct.same(run(dev(s.words, offset=1), n, E, T), ct.expected(n, family, E, T, None, 3, 5), a, E, T, ct.LARGE, (n, family, E, T))


def test_stream_and_prefill():
    """a non-default stream over prefilled outputs (run_dev holds the guards)"""
    s = ct.graph(257, "medium", 3, 8)
    mt = dev(s.words)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ct.check(lambda *args, **kw: run(*args, stream=st, **kw), mt, s, 257, "medium", 8)


def test_device_wrapper():
    """device.reach_cut"""
    e = engine()
    n = 129
    s = ct.graph(n, "layers")
    a, E, T = ct.new_family(n, "layers")
    x = ct.expected(n, "layers", E, T, (0, 1))
    c, pv, nx, r = D.reach_cut(e, dev(s.words), n, 3, list(E), list(T), svc_select=[1, 1, 0], cut=True, paths=True)
    want, flags = x.at(16)
    assert {k: r[k] for k in ct.EXACT} == want and (c.cpu().numpy() == flags).all()
    pv, nx = pv.cpu().numpy().view(np.uint16), nx.cpu().numpy().view(np.uint16)
    ct.check_witness(ct.edge_matrix(s.codes, (0, 1)), E, T, pv, nx, want["n_paths"])
    assert len(D.cut_routes(pv, nx, E)) == want["n_paths"]
    c, pv, nx, r = D.reach_cut(e, dev(s.words), n, 3, [0, 0], [n - 1], max_cut=0)
    assert c is None and pv is None and nx is None and (r["capped"], r["n_paths"], r["cut_size"]) == (1, 1, D.NO_CUT)
    c, pv, nx, r = D.reach_cut(e, dev(s.words)[:, :0, :0].contiguous(), 0, 3, [], [], cut=True)
    assert c.numel() == 0 and r == dict.fromkeys(ct.RESULT_FIELDS, 0)


def test_einval_and_no_end_points():
    e = engine()
    w = torch.zeros(8, dtype=torch.int32, device="cuda")
    bad, keep = ct.bad_specs(w.data_ptr())
    for spec, with_res, names in bad:
        res = _capi.pg_reach_cut_result(*[7] * 9)
        code = lib.pg_reach_cut(e.h, C.byref(spec) if spec is not None else None, None, None, None,
                                C.byref(res) if with_res else None, None)
        assert code == _capi.PG_EINVAL and names in lib.pg_last_error(e.h).decode(), (names, code, lib.pg_last_error(e.h))
    del keep
    buf = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    res = _capi.pg_reach_cut_result(*[7] * 9)
    code = lib.pg_reach_cut(e.h, C.byref(_capi.pg_reach_cut_spec(None, 0, 1, None, None, 0, None, 0, 3)), buf.data_ptr(),
                            buf.data_ptr(), buf.data_ptr(), C.byref(res), None)
    torch.cuda.synchronize()
    assert code == 0 and ct.result_dict(res) == dict.fromkeys(ct.RESULT_FIELDS, 0) and (buf.cpu().numpy() == -1).all()


# ---- matrix -> cut on the device from an engine ----------------------------------------------------
def test_chain_engine_chained():
    """the chain policy with the skips 0 -> 5 and 2 -> 9: pg_reach_matrix's output stays on the device and
    feeds pg_reach_cut; the answers against flow() on the oracle's codes, and bit-equal to the host twin's"""
    c = cc.chain(((0, 5), (2, 9)))
    mt = D.reach_matrix(c.e, cc.CHAIN_IPS, cc.CHAIN_IPS, cc.CHAIN_SERVICES)
    words = mt.cpu().numpy().view(np.uint32)
    for E, T in (((0,), (11,)), ((0, 1), (9, 10)), ((3,), (4,)), ((11,), (0,))):
        for sel in (None, (0,)):
            a = ct.edge_matrix(c.codes, sel)
            d = run_dev(c.e, mt, cc.CHAIN_N, E, T, 16, sel)
            ct.same(d, ct.flow(a, E, T), a, E, T, 16, (E, T, sel))
            equal_runs(ct.run_host(c.e, words, cc.CHAIN_N, E, T, 16, sel), d, (E, T, sel))


def test_reachability_cut():
    """the wrapper on the chain policy against oracle.world.World.conn fed to flow(), and against its host route"""
    c = cc.chain(((0, 5), (2, 9)))
    for pods, entry, target, max_cut in ct.WRAPPER_CASES:
        got = c.e.reachability_cut(pods, cc.CHAIN_SERVICES, entry, target, max_cut)
        ct.check_wrapper(c, got, pods, entry, target, max_cut)
        assert got == c.e.reachability_cut(pods, cc.CHAIN_SERVICES, entry, target, max_cut, host=True)


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
    g = ct.graph(257, "medium", 3, 10)
    a = ct.edge_matrix(g.codes)
    ct.same(run_dev(e, dev(g.words), 257, (0, 1), (255, 256)), ct.expected(257, "medium", (0, 1), (255, 256), None, 3, 10), a, (0, 1), (255, 256),
            ct.LARGE, "counters")
    assert (D.counters_snapshot(e) == snap).all()
    assert (D.read_counters(e) == before).all()
    D.reset_counters(e)
