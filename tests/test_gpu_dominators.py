"""The reachability dominators on the device: pg_reach_dominators against numpy and, byte for byte
including `rounds`, against the host twin over the graphs of tests/dominators_cases.py with blocks_per_cu
unset and 1; the islands at the sizes where the launch plan changes (lanes of 1, 2 and 4 bit-words, one and
two column tiles) and once at 2^15 end points; a random graph of 8193 end points against a torch reference
on the device that tests/test_dominators_host.py pins to numpy; an input that is not 16-B aligned, a
stream of its own over prefilled buffers, a chain of 300, matrix -> dominators -> diff chained on the
device from two engines, the wrapper against the oracle, the arguments, and away from the counters.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import closure_cases as cc
import diff_cases as dc
import dominators_cases as dm
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


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def launch(e, mt, n, entry, select, dom, idom, cut, stream=None):
    """pg_reach_dominators over prefilled outputs with guards -> (dom, idom, cut: the device buffers with
    their guards, the result struct)"""
    rw = cc.row_words(n)
    n_svc = mt.numel() // (n * rw)
    st = stream or torch.cuda.current_stream()
    with torch.cuda.stream(st):
        dbuf = torch.full((n * rw + dm.GUARD,), -1, dtype=torch.int32, device="cuda")
        ibuf = torch.full((n + dm.GUARD,), 0xEEEE - 0x10000, dtype=torch.int16, device="cuda")
        cbuf = torch.full((n + dm.GUARD,), -1, dtype=torch.int32, device="cuda")
    spec, keep = dm.spec_of(mt.data_ptr(), n, n_svc, entry, select)
    res = _capi.pg_reach_dominators_result(77, 77, 77, 77, 77, 77)
    code = lib.pg_reach_dominators(e.h, C.byref(spec), dbuf.data_ptr() if dom else None, ibuf.data_ptr() if idom else None,
                                   cbuf.data_ptr() if cut else None, C.byref(res), C.c_void_p(st.cuda_stream))
    assert code == 0, lib.pg_last_error(e.h)
    del keep
    # (the call has synchronised its stream: no wait here before the outputs are read)
    return dbuf, ibuf, cbuf, res


def run_dev(e, mt, n, entry, select=None, dom=True, idom=True, cut=True, stream=None):
    """launch() with every output on the host; dm.run_host's contract on a device tensor"""
    dbuf, ibuf, cbuf, res = launch(e, mt, n, entry, select, dom, idom, cut, stream)
    return dm.finish(n, u32(dbuf), ibuf.cpu().numpy().view(np.uint16), u32(cbuf), res, dom, idom, cut)


def run(*args, **kw):
    return run_dev(engine(), *args, **kw)


def equal_runs(h, d, what):
    """a host twin's and a device's return value, byte for byte, `rounds` included"""
    assert h[3] == d[3], (what, h[3], d[3])
    for x, y in zip(h[:3], d[:3]):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), what


def both(e, words):
    """a `run` for dm.check over a device tensor: the device's answer, held byte for byte to the host twin's"""
    def go(mt, n, entry, select=None, **kw):
        d = run_dev(e, mt, n, entry, select, **kw)
        equal_runs(dm.run_host(e, words, n, entry, select, **kw), d, (n, entry, select, kw))
        return d
    return go


@pytest.mark.parametrize("family", dm.FAMILIES)
def test_synthetic(family):
    e = engine()
    for n in dm.SIZES:
        s = dm.graph(n, family)
        mt = dev(s.words)
        dm.check(both(e, s.words), mt, s, n, family)
        with e.tuning(blocks_per_cu=1):
            dm.check(run, mt, s, n, family)


def test_chain_300():
    """many cheap rounds: rounds = 299, Dom lower-triangular, idom(v) = v - 1, cut[k] = 299 - k"""
    n = 300
    s = dm.graph(n, "chain", 1)
    d, i, c, res = run(dev(s.words), n, (0,))
    assert res == {"n_reached": n, "n_chokes": n - 2, "top": 1, "top_cut": n - 2, "depth": n - 1, "rounds": n - 1}
    assert (D.unpack_closure(d, n) == np.tri(n, dtype=bool)).all() and (i[1:] == np.arange(n - 1)).all() and i[0] == dm.NO_IDOM
    assert (c == n - 1 - np.arange(n)).all()
    dm.same((d, i, c, res), dm.expected(n, "chain", (0,), None, 1), "chain 300")


# ---- every variant of the plan, sizes read from the plan -------------------------------------------
def plan_shape(e, n):
    p = e.debug_reach_dominators_plan(n)
    return p["lane_words"], p["col_tiles"]


def check_islands(e, c, host_twin):
    """the islands of an IslandCase on the device against the embedded reference; out_dom is compared on
    the device: the island rows to the expected words, every other row zero"""
    n, rw = c.n, cc.row_words(c.n)
    mt = dev(c.s.words)
    dbuf, ibuf, cbuf, res = launch(e, mt, n, c.entry, None, True, True, True)
    assert dm.result_dict(res) == c.result, (n, dm.result_dict(res), c.result)
    assert bool((dbuf[n * rw:] == -1).all()) and bool((ibuf[n:] == 0xEEEE - 0x10000).all()) and bool((cbuf[n:] == -1).all())
    d = dbuf[:n * rw].view(n, rw)
    idx = torch.from_numpy(c.idx).cuda()
    assert (u32(d[idx]) == c.dom_rows()).all(), (n, "dom")
    other = torch.ones(n, dtype=torch.bool, device="cuda")
    other[idx] = False
    assert not bool(d[other].any()), (n, "a row outside the islands")
    i, cut = ibuf[:n].cpu().numpy().view(np.uint16), u32(cbuf[:n])
    assert (i == c.idom).all() and (cut == c.cut).all(), n
    # the result alone, and a single output
    _, _, _, alone = launch(e, mt, n, c.entry, None, False, False, False)
    assert dm.result_dict(alone) == c.result
    _, ibuf2, _, res2 = launch(e, mt, n, c.entry, (0, 2), False, True, False)
    if host_twin:
        h = dm.run_host(e, c.s.words, n, c.entry)
        assert h[3] == c.result and h[1].tobytes() == i.tobytes() and h[2].tobytes() == cut.tobytes()
        assert bool(torch.equal(d, torch.from_numpy(h[0].view(np.int32)).cuda())), (n, "dom against the host twin")
        h2 = dm.run_host(e, c.s.words, n, c.entry, (0, 2), dom=False, cut=False)
        assert h2[3] == dm.result_dict(res2) and h2[1].tobytes() == ibuf2[:n].cpu().numpy().tobytes()


@pytest.mark.parametrize("k", range(9))
def test_islands_at_plan_sizes(k):
    """n at -1, 0, +1 around the three sizes where the plan changes"""
    e = engine()
    n = dm.plan_sizes(e)[k]
    assert plan_shape(e, n) == dm.PLAN_SHAPES[k]
    c = dm.IslandCase(n)
    c.non_trivial()
    check_islands(e, c, host_twin=True)


def test_islands_at_most_end_points():
    """2^15 end points: five column tiles, the reached column alone in the last"""
    e = engine()
    n = 1 << 15
    assert plan_shape(e, n) == (4, 5)
    c = dm.IslandCase(n)
    c.non_trivial()
    check_islands(e, c, host_twin=False)


# ---- one random graph against a reference on the device that shares no code with the kernels -------
def dev_pack(dom):
    """bool [n, n] on the device -> out_dom's packed words on the host (u32 [n, row_words]): ALLOW where set,
    padding zero; in blocks of rows, as sums of 16 cells times 2 * 4^k"""
    n, rw = dom.shape[0], cc.row_words(dom.shape[0])
    weight = torch.tensor([cc.ALLOW << (2 * k) for k in range(16)], dtype=torch.int64, device="cuda")
    out = torch.empty((n, rw), dtype=torch.int64, device="cuda")
    for r0 in range(0, n, 1024):
        cells = torch.zeros((min(1024, n - r0), rw * 16), dtype=torch.int64, device="cuda")
        cells[:, :n] = dom[r0:r0 + 1024]
        out[r0:r0 + 1024] = (cells.view(-1, rw, 16) * weight).sum(dim=2)
    return out.cpu().numpy().astype(np.uint32)


def test_random_graph():
    """4 edges per node at 8193 end points (lanes of 4 bit-words, two column tiles, every row tile alive),
    from node 0 and from 16 random nodes"""
    e = engine()
    n = 8193
    s = cc.LargeMedium(n, seed=cc.LARGE_SEED)
    a = torch.from_numpy(s.edge_matrix()).cuda()
    mt = dev(s.words)
    g = np.random.default_rng(5)
    for entry in ((0,), tuple(int(x) for x in g.integers(0, n, 16))):
        dom, idom, cut, res = dm.torch_expected(a, entry, "cuda")
        assert res["rounds"] >= 5 and res["n_chokes"] >= 1, res
        d, i, c, r = run_dev(e, mt, n, entry)
        assert r == res, (entry, r, res)
        assert (d == dev_pack(dom)).all() and (i == idom.cpu().numpy()).all() and (c == cut.cpu().numpy()).all(), entry


# ---- the launch's surroundings ---------------------------------------------------------------------
def test_unaligned_input():
    """the input one word behind a 16-B boundary"""
    for n, family in ((17, "dense"), (129, "medium"), (257, "tree")):
        s = dm.graph(n, family, 3, 5)
        for ent in dm.entry_sets(n)[:3]:
            dm.same(run(dev(s.words, offset=1), n, ent), dm.expected(n, family, ent, None, 3, 5), (n, family, ent))


def test_stream_and_prefill():
    """a non-default stream over prefilled outputs (run_dev holds the guards)"""
    s = dm.graph(257, "medium", 3, 8)
    mt = dev(s.words)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    dm.check(lambda *args, **kw: run(*args, stream=st, **kw), mt, s, 257, "medium", 8)


def test_device_wrapper():
    """device.reach_dominators"""
    e = engine()
    s = dm.graph(129, "tree")
    x = dm.expected(129, "tree", (0,), (0, 1))
    d, i, c, r = D.reach_dominators(e, dev(s.words), 129, 3, [0], svc_select=[1, 1, 0], dom=True, idom=True, cut=True)
    assert r == x.result and (D.unpack_closure(d, 129) == x.dom).all()
    assert (i.cpu().numpy().view(np.uint16) == x.idom).all() and (u32(c) == x.cut).all()
    d, i, c, r = D.reach_dominators(e, dev(s.words), 129, 3, [0, 5, 5])
    assert d is None and i is None and c is None and r == dm.expected(129, "tree", (0, 5, 5)).result
    d, i, c, r = D.reach_dominators(e, dev(s.words)[:, :0, :0].contiguous(), 0, 3, [], dom=True)
    assert d.numel() == 0 and r == dict.fromkeys(dm.RESULT_FIELDS, 0)


def test_einval_and_no_end_points():
    e = engine()
    w = torch.zeros(8, dtype=torch.int32, device="cuda")
    bad, keep = dm.bad_specs(w.data_ptr())
    for spec, with_res, names in bad:
        res = _capi.pg_reach_dominators_result(7, 7, 7, 7, 7, 7)
        code = lib.pg_reach_dominators(e.h, C.byref(spec) if spec is not None else None, None, None, None,
                                       C.byref(res) if with_res else None, None)
        assert code == _capi.PG_EINVAL and names in lib.pg_last_error(e.h).decode(), (names, code, lib.pg_last_error(e.h))
    del keep
    buf = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    res = _capi.pg_reach_dominators_result(7, 7, 7, 7, 7, 7)
    code = lib.pg_reach_dominators(e.h, C.byref(_capi.pg_reach_dominators_spec(None, 0, 1, None, None, 0)), buf.data_ptr(),
                                   buf.data_ptr(), buf.data_ptr(), C.byref(res), None)
    torch.cuda.synchronize()
    assert code == 0 and dm.result_dict(res) == dict.fromkeys(dm.RESULT_FIELDS, 0) and (buf.cpu().numpy() == -1).all()


# ---- matrix -> dominators -> diff on the device, inputs from two engines ---------------------------
def test_chain_engines_chained():
    """the chain policy with the skips 0 -> 5 and 2 -> 9 (live) and without them (the staged change): the
    device's answers bit-equal to the host twin's, and pg_reach_diff with PG_DIFF_OPENED over the two out_dom
    lists exactly the (v, k) that the reference says became dominators"""
    before, after = cc.chain(((0, 5), (2, 9))), cc.chain()
    doms = []
    for c in (before, after):
        mt = D.reach_matrix(c.e, cc.CHAIN_IPS, cc.CHAIN_IPS, cc.CHAIN_SERVICES)
        for ent in ((0,), (3,), (11, 4, 11)):
            for sel in (None, (0,)):
                d = run_dev(c.e, mt, cc.CHAIN_N, ent, sel)
                dm.same(d, dm.chain_expected(c, ent, sel), (ent, sel))
                equal_runs(dm.run_host(c.e, u32(mt), cc.CHAIN_N, ent, sel), d, (ent, sel))
        doms.append(D.reach_dominators(engine(), mt, cc.CHAIN_N, len(cc.CHAIN_SERVICES), [0], dom=True)[0])   # (the context only names the device)
    opened = ~dm.chain_expected(before, (0,)).dom & dm.chain_expected(after, (0,)).dom
    assert opened.sum() > 0
    k, changes, trans, _ = D.reach_diff(before.e, doms[0], doms[1], cc.CHAIN_N, dc.OPENED)
    row, col, cb, ca = D.unpack_changes(changes)
    assert k == int(opened.sum()) and (np.stack([row, col], axis=1) == np.argwhere(opened)).all()
    assert (cb == 0).all() and (ca == 2).all() and int(trans.sum()) == cc.CHAIN_N ** 2
    assert D.reach_diff(after.e, doms[0], doms[1], cc.CHAIN_N, dc.CLOSED, cap=0)[0] == 0


def test_reachability_dominators():
    """the wrapper on the chain policy against oracle.world.World.conn, and against its host route"""
    c = cc.chain(((0, 5), (2, 9)))
    for pods, entry in ((cc.CHAIN_PODS, ["ns/c0"]), (cc.CHAIN_PODS[::-1], ["ns/c1", "ns/c3"]), (cc.CHAIN_PODS, [])):
        got = c.e.reachability_dominators(pods, cc.CHAIN_SERVICES, entry)
        assert got == dm.chokepoints_want(c, pods, entry), (pods, entry)
        assert got == c.e.reachability_dominators(pods, cc.CHAIN_SERVICES, entry, host=True)


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
    g = dm.graph(257, "medium", 3, 10)
    dm.same(run_dev(e, dev(g.words), 257, (0,)), dm.expected(257, "medium", (0,), None, 3, 10), "counters")
    assert (D.counters_snapshot(e) == snap).all()
    assert (D.read_counters(e) == before).all()
    D.reset_counters(e)
