"""The reachability closure on the device: pg_reach_closure against numpy and, byte for byte, against the
host twin over the graphs of tests/closure_cases.py, the sizes around the launch plan's tile, the islands
and a random graph at the sizes where a lane goes to 4 bit-words and a second column tile begins (against
a torch reference on the device, itself pinned to numpy), an input
that is not 16-B aligned, a stream of its own over prefilled buffers, matrix -> closure -> diff chained on
the device from two engines, and away from the counters.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import closure_cases as cc
import diff_cases as dc
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


def launch(e, mt, n, select, max_hops, hops, counts, stream=None):
    """pg_reach_closure over prefilled outputs with guards -> (packed, hops, counts: the device buffers with
    their guards, the result struct)"""
    rw = cc.row_words(n)
    n_svc = mt.numel() // (n * rw)
    st = stream or torch.cuda.current_stream()
    with torch.cuda.stream(st):
        pbuf = torch.full((n * rw + cc.GUARD,), -1, dtype=torch.int32, device="cuda")
        hbuf = torch.full((n * n + cc.GUARD,), -1, dtype=torch.int16, device="cuda")
        cbuf = torch.full((n + cc.GUARD,), -1, dtype=torch.int32, device="cuda")
    f = cc.flags(select, n_svc)
    spec = _capi.pg_reach_closure_spec(mt.data_ptr(), n, n_svc, f.ctypes.data if f is not None else None, max_hops)
    res = _capi.pg_reach_closure_result(77, 77, 77)
    code = lib.pg_reach_closure(e.h, C.byref(spec), pbuf.data_ptr(), hbuf.data_ptr() if hops else None,
                                cbuf.data_ptr() if counts else None, C.byref(res), C.c_void_p(st.cuda_stream))
    assert code == 0, lib.pg_last_error(e.h)
    # (the call has synchronised its stream: no wait here before the outputs are read)
    return pbuf, hbuf, cbuf, res


def run_dev(e, mt, n, select=None, max_hops=0, hops=True, counts=True, stream=None):
    """launch() with every output on the host; cc.run_host's contract on a device tensor"""
    pbuf, hbuf, cbuf, res = launch(e, mt, n, select, max_hops, hops, counts, stream)
    return cc.finish(n, u32(pbuf), hbuf.cpu().numpy().view(np.uint16), u32(cbuf), res, hops, counts)


def run_big(e, mt, n, select=None, max_hops=0, hops=True, counts=True):
    """run_dev() for a large graph: the hop counts stay on the device (int16 [n, n]), their guard and their
    prefill are checked there; the packed words and the counts come to the host through cc.finish"""
    pbuf, hbuf, cbuf, res = launch(e, mt, n, select, max_hops, hops, counts)
    assert bool((hbuf[n * n:] == -1).all()), "a guard was written"
    assert hops or bool((hbuf == -1).all())
    packed, _, c, r = cc.finish(n, u32(pbuf), np.full(cc.GUARD, 0xFFFF, np.uint16), u32(cbuf), res, False, counts)
    return packed, hbuf[:n * n].view(n, n) if hops else None, c, r


def run(*args, **kw):
    return run_dev(engine(), *args, **kw)


def same_as_host(e, words, mt, n, select=None, max_hops=0):
    h, d = cc.run_host(e, words, n, select, max_hops), run_dev(e, mt, n, select, max_hops)
    assert h[3] == d[3] and all(x.tobytes() == y.tobytes() for x, y in zip(h[:3], d[:3])), (n, select, max_hops)
    return d


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_synthetic(family):
    for n in cc.SIZES:
        s = cc.synthetic(n, family)
        mt = dev(s.words)
        same_as_host(engine(), s.words, mt, n)
        same_as_host(engine(), s.words, mt, n, (0, 2), 2)
        cc.check(run, mt, n, s.expected, s.n_svc, variants=n in (17, 100, 257))


def plan(e, n):
    with e.tuning(blocks_per_cu=1):
        return e.debug_reach_closure_plan(n)


@pytest.mark.parametrize("family", ("medium", "dense", "two-cliques"))
def test_sizes_around_tile(family):
    """n of tile_cols - 1, tile_cols, tile_cols + 1 and tile_rows +- 1, from the plan of the smallest graph"""
    e = engine()
    p = plan(e, 1)
    for n in (p["tile_cols"] - 1, p["tile_cols"], p["tile_cols"] + 1, p["tile_rows"] - 1, p["tile_rows"] + 1):
        s = cc.synthetic(n, family, n_svc=2, seed=3)
        x = s.expected()
        assert x.levels <= 16, (family, n, x.levels)
        grid = plan(e, n)["grid"]
        assert grid >= -(-n // p["tile_rows"])
        mt = dev(s.words)
        with e.tuning(blocks_per_cu=1):
            cc.same(run(mt, n, None, 0), x, 0, (family, n))
            cc.same(run(mt, n, None, 2, counts=False), x, 2, (family, n, "bounded"))


def test_two_column_tiles():
    """a star just past the widest column tile: the widest lanes and a second column of workgroups"""
    e = engine()
    n = plan(e, 1 << 15)["tile_cols"] + 8
    p = plan(e, n)
    assert p["grid"] == 2 * -(-n // p["tile_rows"])
    s = cc.synthetic(n, "star", n_svc=1, seed=4)
    x = s.expected()
    assert x.levels == 2 and x.at(0)[3]["n_reachable"] == n * n
    cc.same(run(dev(s.words), n, None, 0), x, 0, "star")


# ---- past 4096 end points: a reference on the device that shares no code with the kernels ----------
def dev_pack(reach):
    """bool [n, n] on the device -> the closure's packed words on the host (u32 [n, row_words]): ALLOW where
    reachable, padding zero; in blocks of rows, as sums of 16 cells times 2 * 4^k"""
    n, rw = reach.shape[0], cc.row_words(reach.shape[0])
    weight = torch.tensor([cc.ALLOW << (2 * k) for k in range(16)], dtype=torch.int64, device="cuda")
    out = torch.empty((n, rw), dtype=torch.int64, device="cuda")
    for r0 in range(0, n, 1024):
        cells = torch.zeros((min(1024, n - r0), rw * 16), dtype=torch.int64, device="cuda")
        cells[:, :n] = reach[r0:r0 + 1024]
        out[r0:r0 + 1024] = (cells.view(-1, rw, 16) * weight).sum(dim=2)
    return out.cpu().numpy().astype(np.uint32)


class DevExpected:
    """cc.Expected's answers from hop counts held on the device (int16 [n, n])"""

    def __init__(self, hops):
        self.hops, self.n, self.levels = hops, hops.shape[0], int(hops.max()) if hops.numel() else 0

    @classmethod
    def closure(cls, edges):
        """the closure of a bool edge matrix on the device by level-wise boolean products, each an fp32
        matrix product of 0/1 operands (sums <= n < 2^24: exact)"""
        a = edges.float()
        hops, reach, front = edges.to(torch.int16), edges.clone(), edges
        level = int(edges.any())
        while level:
            front = ((front.float() @ a) > 0) & ~reach
            if not bool(front.any()):
                break
            level += 1
            hops.masked_fill_(front, level)
            reach |= front
        assert int(hops.max()) == level
        return cls(hops)

    @classmethod
    def of(cls, hops):
        """from a uint16 numpy matrix"""
        return cls(torch.from_numpy(np.ascontiguousarray(hops).view(np.int16)).cuda())

    def at(self, max_hops=0):
        """(packed u32 on the host, hops int16 on the device, counts u32 on the host, result dict) under max_hops"""
        hops = self.hops if not max_hops else torch.where(self.hops <= max_hops, self.hops, torch.zeros_like(self.hops))
        reach = hops > 0
        res = {"levels": int(hops.max()), "n_edges": int((self.hops == 1).sum()), "n_reachable": int(reach.sum())}
        return dev_pack(reach), hops, reach.sum(dim=1).cpu().numpy().astype(np.uint32), res

    def numbers(self):
        r = self.at(0)[3]
        return r["n_edges"], r["n_reachable"], r["levels"]


def same_big(got, x, max_hops, what):
    """cc.same() for run_big() against a DevExpected: the hop counts are compared on the device"""
    packed, h, c, r = got
    want_packed, want_hops, want_counts, res = x.at(max_hops)
    assert r == res, (what, r, res)
    assert (packed == want_packed).all(), (what, "packed", np.argwhere(packed != want_packed)[:3].tolist())
    assert h is None or torch.equal(h, want_hops), (what, "hops", (h != want_hops).nonzero()[:3].tolist())
    assert c is None or (c == want_counts).all(), (what, "counts", np.flatnonzero(c != want_counts)[:3].tolist())


@pytest.mark.parametrize("family", ("medium", "two-cliques"))
@pytest.mark.parametrize("n", (257, 2049))
def test_device_reference(n, family):
    """the device reference against cc.Expected, bit for bit: hops, and under max_hops 0, 2 and levels - 1 the
    packed words, the counts and the result"""
    s = cc.synthetic(n, family, n_svc=2, seed=3)
    for sel in (None, (1,)):
        x = s.expected(sel)
        d = DevExpected.closure(torch.from_numpy(x.edges).cuda())
        assert d.levels == x.levels and (d.hops.cpu().numpy().view(np.uint16) == x.hops).all(), (n, family, sel)
        for k in (0, 2, max(1, x.levels - 1)):
            reach, hops, counts, res = x.at(k)
            packed, dh, dc_, dres = d.at(k)
            assert dres == res and (packed == cc.pack_reach(reach)).all() and (dc_ == counts).all(), (n, family, sel, k)
            assert (dh.cpu().numpy().view(np.uint16) == hops).all()
        assert (DevExpected.of(x.hops).hops.cpu().numpy().view(np.uint16) == x.hops).all()


def check_large(e, s, n, expected, host_twin):
    """the runs of cc.large_runs over a large graph `s` against `expected(select)` -> DevExpected, and byte for
    byte against the host twin"""
    mt = dev(s.words)
    for sel, k, hops, counts in cc.large_runs(expected(None).levels):
        same_big(run_big(e, mt, n, sel, k, hops, counts), expected(sel), k, (s.family, n, sel, k, hops, counts))
    if host_twin:
        h, d = cc.run_host(e, s.words, n), run_big(e, mt, n)
        assert h[3] == d[3] and h[0].tobytes() == d[0].tobytes() and h[2].tobytes() == d[2].tobytes(), (s.family, n)
        assert torch.equal(d[1], torch.from_numpy(h[1].view(np.int16)).cuda()), (s.family, n, "hops")


def test_edge_plans():
    e = engine()
    sizes = cc.edge_sizes(e)
    assert tuple(cc.plan_shape(e, n) for n in sizes) == cc.EDGE_PLANS


@pytest.mark.parametrize("k", range(6))
def test_islands_at_plan_edges(k):
    """the islands at tile_cols - 1, tile_cols and tile_cols + 1 of the plans of 4096 and of 2^15 end points:
    lanes of 2 and of 4 bit-words, one and two column tiles, the pack kernel's second round"""
    e = engine()
    n = cc.edge_sizes(e)[k]
    assert cc.plan_shape(e, n) == cc.EDGE_PLANS[k]
    s = cc.Islands(n, seed=cc.LARGE_SEED)
    cc.check_walk_shape(s.expected())
    ref = DevExpected.closure(torch.from_numpy(s.expected().edges).cuda())
    assert ref.numbers() == cc.LARGE_WANT[n, "islands", cc.LARGE_SEED]
    assert torch.equal(ref.hops, DevExpected.of(s.expected().hops).hops)
    del ref
    expected = functools.lru_cache(maxsize=None)(lambda sel: DevExpected.of(s.expected(sel).hops))
    check_large(e, s, n, expected, host_twin=True)


@pytest.mark.parametrize("k", (2, 5))
def test_medium_past_plan_edges(k):
    """a random graph of 4 edges per node one past the two tile widths: every row tile alive, frontiers in
    every chunk; the device reference reproduces the numbers the CPU reference gave"""
    e = engine()
    n = cc.edge_sizes(e)[k]
    assert cc.plan_shape(e, n) == cc.EDGE_PLANS[k]
    s = cc.LargeMedium(n, seed=cc.LARGE_SEED)
    expected = functools.lru_cache(maxsize=None)(lambda sel: DevExpected.closure(torch.from_numpy(s.edge_matrix(sel)).cuda()))
    assert expected(None).numbers() == cc.LARGE_WANT[n, "medium", cc.LARGE_SEED]
    check_large(e, s, n, expected, host_twin=k == 2)


def test_unaligned_input():
    """the input one word behind a 16-B boundary"""
    for n, family in ((17, "dense"), (100, "medium"), (257, "two-cliques")):
        s = cc.synthetic(n, family, seed=5)
        cc.check(run, dev(s.words, offset=1), n, s.expected, s.n_svc, variants=False)


def test_stream_and_prefill():
    """a non-default stream over prefilled outputs (run_dev holds the guards)"""
    s = cc.synthetic(257, "medium", seed=8)
    mt = dev(s.words)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    cc.check(lambda *args, **kw: run(*args, stream=st, **kw), mt, 257, s.expected, s.n_svc)


def test_device_wrapper():
    """device.reach_closure and unpack_closure"""
    e = engine()
    s = cc.synthetic(100, "sparse", seed=9)
    x = s.expected((0, 1))
    reach, hops, counts, res = x.at(0)
    packed, h, c, r = D.reach_closure(e, dev(s.words), 100, svc_select=[1, 1, 0], hops=True, counts=True)
    assert r == res and (D.unpack_closure(packed, 100) == reach).all()
    assert (h.cpu().numpy().view(np.uint16) == hops).all() and (u32(c) == counts).all()
    packed, h, c, r = D.reach_closure(e, dev(s.words), 100, max_hops=1)
    assert h is None and c is None and (D.unpack_closure(packed, 100) == s.expected().edges).all() and r["levels"] == 1
    packed, h, c, r = D.reach_closure(e, dev(s.words)[:, :0, :0].contiguous(), 0, hops=True)
    assert packed.numel() == 0 and r == {"levels": 0, "n_edges": 0, "n_reachable": 0}


def test_einval_and_no_end_points():
    e = engine()
    w = torch.zeros(8, dtype=torch.int32, device="cuda")
    ptr, S = w.data_ptr(), _capi.pg_reach_closure_spec
    res = _capi.pg_reach_closure_result(7, 7, 7)
    bad = [(None, ptr, True), (S(None, 4, 1, None, 0), ptr, True), (S(ptr, 4, 1, None, 0), None, True),
           (S(ptr, 4, 1, None, 0), ptr, False), (S(ptr, (1 << 15) + 1, 1, None, 0), ptr, True),
           (S(ptr, 4, 0, None, 0), ptr, True), (S(ptr, 4, 4097, None, 0), ptr, True)]
    for spec, out, with_res in bad:
        code = lib.pg_reach_closure(e.h, C.byref(spec) if spec is not None else None, out, None, None,
                                    C.byref(res) if with_res else None, None)
        assert code == _capi.PG_EINVAL and lib.pg_last_error(e.h), (spec, code)
    buf = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    code = lib.pg_reach_closure(e.h, C.byref(S(ptr, 0, 1, None, 0)), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                                C.byref(res), None)
    torch.cuda.synchronize()
    assert code == 0 and (res.levels, res.n_edges, res.n_reachable) == (0, 0, 0) and (buf.cpu().numpy() == -1).all()


# ---- matrix -> closure -> diff on the device, inputs from two engines ---------------------------
def test_fixture_change_chained():
    """the fixture change under service 0: 984 cells of the closure opened, 138 closed"""
    c, w = cc.fixture_change(), cc.FIXTURE_WANT
    n = len(c.dst)
    sel = [1] + [0] * (len(dc.SERVICES) - 1)
    closures = []
    for e, codes, ctx in zip((c.e0, c.e1), c.closure_codes, (c.e1, engine())):   # the context only names the device
        mt = D.reach_matrix(e, c.dst, c.dst, dc.SERVICES)
        packed, hops, counts, res = D.reach_closure(ctx, mt, n, svc_select=sel, hops=True, counts=True)
        x = cc.Expected(codes, (0,))
        cc.same((u32(packed), hops.cpu().numpy().view(np.uint16), u32(counts), res), x, 0, "fixture")
        host = cc.run_host(ctx, e.debug_reach_matrix_host(c.dst, c.dst, dc.SERVICES, words=False), n, (0,), 0)
        assert host[0].tobytes() == u32(packed).tobytes()
        closures.append(packed)
    b, a = closures
    assert D.reach_diff(c.e0, b, a, n, dc.OPENED, cap=0)[0] == w["closure_opened"]
    k, changes, trans, _ = D.reach_diff(c.e1, b, a, n, dc.CLOSED)
    rb, ra = (cc.Expected(codes, (0,)).hops > 0 for codes in c.closure_codes)
    row, col, cb, ca = D.unpack_changes(changes)
    assert k == w["closure_closed"] and (np.stack([row, col], axis=1) == np.argwhere(rb & ~ra)).all()
    assert (cb == 2).all() and (ca == 0).all() and int(trans.sum()) == n * n and trans[1].sum() == trans[3].sum() == 0


def test_chain_engines_chained():
    """the chain policy before and after the edge c11 -> c0: device closures bit-equal to the host twin's,
    their diff on the device, and the wrappers"""
    before, after = cc.chain(), cc.chain(((11, 0),))
    closures = []
    for c in (before, after):
        mt = D.reach_matrix(c.e, cc.CHAIN_IPS, cc.CHAIN_IPS, cc.CHAIN_SERVICES)
        cc.check(lambda *args, **kw: run_dev(c.e, *args, **kw), mt, cc.CHAIN_N, c.expected, len(cc.CHAIN_SERVICES))
        closures.append(same_as_host(c.e, u32(mt), mt, cc.CHAIN_N)[0])
    b, a = (dev(x) for x in closures)
    assert D.reach_diff(engine(), b, a, cc.CHAIN_N, dc.OPENED, cap=0)[0] == 144 - 66
    x = after.expected(None)
    reach, hops, levels = after.e.reachability_closure(cc.CHAIN_PODS, cc.CHAIN_SERVICES)
    assert levels == 12 and reach.all() and (hops == x.hops).all()
    got = after.e.reachability_closure_diff(before.e, cc.CHAIN_PODS, cc.CHAIN_SERVICES)
    assert len(got) == 144 - 66 and got == after.e.reachability_closure_diff(before.e, cc.CHAIN_PODS, cc.CHAIN_SERVICES, host=True)


def test_counters_untouched():
    """the counters and their snapshots are bit-identical before and after a closure on that context"""
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
    g = cc.synthetic(257, "medium", seed=10)
    cc.same(run_dev(e, dev(g.words), 257), g.expected(), 0, "counters")
    assert (D.counters_snapshot(e) == snap).all()
    assert (D.read_counters(e) == before).all()
    D.reset_counters(e)
