"""The reachability paths on the device: pg_reach_paths against numpy and, byte for byte, against the host
twin over the graphs of tests/closure_cases.py, the chunk boundaries under one workgroup per CU, the
sizes around a 2048-column pass, the deep ring, a hops matrix that is not 16-B aligned, a stream of its
own over prefilled buffers, every output combination, a broken matrix, 2^15 end points, multi-hop paths
at the sizes where out_via moves from LDS to global adds and where the LDS passes 48 KiB, matrix ->
closure -> paths chained on the device from two engines, the wrappers, and away from the counters.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import closure_cases as cc
import diff_cases as dc
import paths_cases as pc
from vpp_amd import _capi
from vpp_amd import device as D
from vpp_amd import renderer as R
from vpp_amd._capi import MODE_CONN, lib

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


def dev_hops(hops, offset=0):
    """hop counts -> an int16 device tensor [n, n]; offset: elements the data starts behind a fresh
    allocation (1: 2 B behind a 16-B boundary)"""
    h = np.ascontiguousarray(hops, np.uint16)
    t = torch.empty(h.size + offset, dtype=torch.int16, device="cuda")
    t[offset:] = torch.from_numpy(h.view(np.int16).ravel()).cuda()
    assert t[offset:].data_ptr() % 16 == (2 * offset) % 16
    torch.cuda.synchronize()   # (a call on a stream of its own follows)
    return t[offset:].reshape(h.shape)


def run_dev(e, ht, n, src, dst, max_len, nodes=True, via=True, stream=None):
    """pg_reach_paths over prefilled outputs with guards; pc.run_host's contract on a device tensor"""
    s, d = np.ascontiguousarray(src, np.uint32), np.ascontiguousarray(dst, np.uint32)
    nq = s.size
    st = stream or torch.cuda.current_stream()
    with torch.cuda.stream(st):
        lbuf, nbuf, vbuf = (torch.from_numpy(b.view(dt)).cuda() for b, dt in zip(pc.buffers(nq, n, max_len),
                                                                                 (np.int16, np.int16, np.int32)))
    st.synchronize()
    spec = _capi.pg_reach_paths_spec(ht.data_ptr(), n, s.ctypes.data, d.ctypes.data, nq, max_len)
    res = _capi.pg_reach_paths_result(77, 77, 77, 77, 77, 77)
    code = lib.pg_reach_paths(e.h, C.byref(spec), lbuf.data_ptr(), nbuf.data_ptr() if nodes else None,
                              vbuf.data_ptr() if via else None, C.byref(res), C.c_void_p(st.cuda_stream))
    assert code == 0, lib.pg_last_error(e.h)
    # (the call has synchronised its stream: no wait here before the outputs are read)
    return pc.finish(nq, n, max_len, lbuf.cpu().numpy().view(np.uint16), nbuf.cpu().numpy().view(np.uint16),
                     vbuf.cpu().numpy().view(np.uint32), res, nodes, via)


def device_runner(e=None, offset=0, stream=None):
    """pc.run_host's contract without the engine, on the device; the hops go up once per matrix"""
    cache = {}

    def run(hops, n, src, dst, max_len, nodes=True, via=True):
        if id(hops) not in cache:
            cache.clear()
            cache[id(hops)] = (hops, dev_hops(hops, offset))
        return run_dev(e or engine(), cache[id(hops)][1], n, src, dst, max_len, nodes, via, stream)
    return run


def same_as_host(e, hops, ht, n, src, dst, max_len, nodes=True, via=True, via_defined=True):
    h, d = pc.run_host(e, hops, n, src, dst, max_len, nodes, via), run_dev(e, ht, n, src, dst, max_len, nodes, via)
    assert h[3] == d[3], (h[3], d[3])
    for k, (x, y) in enumerate(zip(h[:3], d[:3])):
        assert (x is None and y is None) or (k == 2 and not via_defined) or x.tobytes() == y.tobytes(), (n, k)
    return d


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_synthetic(family):
    e = engine()
    for n in cc.SIZES:
        s = cc.synthetic(n, family)
        cx = s.expected()
        src, dst = pc.all_pairs(n)
        same_as_host(e, cx.hops, dev_hops(cx.hops), n, src, dst, max(1, cx.levels))
        pc.check(device_runner(), s, e.debug_reach_paths_plan(n)["chunk_queries"], variants=n in (17, 257))


@pytest.mark.parametrize("family", ("sparse", "chain", "dense"))
def test_chunk_boundaries_one_block_per_cu(family):
    """the chunk-boundary sets and the shuffled set under blocks_per_cu = 1: a workgroup runs several items
    and crosses a src change"""
    e = engine()
    n = 257
    s = cc.synthetic(n, family)
    cx = s.expected()
    x = pc.Expected(cx.hops)
    ht = dev_hops(cx.hops)
    longest = max(1, cx.levels)
    with e.tuning(blocks_per_cu=1):
        for name, (src, dst) in pc.orders(n, e.debug_reach_paths_plan(n)["chunk_queries"]).items():
            if name in ("sorted", "twice"):
                continue
            got = same_as_host(e, cx.hops, ht, n, src, dst, longest)
            pc.same(got, x, src, dst, longest, (family, name))


@pytest.mark.parametrize("n", (2047, 2048, 2049))
def test_pass_boundary(n):
    e = engine()
    for family in ("star", "two-cliques", "hub-last"):
        h, edges = pc.boundary_graph(family, n)
        src, dst, _ = pc.boundary_queries(h)
        got = same_as_host(e, h, dev_hops(h), n, src, dst, 4)
        pc.same(got, pc.Expected(h), src, dst, 4, (family, n))
        pc.valid(got, edges, h, src, dst, 4, (family, n))


def test_ring_depth():
    pc.check_ring(device_runner())
    h = pc.ring_hops(pc.RING_N)
    same_as_host(engine(), h, dev_hops(h), pc.RING_N, *pc.RING_QUERIES, 2049)


def test_unaligned_hops():
    """hops one element (2 B) behind a 16-B boundary: the rows' heads and tails take the narrow loads"""
    for n, family in ((17, "dense"), (100, "medium"), (257, "two-cliques")):
        pc.check(device_runner(offset=1), cc.synthetic(n, family, seed=5), engine().debug_reach_paths_plan(n)["chunk_queries"],
                 variants=False)


def test_stream_prefill_and_outputs():
    """a non-default stream over prefilled outputs (run_dev holds the guards), and every output combination"""
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    pc.check(device_runner(stream=st), cc.synthetic(100, "medium", seed=8), engine().debug_reach_paths_plan(100)["chunk_queries"])
    e = engine()
    s = cc.synthetic(65, "sparse", seed=8)
    cx = s.expected()
    src, dst = pc.all_pairs(65)
    for nodes, via in pc.OUTPUTS:
        same_as_host(e, cx.hops, dev_hops(cx.hops), 65, src, dst, max(1, cx.levels - 1), nodes, via)


def test_broken_matrix():
    pc.check_broken(device_runner())
    s, h, _ = pc.broken_case()
    same_as_host(engine(), h, dev_hops(h), s.n, *pc.all_pairs(s.n), s.n, via_defined=False)


def test_einval_and_empty():
    e = engine()
    h = torch.ones((4, 4), dtype=torch.int16, device="cuda")
    lens = torch.full((4,), 0x1111, dtype=torch.int16, device="cuda")
    rows = torch.full((4, 5), 0x1111, dtype=torch.int16, device="cuda")
    via = torch.full((4 + pc.GUARD,), 9, dtype=torch.int32, device="cuda")

    def one(spec, out_len, out_nodes, out_via, with_result, res=None):
        res = res or _capi.pg_reach_paths_result(7, 7, 7, 7, 7, 7)
        code = lib.pg_reach_paths(e.h, C.byref(spec) if spec is not None else None, out_len, out_nodes, out_via,
                                  C.byref(res) if with_result else None, None)
        return code, lib.pg_last_error(e.h).decode()

    pc.einval(one, h.data_ptr(), lens.data_ptr(), rows.data_ptr())
    res = _capi.pg_reach_paths_result(7, 7, 7, 7, 7, 7)
    code, _ = one(_capi.pg_reach_paths_spec(h.data_ptr(), 4, None, None, 0, 4), lens.data_ptr(), rows.data_ptr(), via.data_ptr(),
                  True, res)
    torch.cuda.synchronize()
    assert code == 0 and pc.result_dict(res) == dict.fromkeys(pc.result_dict(res), 0)
    assert (lens.cpu().numpy() == 0x1111).all() and (rows.cpu().numpy() == 0x1111).all()
    assert via.cpu().numpy().tolist() == [0] * 4 + [9] * pc.GUARD
    via[:] = 9
    res = _capi.pg_reach_paths_result(7, 7, 7, 7, 7, 7)
    code, _ = one(_capi.pg_reach_paths_spec(h.data_ptr(), 0, None, None, 0, 4), lens.data_ptr(), rows.data_ptr(), via.data_ptr(),
                  True, res)
    torch.cuda.synchronize()
    assert code == 0 and pc.result_dict(res) == dict.fromkeys(pc.result_dict(res), 0) and (via.cpu().numpy() == 9).all()


def test_32k_end_points():
    """n = 2^15, the smallest n at which the matrix reaches 2^31 bytes: the star built on the device, eight
    queries with analytic answers"""
    n = 1 << 15
    try:
        h = torch.full((n, n), 2, dtype=torch.int16, device="cuda")
    except torch.cuda.OutOfMemoryError as err:
        pytest.skip("no 2 GiB for the hops matrix: %s" % err)
    h[0, :] = 1
    h[:, 0] = 1
    h[0, 0] = 2
    queries = [(n - 1, n - 2), (0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (1, n - 1), (n // 2, n // 2 + 1), (n - 2, 1)]
    want = [[n - 1, 0, n - 2], [0, 1, 0], [0, n - 1], [n - 1, 0], [n - 1, 0, n - 1], [1, 0, n - 1], [n // 2, 0, n // 2 + 1],
            [n - 2, 0, 1]]
    src, dst = np.array(queries, np.uint32).T
    lens, rows, via, res = run_dev(engine(), h, n, src, dst, 3)
    assert lens.tolist() == [len(p) - 1 for p in want]
    assert rows.tolist() == [p + [pc.NONE] * (4 - len(p)) for p in want]
    expect_via = np.zeros(n, np.uint32)
    expect_via[0], expect_via[1] = 5, 1
    assert (via == expect_via).all()
    assert res == {"n_found": 8, "n_unreachable": 0, "n_too_long": 0, "n_broken": 0, "n_via": 6, "longest": 2}


# ---- the plan's thresholds: where out_via is counted, and the LDS a workgroup asks for -------------
@pytest.mark.parametrize("which, d", (("via_48k", 0), ("via_48k", 1), ("via_lds", 0), ("via_lds", 1)))
def test_medium_at_thresholds(which, d):
    """a random graph of 4 edges per node at the last size whose workgroup counts out_via within 48 KiB of
    LDS and one past it (the launch then asks for more), at the last size that counts it in LDS at all and
    one past it (adds to out_via itself): eight srcs against every dst over the device reference's
    closure, paths of up to levels edges; at via_lds also under one workgroup per CU, which walks many
    items and adds its LDS words once"""
    from test_gpu_closure import DevExpected
    e = engine()
    t = pc.thresholds(e)
    assert t == pc.THRESHOLDS
    n = t[which] + d
    edges = cc.LargeMedium(n, seed=cc.LARGE_SEED, words=False).edge_matrix()
    ref = DevExpected.closure(torch.from_numpy(edges).cuda())
    assert ref.numbers() == cc.LARGE_WANT[n, "medium", cc.LARGE_SEED]
    hops = ref.hops.cpu().numpy().view(np.uint16)
    levels = ref.levels
    del ref
    pc.check_few_sources(device_runner(), hops, edges, levels, outputs=which == "via_lds",
                         one_block=e.tuning(blocks_per_cu=1) if (which, d) == ("via_lds", 0) else None)


def dev_closed_form(family, n):
    """the hops of two-cliques or hub-last built on the device from their closed forms (int16 [n, n])"""
    if family == "hub-last":
        h = torch.full((n, n), 2, dtype=torch.int16, device="cuda")
        h[n - 1, :] = 1
        h[:, n - 1] = 1
        h[n - 1, n - 1] = 2
        return h
    assert family == "two-cliques"
    k = n // 2   # nodes 0 .. k - 1 and k .. n - 1, the bridge k - 1 -> k
    h = torch.zeros((n, n), dtype=torch.int16, device="cuda")
    h[:k, :k] = 1
    h[k:, k:] = 1
    h.diagonal().fill_(2)
    h[:k, k:] = 3
    h[k - 1, k:] = 2
    h[:k, k] = 2
    h[k - 1, k] = 1
    return h


@pytest.mark.parametrize("family", ("two-cliques", "hub-last"))
def test_closed_forms(family):
    for n in (257, 300):
        assert (dev_closed_form(family, n).cpu().numpy().view(np.uint16) == pc.boundary_graph(family, n)[0]).all(), (family, n)


@pytest.mark.parametrize("family", ("two-cliques", "hub-last"))
@pytest.mark.parametrize("size", ("row_48k", "row_48k + 1", "2^15"))
def test_large_rows(size, family):
    """the staged row alone at the last size within 48 KiB of LDS, one past it and past 64 KiB: paths of three
    edges across the bridge, ends in the last bit-word, dst n - 1, the hub's least predecessor, no path"""
    e = engine()
    row = pc.thresholds(e)["row_48k"]
    assert row == pc.THRESHOLDS["row_48k"]
    n = {"row_48k": row, "row_48k + 1": row + 1, "2^15": 1 << 15}[size]
    lds = e.debug_reach_paths_plan(n)["lds_bytes"]
    assert (lds <= pc.KIB48, lds > 64 * 1024) == {"row_48k": (True, False), "row_48k + 1": (False, False), "2^15": (False, True)}[size]
    try:
        h = dev_closed_form(family, n)
    except torch.cuda.OutOfMemoryError as err:
        pytest.skip("no room for the hops matrix: %s" % err)
    queries = pc.analytic_queries(family, n)
    src, dst = np.array([(s, d) for s, d, _ in queries], np.uint32).T
    pc.check_analytic(run_dev(e, h, n, src, dst, 3), n, queries, 3)
    got = run_dev(e, h, n, src[::-1], dst[::-1], 3, via=False)
    assert got[0].tolist() == [len(p) - 1 if p else 0 for _, _, p in queries[::-1]] and got[2] is None


# ---- matrix -> closure -> paths on the device, inputs from two engines --------------------------
def test_chain_engines_chained():
    """the chain policies: device hops into device paths, bit-equal to the host twin's and right by the
    oracle's edges; then the three wrappers against their host=True results"""
    plain, ring = cc.chain(), cc.chain(((11, 0),))
    n, P = cc.CHAIN_N, cc.CHAIN_PODS
    src, dst = pc.all_pairs(n)
    for c in (plain, ring):
        mt = D.reach_matrix(c.e, cc.CHAIN_IPS, cc.CHAIN_IPS, cc.CHAIN_SERVICES)
        _, hop, _, _ = D.reach_closure(c.e, mt, n, hops=True)
        x = c.expected(None)
        h = hop.cpu().numpy().view(np.uint16)
        assert (h == x.hops).all()
        got = same_as_host(engine(), h, hop, n, src, dst, n)   # (the context is another engine's on the same device)
        pc.valid(got, x.edges, h, src, dst, n, "chain")
        pc.same(got, pc.Expected(x.hops), src, dst, n, "chain")
    k = np.arange(n)
    lens, rows, via, res = D.reach_paths(plain.e, D.reach_closure(plain.e, D.reach_matrix(plain.e, cc.CHAIN_IPS, cc.CHAIN_IPS,
                                                                                         cc.CHAIN_SERVICES), n, hops=True)[1],
                                         n, src, dst, via=True)
    assert (via.cpu().numpy() == k * (11 - k)).all() and res["n_via"] == 220 and res["n_found"] == 66
    assert D.unpack_paths(lens, rows)[11] == list(range(12))
    pairs = [(P[0], P[11]), (P[5], P[4]), (P[3], P[3]), (P[11], P[0])]
    for c in (plain, ring):
        assert c.e.reachability_paths(P, cc.CHAIN_SERVICES, pairs) == c.e.reachability_paths(P, cc.CHAIN_SERVICES, pairs, host=True)
        assert c.e.reachability_chokepoints(P, cc.CHAIN_SERVICES) == c.e.reachability_chokepoints(P, cc.CHAIN_SERVICES, host=True)
    assert ring.e.reachability_paths(P, cc.CHAIN_SERVICES, pairs)[1] == [P[(5 + t) % 12] for t in range(12)]
    got = ring.e.reachability_closure_diff(plain.e, P, cc.CHAIN_SERVICES, paths=True)
    assert len(got) == 144 - 66 and got == ring.e.reachability_closure_diff(plain.e, P, cc.CHAIN_SERVICES, host=True, paths=True)


def test_fixture_change_chained():
    """the fixture change under service 0, all on the device: the queries are pg_reach_diff's changes over the
    two closures; each of the 984 opened cells has a path with an edge that is new, the 138 closed ones none"""
    c, w = cc.fixture_change(), cc.FIXTURE_WANT
    n = len(c.dst)
    sel = [1] + [0] * (len(dc.SERVICES) - 1)
    closures, hops = [], []
    for e in (c.e0, c.e1):
        packed, hop, _, _ = D.reach_closure(e, D.reach_matrix(e, c.dst, c.dst, dc.SERVICES), n, svc_select=sel, hops=True)
        closures.append(packed), hops.append(hop)
    eb, ea = (cc.Expected(codes, (0,)).edges for codes in c.closure_codes)
    ha = hops[1].cpu().numpy().view(np.uint16)
    for trans, count in ((dc.OPENED, w["closure_opened"]), (dc.CLOSED, w["closure_closed"])):
        k, changes, _, _ = D.reach_diff(c.e0, closures[0], closures[1], n, trans)
        src, dst, _, _ = D.unpack_changes(changes)
        assert k == count == len(src)
        got = same_as_host(c.e0, ha, hops[1], n, src, dst, n)
        pc.valid(got, ea, ha, src, dst, n, "fixture")
        if trans == dc.CLOSED:
            assert (got[0] == 0).all() and got[3]["n_unreachable"] == count
        else:
            fresh = ea & ~eb
            assert (got[0] > 0).all()
            for d, r in zip(got[0], got[1].astype(np.int64)):
                assert fresh[r[:d], r[1:d + 1]].any(), r[:d + 1]


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
    g = cc.synthetic(257, "medium", seed=10)
    cx = g.expected()
    qs, qd = pc.all_pairs(257)
    pc.same(run_dev(e, dev_hops(cx.hops), 257, qs, qd, max(1, cx.levels)), pc.Expected(cx.hops), qs, qd, max(1, cx.levels), "counters")
    assert (D.counters_snapshot(e) == snap).all()
    assert (D.read_counters(e) == before).all()
    D.reset_counters(e)
