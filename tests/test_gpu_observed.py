"""The observed reachability on the device: pg_reach_observed against numpy and, byte for byte, against the
host twin over the scenarios of tests/observed_cases.py -- the row and word edges with the flow-count
edges, a full grid of the plan plus one flow, flow arrays and out_flow off their alignment, the address and
service edges, lists chosen with the probe, contention under every observed_test_first, the address tables
in LDS and in HBM and around the largest side that is staged, split launches, accumulation -- and a stream
of its own, matrix / observed -> diff -> groups chained on the device, the wrapper, every PG_EINVAL, the
empty cases, and away from the counters and the compiler.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import diff_cases as dc
import groups_cases as gc
import observed_cases as oc
import ports_cases as pc
from vpp_amd import _capi
from vpp_amd import device as D
from vpp_amd import renderer as R
from vpp_amd._capi import MODE_CONN, lib

pytestmark = pytest.mark.gpu

TORCH = {np.dtype(np.uint32): (torch.int32, np.int32), np.dtype(np.uint16): (torch.int16, np.int16),
         np.dtype(np.uint8): (torch.uint8, np.uint8)}


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


def dev(a, offset=0):
    """a numpy array -> a device tensor that starts `offset` elements behind a fresh allocation"""
    tt, nt = TORCH[a.dtype]
    t = torch.empty(len(a) + offset, dtype=tt, device="cuda")
    t[offset:] = torch.from_numpy(np.ascontiguousarray(a).view(nt)).cuda()
    assert t[offset:].data_ptr() % 16 == (a.itemsize * offset) % 16
    return t[offset:]


def run_dev(e, c, into=None, flow=True, svc=True, sport=None, offsets=(0, 0, 0, 0, 0), stream=None):
    """pg_reach_observed over prefilled outputs with guards, out_flow from an odd byte; oc.run_host's contract"""
    st = stream or torch.cuda.current_stream()
    keep = []
    spec = oc.spec_of(c, oc.flags_of(c, into), keep)
    n, nw, nv = len(c.flows[0]), oc.n_words(c), len(c.services)
    with torch.cuda.stream(st):
        fl = [dev(a, o) for a, o in zip(c.flows, offsets)]
        packed = torch.full((nw + oc.GUARD,), -1, dtype=torch.int32, device="cuda")
        if into is not None:
            packed[:nw] = torch.from_numpy(np.ascontiguousarray(into, np.uint32).view(np.int32).ravel()).cuda()
        fbuf = torch.full((n + oc.GUARD + 1,), 0xEE, dtype=torch.uint8, device="cuda")
        sbuf = torch.from_numpy(np.full(nv + oc.GUARD, 0xEEEEEEEEEEEEEEEE, np.uint64).view(np.int64)).cuda()
    assert fbuf[1:].data_ptr() % 2 == 1
    res = _capi.pg_reach_observed_result(7, 7, 7, 7, 7)
    with_sport = c.match if sport is None else sport
    soa = _capi.pg_tuple_soa(*[t.data_ptr() if (i != 2 or with_sport) else None for i, t in enumerate(fl)])
    code = lib.pg_reach_observed(e.h, C.byref(spec), C.byref(soa) if n else None, n, packed.data_ptr(),
                                 fbuf[1:].data_ptr() if flow else None, sbuf.data_ptr() if svc else None, C.byref(res),
                                 C.c_void_p(st.cuda_stream))
    assert code == 0, lib.pg_last_error(e.h)
    # (the call has synchronised its stream: no wait here before the outputs are read)
    return oc.finish(c, packed.cpu().numpy().view(np.uint32), fbuf[1:].cpu().numpy(), sbuf.cpu().numpy().view(np.uint64),
                     res, flow, svc)


def run(c, **kw):
    """the device, and the host twin byte for byte"""
    d = run_dev(engine(), c, **kw)
    host_kw = {k: v for k, v in kw.items() if k in ("into", "flow", "svc", "sport")}
    oc.identical(d, oc.run_host(engine(), c, **host_kw), "host twin")
    return d


@pytest.mark.parametrize("n_dst", oc.N_DST)
def test_rows_and_words(n_dst):
    oc.rows_and_words(run, engine(), n_dst)


def test_full_grid():
    oc.full_grid(run, engine())


def test_alignment():
    """each flow array in turn one element behind a fresh allocation, then all of them; out_flow always
    starts at an odd byte (run_dev)"""
    for match in (False, True):
        c = oc.random_case(65, 33, 3, 5000, seed=1, match=match)
        oc.assert_inputs(c)
        base = oc.check(run, c, "aligned")
        for k in range(5):
            if k == 2 and not match:
                continue   # (src_port is not read)
            off = tuple(int(i == k) for i in range(5))
            oc.identical(oc.check(run, c, ("offset", k), offsets=off), base, ("offset", k))
        oc.identical(oc.check(run, c, "all offset", offsets=(1, 1, 1, 1, 1)), base, "all offset")


def test_address_edges():
    oc.address_edges(run, engine())


def test_collisions():
    e = engine()
    oc.collisions(run, e)
    with e.tuning(observed_lds_bytes=0):
        oc.collisions(run, e)


def test_service_edges():
    oc.service_edges(run, engine())


def test_many_services():
    oc.many_services(run, engine())


def test_contention():
    oc.contention(run, engine())


def test_table_paths():
    oc.table_paths(run, engine())


def test_split_launches():
    oc.split_launches(run, engine())


def test_accumulate():
    oc.accumulate(run, engine())


def test_stream_and_prefill():
    """a non-default stream over prefilled buffers (run_dev holds the guards), every variant"""
    c = oc.random_case(65, 33, 3, 20000, seed=1)
    oc.assert_inputs(c)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    oc.check(lambda c, **kw: run(c, stream=st, **kw), c, "stream", variants=True)


def test_chained_on_the_device():
    """pg_reach_matrix (allowed) and pg_reach_observed over pg_gen_tuples flows with the end points as the
    address pool, then pg_reach_diff CLOSED (allowed, unused) and OPENED (seen, not allowed) and
    pg_reach_groups over the observed matrix: against numpy on the two matrices"""
    e, _, _ = pc.fixture("full")
    src, dst = pc.sides(dc._Side, 37, 53)
    svc = dc.SERVICES
    nv, ns, nd = len(svc), len(src), len(dst)
    allowed = D.reach_matrix(e, src, dst, svc)
    gen = D.counter_layout_gen(e)
    b = D.TupleBatch(1 << 16)
    D.gen_tuples(e, b, seed=11, ip_pool=np.unique(np.concatenate([src, dst])), pool_pct=85, dst_pool_pct=85,
                 port_pool=sorted({s[2] for s in svc}), port_pool_pct=85, tcp_pct=55, udp_pct=30)
    observed, flow, counts, res = e.reach_observed(src, dst, svc, b, flow=True, svc_flows=True)
    assert D.counter_layout_gen(e) == gen
    c = oc.case(src, dst, svc, b.numpy())
    w = oc.expected(c)
    assert min(w.result["n_matched"], w.result["n_no_src"], w.result["n_no_dst"], w.result["n_no_svc"]) > 0
    u = lambda t, dt=np.uint32: t.cpu().numpy().view(dt)
    assert (u(observed) == w.packed).all() and (u(flow, np.uint8) == w.flow).all() and (u(counts, np.uint64) == w.svc_flows).all()
    assert res == w.result
    a_codes, o_codes = D.unpack_reach(allowed, nv, ns, nd), D.unpack_reach(observed, nv, ns, nd)
    for t in (dc.CLOSED, dc.OPENED):
        x = dc.Expected(a_codes.reshape(nv * ns, nd), o_codes.reshape(nv * ns, nd), t)
        k, changes, trans, _ = D.reach_diff(e, allowed, observed, nd, t)
        assert k == x.n > 0 and (u(changes) == x.entries).all() and (trans == x.trans).all(), (t, k, x.n)
    sg, dg = (np.arange(ns) % 4).astype(np.uint32), (np.arange(nd) % 5).astype(np.uint32)
    want_counts, _ = gc.expected(o_codes, sg, dg, 4, 5)
    got_counts, _ = D.reach_groups(e, observed, ns, nd, sg, dg, 4, 5)
    assert (u(got_counts, np.uint64) == want_counts).all() and want_counts[..., oc.ALLOW].sum() == w.result["n_cells"]


def test_device_wrapper():
    """device.reach_observed against numpy: a fresh matrix, then a second batch into it"""
    e = engine()
    c = oc.random_case(65, 33, 3, 8192, seed=1, match=True)
    u = lambda t, dt=np.uint32: t.cpu().numpy().view(dt)
    halves = [oc.part(c, 0, 4096), oc.part(c, 4096, 8192)]
    b = [D.TupleBatch.from_numpy(*h.flows[:2], h.flows[2], h.flows[3], h.flows[4]) for h in halves]
    w0 = oc.expected(halves[0])
    packed, flow, counts, res = D.reach_observed(e, c.src, c.dst, c.services, b[0], match_src_port=True, flow=True, svc_flows=True)
    assert packed.dtype == torch.int32 and (u(packed) == w0.packed).all() and (u(flow, np.uint8) == w0.flow).all()
    assert (u(counts, np.uint64) == w0.svc_flows).all() and res == w0.result
    w1 = oc.expected(halves[1], into=w0.packed)
    again, flow, counts, res = D.reach_observed(e, c.src, c.dst, c.services, b[1], match_src_port=True, into=packed)
    assert again is packed and flow is None and counts is None and (u(packed) == w1.packed).all() and res == w1.result
    assert (w1.packed == oc.expected(c).packed).all()
    empty, _, _, res = D.reach_observed(e, c.src[:0], c.dst, c.services, b[0])
    assert empty.numel() == 0 and res == dict.fromkeys(res, 0)


def test_counters_and_compiler_untouched():
    """the counters and their snapshots are bit-identical before and after a call on that context, and its
    layout generation stays: nothing was compiled"""
    import node_matrix as nm
    s = nm.node_set("uni")
    e = s.e
    D.reset_counters(e)
    src, dst, sport, dport, proto = (x[:4099] for x in s.tup)
    t = D.TupleBatch.from_numpy(src, dst, sport, dport, proto)
    out = torch.empty(t.n, dtype=torch.int32, device="cuda")
    D.classify(e, MODE_CONN, -1, t, out, counters=D.counters_device_ptr(e))
    torch.cuda.synchronize()
    before, snap, gen = D.read_counters(e), D.counters_snapshot(e), D.counter_layout_gen(e)
    assert before.sum() > 0
    c = oc.random_case(65, 33, 3, 8192, seed=1)
    oc.same(run_dev(e, c), oc.expected(c), "counters")
    assert D.counter_layout_gen(e) == gen
    assert (D.counters_snapshot(e) == snap).all()
    assert (D.read_counters(e) == before).all()
    D.reset_counters(e)


def test_einval_and_empty():
    e = engine()
    c = oc.random_case(5, 7, 2, 64, seed=1)
    out = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    fl = [dev(a) for a in c.flows]

    def call(spec, soa, n, packed, res):
        return lib.pg_reach_observed(e.h, C.byref(spec) if spec is not None else None, C.byref(soa) if soa is not None else None,
                                     n, packed, None, None, C.byref(res) if res is not None else None, None)

    oc.einval(call, e, c, out.data_ptr(), [t.data_ptr() for t in fl])
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all()
    oc.empties(run, e)
