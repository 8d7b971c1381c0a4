"""The port sweep on the device: pg_reach_ports against the oracle and against the host twin over the
sets, fixture variants and shapes of tests/ports_cases.py, against pg_classify(CONN) on the
materialised tuples, on a stream of its own over prefilled buffers, and away from the counters.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ports_cases as pc
import reach_cases as rc
from vpp_amd import device as D
from vpp_amd._capi import MODE_CONN

pytestmark = pytest.mark.gpu

PROTOS = (pc.TCP, pc.UDP)
ids = lambda v: {0: "tcp", 1: "udp"}.get(v, v) if isinstance(v, int) else v


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def run(e, src, dst, protocol, open_count=True, words=True, stream=None):
    out = D.reach_ports(e, src, dst, protocol, pc.SPORT, open_count=open_count, words=words, stream=stream)
    torch.cuda.synchronize()
    return (out[0],) + tuple(u32(t) for t in out[1:])


def check(e, c, n_src, n_dst):
    """all three outputs against the oracle and the host twin, then each optional output left out"""
    src, dst, want, want_open = c.shape(n_src, n_dst)
    lo, codes, n_open, words = run(e, src, dst, c.protocol)
    assert np.array_equal(lo, c.lo)
    assert (words == want).all(), pc.mismatch_report(words, want)
    assert (codes == pc.pack(want >> 30)).all(), "codes differ from the words' top two bits"
    assert (n_open == want_open).all()
    if c.K & 15:
        assert (codes[:, :, -1] >> np.uint32(2 * (c.K & 15)) == 0).all(), "padding bits set"
    h = e.debug_reach_ports_host(src, dst, c.protocol, pc.SPORT)
    assert all((a == b).all() for a, b in zip((codes, n_open, words), h[1:]))
    for oc, w in ((False, False), (True, False), (False, True)):
        got = run(e, src, dst, c.protocol, open_count=oc, words=w)[1:]
        assert (got[0] == codes).all()
        if oc:
            assert (got[1] == n_open).all()
        if w:
            assert (got[-1] == words).all()


@pytest.mark.parametrize("protocol", PROTOS, ids=ids)
@pytest.mark.parametrize("name", pc.SET_NAMES)
def test_sweep_equals_oracle(name, protocol):
    e, c = pc.set_case(name, protocol)
    check(e, c, rc.N_SRC, rc.N_DST)


@pytest.mark.parametrize("shape", pc.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ("uni", "uni-wide", "pair"))
def test_shapes(name, shape):
    e, c = pc.set_case(name, pc.TCP)
    check(e, c, *shape)


@pytest.mark.parametrize("shape", pc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_fixture_interval_tails(shape):
    """K = 1 (k16 on UDP), 16, 17 and the fixture's full K = 25 (TCP) and 14 (UDP)"""
    for name, protocol in (("k16", pc.UDP), ("k16", pc.TCP), ("k17", pc.TCP), ("full", pc.TCP), ("full", pc.UDP)):
        e, c = pc.set_case(name, protocol)
        assert c.K == {("k16", pc.UDP): 1, ("k16", pc.TCP): 16, ("k17", pc.TCP): 17}.get((name, protocol), c.K)
        check(e, c, *shape)


def test_form_b_by_knob():
    """uni under node_path = 0: the pairs through conn_q over TabEval"""
    e, c = pc.set_case("uni", pc.TCP)
    with e.tuning(node_path=0):
        check(e, c, rc.N_SRC, rc.N_DST)


def test_grid_stride_rounds():
    """129 x 257 = 33,153 pairs (no multiple of 64) under blocks_per_cu = 1: more 64-lane workgroups
    than the grid of one per CU, so lanes take several pairs"""
    e, c = pc.set_case("uni", pc.TCP)
    src, dst = pc.sides(c.t, 129, 257)
    want = pc.oracle_words(c.t.world, src, dst, pc.TCP, c.lo)
    assert want.shape[0] * want.shape[1] == 33153
    with e.tuning(blocks_per_cu=1):
        lo, codes, n_open, words = run(e, src, dst, pc.TCP)
    assert (words == want).all(), pc.mismatch_report(words, want)
    assert (codes == pc.pack(want >> 30)).all()
    assert (n_open == (((want >> 30) == pc.ALLOW) * pc.lengths(lo)).sum(axis=2)).all()


@pytest.mark.parametrize("name", ("uni", "pair"))
def test_equals_classify_device(name):
    """device against device: D.classify(CONN) on the materialised tuples (src, dst, sport, lo[k])"""
    e, c = pc.set_case(name, pc.TCP)
    src, dst, _, _ = c.shape(rc.N_SRC, rc.N_DST)
    lo, _, _, words = run(e, src, dst, pc.TCP)
    ns, nd, k = len(src), len(dst), len(lo)
    n = ns * nd * k
    b = D.TupleBatch.from_numpy(np.repeat(np.repeat(src, nd), k), np.repeat(np.tile(dst, ns), k),
                                np.full(n, pc.SPORT, np.uint16), np.tile(lo.astype(np.uint16), ns * nd),
                                np.zeros(n, np.uint8))
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    D.classify(e, MODE_CONN, -1, b, out)
    torch.cuda.synchronize()
    assert (u32(out) == words.ravel()).all()


@pytest.mark.parametrize("name,protocol,front", (("k17", pc.TCP, 4), ("uni", pc.TCP, 4), ("k16", pc.UDP, 4),
                                                 ("k16", pc.TCP, 4), ("k16", pc.TCP, 5)))
def test_stream_and_prefill(name, protocol, front):
    """a non-default stream; the three outputs inside 0xFF-filled buffers with guard words on both
    sides: padding bits zero, every word of the arrays written, the guards untouched. front: the
    guard words before the arrays -- 4 keep them 16-B aligned (K = 16: the 16-B stores of out_words),
    5 do not (K = 16 through the 4-B stores)"""
    e, c = pc.set_case(name, protocol)
    src, dst, want, want_open = c.shape(rc.N_SRC, rc.N_DST)
    ns, nd, k = len(src), len(dst), c.K
    rw = D.reach_row_words(k)
    sizes = (ns * nd * rw, ns * nd, ns * nd * k)
    spec, keep = D.ports_spec(src, dst, protocol, pc.SPORT, k)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        bufs = [torch.full((front + n + 1,), -1, dtype=torch.int32, device="cuda") for n in sizes]
        e._ck(D.lib.pg_reach_ports(e.h, C.byref(spec), *[b.data_ptr() + 4 * front for b in bufs],
                                   C.c_void_p(st.cuda_stream)))
    st.synchronize()
    del keep
    got = [u32(b) for b in bufs]
    for g, n in zip(got, sizes):
        assert (g[:front] == 0xFFFFFFFF).all() and g[front + n] == 0xFFFFFFFF, "a word outside the array was written"
    codes, n_open, words = (g[front:front + n] for g, n in zip(got, sizes))
    assert (words.reshape(ns, nd, k) == want).all()
    assert (codes.reshape(ns, nd, rw) == pc.pack(want >> 30)).all()   # (padding bits zero: pack leaves them 0)
    assert (n_open.reshape(ns, nd) == want_open).all()


def test_counters_untouched():
    import node_matrix as nm
    s = nm.node_set("uni")
    e, c = pc.set_case("uni", pc.TCP)
    assert e is s.e
    D.reset_counters(e)
    src, dst, sport, dport, proto = (a[:4099] for a in s.tup)
    b = D.TupleBatch.from_numpy(src, dst, sport, dport, proto)
    out = torch.empty(b.n, dtype=torch.int32, device="cuda")
    D.classify(e, MODE_CONN, -1, b, out, counters=D.counters_device_ptr(e))
    torch.cuda.synchronize()
    before = D.read_counters(e)
    snap = D.counters_snapshot(e)
    assert before.sum() > 0
    run(e, c.src[:rc.N_SRC], c.dst[:rc.N_DST], pc.TCP)
    assert (D.counters_snapshot(e) == snap).all()
    assert (D.read_counters(e) == before).all()
    D.reset_counters(e)


def test_same_call_twice_same_bytes():
    e, c = pc.set_case("pair", pc.UDP)
    a = run(e, c.src, c.dst, pc.UDP)
    b = run(e, c.src, c.dst, pc.UDP)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_empty_sides():
    """an empty side: PG_OK, nothing written"""
    e, c = pc.set_case("uni", pc.TCP)
    buf = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    for ns, nd in ((0, 5), (5, 0)):
        spec, keep = D.ports_spec(c.src[:ns], c.dst[:nd], pc.TCP, pc.SPORT, c.K)
        assert D.lib.pg_reach_ports(e.h, C.byref(spec), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == -1).all()
        lo, codes = D.reach_ports(e, c.src[:ns], c.dst[:nd], pc.TCP)
        assert codes.shape == (ns, nd, (c.K + 15) // 16)
        del keep


def test_open_ports_equals_host():
    """Engine.open_ports on the device == on the host twin (which tests/test_ports_host.py holds
    against the oracle's per-port actions)"""
    t = pc.topo("full")
    pods = ["ns/p%d" % k for k in range(4)] + ["ns/far"]
    for protocol in PROTOS:
        r_dev, n_dev = t.e.open_ports(pods, pods, protocol, src_port=pc.SPORT)
        r_host, n_host = t.e.open_ports(pods, pods, protocol, src_port=pc.SPORT, host=True)
        assert r_dev == r_host and (n_dev == n_host).all() and n_dev.max() > 0
