"""The reachability diff on the device: pg_reach_diff against numpy and against the host twin over the
pairs of tests/diff_cases.py, the real matrix and sweep changes from two engines, the sizes around
the launch plan's tile and chunk, inputs that are not 16-B aligned, a stream of its own over prefilled
buffers, and away from the counters.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import diff_cases as dc
import ports_cases as pc
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


def run_dev(e, bt, at, n_cols, transitions, cap, changes=True, rows=True, trans=True, stream=None):
    """pg_reach_diff over prefilled outputs; dc.run_host's contract on device tensors"""
    n_rows = bt.numel() // dc.row_words(n_cols)
    st = stream or torch.cuda.current_stream()
    with torch.cuda.stream(st):
        buf = torch.full((cap + dc.GUARD, 2), -1, dtype=torch.int32, device="cuda")
        rbuf = torch.full((n_rows + 1,), -1, dtype=torch.int32, device="cuda")
    tbuf = np.full(17, 0xFFFFFFFFFFFFFFFF, np.uint64)
    spec = _capi.pg_reach_diff_spec(bt.data_ptr(), at.data_ptr(), n_rows, n_cols, transitions, cap)
    n = C.c_uint64(dc.FILL)
    code = lib.pg_reach_diff(e.h, C.byref(spec), buf.data_ptr() if changes else None, rbuf.data_ptr() if rows else None,
                             C.byref(n), tbuf.ctypes.data_as(C.c_void_p) if trans else None, C.c_void_p(st.cuda_stream))
    assert code == 0, lib.pg_last_error(e.h)
    # (the call has synchronised its stream: no wait here before the outputs are read)
    buf, rbuf = u32(buf), u32(rbuf)
    assert rbuf[n_rows] == dc.FILL and tbuf[16] == 0xFFFFFFFFFFFFFFFF
    if not changes:
        assert (buf == dc.FILL).all()
    return n.value, buf, tbuf[:16].reshape(4, 4) if trans else None, rbuf[:n_rows] if rows else None


def run(*args, **kw):
    return run_dev(engine(), *args, **kw)


def same_as_host(bw, aw, n_cols, transitions=(dc.ALL, dc.OPENED, dc.SINGLE), offset=0):
    bt, at = dev(bw, offset), dev(aw, offset)
    for t in transitions:
        h = dc.run_host(engine(), bw, aw, n_cols, t, np.asarray(bw).size * 16)
        d = run(bt, at, n_cols, t, np.asarray(bw).size * 16)
        assert h[0] == d[0] and all(x.tobytes() == y.tobytes() for x, y in zip(h[1:], d[1:])), hex(t)
    return bt, at


@pytest.mark.parametrize("n_cols", dc.COLS)
def test_synthetic(n_cols):
    for n_rows in dc.ROWS:
        for p in dc.PS:
            b, a = dc.synthetic(n_rows, n_cols, p)
            bt, at = same_as_host(dc.pack(b), dc.pack(a), n_cols)
            dc.check(run, b, a, bt, at)


@pytest.mark.parametrize("n_cols", dc.COLS)
def test_padding_garbage(n_cols):
    for n_rows in (3, 37):
        b, a = dc.synthetic(n_rows, n_cols, 1.0 / 64, seed=2)
        bt, at = same_as_host(dc.garbage(dc.pack(b), n_cols, 3), dc.garbage(dc.pack(a), n_cols, 4), n_cols)
        dc.check(run, b, a, bt, at)


@pytest.mark.parametrize("n_cols", (1, 17, 53, 64, 1000))
def test_unaligned_inputs(n_cols):
    """both inputs one word behind a 16-B boundary: the 4-B loads"""
    for n_rows in (3, 64):
        b, a = dc.synthetic(n_rows, n_cols, 1.0 / 64, seed=5)
        bt, at = same_as_host(dc.pack(b), dc.pack(a), n_cols, offset=1)
        dc.check(run, b, a, bt, at, variants=False)
        dc.check(run, b, a, bt, dev(dc.pack(a)), transitions=(dc.ALL,), variants=False)   # one aligned, one not


def plan1(e, n_words):
    with e.tuning(blocks_per_cu=1):
        return e.debug_reach_diff_plan(n_words)


def shape_of(n_words):
    """(n_rows, n_cols) with n_rows * row_words == n_words, rows of several words where n_words has a
    small factor, and padding in every row's last word"""
    rw = next((f for f in (31, 7, 5, 3, 2) if n_words % f == 0), 1)
    return n_words // rw, 16 * rw - 3


def test_plan():
    e = engine()
    resident = plan1(e, 1 << 31)["grid"]
    for n_words in (1, 1023, 1024, 1025, 2 * resident * 1024 + 1, (1 << 32) - 1):
        p = plan1(e, n_words)
        assert p["tile_words"] == 1024 and p["chunk_words"] % 1024 == 0 and 1 <= p["grid"] <= resident
        assert p["grid"] * p["chunk_words"] >= n_words > (p["grid"] - 1) * p["chunk_words"]   # no empty workgroup
    assert plan1(e, 1025)["grid"] == 2 and plan1(e, 2 * resident * 1024 + 1)["chunk_words"] == 3 * 1024
    assert e.debug_reach_diff_plan(1 << 31)["grid"] >= resident   # blocks_per_cu caps the grid


def test_sizes_around_tile_and_chunk():
    """n_words of tile - 1, tile, tile + 1 and chunk +- 1 under blocks_per_cu = 1, chunk that of the
    launch with more tiles than workgroups"""
    e = engine()
    resident = plan1(e, 1 << 31)["grid"]
    tile, chunk = 1024, plan1(e, 2 * resident * 1024 + 1)["chunk_words"]
    for n_words in (tile - 1, tile, tile + 1, chunk - 1, chunk, chunk + 1):
        n_rows, n_cols = shape_of(n_words)
        b, a = dc.synthetic(n_rows, n_cols, 1.0 / 64, seed=6)
        bt, at = dev(dc.pack_wide(b)), dev(dc.pack_wide(a))
        with e.tuning(blocks_per_cu=1):
            dc.check(run, b, a, bt, at, transitions=(dc.ALL, dc.CLOSED), variants=n_words == tile + 1)


@pytest.mark.parametrize("p", (1.0 / 64, 1.0), ids=("sparse", "all"))
def test_more_tiles_than_workgroups(p):
    """2 * grid * tile + 1 words under blocks_per_cu = 1 (about 8 M cells): every workgroup walks
    several tiles on a running base and the last chunk is short"""
    e = engine()
    n_words = 2 * plan1(e, 1 << 31)["grid"] * 1024 + 1
    n_rows, n_cols = shape_of(n_words)
    b, a = dc.synthetic(n_rows, n_cols, p, seed=7)
    bt, at = dev(dc.pack_wide(b)), dev(dc.pack_wide(a))
    x = dc.Expected(b, a, dc.ALL)
    with e.tuning(blocks_per_cu=1):
        assert e.debug_reach_diff_plan(n_words)["chunk_words"] >= 2 * 1024
        dc.check(run, b, a, bt, at, transitions=(dc.ALL, dc.OPENED), variants=False)
        for cap in (5, x.n // 2):   # workgroups whose base is past the cap write nothing
            n, buf, trans, rows = run(bt, at, n_cols, dc.ALL, cap)
            assert n == x.n and (buf[:cap] == x.entries[:cap]).all() and (buf[cap:] == dc.FILL).all()
    n, buf, _, _ = run(bt, at, n_cols, dc.ALL, x.n, rows=False, trans=False)   # the default grid
    assert n == x.n and (buf[:x.n] == x.entries).all()


def test_stream_and_prefill():
    """a non-default stream over prefilled outputs (run_dev holds the guards)"""
    b, a = dc.synthetic(64, 1000, 1.0 / 64, seed=8)
    bt, at = dev(dc.pack(b)), dev(dc.pack(a))
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    dc.check(lambda *args, **kw: run(*args, stream=st, **kw), b, a, bt, at, transitions=(dc.ALL, dc.OPENED))


def test_device_wrapper():
    """device.reach_diff: the two-call form (cap None), an explicit cap, count only, row_changes"""
    e = engine()
    b, a = dc.synthetic(37, 53, 1.0 / 64, seed=9)
    bt, at = dev(dc.pack(b)), dev(dc.pack(a))
    x = dc.Expected(b, a, dc.CLOSED)
    n, changes, trans, rows = D.reach_diff(e, bt, at, 53, dc.CLOSED, row_changes=True)
    assert n == x.n and changes.shape == (x.n, 2) and (u32(changes) == x.entries).all()
    assert (trans == x.trans).all() and (u32(rows) == x.row_changes).all()
    row, col, cb, ca = D.unpack_changes(changes)
    assert (row == x.entries[:, 0]).all() and (col == x.entries[:, 1] & 0xFFFFF).all() and (cb == 2).all() and (ca != 2).all()
    n, changes, _, rows = D.reach_diff(e, bt, at, 53, dc.CLOSED, cap=3)
    assert n == x.n and (u32(changes) == x.entries[:3]).all() and rows is None
    n, changes, _, _ = D.reach_diff(e, bt, at, 53, dc.CLOSED, cap=0)
    assert n == x.n and changes.shape == (0, 2)
    n, changes, trans, rows = D.reach_diff(e, bt[:0], at[:0], 53, row_changes=True)
    assert n == 0 and changes.shape == (0, 2) and (trans == 0).all() and rows.numel() == 0


def test_einval_and_no_rows():
    e = engine()
    w = torch.zeros(4, dtype=torch.int32, device="cuda")
    ptr, S = w.data_ptr(), _capi.pg_reach_diff_spec
    n = C.c_uint64(dc.FILL)
    bad = [(None, True), (S(None, ptr, 1, 16, dc.ALL, 0), True), (S(ptr, None, 1, 16, dc.ALL, 0), True),
           (S(ptr, ptr, 1, 16, dc.ALL, 0), False), (S(ptr, ptr, 1, 0, dc.ALL, 0), True),
           (S(ptr, ptr, 1, (1 << 20) + 1, dc.ALL, 0), True), (S(ptr, ptr, 1 << 32, 16, dc.ALL, 0), True),
           (S(ptr, ptr, 1 << 31, 32, dc.ALL, 0), True)]
    for spec, with_n in bad:
        code = lib.pg_reach_diff(e.h, C.byref(spec) if spec is not None else None, None, None,
                                 C.byref(n) if with_n else None, None, None)
        assert code == _capi.PG_EINVAL and lib.pg_last_error(e.h), (spec, code)
    buf = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    trans = np.full(16, 7, np.uint64)
    code = lib.pg_reach_diff(e.h, C.byref(S(ptr, ptr, 0, 16, dc.ALL, 4)), buf.data_ptr(), buf.data_ptr(), C.byref(n),
                             trans.ctypes.data_as(C.c_void_p), None)
    torch.cuda.synchronize()
    assert code == 0 and n.value == 0 and (trans == 0).all() and (buf.cpu().numpy() == -1).all()


# ---- real changes, inputs from two engines ----------------------------------------------------
def test_matrix_change_two_engines():
    c = dc.matrix_change()
    bt = D.reach_matrix(c.e0, c.src, c.dst, dc.SERVICES)
    at = D.reach_matrix(c.e1, c.src, c.dst, dc.SERVICES)
    torch.cuda.synchronize()
    assert (u32(bt).reshape(-1, bt.shape[-1]) == dc.pack(c.b)).all() and (u32(at).reshape(-1, at.shape[-1]) == dc.pack(c.a)).all()
    for e in (c.e1, c.e0, engine()):   # the context only names the device
        dc.check(lambda *args, **kw: run_dev(e, *args, **kw), c.b, c.a, bt, at, variants=e is c.e1)
    assert run_dev(c.e1, bt, at, dc.N_DST, dc.OPENED, 0)[0] == dc.MATRIX_WANT["opened"]
    assert run_dev(c.e1, bt, at, dc.N_DST, dc.CLOSED, 0)[0] == dc.MATRIX_WANT["closed"]
    same_as_host(u32(bt), u32(at), dc.N_DST)


@pytest.mark.parametrize("transitions", (dc.ALL, dc.OPENED, dc.CLOSED), ids=("all", "opened", "closed"))
def test_reachability_diff(transitions):
    c = dc.matrix_change()
    got, trans = c.e1.reachability_diff(c.e0, dc.PODS, dc.PODS, dc.SERVICES, transitions)
    want = dc.pod_tuples(c, transitions)
    assert want and got == want
    host, trans_h = c.e1.reachability_diff(c.e0, dc.PODS, dc.PODS, dc.SERVICES, transitions, host=True)
    assert got == host and (trans == trans_h).all()


@pytest.mark.parametrize("protocol", (pc.TCP, pc.UDP), ids=("tcp", "udp"))
def test_sweep_change(protocol):
    c = dc.sweep_change()
    w = dc.SWEEP_WANT[protocol]
    b, a = c.codes[protocol]
    assert dc.Expected(b, a, dc.ALL).n == w["changed"]
    lo0, bt = D.reach_ports(c.e0, c.src, c.dst, protocol, pc.SPORT)
    lo1, at = D.reach_ports(c.e1, c.src, c.dst, protocol, pc.SPORT)
    torch.cuda.synchronize()
    assert np.array_equal(lo0, lo1) and len(lo0) == w["K"]
    dc.check(lambda *args, **kw: run_dev(c.e1, *args, **kw), b, a, bt, at)
    same_as_host(u32(bt), u32(at), w["K"])
    if protocol == pc.UDP:
        n, _, trans, rows = run_dev(c.e1, bt, at, w["K"], dc.ALL, 0)
        assert n == 0 and (rows == 0).all() and (trans == np.diag(np.diag(trans))).all()


def test_counters_untouched():
    """the counters and their snapshots are bit-identical before and after a diff on that context"""
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
    b, a = dc.synthetic(64, 1000, 1.0, seed=10)
    n, _, _, _ = run_dev(e, dev(dc.pack(b)), dev(dc.pack(a)), 1000, dc.ALL, b.size)
    assert n == b.size
    assert (D.counters_snapshot(e) == snap).all()
    assert (D.read_counters(e) == before).all()
    D.reset_counters(e)
