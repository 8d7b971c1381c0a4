"""The reachability groups on the device: pg_reach_groups against numpy and, byte for byte, against the
host twin over the matrices and groupings of tests/groups_cases.py, the shapes around the launch plan's
chunk and tile, runs of several work items per workgroup, the largest accumulators, an input that is
not 16-B aligned, a stream of its own over prefilled buffers, matrix -> groups -> diff chained on the
device from two engines, the wrappers, and away from the counters.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import diff_cases as dc
import groups_cases as gc
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


def run_dev(e, mt, n_svc, n_src, n_dst, sg, dg, n_sg, n_dg, packed=True, stream=None):
    """pg_reach_groups over prefilled outputs with guards; gc.run_host's contract on a device tensor"""
    st = stream or torch.cuda.current_stream()
    hc, hp = gc.buffers(n_svc, n_sg, n_dg)
    with torch.cuda.stream(st):
        cbuf = torch.full((len(hc),), -1, dtype=torch.int64, device="cuda")
        pbuf = torch.full((len(hp),), -1, dtype=torch.int32, device="cuda")
    spec, keep = gc.spec_of(mt.data_ptr() if mt.numel() else None, n_svc, n_src, n_dst, sg, dg, n_sg, n_dg)
    code = lib.pg_reach_groups(e.h, C.byref(spec), cbuf.data_ptr(), pbuf.data_ptr() if packed else None,
                               C.c_void_p(st.cuda_stream))
    assert code == 0, lib.pg_last_error(e.h)
    # (the call has synchronised its stream: no wait here before the outputs are read)
    return gc.finish(cbuf.cpu().numpy().view(np.uint64), pbuf.cpu().numpy().view(np.uint32), n_svc, n_sg, n_dg, packed)


def run(*args, **kw):
    return run_dev(engine(), *args, **kw)


def same_as_host(e, s, mt):
    """numpy, and the host twin byte for byte"""
    d, h = run_dev(e, mt, *s.args()), gc.run_host(e, s.words, *s.args())
    gc.same(d, s.want, (s.n_svc, s.n_src, s.n_dst))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(h, d)), (s.n_svc, s.n_src, s.n_dst)


def plan():
    """the widest tile and the chunk"""
    p = engine().debug_reach_groups_plan(1 << 20)
    return p["tile_words"], p["chunk_rows"]


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_synthetic(family):
    """the shapes around the chunk and the tile, with blocks_per_cu = 1 and unset"""
    e = engine()
    tw, cr = plan()
    for n_src in (1, 17, cr, cr + 1, 2 * cr + 1):
        for n_dst in (1, 16, 17, 100, 16 * tw - 1, 16 * tw, 16 * tw + 1):
            s = gc.synthetic(2 if n_dst <= 100 else 1, n_src, n_dst, family)
            mt = dev(s.words)
            same_as_host(e, s, mt)
            with e.tuning(blocks_per_cu=1):
                gc.check(run, s, words=mt, variants=(n_src, n_dst) == (cr + 1, 17))
    for mix in ("all-allow", "no-allow"):
        s = gc.synthetic(2, cr + 1, 100, family, mix)
        same_as_host(e, s, dev(s.words))


@pytest.mark.parametrize("family", ("one", "blocks", "random", "skewed"))
def test_runs_of_several_items(family):
    """more chunks than workgroups under blocks_per_cu = 1: a workgroup keeps its accumulators across the
    chunks of one (service, src group) and hands them over when the pair changes"""
    e = engine()
    _, cr = plan()
    s = gc.synthetic(2, 320 * cr, 33, family, seed=3)
    mt = dev(s.words)
    with e.tuning(blocks_per_cu=1):
        same_as_host(e, s, mt)
    gc.check(run, s, words=mt, variants=False)


def test_largest_accumulators():
    """4096 dst groups over 4100 dst (identity, four of them doubled), and 4096 src groups"""
    e = engine()
    s = gc.synthetic(1, 33, 4100, "identity", seed=4)
    assert s.n_dg == 4096 and (s.dg[4096:] == np.arange(4)).all()
    same_as_host(e, s, dev(s.words))
    s = gc.synthetic(1, 4096, 33, "identity", seed=5)
    assert s.n_sg == 4096 and s.n_dg == 33
    mt = dev(s.words)
    same_as_host(e, s, mt)
    with e.tuning(blocks_per_cu=1):
        gc.check(run, s, words=mt, variants=False)


def test_unaligned_input():
    """the input one word behind a 16-B boundary"""
    for n_src, n_dst, family in ((17, 17, "random"), (65, 100, "blocks"), (33, 4097, "skewed")):
        s = gc.synthetic(2, n_src, n_dst, family, seed=6)
        gc.check(run, s, words=dev(s.words, offset=1))


def test_stream_and_prefill():
    """a non-default stream over prefilled outputs (run_dev holds the guards), with and without out_packed"""
    s = gc.synthetic(3, 130, 1000, "random", seed=7)
    mt = dev(s.words)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    gc.check(lambda *args, **kw: run(*args, stream=st, **kw), s, words=mt)


def test_garbage_in_padding():
    s = gc.synthetic(2, 65, 100, "random", seed=8)
    junk = dc.garbage(s.words.reshape(-1, gc.row_words(100)), 100).reshape(s.words.shape)
    gc.check(run, s, words=dev(junk), variants=False)


def test_device_wrapper():
    """device.reach_groups and unpack_groups"""
    e = engine()
    s = gc.synthetic(2, 65, 100, "blocks", seed=9)
    counts, packed = D.reach_groups(e, dev(s.words), 65, 100, s.sg, s.dg, s.n_sg, s.n_dg, packed=True)
    assert counts.dtype == torch.int64 and (counts.cpu().numpy().view(np.uint64) == s.want[0]).all()
    assert (D.unpack_groups(packed, s.n_dg) == s.want[1]).all()
    counts, packed = D.reach_groups(e, dev(s.words), 65, 100, s.sg, s.dg, s.n_sg, s.n_dg)
    assert packed is None and (counts.cpu().numpy().view(np.uint64) == s.want[0]).all()
    counts, packed = D.reach_groups(e, dev(s.words)[:, :0].contiguous(), 0, 100, s.sg[:0], s.dg, 2, s.n_dg, packed=True)
    assert not counts.cpu().numpy().any() and (D.unpack_groups(packed, s.n_dg) == _capi.GROUPS_EMPTY).all()


# ---- matrix -> groups -> diff on the device, inputs from two engines ---------------------------
def test_fixture_change_chained():
    c = dc.matrix_change()
    src, dst = gc.doubled(c.src), gc.doubled(c.dst)
    sg, n_sg, dg, n_dg = gc.fixed_groups(len(src), len(dst))
    n_svc = len(dc.SERVICES)
    summaries, statuses = [], []
    # (the context only names the device: the other engine's, and an engine without tables)
    for e, codes, ctx in zip((c.e0, c.e1), c.matrix_codes(src, dst), (c.e1, engine())):
        mt = D.reach_matrix(e, src, dst, dc.SERVICES)
        want = gc.expected(codes.reshape(n_svc, len(src), len(dst)), sg, dg, n_sg, n_dg)
        gc.same(run_dev(ctx, mt, n_svc, len(src), len(dst), sg, dg, n_sg, n_dg), want, "fixture")
        summaries.append(D.reach_groups(ctx, mt, len(src), len(dst), sg, dg, n_sg, n_dg, packed=True)[1])
        statuses.append(want[1])
    b, a = (s.reshape(n_svc * n_sg, n_dg) for s in statuses)
    x = dc.Expected(b, a, dc.ALL)
    assert x.n > 0, "the edit moved no group pair"
    k, changes, trans, _ = D.reach_diff(engine(), summaries[0], summaries[1], n_dg)
    assert k == x.n and (changes.cpu().numpy().view(np.uint32) == x.entries).all()
    assert (trans == x.trans).all() and int(trans.sum()) == n_svc * n_sg * n_dg


def test_wrappers():
    """the wrappers on the device give what they give on the host twins, and what the oracle says; ns/p0
    sits in two src groups, ns/p1 in two dst groups"""
    c = dc.matrix_change()
    (cb, sb), (ca, sa) = gc.wrapper_want(c)
    for e, wc, ws in ((c.e0, cb, sb), (c.e1, ca, sa)):
        counts, status = e.reachability_groups(gc.SRC_GROUPS, gc.DST_GROUPS, dc.SERVICES)
        hc, hs = e.reachability_groups(gc.SRC_GROUPS, gc.DST_GROUPS, dc.SERVICES, host=True)
        assert counts.dtype == np.uint64 and (counts == hc).all() and (status == hs).all()
        assert (counts == wc).all() and (status == ws).all()
    got = c.e1.reachability_groups_diff(c.e0, gc.SRC_GROUPS, gc.DST_GROUPS, dc.SERVICES)
    assert got and got == c.e1.reachability_groups_diff(c.e0, gc.SRC_GROUPS, gc.DST_GROUPS, dc.SERVICES, host=True)
    assert got == gc.diff_want(sb, sa)


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
    g = gc.synthetic(2, 130, 257, "random", seed=10)
    gc.same(run_dev(e, dev(g.words), *g.args()), g.want, "counters")
    assert (D.counters_snapshot(e) == snap).all()
    assert (D.read_counters(e) == before).all()
    D.reset_counters(e)


def test_einval_and_empty_sides():
    e = engine()
    w = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.full((64,), -1, dtype=torch.int64, device="cuda")
    *keep, bad = gc.bad_specs(w.data_ptr())
    for what, spec, with_counts in bad:
        code = lib.pg_reach_groups(e.h, C.byref(spec) if spec is not None else None, out.data_ptr() if with_counts else None,
                                   out.data_ptr(), None)
        assert code == _capi.PG_EINVAL and lib.pg_last_error(e.h), (what, code)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all()
    for n_svc, n_src, n_dst in ((2, 0, 7), (2, 5, 0)):
        sg, dg = np.zeros(n_src, np.uint32), np.zeros(n_dst, np.uint32)
        counts, words = run(w[:0], n_svc, n_src, n_dst, sg, dg, 3, 18)
        assert not counts.any() and (D.unpack_groups(words, 18) == _capi.GROUPS_EMPTY).all() and (words[:, :, 1] == 0xF).all()
        spec, keep2 = gc.spec_of(None, n_svc, n_src, n_dst, sg, dg, 0, 3)   # no group either: nothing is written
        assert lib.pg_reach_groups(e.h, C.byref(spec), out.data_ptr(), out.data_ptr(), None) == 0
    spec, keep2 = gc.spec_of(None, 0, 5, 7, np.zeros(5, np.uint32), np.zeros(7, np.uint32), 3, 18)
    assert lib.pg_reach_groups(e.h, C.byref(spec), out.data_ptr(), out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all()
