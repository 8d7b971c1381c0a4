"""The reachability classes on the device: pg_reach_classes against numpy and, byte for byte including
`rounds`, against the host twin over the matrices of tests/classes_cases.py: the shapes around the launch
plan's chunk and tile, runs of several work items per workgroup, a row wider than a tile, shortened
signatures (the collision rounds), an input that is not 16-B aligned, a stream of its own over
prefilled buffers, matrix -> classes -> groups -> diff chained on the device from two engines, the
wrappers, and away from the counters.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import classes_cases as kc
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


def run_dev(e, mt, n_svc, n_src, n_dst, src=True, dst=True, reps=True, quotient=True, stream=None):
    """pg_reach_classes over prefilled outputs with guards; kc.run_host's contract on a device tensor"""
    st = stream or torch.cuda.current_stream()
    flags = kc.given(src, dst, reps, quotient)
    with torch.cuda.stream(st):
        bufs = [torch.full((n + kc.GUARD,), -1, dtype=torch.int32, device="cuda") for n in kc.sizes(n_svc, n_src, n_dst)]
    res = _capi.pg_reach_classes_result(kc.FILL, kc.FILL, kc.FILL)
    spec = kc.spec_of(mt.data_ptr() if mt.numel() else None, n_svc, n_src, n_dst)
    code = lib.pg_reach_classes(e.h, C.byref(spec), *[b.data_ptr() if f else None for b, f in zip(bufs, flags)], C.byref(res),
                                C.c_void_p(st.cuda_stream))
    assert code == 0, lib.pg_last_error(e.h)
    # (the call has synchronised its stream: no wait here before the outputs are read)
    return kc.finish([b.cpu().numpy().view(np.uint32) for b in bufs], n_svc, n_src, n_dst, flags, res)


def run(*args, **kw):
    return run_dev(engine(), *args, **kw)


def same_as_host(e, s, mt, **kw):
    """numpy, and the host twin byte for byte, `rounds` included"""
    d, h = run_dev(e, mt, *s.args(), **kw), kc.run_host(e, s.words, *s.args(), **kw)
    kc.same(d, s.want, (s.family,) + s.args())
    kc.identical(d, h, (s.family,) + s.args())
    return d


def plan():
    """the widest tile and the chunk"""
    p = engine().debug_reach_classes_plan(1 << 20)
    return p["tile_words"], p["chunk_rows"]


@pytest.mark.parametrize("family", kc.FAMILIES)
def test_synthetic(family):
    """the shapes around the chunk and the tile, with blocks_per_cu = 1 and unset"""
    e = engine()
    tw, cr = plan()
    for n_src in (1, 17, cr, cr + 1, 2 * cr + 1):
        for n_dst in (1, 16, 17, 100, 16 * tw - 1, 16 * tw, 16 * tw + 1):
            s = kc.synthetic(2 if n_dst <= 100 else 1, n_src, n_dst, family)
            mt = dev(s.words)
            assert same_as_host(e, s, mt).result["rounds"] == 1
            with e.tuning(blocks_per_cu=1):
                kc.check(run, s, words=mt, variants=(n_src, n_dst) == (cr + 1, 17))
    for mix in ("all-allow", "no-allow"):
        s = kc.synthetic(2, cr + 1, 100, family, mix)
        same_as_host(e, s, dev(s.words))


@pytest.mark.parametrize("family", ("distinct", "blocks", "near"))
def test_runs_of_several_items(family):
    """more chunks than workgroups under blocks_per_cu = 1: every workgroup of the column kernels walks a
    run of work items"""
    e = engine()
    _, cr = plan()
    s = kc.synthetic(1, 320 * cr, 33, family, seed=3)
    mt = dev(s.words)
    with e.tuning(blocks_per_cu=1):
        same_as_host(e, s, mt)
    kc.check(run, s, words=mt, variants=False)


def test_wide_row():
    """a row of 2^12 + 4 columns: two column tiles, the second with one word"""
    e = engine()
    for family in ("blocks", "near", "distinct"):
        s = kc.synthetic(2, 33, (1 << 12) + 4, family, seed=4)
        mt = dev(s.words)
        same_as_host(e, s, mt)
        with e.tuning(blocks_per_cu=1):
            kc.check(run, s, words=mt, variants=False)


@pytest.mark.parametrize("bits", (0, 1))
def test_collision_rounds(bits):
    """classes_hash_bits 0 and 1 on the device: the outputs of the 64-bit run, the host twin's rounds"""
    e = engine()
    _, cr = plan()
    for n_svc, n_src, n_dst, family in ((2, cr + 1, 100, "blocks"), (3, 40, 257, "near"), (1, 17, (1 << 12) + 4, "near")):
        s = kc.synthetic(n_svc, n_src, n_dst, family, seed=3)
        mt = dev(s.words)
        full = same_as_host(e, s, mt)
        with e.tuning(classes_hash_bits=bits):
            got = same_as_host(e, s, mt)
            one_side = same_as_host(e, s, mt, dst=False)
        for a, b in zip(got[:5], full[:5]):
            assert a.tobytes() == b.tobytes(), (family, bits)
        n_sc, n_dc = got.result["n_src_classes"], got.result["n_dst_classes"]
        assert full.result["rounds"] == 1 and 1 <= got.result["rounds"] <= max(n_sc, n_dc)
        if bits == 0:
            assert got.result["rounds"] == max(n_sc, n_dc) >= 2 and one_side.result["rounds"] == n_sc


def test_unaligned_input():
    """the input one word behind a 16-B boundary"""
    for n_src, n_dst, family in ((17, 17, "near"), (65, 100, "blocks"), (33, 4097, "dup")):
        s = kc.synthetic(2, n_src, n_dst, family, seed=6)
        kc.check(run, s, words=dev(s.words, offset=1))


def test_stream_and_prefill():
    """a non-default stream over prefilled outputs (run_dev holds the guards), every variant"""
    s = kc.synthetic(3, 130, 1000, "near", seed=7)
    mt = dev(s.words)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    kc.check(lambda *args, **kw: run(*args, stream=st, **kw), s, words=mt)


def test_garbage_in_padding():
    s = kc.synthetic(2, 65, 100, "near", seed=8)
    junk = dc.garbage(s.words.reshape(-1, kc.row_words(100)), 100).reshape(s.words.shape)
    assert (junk[:, :, -1] >> (2 * (100 & 15))).any()
    kc.identical(kc.check(run, s, words=dev(junk), variants=False), kc.run_host(engine(), s.words, *s.args()), "garbage")


def test_device_wrapper():
    """device.reach_classes against numpy"""
    e = engine()
    s = kc.synthetic(2, 65, 100, "blocks", seed=9)
    w = s.want
    sc, dcl, sr, dr, q, res = D.reach_classes(e, dev(s.words), 2, 65, 100, reps=True, quotient=True)
    u = lambda t: t.cpu().numpy().view(np.uint32)
    assert sc.dtype == torch.int32 and (u(sc) == w.src_class).all() and (u(dcl) == w.dst_class).all()
    assert (u(sr) == w.src_rep).all() and (u(dr) == w.dst_rep).all() and (u(q) == w.quotient).all()
    assert res == dict(w.result, rounds=1)
    sc, dcl, sr, dr, q, res = D.reach_classes(e, dev(s.words), 2, 65, 100, src=False)
    assert sc is None and sr is None and dr is None and q is None and (u(dcl) == w.dst_class).all()
    assert res == {"n_src_classes": 0, "n_dst_classes": w.result["n_dst_classes"], "rounds": 1}
    sc, dcl, _, _, q, res = D.reach_classes(e, dev(s.words)[:, :0].contiguous(), 2, 0, 100, quotient=True)
    assert sc.numel() == 0 and dcl.numel() == 100 and q.numel() == 0 and res == {"n_src_classes": 0, "n_dst_classes": 0, "rounds": 0}


# ---- matrix -> classes -> groups -> diff on the device, inputs from two engines ------------------
def test_fixture_change_chained():
    """the classes of the first engine's matrix are the groups under which both matrices are summed; the
    diff of the two summaries lists the class pairs the edit moved"""
    c = dc.matrix_change()
    src, dst = gc.doubled(c.src), gc.doubled(c.dst)
    n_svc, ns, nd = len(dc.SERVICES), len(src), len(dst)
    ctx = engine()   # (the context only names the device: an engine without tables)
    codes = [x.reshape(n_svc, ns, nd) for x in c.matrix_codes(src, dst)]
    mts = [D.reach_matrix(e, src, dst, dc.SERVICES) for e in (c.e0, c.e1)]
    want = kc.expected(codes[0])
    kc.same(run_dev(ctx, mts[0], n_svc, ns, nd), want, "fixture")
    kc.same(run_dev(c.e0, mts[1], n_svc, ns, nd), kc.expected(codes[1]), "fixture, after")
    sc, dcl, _, _, q, res = D.reach_classes(ctx, mts[0], n_svc, ns, nd, quotient=True)
    n_sc, n_dc = res["n_src_classes"], res["n_dst_classes"]
    sg, dg = sc.cpu().numpy().view(np.uint32), dcl.cpu().numpy().view(np.uint32)
    summaries, statuses = [], []
    for mt, cd in zip(mts, codes):
        counts, packed = D.reach_groups(ctx, mt, ns, nd, sg, dg, n_sc, n_dc, packed=True)
        wc, ws = gc.expected(cd, want.src_class, want.dst_class, n_sc, n_dc)
        assert (counts.cpu().numpy().view(np.uint64) == wc).all()
        summaries.append(packed)
        statuses.append(ws)
    # over its own matrix every class pair is uniform: one non-zero count, |cs| * |cd|, at the quotient's code
    counts = D.reach_groups(ctx, mts[0], ns, nd, sg, dg, n_sc, n_dc)[0].cpu().numpy().view(np.uint64)
    cells = np.outer(kc.class_sizes(want.src_class, n_sc), kc.class_sizes(want.dst_class, n_dc))
    codes_q = D.unpack_reach(q, n_svc, n_sc, n_dc)
    assert ((counts != 0).sum(axis=-1) == 1).all()
    assert (np.take_along_axis(counts, codes_q[..., None].astype(np.int64), axis=-1)[..., 0] == cells[None]).all()
    assert not (statuses[0] == _capi.GROUPS_SOME).any()
    b, a = (s.reshape(n_svc * n_sc, n_dc) for s in statuses)
    x = dc.Expected(b, a, dc.ALL)
    assert x.n > 0, "the edit moved no class pair"
    k, changes, trans, _ = D.reach_diff(ctx, summaries[0], summaries[1], n_dc)
    assert k == x.n and (changes.cpu().numpy().view(np.uint32) == x.entries).all() and (trans == x.trans).all()


def test_wrappers():
    """Engine.reachability_classes on the device gives what it gives on the host twins, and what the oracle
    says; one pod is listed twice on each side"""
    c = dc.matrix_change()
    for e, (ws, wd, wq) in zip((c.e0, c.e1), kc.wrapper_want(c, kc.SRC_PODS, kc.DST_PODS)):
        s, d, q = e.reachability_classes(kc.SRC_PODS, kc.DST_PODS, dc.SERVICES)
        hs, hd, hq = e.reachability_classes(kc.SRC_PODS, kc.DST_PODS, dc.SERVICES, host=True)
        assert s == hs and d == hd and (q == hq).all()
        assert s == ws and d == wd and (q == wq).all()


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
    g = kc.synthetic(2, 130, 257, "near", seed=10)
    kc.same(run_dev(e, dev(g.words), *g.args()), g.want, "counters")
    assert (D.counters_snapshot(e) == snap).all()
    assert (D.read_counters(e) == before).all()
    D.reset_counters(e)


def test_einval_and_empty_input():
    e = engine()
    w = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    res = _capi.pg_reach_classes_result(7, 7, 7)
    for what, words, spec, outs, with_result in kc.bad_calls(w.data_ptr(), out.data_ptr()):
        code = lib.pg_reach_classes(e.h, C.byref(spec) if spec is not None else None, *outs,
                                    C.byref(res) if with_result else None, None)
        assert code == _capi.PG_EINVAL and words in lib.pg_last_error(e.h).decode(), (what, code)
    assert (res.n_src_classes, res.n_dst_classes, res.rounds) == (7, 7, 7)
    for n_svc, n_src, n_dst in ((0, 5, 7), (2, 0, 7), (2, 5, 0)):
        spec = kc.spec_of(None, n_svc, n_src, n_dst)
        res = _capi.pg_reach_classes_result(7, 7, 7)
        assert lib.pg_reach_classes(e.h, C.byref(spec), *([out.data_ptr()] * 5), C.byref(res), None) == 0
        assert (res.n_src_classes, res.n_dst_classes, res.rounds) == (0, 0, 0)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all()
