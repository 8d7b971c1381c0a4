"""The reachability classes on the host (no GPU): pg_debug_reach_classes_host running the per-word code,
signatures, rounds and plan of pg_reach_classes (classes.hpp, the functions the kernels and the launch
call) against numpy on the synthetic matrices of tests/classes_cases.py, under shortened signatures
(the collision rounds), chained into the groups and diff twins, and against numpy on the oracle's codes
for real engines: the fixture change of tests/diff_cases.py and four node_matrix topologies.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import classes_cases as kc
import closure_cases as cc
import diff_cases as dc
import groups_cases as gc
from vpp_amd import _capi
from vpp_amd import device as D
from vpp_amd import renderer as R
from vpp_amd._capi import lib


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


def run(*args, **kw):
    return kc.run_host(engine(), *args, **kw)


def plan():
    """the widest tile and the chunk"""
    p = engine().debug_reach_classes_plan(1 << 20)
    return p["tile_words"], p["chunk_rows"]


def test_plan():
    e = engine()
    for n_dst in (1, 16, 17, 100, 1000, 4096, 4097, 1 << 20):
        p = e.debug_reach_classes_plan(n_dst)
        t = p["tile_words"]
        assert p["chunk_rows"] >= p["check_rows"] >= 1 and 1 <= t <= 256 and t & (t - 1) == 0, (n_dst, p)
        assert t >= min(256, kc.row_words(n_dst)), (n_dst, p)


@pytest.mark.parametrize("code_mix", kc.MIXES)
@pytest.mark.parametrize("family", kc.FAMILIES)
def test_synthetic(family, code_mix):
    """every family x mix at the sides around the chunk and the tile; one slice and three"""
    tw, cr = plan()
    for n_svc in (1, 3):
        for n_src in (1, 2, 17, cr, cr + 1, 2 * cr + 1):
            for n_dst in (1, 15, 16, 17, 100, 16 * tw - 1, 16 * tw, 16 * tw + 1):
                got = kc.check(run, kc.synthetic(n_svc, n_src, n_dst, family, code_mix), variants=n_dst in (17, 100))
                assert got.result["rounds"] == 1


@pytest.mark.parametrize("family", kc.FAMILIES)
def test_garbage_in_padding(family):
    """random bits in the padding of every row's last word change nothing"""
    for n_dst in (1, 15, 17, 33, 100, 1000):
        s = kc.synthetic(2, 37, n_dst, family, seed=2)
        junk = dc.garbage(s.words.reshape(-1, kc.row_words(n_dst)), n_dst).reshape(s.words.shape)
        assert (junk[:, :, -1] >> (2 * (n_dst & 15))).any(), "no garbage in the padding"
        kc.identical(kc.check(run, s, words=junk, variants=False), run(s.words, *s.args()), (family, n_dst))


def test_rows_that_differ_in_padding_only():
    """two rows (and so all columns' cells of them) equal in every valid cell, different padding: one class"""
    codes = np.array([[[0, 2, 3], [0, 2, 3], [1, 2, 3]]], np.uint8)   # 1 x 3 x 3
    words = kc.pack3(codes)
    words[0, 1, 0] |= 0xABCDEF << 6
    got = run(words, 1, 3, 3)
    assert got.src_class.tolist() == [0, 0, 1] and got.dst_class.tolist() == [0, 1, 2] and got.src_rep.tolist() == [0, 2]
    assert got.quotient.tolist() == [[[0 | 2 << 2 | 3 << 4], [1 | 2 << 2 | 3 << 4]]]


# ---- collisions ----------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ("blocks", "near"))
def test_collision_rounds(family):
    """classes_hash_bits 64, 2, 1 and 0: the same outputs; one round at 64; with every signature equal (0)
    a round per class of the side that has most"""
    e = engine()
    _, cr = plan()
    for n_svc, n_src, n_dst, mix in ((1, 17, 100, "uniform"), (2, cr + 1, 33, "no-allow"), (3, 40, 257, "uniform"),
                                     (2, 33, 17, "all-allow")):
        s = kc.synthetic(n_svc, n_src, n_dst, family, mix, seed=3)
        n_sc, n_dc = s.want.result["n_src_classes"], s.want.result["n_dst_classes"]
        assert max(n_sc, n_dc) <= 40
        full = kc.check(run, s, variants=False)
        assert full.result["rounds"] == 1
        seen = []
        for bits in (2, 1, 0):
            with e.tuning(classes_hash_bits=bits):
                got = kc.check(run, s, variants=bits == 0)
                only_src, only_dst = run(s.words, *s.args(), dst=False), run(s.words, *s.args(), src=False)
            for a, b in zip(got[:5], full[:5]):
                assert a.tobytes() == b.tobytes(), (family, bits)
            r = got.result["rounds"]
            assert r == max(only_src.result["rounds"], only_dst.result["rounds"])
            assert 1 <= only_src.result["rounds"] <= n_sc and 1 <= only_dst.result["rounds"] <= n_dc
            if bits == 0:   # one bucket: every class but the first costs a round
                assert only_src.result["rounds"] == n_sc and only_dst.result["rounds"] == n_dc
                assert r >= 2 or max(n_sc, n_dc) == 1
            seen.append(r)
        assert seen[0] <= seen[1] <= seen[2], seen   # (fewer bits merge buckets)
        assert e.get_tuning("classes_hash_bits") == 64


# ---- the chain -----------------------------------------------------------------------------------
def test_chain_groups_and_diff():
    """the groups twin over the class arrays: for every (v, cs, cd) one non-zero count, |cs| * |cd|, at
    the code the quotient holds; the diff twin over two quotients of equal class counts"""
    e = engine()
    s = kc.synthetic(3, 65, 100, "near", seed=4)
    got = kc.check(run, s, variants=False)
    n_sc, n_dc = got.result["n_src_classes"], got.result["n_dst_classes"]
    counts, status = gc.run_host(e, s.words, 3, 65, 100, got.src_class, got.dst_class, n_sc, n_dc)
    q = D.unpack_reach(got.quotient, 3, n_sc, n_dc)
    cells = np.outer(kc.class_sizes(got.src_class, n_sc), kc.class_sizes(got.dst_class, n_dc))
    assert ((counts != 0).sum(axis=-1) == 1).all()
    assert (np.take_along_axis(counts, q[..., None].astype(np.int64), axis=-1)[..., 0] == cells[None]).all()
    # another matrix with the same classes: every code moved by one
    t_codes = (s.codes + 1) & 3
    other = run(kc.pack3(t_codes), *s.args())
    assert other.result == got.result and (other.src_class == got.src_class).all()
    x = dc.Expected(q.reshape(3 * n_sc, n_dc), D.unpack_reach(other.quotient, 3, n_sc, n_dc).reshape(3 * n_sc, n_dc), dc.ALL)
    assert x.n == 3 * n_sc * n_dc
    n, buf, trans, rows = dc.run_host(e, got.quotient, other.quotient, n_dc, dc.ALL, x.n)
    assert n == x.n and (buf[:x.n] == x.entries).all() and (trans == x.trans).all() and (rows == x.row_changes).all()


# ---- real engines ------------------------------------------------------------------------------
def test_fixture_change():
    """both engines of the fixture change, one end point of each side listed twice, against the oracle"""
    c = dc.matrix_change()
    src, dst = gc.doubled(c.src), gc.doubled(c.dst)
    n_svc = len(dc.SERVICES)
    counts = []
    for e, codes in zip((c.e0, c.e1), c.matrix_codes(src, dst)):
        want = kc.expected(codes.reshape(n_svc, len(src), len(dst)))
        assert 1 < want.result["n_src_classes"] < len(src) and 1 < want.result["n_dst_classes"] < len(dst)
        assert want.src_class[-1] == want.src_class[0] and want.dst_class[-1] == want.dst_class[0]   # the doubled ones
        m = e.debug_reach_matrix_host(src, dst, dc.SERVICES, words=False)
        got = kc.run_host(e, m, n_svc, len(src), len(dst))
        kc.same(got, want, "fixture")
        assert got.result["rounds"] == 1
        counts.append(want.result)
    assert counts[0] != counts[1], "the edit moved no class"


@pytest.mark.parametrize("name", sorted(cc.TOPOLOGY_WANT))
def test_topology(name):
    import node_matrix as nm
    e, ips, svc, _ = cc.topology(name)
    ends = gc.doubled(ips)
    want = kc.expected(cc.oracle_codes(nm.topo(name).world, ends, svc))
    assert want.result["n_src_classes"] > 1 and want.src_class[-1] == 0
    m = e.debug_reach_matrix_host(ends, ends, svc, words=False)
    kc.same(kc.run_host(e, m, len(svc), len(ends), len(ends)), want, name)


def test_wrapper_host():
    c = dc.matrix_change()
    for e, (ws, wd, wq) in zip((c.e0, c.e1), kc.wrapper_want(c, kc.SRC_PODS, kc.DST_PODS)):
        s, d, q = e.reachability_classes(kc.SRC_PODS, kc.DST_PODS, dc.SERVICES, host=True)
        assert s == ws and d == wd and q.dtype == np.uint8 and (q == wq).all()
        assert s[0][0] == kc.SRC_PODS[0] and kc.SRC_PODS[0] in s[0][1:] and sum(map(len, d)) == len(kc.DST_PODS)
    s, d, q = c.e0.reachability_classes(kc.SRC_PODS, [], dc.SERVICES, host=True)
    assert s == [kc.SRC_PODS] and d == [] and q.shape == (len(dc.SERVICES), 1, 0)


# ---- arguments ---------------------------------------------------------------------------------
def test_einval():
    e = engine()
    w, out = np.zeros(64, np.uint32), np.full(64, kc.FILL, np.uint32)
    res = _capi.pg_reach_classes_result(7, 7, 7)
    for what, words, spec, outs, with_result in kc.bad_calls(w.ctypes.data, out.ctypes.data):
        code = lib.pg_debug_reach_classes_host(e.h, C.byref(spec) if spec is not None else None, *outs,
                                               C.byref(res) if with_result else None)
        assert code == _capi.PG_EINVAL, (what, code)
        assert words in lib.pg_last_error(e.h).decode(), (what, lib.pg_last_error(e.h))
    assert (out == kc.FILL).all() and (res.n_src_classes, res.n_dst_classes, res.rounds) == (7, 7, 7)
    assert lib.pg_debug_reach_classes_host(None, None, None, None, None, None, None, None) == _capi.PG_EINVAL
    spec = kc.spec_of(w.ctypes.data, 1, 4, 4)
    assert lib.pg_debug_reach_classes_host(e.h, C.byref(spec), out.ctypes.data, None, None, None, None, C.byref(res)) == 0
    assert out[:5].tolist() == [0, 0, 0, 0, kc.FILL] and (res.n_src_classes, res.n_dst_classes, res.rounds) == (1, 0, 1)


@pytest.mark.parametrize("empty", ("n_svc", "n_src", "n_dst"))
def test_empty_input(empty):
    """PG_OK, the result zeroed, nothing else written; the matrix may be null"""
    n = {"n_svc": 2, "n_src": 5, "n_dst": 7}
    n[empty] = 0
    bufs = kc.buffers(2, 5, 7)
    res = _capi.pg_reach_classes_result(7, 7, 7)
    spec = kc.spec_of(None, n["n_svc"], n["n_src"], n["n_dst"])
    code = lib.pg_debug_reach_classes_host(engine().h, C.byref(spec), *[b.ctypes.data_as(C.c_void_p) for b in bufs], C.byref(res))
    assert code == 0 and (res.n_src_classes, res.n_dst_classes, res.rounds) == (0, 0, 0)
    assert all((b == kc.FILL).all() for b in bufs)


def test_knob_range():
    e = engine()
    assert e.get_tuning("classes_hash_bits") == 64
    for v in (0, 1, 63, 64):
        with e.tuning(classes_hash_bits=v):
            assert e.get_tuning("classes_hash_bits") == v
    for v in (-1, 65, 1 << 20):
        with pytest.raises(Exception):
            e.set_tuning("classes_hash_bits", v)
        assert lib.pg_ctx_set_tuning(e.h, b"classes_hash_bits", v) == _capi.PG_EINVAL
    assert e.get_tuning("classes_hash_bits") == 64
