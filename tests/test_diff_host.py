"""The reachability diff on the host (no GPU): pg_debug_reach_diff_host running the per-word code of
pg_reach_diff (diff.hpp, the functions the kernels call) against numpy on the synthetic pairs of
tests/diff_cases.py, and against the oracle on a real matrix change and a real sweep change.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import diff_cases as dc
import ports_cases as pc
from vpp_amd import _capi
from vpp_amd import device as D
from vpp_amd import renderer as R
from vpp_amd._capi import lib


@functools.lru_cache(maxsize=None)
def engine():
    return R.Engine(0)


def run(*args, **kw):
    return dc.run_host(engine(), *args, **kw)


@pytest.mark.parametrize("n_cols", dc.COLS)
def test_synthetic(n_cols):
    for n_rows in dc.ROWS:
        for p in dc.PS:
            b, a = dc.synthetic(n_rows, n_cols, p)
            assert p not in (0.0, 1.0) or int((a != b).sum()) == int(p) * b.size
            dc.check(run, b, a, dc.pack(b), dc.pack(a))


@pytest.mark.parametrize("n_cols", dc.COLS)
def test_padding_garbage(n_cols):
    """garbage in both inputs' padding bits: the result is that of the clean inputs"""
    for n_rows in (3, 37):
        b, a = dc.synthetic(n_rows, n_cols, 1.0 / 64, seed=2)
        bw, aw = dc.garbage(dc.pack(b), n_cols, 3), dc.garbage(dc.pack(a), n_cols, 4)
        if n_cols & 15:
            assert (bw != dc.pack(b)).any() and (aw != dc.pack(a)).any()
        dc.check(run, b, a, bw, aw)


def test_unpack_changes():
    b, a = dc.synthetic(37, 53, 1.0 / 64)
    n, changes, trans, rows = engine().debug_reach_diff_host(dc.pack(b), dc.pack(a), 53)
    row, col, cb, ca = D.unpack_changes(changes[:n])
    at = np.argwhere(a != b)
    assert n == len(at) and (row == at[:, 0]).all() and (col == at[:, 1]).all()
    assert (cb == b[a != b]).all() and (ca == a[a != b]).all()
    assert (changes[n:] == dc.FILL).all() and (rows == (a != b).sum(axis=1)).all()
    assert int(trans.sum()) == b.size


def test_max_cols():
    """n_cols = 2^20, the widest row: the column field's 20 bits"""
    n_cols = 1 << 20
    small = dc.synthetic(3, 53, 1.0)[0]
    assert (dc.pack_wide(small) == dc.pack(small)).all()
    b, a = dc.synthetic(1, n_cols, 1.0 / 64)
    dc.check(run, b, a, dc.pack_wide(b), dc.pack_wide(a), transitions=(dc.ALL, dc.CLOSED), variants=False)


def call(e, spec, n_changes=True, changes=None, rows=None, trans=None):
    n = C.c_uint64(dc.FILL)
    p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    code = lib.pg_debug_reach_diff_host(e.h, C.byref(spec) if spec is not None else None, p(changes), p(rows),
                                        C.byref(n) if n_changes else None, p(trans))
    return code, n.value


def test_einval():
    e = engine()
    w = np.zeros(4, np.uint32)
    ptr = w.ctypes.data
    S = _capi.pg_reach_diff_spec
    bad = [(None, True), (S(None, ptr, 1, 16, dc.ALL, 0), True), (S(ptr, None, 1, 16, dc.ALL, 0), True),
           (S(ptr, ptr, 1, 16, dc.ALL, 0), False),                 # null n_changes
           (S(ptr, ptr, 1, 0, dc.ALL, 0), True), (S(ptr, ptr, 1, (1 << 20) + 1, dc.ALL, 0), True),
           (S(ptr, ptr, 1 << 32, 16, dc.ALL, 0), True),            # n_rows >= 2^32
           (S(ptr, ptr, 1 << 31, 32, dc.ALL, 0), True),            # n_rows * row_words = 2^32
           (S(ptr, ptr, (1 << 32) - 1, 17, dc.ALL, 0), True)]
    for spec, with_n in bad:
        code, _ = call(e, spec, n_changes=with_n)
        assert code == _capi.PG_EINVAL, (spec, code)
        assert lib.pg_last_error(e.h), "pg_last_error is empty"
    # the largest shapes the checks let through are not refused for their size
    assert call(e, S(ptr, ptr, 1, 16, dc.ALL, 0))[0] == 0


def test_no_rows():
    """n_rows == 0: PG_OK, *n_changes = 0, trans zeroed, nothing else written"""
    e = engine()
    w = np.zeros(4, np.uint32)
    changes, rows = np.full((4, 2), dc.FILL, np.uint32), np.full(4, dc.FILL, np.uint32)
    trans = np.full(16, 7, np.uint64)
    code, n = call(e, _capi.pg_reach_diff_spec(w.ctypes.data, w.ctypes.data, 0, 16, dc.ALL, 4), True, changes, rows, trans)
    assert code == 0 and n == 0 and (trans == 0).all()
    assert (changes == dc.FILL).all() and (rows == dc.FILL).all()


# ---- a real matrix change ----------------------------------------------------------------------
def test_matrix_oracle_numbers():
    """the oracle alone: the numbers of the edit (diff_cases.MATRIX_WANT)"""
    c = dc.matrix_change()
    x, w = dc.Expected(c.b, c.a, dc.ALL), dc.MATRIX_WANT
    assert c.b.size == w["cells"] and x.n == w["changed"] and dc.off_diagonal(x.trans) == w["trans"]
    assert int((x.row_changes > 0).sum()) == w["rows_changed"] and len(x.row_changes) == w["rows"]
    assert int(x.trans[3, 3]) == w["failure"] and x.trans[3].sum() == w["failure"] and x.trans[:, 3].sum() == w["failure"]


def test_matrix_change():
    c = dc.matrix_change()
    bw = c.e0.debug_reach_matrix_host(c.src, c.dst, dc.SERVICES, words=False)
    aw = c.e1.debug_reach_matrix_host(c.src, c.dst, dc.SERVICES, words=False)
    assert (bw.reshape(-1, bw.shape[-1]) == dc.pack(c.b)).all() and (aw.reshape(-1, aw.shape[-1]) == dc.pack(c.a)).all()
    dc.check(run, c.b, c.a, bw, aw)
    assert run(bw, aw, dc.N_DST, dc.OPENED, 0)[0] == dc.MATRIX_WANT["opened"]
    assert run(bw, aw, dc.N_DST, dc.CLOSED, 0)[0] == dc.MATRIX_WANT["closed"]


@pytest.mark.parametrize("transitions", (dc.ALL, dc.OPENED, dc.CLOSED), ids=("all", "opened", "closed"))
def test_reachability_diff(transitions):
    """Engine.reachability_diff over the fixture's pods, host twins: the oracle's diff as tuples"""
    c = dc.matrix_change()
    got, trans = c.e1.reachability_diff(c.e0, dc.PODS, dc.PODS, dc.SERVICES, transitions, host=True)
    want = dc.pod_tuples(c, transitions)
    assert want and got == want
    ips = np.array(c.pod_ips, np.uint32)
    assert (trans == dc.Expected(*c.matrix_codes(ips, ips), transitions).trans).all()


# ---- a real sweep change that keeps the partition ---------------------------------------------
@pytest.mark.parametrize("protocol", (pc.TCP, pc.UDP), ids=("tcp", "udp"))
def test_sweep_change(protocol):
    c = dc.sweep_change()
    w = dc.SWEEP_WANT[protocol]
    b, a = c.codes[protocol]
    x = dc.Expected(b, a, dc.ALL)
    # the oracle alone
    assert len(c.lo[protocol]) == w["K"] and b.size == w["cells"] and x.n == w["changed"]
    assert dc.off_diagonal(x.trans) == w["trans"] and int((x.row_changes > 0).sum()) == w["pairs"]
    lo0, bw, _, _ = c.e0.debug_reach_ports_host(c.src, c.dst, protocol, pc.SPORT)
    lo1, aw, _, _ = c.e1.debug_reach_ports_host(c.src, c.dst, protocol, pc.SPORT)
    assert np.array_equal(lo0, lo1) and np.array_equal(lo0, c.lo[protocol])
    dc.check(run, b, a, bw, aw)
    if protocol == pc.UDP:   # nothing changes: an all-diagonal trans, row_changes all zero
        n, _, trans, rows = run(bw, aw, w["K"], dc.ALL, 0)
        assert n == 0 and (rows == 0).all() and (trans == np.diag(np.diag(trans))).all()
