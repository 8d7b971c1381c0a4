"""Pairs of packed audit results and their expected diffs (test helper).

Shared by tests/test_diff_host.py (pg_debug_reach_diff_host, no GPU) and tests/test_gpu_diff.py
(pg_reach_diff on the device). Expected values come from numpy on unpacked code arrays (Expected)
and, for the real changes, from oracle.world.World.conn -- never from the product.

Synthetic pairs (synthetic()): codes from rng.integers(0, 4); `after` differs from `before` in a share
p of the cells, each changed to a different code; packed with reach_cases.pack. Columns COLS, rows
ROWS, shares PS. garbage() sets random padding bits in a packed array.

check(run, ...) holds a backend (`run`: the host twin here, the device in test_gpu_diff.py) against
Expected for the transitions ALL, OPENED, CLOSED, one single bit, 0 and the diagonal bits alone:
the list in np.argwhere order, row_changes, trans and its sum, a cap below the total (the exact
prefix, the full total, the rest of the prefilled buffer untouched), count-only calls and every
optional output left out.

The real changes run on the fixture of tests/ports_cases.py, fixture("full"), on instances built
here (never the cached topology other tests share): matrix_change() deletes ACL g and replaces
in-tap2 on the second engine; sweep_change() flips three rule actions, which keeps the port
partition. MATRIX_WANT and SWEEP_WANT are the oracle's numbers for them, measured on the CPU;
the test files assert them on the oracle's output before any product code runs.
"""
import ctypes as C
import functools

import numpy as np

import node_matrix as nm
import ports_cases as pc
import reach_cases as rc
from oracle.world import World
from vpp_amd import _capi
from vpp_amd._capi import lib

ALL, OPENED, CLOSED = _capi.DIFF_ALL, _capi.DIFF_OPENED, _capi.DIFF_CLOSED
DIAG = 0x8421                 # 0->0, 1->1, 2->2, 3->3: ignored
SINGLE = 1 << (4 * 3 + 1)     # 3 -> 1 alone
TRANSITIONS = (ALL, OPENED, CLOSED, SINGLE, 0, DIAG)
COLS = (1, 15, 16, 17, 31, 32, 33, 53, 64, 1000)
ROWS = (1, 3, 37, 64)
PS = (0.0, 1.0 / 64, 1.0)
FILL = 0xFFFFFFFF
GUARD = 3                     # prefilled entries behind `cap` that must stay untouched


def row_words(n_cols):
    return (n_cols + 15) // 16


def synthetic(n_rows, n_cols, p, seed=0):
    """(before, after) uint8 codes [n_rows, n_cols]"""
    g = np.random.default_rng([seed, n_rows, n_cols, int(p * 64)])
    b = g.integers(0, 4, (n_rows, n_cols)).astype(np.uint8)
    change = np.ones(b.shape, bool) if p >= 1.0 else g.random(b.shape) < p
    a = np.where(change, (b + g.integers(1, 4, b.shape)) & 3, b).astype(np.uint8)
    assert ((a != b) == change).all()
    return b, a


def pack(codes):
    """uint8 codes [n_rows, n_cols] -> packed words [n_rows, row_words], padding zero"""
    return rc.pack((codes.astype(np.uint32) << 30)[None])[0]


def pack_wide(codes):
    """pack() without its loop over the columns, for very wide rows"""
    n_rows, n_cols = codes.shape
    c = np.zeros((n_rows, row_words(n_cols) * 16), np.uint32)
    c[:, :n_cols] = codes
    return (c.reshape(n_rows, -1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=2, dtype=np.uint32)


def garbage(packed, n_cols, seed=1):
    """a copy with random bits in the padding of every row's last word"""
    out = packed.copy()
    used = n_cols & 15
    if used:
        g = np.random.default_rng(seed)
        junk = g.integers(0, 1 << 32, out.shape[0], dtype=np.uint64).astype(np.uint32)
        out[:, -1] |= junk & np.uint32((0xFFFFFFFF << (2 * used)) & 0xFFFFFFFF)
    return out


class Expected:
    """the diff of two code arrays under `transitions`, by numpy"""

    def __init__(self, b, a, transitions):
        b, a = np.asarray(b), np.asarray(a)
        sel = np.array([[bc != ac and bool(transitions >> (4 * bc + ac) & 1) for ac in range(4)] for bc in range(4)])
        ch = sel[b, a]
        at = np.argwhere(ch)   # ascending (row, column)
        self.n = len(at)
        cb, ca = b[ch].astype(np.uint32), a[ch].astype(np.uint32)
        self.entries = np.stack([at[:, 0].astype(np.uint32), at[:, 1].astype(np.uint32) | cb << 28 | ca << 30],
                                axis=1).reshape(-1, 2)
        self.row_changes = ch.sum(axis=1).astype(np.uint32)
        self.trans = np.bincount(4 * b.ravel().astype(np.int64) + a.ravel(), minlength=16).astype(np.uint64).reshape(4, 4)


def run_host(e, bw, aw, n_cols, transitions, cap, changes=True, rows=True, trans=True):
    """pg_debug_reach_diff_host over prefilled outputs -> (n_changes, the whole changes buffer u32
    [cap + GUARD, 2], trans [4, 4] or None, row_changes or None)"""
    b, a = np.ascontiguousarray(bw, np.uint32), np.ascontiguousarray(aw, np.uint32)
    n_rows = b.size // row_words(n_cols)
    buf = np.full((cap + GUARD, 2), FILL, np.uint32)
    rbuf = np.full(n_rows + 1, FILL, np.uint32)
    tbuf = np.full(17, 0xFFFFFFFFFFFFFFFF, np.uint64)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    spec = _capi.pg_reach_diff_spec(b.ctypes.data, a.ctypes.data, n_rows, n_cols, transitions, cap)
    n = C.c_uint64(FILL)
    code = lib.pg_debug_reach_diff_host(e.h, C.byref(spec), p(buf) if changes else None, p(rbuf) if rows else None,
                                        C.byref(n), p(tbuf) if trans else None)
    assert code == 0, lib.pg_last_error(e.h)
    assert rbuf[n_rows] == FILL and tbuf[16] == 0xFFFFFFFFFFFFFFFF
    if not changes:
        assert (buf == FILL).all()
    return n.value, buf, tbuf[:16].reshape(4, 4) if trans else None, rbuf[:n_rows] if rows else None


def check(run, b, a, bw, aw, transitions=TRANSITIONS, variants=True):
    """`run(bw, aw, n_cols, transitions, cap, changes=, rows=, trans=)` (run_host's contract without
    the engine) against numpy on the codes b, a [n_rows, n_cols] the packed bw, aw hold"""
    n_rows, n_cols = b.shape
    for t in transitions:
        x = Expected(b, a, t)
        if t in (0, DIAG):
            assert x.n == 0
        n, buf, trans, rows = run(bw, aw, n_cols, t, x.n)
        assert n == x.n, (hex(t), n, x.n)
        assert (buf[:x.n] == x.entries).all(), (hex(t), first_bad(buf[:x.n], x.entries))
        assert (buf[x.n:] == FILL).all(), "an entry past the total was written"
        assert (rows == x.row_changes).all() and (trans == x.trans).all(), hex(t)
        assert int(trans.sum()) == n_rows * n_cols
        if not variants:
            continue
        if x.n > 1:   # a cap below the total: the exact prefix, the full total
            cap = x.n // 2
            n, buf, trans, rows = run(bw, aw, n_cols, t, cap)
            assert n == x.n and (buf[:cap] == x.entries[:cap]).all() and (buf[cap:] == FILL).all()
            assert (rows == x.row_changes).all() and (trans == x.trans).all()
        # count only: no list, and a list of no entries; then each optional output left out
        for kw in ({"changes": False}, {"changes": True}):
            n, buf, trans, rows = run(bw, aw, n_cols, t, 0, **kw)
            assert n == x.n and (buf == FILL).all() and (rows == x.row_changes).all() and (trans == x.trans).all()
        n, buf, trans, rows = run(bw, aw, n_cols, t, x.n, rows=False, trans=False)
        assert n == x.n and (buf[:x.n] == x.entries).all() and trans is None and rows is None
        n, _, trans, rows = run(bw, aw, n_cols, t, 0, changes=False, rows=False)
        assert n == x.n and (trans == x.trans).all()
        n, _, trans, rows = run(bw, aw, n_cols, t, 0, changes=False, trans=False)
        assert n == x.n and (rows == x.row_changes).all()


def first_bad(got, want):
    bad = np.argwhere((got != want).any(axis=1))
    return "%d of %d entries differ; first %s" % (len(bad), len(want), [
        (int(i), [hex(int(v)) for v in got[i[0]]], [hex(int(v)) for v in want[i[0]]]) for i in bad[:3]])


# ---- the real changes ------------------------------------------------------------------------
KEY = "config/vpp/acls/v2/acl/"
N_SRC, N_DST = rc.N_SRC, rc.N_DST
SERVICES = ([(pc.TCP, 40000, p) for p in (0, 80, 150, 250, 443, 1500, 3000, 8080, 40000, 65535)] +
            [(pc.UDP, 40000, p) for p in (53, 123, 5050, 40000)] + [(2, 0, 0), (3, 1234, 80)])
MATRIX_EDIT = [(KEY + "g", None),
               (KEY + "in-tap2", {"name": "in-tap2", "ingress": ["tap2"], "egress": [], "rules": [
                   {"action": 0, "src": "", "dst": "", "tcp": pc._l4(0, 1023)}, {"action": 2, "src": "", "dst": ""}]})]
# the oracle on MATRIX_EDIT: cells, changed cells, off-diagonal transitions, rows with a change / rows,
# FAILURE cells (all unchanged)
MATRIX_WANT = {"cells": 31376, "changed": 4358, "trans": {(0, 1): 312, (0, 2): 3120, (1, 2): 192, (2, 0): 584, (2, 1): 150},
               "rows_changed": 234, "rows": 592, "failure": 12320, "opened": 3312, "closed": 734}
# the oracle on the sweep edit, per protocol: K, cells, changed cells, transitions, pairs with a change
SWEEP_WANT = {pc.TCP: {"K": 25, "cells": 49025, "changed": 450, "trans": {(0, 2): 285, (2, 0): 165}, "pairs": 237},
              pc.UDP: {"K": 14, "cells": 37 * 53 * 14, "changed": 0, "trans": {}, "pairs": 0}}
PODS = ["ns/p0", "ns/p1", "ns/p2", "ns/p3", "ns/lost", "ns/far"]


def sweep_edit():
    acls = pc.fixture_acls("full")
    in1 = [dict(r) for r in acls["in-tap1"][0]]
    out0 = [dict(r) for r in acls["out-tap0"][0]]
    in1[0]["action"] = 1                       # DENY -> PERMIT
    out0[3]["action"], out0[4]["action"] = 0, 2   # TCP 100..199 PERMIT -> DENY, TCP 200..299 DENY -> REFLECT
    return [(KEY + "in-tap1", {"name": "in-tap1", "rules": in1, "ingress": ["tap1"], "egress": []}),
            (KEY + "out-tap0", {"name": "out-tap0", "rules": out0, "ingress": [], "egress": ["tap0"]})]


class _Side:
    fixture = True


def off_diagonal(trans):
    return {(b, a): int(trans[b, a]) for b in range(4) for a in range(4) if b != a and trans[b, a]}


class Change:
    """two fresh fixture("full") engines, the second edited by ApplyTxn(False, edit), and their
    oracle worlds; src / dst: ports_cases.sides at 37 x 53"""

    def __init__(self, edit):
        self.e0, (local, lost), self.pod_ips = pc.fixture("full")
        self.e1, _, _ = pc.fixture("full")
        self.e1.ApplyTxn(False, edit)
        for e in (self.e0, self.e1):
            e.num_tables()
        self.w0 = World(self.e0, local, nm.NODE_IF, no_if_ips=lost)
        self.w1 = World(self.e1, local, nm.NODE_IF, no_if_ips=lost)
        self.src, self.dst = pc.sides(_Side, N_SRC, N_DST)

    def matrix_codes(self, src=None, dst=None):
        """the oracle's ConnActions (before, after), each [n_svc * n_src, n_dst]"""
        src, dst = self.src if src is None else src, self.dst if dst is None else dst
        return tuple((rc.oracle_words(w, src, dst, SERVICES) >> 30).astype(np.uint8).reshape(-1, len(dst))
                     for w in (self.w0, self.w1))

    def sweep_codes(self, protocol, lo):
        """the oracle's ConnActions at the intervals' first ports (before, after), each [n_src * n_dst, K]"""
        return tuple((pc.oracle_words(w, self.src, self.dst, protocol, lo) >> 30).astype(np.uint8).reshape(-1, len(lo))
                     for w in (self.w0, self.w1))


@functools.lru_cache(maxsize=None)
def matrix_change():
    c = Change(MATRIX_EDIT)
    c.b, c.a = c.matrix_codes()
    # preconditions, on the oracle's output alone
    x = Expected(c.b, c.a, ALL)
    assert x.n >= 4000 and len(off_diagonal(x.trans)) >= 5 and 3 * (c.b.size - x.n) >= 2 * c.b.size, (x.n, x.trans)
    return c


@functools.lru_cache(maxsize=None)
def sweep_change():
    c = Change(sweep_edit())
    c.lo = {p: pc.cuts(c.e0, p) for p in (pc.TCP, pc.UDP)}
    for p in (pc.TCP, pc.UDP):
        assert np.array_equal(c.lo[p], pc.cuts(c.e1, p)), "the edit moved the partition"
    c.codes = {p: c.sweep_codes(p, c.lo[p]) for p in (pc.TCP, pc.UDP)}
    x = Expected(*c.codes[pc.TCP], ALL)
    assert x.n >= 400 and x.trans[0, 2] > 0 and x.trans[2, 0] > 0, (x.n, x.trans)
    return c


def pod_tuples(c, transitions):
    """the oracle's diff over PODS x PODS x SERVICES as reachability_diff reports it"""
    ips = np.array(c.pod_ips, np.uint32)
    assert len(ips) == len(PODS)
    b, a = c.matrix_codes(ips, ips)
    row, cell = Expected(b, a, transitions).entries.T
    n = len(PODS)
    return [(int(r) // n, PODS[int(r) % n], PODS[int(j) & 0xFFFFF], int(j) >> 28 & 3, int(j) >> 30)
            for r, j in zip(row, cell)]
