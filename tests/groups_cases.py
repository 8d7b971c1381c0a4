"""Matrices, groupings and expected summaries of the reachability-groups tests (test helper).

Shared by tests/test_groups_host.py (pg_debug_reach_groups_host, no GPU) and tests/test_gpu_groups.py
(pg_reach_groups on the device). Expected values come from numpy alone (expected(): the codes
unpacked to [n_svc, n_src, n_dst] and np.add.at into [n_svc, n_sg, n_dg, 4]; the status from those
counts) and, for real engines, from oracle.world.World.conn -- never from the product.

synthetic(n_svc, n_src, n_dst, family, code_mix, seed): codes per mix (uniform over the four
ConnActions, all ALLOW, no ALLOW), packed with diff_cases.pack, and one grouping family on both sides:
  one        every end point in group 0
  identity   every end point its own group (ids wrap at 4096, the most groups a side may have)
  blocks     up to 7 contiguous blocks
  random     random ids, groups 0 and the last without members, about 10 % PG_GROUP_SKIP
  skewed     four groups, one of them holding 90 %
  all-skip   every end point PG_GROUP_SKIP

run_host / check hold a backend (the host twin here, the device in test_gpu_groups.py) against
expected(): counts, status words and their zero padding; every output is prefilled with 0xFF.. and a
guard of 3 entries behind each output must stay untouched; without out_packed it stays untouched.
"""
import ctypes as C

import numpy as np

import diff_cases as dc
from vpp_amd import _capi
from vpp_amd._capi import lib

SKIP = _capi.GROUP_SKIP
ALLOW = 2
FAMILIES = ("one", "identity", "blocks", "random", "skewed", "all-skip")
MIXES = ("uniform", "all-allow", "no-allow")
FILL, FILL64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
GUARD = 3   # prefilled entries behind every output that must stay untouched
MAX_GROUPS = 4096


def row_words(n):
    return (n + 15) // 16


def grouping(n, family, g):
    """(ids uint32 [n], the group count) of one side"""
    if family == "one":
        return np.zeros(n, np.uint32), 1
    if family == "identity":
        return (np.arange(n) % MAX_GROUPS).astype(np.uint32), min(max(n, 1), MAX_GROUPS)
    if family == "blocks":
        k = max(1, min(n, 7))
        return (np.arange(n) * k // max(n, 1)).astype(np.uint32), k
    if family == "random":
        k = min(MAX_GROUPS, max(4, n // 3))
        ids = g.integers(1, k - 1, n).astype(np.uint32)
        ids[g.random(n) < 0.1] = SKIP
        return ids, k
    if family == "skewed":
        ids = np.where(g.random(n) < 0.9, 1, g.integers(0, 4, n)).astype(np.uint32)
        return ids, 4
    assert family == "all-skip", family
    return np.full(n, SKIP, np.uint32), 3


def pack(codes2d):
    """uint8 codes [rows, cols] -> packed words (diff_cases.pack; its vectorised form for wide rows)"""
    return dc.pack(codes2d) if codes2d.shape[1] <= 1000 else dc.pack_wide(codes2d)


def expected(codes, sg, dg, n_sg, n_dg):
    """(counts u64 [n_svc, n_sg, n_dg, 4], status u8 [n_svc, n_sg, n_dg]) of uint8 codes [n_svc, n_src, n_dst]"""
    codes = np.asarray(codes)
    counts = np.zeros((codes.shape[0], n_sg, n_dg, 4), np.uint64)
    ks, kd = sg != SKIP, dg != SKIP
    c = codes[:, ks][:, :, kd].astype(np.int64)
    np.add.at(counts, (np.arange(codes.shape[0])[:, None, None], sg[ks].astype(np.int64)[None, :, None],
                       dg[kd].astype(np.int64)[None, None, :], c), np.uint64(1))
    return counts, status_of(counts)


def status_of(counts):
    cells, allow = counts.sum(axis=-1), counts[..., ALLOW]
    return np.where(cells == 0, 3, np.where(allow == cells, 2, np.where(allow > 0, 1, 0))).astype(np.uint8)


def pack_status(status):
    """status u8 [n_svc, n_sg, n_dg] -> the packed words [n_svc, n_sg, row_words(n_dg)], padding zero"""
    n_svc, n_sg, n_dg = status.shape
    return pack(status.reshape(n_svc * n_sg, n_dg)).reshape(n_svc, n_sg, row_words(n_dg))


class Synthetic:
    def __init__(self, n_svc, n_src, n_dst, family, code_mix="uniform", seed=0):
        g = np.random.default_rng([seed, n_svc, n_src, n_dst, FAMILIES.index(family), MIXES.index(code_mix)])
        self.n_svc, self.n_src, self.n_dst = n_svc, n_src, n_dst
        shape = (n_svc, n_src, n_dst)
        if code_mix == "uniform":
            self.codes = g.integers(0, 4, shape).astype(np.uint8)
        elif code_mix == "all-allow":
            self.codes = np.full(shape, ALLOW, np.uint8)
        else:
            self.codes = np.array([0, 1, 3], np.uint8)[g.integers(0, 3, shape)]
        self.words = pack(self.codes.reshape(n_svc * n_src, n_dst)).reshape(n_svc, n_src, row_words(n_dst))
        self.sg, self.n_sg = grouping(n_src, family, g)
        self.dg, self.n_dg = grouping(n_dst, family, g)
        self._want = None

    @property
    def want(self):
        if self._want is None:
            self._want = expected(self.codes, self.sg, self.dg, self.n_sg, self.n_dg)
        return self._want

    def args(self):
        return self.n_svc, self.n_src, self.n_dst, self.sg, self.dg, self.n_sg, self.n_dg


def synthetic(n_svc, n_src, n_dst, family, code_mix="uniform", seed=0):
    return Synthetic(n_svc, n_src, n_dst, family, code_mix, seed)


def buffers(n_svc, n_sg, n_dg):
    """prefilled (counts, status words) with their guards, flat"""
    return (np.full(n_svc * n_sg * n_dg * 4 + GUARD, FILL64, np.uint64),
            np.full(n_svc * n_sg * row_words(n_dg) + GUARD, FILL, np.uint32))


def spec_of(matrix_ptr, n_svc, n_src, n_dst, sg, dg, n_sg, n_dg):
    """(pg_reach_groups_spec, the id arrays it points into)"""
    sg, dg = np.ascontiguousarray(sg, np.uint32), np.ascontiguousarray(dg, np.uint32)
    return _capi.pg_reach_groups_spec(matrix_ptr, n_svc, n_src, n_dst, sg.ctypes.data if n_src else None,
                                      dg.ctypes.data if n_dst else None, n_sg, n_dg), (sg, dg)


def finish(cbuf, pbuf, n_svc, n_sg, n_dg, packed):
    """the guards of a run's buffers, and the run's return value (counts, status words or None)"""
    nc, nw = n_svc * n_sg * n_dg * 4, n_svc * n_sg * row_words(n_dg)
    assert (cbuf[nc:] == FILL64).all() and (pbuf[nw:] == FILL).all(), "a guard was written"
    if not packed:
        assert (pbuf == FILL).all(), "out_packed was written though it was not given"
    return cbuf[:nc].reshape(n_svc, n_sg, n_dg, 4), pbuf[:nw].reshape(n_svc, n_sg, row_words(n_dg)) if packed else None


def run_host(e, words, n_svc, n_src, n_dst, sg, dg, n_sg, n_dg, packed=True):
    """pg_debug_reach_groups_host over prefilled outputs with guards -> (counts, status words or None)"""
    m = np.ascontiguousarray(words, np.uint32)
    cbuf, pbuf = buffers(n_svc, n_sg, n_dg)
    spec, keep = spec_of(m.ctypes.data if m.size else None, n_svc, n_src, n_dst, sg, dg, n_sg, n_dg)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    code = lib.pg_debug_reach_groups_host(e.h, C.byref(spec), p(cbuf), p(pbuf) if packed else None)
    assert code == 0, lib.pg_last_error(e.h)
    return finish(cbuf, pbuf, n_svc, n_sg, n_dg, packed)


def same(got, want, what):
    """a run's return value against expected()'s"""
    counts, words = got
    wc, ws = want
    assert (counts == wc).all(), (what, "counts", np.argwhere(counts != wc)[:3].tolist())
    if words is not None:
        assert (words == pack_status(ws)).all(), (what, "status", np.argwhere(words != pack_status(ws))[:3].tolist())


def check(run, s, words=None, variants=True):
    """`run(words, n_svc, n_src, n_dst, sg, dg, n_sg, n_dg, packed=)` (run_host's contract without the
    engine) against numpy on the Synthetic s; words: another packing of s.codes (garbage in the padding)"""
    w = s.words if words is None else words
    what = (s.n_svc, s.n_src, s.n_dst, s.n_sg, s.n_dg)
    same(run(w, *s.args()), s.want, what)
    assert int(s.want[0].sum()) == s.n_svc * int((s.sg != SKIP).sum()) * int((s.dg != SKIP).sum())
    if variants:
        same(run(w, *s.args(), packed=False), s.want, what)


# ---- real engines ------------------------------------------------------------------------------
def fixed_groups(n_src, n_dst):
    """the tests' fixed rule: src index modulo 3; dst in blocks of 8 (the last group has no member).
    The callers list one end point of each side twice, the second time in another group."""
    sg = (np.arange(n_src) % 3).astype(np.uint32)
    dg = (np.arange(n_dst) // 8).astype(np.uint32)
    return sg, 3, dg, int(dg.max()) + 2 if n_dst else 1


def doubled(ips):
    """the end points with the first one listed once more at the end"""
    ips = np.asarray(ips, np.uint32)
    return np.concatenate([ips, ips[:1]])


# ---- the wrappers over the fixture change (diff_cases.matrix_change) -----------------------------
SRC_GROUPS = {"a": ["ns/p0", "ns/p1", "ns/p2"], "b": ["ns/p3", "ns/lost"], "c": ["ns/far", "ns/p0"]}   # p0 in two groups
DST_GROUPS = {"x": ["ns/p0", "ns/p1"], "y": ["ns/p2", "ns/p3", "ns/lost", "ns/far"], "z": ["ns/p1"], "none": []}


def wrapper_want(c):
    """(counts, status) before and after over SRC_GROUPS x DST_GROUPS, from the oracle"""
    ip = dict(zip(dc.PODS, c.pod_ips))
    src = np.array([ip[p] for pods in SRC_GROUPS.values() for p in pods], np.uint32)
    dst = np.array([ip[p] for pods in DST_GROUPS.values() for p in pods], np.uint32)
    sg = np.repeat(np.arange(len(SRC_GROUPS)), [len(p) for p in SRC_GROUPS.values()]).astype(np.uint32)
    dg = np.repeat(np.arange(len(DST_GROUPS)), [len(p) for p in DST_GROUPS.values()]).astype(np.uint32)
    return [expected(codes.reshape(len(dc.SERVICES), len(src), len(dst)), sg, dg, len(SRC_GROUPS), len(DST_GROUPS))
            for codes in c.matrix_codes(src, dst)]


def diff_want(before, after):
    """the numpy diff of two status arrays as reachability_groups_diff lists it"""
    sn, dn = list(SRC_GROUPS), list(DST_GROUPS)
    return [(int(v), sn[i], dn[j], int(before[v, i, j]), int(after[v, i, j])) for v, i, j in np.argwhere(before != after)]


# ---- arguments ---------------------------------------------------------------------------------
def bad_specs(ptr):
    """(what, spec or None, out_counts given) of every PG_EINVAL; the ids must outlive the calls"""
    S = _capi.pg_reach_groups_spec
    ids = np.zeros(1 << 11, np.uint32)
    g = ids.ctypes.data
    bad_s, bad_d = ids[:4].copy(), ids[:4].copy()
    bad_s[2], bad_d[3] = 5, 0xFFFFFFFE
    return ids, bad_s, bad_d, [
        ("null spec", None, True), ("null matrix", S(None, 1, 4, 4, g, g, 1, 1), True),
        ("null out_counts", S(ptr, 1, 4, 4, g, g, 1, 1), False),
        ("null src_group", S(ptr, 1, 4, 4, None, g, 1, 1), True), ("null dst_group", S(ptr, 1, 4, 4, g, None, 1, 1), True),
        ("n_src", S(ptr, 1, (1 << 20) + 1, 4, g, g, 1, 1), True), ("n_dst", S(ptr, 1, 4, (1 << 20) + 1, g, g, 1, 1), True),
        ("n_svc", S(ptr, 4097, 4, 4, g, g, 1, 1), True),
        ("n_src_groups 0", S(ptr, 1, 4, 4, g, g, 0, 1), True), ("n_dst_groups 0", S(ptr, 1, 4, 4, g, g, 1, 0), True),
        ("n_src_groups", S(ptr, 1, 4, 4, g, g, 4097, 1), True), ("n_dst_groups", S(ptr, 1, 4, 4, g, g, 1, 4097), True),
        ("product", S(ptr, 64, 4, 4, g, g, 4096, 4096), True),
        ("src id", S(ptr, 1, 4, 4, bad_s.ctypes.data, g, 5, 1), True),
        ("dst id", S(ptr, 1, 4, 4, g, bad_d.ctypes.data, 1, 7), True)]
