"""Matrices and expected classes of the reachability-classes tests (test helper).

Shared by tests/test_classes_host.py (pg_debug_reach_classes_host, no GPU) and tests/test_gpu_classes.py
(pg_reach_classes on the device). Expected values come from numpy alone (expected(): the codes
unpacked to [n_svc, n_src, n_dst], np.unique(axis=0, return_inverse=True) on the concatenated rows and
on the columns, renumbered to first appearance; the quotient indexed from the codes) and, for real
engines, from oracle.world.World.conn -- never from the product.

synthetic(n_svc, n_src, n_dst, family, code_mix, seed): the codes come from the mix's alphabet (uniform:
the four ConnActions, all-allow: ALLOW alone, no-allow: the other three), packed with diff_cases.pack:
  distinct   every cell drawn on its own
  one        every cell equal
  blocks     4 row patterns x 5 column patterns, the end points assigned to them at random
  near       blocks, then single cells changed to another code so that one end point leaves its class by
             exactly one cell: at column 0, at the last valid cell of the last word, and in the last
             slice only (under all-allow the changed cells are the only ones that are not ALLOW)
  dup        distinct over half as many end points, listed with repeats
assert_inputs() holds the inputs themselves: blocks and near have fewer classes than end points and more
than one wherever the alphabet and the sides allow it, and near has exactly the expected extra classes.

run_host / check hold a backend (the host twin here, the device in test_gpu_classes.py) against
expected(): every output is prefilled with 0xFF.., a guard of 3 entries behind each output must stay
untouched, as must the entries past n_classes and past the quotient's used words and every output that
was not given; the variants are only src, only dst, no reps and no quotient.
"""
import collections
import ctypes as C

import numpy as np

import diff_cases as dc
from vpp_amd import _capi
from vpp_amd.device import unpack_reach
from vpp_amd._capi import lib

ALLOW = 2
FAMILIES = ("distinct", "one", "blocks", "near", "dup")
MIXES = ("uniform", "all-allow", "no-allow")
ALPHABET = {"uniform": (0, 1, 2, 3), "all-allow": (ALLOW,), "no-allow": (0, 1, 3)}
FILL = 0xFFFFFFFF
GUARD = 3   # prefilled entries behind every output that must stay untouched
ROW_PATTERNS, COL_PATTERNS = 4, 5
MIN_SIDE = 15   # a side at least this long holds two members of one pattern and two patterns

Out = collections.namedtuple("Out", "src_class dst_class src_rep dst_rep quotient result")


def row_words(n):
    return (n + 15) // 16


def pack(codes2d):
    """uint8 codes [rows, cols] -> packed words (diff_cases.pack; its vectorised form for wide rows)"""
    return dc.pack(codes2d) if codes2d.shape[1] <= 1000 else dc.pack_wide(codes2d)


def pack3(codes):
    n_svc, n_src, n_dst = codes.shape
    return pack(codes.reshape(n_svc * n_src, n_dst)).reshape(n_svc, n_src, row_words(n_dst))


def first_appearance(inverse):
    """np.unique's inverse -> (ids numbered by first appearance, the least member of every id)"""
    inverse = np.asarray(inverse).ravel()
    n = len(inverse)
    k = int(inverse.max()) + 1 if n else 0
    first = np.full(k, n, np.int64)
    np.minimum.at(first, inverse, np.arange(n))
    order = np.argsort(first)
    new = np.empty(k, np.int64)
    new[order] = np.arange(k)
    return new[inverse].astype(np.uint32), first[order].astype(np.uint32)


def side_classes(signatures):
    """rows of a 2-D array -> (class u32 [n], rep u32 [n_classes])"""
    if signatures.shape[0] == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    # np.unique(signatures, axis=0, return_inverse=True) with every row one opaque element: the same
    # classes (the ids are renumbered anyway) without axis=0's field-by-field compare of wide rows
    rows = np.ascontiguousarray(signatures).view(np.dtype((np.void, signatures.shape[1] * signatures.itemsize)))
    _, inverse = np.unique(rows.ravel(), return_inverse=True)
    return first_appearance(inverse)


def expected(codes):
    """Out of uint8 codes [n_svc, n_src, n_dst], by numpy; the quotient as packed words; rounds None"""
    codes = np.asarray(codes, np.uint8)
    n_svc, n_src, n_dst = codes.shape
    sc, sr = side_classes(codes.transpose(1, 0, 2).reshape(n_src, n_svc * n_dst))
    dcl, dr = side_classes(codes.transpose(2, 0, 1).reshape(n_dst, n_svc * n_src))
    q = codes[:, sr][:, :, dr]
    return Out(sc, dcl, sr, dr, pack3(q) if q.size else np.zeros((n_svc, len(sr), row_words(len(dr))), np.uint32),
               {"n_src_classes": len(sr), "n_dst_classes": len(dr), "rounds": None})


class Synthetic:
    def __init__(self, n_svc, n_src, n_dst, family, code_mix="uniform", seed=0):
        g = np.random.default_rng([seed, n_svc, n_src, n_dst, FAMILIES.index(family), MIXES.index(code_mix)])
        self.n_svc, self.n_src, self.n_dst, self.family, self.mix = n_svc, n_src, n_dst, family, code_mix
        abc = np.array(ALPHABET[code_mix], np.uint8)
        draw = lambda shape: abc[g.integers(0, len(abc), shape)]
        self.flips = []
        if family == "distinct":
            codes = draw((n_svc, n_src, n_dst))
        elif family == "one":
            codes = np.full((n_svc, n_src, n_dst), draw(()), np.uint8)
        elif family == "dup":
            ms, md = (n_src + 1) // 2, (n_dst + 1) // 2
            base = draw((n_svc, ms, md))
            codes = base[:, g.integers(0, max(ms, 1), n_src)][:, :, g.integers(0, max(md, 1), n_dst)]
        else:
            pat = draw((n_svc, ROW_PATTERNS, COL_PATTERNS))
            codes = pat[:, g.integers(0, ROW_PATTERNS, n_src)][:, :, g.integers(0, COL_PATTERNS, n_dst)]
            self.base = expected(codes)
            if family == "near" and codes.size:
                codes = codes.copy()
                rows = g.permutation(n_src)[:3]
                cols = [0, n_dst - 1, int(g.integers(0, n_dst))]
                while n_dst >= 3 and cols[2] in cols[:2]:   # (the third flip off the first two columns)
                    cols[2] = int(g.integers(0, n_dst))
                cols = list(dict.fromkeys(cols))
                slices = [int(g.integers(0, n_svc)), int(g.integers(0, n_svc)), n_svc - 1]
                for i, j, v in zip(rows, cols, slices):
                    others = [c for c in (ALPHABET[code_mix] if len(abc) > 1 else (0, 1, 2, 3)) if c != codes[v, i, j]]
                    codes[v, i, j] = others[int(g.integers(0, len(others)))]
                    self.flips.append((v, int(i), int(j)))
        self.codes = np.ascontiguousarray(codes, np.uint8)
        self.words = pack3(self.codes) if self.codes.size else np.zeros((n_svc, n_src, row_words(n_dst)), np.uint32)
        self._want = None

    @property
    def want(self):
        if self._want is None:
            self._want = expected(self.codes)
        return self._want

    def args(self):
        return self.n_svc, self.n_src, self.n_dst


def synthetic(n_svc, n_src, n_dst, family, code_mix="uniform", seed=0):
    return Synthetic(n_svc, n_src, n_dst, family, code_mix, seed)


def assert_inputs(s):
    """no test passes on a degenerate input"""
    w = s.want.result
    if s.family == "one":
        assert w["n_src_classes"] == w["n_dst_classes"] == 1
    if s.family == "distinct":
        # (asserted where two equal draws are out of the question: n^2 / 2 pairs, a^cells signatures)
        a = float(len(ALPHABET[s.mix]))
        if s.n_src ** 2 / 2 / a ** min(64, s.n_svc * s.n_dst) < 1e-6:
            assert w["n_src_classes"] == s.n_src
        if s.n_dst ** 2 / 2 / a ** min(64, s.n_svc * s.n_src) < 1e-6:
            assert w["n_dst_classes"] == s.n_dst
    if s.family == "dup" and s.n_src > 2 and s.n_dst > 2:
        assert w["n_src_classes"] < s.n_src and w["n_dst_classes"] < s.n_dst
    if s.family in ("blocks", "near") and s.mix != "all-allow":
        if s.n_src >= MIN_SIDE and s.n_dst >= MIN_SIDE:
            assert 1 < w["n_src_classes"] < s.n_src and 1 < w["n_dst_classes"] < s.n_dst, w
    if s.family == "near":
        # a changed end point is a class of its own; a base class lives on where a member was not changed
        for side, changed, cls in (("n_src_classes", {i for _, i, _ in s.flips}, s.base.src_class),
                                   ("n_dst_classes", {j for _, _, j in s.flips}, s.base.dst_class)):
            kept = {int(c) for k, c in enumerate(cls) if k not in changed}
            if s.n_src >= MIN_SIDE and s.n_dst >= MIN_SIDE:   # (on a shorter side one cell may be a whole pattern)
                assert w[side] == len(kept) + len(changed), (side, w, s.flips)
        if s.n_src >= MIN_SIDE and s.n_dst >= MIN_SIDE:
            assert len(s.flips) == 3 and s.flips[0][2] == 0 and s.flips[1][2] == s.n_dst - 1 and s.flips[2][0] == s.n_svc - 1
            assert w["n_src_classes"] > s.base.result["n_src_classes"] and w["n_dst_classes"] > s.base.result["n_dst_classes"]


# ---- running a backend ---------------------------------------------------------------------------
def sizes(n_svc, n_src, n_dst):
    """entries of (src_class, dst_class, src_rep, dst_rep, quotient) without their guards"""
    return n_src, n_dst, n_src, n_dst, n_svc * n_src * row_words(n_dst)


def buffers(n_svc, n_src, n_dst):
    """the five prefilled outputs with their guards"""
    return [np.full(n + GUARD, FILL, np.uint32) for n in sizes(n_svc, n_src, n_dst)]


def given(src, dst, reps, quotient):
    """which of the five outputs a variant hands over"""
    return src, dst, src and reps, dst and reps, quotient and src and dst


def finish(bufs, n_svc, n_src, n_dst, flags, res):
    """the guards and the untouched entries of a run's buffers -> Out (None for what was not given)"""
    n_sc, n_dc = res.n_src_classes, res.n_dst_classes
    used = (n_src, n_dst, n_sc, n_dc, n_svc * n_sc * row_words(n_dc))
    names = ("src_class", "dst_class", "src_rep", "dst_rep", "quotient")
    out = []
    for buf, n, name, flag in zip(bufs, used, names, flags):
        if not flag:
            assert (buf == FILL).all(), name + " was written though it was not given"
            out.append(None)
            continue
        assert (buf[n:] == FILL).all(), name + ": an entry past the used ones, or the guard, was written"
        out.append(buf[:n].copy())
    if out[4] is not None:
        out[4] = out[4].reshape(n_svc, n_sc, row_words(n_dc))
    return Out(*out, {"n_src_classes": n_sc, "n_dst_classes": n_dc, "rounds": res.rounds})


def spec_of(matrix_ptr, n_svc, n_src, n_dst):
    return _capi.pg_reach_classes_spec(matrix_ptr, n_svc, n_src, n_dst)


def run_host(e, words, n_svc, n_src, n_dst, src=True, dst=True, reps=True, quotient=True):
    """pg_debug_reach_classes_host over prefilled outputs with guards -> Out"""
    m = np.ascontiguousarray(words, np.uint32)
    bufs = buffers(n_svc, n_src, n_dst)
    flags = given(src, dst, reps, quotient)
    res = _capi.pg_reach_classes_result(FILL, FILL, FILL)
    spec = spec_of(m.ctypes.data if m.size else None, n_svc, n_src, n_dst)
    ptrs = [b.ctypes.data_as(C.c_void_p) if f else None for b, f in zip(bufs, flags)]
    code = lib.pg_debug_reach_classes_host(e.h, C.byref(spec), *ptrs, C.byref(res))
    assert code == 0, lib.pg_last_error(e.h)
    return finish(bufs, n_svc, n_src, n_dst, flags, res)


def same(got, want, what):
    """a run's Out against expected()'s, on whatever the run was given"""
    for name in ("src_class", "dst_class", "src_rep", "dst_rep", "quotient"):
        g, w = getattr(got, name), getattr(want, name)
        if g is None:
            continue
        assert g.shape == w.shape and (g == w).all(), (what, name, np.argwhere(g != w)[:3].tolist() if g.shape == w.shape else (g.shape, w.shape))
    for side, name in (("n_src_classes", "src_class"), ("n_dst_classes", "dst_class")):
        assert got.result[side] == (want.result[side] if getattr(got, name) is not None else 0), (what, side, got.result)
    if want.result["rounds"] is not None:
        assert got.result["rounds"] == want.result["rounds"], (what, got.result, want.result)


def identical(a, b, what):
    """two runs byte for byte, `rounds` included"""
    for x, y, name in zip(a[:5], b[:5], Out._fields):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), (what, name)
    assert a.result == b.result, (what, a.result, b.result)


VARIANTS = ({"dst": False}, {"src": False}, {"reps": False}, {"quotient": False})


def check(run, s, words=None, variants=True):
    """`run(words, n_svc, n_src, n_dst, src=, dst=, reps=, quotient=)` (run_host's contract without the
    engine) against numpy on the Synthetic s; words: another packing of s.codes (garbage in the padding).
    -> the full run's Out"""
    w = s.words if words is None else words
    what = (s.family, s.mix) + s.args()
    assert_inputs(s)
    full = run(w, *s.args())
    same(full, s.want, what)
    assert full.src_class[0] == 0 and full.dst_class[0] == 0 and (np.diff(full.src_rep.astype(np.int64)) > 0).all()
    assert (np.diff(full.dst_rep.astype(np.int64)) > 0).all() and full.result["rounds"] >= 1
    if variants:
        for kw in VARIANTS:
            got = run(w, *s.args(), **kw)
            same(got, s.want, what + (str(kw),))
            if "reps" in kw or "quotient" in kw:   # (both sides still: the same rounds)
                assert got.result["rounds"] == full.result["rounds"]
            else:
                assert 1 <= got.result["rounds"] <= full.result["rounds"]
    return full


def class_sizes(cls, n):
    return np.bincount(cls, minlength=n).astype(np.uint64)


# ---- Engine.reachability_classes over the fixture change (diff_cases.matrix_change) ---------------
def wrapper_want(c, src_pods, dst_pods):
    """(src classes, dst classes, codes) before and after, from the oracle"""
    ip = dict(zip(dc.PODS, c.pod_ips))
    src, dst = np.array([ip[p] for p in src_pods], np.uint32), np.array([ip[p] for p in dst_pods], np.uint32)
    out = []
    for codes in c.matrix_codes(src, dst):
        w = expected(codes.reshape(len(dc.SERVICES), len(src), len(dst)))
        members = lambda cls, pods, n: [[p for p, k in zip(pods, cls) if k == g] for g in range(n)]
        out.append((members(w.src_class, src_pods, len(w.src_rep)), members(w.dst_class, dst_pods, len(w.dst_rep)),
                    unpack_reach(w.quotient, len(dc.SERVICES), len(w.src_rep), len(w.dst_rep))))
    return out


SRC_PODS = dc.PODS + [dc.PODS[0]]            # one pod listed twice
DST_PODS = dc.PODS[::-1] + [dc.PODS[2]]


# ---- arguments ---------------------------------------------------------------------------------
def bad_calls(ptr, out):
    """(what, the message's key words, spec or None, the five outputs, result given) of every PG_EINVAL;
    ptr: a matrix, out: an output address"""
    S = _capi.pg_reach_classes_spec
    ok = S(ptr, 1, 4, 4)
    both = (out, out, None, None, None)
    return [("null spec", "null spec", None, both, True), ("null result", "result", ok, both, False),
            ("null matrix", "null matrix", S(None, 1, 4, 4), both, True),
            ("no class output", "both null", ok, (None, None, out, out, None), True),
            ("quotient without dst", "out_quotient", ok, (out, None, None, None, out), True),
            ("quotient without src", "out_quotient", ok, (None, out, None, None, out), True),
            ("n_src", "2^20", S(ptr, 1, (1 << 20) + 1, 4), both, True), ("n_dst", "2^20", S(ptr, 1, 4, (1 << 20) + 1), both, True),
            ("n_svc", "4096", S(ptr, 4097, 4, 4), both, True),
            ("words", "2^32", S(ptr, 4096, 1 << 20, 16), both, True)]
