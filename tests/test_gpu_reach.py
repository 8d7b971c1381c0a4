"""The reachability matrix on the device: pg_reach_matrix against the oracle over the sets and shapes
of tests/test_reach_host.py (tests/reach_cases.py: every pair of every case, nothing filtered), and
against pg_classify(CONN) on the materialised tuples.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import kat_driver as kd
import reach_cases as rc
from vpp_amd import device as D
from vpp_amd._capi import MODE_CONN

pytestmark = pytest.mark.gpu


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def run(e, src, dst, svc, stream=None):
    packed, words = D.reach_matrix(e, src, dst, svc, words=True, stream=stream)
    torch.cuda.synchronize()
    return u32(packed), u32(words)


def check(e, src, dst, svc, want):
    packed, words = run(e, src, dst, svc)
    assert (words == want).all(), rc.mismatch_report(words, want)
    assert (packed == rc.pack(want)).all(), "packed output differs from the words' top two bits"
    only = u32(D.reach_matrix(e, src, dst, svc))   # without out_words: the same packed words
    assert (only == packed).all()
    return words


@pytest.mark.parametrize("name", rc.FORM_A_SETS + rc.FORM_B_SETS)
def test_matrix_equals_oracle(name):
    s, c = rc.set_case(name)
    check(s.e, c.src, c.dst, c.svc, c.words)


def test_form_b_by_knob():
    s, c = rc.set_case("uni")
    with s.e.tuning(node_path=0):
        check(s.e, c.src, c.dst, c.svc, c.words)


@pytest.mark.parametrize("name", ("uni", "uni-wide"))
def test_equals_classify_device(name):
    """device against device: D.classify(CONN) on the materialised tuples (its ANY-protocol
    packets through k_node_any)"""
    s, c = rc.set_case(name)
    _, words = run(s.e, c.src, c.dst, c.svc)
    ns, nd = len(c.src), len(c.dst)
    n = ns * nd
    sa, da = np.repeat(c.src, nd), np.tile(c.dst, ns)
    for v, (pr, sp, dp) in enumerate(c.svc):
        b = D.TupleBatch.from_numpy(sa, da, np.full(n, sp, np.uint16), np.full(n, dp, np.uint16),
                                    np.full(n, pr & 0xFF, np.uint8))
        out = torch.empty(n, dtype=torch.int32, device="cuda")
        D.classify(s.e, MODE_CONN, -1, b, out)
        torch.cuda.synchronize()
        assert (u32(out) == words[v].ravel()).all(), (name, v)


@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ("uni", "pair"))
def test_shapes(name, shape):
    s, c = rc.set_case(name)
    for sel in (None, [1], c.any_services(), c.no_any_services()):
        src, dst, svc, want = c.shape(shape[0], shape[1], sel)
        check(s.e, src, dst, svc, want)


def test_grid_stride_rounds():
    """129 x 257 x 19 on big-uni under blocks_per_cu = 1: 629,907 full words (no multiple of 256 or
    64; rows of 257 words, so no 16-B stores) in 41,667 packed words, one lane each -- several
    grid-stride rounds of the grid of one 64-lane workgroup per CU"""
    s, c = rc.set_case("big-uni")
    src, dst = rc.sides(s.t, 129, 257)
    assert len(c.svc) == 19
    want = rc.oracle_words(s.t.world, src, dst, c.svc)
    assert want.size == 629907 and want.size % 64
    with s.e.tuning(blocks_per_cu=1):
        check(s.e, src, dst, c.svc, want)


def test_stream_and_prefill():
    """a non-default stream, out_packed and out_words pre-filled with 0xFF: padding bits zero, every
    word overwritten"""
    s, c = rc.set_case("uni")
    src, dst, svc, want = c.shape(37, 53)
    spec, keep = D.reach_spec(src, dst, svc)
    rw = D.reach_row_words(len(dst))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        packed = torch.full((len(svc), len(src), rw), -1, dtype=torch.int32, device="cuda")
        words = torch.full((len(svc), len(src), len(dst)), -1, dtype=torch.int32, device="cuda")
        s.e._ck(D.lib.pg_reach_matrix(s.e.h, C.byref(spec), packed.data_ptr(), words.data_ptr(), C.c_void_p(st.cuda_stream)))
    st.synchronize()
    del keep
    assert (u32(words) == want).all()
    assert (u32(packed) == rc.pack(want)).all()
    assert (u32(packed)[:, :, -1] >> np.uint32(2 * (len(dst) & 15)) == 0).all()   # the padding bits


def test_counters_untouched():
    s, c = rc.set_case("uni")
    e = s.e
    D.reset_counters(e)
    src, dst, sport, dport, proto = (a[:4099] for a in s.tup)
    b = D.TupleBatch.from_numpy(src, dst, sport, dport, proto)
    out = torch.empty(b.n, dtype=torch.int32, device="cuda")
    D.classify(e, MODE_CONN, -1, b, out, counters=D.counters_device_ptr(e))
    torch.cuda.synchronize()
    before = D.read_counters(e)
    snap = D.counters_snapshot(e)
    assert before.sum() > 0
    run(e, c.src, c.dst, c.svc)
    assert (D.counters_snapshot(e) == snap).all()
    assert (D.read_counters(e) == before).all()
    D.reset_counters(e)


def test_empty_sides():
    """a zero n_src, n_dst or n_svc: PG_OK, nothing written"""
    s, c = rc.set_case("uni")
    buf = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    for ns, nd, nv in ((0, 5, 3), (5, 0, 3), (5, 5, 0)):
        spec, keep = D.reach_spec(c.src[:ns], c.dst[:nd], c.svc[:nv])
        assert D.lib.pg_reach_matrix(s.e.h, C.byref(spec), buf.data_ptr(), buf.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == -1).all()
        assert D.reach_matrix(s.e, c.src[:ns], c.dst[:nd], c.svc[:nv]).shape == (nv, ns, (nd + 15) // 16)


def test_reachability_equals_connections():
    """Engine.reachability == Engine.connections PodToPod on the TestCombinedRules pods"""
    sc = [x for x in kd.load("acl_renderer_kats.json") if x["name"] == "TestCombinedRules"][0]
    prod = kd.ProductBackend(gpu=True)
    assert not kd.run_scenario(prod, sc)
    e = prod.engine
    pods = [p for p, _, _ in sc["setup"]["pods"]]
    svc = sorted({(kd.PROTO[c["args"][2]], c["args"][3], c["args"][4]) for ph in sc["phases"] for c in ph["checks"]
                  if c["kind"] == "ConnectionPodToPod"}) + [(3, 0, 0), (2, 0, 0)]
    got = e.reachability(pods, pods, svc)
    qs = [("PodToPod", a, b, pr, sp, dp) for (pr, sp, dp) in svc for a in pods for b in pods]
    want = np.array(e.connections(qs)[0], np.uint8).reshape(len(svc), len(pods), len(pods))
    assert (got == want).all()
    assert len(np.unique(got)) >= 2
