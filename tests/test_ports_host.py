"""The port sweep on the host (no GPU): pg_port_intervals, and pg_debug_reach_ports_host running the
per-pair code of pg_reach_ports (ports.hpp, the templates the kernel instantiates), against the
oracle (tests/ports_cases.py): every one of the 65,536 dst ports on the 5 x 7 blocks, the first and
the last port of every interval on the 37 x 53 sides of every set.
"""
import ctypes as C

import numpy as np
import pytest

import node_matrix as nm
import ports_cases as pc
import reach_cases as rc
from oracle.world import World
from vpp_amd import _capi
from vpp_amd import device as D
from vpp_amd import renderer as R
from vpp_amd._capi import lib

PROTOS = (pc.TCP, pc.UDP)
ALL_SETS = pc.FIXTURES + pc.SET_NAMES
ids = lambda v: {0: "tcp", 1: "udp"}.get(v, v) if isinstance(v, int) else v


@pytest.mark.parametrize("key", sorted(pc.MEASURED), ids=lambda k: "%s-%s" % (k[0], ("tcp", "udp")[k[1]]))
def test_oracle_floors(key):
    """the helper's recipe on the oracle alone: the preconditions and the measured counts"""
    c = pc.case(*key)
    c.check_preconditions()
    assert c.counts() == pc.MEASURED[key]
    assert (c.first == c.last).all()   # the oracle itself: one word per (pair, interval)


# ---- partition ------------------------------------------------------------------------------
def bounds_allowed(e, protocol):
    """every value a cut may have (condition 2) and the number of rules with that L4 section"""
    f, vals, n = ("tcp", "udp")[protocol], set(), 0
    for name in e.ACLNames():
        for r in e.GetACLByName(name)["rules"]:
            sec = r.get(f)
            if sec and sec.get("dst") is not None:
                vals |= {sec["dst"][0] & 0xFFFF, (sec["dst"][1] & 0xFFFF) + 1}
                n += 1
    return vals, n


@pytest.mark.parametrize("protocol", PROTOS, ids=ids)
@pytest.mark.parametrize("name", ALL_SETS)
def test_partition(name, protocol):
    e, c = pc.set_case(name, protocol)
    lo = e.port_intervals(protocol)
    assert lo.dtype == np.uint32 and lo[0] == 0 and (np.diff(lo.astype(np.int64)) > 0).all() and lo[-1] <= 65535
    vals, n_rules = bounds_allowed(e, protocol)
    assert set(lo[1:].tolist()) <= vals and len(lo) <= 2 * n_rules + 1      # no gratuitous cuts
    assert np.array_equal(lo, c.lo)                                          # the helper's own cut set
    # exact, on the oracle: the words at an interval's two ends agree (all ports: the blocks below)
    assert (c.first == c.last).all()
    # a short buffer gets the first bounds, the return value is K all the same
    buf = np.full(3, 0xFFFFFFFF, np.uint32)
    assert lib.pg_port_intervals(e.h, protocol, buf.ctypes.data_as(C.c_void_p), 2) == len(lo)
    assert buf[:2].tolist() == lo[:2].tolist() + [0xFFFFFFFF] * (2 - min(2, len(lo))) and buf[2] == 0xFFFFFFFF


def test_fixture_bounds():
    """the fixture's cut sets as its docstring promises them"""
    t = pc.topo("full")
    tcp, udp = (t.e.port_intervals(p).tolist() for p in PROTOS)
    for want in (0, 1, 65535, 80, 81, 100, 200, 300, 10, 1000, 1500, 2001, 2501, 443, 444, 5000, 6001):
        assert want in tcp, want
    assert not {65536 + 80, 65536 + 81} & set(tcp) and max(tcp) <= 65535
    for want in (0, 1, 53, 54, 65535, 123, 124, 5000, 5050, 5101, 6001, 40000, 40001):
        assert want in udp, want
    assert [len(pc.topo(v).e.port_intervals(pc.TCP)) for v in ("k16", "k17")] == [16, 17]
    assert [pc.topo(v).e.port_intervals(pc.UDP).tolist() for v in ("k16", "k17")] == [[0], [0]]


@pytest.mark.parametrize("variant", pc.FIXTURES)
def test_partition_exact_per_acl(variant):
    """evalACL through the oracle over all 65,536 ports, every ACL of the fixture, three src / dst
    draws, both protocols: (action, rule) is constant inside each interval"""
    t = pc.topo(variant)
    ports = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    draws = ((pc.POD_IPS[0], pc.POD_IPS[1]), (pc.POD_IPS[1], pc.POD_IPS[0]), (pc.OTHER[1], pc.POD_IPS[2]))
    for protocol in PROTOS:
        lo = t.e.port_intervals(protocol)
        iv = np.searchsorted(lo, np.arange(65536), side="right") - 1
        for name in t.e.ACLNames():
            for src, dst in draws:
                act, slot = t.world.single(t.e.table_id(name), np.full(65536, src, np.uint32),
                                           np.full(65536, dst, np.uint32), ports, np.full(65536, protocol, np.uint8))
                w = (act.astype(np.int64) << 32) | slot.astype(np.int64)
                assert (w == w[lo][iv]).all(), (variant, protocol, name)


def test_partition_errors_and_no_acls():
    e = R.Engine(0)
    assert e.port_intervals(pc.TCP).tolist() == [0] and e.port_intervals(pc.UDP).tolist() == [0]
    for bad in (2, 3, -1, 255):
        assert lib.pg_port_intervals(e.h, bad, None, 0) == _capi.PG_EINVAL
    assert lib.pg_port_intervals(None, 0, None, 0) == _capi.PG_EINVAL


# ---- the sweep ------------------------------------------------------------------------------
def check_padding(codes, k):
    if k & 15:
        assert (codes[:, :, -1] >> np.uint32(2 * (k & 15)) == 0).all(), "padding bits set"


@pytest.mark.parametrize("protocol", PROTOS, ids=ids)
@pytest.mark.parametrize("name", ("full", "uni", "pair"))
def test_block_every_port(name, protocol):
    """5 x 7 end points x 65,536 dst ports: out_words expanded by interval, out_codes expanded by the
    bounds and out_open, each against World.conn at every port"""
    e, c = pc.set_case(name, protocol)
    src, dst, want = c.block()
    kinds = set(c.t.world.kind(np.concatenate([src, dst])).tolist())
    assert kinds == {0, 1, 2}, kinds   # local pods, a remote pod, non-pod addresses
    lo, codes, n_open, words = e.debug_reach_ports_host(src, dst, protocol, pc.SPORT)
    assert np.array_equal(lo, c.lo)
    ln = pc.lengths(lo)
    assert (np.repeat(words, ln, axis=2) == want).all()
    act = D.unpack_ports(codes, len(src), len(dst), len(lo))
    assert (np.repeat(act, ln, axis=2) == (want >> 30)).all()
    assert (n_open == ((want >> 30) == pc.ALLOW).sum(axis=2)).all()
    assert n_open.max() > 0 and n_open.min() < 65536
    check_padding(codes, len(lo))


@pytest.mark.parametrize("protocol", PROTOS, ids=ids)
@pytest.mark.parametrize("name", ALL_SETS)
def test_full_sides(name, protocol):
    """37 x 53: the oracle's words at every interval's first and last port"""
    e, c = pc.set_case(name, protocol)
    if name in rc.FORM_A_SETS:
        ns = e.node_stats()
        assert ns["uniform"] and bool(ns["wide_records"]) == (name == "uni-wide")
    elif name in rc.FORM_B_SETS:
        assert not e.node_stats()["uniform"]
    src, dst, want, want_open = c.shape(rc.N_SRC, rc.N_DST)
    assert (c.last[:rc.N_SRC, :rc.N_DST] == want).all()
    outs = {}
    for node in (True, False):   # flags 1 and 0
        lo, codes, n_open, words = e.debug_reach_ports_host(src, dst, protocol, pc.SPORT, node=node)
        assert np.array_equal(lo, c.lo)
        assert (words == want).all(), pc.mismatch_report(words, want)
        assert (codes == pc.pack(want >> 30)).all()
        assert (n_open == want_open).all()
        check_padding(codes, c.K)
        outs[node] = (codes, n_open, words)
    assert all((a == b).all() for a, b in zip(outs[True], outs[False]))
    if e.node_stats()["uniform"]:
        with e.tuning(node_path=0):
            got = e.debug_reach_ports_host(src, dst, protocol, pc.SPORT)[1:]
        assert all((a == b).all() for a, b in zip(outs[True], got))


@pytest.mark.parametrize("shape", pc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_and_interval_tails(shape):
    """every shape on K = 1 (k16, UDP), 16, 17 and the fixture's full K = 25"""
    for name, protocol in (("k16", pc.UDP), ("k16", pc.TCP), ("k17", pc.TCP), ("full", pc.TCP)):
        e, c = pc.set_case(name, protocol)
        src, dst, want, want_open = c.shape(*shape)
        lo, codes, n_open, words = e.debug_reach_ports_host(src, dst, protocol, pc.SPORT)
        assert len(lo) == c.K and (words == want).all() and (codes == pc.pack(want >> 30)).all()
        assert (n_open == want_open).all()
        check_padding(codes, c.K)


def test_equals_classify_host():
    """out_words == pg_debug_classify_host CONN on the materialised tuples (src, dst, sport, lo[k])"""
    for name in ("uni", "pair"):
        e, c = pc.set_case(name, pc.TCP)
        src, dst = c.src[:9], c.dst[:11]
        lo, _, _, words = e.debug_reach_ports_host(src, dst, pc.TCP, pc.SPORT)
        n = len(src) * len(dst) * len(lo)
        sa, da = np.repeat(np.repeat(src, len(dst)), len(lo)), np.repeat(np.tile(dst, len(src)), len(lo))
        got = e.debug_classify_host(_capi.MODE_CONN, -1, sa, da, np.full(n, pc.SPORT, np.uint16),
                                    np.tile(lo.astype(np.uint16), len(src) * len(dst)), np.zeros(n, np.uint8))
        assert (got == words.ravel()).all()


def test_src_port_is_the_syn_ack_key():
    """another src port moves the verdicts where a rule's range holds one and not the other"""
    e, c = pc.set_case("full", pc.TCP)
    src, dst, _, _ = c.shape(9, 9)
    a = e.debug_reach_ports_host(src, dst, pc.TCP, pc.SPORT)[3]
    b = e.debug_reach_ports_host(src, dst, pc.TCP, 300)[3]
    assert (a != b).any()
    assert (b == pc.oracle_words(c.t.world, src, dst, pc.TCP, c.lo, sport=300)).all()


# ---- errors ---------------------------------------------------------------------------------
def test_empty_sides_write_nothing():
    e, c = pc.set_case("full", pc.TCP)
    for ns, nd in ((0, 5), (5, 0), (0, 0)):
        spec, keep = D.ports_spec(c.src[:ns], c.dst[:nd], pc.TCP, pc.SPORT, c.K)
        buf = np.full(64, 0xFFFFFFFF, np.uint32)
        p = buf.ctypes.data_as(C.c_void_p)
        assert lib.pg_debug_reach_ports_host(e.h, C.byref(spec), p, p, p, 1) == 0
        assert lib.pg_reach_ports(e.h, C.byref(spec), p, p, p, None) == 0   # (returns before any device work)
        assert (buf == 0xFFFFFFFF).all()
        del keep


def test_einval():
    e = pc.fixture("full")[0]   # an engine of this test's own: it commits below
    c = pc.case("full", pc.TCP)
    buf = np.zeros(4096, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    calls = ((lambda s, out: lib.pg_debug_reach_ports_host(e.h, s, out, None, None, 1)),
             (lambda s, out: lib.pg_reach_ports(e.h, s, out, None, None, None)))
    for call in calls:   # (every check precedes the first device call)
        good, keep = D.ports_spec(c.src[:2], c.dst[:2], pc.TCP, pc.SPORT, c.K)
        assert call(None, p) == _capi.PG_EINVAL
        assert call(C.byref(good), None) == _capi.PG_EINVAL
        for field, v in (("protocol", 2), ("protocol", 3), ("protocol", -1), ("n_src", (1 << 20) + 1),
                         ("n_dst", (1 << 20) + 1), ("n_intervals", c.K - 1), ("n_intervals", c.K + 1)):
            bad, _ = D.ports_spec(c.src[:2], c.dst[:2], pc.TCP, pc.SPORT, c.K)
            setattr(bad, field, v)
            assert call(C.byref(bad), p) == _capi.PG_EINVAL, (field, v)
        # 2^16 x 2^15 pairs x row_words(25) = 2 words: 2^32
        big, _ = D.ports_spec(c.src[:2], c.dst[:2], pc.TCP, pc.SPORT, c.K)
        big.n_src, big.n_dst = 1 << 16, 1 << 15
        assert call(C.byref(big), p) == _capi.PG_EINVAL
        assert "2^32" in lib.pg_last_error(e.h).decode()
        del keep
    # a commit that adds a port rule: the caller's K is stale
    acl = e.GetACLByName("in-tap2")
    acl["rules"].insert(0, {"action": 0, "src": "", "dst": "", "tcp": {"src": [0, 65535], "dst": [7000, 7007]}})
    e.ApplyTxn(False, [("config/vpp/acls/v2/acl/in-tap2", acl)])
    assert len(e.port_intervals(pc.TCP)) == c.K + 2
    for call in calls:
        stale, keep = D.ports_spec(c.src[:2], c.dst[:2], pc.TCP, pc.SPORT, c.K)
        assert call(C.byref(stale), p) == _capi.PG_EINVAL
        msg = lib.pg_last_error(e.h).decode()
        assert "n_intervals" in msg and str(c.K + 2) in msg and "changed" in msg, msg
        del keep
    # and with the new K the sweep is the new oracle's
    lo, _, _, words = e.debug_reach_ports_host(c.src[:9], c.dst[:9], pc.TCP, pc.SPORT)
    t = pc.topo("full")
    want = pc.oracle_words(World(e, t.local[0], nm.NODE_IF, no_if_ips=t.local[1]), c.src[:9], c.dst[:9], pc.TCP, lo)
    assert len(lo) == c.K + 2 and (words == want).all()


# ---- Engine.open_ports ------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", PROTOS, ids=ids)
def test_open_ports(protocol):
    """merged ALLOW ranges per pod pair == the ranges merged from the oracle's per-port actions"""
    t = pc.topo("full")
    pods = ["ns/p%d" % k for k in range(4)] + ["ns/far"]
    ips = np.array(pc.POD_IPS + [pc.FAR], np.uint32)
    ranges, n_open = t.e.open_ports(pods, pods[:4], protocol, src_port=pc.SPORT, host=True)
    want = pc.oracle_words(t.world, ips, ips[:4], protocol, np.arange(65536)) >> 30
    some = 0
    for i in range(len(pods)):
        for j in range(4):
            a = np.pad((want[i, j] == pc.ALLOW).astype(np.int8), 1)
            edge = np.diff(a)
            merged = list(zip(np.nonzero(edge == 1)[0].tolist(), (np.nonzero(edge == -1)[0] - 1).tolist()))
            assert ranges[i][j] == merged, (i, j, ranges[i][j][:4], merged[:4])
            assert n_open[i, j] == sum(hi - lo + 1 for lo, hi in merged)
            some += len(merged) > 1
    assert some >= 3   # pairs with several separate open ranges
    with pytest.raises(R.PolicyError):
        t.e.open_ports(["ns/nobody"], pods, protocol, host=True)
