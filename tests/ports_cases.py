"""End points, fixture and oracle answers of the port-sweep tests (test helper).

Shared by tests/test_ports_host.py (pg_port_intervals and pg_debug_reach_ports_host, no GPU) and
tests/test_gpu_ports.py (pg_reach_ports on the device). Topologies and node sets come from
tests/node_matrix.py and sides from tests/reach_cases.py as they are; expected values come from
oracle.world.World.conn alone -- on every one of the 65,536 dst ports for the blocks, on the first
and the last port of every interval for the full sides. The interval bounds a case is compared on
are cuts(), computed here from the GetACLByName rules, never the engine's.

The fixture (fixture(variant)): four local pods p0..p3 on tap0..tap3, "lost" (no interface), "far"
(another node), and ACLs out-tap0, out-tap1, in-tap1, in-tap2 and g (node output). Variant "full"
spreads over them, on both protocols and with PERMIT, DENY and REFLECT: dst ranges 0..0,
65535..65535 and 0..65535; the adjacent 100..199 | 200..299; 1000..2000 (out-tap1) overlapping
1500..2500 (in-tap1); the single ports 80, 53, 443, 123; the empty 500..400; an upper bound of
65536 + 80 (10..80 as evalACL compares it: a cut at 81, none at 80 + 65536) and a lower bound of
65536 + 5000 (5000..6000). Variants "k16" / "k17": TCP ranges chosen for exactly 16 / 17 intervals
(the row_words boundary) and no UDP rule at all (K = 1).

A case (case(name, protocol)) is a topology or fixture variant swept on one protocol with src port
SPORT. Its block is 5 src x 7 dst end points holding local pods, a remote pod and non-pod addresses.
The topologies "grouped" and "wide" have outbound per-pod ACLs only and so no pair whose row mixes
ALLOW with another code: for them the helper builds the node_matrix topology again and adds five
inbound ACLs that reflect a port range (augmented()); the sets uni-grouped and uni-wide run on those
engines here (still a uniform node, narrow and wide records: test_ports_host.py asserts it).

Preconditions (Case.check_preconditions, on the oracle's output alone, before any product code
runs), with the floors measured on the CPU: at least 3 intervals (K below) and, over the full
37 x 53 sides at the intervals' first ports, at least 3 distinct ConnActions and at least
MIXED_FLOOR = 30 pairs whose row mixes ALLOW with another code. MEASURED has every case's (K,
ConnActions present, mixed pairs); the lowest are K = 9 (grouped, wide) and 32 mixed pairs (pair,
TCP). The K = 1 cases (k16 / k17 on UDP) are what they are for and take no precondition.
"""
import functools

import numpy as np

import node_matrix as nm
import reach_cases as rc
from oracle.world import World

SPORT = 40000
TCP, UDP = 0, 1
ALLOW = 2
SHAPES = ((1, 1), (1, 17), (3, 32), (37, 53), (64, 33))
MAX_SRC, MAX_DST = 64, 53
MIXED_FLOOR = 30
# (case, protocol) -> (K, ConnActions present over the 37 x 53 sides, pairs mixing ALLOW with another
# code), measured on the oracle alone (tests/test_ports_host.py::test_oracle_floors asserts them)
MEASURED = {
    ("full", TCP): (25, [0, 2, 3], 813), ("full", UDP): (14, [0, 1, 2, 3], 747),
    ("k16", TCP): (16, [0, 1, 2, 3], 309), ("k17", TCP): (17, [0, 1, 2, 3], 309),
    ("small", TCP): (51, [0, 1, 2, 3], 434), ("small", UDP): (57, [0, 1, 2, 3], 230),
    ("grouped", TCP): (9, [0, 1, 2, 3], 178), ("grouped", UDP): (9, [0, 1, 2, 3], 179),
    ("wide", TCP): (9, [0, 1, 2, 3], 176), ("wide", UDP): (9, [0, 1, 2, 3], 175),
    ("uncovered", TCP): (65, [0, 1, 2, 3], 308), ("uncovered", UDP): (148, [0, 1, 2, 3], 258),
    ("pair", TCP): (113, [0, 1, 2, 3], 32), ("pair", UDP): (129, [0, 1, 2, 3], 202),
    ("big-dst", TCP): (193, [0, 1, 2, 3], 100), ("big-dst", UDP): (193, [0, 1, 2, 3], 100),
}
SET_NAMES = rc.FORM_A_SETS + rc.FORM_B_SETS
FIXTURES = ("full", "k16", "k17")


def _l4(lo, hi):
    return {"src": [0, 65535], "dst": [lo, hi]}


def fixture_acls(variant):
    P, D, R = 1, 0, 2
    if variant in ("k16", "k17"):
        # 0..0 (a cut at 1), seven separate ranges (two cuts each): 16 intervals; k17: and 65535
        out0 = [{"action": P, "src": "", "dst": "", "tcp": _l4(0, 0)}]
        out0 += [{"action": (R, P, D)[k % 3], "src": "", "dst": "", "tcp": _l4(100 * k + 10, 100 * k + 19)}
                 for k in range(1, 8)]
        if variant == "k17":
            out0.append({"action": R, "src": "", "dst": "", "tcp": _l4(65535, 65535)})
        out0.append({"action": P, "src": "", "dst": "", "tcp": _l4(210, 219)})   # (cuts that exist already)
        return {"out-tap0": (out0 + [{"action": D, "src": "", "dst": ""}], [], ["tap0"]),
                "out-tap1": ([{"action": P, "src": "", "dst": "", "tcp": _l4(310, 319)},
                              {"action": P, "src": "10.30.0.1/32", "dst": ""}], [], ["tap1"]),
                "in-tap2": ([{"action": R, "src": "", "dst": ""}], ["tap2"], [])}
    out0 = [
        {"action": P, "src": "", "dst": "", "tcp": _l4(0, 0)},
        {"action": D, "src": "", "dst": "", "tcp": _l4(65535, 65535)},
        {"action": R, "src": "", "dst": "", "tcp": _l4(80, 80)},
        {"action": P, "src": "", "dst": "", "tcp": _l4(100, 199)},
        {"action": D, "src": "", "dst": "", "tcp": _l4(200, 299)},
        {"action": P, "src": "", "dst": "", "tcp": _l4(500, 400)},
        {"action": P, "src": "10.30.0.0/24", "dst": "", "tcp": _l4(10, 65536 + 80)},
        {"action": D, "src": "", "dst": "", "tcp": _l4(65536 + 5000, 6000)},
        {"action": P, "src": "", "dst": "", "udp": _l4(53, 53)},
        {"action": R, "src": "10.30.0.2/32", "dst": "", "udp": _l4(0, 65535)},
        {"action": P, "src": "", "dst": "", "tcp": _l4(32768, 65535)},
        {"action": P, "src": "", "dst": "", "udp": _l4(32768, 65535)},
        {"action": D, "src": "", "dst": ""},
    ]
    out1 = [
        {"action": R, "src": "", "dst": "", "tcp": _l4(1000, 2000)},
        {"action": P, "src": "10.30.0.1/32", "dst": "", "tcp": _l4(0, 65535)},
        {"action": D, "src": "", "dst": "", "udp": _l4(0, 0)},
        {"action": P, "src": "", "dst": "", "udp": _l4(65535, 65535)},
        {"action": P, "src": "", "dst": "", "tcp": _l4(32768, 61000)},
        {"action": R, "src": "", "dst": "", "udp": _l4(5050, 6000)},
    ]   # (no final rule: the table's default-deny slot is reachable)
    in1 = [
        {"action": D, "src": "", "dst": "", "tcp": _l4(1500, 2500)},
        {"action": R, "src": "", "dst": "", "udp": _l4(5000, 5100)},
        {"action": P, "src": "", "dst": ""},
    ]
    glob = [
        {"action": P, "src": "", "dst": "", "tcp": _l4(443, 443)},
        {"action": D, "src": "", "dst": "", "tcp": _l4(8080, 8081)},
        {"action": R, "src": "", "dst": "", "udp": _l4(123, 123)},
        {"action": P, "src": "10.30.0.0/28", "dst": "", "tcp": _l4(3000, 3999)},
        {"action": P, "src": "", "dst": "", "tcp": _l4(32768, 65535)},
        {"action": P, "src": "", "dst": "", "udp": _l4(40000, 40000)},
        {"action": D, "src": "", "dst": ""},
    ]
    return {"out-tap0": (out0, [], ["tap0"]), "out-tap1": (out1, [], ["tap1"]), "in-tap1": (in1, ["tap1"], []),
            "in-tap2": ([{"action": R, "src": "", "dst": ""}], ["tap2"], []), "g": (glob, [], [nm.NODE_IF])}


POD_IPS = [0x0A1E0001, 0x0A1E0002, 0x0A1E0003, 0x0A1E0004]
LOST, FAR = 0x0A1E0011, 0x0A1E0012
OTHER = [0x0A140105, 0x08080808, 0xC0A80101]


def fixture(variant="full"):
    """(engine, (local pods {ip: TAP}, pods without an interface), pod addresses), as
    node_matrix.TOPOLOGIES builders return it"""
    from vpp_amd import renderer as R
    from vpp_amd import workloads as W
    e = R.Engine(0)
    e.SetMainInterfaceName("GbE")
    e.SetVxlanBVIIfName(nm.NODE_IF)
    e.SetHostInterconnectIfName("VPP-Host")
    local = {}
    for k, ip in enumerate(POD_IPS):
        e.SetPodIfName("ns/p%d" % k, "tap%d" % k)
        e.RegisterPod("ns/p%d" % k, W.ip_str(ip), False)
        local[ip] = "tap%d" % k
    e.RegisterPod("ns/lost", W.ip_str(LOST), False)
    e.RegisterPod("ns/far", W.ip_str(FAR), True)
    ops = [("config/vpp/acls/v2/acl/" + n, {"name": n, "rules": rules, "ingress": ing, "egress": eg})
           for n, (rules, ing, eg) in fixture_acls(variant).items()]
    e.ApplyTxn(True, ops)
    return e, (local, [LOST]), POD_IPS + [LOST, FAR]


# node_matrix topologies whose ACLs give no pair a row that mixes ALLOW with another code (their
# per-pod ACLs are outbound only, so a SYN-ACK passes only where the SYN was reflected): augmented()
# adds inbound ACLs that reflect a port range on five of the pods the sides draw from
AUGMENTED = ("grouped", "wide")


def augmented(name):
    e, local, pod_ips = nm.TOPOLOGIES[name]()
    ops = []
    for k in (1, 3, 5, 7, 13):
        rules = [{"action": 2, "src": "", "dst": "", "tcp": _l4(8000, 8999)},
                 {"action": 2, "src": "", "dst": "", "udp": _l4(8500, 9499)},
                 {"action": 1, "src": "", "dst": ""}]
        ops.append(("config/vpp/acls/v2/acl/in-tap%d" % k, {"name": "in-tap%d" % k, "rules": rules,
                                                            "ingress": ["tap%d" % k], "egress": []}))
    e.ApplyTxn(False, ops)
    return e, local, pod_ips


class OwnTopo:
    """what the tests use of a node_matrix.Topology, for an engine built here"""

    def __init__(self, name):
        self.name, self.fixture = name, name in FIXTURES
        self.e, self.local, self.pod_ips = fixture(name) if self.fixture else augmented(name)
        self.e.num_tables()
        self.world = World(self.e, self.local[0], nm.NODE_IF, no_if_ips=self.local[1])


@functools.lru_cache(maxsize=None)
def topo(name):
    return OwnTopo(name) if name in FIXTURES + AUGMENTED else nm.topo(name)


def cuts(e, protocol):
    """the cut set of a protocol from the engine's installed rules as GetACLByName returns them: 0
    and, for every rule whose L4 section of that protocol has a dst range, lower & 0xFFFF and
    (upper & 0xFFFF) + 1 -- evalACL's own comparison bounds -- below 65536, ascending"""
    f = ("tcp", "udp")[protocol]
    s = {0}
    for n in e.ACLNames():
        for r in e.GetACLByName(n)["rules"]:
            sec = r.get(f)
            if sec and sec.get("dst") is not None:
                s |= {sec["dst"][0] & 0xFFFF, (sec["dst"][1] & 0xFFFF) + 1}
    return np.array(sorted(x for x in s if x < 65536), np.uint32)


def sides(t, n_src, n_dst):
    if getattr(t, "fixture", False):   # pods (local, lost, far) and non-pod addresses, interleaved
        pool = [POD_IPS[0], OTHER[0], POD_IPS[1], FAR, POD_IPS[2], OTHER[1], POD_IPS[3], LOST, OTHER[2]]
        return (np.array([pool[i % len(pool)] for i in range(n_src)], np.uint32),
                np.array([pool[(2 * i + 2) % len(pool)] for i in range(n_dst)], np.uint32))
    return rc.sides(t, n_src, n_dst)


def block_sides(t):
    """5 src x 7 dst: local pods, a remote pod and non-pod addresses on both sides"""
    if getattr(t, "fixture", False):
        return (np.array([POD_IPS[0], POD_IPS[1], POD_IPS[2], FAR, OTHER[1]], np.uint32),
                np.array([POD_IPS[1], POD_IPS[0], POD_IPS[3], LOST, FAR, OTHER[0], POD_IPS[2]], np.uint32))
    pods, other = rc.end_points(t)
    kind = t.world.kind(pods)
    loc = [p for p, k in zip(pods, kind) if k == 0 and p in t.local[0]]
    rem = [p for p, k in zip(pods, kind) if k == 1]
    assert len(loc) >= 4 and rem and len(other) >= 3
    return (np.array([loc[0], loc[1], rem[0], other[0], loc[2]], np.uint32),
            np.array([loc[1], loc[0], other[1], rem[0], loc[3], other[2], loc[2]], np.uint32))


def oracle_words(world, src, dst, protocol, ports, sport=SPORT):
    """verdict words (ConnAction << 30 | deciding slot) [n_src, n_dst, len(ports)] of the oracle"""
    ns, nd, k = len(src), len(dst), len(ports)
    if not ns or not nd or not k:
        return np.zeros((ns, nd, k), np.uint32)
    s, d = np.repeat(np.repeat(src, nd), k), np.repeat(np.tile(dst, ns), k)
    dp = np.tile(np.asarray(ports, np.uint16), ns * nd)
    n = len(s)
    act, slot = world.conn(s, d, np.full(n, sport, np.uint16), dp, np.full(n, protocol, np.uint8), threads=4)
    return ((act.astype(np.uint32) << 30) | slot.astype(np.uint32)).reshape(ns, nd, k)


def pack(actions):
    """the packed layout of pg_reach_ports from ConnActions [n_src, n_dst, K]: interval k in bits
    [2 (k & 15), 2 (k & 15) + 1] of word k >> 4 of the pair, padding bits zero"""
    ns, nd, k = actions.shape
    out = np.zeros((ns, nd, (k + 15) // 16), np.uint32)
    for i in range(k):
        out[:, :, i >> 4] |= actions[:, :, i].astype(np.uint32) << np.uint32(2 * (i & 15))
    return out


def lengths(lo):
    return np.diff(np.append(lo.astype(np.int64), 65536))


class Case:
    """a topology (or fixture variant) swept on one protocol: the bounds from its rules, and the
    oracle's words of the 64 x 53 sides (every shape is a prefix) at each interval's first and last
    port"""

    def __init__(self, name, protocol):
        self.name, self.protocol = name, protocol
        self.t = topo(name)
        self.lo = cuts(self.t.e, protocol)
        self.K = len(self.lo)
        self.hi = (self.lo.astype(np.int64) + lengths(self.lo) - 1).astype(np.uint32)
        self.src, self.dst = sides(self.t, MAX_SRC, MAX_DST)
        self.first = oracle_words(self.t.world, self.src, self.dst, protocol, self.lo)
        self.last = oracle_words(self.t.world, self.src, self.dst, protocol, self.hi)
        if (name, protocol) in MEASURED:   # (every case but the K = 1 ones)
            self.check_preconditions()

    def counts(self):
        act = self.first[:rc.N_SRC] >> 30
        allow = (act == ALLOW).any(axis=2)
        return self.K, sorted(np.unique(act).tolist()), int((allow & (act != ALLOW).any(axis=2)).sum())

    def check_preconditions(self):
        k, acts, mixed = self.counts()
        assert k >= 3 and len(acts) >= 3 and mixed >= MIXED_FLOOR, (self.name, self.protocol, k, acts, mixed)

    def shape(self, n_src, n_dst):
        """(src, dst, expected words [n_src, n_dst, K], expected open counts)"""
        w = self.first[:n_src, :n_dst]
        n_open = (((w >> 30) == ALLOW) * lengths(self.lo)).sum(axis=2).astype(np.uint32)
        return self.src[:n_src], self.dst[:n_dst], w, n_open

    @functools.lru_cache(maxsize=None)
    def block(self):
        """(src[5], dst[7], oracle words [5, 7, 65536]): every dst port"""
        src, dst = block_sides(self.t)
        return src, dst, oracle_words(self.t.world, src, dst, self.protocol, np.arange(65536))


@functools.lru_cache(maxsize=None)
def case(name, protocol):
    return Case(name, protocol)


def set_case(set_name, protocol):
    """(engine of a node set or fixture variant, its Case)"""
    if set_name in FIXTURES:
        return topo(set_name).e, case(set_name, protocol)
    spec = nm.SETS[set_name]
    if spec.topology in AUGMENTED:   # (uni-grouped, uni-wide: no compiler knobs)
        assert not spec.knobs
        return topo(spec.topology).e, case(spec.topology, protocol)
    return nm.node_set(set_name).e, case(spec.topology, protocol)


def mismatch_report(got, want, limit=5):
    bad = np.argwhere(got != want)
    return "%d of %d words differ; first (src, dst, interval): %s" % (
        len(bad), want.size, [(tuple(int(x) for x in b), hex(int(got[tuple(b)])), hex(int(want[tuple(b)]))) for b in bad[:limit]])
