"""Pod layouts that put end-point resolution -- IPv4 address -> (interface, its two ACLs, kind) -- at
its edges, their probe addresses and what the oracle says of them (test helper).

Shared by tests/test_endpoint_host.py (no GPU) and tests/test_gpu_endpoints.py (the same products on
the device). Two structures resolve an address: the open-addressing end-point hash (engine.cpp
compile, classify.hpp probe_q: the per-table path, form B of the reachability audits, the node
kernels' ANY-protocol pass) and the node classifier's IPv4 trie (fastpath.cpp build_node). Every
other topology of the suite registers its pods at consecutive addresses, so neither is ever asked
about a collision chain, a wrap, a long miss, the ends of the address space or a deep trie.

A layout is a list of pods (name, address, kind), the kinds cycling LOCAL, LOCAL, NOIF (a pod of this
node without an interface), REMOTE, LOCAL. Its engine has VXLAN-BVI as node interface with the global
ACL "g" on it; local pod k has a TAP and an outbound ACL "out-k" of its own, every second one also an
inbound "in-k" (pod_acls: port bounds, actions and rule order differ from pod to pod, and being
separate tables their slots do anyway: an address resolved to the wrong pod changes the deciding
slot). Names are ns/p0000, ns/p0001, ...: the engine's PodID order is the list's order.

Layouts (LAYOUTS):
  chain          nine pods whose probes all start at one cell (CHAIN_SLOT) of the 64-cell table, found
                 by scanning 10.0.0.0/12 with hash_ip below; misses: a non-pod address starting at each
                 of the chain's nine cells (9 .. 1 steps) and one at the cell behind it
  wrap           the same with the chain starting three cells before the table's end
  extremes       pods at 0.0.0.0, 0.0.0.1, 127.255.255.255, 128.0.0.0, 255.255.255.254, 255.255.255.255
  adjacent       10.15.255.253 .. 10.16.0.4 but 10.16.0.0 (a non-pod gap): across a /24, a /16 and a
                 2^20 boundary (the node trie's widest root stride)
  on-rule-edges  pods on the first and last address of the /24, /28, /31 and /32 that the rules of
                 "g" and of pod 0's ACLs name as src and dst nets; one outside each: non-pods
  growth-N       N = 0, 1, 8, 9, 24, 25, 56, 57 pods from the seeded generator (scattered()): either
                 side of each doubling of the table (32, 64, 128, 256 cells)
  scattered-small / scattered-big   SCATTERED_SMALL / SCATTERED_BIG pods from the same generator: the most
                 for which the engine still builds a node classifier and the fewest for which it does
                 not (bisected on the CPU: bisect_scattered())
  repeat         pods that share an address, in both registration orders: local + remote, local +
                 no interface, two locals on different TAPs (the last in PodID order wins)

Probe set: every pod address, its two neighbours (mod 2^32), the layout's misses and two Internet
hosts; the product is every ordered pair over SERVICES (TCP 80, UDP 53, OTHER, ANY). The scattered
layouts take every pod address as dst and, as src, every pod address (an inbound ACL's rules decide
only where its pod is the src), the neighbours of SCATTERED_SRC evenly spaced pods and the Internet
hosts: 88k tuples.

Expected values come from oracle.world.World alone. pg_debug_endpoint_probe and the hash_ip
restated here only pick addresses and show that they reach the case they are named for; no expected
value comes from either.

Preconditions (Layout.check_preconditions, before any product answer is read): chain / wrap: a hit
and a miss of at least 9 probe steps, wrap: a hit and a miss that pass from the last cell to cell 0;
layouts with two local pods or more: every ConnAction at least ACTION_FLOOR (20) times, every rule
and default slot of the ACLs of every TAP an address resolves to deciding a tuple; and
sensitivity(): every single-end-point mutation of the World -- a pod dropped, moved by +1 or -1, two
pods' end points exchanged, a pod's kind changed -- changes the oracle's CONN words (MUTATIONS
holds the counts; all of them are seen).
"""
import copy
import functools

import numpy as np

import node_matrix as nm
import reach_cases as rc
import rules_cases as kr
from oracle.world import World, winners
from vpp_amd._capi import MODE_CONN, MODE_PERPOD

M32 = 0xFFFFFFFF
LOCAL, NOIF, REMOTE = "local", "noif", "remote"
KIND_CYCLE = (LOCAL, LOCAL, NOIF, REMOTE, LOCAL)
NODE_IF = nm.NODE_IF
TCP, UDP, OTHER, ANY = 0, 1, 2, 3
SPORT_TCP, SPORT_UDP = 40000, 40001
SERVICES = [(TCP, SPORT_TCP, 80), (UDP, SPORT_UDP, 53), (OTHER, 0, 0), (ANY, 0, 0)]
INTERNET = (0x08080808, 0xC6336407)   # 8.8.8.8, 198.51.100.7
ACTION_FLOOR = 20
SEED = 2024
CHAIN_LEN, CHAIN_CAP = 9, 64
CHAIN_SLOT, WRAP_SLOT = 20, CHAIN_CAP - 3
GROWTH = (0, 1, 8, 9, 24, 25, 56, 57)
# the end-point table's cells for that many pods (engine.cpp: the first power of two >= 2 n + 16)
GROWTH_CAP = {0: 16, 1: 32, 8: 32, 9: 64, 24: 64, 25: 128, 56: 128, 57: 256}
# bisect_scattered(): a node classifier for every count up to the first, none from the second on
SCATTERED_SMALL, SCATTERED_BIG = 112, 113
SCATTERED_SRC = 40


def hash_ip(ip):
    """classify.hpp hash_ip over a uint32 array -- to search for addresses only"""
    x = np.asarray(ip, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def ip_str(ip):
    return "%d.%d.%d.%d" % (ip >> 24, ip >> 16 & 255, ip >> 8 & 255, ip & 255)


def _l4(lo, hi):
    return {"src": [0, 65535], "dst": [lo, hi]}


def pod_acls(k, tap):
    """the ACLs of local pod k: "out-k" (egress on its TAP: evaluated for packets to the pod) and for
    even k "in-k" (ingress: packets from it). Rule 0's action cycles permit, deny, reflect; the rules'
    protocol order alternates; the port bounds move with k. No rule is without an L4 section, so
    OTHER packets reach every default slot; an ANY packet matches rule 0."""
    p, act = k % 13, (1, 0, 2)[k % 3]
    tcp, udp = {"src": "", "dst": "", "tcp": _l4(80 - p % 5, 80 + p)}, {"src": "", "dst": "", "udp": _l4(53 - p % 7, 53 + p)}
    first, second = (tcp, udp) if k % 2 == 0 else (udp, tcp)
    out = [dict(first, action=act), dict(second, action=0)]
    ops = [("config/vpp/acls/v2/acl/out-%d" % k, {"name": "out-%d" % k, "rules": out, "ingress": [], "egress": [tap]})]
    if k % 2 == 0:
        # rule 0 decides as the last evaluation only where the pod's outbound rule 0 lets an ANY packet
        # through to it (permit) and the src side reflected -- or by denying
        inb = [dict(tcp, action=2 if act == 1 else 0, tcp=_l4(80 - p % 3, 80 + p % 11)), dict(udp, action=0)]
        ops.append(("config/vpp/acls/v2/acl/in-%d" % k, {"name": "in-%d" % k, "rules": inb, "ingress": [tap], "egress": []}))
    return ops


EDGE_NETS = ("10.40.7.0/24", "10.40.9.16/28", "10.40.11.6/31", "10.40.13.77/32")


def _net_ends(cidr):
    ip, ln = cidr.split("/")
    a, b, c, d = (int(x) for x in ip.split("."))
    net, ln = a << 24 | b << 16 | c << 8 | d, int(ln)
    return net, net | (M32 >> ln)


def global_acl(edges=False):
    """"g", egress on the node interface: what leaves for a remote pod or a non-pod address, and the
    SYN-ACKs towards one. edges: in front, a rule per EDGE_NETS net as src and one as dst"""
    rules = []
    if edges:
        for j, net in enumerate(EDGE_NETS):
            rules.append({"action": j % 2, "src": net, "dst": "", "tcp": _l4(80, 80)})
            rules.append({"action": 1 - j % 2, "src": "", "dst": net, "udp": _l4(53, 53)})
    rules += [{"action": 1, "src": "", "dst": "", "tcp": _l4(SPORT_TCP, SPORT_TCP)},
              {"action": 0, "src": "", "dst": "", "udp": _l4(SPORT_UDP, SPORT_UDP)},
              {"action": 1, "src": "", "dst": "", "tcp": _l4(80, 80)},
              {"action": 2, "src": "", "dst": "", "udp": _l4(53, 53)}]
    return ("config/vpp/acls/v2/acl/g", {"name": "g", "rules": rules, "ingress": [], "egress": [NODE_IF]})


def edge_pod_acls():
    """on-rule-edges: pod 0's ACLs with the EDGE_NETS nets as src (outbound) and dst (inbound) in front"""
    ops = pod_acls(0, "tap0")
    for key, acl in ops:
        field = "src" if acl["egress"] else "dst"
        # (inbound: all deny, the pod's own first rule too -- every pod here lies in one of the nets, so a
        # permit in this inbound ACL is the last evaluation of no connection)
        if field == "dst":
            acl["rules"][0]["action"] = 0
        acl["rules"] =[dict({"action": (j + 1) % 2 if field == "src" else 0, "src": "", "dst": "", "tcp": _l4(80, 80)},
                             **{field: net}) for j, net in enumerate(EDGE_NETS)] + acl["rules"]
    return ops


# ---- addresses ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scan():
    ips = np.arange(0x0A000000, 0x0A100000, dtype=np.uint32)   # 10.0.0.0/12
    return ips, hash_ip(ips) & np.uint32(CHAIN_CAP - 1)


def chain_addresses(slot):
    """(nine pod addresses whose probes start at `slot`, ten miss addresses: one starting at each of
    the chain's cells, one at the cell behind it) from 10.0.0.0/12, every seventh candidate so that
    no two are neighbours"""
    ips, cell = _scan()
    pods = [int(x) for x in ips[cell == slot][::7][:CHAIN_LEN]]
    miss = [int(ips[cell == (slot + j) % CHAIN_CAP][::7][CHAIN_LEN + 1]) for j in range(CHAIN_LEN + 1)]
    return pods, miss


@functools.lru_cache(maxsize=None)
def scattered(n):
    """the first n addresses of the seeded generator: distinct, no two neighbours, none an INTERNET host"""
    g = np.random.default_rng(SEED)
    out, seen = [], set(INTERNET)
    while len(out) < n:
        x = int(g.integers(0, 1 << 32))
        if not {x, (x + 1) & M32, (x - 1) & M32, (x + 2) & M32, (x - 2) & M32} & seen:
            out.append(x)
            seen.add(x)
    return out


def _cycle(addresses, start=0):
    return [("ns/p%04d" % (start + i), ip, KIND_CYCLE[(start + i) % 5]) for i, ip in enumerate(addresses)]


def layout_pods(name):
    """-> (pods [(name, address, kind)], miss addresses)"""
    if name in ("chain", "wrap"):
        pods, miss = chain_addresses(CHAIN_SLOT if name == "chain" else WRAP_SLOT)
        return _cycle(pods), miss
    if name == "extremes":
        return _cycle([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]), []
    if name == "adjacent":
        first = 0x0A0FFFFD
        return _cycle([first + i for i in range(8) if i != 3]), [first + 3]
    if name == "on-rule-edges":
        ends = [x for net in EDGE_NETS for x in sorted(set(_net_ends(net)))]
        out = [x for net in EDGE_NETS for lo, hi in [_net_ends(net)] for x in (lo - 1, hi + 1)]
        return _cycle(ends), [x for x in out if x not in ends]
    if name.startswith("growth-"):
        return _cycle(scattered(int(name[7:]))), []
    if name.startswith("scattered-"):
        n = {"small": SCATTERED_SMALL, "big": SCATTERED_BIG}.get(name[10:]) or int(name[10:])
        return _cycle(scattered(n)), []
    if name == "repeat":
        a = [0x0A320001 + 16 * j for j in range(6)]
        # (first registered, second) per shared address: the second wins, whatever its kind
        pairs = [(LOCAL, REMOTE), (REMOTE, LOCAL), (LOCAL, NOIF), (NOIF, LOCAL), (LOCAL, LOCAL), (LOCAL, LOCAL)]
        pods = []
        for ip, (k1, k2) in zip(a, pairs):
            pods += [("ns/p%04d" % len(pods), ip, k1), ("ns/p%04d" % (len(pods) + 1), ip, k2)]
        return pods + _cycle([0x0A320101, 0x0A320103, 0x0A320105, 0x0A320107], len(pods)), []
    raise KeyError(name)


LAYOUTS = ("chain", "wrap", "extremes", "adjacent", "on-rule-edges") + tuple("growth-%d" % n for n in GROWTH) + (
    "scattered-small", "scattered-big", "repeat")


def build_engine(pods, edges=False, engine=None):
    """the engine of a layout -> (engine, registrations for oracle.world.World(pods=...)); engine: an
    existing one whose pods are a prefix-compatible superset (resync: only the ACLs are replaced)"""
    from vpp_amd import renderer as R
    e = engine or R.Engine(0)
    if engine is None:
        e.SetMainInterfaceName("GbE")
        e.SetVxlanBVIIfName(NODE_IF)
        e.SetHostInterconnectIfName("VPP-Host")
    ops, regs, k = [], [], 0
    for name, ip, kind in pods:
        tap = None
        if kind == LOCAL:
            tap = "tap%d" % k
            if engine is None:
                e.SetPodIfName(name, tap)
            ops += edge_pod_acls() if edges and k == 0 else pod_acls(k, tap)
            k += 1
        if engine is None:
            e.RegisterPod(name, ip_str(ip), kind == REMOTE)
        regs.append((name, ip, tap, kind == REMOTE))
    ops.append(global_acl(edges))
    e.ApplyTxn(True, ops)
    e.num_tables()
    return e, regs


class Layout:
    def __init__(self, name):
        self.name = name
        self.pods, self.miss = layout_pods(name)
        self.e, self.regs = build_engine(self.pods, edges=name == "on-rule-edges")
        self.world = World(self.e, None, NODE_IF, pods=self.regs)
        self.n_slots = self.e.num_counter_slots()
        self.pod_ips = sorted({ip for _, ip, _ in self.pods})
        self.n_local = len(self.world.local_ips[self.world.local_if >= 0])
        self.src, self.dst = self.sides()
        # the oracle, once: CONN words and histograms per service slice, PERPOD over the flat product
        self.words = rc.oracle_words(self.world, self.src, self.dst, SERVICES)
        self.ev, self.ce = kr.slice_hists(self.world, self.src, self.dst, SERVICES)
        self.tup = self.flat(self.src, self.dst)
        s, d, sp, dp, pr = self.tup
        act, slot = self.world.perpod(s, d, dp, pr, threads=4)
        self.exp = {MODE_PERPOD: (act.astype(np.uint32), slot.astype(np.uint32),
                                  np.bincount(slot, minlength=self.n_slots).astype(np.uint64)),
                    MODE_CONN: ((self.words >> 30).ravel(), (self.words & 0x3FFFFFFF).ravel(),
                                self.ev.sum(axis=0, dtype=np.uint64))}
        self.rec = np.arange(len(s))   # (what test_gpu_edges.compare prints of a mismatch: its position)

    def scattered(self):
        return self.name.startswith("scattered-")

    def sides(self):
        nb = lambda ips: [x for ip in ips for x in ((ip - 1) & M32, (ip + 1) & M32)]   # noqa: E731
        if self.scattered():
            pick = [self.pod_ips[j] for j in np.unique(np.round(np.linspace(0, len(self.pod_ips) - 1, SCATTERED_SRC)).astype(np.int64))]
            return (np.array(self.pod_ips + nb(pick) + list(INTERNET), np.uint32), np.array(self.pod_ips, np.uint32))
        seen, side = set(), []
        for ip in self.pod_ips + nb(self.pod_ips) + self.miss + list(INTERNET):
            if ip not in seen:
                seen.add(ip)
                side.append(ip)
        side = np.array(side, np.uint32)
        return side, side

    @staticmethod
    def flat(src, dst):
        """the product as tuples, in the order of the words [service, src, dst]"""
        ns, nd, nv = len(src), len(dst), len(SERVICES)
        col = lambda k, dt: np.repeat(np.array([v[k] for v in SERVICES], dt), ns * nd)   # noqa: E731
        return (np.tile(np.repeat(src, nd), nv), np.tile(np.tile(dst, ns), nv), col(1, np.uint16), col(2, np.uint16),
                col(0, np.uint8))

    def expected(self, mode):
        return self.exp[mode]

    def launch(self, name, counters):
        """Tuning launch knobs of edge_cases.NODE_LAUNCHES for this engine (which has a node): "default",
        "stage0" (node_matrix's shape: nothing of the image staged), "per-table" (node_path = 0)"""
        if name == "default":
            return {}
        if name == "per-table":
            return {"node_path": 0}
        ns = self.e.node_stats()
        if ns is None:   # (no node: every launch is the per-table path)
            return {"node_stage_max_words": 0}
        if ns["image_bytes"] - ns["list_record_bytes"] * ns["list_records_in_image"] > ns["base_image_bytes"]:   # a section
            hist = (self.n_slots + 2) * 4 if counters else 0
            # (an image past the knob's range, 160 KiB, is staged by no launch anyway)
            return {"node_common_lds_max": min(hist + ns["base_image_bytes"], 160 << 10), "node_stage_max_words": 0}
        return {"node_stage_max_words": 0}

    def check_plan(self, name, mode, counters):
        p = self.e.debug_node_launch_plan(mode, counters)
        assert p["path"] == ("per-table" if name == "per-table" or not self.has_node() else "node"), (self.name, name, p)
        assert name != "stage0" or p["stage"] & 7 == 0, (self.name, name, p)
        return p

    def has_node(self):
        return self.e.node_stats() is not None

    # ---- preconditions ---------------------------------------------------------------------------
    def probe_facts(self):
        """{hit: most probe steps of a pod address, miss: of a non-pod probe address, wrap_hit / wrap_miss:
        whether one passes from the last cell to cell 0, cap} by pg_debug_endpoint_probe"""
        ips = np.unique(np.concatenate([self.src, self.dst]))
        steps, slot, cap = self.e.debug_endpoint_probe(ips)
        pod = np.isin(ips, self.pod_ips)
        wraps = slot.astype(np.int64) + steps - 1 >= cap
        mx = lambda m: int(steps[m].max()) if m.any() else 0   # noqa: E731
        return {"hit": mx(pod), "miss": mx(~pod), "wrap_hit": bool((wraps & pod).any()), "wrap_miss": bool((wraps & ~pod).any()),
                "cap": cap}

    def resolved_taps(self):
        return sorted({tap for tap, another in winners(self.regs).values() if tap and not another})

    def undecided(self):
        """rule and default slots, of the ACLs of the TAPs an address resolves to, that are the deciding
        slot of no CONN word and no PERPOD answer"""
        hit = np.zeros(self.n_slots, bool)
        hit[np.unique(self.words & 0x3FFFFFFF)] = True
        hit[np.unique(self.exp[MODE_PERPOD][1])] = True
        out = []
        for tap in self.resolved_taps():
            for name in self.e._if_acls(tap):
                if name:
                    base, n, dflt = self.e.table_info(self.e.table_id(name))
                    out += [(name, s - base if s != dflt else -1) for s in list(range(base, base + n)) + [dflt] if not hit[s]]
        return out

    def check_preconditions(self):
        f = self.probe_facts()
        if self.name in ("chain", "wrap"):
            assert f["cap"] == CHAIN_CAP and f["hit"] >= CHAIN_LEN and f["miss"] >= CHAIN_LEN, (self.name, f)
            assert (f["wrap_hit"] and f["wrap_miss"]) == (self.name == "wrap"), (self.name, f)
        if self.name.startswith("growth-"):
            assert f["cap"] == GROWTH_CAP[int(self.name[7:])], (self.name, f)
        if self.n_local >= 2:
            acts = np.bincount((self.words >> 30).ravel(), minlength=4)
            assert acts.min() >= ACTION_FLOOR, (self.name, acts.tolist())
            assert not self.undecided(), (self.name, self.undecided()[:8])
        n, seen = self.sensitivity()
        assert n == seen, (self.name, n, seen)
        return n

    # ---- sensitivity -----------------------------------------------------------------------------
    def ends(self):
        """{address: TAP name | NOIF | REMOTE} as the World resolves them"""
        return {ip: (REMOTE if another else tap or NOIF) for ip, (tap, another) in winners(self.regs).items()}

    def world_with(self, ends):
        w = copy.copy(self.world)
        loc = sorted(ip for ip, x in ends.items() if x != REMOTE)
        w.local_ips = np.array(loc, np.uint32)
        w.local_if = np.array([w.ifx[ends[ip]] if ends[ip] != NOIF else -1 for ip in loc], np.int32)
        w.remote_ips = np.array(sorted(ip for ip, x in ends.items() if x == REMOTE), np.uint32)
        return w

    def mutations(self):
        """(what, mutated ends) of every single-end-point mutation"""
        base = self.ends()
        ips = sorted(base)
        for i, ip in enumerate(ips):
            m = dict(base)
            del m[ip]
            yield ("drop", ip), m
            for step in (1, -1):
                m = dict(base)
                x = m.pop(ip)
                m[(ip + step) & M32] = x
                yield ("move%+d" % step, ip), m
            other = next((ips[(i + j) % len(ips)] for j in range(1, len(ips)) if base[ips[(i + j) % len(ips)]] != base[ip]), None)
            if other is not None:
                m = dict(base)
                m[ip], m[other] = base[other], base[ip]
                yield ("swap", ip, other), m
            for kind in (NOIF, REMOTE):
                if base[ip] != kind:
                    m = dict(base)
                    m[ip] = kind
                    yield ("kind-" + kind, ip), m

    def sensitivity(self):
        """(mutations, those after which the oracle's CONN words over the probe set differ)"""
        s, d, sp, dp, pr = self.tup
        w0 = self.words.ravel()
        n = seen = 0
        base = self.ends()
        for what, ends in self.mutations():
            touched = np.array(sorted({ip for ip in set(base) | set(ends) if base.get(ip) != ends.get(ip)}), np.uint32)
            idx = np.nonzero(np.isin(s, touched) | np.isin(d, touched))[0]
            n += 1
            if not len(idx):
                continue
            act, slot = self.world_with(ends).conn(s[idx], d[idx], sp[idx], dp[idx], pr[idx])
            seen += bool((((act.astype(np.uint32) << 30) | slot.astype(np.uint32)) != w0[idx]).any())
        return n, seen


@functools.lru_cache(maxsize=None)
def layout(name):
    return Layout(name)


def bisect_scattered(lo=57, hi=300):
    """(most pods with a node classifier, fewest without) between a count that has one and one that has
    none; and that every count below / above the pair agrees is spot-checked by the host test"""
    has = lambda n: build_engine(_cycle(scattered(n)))[0].node_stats() is not None   # noqa: E731
    assert has(lo) and not has(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if has(mid) else (lo, mid)
    return lo, hi


# layout -> single-end-point mutations of its World, every one of which changes the oracle's CONN words
MUTATIONS = {
    "chain": 50, "wrap": 50, "extremes": 34, "adjacent": 40, "on-rule-edges": 40,
    "growth-0": 0, "growth-1": 5, "growth-8": 45, "growth-9": 50, "growth-24": 134, "growth-25": 140,
    "growth-56": 314, "growth-57": 320, "scattered-small": 628, "scattered-big": 633, "repeat": 56,
}
