"""Tables, tuples and oracle answers of the SINGLE-mode form x stage matrix (test helper).

Shared by tests/test_single_matrix_host.py (the kernels' per-tuple code on the host, no GPU) and
tests/test_gpu_single_matrix.py (the same launches on the device): one table per form the compiler
can choose, each in an engine of its own, about 130k tuples per table with the oracle's verdicts
(oracle/fast.py eval_acl) computed once; and one five-table engine whose counter slots exceed the
LDS histogram, for the windowed hit counters. Everything is built on first use and cached for
the process; nothing here touches the GPU.

Two departures from plain fz.rand_acl / fz.rand_tuples, both so that every case meets its
preconditions (both actions, 20 matched rules, default-deny hits) without filtering tuples:
  * the "weird" tables (cross, pair-weird, fd) leave out the rules that fail or match every packet
    (MAC-IP, ICMP, no IpRule / Ip, TCP + UDP, an unparsable src, no src and no L4 section) --
    weird_rules says why. Those evalACL branches are therefore NOT exercised by this matrix on the
    GPU; test_gpu_parity.py's random-ACL tests keep covering them.
  * half of a table's tuples are drawn inside its rules (matrix_tuples), the other half by
    fz.rand_tuples around the table's own prefixes.
"""
import functools
import random

import numpy as np

import acl_fuzz as fz
from oracle import fast
from vpp_amd import renderer as R

N_TUPLES = 130003  # no multiple of 256 (nor is N_TUPLES - 1, the offset=1 batch): a partial last wave and group

# launch knobs of a case (Tuning, launches only: nothing is recompiled)
LAUNCHES = {
    "default": {},
    "nostage": {"stage_max_words": 0},
    "hbm": {"stage_max_words": 0, "stage_root_max_words": 0},
}
ALL_STAGES = (4, 5, 1, 2, 0, 9, 10, 14, 8)


def _ip(s):
    a = [int(x) for x in s.split(".")]
    return a[0] << 24 | a[1] << 16 | a[2] << 8 | a[3]


def _net(cidr):
    """well-formed IPv4 "a.b.c.d/p" or "" -> (network, prefix length); anything else -> None"""
    if not cidr:
        return 0, 0
    try:
        a, p = cidr.split("/")
        p = int(p)
        if ":" in a or a.count(".") != 3 or not 0 <= p <= 32 or any(not 0 <= int(x) <= 255 for x in a.split(".")):
            return None
        return _ip(a) & ((0xFFFFFFFF << (32 - p)) & 0xFFFFFFFF), p
    except ValueError:
        return None


def anchors_of(rules, limit=400):
    """addresses inside the table's own src / dst prefixes (fz.rand_tuples draws half of its
    addresses within 4096 of one), evenly thinned to `limit`, plus fz.ANCHORS"""
    a = []
    for r in rules:
        for f in ("src", "dst"):
            n = _net(r.get(f) or "")
            if n and n[1]:
                a.append(n[0])
    a = sorted(set(a))
    return a[::max(1, len(a) // limit)][:limit] + fz.ANCHORS


def _l4(rnd, spread=(0, 3, 100)):
    kind = rnd.random()
    lo = rnd.randrange(1, 60000)
    if kind < 0.45:
        return {"tcp": {"src": [0, 65535], "dst": [lo, lo + rnd.choice(spread)]}}
    if kind < 0.9:
        return {"udp": {"src": [0, 65535], "dst": [lo, lo + rnd.choice(spread)]}}
    return {}


def nested_rules(seed, n, dst):
    """test_compiler_host's candidate-mode shape: nested /16 /24 /30 src prefixes, TCP / UDP port
    ranges or no L4 section, and (dst) a dst net on half of the rules"""
    rnd = random.Random(seed)
    rules = []
    for k in range(n):
        a, b = rnd.randrange(8), rnd.randrange(64)
        src = rnd.choice(["10.%d.0.0/16" % a, "10.%d.%d.0/24" % (a, b), "10.%d.%d.%d/30" % (a, b, 4 * rnd.randrange(64))])
        r = {"action": rnd.randrange(2), "src": src, "dst": ""}
        if dst:
            r["dst"] = rnd.choice(["", "", "192.168.%d.0/24" % rnd.randrange(4), "192.168.0.%d/32" % rnd.randrange(8)])
        r.update(_l4(rnd))
        rules.append(r)
    return rules


def lists_rules():
    """test_compiler_host's 40-rule global-table shape: src = pod /32, dst = peer nets, ports"""
    rnd = random.Random(5)
    rules = []
    for k in range(40):
        src = "10.1.0.%d/32" % (k % 8 + 1)
        dst = rnd.choice(["10.2.0.0/16", "10.2.%d.0/24" % k, "8.8.8.8/32", ""])
        rules.append({"action": rnd.choice([0, 1]), "src": src, "dst": dst,
                      "tcp": {"src": [0, 65535], "dst": [80, 80 + k % 3]}})
    rules.append({"action": 1, "src": "", "dst": ""})
    return rules


def long_dst_rules():
    """test_compiler_host's long-dst-list shape: egress to 300 pod /32s per src and port"""
    rnd = random.Random(11)
    pods = [0x0A010000 | k for k in range(1, 400)]
    rules = []
    for s in range(12):
        src = "10.1.0.%d/32" % (s + 1)
        rules.append({"action": 1, "src": src, "dst": "", "tcp": {"src": [0, 65535], "dst": [443, 443]}})
        for p in rnd.sample(pods, 300):
            port = rnd.choice([8000, 8001, 8002])
            rules.append({"action": 1, "src": src, "dst": "%d.%d.%d.%d/32" % (p >> 24, p >> 16 & 255, p >> 8 & 255, p & 255),
                          "tcp": {"src": [0, 65535], "dst": [port, port]}})
        rules.append({"action": 1, "src": src, "dst": "10.96.0.10/32", "udp": {"src": [0, 65535], "dst": [53, 53]}})
        rules.append({"action": 0, "src": src, "dst": ""})
    rules.append({"action": 1, "src": "", "dst": ""})
    return rules


def weird_rules(seed, n):
    """fz.rand_acl's weird ACL (every evalACL branch) less the rules that fail or match every
    packet whatever its addresses and ports (a structural error, an unparsable src, no src and no
    L4 section): behind the first of them -- one in ten -- no later rule is ever matched, and a
    60-rule table would not have 20 matched rules"""
    def wide(r):
        bad = r.get("macip") or r.get("icmp") or not r.get("ip_rule", True) or not r.get("ip", True) or (
            r.get("tcp") and r.get("udp"))
        src = _net(r.get("src") or "")
        return bool(bad or src is None or (src == (0, 0) and not (r.get("tcp") or r.get("udp"))))
    return [r for r in fz.rand_acl(random.Random(seed), n, fz.ANCHORS, weird=True, tail=None) if not wide(r)]


def cross_rules():
    """a weird ACL (50 rules) that compiles to a plain cross product and still tests dst: the dst
    net stays on the rules whose port range is inverted -- no TCP / UDP packet matches them (not
    in the cross product, no dst lists), ANY-protocol packets do when their dst is inside (the
    linear path) -- so the table is not dst-free: stages 1 / 2 / 0 with the dst stream read"""
    rules = weird_rules(92, 66)
    for r in rules:
        d = ((r.get("tcp") or r.get("udp") or {}).get("dst"))
        if not (d and (d[0] & 0xFFFF) > (d[1] & 0xFFFF)):
            r["dst"] = ""
    return rules


def fd_rules():
    """about 300 dst-free rules (test_compiler_host test_fd_tables_dst_free)"""
    rules = weird_rules(703, 420)
    for r in rules:
        r["dst"] = ""
    return rules


def oversize_rules(k=8200):
    """No indexed form fits: k rules of any src with a port range are candidates of every src
    class, and k rules of /32s make k classes -- k * k candidates exceed the table compiler's
    2^26 (fastpath.cpp build_fast_table), at any `pair`: the table is flagged linear. (The pair = 2
    fallback of a table PAIR does not fit is CAND, not linear.)"""
    rnd = random.Random(1)
    rules = []
    for i in range(k):
        lo = rnd.randrange(1, 60000)
        rules.append({"action": i % 2, "src": "", "dst": "",
                      ("tcp" if i % 2 else "udp"): {"src": [0, 65535], "dst": [lo, lo + 2]}})
    for i in range(k):
        lo = rnd.randrange(1, 60000)
        rules.append({"action": i % 2, "src": "10.%d.%d.%d/32" % (i >> 14, i >> 6 & 255, (i & 63) * 4),
                      "dst": "10.9.0.0/16" if i % 3 == 0 else "", "tcp": {"src": [0, 65535], "dst": [lo, lo + 50]}})
    return rules


class Spec:
    """one table of the matrix: its rules, the compiler knobs it is built under, the structure
    table_stats must report, the stage code pg_debug_launch_plan must report per LAUNCHES entry,
    and the seed of its tuples"""

    def __init__(self, rules, knobs, structure, stages, seed, tiny=False, one_verdict=False):
        self.rules, self.knobs, self.structure, self.seed = rules, knobs, structure, seed
        self.stages = dict(zip(("default", "nostage", "hbm"), stages))
        self.tiny = tiny                # fewer than 20 rules: every rule must be matched
        self.one_verdict = one_verdict  # an empty table / one catch-all rule: one action only


CAND = {"cross_max_rules": 0, "pair": 0}  # no cross product, no PAIR: the candidate forms
CATCH_ALL = [{"action": 2, "src": "", "dst": ""}]

# name -> Spec. Rule counts of the forced forms: the smallest at which table_stats reports the
# structure and residence wanted (found on the CPU, asserted by test_single_matrix_host):
#   nested_rules(23, n, dst=True) under CAND: "cand" at every n; its blob fits LDS (16368 words)
#     up to n = 155 and is HBM-resident (level-compressed, 25236 words) from n = 156
#   nested_rules(23, n, dst=False) under CAND: HBM-resident from n = 212 and so "candi" (55184
#     words without a window), or with candi = 0 "cand" (30868 words); at n = 211 still "cand" in
#     LDS (16372 words)
#   LDS-sized CANDI: blobs of lc_lds (4096) words or more are rebuilt level-compressed, which is
#     where a dst-free candidate table takes the CANDI form, and the rebuild is kept while it fits
#     LDS: with candi_window_bits 0 or 8 that holds from n = 16 (13868 / 14380 words; n = 15:
#     3940 words, below lc_lds, "cand") up to n = 26
SPECS = {
    "cross": lambda: Spec(cross_rules(), {}, "cross", (1, 2, 0), 1),
    "cross+lists": lambda: Spec(lists_rules(), {}, "cross+lists", (1, 2, 0), 2),
    "pair-long": lambda: Spec(long_dst_rules(), {}, "pair", (2, 2, 0), 3),
    "pair-weird": lambda: Spec(weird_rules(92, 66), {"pair": 2}, "pair", (1, 2, 0), 4),
    "cand-lds": lambda: Spec(nested_rules(23, 155, True), CAND, "cand", (1, 2, 0), 5),
    "cand": lambda: Spec(nested_rules(23, 156, True), CAND, "cand", (2, 2, 0), 6),
    "cand-nodst-lds": lambda: Spec(nested_rules(23, 211, False), CAND, "cand", (9, 10, 8), 7),
    "cand-nodst": lambda: Spec(nested_rules(23, 212, False), dict(CAND, candi=0), "cand", (10, 10, 8), 8),
    "candi-w11": lambda: Spec(nested_rules(23, 212, False), dict(CAND, candi_window_bits=11), "candi", (14, 14, 8), 9),
    "candi-w0": lambda: Spec(nested_rules(23, 212, False), dict(CAND, candi_window_bits=0), "candi", (14, 14, 8), 10),
    "candi-lds": lambda: Spec(nested_rules(23, 16, False), dict(CAND, candi_window_bits=0), "candi", (9, 14, 8), 15, tiny=True),
    "candi-lds-w8": lambda: Spec(nested_rules(23, 16, False), dict(CAND, candi_window_bits=8), "candi", (9, 14, 8), 16,
                                 tiny=True),
    "fd": lambda: Spec(fd_rules(), {}, "fd", (4, 5, 8), 11),
    "linear": lambda: Spec(oversize_rules(), {"pair": 2}, "linear", (0, 0, 0), 12),
    # (no rule tests dst and the cross product is trivial: both compile to the FD form)
    "empty": lambda: Spec([], {}, "fd", (4, 5, 8), 13, tiny=True, one_verdict=True),
    "catch-all": lambda: Spec(CATCH_ALL, {}, "fd", (4, 5, 8), 14, tiny=True, one_verdict=True),
}
# stage code -> why no launch of these tables and knobs takes it: none, every code is launched
UNREACHABLE = {}

def engine_with(rules_by_name, knobs):
    e = R.Engine(0)
    for k, v in knobs.items():
        e.set_tuning(k, v)
    e.ApplyTxn(True, [("config/vpp/acls/v2/acl/" + n, {"name": n, "rules": r, "ingress": [], "egress": ["if-" + n]})
                      for n, r in sorted(rules_by_name.items())])
    e.table_stats(0)  # compile now, under the knobs as set
    return e


def oracle(e, tid, rules, tup):
    """evalACL over the tuples -> (action u32[n], counter slot u32[n]) in the engine's slot layout"""
    src, dst, sport, dport, proto = tup
    a, i = fast.eval_acl(fast.OraACL(rules), src, dst, dport, proto)
    base, _, dflt = e.table_info(tid)
    return a.astype(np.uint32), np.where(i >= 0, base + i, dflt).astype(np.uint32)


class Table:
    def __init__(self, name):
        self.name, self.spec = name, SPECS[name]()
        self.rules = self.spec.rules
        self.e = engine_with({"t": self.rules}, self.spec.knobs)
        self.tid = self.e.table_id("t")
        self.tup = matrix_tuples(self.rules, self.spec.seed)
        self.act, self.slot = oracle(self.e, self.tid, self.rules, self.tup)
        self.n_slots = self.e.num_counter_slots()

    def expected(self, offset):
        """oracle actions, slots and slot histogram of the batch tuples[offset:]"""
        return self.act[offset:], self.slot[offset:], np.bincount(self.slot[offset:], minlength=self.n_slots)

    def check_preconditions(self, offset):
        """what a case presupposes of its tuples, on the oracle's output alone"""
        act, slot, hist = self.expected(offset)
        base, n, dflt = self.e.table_info(self.tid)
        if self.spec.one_verdict:
            assert len(np.unique(act)) == 1
        else:
            assert (act == 0).any() and (act != 0).any(), "the oracle must return DENY and another action"
        matched = int((hist[base:base + n] > 0).sum())
        assert matched >= (n if self.spec.tiny else 20), matched
        catch_all = any(not (r.get("src") or r.get("dst") or r.get("tcp") or r.get("udp")) for r in self.rules)
        assert catch_all or hist[dflt] > 0, "no default-deny hit"
        assert (self.tup[4][offset:] > 2).sum() > 1000  # ANY-protocol packets: the linear path in every form


@functools.lru_cache(maxsize=None)
def table(name):
    return Table(name)


# ---- the windowed hit counters: a table set of more slots than the LDS histogram --------------
WINDOWS = (1, 64, 4096, 16382)
N_BIG = 9000


def big_rules(seed, dst):
    """9k rules: a /24 each (every ninth its /16: later rules behind an earlier one), ports from
    a pool of 24 (the cross product stays small), on every other rule a dst net (dst) -- and a last
    rule that half of the uniform tuples reach (no catch-all: the others are default-deny hits)"""
    rnd = random.Random(seed)
    ports = [rnd.randrange(1, 60000) for _ in range(24)]
    rules = []
    for k in range(N_BIG):
        r = {"action": rnd.randrange(2), "src": "10.%d.%d.0/24" % (k >> 8, k & 255) if k % 9 else "10.%d.0.0/16" % (k >> 8),
             "dst": ""}
        if dst and k % 2:
            r["dst"] = rnd.choice(["192.168.%d.0/24" % rnd.randrange(4), "192.168.0.%d/32" % rnd.randrange(8)])
        lo = rnd.choice(ports)
        if k % 10 < 8:
            r["tcp" if k % 10 < 4 else "udp"] = {"src": [0, 65535], "dst": [lo, lo + rnd.choice([0, 3, 100])]}
        rules.append(r)
    return rules + [{"action": 1, "src": "128.0.0.0/1", "dst": ""}]


def tuples_inside(rules, n, seed):
    """90 %: a rule picked uniformly, its src prefix plus random host bits, a port of its range, a
    dst of its dst net (a field evalACL cannot parse: any value); 10 % (all of them for a table
    without rules) uniform"""
    g = np.random.default_rng(seed)
    src = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    dst = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    dport = g.integers(0, 65536, n).astype(np.uint16)
    sport = g.integers(0, 65536, n).astype(np.uint16)
    proto = g.choice(np.array([0, 1, 2], np.uint8), n, p=[0.45, 0.45, 0.10])
    if rules:
        def fields(r):
            sec = r.get("tcp") or r.get("udp")
            lo, hi = (sec or {}).get("dst") or (0, 65535)
            lo = min(lo, 65535)
            return (_net(r.get("src") or "") or (0, 0)) + (_net(r.get("dst") or "") or (0, 0)) + (
                0 if r.get("tcp") else 1 if r.get("udp") else -1, lo, max(lo, min(hi, 65535)))
        f = np.array([fields(r) for r in rules], np.int64)
        pick = g.integers(0, len(rules), n)
        inside = g.random(n) >= 0.1
        snet, sl, dnet, dl, pr, lo, hi = (f[pick, k] for k in range(7))
        host = lambda bits: (g.integers(0, 1 << 32, n, dtype=np.uint64) >> bits.astype(np.uint64)) * (bits < 32)
        src = np.where(inside, snet + host(sl), src).astype(np.uint32)
        dst = np.where(inside, dnet + host(dl), dst).astype(np.uint32)
        dport = np.where(inside, lo + g.integers(0, 1 << 16, n) % (hi - lo + 1), dport).astype(np.uint16)
        proto = np.where(inside & (pr >= 0), pr, proto).astype(np.uint8)
    return src, dst, sport, dport, proto


def matrix_tuples(rules, seed):
    """fz.rand_tuples around the table's own prefixes with 2 % ANY-protocol packets; every other
    tuple's addresses, port and TCP / UDP / OTHER protocol drawn inside the rules instead
    (rand_tuples alone lands within 4096 addresses of a prefix: a table of /32s is hardly matched)"""
    g = np.random.default_rng(seed)
    a = fz.rand_tuples(g, N_TUPLES, anchors_of(rules), any_pct=0.02)
    b = tuples_inside(rules, N_TUPLES, seed + 1000)
    m = g.random(N_TUPLES) < 0.5
    src, dst, dport = (np.where(m, b[k], a[k]) for k in (0, 1, 3))
    proto = np.where(m & (a[4] <= 2), b[4], a[4])
    return src, dst, a[2], dport, proto


class WindowSet:
    """five ACLs whose names sort into: a 9k-rule dst-testing table, the 40-rule cross+lists table,
    an empty table, a 9k-rule dst-free table, a one-rule catch-all -- 18044 rules, 18051 slots"""

    def __init__(self):
        self.rules = {"a-dst9k": big_rules(31, True), "b-lists40": lists_rules(), "c-empty": [],
                      "d-free9k": big_rules(32, False), "e-all": CATCH_ALL}
        self.big = ("a-dst9k", "d-free9k")
        self.e = engine_with(self.rules, {})
        self.n_slots = self.e.num_counter_slots()
        self.names = sorted(self.rules)
        self.tid = {n: self.e.table_id(n) for n in self.names}
        self.tup, self.act, self.slot, self.hist = {}, {}, {}, {}
        for k, n in enumerate(self.names):
            self.tup[n] = tuples_inside(self.rules[n], N_TUPLES, 50 + k)
            self.act[n], self.slot[n] = oracle(self.e, self.tid[n], self.rules[n], self.tup[n])
            self.hist[n] = np.bincount(self.slot[n], minlength=self.n_slots)

    def window(self, name, cells):
        """[wbase, wbase + wn) of a counted launch on the table with `cells` histogram cells
        (device.hip k_classify: the table's first rules, clipped to the slots)"""
        base = self.e.table_info(self.tid[name])[0]
        return min(base, self.n_slots - cells), cells

    def check_preconditions(self, name, cells):
        base, n, dflt = self.e.table_info(self.tid[name])
        h = self.hist[name]
        assert h.sum() == N_TUPLES and h[:base].sum() == 0 and h[base + n:dflt].sum() == 0 and h[dflt + 1:].sum() == 0
        if name not in self.big:
            return
        wbase, wn = self.window(name, cells)
        assert h[base + n - 1] > 0 and h[dflt] > 0, "no hit at the table's last rule / default slot"
        assert h[wbase:wbase + wn].sum() > 0, "no hit inside the window"
        # past the window: rule slots where the table is longer than it (else only what lies beyond
        # it -- for 16382 cells the default slot of the first table, nothing of the last ones')
        if wn < n:
            assert h[wbase + wn:base + n].sum() > 0, "no rule hit past the window"


@functools.lru_cache(maxsize=None)
def window_set():
    return WindowSet()
