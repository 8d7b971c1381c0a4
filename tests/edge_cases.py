"""Tuples placed on purpose at the bounds of every rule, edge tables, and what the oracle says of
them (test helper).

Shared by tests/test_edge_host.py (no GPU) and tests/test_gpu_edges.py (the same launches on the
device). The random batches of single_matrix / node_matrix / reach_cases land on a prefix's first or
last address, or on a port range's end, only by chance; probes() puts a tuple on each of them and
one step outside, with the rule's other fields matched. Nothing here touches the GPU; everything
is built on first use and cached for the process.

An *edge cell* of a well-formed rule: one constrained field holds one of its four edge values --
a src or dst net of length > 0: net - 1, net, last, last + 1 (mod 2^32); a TCP / UDP dst range:
lo - 1, lo, hi, hi + 1 (mod 2^16) under the rule's protocol -- and the rule's other fields are
matched (an address inside each net; the rule's protocol and a port of its range, or an ANY
protocol code, for a rule with an L4 section). cells_hit() counts the cells a batch hits.

A rule is *well-formed* (rule_fields) when evalACL can match it and its bounds can be read: no
MAC-IP / ICMP / missing IpRule or Ip / TCP + UDP rule, src and dst nets that single_matrix._net
parses, and a dst port range that is not inverted as evalACL compares it (lower & 0xFFFF <= upper &
0xFFFF). An L4 section evalACL fails on before it compares a port (src range missing or not
0..65535, no dst range) keeps its net edges -- inside them the packet fails, outside the rule is
skipped -- and has no port edges. These are single_matrix.weird_rules' exclusions but one: a rule
without src and L4 section stays when it has a dst net (it does not match every packet, and the
node sets' inbound ACLs consist of such rules); without one it has no edge anyway.

Preconditions, all from the oracle's output alone (MEASURED holds the figures, asserted exactly by
tests/test_edge_host.py): decisive pairs -- an (inside, outside) probe pair on one side of one field
whose oracle verdict words differ -- per field kind; edge-cell coverage of the edge batch (100 %)
beside the random batch's; and the share of single-rule mutations (port upper bound + 1, prefix one
bit shorter) whose effect the batch sees, again beside the random batch's. NodeEdges (PERPOD /
CONN over node_matrix's topologies) and ReachEdges (the reachability matrix and the port sweep) do
the same for the node kernels: NODE_MEASURED, NODE_TABLE_MEASURED, REACH_MEASURED.
"""
import functools

import numpy as np

import fd_pipeline_cases as fc
import single_matrix as sm
from oracle import fast

M32 = 0xFFFFFFFF
SRC, DST, PORT, ALT, EXTREME, PAD = range(6)   # kind of a probe: the field its edge value is in
KIND_NAMES = ("src", "dst", "port")
ANY_CODES = (3, 7, 255)
EXT_ADDR = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
EXT_PORT = (0, 1, 32767, 32768, 65534, 65535)
EXT_PROTO = (0, 1, 2, 3, 255)
MAX_TUPLES = 50000
REC = np.dtype([("acl", np.int32), ("rule", np.int32), ("kind", np.uint8), ("pos", np.uint8), ("inside", np.bool_)])


def rule_fields(r):
    """(src net, src length, dst net, dst length, protocol or -1, lo, hi, whether evalACL compares
    the port) of a well-formed rule, the port bounds as evalACL compares them; None for any other"""
    if r.get("macip") or r.get("icmp") or not r.get("ip_rule", True) or not r.get("ip", True) or (
            r.get("tcp") and r.get("udp")):
        return None
    s, d = sm._net(r.get("src") or ""), sm._net(r.get("dst") or "")
    if s is None or d is None:
        return None
    sec = r.get("tcp") or r.get("udp")
    pr, lo, hi, ranged = -1, 0, 65535, False
    if sec:
        pr = 0 if r.get("tcp") else 1
        # (a section whose src range is missing or not 0..65535, or without a dst range, fails every
        # packet of its protocol inside the nets before a port is compared: net edges, no port edges)
        ranged = sec.get("src") is not None and list(sec["src"]) == [0, 65535] and sec.get("dst") is not None
        if ranged:
            lo, hi = sec["dst"][0] & 0xFFFF, sec["dst"][1] & 0xFFFF
            if lo > hi:
                return None
    return s + d + (pr, lo, hi, ranged)


def edge_values(f, kind):
    """the four edge values of a field of rule_fields' f, and whether each lies inside it"""
    if kind == PORT:
        lo, hi = f[5], f[6]
        v = [(lo - 1) & 0xFFFF, lo, hi, (hi + 1) & 0xFFFF]
        return v, [lo <= x <= hi for x in v]
    net, ln = (f[0], f[1]) if kind == SRC else (f[2], f[3])
    last = net | (M32 >> ln)
    mask = (M32 << (32 - ln)) & M32
    v = [(net - 1) & M32, net, last, (last + 1) & M32]
    return v, [(x & mask) == net for x in v]


def constrained(f):
    """the field kinds of a well-formed rule that have edges"""
    return [k for k, on in ((SRC, f[1] > 0), (DST, f[3] > 0), (PORT, f[7])) if on]


def _spaced(items, n):
    if len(items) <= n:
        return items
    return [items[j] for j in np.unique(np.round(np.linspace(0, len(items) - 1, n)).astype(np.int64))]


def select(rules, cap):
    """indices of the rules that are probed: the well-formed ones with a constrained field, and of
    more than `cap` an evenly spaced selection with the first and the last"""
    fields = [rule_fields(r) for r in rules]
    ok = [i for i, f in enumerate(fields) if f is not None and constrained(f)]
    return _spaced(ok, cap)


def rule_probes(rules, cap, seed, fixed=None, repeat=1):
    """the edge probes of probes(), without what it appends: (src, dst, dport, proto, records);
    repeat: so many probes of every edge value, each with its own draw of the other fields"""
    rule, kind, pos, inside, value, proto = [], [], [], [], [], []
    turn = 0
    for i in select(rules, cap) * repeat:
        f = rule_fields(rules[i])
        own = f[4] if f[4] >= 0 else turn % 3
        for k in constrained(f):
            if fixed and k in fixed:
                continue
            v, ins = edge_values(f, k)
            protos = [own]
            if k == PORT:
                protos += [1 - own, 2, ANY_CODES[turn % 3]]
            for j, p in enumerate(protos):
                rule += [i] * 4
                kind += [k if j == 0 else ALT] * 4
                pos += [0, 1, 2, 3]
                inside += ins
                value += v
                proto += [p] * 4
        turn += 1
    n = len(rule)
    rec = np.zeros(n, REC)
    rec["acl"] = -1
    z = np.zeros(0, np.uint32)
    if not n:
        return z, z, np.zeros(0, np.uint16), np.zeros(0, np.uint8), rec
    rec["rule"], rec["kind"], rec["pos"], rec["inside"] = rule, kind, pos, inside
    g = np.random.default_rng(seed)
    f = np.array([rule_fields(r) or (0,) * 8 for r in rules], np.int64)[np.array(rule)]
    snet, sl, dnet, dl, _, lo, hi = (f[:, k] for k in range(7))
    host = lambda bits: (g.integers(0, 1 << 32, n, dtype=np.uint64) >> bits.astype(np.uint64)) * (bits < 32)  # noqa: E731
    src, dst = snet + host(sl), dnet + host(dl)
    dport = lo + g.integers(0, 1 << 16, n) % (hi - lo + 1)
    k, v = rec["kind"], np.array(value, np.int64)
    src, dst, dport = np.where(k == SRC, v, src), np.where(k == DST, v, dst), np.where((k == PORT) | (k == ALT), v, dport)
    for side, ip in (fixed or {}).items():
        (src if side == SRC else dst)[:] = ip
    return src.astype(np.uint32), dst.astype(np.uint32), dport.astype(np.uint16), np.array(proto, np.uint8), rec


def finish(parts, seed, sport=None):
    """the batch of probes(): the parts (rule_probes) one after the other, the extremes, the padding,
    and src ports (random where `sport` gives none)"""
    ext = np.array([(a, b, p, c) for a in EXT_ADDR for b in EXT_ADDR for p in EXT_PORT for c in EXT_PROTO], np.int64)
    erec = np.zeros(len(ext), REC)
    erec["rule"], erec["acl"], erec["kind"] = -1, -1, EXTREME
    parts = list(parts) + [(ext[:, 0].astype(np.uint32), ext[:, 1].astype(np.uint32), ext[:, 2].astype(np.uint16),
                            ext[:, 3].astype(np.uint8), erec)]
    src, dst, dport, proto, rec = (np.concatenate([p[k] for p in parts]) for k in range(5))
    rnd = np.random.default_rng(seed + 1).integers(0, 65536, len(src)).astype(np.uint16)
    if sport is not None:
        rnd[:len(sport)] = sport
    sport = rnd
    pad = 0
    while (len(src) + pad) % 256 == 0 or (len(src) + pad - 1) % 256 == 0:
        pad += 1
    if pad:
        rep = lambda a: np.concatenate([a, np.repeat(a[:1], pad)])  # noqa: E731
        src, dst, sport, dport, proto, rec = rep(src), rep(dst), rep(sport), rep(dport), rep(proto), rep(rec)
        rec["rule"][-pad:], rec["acl"][-pad:], rec["kind"][-pad:] = -1, -1, PAD
    assert len(src) < MAX_TUPLES and len(src) % 256 and (len(src) - 1) % 256
    return (src, dst, sport, dport, proto), rec


def probes(rules, cap=2000, seed=0):
    """-> ((src, dst, sport, dport, proto), records): for every probed rule (select) and constrained
    field the four edge values, the other fields drawn inside the rule (as
    single_matrix.tuples_inside does) under the rule's own protocol (no L4 section: 0, 1, 2 in
    turn); the port edges again under the other L4 protocol, OTHER and an ANY code (3, 7, 255 in
    turn), kind ALT; then the cross product of the global extremes (EXT_*), kind EXTREME; then as
    many copies of the first tuple (kind PAD) as it takes for neither the length nor length - 1 to
    be a multiple of 256. A quad of edge probes is four consecutive tuples, pos 0..3 = low
    outside, low inside, high inside, high outside. records: REC per tuple (rule -1 where none)."""
    return finish([rule_probes(rules, cap, seed)], seed)


def pairs(rec):
    """(inside index, outside index, kind) of every (inside, outside) probe pair: one per side of a
    quad of kind SRC / DST / PORT whose two values lie on different sides of the bound (a /1's low
    neighbour does, the neighbours of a range 0..65535 do not)"""
    q = np.nonzero((rec["pos"] == 0) & (rec["kind"] <= PORT))[0]
    ins = rec["inside"]
    lo = q[ins[q + 1] & ~ins[q]]
    hi = q[ins[q + 2] & ~ins[q + 3]]
    return (np.concatenate([lo + 1, hi + 2]), np.concatenate([lo, hi + 3]),
            np.concatenate([rec["kind"][lo], rec["kind"][hi]]))


def decisive(rec, words):
    """{field kind name: (inside, outside) pairs whose verdict words differ}"""
    i, o, k = pairs(rec)
    d = words[i] != words[o]
    return {KIND_NAMES[c]: int((d & (k == c)).sum()) for c in (SRC, DST, PORT)}


def cells_hit(rules, idx, tup):
    """(edge cells of the rules idx that some tuple of tup hits, edge cells of those rules)"""
    src, dst, _, dport, proto = (np.asarray(a).astype(np.int64) for a in tup)
    order = [np.argsort(a, kind="stable") for a in (src, dst, dport)]
    srt = [a[o] for a, o in zip((src, dst, dport), order)]
    hit = total = 0
    for i in idx:
        f = rule_fields(rules[i])
        snet, sl, dnet, dl, pr, lo, hi, _ = f
        for k in constrained(f):
            for v in edge_values(f, k)[0]:
                total += 1
                a, b = np.searchsorted(srt[k], [v, v + 1])
                c = order[k][a:b]
                if k != SRC and sl:
                    c = c[(src[c] >> (32 - sl)) == (snet >> (32 - sl))]
                if k != DST and dl:
                    c = c[(dst[c] >> (32 - dl)) == (dnet >> (32 - dl))]
                if k == PORT:
                    c = c[proto[c] == pr]
                elif pr >= 0:
                    c = c[(proto[c] > 2) | ((proto[c] == pr) & (dport[c] >= lo) & (dport[c] <= hi))]
                hit += len(c) > 0
    return hit, total


# ---- sensitivity: would the batch notice a rule that is wrong at an edge ------------------------
def mutations(r):
    """the rule with its port upper bound + 1, and with its src (else dst) prefix one bit shorter"""
    f = rule_fields(r)
    out = []
    if f[7] and f[6] < 65535:
        sec = "tcp" if r.get("tcp") else "udp"
        out.append(dict(r, **{sec: dict(r[sec], dst=[f[5], f[6] + 1])}))
    for name, net, ln in (("src", f[0], f[1]), ("dst", f[2], f[3])):
        if ln > 0:
            net &= (M32 << (33 - ln)) & M32
            out.append(dict(r, **{name: "%d.%d.%d.%d/%d" % (net >> 24, net >> 16 & 255, net >> 8 & 255, net & 255, ln - 1)}))
            break
    return out


def sees(mutant, k, tup, idx):
    """whether the oracle's answers on tup change when rule k is replaced by `mutant`, a rule that
    matches whatever rule k does: evalACL takes the first match, so they change exactly on the
    tuples that went past rule k (idx, the oracle's deciding rule: later or none) and that the
    oracle matches against the mutant alone. (test_edge_host holds this against a full
    evaluation of the mutated table.)"""
    past = np.nonzero((idx > k) | (idx < 0))[0]
    if not len(past):
        return False
    src, dst, _, dport, proto = (a[past] for a in tup)
    return bool((fast.eval_acl(fast.OraACL([mutant]), src, dst, dport, proto)[1] == 0).any())


def sees_full(rules, mutant, k, tup, act, idx):
    """sees() by evaluating the whole mutated table"""
    a, i = fast.eval_acl(fast.OraACL(rules[:k] + [mutant] + rules[k + 1:]), tup[0], tup[1], tup[3], tup[4])
    return bool((a != act).any() or (i != idx).any())


def sensitivity(rules, rec, idx, batches, limit=24):
    """(mutations, seen by each of `batches` = [(tuples, oracle rule index)]) over up to `limit`
    evenly spaced rules among those that decide a probe of the edge batch"""
    probed = rec["kind"] <= PORT
    dec = np.unique(idx[probed & (idx == rec["rule"])])
    dec = _spaced(dec.tolist(), limit)
    n, seen = 0, [0] * len(batches)
    for k in dec:
        for m in mutations(rules[k]):
            n += 1
            for b, (tup, bidx) in enumerate(batches):
                seen[b] += sees(m, int(k), tup, bidx)
    return n, seen


# ---- edge tables --------------------------------------------------------------------------------
LADDER_A, LADDER_B = 0x0A4D8105, 0xC0A825C9   # 10.77.129.5, 192.168.37.201: mixed bits at every level


def _cidr(ip, ln):
    ip &= (M32 << (32 - ln)) & M32
    return "%d.%d.%d.%d/%d" % (ip >> 24, ip >> 16 & 255, ip >> 8 & 255, ip & 255, ln)


def ladder_rules(field):
    """32 rules: one address at /32, /31, ..., /1, most specific first, actions alternating, no L4
    section -- every prefix length decides its own sibling range, so every trie level and stride
    boundary has a probe pair on each side. "both": the src ladder with a dst net of a second
    ladder (the lengths in another order), and a TCP or UDP single port on every other rule"""
    rules = []
    for i in range(32):
        r = {"action": i % 2, "src": "", "dst": ""}
        if field in ("src", "both"):
            r["src"] = _cidr(LADDER_A, 32 - i)
        if field == "dst":
            r["dst"] = _cidr(LADDER_A, 32 - i)
        if field == "both":
            r["dst"] = _cidr(LADDER_B, 1 + (11 * i + 7) % 32)
            if i % 2:
                r["tcp" if i % 4 == 1 else "udp"] = {"src": [0, 65535], "dst": [1000 + 7 * i, 1000 + 7 * i]}
        rules.append(r)
    return rules


EXTREME_NETS = ("0.0.0.0/32", "255.255.255.255/32", "255.255.255.0/24", "0.0.0.0/8", "0.0.0.0/1", "128.0.0.0/1")
# ports_cases' "full" fixture: 0..0, 65535..65535, adjacent, overlapping, single ports, the inverted
# 500..400, an upper bound of 65536 + 80 (10..80), a lower bound of 65536 + 5000 (5000..6000), 0..65535
EXTREME_RANGES = ((0, 0), (65535, 65535), (100, 199), (200, 299), (1000, 2000), (1500, 2500), (80, 80), (53, 53),
                  (443, 443), (123, 123), (500, 400), (10, 65536 + 80), (65536 + 5000, 6000), (32768, 65535), (0, 65535))


def extreme_rules():
    """every EXTREME_RANGES range on both protocols -- behind a src net of EXTREME_NETS in turn, and
    on every other rule a dst net -- then the nets alone on src and on dst, most specific first; no
    catch-all"""
    rules = []
    for i, (lo, hi) in enumerate(EXTREME_RANGES):
        for j, sec in enumerate(("tcp", "udp")):
            k = 2 * i + j
            rules.append({"action": k % 3 % 2, "src": EXTREME_NETS[(k + k // 6) % 6] if k % 4 != 3 else "",
                          "dst": EXTREME_NETS[(k // 2 + 4) % 6] if k % 2 else "", sec: {"src": [0, 65535], "dst": [lo, hi]}})
    for k, net in enumerate(EXTREME_NETS):
        rules.append({"action": k % 2, "src": net, "dst": EXTREME_NETS[(k + 3) % 6] if k < 4 else ""})
    for k, net in enumerate(EXTREME_NETS):
        rules.append({"action": 1 - k % 2, "src": "", "dst": net})
    return rules


EDGE_RULES = {"ladder-src": lambda: ladder_rules("src"), "ladder-dst": lambda: ladder_rules("dst"),
              "ladder-both": lambda: ladder_rules("both"), "extremes": extreme_rules}
# the knob sets of single_matrix.SPECS. Under them no edge table is CANDI: the only dst-free one,
# ladder-src, has a candidate blob of 1172 words, below lc_lds (4096), the size from which a blob is
# rebuilt level-compressed -- which is where a dst-free candidate table takes the CANDI form. A
# fifth knob set, for ladder-src alone, lowers lc_lds to 1024 (9040 words, kept in LDS).
KNOBS = {"": {}, "cand": sm.CAND, "candi0": dict(sm.CAND, candi_window_bits=0), "pair": {"pair": 2}}
KNOBS_LC = dict(sm.CAND, candi_window_bits=0, lc_lds=1024)
# "<table>+<knob set>" -> (structure table_stats reports, stage code per single_matrix.LAUNCHES
# entry), found on the CPU and asserted by tests/test_edge_host.py. (pair = 2 makes the dst-free
# ladder-src a PAIR table that launches at the dst-free codes.)
EDGE_FORMS = {
    "ladder-src": ("fd", (4, 5, 8)),                # 32 rules, 4724 words
    "ladder-src+cand": ("cand", (9, 10, 8)),        # 1172 words
    "ladder-src+candi0": ("cand", (9, 10, 8)),      # 1172 words: below lc_lds, not rebuilt
    "ladder-src+pair": ("pair", (9, 10, 8)),        # 1144 words
    "ladder-src+candi-lc": ("candi", (9, 14, 8)),   # 9040 words
    "ladder-dst": ("pair", (1, 2, 0)),              # 32 rules, 1144 words
    "ladder-dst+cand": ("cand", (1, 2, 0)),         # 160 words
    "ladder-dst+candi0": ("cand", (1, 2, 0)),
    "ladder-dst+pair": ("pair", (1, 2, 0)),
    "ladder-both": ("pair", (1, 2, 0)),             # 32 rules, 12620 words
    "ladder-both+cand": ("cand", (1, 2, 0)),        # 3156 words
    "ladder-both+candi0": ("cand", (1, 2, 0)),
    "ladder-both+pair": ("pair", (1, 2, 0)),
    "extremes": ("cross+lists", (1, 2, 0)),         # 42 rules, 6904 words
    "extremes+cand": ("cand", (1, 2, 0)),           # 2192 words
    "extremes+candi0": ("cand", (1, 2, 0)),
    "extremes+pair": ("pair", (1, 2, 0)),           # 8036 words
}


def _knobs(name):
    t, _, k = name.partition("+")
    return t, KNOBS_LC if k == "candi-lc" else KNOBS[k]


EDGE_SPECS = {name: (lambda name=name: sm.Spec(EDGE_RULES[_knobs(name)[0]](), _knobs(name)[1], *EDGE_FORMS[name], seed=0))
              for name in EDGE_FORMS}
# form the edge tables must reach -> why none does under any knob set: none, every form is reached
REQUIRED_FORMS = ("fd", "cross", "pair", "cand", "candi")   # ("cross": cross or cross+lists)
UNREACHABLE = {}

WINDOW_TABLES = ("a-dst9k", "b-lists40", "c-empty", "d-free9k", "e-all")
# stage code per single_matrix.LAUNCHES entry of the tables that have no Spec
OTHER_STAGES = {
    "split": ("fd", (4, 5, 8)),
    "w-a-dst9k": ("cross+lists", (2, 2, 0)),
    "w-b-lists40": ("cross+lists", (1, 2, 0)),
    "w-c-empty": ("fd", (4, 5, 8)),
    "w-d-free9k": ("fd", (5, 5, 8)),
    "w-e-all": ("fd", (4, 5, 8)),
}
SINGLE_TABLES = list(sm.SPECS) + ["split"] + ["w-" + n for n in WINDOW_TABLES] + list(EDGE_SPECS)
FD_TABLES = ("fd", "split", "ladder-src")   # the FD-in-LDS launch (STAGE 4) variants run over these
EXEMPT = ("empty", "catch-all", "w-c-empty", "w-e-all")   # no rule edges: the extremes only
SEED = 97


class EdgeTable:
    """a SINGLE table with its edge batch and the oracle's answers on it"""

    def __init__(self, name):
        self.name = name
        if name in sm.SPECS:
            t = sm.table(name)
            self.e, self.tid, self.rules, self.stages, self.structure = t.e, t.tid, t.rules, t.spec.stages, t.spec.structure
            self.random_tup = t.tup
        elif name == "split":
            t = fc.table("split")
            self.e, self.tid, self.rules, self.structure = t.e, t.tid, t.rules, "fd"
            self.random_tup = t.tup
        elif name.startswith("w-"):
            w = sm.window_set()
            self.e, self.tid, self.rules = w.e, w.tid[name[2:]], w.rules[name[2:]]
            self.random_tup = w.tup[name[2:]]
        else:
            spec = EDGE_SPECS[name]()
            self.rules, self.stages, self.structure = spec.rules, spec.stages, spec.structure
            self.e = sm.engine_with({"t": self.rules}, spec.knobs)
            self.tid = self.e.table_id("t")
            self.random_tup = sm.matrix_tuples(self.rules, SEED)
        if name in OTHER_STAGES:
            self.structure, stages = OTHER_STAGES[name]
            self.stages = dict(zip(sm.LAUNCHES, stages))
        self.n_slots = self.e.num_counter_slots()
        self.tup, self.rec = probes(self.rules, seed=SEED)
        self.act, self.slot, self.idx = self.oracle(self.tup)

    def oracle(self, tup):
        """evalACL over tup -> (action, slot in the engine's layout, rule index or -1)"""
        a, i = fast.eval_acl(fast.OraACL(self.rules), tup[0], tup[1], tup[3], tup[4])
        base, _, dflt = self.e.table_info(self.tid)
        return a.astype(np.uint32), np.where(i >= 0, base + i, dflt).astype(np.uint32), i

    def words(self):
        return (self.act << 30) | self.slot

    def expected(self, offset):
        return self.act[offset:], self.slot[offset:], np.bincount(self.slot[offset:], minlength=self.n_slots)

    def kinds(self):
        """the field kinds the probed rules constrain"""
        return sorted({KIND_NAMES[k] for i in select(self.rules, 2000) for k in constrained(rule_fields(self.rules[i]))})

    @functools.lru_cache(maxsize=None)
    def measured(self):
        """what MEASURED holds of this table: (decisive pairs per field kind, (cells hit, cells) of
        the random batch, of the edge batch, (mutations, seen by the edge batch, by the random
        batch))"""
        idx = select(self.rules, 2000)
        ridx = self.oracle(self.random_tup)[2]
        n, seen = sensitivity(self.rules, self.rec, self.idx, [(self.tup, self.idx), (self.random_tup, ridx)])
        return (decisive(self.rec, self.words()), cells_hit(self.rules, idx, self.random_tup),
                cells_hit(self.rules, idx, self.tup), (n, seen[0], seen[1]))

    def floor(self):
        return 0 if self.name in EXEMPT else 10 if len(self.rules) < 20 else 20


@functools.lru_cache(maxsize=None)
def table(name):
    return EdgeTable(name)


class FdCase:
    """what test_gpu_fd_pipeline.run_case takes of a case: an FD table on its edge batch"""

    def __init__(self, name):
        t = table(name)
        self.t, self.e, self.tid, self.n_slots = t, t.e, t.tid, t.n_slots
        self.tup, self.act, self.slot = t.tup, t.act, t.slot

    def words(self):
        return self.t.words()


# table -> (decisive pairs {kind: n}, random batch (cells hit, cells), edge batch (cells hit, cells),
# (mutations, seen by the edge batch, seen by the random batch)); the oracle alone, on the CPU
MEASURED = {
    "cross": ({'src': 61, 'dst': 0, 'port': 40}, (155, 264), (264, 264), (32, 31, 17)),
    "cross+lists": ({'src': 80, 'dst': 55, 'port': 72}, (292, 464), (464, 464), (48, 42, 20)),
    "pair-long": ({'src': 4000, 'dst': 3972, 'port': 3986}, (14915, 23916), (23916, 23916), (47, 37, 7)),
    "pair-weird": ({'src': 54, 'dst': 47, 'port': 39}, (163, 376), (376, 376), (34, 34, 4)),
    "cand-lds": ({'src': 310, 'dst': 158, 'port': 282}, (617, 1504), (1504, 1504), (47, 47, 5)),
    "cand": ({'src': 312, 'dst': 160, 'port': 284}, (626, 1516), (1516, 1516), (48, 48, 2)),
    "cand-nodst-lds": ({'src': 311, 'dst': 0, 'port': 234}, (656, 1616), (1616, 1616), (47, 45, 8)),
    "cand-nodst": ({'src': 311, 'dst': 0, 'port': 234}, (655, 1624), (1624, 1624), (47, 45, 6)),
    "candi-w11": ({'src': 311, 'dst': 0, 'port': 234}, (662, 1624), (1624, 1624), (47, 45, 7)),
    "candi-w0": ({'src': 311, 'dst': 0, 'port': 234}, (658, 1624), (1624, 1624), (47, 45, 7)),
    "candi-lds": ({'src': 32, 'dst': 0, 'port': 28}, (51, 120), (120, 120), (30, 30, 9)),
    "candi-lds-w8": ({'src': 32, 'dst': 0, 'port': 28}, (53, 120), (120, 120), (30, 30, 10)),
    "fd": ({'src': 213, 'dst': 0, 'port': 97}, (946, 1604), (1604, 1604), (29, 29, 14)),
    "linear": ({'src': 1980, 'dst': 657, 'port': 3642}, (4653, 13332), (13332, 13332), (36, 32, 4)),
    "empty": ({'src': 0, 'dst': 0, 'port': 0}, (0, 0), (0, 0), (0, 0, 0)),
    "catch-all": ({'src': 0, 'dst': 0, 'port': 0}, (0, 0), (0, 0), (0, 0, 0)),
    "split": ({'src': 4000, 'dst': 0, 'port': 4000}, (5453, 16000), (16000, 16000), (48, 41, 1)),
    "w-a-dst9k": ({'src': 1065, 'dst': 611, 'port': 622}, (3622, 18396), (18396, 18396), (43, 41, 8)),
    "w-b-lists40": ({'src': 80, 'dst': 55, 'port': 72}, (291, 464), (464, 464), (48, 42, 19)),
    "w-c-empty": ({'src': 0, 'dst': 0, 'port': 0}, (0, 0), (0, 0), (0, 0, 0)),
    "w-d-free9k": ({'src': 959, 'dst': 0, 'port': 565}, (2565, 14396), (14396, 14396), (40, 36, 6)),
    "w-e-all": ({'src': 0, 'dst': 0, 'port': 0}, (0, 0), (0, 0), (0, 0, 0)),
    "ladder-src": ({'src': 64, 'dst': 0, 'port': 0}, (62, 128), (128, 128), (24, 24, 24)),
    "ladder-src+cand": ({'src': 64, 'dst': 0, 'port': 0}, (62, 128), (128, 128), (24, 24, 24)),
    "ladder-src+candi0": ({'src': 64, 'dst': 0, 'port': 0}, (62, 128), (128, 128), (24, 24, 24)),
    "ladder-src+pair": ({'src': 64, 'dst': 0, 'port': 0}, (62, 128), (128, 128), (24, 24, 24)),
    "ladder-src+candi-lc": ({'src': 64, 'dst': 0, 'port': 0}, (62, 128), (128, 128), (24, 24, 24)),
    "ladder-dst": ({'src': 0, 'dst': 64, 'port': 0}, (59, 128), (128, 128), (24, 24, 24)),
    "ladder-dst+cand": ({'src': 0, 'dst': 64, 'port': 0}, (59, 128), (128, 128), (24, 24, 24)),
    "ladder-dst+candi0": ({'src': 0, 'dst': 64, 'port': 0}, (59, 128), (128, 128), (24, 24, 24)),
    "ladder-dst+pair": ({'src': 0, 'dst': 64, 'port': 0}, (59, 128), (128, 128), (24, 24, 24)),
    "ladder-both": ({'src': 64, 'dst': 59, 'port': 27}, (116, 320), (320, 320), (36, 30, 22)),
    "ladder-both+cand": ({'src': 64, 'dst': 59, 'port': 27}, (116, 320), (320, 320), (36, 30, 22)),
    "ladder-both+candi0": ({'src': 64, 'dst': 59, 'port': 27}, (116, 320), (320, 320), (36, 30, 22)),
    "ladder-both+pair": ({'src': 64, 'dst': 59, 'port': 27}, (116, 320), (320, 320), (36, 30, 22)),
    "extremes": ({'src': 53, 'dst': 40, 'port': 50}, (173, 316), (316, 316), (41, 40, 17)),
    "extremes+cand": ({'src': 53, 'dst': 40, 'port': 50}, (173, 316), (316, 316), (41, 40, 17)),
    "extremes+candi0": ({'src': 53, 'dst': 40, 'port': 50}, (173, 316), (316, 316), (41, 40, 17)),
    "extremes+pair": ({'src': 53, 'dst': 40, 'port': 50}, (173, 316), (316, 316), (41, 40, 17)),
}


# ---- PERPOD / CONN: the node sets of node_matrix ----------------------------------------------------
NODE_RULE_CAP = 1100   # probed rules per topology: at most 20 probes a rule, each also reversed


class NodeEdges:
    """the edge batch of a node_matrix topology, shared by its sets, and the oracle's answers.

    A probe for a rule of ACL A keeps the end point that selects A: the pod on A's interface as dst
    for an egress ACL, as src for an ingress ACL (so that field's own edges are not probed: it
    holds one address); the node interface's ACLs are selected by any address that is no local
    pod, which the probes' own addresses are, so nothing is fixed. Topologies of more than
    NODE_RULE_CAP rules take an evenly spaced selection per ACL. Every probe is followed, in a
    second half of the batch, by its reverse (src <-> dst, sport <-> dport): CONN's SYN-ACK
    evaluations read the tuple reversed, so the edge addresses stand on both sides and the port
    edges in both port fields. Then the extremes and the padding, as in probes()."""

    def __init__(self, topology):
        import node_matrix as nm
        self.name = topology
        self.t = t = nm.topo(topology)
        e = t.e
        tap_ip = {ifn: ip for ip, ifn in t.local[0].items()}
        acls = [(n, e.GetACLByName(n)) for n in e.ACLNames()]
        acls = [(n, a) for n, a in acls if a["rules"]]
        total = sum(len(a["rules"]) for _, a in acls)
        cap = NODE_RULE_CAP if total <= NODE_RULE_CAP else max(2, NODE_RULE_CAP // len(acls))
        self.repeat = max(1, min(4, NODE_RULE_CAP // total))
        parts, self.ingress = [], []
        for k, (n, a) in enumerate(acls):
            side, tap = nm._acl_side(a)
            if side is not None and tap not in tap_ip:
                continue
            fixed = {} if side is None else {(SRC, DST)[side]: tap_ip[tap]}
            p = rule_probes(a["rules"], cap, SEED + k, fixed, self.repeat)
            p[4]["acl"] = e.table_id(n)
            if side == 0:
                self.ingress.append(e.table_id(n))
            parts.append(p)
        src, dst, dport, proto, rec = (np.concatenate([p[k] for p in parts]) for k in range(5))
        sport = np.random.default_rng(SEED).integers(0, 65536, len(src)).astype(np.uint16)
        self.n_probes = len(src)
        fwd = (src, dst, dport, proto, rec)
        rev = (dst, src, sport, proto, rec)
        self.tup, self.rec = finish([fwd, rev], SEED, sport=np.concatenate([sport, dport]))
        self.n_slots = t.n_slots
        src, dst, sport, dport, proto = self.tup
        act, slot = t.world.perpod(src, dst, dport, proto, threads=4)
        self.exp = {nm.MODE_PERPOD: (act.astype(np.uint32), slot.astype(np.uint32),
                                     np.bincount(slot, minlength=self.n_slots).astype(np.uint64))}
        act, slot, hist = t.world.conn(src, dst, sport, dport, proto, threads=4, hist=True)
        self.exp[nm.MODE_CONN] = (act.astype(np.uint32), slot.astype(np.uint32), hist.astype(np.uint64))
        self._prefix = {}

    def expected(self, mode, offset=0):
        """oracle (action, deciding slot, counter histogram) of tuples[offset:]"""
        import node_matrix as nm
        act, slot, hist = self.exp[mode]
        if offset == 0:
            return act, slot, hist
        if mode == nm.MODE_PERPOD:
            return act[offset:], slot[offset:], np.bincount(slot[offset:], minlength=self.n_slots).astype(np.uint64)
        if offset not in self._prefix:   # CONN counts every evaluation: the oracle's histogram of that batch
            src, dst, sport, dport, proto = (a[offset:] for a in self.tup)
            self._prefix[offset] = self.t.world.conn(src, dst, sport, dport, proto, threads=4, hist=True)[2].astype(np.uint64)
        return act[offset:], slot[offset:], self._prefix[offset]

    def words(self, mode):
        return (self.exp[mode][0] << 30) | self.exp[mode][1]

    def pairs(self, mode):
        """pairs() of the probes the mode evaluates at the probed rule: CONN all of them; PERPOD,
        which evaluates the dst interface's outbound ACL alone, the probes as first written (not
        the reversed half) of the egress and node ACLs"""
        import node_matrix as nm
        i, o, k = pairs(self.rec)
        if mode == nm.MODE_PERPOD:
            m = (i < self.n_probes) & ~np.isin(self.rec["acl"][i], self.ingress)
            i, o, k = i[m], o[m], k[m]
        return i, o, k

    def floors(self, mode):
        """{field kind: floor of its decisive pairs}: 20, or 10 where fewer than 20 of the probed
        rules constrain that kind (part of one small ACL), for the kinds that have a pair"""
        i, _, k = self.pairs(mode)
        out = {}
        for c in (SRC, DST, PORT):
            r = self.rec[i[k == c]]
            if len(r):
                out[KIND_NAMES[c]] = 20 if len(np.unique(r[["acl", "rule"]])) >= 20 else 10
        return out

    def decisive(self, mode, tables=None):
        """decisive pairs per field kind; tables: only the pairs whose inside probe is decided in
        one of these tables (the total over the kinds)"""
        w = self.words(mode)
        i, o, k = self.pairs(mode)
        d = w[i] != w[o]
        if tables is None:
            return {KIND_NAMES[c]: int((d & (k == c)).sum()) for c in (SRC, DST, PORT)}
        tab = np.array([self.t.e.slot_info(s)[0] for s in range(self.n_slots)], np.int64)
        return int((d & np.isin(tab[self.exp[mode][1][i]], tables)).sum())

    def kinds(self):
        return sorted({KIND_NAMES[k] for k in np.unique(self.rec["kind"]) if k <= PORT})


@functools.lru_cache(maxsize=None)
def node_edges(topology):
    return NodeEdges(topology)


def node_launch(s, name, counters):
    """(Tuning knobs, expected plan or None) of a node set's edge launch: "default" (no knob set),
    "stage0" and "per-table" from node_matrix's launches() -- the per-table path of a counted big
    set is its window launch at the default hist_window"""
    if name == "default":
        return {}, None
    launches = s.launches(counters)
    if name == "per-table" and name not in launches:
        name = "window4096"
    return launches[name]


NODE_LAUNCHES = ("default", "stage0", "per-table")
NODE_TABLE_SETS = ("pair", "big-pair", "uncovered")
NODE_TABLE_FLOOR = 20


def node_table_pairs(name):
    """decisive pairs, per mode, whose inside probe is decided in a PAIR table of the set (pair,
    big-pair) / in its uncovered node-output table (uncovered)"""
    import node_matrix as nm
    s = nm.node_set(name)
    e = s.e
    tabs = [e.table_id("g")] if name == "uncovered" else [
        k for k in range(e.num_tables()) if e.table_stats(k)["structure"] == "pair"]
    return tuple(node_edges(s.spec.topology).decisive(m, tabs) for m in nm.MODES)


# topology -> {mode: decisive pairs per field kind}; set -> decisive pairs decided in its PAIR
# tables / its uncovered table, per mode (PERPOD, CONN); the oracle alone, on the CPU
NODE_MEASURED = {
    "big": {1: {'src': 1394, 'dst': 0, 'port': 1370}, 2: {'src': 1007, 'dst': 16, 'port': 1644}},
    "big-dst": {1: {'src': 1394, 'dst': 0, 'port': 1370}, 2: {'src': 1018, 'dst': 16, 'port': 1644}},
    "grouped": {1: {'src': 1072, 'dst': 0, 'port': 624}, 2: {'src': 2144, 'dst': 0, 'port': 624}},
    "mid": {1: {'src': 1394, 'dst': 0, 'port': 1370}, 2: {'src': 1004, 'dst': 16, 'port': 1644}},
    "pair": {1: {'src': 261, 'dst': 132, 'port': 266}, 2: {'src': 462, 'dst': 56, 'port': 193}},
    "small": {1: {'src': 104, 'dst': 32, 'port': 152}, 2: {'src': 156, 'dst': 58, 'port': 156}},
    "uncovered": {1: {'src': 752, 'dst': 132, 'port': 896}, 2: {'src': 268, 'dst': 72, 'port': 323}},
    "wide": {1: {'src': 1024, 'dst': 0, 'port': 748}, 2: {'src': 2048, 'dst': 0, 'port': 748}},
    "wide-big": {1: {'src': 2024, 'dst': 0, 'port': 2016}, 2: {'src': 4048, 'dst': 0, 'port': 2016}},
    "wide-mid": {1: {'src': 2024, 'dst': 0, 'port': 2016}, 2: {'src': 4048, 'dst': 0, 'port': 2016}},
}
NODE_TABLE_MEASURED = {
    "pair": (658, 617),
    "big-pair": (2764, 2676),
    "uncovered": (1524, 191),
}


# ---- reachability matrix and port sweep with edge end points ------------------------------------
REACH_SRC, REACH_DST, REACH_SVC = 64, 53, 64
REACH_PAIR_FLOOR = 50


class ReachEdges:
    """sides and services of a topology whose end points and ports sit on rule edges.

    src side (64): pods at the even positions, as reach_cases.sides places them, and at the odd
    ones 16 (outside, inside) address pairs from the edges of the ACLs' src nets, evenly spaced
    over the sorted pairs. dst side (53): the same with 13 pairs from the dst nets' edges (filled
    up from the src nets': CONN's SYN-ACK evaluations read the dst as src). Services: 32 (outside,
    inside) pairs of (protocol, 40000, port) over the port edges of the ACLs' ranges, the first
    three again with the port as src port, and reach_cases.services' OTHER / ANY / out-of-range
    codes. pair_* hold the positions of each pair on its side (outside, inside)."""

    def __init__(self, topology):
        import node_matrix as nm
        import reach_cases as rc
        self.name = topology
        self.t = t = nm.topo(topology)
        e = t.e
        nets, ports = {SRC: set(), DST: set()}, set()
        for n in e.ACLNames():
            for r in e.GetACLByName(n)["rules"]:
                f = rule_fields(r)
                if f is None:
                    continue
                for k in constrained(f):
                    v, ins = edge_values(f, k)
                    for o, i in ((0, 1), (3, 2)):
                        if ins[i] and not ins[o]:
                            (ports.add((f[4], v[o], v[i])) if k == PORT else nets[k].add((v[o], v[i])))
        pods = rc.end_points(t)[0]

        def side(n, pairs):
            out, pos = [], []
            for i in range(n):
                j, odd = divmod(i, 2)
                if not odd or j // 2 >= len(pairs):
                    out.append(pods[j % len(pods)])
                else:
                    out.append(pairs[j // 2][j % 2])
                    if j % 2:
                        pos.append((i - 2, i))
            return np.array(out, np.uint32), np.array(pos, np.int64).reshape(-1, 2)
        spairs = sorted(nets[SRC])
        dpairs = sorted(nets[DST])
        dpairs = _spaced(dpairs, REACH_DST // 4) + _spaced(spairs, max(0, REACH_DST // 4 - len(dpairs)))
        self.src, self.pair_src = side(REACH_SRC, _spaced(spairs, REACH_SRC // 4))
        self.dst, self.pair_dst = side(REACH_DST, dpairs[:REACH_DST // 4])
        pp = _spaced(sorted(ports), REACH_SVC // 2)
        svc = [(pr, 40000, p) for pr, o, i in pp for p in (o, i)]
        self.pair_svc = np.array([(2 * j, 2 * j + 1) for j in range(len(pp))], np.int64).reshape(-1, 2)
        self.svc = svc + [(pr, p, 40000) for pr, _, p in svc[:3]] + rc.services(e)[-6:]
        self.words = rc.oracle_words(t.world, self.src, self.dst, self.svc)

    def counts(self):
        """(ConnActions present, (src, dst, service) cells whose word differs between the inside
        and the outside end point of an address pair, ... of a port pair)"""
        w = self.words
        ends = int((w[:, self.pair_src[:, 0], :] != w[:, self.pair_src[:, 1], :]).sum() +
                   (w[:, :, self.pair_dst[:, 0]] != w[:, :, self.pair_dst[:, 1]]).sum())
        return sorted(np.unique(w >> 30).tolist()), ends, int((w[self.pair_svc[:, 0]] != w[self.pair_svc[:, 1]]).sum())

    def check_preconditions(self):
        acts, ends, ports = self.counts()
        assert acts == [0, 1, 2, 3] and ends >= REACH_PAIR_FLOOR, (self.name, acts, ends, ports)

    @functools.lru_cache(maxsize=None)
    def sweep(self, protocol):
        """(lo, hi, oracle words at every interval's first port, at its last) of the port sweep over
        the same sides; the bounds from the installed rules (ports_cases.cuts)"""
        import ports_cases as pc
        lo = pc.cuts(self.t.e, protocol)
        hi = (lo.astype(np.int64) + pc.lengths(lo) - 1).astype(np.uint32)
        return (lo, hi, pc.oracle_words(self.t.world, self.src, self.dst, protocol, lo),
                pc.oracle_words(self.t.world, self.src, self.dst, protocol, hi))


@functools.lru_cache(maxsize=None)
def reach_edges(topology):
    return ReachEdges(topology)


@functools.lru_cache(maxsize=None)
def reach_edge_hists(topology):
    """the oracle's rule-coverage histograms of a topology's edge product, summed over its services at
    weight 1: (evals [n_slots], cells [n_slots, 4]) (rules_cases.slice_hists)"""
    import rules_cases as kr
    r = reach_edges(topology)
    return kr.weighted(*kr.slice_hists(r.t.world, r.src, r.dst, r.svc))


# topology -> (ConnActions present, end-point pair cells that differ, port pair cells that differ)
REACH_MEASURED = {
    "big-dst": ([0, 1, 2, 3], 29872, 7020),
    "grouped": ([0, 1, 2, 3], 29415, 240),
    "pair": ([0, 1, 2, 3], 18191, 292),
    "small": ([0, 1, 2, 3], 27051, 1776),
    "uncovered": ([0, 1, 2, 3], 8210, 1564),
    "wide": ([0, 1, 2, 3], 28945, 194),
}
