"""End points, services and oracle answers of the reachability-matrix tests (test helper).

Shared by tests/test_reach_host.py (pg_debug_reach_matrix_host, no GPU) and tests/test_gpu_reach.py
(pg_reach_matrix on the device). Topologies and engines come from tests/node_matrix.py (topo,
node_set) as they are; expected values come from oracle.world.World.conn over np.repeat(src, n_dst),
np.tile(dst, n_src) per service -- every pair of every case is compared, nothing is filtered.

End points of a topology: its pods (the first 21 and the last 3 when there are more than 24);
acl_fuzz.ANCHORS[:4]; and for each ACL with rules (the first 15 and the last when there are more than
16) the three src addresses of single_matrix.tuples_inside(rules, 3, 11 + k) and its first dst
address. A side of length n alternates a pod (even positions: pod (i // 2) % npods) and a draw from
the other end points (odd positions), the draws from np.random.default_rng(12), all src draws first.

Services (services()): the 10 most frequent (protocol, lowest dst port) of the ACLs' TCP / UDP rules
with the port as dst port, the first three again with it as src port, and OTHER / ANY / out-of-range
protocol codes.

Preconditions (Case.check_preconditions, on the oracle's output alone, before any product code
runs): every ConnAction at least 250 times, at least 19 deciding slots, at least 50 same-interface
pairs, at least 2 distinct service slices (7 on grouped, wide, mid, big, big-dst).
"""
import functools
from collections import Counter

import numpy as np

import acl_fuzz
import node_matrix as nm
import single_matrix as sm

N_SRC, N_DST = 37, 53
SHAPES = ((1, 1), (1, 15), (1, 16), (1, 17), (3, 32), (37, 53), (64, 33))
MAX_SRC, MAX_DST = 64, 53  # the sides every shape is a prefix of
SLICE_FLOOR = {"grouped": 7, "wide": 7, "mid": 7, "big": 7, "big-dst": 7}
# set (tests/node_matrix.py SETS) -> what it exercises
FORM_A_SETS = ("uni", "uni-nocommon", "uni-grouped", "uni-wide")
FORM_B_SETS = ("nopair", "uncovered", "pair", "big-pair")


def services(e, k=10):   # the k most frequent (proto, lowest dst port) of the ACLs' TCP/UDP rules, ties by value
    cnt = Counter((pr, s["dst"][0]) for n in e.ACLNames() for r in e.GetACLByName(n)["rules"]
                  for pr, f in ((0, "tcp"), (1, "udp")) for s in [r.get(f)]
                  if s and s.get("dst") is not None and s["dst"][0] <= 65535 and s["dst"][0] <= s["dst"][1])
    top = sorted(cnt.items(), key=lambda kv: (-kv[1], kv[0]))[:k]
    svc = [(pr, 40000 + i, p) for i, ((pr, p), _) in enumerate(top)]
    svc += [(pr, p, 40000) for (pr, _, p) in svc[:3]]                       # the port as src port
    return svc + [(0, 0, 0), (2, 0, 0), (3, 0, 0), (3, 1234, 80), (7, 1, 2), (255, 65535, 65535)]


def end_points(t):
    """(pods, other end points) of a node_matrix.Topology, as u32 lists"""
    pods = list(t.pod_ips)
    if len(pods) > 24:
        pods = pods[:21] + pods[-3:]
    other = list(acl_fuzz.ANCHORS[:4])
    names = t.e.ACLNames()
    picked = list(range(len(names))) if len(names) <= 16 else list(range(15)) + [len(names) - 1]
    for k, idx in enumerate(picked):
        rules = t.e.GetACLByName(names[idx])["rules"]
        if not rules:
            continue
        src, dst = sm.tuples_inside(rules, 3, 11 + k)[:2]
        other += [int(x) for x in src] + [int(dst[0])]
    return [int(x) for x in pods], other


def sides(t, n_src, n_dst):
    pods, other = end_points(t)
    g = np.random.default_rng(12)

    def side(n):
        draws = g.integers(0, len(other), n // 2)
        return np.array([pods[(i // 2) % len(pods)] if i % 2 == 0 else other[draws[i // 2]] for i in range(n)],
                        np.uint32)
    src = side(n_src)
    return src, side(n_dst)


def oracle_words(world, src, dst, svc):
    """verdict words (ConnAction << 30 | deciding slot) [n_svc, n_src, n_dst] of the oracle"""
    ns, nd = len(src), len(dst)
    out = np.zeros((len(svc), ns, nd), np.uint32)
    if not ns or not nd:
        return out
    s, d = np.repeat(src, nd), np.tile(dst, ns)
    for v, (pr, sp, dp) in enumerate(svc):
        n = ns * nd
        act, slot = world.conn(s, d, np.full(n, sp, np.uint16), np.full(n, dp, np.uint16), np.full(n, pr, np.uint8))
        out[v] = ((act.astype(np.uint32) << 30) | slot.astype(np.uint32)).reshape(ns, nd)
    return out


def pack(words):
    """the packed layout of pg_reach_matrix from full words [n_svc, n_src, n_dst]: the ConnAction of
    dst j in bits [2 (j & 15), 2 (j & 15) + 1] of word j >> 4 of its row, padding bits zero"""
    nv, ns, nd = words.shape
    rw = (nd + 15) // 16
    out = np.zeros((nv, ns, rw), np.uint32)
    for j in range(nd):
        out[:, :, j >> 4] |= (words[:, :, j] >> 30) << np.uint32(2 * (j & 15))
    return out


class Case:
    """the 37 x 53 matrix of a topology and the sides the shape cases are prefixes of"""

    def __init__(self, topology):
        self.name = topology
        self.t = nm.topo(topology)
        self.svc = services(self.t.e)
        self.src, self.dst = sides(self.t, N_SRC, N_DST)
        self.words = oracle_words(self.t.world, self.src, self.dst, self.svc)
        self.check_preconditions()

    def counts(self):
        act = self.words >> 30
        sif, dif = self.t.world.resolve(self.src), self.t.world.resolve(self.dst)
        ks, kd = self.t.world.kind(self.src), self.t.world.kind(self.dst)
        # pairs the reference has a Connection* call for whose two end points share an interface
        same = int(((sif[:, None] == dif[None, :]) & (sif[:, None] >= 0) & (ks[:, None] + kd[None, :] < 3)).sum())
        slices = len({(self.words[v] >> 30).tobytes() for v in range(len(self.svc))})
        return {"actions": np.bincount(act.ravel(), minlength=4).tolist(),
                "slots": len(np.unique(self.words & 0x3FFFFFFF)), "same_if": same, "slices": slices}

    def check_preconditions(self):
        c = self.counts()
        assert min(c["actions"]) >= 250, (self.name, c)
        assert c["slots"] >= 19, (self.name, c)
        assert c["same_if"] >= 50, (self.name, c)
        assert c["slices"] >= SLICE_FLOOR.get(self.name, 2), (self.name, c)

    @functools.lru_cache(maxsize=None)
    def wide_sides(self):
        """(src[64], dst[53], oracle words) of the shape cases"""
        src, dst = sides(self.t, MAX_SRC, MAX_DST)
        return src, dst, oracle_words(self.t.world, src, dst, self.svc)

    def shape(self, n_src, n_dst, svc_sel=None):
        """(src, dst, services, expected words) of a shape: prefixes of the wide sides, the services
        svc_sel (indices; None = all)"""
        src, dst, words = self.wide_sides()
        sel = list(range(len(self.svc))) if svc_sel is None else list(svc_sel)
        return src[:n_src], dst[:n_dst], [self.svc[v] for v in sel], words[sel][:, :n_src, :n_dst]

    def any_services(self):
        return [v for v, s in enumerate(self.svc) if s[0] > 2]

    def no_any_services(self):
        return [v for v, s in enumerate(self.svc) if s[0] <= 2]


@functools.lru_cache(maxsize=None)
def case(topology):
    return Case(topology)


def set_case(set_name):
    """(node set, Case of its topology)"""
    s = nm.node_set(set_name)
    return s, case(s.spec.topology)


def mismatch_report(got, want, limit=5):
    bad = np.argwhere(got != want)
    return "%d of %d words differ; first (service, src, dst): %s" % (
        len(bad), want.size, [(tuple(int(x) for x in b), hex(int(got[tuple(b)])), hex(int(want[tuple(b)]))) for b in bad[:limit]])
