"""Node sets, launch shapes, tuples and oracle answers of the PERPOD / CONN kernel family x launch
shape matrix (test helper).

Shared by tests/test_node_matrix_host.py (structures, plans, oracle preconditions and the kernels'
per-tuple code on the host, no GPU) and tests/test_gpu_node_matrix.py (the same launches on the
device). Topologies come from tests/test_node_host.py (topology, _many_tables) and two builders
here for the sets of more slots than the LDS histogram; every set is an engine of its own, the
sets of one topology share its tuples and the oracle's answers (oracle.world.World: perpod,
conn(hist=True)). Everything is built on first use and cached for the process; nothing here
touches the GPU.

Sets (SETS: topology, compiler knobs, kernel family), each at the smallest size found on the CPU
that has the wanted structure and meets the preconditions below:

  set                  family   what it is
  uni                  uniform  topology(10 pods): 12 tables, narrow records, list-verdict table, common rows
                                for some (table, class) pairs; the image (13.4k words) fits the default caps
  uni-nocommon         uniform  the same under node_common=0: no common-row section
  uni-grouped          uniform  _many_tables(65): the fewest tables past 64, common-row marks grouped
  uni-wide             wide     _many_tables(253): the fewest tables with wide class records
  uni-mid              uniform  5 pods x 2048 rules: 10k slots and a section smaller than what 16-bit cells
                                save, the one shape at which they are reachable beside the staged section
  wide-mid             wide     _many_tables(253, rules=40): 10.5k slots over the same node classes -- 16-bit
                                cells beside the staged section on the wide build
  nopair               nopair   uni's topology under node_uniform=0 (its lists become dst records in the image)
  nopair-rec           nopair   ... under node_list_table=0: the same structure by the other knob
  nopair-rec-cross     nopair   ... and node_list_words=0: records in the cross array only
  nopair-rec-nocommon  nopair   node_list_table=0, node_common=0: records right after the base image
  uncovered            nopair   topology(10 pods, big=70) under cross_max_rules=64, pair=0: the 101-rule
                                node-output table is a candidate table the node does not cover (the
                                kernels' out-of-line eval_one); 17,000 rules are not needed for that
  pair                 generic  topology(10 pods) under pair=2: 13 PAIR tables in the node
  big-uni              uniform  5 pods x 4096 rules (64 src /24s x 64 port ranges): 20,512 slots in 8
                                tables, 129 IP and 321 key classes; compiles in 0.3 s
  big-nopair           nopair   the same under node_uniform=0
  big-pair             generic  the same rules with dst nets on three of four, under pair=2: PAIR tables
  big-wide             wide     _many_tables(253, rules=66): 17,068 slots, the slot cache on the wide build

Preconditions (NodeSet.check_preconditions, on the oracle's output alone, no tuple filtered): CONN
three ConnActions, PERPOD both actions; 20 deciding slots; hits on a default-deny slot, "no ACL"
and "unresolved"; CONN counter sum above n; 500 ANY-protocol tuples that are evaluated; 100
tuples decided by a rule with a dst net (uni / nopair*), in a PAIR table (pair, big-pair), in the
uncovered table (uncovered); big sets: deciding slots below and above 16382 and inside and outside
every window. topology(open_tail=True) / _many_tables(extra_pods=True) leave the deny-the-rest rule
off every third outbound ACL for the default-deny hits, and add a pod without ACLs, one without an
interface and a remote one where the topology had none.

Launch shapes (launches(): Tuning launch knobs only, computed per set from node_stats() byte counts
and the histogram bytes; all = image words, base = base image words, norec = image words without
the dst records, hist = LDS bytes of the launch's histogram, 0 uncounted). Staged shapes raise
node_stage_max_words to its maximum (36864) so that the LDS budget alone decides:

  stage3-all    node_common_lds_max = 160 KiB                    3, records (if any) staged
  stage3-norec  node_common_lds_max = hist + 4 norec             3, lrec cleared (sets with a copy of the records in the image)
  stage1-recs   (sets without a section, with records)           1, all words, records staged
  stage1-base   node_common_lds_max = hist + 4 base              1, base words (sets with a section: it no longer fits);
                or node_stage_max_words = base                                  (sets without: the records no longer fit)
  stage0        node_common_lds_max = hist + 4 base and          0 (node_stage_max_words = 0 alone still stages an image
                node_stage_max_words = 0                           of up to kCommonStageExtraWords words at STAGE 3)
  half16-s1     node_common_lds_max = 0                          1 + 16 + 256 (small uniform sets, counted)
  half16-s0     node_common_lds_max = 0, node_stage_max_words=0  0 + 16 + 256
  half16-s3     node_common_lds_max = hist16 + 4 all             3 + 16 + 256 (uni-mid, wide-mid: hist16 + 4 all < hist32 + 4 base)
  cacheN        node_hist_cells = N at stage3-all (big, counted) slot cache of N cells; 15 and 0: global atomics only
  global-s1/s0  node_hist_cells = 0 at stage1-base / stage0      global atomics only beside the other stagings
  windowN       node_path = 0, hist_window = N (big, counted)    per-table path, the first N slots in LDS
  per-table     node_path = 0 (every other case)                 per-table path
  bsN           block_stage = N at stage3-all (uni, pair)

(stage, cell width): with 32-bit cells every stage is reachable on every set -- hist + 4 base is
exactly the budget at which the 16-bit condition is still false. With 16-bit cells STAGE 3 needs
hist16 + 4 norec <= node_common_lds_max < hist32 + 4 base, i.e. a section of fewer bytes than two
per slot: unreachable on uni, uni-nocommon and uni-grouped, reachable on uni-mid.
On the wide family the same holds: unreachable on uni-wide (936 slots), reachable on wide-mid.
unreachable() gives the (family, stage, hist_kind) combinations launch_classify<1|2> cannot
dispatch, each with its reason; every other one is run by a set here.
"""
import functools
import random
import time

import numpy as np

import single_matrix as sm
import test_node_host as tn
from oracle.world import World
from vpp_amd._capi import MODE_CONN, MODE_PERPOD

N_TUPLES = 60003      # no multiple of 256 * 4 (nor is N_TUPLES - 1, the offset=1 batch)
LDS_SLOTS = 16382     # device.hpp kLdsHistCells
EXTRA_WORDS = 8192    # device.hpp kCommonStageExtraWords
NODE_IF = "VXLAN-BVI"
FAMILY_CODE = {"generic": 0, "nopair": 32, "uniform": 96, "wide": 96 + 128}
MODES = (MODE_PERPOD, MODE_CONN)


# ---- topologies ---------------------------------------------------------------------------------
def _big(dst, ports=64):
    """5 local pods with an outbound ACL of 4096 rules each -- every (src /24 of 64, port range of
    64) once, shuffled, the ranges' upper ends differing per table -- so the node has few IP and
    key classes for 20k slots; dst: a dst net on three rules of four (PAIR under pair=2). And a
    pod without ACLs, one without an interface, a remote pod, and the node-output table."""
    from vpp_amd import renderer as R
    from vpp_amd import workloads as W
    rnd = random.Random(41)
    e = R.Engine(0)
    e.SetMainInterfaceName("GbE")
    e.SetVxlanBVIIfName(NODE_IF)
    e.SetHostInterconnectIfName("VPP-Host")
    local, ops, pod_ips = {}, [], []
    for k in range(5):
        ip = 0x0A0A0000 | (k + 1)
        pod_ips.append(ip)
        e.SetPodIfName("ns/p%d" % k, "tap%d" % k)
        e.RegisterPod("ns/p%d" % k, W.ip_str(ip), False)
        local[ip] = "tap%d" % k
    bare, lost, far = 0x0A0A0011, 0x0A0A0012, 0x0A0A0013
    e.SetPodIfName("ns/bare", "tap-bare")
    e.RegisterPod("ns/bare", W.ip_str(bare), False)
    local[bare] = "tap-bare"
    e.RegisterPod("ns/lost", W.ip_str(lost), False)
    e.RegisterPod("ns/far", W.ip_str(far), True)
    for k in range(5):
        cells = [(i, j) for i in range(64) for j in range(ports)]
        rnd.shuffle(cells)
        rules = []
        for i, j in cells:
            r = {"action": rnd.choice([0, 1, 1, 2]), "src": "10.20.%d.0/24" % i, "dst": "",
                 ("tcp" if j % 2 else "udp"): {"src": [0, 65535], "dst": [1000 + 16 * j, 1000 + 16 * j + k]}}
            if dst and rnd.random() < 0.75:
                r["dst"] = rnd.choice(["10.10.0.0/16", "10.10.0.0/28", W.ip_str(pod_ips[k]) + "/32", "10.0.0.0/8"])
            rules.append(r)
        ops.append(("config/vpp/acls/v2/acl/out-tap%d" % k, {"name": "out-tap%d" % k, "rules": rules, "ingress": [],
                                                             "egress": ["tap%d" % k]}))
    for k in (0, 1):  # inbound ACLs: CONN evaluates them too (one reflective)
        inb = [{"action": 2, "src": "", "dst": ""}] if k else [
            {"action": j % 2, "src": "", "dst": "10.20.%d.0/24" % j} for j in range(8)]
        ops.append(("config/vpp/acls/v2/acl/in-tap%d" % k, {"name": "in-tap%d" % k, "rules": inb, "ingress": ["tap%d" % k],
                                                            "egress": []}))
    glob = [{"action": k % 2, "src": W.ip_str(pod_ips[k]) + "/32" if k < 5 else "10.20.%d.0/24" % k, "dst": ""}
            for k in range(12)]
    glob.append({"action": 1, "src": "", "dst": ""})
    ops.append(("config/vpp/acls/v2/acl/g", {"name": "g", "rules": glob, "ingress": [], "egress": [NODE_IF]}))
    e.ApplyTxn(True, ops)
    return e, (local, [lost]), pod_ips + [bare, lost, far]


# name -> builder of (engine, (local pods {ip: TAP}, pods without an interface), pod addresses)
TOPOLOGIES = {
    "small": lambda: tn.topology(random.Random(2012), n_pods=10, open_tail=True),
    "grouped": lambda: tn._many_tables(65, 965, extra_pods=True),
    "wide": lambda: tn._many_tables(253, 1153, extra_pods=True),
    "wide-mid": lambda: tn._many_tables(253, 1154, extra_pods=True, rules=40),
    "wide-big": lambda: tn._many_tables(253, 1155, extra_pods=True, rules=66),
    "uncovered": lambda: tn.topology(random.Random(73), n_pods=10, big=70, open_tail=True),
    "pair": lambda: tn.topology(random.Random(3001), n_pods=10, open_tail=True),
    "mid": lambda: _big(False, ports=32),
    "big": lambda: _big(False),
    "big-dst": lambda: _big(True),
}
REC = {"node_list_table": 0}


class Spec:
    """a set as declared: topology, compiler knobs, kernel family, and what decides its launch
    shapes -- a common-row section in the image, a copy of the dst records in the image, more slots
    than the LDS histogram, 16-bit cells reachable beside the staged section (NodeSet.half16_s3)
    -- all asserted against node_stats() and the plan by tests/test_node_matrix_host.py"""

    def __init__(self, topology, knobs, family, section=True, recs=False, big=False, half3=False):
        self.topology, self.knobs, self.family = topology, knobs, family
        self.section, self.recs, self.big, self.half3 = section, recs, big, half3
        self.uniform = family in ("uniform", "wide")


SETS = {
    "uni": Spec("small", {}, "uniform"),
    "uni-nocommon": Spec("small", {"node_common": 0}, "uniform", section=False),
    "uni-grouped": Spec("grouped", {}, "uniform"),
    "uni-wide": Spec("wide", {}, "wide"),
    "uni-mid": Spec("mid", {}, "uniform", half3=True),
    "wide-mid": Spec("wide-mid", {}, "wide", half3=True),
    "nopair": Spec("small", {"node_uniform": 0}, "nopair", recs=True),
    "nopair-rec": Spec("small", REC, "nopair", recs=True),
    "nopair-rec-cross": Spec("small", dict(REC, node_list_words=0), "nopair"),
    "nopair-rec-nocommon": Spec("small", dict(REC, node_common=0), "nopair", section=False, recs=True),
    "uncovered": Spec("uncovered", {"cross_max_rules": 64, "pair": 0}, "nopair", recs=True),
    "pair": Spec("pair", {"pair": 2}, "generic"),
    "big-uni": Spec("big", {}, "uniform", big=True),
    "big-nopair": Spec("big", {"node_uniform": 0}, "nopair", recs=True, big=True),
    "big-pair": Spec("big-dst", {"pair": 2}, "generic", big=True),
    "big-wide": Spec("wide-big", {}, "wide", big=True),
}
CACHE_CELLS = (8192, 256, 16, 15, 0)
WINDOWS = (1, 64, 4096, 16382)
BLOCK_SIZES = (256, 512, 1024)
BLOCK_SETS = ("uni", "pair")

FAMILIES = ("generic", "nopair", "uniform", "wide", "per-table")
KINDS = ("none", "full32", "half16", "cache", "global", "window")


def unreachable(family, stage, kind):
    """why launch_classify<1|2> never dispatches (family, STAGE & 7, hist_kind), or None"""
    if family == "per-table":
        if stage:
            return "the per-table path stages no node image"
        if kind in ("half16", "cache", "global"):
            return "the per-table path counts every slot in LDS, or a window of hist_window cells"
        return None
    if kind == "window":
        return "node launches over more than 16382 slots count through the slot cache or global atomics"
    if kind == "half16" and family in ("generic", "nopair"):
        return "16-bit cells are a build of the uniform layout only (STAGE & 64)"
    return None


TUPLE_SEED = {"big": 7000, "big-dst": 7001, "grouped": 7002, "pair": 7003, "small": 7004, "uncovered": 7005,
              "wide": 7006, "mid": 7007, "wide-mid": 7008, "wide-big": 7009}


def launch_names(name, counters):
    """the launch shapes of a set, from its declaration alone (test parametrisation)"""
    sp = SETS[name]
    out = []
    if sp.section:
        out += ["stage3-all"] + (["stage3-norec"] if sp.recs else []) + ["stage1-base", "stage0"]
    else:
        out += (["stage1-recs"] if sp.recs else []) + ["stage1-base", "stage0"]
    if counters and sp.uniform and not sp.big:
        out += ["half16-s1", "half16-s0"] + (["half16-s3"] if sp.half3 else [])
    if counters and sp.big:
        out += ["cache%d" % n for n in CACHE_CELLS] + ["global-s1", "global-s0"] + ["window%d" % n for n in WINDOWS]
    else:
        out += ["per-table"]
    if name in BLOCK_SETS:
        out += ["bs%d" % n for n in BLOCK_SIZES]
    return out


class Topology:
    def __init__(self, name):
        self.name = name
        t0 = time.time()
        self.e, self.local, self.pod_ips = TOPOLOGIES[name]()
        self.e.num_tables()
        self.build_seconds = time.time() - t0
        self.n_slots = self.e.num_counter_slots()
        self.world = World(self.e, self.local[0], NODE_IF, no_if_ips=self.local[1])
        self.tup = matrix_tuples(self.e, self.local[0], self.pod_ips, TUPLE_SEED[name])
        src, dst, sport, dport, proto = self.tup
        act, slot = self.world.perpod(src, dst, dport, proto, threads=4)
        self.exp = {MODE_PERPOD: (act.astype(np.uint32), slot.astype(np.uint32))}
        conn, cslot, hist = self.world.conn(src, dst, sport, dport, proto, threads=4, hist=True)
        self.exp[MODE_CONN] = (conn.astype(np.uint32), cslot.astype(np.uint32))
        self.conn_hist = hist.astype(np.uint64)
        # CONN's evaluations are not per tuple in the batch's order, so a prefix's histogram is the
        # oracle's over that prefix (computed on demand, cached)
        self._prefix_hist = {}

    def expected(self, mode, offset=0, n=None):
        """oracle (action, deciding slot, counter histogram) of tuples[offset:offset + n]"""
        n = N_TUPLES - offset if n is None else n
        act, slot = (a[offset:offset + n] for a in self.exp[mode])
        if mode == MODE_PERPOD:
            return act, slot, np.bincount(slot, minlength=self.n_slots).astype(np.uint64)
        if (offset, n) == (0, N_TUPLES):
            return act, slot, self.conn_hist
        if (offset, n) not in self._prefix_hist:
            src, dst, sport, dport, proto = (a[offset:offset + n] for a in self.tup)
            if n == 0:
                h = np.zeros(self.n_slots, np.uint64)
            else:
                h = self.world.conn(src, dst, sport, dport, proto, threads=4, hist=True)[2].astype(np.uint64)
            self._prefix_hist[(offset, n)] = h
        return act, slot, self._prefix_hist[(offset, n)]


@functools.lru_cache(maxsize=None)
def topo(name):
    return Topology(name)


def _acl_side(acl):
    """(field the ACL's own pod is on, TAP) of a per-pod ACL, (None, None) for the node-output one"""
    if acl.get("egress") and acl["egress"][0] != NODE_IF:
        return 1, acl["egress"][0]
    if acl.get("ingress") and acl["ingress"][0] != NODE_IF:
        return 0, acl["ingress"][0]
    return None, None


def matrix_tuples(e, local, pod_ips, seed):
    """test_node_host.tuples (60 % pod end points -- local, remote and the pod without an interface
    -- 2 % ANY-protocol, non-pod <-> non-pod pairs among the rest); 40 % of the tuples drawn inside
    the rules of an ACL instead (single_matrix.tuples_inside), with the ACL's own pod as the end
    point it is evaluated for (dst for an outbound ACL, src for an inbound one)"""
    g = np.random.default_rng(seed)
    a = tn.tuples(seed, N_TUPLES, pod_ips)
    out = [x.copy() for x in a]
    tap_ip = {ifn: ip for ip, ifn in local.items()}
    names = e.ACLNames()
    which = np.where(g.random(N_TUPLES) < 0.4, g.integers(0, len(names), N_TUPLES), -1)
    for k, name in enumerate(names):
        idx = np.nonzero(which == k)[0]
        acl = e.GetACLByName(name)
        if not len(idx) or not acl["rules"]:
            continue
        b = [x.copy() for x in sm.tuples_inside(acl["rules"], len(idx), seed + 100 + k)]
        side, tap = _acl_side(acl)
        if side is not None and tap in tap_ip:
            b[side][:] = tap_ip[tap]
            # the other end point: as drawn inside the rule, or a pod (so that CONN evaluates both sides)
            m = g.random(len(idx)) < 0.3
            b[1 - side][m] = np.array(pod_ips, np.uint32)[g.integers(0, len(pod_ips), int(m.sum()))]
        for f in (0, 1, 3):
            out[f][idx] = b[f]
        keep = a[4][idx] > 2  # the ANY-protocol packets stay
        out[4][idx] = np.where(keep, a[4][idx], b[4])
    return tuple(out)


# ---- sets ---------------------------------------------------------------------------------------
STAGE_WORDS_MAX = 36864  # the most node_stage_max_words takes


class NodeSet:
    def __init__(self, name):
        self.name, self.spec = name, SETS[name]
        self.family, self.uniform = self.spec.family, self.spec.uniform
        self.t = topo(self.spec.topology)
        t0 = time.time()
        if self.spec.knobs:
            self.e = TOPOLOGIES[self.spec.topology]()[0]
            for k, v in self.spec.knobs.items():
                self.e.set_tuning(k, v)
        else:
            self.e = self.t.e
        self.ns = self.e.node_stats()  # (compiles under the knobs)
        self.build_seconds = time.time() - t0 + (0 if self.spec.knobs else self.t.build_seconds)
        assert self.e.num_counter_slots() == self.t.n_slots
        self.n_slots = self.t.n_slots
        self.tup = self.t.tup
        self.n_rules = sum(self.e.table_info(t)[1] for t in range(self.e.num_tables()))
        ns = self.ns
        self.all = ns["image_bytes"] // 4
        self.base = ns["base_image_bytes"] // 4
        self.recs = ns["list_record_bytes"] // 4 if ns["list_records_in_image"] else 0
        self.norec = self.all - self.recs
        self.section = self.norec > self.base  # a common-row section was built
        self.big = self.n_slots > LDS_SLOTS
        self.hist32 = (self.n_slots + 2) * 4
        self.hist16 = ((self.n_slots + 1) // 2 + 1) * 4

    def expected(self, mode, offset=0, n=None):
        return self.t.expected(mode, offset, n)

    def half16_s3(self):
        """16-bit cells beside the staged section: only when the section (4 (norec - base) bytes)
        is smaller than what the narrower cells save -- hist16 + 4 norec < hist32 + 4 base"""
        return self.section and self.uniform and not self.big and self.hist16 + 4 * self.norec < self.hist32 + 4 * self.base

    def launches(self, counters):
        """{launch name: (Tuning launch knobs, the plan expected of both modes but for defers_any)}
        of this set with / without counters"""
        fam = FAMILY_CODE[self.family]
        if not counters:
            kind, cells, hist = "none", 0, 0
        elif not self.big:
            kind, cells, hist = "full32", self.n_slots, self.hist32
        else:
            kind, cells, hist = "cache", 256, (256 + 1) * 8  # node_hist_cells at its default
        cnt = 16 if kind == "full32" else 0
        recs = self.recs > 0
        wide_open = {"node_common_lds_max": 160 << 10, "node_stage_max_words": STAGE_WORDS_MAX}

        def plan(stage, words, recs, kind=kind, cells=cells, hist=hist, code=None, path="node"):
            return {"path": path, "stage": (fam + stage + cnt) if code is None else code, "stage_words": words,
                    "records_staged": recs, "hist_kind": kind, "hist_cells": cells, "hist_bytes": hist}

        def shapes(hb, **kw):
            """the staging shapes beside a histogram of hb bytes (kw: its plan fields)"""
            out = {}
            # the budget the base image just fits: no room for the section, and not yet 16-bit cells
            lds1 = hb + 4 * self.base
            if self.section:
                out["stage3-all"] = (dict(wide_open), plan(3, self.all, recs, **kw))
                if recs:
                    out["stage3-norec"] = (dict(wide_open, node_common_lds_max=hb + 4 * self.norec),
                                           plan(3, self.norec, False, **kw))
                out["stage1-base"] = (dict(wide_open, node_common_lds_max=lds1), plan(1, self.base, False, **kw))
                out["stage0"] = ({"node_common_lds_max": lds1, "node_stage_max_words": 0}, plan(0, 0, recs, **kw))
            else:
                if recs:
                    out["stage1-recs"] = (dict(wide_open), plan(1, self.all, True, **kw))
                out["stage1-base"] = (dict(wide_open, node_stage_max_words=self.base), plan(1, self.base, False, **kw))
                out["stage0"] = ({"node_stage_max_words": 0}, plan(0, 0, recs, **kw))
            return out

        out = shapes(hist)
        if counters and self.uniform and not self.big:
            h = {"kind": "half16", "cells": self.n_slots, "hist": self.hist16}
            code = lambda s: fam + s + 16 + 256  # noqa: E731
            out["half16-s1"] = (dict(wide_open, node_common_lds_max=0), plan(1, self.base, False, code=code(1), **h))
            out["half16-s0"] = ({"node_common_lds_max": 0, "node_stage_max_words": 0}, plan(0, 0, False, code=code(0), **h))
            if self.half16_s3():
                out["half16-s3"] = (dict(wide_open, node_common_lds_max=self.hist16 + 4 * self.all),
                                    plan(3, self.all, False, code=code(3), **h))
        pt = {"path": "per-table", "code": 0}
        if counters and self.big:
            for n in CACHE_CELLS:
                k = {"kind": "cache", "cells": n, "hist": (n + 1) * 8} if n >= 16 else {"kind": "global", "cells": 0, "hist": 0}
                first = list(shapes(k["hist"], **k).values())[0]
                out["cache%d" % n] = (dict(first[0], node_hist_cells=n), first[1])
            g = shapes(0, kind="global", cells=0, hist=0)
            for st in ("s1", "s0"):
                knobs, p = g["stage1-base" if st == "s1" else "stage0"]
                out["global-" + st] = (dict(knobs, node_hist_cells=0), p)
            for n in WINDOWS:
                out["window%d" % n] = ({"node_path": 0, "hist_window": n},
                                       plan(0, 0, False, kind="window", cells=n, hist=(n + 2) * 4, **pt))
        else:
            k = {"kind": "full32", "cells": self.n_slots, "hist": self.hist32} if counters else {}
            if counters and self.big:
                k = {}
            out["per-table"] = ({"node_path": 0}, plan(0, 0, False, **k, **pt))
        if self.name in BLOCK_SETS:
            first = list(out.values())[0]
            for bs in BLOCK_SIZES:
                out["bs%d" % bs] = (dict(first[0], block_stage=bs), first[1])
        assert list(out) == launch_names(self.name, counters), (list(out), launch_names(self.name, counters))
        return out

    def defers_any(self, mode, path="node"):
        """a k_node_any launch follows: CONN over a uniform node (PG_CONN_DEFER_ANY; PERPOD: off)"""
        return path == "node" and self.uniform and mode == MODE_CONN

    def check_plan(self, mode, counters, want):
        """the plan of the next launch under the knobs now set equals `want` (launches())"""
        p = self.e.debug_node_launch_plan(mode, counters)
        assert p == dict(want, defers_any=self.defers_any(mode, want["path"])), (self.name, mode, counters, p, want)
        return p

    # -- what a case presupposes of its tuples, on the oracle's output alone --
    def slot_tables(self):
        """table id of every rule / default slot (-1 for "no ACL" and "unresolved")"""
        return np.array([self.e.slot_info(s)[0] for s in range(self.n_slots)], np.int64)

    def check_preconditions(self, offset=0):
        e = self.e
        n = N_TUPLES - offset
        noacl, unres = self.n_slots - 2, self.n_slots - 1
        dflt = [e.table_info(k)[2] for k in range(e.num_tables())]
        proto = self.tup[4][offset:]
        for mode in MODES:
            act, slot, hist = self.expected(mode, offset)
            assert hist.sum() == n if mode == MODE_PERPOD else hist.sum() > n  # CONN: multi-evaluation connections
            assert len(np.unique(act)) >= (3 if mode == MODE_CONN else 2), np.unique(act)
            assert len(np.unique(slot)) >= 20
            assert hist[dflt].sum() > 0 and hist[noacl] > 0 and hist[unres] > 0, (hist[dflt].sum(), hist[noacl], hist[unres])
            assert ((proto > 2) & (slot != unres)).sum() >= 500, ((proto > 2) & (slot != unres)).sum()
            tab = self.slot_tables()[slot]
            if self.spec.topology == "small":
                assert self.decided_by_list_rule(slot) >= 100
            if self.family == "generic":
                pair = [k for k in range(e.num_tables()) if e.table_stats(k)["structure"] == "pair"]
                assert np.isin(tab, pair).sum() >= 100
            if self.name == "uncovered":
                assert (tab == e.table_id("g")).sum() >= 100
            if self.big:
                assert (slot < LDS_SLOTS).any() and (slot > LDS_SLOTS).any()
                for w in WINDOWS:
                    assert hist[:w].sum() > 0 and hist[w:].sum() > 0, w

    def decided_by_list_rule(self, slot):
        """tuples whose deciding rule has a dst net: the rules a cross entry keeps as a dst list"""
        e = self.e
        dst_rule = np.zeros(self.n_slots, bool)
        for name in e.ACLNames():
            base = e.table_info(e.table_id(name))[0]
            for i, r in enumerate(e.GetACLByName(name)["rules"]):
                net = sm._net(r.get("dst") or "")
                dst_rule[base + i] = bool(net and net[1])
        return int(dst_rule[slot].sum())


@functools.lru_cache(maxsize=None)
def node_set(name):
    return NodeSet(name)


# ---- tiny batches: prefixes of a batch whose first tuple is deferred to k_node_any -------------
RAGGED_SIZES = (0, 1, 2, 3, 4, 5, 7, 9, 255, 257, 1023, 4099)
RAGGED_SETS = ("uni", "pair")


class Ragged:
    """the first 4099 tuples of a set's batch with tuple 0 replaced by an ANY-protocol packet
    between two local pods that have outbound ACLs (the smallest k_node_any pass: n = 1), and the
    oracle's answers for every prefix"""

    def __init__(self, name):
        s = node_set(name)
        self.s = s
        tap_ip = {ifn: ip for ip, ifn in s.t.local[0].items()}
        pods = [tap_ip[n[4:]] for n in s.e.ACLNames() if n.startswith("out-tap") and n[4:] in tap_ip]
        n = max(RAGGED_SIZES)
        self.tup = tuple(a[:n].copy() for a in s.tup)
        self.tup[0][0], self.tup[1][0], self.tup[4][0] = pods[0], pods[1], 255
        self._exp = {}

    def expected(self, mode, n):
        if (mode, n) not in self._exp:
            src, dst, sport, dport, proto = (a[:n] for a in self.tup)
            w = self.s.t.world
            if n == 0:
                z = np.zeros(0, np.uint32)
                r = (z, z, np.zeros(self.s.n_slots, np.uint64))
            elif mode == MODE_PERPOD:
                act, slot = w.perpod(src, dst, dport, proto)
                r = (act.astype(np.uint32), slot.astype(np.uint32), np.bincount(slot, minlength=self.s.n_slots).astype(np.uint64))
            else:
                act, slot, hist = w.conn(src, dst, sport, dport, proto, hist=True)
                r = (act.astype(np.uint32), slot.astype(np.uint32), hist.astype(np.uint64))
            self._exp[(mode, n)] = r
        return self._exp[(mode, n)]


@functools.lru_cache(maxsize=None)
def ragged(name):
    return Ragged(name)


def mismatches(got, act, slot):
    """indices where the verdict words differ from the oracle's (action, slot)"""
    return np.nonzero(((got >> 30) != act) | ((got & 0x3FFFFFFF) != slot))[0]


def coverage():
    """{(family or "per-table", STAGE & 7, hist_kind, mode)} over every launch of every set, by the
    plan pg_debug_node_launch_plan reports under the launch's knobs"""
    ran = set()
    for name in SETS:
        s = node_set(name)
        for counters in (False, True):
            for launch, (knobs, _) in s.launches(counters).items():
                with s.e.tuning(**knobs):
                    for mode in MODES:
                        p = s.e.debug_node_launch_plan(mode, counters)
                        ran.add((s.family if p["path"] == "node" else "per-table", p["stage"] & 7, p["hist_kind"], mode))
    return ran
