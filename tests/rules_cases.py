"""Products, weights, fixtures and oracle answers of the rule-coverage tests (test helper).

Shared by tests/test_rules_host.py (pg_debug_reach_rules_host and the plan, no GPU) and
tests/test_gpu_rules.py (pg_reach_rules on the device). Node sets, sides and services are those of
tests/reach_cases.py as they are; expected values come from the oracle alone:
  evals  World.conn(..., hist=True) of every service slice over np.repeat(src, n_dst), np.tile(dst,
         n_src), times the slice's weight, summed
  cells  np.bincount of reach_cases.oracle_words at 4 * slot + ConnAction, times the weight, summed

Preconditions (check_preconditions, on the oracle's output alone, before any product code runs): the
evals histogram differs from the slot marginal of the cells histogram (CONN counts every evaluation
it makes, the cells only the last), and at least 19 slots are hit.

dead_fixture(): the port-sweep fixture's four pods with one outbound ACL on tap0 whose rule 1 is a
copy of rule 0 -- no packet can reach it -- and whose rule 3 nothing of the product matches.
"""
import functools

import numpy as np

import node_matrix as nm
import ports_cases as pc
import reach_cases as rc
from oracle.world import World
from vpp_amd import device as D

FILL = 0xFFFFFFFFFFFFFFFF
GUARD = 5    # prefilled entries behind both outputs that must stay untouched
MAX_WEIGHT = 65536
SETS = rc.FORM_A_SETS + rc.FORM_B_SETS


def slice_hists(world, src, dst, svc):
    """the oracle's histograms of every service slice: (evals [n_svc, n_slots], cells [n_svc, n_slots,
    4]) as uint64"""
    n_slots = world.slot_unresolved + 1
    ns, nd = len(src), len(dst)
    ev = np.zeros((len(svc), n_slots), np.uint64)
    ce = np.zeros((len(svc), n_slots, 4), np.uint64)
    if not ns or not nd:
        return ev, ce
    words = rc.oracle_words(world, src, dst, svc)
    s, d = np.repeat(src, nd), np.tile(dst, ns)
    n = ns * nd
    for v, (pr, sp, dp) in enumerate(svc):
        h = world.conn(s, d, np.full(n, sp, np.uint16), np.full(n, dp, np.uint16), np.full(n, pr, np.uint8), hist=True)[2]
        ev[v] = h.astype(np.uint64)
        idx = ((words[v] & 0x3FFFFFFF).astype(np.int64) << 2) | (words[v] >> 30).astype(np.int64)
        ce[v] = np.bincount(idx.ravel(), minlength=4 * n_slots).astype(np.uint64).reshape(n_slots, 4)
    return ev, ce


def weighted(ev, ce, weights=None):
    """sum over the slices of weight * histogram -> (evals [n_slots], cells [n_slots, 4])"""
    w = np.ones(len(ev), np.uint64) if weights is None else np.asarray(weights, np.uint64)
    return (ev * w[:, None]).sum(axis=0, dtype=np.uint64), (ce * w[:, None, None]).sum(axis=0, dtype=np.uint64)


def weights(n_svc, seed=5):
    """a weight per service: 0, 1 and 65536 among random values of 0 .. 65536"""
    w = np.random.default_rng(seed).integers(0, MAX_WEIGHT + 1, n_svc).astype(np.uint32)
    for k, x in enumerate((0, 1, MAX_WEIGHT)[:n_svc]):
        w[(3 * k + 1) % n_svc] = x
    return w


@functools.lru_cache(maxsize=None)
def shape_hists(topology, n_src, n_dst):
    """(src, dst, services, per-slice evals, per-slice cells) of a shape of a topology's case"""
    c = rc.case(topology)
    src, dst, svc, _ = c.shape(n_src, n_dst)
    return (src, dst, svc) + slice_hists(c.t.world, src, dst, svc)


@functools.lru_cache(maxsize=None)
def case_hists(topology):
    """(src, dst, services, per-slice evals, per-slice cells) of a topology's 37 x 53 case, the
    preconditions checked"""
    c = rc.case(topology)
    ev, ce = slice_hists(c.t.world, c.src, c.dst, c.svc)
    check_preconditions(topology, *weighted(ev, ce))
    return c.src, c.dst, c.svc, ev, ce


def check_preconditions(name, ev, ce):
    marginal = ce.sum(axis=1)
    assert (ev != marginal).any(), (name, "every pair decided by its only evaluation")
    assert int((ev > 0).sum()) >= 19 and int((marginal > 0).sum()) >= 19, (name, int((ev > 0).sum()), int((marginal > 0).sum()))


def n_dead(e, ev):
    """rule slots (pg_slot_info rule index >= 0) without an evaluation in an oracle histogram"""
    return sum(1 for s in range(len(ev)) if e.slot_info(s)[1] >= 0 and not ev[s])


def want_result(e, src, dst, w, ev, evals=True):
    """the result struct a call must report for an oracle histogram"""
    n = len(ev)
    rule_slots = sum(1 for s in range(n) if e.slot_info(s)[1] >= 0)
    return {"n_slots": n, "layout_gen": D.counter_layout_gen(e), "n_cells": len(src) * len(dst) * int(np.asarray(w, np.uint64).sum()),
            "n_evals": int(ev.sum()) if evals else 0, "n_rule_slots": rule_slots, "n_dead_rules": n_dead(e, ev) if evals else 0}


def run_host(e, src, dst, svc, w=None, evals=True, cells=True, node=True):
    return e.debug_reach_rules_host(src, dst, svc, w, evals=evals, cells=cells, node=node)


def same(got, want_ev, want_ce, what=""):
    ev, ce = got[0], got[1]
    if ev is not None:
        bad = np.flatnonzero(ev != want_ev)
        assert not len(bad), (what, "evals", [(int(s), int(ev[s]), int(want_ev[s])) for s in bad[:5]], len(bad))
    if ce is not None:
        bad = np.argwhere(ce != want_ce)
        assert not len(bad), (what, "cells", [(tuple(int(x) for x in b), int(ce[tuple(b)]), int(want_ce[tuple(b)])) for b in bad[:5]], len(bad))


# ---- a dead rule by construction ---------------------------------------------------------------
DEAD_SERVICES = [(pc.TCP, 40000, 80), (pc.TCP, 40000, 81), (pc.UDP, 40000, 80), (3, 0, 0)]


@functools.lru_cache(maxsize=None)
def dead_fixture():
    """(engine, world, src, dst): rule 1 of "dup" copies rule 0 and can never decide; rule 3 (UDP port 9)
    meets no packet of DEAD_SERVICES; rules 0, 2 and the final deny do"""
    from vpp_amd import renderer as R
    from vpp_amd import workloads as W
    e = R.Engine(0)
    e.SetMainInterfaceName("GbE")
    e.SetVxlanBVIIfName(nm.NODE_IF)
    e.SetHostInterconnectIfName("VPP-Host")
    local = {}
    for k, ip in enumerate(pc.POD_IPS):
        e.SetPodIfName("ns/p%d" % k, "tap%d" % k)
        e.RegisterPod("ns/p%d" % k, W.ip_str(ip), False)
        local[ip] = "tap%d" % k
    first = {"action": 1, "src": "", "dst": "", "tcp": pc._l4(80, 80)}
    rules = [first, dict(first), {"action": 2, "src": "", "dst": "", "tcp": pc._l4(81, 81)},
             {"action": 1, "src": "", "dst": "", "udp": pc._l4(9, 9)}, {"action": 0, "src": "", "dst": ""}]
    e.ApplyTxn(True, [("config/vpp/acls/v2/acl/dup", {"name": "dup", "rules": rules, "ingress": [], "egress": ["tap0"]})])
    e.num_tables()
    world = World(e, local, nm.NODE_IF, no_if_ips=[])
    ips = np.array(pc.POD_IPS + [pc.OTHER[0]], np.uint32)
    return e, world, ips, ips


# ---- an engine with pods and no ACL: every evaluation at "no ACL" ---------------------------------
@functools.lru_cache(maxsize=None)
def bare_fixture():
    """(engine, world, pod addresses): four local pods, nothing installed"""
    from vpp_amd import renderer as R
    from vpp_amd import workloads as W
    e = R.Engine(0)
    e.SetMainInterfaceName("GbE")
    e.SetVxlanBVIIfName(nm.NODE_IF)
    e.SetHostInterconnectIfName("VPP-Host")
    local = {}
    for k, ip in enumerate(pc.POD_IPS):
        e.SetPodIfName("ns/p%d" % k, "tap%d" % k)
        e.RegisterPod("ns/p%d" % k, W.ip_str(ip), False)
        local[ip] = "tap%d" % k
    e.num_tables()
    return e, World(e, local, nm.NODE_IF, no_if_ips=[]), list(pc.POD_IPS)


# ---- prefilled, guarded host buffers, the wrappers' expected report, the PG_EINVAL calls ----------
def host_buffers(n_slots, evals=True, cells=True):
    ev = np.full(n_slots + GUARD, FILL, np.uint64) if evals else None
    ce = np.full(4 * n_slots + GUARD, FILL, np.uint64) if cells else None
    return ev, ce


def report_of(e, world, ev, ce):
    """what Engine.rule_coverage must return for oracle histograms, from the oracle's own slot layout"""
    row = lambda s, k: (k, int(ev[s]), [int(x) for x in ce[s]])
    acls, dead = {}, []
    for t, name in enumerate(world.names):
        base, dflt = int(world.base[t]), int(world.dflt[t])
        n_rules = len(e.GetACLByName(name)["rules"])
        acls[name] = [row(base + k, k) for k in range(n_rules)] + [row(dflt, -1)]
        dead += [(name, k) for k in range(n_rules) if not ev[base + k]]
    return {"acls": acls, "no_acl": row(world.slot_noacl, None)[1:], "unresolved": row(world.slot_unresolved, None)[1:],
            "dead_rules": dead}


def einval_calls(e, src, dst, svc, ev_ptr, ce_ptr):
    """(what, word of pg_last_error, spec or None, out_evals, out_cells, with result) of every PG_EINVAL"""
    n = e.num_counter_slots()
    keep = []

    def spec(w=None, n_slots=n, services=svc, **fields):
        s, k = D.rules_spec(src, dst, services, w, n_slots)
        keep.append(k)
        for f, v in fields.items():
            setattr(s, f, v)
        return s
    over = np.ones(len(svc), np.uint32)
    over[-1] = MAX_WEIGHT + 1
    calls = [
        ("null spec", "null spec", None, ev_ptr, ce_ptr, True),
        ("null result", "null spec or result", spec(), ev_ptr, ce_ptr, False),
        ("both outputs null", "both null", spec(), None, None, True),
        ("n_src", "2^20", spec(n_src=(1 << 20) + 1), ev_ptr, ce_ptr, True),
        ("n_dst", "2^20", spec(n_dst=(1 << 20) + 1), ev_ptr, ce_ptr, True),
        ("n_svc", "4096 services", spec(n_svc=4097), ev_ptr, ce_ptr, True),
        ("weight", "above 65536", spec(w=over), ev_ptr, ce_ptr, True),
        ("n_slots", "changed since", spec(n_slots=n + 1), ev_ptr, ce_ptr, True),
        # 2^20 x 2^20 pairs x 32 services of weight 65536 x 4 = 2^63 (the sides are never read)
        ("2^63", "2^63", spec(w=np.full(32, MAX_WEIGHT, np.uint32), services=[svc[0]] * 32, n_src=1 << 20, n_dst=1 << 20),
         ev_ptr, ce_ptr, True),
    ]
    return calls, keep
