"""End-point resolution at its edges, without a GPU: what tests/test_gpu_endpoints.py presupposes of
the layouts of tests/endpoint_cases.py, and the kernels' host twins on them.

Preconditions, from the oracle and pg_debug_endpoint_probe alone: the chain, the wrap and the long
misses are reached; every ConnAction and every slot of the pods' ACLs; every single-end-point
mutation of the World changes the oracle's words (endpoint_cases.MUTATIONS). Then
pg_debug_classify_host (PERPOD and CONN, counted, node classifier and per-table path),
pg_debug_reach_matrix_host, pg_debug_reach_rules_host and pg_debug_reach_ports_host (TCP) against the
oracle, bit for bit; and the regression tests of build_node's failure contract: an engine over
budget has no node at all.
"""
import ctypes as C

import numpy as np
import pytest

import edge_cases as ec
import endpoint_cases as ep
import node_matrix as nm
import ports_cases as pc
import reach_cases as rc
import rules_cases as kr
from oracle.world import World, winners
from vpp_amd._capi import lib


@pytest.mark.parametrize("name", ep.LAYOUTS)
def test_preconditions(name):
    L = ep.layout(name)
    assert L.check_preconditions() == ep.MUTATIONS[name]
    assert set(ep.MUTATIONS) == set(ep.LAYOUTS)
    assert len(L.tup[0]) == L.words.size < 200000


def test_search_hash_is_the_engines():
    """hash_ip as restated for the address search starts every probe where the engine does"""
    L = ep.layout("growth-57")
    ips = np.concatenate([L.src, np.array(ep.scattered(300), np.uint32)])
    _, slot, cap = L.e.debug_endpoint_probe(ips)
    assert cap == 256 and np.array_equal(slot, ep.hash_ip(ips) & np.uint32(cap - 1))


def test_chain_and_wrap_cells():
    for name, first in (("chain", ep.CHAIN_SLOT), ("wrap", ep.WRAP_SLOT)):
        L = ep.layout(name)
        steps, slot, cap = L.e.debug_endpoint_probe(np.array([ip for _, ip, _ in L.pods] + L.miss, np.uint32))
        assert (slot[:9] == first).all() and steps[:9].tolist() == list(range(1, 10))   # PodID order fills the chain
        assert slot[9:].tolist() == [(first + j) % cap for j in range(10)]
        assert steps[9:].tolist() == [10 - j for j in range(9)] + [1]


def test_scattered_counts_are_the_bisection():
    assert ep.bisect_scattered() == (ep.SCATTERED_SMALL, ep.SCATTERED_BIG)
    for name, node in (("scattered-small", True), ("scattered-big", False)):
        L = ep.layout(name)
        assert L.has_node() == node and L.e.num_tables() > 64


def test_repeat_layout_has_every_pairing_in_both_orders():
    L = ep.layout("repeat")
    seen = set()
    by_ip = {}
    for name, ip, kind in L.pods:
        by_ip.setdefault(ip, []).append(kind)
    for ip, kinds in by_ip.items():
        if len(kinds) == 2:
            seen.add(tuple(kinds))
            tap, another = winners(L.regs)[ip]
            assert (ep.REMOTE if another else ep.LOCAL if tap else ep.NOIF) == kinds[1]   # the later pod
    assert seen == {(ep.LOCAL, ep.REMOTE), (ep.REMOTE, ep.LOCAL), (ep.LOCAL, ep.NOIF), (ep.NOIF, ep.LOCAL), (ep.LOCAL, ep.LOCAL)}
    both = [ip for ip, kinds in by_ip.items() if kinds == [ep.LOCAL, ep.LOCAL]]
    taps = {ip: [t for _, a, t, _ in L.regs if a == ip] for ip in both}
    assert len(both) == 2 and all(winners(L.regs)[ip][0] == t[1] != t[0] for ip, t in taps.items())


def test_world_lets_the_last_pod_win_without_a_pod_list():
    """World(local_ifs, ...) with the remote pods read off the engine's RegisterPod calls: an address
    registered for a pod of this node and for one of another node goes to the later PodID"""
    from vpp_amd import renderer as R
    e = R.Engine(0)
    e.SetVxlanBVIIfName(ep.NODE_IF)
    e.SetPodIfName("ns/a", "tap0")
    e.SetPodIfName("ns/d", "tap1")
    for pod, ip, another in (("ns/a", "10.1.0.1", False), ("ns/b", "10.1.0.1", True), ("ns/c", "10.1.0.2", True), ("ns/d", "10.1.0.2", False)):
        e.RegisterPod(pod, ip, another)
    e.num_tables()
    w = World(e, {0x0A010001: "tap0", 0x0A010002: "tap1"}, ep.NODE_IF)
    ips = np.array([0x0A010001, 0x0A010002], np.uint32)
    assert w.kind(ips).tolist() == [1, 0]
    tup = (np.repeat(ips, 2), np.tile(ips, 2), np.zeros(4, np.uint16), np.zeros(4, np.uint16), np.full(4, 3, np.uint8))
    act, slot = w.conn(*tup)
    for node in (True, False):
        got = e.debug_classify_host(nm.MODE_CONN, -1, *tup, node=node)
        assert np.array_equal(got, (act.astype(np.uint32) << 30) | slot)


@pytest.mark.parametrize("name", ep.LAYOUTS)
def test_launch_plans(name):
    """the launches tests/test_gpu_endpoints.py makes take the path and staging they are named for"""
    L = ep.layout(name)
    for launch in ec.NODE_LAUNCHES:
        for counters in (False, True):
            with L.e.tuning(**L.launch(launch, counters)):
                for mode in nm.MODES:
                    L.check_plan(launch, mode, counters)


def classify_equals_oracle(e, L, what):
    for mode in nm.MODES:
        act, slot, hist = L.expected(mode)
        for node in (True, False):
            got, cnt = e.debug_classify_host(mode, -1, *L.tup, counters=True, node=node)
            bad = nm.mismatches(got, act, slot)
            assert len(bad) == 0, (what, mode, node, len(bad), bad[:8], got[bad[:4]], act[bad[:4]], slot[bad[:4]])
            assert np.array_equal(cnt, hist), (what, mode, node, np.nonzero(cnt != hist)[0][:8])


@pytest.mark.parametrize("name", ep.LAYOUTS)
def test_host_classify_equals_oracle(name):
    L = ep.layout(name)
    classify_equals_oracle(L.e, L, name)


@pytest.mark.parametrize("name", ep.LAYOUTS)
def test_reach_host_twins_equal_oracle(name):
    L = ep.layout(name)
    wev, wce = kr.weighted(L.ev, L.ce)
    for node in (True, False):
        packed, words = L.e.debug_reach_matrix_host(L.src, L.dst, ep.SERVICES, words=True, node=node)
        assert (words == L.words).all(), (node, rc.mismatch_report(words, L.words))
        assert (packed == rc.pack(L.words)).all(), node
        for evals, cells in ((True, True), (True, False), (False, True)):
            got = kr.run_host(L.e, L.src, L.dst, ep.SERVICES, evals=evals, cells=cells, node=node)
            kr.same(got, wev, wce, (name, node, evals, cells))
            assert got[2] == kr.want_result(L.e, L.src, L.dst, np.ones(len(ep.SERVICES)), wev, evals=evals)


@pytest.mark.parametrize("name", ep.LAYOUTS)
def test_reach_ports_host_equals_oracle(name):
    L = ep.layout(name)
    lo = pc.cuts(L.e, pc.TCP)
    first = pc.oracle_words(L.world, L.src, L.dst, pc.TCP, lo)
    got_lo, codes, n_open, words = L.e.debug_reach_ports_host(L.src, L.dst, pc.TCP, pc.SPORT)
    assert np.array_equal(got_lo, lo) and len(lo) >= 3
    assert (words == first).all(), pc.mismatch_report(words, first)
    assert (codes == pc.pack(first >> 30)).all()
    assert (n_open == (((first >> 30) == pc.ALLOW) * pc.lengths(lo)).sum(axis=2)).all()


# ---- build_node's failure contract --------------------------------------------------------------
def test_an_engine_over_the_node_budget_has_no_node():
    """scattered-big's node image outgrows its 16-bit map offsets after the IPv4 trie is built: no node
    at all, not a trie without records (fastpath.cpp build_node)"""
    L = ep.layout("scattered-big")
    assert L.e.node_stats() is None
    v = [C.c_uint32(7), C.c_uint32(7), C.c_uint64(7), C.c_uint64(7)]
    assert lib.pg_node_stats(L.e.h, *[C.byref(x) for x in v]) == -2   # PG_ENOENT
    assert [x.value for x in v] == [7, 7, 7, 7]
    assert lib.pg_node_uniform(L.e.h) == -2
    for mode in nm.MODES:
        assert L.e.debug_node_launch_plan(mode, True)["path"] == "per-table"
        on = L.e.debug_classify_host(mode, -1, *L.tup, counters=True, node=True)
        off = L.e.debug_classify_host(mode, -1, *L.tup, counters=True, node=False)
        assert on[0].tobytes() == off[0].tobytes() and on[1].tobytes() == off[1].tobytes()
    classify_equals_oracle(L.e, L, "scattered-big")


def test_a_node_comes_back_when_the_set_fits_again():
    """one engine: scattered-big (no node), then its last pod leaves the IPv4 end points and a resync
    installs scattered-small's ACLs: a node again, and scattered-small's answers"""
    big, small = ep.layout("scattered-big"), ep.layout("scattered-small")
    assert [p[:2] for p in big.pods[:-1]] == [p[:2] for p in small.pods]
    e, _ = ep.build_engine(big.pods)
    assert e.node_stats() is None
    e.RegisterPod(big.pods[-1][0], "2001:db8::1", False)   # (no IPv4 address: not an end point of the tuples)
    ep.build_engine(small.pods, engine=e)
    assert e.node_stats() is not None and e.node_stats()["ip_classes"] == small.e.node_stats()["ip_classes"] > 0
    assert e.num_counter_slots() == small.n_slots
    classify_equals_oracle(e, small, "after the resync")
