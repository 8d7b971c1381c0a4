"""End-point resolution at its edges on the GPU: the layouts of tests/endpoint_cases.py -- a collision
chain in the end-point hash, the same across the table's end, long misses, pods at the ends of the
address space, adjacent pods, pods on rule edges, the table's doubling sizes, scattered pods up to
and past the node classifier's budget, pods that share an address -- through every kernel that
resolves an address, against the oracle bit for bit (verdict word = action << 30 | slot, and the hit
counters) and byte for byte against the host twins. Everything presupposed of the layouts is
verified without a GPU by tests/test_endpoint_host.py.

  pg_classify      PERPOD and CONN, with and without counters, at edge_cases.NODE_LAUNCHES (default,
                   stage0, per-table) where the layout has a node classifier, at the default launch
                   where it has none (scattered-big); a sentinel in front of the batch
  pg_reach_matrix  full words and packed codes, at the default and under node_path = 0 (form A where
                   the node is uniform, form B otherwise)
  pg_reach_ports   TCP
  pg_reach_rules   evals and cells
  Engine.connections  every ordered pod pair of chain, wrap and extremes
"""
import numpy as np
import pytest
import torch

import edge_cases as ec
import endpoint_cases as ep
import node_matrix as nm
import ports_cases as pc
import reach_cases as rc
import rules_cases as kr
import test_gpu_edges as ge
import test_gpu_rules as gr

pytestmark = pytest.mark.gpu

from vpp_amd import device as D  # noqa: E402

batches = ge.batches   # (the module-scoped fixture: an edge batch on the device, uploaded once)


def cases():
    for name in ep.LAYOUTS:
        for launch in (ec.NODE_LAUNCHES if name != "scattered-big" else ("default",)):
            yield name, launch


@pytest.mark.parametrize("counters", [False, True], ids=["nocount", "count"])
@pytest.mark.parametrize("mode", nm.MODES, ids=["perpod", "conn"])
@pytest.mark.parametrize("name,launch", list(cases()))
def test_classify(name, launch, mode, counters, batches):
    L = ep.layout(name)
    assert L.has_node() == (name != "scattered-big")
    with L.e.tuning(**L.launch(launch, counters)):
        L.check_plan(launch, mode, counters)
        got, cnt = ge.launch(L.e, mode, -1, batches("endpoint-" + name, L.tup), 0, counters)
    ge.compare(got, cnt, L.expected(mode), L.rec, (name, launch, mode, counters))


@pytest.mark.parametrize("name", ep.LAYOUTS)
def test_reach_matrix(name):
    L = ep.layout(name)
    for knobs in ({}, {"node_path": 0}):
        with L.e.tuning(**knobs):
            packed, words = D.reach_matrix(L.e, L.src, L.dst, ep.SERVICES, words=True)
            torch.cuda.synchronize()
            host = L.e.debug_reach_matrix_host(L.src, L.dst, ep.SERVICES, words=True, node=not knobs)
        assert (ge.u32(words) == L.words).all(), (knobs, rc.mismatch_report(ge.u32(words), L.words))
        assert (ge.u32(packed) == rc.pack(L.words)).all(), knobs
        assert ge.u32(packed).tobytes() == host[0].tobytes() and ge.u32(words).tobytes() == host[1].tobytes(), knobs


@pytest.mark.parametrize("name", ep.LAYOUTS)
def test_reach_ports(name):
    L = ep.layout(name)
    lo = pc.cuts(L.e, pc.TCP)
    first = pc.oracle_words(L.world, L.src, L.dst, pc.TCP, lo)
    out = D.reach_ports(L.e, L.src, L.dst, pc.TCP, pc.SPORT, open_count=True, words=True)
    torch.cuda.synchronize()
    got_lo, codes, n_open, words = (out[0],) + tuple(ge.u32(x) for x in out[1:])
    assert np.array_equal(got_lo, lo)
    assert (words == first).all(), pc.mismatch_report(words, first)
    assert (codes == pc.pack(first >> 30)).all()
    assert (n_open == (((first >> 30) == pc.ALLOW) * pc.lengths(lo)).sum(axis=2)).all()
    host = L.e.debug_reach_ports_host(L.src, L.dst, pc.TCP, pc.SPORT)
    assert all(a.tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip((codes, n_open, words), host[1:]))


@pytest.mark.parametrize("name", ep.LAYOUTS)
def test_reach_rules(name):
    L = ep.layout(name)
    wev, wce = kr.weighted(L.ev, L.ce)
    for evals, cells in ((True, True), (True, False), (False, True)):
        got = gr.run_dev(L.e, L.src, L.dst, ep.SERVICES, evals=evals, cells=cells)
        kr.same(got, wev, wce, (name, evals, cells))
        gr.identical(got, kr.run_host(L.e, L.src, L.dst, ep.SERVICES, evals=evals, cells=cells), (name, evals, cells))
        assert got[2] == kr.want_result(L.e, L.src, L.dst, np.ones(len(ep.SERVICES)), wev, evals=evals)


@pytest.mark.parametrize("name", ("chain", "wrap", "extremes"))
def test_connections(name):
    """pg_connections resolves pods by name: every ordered pod pair, every service, against the words
    of the same addresses"""
    L = ep.layout(name)
    pos = {int(ip): i for i, ip in enumerate(L.src)}
    qs, want = [], []
    for a, ipa, _ in L.pods:
        for b, ipb, _ in L.pods:
            for v, (proto, sport, dport) in enumerate(ep.SERVICES):
                qs.append(("PodToPod", a, b, proto, sport, dport))
                want.append(L.words[v, pos[ipa], pos[ipb]])
    acts, slots = L.e.connections(qs)
    want = np.array(want, np.uint32)
    assert np.array_equal(np.array(acts, np.uint32), want >> 30)
    assert np.array_equal(np.array(slots, np.uint32), want & 0x3FFFFFFF)
