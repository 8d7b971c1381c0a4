"""The reachability matrix on the host (no GPU): pg_debug_reach_matrix_host runs the per-end-point,
per-service and per-pair code of pg_reach_matrix (reach.hpp, the templates the kernels instantiate)
against the oracle -- every pair of every case, nothing filtered (tests/reach_cases.py).

Form A (a uniform node: class records and key classes hoisted, conn_uni_q per pair) on uni,
uni-nocommon, uni-grouped (narrow records) and uni-wide (wide records); form B (iphash end points,
conn_q over TabEval) on the non-uniform node sets nopair, uncovered, pair and big-pair, on uni under
node_path = 0 and on uni with flags bit 0 clear. The ANY-protocol services take form B on every set.
"""
import ctypes as C

import numpy as np
import pytest

import kat_driver as kd
import node_matrix as nm
import reach_cases as rc
from oracle.world import World
from vpp_amd import _capi
from vpp_amd import device as D
from vpp_amd._capi import MODE_CONN, lib

# the oracle's counts of the 37 x 53 cases: pairs by ConnAction [DENY_SYN, DENY_SYN_ACK, ALLOW,
# FAILURE], deciding slots, same-interface pairs, distinct service slices
COUNTS = {
    "small": ([9379, 3372, 9156, 15352], 21, 54, 2),
    "grouped": ([21735, 5185, 260, 2235], 44, 57, 7),
    "wide": ([20482, 6034, 304, 2595], 49, 50, 8),
    "pair": ([9016, 5893, 6599, 15751], 21, 52, 3),
    "uncovered": ([8148, 8374, 8558, 12179], 19, 77, 5),
    "mid": ([14414, 2559, 5371, 14915], 125, 60, 15),
    "big": ([14465, 2523, 5356, 14915], 167, 60, 15),
    "big-dst": ([14489, 2441, 5965, 14364], 179, 64, 15),
}


def host(e, src, dst, svc, node=True):
    packed, words = e.debug_reach_matrix_host(src, dst, svc, words=True, node=node)
    return packed, words


def check(e, src, dst, svc, want, node=True):
    packed, words = host(e, src, dst, svc, node)
    assert (words == want).all(), rc.mismatch_report(words, want)
    assert (packed == rc.pack(want)).all(), "packed output differs from the words' top two bits"
    return packed, words


@pytest.mark.parametrize("topology", sorted(COUNTS))
def test_oracle_counts(topology):
    """the helper's recipe on the oracle alone: the preconditions (asserted by Case) and the counts"""
    c = rc.case(topology).counts()
    assert (c["actions"], c["slots"], c["same_if"], c["slices"]) == COUNTS[topology], c


@pytest.mark.parametrize("name", rc.FORM_A_SETS + rc.FORM_B_SETS)
def test_matrix_equals_oracle(name):
    s, c = rc.set_case(name)
    uni = s.e.node_stats()["uniform"]
    assert uni == (name in rc.FORM_A_SETS)
    if name == "uni-wide":
        assert s.e.node_stats()["wide_records"]
    _, w_node = check(s.e, c.src, c.dst, c.svc, c.words, node=True)
    _, w_tab = check(s.e, c.src, c.dst, c.svc, c.words, node=False)   # node path == per-table path
    assert (w_node == w_tab).all()


def test_form_b_by_knob():
    """uni under node_path = 0: every service through form B"""
    s, c = rc.set_case("uni")
    with s.e.tuning(node_path=0):
        check(s.e, c.src, c.dst, c.svc, c.words, node=True)


@pytest.mark.parametrize("name", ("uni", "uni-wide", "pair"))
def test_equals_classify_host(name):
    """the matrix == pg_debug_classify_host CONN on the materialised tuples"""
    s, c = rc.set_case(name)
    _, words = host(s.e, c.src, c.dst, c.svc)
    n = len(c.src) * len(c.dst)
    sa, da = np.repeat(c.src, len(c.dst)), np.tile(c.dst, len(c.src))
    for v, (pr, sp, dp) in enumerate(c.svc):
        got = s.e.debug_classify_host(MODE_CONN, -1, sa, da, np.full(n, sp, np.uint16), np.full(n, dp, np.uint16),
                                      np.full(n, pr & 0xFF, np.uint8))
        assert (got == words[v].ravel()).all(), (name, v)


@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ("uni", "pair"))
def test_shapes(name, shape):
    s, c = rc.set_case(name)
    sels = {"all": None, "one": [1], "any-only": c.any_services(), "no-any": c.no_any_services()}
    assert sels["any-only"] and sels["no-any"]
    for sel in sels.values():
        src, dst, svc, want = c.shape(shape[0], shape[1], sel)
        check(s.e, src, dst, svc, want)


def test_empty_sides_write_nothing():
    s, c = rc.set_case("uni")
    for ns, nd, nv in ((0, 5, 3), (5, 0, 3), (5, 5, 0), (0, 0, 0)):
        packed, words = host(s.e, c.src[:ns], c.dst[:nd], c.svc[:nv])
        assert (packed == 0xFFFFFFFF).all() and (words == 0xFFFFFFFF).all()   # the fill, untouched
    assert lib.pg_reach_row_words(0) == 0 and lib.pg_reach_row_words(16) == 1 and lib.pg_reach_row_words(17) == 2


def test_einval():
    s, c = rc.set_case("uni")
    e = s.e
    buf = np.zeros(64, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    spec, keep = D.reach_spec(c.src[:2], c.dst[:2], c.svc[:2])
    for fn, last in ((lib.pg_debug_reach_matrix_host, 1), (lib.pg_reach_matrix, None)):
        assert fn(e.h, None, p, None, last) == _capi.PG_EINVAL
        assert fn(e.h, C.byref(spec), None, None, last) == _capi.PG_EINVAL
        for field, n in (("n_src", (1 << 20) + 1), ("n_dst", (1 << 20) + 1), ("n_svc", 4097)):
            bad, _ = D.reach_spec(c.src[:2], c.dst[:2], c.svc[:2])
            setattr(bad, field, n)
            assert fn(e.h, C.byref(bad), p, None, last) == _capi.PG_EINVAL, field
    del keep


def test_duplicates_give_identical_rows_and_columns():
    s, c = rc.set_case("uni")
    src = np.concatenate([c.src[:9], c.src[:9]])
    dst = np.concatenate([c.dst[:20], c.dst[:20]])
    _, words = host(s.e, src, dst, c.svc)
    assert (words[:, :9] == words[:, 9:]).all() and (words[:, :, :20] == words[:, :, 20:]).all()
    assert (words[:, :9, :20] == rc.oracle_words(s.t.world, src[:9], dst[:20], c.svc)).all()


def test_recompile_drops_everything_hoisted():
    """after an ApplyTxn that changes one ACL the matrix is the new oracle's"""
    c = rc.case("small")
    e, local, _ = nm.TOPOLOGIES["small"]()   # an engine of this test's own
    check(e, c.src, c.dst, c.svc, c.words)
    name = [n for n in e.ACLNames() if len(e.GetACLByName(n)["rules"]) > 2][0]
    acl = e.GetACLByName(name)
    for r in acl["rules"]:
        r["action"] = {0: 1, 1: 0, 2: 0}[r["action"]]
    acl["rules"] = acl["rules"][1:]
    e.ApplyTxn(False, [("config/vpp/acls/v2/acl/" + name, acl)])
    want = rc.oracle_words(World(e, local[0], nm.NODE_IF, no_if_ips=local[1]), c.src, c.dst, c.svc)
    assert (want != c.words).any()
    check(e, c.src, c.dst, c.svc, want)


def test_reachability_kat():
    """Engine.reachability over all pods of TestCombinedRules == the oracle's connection_pod_to_pod"""
    sc = [x for x in kd.load("acl_renderer_kats.json") if x["name"] == "TestCombinedRules"][0]
    ora, prod = kd.OracleBackend(), kd.ProductBackend(gpu=False)
    assert not kd.run_scenario(ora, sc)
    kd.run_scenario(prod, sc)
    pods = [p for p, _, _ in sc["setup"]["pods"]]
    svc = sorted({(kd.PROTO[c["args"][2]], c["args"][3], c["args"][4]) for ph in sc["phases"] for c in ph["checks"]
                  if c["kind"] == "ConnectionPodToPod"}) + [(3, 0, 0), (2, 0, 0)]
    got = prod.engine.reachability(pods, pods, svc, host=True)
    assert got.shape == (len(svc), len(pods), len(pods)) and len(pods) >= 2
    for v, (pr, sp, dp) in enumerate(svc):
        for i, a in enumerate(pods):
            for j, b in enumerate(pods):
                assert got[v, i, j] == ora.engine.connection_pod_to_pod(a, b, pr, sp, dp), (svc[v], a, b)
    assert len(np.unique(got)) >= 2
