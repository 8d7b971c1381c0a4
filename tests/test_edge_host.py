"""Rule edges without a GPU: everything tests/test_gpu_edges.py presupposes of its edge batches
(tests/edge_cases.py), and the kernels' host twins on them.

The preconditions come from the oracle alone: decisive pairs per field kind at or above the floor,
every edge cell of every probed rule hit, the share of single-rule mutations the batch sees, each
equal to what edge_cases.MEASURED records; the structure and stage codes written down for the edge
tables; pg_debug_classify_host (SINGLE, PERPOD, CONN), pg_debug_reach_matrix_host,
pg_debug_reach_ports_host and pg_debug_reach_rules_host on the edge batches against the oracle, bit
for bit; and the C oracle itself on the probes against the pure-Python evalACL.
"""
import functools

import numpy as np
import pytest

import acl_fuzz as fz
import edge_cases as ec
import node_matrix as nm
import ports_cases as pc
import reach_cases as rc
import rules_cases as kr
import single_matrix as sm

TOPOLOGIES = sorted({sp.topology for sp in nm.SETS.values()})
REACH_SETS = rc.FORM_A_SETS + rc.FORM_B_SETS
REACH_TOPOLOGIES = sorted({nm.SETS[s].topology for s in REACH_SETS})


# ---- the probes ---------------------------------------------------------------------------------
def test_probes_are_deterministic_and_shaped():
    rules = sm.lists_rules()
    (a, ra), (b, rb) = ec.probes(rules, seed=5), ec.probes(rules, seed=5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(ra, rb)
    n = len(a[0])
    assert n % 256 and (n - 1) % 256 and n < ec.MAX_TUPLES and len(ra) == n
    # every well-formed rule with a constrained field is probed: four edge values per field, the
    # port's again under three other protocol codes
    idx = ec.select(rules, 2000)
    assert len(idx) == 40   # (all but the catch-all)
    for i in idx:
        f = ec.rule_fields(rules[i])
        for k in ec.constrained(f):
            m = (ra["rule"] == i) & (ra["kind"] == k)
            field = a[0] if k == ec.SRC else a[1] if k == ec.DST else a[3]
            assert field[m].tolist() == ec.edge_values(f, k)[0] and ra["pos"][m].tolist() == [0, 1, 2, 3]
            assert (a[4][m] == f[4]).all()
        m = (ra["rule"] == i) & (ra["kind"] == ec.ALT)
        assert m.sum() == 12 and sorted(set(a[4][m].tolist()) - {1, 2}) in ([3], [7], [255])
        assert a[3][m].tolist() == ec.edge_values(f, ec.PORT)[0] * 3
    # the extremes: the whole cross product, once
    ext = ra["kind"] == ec.EXTREME
    assert ext.sum() == 6 * 6 * 6 * 5
    got = set(zip(a[0][ext].tolist(), a[1][ext].tolist(), a[3][ext].tolist(), a[4][ext].tolist()))
    assert got == {(s, d, p, c) for s in ec.EXT_ADDR for d in ec.EXT_ADDR for p in ec.EXT_PORT for c in ec.EXT_PROTO}


def test_probes_pad_to_a_ragged_length():
    """a batch whose length, or length - 1, would be a multiple of 256 is padded with its first tuple"""
    seen = set()
    for n in range(44, 56):   # 1080 extremes + 4 probes per rule: 1080 + 4 * 50 = 1280 = 5 * 256
        rules = [{"action": 1, "src": "10.0.%d.0/24" % k, "dst": ""} for k in range(n)]
        tup, rec = ec.probes(rules)
        pad = int((rec["kind"] == ec.PAD).sum())
        assert len(tup[0]) == 1080 + 4 * n + pad and len(tup[0]) % 256 and (len(tup[0]) - 1) % 256
        assert pad == (2 if n == 50 else 0)   # (a batch is a multiple of 4 long: never 1 mod 256)
        if pad:
            assert all((a[-pad:] == a[0]).all() for a in tup)
        seen.add(pad)
    assert seen == {0, 2}


def test_selection_is_even_and_keeps_both_ends():
    rules = sm.nested_rules(1, 2500, True)
    idx = ec.select(rules, 2000)
    assert len(idx) == 2000 and idx[0] == 0 and idx[-1] == 2499 and max(np.diff(idx)) <= 2
    assert ec.select(rules[:2000], 2000) == list(range(2000))
    bad = [{"action": 1, "src": "abc", "dst": ""}, {"action": 1, "src": "", "dst": "", "macip": True},
           {"action": 1, "src": "10.0.0.0/8", "dst": "", "tcp": {"src": [0, 65535], "dst": [500, 400]}},
           {"action": 1, "src": "", "dst": ""}, {"action": 1, "src": "10.0.0.0/8", "dst": "::ffff:10.0.0.0/104"}]
    assert ec.select(bad, 2000) == []


# ---- SINGLE: structures, stage codes, preconditions ---------------------------------------------
@pytest.mark.parametrize("name", list(ec.EDGE_SPECS) + list(ec.OTHER_STAGES))
def test_structure_and_stage_codes(name):
    t = ec.table(name)
    assert t.e.table_stats(t.tid)["structure"] == t.structure
    for launch, knobs in sm.LAUNCHES.items():
        with t.e.tuning(**knobs):
            for counters in (False, True):
                assert t.e.debug_launch_plan(t.tid, counters)["stage"] == t.stages[launch], (launch, counters)


def test_edge_tables_reach_every_form():
    forms = {ec.EDGE_FORMS[n][0].replace("cross+lists", "cross") for n in ec.EDGE_SPECS}
    assert set(ec.REQUIRED_FORMS) - set(ec.UNREACHABLE) <= forms and not ec.UNREACHABLE
    assert len(ec.ladder_rules("src")) == 32 and len(ec.EDGE_SPECS) == 17
    # the four knob sets of the matrix for every table; ladder-src once more, for CANDI
    assert {n.partition("+")[2] for n in ec.EDGE_SPECS if not n.startswith("ladder-src")} == set(ec.KNOBS)


def test_every_stage_code_is_launched_on_an_edge_batch():
    ran = {st for n in ec.SINGLE_TABLES for st in ec.table(n).stages.values()}
    assert ran == set(sm.ALL_STAGES)
    fd = {n for n in ec.SINGLE_TABLES if ec.table(n).stages["default"] == 4}
    assert set(ec.FD_TABLES) == fd - set(ec.EXEMPT) and {"fd", "split", "ladder-src"} <= fd


@pytest.mark.parametrize("name", ec.SINGLE_TABLES)
def test_single_preconditions(name):
    t = ec.table(name)
    dec, old, new, (n_mut, seen_edge, seen_random) = m = t.measured()
    assert m == ec.MEASURED[name], m
    assert set(ec.MEASURED) == set(ec.SINGLE_TABLES)
    if name in ec.EXEMPT:   # no rule edges: the extremes only
        assert new == (0, 0) and len(t.tup[0]) == 1080 and t.kinds() == []
        return
    assert t.kinds() and all(dec[k] >= t.floor() for k in t.kinds()), (dec, t.kinds(), t.floor())
    assert new[0] == new[1] == old[1] > 0 and old[0] < old[1], (old, new)
    assert n_mut > 0 and seen_edge >= seen_random and 2 * seen_edge >= n_mut, (n_mut, seen_edge, seen_random)


@pytest.mark.parametrize("name", ["cross", "pair-weird", "extremes", "ladder-both"])
def test_sees_equals_a_full_evaluation(name):
    """sensitivity()'s shortcut -- a widened rule changes exactly the tuples that went past it and
    match it -- against evalACL over the whole mutated table, for every rule and both batches"""
    t = ec.table(name)
    ract, _, ridx = t.oracle(t.random_tup)
    n = 0
    for k, r in enumerate(t.rules):
        if ec.rule_fields(r) is None:
            continue
        for mut in ec.mutations(r):
            n += 1
            assert ec.sees(mut, k, t.tup, t.idx) == ec.sees_full(t.rules, mut, k, t.tup, t.act.astype(np.int32), t.idx)
            assert ec.sees(mut, k, t.random_tup, ridx) == ec.sees_full(t.rules, mut, k, t.random_tup, ract.astype(np.int32), ridx)
    assert n >= 32


@pytest.mark.parametrize("name", ec.SINGLE_TABLES)
def test_single_host_classify_equals_oracle(name):
    t = ec.table(name)
    act, slot, hist = t.expected(0)
    for pred in (True, False):
        got, cnt = t.e.debug_classify_host(0, t.tid, *t.tup, counters=True, pred=pred)
        bad = np.nonzero(((got >> 30) != act) | ((got & 0x3FFFFFFF) != slot))[0]
        assert len(bad) == 0, (pred, bad[:8], t.rec[bad[:4]], got[bad[:4]], act[bad[:4]], slot[bad[:4]])
        assert np.array_equal(cnt, hist.astype(np.uint64)), pred


@functools.lru_cache(maxsize=None)
def _py_eval(rules_repr, name):
    """mismatches between the C oracle and the pure-Python evalACL on 2000 evenly spaced probes"""
    t = ec.table(name)
    pick = np.unique(np.round(np.linspace(0, len(t.tup[0]) - 1, 2000)).astype(np.int64))
    src, dst, _, dport, proto = (a[pick] for a in t.tup)
    a, i = fz.py_eval(fz.to_oracle_acl("t", t.rules), src, dst, dport, proto)
    return int(((a != t.act[pick].astype(np.int64)) | (i != t.idx[pick])).sum()), len(pick)


LARGE = ("pair-long", "linear", "split", "w-a-dst9k", "w-d-free9k")   # more than 400 rules


@pytest.mark.parametrize("name", [n for n in ec.SINGLE_TABLES if n not in LARGE])
def test_c_oracle_equals_python_evalacl_on_probes(name):
    """the oracle has not been probed at rule edges either: tables of up to 400 rules (the tables
    that share their rules are evaluated once)"""
    t = ec.table(name)
    assert len(t.rules) <= 400
    bad, n = _py_eval(repr(t.rules), name)
    assert bad == 0 and n == min(2000, len(t.tup[0]))


def test_py_eval_covers_every_small_table():
    assert all(len(ec.table(n).rules) > 400 for n in LARGE)


# ---- PERPOD / CONN ------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_node_preconditions(topology):
    n = ec.node_edges(topology)
    assert len(n.tup[0]) < ec.MAX_TUPLES and len(n.tup[0]) % 256 and (len(n.tup[0]) - 1) % 256
    # the reversed half: every probe again with its end points and ports exchanged
    k = n.n_probes
    src, dst, sport, dport, proto = n.tup
    assert np.array_equal(src[:k], dst[k:2 * k]) and np.array_equal(dst[:k], src[k:2 * k])
    assert np.array_equal(sport[:k], dport[k:2 * k]) and np.array_equal(dport[:k], sport[k:2 * k])
    assert np.array_equal(n.rec[:k], n.rec[k:2 * k]) and (n.rec["kind"][2 * k:] >= ec.EXTREME).all()
    # a probe keeps the end point that selects its ACL
    e = n.t.e
    tap_ip = {ifn: ip for ip, ifn in n.t.local[0].items()}
    for name in e.ACLNames():
        side, tap = nm._acl_side(e.GetACLByName(name))
        m = n.rec["acl"][:k] == e.table_id(name)
        if side is not None and m.any():
            assert (n.tup[side][:k][m] == tap_ip[tap]).all() and not (n.rec["kind"][:k][m] == (ec.SRC, ec.DST)[side]).any()
        elif m.any():   # the node interface's ACL: a dst is a local pod only where the rule's own dst net asks for it
            rules = e.GetACLByName(name)["rules"]
            pod = m & np.isin(dst[:k], list(tap_ip.values()))
            assert all(ec.rule_fields(rules[i])[3] > 0 for i in np.unique(n.rec["rule"][:k][pod])) and pod.sum() < m.sum() / 2
    got = {mode: n.decisive(mode) for mode in nm.MODES}
    assert got == ec.NODE_MEASURED[topology], got
    for mode in nm.MODES:
        floors = n.floors(mode)
        assert {"src", "port"} <= set(floors) and all(got[mode][kind] >= f for kind, f in floors.items()), (mode, got, floors)
        act, slot, hist = n.expected(mode)
        assert len(np.unique(act)) >= (3 if mode == nm.MODE_CONN else 2)
        assert hist.sum() == len(src) if mode == nm.MODE_PERPOD else hist.sum() > len(src)


@pytest.mark.parametrize("name", ec.NODE_TABLE_SETS)
def test_node_pairs_decided_in_the_sets_own_table_form(name):
    got = ec.node_table_pairs(name)
    assert got == ec.NODE_TABLE_MEASURED[name] and min(got) >= ec.NODE_TABLE_FLOOR, got


@pytest.mark.parametrize("name", list(nm.SETS))
def test_node_launch_plans(name):
    s = nm.node_set(name)
    for counters in (False, True):
        for launch in ec.NODE_LAUNCHES:
            knobs, want = ec.node_launch(s, launch, counters)
            with s.e.tuning(**knobs):
                for mode in nm.MODES:
                    p = s.e.debug_node_launch_plan(mode, counters)
                    if want is not None:
                        s.check_plan(mode, counters, want)
                    assert p["path"] == ("per-table" if launch == "per-table" else "node")
                    assert launch != "stage0" or p["stage"] & 7 == 0


@pytest.mark.parametrize("name", list(nm.SETS))
def test_node_host_classify_equals_oracle(name):
    s = nm.node_set(name)
    n = ec.node_edges(s.spec.topology)
    for mode in nm.MODES:
        act, slot, hist = n.expected(mode)
        got, cnt = s.e.debug_classify_host(mode, -1, *n.tup, counters=True, node=True)
        bad = nm.mismatches(got, act, slot)
        assert len(bad) == 0, (mode, bad[:8], n.rec[bad[:4]], got[bad[:4]], act[bad[:4]], slot[bad[:4]])
        assert np.array_equal(cnt, hist), (mode, np.nonzero(cnt != hist)[0][:8])


# ---- reachability matrix and port sweep ---------------------------------------------------------
@pytest.mark.parametrize("topology", REACH_TOPOLOGIES)
def test_reach_preconditions(topology):
    r = ec.reach_edges(topology)
    r.check_preconditions()
    assert r.counts() == ec.REACH_MEASURED[topology], r.counts()
    assert len(r.src) == 64 and len(r.dst) == 53 and len(r.pair_src) == 16 and len(r.pair_dst) == 13
    assert len(r.pair_svc) >= 12 and len(r.svc) == 2 * len(r.pair_svc) + 9
    pods = rc.end_points(r.t)[0]
    assert all(int(x) in pods for x in r.src[::2]) and all(int(x) in pods for x in r.dst[::2])
    # an address pair is two neighbours, a port pair two neighbouring ports of one protocol
    for side, pos in ((r.src, r.pair_src), (r.dst, r.pair_dst)):
        d = (side[pos[:, 1]].astype(np.int64) - side[pos[:, 0]].astype(np.int64)) % (1 << 32)
        assert np.isin(d, (1, (1 << 32) - 1)).all()
    for o, i in r.pair_svc:
        assert r.svc[o][0] == r.svc[i][0] and (r.svc[o][2] - r.svc[i][2]) % 65536 in (1, 65535)


@pytest.mark.parametrize("name", REACH_SETS)
def test_reach_matrix_host_equals_oracle(name):
    s = nm.node_set(name)
    r = ec.reach_edges(s.spec.topology)
    packed, words = s.e.debug_reach_matrix_host(r.src, r.dst, r.svc, words=True)
    assert (words == r.words).all(), rc.mismatch_report(words, r.words)
    assert (packed == rc.pack(r.words)).all()


@pytest.mark.parametrize("protocol", (pc.TCP, pc.UDP), ids=("tcp", "udp"))
@pytest.mark.parametrize("name", REACH_SETS)
def test_reach_ports_host_equals_oracle(name, protocol):
    s = nm.node_set(name)
    r = ec.reach_edges(s.spec.topology)
    lo, hi, first, last = r.sweep(protocol)
    assert len(lo) >= 3 and (first == last).all()   # the oracle itself: one word per (pair, interval)
    got_lo, codes, n_open, words = s.e.debug_reach_ports_host(r.src, r.dst, protocol, pc.SPORT)
    assert np.array_equal(got_lo, lo)
    assert (words == first).all(), pc.mismatch_report(words, first)
    assert (codes == pc.pack(first >> 30)).all()
    assert (n_open == (((first >> 30) == pc.ALLOW) * pc.lengths(lo)).sum(axis=2)).all()


@pytest.mark.parametrize("name", REACH_SETS)
def test_reach_rules_host_equals_oracle(name):
    """rule coverage of the edge product: evals and cells, together and each alone"""
    s = nm.node_set(name)
    r = ec.reach_edges(s.spec.topology)
    wev, wce = ec.reach_edge_hists(s.spec.topology)
    kr.check_preconditions(name, wev, wce)
    for evals, cells in ((True, True), (True, False), (False, True)):
        got = kr.run_host(s.e, r.src, r.dst, r.svc, evals=evals, cells=cells)
        kr.same(got, wev, wce, (name, evals, cells))
        assert got[2] == kr.want_result(s.e, r.src, r.dst, np.ones(len(r.svc)), wev, evals=evals)
