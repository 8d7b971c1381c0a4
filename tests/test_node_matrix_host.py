"""The PERPOD / CONN kernel family x launch shape matrix without a GPU: everything
tests/test_gpu_node_matrix.py presupposes of its node sets, launch shapes and tuples, and the
kernels' per-tuple code on the host.

Per set of node_matrix.SETS: the structure node_stats() / table_stats() report against its
declaration, the plan pg_debug_node_launch_plan reports for every launch shape (both modes, with
and without counters) against the plan node_matrix.launches() expects, the oracle-side
preconditions of the tuples, and pg_debug_classify_host (node and per-table path, common rows on
and off) against oracle.world.World -- verdict action and slot bit for bit, counters equal to the
oracle's histogram. A last test collects (family, stage, hist_kind, mode) over every launch and
compares it with what launch_classify<1|2> can dispatch.
"""
import numpy as np
import pytest

import node_matrix as nm
import test_node_host as tn
from vpp_amd._capi import MODE_CONN, MODE_PERPOD

SETS = list(nm.SETS)


@pytest.mark.parametrize("name", SETS)
def test_set_structure(name):
    s = nm.node_set(name)
    sp, ns, e = s.spec, s.ns, s.e
    assert ns is not None
    assert (s.section, s.recs > 0, s.big, s.half16_s3()) == (sp.section, sp.recs, sp.big, sp.half3), (s.all, s.base, s.recs)
    assert ns["uniform"] == sp.uniform and ns["wide_records"] == (sp.family == "wide"), ns
    st = [e.table_stats(t)["structure"] for t in range(e.num_tables())]
    assert (st.count("pair") >= 3) == (sp.family == "generic"), st
    # the family as launched: + 96 uniform, + 128 wide, + 32 no PAIR tables
    assert e.debug_node_launch_plan(MODE_CONN)["stage"] & ~7 == nm.FAMILY_CODE[sp.family]
    # the image with a 32-bit histogram of every slot (or the largest slot cache) fits LDS
    assert 4 * s.all + (8193 * 8 if s.big else s.hist32) <= 160 << 10 and s.all <= nm.STAGE_WORDS_MAX
    if sp.topology == "small":  # lists, and common rows for some but not all (table, class) pairs
        assert (ns["list_table_bytes"] > 0) == sp.uniform and (ns["list_record_bytes"] > 0) == (not sp.uniform), ns
        assert (0 < ns["common_row_pairs"] < ns["table_ipclass_pairs"]) == sp.section, ns
        assert e.num_tables() <= 64
    if name == "nopair-rec-cross":
        assert ns["list_record_bytes"] > 0 and not ns["list_records_in_image"]
    if name == "uni-grouped":  # the fewest tables past 64
        assert e.num_tables() == 65
    if name == "uni-wide":  # the fewest tables with wide records (252: narrow)
        assert e.num_tables() == 253 and not tn._many_tables(252, 1, extra_pods=True)[0].node_stats()["wide_records"]
    if name == "uncovered":
        assert e.table_stats(e.table_id("g"))["structure"] == "cand" and e.table_info(e.table_id("g"))[1] == 101
    assert s.big == (name.startswith("big-"))
    if s.big and sp.family != "wide":  # few tables
        assert e.num_tables() <= 8


@pytest.mark.parametrize("name", SETS)
def test_launch_plans(name):
    s = nm.node_set(name)
    for counters in (False, True):
        for launch, (knobs, want) in s.launches(counters).items():
            with s.e.tuning(**knobs):
                for mode in nm.MODES:
                    p = s.check_plan(mode, counters, want)
                    assert p["stage_words"] % 4 == 0 and (p["stage_words"] > 0) == (p["stage"] & 7 != 0), (launch, p)
    assert s.e.debug_node_launch_plan(MODE_CONN, True)["hist_kind"] == ("cache" if s.big else "full32")


def test_what_the_launch_knobs_alone_do():
    """Two cells that are not what turning one knob suggests (both asserted through the plan):
    node_stage_max_words=0 alone still stages at STAGE 3 an image whose common-row section fits
    the kCommonStageExtraWords words past the cap, and node_common_lds_max=0 with counters makes
    every uniform set's histogram the 16-bit-cell one."""
    s = nm.node_set("uni-grouped")
    assert s.all <= nm.EXTRA_WORDS
    with s.e.tuning(node_stage_max_words=0):
        p = s.e.debug_node_launch_plan(MODE_CONN, False)
        assert p["stage"] & 7 == 3 and p["stage_words"] == s.all, p
    with s.e.tuning(node_common_lds_max=0):
        assert s.e.debug_node_launch_plan(MODE_CONN, True)["hist_kind"] == "half16"
        assert s.e.debug_node_launch_plan(MODE_CONN, False)["stage"] & 7 == 1
    s = nm.node_set("nopair-rec")
    with s.e.tuning(node_common_lds_max=0):
        assert s.e.debug_node_launch_plan(MODE_CONN, True)["hist_kind"] == "full32"


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name", SETS)
def test_oracle_preconditions(name, offset):
    nm.node_set(name).check_preconditions(offset)


@pytest.mark.parametrize("name", SETS)
def test_host_classify_equals_oracle(name):
    s = nm.node_set(name)
    for mode in nm.MODES:
        act, slot, hist = s.expected(mode)
        for node, common in ((True, True), (True, False), (False, True)):
            got, cnt = s.e.debug_classify_host(mode, -1, *s.tup, counters=True, node=node, common=common)
            bad = nm.mismatches(got, act, slot)
            assert len(bad) == 0, (mode, node, common, bad[:8], got[bad[:4]], act[bad[:4]], slot[bad[:4]])
            assert np.array_equal(cnt, hist), (mode, node, common, np.nonzero(cnt != hist)[0][:8])


@pytest.mark.parametrize("name", nm.RAGGED_SETS)
def test_ragged_batch_first_tuple_is_deferred(name):
    """tuple 0 of the ragged batch: ANY-protocol, between two local pods, evaluated (not
    unresolved) in both modes -- in CONN over a uniform node the packet k_node_any classifies"""
    r = nm.ragged(name)
    assert r.tup[4][0] > 2
    for mode in nm.MODES:
        act, slot, hist = r.expected(mode, 1)
        # (PERPOD: decided in dst's outbound ACL; CONN: its last evaluation may be of a pod without an inbound ACL)
        assert slot[0] < r.s.n_slots - (2 if mode == MODE_PERPOD else 1) and hist.sum() >= 1, (mode, slot)
        got, cnt = r.s.e.debug_classify_host(mode, -1, *(a[:1] for a in r.tup), counters=True)
        assert len(nm.mismatches(got, act, slot)) == 0 and np.array_equal(cnt, hist)
    assert r.s.e.debug_node_launch_plan(MODE_CONN)["defers_any"] == (name == "uni")
    assert not r.s.e.debug_node_launch_plan(MODE_PERPOD)["defers_any"]


def test_every_dispatchable_combination_ran():
    """(family, STAGE & 7, hist_kind, mode) over every launch of every set, as the plan reports
    them: each combination is run, or node_matrix.unreachable gives the reason launch_classify<1|2>
    cannot dispatch it"""
    ran = nm.coverage()
    for f in nm.FAMILIES:
        for st in (3, 1, 0):
            for k in nm.KINDS:
                why = nm.unreachable(f, st, k)
                for mode in nm.MODES:
                    assert ((f, st, k, mode) in ran) != bool(why), (f, st, k, mode, why)
    assert all(f in nm.FAMILIES and k in nm.KINDS for f, _, k, _ in ran)
