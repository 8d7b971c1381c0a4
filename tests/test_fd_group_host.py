"""The FD group code on the host (no GPU): pg_debug_classify_host runs full groups of four tuples
through classify_fd_group -- the body of the kernels' STAGE 4 / 5 group loop -- and the remainder
one tuple at a time, as the kernels do. Against evalACL (the oracle, independent of the build),
verdict action and slot bit for bit and the hit counters equal to the oracle's slot histogram:
every table and ANY-protocol placement of tests/fd_pipeline_cases.py, at 0..9 tuples (no group, a
remainder only, one and two groups with every remainder) and at all 130003.
"""
import numpy as np
import pytest

import fd_pipeline_cases as fc
import single_matrix as sm

SIZES = tuple(range(10)) + (sm.N_TUPLES,)


@pytest.mark.parametrize("name", fc.TABLES)
def test_tables_are_fd_in_lds(name):
    t = fc.table(name)
    assert t.e.table_stats(t.tid)["structure"] == "fd"
    for counters in (False, True):
        assert t.e.debug_launch_plan(t.tid, counters)["stage"] == 4


def test_split_table_is_the_smallest_whose_walks_split():
    """an even number of reads per lookup (src depth + key depth + 1) means two different depths,
    which build_fd_blob keeps only when they differ by three or more: the split walk's loops run.
    One rule fewer and the walks share one depth (an odd number of reads)."""
    t = fc.table("split")
    assert len(t.rules) == fc.SPLIT_RULES and fc.reads_per_lookup(t) == 12
    assert fc.reads_per_lookup(fc.SplitTable(fc.SPLIT_RULES - 1)) == 11
    for name in fc.SM_TABLES:
        assert fc.reads_per_lookup(fc.table(name)) % 2 == 1, name


@pytest.mark.parametrize("placement", fc.PLACEMENTS)
@pytest.mark.parametrize("name", fc.TABLES)
def test_group_code_equals_oracle(name, placement):
    c = fc.case(name, placement)
    for n in SIZES:
        tup = [x[:n] for x in c.tup]
        got, cnt = c.e.debug_classify_host(0, c.tid, *tup, counters=True)
        act, slot = c.act[:n], c.slot[:n]
        bad = np.nonzero(((got >> 30) != act) | ((got & 0x3FFFFFFF) != slot))[0]
        assert len(bad) == 0, (n, bad[:8], got[bad[:4]], act[bad[:4]], slot[bad[:4]])
        hist = np.bincount(slot, minlength=c.n_slots).astype(np.uint64)
        assert np.array_equal(cnt, hist), (n, np.nonzero(cnt != hist)[0][:8])
