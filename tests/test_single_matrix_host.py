"""The SINGLE-mode form x stage matrix without a GPU: everything tests/test_gpu_single_matrix.py
presupposes of its tables, launches and tuples, and the kernels' per-tuple code on the host.

Per table of single_matrix.SPECS: the structure table_stats reports, the stage code and
histogram cells pg_debug_launch_plan reports for each launch, the oracle-side preconditions of
the tuples, and pg_debug_classify_host (predicated and branching walks, with counters) against
evalACL -- verdict action and slot bit for bit, counters equal to the histogram of the oracle's
slots. The same for the five-table set of the windowed hit counters.
"""
import numpy as np
import pytest

import single_matrix as sm

TABLES = list(sm.SPECS)


@pytest.mark.parametrize("name", TABLES)
def test_structure_and_launch_plan(name):
    t = sm.table(name)
    st = t.e.table_stats(t.tid)
    assert st["structure"] == t.spec.structure, st
    for launch, knobs in sm.LAUNCHES.items():
        with t.e.tuning(**knobs):
            for counters in (False, True):
                p = t.e.debug_launch_plan(t.tid, counters)
                assert p["stage"] == t.spec.stages[launch], (launch, p)
                # one table per engine: every slot fits the LDS histogram, or (linear: 16403) a window
                cells = t.n_slots if t.n_slots <= 16382 else t.e.get_tuning("hist_window")
                assert p["hist_cells"] == (cells if counters else 0), (launch, p)
                assert (p["stage_words"] > 0) == (p["stage"] & 7 != 0) and p["stage_words"] % 4 == 0, (launch, p)
            # the stage pg_debug_walk_stats reports stays the walk's view of it
            z = t.tup[0][:1]
            want = p["stage"] if p["stage"] in (4, 5) else (2 if p["stage"] & 7 == 6 else p["stage"] & 7)
            assert t.e.debug_walk_stats(t.tid, z, z, t.tup[3][:1], t.tup[4][:1])[2] == want


def test_residence_thresholds():
    """the forced forms sit at the smallest rule count with the wanted structure and residence"""
    words = lambda name: sm.table(name).e.table_stats(0)["blob_bytes"] // 4
    count = lambda name: len(sm.table(name).rules)
    # dst-testing cand: one rule fewer and the blob fits LDS
    assert words("cand-lds") <= 16384 < words("cand") and count("cand") == count("cand-lds") + 1
    # dst-free, HBM-resident (CANDI, or cand with candi = 0): one rule fewer and the blob fits LDS as cand
    assert words("cand-nodst-lds") <= 16384 < min(words(n) for n in ("cand-nodst", "candi-w11", "candi-w0"))
    for name in ("candi-w11", "candi-w0", "cand-nodst"):
        assert count(name) == count("cand-nodst-lds") + 1
    # CANDI that fits LDS: the level-compressed rebuild of a blob of lc_lds words or more, kept
    # while it fits; one rule fewer and the blob is below lc_lds, so "cand"
    for name in ("candi-lds", "candi-lds-w8"):
        t = sm.table(name)
        assert t.e.get_tuning("lc_lds") <= words(name) <= 16384
        e = sm.engine_with({"t": t.rules[:-1]}, t.spec.knobs)
        st = e.table_stats(0)
        assert st["structure"] == "cand" and st["blob_bytes"] // 4 < t.e.get_tuning("lc_lds"), st


def test_every_stage_code_is_launched():
    seen = {(sm.table(name).spec.structure, st) for name in TABLES for st in sm.table(name).spec.stages.values()}
    assert {st for _, st in seen} == set(sm.ALL_STAGES) and not sm.UNREACHABLE
    # candi: whole in LDS through the generic walk (9), root + window (14), nothing staged (8)
    assert {("candi", 9), ("candi", 14), ("candi", 8)} <= seen


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name", TABLES)
def test_oracle_preconditions(name, offset):
    sm.table(name).check_preconditions(offset)


@pytest.mark.parametrize("name", TABLES)
def test_host_classify_equals_oracle(name):
    t = sm.table(name)
    act, slot, hist = t.expected(0)
    for pred in (True, False):
        got, cnt = t.e.debug_classify_host(0, t.tid, *t.tup, counters=True, pred=pred)
        bad = np.nonzero(((got >> 30) != act) | ((got & 0x3FFFFFFF) != slot))[0]
        assert len(bad) == 0, (pred, bad[:8], got[bad[:4]], act[bad[:4]], slot[bad[:4]])
        assert np.array_equal(cnt, hist.astype(np.uint64)), pred


def test_window_set_structure_and_plan():
    w = sm.window_set()
    assert w.n_slots > 16382 and w.names == ["a-dst9k", "b-lists40", "c-empty", "d-free9k", "e-all"]
    assert [w.tid[n] for n in w.names] == list(range(5))
    st = {n: w.e.table_stats(w.tid[n]) for n in w.names}
    assert not st["a-dst9k"]["dst_free"] and st["a-dst9k"]["structure"] == "cross+lists"
    assert st["b-lists40"]["structure"] == "cross+lists" and st["d-free9k"]["structure"] == "fd"
    stages = {}
    for launch in ("default", "nostage"):
        with w.e.tuning(**sm.LAUNCHES[launch]):
            stages[launch] = [w.e.debug_launch_plan(w.tid[n], True)["stage"] for n in w.names]
    assert stages == {"default": [2, 1, 4, 5, 4], "nostage": [2, 2, 5, 5, 5]}, stages
    for cells in sm.WINDOWS:
        with w.e.tuning(hist_window=cells):
            for n in w.names:
                assert w.e.debug_launch_plan(w.tid[n], True)["hist_cells"] == cells
                assert w.e.debug_launch_plan(w.tid[n], False)["hist_cells"] == 0
                w.check_preconditions(n, cells)
    # the windows the cases are about
    assert w.window("a-dst9k", 4096) == (0, 4096) and w.window("d-free9k", 4096) == (9042, 4096)  # rule_base > 0
    assert w.window("d-free9k", 16382) == (w.n_slots - 16382, 16382)  # clipped: the default slots inside
    assert w.window("e-all", 4096)[0] == w.n_slots - 4096 and w.window("b-lists40", 4096)[0] == 9001  # xslot1 inside


@pytest.mark.parametrize("name", ["a-dst9k", "b-lists40", "c-empty", "d-free9k", "e-all"])
def test_window_set_host_classify_equals_oracle(name):
    w = sm.window_set()
    for pred in (True, False):
        got, cnt = w.e.debug_classify_host(0, w.tid[name], *w.tup[name], counters=True, pred=pred)
        assert np.array_equal(got >> 30, w.act[name]) and np.array_equal(got & 0x3FFFFFFF, w.slot[name]), pred
        assert np.array_equal(cnt, w.hist[name].astype(np.uint64)), pred
