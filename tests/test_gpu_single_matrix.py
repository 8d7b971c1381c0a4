"""SINGLE mode on the GPU: every table form through every launch stage, with and without hit
counters, vector and scalar loads, against evalACL; and the windowed hit-counter histogram.

The matrix (tables, launches and tuples: tests/single_matrix.py; all of it verified without a GPU
by tests/test_single_matrix_host.py). Forced forms at the smallest rule count with the wanted
structure, found on the CPU:

  form         table            rules  compiler knobs                        stage default / stage_max_words=0 / + stage_root_max_words=0
  cross        cross               50  -                                      1 / 2 / 0
  cross+lists  cross+lists         41  -                                      1 / 2 / 0
  pair         pair-long         3637  -                                      2 / 2 / 0
  pair         pair-weird          50  pair=2                                 1 / 2 / 0
  cand         cand-lds           155  cross_max_rules=0 pair=0               1 / 2 / 0   (the most rules whose blob fits LDS)
  cand         cand               156  cross_max_rules=0 pair=0               2 / 2 / 0   (the fewest HBM-resident)
  cand         cand-nodst-lds     211  cross_max_rules=0 pair=0               9 / 10 / 8  (dst-free, fits LDS: not yet CANDI)
  cand         cand-nodst         212  cross_max_rules=0 pair=0 candi=0       10 / 10 / 8
  candi        candi-w11          212  ... candi_window_bits=11               14 / 14 / 8 (the fewest rules that are CANDI)
  candi        candi-w0           212  ... candi_window_bits=0                14 / 14 / 8
  candi        candi-lds           16  ... candi_window_bits=0                9 / 14 / 8  (the fewest rules whose level-compressed
  candi        candi-lds-w8        16  ... candi_window_bits=8                9 / 14 / 8   rebuild, a CANDI blob, is kept in LDS)
  fd           fd                 302  -                                      4 / 5 / 8
  linear       linear           16400  pair=2 (16403 slots: windowed counters) 0 / 0 / 0
  fd           empty                0  -                                      4 / 5 / 8
  fd           catch-all            1  -                                      4 / 5 / 8

Every case: 130003 tuples (offset=1: 130002; neither a multiple of 256), half fz.rand_tuples
around the table's own prefixes, half drawn inside its rules, 2 % ANY-protocol packets.
"""
import numpy as np
import pytest
import torch

import single_matrix as sm

pytestmark = pytest.mark.gpu

from vpp_amd import device as D  # noqa: E402
from vpp_amd._capi import MODE_SINGLE  # noqa: E402

TABLES = list(sm.SPECS)


@pytest.fixture(scope="module")
def batches():
    """the tuples of a table on the device, uploaded once"""
    cache = {}

    def get(key, tup):
        if key not in cache:
            cache[key] = D.TupleBatch.from_numpy(*tup)
        return cache[key]
    return get


def launch(e, tid, b, offset, counters, reset=True):
    """one SINGLE pg_classify over tuples[offset:] -> (verdict words, counters or None)"""
    out = torch.zeros(b.n, dtype=torch.int32, device="cuda")
    if counters and reset:
        D.reset_counters(e)
    D.classify(e, MODE_SINGLE, tid, b, out, counters=D.counters_device_ptr(e) if counters else None, offset=offset)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert offset == 0 or got[0] == 0  # (nothing written in front of the batch)
    return got[offset:], (D.read_counters(e) if counters else None)


@pytest.mark.parametrize("vec", [True, False], ids=["vec", "scalar"])
@pytest.mark.parametrize("counters", [False, True], ids=["nocount", "count"])
@pytest.mark.parametrize("launch_name", list(sm.LAUNCHES))
@pytest.mark.parametrize("name", TABLES)
def test_form_stage_cell(name, launch_name, counters, vec, batches):
    t = sm.table(name)
    offset = 0 if vec else 1  # every pointer off by one element: the scalar loads
    assert t.e.table_stats(t.tid)["structure"] == t.spec.structure
    t.check_preconditions(offset)
    act, slot, hist = t.expected(offset)
    with t.e.tuning(**sm.LAUNCHES[launch_name]):
        plan = t.e.debug_launch_plan(t.tid, counters)
        assert plan["stage"] == t.spec.stages[launch_name], plan
        got, cnt = launch(t.e, t.tid, batches(name, t.tup), offset, counters)
    bad = np.nonzero(((got >> 30) != act) | ((got & 0x3FFFFFFF) != slot))[0]
    assert len(bad) == 0, (len(bad), bad[:8], got[bad[:4]], act[bad[:4]], slot[bad[:4]])
    if counters:
        assert len(cnt) == t.n_slots and np.array_equal(cnt, hist.astype(np.uint64)), np.nonzero(cnt != hist)[0][:8]


def test_every_stage_code_ran():
    """the cases above launch at the stage code pg_debug_launch_plan reports (asserted there,
    against the code written down per table): together every STAGE code launch_classify<0> can
    dispatch -- each with and without counters, with vector and scalar loads. Unreachable
    codes: none (single_matrix.UNREACHABLE)."""
    ran = set()
    for name in TABLES:
        t = sm.table(name)
        for launch_name, knobs in sm.LAUNCHES.items():
            with t.e.tuning(**knobs):
                ran.add((t.spec.structure, t.e.debug_launch_plan(t.tid)["stage"]))
    assert {st for _, st in ran} == set(sm.ALL_STAGES) - set(sm.UNREACHABLE) and not sm.UNREACHABLE
    assert {("candi", 9), ("candi", 14), ("candi", 8), ("cand", 1), ("cand", 9), ("cand", 10), ("pair", 1), ("pair", 2), ("linear", 0), ("fd", 5), ("fd", 8)} <= ran


# ---- the windowed hit counters ---------------------------------------------------------------
WNAMES = ["a-dst9k", "b-lists40", "c-empty", "d-free9k", "e-all"]


@pytest.mark.parametrize("launch_name", ["default", "nostage"])
@pytest.mark.parametrize("cells", sm.WINDOWS)
@pytest.mark.parametrize("name", WNAMES)
def test_windowed_counters_equal_oracle_histogram(name, cells, launch_name, batches):
    """A set of 18051 slots (more than the LDS histogram's 16382): a counted SINGLE launch counts
    the window [min(rule_base, n_slots - cells), + cells) and the table's default slot and last
    rule in LDS, the rest by global atomics. The whole counter array equals the oracle's
    histogram -- the slots of the other tables zero -- for a table at rule_base 0 and one at 9042,
    the clipped window of the last tables (default-deny slots inside it), tables smaller than the
    window (their last rule inside it), an empty table (last rule = default slot), dst-testing
    and dst-free forms, at 1, 64, 4096 (the default) and 16382 cells."""
    w = sm.window_set()
    w.check_preconditions(name, cells)
    tid = w.tid[name]
    with w.e.tuning(hist_window=cells, **sm.LAUNCHES[launch_name]):
        assert w.e.debug_launch_plan(tid, True)["hist_cells"] == cells
        got, cnt = launch(w.e, tid, batches("w-" + name, w.tup[name]), 0, True)
    assert np.array_equal(got >> 30, w.act[name]) and np.array_equal(got & 0x3FFFFFFF, w.slot[name])
    bad = np.nonzero(cnt != w.hist[name].astype(np.uint64))[0]
    assert len(bad) == 0, (w.window(name, cells), bad[:8], cnt[bad[:8]], w.hist[name][bad[:8]])


@pytest.mark.parametrize("name", ["a-dst9k", "d-free9k"])
def test_windowed_counters_accumulate_and_split(name, batches):
    """two counted launches without a reset between them add up, and one launch split into
    pieces of 64000 tuples (launch_max_tuples) counts what the unsplit one does"""
    w = sm.window_set()
    tid, b = w.tid[name], batches("w-" + name, w.tup[name])
    hist = w.hist[name].astype(np.uint64)
    launch(w.e, tid, b, 0, True)
    _, cnt = launch(w.e, tid, b, 0, True, reset=False)
    assert np.array_equal(cnt, 2 * hist)
    with w.e.tuning(launch_max_tuples=64 * 1000):
        got, cnt = launch(w.e, tid, b, 0, True)
    assert np.array_equal(got >> 30, w.act[name]) and np.array_equal(got & 0x3FFFFFFF, w.slot[name])
    assert np.array_equal(cnt, hist)
