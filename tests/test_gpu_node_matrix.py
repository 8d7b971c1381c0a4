"""PERPOD / CONN on the GPU: every node kernel family through every launch shape, with and without
hit counters, vector and scalar loads, against the oracle's verdicts and counter histogram.

The matrix (sets, launch shapes, tuples: tests/node_matrix.py; all of it verified without a GPU
by tests/test_node_matrix_host.py). Every case asserts the plan pg_debug_node_launch_plan reports
-- path, k_classify STAGE code, staged words, whether the dst records stay in the image, the
counting scheme and its cells -- before it launches. The sets, at the smallest size with the wanted
structure (found on the CPU), and their STAGE codes uncounted / counted:

  set                  tables rules slots  family  stage3-all  stage3-norec  stage1-recs  stage1-base  stage0
  uni                      12    78    92  uniform  99 / 115       -            -          97 / 113   96 / 112
  uni-nocommon             12    78    92  uniform      -          -            -          97 / 113   96 / 112
  uni-grouped              65   177   244  uniform  99 / 115       -            -          97 / 113   96 / 112
  uni-wide                253   681   936  wide    227 / 243       -            -         225 / 241  224 / 240
  uni-mid                   8 10262 10272  uniform  99 / 115       -            -          97 / 113   96 / 112
  wide-mid                253 10261 10516  wide    227 / 243       -            -         225 / 241  224 / 240
  nopair, nopair-rec       12    78    92  nopair   35 / 51     35 / 51         -          33 / 49    32 / 48
  nopair-rec-cross         12    78    92  nopair   35 / 51        -            -          33 / 49    32 / 48
  nopair-rec-nocommon      12    78    92  nopair       -          -         33 / 49       33 / 49    32 / 48
  uncovered                 8   158   168  nopair   35 / 51     35 / 51         -          33 / 49    32 / 48
  pair                     13   184   199  generic   3 / 19        -            -           1 / 17     0 / 16
  big-uni                   8 20502 20512  uniform  99 / 99        -            -          97 / 97    96 / 96
  big-nopair                8 20502 20512  nopair   35 / 35     35 / 35         -          33 / 33    32 / 32
  big-pair                  8 20502 20512  generic   3 / 3         -            -           1 / 1      0 / 0
  big-wide                253 16813 17068  wide    227 / 227       -            -         225 / 225  224 / 224

Counted launches of the uniform sets also at 16-bit cells: half16-s1 369 (wide 497), half16-s0 368
(496), and on uni-mid and wide-mid -- the sets whose section is smaller than what the narrower cells
save -- half16-s3 371 (499). The big sets (counted: the slot cache, no + 16) also at
node_hist_cells 8192, 256, 16 (cache), 15 and 0 (global atomics only; these at stages 3, 1 and 0)
and on the per-table path (node_path=0, code 0) with hist_window 1, 64, 4096 and 16382; every other
set once on the per-table path; uni and pair at block_stage 256, 512 and 1024. Combinations
launch_classify<1|2> cannot dispatch: node_matrix.unreachable.

Every batch: 60003 tuples (offset=1: 60002; neither a multiple of 1024), 60 % pod end points
(local, remote, a pod without an interface), 2 % ANY-protocol, 40 % drawn inside the sets' rules.
"""
import numpy as np
import pytest
import torch

import node_matrix as nm

pytestmark = pytest.mark.gpu

from vpp_amd import device as D  # noqa: E402
from vpp_amd._capi import MODE_CONN, MODE_PERPOD  # noqa: E402

SENTINEL = 0x5EEDF00D
CELLS = [(name, launch, counters) for name in nm.SETS for counters in (False, True)
         for launch in nm.launch_names(name, counters)]


@pytest.fixture(scope="module")
def batches():
    """the tuples of a topology on the device, uploaded once"""
    cache = {}

    def get(key, tup, sport=True):
        if key not in cache:
            cache[key] = D.TupleBatch.from_numpy(*tup)
            if not sport:
                cache[key].sport = None
        return cache[key]
    return get


def launch(e, mode, b, offset=0, counters=False, n=None, reset=True):
    """one pg_classify over tuples[offset:offset + n] -> (verdict words, counters or None); nothing
    may be written in front of the batch or past it"""
    n = b.n - offset if n is None else n
    out = torch.full((b.n,), SENTINEL, dtype=torch.int32, device="cuda")
    if counters and reset:
        D.reset_counters(e)
    D.classify(e, mode, -1, b, out, counters=D.counters_device_ptr(e) if counters else None, offset=offset, n=n)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[:offset] == SENTINEL).all() and (got[offset + n:] == SENTINEL).all(), "written outside the batch"
    return got[offset:offset + n], (D.read_counters(e) if counters else None)


def compare(got, cnt, exp, what):
    act, slot, hist = exp
    bad = nm.mismatches(got, act, slot)
    assert len(bad) == 0, (what, len(bad), bad[:8], got[bad[:4]], act[bad[:4]], slot[bad[:4]])
    if cnt is not None:
        bad = np.nonzero(cnt != hist)[0]  # the whole array: slots not hit must be zero
        assert len(cnt) == len(hist) and len(bad) == 0, (what, len(bad), bad[:8], cnt[bad[:8]], hist[bad[:8]])


@pytest.mark.parametrize("vec", [True, False], ids=["vec", "scalar"])
@pytest.mark.parametrize("mode", nm.MODES, ids=["perpod", "conn"])
@pytest.mark.parametrize("name,launch_name,counters", CELLS,
                         ids=["%s-%s-%s" % (n, ln, "count" if c else "nocount") for n, ln, c in CELLS])
def test_family_stage_cell(name, launch_name, counters, mode, vec, batches):
    s = nm.node_set(name)
    offset = 0 if vec else 1  # every pointer off by one element: the scalar loads
    knobs, want = s.launches(counters)[launch_name]
    with s.e.tuning(**knobs):
        s.check_plan(mode, counters, want)
        got, cnt = launch(s.e, mode, batches(s.spec.topology, s.tup), offset, counters)
    compare(got, cnt, s.expected(mode, offset), (name, launch_name, mode, counters, vec))


@pytest.mark.parametrize("counters", [False, True], ids=["nocount", "count"])
@pytest.mark.parametrize("name", list(nm.SETS))
def test_perpod_without_source_ports(name, counters, batches):
    """PERPOD reads no source port: a batch without the array classifies the same"""
    s = nm.node_set(name)
    b = batches(s.spec.topology + "-nosport", s.tup, sport=False)
    assert b.sport is None
    got, cnt = launch(s.e, MODE_PERPOD, b, 0, counters)
    compare(got, cnt, s.expected(MODE_PERPOD), (name, counters))


@pytest.mark.parametrize("mode", nm.MODES, ids=["perpod", "conn"])
@pytest.mark.parametrize("name", ["uni", "big-uni"])
def test_node_counters_accumulate_and_split(name, mode, batches):
    """two counted launches without a reset between them add up, and one launch split into pieces
    of 6400 tuples (launch_max_tuples; CONN's deferred pass then runs once per piece) gives the
    verdicts and counters of the unsplit one"""
    s = nm.node_set(name)
    b = batches(s.spec.topology, s.tup)
    act, slot, hist = s.expected(mode)
    assert s.e.debug_node_launch_plan(mode, True)["defers_any"] == (mode == MODE_CONN)
    launch(s.e, mode, b, 0, True)
    got, cnt = launch(s.e, mode, b, 0, True, reset=False)
    compare(got, cnt, (act, slot, 2 * hist), (name, mode, "twice"))
    with s.e.tuning(launch_max_tuples=64 * 100):
        for counters in (True, False):
            got, cnt = launch(s.e, mode, b, 0, counters)
            compare(got, cnt, (act, slot, hist), (name, mode, "split", counters))


@pytest.mark.parametrize("mode", nm.MODES, ids=["perpod", "conn"])
@pytest.mark.parametrize("n", nm.RAGGED_SIZES)
@pytest.mark.parametrize("name", nm.RAGGED_SETS)
def test_node_ragged_sizes(name, n, mode, batches):
    """prefixes of a batch whose first tuple is an ANY-protocol packet between two local pods (CONN
    over the uniform set: deferred, so n = 1 is a k_node_any pass over one tuple), counted and
    uncounted; nothing is written past n"""
    r = nm.ragged(name)
    b = batches("ragged-" + name, r.tup)
    for counters in (False, True):
        got, cnt = launch(r.s.e, mode, b, 0, counters, n=n)
        compare(got, cnt, r.expected(mode, n), (name, n, mode, counters))
