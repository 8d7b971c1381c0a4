"""Rule edges on the GPU: every kernel on tuples placed one step below, on the first, on the last and
one step above every prefix and port range of its rules, against the oracle bit for bit (verdict
word = action << 30 | slot, and the hit counters).

The batches, edge tables and preconditions: tests/edge_cases.py, all of it verified without a GPU
by tests/test_edge_host.py (decisive pairs, 100 % edge-cell coverage, sensitivity).

  SINGLE   every table of single_matrix.SPECS, fd_pipeline_cases' split table, the five WindowSet
           tables and the 17 edge tables (ladder-src / -dst / -both, extremes, each under the
           matrix's knob sets) x single_matrix.LAUNCHES x counters x vector / scalar loads, the stage
           code asserted; the FD-in-LDS launch variants of test_gpu_fd_pipeline over fd, split and
           ladder-src
  PERPOD / CONN   every set of node_matrix.SETS x mode x counters at the default launch, stage0 and
           the per-table path
  reach    pg_reach_matrix (packed and full words), pg_reach_ports (TCP, UDP) and pg_reach_rules (evals
           and cells) over sides and services of edge addresses and ports, for reach_cases' form A and
           form B sets
"""
import numpy as np
import pytest
import torch

import edge_cases as ec
import node_matrix as nm
import ports_cases as pc
import reach_cases as rc
import rules_cases as kr
import single_matrix as sm
import test_gpu_fd_pipeline as fp

pytestmark = pytest.mark.gpu

from vpp_amd import device as D  # noqa: E402
from vpp_amd._capi import MODE_SINGLE  # noqa: E402

SENTINEL = 0x5EEDF00D
REACH_SETS = rc.FORM_A_SETS + rc.FORM_B_SETS


@pytest.fixture(scope="module")
def batches():
    """an edge batch on the device, uploaded once"""
    cache = {}

    def get(key, tup):
        if key not in cache:
            cache[key] = D.TupleBatch.from_numpy(*tup)
        return cache[key]
    return get


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def launch(e, mode, tid, b, offset, counters):
    """one pg_classify over tuples[offset:] -> (verdict words, counters or None); nothing may be
    written in front of the batch"""
    out = torch.full((b.n,), SENTINEL, dtype=torch.int32, device="cuda")
    if counters:
        D.reset_counters(e)
    D.classify(e, mode, tid, b, out, counters=D.counters_device_ptr(e) if counters else None, offset=offset)
    torch.cuda.synchronize()
    got = u32(out)
    assert (got[:offset] == SENTINEL).all(), "written in front of the batch"
    return got[offset:], (D.read_counters(e) if counters else None)


def compare(got, cnt, exp, rec, what):
    act, slot, hist = exp
    bad = nm.mismatches(got, act, slot)
    assert len(bad) == 0, (what, len(bad), bad[:8], rec[bad[:4]], got[bad[:4]], act[bad[:4]], slot[bad[:4]])
    if cnt is not None:
        bad = np.nonzero(cnt != hist)[0]   # the whole array: slots not hit must be zero
        assert len(cnt) == len(hist) and len(bad) == 0, (what, len(bad), bad[:8], cnt[bad[:8]], hist[bad[:8]])


# ---- SINGLE -------------------------------------------------------------------------------------
@pytest.mark.parametrize("vec", [True, False], ids=["vec", "scalar"])
@pytest.mark.parametrize("counters", [False, True], ids=["nocount", "count"])
@pytest.mark.parametrize("launch_name", list(sm.LAUNCHES))
@pytest.mark.parametrize("name", ec.SINGLE_TABLES)
def test_single_edges(name, launch_name, counters, vec, batches):
    t = ec.table(name)
    offset = 0 if vec else 1   # every pointer off by one element: the scalar loads
    assert t.e.table_stats(t.tid)["structure"] == t.structure
    act, slot, hist = t.expected(offset)
    with t.e.tuning(**sm.LAUNCHES[launch_name]):
        plan = t.e.debug_launch_plan(t.tid, counters)
        assert plan["stage"] == t.stages[launch_name], plan
        got, cnt = launch(t.e, MODE_SINGLE, t.tid, batches(name, t.tup), offset, counters)
    compare(got, cnt, (act, slot, hist.astype(np.uint64)), t.rec[offset:], (name, launch_name, counters, vec))


def test_every_stage_code_ran_on_an_edge_batch():
    """the cases above launch at the stage code pg_debug_launch_plan reports (asserted there against
    the code written down per table): together every STAGE code launch_classify<0> can dispatch"""
    ran = set()
    for name in ec.SINGLE_TABLES:
        t = ec.table(name)
        for knobs in sm.LAUNCHES.values():
            with t.e.tuning(**knobs):
                ran.add(t.e.debug_launch_plan(t.tid)["stage"])
    assert ran == set(sm.ALL_STAGES)


@pytest.mark.parametrize("variant", list(fp.VARIANTS))
@pytest.mark.parametrize("name", ec.FD_TABLES)
def test_fd_in_lds_variants_on_edges(name, variant):
    """test_gpu_fd_pipeline's sizes and launch variants with the edge batch tiled over them"""
    fp.run_case(ec.FdCase(name), **fp.VARIANTS[variant])


# ---- PERPOD / CONN ------------------------------------------------------------------------------
@pytest.mark.parametrize("launch_name", ec.NODE_LAUNCHES)
@pytest.mark.parametrize("counters", [False, True], ids=["nocount", "count"])
@pytest.mark.parametrize("mode", nm.MODES, ids=["perpod", "conn"])
@pytest.mark.parametrize("name", list(nm.SETS))
def test_node_edges(name, mode, counters, launch_name, batches):
    s = nm.node_set(name)
    n = ec.node_edges(s.spec.topology)
    knobs, want = ec.node_launch(s, launch_name, counters)
    with s.e.tuning(**knobs):
        if want is not None:
            s.check_plan(mode, counters, want)
        got, cnt = launch(s.e, mode, -1, batches("node-" + s.spec.topology, n.tup), 0, counters)
    compare(got, cnt, n.expected(mode), n.rec, (name, mode, counters, launch_name))


# ---- reachability matrix and port sweep ---------------------------------------------------------
@pytest.mark.parametrize("name", REACH_SETS)
def test_reach_matrix_edges(name):
    s = nm.node_set(name)
    r = ec.reach_edges(s.spec.topology)
    r.check_preconditions()
    packed, words = D.reach_matrix(s.e, r.src, r.dst, r.svc, words=True)
    torch.cuda.synchronize()
    assert (u32(words) == r.words).all(), rc.mismatch_report(u32(words), r.words)
    assert (u32(packed) == rc.pack(r.words)).all(), "packed output differs from the words' top two bits"
    only = D.reach_matrix(s.e, r.src, r.dst, r.svc)   # without out_words: the same packed words
    torch.cuda.synchronize()
    assert (u32(only) == u32(packed)).all()


@pytest.mark.parametrize("protocol", (pc.TCP, pc.UDP), ids=("tcp", "udp"))
@pytest.mark.parametrize("name", REACH_SETS)
def test_reach_ports_edges(name, protocol):
    s = nm.node_set(name)
    r = ec.reach_edges(s.spec.topology)
    lo, hi, first, last = r.sweep(protocol)
    assert (first == last).all()
    out = D.reach_ports(s.e, r.src, r.dst, protocol, pc.SPORT, open_count=True, words=True)
    torch.cuda.synchronize()
    got_lo, codes, n_open, words = (out[0],) + tuple(u32(x) for x in out[1:])
    assert np.array_equal(got_lo, lo)
    assert (words == first).all(), pc.mismatch_report(words, first)
    assert (codes == pc.pack(first >> 30)).all(), "codes differ from the words' top two bits"
    assert (n_open == (((first >> 30) == pc.ALLOW) * pc.lengths(lo)).sum(axis=2)).all()


@pytest.mark.parametrize("name", REACH_SETS)
def test_reach_rules_edges(name):
    """rule coverage of the edge product against the oracle and, byte for byte, the host twin"""
    import test_gpu_rules as gr
    s = nm.node_set(name)
    r = ec.reach_edges(s.spec.topology)
    wev, wce = ec.reach_edge_hists(s.spec.topology)
    for evals, cells in ((True, True), (True, False), (False, True)):
        got = gr.run_dev(s.e, r.src, r.dst, r.svc, evals=evals, cells=cells)
        kr.same(got, wev, wce, (name, evals, cells))
        gr.identical(got, kr.run_host(s.e, r.src, r.dst, r.svc, evals=evals, cells=cells), (name, evals, cells))
        assert got[2] == kr.want_result(s.e, r.src, r.dst, np.ones(len(r.svc)), wev, evals=evals)
