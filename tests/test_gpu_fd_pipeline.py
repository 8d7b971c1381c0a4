"""The FD-in-LDS launch (k_classify STAGE 4) on the GPU at the sizes where its group loop can go
wrong, against evalACL bit for bit in action and slot.

The launch stages the blob, loads a group of four tuples per lane ahead of the group it walks,
and strides the resident grid over the batch. With W = one workgroup's group (block x 4 tuples)
and S = one sweep of the resident grid (resident workgroups x W), both from the geometry the
library reports for the launch (pg_debug_last_launch), a case launches n =
    0, 1, 3, 4, 5           no group, a remainder only, one group and a remainder
    W - 1, W, W + 1         one workgroup's lanes all but full, full, and one tuple over
    S - 1, S, S + 1         one sweep: every lane's first group and no second one, ...
    S + W + 3, 2 S + 5      a second and a third group on some lanes only, with a remainder
over a verdict array filled with a sentinel: nothing past n and nothing before the batch may be
written. Tables and ANY-protocol placements: tests/fd_pipeline_cases.py (all of it verified
without a GPU by tests/test_fd_group_host.py); the oracle's verdicts are computed once per table
and placement and tiled to the longest batch.

Variants (each over every table, 2 % ANY-protocol packets at random): every pointer off by one
element (the scalar loop), blocks_per_cu 1 and 3, 1024-thread workgroups, and hit counters equal
to the oracle's slot histogram. The other placements run under the default launch.
"""
import numpy as np
import pytest
import torch

import fd_pipeline_cases as fc

pytestmark = pytest.mark.gpu

from vpp_amd import device as D  # noqa: E402
from vpp_amd._capi import MODE_SINGLE  # noqa: E402

SENTINEL = 0x7FFFFFFF  # no verdict word: its slot is past every table set's
VARIANTS = {
    "default": dict(),
    "offset1": dict(offset=1),
    "bpc1": dict(tune={"blocks_per_cu": 1}),
    "bpc3": dict(tune={"blocks_per_cu": 3}),
    "bs1024": dict(tune={"block_stage": 1024}),
    "counters": dict(counters=True),
}


def sizes(w, s):
    return [0, 1, 3, 4, 5, w - 1, w, w + 1, s - 1, s, s + 1, s + w + 3, 2 * s + 5]


def run_case(c, offset=0, counters=False, tune=None):
    e, tid = c.e, c.tid
    with e.tuning(**(tune or {})):
        assert e.debug_launch_plan(tid, counters)["stage"] == 4
        # the launch geometry under these knobs (and with counters, whose kernel has an occupancy
        # of its own), from a first launch of a few tuples
        cptr = D.counters_device_ptr(e) if counters else None
        probe = D.TupleBatch.from_numpy(*[x[:8 + offset] for x in c.tup])
        D.classify(e, MODE_SINGLE, tid, probe, torch.empty(8 + offset, dtype=torch.int32, device="cuda"), counters=cptr,
                   offset=offset)
        g = D.last_launch()
        # (512 threads, or 1024 where blob + histogram leave LDS for fewer than three workgroups per CU)
        assert g["block"] in ((1024,) if (tune or {}).get("block_stage") == 1024 else (512, 1024)), g
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        per_cu = g["resident"] // cus  # (as many as LDS holds, capped by blocks_per_cu)
        assert g["resident"] == per_cu * cus and 1 <= per_cu <= (tune or {}).get("blocks_per_cu", per_cu), g
        w = g["block"] * 4
        s = g["resident"] * w
        ns = sizes(w, s)
        total = offset + max(ns)
        b = D.TupleBatch.from_numpy(*[np.resize(x, total) for x in c.tup])
        want_np = np.resize(c.words(), total)
        slot_np = np.resize(c.slot, total)
        want = torch.from_numpy(want_np.view(np.int32)).cuda()
        pad = 64
        for n in ns:
            out = torch.full((total + pad,), SENTINEL, dtype=torch.int32, device="cuda")
            if counters:
                D.reset_counters(e)
            D.classify(e, MODE_SINGLE, tid, b, out, counters=cptr, offset=offset, n=n)
            torch.cuda.synchronize()
            if n:  # one lane per group of four (unaligned pointers: per tuple), the grid capped at the resident one
                items = -(-n // 4) if offset == 0 else n
                assert D.last_launch()["grid"] == min(g["resident"], -(-items // g["block"])), (n, D.last_launch())
            assert bool((out[:offset] == SENTINEL).all()), (n, "written before the batch")
            assert bool((out[offset + n:] == SENTINEL).all()), (n, "written past n")
            if not torch.equal(out[offset:offset + n], want[offset:offset + n]):
                got = out[offset:offset + n].cpu().numpy().view(np.uint32)
                bad = np.nonzero(got != want_np[offset:offset + n])[0]
                raise AssertionError((n, len(bad), bad[:8], got[bad[:4]], want_np[offset:offset + n][bad[:4]]))
            if counters:
                cnt = D.read_counters(e)
                hist = np.bincount(slot_np[offset:offset + n], minlength=c.n_slots).astype(np.uint64)
                assert np.array_equal(cnt, hist), (n, np.nonzero(cnt != hist)[0][:8])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", fc.TABLES)
def test_sizes_under_every_launch(name, variant):
    run_case(fc.case(name, "rand2"), **VARIANTS[variant])


@pytest.mark.parametrize("placement", [p for p in fc.PLACEMENTS if p != "rand2"])
@pytest.mark.parametrize("name", fc.TABLES)
def test_any_protocol_placements(name, placement):
    run_case(fc.case(name, placement))
