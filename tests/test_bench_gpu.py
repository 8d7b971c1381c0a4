"""bench.py on the GPU as the child process a driver starts. A plain run (--gpus 1 --steps K
--warmup W) sets up, warms up, times its K steps, writes the last step's verdicts when asked to
and prints the line; --full goes on to the legs reported beside `value` (steady state, stream
ceiling, oracle self-check, CPU baseline, side configs). Both dump the same verdicts: the inputs
are a function of the arguments alone and the later legs do not touch the timed run's output.

Small batch: just above bench.DUMP_MAX, so the dump takes its sampling path (2M + 4097 tuples,
an odd count, several hundred blocks)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from oracle import world as OW
from vpp_amd import device as D
from vpp_amd import workloads as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = bench.DUMP_MAX + 4097
FULL_ONLY = ("steady_state", "parity_sample", "parity_per_rank", "cpu_baseline", "side_config1")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    return _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--tuples", str(N), "--dump-outputs", str(d)), d


@pytest.fixture(scope="module")
def full(tmp_path_factory):
    d = tmp_path_factory.mktemp("full")
    return _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--tuples", str(N), "--dump-outputs", str(d),
                  "--full", "--side", "1", "--check-tuples", "65536", "--cpu-sample", "65536",
                  "--cpu-seconds", "0.2", "--faithful-seconds", "0.1"), d


def _headline(d):
    assert d["metric"] == bench.METRIC and d["unit"] == "Mpps" and d["higher_is_better"] is True
    assert d["dtype"] == "u32" and d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["config"]["tuples_per_gpu"] == N and d["ms_per_step"] > 0
    # value = N tuples per step / ms_per_step; the line rounds ms_per_step to 1e-4 ms and value to
    # 0.1 Mpps: at most 1 % apart for a step of 5 us or more, plus the value's own rounding
    assert d["ms_per_step"] >= 0.005
    assert abs(d["value"] - N / d["ms_per_step"] / 1e3) <= 0.01 * d["value"] + 0.1


def test_plain_run_stops_after_the_timed_steps(plain):
    d, _ = plain
    _headline(d)
    assert not [k for k in FULL_ONLY if k in d]
    assert "measured_stream_gbps" not in d["roofline"] and d["roofline"]["kernel_ms"] > 0


def test_plain_run_dumps_the_last_steps_verdicts(plain):
    """the dumped sample == a classify pass of the same workload in this process, which the
    oracle confirms bit for bit at the sampled tuples"""
    _, path = plain
    idx = np.load(path / "verdict_index.npy")
    v = np.load(path / "verdicts.npy")
    assert v.dtype == idx.dtype == np.float64 and len(v) == len(idx) == bench.DUMP_MAX
    assert sorted(os.listdir(path)) == ["verdict_index.npy", "verdicts.npy"]  # config 2 does not count
    idx = idx.astype(np.int64)
    w = W.config2(0, n_tuples=N)
    e = w.engine
    b = D.TupleBatch(N, with_sport=False)
    D.gen_tuples(e, b, **w.gen)
    out = torch.empty(N, dtype=torch.int32, device="cuda")
    D.classify(e, w.mode, w.table_id, b, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)[idx]
    assert np.array_equal(v, got.astype(np.float64))
    k = 1 << 16  # of the sample, spread over the whole batch
    sel = idx[:: len(idx) // k][:k]
    tup = [x[sel] for x in b.numpy(N)]
    act, slot, _ = OW.expected(e, w.mode, w.table_id, w.local_ifs, w.node_if, *tup, threads=16)
    g = v[:: len(idx) // k][:k].astype(np.uint32)
    assert np.array_equal(g >> 30, act.astype(np.uint32)) and np.array_equal(g & 0x3FFFFFFF, slot)
    assert len(set((g >> 30).tolist())) >= 2


def test_full_run_adds_the_side_legs_and_dumps_the_same(plain, full):
    d, path = full
    _headline(d)
    assert not [k for k in FULL_ONLY if k not in d]
    assert d["parity_sample"]["bit_exact_action_and_rule_index"] is True
    assert d["parity_sample"]["counters_equal_oracle_histogram"] is True
    assert d["cpu_baseline"]["sample_bit_exact_vs_gpu"] is True
    assert d["steady_state"]["kernel_ms"] > 0 and d["roofline"]["measured_stream_gbps"]["probe"] > 0
    assert d["side_config1"]["parity_sample"]["bit_exact_action_and_rule_index"] is True
    for f in ("verdict_index.npy", "verdicts.npy"):
        assert np.array_equal(np.load(path / f), np.load(plain[1] / f))
