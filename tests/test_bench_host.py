"""bench.py's CPU-baseline leg without a GPU: its samples must compare bit-exact with the
product's verdicts, so the baseline times the same calls the product answers. Here the
"GPU" verdicts are the oracle's own (World: the product's semantics, pinned elsewhere against
the reference's KATs), fed through bench.cpu_baseline with small sample budgets."""
import numpy as np
import torch

import bench
from oracle import gen as G
from oracle.world import World
from vpp_amd import workloads as W


class _Batch:
    """the slice of device.TupleBatch that cpu_baseline reads"""

    def __init__(self, tup):
        self.tup, self.n = tup, len(tup[0])

    def numpy(self, k):
        return tuple(x[:k] for x in self.tup)


def _run(w, n):
    tup = G.gen_tuples(n, **w.gen)[:5]
    wd = World(w.engine, w.local_ifs, w.node_if)
    if w.mode == 2:
        act, slot = wd.conn(*tup, threads=4)
    else:
        act, slot = wd.perpod(tup[0], tup[1], tup[3], tup[4], threads=4)
    verdicts = (act.astype(np.uint32) << 30) | slot.astype(np.uint32)
    out = torch.from_numpy(verdicts.view(np.int32).copy())
    return bench.cpu_baseline(w, _Batch(tup), out, n, faithful_s=0.2, budget_s=0.4)


def test_plain_run_is_the_default(monkeypatch):
    """--full is off unless asked for; --dump-outputs takes a directory"""
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(tmp_path):
    """--dump-outputs: a batch up to DUMP_MAX is written whole, a larger one as the same sorted
    sample on every call; float64 holds the u32 verdict word (action bits 30-31 set included) and
    the i64 counters exactly; ranks of a multi-GPU run write their own files."""
    rng = np.random.default_rng(7)
    small = rng.integers(0, 1 << 32, 1001, dtype=np.uint64).astype(np.uint32)
    cnt = torch.arange(5, dtype=torch.int64) << 40
    bench.dump_outputs(str(tmp_path / "a"), torch.from_numpy(small.view(np.int32)), cnt, 0, 1)
    v = np.load(tmp_path / "a" / "verdicts.npy")
    assert v.dtype == np.float64 and np.array_equal(v, small.astype(np.float64)) and v.max() >= 2.0 ** 31
    assert np.array_equal(np.load(tmp_path / "a" / "counters.npy"), cnt.numpy().astype(np.float64))
    assert not (tmp_path / "a" / "verdict_index.npy").exists()

    n = bench.DUMP_MAX + 4097
    big = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    out = torch.from_numpy(big.view(np.int32))
    bench.dump_outputs(str(tmp_path / "b"), out, None, 0, 1)
    bench.dump_outputs(str(tmp_path / "c"), out, None, 1, 2)
    idx = np.load(tmp_path / "b" / "verdict_index.npy")
    v = np.load(tmp_path / "b" / "verdicts.npy")
    assert idx.dtype == np.float64 and len(idx) == len(v) == bench.DUMP_MAX
    assert (np.diff(idx) >= 0).all() and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(v, big[idx.astype(np.int64)].astype(np.float64))
    assert not (tmp_path / "b" / "counters.npy").exists()
    assert np.array_equal(np.load(tmp_path / "c" / "verdict_index_rank1.npy"), idx)
    assert np.array_equal(np.load(tmp_path / "c" / "verdicts_rank1.npy"), v)
    assert v.nbytes + idx.nbytes <= 64 << 20


def test_conn_baseline_uses_the_connection_endpoint_rules():
    """CONN (config 5's topology): remote pod <-> non-pod and non-pod <-> non-pod make no
    evaluation (aclengine_mock.go:343-347, 388-392) in the baseline too -- its sample and its
    reference-faithful sample equal the product's verdicts."""
    w = W.config5(0, n_tuples=1 << 14)
    r = _run(w, 1 << 14)
    assert r["sample_bit_exact_vs_gpu"] is True
    assert r["faithful_variant_bit_exact"] is True
    assert r["faithful_nthreads_bit_exact"] is True and r["faithful_nthreads_cores"] == bench.host_cores()


def test_perpod_baseline_bit_exact():
    """PERPOD (config 3): the pre-parsed and the reference-faithful samples, at one thread and at
    every core, equal the product's verdicts."""
    w = W.config3(0, n_tuples=1 << 14)
    r = _run(w, 1 << 14)
    assert r["sample_bit_exact_vs_gpu"] is True
    assert r["faithful_variant_bit_exact"] is True
    assert r["faithful_nthreads_bit_exact"] is True and r["faithful_nthreads_cores"] == bench.host_cores()
