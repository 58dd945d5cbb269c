"""bench.py --dump-outputs on CPU tensors: the dumped arrays are float64,
exact for every int32 / u32 value, the same seeded sample from call to call,
and bounded by DUMP_SAMPLE whatever the batch size.  CPU only (the tensors
stand in for a step's device outputs)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from cilium_amd.datapath import Verdicts  # noqa: E402


def _out(n, seed):
    g = np.random.default_rng(seed)
    v = g.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)
    i = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return v, i, Verdicts(torch.from_numpy(v), torch.from_numpy(i.view(np.int32)), None,
                          torch.from_numpy((i & 0xFF).astype(np.uint8)))


def test_small_batch_dumped_whole_and_exact(tmp_path):
    v, i, out = _out(1000, 1)
    bench.dump_outputs(str(tmp_path), None, out, out, None, counters=False)
    assert sorted(os.listdir(tmp_path)) == ["ct.npy", "ct_v6.npy", "identity.npy",
                                            "identity_v6.npy", "verdict.npy", "verdict_v6.npy"]
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["verdict"], v.astype(np.float64))
    assert np.array_equal(got["identity"], i.astype(np.float64))   # u32, not int32
    assert np.array_equal(got["ct_v6"], (i & 0xFF).astype(np.float64))


def test_large_batch_sampled_the_same_way_each_time(tmp_path):
    n = bench.DUMP_SAMPLE * 2 + 7
    v, i, out = _out(n, 2)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), None, out, None, None, counters=False)
    bench.dump_outputs(str(b), None, out, None, None, counters=False)
    va, ia = np.load(a / "verdict.npy"), np.load(a / "identity.npy")
    assert va.shape == ia.shape == (bench.DUMP_SAMPLE,)
    assert np.array_equal(va, np.load(b / "verdict.npy"))
    assert np.array_equal(ia, np.load(b / "identity.npy"))
    # the sample is of this batch, in header order, verdict and identity at
    # the same indices
    idx = np.sort(np.random.default_rng(0xD0).integers(0, n, bench.DUMP_SAMPLE))
    assert np.array_equal(va, v[idx].astype(np.float64))
    assert np.array_equal(ia, i[idx].astype(np.float64))
    # every array a run can dump, at the sample size: under 64 MB
    assert 7 * 8 * bench.DUMP_SAMPLE + 8 * (10 * bench.DUMP_RECORDS + 1) < 64 * 10**6
