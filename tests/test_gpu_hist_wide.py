"""The counter kernels at their step and alignment edges
(cilium_amd/csrc/classify.hip).

k_hist and hist_compact take one row of 16 bytes per lane and step (W = 1)
and look at the four atomics' returns once.  That is the step they had
before this file: steps of two and four rows were measured slower and are
not in the library, so the sizes around 4 W are 3, 4 and 5 and the dense and
region cases lie close to those of tests/test_gpu_key_compact.py.

k_hist_reduce is what these tests are new for.  A lane sums four adjacent
keys with 16-byte loads where a job's slab rows are 16-byte aligned and one
key where they are not; a workgroup's four waves take every fourth slice and
add one pair per key.

The batches are the smallest at which that code can go wrong
(tests/hist_wide.py; tests/test_hist_wide.py checks the shapes):
- dense streams that end on every side of a lane's 16 bytes and of a
  workgroup's step, ingress, egress and over misaligned meta;
- compact regions with counts of 0, 1, 3, 4, 5 and 64, ragged ones and one
  cut by a slice edge, also over a workspace full of stale words;
- a hot key that overflows both fields of its slot within one lane's step;
- policy tables on both sides of the reduce's alignment rule, in one, three
  and 33 slices.

Every policy counter row, identity counter, metric and verdict is compared
with the oracle, bit-exact.  Run on an MI355X: pytest -m gpu."""
import dataclasses

import numpy as np
import pytest

import hist_wide as H
import oracle as O
from cilium_amd import synth as S
from cilium_amd import metricsmap
from cilium_amd.datapath import Datapath, pack
from cilium_amd.loader import load_tables, policy_rows

pytestmark = pytest.mark.gpu

DROP_POLICY = -133
SIZES = sorted(set(H.dense_sizes()))
N_MAX = SIZES[-1]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


def offset_meta(torch, b):
    """the batch with its meta array 4 bytes past 16-byte alignment"""
    buf = torch.empty(len(b) + 8, dtype=b.meta.dtype, device=b.meta.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + len(b)]
    v.copy_(b.meta)
    assert v.data_ptr() % 16 == 4
    return dataclasses.replace(b, meta=v)


def check(torch, t, batches, mode=3, ep_lxc=0, meta_off=False, entries=None):
    """Classify the batches in turn on one Datapath (no counters_clear in
    between); verdicts, policy rows, metrics and identity counters against
    the oracle.  entries: what the policy entry count must be modulo 4."""
    dp = Datapath(0)
    try:
        pms = load_tables(dp, t)
        if entries is not None:
            assert dp.stats()["policy_entries"] % 4 == entries
        vers = []
        for h in batches:
            b = pack(h)
            out = dp.classify(offset_meta(torch, b) if meta_off else b, mode, ep_lxc)
            torch.cuda.synchronize()
            vers.append(out.verdict.cpu().numpy())
        dp.counters_sync()
        pol = {lxc: np.array(policy_rows(pm), np.uint64).reshape(-1, 7)
               for lxc, pm in pms.items()}
        met = np.array(metricsmap.dump_rows(dp), np.uint64).reshape(-1, 4)
        ide = dp.identity_counters()
    finally:
        dp.close()
    o = O.Oracle(t)
    for h, v in zip(batches, vers):
        np.testing.assert_array_equal(v, o.classify(h, mode, ep_lxc, nthreads=16)[1])
    for lxc in t.policy:
        np.testing.assert_array_equal(pol[lxc], o.policy_counters(lxc))
    np.testing.assert_array_equal(met, o.metrics())
    np.testing.assert_array_equal(ide, o.identity_counters())
    return o


@pytest.fixture(scope="module")
def small():
    """Small C2 tables, headers, and the index of one header each that bumps
    a policy entry and an identity forward counter, only an identity drop
    counter, and neither."""
    t = S.config_c2(12, n_prefixes=2000, n_policy=512)
    h = S.headers_c2(t, max(N_MAX, 20_000), seed=12)
    o = O.Oracle(t)
    ver = o.classify(h, 3, nthreads=16)[1]

    def alone(i):   # what header i bumps on its own
        o.reset_counters()
        o.classify(S.take(h, np.array([i])), 3)
        hits = sum(int(o.policy_counters(lxc)[:, 5].sum()) for lxc in t.policy)
        ide = o.identity_counters()
        return hits, int(ide[:, 2].sum()), int(ide[:, 4].sum())
    both = next(int(i) for i in np.nonzero(ver >= 0)[0][:500] if alone(i) == (1, 1, 0))
    drop = next(int(i) for i in np.nonzero(ver == DROP_POLICY)[0][:500]
                if alone(i) == (0, 0, 1))
    dead = next(int(i) for i in range(2000) if alone(i) == (0, 0, 0))
    return t, h, np.array([both, drop, dead])


def batch(small, kinds, lengths=None):
    """A batch whose header at position i is the BOTH / DROP / DEAD header
    kinds[i] names."""
    _, h, idx = small
    b = S.take(h, idx[np.asarray(kinds)])
    if lengths is not None:
        b.length = np.asarray(lengths, np.uint16)
    return b


def mixed(small, n, seed):
    rng = np.random.default_rng(seed)
    return batch(small, rng.integers(0, 3, size=n),
                 H.LENGTHS[rng.integers(0, len(H.LENGTHS), size=n)])


def trimmed(t, residue):
    """the tables with policy rows dropped until the entry count is
    `residue` modulo 4"""
    lxc = next(iter(t.policy))
    total = sum(len(p) for p in t.policy.values())
    cut = (total - residue) % 4
    t = dataclasses.replace(t, policy=dict(t.policy))
    t.policy[lxc] = t.policy[lxc][:len(t.policy[lxc]) - cut]
    assert sum(len(p) for p in t.policy.values()) % 4 == residue
    return t


# ---- dense tails
@pytest.mark.parametrize("n", SIZES)
def test_dense_tail_full(torch, small, n):
    """The dense identity stream (and the compact policy stream beside it)
    ending at n: the three headers at random, lengths from both ends of the
    len field."""
    check(torch, small[0], [mixed(small, n, n)])


@pytest.mark.parametrize("n", SIZES)
def test_dense_tail_ingress(torch, small, n):
    t, h, _ = small
    check(torch, t, [S.take(h, np.arange(n))], mode=0)


@pytest.fixture(scope="module")
def egress():
    t = S.config_c2(3, n_prefixes=2000, n_policy=512, n_endpoints=3)
    rng = np.random.default_rng(16)
    h = S.gen_headers_v4(rng, N_MAX, t.ipcache, S.local_v4_addrs(t), local_frac=0.1,
                         src_fixed=S.LXC_IPV4)
    h.length = H.LENGTHS[rng.integers(0, len(H.LENGTHS), size=N_MAX)]
    return t, h


@pytest.mark.parametrize("n", SIZES)
def test_dense_tail_egress(torch, egress, n):
    """mode 1: the second policy stream beside the first and the identity
    stream."""
    t, h = egress
    check(torch, t, [S.take(h, np.arange(n))], mode=1, ep_lxc=S.EP_LXC_ID)


@pytest.fixture(scope="module")
def unpacked():
    """More than 65 535 policy entries: bare-index policy keys, a dense job
    that reads len from the header meta."""
    t = S.config_c2(14, n_prefixes=2000, n_policy=16, n_endpoints=5)
    rng = np.random.default_rng(14)
    pol = S.gen_policy(rng, 13_200, np.unique(t.ipcache["label"]))
    t.policy = {lxc: pol for lxc in t.policy}
    assert sum(len(p) for p in t.policy.values()) > 65535
    return t, S.headers_c2(t, N_MAX, seed=14)


@pytest.mark.parametrize("meta_off", [False, True])
@pytest.mark.parametrize("n", [SIZES[-2], N_MAX])
def test_dense_meta(torch, unpacked, n, meta_off):
    """Unpacked policy keys over meta that is and is not 16-byte aligned
    (the scalar meta path), one word past a workgroup's step and two steps
    with a scalar tail."""
    t, h = unpacked
    check(torch, t, [S.take(h, np.arange(n))], mode=0, meta_off=meta_off)


# ---- compact regions
def region_batch(small):
    kinds = H.region_kinds()
    return batch(small, kinds, H.LENGTHS[np.arange(len(kinds)) % len(H.LENGTHS)])


def test_compact_regions(torch, small):
    """Region counts of 0, 1, 4W - 1, 4W, 4W + 1 and 64 (full), ragged ones,
    and a region cut by the first of three slice edges."""
    o = check(torch, small[0], [region_batch(small)])
    hits = sum(int(o.policy_counters(lxc)[:, 5].sum()) for lxc in small[0].policy)
    assert hits == np.count_nonzero(H.region_kinds() == H.BOTH)


def test_compact_regions_over_stale_words(torch, small):
    """The same after a larger batch of all-hit headers, without
    counters_clear: every word at or past a count is one of that batch's
    keys and must not be counted again."""
    full = batch(small, np.full(20_000, H.BOTH))
    o = check(torch, small[0], [full, region_batch(small), batch(small, np.full(64, H.DEAD))])
    hits = sum(int(o.policy_counters(lxc)[:, 5].sum()) for lxc in small[0].policy)
    assert hits == 20_000 + np.count_nonzero(H.region_kinds() == H.BOTH)


# ---- escapes across the wider step
def test_hot_key_interleaved(torch, small):
    """3000 headers of length 1500 on one policy key and one identity within
    one slice, three of every four positions: several adds of one lane's step
    land on the same slot; its byte field carries and its packet field
    wraps."""
    kinds = H.hot_interleaved()
    o = check(torch, small[0], [batch(small, kinds, np.full(len(kinds), 1500))])
    ide = o.identity_counters()
    assert ide[:, 2].max() == 3000 and ide[:, 3].max() == 3000 * 1500


def test_hot_key_maximal_lengths(torch, small):
    """One key, every header of length 65535: a carry every 33rd add, so
    within consecutive adds of one step."""
    n = 4096
    o = check(torch, small[0], [batch(small, np.full(n, H.BOTH), np.full(n, 65535))])
    assert o.identity_counters()[:, 3].max() == n * 65535


# ---- reduce alignment
@pytest.mark.parametrize("n", [4096, 10_000])        # one slice, three slices
@pytest.mark.parametrize("residue", [0, 1, 2, 3])    # 0: 16-byte rows; else the 4-byte path
def test_reduce_alignment(torch, small, n, residue):
    """Policy tables whose entry count is and is not a multiple of 4 (the
    identity jobs behind a misaligned policy slab start misaligned too), in
    one slice and in three: partial last groups of the reduce."""
    assert H.hist_slices(n, 1000) == (1 if n == 4096 else 3)
    t = trimmed(small[0], residue)
    check(torch, t, [S.take(small[1], np.arange(n))], entries=residue)


def test_reduce_many_slices(torch, small):
    """33 slices: a wave of the reduce takes nine rows, one more than an
    unrolled pass."""
    n = 33 * 4096 - 5
    assert H.hist_slices(n, 1000) == 33
    t, h, _ = small
    check(torch, t, [S.take(h, np.arange(n) % len(h))])
