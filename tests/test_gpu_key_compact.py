"""The compact counter-key streams between k_classify_v4 and k_hist
(cilium_amd/csrc/classify.hpp key_regions): each wave of the classify kernel
appends only its live key words to a region of its own and leaves the
region's count; k_hist reads every region up to its count and never looks at
the stale words behind it.  The library compacts the packed policy streams
(both stages); the identity stream keeps a word per header (an A/B build
compacts it too, classify.hip CFC_KEYS_COMPACT), so every k_hist launch here
mixes compact and dense jobs.  Batches built from one header that bumps a policy
entry and an identity counter, one that bumps only an identity drop counter
and one that bumps nothing, at sizes around the lane, wave, workgroup and
slice boundaries, in lane patterns that leave regions full, empty and ragged,
over a workspace an earlier, larger batch filled — every policy counter row,
identity counter, metric and verdict against the oracle, bit-exact.
Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import oracle as O
from cilium_amd import synth as S
from cilium_amd import metricsmap
from cilium_amd.datapath import Datapath, pack
from cilium_amd.loader import load_tables, policy_rows

pytestmark = pytest.mark.gpu

N_MAX = 70_000      # many workgroups, 18 histogram slices
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 17, N_MAX]
LENGTHS = np.array([0, 1, 59, 1500, 65534, 65535], np.uint16)
DROP_POLICY = -133
BOTH, DROP, DEAD = 0, 1, 2   # what a header bumps: policy entry + identity, identity, nothing


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


def gpu_counters(torch, t, batches, mode=3, ep_lxc=0):
    """Classify the batches in turn on one Datapath (no counters_clear in
    between) -> (verdicts per batch, {lxc: policy rows}, metrics, identity)."""
    dp = Datapath(0)
    try:
        pms = load_tables(dp, t)
        vers = []
        for h in batches:
            out = dp.classify(pack(h), mode, ep_lxc)
            torch.cuda.synchronize()
            vers.append(out.verdict.cpu().numpy())
        dp.counters_sync()
        pol = {lxc: np.array(policy_rows(pm), np.uint64).reshape(-1, 7)
               for lxc, pm in pms.items()}
        met = np.array(metricsmap.dump_rows(dp), np.uint64).reshape(-1, 4)
        return vers, pol, met, dp.identity_counters()
    finally:
        dp.close()


def check(torch, t, batches, mode=3, ep_lxc=0):
    vers, pol, met, ide = gpu_counters(torch, t, batches, mode, ep_lxc)
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
    """Small C2 tables, 70 000 headers, and the index of one header each that
    bumps a policy entry and an identity forward counter, only an identity
    drop counter, and neither."""
    t = S.config_c2(12, n_prefixes=2000, n_policy=512)
    h = S.headers_c2(t, N_MAX, seed=12)
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
    kinds = np.asarray(kinds)
    b = S.take(h, idx[kinds])
    if lengths is not None:
        b.length = np.asarray(lengths, np.uint16)
    return b


def mixed(small, n, seed):
    rng = np.random.default_rng(seed)
    return batch(small, rng.integers(0, 3, size=n),
                 LENGTHS[rng.integers(0, len(LENGTHS), size=n)])


@pytest.mark.parametrize("n", SIZES)
def test_sizes_random_mix(torch, small, n):
    """A lone lane, a wave boundary, a workgroup boundary, a partial last
    workgroup, many workgroups with several histogram slices; the three
    headers at random, lengths from both ends of the len field."""
    o = check(torch, small[0], [mixed(small, n, n)])
    if n >= 64:   # (the mix does bump both kinds of counter)
        ide = o.identity_counters()
        assert ide[:, 2].sum() > 0 and ide[:, 4].sum() > 0


@pytest.mark.parametrize("n", [1024, 3 * 1024 + 17, N_MAX])
def test_all_live(torch, small, n):
    """Every header live in both streams: every region exactly full."""
    o = check(torch, small[0], [batch(small, np.full(n, BOTH))])
    assert o.identity_counters()[:, 2].sum() == n
    assert sum(int(o.policy_counters(lxc)[:, 5].sum()) for lxc in small[0].policy) == n


@pytest.mark.parametrize("n", [1, 1025, N_MAX])
def test_none_live(torch, small, n):
    """Every count zero."""
    o = check(torch, small[0], [batch(small, np.full(n, DEAD))])
    assert o.identity_counters()[:, 2:].sum() == 0


def lane_pattern(name, n):
    i = np.arange(n)
    live = {"lane0": i % 64 == 0,
            "lane63": i % 64 == 63,
            "alternate": i % 2 == 0,
            "odd_waves_dead": (i // 64) % 2 == 0}[name]
    return np.where(live, BOTH, DEAD)


@pytest.mark.parametrize("name", ["lane0", "lane63", "alternate", "odd_waves_dead"])
@pytest.mark.parametrize("n", [3 * 1024 + 17, N_MAX])
def test_lane_patterns(torch, small, name, n):
    kinds = lane_pattern(name, n)
    o = check(torch, small[0], [batch(small, kinds, LENGTHS[np.arange(n) % len(LENGTHS)])])
    assert o.identity_counters()[:, 2].sum() == np.count_nonzero(kinds == BOTH)


def test_identity_stream_alone(torch, small):
    """Headers that bump only the identity drop counter among dead ones:
    every policy region empty while the identity job counts."""
    rng = np.random.default_rng(5)
    check(torch, small[0], [batch(small, np.where(rng.random(N_MAX) < 0.3, DROP, DEAD))])


def test_stale_workspace(torch, small):
    """A full workspace, then smaller batches over it with few and with no
    live words, without counters_clear: the words behind the counts (and the
    regions of workgroups the smaller launches do not have) are the first
    batch's keys and must not be counted again."""
    few = np.full(1025, DEAD)
    few[[0, 63, 64, 700, 1024]] = BOTH
    few[[1, 1023]] = DROP
    o = check(torch, small[0], [batch(small, np.full(N_MAX, BOTH)), batch(small, few),
                                batch(small, np.full(64, DEAD))])
    assert o.identity_counters()[:, 2].sum() == N_MAX + 5
    assert o.identity_counters()[:, 4].sum() == 2


@pytest.mark.parametrize("n", [3 * 1024 + 17, N_MAX])
def test_ingress(torch, small, n):
    t, h, _ = small
    check(torch, t, [S.take(h, np.arange(n))], mode=0)


@pytest.mark.parametrize("n", [1025, 20_000])
def test_egress_both_stages(torch, n):
    """mode 1: the second policy stream (the destination's policy) beside the
    first and the identity stream."""
    t = S.config_c2(3, n_prefixes=2000, n_policy=512, n_endpoints=3)
    rng = np.random.default_rng(16)
    h = S.gen_headers_v4(rng, n, t.ipcache, S.local_v4_addrs(t), local_frac=0.1,
                         src_fixed=S.LXC_IPV4)
    h.length = LENGTHS[rng.integers(0, len(LENGTHS), size=n)]
    check(torch, t, [h], mode=1, ep_lxc=S.EP_LXC_ID)


def test_unpacked_policy_keys_stay_dense(torch):
    """More than 65 535 policy entries: bare-index policy keys, one word per
    header with len from the header meta (never compact), beside the identity
    job; a smaller batch after a larger one."""
    t = S.config_c2(14, n_prefixes=2000, n_policy=16, n_endpoints=5)
    rng = np.random.default_rng(14)
    pol = S.gen_policy(rng, 13_200, np.unique(t.ipcache["label"]))
    t.policy = {lxc: pol for lxc in t.policy}
    assert sum(len(p) for p in t.policy.values()) > 65535
    h = S.headers_c2(t, 20_000, seed=14)
    check(torch, t, [h, S.take(h, np.arange(1025))], mode=0)


def test_dual_stack_one_context(torch):
    """IPv6 launches (dense key arrays) and IPv4 launches (compact) share one
    context's workspace, in both orders."""
    t = S.config_c3(3, n_prefixes=20_000, n_v4_prefixes=2000, n_policy=2000,
                    n_prefilter=2000)
    rng = np.random.default_rng(15)
    h4 = S.gen_headers_v4(rng, 20_000, t.ipcache[t.ipcache["family"] == 1],
                          S.local_v4_addrs(t), proxy_ident=S.proxy_identities(t))
    h6 = S.headers_c3(t, 20_000, seed=4)
    check(torch, t, [h6, h4, S.take(h6, np.arange(3000)), S.take(h4, np.arange(1025))])
