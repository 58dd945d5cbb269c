"""The counter histogram's 32-bit LDS slots (csrc/classify.hip k_hist,
classify.hpp HistSlot): batches that overflow a slot's packet and byte
fields, the identity range boundaries that follow from the slot width, the
unpacked policy keys, IPv6 and the egress stage — every policy counter row,
every identity counter and the metrics against the oracle, bit-exact.
Run on an MI355X: pytest -m gpu."""
import os
import re

import numpy as np
import pytest

import oracle as O
from cilium_amd import synth as S
from cilium_amd import metricsmap
from cilium_amd.datapath import Datapath, pack
from cilium_amd.loader import load_tables, policy_rows

pytestmark = pytest.mark.gpu

N_HOT = 70_000      # 18 histogram slices of ~3.9 k headers
LENGTHS = np.array([0, 1, 59, 1500, 65534, 65535], np.uint16)
DROP_POLICY = -133


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


def _constants():
    """HIST_RANGE, ID_RANGE, ID_PACK_LIMIT as the library is built with."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "cilium_amd", "csrc", "classify.hpp")).read()
    hist = int(re.search(r"constexpr uint32_t HIST_RANGE = (\d+);", src).group(1))
    assert re.search(r"constexpr uint32_t ID_RANGE = HIST_RANGE / 2;", src)
    limit = int(re.search(r"constexpr uint32_t ID_PACK_LIMIT = (\d+);", src).group(1))
    return hist, hist // 2, limit


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
    """Small C2 tables, 70 000 headers, and the index of one header that a
    policy entry forwards and of one that the policy drops (no entry)."""
    t = S.config_c2(12, n_prefixes=2000, n_policy=512)
    h = S.headers_c2(t, N_HOT, seed=12)
    o = O.Oracle(t)
    ver = o.classify(h, 3, nthreads=16)[1]

    def alone(i):   # what header i bumps on its own
        o.reset_counters()
        o.classify(S.take(h, np.array([i])), 3)
        hits = sum(int(o.policy_counters(lxc)[:, 5].sum()) for lxc in t.policy)
        ide = o.identity_counters()
        return hits, int(ide[:, 2].sum()), int(ide[:, 4].sum())
    fwd = next(int(i) for i in np.nonzero(ver >= 0)[0][:500] if alone(i) == (1, 1, 0))
    drop = next(int(i) for i in np.nonzero(ver == DROP_POLICY)[0][:500]
                if alone(i) == (0, 0, 1))
    return t, h, {"forward": fwd, "drop": drop}


def hot_batch(h, i):
    b = S.take(h, np.full(N_HOT, i))
    b.length = np.full(N_HOT, 65535, np.uint16)
    return b


@pytest.mark.parametrize("which", ["forward", "drop"])
def test_hot_key_maximal_lengths(torch, small, which):
    """One key takes every header of every slice at len 65535: > 2047
    packets and ~255 MB per slice, so the packet field wraps and the byte
    field carries every 33rd header."""
    t, h, idx = small
    o = check(torch, t, [hot_batch(h, idx[which])])
    ide = o.identity_counters()
    col = 2 if which == "forward" else 4
    assert ide[:, col].max() == N_HOT and ide[:, col + 1].max() == N_HOT * 65535
    hits = max(int(o.policy_counters(lxc)[:, 5].max()) for lxc in t.policy)
    assert hits == (N_HOT if which == "forward" else 0)


def test_mixed_lengths(torch, small):
    """Half the headers as generated (many keys), half on the hot key,
    lengths from both ends of the byte field."""
    t, h, idx = small
    rng = np.random.default_rng(7)
    hot = rng.random(N_HOT) < 0.5
    b = S.take(h, np.where(hot, idx["forward"], np.arange(N_HOT)))
    b.length = LENGTHS[rng.integers(0, len(LENGTHS), size=N_HOT)]
    check(torch, t, [b])


def test_two_batches_accumulate(torch, small):
    """The hot batch twice without counters_clear: exactly double (the
    escapes' negative packet deltas land in counters that already count)."""
    t, h, idx = small
    b = hot_batch(h, idx["forward"])
    o = check(torch, t, [b, b])
    o1 = O.Oracle(t)
    o1.classify(b, 3, nthreads=16)
    for lxc in t.policy:
        once = o1.policy_counters(lxc)
        once[:, 5:] *= 2
        np.testing.assert_array_equal(o.policy_counters(lxc), once)
    once = o1.identity_counters()
    once[:, 2:] *= 2
    np.testing.assert_array_equal(o.identity_counters(), once)


def test_identity_range_boundaries(torch):
    """Identities on both sides of the first range's end, the last one a
    packed key can carry, and one past it (counted directly)."""
    hist_range, id_range, pack_limit = _constants()
    special = [id_range - 1, id_range, pack_limit - 1, pack_limit + 7]
    rng = np.random.default_rng(13)
    ipc = S.gen_ipcache_v4(rng, 2000, label_mod=64)
    for k, ident in enumerate(special):
        ipc["label"][40 * k:40 * (k + 1)] = ident
    base = S.config_c2(1, n_prefixes=10, n_policy=10)
    t = S.Tables(ipc, base.endpoints, {}, np.zeros(0, S.PREFILTER_DT),
                 {S.EP_LXC_ID: S.EP_SECLABEL})
    t.policy = {S.EP_LXC_ID: S.gen_policy(rng, 512, np.unique(ipc["label"]))}
    loc = S.local_v4_addrs(t)
    parts = [S.gen_headers_v4(rng, 3000, ipc[40 * k:40 * (k + 1)], loc, in_prefix=1.0,
                              mark_host=0, mark_proxy=0)
             for k in range(len(special))]
    # (a drop of the last packed identity at len 65535 is the one key word
    # that equals KEY_NONE: counted directly, like the identity past the limit)
    parts[2].length[::3] = 65535
    parts.append(S.gen_headers_v4(rng, 8000, ipc, loc))
    o = check(torch, t, [S.concat(parts)])
    ide = o.identity_counters()
    for ident in special:   # each took traffic
        rows = ide[ide[:, 0] == ident]
        assert len(rows) and rows[:, [2, 4]].sum() >= 1000, ident


def test_unpacked_policy_keys(torch):
    """More than 65 535 policy entries in all: bare-index keys, len from
    the header meta."""
    t = S.config_c2(14, n_prefixes=2000, n_policy=16, n_endpoints=5)
    rng = np.random.default_rng(14)
    pol = S.gen_policy(rng, 13_200, np.unique(t.ipcache["label"]))
    t.policy = {lxc: pol for lxc in t.policy}
    assert sum(len(p) for p in t.policy.values()) > 65535
    check(torch, t, [S.headers_c2(t, 20_000, seed=14)], mode=0)


def test_dual_stack_full(torch):
    t = S.config_c3(3, n_prefixes=20_000, n_v4_prefixes=2000, n_policy=2000,
                    n_prefilter=2000)
    rng = np.random.default_rng(15)
    h4 = S.gen_headers_v4(rng, 20_000, t.ipcache[t.ipcache["family"] == 1],
                          S.local_v4_addrs(t), proxy_ident=S.proxy_identities(t))
    check(torch, t, [S.headers_c3(t, 20_000, seed=4), h4])


def test_egress_second_stage(torch):
    t = S.config_c2(3, n_prefixes=2000, n_policy=512, n_endpoints=3)
    rng = np.random.default_rng(16)
    h = S.gen_headers_v4(rng, 20_000, t.ipcache, S.local_v4_addrs(t), local_frac=0.1,
                         src_fixed=S.LXC_IPV4)
    check(torch, t, [h], mode=1, ep_lxc=S.EP_LXC_ID)
