"""Conntrack accounting at the widths of its packed fields (csrc/classify.hip
k_acc_agg / k_acc_part1 / k_acc_part2 / k_acc_reduce, and the per-slice
k_ct_count that CFC_ACC_PER_SLICE selects): one flow taking every header of
a full slice at len 65535, slices of 64 512 and 64 512 + 1 headers, a slice
over three LDS tables' worth of distinct flows, both ends of the byte field,
counters that already hold values, the egress second stage, one and several
coarse buckets.  Every CT byte, every CT row (accounting columns included),
policy counters, metrics and identity counters against the oracle, bit-exact.
The streams are ct_edge_streams.py's (preconditions: test_ct_edge_streams.py).
Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import ct_edge_streams as E
import oracle as O
from cilium_amd import metricsmap
from cilium_amd import synth as S
from cilium_amd.datapath import Datapath, pack
from cilium_amd.loader import ct_rows, load_tables, policy_rows
from test_gpu_ctorder import check as check_seq, run_both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


@pytest.fixture(params=["partition", "per_slice"])
def acc(request, monkeypatch):
    """the accounting kernels: the key-range partition (default) or the
    per-slice k_ct_count (CFC_ACC_PER_SLICE, read per call)"""
    if request.param == "per_slice":
        monkeypatch.setenv("CFC_ACC_PER_SLICE", "1")
    return request.param


def run_engine(torch, t, batches, mode, ep_lxc=0, read_between=False):
    """classify (want_ct) + ct_apply of each batch in turn on one Datapath ->
    per-batch outputs, final rows and counters, the stats after each batch"""
    dp = Datapath(0)
    try:
        pms = load_tables(dp, t)
        dp.set_clock(E.CLOCK)
        packed, outs, stats = {}, [], [dp.stats()]
        for k, h in enumerate(batches):
            if id(h) not in packed:
                packed[id(h)] = pack(h)
            b = packed[id(h)]
            out = dp.classify(b, mode, ep_lxc, want_ct=True)
            dp.ct_apply(b, out, mode, ep_lxc)
            torch.cuda.synchronize()
            outs.append((out.action.cpu().numpy().astype(np.int32), out.verdict.cpu().numpy(),
                         out.identity.cpu().numpy().view(np.uint32), out.ct.cpu().numpy()))
            stats.append(dp.stats())
            if read_between and k + 1 < len(batches):   # mirror sync, CT dump
                dp.counters_sync()
                ct_rows(dp, dp.ct_fds)
        dp.counters_sync()
        return dict(outs=outs, stats=stats, rows=ct_rows(dp, dp.ct_fds),
                    counters={lxc: np.array(policy_rows(pm), np.uint64).reshape(-1, 7)
                              for lxc, pm in pms.items()},
                    metrics=np.array(metricsmap.dump_rows(dp), np.uint64).reshape(-1, 4),
                    identity=dp.identity_counters())
    finally:
        dp.close()


def check(torch, t, batches, mode, ep_lxc=0, read_between=False):
    """the engine against the oracle on the same batches, each folded into
    CT in packet order before the next -> (engine results, the oracle)"""
    g = run_engine(torch, t, batches, mode, ep_lxc, read_between)
    o = O.Oracle(t)
    o.set_clock(E.CLOCK)
    for k, h in enumerate(batches):
        want = o.classify(h, mode, ep_lxc, want_ct=True, apply_ct=True)
        for name, a, b in zip(("action", "verdict", "identity", "ct byte"), g["outs"][k], want):
            bad = np.flatnonzero(a != b)
            assert len(bad) == 0, f"batch {k} {name}: {len(bad)} differ, first {bad[:6]} " \
                                  f"{a[bad[:6]]} vs {b[bad[:6]]}"
    rows, want = g["rows"], o.ct_dump()
    if rows.shape == want.shape:
        for r in np.flatnonzero((rows != want).any(1))[:6]:
            cols = np.flatnonzero(rows[r] != want[r])
            print("ct row", r, cols, rows[r][cols], want[r][cols], E.acct(rows[r:r + 1]),
                  E.acct(want[r:r + 1]))
    else:
        print("ct rows", rows.shape, want.shape)
    np.testing.assert_array_equal(rows, want)
    for lxc in t.policy:
        np.testing.assert_array_equal(g["counters"][lxc], o.policy_counters(lxc))
    np.testing.assert_array_equal(g["metrics"], o.metrics())
    np.testing.assert_array_equal(g["identity"], o.identity_counters())
    assert g["stats"][-1]["ct_apply_host"] == 0, g["stats"][-1]
    return g, o


def hot_gain(t, o, per_entry, entries=1):
    """the oracle's rows against the tables as loaded: `entries` rows
    changed, each by {per_entry packets, per_entry * 65535 bytes} in one
    direction"""
    o0 = O.Oracle(t)
    before, after = o0.ct_dump(), o.ct_dump()
    ch = np.flatnonzero((before != after).any(1))
    assert len(ch) == entries, ch
    for d in E.acct(after[ch]) - E.acct(before[ch]):
        assert sorted(d.reshape(2, 2).tolist()) == [[0, 0], [per_entry, per_entry * 65535]], d


@pytest.mark.parametrize("want", [E.ESTABLISHED, E.REPLY], ids=["established", "reply"])
@pytest.mark.parametrize("mode", [3, 0], ids=["full", "ingress"])
@pytest.mark.parametrize("family", [4, 6])
def test_hot_flow_maximal_lengths(torch, acc, family, mode, want):
    """One flow takes all 70 000 headers at len 65535: a slice's LDS entry
    holds 64 512 packets and 4 227 793 920 bytes (the 16-bit packet field and
    the 32-bit byte half nearly full, a high-part record of 4031), and the
    entry's byte counter passes 2^32.  IPv6: keys past ct6_acct_base."""
    t, flows = E.tables(family)
    g, o = check(torch, t, [E.hot_batch(t, flows, mode, want)], mode)
    hot_gain(t, o, E.N_HOT)
    assert g["stats"][-1]["ct_slots"] <= 262_144      # one coarse bucket


@pytest.mark.parametrize("n", [E.SLICE, E.SLICE + 1])
def test_slice_boundary(torch, acc, n):
    """A full slice exactly, and a second slice of one header."""
    t, flows = E.tables(4)
    g, o = check(torch, t, [E.hot_batch(t, flows, 3, E.ESTABLISHED, n)], 3)
    hot_gain(t, o, n)


def test_wide_slice(torch, acc):
    """64 512 headers at len 65535 over ~39 k distinct flows: most become
    single-packet records (three probes into 8192 slots), the LDS table
    fills, its entries carry flag words."""
    t, flows = E.tables(4, 60_000)
    check(torch, t, [E.wide_batch(t, flows)], 3)


def test_mixed(torch, acc):
    """Half the hot flow (1 % FIN: the slot is ordered and goes through the
    apply's fold, its accounting still from the reduce), half the wide draw,
    lengths from both ends of the byte field."""
    t, flows = E.tables(4, 60_000)
    h, _, _ = E.mixed_batch(t, flows, 3)
    check(torch, t, [h], 3)


@pytest.mark.parametrize("read_between", [False, True], ids=["no_read", "read_between"])
def test_two_batches_accumulate(torch, acc, read_between):
    """The hot batch twice: the reduce's read-modify-write lands on counters
    that already hold values — with nothing read in between, and with a
    mirror sync and a CT dump in between.  Exactly double one batch."""
    t, flows = E.tables(4)
    b = E.hot_batch(t, flows, 3, E.ESTABLISHED)
    g, o = check(torch, t, [b, b], 3, read_between=read_between)
    hot_gain(t, o, 2 * E.N_HOT)


def test_egress_second_stage(torch, acc):
    """Egress with local delivery (grid row 1, ct_idx2): a header that hits
    in the sender's lookup and in the receiver's, hot-repeated; both entries
    gain the batch, and the batch is not cut."""
    t, mode, ep, one = E.egress_second_stage()
    b = E.repeat(one, E.N_HOT)
    g, o = check(torch, t, [b], mode, ep)
    hot_gain(t, o, E.N_HOT, entries=2)
    assert g["stats"][-1]["ct_self_segments"] == g["stats"][0]["ct_self_segments"]
    for nib in (g["outs"][0][3] & 0xF, g["outs"][0][3] >> 4):
        assert np.isin(nib, [E.ESTABLISHED, E.REPLY]).all()


def test_several_coarse_buckets(torch):
    """The hot and the wide case on a table of more than 262 144 slots: the
    partition's coarse digit takes more than one value."""
    t, flows = E.tables(4, 150_000)
    g, o = check(torch, t, [E.hot_batch(t, flows, 3, E.ESTABLISHED)], 3)
    hot_gain(t, o, E.N_HOT)
    assert g["stats"][-1]["ct_slots"] > 262_144, g["stats"][-1]
    g, _ = check(torch, t, [E.wide_batch(t, flows)], 3)
    assert g["stats"][-1]["ct_slots"] > 262_144, g["stats"][-1]


def test_per_slice_switch_takes_the_dense_apply(torch, monkeypatch):
    """CFC_ACC_PER_SLICE is observable without a stat of its own: k_ct_count
    keeps no plain-hit summaries, so no apply of such a launch can be sparse.
    A three-batch dependency stream without deletes: sparse applies by
    default, none under the switch, both equal to the sequential oracle."""
    t, flows = E.tables(4, 20_000)
    h = S.headers_c5_seq(t, flows, 60_000, seed=17)
    o = O.Oracle(t)
    o.set_clock(E.CLOCK)
    _, ov, _, oct_ = o.classify(h, 3, 0, nthreads=16, want_ct=True)
    h = S.take(h, np.flatnonzero(~(((oct_ & 0xF) == E.ESTABLISHED) & (ov == -133))))
    g, want = run_both(torch, t, h, 3, clock=E.CLOCK, chunks=3, notify=False)
    check_seq(g, want)
    assert g["stats"]["ct_apply_sparse"] >= 1, g["stats"]
    monkeypatch.setenv("CFC_ACC_PER_SLICE", "1")
    gs, want = run_both(torch, t, h, 3, clock=E.CLOCK, chunks=3, notify=False)
    check_seq(gs, want)
    assert gs["stats"]["ct_apply_sparse"] == 0, gs["stats"]
    assert gs["stats"]["ct_apply_device"] == 3, gs["stats"]
