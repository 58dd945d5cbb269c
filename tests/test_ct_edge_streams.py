"""The streams of test_gpu_ct_acct_edges.py and test_gpu_batch_geometry.py
(ct_edge_streams.py) hold what those tests are about — checked with the
oracle alone, no GPU."""
import numpy as np
import pytest

import ct_edge_streams as E
import oracle as O
from cilium_amd import synth as S


def _seq(t, h, mode, ep_lxc=0):
    o = O.Oracle(t)
    o.set_clock(E.CLOCK)
    before = len(o.ct_dump())
    act, ver, ide, words, ct = o.run_sequential(h, mode, ep_lxc, want_ct=True)
    return ver, ct, before, o


@pytest.mark.parametrize("family", [4, 6])
@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("want", [E.ESTABLISHED, E.REPLY])
def test_hot_flow_deltas(family, mode, want):
    """One entry gains exactly N packets and N * 65535 bytes (past 2^32) in
    one direction's counters; nothing else in the table moves; the packet
    order and the batch fold agree."""
    t, flows = E.tables(family)
    b = E.hot_batch(t, flows, mode, want)
    assert len(b) == E.N_HOT > E.SLICE and b.length.min() == 65535
    ch, a0, a1 = E.hot_delta(t, [b], mode)
    assert len(ch) == 1
    d = (a1 - a0)[0]
    assert sorted(d.reshape(2, 2).tolist()) == [[0, 0], [E.N_HOT, E.N_HOT * 65535]], d
    assert E.N_HOT * 65535 == 4_587_450_000 > 1 << 32
    o = O.Oracle(t)
    o.set_clock(E.CLOCK)
    ct = o.classify(b, mode, 0, nthreads=8, want_ct=True, apply_ct=True, seq=False)[3]
    assert (ct == want).all()
    o2 = O.Oracle(t)
    o2.set_clock(E.CLOCK)
    o2.run_sequential(b, mode, 0)
    np.testing.assert_array_equal(o.ct_dump(), o2.ct_dump())


def test_hot_flow_twice_is_double():
    t, flows = E.tables(4)
    b = E.hot_batch(t, flows, 3, E.ESTABLISHED)
    _, a0, a1 = E.hot_delta(t, [b], 3)
    _, b0, b1 = E.hot_delta(t, [b, b], 3)
    np.testing.assert_array_equal(b1 - b0, 2 * (a1 - a0))


@pytest.mark.parametrize("n_flows", [60_000, 150_000])
def test_wide_slice_keys(n_flows):
    """One full slice over at least three LDS tables' worth of distinct live
    flows, every header a CT hit at the batch's start, no closes."""
    t, flows = E.tables(4, n_flows)
    h = E.wide_batch(t, flows)
    assert len(h) == E.SLICE
    o = O.Oracle(t)
    o.set_clock(E.CLOCK)
    ct = o.classify(h, 3, 0, nthreads=8, want_ct=True)[3]
    assert np.isin(ct & 0xF, [E.ESTABLISHED, E.REPLY]).all()
    pairs = np.unique(h.saddr.astype(np.uint64) << 32 | h.daddr)
    keys = np.unique(E.flow_keys(h), axis=0)
    assert len(keys) >= len(pairs) >= 3 * E.LDS_SLOTS, (len(pairs), len(keys))
    if n_flows == 60_000:
        assert (len(pairs), len(keys)) == (26_526, 39_415)
    assert not (h.flags & S.HF_TCP_CLOSE).any()
    tf = h.tcpflags[h.proto == S.IPPROTO_TCP]
    assert set(np.unique(tf)) == {E.ACK, E.PSH_ACK, E.SYN_ACK}
    assert (h.length == 65535).all()


def test_mixed_batch():
    t, flows = E.tables(4, 60_000)
    h, is_hot, one = E.mixed_batch(t, flows, 3)
    assert 0.45 < is_hot.mean() < 0.55
    same = (E.flow_keys(h) == E.flow_keys(one)[0]).all(1)
    assert (same[is_hot]).all()
    fin = same & ((h.flags & S.HF_TCP_CLOSE) != 0)
    assert 0.005 * is_hot.sum() < fin.sum() < 0.02 * is_hot.sum()
    assert (h.tcpflags[fin] == E.FIN_ACK).all()
    assert not (h.flags[~is_hot] & S.HF_TCP_CLOSE).any()
    assert set(np.unique(h.length)) == set(E.LENGTHS.tolist())
    # the hot flow stays a hit to the end (a closing entry still counts)
    ver, ct, _, _ = _seq(t, h, 3)
    assert ((ct[is_hot] & 0xF) == E.ESTABLISHED).all() and (ver[is_hot] == 0).all()
    assert len(np.unique(E.flow_keys(h)[~is_hot], axis=0)) >= 2 * E.LDS_SLOTS


def test_egress_second_stage_header():
    """Both nibbles of the CT byte a hit, the destination a local endpoint
    other than the sender, and both stages' entries count the hot batch."""
    t, mode, ep, one = E.egress_second_stage()
    assert mode == 1
    assert one.daddr[0] != one.saddr[0] and one.daddr[0] != S.LXC_IPV4
    assert one.daddr[0] in S.local_v4_addrs(t)
    b = E.repeat(one, E.N_HOT)
    ver, ct, _, _ = _seq(t, b, mode, ep)
    assert (ver == 0).all()
    for nib in (ct & 0xF, ct >> 4):
        assert np.isin(nib, [E.ESTABLISHED, E.REPLY]).all()
    ch, a0, a1 = E.hot_delta(t, [b], mode, ep)
    assert len(ch) == 2     # the sender's entry and the receiver's
    for d in a1 - a0:
        assert sorted(d.reshape(2, 2).tolist()) == [[0, 0], [E.N_HOT, E.N_HOT * 65535]], d


@pytest.mark.parametrize("kind", ["v4_full", "v4_ingress", "v4_egress", "v6_full"])
def test_ragged_stream(kind):
    """Every batch of 1023 headers or more creates an entry; the stream
    deletes and closes; the schedule covers the stream exactly."""
    t, h, mode, ep, _ = E.ragged_stream(kind)
    cuts = E.cuts()
    assert cuts[-1][1] == len(h) == sum(E.SIZES)
    ver, ct, before, o = _seq(t, h, mode, ep)
    create = ((ct & 0x8) != 0) | ((ct & 0x80) != 0)
    for a, b in cuts:
        if b - a >= 1023:
            assert create[a:b].any(), (a, b)
    tcp_close = (h.proto == S.IPPROTO_TCP) & ((h.flags & S.HF_TCP_CLOSE) != 0)
    hit = np.isin(ct & 0x7, [E.ESTABLISHED, E.REPLY])
    assert (tcp_close & hit).sum() >= 1                  # a close of a live entry
    assert (((ct & 0xF) == E.ESTABLISHED) & (ver == -133)).sum() >= 1   # a delete
    assert len(o.ct_dump()) != before
