"""The streams of test_gpu_nat_hops.py, checked on the CPU against the oracle
alone: they reach what the GPU tests claim to compare — NAT46 hops behind an
IPv4 egress batch's local delivery (ipv4_policy as the destination's program,
l3.h:103-131 -> bpf_lxc.c:939-944, :1098-1110) and load-balanced NAT64 hops
(an IPv6 egress header to a v4-mapped service VIP).  The builders here are
the GPU tests' too."""
import numpy as np

import golden_io as G
import oracle as O
from cilium_amd import synth as S

MODE_EGRESS = 1
NATLEN = 1 << 24
CLOCK = 1003
HOP_FIXTURES = ["nat46_self_v4", "nat64_lb_v6", "nat64_lb_lo_v6"]


def times(name, k=3, seed=7):
    """the fixture's tables, and its stream k times over, shuffled"""
    g = G.Golden(name)
    h = S.concat([g.headers] * k)
    if k > 1:
        h = S.take(h, np.random.default_rng(seed).permutation(len(h)))
    return g, h


def run_seq(t, h, ep=S.EP_LXC_ID, clock=CLOCK, o=None):
    o = o or O.Oracle(t)
    o.set_clock(clock)
    act, ver, ide, words, ct = o.run_sequential(h, MODE_EGRESS, ep, want_ct=True)
    return o, act, ver, words, ct


def edge_batches():
    """nat46_self_v4's tables and batches cut from its stream, each with the
    number of hop headers it is built for: -> (tables, {name: (headers,
    hops)}).  A hop header is a reply the batch-start view sends through the
    hop (TCP / UDP only: an ICMP error's RELATED lookup depends on the
    batch's creates); the plain ones go to remote peers."""
    g = G.Golden("nat46_self_v4")
    h = g.headers
    o = O.Oracle(g.tables)
    o.set_clock(CLOCK)
    words = o.classify(h, MODE_EGRESS, g.ep_lxc, want_notify=True, seq=False)[3]
    hop = np.flatnonzero(((words & NATLEN) != 0) & (h.proto != S.IPPROTO_ICMP))
    plain = np.flatnonzero(h.daddr != S.LXC_IPV4)
    rng = np.random.default_rng(5)

    def mix(nh, npl):
        idx = np.concatenate([rng.choice(hop, size=nh, replace=False),
                              rng.choice(plain, size=npl, replace=False)])
        return S.take(h, np.sort(idx)), nh   # (stream order: a flow's packets in theirs)

    return g.tables, {
        "one": mix(1, 70),            # one hop header among plain egress headers
        "all": mix(64, 0),            # every header hops
        "pad": mix(7, 30),            # not a multiple of 4 (the rows' 16-byte padding)
        "two_blocks": mix(259, 40),   # just over one 256-row gather block
        "none": mix(0, 60),           # list armed, count 0
    }


def round_trip(seed=71, n=600):
    """-> (tables with empty CT maps, the IPv6 egress batch of NAT64 flows to
    ::ffff:LXC_IPV4, a function (forwarded indices) -> the IPv4 egress batch
    of their replies)"""
    t, ipc4 = S.config_nat_self(seed)
    t.ct = np.zeros(0, S.CT_DT)
    out6 = S.nat64_self_flows(np.random.default_rng(seed + 1), ipc4, n, 20000)
    return t, out6, lambda ok: S.headers_nat46_self(t, ipc4, out6, ok, seed=seed + 2)


def self_tables(seed=73, n_hist=400, lb=False):
    """config_nat_self's tables with the CT state of a self NAT64 history,
    with lb also lb4 services no flow targets; the endpoint admits the
    replies of the first half of the flows only (by their port), ipv6_policy
    drops the others' -> (tables, reply stream)"""
    t, ipc4 = S.config_nat_self(seed, allow_ports=range(20000, 20000 + n_hist // 2))
    rng = np.random.default_rng(seed + 9)
    if lb:
        t.lb4, t.revnat4, vips, ports, protos = S.lb4_services(rng, t, n_services=12)
    hist = S.nat64_self_flows(rng, ipc4, n_hist, 20000)
    o, act, ver, words, ct = run_seq(t, hist, clock=1000)
    t.ct = S.ct_from_rows(o.ct_dump())
    return t, S.headers_nat46_self(t, ipc4, hist, np.flatnonzero(act != 2), seed=seed)


def n6(rows):
    return int((rows[:, 3] == 2).sum())   # (CT_ROW: owner u16, map u8, family u8)


def test_self_stream_times_three():
    g, h = times("nat46_self_v4")
    assert len(h) == 4749
    o, act, ver, words, ct = run_seq(g.tables, h)
    nat = (words & NATLEN) != 0
    print("hops", nat.sum(), "ct rows", len(o.ct_dump()), "v6", n6(o.ct_dump()))
    assert nat.sum() >= 3000
    # the IPv6 rows are the hops' creates (ct_create6)
    before = n6(O.Oracle(g.tables).ct_dump())
    assert n6(o.ct_dump()) > before + 100
    hi = ct[nat] >> 4
    assert (hi == 6).any() and (hi == 7).any()        # REPLY|DONE, RELATED|DONE
    assert (act[nat] != 2).any()


def test_fixture_hops_times_one():
    """the fixture itself: the hop count and high nibbles it was recorded with"""
    g, h = times("nat46_self_v4", 1)
    o = O.Oracle(g.tables)
    act, ver, ide, ct, words = o.classify(h, g.mode, g.ep_lxc, want_ct=True, want_notify=True,
                                          apply_ct=True)
    nat = (words & NATLEN) != 0
    assert len(h) == 1583 and nat.sum() == 1109
    hi = ct >> 4
    assert (hi == 6).sum() == 1120 and (hi == 7).sum() == 143


def test_lb_streams_times_three():
    for name, n in (("nat64_lb_v6", 6102), ("nat64_lb_lo_v6", 6042)):
        g, h = times(name)
        assert len(h) == n
        o, act, ver, words, ct = run_seq(g.tables, h)
        nat = (words & NATLEN) != 0
        assert nat.sum() == n, name                      # every header a hop
        if name == "nat64_lb_v6":
            assert (ver == -158).any()                   # DROP_NO_SERVICE still creates
        assert (ver == -133).any() and (act != 2).any()


def test_edge_batches_hop_counts():
    t, b = edge_batches()
    for name, (h, hops) in b.items():
        o, act, ver, words, ct = run_seq(t, h)
        nat = (words & NATLEN) != 0
        # a dropped hop has no event word: count by the CT byte too — a hop
        # header's high nibble is a hit without create, verdict the hop's
        assert nat.sum() <= hops, name
        got = int(((h.daddr == S.LXC_IPV4) & ((ct >> 4) & 4).astype(bool) &
                   (((ct >> 4) & 3) >= 2)).sum())
        assert got == hops, (name, got, hops)
    assert len(b["pad"][0]) % 4 and b["pad"][1] % 4 and b["two_blocks"][1] > 256


def test_round_trip_and_lb_streams():
    t, out6, replies = round_trip()
    o, act, ver, words, ct = run_seq(t, out6, clock=1000)
    assert ((words & NATLEN) != 0).sum() > 300
    rep = replies(np.flatnonzero(act != 2))
    rows6 = n6(o.ct_dump())
    o, act, ver, words, ct = run_seq(t, rep, clock=1000, o=o)
    assert ((words & NATLEN) != 0).sum() > 300
    assert n6(o.ct_dump()) > rows6
    t, h = self_tables(lb=True)
    assert t.lb4 is not None and len(t.lb4)
    o, act, ver, words, ct = run_seq(t, h)
    nat = (words & NATLEN) != 0
    assert nat.sum() > 300
    # ipv6_policy decides: drops and forwards among the hop headers
    assert (ver[nat] == -133).sum() > 50 and (act[nat] != 2).sum() > 50
