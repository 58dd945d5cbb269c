"""NAT hops the engine carries behind an egress batch, on the GPU:

  NAT46 behind IPv4 egress local delivery — ipv4_policy runs as the
  destination's program (l3.h:103-131), its ct_lookup4 hits an entry with
  nat46 (conntrack.h:241-244) and it leaves for tail_ipv4_to_ipv6 and
  ipv6_policy (bpf_lxc.c:939-944, :1098-1110): classify.hip lists the header
  from the local-delivery stage, nat.hip gathers it with the sender's
  SECLABEL as source identity, cfc_ct_apply folds the egress stage and the
  destination's hit with the IPv4 batch and the hop's ipv6_policy stage — a
  third stage — with the hop batch;

  load-balanced NAT64 — an IPv6 egress header to a v4-mapped service VIP
  (bpf_lxc.c:352-359, :1069-1082, :476-492): the hop batch's service step,
  its CT_SERVICE entries, the loopback backend, the no-backend drop.

Against the reference's fixtures (nat46_self_v4, nat64_lb_v6,
nat64_lb_lo_v6) and the oracle's sequential run.  The streams are
test_nat_hop_streams.py's, which checks on the CPU that they hold the hops.
Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import oracle as O
from cilium_amd import synth as S
from cilium_amd import _lib as L

import test_nat_hop_streams as NS
from test_nat_hop_streams import HOP_FIXTURES, MODE_EGRESS, NATLEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


@pytest.mark.parametrize("layout", ["dir24_8", "trie"])
@pytest.mark.parametrize("name", HOP_FIXTURES)
def test_hop_golden(torch, name, layout):
    """test_gpu_parity.test_golden on the three hop fixtures: action, verdict
    and pinned identity bits, policy counters and metrics against the
    reference's run; every output, the CT byte, the identity counters and
    the CT dump against the oracle; the masked CT rows against the
    reference's"""
    from test_gpu_parity import test_golden
    test_golden(torch, name, layout)


@pytest.mark.parametrize("name", HOP_FIXTURES)
def test_hop_golden_monitor_events(torch, name):
    from test_gpu_notify import test_golden_monitor_events
    test_golden_monitor_events(torch, name)


@pytest.mark.parametrize("name", HOP_FIXTURES)
def test_hop_golden_records(torch, name):
    """the records with the packet outputs on (the load balancer's launch)"""
    from test_gpu_lb import test_lb_golden_records
    test_lb_golden_records(torch, name)


@pytest.mark.parametrize("notify", [True, False])
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("name", HOP_FIXTURES)
def test_hop_streams_vs_sequential(torch, name, chunks, notify):
    """each fixture's stream three times over, shuffled: repeated packets of
    a flow in one batch, the self traffic cut into segments (each with its
    own hop batch and apply), against Oracle.run_sequential"""
    from test_gpu_ctorder import check, run_both
    g, h = NS.times(name)
    gg, want = run_both(torch, g.tables, h, MODE_EGRESS, g.ep_lxc, clock=NS.CLOCK,
                        chunks=chunks, notify=notify)
    check(gg, want)
    assert gg["stats"]["nat_hops"] >= 3000, gg["stats"]
    assert gg["stats"]["ct_apply_host"] == 0, gg["stats"]
    if name == "nat46_self_v4":
        assert gg["stats"]["ct_self_segments"] > 10, gg["stats"]


def test_self_host_apply(torch):
    """the host walk (CT_APPLY_HOST) folds the three stages too: the same
    outputs and CT dump"""
    from test_gpu_parity import run_gpu
    g, h = NS.times("nat46_self_v4", 1)
    act, ver, ide, counters, metrics = run_gpu(torch, g.tables, h, g.mode, g.ep_lxc,
                                               ct_apply=L.CT_APPLY_HOST)
    ctb, rows = run_gpu.ct
    assert run_gpu.stats["ct_apply_host"] > 0 and run_gpu.stats["nat_hops"] > 1000, run_gpu.stats
    o = O.Oracle(g.tables)
    oa, ov, oi, oct_ = o.classify(h, g.mode, g.ep_lxc, want_ct=True, apply_ct=True)
    np.testing.assert_array_equal(act, oa)
    np.testing.assert_array_equal(ver, ov)
    np.testing.assert_array_equal(ide, oi)
    np.testing.assert_array_equal(ctb, oct_)
    np.testing.assert_array_equal(rows, o.ct_dump())


@pytest.fixture(scope="module")
def edges():
    return NS.edge_batches()


@pytest.mark.parametrize("shape", ["one", "all", "pad", "two_blocks", "none"])
def test_hop_edge_shapes(torch, edges, shape):
    """the smallest batches at which the list, its sort, the gather and the
    scatter can go wrong: one hop header, all of them, a count that is no
    multiple of 4, one just over a gather block, none with the list armed"""
    from test_gpu_ctorder import check, run_both
    t, b = edges
    h, hops = b[shape]
    g, want = run_both(torch, t, h, MODE_EGRESS, S.EP_LXC_ID, clock=NS.CLOCK, chunks=1)
    check(g, want)
    assert g["stats"]["nat_hops"] == hops, g["stats"]


def test_hop_round_trip_vs_oracle(torch):
    """NAT64 flows to the endpoint's own IPv4 address opened in one IPv6
    egress batch on empty CT maps, their IPv4 replies in the next egress
    batch: the nat46 entries the device apply created feed the next classify
    (nat46_seen)"""
    from cilium_amd.datapath import Datapath, pack
    from cilium_amd.loader import ct_rows, load_tables
    t, out6, replies = NS.round_trip()
    dp = Datapath(0)
    load_tables(dp, t)
    dp.set_clock(1000)
    b6 = pack(out6)
    o6 = dp.classify(b6, MODE_EGRESS, S.EP_LXC_ID, want_ct=True)
    dp.ct_apply(b6, o6, MODE_EGRESS, S.EP_LXC_ID)
    torch.cuda.synchronize()
    act6 = o6.action.cpu().numpy()
    rep = replies(np.flatnonzero(act6 != 2))
    b4 = pack(rep)
    o4 = dp.classify(b4, MODE_EGRESS, S.EP_LXC_ID, want_ct=True, want_notify=True)
    dp.ct_apply(b4, o4, MODE_EGRESS, S.EP_LXC_ID)
    torch.cuda.synchronize()
    g = dict(act=o4.action.cpu().numpy(), ver=o4.verdict.cpu().numpy(),
             ide=o4.identity.cpu().numpy().view(np.uint32), ct=o4.ct.cpu().numpy(),
             nt=o4.notify.cpu().numpy().view(np.uint32))
    dp.counters_sync()
    rows = ct_rows(dp, dp.ct_fds)
    st = dp.stats()
    dp.close()
    o = O.Oracle(t)
    o.set_clock(1000)
    a6 = o.run_sequential(out6, MODE_EGRESS, S.EP_LXC_ID)[0]
    np.testing.assert_array_equal(act6, a6)
    act, ver, ide, words, ct = o.run_sequential(rep, MODE_EGRESS, S.EP_LXC_ID, want_ct=True)
    for k, w in (("act", act), ("ver", ver), ("ide", ide), ("ct", ct), ("nt", words)):
        bad = np.nonzero(g[k] != w)[0]
        assert len(bad) == 0, f"{k}: {len(bad)} differ, first {bad[:6]} " \
                              f"{g[k][bad[:6]]} vs {w[bad[:6]]}"
    np.testing.assert_array_equal(rows, o.ct_dump())
    hops4 = int(((words & NATLEN) != 0).sum())
    assert hops4 > 300
    assert st["nat_hops"] >= len(out6) + hops4 and st["ct_apply_host"] == 0, st


@pytest.mark.parametrize("lb", [False, True])
def test_hop_beside_services(torch, lb):
    """the self-reply stream on tables that also carry lb4 services no flow
    targets (the LB instantiation of the classify kernel, the service
    step's packet arrays as the gather's source), ipv6_policy dropping half
    of the flows' replies; and the same tables without the services"""
    from test_gpu_ctorder import check, run_both
    t, h = NS.self_tables(lb=lb)
    g, want = run_both(torch, t, h, MODE_EGRESS, S.EP_LXC_ID, clock=NS.CLOCK, chunks=2)
    check(g, want)
    nat = (want["nt"] & NATLEN) != 0
    assert g["stats"]["nat_hops"] >= nat.sum() > 300, g["stats"]
    assert (want["ver"][nat] == -133).any() and (want["act"][nat] != 2).any()
