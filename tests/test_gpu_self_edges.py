"""The self-traffic batch cuts at their structural and semantic edges
(cfc_api.cpp self_cuts / classify, selfseg.hip k_self_mark, selfcut.hpp
self_cut_rule; DESIGN.md §4 "Traffic to itself").  Every case runs classify,
cfc_ct_apply and the monitor records on the engine and compares every output,
CT byte, event word, record, counter and CT row with the oracle in packet
order (Oracle.run_sequential), and asserts the exact number of segments the
Python restatement of the rule gives (self_edges.cut_rule, pinned to the C++
by test_self_edges.py, which also checks that each stream holds the
dependency it claims).  Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import ct_edge_streams as CE
import oracle as O
import self_edges as E
from cilium_amd import _lib as L
from cilium_amd import ctmap, metricsmap
from cilium_amd.datapath import Datapath, pack
from cilium_amd.loader import ct_rows, load_tables, policy_rows
from test_gpu_batch_geometry import GuardedOut, misaligned_batch, run_schedule
from test_gpu_ctorder import check
from test_gpu_self import _self_stream

pytestmark = pytest.mark.gpu
FAMILIES = [4, 6]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


def run_batches(torch, t, batches, mode=E.EGRESS, ep=E.EP, clocks=None, gc=False,
                ct_apply=L.CT_APPLY_DEVICE, off=None, rows_each=False):
    """test_gpu_ctorder.run_both over explicit batches: the engine batch by
    batch on one Datapath (classify, cfc_ct_apply, monitor records) and the
    oracle one header at a time.  clocks: the clock of each batch; gc: both
    sides collect expired entries before each batch (fresh CT state, see
    self_edges.py); off: (inputs', outputs') element offset of guarded views
    (test_gpu_batch_geometry); rows_each: the CT maps are dumped after every
    batch as well ("rows_each" of both sides).  -> (got, want,
    ct_self_segments added by each batch)"""
    clocks = clocks if clocks is not None else [E.BASE_CLOCK] * len(batches)
    dp = Datapath(0)
    try:
        dp.set_option(L.OPT_CT_APPLY, ct_apply)
        pms = load_tables(dp, t)
        g = {k: [] for k in ("act", "ver", "ide", "ct", "nt", "rec", "idx")}
        segs, seen, a, each = [], 0, 0, []
        for h, clock in zip(batches, clocks):
            dp.set_clock(clock)
            if gc:
                ctmap.GC(dp, -1, ctmap.GCFilter(remove_expired=True), now=clock)
            sub = pack(h)
            go = None
            if off is not None:
                sub = misaligned_batch(torch, sub, off[0])
                go = GuardedOut(torch, len(h), off[1], True, sub.ports.device)
            out = dp.classify(sub, mode, ep, out=go.out if go else None, want_ct=True,
                              want_notify=True)
            dp.ct_apply(sub, out, mode, ep)
            rec, idx, total = dp.monitor_events(sub, out, mode, ep)
            torch.cuda.synchronize()
            if go:
                go.intact()
            g["act"].append(out.action.cpu().numpy())
            g["ver"].append(out.verdict.cpu().numpy())
            g["ide"].append(out.identity.cpu().numpy().view(np.uint32))
            g["ct"].append(out.ct.cpu().numpy())
            g["nt"].append(out.notify.cpu().numpy().view(np.uint32))
            g["rec"].append(np.ascontiguousarray(rec.cpu().numpy()).view(O.EVENT_DT).reshape(-1))
            g["idx"].append(idx.cpu().numpy().astype(np.uint64) + a)
            a += len(h)
            now = dp.stats()["ct_self_segments"]
            segs.append(now - seen)
            seen = now
            if rows_each:
                dp.counters_sync()
                each.append(ct_rows(dp, dp.ct_fds))
        g = {k: np.concatenate(v) for k, v in g.items()}
        g["rows_each"] = each
        dp.counters_sync()
        g["counters"] = {lxc: np.array(policy_rows(pm), np.uint64).reshape(-1, 7)
                         for lxc, pm in pms.items()}
        g["metrics"] = np.array(metricsmap.dump_rows(dp), np.uint64).reshape(-1, 4)
        g["identity"] = dp.identity_counters()
        g["rows"] = ct_rows(dp, dp.ct_fds)
        g["stats"] = dp.stats()
    finally:
        dp.close()
    return g, oracle_batches(t, batches, mode, ep, clocks, gc, rows_each), segs


def oracle_batches(t, batches, mode, ep, clocks, gc=False, rows_each=False):
    o = O.Oracle(t)
    w = {k: [] for k in ("act", "ver", "ide", "ct", "nt", "rec", "idx")}
    a, each = 0, []
    for h, clock in zip(batches, clocks):
        o.set_clock(clock)
        if gc:
            o.ct_gc(time=clock)
        act, ver, ide, words, ct = o.run_sequential(h, mode, ep, want_ct=True)
        rec, idx = o.events(h, mode, ep, ver, ide, words)
        for k, v in zip(("act", "ver", "ide", "ct", "nt", "rec", "idx"),
                        (act, ver, ide, ct, words, rec, idx + np.uint64(a))):
            w[k].append(v)
        a += len(h)
        if rows_each:
            each.append(o.ct_dump())
    w = {k: np.concatenate(v) for k, v in w.items()}
    w["rows_each"] = each
    w.update(rows=o.ct_dump(), metrics=o.metrics(), identity=o.identity_counters(),
             counters={lxc: o.policy_counters(lxc) for lxc in t.policy})
    return w


def cuts_of(c, h=None):
    return E.expected_cuts(c.t, c.h if h is None else h, c.mode, c.ep)


# ------------------------------------------------------ 1, 2: pairs, triples
@pytest.mark.parametrize("which", ["pairs", "triples"])
@pytest.mark.parametrize("family", FAMILIES)
def test_blocks_one_batch_each(torch, family, which):
    """every block its own batch on one Datapath, from fresh CT state: each
    batch adds exactly the rule's segments (pairs: 0 or 1) and leaves the
    oracle's CT entries (the next block's collection removes them)"""
    blocks = E.pair_blocks(family) if which == "pairs" else E.triple_blocks(family)
    t = E.env(family).t
    g, want, segs = run_batches(torch, t, [b.h for b in blocks],
                                clocks=[E.clock_of(k) for k in range(len(blocks))], gc=True,
                                rows_each=True)
    exp = [len(E.expected_cuts(t, b.h)) for b in blocks]
    bad = [(b.names, s, e) for b, s, e in zip(blocks, segs, exp) if s != e]
    assert not bad, bad[:8]
    assert 0 < sum(exp) < (len(blocks) if which == "pairs" else 2 * len(blocks))
    for b, got, exp_rows in zip(blocks, g["rows_each"], want["rows_each"]):
        assert got.shape == exp_rows.shape and (got == exp_rows).all(), b.names
    check(g, want)


@pytest.mark.parametrize("which", ["pairs", "triples"])
@pytest.mark.parametrize("family", FAMILIES)
def test_blocks_concatenated(torch, family, which):
    """the same blocks as one batch: the rule's count over the whole list"""
    c = E.cut_cases(family)[which]
    g, want, segs = run_batches(torch, c.t, [c.h])
    assert segs == [len(cuts_of(c))] and segs[0] > 100, segs
    check(g, want)


# ------------------------------------------- 3: the listing's structural edges
@pytest.mark.parametrize("family", FAMILIES)
def test_listing_at_structural_edges(torch, family):
    """n = 8192 * 256 + 257: k_self_mark's grid-stride loop takes a second,
    ragged iteration; listed headers at 0, 1, 63, 64, 255, 256, 2 097 151,
    2 097 152 and n-1, dependent pairs across 63|64, 255|256 and
    2 097 151|2 097 152, and 130 consecutive independent listed headers
    across two wave boundaries.  Eight cuts, every output against the oracle."""
    h, at = E.structural_stream(family)
    c = E.Case(E.env(family).t, h)
    g, want, segs = run_batches(torch, c.t, [h])
    assert segs == [8] and len(cuts_of(c)) == 8, segs
    check(g, want)


# ------------------------------------------------------- 4: segment geometry
@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["one_flow", "edge_cuts"])
@pytest.mark.parametrize("family", FAMILIES)
def test_segment_geometry(torch, family, name, off):
    """299 segments of one header each, and cuts at indices 1 and n-1 only,
    with inputs and outputs at element offsets 0-3 of guarded allocations:
    every segment's sub-batch starts at another alignment; nothing outside
    the views is written"""
    c = E.cut_cases(family)[name]
    g, want, segs = run_batches(torch, c.t, [c.h], off=(off, off))
    assert segs == [299 if name == "one_flow" else 2] and segs == [len(cuts_of(c))]
    check(g, want)


@pytest.mark.parametrize("family", FAMILIES)
def test_ragged_schedule_over_a_self_stream(torch, family):
    """test_gpu_batch_geometry's ragged schedule (batches of 1 ... 20 001
    headers, guarded views at offset 1) over a self stream: every scheduled
    batch is cut again inside"""
    c = E.ragged_self(family, _self_stream, sum(CE.SIZES))
    g = run_schedule(torch, c.t, c.h, c.mode, c.ep, True, 1, 1)
    exp = sum(len(cuts_of(c, c.h.slice(a, b))) for a, b in CE.cuts(CE.SIZES))
    assert g["stats"]["ct_self_segments"] == exp and exp > 1000
    check(g, oracle_batches(c.t, [c.h], c.mode, c.ep, [CE.CLOCK]))


# ---------------------------------------------------------- 5: the address set
ADDRESS_CASES = ["svc_2", "svc_l3", "loopback", "no_services", "no_address", "second_endpoint"]


@pytest.mark.parametrize("family,name", [(f, n) for f in FAMILIES for n in ADDRESS_CASES
                                         if (f, n) != (6, "loopback")])   # (IPv4 only)
def test_address_set(torch, family, name):
    """one stream per shape of the address set self_cuts builds on the host:
    a service with the endpoint at slave slot 2, one with that slot under the
    L3 key, IPV4_LOOPBACK itself, tables without service maps (no loopback
    address; a self TCP flow still cut), an endpoint without an address of
    the family and another endpoint's batch to this one's address (nothing
    listed)"""
    c = E.address_cases(family)[name]
    g, want, segs = run_batches(torch, c.t, [c.h], c.mode, c.ep)
    assert segs == [len(cuts_of(c))], (segs, cuts_of(c))
    assert (segs[0] > 0) == c.cut
    check(g, want)


# ---------------------------------------------------- 6: no cut where none is due
@pytest.mark.parametrize("name", ["ingress", "full", "independent"])
@pytest.mark.parametrize("family", FAMILIES)
def test_no_cut(torch, family, name):
    """the self-addressed stream in INGRESS and FULL mode, and an egress
    batch of pairwise independent listed headers: one launch"""
    c = E.no_cut_cases(family)[name]
    g, want, segs = run_batches(torch, c.t, [c.h], c.mode, c.ep)
    assert segs == [0] and cuts_of(c) == []
    check(g, want)


@pytest.mark.parametrize("family", FAMILIES)
def test_no_cut_without_ct_outputs(torch, family):
    """an egress batch classified without CT outputs is never cut: every
    header is looked up against the maps as the batch found them"""
    c = E.cut_cases(family)["one_flow"]
    dp = Datapath(0)
    try:
        load_tables(dp, c.t)
        dp.set_clock(E.BASE_CLOCK)
        out = dp.classify(pack(c.h), c.mode, c.ep)
        torch.cuda.synchronize()
        got = (out.action.cpu().numpy(), out.verdict.cpu().numpy(),
               out.identity.cpu().numpy().view(np.uint32))
        assert dp.stats()["ct_self_segments"] == 0
    finally:
        dp.close()
    o = O.Oracle(c.t)
    o.set_clock(E.BASE_CLOCK)
    for a, b in zip(got, o.classify(c.h, c.mode, c.ep)):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------ 7: growth and the host walk inside
@pytest.mark.parametrize("family", FAMILIES)
def test_segment_apply_grows_the_table(torch, family):
    """a device table sized for a few hundred entries; 6000 plain new flows
    before the first cut: the first segment's apply, inside cfc_classify,
    takes the table past 3/4 load and grows it on the device"""
    c = E.growth_case(family)
    g, want, segs = run_batches(torch, c.t, [c.h])
    assert segs == [len(cuts_of(c))] and segs[0] == 39
    check(g, want)
    st = g["stats"]
    assert st["ct_grown"] >= 1 and st["ct_apply_host"] == 0, st


_host_walk = {}


def host_walk_run(torch, family):
    if family not in _host_walk:
        c = E.cut_cases(family)["pairs"]
        _host_walk[family] = (c,) + run_batches(torch, c.t, [c.h], ct_apply=L.CT_APPLY_HOST)
    return _host_walk[family]


@pytest.mark.parametrize("family", FAMILIES)
def test_pairs_under_the_host_walk(torch, family):
    """the concatenated pairs with the apply's host walk chosen: the same
    cuts, verdicts, identities, CT bytes, CT rows and counters;
    ct_apply_host counts the caller's one apply, not the segments'.  (The
    event words and records: test_host_walk_event_words.)"""
    c, g, want, segs = host_walk_run(torch, family)
    assert segs == [len(cuts_of(c))]
    assert g["stats"]["ct_apply_host"] == 1, g["stats"]
    # (check() holds every case to the device path: the one host apply is
    # this case's subject and was asserted above)
    g = {k: v for k, v in g.items() if k not in ("nt", "rec", "idx")}
    g["stats"] = dict(g["stats"], ct_apply_host=0)
    check(g, want)


@pytest.mark.parametrize("family", FAMILIES)
def test_host_walk_event_words(torch, family):
    """the host walk re-decides a trace word's CT result and monitor length
    in packet order, as the device apply does (ctapply.hip k_cta_mon): the
    second packet of a flow the batch itself created reports ESTABLISHED and,
    inside the flow's report interval, one byte.  Before it did, 3 of the
    1152 / 1250 words of the pair streams kept the batch-start view (the
    second packets of the never-listed pairs local_tcp, remote_tcp,
    remote_udp: e.g. 0x441011 against the oracle's 0xD41011)."""
    c, g, want, segs = host_walk_run(torch, family)
    bad = np.flatnonzero(g["nt"] != want["nt"])
    print("host walk event words differ at", bad, [hex(x) for x in g["nt"][bad]],
          [hex(x) for x in want["nt"][bad]])
    assert len(bad) == 0, (bad, g["nt"][bad], want["nt"][bad])
    np.testing.assert_array_equal(g["rec"].view(np.uint8), want["rec"].view(np.uint8))
