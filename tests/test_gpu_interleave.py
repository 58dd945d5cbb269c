"""Classified batches outstanding before their applies (include/cfc.h: any
number, applied in any order, matched by cfc_out.ct).  The engine carries
four pieces of state from a batch's cfc_classify to its cfc_ct_apply
(cfc_api.cpp): the last launch's hit slots and work bits (last_cls, valid
while ct_gen stands), the plain-hit summaries (sum_dirty / sum_pending /
sum_want), the NAT hop batches (nat, keyed by cfc_out.ct) and the cut
records of batches with traffic to themselves (segs, keyed the same way).
Every other GPU test calls classify(X), ct_apply(X), then the next batch;
here another batch — its own buffers, another family, a hop batch, a table
growth, or the same buffers with other content — comes in between.

Expected values come from the oracle alone.  A batch classified while
another one's writes are partly folded has a defined answer only when the
two share no CT key, so every scenario's batches are independent by
construction (split by address: a CT key holds both addresses, and so does a
create's ICMP entry) and the expectation is one oracle folding them one after
another in packet order.  test_batches_are_independent (CPU, the oracle only)
checks that condition — the same result in either order — and that each
stream reaches the branch its scenario is about.  The GPU tests run on an
MI355X (pytest -m gpu); every header of every batch is compared, and every
CT entry, policy counter row, metric and identity counter, for equality."""
import copy
import dataclasses
import errno
import functools

import numpy as np
import pytest

import golden_io as G
import oracle as O
from cilium_amd import synth as S

MODE_INGRESS, MODE_EGRESS, MODE_FULL = 0, 1, 3
NATLEN = 1 << 24
KEYS = ("act", "ver", "ide", "ct")


@dataclasses.dataclass
class Batch:
    h: S.Headers
    mode: int
    ep_lxc: int = 0
    # classified into the tensors of this earlier batch (same n, mode and
    # endpoint): the caller reusing its buffers for other content
    into: int | None = None
    # the oracle folds only its first `folded` headers (a cut batch that is
    # classified and never applied: cfc_classify folded its segments before
    # the last); None: all of them
    folded: int | None = None


@dataclasses.dataclass
class Scenario:
    tables: S.Tables
    batches: list
    clock: int | None = None


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


# ---- the schedule runner ---------------------------------------------------

def run_schedule(torch, sc, steps, streams=None):
    """steps ("classify", i) / ("apply", i) over sc.batches on one Datapath
    with the device apply; every batch's packed inputs and Verdicts live to
    the end; a batch's outputs are read after its own apply.  streams: batch
    index -> torch.cuda.Stream of its classify and apply.  -> per-batch
    outputs (None for a batch never applied) and the final state."""
    from cilium_amd import _lib as L
    from cilium_amd import metricsmap
    from cilium_amd.datapath import Datapath, pack
    from cilium_amd.loader import ct_rows, load_tables, policy_rows
    dp = Datapath(0)
    dp.set_option(L.OPT_CT_APPLY, L.CT_APPLY_DEVICE)
    pms = load_tables(dp, sc.tables)
    if sc.clock is not None:
        dp.set_clock(sc.clock)
    nb = len(sc.batches)
    packed = [pack(b.h) for b in sc.batches]
    outs = [None] * nb
    got = [None] * nb
    streams = streams or {}
    for what, i in steps:
        b = sc.batches[i]
        st = streams.get(i)
        j = i if b.into is None else b.into
        if what == "classify":
            if b.into is not None:   # other content in batch j's own tensors
                assert len(b.h) == len(sc.batches[j].h)
                for f in dataclasses.fields(packed[j]):
                    dst, src = getattr(packed[j], f.name), getattr(packed[i], f.name)
                    assert (dst is None) == (src is None), f.name
                    if dst is not None:
                        dst.copy_(src)
            outs[j] = dp.classify(packed[j], b.mode, b.ep_lxc, out=outs[j], want_ct=True,
                                  stream=st)
        elif what == "refuse":
            # the batch's outputs with one header less: not its apply
            n = len(b.h)
            with pytest.raises(OSError) as e:
                dp.ct_apply(packed[j].slice(0, n - 1), outs[j], b.mode, b.ep_lxc, stream=st)
            assert e.value.errno == errno.EINVAL, e.value
        else:
            out = outs[j]
            dp.ct_apply(packed[j], out, b.mode, b.ep_lxc, stream=st)
            torch.cuda.synchronize()
            got[i] = dict(act=out.action.cpu().numpy().astype(np.int32),
                          ver=out.verdict.cpu().numpy(),
                          ide=out.identity.cpu().numpy().view(np.uint32),
                          ct=out.ct.cpu().numpy())
    torch.cuda.synchronize()
    dp.counters_sync()
    state = dict(
        rows=ct_rows(dp, dp.ct_fds),
        counters={lxc: np.array(policy_rows(pm), np.uint64).reshape(-1, 7)
                  for lxc, pm in pms.items()},
        metrics=np.array(metricsmap.dump_rows(dp), np.uint64).reshape(-1, 4),
        identity=dp.identity_counters(), stats=dp.stats())
    dp.close()
    del packed, outs
    return got, state


def fold(sc, order=None):
    """One oracle over the batches in `order` (default: as listed), each in
    packet order (Oracle.run_sequential) -> per-batch outputs, final state.
    A batch with `folded` set: its first `folded` headers that way, the rest
    classified against the maps they left and not folded."""
    o = O.Oracle(sc.tables)
    if sc.clock is not None:
        o.set_clock(sc.clock)
    want = [None] * len(sc.batches)
    for i in (range(len(sc.batches)) if order is None else order):
        b = sc.batches[i]
        k = len(b.h) if b.folded is None else b.folded
        r = o.classify(b.h.slice(0, k), b.mode, b.ep_lxc, want_ct=True, apply_ct=True)
        if k < len(b.h):
            r2 = o.classify(b.h.slice(k, len(b.h)), b.mode, b.ep_lxc, want_ct=True)
            r = tuple(np.concatenate([x, y]) for x, y in zip(r, r2))
        want[i] = dict(zip(KEYS, r))
    state = dict(rows=o.ct_dump(), metrics=o.metrics(), identity=o.identity_counters(),
                 counters={lxc: o.policy_counters(lxc) for lxc in sc.tables.policy})
    return want, state


@functools.lru_cache(maxsize=None)
def expected(name):
    """(scenario, the oracle's per-batch outputs, its final state): computed
    once, shared by the schedules of a scenario, never written to"""
    sc = SCENARIOS[name]()
    want, state = fold(sc)
    for w in want:
        for a in w.values():
            a.setflags(write=False)
    state["rows"].setflags(write=False)
    return sc, want, state


def check(sc, got, state, want, wstate, applied):
    for i in applied:
        for k in KEYS:
            bad = np.nonzero(got[i][k] != want[i][k])[0]
            assert len(bad) == 0, f"batch {i} {k}: {len(bad)} of {len(want[i][k])} differ, " \
                f"first {bad[:6]} {got[i][k][bad[:6]]} vs {want[i][k][bad[:6]]}"
    a, b = state["rows"], wstate["rows"]
    if a.shape == b.shape:
        for r in np.nonzero((a != b).any(1))[0][:4]:
            cols = np.nonzero(a[r] != b[r])[0]
            print("ct row", r, cols, a[r][cols], b[r][cols], a[r].tobytes().hex())
    else:
        print("ct rows", a.shape, b.shape)
    np.testing.assert_array_equal(a, b)
    for lxc, exp in wstate["counters"].items():
        np.testing.assert_array_equal(state["counters"][lxc], exp)
    np.testing.assert_array_equal(state["metrics"], wstate["metrics"])
    np.testing.assert_array_equal(state["identity"], wstate["identity"])


def schedule(text):
    """'cA cB aB aA' -> steps (x: an apply that must be refused)"""
    return [({"c": "classify", "a": "apply", "x": "refuse"}[w[0]], ord(w[1]) - ord("A"))
            for w in text.split()]


def run_and_check(torch, name, text, streams=None):
    sc, want, wstate = expected(name)
    steps = schedule(text)
    got, state = run_schedule(torch, sc, steps, streams)
    st = state["stats"]
    print(name, text, {k: st[k] for k in ("ct_apply_device", "ct_apply_host",
                                          "ct_apply_sparse", "ct_self_segments",
                                          "ct_grown", "nat_hops")})
    check(sc, got, state, want, wstate, [i for w, i in steps if w == "apply"])
    assert st["ct_apply_host"] == 0, st
    return st


# ---- the streams -----------------------------------------------------------

def _self_addrs(t, v6):
    """the destinations that may touch the endpoint's own entries: its
    address, IPV4_LOOPBACK, every service VIP and backend"""
    if v6:
        a = [np.asarray(S.LXC_IPV6, np.uint8)[None, :]]
        lb = getattr(t, "lb6", None)
        if lb is not None:
            a += [lb["addr"], lb["target"]]
        return np.unique(np.concatenate(a), axis=0)
    a = [np.array([S.LXC_IPV4, S.IPV4_LOOPBACK], np.uint32)]
    lb = getattr(t, "lb4", None)
    if lb is not None:
        a += [lb["addr"].astype(np.uint32), lb["target"].astype(np.uint32)]
    return np.unique(np.concatenate(a))


def _to_self(h, addrs):
    if h.family == 6:
        d = np.ascontiguousarray(h.daddr, np.uint8)
        return (d[:, None, :] == addrs[None, :, :]).all(2).any(1)
    return np.isin(h.daddr, addrs)


def _self_scenario(name, seed, n):
    """1: A the self and service part of test_gpu_self's stream (cut by
    cfc_classify), B the plain rest, the same endpoint's egress"""
    from test_gpu_self import _self_stream
    g = G.Golden(name)
    h = _self_stream(g, seed, n)
    own = _to_self(h, _self_addrs(g.tables, h.family == 6))
    a, b = S.take(h, np.flatnonzero(own)), S.take(h, np.flatnonzero(~own))
    return Scenario(g.tables, [Batch(a, g.mode, g.ep_lxc), Batch(b, g.mode, g.ep_lxc)])


def _stale_cut_scenario():
    """2: A is plain egress traffic with two headers to the endpoint's own
    address: one of a protocol conntrack does not know (dropped before any
    CT write) somewhere inside, and an ICMP error as the last header.  Those
    two are the only headers k_self_mark lists, and an ICMP error after any
    listed header is cut (selfcut.hpp), so the one cut is at n - 1:
    cfc_classify folds [0, n - 1) and leaves a record for the last header.
    A is never applied.  A' is A with the two destinations rewritten to a
    plain address, classified into the same tensors, then applied.  The CT
    maps start with the fixture's entries of other address pairs only, so
    the header of A that is never folded hits no entry: a launch counts its
    hits into the entries (cfc.h), the oracle's fold does, and only without
    hits do the two agree on a batch without apply."""
    sc = _self_scenario("self_egress_v4", 5, 12_000)
    t = copy.copy(sc.tables)
    plain = sc.batches[1].h
    # (not empty: without a device CT table no batch is cut)
    def pair(a, b):
        a, b = np.atleast_1d(a).astype(np.uint64), np.atleast_1d(b).astype(np.uint64)
        return np.minimum(a, b) << np.uint64(32) | np.maximum(a, b)
    ea = np.ascontiguousarray(t.ct["tuple"][:, 0:8]).view("<u4").reshape(-1, 2)
    used = np.concatenate([pair(plain.saddr, plain.daddr), pair(S.LXC_IPV4, S.LXC_IPV4)])
    t.ct = t.ct[(t.ct["family"] == 1) & ~np.isin(pair(ea[:, 0], ea[:, 1]), used)]
    assert len(t.ct) >= 16
    mode, ep = sc.batches[1].mode, sc.batches[1].ep_lxc
    n = len(plain)
    me = np.uint32(S.LXC_IPV4)
    a = S.take(plain, np.arange(n))
    a.tcpflags = S.tcp_flags_of(plain).copy()
    for i, (proto, sport) in ((n // 3, (47, 0)), (n - 1, (S.IPPROTO_ICMP, 3))):
        a.saddr[i], a.daddr[i] = me, me
        a.proto[i], a.sport[i], a.dport[i] = proto, sport, 0
        a.flags[i], a.tcpflags[i], a.mark[i] = 0, 0, 0
    a2 = S.take(a, np.arange(n))
    a2.tcpflags = a.tcpflags.copy()
    a2.daddr[[n // 3, n - 1]] = plain.daddr[0]
    return Scenario(t, [Batch(a, mode, ep, folded=n - 1), Batch(a2, mode, ep, into=0)])


def _reuse_cut_scenario():
    """2, the other direction: A' (uncut) classified and never applied, then
    A (cut) in the same tensors, applied"""
    sc = _stale_cut_scenario()
    a, a2 = sc.batches
    return Scenario(sc.tables, [Batch(a2.h, a.mode, a.ep_lxc, folded=0),
                                Batch(a.h, a.mode, a.ep_lxc, into=0)])


def _c5_scenario(mode):
    """3: a reduced headers_c5 stream split by flow (by the remote address:
    every flow and every new header has the endpoint's address on one side)"""
    t, flows = S.config_c5(5, n_flows=20_000, n_prefixes=20_000, n_policy=4000)
    h = S.headers_c5(t, flows, 40_000, seed=33)
    odd = (S.byteswap32(h.saddr) & 1).astype(bool)
    return Scenario(t, [Batch(S.take(h, np.flatnonzero(~odd)), mode),
                        Batch(S.take(h, np.flatnonzero(odd)), mode)])


GROW_FLOWS, GROW_N = 2_000, 80_000


def _grow_scenario():
    """4: as test_gpu_ctgrow — few live flows (a small device table), A with
    enough new flows to take it past 3/4 load, B the other half by address"""
    t, flows = S.config_c5(5, n_flows=GROW_FLOWS, n_prefixes=20_000, n_policy=4000, now=1000)
    t.ct_max_entries = 1 << 20
    h = S.headers_c5_seq(t, flows, GROW_N, seed=23, new_frac=0.5)
    odd = (S.byteswap32(h.saddr) & 1).astype(bool)
    return Scenario(t, [Batch(S.take(h, np.flatnonzero(~odd)), MODE_FULL),
                        Batch(S.take(h, np.flatnonzero(odd)), MODE_FULL)], clock=1003)


def _nat_parts(n=8000):
    """test_gpu_nat's tables and NAT64 egress stream -> (tables, hop headers
    split in two by peer address, plain IPv6 headers without hops)"""
    from test_gpu_nat import nat_tables
    t, ipc4, hist, ok = nat_tables(n_hist=600)
    h = S.headers_nat64(t, ipc4, hist, n)
    o = O.Oracle(t)
    o.set_clock(1003)
    words = o.run_sequential(h, MODE_EGRESS, S.EP_LXC_ID)[3]
    d = np.ascontiguousarray(h.daddr, np.uint8)
    mapped = (d[:, :10] == 0).all(1) & (d[:, 10] == 0xff) & (d[:, 11] == 0xff)
    hop = (words & NATLEN) != 0
    assert not (hop & ~mapped).any()
    peers = np.unique(np.ascontiguousarray(hist.daddr[:, 12:16]).view("<u4"))
    return t, ipc4, h, mapped, peers


def _family_scenario(swap):
    """5: dual-stack tables with both CT maps; an IPv6 egress batch without
    hops (no v4-mapped peer) and an IPv4 ingress batch of new traffic"""
    t, ipc4, h, mapped, peers = _nat_parts()
    rng = np.random.default_rng(71)
    more = S.gen_headers_v6(rng, 3000, t.ipcache[t.ipcache["family"] == 2],
                            S.local_v6_addrs(t), local_frac=0.3, mark_host=0, mark_proxy=0,
                            src_fixed=S.LXC_IPV6, ext=0, exthdr_drop=0)
    b6 = S.concat([S.take(h, np.flatnonzero(~mapped)), more])
    b4 = S.gen_headers_v4(rng, 4000, ipc4, S.local_v4_addrs(t)[:1], local_frac=1.0,
                          mark_host=0, mark_proxy=0, frag=0)
    # (an ICMP packet from a peer of the NAT64 history finds its flow's ICMP
    # entry, which carries nat46, and takes the NAT46 hop: none of those)
    b4 = S.take(b4, np.flatnonzero(~np.isin(b4.saddr, peers)))
    bs = [Batch(b4, MODE_INGRESS, 0), Batch(b6, MODE_EGRESS, S.EP_LXC_ID)]
    return Scenario(t, bs[::-1] if swap else bs, clock=1003)


def _hops_scenario(kind):
    """6: two NAT64 egress batches (v4-mapped peers split by address);
    "plain": B the stream's headers without hops; "reuse": A new NAT64 flows,
    classified (its hops taken) and never applied, then A' — the plain
    headers, as many — classified into A's tensors"""
    t, ipc4, h, mapped, peers = _nat_parts()
    d = np.ascontiguousarray(h.daddr, np.uint8)
    odd = (d[:, 15] & 1).astype(bool)
    ep = S.EP_LXC_ID
    if kind == "two":
        bs = [Batch(S.take(h, np.flatnonzero(mapped & ~odd)), MODE_EGRESS, ep),
              Batch(S.take(h, np.flatnonzero(mapped & odd)), MODE_EGRESS, ep)]
    elif kind == "plain":
        bs = [Batch(S.take(h, np.flatnonzero(mapped)), MODE_EGRESS, ep),
              Batch(S.take(h, np.flatnonzero(~mapped)), MODE_EGRESS, ep)]
    else:
        # (A is never applied: new flows only, which hit no entry — see
        # _stale_cut_scenario)
        p = S.take(h, np.flatnonzero(~mapped))
        a = S.nat64_flows(np.random.default_rng(73), ipc4, 2 * len(p), 30000)
        # (an echo request to a peer of the history finds that flow's ICMP entry)
        a = S.take(a, np.flatnonzero(a.proto != S.IPPROTO_ICMPV6)[:len(p)])
        bs = [Batch(a, MODE_EGRESS, ep, folded=0), Batch(p, MODE_EGRESS, ep, into=0)]
    return Scenario(t, bs, clock=1003)


SCENARIOS = {
    "self_v4": lambda: _self_scenario("self_egress_v4", 5, 12_000),
    "self_v6": lambda: _self_scenario("self_egress_v6", 6, 12_000),
    "stale_cut": _stale_cut_scenario,
    "reuse_cut": _reuse_cut_scenario,
    "c5_mode0": lambda: _c5_scenario(MODE_INGRESS),
    "c5_mode3": lambda: _c5_scenario(MODE_FULL),
    "grow": _grow_scenario,
    "family_46": lambda: _family_scenario(False),
    "family_64": lambda: _family_scenario(True),
    "hops_two": lambda: _hops_scenario("two"),
    "hops_plain": lambda: _hops_scenario("plain"),
    "hops_reuse": lambda: _hops_scenario("reuse"),
}
# scenarios whose batches run one after the other (the same buffers): there
# is one order, so nothing to be independent of
SEQUENTIAL = {"stale_cut", "reuse_cut", "hops_reuse"}


def _hops(sc, i):
    """the oracle's hop count of batch i run on the loaded tables"""
    o = O.Oracle(sc.tables)
    o.set_clock(sc.clock)
    b = sc.batches[i]
    return int(((o.run_sequential(b.h, b.mode, b.ep_lxc)[3] & NATLEN) != 0).sum())


# ---- CPU: the condition and the preconditions (the oracle only) ------------

@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_batches_are_independent(name):
    """Folding a scenario's batches in the listed order and in reverse gives
    the same per-batch outputs, CT maps and counters: they share no CT key,
    so the packet-order fold is what any interleaving must give.  And each
    stream holds what its scenario is about."""
    sc, want, wstate = expected(name)
    for b in sc.batches:
        assert len(b.h) >= 2
    if name not in SEQUENTIAL:
        rev, rstate = fold(sc, order=range(len(sc.batches))[::-1])
        for i in range(len(sc.batches)):
            for k in KEYS:
                np.testing.assert_array_equal(rev[i][k], want[i][k], f"batch {i} {k}")
        np.testing.assert_array_equal(rstate["rows"], wstate["rows"])
        np.testing.assert_array_equal(rstate["metrics"], wstate["metrics"])
        np.testing.assert_array_equal(rstate["identity"], wstate["identity"])
        for lxc, exp in wstate["counters"].items():
            np.testing.assert_array_equal(rstate["counters"][lxc], exp)
    t = sc.tables
    if name.startswith("self_"):
        # A: flows of the endpoint to itself whose answer follows the opening
        # packet (the answer's egress lookup finds the entry the opening
        # packet's ingress stage made: CT_REPLY, conntrack.h:487-494); B: no
        # header the cut rule would list
        a, b = sc.batches
        v6 = a.h.family == 6
        me = np.asarray(S.LXC_IPV6, np.uint8) if v6 else np.uint32(S.LXC_IPV4)
        to_me = (a.h.daddr == me).all(1) if v6 else a.h.daddr == me
        syn = np.flatnonzero(to_me & (S.tcp_flags_of(a.h) == 0x02))
        ans = np.flatnonzero(to_me & (S.tcp_flags_of(a.h) == 0x12))
        first_syn = {(int(a.h.sport[i]), int(a.h.dport[i])): i for i in syn[::-1]}
        after = [j for j in ans
                 if first_syn.get((int(a.h.dport[j]), int(a.h.sport[j])), j) < j]
        assert len(after) > 50, len(after)
        assert ((want[0]["ct"][after] & 3) == 2).sum() > 50   # CFC_CT_REPLY
        assert not _to_self(b.h, _self_addrs(t, v6)).any()
        assert 2000 <= len(a.h) <= 20_000 and len(b.h) >= 500
    for i, (b, w) in enumerate(zip(sc.batches, want)):
        if b.folded is not None:
            # headers classified and never folded hit no entry the maps hold
            # (the launch would count the hit, the oracle's fold did not
            # run): no hit at the first stage, and at the second only an ICMP
            # error's RELATED hit on its own first stage's create, which the
            # launch cannot see — the maps hold no entry with both addresses
            # the endpoint's own when it runs
            c = w["ct"][b.folded:]
            assert not (c & 3).any()
            hit2 = ((c >> 4) & 3) != 0
            if hit2.any():
                assert name == "stale_cut" and len(c) == 1 and (c[0] >> 4) & 3 == 3
                o = O.Oracle(t)
                o.classify(b.h.slice(0, b.folded), b.mode, b.ep_lxc, want_ct=True,
                           apply_ct=True)
                rows = o.ct_dump()
                me = np.frombuffer(np.uint32(S.LXC_IPV4).tobytes(), np.uint8)
                assert not ((rows[:, 4:8] == me).all(1) & (rows[:, 8:12] == me).all(1)).any()
    if name in ("stale_cut", "reuse_cut"):
        a = sc.batches[0 if name == "stale_cut" else 1]
        n = len(a.h)
        # the cut rule's input: the two listed headers, the second an ICMP
        # error — one cut, at n - 1; the other batch lists nothing
        listed = np.flatnonzero(_to_self(a.h, _self_addrs(t, False)))
        assert listed.tolist() == [n // 3, n - 1]
        assert a.h.proto[n - 1] == S.IPPROTO_ICMP and a.h.sport[n - 1] == 3
        other = sc.batches[1 if name == "stale_cut" else 0]
        assert not _to_self(other.h, _self_addrs(t, False)).any()
        w = want[0 if name == "stale_cut" else 1]   # (the cut batch's own fold)
        assert n >= 500 and ((w["ct"] & 0xF) == 0xC).sum() > 100   # creates
        if name == "stale_cut":
            assert a.folded == n - 1
    if name.startswith("c5_"):
        for w in want:
            assert ((w["ct"] & 3) == 1).sum() > 1000     # live flows: ESTABLISHED
            assert ((w["ct"] & 0xF) == 0xC).sum() > 100  # and creates
    if name == "grow":
        # A alone takes the device table past 3/4 load: the table is the
        # least power of two with room for twice the loaded entries, so less
        # than four times them, and its 3/4 less than three times them
        o = O.Oracle(t)
        o.set_clock(sc.clock)
        before = len(o.ct_dump())
        a = sc.batches[0]
        o.classify(a.h, a.mode, a.ep_lxc, want_ct=True, apply_ct=True)
        created = len(o.ct_dump()) - before
        assert before + created > 3 * before, (before, created)
        assert ((want[1]["ct"] & 3) == 1).sum() > 1000   # B hits live entries
    if name.startswith("family_"):
        fams = [b.h.family for b in sc.batches]
        assert sorted(fams) == [4, 6]
        for i in range(2):
            assert _hops(sc, i) == 0
            assert ((want[i]["ct"] & 0xF) == 0xC).sum() > 100
        assert {int(r[3]) for r in wstate["rows"]} >= {1, 2}   # both families' entries
    if name == "hops_two":
        assert _hops(sc, 0) > 500 and _hops(sc, 1) > 500
    if name == "hops_plain":
        assert _hops(sc, 0) > 1000 and _hops(sc, 1) == 0
    if name == "hops_reuse":
        assert _hops(sc, 0) > 300 and _hops(sc, 1) == 0
        assert len(sc.batches[0].h) == len(sc.batches[1].h)


# ---- GPU: the schedules ----------------------------------------------------

PIPELINED = ["cA cB aA aB", "cA cB aB aA"]


@pytest.mark.gpu
@pytest.mark.parametrize("text", PIPELINED)
@pytest.mark.parametrize("name", ["self_v4", "self_v6"])
def test_cut_batch_with_another_launch_between(torch, name, text):
    """1: A was cut for traffic to itself — cfc_classify folded its segments
    before the last — and B is classified before A's apply: the apply folds
    A's last segment only, whichever batch is applied first"""
    st = run_and_check(torch, name, text)
    assert st["ct_self_segments"] >= 2, st


@pytest.mark.gpu
def test_cut_batch_apply_with_other_headers_is_refused(torch):
    """1: an apply that names a cut batch's outputs with other headers (here
    one fewer) is not that batch's: -EINVAL, nothing folded — folded whole,
    its early segments would be folded twice — and the record stays for the
    real apply"""
    st = run_and_check(torch, "self_v4", "cA cB xA aB aA")
    assert st["ct_self_segments"] >= 2, st


@pytest.mark.gpu
def test_stale_cut_record_is_discarded(torch):
    """2: A cut (one cut, at its last header) and never applied, then A'
    without traffic to itself classified into the same tensors and applied:
    A' is folded whole — A's record neither skips its headers [0, n - 1) nor
    survives — after A's first segment and nothing else of A"""
    st = run_and_check(torch, "stale_cut", "cA cB aB")
    assert st["ct_self_segments"] == 1, st


@pytest.mark.gpu
def test_cut_batch_in_reused_buffers(torch):
    """2, the other direction: an uncut batch never applied, then a cut one
    in the same tensors, applied: its last segment alone is left to fold"""
    st = run_and_check(torch, "reuse_cut", "cA cB aB")
    assert st["ct_self_segments"] == 1, st


@pytest.mark.gpu
@pytest.mark.parametrize("text", PIPELINED)
@pytest.mark.parametrize("mode", [MODE_INGRESS, MODE_FULL])
def test_c5_batches_pipelined(torch, mode, text):
    """3: in 'cA cB aA aB' neither apply may use its launch's hit slots (A's
    launch is not the last, and aA moves ct_gen under B's); in 'cA cB aB aA'
    aB takes them and aA probes"""
    st = run_and_check(torch, f"c5_mode{mode}", text)
    assert st["ct_apply_device"] == 2, st


@pytest.mark.gpu
def test_c5_batches_pipelined_on_two_streams(torch):
    """3: each batch's classify and apply on a stream of its own"""
    torch.cuda.synchronize()
    streams = {0: torch.cuda.Stream(), 1: torch.cuda.Stream()}
    st = run_and_check(torch, "c5_mode3", "cA cB aA aB", streams)
    assert st["ct_apply_device"] == 2, st


@pytest.mark.gpu
def test_table_growth_between(torch):
    """4: aA moves the CT table into a larger one on the device; B's hit
    slots, taken in the table as it was, must not be used by aB"""
    st = run_and_check(torch, "grow", "cA cB aA aB")
    assert st["ct_grown"] >= 1, st
    assert st["ct_apply_device"] == 2, st


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["family_46", "family_64"])
def test_other_family_between(torch, name):
    """5: an IPv4 and an IPv6 batch outstanding together, either first"""
    st = run_and_check(torch, name, "cA cB aA aB")
    assert st["nat_hops"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("name,text", [("hops_two", "cA cB aA aB"),
                                       ("hops_plain", "cA cB aA aB"),
                                       ("hops_reuse", "cA cB aB")])
def test_hop_records(torch, name, text):
    """6: two NAT64 hop batches alive at once; a launch without hops between
    a hop batch's classify and its apply; a hop batch never applied whose
    tensors then hold a batch without hops (its record must not be applied
    to that one)"""
    sc = expected(name)[0]
    st = run_and_check(torch, name, text)
    assert st["nat_hops"] == _hops(sc, 0) + _hops(sc, 1), st
