"""The conntrack packet-order pass (csrc/ctorder.hip, and the fold of
ctapply.hip that replays its results) at its chain and structural edges.
The random dependency streams of test_gpu_ctorder.py give each flow one
verdict; here one CT key gets two (ct_order_edges.py: an allowed header A
and a denied header D on the same key), so a batch holds

* mixed slots — a live key with an allowed ESTABLISHED stage and a
  DROP_POLICY stage (k_ord_mixed, k_ord_collect_mix, the branch of
  k_ord_write that adds a plain hit to the work bits), delete-only slots
  (k_ord_deltail), keys the batch creates and deletes again;
* the related round's orders: an ICMP error before the create, one that
  creates, two creates sharing a related key, an error after the delete;
* egress with local delivery (two stages per header) and IPv6 with the
  reverse NAT of k_ord_pkt6;
* chain members on either side of every unit the passes work in (ORD_IT,
  a work-bits word, a block step, k_ord_list_w's LISTW words, the last
  header), 1500 deletes and re-creates of one slot, a fold past FOLD_LONG;
* the host-side fallbacks of ord_resolve_t: ORD_SETFULL, the participant
  list outgrown, the dense filter re-mark.

Every stream runs through classify + cfc_ct_apply against
Oracle.run_sequential: per-header action, verdict, identity and CT byte,
event words and monitor records where notify is on, every CT row, policy,
metrics and identity counters, ct_apply_host == 0 — all exact, no header
excused (test_gpu_ctorder.check).  ct_order_changed counts the stages whose
existence result the pass changed (k_ord_write: NEW <-> ESTABLISHED of a
participant; k_ord_deltail: the later deletes of a delete-only slot); the
create bit follows the result, so it equals the stages whose CT nibble
differs between the oracle's batch-start classify and its sequential run,
and is asserted equal.

Left out: the PSTAGE = 2048 overflow of the collect's LDS stage (batches
beyond two million participants).  Streams: ct_order_edges.py
(preconditions: test_ct_order_edges.py).  Run on an MI355X: pytest -m gpu."""
import functools

import numpy as np
import pytest

import ct_order_edges as C
import oracle as O
from cilium_amd import metricsmap
from cilium_amd import synth as S
from cilium_amd.datapath import Datapath, pack
from cilium_amd.loader import ct_rows, load_tables, policy_rows
from test_gpu_batch_geometry import GuardedOut, misaligned_batch
from test_gpu_ctorder import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


@pytest.fixture(params=["sparse", "dense"])
def passes(request, monkeypatch):
    """the apply's passes: sparse where eligible, or CFC_DENSE_APPLY"""
    if request.param == "dense":
        monkeypatch.setenv("CFC_DENSE_APPLY", "1")
    return request.param


def run_batches(torch, t, h, bounds, mode, ep=0, notify=True, off=None, want_pkt=False):
    """the engine over the stream cut at `bounds` into consecutive batches
    on one Datapath (classify, cfc_ct_apply, monitor records; the shape of
    test_gpu_ctorder.run_both) -> the dict check compares, and the stats
    after every batch.  off: the batch's arrays and the output arrays at
    that element offset of larger allocations (test_gpu_batch_geometry:
    misaligned_batch, GuardedOut) — the ordering pass takes its load path
    and the byte shift of its CT-byte atomics from the outputs' alignment
    (ctorder.hip O.vec) — and nothing outside the output views written"""
    dp = Datapath(0)
    try:
        pms = load_tables(dp, t)
        dp.set_clock(C.CLOCK)
        whole = pack(h)
        g = {k: [] for k in ("act", "ver", "ide", "ct", "nt", "rec", "idx", "pkt")}
        each = [dp.stats()]
        for a, b in zip(bounds[:-1], bounds[1:]):
            sub = whole.slice(a, b)
            if off is not None:
                sub = misaligned_batch(torch, sub, off)
            kw = dict(want_pkt=True) if want_pkt else {}
            go = None
            if off is not None:
                go = GuardedOut(torch, b - a, off, notify, whole.ports.device)
                kw["out"] = go.out
                assert go.out.ct.data_ptr() % 16 == off % 16
                assert go.out.verdict.data_ptr() % 16 == (4 * off) % 16
            out = dp.classify(sub, mode, ep, want_ct=True, want_notify=notify, **kw)
            assert go is None or out is go.out
            dp.ct_apply(sub, out, mode, ep)
            if notify:
                rec, idx, total = dp.monitor_events(sub, out, mode, ep)
            torch.cuda.synchronize()
            if go is not None:
                go.intact()
            g["act"].append(out.action.cpu().numpy())
            g["ver"].append(out.verdict.cpu().numpy())
            g["ide"].append(out.identity.cpu().numpy().view(np.uint32))
            g["ct"].append(out.ct.cpu().numpy())
            if notify:
                g["nt"].append(out.notify.cpu().numpy().view(np.uint32))
                g["rec"].append(np.ascontiguousarray(rec.cpu().numpy()).view(O.EVENT_DT)
                                .reshape(-1))
                g["idx"].append(idx.cpu().numpy().astype(np.uint64) + a)
            if want_pkt:
                g["pkt"].append(out.pkt.cpu().numpy().view(np.uint32))
            each.append(dp.stats())
        g = {k: np.concatenate(v) for k, v in g.items() if v}
        dp.counters_sync()
        g["counters"] = {lxc: np.array(policy_rows(pm), np.uint64).reshape(-1, 7)
                         for lxc, pm in pms.items()}
        g["metrics"] = np.array(metricsmap.dump_rows(dp), np.uint64).reshape(-1, 4)
        g["identity"] = dp.identity_counters()
        g["rows"] = ct_rows(dp, dp.ct_fds)
        g["stats"] = dp.stats()
        g["each"] = each
    finally:
        dp.close()
    return g


def check_stream(st, g, want):
    """check, a differing CT row named by its chain first"""
    if g["rows"].shape != want["rows"].shape or (g["rows"] != want["rows"]).any():
        C.explain_rows(st, g["rows"], want["rows"])
    check(g, want)


def delta(g, name):
    """the stat's gain per batch"""
    return [int(b[name] - a[name]) for a, b in zip(g["each"][:-1], g["each"][1:])]


@functools.lru_cache(maxsize=None)
def expected(maker, *args, want_pkt=False):
    """(stream, the oracle's sequential run over it): computed once, shared
    by the run variants, never written to"""
    st = maker(*args)
    w = C.sequential(st.t, st.h, st.mode, st.ep, want_pkt=want_pkt)
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    b = bounds_of(st)
    w["changed"] = C.order_changed(st.t, [st.h.slice(x, y) for x, y in zip(b[:-1], b[1:])],
                                   st.mode, st.ep)
    return st, w


def bounds_of(st):
    return [0, len(st.h)] if st.split is None else [0, st.split, len(st.h)]


def run_variant(torch, st, want, notify, passes, off=None, want_pkt=False):
    """one stream one way; besides check: the apply's passes as asked, and
    ct_order_changed the oracle's count, batch by batch"""
    bounds = bounds_of(st)
    g = run_batches(torch, st.t, st.h, bounds, st.mode, st.ep, notify=notify, off=off,
                    want_pkt=want_pkt)
    print("sparse", delta(g, "ct_apply_sparse"), "changed", delta(g, "ct_order_changed"),
          want["changed"])
    check_stream(st, g, want)
    sparse = delta(g, "ct_apply_sparse")
    if passes == "dense" or notify or getattr(st.t, "lb6", None) is not None:
        assert sum(sparse) == 0, g["stats"]    # (a service step: the dense passes)
    else:
        assert all(s == 1 for s in sparse[1:]), (sparse, g["stats"])
    assert min(want["changed"]) > 0
    assert delta(g, "ct_order_changed") == want["changed"], g["stats"]
    return g


# ------------------------------------------------------------------ chains
@pytest.mark.parametrize("notify", [True, False], ids=["notify", "quiet"])
@pytest.mark.parametrize("cut", [False, True], ids=["one_batch", "cut"])
@pytest.mark.parametrize("mode", [0, 3], ids=["ingress", "full"])
@pytest.mark.parametrize("family", [4, 6])
def test_two_verdict_chains(torch, passes, family, mode, cut, notify):
    """Every chain of the catalogue (ct_order_edges.LIVE, FRESH) on many
    keys at once: mixed slots, delete-only slots, keys created and deleted
    in the batch.  cut: over two batches, every cut position inside every
    chain, the predecessor then comes from the table."""
    st, want = expected(C.chain_stream, family, mode, cut)
    run_variant(torch, st, want, notify, passes)


@pytest.mark.parametrize("notify", [True, False], ids=["notify", "quiet"])
@pytest.mark.parametrize("cut", [False, True], ids=["one_batch", "cut"])
@pytest.mark.parametrize("mode", [0, 3], ids=["ingress", "full"])
@pytest.mark.parametrize("family", [4, 6])
def test_related_round(torch, passes, family, mode, cut, notify):
    """Round 2's key comparisons (ct_order_edges.RELATED) on address pairs
    without any entry: an ICMP error before the create (allowed: it creates
    its own entry; dropped), after it, after the UDP entry's delete, behind
    two creates sharing the related key, a denied error deleting the related
    entry, an echo request as the creating flow, and a TCP create, whose
    related entry the error must not find.  IPv6: ICMPv6 types 1 to 4."""
    st, want = expected(C.related_stream, family, mode, cut)
    run_variant(torch, st, want, notify, passes)


@pytest.mark.parametrize("notify", [True, False], ids=["notify", "quiet"])
@pytest.mark.parametrize("cut", [False, True], ids=["one_batch", "cut"])
def test_egress_local_delivery(torch, passes, cut, notify):
    """Two stages per header (TWO = true): a new flow three times (creates
    in both stages, then ESTABLISHED in both), a chain whose stage-1 key is
    mixed while its stage-0 key is only hit, a header dropped at stage 0.
    The destination is another endpoint than the sender: no batch is cut."""
    st, want = expected(C.egress_stream, cut)
    assert st.mode == 1
    g = run_variant(torch, st, want, notify, passes)
    assert g["stats"]["ct_self_segments"] == g["each"][0]["ct_self_segments"], g["stats"]


@pytest.mark.parametrize("notify", [True, False], ids=["notify", "quiet"])
@pytest.mark.parametrize("cut", [False, True], ids=["one_batch", "cut"])
@pytest.mark.parametrize("mode", [0, 3], ids=["ingress", "full"])
def test_ipv6_reverse_nat_follows_the_order(torch, passes, mode, cut, notify):
    """IPv6 tables with services and want_pkt (k_ord_pkt6): the later
    packets of a flow the batch creates are reverse-NATed by the index the
    create stored; the packet after a delete is not translated."""
    st, want = expected(C.lb6_stream, mode, cut, want_pkt=True)
    g = run_variant(torch, st, want, notify, passes, want_pkt=True)
    bad = np.flatnonzero((g["pkt"] != want["pkt"]).any(1))
    assert len(bad) == 0, f"pkt: {len(bad)} differ, first {bad[:6]}"


# --------------------------------------------------------------- pipelined
@pytest.mark.parametrize("maker", [C.chain_stream, C.related_stream],
                         ids=["chains", "related"])
@pytest.mark.parametrize("mode", [0, 3], ids=["ingress", "full"])
@pytest.mark.parametrize("family", [4, 6])
def test_pipelined_applies(torch, passes, family, mode, maker):
    """classify A, classify B, apply A, apply B, the two batches without an
    address pair in common: A's apply no longer follows its classify launch,
    so its stages' start slots come from probes (start_slot's find) and its
    creates carry no miss tags (pre-keys)."""
    import test_gpu_interleave as I
    a, b = C.split_by_address(maker(family, mode))
    sc = I.Scenario(a.t, [I.Batch(a.h, mode), I.Batch(b.h, mode)], clock=C.CLOCK)
    want, wstate = I.fold(sc)
    got, state = I.run_schedule(torch, sc, I.schedule("cA cB aA aB"))
    both = C.Stream(a.t, S.concat([a.h, b.h]), mode, 0, a.chains,
                    np.concatenate([a.chain, b.chain]), np.concatenate([a.key, b.key]),
                    np.concatenate([a.member, b.member]))
    if state["rows"].shape != wstate["rows"].shape or (state["rows"] != wstate["rows"]).any():
        C.explain_rows(both, state["rows"], wstate["rows"])
    I.check(sc, got, state, want, wstate, [0, 1])
    assert state["stats"]["ct_apply_host"] == 0, state["stats"]
    # (the halves share no key: the oracle's counts of one after the other)
    changed = C.order_changed(a.t, [a.h, b.h], mode)
    assert min(changed) > 0
    assert state["stats"]["ct_order_changed"] == sum(changed), (state["stats"], changed)


# ------------------------------------------------------ structural placements
@pytest.mark.parametrize("notify", [True, False], ids=["notify", "quiet"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off_by_one"])
def test_structural_placements(torch, passes, off, notify):
    """66 003 headers, almost all plain hits; single chains astride header
    15|16 (a thread's run of ORD_IT), 63|64 (a work-bits word), 4095|4096
    (a block step of mark and collect), 65 535|65 536 (k_ord_list_w's block
    of LISTW words) and ending at the final header (n % 16 == 3); the input
    and output arrays 16-byte aligned (ctorder.hip O.vec: the vector loads,
    CT-byte atomics at shifts 0 and 4) and one element off (the scalar loads,
    the atomics at the other bytes of their words), guard elements around
    every output array intact."""
    st, want = expected(C.structural_stream, 4, 3)
    run_variant(torch, st, want, notify, passes, off=off)


@pytest.mark.parametrize("notify", [True, False], ids=["notify", "quiet"])
def test_long_chains(torch, passes, notify):
    """One live key through 3000 alternating allowed and denied stages (the
    fold deletes and re-creates one slot 1500 times), one new key with a
    create and 1999 counted hits (no start slot; past FOLD_LONG = 512)."""
    st, want = expected(C.long_stream, 4, 3)
    run_variant(torch, st, want, notify, passes)


# -------------------------------------------------------- host-side fallbacks
@functools.lru_cache(maxsize=None)
def fallback_expected(kind):
    f = C.fallback(kind)
    w = C.sequential(f.t, f.h, f.mode)
    w["changed"] = C.order_changed(f.t, f.batches, f.mode)
    return f, w


def run_fallback(torch, kind):
    f, want = fallback_expected(kind)
    g = run_batches(torch, f.t, f.h, f.bounds(), f.mode, notify=False)
    print(kind, "sparse", delta(g, "ct_apply_sparse"), "changed", delta(g, "ct_order_changed"),
          want["changed"])
    check(g, want)
    assert delta(g, "ct_order_changed") == want["changed"], g["stats"]
    return f, g


def test_fallback_key_sets_overflow(torch):
    """70 000 distinct new flows in one quiet batch behind a batch of 8
    creates: the key sets, sized by that batch at 65 536 words, cannot hold
    them (ORD_SETFULL) and the batch takes the dense passes; the ordinary
    batch after it is sparse again."""
    assert C.N_SETFULL > C.set_words(C.FIRST_CREATES) == 65_536
    f, g = run_fallback(torch, "setfull")
    assert delta(g, "ct_apply_sparse")[1:] == [0, 1], g["each"]
    assert sum(delta(g, "ct_grown")) == 0, g["each"]   # (not a grown table's second apply)


def test_fallback_participant_list_outgrown(torch):
    """35 000 new flows, each twice: 70 000 participants against room for
    65 536 + 2 * the last count; the collect runs again and the batch stays
    sparse.  That the collect ran twice is not observed (no counter tells):
    it rests on the arithmetic ct_order_edges restates from ord_resolve_t,
    the list's 65 536 words after the first batch among it; observed are
    the results, the sparse apply and that the table did not grow."""
    assert 2 * C.N_TWICE > C.part_room(65_536, C.FIRST_CREATES)
    assert C.N_TWICE < C.set_words(C.FIRST_CREATES)
    f, g = run_fallback(torch, "twice")
    assert sum(delta(g, "ct_grown")) == 0, g["each"]
    assert delta(g, "ct_apply_sparse")[1:] == [1, 1], g["each"]


def test_fallback_dense_remark(torch, monkeypatch):
    """CFC_DENSE_APPLY, the first batch of a fresh context with 5000
    creates: more than 4 x the 1024 words of a filter sized from nothing, so
    the mark runs again; dropped CT_NEW stages before and after the create
    on 500 of the keys.  The second mark is pinned by that arithmetic, not
    observed: the results and the dense apply are."""
    monkeypatch.setenv("CFC_DENSE_APPLY", "1")
    assert C.dense_remark(C.N_REMARK, C.filter_words(0))
    f, g = run_fallback(torch, "remark")
    assert sum(delta(g, "ct_apply_sparse")) == 0, g["each"]
