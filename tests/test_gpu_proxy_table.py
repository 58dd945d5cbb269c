"""CFC_OPT_PROXY_APPLY = CFC_PROXY_APPLY_DEVICE on the GPU: the records of a
cfc_proxy_apply_* call translate in the next cfc_classify_from_host_* without
a commit — folded into the family's live table in place (rpapply.hip) or, when
the table cannot take them, by a rebuild from the map.

Expected values never come from the code under test: the expected table is
the host map's dump (Datapath.dump), fed to the composition
revproxy_streams.expect() that the commit path is checked against
(test_gpu_revproxy.py), and every output of every header is compared with that
module's check().  Every from-host batch carries one header per key of the
map (each must hit with its own value), four near misses per key (another
address, source port, destination port, protocol: each must miss) and plain
headers (rp_table.probes; test_proxy_table_opt.py asserts that on the CPU,
with the home slots, clusters and the wrap of the structural key set).
Run on an MI355X: pytest -m gpu."""
import functools

import numpy as np
import pytest

import revproxy_streams as RS
import rp_table as T
from cilium_amd import _lib as L
from cilium_amd import proxymap as PM
from cilium_amd.datapath import Datapath, Verdicts, pack
from cilium_amd.loader import ct_rows, load_tables
from test_gpu_revproxy import check, shifted, u32

pytestmark = pytest.mark.gpu
CLOCK = RS.CLOCK
FAMS = pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
DEVICE = (L.OPT_PROXY_APPLY, L.PROXY_APPLY_DEVICE)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


def fd_of(dp, v6):
    return dp.proxy.fd6 if v6 else dp.proxy.fd4


def dump(dp, v6):
    k, v = dp.dump(fd_of(dp, v6))
    return {bytes(a): bytes(c) for a, c in zip(k, v)}


def open_small(v6, entries=None, device_at_commit=False, max_entries=None):
    """RS.small's tables with `entries` in the family's proxy map, committed;
    then the device option on (device_at_commit: before that commit, so the
    1/4 rule sizes the table)"""
    dp = Datapath(0)
    orig = PM.ProxyMap
    try:
        if max_entries is not None:   # (load_tables opens the maps)
            PM.ProxyMap = functools.partial(orig, max_entries=max_entries)
        load_tables(dp, RS.small(v6), commit=False)
    finally:
        PM.ProxyMap = orig
    dp.set_clock(CLOCK)
    if device_at_commit:
        dp.set_option(*DEVICE)
    for k, v in (entries or {}).items():
        dp.update_element(fd_of(dp, v6), k, v)
    dp.commit()
    dp.set_option(*DEVICE)
    return dp


def apply_raw(torch, dp, h, ver, ide, stream=None):
    """proxy_apply of hand-made outputs (INGRESS, no CT bytes)"""
    out = Verdicts(torch.from_numpy(np.asarray(ver, np.int32)).cuda(),
                   torch.from_numpy(np.asarray(ide, np.uint32).view(np.int32)).cuda(), None)
    b = pack(h)
    torch.cuda.synchronize()
    return dp.proxy_apply(b, out, 0, 0, stream=stream)


def apply_keys(torch, dp, v6, keys, first=0, n=None, at=None, stream=None):
    """a batch redirecting one header per key (values dest(first + i))"""
    recs = [(k, T.dest(v6, first + i)) for i, k in enumerate(keys)]
    h, ver, ide = T.redirect_headers(v6, recs, n, at)
    return apply_raw(torch, dp, h, ver, ide, stream)


def from_host(torch, dp, h, stream=None, b=None):
    """classify_from_host of h -> everything it wrote (test_gpu_revproxy.run's
    dict); stream: queued there, nothing synchronised before the call"""
    if b is None:
        b = pack(h)
        torch.cuda.synchronize()
    if stream is None:
        out, tr = dp.classify_from_host(b, want_ct=True, want_notify=True)
    else:
        with torch.cuda.stream(stream):   # (the outputs are allocated there too)
            out, tr = dp.classify_from_host(b, want_ct=True, want_notify=True, stream=stream)
    torch.cuda.synchronize()
    tb = tr.batch
    return dict(b=b, out=out, tr=tr, ver=out.verdict.cpu().numpy(), ide=u32(out.identity),
                act=out.action.cpu().numpy().astype(np.int32), ct=out.ct.cpu().numpy(),
                words=u32(out.notify),
                saddr=tb.saddr.cpu().numpy().view(np.uint8).reshape(len(h), -1),
                l4=u32(tb.ports), mark=u32(tb.mark), tid=u32(tr.identity),
                hits=int(tr.hits.item()))


OUTPUTS = ("ver", "ide", "act", "ct", "words", "saddr", "l4", "mark", "tid", "hits")


def probe(torch, dp, v6, table, keys=None, extra_miss=(), stream=None):
    """the from-host batch over `keys` (default: the table's) against the
    composition on `table`: the keys of the table hit with their own value,
    everything else misses -> the run"""
    keys = sorted(table) if keys is None else list(keys)
    h, hit, miss = T.probes(v6, keys + list(extra_miss))
    x = RS.expect(RS.small(v6), table, h)
    want = np.zeros(len(h), bool)
    want[[i for i, k in enumerate(keys + list(extra_miss)) if k in table]] = True
    np.testing.assert_array_equal(x.tr.hit, want)
    assert x.extra["unlabelled"]
    r = from_host(torch, dp, h, stream=stream)
    check(r, x)
    return r


def same_outputs(a, b):
    for f in OUTPUTS:
        np.testing.assert_array_equal(a[f], b[f])


# ------------------------------------------------- 1, 2, 9. the round trip
def round_trip(torch, v6, device, off=0, ct=True):
    """test_gpu_revproxy.round_trip_engine without the commit between the
    apply and the from-host batch -> (the stream, the run, the map, stats)"""
    x = RS.round_trip(v6)
    h1, ep = x.extra["h1"], x.extra["ep"]
    dp = Datapath(0)
    load_tables(dp, x.tables)
    dp.set_clock(CLOCK)
    dp.commit()
    if device:
        dp.set_option(*DEVICE)
    try:
        b1 = pack(h1)
        if off:
            b1 = shifted(torch, b1, off)
        out1 = dp.classify(b1, 1, ep, want_ct=True, want_pkt=True)
        if ct:
            dp.ct_apply(b1, out1, 1, ep)
        st = dp.proxy_apply(b1, out1, 1, ep)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out1.verdict.cpu().numpy(), x.extra["ver1"])
        assert st["failed"] == 0 and st["entries"] > 0
        rows = dump(dp, v6)
        r = from_host(torch, dp, x.h)
        if not ct:
            return x, r, rows, dp.proxy_table_stats(v6), dp
        dp.ct_apply(r["tr"].batch, r["out"], 0, 0)
        torch.cuda.synchronize()
        r["ct"] = r["out"].ct.cpu().numpy()
        r["words"] = u32(r["out"].notify)
        rec, idx, total = dp.monitor_events(r["tr"].batch, r["out"], 0, 0)
        r["rec"], r["idx"] = rec.cpu().numpy(), idx.cpu().numpy().astype(np.uint64)
        dp.counters_sync()
        r["ct_rows"] = ct_rows(dp, dp.ct_fds)
        return x, r, rows, dp.proxy_table_stats(v6), None
    except BaseException:
        ct = True
        raise
    finally:
        if ct:
            dp.close()


def check_round_trip(x, r, rows, ts):
    assert rows == x.entries
    check(r, x)
    np.testing.assert_array_equal(r["ct_rows"], x.extra["ct_dump"])
    orec, oidx = x.extra["events"]
    np.testing.assert_array_equal(r["idx"], oidx)
    np.testing.assert_array_equal(np.ascontiguousarray(r["rec"]).view(np.uint8).reshape(-1),
                                  np.ascontiguousarray(orec).view(np.uint8).reshape(-1))
    assert x.tr.hit.sum() >= 600
    assert ts["patched"] + ts["rebuilt"] == 1
    assert ts["entries"] == len(rows) and ts["slots"] == T.slots_for(len(rows), True)


@FAMS
def test_round_trip_without_the_commit(torch, v6):
    """redirect, proxy entries, and the proxy's packets back at once: every
    output, the CT maps and the monitor records as after a commit (what
    fails without the feature: no row would be translated)"""
    x, r, rows, ts, _ = round_trip(torch, v6, device=True)
    check_round_trip(x, r, rows, ts)


@FAMS
def test_ragged_batch(torch, v6):
    x, r, rows, ts, _ = round_trip(torch, v6, device=True, off=3)
    check_round_trip(x, r, rows, ts)


@FAMS
def test_default_option_still_needs_the_commit(torch, v6):
    """option 0: the from-host batch before a commit sees the map as it was
    before the apply (empty: no hit), after it the entries; nothing is
    patched.  (No CT fold here, so that the composition's empty CT maps are
    the engine's.)"""
    x, r, rows, ts, dp = round_trip(torch, v6, device=False, ct=False)
    try:
        assert len(rows) > 0
        before = RS.expect(x.tables, {}, x.h)
        assert not before.tr.hit.any()
        check(r, before)
        assert ts == dict(slots=0, entries=0, patched=0, rebuilt=0, inserted=0, updated=0)
        dp.commit()
        after = RS.expect(x.tables, rows, x.h)
        assert after.tr.hit.sum() >= 100
        check(from_host(torch, dp, x.h), after)
        ts = dp.proxy_table_stats(v6)
        assert ts == dict(slots=T.slots_for(len(rows), False), entries=len(rows), patched=0,
                          rebuilt=0, inserted=0, updated=0)
    finally:
        dp.close()


# -------------------------------------------------------- 3. structural edges
@FAMS
def test_structural_edges(torch, v6):
    """a 128-slot table of 33 entries and one 257-header batch whose records
    are: three new keys of one home slot, a new key homed at the head of a
    cluster of three, one landing behind the 127 -> 0 wrap, an existing key
    two slots from home with a new value, keys differing in the address only
    and in the ports only, and an identical re-write"""
    e = T.edges(v6)
    dp = open_small(v6, e.base)
    try:
        ts0 = dp.proxy_table_stats(v6)
        assert ts0 == dict(slots=128, entries=33, patched=0, rebuilt=0, inserted=0, updated=0)
        probe(torch, dp, v6, e.base, keys=sorted(set(e.base) | set(e.new)))
        h, ver, ide = T.redirect_headers(v6, e.recs, 257, e.at)
        st = apply_raw(torch, dp, h, ver, ide)
        assert st == dict(redirects=10, entries=10, created=8, updated=2, failed=0)
        rows = dump(dp, v6)
        want = dict(e.base)
        want.update(T.records_of(v6, e.recs))
        assert rows == want and len(rows) == 41
        ts = dp.proxy_table_stats(v6)
        assert ts == dict(slots=128, entries=41, patched=1, rebuilt=0, inserted=8, updated=2)
        r1 = probe(torch, dp, v6, rows)
        # the identical batch again: every record overwrites
        st = apply_raw(torch, dp, h, ver, ide)
        assert st == dict(redirects=10, entries=10, created=0, updated=10, failed=0)
        ts = dp.proxy_table_stats(v6)
        assert ts == dict(slots=128, entries=41, patched=2, rebuilt=0, inserted=8, updated=12)
        same_outputs(probe(torch, dp, v6, rows), r1)
        # ... and a table rebuilt from the map gives the same
        epoch = dp.stats()["epoch"]
        dp.delete_element(fd_of(dp, v6), e.shape["wrap"][0])
        dp.update_element(fd_of(dp, v6), e.shape["wrap"][0], rows[e.shape["wrap"][0]])
        dp.commit()
        assert dp.stats()["epoch"] == epoch + 1
        assert dp.proxy_table_stats(v6)["slots"] == T.slots_for(41, True)
        same_outputs(probe(torch, dp, v6, rows), r1)
    finally:
        dp.close()


# ----------------------------------------------------------- 4. load boundary
@FAMS
def test_load_boundary(torch, v6):
    e = T.edges(v6)
    dp = open_small(v6, e.base)
    try:
        extra = T.more_keys(v6, 32, set(e.base))
        for a, b in ((0, 16), (16, 31)):
            st = apply_keys(torch, dp, v6, extra[a:b], first=a)
            assert st["created"] == b - a and st["failed"] == 0
        rows = dump(dp, v6)
        assert len(rows) == 64
        assert dp.proxy_table_stats(v6) == dict(slots=128, entries=64, patched=2, rebuilt=0,
                                                inserted=31, updated=0)
        probe(torch, dp, v6, rows, extra_miss=extra[31:])
        st = apply_keys(torch, dp, v6, extra[31:], first=31)
        assert st["created"] == 1
        rows = dump(dp, v6)
        assert len(rows) == 65 and T.slots_for(65, True) == 512
        assert dp.proxy_table_stats(v6) == dict(slots=512, entries=65, patched=2, rebuilt=1,
                                                inserted=31, updated=0)
        probe(torch, dp, v6, rows)
    finally:
        dp.close()


# ------------------------------------------------------------ 5. no table yet
@FAMS
def test_no_table_yet(torch, v6):
    dp = open_small(v6, {})
    try:
        zero = dict(slots=0, entries=0, patched=0, rebuilt=0, inserted=0, updated=0)
        assert dp.proxy_table_stats(v6) == zero
        h, ver, ide = T.redirect_headers(v6, [], 64)
        st = apply_raw(torch, dp, h, ver, ide)
        assert st == dict(redirects=0, entries=0, created=0, updated=0, failed=0)
        assert dp.proxy_table_stats(v6) == zero
        keys = T.more_keys(v6, 5, set())
        assert apply_keys(torch, dp, v6, keys, n=70, at=[0, 63, 64, 65, 69])["created"] == 5
        rows = dump(dp, v6)
        assert sorted(rows) == sorted(keys)
        assert dp.proxy_table_stats(v6) == dict(slots=T.slots_for(5, True), entries=5, patched=0,
                                                rebuilt=1, inserted=0, updated=0)
        probe(torch, dp, v6, rows)
        # no redirect: nothing patched, the stats stay
        ts = dp.proxy_table_stats(v6)
        assert apply_raw(torch, dp, h, ver, ide)["redirects"] == 0
        assert dp.proxy_table_stats(v6) == ts
        # the other family has no table
        assert dp.proxy_table_stats(not v6) == zero
    finally:
        dp.close()


# ------------------------------------------------------------- 6. refused key
@FAMS
def test_refused_key_never_translates(torch, v6):
    keys = T.more_keys(v6, 6, set())
    held, refused = keys[:5], keys[5]
    base = {k: T.value(v6, *T.dest(v6, 30 + i)) for i, k in enumerate(held)}
    dp = open_small(v6, base, device_at_commit=True, max_entries=5)
    try:
        assert dp.proxy_table_stats(v6)["slots"] == T.slots_for(5, True)
        st = apply_keys(torch, dp, v6, [refused, held[2]], first=90)
        assert st == dict(redirects=2, entries=2, created=0, updated=1, failed=1)
        rows = dump(dp, v6)
        assert sorted(rows) == sorted(held) and rows[held[2]] != base[held[2]]
        assert rows[held[2]] == T.value(v6, *T.dest(v6, 91))
        ts = dp.proxy_table_stats(v6)
        assert (ts["patched"], ts["rebuilt"], ts["entries"]) == (0, 1, 5)
        r = probe(torch, dp, v6, rows, extra_miss=[refused])
        dp.commit()
        same_outputs(probe(torch, dp, v6, rows, extra_miss=[refused]), r)
    finally:
        dp.close()


# ---------------------------------------------------- 7. pending host changes
@FAMS
def test_pending_host_changes_wait_for_the_commit(torch, v6):
    e = T.edges(v6)
    dp = open_small(v6, e.base)
    try:
        fd = fd_of(dp, v6)
        extra = T.more_keys(v6, 6, set(e.base))
        gone, added = e.shape["cluster"][1], extra[0]
        dp.delete_element(fd, gone)
        dp.update_element(fd, added, T.value(v6, *T.dest(v6, 40)))
        assert apply_keys(torch, dp, v6, extra[1:4], first=50)["created"] == 3
        ts = dp.proxy_table_stats(v6)
        assert (ts["slots"], ts["entries"], ts["patched"], ts["rebuilt"]) == (128, 36, 1, 0)
        rows = dump(dp, v6)
        assert gone not in rows and added in rows and len(rows) == 36
        # the table: the batch's keys in, the deleted key still in, the added
        # key not yet
        table = {k: v for k, v in rows.items() if k != added}
        table[gone] = e.base[gone]
        probe(torch, dp, v6, table, extra_miss=[added])
        # the signature was left stale: the commit rebuilds
        epoch = dp.stats()["epoch"]
        dp.commit()
        assert dp.stats()["epoch"] == epoch + 1
        ts = dp.proxy_table_stats(v6)
        assert (ts["slots"], ts["entries"]) == (T.slots_for(36, True), 36)
        assert (ts["patched"], ts["rebuilt"]) == (1, 0)
        probe(torch, dp, v6, rows, extra_miss=[gone])
        # nothing pending: a patch keeps the table's signature current, and
        # the next commit has nothing to rebuild
        assert apply_keys(torch, dp, v6, extra[4:6], first=70)["created"] == 2
        assert dp.proxy_table_stats(v6)["patched"] == 2
        rows = dump(dp, v6)
        r = probe(torch, dp, v6, rows, extra_miss=[gone])
        epoch = dp.stats()["epoch"]
        dp.commit()
        assert dp.stats()["epoch"] == epoch
        same_outputs(probe(torch, dp, v6, rows, extra_miss=[gone]), r)
    finally:
        dp.close()


# ----------------------------------------------------------- 8. another stream
@FAMS
def test_apply_and_lookup_on_different_streams(torch, v6):
    e = T.edges(v6)
    dp = open_small(v6, e.base)
    try:
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        want = dict(e.base)
        want.update(T.records_of(v6, e.recs))
        ph, hit, miss = T.probes(v6, sorted(want))
        x = RS.expect(RS.small(v6), want, ph)
        assert x.tr.hit[hit].all() and not x.tr.hit[miss].any()
        pb = pack(ph)
        h, ver, ide = T.redirect_headers(v6, e.recs, 257, e.at)
        st = apply_raw(torch, dp, h, ver, ide, stream=sa)     # (inputs ready: synchronised)
        r = from_host(torch, dp, ph, stream=sb, b=pb)
        assert st["created"] == 8 and dump(dp, v6) == want
        assert dp.proxy_table_stats(v6)["patched"] == 1
        check(r, x)
    finally:
        dp.close()
