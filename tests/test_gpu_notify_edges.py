"""The monitor-record compaction (csrc/notify.hip k_nt_count / k_nt_scan /
k_nt_write behind cfc_drop_notify_v4/v6 and cfc_monitor_events_v4/v6) at its
structural and field edges.  Every case hands the engine event words,
verdicts and identities the test built itself (notify_edges.py, whose claims
test_notify_edges.py checks on the CPU) and compares the record count, the
header indices and every byte of the records with Oracle.events on the same
numpy arrays — which the CPU suite pins record by record to the reference's
perf ring (test_oracle_golden.py).  Everything is exact.  Run on an MI355X:
pytest -m gpu."""
import ctypes
import errno

import numpy as np
import pytest

import notify_edges as E
import oracle as O
from cilium_amd.datapath import Datapath, Verdicts, hdr_struct, out_struct, pack
from cilium_amd.loader import load_tables
from test_gpu_batch_geometry import misaligned_batch

pytestmark = pytest.mark.gpu
GUARD_ROWS = E.GUARD_ROWS


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


def new_datapath():
    """the catalogue's tables, and one header classified: the records read
    the endpoint table of the epoch a classify call took (-ENOENT before)"""
    dp = Datapath(0)
    load_tables(dp, E.tables())
    dp.classify(pack(E.headers(4, 1, 1)), E.INGRESS, 0)
    return dp


@pytest.fixture(scope="module")
def dp(torch):
    d = new_datapath()
    torch.cuda.synchronize()
    yield d
    d.close()


@pytest.fixture(scope="module")
def oracle():
    return O.Oracle(E.tables())


def want_of(oracle, c, traces):
    rec, idx = oracle.events(c.h, c.mode, c.ep, c.ver, c.ide, c.words, traces=bool(traces))
    return np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 32), idx


def upload(torch, c):
    """-> (device batch, Verdicts holding the case's verdicts, identities and
    event words)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()   # noqa: E731
    return pack(c.h), Verdicts(t(c.ver), t(c.ide), None, None, t(c.words))


def rows_of(rec):
    return np.ascontiguousarray(rec.cpu().numpy()).view(np.uint8).reshape(-1, 32)


def compare(got, want, what=""):
    """(records, indices, total) of the engine against the oracle's"""
    rec, idx, total = got
    wrec, widx = want
    assert total == len(widx), (what, total, len(widx))
    gi = idx.cpu().numpy().astype(np.uint64)
    bad = np.flatnonzero(gi != widx)
    assert len(bad) == 0, (what, "header index", bad[:5], gi[bad[:5]], widx[bad[:5]])
    g = rows_of(rec)
    bad = np.flatnonzero((g != wrec).any(1))
    assert len(bad) == 0, (what, "record", bad[:5], widx[bad[:5]],
                           g[bad[:3]].view("<u4"), wrec[bad[:3]].view("<u4"))


def run(torch, dp, oracle, c, traces, what=""):
    b, out = upload(torch, c)
    fn = dp.monitor_events if traces else dp.drop_notify
    compare(fn(b, out, c.mode, c.ep), want_of(oracle, c, traces), what)


# ------------------------------------------------------ 1: sizes and patterns
@pytest.mark.parametrize("n", E.SIZES)
@pytest.mark.parametrize("family,mode", E.PATTERN_MODES)
def test_patterns(torch, dp, oracle, family, mode, n):
    """nothing, everything, single lanes, one wave of every round, one round
    of every block, the first or last header only and a random third, with
    and without traces, unsent trace words in between"""
    for name in E.PATTERNS:
        for traces in (0, 1):
            run(torch, dp, oracle, E.pattern_case(family, mode, n, name, traces), traces,
                (name, traces))


# ---------------------------------------------------------------- 2: the scan
@pytest.mark.parametrize("traces", [0, 1])
@pytest.mark.parametrize("nb", E.SCAN_NB)
def test_scan(torch, dp, oracle, nb, traces):
    """1024, 1025 and 2049 block counts: one, two and three per thread of
    k_nt_scan, empty and full blocks among uneven ones.  A wrong prefix moves
    every later block's records."""
    c = E.scan_case(nb)
    b, out = upload(torch, c)
    total = int(E.selected(c.words, traces).sum())
    fn = dp.monitor_events if traces else dp.drop_notify
    got = fn(b, out, c.mode, c.ep, cap=total + GUARD_ROWS)
    compare(got, want_of(oracle, c, traces), nb)


# ---------------------------------------------------- 3: cap and the buffers
class Buffers:
    """records, header indices and the count in guarded allocations of the
    test's own, for the C entry points"""

    def __init__(self, torch, rows, off=0):
        self.torch = torch
        self.rec = torch.full((rows + 2, 8), E.GUARD32, dtype=torch.int32, device="cuda")
        self.idx = torch.full((rows + 4,), E.GUARD64, dtype=torch.int64, device="cuda")
        self.cnt = torch.full((4,), E.GUARD64, dtype=torch.int64, device="cuda")
        assert self.rec.data_ptr() % 16 == 0
        self.rows, self.off = rows, off

    def call(self, dp, b, out, c, traces, cap, rec="buf", idx=True, rec_bytes=0, n=None):
        assert 0 <= cap <= self.rows      # (what the engine may write fits)
        v6 = c.family == 6
        fn = ((dp.L.cfc_monitor_events_v6 if v6 else dp.L.cfc_monitor_events_v4) if traces
              else (dp.L.cfc_drop_notify_v6 if v6 else dp.L.cfc_drop_notify_v4))
        o = self.off
        rp = None if rec is None else ctypes.c_void_p(self.rec[1:].data_ptr() + rec_bytes)
        ip = ctypes.c_void_p(self.idx[o:].data_ptr()) if idx else None
        rc = fn(dp.h, ctypes.byref(hdr_struct(b, n)), ctypes.byref(out_struct(out)), c.mode,
                c.ep, rp, ip, cap, ctypes.c_void_p(self.cnt[o:].data_ptr()),
                dp._stream(None))
        self.torch.cuda.synchronize()
        return rc

    def read(self):
        o = self.off
        rec = self.rec.cpu().numpy().view(np.uint8).reshape(-1, 32)
        idx = self.idx.cpu().numpy().view(np.uint64)
        cnt = self.cnt.cpu().numpy().view(np.uint64)
        # the guard rows around the views
        assert (rec[0].view("<u4") == E.GUARD32).all() and \
            (rec[-1].view("<u4") == E.GUARD32).all(), "records: written outside"
        assert (idx[:o] == E.GUARD64).all() and (idx[o + self.rows:] == E.GUARD64).all()
        assert (cnt[:o] == E.GUARD64).all() and (cnt[o + 1:] == E.GUARD64).all()
        return rec[1:-1], idx[o:o + self.rows], int(cnt[o])

    def untouched(self):
        rec, idx, cnt = self.read()
        return (rec.view("<u4") == E.GUARD32).all() and (idx == E.GUARD64).all() and \
            cnt == E.GUARD64


def check_capped(buf, want, cap, T, what, idx=True):
    """rows before min(T, cap) are the oracle's, every row from there on
    still holds the guard pattern, count is the total"""
    rec, gi, cnt = buf.read()
    wrec, widx = want
    m = min(T, cap)
    assert cnt == T == len(widx), (what, cnt, T)
    assert (rec[m:].view("<u4") == E.GUARD32).all(), (what, "records past min(T, cap)")
    bad = np.flatnonzero((rec[:m] != wrec[:m]).any(1))
    assert len(bad) == 0, (what, bad[:5])
    if idx:
        assert (gi[m:] == E.GUARD64).all(), (what, "indices past min(T, cap)")
        np.testing.assert_array_equal(gi[:m], widx[:m], str(what))
    else:
        assert (gi == E.GUARD64).all()


@pytest.mark.parametrize("family", [4, 6])
def test_cap(torch, dp, oracle, family):
    """caps 0, 1, T-1, T, T+1 and +-1 around the record count reached inside
    the first wave, at the end of the first round and of the first block, in
    buffers of cap + 64 guarded rows"""
    for traces in (1, 0):
        c = E.cap_case(family, traces)
        b, out = upload(torch, c)
        caps, T, at = E.caps_of(c, traces)
        want = want_of(oracle, c, traces)
        for cap in caps:
            buf = Buffers(torch, cap + GUARD_ROWS)
            assert buf.call(dp, b, out, c, traces, cap) == 0
            check_capped(buf, want, cap, T, (traces, cap))


@pytest.mark.parametrize("family", [4, 6])
def test_null_buffers_and_empty_batch(torch, dp, oracle, family):
    c = E.cap_case(family)
    b, out = upload(torch, c)
    caps, T, at = E.caps_of(c)
    want = want_of(oracle, c, 1)
    # cap 0 without a records buffer (and without an index buffer): the count
    buf = Buffers(torch, GUARD_ROWS)
    assert buf.call(dp, b, out, c, 1, 0, rec=None) == 0
    check_capped(buf, want, 0, T, "records NULL")
    buf = Buffers(torch, GUARD_ROWS)
    assert buf.call(dp, b, out, c, 1, 0, rec=None, idx=False) == 0
    check_capped(buf, want, 0, T, "both NULL", idx=False)
    # a cap without a records buffer is refused
    buf = Buffers(torch, GUARD_ROWS)
    assert buf.call(dp, b, out, c, 1, 1, rec=None) == -errno.EINVAL and buf.untouched()
    # no index buffer: the same records
    for cap in (T + 1, at[1]):
        buf = Buffers(torch, cap + GUARD_ROWS)
        assert buf.call(dp, b, out, c, 1, cap, idx=False) == 0
        check_capped(buf, want, cap, T, ("hdr_index NULL", cap), idx=False)
    # an empty batch: count 0 over the pattern, nothing else written
    buf = Buffers(torch, T + GUARD_ROWS)
    assert buf.call(dp, b, out, c, 1, T, n=0) == 0
    rec, gi, cnt = buf.read()
    assert cnt == 0 and (rec.view("<u4") == E.GUARD32).all() and (gi == E.GUARD64).all()
    # records 4 and 8 bytes past 16-byte alignment: refused, nothing written
    for nbytes in (4, 8):
        buf = Buffers(torch, T + GUARD_ROWS)
        assert buf.call(dp, b, out, c, 1, T, rec_bytes=nbytes) == -errno.EINVAL
        assert buf.untouched(), nbytes


# ------------------------------------------------------------------ 4: fields
@pytest.mark.parametrize("family,mode", E.FIELD_MODES)
def test_fields(torch, dp, oracle, family, mode):
    """every word shape of the mode at every edge of length, verdict,
    identity and LXC_ID: both length caps, the NAT lengths, 16-bit drop
    labels against 32-bit trace labels, ids without an endpoint"""
    c = E.field_case(family, mode)
    run(torch, dp, oracle, c, 1, "events")
    run(torch, dp, oracle, c, 0, "drops")


# -------------------------------------------------------------------- 5: hash
@pytest.mark.parametrize("family", [4, 6])
def test_skb_hash(torch, dp, oracle, family):
    """the batch's own skb->hash goes into the records verbatim"""
    c = E.skb_hash_case(family)
    b, out = upload(torch, c)
    assert b.hash is not None
    got = dp.monitor_events(b, out, c.mode, c.ep)
    compare(got, want_of(oracle, c, 1))
    np.testing.assert_array_equal(rows_of(got[0]).view(O.EVENT_DT)["hash"].ravel(), c.h.hash)


@pytest.mark.parametrize("family", [4, 6])
def test_flow_hash(torch, dp, oracle, family):
    """CFC_FLOW_HASH against the oracle's, and on the engine's own output: a
    tuple and its reverse carry the same hash"""
    c = E.flow_hash_case(family)
    b, out = upload(torch, c)
    assert b.hash is None
    got = dp.monitor_events(b, out, c.mode, c.ep)
    compare(got, want_of(oracle, c, 1))
    hs = rows_of(got[0]).view(O.EVENT_DT)["hash"].ravel()
    assert len(hs) == len(c)
    np.testing.assert_array_equal(hs[0::2], hs[1::2])
    assert len(np.unique(hs[0::2])) == len(hs) // 2


# -------------------------------------------------------- 6: workspace growth
def test_workspace_grows_between_two_streams(torch, oracle):
    """a fresh Datapath: 100 headers on one stream (the first notify call: a
    one-block workspace), 8 388 609 on another (the workspace grows inside
    the call), 100 on the first again, nothing waited for in between"""
    cases = [E.small_case(0), E.scan_case(2049), E.small_case(1)]
    ups = [upload(torch, c) for c in cases]
    d = new_datapath()
    try:
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        big_total = int(E.selected(cases[1].words, 1).sum())
        res = []
        for c, (b, out), s, cap in zip(cases, ups, (s1, s2, s1), (None, big_total, None)):
            with torch.cuda.stream(s):   # (the result tensors are zeroed on s too)
                res.append(d.monitor_events(b, out, c.mode, c.ep, cap=cap, stream=s,
                                            sync=False))
        torch.cuda.synchronize()
        for k, (c, (rec, idx, cnt)) in enumerate(zip(cases, res)):
            total = int(cnt.item())
            compare((rec[:total], idx[:total], total), want_of(oracle, c, 1), k)
    finally:
        d.close()


# ------------------------------------------------------------------ 7: slices
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("family", [4, 6])
def test_slices(torch, dp, oracle, family, off):
    """inputs, header indices and the count at element offsets 1-3 of larger
    tensors, the records 16-byte aligned between guard rows"""
    c = E.slice_case(family)
    b, out = upload(torch, c)
    b = misaligned_batch(torch, b, off)

    def shifted(x):
        buf = torch.zeros(x.numel() + 8, dtype=x.dtype, device=x.device)
        buf[off:off + x.numel()].copy_(x)
        return buf[off:off + x.numel()]
    out = Verdicts(shifted(out.verdict), shifted(out.identity), None, None,
                   shifted(out.notify))
    assert out.notify.data_ptr() % 16 == 4 * off and b.meta.data_ptr() % 16 == 4 * off
    want = want_of(oracle, c, 1)
    T = len(want[1])
    for cap in (T, T // 2):
        buf = Buffers(torch, cap + GUARD_ROWS, off)
        assert buf.call(dp, b, out, c, 1, cap) == 0
        check_capped(buf, want, cap, T, (off, cap))
