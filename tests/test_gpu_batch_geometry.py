"""Batch geometry: header and output arrays at every 4-byte (u32) and 1-byte
(u8) offset the ABI admits — the scalar paths behind the 16-byte alignment
guards of k_acc_agg, k_hist, the apply's scan and the ordering passes — and
a ragged schedule of batch sizes on either side of every unit the passes work
in (4, 16, 64, 1024, 4096 headers).  One dependency stream cut into those
batches on one Datapath (classify, cfc_ct_apply, monitor records) against
one sequential run of the oracle over the whole stream: per-header outputs,
event words, records, CT rows, counters; the guard elements around every
output array stay untouched.  Streams: ct_edge_streams.py (preconditions:
test_ct_edge_streams.py).  Run on an MI355X: pytest -m gpu."""
import dataclasses

import numpy as np
import pytest

import ct_edge_streams as E
import oracle as O
from cilium_amd import metricsmap
from cilium_amd.datapath import Datapath, Verdicts, pack
from cilium_amd.loader import ct_rows, load_tables, policy_rows
from test_gpu_ctorder import check

pytestmark = pytest.mark.gpu

PAD = 16                # guard elements on both sides of a view (a multiple of 16 bytes)
GUARD32, GUARD8 = 0x5A5A5A5A, 0xA5
# (inputs' offset, outputs' offset): together, and each side alone — the
# guards of k_acc_agg / k_hist (meta, tcp_flags), the apply's scan and the
# ordering passes depend on different arrays
GEOMETRY = [(0, 0), (1, 1), (2, 2), (3, 3), (1, 0), (0, 1)]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


def _view(torch, x, off):
    """a copy of the 1-D tensor x that starts at element `off` of a larger
    allocation (u32 arrays: 4 * off bytes past 16-byte alignment; byte
    arrays: off bytes)"""
    buf = torch.empty(x.numel() + 2 * PAD, dtype=x.dtype, device=x.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[PAD + off:PAD + off + x.numel()]
    v.copy_(x)
    return v


def misaligned_batch(torch, b, off):
    """the packed batch copied into views at element `off` (0: 16-byte
    aligned, which a slice of a larger batch is not); IPv6 address rows stay
    16-byte aligned (include/cfc.h)"""
    kw = {}
    for f in dataclasses.fields(b):
        x = getattr(b, f.name)
        if x is not None and x.dim() == 1:
            x = _view(torch, x, off)
            assert x.data_ptr() % 16 == (off * x.element_size()) % 16
        kw[f.name] = x
    return type(b)(**kw)


class GuardedOut:
    """Verdicts whose arrays are views at element `off` of allocations
    filled with a guard pattern; intact() after the calls: nothing outside
    the views was written"""

    def __init__(self, torch, n, off, notify, device):
        self.bufs = []

        def arr(dtype, guard):
            buf = torch.full((n + 2 * PAD,), guard, dtype=dtype, device=device)
            self.bufs.append((buf, PAD + off, n, guard))
            return buf[PAD + off:PAD + off + n]
        self.out = Verdicts(arr(torch.int32, GUARD32), arr(torch.int32, GUARD32),
                            arr(torch.uint8, GUARD8), arr(torch.uint8, GUARD8),
                            arr(torch.int32, GUARD32) if notify else None)

    def intact(self):
        for buf, off, n, guard in self.bufs:
            b = buf.cpu().numpy()
            outside = np.concatenate([b[:off], b[off + n:]])
            assert (outside == np.asarray(guard).astype(b.dtype)).all(), \
                (b.dtype, off, n, np.flatnonzero(outside != np.asarray(guard).astype(b.dtype)))


def run_schedule(torch, t, h, mode, ep_lxc, notify, off_in, off_out, sizes=E.SIZES):
    """the engine over the stream cut into consecutive batches of `sizes`,
    and the oracle one header at a time over the whole stream (the shapes
    test_gpu_ctorder.check compares)"""
    dp = Datapath(0)
    try:
        pms = load_tables(dp, t)
        dp.set_clock(E.CLOCK)
        whole = pack(h)
        g = {k: [] for k in ("act", "ver", "ide", "ct", "nt", "rec", "idx")}
        for a, b in E.cuts(sizes):
            sub = misaligned_batch(torch, whole.slice(a, b), off_in)
            go = GuardedOut(torch, b - a, off_out, notify, whole.ports.device)
            out = dp.classify(sub, mode, ep_lxc, out=go.out, want_ct=True, want_notify=notify)
            assert out is go.out
            dp.ct_apply(sub, out, mode, ep_lxc)
            if notify:
                rec, idx, total = dp.monitor_events(sub, out, mode, ep_lxc)
            torch.cuda.synchronize()
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
        g = {k: np.concatenate(v) for k, v in g.items() if v}
        dp.counters_sync()
        g["counters"] = {lxc: np.array(policy_rows(pm), np.uint64).reshape(-1, 7)
                         for lxc, pm in pms.items()}
        g["metrics"] = np.array(metricsmap.dump_rows(dp), np.uint64).reshape(-1, 4)
        g["identity"] = dp.identity_counters()
        g["rows"] = ct_rows(dp, dp.ct_fds)
        g["stats"] = dp.stats()
    finally:
        dp.close()
    return g


_want = {}


def oracle_run(kind):
    """the stream and the oracle's sequential run over it, computed once"""
    if kind not in _want:
        t, h, mode, ep, notify = E.ragged_stream(kind)
        o = O.Oracle(t)
        o.set_clock(E.CLOCK)
        act, ver, ide, words, ct = o.run_sequential(h, mode, ep, want_ct=True)
        rec, idx = o.events(h, mode, ep, ver, ide, words)
        _want[kind] = (t, h, mode, ep, notify,
                       dict(act=act, ver=ver, ide=ide, ct=ct, nt=words, rec=rec, idx=idx,
                            rows=o.ct_dump(), metrics=o.metrics(),
                            identity=o.identity_counters(),
                            counters={lxc: o.policy_counters(lxc) for lxc in t.policy}))
    return _want[kind]


KINDS = ["v4_full", "v4_ingress", "v4_egress", "v6_full"]


@pytest.mark.parametrize("off_in,off_out", GEOMETRY,
                         ids=[f"in{a}_out{b}" for a, b in GEOMETRY])
@pytest.mark.parametrize("kind", KINDS)
def test_ragged_schedule(torch, kind, off_in, off_out):
    """IPv4 FULL without event words (the sparse-eligible apply), IPv4
    INGRESS with monitor records, IPv4 EGRESS with local delivery, IPv6
    FULL: batches of 1 ... 20 001 headers at each array offset."""
    t, h, mode, ep, notify, want = oracle_run(kind)
    g = run_schedule(torch, t, h, mode, ep, notify, off_in, off_out)
    check(g, want)
    if kind == "v4_full" and off_in == 0:
        assert g["stats"]["ct_apply_sparse"] >= 1, g["stats"]


@pytest.mark.parametrize("kind", KINDS)
def test_ragged_schedule_dense_apply(torch, kind, monkeypatch):
    """the same with the apply's dense passes forced (CFC_DENSE_APPLY)"""
    monkeypatch.setenv("CFC_DENSE_APPLY", "1")
    t, h, mode, ep, notify, want = oracle_run(kind)
    g = run_schedule(torch, t, h, mode, ep, notify, 1, 1)
    check(g, want)
    assert g["stats"]["ct_apply_sparse"] == 0, g["stats"]


@pytest.mark.parametrize("off", [1, 2, 3])
def test_unpacked_hist_keys_misaligned_meta(torch, off):
    """More than 65 535 policy entries (bare-index keys, the length taken
    from the header meta) with meta off 16-byte alignment: k_hist's
    !packed && !meta16 branch, n = 20 003.  Every counter against the oracle."""
    from cilium_amd.datapath import pack_v4
    t, h = E.unpacked_policy_tables()
    assert sum(len(p) for p in t.policy.values()) > 65535 and len(h) == 20_003
    dp = Datapath(0)
    try:
        pms = load_tables(dp, t)
        b = misaligned_batch(torch, pack_v4(h), off)
        assert b.meta.data_ptr() % 16 == 4 * off
        go = GuardedOut(torch, len(h), off, False, b.meta.device)
        go.out.ct = None
        out = dp.classify(b, 0, 0, out=go.out)
        torch.cuda.synchronize()
        go.intact()
        ver = out.verdict.cpu().numpy()
        dp.counters_sync()
        pol = {lxc: np.array(policy_rows(pm), np.uint64).reshape(-1, 7)
               for lxc, pm in pms.items()}
        met = np.array(metricsmap.dump_rows(dp), np.uint64).reshape(-1, 4)
        ide = dp.identity_counters()
    finally:
        dp.close()
    o = O.Oracle(t)
    np.testing.assert_array_equal(ver, o.classify(h, 0, 0, nthreads=16)[1])
    for lxc in t.policy:
        np.testing.assert_array_equal(pol[lxc], o.policy_counters(lxc))
    np.testing.assert_array_equal(met, o.metrics())
    np.testing.assert_array_equal(ide, o.identity_counters())
