"""cfc_proxy_entries_v4/v6 and cfc_proxy_apply_v4/v6 on the GPU against the
restatement of the reference's proxy-map writes (proxy_entries.py), whose
inputs are the oracle's outputs.  Streams: proxy_streams.py (their
preconditions: test_proxymap.py).  Every stream test first asserts that the
engine's verdict, identity and CT byte equal the oracle's, then compares the
records, or the dumped map, byte for byte.

The structural tests call the entry kernels on hand-made outputs (the calls
read a batch's outputs as they stand), so each batch is tiny and its keys are
placed exactly: sizes around the wave, the emit group and the mark kernel's
slice (4096 headers), odd element offsets, the LDS table's 1024 slots and its
probe limit, the global table at exactly half load.
Run on an MI355X: pytest -m gpu."""
import dataclasses
import errno

import numpy as np
import pytest

import golden_io as G
import proxy_entries as P
import proxy_streams as PS
from cilium_amd import _lib as L
from cilium_amd import proxymap as PM
from cilium_amd import synth as S
from cilium_amd.datapath import Datapath, Verdicts, pack
from cilium_amd.loader import load_tables

pytestmark = pytest.mark.gpu

SLICE = 4096            # proxymap.hip PX_SLICE
PAD = 16
CLOCK = PS.CLOCK
PORT = int(S.htons(10001))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


def _bytes(rec):
    return np.ascontiguousarray(rec.cpu().numpy()).view(np.uint8)   # (m, 32 | 64)


def _check_records(got, want):
    rec, idx, total = got
    wrec, widx, st = want
    assert total == len(wrec)
    np.testing.assert_array_equal(idx.cpu().numpy().astype(np.uint64), widx)
    np.testing.assert_array_equal(_bytes(rec), wrec)


# ---- streams through classify + ct_apply -------------------------------------

def run_stream(torch, t, batches, outs, last):
    """the batches through classify + ct_apply on one Datapath, each checked
    against the oracle's outputs; `last(dp, batch, out, mode, ep)` on the
    last one -> its result"""
    dp = Datapath(0)
    try:
        load_tables(dp, t)
        dp.set_clock(CLOCK)
        for k, ((h, mode, ep), (act, ver, ide, ct, pkt)) in enumerate(zip(batches, outs)):
            b = pack(h)
            out = dp.classify(b, mode, ep, want_ct=True, want_pkt=mode == 1)
            dp.ct_apply(b, out, mode, ep)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out.verdict.cpu().numpy(), ver)
            np.testing.assert_array_equal(out.identity.cpu().numpy().view(np.uint32), ide)
            np.testing.assert_array_equal(out.ct.cpu().numpy(), ct)
            if mode == 1:
                np.testing.assert_array_equal(out.pkt.cpu().numpy().view(np.uint32), pkt)
            if k == len(batches) - 1:
                return last(dp, b, out, mode, ep)
    finally:
        dp.close()


def _entries(dp, b, out, mode, ep):
    return dp.proxy_entries(b, out, mode, ep)


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
@pytest.mark.parametrize("kind", ["ingress", "egress", "dest"])
def test_stream_records(torch, kind, v6):
    """ingress (NEW / ESTABLISHED, keys rewritten many times), egress after a
    seeding ingress batch (NEW, ESTABLISHED and unreversed REPLY tuples), and
    egress redirected by the destination's stage"""
    t, batches, outs, want = PS.want(kind, v6)
    st = want[2]
    if kind == "ingress":
        assert st["redirects"] >= 1000 and st["rewrites"] >= 500, st
    elif kind == "egress":
        assert min(st["new"], st["established"], st["reply"]) >= 200, st
    else:
        assert st["redirects"] >= 1000 and st["dest_stage"] == st["redirects"], st
    _check_records(run_stream(torch, t, batches, outs, _entries), want)


def test_service_translated_egress(torch):
    """orig_daddr / orig_dport are the backend's (the oracle's want_pkt); a
    looped-back flow keeps the service address"""
    t, h, mode, ep = PS.lb_tables()
    batches = [(h, mode, ep)]
    outs = PS.oracle_run(t, batches)
    act, ver, ide, ct, pkt = outs[0]
    want = P.expected_entries(h, mode, ver, ide, ct, pkt, seclabel=t.seclabel[ep], now=CLOCK)
    assert want[2]["translated"] >= 32, want[2]
    _check_records(run_stream(torch, t, batches, outs, _entries), want)

    def no_pkt(dp, b, out, mode, ep):
        out.pkt = None
        with pytest.raises(L.CfcError) as e:
            dp.proxy_entries(b, out, mode, ep)
        return e.value.errno
    # the service maps hold entries: the packet outputs are needed
    assert run_stream(torch, t, batches, outs, no_pkt) == errno.EINVAL


@pytest.mark.parametrize("name", sorted(["edge_ingress_v4", "edge_ingress_v6",
                                         "ct_seq_ingress_v4", "c2_ingress_v4",
                                         "c3_ingress_v6"]))
def test_fixture_maps(torch, name):
    """the reference fixtures with redirected headers through classify +
    ct_apply + proxy_apply: the dumped map against the restatement"""
    g = G.Golden(name)
    t = g.tables
    if t.ct is None:
        t.ct = np.zeros(0, S.CT_DT)
    batches = [(g.headers, g.mode, g.ep_lxc)]
    outs = PS.oracle_run(t, batches)
    act, ver, ide, ct, pkt = outs[0]
    want = P.expected_entries(g.headers, g.mode, ver, ide, ct, pkt, now=CLOCK)
    assert want[2]["redirects"] == int((g.verdict > 0).sum()) > 0

    def apply(dp, b, out, mode, ep):
        st = dp.proxy_apply(b, out, mode, ep)
        k, v = dp.dump(dp.proxy.fd6 if g.headers.family == 6 else dp.proxy.fd4)
        return st, {bytes(a): bytes(c) for a, c in zip(k, v)}
    st, rows = run_stream(torch, t, batches, outs, apply)
    assert rows == P.map_rows(want[0])
    assert st == dict(redirects=want[2]["redirects"], entries=len(want[0]),
                      created=len(want[0]), updated=0, failed=0)


# ---- hand-made outputs ---------------------------------------------------------

@pytest.fixture(scope="module")
def rawdp(torch):
    dp = Datapath(0)
    dp.proxy = PM.ProxyMap(dp)
    dp.set_clock(CLOCK)
    dp.endpoint_config(7, 4242)
    yield dp
    dp.close()


def raw_headers(keys, v6=False, seed=0):
    """one TCP header per element of `keys`: the key's source address and
    port come from keys[i] (equal numbers: equal proxy-map keys), the
    destination varies (so a key's writers carry different values)"""
    rng = np.random.default_rng(seed)
    keys = np.asarray(keys, np.uint32)
    n = len(keys)
    if v6:
        sa = np.zeros((n, 16), np.uint8)
        sa[:, 0] = 0xfd
        sa[:, 8:12] = (keys >> 4).astype(">u4").view(np.uint8).reshape(n, 4)
        da = np.zeros((n, 16), np.uint8)
        da[:, 0], da[:, 15] = 0xfc, rng.integers(1, 9, size=n)
        da[:, 12:14] = 0x01, 0x65          # reverse-NAT bits (bpf_lxc.c:789)
    else:
        sa = ((keys >> 4) + np.uint32(0x0A000000)).astype(">u4").view("<u4")
        da = (np.uint32(0x0B000000) + rng.integers(1, 9, size=n).astype(np.uint32)) \
            .astype(">u4").view("<u4")
    sp = S.htons(1024 + (keys & 15))
    dp = S.htons(rng.choice(np.array([80, 8080, 443]), size=n))
    return S.Headers(6 if v6 else 4, sa, da, sp, dp, np.full(n, 6, np.uint8),
                     np.zeros(n, np.uint8), np.full(n, 100, np.uint16), np.zeros(n, np.uint32))


def _view(torch, x, off):
    """a copy of 1-D x at element `off` of a larger allocation"""
    buf = torch.zeros(x.numel() + 2 * PAD, dtype=x.dtype, device=x.device)
    v = buf[PAD + off:PAD + off + x.numel()]
    v.copy_(x)
    return v


def run_raw(torch, dp, h, ver, ide=None, ct=None, pkt=None, mode=0, ep=0, cap=None, off=0):
    """proxy_entries on hand-made outputs (arrays at element offset `off`)"""
    n = len(h)
    dev = "cuda"
    ide = np.zeros(n, np.uint32) if ide is None else ide
    b = pack(h)
    tv = torch.from_numpy(np.asarray(ver, np.int32)).to(dev)
    ti = torch.from_numpy(np.asarray(ide, np.uint32).view(np.int32)).to(dev)
    tc = None if ct is None else torch.from_numpy(np.asarray(ct, np.uint8)).to(dev)
    if off:
        kw = {}
        for f in dataclasses.fields(b):
            x = getattr(b, f.name)
            kw[f.name] = _view(torch, x, off) if x is not None and x.dim() == 1 else x
        b = type(b)(**kw)
        tv, ti = _view(torch, tv, off), _view(torch, ti, off)
        tc = None if tc is None else _view(torch, tc, off)
        assert tv.data_ptr() % 16 == (4 * off) % 16
    out = Verdicts(tv, ti, None, tc, None)
    if pkt is not None:
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(pkt, np.uint32).view(np.int32)))
        if h.family == 6:   # saddr rows, daddr rows, L4 words
            out.pkt_raw = torch.cat([p[:, 0:4].reshape(-1), p[:, 4:8].reshape(-1),
                                     p[:, 8].reshape(-1)]).to(dev)
        else:
            out.pkt = p.t().contiguous().to(dev).t()
    return dp.proxy_entries(b, out, mode, ep, cap=cap)


def _raw_case(n, seed, nkeys=64, frac=0.5):
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, max(nkeys, 1), size=n)
    ver = np.where(rng.random(n) < frac, PORT, rng.choice(np.array([0, -133]), size=n))
    ide = rng.integers(256, 70000, size=n).astype(np.uint32)
    ct = (rng.integers(0, 2, size=n) | 4).astype(np.uint8)   # NEW / ESTABLISHED, looked up
    return keys, ver.astype(np.int32), ide, ct


SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 1]


@pytest.mark.parametrize("n", SIZES)
def test_sizes(torch, rawdp, n):
    keys, ver, ide, ct = _raw_case(n, 100 + n)
    h = raw_headers(keys, seed=n)
    _check_records(run_raw(torch, rawdp, h, ver, ide, ct),
                   P.expected_entries(h, 0, ver, ide, ct, now=CLOCK))


@pytest.mark.parametrize("n", [65, SLICE + 1])
def test_sizes_v6(torch, rawdp, n):
    keys, ver, ide, ct = _raw_case(n, 300 + n)
    h = raw_headers(keys, v6=True, seed=n)
    _check_records(run_raw(torch, rawdp, h, ver, ide, ct),
                   P.expected_entries(h, 0, ver, ide, ct, now=CLOCK))


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("n", [67, SLICE + 5])
def test_odd_element_offsets(torch, rawdp, n, off):
    """arrays that start 4, 8, 12 bytes past 16-byte alignment (a slice of a
    larger batch): the scalar verdict loads"""
    keys, ver, ide, ct = _raw_case(n, 200 + n + off)
    h = raw_headers(keys, seed=n)
    _check_records(run_raw(torch, rawdp, h, ver, ide, ct, off=off),
                   P.expected_entries(h, 0, ver, ide, ct, now=CLOCK))


def test_none_and_all_redirected(torch, rawdp):
    n = SLICE + 77
    keys, ver, ide, ct = _raw_case(n, 7, frac=0.0)
    h = raw_headers(keys)
    rec, idx, total = run_raw(torch, rawdp, h, ver, ide, ct)
    assert total == 0 and len(rec) == 0
    keys, ver, ide, ct = _raw_case(n, 8, frac=1.0)
    assert (ver > 0).all()
    _check_records(run_raw(torch, rawdp, h, ver, ide, ct),
                   P.expected_entries(h, 0, ver, ide, ct, now=CLOCK))


@pytest.mark.parametrize("predup", [True, False], ids=["predup", "bypass"])
def test_one_key_every_header(torch, rawdp, monkeypatch, predup):
    """the record carries the last header's value and index"""
    if not predup:
        monkeypatch.setenv("CFC_PROXY_NO_PREDUP", "1")
    n = 2 * SLICE + 1
    keys, ver, ide, ct = _raw_case(n, 9, nkeys=1, frac=1.0)
    h = raw_headers(keys)
    got = run_raw(torch, rawdp, h, ver, ide, ct)
    want = P.expected_entries(h, 0, ver, ide, ct, now=CLOCK)
    assert len(want[0]) == 1 and want[1][0] == n - 1
    _check_records(got, want)


def test_last_writer_across_workgroups(torch, rawdp):
    """key A in every slice (its last writer in the last workgroup); key B
    many times in the first slice only, while the other workgroups hold A;
    key C late in the first slice and early in the last: the header index
    decides, not the position within a slice"""
    n = 3 * SLICE
    keys = 1000 + np.arange(n)               # distinct filler keys
    ver = np.zeros(n, np.int32)
    for s in range(3):
        ver[s * SLICE + np.array([5, 700, 3000])] = PORT
        keys[s * SLICE + np.array([5, 700, 3000])] = 1        # A
    keys[[9, 1500, 4000]] = 2                                  # B
    ver[[9, 1500, 4000]] = PORT
    keys[[4090, 2 * SLICE + 3]] = 3                            # C
    ver[[4090, 2 * SLICE + 3]] = PORT
    ide = np.arange(n, dtype=np.uint32) + 256
    ct = np.full(n, 4, np.uint8)
    h = raw_headers(keys)
    want = P.expected_entries(h, 0, ver, ide, ct, now=CLOCK)
    assert want[1].tolist() == [4000, 2 * SLICE + 3, 2 * SLICE + 3000]
    _check_records(run_raw(torch, rawdp, h, ver, ide, ct), want)


@pytest.mark.parametrize("distinct", [900, 1024, 3000])
def test_more_keys_than_the_lds_table(torch, rawdp, distinct):
    """one slice with 900 keys (some past the LDS probe limit), exactly as
    many keys as LDS slots, and three times as many: the overflow goes to the
    global table directly, and every key still gets its last writer"""
    n = SLICE
    rng = np.random.default_rng(distinct)
    keys = np.concatenate([np.arange(distinct), rng.integers(0, distinct, size=n - distinct)])
    keys = keys[rng.permutation(n)]
    ver = np.full(n, PORT, np.int32)
    ide = np.arange(n, dtype=np.uint32) + 256
    ct = np.full(n, 4, np.uint8)
    h = raw_headers(keys)
    want = P.expected_entries(h, 0, ver, ide, ct, now=CLOCK)
    assert len(want[0]) == distinct
    _check_records(run_raw(torch, rawdp, h, ver, ide, ct), want)


@pytest.mark.parametrize("distinct", [512, 2048])
def test_distinct_keys_at_a_power_of_two(torch, rawdp, distinct):
    """every redirect its own key, a power of two of them: the global table
    (a power of two at least twice the redirects) is exactly half full"""
    n = distinct + 300
    keys = np.arange(n)
    ver = np.zeros(n, np.int32)
    ver[np.random.default_rng(distinct).permutation(n)[:distinct]] = PORT
    ide = np.arange(n, dtype=np.uint32) + 256
    ct = np.full(n, 4, np.uint8)
    h = raw_headers(keys)
    want = P.expected_entries(h, 0, ver, ide, ct, now=CLOCK)
    assert len(want[0]) == distinct
    _check_records(run_raw(torch, rawdp, h, ver, ide, ct), want)


@pytest.mark.parametrize("cap", [0, 1, 17])
def test_cap_below_total(torch, rawdp, cap):
    """*count is still the total, the first cap records are the same"""
    n = 1500
    keys, ver, ide, ct = _raw_case(n, 11)
    h = raw_headers(keys)
    wrec, widx, st = P.expected_entries(h, 0, ver, ide, ct, now=CLOCK)
    assert len(wrec) > 17
    rec, idx, total = run_raw(torch, rawdp, h, ver, ide, ct, cap=cap)
    assert total == len(wrec) and len(rec) == cap
    np.testing.assert_array_equal(_bytes(rec), wrec[:cap])
    np.testing.assert_array_equal(idx.cpu().numpy().astype(np.uint64), widx[:cap])


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_every_orientation_on_hand_made_egress(torch, rawdp, v6):
    """an EGRESS batch whose CT bytes take every state in both stages and
    whose packet outputs differ from the headers in some rows (a translated
    destination, a rewritten source): every branch of the entry against the
    restatement"""
    n = 3000
    rng = np.random.default_rng(77 + v6)
    keys = rng.integers(0, 200, size=n)
    h = raw_headers(keys, v6=v6, seed=5)
    ver = np.where(rng.random(n) < 0.7, PORT, 0).astype(np.int32)
    lo = (rng.integers(0, 4, size=n) | 4).astype(np.uint8)
    hi = np.where(rng.random(n) < 0.4, rng.integers(0, 2, size=n) | 4, 0).astype(np.uint8)
    ct = (lo | hi << 4).astype(np.uint8)
    w = h.sport.astype(np.uint32) | h.dport.astype(np.uint32) << 16
    if v6:
        pkt = np.concatenate([np.ascontiguousarray(h.saddr).view("<u4").reshape(n, 4),
                              np.ascontiguousarray(h.daddr).view("<u4").reshape(n, 4),
                              w.reshape(n, 1)], 1).astype(np.uint32)
        tr = rng.random(n) < 0.3
        pkt[tr, 4] ^= 0x00010000             # another destination
        pkt[tr, 8] = (pkt[tr, 8] & 0xFFFF) | (int(S.htons(9090)) << 16)
        bits = rng.random(n) < 0.2
        pkt[bits, 7] &= 0xFFFF0000           # ipv6_policy cleared the reverse-NAT bits
    else:
        pkt = np.stack([h.saddr, h.daddr, w], 1).astype(np.uint32)
        tr = rng.random(n) < 0.3
        pkt[tr, 1] ^= 0x01000000
        pkt[tr, 2] = (pkt[tr, 2] & 0xFFFF) | (int(S.htons(9090)) << 16)
        src = rng.random(n) < 0.2
        pkt[src, 0] = S.IPV4_LOOPBACK
    want = P.expected_entries(h, 1, ver, None, ct, pkt, seclabel=4242, now=CLOCK)
    assert min(want[2][k] for k in ("new", "established", "reply", "related")) > 50
    assert want[2]["dest_stage"] > 100 and want[2]["translated"] > 100
    _check_records(run_raw(torch, rawdp, h, ver, None, ct, pkt=pkt, mode=1, ep=7), want)


def test_argument_errors(torch, rawdp):
    keys, ver, ide, ct = _raw_case(100, 3)
    h = raw_headers(keys)
    with pytest.raises(L.CfcError) as e:     # EGRESS needs the CT bytes
        run_raw(torch, rawdp, h, ver, ide, None, mode=1, ep=7)
    assert e.value.errno == errno.EINVAL
    dp = Datapath(0)
    try:                                      # the family's map is not open
        with pytest.raises(L.CfcError) as e:
            run_raw(torch, dp, h, ver, ide, ct)
        assert e.value.errno == errno.ENOENT
    finally:
        dp.close()


# ---- the pre-dedup switch, the apply, the map ----------------------------------

def test_predup_switch_same_records(torch, monkeypatch):
    """both settings of CFC_PROXY_NO_PREDUP on the ingress stream"""
    t, batches, outs, want = PS.want("ingress", False)
    a = run_stream(torch, t, batches, outs, _entries)
    monkeypatch.setenv("CFC_PROXY_NO_PREDUP", "1")
    b = run_stream(torch, t, batches, outs, _entries)
    _check_records(a, want)
    _check_records(b, want)


def test_apply_twice_refreshes_lifetimes(torch):
    t, batches, outs, want = PS.want("ingress", False)
    m = len(want[0])

    def twice(dp, b, out, mode, ep):
        st1 = dp.proxy_apply(b, out, mode, ep)
        rows1 = dict(zip(*[[bytes(x) for x in a] for a in dp.dump(dp.proxy.fd4)]))
        dp.set_clock(CLOCK + 50)
        st2 = dp.proxy_apply(b, out, mode, ep)
        rows2 = dict(zip(*[[bytes(x) for x in a] for a in dp.dump(dp.proxy.fd4)]))
        # gc at the first lifetime + 1: nothing of the refreshed map expires
        gone = dp.proxy.gc(CLOCK + 720 + 1)
        return st1, rows1, st2, rows2, gone
    st1, rows1, st2, rows2, gone = run_stream(torch, t, batches, outs, twice)
    red = want[2]["redirects"]
    assert st1 == dict(redirects=red, entries=m, created=m, updated=0, failed=0)
    assert st2 == dict(redirects=red, entries=m, created=0, updated=m, failed=0)
    assert rows1 == P.map_rows(want[0])
    later = want[0].copy()
    later[:, 28:32] = np.frombuffer(np.uint32(CLOCK + 50 + 720).tobytes(), np.uint8)
    assert rows2 == P.map_rows(later)
    assert gone == 0


def test_gc_after_set_clock(torch):
    """entries written at two clocks: gc deletes exactly the expired ones"""
    t, batches, outs, want = PS.want("ingress", False)
    h, mode, ep = batches[-1]
    half = len(h) - 512       # (some keys' writers all sit before the cut)
    act, ver, ide, ct, pkt = outs[-1]
    first = P.expected_entries(h.slice(0, half), mode, ver[:half], ide[:half], ct[:half],
                               now=CLOCK)
    second = P.expected_entries(h.slice(half, len(h)), mode, ver[half:], ide[half:], ct[half:],
                                now=CLOCK + 100)

    def run(dp, b, out, mode, ep):
        sl = lambda o, a, z: Verdicts(o.verdict[a:z], o.identity[a:z], None, o.ct[a:z])  # noqa
        dp.proxy_apply(b.slice(0, half), sl(out, 0, half), mode, ep)
        dp.set_clock(CLOCK + 100)
        dp.proxy_apply(b.slice(half, len(h)), sl(out, half, len(h)), mode, ep)
        gone = dp.proxy.gc(CLOCK + 720 + 1)     # the first clock's lifetimes are < this
        return gone, dict(zip(*[[bytes(x) for x in a] for a in dp.dump(dp.proxy.fd4)]))
    gone, rows = run_stream(torch, t, batches, outs, run)
    keep = P.map_rows(second[0])
    only_first = set(P.map_rows(first[0])) - set(keep)
    assert len(only_first) > 0 and gone == len(only_first)
    assert rows == keep


def test_max_entries_8(torch, rawdp):
    """a full map refuses new keys (failed), holds the first 8 records' keys,
    and still updates the keys it holds"""
    dp = Datapath(0)
    try:
        dp.proxy = PM.ProxyMap(dp, max_entries=8)
        dp.set_clock(CLOCK)
        n = 600
        keys, ver, ide, ct = _raw_case(n, 21, nkeys=40, frac=0.8)
        h = raw_headers(keys)
        wrec, widx, wst = P.expected_entries(h, 0, ver, ide, ct, now=CLOCK)
        m = len(wrec)
        assert m > 8
        b = pack(h)
        out = Verdicts(torch.from_numpy(ver).cuda(), torch.from_numpy(ide.view(np.int32)).cuda(),
                       None, torch.from_numpy(ct).cuda())
        st = dp.proxy_apply(b, out, 0, 0)
        assert st == dict(redirects=wst["redirects"], entries=m, created=8, updated=0,
                          failed=m - 8)
        rows = dict(zip(*[[bytes(x) for x in a] for a in dp.dump(dp.proxy.fd4)]))
        assert rows == P.map_rows(wrec[:8])
        dp.set_clock(CLOCK + 9)
        st = dp.proxy_apply(b, out, 0, 0)
        assert st == dict(redirects=wst["redirects"], entries=m, created=0, updated=8,
                          failed=m - 8)
        later = wrec[:8].copy()
        later[:, 28:32] = np.frombuffer(np.uint32(CLOCK + 9 + 720).tobytes(), np.uint8)
        rows = dict(zip(*[[bytes(x) for x in a] for a in dp.dump(dp.proxy.fd4)]))
        assert rows == P.map_rows(later)
    finally:
        dp.close()
