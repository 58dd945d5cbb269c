"""Streams of the CT accounting edge tests (test_gpu_ct_acct_edges.py) and
the batch geometry tests (test_gpu_batch_geometry.py), built with numpy and
the oracle alone: test_ct_edge_streams.py checks on the CPU that each holds
what it is about, the GPU files run them through the engine."""
import copy

import numpy as np

import golden_io as G
import oracle as O
from cilium_amd import synth as S

CLOCK = 1003            # the tables' flows were created at 1000
N_HOT = 70_000          # two accounting slices: 64 512 + 5 488 headers
SLICE = 63 * 1024       # kern_common.hpp COUNT_PER_BLOCK
LDS_SLOTS = 8192        # classify.hip CT_LDS_SLOTS
LENGTHS = np.array([0, 1, 59, 1500, 65534, 65535], np.uint16)
ACK, PSH_ACK, SYN_ACK, FIN_ACK = 0x10, 0x18, 0x12, 0x11
ESTABLISHED, REPLY = 1 | 4, 2 | 4   # CT byte, low nibble (cfc.h CFC_CT_DONE)
SMALL = dict(n_flows=2_000, n_prefixes=2_000, n_policy=512, now=1000)
# the ragged schedule of the geometry tests: every unit the passes work in
# (4, 16, 64, 1024, 4096 headers) missed by one on either side
SIZES = [1, 2, 3, 5, 63, 64, 65, 255, 1023, 1025, 4099, 16_385, 20_001]

_cache = {}


def tables(family=4, n_flows=2_000):
    """(tables, flows) of the C5 shape at test size; built once per size"""
    key = (family, n_flows)
    if key not in _cache:
        kw = dict(SMALL, n_flows=n_flows)
        _cache[key] = S.config_c5(5, **kw) if family == 4 else S.config_c5_v6(6, **kw)
    return _cache[key]


def _draw(t, flows, n, **kw):
    fn = S.headers_c5 if flows.family == 4 else S.headers_c5_v6
    return fn(t, flows, n, new_frac=0.0, s=0.0, **kw)


def hot_header(t, flows, mode, want):
    """One forwarded TCP header of a live flow whose CT byte is `want`
    (ESTABLISHED or REPLY), picked with the oracle -> a 1-header batch"""
    h = _draw(t, flows, 4000)
    o = O.Oracle(t)
    o.set_clock(CLOCK)
    _, ver, _, ct = o.classify(h, mode, 0, nthreads=8, want_ct=True)
    ok = (h.proto == S.IPPROTO_TCP) & (ver == 0) & ((ct & 0xF) == want)
    assert ok.any(), "no such header"
    return S.take(h, np.flatnonzero(ok)[:1])


def repeat(one, n, length=65535, tcpflags=ACK):
    """the 1-header batch `one` n times at the given length"""
    b = S.take(one, np.zeros(n, np.int64))
    b.length = np.full(n, length, np.uint16)
    b.flags = b.flags.copy()
    b.tcpflags = np.full(n, tcpflags, np.uint8)
    return b


def hot_batch(t, flows, mode, want, n=N_HOT):
    return repeat(hot_header(t, flows, mode, want), n)


def wide_batch(t, flows, n=SLICE, seed=5):
    """n headers drawn evenly from the live flows, each at length 65535, TCP
    flags ACK / PSH|ACK / SYN|ACK (no FIN, no RST): far more distinct keys
    than the slice's LDS table takes in three probes"""
    h = _draw(t, flows, n, seed=seed)
    rng = np.random.default_rng(seed + 31)
    h.length = np.full(n, 65535, np.uint16)
    tf = rng.choice(np.array([ACK, PSH_ACK, SYN_ACK], np.uint8), size=n)
    h.tcpflags = np.where(h.proto == S.IPPROTO_TCP, tf, 0).astype(np.uint8)
    h.flags = (h.flags & np.uint8(0xFF ^ S.HF_TCP_CLOSE)).astype(np.uint8)
    return h


def flow_keys(h):
    """one u64-pair row per header: equal rows, equal 5-tuple (IPv4)"""
    return np.stack([h.saddr.astype(np.uint64) << 32 | h.daddr,
                     h.sport.astype(np.uint64) << 32 | h.dport.astype(np.uint64) << 16 |
                     h.proto], 1)


def mixed_batch(t, flows, mode, n=N_HOT, seed=9):
    """half the headers the hot flow, half the wide draw, lengths from both
    ends of the byte field; about 1 % of the hot flow's packets carry FIN"""
    rng = np.random.default_rng(seed)
    one = hot_header(t, flows, mode, ESTABLISHED)
    hot = repeat(one, n)
    fin = rng.random(n) < 0.01
    hot.tcpflags[fin] = FIN_ACK
    hot.flags[fin] |= np.uint8(S.HF_TCP_CLOSE)
    wide = wide_batch(t, flows, n, seed=seed)
    is_hot = rng.random(n) < 0.5
    h = S.take(S.concat([hot, wide]), np.where(is_hot, 0, n) + np.arange(n))
    h.length = LENGTHS[rng.integers(0, len(LENGTHS), size=n)]
    return h, is_hot, one


def acct(rows):
    """(n, 4) u64 {rx_packets, rx_bytes, tx_packets, tx_bytes} of CT rows"""
    return np.ascontiguousarray(rows[:, 44:76]).view("<u8").reshape(-1, 4)


def hot_delta(t, batches, mode, ep_lxc=0):
    """The oracle over the batches in packet order -> (rows that changed,
    their accounting before, after): CT rows compared by key"""
    o = O.Oracle(t)
    o.set_clock(CLOCK)
    before = o.ct_dump()
    for b in batches:
        o.run_sequential(b, mode, ep_lxc)
    after = o.ct_dump()
    assert before.shape == after.shape and (before[:, :44] == after[:, :44]).all()
    ch = np.flatnonzero((before != after).any(1))
    return ch, acct(before[ch]), acct(after[ch])


def egress_second_stage(name="self_egress_v4"):
    """An egress fixture's tables with the CT state its stream leaves, and a
    forwarded TCP header of that stream that now hits in both stages (the
    sender's lookup and the local destination's), its destination another
    endpoint than the sender -> (tables, mode, ep_lxc, 1-header batch)"""
    g = G.Golden(name)
    t = copy.copy(g.tables)
    h = copy.copy(g.headers)
    h.hash = None
    o = O.Oracle(t)
    o.set_clock(CLOCK)
    o.run_sequential(h, g.mode, g.ep_lxc)
    t.ct = S.ct_from_rows(o.ct_dump())
    o = O.Oracle(t)
    o.set_clock(CLOCK)
    _, ver, _, ct = o.classify(h, g.mode, g.ep_lxc, nthreads=8, want_ct=True)
    hit = lambda x: ((x & 3) != 0) & ((x & 3) != 3) & ((x & 0xC) == 4)   # noqa: E731
    ok = hit(ct) & hit(ct >> 4) & (ver == 0) & (h.proto == S.IPPROTO_TCP) & \
        (h.daddr != h.saddr) & (h.daddr != S.LXC_IPV4)
    assert ok.any(), "no header that hits in both stages"
    return t, g.mode, g.ep_lxc, S.take(h, np.flatnonzero(ok)[:1])


# ---------------------------------------------------------------- geometry
def ragged_stream(kind):
    """(tables, headers, mode, ep_lxc, notify) of a geometry case: sum(SIZES)
    headers with multi-packet new flows, closes and denied live flows"""
    n = sum(SIZES)
    if kind in ("v4_full", "v4_ingress"):
        t, flows = tables(4, 20_000)
        h = S.headers_c5_seq(t, flows, 45_000, seed=23).slice(0, n)
        return (t, h, 3, 0, False) if kind == "v4_full" else (t, h, 0, 0, True)
    if kind == "v4_egress":   # local delivery: the receiver's CT map as well
        g = G.Golden("ct_seq_egress_v4")
        rng = np.random.default_rng(29)
        reps = (n + len(g.headers) - 1) // len(g.headers)
        h = S.concat([g.headers] * reps)
        # each copy keeps the fixture's packet order; the copies interleave
        pos = np.concatenate([np.sort(rng.random(len(g.headers))) for _ in range(reps)])
        h = S.take(h, np.argsort(pos, kind="stable")).slice(0, n)
        h.hash = None
        return g.tables, h, g.mode, g.ep_lxc, True
    assert kind == "v6_full"
    t, flows = tables(6, 20_000)
    m = n * 4 // 5
    h, new = S.headers_c5_v6(t, flows, m, seed=27, new_frac=0.1, return_new=True)
    rng = np.random.default_rng(27)
    tf = rng.choice(np.array([ACK, PSH_ACK], np.uint8), size=m)
    tf[new] = 0x02
    close = ~new & (rng.random(m) < 0.02)
    tf[close] = FIN_ACK
    h.flags = h.flags.copy()
    h.flags[close & (h.proto == S.IPPROTO_TCP)] |= np.uint8(S.HF_TCP_CLOSE)
    h.tcpflags = np.where(h.proto == S.IPPROTO_TCP, tf, 0).astype(np.uint8)
    # later packets of the new flows (and of some live ones), after their first
    more = np.concatenate([np.flatnonzero(new), rng.integers(0, m, size=n)])[:n - m]
    h2 = S.take(h, more)
    h2.tcpflags = np.where(h2.proto == S.IPPROTO_TCP, ACK, 0).astype(np.uint8)
    h2.flags = (h2.flags & np.uint8(0xFF ^ S.HF_TCP_CLOSE)).astype(np.uint8)
    pos = np.concatenate([np.arange(m, dtype=np.float64),
                          more + rng.random(n - m) * (m - more)])
    h = S.take(S.concat([h, h2]), np.argsort(pos, kind="stable"))
    return t, h, 3, 0, True


def cuts(sizes=SIZES):
    """[(a, b)] of the consecutive batches"""
    a = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(a[i]), int(a[i + 1])) for i in range(len(sizes))]


def unpacked_policy_tables():
    """more than 65 535 policy entries in all: bare-index histogram keys"""
    t = S.config_c2(14, n_prefixes=2000, n_policy=16, n_endpoints=5)
    rng = np.random.default_rng(14)
    pol = S.gen_policy(rng, 13_200, np.unique(t.ipcache["label"]))
    t.policy = {lxc: pol for lxc in t.policy}
    return t, S.headers_c2(t, 20_003, seed=14)
