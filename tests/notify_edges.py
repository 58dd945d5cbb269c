"""Event words and header batches that put the monitor-record compaction
(csrc/notify.hip k_nt_count / k_nt_scan / k_nt_write behind
cfc_drop_notify_v4/v6 and cfc_monitor_events_v4/v6) at its structural and
field edges, built with numpy alone.  The entry points take the event words,
verdicts and identities as plain device arrays and Oracle.events takes the
same as numpy arrays, so no classify call stands between a case and the code
under test: test_notify_edges.py checks on the CPU that every case holds what
its name says, test_gpu_notify_edges.py hands both sides the same arrays and
compares count, header indices and records byte for byte.

Domain.  A word is built only from a (family, mode, kind, CFC_NT_NATLEN)
tuple a classify call can produce: DOMAIN below, which test_notify_edges.py
recomputes from the golden fixtures.  Two places where engine and oracle would
differ outside it are not asserted anywhere:
  * kind 2 (CFC_NT_EGRESS) outside egress mode: the engine's src_label is the
    SECLABEL of the ep_lxc argument, the oracle's is 0;
  * a nonzero word of kind 0: the engine writes a drop record for it, the
    oracle selects nothing.
Every other field — LXC_ID, identity, verdict, length, addresses, ports,
protocol, skb->hash — is data to this code and set freely."""
import copy
import dataclasses
import functools
import itertools

import numpy as np

import golden_io as G
from cilium_amd import synth as S

INGRESS, EGRESS, FULL = 0, 1, 3
NATLEN = 0x01000000             # cfc.h CFC_NT_NATLEN
WAVE, ROUND, BLOCK = 64, 256, 4096   # notify.hip: lanes, NT_THREADS, NT_PER_BLOCK
SCAN_THREADS = 1024             # k_nt_scan's one block

# (family, mode) -> {kind: the CFC_NT_NATLEN values it occurs with}
DOMAIN = {
    (4, INGRESS): {1: (0,), 3: (0, 1), 4: (0, 1), 5: (0,)},
    (4, EGRESS): {2: (0,), 3: (0,), 4: (0,), 6: (0,), 7: (0,)},
    (4, FULL): {3: (0,), 4: (0,)},
    (6, INGRESS): {1: (0,), 3: (0,), 4: (0,), 5: (0,)},
    (6, EGRESS): {2: (0, 1), 3: (0, 1), 4: (0, 1), 6: (0,), 7: (0, 1)},
    (6, FULL): {1: (0,), 3: (0,), 4: (0,)},
}
# mode -> (monitor length classes, CT reasons) of a trace word
TRACE_FIELDS = {INGRESS: ((0, 1, 2, 3), (0, 1, 2, 3)),
                EGRESS: ((0, 1, 2, 3), (0, 1, 2, 3)),
                FULL: ((1, 2), (0,))}
MON_LEN = {1: 128, 2: 1500, 3: 1}   # TRACE_PAYLOAD_LEN, MTU, an active flow's report

# ----------------------------------------------------------------- the tables
EP = S.EP_LXC_ID                # the sending endpoint of the egress cases
LXC_NONE_MID = 0x8000           # no endpoint, like LXC_ID 0
HOST_IFINDEX = 0x30007
# LXC_ID -> (SECLABEL, ifindex): labels above 2^16 whose low halves differ
# from the whole, distinct ifindexes, one of them above 2^16
ENDPOINTS = {1: (0x00012345, 7), EP: (0x0002BEEF, 9), 300: (0x00010000, 11),
             65535: (0xFFFEFFFF, 0x12345)}
LXC_EDGES = (0, 1, LXC_NONE_MID, 65535)


@functools.lru_cache(None)
def tables():
    """small_ingress_v4's ipcache with the endpoints above under both
    families; no policy maps (nothing here is classified but one warm-up
    header)"""
    t = copy.deepcopy(G.Golden("small_ingress_v4").tables)
    eps = []
    for k, (lxc, (lab, ifx)) in enumerate(sorted(ENDPOINTS.items())):
        eps.append(S.endpoint_v4(S.ip4(f"10.9.0.{k + 1}"), ifx, lxc))
        eps.append(S.endpoint_v6(S.ip6(f"fd00:9::{k + 1}"), ifx, lxc))
    t.endpoints = np.concatenate(eps)
    t.seclabel = {lxc: lab for lxc, (lab, ifx) in ENDPOINTS.items()}
    t.policy = {}
    t.ct = None
    t.node = (0x0000000A, 0x000000FF, S.ip6("fd00:1:2:3::1"), HOST_IFINDEX)
    return t


# ------------------------------------------------------------------ the words
def word(kind, lxc=0, nat=0, reason=0, mc=0):
    """cfc.h: EVENT_SOURCE | kind << 16 | CT reason << 20 | monitor length
    class << 22 | CFC_NT_NATLEN"""
    return (lxc & 0xFFFF) | kind << 16 | reason << 20 | mc << 22 | (NATLEN if nat else 0)


def tuples(family, mode, classes=None):
    """(kind, nat, reason, class) of every word shape of DOMAIN and
    TRACE_FIELDS for this (family, mode); classes: only these length classes"""
    cl, rs = TRACE_FIELDS[mode]
    out = []
    for kind, nats in sorted(DOMAIN[(family, mode)].items()):
        for nat in nats:
            if kind < 4:
                out.append((kind, nat, 0, 0))
            else:
                out += [(kind, nat, r, c) for c in cl for r in rs
                        if classes is None or c in classes]
    return out


def selected(words, traces):
    """which words a call records (cfc.h): drops always, traces when asked
    and their monitor length class is not 0"""
    w = np.asarray(words, np.uint32)
    kind = (w >> 16) & 0xF
    return (w != 0) & ((kind < 4) | (bool(traces) & (((w >> 22) & 3) != 0)))


@dataclasses.dataclass
class Case:
    h: S.Headers
    mode: int
    ep: int
    ver: np.ndarray      # int32
    ide: np.ndarray      # uint32
    words: np.ndarray    # uint32

    def __len__(self):
        return len(self.words)

    @property
    def family(self):
        return self.h.family


def ep_of(mode):
    return EP if mode == EGRESS else 0


# ---------------------------------------------------------------- the headers
PROTOS = np.array([0, 1, 6, 17, 58, 255], np.uint8)


def headers(family, n, seed, length=None):
    """n headers with every field random (lengths over the whole 16 bits)"""
    rng = np.random.default_rng(seed)
    if family == 4:
        sa = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        da = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    else:
        sa = rng.integers(0, 256, (n, 16), dtype=np.uint16).astype(np.uint8)
        da = rng.integers(0, 256, (n, 16), dtype=np.uint16).astype(np.uint8)
    ln = rng.integers(40, 1 << 16, n).astype(np.uint16) if length is None else \
        np.full(n, length, np.uint16)
    return S.Headers(family, sa, da,
                     rng.integers(0, 1 << 16, n).astype(np.uint16),
                     rng.integers(0, 1 << 16, n).astype(np.uint16),
                     PROTOS[rng.integers(0, len(PROTOS), n)],
                     np.zeros(n, np.uint8), ln, np.zeros(n, np.uint32))


def constant_headers(n):
    """IPv4 headers of one flow, tiled (the scan cases: 8 M headers)"""
    f = lambda v, dt: np.full(n, v, dt)   # noqa: E731
    return S.Headers(4, f(S.ip4("10.1.2.3"), np.uint32), f(S.ip4("10.9.0.1"), np.uint32),
                     f(S.htons(40000), np.uint16), f(S.htons(443), np.uint16),
                     f(6, np.uint8), f(0, np.uint8), f(777, np.uint16), f(0, np.uint32))


def _fill(rng, n, shapes):
    """n words drawn from the word shapes, LXC_IDs from the endpoints and
    the ids without one"""
    ids = np.array(sorted(ENDPOINTS) + [0, LXC_NONE_MID], np.uint32)
    sh = np.array([word(k, 0, nat, r, c) for k, nat, r, c in shapes], np.uint32)
    return sh[rng.integers(0, len(sh), n)] | ids[rng.integers(0, len(ids), n)]


def words_for(family, mode, mask, traces, seed):
    """event words that the call with `traces` selects exactly at mask.
    traces=1: drops and sendable traces at the mask, and between them zeros
    and length-class-0 trace words (kept by classify, not sent).  traces=0:
    drops at the mask, and between them zeros and trace words of every
    class, which that call must pass over."""
    rng = np.random.default_rng(seed)
    n = len(mask)
    drops = [t for t in tuples(family, mode) if t[0] < 4]
    sent = [t for t in tuples(family, mode, classes=(1, 2, 3)) if t[0] >= 4]
    quiet = [t for t in tuples(family, mode, classes=(0,)) if t[0] >= 4]
    on = _fill(rng, n, drops)
    if traces:   # (as many traces as drops)
        on = np.where(rng.random(n) < 0.5, on, _fill(rng, n, sent))
    off = _fill(rng, n, quiet if traces else quiet + sent)
    off[rng.random(n) < 0.5] = 0
    return np.where(mask, on, off).astype(np.uint32)


def outputs(n, seed):
    """verdicts (negative: drop reasons) and identities over their widths"""
    rng = np.random.default_rng(seed)
    ver = -rng.integers(1, 257, n).astype(np.int32)
    ide = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ide[rng.random(n) < 0.3] &= 0x1FFFF
    return ver, ide


# ------------------------------------------------------ 1: sizes and patterns
SIZES = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193)
PATTERNS = ("none", "all", "lane0", "lane63", "lanes31_32", "wave3", "round15",
            "last", "first", "third")
PATTERN_MODES = ((4, INGRESS), (6, EGRESS))


def pattern_mask(name, n, seed=7):
    i = np.arange(n)
    if name == "none":
        return np.zeros(n, bool)
    if name == "all":
        return np.ones(n, bool)
    if name == "lane0":
        return i % WAVE == 0
    if name == "lane63":
        return i % WAVE == 63
    if name == "lanes31_32":
        return (i % WAVE == 31) | (i % WAVE == 32)
    if name == "wave3":
        return (i % ROUND) // WAVE == 3
    if name == "round15":
        return (i % BLOCK) // ROUND == 15
    if name == "last":
        return i == n - 1
    if name == "first":
        return i == 0
    assert name == "third"
    return np.random.default_rng(seed + n).random(n) < 1 / 3


@functools.lru_cache(None)
def _pool(family):
    n = max(SIZES)
    return headers(family, n, 100 + family), outputs(n, 200 + family)


def pattern_case(family, mode, n, name, traces):
    h, (ver, ide) = _pool(family)
    mask = pattern_mask(name, n)
    return Case(h.slice(0, n), mode, ep_of(mode), ver[:n], ide[:n],
                words_for(family, mode, mask, traces, 31 * n + traces))


# ---------------------------------------------------------------- 2: the scan
SCAN_NB = (1024, 1025, 2049)    # per = 1 (every thread busy), 2 (idle threads,
#                                 a one-block last chunk), 3 (idle threads)
SCAN_MAX_RECORDS = 400_000
SCAN_STRIDE = 67                # 60 records of a block reach its last round


def scan_n(nb):
    return (nb - 1) * BLOCK + 1 if nb > 1024 else nb * BLOCK


def scan_per(nb):
    """k_nt_scan: block counts per thread"""
    return (nb + SCAN_THREADS - 1) // SCAN_THREADS


def scan_block_counts(nb):
    """selected headers of each block: none in every fourth, all 4096 in one
    of 32, else 1 + 37 b mod 60 (two neighbours never equal)"""
    b = np.arange(nb)
    c = 1 + (b * 37) % 60
    c[b % 4 == 0] = 0
    c[b % 32 == 5] = BLOCK
    return c


@functools.lru_cache(None)
def scan_case(nb):
    """IPv4 ingress, n = scan_n(nb) headers of one flow; a block's c selected
    headers sit at its offsets 67 j + b mod 67 (spread over its rounds and
    lanes); the words are drops of the destination's policy program at
    LXC_ID 1"""
    n = scan_n(nb)
    c = scan_block_counts(nb)
    j = np.arange(BLOCK)
    b = np.arange(nb)[:, None]
    at = (j[None, :] - b % SCAN_STRIDE)
    mask = ((at >= 0) & (at % SCAN_STRIDE == 0) & (at // SCAN_STRIDE < c[:, None])) | \
        (c[:, None] == BLOCK)
    mask = mask.reshape(-1)[:n].copy()
    mask[-1] = True             # (a ragged last block holds a record too)
    words = np.where(mask, np.uint32(word(3, 1)), np.uint32(0)).astype(np.uint32)
    # (a sendable trace word in every fourth block: drop_notify passes it over)
    tr = np.arange(1, nb - 1, 4) * BLOCK + np.arange(1, nb - 1, 4) * 7 % BLOCK
    words[tr[~mask[tr]]] = word(4, 65535, 0, 1, 2)
    i = np.arange(n, dtype=np.uint32)
    ver = -(1 + (i % 255).astype(np.int32))
    return Case(constant_headers(n), INGRESS, 0, ver, i * np.uint32(2654435761), words)


def block_counts(words, traces):
    """selected words of every 4096-header block"""
    s = selected(words, traces)
    pad = -len(s) % BLOCK
    return np.concatenate([s, np.zeros(pad, bool)]).reshape(-1, BLOCK).sum(1)


# ------------------------------------------------------------- 3: the buffers
GUARD32, GUARD64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD_ROWS = 64
CAP_N = 8193
CAP_INSIDE_WAVE = 40            # headers into the first wave


@functools.lru_cache(None)
def cap_case(family, traces=1):
    """8193 headers, about a third selected by a call with `traces`, the
    last one among them (every block holds records)"""
    mode = INGRESS if family == 4 else EGRESS
    mask = pattern_mask("third", CAP_N, seed=11)
    mask[-1] = True
    ver, ide = outputs(CAP_N, 300 + family)
    return Case(headers(family, CAP_N, 310 + family), mode, ep_of(mode), ver, ide,
                words_for(family, mode, mask, traces, 320 + family))


def caps_of(case, traces=1):
    """the caps of the case: 0, 1, the total +-1, and the record count
    reached inside the first wave, after the first round and the first block,
    each +-1"""
    s = selected(case.words, traces)
    T = int(s.sum())
    at = [int(s[:k].sum()) for k in (CAP_INSIDE_WAVE, ROUND, BLOCK)]
    caps = {0, 1, T - 1, T, T + 1}
    for a in at:
        caps |= {a - 1, a, a + 1}
    assert min(caps) == 0 and 1 < at[0], (caps, at)
    return sorted(caps), T, at


# ------------------------------------------------------------------ 4: fields
LENGTHS = (0, 1, 19, 20, 21, 127, 128, 129, 1499, 1500, 1501, 65515, 65516, 65535)
# behind a NAT hop an IPv6 batch's header is at least its own 40 bytes
LENGTHS_NAT6 = (40, 41, 59, 60, 61) + LENGTHS[5:]
VERDICTS = (-1, -130, -255, -256)
IDENTITIES = (0, 1, 0xFFFF, 0x10000, 0x1FFFF, 0xFFFFFF, 0xFFFFFFFF)
FIELD_MODES = tuple(sorted(DOMAIN))


@functools.lru_cache(None)
def field_case(family, mode):
    """every word shape of the mode with every length, verdict, identity and
    LXC_ID edge in turn, the other three fields cycling through their edges"""
    rows = []   # (word shape, fields)
    k = 0
    for shape in tuples(family, mode):
        lens = LENGTHS_NAT6 if shape[1] and family == 6 else LENGTHS
        for axis, vals in (("ln", lens), ("ver", VERDICTS), ("ide", IDENTITIES),
                           ("lxc", LXC_EDGES)):
            for v in vals:
                k += 1
                f = dict(ln=lens[k % len(lens)], ver=VERDICTS[k % 4],
                         ide=IDENTITIES[k % 7], lxc=LXC_EDGES[(k // 3) % 4])
                f[axis] = v
                rows.append((shape, f))
    n = len(rows)
    h = headers(family, n, 400 + family + mode)
    h.length = np.array([f["ln"] for s, f in rows], np.uint16)
    return Case(h, mode, ep_of(mode),
                np.array([f["ver"] for s, f in rows], np.int32),
                np.array([f["ide"] for s, f in rows], np.uint32),
                np.array([word(s[0], f["lxc"], s[1], s[2], s[3]) for s, f in rows],
                         np.uint32))


# -------------------------------------------------------------------- 5: hash
HASH_EDGES = (0, 1, 0xFFFFFFFF)


def _alternate_words(family, n):
    """a policy drop and a TO_LXC trace in turn (in every ingress domain)"""
    assert 3 in DOMAIN[(family, INGRESS)] and 4 in DOMAIN[(family, INGRESS)]
    w = np.where(np.arange(n) % 2 == 0, word(3, 1), word(4, 65535, 0, 0, 1))
    return w.astype(np.uint32)


@functools.lru_cache(None)
def skb_hash_case(family, n=300):
    """the caller's skb->hash: the edges among random values"""
    h = headers(family, n, 500 + family)
    rng = np.random.default_rng(510 + family)
    hs = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    hs[:6] = HASH_EDGES + HASH_EDGES    # (a drop and a trace each)
    h.hash = hs
    ver, ide = outputs(n, 520 + family)
    return Case(h, INGRESS, 0, ver, ide, _alternate_words(family, n))


def _addr_pairs(family):
    """(saddr, daddr) pairs: equal, plain, and for IPv6 addresses that differ
    in exactly one of the four words (each word), and two that hold the same
    words in another order"""
    if family == 4:
        a, b = S.ip4("10.1.2.3"), S.ip4("203.0.113.77")
        return [(a, a), (a, b), (0, 0xFFFFFFFF), (0x01020304, 0x04030201)]
    w = np.array([0x11223344, 0x55667788, 0x99AABBCC, 0xDDEEFF01], "<u4")
    addr = lambda x: np.ascontiguousarray(x, "<u4").view(np.uint8).copy()   # noqa: E731
    out = [(addr(w), addr(w)), (addr(w), addr(w[::-1]))]
    for k in range(4):
        v = w.copy()
        v[k] ^= 0x00010000
        out.append((addr(w), addr(v)))
    out.append((addr(w[[1, 0, 2, 3]]), addr(w[[0, 1, 3, 2]])))
    out.append((np.zeros(16, np.uint8), np.full(16, 255, np.uint8)))
    return out


HASH_PORTS = ((1234, 1234), (0, 0xFFFF), (0, 0), (0xFFFF, 0xFFFF), (80, 40000), (0x0100, 0x0001))
HASH_PROTOS = (0, 6, 17, 58, 255)


@functools.lru_cache(None)
def flow_hash_case(family):
    """the computed CFC_FLOW_HASH: every (address pair, port pair, protocol)
    at header 2k and its reverse at 2k + 1"""
    rows = []
    for (sa, da), (sp, dp), pr in itertools.product(_addr_pairs(family), HASH_PORTS,
                                                    HASH_PROTOS):
        rows.append((sa, da, sp, dp, pr))
        rows.append((da, sa, dp, sp, pr))
    n = len(rows)
    adt = np.uint32 if family == 4 else np.uint8
    h = S.Headers(family, np.array([r[0] for r in rows], adt),
                  np.array([r[1] for r in rows], adt),
                  np.array([r[2] for r in rows], np.uint16),
                  np.array([r[3] for r in rows], np.uint16),
                  np.array([r[4] for r in rows], np.uint8), np.zeros(n, np.uint8),
                  np.full(n, 100, np.uint16), np.zeros(n, np.uint32))
    ver, ide = outputs(n, 530 + family)
    # (a drop and a trace for each tuple: the same word on both directions)
    w = np.where(np.arange(n) // 2 % 2 == 0, word(3, 1), word(4, 65535, 0, 0, 1))
    return Case(h, INGRESS, 0, ver, ide, w.astype(np.uint32))


# ------------------------------------------------------ 6, 7: growth, slices
SMALL_N = 100
SLICE_N = 4097


@functools.lru_cache(None)
def small_case(k):
    """100 IPv4 headers, about a third selected (k: which of the two)"""
    mask = pattern_mask("third", SMALL_N, seed=40 + k)
    ver, ide = outputs(SMALL_N, 600 + k)
    return Case(headers(4, SMALL_N, 610 + k), INGRESS, 0, ver, ide,
                words_for(4, INGRESS, mask, 1, 620 + k))


@functools.lru_cache(None)
def slice_case(family):
    mode = INGRESS if family == 4 else EGRESS
    mask = pattern_mask("third", SLICE_N, seed=50)
    ver, ide = outputs(SLICE_N, 700 + family)
    return Case(headers(family, SLICE_N, 710 + family), mode, ep_of(mode), ver, ide,
                words_for(family, mode, mask, 1, 720 + family))
