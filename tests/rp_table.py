"""The reverse-proxy device tables (cilium_amd/csrc/layout.h RevTables,
flatten.cpp build_revproxy) restated in Python, and the key sets the device
upsert's tests (test_gpu_proxy_table.py; CFC_OPT_PROXY_APPLY) are built from.

  rp4_hash / rp6_hash   the hashes (test_proxy_table_opt.py pins them against
                        layout.h with known answers from a host program)
  home, place           a key's home slot; the slot of every key of a map as
                        build_revproxy places them (the map's iteration order
                        is the byte order of its keys)
  edges(v6)             a 33-entry map in 128 slots and one 257-header batch
                        whose records meet every structural shape of the
                        upsert (claims asserted on the CPU first)
The redirect batches carry hand-made outputs (verdict = the proxy port on the
redirected rows, no CT bytes: every stage CT_NEW), so a record's key is {the
header's source address, the proxy port, its source port, its protocol} and
its value {its destination address and port, the identity column, the clock
+ 720}: the tests choose every bit of a key."""
import dataclasses

import numpy as np

import lookup_edges as E
import revproxy_ref as R
import revproxy_streams as RS
from cilium_amd import synth as S

U64 = np.uint64
CLOCK = RS.CLOCK
PROXY_PORT = RS.PROXY_PORT            # be16 raw
IDENT = 777                           # the redirect batches' identity column
SLOTS = 128
MASK = SLOTS - 1


# ------------------------------------------------------------------- hashes
def _nh_mul(nh):
    return E._mul32(nh, 0x01000193)


def rp4_hash(saddr, ports, nexthdr):
    return E.fmix32(E.fmix32(E._a(saddr) ^ U64(0x7ed55d16)) ^ E._a(ports) ^ _nh_mul(nexthdr))


def rp6_hash(a0, a1, a2, a3, ports, nexthdr):
    return E.l6_hash(a0, a1, a2, a3, E._a(ports) ^ _nh_mul(nexthdr) ^ U64(0x3c6ef372))


def key_words(key):
    """struct proxy{4,6}_tbl_key -> (address words, the port word, nexthdr)
    as the tables hold them (little-endian loads; the pad byte is not part)"""
    al = len(key) - 6
    a = tuple(int(x) for x in np.frombuffer(key[:al], "<u4"))
    return a, int.from_bytes(key[al:al + 4], "little"), key[al + 4]


def hash_of(key):
    a, pt, nh = key_words(key)
    return int(rp4_hash(a[0], pt, nh) if len(a) == 1 else rp6_hash(*a, pt, nh))


def home(key, slots=SLOTS):
    return hash_of(key) & (slots - 1)


def slots_for(n, quarter):
    """build_revproxy's slot count for n entries (0: no table)"""
    return E.pow2_at_least((4 if quarter else 2) * n) if n else 0


def place(keys, slots=SLOTS):
    """{key: slot} as build_revproxy fills an empty table of `slots` from a
    map holding `keys`"""
    used, at = set(), {}
    for k in sorted(keys):
        s = home(k, slots)
        while s in used:
            s = (s + 1) & (slots - 1)
        used.add(s)
        at[k] = s
    return at


# --------------------------------------------------------------------- keys
def ab(v6, a):
    """an address as the streams hold it -> its 4 / 16 raw bytes"""
    return bytes(np.asarray(a, np.uint8)) if v6 else np.uint32(a).tobytes()


def key(v6, addr, sport, nexthdr=6, dport=PROXY_PORT):
    """addr: raw bytes; sport / dport: be16 raw (dport: the proxy's)"""
    return R.entry(6 if v6 else 4, addr, sport, dport, nexthdr, bytes(16 if v6 else 4), 0)[0]


def value(v6, odaddr, odport, identity=IDENT, lifetime=CLOCK + 720):
    return R.entry(6 if v6 else 4, bytes(16 if v6 else 4), 0, 0, 6, odaddr, odport, identity,
                   lifetime)[1]


def addrs(v6):
    """the two addresses keys are made of: the endpoint's and another"""
    return ab(v6, RS.ep_addr(v6)), ab(v6, RS.src_addrs(v6)["real"])


def dest(v6, k):
    """the k-th original destination: (address bytes, port be16 raw)"""
    return ab(v6, RS.orig_daddr(v6, k % 200)), int(S.htons(80 + k % 1000))


def _col(v6, rows):
    if v6:
        return np.stack([np.frombuffer(r, np.uint8) for r in rows])
    return np.array([np.frombuffer(r, "<u4")[0] for r in rows], np.uint32)


def redirect_headers(v6, recs, n=None, at=None, ident=IDENT):
    """a batch of n headers (default: one per record) with recs — [(key,
    (dest address, dest port))] — at the indices `at`; the other headers
    are not redirected -> (headers, verdicts, identities)"""
    n = len(recs) if n is None else n
    at = list(range(len(recs))) if at is None else list(at)
    assert len(at) == len(recs) and len(set(at)) == len(at) and max(at, default=0) < n
    al = 16 if v6 else 4
    sa = [ab(v6, RS.src_addrs(v6)["none"])] * n
    da = [ab(v6, RS.ep_addr(v6))] * n
    sp = S.htons(2000 + np.arange(n)).astype(np.uint16)
    dp = np.full(n, S.htons(81), np.uint16)
    proto = np.full(n, 6, np.uint8)
    ver = np.zeros(n, np.int32)
    for i, (k, (od, op)) in zip(at, recs):
        sa[i], da[i] = k[:al], od
        assert int.from_bytes(k[al:al + 2], "little") == PROXY_PORT
        sp[i], dp[i], proto[i] = int.from_bytes(k[al + 2:al + 4], "little"), op, k[al + 4]
        ver[i] = PROXY_PORT
    h = S.Headers(6 if v6 else 4, _col(v6, sa), _col(v6, da), sp, dp, proto,
                  np.zeros(n, np.uint8), np.full(n, 100, np.uint16), np.zeros(n, np.uint32))
    return h, ver, np.full(n, ident, np.uint32)


def records_of(v6, recs, ident=IDENT):
    """the map rows the batch of redirect_headers(recs) writes"""
    return {k: value(v6, od, op, ident) for k, (od, op) in recs}


MARKS = (0xB00 | R.enc(RS.ID_A), 0, 0xC00, 0xA00 | R.enc(RS.ID_P))


def probes(v6, keys, plain=9):
    """the from-host batch of the tests: one header per key (each hits when
    the table holds the key), four near misses per key — another address,
    source port, destination port, protocol, each a header no key of these
    streams matches — and plain headers -> (headers, hit rows, miss rows)"""
    al = 16 if v6 else 4
    src = ab(v6, RS.host_addr(v6))
    rows = []

    def pkt(da, sport, dport, proto):
        i = len(rows)
        rows.append((src, da, sport, dport, proto, MARKS[i % 4]))

    for k in keys:
        pkt(k[:al], PROXY_PORT, int.from_bytes(k[al + 2:al + 4], "little"), k[al + 4])
    nk = len(rows)
    for j, k in enumerate(keys):
        cp = int.from_bytes(k[al + 2:al + 4], "little")
        pkt(ab(v6, RS.orig_daddr(v6, 150 + j % 40)), PROXY_PORT, cp, k[al + 4])
        pkt(k[:al], int(S.htons(10002)), cp, k[al + 4])
        pkt(k[:al], PROXY_PORT, int(S.htons(1 + j % 1000)), k[al + 4])   # (keys: ports >= 1024)
        pkt(k[:al], PROXY_PORT, cp, 17 if k[al + 4] == 6 else 6)
    nm = len(rows)
    h = S.Headers(6 if v6 else 4, _col(v6, [r[0] for r in rows]), _col(v6, [r[1] for r in rows]),
                  np.array([r[2] for r in rows], np.uint16),
                  np.array([r[3] for r in rows], np.uint16),
                  np.array([r[4] for r in rows], np.uint8), np.zeros(nm, np.uint8),
                  (60 + (np.arange(nm) * 37) % 1400).astype(np.uint16),
                  np.array([r[5] for r in rows], np.uint32))
    s = RS.src_addrs(v6)
    # (plain: not from the proxy's port, so no key of any stream matches)
    parts = [h] + [RS.proxy_pkt(v6, s[("real", "none", "host")[i % 3]], RS.CLIENT0 + i,
                                MARKS[i % 4], proto=17 if i % 2 else 6,
                                sport=int(S.htons(5555))) for i in range(plain)]
    return RS.concat(parts), np.arange(nk), np.arange(nk, nm + plain)


# --------------------------------------------------------- the candidate keys
def candidates(v6):
    """every (address, source port >= 1024) key of the two addresses with its
    home slot in a 128-slot table -> [(key, home)] in a fixed order"""
    out = []
    ports = np.arange(1024, 65536, dtype=np.uint32)
    sp = S.htons(ports).astype(np.uint32)
    pt = np.uint32(PROXY_PORT) | (sp << np.uint32(16))
    for a in addrs(v6):
        w = [int(x) for x in np.frombuffer(a, "<u4")]
        hs = rp6_hash(*w, pt, 6) if v6 else rp4_hash(w[0], pt, 6)
        hs = (hs & U64(MASK)).astype(np.int64)
        out.append((a, sp, hs))
    return out


def pick(cands, used, want_home, addr=None, n=1):
    """n unused keys with home slot `want_home` (of address index addr)"""
    got = []
    for ai, (a, sp, hs) in enumerate(cands):
        if addr is not None and ai != addr:
            continue
        for j in np.flatnonzero(hs == want_home):
            k = key(len(a) == 16, a, int(sp[j]))
            if k not in used:
                used.add(k)
                got.append(k)
                if len(got) == n:
                    return got
    raise AssertionError(f"no key with home {want_home}")


@dataclasses.dataclass
class Edges:
    v6: bool
    base: dict          # the 33-entry map the 128-slot table is committed from
    recs: list          # the batch's records [(key, (dest address, dest port))]
    at: list            # their header indices in the 257-header batch
    new: list           # record keys the table lacks
    old: list           # record keys it holds
    shape: dict         # named keys, for the claims


# zones of the 128 slots (everything else stays free):
#   126 127 0   the wrapping cluster; a new key of home 127 lands on 1
#   8 9 10      a cluster of three; a new key of home 8 lands on 11
#   16 17 18    three keys of home 16: one sits two slots from home
#   24..26      three new keys of home 24
#   30          the key re-written with an identical value
#   40..84      23 fillers on even slots
#   96..120     the new keys of the address / port pairs
_cache = {}


def edges(v6):
    if v6 in _cache:
        return _cache[v6]
    c = candidates(v6)
    used = set()
    one = lambda h, **kw: pick(c, used, h, **kw)[0]   # noqa: E731
    wrap = [one(126), one(127), one(0)]
    cluster = [one(8), one(9), one(10)]
    trio = pick(c, used, 16, n=3)
    same = one(30)
    fill = [one(h) for h in range(40, 86, 2)]
    base_keys = wrap + cluster + trio + [same] + fill
    assert len(base_keys) == 33
    d_same = dest(v6, 7)
    base = {k: value(v6, *dest(v6, 20 + i), identity=5, lifetime=CLOCK + 9)
            for i, k in enumerate(base_keys)}
    base[same] = value(v6, *d_same)            # what the batch writes again
    at0 = place(base_keys)
    displaced = [k for k in trio if at0[k] == 18]
    assert len(displaced) == 1
    displaced = displaced[0]
    new24 = pick(c, used, 24, n=3)
    new_head = one(8)
    new_wrap = one(127)
    # equal ports and next header, different addresses; equal address,
    # different ports: homes in the free zone, two slots apart at least
    a0, sp0, h0 = c[0]
    a1, sp1, h1 = c[1]
    pair = None
    for j in range(len(sp0)):
        if 96 <= h0[j] <= 120 and 96 <= h1[j] <= 120 and abs(int(h0[j]) - int(h1[j])) >= 2:
            pair = [key(v6, a0, int(sp0[j])), key(v6, a1, int(sp1[j]))]
            break
    assert pair and not (set(pair) & used)
    used.update(pair)
    hp = {home(k) for k in pair}
    other = None
    for j in range(len(sp0)):
        k = key(v6, a0, int(sp0[j]))
        if 96 <= h0[j] <= 120 and all(abs(int(h0[j]) - x) >= 2 for x in hp) and k not in used:
            other = k
            break
    assert other
    used.add(other)
    new = new24 + [new_head, new_wrap] + pair + [other]
    old = [displaced, same]
    order = [new24[0], displaced, new_head, pair[0], new24[1], same, new_wrap, pair[1],
             other, new24[2]]
    recs = [(k, d_same if k == same else dest(v6, 60 + i)) for i, k in enumerate(order)]
    at = [0, 1, 63, 64, 100, 128, 129, 200, 255, 256]
    x = Edges(v6, base, recs, at, new, old,
              dict(wrap=wrap, cluster=cluster, trio=trio, same=same, displaced=displaced,
                   new24=new24, new_head=new_head, new_wrap=new_wrap, pair=pair, other=other))
    _cache[v6] = x
    return x


def more_keys(v6, n, skip):
    """n further keys (any home) outside `skip`, in a fixed order"""
    out = []
    for a, sp, hs in candidates(v6):
        for j in range(0, len(sp), 97):
            k = key(v6, a, int(sp[j]))
            if k not in skip:
                out.append(k)
                if len(out) == n:
                    return out
    raise AssertionError("not enough keys")
