"""Tables and probe streams that put the device table lookups (csrc
kern_common.hpp l4_lookup / lxc_resolve / pf_resolve / policy_issue /
policy_resolve_walk, classify.hip's DIR-24-8 probe, classify6.hip lpm6_lookup
/ lxc6_find) at their structural edges, built with numpy, synth and the
oracle alone.  The layout.h hashes and the sizing rules of flatten.cpp are
restated here so that keys can be placed on purpose: probe chains that wrap
from a table's last slot to slot 0, Bloom false positives, every shape of the
compact IPv4 LPM's /16 directory, endpoint tables just over the LDS limits.
test_lookup_edges.py checks on the CPU that every case holds what it claims;
test_gpu_lookup_edges.py runs them through the engine."""
import dataclasses
import functools
import struct

import numpy as np

from cilium_amd import synth as S

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
LAST16 = 0xFFFF     # a hash whose low 16 bits are all ones: the last slot of
#                     any power-of-two table of up to 65 536 slots

# layout.h / flatten.cpp constants
L4_LIST_MAX, L4_INLINE = 16, 2
L6_GROUP_FIRST, L6_GROUP_MAX, L6_LXC_TAG = 1 << 16, 4, 0x200
LXC_LDS_MAX_SLOTS, LXC6_LDS_MAX_SLOTS = 512, 256
POL_BLOOM_MAX_WORDS = PF_BLOOM_MAX_WORDS = 8192
PF_SLOTS = 4
DROP_POLICY, DROP_PREFILTER = -133, -1


# ------------------------------------------------------------ layout.h hashes
def _a(x):
    return np.asarray(x, dtype=np.uint64)


def _mul32(a, c):
    return (_a(a) * U64(c)) & M32      # (32 x 32 bits: no 64-bit overflow)


def fmix32(h):
    h = _a(h) & M32
    h = h ^ (h >> U64(16))
    h = _mul32(h, 0x85ebca6b)
    h = h ^ (h >> U64(13))
    h = _mul32(h, 0xc2b2ae35)
    return h ^ (h >> U64(16))


def hash32(k, mask):
    with np.errstate(over="ignore"):
        x = _a(k) * U64(0x9E3779B97F4A7C15)
    return (x >> U64(32)) & _a(mask)


def pol_key_pre(lo, hi):
    return fmix32(_mul32(lo, 0x9E3779B1) ^ _a(hi))


def pol_slot(pre, mask):
    return _a(pre) & _a(mask)


def bloom_bits(h):
    h = _a(h)
    one = U64(1)
    return (one << ((h >> U64(17)) & U64(31))) | (one << ((h >> U64(22)) & U64(31))) | \
        (one << (h >> U64(27)))


def pol_bloom_salt(base):
    return _mul32((_a(base) + U64(1)) & M32, 0x9E3779B1)


def pol_bloom_hash(salt, pre):
    salt, pre = _a(salt), _a(pre)
    return pre ^ (salt >> U64(16)) ^ (pre >> U64(19))


def pf_bloom_hash(addr):
    return fmix32(_a(addr) ^ U64(0x5bd1e995))


def l6_word_mask(length, i):
    b = np.asarray(length, np.int64) - 32 * np.asarray(i, np.int64)
    sh = np.clip(32 - b, 0, 32).astype(np.uint64)
    return (M32 << sh) & M32


def l6_hash(w0, w1, w2, w3, tag):
    return fmix32((_mul32(w0, 0x9E3779B1) + _mul32(w1, 0x85EBCA77) + _mul32(w2, 0xC2B2AE3D) +
                   _mul32(w3, 0x27D4EB2F) + _mul32(tag, 0x165667B1)) & M32)


def l6_group_hash(w, sel):
    m = [_a(w[i]) & l6_word_mask(sel, i) for i in range(4)]
    return l6_hash(m[0], m[1], m[2], m[3], _a(sel) | U64(0x100))


def l6_bloom_bits(h):
    h = _a(h)
    return (U64(1) << ((h >> U64(20)) & U64(63))) | (U64(1) << (h >> U64(26)))


def pf6_bloom_hash(w0, w1, w2, w3):
    return fmix32(l6_hash(w0, w1, w2, w3, 0x300) ^ U64(0x5bd1e995))


HASHES = dict(fmix32=fmix32, hash32=hash32, pol_key_pre=pol_key_pre, pol_slot=pol_slot,
              bloom_bits=bloom_bits, pol_bloom_salt=pol_bloom_salt,
              pol_bloom_hash=pol_bloom_hash, pf_bloom_hash=pf_bloom_hash,
              l6_word_mask=l6_word_mask, l6_hash=l6_hash,
              l6_group_hash=lambda a, b, c, d, sel: l6_group_hash((a, b, c, d), sel),
              l6_bloom_bits=l6_bloom_bits, pf6_bloom_hash=pf6_bloom_hash)


# ------------------------------------------------- flatten.cpp sizing, placing
def pow2_at_least(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def bloom_words(keys, max_words=POL_BLOOM_MAX_WORDS):
    return min(pow2_at_least(max(64, keys)), max_words)


def _place(slots, home, item):
    """linear probing from `home`; -> the slot taken"""
    s = home
    while slots[s] is not None:
        s = (s + 1) & (len(slots) - 1)
    slots[s] = item
    return s


def pol_key_words(r):
    """(lo, hi) of a POLICY_DT row's struct policy_key"""
    return int(r["identity"]), int(r["dport"]) | int(r["proto"]) << 16 | int(r["egress"]) << 24


def policy_model(policy):
    """{lxc: POLICY_DT rows} -> the policy array as build_image lays it out:
    per lxc {base, mask, slots: [(lo, hi, proxy) | None], home: {(lo, hi): slot}},
    and the Bloom filter words (None: no key at all).  Tables in ascending lxc
    id, keys in the map's (byte) order."""
    nkeys = sum(len(p) for p in policy.values())
    bloom = np.zeros(bloom_words(nkeys), np.uint64) if nkeys else None
    out, base = {}, 0
    for lxc in sorted(policy):
        rows = sorted(policy[lxc], key=lambda r: struct.pack(
            "<IHBB", int(r["identity"]), int(r["dport"]), int(r["proto"]), int(r["egress"])))
        ns = pow2_at_least(max(8, 4 * len(rows)))
        slots, where, home = [None] * ns, {}, {}
        for r in rows:
            lo, hi = pol_key_words(r)
            pre = int(pol_key_pre(lo, hi))
            home[(lo, hi)] = pre & (ns - 1)
            where[(lo, hi)] = _place(slots, pre & (ns - 1), (lo, hi, int(r["proxy_port"])))
            h = int(pol_bloom_hash(pol_bloom_salt(base), pre))
            bloom[h & (len(bloom) - 1)] |= bloom_bits(h)
        out[lxc] = dict(base=base, mask=ns - 1, slots=slots, where=where, home=home)
        base += ns
    return out, bloom


def pol_maybe(model, bloom, lxc, lo, hi):
    """the answer of the policy Bloom filter for key (lo, hi) of lxc's table"""
    if bloom is None:
        return True
    h = int(pol_bloom_hash(pol_bloom_salt(model[lxc]["base"]), pol_key_pre(lo, hi)))
    b = int(bloom_bits(h))
    return (int(bloom[h & (len(bloom) - 1)]) & b) == b


def pol_walk(model, lxc, lo, hi):
    """the slots policy_resolve_walk reads for (lo, hi) -> ([slots], hit)"""
    m = model[lxc]
    s, seen = int(pol_key_pre(lo, hi)) & m["mask"], []
    while True:
        seen.append(s)
        e = m["slots"][s]
        if e is None or e[:2] == (lo, hi):
            return seen, e is not None
        s = (s + 1) & m["mask"]


def lxc4_model(endpoints):
    """ENDPOINT_DT rows -> (slots [raw address | None], where {raw: slot})"""
    e = endpoints[endpoints["family"] == 1]
    raws = sorted((bytes(a[:4]) for a in e["addr"]))
    ns = pow2_at_least(max(8, 4 * len(raws)))
    slots, where = [None] * ns, {}
    for b in raws:
        raw = int.from_bytes(b, "little")
        where[raw] = _place(slots, int(hash32(raw, ns - 1)), raw)
    return slots, where


def raw_words6(addr16):
    """16 network-order bytes -> the four words as the kernels load them"""
    return tuple(int(x) for x in np.frombuffer(bytes(addr16), "<u4"))


def host_words6(addr16):
    return tuple(int(x) for x in np.frombuffer(bytes(addr16), ">u4"))


def lxc6_model(endpoints):
    e = endpoints[endpoints["family"] == 2]
    keys = sorted(bytes(a) for a in e["addr"])
    ns = pow2_at_least(max(8, 4 * len(keys)))
    slots, where = [None] * ns, {}
    for b in keys:
        w = raw_words6(b)
        where[b] = _place(slots, int(l6_hash(*w, L6_LXC_TAG)) & (ns - 1), b)
    return slots, where


def pf_fix_model(prefilter):
    """PREFILTER_DT rows -> dict(buckets [[raw, ...]], zero, bloom) of the
    IPv4 exact set (None: no nonzero address)"""
    p = prefilter[(prefilter["family"] == 1) & (prefilter["dyn"] == 0) &
                  (prefilter["plen"] == 32)]
    raws = sorted(bytes(a[:4]) for a in p["addr"])
    zero = b"\0\0\0\0" in raws
    raws = [int.from_bytes(b, "little") for b in raws if b != b"\0\0\0\0"]
    if not raws:
        return dict(buckets=None, zero=zero, bloom=None, where={})
    bloom = np.zeros(bloom_words(2 * len(raws), PF_BLOOM_MAX_WORDS), np.uint64)
    nb = pow2_at_least(len(raws))
    buckets, where = [[] for _ in range(nb)], {}
    for a in raws:
        h = int(pf_bloom_hash(a))
        bloom[h & (len(bloom) - 1)] |= bloom_bits(h)
        b = int(hash32(a, nb - 1))
        while len(buckets[b]) == PF_SLOTS:
            b = (b + 1) & (nb - 1)
        buckets[b].append(a)
        where[a] = b
    return dict(buckets=buckets, zero=zero, bloom=bloom, where=where)


def pf_maybe(model, raw):
    h = int(pf_bloom_hash(raw))
    b = int(bloom_bits(h))
    return (int(model["bloom"][h & (len(model["bloom"]) - 1)]) & b) == b


def mask4(plen):
    return (0xFFFFFFFF << (32 - plen)) & 0xFFFFFFFF if plen else 0


def l4_dir_cases(prefixes):
    """[(host-order address, plen, label)] -> {/16 index: case} for every /16
    that holds a prefix longer than /16: ("inline", n), ("list", cnt) with
    cnt the padded list length behind the two inline entries, or ("chunk", n)
    (flatten.cpp L4Trie::node at the directory level)"""
    n16 = {}
    for a, l, _ in prefixes:
        if l > 16:
            n16[a >> 16] = n16.get(a >> 16, 0) + 1
    out = {}
    for d, n in n16.items():
        if n + 1 >= L4_LIST_MAX:
            out[d] = ("chunk", n)
        elif n <= L4_INLINE:
            out[d] = ("inline", n)
        else:
            cnt = n - L4_INLINE + 1
            out[d] = ("list", cnt + (cnt & 1))
    return out


def mask128(plen):
    return ((1 << 128) - 1) ^ ((1 << (128 - plen)) - 1)


def words_of(x):
    """a 128-bit address as four host-order words"""
    return tuple((x >> s) & 0xFFFFFFFF for s in (96, 64, 32, 0))


def lpm6_model(prefixes):
    """[(128-bit address, plen, label)] -> the image build_lpm6 makes: lens,
    groups, bloom (u64 words), slots64 / slots ([(addr, plen, label) | None]
    or None), where, def_label.  Keys go in longest length first, each length
    in ascending address order (the ipcache map's)."""
    by_len, def_label = {}, 0
    for a, l, lab in sorted(set(prefixes)):
        if l == 0:
            def_label = lab
        else:
            by_len.setdefault(l, []).append((a & mask128(l), l, lab))
    L = sorted(by_len, reverse=True)
    m = dict(lens=[], groups=0, bloom=None, slots64=None, slots=None, where={},
             def_label=def_label, sel={})
    if not L:
        return m

    def max_pile(i, k):
        seen = {}
        for j in range(i, k + 1):
            for a, _, _ in by_len[L[j]]:
                x = a & mask128(L[k])
                seen[x] = seen.get(x, 0) + 1
        return max(seen.values())
    i = 0
    while i < len(L):
        k = i
        while k + 1 < len(L) and max_pile(i, k + 1) <= L6_GROUP_MAX:
            k += 1
        for j in range(i, k + 1):
            m["lens"].append(L[j] | L[k] << 8 | (L6_GROUP_FIRST if j == i else 0))
            m["sel"][L[j]] = L[k]
        m["groups"] += 1
        i = k + 1
    nkeys = sum(len(v) for v in by_len.values())
    n64 = sum(len(v) for l, v in by_len.items() if l <= 64)
    m["bloom"] = np.zeros(pow2_at_least(max(64, nkeys // 4)), np.uint64)
    if nkeys > n64:
        m["slots"] = [None] * pow2_at_least(max(16, 2 * (nkeys - n64)))
    if n64:
        m["slots64"] = [None] * pow2_at_least(max(16, 2 * n64))
    for l in L:
        for a, _, lab in by_len[l]:
            w = words_of(a)
            h = int(l6_hash(*w, l))
            g = int(l6_group_hash(w, m["sel"][l])) & (len(m["bloom"]) - 1)
            m["bloom"][g] |= l6_bloom_bits(h)
            tab = m["slots64"] if l <= 64 else m["slots"]
            m["where"][(a, l)] = _place(tab, h & (len(tab) - 1), (a, l, lab))
    return m


def lpm6_model_lookup(m, addr, check_len=True):
    """lpm6_lookup over the model; check_len=False: the slots64 probe
    without its `k.w == len` (what a wrong kernel would do)"""
    bw = 0
    for e in m["lens"]:
        l = e & 255
        if e & L6_GROUP_FIRST:
            g = int(l6_group_hash(words_of(addr), (e >> 8) & 255))
            bw = int(m["bloom"][g & (len(m["bloom"]) - 1)])
        x = addr & mask128(l)
        h = int(l6_hash(*words_of(x), l))
        b = int(l6_bloom_bits(h))
        if (bw & b) != b:
            continue
        tab = m["slots64"] if l <= 64 else m["slots"]
        s = h & (len(tab) - 1)
        while tab[s] is not None:
            ka, kl, lab = tab[s]
            if ka == x and (kl == l or (l <= 64 and not check_len)):
                return lab
            s = (s + 1) & (len(tab) - 1)
    return m["def_label"]


# ------------------------------------------------------ brute-force references
def brute_lpm4(prefixes, host_addrs):
    """longest-prefix match of host-order addresses -> (label, matched)"""
    a = np.asarray(host_addrs, np.uint32)
    best = np.full(len(a), -1, np.int64)
    lab = np.zeros(len(a), np.uint32)
    for pa, pl, pv in prefixes:
        hit = ((a & np.uint32(mask4(pl))) == np.uint32(pa)) & (pl > best)
        best[hit] = pl
        lab[hit] = pv
    return lab, best >= 0


def brute_lpm6(prefixes, addrs):
    """the same over 128-bit Python ints"""
    by_len = {}
    for a, l, v in prefixes:
        by_len.setdefault(l, {})[a & mask128(l) if l else 0] = v
    L = sorted(by_len, reverse=True)
    lab, hit = [], []
    for x in addrs:
        for l in L:
            v = by_len[l].get(x & mask128(l) if l else 0)
            if v is not None:
                lab.append(v)
                hit.append(True)
                break
        else:
            lab.append(0)
            hit.append(False)
    return np.array(lab, np.uint32), np.array(hit)


def brute_deny4(prefilter, raw_saddr):
    """prefilter verdict of IPv4 sources (be32 raw): in the exact /32 set, or
    inside a dynamic prefix"""
    p = prefilter[prefilter["family"] == 1]
    raw = np.asarray(raw_saddr, np.uint32)
    host = S.byteswap32(raw)
    deny = np.zeros(len(raw), bool)
    for r in p:
        a = int.from_bytes(bytes(r["addr"][:4]), "big")
        l = int(r["plen"])
        if r["dyn"]:
            deny |= (host & np.uint32(mask4(l))) == np.uint32(a & mask4(l))
        elif l == 32:
            deny |= host == np.uint32(a)
    return deny


def brute_deny6(prefilter, addrs):
    """the same for 128-bit sources (Python ints)"""
    p = prefilter[prefilter["family"] == 2]
    exact = set(int.from_bytes(bytes(r["addr"]), "big") for r in p
                if not r["dyn"] and r["plen"] == 128)
    dyn = [(int.from_bytes(bytes(r["addr"]), "big"), int(r["plen"])) for r in p if r["dyn"]]
    return np.array([x in exact or any((x & mask128(l)) == (a & mask128(l)) for a, l in dyn)
                     for x in addrs])


# ------------------------------------------------------------------- searches
@functools.lru_cache(None)
def last_slot_v4():
    """be32-raw addresses of 10.0.0.0/8 whose hash32 is the last slot of any
    table of up to 65 536 slots (endpoints, prefilter buckets), ascending by
    host order"""
    host = (np.uint32(10 << 24) + np.arange(1 << 24, dtype=np.uint32))
    raw = S.byteswap32(host)
    return raw[hash32(raw, LAST16) == LAST16]


@functools.lru_cache(None)
def last_slot_policy_ids(dport_raw, proto, egress, lo=256, hi=1 << 22):
    """identities whose key {id, dport, proto, egress} is homed at the last
    slot of any policy table of up to 65 536 slots"""
    ids = np.arange(lo, hi, dtype=np.uint64)
    pre = pol_key_pre(ids, dport_raw | proto << 16 | egress << 24)
    return ids[(pre & U64(LAST16)) == LAST16].astype(np.uint32)


def last_slot_l6(w, tag, vary, n=1 << 22, step=1):
    """values of word `vary` (the others from w) for which l6_hash(w, tag)
    has its low 16 bits all ones"""
    v = np.arange(n, dtype=np.uint64) * U64(step)
    ws = [v if i == vary else U64(w[i]) for i in range(4)]
    return v[(l6_hash(*ws, tag) & U64(LAST16)) == LAST16]


# ------------------------------------------------------------------ the cases
@dataclasses.dataclass
class Case:
    tables: S.Tables
    headers: S.Headers
    mode: int
    ep_lxc: int
    claims: dict

    def __iter__(self):          # (tables, headers, mode, ep_lxc, claims)
        return iter((self.tables, self.headers, self.mode, self.ep_lxc, self.claims))


EP0 = S.EP_LXC_ID
PORTS = np.array([80, 81, 443, 53], np.uint32)
LENGTHS = np.array([60, 61, 1500, 65535, 577], np.uint16)


def hdr4(saddr, daddr, dport=80, proto=S.IPPROTO_TCP, flags=0, mark=0):
    """IPv4 headers from be32-raw addresses (each argument broadcast)"""
    saddr, daddr, dport, proto, flags = np.broadcast_arrays(
        np.asarray(saddr, np.uint32), np.asarray(daddr, np.uint32), np.asarray(dport, np.uint32),
        np.asarray(proto, np.uint8), np.asarray(flags, np.uint8))
    n = len(saddr)
    k = np.arange(n)
    return S.Headers(4, saddr.copy(), daddr.copy(), S.htons(40000 + k % 1000), S.htons(dport),
                     proto.copy(), flags.copy(), LENGTHS[k % len(LENGTHS)].copy(),
                     np.full(n, mark, np.uint32))


def bytes6(x):
    return np.frombuffer(int(x).to_bytes(16, "big"), np.uint8)


def hdr6(saddr, daddr, dport=80, proto=S.IPPROTO_TCP, flags=0):
    """IPv6 headers from (n, 16) byte arrays"""
    saddr, daddr = np.asarray(saddr, np.uint8), np.asarray(daddr, np.uint8)
    n = max(saddr.reshape(-1, 16).shape[0], daddr.reshape(-1, 16).shape[0])
    saddr = np.broadcast_to(saddr.reshape(-1, 16), (n, 16)).copy()
    daddr = np.broadcast_to(daddr.reshape(-1, 16), (n, 16)).copy()
    k = np.arange(n)
    dport = np.broadcast_to(np.asarray(dport, np.uint32), (n,))
    return S.Headers(6, saddr, daddr, S.htons(40000 + k % 1000), S.htons(dport),
                     np.broadcast_to(np.asarray(proto, np.uint8), (n,)).copy(),
                     np.broadcast_to(np.asarray(flags, np.uint8), (n,)).copy(),
                     LENGTHS[k % len(LENGTHS)].copy(), np.zeros(n, np.uint32))


def tile(h, n, seed=None):
    """h repeated up to n headers; seed: shuffled"""
    idx = np.arange(n) % len(h)
    if seed is not None:
        idx = np.random.default_rng(seed).permutation(idx)
    out = S.take(h, idx)
    out.length = LENGTHS[np.arange(n) % len(LENGTHS)].copy()
    return out


def pol_rows(rows):
    """[(identity, dport host order, proto, egress, proxy host order)]"""
    out = np.zeros(len(rows), S.POLICY_DT)
    for i, (ident, dport, proto, egress, proxy) in enumerate(rows):
        out[i] = (ident, int(S.htons(dport)), proto, egress, int(S.htons(proxy)))
    return out


def host4(s):
    return int.from_bytes(bytes(int(p) for p in s.split(".")), "big")


def raw4(host):
    return S.byteswap32(np.asarray(host, np.uint32))


def ipc4(prefixes):
    """[(host-order address, plen, label)] -> IPCACHE_DT rows"""
    a = np.array([p[0] for p in prefixes], np.uint32)
    return S._v4_entries(raw4(a), [p[1] for p in prefixes], [p[2] for p in prefixes])


def ipc6(prefixes):
    a = np.stack([bytes6(p[0]) for p in prefixes])
    return S._v6_entries(a, [p[1] for p in prefixes], [p[2] for p in prefixes])


def endpoints4(raws, first_lxc=EP0):
    return np.concatenate([S.endpoint_v4(int(a), 100 + i, first_lxc + i)
                           for i, a in enumerate(raws)])


def boundary4(prefixes):
    """first and last address of every prefix and the ones before and after,
    host order, sorted and unique"""
    out = set()
    for a, l, _ in prefixes:
        last = a | (~mask4(l) & 0xFFFFFFFF)
        out.update((a, last, (a - 1) & 0xFFFFFFFF, (last + 1) & 0xFFFFFFFF))
    return np.array(sorted(out), np.uint32)


def boundary6(prefixes):
    out = set()
    full = (1 << 128) - 1
    for a, l, _ in prefixes:
        a &= mask128(l) if l else 0
        last = a | (full ^ (mask128(l) if l else 0))
        out.update((a, last, (a - 1) & full, (last + 1) & full))
    return sorted(out)


# ---- IPv4 LPM
PILES = (1, 2, 3, 4, 5, 13, 14, 15, 16, 40, 300)
TOWER4 = host4("20.60.165.195")
WIDE26, WIDE30 = 1 << 26, 1 << 30


@functools.lru_cache(None)
def lpm4_prefixes():
    """-> ([(host-order address, plen, label)], {/16 index: intended case})"""
    rng = np.random.default_rng(408)
    P, want = {}, {}

    def add(a, l, label=None):
        a &= mask4(l)
        if (a, l) in P:
            return 0
        P[(a, l)] = 1000 + len(P) if label is None else label
        return 1

    def pile(base, n, lo=17):
        k = 0
        while k < n:
            k += add(base | int(rng.integers(0, 1 << (32 - lo + 1))), int(rng.integers(lo, 33)))

    def relabel(d16, labels):
        """the longest prefixes of /16 d16 (the order the builder lists them)"""
        keys = sorted((k for k in P if k[0] >> 16 == d16 and k[1] > 16), key=lambda k: -k[1])
        for k, v in zip(keys, labels):
            P[k] = v
    for i, n in enumerate(PILES):
        d16 = 20 << 8 | (i + 1)
        pile(d16 << 16, n)
        want[d16] = ("inline", n) if n <= 2 else ("chunk", n) if n >= 15 else \
            ("list", (n - 1) + ((n - 1) & 1))
    # 40 prefixes of /25-/32 under one /24: chunk -> chunk -> leaf
    pile(host4("20.40.7.0"), 40, lo=25)
    want[20 << 8 | 40] = ("chunk", 40)
    # one address at every length: its /16 holds 16 longer prefixes
    for l in range(33):
        add(TOWER4, l, 3000 + l)
    want[TOWER4 >> 16] = ("chunk", 16)
    # a /12 and a /15 over the piles (the tower's /8 covers them all), piles
    # under the tower's /12 and /15, one outside 20.0.0.0/8
    add(host4("20.0.0.0"), 12, 3100)
    add(host4("20.2.0.0"), 15, 3101)
    for s, n in (("20.50.0.0", 3), ("20.61.0.0", 4), ("21.1.0.0", 3)):
        pile(host4(s), n)
        want[host4(s) >> 16] = ("list", (n - 1) + ((n - 1) & 1))
    # label 0 under a longer labelled prefix, over a shorter one
    add(host4("20.30.0.0"), 16, 500)
    add(host4("20.30.16.0"), 20, 0)
    add(host4("20.30.17.16"), 28, 501)
    want[20 << 8 | 30] = ("inline", 2)
    P[(TOWER4 & mask4(20), 20)] = 0
    # labels of 2^26 and more (a list entry's leaf goes through lbl_ovf) and
    # of 2^30 and more (so does a plain leaf), inline and in lists and chunks
    relabel(20 << 8 | 2, [WIDE26 + 11, WIDE30 + 12])                       # inline
    relabel(20 << 8 | 5, [WIDE30 + 21, WIDE26 + 22, WIDE26 + 23, WIDE30 + 24, WIDE26 + 25])
    relabel(20 << 8 | 7, [1900, WIDE26 + 31, WIDE30 + 32, 0, WIDE30 + 33])   # the 14-pile
    relabel(20 << 8 | 10, [WIDE30 + 41, 0, WIDE26 + 42, WIDE30 + 43])        # the 40-pile
    relabel(20 << 8 | 4, [S.HOST_ID, S.CLUSTER_ID])
    relabel(20 << 8 | 6, [1901, 0, S.CLUSTER_ID, S.HOST_ID])                 # the 13-pile
    return [(a, l, v) for (a, l), v in sorted(P.items())], want


def _lpm4_policy(labels):
    """per-label keys in both directions: L3 for odd labels, an L4 proxy
    redirect on tcp/80 for every third, nothing for the rest"""
    rows = []
    for v in sorted(set(int(x) for x in labels) - {0}):   # (identity 0: the wildcard key)
        for eg in (0, 1):
            if v % 2:
                rows.append((v, 0, 0, eg, 0))
            if v % 3 == 0:
                rows.append((v, 80, S.IPPROTO_TCP, eg, 10001 + eg))
    return pol_rows(rows)


@functools.lru_cache(None)
def _lpm4_tables():
    pfx, want = lpm4_prefixes()
    eps = endpoints4([S.LXC_IPV4, S.ip4("10.1.0.1"), S.ip4("10.1.0.2")])
    pol = _lpm4_policy([p[2] for p in pfx] + [S.WORLD_ID])
    t = S.Tables(ipc4(pfx), eps, {EP0 + i: pol for i in range(3)},
                 np.zeros(0, S.PREFILTER_DT), {EP0 + i: S.EP_SECLABEL for i in range(3)})
    return t


def lpm4_structural(order="grouped", direction="ingress"):
    """Every shape of the compact layout's /16 directory (and the same
    prefixes for DIR-24-8), probed at every prefix's boundary addresses.
    grouped: the probes of one /16 fill whole waves of 64; shuffled: every
    case in neighbouring lanes.  ingress: probes as sources; egress: as
    destinations of the first endpoint."""
    pfx, want = lpm4_prefixes()
    t = _lpm4_tables()
    probes = boundary4(pfx)
    groups = []
    for d16 in np.unique(probes >> 16):
        g = probes[probes >> 16 == d16]
        groups.append(np.resize(g, -(-len(g) // 64) * 64))
    host = np.concatenate(groups)
    if order == "shuffled":
        host = np.random.default_rng(16).permutation(host)
    k = np.arange(len(host))
    eps = S.local_v4_addrs(t)
    if direction == "ingress":
        h = hdr4(raw4(host), eps[k % 3], PORTS[(k // 3) % 4],
                 np.where(k % 5 == 4, S.IPPROTO_UDP, S.IPPROTO_TCP))
        mode, ep = 0, 0
    else:
        h = hdr4(S.LXC_IPV4, raw4(host), PORTS[k % 4],
                 np.where(k % 5 == 4, S.IPPROTO_UDP, S.IPPROTO_TCP))
        mode, ep = 1, EP0
    return Case(t, h, mode, ep, dict(prefixes=pfx, dir_cases=want, probes=probes, host=host))


# ---- IPv6 LPM
TOWER6 = int.from_bytes(bytes(S.ip6("2001:db8:1234:5678:9abc:def0:fed:cba9")), "big")


def _pile6(rng, base, blen, n, lens, label0):
    out, seen = [], set()
    while len(out) < n:
        l = int(rng.choice(lens))
        a = (base | int.from_bytes(rng.bytes(16), "big") & ~mask128(blen)) & mask128(l)
        if (a, l) not in seen:
            seen.add((a, l))
            out.append((a, l, label0 + len(out)))
    return out


def _last_slot_keys6(base_words, plen, count, label0, skip=0):
    """`count` keys of length plen homed at the last slot of their table: the
    word holding the prefix's last bits varies"""
    vary = (plen - 1) // 32
    sh = 32 * (vary + 1) - plen
    v = last_slot_l6(base_words, plen, vary, n=1 << 22, step=1 << sh)
    out = []
    for x in v[skip:skip + count]:
        w = list(base_words)
        w[vary] = int(x)
        for i in range(vary + 1, 4):
            w[i] = 0
        out.append((sum(w[i] << (96 - 32 * i) for i in range(4)), plen, label0 + len(out)))
    assert len(out) == count
    return out


@functools.lru_cache(None)
def _confuse6():
    """(X, l40, l44): X/40 and X/44 with the absent key (X, 48) a Bloom
    "maybe" homed at X/40's slot of a 16-slot slots64 — the probe for length
    48 of address X meets a slot with the same words and another length"""
    rng = np.random.default_rng(48)
    n = 1 << 21
    w0 = U64(0x2a000000) | rng.integers(0, 1 << 24, size=n).astype(np.uint64)
    w1 = rng.integers(0, 256, size=n).astype(np.uint64) << U64(24)
    h48, h44, h40 = (l6_hash(w0, w1, 0, 0, l) for l in (48, 44, 40))
    have = l6_bloom_bits(h44) | l6_bloom_bits(h40)
    ok = ((l6_bloom_bits(h48) & have) == l6_bloom_bits(h48)) & \
        ((h48 & U64(15)) == (h40 & U64(15))) & ((h44 & U64(15)) != (h40 & U64(15)))
    return [(int(a) << 96 | int(b) << 64) for a, b in zip(w0[ok], w1[ok])]


@functools.lru_cache(None)
def lpm6_prefixes(variant):
    """full: the tower /0-/128, piles under one /48 and one /64, wrapping
    chains in both slot arrays; short: prefixes of at most /64 only, no ::/0,
    with the length-confusion key; long: longer than /64 only, with ::/0"""
    rng = np.random.default_rng(600 + len(variant))
    P = []
    b48 = int.from_bytes(bytes(S.ip6("2001:db8:5::")), "big")
    b64 = int.from_bytes(bytes(S.ip6("2001:db8:6:7::")), "big")
    chain64 = _last_slot_keys6((0x20010db9, 0, 0, 0), 64, 5, 7000)
    chain128 = _last_slot_keys6((0x20010dba, 1, 2, 0), 128, 5, 7100)
    if variant == "full":
        for l in range(129):
            P.append((TOWER6 & (mask128(l) if l else 0), l, 0 if l == 77 else 4000 + l))
        P += _pile6(rng, b48, 48, 24, [56, 60, 64], 5000)
        P += _pile6(rng, b64, 64, 24, [96, 112, 120, 128], 5100)
        P += [(b48, 48, 5200), (b64, 64, 5201)]
        P += chain64 + chain128
    elif variant == "short":
        P += _pile6(rng, b48, 48, 24, [49, 56, 63, 64], 5000)
        P += _pile6(rng, 0x2b << 120, 8, 30, [12, 24, 31, 32, 33, 40], 5300)
        P += [(b48, 48, 5200), (0x2c << 120, 8, 0), (0x2c0f << 112, 16, 5400)]
        P += chain64
    else:
        assert variant == "long"
        P += _pile6(rng, b64, 64, 30, [65, 72, 95, 96, 97, 127, 128], 5100)
        P += chain128
        P += [(0, 0, 77)]
    return sorted(set(P))


def _v6_endpoint_tables(pfx):
    eps = np.concatenate([S.endpoint_v6(S.LXC_IPV6, 100, EP0)])
    labels = [p[2] for p in pfx] + [S.WORLD_ID]
    t = S.Tables(ipc6(pfx), eps, {EP0: _lpm4_policy(labels)}, np.zeros(0, S.PREFILTER_DT),
                 {EP0: S.EP_SECLABEL})
    return t


def lpm6_structural(variant="full"):
    """IPv6 LPM at the word boundaries, the Bloom-group boundaries and the
    ends of both slot arrays; probes as sources of ingress traffic."""
    return _lpm6_structural(variant)


@functools.lru_cache(None)
def _lpm6_structural(variant):
    pfx = lpm6_prefixes(variant)
    probes = boundary6(pfx)
    t = _v6_endpoint_tables(pfx)
    n = -(-max(len(probes), 2048) // len(probes)) * len(probes)
    src = np.stack([bytes6(x) for x in probes])
    k = np.arange(n)
    h = hdr6(src[k % len(probes)], S.LXC_IPV6, PORTS[(k // len(probes)) % 4])
    return Case(t, h, 0, 0, dict(prefixes=pfx, probes=probes, model=lpm6_model(pfx)))


@functools.lru_cache(None)
def lpm6_confusion():
    """The slots64 probe must compare the stored length: X/40 (label 6040)
    and X/44 (6044) with a third prefix of /48 elsewhere; address X probes
    length 48 first, whose absent key passes the Bloom filter and lands on
    X/40's slot.  The answer is X/44's label."""
    for x in _confuse6():
        pfx = [(x, 40, 6040), (x, 44, 6044), (0x2a << 120 | 0xbad << 80, 48, 6048)]
        m = lpm6_model(pfx)
        if m["groups"] == 1 and lpm6_model_lookup(m, x, check_len=False) == 6040 and \
                lpm6_model_lookup(m, x) == 6044:
            break
    else:
        raise AssertionError("no such key")
    probes = sorted(set(boundary6(pfx) + [x, x | 1, x | 0xFFFF << 64]))
    t = _v6_endpoint_tables(pfx)
    src = np.stack([bytes6(a) for a in probes])
    k = np.arange(2048)
    h = hdr6(src[k % len(probes)], S.LXC_IPV6, PORTS[(k // len(probes)) % 4])
    return Case(t, h, 0, 0, dict(prefixes=pfx, probes=probes, model=m, x=x))


# ---- endpoint tables outside LDS
ID_A, ID_B, ID_C = 300, 301, 302


def _ep_policy(i):
    rows = [(ID_A, 0, 0, 0, 0), (ID_B, 80, S.IPPROTO_TCP, 0, 10000 + i),
            (ID_A, 0, 0, 1, 0), (ID_B, 80, S.IPPROTO_TCP, 1, 20000 + i)]
    if i % 2 == 0:
        rows.append((S.EP_SECLABEL, 0, 0, 0, 0))
    return pol_rows(rows)


@functools.lru_cache(None)
def _v6_chain_addrs():
    """endpoint addresses beef::1:xxxx:xxxx homed at the last lxc6 slot"""
    w = list(raw_words6(S.LXC_IPV6))
    v = np.arange(1 << 22, dtype=np.uint32)
    raw3 = S.byteswap32(v).astype(np.uint64)
    ok = (l6_hash(w[0], w[1], w[2], raw3, L6_LXC_TAG) & U64(LAST16)) == LAST16
    out = []
    for x in v[ok]:
        a = S.LXC_IPV6.copy()
        a[12:] = np.frombuffer(int(x).to_bytes(4, "big"), np.uint8)
        out.append(a)
    return out


def endpoints_many(family=4, twin=False, direction="ingress"):
    """130 IPv4 / 66 IPv6 endpoints: the first counts at which the endpoint
    table is no longer copied to LDS (twin: 40 / 20, which is); five of them
    homed at the table's last slot, three absent addresses homed there too.
    ingress: traffic to every endpoint and to the absent addresses; egress:
    from an endpoint that sits at a wrapped position of the chain."""
    return _endpoints_many(family, bool(twin), direction)


@functools.lru_cache(None)
def _endpoints_many(family, twin, direction):
    n = (40 if twin else 130) if family == 4 else (20 if twin else 66)
    if family == 4:
        cand = last_slot_v4()
        chain, absent = [int(x) for x in cand[:5]], [int(x) for x in cand[5:8]]
        rest = [S.ip4(f"10.1.{i >> 8}.{i & 255}") for i in range(1, n - 4)]
        addrs = chain + rest
        eps = endpoints4(addrs)
        ipc = ipc4([(host4("30.0.0.0"), 24, ID_A), (host4("30.0.1.0"), 24, ID_B),
                    (host4("30.0.2.0"), 24, ID_C)])
        slots, where = lxc4_model(eps)
        srcs = raw4([host4("30.0.0.9"), host4("30.0.1.9"), host4("30.0.2.9")])
    else:
        cand = _v6_chain_addrs()
        chain, absent = cand[:5], cand[5:8]
        rest = []
        for i in range(1, n - 4):
            a = S.LXC_IPV6.copy()
            a[12:] = [0, 0, i >> 8, i & 255]
            rest.append(a)
        addrs = chain + rest
        eps = np.concatenate([S.endpoint_v6(a, 100 + i, EP0 + i) for i, a in enumerate(addrs)])
        b = int.from_bytes(bytes(S.ip6("2001:db8:a::")), "big")
        ipc = ipc6([(b, 64, ID_A), (b + (1 << 64), 64, ID_B), (b + (2 << 64), 64, ID_C)])
        slots, where = lxc6_model(eps)
        srcs = np.stack([bytes6(b + 9), bytes6(b + (1 << 64) + 9), bytes6(b + (2 << 64) + 9)])
        where = {bytes(k): v for k, v in where.items()}
    assert len(addrs) == n
    t = S.Tables(ipc, eps, {EP0 + i: _ep_policy(i) for i in range(n)},
                 np.zeros(0, S.PREFILTER_DT), {EP0 + i: S.EP_SECLABEL for i in range(n)})
    key = (lambda a: int(a)) if family == 4 else (lambda a: bytes(a))
    chain_slots = [where[key(a)] for a in chain]
    # the chain endpoint the egress traffic comes from: one past the wrap
    sender = next(i for i, s in enumerate(chain_slots) if s < len(slots) // 2)
    claims = dict(n=n, slots=len(slots), chain=chain, absent=absent, chain_slots=chain_slots,
                  sender=sender, in_lds=len(slots) <= (LXC_LDS_MAX_SLOTS if family == 4
                                                      else LXC6_LDS_MAX_SLOTS))
    mk = hdr4 if family == 4 else hdr6
    dsts = addrs + absent
    dst = np.array(dsts, np.uint32) if family == 4 else np.stack(dsts)
    if direction == "ingress":
        k = np.arange(6 * len(dsts))
        h = mk(srcs[k % 3], dst[k // 6], PORTS[(k // 3) % 2])
        return Case(t, tile(h, 4 * len(h), seed=13), 0, 0, claims)
    # egress: valid source, the absent sources and another chain endpoint's
    t = endpoints_many(family, twin, "ingress").tables      # (one table set per shape)
    remote = raw4([host4("30.0.0.7"), host4("30.0.1.7"), host4("30.0.2.7"), host4("9.9.9.9")]) \
        if family == 4 else np.stack([srcs[0], srcs[1], srcs[2], bytes6(0x2009 << 112 | 9)])
    dst = np.concatenate([remote, dst[:12], dst[-3:]])
    src_list = [chain[sender]] * 4 + absent[:1] + [chain[(sender + 1) % 5]]
    src = np.array(src_list, np.uint32) if family == 4 else np.stack(src_list)
    k = np.arange(len(src) * len(dst))
    h = mk(src[k % len(src)], dst[k // len(src)], PORTS[(k // 5) % 2])
    return Case(t, tile(h, 3072, seed=14), 1, EP0 + sender, claims)


# ---- policy tables
@functools.lru_cache(None)
def policy_chains():
    """Three endpoints; the middle one's policy table has three L4 and two L3
    keys homed at its last slot (the chain wraps into slots 0-3), the same
    keys sit in the next endpoint's table with other proxy ports, and absent
    keys homed into the chain are looked up too."""
    l4 = [int(x) for x in last_slot_policy_ids(int(S.htons(80)), S.IPPROTO_TCP, 0)[:5]]
    l3 = [int(x) for x in last_slot_policy_ids(0, 0, 0)[:3]]
    present4, absent4, present3, absent3 = l4[:3], l4[3:], l3[:2], l3[2:]
    fill = [901, 902, 903]

    def table(e, keys=True):
        rows = [(f, 0, 0, 0, 0) for f in fill[:3 if keys else 2]] + \
               [(fill[0], 443, S.IPPROTO_TCP, 0, 9000 + e)]
        if keys:
            rows += [(i, 80, S.IPPROTO_TCP, 0, 11000 + 100 * e + k) for k, i in enumerate(present4)]
            rows += [(i, 0, 0, 0, 0) for i in present3]
        return pol_rows(rows)
    pol = {EP0: table(0, keys=False), EP0 + 1: table(1), EP0 + 2: table(2)}
    idents = present4 + absent4 + present3 + absent3 + fill
    pfx = [(host4("30.1.0.0") + k, 32, v) for k, v in enumerate(idents)]
    eps = endpoints4([S.ip4("10.1.0.1"), S.ip4("10.1.0.2"), S.ip4("10.1.0.3")])
    t = S.Tables(ipc4(pfx), eps, pol, np.zeros(0, S.PREFILTER_DT),
                 {EP0 + i: S.EP_SECLABEL for i in range(3)})
    src = raw4([p[0] for p in pfx])
    k = np.arange(len(src) * 3 * 3)
    ident = np.array(idents)[k % len(src)]
    h = hdr4(src[k % len(src)], S.local_v4_addrs(t)[(k // len(src)) % 3],
             np.array([80, 81, 443])[k // (3 * len(src))])
    claims = dict(present4=present4, absent4=absent4, present3=present3, absent3=absent3,
                  ident=ident, ep=(k // len(src)) % 3, dport=np.array([80, 81, 443])[k // (3 * len(src))],
                  model=policy_model(pol))
    hh = tile(h, 64 * len(h))
    claims["index"] = np.arange(len(hh)) % len(h)
    return Case(t, hh, 0, 0, claims)


FB_ID, FB_OTHER = 777, 778


def _fallback_policy(subset, e):
    rows = []
    for eg in (0, 1):
        if subset & 1:
            rows.append((FB_ID, 80, S.IPPROTO_TCP, eg, 11000 + e + 500 * eg))
        if subset & 2:
            rows.append((FB_ID, 0, 0, eg, 13000 + e + 500 * eg))
        if subset & 4:
            rows.append((0, 80, S.IPPROTO_TCP, eg, 12000 + e + 500 * eg))
    return pol_rows(rows)


def policy_fallback(direction="ingress", empty=False, sender=0):
    """Eight endpoints, one per subset of {L4, L3, wildcard port} of the
    keys of (identity 777, tcp/80), each key with a proxy port of its own
    (subset 0: an empty policy map); with and without the fragment flag; a
    second identity and a second port that match less.  empty: no endpoint
    has a key, so the epoch has no policy Bloom filter.  egress: from
    endpoint `sender`."""
    return _policy_fallback(direction, bool(empty), sender)


@functools.lru_cache(None)
def _policy_fallback(direction, empty, sender):
    eps = endpoints4([S.ip4(f"10.2.0.{e + 1}") for e in range(8)])
    pol = {EP0 + e: _fallback_policy(0 if empty else e, e) for e in range(8)}
    pfx = [(host4("30.2.0.1"), 32, FB_ID), (host4("30.2.0.2"), 32, FB_OTHER)]
    t = S.Tables(ipc4(pfx), eps, pol, np.zeros(0, S.PREFILTER_DT),
                 {EP0 + e: S.EP_SECLABEL for e in range(8)})
    k = np.arange(64)
    remote = raw4([host4("30.2.0.1"), host4("30.2.0.2")])[k % 2]
    dport = np.array([80, 81])[(k // 2) % 2]
    flags = np.where((k // 4) % 2, S.HF_FRAG, 0)
    e = k // 8
    claims = dict(subset=e, frag=flags != 0, ident=np.array([FB_ID, FB_OTHER])[k % 2],
                  dport=dport, model=policy_model(pol))
    if direction == "ingress":
        h = hdr4(remote, S.local_v4_addrs(t)[e], dport, flags=flags)
        hh = tile(h, 3200)
        claims["index"] = np.arange(3200) % 64
        return Case(t, hh, 0, 0, claims)
    t = policy_fallback("ingress", empty).tables            # (one table set per shape)
    h = hdr4(S.local_v4_addrs(t)[sender], remote, dport, flags=flags)
    hh = tile(S.take(h, np.arange(8)), 512)
    claims["index"] = np.arange(512) % 8
    return Case(t, hh, 1, EP0 + sender, claims)


@functools.lru_cache(None)
def policy_bloom_fp():
    """One endpoint with 200 keys; found in the model of its Bloom filter:
    (a) an absent L4 key the filter answers "maybe", its L3 key present;
    (b) the same with nothing after it (DROP_POLICY); (c) one whose home slot
    another key occupies (the walk passes it)."""
    base = [(1000 + i, 0, 0, 0, 0) if i % 2 else (1000 + i, 80, S.IPPROTO_TCP, 0, 15000 + i)
            for i in range(200)]
    hi = int(S.htons(80)) | S.IPPROTO_TCP << 16

    def fps(pol, need_occupied):
        model, bloom = policy_model({EP0: pol})
        ids = np.arange(2000, 1 << 22, dtype=np.uint64)
        pre = pol_key_pre(ids, hi)
        h = pol_bloom_hash(pol_bloom_salt(0), pre)
        b = bloom_bits(h)
        ok = (bloom[(h & U64(len(bloom) - 1)).astype(np.int64)] & b) == b
        occ = np.array([s is not None for s in model[EP0]["slots"]])
        ok &= occ[(pre & U64(model[EP0]["mask"])).astype(np.int64)] == need_occupied
        return [int(x) for x in ids[ok][:64]]
    id_a = fps(pol_rows(base), False)[0]
    pol = pol_rows(base + [(id_a, 0, 0, 0, 0)])
    model, bloom = policy_model({EP0: pol})
    id_b = next(x for x in fps(pol, False) if x != id_a and not pol_maybe(model, bloom, EP0, x, 0))
    id_c = next(x for x in fps(pol, True) if not pol_maybe(model, bloom, EP0, x, 0))
    idents = [id_a, id_b, id_c, 1000, 1001, 1199]
    pfx = [(host4("30.3.0.0") + k, 32, v) for k, v in enumerate(idents)]
    eps = endpoints4([S.LXC_IPV4])
    t = S.Tables(ipc4(pfx), eps, {EP0: pol}, np.zeros(0, S.PREFILTER_DT), {EP0: S.EP_SECLABEL})
    k = np.arange(len(idents) * 2)
    h = hdr4(raw4([p[0] for p in pfx])[k % len(idents)], S.LXC_IPV4,
             np.array([80, 8080])[k // len(idents)])
    hh = tile(h, 3072)
    claims = dict(id_a=id_a, id_b=id_b, id_c=id_c, hi=hi, model=(model, bloom),
                  ident=np.array(idents)[np.arange(3072) % len(k) % len(idents)],
                  dport=np.array([80, 8080])[np.arange(3072) % len(k) // len(idents)])
    return Case(t, hh, 0, 0, claims)


# ---- prefilter
def _pf_rows(exact=(), dyn=(), exact6=(), dyn6=()):
    """exact: be32-raw addresses; dyn: (host-order address, plen); exact6:
    128-bit ints; dyn6: (128-bit int, plen)"""
    n = len(exact) + len(dyn) + len(exact6) + len(dyn6)
    pf = np.zeros(n, S.PREFILTER_DT)
    i = 0
    for a in exact:
        pf[i] = (1, 32, np.frombuffer(int(a).to_bytes(4, "little") + bytes(12), np.uint8), 0)
        i += 1
    for a, l in dyn:
        pf[i] = (1, l, np.frombuffer((a & mask4(l)).to_bytes(4, "big") + bytes(12), np.uint8), 1)
        i += 1
    for a in exact6:
        pf[i] = (2, 128, bytes6(a), 0)
        i += 1
    for a, l in dyn6:
        pf[i] = (2, l, bytes6(a & (mask128(l) if l else 0)), 1)
        i += 1
    return pf


DYN4_TOWER = [(0xFFFFFFFF, l) for l in range(1, 8)] + \
             [(l << 24 | 0x5A5A5A, l) for l in range(8, 33)]
DYN4_SPREAD = [(host4("64.0.0.0"), 2), (host4("160.0.0.0"), 3), (host4("208.0.0.0"), 4),
               (host4("8.0.0.0"), 5), (host4("20.0.0.0"), 6), (host4("26.0.0.0"), 7)] + \
              [((216 + l) << 24 | 0xA5A5A5, l) for l in range(8, 33)]
DYN6 = [(1 << (128 - l), l) for l in range(1, 8)] + \
       [((1 << 128) - 1, l) for l in range(8, 16)] + \
       [((0x0100 + l) << 112 | 0x5A5A5A5A5A5A5A5A5A5A5A5A5A5A, l) for l in range(16, 129)]


@functools.lru_cache(None)
def _pf4_fp(nb, words, have):
    """an absent 10.x address, "maybe" in a filter of `words` words holding
    the addresses `have`, homed at the last of nb buckets"""
    bloom = np.zeros(words, np.uint64)
    for a in have:
        h = int(pf_bloom_hash(a))
        bloom[h & (words - 1)] |= bloom_bits(h)
    host = np.uint32(10 << 24) + np.arange(1 << 24, dtype=np.uint32)
    raw = S.byteswap32(host)
    h = pf_bloom_hash(raw)
    b = bloom_bits(h)
    ok = ((bloom[(h & U64(words - 1)).astype(np.int64)] & b) == b) & \
        (hash32(raw, nb - 1) == nb - 1) & ~np.isin(raw, np.array(have, np.uint32))
    return int(raw[ok][0])


def prefilter_edges(family=4, variant="spill1", mode=2):
    """IPv4 variants — spill1: 5 exact addresses homed at the last bucket
    (one spill into bucket 0) and an absent "maybe" homed there; spill2: 9
    (two spills) beside 0.0.0.0/32, with dynamic prefixes /1-/32; zero: the
    deny set {0.0.0.0/32} alone; dyn: dynamic prefixes alone.  IPv6 — spill:
    5 exact addresses homed at the last slot, ::/128 and an absent "maybe";
    dyn: prefixes /1-/128 beside ::/128.  Sources at every boundary.  mode:
    XDP (2) or FULL (3)."""
    t, h, claims = _prefilter(family, variant)
    return Case(t, h, mode, 0, claims)


@functools.lru_cache(None)
def _prefilter(family, variant):
    claims = {}
    if family == 4:
        cand = [int(x) for x in last_slot_v4()]
        other = [int(x) for x in raw4([host4("50.0.0.1"), host4("50.0.0.2"), host4("50.0.0.3")])]
        exact, dyn = [], []
        if variant == "spill1":
            exact = cand[8:13] + other
        elif variant == "spill2":
            exact, dyn = cand[8:17] + other + [0], DYN4_TOWER
        elif variant == "zero":
            exact = [0]
        else:
            assert variant == "dyn"
            dyn = DYN4_SPREAD
        pf = _pf_rows(exact, dyn)
        model = pf_fix_model(pf)
        probes = set([0, 1, int(raw4(1)), 0xFFFFFFFF, int(raw4(host4("50.0.0.4")))])
        for a in exact:
            hst = int(S.byteswap32(a))
            probes.update(int(raw4((hst + d) & 0xFFFFFFFF)) for d in (-1, 0, 1))
        if model["buckets"] is not None:
            nz = [a for a in exact if a]
            fp = _pf4_fp(len(model["buckets"]), len(model["bloom"]), tuple(nz))
            probes.add(fp)
            claims["fp"] = fp
            probes.update(cand[20:23])        # absent, homed there, mostly screened
        probes.update(int(x) for x in raw4(boundary4([(a & mask4(l), l, 1) for a, l in dyn])))
        src = np.array(sorted(probes), np.uint32)
        eps = endpoints4([S.LXC_IPV4])
        t = S.Tables(ipc4([(host4("50.0.0.0"), 8, 350), (host4("10.0.0.0"), 8, 351)]), eps,
                     {EP0: pol_rows([(350, 0, 0, 0, 0), (351, 80, S.IPPROTO_TCP, 0, 10001)])},
                     pf, {EP0: S.EP_SECLABEL})
        h = hdr4(src, S.LXC_IPV4, 80)
        claims.update(model=model, src=src, chain=[a for a in exact if a in cand])
    else:
        zero6 = 0
        base = (0x20010dbb, 3, 4, 0)
        chain = [k[0] for k in _last_slot_keys6(base, 128, 8, 1)]
        others = [0x2001 << 112 | 0x50 << 64 | i for i in (1, 2, 3)]
        if variant == "spill":
            exact, dyn = chain[:5] + others + [zero6], []
        else:
            assert variant == "dyn"
            exact, dyn = [zero6], DYN6
        pf = _pf_rows(exact6=exact, dyn6=dyn)
        m = lpm6_model([(a, 128, 1) for a in exact])
        full = (1 << 128) - 1
        probes = set([0, 1, full, 0x2001 << 112 | 0x50 << 64 | 4])
        for a in exact:
            probes.update(((a - 1) & full, a, (a + 1) & full))
        probes.update(boundary6([(a, l, 1) for a, l in dyn]))
        if variant == "spill":
            words = bloom_words(2 * len(exact), PF_BLOOM_MAX_WORDS)
            bloom = np.zeros(words, np.uint64)
            for a in exact:
                hh = int(pf6_bloom_hash(*words_of(a)))
                bloom[hh & (words - 1)] |= bloom_bits(hh)
            # absent, "maybe" in the address filter, homed at the last slot
            v = np.arange(1 << 24, dtype=np.uint64)
            hb = pf6_bloom_hash(base[0], base[1], base[2], v)
            b = bloom_bits(hb)
            ns = len(m["slots"])
            ok = ((bloom[(hb & U64(words - 1)).astype(np.int64)] & b) == b) & \
                ((l6_hash(base[0], base[1], base[2], v, 128) & U64(ns - 1)) == ns - 1)
            fp = [sum(w << (96 - 32 * i) for i, w in enumerate(base[:3])) | int(x) for x in v[ok]]
            fp = [x for x in fp if x not in exact][0]
            probes.add(fp)
            probes.update(chain[5:8])
            claims.update(fp=fp, bloom=bloom)
        srcl = sorted(probes)
        t = S.Tables(ipc6([(0x2001 << 112, 16, 350)]),
                     np.concatenate([S.endpoint_v6(S.LXC_IPV6, 100, EP0)]),
                     {EP0: pol_rows([(350, 0, 0, 0, 0), (S.WORLD_ID, 0, 0, 0, 0)])}, pf,
                     {EP0: S.EP_SECLABEL})
        h = hdr6(np.stack([bytes6(x) for x in srcl]), S.LXC_IPV6, 80)
        claims.update(model=m, src=srcl, chain=[a for a in exact if a in chain])
    n = -(-2048 // len(h)) * len(h)
    return t, tile(h, n), claims
