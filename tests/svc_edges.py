"""Cases of the service step's packet-order pass (svcorder.hip k_svo_mark /
k_svo_replay, its consumers lb.hip k_lb4_egress and classify6.hip lb6_egress,
the apply's k_cta_lb / k_cta_svc in ctapply.hip; DESIGN.md "The service step
in packet order"), built with numpy and the oracle alone:
test_svc_edges.py checks on the CPU that each stream holds what it claims,
test_gpu_svc_edges.py runs them through the engine and asserts the exact
cfc_stats.svc_ordered this file's restatement of the pass gives.

Restated here from the C++: the layout.h mixers (fmix32, ct_hash4 / ct_hash6:
the list's fingerprints; ct_home4 / ct_home6: the apply's grouping), pinned
by `selftest kat svchash`; the CT_SERVICE key words (d, s, z, w) of a header
(kern_common.hpp ct_probe), pinned by the oracle's CT dump; svo_reach's gates
and svc_next4/6, pinned by the oracle's packet order (the slaves Pass.batch
hands on are the backends Oracle.run_sequential reaches).

The tables: synth.config_c2 / config_c3 with ~2000 prefixes and hand-written
services (VIPs 172.20.0.k / fd00:5ec0::k):
  a, b, c   L3 services (dport 0: every port and ICMP) of 3, 5, 4 backends
  l4        port 80, 3 backends
  gap       port 80, count 3, slot 2 absent; the fall-back lookup (the key as
            it stands, slave 2: lb.h:737-744) finds {vip, 0, 2} with count 4,
            so a re-selection is hash % 4 + 1, and 2 is the gone slot again
  none      port 80, count 3, slot 2 absent, nothing under the L3 key:
            DROP_NO_SERVICE
  lo        (IPv4) port 80, its one backend the sending endpoint
  deny      port 80, two backends of one identity the egress policy denies
The CT maps hold a history the oracle ran while gap still had its slot 2:
three flows stored with slave 2 (sports 41000, 41001, 41003; the last one's
entry has lb_loopback set by hand, IPv4 only), and a few established flows.

An ICMP header's sport holds [type, code] as bytes (the type is the low
byte), its dport the next two bytes (an echo's identifier)."""
import copy
import dataclasses

import numpy as np

import oracle as O
from cilium_amd import synth as S

EGRESS = 1
EP = S.EP_LXC_ID
TCP, UDP = S.IPPROTO_TCP, S.IPPROTO_UDP
M32 = 0xFFFFFFFF
GOLD = 0x9E3779B9
DROP_NO_SERVICE, DROP_POLICY = -158, -133


# ------------------------------------------------------------- the mixers
def fmix32(h):
    h &= M32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    return h ^ h >> 16


def ct_hash4(x, y, z, w):
    h = fmix32(x ^ GOLD)
    h = fmix32(h ^ y)
    h = fmix32(h ^ z)
    return fmix32(h ^ w)


def _fold6(d, s):
    """ct_hash6 up to its outer ct_hash4: the addresses' part"""
    h = ct_hash4(*d)
    for x in s:
        h = fmix32(h ^ x)
    return h


def ct_hash6(d, s, z, w):
    return ct_hash4(_fold6(d, s), z, w, 0x7F4A7C15)


def _pair(z):
    pa, pb = z & 0xFFFF, z >> 16
    return min(pa, pb) | max(pa, pb) << 16


def ct_home4(x, y, z, w):
    return ct_hash4(min(x, y), max(x, y), _pair(z), w & ~0x100 & M32)


def ct_home6(d, s, z, w):
    hd, hs = ct_hash4(*d), ct_hash4(*s)
    return ct_hash4(min(hd, hs), max(hd, hs), _pair(z), (w & ~0x100 & M32) ^ 0x7F4A7C15)


def khash(key):
    d, s, z, w = key
    return ct_hash6(d, s, z, w) if isinstance(d, tuple) else ct_hash4(d, s, z, w)


def khome(key):
    d, s, z, w = key
    return ct_home6(d, s, z, w) if isinstance(d, tuple) else ct_home4(d, s, z, w)


# ----------------------------------------------------------- the key words
def ct_word(nexthdr, flags, owner=0):
    return nexthdr | (flags & 7) << 8 | owner


def addr_words(a, family):
    """an address as the kernels load it: one little-endian word of the
    network bytes, four for IPv6"""
    if family == 4:
        return int(a)
    b = bytes(np.asarray(a, np.uint8))
    return tuple(int.from_bytes(b[4 * k:4 * k + 4], "little") for k in range(4))


def service_zw(family, proto, pt, owner=0):
    """kern_common.hpp ct_probe(CT_SERVICE): z = tuple bytes 8-11 (the L4
    word as loaded; ICMP: the echo type on the side that sent the echo), w =
    ct_word(nexthdr, TUPLE_F_SERVICE | RELATED for an ICMP error, owner)"""
    fl = 4
    if proto in (TCP, UDP):
        td, ts = pt & 0xFFFF, pt >> 16
    else:
        typ = pt & 0xFF
        related = (1 <= typ <= 4) if family == 6 else typ in (3, 11, 12)
        echo, reply = (128, 129) if family == 6 else (8, 0)
        td = echo if (not related and typ == reply) else 0
        ts = echo if (not related and typ == echo) else 0
        fl |= 2 if related else 0
    return td | ts << 16, ct_word(proto, fl, owner)


def _pt(h, i):
    return int(h.sport[i]) | int(h.dport[i]) << 16


def key_words(h, i, owner=0):
    """the CT_SERVICE key (d, s, z, w) of header i, as svo_reach builds it"""
    z, w = service_zw(h.family, int(h.proto[i]), _pt(h, i), owner)
    return addr_words(h.daddr[i], h.family), addr_words(h.saddr[i], h.family), z, w


def ct_service_keys(ct, family):
    """the CT_SERVICE entries of CT_DT records (or CT dump rows through
    synth.ct_from_rows) -> {(d, s, z, w): (slave, lb_loopback)}"""
    out = {}
    al = 4 if family == 4 else 16
    for r in ct[ct["family"] == (1 if family == 4 else 2)]:
        tp = bytes(r["tuple"])
        nexthdr, fl = tp[2 * al + 4], tp[2 * al + 5]
        if not fl & 4:
            continue
        lxc = int(r["lxc"])
        owner = 0 if lxc < 0 else (1 << 11 | lxc << 16)
        if family == 4:
            d, s = int.from_bytes(tp[0:4], "little"), int.from_bytes(tp[4:8], "little")
        else:
            d = addr_words(np.frombuffer(tp[0:16], np.uint8), 6)
            s = addr_words(np.frombuffer(tp[16:32], np.uint8), 6)
        z = int.from_bytes(tp[2 * al:2 * al + 4], "little")
        e = bytes(r["entry"])
        # struct ct_entry (common.h:380-406): the bitfield at 36 (lb_loopback
        # is bit 3), rev_nat_index at 38, slave at 40
        out[(d, s, z, ct_word(nexthdr, fl, owner))] = (int.from_bytes(e[40:42], "little"),
                                                       (e[36] >> 3) & 1)
    return out


# -------------------------------------------------- the pass, restated
class Lb:
    """cilium_lb{4,6}_services as lb4_get / lb4_service read it"""

    def __init__(self, rows, family):
        self.family = family
        self.m = {}
        for r in rows:
            self.m[(addr_words(r["addr"], family), int(r["dport"]), int(r["slave"]))] = \
                int(r["count"])

    def get(self, addr, dport, slave):
        return self.m.get((addr, dport, slave))

    def service(self, addr, dport, slave):
        """lb4_lookup_service (lb.h:604-635): the L4 key while its dport is
        set, then the L3 key; count must be nonzero -> (key dport, count)"""
        if dport:
            c = self.get(addr, dport, slave)
            if c:
                return dport, c
        c = self.get(addr, 0, slave)
        return (0, c) if c else None


def svc_next(lb, da, proto, pt, hash_, e):
    """kern_common.hpp svc_next4/6: the entry e = (exists, slave) as the
    header finds it -> as it leaves it, and whether it re-selected"""
    kd = pt >> 16 if proto in (TCP, UDP) else 0
    m = lb.service(da, kd, 0)
    if not m:
        return e, False
    kd, count = m
    slave = e[1] if e[0] else hash_ % count + 1          # lb4_select_slave
    again = False
    if lb.get(da, kd, slave) is None:
        f = lb.service(da, kd, slave)
        if f:
            slave, again = hash_ % f[1] + 1, True         # ct_update4_slave
    return (True, slave), again


@dataclasses.dataclass
class Plan:
    listed: np.ndarray     # the header passes svo_reach's gates
    marked: np.ndarray     # ... and is handed an override word
    slave: np.ndarray      # the slave in that word (0: none)
    keys: list             # the listed headers' keys, None for the others
    unstable: list         # the keys listed (in order of first appearance)
    reselect: np.ndarray   # the header re-selects (ct_update4/6_slave)
    svc_ordered: int       # cfc_stats.svc_ordered's increase


class Pass:
    """svcorder.hip's pass over one batch after another: the CT_SERVICE
    entries as the batches leave them carry over (cfc_ct_apply)"""

    def __init__(self, t, family, ep=EP):
        self.family, self.ep = family, ep
        self.lb = Lb(t.lb4 if family == 4 else t.lb6, family)
        self.entry = ct_service_keys(t.ct, family)
        fam = 1 if family == 4 else 2
        e = t.endpoints
        self.src = {addr_words(int.from_bytes(bytes(r["addr"][:4]), "little") if family == 4
                               else r["addr"], family): int(r["lxc_id"])
                    for r in e[e["family"] == fam]}
        self.router = addr_words(S.ROUTER_IPV6, 6)

    def reach(self, h, i):
        """svo_reach's gates -> the header's key, or None"""
        proto = int(h.proto[i])
        icmp = S.IPPROTO_ICMPV6 if self.family == 6 else S.IPPROTO_ICMP
        if proto not in (TCP, UDP, icmp):
            return None
        key = key_words(h, i)
        pt = _pt(h, i)
        if self.family == 6 and proto == icmp and not int(h.flags[i]) & S.HF_EXTHDR:
            typ = pt & 0xFF
            if typ == 135 or (typ == 128 and key[0] == self.router):
                return None   # icmp6_handle answers it
        if self.src.get(key[1]) != self.ep:
            return None       # is_valid_lxc_src_ip
        if not self.lb.service(key[0], pt >> 16 if proto in (TCP, UDP) else 0, 0):
            return None
        return key

    def stable(self, key, proto, pt):
        if key not in self.entry:
            return False
        kd, _ = self.lb.service(key[0], pt >> 16 if proto in (TCP, UDP) else 0, 0)
        return self.lb.get(key[0], kd, self.entry[key][0]) is not None

    def batch(self, h):
        n = len(h)
        hs = h.hash if h.hash is not None else O.flow_hash(h, np.arange(n))
        p = Plan(np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, np.uint32), [None] * n, [],
                 np.zeros(n, bool), 0)
        runs = {}
        for i in range(n):
            key = self.reach(h, i)
            if key is None:
                continue
            p.keys[i] = key
            if self.stable(key, int(h.proto[i]), _pt(h, i)):
                continue
            p.listed[i] = True
            runs.setdefault(key, []).append(i)
        for key, idx in runs.items():
            p.unstable.append(key)
            have = self.entry.get(key)
            e = (have is not None, have[0] if have else 0)
            for k, i in enumerate(idx):
                if k:
                    p.marked[i], p.slave[i] = True, e[1]
                e, p.reselect[i] = svc_next(self.lb, key[0], int(h.proto[i]), _pt(h, i),
                                            int(hs[i]), e)
            self.entry[key] = (e[1], have[1] if have else 0)
            p.svc_ordered += len(idx) - 1
        return p


def sorted_list(h, plan):
    """the list k_svo_replay walks: (fingerprint, header index) of the listed
    headers, sorted -> that list and its runs of equal fingerprints as
    (first, last) positions"""
    lst = sorted((khash(plan.keys[i]), int(i)) for i in np.flatnonzero(plan.listed))
    runs, a = [], 0
    for r in range(1, len(lst) + 1):
        if r == len(lst) or lst[r][0] != lst[a][0]:
            runs.append((a, r - 1))
            a = r
    return lst, runs


# -------------------------------------------------------------- the tables
@dataclasses.dataclass
class Env:
    family: int
    t: S.Tables
    vip: dict             # service name -> VIP
    count: dict           # service name -> master count
    backends: dict        # service name -> {slave: target}
    own: object           # the sending endpoint's address
    other: object         # another endpoint's address (an invalid source here)
    deny_identity: int


SERVICES = ("a", "b", "c", "l4", "gap", "none", "lo", "deny")
COUNT = {"a": 3, "b": 5, "c": 4, "l4": 3, "gap": 3, "none": 3, "lo": 1, "deny": 2}
PORT = {"a": 0, "b": 0, "c": 0}     # the others: 80
GAP_FALLBACK_COUNT = 4
HIST_SPORT = {"i": 41000, "ii": 41001, "loop": 41003}
HIST_STABLE = range(40000, 40008)     # established flows to a
_env = {}


def _vip(family, k):
    if family == 4:
        return np.uint32((S.SVC_NET + (k << 24)) & M32)
    a = S.SVC6_NET.copy()
    a[15] = k
    return a


def _allow(t, idents):
    """L3 allow entries, both directions, for `idents` and the reserved
    identities, in every endpoint's policy (test_gpu_lb._allow_most)"""
    for lxc, pol in t.policy.items():
        one = np.zeros(len(idents) + 4, S.POLICY_DT)
        one["identity"][:len(idents)] = idents
        one["identity"][len(idents):] = [S.WORLD_ID, S.CLUSTER_ID, S.HOST_ID, S.EP_SECLABEL]
        add = np.concatenate([one, one])
        add["egress"][len(one):] = 1
        have = {(int(r["identity"]), int(r["dport"]), int(r["proto"]), int(r["egress"]))
                for r in pol}
        add = add[[(int(r["identity"]), 0, 0, int(r["egress"])) not in have for r in add]]
        t.policy[lxc] = np.concatenate([pol, add])


def env(family):
    """the tables with their history, built once per family"""
    if family in _env:
        return _env[family]
    v6 = family == 6
    if v6:
        t = S.config_c3(23, n_prefixes=2000, n_v4_prefixes=500, n_policy=300, n_endpoints=2,
                        n_prefilter=0)
    else:
        t = S.config_c2(22, n_prefixes=2000, n_policy=300, n_endpoints=2)
    rng = np.random.default_rng(220 + family)
    ipc = t.ipcache[t.ipcache["family"] == (2 if v6 else 1)]
    draw = S._addr_in_prefix_v6 if v6 else S._addr_in_prefix_v4
    o = O.Oracle(t)
    own = np.asarray(S.LXC_IPV6, np.uint8) if v6 else np.uint32(S.LXC_IPV4)
    loc = S.local_v6_addrs(t) if v6 else S.local_v4_addrs(t)
    other = loc[1]
    assert addr_words(other, family) != addr_words(own, family)

    # remote backends with an identity; the denied service's two share one
    # that no other backend has and no policy entry names
    pool = draw(rng, ipc, rng.integers(0, len(ipc), size=64))
    lab, hit = o.ipcache_lookup(family, pool)
    pool, lab = pool[(hit != 0) & (lab > 255)], lab[(hit != 0) & (lab > 255)]
    named = set(int(x) for p in t.policy.values() for x in p["identity"])
    deny = None
    for k in range(len(ipc)):
        two = draw(rng, ipc, np.array([k, k]))
        l2, h2 = o.ipcache_lookup(family, two)
        if h2.all() and l2[0] == l2[1] and l2[0] > 255 and int(l2[0]) not in named and \
                addr_words(two[0], family) != addr_words(two[1], family):
            deny = (two, int(l2[0]))
            break
    assert deny is not None
    keep = lab != deny[1]
    pool, lab = pool[keep], lab[keep]
    assert len(pool) >= 24
    _allow(t, np.unique(lab))

    dt = S.LB6_DT if v6 else S.LB4_DT
    rdt = S.REVNAT6_DT if v6 else S.REVNAT4_DT
    rows, rns = [], []

    def put(r, f, a):
        if v6:
            r[f][0] = a
        else:
            r[f] = a

    def row(addr, dport, slave, target=None, count=0, rev=0):
        r = np.zeros(1, dt)
        put(r, "addr", addr)
        if target is not None:
            put(r, "target", target)
        r["dport"], r["slave"], r["count"], r["rev_nat"] = dport, slave, count, rev
        rows.append(r)

    p80 = int(S.htons(80))
    vip, backends, nxt = {}, {}, 0
    for k, name in enumerate(SERVICES, start=1):
        if name == "lo" and v6:
            continue
        vip[name] = _vip(family, k)
        dport = int(S.htons(PORT.get(name, 80)))
        row(vip[name], dport, 0, count=COUNT[name], rev=k)
        rn = np.zeros(1, rdt)
        put(rn, "addr", vip[name])
        rn["index"], rn["port"] = k, dport
        rns.append(rn)
        backends[name] = {}
        for j in range(1, COUNT[name] + 1):
            if name == "none" and j == 2:
                continue
            if name == "lo":
                tgt = own
            elif name == "deny":
                tgt = deny[0][j - 1]
            else:
                tgt, nxt = pool[nxt], nxt + 1
            backends[name][j] = tgt
            row(vip[name], dport, j, target=tgt, rev=k)
    # gap's fall-back: slot 2 under the L3 key, with a count of its own
    row(vip["gap"], 0, 2, target=pool[nxt], count=GAP_FALLBACK_COUNT, rev=SERVICES.index("gap") + 1)
    full = np.concatenate(rows)
    rn = np.concatenate(rns)
    if v6:
        t.lb6, t.revnat6 = full, rn
    else:
        t.lb4, t.revnat4 = full, rn
    e = Env(family, t, vip, dict(COUNT), backends, own, other, deny[1])
    _env[family] = e   # (flow() reads it)

    # the history, run while gap has its slot 2: hash 1 selects it
    hist = S.concat([flow(family, "gap", HIST_SPORT[k], [1]) for k in ("i", "ii", "loop")] +
                    [flow(family, "a", p, [p]) for p in HIST_STABLE])
    hist.hash = np.array([1, 1, 1] + list(HIST_STABLE), np.uint32)
    o = O.Oracle(t)
    o.classify(hist, EGRESS, EP, want_ct=True, apply_ct=True)
    t.ct = S.ct_from_rows(o.ct_dump())
    if not v6:   # lb_loopback on the third flow's CT_SERVICE entry
        kw = key_words(hist, 2)
        hit = 0
        for r in t.ct:
            tp = bytes(r["tuple"])
            if r["family"] == 1 and tp[13] & 4 and \
                    int.from_bytes(tp[8:12], "little") == kw[2] and \
                    int.from_bytes(tp[0:4], "little") == kw[0]:
                r["entry"][36] |= 8
                hit += 1
        assert hit == 1
    gone = [i for i in range(len(full)) if int(full["slave"][i]) == 2 and
            int(full["dport"][i]) == p80 and
            addr_words(full["addr"][i], family) == addr_words(vip["gap"], family)]
    assert len(gone) == 1
    left = np.delete(full, gone[0])
    if v6:
        t.lb6 = left
    else:
        t.lb4 = left
    del e.backends["gap"][2]
    return e


# ------------------------------------------------------------- the streams
def _hdr(family, n):
    own = env(family).own
    sa = np.tile(own, (n, 1)) if family == 6 else np.full(n, own, np.uint32)
    return S.Headers(family, sa, sa.copy(), np.zeros(n, np.uint16), np.zeros(n, np.uint16),
                     np.full(n, TCP, np.uint8), np.zeros(n, np.uint8),
                     (100 + 7 * np.arange(n) % 1400).astype(np.uint16), np.zeros(n, np.uint32),
                     None, np.zeros(n, np.uint32))


def flow(family, svc, sport, hashes, dport=80, proto=TCP):
    """len(hashes) headers of one flow from the endpoint to a service; for
    ICMP sport / dport are the raw L4 halves"""
    n = len(hashes)
    h = _hdr(family, n)
    h.daddr[:] = env(family).vip[svc]
    h.proto[:] = proto
    raw = proto not in (TCP, UDP)
    h.sport[:] = sport if raw else S.htons(sport)
    h.dport[:] = dport if raw else S.htons(dport)
    h.hash[:] = np.asarray(hashes, np.uint64).astype(np.uint32)
    return h


def interleave(hs):
    """A B C A B C ... while each lasts"""
    off = np.concatenate([[0], np.cumsum([len(h) for h in hs])])
    order = [off[k] + i for i in range(max(len(h) for h in hs)) for k, h in enumerate(hs)
             if i < len(h)]
    return S.take(S.concat(hs), np.array(order))


@dataclasses.dataclass
class Case:
    family: int
    t: S.Tables
    batches: list          # S.Headers, classified and applied one after another
    plans: list = None     # Plan per batch

    @property
    def h(self):
        assert len(self.batches) == 1
        return self.batches[0]

    @property
    def plan(self):
        assert len(self.plans) == 1
        return self.plans[0]

    @property
    def svc_ordered(self):
        return [p.svc_ordered for p in self.plans]


def case(family, batches):
    e = env(family)
    p = Pass(e.t, family)
    return Case(family, e.t, list(batches), [p.batch(h) for h in batches])


def chunked(c, chunks=3):
    """the case's one batch cut as test_gpu_ctorder.run_both cuts it"""
    h = c.h
    step = (len(h) + chunks - 1) // chunks
    return case(c.family, [h.slice(a, a + step) for a in range(0, len(h), step)])


def one_flow(family, n, sport=1000, hashed=True):
    """n headers of one new flow to a, each with its own skb->hash (7, 8,
    ...: three different selections among the first three).  n - 1 words.
    hashed=False: no hash array, every header the engine's flow hash"""
    h = flow(family, "a", sport, 7 + np.arange(n))
    if not hashed:
        h.hash = None
    return case(family, [h])


def distinct(family, n):
    """n new flows to a, one header each: the list holds every header
    (m == n), no word"""
    h = S.concat([flow(family, "a", 2000 + i, [11 * i + 3]) for i in range(n)])
    return case(family, [h])


def straddle(family, which):
    """~300 listed headers whose runs sit at chosen positions of the sorted
    list.  'across': one run at 250..262, over the first block's edge (its
    thread is the first block's, its entries mostly the second's).  'abut':
    a run ending at 255 and the next starting at 256.  (One list cannot hold
    the three at the same edge.)  Every other position is a single-header
    key; the headers are shuffled in the batch."""
    e = env(family)
    want = {"across": {250: 13}, "abut": {249: 7, 256: 6}}[which]
    total = 300
    cand = []
    for j in range(total):
        f = flow(family, "abc"[j % 3], 3000 + j, [0], dport=80 + j % 7)
        cand.append((khash(key_words(f, 0)), j, f))
    cand.sort(key=lambda c: c[0])
    assert len({c[0] for c in cand}) == len(cand)
    parts, pos = [], 0
    for fp, j, f in cand:
        k = want.get(pos, 1)
        parts.append(S.take(f, np.zeros(k, np.int64)))
        pos += k
        if pos >= total:
            break
    h = S.concat(parts)
    h.hash = (5 + 7 * np.arange(len(h))).astype(np.uint32)
    rng = np.random.default_rng(31 + family)
    h = S.take(h, rng.permutation(len(h)))
    h.length = (100 + 7 * np.arange(len(h)) % 1400).astype(np.uint16)
    return case(family, [h])


def collide_keys(family, k):
    """k keys of equal 32-bit fingerprint to the L3 services a, b(, c): the
    same source and w, so the L4 word of each makes up for its destination's
    part of the hash -> [(service, sport, dport)] host order"""
    e = env(family)
    rng = np.random.default_rng(41 + family)
    svcs = ["a", "b", "c"][:k]
    s = addr_words(e.own, family)

    def part(svc):   # the hash just before z goes in
        d = addr_words(e.vip[svc], family)
        if family == 4:
            return fmix32(fmix32(d ^ GOLD) ^ s)
        return fmix32(_fold6(d, s) ^ GOLD)

    while True:
        za = int(rng.integers(0, 1 << 32))
        zs = [za ^ part("a") ^ part(v) for v in svcs]
        if all(z & 0xFFFF and z >> 16 for z in zs):
            break
    # z = sport | dport << 16, both raw (network order)
    return [(v, int(S.ntohs(z & 0xFFFF)), int(S.ntohs(z >> 16))) for v, z in zip(svcs, zs)]


def collide(family, k, n_each=6):
    """headers of k fingerprint-equal keys interleaved A B (C) A B (C) ...,
    each with its own hash; the first headers select slaves 2, 5(, 4): 5 and
    4 are no slots of a, so a replay that took the run for one key would
    hand on a slave the other service does not have"""
    first = [1, 4, 3]   # % 3 + 1 = 2, % 5 + 1 = 5, % 4 + 1 = 4
    hs = [flow(family, v, sp, [first[j]] + [100 + 7 * j + 13 * i for i in range(1, n_each)],
               dport=dp) for j, (v, sp, dp) in enumerate(collide_keys(family, k))]
    return case(family, [interleave(hs)])


def merged(c):
    """collide's batch with every header renamed to the first one's key"""
    h = copy.deepcopy(c.h)
    h.daddr[:] = h.daddr[0]
    h.sport[:] = h.sport[0]
    h.dport[:] = h.dport[0]
    return h


def same_home(family, n_each=5):
    """two keys to c with sport and dport exchanged: one home slot under any
    table mask (ct_home4/6 take the ports as an unordered pair), two
    fingerprints; interleaved, own hashes"""
    a = flow(family, "c", 5001, [0, 1, 2, 3, 5][:n_each], dport=6002)
    b = flow(family, "c", 6002, [2, 3, 0, 1, 6][:n_each], dport=5001)
    return case(family, [interleave([a, b])])


def reslave(family, which, n=8):
    """the entries stored with gap's slot 2, which is gone:
    i     the first header's hash re-selects the live slot 1 (4 % 4 + 1),
          every later header carries it
    ii    the first two re-select 2 again (hash % 4 == 1), the third slot 3
    iii   a new flow whose first header selects 2 (4 % 3 + 1) and re-selects
          the live slot 1 (4 % 4 + 1)
    iv    `none`: the first header selects the absent slot, the fall-back
          finds nothing; the entry exists, every header drops
    loop  (IPv4) i on the entry with lb_loopback: the words carry it"""
    tail = [9 + 5 * i for i in range(n)]
    if which == "i":
        h = flow(family, "gap", HIST_SPORT["i"], ([4] + tail)[:n])
    elif which == "ii":
        h = flow(family, "gap", HIST_SPORT["ii"], ([1, 5, 6] + tail)[:n])
    elif which == "iii":
        h = flow(family, "gap", 41002, ([4] + tail)[:n])
    elif which == "iv":
        h = flow(family, "none", 41004, ([1] + tail)[:n])
    elif which == "loop":
        h = flow(family, "gap", HIST_SPORT["loop"], ([4] + tail)[:n])
    else:
        raise KeyError(which)
    return case(family, [h])


def gates(family, n=6):
    """one new flow to a, interleaved with headers that share its addresses
    and never reach lb_local — protocol 47, another endpoint's source
    address, (IPv6) a neighbour solicitation — and with ICMP echoes of
    differing code and identifier to the same L3 service: one key of their
    own (the key words hold the type alone)"""
    e = env(family)
    icmp = S.IPPROTO_ICMPV6 if family == 6 else S.IPPROTO_ICMP
    echo = 128 if family == 6 else 8
    key = flow(family, "a", 42000, 3 + np.arange(n))
    gre = flow(family, "a", 42000, 50 + np.arange(n))
    gre.proto[:] = 47
    bad = flow(family, "a", 42000, 60 + np.arange(n))
    bad.saddr[:] = e.other
    hs = [key, gre, bad]
    if family == 6:
        hs.append(flow(family, "a", 135, 70 + np.arange(n), dport=0, proto=icmp))
    ech = flow(family, "a", echo, 80 + np.arange(n), dport=0, proto=icmp)
    ech.sport[:] = echo | (np.arange(n) % 3) << 8        # the code
    ech.dport[:] = 0x1100 + np.arange(n)                 # the identifier
    hs.append(ech)
    return case(family, [interleave(hs)])


def denied_first(family, n=6):
    """a new flow to deny: lb_local runs before the policy, so the first
    header creates the entry although the policy drops it, and the later
    ones take its slave"""
    return case(family, [flow(family, "deny", 43000, [1, 2, 4, 6, 8, 10, 12, 14][:n])])


def stale_and_growth(family):
    """six batches on one datapath: one_flow(513); 513 headers of the same,
    now stable, flow under other hashes (no word); 512 headers of the
    history's stable flows, whose stored slaves are not the first batch's,
    and one new flow of one header — a listed header arms the words'
    consumers (the launch reads them only when the list is not empty), so a
    word left over from the first batch at any of these indices would
    redirect its header; one_flow(2049) of another flow (the svo_*
    workspaces grow); then the second and third batch's shapes again"""
    def armed(sport):
        h = flow(family, "a", sport, list(2000 + 3 * np.arange(512)) + [5])
        h.sport[:512] = S.htons(np.array(HIST_STABLE)[np.arange(512) % len(HIST_STABLE)])
        return h

    b1 = flow(family, "a", 1000, 7 + np.arange(513))
    b2 = flow(family, "a", 1000, 1000 + 5 * np.arange(513))
    b3 = flow(family, "a", 1001, 9 + np.arange(2049))
    return case(family, [b1, b2, armed(1002), b3, copy.deepcopy(b2), armed(1003)])


STREAMS = {
    "straddle_across": lambda f: straddle(f, "across"),
    "straddle_abut": lambda f: straddle(f, "abut"),
    "collide2": lambda f: collide(f, 2),
    "collide3": lambda f: collide(f, 3),
    "same_home": same_home,
    "reslave_i": lambda f: reslave(f, "i"),
    "reslave_ii": lambda f: reslave(f, "ii"),
    "reslave_iii": lambda f: reslave(f, "iii"),
    "reslave_iv": lambda f: reslave(f, "iv"),
    "gates": gates,
    "denied_first": denied_first,
}
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513)


def stream(family, name):
    return STREAMS[name](family)


# ------------------------------------------------------- the NAT64 hop batch
def nat64_hops(m, seed=5):
    """nat64_lb_v6's tables; m IPv6 egress headers of one new flow to a
    v4-mapped VIP (a TCP service with every slot there and two or more
    backends), each with its own hash, spread among 3 m plain IPv6 headers:
    the hop batch's rows are not the batch's.  -> (tables, headers, hop
    header indices); the hop batch's pass hands on m - 1 words"""
    import golden_io as G
    g = G.Golden("nat64_lb_v6")
    t = g.tables
    lb = t.lb4
    keys = {(int(r["addr"]), int(r["dport"]), int(r["slave"])) for r in lb}
    pick = None
    for r in lb[lb["slave"] == 0]:
        c, a, dp = int(r["count"]), int(r["addr"]), int(r["dport"])
        if c >= 2 and dp and all((a, dp, j) in keys for j in range(1, c + 1)) and \
                (a, 0, 0) not in keys:
            pick = (a, dp, c)
            break
    assert pick is not None
    rng = np.random.default_rng(seed)
    ipc6 = t.ipcache[t.ipcache["family"] == 2]
    plain = S.gen_headers_v6(rng, 3 * m, ipc6, S.local_v6_addrs(t), local_frac=0.3,
                             mark_host=0, mark_proxy=0, src_fixed=S.LXC_IPV6, ext=0,
                             exthdr_drop=0)
    plain = S.Headers(6, plain.saddr, plain.daddr, plain.sport, plain.dport, plain.proto,
                      plain.flags, plain.length, plain.mark, S.tcp_flags_of(plain),
                      (900 + np.arange(3 * m)).astype(np.uint32))
    hop = S.take(plain, np.zeros(m, np.int64))
    hop.daddr = S.v4_mapped(np.full(m, pick[0], np.uint32))
    hop.sport = np.full(m, S.htons(61234), np.uint16)
    hop.dport = np.full(m, pick[1], np.uint16)
    hop.proto = np.full(m, TCP, np.uint8)
    hop.flags = np.zeros(m, np.uint8)
    hop.tcpflags = np.full(m, 0x02, np.uint8)
    hop.length = (120 + np.arange(m) % 1000).astype(np.uint16)
    hop.hash = (3 + np.arange(m)).astype(np.uint32)
    at = np.sort(rng.choice(4 * m, size=m, replace=False))
    order = np.full(4 * m, -1, np.int64)
    order[at] = 3 * m + np.arange(m)
    order[order < 0] = np.arange(3 * m)
    return t, S.take(S.concat([plain, hop]), order), at
