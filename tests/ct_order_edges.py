"""Streams of the conntrack packet-order edge tests (test_gpu_ct_order_edges.py),
built with numpy, synth and the oracle alone: test_ct_order_edges.py checks
on the CPU that each holds what it is about, the GPU file runs them through
the engine.

The random dependency streams (synth.headers_c5_seq) give each flow one
verdict, so a key is created, hit and closed and nothing else.  Here one CT
key gets two verdicts: A is a header the policy allows, D a header with the
same CT key the policy denies (DROP_POLICY: a delete when the entry exists) —
the IPv4 fragment of a flow only an L4 rule admits, or the same header with a
proxy-egress mark carrying an identity the endpoint denies.  E is a key that
exists when the batch starts, N one that does not.  A chain is a sequence of
A / D stages on one key; a batch holds the same chain on many keys, members
of different keys interleaved, plain hits of other live flows between them.

Left out: the PSTAGE = 2048 overflow of the collect's LDS participant stage
(ctorder.hip part_put).  A block of the grid-stride collect meets more than
2048 participants only in batches beyond two million participants, which is
no few-second test."""
import copy
import dataclasses
import functools

import numpy as np

import ct_edge_streams as E
import golden_io as G
import oracle as O
from cilium_amd import synth as S

CLOCK = E.CLOCK
DROP_POLICY = -133
NEW, EST, CREATE = 4, 5, 8       # CT byte, low nibble (cfc.h CFC_CT_DONE = 4)
SPORT0 = 1024                    # new keys: the live flow's source port replaced
TUPLE_F_RELATED = 2


def proxy_mark(ident):
    """skb->mark of a packet from the egress proxy carrying `ident`
    (MARK_MAGIC_PROXY_EGRESS, common.h get_identity_via_proxy)"""
    ident = np.asarray(ident, np.uint32)
    return (np.uint32(0xB00) | ((ident >> 16) & 0xFF) | ((ident & 0xFFFF) << 16)).astype(np.uint32)


def clone(h):
    return S.take(h, np.arange(len(h)))


def flow_key(h):
    """one row of bytes per header: equal rows, equal 5-tuple"""
    n = len(h)
    a = np.ascontiguousarray(h.saddr).view(np.uint8).reshape(n, -1)
    b = np.ascontiguousarray(h.daddr).view(np.uint8).reshape(n, -1)
    p = np.stack([h.sport & 0xFF, h.sport >> 8, h.dport & 0xFF, h.dport >> 8, h.proto], 1)
    return np.concatenate([a, b, p.astype(np.uint8)], 1)


def addr_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def first_of_key(h):
    """mask: the first header of every distinct 5-tuple"""
    _, i = np.unique(flow_key(h), axis=0, return_index=True)
    m = np.zeros(len(h), bool)
    m[i] = True
    return m


def look(t, h, mode, ep=0):
    """(verdict, identity, CT byte) of every header against the tables as
    they stand (no header sees another's writes)"""
    o = O.Oracle(t)
    o.set_clock(CLOCK)
    _, ver, ide, ct = o.classify(h, mode, ep, nthreads=8, want_ct=True)
    return ver, ide, ct


def sequential(t, h, mode, ep=0, want_pkt=False):
    """the oracle one header at a time -> the dict test_gpu_ctorder.check
    compares, the oracle itself under "oracle" """
    o = O.Oracle(t)
    o.set_clock(CLOCK)
    r = o.run_sequential(h, mode, ep, want_ct=True, want_pkt=want_pkt)
    act, ver, ide, words, ct = r[:5]
    rec, idx = o.events(h, mode, ep, ver, ide, words)
    w = dict(act=act, ver=ver, ide=ide, ct=ct, nt=words, rec=rec, idx=idx,
             rows=o.ct_dump(), metrics=o.metrics(), identity=o.identity_counters(),
             counters={lxc: o.policy_counters(lxc) for lxc in t.policy}, oracle=o)
    if want_pkt:
        w["pkt"] = r[5]
    return w


def order_changed(t, batches, mode, ep=0):
    """per batch, the stages whose CT nibble differs between the oracle's
    batch-start classify and its sequential run"""
    o = O.Oracle(t)
    o.set_clock(CLOCK)
    out = []
    for h in batches:
        t0 = copy.copy(t)
        t0.ct = S.ct_from_rows(o.ct_dump())
        c0 = look(t0, h, mode, ep)[2]
        c1 = o.run_sequential(h, mode, ep, want_ct=True)[4]
        x = c0 ^ c1
        out.append(int(((x & 0xF) != 0).sum() + ((x >> 4) != 0).sum()))
    return out


def denied_copies(t, a, mode, ep, want_ct, frag=True):
    """Per header of `a` a copy with the same CT key that the policy drops
    with CT byte `want_ct`: its fragment (IPv4, a flow an L4 rule admits), or
    the header under a proxy-egress mark with an identity the oracle drops
    -> (copies, found, by fragment)"""
    d = clone(a)
    found = np.zeros(len(a), bool)
    by_frag = np.zeros(len(a), bool)
    if a.family == 4 and frag:
        f = clone(a)
        f.flags = (f.flags | np.uint8(S.HF_FRAG)).astype(np.uint8)
        v, _, c = look(t, f, mode, ep)
        by_frag = (v == DROP_POLICY) & (c == want_ct)
        d.flags[by_frag] |= np.uint8(S.HF_FRAG)
        found |= by_frag
    return d, found, by_frag


def _mark_denied(t, a, d, found, ids, mode, ep, want_ct):
    for ident in ids:
        if found.all():
            break
        m = clone(a)
        m.mark = np.full(len(a), proxy_mark(ident), np.uint32)
        v, _, c = look(t, m, mode, ep)
        ok = ~found & (v == DROP_POLICY) & (c == want_ct)
        d.mark[ok] = proxy_mark(ident)
        found |= ok
    return d, found


@dataclasses.dataclass
class Pool:
    t: S.Tables
    family: int
    mode: int
    ep: int
    A: S.Headers          # one allowed header per E key (CT byte 05)
    D: S.Headers          # its denied copy (05, DROP_POLICY)
    by_frag: np.ndarray   # D is the fragment (else the marked header)
    base: S.Headers       # allowed ESTABLISHED live flows: new keys derive from them
    live: S.Headers       # filler: allowed hits of the other live flows
    denied_ids: np.ndarray


@functools.lru_cache(maxsize=None)
def pool(family, mode, n_flows=2_000, denied=True):
    """the E keys of the tables (SMALL by default): every live flow the
    policy allows and finds ESTABLISHED, for which a denied copy on the same
    key exists; denied=False: no denied copies sought (A and D stay empty)"""
    t, flows = E.tables(family, n_flows)
    h = clone(flows)
    ver, ide, ct = look(t, h, mode)
    ok_a = (ver == 0) & (ct == EST) & first_of_key(h)
    ids = np.unique(ide[ver == DROP_POLICY])[:32]
    found, by_frag, d = np.zeros(len(h), bool), np.zeros(len(h), bool), h
    if denied:
        d, found, by_frag = denied_copies(t, h, mode, 0, EST)
        d, found = _mark_denied(t, h, d, found, ids, mode, 0, EST)
    key = ok_a & found
    hit = (ver == 0) & np.isin(ct, [EST, E.REPLY]) & ~key
    sel = np.flatnonzero(key)
    return Pool(t, family, mode, 0, S.take(h, sel), S.take(d, sel), by_frag[sel],
                S.take(h, np.flatnonzero(ok_a)), S.take(h, np.flatnonzero(hit)), ids)


def with_sport(h, j):
    """the headers with source port SPORT0 + j (network order)"""
    n = clone(h)
    n.sport = S.htons((SPORT0 + np.broadcast_to(j, (len(h),))).astype(np.uint32)) \
        .astype(np.uint16)
    return n


def new_keys(p, n):
    """n keys that do not exist (an E key with its source port replaced:
    still allowed) -> (A, D): CT bytes 0c and 04 against the empty key"""
    ne = len(p.A)
    m = n + n // 8 + 16
    j = np.arange(m)
    a = with_sport(S.take(p.A, j % ne), j // ne)
    d = with_sport(S.take(p.D, j % ne), j // ne)
    va, _, ca = look(p.t, a, p.mode, p.ep)
    vd, _, cd = look(p.t, d, p.mode, p.ep)
    ok = np.flatnonzero((va == 0) & (ca == (NEW | CREATE)) & (vd == DROP_POLICY) & (cd == NEW) &
                        first_of_key(a))
    assert len(ok) >= n, (len(ok), n)
    return S.take(a, ok[:n]), S.take(d, ok[:n])


def new_flows(p, n):
    """n distinct allowed new flows (no denied copy needed)"""
    nb = len(p.base)
    m = n + n // 8 + 16
    j = np.arange(m)
    a = with_sport(S.take(p.base, j % nb), j // nb)
    va, _, ca = look(p.t, a, p.mode, p.ep)
    ok = np.flatnonzero((va == 0) & (ca == (NEW | CREATE)) & first_of_key(a))
    assert len(ok) >= n, (len(ok), n)
    return S.take(a, ok[:n])


def _sig(a, b, p, q, proto):
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return [bytes(x) for x in np.concatenate([lo, hi, np.minimum(p, q), np.maximum(p, q),
                                              proto], 1)]


def header_sigs(h):
    """per header a signature of its flow that does not depend on direction"""
    n = len(h)
    pt = lambda x: np.ascontiguousarray(x).view(np.uint8).reshape(n, 2)   # noqa: E731
    return _sig(addr_bytes(h.saddr), addr_bytes(h.daddr), pt(h.sport), pt(h.dport),
                np.asarray(h.proto, np.uint8).reshape(n, 1))


def row_sigs(rows, family):
    w = 4 if family == 4 else 16
    tu = rows[:, 4:42]
    return _sig(tu[:, :w], tu[:, w:2 * w], tu[:, 2 * w:2 * w + 2], tu[:, 2 * w + 2:2 * w + 4],
                tu[:, 2 * w + 4:2 * w + 5])


def explain_rows(st, got, want):
    """which chains the CT rows that differ belong to (printed: a failing
    comparison then names the chain)"""
    sig = {}
    for s, c, k in zip(header_sigs(st.h), st.chain, st.key):
        if c >= 0:
            sig[s] = (int(c), int(k))
    gs, ws = {bytes(r) for r in got}, {bytes(r) for r in want}
    for name, rows in (("only the engine has", [r for r in got if bytes(r) not in ws]),
                       ("only the oracle has", [r for r in want if bytes(r) not in gs])):
        if not rows:
            continue
        rows = np.array(rows)
        per = {}
        for s, r in zip(row_sigs(rows, st.h.family), rows):
            c = sig.get(s, (-1, -1))[0]
            per.setdefault(c, []).append(r)
        for c, rs in sorted(per.items()):
            what = "other keys" if c < 0 else f"chain {st.chains[c][0]} {st.chains[c][1]}"
            print(f"{name} {len(rs)} rows of {what}; first {bytes(rs[0][:44]).hex()} "
                  f"{bytes(rs[0][44:100]).hex()}")


# ------------------------------------------------------------------ chains
# (start, stages, the oracle's CT bytes in packet order)
LIVE = [("E", "ADADA", (0x05, 0x05, 0x0c, 0x05, 0x0c)),   # mixed slot, ends fresh
        ("E", "DDD", (0x05, 0x04, 0x04)),                 # delete only: k_ord_deltail
        ("E", "DAD", (0x05, 0x0c, 0x05)),                 # ends gone
        ("E", "AD", (0x05, 0x05)),                        # ends gone
        ("E", "DA", (0x05, 0x0c))]                        # ends fresh
FRESH = [("N", "AAA", (0x0c, 0x05, 0x05)),
         ("N", "ADA", (0x0c, 0x05, 0x0c)),                # deletes a key the batch created
         ("N", "DAD", (0x04, 0x0c, 0x05)),
         ("N", "DDA", (0x04, 0x04, 0x0c))]
CHAINS = LIVE + FRESH


def model(start, stages):
    """the state machine of ctorder.hip's header comment: a stage sees the
    previous stage's outcome on its key -> (CT bytes, the key exists after)"""
    there = start == "E"
    out = []
    for s in stages:
        if s == "A":
            out.append(EST if there else NEW | CREATE)
            there = True
        else:
            out.append(EST if there else NEW)
            there = False
    return tuple(out), there


@dataclasses.dataclass
class Stream:
    t: S.Tables
    h: S.Headers
    mode: int
    ep: int
    chains: list              # the catalogue: (start, stages, bytes)
    chain: np.ndarray         # per header: index into chains, -1 filler
    key: np.ndarray           # per header: the chain key's number, -1 filler
    member: np.ndarray        # per header: its place in the chain
    split: int = None         # cut streams: the first batch's size

    def want_ct(self):
        """the catalogue's CT byte per chain member (0xFF: filler)"""
        w = np.full(len(self.h), 0xFF, np.uint8)
        for c, (_, _, b) in enumerate(self.chains):
            m = self.chain == c
            w[m] = np.asarray(b, np.uint8)[self.member[m]]
        return w


def weave(t, mode, ep, chains, members, filler, n_filler, seed, cut=False):
    """members[c]: the headers of chain c, one batch of K keys per stage.
    Every key's members keep their order, at random places of the stream;
    cut: key k's members from place 1 + k % (L - 1) on go to a second batch
    (every cut position inside every chain, over the keys)"""
    rng = np.random.default_rng(seed)
    parts, pos, chain, key, member = [], [], [], [], []
    k0 = 0
    for c, ms in enumerate(members):
        nk, ln = len(ms[0]), len(ms)
        at = np.sort(rng.random((nk, ln)), axis=1)
        kid = k0 + np.arange(nk)
        k0 += nk
        if cut:
            first = 1 + kid % max(1, ln - 1)
            at = at + (np.arange(ln)[None, :] >= first[:, None])
        for j, m in enumerate(ms):
            assert len(m) == nk
            parts.append(m)
            pos.append(at[:, j])
            chain.append(np.full(nk, c))
            key.append(kid)
            member.append(np.full(nk, j))
    if n_filler:
        parts.append(S.take(filler, rng.integers(0, len(filler), size=n_filler)))
        pos.append(rng.random(n_filler) * (2 if cut else 1))
        for x in (chain, key, member):
            x.append(np.full(n_filler, -1))
    pos = np.concatenate(pos)
    order = np.argsort(pos, kind="stable")
    h = S.take(S.concat(parts), order)
    h.tcpflags = None
    return Stream(t, h, mode, ep, list(chains), np.concatenate(chain)[order],
                  np.concatenate(key)[order], np.concatenate(member)[order],
                  int((pos < 1).sum()) if cut else None)


def _ad_members(p, chains, per_e, per_n):
    """the A / D headers of each chain: E chains share out the pool's E
    keys, N chains take new keys"""
    ne = sum(1 for c in chains if c[0] == "E")
    nn = len(chains) - ne
    per_e = min(per_e, len(p.A) // max(1, ne))
    assert per_e >= 8, (len(p.A), ne)
    na, nd = new_keys(p, per_n * nn) if nn else (None, None)
    members, ie, i_n = [], 0, 0
    for start, stages, _ in chains:
        if start == "E":
            idx = np.arange(ie, ie + per_e)
            ie += per_e
            a, d = S.take(p.A, idx), S.take(p.D, idx)
        else:
            idx = np.arange(i_n, i_n + per_n)
            i_n += per_n
            a, d = S.take(na, idx), S.take(nd, idx)
        members.append([clone(a) if s == "A" else clone(d) for s in stages])
    return members


@functools.lru_cache(maxsize=None)
def chain_stream(family, mode, cut=False):
    """every LIVE and FRESH chain on many keys at once (a few hundred keys),
    3000 plain hits as filler"""
    p = pool(family, mode)
    members = _ad_members(p, CHAINS, 40, 40)
    return weave(p.t, mode, 0, CHAINS, members, p.live, 3000, 51 + family + mode, cut)


def split_by_address(st):
    """the stream as two batches with no address pair in common (a CT key
    and a create's related entry hold both addresses): even and odd keys'
    remote address words -> (Stream, Stream)"""
    a = st.h.saddr if st.h.family == 4 else st.h.saddr.view("<u4").reshape(-1, 4).sum(1)
    side = ((a.astype(np.uint64) * 0x9E3779B1 >> 13) & 1).astype(bool)
    out = []
    for s in (False, True):
        i = np.flatnonzero(side == s)
        out.append(Stream(st.t, S.take(st.h, i), st.mode, st.ep, st.chains, st.chain[i],
                          st.key[i], st.member[i]))
    return out


# ----------------------------------------------------------- related round
# U an allowed new UDP header on an address pair with no entry of any kind,
# V the same pair with another source port, D the denied U, T / P the pair's
# TCP header / ICMP echo request, X its ICMP error (IPv4 type 3; IPv6 types
# 1-4 over the keys): x where the policy drops the error by itself.  (With
# an echo request as the creating flow only the orders with an allowed error:
# the rule that admits the echo, an L3 rule, admits the pair's error as well,
# and no denied copy of the echo is built.)
RELATED = [("U X", (0x0c, 0x05)),
           ("X U X", (0x0c, 0x0c, 0x05)),        # the error creates its own entry
           ("x U x", (0x04, 0x0c, 0x05)),        # an error before the create, dropped
           ("U D X", (0x0c, 0x05, 0x05)),        # the delete leaves the related entry
           ("U V X", (0x0c, 0x0c, 0x05)),        # two creates share one related key
           ("U X X", (0x0c, 0x05, 0x05)),
           ("U x x", (0x0c, 0x05, 0x04)),        # the denied error deletes the related entry
           ("P X", (0x0c, 0x05)),                # an echo request creates
           ("X P X", (0x0c, 0x0c, 0x05)),        # the error first, then the echo's create
           ("P U X", (0x0c, 0x0c, 0x05)),        # the echo's and a UDP create share the key
           ("P X X", (0x0c, 0x05, 0x05)),
           ("T X", (0x0c, 0x0c))]                # a TCP map's related entry is not found


def icmp_proto(family):
    return S.IPPROTO_ICMP if family == 4 else S.IPPROTO_ICMPV6


def as_icmp(h, types):
    x = clone(h)
    x.proto[:] = icmp_proto(h.family)
    x.sport = np.broadcast_to(np.asarray(types, np.uint16), (len(h),)).copy()
    x.dport = np.zeros(len(h), np.uint16)
    return x


def row_addrs(rows, family):
    """the two address columns of CT dump rows"""
    w = 4 if family == 4 else 16
    return rows[:, 4:4 + w], rows[:, 4 + w:4 + 2 * w]


@dataclasses.dataclass
class RelPool:
    t: S.Tables
    family: int
    mode: int
    H: dict               # stage letter -> headers, one row per address pair
    x_allowed: np.ndarray  # the policy allows the pair's error by itself


@functools.lru_cache(maxsize=None)
def rel_pool(family, mode):
    t, _ = E.tables(family)
    rng = np.random.default_rng(40 + family)
    n = 12_000
    ipc = t.ipcache[t.ipcache["family"] == (1 if family == 4 else 2)]
    if family == 4:
        u = S.gen_headers_v4(rng, n, ipc, S.local_v4_addrs(t)[:1], in_prefix=1.0,
                             local_frac=1.0, frag=0, mark_host=0, mark_proxy=0, other_proto=0)
    else:
        u = S.gen_headers_v6(rng, n, ipc, S.local_v6_addrs(t)[:1], in_prefix=1.0,
                             local_frac=1.0, ext=0, exthdr_drop=0, mark_host=0, mark_proxy=0,
                             other_proto=0)
    u.proto[:] = S.IPPROTO_UDP
    u.flags[:] = 0
    u.sport = S.htons(rng.integers(32768, 65536, size=n).astype(np.uint32)).astype(np.uint16)
    u.dport = S.htons(rng.choice(S.PORT_SET, size=n).astype(np.uint32)).astype(np.uint16)
    # the second half from the (identity, port, UDP) rules of identities
    # without an L3 rule: the flow passes, its ICMP error by itself does not
    pol = t.policy[S.EP_LXC_ID]
    pol = pol[pol["egress"] == 0]
    l3 = pol["identity"][pol["dport"] == 0]
    rules = pol[(pol["identity"] != 0) & (pol["dport"] != 0) & (pol["proto"] == S.IPPROTO_UDP) &
                ~np.isin(pol["identity"], l3)]
    pref = np.flatnonzero(np.isin(ipc["label"], rules["identity"]))
    assert len(pref) and len(rules)
    half = np.arange(n // 2, n)
    pick = pref[rng.integers(0, len(pref), size=len(half))]
    if family == 4:
        u.saddr[half] = S._addr_in_prefix_v4(rng, ipc, pick)
    else:
        u.saddr[half] = S._addr_in_prefix_v6(rng, ipc, pick)
    by_id = {int(r["identity"]): r["dport"] for r in rules}
    u.dport[half] = np.array([by_id[int(x)] for x in ipc["label"][pick]], np.uint16)
    # one candidate per remote address, none that any CT entry holds
    rows = O.Oracle(t).ct_dump()
    held = set()
    for col in row_addrs(rows, family):
        held |= {bytes(r) for r in col}
    sa = addr_bytes(u.saddr)
    _, first = np.unique(sa, axis=0, return_index=True)
    keep = np.zeros(n, bool)
    keep[first] = True
    keep &= np.array([bytes(r) not in held for r in sa])
    u = S.take(u, np.flatnonzero(keep))
    k = np.arange(len(u))
    H = dict(U=u, V=with_sport(u, 7), T=clone(u), P=as_icmp(u, 8 if family == 4 else 128),
             X=as_icmp(u, 3 if family == 4 else 1 + k % 4))
    H["V"].sport = (u.sport ^ np.uint16(0x0100)).astype(np.uint16)
    H["T"].proto[:] = S.IPPROTO_TCP
    vu, _, cu = look(t, u, mode)
    d, found, _ = denied_copies(t, u, mode, 0, NEW)
    d, found = _mark_denied(t, u, d, found, pool(family, mode).denied_ids, mode, 0, NEW)
    H["D"] = d
    vx, _, cx = look(t, H["X"], mode)
    ok = found & (vu == 0) & (cu == (NEW | CREATE)) & ((cx & 7) == NEW)
    v, _, c = look(t, H["V"], mode)
    ok &= (v == 0) & (c == (NEW | CREATE))
    # the pairs whose error the policy allows by itself (an L3 rule: their
    # TCP header and echo request pass as well), and those it drops
    xa = (vx == 0) & (cx == (NEW | CREATE))
    for s in "TP":
        v, _, c = look(t, H[s], mode)
        xa &= (v == 0) & (c == (NEW | CREATE))
    ok &= xa | ((vx == DROP_POLICY) & (cx == NEW))
    sel = np.flatnonzero(ok)
    return RelPool(t, family, mode, {s: S.take(h, sel) for s, h in H.items()}, xa[sel])


@functools.lru_cache(maxsize=None)
def related_stream(family, mode, cut=False):
    """every RELATED chain on its own address pairs, interleaved, with plain
    hits of live flows between them"""
    r = rel_pool(family, mode)
    ya, na = np.flatnonzero(r.x_allowed), np.flatnonzero(~r.x_allowed)
    n_x = sum(1 for c, _ in RELATED if "x" in c)
    per_a = min(24, len(ya) // (len(RELATED) - n_x))
    per_d = min(24, len(na) // n_x)
    assert per_a >= 4 and per_d >= 4, (len(ya), len(na))
    members, ia, i_d = [], 0, 0
    for stages, _ in RELATED:
        if "x" in stages:
            idx = na[i_d:i_d + per_d]
            i_d += per_d
        else:
            idx = ya[ia:ia + per_a]
            ia += per_a
        members.append([S.take(r.H[s.upper()], idx) for s in stages.split()])
    chains = [("R", c.split(), b) for c, b in RELATED]
    return weave(r.t, mode, 0, chains, members, pool(family, mode).live, 1500,
                 61 + family + mode, cut)


# ------------------------------------------------------ structural placements
N_STRUCT = 66_003      # n % 16 == 3: the last thread's run of ORD_IT is short
# the first index of the later unit: ORD_IT = 16 headers per thread and step
# (ctorder.hip:172), 64 headers per work-bits word, 256 * ORD_IT = 4096 per
# block step of mark and collect (k_ord_mark: span), 64 * LISTW = 65 536
# headers per block of k_ord_list_w (ctorder.hip:611)
ORD_IT, WORD, BLOCK_STEP, LISTW = 16, 64, 256 * 16, 1024
BOUNDARIES = [ORD_IT, WORD, BLOCK_STEP, WORD * LISTW]
E_AT, N_AT = (-3, -1, 0, 2), (-2, 1, 3)      # E: A D A D, N: A D A around a boundary
STRUCT_CHAINS = [("E", "ADAD", (0x05, 0x05, 0x0c, 0x05)), ("N", "ADA", (0x0c, 0x05, 0x0c))]


def placed(t, mode, n, filler, seed, places):
    """n headers of filler, then places [(chain index, key number, member,
    index, 1-header batch)] written over it"""
    rng = np.random.default_rng(seed)
    h = S.take(filler, rng.integers(0, len(filler), size=n))
    h.tcpflags = None
    chain, key, member = (np.full(n, -1) for _ in range(3))
    for c, k, m, i, one in places:
        assert chain[i] == -1 and len(one) == 1
        for f in ("saddr", "daddr", "sport", "dport", "proto", "flags", "length", "mark"):
            getattr(h, f)[i] = getattr(one, f)[0]
        chain[i], key[i], member[i] = c, k, m
    return h, chain, key, member


@functools.lru_cache(maxsize=None)
def structural_stream(family=4, mode=3):
    """about 66 000 headers, almost all filler; one E chain and one N chain
    astride each boundary, and both ending at the final headers"""
    p = pool(family, mode)
    nb = len(BOUNDARIES) + 1
    na, nd = new_keys(p, nb)
    places = []
    for k, b in enumerate(BOUNDARIES + [None]):
        e_at = [b + x for x in E_AT] if b else [N_STRUCT - 7, N_STRUCT - 5, N_STRUCT - 3,
                                                N_STRUCT - 1]
        n_at = [b + x for x in N_AT] if b else [N_STRUCT - 6, N_STRUCT - 4, N_STRUCT - 2]
        for c, (at, a, d) in enumerate([(e_at, p.A, p.D), (n_at, na, nd)]):
            for m, (i, s) in enumerate(zip(at, STRUCT_CHAINS[c][1])):
                places.append((c, 2 * k + c, m, i, S.take(a if s == "A" else d, [k])))
    h, chain, key, member = placed(p.t, mode, N_STRUCT, S.take(p.live, np.arange(len(p.live))),
                                   71, places)
    return Stream(p.t, h, mode, 0, STRUCT_CHAINS, chain, key, member)


N_ALT, N_HITS, FOLD_LONG = 3000, 2000, 512     # ctapply.hip:1375 FOLD_LONG
LONG_CHAINS = [("E", "AD" * (N_ALT // 2), None), ("N", "A" * N_HITS, None)]


@functools.lru_cache(maxsize=None)
def long_stream(family=4, mode=3):
    """one live key with 3000 alternating A / D stages (the fold deletes and
    re-creates one slot 1500 times) and one new key with a create and 1999
    counted hits (no start slot, past FOLD_LONG), 3000 plain hits between"""
    p = pool(family, mode)
    na, _ = new_keys(p, 1)
    one = lambda h: S.take(h, [len(h) - 1])   # noqa: E731
    chains = [(s, st, model(s, st)[0]) for s, st, _ in LONG_CHAINS]
    members = [[one(p.A) if s == "A" else one(p.D) for s in LONG_CHAINS[0][1]],
               [clone(na) for _ in range(N_HITS)]]
    return weave(p.t, mode, 0, chains, members, p.live, 3000, 73)


# -------------------------------------------------------- host-side fallbacks
# the arithmetic of ord_resolve_t (ctorder.hip), restated once; SOURCE holds
# the lines restated, which test_ct_order_edges.py looks up in the file
SOURCE = [
    "uint32_t words = 1u << 16, fwords = 1u << 12;",
    "while (words < 4ull * hint + 4096 && words < (1u << 28))",
    "const uint64_t cap0 = std::max<uint64_t>(B.part.bytes / 4, 2ull * B.part_hint + 65536);",
    "uint32_t words = 1024;",
    "while (words < nc && words < (1u << 26))",
    "(untagged || (hc[ORD_NCREATE] > 4ull * (O.cb_mask + 1) && O.cb_mask + 1 < (1u << 26)))) {",
    "constexpr uint32_t SET_SHARED = 2u, SET_ERR = 1u, SET_PROBES = 64;",
    "constexpr int ORD_IT = 16;",
    "constexpr uint32_t LISTW = 1024;",
    "constexpr uint32_t PSTAGE = 2048;",
    "const uint64_t span = 256ull * ORD_IT, stride = (uint64_t)gridDim.x * span;",
]
SOURCE_APPLY = ["constexpr uint32_t FOLD_LONG = 512;"]
FIRST_CREATES = 8              # the small first batch of every fallback case
N_SETFULL, N_TWICE, N_REMARK, N_REMARK_DROPS = 70_000, 35_000, 5_000, 500
N_FLOWS_ROOMY = 150_000        # more than 262 144 slots (test_gpu_ct_acct_edges.py)


def set_words(hint):
    """words of each sparse key set, sized by the previous batch's creates"""
    words = 1 << 16
    while words < 4 * hint + 4096 and words < (1 << 28):
        words *= 2
    return words


def part_room(part_words, part_hint):
    """participants the sparse collect has room for before it runs again"""
    return max(part_words, 2 * part_hint + 65536)


def filter_words(creates_hint):
    """words of the dense passes' filter of creates"""
    words = 1024
    while words < creates_hint and words < (1 << 26):
        words *= 2
    return words


def dense_remark(creates, words):
    """the dense mark runs again on a filter of the batch's own size"""
    return creates > 4 * words and words < (1 << 26)


@dataclasses.dataclass
class Fallback:
    t: S.Tables
    mode: int
    batches: list          # Headers per batch
    case: int              # the index of the batch the case is about

    @property
    def h(self):
        return S.concat(self.batches)

    def bounds(self):
        return [0] + np.cumsum([len(b) for b in self.batches]).tolist()


@functools.lru_cache(maxsize=None)
def fallback(kind, mode=3):
    """setfull: 8 creates, 70 000 distinct new flows, an ordinary batch;
    twice: 8 creates, 35 000 new flows each twice; remark: (fresh context,
    CFC_DENSE_APPLY) 5000 creates, 500 of the keys with a dropped CT_NEW
    stage before and after the create"""
    rng = np.random.default_rng(81)
    # (the two sparse cases on a table with room for their creates: a batch
    # that grows the table is applied again, densely, whatever its keys)
    p = pool(4, mode) if kind == "remark" else pool(4, mode, N_FLOWS_ROOMY, False)
    if kind == "remark":
        na, nd = new_keys(p, N_REMARK_DROPS)
        rest = new_flows(p, N_REMARK + N_REMARK_DROPS)
        seen = {bytes(r) for r in flow_key(na)}
        rest = S.take(rest, np.flatnonzero([bytes(r) not in seen for r in flow_key(rest)]))
        rest = S.take(rest, np.arange(N_REMARK - N_REMARK_DROPS))
        chains = [("N", "DAD", model("N", "DAD")[0]), ("N", "A", (NEW | CREATE,))]
        st = weave(p.t, mode, 0, chains, [[clone(nd), clone(na), clone(nd)], [rest]], p.live,
                   2000, 83)
        return Fallback(p.t, mode, [st.h], 0)
    n = N_SETFULL if kind == "setfull" else N_TWICE
    f = new_flows(p, FIRST_CREATES + n + 500)
    first = S.concat([S.take(f, np.arange(FIRST_CREATES)),
                      S.take(p.live, rng.integers(0, len(p.live), size=56))])
    body = S.take(f, FIRST_CREATES + np.arange(n))
    if kind == "twice":
        pos = np.sort(rng.random((n, 2)), axis=1)
        body = S.take(S.concat([body, body]), np.argsort(pos.T.ravel(), kind="stable"))
    last = S.concat([S.take(f, FIRST_CREATES + n + np.arange(500)),
                     S.take(p.live, rng.integers(0, len(p.live), size=1500))])
    last = S.take(last, rng.permutation(len(last)))
    for b in (first, body, last):
        b.tcpflags = None
    return Fallback(p.t, mode, [first, body, last], 1)


# ------------------------------------------------- egress with local delivery
# Two CT stages per header (the sender's egress lookup, the local
# destination's ingress lookup): the CT byte's low nibble is stage 0, the
# high nibble stage 1.  A: the sender to the other local endpoint on the port
# only an L4 rule of that endpoint admits; D its fragment, which the sender's
# L3 rule lets out and the receiver's L4 rule cannot match (DROP_POLICY at
# stage 1: the stage-1 key is deleted, the stage-0 key only hit); Z a header
# the sender's own policy drops (stage 0 only)
EGRESS = [("N", "AAA", (0xcc, 0x55, 0x55)),        # creates in both stages, then hits in both
          ("E", "ADAD", (0x55, 0x55, 0xc5, 0x55)),  # stage-1 key mixed, stage-0 key only hit
          ("N", "DAD", (0x4c, 0xc5, 0x55)),
          ("Z", "ZZ", (0x04, 0x04))]                # dropped at stage 0: no stage 1
EGRESS_FIXTURE = "ct_seq_egress_v4"


@functools.lru_cache(maxsize=None)
def egress_stream(cut=False, per=40):
    g = G.Golden(EGRESS_FIXTURE)
    t = copy.copy(g.tables)
    h = copy.copy(g.headers)
    h.hash = None
    h = clone(h)
    h.flags = (h.flags & np.uint8(0xFF ^ S.HF_TCP_CLOSE)).astype(np.uint8)
    mode, ep = g.mode, g.ep_lxc
    other = [a for a in S.local_v4_addrs(t) if a != S.LXC_IPV4][0]
    ver, _, ct = look(t, h, mode, ep)
    local = (h.daddr == other) & (h.saddr == S.LXC_IPV4) & (h.flags == 0) & first_of_key(h)
    a0 = np.flatnonzero(local & (ver == 0) & (ct == 0xcc))
    assert len(a0), "no new flow the fixture's policy delivers locally"
    # 2 * per E and N keys: the template with other source ports
    tpl = S.take(h, np.full(4 * per, a0[0]))
    a = with_sport(tpl, 3000 + np.arange(4 * per))
    d = clone(a)
    d.flags = (d.flags | np.uint8(S.HF_FRAG)).astype(np.uint8)
    va, _, ca = look(t, a, mode, ep)
    vd, _, cd = look(t, d, mode, ep)
    ok = np.flatnonzero((va == 0) & (ca == 0xcc) & (vd == DROP_POLICY) & (cd == 0x4c))
    assert len(ok) >= 3 * per, len(ok)
    a, d = S.take(a, ok[:3 * per]), S.take(d, ok[:3 * per])
    z = np.flatnonzero(local & (ver == DROP_POLICY) & (ct == 0x04))[:per]
    assert len(z) >= 8
    # the E keys' entries: the oracle's own creates, as table state
    o = O.Oracle(t)
    o.set_clock(CLOCK)
    o.run_sequential(S.take(a, np.arange(per)), mode, ep)
    t.ct = S.ct_from_rows(o.ct_dump())
    fill = np.flatnonzero((ver == 0) & np.isin(ct & 0xF, [EST, E.REPLY]) &
                          np.isin(ct >> 4, [0, EST, E.REPLY]) & ~local)
    assert len(fill) >= 16, len(fill)
    idx = [np.arange(per, 2 * per), np.arange(per), np.arange(2 * per, 3 * per)]
    members = []
    for (start, stages, _), i in zip(EGRESS[:3], idx):
        members.append([S.take(a if s == "A" else d, i) for s in stages])
    members.append([S.take(h, z), S.take(h, z)])
    return weave(t, mode, ep, EGRESS, members, S.take(h, fill), 2000, 91, cut)


# --------------------------------- IPv6 reverse NAT of the packets (k_ord_pkt6)
LB6 = [("N", "AAA", (0x0c, 0x05, 0x05)),     # the later packets reverse-NATed by the
                                              # index the create stored
       ("E", "ADA", (0x05, 0x05, 0x0c))]     # the packet after the delete is not


@functools.lru_cache(maxsize=None)
def lb6_stream(mode=0, cut=False):
    """the IPv6 SMALL tables with services (synth.lb6_services: a reverse-NAT
    entry under the endpoint's own index, which ipv6_policy stores in the
    flows it creates) -> Stream; run with want_pkt"""
    p = pool(6, mode)
    t = copy.copy(p.t)
    t.lb6, t.revnat6, _, _, _ = S.lb6_services(np.random.default_rng(95), t, n_services=24)
    per = len(p.A)
    na, nd = new_keys(p, per)
    for x in (p.A, p.D, na, nd, p.live):   # the services leave these as they were
        v, _, c = look(t, x, mode)
        v0, _, c0 = look(p.t, x, mode)
        assert (v == v0).all() and (c == c0).all()
    members = [[clone(na), clone(na), clone(na)], [clone(p.A), clone(p.D), clone(p.A)]]
    return weave(t, mode, 0, LB6, members, p.live, 2000, 97, cut)
