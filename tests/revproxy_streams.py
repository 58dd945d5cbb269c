"""Streams for the from-host tests (cfc_classify_from_host_*): tables, proxy
map entries and header batches, with their expected outputs taken from the
existing oracle by composition — revproxy_ref.translate() rewrites the batch,
the translated batch goes through the oracle in INGRESS mode with the hit
rows' mark as 0xA00 | enc(identity).  test_revproxy.py checks on the CPU what
each stream claims about itself; test_gpu_revproxy.py runs the engine.

  round_trip(v6)   the first endpoint's egress batch to the two others, whose
                   ingress policy redirects it (proxy_streams' `dest` shape);
                   then the proxy's packets back to that endpoint, mixed with
                   plain from-host traffic.  The translated replies are
                   CT_REPLY of the flows batch 1 created; untranslated they
                   are new flows from the host that the policy drops.
  identity_rows    one header per case of the source-identity rule
  small(v6)        one endpoint, a handful of identities: the tables behind
                   the skip-proxy, never-translated and structural tests"""
import dataclasses

import numpy as np

import lookup_edges as E
import oracle as O
import proxy_entries as P
import proxy_streams as PS
import revproxy_ref as R
from cilium_amd import synth as S

CLOCK = PS.CLOCK
PROXY_PORT = int(S.htons(10001))          # be16 raw, as a verdict carries it
HOST4 = S.ip4("10.15.0.1")
BIG = 0x01000005                          # an identity the mark cannot carry


def host_addr(v6, n=None):
    """the proxy's own address (the node's): outside every prefix of the
    streams' ipcaches"""
    a = np.frombuffer(bytes(S.ip6("fd77::1")), np.uint8) if v6 else np.uint32(HOST4)
    if n is None:
        return a
    return np.tile(a, (n, 1)) if v6 else np.full(n, a, np.uint32)


def labels_of(oracle, h):
    lab, hit = oracle.ipcache_lookup(h.family, h.saddr)
    return np.where(hit != 0, lab, 0).astype(np.uint32)


def concat(parts):
    f = parts[0].family
    cat = lambda name: np.concatenate([getattr(p, name) for p in parts])  # noqa: E731
    return S.Headers(f, cat("saddr"), cat("daddr"), cat("sport"), cat("dport"), cat("proto"),
                     cat("flags"), cat("length"), cat("mark"))


@dataclasses.dataclass
class Expect:
    """a from-host batch and everything the engine must give for it"""
    tables: S.Tables
    entries: dict                 # the family's proxy map {key: value}
    h: S.Headers                  # the batch as it arrives
    tr: R.Translation             # the restatement's translation
    th: S.Headers                 # translated, hit marks as the oracle reads them
    act: np.ndarray = None
    ver: np.ndarray = None
    ide: np.ndarray = None
    ct: np.ndarray = None
    words: np.ndarray = None
    extra: dict = dataclasses.field(default_factory=dict)


def precondition_unlabelled(oracle, tr):
    """every translated source lies outside every ipcache prefix, so the
    oracle cannot derive an identity of its own for a hit row"""
    if not tr.hit.any():
        return True
    fam = 4 if tr.saddr.ndim == 1 else 6
    lab, hit = oracle.ipcache_lookup(fam, tr.saddr[tr.hit])
    return not hit.any()


# ---------------------------------------------------------------- round trip
_rt = {}


def round_trip(v6, n_hits=700, n_plain=900, n_near=200, seed=31):
    if v6 in _rt:
        return _rt[v6]
    t, peers, lab, addrs, lxcs = PS.tables(v6)
    h1 = PS.dest_stream(v6, n=2048)
    ep = lxcs[0]
    o = O.Oracle(t)
    o.set_clock(CLOCK)
    act1, ver1, ide1, ct1, pkt1 = o.classify(h1, 1, ep, want_ct=True, apply_ct=True,
                                            want_pkt=True)
    rec, idx, st = P.expected_entries(h1, 1, ver1, ide1, ct1, pkt1,
                                      seclabel=t.seclabel.get(ep, 0), now=CLOCK)
    entries = P.map_rows(rec)
    rng = np.random.default_rng(seed)
    red = np.flatnonzero(ver1 > 0)
    j = rng.choice(red, size=n_hits)
    idents = np.array(sorted(set(int(x) for x in lab)), np.uint32)
    # the proxy's packets towards the client (the first endpoint): source the
    # node's address and the proxy port, destination the client's address and
    # port; marks as the proxy sets them, and a few without
    mk = np.array([(0xA00 if k % 3 else 0xB00) | R.enc(idents[k % len(idents)])
                   for k in range(n_hits)], np.uint32)
    mk[::17] = 0
    mk[5::29] = 0xC00
    hits = S.Headers(6 if v6 else 4, host_addr(v6, n_hits), h1.saddr[j].copy(),
                     ver1[j].astype(np.uint16), h1.sport[j].copy(), h1.proto[j].copy(),
                     np.zeros(n_hits, np.uint8),
                     rng.integers(60, 1501, size=n_hits).astype(np.uint16), mk)
    # plain from-host traffic from the peers, and the proxy's packets of
    # connections the map does not hold (another client port)
    plain = PS.ingress_stream(v6, n_plain, seed=seed + 1, dst=0)
    near = S.take(hits, rng.integers(0, n_hits, size=n_near))
    near.dport = S.htons(30000 + rng.integers(0, 64, size=n_near))
    h2 = S.take(concat([hits, plain, near]), rng.permutation(n_hits + n_plain + n_near))
    tr = R.translate(h2, entries, labels_of(o, h2))
    th = tr.headers(h2)
    x = Expect(t, entries, h2, tr, th)
    x.extra["h1"], x.extra["ep"] = h1, ep
    x.extra["ver1"], x.extra["ide1"], x.extra["ct1"] = ver1, ide1, ct1
    x.extra["unlabelled"] = precondition_unlabelled(o, tr)
    x.act, x.ver, x.ide, x.words, x.ct = o.run_sequential(th, 0, 0, want_ct=True)
    x.extra["events"] = o.events(th, 0, 0, x.ver, x.ide, x.words)
    x.extra["ct_dump"] = o.ct_dump()
    # the same batch without the translation (looked up only, and last: a
    # lookup counts into the entries it hits).  The hit rows' untranslated
    # tuples are in no CT map, before or after the fold
    x.extra["plain"] = o.classify(h2, 0, 0, want_ct=True)
    _rt[v6] = x
    return x


# ------------------------------------------------------- one endpoint, by hand
EP = E.EP0
REAL, ID_A, ID_P = 1000, 777, 888         # a labelled source; identities marks carry
CLIENT0 = 41000                           # the endpoint's client ports start here


def ep_addr(v6):
    return np.frombuffer(bytes(S.LXC_IPV6), np.uint8) if v6 else np.uint32(S.LXC_IPV4)


def _a4(s):
    return E.raw4(E.host4(s))


def _a6(s):
    return np.frombuffer(bytes(S.ip6(s)), np.uint8)


def src_addrs(v6):
    """original sources by ipcache label"""
    if v6:
        return dict(real=_a6("2001:db8:a::1"), host=_a6("2001:db8:b::1"),
                    cluster=_a6("2001:db8:c::1"), none=_a6("2001:db8:d::1"),
                    big=_a6("2001:db8:e::1"))
    return dict(real=_a4("20.1.0.1"), host=_a4("20.2.0.1"), cluster=_a4("20.3.0.1"),
                none=_a4("20.4.0.1"), big=_a4("20.5.0.1"))


def orig_daddr(v6, k, labelled=False):
    """the k-th original destination (what a hit's source becomes): outside
    every prefix, or (labelled) inside one with the label 2000 + k"""
    if v6:
        return _a6(f"2001:db8:{'f1' if labelled else 'f0'}:{k + 1:x}::9")
    return _a4(f"{'30' if labelled else '31'}.0.{k + 1}.9")


def small(v6, labelled_dst=0, policy=None, big_allowed=True):
    """one endpoint EP; sources labelled REAL / HOST_ID / CLUSTER_ID / BIG;
    labelled_dst: that many orig_daddr(k, True) carry the label 2000 + k.
    policy (ingress rows of EP): default L3 allow for REAL, ID_A, HOST_ID,
    2000.. and (big_allowed) BIG; everything else is denied"""
    s = src_addrs(v6)
    pfx = [("real", REAL), ("host", S.HOST_ID), ("cluster", S.CLUSTER_ID), ("big", BIG)]
    if v6:
        rows = [(int.from_bytes(bytes(s[k]), "big"), 128, l) for k, l in pfx]
        rows += [(int.from_bytes(bytes(orig_daddr(True, k, True)), "big"), 128, 2000 + k)
                 for k in range(labelled_dst)]
        ipc = E.ipc6(rows)
        eps = S.endpoint_v6(S.LXC_IPV6, 100, EP)
    else:
        rows = [(int(E.raw4(s[k])), 32, l) for k, l in pfx]
        rows += [(int(E.raw4(orig_daddr(False, k, True))), 32, 2000 + k)
                 for k in range(labelled_dst)]
        ipc = E.ipc4(rows)
        eps = E.endpoints4([S.LXC_IPV4])
    if policy is None:
        policy = [(i, 0, 0, 0, 0) for i in
                  [REAL, ID_A, S.HOST_ID] + [2000 + k for k in range(labelled_dst)] +
                  ([BIG] if big_allowed else [])]
    t = S.Tables(ipc, eps, {EP: E.pol_rows(policy)}, np.zeros(0, S.PREFILTER_DT),
                 {EP: S.EP_SECLABEL})
    t.ct = np.zeros(0, S.CT_DT)
    return t


def proxy_pkt(v6, src, client_port, mark=0, proto=6, flags=0, sport=None, daddr=None):
    """one packet of the proxy towards EP's client port: (source address as
    it arrives, the client port host order, mark)"""
    n = 1
    sa = np.asarray(src).reshape((1, 16) if v6 else (1,))
    da = np.asarray(ep_addr(v6) if daddr is None else daddr).reshape((1, 16) if v6 else (1,))
    sp = np.uint16(PROXY_PORT if sport is None else sport)
    return S.Headers(6 if v6 else 4, sa.copy(), da.copy(), np.full(n, sp, np.uint16),
                     S.htons(np.full(n, client_port)), np.full(n, proto, np.uint8),
                     np.full(n, flags, np.uint8), np.full(n, 100, np.uint16),
                     np.full(n, mark, np.uint32))


def entry_for(v6, h, i, odaddr, odport=80, identity=0, lifetime=CLOCK + 720, nexthdr=None):
    """the map entry header i of h hits: key from the packet, value given
    (odport host order)"""
    word = int(h.sport[i]) | int(h.dport[i]) << 16
    k = R.key_of(h.family, h.daddr[i], word, h.proto[i] if nexthdr is None else nexthdr)
    al = 16 if v6 else 4
    od = bytes(np.asarray(odaddr, np.uint8)) if v6 else \
        bytes(np.asarray(odaddr, np.uint32).reshape(1).view(np.uint8))
    v = od + int(S.htons(odport)).to_bytes(2, "little") + b"\0\0" + \
        int(identity).to_bytes(4, "little") + int(lifetime).to_bytes(4, "little")
    assert len(od) == al
    return k, v


def expect(t, entries, h, oracle_tables=None, seq=False):
    """the composition for a hand-made batch: CT maps empty, looked up only
    (seq: folded header by header)"""
    o = O.Oracle(t if oracle_tables is None else oracle_tables)
    o.set_clock(CLOCK)
    tr = R.translate(h, entries, labels_of(O.Oracle(t), h))
    th = tr.headers(h)
    x = Expect(t, entries, h, tr, th)
    if seq:
        x.act, x.ver, x.ide, x.words, x.ct = o.run_sequential(th, 0, 0, want_ct=True)
    else:
        x.act, x.ver, x.ide, x.ct, x.words = o.classify(th, 0, 0, want_ct=True,
                                                        want_notify=True)
    x.extra["unlabelled"] = precondition_unlabelled(o, tr)
    return x


# --------------------------------------------------------------- final identity
def identity_rows(v6):
    """-> (tables, tables without the orig_daddr prefixes, entries, headers,
    [(case name, final identity)]): every header hits, its orig_daddr is
    labelled 2000 + k in `tables`"""
    s = src_addrs(v6)
    host_over = S.HOST_ID if v6 else S.WORLD_ID     # the family difference
    cases = [
        ("mark0-real", s["real"], 0, REAL),
        ("mark0-host", s["host"], 0, host_over),
        ("mark0-cluster", s["cluster"], 0, S.WORLD_ID),
        ("mark0-none", s["none"], 0, S.WORLD_ID),
        ("host-none", s["none"], 0xC00, S.HOST_ID),
        ("host-real", s["real"], 0xC00, REAL),
        ("ingress-real-id", s["real"], 0xA00 | R.enc(ID_A), ID_A),
        ("egress-real-id", s["real"], 0xB00 | R.enc(ID_A), ID_A),
        ("ingress-world-real", s["real"], 0xA00 | R.enc(2), REAL),
        ("ingress-world-none", s["none"], 0xA00 | R.enc(2), S.WORLD_ID),
        ("ingress-zero-real", s["real"], 0xA00 | R.enc(0), REAL),
        ("ingress-zero-none", s["none"], 0xA00 | R.enc(0), 0),
        ("ingress-host-host", s["host"], 0xA00 | R.enc(1), S.HOST_ID),
    ]
    parts, entries = [], {}
    for k, (name, src, mark, want) in enumerate(cases):
        p = proxy_pkt(v6, src, CLIENT0 + k, mark)
        key, val = entry_for(v6, p, 0, orig_daddr(v6, k, True))
        entries[key] = val
        parts.append(p)
    t = small(v6, labelled_dst=len(cases))
    t2 = small(v6, labelled_dst=0)
    t2.policy = t.policy
    return t, t2, entries, concat(parts), [(c[0], c[3]) for c in cases]


def big_identity(v6, allowed):
    """a source whose ipcache label does not fit a mark's 24 bits: -> (tables,
    entries, header, a stand-in header for the oracle — the same packet from
    the REAL source, whose identity has the same policy rows when `allowed`
    and ID_P (no rows) otherwise)"""
    s = src_addrs(v6)
    t = small(v6, big_allowed=allowed)
    p = proxy_pkt(v6, s["big"], CLIENT0, 0)
    key, val = entry_for(v6, p, 0, orig_daddr(v6, 0))
    stand = proxy_pkt(v6, s["real"] if allowed else s["none"], CLIENT0,
                      0 if allowed else 0xB00 | R.enc(ID_P))
    return t, {key: val}, p, stand
