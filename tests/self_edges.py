"""Cases of the self-traffic batch cuts (cfc_api.cpp self_cuts / classify,
selfseg.hip k_self_mark, selfcut.hpp self_cut_rule; DESIGN.md §4 "Traffic to
itself"), built with numpy alone: test_self_edges.py checks on the CPU that
each stream holds the dependency it claims, test_gpu_self_edges.py runs them
through the engine and asserts the exact segment count this file's
restatement of the rule gives.

The tables are the self_egress_v4 / self_egress_v6 fixtures' with three more
services whose backend is the sending endpoint: one at slave slot 1, one at
slave slot 2, one whose slot 2 lives only under the L3 (port 0) key.

ICMP types are the first byte of the header's L4 word (include/cfc.h), so a
header's sport holds the type itself, not htons(type).

Fresh CT state between blocks: every ICMP header of an endpoint to itself
shares one CT key, so the pair and triple blocks need it.  Loading the
fixture's tables takes ~30 ms per oracle, more than a minute over the two
views of both families' ~1400 blocks (the second way of the two: a fresh
Datapath and Oracle per block would exceed 10 s); so instead both clocks move past every lifetime (STEP seconds, more than the
21600 s of an established TCP flow) and both sides collect expired entries
before each block (clock_of(k), the GC calls of test_gpu_ctgc.py)."""
import copy
import dataclasses

import numpy as np

import golden_io as G
from cilium_amd import synth as S

INGRESS, EGRESS, FULL = 0, 1, 3
EP = S.EP_LXC_ID
BASE_CLOCK = 1 << 28     # past every lifetime the fixtures' entries carry
STEP = 30_000            # > CT_CONNECTION_LIFETIME_TCP (21600 s)
GRID = 8192 * 256        # k_self_mark's grid: one loop iteration covers this many
N_STRUCT = GRID + 257    # a second, ragged iteration

SYN, SYN_ACK, ACK, FIN_ACK, RST_ACK = 0x02, 0x12, 0x10, 0x11, 0x14
TCP, UDP = S.IPPROTO_TCP, S.IPPROTO_UDP


def clock_of(k):
    """the clock block k runs at"""
    return BASE_CLOCK + STEP * (k + 1)


# ---------------------------------------------------------------- the rule
def cut_rule(rows, n_own, v6):
    """selfcut.hpp self_cut_rule restated: rows (x header index, y L4 word,
    z meta, w address matched) in header order -> the header indices later
    segments start at.  Pinned to the C++ by `selftest kat selfcut`."""
    icmp = 58 if v6 else 1
    l4 = set()
    any_, svc, icmp_plain = False, False, False
    cuts = []
    for x, y, z, w in rows:
        proto, typ = z & 0xFF, y & 0xFF
        lo = w >= n_own
        is_icmp = proto == icmp
        err = is_icmp and ((1 <= typ <= 4) if v6 else typ in (3, 11, 12))
        a, b = y & 0xFFFF, (y >> 16) & 0xFFFF
        key = (proto, min(a, b), max(a, b))
        l4p = proto in (6, 17)
        dep = False
        if any_:
            if lo or svc or err:
                dep = True
            elif is_icmp:
                dep = icmp_plain
            elif l4p:
                dep = key in l4
        if dep:
            cuts.append(int(x))
            l4.clear()
            svc = icmp_plain = False
        any_ = True
        svc = svc or lo
        icmp_plain = icmp_plain or (is_icmp and not err)
        if l4p:
            l4.add(key)
    return cuts


def address_set(t, ep, family):
    """the addresses self_cuts lists headers by -> (own, loopback) lists of
    bytes: the endpoint's cilium_lxc addresses of the family (none: nothing
    is listed); the VIPs of services with one of them in a slave slot, and
    IPV4_LOOPBACK when a cilium_lb4_services map exists"""
    fam = 1 if family == 4 else 2
    al = 4 if family == 4 else 16
    e = t.endpoints
    own = []
    for r in e[(e["family"] == fam) & (e["lxc_id"] == ep) & ((e["flags"] & 1) == 0)]:
        a = bytes(r["addr"][:al])
        if a not in own:
            own.append(a)
    lo = []
    if not own:
        return own, lo
    lb = getattr(t, "lb4" if family == 4 else "lb6", None)
    if lb is not None:
        for r in lb:
            if int(r["slave"]) == 0:
                continue
            tgt = (int(r["target"]).to_bytes(4, "little") if family == 4
                   else bytes(np.asarray(r["target"], np.uint8)))
            vip = (int(r["addr"]).to_bytes(4, "little") if family == 4
                   else bytes(np.asarray(r["addr"], np.uint8)))
            if tgt in own and vip not in own and vip not in lo:
                lo.append(vip)
        if family == 4:
            b = int(S.IPV4_LOOPBACK).to_bytes(4, "little")
            if b not in own and b not in lo:
                lo.append(b)
    return own, lo


def _l4_meta(h):
    pt = h.sport.astype(np.uint32) | h.dport.astype(np.uint32) << 16
    mt = (h.proto.astype(np.uint32) | h.flags.astype(np.uint32) << 8 |
          h.length.astype(np.uint32) << 16)
    return pt, mt


def listed_rows(t, h, ep=EP):
    """the rows k_self_mark lists for the batch h of endpoint ep, in header
    order, and the number of own addresses"""
    own, lo = address_set(t, ep, h.family)
    if not own:
        return [], 0
    idx = {a: k for k, a in enumerate(own + lo)}
    if h.family == 4:
        d = [int(a).to_bytes(4, "little") for a in np.asarray(h.daddr, np.uint32)]
    else:
        d = [bytes(a) for a in np.asarray(h.daddr, np.uint8)]
    pt, mt = _l4_meta(h)
    return [(i, int(pt[i]), int(mt[i]), idx[a]) for i, a in enumerate(d) if a in idx], len(own)


def expected_cuts(t, h, mode=EGRESS, ep=EP, want_ct=True):
    """the cuts cfc_classify makes in the batch h (self_cuts' early returns,
    then the rule over the listed rows)"""
    if mode != EGRESS or not want_ct or len(h) < 2:
        return []
    rows, n_own = listed_rows(t, h, ep)
    if len(rows) < 2:
        return []
    return cut_rule(rows, n_own, h.family == 6)


# -------------------------------------------------------------- the tables
@dataclasses.dataclass
class Env:
    family: int
    t: S.Tables
    addr: dict            # destination name -> address (u32 / 16 bytes)
    svc_port: dict        # service destination name -> host-order dport
    hash: int             # skb->hash under which every service picks the endpoint's slot
    plain: S.Headers      # non-self headers of the fixture's kind (filler)


_env = {}


def _other_local(t, family):
    loc = S.local_v4_addrs(t) if family == 4 else S.local_v6_addrs(t)
    own = S.LXC_IPV4 if family == 4 else np.asarray(S.LXC_IPV6, np.uint8)
    for a in loc:
        if family == 4 and int(a) != int(own):
            return np.uint32(a)
        if family == 6 and not (np.asarray(a) == own).all():
            return np.asarray(a, np.uint8)
    raise AssertionError("no second local endpoint")


def env(family):
    """the fixture's tables with the extra service shapes, built once"""
    if family in _env:
        return _env[family]
    g = G.Golden("self_egress_v4" if family == 4 else "self_egress_v6")
    t = g.tables
    v6 = family == 6
    own = np.asarray(S.LXC_IPV6, np.uint8) if v6 else np.uint32(S.LXC_IPV4)
    lb = t.lb6 if v6 else t.lb4
    rn = t.revnat6 if v6 else t.revnat4
    same = (lambda a, b: (np.asarray(a) == np.asarray(b)).all()) if v6 else \
        (lambda a, b: int(a) == int(b))
    k = [i for i in range(len(lb)) if int(lb["slave"][i]) and same(lb["target"][i], own)]
    assert len(k) == 1, "the fixture has one looped-back service"
    k = k[0]
    assert int(lb["slave"][k]) == 1
    fx_vip, fx_port = lb["addr"][k].copy(), int(lb["dport"][k])
    master = [i for i in range(len(lb)) if int(lb["slave"][i]) == 0 and
              same(lb["addr"][i], fx_vip) and int(lb["dport"][i]) == fx_port][0]
    fx_count = int(lb["count"][master])
    remote = [lb["target"][i].copy() for i in range(len(lb)) if int(lb["slave"][i]) and
              not same(lb["target"][i], own)][0]

    def vip(n):
        if v6:
            a = S.SVC6_NET.copy()
            a[14], a[15] = n >> 8, n & 255
            return a
        return np.uint32((S.SVC_NET + (n << 24)) & 0xFFFFFFFF)

    rows, rns = [], []
    p80 = int(S.htons(80))

    def row(addr, dport, slave, target=None, count=0, rev=0):
        r = np.zeros(1, lb.dtype)
        if v6:
            r["addr"][0] = addr
            if target is not None:
                r["target"][0] = target
        else:
            r["addr"] = addr
            r["target"] = 0 if target is None else target
        r["dport"], r["slave"], r["count"], r["rev_nat"] = dport, slave, count, rev
        rows.append(r)

    def revnat(index, addr, port):
        r = np.zeros(1, rn.dtype)
        r["index"], r["port"] = index, port
        if v6:
            r["addr"][0] = addr
        else:
            r["addr"] = addr
        rns.append(r)

    # hash % count + 1 (lb.h lb4_select_slave): one skb->hash for the whole
    # stream that picks slot 1 of the fixture's service (a multiple of its
    # count) and slot 2 of the two added ones (count c, hash % c == 1)
    c = 2 if fx_count % 2 else 3
    hs = [x for x in range(fx_count, 64, fx_count) if x % c == 1]
    assert hs, "no skb->hash picks the endpoint's slot of every service"
    # the endpoint at slot 1 of one backend; at slot 2 of c; at slot 2 of c,
    # that slot under the L3 key only
    v1, v2, v3 = vip(201), vip(202), vip(203)
    row(v1, p80, 0, count=1, rev=201)
    row(v1, p80, 1, target=own, rev=201)
    for v, rev in ((v2, 202), (v3, 203)):
        row(v, p80, 0, count=c, rev=rev)
        for j in range(1, c + 1):
            if j != 2:
                row(v, p80, j, target=remote, rev=rev)
    row(v2, p80, 2, target=own, rev=202)
    row(v3, 0, 2, target=own, count=c, rev=203)
    for n, v in ((201, v1), (202, v2), (203, v3)):
        revnat(n, v, p80)
    assert not set(int(x) for x in rn["index"]) & {201, 202, 203}
    if v6:
        t.lb6 = np.concatenate([lb] + rows)
        t.revnat6 = np.concatenate([rn] + rns)
    else:
        t.lb4 = np.concatenate([lb] + rows)
        t.revnat4 = np.concatenate([rn] + rns)
    addr = {"own": own, "svc_lo": fx_vip, "svc_1": v1, "svc_2": v2, "svc_l3": v3,
            "local": _other_local(t, family)}
    if not v6:
        addr["loopback"] = np.uint32(S.IPV4_LOOPBACK)
    # the fixture's plain traffic: everything not to a listed address
    h0 = g.headers
    h0 = S.Headers(h0.family, h0.saddr, h0.daddr, h0.sport, h0.dport, h0.proto, h0.flags,
                   h0.length, h0.mark, S.tcp_flags_of(h0), None)
    o, l = address_set(t, EP, family)
    if v6:
        d = [bytes(a) for a in np.asarray(h0.daddr, np.uint8)]
    else:
        d = [int(a).to_bytes(4, "little") for a in np.asarray(h0.daddr, np.uint32)]
    plain = S.take(h0, np.flatnonzero([a not in o + l for a in d]))
    i = np.flatnonzero(plain.proto == TCP)[0]   # a remote destination
    addr["remote"] = np.asarray(plain.daddr[i]).copy()
    e = Env(family, t, addr, {"svc_lo": int(S.ntohs(fx_port)), "svc_1": 80, "svc_2": 80,
                              "svc_l3": 80}, hs[0], plain)
    _env[family] = e
    return e


def variant(family, what):
    """a copy of the tables for the address-set cases: 'no_services' (no
    service maps at all), 'no_address' (the endpoint's cilium_lxc entry of
    this family taken out)"""
    t = copy.copy(env(family).t)
    if what == "no_services":
        for f in ("lb4", "revnat4", "lb6", "revnat6"):
            if getattr(t, f, None) is not None:
                setattr(t, f, None)
    elif what == "no_address":
        e = t.endpoints
        fam = 1 if family == 4 else 2
        t.endpoints = e[~((e["family"] == fam) & (e["lxc_id"] == EP))]
    else:
        raise KeyError(what)
    return t


# --------------------------------------------------------------- the kinds
# (name, destination, protocol, sport, dport, TCP flags).  Ports: x the
# block's ephemeral port, y 80 (TCP; the endpoint's own ingress admits it) /
# 53 (UDP), x2 / y2 another pair, s one port on both sides, v the service's;
# an ICMP kind's "sport" is its type.
def kinds(family):
    v6 = family == 6
    icmp = S.IPPROTO_ICMPV6 if v6 else S.IPPROTO_ICMP
    echo, reply = (128, 129) if v6 else (8, 0)
    errs = (1, 2, 3, 4) if v6 else (3, 11, 12)
    other = (133, 135) if v6 else (13,)
    k = [("tcp_syn", "own", TCP, "x", "y", SYN),
         ("tcp_synack", "own", TCP, "y", "x", SYN_ACK),
         ("tcp_ack", "own", TCP, "x", "y", ACK),
         ("tcp_fin", "own", TCP, "x", "y", FIN_ACK),
         ("tcp_rst", "own", TCP, "y", "x", RST_ACK),
         ("tcp_other", "own", TCP, "x2", "y2", SYN),
         ("tcp_same", "own", TCP, "s", "s", SYN),
         ("udp_xy", "own", UDP, "x", "u", 0),
         ("udp_yx", "own", UDP, "u", "x", 0),
         ("udp_on_tcp", "own", UDP, "x", "y", 0),
         ("icmp_echo", "own", icmp, echo, 0, 0),
         ("icmp_reply", "own", icmp, reply, 0, 0)]
    k += [(f"icmp_err{e}", "own", icmp, e, 0, 0) for e in errs]
    k += [(f"icmp_other{e}", "own", icmp, e, 0, 0) for e in other]
    k += [("svc_lo", "svc_lo", TCP, "x", "v", SYN),
          ("svc_1", "svc_1", TCP, "x", "v", SYN),
          ("svc_2", "svc_2", TCP, "x", "v", SYN),
          ("svc_l3", "svc_l3", TCP, "x", "v", SYN)]
    if not v6:
        k += [("loopback", "loopback", TCP, "y", "x", SYN_ACK)]
    k += [("local_tcp", "local", TCP, "x", "y", SYN),
          ("remote_tcp", "remote", TCP, "x", "y", SYN),
          ("remote_udp", "remote", UDP, "x", "u", 0)]
    return k


NEVER_LISTED = ("local", "remote")


def kind(family, name):
    return next(k for k in kinds(family) if k[0] == name)


def headers(family, specs):
    """specs: (kind, block port base) per header -> S.Headers from the
    sending endpoint, the way test_gpu_self._self_stream builds them"""
    e = env(family)
    v6 = family == 6
    m = len(specs)
    own = e.addr["own"]
    sa = np.tile(own, (m, 1)) if v6 else np.full(m, own, np.uint32)
    da = sa.copy()
    sp, dp = np.zeros(m, np.uint16), np.zeros(m, np.uint16)
    proto, tf = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    for i, ((name, dst, pr, a, b, f), p) in enumerate(specs):
        da[i] = e.addr[dst]
        proto[i], tf[i] = pr, f
        port = {"x": p, "y": 80, "x2": p + 1, "y2": 8080, "u": 53, "s": p + 2,
                "v": e.svc_port.get(dst, 0)}
        if pr in (TCP, UDP):
            sp[i], dp[i] = S.htons(port[a]), S.htons(port[b])
        else:
            sp[i], dp[i] = a, b   # bytes [type, code]: the type is the low byte
    h = S.Headers(family, sa, da, sp, dp, proto, np.zeros(m, np.uint8),
                  (100 + 7 * np.arange(m) % 1400).astype(np.uint16), np.zeros(m, np.uint32), tf,
                  np.full(m, e.hash, np.uint32))
    h.flags[(proto == TCP) & ((tf & 0x05) != 0)] = S.HF_TCP_CLOSE
    return h


@dataclasses.dataclass
class Block:
    names: tuple
    h: S.Headers


def pair_blocks(family):
    """every ordered pair of kinds as a block of two headers, each block on
    ports no other block uses (x = 20000 + 4 k)"""
    ks = kinds(family)
    out = []
    for a in ks:
        for b in ks:
            p = 20000 + 4 * len(out)
            out.append(Block((a[0], b[0]), headers(family, [(a, p), (b, p)])))
    assert 20000 + 4 * len(out) < 29000   # (the fixture's history starts there)
    return out


def triple_blocks(family):
    """triples whose third header depends on the first: with a middle header
    that forces a cut (the rule starts the new segment's l4 / svc /
    icmp_plain from the cutting header alone: the first header's writes are
    folded by then), and with a never-listed middle header (the rule's state
    carries across it)"""
    firsts = ["tcp_syn", "udp_xy", "icmp_echo", "svc_1"]
    middles = ["tcp_synack", "icmp_err3", "svc_2", "icmp_reply", "remote_tcp", "local_tcp"]
    thirds = ["tcp_ack", "tcp_synack", "udp_yx", "icmp_reply", "tcp_fin"]
    out = []
    for a in firsts:
        for m in middles:
            for c in thirds:
                p = 50000 + 4 * len(out)
                out.append(Block((a, m, c), headers(
                    family, [(kind(family, a), p), (kind(family, m), p),
                             (kind(family, c), p)])))
    return out


def concat_blocks(blocks):
    h = S.concat([b.h for b in blocks])
    h.hash = np.concatenate([b.h.hash for b in blocks])
    return h


def filler(family, n, distinct=4096, seed=71):
    """n plain headers from the endpoint, none to a listed address, cycling
    over `distinct` flows of the fixture's kind (first packets create the
    entries, the rest hit them)"""
    e = env(family)
    rng = np.random.default_rng(seed)
    t = e.t
    if family == 4:
        h = S.gen_headers_v4(rng, 2 * distinct, t.ipcache[t.ipcache["family"] == 1],
                             S.local_v4_addrs(t), local_frac=0.3, mark_host=0, mark_proxy=0,
                             src_fixed=S.LXC_IPV4, frag=0)
        d = [int(a).to_bytes(4, "little") for a in np.asarray(h.daddr, np.uint32)]
    else:
        h = S.gen_headers_v6(rng, 2 * distinct, t.ipcache[t.ipcache["family"] == 2],
                             S.local_v6_addrs(t), local_frac=0.3, mark_host=0, mark_proxy=0,
                             src_fixed=S.LXC_IPV6, ext=0, exthdr_drop=0)
        d = [bytes(a) for a in np.asarray(h.daddr, np.uint8)]
    o, l = address_set(t, EP, family)
    keep = np.flatnonzero([a not in o + l for a in d])[:distinct]
    h = S.Headers(h.family, h.saddr, h.daddr, h.sport, h.dport, h.proto, h.flags, h.length,
                  h.mark, S.tcp_flags_of(h), None)
    h = S.take(h, keep[np.arange(n) % len(keep)])
    h.hash = np.full(n, e.hash, np.uint32)
    return h


def _put(h, at, src):
    for f in ("saddr", "daddr", "sport", "dport", "proto", "flags", "length", "mark",
              "tcpflags", "hash"):
        getattr(h, f)[at] = getattr(src, f)


def boundary_stream(family, n, boundaries, lone=(), run=None):
    """plain traffic with listed headers around each boundary b (the index
    of the first header past it): one TCP flow's SYN at b-1 and its SYN-ACK
    at b — the dependent pair straddles the boundary — and before them
    another flow's SYN at b-3 and SYN-ACK at b-2, so a header on each side
    of the boundary depends on an earlier one (cuts at b-2 and b).  Boundary
    1 has only the SYN at 0 and the SYN-ACK at 1.  lone: indices of
    single listed headers on ports of their own; at index n-1 another ACK of
    the last boundary's flow (a cut at the last header).  run: (start,
    length) of consecutive listed SYNs on distinct ports, no dependency
    among them.  -> (headers, the indices that hold a listed header)"""
    h = filler(family, n)
    for f in ("saddr", "daddr", "sport", "dport", "proto", "flags", "length", "mark",
              "tcpflags", "hash"):
        setattr(h, f, np.array(getattr(h, f)))
    K = lambda name: kind(family, name)   # noqa: E731
    at, specs = [], []
    for j, b in enumerate(boundaries):
        p = 60000 + 4 * j
        for i, name, q in ((b - 3, "tcp_syn", p + 400), (b - 2, "tcp_synack", p + 400),
                           (b - 1, "tcp_syn", p), (b, "tcp_synack", p)):
            if 0 <= i < n:
                at.append(i)
                specs.append((K(name), q))
    for j, i in enumerate(lone):
        at.append(i)
        if i == n - 1:
            specs.append((K("tcp_ack"), 60000 + 4 * (len(boundaries) - 1)))
        else:
            specs.append((K("tcp_other"), 61000 + 4 * j))
    if run:
        for j in range(run[1]):
            at.append(run[0] + j)
            specs.append((K("tcp_syn"), 62000 + j))
    assert len(set(at)) == len(at), "listed headers collide"
    _put(h, np.array(at), headers(family, specs))
    return h, sorted(at)


BOUNDARIES = (1, 64, 256, GRID)
RUN = (1000, 130)        # 24 lanes of one wave, a whole wave, 42 of the next


def structural_stream(family):
    """n = 8192 * 256 + 257: listed headers at 0, 1, 61-64, 253-256, GRID-3
    .. GRID and n-1 (cuts at 1, 62, 64, 254, 256, GRID-2, GRID, n-1), and a
    run of 130 across two wave boundaries"""
    return boundary_stream(family, N_STRUCT, BOUNDARIES, lone=(N_STRUCT - 1,), run=RUN)


def one_flow(family, n=300):
    """every header listed and dependent on the one before: one TCP flow's
    SYN, SYN-ACK, then ACKs both ways (n - 1 cuts: segments of length 1)"""
    names = ["tcp_syn", "tcp_synack"] + ["tcp_ack" if i % 2 == 0 else "tcp_synack"
                                          for i in range(n - 2)]
    h = headers(family, [(kind(family, x), 63000) for x in names])
    h.tcpflags[2:] = ACK
    return h


def edge_cuts(family, n=300):
    """cuts at indices 1 and n-1 only: a flow's SYN at 0, its SYN-ACK at 1,
    its ACK at n-1, plain traffic between"""
    h, _ = boundary_stream(family, n, (1,), lone=(n - 1,))
    return h


def independent(family, n=200):
    """listed headers only, pairwise independent: TCP SYNs and UDP on
    distinct ports, one ICMP echo; no error, no service"""
    specs = [(kind(family, "tcp_syn" if i % 3 else "udp_xy"), 64000 + i) for i in range(n)]
    specs[n // 2] = (kind(family, "icmp_echo"), 0)
    return headers(family, specs)


def self_addressed(family, n=600, seed=9):
    """a stream of the catalogue's own-address kinds, several packets per
    flow: what the ingress / FULL cases run (as the packets arriving at the
    endpoint), and the growth case's self part"""
    rng = np.random.default_rng(seed)
    ks = [k for k in kinds(family) if k[1] == "own"]
    specs = [(ks[int(rng.integers(len(ks)))], 65000 + int(rng.integers(n // 8)))
             for _ in range(n)]
    return headers(family, specs)


# ------------------------------------------------- the GPU tests' streams
@dataclasses.dataclass
class Case:
    t: S.Tables
    h: S.Headers
    mode: int = EGRESS
    ep: int = EP
    cut: bool = True      # the test claims cuts (False: one launch)


def _K(family, names, p0):
    """one header per name; `name@k` puts it on block port p0 + 4 k"""
    specs = []
    for nm in names:
        nm, _, k = nm.partition("@")
        specs.append((kind(family, nm), p0 + 4 * int(k or 0)))
    return headers(family, specs)


def cut_cases(family):
    """small batches that are cut: the concatenated pair and triple blocks,
    299 segments of one header, cuts at 1 and n-1 only"""
    t = env(family).t
    return {"pairs": Case(t, concat_blocks(pair_blocks(family))),
            "triples": Case(t, concat_blocks(triple_blocks(family))),
            "one_flow": Case(t, one_flow(family)),
            "edge_cuts": Case(t, edge_cuts(family))}


def address_cases(family):
    """one small stream per shape of the address set self_cuts builds"""
    e = env(family)
    c = {}
    # the service comes first, an independent own-address flow and its
    # answer follow: cut at 1 by the service alone, at 3 by the flow
    for name in ("svc_2", "svc_l3") + (("loopback",) if family == 4 else ()):
        c[name] = Case(e.t, _K(family, [name, "tcp_syn@1", "remote_tcp@2", "tcp_synack@1"],
                               52000))
    # no service map: the VIPs and IPV4_LOOPBACK are plain addresses, a self
    # TCP flow is still cut (at its answer only)
    names = ["tcp_syn", "svc_1@1", "tcp_synack"]
    if family == 4:
        names.insert(2, "loopback@2")
    c["no_services"] = Case(variant(family, "no_services"), _K(family, names, 52100))
    # the endpoint has no address of this family: nothing is listed
    c["no_address"] = Case(variant(family, "no_address"), one_flow(family, 20), cut=False)
    # another endpoint's batch to this endpoint's address: not its own
    other = e.t.endpoints[(e.t.endpoints["lxc_id"] != EP) & ((e.t.endpoints["flags"] & 1) == 0) &
                          (e.t.endpoints["family"] == (1 if family == 4 else 2))][0]
    h = one_flow(family, 20)
    if family == 4:
        h.saddr[:] = int.from_bytes(bytes(other["addr"][:4]), "little")
    else:
        h.saddr[:] = other["addr"]
    c["second_endpoint"] = Case(e.t, h, ep=int(other["lxc_id"]), cut=False)
    return c


def no_cut_cases(family):
    """streams no cut is due in: the self-addressed stream arriving at the
    endpoint (INGRESS) and in FULL mode, and an egress batch of pairwise
    independent listed headers"""
    t = env(family).t
    h = self_addressed(family)
    return {"ingress": Case(t, h, mode=INGRESS, ep=0, cut=False),
            "full": Case(t, h, mode=FULL, ep=0, cut=False),
            "independent": Case(t, independent(family), cut=False)}


def ragged_self(family, self_stream, total):
    """the fixture's own tables and test_gpu_self._self_stream cut to
    `total` headers (the ragged schedule's sum)"""
    g = G.Golden("self_egress_v4" if family == 4 else "self_egress_v6")
    h = self_stream(g, 15 + family, 100_000)
    assert len(h) >= total
    return Case(g.tables, h.slice(0, total))


def growth_case(family, n_new=6000, n_self=40):
    """a device CT table sized for the fixture's few hundred entries, maps
    with room; n_new plain new flows, then one self flow of n_self headers:
    the first segment (everything before the flow's answer) creates far more
    entries than 3/4 of the table holds"""
    t = copy.copy(env(family).t)
    t.ct_max_entries = 1 << 20
    h = S.concat([filler(family, n_new, distinct=n_new, seed=73), one_flow(family, n_self)])
    return Case(t, h)
