"""Streams for the proxy-map tests: tables whose policy rows carry proxy ports
for the streams' own identities, and header batches crafted so that the
oracle alone produces the cases (test_proxymap.py checks the counts on the
CPU; test_gpu_proxymap.py runs the engine against them).

Shapes, per family (config_c2 / config_c3 with three endpoints):
  ingress  24 peers x 3 source ports to the local endpoints: NEW and
           ESTABLISHED redirects, most keys written many times
  egress   the first endpoint to the same peers after a 512-header ingress
           batch from them seeded the CT: NEW, ESTABLISHED and REPLY redirects
           (the REPLY ones keep the tuple unreversed)
  dest     the first endpoint to the two other endpoints: its egress policy
           has no proxy port, theirs redirect identity SECLABEL — every
           redirect is the destination stage's after local delivery"""
import numpy as np

import oracle as O
from cilium_amd import synth as S

CLOCK = 1000
N = 4096
N_SEED = 512
# destination port -> (protocol, proxy port); 443 is allowed without a proxy,
# 22 has no row (denied)
PROXY = {80: (6, 10001), 8080: (6, 10002), 53: (17, 10003)}
PORTS = np.array([80, 8080, 53, 443, 22])
PORT_P = np.array([0.30, 0.25, 0.25, 0.10, 0.10])
PROTO_OF = {80: 6, 8080: 6, 53: 17, 443: 6, 22: 6}


def _rows(rows):
    out = np.zeros(len(rows), S.POLICY_DT)
    a = np.array(rows, np.int64).reshape(-1, 5)
    out["identity"], out["dport"], out["proto"] = a[:, 0], a[:, 1], a[:, 2]
    out["egress"], out["proxy_port"] = a[:, 3], a[:, 4]
    return out


def _l4_rows(identities, egress, proxied):
    """for each identity the three proxied ports (proxy port only for the
    identities in `proxied`) and 443 without a proxy"""
    rows = []
    for ident in identities:
        for port, (proto, pp) in PROXY.items():
            rows.append((int(ident), int(S.htons(port)), proto, egress,
                         int(S.htons(pp)) if ident in proxied else 0))
        rows.append((int(ident), int(S.htons(443)), 6, egress, 0))
    return rows


_cases = {}


def tables(v6):
    """-> (tables, peers (24 addresses), their identities, the endpoints'
    addresses, lxc ids)"""
    if v6 in _cases:
        return _cases[v6]
    if v6:
        t = S.config_c3(3, n_prefixes=2000, n_v4_prefixes=500, n_policy=64, n_endpoints=3,
                        n_prefilter=0)
    else:
        t = S.config_c2(2, n_prefixes=2000, n_policy=64, n_endpoints=3)
    t.ct = np.zeros(0, S.CT_DT)            # the global CT maps, empty
    fam = 2 if v6 else 1
    rng = np.random.default_rng(91 + fam)
    ipc = t.ipcache[t.ipcache["family"] == fam]
    pick = rng.choice(len(ipc), size=24, replace=False)
    peers = S._addr_in_prefix_v6(rng, ipc, pick) if v6 else S._addr_in_prefix_v4(rng, ipc, pick)
    lab, hit = O.Oracle(t).ipcache_lookup(6 if v6 else 4, peers)
    assert hit.all() and (lab >= 256).all()
    idents = sorted(set(int(x) for x in lab))
    proxied = set(idents[: (2 * len(idents) + 2) // 3])
    eps = t.endpoints[(t.endpoints["family"] == fam) & ((t.endpoints["flags"] & 1) == 0)]
    lxcs = [int(x) for x in eps["lxc_id"]]
    addrs = eps["addr"].copy() if v6 else eps["addr"][:, :4].copy().view("<u4").ravel()
    sec = S.EP_SECLABEL
    for k, lxc in enumerate(lxcs):
        rows = _l4_rows(idents, 0, proxied)                 # ingress, from the peers
        if k == 0:
            rows += _l4_rows(idents, 1, proxied)            # egress, to the peers
            # egress to the other endpoints: L3 allow for what their
            # addresses resolve to (no ipcache entry: WORLD or CLUSTER)
            rows += [(i, 0, 0, 1, 0) for i in (S.WORLD_ID, S.CLUSTER_ID)]
        else:
            rows += _l4_rows([sec], 0, {sec})               # from the first endpoint
        t.policy[lxc] = _rows(rows)
    _cases[v6] = (t, peers, lab.astype(np.uint32), addrs, lxcs)
    return _cases[v6]


def _headers(v6, saddr, daddr, sp, dp, rng):
    n = len(sp)
    proto = np.array([PROTO_OF[int(p)] for p in dp], np.uint8)
    length = rng.integers(60, 1501, size=n).astype(np.uint16)
    return S.Headers(6 if v6 else 4, saddr, daddr, S.htons(sp), S.htons(dp), proto,
                     np.zeros(n, np.uint8), length, np.zeros(n, np.uint32))


def ingress_stream(v6, n=N, seed=5, dst=None):
    t, peers, lab, addrs, lxcs = tables(v6)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(peers), size=n)
    sp = 40000 + 16 * k + rng.integers(0, 3, size=n)
    d = rng.integers(0, len(addrs), size=n) if dst is None else np.full(n, dst)
    dp = rng.choice(PORTS, size=n, p=PORT_P)
    return _headers(v6, peers[k], addrs[d], sp, dp, rng)


def egress_stream(v6, n=N, seed=6):
    """-> (seed batch (ingress, from the peers to the first endpoint), the
    egress batch of the first endpoint)"""
    t, peers, lab, addrs, lxcs = tables(v6)
    seedb = ingress_stream(v6, N_SEED, seed=seed + 100, dst=0)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(peers), size=n)
    sp = 50000 + 16 * k + rng.integers(0, 10, size=n)
    dp = rng.choice(PORTS, size=n, p=PORT_P)
    own = np.tile(addrs[0], (n, 1)) if v6 else np.full(n, addrs[0], np.uint32)
    h = _headers(v6, own, peers[k], sp, dp, rng)
    # 45 %: the reply to a seed packet (ports as raw be16, swapped)
    rep = np.flatnonzero(rng.random(n) < 0.45)
    j = rng.integers(0, N_SEED, size=len(rep))
    h.daddr[rep] = seedb.saddr[j]
    h.sport[rep] = seedb.dport[j]
    h.dport[rep] = seedb.sport[j]
    h.proto[rep] = seedb.proto[j]
    return seedb, h


def dest_stream(v6, n=N, seed=7):
    t, peers, lab, addrs, lxcs = tables(v6)
    rng = np.random.default_rng(seed)
    d = rng.integers(1, len(addrs), size=n)
    sp = 60000 + rng.integers(0, 40, size=n)
    dp = rng.choice(PORTS, size=n, p=np.array([0.35, 0.3, 0.3, 0.03, 0.02]))
    own = np.tile(addrs[0], (n, 1)) if v6 else np.full(n, addrs[0], np.uint32)
    return _headers(v6, own, addrs[d], sp, dp, rng)


def lb_tables():
    """the lb_egress_v4 fixture's tables and stream, plus L4 egress rows with
    a proxy port for the backends' identities: {the identity, the backend's
    port, protocol} of the service-translated headers the fixture's own
    policy forwards (two keys in three)"""
    import golden_io
    g = golden_io.Golden("lb_egress_v4")
    t, h = g.tables, g.headers
    if t.ct is None:
        t.ct = np.zeros(0, S.CT_DT)
    act, ver, ide, ct, pkt = oracle_run(t, [(h, g.mode, g.ep_lxc)])[0]
    tr = (pkt[:, 1] != h.daddr) & (ver == 0) & np.isin(h.proto, (6, 17))
    keys = sorted(set(zip(ide[tr].tolist(), (pkt[tr, 2] >> 16).tolist(), h.proto[tr].tolist())))
    keys = [k for j, k in enumerate(keys) if j % 3 != 2]
    pol = t.policy[g.ep_lxc]
    have = set(zip(pol["identity"].tolist(), pol["dport"].tolist(), pol["proto"].tolist(),
                   pol["egress"].tolist()))
    rows = [(i, p, pr, 1, int(S.htons(10004))) for i, p, pr in keys if (i, p, pr, 1) not in have]
    pol = pol.copy()
    for i, p, pr in keys:
        m = (pol["identity"] == i) & (pol["dport"] == p) & (pol["proto"] == pr) & \
            (pol["egress"] == 1)
        pol["proxy_port"][m] = S.htons(10004)
    t.policy[g.ep_lxc] = np.concatenate([pol, _rows(rows)]) if rows else pol
    return t, h, g.mode, g.ep_lxc


def oracle_run(t, batches, clock=CLOCK):
    """The oracle over the batches in order, one header at a time: batches =
    [(headers, mode, ep_lxc)] -> [(act, ver, ide, ct, pkt)] per batch."""
    o = O.Oracle(t)
    o.set_clock(clock)
    out = []
    for h, mode, ep in batches:
        out.append(o.classify(h, mode, ep, want_ct=True, apply_ct=True, want_pkt=True))
    return out


def shape(kind, v6):
    """-> (tables, [(headers, mode, ep_lxc)] — the last batch is the one
    under test, the ones before seed the CT)"""
    t, peers, lab, addrs, lxcs = tables(v6)
    if kind == "ingress":
        return t, [(ingress_stream(v6), 0, 0)]
    if kind == "egress":
        seedb, h = egress_stream(v6)
        return t, [(seedb, 0, 0), (h, 1, lxcs[0])]
    assert kind == "dest"
    return t, [(dest_stream(v6), 1, lxcs[0])]


_want = {}


def want(kind, v6):
    """the shape's oracle run and expected entries of its last batch, once:
    -> (tables, batches, oracle outputs per batch, (records, idx, stats))"""
    import proxy_entries as P
    key = (kind, v6)
    if key not in _want:
        t, batches = shape(kind, v6)
        outs = oracle_run(t, batches)
        h, mode, ep = batches[-1]
        act, ver, ide, ct, pkt = outs[-1]
        exp = P.expected_entries(h, mode, ver, ide, ct, pkt, seclabel=t.seclabel.get(ep, 0),
                                 now=CLOCK)
        _want[key] = (t, batches, outs, exp)
    return _want[key]
