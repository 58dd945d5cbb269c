"""Direct placement of the policy keys (csrc layout.h pol_slot_direct,
flatten.cpp pol_place_direct, kern_common.hpp policy_key_slot) restated in
Python on top of lookup_edges.py's linear model, and the tables and header
streams that put it at its edges: the smallest tables with a displaced slot
wrapping past the last one, two keys of one bucket with one home slot, a
bucket whose keys sit in two endpoints' tables of different sizes, absent L4
keys the filter passes whose direct slot holds another key, two keys with
equal pre (no displacement exists), a key with a nonzero displacement whose
proxy port is patched.  Keys are found by CPU searches over identities, as
lookup_edges.last_slot_policy_ids does.  test_pol_direct.py checks on the CPU
that every case holds what it claims; test_gpu_pol_direct.py runs them."""
import collections
import functools

import numpy as np

import lookup_edges as E
from cilium_amd import synth as S

U64 = np.uint64
POL_DISP_MAX = 255
EP0 = E.EP0
TCP, UDP = S.IPPROTO_TCP, S.IPPROTO_UDP
HI80 = int(S.htons(80)) | TCP << 16          # hi word of an ingress tcp/80 key


def pol_slot_direct(pre, d, mask):
    pre = E._a(pre)
    return (pre + E._a(d) * ((pre >> U64(16)) | U64(1))) & E._a(mask)


def bucket_of(base, pre, words):
    return E.pol_bloom_hash(E.pol_bloom_salt(base), pre) & U64(words - 1)


def direct_model(policy):
    """{lxc: POLICY_DT rows} -> the direct placement pol_place_direct makes of
    the linear tables: dict(words, disp {bucket: d}, max_d, slots {lxc: [(lo,
    hi, proxy) | None]}, where {lxc: {(lo, hi): slot}}, buckets {bucket:
    [(lxc, lo, hi)]}, linear (the policy_model), bloom), or None when some
    bucket finds no displacement.  Buckets largest first, then by word; a
    bucket's keys by table and key."""
    model, bloom = E.policy_model(policy)
    if bloom is None:
        return None
    words = len(bloom)
    ents = []
    for lxc in sorted(model):
        m = model[lxc]
        for e in m["slots"]:
            if e is None:
                continue
            pre = int(E.pol_key_pre(e[0], e[1]))
            ents.append((int(bucket_of(m["base"], pre, words)), m["base"], e[1] << 32 | e[0],
                         pre, m["mask"], lxc, e))
    count = collections.Counter(x[0] for x in ents)
    ents.sort(key=lambda x: (-count[x[0]], x[0], x[1], x[2]))
    slots = {lxc: [None] * (model[lxc]["mask"] + 1) for lxc in model}
    where = {lxc: {} for lxc in model}
    disp, buckets = {}, collections.defaultdict(list)
    i = 0
    while i < len(ents):
        j = i
        while j < len(ents) and ents[j][0] == ents[i][0]:
            j += 1
        for d in range(POL_DISP_MAX + 1):
            put = []
            for (_, _, _, pre, mask, lxc, e) in ents[i:j]:
                s = int(pol_slot_direct(pre, d, mask))
                if slots[lxc][s] is not None:
                    break
                slots[lxc][s] = e
                put.append((lxc, s))
            if len(put) == j - i:
                break
            for lxc, s in put:
                slots[lxc][s] = None
        else:
            return None
        disp[ents[i][0]] = d
        for (lxc, s), x in zip(put, ents[i:j]):
            where[lxc][x[6][:2]] = s
            buckets[ents[i][0]].append((lxc,) + x[6][:2])
        i = j
    return dict(words=words, disp=disp, max_d=max(disp.values()), slots=slots, where=where,
                buckets=dict(buckets), linear=model, bloom=bloom)


def first_probe(dm, lxc, lo, hi):
    """the one slot a direct lookup of (lo, hi) reads in lxc's table, and what
    it holds"""
    m = dm["linear"][lxc]
    pre = int(E.pol_key_pre(lo, hi))
    d = dm["disp"].get(int(bucket_of(m["base"], pre, dm["words"])), 0)
    s = int(pol_slot_direct(pre, d, m["mask"]))
    return s, dm["slots"][lxc][s]


# ------------------------------------------------------------------ searches
def l4_ids(base, mask, words, hi=HI80, lo=256, top=1 << 20):
    """identities lo..top with the pre, bucket and home slot of their key
    {id, hi} in a table at `base` with `mask`, behind `words` Bloom words"""
    ids = np.arange(lo, top, dtype=np.uint64)
    pre = E.pol_key_pre(ids, hi)
    return ids, pre, bucket_of(base, pre, words), pre & U64(mask)


def same_bucket_and_home(base, mask, words, n=400, **kw):
    """-> up to n pairs of identities whose tcp/80 keys share a Bloom word and
    a home slot in the table at base, those homed at the highest slots first
    (from the last slot every displacement wraps)"""
    ids, pre, b, home = l4_ids(base, mask, words, **kw)
    code = ((U64(mask) - home) << U64(32)) | b
    order = np.argsort(code, kind="stable")
    c = code[order]
    k = np.flatnonzero(c[1:] == c[:-1])[:n]
    return [(int(ids[order[x]]), int(ids[order[x + 1]])) for x in k]


# --------------------------------------------------------------- the scaffold
def tables_for(pol, idents, extra_eps=0):
    """one endpoint per policy table (10.9.0.1 ...), each identity behind a
    /32 of 30.9.0.0/16"""
    n = len(pol) + extra_eps
    eps = E.endpoints4([S.ip4(f"10.9.0.{e + 1}") for e in range(n)])
    pfx = [(E.host4("30.9.0.0") + k, 32, int(v)) for k, v in enumerate(idents)]
    t = S.Tables(E.ipc4(pfx), eps, pol, np.zeros(0, S.PREFILTER_DT),
                 {EP0 + e: S.EP_SECLABEL for e in range(n)})
    return t, E.raw4([p[0] for p in pfx])


def ingress(t, src, dports, protos=(TCP,), frag=(0,), n=2048 + 37):
    """every source x endpoint x dport x proto x fragment flag, tiled to n
    headers (a partial last wave)"""
    la = S.local_v4_addrs(t)
    g = np.stack(np.meshgrid(np.arange(len(src)), np.arange(len(la)), np.arange(len(dports)),
                             np.arange(len(protos)), np.arange(len(frag)), indexing="ij"),
                 -1).reshape(-1, 5)
    h = E.hdr4(src[g[:, 0]], la[g[:, 1]], np.asarray(dports)[g[:, 2]],
               np.asarray(protos, np.uint8)[g[:, 3]],
               np.where(np.asarray(frag)[g[:, 4]], S.HF_FRAG, 0))
    n = max(n, len(h) + 37)
    return E.tile(h, n), g[np.arange(n) % len(g)]


def egress(t, sender, dst, dports, n=2048 + 37):
    """from endpoint `sender` to every destination x dport"""
    la = S.local_v4_addrs(t)
    g = np.stack(np.meshgrid(np.arange(len(dst)), np.arange(len(dports)), indexing="ij"),
                 -1).reshape(-1, 2)
    h = E.hdr4(la[sender], np.asarray(dst, np.uint32)[g[:, 0]], np.asarray(dports)[g[:, 1]])
    n = max(n, len(h) + 37)
    return E.tile(h, n), g[np.arange(n) % len(g)]


FILL = [901 + i for i in range(10)]


def fill_rows(n=10):
    return [(f, 0, 0, 0, 0) for f in FILL[:n]]


# ------------------------------------------------------------------ the cases
@functools.lru_cache(None)
def smallest(nkeys):
    """One endpoint whose table holds nkeys (2: 8 slots; 3: 16 slots, the
    smallest the builder's four slots per key give three keys) tcp/80 keys of
    one Bloom word, two of them with one home slot, so the word's
    displacement is not 0; chosen so that a displaced slot wraps past the
    table's last slot."""
    mask = E.pow2_at_least(max(8, 4 * nkeys)) - 1
    for a, c in same_bucket_and_home(0, mask, 64):
        ids, pre, b, _ = l4_ids(0, mask, 64, top=1 << 16)
        ba = int(bucket_of(0, E.pol_key_pre(a, HI80), 64))
        third = [int(x) for x in ids[b == U64(ba)] if int(x) not in (a, c)][:nkeys - 2]
        keys = [a, c] + third
        pol = {EP0: E.pol_rows([(i, 80, TCP, 0, 11000 + k) for k, i in enumerate(keys)])}
        dm = direct_model(pol)
        if dm is None or dm["disp"].get(ba, 0) == 0:
            continue
        d = dm["disp"][ba]
        wraps = [i for i in keys
                 if (int(E.pol_key_pre(i, HI80)) & mask) +
                 (d * ((int(E.pol_key_pre(i, HI80)) >> 16) | 1) & mask) > mask]
        if not wraps:
            continue
        absent = [int(x) for x in ids[b == U64(ba)] if int(x) not in keys][:3]
        t, src = tables_for(pol, keys + absent)
        h, g = ingress(t, src, [80, 81])
        return E.Case(t, h, 0, 0, dict(keys=keys, absent=absent, bucket=ba, d=d, wraps=wraps,
                                       dm=dm, grid=g, mask=mask))
    raise AssertionError("no such keys")


def shared_home(direction="ingress"):
    return _shared_home()[direction]


@functools.lru_cache(None)
def _shared_home():
    """One endpoint, a 64-slot table: ten L3 keys, a key of the endpoints'
    own SECLABEL (the egress second stage's), and two tcp/80 keys of one
    Bloom word with one home slot.  A second endpoint sends the egress batch
    (its own table: egress keys for the remote identities)."""
    for a, c in same_bucket_and_home(0, 63, 64):
        rows = fill_rows() + [(S.EP_SECLABEL, 80, TCP, 0, 12001),
                              (a, 80, TCP, 0, 11001), (c, 80, TCP, 0, 11002)]
        rows2 = [(a, 80, TCP, 1, 13001), (c, 0, 0, 1, 0), (FILL[0], 80, TCP, 1, 13002),
                 (S.WORLD_ID, 0, 0, 1, 0), (S.CLUSTER_ID, 0, 0, 1, 0)]
        pol = {EP0: E.pol_rows(rows), EP0 + 1: E.pol_rows(rows2)}
        dm = direct_model(pol)
        ba = int(bucket_of(0, E.pol_key_pre(a, HI80), 64))
        if dm is not None and dm["disp"].get(ba, 0) != 0:
            break
    else:
        raise AssertionError("no such keys")
    idents = [a, c] + FILL[:3] + [77]
    t, src = tables_for(pol, idents)
    claims = dict(a=a, c=c, bucket=ba, d=dm["disp"][ba], dm=dm, idents=idents)
    h, g = ingress(t, src, [80, 81], frag=(0, 1))
    ing = E.Case(t, h, 0, 0, dict(claims, grid=g))
    # egress from the second endpoint: to the first (local delivery, its
    # ingress policy looked up with the sender's SECLABEL) and to the remotes
    la = S.local_v4_addrs(t)
    h, g = egress(t, 1, np.concatenate([la[:1], src]), [80, 81])
    return dict(ingress=ing, egress=E.Case(t, h, 1, EP0 + 1, dict(claims, grid=g)))


@functools.lru_cache(None)
def shared_bucket():
    """Two endpoints' tables of 8 and 64 slots.  Keys a and c sit in both
    (other proxy ports in each); in the small table they share Bloom word and
    home slot, and the large table's key b falls into the same word (the
    word index is rotated per table): one displacement, not 0, fits both."""
    for a, c in same_bucket_and_home(0, 7, 64):
        ba = int(bucket_of(0, E.pol_key_pre(a, HI80), 64))
        ids, pre, b, _ = l4_ids(8, 63, 64, top=1 << 14)
        bs = [int(x) for x in ids[b == U64(ba)] if int(x) not in (a, c)]
        if not bs:
            continue
        kb = bs[0]
        pol = {EP0: E.pol_rows([(a, 80, TCP, 0, 11001), (c, 80, TCP, 0, 11002)]),
               EP0 + 1: E.pol_rows(fill_rows(8) + [(a, 80, TCP, 0, 21001), (c, 80, TCP, 0, 21002),
                                                   (kb, 80, TCP, 0, 21003)])}
        dm = direct_model(pol)
        if dm is None or dm["disp"].get(ba, 0) == 0:
            continue
        assert dm["linear"][EP0]["mask"] == 7 and dm["linear"][EP0 + 1]["mask"] == 63
        assert dm["linear"][EP0 + 1]["base"] == 8
        t, src = tables_for(pol, [a, c, kb, FILL[0], 77])
        h, g = ingress(t, src, [80, 81])
        return E.Case(t, h, 0, 0, dict(a=a, c=c, b=kb, bucket=ba, d=dm["disp"][ba], dm=dm, grid=g))
    raise AssertionError("no such keys")


HI8080 = int(S.htons(8080)) | TCP << 16


@functools.lru_cache(None)
def absent_l4():
    """One endpoint with 200 keys and a wildcard key for tcp/8080.  Found in
    the model: absent L4 keys the filter passes whose direct slot holds
    another key — id_a with its L3 key present, id_w (tcp/8080) with the
    wildcard key behind it, id_n with nothing (its L3 and wildcard keys fail
    the filter): DROP_POLICY from the one probe.  Each also as a fragment,
    which sees the L3 key only."""
    base = [(1000 + i, 0, 0, 0, 0) if i % 2 else (1000 + i, 80, TCP, 0, 15000 + i)
            for i in range(200)] + [(0, 8080, TCP, 0, 16000)]

    def maybe(dm, lo, hi):
        m = dm["linear"][EP0]
        h = E.pol_bloom_hash(E.pol_bloom_salt(m["base"]), E.pol_key_pre(lo, hi))
        b = E.bloom_bits(h)
        return (dm["bloom"][(h & U64(dm["words"] - 1)).astype(np.int64)] & b) == b

    def cands(dm, hi, behind):
        """identities whose L4 key {id, hi} is absent, passes the filter and
        probes an occupied slot; behind: also no L3 key passes"""
        m = dm["linear"][EP0]
        ids = np.arange(2000, 1 << 22, dtype=np.uint64)
        pre = E.pol_key_pre(ids, hi)
        bk = bucket_of(m["base"], pre, dm["words"]).astype(np.int64)
        darr = np.zeros(dm["words"], np.uint64)
        for k, v in dm["disp"].items():
            darr[k] = v
        occ = np.array([s is not None for s in dm["slots"][EP0]])
        ok = maybe(dm, ids, hi) & occ[pol_slot_direct(pre, darr[bk], m["mask"]).astype(np.int64)]
        if not behind:
            ok &= ~maybe(dm, ids, 0)
        return [int(x) for x in ids[ok][:64]]
    dm0 = direct_model({EP0: E.pol_rows(base)})
    for id_a in cands(dm0, HI80, True):
        pol = E.pol_rows(base + [(id_a, 0, 0, 0, 0)])
        dm = direct_model({EP0: pol})
        if id_a in cands(dm, HI80, True):
            break
    else:
        raise AssertionError("no id_a")
    assert not bool(maybe(dm, 0, HI80)), "the tcp/80 wildcard key passes the filter"
    id_w = cands(dm, HI8080, False)[0]
    id_n = next(x for x in cands(dm, HI80, False) if x != id_a)
    idents = [id_a, id_w, id_n, 1000, 1001, 1199]
    t, src = tables_for({EP0: pol}, idents)
    h, g = ingress(t, src, [80, 8080], frag=(0, 1), n=3072 + 5)
    return E.Case(t, h, 0, 0, dict(id_a=id_a, id_w=id_w, id_n=id_n, dm=dm, grid=g,
                                   ident=np.array(idents)[g[:, 0]],
                                   dport=np.array([80, 8080])[g[:, 2]], frag=g[:, 4] != 0))


@functools.lru_cache(None)
def equal_pre():
    """Two distinct keys with equal pre in one table: {lo, tcp/80} and {lo',
    hi'} with hi' = lo' * K ^ lo * K ^ hi, its top byte clear and its protocol
    TCP or UDP.  No displacement parts them."""
    K, lo = 0x9E3779B1, 5000
    lo2 = np.arange(256, 1 << 22, dtype=np.uint64)
    hi2 = E._mul32(lo2, K) ^ E._mul32(lo, K) ^ U64(HI80)
    ok = ((hi2 >> U64(24)) == 0) & np.isin((hi2 >> U64(16)) & U64(0xFF), [TCP, UDP]) & \
        (lo2 != U64(lo))
    lo2, hi2 = int(lo2[ok][0]), int(hi2[ok][0])
    assert (lo2, hi2) != (lo, HI80)
    assert int(E.pol_key_pre(lo, HI80)) == int(E.pol_key_pre(lo2, hi2))
    dport2, proto2 = int(S.htons(hi2 & 0xFFFF)), (hi2 >> 16) & 0xFF
    pol = {EP0: E.pol_rows(fill_rows(6) + [(lo, 80, TCP, 0, 11001),
                                           (lo2, dport2, proto2, 0, 11002)])}
    t, src = tables_for(pol, [lo, lo2, FILL[0], 77])
    h, g = ingress(t, src, [80, dport2], protos=(TCP, UDP))
    return E.Case(t, h, 0, 0, dict(keys=[(lo, HI80), (lo2, hi2)], dport2=dport2, proto2=proto2,
                                   grid=g))


# --------------------------------------------------- the C2 walk, restated
def first_probe_decides(policy, lxc, ident, dport, proto, frag, direct):
    """Per header that reaches lxc's policy stage (identity, raw dport,
    proto, fragment flag): does policy_resolve finish with the probe
    policy_issue made?  -> (probed: some key passed the filter, walks: the
    header enters policy_resolve_walk).  direct: under the direct placement
    (a miss at the one slot is an absence), else linear probing."""
    dm = direct_model(policy)
    m = dm["linear"][lxc]
    words, mask = dm["words"], m["mask"]
    darr = np.zeros(words, np.uint64)
    if direct:
        for k, v in dm["disp"].items():
            darr[k] = v
    tab = dm["slots"][lxc] if direct else m["slots"]
    klo = np.full(mask + 1, 0xFFFFFFFF, np.uint64)
    khi = np.full(mask + 1, 0xFFFFFFFF, np.uint64)
    for s, e in enumerate(tab):
        if e is not None:
            klo[s], khi[s] = e[0], e[1]
    ident, pp = E._a(ident), E._a(dport) | (E._a(proto) << U64(16))
    keys = [(ident, pp), (ident, np.zeros_like(pp)), (np.zeros_like(ident), pp)]
    n = len(ident)
    maybe = np.zeros((3, n), bool)
    slot = np.zeros((3, n), np.int64)
    for j, (lo, hi) in enumerate(keys):
        pre = E.pol_key_pre(lo, hi)
        h = E.pol_bloom_hash(E.pol_bloom_salt(m["base"]), pre)
        b = E.bloom_bits(h)
        w = (h & U64(words - 1)).astype(np.int64)
        maybe[j] = (dm["bloom"][w] & b) == b
        slot[j] = pol_slot_direct(pre, darr[w], mask).astype(np.int64)
    maybe[0] &= ~frag
    maybe[2] &= ~frag
    j0 = np.where(maybe[0], 0, np.where(maybe[1], 1, 2))
    probed = maybe.any(0)
    k = np.arange(n)
    s0 = slot[j0, k]
    lo0 = np.choose(j0, [keys[0][0], keys[1][0], keys[2][0]])
    hi0 = np.choose(j0, [keys[0][1], keys[1][1], keys[2][1]])
    hit = (klo[s0] == lo0) & (khi[s0] == hi0)
    empty = (klo[s0] == U64(0xFFFFFFFF)) & (khi[s0] == U64(0xFFFFFFFF))
    others = maybe.sum(0) > 1
    done = hit | ((empty | direct) & ~others)
    return probed, probed & ~done
