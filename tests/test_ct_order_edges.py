"""The streams of test_gpu_ct_order_edges.py (ct_order_edges.py) hold what
those tests are about — checked with the oracle alone, no GPU: the CT byte
sequences of the chain catalogues, one CT key per chain (on the dumped
rows), the related round's address pairs empty at the start, the structural
indices, and the arithmetic of ord_resolve_t's fallbacks against the source
lines it restates."""
import os
import re

import numpy as np
import pytest

import ct_order_edges as C
import oracle as O
from cilium_amd import synth as S

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "cilium_amd", "csrc")
FAMILIES_MODES = [(4, 0), (4, 3), (6, 0), (6, 3)]


def chain_bytes(st, want):
    """every chain member's CT byte is the catalogue's; -> members per chain"""
    exp = st.want_ct()
    m = st.chain >= 0
    bad = np.flatnonzero(m & (want["ct"] != exp))
    assert len(bad) == 0, [(int(i), st.chains[st.chain[i]][:2], int(st.member[i]),
                            hex(want["ct"][i])) for i in bad[:6]]
    # members of one key in chain order, keys of a chain interleaved
    for k in np.unique(st.key[m]):
        mem = st.member[st.key == k]
        assert (mem == np.arange(len(mem))).all(), k
    return np.bincount(st.chain[m], minlength=len(st.chains))


def one_key_per_chain(st):
    """all members of a chain key have one 5-tuple (A / D chains)"""
    fk = C.flow_key(st.h)
    for k in np.unique(st.key[st.key >= 0]):
        rows = fk[st.key == k]
        assert (rows == rows[0]).all(), k


def plain_rows(rows):
    """the CT rows without TUPLE_F_RELATED, as a set of bytes"""
    fam = rows[:, 3]
    flags = np.where(fam == 1, rows[:, 4 + 13], rows[:, 4 + 37])
    return {bytes(r[:44]) for r in rows[(flags & C.TUPLE_F_RELATED) == 0]}


def test_catalogue_is_the_state_machine():
    """the bytes the issue lists are what ctorder.hip's header comment
    derives: a stage sees the previous stage's outcome on its key"""
    for start, stages, want in C.CHAINS + C.STRUCT_CHAINS:
        assert C.model(start, stages)[0] == want, (start, stages)
    ends = {(s, st): C.model(s, st)[1] for s, st, _ in C.CHAINS}
    assert ends[("E", "ADADA")] and ends[("E", "DA")]            # end fresh
    assert not ends[("E", "DAD")] and not ends[("E", "AD")] and not ends[("E", "DDD")]


@pytest.mark.parametrize("family,mode", FAMILIES_MODES)
def test_pool(family, mode):
    """A is allowed and ESTABLISHED, D the same key dropped with DROP_POLICY
    while ESTABLISHED; by fragment (IPv4) and by proxy-egress mark"""
    p = C.pool(family, mode)
    assert len(p.A) == len(p.D) >= 40
    va, _, ca = C.look(p.t, p.A, mode)
    vd, _, cd = C.look(p.t, p.D, mode)
    assert (va == 0).all() and (ca == C.EST).all()
    assert (vd == C.DROP_POLICY).all() and (cd == C.EST).all()
    assert (C.flow_key(p.A) == C.flow_key(p.D)).all()
    assert len(np.unique(C.flow_key(p.A), axis=0)) == len(p.A)
    frag = (p.D.flags & S.HF_FRAG) != 0
    assert (frag == p.by_frag).all() and ((p.D.mark != 0) == ~p.by_frag).all()
    assert (p.D.mark[~frag] & 0xF00 == 0xB00).all()
    if family == 4:
        assert frag.sum() >= 40 and (~frag).sum() >= 20, (frag.sum(), len(frag))
    else:
        assert not frag.any()
    # new keys: 0c when allowed, 04 when denied
    a, d = C.new_keys(p, 50)
    assert (C.look(p.t, a, mode)[2] == (C.NEW | C.CREATE)).all()
    assert (C.look(p.t, d, mode)[2] == C.NEW).all()


@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("family,mode", FAMILIES_MODES)
def test_chain_stream(family, mode, cut):
    st = C.chain_stream(family, mode, cut)
    want = C.sequential(st.t, st.h, mode)
    per = chain_bytes(st, want)
    one_key_per_chain(st)
    nkeys = int(st.key.max()) + 1
    assert nkeys >= 200 and (per > 0).all(), (nkeys, per)
    # one CT key per chain key, on the dumped rows: the keys that end alive
    # are exactly the rows gained or kept, those that end gone are lost
    before = plain_rows(O.Oracle(st.t).ct_dump())
    after = plain_rows(want["rows"])
    alive = {(s, stg): C.model(s, stg)[1] for s, stg, _ in st.chains}
    n_gain = n_lost = 0
    for c, (s, stg, _) in enumerate(st.chains):
        nk = len(np.unique(st.key[st.chain == c]))
        n_gain += nk if (s == "N" and alive[(s, stg)]) else 0
        n_lost += nk if (s == "E" and not alive[(s, stg)]) else 0
    assert len(after - before) == n_gain and len(before - after) == n_lost
    # filler: plain hits, none on a chain's key
    fill = st.chain < 0
    assert np.isin(want["ct"][fill], [C.EST, 6]).all() and (want["ver"][fill] == 0).all()
    keys = {bytes(r) for r in C.flow_key(S.take(st.h, np.flatnonzero(~fill)))}
    assert not any(bytes(r) in keys for r in C.flow_key(S.take(st.h, np.flatnonzero(fill))))
    changed = C.order_changed(st.t, [st.h] if not cut else
                              [st.h.slice(0, st.split), st.h.slice(st.split, len(st.h))], mode)
    assert min(changed) > 0
    if cut:   # every cut position inside every chain
        for c, (_, stg, _) in enumerate(st.chains):
            m = st.chain == c
            first = np.array([st.member[m & (st.key == k) & (np.arange(len(st.h)) >= st.split)]
                              .min() for k in np.unique(st.key[m])])
            assert set(first.tolist()) == set(range(1, max(2, len(stg)))), (stg, set(first))


@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("family,mode", FAMILIES_MODES)
def test_related_stream(family, mode, cut):
    st = C.related_stream(family, mode, cut)
    want = C.sequential(st.t, st.h, mode)
    per = chain_bytes(st, want)
    assert (per > 0).all()
    # the address pairs hold no entry of any kind at the start
    rows = O.Oracle(st.t).ct_dump()
    held = set()
    for col in C.row_addrs(rows, family):
        held |= {bytes(r) for r in col}
    m = st.chain >= 0
    sa = C.addr_bytes(st.h.saddr)
    assert not any(bytes(r) in held for r in sa[m])
    # one address pair per chain key, no pair in two keys
    pair = {}
    for k, r in zip(st.key[m], sa[m]):
        assert pair.setdefault(bytes(r), int(k)) == int(k)
    assert len(pair) == len(np.unique(st.key[m]))
    # the errors' types: 3 (IPv4), all of 1 to 4 (IPv6)
    icmp = m & (st.h.proto == C.icmp_proto(family)) & ~np.isin(st.h.sport, [8, 128])
    assert set(np.unique(st.h.sport[icmp]).tolist()) == ({3} if family == 4 else {1, 2, 3, 4})
    # the ICMP error alone is CT_NEW against the tables
    assert ((C.look(st.t, S.take(st.h, np.flatnonzero(icmp)), mode)[2] & 7) == C.NEW).all()


@pytest.mark.parametrize("cut", [False, True])
def test_egress_stream(cut):
    st = C.egress_stream(cut)
    want = C.sequential(st.t, st.h, st.mode, st.ep)
    per = chain_bytes(st, want)
    assert st.mode == 1 and (per > 0).all()
    m = st.chain >= 0
    # the destination another local endpoint than the sender: no self cut
    assert (st.h.saddr[m] == S.LXC_IPV4).all() and (st.h.daddr[m] != S.LXC_IPV4).all()
    assert np.isin(st.h.daddr[m], S.local_v4_addrs(st.t)).all()
    # stage 1's key mixed, stage 0's only hit: the E chain's low nibbles all 5
    e = st.chain == 1
    assert ((want["ct"][e] & 0xF) == C.EST).all() and len(np.unique(want["ct"][e] >> 4)) > 1
    z = st.chain == 3
    assert (want["ct"][z] >> 4 == 0).all() and (want["ver"][z] == C.DROP_POLICY).all()


@pytest.mark.parametrize("mode", [0, 3])
def test_lb6_stream(mode):
    st = C.lb6_stream(mode)
    want = C.sequential(st.t, st.h, mode, want_pkt=True)
    chain_bytes(st, want)
    src = np.ascontiguousarray(want["pkt"][:, 0:4]).view(np.uint8).reshape(-1, 16)
    moved = (src != st.h.saddr).any(1)
    sel = lambda c, j: (st.chain == c) & (st.member == j)   # noqa: E731
    # a created flow's first packet as it came, its later ones reverse-NATed
    assert not moved[sel(0, 0)].any() and moved[sel(0, 1)].all() and moved[sel(0, 2)].all()
    # a live flow's hits translated, the packet after its delete not
    assert moved[sel(1, 0)].all() and not moved[sel(1, 2)].any()


@pytest.mark.parametrize("mode", [0, 3])
def test_structural_stream(mode):
    st = C.structural_stream(4, mode)
    want = C.sequential(st.t, st.h, mode)
    chain_bytes(st, want)
    one_key_per_chain(st)
    n = len(st.h)
    assert n == C.N_STRUCT and n % C.ORD_IT != 0 and n > C.WORD * C.LISTW
    at = np.flatnonzero(st.chain >= 0)
    assert len(at) == 7 * (len(C.BOUNDARIES) + 1)
    assert C.BOUNDARIES == [16, 64, 4096, 65_536]
    for b in C.BOUNDARIES:   # each chain has members on both sides of the boundary
        for c in (0, 1):
            i = np.flatnonzero((st.chain == c) & (np.abs(np.arange(n) - b) < 8))
            assert len(np.unique(st.key[i])) == 1
            assert (i < b).any() and (i >= b).any(), (b, c, i)
        assert st.chain[b - 1] == st.chain[b] == 0       # consecutive stages of one key
    assert st.chain[n - 1] >= 0 and st.chain[n - 2] >= 0
    fill = st.chain < 0
    assert np.isin(want["ct"][fill], [C.EST, 6]).all()


def test_long_stream():
    st = C.long_stream(4, 3)
    want = C.sequential(st.t, st.h, 3)
    per = chain_bytes(st, want)
    one_key_per_chain(st)
    assert per.tolist() == [C.N_ALT, C.N_HITS] and C.N_HITS > C.FOLD_LONG
    alt = want["ct"][st.chain == 0]
    assert (alt[0::2][1:] == 0x0c).all() and (alt[1::2] == 0x05).all()   # 1499 re-creates
    hits = want["ct"][st.chain == 1]
    assert hits[0] == 0x0c and (hits[1:] == 0x05).all()


def _source(name):
    """the file's text, runs of white space as one blank"""
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_fallback_arithmetic_restates_the_source():
    """every line ct_order_edges restates stands in the source as quoted: a
    changed constant fails here, not silently in the GPU cases"""
    have = _source("ctorder.hip")
    for ln in C.SOURCE:
        assert ln in have, ln
    have = _source("ctapply.hip")
    for ln in C.SOURCE_APPLY:
        assert ln in have, ln
    assert (C.ORD_IT, C.LISTW, C.FOLD_LONG) == (16, 1024, 512)
    assert C.BLOCK_STEP == 256 * C.ORD_IT
    # key sets: sized by the 8 creates of the first batch
    assert C.set_words(C.FIRST_CREATES) == 65_536 < C.N_SETFULL
    assert C.set_words(16_000) == 131_072
    # the participants' room behind a batch without participants
    assert C.part_room(65_536, 0) == 65_536 < 2 * C.N_TWICE
    assert C.N_TWICE < C.set_words(C.FIRST_CREATES)      # (its keys fit the sets)
    # the dense filter of a fresh context, and its re-mark
    assert C.filter_words(0) == 1024
    assert C.dense_remark(C.N_REMARK, C.filter_words(0))
    assert not C.dense_remark(4 * 1024, C.filter_words(0))


@pytest.mark.parametrize("kind", ["setfull", "twice", "remark"])
def test_fallback_streams(kind):
    f = C.fallback(kind)
    want = C.sequential(f.t, f.h, f.mode)
    b = f.bounds()
    ct = [want["ct"][x:y] for x, y in zip(b[:-1], b[1:])]
    create = C.NEW | C.CREATE
    if kind == "remark":
        assert len(f.batches) == 1
        assert (ct[0] == create).sum() == C.N_REMARK
        assert (ct[0] == C.NEW).sum() == C.N_REMARK_DROPS          # dropped, before the create
        assert C.order_changed(f.t, f.batches, f.mode) == [C.N_REMARK_DROPS]   # and after it
        return
    assert (ct[0] == create).sum() == C.FIRST_CREATES and len(ct[0]) == 64
    keys = np.unique(C.flow_key(f.batches[1]), axis=0)
    if kind == "setfull":
        assert len(keys) == C.N_SETFULL and (ct[1] == create).all()
    else:
        assert len(keys) == C.N_TWICE and len(ct[1]) == 2 * C.N_TWICE
        assert (ct[1] == create).sum() == (ct[1] == C.EST).sum() == C.N_TWICE
        assert C.order_changed(f.t, f.batches, f.mode)[1] == C.N_TWICE
    assert (ct[2] == create).sum() == 500           # the ordinary batch after it
    # the table has room: no growth stands between the batch and its passes
    assert len(O.Oracle(f.t).ct_dump()) > 262_144 // 2
