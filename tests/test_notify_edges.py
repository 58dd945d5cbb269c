"""The cases of test_gpu_notify_edges.py (notify_edges.py) hold what they
claim — checked on the CPU with numpy and the oracle alone: the word domain
against what the oracle's classify gives over every golden fixture, every
selection pattern against a reshape into waves, rounds and blocks, the scan
sizes against k_nt_scan's own chunking, the caps against the running record
count, and the field batches against the oracle's own records (every length
cap binding and not binding, a drop label losing its high half where a trace
record keeps it).  No GPU."""
import numpy as np
import pytest

import golden_io as G
import notify_edges as E
import oracle as O


@pytest.fixture(scope="module")
def oracle():
    return O.Oracle(E.tables())


def events(oracle, c, traces=True):
    return oracle.events(c.h, c.mode, c.ep, c.ver, c.ide, c.words, traces=traces)


# ------------------------------------------------------------------ the domain
@pytest.fixture(scope="module")
def measured():
    """(family, mode) -> the (kind, NATLEN) pairs, and the trace words'
    (class, reason) pairs, of every fixture's event words"""
    kinds, traces = {}, {}
    for name in G.names():
        g = G.Golden(name)
        o = O.Oracle(g.tables)
        if g.clock is not None:
            o.set_clock(int(np.median(g.clock[g.clock != 0xFFFFFFFF])))
        w = o.classify(g.headers, g.mode, g.ep_lxc, nthreads=8, want_notify=True)[3]
        w = np.unique(w[w != 0] & np.uint32(0xFFFF0000))
        key = (g.headers.family, g.mode)
        assert not (w >> 25).any(), name      # (no bit above CFC_NT_NATLEN)
        k = (w >> 16) & 0xF
        kinds.setdefault(key, set()).update(zip(k.tolist(), ((w >> 24) & 1).tolist()))
        assert not ((w >> 20) & 0xF)[k < 4].any(), name   # (a drop word: no trace fields)
        t = w[k >= 4]
        traces.setdefault(key, set()).update(zip(((t >> 22) & 3).tolist(),
                                                 ((t >> 20) & 3).tolist()))
    return kinds, traces


def test_domain_is_what_classify_produces(measured):
    kinds, traces = measured
    for key, dom in E.DOMAIN.items():
        lit = {(k, nat) for k, nats in dom.items() for nat in nats}
        assert lit <= kinds[key], (key, lit - kinds[key])
        cl, rs = E.TRACE_FIELDS[key[1]]
        assert set(cl) <= {c for c, r in traces[key]}, key
        assert set(rs) <= {r for c, r in traces[key]}, key
    assert {k for dom in E.DOMAIN.values() for k in dom} == set(range(1, 8))


def test_every_case_stays_inside_the_domain():
    cases = [E.pattern_case(f, m, 257, p, tr) for f, m in E.PATTERN_MODES
             for p in E.PATTERNS for tr in (0, 1)]
    cases += [E.field_case(f, m) for f, m in E.FIELD_MODES]
    cases += [E.cap_case(f, tr) for f in (4, 6) for tr in (0, 1)]
    cases += [E.slice_case(f) for f in (4, 6)]
    cases += [E.skb_hash_case(f) for f in (4, 6)] + [E.flow_hash_case(f) for f in (4, 6)]
    cases += [E.small_case(0), E.small_case(1), E.scan_case(1024)]
    for c in cases:
        w = np.unique(c.words[c.words != 0] & np.uint32(0xFFFF0000))
        dom = E.DOMAIN[(c.family, c.mode)]
        cl, rs = E.TRACE_FIELDS[c.mode]
        for x in w.tolist():
            k, nat = (x >> 16) & 0xF, (x >> 24) & 1
            assert k in dom and nat in dom[k] and not x >> 25, hex(x)
            if k >= 4:
                assert (x >> 22) & 3 in cl and (x >> 20) & 3 in rs, hex(x)
            else:
                assert not (x >> 20) & 0xF, hex(x)
        # the NAT length of an IPv6 batch never goes below zero
        nat = (c.words & E.NATLEN) != 0
        if c.family == 6:
            assert (np.asarray(c.h.length)[nat] >= 40).all()


def test_tables():
    t = E.tables()
    labs = list(t.seclabel.values())
    assert all(v > 0xFFFF and (v & 0xFFFF) != v for v in labs)
    assert len({v & 0xFFFF for v in labs}) == len(labs)
    ifx = {int(e["lxc_id"]): int(e["ifindex"]) for e in t.endpoints}
    assert {1, 65535, E.EP} <= set(ifx) and 0 not in ifx and E.LXC_NONE_MID not in ifx
    assert len(set(ifx.values())) == len(ifx) and max(ifx.values()) > 0xFFFF
    assert set(t.seclabel) == set(ifx)
    for e in t.endpoints:     # (one ifindex per LXC_ID under both families)
        assert int(e["ifindex"]) == E.ENDPOINTS[int(e["lxc_id"])][1]


# ---------------------------------------------------------------- 1: patterns
def _grid(sel):
    """selected per (block, round, wave, lane)"""
    pad = -len(sel) % E.BLOCK
    return np.concatenate([sel, np.zeros(pad, bool)]).reshape(-1, 16, 4, 64)


@pytest.mark.parametrize("traces", [0, 1])
@pytest.mark.parametrize("family,mode", E.PATTERN_MODES)
def test_patterns_select_what_their_names_say(oracle, family, mode, traces):
    for n in E.SIZES:
        exists = _grid(np.ones(n, bool))
        for name in E.PATTERNS:
            c = E.pattern_case(family, mode, n, name, traces)
            sel = E.selected(c.words, traces)
            np.testing.assert_array_equal(sel, E.pattern_mask(name, n))
            # (the oracle selects the same headers)
            np.testing.assert_array_equal(events(oracle, c, traces)[1], np.flatnonzero(sel))
            g = _grid(sel)
            want = {"none": np.zeros_like(exists), "all": exists}.get(name)
            if name in ("lane0", "lane63", "lanes31_32"):
                lanes = {"lane0": [0], "lane63": [63], "lanes31_32": [31, 32]}[name]
                want = np.zeros_like(exists)
                want[..., lanes] = exists[..., lanes]
            elif name == "wave3":
                want = np.zeros_like(exists)
                want[:, :, 3] = exists[:, :, 3]
            elif name == "round15":
                want = np.zeros_like(exists)
                want[:, 15] = exists[:, 15]
            elif name in ("last", "first"):
                want = np.zeros(n, bool)
                want[-1 if name == "last" else 0] = True
                want = _grid(want)
            if want is not None:
                assert (g == want).all(), (name, n)
                assert g.sum() == want.sum()
            else:   # about a third, in every wave of a batch of some size
                assert name == "third"
                if n >= 255:
                    per_wave = g.sum(-1)[exists.sum(-1) == 64]
                    assert (per_wave > 4).all() and (per_wave < 44).all()
            # what lies between the selected words is not only zeros
            if 0 < sel.sum() < n - 8:
                rest = c.words[~sel]
                assert (rest != 0).any() and (rest == 0).any(), (name, n)
                if traces:
                    assert (((rest[rest != 0] >> 22) & 3) == 0).all()
                else:   # a call without traces passes over sendable trace words
                    assert (((rest >> 22) & 3) != 0).any()
    # lanes 0 and 63 and a whole wave do occur at the sizes chosen
    assert E.pattern_mask("lane63", 63).sum() == 0 and E.pattern_mask("lane63", 64).sum() == 1
    assert E.pattern_mask("wave3", 255).sum() == 63 and E.pattern_mask("wave3", 257).sum() == 64
    assert E.pattern_mask("round15", 4095).sum() == 255
    assert E.pattern_mask("round15", 8193).sum() == 512


# -------------------------------------------------------------------- 2: scan
@pytest.mark.parametrize("nb,per", zip(E.SCAN_NB, (1, 2, 3)))
def test_scan_cases(nb, per):
    c = E.scan_case(nb)
    n = len(c)
    assert n == E.scan_n(nb) and (n + E.BLOCK - 1) // E.BLOCK == nb
    assert n == {1024: 4_194_304, 1025: 4_194_305, 2049: 8_388_609}[nb]
    assert E.scan_per(nb) == per
    for traces in (0, 1):
        cnt = E.block_counts(c.words, traces)
        assert len(cnt) == nb and cnt.sum() < E.SCAN_MAX_RECORDS
        assert (cnt == 0).any() and (cnt == E.BLOCK).any()
        mid = cnt[(cnt != 0) & (cnt != E.BLOCK)]
        assert mid.max() < 257 and len(np.unique(mid)) > 30
        # k_nt_scan's chunks: thread t owns blocks [t per, min(nb, t per + per))
        busy = 0
        for t in range(E.SCAN_THREADS):
            b0, b1 = t * per, min(nb, t * per + per)
            if b0 < b1:
                busy += 1
                if b1 - b0 > 1:
                    assert len(set(cnt[b0:b1].tolist())) > 1, (t, cnt[b0:b1])
        # per 1: every thread owns a block and neighbours differ; else idle
        # threads, some of them with b0 > nb
        if per == 1:
            assert busy == E.SCAN_THREADS and (np.diff(cnt) != 0).all()
        else:
            assert busy < E.SCAN_THREADS and (E.SCAN_THREADS - 1) * per > nb
        # the ragged last block holds a record
        if n % E.BLOCK:
            assert cnt[-1] == 1 and n % E.BLOCK == 1
    # the one-block last chunk (per 2): thread 512 owns block 1024 alone
    assert min(1025, 512 * 2 + 2) - 512 * 2 == 1
    # a full block, a partly filled one (43 records over 12 rounds and as
    # many lanes) and an empty one
    s = E.selected(c.words[5 * E.BLOCK:9 * E.BLOCK], 0).reshape(4, 16, 4, 64)
    assert s[0].all() and s[1].sum() == 43 and not s[3].any()
    assert s[1].any((1, 2)).sum() == 12 and s[1].any((0, 1)).sum() == 43


# -------------------------------------------------------------------- 3: caps
@pytest.mark.parametrize("traces", [0, 1])
@pytest.mark.parametrize("family", [4, 6])
def test_cap_case(oracle, family, traces):
    c = E.cap_case(family, traces)
    caps, T, (w, r, b) = E.caps_of(c, traces)
    rec, idx = events(oracle, c, traces)
    assert len(rec) == T and len(c) == E.CAP_N
    assert 0 < w < r < b < T - 1 and caps[0] == 0 and caps[-1] == T + 1
    # header indices on both sides of each cap: inside the first wave, at the
    # first round's and the first block's end
    assert idx[w - 1] < E.CAP_INSIDE_WAVE <= idx[w] < E.WAVE
    assert idx[r - 1] < E.ROUND <= idx[r] and idx[b - 1] < E.BLOCK <= idx[b]
    assert {w - 1, w, w + 1, r - 1, r, r + 1, b - 1, b, b + 1, 0, 1, T - 1, T, T + 1} == set(caps)
    assert (E.block_counts(c.words, traces) > 0).all() and idx[-1] == E.CAP_N - 1


# ------------------------------------------------------------------ 4: fields
@pytest.mark.parametrize("family,mode", E.FIELD_MODES)
def test_field_case(oracle, family, mode):
    c = E.field_case(family, mode)
    rec, idx = events(oracle, c)
    idx = idx.astype(np.int64)
    w = c.words[idx]
    kind = (w >> 16) & 0xF
    # every shape the mode has, with every edge of every field
    shapes = {(k, nat, r, cl) for k, nat, r, cl in E.tuples(family, mode)}
    seen = set(zip(((c.words >> 16) & 0xF).tolist(), ((c.words >> 24) & 1).tolist(),
                   ((c.words >> 20) & 3).tolist(), ((c.words >> 22) & 3).tolist()))
    assert seen == shapes
    for k, nat, r, cl in shapes:
        m = c.words >> 16 == E.word(k, 0, nat, r, cl) >> 16
        lens = E.LENGTHS_NAT6 if nat and family == 6 else E.LENGTHS
        assert set(lens) <= set(c.h.length[m].tolist())
        assert set(E.VERDICTS) <= set(c.ver[m].tolist())
        assert set(E.IDENTITIES) <= set(c.ide[m].tolist())
        assert set(E.LXC_EDGES) <= set((c.words[m] & 0xFFFF).tolist())
    # each length cap binds and does not bind: drops at 128, traces at 128,
    # 1500 and 1
    caps = [(kind < 4, 128)] + [((kind >= 4) & (((w >> 22) & 3) == cl), ln)
                                for cl, ln in E.MON_LEN.items()
                                if cl in E.TRACE_FIELDS[mode][0]]
    for m, ln in caps:
        lo, lc = rec["len_orig"][m], rec["len_cap"][m]
        assert ((lc < lo) & (lc == ln)).any() and ((lc == lo) & (lo <= ln)).any(), ln
        assert (lc == np.minimum(lo, ln)).all()
    # NAT lengths: 20 more (IPv4) or less (IPv6) than the header's, at the caps
    nat = (w & E.NATLEN) != 0
    if nat.any():
        d = rec["len_orig"][nat].astype(np.int64) - c.h.length[idx][nat]
        assert (d == (20 if family == 4 else -20)).all()
        if family == 4:
            assert rec["len_orig"].max() == 65535 + 20
    # subtype = -verdict over its 8 bits: 1, 130, 255 and 0 (-256)
    d = kind < 4
    assert {1, 130, 255, 0} <= set(rec["subtype"][d].tolist())
    # a drop label loses its high half, the trace record of the same
    # identity keeps it: the peer identity is a drop's dst (egress kind 2) or
    # src (kind 3), a trace's dst (TO_STACK) or src (TO_LXC)
    dk, dcol, tk, tcol = ((2, "dst_label", 7, "dst_label") if mode == E.EGRESS
                          else (3, "src_label", 4, "src_label"))
    ide = c.ide[idx]
    big = ide > 0xFFFF
    dm, tm = (kind == dk) & big, (kind == tk) & big
    assert dm.any() and tm.any()
    assert (rec[dcol][dm] == (ide[dm] & 0xFFFF)).all() and (rec[dcol][dm] != ide[dm]).all()
    assert (rec[tcol][tm] == ide[tm]).all()
    assert set(ide[dm].tolist()) & set(ide[tm].tolist())
    # SECLABELs likewise (kind 3: the destination's; kind 4 the same in full)
    lab = np.array([E.ENDPOINTS.get(int(x), (0, 0))[0] for x in (w & 0xFFFF)], np.uint32)
    m3, m4 = (kind == 3) & (lab != 0), (kind == 4) & (lab != 0)
    assert m3.any() and (rec["dst_label"][m3] == (lab[m3] & 0xFFFF)).all()
    assert m4.any() and (rec["dst_label"][m4] == lab[m4]).all()
    # ids without an endpoint: label and ifindex 0
    none = np.isin(w & 0xFFFF, [0, E.LXC_NONE_MID]) & ((kind == 3) | (kind == 4))
    assert none.any() and not rec["ifindex"][none].any() and not rec["dst_label"][none].any()
    assert (rec["ifindex"][(kind == 3) & ((w & 0xFFFF) == 65535)] == 0x12345).all()


# -------------------------------------------------------------------- 5: hash
@pytest.mark.parametrize("family", [4, 6])
def test_hash_cases(oracle, family):
    c = E.skb_hash_case(family)
    rec, idx = events(oracle, c)
    assert len(rec) == len(c)
    np.testing.assert_array_equal(rec["hash"], c.h.hash)
    assert set(E.HASH_EDGES) <= set(rec["hash"][rec["type"] == 1].tolist())
    assert set(E.HASH_EDGES) <= set(rec["hash"][rec["type"] == 4].tolist())
    c = E.flow_hash_case(family)
    h = c.h
    rec, idx = events(oracle, c)
    assert len(rec) == len(c) and len(c) % 2 == 0
    # header 2k + 1 is header 2k reversed, and the oracle's hash is symmetric
    a, b = slice(0, None, 2), slice(1, None, 2)
    assert (h.saddr[a] == h.daddr[b]).all() and (h.daddr[a] == h.saddr[b]).all()
    assert (h.sport[a] == h.dport[b]).all() and (h.dport[a] == h.sport[b]).all()
    np.testing.assert_array_equal(rec["hash"][a], rec["hash"][b])
    sa = h.saddr if family == 4 else [bytes(x) for x in h.saddr]
    da = h.daddr if family == 4 else [bytes(x) for x in h.daddr]
    same = np.array([x == y for x, y in zip(sa, da)])
    assert same.any() and (h.sport == h.dport).any() and (~same & (h.sport != h.dport)).any()
    assert {0, 0xFFFF} <= set(h.sport.tolist()) and set(E.HASH_PROTOS) == set(h.proto.tolist())
    if family == 6:   # pairs that differ in exactly one word, each word once
        w = np.ascontiguousarray(h.saddr).view("<u4") != np.ascontiguousarray(h.daddr).view("<u4")
        one = w[w.sum(1) == 1]
        assert one.any(0).all()
    # distinct tuples hash apart (32 bits over a few hundred tuples)
    assert len(np.unique(rec["hash"][a])) == len(rec["hash"][a])


def test_small_and_slice_cases(oracle):
    for c in (E.small_case(0), E.small_case(1), E.slice_case(4), E.slice_case(6)):
        rec, idx = events(oracle, c)
        assert 0 < len(rec) < len(c) and set(rec["type"].tolist()) == {1, 4}
    a, b = events(oracle, E.small_case(0))[0], events(oracle, E.small_case(1))[0]
    assert a.tobytes() != b.tobytes()
