"""The streams of test_gpu_svc_edges.py (svc_edges.py) hold what they claim —
checked on the CPU with the oracle alone: the Python restatement of the
layout.h mixers against the host self-test's known answers (`selftest kat
svchash`), the restated CT_SERVICE key words and the restated replay
(svc_next) against the oracle's CT dump and packet outputs, the expected
svc_ordered of every stream against the headers the builder marks, a header
that differs between packet order and the batch-start view in every stream
that claims one (and only at marked headers), and the placements the
structural streams name.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import svc_edges as E
from cilium_amd import synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = [4, 6]
NATLEN = 1 << 24


def test_hash_restatement_matches_layout_h():
    """selftest prints LCG-drawn (d, s, z, w) rows of both families with
    ct_hash4/6 and ct_home4/6; the restatement gives the same"""
    csrc = os.path.join(ROOT, "cilium_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-s", "selftest"], check=True)
    r = subprocess.run([os.path.join(csrc, "build", "selftest"), "kat", "svchash"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    n = {4: 0, 6: 0}
    homes = {4: set(), 6: set()}
    fl, owners = set(), set()
    for line in r.stdout.splitlines():
        w = line.split()
        assert w[0] == "svchash", line
        v = [int(x, 16) for x in w[2:]]
        if w[1] == "4":
            d, s, z, kw, h, home = v
            assert E.ct_hash4(d, s, z, kw) == h and E.ct_home4(d, s, z, kw) == home, line
        else:
            d, s, (z, kw, h, home) = tuple(v[0:4]), tuple(v[4:8]), v[8:]
            assert E.ct_hash6(d, s, z, kw) == h and E.ct_home6(d, s, z, kw) == home, line
        assert E.khash((d, s, z, kw)) == h and E.khome((d, s, z, kw)) == home
        fam = int(w[1])
        n[fam] += 1
        homes[fam].add(home)
        fl.add((kw >> 8) & 7)
        owners.add(kw >> 11)
    # the rows are about something: both families, every flag value, local
    # and global owners, and the reversed rows share their home
    assert n == {4: 200, 6: 200} and fl == set(range(8)) and 0 in owners and len(owners) > 20
    assert all(len(homes[f]) == 150 for f in FAMILIES)


def _seq(t, h):
    o = O.Oracle(t)
    r = o.classify(h, E.EGRESS, E.EP, want_ct=True, want_pkt=True, apply_ct=True)
    return o, r


def _bat(t, h):
    return O.Oracle(t).classify(h, E.EGRESS, E.EP, want_ct=True, want_pkt=True)


def _differ(s, b):
    """headers whose action, CT byte or packet output differ between views"""
    return (s[0] != b[0]) | (s[3] != b[3]) | (s[4] != b[4]).any(1)


def _service_of(e, h, i):
    w = E.addr_words(h.daddr[i], e.family)
    return next(k for k, v in e.vip.items() if E.addr_words(v, e.family) == w)


def check_stream(c):
    """what every one-batch stream must hold -> (oracle, sequential view)"""
    e = E.env(c.family)
    h, p = c.h, c.plan
    assert p.svc_ordered == int(p.marked.sum())
    assert not (p.marked & ~p.listed).any()
    o, s = _seq(c.t, h)
    b = _bat(c.t, h)
    d = _differ(s, b)
    if p.svc_ordered and h.hash is not None:
        assert d.any(), "packet order shows nowhere"
    assert not (d & ~p.marked).any(), np.flatnonzero(d & ~p.marked)
    # the restated keys and the restated replay against the oracle's maps:
    # the CT_SERVICE entries after the batch are the history's and the
    # listed keys', each with the slave the plan leaves
    got = E.ct_service_keys(S.ct_from_rows(o.ct_dump()), c.family)
    want = E.Pass(c.t, c.family)
    want.batch(h)
    # (but for the ICMP "related" entry every create writes beside its own,
    # conntrack.h:648-660: no stream here sends an ICMP error)
    plain = lambda m: {k: v[0] for k, v in m.items() if not k[3] & 0x200}   # noqa: E731
    assert plain(got) == plain(want.entry)
    assert set(p.unstable) <= set(got) and len(set(p.unstable)) == len(p.unstable)
    # the word's slave is the backend the oracle's packet reached
    al = 1 if c.family == 4 else 4
    pkt = s[4]
    for i in np.flatnonzero(p.marked):
        svc = _service_of(e, h, i)
        tgt = e.backends[svc].get(int(p.slave[i]))
        if tgt is None or svc == "lo" or p.reselect[i]:
            continue
        da = tuple(int(x) for x in pkt[i, al:2 * al])
        tw = E.addr_words(tgt, c.family)
        assert da == ((tw,) if c.family == 4 else tw), (i, svc, p.slave[i])
    return o, s


@pytest.mark.parametrize("family", FAMILIES)
def test_key_words_match_oracle_ct_dump(family):
    """a handful of flows of every kind — TCP and UDP to L3 services and to
    the L4 one, an ICMP echo to an L3 service: the restated (d, s, z, w) are
    the CT_SERVICE rows the oracle's maps hold afterwards"""
    icmp = S.IPPROTO_ICMPV6 if family == 6 else S.IPPROTO_ICMP
    h = S.concat([E.flow(family, "a", 7001, [1, 2]),
                  E.flow(family, "b", 7002, [3, 4], dport=53, proto=E.UDP),
                  E.flow(family, "l4", 7003, [5, 6]),
                  E.flow(family, "l4", 7004, [7, 8], proto=E.UDP),
                  E.flow(family, "c", 128 if family == 6 else 8, [9, 10], dport=0x2211,
                         proto=icmp)])
    c = E.case(family, [h])
    assert len(c.plan.unstable) == 5 and c.plan.svc_ordered == 5
    assert len({k[3] for k in c.plan.unstable}) == 3     # TCP, UDP, ICMP
    o, s = check_stream(c)
    got = E.ct_service_keys(S.ct_from_rows(o.ct_dump()), family)
    assert set(c.plan.unstable) <= set(got)
    assert not set(c.plan.unstable) & set(E.ct_service_keys(c.t.ct, family))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", list(E.STREAMS))
def test_stream_holds_its_claim(family, name):
    c = E.stream(family, name)
    assert c.plan.svc_ordered > 0
    check_stream(c)


@pytest.mark.parametrize("family", FAMILIES)
def test_one_flow_and_distinct_sizes(family):
    for n in E.SIZES:
        c = E.one_flow(family, n)
        assert len(c.h) == n and c.plan.svc_ordered == n - 1 and c.plan.listed.all()
        o, s = check_stream(c)
        if n > 1:   # own hashes: two backends or more would be selected
            assert len({E.svc_next(E.Lb(c.t.lb4 if family == 4 else c.t.lb6, family),
                                   E.key_words(c.h, i)[0], E.TCP, E._pt(c.h, i),
                                   int(c.h.hash[i]), (False, 0))[0][1]
                        for i in range(n)}) >= 2
            assert len(np.unique(s[4][:, 1 if family == 4 else 4])) == 1
        c = E.distinct(family, n)
        assert len(c.h) == n and c.plan.svc_ordered == 0
        assert c.plan.listed.all() and len(c.plan.unstable) == n     # m == n
        o, s = check_stream(c)
        assert not _differ(s, _bat(c.t, c.h)).any()


@pytest.mark.parametrize("family", FAMILIES)
def test_one_flow_without_hash_array(family):
    """every header of the flow has the engine's flow hash: the views agree,
    the words are handed on all the same"""
    c = E.one_flow(family, 257, hashed=False)
    assert c.h.hash is None and c.plan.svc_ordered == 256
    assert len(set(int(x) for x in O.flow_hash(c.h, np.arange(257)))) == 1
    o, s = check_stream(c)
    b = _bat(c.t, c.h)
    assert not ((s[0] != b[0]) | (s[4] != b[4]).any(1)).any()


@pytest.mark.parametrize("family", FAMILIES)
def test_straddle_placements(family):
    for which, want in (("across", [(250, 262)]), ("abut", [(249, 255), (256, 261)])):
        c = E.straddle(family, which)
        lst, runs = E.sorted_list(c.h, c.plan)
        assert len(lst) == len(c.h) >= 300
        assert [r for r in runs if r[1] > r[0]] == want
        # shuffled: a run's headers are not neighbours in the batch
        for a, b in want:
            idx = [i for _, i in lst[a:b + 1]]
            assert idx == sorted(idx) and max(np.diff(idx)) > 1


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("k", [2, 3])
def test_collide(family, k):
    c = E.collide(family, k)
    e = E.env(family)
    keys = c.plan.unstable
    assert len(keys) == k and len({E.khash(x) for x in keys}) == 1
    assert len({x[0] for x in keys}) == k and len({x[2] for x in keys}) == k
    lst, runs = E.sorted_list(c.h, c.plan)
    assert runs == [(0, len(c.h) - 1)]
    assert [c.plan.keys[i] for i in range(k)] == keys      # A B (C) A B (C) ...
    assert all(x[2] & 0xFFFF and x[2] >> 16 for x in keys)
    # a replay that took the run for one key: every header renamed to the
    # first key.  The slaves its later headers carry are not the true ones
    o, s = _seq(c.t, c.h)
    hm = E.merged(c)
    pm = E.Pass(c.t, family).batch(hm)
    assert pm.svc_ordered == len(c.h) - 1 != c.plan.svc_ordered
    other = np.flatnonzero([c.plan.keys[i] != keys[0] for i in range(len(c.h))])
    assert (pm.slave[other] != c.plan.slave[other]).all()
    # ... and a slave of b's or c's is no slot of a
    assert max(int(x) for x in c.plan.slave) > e.count["a"]
    om, sm = _seq(c.t, hm)
    al = 1 if family == 4 else 4
    assert ((s[4][other, al:2 * al] != sm[4][other, al:2 * al]).any(1)).all()


@pytest.mark.parametrize("family", FAMILIES)
def test_same_home(family):
    c = E.same_home(family)
    a, b = c.plan.unstable
    assert a != b and E.khome(a) == E.khome(b) and E.khash(a) != E.khash(b)
    assert [c.plan.keys[i] for i in range(4)] == [a, b, a, b]


@pytest.mark.parametrize("family", FAMILIES)
def test_reslave_chains(family):
    e = E.env(family)
    stored = E.ct_service_keys(e.t.ct, family)
    for which, resel, first in (("i", [0], 1), ("ii", [0, 1, 2], 3), ("iii", [0], 1)):
        c = E.reslave(family, which)
        p = c.plan
        key = p.unstable[0]
        assert (key in stored) == (which != "iii")
        if which != "iii":
            assert stored[key][0] == 2 and 2 not in e.backends["gap"]
        assert list(np.flatnonzero(p.reselect)) == resel
        # the words: the gone slot while the chain lasts, then the live one
        assert [int(x) for x in p.slave[1:]] == [2] * (len(resel) - 1) + \
            [first] * (len(c.h) - len(resel))
        o, s = check_stream(c)
        assert (s[1] == 0).all()
    c = E.reslave(family, "iv")
    o, s = check_stream(c)
    assert (s[1] == E.DROP_NO_SERVICE).all() and (s[0] == 2).all()
    got = E.ct_service_keys(S.ct_from_rows(o.ct_dump()), family)
    assert got[c.plan.unstable[0]][0] == 2     # the entry exists, no backend answers
    # batch view: the headers whose own hash selects a live slot pass
    assert (_bat(c.t, c.h)[1] == 0).any()


def test_reslave_loopback_entry():
    c = E.reslave(4, "loop")
    stored = E.ct_service_keys(c.t.ct, 4)
    assert stored[c.plan.unstable[0]] == (2, 1)
    assert sum(v[1] for v in stored.values()) == 1
    check_stream(c)


@pytest.mark.parametrize("family", FAMILIES)
def test_gates(family):
    c = E.gates(family)
    p, h = c.plan, c.h
    icmp = S.IPPROTO_ICMPV6 if family == 6 else S.IPPROTO_ICMP
    echo = (h.proto == icmp) & ((h.sport & 0xFF) == (128 if family == 6 else 8))
    tcp = (h.proto == E.TCP) & np.array([E.addr_words(a, family) ==
                                         E.addr_words(E.env(family).own, family)
                                         for a in h.saddr])
    assert (p.listed == (echo | tcp)).all() and echo.sum() == tcp.sum() == 6
    assert (~p.listed).sum() == (18 if family == 6 else 12)
    # the echoes differ in code and identifier and are one key
    assert len({(int(a), int(b)) for a, b in zip(h.sport[echo], h.dport[echo])}) == 6
    assert len(p.unstable) == 2 and p.svc_ordered == 10
    o, s = check_stream(c)
    assert (s[1][~p.listed] != 0).all()


@pytest.mark.parametrize("family", FAMILIES)
def test_denied_first(family):
    c = E.denied_first(family)
    o, s = check_stream(c)
    assert (s[1] == E.DROP_POLICY).all()
    lab, _ = o.ipcache_lookup(family, np.array(list(E.env(family).backends["deny"].values())))
    assert set(int(x) for x in lab) == {E.env(family).deny_identity}


@pytest.mark.parametrize("family", FAMILIES)
def test_stale_and_growth_batches(family):
    c = E.stale_and_growth(family)
    assert [len(h) for h in c.batches] == [513, 513, 513, 2049, 513, 513]
    assert c.svc_ordered == [512, 0, 0, 2048, 0, 0]
    assert not c.plans[1].listed.any() and not c.plans[4].listed.any()
    # the armed batches: one listed header, the last; the others' stored
    # slaves are mostly not the slave the words before them carried
    for k, left in ((2, c.plans[0].slave[1:]), (5, c.plans[3].slave[1:513])):
        assert list(np.flatnonzero(c.plans[k].listed)) == [512]
        stored = E.ct_service_keys(c.t.ct, family)
        own = np.array([stored[c.plans[k].keys[i]][0] for i in range(512)])
        assert len(set(left)) == 1 and (own[1:] != left[:511]).sum() > 300
    # batch 2 in packet order after batch 1: every header the stored slave,
    # which is not what every header's own hash selects
    o = O.Oracle(c.t)
    al = 1 if family == 4 else 4
    outs = [o.classify(h, E.EGRESS, E.EP, want_ct=True, want_pkt=True, apply_ct=True)
            for h in c.batches]
    assert len(np.unique(outs[1][4][:, al])) == 1
    lb = E.Lb(c.t.lb4 if family == 4 else c.t.lb6, family)
    h = c.batches[1]
    own = {E.svc_next(lb, E.key_words(h, i)[0], E.TCP, E._pt(h, i), int(h.hash[i]),
                      (False, 0))[0][1] for i in range(len(h))}
    assert len(own) == 3


@pytest.mark.parametrize("m", [1, 257])
def test_nat64_hop_stream(m):
    t, h, at = E.nat64_hops(m)
    assert len(h) == 4 * m and len(at) == m
    if m > 1:
        assert list(at) != list(range(m))     # the hop rows' indices are not the batch's
    o = O.Oracle(t)
    o.set_clock(1003)
    act, ver, ide, words, ct = o.run_sequential(h, E.EGRESS, E.EP, want_ct=True)
    nat = (words & NATLEN) != 0
    assert list(np.flatnonzero(nat)) == list(at)
    before = E.ct_service_keys(t.ct, 4)
    after = E.ct_service_keys(S.ct_from_rows(o.ct_dump()), 4)
    assert len(after) == len(before) + 1     # one new CT_SERVICE entry, IPv4
