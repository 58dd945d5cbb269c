"""The cases of test_gpu_lookup_edges.py (lookup_edges.py) hold what they
claim — checked on the CPU: the Python restatements of the layout.h hashes
against the host self-test's known answers, every chain, false positive and
directory shape against the Python model of flatten.cpp's placement, and the
oracle against a brute-force longest-prefix match / set membership on every
probe.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import lookup_edges as E
import oracle as O
from cilium_amd import synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hash_restatements_match_layout_h():
    """selftest prints `kat <name> <inputs> <value>` (hex) per layout.h hash"""
    csrc = os.path.join(ROOT, "cilium_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-s", "selftest"], check=True)
    r = subprocess.run([os.path.join(csrc, "build", "selftest"), "kat"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    kats = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("kat ")]
    seen = {}
    for name, *args in kats:
        *ins, want = (int(x, 16) for x in args)
        got = int(E.HASHES[name](*ins))
        assert got == want, f"{name}{tuple(hex(i) for i in ins)}: {got:#x}, layout.h {want:#x}"
        seen.setdefault(name, set()).update(ins)
    assert set(seen) == set(E.HASHES), set(E.HASHES) ^ set(seen)
    for name, ins in seen.items():        # fixed inputs including 0 and 0xFFFFFFFF
        assert 0 in ins and (0xFFFFFFFF in ins or name == "l6_word_mask"), name
    assert len(kats) > 300


def test_last_slot_searches():
    """a hash with its low 16 bits all ones is the last slot of every table
    size up to 65 536; the searches find enough such keys"""
    a = E.last_slot_v4()
    assert len(a) >= 40
    for mask in (7, 511, 1023, 0xFFFF):
        assert (E.hash32(a, mask) == mask).all()
    ids = E.last_slot_policy_ids(int(S.htons(80)), S.IPPROTO_TCP, 0)
    assert len(ids) >= 5 and len(E.last_slot_policy_ids(0, 0, 0)) >= 3
    pre = E.pol_key_pre(ids, int(S.htons(80)) | S.IPPROTO_TCP << 16)
    assert (E.pol_slot(pre, 63) == 63).all()


# ------------------------------------------------------------------ IPv4 LPM
def test_lpm4_structural_shapes_and_reference():
    c = E.lpm4_structural()
    pfx, want = c.claims["prefixes"], c.claims["dir_cases"]
    got = E.l4_dir_cases(pfx)
    assert got == want
    # the intended cases: inline-only with one and two entries, lists of 2..14
    # (padded and not, the longest before the split), chunks
    assert {("inline", 1), ("inline", 2), ("list", 2), ("list", 4), ("list", 12), ("list", 14),
            ("chunk", 15), ("chunk", 16), ("chunk", 40), ("chunk", 300)} <= set(want.values())
    n16 = {}
    for a, l, _ in pfx:
        if l > 16:
            n16[a >> 16] = n16.get(a >> 16, 0) + 1
    assert sorted(n for n in n16.values() if n + 1 < E.L4_LIST_MAX)[-1] == 14   # 14 + 1 < 16
    # padded lists: an odd count behind the inline pair (4 -> 3, 14 -> 13); unpadded: 3, 5, 13
    assert {n for n in n16.values() if 2 < n < 15} >= {3, 4, 5, 13, 14}
    # chunk -> chunk -> leaf: a /24 with at least 15 longer prefixes
    n24 = {}
    for a, l, _ in pfx:
        if l > 24:
            n24[a >> 8] = n24.get(a >> 8, 0) + 1
    assert max(n24.values()) >= 15
    # chunk -> list: a /24 of a split /16 with 1..14 longer prefixes
    assert any(0 < n < 15 and got[d >> 8][0] == "chunk" for d, n in n24.items())
    labels = np.array([p[2] for p in pfx], np.uint64)
    lens = np.array([p[1] for p in pfx])
    assert set(range(33)) == set(lens.tolist())
    for lo in (E.WIDE26, E.WIDE30):
        wide = {(p[0] >> 16) for p in pfx if p[2] >= lo and p[1] > 16}
        kinds = {got[d][0] for d in wide}
        assert {"inline", "list", "chunk"} <= kinds, (lo, kinds)
    assert (labels == 0).sum() >= 3 and (labels == S.HOST_ID).any() and (labels == S.CLUSTER_ID).any()
    # a label 0 with a shorter labelled prefix around it and a longer one inside
    z = E.host4("20.30.16.0")
    lab, hit = E.brute_lpm4(pfx, [z, E.host4("20.30.17.17"), E.host4("20.30.32.0")])
    assert lab.tolist() == [0, 501, 500] and hit.all()
    # the oracle (one hash table per length) equals brute force on every probe
    probes = c.claims["probes"]
    assert len(pfx) >= 460 and len(probes) >= 1400
    for a, l, _ in pfx:
        assert a in probes and (a | (~E.mask4(l) & 0xFFFFFFFF)) in probes
    o = O.Oracle(c.tables)
    lab, hit = o.ipcache_lookup(4, E.raw4(probes))
    bl, bh = E.brute_lpm4(pfx, probes)
    np.testing.assert_array_equal(lab, bl)
    np.testing.assert_array_equal(hit.astype(bool), bh)
    assert len(np.unique(bl)) >= 400


@pytest.mark.parametrize("direction", ["ingress", "egress"])
@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_lpm4_streams(order, direction):
    c = E.lpm4_structural(order, direction)
    h, host = c.headers, c.claims["host"]
    assert 3000 <= len(h) <= 20_000 and len(h) % 64 == 0
    assert set(host.tolist()) == set(c.claims["probes"].tolist())
    waves = (host >> 16).reshape(-1, 64)
    uniform = (waves == waves[:, :1]).all(1)
    assert uniform.all() if order == "grouped" else uniform.mean() < 0.05
    probe = h.saddr if direction == "ingress" else h.daddr
    np.testing.assert_array_equal(probe, E.raw4(host))
    # the header's identity is the probe's label wherever the datapath takes it
    _, ver, ide = O.Oracle(c.tables).classify(h, c.mode, c.ep_lxc)
    lab, _ = E.brute_lpm4(c.claims["prefixes"], host)
    keep = ~np.isin(lab, [0, S.HOST_ID, S.CLUSTER_ID]) if direction == "ingress" else lab != 0
    np.testing.assert_array_equal(ide[keep], lab[keep])
    assert len(np.unique(ver)) >= 3


# ------------------------------------------------------------------ IPv6 LPM
@pytest.mark.parametrize("variant", ["full", "short", "long"])
def test_lpm6_structural(variant):
    c = E.lpm6_structural(variant)
    pfx, probes, m = c.claims["prefixes"], c.claims["probes"], c.claims["model"]
    lens = {p[1] for p in pfx}
    assert m["groups"] >= 2
    assert len(m["lens"]) == len(lens - {0})
    if variant == "full":
        assert lens == set(range(129)) and m["def_label"] == 4000
        assert any(p[2] == 0 and p[1] == 77 for p in pfx)
        assert {32, 33, 64, 65, 96, 97, 127, 128} <= lens
    elif variant == "short":
        assert max(lens) <= 64 and m["slots"] is None and m["def_label"] == 0 and 0 not in lens
        assert {31, 32, 33, 63, 64} <= lens
    else:
        assert min(lens - {0}) > 64 and m["slots64"] is None and m["def_label"] == 77
        assert {65, 95, 96, 97, 127, 128} <= lens
    # a group boundary inside a pile: consecutive lengths in different groups
    firsts = [e & 255 for e in m["lens"] if e & E.L6_GROUP_FIRST]
    assert len(firsts) == m["groups"]
    # chains of 5 keys homed at the last slot of each array, wrapping to slot 0
    for tab, plen in ((m["slots64"], 64), (m["slots"], 128)):
        if tab is None:
            continue
        last = len(tab) - 1
        chain = [(a, l) for a, l, _ in pfx
                 if l == plen and int(E.l6_hash(*E.words_of(a), l)) & 0xFFFF == 0xFFFF]
        assert len(chain) >= 4
        at = sorted(m["where"][k] for k in chain)
        assert at[0] < 8 and at[-1] == last, at          # crosses the table's end
        assert all(tab[s] is not None for s in range(at[0] + 1)), "chain broken"
    # four boundary probes per prefix
    for a, l, _ in pfx:
        if l:
            assert a in probes and (a | ((1 << (128 - l)) - 1)) in probes
    # the model of the device lookup, the oracle and brute force agree
    bl, bh = E.brute_lpm6(pfx, probes)
    ml = np.array([E.lpm6_model_lookup(m, x) for x in probes], np.uint32)
    np.testing.assert_array_equal(ml, bl)
    lab, hit = O.Oracle(c.tables).ipcache_lookup(6, np.stack([E.bytes6(x) for x in probes]))
    np.testing.assert_array_equal(np.where(hit, lab, 0), bl)
    np.testing.assert_array_equal(hit.astype(bool), bh)
    assert 2000 <= len(c.headers) <= 20_000


def test_lpm6_confusion_depends_on_the_length_compare():
    c = E.lpm6_confusion()
    m, x, pfx = c.claims["model"], c.claims["x"], c.claims["prefixes"]
    assert m["slots64"] is not None and len(m["slots64"]) == 16 and m["groups"] == 1
    h48 = int(E.l6_hash(*E.words_of(x), 48))
    b = int(E.l6_bloom_bits(h48))
    word = int(m["bloom"][int(E.l6_group_hash(E.words_of(x), 40)) & 63])
    assert (x, 48) not in m["where"] and (word & b) == b            # absent, "maybe"
    assert m["where"][(x, 40)] == h48 & 15                          # lands on X/40
    assert E.lpm6_model_lookup(m, x) == 6044
    assert E.lpm6_model_lookup(m, x, check_len=False) == 6040
    bl, _ = E.brute_lpm6(pfx, c.claims["probes"])
    lab, hit = O.Oracle(c.tables).ipcache_lookup(6, np.stack([E.bytes6(a) for a in c.claims["probes"]]))
    np.testing.assert_array_equal(np.where(hit, lab, 0), bl)
    assert bl[c.claims["probes"].index(x)] == 6044
    # and the header's identity shows it
    _, _, ide = O.Oracle(c.tables).classify(c.headers, 0, 0)
    k = np.flatnonzero((c.headers.saddr == E.bytes6(x)).all(1))
    assert len(k) and (ide[k] == 6044).all()


# ----------------------------------------------------------------- endpoints
@pytest.mark.parametrize("family", [4, 6])
def test_endpoints_many(family):
    big, twin = E.endpoints_many(family), E.endpoints_many(family, twin=True)
    limit = E.LXC_LDS_MAX_SLOTS if family == 4 else E.LXC6_LDS_MAX_SLOTS
    n = 130 if family == 4 else 66
    assert big.claims["n"] == n and big.claims["slots"] == 2 * limit and not big.claims["in_lds"]
    assert E.pow2_at_least(4 * (n - 2)) == limit       # one pair fewer would still fit
    assert twin.claims["slots"] <= limit and twin.claims["in_lds"]
    for c in (big, twin):
        cl = c.claims
        slots, where = (E.lxc4_model if family == 4 else E.lxc6_model)(c.tables.endpoints)
        assert len(slots) == cl["slots"]
        last = len(slots) - 1
        at = sorted(cl["chain_slots"])
        assert len(at) == 5 and at[-1] == last and at[0] <= 1 and at[-2] <= 8   # wraps
        assert all(slots[s] is not None for s in range(at[-2] + 1))             # unbroken
        assert 0 <= cl["chain_slots"][cl["sender"]] < 8                         # past the wrap
        # the absent addresses are homed at the last slot and are no endpoints
        for a in cl["absent"]:
            if family == 4:
                assert int(E.hash32(a, last)) == last and int(a) not in where
            else:
                assert int(E.l6_hash(*E.raw_words6(a), E.L6_LXC_TAG)) & last == last
                assert bytes(a) not in where
        # traffic reaches every endpoint and every absent address
        d = c.headers.daddr
        got = set(d.tolist()) if family == 4 else set(bytes(x) for x in d)
        want = list(cl["chain"]) + list(cl["absent"])
        assert all((int(a) if family == 4 else bytes(a)) in got for a in want)
        assert len(got) == cl["n"] + 3
        # each endpoint answers with its own proxy port: a wrong slot shows
        _, ver, _ = O.Oracle(c.tables).classify(c.headers, 0, 0)
        assert len(np.unique(ver[ver > 0])) == cl["n"]
        e = E.endpoints_many(family, c is twin, "egress")
        assert e.ep_lxc == E.EP0 + cl["sender"] and e.mode == 1
        _, ver, _ = O.Oracle(e.tables).classify(e.headers, 1, e.ep_lxc)
        assert (ver == 0).sum() > 50 and (ver == -132).sum() > 50       # valid and invalid sources
        assert len(np.unique(ver)) >= 3


# -------------------------------------------------------------------- policy
def test_policy_chains():
    c = E.policy_chains()
    cl = c.claims
    model, bloom = cl["model"]
    a, b, cc = sorted(model)
    assert model[a]["base"] == 0 and model[b]["base"] == model[a]["mask"] + 1
    assert model[cc]["base"] == model[b]["base"] + model[b]["mask"] + 1    # b is not the last
    hi4 = int(S.htons(80)) | S.IPPROTO_TCP << 16
    keys = [(i, hi4) for i in cl["present4"]] + [(i, 0) for i in cl["present3"]]
    for lxc in (b, cc):
        m = model[lxc]
        assert all(m["home"][k] == m["mask"] for k in keys)
        assert sorted(m["where"][k] for k in keys) == [0, 1, 2, 3, m["mask"]]
    # the same keys, other proxy ports in the next table
    for k in keys[:3]:
        pb = model[b]["slots"][model[b]["where"][k]][2]
        pc = model[cc]["slots"][model[cc]["where"][k]][2]
        assert pb != pc and pb and pc
    # the absent keys are homed there too and walk the whole chain
    for k in [(i, hi4) for i in cl["absent4"]] + [(i, 0) for i in cl["absent3"]]:
        seen, hit = E.pol_walk(model, b, *k)
        assert not hit and seen[:5] == [model[b]["mask"], 0, 1, 2, 3]
    # headers whose verdict is the proxy port stored at a wrapped slot of b
    _, ver, ide = O.Oracle(c.tables).classify(c.headers, 0, 0)
    idx = cl["index"]
    wrapped = 0
    for i in cl["present4"]:
        s = model[b]["where"][(i, hi4)]
        sel = (cl["ident"][idx] == i) & (cl["ep"][idx] == 1) & (cl["dport"][idx] == 80)
        assert sel.sum() >= 64 and (ide[sel] == i).all()
        assert (ver[sel] == model[b]["slots"][s][2]).all()
        wrapped += s < 4
    assert wrapped >= 2
    sel = np.isin(cl["ident"][idx], cl["absent4"] + cl["absent3"])
    assert (ver[sel] == E.DROP_POLICY).all()
    sel = np.isin(cl["ident"][idx], cl["present3"]) & (cl["ep"][idx] > 0)
    assert (ver[sel] == 0).all()


@pytest.mark.parametrize("direction", ["ingress", "egress"])
def test_policy_fallback(direction):
    """the winner of every subset, by the reference's order: L4, L3,
    wildcard port; a fragment on ingress sees the L3 key only"""
    for sender in range(8) if direction == "egress" else [0]:
        c = E.policy_fallback(direction, False, sender)
        cl = c.claims
        _, ver, _ = O.Oracle(c.tables).classify(c.headers, c.mode, c.ep_lxc)
        idx = cl["index"]
        eg = int(direction == "egress")
        for j in range(len(ver)):
            k = idx[j]
            e = int(cl["subset"][k]) if direction == "ingress" else sender
            frag = bool(cl["frag"][k]) and not eg
            mine, p80 = cl["ident"][k] == E.FB_ID, cl["dport"][k] == 80
            if e & 1 and mine and p80 and not frag:
                want = int(S.htons(11000 + e + 500 * eg))
            elif e & 2 and mine:
                want = 0
            elif e & 4 and p80 and not frag:
                want = int(S.htons(12000 + e + 500 * eg))
            else:
                want = E.DROP_POLICY
            assert ver[j] == want, (j, e, frag, mine, p80, ver[j], want)
    model, bloom = E.policy_fallback(direction, True).claims["model"]
    assert bloom is None and all(all(s is None for s in m["slots"]) for m in model.values())
    model, bloom = E.policy_fallback(direction).claims["model"]
    assert bloom is not None and all(s is None for s in model[E.EP0]["slots"])   # the empty map
    c = E.policy_fallback(direction, True)
    _, ver, _ = O.Oracle(c.tables).classify(c.headers, c.mode, c.ep_lxc)
    assert (ver == E.DROP_POLICY).all()


def test_policy_bloom_false_positives():
    c = E.policy_bloom_fp()
    cl = c.claims
    model, bloom = cl["model"]
    hi = cl["hi"]
    m = model[E.EP0]
    assert len(bloom) == 256 and m["mask"] == 1023
    for i in (cl["id_a"], cl["id_b"], cl["id_c"]):
        assert (i, hi) not in m["where"] and E.pol_maybe(model, bloom, E.EP0, i, hi)
    assert (cl["id_a"], 0) in m["where"]                       # (a) its L3 key is there
    for i in (cl["id_b"], cl["id_c"]):                         # (b), (c) nothing after
        assert (i, 0) not in m["where"] and (0, hi) not in m["where"]
    seen, hit = E.pol_walk(model, E.EP0, cl["id_b"], hi)
    assert not hit and len(seen) == 1                          # (b) home slot free
    seen, hit = E.pol_walk(model, E.EP0, cl["id_c"], hi)
    assert not hit and len(seen) >= 2                          # (c) walks past another key
    _, ver, ide = O.Oracle(c.tables).classify(c.headers, 0, 0)
    p80 = cl["dport"] == 80
    assert (ver[(cl["ident"] == cl["id_a"])] == 0).all()
    assert (ver[np.isin(cl["ident"], [cl["id_b"], cl["id_c"]])] == E.DROP_POLICY).all()
    assert (ver[(cl["ident"] == 1000) & p80] > 0).all() and (ver[cl["ident"] == 1001] == 0).all()
    np.testing.assert_array_equal(ide, cl["ident"])


# ----------------------------------------------------------------- prefilter
@pytest.mark.parametrize("variant", ["spill1", "spill2", "zero", "dyn"])
def test_prefilter_v4(variant):
    c = E.prefilter_edges(4, variant, 2)
    cl = c.claims
    m = cl["model"]
    src = c.headers.saddr
    assert 0 in src and 2000 <= len(src) <= 20_000
    if variant in ("spill1", "spill2"):
        nb = len(m["buckets"])
        n = len(cl["chain"])
        assert n == (5 if variant == "spill1" else 9)
        assert all(int(E.hash32(a, nb - 1)) == nb - 1 for a in cl["chain"])
        spill = sorted(set(m["where"][a] for a in cl["chain"]))
        assert spill == [nb - 1] + list(range((n - 1) // 4)) or \
            spill == list(range((n - 1) // 4)) + [nb - 1]
        assert len(m["buckets"][nb - 1]) == 4
        fp = cl["fp"]
        assert fp not in m["where"] and E.pf_maybe(m, fp) and int(E.hash32(fp, nb - 1)) == nb - 1
        assert fp in src and all(a in src for a in cl["chain"])
    assert m["zero"] == (variant in ("spill2", "zero"))
    if variant == "zero":
        assert m["buckets"] is None and len(c.tables.prefilter) == 1
    if variant == "dyn":
        assert m["buckets"] is None and not m["zero"]
    dyn = c.tables.prefilter[c.tables.prefilter["dyn"] == 1]
    if variant in ("spill2", "dyn"):
        assert set(dyn["plen"].tolist()) >= set(range(2, 33))
        assert variant == "dyn" or 1 in dyn["plen"]
    else:
        assert len(dyn) == 0
    deny = E.brute_deny4(c.tables.prefilter, src)
    assert deny.any() and not deny.all()
    for mode in (2, 3):
        cc = E.prefilter_edges(4, variant, mode)
        assert cc.headers is c.headers and cc.mode == mode
        _, ver, _ = O.Oracle(cc.tables).classify(cc.headers, mode, 0)
        np.testing.assert_array_equal(ver == E.DROP_PREFILTER, deny)
    assert deny[src == 0].all() == m["zero"]


@pytest.mark.parametrize("variant", ["spill", "dyn"])
def test_prefilter_v6(variant):
    c = E.prefilter_edges(6, variant, 2)
    cl = c.claims
    m = cl["model"]
    src = [int.from_bytes(bytes(a), "big") for a in c.headers.saddr]
    assert 0 in src and (0, 128) in m["where"]              # ::/128 and a source ::
    if variant == "spill":
        last = len(m["slots"]) - 1
        at = sorted(m["where"][(a, 128)] for a in cl["chain"])
        assert len(at) == 5 and at[-1] == last and at[-2] <= 8              # wraps
        assert all(m["slots"][s] is not None for s in range(at[-2] + 1))    # unbroken
        fp = cl["fp"]
        assert (fp, 128) not in m["where"] and fp in src
        h = int(E.pf6_bloom_hash(*E.words_of(fp)))
        b = int(E.bloom_bits(h))
        assert (int(cl["bloom"][h & (len(cl["bloom"]) - 1)]) & b) == b
        assert int(E.l6_hash(*E.words_of(fp), 128)) & last == last
    else:
        dyn = c.tables.prefilter[c.tables.prefilter["dyn"] == 1]
        assert set(dyn["plen"].tolist()) == set(range(1, 129))
    deny = E.brute_deny6(c.tables.prefilter, src)
    assert deny.any() and not deny.all() and deny[np.array(src) == 0].all()
    for mode in (2, 3):
        _, ver, _ = O.Oracle(c.tables).classify(c.headers, mode, 0)
        np.testing.assert_array_equal(ver == E.DROP_PREFILTER, deny)
