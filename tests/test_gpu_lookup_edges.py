"""The device table lookups at their structural edges (csrc kern_common.hpp
l4_lookup / lxc_resolve / pf_resolve / policy_issue / policy_resolve_walk,
classify.hip's DIR-24-8 probe, classify6.hip lpm6_lookup / lxc6_find): every
shape of the compact IPv4 LPM's /16 directory and both layouts at every
prefix's boundary addresses, IPv6 prefixes at the word and Bloom-group
boundaries, endpoint tables outside LDS, probe chains that wrap from a
table's last slot to slot 0, policy fallback behind Bloom false positives, the
prefilter's corner shapes.  Action, verdict and identity per header, policy
counters, metrics and identity counters against the oracle, bit-exact.  The
cases are lookup_edges.py's (preconditions: test_lookup_edges.py).
Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import lookup_edges as E
import oracle as O
from cilium_amd import _lib as L
from cilium_amd import metricsmap
from cilium_amd import synth as S
from cilium_amd.datapath import Datapath, pack
from cilium_amd.loader import load_tables, policy_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


def check(torch, cases, lpm4=L.LPM4_AUTO):
    """The cases (one table set) in turn on one Datapath and one Oracle:
    outputs per case, counters at the end -> ([(action, verdict, identity)],
    the stats)"""
    t = cases[0].tables
    assert all(c.tables is t for c in cases)
    dp = Datapath(0)
    try:
        dp.set_option(L.OPT_LPM4, lpm4)
        pms = load_tables(dp, t)
        st = dp.stats()
        o = O.Oracle(t)
        outs = []
        for k, c in enumerate(cases):
            assert 0 < len(c.headers) <= 20_000
            out = dp.classify(pack(c.headers), c.mode, c.ep_lxc)
            torch.cuda.synchronize()
            got = (out.action.cpu().numpy().astype(np.int32), out.verdict.cpu().numpy(),
                   out.identity.cpu().numpy().view(np.uint32))
            want = o.classify(c.headers, c.mode, c.ep_lxc, nthreads=8)
            for name, a, b in zip(("action", "verdict", "identity"), got, want):
                bad = np.flatnonzero(a != b)
                assert len(bad) == 0, f"case {k} {name}: {len(bad)} differ, first {bad[:6]} " \
                                      f"{a[bad[:6]]} vs {b[bad[:6]]}"
            outs.append(got)
        dp.counters_sync()
        for lxc, pm in pms.items():
            np.testing.assert_array_equal(np.array(policy_rows(pm), np.uint64).reshape(-1, 7),
                                          o.policy_counters(lxc))
        np.testing.assert_array_equal(
            np.array(metricsmap.dump_rows(dp), np.uint64).reshape(-1, 4), o.metrics())
        np.testing.assert_array_equal(dp.identity_counters(), o.identity_counters())
        return outs, st
    finally:
        dp.close()


# ------------------------------------------------------------------ IPv4 LPM
@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("layout", ["trie", "dir24_8"])
def test_lpm4_structural(torch, layout, order):
    """Inline-only /16s, lists of every padded length up to the longest
    before the split, chunk -> list, chunk -> chunk -> leaf, labels through
    lbl_ovf in every position, label 0 over a shorter prefix: first and last
    address of each prefix and their neighbours, as ingress sources and as
    egress destinations."""
    want = L.LPM4_TRIE if layout == "trie" else L.LPM4_DIR24_8
    cases = [E.lpm4_structural(order, "ingress"), E.lpm4_structural(order, "egress")]
    outs, st = check(torch, cases, lpm4=want)
    assert st["lpm4_layout"] == want
    assert st["ipcache_v4_prefixes"] == len(cases[0].claims["prefixes"])
    # the identity is the probe's longest prefix's label
    lab, _ = E.brute_lpm4(cases[0].claims["prefixes"], cases[0].claims["host"])
    keep = ~np.isin(lab, [0, S.HOST_ID, S.CLUSTER_ID])
    np.testing.assert_array_equal(outs[0][2][keep], lab[keep])
    np.testing.assert_array_equal(outs[1][2][lab != 0], lab[lab != 0])


# ------------------------------------------------------------------ IPv6 LPM
@pytest.mark.parametrize("variant", ["full", "short", "long"])
def test_lpm6_structural(torch, variant):
    """Every length /0-/128 (full), slots64 alone without ::/0 (short),
    slots alone (long); chains of five keys wrapping at the end of each slot
    array; piles that split the Bloom groups."""
    c = E.lpm6_structural(variant)
    outs, st = check(torch, [c, E.Case(c.tables, c.headers, 3, 0, c.claims)])
    m = c.claims["model"]
    assert st["lpm6_groups"] == m["groups"] >= 2
    assert st["lpm6_lengths"] == len(m["lens"])
    lab, _ = E.brute_lpm6(c.claims["prefixes"], c.claims["probes"])
    lab = lab[np.arange(len(c.headers)) % len(lab)]
    keep = ~np.isin(lab, [0, S.HOST_ID, S.CLUSTER_ID])
    np.testing.assert_array_equal(outs[0][2][keep], lab[keep])


def test_lpm6_length_compare(torch):
    """The slots64 probe of length 48 lands on a slot holding the same words
    at length 40: the answer is the /44's label."""
    c = E.lpm6_confusion()
    outs, st = check(torch, [c])
    assert st["lpm6_groups"] == 1 and st["lpm6_lengths"] == 3
    k = np.flatnonzero((c.headers.saddr == E.bytes6(c.claims["x"])).all(1))
    assert len(k) and (outs[0][2][k] == 6044).all()


# ----------------------------------------------------------------- endpoints
@pytest.mark.parametrize("twin", [False, True], ids=["global", "lds"])
@pytest.mark.parametrize("family", [4, 6])
def test_endpoints_many(torch, family, twin):
    """130 IPv4 / 66 IPv6 endpoints: the table stays in global memory (the
    non-FAST instance of k_classify_v4); five endpoints in a chain across the
    table's end, absent addresses homed into it; egress from an endpoint
    past the wrap.  The twin has the same chain in LDS."""
    cases = [E.endpoints_many(family, twin, "ingress"), E.endpoints_many(family, twin, "egress")]
    cl = cases[0].claims
    assert cl["in_lds"] == twin
    outs, st = check(torch, cases)
    assert st["endpoints" if family == 4 else "endpoints_v6"] == cl["n"]
    # every endpoint answered with its own proxy port
    ver = outs[0][1]
    assert len(np.unique(ver[ver > 0])) == cl["n"]
    d = cases[0].headers.daddr
    for i, a in enumerate(cl["chain"]):
        sel = (d == a) if family == 4 else (d == a).all(1)
        p = np.unique(ver[sel & (ver > 0)])
        assert p.tolist() == [int(S.htons(10000 + i))], (i, p)
    assert (outs[1][1] == 0).sum() > 50


# -------------------------------------------------------------------- policy
def test_policy_chains(torch):
    """Five keys homed at the last slot of the middle endpoint's table: the
    verdicts are the proxy ports stored at its slots 0-3 (the next table
    holds the same keys with others), absent keys walk the chain and drop."""
    c = E.policy_chains()
    outs, st = check(torch, [c])
    cl = c.claims
    model, _ = cl["model"]
    b, nxt = sorted(model)[1:]
    hi4 = int(S.htons(80)) | S.IPPROTO_TCP << 16
    idx, ver = cl["index"], outs[0][1]
    for i in cl["present4"]:
        sel = (cl["ident"][idx] == i) & (cl["ep"][idx] == 1) & (cl["dport"][idx] == 80)
        own = model[b]["slots"][model[b]["where"][(i, hi4)]][2]
        other = model[nxt]["slots"][model[nxt]["where"][(i, hi4)]][2]
        assert own != other and (ver[sel] == own).all()
    sel = np.isin(cl["ident"][idx], cl["absent4"] + cl["absent3"])
    assert (ver[sel] == E.DROP_POLICY).all()


@pytest.mark.parametrize("empty", [False, True], ids=["keys", "no_bloom"])
def test_policy_fallback(torch, empty):
    """Every subset of {L4, L3, wildcard port} for one identity and port,
    with and without the fragment flag, ingress and egress from every
    endpoint; then the same with no key at all (no policy Bloom filter)."""
    cases = [E.policy_fallback("ingress", empty)] + \
            [E.policy_fallback("egress", empty, s) for s in range(8)]
    outs, st = check(torch, cases)
    ver = outs[0][1]
    if empty:
        assert all((o[1] == E.DROP_POLICY).all() for o in outs)
    else:
        assert len(np.unique(ver)) == 10        # 4 L4 + 4 wildcard proxy ports, pass, drop
        assert sum(len(np.unique(o[1])) for o in outs[1:]) >= 16


def test_policy_bloom_false_positives(torch):
    """Absent L4 keys the filter passes: (a) falls through to its L3 key,
    (b) to nothing, (c) walks past the key in its home slot first."""
    c = E.policy_bloom_fp()
    outs, st = check(torch, [c])
    cl, ver = c.claims, outs[0][1]
    assert (ver[cl["ident"] == cl["id_a"]] == 0).all()
    assert (ver[np.isin(cl["ident"], [cl["id_b"], cl["id_c"]])] == E.DROP_POLICY).all()


# ----------------------------------------------------------------- prefilter
@pytest.mark.parametrize("family,variant", [(4, "spill1"), (4, "spill2"), (4, "zero"), (4, "dyn"),
                                            (6, "spill"), (6, "dyn")])
def test_prefilter_edges(torch, family, variant):
    """Exact addresses spilling from the last bucket into the first (one and
    two spills), an absent address the filter passes, {0.0.0.0/32} alone
    (pf_fix null, pf_fix_zero set) and beside others, a source of 0, dynamic
    prefixes of every length at their boundaries; the IPv6 twins.  XDP and
    FULL."""
    cases = [E.prefilter_edges(family, variant, 2), E.prefilter_edges(family, variant, 3)]
    outs, st = check(torch, cases)
    pf = cases[0].tables.prefilter
    fam = "v4" if family == 4 else "v6"
    assert st[f"prefilter_{fam}_fix"] == int((pf["dyn"] == 0).sum())
    assert st[f"prefilter_{fam}_dyn"] == int((pf["dyn"] == 1).sum())
    src = cases[0].headers.saddr
    if family == 4:
        deny = E.brute_deny4(pf, src)
    else:
        deny = E.brute_deny6(pf, [int.from_bytes(bytes(a), "big") for a in src])
    for o in outs:
        np.testing.assert_array_equal(o[1] == E.DROP_PREFILTER, deny)
