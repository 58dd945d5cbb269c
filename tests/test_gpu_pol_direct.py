"""The policy lookup under both placements of the policy keys (forced through
CFC_OPT_POL_PLACEMENT: linear probing, and the direct hash-and-displace
placement of layout.h pol_slot_direct): kern_common.hpp policy_issue /
policy_resolve against the oracle on action, verdict, identity, policy-entry
counters, metrics and per-identity counters.  The cases of pol_direct.py (the
smallest tables, a shared home slot, a Bloom word shared by two tables,
absent L4 keys whose one probe hits another key, two keys with equal pre, a
proxy port patched in place, the egress second stage, an IPv6 batch) and the
policy cases of lookup_edges.py.  Run on an MI355X: pytest -m gpu."""
import errno

import numpy as np
import pytest

import lookup_edges as E
import oracle as O
import pol_direct as PD
from cilium_amd import _lib as L
from cilium_amd import metricsmap
from cilium_amd import policymap
from cilium_amd import synth as S
from cilium_amd.datapath import Datapath, pack
from cilium_amd.loader import load_tables, policy_rows

pytestmark = pytest.mark.gpu
LINEAR, DIRECT, AUTO = L.POL_PLACEMENT_LINEAR, L.POL_PLACEMENT_DIRECT, L.POL_PLACEMENT_AUTO
BOTH = pytest.mark.parametrize("placement", [LINEAR, DIRECT], ids=["linear", "direct"])


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


def classify_all(torch, dp, o, cases):
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
    return outs


def counters_match(dp, o, pms):
    dp.counters_sync()
    for lxc, pm in pms.items():
        np.testing.assert_array_equal(np.array(policy_rows(pm), np.uint64).reshape(-1, 7),
                                      o.policy_counters(lxc))
    np.testing.assert_array_equal(
        np.array(metricsmap.dump_rows(dp), np.uint64).reshape(-1, 4), o.metrics())
    np.testing.assert_array_equal(dp.identity_counters(), o.identity_counters())


def check(torch, cases, placement, took=None, max_d=None):
    """The cases (one table set) on a context with the placement forced (or
    auto) -> [(action, verdict, identity)]; took: the placement the epoch
    must report (default: the forced one)"""
    t = cases[0].tables
    assert all(c.tables is t for c in cases)
    dp = Datapath(0)
    try:
        dp.set_option(L.OPT_POL_PLACEMENT, placement)
        pms = load_tables(dp, t)
        p, d = dp.pol_placement()
        assert p == (placement if took is None else took)
        assert d == 0 or p == DIRECT
        if max_d is not None and p == DIRECT:
            assert d == max_d
        o = O.Oracle(t)
        outs = classify_all(torch, dp, o, cases)
        counters_match(dp, o, pms)
        return outs
    finally:
        dp.close()


# ------------------------------------------------------------ pol_direct.py
@BOTH
@pytest.mark.parametrize("nkeys", [2, 3])
def test_smallest_tables(torch, nkeys, placement):
    """An 8-slot table with two keys and a 16-slot table with three (four
    slots per key leave three keys no 8-slot table), all of one Bloom word,
    a displaced slot wrapping past the last one; absent keys of that word."""
    c = PD.smallest(nkeys)
    cl = c.claims
    (act, ver, _), = check(torch, [c], placement, max_d=cl["d"])
    g = cl["grid"]
    for k, i in enumerate(cl["keys"]):
        sel = (g[:, 0] == k) & (g[:, 2] == 0)
        assert sel.any() and (ver[sel] == int(S.htons(11000 + k))).all()
    assert (ver[g[:, 0] >= nkeys] == E.DROP_POLICY).all()
    assert (ver[g[:, 2] == 1] == E.DROP_POLICY).all()


@BOTH
def test_shared_home_slot(torch, placement):
    """Two keys of one bucket with one home slot, ingress (with fragments)
    and the egress batch of the second endpoint, whose local delivery looks
    the sender's SECLABEL up in the first endpoint's table."""
    ci, ce = PD.shared_home("ingress"), PD.shared_home("egress")
    cl = ci.claims
    assert ce.tables is ci.tables
    outs = check(torch, [ci, ce], placement, max_d=cl["dm"]["max_d"])
    ver, g = outs[0][1], cl["grid"]
    for k, port in ((0, 11001), (1, 11002)):
        sel = (g[:, 0] == k) & (g[:, 1] == 0) & (g[:, 2] == 0) & (g[:, 4] == 0)
        assert sel.any() and (ver[sel] == int(S.htons(port))).all()
    # the egress second stage: the destination endpoint's key of the SECLABEL
    ge = ce.claims["grid"]
    sel = (ge[:, 0] == 0) & (ge[:, 1] == 0)
    assert sel.any() and (outs[1][1][sel] == int(S.htons(12001))).all()
    assert len(np.unique(outs[1][1])) >= 3


@BOTH
def test_shared_bucket_across_tables(torch, placement):
    """An 8-slot and a 64-slot table whose keys share a Bloom word and so
    its displacement: each endpoint answers with its own proxy ports."""
    c = PD.shared_bucket()
    cl = c.claims
    (_, ver, _), = check(torch, [c], placement, max_d=cl["dm"]["max_d"])
    g = cl["grid"]
    for ep, ports in ((0, (11001, 11002, None)), (1, (21001, 21002, 21003))):
        for k, port in enumerate(ports):
            sel = (g[:, 0] == k) & (g[:, 1] == ep) & (g[:, 2] == 0)
            want = E.DROP_POLICY if port is None else int(S.htons(port))
            assert sel.any() and (ver[sel] == want).all(), (ep, k)


@BOTH
def test_absent_l4_key(torch, placement):
    """Absent L4 keys the filter passes, their one probe on another key:
    the L3 key behind it, the wildcard key behind it, nothing behind it
    (DROP_POLICY); as fragments too."""
    c = PD.absent_l4()
    cl = c.claims
    (_, ver, _), = check(torch, [c], placement, max_d=cl["dm"]["max_d"])
    sel = lambda i, p, f: (cl["ident"] == i) & (cl["dport"] == p) & (cl["frag"] == f)
    assert (ver[sel(cl["id_a"], 80, False)] == 0).all()
    assert (ver[sel(cl["id_w"], 8080, False)] == int(S.htons(16000))).all()
    assert (ver[sel(cl["id_w"], 8080, True)] == E.DROP_POLICY).all()
    assert (ver[sel(cl["id_n"], 80, False)] == E.DROP_POLICY).all()
    assert (ver[sel(cl["id_n"], 80, True)] == E.DROP_POLICY).all()


def test_equal_pre_keeps_linear(torch):
    """Two keys with equal pre: auto takes linear probing and answers both;
    forced direct fails the commit."""
    c = PD.equal_pre()
    for placement in (AUTO, LINEAR):
        (_, ver, _), = check(torch, [c], placement, took=LINEAR)
        assert {int(S.htons(11001)), int(S.htons(11002))} <= set(np.unique(ver).tolist())
    dp = Datapath(0)
    try:
        dp.set_option(L.OPT_POL_PLACEMENT, DIRECT)
        with pytest.raises(OSError) as e:
            load_tables(dp, c.tables)
        assert e.value.errno == errno.ENOSPC
        # the option back to auto: the same maps commit
        dp.set_option(L.OPT_POL_PLACEMENT, AUTO)
        dp.commit()
        assert dp.pol_placement() == (LINEAR, 0)
        classify_all(torch, dp, O.Oracle(c.tables), [c])
    finally:
        dp.close()


@BOTH
def test_proxy_port_patch(torch, placement):
    """The proxy port of a key with a nonzero displacement overwritten, then
    a commit: patched in place (the epoch number stays), the new port is the
    verdict."""
    c = PD.shared_home("ingress")
    cl = c.claims
    a = cl["a"]
    dp = Datapath(0)
    try:
        dp.set_option(L.OPT_POL_PLACEMENT, placement)
        pms = load_tables(dp, c.tables)
        assert dp.pol_placement()[0] == placement
        epoch = dp.stats()["epoch"]
        key = policymap.PolicyKey(a, int(S.htons(80)), PD.TCP, 0)
        dp.update_element(pms[E.EP0].Fd, key.pack(),
                          policymap.PolicyEntry(int(S.htons(31001))).pack())
        dp.commit()
        assert dp.stats()["epoch"] == epoch
        pol = dict(c.tables.policy)
        rows = pol[E.EP0].copy()
        k, = np.flatnonzero((rows["identity"] == a) & (rows["dport"] == int(S.htons(80))))
        rows["proxy_port"][k] = int(S.htons(31001))
        pol[E.EP0] = rows
        t2 = S.Tables(c.tables.ipcache, c.tables.endpoints, pol, c.tables.prefilter,
                      c.tables.seclabel)
        o = O.Oracle(t2)
        (_, ver, _), = classify_all(torch, dp, o, [E.Case(t2, c.headers, 0, 0, {})])
        g = cl["grid"]
        sel = (g[:, 0] == 0) & (g[:, 1] == 0) & (g[:, 2] == 0) & (g[:, 4] == 0)
        assert sel.any() and (ver[sel] == int(S.htons(31001))).all()
        counters_match(dp, o, pms)
    finally:
        dp.close()


@BOTH
def test_ipv6_batch(torch, placement):
    """classify6.hip shares the lookup: an IPv6 endpoint with the shared-home
    table, its identities behind /128s."""
    cl = PD.shared_home("ingress").claims
    idents = cl["idents"]
    base = int.from_bytes(bytes(S.ip6("2001:db8:9::")), "big")
    pfx = [(base + k + 1, 128, int(v)) for k, v in enumerate(idents)]
    eps = np.concatenate([S.endpoint_v6(S.LXC_IPV6, 100, E.EP0)])
    pol = {E.EP0: PD.shared_home("ingress").tables.policy[E.EP0]}
    t = S.Tables(E.ipc6(pfx), eps, pol, np.zeros(0, S.PREFILTER_DT), {E.EP0: S.EP_SECLABEL})
    n = 2048 + 37
    k = np.arange(n)
    src = np.stack([E.bytes6(p[0]) for p in pfx])
    h = E.hdr6(src[k % len(pfx)], S.LXC_IPV6, np.array([80, 81])[(k // len(pfx)) % 2])
    (_, ver, _), = check(torch, [E.Case(t, h, 0, 0, {})], placement)
    for i, port in ((0, 11001), (1, 11002)):
        sel = (k % len(pfx) == i) & ((k // len(pfx)) % 2 == 0)
        assert (ver[sel] == int(S.htons(port))).all()


# ----------------------------------------------- lookup_edges.py's policy cases
@BOTH
def test_policy_chains(torch, placement):
    c = E.policy_chains()
    (_, ver, _), = check(torch, [c], placement)
    cl = c.claims
    sel = np.isin(cl["ident"][cl["index"]], cl["absent4"] + cl["absent3"])
    assert (ver[sel] == E.DROP_POLICY).all()


@BOTH
def test_policy_fallback(torch, placement):
    cases = [E.policy_fallback("ingress")] + [E.policy_fallback("egress", False, s)
                                              for s in range(8)]
    outs = check(torch, cases, placement)
    assert len(np.unique(outs[0][1])) == 10


@BOTH
def test_policy_bloom_false_positives(torch, placement):
    c = E.policy_bloom_fp()
    (_, ver, _), = check(torch, [c], placement)
    cl = c.claims
    assert (ver[cl["ident"] == cl["id_a"]] == 0).all()
    assert (ver[np.isin(cl["ident"], [cl["id_b"], cl["id_c"]])] == E.DROP_POLICY).all()
