"""The compact IPv4 LPM at every directory width (layout.h l4d, dir_bits 16,
17 or 18, forced through CFC_OPT_LPM4_DIR_BITS): kern_common.hpp l4_lookup and
classify.hip r2_issue against the oracle on action, verdict and identity, and
against the same stream at /16.  The structural streams of lookup_edges.py,
a table for the edges a wider directory adds (the painting of /D-1 and /D
prefixes, a len - D = 1 inline entry, the list limits of a /D node, a split
node whose second chunk is the narrow last one, wide labels in every place,
directory indices of all ones and zeros, a partial last wave), and two
commits on one context under auto.  Run on an MI355X: pytest -m gpu."""
import functools
import struct

import numpy as np
import pytest

import lookup_edges as E
import oracle as O
from cilium_amd import _lib as L
from cilium_amd import ipcache
from cilium_amd import synth as S
from cilium_amd.datapath import Datapath, pack
from cilium_amd.loader import load_tables

pytestmark = pytest.mark.gpu
WIDTHS = (16, 17, 18)


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


def run(torch, cases, dir_bits):
    """The cases (one table set) on a context with the width forced ->
    ([(action, verdict, identity)], the stats)"""
    t = cases[0].tables
    dp = Datapath(0)
    try:
        dp.set_option(L.OPT_LPM4_DIR_BITS, dir_bits)
        load_tables(dp, t)
        st = dp.stats()
        assert st["lpm4_layout"] == L.LPM4_TRIE
        # the directory is 16 B x 2^D; these tables' chunks and lists are small
        assert st["lpm4_kib"] >> 10 == 1 << (dir_bits - 16), st["lpm4_kib"]
        return classify_all(torch, dp, O.Oracle(t), cases), st
    finally:
        dp.close()


def same(a, b):
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)


# ---------------------------------------- the structural streams, every width
@functools.lru_cache(None)
def structural_at_16(torch, order):
    cases = [E.lpm4_structural(order, "ingress"), E.lpm4_structural(order, "egress")]
    return run(torch, cases, 16)[0]


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("dir_bits", [17, 18])
def test_structural_streams(torch, dir_bits, order):
    cases = [E.lpm4_structural(order, "ingress"), E.lpm4_structural(order, "egress")]
    outs, _ = run(torch, cases, dir_bits)
    same(outs, structural_at_16(torch, order))
    lab, _ = E.brute_lpm4(cases[0].claims["prefixes"], cases[0].claims["host"])
    np.testing.assert_array_equal(outs[1][2][lab != 0], lab[lab != 0])


# ------------------------------------------------- the edges of a /D directory
W26 = E.WIDE26


@functools.lru_cache(None)
def edge_prefixes(D):
    """-> ([(host-order address, plen, label)], probes) for a /D directory"""
    sh = 32 - D
    P, pr = {}, []

    def add(a, l, label):
        P[(a & E.mask4(l), l)] = label
    # lengths D-1, D, D+1 and 32 at one address: the painting over two (at a
    # narrower width four) entries, the entry's own leaf, a len - D = 1
    # inline entry
    A = E.host4("10.20.0.0")
    add(A, D - 1, 1011)
    add(A, D, 1012)
    add(A, D + 1, 1013)
    add(A + 1, 32, 1014)
    pr += [(A + o) & 0xFFFFFFFF for o in (0, 1, 2, 1 << (sh - 1), (1 << (sh - 1)) - 1, 1 << sh,
                                          (1 << sh) - 1, 2 << sh, (2 << sh) - 1, -1)]
    # a /D node with 2 (inline only), 3 (the shortest list), 14 (the longest)
    # and 15 (split) longer prefixes; a label past 26 bits on the longest
    # (inline) and on the shortest (a list entry, or a chunk's leaf)
    for k, n in enumerate((2, 3, 14, 15)):
        N = E.host4("10.32.0.0") + (k << sh)
        for i in range(n):
            a = N | (i + 1) << 4
            l = 32 if i == 0 else D + 1 if i == n - 1 else 28
            add(a, l, (W26 if i in (0, n - 1) else 0) + 1100 + 100 * k + i)
            pr += [a, a + 1, a + 15, a + 16]
        pr += [N, N + (1 << sh) - 1, N + (1 << (sh - 1)), N + (1 << (sh - 1)) - 1]
    # twenty /31 and /32 prefixes inside one /26: a split node whose second
    # chunk is the last one (128 entries at /17, 64 at /18), probed at every
    # address of the /26 and on both sides of it
    M = E.host4("10.48.0.64")
    for i in range(20):
        add(M + 3 * i, 31 if i % 5 == 4 else 32, (W26 if i & 1 else 0) + 2000 + i)
    pr += [M - 1 + o for o in range(66)]
    # directory indices of all ones and all zeros
    add(0xFFFFFF00, 24, 1031)
    add(0xFFFFFFFF, 32, W26 + 1032)
    add(0, D + 1, 1033)
    add(1, 32, 1034)
    pr += [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFF00, 0xFFFFFEFF, 0xFFFFC000, 0, 1, 2,
           (1 << (sh - 1)) - 1, 1 << (sh - 1), 1 << sh]
    return [(a, l, v) for (a, l), v in sorted(P.items())], np.array(pr, np.uint32)


@functools.lru_cache(None)
def edge_cases(D):
    pfx, probes = edge_prefixes(D)
    eps = E.endpoints4([S.LXC_IPV4, S.ip4("10.1.0.1"), S.ip4("10.1.0.2")])
    pol = E._lpm4_policy([p[2] for p in pfx] + [S.WORLD_ID])
    t = S.Tables(E.ipc4(pfx), eps, {E.EP0 + i: pol for i in range(3)},
                 np.zeros(0, S.PREFILTER_DT), {E.EP0 + i: S.EP_SECLABEL for i in range(3)})
    # every probe in 21 neighbouring lanes' worth of copies, shuffled; the
    # last wave is partial
    host = np.random.default_rng(D).permutation(np.resize(probes, 64 * 60 + 37))
    k = np.arange(len(host))
    la = S.local_v4_addrs(t)
    proto = np.where(k % 5 == 4, S.IPPROTO_UDP, S.IPPROTO_TCP)
    ing = E.Case(t, E.hdr4(E.raw4(host), la[k % 3], E.PORTS[(k // 3) % 4], proto), 0, 0, {})
    egr = E.Case(t, E.hdr4(S.LXC_IPV4, E.raw4(host), E.PORTS[k % 4], proto), 1, E.EP0, {})
    return pfx, host, [ing, egr]


@functools.lru_cache(None)
def edges_at(torch, D, dir_bits):
    return run(torch, edge_cases(D)[2], dir_bits)[0]


@pytest.mark.parametrize("dir_bits", WIDTHS)
@pytest.mark.parametrize("D", WIDTHS)
def test_directory_edges(torch, D, dir_bits):
    """The table built for a /D directory's edges, looked up at every width."""
    pfx, host, cases = edge_cases(D)
    assert len(host) % 64 == 37
    outs = edges_at(torch, D, dir_bits)
    same(outs, edges_at(torch, D, 16))
    lab, _ = E.brute_lpm4(pfx, host)
    assert (lab >= W26).sum() > 50 and (lab == 0).sum() > 0
    np.testing.assert_array_equal(outs[1][2][lab != 0], lab[lab != 0])


# ------------------------------------------------------ two commits under auto
def test_auto_widens_at_a_later_commit(torch):
    """A table a /16 directory resolves keeps /16; a commit that adds four
    prefixes to each of forty /16s (two per /17 half: a /16 directory leaves
    two of each four to a list, a /17 directory none) takes the width
    cfc_lpm4_dir_stats names, and lpm4_kib shows it.  A batch after each
    commit against the oracle."""
    first = [(E.host4(f"30.{i}.7.0"), 24, 1200 + i % 7) for i in range(50)]
    more = [(E.host4(f"31.{i}.{b}.0"), 24, 1200 + (i + b) % 7)
            for i in range(40) for b in (3, 100, 130, 250)]
    eps = E.endpoints4([S.LXC_IPV4])
    pol = E._lpm4_policy([p[2] for p in first] + [S.WORLD_ID])

    def tables(pfx):
        return S.Tables(E.ipc4(pfx), eps, {E.EP0: pol}, np.zeros(0, S.PREFILTER_DT),
                        {E.EP0: S.EP_SECLABEL})

    def case(t, pfx):
        host = np.resize(E.boundary4(pfx), 2000 + 13)
        k = np.arange(len(host))
        return E.Case(t, E.hdr4(E.raw4(host), S.LXC_IPV4, E.PORTS[k % 4]), 0, 0, {})
    dp = Datapath(0)
    try:
        t1 = tables(first)
        load_tables(dp, t1)
        st, auto = dp.lpm4_dir_stats()
        assert auto == 16 and st[16]["unresolved"] == 0
        assert dp.stats()["lpm4_kib"] == 1024
        classify_all(torch, dp, O.Oracle(t1), [case(t1, first)])
        ipc = ipcache.Map(dp, max_entries=ipcache.MaxEntries)
        for e in E.ipc4(more):
            ipc.Update(ipcache.Key(32 + int(e["plen"]), int(e["family"]), bytes(e["addr"])),
                       ipcache.RemoteEndpointInfo(int(e["label"]),
                                                  struct.pack("<I", int(e["tunnel"]))))
        dp.commit()
        st, auto = dp.lpm4_dir_stats()
        assert st[16]["unresolved"] == 80 and st[17]["unresolved"] == 0
        assert auto == AUTO_WIDER, (st, auto)
        assert dp.stats()["lpm4_kib"] == (st[auto]["bytes"] + 1023) // 1024
        assert dp.stats()["lpm4_kib"] >> 10 == 1 << (auto - 16)
        t2 = tables(first + more)
        classify_all(torch, dp, O.Oracle(t2), [case(t2, first + more)])
    finally:
        dp.close()


# what auto takes for a table whose /16 directory leaves 80 of 210 prefixes to
# a second load and whose /17 directory none (flatten.hpp L4_AUTO_SHARE_*:
# a tenth of the prefixes; DESIGN.md section 4 has the measurements behind it)
AUTO_WIDER = 17
