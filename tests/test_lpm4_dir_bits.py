"""The directory width of the compact IPv4 LPM (layout.h l4d, dir_bits 16, 17
or 18; CFC_OPT_LPM4_DIR_BITS) without a GPU: the selftest's host restatement
of l4_lookup against a brute-force longest-prefix match at every width, a
Python restatement of the builder's placement rule on the C2 tables (how many
headers need a second LPM load), and the builder's own counts through a
host-only context."""
import functools
import os
import re
import subprocess

import numpy as np

from cilium_amd import synth as S
from cilium_amd.datapath import host_only
from cilium_amd.loader import load_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L4_INLINE = 2
WIDTHS = (16, 17, 18)


def test_selftest_lpm4_every_width():
    csrc = os.path.join(ROOT, "cilium_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-s", "selftest"], check=True)
    r = subprocess.run([os.path.join(csrc, "build", "selftest"), "lpm4"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = re.findall(r"^lpm4 (\S+)\s+/(\d+) .* -> (\w+)$", r.stdout, flags=re.M)
    names = {n for n, _, _ in rows}
    assert {"random", "piled", "deep", "edges-16", "edges-17", "edges-18"} <= names
    for n in names:
        assert sorted(int(d) for m, d, _ in rows if m == n) == list(WIDTHS), n
    assert all(res == "ok" for _, _, res in rows), [x for x in rows if x[2] != "ok"]


@functools.lru_cache(None)
def c2():
    t = S.config_c2_bench(2)
    h = S.headers_c2(t, 400_000)
    e = t.ipcache[t.ipcache["family"] == 1]
    addr = S.byteswap32(e["addr"][:, :4].copy().view("<u4").ravel())
    plen = e["plen"].astype(np.int64)
    addr = addr & np.where(plen > 0, (0xFFFFFFFF << (32 - plen)) & 0xFFFFFFFF, 0).astype(np.uint32)
    return t, addr, plen, S.byteswap32(h.saddr)


def second_load_share(addr, plen, probes, D):
    """The share of probes whose /D directory entry does not answer them:
    the entry holds its two longest prefixes longer than /D inline
    (flatten.cpp L4Trie::node: longest first, equal lengths by address); a
    node with more sends every address outside those two to a list or a
    chunk.  Also the prefixes left to that second load."""
    sh = 32 - D
    lng = plen > D
    a, l = addr[lng].astype(np.int64), plen[lng]
    idx = a >> sh
    order = np.lexsort((a, -l, idx))
    a, l, idx = a[order], l[order], idx[order]
    nodes, first, cnt = np.unique(idx, return_index=True, return_counts=True)
    unresolved = int(np.maximum(cnt - L4_INLINE, 0).sum())
    p = probes.astype(np.int64)
    k = np.searchsorted(nodes, p >> sh)
    k[k == len(nodes)] = 0
    hit = nodes[k] == p >> sh
    many = hit & (cnt[k] > L4_INLINE)
    inl = np.zeros(len(p), bool)
    for j in range(L4_INLINE):
        e = np.minimum(first[k] + j, len(a) - 1)
        m = (0xFFFFFFFF << (32 - l[e])) & 0xFFFFFFFF
        inl |= (p & m) == a[e]
    return float((many & ~inl).mean()), unresolved


def test_second_load_share_halves_per_bit():
    """Measured: 0.207 / 0.069 / 0.020 of the headers at /16 / /17 / /18."""
    _, addr, plen, probes = c2()
    share = {D: second_load_share(addr, plen, probes, D)[0] for D in WIDTHS}
    print("second-load share", share)
    assert share[17] < share[16] / 2
    assert share[18] < share[17] / 2


def test_builder_counts_order_the_same_way():
    """cfc_lpm4_dir_stats on a host-only context: the builder's unresolved
    prefixes per width are the restatement's, fall with the width, and a
    wider directory costs bytes."""
    t, addr, plen, probes = c2()
    dp = host_only()
    try:
        only = S.Tables(t.ipcache, t.endpoints[:0], {}, t.prefilter[:0], {})
        load_tables(dp, only, commit=False)
        st, auto = dp.lpm4_dir_stats()
    finally:
        dp.close()
    print("builder", st, "auto", auto)
    for D in WIDTHS:
        assert st[D]["prefixes"] == len(addr)
        assert st[D]["unresolved"] == second_load_share(addr, plen, probes, D)[1]
        assert st[D]["bytes"] >= 16 << D
    assert st[16]["unresolved"] > st[17]["unresolved"] > st[18]["unresolved"]
    assert st[16]["bytes"] < st[17]["bytes"] < st[18]["bytes"]
    assert auto in WIDTHS


def test_option_values():
    from cilium_amd import _lib as L
    dp = host_only()
    try:
        for v in (0, 16, 17, 18):
            dp.set_option(L.OPT_LPM4_DIR_BITS, v)
        for v in (1, 15, 19, -1):
            try:
                dp.set_option(L.OPT_LPM4_DIR_BITS, v)
            except OSError:
                continue
            raise AssertionError(f"dir_bits {v} accepted")
        st, auto = dp.lpm4_dir_stats()   # no ipcache map: nothing to resolve
        assert auto == 16 and all(st[D]["unresolved"] == 0 for D in WIDTHS)
    finally:
        dp.close()
