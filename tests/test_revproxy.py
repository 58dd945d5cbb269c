"""The reverse-proxy pass without a GPU: the host flattener of the proxy maps
against a brute-force map lookup (the selftest's `revproxy` section), the
restatement (revproxy_ref.py) on hand-made headers, what the streams of
test_gpu_revproxy.py claim about themselves, and the ABI of
cfc_classify_from_host_v4/v6 on a host-only context."""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import revproxy_ref as R
import revproxy_streams as RS
from cilium_amd import _lib as L
from cilium_amd import synth as S
from cilium_amd.datapath import host_only

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------- host flattener
def test_selftest_revproxy():
    csrc = os.path.join(ROOT, "cilium_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-s", "selftest"], check=True)
    r = subprocess.run([os.path.join(csrc, "build", "selftest"), "revproxy"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    rows = re.findall(r"^revproxy (\S+) +v(\d) (\d+) entries, (\d+) slots, (\d+) absent keys, "
                      r"(\d+) wrapped -> ok$", r.stdout, flags=re.M)
    got = {(name, int(f)): (int(n), int(s), int(w)) for name, f, n, s, a, w in rows}
    for f in (4, 6):
        # 0, 1, 2 entries; a power of two and one above it: the slot count
        # doubles between them (load <= 1/2)
        for n, slots in ((0, 0), (1, 2), (2, 4), (4, 8), (5, 16), (64, 128), (65, 256),
                         (1000, 2048)):
            assert got[(f"n{n}", f)][:2] == (n, slots)
        assert got[("one-field", f)][:2] == (5, 16)
        assert got[("wrap", f)][:2] == (4, 8) and got[("wrap", f)][2] >= 2
    assert len(rows) == 20 and "FAIL" not in r.stdout


# -------------------------------------------------------------- the restatement
def test_mark_encoding():
    for ident in (0, 1, 2, 255, 256, 777, 0xFFFF, 0x10000, 0xABCDEF, 0xFFFFFF):
        for magic in (0xA00, 0xB00):
            got, skip = R.identity_from_mark(magic | R.enc(ident))
            assert got == ident and skip == (magic == 0xA00)
        assert R.enc(ident) & 0xFF00 == 0          # the magic's and bit 12's byte stays free
    assert R.identity_from_mark(0) == (S.WORLD_ID, False)
    assert R.identity_from_mark(0xC00) == (S.HOST_ID, False)
    assert R.identity_from_mark(0xD00 | R.enc(777)) == (S.WORLD_ID, False)
    assert R.MARK_HIT == L.MARK_HIT == 0x1A00 and R.MARK_HIT & 0xF00 == 0xA00
    # bit 12 changes nothing a plain classify reads from a mark
    assert R.identity_from_mark(R.MARK_HIT) == R.identity_from_mark(0xA00)


def test_source_identity_rule():
    for fam in (4, 6):
        assert R.source_identity(fam, 0, 1000) == 1000
        assert R.source_identity(fam, 0, 0) == S.WORLD_ID
        assert R.source_identity(fam, 0, S.CLUSTER_ID) == S.WORLD_ID
        assert R.source_identity(fam, 0xC00, 0) == S.HOST_ID
        assert R.source_identity(fam, 0xC00, 1000) == 1000
        assert R.source_identity(fam, 0xA00 | R.enc(777), 1000) == 777
        assert R.source_identity(fam, 0xB00 | R.enc(777), 1000) == 777
        assert R.source_identity(fam, 0xA00 | R.enc(2), 1000) == 1000
        assert R.source_identity(fam, 0xA00 | R.enc(0), 0) == 0
        assert R.source_identity(fam, 0xA00 | R.enc(0), 1000) == 1000
        assert R.source_identity(fam, 0, RS.BIG) == RS.BIG
    # the family difference: IPv4 ignores a HOST_ID label, IPv6 takes it
    assert R.source_identity(4, 0, S.HOST_ID) == S.WORLD_ID
    assert R.source_identity(6, 0, S.HOST_ID) == S.HOST_ID


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_translate_by_hand(v6):
    s = RS.src_addrs(v6)
    p = RS.proxy_pkt(v6, s["real"], 41000, 0xB00 | R.enc(777))
    key, val = RS.entry_for(v6, p, 0, RS.orig_daddr(v6, 0), odport=8080, lifetime=1)
    al = 16 if v6 else 4
    # the key: {saddr = the packet's daddr, dport = its source port, sport =
    # its destination port, nexthdr, pad}
    assert key[:al] == bytes(np.asarray(RS.ep_addr(v6)).reshape(-1).view(np.uint8))
    assert key[al:al + 2] == int(RS.PROXY_PORT).to_bytes(2, "little")
    assert key[al + 2:al + 4] == int(S.htons(41000)).to_bytes(2, "little")
    assert key[al + 4:] == bytes([6, 0])
    # misses: another address, either port, the other protocol, ICMP, SCTP;
    # IPv6 behind an extension header
    other = RS.proxy_pkt(v6, s["real"], 41000, 0, daddr=RS.orig_daddr(v6, 5))
    parts = [p, other, RS.proxy_pkt(v6, s["real"], 41001), RS.proxy_pkt(v6, s["real"], 41000,
             sport=int(S.htons(10002))), RS.proxy_pkt(v6, s["real"], 41000, proto=17),
             RS.proxy_pkt(v6, s["real"], 41000, proto=58 if v6 else 1),
             RS.proxy_pkt(v6, s["real"], 41000, proto=132),
             RS.proxy_pkt(v6, s["real"], 41000, flags=S.HF_FRAG)]
    if v6:
        parts.append(RS.proxy_pkt(v6, s["real"], 41000, flags=S.HF_EXTHDR))
    h = RS.concat(parts)
    tr = R.translate(h, {key: val}, np.full(len(h), 1000, np.uint32))
    want_hit = [True] + [False] * 6 + [True] + ([False] if v6 else [])   # (a fragment is looked up)
    assert tr.hit.tolist() == want_hit
    for i in np.flatnonzero(tr.hit):
        assert bytes(np.asarray(tr.saddr[i]).reshape(-1).view(np.uint8)) == val[:al]
        assert int(tr.l4word[i]) == int(S.htons(8080)) | int(S.htons(41000)) << 16
        # (the first carries the proxy's mark; the fragment mark 0: the label)
        assert int(tr.mark[i]) == R.MARK_HIT and int(tr.identity[i]) == (777 if i == 0 else 1000)
    miss = ~tr.hit
    assert (tr.mark[miss] == h.mark[miss]).all() and (tr.identity[miss] == 0).all()
    assert (tr.l4word[miss] == (h.sport.astype(np.uint32) | h.dport.astype(np.uint32) << 16)[miss]).all()
    th = tr.headers(h)
    assert int(th.mark[0]) == 0xA00 | R.enc(777) and (th.daddr == h.daddr).all()


# --------------------------------------------------- what the streams claim
@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_round_trip_stream(v6):
    x = RS.round_trip(v6)
    hit = x.tr.hit
    assert 600 <= hit.sum() <= 700 and (~hit).sum() >= 1000
    assert x.extra["unlabelled"]
    assert (x.extra["ver1"] > 0).sum() >= 1000         # batch 1: redirected
    # every kind of mark among the hit rows, and identities from the marks
    magic = x.h.mark[hit] & 0xF00
    assert {0, 0xA00, 0xB00, 0xC00} <= set(magic.tolist())
    assert (x.ide[hit] == x.tr.identity[hit]).all()
    # the translated replies belong to the flows batch 1 created: CT_REPLY,
    # forwarded whatever the policy says; untranslated they are new flows
    # the endpoint's policy drops
    pa, pv, pi, pc = x.extra["plain"]
    assert ((x.ct[hit] & 3) == 2).all() and (x.ver[hit] == 0).all()
    assert ((pc[hit] & 3) == 0).all() and (pv[hit] < 0).all()
    assert (pi[~hit] == x.ide[~hit]).all()           # rows that miss: the same packet
    assert len(x.extra["events"][0]) >= hit.sum()     # TRACE_TO_LXC records of the replies


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_identity_rows_stream(v6):
    t, t2, entries, h, cases = RS.identity_rows(v6)
    x = RS.expect(t, entries, h, oracle_tables=t2)
    assert x.tr.hit.all() and x.extra["unlabelled"]       # (for the second oracle)
    # ... while the first one's ipcache labels every translated source
    import oracle as O
    lab, hit = O.Oracle(t).ipcache_lookup(h.family, x.tr.saddr)
    assert hit.all() and (lab >= 2000).all()
    assert [int(i) for i in x.tr.identity] == [c[1] for c in cases]
    assert (x.ide == x.tr.identity).all()
    want_ver = [0 if c[1] in (RS.REAL, RS.ID_A, S.HOST_ID) else -133 for c in cases]
    assert x.ver.tolist() == want_ver
    names = dict(cases)
    assert names["mark0-host"] == (S.HOST_ID if v6 else S.WORLD_ID)
    # with the prefixes in, the oracle would take the translated source's
    # label for the reserved identities: that is what must not happen
    y = RS.expect(t, entries, h)
    differs = y.ide != x.ide
    assert differs.any() and (x.ide[differs] < 4).all() and (y.ide[differs] >= 2000).all()


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
@pytest.mark.parametrize("allowed", [True, False], ids=["allowed", "denied"])
def test_big_identity_stream(v6, allowed):
    t, entries, p, stand = RS.big_identity(v6, allowed)
    tr = R.translate(p, entries, RS.labels_of(__import__("oracle").Oracle(t), p))
    assert tr.hit.all() and int(tr.identity[0]) == RS.BIG >= 1 << 24
    x = RS.expect(t, entries, stand)
    assert x.tr.hit.all() and x.ver.tolist() == [0 if allowed else -133]
    assert int(x.ide[0]) == (RS.REAL if allowed else RS.ID_P)


# -------------------------------------------------------------------- the ABI
def test_abi():
    lib = L.lib()
    assert lib.cfc_abi_version() == 13
    for name in ("cfc_classify_from_host_v4", "cfc_classify_from_host_v6"):
        assert name in L.EXPORTS and hasattr(lib, name)
    dp = host_only()
    try:
        buf = (ctypes.c_uint32 * 64)()
        p = ctypes.addressof(buf)
        a16 = (p + 15) & ~15
        out = L.Out(p, p, None, None, None, None, None, None)
        for fn, hdr in ((lib.cfc_classify_from_host_v4, L.HdrV4), (lib.cfc_classify_from_host_v6,
                                                                  L.HdrV6)):
            v6 = hdr is L.HdrV6
            h = hdr(a16, a16, p, p, None, None, 1, None)
            good = L.RevproxyCols(a16, p, p, p, None)
            run = lambda hh, cc, oo: fn(dp.h, ctypes.byref(hh) if hh else None,  # noqa: E731
                                        ctypes.byref(cc) if cc else None,
                                        ctypes.byref(oo) if oo else None, None)
            assert run(h, good, out) == -errno.ENODEV          # a host-only context
            assert run(None, good, out) == -errno.EINVAL
            assert run(h, None, out) == -errno.EINVAL
            assert run(h, good, None) == -errno.EINVAL
            for k in range(4):                                  # a NULL required column
                cols = [a16, p, p, p, None]
                cols[k] = None
                assert run(h, L.RevproxyCols(*cols), out) == -errno.EINVAL
            assert run(h, good, L.Out(None, p, None, None, None, None, None, None)) == -errno.EINVAL
            assert run(hdr(None, a16, p, p, None, None, 1, None), good, out) == -errno.EINVAL
            if v6:                                              # a misaligned IPv6 row
                assert run(h, L.RevproxyCols(a16 + 4, p, p, p, None), out) == -errno.EINVAL
                assert run(hdr(a16 + 8, a16, p, p, None, None, 1, None), good, out) == -errno.EINVAL
                assert run(hdr(a16, a16 + 4, p, p, None, None, 1, None), good, out) == -errno.EINVAL
            else:
                assert run(h, L.RevproxyCols(a16 + 4, p, p, p, None), out) == -errno.ENODEV
    finally:
        dp.close()
