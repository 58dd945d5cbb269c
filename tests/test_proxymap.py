"""cilium_proxy4 / cilium_proxy6 without a GPU: the maps' roles and geometry,
the map API on a host-only context, the pkg/maps/proxymap mirror
(cilium_amd/proxymap.py) against hand-written reference-format strings and
hand-made maps, the restatement of the entries (proxy_entries.py) against
what the reference fixtures pin, and the preconditions of the GPU streams
(proxy_streams.py) from the oracle alone."""
import ctypes
import errno
import struct

import numpy as np
import pytest

import golden_io as G
import oracle as O
import proxy_entries as P
import proxy_streams as PS
from cilium_amd import _lib as L
from cilium_amd import proxymap as PM
from cilium_amd.datapath import host_only


@pytest.fixture
def dp():
    d = host_only()
    yield d
    d.close()


def _open_rc(dp, name, mtype, ks, vs, n=64):
    fd, created = ctypes.c_int(), ctypes.c_int()
    return dp.L.cfc_map_open(dp.h, name.encode(), mtype, ks, vs, n, 0, ctypes.byref(fd),
                             ctypes.byref(created))


# ---- roles ---------------------------------------------------------------

@pytest.mark.parametrize("name,mtype,ks,vs", [
    ("cilium_proxy4", 1, 10, 12), ("cilium_proxy4", 1, 12, 16), ("cilium_proxy4", 9, 10, 16),
    ("cilium_proxy6", 1, 22, 16), ("cilium_proxy6", 1, 10, 16), ("cilium_proxy6", 11, 22, 28),
    ("/sys/fs/bpf/tc/globals/cilium_proxy4", 1, 14, 56),
])
def test_role_geometry_refused(dp, name, mtype, ks, vs):
    """struct proxy4_tbl_key / _value are 10 / 16 bytes, proxy6's 22 / 28
    (common.h:478-508), both HASH: anything else is -EINVAL, as for the other
    role maps"""
    assert _open_rc(dp, name, mtype, ks, vs) == -errno.EINVAL


def test_role_geometry_accepted_and_shared(dp):
    fd, new = dp.open_or_create_map("cilium_proxy4", 1, 10, 16, 64)
    assert new
    # the pin path's basename selects the role: the same map
    fd2, new2 = dp.open_or_create_map("/sys/fs/bpf/tc/globals/cilium_proxy4", 1, 10, 16, 64)
    assert not new2
    dp.update_element(fd, b"\x01" * 10, b"\x02" * 16)
    assert dp.lookup_element(fd2, b"\x01" * 10) == b"\x02" * 16
    assert _open_rc(dp, "cilium_proxy4", 1, 10, 16, 128) == -errno.EINVAL   # objCheck
    fd6, new6 = dp.open_or_create_map("cilium_proxy6", 1, 22, 28, 64)
    assert new6


def test_map_api_host_only(dp):
    """lookup, delete, get_next_key and dump — what proxymap.Lookup, GC and
    CleanupOnRedirectClose use — and HASH's -E2BIG at max_entries"""
    fd, _ = dp.open_or_create_map("cilium_proxy4", 1, 10, 16, 4)
    keys = [PM.Proxy4Key(f"10.0.0.{i}", 1000 + i, 10001).pack() for i in range(4)]
    vals = [PM.Proxy4Value(f"10.9.0.{i}", 80, 100 + i, 720).pack() for i in range(4)]
    for k, v in zip(keys, vals):
        dp.update_element(fd, k, v)
    with pytest.raises(L.CfcError) as e:
        dp.update_element(fd, PM.Proxy4Key("10.0.0.9", 1, 2).pack(), vals[0])
    assert e.value.errno == errno.E2BIG
    dp.update_element(fd, keys[1], vals[3])            # an existing key still updates
    assert dp.lookup_element(fd, keys[1]) == vals[3]
    assert sorted(dp.keys(fd)) == sorted(keys)
    k, v = dp.dump(fd)
    assert k.shape == (4, 10) and v.shape == (4, 16)
    assert {bytes(a): bytes(b) for a, b in zip(k, v)} == \
        {keys[0]: vals[0], keys[1]: vals[3], keys[2]: vals[2], keys[3]: vals[3]}
    dp.delete_element(fd, keys[0])
    assert dp.lookup_element(fd, keys[0]) is None
    with pytest.raises(L.CfcError) as e:
        dp.delete_element(fd, keys[0])
    assert e.value.errno == errno.ENOENT


def test_proxy_calls_host_only(dp):
    """no device: -ENODEV from all four calls (before anything else of the
    arguments matters); NULL arguments are -EINVAL"""
    PM.ProxyMap(dp)
    hdr4, hdr6, out, st = L.HdrV4(), L.HdrV6(), L.Out(), L.ProxyStats()
    cnt = ctypes.c_uint64()
    for fn, hdr in ((dp.L.cfc_proxy_apply_v4, hdr4), (dp.L.cfc_proxy_apply_v6, hdr6)):
        assert fn(dp.h, ctypes.byref(hdr), ctypes.byref(out), 0, 0, ctypes.byref(st),
                  None) == -errno.ENODEV
        assert fn(dp.h, ctypes.byref(hdr), ctypes.byref(out), 0, 0, None, None) == -errno.EINVAL
        assert fn(dp.h, ctypes.byref(hdr), ctypes.byref(out), 7, 0, ctypes.byref(st),
                  None) == -errno.EINVAL
    for fn, hdr in ((dp.L.cfc_proxy_entries_v4, hdr4), (dp.L.cfc_proxy_entries_v6, hdr6)):
        assert fn(dp.h, ctypes.byref(hdr), ctypes.byref(out), 0, 0, None, None, 0,
                  ctypes.byref(cnt), None) == -errno.ENODEV
        assert fn(dp.h, ctypes.byref(hdr), ctypes.byref(out), 0, 0, None, None, 0, None,
                  None) == -errno.EINVAL


def test_exports_and_abi():
    for name in ("cfc_proxy_entries_v4", "cfc_proxy_entries_v6", "cfc_proxy_apply_v4",
                 "cfc_proxy_apply_v6"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().cfc_abi_version() == 13
    assert ctypes.sizeof(L.ProxyStats) == 40


# ---- pkg/maps/proxymap ------------------------------------------------------

def test_pack_and_string_forms():
    """byte layouts of common.h:478-508 and the String() forms of
    proxymap/ipv4.go:98-124, ipv6.go:93-119, written out by hand"""
    k = PM.Proxy4Key("10.1.2.3", 40000, 10001, 6)
    # saddr, dport be16, sport be16, nexthdr, pad
    assert k.pack() == bytes([10, 1, 2, 3, 0x27, 0x11, 0x9C, 0x40, 6, 0])
    assert k.String() == "10.1.2.3:40000 (6) => 10001"
    assert k.HostPort() == "10.1.2.3:40000"
    assert PM.Proxy4Key.unpack(k.pack()) == k
    v = PM.Proxy4Value("192.168.7.9", 8080, 1234, 1720)
    assert v.pack() == bytes([192, 168, 7, 9, 0x1F, 0x90, 0, 0]) + struct.pack("<II", 1234, 1720)
    assert v.String() == "192.168.7.9:8080 identity 1234 lifetime 1720"
    assert v.HostPort() == "192.168.7.9:8080" and v.GetSourceIdentity() == 1234
    assert PM.Proxy4Value.unpack(v.pack()) == v
    k6 = PM.Proxy6Key("fd00::1:2", 53, 10003, 17)
    a6 = bytes([0xfd, 0] + [0] * 10 + [0, 1, 0, 2])
    assert k6.pack() == a6 + bytes([0x27, 0x13, 0x00, 0x35, 17, 0]) and len(k6.pack()) == 22
    assert k6.String() == "[fd00::1:2]:53 (17) => 10003"
    assert PM.Proxy6Key.unpack(k6.pack()) == k6
    v6 = PM.Proxy6Value("beef::1", 443, 70000, 5)
    assert v6.pack() == bytes([0xbe, 0xef] + [0] * 13 + [1]) + bytes([0x01, 0xBB, 0, 0]) + \
        struct.pack("<II", 70000, 5)
    assert len(v6.pack()) == 28
    assert v6.String() == "beef::1:443 identity 70000 lifetime 5"   # (no brackets: ipv6.go:117)
    assert v6.HostPort() == "[beef::1]:443"
    assert PM.Proxy6Value.unpack(v6.pack()) == v6


def _hand_made(dp):
    m = PM.ProxyMap(dp, max_entries=64)
    rows4 = [(PM.Proxy4Key("10.0.0.1", 1001, 10001, 6), PM.Proxy4Value("10.9.0.1", 80, 300, 100)),
             (PM.Proxy4Key("10.0.0.2", 1002, 10001, 17), PM.Proxy4Value("10.9.0.1", 53, 301, 200)),
             (PM.Proxy4Key("10.0.0.3", 1003, 10002, 6), PM.Proxy4Value("10.9.0.2", 80, 302, 300)),
             (PM.Proxy4Key("10.0.0.4", 1004, 10001, 6), PM.Proxy4Value("10.9.0.2", 80, 303, 400))]
    rows6 = [(PM.Proxy6Key("fd00::1", 2001, 10001, 6), PM.Proxy6Value("fd00::9", 80, 400, 150)),
             (PM.Proxy6Key("fd00::2", 2002, 10001, 58), PM.Proxy6Value("fd00::9", 0, 401, 350))]
    for k, v in rows4:
        dp.update_element(m.fd4, k.pack(), v.pack())
    for k, v in rows6:
        dp.update_element(m.fd6, k.pack(), v.pack())
    return m, rows4, rows6


def test_lookup_and_delete(dp):
    m, rows4, rows6 = _hand_made(dp)
    assert m.lookup(rows4[2][0]) == rows4[2][1]
    assert m.lookup(rows6[1][0]).String() == "fd00::9:0 identity 401 lifetime 350"
    with pytest.raises(KeyError) as e:
        m.lookup(PM.Proxy4Key("10.0.0.1", 1001, 10009, 6))
    assert "unable to find IPv4 proxy entry for 10.0.0.1:1001 (6) => 10009" in str(e.value)
    m.delete(rows4[2][0])
    with pytest.raises(KeyError):
        m.lookup(rows4[2][0])
    assert len(m.dump()) == 3 and len(m.dump(v6=True)) == 2


def test_gc_deletes_expired_only(dp):
    """doGc: lifetime < time (ipv4.go:151), both maps"""
    m, rows4, rows6 = _hand_made(dp)
    assert m.gc(100) == 0                       # lifetime 100 is not < 100
    assert m.gc(201) == 3                       # 100, 200 and the IPv6 150
    assert {k.String() for k, _ in m.dump()} == {rows4[2][0].String(), rows4[3][0].String()}
    assert [k for k, _ in m.dump(v6=True)] == [rows6[1][0]]
    assert m.gc(201) == 0


def test_flush(dp):
    m, rows4, rows6 = _hand_made(dp)
    assert m.flush() == 6
    assert m.dump() == [] and m.dump(v6=True) == []


def test_cleanup_on_redirect_close_tcp_only(dp):
    """cleanupIPv4Redirects / cleanupIPv6Redirects (ipv4.go:175-196,
    ipv6.go:149-170) delete the port's TCP entries and leave its UDP and
    ICMPv6 ones"""
    m, rows4, rows6 = _hand_made(dp)
    assert m.cleanup_on_redirect_close(10001) == 3
    assert {k.String() for k, _ in m.dump()} == {"10.0.0.2:1002 (17) => 10001",
                                                  "10.0.0.3:1003 (6) => 10002"}
    assert [k.String() for k, _ in m.dump(v6=True)] == ["[fd00::2]:2002 (58) => 10001"]
    assert m.cleanup_on_redirect_close(10001) == 0


# ---- the restatement against the reference fixtures ---------------------------

# redirected headers per ingress fixture (counted from the fixtures)
FIXTURES = {"edge_ingress_v4": 42, "edge_ingress_v6": 135, "ct_seq_ingress_v4": 17,
            "c2_ingress_v4": 2, "c3_ingress_v6": 1}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_restatement_matches_fixture_pins(name):
    """What the reference's own run pins of its proxy-map writes: the
    entry's identity (x_identity, full mask: gen_golden reads it from
    cilium_proxy4/6), the rewritten destination port (x_verdict) = the key's
    dport, and the unchanged source port (x_pkt) = the key's sport"""
    g = G.Golden(name)
    red = np.flatnonzero(g.verdict > 0)
    assert len(red) == FIXTURES[name] and g.mode in (0, 3)
    assert (g.idmask_reported[red] == 0xFFFFFFFF).all()
    o = O.Oracle(g.tables)
    r = o.classify(g.headers, g.mode, g.ep_lxc, want_ct=True, want_pkt=True,
                   apply_ct=g.ct_after is not None)
    act, ver, ide, ct, pkt = r
    np.testing.assert_array_equal(ver[red], g.verdict[red])
    np.testing.assert_array_equal(ide[red], g.identity_reported[red])
    v6 = g.headers.family == 6
    n = 16 if v6 else 4
    for i in red:
        key, val, res, dest, tr = P.entry_of(g.headers, int(i), g.mode, ver, ide, ct, pkt)
        dport, sport, nh = struct.unpack_from("<HHB", key, n)
        assert res in (P.CT_NEW, P.CT_ESTABLISHED) and not dest and not tr
        assert dport == int(g.verdict[i]) & 0xFFFF
        assert struct.unpack_from("<I", val, n + 4)[0] == int(g.identity_reported[i])
        assert nh == int(g.headers.proto[i])
        if g.pkt is not None:
            assert sport == int(g.pkt[i, 8 if v6 else 2]) & 0xFFFF
        assert sport == int(g.headers.sport[i])
        # the key's address is the packet's source, the value its destination
        assert key[:n] == P._addr(g.headers.saddr[i], v6)
        assert val[:n] == P._addr(g.headers.daddr[i], v6)
        assert struct.unpack_from("<H", val, n)[0] == int(g.headers.dport[i])
    rec, idx, st = P.expected_entries(g.headers, g.mode, ver, ide, ct, pkt)
    assert st["redirects"] == len(red)
    if name == "ct_seq_ingress_v4":
        assert len(rec) == 1 and idx[0] == red[-1]   # 17 writes of one key


# ---- preconditions of the GPU streams ----------------------------------------

@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_stream_preconditions(v6):
    """the oracle alone gives the cases test_gpu_proxymap.py relies on"""
    st = PS.want("ingress", v6)[3][2]
    assert st["redirects"] >= 1000 and st["rewrites"] >= 500, st
    assert st["new"] >= 200 and st["established"] >= 200 and st["dest_stage"] == 0, st
    st = PS.want("egress", v6)[3][2]
    assert min(st["new"], st["established"], st["reply"]) >= 200, st
    st = PS.want("dest", v6)[3][2]
    assert st["redirects"] >= 1000 and st["dest_stage"] == st["redirects"], st


def test_service_stream_preconditions():
    t, h, mode, ep = PS.lb_tables()
    act, ver, ide, ct, pkt = PS.oracle_run(t, [(h, mode, ep)])[0]
    rec, idx, st = P.expected_entries(h, mode, ver, ide, ct, pkt, seclabel=t.seclabel[ep],
                                      now=PS.CLOCK)
    assert st["translated"] >= 32, st
    # a flow looped back into its sender keeps the service address as orig_dip
    loop = (pkt[:, 0] != h.saddr) & (ver > 0) & ((ct & 3) < 2)
    assert loop.sum() >= 1
    i = int(np.flatnonzero(loop)[0])
    key, val, *_ = P.entry_of(h, i, mode, ver, ide, ct, pkt, seclabel=t.seclabel[ep])
    assert val[:4] == struct.pack("<I", int(h.daddr[i]))


def test_restatement_orientation_by_hand():
    """one TCP header by hand in each orientation"""
    from cilium_amd import synth as S
    h = S.Headers(4, np.array([S.ip4("10.0.0.1")], np.uint32),
                  np.array([S.ip4("10.0.0.2")], np.uint32), S.htons(np.array([4000])),
                  S.htons(np.array([80])), np.array([6], np.uint8), np.zeros(1, np.uint8),
                  np.array([100], np.uint16), np.zeros(1, np.uint32))
    ver = np.array([int(S.htons(10001))], np.int32)
    ide = np.array([777], np.uint32)
    # ingress, CT_NEW: key = the source, orig = the destination
    key, val, *_ = P.entry_of(h, 0, 0, ver, ide, np.array([4 | 8], np.uint8), now=5)
    assert PM.Proxy4Key.unpack(key).String() == "10.0.0.1:4000 (6) => 10001"
    assert PM.Proxy4Value.unpack(val).String() == "10.0.0.2:80 identity 777 lifetime 725"
    # egress, CT_REPLY: the tuple stays as loaded
    key, val, *_ = P.entry_of(h, 0, 1, ver, ide, np.array([4 | 2], np.uint8), seclabel=9)
    assert PM.Proxy4Key.unpack(key).String() == "10.0.0.2:80 (6) => 10001"
    assert PM.Proxy4Value.unpack(val).String() == "10.0.0.2:4000 identity 9 lifetime 720"
