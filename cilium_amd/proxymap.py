"""pkg/maps/proxymap over the engine's map API: cilium_proxy4 and
cilium_proxy6, which ipv{4,6}_redirect_to_host_port (bpf/lib/lxc.h:96-191)
writes for every packet redirected to the L7 proxy — here
Datapath.proxy_apply — and pkg/proxy reads for every connection it accepts
(pkg/proxy/socket.go:441 proxymap.Lookup).

Keys and values hold ports in host order, as the Go structs do after
ToNetwork() of a map entry; pack() is ToNetwork() (ipv4.go:105-111, 118-123):
struct proxy4_tbl_key {saddr, dport, sport, nexthdr, pad} / proxy4_tbl_value
{orig_daddr, orig_dport, pad, identity, lifetime} (common.h:478-508)."""
from __future__ import annotations

import socket
import struct

from .datapath import Datapath

MaxEntries = 524288                       # proxymap.go:25
Proxy4MapName = "cilium_proxy4"           # ipv4.go:32
Proxy6MapName = "cilium_proxy6"
MAP_TYPE_HASH = 1
PROXY_DEFAULT_LIFETIME = 720              # common.h:466


def _be16(x):
    return struct.unpack("<H", struct.pack(">H", x & 0xFFFF))[0]


def _ip(ip, v6):
    if isinstance(ip, (bytes, bytearray)):
        return bytes(ip)
    return socket.inet_pton(socket.AF_INET6 if v6 else socket.AF_INET, ip)


def _ntop(b):
    return socket.inet_ntop(socket.AF_INET6 if len(b) == 16 else socket.AF_INET, b)


def _join_host_port(host, port):          # net.JoinHostPort
    return f"[{host}]:{port}" if ":" in host else f"{host}:{port}"


class Proxy4Key:
    """struct proxy4_tbl_key (10 bytes)."""
    V6 = False
    SIZE = 10

    def __init__(self, saddr, sport, dport, nexthdr=6):
        self.SAddr = _ip(saddr, self.V6)
        self.SPort, self.DPort, self.Nexthdr = int(sport), int(dport), int(nexthdr)

    def pack(self):
        return self.SAddr + struct.pack("<HHBB", _be16(self.DPort), _be16(self.SPort),
                                        self.Nexthdr, 0)

    @classmethod
    def unpack(cls, b):
        n = cls.SIZE - 6
        dport, sport, nh, _ = struct.unpack_from("<HHBB", b, n)
        return cls(bytes(b[:n]), _be16(sport), _be16(dport), nh)

    def HostPort(self):                                 # ipv4.go:44-47
        return _join_host_port(_ntop(self.SAddr), self.SPort)

    def String(self):                                   # ipv4.go:98-100
        return f"{self.HostPort()} ({self.Nexthdr}) => {self.DPort}"

    def __eq__(self, o):
        return type(o) is type(self) and o.pack() == self.pack()

    def __hash__(self):
        return hash(self.pack())


class Proxy4Value:
    """struct proxy4_tbl_value (16 bytes)."""
    V6 = False
    SIZE = 16

    def __init__(self, orig_daddr, orig_dport, identity=0, lifetime=0):
        self.OrigDAddr = _ip(orig_daddr, self.V6)
        self.OrigDPort, self.SourceIdentity = int(orig_dport), int(identity)
        self.Lifetime = int(lifetime)

    def pack(self):
        return self.OrigDAddr + struct.pack("<HHII", _be16(self.OrigDPort), 0,
                                            self.SourceIdentity, self.Lifetime)

    @classmethod
    def unpack(cls, b):
        n = cls.SIZE - 12
        dport, _, ident, life = struct.unpack_from("<HHII", b, n)
        return cls(bytes(b[:n]), _be16(dport), ident, life)

    def GetSourceIdentity(self):
        return self.SourceIdentity

    def HostPort(self):                                 # ipv4.go:62-65
        return _join_host_port(_ntop(self.OrigDAddr), self.OrigDPort)

    def String(self):                                   # ipv4.go:121-124
        return (f"{_ntop(self.OrigDAddr)}:{self.OrigDPort} identity "
                f"{self.SourceIdentity} lifetime {self.Lifetime}")

    def __eq__(self, o):
        return type(o) is type(self) and o.pack() == self.pack()


class Proxy6Key(Proxy4Key):
    """struct proxy6_tbl_key (22 bytes); String as ipv6.go:93-95."""
    V6 = True
    SIZE = 22


class Proxy6Value(Proxy4Value):
    """struct proxy6_tbl_value (28 bytes); String as ipv6.go:116-119."""
    V6 = True
    SIZE = 28


class ProxyMap:
    """Both maps, with the package's calls (proxymap.go)."""

    def __init__(self, dp: Datapath, max_entries=MaxEntries):
        self.dp = dp
        self.fd4, _ = dp.open_or_create_map(Proxy4MapName, MAP_TYPE_HASH, Proxy4Key.SIZE,
                                            Proxy4Value.SIZE, max_entries)
        self.fd6, _ = dp.open_or_create_map(Proxy6MapName, MAP_TYPE_HASH, Proxy6Key.SIZE,
                                            Proxy6Value.SIZE, max_entries)

    def _fd(self, key):
        return self.fd6 if key.V6 else self.fd4

    def lookup(self, key):
        """proxymap.Lookup (proxymap.go:50-71) -> Proxy4Value / Proxy6Value;
        KeyError with the reference's message when there is no entry."""
        raw = self.dp.lookup_element(self._fd(key), key.pack())
        if raw is None:
            fam = "IPv6" if key.V6 else "IPv4"
            raise KeyError(f"unable to find {fam} proxy entry for {key.String()}")
        return (Proxy6Value if key.V6 else Proxy4Value).unpack(raw)

    def delete(self, key):
        """proxymap.Delete (proxymap.go:38-47)."""
        self.dp.delete_element(self._fd(key), key.pack())

    def dump(self, v6=False):
        """[(key, value)] of one map in iteration order."""
        K, V = (Proxy6Key, Proxy6Value) if v6 else (Proxy4Key, Proxy4Value)
        k, v = self.dp.dump(self.fd6 if v6 else self.fd4)
        return [(K.unpack(k[i].tobytes()), V.unpack(v[i].tobytes())) for i in range(len(k))]

    def _gc(self, fd, vsz, tsec):
        deleted = 0
        k, v = self.dp.dump(fd)
        for i in range(len(k)):
            if struct.unpack_from("<I", v[i].tobytes(), vsz - 4)[0] < tsec:   # doGc, ipv4.go:151
                self.dp.delete_element(fd, k[i].tobytes())
                deleted += 1
        return deleted

    def gc(self, time):
        """proxymap.GC (proxymap.go:80-83): delete the entries of both maps
        whose lifetime < time -> the number deleted.  `time` is in seconds of
        the datapath clock (cfc_set_clock), what the reference derives from
        bpf.GetMtime() / 1e9.  (The reference's gc6 walks cilium_proxy4 a
        second time, ipv6.go:122-146 through doGc's Proxy4Map.GetFd(): an
        oversight; here the IPv6 map is collected.)"""
        tsec = int(time) & 0xFFFFFFFF
        return (self._gc(self.fd4, Proxy4Value.SIZE, tsec) +
                self._gc(self.fd6, Proxy6Value.SIZE, tsec))

    def flush(self):
        """proxymap.Flush (proxymap.go:86-88): gc(math.MaxUint64), whose
        uint32(time / 1e9) is 1266874889 — every entry a monotonic clock can
        have stamped."""
        return self.gc(((1 << 64) - 1) // 1000000000)

    def cleanup_on_redirect_close(self, port):
        """proxymap.CleanupOnRedirectClose (proxymap.go:75-78): remove the
        entries to proxy port `port` (host order) — TCP ones only, as
        cleanupIPv4Redirects / cleanupIPv6Redirects do (ipv4.go:188,
        ipv6.go:163) -> the number removed."""
        removed = 0
        for fd, n in ((self.fd4, 4), (self.fd6, 16)):
            for key in self.dp.keys(fd):
                dport, _, nh = struct.unpack_from("<HHB", key, n)
                if dport == _be16(port) and nh == 6:
                    self.dp.delete_element(fd, key)
                    removed += 1
        return removed


__all__ = ["ProxyMap", "Proxy4Key", "Proxy4Value", "Proxy6Key", "Proxy6Value",
           "MaxEntries", "PROXY_DEFAULT_LIFETIME"]
