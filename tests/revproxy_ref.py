"""reverse_proxy / reverse_proxy6 and the from-host source identity, restated
in plain Python from the reference's lines (bpf/bpf_netdev.c of the modelled
tree; nothing here is run against the reference's own harness — the oracle
is not extended, so cfc_classify_from_host_* rests on this restatement and on
the existing oracle for everything behind the rewrite).

  handle_identity_from_host  bpf_netdev.c:128-153
      magic = mark & MARK_MAGIC_HOST_MASK (0xF00)
      0xA00 MARK_MAGIC_PROXY_INGRESS: identity via proxy, TC_INDEX_F_SKIP_PROXY
      0xB00 MARK_MAGIC_PROXY_EGRESS:  identity via proxy
      0xC00 MARK_MAGIC_HOST:          HOST_ID
      else                            WORLD_ID
      get_identity_via_proxy: (mark & 0xFF) << 16 | mark >> 16
  handle_ipv4  :375-398  a reserved identity takes the ipcache label of the
      source unless the label is 0, CLUSTER_ID or HOST_ID; then :400-416
      reverse_proxy on the packet
  handle_ipv6  :203-213  the same, the label ignored only when 0 or
      CLUSTER_ID; then :218-234 reverse_proxy6 with ip6->nexthdr
  reverse_proxy  :293-354 / reverse_proxy6 :67-124
      only IPPROTO_TCP and IPPROTO_UDP; key = {saddr = ip->daddr, the first
      four L4 bytes loaded at key.dport (so dport = the packet's source port,
      sport = its destination port), nexthdr, pad 0}; on a hit the source
      address becomes orig_daddr, the source port orig_dport, and
      TC_INDEX_F_SKIP_PROXY is set.  `lifetime` is not read.

The identity is settled BEFORE the rewrite, from the original source.  The
datapath's translated header carries the mark 0xA00 | CFC_MARK_TRANSLATED
(bit 12) and the identity in a column of its own; towards the existing
oracle a hit row is expressed as mark 0xA00 | enc(identity), which makes its
handle_identity_from_host return that identity with skip-proxy set (24 bits:
an identity above 2^24 cannot be expressed that way).
"""
import dataclasses

import numpy as np

from cilium_amd import synth as S

MARK_TRANSLATED = 0x1000
MARK_HIT = 0xA00 | MARK_TRANSLATED
HEALTH_ID = 4    # identity_is_reserved(): below it (HOST, WORLD, CLUSTER; 0)


def enc(ident):
    """the via-proxy mark bits of a 24-bit identity (the inverse of
    get_identity_via_proxy)"""
    ident = int(ident)
    assert 0 <= ident < 1 << 24
    return ((ident >> 16) & 0xFF) | ((ident & 0xFFFF) << 16)


def identity_from_mark(mark):
    """handle_identity_from_host -> (identity, skip_proxy)"""
    mark = int(mark) & 0xFFFFFFFF
    magic = mark & 0xF00
    if magic in (0xA00, 0xB00):
        return ((mark & 0xFF) << 16) | (mark >> 16), magic == 0xA00
    return (S.HOST_ID if magic == 0xC00 else S.WORLD_ID), False


def source_identity(family, mark, label):
    """the src_identity handle_ipv4 / handle_ipv6 pass on: `label` is the
    ipcache's sec_label of the packet's source (0: no entry, or label 0)"""
    ident, _ = identity_from_mark(mark)
    label = int(label)
    if ident < HEALTH_ID and label and label != S.CLUSTER_ID:
        if family == 6 or label != S.HOST_ID:
            ident = label
    return ident


def key_of(family, daddr, l4word, nexthdr):
    """struct proxy{4,6}_tbl_key of a packet: daddr raw bytes, the first L4
    word as loaded (sport | dport << 16 of the header batch), nexthdr, pad 0"""
    a = bytes(np.asarray(daddr, np.uint32).reshape(1).view(np.uint8)) if family == 4 \
        else bytes(np.asarray(daddr, np.uint8))
    return a + int(l4word).to_bytes(4, "little") + bytes([int(nexthdr), 0])


@dataclasses.dataclass
class Translation:
    hit: np.ndarray        # bool
    saddr: np.ndarray      # as Headers.saddr
    l4word: np.ndarray     # u32: sport | dport << 16
    mark: np.ndarray       # u32: the datapath's mark column (MARK_HIT on hits)
    identity: np.ndarray   # u32: final source identity (hit rows; 0 elsewhere)

    def headers(self, h, oracle_marks=True):
        """the translated batch as S.Headers; oracle_marks: the hit rows'
        mark as 0xA00 | enc(identity) (what the existing oracle understands)"""
        mark = self.mark.copy()
        if oracle_marks:
            for i in np.flatnonzero(self.hit):
                mark[i] = 0xA00 | enc(self.identity[i])
        return dataclasses.replace(h, saddr=self.saddr.copy(),
                                   sport=(self.l4word & 0xFFFF).astype(np.uint16),
                                   dport=(self.l4word >> 16).astype(np.uint16), mark=mark)


def translate(h, entries, labels):
    """reverse_proxy over a from-host batch.
    h: S.Headers; entries: {key bytes: value bytes} of the family's proxy map
    (struct proxy{4,6}_tbl_key / _value, as Datapath.dump gives them);
    labels: the ipcache sec_label of every header's ORIGINAL source (u32, 0 =
    none; Oracle.ipcache_lookup)."""
    n = len(h)
    fam = h.family
    al = 4 if fam == 4 else 16
    word = h.sport.astype(np.uint32) | (h.dport.astype(np.uint32) << 16)
    mark_in = np.zeros(n, np.uint32) if h.mark is None else np.asarray(h.mark, np.uint32)
    t = Translation(np.zeros(n, bool), h.saddr.copy(), word.copy(), mark_in.copy(),
                    np.zeros(n, np.uint32))
    for i in range(n):
        nh = int(h.proto[i])
        if nh not in (6, 17):              # "default: ignore"
            continue
        if fam == 6 and int(h.flags[i]) & S.HF_EXTHDR:
            continue                       # ip6->nexthdr is the extension header
        v = entries.get(key_of(fam, h.daddr[i], word[i], nh))
        if v is None:
            continue
        t.hit[i] = True
        if fam == 4:
            t.saddr[i] = np.frombuffer(v[:4], "<u4")[0]
        else:
            t.saddr[i] = np.frombuffer(v[:16], np.uint8)
        orig_dport = int.from_bytes(v[al:al + 2], "little")
        t.l4word[i] = (int(word[i]) & 0xFFFF0000) | orig_dport
        t.mark[i] = MARK_HIT
        t.identity[i] = source_identity(fam, mark_in[i], labels[i])
    return t


def entry(family, saddr, sport, dport, nexthdr, orig_daddr, orig_dport, identity=0,
          lifetime=0):
    """one map entry -> (key bytes, value bytes); addresses as raw bytes,
    ports raw be16 (as the header batch holds them): sport / dport are the
    KEY's fields (sport = the client's port, dport = the proxy's)"""
    k = bytes(saddr) + int(dport).to_bytes(2, "little") + int(sport).to_bytes(2, "little") + \
        bytes([int(nexthdr), 0])
    v = bytes(orig_daddr) + int(orig_dport).to_bytes(2, "little") + b"\0\0" + \
        int(identity).to_bytes(4, "little") + int(lifetime).to_bytes(4, "little")
    assert len(k) == (10 if family == 4 else 22) and len(v) == (16 if family == 4 else 28)
    return k, v
