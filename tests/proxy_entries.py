"""The cilium_proxy4 / cilium_proxy6 entries a batch leaves, restated from
the reference: ipv{4,6}_redirect_to_host_port (bpf/lib/lxc.h:96-191) at its
four call sites (bpf_lxc.c:280, 585 egress; :858, :989 the policy programs).

Inputs are the oracle's outputs for the batch — Oracle.classify(...,
want_ct=True, apply_ct=True, want_pkt=True): verdict, identity, CT byte and
the packet as the programs left it — plus the headers, the sender's SECLABEL
and the clock.  One packet at a time, as the reference: every redirected
packet does map_update_elem(&cilium_proxy4, &key, &value, BPF_ANY), so a key
keeps its last writer's value.

  key   = {saddr = tuple->daddr, dport = new_port, sport = tuple->sport,
           nexthdr}                        (struct proxy4_tbl_key, common.h:478)
  value = {orig_daddr = old_ip, orig_dport = old_port (tuple.dport), pad,
           identity, lifetime = now + PROXY_DEFAULT_LIFETIME}        (:486)

ct_lookup4/6 (conntrack.h:467-590, 310-437) loads the first L4 word into
{tuple->dport, tuple->sport} — dport = the packet's source port — and calls
ipv{4,6}_ct_tuple_reverse only after the first lookup missed: a CT_REPLY /
CT_RELATED packet keeps the tuple as loaded, CT_NEW / CT_ESTABLISHED has it
reversed (addresses and ports swapped)."""
import struct

import numpy as np

PROXY_DEFAULT_LIFETIME = 720   # common.h:466
CT_NEW, CT_ESTABLISHED, CT_REPLY, CT_RELATED = 0, 1, 2, 3
CT_DONE = 4


def _icmp_ports(v6, icmp_type):
    """tuple->dport, ->sport ct_lookup sets for an ICMP type, and whether it
    set TUPLE_F_RELATED (conntrack.h:339-372, 496-526)"""
    related = (1, 2, 3, 4) if v6 else (3, 11, 12)
    echo, reply = (128, 129) if v6 else (8, 0)
    if icmp_type in related:
        return 0, 0
    if icmp_type == reply:
        return echo, 0
    if icmp_type == echo:
        return 0, echo
    return 0, 0


def _addr(a, v6):
    return bytes(np.asarray(a, np.uint8)) if v6 else struct.pack("<I", int(a))


def _pkt_row(pkt, i, v6):
    """(saddr bytes, daddr bytes, sport raw, dport raw) of the packet as left"""
    r = np.asarray(pkt[i], np.uint32)
    if v6:
        sa, da, w = r[0:4].tobytes(), r[4:8].tobytes(), int(r[8])
    else:
        sa, da, w = struct.pack("<I", int(r[0])), struct.pack("<I", int(r[1])), int(r[2])
    return sa, da, w & 0xFFFF, w >> 16


def entry_of(h, i, mode, verdict, identity, ct, pkt=None, seclabel=0, now=0):
    """The map_update_elem of redirected header i -> (key bytes, value bytes,
    the redirecting stage's CT result, 1 if that was the destination's stage,
    1 if the service step had rewritten the destination)."""
    v6 = h.family == 6
    egress = mode == 1
    translated = 0
    ctb = int(ct[i]) if ct is not None else 0
    proto = int(h.proto[i])
    # the packet the redirecting stage's ct_lookup saw
    sa, da = _addr(h.saddr[i], v6), _addr(h.daddr[i], v6)
    sp, dp = int(h.sport[i]), int(h.dport[i])
    dest = egress and bool((ctb >> 4) & CT_DONE)
    res = ((ctb >> 4) if dest else ctb) & 3
    reversed_ = res in (CT_NEW, CT_ESTABLISHED)
    if egress and pkt is not None:
        psa, pda, psp, pdp = _pkt_row(pkt, i, v6)
        if dest:
            # the destination's ipv{4,6}_policy after local delivery: the
            # packet as the egress program left it.  IPv6: ipv6_policy itself
            # clears the destination's reverse-NAT bits after it copied
            # orig_dip (bpf_lxc.c:775-795) and may reverse-NAT the source
            # (:814-821), lb6_local never touches the source
            if v6:
                # (dip.p4 &= ~0xFFFF: bytes 12 and 13)
                if pda[:12] + pda[14:] != da[:12] + da[14:]:
                    da = pda
            else:
                sa, da = psa, pda
            sp, dp = psp, pdp
        else:
            # the egress program: ct_lookup runs behind the service step
            # (lb4_local / lb6_local rewrote tuple->daddr and the destination
            # port, bpf_lxc.c:166-181, 486-501) and before lb4_rev_nat /
            # lb6_rev_nat of a reply (:568-575), which rewrites the packet's
            # source only.  A flow looped back into its sender keeps
            # tuple->daddr (lb.h:761-770)
            dp = pdp
            if v6:
                da = pda
            else:
                looped = reversed_ and psa != sa
                revnat = (not reversed_) and (psa != sa or psp != sp)
                if not looped and not revnat:
                    da = pda
            if da != _addr(h.daddr[i], v6) or dp != int(h.dport[i]):
                translated = 1
    if proto in (6, 17):
        t_dport, t_sport = sp, dp            # the 4-byte load at &tuple->dport
    else:
        t_dport, t_sport = _icmp_ports(v6, sp & 0xFF)
    t_daddr, t_saddr = da, sa
    orig_dip = da                            # bpf_lxc.c:181, 501, 775, 925
    if reversed_:
        t_daddr, t_saddr = t_saddr, t_daddr
        t_dport, t_sport = t_sport, t_dport
    ident = int(seclabel) if egress else int(identity[i])
    key = t_daddr + struct.pack("<HHBB", int(verdict[i]) & 0xFFFF, t_sport, proto, 0)
    val = orig_dip + struct.pack("<HHII", t_dport, 0, ident & 0xFFFFFFFF,
                                 (int(now) + PROXY_DEFAULT_LIFETIME) & 0xFFFFFFFF)
    return key, val, res, int(dest), translated


def expected_entries(h, mode, verdict, identity, ct, pkt=None, seclabel=0, now=0):
    """-> (records (m, 32) u8 in the cfc_proxy4_entry layout — (m, 64),
    cfc_proxy6_entry —, last writers' header indices (m,) u64, stats dict
    {redirects, rewrites, by state}) in the order of the last writers."""
    v6 = h.family == 6
    entries = {}     # key bytes -> (value bytes, header index)
    redirects = rewrites = dest_stage = translated = 0
    states = [0, 0, 0, 0]
    for i in np.flatnonzero(np.asarray(verdict) > 0):
        i = int(i)
        key, val, res, dest, tr = entry_of(h, i, mode, verdict, identity, ct, pkt, seclabel, now)
        redirects += 1
        states[res] += 1
        dest_stage += dest
        translated += tr
        if key in entries:
            rewrites += 1
            del entries[key]                     # keep insertion order = last writer's
        entries[key] = (val, i)
    rsz = 64 if v6 else 32
    rec = np.zeros((len(entries), rsz), np.uint8)
    idx = np.zeros(len(entries), np.uint64)
    for k, (key, (val, i)) in enumerate(entries.items()):
        rec[k, :len(key)] = np.frombuffer(key, np.uint8)
        rec[k, rsz // 2:rsz // 2 + len(val)] = np.frombuffer(val, np.uint8)
        idx[k] = i
    stats = dict(redirects=redirects, rewrites=rewrites, new=states[0], established=states[1],
                 reply=states[2], related=states[3], dest_stage=dest_stage,
                 translated=translated)
    return rec, idx, stats


def map_rows(rec):
    """records -> {key bytes: value bytes} as the map would hold them"""
    v6 = rec.shape[1] == 64
    ks, vo, vs = (22, 32, 28) if v6 else (10, 16, 16)
    return {bytes(r[:ks]): bytes(r[vo:vo + vs]) for r in rec}
