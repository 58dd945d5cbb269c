// The host side of the device CT tables, once per address family (cfc_api.cpp;
// DESIGN.md §4): a family's table state (CtTab), what differs between the
// families (CtFamily<V6>), and the replay of the device's records into the
// host mirror and the CT maps (ct_replay) — host-only, no HIP call, so
// selftest.cpp can check it without a GPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "classify.hpp"
#include "flatten.hpp"
#include "maps.hpp"

namespace cfc {

using CtMaps = std::map<uint64_t, Map *>;   // ct_map_key -> map

// One family's device table and its host mirror.
template <class Slot>
struct CtTab {
    DevBuf key;    // the slots (Ct4Slot / Ct6Slot)
    DevBuf lb;     // per-slot LB state (with a load balancer)
    DevBuf ms;     // device CT apply state (ctapply.hip)
    // a device growth's remap still to apply to the mirror (mirror_sync): per
    // mirror slot its slot in the current table (NONE: dropped)
    DevBuf pend;
    // the host mirror: slot -> key as the host maps hold it (to fold the
    // accounting, patch host-side changes, take the device's records)
    std::vector<Slot> host;
    // the device table's slots (the mirror's size, once any growth's remap
    // has been applied to it)
    uint64_t slots = 0;
    uint32_t mask = 0, probe = 0;
    uint32_t n = 0;      // live entries
    uint32_t tomb = 0;   // deleted slots (CT_TOMBSTONE)
    uint64_t used() const { return (uint64_t)n + tomb; }
};

// a tuple as a slot or a device record holds it: daddr, saddr (al bytes
// each), ports, ct word
struct CtKey {
    const uint32_t *d, *s;
    uint32_t z, w;
};

template <bool V6>
struct CtFamily;
template <>
struct CtFamily<false> {
    using Slot = Ct4Slot;
    using SyncRec = CtSyncRec;
    using GcRec = CtGcRec;
    using Log = CtLog;
    using Addr = uint32_t;   // a GC address set's element (raw be32)
    static constexpr int family = 4;
    static constexpr Role role = ROLE_CT4;
    static constexpr uint32_t al = 4;
    template <class R>   // Slot, SyncRec, GcRec: x daddr, y saddr
    static CtKey key(const R &r) { return CtKey{&r.x, &r.y, r.z, r.w}; }
    static uint32_t home(const CtKey &k) { return ct_home4(*k.d, *k.s, k.z, k.w); }
    static void set_key(Slot &h, const CtKey &k) { h = Slot{*k.d, *k.s, k.z, k.w}; }
    static Slot tombstone() { return Slot{0, 0, 0, CT_TOMBSTONE}; }
    // a log record's rev_nat_index | lb_loopback << 16
    static uint32_t log_lbw(const Log &g) { return g.lbw; }
    static bool addr_less(Addr a, Addr b) { return a < b; }
};
template <>
struct CtFamily<true> {
    using Slot = Ct6Slot;
    using SyncRec = CtSyncRec6;
    using GcRec = CtGcRec6;
    using Log = CtLog6;
    using Addr = uint4;      // raw
    static constexpr int family = 6;
    static constexpr Role role = ROLE_CT6;
    static constexpr uint32_t al = 16;
    static CtKey key(const Slot &r) { return CtKey{r.d, r.s, r.z, r.w}; }
    static CtKey key(const SyncRec &r) { return CtKey{r.d, r.s, r.z, r.w}; }
    static CtKey key(const GcRec &r) { return CtKey{&r.d.x, &r.s.x, r.z, r.w}; }
    static uint32_t home(const CtKey &k) { return ct_home6(k.d, k.s, k.z, k.w); }
    static void set_key(Slot &h, const CtKey &k)
    {
        memcpy(h.d, k.d, 16);
        memcpy(h.s, k.s, 16);
        h.z = k.z;
        h.w = k.w;
    }
    static Slot tombstone()
    {
        Slot t{};
        t.w = CT_TOMBSTONE;
        return t;
    }
    // IPv6 has no loopback service address: a CtLog6 carries only the
    // rev_nat_index, and the lb_loopback bit is never set
    static uint32_t log_lbw(const Log &g) { return (uint16_t)g.rev; }
    static bool addr_less(const Addr &a, const Addr &b)
    {
        return a.x != b.x ? a.x < b.x : a.y != b.y ? a.y < b.y : a.z != b.z ? a.z < b.z
                                                                            : a.w < b.w;
    }
};

template <bool V6>
bool ct_key_eq(const CtKey &a, const CtKey &b)
{
    constexpr uint32_t al = CtFamily<V6>::al;
    return a.z == b.z && a.w == b.w && !memcmp(a.d, b.d, al) && !memcmp(a.s, b.s, al);
}

// CT map and key bytes of a device slot (the slot holds the whole tuple)
inline Map *ct_slot_key(const CtMaps &maps, int family, const CtKey &k, std::string *key)
{
    const uint32_t al = family == 4 ? 4 : 16;
    char b[38];
    memcpy(b, k.d, al);
    memcpy(b + al, k.s, al);
    memcpy(b + 2 * al, &k.z, 4);
    b[2 * al + 4] = (char)(k.w & 0xFF);
    b[2 * al + 5] = (char)((k.w >> 8) & 7);
    key->assign(b, 2 * al + 6);
    auto it = maps.find(ct_map_key(family, k.w & ~0x7FFu, (k.w & 0xFF) != 6));
    return it == maps.end() ? nullptr : it->second;
}

// struct ct_entry fields the device keeps (CtTimer, CtInfo) into a value:
// lifetime @32, bits @36 (rx/tx_closing, nat46, seen_non_syn, lb_loopback
// with a load balancer; others kept), rev_nat_index @38, slave @40 (with a load
// balancer), tx/rx_flags_seen @42/43, src_sec_id @44, last_tx/rx
// @48/52.  Rec: CtSyncRec or CtSyncRec6 (the fields both carry).
template <class Rec>
void ct_value_from_dev(std::string &v, const Rec &r, bool created)
{
    uint16_t bits = 0;
    if (!created)
        memcpy(&bits, &v[36], 2);
    bits = (uint16_t)((bits & ~(1u | 2u | 4u | 16u)) | ((r.flags >> 16) & 3) |
                      ((r.flags & CTT_NON_SYN) ? 16u : 0u) | ((r.flags & CTT_NAT46) ? 4u : 0u));
    if (r.pad >> 31) {   // the load balancer's ct_state (the table's LB words)
        bits = (uint16_t)((bits & ~8u) | (((r.pad >> 16) & 1) ? 8u : 0u));
        const uint16_t slave = (uint16_t)(r.pad & 0xFFFF);
        memcpy(&v[40], &slave, 2);
    }
    memcpy(&v[32], &r.lifetime, 4);
    memcpy(&v[36], &bits, 2);
    v[42] = (char)((r.flags >> 8) & 0xFF);
    v[43] = (char)(r.flags & 0xFF);
    memcpy(&v[48], &r.last_tx, 4);
    memcpy(&v[52], &r.last_rx, 4);
    if (created) {
        const uint16_t rev = (uint16_t)(r.info.y & 0xFFFF);
        memcpy(&v[38], &rev, 2);
        memcpy(&v[44], &r.info.sec, 4);
    }
}

// One family's device records into its host mirror and CT maps (ct_sync):
// the GC's deletes first (they precede every dirty record of their slots: a
// GC clears the slot's dirty bits), then the applies' deletes (an entry
// deleted and created again lives in another slot, created after the
// delete), then creates and updates, then the TCP maps' ICMP entries of the
// creates (log, sorted here) in batch and header order.
template <bool V6>
void ct_replay(CtTab<typename CtFamily<V6>::Slot> &T, const CtMaps &maps,
               const std::vector<typename CtFamily<V6>::GcRec> &gc,
               const std::vector<typename CtFamily<V6>::SyncRec> &rec,
               std::vector<typename CtFamily<V6>::Log> &log)
{
    using F = CtFamily<V6>;
    using Slot = typename F::Slot;
    using Log = typename F::Log;
    constexpr uint32_t al = F::al;
    std::string key;
    for (const typename F::GcRec &r : gc) {
        const CtKey k = F::key(r);
        if (Map *m = ct_slot_key(maps, F::family, k, &key))
            m->erase_raw(key);
        if (r.slot == 0xFFFFFFFFu) {   // (a growth since dropped its tombstone: ct_grow)
            T.n--;
            continue;
        }
        Slot &h = T.host[r.slot];
        if (ct_key_eq<V6>(F::key(h), k)) {
            T.n--;
            T.tomb++;
        } else if (h.w == 0) {
            T.tomb++;
        }
        h = F::tombstone();
    }
    for (int pass = 0; pass < 2; pass++) {
        for (const typename F::SyncRec &r : rec) {
            const bool del = (r.w & CT_TOMBSTONE) == CT_TOMBSTONE;
            if (del != (pass == 0))
                continue;
            CtKey k = F::key(r);
            k.w = r.w & ~CT_TOMBSTONE;
            Slot &h = T.host[r.slot];
            const bool prev_live = h.w != 0 && h.w != CT_TOMBSTONE;
            Map *m = ct_slot_key(maps, F::family, k, &key);
            if (del) {
                if (m)
                    m->erase_raw(key);
                if (prev_live) {
                    T.n--;
                    T.tomb++;
                } else if (h.w == 0) {
                    T.tomb++;
                }
                h = F::tombstone();
            } else if (r.info.y & CTI_CREATED) {
                if (m) {
                    std::string v(m->value_bytes(), '\0');
                    ct_value_from_dev(v, r, true);
                    m->put_raw(key, v);
                }
                if (!prev_live) {
                    T.n++;
                    if (h.w == CT_TOMBSTONE)
                        T.tomb--;
                }
                F::set_key(h, k);
            } else if (m) {
                auto it = m->kv.find(key);
                if (it != m->kv.end() && it->second.val.size() >= 56)
                    ct_value_from_dev(it->second.val, r, false);
            }
        }
    }
    std::sort(log.begin(), log.end(), [](const Log &a, const Log &b) {
        return a.seq != b.seq ? a.seq < b.seq : a.order < b.order;
    });
    for (const Log &g : log) {
        // ct_create4's / ct_create6's second write into the TCP map
        // (conntrack.h:741-760, 648-660)
        auto it = maps.find(ct_map_key(F::family, g.w & ~0x7FFu, 0));
        if (it == maps.end())
            continue;
        char k[2 * al + 6];
        const uint32_t z = 0;
        memcpy(k, &g.x, al);
        memcpy(k + al, &g.y, al);
        memcpy(k + 2 * al, &z, 4);
        k[2 * al + 4] = (char)(g.w & 0xFF);
        k[2 * al + 5] = (char)((g.w >> 8) & 7);
        std::string v(it->second->value_bytes(), '\0');
        const uint32_t dir = g.dirlen >> 31;
        const uint64_t one = 1, len = g.dirlen & (CTLOG_NAT46 - 1);
        memcpy(&v[dir ? 0 : 16], &one, 8);
        memcpy(&v[dir ? 8 : 24], &len, 8);
        const uint32_t life = g.now + 60, last = 5u < g.now ? g.now : 0u;
        // seen_non_syn ("for ICMP, there is no SYN"), a load balancer's
        // ct_state (lb_loopback: IPv4 only, CtFamily::log_lbw), nat46
        const uint32_t lbw = F::log_lbw(g);
        const uint16_t bits = (uint16_t)(16u | (((lbw >> 16) & 1) ? 8u : 0u) |
                                         ((g.dirlen & CTLOG_NAT46) ? 4u : 0u));
        const uint16_t rev = (uint16_t)(lbw & 0xFFFF), slave = (uint16_t)g.slave;
        memcpy(&v[32], &life, 4);
        memcpy(&v[36], &bits, 2);
        memcpy(&v[38], &rev, 2);
        memcpy(&v[40], &slave, 2);
        memcpy(&v[44], &g.sec, 4);
        memcpy(&v[dir ? 52 : 48], &last, 4);
        it->second->put_raw(std::string(k, sizeof(k)), v);
    }
}

}  // namespace cfc
