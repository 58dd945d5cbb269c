// Host self-test of the IPv6 LPM flattener (flatten.cpp build_lpm6): the
// lookup the device performs (lpm6_lookup_host restates k_classify_v6's
// lpm6_lookup over the same image) against a brute-force longest-prefix
// match, on prefix sets that exercise the Bloom grouping: random C3-like
// sets, prefixes piled under one /48 or /64 (groups must split), a ::/0,
// and label-0 prefixes that shadow shorter ones.  No GPU needed.
#include <cstdio>
#include <cerrno>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "classify.hpp"
#include "flatten.hpp"
#include "maps.hpp"
#include "selfcut.hpp"
#include "ctmirror.hpp"

using namespace cfc;

// ---- the replay of the device's CT records into the host mirror and the CT
// maps (ctmirror.hpp ct_replay), per family: a 16-slot mirror, the global
// TCP and ANY maps, hand-written records
template <bool V6>
struct ReplayCase {
    using F = CtFamily<V6>;
    using Rec = typename F::SyncRec;
    CtTab<typename F::Slot> T;
    Map tcp, any;
    CtMaps maps;
    int fail = 0;
    ReplayCase()
    {
        T.host.resize(16);
        T.slots = 16;
        T.mask = 15;
        for (Map *m : {&tcp, &any}) {
            m->role = F::role;
            m->type = MT_HASH;
            m->ksz = 2 * F::al + 6;
            m->vsz = 56;
            m->max_entries = 64;
        }
        any.ct_any = 1;
        maps[ct_map_key(F::family, 0, 0)] = &tcp;
        maps[ct_map_key(F::family, 0, 1)] = &any;
    }
    // address a of a test tuple: one word (IPv4), four (IPv6)
    static void addr(uint32_t a, uint32_t out[4])
    {
        for (int i = 0; i < 4; i++)
            out[i] = a + 0x01010101u * (uint32_t)i;
    }
    // the map key of tuple (d, s, z, nexthdr, flags), written out by hand
    static std::string mapkey(uint32_t d, uint32_t s, uint32_t z, uint8_t nh, uint8_t fl)
    {
        uint32_t da[4], sa[4];
        addr(d, da);
        addr(s, sa);
        std::string k((const char *)da, F::al);
        k.append((const char *)sa, F::al);
        k.append((const char *)&z, 4);
        k.push_back((char)nh);
        k.push_back((char)fl);
        return k;
    }
    template <class R>   // a sync or GC record's key fields
    static void setkey(R &r, uint32_t d, uint32_t s, uint32_t z, uint32_t w)
    {
        uint32_t da[4], sa[4];
        addr(d, da);
        addr(s, sa);
        if constexpr (V6) {
            memcpy(&r.d, da, 16);
            memcpy(&r.s, sa, 16);
        } else {
            r.x = da[0];
            r.y = sa[0];
        }
        r.z = z;
        r.w = w;
    }
    static Rec rec(uint32_t slot, uint32_t d, uint32_t s, uint32_t z, uint32_t w, uint32_t dirty,
                   uint32_t rev, uint32_t sec)
    {
        Rec r{};
        r.slot = slot;
        setkey(r, d, s, z, w);
        r.info.sec = sec;
        r.info.y = rev | dirty;
        return r;
    }
    static typename F::Log logrec(uint32_t sa, uint32_t da, uint32_t seq, uint32_t order,
                                  uint32_t sec)
    {
        typename F::Log g{};
        uint32_t a[4];
        addr(sa, a);
        memcpy(&g.x, a, F::al);
        addr(da, a);
        memcpy(&g.y, a, F::al);
        g.w = ct_word(V6 ? 58 : 1, 0, 0);
        g.now = 1000;
        g.dirlen = 1u << 31 | 84;
        g.seq = seq;
        g.order = order;
        g.sec = sec;
        return g;
    }
    void replay(const std::vector<typename F::GcRec> &gc, const std::vector<Rec> &rs,
                std::vector<typename F::Log> lg = {})
    {
        ct_replay<V6>(T, maps, gc, rs, lg);
    }
    template <class V>
    static V at(const std::string &v, size_t off)
    {
        V x;
        memcpy(&x, &v[off], sizeof(V));
        return x;
    }
    void expect(bool ok, const char *what)
    {
        if (!ok) {
            printf("ct_replay v%d %s FAIL (n %u, tomb %u)\n", F::family, what, T.n, T.tomb);
            fail = 1;
        }
    }
    int run()
    {
        const uint32_t W = ct_word(6, 1, 0), Z = 0x00500400u;
        const std::string K = mapkey(10, 20, Z, 6, 1);
        // create: every field ct_value_from_dev writes
        Rec c = rec(3, 10, 20, Z, W, CTI_CREATED, 7, 0x1234);
        c.last_rx = 11;
        c.last_tx = 12;
        c.flags = 2u << 16 | CTT_NON_SYN | 0xAB << 8 | 0xCD;
        c.lifetime = 1060;
        replay({}, {c});
        const std::string *v = tcp.kv.count(K) ? &tcp.kv[K].val : nullptr;
        expect(v && v->size() == 56 && any.kv.empty() && T.n == 1 && T.tomb == 0, "create");
        expect(v && at<uint32_t>(*v, 32) == 1060 && at<uint16_t>(*v, 36) == (2 | 16) &&
                   at<uint16_t>(*v, 38) == 7 && at<uint16_t>(*v, 40) == 0 &&
                   (uint8_t)(*v)[42] == 0xAB && (uint8_t)(*v)[43] == 0xCD &&
                   at<uint32_t>(*v, 44) == 0x1234 && at<uint32_t>(*v, 48) == 12 &&
                   at<uint32_t>(*v, 52) == 11,
               "create value");
        expect(ct_key_eq<V6>(F::key(T.host[3]), F::key(c)), "create mirror");
        // update: rev_nat_index and src_sec_id stay; then the LB state in pad
        Rec u = rec(3, 10, 20, Z, W, CTI_UPDATED, 99, 0x9999);
        u.flags = 1u << 16 | CTT_NAT46;
        u.lifetime = 2000;
        replay({}, {u});
        v = &tcp.kv[K].val;
        expect(at<uint32_t>(*v, 32) == 2000 && at<uint16_t>(*v, 36) == (1 | 4) &&
                   at<uint16_t>(*v, 38) == 7 && at<uint32_t>(*v, 44) == 0x1234 && T.n == 1,
               "update");
        u.pad = 1u << 31 | 1u << 16 | 0x55;
        replay({}, {u});
        expect(at<uint16_t>(*v, 36) == (1 | 4 | 8) && at<uint16_t>(*v, 40) == 0x55, "update lb");
        // deleted and created again in another slot, the create listed first
        Rec d = rec(3, 10, 20, Z, W | CT_TOMBSTONE, CTI_DELETED, 0, 0);
        Rec c2 = rec(5, 10, 20, Z, W, CTI_CREATED, 8, 0x4321);
        replay({}, {c2, d});
        expect(tcp.kv.count(K) && at<uint16_t>(tcp.kv[K].val, 38) == 8 && T.n == 1 &&
                   T.tomb == 1 && T.host[3].w == CT_TOMBSTONE &&
                   ct_key_eq<V6>(F::key(T.host[5]), F::key(c2)),
               "delete, re-create");
        // GC records: one that matches the mirror's slot
        typename F::GcRec g{};
        g.slot = 5;
        setkey(g, 10, 20, Z, W);
        replay({g}, {});
        expect(!tcp.kv.count(K) && T.n == 0 && T.tomb == 2 && T.host[5].w == CT_TOMBSTONE,
               "gc match");
        // one whose slot holds another key since, one whose slot is free,
        // one a growth dropped (NONE): the map entry goes every time
        const uint32_t WU = ct_word(17, 0, 0);
        replay({}, {rec(7, 30, 40, Z, WU, CTI_CREATED, 0, 1), rec(8, 31, 41, Z, WU, CTI_CREATED, 0, 1),
                    rec(9, 32, 42, Z, WU, CTI_CREATED, 0, 1)});
        expect(any.kv.size() == 3 && T.n == 3 && T.tomb == 2, "gc setup");
        g.slot = 7;
        setkey(g, 31, 41, Z, WU);
        replay({g}, {});
        expect(any.kv.size() == 2 && !any.kv.count(mapkey(31, 41, Z, 17, 0)) && T.n == 3 &&
                   T.tomb == 2 && T.host[7].w == CT_TOMBSTONE,
               "gc other key");
        g.slot = 12;
        setkey(g, 32, 42, Z, WU);
        replay({g}, {});
        expect(any.kv.size() == 1 && T.n == 3 && T.tomb == 3 && T.host[12].w == CT_TOMBSTONE,
               "gc free slot");
        g.slot = 0xFFFFFFFFu;
        setkey(g, 30, 40, Z, WU);
        replay({g}, {});
        expect(any.kv.empty() && T.n == 2 && T.tomb == 3, "gc dropped slot");
        // the log out of (seq, order) order: the latest record's value stays
        const std::string KL = mapkey(50, 60, 0, V6 ? 58 : 1, 0);
        replay({}, {}, {logrec(50, 60, 2, 1, 333), logrec(50, 60, 2, 0, 222),
                        logrec(50, 60, 1, 5, 111)});
        v = tcp.kv.count(KL) ? &tcp.kv[KL].val : nullptr;
        expect(v && tcp.kv.size() == 1 && at<uint32_t>(*v, 44) == 333 &&
                   at<uint64_t>(*v, 0) == 1 && at<uint64_t>(*v, 8) == 84 &&
                   at<uint32_t>(*v, 32) == 1060 && at<uint16_t>(*v, 36) == 16 &&
                   at<uint32_t>(*v, 52) == 1000,
               "log order");
        // the lb_loopback bit: an IPv4 record carries it, an IPv6 one cannot
        typename F::Log lo = logrec(51, 61, 3, 0, 1);
        if constexpr (V6)
            lo.rev = 9;
        else
            lo.lbw = 9 | 1u << 16;
        lo.slave = 4;
        replay({}, {}, {lo});
        v = &tcp.kv[mapkey(51, 61, 0, V6 ? 58 : 1, 0)].val;
        expect(v->size() == 56 && at<uint16_t>(*v, 36) == (V6 ? 16 : 16 | 8) &&
                   at<uint16_t>(*v, 38) == 9 && at<uint16_t>(*v, 40) == 4,
               "log loopback");
        printf("ct_replay v%d %s\n", F::family, fail ? "FAIL" : "ok");
        return fail;
    }
};

// the cut rule of an egress batch with traffic to itself (selfcut.hpp)
struct Row {
    uint32_t x, y, z, w;   // header index, L4 word, meta, address matched
};
static uint32_t ports(uint32_t sp, uint32_t dp) { return sp | dp << 16; }
static int cuts_case(const char *name, const std::vector<Row> &rows, bool v6,
                     const std::vector<uint64_t> &want)
{
    std::vector<uint64_t> got;
    self_cut_rule(rows, 1, v6, &got);   // (address 0 the endpoint's own, 1 a loopback one)
    const bool ok = got == want;
    printf("selfcut %-24s %s (%zu cuts)\n", name, ok ? "ok" : "FAIL", got.size());
    return ok ? 0 : 1;
}
static int selfcut_tests()
{
    const uint32_t TCP = 6, UDP = 17, ICMP = 1, ICMP6 = 58;
    int fail = 0;
    // an opening packet and its answer (ports swapped): cut at the answer
    fail |= cuts_case("tcp-answer", {{3, ports(1000, 80), TCP, 0}, {9, ports(80, 1000), TCP, 0}},
                      false, {9});
    // a second packet of the same direction: also cut (conservative)
    fail |= cuts_case("tcp-same-dir", {{3, ports(1000, 80), TCP, 0}, {5, ports(1000, 80), TCP, 0}},
                      false, {5});
    // two flows on other ports, or another protocol: one segment
    fail |= cuts_case("tcp-unrelated", {{3, ports(1000, 80), TCP, 0}, {4, ports(1001, 80), TCP, 0},
                                        {6, ports(80, 1000), UDP, 0}}, false, {});
    // an ICMP error after anything: cut; echo after echo: cut; TCP after echo: none
    fail |= cuts_case("icmp-error", {{1, ports(1000, 80), TCP, 0}, {2, 3, ICMP, 0}}, false, {2});
    fail |= cuts_case("icmp-echo", {{1, 8, ICMP, 0}, {2, ports(1000, 80), TCP, 0}, {7, 0, ICMP, 0}},
                      false, {7});
    fail |= cuts_case("icmp6-error", {{1, ports(1000, 80), UDP, 0}, {2, 1, ICMP6, 0}}, true, {2});
    // (IPv4 type 1 is no error: an ICMPv4 "other" after a TCP flow, none)
    fail |= cuts_case("icmp4-type1", {{1, ports(1000, 80), TCP, 0}, {2, 1, ICMP, 0}}, false, {});
    // a loopback address on either side: cut
    fail |= cuts_case("loopback", {{1, ports(1000, 80), TCP, 1}, {2, ports(2000, 90), TCP, 0},
                                   {3, ports(3000, 90), TCP, 1}}, false, {2, 3});
    // a cut starts a new segment: a key of the segment before no longer counts
    fail |= cuts_case("reset", {{1, ports(1000, 80), TCP, 0}, {2, ports(80, 1000), TCP, 0},
                                {3, ports(2000, 80), TCP, 0}, {4, ports(1000, 80), TCP, 0}},
                      false, {2, 4});
    fail |= cuts_case("one-header", {{5, ports(1000, 80), TCP, 0}}, false, {});
    return fail;
}

// `kat selfcut`: a fixed pseudo-random row list per family and the cuts the
// rule gives, for the restatement in tests/self_edges.py (cut_rule).  Lines
// `selfcut family <v6> <n_own>`, `selfcut row <x> <y> <z> <w>`, `selfcut cut
// <x>`, decimal.  Few ports, so keys collide; bits above the protocol byte
// of the meta word and above the type byte of an ICMP L4 word are noise the
// rule must mask; two own addresses (w 0, 1) and two loopback ones (2, 3).
static void selfcut_kats()
{
    uint32_t s = 0x5e1fc075u;
    auto lcg = [&s]() -> uint32_t {
        s = s * 1664525u + 1013904223u;
        return s >> 8;
    };
    const uint32_t PORTS[] = {1000, 1001, 80, 53, 0xE803, 0x5000};
    const uint32_t TYPES4[] = {0, 8, 3, 11, 12, 13, 1, 4, 5};
    const uint32_t TYPES6[] = {128, 129, 1, 2, 3, 4, 133, 135, 0, 5};
    for (int v6 = 0; v6 < 2; v6++) {
        const uint32_t n_own = 2;
        std::vector<Row> rows;
        uint32_t x = lcg() % 3;
        for (int i = 0; i < 400; i++, x += 1 + lcg() % 3) {
            const uint32_t sel = lcg() % 16;
            const uint32_t proto = sel < 7 ? 6 : sel < 11 ? 17 : sel < 15 ? (v6 ? 58 : 1) : 47;
            uint32_t pt = PORTS[lcg() % 6] | PORTS[lcg() % 6] << 16;
            if (proto == 1)
                pt = TYPES4[lcg() % 9] | lcg() << 8;
            else if (proto == 58)
                pt = TYPES6[lcg() % 10] | lcg() << 8;
            uint32_t w = lcg() % 48;
            w = w < 4 ? w : w & 1;
            rows.push_back({x, pt, proto | lcg() << 8, w});
        }
        std::vector<uint64_t> cuts;
        self_cut_rule(rows, n_own, v6 != 0, &cuts);
        printf("selfcut family %d %u\n", v6, n_own);
        for (const Row &r : rows)
            printf("selfcut row %u %u %u %u\n", r.x, r.y, r.z, r.w);
        for (uint64_t c : cuts)
            printf("selfcut cut %llu\n", (unsigned long long)c);
    }
}

// `kat svchash`: LCG-drawn CT key words (d, s, z, w) of both families with
// their layout.h fingerprint (ct_hash4 / ct_hash6: what svcorder.hip groups
// its list by) and home slot (ct_home4 / ct_home6: what ctapply.hip k_cta_svc
// groups by), for the restatement in tests/svc_edges.py.  Lines `svchash 4
// <d> <s> <z> <w> <hash> <home>` and `svchash 6 <d0..d3> <s0..s3> <z> <w>
// <hash> <home>`, hex.  Every fourth row repeats the one before it with the
// two addresses and the two ports exchanged and the direction bit of w
// flipped: the same home, another fingerprint.
static void svchash_kats()
{
    uint32_t s = 0x51c0a7e5u;
    auto lcg = [&s]() -> uint32_t {
        s = s * 1664525u + 1013904223u;
        return s >> 8;
    };
    auto word = [&lcg]() -> uint32_t { return lcg() << 16 ^ lcg(); };
    const uint32_t PROTO[] = {6, 17, 1, 58};
    uint32_t d[4] = {0, 0, 0, 0}, a[4] = {0, 0, 0, 0}, z = 0, w = 0;
    for (int v6 = 0; v6 < 2; v6++)
        for (int i = 0; i < 200; i++) {
            if (i % 4 == 3) {
                for (int k = 0; k < 4; k++)
                    std::swap(d[k], a[k]);
                z = z >> 16 | z << 16;
                w ^= 0x100u;
            } else {
                for (int k = 0; k < 4; k++) {
                    d[k] = word();
                    a[k] = word();
                }
                z = i % 5 == 0 ? word() & 0xFFFFu : word();
                w = ct_word(PROTO[lcg() % 4], lcg() % 8,
                            lcg() % 2 ? ct_owner_word(lcg() & 0xFFFFu, true) : 0u);
            }
            if (v6)
                printf("svchash 6 %x %x %x %x %x %x %x %x %x %x %x %x\n", d[0], d[1], d[2], d[3],
                       a[0], a[1], a[2], a[3], z, w, ct_hash6(d, a, z, w), ct_home6(d, a, z, w));
            else
                printf("svchash 4 %x %x %x %x %x %x\n", d[0], a[0], z, w,
                       ct_hash4(d[0], a[0], z, w), ct_home4(d[0], a[0], z, w));
        }
}

static uint32_t brute(const std::vector<Pfx6> &pfx, const uint32_t w[4])
{
    int best = -1;
    uint32_t label = 0;
    for (const Pfx6 &p : pfx) {
        bool ok = true;
        for (int i = 0; i < 4 && ok; i++)
            ok = (w[i] & l6_word_mask(p.plen, i)) == p.w[i];
        if (ok && (int)p.plen > best) {
            best = p.plen;
            label = p.label;
        }
    }
    return label;
}

static void add(std::vector<Pfx6> &v, const uint32_t a[4], int len, uint32_t label)
{
    Pfx6 p;
    p.plen = (uint8_t)len;
    p.label = label;
    for (int i = 0; i < 4; i++)
        p.w[i] = a[i] & l6_word_mask(len, i);
    for (const Pfx6 &q : v)
        if (q.plen == p.plen && !memcmp(q.w, p.w, 16))
            return;   // unique (prefix, length) like the map
    v.push_back(p);
}

template <class R>
static int run(const char *name, const std::vector<Pfx6> &pfx, R &rng,
               int queries)
{
    Lpm6Host t;
    build_lpm6(pfx, &t);
    int bad = 0;
    for (int q = 0; q < queries; q++) {
        uint32_t w[4];
        for (int i = 0; i < 4; i++)
            w[i] = rng();
        if (!pfx.empty() && (q & 3)) {   // mostly inside some prefix
            const Pfx6 &p = pfx[rng() % pfx.size()];
            for (int i = 0; i < 4; i++)
                w[i] = p.w[i] | (w[i] & ~l6_word_mask(p.plen, i));
        }
        const uint32_t a = lpm6_lookup_host(t, w), b = brute(pfx, w);
        if (a != b && bad++ < 5)
            printf("%s: %08x:%08x:%08x:%08x -> %u, want %u\n", name, w[0], w[1],
                   w[2], w[3], a, b);
    }
    printf("%-12s prefixes %5zu lengths %3zu groups %3u bloom %6zu slots %6zu: %s\n",
           name, pfx.size(), t.lens.size(), t.groups, t.bloom.size(), t.slots.size(),
           bad ? "FAIL" : "ok");
    return bad != 0;
}

// test/bpf/unit-test.c test_ipv6_addr_clear_suffix: the words an all-ones
// address keeps under a prefix length (ipv6_addr_clear_suffix, ipv6.h:136-150),
// here as l6_word_mask (layout.h), which builds and probes the IPv6 LPM
static int clear_suffix_kats()
{
    struct { uint32_t len, w[4]; } k[] = {
        {128, {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}},
        {127, {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xfffffffeu}},
        {95, {0xffffffffu, 0xffffffffu, 0xfffffffeu, 0}},
        {1, {0x80000000u, 0, 0, 0}},
        {0, {0, 0, 0, 0}},   // (the reference's -1 case: no prefix bits)
    };
    int bad = 0;
    for (const auto &c : k)
        for (int i = 0; i < 4; i++)
            bad += l6_word_mask(c.len, i) != c.w[i];
    printf("clear_suffix kats: %s\n", bad ? "FAIL" : "ok");
    return bad != 0;
}

// the IPv4 LPM builders (flatten.cpp build_dir24_8, build_l4trie) through
// host restatements of the device lookups (classify.hip's DIR-24-8 probe,
// kern_common.hpp l4_lookup) against a brute-force longest-prefix match:
// random lengths, prefixes piled under one /16 (lists, then chunk splits),
// a /0, labels past a list entry's 26 bits (lbl_ovf)
static uint32_t dir24_lookup_host(const std::vector<uint32_t> &t24,
                                  const std::vector<uint32_t> &t8, uint32_t a)
{
    uint32_t e = t24[a >> 8];
    if (e & LPM_GROUP)
        e = t8[((size_t)(e & ~LPM_GROUP) << 8) | (a & 255)];
    return e;
}
static uint32_t l4_lookup_host(const std::vector<uint32_t> &d, const std::vector<uint32_t> &c,
                               const std::vector<uint64_t> &l, const std::vector<uint32_t> &ovf,
                               uint32_t a, int dir_bits)
{
    auto list_leaf = [&](uint32_t hi) {
        const uint32_t x = hi & (LL_INDIRECT | LL_PAYLOAD);
        return (x & LL_INDIRECT) ? ovf[x & LL_PAYLOAD] : x;
    };
    uint32_t shift = 32u - (uint32_t)dir_bits;
    const uint32_t *D = &d[4 * (size_t)(a >> shift)];
    const uint32_t e1 = (D[2] >> 16) | (D[3] << 16);
    if (l4_inline_match(a, D[1], shift))
        return list_leaf((D[1] >> 21) | (D[2] << 11));
    if (l4_inline_match(a, e1, shift))
        return list_leaf(D[3] >> 5);
    uint32_t e = D[0];
    while (e & L4_PTR) {
        const uint32_t cnt = (e >> 24) & 127, off = e & L4_OFF;
        if (cnt == 0) {
            const uint32_t bits = l4_chunk_bits(shift);
            shift -= bits;
            e = c.at(off + ((a >> shift) & ((1u << bits) - 1)));
            continue;
        }
        for (uint32_t i = 0; i < cnt; i += 2) {
            const uint64_t u = l[off + i], v = l[off + i + 1];
            const bool m0 = l4_match(a, (uint32_t)u, (uint32_t)(u >> 32));
            if (m0 || l4_match(a, (uint32_t)v, (uint32_t)(v >> 32)))
                return list_leaf(m0 ? (uint32_t)(u >> 32) : (uint32_t)(v >> 32));
        }
        return 0;
    }
    return (e & LPM_INDIRECT) ? ovf[e & LPM_PAYLOAD] : e;
}
// (probes: addresses every case asks besides the random ones; one line per
// directory width, and a line for the case unless it has probes)
static int lpm4_case(const char *name, std::vector<Pfx4> pfx, std::mt19937 &gen, int nq,
                     const std::vector<uint32_t> &probes = {})
{
    {   // one prefix per (masked address, length), as the ipcache map holds
        std::map<std::pair<uint32_t, int>, Pfx4> u;
        for (Pfx4 p : pfx) {
            p.addr &= p.plen ? 0xFFFFFFFFu << (32 - p.plen) : 0u;
            u.emplace(std::make_pair(p.addr, (int)p.plen), p);
        }
        pfx.clear();
        for (auto &kv : u)
            pfx.push_back(kv.second);
    }
    std::vector<uint32_t> t24, t8, ovf[3], d[3], c[3];
    std::vector<uint64_t> l[3];
    build_dir24_8(pfx, &t24, &t8);
    int bad = 0;
    for (int D = 16; D <= 18; D++)
        bad += !build_l4trie(pfx, &ovf[D - 16], &d[D - 16], &c[D - 16], &l[D - 16], D) ||
               d[D - 16].size() != (size_t)4 << D;
    for (int q = 0; q < nq + (int)probes.size(); q++) {
        uint32_t a = gen();
        if (q >= nq) {
            a = probes[q - nq];
        } else if (!pfx.empty() && (q & 3)) {   // mostly inside some prefix
            const Pfx4 &p = pfx[gen() % pfx.size()];
            const uint32_t m = p.plen ? 0xFFFFFFFFu << (32 - p.plen) : 0u;
            a = p.addr | (a & ~m);
        }
        uint32_t want = 0;
        int best = -1;
        for (const Pfx4 &p : pfx) {
            const uint32_t m = p.plen ? 0xFFFFFFFFu << (32 - p.plen) : 0u;
            if ((int)p.plen > best && (a & m) == p.addr)
                best = p.plen, want = p.leaf;
        }
        const uint32_t x = dir24_lookup_host(t24, t8, a);
        if (x != want && bad++ < 5)
            printf("%s: %08x -> dir24 %u, want %u\n", name, a, x, want);
        for (int D = 16; D <= 18; D++) {
            const uint32_t y =
                l4_lookup_host(d[D - 16], c[D - 16], l[D - 16], ovf[D - 16], a, D);
            if (y != want && bad++ < 5)
                printf("%s: %08x -> trie /%d %u, want %u\n", name, a, D, y, want);
        }
    }
    for (int D = 16; D <= 18; D++)
        printf("lpm4 %-14s /%d chunk words %6zu list %6zu unresolved %5llu -> %s\n", name, D,
               c[D - 16].size(), l[D - 16].size(), (unsigned long long)l4_unresolved(pfx, D),
               bad ? "FAIL" : "ok");
    if (probes.empty())
        printf("lpm4 %-14s prefixes %5zu: %s\n", name, pfx.size(), bad ? "FAIL" : "ok");
    return bad != 0;
}
static int lpm4_tests(std::mt19937 &gen)
{
    int fail = 0;
    std::vector<Pfx4> v;
    for (int i = 0; i < 4000; i++)   // random lengths, some wide labels
        v.push_back({(uint32_t)gen(), (uint8_t)(gen() % 33),
                     (i % 9) ? 1 + (uint32_t)(gen() % 100000) : (1u << 27) + i});
    fail |= lpm4_case("random", v, gen, 40000);
    v.clear();   // piled under 10.20.0.0/16: lists, then chunks, then deeper
    for (int i = 0; i < 3000; i++)
        v.push_back({0x0A140000u | (uint32_t)(gen() & 0xFFFF), (uint8_t)(17 + gen() % 16),
                     1 + (uint32_t)i});
    v.push_back({0x0A140000u, 16, 77});
    v.push_back({0, 0, 5});
    fail |= lpm4_case("piled", v, gen, 40000);
    v.clear();   // piled under one /24 too: a second chunk level
    for (int i = 0; i < 600; i++)
        v.push_back({0x0A141E00u | (uint32_t)(gen() & 0xFF), (uint8_t)(25 + gen() % 8),
                     1 + (uint32_t)i});
    for (int i = 0; i < 40; i++)
        v.push_back({0x0A140000u | (uint32_t)(gen() & 0xFFFF), (uint8_t)(17 + gen() % 16),
                     (1u << 26) + (uint32_t)i});
    fail |= lpm4_case("deep", v, gen, 40000);
    for (int n : {1, 2, 3, 15, 16, 17}) {   // around the inline and list limits
        v.clear();
        for (int i = 0; i < n; i++)
            v.push_back({0xC0A80000u | (uint32_t)(gen() & 0xFFFF), (uint8_t)(17 + gen() % 16),
                         100 + (uint32_t)i});
        char nm[32];
        snprintf(nm, sizeof nm, "small-%d", n);
        fail |= lpm4_case(nm, v, gen, 5000);
    }
    // the edges of a /D directory, one table per D (every table is looked up
    // at all three widths)
    for (int D = 16; D <= 18; D++) {
        v.clear();
        std::vector<uint32_t> pr;
        const uint32_t sh = 32 - D, wide = 1u << 26;
        // lengths D-1, D, D+1 and 32 at one address: the painting over two
        // entries, the entry's own leaf, a len - D = 1 inline entry
        const uint32_t A = 0x0A140000u;
        v.push_back({A, (uint8_t)(D - 1), 11});
        v.push_back({A, (uint8_t)D, 12});
        v.push_back({A, (uint8_t)(D + 1), 13});
        v.push_back({A + 1, 32, 14});
        for (uint32_t o : {0u, 1u, 2u, 1u << (sh - 1), (1u << (sh - 1)) - 1, 1u << sh,
                           (1u << sh) - 1, 2u << sh, (2u << sh) - 1, ~0u})
            pr.push_back(A + o);
        // a /D node with 2 (inline only), 3 (the shortest list), 14 (the
        // longest) and 15 (split) longer prefixes; a label past 26 bits on
        // the longest (inline) and on the shortest (list, or a chunk leaf)
        uint32_t k = 0;
        for (int n : {2, 3, 14, 15}) {
            const uint32_t N = 0x0A200000u + (k++ << sh);
            for (int i = 0; i < n; i++) {
                const uint32_t a = N | (uint32_t)(i + 1) << 4;
                const uint8_t len = i == 0 ? 32 : i == n - 1 ? D + 1 : 28;
                const uint32_t m = 0xFFFFFFFFu << (32 - len);
                v.push_back({a & m, len,
                             i == 0 || i == n - 1 ? wide + 100u * n + i : 100u * n + i});
                for (uint32_t o : {0u, 1u, 15u, 16u})
                    pr.push_back(a + o);
            }
            pr.push_back(N);
            pr.push_back(N + (1u << sh) - 1);
            pr.push_back(N + (1u << (sh - 1)));
            pr.push_back(N + (1u << (sh - 1)) - 1);
        }
        // twenty /31 and /32 prefixes inside one /26: a split node whose
        // second chunk is the last one (128 or 64 entries at /17 and /18)
        const uint32_t M = 0x0A300040u;
        for (uint32_t i = 0; i < 20; i++) {
            const bool p31 = i % 5 == 4;
            v.push_back({M + 3 * i - (p31 ? (3 * i) & 1 : 0), (uint8_t)(p31 ? 31 : 32),
                         (i & 1 ? wide : 0) + 2000 + i});
        }
        for (uint32_t o = 0; o < 66; o++)
            pr.push_back(M - 1 + o);
        // directory indices of all ones and all zeros
        v.push_back({0xFFFFFF00u, 24, 31});
        v.push_back({0xFFFFFFFFu, 32, wide + 32});
        v.push_back({0, (uint8_t)(D + 1), 33});
        v.push_back({1, 32, 34});
        for (uint32_t a : {0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFF00u, 0xFFFFFEFFu, 0xFFFFC000u, 0u,
                           1u, 2u, (1u << (sh - 1)) - 1, 1u << (sh - 1), 1u << sh})
            pr.push_back(a);
        char nm[32];
        snprintf(nm, sizeof nm, "edges-%d", D);
        fail |= lpm4_case(nm, v, gen, 5000, pr);
    }
    return fail;
}

// the host map store (maps.cpp) against a plain model under random
// operations: a HASH (hashtab.c: -EEXIST / -ENOENT by flag, -E2BIG when
// full, get_next_key visits every key once) and an LPM_TRIE (lpm_trie.c:
// longest stored prefix no longer than the key's, data past the prefix
// ignored, -ENOSPC when full, -EINVAL past 32 bits)
static int map_fuzz(std::mt19937 &gen)
{
    int bad = 0;
    {
        Map m;
        m.type = MT_HASH, m.ksz = 8, m.vsz = 8, m.max_entries = 64;
        std::map<uint64_t, uint64_t> model;
        for (int it = 0; it < 200000; it++) {
            const uint64_t k = gen() % 96, v = gen();
            const int op = gen() % 4;
            if (op <= 1) {
                const uint64_t fl = gen() % 3;
                const bool has = model.count(k) != 0;
                const int want = fl == 1 && has ? -EEXIST : fl == 2 && !has ? -ENOENT
                                 : !has && model.size() >= 64 ? -E2BIG : 0;
                bad += m.update(&k, &v, fl) != want;
                if (!want)
                    model[k] = v;
            } else if (op == 2) {
                uint64_t got = 0;
                const int rc = m.lookup(&k, &got);
                bad += model.count(k) ? (rc != 0 || got != model[k]) : rc != -ENOENT;
            } else {
                bad += m.erase(&k) != (model.erase(k) ? 0 : -ENOENT);
            }
        }
        std::map<uint64_t, int> seen;   // a get_next_key walk from no key
        uint64_t cur = 0, nxt = 0;
        for (int rc = m.next_key(nullptr, &nxt); !rc; rc = m.next_key(&cur, &nxt))
            seen[cur = nxt]++;
        bad += seen.size() != model.size();
        for (auto &kv : seen)
            bad += kv.second != 1 || !model.count(kv.first);
    }
    {
        Map m;
        m.type = MT_LPM_TRIE, m.ksz = 8, m.vsz = 4, m.max_entries = 48;
        std::map<std::pair<uint32_t, uint32_t>, uint32_t> model;   // (plen, masked) -> v
        auto msk = [](uint32_t a, uint32_t p) { return p ? a & (0xFFFFFFFFu << (32 - p)) : 0u; };
        for (int it = 0; it < 100000; it++) {
            const uint32_t plen = gen() % 34, a = gen() & 0xFF0F00FFu, v = gen();
            uint8_t key[8];
            const uint32_t be = __builtin_bswap32(a);   // data in network order
            memcpy(key, &plen, 4);
            memcpy(key + 4, &be, 4);
            const int op = gen() % 3;
            if (op == 0) {
                const auto mk = std::make_pair(plen, plen <= 32 ? msk(a, plen) : 0u);
                const int want = plen > 32 ? -EINVAL
                                 : !model.count(mk) && model.size() >= 48 ? -ENOSPC : 0;
                bad += m.update(key, &v, 0) != want;
                if (!want)
                    model[mk] = v;
            } else if (op == 1) {
                uint32_t got = 0, want = 0;
                int best = -1;
                for (auto &e : model)
                    if ((int)e.first.first > best && e.first.first <= std::min(plen, 32u) &&
                        msk(a, e.first.first) == e.first.second)
                        best = (int)e.first.first, want = e.second;
                const int rc = m.lookup(key, &got);
                bad += best < 0 ? rc != -ENOENT : (rc != 0 || got != want);
            } else if (plen <= 32) {
                bad += m.erase(key) != (model.erase(std::make_pair(plen, msk(a, plen))) ? 0
                                                                                         : -ENOENT);
            }
        }
    }
    printf("map fuzz (hash, lpm): %s\n", bad ? "FAIL" : "ok");
    return bad != 0;
}

// the 32-bit histogram slot (classify.hpp HistSlot): k_hist's per-header
// update replayed in order on one slot, its carries and wraps counted as the
// kernel's escape table does, and the recombined sums against plain u64
// sums — for lengths that never, always and sometimes overflow the byte
// field, and add counts around the packet field's 2^11
static int hist_slot_case(const char *name, const std::vector<uint32_t> &lens)
{
    uint32_t slot = 0;
    uint64_t carries = 0, wraps = 0, packets = 0, bytes = 0;
    for (uint32_t len : lens) {
        uint32_t carry, wrap;
        HistSlot::spill(slot, len, carry, wrap);   // (slot: what the atomic returns)
        slot += HistSlot::inc(len);
        carries += carry;
        wraps += wrap;
        packets++;
        bytes += len;
    }
    const uint64_t pk = HistSlot::packets(slot) + HistSlot::esc_packets(carries, wraps);
    const uint64_t by = HistSlot::bytes(slot) + HistSlot::esc_bytes(carries);
    const bool ok = pk == packets && by == bytes;
    if (!ok)
        printf("hist slot %s n=%zu: packets %llu want %llu, bytes %llu want %llu\n", name,
               lens.size(), (unsigned long long)pk, (unsigned long long)packets,
               (unsigned long long)by, (unsigned long long)bytes);
    return !ok;
}
static int hist_slot_tests(std::mt19937 &gen)
{
    int bad = 0;
    const uint32_t pick[] = {0, 1, 59, 1500, 65534, 65535};
    for (size_t n : {(size_t)1, (size_t)2047, (size_t)2048, (size_t)2049, (size_t)100000}) {
        std::vector<uint32_t> v(n);
        std::fill(v.begin(), v.end(), 65535u);
        bad += hist_slot_case("max", v);
        std::fill(v.begin(), v.end(), 0u);
        bad += hist_slot_case("zero", v);
        for (size_t i = 0; i < n; i++)
            v[i] = (i & 1) ? 65535u : 0u;
        bad += hist_slot_case("alternating", v);
        for (size_t i = 0; i < n; i++)
            v[i] = gen() & 0xFFFF;
        bad += hist_slot_case("random", v);
        for (size_t i = 0; i < n; i++)
            v[i] = pick[gen() % 6];
        bad += hist_slot_case("mixed", v);
    }
    // the ranges that follow from the slot width: every identity a packed
    // key can carry has a range, and id_cover has a bit for it
    bad += ID_RANGES > 32 || id_range_of(ID_PACK_LIMIT - 1) != ID_RANGES - 1 ||
           2 * ID_RANGE != HIST_RANGE;
    printf("hist slot u32 {%u | %u}, %u ranges of %u identities     %s\n", HistSlot::PK,
           HistSlot::BY, ID_RANGES, ID_RANGE, bad ? "FAIL" : "ok");
    return bad != 0;
}

// known answers of the layout.h hashes, one `kat <name> <inputs> <value>`
// line each (hex): what a restatement elsewhere (tests/lookup_edges.py, which
// places keys by them) is compared with
static void hash_kats()
{
    const uint32_t V[] = {0u, 0xFFFFFFFFu, 1u, 0x0100000Au, 0x9E3779B9u, 0x80000000u, 0x1010u};
    const uint32_t MASKS[] = {0u, 7u, 511u, 0xFFFFu, 0xFFFFFFFFu};
    for (uint32_t a : V) {
        printf("kat fmix32 %x %x\n", a, fmix32(a));
        printf("kat bloom_bits %x %x\n", a, bloom_bits(a));
        printf("kat pol_bloom_salt %x %x\n", a, pol_bloom_salt(a));
        printf("kat pf_bloom_hash %x %x\n", a, pf_bloom_hash(a));
        printf("kat l6_bloom_bits %x %llx\n", a, (unsigned long long)l6_bloom_bits(a));
        for (uint32_t m : MASKS) {
            printf("kat hash32 %x %x %x\n", a, m, hash32(a, m));
            printf("kat pol_slot %x %x %x\n", a, m, pol_slot(a, m));
        }
        for (uint32_t b : V) {
            printf("kat pol_key_pre %x %x %x\n", a, b, pol_key_pre(a, b));
            printf("kat pol_bloom_hash %x %x %x\n", a, b, pol_bloom_hash(a, b));
        }
    }
    for (uint32_t len : {0u, 1u, 31u, 32u, 33u, 63u, 64u, 65u, 95u, 96u, 97u, 127u, 128u})
        for (int i = 0; i < 4; i++)
            printf("kat l6_word_mask %x %x %x\n", len, (uint32_t)i, l6_word_mask(len, i));
    const uint32_t W[][4] = {{0, 0, 0, 0},
                             {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu},
                             {0x20010db8u, 0x00050000u, 0, 1},
                             {0xbeef0000u, 0, 0x00000001u, 0x016582bcu},
                             {1, 2, 3, 4}};
    for (const auto &w : W) {
        for (uint32_t tag : {0u, 1u, 64u, 65u, 128u, 0x200u, 0xFFFFFFFFu})
            printf("kat l6_hash %x %x %x %x %x %x\n", w[0], w[1], w[2], w[3], tag,
                   l6_hash(w[0], w[1], w[2], w[3], tag));
        for (uint32_t sel : {1u, 32u, 33u, 48u, 64u, 65u, 127u, 128u})
            printf("kat l6_group_hash %x %x %x %x %x %x\n", w[0], w[1], w[2], w[3], sel,
                   l6_group_hash(w, sel));
        printf("kat pf6_bloom_hash %x %x %x %x %x\n", w[0], w[1], w[2], w[3],
               pf6_bloom_hash(w[0], w[1], w[2], w[3]));
    }
}

// ---- direct placement of the policy keys (flatten.cpp pol_place_direct,
// layout.h pol_slot_direct): the tables built as build_image builds them
// (linear, 4 slots per key, at least 8), re-placed, and the lookup the device
// performs (one probe at the bucket's displacement: the slot holds the key or
// the key is absent) against brute force: every key found once with the
// counter index it had, absent keys not found, nothing lost or added.
struct PolTabs {
    std::vector<PolSlot> pol;
    std::vector<PolLoc> tabs;
    std::vector<std::vector<uint64_t>> keys;
};
static PolTabs pol_linear(const std::vector<std::vector<uint64_t>> &keys)
{
    PolTabs P;
    P.keys = keys;
    PolSlot empty{};
    empty.key = POL_EMPTY;
    empty.ctr = EMPTY;
    uint32_t ctr = 0;
    for (const auto &ks : keys) {
        uint32_t ns = 8;
        while (ns < 4 * ks.size())
            ns <<= 1;
        PolLoc loc;
        loc.present = 1;
        loc.base = (uint32_t)P.pol.size();
        loc.mask = ns - 1;
        P.pol.resize(P.pol.size() + ns, empty);
        for (uint64_t k : ks) {
            uint32_t s = pol_slot(pol_key_pre((uint32_t)k, (uint32_t)(k >> 32)), loc.mask);
            while (P.pol[loc.base + s].key != POL_EMPTY)
                s = (s + 1) & loc.mask;
            P.pol[loc.base + s].key = k;
            P.pol[loc.base + s].proxy_port = (uint16_t)(ctr * 7);
            P.pol[loc.base + s].ctr = ctr++;
        }
        P.tabs.push_back(loc);
    }
    return P;
}
static int pol_direct_case(const char *name, const std::vector<std::vector<uint64_t>> &keys,
                           uint32_t words, bool want_placed, std::mt19937 &gen)
{
    PolTabs P = pol_linear(keys);
    const std::vector<PolSlot> before = P.pol;
    std::vector<uint8_t> disp;
    uint32_t maxd = 0;
    const bool placed = pol_place_direct(&P.pol, P.tabs, words, &disp, &maxd);
    int bad = placed != want_placed;
    size_t nkeys = 0, d0 = 0;
    if (!placed) {   // the linear tables stay as they were
        bad |= !disp.empty() || memcmp(before.data(), P.pol.data(), sizeof(PolSlot) * before.size());
    } else {
        bad |= disp.size() != words;
        uint32_t ctr = 0;
        for (size_t t = 0; t < keys.size(); t++) {
            const PolLoc &L = P.tabs[t];
            const PolSlot *tab = P.pol.data() + L.base;
            for (uint64_t k : keys[t]) {
                const uint32_t s = pol_find_slot(tab, L.base, L.mask, k, disp);
                bad |= s == EMPTY || tab[s].key != k || tab[s].ctr != ctr ||
                       tab[s].proxy_port != (uint16_t)(ctr * 7);
                ctr++;
            }
            size_t used = 0;
            for (uint32_t s = 0; s <= L.mask; s++)
                used += tab[s].key != POL_EMPTY;
            bad |= used != keys[t].size();
            nkeys += used;
            for (int q = 0; q < 2000; q++) {   // absent keys (and, rarely, present ones)
                const uint64_t k = ((uint64_t)(gen() & 0x01FFFFFFu) << 32) | (gen() & 0xFFFFu);
                bool in = false;
                for (uint64_t x : keys[t])
                    in |= x == k;
                bad |= (pol_find_slot(tab, L.base, L.mask, k, disp) != EMPTY) != in;
            }
        }
        for (uint8_t d : disp)
            d0 += d == 0;
    }
    printf("poldirect %-12s %zu tables, %zu keys, %u words: %s, max d %u, %zu words at d 0 -> %s\n",
           name, keys.size(), nkeys, words, placed ? "placed" : "linear", maxd, d0,
           bad ? "FAIL" : "ok");
    return bad;
}
static uint64_t pol_rand_key(std::mt19937 &gen)
{
    // {identity, dport, proto, egress}: pad bits clear
    return ((uint64_t)(gen() & 0x01FFFFFFu) << 32) | (gen() & 0xFFFFFFu);
}
static int pol_direct_tests()
{
    std::mt19937 gen(4242);   // (its own stream: the same cases alone and in the whole run)
    int fail = 0;
    auto distinct = [&](size_t n) {
        std::map<uint64_t, int> seen;
        std::vector<uint64_t> v;
        while (v.size() < n) {
            const uint64_t k = pol_rand_key(gen);
            if (seen.emplace(k, 1).second)
                v.push_back(k);
        }
        return v;
    };
    {   // random: tables of every size class, about two keys per word
        std::vector<std::vector<uint64_t>> T;
        for (size_t n : {1u, 2u, 3u, 5u, 16u, 17u, 100u, 700u, 2000u, 4000u, 9000u})
            T.push_back(distinct(n));
        fail |= pol_direct_case("random", T, 8192, true, gen);
    }
    {   // piled: 400 smallest tables (2 and 3 keys in 8 and 16 slots) behind 64
        // words, 15 keys to a word (a step is one of four values modulo 8:
        // two keys of one 8-slot table that share word, home slot and step
        // would never part; this seed's 1000 keys hold no such pair); and
        // one table whose keys share a home slot
        std::vector<std::vector<uint64_t>> T;
        for (int i = 0; i < 400; i++)
            T.push_back(distinct(2 + i % 2));
        fail |= pol_direct_case("piled-small", T, 64, true, gen);
        std::vector<uint64_t> same;
        while (same.size() < 12) {
            const uint64_t k = pol_rand_key(gen);
            if ((pol_key_pre((uint32_t)k, (uint32_t)(k >> 32)) & 63) == 5)
                same.push_back(k);
        }
        fail |= pol_direct_case("piled-home", {same}, 64, true, gen);
    }
    {   // equal pre: lo' * K ^ hi' = lo * K ^ hi — no displacement separates them
        const uint32_t K = 0x9E3779B1u, lo = 1234, hi = 0x00060050u;
        uint32_t lo2 = 1;
        while (((lo2 * K) ^ (lo * K) ^ hi) >> 25)
            lo2++;
        const uint32_t hi2 = (lo2 * K) ^ (lo * K) ^ hi;
        std::vector<uint64_t> v = distinct(20);
        v.push_back((uint64_t)hi << 32 | lo);
        v.push_back((uint64_t)hi2 << 32 | lo2);
        fail |= pol_key_pre(lo, hi) != pol_key_pre(lo2, hi2) || (lo == lo2 && hi == hi2);
        fail |= pol_direct_case("equal-pre", {v}, 64, false, gen);
    }
    {   // hundreds of keys to a word: no displacement within a byte
        fail |= pol_direct_case("crowded", {distinct(40000)}, 64, false, gen);
    }
    return fail;
}
// known answers of pol_slot_direct: `pd pol_slot_direct <pre> <d> <mask> <slot>`
static void pol_direct_kats()
{
    const uint32_t V[] = {0u, 0xFFFFFFFFu, 1u, 0x0100000Au, 0x9E3779B9u, 0x80000000u, 0x1010u,
                          0x00070007u};
    for (uint32_t pre : V)
        for (uint32_t d : {0u, 1u, 2u, 7u, 19u, 255u})
            for (uint32_t m : {7u, 63u, 511u, 0xFFFFu, 0xFFFFFu})
                printf("pd pol_slot_direct %x %x %x %x\n", pre, d, m, pol_slot_direct(pre, d, m));
}

// ---- the proxy maps' device tables (flatten.cpp build_revproxy) against a
// brute-force lookup of the maps themselves
struct RpKey {
    uint32_t a[4];       // saddr raw (IPv4: a[0])
    uint32_t ports;      // dport | sport << 16
    uint8_t nh;
};
static void rp_put(Map &m, bool v6, const RpKey &k, uint32_t tag)
{
    uint8_t key[22] = {0}, val[28] = {0};
    const size_t al = v6 ? 16 : 4;
    memcpy(key, k.a, al);
    memcpy(key + al, &k.ports, 4);
    key[al + 4] = k.nh;
    uint32_t od[4] = {tag * 2654435761u, tag ^ 0x5555u, tag + 7, ~tag};
    const uint16_t op = (uint16_t)(tag * 40503u);
    const uint32_t ident = tag, life = 1;
    memcpy(val, od, al);
    memcpy(val + al, &op, 2);
    memcpy(val + al + 4, &ident, 4);
    memcpy(val + al + 8, &life, 4);
    if (m.update(key, val, 0))
        abort();
}
// the table's answer for k against the map's: 0 when they agree
static int rp_check(const Map &m, const HostImage &img, bool v6, const RpKey &k)
{
    uint8_t key[22] = {0}, val[28] = {0};
    const size_t al = v6 ? 16 : 4;
    memcpy(key, k.a, al);
    memcpy(key + al, &k.ports, 4);
    key[al + 4] = k.nh;
    const bool have = m.lookup(key, val) == 0;
    const int64_t s = v6 ? rp6_find_slot(img, k.a, k.ports, k.nh)
                         : rp4_find_slot(img, k.a[0], k.ports, k.nh);
    if (!have)
        return s >= 0;
    if (s < 0)
        return 1;
    uint16_t op;
    memcpy(&op, val + al, 2);
    if (v6) {
        const uint4 od = img.rp6_val[s];
        return memcmp(&od, val, 16) != 0 || img.rp6[2 * s + 1].z != op;
    }
    return memcmp(&img.rp4[s].w, val, 4) != 0 || img.rp4_val[s] != op;
}
static RpKey rp_rand(std::mt19937 &gen, bool v6)
{
    RpKey k{{(uint32_t)gen(), v6 ? (uint32_t)gen() : 0u, v6 ? (uint32_t)gen() : 0u,
             v6 ? (uint32_t)gen() : 0u},
            (uint32_t)gen(), (uint8_t)((gen() & 1) ? 6 : 17)};
    return k;
}
static uint32_t rp_home(const RpKey &k, bool v6, uint32_t mask)
{
    return (v6 ? rp6_hash(k.a[0], k.a[1], k.a[2], k.a[3], k.ports, k.nh)
               : rp4_hash(k.a[0], k.ports, k.nh)) & mask;
}
static int rp_case(const char *name, bool v6, const std::vector<RpKey> &keys,
                   const std::vector<RpKey> &absent, uint32_t want_slots, bool want_wrap)
{
    Map m;
    m.type = MT_HASH, m.ksz = v6 ? 22 : 10, m.vsz = v6 ? 28 : 16, m.max_entries = 1u << 20;
    m.role = v6 ? ROLE_PROXY6 : ROLE_PROXY4;
    for (size_t i = 0; i < keys.size(); i++)
        rp_put(m, v6, keys[i], (uint32_t)i + 1);
    HostImage img;
    build_revproxy(v6 ? nullptr : &m, v6 ? &m : nullptr, &img);
    const uint32_t slots = v6 ? (uint32_t)img.rp6_val.size() : (uint32_t)img.rp4.size();
    const uint32_t mask = v6 ? img.rp6_mask : img.rp4_mask, n = v6 ? img.n_rp6 : img.n_rp4;
    int bad = slots != want_slots || n != keys.size() || (slots && mask != slots - 1) ||
              (slots & (slots - 1)) || 2 * n > slots;
    bad |= (v6 ? img.rp4.size() : img.rp6.size()) != 0;   // the other family: no table
    uint32_t used = 0, wraps = 0;
    for (uint32_t s = 0; s < slots; s++)
        used += ((v6 ? img.rp6[2 * s + 1].y : img.rp4[s].z) & RP_USED) != 0;
    bad |= used != n;
    for (const RpKey &k : keys) {
        bad |= rp_check(m, img, v6, k);
        const int64_t s = v6 ? rp6_find_slot(img, k.a, k.ports, k.nh)
                             : rp4_find_slot(img, k.a[0], k.ports, k.nh);
        wraps += s >= 0 && (uint32_t)s < rp_home(k, v6, mask);
    }
    for (const RpKey &k : absent)
        bad |= rp_check(m, img, v6, k);
    bad |= want_wrap && !wraps;
    printf("revproxy %-10s v%d %zu entries, %u slots, %zu absent keys, %u wrapped -> %s\n", name,
           v6 ? 6 : 4, keys.size(), slots, absent.size(), wraps, bad ? "FAIL" : "ok");
    return bad;
}
static int revproxy_tests()
{
    std::mt19937 gen(777);   // (its own stream: the same cases alone and in the whole run)
    int fail = 0;
    for (int f = 0; f < 2; f++) {
        const bool v6 = f != 0;
        auto absent_of = [&](const std::vector<RpKey> &keys) {
            // random keys, and every key with exactly one field changed
            std::vector<RpKey> q;
            for (int i = 0; i < 64; i++)
                q.push_back(rp_rand(gen, v6));
            for (const RpKey &k : keys) {
                if (q.size() > 4000)
                    break;
                RpKey a = k, d = k, s = k, p = k;
                a.a[v6 ? 3 : 0] ^= 0x01000000u;
                d.ports ^= 0x0100u;
                s.ports ^= 0x01000000u;
                p.nh = k.nh == 6 ? 17 : 6;
                q.insert(q.end(), {a, d, s, p});
            }
            return q;
        };
        // 0, 1, 2 entries; a power of two and one above it (2n slots: the
        // slot count doubles between them)
        const uint32_t sizes[][2] = {{0, 0}, {1, 2}, {2, 4}, {4, 8}, {5, 16}, {64, 128},
                                     {65, 256}, {1000, 2048}};
        for (auto &sz : sizes) {
            std::vector<RpKey> keys;
            for (uint32_t i = 0; i < sz[0]; i++)
                keys.push_back(rp_rand(gen, v6));
            char name[32];
            snprintf(name, sizeof name, "n%u", sz[0]);
            fail |= rp_case(name, v6, keys, absent_of(keys), sz[1], false);
        }
        {   // entries that differ in exactly one field each: all present, each its own value
            const RpKey k = rp_rand(gen, v6);
            RpKey a = k, d = k, s = k, p = k;
            a.a[v6 ? 2 : 0] ^= 0x00010000u;
            d.ports ^= 0x0001u;
            s.ports ^= 0x00010000u;
            p.nh = k.nh == 6 ? 17 : 6;
            const std::vector<RpKey> keys = {k, a, d, s, p};
            fail |= rp_case("one-field", v6, keys, absent_of(keys), 16, false);
        }
        {   // a probe chain that wraps the end of the table: three keys whose
            // home is the last of 8 slots, and a fourth elsewhere
            std::vector<RpKey> keys;
            while (keys.size() < 3) {
                const RpKey k = rp_rand(gen, v6);
                if (rp_home(k, v6, 7) == 7)
                    keys.push_back(k);
            }
            for (;;) {
                const RpKey k = rp_rand(gen, v6);
                if (rp_home(k, v6, 7) == 3) {
                    keys.push_back(k);
                    break;
                }
            }
            // absent keys that start on the chain and walk it to its free end
            std::vector<RpKey> q = absent_of(keys);
            while (q.size() < 100) {
                const RpKey k = rp_rand(gen, v6);
                if (rp_home(k, v6, 7) == 7 || rp_home(k, v6, 7) == 0)
                    q.push_back(k);
            }
            fail |= rp_case("wrap", v6, keys, q, 8, true);
        }
    }
    return fail;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "revproxy"))   // the proxy maps' tables alone
        return revproxy_tests();
    if (argc > 1 && !strcmp(argv[1], "poldirect")) {   // the direct policy placement alone
        pol_direct_kats();
        return pol_direct_tests();
    }
    if (argc > 2 && !strcmp(argv[1], "kat") && !strcmp(argv[2], "selfcut")) {
        selfcut_kats();   // the cut rule's known answers alone
        return 0;
    }
    if (argc > 2 && !strcmp(argv[1], "kat") && !strcmp(argv[2], "svchash")) {
        svchash_kats();   // the CT key fingerprints and home slots alone
        return 0;
    }
    hash_kats();
    if (argc > 1 && !strcmp(argv[1], "kat"))   // the known answers alone
        return 0;
    std::mt19937 gen(12345);
    if (argc > 1 && !strcmp(argv[1], "lpm4"))   // the IPv4 LPM builders alone
        return lpm4_tests(gen);
    auto rng = [&gen]() -> uint32_t { return (uint32_t)gen(); };
    int fail = 0;
    {   // C3-like: /32../128, mass at /48 /56 /64 /128
        const int lens[] = {32, 40, 48, 48, 48, 56, 56, 64, 64, 64, 96, 128, 128};
        std::vector<Pfx6> v;
        for (int i = 0; i < 3000; i++) {
            uint32_t a[4] = {0x20000000u | (rng() & 0x0FFFFFFFu), rng(), rng(), rng()};
            add(v, a, lens[rng() % 13], 256 + i);
        }
        fail |= run("c3-like", v, rng, 20000);
    }
    {   // piled: pods (/128) under few /64s, /64s under one /48, a /0
        std::vector<Pfx6> v;
        uint32_t base[4] = {0x20010db8u, 0x00050000u, 0, 0};
        add(v, base, 48, 1000);
        for (int n = 0; n < 40; n++) {
            uint32_t a[4] = {base[0], base[1] | (rng() & 0xFFFF), rng(), rng()};
            add(v, a, 64, 2000 + n);
            for (int k = 0; k < 30; k++) {
                uint32_t b[4] = {a[0], a[1], rng(), rng()};
                add(v, b, 128, 5000 + 100 * n + k);
            }
        }
        uint32_t z[4] = {0, 0, 0, 0};
        add(v, z, 0, 7);
        fail |= run("piled", v, rng, 20000);
    }
    {   // every length 1..128, label 0 shadows, overlapping chains
        std::vector<Pfx6> v;
        uint32_t a[4] = {0x20010db8u, 0x12345678u, 0x9abcdef0u, 0x0fedcba9u};
        for (int len = 1; len <= 128; len++)
            add(v, a, len, (len % 7) ? 100 + len : 0);
        for (int i = 0; i < 500; i++) {
            uint32_t b[4] = {rng(), rng(), rng(), rng()};
            add(v, b, 1 + rng() % 128, (i % 5) ? 300 + i : 0);
        }
        fail |= run("all-lengths", v, rng, 20000);
    }
    {   // exact /128 set (the prefilter's fix map) and an empty table
        std::vector<Pfx6> v;
        for (int i = 0; i < 5000; i++) {
            uint32_t a[4] = {rng(), rng(), rng(), rng()};
            add(v, a, 128, 1);
        }
        fail |= run("exact128", v, rng, 20000);
        fail |= run("empty", std::vector<Pfx6>(), rng, 1000);
    }
    fail |= selfcut_tests();
    fail |= clear_suffix_kats();
    fail |= map_fuzz(gen);
    fail |= lpm4_tests(gen);
    fail |= hist_slot_tests(gen);
    fail |= pol_direct_tests();
    fail |= ReplayCase<false>().run();
    fail |= ReplayCase<true>().run();
    fail |= revproxy_tests();
    return fail;
}
