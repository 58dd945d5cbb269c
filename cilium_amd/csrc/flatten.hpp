// Flattening of the host maps into the device layouts of layout.h.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "layout.h"
#include "maps.hpp"

namespace cfc {

struct PolLoc {
    uint32_t base = 0, mask = 0, present = 0;
};

// IPv4 ipcache layouts (cfc_set_option CFC_OPT_LPM4)
enum Lpm4Layout { LPM4_AUTO = 0, LPM4_DIR24_8 = 1, LPM4_TRIE = 2 };

// The compact layout's directory width (cfc_set_option
// CFC_OPT_LPM4_DIR_BITS; layout.h l4d).  Auto takes the narrowest width that
// leaves less than L4_AUTO_SHARE_NUM / L4_AUTO_SHARE_DEN of the prefixes to a
// second load (l4_unresolved), else the widest, as long as l4d + l4c + l4l
// stay within L4_AUTO_BUDGET bytes (it narrows again while they do not).
// Both constants come from the C2 measurements in DESIGN.md section 4
// "Directory width": 19 % of the C2 prefixes unresolved at /16 cost 5 % of
// the classify kernel, 7 % at /17 and 2 % at /18 measure the same, and a
// 4 MiB directory fills an XCD's L2 on its own.
constexpr int L4_DIR_BITS_MIN = 16, L4_DIR_BITS_MAX = 18;
constexpr uint64_t L4_AUTO_SHARE_NUM = 1, L4_AUTO_SHARE_DEN = 10;
constexpr uint64_t L4_AUTO_BUDGET = 3u << 20;

// Placement of the policy keys (cfc_set_option CFC_OPT_POL_PLACEMENT;
// layout.h pol_slot_direct).  Auto takes direct when every bucket finds a
// displacement and the displacement bytes fit the classify workgroups' LDS
// image, else linear probing; forced direct fails the commit instead.
enum PolPlacement { POL_PLACE_AUTO = 0, POL_PLACE_LINEAR = 1, POL_PLACE_DIRECT = 2 };

struct BuildOpts {
    int lpm4 = LPM4_AUTO;
    int lpm4_dir_bits = 0;   // 0 = auto, or 16..18
    int pol_placement = POL_PLACE_AUTO;
    // the proxy maps' tables at 1/4 load instead of 1/2 where they fit
    // (CFC_OPT_PROXY_APPLY device: room for the in-place inserts)
    bool rp_quarter = false;
};

// IPv6 LPM (layout.h Lpm6), host side
struct Pfx6 {
    uint32_t w[4];   // host-order words, masked
    uint8_t plen;
    uint32_t label;
};
struct Lpm6Host {
    std::vector<L6Slot> slots;     // prefixes longer than /64
    std::vector<uint4> slots64;    // /1-/64: {w0, w1, label, len}
    std::vector<uint64_t> bloom;
    std::vector<uint32_t> lens;
    uint32_t def_label = 0;
    uint32_t n = 0;        // prefixes (incl. /0)
    uint32_t groups = 0;   // Bloom groups
    uint64_t bytes() const
    {
        return sizeof(L6Slot) * slots.size() + 16ull * slots64.size() + 8ull * bloom.size() +
               4ull * lens.size();
    }
};
// lpm6_find_slot's answer for a prefix in slots64: L6_S64 | its slot
constexpr int64_t L6_S64 = (int64_t)1 << 40;
void build_lpm6(const std::vector<Pfx6> &pfx, Lpm6Host *out);
// one ipcache entry (normalised key, value) as an IPv6 prefix; false when it
// is not one the IPv6 table holds on its own (prefix within the static part)
bool ipcache_v6_entry(const std::string &nk, const std::string &val, Pfx6 *p);
// the slot of prefix p in a built table, or -1
int64_t lpm6_find_slot(const Lpm6Host &t, const Pfx6 &p);
// host reference of the device lookup (unit tests): the label of the
// longest prefix containing w, def_label when none
uint32_t lpm6_lookup_host(const Lpm6Host &t, const uint32_t w[4]);

struct HostImage {
    // the CT tables' least slot counts (a device apply that outgrew the
    // table asked for more: cfc_api.cpp ct_apply_dev)
    uint64_t ct_min4 = 0, ct_min6 = 0;
    // IPv4 ipcache: compact multibit (l4c/l4l) or DIR-24-8 (tbl24/tbl8)
    std::vector<uint32_t> tbl24, tbl8, lbl_ovf;
    std::vector<uint32_t> l4d, l4c;    // l4d: 4 words per directory entry
    std::vector<uint64_t> l4l;
    int l4_dir_bits = 0;           // the directory's width (compact layout)
    // per width 16, 17, 18: prefixes its directory load cannot resolve
    uint64_t l4_unresolved[3] = {0, 0, 0};
    int lpm4_layout = 0;           // LPM4_DIR24_8 / LPM4_TRIE, 0 = empty
    uint32_t n_prefix4 = 0;
    // prefilter
    std::vector<uint32_t> pf_tbl24, pf_tbl8;
    uint32_t n_pf_dyn = 0;
    std::vector<uint32_t> pf_fix;
    uint32_t pf_fix_mask = 0, pf_fix_zero = 0, n_pf_fix = 0;
    std::vector<uint32_t> pf_bloom;                 // words (pow2) or empty
    std::vector<uint32_t> pf6_bloom;                // over pf6_fix (all /128), or empty
    // endpoints
    std::vector<LxcSlot> lxc4;
    uint32_t lxc4_mask = 0, n_eps = 0;
    // policy
    std::vector<PolSlot> pol;
    std::vector<uint32_t> pol_bloom;
    // direct placement: one displacement byte per Bloom word (empty: linear)
    std::vector<uint8_t> pol_disp;
    bool pol_direct = false;
    bool pol_direct_failed = false;                // tried, and kept linear
    uint32_t pol_max_disp = 0;
    std::unordered_map<int, PolLoc> pol_loc;       // lxc_id -> table
    // IPv6
    Lpm6Host ipc6, pf6_fix, pf6_dyn;
    std::vector<Lxc6Slot> lxc6;
    uint32_t lxc6_mask = 0, n_eps6 = 0;
    // per LXC_ID its IPv4 / IPv6 address (raw), endpoints with one
    std::map<uint16_t, uint32_t> nat4;
    std::map<uint16_t, uint4> nat6;
    std::vector<std::pair<Map *, std::string>> ctr_owner;  // ctr -> entry
    // conntrack (layout.h): every CT map in one table per family
    std::vector<Ct4Slot> ct4;
    std::vector<Ct6Slot> ct6;
    std::vector<CtTimer> ct4_tm, ct6_tm;     // parallel to ct4 / ct6
    uint32_t ct4_mask = 0, ct4_probe = 0, ct6_mask = 0, ct6_probe = 0;
    uint32_t n_ct4 = 0, n_ct6 = 0;           // entries placed
    uint32_t n_nat46 = 0;                    // IPv4 entries with nat46
    std::vector<uint8_t> ct_local;           // lxc_id -> has local CT maps
    // load balancing (layout.h): service slots, reverse NAT, and per CT4
    // slot the entry's LB state (built with GROUP_CT when lb_ct is set)
    std::vector<uint4> lb4;
    uint32_t lb4_mask = 0, n_lb4 = 0;
    std::vector<uint2> rnat4;
    std::vector<uint4> ct4_lb;
    bool lb_ct = false;                      // ct4_lb wanted
    std::vector<uint4> lb6;                  // IPv6: 3 per slot
    uint32_t lb6_mask = 0, n_lb6 = 0;
    std::vector<uint4> rnat6;                // 2 per index
    std::vector<uint4> ct6_lb;
    bool lb6_ct = false;                     // ct6_lb wanted
    // proxy maps for reverse_proxy (layout.h RevTables); rp6: 2 per slot
    std::vector<uint4> rp4, rp6, rp6_val;
    std::vector<uint32_t> rp4_val;
    uint32_t rp4_mask = 0, rp6_mask = 0, n_rp4 = 0, n_rp6 = 0;
    bool rp_too_big = false;                 // a table would pass RP_MAX_TABLE_BYTES
    uint64_t device_bytes() const;
};

// the CT map a slot's entry lives in: (family 4/6, owner word, any) key
uint64_t ct_map_key(int family, uint32_t owner, int any);
// the device slot of a CT map entry; false when no lookup reaches it
bool ct_slot_of(const Map *m, const std::string &key, Ct4Slot *s4, Ct6Slot *s6);
// the report state the kernels read (CtTimer) of a struct ct_entry value
CtTimer ct_timer_of(const std::string &val);
// the LB state a CT4 slot carries (ct4_lb) of a struct ct_entry value
uint4 ct_lb_of(const std::string &val);

// Table groups an epoch is built from; a commit rebuilds only the groups
// whose maps changed (the others' device buffers carry over).
enum : unsigned {
    GROUP_IPCACHE4 = 1,   // ipcache, IPv4 LPM (+ lbl_ovf)
    GROUP_PREFILTER = 2,  // XDP prefilter, both families
    GROUP_ENDPOINTS = 4,  // cilium_lxc + every policymap (+ counter layout)
    GROUP_CT = 8,         // every CT map
    GROUP_IPCACHE6 = 16,  // ipcache, IPv6 LPM
    GROUP_LB = 32,        // cilium_lb{4,6}_services, cilium_lb{4,6}_reverse_nat
    GROUP_PROXY = 64,     // cilium_proxy4, cilium_proxy6 (reverse_proxy's table)
    GROUP_ALL = 127,
};
// the proxy maps (either may be null) into img's rp4 / rp6 tables; quarter:
// sized for 1/4 load where RP_MAX_TABLE_BYTES allows, else for 1/2
void build_revproxy(const Map *p4, const Map *p6, HostImage *img, bool quarter = false);
// host reference of the device lookup (unit tests): the slot of the key
// {saddr, ports (dport | sport << 16), nexthdr} in a built table, or -1
int64_t rp4_find_slot(const HostImage &img, uint32_t saddr, uint32_t ports, uint32_t nexthdr);
int64_t rp6_find_slot(const HostImage &img, const uint32_t saddr[4], uint32_t ports,
                      uint32_t nexthdr);
// maps: every map of the context; groups: which parts of img to build
// (ct_local, which only depends on which CT maps exist, always is).
void build_image(const std::vector<Map *> &maps, const BuildOpts &opt,
                 HostImage *img, unsigned groups = GROUP_ALL);

// Re-place the keys of linearly built policy tables (tabs: every table of
// pol) collision-free by hash-and-displace over `words` Bloom words
// (layout.h pol_slot_direct): buckets largest first, each the smallest d in
// 0..POL_DISP_MAX that puts all its keys on free slots of their own tables.
// Entries keep their proxy port and counter index.  False, with pol
// untouched and disp empty, when a bucket finds none (two keys of one table
// with equal pre, or hundreds of keys to a word).
bool pol_place_direct(std::vector<PolSlot> *pol, const std::vector<PolLoc> &tabs,
                      uint32_t words, std::vector<uint8_t> *disp, uint32_t *max_disp);
// the slot of `key` in the table at tab (its base and mask) under the
// epoch's placement (disp empty: linear probing), or EMPTY
uint32_t pol_find_slot(const PolSlot *tab, uint32_t base, uint32_t mask, uint64_t key,
                       const std::vector<uint8_t> &disp);

// exposed for host-side unit tests of the LPM builders
struct Pfx4 {
    uint32_t addr;   // host byte order
    uint8_t plen;
    uint32_t leaf;   // encoded LPM leaf
};
void build_dir24_8(std::vector<Pfx4> pfx, std::vector<uint32_t> *tbl24,
                   std::vector<uint32_t> *tbl8);
// compact multibit layout (layout.h); labels too wide for a list entry get
// lbl_ovf entries.  False when an offset would not fit its 24 bits.
bool build_l4trie(std::vector<Pfx4> pfx, std::vector<uint32_t> *ovf,
                  std::vector<uint32_t> *l4d, std::vector<uint32_t> *l4c,
                  std::vector<uint64_t> *l4l, int dir_bits = L4_DIR_BITS_MIN);
// the prefixes a directory of dir_bits bits cannot resolve in its one load:
// over its entries, max(0, prefixes longer than dir_bits - L4_INLINE)
uint64_t l4_unresolved(const std::vector<Pfx4> &pfx, int dir_bits);
// the width auto starts from (before the byte budget, build_image)
int l4_auto_dir_bits(const std::vector<Pfx4> &pfx);
// the IPv4 prefixes of an ipcache map as the LPM builders take them (ovf:
// labels too wide for a leaf)
void ipcache_v4_prefixes(const Map *m, std::vector<Pfx4> *out, std::vector<uint32_t> *ovf);

}  // namespace cfc
