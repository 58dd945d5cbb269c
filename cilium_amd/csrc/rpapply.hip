// The device upsert of a cfc_proxy_apply_* batch's records into the family's
// live reverse-proxy table (layout.h RevTables / RevWriter; CFC_OPT_PROXY_APPLY
// = CFC_PROXY_APPLY_DEVICE): what a BPF map update is to the next packet's
// reverse_proxy lookup, without re-flattening and uploading the host map.
//
// The records are the ones launch_proxy_write left on the device
// (cfc_proxy4_entry / cfc_proxy6_entry: key at byte 0, value at byte 16 / 32),
// one per distinct key.  The table rules are build_revproxy's: rp4_hash /
// rp6_hash masked, linear probing walked to the first slot with RP_USED
// clear, the key's pad byte not compared, no tombstones.
//
// Two launches, one lane per record in each:
//   k_rp_find    walks the record's probe sequence.  A key the table holds
//                gets its value overwritten in its slot; an absent key's
//                record index goes to a list (one atomic per wave).
//   k_rp_insert  a lane per listed record claims the first free slot of its
//                walk with a CAS on the slot's used word (0 -> nexthdr |
//                RP_USED), then writes the slot's other words.  A lost CAS
//                moves on.  It compares no key.
// They must be separate: a lane comparing keys against a slot another lane
// has claimed but not yet filled could match it (a key with saddr 0 and ports
// 0 equals a claimed, unfilled IPv4 slot word for word).  In k_rp_find no
// key or used word changes — only values, of keys no other lane holds, since
// a batch's records have distinct keys — so every walk sees the table as the
// launch found it; in k_rp_insert nothing is compared, and the listed keys
// are distinct and absent, so each takes exactly one slot.  The host keeps
// the table at most half full (cfc_api.cpp), so a walk always ends.
//
// A from-host pass racing an upsert on another stream may see a claimed slot
// before its key words: it reads the zeroes build_revproxy left there, as a
// BPF lookup racing an update sees the old or the new map.
#include "kern_common.hpp"

namespace cfc {
namespace {

constexpr int RPA_BLOCK = 256;

struct Rec4 {
    uint32_t sa, pt, nh, od, op;
};
struct Rec6 {
    uint4 a, od;
    uint32_t pt, nh, op;
};

// record i of the batch (the key's pad byte, bits 8-15 of its last word, and
// the value's pad are not part of the table)
__device__ __forceinline__ Rec4 rp_rec4(const uint4 *rec, uint32_t i)
{
    const uint4 k = rec[2 * (uint64_t)i], v = rec[2 * (uint64_t)i + 1];
    return Rec4{k.x, k.y, k.z & 0xFFu, v.x, v.y & 0xFFFFu};
}
__device__ __forceinline__ Rec6 rp_rec6(const uint4 *rec, uint32_t i)
{
    const uint4 *r = rec + 4 * (uint64_t)i;
    const uint4 k1 = r[1], v1 = r[3];
    return Rec6{r[0], r[2], k1.x, k1.y & 0xFFu, v1.x & 0xFFFFu};
}

template <bool V6>
__global__ __launch_bounds__(RPA_BLOCK) void k_rp_find(RevWriter W, const uint4 *rec, uint32_t n,
                                                        uint32_t *list, uint32_t *cnt)
{
    const uint32_t i = blockIdx.x * RPA_BLOCK + threadIdx.x;
    const bool ok = i < n;
    bool absent = false;
    if (ok) {
        if (V6) {
            const Rec6 r = rp_rec6(rec, i);
            uint32_t s = rp6_hash(r.a.x, r.a.y, r.a.z, r.a.w, r.pt, r.nh) & W.mask;
            for (;; s = (s + 1) & W.mask) {
                const uint4 w = W.tab[2 * (uint64_t)s + 1];
                if (!(w.y & RP_USED)) {
                    absent = true;
                    break;
                }
                if (w.x != r.pt || w.y != (r.nh | RP_USED))
                    continue;
                const uint4 a = W.tab[2 * (uint64_t)s];
                if (a.x == r.a.x && a.y == r.a.y && a.z == r.a.z && a.w == r.a.w)
                    break;
            }
            if (!absent) {
                W.tab[2 * (uint64_t)s + 1].z = r.op;
                reinterpret_cast<uint4 *>(W.val)[s] = r.od;
            }
        } else {
            const Rec4 r = rp_rec4(rec, i);
            uint32_t s = rp4_hash(r.sa, r.pt, r.nh) & W.mask;
            for (;; s = (s + 1) & W.mask) {
                const uint4 w = W.tab[s];
                if (!(w.z & RP_USED)) {
                    absent = true;
                    break;
                }
                if (w.x == r.sa && w.y == r.pt && w.z == (r.nh | RP_USED))
                    break;
            }
            if (!absent) {
                W.tab[s].w = r.od;
                reinterpret_cast<uint32_t *>(W.val)[s] = r.op;
            }
        }
    }
    // cnt[0]: absent keys (the list's length), cnt[1]: keys overwritten
    list_append(list, cnt, absent, i);
    const uint64_t upd = __ballot(ok && !absent);
    if (upd && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(upd))
        atomicAdd(cnt + 1, (uint32_t)__popcll(upd));
}

// (grid-stride over the list's device count: the host does not wait for it)
template <bool V6>
__global__ __launch_bounds__(RPA_BLOCK) void k_rp_insert(RevWriter W, const uint4 *rec,
                                                          const uint32_t *list,
                                                          const uint32_t *cnt)
{
    const uint32_t m = cnt[0];
    for (uint32_t j = blockIdx.x * RPA_BLOCK + threadIdx.x; j < m; j += gridDim.x * RPA_BLOCK) {
        const uint32_t i = list[j];
        if (V6) {
            const Rec6 r = rp_rec6(rec, i);
            uint32_t s = rp6_hash(r.a.x, r.a.y, r.a.z, r.a.w, r.pt, r.nh) & W.mask;
            while (atomicCAS(&W.tab[2 * (uint64_t)s + 1].y, 0u, r.nh | RP_USED) != 0u)
                s = (s + 1) & W.mask;
            W.tab[2 * (uint64_t)s] = r.a;
            W.tab[2 * (uint64_t)s + 1].x = r.pt;
            W.tab[2 * (uint64_t)s + 1].z = r.op;
            reinterpret_cast<uint4 *>(W.val)[s] = r.od;
        } else {
            const Rec4 r = rp_rec4(rec, i);
            uint32_t s = rp4_hash(r.sa, r.pt, r.nh) & W.mask;
            while (atomicCAS(&W.tab[s].z, 0u, r.nh | RP_USED) != 0u)
                s = (s + 1) & W.mask;
            W.tab[s].x = r.sa;
            W.tab[s].y = r.pt;
            W.tab[s].w = r.od;
            reinterpret_cast<uint32_t *>(W.val)[s] = r.op;
        }
    }
}

}  // namespace

int launch_rp_upsert(const RevWriter &W, bool v6, const void *rec, uint32_t n, uint32_t *list,
                     uint32_t *cnt, hipStream_t s)
{
    if (!n)
        return 0;
    const uint4 *r = reinterpret_cast<const uint4 *>(rec);
    const dim3 grid((n + RPA_BLOCK - 1) / RPA_BLOCK), block(RPA_BLOCK);
    if (v6) {
        hipLaunchKernelGGL(k_rp_find<true>, grid, block, 0, s, W, r, n, list, cnt);
        hipLaunchKernelGGL(k_rp_insert<true>, grid, block, 0, s, W, r, list, cnt);
    } else {
        hipLaunchKernelGGL(k_rp_find<false>, grid, block, 0, s, W, r, n, list, cnt);
        hipLaunchKernelGGL(k_rp_insert<false>, grid, block, 0, s, W, r, list, cnt);
    }
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

}  // namespace cfc
