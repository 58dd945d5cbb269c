// cilium_proxy4 / cilium_proxy6 entries of a classified batch: what
// ipv{4,6}_redirect_to_host_port (bpf/lib/lxc.h:96-191) writes for every
// header the policy sent to the L7 proxy (verdict > 0).
//
// The reference does one map_update_elem per redirected packet, so a key's
// entry ends up as its last packet wrote it.  Here, per batch:
//   count   headers with verdict > 0 (sizes the table; one host wait)
//   mark    every redirected header builds its key; a global open-addressing
//           table keeps per key the greatest header index that wrote it
//           (atomicMax).  A workgroup first dedupes its slice of PX_SLICE
//           contiguous headers in an LDS table, so a hot flow costs one
//           global atomic pair per workgroup, not per packet
//   bits    each occupied slot sets its winner's bit in a bitmap over headers
//   emit    the bitmap compacted in header order (per-group popcounts, one
//           scan block, then the records): no sort
// A slot stores no key: it is claimed with {hash, header index + 1} and a
// probe compares against the claiming header's key, rebuilt from the batch.
// Bytes streamed: count 4 B/header (verdict); mark 4 B/header plus ~25 B
// (IPv4) of header words per redirected header; bits 4 B per table slot;
// emit n/8 B twice plus 32/64 B per record.
#include <cerrno>

#include "kern_common.hpp"

namespace cfc {

namespace {

constexpr int PX_THREADS = 256;
constexpr uint32_t PX_SLICE = 4096;    // headers per workgroup (mark), per group (emit)
constexpr uint32_t PX_ROUND = 4 * PX_THREADS;   // four consecutive headers per thread
constexpr uint32_t PX_LDS = 1024;      // slots of the workgroup's table
constexpr uint32_t PX_PROBES = 8;      // LDS probes before a key goes to the global table

// ---- the entry of header i -------------------------------------------------
// key   {saddr = tuple->daddr, sport = tuple->sport, dport = proxy port,
//        nexthdr} (lxc.h:103-108, 155-160)
// value {orig_daddr = orig_dip, orig_dport = tuple->dport, identity, lifetime}
// ct_lookup4/6 loads the L4 word into {tuple->dport, tuple->sport} and
// reverses the tuple only after its first lookup missed (conntrack.h:540-584):
// CT_NEW / CT_ESTABLISHED have it reversed, CT_REPLY / CT_RELATED do not.
// Key words: the address (1 or 4), dport | sport << 16, nexthdr.
template <bool V6>
struct PxEntry {
    static constexpr int NA = V6 ? 4 : 1;
    uint32_t saddr[NA], ps, proto;      // the key
    uint32_t orig[NA], orig_dport, identity;
};

template <bool V6>
__device__ __forceinline__ void px_addr(const uint32_t *p, uint64_t i, uint32_t *o)
{
    if (V6) {
        const uint4 v = ld16(p + 4 * i);
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else {
        o[0] = p[i];
    }
}

template <bool V6, bool VAL>
__device__ __forceinline__ void px_entry(const ProxyArgs &a, uint64_t i, PxEntry<V6> &e)
{
    constexpr int NA = V6 ? 4 : 1;
    const uint32_t ver = (uint32_t)a.verdict[i];
    const uint32_t ctb = a.ct ? a.ct[i] : 0u;
    const uint32_t proto = a.meta[i] & 0xFF;
    const uint32_t pin = a.ports[i];
    const uint32_t pout = a.pkt_ports ? a.pkt_ports[i] : pin;
    // an egress header whose destination stage ran was redirected by the
    // destination's ipv{4,6}_policy after local delivery (bpf_lxc.c:851,985);
    // otherwise by the egress stage (:280,582)
    const bool dest = a.egress && (ctb & (CFC_CT_DONE << 4));
    const uint32_t res = (dest ? ctb >> 4 : ctb) & CFC_CT_RES_MASK;
    const bool rev = res == CT_NEW || res == CT_ESTABLISHED;
    // the L4 word the stage's ct_lookup loaded: the egress stage runs behind
    // the service translation (the destination port) and before any reverse
    // NAT (the source port); the destination stage sees the packet as left
    const uint32_t pt = !a.egress ? pin
                        : dest    ? pout
                                  : ((pin & 0xFFFFu) | (pout & 0xFFFF0000u));
    uint32_t td, ts;   // tuple->dport / ->sport as loaded
    if (proto == 6 || proto == 17) {
        td = pt & 0xFFFF;
        ts = pt >> 16;
    } else {   // ICMP / ICMPv6 (conntrack.h:339-372, 496-526)
        const uint32_t type = pt & 0xFF;
        const bool related = V6 ? (type >= 1 && type <= 4)
                                : (type == 3 || type == 11 || type == 12);
        const uint32_t echo = V6 ? 128u : 8u, reply = V6 ? 129u : 0u;
        td = (!related && type == reply) ? echo : 0u;
        ts = (!related && type == echo) ? echo : 0u;
    }
    uint32_t sa[NA], da[NA];   // tuple->saddr / ->daddr as the stage set them
    px_addr<V6>(a.saddr, i, sa);
    px_addr<V6>(a.daddr, i, da);
    if (a.egress && (a.pkt_daddr || a.pkt_saddr)) {
        uint32_t psa[NA], pda[NA];
        px_addr<V6>(a.pkt_saddr ? a.pkt_saddr : a.saddr, i, psa);
        px_addr<V6>(a.pkt_daddr ? a.pkt_daddr : a.daddr, i, pda);
        if (V6) {
            // lb6_local rewrites tuple->daddr only; the destination's
            // ipv6_policy clears the address's reverse-NAT bits after it
            // copied orig_dip (bpf_lxc.c:775-795): a destination that differs
            // from the input in those bits alone is the input's
            const bool same = dest && pda[0] == da[0] && pda[1] == da[1] && pda[2] == da[2] &&
                              ((pda[3] ^ da[3]) & 0xFFFF0000u) == 0;
            if (!same) {
#pragma unroll
                for (int j = 0; j < NA; j++)
                    da[j] = pda[j];
            }
        } else if (dest) {
            sa[0] = psa[0];   // as delivered (a looped-back flow: IPV4_LOOPBACK)
            da[0] = pda[0];
        } else {
            // lb4_local leaves tuple->daddr alone for a flow looped back into
            // its sender (lb.h:761-770: the packet's source becomes
            // IPV4_LOOPBACK); a reply's reverse NAT (lb4_rev_nat, after the
            // lookup) rewrites the packet, not orig_dip
            const bool rewritten = psa[0] != sa[0] || (!rev && (pout & 0xFFFFu) != (pin & 0xFFFFu));
            if (!rewritten)
                da[0] = pda[0];
        }
    }
#pragma unroll
    for (int j = 0; j < NA; j++)
        e.saddr[j] = rev ? sa[j] : da[j];
    e.ps = (ver & 0xFFFFu) | (rev ? td : ts) << 16;
    e.proto = proto;
    if (VAL) {
#pragma unroll
        for (int j = 0; j < NA; j++)
            e.orig[j] = da[j];
        e.orig_dport = rev ? ts : td;
        e.identity = a.egress ? a.own_seclabel : a.identity[i];
    }
}

template <bool V6>
__device__ __forceinline__ uint32_t px_hash(const PxEntry<V6> &e)
{
    uint32_t h = fmix32(e.ps * 0x9E3779B1u + e.proto);
#pragma unroll
    for (int j = 0; j < (V6 ? 4 : 1); j++)
        h = fmix32(e.saddr[j] + h * 0x85EBCA77u);
    return h;
}

template <bool V6>
__device__ __forceinline__ bool px_same(const PxEntry<V6> &x, const PxEntry<V6> &y)
{
    bool eq = x.ps == y.ps && x.proto == y.proto;
#pragma unroll
    for (int j = 0; j < (V6 ? 4 : 1); j++)
        eq = eq && x.saddr[j] == y.saddr[j];
    return eq;
}

// key e (hash h) was written by header `lastidx`: claim or find its slot and
// raise the slot's last writer.  rep: a header that has the key (the claim).
// The table holds at most half as many keys as slots, so a free slot exists.
template <bool V6>
__device__ __forceinline__ void px_insert(const ProxyArgs &a, const ProxyWs &w,
                                          const PxEntry<V6> &e, uint32_t h, uint32_t rep,
                                          uint32_t lastidx)
{
    const unsigned long long mine = ((unsigned long long)h << 32) | (rep + 1u);
    uint32_t s = h & w.mask;
    for (uint32_t p = 0; p <= w.mask; p++, s = (s + 1) & w.mask) {
        const unsigned long long old = atomicCAS(&w.own[s], 0ull, mine);
        if (old != 0) {
            if ((uint32_t)(old >> 32) != h)
                continue;
            PxEntry<V6> o;
            px_entry<V6, false>(a, (uint32_t)old - 1u, o);
            if (!px_same<V6>(e, o))
                continue;
        }
        atomicMax(&w.last[s], lastidx + 1u);
        return;
    }
}

__global__ __launch_bounds__(PX_THREADS) void k_px_count(const int32_t *verdict, uint64_t n,
                                                         unsigned long long *total)
{
    const uint64_t base = (uint64_t)blockIdx.x * PX_SLICE;
    const bool v16 = (reinterpret_cast<uintptr_t>(verdict) & 15) == 0;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t r = 0; r < PX_SLICE / PX_ROUND; r++) {
        const uint64_t i0 = base + r * PX_ROUND + 4 * threadIdx.x;
        if (v16 && i0 + 4 <= n) {
            const int4 q = *reinterpret_cast<const int4 *>(verdict + i0);
            c += (q.x > 0) + (q.y > 0) + (q.z > 0) + (q.w > 0);
        } else {
            for (uint32_t j = 0; j < 4; j++)
                c += (i0 + j < n && verdict[i0 + j] > 0) ? 1u : 0u;
        }
    }
    for (int o = 32; o > 0; o >>= 1)
        c += __shfl_xor(c, o);
    __shared__ uint32_t s[PX_THREADS / 64];
    if ((threadIdx.x & 63) == 0)
        s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int v = 0; v < PX_THREADS / 64; v++)
            t += s[v];
        if (t)
            atomicAdd(total, (unsigned long long)t);
    }
}

template <bool V6>
__global__ __launch_bounds__(PX_THREADS) void k_px_mark(ProxyArgs a, ProxyWs w)
{
    constexpr int NW = V6 ? 6 : 3;
    __shared__ uint32_t l_tag[PX_LDS], l_last[PX_LDS], l_key[PX_LDS * NW];
    const uint32_t tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * PX_SLICE;
    if (a.predup) {
        for (uint32_t s = tid; s < PX_LDS; s += PX_THREADS) {
            l_tag[s] = 0;
            l_last[s] = 0;
        }
        __syncthreads();
    }
    const bool v16 = (reinterpret_cast<uintptr_t>(a.verdict) & 15) == 0;
    for (uint32_t r = 0; r < PX_SLICE / PX_ROUND; r++) {
        const uint32_t l0 = r * PX_ROUND + 4 * tid;   // index within the slice
        const uint64_t i0 = base + l0;
        uint32_t m = 0;
        if (v16 && i0 + 4 <= a.n) {
            const int4 q = *reinterpret_cast<const int4 *>(a.verdict + i0);
            m = (q.x > 0) | (q.y > 0) << 1 | (q.z > 0) << 2 | (q.w > 0) << 3;
        } else {
            for (uint32_t j = 0; j < 4; j++)
                m |= (i0 + j < a.n && a.verdict[i0 + j] > 0) ? 1u << j : 0u;
        }
        if (!a.predup) {
            for (uint32_t j = 0; j < 4; j++) {
                if (!((m >> j) & 1))
                    continue;
                PxEntry<V6> e;
                px_entry<V6, false>(a, i0 + j, e);
                px_insert<V6>(a, w, e, px_hash<V6>(e), (uint32_t)(i0 + j), (uint32_t)(i0 + j));
            }
            continue;
        }
        if (!__syncthreads_or((int)m))
            continue;
        for (uint32_t j = 0; j < 4; j++) {
            const bool act = (m >> j) & 1;
            PxEntry<V6> e;
            uint32_t h = 0, slot = NONE;
            bool owner = false;
            if (act) {
                px_entry<V6, false>(a, i0 + j, e);
                h = px_hash<V6>(e);
                const uint32_t tag = h | 1u;
                for (uint32_t p = 0; p < PX_PROBES; p++) {
                    const uint32_t s = (h + p) & (PX_LDS - 1);
                    const uint32_t old = atomicCAS(&l_tag[s], 0u, tag);
                    if (old == 0 || old == tag) {
                        slot = s;
                        owner = old == 0;
                        break;
                    }
                }
            }
            __syncthreads();
            if (owner) {
#pragma unroll
                for (int k = 0; k < NW - 2; k++)
                    l_key[slot * NW + k] = e.saddr[k];
                l_key[slot * NW + NW - 2] = e.ps;
                l_key[slot * NW + NW - 1] = e.proto;
            }
            __syncthreads();
            if (act) {
                bool eq = slot != NONE && l_key[slot * NW + NW - 2] == e.ps &&
                          l_key[slot * NW + NW - 1] == e.proto;
#pragma unroll
                for (int k = 0; k < NW - 2; k++)
                    eq = eq && l_key[(slot == NONE ? 0 : slot) * NW + k] == e.saddr[k];
                if (eq)   // a larger index within the slice is a later packet
                    atomicMax(&l_last[slot], l0 + j + 1u);
                else      // no LDS slot within the probe limit, or a tag shared by two keys
                    px_insert<V6>(a, w, e, h, (uint32_t)(i0 + j), (uint32_t)(i0 + j));
            }
        }
    }
    if (!a.predup)
        return;
    __syncthreads();
    // the workgroup's survivors into the global table
    for (uint32_t s = tid; s < PX_LDS; s += PX_THREADS) {
        const uint32_t lw = l_last[s];
        if (!lw)
            continue;
        PxEntry<V6> e;
#pragma unroll
        for (int k = 0; k < NW - 2; k++)
            e.saddr[k] = l_key[s * NW + k];
        e.ps = l_key[s * NW + NW - 2];
        e.proto = l_key[s * NW + NW - 1];
        const uint32_t idx = (uint32_t)(base + lw - 1u);
        px_insert<V6>(a, w, e, px_hash<V6>(e), idx, idx);
    }
}

// each occupied slot's last writer is its key's winner
__global__ __launch_bounds__(PX_THREADS) void k_px_bits(ProxyWs w, uint64_t n)
{
    const uint64_t s = (uint64_t)blockIdx.x * PX_THREADS + threadIdx.x;
    if (s > w.mask)
        return;
    const uint32_t lw = w.last[s];
    if (lw && (uint64_t)(lw - 1u) < n)
        atomicOr(reinterpret_cast<uint32_t *>(w.bitmap) + ((lw - 1u) >> 5), 1u << ((lw - 1u) & 31));
}

// winners per group of PX_SLICE headers (64 bitmap words: one wave)
__global__ __launch_bounds__(PX_THREADS) void k_px_groups(const uint64_t *bitmap, uint64_t groups,
                                                          uint64_t *blk)
{
    const uint64_t g = (uint64_t)blockIdx.x * (PX_THREADS / 64) + (threadIdx.x >> 6);
    if (g >= groups)   // (whole waves)
        return;
    uint32_t c = __popcll(bitmap[g * 64 + (threadIdx.x & 63)]);
    for (int o = 32; o > 0; o >>= 1)
        c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0)
        blk[g] = c;
}

// exclusive scan of nb group counts in place (one 1024-thread block), total
// into *count (as notify.hip k_nt_scan)
__global__ __launch_bounds__(1024) void k_px_scan(uint64_t *blk, uint64_t nb, uint64_t *count)
{
    __shared__ uint64_t s[1024];
    const uint64_t per = (nb + 1023) / 1024;
    const uint64_t b0 = min(nb, threadIdx.x * per), b1 = min(nb, b0 + per);
    uint64_t sum = 0;
    for (uint64_t b = b0; b < b1; b++)
        sum += blk[b];
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint64_t v = threadIdx.x >= (unsigned)o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = s[threadIdx.x] - sum;
    for (uint64_t b = b0; b < b1; b++) {
        const uint64_t v = blk[b];
        blk[b] = run;
        run += v;
    }
    if (threadIdx.x == 1023)
        *count = s[1023];
}

// one workgroup per group; each wave writes the records of 16 bitmap words
template <bool V6>
__global__ __launch_bounds__(PX_THREADS) void k_px_write(ProxyArgs a, ProxyWs w)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t g = blockIdx.x;
    const uint64_t mine = w.bitmap[g * 64 + lane];
    // exclusive prefix of the words' popcounts over the lanes
    uint32_t inc = __popcll(mine);
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o);
        inc += lane >= (uint32_t)o ? v : 0u;
    }
    const uint32_t exc = inc - (uint32_t)__popcll(mine);
    const uint64_t goff = w.blk[g];
    for (uint32_t k = 0; k < 16; k++) {
        const int j = (int)(wave * 16 + k);
        const uint64_t word = __shfl(mine, j);
        const uint32_t before = __shfl(exc, j);
        const uint64_t pos = goff + before + __popcll(word & ((1ull << lane) - 1));
        if (!((word >> lane) & 1) || pos >= a.cap)
            continue;
        const uint64_t i = g * PX_SLICE + (uint64_t)j * 64 + lane;
        PxEntry<V6> e;
        px_entry<V6, true>(a, i, e);
        if (V6) {
            uint4 *p = reinterpret_cast<uint4 *>(a.rec) + 4 * pos;
            p[0] = make_uint4(e.saddr[0], e.saddr[V6 ? 1 : 0], e.saddr[V6 ? 2 : 0],
                              e.saddr[V6 ? 3 : 0]);
            p[1] = make_uint4(e.ps, e.proto, 0u, 0u);
            p[2] = make_uint4(e.orig[0], e.orig[V6 ? 1 : 0], e.orig[V6 ? 2 : 0],
                              e.orig[V6 ? 3 : 0]);
            p[3] = make_uint4(e.orig_dport, e.identity, a.lifetime, 0u);
        } else {
            uint4 *p = reinterpret_cast<uint4 *>(a.rec) + 2 * pos;
            p[0] = make_uint4(e.saddr[0], e.ps, e.proto, 0u);
            p[1] = make_uint4(e.orig[0], e.orig_dport, e.identity, a.lifetime);
        }
        if (a.hdr_index)
            a.hdr_index[pos] = i;
    }
}

}  // namespace

uint64_t proxy_groups(uint64_t n)
{
    return (n + PX_SLICE - 1) / PX_SLICE;
}

size_t proxy_bitmap_bytes(uint64_t n)
{
    return proxy_groups(n) * (PX_SLICE / 8);
}

int launch_proxy_count(const ProxyArgs &a, unsigned long long *total, hipStream_t s)
{
    const uint64_t nb = proxy_groups(a.n);
    if (nb == 0)
        return 0;
    if (nb > 0x7FFFFFFFull || a.n > 0xFFFFFFFEull)   // header index + 1 in 32 bits
        return -E2BIG;
    k_px_count<<<(uint32_t)nb, PX_THREADS, 0, s>>>(a.verdict, a.n, total);
    return hipGetLastError() == hipSuccess ? 0 : -EINVAL;
}

int launch_proxy_mark(int family, const ProxyArgs &a, const ProxyWs &w, hipStream_t s)
{
    const uint64_t nb = proxy_groups(a.n);
    if (nb == 0 || nb > 0x7FFFFFFFull || a.n > 0xFFFFFFFEull)
        return -EINVAL;
    if (family == 6)
        k_px_mark<true><<<(uint32_t)nb, PX_THREADS, 0, s>>>(a, w);
    else
        k_px_mark<false><<<(uint32_t)nb, PX_THREADS, 0, s>>>(a, w);
    const uint64_t slots = (uint64_t)w.mask + 1;
    k_px_bits<<<(uint32_t)((slots + PX_THREADS - 1) / PX_THREADS), PX_THREADS, 0, s>>>(w, a.n);
    constexpr uint64_t per = PX_THREADS / 64;
    k_px_groups<<<(uint32_t)((nb + per - 1) / per), PX_THREADS, 0, s>>>(w.bitmap, nb, w.blk);
    k_px_scan<<<1, 1024, 0, s>>>(w.blk, nb, a.count);
    return hipGetLastError() == hipSuccess ? 0 : -EINVAL;
}

int launch_proxy_write(int family, const ProxyArgs &a, const ProxyWs &w, hipStream_t s)
{
    const uint64_t nb = proxy_groups(a.n);
    if (nb == 0 || nb > 0x7FFFFFFFull)
        return -EINVAL;
    if (family == 6)
        k_px_write<true><<<(uint32_t)nb, PX_THREADS, 0, s>>>(a, w);
    else
        k_px_write<false><<<(uint32_t)nb, PX_THREADS, 0, s>>>(a, w);
    return hipGetLastError() == hipSuccess ? 0 : -EINVAL;
}

}  // namespace cfc
