// reverse_proxy / reverse_proxy6 of a from-host batch (bpf_netdev.c:293-354,
// :67-124, called from handle_ipv4 :400-416 and handle_ipv6 :218-234): the L7
// proxy's own packets towards an endpoint get the source address and port of
// the connection the proxy stands in for, from the cilium_proxy4 /
// cilium_proxy6 entry the redirect wrote (cfc_proxy_apply_*).
//
// One streaming pass in front of the INGRESS classify launch
// (cfc_classify_from_host_*), one header per lane and RP_U of them in flight
// per iteration.  Per header it reads daddr, the L4 word and meta (non-temporal: nothing reads them
// again before the classify kernel streams them itself) and probes the
// family's table (layout.h RevTables: one 16-byte load per probe for IPv4,
// two for IPv6).  Most from-host headers miss and touch nothing else.  A hit
// reads the source address and the mark, settles the source identity as
// handle_identity_from_host and handle_ipv4 / handle_ipv6 do BEFORE the
// rewrite — from the mark, a reserved one overridden by the ipcache label of
// the original source — and writes the translated source, L4 word, mark and
// that identity.  Hits are rare, so their LPM lookups take the global-memory
// paths (no LDS images of the tables; IPv6 keeps the length list in LDS, as
// lpm6_lookup reads it from there).
#include "kern_common.hpp"

namespace cfc {
namespace {

constexpr int RP_BLOCK = 256;
constexpr uint32_t RP_HIT_MARK = 0xA00u | CFC_MARK_TRANSLATED;

// the ipcache label of an IPv4 source (be32 raw), 0 = none: the compact
// layout or DIR-24-8, as classify.hip's rounds 2 and 3 walk them
__device__ __forceinline__ uint32_t rp_label4(const DevTables &T, uint32_t sa)
{
    const uint32_t lh = __builtin_bswap32(sa);
    if (T.l4d)
        return l4_lookup(T, lh, ldt16(T.l4d, (lh >> T.l4_shift) * 16u));
    if (!T.tbl24)
        return 0;
    uint32_t e = T.tbl24[lh >> 8];
    if (e & LPM_GROUP)
        e = T.tbl8[((e & ~LPM_GROUP) << 8) | (lh & 0xFF)];
    if (e & LPM_INDIRECT)
        e = T.lbl_ovf[e & LPM_PAYLOAD];
    return e;
}

// handle_identity_from_host (bpf_netdev.c:128-153), then the override of
// handle_ipv4 (:375-398: labels 0, CLUSTER_ID and HOST_ID ignored) or
// handle_ipv6 (:203-213: labels 0 and CLUSTER_ID ignored)
template <bool V6>
__device__ __forceinline__ uint32_t rp_identity(uint32_t mk, uint32_t label)
{
    const uint32_t magic = mk & 0xF00u;
    const bool viap = (magic == 0xA00u) | (magic == 0xB00u);
    const uint32_t id = viap ? (((mk & 0xFF) << 16) | (mk >> 16))
                             : (magic == 0xC00u ? HOST_ID : WORLD_ID);
    const bool ovr = (id < HEALTH_ID) & (label != 0u) & (label != CLUSTER_ID) &
                     (V6 | (label != HOST_ID));
    return ovr ? label : id;
}

// U headers per lane per iteration: their streaming loads go out together,
// then their first probes, so a lane has U independent chains in flight (a
// single chain per lane left the pass latency-bound at a quarter of what the
// same bytes stream at; DESIGN.md section 4 "Reverse proxy")
constexpr int RP_U = 4;

template <bool V6>
__global__ __launch_bounds__(RP_BLOCK) void k_revproxy(DevTables T, RevTables R, RevArgs A)
{
    __shared__ uint32_t s_hits;
    if (threadIdx.x == 0)
        s_hits = 0;
    if (V6) {   // the ipcache's length list, where lpm6_lookup reads it (dword 0)
        uint32_t *lw = reinterpret_cast<uint32_t *>(cfc_smem);
        for (uint32_t j = threadIdx.x; j < T.ipc6.nlen; j += RP_BLOCK)
            lw[j] = T.ipc6.lens[j];
    }
    __syncthreads();
    const uint32_t *sa_in = reinterpret_cast<const uint32_t *>(A.sa);
    const uint32_t *da_in = reinterpret_cast<const uint32_t *>(A.da);
    uint32_t *osa = reinterpret_cast<uint32_t *>(A.osa);
    // (uniform) a column that is its input is written on hit rows only
    const bool cp_sa = A.osa != A.sa, cp_pt = A.opt != A.pt, cp_mk = A.omk != A.mk;
    const bool table = V6 ? R.rp6 != nullptr : R.rp4 != nullptr;
    const uint32_t mask = V6 ? R.rp6_mask : R.rp4_mask;
    const uint64_t stride = (uint64_t)gridDim.x * RP_BLOCK * RP_U;
    uint32_t nh = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * RP_BLOCK * RP_U + threadIdx.x; base < A.n;
         base += stride) {
        // lanes past the end take the last header and write nothing
        uint64_t idx[RP_U];
        bool ok[RP_U], l4[RP_U];
        uint32_t pt[RP_U], mt[RP_U], slot[RP_U];
        uint4 da[RP_U], k[RP_U];   // (IPv4: da.x; k: the first probe's load)
#pragma unroll
        for (int u = 0; u < RP_U; u++) {
            const uint64_t i = base + (uint64_t)u * RP_BLOCK;
            ok[u] = i < A.n;
            idx[u] = ok[u] ? i : A.n - 1;
            pt[u] = ld_nt(A.pt + idx[u]);
            mt[u] = ld_nt(A.mt + idx[u]);
            da[u] = V6 ? ld_nt4(da_in + 4 * idx[u])
                       : make_uint4(ld_nt(da_in + idx[u]), 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < RP_U; u++) {
            const uint32_t proto = mt[u] & 0xFF;
            // TCP and UDP only; IPv6 by the first next header (ip6->nexthdr)
            l4[u] = table && (proto == 6u || proto == 17u) &&
                    !(V6 && (mt[u] & CFC_HF_EXTHDR));
            slot[u] = (V6 ? rp6_hash(da[u].x, da[u].y, da[u].z, da[u].w, pt[u], proto)
                          : rp4_hash(da[u].x, pt[u], proto)) & mask;
            k[u] = make_uint4(0, 0, 0, 0);
            if (l4[u])
                k[u] = V6 ? ldt16(R.rp6, slot[u] * 32u + 16u) : ldt16(R.rp4, slot[u] * 16u);
        }
#pragma unroll
        for (int u = 0; u < RP_U; u++) {
            const uint64_t i = idx[u];
            const uint32_t proto = mt[u] & 0xFF;
            bool hit = false;
            uint32_t s = slot[u];
            uint4 w = k[u];
            if (V6) {
                // w: {ports, nexthdr | RP_USED, orig_dport, 0} of slot s
                while (l4[u] && (w.y & RP_USED)) {
                    if (w.x == pt[u] && w.y == (proto | RP_USED)) {
                        const uint4 a = ldt16(R.rp6, s * 32u);
                        if (a.x == da[u].x && a.y == da[u].y && a.z == da[u].z &&
                            a.w == da[u].w) {
                            hit = true;
                            break;
                        }
                    }
                    s = (s + 1) & mask;
                    w = ldt16(R.rp6, s * 32u + 16u);
                }
                if (hit && ok[u]) {
                    const uint4 od = ld16(R.rp6_val + s);
                    const uint4 sa = bswap4(ld_nt4(sa_in + 4 * i));
                    const uint32_t mk = A.mk ? A.mk[i] : 0u;
                    const uint32_t label = lpm6_lookup(T.ipc6, 0, sa);
                    *reinterpret_cast<uint4 *>(osa + 4 * i) = od;
                    A.opt[i] = (pt[u] & 0xFFFF0000u) | (w.z & 0xFFFFu);
                    A.omk[i] = RP_HIT_MARK;
                    A.oid[i] = rp_identity<true>(mk, label);
                    nh++;
                } else if (cp_sa && ok[u]) {
                    *reinterpret_cast<uint4 *>(osa + 4 * i) = ld_nt4(sa_in + 4 * i);
                }
            } else {
                // w: {saddr, ports, nexthdr | RP_USED, orig_daddr} of slot s
                while (l4[u] && (w.z & RP_USED)) {
                    if (w.x == da[u].x && w.y == pt[u] && w.z == (proto | RP_USED)) {
                        hit = true;
                        break;
                    }
                    s = (s + 1) & mask;
                    w = ldt16(R.rp4, s * 16u);
                }
                if (hit && ok[u]) {
                    const uint32_t sa = sa_in[i];
                    const uint32_t mk = A.mk ? A.mk[i] : 0u;
                    const uint32_t label = rp_label4(T, sa);
                    osa[i] = w.w;
                    A.opt[i] = (pt[u] & 0xFFFF0000u) | (R.rp4_val[s] & 0xFFFFu);
                    A.omk[i] = RP_HIT_MARK;
                    A.oid[i] = rp_identity<false>(mk, label);
                    nh++;
                } else if (cp_sa && ok[u]) {
                    osa[i] = ld_nt(sa_in + i);
                }
            }
            if (!hit && ok[u]) {
                if (cp_pt)
                    A.opt[i] = pt[u];
                if (cp_mk)
                    A.omk[i] = A.mk ? ld_nt(A.mk + i) : 0u;
            }
        }
    }
    // the hit count: one global atomic per workgroup (none without a hit)
    if (A.hits) {
        if (nh)
            atomicAdd(&s_hits, nh);
        __syncthreads();
        if (threadIdx.x == 0 && s_hits)
            atomicAdd(A.hits, (unsigned long long)s_hits);
    }
}

}  // namespace

int launch_revproxy(const DevTables &T, const RevTables &R, const RevArgs &A, bool v6,
                    int num_cus, hipStream_t s)
{
    if (!A.n)
        return 0;
    const uint64_t want = (A.n + (uint64_t)RP_BLOCK * RP_U - 1) / ((uint64_t)RP_BLOCK * RP_U);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)num_cus * 8);
    if (v6)
        hipLaunchKernelGGL(k_revproxy<true>, dim3(grid), dim3(RP_BLOCK),
                           4 * ((T.ipc6.nlen + 3) & ~3u), s, T, R, A);
    else
        hipLaunchKernelGGL(k_revproxy<false>, dim3(grid), dim3(RP_BLOCK), 0, s, T, R, A);
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

}  // namespace cfc
