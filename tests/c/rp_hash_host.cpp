// Known answers of the reverse-proxy tables' hashes (cilium_amd/csrc/layout.h
// rp4_hash / rp6_hash) for the Python restatement in tests/rp_table.py: reads
// one key per line from stdin —
//   4 saddr ports nexthdr
//   6 a0 a1 a2 a3 ports nexthdr
// (words in hex) — and prints the hash of each, in hex, one per line.
// Built and run by tests/test_proxy_table_opt.py; no GPU.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "layout.h"

int main()
{
    unsigned fam, w[6];
    while (std::scanf("%u", &fam) == 1) {
        const int n = fam == 4 ? 3 : 6;
        for (int i = 0; i < n; i++)
            if (std::scanf("%x", &w[i]) != 1)
                return 1;
        const uint32_t h = fam == 4 ? cfc::rp4_hash(w[0], w[1], w[2])
                                    : cfc::rp6_hash(w[0], w[1], w[2], w[3], w[4], w[5]);
        std::printf("%08x\n", h);
    }
    return 0;
}
