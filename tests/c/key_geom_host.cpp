// Host check of the compact key streams' geometry (cilium_amd/csrc/classify.hpp
// key_per_block / key_regions): for every batch size and device width the
// classify kernel's regions are disjoint, lie inside the sized key array, hold
// every position their wave handles, and the count array covers them all.
// Built and run by tests/test_key_geometry.py; no GPU.
#include <cstdint>
#include <cstdio>

#include "classify.hpp"

using namespace cfc;

static int fails;
#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            if (fails++ < 20)                                                      \
                std::printf("FAIL n=%llu cus=%d: %s\n", (unsigned long long)n, cus, #c); \
        }                                                                          \
    } while (0)

static void check(uint64_t n, int cus, uint64_t wg_per_cu, uint64_t unroll)
{
    const uint64_t step = (uint64_t)BLOCK * unroll;
    const uint64_t per_block = key_per_block(n, (uint64_t)cus * wg_per_cu, step);
    CHECK(per_block > 0 && per_block % step == 0 && per_block < (1ull << 30) + step);
    const uint64_t grid = (n + per_block - 1) / per_block;
    const KeyRegions G = key_regions(n, per_block);
    const KeyRegions K = key_regions_grid(grid, per_block);   // the kernel's view
    CHECK(G.extent == K.extent && G.cap == K.cap && G.regions == K.regions);
    // every header has a workgroup, and every workgroup at least one header
    CHECK(grid * per_block >= n && (grid - 1) * per_block < n);
    CHECK(G.extent == grid * per_block);
    // a wave handles 64 positions of every BLOCK positions of the slice
    const uint64_t wave_positions = per_block / BLOCK * 64;
    CHECK(G.cap >= wave_positions);
    CHECK(G.cap % 4 == 0);   // k_hist's 16-byte steps never span two regions
    CHECK(G.regions == grid * KEY_WAVES);
    uint64_t prev_end = 0;
    for (uint64_t g = 0; g < grid; g++) {
        for (uint32_t w = 0; w < KEY_WAVES; w++) {
            const uint32_t r = (uint32_t)(g * KEY_WAVES + w);   // the kernel's count index
            CHECK(r < G.regions);
            const uint64_t b = G.base(r);
            CHECK(b >= prev_end);                      // disjoint, in order
            CHECK(b + G.cap <= G.extent);              // inside the regions' extent
            CHECK(b >= g * per_block && b + G.cap <= (g + 1) * per_block);
            // the flat position space maps back to (region, offset)
            CHECK(b / G.cap == r && (b + G.cap - 1) / G.cap == r);
            prev_end = b + G.cap;
        }
    }
    // counts behind the regions, all inside the sized array
    CHECK(G.counts() >= prev_end);
    CHECK(G.counts() + G.regions <= G.words());
    CHECK(G.words() % 4 == 0);
}

int main()
{
    const uint64_t ns[] = {1, 64, 1024, 1025, 70000, 1ull << 26, (1ull << 26) + 5};
    const int cus[] = {1, 8, 256};
    for (uint64_t n : ns)
        for (int c : cus)
            for (uint64_t unroll : {1ull, 2ull})
                check(n, c, 2, unroll);
    // (a slice is capped below 2^30 headers: more workgroups than the device has)
    check(1ull << 32, 1, 1, 1);
    if (fails) {
        std::printf("key_geom_host: %d failures\n", fails);
        return 1;
    }
    std::printf("key_geom_host: ok\n");
    return 0;
}
