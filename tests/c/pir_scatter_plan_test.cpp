// pir_scatter_plan_test.cpp — the private write's launch plan
// (dpf-go_amd/csrc/pir_scatter_plan.hpp) as a stand-alone program: over a grid
// of shapes and limits the planned (super-group run, column group, key tile)
// units cover every (super-group, column, key) exactly once and no unit or
// launch exceeds its limit.  Built with -fsanitize=address,undefined and run
// directly by tests/test_pir_write_cpu.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pir_scatter_plan.hpp"

using namespace dpfh;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++g_fail <= 20) {                          \
                printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
                printf(__VA_ARGS__);                       \
                printf("\n");                              \
            }                                              \
        }                                                  \
    } while (0)

static void check(uint64_t nrec, uint32_t C, uint64_t nkeys, uint32_t cus, uint32_t max_blocks, uint32_t max_sg) {
    const ScatterPlan p = plan_scatter(nrec, C, nkeys, cus, max_blocks, max_sg);
    const uint64_t nsg = (nrec + 255) / 256;
    const uint64_t cap = max_blocks ? max_blocks : kFoldMaxBlocks;
    const uint64_t msg = max_sg ? max_sg : kFoldMaxSg;
    const uint64_t tiles = p.key_tiles();
#define AT "nrec=%llu C=%u nkeys=%llu blocks=%u sg=%u", (unsigned long long)nrec, C, (unsigned long long)nkeys, max_blocks, max_sg
    if (nsg == 0 || nkeys == 0) {
        CHECK(p.units == 0 && tiles == 0 && p.launches() == 0, AT);
        return;
    }
    CHECK(p.nsg == nsg && p.C == C && p.nkeys == nkeys, AT);
    CHECK(tiles == (nkeys + kScatterKeyTile - 1) / kScatterKeyTile, AT);
    CHECK(p.units > 0 && p.per_launch >= 1 && p.per_launch <= cap, AT);
    // The launches are consecutive ranges of the workgroups, none over the cap.
    uint64_t next = 0;
    for (uint64_t l = 0; l < p.launches(); ++l) {
        CHECK(p.first(l) == next, AT);
        CHECK(p.blocks(l) >= 1 && p.blocks(l) <= cap, AT);
        next += p.blocks(l);
    }
    CHECK(next == p.units, AT);
    // Every cell once: a counter per (S, c, k) where that is small enough ...
    const uint64_t cells = nsg * C * nkeys;
    const bool exhaustive = cells <= (1ull << 23);
    std::vector<uint8_t> cnt(exhaustive ? cells : 0);
    // ... and always the walk: within a key tile the units, in launch order,
    // tile the (S, c) plane row by row, and the key tiles follow one another.
    uint64_t k_at = 0;
    for (uint64_t t = 0; t < tiles; ++t) {
        uint64_t s_at = 0, s_end = 0;
        uint32_t c_at = C;                         // "row finished"
        uint64_t k0 = 0, k1 = 0;
        if (t > 0 && p.units > (1u << 20)) {
            // Millions of workgroups per key tile (the 2^24-record shapes under
            // max_sg 1 or 5): the first tile is walked in full below, a later
            // one is compared with it at every 4099th workgroup and at the ends.
            for (uint64_t u = 0; u < p.units; u = u + 4099 < p.units || u == p.units - 1 ? u + 4099 : p.units - 1) {
                const ScatterUnit a = p.unit(0, u), x = p.unit(t, u);
                CHECK(x.s0 == a.s0 && x.s1 == a.s1 && x.c0 == a.c0 && x.c1 == a.c1, AT);
                CHECK(x.k0 == k_at && x.k1 > x.k0 && x.k1 <= nkeys && x.k1 - x.k0 <= kScatterKeyTile, AT);
                CHECK(u == 0 || (x.k0 == k0 && x.k1 == k1), AT);
                k0 = x.k0;
                k1 = x.k1;
            }
            k_at = k1;
            continue;
        }
        for (uint64_t u = 0; u < p.units; ++u) {
            const ScatterUnit x = p.unit(t, u);
            if (u == 0) {
                k0 = x.k0;
                k1 = x.k1;
                CHECK(k0 == k_at && k1 > k0 && k1 <= nkeys && k1 - k0 <= kScatterKeyTile, AT);
            }
            CHECK(x.k0 == k0 && x.k1 == k1, AT);
            CHECK(x.s0 < x.s1 && x.s1 <= nsg && x.s1 - x.s0 <= msg, AT);
            CHECK(x.c0 < x.c1 && x.c1 <= C && x.c1 - x.c0 <= kScatterMaxCols && x.c1 - x.c0 <= p.cols, AT);
            if (c_at == C) {                       // a new row of column groups starts where the last one ended
                CHECK(x.s0 == s_end && x.c0 == 0, AT);
                s_at = x.s0;
                s_end = x.s1;
            } else {
                CHECK(x.s0 == s_at && x.s1 == s_end && x.c0 == c_at, AT);
            }
            c_at = x.c1;
            if (exhaustive)
                for (uint64_t S = x.s0; S < x.s1; ++S)
                    for (uint32_t c = x.c0; c < x.c1; ++c)
                        for (uint64_t k = x.k0; k < x.k1; ++k) {
                            uint8_t& n = cnt[(S * C + c) * nkeys + k];
                            if (n < 255) ++n;
                        }
        }
        CHECK(c_at == C && s_end == nsg, AT);
        k_at = k1;
    }
    CHECK(k_at == nkeys, AT);
    for (uint64_t i = 0; i < cnt.size(); ++i)
        if (cnt[i] != 1) {
            CHECK(cnt[i] == 1, AT);
            break;
        }
#undef AT
}

int main() {
    const uint64_t nrecs[] = {0, 1, 255, 256, 257, 5000, (1ull << 24) + (1ull << 21)};
    const uint32_t Cs[] = {1, 2, 3, 5, 32, 1024};
    const uint64_t nks[] = {0, 1, 63, 64, 65, 130, 300};
    const uint32_t blocks[] = {1, 3, 0};
    const uint32_t sgs[] = {1, 5, 0};
    uint64_t n = 0;
    for (uint64_t nrec : nrecs)
        for (uint32_t C : Cs)
            for (uint64_t nk : nks)
                for (uint32_t mb : blocks)
                    for (uint32_t ms : sgs) {
                        check(nrec, C, nk, 256, mb, ms);
                        ++n;
                    }
    // Other CU budgets (a CU-masked stream, a small part): the same properties.
    for (uint32_t cus : {1u, 7u, 304u})
        for (uint64_t nrec : {257ull, 70000ull})
            for (uint32_t C : {1u, 5u}) check(nrec, C, 65, cus, 0, 0);
    // The flagship shape in one launch of four workgroups per CU.
    const ScatterPlan p = plan_scatter(1ull << 24, 1, 64, 256, 0, 0);
    CHECK(p.launches() == 1 && p.units == 1024 && p.run == 64 && p.cols == 1, "flagship plan");
    if (g_fail) {
        printf("pir_scatter_plan: %d failures\n", g_fail);
        return 1;
    }
    printf("pir_scatter_plan ok (%llu shapes)\n", (unsigned long long)n);
    return 0;
}
