// pir_group_plan_test.cpp — the grouped layout rule and the grouped fold's
// launch plan (dpf-go_amd/csrc/pir_group_plan.hpp) as a stand-alone program.
// Over ngroups x gsg x C x kpg x CU counts x limits every plan folds each
// (group, super-group, column, key) cell exactly once, has no empty run and no
// run across a group boundary, keeps every launch inside the workgroup cap and
// the grid's x dimension, and writes no more scratch than the size function
// promises.  Cells are counted one by one where a shape has at most 2^21
// (group, super-group, column) triples; every shape is also walked run by run
// (each run must start where the previous run of its group and column ended,
// and the last must end at gsg), which is the same statement without a byte
// per cell: the largest shape here has 10^9 triples.  Then group_stride /
// group_flat and the grouped update split at a shard edge.  Built with
// -fsanitize=address,undefined and run directly by tests/test_group_plan_cpu.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pir_group_plan.hpp"

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

typedef unsigned long long ull;
static uint64_t g_plans = 0, g_launches = 0, g_exhaustive = 0;

constexpr uint64_t kGridX = (1ull << 31) - 1;   // HIP's bound on gridDim.x

static void check_plan(uint64_t ngroups, uint64_t gsg, uint32_t C, uint32_t kpg, uint64_t cus, uint32_t max_blocks) {
#define AT "ngroups=%llu gsg=%llu C=%u kpg=%u cus=%llu max_blocks=%u", (ull)ngroups, (ull)gsg, C, kpg, (ull)cus, max_blocks
    const FoldLimits lim = clamp_fold_limits(max_blocks, 0);
    const GroupedPlan p = plan_fold_grouped(ngroups, gsg, C, kpg, cus, lim);
    ++g_plans;
    const uint64_t cap = max_blocks ? max_blocks : kGroupMaxBlocks;
    CHECK(p.cap == cap && p.cap <= kGridX, AT);
    CHECK(p.runs >= 1 && p.runs <= gsg && p.spr >= 1, AT);
    CHECK((p.runs - 1) * p.spr < gsg && p.runs * p.spr >= gsg, AT);   // no empty run, the runs reach gsg
    CHECK(p.route == kScatterRouteGrouped, AT);                       // a fold has no other route
    CHECK(p.scratch_bytes() == 0, AT);                                // what the size function promises: none
    // Few large groups split into runs of whole pairs; groups enough to fill the chip do not.
    if (2 * ngroups * C <= cus * kGroupPerCu && gsg >= 3) CHECK(p.runs > 1, AT);
    if (ngroups * C >= cus * kGroupPerCu) CHECK(p.runs == 1, AT);
    CHECK(p.runs == 1 || p.spr % 2 == 0, AT);
    const uint64_t triples = ngroups * gsg * C, lanes = ngroups * C;
    const bool exhaustive = triples <= (1u << 21);
    g_exhaustive += exhaustive;
    std::vector<uint16_t> keys(exhaustive ? triples : 0);   // per triple: the keys folded so far, one bit each
    std::vector<uint64_t> next(lanes);                      // per (group, column): where its next run must start
    uint32_t k_at = 0;                                      // keys [0, k_at) are done
    uint64_t u_at = p.units();                              // units [0, u_at) of the current pass are done
    uint32_t pass_k0 = 0, pass_kp = 0;
    p.for_each_launch([&](const GroupLaunch& l) {
        ++g_launches;
        if (u_at == p.units()) {                            // a new key pass
            for (uint64_t i = 0; i < lanes; ++i) CHECK(k_at == 0 || next[i] == gsg, AT);
            CHECK(l.k0 == k_at && l.kp >= 1 && l.kp <= kGroupKeysPerPass && l.k0 + l.kp <= kpg, AT);
            pass_k0 = l.k0, pass_kp = l.kp, k_at = l.k0 + l.kp, u_at = 0;
            next.assign(lanes, 0);
        }
        CHECK(l.k0 == pass_k0 && l.kp == pass_kp, AT);
        CHECK(l.u0 == u_at && l.blocks >= 1 && l.blocks <= cap && l.blocks <= kGridX, AT);
        CHECK(l.u0 + l.blocks <= p.units(), AT);
        u_at = l.u0 + l.blocks;
        for (uint64_t u = l.u0; u < l.u0 + l.blocks && g_fail == 0; ++u) {
            const GroupUnit x = p.unit(u), d = group_unit(u, p.runs, p.spr, p.gsg, p.C);
            CHECK(x.g == d.g && x.s0 == d.s0 && x.s1 == d.s1 && x.c == d.c, AT);   // the kernels' decode
            CHECK(x.g < ngroups && x.c < C, AT);
            CHECK(x.s0 < x.s1 && x.s1 <= gsg, AT);          // not empty, inside its group
            if (!(x.g < ngroups && x.c < C && x.s0 < x.s1 && x.s1 <= gsg)) return 0;
            uint64_t& nx = next[x.g * C + x.c];
            CHECK(nx == x.s0, AT);
            nx = x.s1;
            if (exhaustive)
                for (uint64_t S = x.s0; S < x.s1; ++S) {
                    uint16_t& m = keys[(x.g * gsg + S) * C + x.c];
                    const uint16_t add = (uint16_t)(((1u << l.kp) - 1) << l.k0);
                    CHECK((m & add) == 0, AT);              // no cell twice
                    m |= add;
                }
        }
        return 0;
    });
    CHECK(k_at == kpg && u_at == p.units(), AT);
    for (uint64_t i = 0; i < lanes; ++i) CHECK(next[i] == gsg, AT);
    for (uint16_t m : keys) CHECK(m == (uint16_t)((1u << kpg) - 1), AT);   // every cell, every key
#undef AT
}

static void check_layout() {
    const uint64_t want_stride[][2] = {{1, 256}, {255, 256}, {256, 256}, {257, 512}};
    for (const auto& w : want_stride) {
        const uint64_t nrec = w[0], gs = w[1];
        CHECK(group_stride(nrec) == gs, "nrec=%llu", (ull)nrec);
        for (uint64_t g : {0ull, 1ull, 2ull, 1000ull})
            for (uint64_t i : {(uint64_t)0, nrec / 2, nrec - 1}) {
                CHECK(group_flat(g * nrec + i, nrec) == g * gs + i, "nrec=%llu g=%llu i=%llu", (ull)nrec, (ull)g, (ull)i);
            }
        // Consecutive indices across a group edge: the padding is skipped.
        CHECK(group_flat(nrec, nrec) - group_flat(nrec - 1, nrec) == gs - nrec + 1, "nrec=%llu", (ull)nrec);
    }
    CHECK(group_stride(0) == 0, "0");
    uint64_t b = 1;
    CHECK(grouped_bytes(3, 257, 20, &b) && b == 3 * 512 * 20, "bytes");
    CHECK(grouped_bytes(0, 5, 4, &b) && b == 0, "no groups");
    CHECK(!grouped_bytes(1ull << 40, 1ull << 30, 4, &b), "overflow");
    CHECK(!grouped_bytes(1, UINT64_MAX, 4, &b), "overflow of the stride");
}

// 7 groups of 300 records (stride 512) on 3 shards: 3, 3 and 1 groups.
static void check_update_split() {
    const uint64_t ngroups = 7, nrec = 300, gs = 512;
    const size_t nshards = 3;
    const ShardRanges r = grouped_shards(ngroups, nrec, nshards);
    CHECK(groups_per_shard(ngroups, nshards) == 3 && r.slice == 3 * gs && r.nrec == 7 * gs, "ranges");
    CHECK(r.lo(0) == 0 && r.hi(0) == 3 * gs && r.lo(2) == 6 * gs && r.hi(2) == 7 * gs, "ranges");
    // Both sides of both shard edges, a group edge inside a shard, one index twice, unsorted.
    const uint64_t idx[] = {3 * nrec, 3 * nrec - 1, 6 * nrec, 6 * nrec - 1, 300, 299, 0, 3 * nrec, 7 * nrec - 1};
    const size_t n = sizeof(idx) / sizeof(idx[0]);
    for (bool keep_last : {true, false}) {
        PirUpdatePlan p;
        CHECK(plan_pir_update_grouped(idx, n, ngroups, nrec, nshards, keep_last, &p), "plan");
        CHECK(p.shard_off.size() == nshards + 1 && p.shard_off[nshards] == (keep_last ? n - 1 : n), "offsets");
        for (size_t s = 0; s < nshards; ++s)
            for (size_t k = p.shard_off[s]; k < p.shard_off[s + 1]; ++k) {
                const uint64_t v = idx[p.src[k]], g = v / nrec, i = v % nrec;
                CHECK(g / 3 == s, "idx %llu in shard %zu", (ull)v, s);
                CHECK(p.local[k] == (g - 3 * s) * gs + i, "idx %llu local %llu", (ull)v, (ull)p.local[k]);
                CHECK(r.lo(s) + p.local[k] == group_flat(v, nrec), "idx %llu", (ull)v);
                if (k > p.shard_off[s]) CHECK(p.local[k - 1] <= p.local[k], "order");
                if (keep_last && v == 3 * nrec) CHECK(p.src[k] == 7, "the last of a repeated index stays");
            }
    }
    PirUpdatePlan q;
    q.local.push_back(77);
    const uint64_t bad[] = {0, ngroups * nrec};
    CHECK(!plan_pir_update_grouped(bad, 2, ngroups, nrec, nshards, true, &q) && q.local.size() == 1, "index past the DB");
}

int main() {
    check_layout();
    check_update_split();
    for (uint64_t ngroups : {1ull, 2ull, 3ull, 65ull, 1000ull, 100000ull})
        for (uint64_t gsg : {1ull, 2ull, 3ull, 16ull, 2049ull})
            for (uint32_t C : {1u, 2u, 5u})
                for (uint32_t kpg : {1u, 2u, 3u, 4u, 5u, 9u})
                    for (uint64_t cus : {1ull, 32ull, 256ull})
                        for (uint32_t mb : {0u, 1u, 2u, 7u}) check_plan(ngroups, gsg, C, kpg, cus, mb);
    // The default limits are the plan's own cap; an explicit limit at or above the folds' default is the same.
    CHECK(plan_fold_grouped(5, 3, 1, 1, 256, clamp_fold_limits(1024, 0)).cap == kGroupMaxBlocks, "cap");
    CHECK(plan_fold_grouped(5, 3, 1, 1, 256, clamp_fold_limits(1023, 0)).cap == 1023, "cap");
    // One more key pass shape: the knob narrows the passes.
    CHECK(plan_fold_grouped(5, 3, 1, 9, 256, clamp_fold_limits(0, 0), 2).kp_max == 2, "knob");
    printf("plans=%llu launches=%llu exhaustive=%llu\n", (ull)g_plans, (ull)g_launches, (ull)g_exhaustive);
    if (g_fail) {
        printf("pir_group_plan FAILED (%d)\n", g_fail);
        return 1;
    }
    printf("pir_group_plan ok\n");
    return 0;
}
