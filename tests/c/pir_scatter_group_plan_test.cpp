// pir_scatter_group_plan_test.cpp — the launch plan of the grouped private
// write (dpf-go_amd/csrc/pir_group_scatter_plan.hpp) as a stand-alone program.
// Over ngroups x gsg x C x kpg x CU counts x limits every plan applies each
// (group, super-group, column, key) cell exactly once; has no empty run, none
// across a group boundary and none longer than max_sg; keeps every launch
// inside the workgroup cap and the grid's x dimension; has no two writers of
// one tile in a launch (nor in a pass: a pass reads and writes a tile at most
// once); and its pass widths are 4s and one last pass of 1 to 3 that sum to
// kpg, ceil(kpg / 4) passes in all.  Cells
// are counted one by one where a shape has at most 2^21 (group, super-group,
// column) triples; every shape is also walked run by run (each run must start
// where the previous run of its group and column ended, and the last must end
// at gsg), which is the same statement without a byte per cell.  Then the
// route rule on a recorded list of shapes.  Built with
// -fsanitize=address,undefined and run directly by
// tests/test_group_scatter_plan_cpu.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pir_group_scatter_plan.hpp"

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

static void check_plan(uint64_t ngroups, uint64_t gsg, uint32_t C, uint32_t kpg, uint64_t cus, uint32_t max_blocks,
                       uint32_t max_sg) {
#define AT "ngroups=%llu gsg=%llu C=%u kpg=%u cus=%llu max_blocks=%u max_sg=%u", (ull)ngroups, (ull)gsg, C, kpg, (ull)cus, max_blocks, max_sg
    const FoldLimits lim = clamp_fold_limits(max_blocks, max_sg);
    const GroupedPlan p = plan_scatter_grouped(ngroups, gsg, C, kpg, cus, lim);
    ++g_plans;
    const uint64_t cap = max_blocks ? max_blocks : kGroupMaxBlocks;
    CHECK(p.cap == cap && p.cap <= kGridX, AT);
    if (ngroups == 0 || gsg == 0 || kpg == 0) {               // nothing to do: no unit, no launch
        uint64_t n = 0;
        p.for_each_launch([&](const GroupLaunch&) { return ++n, 0; });
        CHECK(p.units() == 0 && p.passes() == 0 && n == 0, AT);
        return;
    }
    CHECK(p.runs >= 1 && p.runs <= gsg && p.spr >= 1, AT);
    CHECK((p.runs - 1) * p.spr < gsg && p.runs * p.spr >= gsg, AT);   // no empty run, the runs reach gsg
    if (max_sg) CHECK(p.spr <= max_sg, AT);
    CHECK(p.units() == ngroups * C * p.runs, AT);
    CHECK(p.route == scatter_route(ngroups, gsg, C, kpg), AT);        // the route is a function of the shape alone
    // Few large groups split into runs; groups enough to fill the chip do not (unless max_sg cuts them).
    if (2 * ngroups * C <= cus * kGroupPerCu && gsg >= 2) CHECK(p.runs > 1, AT);
    if (ngroups * C >= cus * kGroupPerCu && !max_sg) CHECK(p.runs == 1, AT);
    const uint64_t triples = ngroups * gsg * C, lanes = ngroups * C;
    const bool exhaustive = triples <= (1u << 21);
    g_exhaustive += exhaustive;
    std::vector<uint16_t> keys(exhaustive ? triples : 0);   // per triple: the keys applied so far, one bit each
    std::vector<uint64_t> next(lanes);                      // per (group, column): where its next run must start
    uint32_t k_at = 0;                                      // keys [0, k_at) are done
    uint64_t u_at = p.units();                              // units [0, u_at) of the current pass are done
    uint32_t pass_k0 = 0, pass_kp = 0, last_kp = kGroupKeysPerPass, width_sum = 0;
    uint64_t passes = 0;
    p.for_each_launch([&](const GroupLaunch& l) {
        ++g_launches;
        if (u_at == p.units()) {                            // a new key pass
            for (uint64_t i = 0; i < lanes; ++i) CHECK(k_at == 0 || next[i] == gsg, AT);
            CHECK(l.k0 == k_at && l.kp >= 1 && l.kp <= kGroupKeysPerPass && l.k0 + l.kp <= kpg, AT);
            CHECK(last_kp == kGroupKeysPerPass, AT);   // 4s, then one last pass of the 1 to 3 keys left
            CHECK(l.kp == kGroupKeysPerPass || l.k0 + l.kp == kpg, AT);
            pass_k0 = l.k0, pass_kp = l.kp, last_kp = l.kp, k_at = l.k0 + l.kp, u_at = 0;
            width_sum += l.kp;
            ++passes;
            next.assign(lanes, 0);
        }
        CHECK(l.k0 == pass_k0 && l.kp == pass_kp, AT);
        CHECK(l.u0 == u_at && l.blocks >= 1 && l.blocks <= cap && l.blocks <= kGridX, AT);
        CHECK(l.u0 + l.blocks <= p.units(), AT);
        u_at = l.u0 + l.blocks;
        for (uint64_t u = l.u0; u < l.u0 + l.blocks && g_fail == 0; ++u) {
            const GroupUnit x = p.unit(u);
            CHECK(x.g < ngroups && x.c < C, AT);
            CHECK(x.s0 < x.s1 && x.s1 <= gsg, AT);          // not empty, inside its group
            if (max_sg) CHECK(x.s1 - x.s0 <= max_sg, AT);
            if (!(x.g < ngroups && x.c < C && x.s0 < x.s1 && x.s1 <= gsg)) return 0;
            // One writer per tile and pass: the run starts where its lane's last one ended,
            // so no tile is met twice in this pass, let alone in this launch.
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
    CHECK(k_at == kpg && u_at == p.units() && width_sum == kpg, AT);
    CHECK(passes == p.passes() && passes == group_scatter_passes(kpg), AT);
    for (uint64_t i = 0; i < lanes; ++i) CHECK(next[i] == gsg, AT);
    for (uint16_t m : keys) CHECK(m == (uint16_t)((1u << kpg) - 1), AT);   // every cell, every key
#undef AT
}

// The route of a recorded list of shapes: (ngroups, gsg, C, kpg) -> route.
// The grouped kernel where the groups are many or the keys few; the loop of
// dense scatters for few large groups with many keys each.
static void check_routes() {
    struct R {
        uint64_t ngroups, gsg;
        uint32_t C, kpg;
        GroupScatterRoute want;
    };
    const R rows[] = {
        // The measured table's shapes (2^24 x 32 B kept 3-fold in 96 and 384 groups): at 96 groups the
        // grouped kernel won at 1, 2, 3 and 4 keys and lost at 5, 7, 8, 16 and 64; the rule's crossover is its second pass.
        {96, 2048, 1, 1, kScatterRouteGrouped},   {96, 2048, 1, 2, kScatterRouteGrouped},
        {96, 2048, 1, 3, kScatterRouteGrouped},   {96, 2048, 1, 6, kScatterRouteLoop},
        {96, 2048, 1, 4, kScatterRouteGrouped},   {96, 2048, 1, 8, kScatterRouteLoop},
        {96, 2048, 1, 5, kScatterRouteLoop},      {96, 2048, 1, 7, kScatterRouteLoop},
        {96, 2048, 1, 16, kScatterRouteLoop},     {96, 2048, 1, 64, kScatterRouteLoop},
        {384, 512, 1, 1, kScatterRouteGrouped},   {384, 512, 1, 4, kScatterRouteGrouped},
        // (only 1 key was measured at 384 groups: the rest is the rule, the kernel up to 12 keys and the loop from 13)
        {384, 512, 1, 3, kScatterRouteGrouped},   {384, 512, 1, 5, kScatterRouteGrouped},
        {384, 512, 1, 7, kScatterRouteGrouped},   {384, 512, 1, 8, kScatterRouteGrouped},
        {384, 512, 1, 9, kScatterRouteGrouped},   {384, 512, 1, 11, kScatterRouteGrouped},
        {384, 512, 1, 12, kScatterRouteGrouped},  {384, 512, 1, 13, kScatterRouteLoop},
        {384, 512, 1, 16, kScatterRouteLoop},     {384, 512, 1, 17, kScatterRouteLoop},
        {384, 512, 1, 64, kScatterRouteLoop},
        // 12 and 24 groups of the same size: as at 96.
        {24, 2048, 1, 3, kScatterRouteGrouped},   {24, 2048, 1, 4, kScatterRouteGrouped},
        {24, 2048, 1, 5, kScatterRouteLoop},      {12, 2048, 1, 3, kScatterRouteGrouped},
        {12, 2048, 1, 4, kScatterRouteGrouped},   {12, 2048, 1, 5, kScatterRouteLoop},
        // Tiny groups: a launch per group never pays.
        {100000, 1, 1, 1, kScatterRouteGrouped},  {100000, 1, 1, 64, kScatterRouteGrouped},
        {300, 1, 1, 5, kScatterRouteGrouped},     {7, 2, 2, 7, kScatterRouteGrouped},
        {7, 2, 5, 9, kScatterRouteGrouped},
        // One or two groups: from the second key pass (5 keys) the dense scatter's single launch wins.
        {1, 3, 1, 3, kScatterRouteGrouped},       {1, 3, 1, 5, kScatterRouteLoop},
        {1, 3, 1, 1, kScatterRouteGrouped},       {1, 3, 1, 2, kScatterRouteGrouped},
        {1, 3, 1, 9, kScatterRouteLoop},          {1, 3, 1, 70, kScatterRouteLoop},
        {2, 3, 5, 70, kScatterRouteLoop},         {2, 3, 1, 4, kScatterRouteGrouped},
    };
    for (const R& r : rows)
        CHECK(scatter_route(r.ngroups, r.gsg, r.C, r.kpg) == r.want, "route of ngroups=%llu gsg=%llu C=%u kpg=%u",
              (ull)r.ngroups, (ull)r.gsg, r.C, r.kpg);
    // Nothing to do is the grouped route (no launch either way), and huge shapes do not overflow.
    CHECK(scatter_route(0, 5, 1, 3) == kScatterRouteGrouped && scatter_route(5, 0, 1, 3) == kScatterRouteGrouped, "empty");
    (void)scatter_route(UINT64_MAX, UINT64_MAX, UINT32_MAX, UINT32_MAX);
    CHECK(group_scatter_passes(0) == 0 && group_scatter_passes(1) == 1 && group_scatter_passes(3) == 1 &&
              group_scatter_passes(4) == 1 && group_scatter_passes(5) == 2 && group_scatter_passes(7) == 2 &&
              group_scatter_passes(9) == 3 && group_scatter_passes(70) == 18,
          "passes");
}

int main() {
    check_routes();
    for (uint64_t ngroups : {1ull, 2ull, 3ull, 65ull, 1000ull, 100000ull})
        for (uint64_t gsg : {1ull, 2ull, 3ull, 16ull, 2049ull})
            for (uint32_t C : {1u, 2u, 5u})
                for (uint32_t kpg : {1u, 2u, 3u, 4u, 5u, 7u, 9u})
                    for (uint64_t cus : {1ull, 32ull, 256ull})
                        for (uint32_t mb : {0u, 1u, 2u, 7u}) check_plan(ngroups, gsg, C, kpg, cus, mb, 0);
    // max_sg cuts the runs of groups that would otherwise be one run.
    for (uint64_t ngroups : {1ull, 7ull, 3000ull})
        for (uint64_t gsg : {1ull, 5ull, 16ull, 2049ull})
            for (uint32_t msg : {1u, 2u, 3u})
                for (uint32_t mb : {0u, 8u}) check_plan(ngroups, gsg, 2, 7, 256, mb, msg);
    // Nothing to do: no launch.
    check_plan(0, 5, 1, 3, 256, 0, 0);
    check_plan(5, 0, 1, 3, 256, 0, 0);
    check_plan(5, 5, 1, 0, 256, 0, 0);
    // The default limits are the plan's own cap; an explicit limit at or above the folds' default is the same.
    CHECK(plan_scatter_grouped(5, 3, 1, 1, 256, clamp_fold_limits(1024, 0)).cap == kGroupMaxBlocks, "cap");
    CHECK(plan_scatter_grouped(5, 3, 1, 1, 256, clamp_fold_limits(1023, 0)).cap == 1023, "cap");
    // 10^5 tiny groups are one grid per pass.
    {
        const GroupedPlan p = plan_scatter_grouped(100000, 1, 1, 1, 256, clamp_fold_limits(0, 0));
        uint64_t n = 0;
        p.for_each_launch([&](const GroupLaunch& l) { return ++n, (void)l, 0; });
        CHECK(n == 1 && p.units() == 100000, "one grid");
    }
    printf("plans=%llu launches=%llu exhaustive=%llu\n", (ull)g_plans, (ull)g_launches, (ull)g_exhaustive);
    if (g_fail) {
        printf("pir_scatter_group_plan FAILED (%d)\n", g_fail);
        return 1;
    }
    printf("pir_scatter_group_plan ok\n");
    return 0;
}
