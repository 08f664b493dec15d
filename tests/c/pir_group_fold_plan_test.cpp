// pir_group_fold_plan_test.cpp — the grouped fold's route and the launch plan
// of its matrix-core route (dpf-go_amd/csrc/pir_group_fold_plan.hpp) as a
// stand-alone program.  Over ngroups x gsg x C x kpg x CU counts x limits, with
// the route forced to the matrix cores, every plan folds each (group,
// super-group, column, key) cell exactly once; has no empty run, none across a
// group boundary and none longer than min(kFoldMaxSg, max_sg); cuts runs at
// whole staged blocks of its tile shape (or, where max_sg is below one, at
// max_sg); keeps every key tile inside one group and inside its shape's 32 MT
// key rows, the tiles' widths (at most 256) summing to kpg and the last tile
// taking the smallest shape that holds it; keeps every launch inside the
// workgroup cap and the grid's x dimension; and clears the answers exactly when
// some tile has several runs.  Cells are counted one by one where a shape has
// at most 2^21 (group, super-group, column) triples; every shape is also walked
// run by run.  The direct route must return plan_fold_grouped's plan field for
// field, kpg <= 4 must be direct without the knob, and the route rule must give
// the recorded routes of the measured shapes.  Built with
// -fsanitize=address,undefined and run directly by
// tests/test_group_fold_plan_cpu.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pir_group_fold_plan.hpp"

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

static bool same_plan(const GroupedPlan& a, const GroupedPlan& b) {
    return a.ngroups == b.ngroups && a.gsg == b.gsg && a.C == b.C && a.kpg == b.kpg && a.runs == b.runs && a.spr == b.spr &&
           a.cap == b.cap && a.kp_max == b.kp_max && a.halve == b.halve && a.route == b.route;
}

static void check_plan(uint64_t ngroups, uint64_t gsg, uint32_t C, uint32_t kpg, uint64_t cus, uint32_t max_blocks,
                       uint32_t max_sg) {
#define AT "ngroups=%llu gsg=%llu C=%u kpg=%u cus=%llu max_blocks=%u max_sg=%u", (ull)ngroups, (ull)gsg, C, kpg, (ull)cus, max_blocks, max_sg
    const FoldLimits lim = clamp_fold_limits(max_blocks, max_sg);
    ++g_plans;
    // The rule, and the direct route: plan_fold_grouped's plan, whatever the route.
    const GroupedPlan want = plan_fold_grouped(ngroups, gsg, C, kpg, cus, lim);
    const GroupFoldKeysPlan ruled = plan_fold_grouped_keys(ngroups, gsg, C, kpg, cus, lim);
    CHECK(ruled.route == fold_route(ngroups, gsg, C, kpg), AT);
    if (kpg <= 4) CHECK(ruled.route == kFoldRouteDirect, AT);
    const GroupFoldKeysPlan direct = plan_fold_grouped_keys(ngroups, gsg, C, kpg, cus, lim, (int)kFoldRouteDirect);
    CHECK(direct.route == kFoldRouteDirect && same_plan(direct.direct, want) && same_plan(ruled.direct, want), AT);
    CHECK(direct.atomic() == want.atomic(), AT);
    for (uint32_t kpm : {1u, 2u})
        CHECK(same_plan(plan_fold_grouped_keys(ngroups, gsg, C, kpg, cus, lim, (int)kFoldRouteDirect, kpm).direct,
                        plan_fold_grouped(ngroups, gsg, C, kpg, cus, lim, kpm)), AT);
    // The matrix-core route.
    const GroupFoldKeysPlan p = plan_fold_grouped_keys(ngroups, gsg, C, kpg, cus, lim, (int)kFoldRouteMfma);
    CHECK(p.route == kFoldRouteMfma && p.scratch_bytes() == 0, AT);
    if (ruled.route == kFoldRouteMfma)
        CHECK(ruled.tiles() == p.tiles() && ruled.full.runs == p.full.runs && ruled.last.runs == p.last.runs, AT);
    const uint64_t cap = max_blocks ? max_blocks : kGroupMaxBlocks;
    CHECK(p.cap == cap && p.cap <= kGridX, AT);
    CHECK(p.tiles() == (kpg + kFoldKeyGroup - 1) / kFoldKeyGroup, AT);
    if (ngroups == 0 || gsg == 0 || kpg == 0) {               // nothing to do: no unit, no launch, no clear
        uint64_t n = 0;
        p.for_each_launch([&](const GroupFoldLaunch&) { return ++n, 0; });
        CHECK(n == 0 && !p.atomic(), AT);
        return;
    }
    const uint64_t msg = max_sg != 0 && max_sg < kFoldMaxSg ? max_sg : kFoldMaxSg;
    const uint64_t triples = ngroups * gsg * C;
    const bool exhaustive = triples <= (1u << 21);
    g_exhaustive += exhaustive;
    std::vector<uint8_t> seen(exhaustive ? triples : 0);    // per (group, super-group, column): folded in this tile
    std::vector<uint64_t> next;                             // per (group, column group): where its next run must start
    uint32_t k_at = 0, tile_at = 0, width_sum = 0;
    uint64_t u_at = 0, units = 0;
    bool any_runs = false, open = false;
    GroupFoldPass cur;
    auto close_tile = [&]() {
        if (!open) return;
        CHECK(u_at == units, AT);
        for (uint64_t v : next) CHECK(v == gsg, AT);
        for (uint8_t v : seen) CHECK(v == 1, AT);           // every cell of the tile's keys, once
        open = false;
    };
    p.for_each_launch([&](const GroupFoldLaunch& l) {
        ++g_launches;
        const GroupFoldPass& t = l.pass;
        if (!open || t.k0 != cur.k0) {                      // a new key tile
            close_tile();
            cur = t, open = true;
            const FoldTile& sh = kFoldTiles[t.shape];
            CHECK(t.k0 == k_at && t.kp >= 1 && t.kp <= kFoldKeyGroup && t.k0 + t.kp <= kpg, AT);   // inside one group's keys
            CHECK(t.kp == kFoldKeyGroup || t.k0 + t.kp == kpg, AT);
            CHECK(t.shape >= 0 && t.shape < kFoldTileCount && t.kp <= 32u * (uint32_t)sh.MT, AT);
            CHECK(t.shape == fold_tile_index(t.kp, fold_cg(C, 4)), AT);                           // the smallest that holds it
            CHECK(t.cg == (uint32_t)sh.CG && t.cg * t.ncg == C && t.ncg >= 1, AT);
            CHECK(t.runs >= 1 && t.spr >= 1 && t.spr <= msg, AT);
            CHECK((t.runs - 1) * t.spr < gsg && t.runs * t.spr >= gsg, AT);                       // no empty run, the runs reach gsg
            CHECK(t.spr % (uint64_t)sh.SG == 0 || (t.spr == msg && msg < (uint64_t)sh.SG), AT);
            // Groups enough to fill the chip are one run each unless the limit cuts them; few large ones are cut.
            if (ngroups * t.ncg >= 2 * cus * fold_tile_per_cu(sh) && gsg <= kFoldMaxSg && !max_sg) CHECK(t.runs == 1, AT);
            if (2 * ngroups * t.ncg <= cus * fold_tile_per_cu(sh) && gsg >= 2 * (uint64_t)sh.SG) CHECK(t.runs > 1, AT);
            any_runs |= t.runs > 1;
            units = p.units(t);
            CHECK(units == ngroups * t.ncg * t.runs, AT);
            k_at = t.k0 + t.kp, width_sum += t.kp, u_at = 0, ++tile_at;
            next.assign(ngroups * t.ncg, 0);
            seen.assign(seen.size(), 0);
        }
        CHECK(t.kp == cur.kp && t.shape == cur.shape && t.runs == cur.runs && t.spr == cur.spr && t.ncg == cur.ncg, AT);
        CHECK(l.u0 == u_at && l.blocks >= 1 && l.blocks <= cap && l.blocks <= kGridX && l.u0 + l.blocks <= units, AT);
        u_at = l.u0 + l.blocks;
        for (uint64_t u = l.u0; u < l.u0 + l.blocks && g_fail == 0; ++u) {
            const GroupUnit x = p.unit(t, u);
            CHECK(x.g < ngroups && x.c < t.ncg, AT);
            CHECK(x.s0 < x.s1 && x.s1 <= gsg && x.s1 - x.s0 <= msg, AT);   // not empty, inside its group, fp32-exact
            if (!(x.g < ngroups && x.c < t.ncg && x.s0 < x.s1 && x.s1 <= gsg)) return 0;
            uint64_t& nx = next[x.g * t.ncg + x.c];
            CHECK(nx == x.s0, AT);
            nx = x.s1;
            if (exhaustive)
                for (uint64_t S = x.s0; S < x.s1; ++S)
                    for (uint32_t cw = 0; cw < t.cg; ++cw) ++seen[(x.g * gsg + S) * C + x.c * t.cg + cw];
        }
        return 0;
    });
    close_tile();
    CHECK(k_at == kpg && width_sum == kpg && tile_at == p.tiles(), AT);
    CHECK(p.atomic() == any_runs, AT);                      // one run: no clear; several: a clear
#undef AT
}

// The recorded routes: (ngroups, gsg, C, kpg) -> route.  The measured shapes
// (DESIGN.md §4.4 "Many keys per group") and the rule beside them.
static void check_routes() {
    struct R {
        uint64_t ngroups, gsg;
        uint32_t C, kpg;
        GroupFoldRoute want;
    };
    const GroupFoldRoute D = kFoldRouteDirect, M = kFoldRouteMfma;
    const R rows[] = {
        // 2^24 x 32 B kept 3-fold as 96 x 2^19 and as 384 x 2^17, kpg 4, 5, 8, 12, 16, 32, 64, 256.
        {96, 2048, 1, 4, D},   {96, 2048, 1, 5, M},   {96, 2048, 1, 8, M},   {96, 2048, 1, 12, M},
        {96, 2048, 1, 16, M},  {96, 2048, 1, 32, M},  {96, 2048, 1, 64, M},  {96, 2048, 1, 256, M},
        {384, 512, 1, 4, D},   {384, 512, 1, 5, M},   {384, 512, 1, 8, M},   {384, 512, 1, 12, M},
        {384, 512, 1, 16, M},  {384, 512, 1, 32, M},  {384, 512, 1, 64, M},  {384, 512, 1, 256, M},
        // The wide shape (256-byte records, the same bytes) and the small-group one (4096 groups of 2^12).
        {96, 256, 8, 4, D},    {96, 256, 8, 8, M},    {96, 256, 8, 16, M},   {96, 256, 8, 64, M},
        {4096, 16, 1, 4, D},   {4096, 16, 1, 8, M},   {4096, 16, 1, 16, M},  {4096, 16, 1, 64, M},
        // Up to 4 keys: one direct pass at the speed of the stream, at any shape.
        {1, 1, 1, 1, D},       {1, 40000, 1, 4, D},   {100000, 1, 5, 3, D},  {7, 2, 2, 2, D},
        {1, 1, 1, 5, M},       {100000, 1, 5, 600, M},
    };
    for (const R& r : rows)
        CHECK(fold_route(r.ngroups, r.gsg, r.C, r.kpg) == r.want, "route of ngroups=%llu gsg=%llu C=%u kpg=%u",
              (ull)r.ngroups, (ull)r.gsg, r.C, r.kpg);
    CHECK(fold_route(0, 5, 1, 0) == kFoldRouteDirect, "empty");
    (void)fold_route(UINT64_MAX, UINT64_MAX, UINT32_MAX, UINT32_MAX);
}

int main() {
    check_routes();
    const uint32_t keys[] = {1, 2, 4, 5, 9, 32, 33, 64, 65, 128, 129, 256, 257, 260, 512, 600};
    for (uint64_t ngroups : {1ull, 2ull, 3ull, 65ull, 1000ull})
        for (uint64_t gsg : {1ull, 2ull, 3ull, 4ull, 5ull, 16ull, 20ull, 2049ull})
            for (uint32_t C : {1u, 2u, 4u, 5u, 8u})
                for (uint32_t kpg : keys) {
                    if (ngroups * gsg * C > (1u << 20) && kpg > 260) continue;
                    for (uint64_t cus : {1ull, 32ull, 256ull})
                        for (uint32_t mb : {0u, 2u, 7u}) {
                            if (mb != 0 && ngroups * gsg * C > (1u << 16)) continue;   // launches by the hundred thousand
                            check_plan(ngroups, gsg, C, kpg, cus, mb, 0);
                        }
                }
    // 10^5 tiny groups, and groups above 2^15 super-groups (the fp32 bound cuts them).
    for (uint32_t kpg : {1u, 9u, 64u, 600u}) {
        check_plan(100000, 1, 1, kpg, 256, 0, 0);
        check_plan(100000, 2, 4, kpg, 256, 0, 0);
        check_plan(1, 40000, 1, kpg, 256, 0, 0);
        check_plan(1000, 40000, 2, kpg, 256, 0, 0);
        check_plan(3, 65537, 1, kpg, 1, 0, 0);
    }
    // max_sg cuts the runs of groups that would otherwise be one run, below a staged block too.
    for (uint64_t ngroups : {1ull, 7ull, 3000ull})
        for (uint64_t gsg : {1ull, 5ull, 16ull, 20ull, 2049ull})
            for (uint32_t msg : {1u, 2u, 3u, 4u, 6u, 100u})
                for (uint32_t kpg : {2u, 9u, 33u, 130u, 260u})
                    for (uint32_t mb : {0u, 8u}) {
                        if (mb != 0 && ngroups * gsg > 20000) continue;
                        check_plan(ngroups, gsg, 2, kpg, 256, mb, msg);
                    }
    // Nothing to do: no launch.
    check_plan(0, 5, 1, 33, 256, 0, 0);
    check_plan(5, 0, 1, 33, 256, 0, 0);
    check_plan(5, 5, 1, 0, 256, 0, 0);
    // What the run rule does at the measured shapes on 256 CUs: whole rounds of resident workgroups.
    {
        const FoldLimits lim = clamp_fold_limits(0, 0);
        GroupFoldKeysPlan p = plan_fold_grouped_keys(96, 2048, 1, 256, 256, lim);
        CHECK(p.full.runs == 8 && p.full.spr == 256 && p.atomic(), "96 groups, 256 keys");
        p = plan_fold_grouped_keys(384, 512, 1, 256, 256, lim);
        CHECK(p.full.runs == 2 && p.full.spr == 256, "384 groups, 256 keys");
        p = plan_fold_grouped_keys(4096, 16, 1, 16, 256, lim);
        CHECK(p.last.runs == 1 && p.last.spr == 16 && !p.atomic() && p.tiles() == 1, "4096 groups");
        CHECK(group_fold_want_runs(96, 256) == 8 && group_fold_want_runs(384, 512) == 4 && group_fold_want_runs(1, 256) == 256 &&
                  group_fold_want_runs(256, 256) == 1 && group_fold_want_runs(1000, 256) == 1 && group_fold_want_runs(0, 256) == 1,
              "want runs");
    }
    printf("plans=%llu launches=%llu exhaustive=%llu\n", (ull)g_plans, (ull)g_launches, (ull)g_exhaustive);
    if (g_fail) {
        printf("pir_group_fold_plan FAILED (%d)\n", g_fail);
        return 1;
    }
    printf("pir_group_fold_plan ok\n");
    return 0;
}
