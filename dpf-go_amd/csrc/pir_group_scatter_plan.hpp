// pir_group_scatter_plan.hpp — the grouped private write (k_scatter_grouped,
// pir_scatter_grouped.hip): its builder of pir_group_plan.hpp's launch plan and
// its route rule.  Host-only and header-only (no HIP), so
// tests/c/pir_scatter_group_plan_test.cpp runs it under ASan/UBSan without a
// device.
//
// Plan.  pir_group_plan.hpp's GroupedPlan, with its guarantees, under the
// scatter's three rules (plan_scatter_grouped below).  A unit's column group is
// ONE 32-byte column, as in the grouped fold: the selection words are
// wave-uniform scalar loads and not staged in LDS, so columns that shared them
// would share no vector memory traffic.  Runs are ceil(gsg / want) super-groups,
// cut to dpf_set_fold_limits' max_sg.  The keys of a group are applied in
// passes of 4 and one last pass of what is left, 1, 2 or 3, so kpg keys cost
// ceil(kpg / 4) passes over the DB: 3 keys are one pass, not a 2 and a 1.
//
// Route.  The same write is also a loop of launch_scatter_sliced over each
// group's contiguous flat range (correct by the layout rule): one launch per
// group and 64 keys, each a pass over that group with the 64-slot key tile of
// k_scatter_sliced.  The grouped kernel pays a pass over the DB per 4 keys but
// only a launch per pass; the loop pays a launch per group, and its pass
// slows with the keys of its tile.  scatter_route() compares the two in units
// of grouped tile passes (one 16 KiB tile read and written: 3.6 ns measured):
//   grouped = passes(kpg) * (L + ngroups * gsg * C)
//   loop    = ngroups * (nt * L + gsg * C * (32 * nt + kpg) / 32),  nt = ceil(kpg / 64)
// L = kGroupScatterLaunchTiles is the cost of issuing one launch; a dense
// scatter's tile pass over kt keys costs (32 + kt) / 32 grouped ones.
// Measured on one MI355X (tools/grouped_write_ab.py, profiles/grouped_write/;
// DESIGN.md §4.4 "Grouped private writes"), 2^24 x 32 B kept 3-fold: the
// grouped kernel takes 0.71 ms a pass over the 1.5 GiB; the loop with one key
// per group 0.98 ms at 96 groups and 1.90 ms at 384, which gives L = 3.2 us =
// 900 tile passes, and 2.35 ms at 96 groups of 64 keys, which gives the
// slope.  What the rule then does at the measured shapes (pinned in
// tests/c/pir_scatter_group_plan_test.cpp): at 96 groups of 2048 super-groups
// the grouped kernel for 1 to 4 keys per group and the loop from 5, where the
// second pass starts (measured: grouped ahead at 1, 2, 3 and 4 keys, behind at
// 5, 7, 8, 16 and 64); at 384 groups of 512 super-groups the grouped kernel up
// to 12 keys and the loop from 13 (only 1 key was measured there).  The rule
// compares a step function of kpg with a line, so near a crossover it can
// take the loop at 4 k + 1 keys and the kernel again at 4 k + 4.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pir_group_plan.hpp"
#include "pir_scatter_plan.hpp"

namespace dpfh {

// The route model's constants (fitted as the header comment says).
constexpr uint64_t kGroupScatterLaunchTiles = 900;
constexpr uint64_t kGroupScatterLoopKeyDen = 32;    // a dense tile pass over kt keys: (32 + kt) / 32 grouped ones

// Key passes of kpg keys: fours, then one pass of the 1, 2 or 3 left.
inline uint64_t group_scatter_passes(uint64_t kpg) { return kpg / 4 + (kpg % 4 != 0); }

// The route for ngroups groups of gsg super-groups and C columns, kpg keys a
// group (above).  Saturating arithmetic: the products of a shape that fits
// memory stay far below 2^64, and one that does not gets the grouped route.
inline GroupScatterRoute scatter_route(uint64_t ngroups, uint64_t gsg, uint32_t C, uint32_t kpg) {
    if (ngroups == 0 || gsg == 0 || C == 0 || kpg == 0) return kScatterRouteGrouped;
    auto mul = [](uint64_t a, uint64_t b) { return b != 0 && a > UINT64_MAX / b ? UINT64_MAX : a * b; };
    auto add = [](uint64_t a, uint64_t b) { return a > UINT64_MAX - b ? UINT64_MAX : a + b; };
    const uint64_t tiles = mul(gsg, C);
    const uint64_t grouped = mul(group_scatter_passes(kpg), add(kGroupScatterLaunchTiles, mul(ngroups, tiles)));
    const uint64_t nt = ((uint64_t)kpg + kScatterKeyTile - 1) / kScatterKeyTile;
    const uint64_t loop_tiles = mul(tiles, kGroupScatterLoopKeyDen * nt + kpg) / kGroupScatterLoopKeyDen;
    const uint64_t loop = mul(ngroups, add(mul(nt, kGroupScatterLaunchTiles), loop_tiles));
    return loop < grouped ? kScatterRouteLoop : kScatterRouteGrouped;
}

// The grouped write of ngroups groups of gsg super-groups and C columns, kpg
// keys per group, on `cus` CUs: the three rules above.
inline GroupedPlan plan_scatter_grouped(uint64_t ngroups, uint64_t gsg, uint32_t C, uint32_t kpg, uint64_t cus,
                                        FoldLimits lim) {
    GroupedPlan p = grouped_plan_shape(ngroups, gsg, C, kpg, lim);
    p.route = scatter_route(ngroups, gsg, C, kpg);
    if (gsg == 0) return p;
    const uint64_t want = grouped_want_runs(ngroups, gsg, C, cus);
    p.spr = (gsg + want - 1) / want;
    if (lim.max_sg != 0 && p.spr > lim.max_sg) p.spr = lim.max_sg;
    p.runs = (gsg + p.spr - 1) / p.spr;
    return p;
}

}  // namespace dpfh
