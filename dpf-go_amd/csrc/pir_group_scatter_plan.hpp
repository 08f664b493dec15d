// pir_group_scatter_plan.hpp — the launch plan of the grouped private write
// (k_scatter_grouped, pir_scatter_grouped.hip), the dual of the grouped fold
// planned in pir_group_plan.hpp.  Host-only and header-only (no HIP), so
// tests/c/pir_scatter_group_plan_test.cpp runs it under ASan/UBSan without a
// device.  The layout rule (group_stride, group_flat) is pir_group_plan.hpp's.
//
// Plan.  A workgroup ("unit") rewrites one run of whole super-groups of one
// column group of one group for kp <= kGroupScatterKeysPerPass keys of that
// group.  A column group is ONE 32-byte column, as in the grouped fold: the
// selection words are wave-uniform scalar loads and not staged in LDS, so
// columns that shared them would share no vector memory traffic.  Units are
// numbered run-fastest, then column, then group (GroupedScatterPlan::unit), and
// a launch is a 1-D grid over a contiguous range of unit numbers: 10^5 tiny
// groups stay in one grid, and few large groups are cut into runs inside
// [0, gsg) of their group.  The keys of a group are applied in passes of 4 and
// one last pass of what is left, 1, 2 or 3 (one kernel instantiation per
// width), in stream order; every pass walks all units.  So kpg keys cost
// ceil(kpg / 4) passes over the DB: 3 keys are one pass, not a 2 and a 1.
// What the plan guarantees, and no kernel can check:
//   - every (group, super-group, column, key) cell is applied exactly once;
//   - no run is empty, none crosses a group boundary, none is longer than
//     dpf_set_fold_limits' max_sg;
//   - the units of a pass are distinct (group, column, run) triples, so within
//     one launch (and within one pass) no two workgroups touch the same tile,
//     and a pass reads and writes a tile at most once: no atomics, no scratch;
//   - a launch has at most lim.max_blocks workgroups when dpf_set_fold_limits
//     set fewer than its default, else at most kGroupMaxBlocks;
//   - the pass widths sum to kpg.
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

constexpr uint32_t kGroupScatterKeysPerPass = 4;    // widest k_scatter_grouped<KP>
constexpr uint64_t kGroupScatterPerCu = 8;          // workgroups per CU a pass aims at (the grouped fold's)
// The route model's constants (fitted as the header comment says).
constexpr uint64_t kGroupScatterLaunchTiles = 900;
constexpr uint64_t kGroupScatterLoopKeyDen = 32;    // a dense tile pass over kt keys: (32 + kt) / 32 grouped ones

enum GroupScatterRoute : uint32_t { kScatterRouteGrouped = 0, kScatterRouteLoop = 1 };

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

// One launch: units [u0, u0 + blocks) for keys [k0, k0 + kp) of every group.
struct GroupScatterLaunch {
    uint64_t u0, blocks;
    uint32_t k0, kp;
};

struct GroupedScatterPlan {
    uint64_t ngroups = 0, gsg = 0;
    uint32_t C = 0, kpg = 0;
    uint64_t runs = 1, spr = 1;   // runs per (group, column), super-groups per run (the last run what is left)
    uint64_t cap = 1;             // workgroups per launch
    uint32_t kp_max = kGroupScatterKeysPerPass;
    GroupScatterRoute route = kScatterRouteGrouped;

    uint64_t units() const { return kpg == 0 ? 0 : ngroups * C * (gsg ? runs : 0); }
    uint64_t passes() const { return units() ? group_scatter_passes(kpg) : 0; }
    // What unit u rewrites: super-groups [s0, s1) (group-local) of column c of group g.
    GroupUnit unit(uint64_t u) const {
        const uint64_t r = u % runs, t = u / runs, s0 = r * spr;
        return {t / C, s0, s0 + spr < gsg ? s0 + spr : gsg, (uint32_t)(t % C)};
    }

    // fn(const GroupScatterLaunch&) for every launch of the grouped route in
    // stream order, until one returns a nonzero (error) value, which is returned.
    template <class F>
    auto for_each_launch(F fn) const -> decltype(fn(GroupScatterLaunch{})) {
        const uint64_t n = units();
        if (n == 0) return {};
        for (uint32_t k0 = 0; k0 < kpg;) {
            const uint32_t kp = kpg - k0 < kp_max ? kpg - k0 : kp_max;
            for (uint64_t u0 = 0; u0 < n; u0 += cap)
                if (auto e = fn(GroupScatterLaunch{u0, n - u0 < cap ? n - u0 : cap, k0, kp}); e != decltype(e){}) return e;
            k0 += kp;
        }
        return {};
    }
};

// ngroups groups of gsg super-groups and C columns, kpg keys per group, on
// `cus` CUs, under dpf_set_fold_limits' values as fold_limits() snapshots them
// (clamp_fold_limits).  Few large groups split into runs until a pass has about
// cus * kGroupScatterPerCu workgroups; from ngroups * C workgroups upwards a
// group is one run, unless lim.max_sg asks for shorter runs.
inline GroupedScatterPlan plan_scatter_grouped(uint64_t ngroups, uint64_t gsg, uint32_t C, uint32_t kpg, uint64_t cus,
                                               FoldLimits lim) {
    GroupedScatterPlan p;
    p.ngroups = ngroups, p.gsg = gsg, p.C = C, p.kpg = kpg;
    p.cap = lim.max_blocks != 0 && lim.max_blocks < kFoldMaxBlocks ? lim.max_blocks : kGroupMaxBlocks;
    p.route = scatter_route(ngroups, gsg, C, kpg);
    if (gsg == 0) return p;
    const uint64_t cells = ngroups * C, aim = (cus ? cus : 1) * kGroupScatterPerCu;
    uint64_t want = cells ? (aim + cells - 1) / cells : 1;
    if (want > gsg) want = gsg;
    if (want < 1) want = 1;
    uint64_t spr = (gsg + want - 1) / want;
    if (lim.max_sg != 0 && spr > lim.max_sg) spr = lim.max_sg;
    p.spr = spr;
    p.runs = (gsg + spr - 1) / spr;
    return p;
}

}  // namespace dpfh
