// pir_group_fold_plan.hpp — the grouped fold for any number of keys per group:
// its route rule and the launch plan of the matrix-core grouped fold
// (k_fold_grouped_mfma, pir_fold_grouped_mfma.hip) beside pir_group_plan.hpp's
// plan of the popcount one (k_fold_grouped).  Host-only and header-only (no
// HIP), so tests/c/pir_group_fold_plan_test.cpp runs it under ASan/UBSan
// without a device.
//
// Routes.  k_fold_grouped takes the keys of a group four at a time, a pass
// over the whole DB each (the direct route: plan_fold_grouped's GroupedPlan,
// unchanged).  k_fold_grouped_mfma folds up to 256 keys of every group in one
// pass over the group's tiles (the matrix-core route), so kpg keys are
// ceil(kpg / 256) passes.
//
// Plan of the matrix-core route.  The keys of a group are cut into key tiles
// of kFoldKeyGroup = 256; the last tile takes the smallest shape of
// dpfh::kFoldTiles that holds what is left (fold_tile_index), every tile the
// columns per workgroup of its shape (CG, from fold_cg).  A key tile is one
// pass: its units are numbered run-fastest, then column group, then group and
// decoded by group_unit with ncg = C / CG in the place of the columns, and a
// launch is a 1-D grid over a contiguous range of unit numbers of at most
// `cap` workgroups.  Runs are whole multiples of the shape's SG super-groups
// (the staged block), never longer than lim.max_sg (clamp_fold_limits: at most
// kFoldMaxSg, below which the fp32 counts are exact); where max_sg is below SG
// a run is max_sg super-groups, a partial staged block, which the kernel folds
// like the ragged end of any run.  Few large groups are cut into more runs
// until a pass fills the resident workgroups of the chip (group_fold_want_runs
// below), as plan_fold_mfma aims.
// What a plan guarantees, and no kernel can check:
//   - every (group, super-group, column, key) cell is folded exactly once;
//   - no run is empty and none crosses a group boundary;
//   - a key tile holds keys of one group only, at most 32 MT of its shape, and
//     the tiles' widths sum to kpg;
//   - a launch has at most `cap` workgroups (grouped_plan_shape's rule);
//   - a pass with one run per (group, column group) has one writer per answer
//     word, which stores it; if any pass has more, atomic() is set: the
//     launcher clears all answers first and the runs of such a pass XOR their
//     words in with vector atomics (k_fold_grouped's contract);
//   - no scratch: neither partials nor a combining launch.
//
// The route rule is a function of (ngroups, gsg, C, kpg) alone (fold_route
// below).  kpg <= 4 is one direct pass at the speed of the DB stream, fixed in
// advance to stay direct.  From 5 keys the direct route is two passes or more
// against one matrix-core pass, so the rule takes the matrix-core route from
// kGroupFoldMfmaMinKeys = 5 keys per group at every shape.  Measured on one
// MI355X (tools/grouped_pir_keys_ab.py, profiles/grouped_pir_mfma/; DESIGN.md
// §4.4 "Many keys per group"), fold alone, matrix-core against direct, µs:
//   96 x 2^19 x 32 B     kpg 5: 286 / 575   8: 286 / 599   16: 297 / 1178
//                        64: 400 / 4699   256: 1194 / 18612
//   384 x 2^17 x 32 B    kpg 5: 294 / 575   16: 301 / 1150   256: 1199 / 18489
//   96 x 2^16 x 256 B    kpg 8: 283 / 613   64: 382 / 4791
//   4096 x 2^12 x 32 B   kpg 8: 97 / 196    64: 171 / 1840
// The matrix-core route was ahead in 6 of 6 pairs at every measured shape and
// key count, kpg = 4 included (287 against 304 at 96 groups, 93 against 97 at
// 4096): the two routes do not cross above 4 keys, so the crossover is the step
// from one direct pass to two and does not move with the shape.  The recorded routes (direct at 4, matrix-core from 5, at all four
// shapes) are pinned in tests/c/pir_group_fold_plan_test.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pir_group_plan.hpp"

namespace dpfh {

enum GroupFoldRoute : uint32_t { kFoldRouteDirect = 0, kFoldRouteMfma = 1 };
constexpr uint32_t kGroupFoldMfmaMinKeys = 5;   // keys per group from which the matrix-core route is taken

inline GroupFoldRoute fold_route(uint64_t ngroups, uint64_t gsg, uint32_t C, uint32_t kpg) {
    (void)ngroups, (void)gsg, (void)C;          // the crossover did not move with the shape (header comment)
    return kpg >= kGroupFoldMfmaMinKeys ? kFoldRouteMfma : kFoldRouteDirect;
}

// Workgroups of tile shape t resident on a CU: a workgroup is 4 CG waves, one
// CG-th of them on each SIMD, and the shape is compiled for WPE waves a SIMD.
constexpr uint64_t fold_tile_per_cu(const FoldTile& t) { return t.WPE / t.CG > 0 ? (uint64_t)(t.WPE / t.CG) : 1; }

// Runs per (group, column group) so that a pass of cells * runs workgroups
// fills whole rounds of `aim` resident ones: the r from aim / cells upwards
// (a few candidates) with the largest cells * r / (ceil(cells * r / aim) * aim),
// the smallest such r.  96 cells on 256: 8 runs, 768 workgroups in 3 full
// rounds, where 3 runs would leave 32 workgroups for a second round as long as
// the first.  Cells for two rounds or more: one run (no clear, no atomics).
inline uint64_t group_fold_want_runs(uint64_t cells, uint64_t aim) {
    if (cells == 0 || cells / 2 >= aim) return 1;
    const uint64_t lo = aim > cells ? aim / cells : 1, span = 3 * lo + 4 < 64 ? 3 * lo + 4 : 64;
    uint64_t best = lo, bn = 0, bd = 1;
    for (uint64_t r = lo; r <= lo + span; ++r) {
        const uint64_t n = cells * r, d = (n + aim - 1) / aim * aim;
        if (n * bd > bn * d) best = r, bn = n, bd = d;
        if (n == d) break;
    }
    return best;
}

// One key tile of the matrix-core route: keys [k0, k0 + kp) of every group with
// tile shape kFoldTiles[shape], cg columns per workgroup in ncg column groups,
// `runs` runs of spr super-groups (the last what is left of gsg).
struct GroupFoldPass {
    uint32_t k0 = 0, kp = 0;
    int shape = 0;
    uint32_t cg = 1, ncg = 1;
    uint64_t runs = 1, spr = 1;
};
// One launch: units [u0, u0 + blocks) of key tile `pass`.
struct GroupFoldLaunch {
    uint64_t u0, blocks;
    GroupFoldPass pass;
};

inline GroupFoldPass group_fold_pass(uint64_t ngroups, uint64_t gsg, uint32_t C, uint32_t k0, uint32_t kp, uint64_t cus,
                                     FoldLimits lim) {
    GroupFoldPass p;
    p.k0 = k0, p.kp = kp;
    p.shape = fold_tile_index(kp, fold_cg(C, FoldKnobs{}.wide_cg));
    const FoldTile& t = kFoldTiles[p.shape];
    p.cg = (uint32_t)t.CG, p.ncg = C / (uint32_t)t.CG;
    if (gsg == 0) return p;
    const uint64_t sg = (uint64_t)t.SG;
    const uint64_t lim_sg = lim.max_sg != 0 && lim.max_sg < kFoldMaxSg ? lim.max_sg : kFoldMaxSg;
    const uint64_t msg = lim_sg >= sg ? lim_sg / sg * sg : lim_sg;
    const uint64_t staged = (gsg + sg - 1) / sg;
    uint64_t want = group_fold_want_runs(ngroups * p.ncg, (cus ? cus : 1) * fold_tile_per_cu(t));
    if (want > staged) want = staged;
    uint64_t spr = ((gsg + want - 1) / want + sg - 1) / sg * sg;
    if (spr > msg) spr = msg;
    p.spr = spr, p.runs = (gsg + spr - 1) / spr;
    return p;
}

struct GroupFoldKeysPlan {
    GroupFoldRoute route = kFoldRouteDirect;
    GroupedPlan direct;            // the direct route's plan (plan_fold_grouped's, whatever the route)
    uint64_t ngroups = 0, gsg = 0;
    uint32_t C = 0, kpg = 0;
    uint64_t cap = 1;              // workgroups per launch
    uint32_t nfull = 0;            // key tiles of kFoldKeyGroup keys
    GroupFoldPass full, last;      // the shape of those, and the tile of the keys left (last.kp == 0: none)

    uint32_t tiles() const { return nfull + (last.kp != 0); }
    GroupFoldPass tile(uint32_t i) const {
        GroupFoldPass p = i < nfull ? full : last;
        if (i < nfull) p.k0 = i * kFoldKeyGroup;
        return p;
    }
    uint64_t units(const GroupFoldPass& p) const { return kpg == 0 || gsg == 0 ? 0 : ngroups * p.ncg * p.runs; }
    GroupUnit unit(const GroupFoldPass& p, uint64_t u) const { return group_unit(u, p.runs, p.spr, gsg, p.ncg); }
    // Some pass has several runs per (group, column group): cleared answers, atomic XORs there.
    bool atomic() const {
        if (route == kFoldRouteDirect) return direct.atomic();
        return (nfull != 0 && full.runs > 1) || (last.kp != 0 && last.runs > 1);
    }
    size_t scratch_bytes() const { return 0; }

    // fn(const GroupFoldLaunch&) for every launch of the matrix-core route in
    // stream order, until one returns a nonzero (error) value, which is returned.
    template <class F>
    auto for_each_launch(F fn) const -> decltype(fn(GroupFoldLaunch{})) {
        for (uint32_t i = 0; i < tiles(); ++i) {
            const GroupFoldPass p = tile(i);
            const uint64_t n = units(p);
            for (uint64_t u0 = 0; u0 < n; u0 += cap)
                if (auto e = fn(GroupFoldLaunch{u0, n - u0 < cap ? n - u0 : cap, p}); e != decltype(e){}) return e;
        }
        return {};
    }
};

// The grouped fold of ngroups groups of gsg super-groups and C columns, kpg
// keys per group, on `cus` CUs.  route_knob: kFoldRouteDirect or kFoldRouteMfma
// forces that route (measurement), anything else leaves it to fold_route.
// kp_max: plan_fold_grouped's, for the direct route.
inline GroupFoldKeysPlan plan_fold_grouped_keys(uint64_t ngroups, uint64_t gsg, uint32_t C, uint32_t kpg, uint64_t cus,
                                                FoldLimits lim, int route_knob = -1, uint32_t kp_max = 0) {
    GroupFoldKeysPlan p;
    p.direct = plan_fold_grouped(ngroups, gsg, C, kpg, cus, lim, kp_max);
    p.route = route_knob == (int)kFoldRouteDirect || route_knob == (int)kFoldRouteMfma ? (GroupFoldRoute)route_knob
                                                                                       : fold_route(ngroups, gsg, C, kpg);
    p.ngroups = ngroups, p.gsg = gsg, p.C = C, p.kpg = kpg, p.cap = p.direct.cap;
    p.nfull = kpg / kFoldKeyGroup;
    if (p.nfull) p.full = group_fold_pass(ngroups, gsg, C, 0, kFoldKeyGroup, cus, lim);
    if (const uint32_t rest = kpg % kFoldKeyGroup)
        p.last = group_fold_pass(ngroups, gsg, C, p.nfull * kFoldKeyGroup, rest, cus, lim);
    return p;
}

}  // namespace dpfh
