// pir_group_plan.hpp — grouped PIR: the layout rule of a grouped DB and the
// launch plan of the grouped kernels (k_fold_grouped, pir_fold_grouped.hip;
// k_scatter_grouped, pir_scatter_grouped.hip).
// Header-only and plain C++ (no HIP), like pir_fold_plan.hpp, so
// tests/c/pir_group_plan_test.cpp runs it under ASan/UBSan without a device;
// under hipcc group_unit is device code as well.
//
// Layout.  A grouped DB is ngroups groups of nrec records, all of one shape.
// On the device it is the any-width sliced layout of ONE flat DB in which
// group g, record i sits at flat position g * gs + i, gs = group_stride(nrec)
// = nrec rounded up to whole super-groups of 256 records; flat positions
// [nrec, gs) of every group are zero records, which select nothing.  So a
// group is gsg = gs / 256 whole super-groups starting at byte g * gs *
// rec_bytes, and the slice / update / gather / scatter launchers work on it
// by flat position.
//
// Plan.  A workgroup ("unit") works on one run of whole super-groups of one
// 32-byte column of one group for kp <= kGroupKeysPerPass keys of that group:
// the fold XORs the selected words into the keys' answers, the scatter XORs the
// keys' messages into the selected words.  Units are numbered run-fastest, then
// column, then group (group_unit, the one decode of host and device), and a
// launch is a 1-D grid over a contiguous range of unit numbers: however many
// groups there are, no grid dimension sees more than `cap` workgroups, and few
// large groups are cut into runs inside [0, gsg) of their group.  The keys of
// a group are taken in passes (one kernel instantiation per width) in stream
// order; every pass walks all units.  The fold and the scatter share this
// GroupedPlan and differ in three rules, which are their builders'
// (plan_fold_grouped here, plan_scatter_grouped in pir_group_scatter_plan.hpp):
// how a group is cut into runs, the pass widths, and the route.
// What a plan guarantees, and no kernel can check:
//   - every (group, super-group, column, key) cell is worked on exactly once;
//   - no run is empty and none crosses a group boundary;
//   - the units of a pass are distinct (group, column, run) triples;
//   - a launch has at most lim.max_blocks workgroups when dpf_set_fold_limits
//     set fewer than its default, else at most kGroupMaxBlocks;
//   - the launches write no scratch: scratch_bytes() is 0.
//   Fold only: with one run per group (runs == 1) every answer word has
//     exactly one writer, which stores it; with more, the answers are cleared
//     by a zero-fill launch earlier in stream order and every run XORs its
//     words in with one vector atomic each (XOR is order-free, so the answers
//     are deterministic): atomic().
//   Scatter only: no run is longer than dpf_set_fold_limits' max_sg; within one
//     launch (and within one pass) no two workgroups touch the same tile, and a
//     pass reads and writes a tile at most once: no atomics; the pass widths
//     sum to kpg.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pir_fold_plan.hpp"
#include "pir_update_plan.hpp"

namespace dpfh {

// ---- the layout rule ---------------------------------------------------------
inline uint64_t group_stride(uint64_t nrec) { return (nrec + 255) / 256 * 256; }
// Flat position of caller index idx = g * nrec + i (nrec > 0).
inline uint64_t group_flat(uint64_t idx, uint64_t nrec) { return idx / nrec * group_stride(nrec) + idx % nrec; }
// Bytes of the grouped layout into *out; false where the product does not fit 64 bits.
inline bool grouped_bytes(uint64_t ngroups, uint64_t nrec, uint64_t rec_bytes, uint64_t* out) {
    if (nrec > UINT64_MAX - 255) return false;
    const uint64_t gs = group_stride(nrec);
    if (gs != 0 && ngroups > UINT64_MAX / gs) return false;
    if (rec_bytes != 0 && ngroups * gs > UINT64_MAX / rec_bytes) return false;
    *out = ngroups * gs * rec_bytes;
    return true;
}

// ---- the launch plan ---------------------------------------------------------
#ifndef DPF_HD
#if defined(__HIPCC__)
#define DPF_HD __host__ __device__
#else
#define DPF_HD
#endif
#endif

constexpr uint64_t kGroupMaxBlocks = 1ull << 20;   // workgroups per launch, the plan's own cap
constexpr uint32_t kGroupKeysPerPass = 4;          // widest k_fold_grouped<KP> and k_scatter_grouped<KP>
constexpr uint64_t kGroupPerCu = 8;                // workgroups per CU a pass aims at (k_fold_sliced_direct's)

// How the grouped write runs (scatter_route, pir_group_scatter_plan.hpp); a fold is always grouped.
enum GroupScatterRoute : uint32_t { kScatterRouteGrouped = 0, kScatterRouteLoop = 1 };

// One launch: units [u0, u0 + blocks) for keys [k0, k0 + kp) of every group.
struct GroupLaunch {
    uint64_t u0, blocks;
    uint32_t k0, kp;
};
// What a unit works on: super-groups [s0, s1) (group-local) of column c of group g.
struct GroupUnit {
    uint64_t g, s0, s1;
    uint32_t c;
};
// Unit u of a plan with `runs` runs of spr super-groups (the last what is left
// of gsg) per (group, column) and C columns, on the host and in the kernels.
DPF_HD inline GroupUnit group_unit(uint64_t u, uint64_t runs, uint64_t spr, uint64_t gsg, uint32_t C) {
    const uint64_t r = u % runs, t = u / runs, g = t / C;
    const uint32_t c = (uint32_t)(t % C);
    const uint64_t s0 = r * spr;
    return {g, s0, s0 + spr < gsg ? s0 + spr : gsg, c};
}

struct GroupedPlan {
    uint64_t ngroups = 0, gsg = 0;
    uint32_t C = 0, kpg = 0;
    uint64_t runs = 1, spr = 1;   // runs per (group, column), super-groups per run (the last run what is left)
    uint64_t cap = 1;             // workgroups per launch
    uint32_t kp_max = kGroupKeysPerPass;   // widest key pass, a power of two
    bool halve = false;   // fewer than kp_max keys left: widths halved until they fit (fold), else one pass of them (scatter)
    GroupScatterRoute route = kScatterRouteGrouped;

    uint64_t units() const { return kpg == 0 || gsg == 0 ? 0 : ngroups * C * runs; }
    uint32_t pass_width(uint32_t left) const {
        uint32_t kp = kp_max;
        if (!halve) return left < kp ? left : kp;
        while (kp > left) kp /= 2;
        return kp;
    }
    uint64_t passes() const {
        const uint32_t rest = kpg % kp_max;
        return units() ? kpg / kp_max + (halve ? (uint64_t)__builtin_popcount(rest) : rest != 0) : 0;
    }
    GroupUnit unit(uint64_t u) const { return group_unit(u, runs, spr, gsg, C); }
    // Fold: more than one run per group, so cleared answers and atomic XORs (above).
    bool atomic() const { return runs > 1; }
    size_t scratch_bytes() const { return 0; }

    // fn(const GroupLaunch&) for every launch of the grouped route in stream
    // order, until one returns a nonzero (error) value, which is returned.
    template <class F>
    auto for_each_launch(F fn) const -> decltype(fn(GroupLaunch{})) {
        const uint64_t n = units();
        if (n == 0) return {};
        for (uint32_t k0 = 0; k0 < kpg;) {
            const uint32_t kp = pass_width(kpg - k0);
            for (uint64_t u0 = 0; u0 < n; u0 += cap)
                if (auto e = fn(GroupLaunch{u0, n - u0 < cap ? n - u0 : cap, k0, kp}); e != decltype(e){}) return e;
            k0 += kp;
        }
        return {};
    }
};

// What both builders start from: the shape and the workgroup cap (lim: clamp_fold_limits').
inline GroupedPlan grouped_plan_shape(uint64_t ngroups, uint64_t gsg, uint32_t C, uint32_t kpg, FoldLimits lim) {
    GroupedPlan p;
    p.ngroups = ngroups, p.gsg = gsg, p.C = C, p.kpg = kpg;
    p.cap = lim.max_blocks != 0 && lim.max_blocks < kFoldMaxBlocks ? lim.max_blocks : kGroupMaxBlocks;
    return p;
}
// The runs per (group, column) a builder aims at (gsg > 0): few large groups
// split until a pass has about cus * kGroupPerCu workgroups
// (plan_fold_sliced_direct's aim); from that many (group, column) pairs, one run.
inline uint64_t grouped_want_runs(uint64_t ngroups, uint64_t gsg, uint32_t C, uint64_t cus) {
    const uint64_t cells = ngroups * C, aim = (cus ? cus : 1) * kGroupPerCu;
    const uint64_t want = cells ? (aim + cells - 1) / cells : 1;
    return want > gsg ? gsg : want;
}

// The grouped fold of ngroups groups of gsg super-groups and C columns, kpg
// keys per group, on `cus` CUs.  Runs are whole pairs of super-groups
// (lim.max_sg does not apply); the passes are 4, then 2, then 1 keys wide.
// kp_max: the widest key pass (measurement knob; 0 or more than
// kGroupKeysPerPass: that).
inline GroupedPlan plan_fold_grouped(uint64_t ngroups, uint64_t gsg, uint32_t C, uint32_t kpg, uint64_t cus,
                                     FoldLimits lim, uint32_t kp_max = 0) {
    GroupedPlan p = grouped_plan_shape(ngroups, gsg, C, kpg, lim);
    p.halve = true;
    p.kp_max = kp_max >= 4 || kp_max == 0 ? 4u : kp_max >= 2 ? 2u : 1u;
    if (gsg == 0) return p;
    const ChunkSplit s = split_chunks(gsg, grouped_want_runs(ngroups, gsg, C, cus), 2, gsg);
    p.runs = s.blocks, p.spr = s.cpb;
    return p;
}

// ---- the handle's shards and its update split ----------------------------------
// Shard s of a grouped handle holds the groups [s * gps, (s + 1) * gps) cut at
// ngroups, gps = ceil(ngroups / nshards): as a range of flat positions.
inline uint64_t groups_per_shard(uint64_t ngroups, size_t nshards) {
    return (ngroups + (uint64_t)nshards - 1) / (uint64_t)nshards;
}
inline ShardRanges grouped_shards(uint64_t ngroups, uint64_t nrec, size_t nshards) {
    const uint64_t gs = group_stride(nrec);
    return ShardRanges{ngroups * gs, groups_per_shard(ngroups, nshards) * gs};
}
// plan_pir_update for a grouped handle: caller index idx = g * nrec + i
// (< ngroups * nrec) goes to the shard that holds flat position
// group_flat(idx, nrec), at that position less the shard's first.
inline bool plan_pir_update_grouped(const uint64_t* idx, size_t n, uint64_t ngroups, uint64_t nrec, size_t nshards,
                                    bool keep_last, PirUpdatePlan* plan) {
    const uint64_t slice = grouped_shards(ngroups, nrec, nshards).slice;
    return plan_pir_update_split(idx, n, ngroups * nrec, nshards, keep_last,
                                 [=](uint64_t v, size_t* shard, uint64_t* local) {
                                     const uint64_t f = group_flat(v, nrec);
                                     *shard = (size_t)(f / slice);
                                     *local = f % slice;
                                 },
                                 plan);
}

}  // namespace dpfh
