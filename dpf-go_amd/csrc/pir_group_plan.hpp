// pir_group_plan.hpp — grouped PIR: the layout rule of a grouped DB and the
// launch plan of the grouped fold (k_fold_grouped, pir_fold_grouped.hip).
// Host-only and header-only (no HIP), like pir_fold_plan.hpp, so
// tests/c/pir_group_plan_test.cpp runs it under ASan/UBSan without a device.
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
// Plan.  A workgroup ("unit") folds one run of whole super-groups of one
// column of one group for kp <= kGroupKeysPerPass keys of that group.  Units
// are numbered run-fastest, then column, then group (GroupedFoldPlan::unit),
// and a launch is a 1-D grid over a contiguous range of unit numbers: however
// many groups there are, no grid dimension sees more than `cap` workgroups.
// The keys of a group are taken in passes of 4, then 2, then 1 (one kernel
// instantiation each); every pass walks all units.
// What the plan guarantees, and no kernel can check:
//   - every (group, super-group, column, key) cell is folded exactly once;
//   - no run is empty and none crosses a group boundary (runs are cut inside
//     [0, gsg) of their group);
//   - a launch has at most lim.max_blocks workgroups when dpf_set_fold_limits
//     set fewer than its default, else at most kGroupMaxBlocks;
//   - the launches write no scratch: with one run per group (runs == 1) every
//     answer word has exactly one writer, which stores it; with more, the
//     answers are cleared by a zero-fill launch earlier in stream order and every
//     run XORs its words in with one vector atomic each (XOR is order-free,
//     so the answers are deterministic).  scratch_bytes() is therefore 0.
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
constexpr uint64_t kGroupMaxBlocks = 1ull << 20;   // workgroups per launch, the plan's own cap
constexpr uint32_t kGroupKeysPerPass = 4;          // widest k_fold_grouped<KP>
constexpr uint64_t kGroupPerCu = 8;                // workgroups per CU a pass aims at (k_fold_sliced_direct's)

// One launch: units [u0, u0 + blocks) for keys [k0, k0 + kp) of every group.
struct GroupLaunch {
    uint64_t u0, blocks;
    uint32_t k0, kp;
};
// What a unit folds: super-groups [s0, s1) (group-local) of column c of group g.
struct GroupUnit {
    uint64_t g, s0, s1;
    uint32_t c;
};

struct GroupedFoldPlan {
    uint64_t ngroups, gsg;
    uint32_t C, kpg;
    uint64_t runs, spr;   // runs per (group, column), super-groups per run (the last run what is left)
    uint64_t cap;         // workgroups per launch
    uint32_t kp_max;      // keys per pass, a power of two <= kGroupKeysPerPass

    uint64_t units() const { return ngroups * C * runs; }
    // More than one run per group: cleared answers and atomic XORs (above).
    bool atomic() const { return runs > 1; }
    size_t scratch_bytes() const { return 0; }
    GroupUnit unit(uint64_t u) const {
        const uint64_t r = u % runs, t = u / runs, s0 = r * spr;
        return {t / C, s0, s0 + spr < gsg ? s0 + spr : gsg, (uint32_t)(t % C)};
    }

    // fn(const GroupLaunch&) for every launch in stream order, until one
    // returns a nonzero (error) value, which is returned.
    template <class F>
    auto for_each_launch(F fn) const -> decltype(fn(GroupLaunch{})) {
        const uint64_t n = units();
        for (uint32_t k0 = 0; k0 < kpg;) {
            uint32_t kp = kp_max;
            while (kp > kpg - k0) kp /= 2;
            for (uint64_t u0 = 0; u0 < n; u0 += cap)
                if (auto e = fn(GroupLaunch{u0, n - u0 < cap ? n - u0 : cap, k0, kp}); e != decltype(e){}) return e;
            k0 += kp;
        }
        return {};
    }
};

// ngroups groups of gsg super-groups and C columns, kpg keys per group, on
// `cus` CUs.  Few large groups split into runs of whole pairs of super-groups
// until a pass has about cus * kGroupPerCu workgroups (plan_fold_sliced_direct's
// aim for its one DB); from ngroups * C workgroups upwards a group is one run.
// kp_max: the widest key pass (measurement knob; 0 or more than
// kGroupKeysPerPass: that).
inline GroupedFoldPlan plan_fold_grouped(uint64_t ngroups, uint64_t gsg, uint32_t C, uint32_t kpg, uint64_t cus,
                                         FoldLimits lim, uint32_t kp_max = 0) {
    const uint64_t cells = ngroups * C, aim = (cus ? cus : 1) * kGroupPerCu;
    uint64_t want = cells ? (aim + cells - 1) / cells : 1;
    if (want > gsg) want = gsg;
    if (want < 1) want = 1;
    const ChunkSplit s = gsg ? split_chunks(gsg, want, 2, gsg) : ChunkSplit{0, 1};
    const uint64_t cap = lim.max_blocks != 0 && lim.max_blocks < kFoldMaxBlocks ? lim.max_blocks : kGroupMaxBlocks;
    const uint32_t kp = kp_max >= 4 || kp_max == 0 ? 4u : kp_max >= 2 ? 2u : 1u;
    return {ngroups, gsg, C, kpg, s.blocks, s.cpb, cap, kp};
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
